"""gesummv parity on the GPU.

Contract: bit-exact vs the oracle's restatement of the row-streamed fold of
examples/kernels/gesummv_rank0.cl:53-203 (our build's order; the emulator's
FP contraction is not knowable here), and accepted by the reference host's
own check (rel. err < 1e-4, examples/host/gesummv_smi.cpp:40-46,299-313).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# m spans: one chunk, odd chunk counts (a lone last tile), slab (64-chunk)
# boundaries +-1, several full slabs
@pytest.mark.parametrize("shape", [(1, 64), (5, 128), (17, 192), (128, 1024), (64, 4096), (3, 33 * 64),
                                   (7, 65 * 64), (9, 127 * 64), (4, 129 * 64), (6, 3 * 64 * 64)])
def test_gemv_rows_matches_oracle(gpu, oracle_mod, shape):
    from smi_amd import gesummv
    n, m = shape
    rng = np.random.default_rng(n * m)
    A = (rng.random((n, m), dtype=np.float32) * 2 - 1)
    B = (rng.random((n, m), dtype=np.float32) * 2 - 1)
    x = (rng.random(m, dtype=np.float32) * 2 - 1)
    want = oracle_mod.gesummv(A, B, x, 1.5, 0.5)
    got = gesummv.gemv_rows(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(),
                            torch.from_numpy(x).cuda(), 1.5, 0.5).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_gemv_rows_strided_and_single_matrix(gpu, oracle_mod):
    """lda > m (a column window of a wider matrix) and the A-only form
    (rank 0 of the reference with beta = 0, gesummv_smi.cpp:224)."""
    from smi_amd import gesummv
    n, m, lda = 13, 130 * 64, 130 * 64 + 4
    rng = np.random.default_rng(5)
    W = rng.random((n, lda), dtype=np.float32) * 2 - 1
    x = rng.random(m, dtype=np.float32) * 2 - 1
    A = torch.from_numpy(W).cuda()[:, :m]
    got = gesummv.gemv_rows(A, A, torch.from_numpy(x).cuda(), 1.25, -0.75).cpu().numpy()
    want = oracle_mod.gesummv(W[:, :m], W[:, :m], x, 1.25, -0.75)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got1 = gesummv.gemv_rows(A, None, torch.from_numpy(x).cuda(), 1.25, 0.0).cpu().numpy()
    want1 = oracle_mod.gesummv(W[:, :m], np.zeros((n, m), np.float32), x, 1.25, 0.0)
    assert np.array_equal(got1, want1)


def same_bits(a, b):
    """NaN positions match and every other element matches bitwise."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def _uniform(rng, *shape):
    return rng.random(shape, dtype=np.float32) * 2 - 1


# Rows longer than 32768 columns leave the row-split kernel for the
# one-wave-per-row kernel: 513 chunks (8 slabs + 1 chunk, odd; n % 4 = 1 leaves
# three waves of the workgroup without a row), a full workgroup, a single row,
# 577 chunks (one chunk in the last slab), 1026 chunks (two chunks = one tile in
# the last slab), whole slabs only.
LONG_ROW_SHAPES = [(5, 32832), (4, 32832), (1, 32832), (3, 36928), (2, 65664), (6, 32768 + 64 * 64)]


@pytest.mark.parametrize("shape", LONG_ROW_SHAPES)
def test_gemv_long_rows_match_oracle(gpu, oracle_mod, shape):
    from smi_amd import gesummv
    n, m = shape
    rng = np.random.default_rng(n * m)
    A, B, x = _uniform(rng, n, m), _uniform(rng, n, m), _uniform(rng, m)
    want = oracle_mod.gesummv(A, B, x, 1.5, 0.5)
    got = gesummv.gemv_rows(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(),
                            torch.from_numpy(x).cuda(), 1.5, 0.5).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_gemv_long_rows_strided_and_single_matrix(gpu, oracle_mod):
    """The long-row kernel on a column window (lda = m + 4), as A is B and
    as the A-only form."""
    from smi_amd import gesummv
    n, m, lda = 5, 32832, 32832 + 4
    rng = np.random.default_rng(6)
    W = _uniform(rng, n, lda)
    x = _uniform(rng, m)
    A = torch.from_numpy(W).cuda()[:, :m]
    assert A.stride(0) == lda
    got = gesummv.gemv_rows(A, A, torch.from_numpy(x).cuda(), 1.25, -0.75).cpu().numpy()
    want = oracle_mod.gesummv(W[:, :m], W[:, :m], x, 1.25, -0.75)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got1 = gesummv.gemv_rows(A, None, torch.from_numpy(x).cuda(), 1.25, 0.0).cpu().numpy()
    want1 = oracle_mod.gesummv(W[:, :m], np.zeros((n, m), np.float32), x, 1.25, 0.0)
    assert np.array_equal(got1.view(np.uint32), want1.view(np.uint32))


def test_gemv_long_row_and_split_kernels_agree_at_the_seam(gpu, oracle_mod):
    """The two kernels claim the same tile values and fold order.  With the
    last 64 entries of x at +0 the 513th chunk's c is +0 and its tile adds +0,
    so 32832 columns on the long-row kernel and the first 32768 of the same
    storage on the row-split kernel (strided views) must give the same bits,
    and both the oracle's."""
    from smi_amd import gesummv
    n, m, ms = 4, 32832, 32768
    rng = np.random.default_rng(7)
    A, B, x = _uniform(rng, n, m), _uniform(rng, n, m), _uniform(rng, m)
    x[ms:] = 0.0
    dA, dB, dx = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(x).cuda()
    long_rows = gesummv.gemv_rows(dA, dB, dx, 1.5, -0.5).cpu().numpy()
    vA, vB = dA[:, :ms], dB[:, :ms]
    assert vA.stride(0) == m and vA.data_ptr() == dA.data_ptr()
    split = gesummv.gemv_rows(vA, vB, dx[:ms], 1.5, -0.5).cpu().numpy()
    want = oracle_mod.gesummv(A, B, x, 1.5, -0.5)
    assert np.array_equal(long_rows.view(np.uint32), split.view(np.uint32))
    assert np.array_equal(long_rows.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want.view(np.uint32),
                          oracle_mod.gesummv(A[:, :ms], B[:, :ms], x[:ms], 1.5, -0.5).view(np.uint32))


@pytest.mark.parametrize("shape", [(5, 32832), (2, 65664)])
def test_gemv_long_rows_within_summation_bound(gpu, shape):
    """A backstop that does not depend on the oracle's order: any summation
    order of m fp32 products, scaled and added, stays within
    (m + 2) * 2^-24 * (|alpha| |A| |x| + |beta| |B| |x|) of the float64 value,
    row by row.  The oracle sits about 10^6 times below the bound; it is a
    worst-case bound, so it catches errors of the size of the row's terms
    (a wrong alpha, rows or slabs mixed up), not one lost 64-column chunk of
    uniform data, which changes a row by 0.002 to 0.15 of the bound here --
    that is what the bitwise comparisons above are for."""
    from smi_amd import gesummv
    n, m = shape
    alpha, beta = 1.5, 0.5
    rng = np.random.default_rng(n + m)
    A, B, x = _uniform(rng, n, m), _uniform(rng, n, m), _uniform(rng, m)
    got = gesummv.gemv_rows(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(),
                            torch.from_numpy(x).cuda(), alpha, beta).cpu().numpy()
    A64, B64, x64 = A.astype(np.float64), B.astype(np.float64), x.astype(np.float64)
    y64 = alpha * (A64 @ x64) + beta * (B64 @ x64)
    bound = (m + 2) * 2.0 ** -24 * (abs(alpha) * (np.abs(A64) @ np.abs(x64)) + abs(beta) * (np.abs(B64) @ np.abs(x64)))
    err = np.abs(got.astype(np.float64) - y64)
    print(f"gemv long rows {shape}: max err / bound = {float(np.max(err / bound)):.3e}")
    assert np.all(err <= bound), (err, bound)


def special_value_case(m, seed=1):
    """Eight rows, uniform in [-1, 1] except for the special values, which sit
    in the last 64-column chunk (at m = 32832 that is the last slab of the
    long-row kernel), and an x whose first chunk is scaled into the range
    where the products of rows 4 and 6 are subnormal."""
    rng = np.random.default_rng(seed)
    W = _uniform(rng, 8, m)
    x = _uniform(rng, m)
    c0 = m - 64
    W[1, c0 + 7] = np.inf
    W[2, c0 + 11] = np.nan
    W[3, :] = 0.0
    W[3, c0 + 13] = -0.0
    W[4, :] = 1e-30
    W[5, c0 + 20] = -np.inf
    W[5, c0 + 21] = np.inf
    W[6, :] *= np.float32(1e-38)
    x[:64] *= np.float32(1e-10)
    return W, x


@pytest.mark.parametrize("m", [192, 32832])
def test_gemv_special_values(gpu, oracle_mod, m):
    """Inf, NaN, signed zeros and subnormals through both kernels (m = 192:
    row split; m = 32832: one wave per row), alpha = -1.25, beta = 0.75,
    A is B.  Row 1 turns Inf - Inf into NaN only at the final A + B add."""
    from smi_amd import gesummv
    alpha, beta = -1.25, 0.75
    W, x = special_value_case(m)
    want = oracle_mod.gesummv(W, W, x, alpha, beta)
    # the case is what it claims to be, on the oracle alone
    assert np.flatnonzero(np.isnan(want)).tolist() == [1, 2, 5]
    assert np.isfinite(want[[4, 6]]).all() and (want[[4, 6]] != 0).all()
    tiny = float(np.finfo(np.float32).tiny)
    for r in (4, 6):  # fp32 products that are subnormal and not zero: flushing them changes the row
        p = np.abs(W[r] * x)
        assert ((p > 0) & (p < tiny)).sum() >= 32
    assert want[3:4].view(np.uint32)[0] == 0
    dW = torch.from_numpy(W).cuda()
    got = gesummv.gemv_rows(dW, dW, torch.from_numpy(x).cuda(), alpha, beta).cpu().numpy()
    assert same_bits(got, want), (got, want)


def test_reference_pattern(gpu, oracle_mod):
    from smi_amd import gesummv
    n, m = 256, 512
    A = gesummv.reference_matrix(n, m)
    x = gesummv.reference_vector(m)
    got = gesummv.gemv_rows(torch.from_numpy(A).cuda(), torch.from_numpy(A).cuda(),
                            torch.from_numpy(x).cuda(), 2.0, 3.0).cpu().numpy()
    assert oracle_mod.gesummv_reference_check(got, A, A, x, 2.0, 3.0)
    assert np.array_equal(got, oracle_mod.gesummv(A, A, x, 2.0, 3.0))


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_distributed_gesummv(gpu, oracle_mod, nranks):
    from smi_amd import LocalGroup, gesummv
    n, m = 203, 640
    rng = np.random.default_rng(nranks)
    A = rng.random((n, m), dtype=np.float32)
    B = rng.random((n, m), dtype=np.float32)
    x = rng.random(m, dtype=np.float32)
    root = nranks - 1

    def fn(comm):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            r0, r1 = gesummv.row_range(n, comm.size, comm.rank)
            y = gesummv.gesummv(comm, torch.from_numpy(A[r0:r1].copy()).cuda(),
                                torch.from_numpy(B[r0:r1].copy()).cuda(), torch.from_numpy(x).cuda(),
                                n, 1.5, 0.5, root=root)
            s.synchronize()
            return None if y is None else y.cpu().numpy()

    got = LocalGroup(nranks).run(fn)[root]
    want = oracle_mod.gesummv(A, B, x, 1.5, 0.5)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
