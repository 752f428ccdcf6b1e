"""smi_kmeans_means (the fold of all ranks' sums and counts plus the divide,
one kernel) and smi_kmeans under set_means(1) (one record exchange per
iteration) on the GPU.

Contract: centroid = fold(sums column) / (float)fold(counts column) with the
canonical rank-order SMI_ADD folds of the reduce (4 slots fp32, 1 slot int32,
which wraps) and IEEE division -- bit for bit the oracle's reduce and numpy's
float32 division, NaN payloads aside; set_means(1) gives mode 0's centroids.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOAT, INT, ADD = 2, 1, 0


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def want_means(oracle_mod, sums, counts):
    """sums (nranks, clusters, dims) fp32, counts (nranks, clusters) int32."""
    n, k, d = sums.shape
    s = oracle_mod.reduce(sums.reshape(n, k * d), FLOAT, ADD).reshape(k, d)
    c = oracle_mod.reduce(counts, INT, ADD)
    with np.errstate(all="ignore"):
        return s / c.astype(np.float32)[:, None]


@pytest.mark.parametrize("nranks", [1, 2, 3, 4, 8, 9, 17, 64])
def test_means_matches_numpy(gpu, oracle_mod, nranks):
    """Partial batches of 8 rows (1..4, 9, 17) and whole ones (8, 64); the
    vector path (dims % 4 == 0) and the scalar one ((1, 1))."""
    from smi_amd import kmeans
    for clusters, dims in ((8, 64), (5, 48), (1, 1), (256, 8)):
        rng = np.random.default_rng(nranks * 1000 + clusters)
        sums = (rng.standard_normal((nranks, clusters, dims)) * 100).astype(np.float32)
        counts = rng.integers(0, 5000, (nranks, clusters)).astype(np.int32)
        counts[:, 0] += 1
        want = want_means(oracle_mod, sums, counts)
        got = kmeans.means(dev(sums), dev(counts)).cpu().numpy()
        assert got.shape == (clusters, dims)
        assert same_bits(got, want), (nranks, clusters, dims)


@pytest.mark.parametrize("nranks", [1, 3, 9])
def test_means_special_values(gpu, oracle_mod, nranks):
    from smi_amd import kmeans
    clusters, dims = 6, 8
    rng = np.random.default_rng(nranks)
    sums = rng.standard_normal((nranks, clusters, dims)).astype(np.float32)
    counts = rng.integers(1, 100, (nranks, clusters)).astype(np.int32)
    counts[:, 0] = 0
    sums[:, 0] = 0.0                       # empty on every rank: 0/0 = NaN
    counts[:, 1] = 0
    sums[:, 1] = 0.0
    sums[0, 1, :4] = 3.0                   # count 0, sum != 0: +inf / -inf
    sums[0, 1, 4:] = -3.0
    sums[:, 2] = -0.0                      # -0 on every rank: +0 through the +0 start
    if nranks > 1:
        counts[:, 3] = 0x7fffffff // nranks + 12345   # the int fold wraps past 2^31
    else:
        counts[0, 3] = -7                  # a negative count divides as it is
    want = want_means(oracle_mod, sums, counts)
    got = kmeans.means(dev(sums), dev(counts)).cpu().numpy()
    assert same_bits(got, want)
    assert np.isnan(got[0]).all()
    assert (got[1, :4] == np.inf).all() and (got[1, 4:] == -np.inf).all()
    assert (got[2].view(np.uint32) == 0).all()
    total = int(counts[:, 3].astype(np.int64).sum())
    wrapped = (total + 2**31) % 2**32 - 2**31
    if nranks > 1:
        assert wrapped != total and wrapped < 0
    with np.errstate(all="ignore"):
        assert same_bits(got[3], want_means(oracle_mod, sums, counts)[3])
        assert same_bits(got[3], oracle_mod.reduce(sums[:, 3], FLOAT, ADD) / np.float32(wrapped))


@pytest.mark.parametrize("nranks", [2, 9])
def test_means_padded_and_misaligned_rows(gpu, oracle_mod, nranks):
    """Rank rows as windows of wider buffers: pitch 8*64 + 4 keeps every row
    16-byte aligned at offset 0 (vector path); offset 1 misaligns every row
    (scalar path).  `out` given by the caller."""
    from smi_amd import kmeans
    clusters, dims = 8, 64
    kd = clusters * dims
    rng = np.random.default_rng(nranks)
    wide_s = (rng.standard_normal((nranks, kd + 4)) * 10).astype(np.float32)
    wide_c = rng.integers(1, 1000, (nranks, clusters + 3)).astype(np.int32)
    ds, dc = dev(wide_s), dev(wide_c)
    for lo in (0, 1):
        vs = ds[:, lo:lo + kd].unflatten(1, (clusters, dims))
        vc = dc[:, lo:lo + clusters]
        assert vs.stride(0) == kd + 4 and (vs.data_ptr() % 16 == 0) == (lo == 0)
        out = torch.full((clusters, dims), -1.0, device="cuda")
        assert kmeans.means(vs, vc, out=out) is out
        want = want_means(oracle_mod, np.ascontiguousarray(wide_s[:, lo:lo + kd]).reshape(nranks, clusters, dims),
                          np.ascontiguousarray(wide_c[:, lo:lo + clusters]))
        assert same_bits(out.cpu().numpy(), want), (nranks, lo)


def test_means_bad_arguments_raise(gpu):
    from smi_amd import SMIError, kmeans
    with pytest.raises(SMIError):
        kmeans.means(torch.zeros((65, 2, 4), device="cuda"), torch.zeros((65, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(SMIError):
        kmeans.means(torch.zeros((2, 2, 4), device="cuda"), torch.zeros((2, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(SMIError):
        kmeans.means(torch.zeros((2, 2, 4), device="cuda").double(),
                     torch.zeros((2, 2), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------- the whole program --
def _blobs(n, dims, clusters, seed):
    rng = np.random.default_rng(seed)
    centres = (rng.random((clusters, dims), dtype=np.float32) * 10 - 5)
    pts = rng.standard_normal((n, dims), dtype=np.float32) + centres[np.arange(n) % clusters]
    return pts, pts[rng.choice(n, clusters, replace=False)].copy()


def _run_program(pts, cen0, iters, ranks, width, mode):
    from smi_amd import LocalGroup, kmeans
    kmeans.set_means(mode)
    try:
        def fn(comm):
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                local = dev(kmeans.split_points(pts, comm.size, comm.rank))
                c = dev(cen0.copy())
                kmeans.kmeans(comm, local, c, iters, width=width)
                s.synchronize()
                return c.cpu().numpy()

        return LocalGroup(ranks).run(fn)
    finally:
        kmeans.set_means(0)


def _check_program(oracle_mod, pts, cen0, ranks, width, iters=3):
    want = oracle_mod.kmeans(pts, cen0, iters, ranks=ranks, width=width)
    fused = _run_program(pts, cen0, iters, ranks, width, 1)
    plain = _run_program(pts, cen0, iters, ranks, width, 0)
    for r in range(ranks):
        assert same_bits(fused[r], want), r
        assert same_bits(fused[r], plain[r]), r
        # mode 0's bits exactly where neither is a NaN, and NaN in the same places
        assert np.array_equal(np.isnan(fused[r]), np.isnan(plain[r]))
    return want


@pytest.mark.parametrize("ranks", [1, 2, 4, 8])
@pytest.mark.parametrize("clusters,dims,width", [(8, 64, 16), (5, 48, 3)])
def test_program_fused_means_matches_oracle_and_mode0(gpu, oracle_mod, ranks, clusters, dims, width):
    pts, cen0 = _blobs(64 * ranks, dims, clusters, seed=ranks + clusters)
    _check_program(oracle_mod, pts, cen0, ranks, width)


@pytest.mark.parametrize("ranks", [1, 2, 4, 8])
def test_program_fused_means_empty_cluster(gpu, oracle_mod, ranks):
    """A centroid no point ever picks: 0/0 = NaN on every rank, which then
    never wins a point."""
    pts, cen0 = _blobs(64 * ranks, 64, 8, seed=40 + ranks)
    cen0[4] = 1e6
    want = _check_program(oracle_mod, pts, cen0, ranks, 16)
    assert np.isnan(want[4]).all() and not np.isnan(np.delete(want, 4, axis=0)).any()


@pytest.mark.parametrize("ranks", [1, 2, 4, 8])
def test_program_fused_means_record_fallback(gpu, oracle_mod, ranks):
    """16 clusters x 4112 dims: the sums alone are 263,168 B, so the record is
    above 256 KiB and takes two allreduces and the divide;
    clusters * dims / width = 4112 <= 16384."""
    pts, cen0 = _blobs(64 * ranks, 4112, 16, seed=70 + ranks)
    _check_program(oracle_mod, pts, cen0, ranks, 16)
