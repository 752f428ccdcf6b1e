"""kmeans_smi parity on the GPU (examples/kernels/kmeans_smi.cl,
examples/host/kmeans_smi.cpp), all through the C ABI.

Contract: bit-exact vs the oracle's restatement (oracle/smi_oracle.c) --
assignments and counts exactly; per-cluster sums bitwise (fp32 chains in
point order; the oracle restates the literal `+= (index == k) ? x : 0` of
kmeans_smi.cl:122); centroids bitwise after the canonical reduce fold and
IEEE division, NaN payloads aside (an empty cluster is 0/0 in both).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n,dims,clusters,width", [
    (1, 64, 8, 16), (1000, 64, 8, 16), (4099, 64, 8, 1), (777, 48, 5, 3), (300, 8, 256, 4),
    (2500, 256, 16, 16), (513, 100, 3, 100), (65536, 64, 8, 16)])
def test_assign_matches_oracle(gpu, oracle_mod, n, dims, clusters, width):
    from smi_amd import kmeans
    rng = np.random.default_rng(n * 7 + dims)
    pts = rng.standard_normal((n, dims), dtype=np.float32)
    cen = rng.standard_normal((clusters, dims), dtype=np.float32)
    want = oracle_mod.kmeans_assign(pts, cen, width)
    got = kmeans.assign(dev(pts), dev(cen), width).cpu().numpy()
    assert np.array_equal(got, want)


def test_assign_ties_nan_inf(gpu, oracle_mod):
    """Strict < from +inf (kmeans_smi.cl:75-83): duplicate centroids keep the
    lower index, NaN distances never win, all-NaN/inf points go to 0."""
    from smi_amd import kmeans
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((600, 32), dtype=np.float32)
    pts[5] = np.nan
    pts[6] = np.inf
    c = rng.standard_normal((2, 32), dtype=np.float32)
    cen = np.stack([c[0], c[0], np.full(32, np.nan, np.float32), np.full(32, np.inf, np.float32), c[1]])
    for width in (1, 4, 16):
        want = oracle_mod.kmeans_assign(pts, cen, width)
        got = kmeans.assign(dev(pts), dev(cen), width).cpu().numpy()
        assert np.array_equal(got, want), width
        assert not np.any(got == 1) and got[5] == 0 and got[6] == 0


@pytest.mark.parametrize("n,dims,clusters", [(0, 64, 8), (1, 64, 8), (255, 64, 8), (257, 64, 3), (5000, 64, 8),
                                             (70000, 130, 11), (200000, 64, 8), (3000, 16, 256), (900, 64, 1)])
def test_accumulate_matches_oracle(gpu, oracle_mod, n, dims, clusters):
    from smi_amd import kmeans
    rng = np.random.default_rng(n + clusters)
    pts = rng.standard_normal((n, dims), dtype=np.float32) * 3
    asg = rng.integers(0, max(clusters - 1, 1), n).astype(np.int32)  # the last cluster stays empty
    if n > 10:
        asg[::97] = -1          # outside [0, clusters): no cluster (`index == k` never holds)
        asg[1::89] = clusters
    want_s, want_c = oracle_mod.kmeans_accumulate(pts, asg, clusters)
    s, c = kmeans.accumulate(dev(pts), dev(asg), clusters)
    assert np.array_equal(c.cpu().numpy(), want_c)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want_s.view(np.uint32))


def test_accumulate_long_chain(gpu, oracle_mod):
    """A cluster holding almost all of 2^20 points: one ~10^6-long fp32 chain
    per dimension across thousands of LDS tiles."""
    from smi_amd import kmeans
    n, dims = 1 << 20, 64
    rng = np.random.default_rng(9)
    pts = rng.random((n, dims), dtype=np.float32)
    asg = np.zeros(n, np.int32)
    asg[rng.integers(0, n, 1000)] = 1
    want_s, want_c = oracle_mod.kmeans_accumulate(pts, asg, 2)
    s, c = kmeans.accumulate(dev(pts), dev(asg), 2)
    assert np.array_equal(c.cpu().numpy(), want_c)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want_s.view(np.uint32))


# The fold walks a cluster in LDS tiles of 2048 rows, two steps (register
# buffers) per loop trip: one row short of a tile, a full tile with no tail, a
# second tile of one row, two full tiles, a third tile (odd step) of one row,
# an empty cluster, a single row, three full tiles.
TILE_EDGE_SIZES = [2047, 2048, 2049, 4096, 4097, 0, 1, 6144]


@pytest.mark.parametrize("dims", [12, 8, 1])
def test_accumulate_tile_boundaries(gpu, oracle_mod, dims):
    """dims = 12: a full and a partial 8-dimension workgroup; 1: one lane column."""
    from smi_amd import kmeans
    asg = np.repeat(np.arange(len(TILE_EDGE_SIZES), dtype=np.int32), TILE_EDGE_SIZES)
    rng = np.random.default_rng(2048)
    rng.shuffle(asg)  # every cluster's rows scattered over the points
    n = len(asg)
    assert n == 20482
    pts = rng.standard_normal((n, dims), dtype=np.float32) * 3
    want_s, want_c = oracle_mod.kmeans_accumulate(pts, asg, len(TILE_EDGE_SIZES))
    assert want_c.tolist() == TILE_EDGE_SIZES
    s, c = kmeans.accumulate(dev(pts), dev(asg), len(TILE_EDGE_SIZES))
    assert np.array_equal(c.cpu().numpy(), want_c)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want_s.view(np.uint32))


SPECIAL_SEED = 11  # the oracle-side conditions below hold for this seed


def special_accumulate_case():
    """5000 normally distributed points in 4 clusters: cluster 0 starts (in
    point order) with an all -0.0 point; cluster 1 has one +Inf (dim 2) and one
    NaN (dim 9); cluster 2 one -Inf (dim 5) and, in dim 11, +Inf before -Inf;
    cluster 3 is scaled into the subnormal range."""
    rng = np.random.default_rng(SPECIAL_SEED)
    n, dims, clusters = 5000, 16, 4
    pts = rng.standard_normal((n, dims), dtype=np.float32)
    asg = rng.integers(0, clusters, n).astype(np.int32)
    members = [np.flatnonzero(asg == k) for k in range(clusters)]
    pts[members[0][0], :] = -0.0
    pts[members[1][40], 2] = np.inf
    pts[members[1][300], 9] = np.nan
    pts[members[2][17], 5] = -np.inf
    pts[members[2][100], 11] = np.inf
    pts[members[2][900], 11] = -np.inf
    pts[members[3]] = (pts[members[3]].astype(np.float64) * 1e-39).astype(np.float32)
    return pts, asg, clusters


def test_accumulate_special_values(gpu, oracle_mod):
    """Skipping the other clusters' +0 must not show with -0, Inf, NaN or
    subnormal coordinates: the literal form of the oracle, NaN-aware bitwise."""
    from smi_amd import kmeans
    pts, asg, clusters = special_accumulate_case()
    want_s, want_c = oracle_mod.kmeans_accumulate(pts, asg, clusters)
    # the case is what it claims to be, on the oracle alone
    assert np.isnan(want_s).sum() == 2 and np.isnan(want_s).sum() < want_s.size // 4
    assert np.isnan(want_s[1, 9]) and np.isnan(want_s[2, 11])
    assert want_s[1, 2] == np.inf and want_s[2, 5] == -np.inf
    tiny = np.finfo(np.float32).tiny
    assert (want_s[3] != 0).all()
    assert (np.abs(pts[asg == 3]) < tiny).all() and (pts[asg == 3] != 0).mean() > 0.99
    s, c = kmeans.accumulate(dev(pts), dev(asg), clusters)
    assert np.array_equal(c.cpu().numpy(), want_c)
    assert same_bits(s.cpu().numpy(), want_s)


def test_assign_at_the_lds_limit(gpu, oracle_mod):
    """clusters * dims / width = 16384: 64 KiB of dynamic LDS, the documented
    limit; one more lane per cluster is refused."""
    from smi_amd import SMIError, kmeans
    n, dims, clusters = 300, 64, 256
    rng = np.random.default_rng(16384)
    pts = rng.standard_normal((n, dims), dtype=np.float32)
    cen = rng.standard_normal((clusters, dims), dtype=np.float32)
    want = oracle_mod.kmeans_assign(pts, cen, 1)
    assert len(np.unique(want)) > 64
    got = kmeans.assign(dev(pts), dev(cen), 1).cpu().numpy()
    assert np.array_equal(got, want)
    with pytest.raises(SMIError):
        kmeans.assign(torch.zeros((n, 65), device="cuda"), torch.zeros((clusters, 65), device="cuda"), 1)


def _run_program(pts, cen0, iters, ranks, width):
    from smi_amd import LocalGroup, kmeans

    def fn(comm):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            local = dev(kmeans.split_points(pts, comm.size, comm.rank))
            c = dev(cen0.copy())
            kmeans.kmeans(comm, local, c, iters, width=width)
            s.synchronize()
            return c.cpu().numpy()

    return LocalGroup(ranks).run(fn)


@pytest.mark.parametrize("ranks", [1, 2, 4, 8])
def test_program_matches_oracle(gpu, oracle_mod, ranks):
    """The kmeans_smi program on the reference host's own input (its
    generator, seed 5, 8 clusters x 64 dims, W = 16) split over `ranks`."""
    _, pts, cen0 = oracle_mod.kmeans_reference_data(4096, 8, 64)
    want = oracle_mod.kmeans(pts, cen0, 6, ranks=ranks, width=16)
    for got in _run_program(pts, cen0, 6, ranks, 16):
        assert same_bits(got, want)


def test_program_golden_fixture(gpu, oracle_mod):
    """The committed fixture (tests/golden/golden.json, 8 ranks, W = 16,
    10 iterations) reproduced by the HIP path."""
    import hashlib
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")) as f:
        case = json.load(f)["kmeans"][0]
    _, pts, cen0 = oracle_mod.kmeans_reference_data(case["num_points"], case["clusters"], case["dims"])
    got = _run_program(pts, cen0, case["iterations"], case["ranks"], case["width"])[0]
    assert hashlib.sha256(got.tobytes()).hexdigest() == case["sha256"]


def test_program_plain_distance_and_empty_cluster(gpu, oracle_mod):
    """width = 1 (the plain squared distance) on 3 ranks with a centroid no
    point ever picks: 0/0 = NaN, which then stays empty."""
    _, pts, cen0 = oracle_mod.kmeans_reference_data(1536, 8, 64)
    cen0 = cen0.copy()
    cen0[4] = 1e6
    want = oracle_mod.kmeans(pts, cen0, 5, ranks=3, width=1)
    assert np.isnan(want[4]).all()
    for got in _run_program(pts, cen0, 5, 3, 1):
        assert same_bits(got, want)


def test_bad_arguments_raise(gpu):
    from smi_amd import SMIError, kmeans
    pts = torch.zeros((10, 64), device="cuda")
    with pytest.raises(SMIError):
        kmeans.assign(pts, torch.zeros((8, 64), device="cuda"), width=5)      # 64 % 5 != 0
    with pytest.raises(SMIError):
        kmeans.assign(pts, torch.zeros((257, 64), device="cuda"), width=16)   # > 256 clusters
    with pytest.raises(SMIError):
        kmeans.assign(pts.double(), torch.zeros((8, 64), device="cuda"))
