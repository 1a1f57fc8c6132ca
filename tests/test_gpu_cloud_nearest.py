"""prg_nearest_ragged_f64 / geometry.nearest_ragged / postprocess.nearest_hip on an MI355X.  Run with `-m gpu`.

Everything is BIT-EXACT: three float64 differences, three products and two sums without contraction, a strict < over the
other cloud in ascending row order have one right answer, which `postprocess.nearest` states in numpy and
tests/test_cloud_nearest_spec.py checks against a KD-tree on the CPU.  The kernel stages the other cloud in tiles of 256 rows
and answers 2 x 256 query rows per workgroup: the sizes below sit on both sides of 64 (a wave), 256 (a tile, a half slab),
512 (a slab) and their doubles."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

PRG_E_INVALID = -1
D2_SENTINEL, IDX_SENTINEL = -7.0, -77
POISON = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]


@pytest.fixture(scope="module")
def L():
    from pointreggpt_amd import _lib
    _lib.load()
    return _lib


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cloud(rng, n):
    return rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


def pack(segs, head=0, tail=0):
    """Ragged buffer with `head` / `tail` poisoned rows (NaN with a recognisable payload) outside every segment."""
    offs = np.zeros(len(segs) + 1, dtype=np.int64)
    offs[0] = head
    offs[1:] = head + np.cumsum([len(s) for s in segs])
    pts = np.concatenate([np.full((head, 3), POISON)] + [np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in segs]
                         + [np.full((tail, 3), POISON)], 0)
    return pts, offs


def launch(L, pairs, head=0, tail=0, max_cloud=None):
    """One call on sentinel-filled outputs -> (d2, idx, offs, pts after the call), all on the host."""
    segs = [c for pair in pairs for c in pair]
    pts, offs = pack(segs, head, tail)
    n = max(len(pts), 1)
    d_pts = D(pts if len(pts) else np.zeros((1, 3)))
    d2 = torch.full((n,), D2_SENTINEL, dtype=torch.float64, device="cuda")
    idx = torch.full((n,), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    if max_cloud is None:
        max_cloud = max(1, max(len(s) for s in segs))
    rc = L.load().prg_nearest_ragged_f64(L.ptr(d_pts), L.ptr(D(offs)), len(pairs), int(max_cloud), L.ptr(d2), L.ptr(idx),
                                         L.stream_ptr())
    assert rc == 0, L.load().prg_last_error()
    torch.cuda.synchronize()
    return d2.cpu().numpy()[:len(pts)], idx.cpu().numpy()[:len(pts)], offs, d_pts.cpu().numpy()[:len(pts)]


def check(L, pairs, head=0, tail=0):
    """The call against the numpy specification, bit for bit, both directions of every pair; rows outside every segment keep
    the sentinels and `pts` keeps its poison."""
    d2, idx, offs, pts_after = launch(L, pairs, head, tail)
    pts_before, _ = pack([c for pair in pairs for c in pair], head, tail)
    assert np.array_equal(bits(pts_after), bits(pts_before))
    for p, (a, b) in enumerate(pairs):
        o0, o1, o2 = offs[2 * p], offs[2 * p + 1], offs[2 * p + 2]
        for (lo, hi), (q, r) in (((o0, o1), (a, b)), ((o1, o2), (b, a))):
            want_d2, want_idx = PP.nearest(q, r)
            assert np.array_equal(bits(d2[lo:hi]), bits(want_d2)), ("d2", p, len(q), len(r))
            assert np.array_equal(idx[lo:hi], want_idx), ("idx", p, len(q), len(r))
    outside = np.r_[0:offs[0], offs[-1]:len(d2)]
    assert np.all(d2[outside] == D2_SENTINEL) and np.all(idx[outside] == IDX_SENTINEL)
    return d2, idx, offs


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_the_spec(L, n):
    """n rows against n + 1, against 300 (more than one tile, not a multiple) and against 1 — one launch of three pairs."""
    rng = np.random.default_rng(n)
    check(L, [(cloud(rng, n), cloud(rng, n + 1)), (cloud(rng, n), cloud(rng, 300)), (cloud(rng, 1), cloud(rng, n))])


def test_lopsided_pairs(L):
    rng = np.random.default_rng(7)
    check(L, [(cloud(rng, 3), cloud(rng, 1500))])
    check(L, [(cloud(rng, 1500), cloud(rng, 3))])
    check(L, [(cloud(rng, 3), cloud(rng, 1500)), (cloud(rng, 1500), cloud(rng, 3))])


def test_empty_clouds(L):
    rng = np.random.default_rng(8)
    e = np.zeros((0, 3))
    d2, idx, offs = check(L, [(e, cloud(rng, 300)), (cloud(rng, 300), e), (e, e), (cloud(rng, 5), cloud(rng, 6))])
    assert np.all(np.isposinf(d2[:600])) and np.all(idx[:600] == -1)                 # nothing to find in an empty cloud
    check(L, [(e, cloud(rng, 70))])
    check(L, [(cloud(rng, 70), e)])
    d2, idx, _, _ = launch(L, [(e, e)], head=0, tail=4)                              # both empty: nothing is written at all
    assert np.all(d2 == D2_SENTINEL) and np.all(idx == IDX_SENTINEL)


@pytest.mark.parametrize("head,tail", [(5, 0), (0, 9), (301, 777)])
def test_rows_outside_every_segment_are_left_alone(L, head, tail):
    rng = np.random.default_rng(head + tail)
    check(L, [(cloud(rng, 257), cloud(rng, 513)), (cloud(rng, 64), cloud(rng, 1))], head=head, tail=tail)


def test_duplicates_across_a_tile_boundary_take_the_lowest_row(L):
    rng = np.random.default_rng(9)
    b = cloud(rng, 700)
    for lo, hi in ((255, 256), (100, 600), (511, 512), (254, 258)):
        b[hi] = b[lo]
    a = np.concatenate([b[[255, 100, 511, 254]], b[[255, 100, 511, 254]] + 1e-7, cloud(rng, 50)])
    d2, idx, offs = check(L, [(a, b)])
    assert idx[:8].tolist() == [255, 100, 511, 254] * 2 and np.all(d2[:4] == 0.0)
    # four candidates at one distance from the query, one per tile
    b = cloud(rng, 1025) + 10.0
    for j, v in ((3, [1.0, 0, 0]), (300, [-1.0, 0, 0]), (600, [0, 1.0, 0]), (1024, [0, 0, -1.0])):
        b[j] = v
    d2, idx, _ = check(L, [(np.zeros((1, 3)), b)])
    assert idx[0] == 3 and d2[0] == 1.0


def test_a_cloud_against_itself(L):
    rng = np.random.default_rng(10)
    a = cloud(rng, 777)
    a[600] = a[4]
    a[300] = a[299]
    d2, idx, offs = check(L, [(a, a)])
    want = np.arange(777)
    want[600], want[300] = 4, 299
    assert np.all(d2 == 0.0) and np.array_equal(idx[:777], want) and np.array_equal(idx[777:], want)


def test_nan_rows(L):
    rng = np.random.default_rng(11)
    a, b = cloud(rng, 300), cloud(rng, 520)
    a[0, 0] = a[17, 1] = a[299, 2] = np.nan
    b[0] = np.nan
    b[255, 1] = b[256, 2] = b[519, 0] = np.nan
    d2, idx, offs = check(L, [(a, b), (cloud(rng, 9), np.full((4, 3), np.nan))])
    assert np.all(np.isposinf(d2[[0, 17, 299]])) and np.all(idx[[0, 17, 299]] == -1)
    assert not np.isin(idx[:300], [0, 255, 256, 519]).any()
    assert np.all(np.isposinf(d2[offs[2]:offs[4]])) and np.all(idx[offs[2]:offs[4]] == -1)


def test_overflowing_distances(L):
    rng = np.random.default_rng(12)
    a, b = cloud(rng, 70), cloud(rng, 80)
    a[3] = [1e200, 0.0, 0.0]
    b[5] = [0.0, -1e200, 1e200]
    d2, idx, offs = check(L, [(a, b), (np.full((2, 3), 1e200), np.full((3, 3), -1e200))])
    assert np.isposinf(d2[3]) and idx[3] == -1 and np.isposinf(d2[70 + 5]) and idx[70 + 5] == -1
    assert np.all(np.isposinf(d2[offs[2]:])) and np.all(idx[offs[2]:] == -1)


@pytest.mark.parametrize("n_pairs", [1, 3, 64])
def test_a_pair_does_not_depend_on_its_neighbours(L, n_pairs):
    """One pair alone gives the bits it gives as the first, middle and last of n_pairs pairs (checked against the spec too)."""
    rng = np.random.default_rng(13)
    mine = (cloud(rng, 600), cloud(rng, 333))
    alone_d2, alone_idx, _, _ = launch(L, [mine])
    sizes = rng.integers(0, 700, size=(n_pairs, 2))
    others = [(cloud(rng, int(n)), cloud(rng, int(m))) for n, m in sizes]
    for pos in sorted({0, n_pairs // 2, n_pairs - 1}):
        pairs = list(others)
        pairs[pos] = mine
        if pos == 0:
            d2, idx, offs = check(L, pairs)                      # every pair of one of the launches against the spec
        else:
            d2, idx, offs, _ = launch(L, pairs)
        lo, hi = offs[2 * pos], offs[2 * pos + 2]
        assert np.array_equal(bits(d2[lo:hi]), bits(alone_d2)) and np.array_equal(idx[lo:hi], alone_idx)


def test_counts_below_r_squared_are_prg_overlap_counts(L):
    """(d2 < r*r) per cloud is the overlap count of the same buffer: the two kernels share the distance expression."""
    rng = np.random.default_rng(14)
    r = 0.0375
    pairs = []
    for n, m in ((900, 1100), (257, 64), (40, 0), (513, 513)):
        a = rng.uniform(-0.3, 0.3, (n, 3))
        b = np.concatenate([a[: m // 2] + rng.normal(0, r / 2, (m // 2, 3)), rng.uniform(-0.3, 0.3, (m - m // 2, 3))])
        pairs.append((a, b))
    pts, offs = pack([c for p in pairs for c in p], head=3, tail=2)
    d_pts, d_offs = D(pts), D(offs)
    from pointreggpt_amd import geometry as G
    d2, _idx = G.nearest_ragged(d_pts, d_offs, len(pairs), 1100)
    counts = torch.full((len(pairs), 2), -1, dtype=torch.int32, device="cuda")
    lib = L.load()
    L.check(lib.prg_overlap_counts(L.ptr(d_pts), L.ptr(d_offs), len(pairs), 1100, r, L.ptr(counts), L.stream_ptr()))
    torch.cuda.synchronize()
    d2, counts = d2.cpu().numpy(), counts.cpu().numpy().reshape(-1)
    mine = np.array([int((d2[offs[k]:offs[k + 1]] < r * r).sum()) for k in range(2 * len(pairs))])
    assert np.array_equal(mine, counts)
    assert 0 < mine[0] < 900 and 0 < mine[1] < 1100                                 # the radius actually splits the clouds
    assert np.all(np.isposinf(d2[:3])) and np.all(np.isposinf(d2[-2:]))             # nearest_ragged's own fill outside


def test_python_layers(L):
    """geometry.nearest_ragged returns device tensors; postprocess.nearest_hip splits them per pair."""
    rng = np.random.default_rng(15)
    e = np.zeros((0, 3))
    pairs = [(cloud(rng, 130), cloud(rng, 700)), (e, cloud(rng, 10)), (cloud(rng, 513), cloud(rng, 2))]
    got = PP.nearest_hip(pairs)
    assert len(got) == 3
    for (a, b), (d2_ab, i_ab, d2_ba, i_ba) in zip(pairs, got):
        for (q, r), (d2, idx) in (((a, b), (d2_ab, i_ab)), ((b, a), (d2_ba, i_ba))):
            want_d2, want_idx = PP.nearest(q, r)
            assert d2.dtype == np.float64 and idx.dtype == np.int32
            assert np.array_equal(bits(d2), bits(want_d2)) and np.array_equal(idx, want_idx)
    assert PP.nearest_hip([]) == []
    (d2_ab, i_ab, d2_ba, i_ba), = PP.nearest_hip([(e, e)])
    assert d2_ab.shape == i_ab.shape == d2_ba.shape == i_ba.shape == (0,)
    from pointreggpt_amd import geometry as G
    with pytest.raises(L.PrgError):
        G.nearest_ragged(torch.zeros((4, 3), dtype=torch.float64), torch.zeros(3, dtype=torch.int64), 1, 4)


def test_bad_arguments(L):
    lib = L.load()
    pts, offs = D(np.zeros((4, 3))), D(np.array([0, 2, 4], dtype=np.int64))
    d2 = torch.full((4,), D2_SENTINEL, dtype=torch.float64, device="cuda")
    idx = torch.full((4,), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    s = L.stream_ptr()
    p, o, d, i = L.ptr(pts), L.ptr(offs), L.ptr(d2), L.ptr(idx)
    for args in ((None, o, 1, 2, d, i), (p, None, 1, 2, d, i), (p, o, 1, 2, None, i), (p, o, 1, 2, d, None),
                 (p, o, 0, 2, d, i), (p, o, 65536, 2, d, i), (p, o, -1, 2, d, i), (p, o, 1, 0, d, i)):
        rc = lib.prg_nearest_ragged_f64(*args, s)
        assert rc == PRG_E_INVALID and b"prg_nearest_ragged_f64" in lib.prg_last_error(), args
    torch.cuda.synchronize()
    assert np.all(d2.cpu().numpy() == D2_SENTINEL) and np.all(idx.cpu().numpy() == IDX_SENTINEL)
    assert lib.prg_nearest_ragged_f64(p, o, 1, 2, d, i, s) == 0
    torch.cuda.synchronize()
    assert np.all(d2.cpu().numpy() == 0.0) and np.all(idx.cpu().numpy() == 0)
