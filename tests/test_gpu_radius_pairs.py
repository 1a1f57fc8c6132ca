"""prg_radius_count_ragged_f64 / prg_radius_fill_ragged_f64 / geometry.radius_pairs_ragged / postprocess.radius_pairs_hip on an
MI355X.  Run with `-m gpu`.

Everything is BIT-EXACT: three float64 differences, three products and two sums without contraction and a strict < against
r*r have one right answer per (i, j), and the order (pair, i, j) is fixed; `postprocess.radius_pairs` states both in numpy and
tests/test_radius_pairs_spec.py checks it against a KD-tree on the CPU.  The kernels stage the candidate cloud in tiles of 256
rows and answer 2 x 256 query rows per workgroup (a slab of 512, the sibling kernel's): the sizes below sit on both sides of 64
(a wave), 256 (a tile, a half slab), 512 (a slab) and 1024 (two slabs, one block of the row scan)."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

R = 0.5                    # ~8 matches per query row of a 1025-row cloud in the 64 m^3 box (tests/test_radius_pairs_spec.py)
ROW_SENTINEL, CORR_SENTINEL = -7, -77
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


def launch(L, pairs, radius=R, head=0, tail=0, capacity=None, slack=8):
    """count + fill on sentinel-filled outputs -> (row_start (total+1), corr buffer (capacity + slack rows), offs, total), host."""
    lib = L.load()
    segs = [c for pair in pairs for c in pair]
    pts, offs = pack(segs, head, tail)
    total = len(pts)
    d_pts = D(pts if total else np.zeros((1, 3)))
    d_offs = D(offs)
    max_cloud = max(1, max(len(s) for s in segs))
    row_start = torch.full((total + 1,), ROW_SENTINEL, dtype=torch.int64, device="cuda")
    ws = torch.empty((int(lib.prg_radius_pairs_workspace_bytes(total)),), dtype=torch.uint8, device="cuda")
    rc = lib.prg_radius_count_ragged_f64(L.ptr(d_pts), L.ptr(d_offs), len(pairs), total, max_cloud, radius, L.ptr(row_start),
                                         L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == 0, lib.prg_last_error()
    rs = row_start.cpu().numpy()
    K = int(rs[-1])
    if capacity is None:
        capacity = K
    corr = torch.full((capacity + slack, 2), CORR_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.prg_radius_fill_ragged_f64(L.ptr(d_pts), L.ptr(d_offs), len(pairs), max_cloud, radius, L.ptr(row_start), capacity,
                                        L.ptr(corr), L.stream_ptr())
    assert rc == 0, lib.prg_last_error()
    torch.cuda.synchronize()
    if total:
        assert np.array_equal(bits(d_pts.cpu().numpy()), bits(pts))                   # pts unchanged, poison included
    assert np.array_equal(row_start.cpu().numpy(), rs)                                # fill does not touch row_start
    return rs, corr.cpu().numpy(), offs, total


def check(L, pairs, radius=R, head=0, tail=0):
    """Both passes against the numpy specification, bit for bit; -> (per-pair corr, row_start, offs)."""
    rs, corr, offs, total = launch(L, pairs, radius, head, tail)
    K = int(rs[-1])
    assert rs.shape == (total + 1,) and rs[0] == 0 and np.all(np.diff(rs) >= 0)       # written in full, non-decreasing
    assert np.all(rs[:offs[0] + 1] == 0) and np.all(rs[offs[-1]:] == K)               # rows outside contribute nothing
    assert np.all(corr[K:] == CORR_SENTINEL)                                          # nothing past the list
    got = []
    for p, (a, b) in enumerate(pairs):
        o0, o1, o2 = offs[2 * p], offs[2 * p + 1], offs[2 * p + 2]
        want = PP.radius_pairs(a, b, radius)
        mine = corr[rs[o0]:rs[o2]]
        assert np.array_equal(mine, want), (p, len(a), len(b), len(mine), len(want))
        assert np.all(rs[o1:o2 + 1] == rs[o1])                                        # rows of B are no query rows
        per_row = np.bincount(want[:, 0], minlength=len(a)) if len(a) else np.zeros(0, dtype=np.int64)
        assert np.array_equal(np.diff(rs[o0:o1 + 1]), per_row)                        # each query row owns its range
        got.append(mine)
    assert sum(len(g) for g in got) == K
    return got, rs, offs


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_the_spec(L, n):
    """n rows against n + 1, against 300 (more than one tile, not a multiple) and against 1 — one launch of three pairs."""
    rng = np.random.default_rng(n)
    one = cloud(rng, 1)
    a3 = cloud(rng, n)
    a3[n // 2] = one[0] + 0.01                                                        # the single candidate has a match
    got, _, _ = check(L, [(cloud(rng, n), cloud(rng, n + 1)), (cloud(rng, n), cloud(rng, 300)), (a3, one)])
    assert len(got[2]) >= 1
    if n >= 255:
        assert len(got[0]) > 0 and len(got[1]) > 0


def test_a_pair_with_no_match_among_pairs_that_have_some(L):
    rng = np.random.default_rng(21)
    got, rs, offs = check(L, [(cloud(rng, 600), cloud(rng, 520)), (cloud(rng, 300), cloud(rng, 300) + 100.0),
                              (cloud(rng, 257), cloud(rng, 700))])
    assert len(got[0]) > 0 and len(got[1]) == 0 and len(got[2]) > 0


def test_empty_clouds(L):
    rng = np.random.default_rng(22)
    e = np.zeros((0, 3))
    got, rs, offs = check(L, [(e, cloud(rng, 300)), (cloud(rng, 300), e), (e, e), (cloud(rng, 600), cloud(rng, 600))])
    assert [len(g) for g in got[:3]] == [0, 0, 0] and len(got[3]) > 0
    check(L, [(e, cloud(rng, 70))])
    check(L, [(cloud(rng, 70), e)])
    rs, corr, _, total = launch(L, [(e, e), (e, e)], tail=4)                          # every cloud empty
    assert np.all(rs == 0) and rs.shape == (5,) and np.all(corr == CORR_SENTINEL)
    rs, corr, _, total = launch(L, [(e, e)])                                          # ... and no row at all
    assert total == 0 and rs.tolist() == [0] and np.all(corr == CORR_SENTINEL)


@pytest.mark.parametrize("head,tail", [(5, 0), (0, 9), (301, 1777), (1_048_877, 3)])
def test_rows_outside_every_segment_are_left_alone(L, head, tail):
    """offsets[0] > 0, NaN-poisoned rows before and after: not read (they would poison nothing, but pts must stay as it is),
    and row_start is flat over them.  The last case puts the pairs behind more than 1024 blocks of the row scan, where the
    one-workgroup scan over the block sums is in the second round of its carry loop."""
    rng = np.random.default_rng(head + tail)
    got, _, _ = check(L, [(cloud(rng, 700), cloud(rng, 513)), (cloud(rng, 64), cloud(rng, 1))], head=head, tail=tail)
    assert len(got[0]) > 0


def test_nan_rows(L):
    rng = np.random.default_rng(23)
    a, b = cloud(rng, 600), cloud(rng, 520)
    a[0, 0] = a[17, 1] = a[599, 2] = np.nan
    b[0] = np.nan
    b[255, 1] = b[256, 2] = b[519, 0] = np.nan
    got, _, _ = check(L, [(a, b), (cloud(rng, 9), np.full((4, 3), np.nan)), (np.full((4, 3), np.nan), cloud(rng, 300))])
    assert len(got[0]) > 0 and len(got[1]) == 0 and len(got[2]) == 0
    assert not np.isin(got[0][:, 0], [0, 17, 599]).any() and not np.isin(got[0][:, 1], [0, 255, 256, 519]).any()


def test_duplicate_points(L):
    """Equal distances, several j per i, across tile boundaries; a cloud against itself has at least its diagonal."""
    rng = np.random.default_rng(24)
    b = cloud(rng, 700)
    for lo, hi in ((255, 256), (100, 600), (511, 512), (254, 258)):
        b[hi] = b[lo]
    a = np.concatenate([b[[255, 100, 511, 254]], b[[255, 100, 511, 254]] + 1e-7, cloud(rng, 50)])
    got, _, _ = check(L, [(a, b)], radius=1e-3)
    assert got[0][:8].tolist() == [[0, 255], [0, 256], [1, 100], [1, 600], [2, 511], [2, 512], [3, 254], [3, 258]]
    c = cloud(rng, 777)
    c[600] = c[4]
    got, _, _ = check(L, [(c, c)])
    diag = got[0][got[0][:, 0] == got[0][:, 1]]
    assert np.array_equal(diag[:, 0], np.arange(777))
    assert [4, 600] in got[0].tolist() and [600, 4] in got[0].tolist()
    # the bound is strict: a candidate at exactly the radius is out, one ulp further in it is in
    q, cand = np.zeros((1, 3)), np.array([[0.5, 0, 0], [0, np.nextafter(0.5, 0), 0], [0, 0, -0.5]])
    got, _, _ = check(L, [(q, cand)], radius=0.5)
    assert got[0].tolist() == [[0, 1]]


def voxel_like(rng, n):
    """A 2.5 cm grid surface patch and the same patch with a 1 cm jitter: what a finished pair looks like at loader radii."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a, b[rng.permutation(n)]


def test_voxel_grid_like_clouds_at_the_loader_radius(L):
    rng = np.random.default_rng(25)
    pairs = [voxel_like(rng, 1500), voxel_like(rng, 700)]
    got, _, _ = check(L, pairs, radius=0.0375)
    assert 3 * 1500 < len(got[0]) < 12 * 1500                                        # several matches per overlapping point


@pytest.mark.parametrize("n_pairs", [1, 3, 64])
def test_a_pair_does_not_depend_on_its_neighbours(L, n_pairs):
    """One pair alone gives the list it gives as the first, middle and last of n_pairs pairs (checked against the spec too)."""
    rng = np.random.default_rng(26)
    mine = (cloud(rng, 600), cloud(rng, 333))
    (alone,), _, _ = check(L, [mine])
    assert len(alone) > 0
    sizes = rng.integers(0, 700, size=(n_pairs, 2))
    others = [(cloud(rng, int(n)), cloud(rng, int(m))) for n, m in sizes]
    for pos in sorted({0, n_pairs // 2, n_pairs - 1}):
        pairs = list(others)
        pairs[pos] = mine
        if pos == 0:
            got, rs, offs = check(L, pairs)                       # every pair of one of the launches against the spec
            assert np.array_equal(got[pos], alone)
        else:
            rs, corr, offs, _ = launch(L, pairs)
            assert np.array_equal(corr[rs[offs[2 * pos]]:rs[offs[2 * pos + 2]]], alone)


def test_capacity_smaller_than_the_list(L):
    """capacity = K - 3 on a K + 8-row buffer: the first K - 3 rows are the spec's, every later row keeps the sentinel."""
    rng = np.random.default_rng(27)
    pairs = [(cloud(rng, 600), cloud(rng, 520)), (cloud(rng, 130), cloud(rng, 257))]
    want = np.concatenate([PP.radius_pairs(a, b, R) for a, b in pairs])
    K = len(want)
    assert K > 100
    rs, corr, offs, _ = launch(L, pairs, capacity=K - 3, slack=11)
    assert int(rs[-1]) == K and corr.shape == (K + 8, 2)
    assert np.array_equal(corr[:K - 3], want[:K - 3]) and np.all(corr[K - 3:] == CORR_SENTINEL)
    rs, corr, offs, _ = launch(L, pairs, capacity=0, slack=K + 8)                     # capacity 0: nothing is written
    assert int(rs[-1]) == K and np.all(corr == CORR_SENTINEL)


def test_agrees_with_the_overlap_and_nearest_kernels(L):
    """On one buffer: A rows with a non-empty range = prg_overlap_counts' counts[p][0], distinct j = counts[p][1], and a row has
    matches iff prg_nearest_ragged_f64 gives it d2 < r*r — the three kernels share the distance expression."""
    from pointreggpt_amd import geometry as G
    rng = np.random.default_rng(28)
    r = 0.0375
    pairs = []
    for n, m in ((900, 1100), (257, 64), (40, 0), (513, 513)):
        a = rng.uniform(-0.3, 0.3, (n, 3))
        b = np.concatenate([a[: m // 2] + rng.normal(0, r / 2, (m // 2, 3)), rng.uniform(-0.3, 0.3, (m - m // 2, 3))])
        pairs.append((a, b))
    pts, offs = pack([c for p in pairs for c in p], head=3, tail=2)
    d_pts, d_offs = D(pts), D(offs)
    lib = L.load()
    corr, po = G.radius_pairs_ragged(d_pts, d_offs, len(pairs), 1100, r)
    d2, _idx = G.nearest_ragged(d_pts, d_offs, len(pairs), 1100)
    counts = torch.full((len(pairs), 2), -1, dtype=torch.int32, device="cuda")
    L.check(lib.prg_overlap_counts(L.ptr(d_pts), L.ptr(d_offs), len(pairs), 1100, r, L.ptr(counts), L.stream_ptr()))
    torch.cuda.synchronize()
    corr, po, d2, counts = corr.cpu().numpy(), po.cpu().numpy(), d2.cpu().numpy(), counts.cpu().numpy()
    assert po.shape == (len(pairs) + 1,) and po[0] == 0 and po[-1] == len(corr)
    for p, (a, b) in enumerate(pairs):
        mine = corr[po[p]:po[p + 1]]
        assert np.array_equal(mine, PP.radius_pairs(a, b, r))
        assert len(np.unique(mine[:, 0])) == counts[p, 0] and len(np.unique(mine[:, 1])) == counts[p, 1]
        has = np.zeros(len(a), dtype=bool)
        has[mine[:, 0]] = True
        assert np.array_equal(has, d2[offs[2 * p]:offs[2 * p + 1]] < r * r)
    assert 0 < counts[0, 0] < 900 and 0 < counts[0, 1] < 1100                        # the radius actually splits the clouds


def test_python_layers(L):
    """geometry.radius_pairs_ragged returns device tensors of exactly K rows; postprocess.radius_pairs_hip splits them per pair."""
    from pointreggpt_amd import geometry as G
    rng = np.random.default_rng(29)
    e = np.zeros((0, 3))
    pairs = [(cloud(rng, 700), cloud(rng, 530)), (e, cloud(rng, 10)), (cloud(rng, 513), cloud(rng, 2)), (cloud(rng, 300), cloud(rng, 300) + 50.0)]
    got = PP.radius_pairs_hip(pairs, R)
    assert len(got) == len(pairs) and len(got[0]) > 0
    for (a, b), corr in zip(pairs, got):
        assert corr.dtype == np.int32 and corr.ndim == 2 and corr.shape[1] == 2
        assert np.array_equal(corr, PP.radius_pairs(a, b, R))
    assert PP.radius_pairs_hip([], R) == []
    (c,) = PP.radius_pairs_hip([(e, e)], R)
    assert c.shape == (0, 2) and c.dtype == np.int32
    far = PP.radius_pairs_hip([pairs[3]], R)                                           # K = 0 with rows present: no fill at all
    assert far[0].shape == (0, 2)
    pts, offs = pack([pairs[0][0], pairs[0][1]])
    corr, po = G.radius_pairs_ragged(D(pts), D(offs), 1, 700, R)
    assert corr.is_cuda and corr.dtype == torch.int32 and po.is_cuda and po.dtype == torch.int64
    assert corr.shape == (len(got[0]), 2) and po.cpu().tolist() == [0, len(got[0])]
    with pytest.raises(L.PrgError):
        G.radius_pairs_ragged(torch.zeros((4, 3), dtype=torch.float64), torch.zeros(3, dtype=torch.int64), 1, 4, R)
    with pytest.raises(L.PrgError):
        G.radius_pairs_ragged(D(pts), D(offs), 1, 700, float("nan"))
