"""prg_patch_tables_ragged / prg_patch_overlap_ragged_f64 and their Python layers on an MI355X.  Run with `-m gpu`.

Everything is BIT-EXACT against `postprocess.node_patches` / `postprocess.patch_overlaps`, which tests/test_patch_spec.py checks
against an independent formulation on the CPU.  The rank kernel gives one thread to a point and streams its cloud through LDS in
256-row tiles; the pad and box kernels give a wave to a table row, four rows to a workgroup; the overlap kernel gives a thread to
a node pair, 256 pairs to a workgroup, and a wave with 64-slot chunks to a patch: the cloud sizes below sit on both sides of 64
and 256, the node counts on both sides of 4 and 64, the limits on both sides of a wave, and the 1100-member node needs five tiles."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

SENTINEL = -777
LEAD, SLACK = 2, 3         # table rows / node pairs before the first and after the last that nobody owns
POISON = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]
HUGE = 1e300               # a finite row outside every segment: squares overflow


@pytest.fixture(scope="module")
def L():
    from pointreggpt_amd import _lib
    _lib.load()
    return _lib


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pack(segs, head=0, tail=0):
    """Ragged buffer with `head` / `tail` poisoned rows (NaN with a recognisable payload, then huge) outside every segment."""
    offs = np.zeros(len(segs) + 1, dtype=np.int64)
    offs[0] = head
    offs[1:] = head + np.cumsum([len(s) for s in segs])
    poison = lambda n: np.where(np.arange(n)[:, None] % 2 == 0, POISON, HUGE) * np.ones((n, 3))      # noqa: E731
    pts = np.concatenate([poison(head)] + [np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in segs] + [poison(tail)], 0)
    return pts, offs


def surface(rng, n, shift=0.0):
    p = rng.uniform(0, 1, (n, 3))
    p[:, 2] = 0.2 * np.sin(3 * p[:, 0]) + shift
    return p


def nodes_of(rng, pts, m):
    """m nodes: points of the cloud with a little noise while it has that many, the rest far away (nodes without members)."""
    k = min(m, len(pts))
    near = pts[rng.choice(len(pts), k, replace=False)] + rng.normal(0, 0.01, (k, 3))
    return np.concatenate([near, rng.uniform(30, 40, (m - k, 3))])[rng.permutation(m)]


def tables(L, clouds, limit, head=0, tail=0, index_base=None, pad=None):
    """prg_nearest_ragged_f64 + prg_patch_tables_ragged on [points_c | nodes_c] with sentinel-filled outputs, twice -> per cloud
    (assign, table, sizes) on the host.  The inputs must come back as they went in; so must the table rows and sizes that belong
    to no node; every slot and size of every node must have been written; the second run must give the same bytes."""
    lib = L.load()
    segs = [s for c in clouds for s in c]
    pts, offs = pack(segs, head, tail)
    total = len(pts)
    d_pts, d_offs = D(pts if total else np.zeros((1, 3))), D(offs)
    C = len(clouds)
    max_cloud, max_nodes = max(1, max(len(p) for p, _ in clouds)), max(1, max(len(q) for _, q in clouds))
    d2 = torch.full((max(total, 1),), float("inf"), dtype=torch.float64, device="cuda")
    idx = torch.full((max(total, 1),), -1, dtype=torch.int32, device="cuda")
    rc = lib.prg_nearest_ragged_f64(L.ptr(d_pts), L.ptr(d_offs), C, max(max_cloud, max_nodes), L.ptr(d2), L.ptr(idx), L.stream_ptr())
    assert rc == 0, lib.prg_last_error()
    d2_before, idx_before = d2.cpu().numpy(), idx.cpu().numpy()
    m = np.array([len(q) for _, q in clouds], dtype=np.int64)
    t_offs = LEAD + np.concatenate([[0], np.cumsum(m)])
    M = int(m.sum())
    # every device tensor has a name until the launch has finished: a temporary's block goes back to the allocator at once
    d_toffs = D(t_offs[:-1])
    d_base = None if index_base is None else D(np.asarray(index_base, dtype=np.int32))
    d_pad = None if pad is None else D(np.asarray(pad, dtype=np.int32))
    runs = []
    for _ in range(2):
        table = torch.full((LEAD + M + SLACK, limit), SENTINEL, dtype=torch.int32, device="cuda")
        sizes = torch.full((LEAD + M + SLACK,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = lib.prg_patch_tables_ragged(L.ptr(d2), L.ptr(idx), L.ptr(d_offs), C, max_cloud, max_nodes, limit, L.ptr(d_toffs),
                                         L.ptr(d_base), L.ptr(d_pad), L.ptr(table), L.ptr(sizes), L.stream_ptr())
        assert rc == 0, lib.prg_last_error()
        torch.cuda.synchronize()
        runs.append((table.cpu().numpy(), sizes.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    if total:
        assert np.array_equal(bits(d_pts.cpu().numpy()), bits(pts))
    assert np.array_equal(bits(d2.cpu().numpy()), bits(d2_before)) and np.array_equal(idx.cpu().numpy(), idx_before)
    tab, siz = runs[0]
    for out in (tab, siz):
        assert np.all(out[:LEAD] == SENTINEL) and np.all(out[LEAD + M:] == SENTINEL)      # nothing outside the nodes' rows
        assert not np.any(out[LEAD:LEAD + M] == SENTINEL)                                 # every slot and size written
    return [(idx_before[offs[2 * c]:offs[2 * c + 1]], tab[t_offs[c]:t_offs[c + 1]], siz[t_offs[c]:t_offs[c + 1]]) for c in range(C)]


def check_tables(L, clouds, limit, head=0, tail=0, index_base=None, pad=None):
    got = tables(L, clouds, limit, head, tail, index_base, pad)
    for c, (p, q) in enumerate(clouds):
        assign, table, sizes = PP.node_patches(p, q, limit)
        base, padv = 0 if index_base is None else index_base[c], len(p) if pad is None else pad[c]
        table = np.where(table < len(p), table + np.int32(base), np.int32(padv)).astype(np.int32)
        assert np.array_equal(got[c][0], assign), (c, len(p), len(q))
        assert got[c][1].shape == table.shape and np.array_equal(got[c][1], table), (c, len(p), len(q), limit,
                                                                                   np.argwhere(got[c][1] != table)[:4].tolist())
        assert np.array_equal(got[c][2], sizes), (c, len(p), len(q))
    return got


LIMITS = (1, 4, 64, 65, 256)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 700])
def test_tables_sizes_nodes_and_limits(L, n):
    """Four clouds of n rows with 1, 3, 64 and 65 nodes in one launch, at every limit; index_base / pad NULL and given."""
    rng = np.random.default_rng(n)
    clouds = []
    for m in (1, 3, 64, 65):
        p = surface(rng, n)
        clouds.append((p, nodes_of(rng, p, m)))
    for limit in LIMITS:
        got = check_tables(L, clouds, limit)
        if limit == 4 and n >= 255:
            assert (got[1][2] > 4).any() and got[1][2].sum() == n                   # three nodes own n points: truncated rows
        if n <= 63:
            assert (got[3][2] == 0).any() and (got[3][1] == n).any()                # nodes without members, pads
    check_tables(L, clouds, 4, index_base=[1000, 0, 7, 123456], pad=[-1, 5, 2 ** 31 - 1, 0])
    check_tables(L, clouds, 65, head=3, tail=5, index_base=[10, 20, 30, 40], pad=[n, n, n, n])


def test_tables_one_node_owns_40_and_one_owns_1100(L):
    """Members far beyond the limit, and beyond a tile: 1100 points of one node, copies of a point spread over all five tiles so
    that equal distances are ordered by row across tile boundaries."""
    rng = np.random.default_rng(40)
    p40 = np.concatenate([rng.normal(0, 0.01, (40, 3)), rng.normal(5, 0.01, (9, 3))])
    big = np.concatenate([rng.normal(0, 0.02, (1100, 3)), rng.normal(3, 0.02, (100, 3))])
    dup = [5, 250, 256, 300, 511, 512, 600, 1023, 1024, 1099]
    big[dup] = [0.0009765625, 0.0, 0.0]                   # ten copies of the point next to the node: ranks 2 .. 11, by row
    big[[7, 700]] = 0.0                                   # two copies of the node itself: distance 0, ranks 0 and 1
    nodes = np.array([[0.0, 0.0, 0.0], [3.0, 3.0, 3.0], [9.0, 9.0, 9.0]])
    clouds = [(p40, np.array([[0.0, 0.0, 0.0], [5.0, 5.0, 5.0]])), (big, nodes)]
    for limit in (4, 64, 256):
        got = check_tables(L, clouds, limit)
        assert got[0][2].tolist() == [40, 9] and got[1][2].tolist() == [1100, 100, 0]
        assert got[1][1][0][:12].tolist() == ([7, 700] + dup)[:limit]


def test_tables_nan_points_empty_cloud_and_poisoned_surroundings(L):
    rng = np.random.default_rng(41)
    a, b, c = surface(rng, 300), surface(rng, 129), surface(rng, 70)
    a[[0, 17, 299]] = np.nan
    a[64, 1] = np.nan
    na = nodes_of(rng, a[100:200], 9)
    na[4] = np.nan                                        # a NaN node is nobody's nearest
    clouds = [(a, na), (np.zeros((0, 3)), nodes_of(rng, b, 5)), (b, nodes_of(rng, b, 66)), (c, np.zeros((0, 3)))]
    for head, tail in ((0, 0), (5, 4)):
        got = check_tables(L, clouds, 16, head=head, tail=tail)
        assert (got[0][0][[0, 17, 64, 299]] == -1).all() and got[0][2].sum() == 296 and got[0][2][4] == 0
        assert (got[1][2] == 0).all() and (got[1][1] == 0).all()                    # an empty cloud: all pads, and the pad is 0
        assert (got[3][0] == -1).all() and got[3][1].shape == (0, 16)


# ---- patch against patch -------------------------------------------------------------------------------------------------------
def dense_want(a, ta, b, tb, radius):
    corr, hits, _ = PP.patch_overlaps(a, ta, b, tb, radius)
    d = np.zeros((len(ta), len(tb), 2), dtype=np.int32)
    d[corr[:, 0], corr[:, 1]] = hits
    return d.reshape(-1, 2)


def overlaps(L, items, radius, head=0, tail=0, prefilter=True):
    """prg_patch_overlap_ragged_f64 on sentinel-filled dense output, twice -> per item (ms * mt, 2) on the host."""
    lib = L.load()
    pts, offs = pack([c for it in items for c in (it[0], it[2])], head, tail)
    tabs = [np.ascontiguousarray(t, dtype=np.int32) for it in items for t in (it[1], it[3])]
    limit = tabs[0].shape[1]
    m = np.array([len(t) for t in tabs], dtype=np.int64)
    t_offs = 1 + np.concatenate([[0], np.cumsum(m)])                       # one table row in front that belongs to nobody
    tab = np.concatenate([np.full((1, limit), 2 ** 30, np.int32)] + tabs + [np.full((1, limit), -5, np.int32)], 0)
    per_item = m[0::2] * m[1::2]
    h_offs = LEAD + np.concatenate([[0], np.cumsum(per_item)])
    total = int(h_offs[-1]) + SLACK
    d_pts, d_tab, d_offs, d_toffs, d_hoffs = D(pts), D(tab), D(offs), D(t_offs), D(h_offs)   # named until the launch has finished
    runs = []
    for _ in range(2):
        hits = torch.full((total, 2), SENTINEL, dtype=torch.int32, device="cuda")
        boxes = torch.full((len(tab), 6), float(SENTINEL), dtype=torch.float64, device="cuda") if prefilter else None
        rc = lib.prg_patch_overlap_ragged_f64(L.ptr(d_pts), L.ptr(d_offs), len(items), L.ptr(d_tab), L.ptr(d_toffs),
                                              max(1, int(m.max())), limit, radius, L.ptr(d_hoffs), total, int(per_item.max()),
                                              L.ptr(boxes), L.ptr(hits), L.stream_ptr())
        assert rc == 0, lib.prg_last_error()
        torch.cuda.synchronize()
        runs.append(hits.cpu().numpy())
        if prefilter:
            bx = boxes.cpu().numpy()
            assert np.all(bx[0] == SENTINEL) and np.all(bx[-1] == SENTINEL) and not np.any(bx[1:-1] == SENTINEL)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert np.array_equal(bits(d_pts.cpu().numpy()), bits(pts)) and np.array_equal(d_tab.cpu().numpy(), tab)
    h = runs[0]
    assert np.all(h[:LEAD] == SENTINEL) and np.all(h[h_offs[-1]:] == SENTINEL)            # nothing outside the node pairs
    assert not np.any(h[LEAD:h_offs[-1]] == SENTINEL)                                    # every node pair written
    return [h[h_offs[p]:h_offs[p + 1]] for p in range(len(items))]


def check_overlaps(L, items, radius, head=0, tail=0):
    """With and without the pre-filter, against the specification; -> per item the dense hits."""
    got = overlaps(L, items, radius, head, tail, prefilter=True)
    plain = overlaps(L, items, radius, head, tail, prefilter=False)
    for p, (a, ta, b, tb) in enumerate(items):
        want = dense_want(a, ta, b, tb, radius)
        assert got[p].shape == want.shape and np.array_equal(got[p], want), (p, np.argwhere(got[p] != want)[:4].tolist())
        assert np.array_equal(plain[p], want), (p, "no pre-filter", np.argwhere(plain[p] != want)[:4].tolist())
    return got


def item(rng, n, ms, mt, limit, shift=0.03):
    a = surface(rng, n)
    k = max(1, n - n // 8)
    b = a[rng.permutation(n)][:k] + rng.normal(0, 0.004, (k, 3))
    b[:, 0] += shift
    return a, PP.node_patches(a, nodes_of(rng, a, ms), limit)[1], b, PP.node_patches(b, nodes_of(rng, b, mt), limit)[1]


@pytest.mark.parametrize("limit", LIMITS)
def test_overlap_limits_sizes_and_nodes(L, limit):
    """Three items in one launch: clouds on both sides of 64 and 256 rows, node counts 1, 3, 64 and 65 (65 * 64 node pairs: more
    than one workgroup, the last one partly filled), patches from empty to 256 points."""
    rng = np.random.default_rng(100 + limit)
    items = [item(rng, 700, 65, 64, limit), item(rng, 257, 3, 65, limit), item(rng, 63, 1, 3, limit)]
    got = check_overlaps(L, items, 0.05)
    assert all((g[:, 0] > 0).any() and (g[:, 0] == 0).any() for g in got[:2])
    assert all(np.array_equal(g[:, 0] > 0, g[:, 1] > 0) for g in got)
    check_overlaps(L, items[1:], 0.0125, head=4, tail=3)


def test_overlap_none_one_all_and_the_strict_bound(L):
    """Hand-made patches on a power-of-two grid, radius 0.125: a pair of points at squared distance exactly radius*radius does
    not count, one grid step closer does."""
    g = 0.0625
    src = np.array([[0, 0, 0], [g, 0, 0], [0, g, 0], [g, g, 0], [8.0, 8.0, 8.0], [np.nan, 0, 0]], dtype=np.float64)
    tgt = np.array([[0, 0, 0], [g, 0, 0], [0, g, 0], [g, g, 0],           # patch 0: the source's patch 0 itself: all hit
                    [-0.125, 0, 0], [g + 0.125, g, 0],                    # patch 1: exactly radius from a source point each: none
                    [-g, 0, 0], [1.0, 1.0, 1.0],                          # patch 2: one point within reach of two source points
                    [8.0, 8.0, 8.0 + 0.125], [8.0, 8.0 + g, 8.0],         # patch 3: against source patch 1: one of two
                    [-0.125, 0, 0]], dtype=np.float64)                    # patch 4: its box exactly radius from source patch 0's
    n, k = len(src), len(tgt)
    ta = np.array([[0, 1, 2, 3], [4, 5, n, n], [n, n, n, n]], dtype=np.int32)
    tb = np.array([[0, 1, 2, 3], [4, 5, k, k], [6, 7, k, k], [8, 9, k, k], [10, k, k, k]], dtype=np.int32)
    got = check_overlaps(L, [(src, ta, tgt, tb)], 0.125)[0].reshape(3, 5, 2)
    assert got[0].tolist() == [[4, 4], [0, 0], [2, 1], [0, 0], [0, 0]]
    assert got[1].tolist() == [[0, 0], [0, 0], [0, 0], [1, 1], [0, 0]]
    assert (got[2] == 0).all()                                            # an empty patch overlaps nothing
    corr, hits, ov = PP.patch_overlaps_hip([(src, ta, tgt, tb)], 0.125)[0]
    assert corr.tolist() == [[0, 0], [0, 2], [1, 3]] and hits.tolist() == [[4, 4], [2, 1], [1, 1]]
    assert ov.tolist() == [1.0, (2 / 4 + 1 / 2) / 2, (1 / 2 + 1 / 2) / 2]


# ---- the Python layers ---------------------------------------------------------------------------------------------------------
def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def test_python_layers_match_the_specification():
    from pointreggpt_amd import geometry as G
    rng = np.random.default_rng(77)
    limit, radius = 12, 0.05
    pts = [surface(rng, n) for n in (300, 257, 0, 65)]
    pts[1] = pts[0][rng.permutation(300)][:257] + rng.normal(0, 0.004, (257, 3))
    pts[0][[3, 44]] = np.nan
    nds = [nodes_of(rng, pts[0][50:], 20), nodes_of(rng, pts[1], 17), nodes_of(rng, pts[3], 4), np.zeros((0, 3))]
    want = [PP.node_patches(p, q, limit) for p, q in zip(pts, nds)]
    for got, ref in zip(PP.node_patches_hip(list(zip(pts, nds)), limit), want):
        same(got, ref)
    # offsets that do not start at 0, device offsets, index_base / pad
    po, no = 2 + np.concatenate([[0], np.cumsum([len(p) for p in pts])]), 1 + np.concatenate([[0], np.cumsum([len(q) for q in nds])])
    P = D(np.concatenate([np.full((2, 3), POISON)] + pts + [np.full((3, 3), HUGE)]))
    N = D(np.concatenate([np.full((1, 3), POISON)] + nds + [np.full((2, 3), HUGE)]))
    base, pad = np.array([5, 6, 7, 8], np.int32), np.array([-1, -2, -3, -4], np.int32)
    assign, table, sizes = G.node_patches_ragged(P, D(po), N, no, limit, index_base=D(base), pad=D(pad))
    assert assign.shape == (len(P),) and table.shape == (no[-1] - no[0], limit) and (assign[:2] == -1).all() and (assign[-3:] == -1).all()
    assign, table, sizes = assign.cpu().numpy(), table.cpu().numpy(), sizes.cpu().numpy()
    for c in range(4):
        a, t, s = want[c]
        assert np.array_equal(assign[po[c]:po[c + 1]], a) and np.array_equal(sizes[no[c] - 1:no[c + 1] - 1], s)
        assert np.array_equal(table[no[c] - 1:no[c + 1] - 1], np.where(t < len(pts[c]), t + base[c], pad[c]))
    # two items: (cloud 0, cloud 1) and (cloud 2, cloud 3) — the second has an empty source and a target without nodes
    items = [(pts[0], want[0][1], pts[1], want[1][1]), (pts[2], want[2][1], pts[3], want[3][1])]
    refs = [PP.patch_overlaps(*it, radius) for it in items]
    assert len(refs[0][0]) > 0 and len(refs[1][0]) == 0
    for pre in (True, False):
        for got, ref in zip(PP.patch_overlaps_hip(items, radius, prefilter=pre), refs):
            same(got, ref)
