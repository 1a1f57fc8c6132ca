"""postprocess.node_patches / patch_overlaps / coarse_ground_truth — the numpy specifications of the patch kernels — against an
independent formulation: a dense float64 distance matrix with the same expression, a per-point scan for the nearest node,
np.lexsort per node for the order and Python sets for the hits.  Both sides use the same arithmetic, so every comparison is
exact."""
import numpy as np
import pytest

from pointreggpt_amd import postprocess as PP


def dense_d2(a, b):
    """(len(a), len(b)) squared distances, dx = b.x - a.x, products written out, summed left to right."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = b[None, :, 0] - a[:, None, 0], b[None, :, 1] - a[:, None, 1], b[None, :, 2] - a[:, None, 2]
        return dx * dx + dy * dy + dz * dz


def ref_node_patches(points, nodes, limit):
    points, nodes = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(nodes, np.float64).reshape(-1, 3)
    n, m = len(points), len(nodes)
    D = dense_d2(points, nodes)
    assign, d2 = np.full(n, -1, np.int32), np.full(n, np.inf)
    for i in range(n):
        for k in range(m):
            if D[i, k] < d2[i]:                          # strict: the lowest node row keeps a tie, a NaN never wins
                d2[i], assign[i] = D[i, k], k
    table, sizes = np.full((m, limit), n, np.int32), np.zeros(m, np.int32)
    for k in range(m):
        members = np.flatnonzero(assign == k)
        sizes[k] = len(members)
        members = members[np.lexsort((members, d2[members]))][:limit]
        table[k, :len(members)] = members
    return assign, table, sizes


def ref_patch_overlaps(a, ta, b, tb, radius):
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    W = dense_d2(a, b) < np.float64(radius) * np.float64(radius)
    corr, hits, overlap = [], [], []
    for s in range(len(ta)):
        pa = [int(i) for i in ta[s] if i != len(a)]
        for t in range(len(tb)):
            pb = [int(j) for j in tb[t] if j != len(b)]
            src = {i for i in pa for j in pb if W[i, j]}
            tgt = {j for i in pa for j in pb if W[i, j]}
            assert bool(src) == bool(tgt)
            if src:
                corr.append((s, t))
                hits.append((len(src), len(tgt)))
                overlap.append((np.float64(len(src)) / np.float64(len(pa)) + np.float64(len(tgt)) / np.float64(len(pb))) / 2)
    return (np.array(corr, np.int32).reshape(-1, 2), np.array(hits, np.int32).reshape(-1, 2), np.array(overlap, np.float64))


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def surface(rng, n, shift=0.0):
    p = rng.uniform(0, 1, (n, 3))
    p[:, 2] = 0.2 * np.sin(3 * p[:, 0]) + shift
    return p


REGIMES = {"most_truncated": (400, 10, 8), "none_truncated": (300, 20, 256), "limit_1": (200, 15, 1)}


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_node_patches_regimes(name):
    n, m, limit = REGIMES[name]
    rng = np.random.default_rng(len(name))
    pts = surface(rng, n)
    nodes = pts[rng.choice(n, m, replace=False)] + rng.normal(0, 0.01, (m, 3))
    got = PP.node_patches(pts, nodes, limit)
    same(got, ref_node_patches(pts, nodes, limit))
    truncated = (got[2] > limit).mean()
    assert {"most_truncated": truncated > 0.5, "none_truncated": truncated == 0, "limit_1": truncated > 0.5}[name]
    assert got[2].sum() == n and got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int32


def test_node_patches_many_empty_nodes():
    rng = np.random.default_rng(5)
    pts = surface(rng, 250)
    nodes = np.concatenate([pts[:6], rng.uniform(50, 60, (54, 3))])[rng.permutation(60)]
    got = PP.node_patches(pts, nodes, 16)
    same(got, ref_node_patches(pts, nodes, 16))
    assert (got[2] == 0).sum() >= 54 and (got[1][got[2] == 0] == 250).all()


def test_node_patches_ties_nan_and_empty_inputs():
    rng = np.random.default_rng(6)
    pts = surface(rng, 120)
    pts[40:80] = pts[7]                                  # forty-one copies of one point: equal d2, ordered by row
    pts[100] = [0.5, 0.25, 0.0]                          # exactly between nodes 1 and 3 (below): the lower node row wins
    pts[[3, 90]] = np.nan
    pts[91, 1] = np.nan
    nodes = np.concatenate([pts[[7]], [[0.25, 0.25, 0.0]], [[np.nan, 0.0, 0.0]], [[0.75, 0.25, 0.0]], pts[[20, 110]]])
    assign, table, sizes = got = PP.node_patches(pts, nodes, 8)
    same(got, ref_node_patches(pts, nodes, 8))
    assert assign[100] == 1 and (assign[[3, 90, 91]] == -1).all() and sizes[2] == 0 and sizes.sum() == 117
    assert list(table[0][:8]) == [7] + list(range(40, 47))            # row 7 and its copies, by row
    for limit in (1, 64):
        same(PP.node_patches(pts[:0], nodes, limit), ref_node_patches(pts[:0], nodes, limit))
        same(PP.node_patches(pts, nodes[:0], limit), ref_node_patches(pts, nodes[:0], limit))
    a, t, s = PP.node_patches(pts, nodes[:0], 4)
    assert (a == -1).all() and t.shape == (0, 4) and s.shape == (0,)
    a, t, s = PP.node_patches(pts[:0], nodes, 4)
    assert a.shape == (0,) and (t == 0).all() and t.shape == (6, 4) and (s == 0).all()
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError):
            PP.node_patches(pts, nodes, bad)


def two_clouds(seed, n=260, m=14, shift=0.03):
    rng = np.random.default_rng(seed)
    a = surface(rng, n)
    b = a[rng.permutation(n)][: n - 30] + rng.normal(0, 0.004, (n - 30, 3))
    b[:, 0] += shift
    return a, a[rng.choice(n, m, replace=False)], b, b[rng.choice(len(b), m + 3, replace=False)]


@pytest.mark.parametrize("limit,radius", [(6, 0.05), (256, 0.05), (1, 0.08), (12, 0.0125)])
def test_patch_overlaps_regimes(limit, radius):
    a, na, b, nb = two_clouds(limit)
    ta, tb = PP.node_patches(a, na, limit)[1], PP.node_patches(b, nb, limit)[1]
    got = PP.patch_overlaps(a, ta, b, tb, radius)
    want = ref_patch_overlaps(a, ta, b, tb, radius)
    same(got, want)
    assert len(got[0]) > 0 and got[2].dtype == np.float64 and (got[2] > 0).all() and (got[2] <= 1).all()
    same(PP.patch_overlaps(a, ta, b, tb, radius, chunk=1), want)      # the blocking changes nothing


def test_patch_overlaps_nan_empty_and_the_strict_bound():
    a, na, b, nb = two_clouds(9)
    a[[5, 17]] = np.nan
    b[11, 2] = np.nan
    na[2] = np.nan                                       # a node nobody is nearest to: an empty patch
    far = np.concatenate([nb, [[40.0, 40.0, 40.0]]])
    ta, tb = PP.node_patches(a, na, 10)[1], PP.node_patches(b, far, 10)[1]
    same(PP.patch_overlaps(a, ta, b, tb, 0.05), ref_patch_overlaps(a, ta, b, tb, 0.05))
    for args in ((a[:0], PP.node_patches(a[:0], na, 4)[1], b, PP.node_patches(b, nb, 4)[1]),
                 (a, PP.node_patches(a, na[:0], 4)[1], b, PP.node_patches(b, nb, 4)[1]),
                 (a, PP.node_patches(a, na, 4)[1], b[:0], PP.node_patches(b[:0], nb, 4)[1])):
        got = PP.patch_overlaps(*args, 0.05)
        same(got, ref_patch_overlaps(*args, 0.05))
        assert got[0].shape == (0, 2) and got[1].shape == (0, 2) and got[2].shape == (0,)
    # squared distance exactly radius*radius does not count; one grid step closer does
    src, tgt = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), np.array([[0.125, 0.0, 0.0], [1.0, 0.0625, 0.0]])
    t = np.array([[0, 1]], np.int32)
    corr, hits, ov = PP.patch_overlaps(src, t, tgt, t, 0.125)
    assert corr.tolist() == [[0, 0]] and hits.tolist() == [[1, 1]] and ov.tolist() == [0.5]
    with pytest.raises(ValueError):
        PP.patch_overlaps(src, t, tgt, t, 0.0)


@pytest.mark.parametrize("fine_level", [0, 1, 2])
def test_coarse_ground_truth_is_the_two_functions_per_cloud_and_item(fine_level):
    rng = np.random.default_rng(3)
    clouds = []
    for p in range(2):
        a = surface(rng, 500 + 40 * p) * 0.6
        clouds += [a, a[rng.permutation(len(a))][:450] + rng.normal(0, 0.002, (450, 3))]
    lens = [len(c) for c in clouds]
    pyr = PP.neighbor_pyramid(np.concatenate(clouds), lens, num_stages=3, voxel_size=0.025, radius=0.0625, neighbor_limits=[8, 8, 8])
    limit, radius = 16, 0.05
    got = PP.coarse_ground_truth(pyr, fine_level=fine_level, limit=limit, radius=radius)
    F, N = pyr["points"][fine_level], pyr["points"][-1]
    fo, no = np.concatenate([[0], np.cumsum(pyr["lengths"][fine_level])]), np.concatenate([[0], np.cumsum(pyr["lengths"][-1])])
    assert len(N) > 8 and got["table"].shape == (len(N), limit) and got["assign"].shape == (len(F),)
    local = []
    for c in range(4):
        a, t, s = ref_node_patches(F[fo[c]:fo[c + 1]], N[no[c]:no[c + 1]], limit)
        local.append(t)
        assert np.array_equal(got["assign"][fo[c]:fo[c + 1]], np.where(a >= 0, a + no[c], -1))
        assert np.array_equal(got["table"][no[c]:no[c + 1]], np.where(t < fo[c + 1] - fo[c], t + fo[c], len(F)))
        assert np.array_equal(got["sizes"][no[c]:no[c + 1]], s)
    assert got["corr_offsets"].tolist()[0] == 0 and len(got["corr_offsets"]) == 3 and got["corr_offsets"][-1] == len(got["node_corr"])
    for p in range(2):
        s, t = 2 * p, 2 * p + 1
        corr, hits, ov = ref_patch_overlaps(F[fo[s]:fo[s + 1]], local[s], F[fo[t]:fo[t + 1]], local[t], radius)
        rows = slice(got["corr_offsets"][p], got["corr_offsets"][p + 1])
        assert len(corr) > 0
        assert np.array_equal(got["node_corr"][rows], corr + [no[s], no[t]]) and got["node_corr"].dtype == np.int32
        assert np.array_equal(got["hits"][rows], hits) and got["overlap"][rows].tobytes() == ov.tobytes()
    if fine_level == 2:                                  # the nodes themselves: every node is its own patch
        assert np.array_equal(got["assign"], np.arange(len(N))) and (got["sizes"] == 1).all()
        assert np.array_equal(got["table"][:, 0], np.arange(len(N))) and (got["table"][:, 1:] == len(N)).all()
    with pytest.raises(ValueError):
        PP.coarse_ground_truth(pyr, fine_level=3, limit=limit, radius=radius)
