"""`postprocess.radius_neighbors` and `postprocess.neighbor_pyramid`, the numpy specifications of the neighbour-table kernel and of
the KPConv pyramid, against a KD-tree on the CPU.

Random clouds in the box [-2,2] x [-2,2] x [0,4] (64 m^3), as tests/test_radius_pairs_spec.py: at 1025 rows a sphere of radius 0.5
holds some 8 points, so limit 4 truncates most rows, limit 16 a few and limit 64 none; against 300 rows a tenth of the query rows
find nothing.  The tree tests `<=` in its own arithmetic, the specification `<` on products summed left to right: they can only
disagree on a squared distance within rounding of r^2, and the test asserts that no distance lies within 1e-9 relative of it."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from pointreggpt_amd import postprocess as PP

R = 0.5
SEED = 20
CASES = [(1025, 1025, 4), (1025, 1025, 16), (513, 300, 64)]


def cloud(rng, n):
    return rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


def case(na, nb, limit):
    rng = np.random.default_rng(SEED + limit)
    return cloud(rng, na), cloud(rng, nb)


def tree_table(a, b, r, limit):
    """Ball query, candidates in ascending j, then a STABLE sort by the squared distance: (d2, j) order."""
    idx = np.full((len(a), limit), len(b), dtype=np.int32)
    count = np.zeros(len(a), dtype=np.int32)
    for i, js in enumerate(cKDTree(b).query_ball_point(a, r)):
        js = np.sort(np.asarray(js, dtype=np.int64))
        dx, dy, dz = b[js, 0] - a[i, 0], b[js, 1] - a[i, 1], b[js, 2] - a[i, 2]
        js = js[np.argsort(dx * dx + dy * dy + dz * dz, kind="stable")]
        count[i] = len(js)
        idx[i, :min(limit, len(js))] = js[:limit]
    return idx, count


@pytest.mark.parametrize("na,nb,limit", CASES)
def test_against_the_kd_tree(na, nb, limit):
    a, b = case(na, nb, limit)
    d2 = ((b[None] - a[:, None]) ** 2).sum(-1)
    assert not np.any(np.abs(d2 - R * R) <= 1e-9 * R * R)            # no distance on the boundary: < and <= agree
    idx, count = PP.radius_neighbors(a, b, R, limit)
    assert idx.dtype == np.int32 and idx.shape == (na, limit) and count.dtype == np.int32 and count.shape == (na,)
    want, wcount = tree_table(a, b, R, limit)
    assert np.array_equal(count, wcount)
    assert np.array_equal(idx, want)


def test_the_cases_truncate_pad_and_leave_rows_empty():
    over, empty = {}, {}
    for na, nb, limit in CASES:
        _, count = PP.radius_neighbors(*case(na, nb, limit), R, limit)
        over[limit], empty[limit] = int((count > limit).sum()), int((count == 0).sum())
    assert over[4] > 512 and empty[4] >= 1                           # most rows over the limit, some row without a match
    assert 0 < over[16] < 100                                        # a few rows over the limit, nearly all padded
    assert over[64] == 0 and empty[64] > 10                          # none over the limit, many empty rows


def test_rows_are_ordered_by_distance_and_padded_at_the_end():
    a, b = case(1025, 1025, 16)
    idx, count = PP.radius_neighbors(a, b, R, 16)
    for i in range(len(a)):
        k = min(16, count[i])
        assert np.all(idx[i, :k] < len(b)) and np.all(idx[i, k:] == len(b))
        d2 = ((b[idx[i, :k]] - a[i]) ** 2).sum(-1)
        assert np.all(np.diff(d2) >= 0) and np.all(d2 < R * R)
    full, _ = PP.radius_neighbors(a, b, R, 64)
    assert np.array_equal(full[:, :16], idx)                         # a smaller limit is a prefix


def test_limit_one_is_the_nearest_row():
    a, b = case(513, 300, 64)
    idx, count = PP.radius_neighbors(a, b, R, 1)
    d2, near = PP.nearest(a, b)
    assert idx.shape == (513, 1)
    assert np.array_equal(idx[:, 0], np.where(d2 < R * R, near, 300))
    assert np.array_equal(count > 0, d2 < R * R)


def test_duplicates_are_ordered_by_j_and_the_bound_is_strict():
    b = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [0.5, 0, 0], [0.0, 0.5, 0], [0.0, 0, 0], [0.25, 0, 0], [-0.25, 0, 0]])
    a = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    idx, count = PP.radius_neighbors(a, b, 0.5, 6)                   # 0.25 < 0.25 is false: rows 3 and 4 are out for i = 0
    assert idx.tolist() == [[0, 2, 5, 6, 7, 8], [1, 8, 8, 8, 8, 8]] and count.tolist() == [5, 1]
    idx, count = PP.radius_neighbors(a, b, 0.5, 2)
    assert idx.tolist() == [[0, 2], [1, 8]] and count.tolist() == [5, 1]
    q, cand = np.zeros((1, 3)), np.array([[0.5, 0, 0], [0, np.nextafter(0.5, 0), 0], [0, 0, -0.5]])
    idx, count = PP.radius_neighbors(q, cand, 0.5, 2)                # exactly at the radius: out; one ulp inside: in
    assert idx.tolist() == [[1, 3]] and count.tolist() == [1]
    idx, count = PP.radius_neighbors(q, cand, np.nextafter(0.5, 1.0), 4)
    assert idx.tolist() == [[1, 0, 2, 3]] and count.tolist() == [3]  # the two at 0.25 exactly: by j, after the nearer one


def test_nan_rows_never_match_and_are_never_matched():
    a, b = case(513, 300, 64)
    a, b = a.copy(), b.copy()
    clean, _ = PP.radius_neighbors(a, b, R, 64)
    a[3, 0] = a[100, 1] = a[512, 2] = np.nan
    b[0] = np.nan
    b[150, 1] = np.nan
    idx, count = PP.radius_neighbors(a, b, R, 64)
    assert np.all(idx[[3, 100, 512]] == 300) and np.all(count[[3, 100, 512]] == 0)
    assert not np.isin(idx, [0, 150]).any()
    for i in range(len(a)):
        if i not in (3, 100, 512):                                   # every other row: as before without the NaN candidates
            kept = [j for j in clean[i] if j not in (0, 150, 300)]
            assert idx[i, :len(kept)].tolist() == kept and np.all(idx[i, len(kept):] == 300)
    idx, count = PP.radius_neighbors(np.full((4, 3), np.nan), b, R, 3)
    assert np.all(idx == 300) and np.all(count == 0)


def test_empty_clouds():
    rng = np.random.default_rng(SEED)
    c, e = cloud(rng, 65), np.zeros((0, 3))
    idx, count = PP.radius_neighbors(e, c, R, 5)
    assert idx.shape == (0, 5) and idx.dtype == np.int32 and count.shape == (0,) and count.dtype == np.int32
    idx, count = PP.radius_neighbors(c, e, R, 5)
    assert idx.shape == (65, 5) and np.all(idx == 0) and np.all(count == 0)        # all pads, and the pad is 0
    idx, count = PP.radius_neighbors(e, e, R, 5)
    assert idx.shape == (0, 5) and count.shape == (0,)
    idx, count = PP.radius_neighbors(c, c + 100.0, R, 5)                          # nothing within the radius
    assert np.all(idx == 65) and np.all(count == 0)


@pytest.mark.parametrize("radius,limit", [(0.5, 0), (0.5, -3), (0.0, 4), (-1.0, 4), (float("inf"), 4), (float("nan"), 4)])
def test_bad_arguments_raise(radius, limit):
    rng = np.random.default_rng(SEED)
    with pytest.raises(ValueError):
        PP.radius_neighbors(cloud(rng, 4), cloud(rng, 4), radius, limit)


# ---- the pyramid -------------------------------------------------------------------------------------------------------------
def voxel_like(rng, n):
    """A 2.5 cm grid surface patch and the same patch with a 1 cm jitter: what a finished pair looks like at loader radii."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a, b[rng.permutation(n)]


@pytest.fixture(scope="module")
def pyramid():
    rng = np.random.default_rng(25)
    (a, _), (b, _) = voxel_like(rng, 1500), voxel_like(rng, 700)
    pts = np.concatenate([a, b])
    return pts, PP.neighbor_pyramid(pts, [1500, 700], 3, 0.025, 0.0625, (38, 36, 36))


def test_pyramid_levels(pyramid):
    pts, pyr = pyramid
    assert sorted(pyr) == ["counts", "lengths", "neighbors", "points", "subsampling", "upsampling"]
    assert sorted(pyr["counts"]) == ["neighbors", "subsampling", "upsampling"]
    assert len(pyr["points"]) == len(pyr["lengths"]) == len(pyr["neighbors"]) == 3
    assert len(pyr["subsampling"]) == len(pyr["upsampling"]) == 2
    assert pyr["points"][0] is not None and np.array_equal(pyr["points"][0], pts) and pyr["lengths"][0].tolist() == [1500, 700]
    sizes = [len(p) for p in pyr["points"]]
    assert sizes[0] > sizes[1] > sizes[2] > 0                        # level sizes strictly decrease
    for l in range(3):
        assert pyr["lengths"][l].sum() == sizes[l] and pyr["lengths"][l].shape == (2,)
    for l in range(2):                                               # level l+1 = the grid of every cloud of level l, re-stacked
        o = np.concatenate([[0], np.cumsum(pyr["lengths"][l])])
        want = np.concatenate([PP.voxel_down_sample(pyr["points"][l][o[c]:o[c + 1]], 0.025 * 2 ** (l + 1)) for c in range(2)])
        assert np.array_equal(pyr["points"][l + 1], want)


def test_pyramid_tables(pyramid):
    _, pyr = pyramid
    limits = (38, 36, 36)
    offs = [np.concatenate([[0], np.cumsum(n)]) for n in pyr["lengths"]]
    sizes = [len(p) for p in pyr["points"]]

    def check(table, count, q_level, c_level, limit, r):
        assert table.dtype == np.int32 and table.shape == (sizes[q_level], limit) and count.shape == (sizes[q_level],)
        pad = sizes[c_level]
        assert np.all((table >= 0) & (table <= pad))                 # every index below the pad or equal to it
        for c in range(2):                                           # no index crosses a cloud
            rows = table[offs[q_level][c]:offs[q_level][c + 1]]
            real = rows[rows != pad]
            assert np.all((real >= offs[c_level][c]) & (real < offs[c_level][c + 1]))
            a = pyr["points"][q_level][offs[q_level][c]:offs[q_level][c + 1]]
            b = pyr["points"][c_level][offs[c_level][c]:offs[c_level][c + 1]]
            idx, cnt = PP.radius_neighbors(a, b, r, limit)
            assert np.array_equal(rows, np.where(idx < len(b), idx + offs[c_level][c], pad))
            assert np.array_equal(count[offs[q_level][c]:offs[q_level][c + 1]], cnt)

    for l in range(3):
        r = 0.0625 * 2 ** l
        check(pyr["neighbors"][l], pyr["counts"]["neighbors"][l], l, l, limits[l], r)
        assert np.array_equal(pyr["neighbors"][l][:, 0], np.arange(sizes[l]))     # a row's nearest neighbour is the row itself
        if l < 2:
            check(pyr["subsampling"][l], pyr["counts"]["subsampling"][l], l + 1, l, limits[l], r)
            check(pyr["upsampling"][l], pyr["counts"]["upsampling"][l], l, l + 1, limits[l + 1], 2 * r)
            assert np.all(pyr["counts"]["subsampling"][l] > 0) and np.all(pyr["counts"]["upsampling"][l] > 0)


def test_pyramid_of_one_stage_and_bad_arguments():
    rng = np.random.default_rng(SEED)
    c = cloud(rng, 65)
    pyr = PP.neighbor_pyramid(c, [40, 25], 1, 0.025, R, [5])
    assert len(pyr["points"]) == 1 and pyr["subsampling"] == [] and pyr["upsampling"] == []
    assert pyr["neighbors"][0].shape == (65, 5)
    with pytest.raises(ValueError):
        PP.neighbor_pyramid(c, [40, 24], 1, 0.025, R, [5])           # lengths do not add up
    with pytest.raises(ValueError):
        PP.neighbor_pyramid(c, [40, 25], 2, 0.025, R, [5])           # one limit per stage
    with pytest.raises(ValueError):
        PP.neighbor_pyramid(c, [40, 25], 1, 0.025, R, [0])
