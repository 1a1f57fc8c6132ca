"""`postprocess.radius_pairs`, the numpy specification of the radius-pairs kernels, against a KD-tree on the CPU.

Random clouds in the box [-2,2] x [-2,2] x [0,4] (64 m^3).  At 1025 rows that is 16 points / m^3; a sphere of radius 0.5 holds
0.52 m^3, so a query row has some 8 matches.  The tree tests `<=` in its own arithmetic, the specification `<` on products
summed left to right: the two can only disagree on a squared distance within rounding of r^2, and the test asserts that the seed
below puts none within 1e-9 relative of it."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from pointreggpt_amd import postprocess as PP

SIZES = [1, 2, 65, 257, 1025]
R = 0.5
SEED = 20


def cloud(rng, n):
    return rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


def clouds():
    rng = np.random.default_rng(SEED)
    return {n: cloud(rng, n) for n in SIZES}


def tree_sets(a, b, r):
    return [set(js) for js in cKDTree(b).query_ball_point(a, r)]


def rows_as_sets(corr, n):
    out = [set() for _ in range(n)]
    for i, j in corr.tolist():
        out[i].add(j)
    return out


@pytest.mark.parametrize("na", SIZES)
@pytest.mark.parametrize("nb", SIZES)
def test_against_the_kd_tree(na, nb):
    c = clouds()
    a, b = c[na], c[nb][::-1].copy()                                 # another cloud also when na == nb
    d2 = ((b[None] - a[:, None]) ** 2).sum(-1)
    assert not np.any(np.abs(d2 - R * R) <= 1e-9 * R * R)            # no distance on the boundary: < and <= agree
    corr = PP.radius_pairs(a, b, R)
    assert corr.dtype == np.int32 and corr.ndim == 2 and corr.shape[1] == 2
    assert rows_as_sets(corr, na) == tree_sets(a, b, R)
    assert len(corr) == sum(len(s) for s in tree_sets(a, b, R))     # no row twice


def test_the_spec_finds_matches():
    c = clouds()
    corr = PP.radius_pairs(c[1025], c[257], R)
    assert len(corr) > 0
    per_row = len(PP.radius_pairs(c[1025], c[1025][::-1].copy(), R)) / 1025.0
    assert 4.0 < per_row < 12.0                                      # the docstring's estimate of 8


def test_rows_are_ordered_by_i_then_j():
    c = clouds()
    corr = PP.radius_pairs(c[1025], c[257], R)
    key = corr[:, 0].astype(np.int64) * 257 + corr[:, 1]
    assert np.all(np.diff(key) > 0)                                  # strictly: ordered and unique


@pytest.mark.parametrize("chunk", [1, 7, 64, 256, 1024, 5000])
def test_chunking_changes_nothing(chunk):
    c = clouds()
    want = PP.radius_pairs(c[257], c[1025], R)
    assert np.array_equal(PP.radius_pairs(c[257], c[1025], R, chunk=chunk), want)


def test_empty_inputs():
    c = clouds()
    e = np.zeros((0, 3))
    for a, b in ((e, c[65]), (c[65], e), (e, e)):
        corr = PP.radius_pairs(a, b, R)
        assert corr.shape == (0, 2) and corr.dtype == np.int32
    far = PP.radius_pairs(c[65], c[65] + 100.0, R)                   # nothing within the radius
    assert far.shape == (0, 2) and far.dtype == np.int32


def test_nan_rows_never_match():
    c = clouds()
    a, b = c[257].copy(), c[1025].copy()
    clean = PP.radius_pairs(a, b, R)
    a[3, 0] = a[100, 1] = a[256, 2] = np.nan
    b[0] = np.nan
    b[500, 1] = np.nan
    corr = PP.radius_pairs(a, b, R)
    assert not np.isin(corr[:, 0], [3, 100, 256]).any() and not np.isin(corr[:, 1], [0, 500]).any()
    keep = ~np.isin(clean[:, 0], [3, 100, 256]) & ~np.isin(clean[:, 1], [0, 500])
    assert np.array_equal(corr, clean[keep])                         # every other row as before
    assert PP.radius_pairs(np.full((4, 3), np.nan), b, R).shape == (0, 2)


def test_duplicates_and_the_strict_bound():
    b = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [0.5, 0, 0], [0.0, 0.5, 0]])
    a = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    corr = PP.radius_pairs(a, b, 0.5)                                # 0.25 < 0.25 is false: rows 3 and 4 are out for i = 0
    assert corr.tolist() == [[0, 0], [0, 2], [1, 1]]
    assert PP.radius_pairs(a, b, np.nextafter(0.5, 1.0)).tolist() == [[0, 0], [0, 2], [0, 3], [0, 4], [1, 1], [1, 3]]


@pytest.mark.parametrize("na,nb", [(1025, 257), (257, 1025), (65, 2), (1, 1025)])
def test_consistent_with_nearest(na, nb):
    """A row has matches iff `nearest` gives it d2 < r*r, and its nearest row is among its j."""
    c = clouds()
    a, b = c[na], c[nb][::-1].copy()
    a = a.copy()
    a[0] = np.nan
    d2, idx = PP.nearest(a, b)
    corr = PP.radius_pairs(a, b, R)
    sets = rows_as_sets(corr, na)
    has = np.array([len(s) > 0 for s in sets])
    assert np.array_equal(has, d2 < R * R)
    assert all(int(idx[i]) in sets[i] for i in np.flatnonzero(has))
    assert not has[0]
