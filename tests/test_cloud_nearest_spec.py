"""The numpy specification of the nearest-neighbour comparison (postprocess.nearest, cloud_distance_metrics) on the CPU.
`nearest` is what prg_nearest_ragged_f64 must reproduce bit for bit (tests/test_gpu_cloud_nearest.py); here it is checked
against an independent implementation, scipy's cKDTree, and on the edge cases its definition names."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from pointreggpt_amd import postprocess as PP


def cloud(rng, n):
    return rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


@pytest.mark.parametrize("na,nb,chunk", [(1, 1, 1024), (7, 300, 1024), (300, 7, 64), (1500, 2100, 1024), (2100, 1500, 1000)])
def test_nearest_against_kdtree(na, nb, chunk):
    """Random points are distinct, so the nearest row is unique: equal indices.  The tree computes sqrt(dz^2 + dy^2 + dx^2)-like
    sums in its own order: each of the two additions and the square root round once (0.5 ulp each, the sum's error halved by
    the root), so the two distances agree to well within the 4 ulp allowed."""
    rng = np.random.default_rng(na * 10007 + nb)
    a, b = cloud(rng, na), cloud(rng, nb)
    d2, idx = PP.nearest(a, b, chunk=chunk)
    dist, ref = cKDTree(b).query(a, k=1)
    assert d2.dtype == np.float64 and idx.dtype == np.int32 and d2.shape == (na,) and idx.shape == (na,)
    assert np.array_equal(idx, ref)
    d = np.sqrt(d2)
    assert np.all(np.abs(d - dist) <= 4 * np.spacing(dist))
    # and d2 is literally the written-out expression at the returned row
    diff = b[idx] - a
    assert np.array_equal(d2, diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])


def test_ties_take_the_lowest_index():
    rng = np.random.default_rng(1)
    b = cloud(rng, 40)
    b[31] = b[5]
    b[17] = b[5]
    a = np.stack([b[5], b[5] + [0.0, 0.0, 1e-9], [9.0, 9.0, 9.0]])
    d2, idx = PP.nearest(a, b)
    assert idx[0] == 5 and idx[1] == 5 and d2[0] == 0.0
    # two candidates at the same distance on either side of the query
    d2, idx = PP.nearest(np.zeros((1, 3)), np.array([[3.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0]]))
    assert idx[0] == 1 and d2[0] == 1.0
    # a cloud against itself: zero, and the row's own first duplicate
    d2, idx = PP.nearest(b, b)
    want = np.arange(40)
    want[[17, 31]] = 5
    assert np.array_equal(idx, want) and np.all(d2 == 0.0)


def test_empty_clouds():
    rng = np.random.default_rng(2)
    a = cloud(rng, 9)
    d2, idx = PP.nearest(a, np.zeros((0, 3)))
    assert np.all(np.isposinf(d2)) and np.all(idx == -1) and len(d2) == 9
    d2, idx = PP.nearest(np.zeros((0, 3)), a)
    assert d2.shape == (0,) and idx.shape == (0,) and d2.dtype == np.float64 and idx.dtype == np.int32
    d2, idx = PP.nearest(np.zeros((0, 3)), np.zeros((0, 3)))
    assert d2.shape == (0,) and idx.shape == (0,)


def test_nan_rows_never_win():
    rng = np.random.default_rng(3)
    a, b = cloud(rng, 20), cloud(rng, 30)
    a[4, 1] = np.nan
    b[0] = np.nan                               # would be argmin's pick if NaN were not replaced
    b[12, 2] = np.nan
    d2, idx = PP.nearest(a, b)
    assert np.isposinf(d2[4]) and idx[4] == -1
    keep = np.array([j for j in range(30) if j not in (0, 12)])
    d2_ref, idx_ref = PP.nearest(np.delete(a, 4, axis=0), b[keep])
    assert np.array_equal(np.delete(d2, 4), d2_ref) and np.array_equal(np.delete(idx, 4), keep[idx_ref])
    d2, idx = PP.nearest(a, np.full((3, 3), np.nan))
    assert np.all(np.isposinf(d2)) and np.all(idx == -1)


def test_overflowing_distances_leave_no_neighbour():
    d2, idx = PP.nearest(np.array([[1e200, 0, 0], [0.0, 0, 0]]), np.array([[-1e200, 0, 0], [0.0, 0, 1.0]]))
    assert np.isposinf(d2[0]) and idx[0] == -1 and d2[1] == 1.0 and idx[1] == 1


def test_metrics_by_hand():
    """a = (0,0,0), (1,0,0), (5,0,0); b = (0,0,0), (1,0,2).  Squared distances a -> b: to b0 0, 1, 25; to b1 5, 4, 20, so
    d2_ab = 0, 1, 20 at rows 0, 0, 1.  b -> a: b0 is a0; b1 is 5, 4, 20 away, so d2_ba = 0, 4 at rows 0, 1."""
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [5.0, 0, 0]])
    b = np.array([[0.0, 0, 0], [1.0, 0, 2.0]])
    d2_ab, i_ab = PP.nearest(a, b)
    d2_ba, i_ba = PP.nearest(b, a)
    assert d2_ab.tolist() == [0.0, 1.0, 20.0] and i_ab.tolist() == [0, 0, 1]
    assert d2_ba.tolist() == [0.0, 4.0] and i_ba.tolist() == [0, 1]
    m = PP.cloud_distance_metrics(d2_ab, d2_ba, thresholds=(0.5, 1.0, 2.0, 10.0))
    s20 = np.sqrt(20.0)
    assert m["n_a"] == 3 and m["n_b"] == 2 and m["empty"] is False
    assert m["chamfer"] == ((0.0 + 1.0 + s20) / 3 + (0.0 + 2.0) / 2) / 2
    assert m["hausdorff"] == s20
    both = np.array([0.0, 1.0, s20, 0.0, 2.0])                      # sorted: 0, 0, 1, 2, sqrt20
    assert m["p50"] == 1.0
    assert m["p95"] == np.percentile(both, 95) and m["p99"] == np.percentile(both, 99)
    assert m["p95"] == pytest.approx(2.0 + 0.8 * (s20 - 2.0), rel=1e-12)
    assert m["within"] == {0.5: 0.4, 1.0: 0.6, 2.0: 0.8, 10.0: 1.0}


def test_metrics_default_thresholds_and_identical_clouds():
    z = np.zeros(5)
    m = PP.cloud_distance_metrics(z, z)
    assert list(m["within"]) == [1e-4, 1e-3, 0.0125, 0.0375] and PP.DISTANCE_THRESHOLDS == (1e-4, 1e-3, 0.0125, 0.0375)
    assert m["chamfer"] == 0.0 and m["hausdorff"] == 0.0 and m["p99"] == 0.0 and all(v == 1.0 for v in m["within"].values())
    m = PP.cloud_distance_metrics(np.array([1e-10, 4e-6]), np.array([1e-4]))         # d = 1e-5, 2e-3, 1e-2
    assert m["within"][1e-4] == pytest.approx(1 / 3) and m["within"][1e-3] == pytest.approx(1 / 3)
    assert m["within"][0.0125] == 1.0


@pytest.mark.parametrize("na,nb", [(0, 4), (4, 0), (0, 0)])
def test_metrics_of_an_empty_cloud(na, nb):
    rng = np.random.default_rng(5)
    a, b = cloud(rng, na), cloud(rng, nb)
    m = PP.cloud_distance_metrics(PP.nearest(a, b)[0], PP.nearest(b, a)[0])
    assert m["empty"] is True and m["n_a"] == na and m["n_b"] == nb
    for k in ("chamfer", "hausdorff", "p50", "p95", "p99"):
        assert np.isnan(m[k])
    assert len(m["within"]) == 4 and all(np.isnan(v) for v in m["within"].values())
