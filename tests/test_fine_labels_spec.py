"""The fine-level ground truth's numpy specification (postprocess.patch_corr_labels, select_node_corr, fine_ground_truth) against an
independent formulation: Python loops over the slots, one dense distance matrix per pair, sets of matched slots.  No GPU."""
import numpy as np
import pytest

from pointreggpt_amd import postprocess as PP

KW = dict(num_stages=3, voxel_size=0.025, radius=0.0625, neighbor_limits=(20, 20, 20))
LIMIT, RADIUS = 8, 0.05


def labels_by_loops(points, table, pairs, radius):
    points, table = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(table)
    n, (m, K) = len(points), table.shape
    out = np.zeros((len(pairs), K + 1, K + 1), dtype=bool)
    r2 = np.float64(radius) * np.float64(radius)
    for s, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        if not (0 <= a < m and 0 <= b < m):
            continue
        us = [u for u in range(K) if 0 <= table[a, u] < n]
        vs = [v for v in range(K) if 0 <= table[b, v] < n]
        if us and vs:
            A, B = points[table[a, us]], points[table[b, vs]]
            with np.errstate(invalid="ignore", over="ignore"):
                d = B[None, :, :] - A[:, None, :]
                d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        matched = {(u, v) for x, u in enumerate(us) for y, v in enumerate(vs) if d2[x, y] < r2}
        for u, v in matched:
            out[s, u, v] = True
        for u in set(us) - {u for u, _ in matched}:
            out[s, u, K] = True
        for v in set(vs) - {v for _, v in matched}:
            out[s, K, v] = True
    return out


def check(points, table, pairs, radius):
    got = PP.patch_corr_labels(points, table, pairs, radius)
    want = labels_by_loops(points, table, pairs, radius)
    assert got.dtype == np.bool_ and got.shape == want.shape and np.array_equal(got, want)
    return got


def test_full_partial_empty_patches_pads_mid_row_same_patch_and_out_of_range_pairs():
    rng = np.random.default_rng(7)
    n, K = 90, 6
    pts = rng.uniform(0, 0.12, (n, 3))
    table = np.full((7, K), n, dtype=np.int32)
    table[0] = rng.permutation(n)[:K]                                  # full
    table[1, :3] = rng.permutation(n)[:3]                              # partial, a prefix
    table[2, [1, 4]] = [5, 17]                                         # pads in the middle of the row
    table[3] = rng.permutation(n)[:K]
    table[4, [0, 5]] = [3, 88]
    table[4, 2] = -1                                                   # a pad that is not n
    table[6] = rng.permutation(n)[:K]                                  # row 5 stays empty
    pairs = np.array([[0, 3], [1, 2], [2, 4], [5, 0], [0, 5], [5, 5], [0, 0], [6, 6], [7, 0], [0, -1], [3, 6], [100, 100]],
                     dtype=np.int32)
    got = check(pts, table, pairs, 0.05)
    K1 = K + 1
    assert got[:, :K, :K].any() and got[:, :K, K].any() and got[:, K, :K].any() and not got[:, K, K].any()
    assert not got[5].any()                                            # two empty patches: nobody is valid, not even for the slack
    assert got[3, K, :K].all() and not got[3, :K].any()                # empty against full: every target point is slack
    assert got[4, :K, K].all() and not got[4, K].any()                 # full against empty: every source point is slack
    assert np.array_equal(got[6, :K, :K], got[6, :K, :K].T) and got[6, :K, :K].diagonal().all()     # a == b
    assert not got[8].any() and not got[9].any() and not got[11].any() # out-of-range pair rows: two empty patches
    assert got.shape == (len(pairs), K1, K1)
    for s in range(len(pairs)):                                        # a valid slot is matched or slack, never both
        assert not (got[s, :K, :K].any(1) & got[s, :K, K]).any() and not (got[s, :K, :K].any(0) & got[s, K, :K]).any()


def test_nan_point_in_a_valid_slot_matches_nothing_and_is_slack():
    pts = np.array([[0, 0, 0], [0.01, 0, 0], [np.nan, 0, 0], [0, 0.01, 0]], dtype=np.float64)
    table = np.array([[0, 2, 4], [1, 2, 3]], dtype=np.int32)
    got = check(pts, table, np.array([[0, 1], [1, 0], [0, 0]], dtype=np.int32), 0.05)
    assert got[0, 1, 3] and got[0, 3, 1] and not got[0, 1, :3].any() and not got[0, :3, 1].any()
    assert not got[0, 2].any() and not got[0, 3, 2]                    # entry 4 = len(points): the pad slot of patch 0
    assert got[2, 1, 3] and got[2, 3, 1] and got[2, 0, 0] and not got[2, 1, 1]      # a NaN point does not even match itself


def test_limit_one_and_no_pairs_and_bad_arguments():
    pts = np.array([[0, 0, 0], [0.03, 0, 0], [1, 1, 1]], dtype=np.float64)
    table = np.array([[0], [1], [2], [3]], dtype=np.int32)
    got = check(pts, table, np.array([[0, 1], [0, 2], [3, 0], [0, 3]], dtype=np.int32), 0.05)
    assert got.tolist() == [[[True, False], [False, False]], [[False, True], [True, False]], [[False, False], [True, False]],
                            [[False, True], [False, False]]]
    empty = PP.patch_corr_labels(pts, table, np.zeros((0, 2), dtype=np.int32), 0.05)
    assert empty.shape == (0, 2, 2) and empty.dtype == np.bool_
    assert PP.patch_corr_labels(pts, np.zeros((0, 5), np.int32), np.zeros((0, 2), np.int32), 0.05).shape == (0, 6, 6)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            PP.patch_corr_labels(pts, table, np.zeros((1, 2), np.int32), bad)
    for k in (0, 257):
        with pytest.raises(ValueError):
            PP.patch_corr_labels(pts, np.zeros((2, k), np.int32), np.zeros((1, 2), np.int32), 0.05)


def test_a_pair_at_exactly_the_radius_is_no_match_and_one_ulp_inside_is():
    r = 0.5                                                            # exactly representable, and so is r * r
    pts = np.array([[0, 0, 0], [r, 0, 0], [np.nextafter(r, 0), 0, 0], [0, 0, -r], [0, np.nextafter(r, 1), 0]], dtype=np.float64)
    table = np.array([[0, 5], [1, 2], [3, 4]], dtype=np.int32)
    got = check(pts, table, np.array([[0, 1], [1, 0], [0, 2]], dtype=np.int32), r)
    assert got[0, :2, :2].tolist() == [[False, True], [False, False]] and got[0, 2].tolist() == [True, False, False]
    assert got[1, :2, :2].tolist() == [[False, False], [True, False]] and got[1, :, 2].tolist() == [True, False, False]
    assert not got[2, :2, :2].any() and got[2, 0, 2] and got[2, 2].tolist() == [True, True, False]


def select_by_loops(overlap, co, keys, min_overlap, num_targets):
    rows, so = [], [0]
    for p in range(len(co) - 1):
        cand = [r for r in range(co[p], co[p + 1]) if overlap[r] > min_overlap]
        if len(cand) > num_targets:
            cand = sorted(sorted(cand, key=lambda r: (keys[r], r))[:num_targets])
        rows += cand
        so.append(len(rows))
    return np.asarray(rows, dtype=np.int64), np.asarray(so, dtype=np.int64)


def test_select_node_corr_cases():
    #          item 0: 3 candidates of 5   | item 1: none above | item 2: no rows | item 3: 6 candidates, equal keys among them
    overlap = np.array([0.5, 0.1, 0.30000001, 0.05, 0.9, 0.1, 0.02, 0.4, 0.4, 0.4, 0.4, 0.11, 0.7, 0.1])
    co = np.array([0, 5, 7, 7, 14], dtype=np.int64)
    keys = np.array([0.9, 0.0, 0.1, 0.0, 0.5, 0.0, 0.0, 0.25, 0.75, 0.25, 0.25, 0.8, 0.1, 0.0])
    rows, so = PP.select_node_corr(overlap, co, keys, min_overlap=0.1, num_targets=4)
    assert rows.dtype == np.int64 and so.dtype == np.int64
    assert rows.tolist() == [0, 2, 4, 7, 9, 10, 12] and so.tolist() == [0, 3, 3, 3, 7]
    # overlap == min_overlap is excluded (rows 1, 5, 13); fewer candidates than num_targets keeps all (item 0); equal keys 0.25 at
    # rows 7, 9, 10 go by row: with num_targets=3 the kept ones are key 0.1 (row 12) and the two lowest rows of the tie
    rows, so = PP.select_node_corr(overlap, co, keys, min_overlap=0.1, num_targets=3)
    assert rows.tolist() == [0, 2, 4, 7, 9, 12] and so.tolist() == [0, 3, 3, 3, 6]
    rows, so = PP.select_node_corr(overlap, co, keys, min_overlap=0.1, num_targets=1)
    assert rows.tolist() == [2, 12] and so.tolist() == [0, 1, 1, 1, 2]
    rng = np.random.default_rng(3)
    for _ in range(20):
        sizes = rng.integers(0, 12, size=5)
        co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        ov = rng.choice([0.0, 0.1, 0.2, 0.3, 0.6], size=co[-1])
        ky = rng.choice([0.1, 0.2, 0.3, 0.4], size=co[-1])               # many ties
        for k in (1, 3, 50):
            got, want = PP.select_node_corr(ov, co, ky, min_overlap=0.1, num_targets=k), select_by_loops(ov, co, ky, 0.1, k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    e_rows, e_so = PP.select_node_corr(np.zeros(0), np.zeros(3, np.int64), np.zeros(0), min_overlap=0.1, num_targets=2)
    assert e_rows.shape == (0,) and e_rows.dtype == np.int64 and e_so.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        PP.select_node_corr(overlap, co, keys, min_overlap=0.1, num_targets=0)


def voxel_like(rng, n):
    """tests/test_gpu_coarse_ground_truth.py's clouds: a 2.5 cm grid surface patch and the same patch with a 1 cm jitter."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a, b[rng.permutation(n)][: n - n // 10]


@pytest.fixture(scope="module")
def pyramid():
    rng = np.random.default_rng(31)
    clouds = [c for n in (620, 577) for c in voxel_like(rng, n)]
    pts32 = np.concatenate(clouds).astype(np.float32)
    return PP.neighbor_pyramid(pts32, [len(c) for c in clouds], KW["num_stages"], KW["voxel_size"], KW["radius"],
                               KW["neighbor_limits"])


@pytest.mark.parametrize("fine_level", [0, 1, 2])
def test_fine_ground_truth_is_the_two_functions_composed(pyramid, fine_level):
    gt = PP.coarse_ground_truth(pyramid, fine_level=fine_level, limit=LIMIT, radius=RADIUS)
    P = len(gt["overlap"])
    keys = np.random.default_rng(100 + fine_level).random(P)
    out = PP.fine_ground_truth(pyramid, gt, fine_level=fine_level, radius=RADIUS, keys=keys, min_overlap=0.3, num_targets=64)
    assert sorted(out) == ["labels", "node_corr", "rows", "sel_offsets", "src_mask", "src_table", "tgt_mask", "tgt_table"]
    rows, so = PP.select_node_corr(gt["overlap"], gt["corr_offsets"], keys, min_overlap=0.3, num_targets=64)
    fine = np.asarray(pyramid["points"][fine_level], dtype=np.float64)
    corr = gt["node_corr"][rows]
    assert np.array_equal(out["rows"], rows) and np.array_equal(out["sel_offsets"], so)
    assert out["node_corr"].dtype == np.int32 and np.array_equal(out["node_corr"], corr)
    assert out["src_table"].dtype == np.int32 and np.array_equal(out["src_table"], gt["table"][corr[:, 0]])
    assert np.array_equal(out["tgt_table"], gt["table"][corr[:, 1]])
    assert out["src_mask"].dtype == np.bool_ and np.array_equal(out["src_mask"], out["src_table"] != len(fine))
    assert np.array_equal(out["tgt_mask"], out["tgt_table"] != len(fine))
    want = labels_by_loops(fine, gt["table"], corr, RADIUS)
    assert out["labels"].dtype == np.bool_ and np.array_equal(out["labels"], want)
    assert np.array_equal(out["labels"], PP.patch_corr_labels(fine, gt["table"], corr, RADIUS))
    L = out["labels"]
    assert L[:, :LIMIT, :LIMIT].any(axis=(1, 2)).all()          # a listed pair overlaps: its matrix is never empty
    # the regimes, so that nothing here can go vacuous
    co = gt["corr_offsets"]
    cand = [int((gt["overlap"][co[p]:co[p + 1]] > 0.3).sum()) for p in range(2)]
    counts = np.diff(so).tolist()
    if fine_level == 0:
        assert P == 390 and sum(cand) == 285 and counts == [64, 64]
        assert int(L[:, :LIMIT, :LIMIT].sum()) > 0 and L[:, :LIMIT, LIMIT].any() and (~out["src_mask"]).any()
        full = PP.fine_ground_truth(pyramid, gt, fine_level=0, radius=RADIUS, keys=keys, min_overlap=-1.0, num_targets=10 ** 6)
        assert len(full["rows"]) == 390 and int(full["labels"][:, :LIMIT, :LIMIT].sum()) == 5199
        assert int(full["labels"][:, :LIMIT, LIMIT].sum()) == 1440 and (~full["src_mask"]).any() and (~full["tgt_mask"]).any()
    if fine_level == 1:
        assert P == 330 and sum(cand) == 261 and counts == [64, 64]
    if fine_level == 2:
        assert cand == [53, 43] and counts == cand                                        # fewer than num_targets: all kept
        assert (L[:, :LIMIT, :LIMIT].sum(axis=(1, 2)) == 1).all() and L[:, 0, 0].all()    # node against node: a single match
