"""`postprocess.augment_cloud`, the numpy specification of prg_augment_ragged_f64, and the pose drawing of
`stream.PairStream(augment=...)`, checked on the host: the package's Philox against the oracle's word for word, the properties
of the cut and of the noise, and the poses."""
import numpy as np
import pytest

from oracle import philox as oracle_philox
from pointreggpt_amd import philox
from pointreggpt_amd import postprocess as PP
from pointreggpt_amd import synthetic
from pointreggpt_amd.stream import Augment, augment_poses, uniform_rotation

TAG = 0x6175676D


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cloud(n, seed=0):
    return np.random.RandomState(seed).uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


def test_package_philox_equals_the_oracle_word_for_word():
    rng = np.random.RandomState(1)
    c = [rng.randint(0, 2 ** 32, 4096, dtype=np.uint64) for _ in range(4)]
    for key in [0, 1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF] + [int(k) for k in rng.randint(0, 2 ** 63, 4, dtype=np.uint64) * 2 + 1]:
        want = oracle_philox.philox4x32_10(c, (key & 0xFFFFFFFF, key >> 32))
        got = philox.philox4x32_10(*c, key)
        for g, w in zip(got, want):
            assert g.dtype == np.uint32 and np.array_equal(g.astype(np.uint64), w)
    # the counter layout of the augmentation: scalars broadcast against the row index
    got = philox.philox4x32_10(np.arange(100), 3, TAG, 0, 77)
    want = oracle_philox.philox4x32_10((np.arange(100), np.full(100, 3), np.full(100, TAG), np.zeros(100)), (77, 0))
    assert all(np.array_equal(g.astype(np.uint64), w) for g, w in zip(got, want))


def test_augment_seed_is_built_like_noise_seed():
    want = int(np.random.SeedSequence([11, 5, TAG]).generate_state(1, np.uint64)[0])
    assert synthetic.augment_seed(11, 5, 0) == want == synthetic.augment_seed(11, 5)
    assert synthetic.augment_seed(11, 5, 2) == int(np.random.SeedSequence([11, 5, TAG, 2]).generate_state(1, np.uint64)[0])
    seeds = {synthetic.augment_seed(11, s, c) for s in range(4) for c in range(3)} | {synthetic.noise_seed(11, s) for s in range(4)}
    assert len(seeds) == 16
    with pytest.raises(ValueError):
        synthetic.augment_seed(11, 5, 3)


@pytest.mark.parametrize("n,limit", [(40, 10), (40, 39), (40, 40), (40, 41), (40, None), (1, 1), (0, 5), (300, 256)])
def test_cut_keeps_distinct_rows_and_order_when_nothing_is_cut(n, limit):
    pts = cloud(n)
    out, rows = PP.augment_cloud(pts, seed=0xABCDEF0123456789, limit=limit)
    m = n if limit is None else min(n, limit)
    assert out.shape == (m, 3) and out.dtype == np.float64 and rows.shape == (m,) and rows.dtype == np.int32
    assert len(set(rows.tolist())) == m and ((rows >= 0) & (rows < max(n, 1))).all()
    assert np.array_equal(bits(out), bits(pts[rows]))
    if m == n:
        assert np.array_equal(rows, np.arange(n))
    else:                                                               # in key order: the rank-by-counting definition
        w0 = philox.philox4x32_10(np.arange(n), 0, TAG, 0, 0xABCDEF0123456789)[0]
        rank = np.array([sum((w0[u], u) < (w0[i], i) for u in range(n)) for i in range(n)])
        assert np.array_equal(rank[rows], np.arange(m)) and set(np.flatnonzero(rank < m)) == set(rows.tolist())


def test_equal_keys_keep_the_first_rows():
    pts = cloud(50)
    out, rows = PP.augment_cloud(pts, seed=3, limit=20, keys=np.full(50, 9, dtype=np.uint32))
    assert np.array_equal(rows, np.arange(20)) and np.array_equal(bits(out), bits(pts[:20]))
    keys = np.arange(50, dtype=np.uint32)[::-1].copy()                  # caller keys decide, largest key last
    assert np.array_equal(PP.augment_cloud(pts, seed=3, limit=20, keys=keys)[1], np.arange(49, 29, -1))


def test_noise_is_a_function_of_the_row_and_inside_half_the_amplitude():
    n, noise = 500, 0.005
    pts = cloud(n)
    full, rows_full = PP.augment_cloud(pts, seed=21, draw=4, noise=noise)
    part, rows = PP.augment_cloud(pts, seed=21, draw=4, noise=noise, limit=100)
    assert np.array_equal(rows_full, np.arange(n)) and np.array_equal(bits(part), bits(full[rows]))
    w = philox.philox4x32_10(np.arange(n), 4, TAG, 0, 21)
    u = (np.stack(w[1:], axis=1).astype(np.float64) + 0.5) * 2.0 ** -32
    assert np.array_equal(bits(full), bits(pts + (u - 0.5) * noise))
    # strictly inside: at the extreme words too (no row of a small cloud is likely to draw them)
    for word in (0, 2 ** 32 - 1):
        d = ((np.float64(word) + 0.5) * 2.0 ** -32 - 0.5) * noise
        assert abs(d) < noise / 2
    assert (np.abs((u - 0.5) * noise) < noise / 2).all() and np.abs(full - pts).max() > noise / 4


def test_nothing_to_do_returns_the_input_bits():
    pts = cloud(64)
    pts[3, 0] = pts[9, 2] = -0.0
    out, rows = PP.augment_cloud(pts, seed=1)
    assert np.array_equal(bits(out), bits(pts)) and np.signbit(out[3, 0]) and np.signbit(out[9, 2])
    assert np.array_equal(rows, np.arange(64))
    assert out is not pts and not np.shares_memory(out, pts)


def test_move_comes_first_and_is_rigid_moves_bits():
    from scipy.spatial.transform import Rotation
    pts = cloud(100)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("XYZ", [0.3, -0.2, 0.9]).as_matrix()
    T[:3, 3] = [0.1, -0.4, 0.25]
    out, rows = PP.augment_cloud(pts, seed=5, limit=30, T=T)
    assert np.array_equal(bits(out), bits(PP.rigid_move(pts[rows], T)))
    noisy, rows2 = PP.augment_cloud(pts, seed=5, limit=30, T=T, noise=0.01)
    assert np.array_equal(rows, rows2)
    w = philox.philox4x32_10(np.arange(100), 0, TAG, 0, 5)
    u = (np.stack(w[1:], axis=1).astype(np.float64) + 0.5) * 2.0 ** -32
    assert np.array_equal(bits(noisy), bits(out + ((u - 0.5) * 0.01)[rows]))
    assert np.abs(noisy - out).max() < 0.005


def test_draw_and_seed_change_the_result():
    pts = cloud(200)
    base = PP.augment_cloud(pts, seed=5, draw=0, noise=0.005, limit=50)
    for kw in (dict(seed=5, draw=1), dict(seed=6, draw=0), dict(seed=5 + 2 ** 32, draw=0)):       # the key's high word counts
        other = PP.augment_cloud(pts, noise=0.005, limit=50, **kw)
        assert not np.array_equal(other[1], base[1]) and not np.array_equal(bits(other[0]), bits(base[0]))
    again = PP.augment_cloud(pts, seed=5, draw=0, noise=0.005, limit=50)
    assert np.array_equal(again[1], base[1]) and np.array_equal(bits(again[0]), bits(base[0]))


def test_bad_arguments():
    pts = cloud(10)
    for kw in (dict(noise=-1.0), dict(noise=np.nan), dict(limit=0), dict(limit=2.5), dict(draw=2 ** 32), dict(draw=-1),
               dict(limit=5, keys=np.zeros(9, dtype=np.uint32))):
        with pytest.raises(ValueError):
            PP.augment_cloud(pts, seed=1, **kw)


def test_every_row_is_kept_a_quarter_of_the_time():
    """n = 40, limit = 10 over 2000 draws: a row's inclusion count is Binomial(2000, 1/4) if the cut is a uniform subset;
    6 standard deviations (sqrt(2000 * 1/4 * 3/4) = 19.4) hold for all 40 rows with a failure probability below 1e-7."""
    pts, n_draws = cloud(40), 2000
    count = np.zeros(40, dtype=np.int64)
    for d in range(n_draws):
        count[PP.augment_cloud(pts, seed=0x5EED5EED5EED, draw=d, limit=10)[1]] += 1
    assert count.sum() == 10 * n_draws
    assert (np.abs(count - n_draws / 4) <= 6 * np.sqrt(n_draws * 0.25 * 0.75)).all(), count


# ---- the poses --------------------------------------------------------------------------------------------------------------
def test_rotations_are_proper():
    rng = np.random.Generator(np.random.Philox(key=5))
    for _ in range(50):
        R = uniform_rotation(rng)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14


@pytest.mark.parametrize("rotation", ["src", "both"])
def test_poses_are_deterministic_per_seed_scene_and_epoch(rotation):
    aug = Augment(rotation=rotation, translation=0.7)
    a, b = augment_poses(11, 3, 2, aug), augment_poses(11, 3, 2, aug)
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(bits(x), bits(y))
    for other in ((12, 3, 2), (11, 4, 2), (11, 3, 3)):
        assert not np.array_equal(augment_poses(*other, aug)[2], a[2])
    move_src, move_tgt, transform = a
    assert (move_tgt is None) == (rotation == "src")
    for M in (move_src, transform) + (() if move_tgt is None else (move_tgt,)):
        assert M.dtype == np.float64 and M.shape == (4, 4) and np.array_equal(M[3], [0, 0, 0, 1])
        assert np.abs(M[:3, :3].T @ M[:3, :3] - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(M[:3, :3]) - 1.0) < 1e-14
    # the documented stream and order: R, t, then R2
    rng = np.random.Generator(np.random.Philox(key=synthetic.augment_seed(11, 3, 2), counter=[0, 0, 0, 2]))
    R = uniform_rotation(rng)
    t = rng.standard_normal(3) * 0.7
    assert np.array_equal(move_src[:3, :3], R.T) and np.array_equal(move_src[:3, 3], -(R.T @ t))
    if rotation == "src":
        assert np.array_equal(transform[:3, :3], R) and np.array_equal(transform[:3, 3], t)
    else:
        assert np.array_equal(move_tgt[:3, :3], uniform_rotation(rng)) and np.array_equal(move_tgt[:3, 3], [0, 0, 0])


def test_no_rotation_draws_nothing():
    assert augment_poses(11, 3, 0, Augment(rotation=None))[:2] == (None, None)
    assert np.array_equal(augment_poses(11, 3, 0, Augment(rotation=None))[2], np.eye(4))


@pytest.mark.parametrize("rotation", ["src", "both"])
def test_transform_takes_the_moved_source_back(rotation):
    """Noise-free item: rigid_move(src_aug, transform) is the source in the target's frame.  Coordinates under 8 m: two float64
    moves and a host-built inverse round to about 1e-13 there; 1e-12 leaves a factor of ten."""
    rng = np.random.RandomState(4)
    src = rng.uniform(-3.0, 3.0, (2000, 3))
    for scene in range(5):
        move_src, move_tgt, transform = augment_poses(11, scene, 0, Augment(rotation=rotation, translation=1.0, noise=0.0))
        src_aug, rows = PP.augment_cloud(src, seed=synthetic.augment_seed(11, scene, 0), limit=500, T=move_src)
        assert np.abs(src_aug).max() < 8.0
        want = src[rows] if move_tgt is None else PP.rigid_move(src[rows], move_tgt)
        assert np.abs(PP.rigid_move(src_aug, transform) - want).max() < 1e-12
