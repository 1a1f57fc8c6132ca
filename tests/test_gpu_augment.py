"""prg_augment_ragged_f64 on an MI355X against its numpy specification `postprocess.augment_cloud`, bit for bit.  Run with
`-m gpu`.

One ragged batch serves every test: clouds of 0, 1, 63, 64, 65, 255, 256, 257, 1000 and 2049 rows (around the wave, the 256-row
tile / workgroup, and long enough for the grid-stride loop: 7 workgroups per cloud at this batch, so the workgroup that took
rows 0..255 of the last cloud also takes 1792..2047), between poisoned rows that belong to no segment.  `out` and `rows` are
preset to sentinels, and every element the specification does not define must still hold them afterwards."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 2049]
C = len(SIZES)
LEAD, TAIL = 5, 7                       # poisoned rows before the first and after the last segment, input and output
SEEDS = [(0x9E3779B97F4A7C15 * (c + 1) + (c << 40)) & 0xFFFFFFFFFFFFFFFF | (1 << 63) for c in range(C)]      # high words set
OUT_SENTINEL, ROW_SENTINEL = -77.25, -7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _pose(rng):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("XYZ", rng.uniform(-3.0, 3.0, 3)).as_matrix()
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3)
    return T


@pytest.fixture(scope="module")
def batch():
    from pointreggpt_amd import _lib
    _lib.load()
    rng = np.random.RandomState(20250101)
    clouds = [rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3)) for n in SIZES]
    clouds[4][3, 0] = clouds[9][2000, 2] = -0.0
    offs = LEAD + np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    buf = np.full((offs[-1] + TAIL, 3), np.nan)
    buf[offs[0]:offs[-1]] = np.concatenate(clouds)
    T = np.stack([_pose(rng) for _ in range(C)])
    return dict(clouds=clouds, offs=offs, buf=buf, T=T, dev=torch.from_numpy(buf).cuda())


def run(batch, *, limit=None, noise=0.0, draw=0, T=None, has_T=None, keys=None, capacity=None, pts=None, clouds=None):
    """One launch on the batch -> nothing; asserts every output bit against the specification, the sentinels elsewhere, and that
    the inputs are unchanged.  keys: per-cloud list of uint32 arrays; capacity: per-cloud output segment sizes."""
    from pointreggpt_amd import _lib
    lib = _lib.load()
    clouds = batch["clouds"] if clouds is None else clouds
    src = batch["dev"] if pts is None else pts
    before = src.clone()
    offs = batch["offs"]
    want = []
    for c, cl in enumerate(clouds):
        lim = limit
        if capacity is not None:
            lim = capacity[c] if limit is None else min(limit, capacity[c])
        if lim == 0:
            want.append((np.zeros((0, 3)), np.zeros(0, dtype=np.int32)))
            continue
        want.append(PP.augment_cloud(cl, seed=SEEDS[c], draw=draw, noise=noise, limit=lim,
                                     T=None if T is None or (has_T is not None and not has_T[c]) else T[c],
                                     keys=None if keys is None else keys[c]))
    cap = [min(n, limit or n) for n in SIZES] if capacity is None else list(capacity)
    o_offs = LEAD + np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
    out_total = int(o_offs[-1]) + TAIL
    out = torch.full((out_total, 3), OUT_SENTINEL, dtype=torch.float64, device="cuda")
    rows = torch.full((out_total,), ROW_SENTINEL, dtype=torch.int32, device="cuda")
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kd = None
    if keys is not None:
        flat = np.zeros(len(batch["buf"]), dtype=np.uint32)
        flat[offs[0]:offs[-1]] = np.concatenate(keys)
        kd = dev(flat.view(np.int32))
    d_offs, d_ooffs, d_T, d_has = dev(offs), dev(o_offs), dev(T), dev(None if has_T is None else np.asarray(has_T, dtype=np.uint8))
    d_seeds = dev(np.array(SEEDS, dtype=np.uint64).view(np.int64))
    _lib.check(lib.prg_augment_ragged_f64(_lib.ptr(src), _lib.ptr(d_offs), C, src.shape[0], _lib.ptr(d_T), _lib.ptr(d_has),
                                          _lib.ptr(d_seeds), draw, _lib.ptr(kd), limit or 0, noise, _lib.ptr(d_ooffs), out_total,
                                          _lib.ptr(out), _lib.ptr(rows), _lib.stream_ptr()), "prg_augment_ragged_f64")
    got, got_rows = out.cpu().numpy(), rows.cpu().numpy()
    exp = np.full((out_total, 3), OUT_SENTINEL)
    exp_rows = np.full(out_total, ROW_SENTINEL, dtype=np.int32)
    for c, (w, r) in enumerate(want):
        assert len(w) == min(SIZES[c], limit or SIZES[c], cap[c])
        exp[o_offs[c]:o_offs[c] + len(w)] = w
        exp_rows[o_offs[c]:o_offs[c] + len(r)] = r
    assert np.array_equal(got_rows, exp_rows)
    assert np.array_equal(bits(got), bits(exp))
    assert torch.equal(src.view(torch.int64), before.view(torch.int64))              # NaN poison included
    return got, got_rows, o_offs


HAS_T = [1, 0, 1, 1, 0, 1, 0, 1, 0, 1]


@pytest.mark.parametrize("limit", [1, 64, 256, 257, 1000, None])
@pytest.mark.parametrize("noise,draw", [(0.005, 0), (0.0, 0), (0.005, 3)])
def test_every_limit_with_philox_keys_and_a_mix_of_moves(batch, limit, noise, draw):
    run(batch, limit=limit, noise=noise, draw=draw, T=batch["T"], has_T=HAS_T)


def test_draws_differ(batch):
    a = run(batch, limit=64, noise=0.005, draw=0)
    b = run(batch, limit=64, noise=0.005, draw=1)
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(bits(a[0]), bits(b[0]))


@pytest.mark.parametrize("limit", [1, 64, 257])
def test_equal_caller_keys_keep_the_first_rows(batch, limit):
    keys = [np.full(n, 0xFFFFFFFF, dtype=np.uint32) for n in SIZES]         # the value the pad slots of a tile hold
    _, rows, o = run(batch, limit=limit, noise=0.005, keys=keys, T=batch["T"])
    for c, n in enumerate(SIZES):
        assert np.array_equal(rows[o[c]:o[c] + min(n, limit)], np.arange(min(n, limit)))


@pytest.mark.parametrize("limit", [64, 1000, 2048])
def test_caller_keys_with_ties_across_tile_and_workgroup_boundaries(batch, limit):
    rng = np.random.RandomState(7)
    keys = [(rng.randint(1, 6, n) * 0x30000000).astype(np.uint32) for n in SIZES]    # heavy ties, the sign bit in use
    for c, n in enumerate(SIZES):
        for edge in (64, 256, 1024, 1792, 2048):          # wave, tile, the grid-stride step of the 2049-row cloud, its last tile
            if n > edge:
                keys[c][edge - 2:edge + 1] = 0            # the smallest key on both sides: rows edge-2 .. edge all survive a cut
    _, rows, o = run(batch, limit=limit, noise=0.005, keys=keys, T=batch["T"], has_T=HAS_T)
    first = rows[o[9]:o[9] + 15]
    assert np.array_equal(first, [62, 63, 64, 254, 255, 256, 1022, 1023, 1024, 1790, 1791, 1792, 2046, 2047, 2048])


@pytest.mark.parametrize("limit", [None, 256])
def test_a_short_output_segment_clamps(batch, limit):
    capacity = [0, 1, 10, 64, 0, 100, 256, 256, 999, 300]
    run(batch, limit=limit, noise=0.005, T=batch["T"], has_T=HAS_T, capacity=capacity)


def test_moves_alone_are_rigid_crop_raggeds_bits(batch):
    from pointreggpt_amd import geometry as G
    got, rows, o = run(batch, T=batch["T"], has_T=HAS_T)
    offs = batch["offs"]
    ref, _ = G.rigid_crop_ragged(batch["dev"], None, torch.from_numpy(offs).cuda(), T=batch["T"], has_T=np.array(HAS_T, np.uint8))
    ref = ref.cpu().numpy()
    assert np.array_equal(bits(got[o[0]:o[-1]]), bits(ref[offs[0]:offs[-1]]))
    assert np.array_equal(rows[o[0]:o[-1]], np.concatenate([np.arange(n) for n in SIZES]))


def test_nothing_on_copies_the_bits(batch):
    got, _, o = run(batch)
    assert np.array_equal(bits(got[o[0]:o[-1]]), bits(np.concatenate(batch["clouds"])))
    assert np.signbit(got[o[4] + 3, 0]) and np.signbit(got[o[9] + 2000, 2])


def test_float32_rounded_input(batch):
    clouds = [c.astype(np.float32).astype(np.float64) for c in batch["clouds"]]
    buf = batch["buf"].copy()
    buf[batch["offs"][0]:batch["offs"][-1]] = np.concatenate(clouds)
    run(batch, limit=256, noise=0.005, T=batch["T"], has_T=HAS_T, pts=torch.from_numpy(buf).cuda(), clouds=clouds)


def test_wrapper_and_host_convenience(batch):
    """`geometry.augment_clouds` (device in, device out, float32 widened) and `postprocess.augment_clouds_hip` (host in, host out)."""
    from pointreggpt_amd import geometry as G
    clouds = [c.astype(np.float32) for c in batch["clouds"]]
    want = [PP.augment_cloud(cl, seed=SEEDS[c], draw=2, noise=0.005, limit=256, T=batch["T"][c] if HAS_T[c] else None)
            for c, cl in enumerate(clouds)]
    res = G.augment_clouds(torch.from_numpy(np.concatenate(clouds)).cuda(), SIZES, seeds=SEEDS, draw=2, noise=0.005, limit=256,
                           T=batch["T"], has_T=np.array(HAS_T, np.uint8))
    assert all(res[k].is_cuda for k in ("points", "lengths", "rows"))
    assert res["points"].dtype == torch.float64 and res["rows"].dtype == torch.int32 and res["lengths"].dtype == torch.int64
    assert res["lengths"].cpu().tolist() == [min(n, 256) for n in SIZES]
    assert np.array_equal(bits(res["points"].cpu().numpy()), bits(np.concatenate([w for w, _ in want])))
    assert np.array_equal(res["rows"].cpu().numpy(), np.concatenate([r for _, r in want]))
    host = PP.augment_clouds_hip(clouds, seeds=SEEDS, draw=2, noise=0.005, limit=256,
                                 T=[batch["T"][c] if HAS_T[c] else None for c in range(C)])
    for (p, r), (wp, wr) in zip(host, want):
        assert np.array_equal(bits(p), bits(wp)) and np.array_equal(r, wr) and r.dtype == np.int32
    keys = [np.random.RandomState(c).randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for c, n in enumerate(SIZES)]
    host = PP.augment_clouds_hip(clouds, seeds=SEEDS, limit=100, keys=keys)
    for c, (p, r) in enumerate(host):
        wp, wr = PP.augment_cloud(clouds[c], seed=SEEDS[c], limit=100, keys=keys[c])
        assert np.array_equal(bits(p), bits(wp)) and np.array_equal(r, wr)
    empty = G.augment_clouds(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), [0, 0], seeds=[1, 2], noise=0.005)
    assert empty["points"].shape == (0, 3) and empty["rows"].shape == (0,) and empty["lengths"].cpu().tolist() == [0, 0]
