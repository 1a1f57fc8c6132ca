"""The device voxel grid (prg_voxel_grid_ragged, prg_merge_memory_f64) and the three paths that use it, on an MI355X.

Everything here is BIT-EXACT against the host grid (`PP.native_voxel_down_sample`, csrc/hostpool.cpp): a minimum, float64
subtract / divide / floor, integer keys, a stable sort and a sequential in-order sum per voxel have one right answer.  Against
the oracle's dictionary grid (unspecified voxel order) the comparison is as a point set, still with tolerance 0.  The numpy
specification (`PP.voxel_down_sample`) is compared with `np.array_equal` too.  Run with `-m gpu`.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOXELS = (0.002, 0.005, 0.025)


@pytest.fixture(scope="module")
def hip():
    from pointreggpt_amd import _lib, geometry
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import MaskUnet, Unet
    _lib.load()

    class NS:
        pass

    ns = NS()
    ns.G, ns.GaussianDiffusion, ns.MaskUnet, ns.Unet, ns.lib = geometry, GaussianDiffusion, MaskUnet, Unet, _lib
    return ns


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run_grid(hip, segs, v, valids=None):
    """segs: list of (n,3) float64; valids: list of bool arrays (or None = no mask at all) -> host copies of the outputs."""
    offs = np.zeros(len(segs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in segs])
    pts = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in segs], 0)
    d_valid = None if valids is None else D(np.concatenate(valids).astype(np.uint8))
    out, oo, st = hip.G.voxel_grid_ragged(D(pts), d_valid, D(offs), v)
    torch.cuda.synchronize()
    return out.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()


def lexsorted(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def check_against_host(segs, valids, v, out, oo, st, oracle=True):
    from oracle import postprocess as OP
    from pointreggpt_amd import postprocess as PP
    assert oo[0] == 0 and np.all(np.diff(oo) >= 0)
    for b, seg in enumerate(segs):
        rows = np.asarray(seg, dtype=np.float64).reshape(-1, 3)
        if valids is not None:
            rows = rows[np.asarray(valids[b], dtype=bool)]
        got = out[oo[b]:oo[b + 1]]
        assert st[b] == 0, (b, st[b])
        want = PP.native_voxel_down_sample(rows, v)
        assert np.array_equal(got, want) and same_bits(got, want), (b, got.shape, want.shape)
        if oracle and len(rows):
            orc = OP.voxel_down_sample(rows, v)
            assert np.array_equal(lexsorted(got), lexsorted(orc)), b          # point set, atol = 0 on matched voxels


def check_against_numpy_spec(segs, valids, v, out, oo):
    """Every segment against `PP.voxel_down_sample`; the figures are printed before the assertion."""
    from pointreggpt_amd import postprocess as PP
    bad = []
    for b, seg in enumerate(segs):
        rows = np.asarray(seg, dtype=np.float64).reshape(-1, 3)
        if valids is not None:
            rows = rows[np.asarray(valids[b], dtype=bool)]
        got = out[oo[b]:oo[b + 1]]
        spec = PP.voxel_down_sample(rows, v).reshape(-1, 3)
        assert got.shape == spec.shape, (b, got.shape, spec.shape)
        host = PP.native_voxel_down_sample(rows, v)
        differ = np.flatnonzero((got != spec).any(axis=1))
        if len(differ):
            print(f"segment {b}: {len(differ)} of {len(got)} voxels differ from the numpy specification, max |diff| "
                  f"{np.abs(got - spec).max():.3e}; device == host C++ grid bit for bit: {same_bits(got, host)}; "
                  f"host C++ grid == numpy specification: {np.array_equal(host, spec)}")
            bad.append(b)
    assert not bad, bad


def box(rng, n):
    return rng.uniform([-1.5, -1.5, 0.5], [1.5, 1.5, 3.5], (n, 3))


def mixed_segments(rng, v):
    """One call with every small case of the list: -> (segs, valids)."""
    segs, valids = [], []

    def add(p, m=None):
        segs.append(np.asarray(p, dtype=np.float64))
        valids.append(np.ones(len(p), dtype=bool) if m is None else m)

    add(box(rng, 20000))                                                   # random cloud in the crop box
    add(rng.uniform(-3.0, -0.25, (15000, 3)))                              # negative coordinates only
    few = box(rng, 400)
    add(few[rng.integers(0, 400, 30000)])                                  # many exact duplicates
    base = np.array([-1.0, -1.25, 0.75])                                   # points exactly on org + k*v
    ks = rng.integers(1, 300, (12000, 3)).astype(np.float64)
    add(np.concatenate([base[None], (base - v * 0.5) + ks * v], 0))
    add(box(rng, 25000).astype(np.float32).astype(np.float64))             # float32-valued (the memory case)
    add(np.zeros((0, 3)))                                                  # empty segment
    add(box(rng, 5000), np.zeros(5000, dtype=bool))                        # all rows invalid
    p = box(rng, 18000)
    m = rng.random(18000) > 0.3
    p[~m] = np.nan                                                         # NaN rows masked by valid
    add(p, m)
    surf = box(rng, 30000)
    surf[:, 2] = 2.0 + 0.05 * np.sin(3 * surf[:, 0]) + 0.0005 * rng.standard_normal(30000)   # a dense surface: runs of many rows
    add(surf)
    return segs, valids


def ragged_64(rng):
    sizes = np.linspace(0, 60000, 64).astype(np.int64)
    rng.shuffle(sizes)
    assert sizes.min() == 0 and sizes.max() == 60000
    segs, valids = [], []
    for n in sizes:
        p = box(rng, int(n))
        m = rng.random(int(n)) > 0.1
        p[~m] = np.nan
        segs.append(p)
        valids.append(m)
    return segs, valids


CASES = ("small", "million", "ragged64")
_RESULTS = {}


def case(hip, name, v):
    """(segs, valids, out, out_offsets, status) of one case, computed once for the tests that look at it."""
    if (name, v) not in _RESULTS:
        rng = np.random.default_rng(int(v * 1e4) + CASES.index(name))
        if name == "small":
            segs, valids = mixed_segments(rng, v)
        elif name == "million":
            segs, valids = [box(rng, 1_000_000)], None                      # B = 1, one very large cloud, no mask array
        else:
            segs, valids = ragged_64(rng)
        _RESULTS[(name, v)] = (segs, valids) + run_grid(hip, segs, v, valids)
    return _RESULTS[(name, v)]


@pytest.mark.parametrize("v", VOXELS)
@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_host_bit_for_bit(hip, name, v):
    """Per segment: np.array_equal (and the same bytes) against the host C++ grid; the same point set, tolerance 0, against
    the oracle's dictionary grid."""
    segs, valids, out, oo, st = case(hip, name, v)
    check_against_host(segs, valids, v, out, oo, st)
    if name == "small":
        assert oo[6] == oo[5] == oo[7], "empty and all-invalid segments produce no rows"
        # the same clouds without a mask array at all (valid = NULL): only the fully valid segments
        plain = [s for s, m in zip(segs, valids) if m.all()]
        out, oo, st = run_grid(hip, plain, v, None)
        check_against_host(plain, None, v, out, oo, st, oracle=False)


@pytest.mark.parametrize("v", VOXELS)
@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_numpy_specification(hip, name, v):
    """np.array_equal against the numpy specification `PP.voxel_down_sample` on the same cases.  (The specification adds the
    rows of a voxel one after the other, like the C++ and the device grid; `np.add.reduceat`, which it used before, adds runs of
    8 or more rows pairwise and was up to 6.7e-15 m away from both on the duplicates cloud.)"""
    segs, valids, out, oo, st = case(hip, name, v)
    assert not st.any()
    check_against_numpy_spec(segs, valids, v, out, oo)


def test_more_than_1024_scan_blocks(hip):
    """1 100 000 rows are 1075 blocks of 1024 sorted rows: the one-workgroup scan over the block counts takes 1024 per round,
    so its second round, which starts from the first round's carry, runs only here ("million" has 977 blocks).  Two segments,
    no mask array; bit for bit against the host C++ grid.  At 0.025 the box has 1.7 million cells, so most rows are a voxel of
    their own: every block has heads, and the slots of the last 51 blocks' voxels and the total depend on the carry."""
    rng = np.random.default_rng(1075)
    segs, v = [box(rng, 600_000), box(rng, 500_000)], 0.025
    assert (len(segs[0]) + len(segs[1]) + 1023) // 1024 == 1075
    out, oo, st = run_grid(hip, segs, v, None)
    check_against_host(segs, None, v, out, oo, st, oracle=False)


def test_total_zero(hip):
    for B in (1, 5):
        out, oo, st = hip.G.voxel_grid_ragged(torch.empty((0, 3), dtype=torch.float64, device="cuda"), None,
                                              torch.zeros(B + 1, dtype=torch.int64, device="cuda"), 0.002)
        torch.cuda.synchronize()
        assert out.shape == (0, 3) and oo.cpu().tolist() == [0] * (B + 1) and st.cpu().tolist() == [0] * B


def test_capacity_rows_beyond_the_last_offset_are_ignored(hip):
    """`total` may be a buffer's capacity: rows outside [offsets[0], offsets[B]) take no part, whatever they hold."""
    from pointreggpt_amd import postprocess as PP
    rng = np.random.default_rng(3)
    a, b = box(rng, 3000), box(rng, 2000)
    junk = np.full((700, 3), np.nan)
    pts = np.concatenate([a, b, junk], 0)
    out, oo, st = hip.G.voxel_grid_ragged(D(pts), None, D(np.array([0, 3000, 5000], dtype=np.int64)), 0.025)
    out, oo, st = out.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == [0, 0]
    assert same_bits(out[oo[0]:oo[1]], PP.native_voxel_down_sample(a, 0.025))
    assert same_bits(out[oo[1]:oo[2]], PP.native_voxel_down_sample(b, 0.025))


def test_status_nonfinite_and_too_small(hip):
    from pointreggpt_amd import postprocess as PP
    rng = np.random.default_rng(17)
    a, c, e = box(rng, 9000), box(rng, 7000), box(rng, 4000)
    bad_nan, bad_inf = box(rng, 5000), box(rng, 5000)
    bad_nan[1234, 1] = np.nan
    bad_inf[4999, 2] = np.inf
    segs = [a, bad_nan, c, bad_inf, e]
    out, oo, st = run_grid(hip, segs, 0.005)
    assert st.tolist() == [0, 1, 0, 1, 0]
    assert oo[2] == oo[1] and oo[4] == oo[3], "a failed segment produces no rows"
    for b in (0, 2, 4):
        assert same_bits(out[oo[b]:oo[b + 1]], PP.native_voxel_down_sample(segs[b], 0.005)), b
    for bad in (bad_nan, bad_inf):
        with pytest.raises(hip.lib.PrgError, match="non-finite"):
            PP.native_voxel_down_sample(bad, 0.005)
    # the host's "voxel_size is too small"
    tiny = 1e-7
    with pytest.raises(hip.lib.PrgError, match="too small"):
        PP.native_voxel_down_sample(a, tiny)
    with pytest.raises(ValueError, match="too small"):
        PP.voxel_down_sample(a, tiny)
    out, oo, st = run_grid(hip, [c, a, e], tiny)
    assert st.tolist() == [2, 2, 2] and oo.tolist() == [0, 0, 0, 0]
    # ... and one segment's failure leaves the others alone: a far outlier makes only ITS grid too large
    wide = np.concatenate([a, [[1e9, 1e9, 1e9]]], 0)
    out, oo, st = run_grid(hip, [c, wide, e], 0.002)
    assert st.tolist() == [0, 2, 0] and oo[2] == oo[1]
    assert same_bits(out[oo[0]:oo[1]], PP.native_voxel_down_sample(c, 0.002))
    assert same_bits(out[oo[2]:oo[3]], PP.native_voxel_down_sample(e, 0.002))
    with pytest.raises(hip.lib.PrgError):
        hip.G.voxel_grid_ragged(D(a), None, D(np.array([0, len(a)], dtype=np.int64)), 0.0)


def test_independence_and_determinism(hip):
    rng = np.random.default_rng(23)
    x = box(rng, 40000)
    x[::7] = x[::7].astype(np.float32)
    xm = rng.random(40000) > 0.05
    v = 0.002
    alone, oo, st = run_grid(hip, [x], v, [xm])
    alone = alone[:oo[1]].copy()
    assert st.tolist() == [0] and len(alone) > 1000
    others = [box(rng, int(n)) for n in rng.integers(0, 30000, 63)]
    for pos in (0, 63, 31):
        segs = others[:pos] + [x] + others[pos:]
        valids = [np.ones(len(s), dtype=bool) for s in segs]
        valids[pos] = xm
        out, oo, st = run_grid(hip, segs, v, valids)
        assert not st.any()
        assert same_bits(out[oo[pos]:oo[pos + 1]], alone), pos
        again, oo2, _ = run_grid(hip, segs, v, valids)
        assert np.array_equal(oo, oo2) and same_bits(out[:oo[-1]], again[:oo2[-1]]), pos


def test_merge_kernel(hip):
    rng = np.random.default_rng(5)
    B, HW = 4, 32 * 32
    mem = [box(rng, n).astype(np.float32) for n in (700, 0, 1500, 33)]
    xyz = rng.uniform(-2, 2, (B, HW, 3))
    valid = rng.random((B, HW)) > 0.4
    xyz[~valid] = np.nan
    mem_pts, mem_offs = hip.G.upload_clouds(mem, "cuda")
    # capacity larger than the rows in use (the tail of a previous grid's output buffer)
    mem_pts = torch.cat([mem_pts, torch.full((50, 3), float("nan"), device="cuda")])
    merged, mvalid, moffs = hip.G.merge_memory(mem_pts, mem_offs, D(xyz), D(valid))
    torch.cuda.synchronize()
    merged, mvalid, moffs = merged.cpu().numpy(), mvalid.cpu().numpy(), moffs.cpu().numpy()
    assert merged.shape == (sum(len(m) for m in mem) + 50 + B * HW, 3)
    want_offs = np.cumsum([0] + [len(m) + HW for m in mem])
    assert moffs.tolist() == want_offs.tolist()
    for b in range(B):
        want = np.concatenate([mem[b].astype(np.float64), xyz[b]])
        assert same_bits(merged[moffs[b]:moffs[b + 1]], want), b                    # NaN rows included, bit for bit
        want_valid = np.concatenate([np.ones(len(mem[b]), dtype=np.uint8), valid[b].astype(np.uint8)])
        assert np.array_equal(mvalid[moffs[b]:moffs[b + 1]], want_valid), b
    # ... and the grid over it is the host's memory update
    from pointreggpt_amd import postprocess as PP
    out, oo, st = hip.G.voxel_grid_ragged(D(merged), D(mvalid), D(moffs), 0.002)
    out, oo = out.cpu().numpy(), oo.cpu().numpy()
    for b in range(B):
        host = PP.native_voxel_down_sample(np.concatenate([mem[b], xyz[b][valid[b]]], axis=0), 0.002)
        assert same_bits(out[oo[b]:oo[b + 1]], host), b


def _tree(root):
    files = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            files[os.path.relpath(p, root)] = open(p, "rb").read()
    return files


@pytest.mark.parametrize("B", [2, 5])
def test_generator_device_memory_writes_the_same_bytes(hip, tmp_path, monkeypatch, B):
    """The set-up of test_num_samples_3_against_oracle_sequence, once per backend: every file byte-identical, every
    condition the sampler saw identical, and the device run never voxelises on the host inside the sample loop."""
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd.generator import Generator
    S, NSMP, seed = 64, 3, 11
    net = hip.Unet(16, dtype="fp32").init_synthetic(3)
    mask = hip.MaskUnet(16, dtype="fp32").init_synthetic(4, final_bias=8.0)
    diff = hip.GaussianDiffusion(net, image_size=S, timesteps=1000, sampling_timesteps=4)
    real_sample, real_grid = diff.sample, PP.native_voxel_down_sample
    conds, grid_calls = {}, {}

    def run(backend):
        conds[backend], grid_calls[backend] = [], 0

        def spy(**kw):
            conds[backend].append(kw["img_cond"].detach().cpu().clone())
            return real_sample(**kw)

        def grid_spy(pts, voxel_size):
            grid_calls[backend] += 1
            return real_grid(pts, voxel_size)

        diff.sample = spy
        monkeypatch.setattr(PP, "native_voxel_down_sample", grid_spy)
        gen = Generator(diff, None, batch_size=B, samples_folder=str(tmp_path / backend / "data"), synthetic_seed=seed)
        gen.generate(0, B, NSMP, depth_correction=mask, mask_threshold=0.5, noise_seed=seed, voxel_backend=backend)
        torch.cuda.synchronize()
        monkeypatch.setattr(PP, "native_voxel_down_sample", real_grid)
        diff.sample = real_sample

    run("host")
    run("device")
    assert grid_calls["host"] == B * (NSMP - 1) and grid_calls["device"] == 0, grid_calls
    assert len(conds["host"]) == len(conds["device"]) == NSMP
    for s in range(NSMP):
        assert torch.equal(conds["host"][s], conds["device"][s]), s
    host, dev = _tree(tmp_path / "host"), _tree(tmp_path / "device")
    assert sorted(host) == sorted(dev) and len(host) >= B * (2 + 4 * NSMP)
    for name in host:
        assert host[name] == dev[name], name
    diff.close(); net.close(); mask.close()


def test_tester_generate_backends_agree(hip, tmp_path):
    from pointreggpt_amd.tester import Tester
    net = hip.Unet(16, dtype="fp32").init_synthetic(32)
    diff = hip.GaussianDiffusion(net, image_size=32, timesteps=1000, sampling_timesteps=3)
    got = {}
    for backend in ("host", "device"):
        np.random.seed(5)
        t = Tester(diff, batch_size=2, samples_folder=str(tmp_path / backend), seed=9)
        got[backend] = t.generate(3, 3, voxel_size=0.005, voxel_backend=backend)
    assert [len(b) for b in got["host"]] == [len(b) for b in got["device"]] == [2, 1]
    for bh, bd in zip(got["host"], got["device"]):
        for a, b in zip(bh, bd):
            assert a.dtype == b.dtype == np.float32 and len(a) > 0 and np.array_equal(a, b)
    for i in range(3):
        assert (tmp_path / "host" / f"scene-{i}.ply").read_bytes() == (tmp_path / "device" / f"scene-{i}.ply").read_bytes(), i
    diff.close(); net.close()


def test_generate_gt_backends_agree(hip, tmp_path):
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd.generator import generate_gt
    rng = np.random.default_rng(12)

    def cloud(n, shift):
        return np.c_[rng.uniform(-1.2, 1.2, n) + shift, rng.uniform(-1.0, 1.0, n), 2.0 + 0.05 * rng.standard_normal(n)]

    scenes = []
    for i in range(9):
        if i % 3 == 0:
            scenes.append([cloud(6000, 0.0), cloud(5000, 0.3), cloud(4000, 0.8)])          # overlapping
        elif i % 3 == 1:
            scenes.append([cloud(3000, 0.0), cloud(3000, 6.0), cloud(2500, 0.05)])         # one disjoint from the others
        else:
            scenes.append([cloud(4000, 0.0), cloud(600, 0.0), cloud(3500, 0.4)])           # one below 1000 points: skipped
    for root in ("dev", "host"):
        for i, clouds in enumerate(scenes):
            d = tmp_path / root / "ds" / "data" / "scene-{:0>6d}".format(i)
            d.mkdir(parents=True)
            for k, c in enumerate(clouds):
                PP.write_ply(str(d / "sample-{:0>6d}.cloud.ply".format(k)), c)
    generate_gt("ds", 0, 9, 3, root=str(tmp_path / "dev"), voxel="device")
    generate_gt("ds", 0, 9, 3, root=str(tmp_path / "host"), voxel="host")
    n_lines = 0
    for i in range(9):
        a = (tmp_path / "dev" / "ds" / "data" / "scene-{:0>6d}".format(i) / "gt.log").read_bytes()
        b = (tmp_path / "host" / "ds" / "data" / "scene-{:0>6d}".format(i) / "gt.log").read_bytes()
        assert a == b, i
        n_lines += a.count(b"\n")
    assert n_lines >= 9
    pairs = [(s[a], s[b]) for s in scenes for a, b in ((0, 1), (0, 2), (1, 2))]
    dev = PP.overlap_ratios_hip(pairs, voxel="device")
    assert dev == PP.overlap_ratios_hip(pairs, voxel="host")
    assert dev == [PP.compute_overlap_ratio(a, b) for a, b in pairs]
    assert any(r == (0.0, 0.0) for r in dev) and any(0.2 < r[0] < 1.0 for r in dev)
