"""Finishing clouds on the device (prg_rigid_crop_ragged_f64, geometry.finish_clouds) and `Generator.generate(gt_log=True)`,
on an MI355X.  Run with `-m gpu`.

Everything is BIT-EXACT: a rigid move written as three products summed left to right in float64 without contraction, six
inclusive comparisons, and the voxel grid (bit-exact already, tests/test_gpu_voxel_grid.py) have one right answer, which
`postprocess.finish_cloud` states in numpy and tests/test_cloud_finish_abi.py pins to the writer pool's PLY payload on the CPU.
The end-to-end tests compare whole dataset trees byte for byte: two passes (generate, then generate_gt) against one
(`gt_log=True`).  Synthetic scene / noise seed of those runs: SEED below, picked because the two-pass reference path alone
yields a gt.log line for each of its three scenes with it (asserted: at least one)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (PP.BBOX_MIN, PP.BBOX_MAX)
SEED = 11
PRG_E_INVALID = -1


@pytest.fixture(scope="module")
def G():
    from pointreggpt_amd import _lib, geometry
    _lib.load()
    return geometry


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pose(rng):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("XYZ", rng.uniform(-0.3, 0.3, 3)).as_matrix()
    T[:3, 3] = rng.uniform(-0.4, 0.4, 3)
    return T.astype(np.float32).astype(np.float64)


def cloud(rng, n):
    return rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


def pack(segs, valids=None, head=0, tail=0):
    """Ragged buffer with `head` / `tail` poisoned rows (NaN with a recognisable payload) outside every segment."""
    poison = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]
    offs = np.zeros(len(segs) + 1, dtype=np.int64)
    offs[0] = head
    offs[1:] = head + np.cumsum([len(s) for s in segs])
    pts = np.concatenate([np.full((head, 3), poison)] + [np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in segs]
                         + [np.full((tail, 3), poison)], 0)
    valid = None
    if valids is not None:
        valid = np.concatenate([np.full(head, 0xAB, np.uint8)] + [np.asarray(v, dtype=np.uint8) for v in valids]
                               + [np.full(tail, 0xAB, np.uint8)])
    return pts, valid, offs


def spec(segs, valids, pres, posts, crop, voxel):
    return [PP.finish_cloud(s, None if valids is None else valids[b], pre=pres[b], crop=crop, lo=BOX[0], hi=BOX[1], voxel=voxel,
                            post=posts[b]) for b, s in enumerate(segs)]


def run_finish(G, segs, valids, pres, posts, crop, voxel, head=0, tail=0):
    B = len(segs)
    pts, valid, offs = pack(segs, valids, head, tail)
    eye = np.eye(4)
    pre = None if all(p is None for p in pres) else np.stack([eye if p is None else p for p in pres])
    post = None if all(p is None for p in posts) else np.stack([eye if p is None else p for p in posts])
    has_pre = None if pre is None or all(p is not None for p in pres) else np.array([p is not None for p in pres])
    has_post = None if post is None or all(p is not None for p in posts) else np.array([p is not None for p in posts])
    d_pts, d_valid = D(pts), None if valid is None else D(valid)
    out, oo, st = G.finish_clouds(d_pts, d_valid, D(offs), voxel, pre=pre, has_pre=has_pre, crop=BOX if crop else None, post=post,
                                  has_post=has_post)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_pts.cpu().numpy()), bits(pts))                     # the input is left as it is
    assert valid is None or np.array_equal(d_valid.cpu().numpy(), valid)
    out, oo, st = out.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()
    assert oo.shape == (B + 1,) and oo[0] == 0 and np.all(np.diff(oo) >= 0) and st.shape == (B,)
    return [out[oo[b]:oo[b + 1]] for b in range(B)], st


def mixed_case():
    """B = 5 ragged segments of 0, 1, 257, 5000 and 3 rows."""
    rng = np.random.RandomState(77)
    sizes = [0, 1, 257, 5000, 3]
    segs = [cloud(rng, n) for n in sizes]
    segs[1][0] = PP.BBOX_MAX                                                          # a single row exactly on hi
    s3 = segs[3]                                                                      # not moved: bounds and signed zeros survive
    s3[:, :2] *= 0.5
    s3[:, 2] = s3[:, 2] * 0.5 + 1.0
    s3[23::13, 1] = -0.0
    segs[4] = segs[4] + [0.0, 0.0, 20.0]                                              # wholly outside the box
    valids = [np.ones(n, dtype=bool) for n in sizes]
    for b in (2, 3):                                                                  # masked rows hold NaN and +-inf
        valids[b] = rng.rand(sizes[b]) < 0.7
        dead = np.flatnonzero(~valids[b])
        segs[b][dead] = np.nan
        segs[b][dead[::2], 1] = np.inf
        segs[b][dead[1::4], 2] = -np.inf
    special = np.r_[10:15, 20:sizes[3]:9]
    valids[3][special] = True
    s3[10], s3[11] = PP.BBOX_MIN, PP.BBOX_MAX                                         # rows on both bounds
    s3[12] = [-1.5, 1.5, 0.5]
    s3[13] = [np.nextafter(1.5, 2.0), 0.0, 1.0]                                      # one ulp outside
    s3[14] = [0.0, 0.0, np.nextafter(0.5, 0.0)]
    s3[20::9, 0] = -0.0
    s3[20::9, 1:] = rng.uniform([-1.0, 1.0], [1.0, 3.0], (len(s3[20::9]), 2))
    T = [pose(rng) for _ in sizes]
    pres = [T[0], None, T[2], None, T[4]]
    posts = [None, np.linalg.inv(T[1]), np.linalg.inv(T[2]), None, np.linalg.inv(T[4])]
    return segs, valids, pres, posts


@pytest.mark.parametrize("voxel", [0.025, 0.0])
def test_finish_clouds_equals_the_numpy_specification(G, voxel):
    segs, valids, pres, posts = mixed_case()
    want = spec(segs, valids, pres, posts, True, voxel)
    got, st = run_finish(G, segs, valids, pres, posts, True, voxel, head=2, tail=37)
    assert not st.any()
    for b in range(len(segs)):
        assert np.array_equal(got[b], want[b]) and same_bits(got[b], want[b]), (b, got[b].shape, want[b].shape)
    assert len(want[0]) == 0 and len(want[1]) == 1 and len(want[4]) == 0 and len(want[2]) > 20 and len(want[3]) > 1000
    if voxel == 0:
        rows = {r.tobytes() for r in got[3]}
        for k in (10, 11, 12):
            assert segs[3][k].tobytes() in rows                                       # on the bounds: kept
        for k in (13, 14):
            assert segs[3][k].tobytes() not in rows                                   # one ulp outside: dropped
        zero = got[3][:, 0] == 0
        assert zero.sum() >= 500 and np.signbit(got[3][zero, 0]).all()                # -0.0 stays -0.0 in a segment that is not moved


def test_no_mask_and_no_crop(G):
    rng = np.random.RandomState(5)
    segs = [cloud(rng, n) for n in (300, 0, 1025)]
    T = [pose(rng) for _ in segs]
    for pres, posts, crop in (([T[0], None, T[2]], [None, None, np.linalg.inv(T[2])], False), ([None] * 3, [None] * 3, True),
                              ([None] * 3, [None] * 3, False)):
        for voxel in (0.025, 0.0):
            want = spec(segs, None, pres, posts, crop, voxel)
            got, st = run_finish(G, segs, None, pres, posts, crop, voxel, tail=5)
            assert not st.any() and all(same_bits(g, w) for g, w in zip(got, want))


def test_a_segment_does_not_depend_on_its_neighbours(G):
    rng = np.random.RandomState(9)
    seg, valid, T = cloud(rng, 3000), rng.rand(3000) < 0.8, pose(rng)
    Ti = np.linalg.inv(T)
    alone, st = run_finish(G, [seg], [valid], [T], [Ti], True, 0.025)
    assert same_bits(alone[0], spec([seg], [valid], [T], [Ti], True, 0.025)[0]) and len(alone[0]) > 500
    for at in (0, 31, 63):
        sizes = rng.randint(0, 400, 64)
        segs = [cloud(rng, n) for n in sizes]
        valids = [rng.rand(n) < 0.9 for n in sizes]
        Ts = [pose(rng) if b % 3 else None for b in range(64)]
        segs[at], valids[at], Ts[at] = seg, valid, T
        posts = [None if t is None else np.linalg.inv(t) for t in Ts]
        got, st = run_finish(G, segs, valids, Ts, posts, True, 0.025, head=at, tail=3)
        assert not st.any() and same_bits(got[at], alone[0]), at


def test_kernel_in_place_tail_and_null_outputs(G):
    """prg_rigid_crop_ragged_f64 itself: in place == out of place; rows outside [offsets[0], offsets[B]) are not written;
    lo / hi NULL with valid_out NULL moves and copies only."""
    segs, valids, pres, _ = mixed_case()
    pts, valid, offs = pack(segs, valids, head=3, tail=41)
    lo_row, hi_row = int(offs[0]), int(offs[-1])
    T = np.stack([np.eye(4) if p is None else p for p in pres])
    has = np.array([p is not None for p in pres])
    fill = np.frombuffer(np.uint64(0x7FF8000000C0FFEE).tobytes(), dtype=np.float64)[0]
    out = D(np.full_like(pts, fill))
    vout = D(np.full(len(pts), 0xCD, np.uint8))
    G.rigid_crop_ragged(D(pts), D(valid), D(offs), T=T, has_T=has, crop=BOX, out=out, valid_out=vout)
    p_in, v_in = D(pts), D(valid)
    r_pts, r_valid = G.rigid_crop_ragged(p_in, v_in, D(offs), T=T, has_T=has, crop=BOX, out=p_in, valid_out=v_in)
    torch.cuda.synchronize()
    assert r_pts.data_ptr() == p_in.data_ptr() and r_valid.data_ptr() == v_in.data_ptr()
    out, vout, p_in, v_in = out.cpu().numpy(), vout.cpu().numpy(), p_in.cpu().numpy(), v_in.cpu().numpy()
    for a, ref in ((out, fill), (p_in, pts[0, 0])):                                  # head and tail untouched
        assert np.all(bits(a[:lo_row]) == bits(np.float64(ref))) and np.all(bits(a[hi_row:]) == bits(np.float64(ref)))
    assert np.all(vout[:lo_row] == 0xCD) and np.all(vout[hi_row:] == 0xCD)
    assert np.all(v_in[:lo_row] == 0xAB) and np.all(v_in[hi_row:] == 0xAB)
    assert np.array_equal(vout[lo_row:hi_row], v_in[lo_row:hi_row]) and set(np.unique(vout[lo_row:hi_row])) <= {0, 1}
    keep = vout[lo_row:hi_row] != 0
    assert np.array_equal(bits(out[lo_row:hi_row][keep]), bits(p_in[lo_row:hi_row][keep]))
    for b, s in enumerate(segs):                                                     # against the specification, row by row
        with np.errstate(invalid="ignore"):
            moved = s if pres[b] is None else PP.rigid_move(s, pres[b])
            inside = np.all((moved >= BOX[0]) & (moved <= BOX[1]), axis=1) & valids[b]
        assert np.array_equal(vout[offs[b]:offs[b + 1]] != 0, inside), b
        assert np.array_equal(bits(out[offs[b]:offs[b + 1]][inside]), bits(moved[inside])), b
    # no crop, no valid_out: a move (or a bit-for-bit copy) of every row of every segment
    finite = [np.where(np.isfinite(s), s, 1.0) for s in segs]
    finite[3][20::9, 0] = -0.0
    pts2, _, offs2 = pack(finite, None, head=3, tail=41)
    o2, v2 = G.rigid_crop_ragged(D(pts2), None, D(offs2), T=T, has_T=has)
    assert v2 is None
    o2 = o2.cpu().numpy()
    for b, s in enumerate(finite):
        want = s if pres[b] is None else PP.rigid_move(s, pres[b])
        assert np.array_equal(bits(o2[offs2[b]:offs2[b + 1]]), bits(want)), b
    assert np.signbit(o2[offs2[3]:offs2[4]][20::9, 0]).all()


def test_empty_call(G):
    T = pose(np.random.RandomState(1))[None]
    for voxel in (0.025, 0.0):
        out, oo, st = G.finish_clouds(D(np.zeros((0, 3))), None, D(np.zeros(2, dtype=np.int64)), voxel, pre=T, crop=BOX,
                                      post=np.linalg.inv(T[0])[None])
        torch.cuda.synchronize()
        assert out.shape == (0, 3) and oo.cpu().tolist() == [0, 0] and st.cpu().tolist() == [0]


def test_bad_arguments(G):
    from pointreggpt_amd import _lib
    lib = _lib.load()
    pts, offs = D(np.zeros((4, 3))), D(np.array([0, 4], dtype=np.int64))
    vout = torch.zeros(4, dtype=torch.uint8, device="cuda")
    lo, hi = (np.ascontiguousarray(b, dtype=np.float64) for b in BOX)
    lo_p, hi_p = lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)
    s = _lib.stream_ptr()
    rc = lib.prg_rigid_crop_ragged_f64(_lib.ptr(pts), None, _lib.ptr(offs), 1, 4, None, None, lo_p, hi_p, _lib.ptr(pts), None, s)
    assert rc == PRG_E_INVALID and b"prg_rigid_crop_ragged_f64" in lib.prg_last_error()
    rc = lib.prg_rigid_crop_ragged_f64(_lib.ptr(pts), None, _lib.ptr(offs), 0, 4, None, None, lo_p, hi_p, _lib.ptr(pts), _lib.ptr(vout), s)
    assert rc == PRG_E_INVALID and b"prg_rigid_crop_ragged_f64" in lib.prg_last_error()
    rc = lib.prg_rigid_crop_ragged_f64(_lib.ptr(pts), None, _lib.ptr(offs), 1, 4, None, None, lo_p, hi_p, _lib.ptr(pts), _lib.ptr(vout), s)
    assert rc == 0
    torch.cuda.synchronize()


# ---- end to end: one pass with gt_log=True leaves the files of two passes ------------------------------------------------------
S, DIM, STEPS, BATCH, SCENES = 64, 16, 4, 2, 3


def tree(root):
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def nets(G):
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import MaskUnet, Unet
    made = []

    def one():
        net = Unet(DIM, dtype="fp32").init_synthetic(3)
        mask = MaskUnet(DIM, dtype="fp32").init_synthetic(4, final_bias=8.0)          # keep-probability ~1: no threshold flips
        diff = GaussianDiffusion(net, image_size=S, timesteps=1000, sampling_timesteps=STEPS)
        made.append((diff, net, mask))
        return diff, mask

    yield one(), one()
    for diff, net, mask in made:
        diff.close(); net.close(); mask.close()


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):
    """Per num_samples: tree A (generate, generate_gt, gather_gt), tree B (generate(gt_log=True), gather_gt), their roots."""
    from pointreggpt_amd.generator import Generator, gather_gt, generate_gt
    (diff, mask), _lane = nets
    out = {}
    for ns in (1, 2):
        base = tmp_path_factory.mktemp("ns%d" % ns)
        for which in ("A", "B"):
            gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(base / which / "ds" / "data"), synthetic_seed=SEED)
            gen.generate(0, SCENES, ns, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=which == "B")
            if which == "A":
                generate_gt("ds", 0, SCENES, 2, root=str(base / "A"), overlap="hip")
            gather_gt("ds", 0, SCENES, root=str(base / which))
        out[ns] = (tree(str(base / "A")), tree(str(base / "B")), base)
    return out


@pytest.mark.parametrize("ns", [1, 2])
def test_one_pass_leaves_the_files_of_two(runs, ns):
    a, b, _ = runs[ns]
    assert sorted(a) == sorted(b)
    kinds = {os.path.splitext(n)[1] for n in a}
    assert {".ply", ".png", ".txt", ".log"} <= kinds and len(a) >= SCENES * (7 + 3 * ns) + 1
    for name in sorted(a):
        assert a[name] == b[name], name
    for i in range(SCENES):
        assert "ds/data/scene-{:0>6d}/gt.log".format(i) in b
    lines = a["ds/metadata/gt.log"].decode().splitlines()
    assert len(lines) >= 1                                                             # the reference path alone yields pairs
    for line in lines:
        name, s, t, o1, o2 = line.split("\t")
        assert name.startswith("scene-") and (s, t) == ("0", "1") and len(o1.split(".")[1]) == 4 and len(o2.split(".")[1]) == 4


@pytest.mark.parametrize("ns", [1, 2])
def test_two_lanes_leave_the_same_files(runs, nets, ns, tmp_path):
    from pointreggpt_amd.generator import Generator, gather_gt
    (diff, mask), lane = nets
    gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(tmp_path / "ds" / "data"), synthetic_seed=SEED)
    stats = {}
    gen.generate(0, SCENES, ns, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=True, lanes=[lane], stats=stats)
    gather_gt("ds", 0, SCENES, root=str(tmp_path))
    assert stats["lanes"] == 2 and stats["pairs"] == SCENES
    assert tree(str(tmp_path)) == runs[ns][1]


def test_a_second_run_skips_and_keeps_every_gt_log(runs, nets, capsys):
    from pointreggpt_amd.generator import Generator
    (diff, mask), _lane = nets
    _, b, base = runs[2]
    data = base / "B" / "ds" / "data"
    before = {p: os.stat(p).st_mtime_ns for p in map(str, data.glob("scene-*/gt.log"))}
    assert len(before) == SCENES
    capsys.readouterr()
    gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(data), synthetic_seed=SEED)
    gen.generate(0, SCENES, 2, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=True)
    printed = capsys.readouterr().out
    assert printed.count("Skip completed scene") == 2                                 # batches [0, 1] and [2]
    assert {p: os.stat(p).st_mtime_ns for p in before} == before
    assert tree(str(base / "B")) == b


def test_cli_with_gt_then_generate_gt_is_the_two_pass_result(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--dataset_name", "ds", "-start", "0", "-stop", str(SCENES)]
    gen = [sys.executable, os.path.join(ROOT, "generate_dataset.py"), "--resume", "synthetic:3", "--synthetic", str(SEED), "--image_size",
           str(S), "--sampling_timesteps", str(STEPS), "--batch_size", str(BATCH), "--dim", str(DIM), "--mask_threshold", "0.5",
           "--streams", "1"] + common
    gt = [sys.executable, os.path.join(ROOT, "generate_gt.py"), "--disable_tqdm"] + common
    logs = {}
    for which, extra in (("two", []), ("one", ["--with_gt"])):
        cwd = tmp_path / which
        cwd.mkdir()
        r = subprocess.run(gen + extra, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        made = sorted(p.name for p in (cwd / "ds" / "data").glob("scene-*/gt.log"))
        assert len(made) == (SCENES if extra else 0)
        r = subprocess.run(gt, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.count("scene gt log has existed") == (SCENES if extra else 0)
        logs[which] = (cwd / "ds" / "metadata" / "gt.log").read_bytes()
    assert logs["one"] == logs["two"] and len(logs["two"].splitlines()) >= 1
