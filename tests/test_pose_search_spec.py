"""Overlap-targeted poses without a GPU: the numpy definition of the candidate scores (`postprocess.pose_candidate_counts`)
against its native twin (prg_cpu_pose_candidate_counts) bit for bit, the properties the definition promises, the mistakes the
test inputs tell apart, the selection rule, the keying of the candidates, and the generator on the CPU twins — the default
path byte for byte what it was, and `overlap=(lo, hi)` choosing the poses the host rule selects.

Everything is integers or bytes: no tolerance is involved."""
import os

import numpy as np
import pytest
import torch

from _pose_search import BOX, CASES, Z_TOL, case, spec
from pointreggpt_amd import cpu
from pointreggpt_amd import geometry as G
from pointreggpt_amd import postprocess as PP


def twin(clouds, poses, K, S, **kw):
    pts, offs = cpu.ops.upload_clouds(clouds)
    return cpu.ops.pose_candidate_counts(pts, offs, poses, K, S, **kw).numpy()


@pytest.fixture(scope="module")
def cases():
    cs = [case(k) for k in range(len(CASES))]
    for c in cs:
        c["want"] = spec(c)
    return cs


# ---- the definition against the twin ---------------------------------------------------------------------------------------------
def test_spec_equals_twin_on_the_kernel_cases(cases):
    for c in cases:
        pts, offs = torch.from_numpy(c["pts"]), torch.from_numpy(c["offs"])               # offsets[0] > 0, poisoned head and tail
        got = cpu.ops.pose_candidate_counts(pts, offs, c["poses"], c["K"], (c["H"], c["W"]), box=BOX, z_tol=Z_TOL).numpy()
        assert got.dtype == np.int32 and got.shape == (3, c["N"], 3)
        assert np.array_equal(got, c["want"])
        assert np.array_equal(twin(c["clouds"], c["poses"], c["K"], (c["H"], c["W"])), spec(c, box=None))     # and without a box
    # the cases are not degenerate: all three counts differ somewhere, the tolerance and the box both bite
    every = np.concatenate([c["want"].reshape(-1, 3) for c in cases])
    assert (every[:, 1] < every[:, 0]).any() and (every[:, 2] < every[:, 0]).any() and (every[:, 1] > 0).any()


def test_spec_equals_twin_on_random_ragged_inputs():
    rng = np.random.default_rng(7)
    for trial in range(6):
        B, N = int(rng.integers(1, 5)), int(rng.integers(1, 7))
        H, W = int(rng.integers(3, 20)), int(rng.integers(3, 20))
        clouds = [(rng.normal(size=(int(n), 3)) * [1.0, 0.8, 0.9] + [0, 0, 2.2]).astype(np.float32) for n in rng.integers(0, 400, B)]
        poses = np.stack([G.pose_candidates(trial, b, 1, N, 2.0) for b in range(B)])
        K = np.zeros((B, 3, 3), dtype=np.float32)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = rng.uniform(5, 30, B), rng.uniform(5, 30, B), W / 2, H / 2
        tol = float(rng.choice([0.0, 0.0375, 0.5]))
        for box in (None, BOX):
            assert np.array_equal(twin(clouds, poses, K, (H, W), box=box, z_tol=tol),
                                  PP.pose_candidate_counts(clouds, poses, K, (H, W), box=box, z_tol=tol))


def test_fma32_is_the_exact_fused_multiply_add():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=2000).astype(np.float32), rng.normal(size=2000).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.normal(size=2000) * 1e-7)).astype(np.float32)        # heavy cancellation
    got = PP._fma32(a, b, c)
    for x, y, z, g in zip(a[:400], b[:400], c[:400], got[:400]):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(exact - Fraction(float(g))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))


# ---- properties ------------------------------------------------------------------------------------------------------------------
def both(clouds, poses, K, S, **kw):
    a = PP.pose_candidate_counts(clouds, poses, K, S, **kw)
    assert np.array_equal(a, twin(clouds, poses, K, S, **kw))
    return a


def test_covered_is_the_mask_count_of_the_projection(cases):
    for c in cases:
        lib = cpu.load()                               # (`cpu.ops.project_clouds` makes square images: the entry point takes H and W)
        pts, offs = cpu.ops.upload_clouds(c["clouds"])
        Kt = torch.from_numpy(c["K"])
        for k in range(c["N"]):
            P = torch.from_numpy(np.ascontiguousarray(c["poses"][:, k]))
            depth = torch.empty((3, 1, c["H"], c["W"]), dtype=torch.float32)
            mask = torch.empty((3, 1, c["H"], c["W"]), dtype=torch.uint8)
            cpu.check(lib.prg_cpu_project_points_zbuffer(pts.data_ptr(), offs.data_ptr(), P.data_ptr(), Kt.data_ptr(), depth.data_ptr(),
                                                         mask.data_ptr(), 3, c["H"], c["W"], 1.0))
            assert np.array_equal(mask.view(3, -1).sum(1).numpy(), c["want"][:, k, 2])


def test_unprojected_depth_map_under_the_identity_is_seen_whole():
    S = 24
    rng = np.random.default_rng(0)
    depth = rng.uniform(0.06, 0.4, (2, 1, S, S)).astype(np.float32)                 # 0.6 .. 4 m: every pixel valid
    K = np.zeros((2, 3, 3), dtype=np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = (21.5, 27.25), (22.0, 26.5), S / 2, S / 2, 1
    pc, valid = cpu.ops.depth2pc_tensor(torch.from_numpy(depth) * 10, torch.from_numpy(K), clip=(0.5, 10))
    assert bool(valid.all())
    clouds = [pc[b].numpy() for b in range(2)]
    eye = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1, 1))
    got = both(clouds, eye, K, S, box=None, z_tol=0.0)
    assert got.tolist() == [[[S * S] * 3]] * 2                                      # in_frame == seen == covered == rows


K1 = np.array([[[10.0, 0, 8], [0, 10.0, 8], [0, 0, 1]]], dtype=np.float32)
EYE = np.eye(4, dtype=np.float32)[None, None]


def test_ties_tolerance_edge_and_box_edges():
    tol = np.float32(Z_TOL)
    z0 = np.float32(2.0)
    edge = np.float32(z0 + tol)                                                     # exactly zmin + z_tol in float32: seen
    behind = np.nextafter(edge, np.float32(np.inf))                                 # 3.75 cm + 1 ulp behind: not seen
    rows = np.array([[0, 0, z0], [0, 0, z0], [0, 0, edge], [0, 0, behind]], dtype=np.float32)
    assert both([rows[:2]], EYE, K1, 16, z_tol=Z_TOL).tolist() == [[[2, 2, 1]]]     # coincident rows both count as seen
    assert both([rows[:3]], EYE, K1, 16, z_tol=Z_TOL).tolist() == [[[3, 3, 1]]]
    assert both([rows], EYE, K1, 16, z_tol=Z_TOL).tolist() == [[[4, 3, 1]]]
    assert both([rows], EYE, K1, 16, z_tol=0.0).tolist() == [[[4, 2, 1]]]
    # box edges are inclusive, one ulp outside is out — in float32, on each side of each axis
    lo, hi = np.float32([-0.5, -0.25, 1.0]), np.float32([0.5, 0.25, 3.0])
    mid = np.float32([0.1, 0.05, 2.0])
    for axis in range(3):
        for bound, out in ((lo, -np.inf), (hi, np.inf)):
            on, off = mid.copy(), mid.copy()
            on[axis] = bound[axis]
            off[axis] = np.nextafter(bound[axis], np.float32(out))
            assert both([on[None]], EYE, K1, 16, box=(lo, hi)).tolist() == [[[1, 1, 1]]], (axis, out)
            assert both([off[None]], EYE, K1, 16, box=(lo, hi)).tolist() == [[[1, 0, 1]]], (axis, out)


def test_the_box_is_tested_on_the_moved_row():
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 1.0                                                                   # the candidate shifts the cloud 1 m along x
    lo, hi = np.float32([0.9, -1, 1]), np.float32([1.1, 1, 3])
    row = np.float32([[0.0, 0.0, 2.0]])                                             # outside the box before the move, inside after
    assert both([row], T[None, None], K1, 16, box=(lo, hi)).tolist() == [[[1, 1, 1]]]
    assert PP.pose_candidate_counts([row], T[None, None], K1, 16, box=(lo, hi), box_frame="source").tolist() == [[[1, 0, 1]]]


def test_nan_rows_rows_behind_the_camera_and_empty_clouds_count_nowhere():
    rows = np.float32([[np.nan, 0, 2], [0, np.nan, 2], [0, 0, np.nan], [0, 0, 0.0], [0, 0, -2.0], [0.1, 0.1, 2.0]])
    assert both([rows], EYE, K1, 16).tolist() == [[[1, 1, 1]]]
    assert both([rows[:5]], EYE, K1, 16).tolist() == [[[0, 0, 0]]]
    assert both([np.zeros((0, 3), np.float32), rows[5:]], np.tile(EYE, (2, 3, 1, 1)), np.tile(K1, (2, 1, 1)), 16).tolist() == \
        [[[0, 0, 0]] * 3, [[1, 1, 1]] * 3]
    assert both([np.float32([[100.0, 0, 2.0]])], EYE, K1, 16).tolist() == [[[0, 0, 0]]]          # out of frame


# ---- mutations: mistakes the kernel cases tell apart ----------------------------------------------------------------------------
def chunked(c, chunk, skip_last=False):
    """The definition evaluated the way the call works through a small workspace: `chunk` candidates at a time."""
    out = np.zeros_like(c["want"])
    starts = list(range(0, c["N"], chunk))
    for c0 in (starts[:-1] if skip_last else starts):
        part = dict(c, poses=c["poses"][:, c0:c0 + chunk])
        out[:, c0:c0 + chunk] = spec(part)
    return out


def test_chunking_the_definition_changes_nothing(cases):
    for c in cases:
        for chunk in (1, 2, c["N"]):
            assert np.array_equal(chunked(c, chunk), c["want"])


MUTATIONS = {
    "tolerance dropped": lambda c: spec(c, z_tol=0.0),
    "box tested in the source frame": lambda c: spec(c, box_frame="source"),
    "candidate c + 1's pose": lambda c: spec(dict(c, poses=np.roll(c["poses"], -1, axis=1))),
    "scene b + 1's K": lambda c: spec(dict(c, K=np.roll(c["K"], -1, axis=0))),
    "rows and columns swapped": lambda c: spec(c, swap_rc=True),
    "the last chunk skipped": lambda c: chunked(c, 2, skip_last=True),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_every_mutation_changes_the_counts_on_the_kernel_cases(cases, name):
    changed = [k for k, c in enumerate(cases) if not np.array_equal(MUTATIONS[name](c), c["want"])]
    print(name, "changes cases", changed)
    assert changed
    if name == "rows and columns swapped":
        assert all(cases[k]["H"] != cases[k]["W"] for k in changed) and len(changed) == 3         # every 8 x 24 case, no square one


# ---- the selection rule ------------------------------------------------------------------------------------------------------------
def counts_of(seen):
    return np.array([[s + 5, s, 1] for s in seen], dtype=np.int32)


def test_selection_rule():
    sel = G.select_pose_candidates
    assert sel(counts_of([50, 20, 25, 10]), 100, (0.1, 0.3)) == (1, 0.2, True)              # the FIRST in band, not the best centred
    assert sel(counts_of([10, 30]), 100, (0.1, 0.3)) == (0, 0.1, True)                      # the band's ends are inside
    assert sel(counts_of([31, 30]), 100, (0.1, 0.3)) == (1, 0.3, True)
    assert sel(counts_of([50, 40, 2, 45]), 100, (0.1, 0.3)) == (2, 0.02, False)             # nearest: 0.08 below beats 0.10 above
    assert sel(counts_of([50, 45, 0]), 100, (0.1, 0.3)) == (2, 0.0, False)
    assert sel(counts_of([75, 0, 75, 0]), 100, (0.25, 0.5)) == (0, 0.75, False)             # ties (0.25 exactly, either side) go to the
    assert sel(counts_of([0, 75, 0, 75]), 100, (0.25, 0.5)) == (0, 0.0, False)              # lowest index
    assert sel(counts_of([0, 40]), 100, (0.1, 0.3)) == (0, 0.0, False)
    assert sel(counts_of([0, 0, 0]), 0, (0.1, 0.3)) == (0, 0.0, False)                      # no rows: candidate 0
    assert sel(counts_of([0, 0]), 0, (0.0, 0.3)) == (0, 0.0, True)
    c, r, ok = sel(counts_of([1, 2]), 3, (0.3, 0.4))
    assert (c, ok) == (0, True) and r == 1 / 3                                              # float64 on the host
    for bad in ((0.3, 0.1), (0.2, 0.2), (-0.1, 0.3), (0.1, 1.5), (float("nan"), 0.5), 0.3, (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError):
            G.check_overlap_band(bad)
    assert G.check_overlap_band([0, 1]) == (0.0, 1.0)


# ---- the candidates --------------------------------------------------------------------------------------------------------------
def test_candidates_are_keyed_by_seed_scene_and_view_alone():
    a = G.pose_candidates(7, 3, 0, 16, 3.0)
    assert a.shape == (16, 4, 4) and a.dtype == np.float32
    assert np.array_equal(a, G.pose_candidates(7, 3, 0, 16, 3.0))
    assert np.array_equal(a[:5], G.pose_candidates(7, 3, 0, 5, 3.0))                        # a shorter list is a prefix
    for other in (G.pose_candidates(8, 3, 0, 16, 3.0), G.pose_candidates(7, 4, 0, 16, 3.0), G.pose_candidates(7, 3, 1, 16, 3.0)):
        assert not np.array_equal(a, other)
    # the documented draw order, restated: per candidate theta, phi, then three normals from the (seed, scene, "pose", view) stream
    from scipy.spatial.transform import Rotation
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([7, 3, 0x706F7365, 0])))
    for c in range(3):
        th, ph = (rng.random() * (np.pi / 12) - np.pi / 24) * 3.0, (rng.random() * (np.pi / 6) - np.pi / 12) * 3.0
        jit = rng.standard_normal(3) / 3 * 3.0
        R = Rotation.from_euler("XYZ", [th, ph, 0.0]).as_matrix()
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, np.array([0, 0, 3.0]) - R @ np.array([0, 0, 3.0]) + [jit[0], jit[1], 0.0]
        assert np.array_equal(a[c], T.astype(np.float32))
    for bad in (dict(n=0), dict(spread=0.0), dict(spread=float("nan")), dict(seed=-1)):
        with pytest.raises(ValueError):
            G.pose_candidates(**dict(dict(seed=7, scene=3, sample_idx=0, n=4, spread=1.0), **bad))


def test_spread_one_stays_inside_the_reference_ranges():
    from scipy.spatial.transform import Rotation
    T = np.concatenate([G.pose_candidates(1, s, 0, 64, 1.0) for s in range(8)]).astype(np.float64)
    ang = Rotation.from_matrix(T[:, :3, :3]).as_euler("XYZ")
    assert np.abs(ang[:, 0]).max() <= np.pi / 24 + 1e-6 and np.abs(ang[:, 1]).max() <= np.pi / 12 + 1e-6
    assert np.abs(ang[:, 2]).max() < 1e-6
    assert np.abs(ang[:, 0]).max() > 0.8 * np.pi / 24 and np.abs(ang[:, 1]).max() > 0.8 * np.pi / 12      # and fills them
    c = np.array([0, 0, 3.0])
    jitter = T[:, :3, 3] - (c - T[:, :3, :3] @ c)
    assert np.abs(jitter[:, 2]).max() < 1e-6 and 0.25 < jitter[:, :2].std() < 0.42                    # sigma = 1/3 m, xy only
    wide = np.concatenate([G.pose_candidates(1, s, 0, 64, 3.0) for s in range(8)]).astype(np.float64)
    assert np.abs(Rotation.from_matrix(wide[:, :3, :3]).as_euler("XYZ")[:, 1]).max() > np.pi / 12


# ---- the generator on the CPU twins ------------------------------------------------------------------------------------------------
S, DIM, STEPS, SEED, SCENES = 32, 16, 2, 5, 3


def tree(root):
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def nets():
    unet = cpu.Unet(DIM).init_synthetic(3)
    mask = cpu.MaskUnet(DIM).init_synthetic(4, final_bias=8.0)
    return cpu.GaussianDiffusion(unet, image_size=S, timesteps=1000, sampling_timesteps=STEPS), mask


def generate(nets, folder, batch, **kw):
    from pointreggpt_amd.generator import Generator
    diff, mask = nets
    gen = Generator(diff, None, batch_size=batch, samples_folder=str(folder / "ds" / "data"), synthetic_seed=SEED, device="cpu")
    gen.generate(0, SCENES, 2, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, clouds="per_view", **kw)
    return gen


def test_default_is_unchanged_and_scores_nothing(nets, tmp_path, monkeypatch):
    generate(nets, tmp_path / "plain", 2)

    def never(*_a, **_k):
        raise AssertionError("overlap=None must not score or draw candidates")

    monkeypatch.setattr(cpu.ops, "pose_candidate_counts", staticmethod(never))
    monkeypatch.setattr(cpu.ops, "pose_candidates", staticmethod(never))
    stats = {}
    generate(nets, tmp_path / "none", 2, overlap=None, pose_candidates=7, pose_spread=2.0, stats=stats)
    a, b = tree(str(tmp_path / "plain")), tree(str(tmp_path / "none"))
    assert sorted(a) == sorted(b) and len(a) > SCENES * 9
    for name in a:
        assert a[name] == b[name], name
    assert "pose_search" not in stats


def test_overlap_on_the_cpu_chooses_what_the_host_rule_selects(nets, tmp_path, capsys):
    from pointreggpt_amd.generator import Generator
    band, n, spread = (0.2, 0.6), 6, 2.0
    stats = {}
    seen = []
    real = Generator._view

    def view(self, memory, pose, *a, **k):
        seen.append(pose.copy())
        return real(self, memory, pose, *a, **k)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(Generator, "_view", view)
        gen = generate(nets, tmp_path / "b2", 2, overlap=band, pose_candidates=n, pose_spread=spread, stats=stats)
    assert "pose search: 6 views" in capsys.readouterr().out
    generate(nets, tmp_path / "b3", 3, overlap=band, pose_candidates=n, pose_spread=spread)
    a, b = tree(str(tmp_path / "b2")), tree(str(tmp_path / "b3"))
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)                      # the batch size changes no byte
    # the poses of every (scene, view), restated from the definition, the source frames and the rule
    _K, _Kd, _d0, _pc, scene_pcs = gen._batch_setup(list(range(SCENES)), None)
    K = _K
    used = {(i, v): p for v, batch in ((0, seen[0]), (1, seen[1])) for i, p in zip((0, 1), batch)}
    used.update({(2, 0): seen[2][0], (2, 1): seen[3][0]})
    want_stats = []
    for i in range(SCENES):
        for v in range(2):
            cands = G.pose_candidates(SEED, i, v, n, spread)
            counts = PP.pose_candidate_counts([scene_pcs[i]], cands[None], K[i:i + 1], S, box=BOX, z_tol=Z_TOL)[0]
            c, r, _ok = G.select_pose_candidates(counts, len(scene_pcs[i]), band)
            assert np.array_equal(used[(i, v)], cands[c]), (i, v)
            want_stats.append((i, v + 1, r))
            txt = np.loadtxt(str(tmp_path / "b2" / "ds" / "data" / "scene-{:0>6d}".format(i) / "sample-{:0>6d}.pose.txt".format(v + 1)))
            assert np.allclose(txt, np.linalg.inv(cands[c].astype(np.float64)), rtol=0, atol=1e-6)
            assert np.allclose(txt @ cands[c].astype(np.float64), np.eye(4), atol=1e-5)
    ps = stats["pose_search"]
    assert ps["views"] == 6 and ps["predicted"] == want_stats and ps["in_band"] == sum(band[0] <= r <= band[1] for _i, _v, r in want_stats)


def test_overlap_needs_a_seed_with_real_data(tmp_path):
    from pointreggpt_amd.generator import Generator

    class _Diff:
        image_size = 32

    gen = Generator(_Diff(), str(tmp_path), samples_folder=str(tmp_path / "out"), synthetic_seed=None, device="cpu")
    with pytest.raises(ValueError, match="seed"):
        gen.generate(0, 1, 1, overlap=(0.1, 0.3))                                       # no noise_seed: seed_poses resolves to False
    with pytest.raises(ValueError, match="seed"):
        gen.generate(0, 1, 1, overlap=(0.1, 0.3), noise_seed=3, seed_poses=False)
    for bad in (dict(overlap=(0.3, 0.1)), dict(overlap=(0.1, 0.3), pose_candidates=0), dict(overlap=(0.1, 0.3), pose_spread=0.0)):
        with pytest.raises(ValueError):
            gen.generate(0, 1, 1, noise_seed=3, **bad)
