"""Overlap-targeted poses on an MI355X: prg_pose_candidate_counts against its twin and the numpy definition, exactly, and one
end-to-end run of `Generator.generate(overlap=(0.1, 0.3))` and `PairStream(overlap=...)`.  Run with `-m gpu`.

Kernel part: the cases of tests/_pose_search.py (B = 3 with an empty scene, rows from {1, 63, 64, 65, 257, 5000}, N in {1, 5,
33}, 16 x 16 and 8 x 24, offsets[0] > 0, ties, NaN rows).  The counts are integers from integer atomics: compared with ==.

End to end: synthetic seed 0, scenes 0..7 at 64 x 64, batches of 4 and of 8, dim-16 fp32 synthetic networks, 4 DDIM steps of 1000,
`mask_threshold=0.5`, `gt_log=True`, 16 candidates, spread 3, band [0.1, 0.3]; the same scenes once more with `overlap=None`.
DDNM keeps every reprojected pixel, so the realised overlap follows the pose whatever the networks in-paint."""
import os

import numpy as np
import pytest
import torch

from _pose_search import BOX, CASES, Z_TOL, case, spec
from pointreggpt_amd import cpu
from pointreggpt_amd import geometry as G
from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def cases():
    out = []
    for k in range(len(CASES)):
        c = case(k)
        c["want"] = cpu.ops.pose_candidate_counts(torch.from_numpy(c["pts"]), torch.from_numpy(c["offs"]), c["poses"], c["K"],
                                                  (c["H"], c["W"]), box=BOX, z_tol=Z_TOL).numpy()
        assert np.array_equal(c["want"], spec(c))                                   # twin == definition (also a CPU test)
        out.append(c)
    return out


# ---- 1. the kernels alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)))
def test_counts_equal_the_twin_for_every_chunking(cases, k):
    c = cases[k]
    one = 3 * c["H"] * c["W"] * 4                                                   # bytes of one candidate per scene
    pts, offs = D(c["pts"]), D(c["offs"])
    full = G.pose_candidate_counts(pts, offs, c["poses"], c["K"], (c["H"], c["W"]), box=BOX, z_tol=Z_TOL)
    assert full.dtype == torch.int32 and tuple(full.shape) == (3, c["N"], 3) and full.is_cuda
    got = full.cpu().numpy()
    print("case", k, "counts[0]", got[:, 0].tolist())
    assert np.array_equal(got, c["want"])
    for per_chunk in (1, 2, c["N"]):
        for extra in (0, one - 1):                                                  # a ragged tail of the workspace buys nothing
            part = G.pose_candidate_counts(pts, offs, c["poses"], c["K"], (c["H"], c["W"]), box=BOX, z_tol=Z_TOL,
                                           workspace_bytes=per_chunk * one + extra)
            assert np.array_equal(part.cpu().numpy(), c["want"]), (per_chunk, extra)
    nobox = G.pose_candidate_counts(pts, offs, c["poses"], c["K"], (c["H"], c["W"]), box=None, z_tol=0.0)
    assert np.array_equal(nobox.cpu().numpy(), spec(c, box=None, z_tol=0.0))
    assert np.array_equal(pts.cpu().numpy(), c["pts"], equal_nan=True)              # the cloud is read only
    assert np.array_equal(PP.pose_candidate_counts_hip(c["clouds"], c["poses"], c["K"], (c["H"], c["W"]), box=BOX, z_tol=Z_TOL),
                          c["want"])                                                # the host-cloud form of the same call


@pytest.mark.parametrize("k", [1, 5])
def test_covered_is_the_mask_count_of_project_points_zbuffer(cases, k):
    from pointreggpt_amd import _lib
    lib = _lib.load()
    c = cases[k]
    pts, offs, K = D(c["pts"]), D(c["offs"]), D(c["K"])
    for n in range(c["N"]):
        P = D(c["poses"][:, n])
        depth = torch.empty((3, 1, c["H"], c["W"]), dtype=torch.float32, device="cuda")
        mask = torch.empty((3, 1, c["H"], c["W"]), dtype=torch.uint8, device="cuda")
        _lib.check(lib.prg_project_points_zbuffer(_lib.ptr(pts), _lib.ptr(offs), _lib.ptr(P), _lib.ptr(K), _lib.ptr(depth),
                                                  _lib.ptr(mask), 3, c["H"], c["W"], 1.0, _lib.stream_ptr()))
        assert np.array_equal(mask.view(3, -1).sum(1).cpu().numpy(), c["want"][:, n, 2]), n


def test_garbage_in_counts_is_cleared_and_guard_words_stay(cases):
    from pointreggpt_amd import _lib
    lib = _lib.load()
    c = cases[4]                                                                    # N = 5, 8 x 24, a 5000-row scene
    B, N, H, W = 3, c["N"], c["H"], c["W"]
    GUARD, WORD = 16, 0x5EA1
    counts = torch.full((B * N * 3 + GUARD,), 0x7ABCDEF0, dtype=torch.int32, device="cuda")
    counts[B * N * 3:] = WORD
    ws_bytes = 2 * B * H * W * 4                                                    # two candidates per chunk: three chunks
    ws = torch.full((ws_bytes // 4 + GUARD,), WORD, dtype=torch.int32, device="cuda")
    pts, offs, P, K = D(c["pts"]), D(c["offs"]), D(c["poses"]), D(c["K"])
    box = np.concatenate([np.float32(BOX[0]), np.float32(BOX[1])])
    _lib.check(lib.prg_pose_candidate_counts(_lib.ptr(pts), _lib.ptr(offs), _lib.ptr(P), _lib.ptr(K), B, N, H, W, box.ctypes.data,
                                             Z_TOL, _lib.ptr(counts), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()),
               "prg_pose_candidate_counts")
    torch.cuda.synchronize()
    assert np.array_equal(counts[:B * N * 3].view(B, N, 3).cpu().numpy(), c["want"])
    assert bool((counts[B * N * 3:] == WORD).all()) and bool((ws[ws_bytes // 4:] == WORD).all())


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------
S, DIM, STEPS, SCENES, SEED = 64, 16, 4, 8, 0
BAND, CANDIDATES, SPREAD = (0.1, 0.3), 16, 3.0


def tree(root):
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def net():
    from pointreggpt_amd import _lib
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import MaskUnet, Unet
    _lib.load()
    unet = Unet(DIM, dtype="fp32").init_synthetic(3)
    mask = MaskUnet(DIM, dtype="fp32").init_synthetic(4, final_bias=8.0)
    diff = GaussianDiffusion(unet, image_size=S, timesteps=1000, sampling_timesteps=STEPS)
    yield diff, mask
    diff.close(); unet.close(); mask.close()


@pytest.fixture(scope="module")
def runs(net, tmp_path_factory):
    """The three datasets, each generated once: (root, stats, poses handed to the view step) for B = 4, B = 8 and overlap=None."""
    from pointreggpt_amd.generator import Generator
    diff, mask = net
    out = {}
    for name, batch, kw in (("b4", 4, dict(overlap=BAND, pose_candidates=CANDIDATES, pose_spread=SPREAD)),
                            ("b8", 8, dict(overlap=BAND, pose_candidates=CANDIDATES, pose_spread=SPREAD)), ("none", 8, {})):
        root = tmp_path_factory.mktemp(name)
        stats, seen = {}, []
        real = Generator._view

        def view(self, memory, pose, *a, _seen=seen, _real=real, **k):
            _seen.append(pose.copy())
            return _real(self, memory, pose, *a, **k)

        gen = Generator(diff, None, batch_size=batch, samples_folder=str(root / "ds" / "data"), synthetic_seed=SEED)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(Generator, "_view", view)
            gen.generate(0, SCENES, 1, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=True, stats=stats, **kw)
        out[name] = (root, stats, np.concatenate(seen, 0), gen)
    return out


def gt_lines(root):
    """scene -> (overlap_src, overlap_tgt) of the scenes generate_gt's filter keeps."""
    kept = {}
    for i in range(SCENES):
        text = (root / "ds" / "data" / "scene-{:0>6d}".format(i) / "gt.log").read_text()
        for line in text.splitlines():
            _name, s, t, o_s, o_t = line.split("\t")
            assert (s, t) == ("0", "1")
            kept[i] = (float(o_s), float(o_t))
    return kept


def test_chosen_poses_are_the_host_rule_on_the_same_candidates(runs):
    root, stats, used, gen = runs["b4"]
    K, _Kd, _d0, _pc, scene_pcs = gen._batch_setup(list(range(SCENES)), None)
    predicted = []
    for i in range(SCENES):
        cands = G.pose_candidates(SEED, i, 0, CANDIDATES, SPREAD)
        counts = PP.pose_candidate_counts([scene_pcs[i]], cands[None], K[i:i + 1], S, box=BOX, z_tol=Z_TOL)[0]
        c, r, ok = G.select_pose_candidates(counts, len(scene_pcs[i]), BAND)
        predicted.append((i, 1, r))
        assert np.array_equal(used[i], cands[c]), i
        txt = np.loadtxt(str(root / "ds" / "data" / "scene-{:0>6d}".format(i) / "sample-000001.pose.txt"))
        assert np.allclose(txt, np.linalg.inv(cands[c].astype(np.float64)), rtol=0, atol=1e-6), i         # pose.txt: the inverse
    print("predicted overlap_src", [round(p[2], 4) for p in predicted])
    assert stats["pose_search"]["predicted"] == predicted and stats["pose_search"]["views"] == SCENES
    # every predicted ratio is in band: the CPU probe behind this feature found a candidate for every scene of seed 0
    assert all(BAND[0] <= r <= BAND[1] for _i, _v, r in predicted) and stats["pose_search"]["in_band"] == SCENES
    assert np.array_equal(runs["b8"][2], used) and runs["b8"][1]["pose_search"] == stats["pose_search"]


def test_both_batch_sizes_write_the_same_bytes(runs):
    a, b = tree(str(runs["b4"][0])), tree(str(runs["b8"][0]))
    assert sorted(a) == sorted(b) and len(a) == SCENES * 10
    for name in a:
        assert a[name] == b[name], name
    base = tree(str(runs["none"][0]))
    assert any(a[n] != base[n] for n in a if n.endswith("pose.txt")) and "pose_search" not in runs["none"][1]


def test_more_kept_scenes_realise_a_low_overlap_than_without_the_search(runs):
    low = lambda kept: sorted(i for i, (o_s, _o_t) in kept.items() if 0.05 <= o_s <= 0.35)
    searched, baseline = gt_lines(runs["b4"][0]), gt_lines(runs["none"][0])
    predicted = {i: r for i, _v, r in runs["b4"][1]["pose_search"]["predicted"]}
    print("searched: kept", len(searched), "of", SCENES, "realised overlap_src", {i: v[0] for i, v in searched.items()})
    print("realised - predicted", {i: round(v[0] - predicted[i], 4) for i, v in searched.items()})
    print("baseline: kept", len(baseline), "of", SCENES, "realised overlap_src", {i: v[0] for i, v in baseline.items()})
    print("in [0.05, 0.35]: searched", low(searched), "baseline", low(baseline))
    assert len(low(searched)) > len(low(baseline))


def test_pair_stream_carries_the_predicted_overlap(runs, net):
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream
    diff, mask = net
    root, stats, _used, _gen = runs["b4"]
    gen = Generator(diff, None, batch_size=4, samples_folder=str(root / "stream"), synthetic_seed=SEED)
    stream = PairStream(gen, mask, start=0, stop=SCENES, noise_seed=SEED, mask_threshold=0.5, overlap=BAND, pose_candidates=CANDIDATES,
                        pose_spread=SPREAD)
    items = list(stream)
    kept = gt_lines(root)
    predicted = {i: r for i, _v, r in stats["pose_search"]["predicted"]}
    assert sorted(it["scene"] for it in items) == sorted(kept)
    for it in items:
        assert it["predicted_overlap"] == (predicted[it["scene"]],)
        assert "{:.4f}".format(it["overlap_src"]) == "{:.4f}".format(kept[it["scene"]][0])
        assert np.array_equal(it["src"], PP.read_ply(str(root / "ds" / "data" / "scene-{:0>6d}".format(it["scene"]) / "sample-000000.cloud.ply")))
    plain = next(iter(PairStream(gen, mask, start=0, stop=4, noise_seed=SEED, mask_threshold=0.5)))
    assert "predicted_overlap" not in plain
