"""`pointreggpt_amd.scene_memory` and the one gt.log rule / one pair walk of `pointreggpt_amd.generator`.

Without a GPU: `HostMemory`'s update against its arithmetic written out, the pair rule on a table of border cases through both of
its callers (`Generator._pair_ratios_at`, `generator._finish_gt`), the walk over a finished batch's pairs.  On an MI355X (`-m
gpu`): `DeviceMemory` against `HostMemory`, bit for bit."""
from itertools import combinations

import numpy as np
import pytest
import torch

from pointreggpt_amd import generator as GEN
from pointreggpt_amd import postprocess as PP
from pointreggpt_amd.generator import Generator
from pointreggpt_amd.scene_memory import DeviceMemory, HostMemory, HostRows


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- HostMemory ------------------------------------------------------------------------------------------------------------------
def test_host_memory_update_is_concatenate_grid_float32():
    rng = np.random.default_rng(5)
    v = 0.05
    start = [rng.uniform(-1, 1, (300, 3)).astype(np.float32), rng.uniform(-1, 1, (1, 3)).astype(np.float32)]
    mem = HostMemory(None, start, "cpu")
    want = list(start)
    # view 1: scene 0 gains rows, scene 1 none (it stays its single row); view 2: nothing is valid anywhere
    views = [(rng.uniform(-1, 1, (2, 400, 3)), np.stack([rng.random(400) < 0.6, np.zeros(400, bool)])),
             (rng.uniform(-1, 1, (2, 400, 3)), np.zeros((2, 400), bool))]
    for xyz, valid in views:
        mem.update(torch.from_numpy(xyz), torch.from_numpy(valid), v)
        mem.settle(["a", "b"], HostRows.copy(torch.from_numpy(xyz), torch.from_numpy(valid)))
        before = mem.clouds()[1]
        mem.settle_scene(0)                                            # scene by scene: the other one is untouched meanwhile
        assert mem.clouds()[1] is before
        mem.settle_scene(1)
        want = [PP.native_voxel_down_sample(np.concatenate([old, xyz[j][valid[j]]], axis=0), v).astype(np.float32)
                for j, old in enumerate(want)]
        got = mem.clouds()
        for j in range(2):
            assert got[j].dtype == np.float32 and got[j].shape == want[j].shape and np.array_equal(bits32(got[j]), bits32(want[j]))
    assert len(want[0]) > 1 and np.array_equal(bits32(mem.clouds()[1]), bits32(start[1]))
    mem.settle(["a", "b"], None)                                       # nothing queued: nothing happens
    mem.settle_scene(0)
    assert np.array_equal(bits32(mem.clouds()[0]), bits32(want[0]))


# ---- the gt.log rule -------------------------------------------------------------------------------------------------------------
# (rows of a, rows of b, (count, down-sampled rows) of a, of b, the two ratios, kept)
RULE = [(999, 1000, (5, 10), (5, 10), (0.5, 0.5), False),
        (1000, 999, (5, 10), (5, 10), (0.5, 0.5), False),
        (1000, 1000, (5, 10), (5, 10), (0.5, 0.5), True),
        (1000, 1000, (0, 0), (5, 10), (float("nan"), 0.5), False),          # 0 / 0
        (1000, 1000, (999, 10000), (999, 10000), (0.0999, 0.0999), False),
        (1000, 1000, (100, 1000), (5, 100), (0.1, 0.05), True),             # exactly 0.1 is not below 0.1
        (1000, 1000, (3, 10), (0, 10), (0.3, 0.0), True)]


def expected_line(name, s, t, ratios):
    return "{}\t{}\t{}\t{:.4f}\t{:.4f}\n".format(name, s, t, ratios[0], ratios[1])


def test_pair_rule_through_pair_ratios_at():
    for rows_a, rows_b, (ca, da), (cb, db), ratios, kept in RULE:
        offs, d_offs = np.array([0, rows_a, rows_a + rows_b]), np.array([0, da, da + db])
        got, why = Generator._pair_ratios_at(offs, d_offs, np.array([ca, cb]), 0, 1)
        assert Generator._pair_ratios(offs, d_offs, np.array([[ca, cb]]), 0) == (got, why)
        if kept:
            assert why is None and got == ratios
            assert Generator.GT_LINE.format("scene-000007", 0, 1, *got) == expected_line("scene-000007", 0, 1, ratios)
        else:
            assert got is None and isinstance(why, str) and why
        assert (Generator._pair_dropped(rows_a, rows_b, *ratios) is None) == kept


def test_pair_rule_through_finish_gt(tmp_path, monkeypatch):
    """One scene per case and one scene with all of them as its pairs, `compute_overlap_ratio` patched to the table's ratios."""
    todo = [("scene-{:0>6d}".format(i), tmp_path / "scene-{:0>6d}".format(i) / "gt.log",
             [(0, 1, np.zeros((ra, 3)), np.zeros((rb, 3)))]) for i, (ra, rb, *_rest) in enumerate(RULE)]
    todo.append(("scene-000099", tmp_path / "scene-000099" / "gt.log",
                 [(i, i + 1, np.zeros((ra, 3)), np.zeros((rb, 3))) for i, (ra, rb, *_rest) in enumerate(RULE)]))
    answers = iter([case[4] for case in RULE] * 2)
    monkeypatch.setattr(PP, "compute_overlap_ratio", lambda src, tgt: next(answers))
    GEN._finish_gt(todo, "numpy-spec")
    for i, case in enumerate(RULE):
        assert (tmp_path / "scene-{:0>6d}".format(i) / "gt.log").read_text() == \
            (expected_line("scene-{:0>6d}".format(i), 0, 1, case[4]) if case[5] else "")
    assert (tmp_path / "scene-000099" / "gt.log").read_text() == \
        "".join(expected_line("scene-000099", i, i + 1, case[4]) for i, case in enumerate(RULE) if case[5])


# ---- the pair walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_pair_walk_is_scene_major_combinations_over_the_pair_table(n, monkeypatch):
    B = 2
    offs = np.arange(n * B + 1) * 2000
    d_offs = np.arange(n * B + 1) * 100
    cnt = np.arange(B * len(list(combinations(range(n), 2))) * 2).reshape(-1, 2) + 50
    seen = []

    def ratios_at(cls, offs_, d_offs_, cnt_, a, b):
        seen.append((tuple(cnt_), a, b))
        return (0.5, 0.5), None

    monkeypatch.setattr(Generator, "_pair_ratios_at", classmethod(ratios_at))
    walked = list(Generator._pair_walk(offs, d_offs, cnt, B))
    assert [(j, s, t) for j, s, t, _r, _w in walked] == [(j, s, t) for j in range(B) for s, t in combinations(range(n), 2)]
    assert all(r == (0.5, 0.5) and w is None for _j, _s, _t, r, w in walked)
    table = Generator._pair_table(B, n, "cpu").numpy()                  # the rows prg_overlap_counts_indexed counts in
    assert table.dtype == np.int32 and table.tolist() == [list(r) for r in Generator._pair_rows(B, n)]
    assert seen == [(tuple(cnt[p]), int(a), int(b)) for p, (a, b) in enumerate(table)]
    assert [(n * j + s, n * j + t) for j, s, t, _r, _w in walked] == [tuple(r) for r in table.tolist()]


def test_two_clouds_per_scene_go_through_pair_ratios(monkeypatch):
    B = 2
    offs, d_offs, cnt = np.arange(2 * B + 1) * 2000, np.arange(2 * B + 1) * 100, np.full((B, 2), 50)
    called = []

    def picky(cls, offs_, d_offs_, cnt_, j):
        called.append(j)
        return (None, "turned away") if j == 1 else ((0.25, 0.75), None)

    monkeypatch.setattr(Generator, "_pair_ratios", classmethod(picky))
    assert list(Generator._pair_walk(offs, d_offs, cnt, B)) == [(0, 0, 1, (0.25, 0.75), None), (1, 0, 1, None, "turned away")]
    assert called == [0, 1]


# ---- DeviceMemory against HostMemory ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_memory_is_host_memory_bit_for_bit():
    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    _lib.load()
    B, S, v = 3, 32, 0.02
    rng = np.random.default_rng(9)
    clouds = [rng.uniform([-1.0, -1.0, 1.0], [1.0, 1.0, 3.0], (n, 3)).astype(np.float32) for n in (2000, 300, 1)]
    K = np.tile(np.array([[30.0, 0, 16.0], [0, 30.0, 16.0], [0, 0, 1]], dtype=np.float32), (B, 1, 1))
    K_dev = torch.from_numpy(K).cuda()
    names = ["scene-a", "scene-b", "scene-c"]
    dev, host = DeviceMemory.upload(G, clouds, "cuda"), HostMemory(G, clouds, "cuda")
    assert dev.rows0 == [2000, 300, 1] and dev.mem_pts0 is dev.pts and dev.mem_offs0 is dev.offs

    def same():
        got, want = dev.clouds(), host.clouds()
        for j in range(B):
            assert got[j].dtype == np.float32 and got[j].shape == want[j].shape and np.array_equal(bits32(got[j]), bits32(want[j])), j

    def same_projection():
        pose = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
        pose[:, :3, 3] = rng.uniform(-0.1, 0.1, (B, 3))
        a, b = dev.project(pose, K, S, 0.1), host.project(pose, K, S, 0.1)
        assert a[1].any() and torch.equal(a[1], b[1]) and np.array_equal(bits32(a[0].cpu().numpy()), bits32(b[0].cpu().numpy()))
        return pose

    for step in range(2):
        pose = same_projection()                                       # of the uploaded clouds, then after the first settle
        depth = torch.from_numpy(rng.uniform(0.06, 0.3, (B, 1, S, S)).astype(np.float32))
        if step == 1:
            depth[1] = 0                                               # scene b: nothing of the second view is valid
        xyz, valid = G.unproject_f64(depth.cuda(), K_dev, torch.from_numpy(pose).cuda())
        assert bool(valid[0].any()) and bool(valid[1].any()) == (step == 0)
        for mem in (dev, host):
            mem.update(xyz, valid, v)
            mem.settle(names, HostRows.copy(xyz, valid))
            for j in range(B):
                mem.settle_scene(j)
        same()
    same_projection()                                                  # after the second settle, with the all-invalid scene
    assert dev.mem_pts0.shape[0] == 2301 and dev.pts is not dev.mem_pts0      # the source frames are kept as they were uploaded
    xyz = xyz.clone()
    xyz[1, 5, 2] = float("nan")
    valid = valid.clone()
    valid[1, 5] = True
    dev.update(xyz, valid, v)
    with pytest.raises(_lib.PrgError, match="scene-b"):
        dev.settle(names)
