"""Inputs shared by tests/test_pose_search_spec.py (CPU: the numpy definition, the twin, the mutations) and
tests/test_gpu_pose_search.py (the kernels): the cases on which prg_pose_candidate_counts must equal its twin exactly.

Every case: B = 3 scenes, one of them empty, cloud sizes from {1, 63, 64, 65, 257, 5000} (the edges of a wave and of a 256-row
slab, and a cloud of many slabs), N in {1, 5, 33} candidates, a 16 x 16 image or an 8 x 24 one (H != W: a row / column swap shows),
a different K per scene, offsets[0] > 0 in front of poisoned rows, duplicated rows (ties for a pixel's nearest depth) and NaN rows.
The clouds fill a frustum a little wider than the crop box and the frame, so every test of the definition has rows on both sides."""
import numpy as np

from pointreggpt_amd import geometry as G
from pointreggpt_amd import postprocess as PP

BOX = (PP.BBOX_MIN, PP.BBOX_MAX)
Z_TOL = 0.0375
HEAD, TAIL = 7, 5
SIZES = (1, 63, 64, 65, 257, 5000)
CASES = [  # (N, (H, W), rows of the three scenes)
    (1, (16, 16), (5000, 0, 1)),
    (5, (16, 16), (63, 257, 0)),
    (33, (16, 16), (0, 64, 65)),
    (1, (8, 24), (257, 0, 5000)),
    (5, (8, 24), (0, 5000, 63)),
    (33, (8, 24), (65, 1, 0)),
]


def cloud(rng, n):
    pts = np.stack([rng.uniform(-1.8, 1.8, n), rng.uniform(-1.8, 1.8, n), rng.uniform(0.3, 3.8, n)], axis=1).astype(np.float32)
    if n >= 63:
        pts[5] = pts[17]                    # coincident rows: a tie wherever they land
        pts[n // 2] = np.nan                # NaN rows count nowhere
        pts[n - 2, 2] = np.nan
        pts[9, 2] = -pts[9, 2]              # behind the camera for the identity, maybe not for every candidate
    return pts


def intrinsics(H, W):
    K = np.zeros((3, 3, 3), dtype=np.float32)
    for b, f in enumerate((0.9, 1.1, 1.4)):  # a different camera per scene
        K[b, 0, 0], K[b, 1, 1] = f * W, f * 1.07 * H
        K[b, 0, 2], K[b, 1, 2], K[b, 2, 2] = W / 2 - 0.25 * b, H / 2 + 0.5 * b, 1.0
    return K


def case(k):
    """-> dict(clouds, pts (ragged buffer with poisoned head and tail rows), offs, poses (3,N,4,4), K (3,3,3), H, W, N)."""
    N, (H, W), sizes = CASES[k]
    rng = np.random.default_rng(100 + k)
    clouds = [cloud(rng, n) for n in sizes]
    offs = np.zeros(4, dtype=np.int64)
    offs[0] = HEAD
    offs[1:] = HEAD + np.cumsum(sizes)
    poison = np.full((1, 3), 2.0, dtype=np.float32)      # in front of every camera: a row read by mistake lands in a frame
    pts = np.concatenate([np.repeat(poison, HEAD, 0)] + clouds + [np.repeat(poison, TAIL, 0)], 0)
    poses = np.stack([G.pose_candidates(5, 10 * k + b, 0, N, 3.0) for b in range(3)])
    return dict(clouds=clouds, pts=pts, offs=offs, poses=poses, K=intrinsics(H, W), H=H, W=W, N=N)


def spec(c, **kw):
    kw.setdefault("box", BOX)
    kw.setdefault("z_tol", Z_TOL)
    return PP.pose_candidate_counts(c["clouds"], c["poses"], c["K"], (c["H"], c["W"]), **kw)
