"""`PairStream`: finished cloud pairs straight from the GPU, with their ground-truth correspondences, and no file in between.

A registration network (Predator, CoFiNet, GeoTransformer) trains at batch size 1, a few iterations per second; one MI355X
generates more pairs than that.  Instead of ~13 files per scene on disk and a KD-tree per item in the loader
(`get_correspondences` of the example loaders), iterate a `PairStream`: it runs `Generator.generate`'s device sequence for
`num_samples = 1` batch by batch and yields, per surviving scene, the two finished clouds — the rows `generate(gt_log=True)`
writes to `sample-000000.cloud.ply` / `sample-000001.cloud.ply` — the two overlap ratios behind the scene's `gt.log` line, and
`corr`, every (row of src, row of tgt) within `matching_radius` (`geometry.radius_pairs_ragged`; INTEGRATION.md says how the
loaders' lists map onto it).

    stream = PairStream(generator, mask_unet, start=0, stop=100000, noise_seed=7, matching_radius=0.0375, to="torch")
    for item in stream:
        item["scene"], item["src"], item["tgt"], item["overlap_src"], item["overlap_tgt"], item["corr"]

Reproducibility: a scene's item has the bits of the file path (`generate(start, stop, 1, gt_log=True, noise_seed=...)`) for the
same `batch_size`, `start` and seeds.  `noise_seed` is required: besides the diffusion noise it seeds, with real-data input, the
pose stream per (job seed, first scene of the batch) exactly as `generate(noise_seed=...)` does — the batches, and so the
poses, are the same only for the same `start` and `batch_size`.  There is no unseeded mode here.

Augmentation: `PairStream(..., augment=Augment(...), epoch=e)` applies the registration loaders' per-item augmentation on the
device — a random pose, the cut to a point limit, uniform per-point noise — keyed per (noise_seed, scene, epoch), and searches
`corr` on the augmented clouds under the ground-truth `transform` (see `Augment`).  With `augment=None` (the default) the
items are exactly the ones described above.

Several views per scene: `PairStream(..., num_samples=k, clouds="per_view")` runs k views per scene as `generate` does (the
scene memory updated on the device between the views) and yields, per scene and in `itertools.combinations` order, one item for
every pair (s, t) of the scene's k + 1 clouds that gets a `gt.log` line — the rows of the files s and t of `generate(...,
num_samples=k, clouds="per_view", gt_log=True)`, the line's two ratios, `corr` of exactly these two clouds — with the two
extra keys `src_idx` = s and `tgt_idx` = t; `skipped` names every dropped pair as (scene, "pair (s, t): <reason>").  An
augmented item of pair (s, t) draws from its own keys (`synthetic.augment_seed_pair(..., pair=(s, t))`).  With `clouds="fused"` (the
default) and `num_samples=k` the stream yields the one fused pair per scene that `generate(num_samples=k, gt_log=True)` writes.

Overlap-targeted poses: `PairStream(..., overlap=(lo, hi), pose_candidates=16, pose_spread=3.0)` chooses every view's pose as
`generate(overlap=...)` does (`Generator._view_poses`: candidates keyed per (seed, scene, view), scored against the scene's
source frame on the device) and adds `predicted_overlap` to every item of the scene: a tuple with the predicted share of seen
source rows of each of its views, in view order.  With `overlap=None` (the default) nothing is scored and the key is absent.

Normals: `PairStream(..., normals=Normals(radius=0.1, limit=30))` adds `src_normals` and `tgt_normals` to every item: float64,
one row per row of `src` / `tgt`, `geometry.estimate_normals` of the clouds the item holds — after the augmentation's move,
cut and noise when `augment` is set — every cloud oriented towards the camera centre of the view that produced it, in the frame
the cloud is handed out in; the two centres are the item's `src_camera` and `tgt_camera` (3 float64 each).  All clouds of a
batch go through one search and one kernel launch.  With `normals=None` (the default) every item is exactly the one described
above.  A fused target of several views has no single camera: `clouds="fused"` with `num_samples > 1` raises.

The stream runs on the calling thread's current HIP stream.  It uses no writer pool and no lanes, writes no file and creates
nothing under the generator's `samples_folder` (the folder itself is `Generator.__init__`'s doing).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import postprocess as PP
from . import synthetic
from .scene_memory import DeviceMemory
from .sharding import index_batches


@dataclass(frozen=True)
class Augment:
    """What the example loaders (Predator, CoFiNet, GeoTransformer) do to an item before they search its correspondences.

    noise: both clouds get uniform per-point noise strictly inside (-noise/2, noise/2) per axis (the loaders' `augment_noise`);
    point_limit: a cloud with more rows is cut to that many by a random permutation (None: never);
    rotation: None — the clouds stay in their common frame, `transform` is the identity and nothing is drawn; "src" — the
      source is moved by a uniform random pose, `src_aug = (src - t) @ R`; "both" — a second uniform rotation R2 moves the target
      too, `tgt_aug = tgt @ R2.T`;
    translation: the standard deviation of the Gaussian t, in metres."""
    noise: float = 0.005
    point_limit: Optional[int] = 30000
    rotation: Optional[str] = "src"
    translation: float = 1.0

    def __post_init__(self):
        if self.rotation not in (None, "src", "both"):
            raise ValueError("rotation must be None, 'src' or 'both'")
        if not (np.isfinite(self.translation) and self.translation >= 0):
            raise ValueError("translation must be finite and >= 0")
        PP._check_augment(self.noise, self.point_limit)


@dataclass(frozen=True)
class Normals:
    """Per-point normals for the items of a `PairStream`: the PCA normal of a row's `limit` nearest rows within `radius` of its
    own cloud, itself included (open3d's KDTreeSearchParamHybrid(radius, max_nn=limit)), oriented towards the cloud's camera —
    `postprocess.estimate_normals` states the arithmetic."""
    radius: float = 0.1
    limit: int = 30

    def __post_init__(self):
        if not (np.isfinite(self.radius) and self.radius > 0):
            raise ValueError("radius must be finite and > 0")
        if int(self.limit) != self.limit or not 3 <= self.limit <= 1024:
            raise ValueError("limit must be an integer in 3..1024")


def uniform_rotation(rng: np.random.Generator) -> np.ndarray:
    """A rotation uniform on SO(3) (Haar measure) by the loaders' construction: the Q of the QR decomposition of a 3x3 Gaussian
    matrix, its columns signed so that R's diagonal is positive, the whole negated if that leaves a reflection."""
    z = rng.standard_normal((3, 3))
    while np.linalg.matrix_rank(z) != 3:
        z = rng.standard_normal((3, 3))
    q, r = np.linalg.qr(z)
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def augment_poses(noise_seed: int, scene: int, epoch: int, augment: Augment, pair=None):
    """The poses of one scene's item -> (move_src, move_tgt, transform): float64 4x4 matrices built on the host, a move being
    None for a cloud that stays where it is.  `src_aug = rigid_move(src, move_src)`, `tgt_aug = rigid_move(tgt, move_tgt)`, and
    `transform` takes the augmented source into the augmented target's frame.

    Drawn from `np.random.Generator(np.random.Philox(key=synthetic.augment_seed_pair(noise_seed, scene, 2, pair), counter=[0, 0, 0,
    epoch]))` (`pair`: the (s, t) of an item of a scene with per-view clouds; None or (0, 1): today's key) in this order: R (`uniform_rotation`), t = standard_normal(3) * translation, and for "both" R2.  "src":
    move_src = [[R^T, -R^T t], [0, 1]] (the loaders' `(src - t) @ R`), transform = [R | t].  "both": move_tgt = [R2 | 0],
    transform = R2 [R | t]."""
    if augment.rotation is None:
        return None, None, np.eye(4)
    rng = np.random.Generator(np.random.Philox(key=synthetic.augment_seed_pair(noise_seed, scene, 2, pair), counter=[0, 0, 0, int(epoch)]))
    R = uniform_rotation(rng)
    t = rng.standard_normal(3) * float(augment.translation)
    move_src, transform = np.eye(4), np.eye(4)
    move_src[:3, :3], move_src[:3, 3] = R.T, -(R.T @ t)
    transform[:3, :3], transform[:3, 3] = R, t
    move_tgt = None
    if augment.rotation == "both":
        move_tgt = np.eye(4)
        move_tgt[:3, :3] = uniform_rotation(rng)
        transform = move_tgt @ transform
    return move_src, move_tgt, transform


class PairStream:
    def __init__(self, generator, depth_correction, *, start: int, stop: int, noise_seed: int,
                 matching_radius: Optional[float] = None, mask_threshold: float = 0.99, has_refine_step: bool = False,
                 save_voxel_size: float = 0.025, to: str = "numpy", augment: Optional[Augment] = None, epoch: int = 0,
                 num_samples: int = 1, clouds: str = "fused", memory_voxel_size: float = 0.002, overlap=None,
                 pose_candidates: int = 16, pose_spread: float = 3.0, normals: Optional[Normals] = None):
        if to not in ("numpy", "torch"):
            raise ValueError("to must be 'numpy' or 'torch'")
        if generator.device.type == "cpu":
            raise ValueError("PairStream needs the clouds on a HIP device (Generator(device='cuda'))")
        if noise_seed is None:
            raise ValueError("PairStream needs a noise_seed (it also seeds the real-data pose stream per batch)")
        if matching_radius is not None and not (np.isfinite(matching_radius) and matching_radius > 0):
            raise ValueError("matching_radius must be finite and > 0 (or None for no correspondences)")
        if augment is not None and not isinstance(augment, Augment):
            raise ValueError("augment must be a stream.Augment (or None)")
        if not 0 <= int(epoch) < 2 ** 32:
            raise ValueError("epoch must fit 32 bits")
        if clouds not in ("fused", "per_view"):
            raise ValueError("clouds must be 'fused' or 'per_view'")
        if int(num_samples) < 1:
            raise ValueError("num_samples must be >= 1")
        if normals is not None and not isinstance(normals, Normals):
            raise ValueError("normals must be a stream.Normals (or None)")
        if normals is not None and clouds == "fused" and int(num_samples) > 1:
            raise ValueError("normals= needs one camera per cloud: a fused target of several views has none, use clouds=\"per_view\"")
        self.normals = normals
        self.num_samples, self.per_view, self.memory_voxel_size = int(num_samples), clouds == "per_view", memory_voxel_size
        self.search = generator._pose_search(overlap, pose_candidates, pose_spread, int(noise_seed), True)
        self.augment, self.epoch = augment, int(epoch)
        self.generator = generator
        self.depth_correction = depth_correction
        self.start, self.stop = int(start), int(stop)
        self.noise_seed = int(noise_seed)
        self.matching_radius = None if matching_radius is None else float(matching_radius)
        self.mask_threshold = mask_threshold
        self.has_refine_step = has_refine_step
        self.save_voxel_size = save_voxel_size
        self.to = to
        self.skipped: List[Tuple[int, str]] = []     # (scene, reason) of the pairs generate_gt's filter drops

    # -- the device sequence of one batch: the set-up, view step and scene memory of Generator._lane, no file, no image copy -----
    @torch.no_grad()
    def _batch(self, idxs, info_train):
        gen = self.generator
        K, K_dev, _depth0, param_cond, scene_pcs = gen._batch_setup(idxs, info_train)
        memory = DeviceMemory.upload(gen.G, scene_pcs, gen.device)
        views, poses = [], []
        source = None if self.search is None else gen._search_source(memory, scene_pcs)
        self._predicted = [() for _ in idxs]                                                   # per scene: one ratio per view
        for sample_idx in range(self.num_samples):
            pose, found = gen._view_poses(idxs, sample_idx, self.noise_seed, K, source, self.search)
            if found is not None:
                self._predicted = [p + (r,) for p, (r, _ok) in zip(self._predicted, found)]
            seeds = [synthetic.noise_seed(self.noise_seed, i, sample_idx) for i in idxs]
            _rpj, _rpj_c, _images, xyz, valid = gen._view(memory, pose, K, K_dev, param_cond, gen.model, self.depth_correction, seeds,
                                                          self.mask_threshold, self.has_refine_step)
            views.append((xyz, valid))
            poses.append(pose)
            if sample_idx < self.num_samples - 1:                                              # memory update (sd:2661-2680)
                memory.update(xyz, valid, self.memory_voxel_size)
                memory.settle(["scene-{:0>6d}".format(i) for i in idxs])
        self._poses = poses                                                                    # per view: (B,4,4), for the cameras
        return gen._finish_pairs_launch(memory, views, poses, self.per_view, self.save_voxel_size)

    def _cameras(self, keep, moves):
        """(2 * len(keep), 3) float64: the camera centre of every cloud of the surviving pairs, in the frame the cloud is handed
        out in.  Cloud 0 of a scene is its source frame, seen from the origin of the common frame; cloud i >= 1 is view i, whose
        pose takes the common frame into the camera's, so its centre is the translation of the inverse pose (the float64 inverse
        `_finish_pairs_launch` moves the cloud back with).  moves[k]: the augmentation's (move_src, move_tgt) of pair k, or None."""
        cams = np.zeros((2 * len(keep), 3), dtype=np.float64)
        for k, (j, s, t) in enumerate(keep):
            for c, i in enumerate((s, t)):
                if i >= 1:
                    cams[2 * k + c] = np.linalg.inv(self._poses[i - 1][j].astype(np.float64))[:3, 3]
                if moves is not None and moves[k][c] is not None:
                    cams[2 * k + c] = PP.rigid_move(cams[2 * k + c], moves[k][c])[0]
        return cams

    # -- the loaders' augmentation of the surviving pairs of a batch: one launch for all of them -------------------------------
    def _augment(self, pts, sizes, scenes, pairs):
        """pts / sizes: the ragged buffer of the pairs (segments 2k, 2k+1 = src, tgt of scenes[k]; pairs[k] = the (s, t) behind
        them, or None) -> (augmented buffer, its sizes, int32 rows, [transform per pair])."""
        aug, G_ = self.augment, self.generator.G
        n = len(scenes)
        T = np.tile(np.eye(4), (2 * n, 1, 1))
        has_T = np.zeros(2 * n, dtype=np.uint8)
        seeds, transforms, self._moves = [], [], []
        for k, scene in enumerate(scenes):
            moves = augment_poses(self.noise_seed, scene, self.epoch, aug, pairs[k])
            for c in (0, 1):
                if moves[c] is not None:
                    T[2 * k + c], has_T[2 * k + c] = moves[c], 1
                seeds.append(synthetic.augment_seed_pair(self.noise_seed, scene, c, pairs[k]))
            transforms.append(moves[2])
            self._moves.append(moves[:2])
        res = G_.augment_clouds(pts, sizes, seeds=seeds, draw=self.epoch, noise=aug.noise, limit=aug.point_limit,
                                T=T if has_T.any() else None, has_T=has_T if has_T.any() else None)
        if aug.point_limit is not None:
            sizes = np.minimum(sizes, int(aug.point_limit))
        return res["points"], sizes, res["rows"], transforms

    def __iter__(self):
        gen = self.generator
        self.skipped = []
        info_train = gen._train_info()
        for idxs in index_batches(self.start, self.stop, gen.batch_size):
            batch, finished = len(idxs), self._batch(idxs, info_train)
            fin = finished.points
            offs, d_offs, cnt = gen._finish_pairs_words(finished, idxs)          # the one copy of the small words
            n = (len(offs) - 1) // batch                                         # clouds per scene
            keep, ratios = [], []                                                # keep: (scene of the batch, s, t)
            for j, s, t, r, why in gen._pair_walk(offs, d_offs, cnt, batch):
                if r is None:
                    self.skipped.append((idxs[j], "pair ({}, {}): {}".format(s, t, why) if self.per_view else why))
                else:
                    keep.append((j, s, t))
                    ratios.append(r)
            if not keep:
                continue
            # one ragged buffer of the surviving pairs: segments (2k, 2k+1) = the clouds (s, t) of keep[k]
            segs = [n * j + c for j, s, t in keep for c in (s, t)]
            sizes = np.array([offs[a + 1] - offs[a] for a in segs], dtype=np.int64)
            k_offs = np.zeros(len(sizes) + 1, dtype=np.int64)
            k_offs[1:] = np.cumsum(sizes)
            if n == 2 and len(keep) == batch:
                pts = fin[int(offs[0]):int(offs[-1])]
            else:
                pts = torch.cat([fin[int(offs[a]):int(offs[a + 1])] for a in segs], dim=0)
            rows = transforms = None
            if self.augment is not None:
                pts, sizes, rows, transforms = self._augment(pts, sizes, [idxs[j] for j, _s, _t in keep],
                                                             [(s, t) if self.per_view else None for _j, s, t in keep])
                k_offs[1:] = np.cumsum(sizes)
            corr = c_offs = None
            if self.matching_radius is not None:
                d_offs = torch.from_numpy(k_offs).to(pts.device)
                search = pts.contiguous()
                if transforms is not None:           # the correspondences hold under the ground truth: a moved copy of the sources
                    T = np.tile(np.eye(4), (2 * len(keep), 1, 1))
                    T[0::2] = transforms
                    search, _ = gen.G.rigid_crop_ragged(search, None, d_offs, T=T, has_T=np.tile(np.array([1, 0], np.uint8), len(keep)))
                corr, c_offs = gen.G.radius_pairs_ragged(search, d_offs, len(keep), int(sizes.max()), self.matching_radius)
                c_offs = c_offs.cpu().numpy()
            normals = cams = None
            if self.normals is not None:             # last: on the clouds the items hold, one search and one launch per batch
                cams = self._cameras(keep, None if self.augment is None else self._moves)
                normals = gen.G.estimate_normals(pts, sizes, radius=self.normals.radius, limit=self.normals.limit, viewpoints=cams)
            if self.to == "numpy":
                normals = None if normals is None else normals.cpu().numpy()
                pts = pts.cpu().numpy()
                rows = None if rows is None else rows.cpu().numpy()
                corr = None if corr is None else corr.cpu().numpy()
                own = np.copy
            else:
                cams = None if cams is None else torch.from_numpy(cams).to(pts.device)
                own = torch.clone
            for k, (j, s, t) in enumerate(keep):
                item = dict(scene=idxs[j], src=own(pts[k_offs[2 * k]:k_offs[2 * k + 1]]), tgt=own(pts[k_offs[2 * k + 1]:k_offs[2 * k + 2]]),
                            overlap_src=ratios[k][0], overlap_tgt=ratios[k][1])
                if self.per_view:
                    item["src_idx"], item["tgt_idx"] = s, t
                if self.search is not None:
                    item["predicted_overlap"] = self._predicted[j]
                if corr is not None:
                    item["corr"] = own(corr[c_offs[k]:c_offs[k + 1]])
                if rows is not None:
                    item["transform"] = transforms[k] if self.to == "numpy" else torch.from_numpy(transforms[k]).to(pts.device)
                    item["src_rows"] = own(rows[k_offs[2 * k]:k_offs[2 * k + 1]])
                    item["tgt_rows"] = own(rows[k_offs[2 * k + 1]:k_offs[2 * k + 2]])
                if normals is not None:
                    item["src_normals"] = own(normals[k_offs[2 * k]:k_offs[2 * k + 1]])
                    item["tgt_normals"] = own(normals[k_offs[2 * k + 1]:k_offs[2 * k + 2]])
                    item["src_camera"], item["tgt_camera"] = own(cams[2 * k]), own(cams[2 * k + 1])
                yield item
