"""`Generator.generate` (sd:2250-2694) on the HIP hot path: same sequence, same on-disk layout, batched geometry.

Per batch of scenes: source depth frame -> scene "memory" cloud (crop box) -> sample-000000.cloud.ply; for each sample:
random pose -> z-buffer reprojection of the memory clouds (ONE launch for the ragged batch) -> depth correction ->
DDNM condition -> diffusion sampler -> depth correction -> float64 unprojection into the common frame -> fragment
-> crop / voxel / sample-000001.cloud.ply, plus the pose / intrinsic / png side files the reference writes.

Input side: `--synthetic` scenes (pointreggpt_amd.synthetic; what tests and benchmarks use — neither box has 3DMatch)
or the reference's real-data layout (train_info.pkl + `<cloud>.info.txt` + 3DMatch RGB-D frames, sd:2352-2459).
The real-data decode path mirrors torchvision Resize(NEAREST)/CenterCrop/ToTensor with PIL and is parity-unpinned.

Sharding: scenes are independent; under torchrun every rank takes a contiguous block of the requested range
(pointreggpt_amd.sharding) — the reference leaves this to manual -start/-stop.
sd = /root/reference/denoising_diffusion_pytorch/successive_ddnm_diffusion.py
"""
from __future__ import annotations

import functools
import os
import pickle
import shutil
import sys
import threading
from itertools import combinations
from pathlib import Path
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import geometry as G
from . import postprocess as PP
from . import synthetic
from .scene_memory import DeviceMemory, HostMemory, HostRows
from .sharding import index_batches

PAIRS_PER_LAP = 20642   # real pairs per lap of the scene index; src/tgt swap on odd laps (sd:2397-2410)


class FinishedPairs(NamedTuple):
    """What `_finish_pairs_launch` leaves on the device, n clouds per scene, scene-major."""
    points: torch.Tensor          # the finished clouds, one ragged float64 buffer
    offsets: torch.Tensor         # (nB+1) int64
    status_save: torch.Tensor     # (nB) voxel statuses of the finish at save_voxel_size
    status_gt: torch.Tensor       # (nB) voxel statuses of the grid at GT_VOXEL
    counts: torch.Tensor          # (B * C(n, 2), 2) overlap counts, in `_pair_rows` order
    down_offsets: torch.Tensor    # (nB+1) int64 offsets of the clouds down-sampled at GT_VOXEL


class PoseSearch(NamedTuple):
    """`generate(overlap=...)`: the overlap target of a run, checked by `Generator._pose_search`."""
    band: tuple                   # (lo, hi) of the predicted overlap of the source cloud
    n: int                        # candidates per (scene, view)
    spread: float                 # multiplies the reference's pose ranges
    seed: int                     # keys the candidate streams: the synthetic seed, or noise_seed with real data


class Generator:
    def __init__(self, diffusion_model, folder: Optional[str], *, batch_size=16, samples_folder="./samples",
                 results_folder="./results", synthetic_seed: Optional[int] = None, device="cuda", **_ignored):
        self.model = diffusion_model                  # pointreggpt_amd.diffusion.GaussianDiffusion
        self.folder = folder
        self.batch_size = int(batch_size)
        self.image_size = diffusion_model.image_size
        self.samples_folder = Path(samples_folder)
        self.samples_folder.mkdir(parents=True, exist_ok=True)
        self.results_folder = Path(results_folder)
        self.synthetic_seed = synthetic_seed
        self.device = torch.device(device)
        # device ops: the HIP library (default; raises without a GPU) or, ONLY when asked for with device="cpu", the
        # prg_cpu_* twins (BASELINE configs[0]: the plumbing run that needs no GPU)
        if self.device.type == "cpu":
            from . import cpu as _cpu
            self.G = _cpu.ops
        else:
            self.G = G

    # -- weights (sd:2307-2324): the generator samples from the EMA copy ------------------------------------------
    def load(self, milestone, unet=None):
        from .weights import unet_state_from_checkpoint
        data = torch.load(str(self.results_folder / f"model-{milestone}.pt"), map_location="cpu")
        net = unet if unet is not None else self.model.model
        net.load_state_dict(unet_state_from_checkpoint(data, net.cfg))

    # -- input side ------------------------------------------------------------------------------------------------
    def _real_scene(self, abs_idx: int, info_train, scene_dir: Path):
        """Source frame of scene `abs_idx` from the 3DMatch layout (sd:2397-2459).  Returns depth (S,S) f32 in
        10 m units and K (3,3) f32."""
        from PIL import Image
        S = self.image_size
        lap_odd = (abs_idx // PAIRS_PER_LAP) % 2 == 1
        rel = info_train["tgt" if lap_odd else "src"][abs_idx % PAIRS_PER_LAP]
        info_path = os.path.join("./dataset/indoor/data", rel).replace(".pth", ".info.txt")
        with open(info_path) as f:
            scene_name, seq_name, f0, _f1 = f.readline().rstrip("\n").split()
        root = os.path.join(self.folder, scene_name)
        K = G.intrinsic_transform(np.loadtxt(os.path.join(root, "camera-intrinsics.txt")), resize=S,
                                  centercrop=S).astype(np.float32)
        img = Image.open(os.path.join(root, seq_name, "frame-{:0>6d}.depth.png".format(int(f0))))
        w, h = img.size                                   # Resize(S): short side -> S (sd:2356-2361)
        if w <= h:
            nw, nh = S, int(S * h / w)
        else:
            nw, nh = int(S * w / h), S
        img = img.resize((nw, nh), Image.NEAREST)
        left, top = int(round((nw - S) / 2.0)), int(round((nh - S) / 2.0))
        img = img.crop((left, top, left + S, top + S))
        depth = np.asarray(img).astype(np.float32) * np.float32(1e-4)      # uint16 mm -> 10 m units
        depth[depth > 1] = 0
        return depth, K

    def _train_info(self):
        """The real-data scene index (sd:2352); None with synthetic input."""
        if self.synthetic_seed is not None:
            return None
        with open("./dataset/indoor/metadata/train_info.pkl", "rb") as f:
            return pickle.load(f)

    def _scene_inputs(self, abs_idx: int, info_train, scene_dir: Path):
        if self.synthetic_seed is not None:
            depth, K, _pose = synthetic.synth_scene(self.synthetic_seed, abs_idx, self.image_size)
            return depth, K
        return self._real_scene(abs_idx, info_train, scene_dir)

    def _poses(self, idxs: List[int], sample_idx: int, pose_seed: Optional[int] = None) -> np.ndarray:
        if self.synthetic_seed is None:
            if pose_seed is not None:          # reproducible and shard-invariant: a LOCAL legacy stream per (job, batch, sample)
                from .sharding import batch_pose_seed                      # (the process-wide numpy state is left alone)
                rs = np.random.RandomState(batch_pose_seed(pose_seed, idxs[0], sample_idx))
                return G.random_sample_pose(len(idxs), rng=rs).astype(np.float32)
            with Generator._pose_lock:         # numpy's legacy GLOBAL stream, as the reference (single lane only)
                return G.random_sample_pose(len(idxs)).astype(np.float32)
        out = []
        for i in idxs:                                                      # shard-invariant per-scene stream
            rng = synthetic.scene_rng(self.synthetic_seed, i)
            rng.random(4096 + 64 * sample_idx)                              # decorrelate from the depth draw
            out.append(synthetic.synth_pose(rng))
        return np.stack(out)

    # -- overlap-targeted poses: candidates scored against the source frame before a chain is spent on one -----------------------
    def _pose_search(self, overlap, pose_candidates, pose_spread, noise_seed, seed_poses) -> Optional["PoseSearch"]:
        """The `overlap=` / `pose_candidates=` / `pose_spread=` keywords of `generate` and `PairStream`, checked -> what
        `_view_poses` takes; None for overlap=None."""
        if overlap is None:
            return None
        band = G.check_overlap_band(overlap)
        if int(pose_candidates) != pose_candidates or not 1 <= pose_candidates <= 65535:
            raise ValueError("pose_candidates must be an integer in 1..65535")
        if not (np.isfinite(pose_spread) and pose_spread > 0):
            raise ValueError("pose_spread must be finite and > 0")
        if self.synthetic_seed is None and not seed_poses:
            raise ValueError("overlap=(lo, hi) needs a seed to key the pose candidates: pass noise_seed (numpy's global stream, "
                             "seed_poses=False, cannot)")
        seed = self.synthetic_seed if self.synthetic_seed is not None else noise_seed
        return PoseSearch(band, int(pose_candidates), float(pose_spread), int(seed))

    def _search_source(self, memory, scene_pcs):
        """The clouds the candidates are scored against, a batch's source frames as one ragged float32 buffer -> (pts, offs, rows):
        `DeviceMemory`'s `mem_pts0` / `mem_offs0`, which are on the device already; otherwise the list, uploaded (with
        device="cpu": laid out for the twin)."""
        if isinstance(memory, DeviceMemory):
            return memory.mem_pts0, memory.mem_offs0, memory.rows0
        return (*self.G.upload_clouds(scene_pcs, self.device), [len(c) for c in scene_pcs])

    def _view_poses(self, idxs, sample_idx, pose_seed, K, source, search):
        """The poses of one view of a batch -> (pose (B,4,4) float32, predicted): `_poses`' draw and None without a search; with
        one, per scene the candidate `select_pose_candidates` picks from `pose_candidates(seed, scene, sample_idx, n, spread)`,
        all B * n scored against the scenes' source frames by ONE `pose_candidate_counts` call — box = the crop box, z_tol =
        0.0375 — and the host learns B * n * 3 integers in one blocking copy.  predicted: [(ratio, in band), ...] per scene."""
        if search is None:
            return self._poses(idxs, sample_idx, pose_seed), None
        pts, offs, rows = source
        cands = np.stack([self.G.pose_candidates(search.seed, i, sample_idx, search.n, search.spread) for i in idxs])
        counts = self.G.pose_candidate_counts(pts, offs, cands, K, self.image_size, box=(PP.BBOX_MIN, PP.BBOX_MAX),
                                              z_tol=G.POSE_Z_TOL).cpu().numpy()
        pose, predicted = np.empty((len(idxs), 4, 4), dtype=np.float32), []
        for j in range(len(idxs)):
            c, r, ok = self.G.select_pose_candidates(counts[j], rows[j], search.band)
            pose[j] = cands[j, c]
            predicted.append((r, ok))
        return pose, predicted

    # -- the pipeline ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, start_scene_index, stop_scene_index, num_samples, memory_voxel_size=0.002,
                 save_voxel_size=0.025, has_refine_step=False, depth_correction=None, mask_threshold=0.99,
                 noise_seed: Optional[int] = None, progress: bool = False, writer_threads: int = 0, stats: Optional[dict] = None,
                 seed_poses: Optional[bool] = None, lanes: Optional[list] = None, voxel_backend: str = "device",
                 gt_log: bool = False, clouds: str = "fused", overlap=None, pose_candidates: int = 16, pose_spread: float = 3.0):
        """Same sequence as sd:2363-2694.  File output is asynchronous: every batch's clouds / images / text files are
        handed to the library's C++ writer pool (crop, voxel grid, PLY / PNG encoding on worker threads) and are
        produced while the GPU samples the next batch.  A batch's resume marker — the generated cloud of its LAST scene
        (sd:2371-2381) — is submitted only after everything else of that batch is on disk, so an interrupted run never
        skips an incomplete batch.

        ``lanes``: extra (GaussianDiffusion, MaskUnet) pairs holding THE SAME weights on their own library handles.  With
        n lanes (this object's model + ``depth_correction`` is lane 0) the batches are dealt round-robin to n host threads,
        each on its own HIP stream: a batch is still one B-scene launch sequence, but the launch boundaries, ramps and
        drains of one lane (139 kernels per U-Net evaluation) are filled by the other lane's kernels (+7 % pairs/s measured
        at B = 64, 128x128).  A scene's files do not depend on the lane that produced it.
        ``seed_poses`` (real-data input only): draw the poses from a local legacy stream per (job seed, batch, sample) so that
        a run can be re-sharded / resumed reproducibly; False = numpy's global stream like the reference (single lane only).
        Default: True when the caller passes a `noise_seed` (ANY value, 0 included: `None` is the "no seed" sentinel) or lanes,
        False (the reference's unseeded behaviour) otherwise.
        ``voxel_backend`` (num_samples > 1): where the scene memory lives between views (`scene_memory`): "device" (the default
        on a HIP device), `DeviceMemory`, no copy of the memory cloud to the host; "host", `HostMemory` (the only path of a
        `device="cpu"` generator).  Both produce the same bytes.
        ``gt_log`` (HIP device only, `voxel_backend="device"`): finish both clouds of every scene on the GPU and write the
        scene's ``gt.log`` in the batch that sampled it — the line `generate_gt` would write after re-reading the two PLY files.
        The memory clouds are uploaded once (also for num_samples == 1), the float64 views stay on the device, and
        `_finish_pairs_launch` does the rest; the clouds come to the host once for the PLY writers (write-only jobs).  Every file
        has the bytes of the default path followed by `generate_gt`; a batch's gt.log files are on disk before its resume marker
        is submitted.  Afterwards `generate_gt` finds every scene done and only `gather_gt` is left.
        ``clouds``: "fused" (the default, the reference's layout): all `num_samples` views of a scene end in ONE target cloud,
        sample-000001.cloud.ply, finished in the first view's camera frame.  "per_view": every view i = 1..num_samples gets its
        own sample-{i:06d}.cloud.ply — `postprocess.finish_cloud(xyz_i[valid_i], pre=pose_i, crop=the box, voxel=save_voxel_size,
        post=inv(pose_i))`, the view alone in its own camera frame — so that `generate_gt(num_samples=k+1)`, or `gt_log=True`
        in the same pass, lists up to C(k+1, 2) pairs per scene for k chains.  Every other file and the memory update between
        the views are the same in both modes, and for num_samples == 1 so are the clouds.
        ``overlap``: None (the default) draws one pose per (scene, view) as the reference does — the code path, the calls and every
        file's bytes of a run that never mentions the keyword.  (lo, hi) with 0 <= lo < hi <= 1 chooses every view's pose for the
        overlap it is PREDICTED to give (`_view_poses`): ``pose_candidates`` candidates per (scene, view) from
        `geometry.pose_candidates` — the reference's pose ranges times ``pose_spread`` — are scored against the scene's source
        frame on the device (`geometry.pose_candidate_counts`), and the first whose share of seen source rows lies in [lo, hi]
        goes exactly where the drawn pose went: the view step, pose.txt, the finish.  The candidates are keyed by (seed, scene,
        view) — the synthetic seed, or `noise_seed` with real data — and depend on nothing else; real data with
        `seed_poses=False` raises ValueError.  `stats["pose_search"]` = {views, in_band, predicted: [(scene, view, ratio), ...]},
        and each rank prints one summary line."""
        if voxel_backend not in ("device", "host"):
            raise ValueError("voxel_backend must be 'device' or 'host'")
        if clouds not in ("fused", "per_view"):
            raise ValueError("clouds must be 'fused' or 'per_view'")
        if gt_log and (self.device.type == "cpu" or voxel_backend != "device"):
            raise ValueError("gt_log=True needs the clouds on a HIP device (device='cuda', voxel_backend='device')")
        if self.device.type == "cpu":
            voxel_backend = "host"
        if seed_poses is None:
            seed_poses = noise_seed is not None or (lanes is not None and len(lanes) > 0)
        noise_seed = 0 if noise_seed is None else int(noise_seed)
        search = self._pose_search(overlap, pose_candidates, pose_spread, noise_seed, seed_poses)
        info_train = self._train_info()
        batches = []
        for idxs in index_batches(start_scene_index, stop_scene_index, self.batch_size):
            # resume: skip a batch whose last scene already has its generated cloud (sd:2371-2381)
            done = self.samples_folder / "scene-{:0>6d}/sample-{:0>6d}.cloud.ply".format(idxs[-1], num_samples // 2)
            if done.is_file():
                print("Skip completed scene {:0>6d} - {:0>6d}.".format(idxs[0], idxs[-1]))
                continue
            batches.append(idxs)
        pairs = [(self.model, depth_correction)] + list(lanes or [])
        if self.device.type == "cpu":
            pairs = pairs[:1]                 # lanes are HIP streams
        if self.synthetic_seed is None and not seed_poses:
            pairs = pairs[:1]                 # one global pose stream cannot be shared by concurrent lanes
        pairs = pairs[:max(1, len(batches))]
        kw = dict(num_samples=num_samples, memory_voxel_size=memory_voxel_size, save_voxel_size=save_voxel_size,
                  has_refine_step=has_refine_step, mask_threshold=mask_threshold, noise_seed=noise_seed, progress=progress,
                  seed_poses=seed_poses, info_train=info_train, per_view=clouds == "per_view", gt_log=gt_log, search=search,
                  on_device=(voxel_backend == "device" and num_samples > 1) or gt_log)      # where the scene memory lives
        n = len(pairs)
        wt = writer_threads if writer_threads <= 0 or n == 1 else max(1, writer_threads // n)
        results = [None] * n
        if n == 1:
            results[0] = self._lane(batches, pairs[0][0], pairs[0][1], wt, 1, **kw)
        else:
            errs = []
            stop = threading.Event()          # set by the first failing lane: the others stop at their next batch
            dev = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())

            def work(k):
                try:
                    torch.cuda.set_device(dev)
                    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                        results[k] = self._lane(batches[k::n], pairs[k][0], pairs[k][1], wt, n, stop=stop, **kw)
                        torch.cuda.current_stream().synchronize()
                except BaseException as e:      # noqa: BLE001 — re-raised on the calling thread
                    errs.append((k, e))
                    stop.set()

            threads = [threading.Thread(target=work, args=(k,)) for k in range(n)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            if errs:
                for k, e in errs[1:]:         # nothing is dropped: later lanes' errors are reported, the first is raised
                    print("lane {} also failed: {!r}".format(k, e), file=sys.stderr)
                raise errs[0][1]
            if stop.is_set():
                raise RuntimeError("a lane stopped early without an error")
        if stats is not None:
            stats.update(pairs=sum(r[0] for r in results), writer_jobs=sum(r[1] for r in results),
                         writer_threads=sum(r[2] for r in results), lanes=n)
        if search is not None:
            predicted = sorted(p for r in results for p in r[3])
            in_band = sum(1 for p in predicted if p[3])
            if stats is not None:
                stats["pose_search"] = dict(views=len(predicted), in_band=in_band, predicted=[p[:3] for p in predicted])
            if predicted:
                r = np.array([p[2] for p in predicted])
                print("pose search: {} views, {} predicted inside [{:g}, {:g}] ({} candidates, spread {:g}); predicted overlap "
                      "min / median / max {:.3f} / {:.3f} / {:.3f}".format(len(predicted), in_band, *search.band, search.n,
                                                                           search.spread, r.min(), float(np.median(r)), r.max()))

    _pose_lock = threading.Lock()      # guards numpy's process-wide legacy stream (seed_poses=False)

    def _batch_setup(self, idxs, info_train, sdirs=None, each=None):
        """A batch's inputs -> (K (B,3,3), K_dev, depth0 (B,1,S,S), param_cond, the scene "memory" clouds (sd:2484-2490): the
        source frames of the whole batch in ONE unprojection (sd:2479-2483 does it per scene), cropped to the box one by one;
        `each(j, K_j, depth0_j, cloud_j)` is called as soon as scene j is cropped)."""
        K = np.zeros((len(idxs), 3, 3), dtype=np.float32)
        depth0 = np.zeros((len(idxs), 1, self.image_size, self.image_size), dtype=np.float32)
        for j, idx in enumerate(idxs):
            depth0[j, 0], K[j] = self._scene_inputs(idx, info_train, None if sdirs is None else sdirs[j])
        K_dev = torch.from_numpy(K).to(self.device)
        frames = self.G.point_clouds(torch.from_numpy(depth0).to(self.device), K_dev, None)
        clouds = []
        for j, f in enumerate(frames):
            clouds.append(PP.crop_aabb(f.astype(np.float32)).astype(np.float32))
            if each is not None:                           # scene j's first files go to the writers while the next one is cropped
                each(j, K[j], depth0[j, 0], clouds[j])
        return K, K_dev, depth0, self.G.param_vector(K_dev), clouds

    def _view(self, memory, pose, K, K_dev, param_cond, model, depth_correction, seeds, mask_threshold, has_refine_step):
        """One view of every scene of a batch, launches only: the memory z-buffered into the cameras `pose`, corrected, the DDNM
        condition, the sampler, corrected again, unprojected into the common frame in float64 (sd:2623-2628)."""
        pose_dev = torch.from_numpy(pose).to(self.device)
        rpj, hit = memory.project(pose, K, self.image_size, 0.1)
        prob = depth_correction(rpj)
        rpj_c, _hit_c, cond = self.G.apply_mask(prob, rpj, hit, mask_threshold)
        images = model.sample(param_cond=param_cond, img_cond=cond, seeds=seeds, has_refine_step=has_refine_step)
        prob2 = depth_correction(images)
        images, _, _ = self.G.apply_mask(prob2, images, None, mask_threshold, want_cond=False)
        xyz, valid = self.G.unproject_f64(images, K_dev, pose_dev)
        return rpj, rpj_c, images, xyz, valid

    def _lane(self, batches, model, depth_correction, writer_threads, n_lanes, *, num_samples, memory_voxel_size,
              save_voxel_size, has_refine_step, mask_threshold, noise_seed, progress, seed_poses, info_train, stop=None,
              on_device=False, per_view=False, gt_log=False, search=None):
        """One lane's share of the batches (all of them with a single lane), on the calling thread's current stream.  Per
        batch: set-up; per view: step, memory update, blocking copies, side files, clouds; then the resume marker."""
        if writer_threads <= 0 and n_lanes > 1:
            writer_threads = max(2, min(16, PP.rank_cpu_budget() // 2) // n_lanes)
        with PP.WriterPool(writer_threads) as pool:
            marker_prev, n_pairs = None, 0    # marker_prev: deferred submission of the previous batch's resume marker
            predicted = []                    # (scene, view, predicted overlap, in band) of every searched pose
            out = _Clouds(self, pool, num_samples, save_voxel_size, per_view, gt_log)

            def flush_marker():
                nonlocal marker_prev
                if marker_prev is not None:
                    pool.wait()               # the previous batch had a whole GPU batch time to finish: no stall in practice
                    marker_prev()
                    marker_prev = None

            for idxs in batches:
                if stop is not None and stop.is_set():
                    break                      # another lane failed: do not sample this lane's whole share first
                sdirs = [self.samples_folder / "scene-{:0>6d}".format(idx) for idx in idxs]
                for sdir in sdirs:
                    shutil.rmtree(str(sdir), ignore_errors=True)        # (a scene folder of an interrupted run, if there is one)
                    sdir.mkdir(parents=True, exist_ok=True)
                out.begin(idxs, sdirs)

                def first_files(j, K_j, depth0_j, scene_pc):
                    pool.text(str(sdirs[j] / "camera-intrinsics.txt"), K_j)
                    pool.image01(str(sdirs[j] / "sample-{:0>6d}.image.png".format(0)), depth0_j)
                    out.source(j, scene_pc)

                K, K_dev, _depth0, param_cond, scene_pcs = self._batch_setup(idxs, info_train, sdirs, first_files)
                memory = DeviceMemory.upload(self.G, scene_pcs, self.device) if on_device else HostMemory(self.G, scene_pcs, self.device)
                names = ["scene-{:0>6d}".format(i) for i in idxs]
                source = None if search is None else self._search_source(memory, scene_pcs)
                for sample_idx in range(num_samples):
                    pose, found = self._view_poses(idxs, sample_idx, noise_seed if seed_poses else None, K, source, search)
                    if found is not None:
                        predicted += [(i, sample_idx + 1, r, ok) for i, (r, ok) in zip(idxs, found)]
                    seeds = [synthetic.noise_seed(noise_seed, i, sample_idx) for i in idxs]
                    rpj, rpj_c, images, xyz, valid = self._view(memory, pose, K, K_dev, param_cond, model, depth_correction, seeds,
                                                                mask_threshold, has_refine_step)
                    if sample_idx < num_samples - 1:                                # memory update (sd:2661-2680): queued
                        memory.update(xyz, valid, memory_voxel_size)
                    out.add_view(memory, pose, xyz, valid)                          # (gt_log: the finish is queued with the last)
                    # one blocking copy per tensor: the host waits here for the GPU while the pool writes the previous batch
                    rpj_host, crt_host, img_host = rpj.cpu().numpy(), rpj_c.cpu().numpy(), images.cpu().numpy()
                    rows = None if gt_log else HostRows.copy(xyz, valid)            # (gt_log: the views stay on the device)
                    memory.settle(names, rows)
                    flush_marker()
                    for j, sdir in enumerate(sdirs):
                        pool.image01(str(sdir / "reprojected.image.png"), rpj_host[j])
                        pool.text(str(sdir / "sample-{:0>6d}.pose.txt".format(sample_idx + 1)), np.linalg.inv(pose[j]))
                        pool.image01(str(sdir / "corrected.image.png"), crt_host[j])
                        pool.image01(str(sdir / "sample-{:0>6d}.image.png".format(sample_idx + 1)), img_host[j])
                        pool.depth16(str(sdir / "sample-{:0>6d}.depth.png".format(sample_idx + 1)), img_host[j])
                        memory.settle_scene(j)                                      # (host memory: this scene's grid, on this thread)
                        out.write(j, rows)
                    if progress:
                        print("batch {:0>6d}-{:0>6d}: sample {}/{}".format(idxs[0], idxs[-1], sample_idx + 1, num_samples))
                n_pairs += len(idxs)
                flush_marker()                # (only reached with a pending marker when the sample loop did not run)
                marker_prev = out.marker
            flush_marker()
            return n_pairs, pool.wait(), pool.threads, predicted

    # -- gt_log: every cloud of a scene finished on the device, the scene's gt.log written with them ---------------------------
    GT_VOXEL, GT_FACTOR, GT_MIN_POINTS = 0.025, 1.5, 1000      # generate_gt's fixed literals (generate_gt.py:68-102, 133-140)
    GT_LINE = "{}\t{}\t{}\t{:.4f}\t{:.4f}\n"                   # a gt.log line: scene name, s, t, overlap of s, overlap of t

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _pair_table(B, n_seg, dev):
        """`_pair_rows` as the (pairs, 2) int32 device table that prg_overlap_counts_indexed takes.  Uploaded once."""
        return torch.from_numpy(np.array(Generator._pair_rows(B, n_seg), dtype=np.int32)).to(dev)

    @staticmethod
    def _pair_rows(B, n_seg):
        """Every pair (s, t), s < t, of every scene's n_seg segments, scene-major and in `combinations` order, as rows
        (n_seg * j + s, n_seg * j + t) of the batch's segment list."""
        return [(n_seg * j + s, n_seg * j + t) for j in range(B) for s, t in combinations(range(n_seg), 2)]

    def _finish_pairs_launch(self, memory, views, poses, per_view, save_voxel_size) -> FinishedPairs:
        """Device work of a batch's pairs, nothing read back.  Segment n*j is scene j's source frame (`memory.mem_pts0`, float32
        widened to float64).  `poses`: one array (B,4,4) per view.  Fused: n = 2, segment 2j+1 is all the views in view order, moved
        by the FIRST view's pose and back.  `per_view`: n = 1 + views, segment n*j+i is view i alone, moved by ITS pose and back.
        Either way the segments are offset arithmetic on `merge_memory`'s buffer [memory_j | view 1 rows | ... | view k rows]; the
        source frames are not moved, and the crop box, applied to every segment, is a no-op on them.  Every cloud
        is gridded once at generate_gt's 0.025 and all B * C(n, 2) pairs go through ONE prg_overlap_counts_indexed launch."""
        G_, mem_pts0, mem_offs0, mem_rows = self.G, memory.mem_pts0, memory.mem_offs0, memory.rows0
        B, dev = len(mem_rows), mem_pts0.device
        xyz = views[0][0] if len(views) == 1 else torch.cat([v[0] for v in views], dim=1)         # (B, n_views*HW, 3)
        valid = views[0][1] if len(views) == 1 else torch.cat([v[1] for v in views], dim=1)
        rows_v = xyz.shape[1]
        rows_seg = views[0][0].shape[1] if per_view else rows_v                                   # rows of a view segment
        n = 1 + (len(views) if per_view else 1)
        merged, mvalid, moffs = G_.merge_memory(mem_pts0, mem_offs0, xyz, valid)
        first = mem_offs0[1:] + torch.arange(B, dtype=torch.int64, device=dev) * rows_v           # scene j's first view row
        offs = torch.empty((n * B + 1,), dtype=torch.int64, device=dev)
        offs[0:n * B:n] = moffs[:-1]
        for i in range(1, n):
            offs[i:n * B:n] = first + (i - 1) * rows_seg
        offs[n * B] = moffs[-1]
        pre = np.zeros((n * B, 4, 4), dtype=np.float64)
        post = np.zeros((n * B, 4, 4), dtype=np.float64)
        has = np.zeros((n * B,), dtype=np.uint8)
        for j in range(B):
            for i in range(1, n):
                T = poses[i - 1][j].astype(np.float64)
                pre[n * j + i], post[n * j + i], has[n * j + i] = T, np.linalg.inv(T), 1     # the same 16 doubles as the host path
        fin, fin_offs, st_save = G_.finish_clouds(merged, mvalid, offs, save_voxel_size, pre=pre, has_pre=has,
                                                  crop=(PP.BBOX_MIN, PP.BBOX_MAX), post=post, has_post=has)
        down, down_offs, st_gt = G_.voxel_grid_ragged(fin, None, fin_offs, self.GT_VOXEL)
        # max_cloud only bounds the query slabs: no finished cloud has more rows than went into it
        counts = G_.overlap_counts_indexed(down, down_offs, self._pair_table(B, n, dev), int(max(max(mem_rows), rows_seg)),
                                           float(self.GT_VOXEL * self.GT_FACTOR))
        return FinishedPairs(fin, fin_offs, st_save, st_gt, counts, down_offs)

    def _finish_pairs_write(self, pool, finished, idxs, sdirs, submit):
        """Host side: ONE copy of the finished clouds, the PLY files as write-only jobs handed to `submit(job, j, k)`, every
        scene's gt.log written before this returns — one line per surviving pair (s, t), s < t, in `combinations` order."""
        offs, d_offs, cnt = self._finish_pairs_words(finished, idxs)
        n = (len(offs) - 1) // len(idxs)
        pts = finished.points[:max(int(offs[-1]), 0)].cpu().numpy()
        for j, sdir in enumerate(sdirs):
            for k in range(n):
                submit((lambda path=str(sdir / "sample-{:0>6d}.cloud.ply".format(k)), pc=pts[offs[n * j + k]:offs[n * j + k + 1]]:
                        pool.cloud(path, pc, None, crop=False, voxel=0)), j, k)
        lines = [[] for _ in idxs]
        for j, s, t, ratios, _why in self._pair_walk(offs, d_offs, cnt, len(idxs)):
            if ratios is not None:
                lines[j].append(self.GT_LINE.format("scene-{:0>6d}".format(idxs[j]), s, t, *ratios))
        for sdir, ln in zip(sdirs, lines):
            (sdir / "gt.log").write_text("".join(ln))

    def _finish_pairs_words(self, finished, idxs):
        """The small words of a finished batch in ONE copy, voxel statuses checked: -> (offsets (nB+1), down-sampled offsets
        (nB+1), overlap counts (B * C(n, 2), 2)) on the host, n clouds per scene."""
        N = finished.offsets.numel() - 1                                      # n * B segments
        small = torch.cat([finished.offsets, finished.down_offsets, finished.status_save.to(torch.int64),
                           finished.status_gt.to(torch.int64), finished.counts.view(-1).to(torch.int64)]).cpu().numpy()
        names = ["scene-{:0>6d} sample-{:0>6d}".format(i, k) for i in idxs for k in range(N // len(idxs))]
        self.G.check_voxel_status(small[2 * N + 2:3 * N + 2], names)
        self.G.check_voxel_status(small[3 * N + 2:4 * N + 2], names)
        return small[:N + 1], small[N + 1:2 * N + 2], small[4 * N + 2:].reshape(-1, 2)

    @classmethod
    def _pair_walk(cls, offs, d_offs, cnt, B):
        """Every pair of a finished batch (the words of `_finish_pairs_words`) in `_pair_rows` order: yields (j, s, t, ratios or
        None, reason) — scene j of the batch, its clouds s < t, `_pair_ratios_at`'s answer (two clouds per scene: `_pair_ratios`')."""
        n = (len(offs) - 1) // B
        for p, (a, b) in enumerate(cls._pair_rows(B, n)):
            j = a // n
            ratios, why = cls._pair_ratios(offs, d_offs, cnt, j) if n == 2 else cls._pair_ratios_at(offs, d_offs, cnt[p], a, b)
            yield j, a - n * j, b - n * j, ratios, why

    @classmethod
    def _pair_ratios(cls, offs, d_offs, cnt, j):
        """generate_gt's filter on pair j of a finished batch of two clouds per scene: -> ((overlap of the source, of the target),
        None) when the pair gets a gt.log line, (None, reason) when it does not."""
        return cls._pair_ratios_at(offs, d_offs, cnt[j], 2 * j, 2 * j + 1)

    @classmethod
    def _pair_ratios_at(cls, offs, d_offs, cnt, a, b):
        """The general form: the pair of segments (a, b) of a finished batch, `cnt` that pair's two overlap counts."""
        with np.errstate(invalid="ignore", divide="ignore"):
            o_s = float(np.float64(cnt[0]) / np.float64(d_offs[a + 1] - d_offs[a]))
            o_t = float(np.float64(cnt[1]) / np.float64(d_offs[b + 1] - d_offs[b]))
        why = cls._pair_dropped(offs[a + 1] - offs[a], offs[b + 1] - offs[b], o_s, o_t)
        return ((o_s, o_t), None) if why is None else (None, why)

    @classmethod
    def _pair_too_small(cls, rows_a, rows_b):
        """The size part of the rule: such a pair is dropped whatever its ratios, so none need be computed for it."""
        return rows_a < cls.GT_MIN_POINTS or rows_b < cls.GT_MIN_POINTS

    @classmethod
    def _pair_dropped(cls, rows_a, rows_b, o_s, o_t):
        """THE gt.log rule (generate_gt.py:133-140, 160-165) on a pair of saved clouds with `rows_a` / `rows_b` rows and overlap
        ratios (o_s, o_t): None when the pair gets a line, the reason when it does not."""
        if cls._pair_too_small(rows_a, rows_b):
            return "a cloud has fewer than {} points".format(cls.GT_MIN_POINTS)
        if np.isnan(o_s) or np.isnan(o_t):
            return "an overlap ratio is NaN"
        if o_s < 0.1 and o_t < 0.1:
            return "both overlap ratios are below 0.1"
        return None


class _Clouds:
    """Where a lane's clouds go, one of three ways chosen once per `generate` call.  `gt_log`: the views stay on the device and the
    last one queues the finish of every cloud; otherwise the writer pool finishes them (crop, voxel grid, PLY) from host copies
    of the views (`rows`), all the views of a scene in ONE cloud in the first view's frame, or `per_view` each alone in its own.
    Per batch `begin`, then `source(j, cloud)` per scene; per view `add_view` before the blocking copies and `write(j, rows)` right
    after scene j's side files, so that the writers get work scene by scene; then `marker` is the batch's resume marker (the
    cloud file the resume check looks for), a job not yet submitted."""

    def __init__(self, gen, pool, num_samples, save_voxel_size, per_view, gt_log):
        self.gen, self.pool, self.num_samples, self.voxel, self.per_view, self.gt_log = gen, pool, num_samples, save_voxel_size, per_view, gt_log
        self.source = self._no_source if gt_log else self._source              # (gt_log: cloud 0 comes from the device as well)
        # (one view per scene: the fused cloud IS the view's, and the worker compacts it)
        self.write = self._write_finished if gt_log else self._write_per_view if per_view or num_samples == 1 else self._write_fused

    def begin(self, idxs, sdirs):
        self.idxs, self.sdirs, self.marker, self.views, self.poses, self.frags = idxs, sdirs, None, [], [], [None] * len(idxs)

    def submit(self, job, j, k):
        """THE marker rule: cloud k of the batch's last scene is held back until everything else of the batch is on disk."""
        if j == len(self.sdirs) - 1 and k == self.num_samples // 2:
            self.marker = job
        else:
            job()

    def cloud(self, j, k, pc, valid, T):
        """Cloud k of scene j: `pc[valid]` moved by T, cropped, gridded, moved back (sd:2640-2658); T None: gridded as it is."""
        path = str(self.sdirs[j] / "sample-{:0>6d}.cloud.ply".format(k))
        self.submit(lambda: self.pool.cloud(path, pc, valid, pre=T, crop=T is not None, voxel=self.voxel,
                                            post=None if T is None else np.linalg.inv(T)), j, k)

    def _source(self, j, pc):
        self.cloud(j, 0, pc, None, None)

    def _no_source(self, j, pc):
        pass

    def add_view(self, memory, pose, xyz, valid):
        self.poses.append(pose)
        if self.gt_log:
            self.views.append((xyz, valid))
            if len(self.poses) == self.num_samples:
                self.finished = self.gen._finish_pairs_launch(memory, self.views, self.poses, self.per_view, self.voxel)

    def _write_finished(self, j, rows):                    # once, after the side files of the last view's last scene
        if j == len(self.sdirs) - 1 and len(self.poses) == self.num_samples:
            self.gen._finish_pairs_write(self.pool, self.finished, self.idxs, self.sdirs, self.submit)

    def _write_per_view(self, j, rows):
        self.cloud(j, len(self.poses), rows.xyz[j], rows.valid[j], self.poses[-1][j].astype(np.float64))

    def _write_fused(self, j, rows):
        first = len(self.poses) == 1
        self.frags[j] = rows.compact(j) if first else np.concatenate([self.frags[j], rows.compact(j)], axis=0)
        if len(self.poses) == self.num_samples:
            self.cloud(j, 1, self.frags[j], None, self.poses[0][j].astype(np.float64))


def generate_gt(dataset_name: str, start_scene_index: int, stop_scene_index: int, num_samples: int,
                root: str = ".", overlap: str = "hip", scenes_per_launch: int = 512, voxel: str = "device") -> None:
    """generate_gt.py:105-175 — per scene, every pair of .cloud.ply -> overlap ratios -> scene gt.log.

    The reference queries a KD-tree once per point in a Python loop (the wall-clock tail of a 10k-scene dataset); here the
    clouds of up to `scenes_per_launch` scenes are voxel-down-sampled by ONE ragged device call (`voxel='device'`; 'host' =
    one by one in C++ on the calling thread, same ratios), every cloud once however many of its scene's pairs it is in, and all
    their pairs go through ONE prg_overlap_counts_indexed launch.  `overlap='numpy-spec'` selects the numpy specification in postprocess.py instead — a test
    hook for boxes without a GPU, never chosen implicitly."""
    if overlap not in ("hip", "numpy-spec"):
        raise ValueError("overlap must be 'hip' or 'numpy-spec'")
    data = Path(root) / dataset_name / "data"
    todo = []                                   # (scene_name, gt_path, [(s, t, src, tgt), ...])
    for scene_idx in range(start_scene_index, stop_scene_index):
        scene_name = "scene-{:0>6d}".format(scene_idx)
        sdir = data / scene_name
        gt_path = sdir / "gt.log"
        if gt_path.exists():
            print("scene gt log has existed, skip over it")
            continue
        cand = []
        for s, t in combinations(range(num_samples), 2):
            ps, pt = sdir / "sample-{:0>6d}.cloud.ply".format(s), sdir / "sample-{:0>6d}.cloud.ply".format(t)
            if not ps.exists() or not pt.exists():
                continue
            src, tgt = PP.read_ply(str(ps)), PP.read_ply(str(pt))
            if not Generator._pair_too_small(len(src), len(tgt)):
                cand.append((s, t, src, tgt))
        todo.append((scene_name, gt_path, cand))
        if len(todo) >= scenes_per_launch:
            _finish_gt(todo, overlap, voxel)
            todo = []
    if todo:
        _finish_gt(todo, overlap, voxel)


def _finish_gt(todo, overlap: str, voxel: str = "device") -> None:
    if overlap == "hip":             # every cloud uploaded and gridded once, however many of its scene's pairs it is in
        clouds, pairs = [], []
        for _n, _p, cand in todo:
            at = {}                  # sample index -> position in `clouds`, within this scene
            for (s, t, src, tgt) in cand:
                for k, c in ((s, src), (t, tgt)):
                    if k not in at:
                        at[k] = len(clouds)
                        clouds.append(c)
                pairs.append((at[s], at[t]))
        ratios = PP.overlap_ratios_indexed_hip(clouds, pairs, voxel=voxel)
    else:
        ratios = [PP.compute_overlap_ratio(src, tgt) for _n, _p, cand in todo for (_s, _t, src, tgt) in cand]
    ratios = iter(ratios)            # in the order of the candidates
    for scene_name, gt_path, cand in todo:
        rated = [(s, t, len(src), len(tgt), *next(ratios)) for (s, t, src, tgt) in cand]
        lines = [Generator.GT_LINE.format(scene_name, s, t, o_s, o_t) for s, t, ra, rb, o_s, o_t in rated
                 if Generator._pair_dropped(ra, rb, o_s, o_t) is None]
        gt_path.parent.mkdir(exist_ok=True)
        gt_path.write_text("".join(lines))


def gather_gt(dataset_name: str, start_index: int, stop_index: int, root: str = ".") -> None:
    """generate_gt.py:177-188 — concatenate the scene logs in index order into metadata/gt.log (replacing it)."""
    final = Path(root) / dataset_name / "metadata" / "gt.log"
    final.parent.mkdir(parents=True, exist_ok=True)
    if final.exists():
        os.remove(str(final))
    with open(final, "ab") as out:
        for scene_idx in range(start_index, stop_index):
            p = Path(root) / dataset_name / "data" / "scene-{:0>6d}".format(scene_idx) / "gt.log"
            if p.exists():
                out.write(p.read_bytes())
