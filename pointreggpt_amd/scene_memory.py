"""The scene "memory" of a batch between two views (sd:2484-2490, sd:2661-2680 of the reference's successive_ddnm_diffusion.py):
what the next view's z-buffer reads and every new view is merged into.  Two holders, the same bits, the same operations:
    project(pose, K, S, depth_scale) -> (rpj, hit)    the clouds moved by `pose` and z-buffered, one ragged launch
    update(xyz, valid, voxel)                         queue memory_j <- voxel grid of [memory_j | xyz[j][valid[j]]], device tensors
    settle(names, rows)                               after the caller's blocking copies; rows: the view as `HostRows`, or None
    settle_scene(j)                                   per scene, between the caller's file submissions of that scene
The device holder launches in `update`, reads its status words in `settle` (a failed grid raises naming names[j]) and has nothing
left per scene; the host holder does scene j's grid in `settle_scene(j)`, on the calling thread, while the writer pool works.
`ops` holds the device calls (`geometry`, or `cpu.ops`), looked up at every call."""
from __future__ import annotations

import numpy as np
import torch

from . import postprocess as PP


class HostRows:
    """A view on the host: xyz (B, HW, 3) float64 and valid (B, HW) as numpy; a scene's valid rows are compacted once."""

    def __init__(self, xyz, valid):
        self.xyz, self.valid, self._compact = xyz, valid, {}

    @classmethod
    def copy(cls, xyz, valid):                         # two blocking copies
        return cls(xyz.cpu().numpy(), valid.cpu().numpy())

    def compact(self, j):
        if j not in self._compact:
            self._compact[j] = self.xyz[j][np.asarray(self.valid[j], dtype=bool)]
        return self._compact[j]


class DeviceMemory:
    """One float32 ragged buffer on the GPU (`pts`, `offs` (B+1) int64), read by the next z-buffer in place.  `mem_pts0` / `mem_offs0`
    / `rows0` (row counts, known after `upload`) stay what it was built from: the source frames of the device finish of the pairs."""

    def __init__(self, ops, pts, offs, rows0=None):
        self.ops, self.pts, self.offs, self._status = ops, pts, offs, None
        self.mem_pts0, self.mem_offs0, self.rows0 = pts, offs, rows0

    @classmethod
    def upload(cls, ops, clouds, device):              # the ONE upload of a batch's host clouds
        return cls(ops, *ops.upload_clouds(clouds, device), rows0=[len(c) for c in clouds])

    def project(self, pose, K, S, depth_scale):
        return self.ops.project_cloud_buffer(self.pts, self.offs, pose, K, S, depth_scale=depth_scale)

    def update(self, xyz, valid, voxel):               # launches only, no host trip
        merged, mvalid, moffs = self.ops.merge_memory(self.pts, self.offs, xyz, valid)
        out, self.offs, self._status = self.ops.voxel_grid_ragged(merged, mvalid, moffs, voxel)
        self.pts = out.to(torch.float32)

    def settle(self, names, rows=None):
        if self._status is not None:                   # B status words + the row count: all the host learns of the update
            st_n = torch.cat([self._status.to(torch.int64), self.offs[-1:]]).cpu().numpy()
            self._status = None
            self.ops.check_voxel_status(st_n[:-1], names)
            self.pts = self.pts[:max(int(st_n[-1]), 1)]

    def settle_scene(self, j):
        pass

    def clouds(self):                                  # the ONE copy back to the host: (n_j, 3) float32 arrays
        o, p = self.offs.cpu().numpy(), self.pts.cpu().numpy()
        return [p[o[j]:o[j + 1]].copy() for j in range(len(o) - 1)]


class HostMemory:
    """A list of float32 numpy clouds, re-voxelised one by one in C++ on the calling thread (the only holder with `device="cpu"`)."""

    def __init__(self, ops, clouds, device):
        self.ops, self.device, self.list, self._queued, self._now = ops, device, list(clouds), None, None

    def project(self, pose, K, S, depth_scale):
        return self.ops.project_clouds(self.list, pose, K, S, self.device, depth_scale=depth_scale)

    def update(self, xyz, valid, voxel):
        self._queued = voxel

    def settle(self, names, rows):
        self._now, self._queued = (None if self._queued is None else (rows, self._queued)), None

    def settle_scene(self, j):
        if self._now is not None:
            rows, voxel = self._now
            merged = np.concatenate([self.list[j], rows.compact(j)], axis=0)
            self.list[j] = PP.native_voxel_down_sample(merged, voxel).astype(np.float32)

    def clouds(self):
        return self.list
