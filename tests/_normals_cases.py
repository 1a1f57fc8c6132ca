"""Inputs shared by tests/test_normals_spec.py (CPU) and tests/test_gpu_normals.py: ragged stacks of clouds with their neighbour
tables, as prg_normals_ragged_f64 takes them, and a plain-Python restatement of `postprocess.estimate_normals` for one row that
can make the mistakes the tests must detect.

The kernel gives 8 lanes to a row and 32 rows to a workgroup: the cloud sizes sit on both sides of 32 and 64 rows, the limits on
both sides of 8, and the 1024 case has a cluster of 1100 rows inside one radius so that rows really fill 1024 slots.  Every
cloud of 31 rows or more also carries an isolated row (count 1), an isolated triple (count 3) and, at the small limits, rows with
count > limit."""
import math

import numpy as np

from pointreggpt_amd import postprocess as PP

POISON = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]
VIEWS = np.array([[0.5, 0.5, 5.0], [0.5, 0.5, -5.0], [5.0, 0.5, 1.0], [0.25, -4.0, 1.5], [-3.0, 0.5, 0.75]])
EXTRAS = np.array([[10.0, 10.0, 10.0], [20.0, 20.0, 20.0], [20.05, 20.0, 20.01], [20.0, 20.04, 20.02]])

# (limit, radius, cloud sizes, head rows, tail rows)
CASES = [(3, 0.3, [31, 0, 32, 1, 33], 2, 3),
         (7, 0.3, [63, 64, 65], 0, 1),
         (8, 0.3, [64, 5, 97], 1, 0),
         (9, 0.3, [65, 128], 0, 0),
         (64, 0.3, [300, 129], 3, 2),
         (1024, 0.3, [1140], 0, 2)]


def patch(rng, n, kind=0):
    """n rows of a noisy surface patch over the unit square at z ~ 1: a tilted plane (kind 0) or a paraboloid (kind 1)."""
    xy = rng.uniform(0.0, 1.0, (n, 2))
    z = 1.0 + (0.3 * xy[:, 0] - 0.2 * xy[:, 1] if kind == 0 else 0.8 * ((xy[:, 0] - 0.5) ** 2 + (xy[:, 1] - 0.5) ** 2))
    return np.column_stack([xy, z + rng.normal(0.0, 0.004, n)])


def case_clouds(index):
    limit, radius, sizes, head, tail = CASES[index]
    rng = np.random.default_rng(100 + index)
    clouds = []
    for c, n in enumerate(sizes):
        if limit == 1024:                                # 1100 rows within one radius, 40 rows of a sparse patch
            pts = np.concatenate([np.array([0.5, 0.5, 1.0]) + rng.uniform(-0.08, 0.08, (n - 40, 3)), patch(rng, 40)], 0)
        else:
            pts = patch(rng, n, c % 2)
        if n >= 31:
            pts[-4:] = EXTRAS + 0.001 * c
        clouds.append(pts)
    return limit, radius, clouds, head, tail


_built = {}


def build(index):
    """-> dict(limit, pts (total,3) with poisoned head / tail rows, offsets (C+1), table (Q, limit) int32 with stack indices,
    table_offsets (C+1), count (Q,), views (C,3), clouds, tables: per cloud the LOCAL (table, count) of radius_neighbors).
    Built once per case and shared: treat it as read-only."""
    if index in _built:
        return _built[index]
    limit, radius, clouds, head, tail = case_clouds(index)
    C = len(clouds)
    offsets = head + np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.concatenate([np.full((head, 3), POISON)] + clouds + [np.full((tail, 3), POISON)], 0)
    tables = [PP.radius_neighbors(c, c, radius, limit) for c in clouds]
    total = len(pts)
    table = np.concatenate([np.where(t < len(c), t + np.int32(offsets[i]), np.int32(total)).astype(np.int32)
                            for i, (c, (t, _k)) in enumerate(zip(clouds, tables))], 0)
    count = np.concatenate([k for _t, k in tables]).astype(np.int32)
    out = dict(limit=limit, radius=radius, pts=pts, offsets=offsets, table=table, table_offsets=offsets - head, count=count,
               views=VIEWS[:C].copy(), clouds=clouds, tables=tables)
    _built[index] = out
    return out


def _lane_sum(vals):
    part = [0.0] * 8
    for s, x in enumerate(vals):
        part[s % 8] = part[s % 8] + x
    return ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]))


def row_reference(points, row, count, i, view, *, sweeps=6, min_neighbors=3, mistake=None):
    """`postprocess.estimate_normals` for row i in plain Python floats (IEEE float64, math.sqrt) -> ((nx, ny, nz), variation).
    mistake: None, "mean_over_limit", "pad_included" (the pad slot is the shadow row of zeros KPConv networks append),
    "largest" (eigenvalue), or a viewpoint mistake made by the caller through `view`."""
    limit = len(row)
    k = min(int(count), limit)
    p = [float(x) for x in points[i]]
    if k < min_neighbors or not all(math.isfinite(x) for x in p):
        return (0.0, 0.0, 1.0), 0.0
    nb = [[float(x) for x in points[j]] for j in row[:k]]
    if mistake == "pad_included" and k < limit:
        nb.append([0.0, 0.0, 0.0])
        k += 1
    div = float(limit if mistake == "mean_over_limit" else k)
    m = [_lane_sum([q[a] for q in nb]) / div for a in range(3)]
    d = [[q[a] - m[a] for a in range(3)] for q in nb]
    A = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            A[a][b] = A[b][a] = _lane_sum([q[a] * q[b] for q in d])
    V = [[1.0 if a == b else 0.0 for b in range(3)] for a in range(3)]
    for _ in range(sweeps):
        for p_, q_ in ((0, 1), (0, 2), (1, 2)):
            r_ = 3 - p_ - q_
            apq = A[p_][q_]
            if apq == 0.0:
                continue
            theta = (A[q_][q_] - A[p_][p_]) / (2.0 * apq)               # float / and * overflow to inf, they do not raise
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            h = t * apq
            A[p_][p_], A[q_][q_] = A[p_][p_] - h, A[q_][q_] + h
            apr, aqr = c * A[p_][r_] - s * A[q_][r_], s * A[p_][r_] + c * A[q_][r_]
            A[p_][r_] = A[r_][p_] = apr
            A[q_][r_] = A[r_][q_] = aqr
            A[p_][q_] = A[q_][p_] = 0.0
            for j in range(3):
                V[j][p_], V[j][q_] = c * V[j][p_] - s * V[j][q_], s * V[j][p_] + c * V[j][q_]
    lam = [A[0][0], A[1][1], A[2][2]]
    col = 0
    for a in (1, 2):
        if (lam[a] > lam[col]) if mistake == "largest" else (lam[a] < lam[col]):
            col = a
    n = [V[0][col], V[1][col], V[2][col]]
    total = (lam[0] + lam[1]) + lam[2]
    var = 0.0 if total == 0.0 else lam[col] / total
    dot = (n[0] * (float(view[0]) - p[0]) + n[1] * (float(view[1]) - p[1])) + n[2] * (float(view[2]) - p[2])
    if dot < 0.0:
        n = [-x for x in n]
    return tuple(n), var


def spec_stack(case):
    """The specification on every cloud of a built case -> (normals (Q,3), variation (Q,), scatter (Q,6))."""
    out = [], [], []
    for c, (cloud, (t, k)) in enumerate(zip(case["clouds"], case["tables"])):
        parts = {}
        n, v = PP.estimate_normals(cloud, t, k, viewpoint=case["views"][c], _parts=parts)
        for o, a in zip(out, (n, v, parts["scatter"])):
            o.append(a)
    return tuple(np.concatenate(o, 0) for o in out)
