"""prg_patch_corr_labels_f64 and its Python layers on an MI355X.  Run with `-m gpu`.

Everything is BIT-EXACT against `postprocess.patch_corr_labels`, which tests/test_fine_labels_spec.py checks against an independent
formulation on the CPU.  The kernel gives a wave to a selected pair, four pairs to a workgroup, and 64-slot chunks along the target
slots to a patch; a label row is limit + 1 bytes.  So the limits below sit on both sides of every chunk boundary and give odd and
even row strides, and the pair counts give one partial workgroup, one full one, one more than full, and many."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xAB, 67           # the labels start at an odd address: nothing may lean on their alignment
R = 0.5                          # exactly representable, and so is R * R
LIMITS = [1, 4, 63, 64, 65, 128, 256]
COUNTS = [1, 3, 4, 5, 257]


@pytest.fixture(scope="module")
def L():
    from pointreggpt_amd import _lib
    _lib.load()
    return _lib


def D(a):
    return torch.from_numpy(np.array(a)).cuda()                                  # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def problem(limit):
    """(points, table, pairs, labels of the specification) for 257 pairs — computed once per limit, shared, never written.
    Points: a cloud in a 1.2-wide cube (radius 0.5: a good share of every kind of label), one NaN row, and three rows far below
    it at distance exactly R and one ulp less along x.  Table rows: 0 full, 1 a prefix, 2 empty, 3 pads mid-row (n, -1 and a huge
    entry), 4 holds the NaN row, 5 and 6 the exact-radius rows, 7.. random."""
    rng = np.random.default_rng(1000 + limit)
    n_cloud = max(40, 2 * limit)
    pts = np.concatenate([rng.uniform(0, 1.2, (n_cloud, 3)), [[np.nan, 0.3, 0.3]],
                          [[0, 0, -5], [R, 0, -5], [np.nextafter(R, 0), 0, -5]]])
    n, i_nan, i_o, i_r, i_in = len(pts), n_cloud, n_cloud + 1, n_cloud + 2, n_cloud + 3
    M = 12
    table = np.full((M, limit), n, dtype=np.int32)
    pick = lambda k: rng.choice(n_cloud, k, replace=n_cloud < k).astype(np.int32)                  # noqa: E731
    table[0] = pick(limit)
    table[1, :(limit + 1) // 2] = pick((limit + 1) // 2)
    table[3] = pick(limit)
    table[3, rng.random(limit) < 0.5] = n
    table[3, rng.random(limit) < 0.2] = -1
    table[3, rng.random(limit) < 0.1] = np.iinfo(np.int32).max
    table[4] = pick(limit)
    table[4, limit // 2] = i_nan
    table[5, limit - 1] = i_o
    table[6, 0] = i_r
    if limit > 1:
        table[6, limit // 2 if limit > 2 else 1] = i_in
    for k in range(7, M):
        table[k] = pick(limit)
        table[k, rng.random(limit) < rng.uniform(0, 0.6)] = n
    fixed = [[0, 3], [5, 6], [6, 5], [M, 0], [4, 4], [2, 0], [0, 2], [-1, 1], [1, np.iinfo(np.int32).min], [2, 2], [3, 1],
             [np.iinfo(np.int32).max, np.iinfo(np.int32).max], [4, 0], [7, 7]]
    pairs = np.concatenate([np.array(fixed, dtype=np.int64), rng.integers(-1, M + 1, (257 - len(fixed), 2))]).astype(np.int32)
    want = PP.patch_corr_labels(pts, table, pairs, R)
    for a in (pts, table, pairs, want):
        a.setflags(write=False)
    # the cases are really there
    K = limit
    assert not want[1, K - 1, 0] and want[1, K, 0]                               # exactly R apart: no match, the target is slack
    assert want[1, K - 1, K] == (limit == 1)                                     # ... and the source too, when it has no other
    if limit > 1:
        assert want[1, K - 1, limit // 2 if limit > 2 else 1] and want[1, K - 1].sum() == 1      # one ulp inside: a match
        assert want[4, limit // 2, K] and want[4, K, limit // 2] and not want[4, limit // 2, :K].any()       # the NaN row
        assert want[:, :K, :K].any() and not want[:, :K, :K].all()
    assert not want[[3, 7, 8, 9, 11]].any()
    return pts, table, pairs, want


def run(L, pts, table, pairs, limit, radius=R):
    """The entry point through ctypes on a 0xAB-filled buffer with guard bytes on both sides, twice: the guards must survive, every
    label byte must be 0 or 1, both runs must agree, the inputs must come back as they went in."""
    lib = L.load()
    n, m, S = len(pts), len(table), len(pairs)
    d_pts = D(pts) if n else None
    d_table, d_pairs = D(table), D(pairs)
    size = S * (limit + 1) ** 2
    outs = []
    for _ in range(2):
        buf = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        rc = lib.prg_patch_corr_labels_f64(L.ptr(d_pts), n, L.ptr(d_table), m, limit, L.ptr(d_pairs), S, radius,
                                           C.c_void_p(buf.data_ptr() + GUARD), L.stream_ptr())
        assert rc == 0, lib.prg_last_error()
        torch.cuda.synchronize()
        outs.append(buf.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    out = outs[0]
    assert (out[:GUARD] == FILL).all() and (out[GUARD + size:] == FILL).all()
    body = out[GUARD:GUARD + size]
    assert (body <= 1).all()                                                     # every byte overwritten, with 0 or 1
    if n:
        assert d_pts.cpu().numpy().tobytes() == np.ascontiguousarray(pts).tobytes()
    assert np.array_equal(d_table.cpu().numpy(), table) and np.array_equal(d_pairs.cpu().numpy(), pairs)
    return body.reshape(S, limit + 1, limit + 1)


@pytest.mark.parametrize("limit", LIMITS)
def test_kernel_equals_the_specification(L, limit):
    pts, table, pairs, want = problem(limit)
    for S in COUNTS:
        got = run(L, pts, table, pairs[:S], limit)
        assert np.array_equal(got.astype(bool), want[:S]), (limit, S)


def test_no_points_at_all(L):
    table = np.zeros((3, 5), dtype=np.int32)                                     # every entry is outside [0, 0): a pad
    table[1] = [-1, 7, 0, 3, 2 ** 31 - 1]
    pairs = np.array([[0, 1], [1, 2], [3, 0], [2, 2], [1, 1]], dtype=np.int32)
    got = run(L, np.zeros((0, 3)), table, pairs, 5, radius=0.05)
    assert not got.any()
    assert not PP.patch_corr_labels(np.zeros((0, 3)), table, pairs, 0.05).any()


@pytest.mark.parametrize("limit", [4, 65])
def test_python_layers_equal_the_specification(limit):
    from pointreggpt_amd import geometry as G
    pts, table, pairs, want = problem(limit)
    got = G.patch_corr_labels(D(pts), D(table), D(pairs), R)
    assert got.is_cuda and got.dtype == torch.bool and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    host = PP.patch_corr_labels_hip(pts, table, pairs, R)
    assert host.dtype == np.bool_ and np.array_equal(host, want)
    # float32 points are converted, not refused
    p32 = np.where(np.isnan(pts), np.nan, pts).astype(np.float32)
    got32 = G.patch_corr_labels(D(p32), D(table), D(pairs[:9]), R)
    assert np.array_equal(got32.cpu().numpy(), PP.patch_corr_labels(p32.astype(np.float64), table, pairs[:9], R))
    # no pair: the empty tensor; no node: every pair stands for two empty patches
    none = G.patch_corr_labels(D(pts), D(table), D(np.zeros((0, 2), dtype=np.int32)), R)
    assert tuple(none.shape) == (0, limit + 1, limit + 1) and none.dtype == torch.bool and none.is_cuda
    no_nodes = G.patch_corr_labels(D(pts), torch.zeros((0, limit), dtype=torch.int32, device="cuda"), D(pairs[:3]), R)
    assert tuple(no_nodes.shape) == (3, limit + 1, limit + 1) and not no_nodes.any().item()
