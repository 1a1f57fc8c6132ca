"""The weight packings, restated in numpy from the layout comments of csrc/conv.h (ConvLaunch) and csrc/weights_host.h and compared
bit for bit with what the library packs (prg_debug_pack_conv, host only: no GPU).  Shapes with padding in both directions:
Cout = 72 (CoutPad 128), Cin = 40 (two chunks of 32, three of 16), K = 3; and Cout = Cin = 8, K = 1.  Every restatement is also shown to
catch a planted mistake: transposed CoutPad / BK, hi and lo swapped, the scale not inverted, a chunk boundary off by one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mx as MX   # noqa: E402
from pointreggpt_amd import _lib   # noqa: E402

F32, BF16, MXFP8, F16X3 = 0, 1, 2, 3
MAIN, S2D, UP, MXD, MXS, H16, SPLIT, SPLIT_SCALE, UP_SPLIT, UP_SPLIT_SCALE, S2D_OIHW, UP_OIHW = range(12)   # PRG_PACK_*
CONV2, UPSAMPLE = 1, 2
SHAPES = ((72, 40, 3), (8, 8, 1))


def packed(w, dtype, packing, np_dtype, role=0):
    Cout, Cin, K, _ = w.shape
    w = np.ascontiguousarray(w, np.float32)
    buf, n = np.empty(64 * w.nbytes + 65536, np.uint8), C.c_int64(0)
    _lib.check(_lib.load().prg_debug_pack_conv(w.ctypes.data_as(C.c_void_p), Cout, Cin, K, dtype, role, packing,
                                               buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)), "prg_debug_pack_conv")
    return buf[:n.value].view(np_dtype).copy()


def weights(Cout, Cin, K, seed=0):
    return np.random.default_rng(seed).standard_normal((Cout, Cin, K, K)).astype(np.float32) * np.float32(0.05)


def bf16_bits(x):
    """round to nearest even, NaN kept (quiet bit set)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, ((u >> 16) | 0x40).astype(np.uint16), r)


def tiled(x, BK, mistake=None):
    """[Cout][Cin][KH][KW] -> [tap = kh*KW+kw][chunk][CoutPad][BK], zero padded in Cout (to 64) and channel"""
    Cout, Cin, KH, KW = x.shape
    cp, kcn = (Cout + 63) // 64 * 64, (Cin + BK - 1) // BK
    pad = np.zeros((cp, kcn * BK + 1, KH * KW), x.dtype)
    off = 1 if mistake == "chunk" else 0                   # the planted mistake: every chunk boundary one channel late
    pad[:Cout, off:off + Cin] = x.reshape(Cout, Cin, KH * KW)
    pad = pad[:, :kcn * BK]
    t = pad.reshape(cp, kcn, BK, KH * KW).transpose(3, 1, 0, 2)
    if mistake == "transposed":
        t = t.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(t)


def split_ref(w, mistake=None):
    Cout = w.shape[0]
    cp = (Cout + 63) // 64 * 64
    m = np.abs(w.reshape(Cout, -1)).max(axis=1)
    e = np.frexp(m)[1]                                    # m = f 2^e, f in [0.5, 1)
    live = (m >= 2.0 ** -100) & np.isfinite(m)
    k = np.where(live, 10 - e, 0)
    mul = np.ldexp(np.float32(1), k).astype(np.float32)
    scale = np.ones(cp, np.float32)
    scale[:Cout] = np.ldexp(np.float32(1), k if mistake == "scale" else -k)
    v = w * mul[:, None, None, None]
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    if mistake == "swapped":
        hi, lo = lo, hi
    tm = "chunk" if mistake == "chunk" else None
    return np.concatenate([tiled(hi.view(np.uint16), 32, tm), tiled(lo.view(np.uint16), 32, tm)], axis=3).reshape(-1), scale


@pytest.mark.parametrize("shape", SHAPES)
def test_main_packing_float_and_bf16(shape):
    w = weights(*shape)
    w[0, 0, 0, 0], w[1, 1, 0, 0] = np.nan, np.float32(1.00390625)       # NaN is kept; 1 + 2^-8 is a tie: rounds to even (1.0)
    got32, got16 = packed(w, F32, MAIN, np.uint32), packed(w, BF16, MAIN, np.uint16)
    assert np.array_equal(got32, tiled(w.view(np.uint32), 16).reshape(-1))
    assert np.array_equal(got16, tiled(bf16_bits(w), 32).reshape(-1))
    assert bf16_bits(np.float32([1.00390625, 1.01171875]))[0] == 0x3F80 and bf16_bits(np.float32([1.01171875]))[0] == 0x3F82
    for mistake in ("transposed", "chunk"):
        assert not np.array_equal(got32, tiled(w.view(np.uint32), 16, mistake).reshape(-1)), mistake
        assert not np.array_equal(got16, tiled(bf16_bits(w), 32, mistake).reshape(-1)), mistake


def test_f16_twin():
    w = weights(64, 64, 3)                                 # (h16_eligible: Cin = Cout, a multiple of 64, the second conv of a block)
    got = packed(w, BF16, H16, np.uint16, CONV2)
    assert np.array_equal(got, tiled(w.astype(np.float16).view(np.uint16), 32).reshape(-1))
    assert not np.array_equal(got, tiled(w.astype(np.float16).view(np.uint16), 32, "transposed").reshape(-1))
    assert packed(w, BF16, H16, np.uint16, 0).size == 0    # only conv2 has the twin


@pytest.mark.parametrize("shape", SHAPES)
def test_split_form_and_scales(shape):
    w = weights(*shape)
    w[2] = 0.0                                             # a dead channel and a denormal-sized one: both stay unscaled and finite
    w[3] = 0.0
    w[3, 0, 0, 0] = np.float32(2.0 ** -110)
    got, got_scale = packed(w, F16X3, SPLIT, np.uint16), packed(w, F16X3, SPLIT_SCALE, np.float32)
    ref, ref_scale = split_ref(w)
    assert np.array_equal(got, ref) and np.array_equal(got_scale, ref_scale)
    assert got_scale[2] == 1.0 and got_scale[3] == 1.0 and np.isfinite(got_scale).all()
    assert np.isfinite(got.view(np.float16).astype(np.float32)).all()
    assert not np.array_equal(got, split_ref(w, "swapped")[0])
    assert not np.array_equal(got, split_ref(w, "chunk")[0])
    assert not np.array_equal(got_scale, split_ref(w, "scale")[1])


def e4m3_value(b):
    b = b.astype(np.int64)
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    x = np.where(e == 0, np.ldexp(m.astype(np.float64), -9), np.ldexp(1.0 + m / 8.0, e - 7))
    return np.where(s == 1, -x, x)


def test_mx_packing_against_the_oracle():
    Cout, Cin = 64, 128                                    # (mx_eligible: multiples of 64 both ways, so this packing never pads)
    w = weights(Cout, Cin, 3)
    w[5, 32:64] = 0.0                                      # an all-zero block: scale byte 0
    data = packed(w, MXFP8, MXD, np.uint8).reshape(9, Cin // 64, 64, 64)          # [tap][64-channel chunk][CoutPad][64]
    scales = packed(w, MXFP8, MXS, np.uint8).reshape(9, Cin // 64, 64, 2)         # one E8M0 byte per 32 channels
    val = e4m3_value(data).reshape(9, Cin // 64, 64, 2, 32) * np.exp2(scales.astype(np.float64) - 127)[..., None]
    got = val.transpose(2, 1, 3, 4, 0).reshape(Cout, Cin, 3, 3)                    # -> [Cout][chunk, block, k][tap]
    assert np.array_equal(got, MX.mx_quantize_dequantize(w, axis=1))
    assert not np.array_equal(val.transpose(2, 3, 1, 4, 0).reshape(Cout, Cin, 3, 3), MX.mx_quantize_dequantize(w, axis=1))   # block / chunk swapped


def test_space_to_depth_and_sub_pixel_tensors():
    Co, Ci = 5, 3
    w4 = weights(Co, Ci, 4)
    weq = np.zeros((Co, 4 * Ci, 3, 3), np.float32)         # (test_downsample_equals_two_by_two_taps_over_space_to_depth, test_host_logic.py)
    for ky in range(4):
        for kx in range(4):
            by, dy, bx, dx = ky >> 1, ky & 1, kx >> 1, kx & 1
            weq[:, (2 * dy + dx) * Ci:(2 * dy + dx + 1) * Ci, 1 + by, 1 + bx] = w4[:, :, ky, kx]
    assert np.array_equal(packed(w4, BF16, S2D_OIHW, np.float32).reshape(weq.shape), weq)
    # nearest x2 then 3x3 / pad 1: output sub-pixel dy sees kernel rows {0 | 1, 2} (dy = 0) or {0, 1 | 2} (dy = 1) on its two source rows
    w3 = weights(Co, Ci, 3).astype(np.float64)
    rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    up = np.zeros((4, Co, Ci, 2, 2))
    for dy in (0, 1):
        for dx in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    up[2 * dy + dx, :, :, a, b] = sum(w3[:, :, ky, kx] for ky in rows[dy][a] for kx in rows[dx][b])
    got = packed(w3.astype(np.float32), BF16, UP_OIHW, np.float32).reshape(up.shape)
    assert np.array_equal(got, up.astype(np.float32))
    assert not np.array_equal(got, up[[0, 2, 1, 3]].astype(np.float32))            # dy and dx swapped in the phase index


def test_split_stem_fragments_and_their_scales():
    """The f16x3 stem: w [64][Cin][7][7] as MFMA A fragments [Cin][2 row tiles][hi | lo][4 k-steps][64 lanes][8] (lane -> output channel
    rt * 32 + lane % 32, kernel row 2 kk + lane // 32, j = kernel column; row 7 and column 7 are zero), every output channel scaled by
    its own power of two.  Through the arena hook on a one-level MaskUnet whose stem channels differ in size by up to 2^6."""
    from pointreggpt_amd import weights as W
    from pointreggpt_amd.unet import _cfg_c, flatten_state_dict
    cfg = W.maskunet_config(64, dim_mults=(1,))
    flat = flatten_state_dict(cfg, W.synth_state_dict(cfg, 3))
    Cin = cfg.in_channels
    stem = flat[:64 * Cin * 49].reshape(64, Cin, 7, 7)     # (the stem comes first in the state dict)
    stem *= np.exp2(np.arange(64) % 7 - 3).astype(np.float32)[:, None, None, None]
    stem[5] = 0.0
    stem[6] = 0.0
    stem[6, 0, 0, 0] = np.float32(2.0 ** -110)

    def arena(i, dt):
        buf, n, cc = np.empty(1 << 20, np.uint8), C.c_int64(0), _cfg_c(cfg)
        _lib.check(_lib.load().prg_debug_weight_arena(C.byref(cc), flat.ctypes.data_as(C.c_void_p), flat.size, F16X3, 14, i,
                                                      buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)), "prg_debug_weight_arena")
        return buf[:n.value].view(dt).copy()

    got, got_scale = arena(9, np.uint16), arena(10, np.float32)                    # PRG_ARENA_STEM_SPLIT, PRG_ARENA_STEM_SPLIT_SCALE
    m = np.abs(stem.reshape(64, -1)).max(axis=1)
    k = np.where(m >= 2.0 ** -100, 10 - np.frexp(m)[1], 0)
    v = stem * np.ldexp(np.float32(1), k).astype(np.float32)[:, None, None, None]
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    ref = np.zeros((Cin, 2, 2, 4, 64, 8), np.uint16)
    for half, x in enumerate((hi, lo)):
        pad = np.zeros((64, Cin, 8, 8), np.uint16)
        pad[:, :, :7, :7] = x.view(np.uint16)
        # [co = rt*32 + l][c][kh = 2*kk + g][j] -> [c][rt][kk][lane = g*32 + l][j]
        ref[:, :, half] = pad.reshape(2, 32, Cin, 4, 2, 8).transpose(2, 0, 3, 4, 1, 5).reshape(Cin, 2, 4, 64, 8)
    assert np.array_equal(got_scale, np.ldexp(np.float32(1), -k).astype(np.float32))
    assert len(set(got_scale.tolist())) >= 7 and got_scale[5] == 1.0 and got_scale[6] == 1.0
    assert np.array_equal(got, ref.reshape(-1))
    assert not np.array_equal(got, ref[:, :, ::-1].reshape(-1))                     # hi and lo swapped
