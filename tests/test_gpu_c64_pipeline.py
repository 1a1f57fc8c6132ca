"""conv3x3_c64_kernel's step pipeline on the device (conv_c64.hip; schedule: pointreggpt_amd/csrc/c64_schedule.h, proved for every
step count in tests/test_c64_schedule.py): launches whose workgroups take 1, 1-2, 2-3 and 3-4 tiles, so the three-step producer
loop runs with zero, one and two padding steps and the consumers' early epilogue crosses image boundaries.

Entry points: prg_debug_conv3x3 (bf16, 64 -> 64: the plain instantiation) and prg_debug_block_pair with h16 = 1 (conv1 = the f16-output
instantiation, conv2 = the one with the packed-f16 GroupNorm + SiLU prologue and its per-image coefficient queue).  Inputs and
GroupNorm statistics differ per image.  One float64 reference per entry point, at the largest batch, shared by the smaller ones
(both chains are per-image)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = 8


@pytest.fixture(scope="module")
def lib():
    from pointreggpt_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def batches():
    """B at 128 x 128 (64 tiles of 8 x 32 per image) for tiles = k N + N / 4, k = 1, 2, 3, N = the device's CU count: 5, 9, 13 at 256."""
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return [-(-(k * n + n // 4) // 64) for k in (1, 2, 3)]


def _operands(seed):
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn((64, 64, 3, 3), generator=g) / (3.0 * 8.0)
    w2 = torch.randn((64, 64, 3, 3), generator=g) / (3.0 * 8.0)
    b1, b2 = torch.randn((64,), generator=g), torch.randn((64,), generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn((64,), generator=g), 0.3 * torch.randn((64,), generator=g)
    return w1, b1, gamma, beta, w2, b2


def _images(seed, B, H, Wd):
    """Every image with its own amplitude and offset (so its GroupNorm statistics are its own), every channel with its own scale."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 64, H, Wd), generator=g) * torch.exp(0.5 * torch.randn((1, 64, 1, 1), generator=g))
    return x * torch.exp(0.5 * torch.randn((B, 1, 1, 1), generator=g)) + 0.5 * torch.randn((B, 1, 1, 1), generator=g)


def _conv(lib, x, w, bias):
    out = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    wh, bh = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(bias.numpy())
    B, _, H, Wd = x.shape
    lib.check(lib.load().prg_debug_conv3x3(lib.ptr(x.cuda().contiguous()), wh.ctypes.data_as(C.c_void_p), bh.ctypes.data_as(C.c_void_p),
                                           lib.ptr(out), B, 64, 64, H, Wd, lib.PRG_BF16, lib.stream_ptr()), "prg_debug_conv3x3")
    return out.cpu()


def _pair(lib, x, ops):
    out = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    arrs = [np.ascontiguousarray(t.numpy()) for t in ops]
    B, _, H, Wd = x.shape
    lib.check(lib.load().prg_debug_block_pair(lib.ptr(x.cuda().contiguous()), *[a.ctypes.data_as(C.c_void_p) for a in arrs], lib.ptr(out),
                                              B, 64, 64, H, Wd, GROUPS, 1, lib.stream_ptr()), "prg_debug_block_pair")
    return out.cpu()


def _conv_ref(x, w, bias):
    return torch.nn.functional.conv2d(x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double(), bias.double(), padding=1)


def _pair_ref(x, ops):
    w1, b1, gamma, beta, w2, b2 = ops
    h = _conv_ref(x, w1, b1)
    a = torch.nn.functional.silu(torch.nn.functional.group_norm(h, GROUPS, gamma.double(), beta.double(), eps=1e-5))
    return torch.nn.functional.conv2d(a, w2.double(), b2.double(), padding=1)


def _check_conv(got, ref):
    # the rule of test_gpu_parity.py::test_conv3x3_kernels_one_at_a_time: against a float64 convolution of the same bf16-rounded operands
    # "what remains is fp32 accumulation order and the bf16 rounding of the output (half an ulp = 2^-9 relative)"
    err = (got.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-4 * float(ref.abs().max())
    print(f"conv: max err {float(err.max()):.3e}, worst err - tol {float((err - tol).max()):.3e}")
    assert bool((err <= tol).all()), float((err - tol).max())


def _check_pair(got, ref):
    # the rule of test_gpu_parity.py::test_block_pair_h16_against_float64 for the f16 form: finite, and max error <= 2^-7 max|ref|
    # ("both inside their rounding budgets")
    assert bool(torch.isfinite(got).all())
    err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
    print(f"pair: max err {err:.3e}, bound {2.0 ** -7 * scale:.3e}")
    assert err <= 2.0 ** -7 * scale, (err, scale)


@pytest.fixture(scope="module")
def big(batches):
    """The 128 x 128 inputs at the largest batch and both float64 references; the smaller batches take the leading images."""
    ops = _operands(64128)
    x = _images(128, batches[-1], 128, 128)
    return dict(ops=ops, x=x, conv=_conv_ref(x, ops[0], ops[1]), pair=_pair_ref(x, ops))


def test_one_step_eight_tiles(lib):
    """1 x 32 x 64: eight tiles, eight workgroups, one step each (two padding steps in the three-set loop)."""
    ops = _operands(3264)
    x = _images(32, 1, 32, 64)
    got = _conv(lib, x, ops[0], ops[1])
    _check_conv(got, _conv_ref(x, ops[0], ops[1]))
    assert torch.equal(got, _conv(lib, x, ops[0], ops[1]))
    gotp = _pair(lib, x, ops)
    _check_pair(gotp, _pair_ref(x, ops))
    assert torch.equal(gotp, _pair(lib, x, ops))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_mixed_step_counts_single_conv(lib, batches, big, k):
    """tiles = (k + 1) N + N / 4: workgroups with k + 1 and k + 2 steps in one launch."""
    B = batches[k]
    x = big["x"][:B]
    got = _conv(lib, x, big["ops"][0], big["ops"][1])
    _check_conv(got, big["conv"][:B])
    assert torch.equal(got, _conv(lib, x, big["ops"][0], big["ops"][1]))       # a second call returns the same bits


@pytest.mark.parametrize("k", [0, 1, 2])
def test_mixed_step_counts_block_pair_h16(lib, batches, big, k):
    B = batches[k]
    x = big["x"][:B]
    got = _pair(lib, x, big["ops"])
    _check_pair(got, big["pair"][:B])
    assert torch.equal(got, _pair(lib, x, big["ops"]))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_scene_replicated_gives_equal_slots(lib, batches, big, k):
    """The same image in every slot: whichever workgroup, step and register set a tile lands in, its output is the same bits."""
    B = batches[k]
    x = big["x"][1:2].expand(B, -1, -1, -1).contiguous()
    for got in (_conv(lib, x, big["ops"][0], big["ops"][1]), _pair(lib, x, big["ops"])):
        assert bool((got == got[:1]).all())
    # and they are the bits this image has in the mixed batch's slot 1 for the plain conv (no cross-image term in it)
    assert torch.equal(_conv(lib, x, big["ops"][0], big["ops"][1])[0], _conv(lib, big["x"][:B], big["ops"][0], big["ops"][1])[1])
