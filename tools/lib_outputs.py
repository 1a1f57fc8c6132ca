#!/usr/bin/env python
"""Outputs of the HIP library on a fixed case list, for bit-for-bit A/B of two builds (a refactor against its parent).

  PRG_HIP_LIB=/path/to/libprg_hip.so python tools/lib_outputs.py OUT.npz     # every case, synthetic weights, fixed seeds
  python tools/lib_outputs.py --compare A.npz B.npz                            # per case: identical or not; exit 1 on any difference

The cases cover every weight packing a handle can build (the kernels are deterministic, so two builds that pack the same bytes
give the same bits): the conditional dim-64 U-Net at 128 x 128 with B = 2 and 16 in all four modes, the switches read during
weight preparation, the MaskUnet's 3-channel stems, a dim-16 network on the generic paths and an 8-step sampler chain with and
without graph capture.  They also cover every branch of the forward pass's host code (csrc/unet.hip): small shapes (B = 2 at
64 x 64, and at 40 x 40 where tiles do not divide and the second conv of a block has no fused prologue) under each switch that
moves a ResnetBlock onto another path, and the debug taps, which turn the fused head off.  The f16x3 networks reach every
instantiation of conv_split.hip / conv_split512.hip but conv3x3_split_kernel<4, 32, 2> (choose_conv at 256 CUs); the kind
"conv_fused" launches that one alone (prg_debug_conv_fused).  The network cases reach the fused ResnetBlock tail, linear attention
with the library's own choice of row-sum form and the bf16 bottleneck core at N = 64 and 256 only; the kinds "attention_core",
"attention_block" and "resblock_tail" launch every instantiation of attn_fused.hip, attn_split.hip and resblock_tail.hip through
the test hooks, on the small shapes of tests/test_gpu_attention.py and tests/test_gpu_resblock_tail.py.  The library reads its
PRG_* switches once per process: every switch setting runs in a child of its own."""
import json
import os
import subprocess
import sys

MODES = ("fp32", "bf16", "mxfp8", "f16x3")
TAPS = ("init_conv", "down0_block0", "down0_attn", "down0_out", "mid_attn", "up0_out", "final_res")   # + "augment": MaskUnet


def SMALL(mode):
    return [("unet", 64, 2, S, mode) for S in (64, 40)]


# (environment of the child process, [(kind, dim, B, S, mode), ...])
GROUPS = [
    ({}, [("unet", 64, B, 128, m) for m in MODES for B in (2, 16)]
         + [("maskunet", 64, 2, 128, m) for m in ("bf16", "f16x3")]
         + [("unet", 16, 3, 32, m) for m in MODES]
         + [("chain8_graph", 64, 2, 128, "bf16"), ("chain8_nograph", 64, 2, 128, "bf16")]
         + [("unet", 64, 2, S, m) for m in MODES for S in (40, 64)]
         + [("maskunet", 64, 2, 64, m) for m in ("fp32", "mxfp8")]
         + [(k, 64, 2, 64, m) for k in ("unet_taps", "maskunet_taps") for m in ("bf16", "fp32")]),
    ({"PRG_SPLIT_UP2X2": "1"}, [("unet", 64, B, 128, "f16x3") for B in (2, 16)]),
    ({"PRG_LA_KSHIFT": "0"}, [("unet", 64, B, 128, "bf16") for B in (2, 16)]),
    ({"PRG_FUSED_ATTN": "0"}, [("unet", 64, B, 128, "bf16") for B in (2, 16)]),
    # the branches of UnetImpl::resblock / attention / forward: slabs everywhere, no h16, no res_conv epilogue, no fused head, ...
    ({"PRG_GN_ACC": "0"}, SMALL("bf16") + [("chain8_graph", 64, 2, 64, "bf16"), ("chain8_nograph", 64, 2, 64, "bf16")]),
    ({"PRG_H16": "0"}, SMALL("bf16")),
    ({"PRG_RES_EPILOGUE": "0"}, SMALL("bf16")),
    ({"PRG_HEAD_FUSE": "0"}, SMALL("bf16")),
    ({"PRG_CONV_C64": "0"}, SMALL("bf16")),
    # a bf16 handle whose convs report no accumulators
    ({"PRG_CONV_WS": "0", "PRG_CONV_C64": "0", "PRG_CONV_W256": "0", "PRG_CONV_DOWN_W256": "0"}, SMALL("bf16")),
    ({"PRG_W256_MIN_TILES": "1"}, SMALL("bf16")),
    # switches of the conv selection (tests/golden/conv_dispatch.json) that change a kernel at these shapes
    ({"PRG_CONV_W256": "0"}, SMALL("bf16") + [("unet", 64, 2, 128, "bf16")]),
    ({"PRG_UP2X2": "0"}, SMALL("bf16") + [("unet", 64, 2, 128, "bf16")]),
    ({"PRG_SPLIT_P64": "1"}, SMALL("f16x3")),
    ({"PRG_SPLIT_W512": "2"}, SMALL("f16x3")),
    ({"PRG_SPLIT_FULLATTN": "0", "PRG_SPLIT_LA_ONLINE": "0"}, SMALL("f16x3")),
    ({}, [("conv_fused", 64, 2, 12, "f16x3")]),
    ({}, [("attention_core", 0, 0, 0, m) for m in ("bf16", "f16x3")] + [("attention_block", 0, 0, 0, m) for m in ("bf16", "f16x3")]),
    ({"PRG_SPLIT_LA_ONLINE": "0"}, [("attention_block", 0, 0, 0, "f16x3")]),
    ({}, [("resblock_tail", 0, 0, 0, "bf16")]),
]
# kind "conv_fused": one f16x3 3x3 conv through the test hook, statistics off and as slabs.  (tag, (B, C0, C1, Cout, H, W), prologue,
# expected (family, th, tw)): the smallest shapes of tests/test_gpu_conv_fused_f32.py that select the 4 x 32 split halo tile
CONV_FUSED = [("two_source", (2, 64, 64, 64, 12, 32), None, ("split_halo", 4, 32)),
              ("prologue", (2, 64, 0, 128, 12, 32), "tables", ("split_halo", 4, 32))]


def case_name(env, case):
    kind, dim, B, S, mode = case
    tag = "".join(f"+{k}={v}" for k, v in sorted(env.items()))
    return f"{kind}{dim}_B{B}_S{S}_{mode}{tag}"


def run_conv_fused(name, res):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_conv_fused_f32_refs import F16X3, make_case32
    from test_gpu_conv_fused import OFF, SLABS, run
    for i, (tag, shape, pro, want) in enumerate(CONV_FUSED):
        d = make_case32(shape, pro=pro, seed=900 + i)
        for stats in (OFF, SLABS):
            got = run(d, stats=stats, storage=F16X3, want_slabs=True)
            assert got["choice"][:3] == want, (tag, got["choice"])
            for k in ("out", "slabs", "sums", "coef_a", "coef_b"):
                if k in got:
                    res[f"{name}:{tag}:stats{stats}:{k}"] = got[k].numpy()


def run_attention(kind, mode, name, res):
    """attention_core: the bottleneck core's matrix-pipe kernels (full_attn_mfma_kernel<2, 4, 8>, full_attn_mfma_big_kernel<16, 2>,
    <32, 4>, <32, 2>; full_attn_split_kernel<4, 1>, <8, 2>, <16, 4>, <32, 4>, <8, 1>, <32, 2> on the tests' shapes, and <16, 1>, which
    needs B >= 32 at N = 512).  attention_block: bf16 every la_kmax<C>, la_ctx<C, *, *> and la_out<C, *> (family E keeps the static bound at
    every width) with a partial tile (N = 100) and a short last slab (576); f16x3 la_ctx_split<C, online>, la_out_split<C>."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_attention_refs import FULL_MFMA_N, FULL_SPLIT_N, block_case
    from test_gpu_attention import core_case, run_block, run_core
    if kind == "attention_core":
        big = [(32, 1024)] if mode == "bf16" else [(32, 256), (32, 512), (32, 1024)]
        for B, N in [(3, n) for n in (FULL_MFMA_N if mode == "bf16" else FULL_SPLIT_N)] + big:
            for fam in ("F1", "F2"):
                res[f"{name}:{fam}:B{B}:N{N}"] = run_core(core_case(fam, B, N, mode, 0), mode, 0, 1).numpy()
    elif mode == "bf16":
        for Cc in (64, 128, 256):
            for N in (100, 576):
                W, x = block_case(Cc, 3, N, "E", "bf16")[:2]
                for shift_mode in (0, 1):
                    for psum in (0, 1):
                        rc, out, used = run_block(W, x, "bf16", shift_mode, psum)
                        assert rc == 0 and used == shift_mode, (Cc, N, shift_mode, psum, rc, used)
                        res[f"{name}:C{Cc}:N{N}:shift{shift_mode}:psum{psum}"] = out.numpy()
    else:
        for Cc in (64, 128):
            W, x = block_case(Cc, 3, 576, "R", "f16x3")[:2]
            rc, out, used = run_block(W, x, "f16x3", -1, -1)
            assert rc == 0 and used == 0, (Cc, rc, used)
            res[f"{name}:C{Cc}:N576"] = out.numpy()


def run_resblock_tail(name, res):
    """resblock_tail_fused_kernel<128, 64>, <192, 128>, <256, 128>: a partial second tile and a second block of one tile"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_gpu_resblock_tail import CONFIGS, T_TILES, inputs, run
    for C0, C1, Cout in CONFIGS:
        for N in (100, 64 * T_TILES + 64):
            d = inputs(C0, C1, Cout, 3, N, "normal", 1000 * Cout + 10 * N + 3 + C0)
            for ip in (0, 1):
                res[f"{name}:{C0}+{C1}->{Cout}:N{N}:in_place{ip}"] = run(d, False, False, ip).numpy()
                for sigmoid in (False, True) if Cout == 64 else ():
                    res[f"{name}:{C0}+{C1}->{Cout}:N{N}:in_place{ip}:head:sigmoid{int(sigmoid)}"] = run(d, True, sigmoid, ip).numpy()


def run_group(index, out):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pointreggpt_amd import weights as W
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import MaskUnet, Unet
    env, cases = GROUPS[index]
    res = {}
    for case in cases:
        kind, dim, B, S, mode = case
        if kind == "conv_fused":
            run_conv_fused(case_name(env, case), res)
            continue
        if kind in ("attention_core", "attention_block"):
            run_attention(kind, mode, case_name(env, case), res)
            continue
        if kind == "resblock_tail":
            run_resblock_tail(case_name(env, case), res)
            continue
        g = torch.Generator().manual_seed(1000 + dim + B + S)
        taps = ()
        if kind in ("maskunet", "maskunet_taps"):
            net = MaskUnet(dim, dtype=mode).load_state_dict(W.synth_state_dict(W.maskunet_config(dim), 21))
            if kind == "maskunet_taps":
                net.set_taps(True)
                taps = TAPS + ("augment",)
            y = net(torch.rand((B, 1, S, S), generator=g).cuda())
        else:
            net = Unet(dim, dtype=mode).load_state_dict(W.synth_state_dict(W.unet_config(dim), 20))
            pc = torch.rand((B, 4), generator=g)
            if kind in ("unet", "unet_taps"):
                if kind == "unet_taps":
                    net.set_taps(True)
                    taps = TAPS
                x = torch.randn((B, 1, S, S), generator=g)
                t = torch.randint(0, 1000, (B,), generator=g)
                y = net(x.cuda(), t.cuda(), pc.cuda())
            else:
                d8 = GaussianDiffusion(net, image_size=S, timesteps=8)
                cond = torch.rand((B, 2, S, S), generator=g) * 2 - 1
                noise = torch.randn((d8.n_draws, B, 1, S, S), generator=g)
                y = d8.sample(param_cond=pc, img_cond=cond, noise=noise, use_graph=kind == "chain8_graph")
        torch.cuda.synchronize()
        res[case_name(env, case)] = y.cpu().numpy()
        for k in taps:
            res[f"{case_name(env, case)}:{k}"] = net.get_tap(k, B, max_floats=B * 512 * S * S).cpu().numpy()
        net.close()
    np.savez(out, **res)


def run_all(out):
    import numpy as np
    merged = {}
    for i, (env, _) in enumerate(GROUPS):
        part = f"{out}.part{i}.npz"
        subprocess.run([sys.executable, os.path.abspath(__file__), "--group", str(i), part], env=dict(os.environ, **env),
                       check=True, timeout=900)
        with np.load(part) as z:
            merged.update({k: z[k] for k in z.files})
        os.remove(part)
    np.savez(out, **merged)
    print(json.dumps({"lib": os.environ.get("PRG_HIP_LIB", "default"), "cases": len(merged), "out": out}))


def compare(a, b):
    import numpy as np
    za, zb = np.load(a), np.load(b)
    bad = sorted(set(za.files) ^ set(zb.files))
    for k in bad:
        print(f"{k:56s} only in one file")
    for k in sorted(set(za.files) & set(zb.files)):
        same = za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes()
        finite = bool(np.isfinite(za[k]).all())
        note = "" if same else f"  max |a - b| = {float(np.abs(za[k].astype(np.float64) - zb[k]).max()):.3e}" if za[k].shape == zb[k].shape else "  shapes differ"
        print(f"{k:56s} {'identical' if same else 'DIFFERENT'}{'' if finite else '  (non-finite values)'}{note}")
        if not same:
            bad.append(k)
    print(f"{len(za.files)} cases, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 4 and sys.argv[1] == "--group":
        run_group(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) == 2 and not sys.argv[1].startswith("-"):
        run_all(sys.argv[1])
    else:
        sys.exit(__doc__)
