"""Generate tests/golden/*.npz by running the REAL reference (/root/reference, read-only) in this container.

Run:  python tools/make_goldens.py            (needs /root/reference; takes ~1-2 minutes on 8 cores)

Every fixture stores the inputs and the reference's outputs.  Network weights are NOT stored: they come from
the build's deterministic initialiser (pointreggpt_amd.weights.synth_state_dict(cfg, seed)), loaded into the
reference modules with load_state_dict, and are regenerated bit-identically by the tests.
Fixture ids follow SURVEY.md §8c (G1..G12); G19/G20 (round 3: chains of real length on the calibrated denoiser,
~40 minutes of CPU) and G12b..G18 (round 2) were added later; G12b..G17 cover (benchmarked 128x128 configuration,
the reference's shipped 256x256 resolution, float64 "exact arithmetic" envelopes, DDIM with known pixels > 1).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from _refimport import import_reference  # noqa: E402
from pointreggpt_amd import synthetic, weights  # noqa: E402

sd, dc = import_reference()
OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)
torch.set_grad_enabled(False)


def save(name, **arrs):
    conv = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        conv[k] = np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **conv)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB  [{', '.join(conv)}]")


def ref_unet(dim, seed):
    m = sd.Unet(dim=dim, param_cond_dim=4, dim_mults=(1, 2, 4, 8), channels=1)
    m.load_state_dict(weights.synth_state_dict(weights.unet_config(dim), seed))
    return m.eval()


def ref_maskunet(dim, seed, final_bias=None):
    m = dc.MaskUnet(dim=dim, dim_mults=(1, 2, 4, 8))
    m.load_state_dict(weights.synth_state_dict(weights.maskunet_config(dim), seed, final_bias=final_bias))
    return m.eval()


def ref_diffusion(model, S, T=1000, steps=None):
    return sd.GaussianDiffusion(model, image_size=S, timesteps=T, sampling_timesteps=steps, loss_type="l1",
                                objective="pred_x0", beta_schedule="sigmoid", ddim_sampling_eta=1.0,
                                is_ddnm_sampling=True)


def hook_taps(model, names):
    """Forward hooks on reference sub-modules -> dict of outputs."""
    taps = {}
    for key, mod in names.items():
        mod.register_forward_hook(lambda _m, _i, o, key=key: taps.__setitem__(key, o.detach().clone()))
    return taps


def recorded_noise(fn, seed):
    """Run fn() under torch.manual_seed(seed) while recording every randn / randn_like draw, in order."""
    draws = []
    o_randn, o_like = torch.randn, torch.randn_like

    def randn(*a, **k):
        t = o_randn(*a, **k)
        draws.append(t.clone())
        return t

    def randn_like(x, **k):
        t = o_like(x, **k)
        draws.append(t.clone())
        return t

    torch.manual_seed(seed)
    torch.randn, torch.randn_like = randn, randn_like
    try:
        out = fn()
    finally:
        torch.randn, torch.randn_like = o_randn, o_like
    return out, (torch.stack(draws) if draws else torch.zeros(0))


def mixed_cond(B, S, seed):
    """A DDNM condition with a mixed known/unknown mask: (B,2,S,S) in [-1,1]."""
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand((B, 1, S, S), generator=g) * 0.3 + 0.05
    mask = (torch.rand((B, 1, S, S), generator=g) > 0.45).float()
    depth = depth * mask
    return torch.cat([depth, mask], 1) * 2 - 1


# ------------------------------------------------------------------------------------------------
def g1_schedule():
    m = ref_unet(8, 7)
    d = ref_diffusion(m, 32)
    names = ["betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
             "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
             "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
             "posterior_mean_coef1", "posterior_mean_coef2", "loss_weight"]
    out = {n: getattr(d, n) for n in names}
    for steps in (5, 50, 250):
        t = torch.linspace(-1, 999, steps=steps + 1)
        out[f"ddim_times_{steps}"] = np.array(list(reversed(t.int().tolist())), dtype=np.int64)
    d8 = ref_diffusion(m, 32, T=8)
    for n in names:
        out["T8_" + n] = getattr(d8, n)
    save("G1_schedule", **out)


def g2_intrinsics():
    K = np.array([[[f, 0.0, 320.0], [0.0, f, 240.0], [0.0, 0.0, 1.0]] for f in
                  (585.0, 572.0, 583.0, 540.021232, 570.342205, 533.069214)], dtype=np.float32)
    out = {"K": K}
    for S in (32, 64, 128, 256):
        out[f"S{S}"] = np.stack([sd.intrinsic_transform(k, resize=S, centercrop=S) for k in K])
        out[f"S{S}_batched"] = sd.intrinsic_transform(K, resize=S, centercrop=S)
    out["none"] = sd.intrinsic_transform(K[4])
    save("G2_intrinsic_transform", **out)


def g3_pose():
    out = {}
    for s in (0, 1, 12345):
        np.random.seed(s)
        out[f"pose_seed{s}"] = sd.random_sample_pose(4)
        out[f"after_seed{s}"] = np.random.rand(2)       # pins how much of the stream was consumed
        np.random.seed(s)
        out[f"intr_seed{s}"] = sd.random_sample_intrinsic(16)
    save("G3_random_sample_pose", **out)


def g4_pc2depth():
    rng = np.random.default_rng(4)
    B, N, S = 2, 20000, 64
    K = np.stack([sd.intrinsic_transform(np.array([[570.342205, 0, 320], [0, 570.342205, 240], [0, 0, 1]],
                                                  dtype=np.float32), resize=S, centercrop=S)] * B).astype(np.float32)
    K[1, 0, 0] *= 1.03
    pc = np.empty((B, N, 3), dtype=np.float32)
    pc[..., 2] = rng.uniform(0.5, 4.0, (B, N))
    pc[..., 0] = rng.uniform(-1.6, 1.6, (B, N)) * pc[..., 2]      # spills outside the frame on both sides
    pc[..., 1] = rng.uniform(-1.6, 1.6, (B, N)) * pc[..., 2]
    # exact half-pixel ties: x*fx/z + cx == k + 0.5  (fx=cx-free construction: choose z=fx, x = k+0.5-cx)
    for b in range(B):
        fx, fy, cx, cy = K[b, 0, 0], K[b, 1, 1], K[b, 0, 2], K[b, 1, 2]
        for i, k in enumerate(range(0, 40)):
            pc[b, i] = [np.float32(k + 0.5) - cx, np.float32(k % 7 + 0.5) - cy, 1.0]
            pc[b, i, 0] /= fx
            pc[b, i, 1] /= fy
    pc[:, 100:160, 2] *= -1                                        # behind the camera
    pc[:, 160:170, 2] = 0.0                                        # z == 0
    pc[:, 170:180, 0] = np.nan                                     # NaN coordinates
    pc[:, 200:1200] = pc[:, 1200:2200]                             # exact duplicates -> collisions
    pc[:, 200:1200, 2] *= np.float32(1.25)
    pc[:, 200:1200, :2] *= np.float32(1.25)                        # same pixel, farther: must lose
    valid = rng.random((B, N)) > 0.1
    d, m = sd.pc2depth_tensor(torch.tensor(pc), torch.tensor(valid), torch.tensor(K), image_size=[S, S])
    # non-square + empty cloud
    d2, m2 = sd.pc2depth_tensor(torch.tensor(pc[:, :5000]), torch.tensor(valid[:, :5000]), torch.tensor(K),
                                image_size=[48, 80])
    save("G4_pc2depth", pc=pc, valid=valid, K=K, depth=d, mask=m, depth_48x80=d2, mask_48x80=m2)


def g5_g6_reproject():
    S, B = 64, 3
    depth, K, pose = synthetic.synth_batch(5, range(B), S)
    pose[2] = np.eye(4, dtype=np.float32)                          # identity: bit-exact round trip
    dm = torch.tensor(depth) * 10
    d, m = sd.reproject_tensor(dm, torch.tensor(K), torch.tensor(pose), clip=[0, 10])
    d05, m05 = sd.reproject_tensor(dm, torch.tensor(K), torch.tensor(pose), clip=[0.5, 10])
    pc, valid = sd.depth2pc_tensor(dm, torch.tensor(K), clip=[0.5, 10])
    pc0, valid0 = sd.depth2pc_tensor(dm, torch.tensor(K), clip=[0, 10], invalid_num=0.0)
    clouds = {}
    for b in range(B):
        p = sd.point_cloud(depth[b, 0] * 10, K[b], clip=[0.5, 10])
        clouds[f"cloud{b}"] = p
        clouds[f"cloud{b}_common"] = (p - pose[b, :3, 3]) @ pose[b, :3, :3]
    # the generator's per-scene form: float32 numpy cloud, numpy rigid move, batch-of-one z-buffer (sd:2531-2547)
    gen = {}
    for b in range(B):
        cloud = clouds[f"cloud{b}"].astype(np.float32)
        moved = cloud @ pose[b, :3, :3].T + pose[b, :3, 3]
        dd, mm = sd.pc2depth_tensor(torch.tensor(moved[None]), torch.ones((1, len(moved)), dtype=torch.bool),
                                    torch.tensor(K[b][None]), image_size=[S, S])
        gen[f"gen_depth{b}"], gen[f"gen_mask{b}"] = dd[0], mm[0]
    save("G5_G6_reproject_unproject", depth=depth, K=K, pose=pose, rpj_depth=d, rpj_mask=m, rpj05_depth=d05,
         rpj05_mask=m05, pc=pc, pc_valid=valid, pc0=pc0, pc0_valid=valid0, **clouds, **gen)


def g7_unet_taps():
    out = {}
    for dim, S in ((8, 32), (16, 32)):
        m = ref_unet(dim, 7)
        taps = hook_taps(m, {"init_conv": m.init_conv, "down0_block0": m.downs[0][0], "down0_attn": m.downs[0][2],
                             "down0_out": m.downs[0][3], "mid_attn": m.mid_attn, "up0_out": m.ups[0][3],
                             "final_res": m.final_res_block})
        g = torch.Generator().manual_seed(70 + dim)
        x = torch.randn((2, 1, S, S), generator=g)
        t = torch.tensor([3, 871])
        pc = torch.tensor([[75.7486, 76.0456, 32.5, 32.0], [80.0, 79.5, 31.5, 32.5]]) * (S / 64)
        y = m(x, t, pc)
        out.update({f"d{dim}_x": x, f"d{dim}_t": t, f"d{dim}_pc": pc, f"d{dim}_y": y})
        out.update({f"d{dim}_tap_{k}": v for k, v in taps.items()})
    save("G7_unet_small_taps", **out)


def g8_unet_full():
    m = ref_unet(64, 8)
    g = torch.Generator().manual_seed(8)
    S = 64
    x = torch.randn((2, 1, S, S), generator=g)
    t = torch.tensor([0, 999])
    pc = torch.tensor([[75.7486, 76.0456, 32.5, 32.0], [73.1, 73.4, 32.5, 32.0]])
    save("G8_unet_dim64", x=x, t=t, pc=pc, y=m(x, t, pc))


def g9_g10_sampler():
    S, B, dim = 32, 2, 16
    m = ref_unet(dim, 9)
    pc = torch.tensor([[37.87, 38.02, 16.25, 16.0], [36.5, 36.7, 16.25, 16.0]])
    cond = mixed_cond(B, S, 9)
    out = {"pc": pc, "cond": cond}
    d = ref_diffusion(m, S)
    g = torch.Generator().manual_seed(99)
    x = torch.randn((B, 1, S, S), generator=g)
    out["x"] = x
    # G9a: single ancestral steps
    for t in (999, 500, 1, 0):
        (img, x0), nz = recorded_noise(lambda t=t: d.p_sample(x, t, pc, cond), 100 + t)
        out[f"ps{t}_img"], out[f"ps{t}_x0"] = img, x0
        out[f"ps{t}_noise"] = nz[0] if len(nz) else torch.zeros_like(x)
    # G9b: unconditional (img_cond=None) single step
    (img, x0), nz = recorded_noise(lambda: d.p_sample(x, 500, pc, None), 77)
    out["ps500_nocond_img"], out["ps500_nocond_noise"] = img, nz[0]
    # G10a: full short ancestral chain T=8
    d8 = ref_diffusion(m, S, T=8)
    img, nz = recorded_noise(lambda: d8.sample(param_cond=pc, img_cond=cond, disable_tqdm=True), 1234)
    out["chain8_out"], out["chain8_noise"] = img, nz
    # G10b: 1000 -> 5 DDIM
    d5 = ref_diffusion(m, S, T=1000, steps=5)
    img, nz = recorded_noise(lambda: d5.sample(param_cond=pc, img_cond=cond, disable_tqdm=True), 4321)
    out["ddim5_out"], out["ddim5_noise"] = img, nz
    # G10c: DDIM without a condition
    img, nz = recorded_noise(lambda: d5.sample(param_cond=pc, img_cond=None, disable_tqdm=True), 555)
    out["ddim5_nocond_out"], out["ddim5_nocond_noise"] = img, nz
    save("G9_G10_sampler", **out)


def g11_maskunet():
    S, B = 32, 2
    depth, _, _ = synthetic.synth_batch(11, range(B), S)
    depth[1, 0, :6, :6] = 0.0                                      # an all-zero 3x3 window
    x = torch.tensor(depth)
    aug = dc.DepthAugment()(x)
    out = {"depth": x, "augment": aug}
    for dim in (8, 16):
        m = ref_maskunet(dim, 11, final_bias=4.0)                 # logit shift: probabilities straddle 0.99
        prob = m(x)
        out[f"d{dim}_prob"] = prob
    # threshold + condition assembly exactly as Generator.generate does (sd:2564-2570)
    prob = out["d16_prob"]
    g = torch.Generator().manual_seed(11)
    hit = torch.rand((B, 1, S, S), generator=g) > 0.3
    thr = float(np.quantile(prob.numpy(), 0.4))                    # mixed mask whatever the weights give
    images = x.clone()
    mask_crt = prob > thr
    images[~mask_crt] = 0
    mask_rpj = hit & mask_crt
    cond = sd.normalize_to_neg_one_to_one(torch.cat([images, mask_rpj], dim=1))
    out.update(hit=hit, thr=np.float32(thr), corrected=images, mask_out=mask_rpj, img_cond=cond)
    save("G11_maskunet", **out)


def g12_end_to_end():
    """Config 1: one synthetic pair at 64x64, 50-step DDIM, dim=64 networks, depth-map form of the pipeline."""
    S, B = 64, 1
    depth, K, pose = synthetic.synth_batch(12, range(B), S)
    unet, mask = ref_unet(64, 12), ref_maskunet(64, 13, final_bias=6.0)
    d = ref_diffusion(unet, S, T=1000, steps=50)
    Kt, Pt = torch.tensor(K), torch.tensor(pose)
    d_rpj, hit = sd.reproject_tensor(torch.tensor(depth) * 10, Kt, Pt, clip=[0, 10])
    images_rpj = d_rpj * 0.1
    prob1 = mask(images_rpj)
    thr1 = float(np.quantile(prob1.numpy(), 0.25))
    mask_crt = prob1 > thr1
    images_rpj[~mask_crt] = 0
    mask_rpj = hit & mask_crt
    img_cond = sd.normalize_to_neg_one_to_one(torch.cat([images_rpj, mask_rpj], dim=1))
    pc = sd.param_vector(Kt)
    images, nz = recorded_noise(lambda: d.sample(param_cond=pc, img_cond=img_cond, disable_tqdm=True), 2024)
    prob2 = mask(images)
    thr2 = float(np.quantile(prob2.numpy(), 0.25))
    out_img = images.clone()
    out_img[~(prob2 > thr2)] = 0
    cloud = sd.point_cloud(out_img[0, 0].numpy() * 10, K[0], clip=[0.5, 10])
    cloud = (cloud - pose[0, :3, 3]) @ pose[0, :3, :3]
    save("G12_end_to_end_64", depth=depth, K=K, pose=pose, rpj_depth=d_rpj * 0.1, rpj_mask=hit, prob1=prob1,
         thr1=np.float32(thr1), img_cond=img_cond, noise=nz, sampled=images, prob2=prob2, thr2=np.float32(thr2),
         depth_out=out_img, cloud=cloud)


# ------------------------------------------------------------------------------------------------
# Round-2 fixtures: the BENCHMARKED configuration (dim 64, 128x128) and the reference's shipped setting (256x256),
# each with the oracle evaluated in float64 on the same fp32 weights ("exact arithmetic": the oracle is pinned
# bit-exactly to the reference in fp32, so its fp64 evaluation is the reference's function without roundoff) — the
# distance |reference fp32 - exact| is the noise floor any fp32 implementation with another summation order sits in.
# ------------------------------------------------------------------------------------------------
from oracle import diffusion as OD  # noqa: E402  (tools may use the oracle; the product never does)
from oracle import geometry as OG  # noqa: E402
from oracle import unet as OU  # noqa: E402

TAP_NAMES = ("init_conv", "down0_block0", "down0_attn", "down0_out", "mid_attn", "up0_out", "final_res")
N_TAP_SAMPLES = 8192


def f64(sdict):
    return {k: v.double() for k, v in sdict.items()}


def tap_index(name, numel, seed):
    """Fixed pseudo-random flat indices into a (B,C,H,W) tap (full taps at 128x128 would be 8 MB each)."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    return np.sort(rng.choice(numel, size=min(N_TAP_SAMPLES, numel), replace=False)).astype(np.int64)


def unet_fixture(prefix, dim, wseed, S, B, xseed, t, out):
    """Reference U-Net forward + subsampled taps, and the same from the float64 oracle."""
    m = ref_unet(dim, wseed)
    taps = hook_taps(m, {"init_conv": m.init_conv, "down0_block0": m.downs[0][0], "down0_attn": m.downs[0][2],
                         "down0_out": m.downs[0][3], "mid_attn": m.mid_attn, "up0_out": m.ups[0][3],
                         "final_res": m.final_res_block})
    g = torch.Generator().manual_seed(xseed)
    x = torch.randn((B, 1, S, S), generator=g)
    tt = torch.tensor(t)
    pc = (torch.tensor([[75.7486, 76.0456, 32.5, 32.0], [73.1, 73.4, 32.5, 32.0]]) * (S / 64))[:B]
    y = m(x, tt, pc)
    sdict = weights.synth_state_dict(weights.unet_config(dim), wseed)
    taps64 = {}
    y64 = OU.unet_forward(f64(sdict), x.double(), tt.double(), pc.double(), taps=taps64)
    taps32 = {}
    y32 = OU.unet_forward(sdict, x, tt, pc, taps=taps32)
    assert torch.equal(y32, y), "oracle fp32 must reproduce the reference bit-exactly"
    out.update({f"{prefix}x": x, f"{prefix}t": tt, f"{prefix}pc": pc, f"{prefix}y": y, f"{prefix}y64": y64})
    for k in TAP_NAMES:
        assert torch.equal(taps32[k], taps[k]), k
        idx = tap_index(k, taps[k].numel(), wseed)
        out[f"{prefix}tap_{k}_idx"] = idx
        out[f"{prefix}tap_{k}"] = taps[k].reshape(-1)[idx]
        out[f"{prefix}tap_{k}_64"] = taps64[k].reshape(-1)[idx]
    e = (y.double() - y64).abs().max().item()
    print(f"  {prefix or 'unet'} S={S}: |ref32 - exact|max = {e:.3e} on |y|max {y.abs().max().item():.2f}")


def g13_unet_128():
    out = {}
    unet_fixture("", 64, 13, 128, 2, 13, [3, 900], out)
    save("G13_unet_dim64_128", **out)


def g14_chain_128():
    """dim-64 ancestral chain (timesteps=8) at 128x128, B=2, mixed DDNM mask, stored noise; + the float64 oracle chain."""
    S, B = 128, 2
    m = ref_unet(64, 14)
    pc = torch.tensor([[151.5, 152.1, 64.5, 64.0], [146.2, 146.8, 64.5, 64.0]])
    cond = mixed_cond(B, S, 14)
    d8 = ref_diffusion(m, S, T=8)
    img, nz = recorded_noise(lambda: d8.sample(param_cond=pc, img_cond=cond, disable_tqdm=True), 1414)
    sdict = weights.synth_state_dict(weights.unet_config(64), 14)
    sch8 = OD.schedule(8)
    den32 = lambda x, t, c: OU.unet_forward(sdict, x, t, c)
    o32 = OD.sample(sch8, den32, pc, cond, S, OD.stored_noise(nz))
    assert torch.equal(o32, img), "oracle fp32 chain must reproduce the reference bit-exactly"
    s64 = f64(sdict)
    den64 = lambda x, t, c: OU.unet_forward(s64, x.double(), t.double(), c.double())
    o64 = OD.sample(sch8, den64, pc, cond.double(), S, lambda k: nz[k].double())
    print(f"  chain8@128: |ref32 - exact|max = {(img.double() - o64).abs().max().item():.3e}")
    save("G14_chain8_dim64_128", pc=pc, cond=cond, noise=nz, out=img, out64=o64)


def g15_maskunet_128():
    S, B = 128, 2
    depth, _, _ = synthetic.synth_batch(15, range(B), S)
    x = torch.tensor(depth)
    m = ref_maskunet(64, 15, final_bias=6.0)
    prob = m(x)
    sdict = weights.synth_state_dict(weights.maskunet_config(64), 15, final_bias=6.0)
    logit64 = OU.maskunet_forward(f64(sdict), x.double(), return_logits=True)
    assert torch.equal(OU.maskunet_forward(sdict, x), prob)
    save("G15_maskunet_dim64_128", depth=x, prob=prob, prob64=torch.sigmoid(logit64))


def g16_unet_256():
    """The reference's shipped resolution (generate_dataset.py:34-49): one dim-64 U-Net forward at 256x256, B=1."""
    out = {}
    unet_fixture("", 64, 16, 256, 1, 16, [417], out)
    save("G16_unet_dim64_256", **out)


def g17_ddim_cond_gt1():
    """DDIM transitions whose known pixels exceed 1 after normalisation (a memory point farther than 10 m): ddim_sample
    clamps only the raw network output (sd:1197-1201), the replaced values enter the state unclamped (sd:1218, 1371)."""
    S, B, dim = 32, 2, 16
    m = ref_unet(dim, 9)
    pc = torch.tensor([[37.87, 38.02, 16.25, 16.0], [36.5, 36.7, 16.25, 16.0]])
    cond = mixed_cond(B, S, 17)
    g = torch.Generator().manual_seed(171)
    far = (torch.rand((B, 1, S, S), generator=g) < 0.2) & (cond[:, 1:2] > 0)
    cond[:, 0:1][far] = 1.0 + torch.rand((int(far.sum()),), generator=g)          # depth in (1, 2]: 10-15 m
    d5 = ref_diffusion(m, S, T=1000, steps=5)
    img, nz = recorded_noise(lambda: d5.sample(param_cond=pc, img_cond=cond, disable_tqdm=True), 1717)
    d8 = ref_diffusion(m, S, T=8)
    img8, nz8 = recorded_noise(lambda: d8.sample(param_cond=pc, img_cond=cond, disable_tqdm=True), 1718)
    save("G17_ddim_cond_gt1", pc=pc, cond=cond, ddim5_noise=nz, ddim5_out=img, chain8_noise=nz8, chain8_out=img8)


def g18_refine_and_tester():
    """has_refine_step for both samplers (sd:1307-1314, 1374-1388), occlusion_filter (sd:446-463) and
    random_sample_transform (sd:377-415): the pieces Tester.sample / Tester.generate add to the generator's path."""
    S, B, dim = 32, 2, 16
    m = ref_unet(dim, 9)
    pc = torch.tensor([[37.87, 38.02, 16.25, 16.0], [36.5, 36.7, 16.25, 16.0]])
    cond = mixed_cond(B, S, 18)
    out = {"pc": pc, "cond": cond}
    d5 = ref_diffusion(m, S, T=1000, steps=5)
    img, nz = recorded_noise(lambda: d5.sample(param_cond=pc, img_cond=cond, disable_tqdm=True, has_refine_step=True), 1801)
    out["ddim5_refine_out"], out["ddim5_refine_noise"] = img, nz
    d8 = ref_diffusion(m, S, T=8)
    img, nz = recorded_noise(lambda: d8.sample(param_cond=pc, img_cond=cond, disable_tqdm=True, has_refine_step=True), 1802)
    out["chain8_refine_out"], out["chain8_refine_noise"] = img, nz
    # occlusion filter on a reprojected synthetic batch (metres), incl. an image with an empty hit mask
    depth, K, pose = synthetic.synth_batch(18, range(3), 64)
    d_rpj, hit = sd.reproject_tensor(torch.tensor(depth) * 10, torch.tensor(K), torch.tensor(pose), clip=[0, 10])
    hit[2] = False
    d_rpj[2] = 0
    of_d, of_m = sd.occlusion_filter(d_rpj.clone(), hit.clone())
    out.update(of_depth_in=d_rpj, of_mask_in=hit, of_depth_out=of_d, of_mask_out=of_m)
    for s_ in (0, 7):
        np.random.seed(s_)
        out[f"rst_seed{s_}"] = sd.random_sample_transform(K, image_size=64)
        out[f"rst_after_seed{s_}"] = np.random.rand(2)
    out["rst_K"] = K
    save("G18_refine_occlusion_transform", **out)


def g0_host_tables():
    """Float32 tables the reference evaluates with torch on ITS host and whose last bit matters downstream: the
    SinusoidalPosEmb frequencies (sd:645-657).  A 1-ulp difference in a frequency times t <= 999 moves every time
    embedding by up to 6e-5; the same reference code on two CPUs ends a 50-step chain 4.5e-5 apart (tools/chain_budget.py).
    The fixtures below were produced with THESE tables; the GPU tests hand them to the library (prg_unet_set_time_freqs)."""
    import math
    out = {}
    for dim in (8, 16, 64):
        half = dim // 2
        f = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
        emb = sd.SinusoidalPosEmb(dim)(torch.tensor([1.0, 999.0]))
        assert torch.equal(emb[:, :half], (torch.tensor([1.0, 999.0])[:, None] * f[None, :]).sin())
        out[f"freqs_dim{dim}"] = f
    # DDIM coefficients (sd:1357-1368): sigma = eta sqrt((1 - a/a')(1 - a')/(1 - a)), c = sqrt(1 - a' - sigma^2) are float32
    # expressions with cancellation; two x86 hosts disagree by 8.7e-6 (relative) on c of the FIRST transition, which is
    # 3.4e-5 in the state at once (tools/_dump_chain.py).  The product evaluates them with torch on ITS host exactly as the
    # reference does; comparisons with these fixtures need the values of the host that made them.
    from pointreggpt_amd.diffusion import GaussianDiffusion

    class _Net:
        channels = out_dim = 1
        random_or_learned_sinusoidal_cond = False

    for steps in (5, 50, 250):
        rows = GaussianDiffusion(_Net(), image_size=32, timesteps=1000, sampling_timesteps=steps).step_table()
        out[f"ddim{steps}_rows"] = np.array([[r["c_x0"], r["c_x"], r["c_eps"], r["sigma"], r["sqrt_recip"], r["sqrt_recipm1"]]
                                             for r in rows], dtype=np.float32)
        out[f"ddim{steps}_t"] = np.array([r["t"] for r in rows], dtype=np.int32)
    # the ancestral chain's per-step noise scale exp(0.5 * logvar) is a float32 exp evaluated on the host too (sd:1280)
    rows = GaussianDiffusion(_Net(), image_size=32, timesteps=1000).step_table()
    out["anc1000_rows"] = np.array([[r["c_x0"], r["c_x"], r["c_eps"], r["sigma"], r["sqrt_recip"], r["sqrt_recipm1"]]
                                    for r in rows], dtype=np.float32)
    out["anc1000_t"] = np.array([r["t"] for r in rows], dtype=np.int32)
    save("G0_host_tables", **out)


def g12b_envelope():
    """Noise floor of the parity metric on the G12 chain (64x64, 50-step DDIM, dim 64): the reference against (a) itself
    with one thread instead of eight (another oneDNN blocking: another summation order) and (b) exact arithmetic."""
    g = np.load(os.path.join(OUT, "G12_end_to_end_64.npz"))
    sdict = weights.synth_state_dict(weights.unet_config(64), 12)
    mask_sd = weights.synth_state_dict(weights.maskunet_config(64), 13, final_bias=6.0)
    sch = OD.schedule(1000)
    K, pose = g["K"], g["pose"]
    pc = OG.param_vector(torch.tensor(K))
    cond, noise, ref = torch.tensor(g["img_cond"]), torch.tensor(g["noise"]), torch.tensor(g["sampled"])

    def cloud_of(img, thr2, msd):
        prob2 = OU.maskunet_forward(msd, img)
        o = torch.where(prob2 > thr2, img, torch.zeros_like(img))
        c = OG.point_cloud(o[0, 0].numpy() * 10, K[0], (0.5, 10.0))
        return OG.inverse_pose_apply(c, pose[0]), (o > 0)

    den = lambda x, t, c: OU.unet_forward(sdict, x, t, c)
    torch.set_num_threads(1)
    s1 = OD.sample(sch, den, pc, cond, 64, OD.stored_noise(noise), sampling_steps=50)
    torch.set_num_threads(8)
    s8 = OD.sample(sch, den, pc, cond, 64, OD.stored_noise(noise), sampling_steps=50)
    assert torch.equal(s8, ref)
    s64d = f64(sdict)
    den64 = lambda x, t, c: OU.unet_forward(s64d, x.double(), t.double(), c.double())
    s64 = OD.sample(sch, den64, pc, cond.double(), 64, lambda k: noise[k].double(), sampling_steps=50)
    thr2 = float(g["thr2"])
    c_ref, m_ref = cloud_of(ref, thr2, mask_sd)
    assert np.array_equal(c_ref, g["cloud"])
    c1, m1 = cloud_of(s1, thr2, mask_sd)
    c64, m64 = cloud_of(s64.float(), thr2, mask_sd)
    rep = {"depth_1thread": (s1 - ref).abs().max().item(), "depth_exact": (s64 - ref.double()).abs().max().item()}
    for name, c, mk in (("xyz_1thread", c1, m1), ("xyz_exact", c64, m64)):
        rep[name] = float(np.abs(c - c_ref).max()) if torch.equal(mk, m_ref) else float("nan")
    print("  G12 envelope:", rep)
    save("G12b_envelope", sampled_1thread=s1, sampled_exact=s64,
         **{k: np.float64(v) for k, v in rep.items()})


# ------------------------------------------------------------------------------------------------
# Round-3 fixtures: chains of REAL length on the calibrated (non-saturating) synthetic denoiser.
#   G19  1000-step ancestral DDNM chain (p_sample_loop, sd:1283-1317) at 64x64, B=1, dim 64
#   G20  250-step DDIM chain (ddim_sample, sd:1319-1392: the setting generate_dataset.py ships) at 128x128, B=1, dim 64
# Each: a synthetic scene reprojected by the reference (sd:268-286) as the DDNM condition, the reference's result with 8
# threads and with 1 thread (the reference's own reproducibility: the floor of the parity metric), the float64 twin, the
# state after 20 transitions (so the CPU suite can check the oracle on a prefix in seconds), and the unprojected clouds.
# The noise (16 MB per chain) is NOT stored: the reference draws it from torch's global CPU generator, so the fixture keeps
# the seed and a sha256 of the draws; tests regenerate it with the same torch build and refuse to run on a mismatch.
# ------------------------------------------------------------------------------------------------
import hashlib  # noqa: E402


def regenerate_noise(seed, n_draws, shape):
    """The reference's draw order from torch's global CPU generator: randn(shape), then one randn_like per transition."""
    torch.manual_seed(seed)
    return torch.stack([torch.randn(shape) for _ in range(n_draws)])


def long_chain_fixture(name, S, wseed, scene_seed, noise_seed, steps):
    B, T = 1, 1000
    depth, K, pose = synthetic.synth_batch(scene_seed, range(B), S)
    Kt, Pt = torch.tensor(K), torch.tensor(pose)
    d_rpj, hit = sd.reproject_tensor(torch.tensor(depth) * 10, Kt, Pt, clip=[0, 10])
    img_cond = sd.normalize_to_neg_one_to_one(torch.cat([d_rpj * 0.1, hit], dim=1))
    pc = sd.param_vector(Kt)
    sdict = weights.synth_state_dict(weights.unet_config(64), wseed, calibrated=True)
    m = sd.Unet(dim=64, param_cond_dim=4, dim_mults=(1, 2, 4, 8), channels=1)
    m.load_state_dict(sdict)
    m.eval()
    d = ref_diffusion(m, S, T=T, steps=steps)
    states = {}
    calls = [0]

    def pre(_m, args):
        if calls[0] == 20:
            states["x20"] = args[0].detach().clone()
        calls[0] += 1

    hnd = m.register_forward_pre_hook(pre)
    import time
    t0 = time.time()
    torch.set_num_threads(8)
    img8, nz = recorded_noise(lambda: d.sample(param_cond=pc, img_cond=img_cond, disable_tqdm=True), noise_seed)
    hnd.remove()
    print(f"  {name}: reference, 8 threads: {time.time() - t0:.0f} s ({len(nz)} draws)")
    assert torch.equal(nz, regenerate_noise(noise_seed, len(nz), tuple(nz.shape[1:]))), "noise is not regenerable"
    sha = hashlib.sha256(nz.numpy().tobytes()).hexdigest()
    t0 = time.time()
    torch.set_num_threads(1)
    torch.manual_seed(noise_seed)
    img1 = d.sample(param_cond=pc, img_cond=img_cond, disable_tqdm=True)
    torch.set_num_threads(8)
    print(f"  {name}: reference, 1 thread: {time.time() - t0:.0f} s; |8thr - 1thr|max = {(img8 - img1).abs().max().item():.3e}")
    # the oracle must reproduce the whole chain bit-exactly (the CPU suite re-checks only the 20-transition prefix)
    sch = OD.schedule(T)
    den32 = lambda x, t, c: OU.unet_forward(sdict, x, t, c)
    t0 = time.time()
    o32 = OD.sample(sch, den32, pc, img_cond, S, OD.stored_noise(nz), sampling_steps=steps)
    assert torch.equal(o32, img8), "oracle fp32 chain must reproduce the reference bit-exactly"
    print(f"  {name}: oracle fp32 == reference over the whole chain ({time.time() - t0:.0f} s)")
    s64 = f64(sdict)
    den64 = lambda x, t, c: OU.unet_forward(s64, x.double(), t.double(), c.double())
    t0 = time.time()
    o64 = OD.sample(sch, den64, pc, img_cond.double(), S, lambda k: nz[k].double(), sampling_steps=steps)
    print(f"  {name}: float64 twin {time.time() - t0:.0f} s; |ref - exact|max = {(img8.double() - o64).abs().max().item():.3e}")

    def cloud_of(img):
        c = sd.point_cloud(img[0, 0].numpy() * 10, K[0], clip=[0.5, 10])
        return (c - pose[0, :3, 3]) @ pose[0, :3, :3]

    valid8 = (img8[0, 0] * 10 > 0.5) & (img8[0, 0] * 10 < 10)
    c8, c1, c64 = cloud_of(img8), cloud_of(img1), cloud_of(o64.float())
    same1 = torch.equal(valid8, (img1[0, 0] * 10 > 0.5) & (img1[0, 0] * 10 < 10))
    same64 = torch.equal(valid8, (o64.float()[0, 0] * 10 > 0.5) & (o64.float()[0, 0] * 10 < 10))
    free = ~((img_cond[:, 1:2] + 1) * 0.5 > 0.5)
    rep = {"xyz_spread_1_vs_8_threads_m": float(np.abs(c8 - c1).max()) if same1 else float("nan"),
           "xyz_ref_to_exact_m": float(np.abs(c8 - c64).max()) if same64 else float("nan"),
           "depth_spread_1_vs_8_threads": (img8 - img1).abs().max().item(),
           "depth_ref_to_exact": (img8.double() - o64).abs().max().item(),
           "saturated_fraction_inpainted": float(((img8 <= 0) | (img8 >= 1))[free].float().mean()),
           "inpainted_fraction": float(free.float().mean())}
    print(f"  {name}:", rep)
    save(name, depth=depth, K=K, pose=pose, img_cond=img_cond, pc=pc, noise_seed=np.int64(noise_seed),
         n_draws=np.int64(len(nz)), noise_sha256=np.frombuffer(bytes.fromhex(sha), dtype=np.uint8),
         noise_probe=nz[[0, 1, len(nz) - 1]].reshape(3, -1)[:, :8], x20=states["x20"], sampled=img8, sampled_1thread=img1,
         sampled_exact=o64, cloud=c8, wseed=np.int64(wseed), steps=np.int64(steps),
         **{k: np.float64(v) for k, v in rep.items()})


def g19_chain1000_64():
    long_chain_fixture("G19_chain1000_ancestral_64", 64, 19, 19, 1900, 1000)


def g20_ddim250_128():
    long_chain_fixture("G20_ddim250_128", 128, 20, 20, 2000, 250)


def g21_ddim250_256():
    """BASELINE configs[4]'s chain in the reference's shipped setting: 250-step DDIM at 256x256 (generate_dataset.py:34-49).
    ~70 minutes of CPU (the 1-thread reference run dominates)."""
    long_chain_fixture("G21_ddim250_256", 256, 21, 21, 2100, 250)


def g21b_ddim250_256():
    """G21 on a calibrated seed (round-3 VERDICT: 16.6 % of G21's in-painted pixels sit on the clamp in the reference itself).
    Seed 20 was picked by screening candidates on the GPU (tools/screen_chain_seeds.py: 0.47 % saturated at 256x256)."""
    long_chain_fixture("G21b_ddim250_256", 256, 20, 20, 2000, 250)


def g22_chain1000_128():
    """THE HEADLINE CHAIN (BASELINE metric / configs[1]): 1000-step ancestral DDNM (`p_sample_loop`, sd:1283-1317) at 128x128,
    dim 64, with the weights (seed 1, calibrated) and scene 0 of the inputs `bench.py` itself times.  ~1.5 h of CPU."""
    long_chain_fixture("G22_chain1000_ancestral_128", 128, 1, 0, 2200, 1000)


def recorded_draws(fn, d, seed, normal_seed):
    """recorded_noise's sibling for chains that also draw keep masks: run fn() under torch.manual_seed(seed) and record, per
    evaluation of the network d.model (= per transition, refine row included), the Tensor.uniform_ draw made after it and the
    threshold the reference itself compares that draw with (the right-hand side of its `uniform_(0, 1) > p`, as float32: torch
    compares a float32 tensor with a 0-dim float64 tensor in float32).  The normals come from a generator of their own
    (normal_seed), so that chains of one sampler share them and the file stays small; they are recorded in order like
    recorded_noise does.  Returns out, normals (n,B,1,S,S), uniforms (rows,B,1,S,S) with NaN slabs where nothing was drawn,
    keep_p (rows,) float32 with -1 where nothing was drawn."""
    normals, rows, last = [], [], [None]
    gn = torch.Generator().manual_seed(normal_seed)
    o_randn, o_like, o_uniform, o_gt = torch.randn, torch.randn_like, torch.Tensor.uniform_, torch.Tensor.__gt__

    def randn(*a, **k):
        t = o_randn(*a, generator=gn, **k)
        normals.append(t.clone())
        return t

    def randn_like(x, **k):
        t = o_randn(x.shape, generator=gn, dtype=x.dtype, device=x.device)
        normals.append(t.clone())
        return t

    def uniform_(self, *a, **k):
        t = o_uniform(self, *a, **k)
        assert rows and rows[-1]["u"] is None, "a uniform_ draw outside a transition, or two in one"
        rows[-1]["u"] = t.clone()
        last[0] = t
        return t

    def gt(self, other):
        if last[0] is not None and self is last[0]:
            assert self.dtype == torch.float32
            rows[-1]["p"] = np.float32(float(other))
            last[0] = None
        return o_gt(self, other)

    hook = d.model.register_forward_hook(lambda *_: rows.append({"u": None, "p": np.float32(-1.0)}))
    torch.manual_seed(seed)
    torch.randn, torch.randn_like, torch.Tensor.uniform_, torch.Tensor.__gt__ = randn, randn_like, uniform_, gt
    try:
        out = fn()
    finally:
        torch.randn, torch.randn_like, torch.Tensor.uniform_, torch.Tensor.__gt__ = o_randn, o_like, o_uniform, o_gt
        hook.remove()
    assert last[0] is None and all((r["u"] is None) == (r["p"] < 0) for r in rows)
    nan = torch.full_like(normals[0], float("nan"))
    return out, torch.stack(normals), torch.stack([nan if r["u"] is None else r["u"] for r in rows]), \
        np.array([r["p"] for r in rows], dtype=np.float32)


def g23_ddnm_dropout():
    """Stochastic DDNM (sd:1075-1094, 1210-1227) and denoise() (sd:1411-1427) on the G9_G10 network, pc and cond, p = 0.3:
    per chain the output, the uniforms re-indexed to one slab per transition and the reference's own thresholds; the normals
    per sampler (`T8_normals`, `ddim5_normals`: every chain of that sampler drew exactly these).  Every output has at least
    60 % of its pixels strictly inside (0,1), so that the comparison is not one of clamped values."""
    S, B, dim = 32, 2, 16
    m = ref_unet(dim, 9)
    pc = torch.tensor([[37.87, 38.02, 16.25, 16.0], [36.5, 36.7, 16.25, 16.0]])
    cond = mixed_cond(B, S, 9)
    out = {"pc": pc, "cond": cond, "p": np.float64(0.3)}
    # name: (T, steps, schedule, is_ddnm_sampling, refine, method, seed of the uniforms)
    chains = {"T8_linear": (8, None, "linear", True, False, "sample", 2301),
              "T8_none_refine": (8, None, "none", True, True, "sample", 2302),
              "ddim5_none": (1000, 5, "none", True, False, "sample", 2303),
              "ddim5_linear_refine": (1000, 5, "linear", True, True, "sample", 2304),
              "denoise_T8": (8, None, "none", False, False, "denoise", 2305),
              "denoise_ddim5_refine": (1000, 5, "none", False, True, "denoise", 2306)}
    shared = {}
    for name, (T, steps, sched, ddnm, refine, method, seed) in chains.items():
        d = sd.GaussianDiffusion(m, image_size=S, timesteps=T, sampling_timesteps=steps, loss_type="l1", objective="pred_x0",
                                 beta_schedule="sigmoid", ddim_sampling_eta=1.0, is_ddnm_sampling=ddnm,
                                 ddnm_sampling_dropout=0.3, ddnm_dropout_schedule=sched)
        sampler = "T8" if steps is None else "ddim5"
        img, nz, un, kp = recorded_draws(lambda: getattr(d, method)(param_cond=pc, img_cond=cond, disable_tqdm=True,
                                                                    has_refine_step=refine), d, seed, 2300 if steps is None else 2350)
        inside = float(((img > 0) & (img < 1)).float().mean())
        print(f"  {name}: {int((kp >= 0).sum())} uniform draws over {len(kp)} rows, {inside:.2f} of the output inside (0,1)")
        assert inside >= 0.6, "choose another seed: the chain's output is mostly clamped"
        assert len(kp) == (T if steps is None else steps) + int(refine) and un.shape[0] == len(kp)
        if sampler + "_normals" in shared:
            assert torch.equal(shared[sampler + "_normals"], nz)
        shared[sampler + "_normals"] = nz
        out[name + "_out"], out[name + "_uniforms"], out[name + "_keep_p"] = img, un, kp
    out.update(shared)
    save("G23_ddnm_dropout", **out)


G24_OBJECTIVES = ("pred_x0", "pred_noise", "pred_v")
G24_SCHEDULES = ("sigmoid", "cosine", "linear")
G24_BUFFERS = ("betas", "alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
               "posterior_mean_coef2", "posterior_log_variance_clipped")
# the pairs that get all four chains (ancestral / ddim5, each with and without the refine step); the other five new pairs get one
G24_FULL = (("pred_noise", "cosine"), ("pred_v", "linear"), ("pred_x0", "cosine"))
G24_ONE = {("pred_noise", "linear"): ("ddim5", False), ("pred_noise", "sigmoid"): ("anc", True), ("pred_v", "cosine"): ("ddim5", True),
           ("pred_v", "sigmoid"): ("anc", False), ("pred_x0", "linear"): ("anc", False)}
G24_SEED = 2400


def g24_anc_T(schedule):
    """Timesteps of the short ancestral chain: below 21 the linear schedule's last beta exceeds 1 and the reference samples NaN."""
    return 40 if schedule == "linear" else 8


def g24_objectives():
    """pred_noise / pred_v and the linear / cosine schedules (sd:976-994, 1153-1171, 1194-1208) on the G9_G10 network, pc and
    cond.  Per schedule the reference's float64 betas / alphas_cumprod (its schedule function's output and the cumprod its
    constructor takes of it; the class itself keeps float32 copies, which are compared) and the float32 buffers the transition
    table is made of, at T = 1000 and at the short chain's T; per chain the output
    computed with 8 threads and with 1 thread; the normals per sampler (`anc_normals`: 40 slabs, the T = 8 chains drew the first
    8; `ddim5_normals`); one pred_noise chain with ddnm_sampling_dropout = 0.3 and its uniforms; the DDIM rows of this host
    (G0_host_tables' layout) per chain that needs them.  Every output has at least 60 % of its pixels strictly inside (0,1) and
    moves by at most FP32_TOL / 4 = 2.5e-5 between 8 threads and 1."""
    from pointreggpt_amd.diffusion import GaussianDiffusion

    class _Net:
        channels = out_dim = 1
        random_or_learned_sinusoidal_cond = False

    S, B, dim = 32, 2, 16
    m = ref_unet(dim, 9)
    pc = torch.tensor([[37.87, 38.02, 16.25, 16.0], [36.5, 36.7, 16.25, 16.0]])
    cond = mixed_cond(B, S, 9)
    out = {"pc": pc, "cond": cond, "p": np.float64(0.3)}

    def ref(objective, schedule, T, steps=None, dropout=0.0):
        return sd.GaussianDiffusion(m, image_size=S, timesteps=T, sampling_timesteps=steps, loss_type="l1", objective=objective,
                                    beta_schedule=schedule, ddim_sampling_eta=1.0, is_ddnm_sampling=True,
                                    ddnm_sampling_dropout=dropout, ddnm_dropout_schedule="none")

    # ---- schedule arrays: they do not depend on the objective (asserted), so one set per (schedule, T) ----
    fn = {"sigmoid": sd.sigmoid_beta_schedule, "cosine": sd.cosine_beta_schedule, "linear": sd.linear_beta_schedule}
    for schedule in G24_SCHEDULES:
        for T in (1000, g24_anc_T(schedule)):
            betas64 = fn[schedule](T)
            ds = [ref(o, schedule, T) for o in G24_OBJECTIVES]
            assert betas64.dtype == torch.float64 and torch.equal(betas64.to(torch.float32), ds[0].betas)
            for name in G24_BUFFERS:
                assert all(torch.equal(getattr(d, name), getattr(ds[0], name)) for d in ds)
                if name not in ("betas", "alphas_cumprod"):
                    assert getattr(ds[0], name).dtype == torch.float32
                    out[f"{schedule}_T{T}_{name}"] = getattr(ds[0], name)
            # the class keeps float32 copies only; the float64 arrays are the schedule function's and their cumprod (sd:1048-1050)
            out[f"{schedule}_T{T}_betas"] = betas64
            out[f"{schedule}_T{T}_alphas_cumprod"] = torch.cumprod(1.0 - betas64, dim=0)
            assert torch.equal(out[f"{schedule}_T{T}_alphas_cumprod"].to(torch.float32), ds[0].alphas_cumprod)

    # ---- chains ----
    chains = []     # (name, objective, schedule, sampler, refine, dropout)
    for o, s_ in G24_FULL:
        chains += [(f"{o}_{s_}_{smp}{'_refine' if r else ''}", o, s_, smp, r, 0.0) for smp in ("anc", "ddim5") for r in (False, True)]
    chains += [(f"{o}_{s_}_{smp}{'_refine' if r else ''}", o, s_, smp, r, 0.0) for (o, s_), (smp, r) in G24_ONE.items()]
    chains.append(("pred_noise_cosine_anc_dropout", "pred_noise", "cosine", "anc", False, 0.3))
    shared = {}
    for i, (name, o, s_, smp, refine, dropout) in enumerate(chains):
        T, steps = (g24_anc_T(s_), None) if smp == "anc" else (1000, 5)
        d = ref(o, s_, T, steps, dropout)
        res = {}
        for threads in (8, 1):
            torch.set_num_threads(threads)
            res[threads] = recorded_draws(lambda: d.sample(param_cond=pc, img_cond=cond, disable_tqdm=True, has_refine_step=refine),
                                          d, G24_SEED + 1 + i, G24_SEED if smp == "anc" else G24_SEED + 50)
        torch.set_num_threads(8)
        (img, nz, un, kp), (img1, nz1, un1, kp1) = res[8], res[1]
        assert torch.equal(nz, nz1) and torch.equal(un.nan_to_num(7.0), un1.nan_to_num(7.0)) and np.array_equal(kp, kp1)
        inside = min(float(((x > 0) & (x < 1)).float().mean()) for x in (img, img1))
        spread = float((img - img1).abs().max())
        print(f"  {name}: T = {T}, {inside:.2f} of the output inside (0,1), |8 threads - 1 thread|max = {spread:.2e}")
        assert torch.isfinite(img).all() and inside >= 0.6, "choose another seed: the chain's output is mostly clamped"
        assert spread <= 2.5e-5, "choose another seed: the chain amplifies the summation order beyond FP32_TOL / 4"
        assert len(kp) == (T if steps is None else steps) + int(refine) and bool((kp >= 0).any()) == (dropout > 0)
        key = smp + "_normals"
        if key in shared:                       # one stream per sampler: a shorter chain drew a prefix of a longer one's
            n = min(len(nz), len(shared[key]))
            assert torch.equal(shared[key][:n], nz[:n])
        if key not in shared or len(nz) > len(shared[key]):
            shared[key] = nz
        out[name + "_out"], out[name + "_out_1thread"] = img, img1
        if dropout > 0:
            out[name + "_uniforms"], out[name + "_keep_p"] = un, kp
        if steps is not None and f"{s_}_ddim5_rows" not in out:
            rows = GaussianDiffusion(_Net(), image_size=S, timesteps=T, sampling_timesteps=steps, objective=o,
                                     beta_schedule=s_).step_table()
            out[f"{s_}_ddim5_rows"] = np.array([[r["c_x0"], r["c_x"], r["c_eps"], r["sigma"], r["sqrt_recip"], r["sqrt_recipm1"]]
                                               for r in rows], dtype=np.float32)
            out[f"{s_}_ddim5_t"] = np.array([r["t"] for r in rows], dtype=np.int32)
    out["chains"] = np.array([c[0] for c in chains])
    out.update(shared)
    save("G24_objectives", **out)


G25_T = (0, 500, 999)


def g25_stub_output(x, t, pc):
    """The stub network of G25: a fixed elementwise function of (x, t, param_cond), one rounded float32 operation per step, so
    that numpy restates it bit for bit (tests/test_validation_spec.py does)."""
    tf = (t.to(torch.float32) * 1e-3).reshape(-1, 1, 1, 1)
    p0 = (pc[:, 0] * 0.01).reshape(-1, 1, 1, 1)
    return (x * 0.75 + tf * 0.25) - p0


def g25_validation():
    """GaussianDiffusion.q_sample / predict_v / p_losses (sd:1164-1167, 1448-1497) and MaskTrainer.compute_metrics (dc:1229-1275)
    of the reference itself.  B = 3, S = 32, T = 1000, t = (0, 500, 999), a stub network (g25_stub_output).  Per schedule: x_t and
    the pred_v target.  Per (objective, schedule, min-SNR): the float32 loss_weight array.  Per (objective, schedule, loss type,
    min-SNR): p_losses with 8 threads and with 1, and a float64 recomputation from the reference's own float32 terms.  One real
    network (G24's: dim 16, weight seed 9, S = 32, B = 2, pred_x0 / sigmoid, l1): p_losses and the per-sample unweighted means.
    compute_metrics: two batches per threshold (0.5, 0.99) through one AverageMeter set, and a batch whose two masks are empty."""
    import types
    import torch.nn.functional as F

    class _Stub(torch.nn.Module):
        channels = out_dim = 1
        random_or_learned_sinusoidal_cond = False

        def forward(self, x, t, pc):
            return g25_stub_output(x, t, pc)

    B, S, T = 3, 32, 1000
    gen = torch.Generator().manual_seed(2501)
    x0 = torch.rand((B, 1, S, S), generator=gen) * 2 - 1
    noise = torch.randn((B, 1, S, S), generator=gen)
    t = torch.tensor(G25_T)
    pc = torch.tensor([[37.87, 38.02, 16.25, 16.0], [36.5, 36.7, 16.25, 16.0], [40.0, 40.0, 16.0, 16.0]])
    out = {"x0": x0, "noise": noise, "t": t, "pc": pc}

    def ref(model, S_, objective, schedule, loss_type="l1", min_snr=False):
        return sd.GaussianDiffusion(model, image_size=S_, timesteps=T, loss_type=loss_type, objective=objective, beta_schedule=schedule,
                                    min_snr_loss_weight=min_snr, min_snr_gamma=5)

    def terms_of(d, model, x0_, t_, pc_, noise_):
        """The reference's own float32 terms: loss_fn(model_out, target, reduction='none') as p_losses forms them."""
        x = d.q_sample(x_start=x0_, t=t_, noise=noise_)
        u = model(x, t_, pc_)
        target = {"pred_noise": noise_, "pred_x0": x0_}.get(d.objective)
        if target is None:
            target = d.predict_v(x0_, t_, noise_)
        return u, d.loss_fn(u, target, reduction="none").reshape(len(x0_), -1)

    gap = 0.0
    stub = _Stub()
    for schedule in ("sigmoid", "cosine", "linear"):
        d0 = ref(stub, S, "pred_v", schedule)
        out[f"{schedule}_x_t"] = d0.q_sample(x_start=x0, t=t, noise=noise)
        out[f"{schedule}_v"] = d0.predict_v(x0, t, noise)
        if schedule == "sigmoid":
            out["sigmoid_u"] = stub(out["sigmoid_x_t"], t, pc)
        for objective in ("pred_x0", "pred_noise", "pred_v"):
            for min_snr in (False, True):
                key = f"{objective}_{schedule}_snr{int(min_snr)}"
                for loss_type in ("l1", "l2"):
                    d = ref(stub, S, objective, schedule, loss_type, min_snr)
                    assert torch.equal(d.q_sample(x_start=x0, t=t, noise=noise), out[f"{schedule}_x_t"])   # objective-independent
                    out[key + "_loss_weight"] = d.loss_weight
                    res = {}
                    for threads in (8, 1):
                        torch.set_num_threads(threads)
                        res[threads] = d.p_losses(x0, t, pc, noise=noise)
                    torch.set_num_threads(8)
                    _u, terms = terms_of(d, stub, x0, t, pc, noise)
                    assert terms.dtype == torch.float32
                    f64 = (terms.to(torch.float64).mean(dim=1) * d.loss_weight[t].to(torch.float64)).mean()
                    out[f"{key}_{loss_type}_loss"], out[f"{key}_{loss_type}_loss_1thread"] = res[8], res[1]
                    out[f"{key}_{loss_type}_loss_f64"] = f64
                    if float(f64) != 0.0:
                        gap = max(gap, abs(float(res[8]) - float(f64)) / abs(float(f64)), abs(float(res[1]) - float(f64)) / abs(float(f64)))
    print(f"  largest relative gap between the reference's float32 loss and its float64 recomputation: {gap:.2e}")
    out["f32_f64_gap"] = np.float64(gap)

    # ---- one real network: G24's ----
    m = ref_unet(16, 9)
    pc2 = pc[:2].clone()
    depth, _K, _pose = synthetic.synth_batch(3, range(2), S)
    rx0 = torch.from_numpy(depth) * 2 - 1
    rnoise = torch.randn((2, 1, S, S), generator=gen)
    rt = torch.tensor([100, 700])
    d = ref(m, S, "pred_x0", "sigmoid", "l1")
    res = {}
    for threads in (8, 1):
        torch.set_num_threads(threads)
        _u, terms = terms_of(d, m, rx0, rt, pc2, rnoise)
        res[threads] = (d.p_losses(rx0, rt, pc2, noise=rnoise), terms.mean(dim=1))
    torch.set_num_threads(8)
    out.update(net_x0=rx0, net_noise=rnoise, net_t=rt, net_pc=pc2, net_loss=res[8][0], net_loss_1thread=res[1][0],
               net_unweighted=res[8][1], net_unweighted_1thread=res[1][1])
    print(f"  real network: p_losses = {float(res[8][0]):.6f}, unweighted per sample {res[8][1].tolist()}, "
          f"|8 threads - 1 thread| = {float((res[8][1] - res[1][1]).abs().max()):.2e}")

    # ---- compute_metrics, called unbound on a namespace ----
    def trainer():
        return types.SimpleNamespace(accelerator=types.SimpleNamespace(is_main_process=True), metrics={"current": {}})

    def matrix_of(data, prob, thr):
        return torch.bincount(2 * (data["mask"] > thr).flatten() + (prob > thr).flatten(), minlength=4).reshape((2, 2))

    def batch(seed, empty=False):
        g = torch.Generator().manual_seed(seed)
        inp = torch.rand((2, 1, 16, 16), generator=g)
        lab = inp + (torch.rand((2, 1, 16, 16), generator=g) - 0.5) * 0.02
        prob = torch.rand((2, 1, 16, 16), generator=g)
        prob[0, 0, 0, :4] = 0.5                      # exactly at the threshold: not output
        prob[1, 0, 1, :4] = torch.tensor(0.99)
        mask = (torch.abs(lab - inp) < 0.005).to(dtype=torch.float32)
        if empty:
            prob, mask = prob * 0.25, torch.zeros_like(mask)
        return {"input_img": inp, "label_img": lab, "mask": mask}, prob

    KEYS = ("MSE", "MAE", "SAE", "mIoU", "PAcc", "FP")
    batches = {"a": batch(2511), "b": batch(2512), "empty": batch(2513, empty=True)}
    for name, (data, prob) in batches.items():
        out.update({f"mask_{name}_input": data["input_img"], f"mask_{name}_label": data["label_img"], f"mask_{name}_mask": data["mask"],
                    f"mask_{name}_prob": prob})
    for thr in (0.5, 0.99):
        tag = f"thr{int(thr * 100)}"
        tr = trainer()
        for name in ("a", "b"):
            data, prob = batches[name]
            dc.MaskTrainer.compute_metrics(tr, data, prob, mask_threshold=thr)
            out[f"mask_{name}_{tag}_values"] = np.array([float(tr.metrics["current"][k].val) for k in KEYS], dtype=np.float64)
            out[f"mask_{name}_{tag}_matrix"] = matrix_of(data, prob, thr)
        out[f"mask_{tag}_avg"] = np.array([float(tr.metrics["current"][k].avg) for k in KEYS], dtype=np.float64)
        tr = trainer()
        data, prob = batches["empty"]
        dc.MaskTrainer.compute_metrics(tr, data, prob, mask_threshold=thr)
        out[f"mask_empty_{tag}_values"] = np.array([float(tr.metrics["current"][k].val) for k in KEYS], dtype=np.float64)
        out[f"mask_empty_{tag}_matrix"] = matrix_of(data, prob, thr)
    out["mask_keys"] = np.array(KEYS)
    save("G25_validation", **out)
    assert os.path.getsize(os.path.join(OUT, "G25_validation.npz")) < 256 * 1024


def spec_fixture():
    import json
    spec = {"unet64": [[k, list(v.shape)] for k, v in sd.Unet(dim=64, param_cond_dim=4).state_dict().items()],
            "mask64": [[k, list(v.shape)] for k, v in dc.MaskUnet(dim=64).state_dict().items()],
            "unet8": [[k, list(v.shape)] for k, v in sd.Unet(dim=8, param_cond_dim=4).state_dict().items()]}
    with open(os.path.join(OUT, "state_dict_spec.json"), "w") as f:
        json.dump(spec, f)
    print("state_dict_spec.json written")


if __name__ == "__main__":
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    jobs = [("g0", g0_host_tables), ("g1", g1_schedule), ("g2", g2_intrinsics), ("g3", g3_pose), ("g4", g4_pc2depth), ("g5", g5_g6_reproject),
            ("g7", g7_unet_taps), ("g8", g8_unet_full), ("g9", g9_g10_sampler), ("g11", g11_maskunet),
            ("g12", g12_end_to_end), ("g12b", g12b_envelope), ("g13", g13_unet_128), ("g14", g14_chain_128),
            ("g15", g15_maskunet_128), ("g16", g16_unet_256), ("g17", g17_ddim_cond_gt1), ("g18", g18_refine_and_tester), ("g19", g19_chain1000_64),
            ("g20", g20_ddim250_128), ("g21", g21_ddim250_256), ("g21b", g21b_ddim250_256), ("g22", g22_chain1000_128), ("g23", g23_ddnm_dropout),
            ("g24", g24_objectives), ("g25", g25_validation), ("spec", spec_fixture)]
    for name, fn in jobs:
        if not only or name in only:
            fn()
