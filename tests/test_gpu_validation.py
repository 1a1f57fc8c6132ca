"""The validation kernels (csrc/validate.hip) on the GPU.

  * prg_q_sample / prg_diffusion_loss / prg_mask_metrics alone against their numpy specifications (pointreggpt_amd/validate.py):
    bit for bit on stored noise, at HW in {4, 36, 1024, 4100} and B in {1, 3} (4100 = one full block of 4096 pixels and a partial
    one: the partial-block path and a second pass over two partials), t in {0, T - 1}, three objectives, two loss types;
  * Philox noise: reproducible, a function of the sample's seed alone, not the sampler's stream, regenerated identically by the
    loss kernel, standard normal (mean within 5 / sqrt(N), variance within 5 sqrt(2 / N) of 1: five standard errors);
  * NaN and threshold rules; guard rows around every output;
  * p_losses end to end on G24's network: bitwise the specification applied to Unet.forward's output, in fp32 and bf16, and in
    fp32 within FP32_TOL (the project's bound on a float32 network output; the L1 mean is 1-Lipschitz in it) plus the summation
    bound (N - 1 + 3) 2^-24 of the reference's p_losses (tests/golden/G25_validation.npz);
  * sample() returns the same bits before and after a p_losses call on the same network."""
import ctypes as C

import numpy as np
import pytest
import torch

from pointreggpt_amd import validate as V
from pointreggpt_amd import weights as W
from pointreggpt_amd.diffusion import make_schedule

pytestmark = pytest.mark.gpu

T = 1000
# (2, 37): rows that are not 16-byte aligned take the kernels' pixel-by-pixel loads (stored noise only)
SHAPES = [(B, HW) for HW in (4, 36, 1024, 4100) for B in (1, 3)] + [(2, 37)]
SEEDS = [0x9E3779B97F4A7C15, 7, 2 ** 63 + 12345]
GUARD = 7.0
FP32_TOL = 1e-4
U24 = 2.0 ** -24


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def hip():
    from pointreggpt_amd import _lib
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import Unet

    class NS:
        pass

    ns = NS()
    ns._lib, ns.lib, ns.GaussianDiffusion, ns.Unet = _lib, _lib.load(), GaussianDiffusion, Unet
    return ns


@pytest.fixture(scope="module")
def data():
    """(B, HW) -> the inputs of one shape, drawn once: x0, noise, u, and per t in {0, T - 1} the coefficients of the sigmoid schedule."""
    buf = make_schedule(T, "sigmoid")
    cache = {}

    def get(B, HW):
        if (B, HW) not in cache:
            rng = np.random.default_rng(1000 * B + HW)
            d = {k: rng.standard_normal((B, HW)).astype(np.float32) for k in ("x0", "noise", "u")}
            d["x0"] = np.clip(d["x0"], -1, 1)
            for t in (0, T - 1):
                tt = torch.full((B,), t)
                d[t] = tuple(buf[k][tt].numpy() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "loss_weight"))
            cache[(B, HW)] = d
        return cache[(B, HW)]

    return get


def guarded(B, HW, dtype=torch.float32):
    """A (B, HW) device view between two guard rows."""
    buf = torch.full((B + 2, HW), GUARD, dtype=dtype, device="cuda")
    return buf, buf[1:B + 1]


def q_sample(hip, x0, a, s, noise=None, seeds=None, draw=0, want_noise=False):
    B, HW = x0.shape
    xb, x_t = guarded(B, HW)
    nb, n_out = guarded(B, HW) if want_noise else (None, None)
    sd = None if seeds is None else D(np.array(seeds, dtype=np.uint64).view(np.int64))
    keep = (D(x0), D(a), D(s), None if noise is None else D(noise))
    hip._lib.check(hip.lib.prg_q_sample(hip._lib.ptr(keep[0]), hip._lib.ptr(keep[1]), hip._lib.ptr(keep[2]), hip._lib.ptr(keep[3]),
                                        hip._lib.ptr(sd), draw, B, HW, hip._lib.ptr(x_t), hip._lib.ptr(n_out), None), "prg_q_sample")
    torch.cuda.synchronize()
    outs = []
    for b_ in (xb, nb):
        if b_ is not None:
            h = b_.cpu().numpy()
            assert np.all(h[0] == GUARD) and np.all(h[-1] == GUARD), "prg_q_sample wrote outside its rows"
            outs.append(h[1:B + 1].copy())
    return outs if want_noise else outs[0]


def loss(hip, u, x0, a, s, w, objective, loss_type, noise=None, seeds=None, draw=0):
    B, HW = x0.shape
    n = hip.lib.prg_validate_workspace_bytes(B, HW)
    assert n == B * (-(-HW // 4096)) * 24
    ws = torch.full((n // 8 + 2,), GUARD, dtype=torch.float64, device="cuda")
    ob, out = guarded(B, 2, torch.float64)
    sd = None if seeds is None else D(np.array(seeds, dtype=np.uint64).view(np.int64))
    keep = (D(u), D(x0), None if noise is None else D(noise), D(a), D(s), D(w))
    hip._lib.check(hip.lib.prg_diffusion_loss(hip._lib.ptr(keep[0]), hip._lib.ptr(keep[1]), hip._lib.ptr(keep[2]), hip._lib.ptr(sd), draw,
                                              hip._lib.ptr(keep[3]), hip._lib.ptr(keep[4]), hip._lib.ptr(keep[5]), objective, loss_type,
                                              B, HW, C.c_void_p(ws.data_ptr()), n, hip._lib.ptr(out), None), "prg_diffusion_loss")
    torch.cuda.synchronize()
    h = ob.cpu().numpy()
    assert np.all(h[0] == GUARD) and np.all(h[-1] == GUARD) and np.all(ws[n // 8:].cpu().numpy() == GUARD)
    return h[1:B + 1].copy()


def metrics(hip, prob, inp, lab, mask, thr, tol=V.LABEL_TOL):
    B, HW = prob.shape
    n = hip.lib.prg_validate_workspace_bytes(B, HW)
    ws = torch.full((n // 8 + 2,), GUARD, dtype=torch.float64, device="cuda")
    cb, counts = guarded(B, 4, torch.int64)
    sb, sums = guarded(B, 2, torch.float64)
    keep = (D(prob), D(inp), D(lab), None if mask is None else D(mask))
    hip._lib.check(hip.lib.prg_mask_metrics(hip._lib.ptr(keep[0]), hip._lib.ptr(keep[1]), hip._lib.ptr(keep[2]), hip._lib.ptr(keep[3]),
                                            thr, tol, B, HW, C.c_void_p(ws.data_ptr()), n, hip._lib.ptr(counts), hip._lib.ptr(sums), None),
                   "prg_mask_metrics")
    torch.cuda.synchronize()
    c, s = cb.cpu().numpy(), sb.cpu().numpy()
    assert np.all(c[0] == 7) and np.all(c[-1] == 7) and np.all(s[0] == GUARD) and np.all(s[-1] == GUARD)
    assert np.all(ws[n // 8:].cpu().numpy() == GUARD)
    return c[1:B + 1].copy(), s[1:B + 1].copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone against the specifications, stored noise
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW", SHAPES)
def test_q_sample_and_loss_are_the_specifications_bits(hip, data, B, HW):
    d = data(B, HW)
    for t in (0, T - 1):
        a, s, w = d[t]
        x_t, n_out = q_sample(hip, d["x0"], a, s, noise=d["noise"], want_noise=True)
        assert same_bits(x_t, V.q_sample_spec(d["x0"], a, s, d["noise"])) and same_bits(n_out, d["noise"]), (t, "q_sample")
        for objective in (0, 1, 2):
            for lt in (0, 1):
                got = loss(hip, d["u"], d["x0"], a, s, w, objective, lt, noise=d["noise"])
                ref = V.diffusion_loss_spec(d["u"], d["x0"], d["noise"], a, s, w, objective, lt)
                assert same_bits(got, ref), (t, objective, lt, got, ref)


@pytest.mark.parametrize("B,HW", SHAPES)
def test_mask_metrics_are_the_specifications_bits(hip, data, B, HW):
    rng = np.random.default_rng(77 * B + HW)
    inp = rng.random((B, HW), dtype=np.float32)
    lab = (inp + (rng.random((B, HW), dtype=np.float32) - np.float32(0.5)) * np.float32(0.02)).astype(np.float32)
    prob = rng.random((B, HW), dtype=np.float32)
    mask = (rng.random((B, HW), dtype=np.float32) > 0.4).astype(np.float32)
    for thr in (0.5, 0.99):
        for m in (mask, None):
            c, s = metrics(hip, prob, inp, lab, m, thr)
            rc, rs = V.mask_metrics_spec(prob, inp, lab, m, thr)
            assert np.array_equal(c, rc) and same_bits(s, rs), (thr, m is None)
            assert (c.sum(axis=1) == HW).all()


# ------------------------------------------------------------------------------------------------------------------
# 2. Philox noise
# ------------------------------------------------------------------------------------------------------------------
def test_philox_noise(hip, data):
    B, HW = 3, 4100
    d = data(B, HW)
    a, s, w = d[T - 1]
    x_t, n1 = q_sample(hip, d["x0"], a, s, seeds=SEEDS, draw=1, want_noise=True)
    x_t2, n2 = q_sample(hip, d["x0"], a, s, seeds=SEEDS, draw=1, want_noise=True)
    assert same_bits(n1, n2) and same_bits(x_t, x_t2) and np.isfinite(n1).all()
    assert same_bits(x_t, V.q_sample_spec(d["x0"], a, s, n1))                    # the arithmetic is the stored-noise path's
    for b in range(B):                                                             # sample b alone = sample b in the batch of 3
        xb, nb = q_sample(hip, d["x0"][b:b + 1], a[b:b + 1], s[b:b + 1], seeds=SEEDS[b:b + 1], draw=1, want_noise=True)
        assert same_bits(nb[0], n1[b]) and same_bits(xb[0], x_t[b])
    _x, other = q_sample(hip, d["x0"], a, s, seeds=SEEDS, draw=2, want_noise=True)
    assert not np.array_equal(other, n1)
    # not the sampler's stream: its draw 1 of the same keys (x' = 0 x0 + 1 n through the transition kernel)
    row = hip._lib.StepC(0, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    z, sd = torch.zeros((B, HW), device="cuda"), D(np.array(SEEDS, dtype=np.uint64).view(np.int64))
    hip._lib.check(hip.lib.prg_debug_sampler_step(hip._lib.ptr(z), hip._lib.ptr(torch.zeros_like(z)), None, hip._lib.ptr(sd), C.byref(row),
                                                  B, HW, 1, None, None), "prg_debug_sampler_step")
    smp = z.cpu().numpy()
    assert np.isfinite(smp).all() and smp.std() > 0.9 and (smp != n1).mean() > 0.999
    # the host statement of the same draws (numpy's logf / sincosf: a few ulp, not bits)
    host = V.philox_normals(SEEDS, 1, HW)
    assert float(np.abs(host - n1).max()) <= 1e-5
    # the loss kernel regenerates what q_sample drew
    for objective in (0, 1, 2):
        for lt in (0, 1):
            assert same_bits(loss(hip, d["u"], d["x0"], a, s, w, objective, lt, seeds=SEEDS, draw=1),
                             loss(hip, d["u"], d["x0"], a, s, w, objective, lt, noise=n1)), (objective, lt)
    N = n1.size
    mean, var = float(n1.astype(np.float64).mean()), float(n1.astype(np.float64).var())
    print(f"Philox normals, N = {N}: mean {mean:+.4f} (bound {5 / np.sqrt(N):.4f}), variance {var:.4f} (bound {5 * np.sqrt(2 / N):.4f})")
    assert abs(mean) <= 5 / np.sqrt(N) and abs(var - 1) <= 5 * np.sqrt(2 / N)


# ------------------------------------------------------------------------------------------------------------------
# 3. NaN and threshold rules
# ------------------------------------------------------------------------------------------------------------------
def test_nan_stays_in_its_sample(hip, data):
    B, HW = 3, 4100
    d = data(B, HW)
    a, s, w = d[T - 1]
    clean = loss(hip, d["u"], d["x0"], a, s, w, 2, 1, noise=d["noise"])
    bad = d["u"].copy()
    bad[1, 4097] = np.nan
    got = loss(hip, bad, d["x0"], a, s, w, 2, 1, noise=d["noise"])
    assert np.isnan(got[1]).all() and same_bits(got[[0, 2]], clean[[0, 2]])
    rng = np.random.default_rng(5)
    inp, lab, prob = (rng.random((B, HW), dtype=np.float32) for _ in range(3))
    c0, s0 = metrics(hip, prob, inp, lab, None, 0.5)
    prob2 = prob.copy()
    was = prob2[1, 10] > 0.5
    prob2[1, 10] = np.nan                                       # a NaN probability is "not output": finite sums, one count moves
    prob2[1, 11] = np.float32(0.5)                              # exactly at the threshold: false
    c1, s1 = metrics(hip, prob2, inp, lab, None, 0.5)
    rc, rs = V.mask_metrics_spec(prob2, inp, lab, None, 0.5)
    assert np.array_equal(c1, rc) and same_bits(s1, rs) and np.isfinite(s1).all()
    assert np.array_equal(c1[[0, 2]], c0[[0, 2]]) and same_bits(s1[[0, 2]], s0[[0, 2]])
    assert c1[1, 1] + c1[1, 3] == c0[1, 1] + c0[1, 3] - int(was) - int(prob[1, 11] > 0.5)
    inp2 = inp.copy()
    inp2[1, 20] = np.nan                                        # a NaN depth: that row's sums are NaN, the others keep their bits
    prob2[1, 20] = 1.0
    c2, s2 = metrics(hip, prob2, inp2, lab, None, 0.5)
    assert np.isnan(s2[1]).all() and same_bits(s2[[0, 2]], s0[[0, 2]])


# ------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(hip, golden):
    made = {}

    def get(dtype):
        if dtype not in made:
            net = hip.Unet(16, dtype=dtype).load_state_dict(W.synth_state_dict(W.unet_config(16), 9))
            made[dtype] = net.set_time_freqs(golden("G0_host_tables")["freqs_dim16"])
        return made[dtype]

    yield get
    for net in made.values():
        net.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("objective,lt", [("pred_x0", "l1"), ("pred_v", "l2")])
def test_p_losses_is_the_specification_on_the_networks_output(hip, golden, nets, dtype, objective, lt):
    g = golden("G25_validation")
    net = nets(dtype)
    d = hip.GaussianDiffusion(net, image_size=32, objective=objective, beta_schedule="sigmoid", loss_type=lt)
    x0, t, pc, nz = D(g["net_x0"]), torch.from_numpy(g["net_t"]), D(g["net_pc"]), D(g["net_noise"])
    a, s, w = (getattr(d, k)[t].numpy() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "loss_weight"))
    # stored noise
    tab = d.p_losses(x0, t, pc, noise=nz, per_sample=True)
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (2, 2)
    x_t = d.q_sample(x0, t, noise=nz)
    assert same_bits(x_t.cpu().numpy(), V.q_sample_spec(g["net_x0"], a, s, g["net_noise"]))
    u = net(x_t, t.cuda(), pc).cpu().numpy()
    ref = V.diffusion_loss_spec(u, g["net_x0"], g["net_noise"], a, s, w, objective, lt)
    assert same_bits(tab.cpu().numpy(), ref)
    assert float(d.p_losses(x0, t, pc, noise=nz)) == float(ref[:, 1].mean())
    # Philox noise: never stored by p_losses; the same numbers from the normals q_sample reports
    seeds = SEEDS[:2]
    tab2 = d.p_losses(x0, t, pc, seeds=seeds, draw=3, per_sample=True).cpu().numpy()
    x_t2, n2 = V.q_sample_hip(x0, D(a), D(s), seeds=seeds, draw=3, want_noise=True)
    u2 = net(x_t2, t.cuda(), pc).cpu().numpy()
    assert same_bits(tab2, V.diffusion_loss_spec(u2, g["net_x0"], n2.cpu().numpy(), a, s, w, objective, lt))
    if dtype == "fp32" and (objective, lt) == ("pred_x0", "l1"):
        for ref32 in (g["net_unweighted"], g["net_unweighted_1thread"]):
            e = np.abs(tab.cpu().numpy()[:, 0] - ref32.astype(np.float64))
            print(f"fp32 l1 unweighted loss {tab.cpu().numpy()[:, 0]} reference {ref32} |difference| {e}")
            assert (e <= FP32_TOL + (1024 - 1 + 3) * U24 * np.abs(ref32)).all()
    d.close()


def test_sample_keeps_its_bits_around_a_p_losses_call(hip, golden, nets):
    g24, g = golden("G24_objectives"), golden("G25_validation")
    net = nets("fp32")
    kw = dict(param_cond=D(g24["pc"]), img_cond=D(g24["cond"]), seeds=SEEDS[:2], use_graph=True)
    before = hip.GaussianDiffusion(net, image_size=32, timesteps=1000, sampling_timesteps=5)
    first = before.sample(**kw).cpu().numpy()
    loss1 = before.p_losses(D(g["net_x0"]), torch.from_numpy(g["net_t"]), D(g["net_pc"]), seeds=SEEDS[:2], per_sample=True).cpu().numpy()
    again = before.sample(**kw).cpu().numpy()                    # the handle (and its captured graph) from before the call
    after = hip.GaussianDiffusion(net, image_size=32, timesteps=1000, sampling_timesteps=5)
    fresh = after.sample(**kw).cpu().numpy()                     # a handle created after it
    loss2 = after.p_losses(D(g["net_x0"]), torch.from_numpy(g["net_t"]), D(g["net_pc"]), seeds=SEEDS[:2], per_sample=True).cpu().numpy()
    assert np.isfinite(first).all() and same_bits(first, again) and same_bits(first, fresh) and same_bits(loss1, loss2)
    before.close()
    after.close()
