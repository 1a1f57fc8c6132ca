"""The validation path on the host against the reference's own numbers (tests/golden/G25_validation.npz, made by
tools/make_goldens.py g25 from GaussianDiffusion.q_sample / predict_v / p_losses and MaskTrainer.compute_metrics).

Tolerances.  q_sample, the pred_v target and loss_weight: bit for bit.  A loss against the reference's float32 value: the bound
that holds for ANY order of summing N non-negative float32 terms in float32, (N - 1) 2^-24 relative, plus three more roundings
(the division, the weight, the batch mean): (N - 1 + 3) 2^-24 = 6.1e-5 at N = 1024.  Against the float64 recomputation from the
reference's float32 terms: N 2^-52 relative (two float64 sums of the same terms in different orders).  Both are derived; the
measured gap between the reference's float32 loss and its float64 recomputation (1.1e-7) is recorded in the fixture, not used.
Mask metrics: the confusion matrix and FP exact, mIoU / PAcc equal to the same float64 divisions of the reference's matrix (and
to the reference's float32 numbers within float32 rounding), MSE / MAE / SAE within the summation bound at N = 512."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import cpu, validate as V
from pointreggpt_amd.diffusion import GaussianDiffusion, loss_weight, make_schedule

SCHEDULES = ("sigmoid", "cosine", "linear")
OBJECTIVES = ("pred_x0", "pred_noise", "pred_v")
FP32_TOL = 1e-4                 # the project's bound on a float32 network output (tests/_objectives.py, tools/make_goldens.py)
U24, U52 = 2.0 ** -24, 2.0 ** -52


@pytest.fixture(scope="module")
def g(golden):
    return golden("G25_validation")


def coefficients(schedule, t):
    buf = make_schedule(1000, schedule)
    return buf["sqrt_alphas_cumprod"][t].numpy(), buf["sqrt_one_minus_alphas_cumprod"][t].numpy()


def stub_output(x, t, pc):
    """tools/make_goldens.py, g25_stub_output, in numpy float32: one rounded operation per step."""
    f = np.float32
    tf = (t.astype(f) * f(1e-3)).reshape(-1, 1, 1, 1)
    p0 = (pc[:, 0].astype(f) * f(0.01)).reshape(-1, 1, 1, 1)
    return ((x * f(0.75) + tf * f(0.25)) - p0).astype(f)


class StubNet:
    random_or_learned_sinusoidal_cond = False
    channels = out_dim = 1

    def __call__(self, x, t, pc):
        return torch.from_numpy(stub_output(x.numpy(), t.numpy(), pc.numpy()))


def test_q_sample_and_the_v_target_are_the_references_bits(g):
    t = torch.from_numpy(g["t"])
    assert g["t"].tolist() == [0, 500, 999]
    for schedule in SCHEDULES:
        a, s = coefficients(schedule, t)
        assert np.array_equal(V.q_sample_spec(g["x0"], a, s, g["noise"]), g[schedule + "_x_t"]), schedule
        assert np.array_equal(V.predict_v_spec(g["x0"], a, s, g["noise"]), g[schedule + "_v"]), schedule
    assert np.array_equal(stub_output(g["sigmoid_x_t"], g["t"], g["pc"]), g["sigmoid_u"])


def test_loss_weight_is_the_references_float32_array(g):
    for objective in OBJECTIVES:
        for schedule in SCHEDULES:
            for snr in (False, True):
                ref = g[f"{objective}_{schedule}_snr{int(snr)}_loss_weight"]
                w = loss_weight(1000, schedule, objective, snr, 5)
                assert w.dtype == torch.float32 and np.array_equal(w.numpy(), ref), (objective, schedule, snr)
                d = GaussianDiffusion(StubNet(), image_size=32, objective=objective, beta_schedule=schedule, min_snr_loss_weight=snr)
                assert np.array_equal(d.loss_weight.numpy(), ref)
    # the generator's configuration keeps the entry make_schedule always carried
    assert torch.equal(GaussianDiffusion(StubNet(), image_size=32).loss_weight, make_schedule(1000, "sigmoid")["loss_weight"])


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_batch_loss_against_the_reference(g, schedule):
    """cpu.GaussianDiffusion.p_losses (the specifications end to end) on the fixture's stub network and stored noise."""
    N = g["x0"][0].size
    assert N == 1024
    worst32 = worst64 = 0.0
    for objective in OBJECTIVES:
        for snr in (False, True):
            for lt in ("l1", "l2"):
                d = cpu.GaussianDiffusion(StubNet(), image_size=32, objective=objective, beta_schedule=schedule, loss_type=lt,
                                          min_snr_loss_weight=snr)
                got = d.p_losses(torch.from_numpy(g["x0"]), torch.from_numpy(g["t"]), torch.from_numpy(g["pc"]),
                                 noise=torch.from_numpy(g["noise"]))
                assert got.dtype == torch.float64 and got.ndim == 0
                got = float(got)
                key = f"{objective}_{schedule}_snr{int(snr)}_{lt}_loss"
                f64 = float(g[key + "_f64"])
                for ref in (float(g[key]), float(g[key + "_1thread"])):
                    e = abs(got - ref) / abs(ref)
                    worst32 = max(worst32, e)
                    assert e <= (N - 1 + 3) * U24, (key, got, ref, e)
                e = abs(got - f64) / abs(f64)
                worst64 = max(worst64, e)
                assert e <= N * U52, (key, got, f64, e)
                # the table behind the mean: per_sample rows, weighted = unweighted * (double)w
                tab = d.p_losses(torch.from_numpy(g["x0"]), torch.from_numpy(g["t"]), torch.from_numpy(g["pc"]),
                                 noise=torch.from_numpy(g["noise"]), per_sample=True).numpy()
                w = g[f"{objective}_{schedule}_snr{int(snr)}_loss_weight"][g["t"]].astype(np.float64)
                assert tab.shape == (3, 2) and np.array_equal(tab[:, 1], tab[:, 0] * w) and float(tab[:, 1].mean()) == got
    print(f"{schedule}: worst relative gap to the reference's float32 loss {worst32:.2e}, to its float64 recomputation {worst64:.2e}")


def test_cpu_path_on_a_real_network_against_the_references_p_losses(g):
    """prg_cpu_unet_forward between the two specifications, G24's network: the L1 mean is 1-Lipschitz in the network output, so
    the unweighted loss lies within FP32_TOL plus the summation bound of the reference's."""
    from pointreggpt_amd.weights import synth_state_dict, unet_config
    net = cpu.Unet(16).load_state_dict(synth_state_dict(unet_config(16), 9))
    d = cpu.GaussianDiffusion(net, image_size=32, loss_type="l1")
    tab = d.p_losses(torch.from_numpy(g["net_x0"]), torch.from_numpy(g["net_t"]), torch.from_numpy(g["net_pc"]),
                     noise=torch.from_numpy(g["net_noise"]), per_sample=True).numpy()
    N = 1024
    for ref in (g["net_unweighted"], g["net_unweighted_1thread"]):
        e = np.abs(tab[:, 0] - ref.astype(np.float64))
        print("unweighted", tab[:, 0], "reference", ref, "error", e)
        assert (e <= FP32_TOL + (N - 1 + 3) * U24 * np.abs(ref)).all()
    net.close()


def test_ordered_sum_depends_on_the_row_alone():
    rng = np.random.default_rng(7)
    for HW in (1, 4, 36, 1023, 4096, 4100, 9001):
        t = rng.random((3, HW), dtype=np.float32)
        s = V.ordered_sum(t)
        assert all(V.ordered_sum(t[b:b + 1])[0] == s[b] for b in range(3))
        assert np.allclose(s, t.astype(np.float64).sum(axis=1), rtol=HW * U52, atol=0)
        t[1, HW // 2] = np.nan
        s2 = V.ordered_sum(t)
        assert np.isnan(s2[1]) and s2[0] == s[0] and s2[2] == s[2]
    k = np.arange(4100, dtype=np.float32)[None]
    assert V.ordered_sum(k)[0] == 4099 * 4100 / 2                   # integers: exact in any order


def test_nan_stays_in_its_sample():
    rng = np.random.default_rng(8)
    u, x0, n = (rng.standard_normal((3, 36)).astype(np.float32) for _ in range(3))
    a = s = w = np.full(3, 0.5, dtype=np.float32)
    ref = V.diffusion_loss_spec(u, x0, n, a, s, w, "pred_v", "l2")
    u[1, 5] = np.nan
    got = V.diffusion_loss_spec(u, x0, n, a, s, w, "pred_v", "l2")
    assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], ref[[0, 2]])
    with pytest.raises(ValueError):
        V.diffusion_loss_spec(u, x0, n, a, s, w, "pred_eps", "l2")
    with pytest.raises(ValueError):
        V.diffusion_loss_spec(u, x0, n, a, s, w, "pred_v", "huber")


@pytest.mark.parametrize("thr", (0.5, 0.99))
def test_mask_metrics_against_compute_metrics(g, thr):
    tag = f"thr{int(thr * 100)}"
    keys = [str(k) for k in g["mask_keys"]]
    assert keys == list(V.MetricMeter.KEYS)
    meter = V.MetricMeter()
    for name in ("a", "b"):
        sums = V.mask_metrics_spec(g[f"mask_{name}_prob"], g[f"mask_{name}_input"], g[f"mask_{name}_label"], g[f"mask_{name}_mask"], thr)
        # without a stored mask the kernel's rule is the dataset's (dc:941), which made the fixture's mask
        rule = V.mask_metrics_spec(g[f"mask_{name}_prob"], g[f"mask_{name}_input"], g[f"mask_{name}_label"], None, thr)
        assert np.array_equal(sums[0], rule[0]) and np.array_equal(sums[1], rule[1])
        m = V.mask_metrics(sums)
        ref = dict(zip(keys, g[f"mask_{name}_{tag}_values"]))
        matrix = g[f"mask_{name}_{tag}_matrix"]
        check_metrics(m, ref, matrix, N=g[f"mask_{name}_prob"].size)
        meter.update(m)
    avg = dict(zip(keys, g[f"mask_{tag}_avg"]))
    for k in keys:
        assert abs(meter.avg[k] - avg[k]) <= 512 * U24 * abs(avg[k]), k
    assert meter.avg["FP"] == avg["FP"]


def check_metrics(m, ref, matrix, N):
    assert np.array_equal(m["matrix"], matrix) and m["FP"] == ref["FP"] == matrix[0, 1]
    inter = np.diag(matrix).astype(np.float64)
    with np.errstate(invalid="ignore"):
        iou = inter / ((matrix.sum(1) + matrix.sum(0)).astype(np.float64) - inter)
    assert m["mIoU"] == float(np.nanmean(iou)) and m["PAcc"] == float(inter.sum() / matrix.sum())
    assert abs(m["mIoU"] - ref["mIoU"]) <= 4 * U24 and abs(m["PAcc"] - ref["PAcc"]) <= 2 * U24   # the reference divides in float32
    for k in ("MSE", "MAE", "SAE"):
        assert abs(m[k] - ref[k]) <= (N - 1 + 3) * U24 * abs(ref[k]), (k, m[k], ref[k])
    return iou


@pytest.mark.parametrize("thr", (0.5, 0.99))
def test_empty_masks_give_one_nan_iou_that_nanmean_skips(g, thr):
    tag = f"thr{int(thr * 100)}"
    sums = V.mask_metrics_spec(g["mask_empty_prob"], g["mask_empty_input"], g["mask_empty_label"], g["mask_empty_mask"], thr)
    m = V.mask_metrics(sums)
    matrix = g[f"mask_empty_{tag}_matrix"]
    assert matrix[0, 0] == g["mask_empty_prob"].size and matrix.sum() == matrix[0, 0]
    iou = check_metrics(m, dict(zip(V.MetricMeter.KEYS, g[f"mask_empty_{tag}_values"])), matrix, N=g["mask_empty_prob"].size)
    assert np.isnan(iou[1]) and iou[0] == 1.0 and m["mIoU"] == 1.0 and m["MSE"] == 0.0


def test_threshold_and_nan_rules():
    f = np.float32
    prob = np.array([[0.5, np.nan, 0.50000006, 0.2]], dtype=f)
    inp = np.array([[0.3, 0.3, 0.3, 0.3]], dtype=f)
    lab = np.array([[0.3, 0.302, 0.4, 0.3049]], dtype=f)
    counts, sums = V.mask_metrics_spec(prob, inp, lab, None, 0.5)
    # pixel 0: at the threshold -> not output, label kept; 1: NaN -> not output; 2: output, label dropped (|d| > tol); 3: label kept (just
    # inside tol), not output
    assert counts.tolist() == [[0, 1, 3, 0]]
    d = np.array([f(0.3), f(0.302), f(0) - f(0.3), f(0.3049)], dtype=f)
    assert sums[0, 0] == V.ordered_sum(np.abs(d)[None])[0] and sums[0, 1] == V.ordered_sum((d * d)[None])[0]


def test_timesteps_is_a_pure_function_of_its_key():
    T = 1000
    scenes = np.arange(50)
    t = V.timesteps(11, scenes, 3, T)
    assert t.dtype == np.int64 and t.min() >= 0 and t.max() < T and len(set(t.tolist())) > 25
    assert np.array_equal(np.concatenate([V.timesteps(11, scenes[:7], 3, T), V.timesteps(11, scenes[7:], 3, T)]), t)
    assert [int(V.timesteps(11, [s], 3, T)[0]) for s in (49, 0, 17)] == [int(t[49]), int(t[0]), int(t[17])]
    assert not np.array_equal(V.timesteps(12, scenes, 3, T), t) and not np.array_equal(V.timesteps(11, scenes, 4, T), t)
    hits = {int(V.timesteps(5, [0], d, 4)[0]) for d in range(64)}
    assert hits == {0, 1, 2, 3}
    assert (V.timesteps(5, scenes, 0, 1) == 0).all()
    with pytest.raises(ValueError):
        V.timesteps(5, scenes, 0, 0)


def test_constructor_and_forward(g):
    with pytest.raises(ValueError):
        GaussianDiffusion(StubNet(), image_size=32, loss_type="huber")
    d = cpu.GaussianDiffusion(StubNet(), image_size=32, loss_type="l2")
    assert d.loss_type == "l2" and d.sqrt_alphas_cumprod.dtype == torch.float32 and d.sqrt_one_minus_alphas_cumprod.shape == (1000,)
    img = torch.from_numpy((g["x0"] + 1) / 2)
    K = torch.zeros((3, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 37.0, 38.0, 16.0, 16.0
    whole = d.forward({"img": img, "intrinsic": K, "scene": [4, 5, 6]}, seed=9, per_sample=True).numpy()
    part = d.forward({"img": img[1:2], "intrinsic": K[1:2], "scene": [5]}, seed=9, per_sample=True).numpy()
    assert np.isfinite(whole).all() and np.array_equal(part[0], whole[1])           # keyed by (seed, scene), not by the batch
    # Philox noise on the host: standard normals under the validation tag, not the sampler's stream
    n = V.philox_normals([1, 2, 3], 0, 4100)
    assert abs(float(n.mean())) <= 5 / np.sqrt(n.size) and abs(float(n.var()) - 1) <= 5 * np.sqrt(2 / n.size)
    assert not np.array_equal(n, V.philox_normals([1, 2, 3], 0, 4100, tag=0x70726721))
    prof = V.loss_profile(d, img, K, timesteps=[0, 999], seeds=[1, 2, 3])
    assert prof.shape == (2, 3, 2) and np.isfinite(prof).all()
