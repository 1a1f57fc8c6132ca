"""The independent Philox oracle (oracle/philox.py) against the published known-answer vectors, and the CPU twin's seeded
path against that oracle.  No GPU needed: this proves the harness tests/test_gpu_sampler_step.py then holds the device to.

Bound on a normal (derived, not observed): float32 log, sqrt, sin and cos of the C library and of the device are documented
to <= 1 ulp; with the two float32 roundings of -2 * log and r * cos that is about 4 ulp of the Box-Muller radius r; the bound is
twice that: |n - n_ref| <= 8 * 2^-23 * r_ref.  Through the output map (x + 1) / 2 (one more float32 rounding, of x + 1; the halving
is exact) the same statement reads: out lies between the images of the two ends of that interval, because the map is monotone."""
import numpy as np
import pytest
import torch

from oracle import philox as PH
from pointreggpt_amd import cpu

SEEDS = [0, 1, 2 ** 32, 0x123456789ABCDEF0, 2 ** 64 - 1]
ULP = 2.0 ** -23
NORMAL_BOUND_ULP = 8.0


def identity_chain(G, net, S):
    """A GaussianDiffusion whose single transition returns its input: the output is (start image + 1) / 2."""
    d = G(net, image_size=S, timesteps=1000, sampling_timesteps=1)
    rows = d.step_table()[:1]
    rows[0].update(c_x0=0.0, c_x=1.0, c_eps=0.0, sigma=0.0)
    d.step_table = lambda: rows
    return d


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox4x32_10_known_answers(counter, key, expect):
    """The Random123 known-answer vectors of Philox4x32-10 (kat_vectors: zeros, all ones, digits of pi)."""
    out = PH.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
    assert tuple(int(w[0]) for w in out) == expect, [hex(int(w[0])) for w in out]
    # and the vectors do tell the generator's parts apart: nine rounds, or a key whose high word is dropped, miss them
    assert tuple(int(w[0]) for w in PH.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key, rounds=9)) != expect
    if key[1]:
        assert tuple(int(w[0]) for w in PH.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], (key[0], 0))) != expect


def test_oracle_normals_shape_and_contract():
    """normals(): four pixels per counter, |n| <= r, draws and keys all give different fields, the high key word included."""
    n, r = PH.normals(SEEDS[3], 2, 1024)
    assert n.shape == r.shape == (1024,) and n.dtype == np.float64
    assert np.all(np.abs(n) <= r) and np.array_equal(r[0::4], r[1::4]) and np.array_equal(r[2::4], r[3::4])
    assert np.allclose(n[0::4] ** 2 + n[1::4] ** 2, r[0::4] ** 2, rtol=1e-12, atol=0)
    fields = [PH.normals(s, d, 1024)[0] for s in SEEDS for d in (0, 1)]
    for i in range(len(fields)):
        for j in range(i):
            assert not np.array_equal(fields[i], fields[j]), (i, j)
    # a prefix of a longer draw is the shorter draw: pixel 4q+i depends on (key, draw, q, i) only
    assert np.array_equal(PH.normals(SEEDS[3], 2, 64)[0], n[:64])
    big = np.concatenate([PH.normals(s, 0, 16384)[0] for s in SEEDS])
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02


def test_cpu_twin_start_image_against_the_oracle():
    """prg_cpu_sampler_run with seeds, through the identity transition: the output is ((draw 0 of seeds[b]) + 1) / 2 within
    the bound above, for seeds that differ in the low word only, the high word only, and both."""
    S = 32
    net = cpu.Unet(8).init_synthetic(1)
    d = identity_chain(cpu.GaussianDiffusion, net, S)
    pc = torch.tensor([[37.9, 38.0, 16.25, 16.0]]).repeat(len(SEEDS), 1)
    out = d.sample(param_cond=pc, seeds=SEEDS).numpy().reshape(len(SEEDS), -1)
    worst = 0.0
    for b, s in enumerate(SEEDS):
        n, r = PH.normals(s, 0, S * S)
        lo, hi = PH.start_image_interval(n, r, NORMAL_BOUND_ULP)
        nz = r > 0
        worst = max(worst, float(np.max(np.abs(out[b].astype(np.float64) * 2 - 1 - n)[nz] / (ULP * r[nz]))))
        assert np.all((out[b] >= lo) & (out[b] <= hi)), (hex(s), int(np.sum((out[b] < lo) | (out[b] > hi))))
        # the neighbouring draw and the key without its high word are O(1) away: the check can tell them apart
        assert np.max(np.abs(out[b] * 2 - 1 - PH.normals(s, 1, S * S)[0])) > 1.0
        if s >> 32:
            assert np.max(np.abs(out[b] * 2 - 1 - PH.normals(s & 0xFFFFFFFF, 0, S * S)[0])) > 1.0
    print(f"CPU twin start image vs oracle: max |2 out - 1 - n_ref| = {worst:.2f} ulp of r (includes the rounding of x + 1)")


def test_cpu_twin_keeps_nan_visible():
    """A one-row ancestral chain (t = 0: clamp after the DDNM replacement) from a start image that holds a NaN: the network
    output is NaN, the known pixels return the condition exactly and every in-painted pixel stays NaN (clamp propagates it)."""
    S = 32
    net = cpu.Unet(8).init_synthetic(1)
    d = cpu.GaussianDiffusion(net, image_size=S, timesteps=1000)
    rows = [d.step_table()[-1]]
    assert rows[0]["t"] == 0 and rows[0]["clip_pred"] == 2
    d.step_table = lambda: rows
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1, 1, 1, S, S), generator=g)
    x[0, 0, 0, 5, 7] = float("nan")
    cond = torch.cat([torch.rand((1, 1, S, S), generator=g) * 2 - 1, (torch.rand((1, 1, S, S), generator=g) > 0.5).float() * 2 - 1], 1)
    out = d.sample(param_cond=torch.tensor([[37.9, 38.0, 16.25, 16.0]]), img_cond=cond, noise=x).numpy()
    known = (cond[:, 1:2].numpy() + 1) * 0.5 > 0.5
    c1 = float(np.float32(rows[0]["c_x0"]))
    assert c1 == 1.0 and rows[0]["c_x"] == 0.0               # posterior mean at t = 0 is x0 itself
    assert np.array_equal(out[known], ((cond[:, 0:1].numpy() + np.float32(1)) * np.float32(0.5))[known])
    assert known.any() and (~known).any() and np.isnan(out[~known]).all()
