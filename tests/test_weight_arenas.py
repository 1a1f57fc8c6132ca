"""Everything a U-Net handle holds, pinned byte for byte without a GPU: prg_debug_weight_arena (include/prg.h) returns each arena
that prg_unet_create would upload, and the layout's offsets; their sha256 must equal tests/golden/weight_arenas.json, which was
recorded from the build that only MOVED the packers into csrc/weights_host.cpp (before any of them was rewritten).

Inputs: synth_state_dict (counter-based Philox: the same floats on every host); the fixture stores the digest of each flat input
and a mismatch there FAILS.  Cases: dim 16 in all four modes; dim 64 in bf16 and f16x3 only (packing 36 M parameters as MX-fp8 or
as plain float32 adds seconds and no packer that dim 16 and the per-conv tests of test_weight_layouts.py do not run); under the
default switches and under each setting that changes an arena: sub-pixel split packings on, fused attention off, static shifts
off, split stem off.

    python tests/test_weight_arenas.py --record      rewrites the fixture from the library that is built (a deliberate act)
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pointreggpt_amd import _lib, weights as W   # noqa: E402
from pointreggpt_amd.unet import _cfg_c, flatten_state_dict   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "weight_arenas.json")
ARENAS = ("layout", "packed", "mx", "mx_scale", "h16", "split", "split_scale", "stem", "stem_frag", "stem_split", "stem_split_scale",
          "freqs", "attn_split", "pq_static", "cond_entries", "attn", "kshift")          # PRG_ARENA_* in order
DTYPES = {"fp32": 0, "bf16": 1, "mxfp8": 2, "f16x3": 3}
UP2X2, FUSED, KSHIFT, STEM = 1, 2, 4, 8                                                  # PRG_WOPT_*
DEFAULT = FUSED | KSHIFT | STEM
# (name, bits, the modes whose arenas the setting can change)
OPTIONS = (("default", DEFAULT, tuple(DTYPES)), ("split_up2x2", DEFAULT | UP2X2, ("f16x3",)),
           ("no_fused_attn", DEFAULT & ~FUSED, ("bf16", "mxfp8")), ("no_kshift", DEFAULT & ~KSHIFT, ("bf16", "mxfp8")),
           ("no_split_stem", DEFAULT & ~STEM, ("f16x3",)))
NETS = (("unet", 64, 20), ("maskunet", 64, 21), ("unet", 16, 20), ("maskunet", 16, 21))   # (kind, dim, seed)
CASES = [(kind, dim, seed, mode, oname, bits) for kind, dim, seed in NETS for mode in DTYPES if dim == 16 or mode in ("bf16", "f16x3")
         for oname, bits, modes in OPTIONS if mode in modes]

_flat = {}


def flat_input(kind, dim, seed):
    if (kind, dim) not in _flat:
        cfg = W.unet_config(dim) if kind == "unet" else W.maskunet_config(dim)
        _flat[(kind, dim)] = (cfg, flatten_state_dict(cfg, W.synth_state_dict(cfg, seed)))
    return _flat[(kind, dim)]


def arena_bytes(lib, cfg, flat, dtype, bits, arena):
    cc, n = _cfg_c(cfg), C.c_int64(0)
    args = (C.byref(cc), flat.ctypes.data_as(C.c_void_p), flat.size, dtype, bits, arena)
    buf = np.empty(8 * flat.nbytes + (1 << 20), np.uint8)     # (no arena set is 8 times its input; untouched pages cost nothing)
    _lib.check(lib.prg_debug_weight_arena(*args, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)), "prg_debug_weight_arena")
    return buf[:n.value].tobytes()


def digests(case):
    kind, dim, seed, mode, _, bits = case
    cfg, flat = flat_input(kind, dim, seed)
    blob, out, pos = arena_bytes(_lib.load(), cfg, flat, DTYPES[mode], bits, -1), {}, 0       # PRG_ARENA_ALL: one build per case
    for name in ARENAS:
        n = int(np.frombuffer(blob, np.int64, 1, pos)[0])
        out[name] = hashlib.sha256(blob[pos + 8:pos + 8 + n]).hexdigest()
        pos += 8 + n
    assert pos == len(blob)
    return out


def case_id(case):
    kind, dim, _, mode, oname, _ = case
    return f"{kind}{dim}-{mode}-{oname}"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_exactly_the_cases(golden):
    assert sorted(golden["arenas"]) == sorted(case_id(c) for c in CASES)
    assert sorted(golden["inputs"]) == sorted(f"{k}{d}" for k, d, _ in NETS)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_arenas_and_layout_match_the_recorded_digests(case, golden):
    kind, dim, seed = case[:3]
    _, flat = flat_input(kind, dim, seed)
    assert hashlib.sha256(flat.tobytes()).hexdigest() == golden["inputs"][f"{kind}{dim}"], "the synthetic state dict itself changed"
    got, want = digests(case), golden["arenas"][case_id(case)]
    assert got == want, sorted(k for k in ARENAS if got[k] != want.get(k))


def test_every_setting_changes_an_arena(golden):
    """Each non-default setting is in the list because it moves at least one arena of its mode at dim 64 (dim 16 has no shape that
    the sub-pixel, fused-attention or MFMA-stem packings cover: there the settings must change nothing, which the digests pin too)."""
    for kind, dim, _, mode, oname, _ in CASES:
        if oname != "default" and dim == 64:
            assert golden["arenas"][f"{kind}{dim}-{mode}-{oname}"] != golden["arenas"][f"{kind}{dim}-{mode}-default"], (kind, dim, mode, oname)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    out = {"inputs": {f"{k}{d}": hashlib.sha256(flat_input(k, d, s)[1].tobytes()).hexdigest() for k, d, s in NETS},
           "arenas": {case_id(c): digests(c) for c in CASES}}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases to {GOLDEN}")
