"""Which kernel runs every convolution, pinned without a GPU: prg_debug_conv_choice (include/prg.h) answers with the library's own
selection function (csrc/conv_choose.cpp) for a descriptor, the options of the launch, a CU count and the PRG_* switches, and this
test compares every answer with tests/golden/conv_dispatch.json.  The file was recorded (python tests/test_conv_dispatch.py
--record) from the build that moved each launcher's conditions word for word into conv_choose.cpp
(profiles/conv_dispatch_refactor_ab.txt has its checksums); a later form of the selection has to give the same table.
Re-recorded once since, for one rule: tile_fuse asks that the group width divide the channel tile (bn % cpg == 0), so the cout192 /
cout384 queries of edges() (groups of 24 / 48 channels) no longer fuse their statistics; the nine edge walks' digests moved, no other.

The queries are derived here: walk() restates which convolutions UnetImpl::forward (csrc/unet.hip) launches and with which
options, as far as the selection reads them; conv2's options depend on what conv1's choice reports (acc_done), as in the forward
pass.  The golden file holds a digest of every distinct walk's answers in walk order, per case (in cases() order) the index of its
walk, and how many answers chose each family: --show CASE prints a case's current answers in full."""
import ctypes as C
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from pointreggpt_amd import _lib  # noqa: E402
from pointreggpt_amd.weights import maskunet_config, unet_config  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json")
DTYPES = {"fp32": _lib.PRG_F32, "bf16": _lib.PRG_BF16, "mxfp8": _lib.PRG_MXFP8, "f16x3": _lib.PRG_F16X3}
SWITCHES = ("PRG_CONV_WS", "PRG_CONV_C64", "PRG_CONV_W256", "PRG_CONV_DOWN_W256", "PRG_CONV_W256MX", "PRG_W256_MIN_TILES", "PRG_UP2X2",
            "PRG_H16", "PRG_MX_PURE", "PRG_SPLIT_UP2X2", "PRG_SPLIT_P64", "PRG_SPLIT_W512")
DEFAULTS = dict(zip(SWITCHES, (1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 256, 1)))
Q = ("dtype", "B", "Hin", "Win", "C0", "C1", "ups", "KH", "KW", "stride", "pad", "Hout", "Wout", "Cout", "CoutPad", "kchunks", "present",
     "gn_groups", "fold_G", "fold_cpg", "in_f16", "out_f16", "mx_pure", "num_cus")
CC = ("family", "th", "tw", "bm", "bn", "pro", "mode", "tiles_x", "tiles_y", "tiles_n", "grid", "fuse_stats", "nsplit", "acc_done",
      "fill_tables", "is_mx", "supports_prologue", "h16_pair")
CP = dict(bias=1, residual=2, res_a=4, pro_a=8, gn_partials=16, gn_acc=32, mx=64, s2d=128, up=256, split=512, up_split=1024, f16=2048,
          res_fold_acc=4096, fold_acc=8192, fold_pq=16384)
FAMILY = ("none", "igemm", "halo", "mx_halo", "c64", "ws", "w256", "w256mx", "split_halo", "split_ws", "split_p64", "split_w512",
          "split_igemm")
HIDDEN = 128


def header_enum(prefix):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prg.h")).read(), flags=re.S)
    return re.findall(rf"\b{prefix}_(\w+)\b", hdr)


def conv(dtype, B, Hin, Win, C0, Cout, K=3, C1=0, stride=1, pad=None, ups=0, **present):
    """One query (without num_cus and switches): the descriptor as UnetImpl::make_desc builds it, and the present pointers."""
    bf16 = dtype in ("bf16", "mxfp8")
    pad = (1 if K > 1 else 0) if pad is None else pad
    Hl, Wl = (2 * Hin, 2 * Win) if ups else (Hin, Win)
    q = dict(dtype=DTYPES[dtype], B=B, Hin=Hin, Win=Win, C0=C0, C1=C1, ups=ups, KH=K, KW=K, stride=stride, pad=pad,
             Hout=(Hl + 2 * pad - K) // stride + 1, Wout=(Wl + 2 * pad - K) // stride + 1, Cout=Cout, CoutPad=(Cout + 63) // 64 * 64,
             kchunks=-(-(C0 + C1) // (32 if bf16 else 16)), gn_groups=8, fold_G=0, fold_cpg=0, in_f16=0, out_f16=0, mx_pure=0)
    for k in ("gn_groups", "fold_G", "fold_cpg", "in_f16", "out_f16", "mx_pure"):
        if k in present:
            q[k] = present.pop(k)
    q["present"] = sum(CP[k] for k, v in present.items() if v)
    return q


def packings(dtype, Cin, Cout, K, conv2=False, upsample=False, split_up2x2=False):
    """The optional packings a handle of `dtype` holds for a conv (csrc/weights_host.h: *_eligible; weights_host.cpp: pack_conv_host)."""
    bf16 = dtype in ("bf16", "mxfp8")
    return dict(mx=dtype == "mxfp8" and K == 3 and Cin % 64 == 0 and Cout % 64 == 0,
                s2d=bf16 and K == 4 and Cin % 64 == 0 and Cout % 64 == 0,
                f16=bf16 and conv2 and K == 3 and Cin == Cout and Cin % 64 == 0,
                up=bf16 and upsample and K == 3 and Cin % 64 == 0 and (Cout == 64 or Cout % 128 == 0),
                split=dtype == "f16x3",
                up_split=dtype == "f16x3" and upsample and split_up2x2 and K == 3 and Cin % 32 == 0 and Cout % 128 == 0)


class Hook:
    def __init__(self, num_cus, switches):
        self.lib = _lib.load()
        self.tail = [num_cus] + [dict(DEFAULTS, **switches)[k] for k in SWITCHES]
        self.out = (C.c_int32 * len(CC))()
        self.scale = C.c_float()

    def array(self, q):
        return (C.c_int32 * (len(Q) + len(SWITCHES)))(*([q[k] for k in Q[:-1]] + self.tail))

    def __call__(self, q, q2=None):
        """the answer as a tuple: the PRG_CC_* ints and exec_scale (as a ratio of small integers: 1 or 4 / 9)"""
        rc = self.lib.prg_debug_conv_choice(self.array(q), self.array(q2) if q2 else None, self.out, C.byref(self.scale))
        _lib.check(rc, "prg_debug_conv_choice")
        return tuple(self.out) + (round(self.scale.value * 9),)


def walk(cfg, dtype, B, S, ask, split_up2x2=False):
    """Every launch_conv of one forward pass, in order; ask(name, query, query2=None) -> the answer (dict by CC name)."""
    acc = dtype in ("bf16", "mxfp8")          # fixed-point statistics are offered (PRG_GN_ACC default)
    G = cfg.groups
    dims = cfg.dims
    nl = len(dims) - 1

    def resblock(name, c0, c1, cout, H):
        stats = dict(bias=1, gn_partials=1, gn_acc=acc)
        q1 = conv(dtype, B, H, H, c0, cout, C1=c1, **stats, **packings(dtype, c0 + c1, cout, 3))
        q2 = conv(dtype, B, H, H, cout, cout, **stats, **packings(dtype, cout, cout, 3, conv2=True))
        fuse_pro = ask(name + ".c2?", q2)["supports_prologue"]
        fold = dict(fold_acc=1, fold_pq=1, pro_a=1, fold_G=G, fold_cpg=cout // G)
        h16 = 0
        if acc and fuse_pro and q2["present"] & CP["f16"]:
            p2 = conv(dtype, B, H, H, cout, cout, **stats, **fold, **packings(dtype, cout, cout, 3, conv2=True))
            h16 = ask(name + ".h16", q1, p2)["h16_pair"]
        r1 = ask(name + ".c1", dict(q1, out_f16=h16))
        if fuse_pro:
            pro = fold if r1["acc_done"] else dict(pro_a=1)
            q2 = conv(dtype, B, H, H, cout, cout, in_f16=h16, **stats, **pro, **packings(dtype, cout, cout, 3, conv2=True))
        r2 = ask(name + ".c2", q2)
        if c0 + c1 != cout:
            # the res_conv: alone (Tail::Plain), and with the block's tail in its epilogue (Tail::ResEpilogue)
            pk = packings(dtype, c0 + c1, cout, 1)
            ask(name + ".res", conv(dtype, B, H, H, c0, cout, K=1, C1=c1, bias=1, **pk))
            if dtype != "fp32" and cout % 8 == 0:
                tail = dict(res_fold_acc=1) if r2["acc_done"] and (cout // G) % 8 == 0 else dict(res_a=1)
                ask(name + ".res+tail", conv(dtype, B, H, H, c0, cout, K=1, C1=c1, bias=1, residual=1, **tail, **pk))

    def attention(name, c, H, linear):
        ask(name + ".qkv", conv(dtype, B, H, H, c, 3 * HIDDEN, K=1, **packings(dtype, c, 3 * HIDDEN, 1)))
        ask(name + ".out", conv(dtype, B, H, H, HIDDEN, c, K=1, bias=1, residual=not linear, **packings(dtype, HIDDEN, c, 1)))

    H = S
    for i in range(nl):
        c, co = dims[i], dims[i + 1]
        resblock(f"down{i}.r0", c, 0, c, H)
        resblock(f"down{i}.r1", c, 0, c, H)
        attention(f"down{i}.attn", c, H, True)
        if i < nl - 1:
            ask(f"down{i}.resample", conv(dtype, B, H, H, c, co, K=4, stride=2, pad=1, bias=1, **packings(dtype, c, co, 4)))
            H //= 2
        else:
            ask(f"down{i}.resample", conv(dtype, B, H, H, c, co, bias=1, **packings(dtype, c, co, 3)))
    c = dims[-1]
    resblock("mid1", c, 0, c, H)
    attention("mid.attn", c, H, False)
    resblock("mid2", c, 0, c, H)
    for i in range(nl):
        ci, co = dims[nl - 1 - i], dims[nl - i]
        resblock(f"up{i}.r0", co, ci, co, H)
        resblock(f"up{i}.r1", co, ci, co, H)
        attention(f"up{i}.attn", co, H, True)
        strided = i < nl - 1
        ask(f"up{i}.resample", conv(dtype, B, H, H, co, ci, ups=int(strided), bias=1,
                                    **packings(dtype, co, ci, 3, upsample=strided, split_up2x2=split_up2x2)))
        if strided:
            H *= 2
    resblock("final", dims[0], dims[0], dims[0], H)


def edges(ask):
    """The conditions the predicates exist for, one query each (bf16 unless said)."""
    st = dict(bias=1, gn_partials=1, gn_acc=1)
    for cout in (192, 384):                               # tiles_n = 3, cpg = 24 / 48: not a power of two
        for dt in ("bf16", "f16x3", "fp32"):
            ask(f"cout{cout}.{dt}", conv(dt, 2, 64, 64, cout, cout, **dict(st, gn_acc=dt == "bf16"), **packings(dt, cout, cout, 3)))
    for H, W in ((24, 24), (40, 24), (12, 32), (20, 32), (8, 48), (16, 16), (8, 16), (4, 32)):   # W % 16, H % 8 with W % 32 == 0, ...
        for cout in (64, 128):
            for dt in ("bf16", "mxfp8", "f16x3", "fp32"):
                ask(f"{H}x{W}.{cout}.{dt}", conv(dt, 16, H, W, 128, cout, **dict(st, gn_acc=dt in ("bf16", "mxfp8")), **packings(dt, 128, cout, 3)))
    for B in (2, 64):
        ask(f"up64.B{B}", conv("bf16", B, 32, 32, 64, 64, ups=1, bias=1, up=1))                  # a 64 -> 64 Upsample
        ask(f"up64.mx.B{B}", conv("mxfp8", B, 32, 32, 64, 64, ups=1, bias=1, up=1, mx=1))
        ask(f"up128.stats.B{B}", conv("bf16", B, 32, 32, 128, 128, ups=1, up=1, **st))          # statistics keep it on the nine taps
        ask(f"two_sources_pro.B{B}", conv("bf16", B, 64, 64, 64, 128, C1=64, bias=1, pro_a=1))   # C1 > 0 with pro_a
        for cin, cout in ((64, 64), (128, 128), (256, 128)):
            ask(f"residual.{cin}.{cout}.B{B}", conv("bf16", B, 64, 64, cin, cout, bias=1, residual=1))
            ask(f"no_bias.{cin}.{cout}.B{B}", conv("bf16", B, 64, 64, cin, cout))
            ask(f"slabs_only.{cin}.{cout}.B{B}", conv("bf16", B, 64, 64, cin, cout, bias=1, gn_partials=1))
            ask(f"slabs_or_acc.{cin}.{cout}.B{B}", conv("bf16", B, 64, 64, cin, cout, **st))
            # pro_fold whose 8-channel units straddle groups (cpg = 4), and one that folds in the kernel
            for g in (cin // 4, 8):
                ask(f"fold.g{g}.{cin}.{cout}.B{B}", conv("bf16", B, 64, 64, cin, cout, bias=1, pro_a=1, fold_acc=1, fold_pq=1, fold_G=g, fold_cpg=cin // g))
            ask(f"fold_no_pq.{cin}.{cout}.B{B}", conv("bf16", B, 64, 64, cin, cout, bias=1, pro_a=1, fold_acc=1, fold_G=8, fold_cpg=cin // 8))
            ask(f"mx_pure.{cin}.{cout}.B{B}", conv("mxfp8", B, 64, 64, cin, cout, mx=1, mx_pure=1, **st))
            ask(f"in_f16_alone.{cin}.{cout}.B{B}", conv("bf16", B, 64, 64, cin, cout, in_f16=1, bias=1, pro_a=1))
    # the 2 GiB limit of the c64 kernel's 32-bit input offsets: B = 256 at 256 x 256 is the first launch beyond it
    for B, H in ((255, 256), (256, 256), (257, 256), (256, 248), (256, 264)):
        ask(f"c64_2gib.B{B}.H{H}", conv("bf16", B, H, 256, 64, 64, **st))
    # kGnMaxSplit: 256 x 256 is the last size whose slabs fit (8 groups: 512 slabs; 1 group, cpg = 64: 1024); 512 x 512 does not
    for H in (256, 512):
        for g in (8, 2, 1):
            for cout in (64, 128):
                ask(f"slabs.H{H}.g{g}.{cout}", conv("bf16", 4, H, H, cout, cout, gn_groups=g, **st))
                ask(f"slabs.H{H}.g{g}.{cout}.f16x3", conv("f16x3", 4, H, H, cout, cout, gn_groups=g, bias=1, gn_partials=1, split=1))


NETS = {"unet": unet_config, "maskunet": maskunet_config}
ONE_SWITCH = ([{k: 0} for k in SWITCHES[:5]] + [{"PRG_UP2X2": 0}, {"PRG_H16": 0}, {"PRG_MX_PURE": 1}, {"PRG_W256_MIN_TILES": 1},
              {"PRG_SPLIT_UP2X2": 1}, {"PRG_SPLIT_P64": 0}, {"PRG_SPLIT_P64": 1}, {"PRG_SPLIT_W512": 0}, {"PRG_SPLIT_W512": 2},
              {"PRG_CONV_WS": 0, "PRG_CONV_C64": 0, "PRG_CONV_W256": 0, "PRG_CONV_DOWN_W256": 0}])   # the last: tools/lib_outputs.py


def cases():
    """(name, num_cus, switches, function(ask))"""
    for net, cfg in NETS.items():
        for dt in DTYPES:
            for S in (32, 40, 64, 128, 256):
                for B in (1, 2, 8, 16, 64):
                    for cus in (256, 64, 8, 7, 0):
                        yield (f"{net}64_S{S}_B{B}_{dt}_cus{cus}", cus, {}, lambda ask, c=cfg(), dt=dt, B=B, S=S: walk(c, dt, B, S, ask))
            for sw in ONE_SWITCH:
                tag = "".join(f"+{k}={v}" for k, v in sorted(sw.items()))
                for S in (64, 128):
                    for B in (2, 16):
                        yield (f"{net}64_S{S}_B{B}_{dt}_cus256{tag}", 256, sw,
                               lambda ask, c=cfg(), dt=dt, B=B, S=S, up=sw.get("PRG_SPLIT_UP2X2", 0): walk(c, dt, B, S, ask, split_up2x2=bool(up)))
    for dt in DTYPES:
        yield (f"unet16_S32_B3_{dt}_cus256", 256, {}, lambda ask, dt=dt: walk(unet_config(dim=16), dt, 3, 32, ask))
    for cus in (256, 64, 8, 7, 0):
        yield (f"edges_cus{cus}", cus, {}, edges)
    for sw in ({"PRG_W256_MIN_TILES": 1}, {"PRG_MX_PURE": 1}, {"PRG_SPLIT_W512": 2}, {"PRG_SPLIT_P64": 1}):
        yield ("edges_cus256" + "".join(f"+{k}={v}" for k, v in sw.items()), 256, sw, edges)


def answers():
    """{case: [(conv name, answer tuple), ...]}, the sha256 of every query asked (so that a changed walk is told from a changed answer),
    and {(case, conv name): query}"""
    res, sha, queries = {}, hashlib.sha256(), {}
    for name, cus, sw, fn in cases():
        hook, got = Hook(cus, sw), []

        def ask(conv_name, q, q2=None):
            sha.update(bytes(hook.array(q)) + (bytes(hook.array(q2)) if q2 else b""))
            a = hook(q, q2)
            got.append((conv_name, a))
            queries[(name, conv_name)] = q
            return dict(zip(CC, a))
        fn(ask)
        res[name] = got
    return res, sha.hexdigest(), queries


def digest(got):
    """sha256 of a case's answers in walk order, first 16 hex digits"""
    return hashlib.sha256(repr([a for _, a in got]).encode()).hexdigest()[:16]


def table(res):
    """the golden document of {case: answers}: the digest of every distinct walk, per case (in cases() order) the index of its walk,
    and how many answers chose each family"""
    walks, order, chosen = {}, [], [0] * len(FAMILY)
    for got in res.values():
        order.append(walks.setdefault(digest(got), len(walks)))
        for _, a in got:
            chosen[a[0]] += 1
    return {"columns": list(CC) + ["exec_scale_ninths"], "families": list(FAMILY), "chosen": chosen, "walks": list(walks), "cases": order}


def record():
    res, sha, _ = answers()
    doc = dict(table(res), queries_sha256=sha, answers=sum(len(g) for g in res.values()))
    with open(GOLDEN, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('","', '",\n"'))
        f.write("\n")
    print(f"{GOLDEN}: {len(res)} cases, {doc['answers']} queries, {len(doc['walks'])} distinct walks")


def compare(res, golden):
    """the cases whose answers differ from the recorded ones"""
    assert len(res) == len(golden["cases"]), (len(res), len(golden["cases"]))
    return [name for (name, got), w in zip(res.items(), golden["cases"]) if digest(got) != golden["walks"][w]]


_cache = {}


def recorded_and_current():
    if not _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
        _cache["res"], _cache["sha"], _cache["queries"] = answers()
    return _cache["golden"], _cache["res"], _cache["sha"], _cache["queries"]


def test_header_enums_are_the_tested_ones():
    assert header_enum("PRG_CQ")[:len(Q)] == [q.upper() for q in Q] and header_enum("PRG_CQ")[len(Q):] == ["SWITCHES", "COUNT", "SWITCHES"]
    assert header_enum("PRG_CC") == [c.upper() for c in CC] + ["COUNT"]
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    for k, v in CP.items():
        assert re.search(rf"PRG_CP_{k.upper()} = {v}\b", hdr), k
    # the selection's switches, their order in the query and their defaults: the one function that reads them (conv.hip)
    src = open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "conv.hip")).read()
    assert re.findall(r"env_int\(\"(PRG_\w+)\", (\d+)\)", src) == [(k, str(DEFAULTS[k])) for k in SWITCHES]
    choose = open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "conv_choose.h")).read()
    assert re.findall(r"= (\d+);\s+// (PRG_\w+)", choose) == [(str(DEFAULTS[k]), k) for k in SWITCHES]
    assert [f.lower() for f in re.findall(r"^  kConv(\w+)", choose, flags=re.M)] == [f.replace("_", "") for f in FAMILY]


def test_every_choice_matches_the_recorded_table():
    """On a mismatch: `python tests/test_conv_dispatch.py --show CASE` prints the case's current answers, conv by conv."""
    golden, res, sha, _ = recorded_and_current()
    assert golden["columns"] == list(CC) + ["exec_scale_ninths"] and golden["families"] == list(FAMILY)
    assert sha == golden["queries_sha256"], "the queries changed (walk(), edges() or cases()): the table no longer belongs to them"
    bad = compare(res, golden)
    assert not bad, (len(bad), bad[:5])
    assert golden["chosen"] == table(res)["chosen"] and all(golden["chosen"])   # every family is chosen somewhere, "none" included


def test_the_table_notices_planted_mistakes():
    """Two mistakes a later edit could make, applied to the answers in the queries where they would show: the comparison with the
    recorded table has to report exactly the cases that hold such a query.
      1. c64 without its `grid < 8` rule: with 7 CUs (grid = 7 & ~7 = 0) the 64 -> 64 convs would stay on conv3x3_c64_kernel.
      2. w256 asked before up_w256: a wide Upsample conv would run the nine-tap form (mode 0) instead of the sub-pixel one."""
    golden, res, _, queries = recorded_and_current()
    assert not compare(res, golden)
    fam, mode, grid = CC.index("family"), CC.index("mode"), CC.index("grid")

    def plant(change):
        """the answers with change(case, position, conv name, answer) -> new answer or None applied; and the cases it touched"""
        out, touched = {}, set()
        for name, got in res.items():
            new = [change(name, k, cn, a) for k, (cn, a) in enumerate(got)]
            out[name] = [(cn, a if n is None else n) for (cn, a), n in zip(got, new)]
            if any(n is not None for n in new):
                touched.add(name)
        return out, touched

    # 1: the answers of the cus7 cases whose cus8 twin (the same walk but for the CU count) runs c64
    def no_grid_rule(name, k, cn, a):
        if "_cus7" not in name or name.startswith("edges"):
            return None
        t = res[name.replace("_cus7", "_cus8")][k][1]
        return (t[fam],) + a[1:] if FAMILY[t[fam]] == "c64" and FAMILY[a[fam]] != "c64" else None
    r1, touched1 = plant(no_grid_rule)
    assert touched1 and set(compare(r1, golden)) == touched1

    # 2: every sub-pixel Upsample launch (default switches) that the 3x3 entry covers too: Cout % 128 == 0 and at least `grid`
    # 256-pixel x 128-channel tiles of the OUTPUT image
    def w256_first(name, k, cn, a):
        if "+" in name or name.startswith("edges") or FAMILY[a[fam]] != "w256" or a[mode] != 2:
            return None
        q = queries[(name, cn)]
        tiles = q["Hout"] * q["Wout"] // 256 * (q["Cout"] // 128) * q["B"]
        return a[:mode] + (0,) + a[mode + 1:] if q["Cout"] % 128 == 0 and tiles >= a[grid] else None
    r2, touched2 = plant(w256_first)
    assert touched2 and set(compare(r2, golden)) == touched2
    # and the answers hold both sides of the second decision: the same Upsample conv as mode 2 by default, as mode 0 under PRG_UP2X2=0
    up = [dict(res[n])["up1.resample"] for n in ("unet64_S128_B16_bf16_cus256", "unet64_S128_B16_bf16_cus256+PRG_UP2X2=0")]
    assert [(FAMILY[a[fam]], a[mode]) for a in up] == [("w256", 2), ("w256", 0)]


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    elif sys.argv[1:2] == ["--show"] and len(sys.argv) == 3:
        for cn, a in answers()[0][sys.argv[2]]:
            print(f"{cn:22s}", FAMILY[a[0]], dict(zip(CC[1:] + ("exec_scale_ninths",), a[1:])))
    else:
        sys.exit("usage: python tests/test_conv_dispatch.py --record | --show CASE")
