"""Static check of conv3x3_c64_kernel's consumer tile loop from the gfx950 assembly (no GPU needed).

usage: python tools/c64_isa_stats.py [file.s]
Without an argument it compiles pointreggpt_amd/csrc/conv_c64.hip with the Makefile's device flags into a temporary .s.
Per instantiation: MFMAs of the tile loop (must be 144), VALU instructions, global stores and LDS reads BETWEEN its first and last
MFMA (what runs in MFMA shadows), how many instructions after the last MFMA the workgroup barrier comes, and the register / spill /
scratch figures of the kernel descriptor."""
import bisect
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORES = ("global_store", "buffer_store", "flat_store")


def assembly():
    if len(sys.argv) > 1:
        return open(sys.argv[1]).read()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "conv_c64.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "conv_c64.hip", "-o", out],
                       cwd=os.path.join(ROOT, "pointreggpt_amd", "csrc"), check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


txt = assembly()
for m in re.finditer(r"^(_ZN3prg\S*conv3x3_c64_kernel\S*):[^\n]*\n(.*?)\n\.Lfunc_end", txt, re.S | re.M):
    name, body = m.group(1), m.group(2)
    lines, labels = [], []
    for l in body.split("\n"):
        l = l.strip()
        if re.match(r"^\.LBB\S*:", l):
            labels.append(len(lines))
        elif l and not l.startswith((";", ".")):
            lines.append(l)
    blocks = {}
    for i, l in enumerate(lines):
        if l.startswith("v_mfma"):
            blocks.setdefault(bisect.bisect_right(labels, i), []).append(i)
    pro, o16 = re.search(r"ILi(\d)ELb(\d)", name).groups()
    for b, g in blocks.items():
        seg = lines[g[0]:g[-1] + 1]
        rest = lines[g[-1] + 1:]
        bar = next(k for k, l in enumerate(rest) if l.startswith("s_barrier"))
        print(f"<{pro},{'true' if o16 == '1' else 'false'}>: {len(g)} MFMAs | between first and last MFMA: "
              f"{sum(1 for l in seg if l.startswith('v_') and not l.startswith('v_mfma'))} VALU, {sum(1 for l in seg if l.startswith(STORES))} stores, "
              f"{sum(1 for l in seg if l.startswith('ds_read'))} ds_read | s_barrier {bar} instructions after the last MFMA")
for m in re.finditer(r"\.name:\s+(\S*conv3x3_c64_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                     r"\s+\.vgpr_spill_count:\s+(\d+)", txt):
    pro, o16 = re.search(r"ILi(\d)ELb(\d)", m.group(1)).groups()
    print(f"<{pro},{'true' if o16 == '1' else 'false'}>: .vgpr_count {m.group(3)}  .vgpr_spill_count {m.group(4)}  .private_segment_fixed_size {m.group(2)}")
