"""What the compiler made of the Newton loop of the workgroup vertex program, counted in the device assembly:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -Iinclude -Igcs_admm_amd/csrc [the 512-thread defines of build.py] \\
          gcs_admm_amd/csrc/vertex_wg.hip -o wg.s
    python tools/wg_loop_stats.py wg.s [kernel name filter]

Per kernel: registers, spilled scalars and code bytes from its metadata; then, between the header of the Newton loop and its back edge
(the longest backward branch of the kernel that does not go to an exit block): instructions, vector instructions, v_readlane_b32 reloads
from the spill registers (the registers v_writelane_b32 writes), s_nop, 32-bit and 24-bit multiplies, scalar multiplies, conditional
branches.  The table of profiles/wg_scalars/README.md was made with it."""
import re, sys
path = sys.argv[1]; flt = sys.argv[2] if len(sys.argv) > 2 else "vertex_wg"
lines = open(path).read().split("\n")
# kernels: from "name:" to ".Lfunc_end"
starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
meta = {}
cur = None
for l in lines:
    m = re.match(r"\s+\.name:\s+(\S+)", l)
    if m: cur = m.group(1); meta.setdefault(cur, {})
    for k in ("sgpr_spill_count", "vgpr_count", "sgpr_count", "private_segment_fixed_size"):
        m = re.match(r"\s+\.%s:\s+(\d+)" % k, l)
        if m and cur: meta[cur][k] = int(m.group(1))
for (i0, name) in starts:
    if flt not in name: continue
    i1 = next(j for j in range(i0, len(lines)) if lines[j].startswith(".Lfunc_end"))
    body = lines[i0:i1]
    labels = {}
    for j, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m: labels[m.group(1)] = j
    best = (0, 0, 0)
    for j, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < j and j - labels[m.group(1)] > best[0] and not any('s_endpgm' in x for x in body[labels[m.group(1)]:labels[m.group(1)] + 4]):
            best = (j - labels[m.group(1)], labels[m.group(1)], j)
    spillregs = set(re.match(r"\s+v_writelane_b32\s+(v\d+)", l).group(1) for l in body if re.match(r"\s+v_writelane_b32", l))
    loop = body[best[1]:best[2] + 1]
    ins = [l.strip() for l in loop if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    def cnt(pred): return sum(1 for l in ins if pred(l))
    rl = cnt(lambda l: l.startswith("v_readlane_b32") and l.split(",")[1].strip() in spillregs)
    wl_all = sum(1 for l in body if l.strip().startswith("v_writelane_b32"))
    size = None
    for l in lines[i1:i1 + 400]:
        m = re.match(r"; codeLenInByte = (\d+)", l)
        if m: size = int(m.group(1)); break
    print(name[:60], meta.get(name, {}), "code", size, "spillregs", sorted(spillregs), "writelane total", wl_all)
    print("   loop lines", len(loop), "instr", len(ins), "VALU", cnt(lambda l: l.startswith("v_")), "reloads", rl,
          "writelane", cnt(lambda l: l.startswith("v_writelane")), "s_nop", cnt(lambda l: l.startswith("s_nop")),
          "mul_lo_u32", cnt(lambda l: l.startswith("v_mul_lo_u32")), "mul24", cnt(lambda l: "u24" in l or "i24" in l),
          "s_mul", cnt(lambda l: l.startswith("s_mul")), "cbranch", cnt(lambda l: l.startswith("s_cbranch")))
