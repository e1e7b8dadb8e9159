#!/bin/bash
# Register / spill report of the kernel translation units (host-side compile only):
#   tools/regs.sh [k_ingest_nv1 k_merge_nw1 ...]
# per kernel VGPRs, VGPR and SGPR spills, scratch bytes per lane, occupancy (waves per SIMD) and LDS bytes.
# Instruction mix of their kernels, from the same compile with -S:
#   tools/regs.sh --mix [k_ingest_pack ...]
# per kernel the instruction count, the counts by class (v_*, s_*, ds_*, global_*) and of the
# instructions that tell spill traffic, hazard padding, integer multiplies and selects.  For
# k_ingest_pack the same for Section A (first barrier to the next: route, slice, pack, rank) and
# Section B (from the last barrier of the block-wide vote that follows, i.e. the barriers closer
# than 24 instructions to their predecessor, to the next barrier: range statistics, run claims,
# first part of the scan).
cd "$(dirname "$0")/../flink_amd/csrc"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -DFW_DIAG=0"
if [ "$1" = "--mix" ]; then
  shift
  units=${@:-"k_ingest_pack k_ingest_pack_g1"}
  for f in $units; do
    /opt/rocm/bin/hipcc $FLAGS --cuda-device-only -S -o /tmp/_mix_$f.s $f.hip 2>/dev/null || exit 1
    python3 - /tmp/_mix_$f.s <<'EOF'
import re, subprocess, sys
WATCH = ["v_readlane_b32", "v_writelane_b32", "s_nop", "v_mul_lo_u32", "v_cndmask_b32"]
kernels, cur = [], None
for line in open(sys.argv[1]):
    m = re.match(r"^(_Z\w+):", line)
    if m:
        cur = [m.group(1), []]
        continue
    if cur is None:
        continue
    m = re.match(r"^\s+([a-z][a-z0-9_]+)\b", line)
    if m:
        cur[1].append(m.group(1))
        if m.group(1) == "s_endpgm" and cur not in kernels:
            kernels.append(cur)
    if ".end_amdhsa_kernel" in line:
        cur = None
names = subprocess.run(["c++filt"], input="\n".join(k[0] for k in kernels), capture_output=True, text=True).stdout.split("\n")
def row(label, ins):
    cls = {p: sum(1 for i in ins if i.startswith(p)) for p in ("v_", "s_", "ds_", "global_")}
    print("  %-10s total %5d | v %5d s %5d ds %4d global %4d | " % (label, len(ins), cls["v_"], cls["s_"], cls["ds_"], cls["global_"]) +
          " ".join("%s %d" % (w.replace("_b32", "").replace("_u32", ""), sum(1 for i in ins if i.startswith(w))) for w in WATCH))
for (sym, ins), n in zip(kernels, names):
    print(re.sub(r"fw::|\(fw::\w+\)|void ", "", n))
    row("kernel", ins)
    if "k_ingest_pack" not in sym:
        continue
    b = [i for i, x in enumerate(ins) if x == "s_barrier"]
    if len(b) < 3:
        continue
    k = 1
    while k + 1 < len(b) - 1 and b[k + 1] - b[k] < 24:
        k += 1
    a, bb = ins[b[0] + 1:b[1]], ins[b[k] + 1:b[k + 1]]
    row("section A", a)
    row("section B", bb)
    print("  A + B      total %5d" % (len(a) + len(bb)))
EOF
  done
  exit 0
fi
units=${@:-"k_ingest_nv0 k_ingest_nv1 k_ingest_nv2 k_ingest_pack k_ingest_pack_g1 k_merge_nw1 k_merge_nw2 k_merge_nw4"}
for f in $units; do
  /opt/rocm/bin/hipcc $FLAGS -c -o /tmp/_regs_$f.o $f.hip \
      -Rpass-analysis=kernel-resource-usage 2>&1 |
    python3 -c '
import re, sys, subprocess
cur = None; rows = []
for line in sys.stdin:
    m = re.search(r"Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}; rows.append(cur); continue
    m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
    if m and cur is not None: cur[m.group(1)] = int(m.group(2))
names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.split("\n")
for r, n in zip(rows, names):
    n = re.sub(r"fw::|\(fw::\w+\)|void ", "", n)
    g = lambda k: r.get(k, 0)
    print("%-70s vgpr %4d vspill %4d sspill %4d scratch %d occ %d lds %d" % (n, g("VGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]"), g("LDS Size [bytes/block]")))
'
  done
