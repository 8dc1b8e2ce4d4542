#!/usr/bin/env python3
"""Register budget of every kernel of pt_kernels.hip as the Makefile builds it: VGPRs, SGPRs, spills, scratch, LDS, occupancy
(from the compiler's own summary comments in the ISA listing).   python3 scripts/kernel_regs.py [name-filter] [-Dmacro ...]"""
import os, re, shutil, subprocess, sys
from kernel_listing import listing
flt = [a for a in sys.argv[1:] if not a.startswith("-")]
extra = [a for a in sys.argv[1:] if a.startswith("-") and a != "--keep"]
src_dir = os.environ.get("PT_SRC_DIR")   # another source tree: its pt_kernels.hip, and its headers ahead of this tree's
txt = listing("pt_kernels.hip", open(os.path.join(src_dir, "pt_kernels.hip")).read() if src_dir else None, (["-I" + src_dir] if src_dir else []) + extra)
if "--keep" in sys.argv: open("/tmp/pt_kernels.s", "w").write(txt)
cur = None; rows = {}
for line in txt.split("\n"):
    m = re.match(r"^(\S+):\s*; @(\S+)", line)
    if m: cur = m.group(2)
    for key in ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy", "LDSByteSize", "VGPRBlocks"):
        m = re.match(r"^; %s: (\d+)" % key, line)
        if m and cur: rows.setdefault(cur, {})[key] = int(m.group(1))
filt = shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
for k, v in rows.items():
    if "Occupancy" not in v: continue
    name = subprocess.run([filt, k], capture_output=True, text=True).stdout.strip() if filt else k
    name = re.sub(r"\(ptamd::KParams.*", "", name).replace("void ptamd::", "")
    if flt and not any(f in name for f in flt): continue
    print("%-60s vgpr %3d agpr %3d sgpr %3d scratch %4d occupancy %d" % (name[:60], v.get("NumVgprs", -1), v.get("NumAgprs", 0), v.get("NumSgprs", -1), v.get("ScratchSize", 0), v["Occupancy"]))
