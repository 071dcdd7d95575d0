#!/usr/bin/env python3
"""Compile every unit of the library for gfx950 with the product flags (lft_amd/_lib.py) and print per-kernel register / spill /
occupancy / static LDS figures (extra arguments go to hipcc)."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lft_amd import _lib
cmds = _lib.unit_commands("/opt/rocm/bin/hipcc", "device", lambda unit: "/dev/null", ["-c", "-Rpass-analysis=kernel-resource-usage"] + sys.argv[1:])
procs = [subprocess.Popen(c, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for c in cmds.values()]
out = "".join(p.communicate()[1] for p in procs)
cur = None
rows = {}
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1); rows[cur] = {}
    for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "LDS Size [bytes/block]"):
        m = re.search(re.escape(key) + r": (\d+)", line)
        if m and cur: rows[cur][key] = int(m.group(1))
print(f"{'kernel':58s} VGPR AGPR spill scratch occ    lds")
for k, r in rows.items():
    if "k_" not in k: continue
    name = k[:56]
    print(f"{name:58s} {r.get('VGPRs',0):4d} {r.get('AGPRs',0):4d} {r.get('VGPRs Spill',0):5d} {r.get('ScratchSize [bytes/lane]',0):7d} {r.get('Occupancy [waves/SIMD]',0):3d} {r.get('LDS Size [bytes/block]',0):6d}")
