#!/usr/bin/env python
"""Writes the compiler's resource report of csrc/plas.hip (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, the unit's own
flags; no GPU needed) as JSON for tools/plas_bench.py --kernel-resources: per kernel VGPRs, AGPRs, SGPRs, scratch, waves per
SIMD and static LDS (none of the kernels uses dynamic LDS).

usage: python tools/plas_resources.py OUT.json"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-ffp-contract=off"]
FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes",
          "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_static_bytes"}


def main():
    src = os.path.join(ROOT, "gsplat_amd", "csrc", "plas.hip")
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c",
                              src, "-o", os.path.join(tmp, "plas.o")], capture_output=True, text=True, check=True).stderr
    out, cur = {"flags": " ".join(FLAGS)}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: _ZN3gsx\d+(\w+?_kernel)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:.*?\s{2,}([A-Z][A-Za-z ]*(?: \[[^\]]*\])?): (\d+) \[", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
