#!/usr/bin/env python
"""Golden operator schemas (TEST INFRASTRUCTURE): the schema of every operator the reference's TORCH_LIBRARY(gsplat) block
declares (gsplat/cuda/ext.cpp), read from its m.def(...) string literals and stored as tests/golden/reference_schemas.json
(operator name -> schema text) for tests/test_composite_ops.py::test_schemas_are_the_references.
Run only where the reference checkout exists:  python oracle/pin_schemas_against_reference.py --ref <reference checkout>"""
import argparse
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_schemas(ref: str) -> dict:
    with open(os.path.join(ref, "gsplat", "cuda", "ext.cpp")) as f:
        src = f.read()
    out = {}
    for m in re.finditer(r"m\.def\(\s*((?:\"[^\"]*\"\s*)+)\)", src):
        text = "".join(re.findall(r"\"([^\"]*)\"", m.group(1)))
        out[text.split("(", 1)[0].strip()] = text
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "reference_schemas.json"))
    args = ap.parse_args()
    schemas = reference_schemas(args.ref)
    assert schemas, "no m.def(...) found"
    with open(args.out, "w") as f:
        json.dump(schemas, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(schemas)} schemas -> {args.out}")
