#!/usr/bin/env python
"""CPU only: the share of Gaussians of the c3 scene (bench.make_workload) whose gradient is exactly zero in every leaf after one
step of the oracle pipeline, loss = render_colors.sum() as bench.py takes it. These are the rows the per-Gaussian backward
kernels (csrc/sh.hip, csrc/projection.hip) skip; DESIGN.md section 4 derives the bytes of the two stages from this figure.

At the benchmark's own size the counts are compared with the figures DESIGN.md quotes; a mismatch is an error (exit status 1).

    python tools/dead_row_share.py [--gaussians 1000000]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.pipeline import rasterization_cpu  # noqa: E402


# c3 (1 000 000 Gaussians): what DESIGN.md section 4 and profiles/r12_dead_rows.md quote
EXPECTED_C3 = {"n_isects": 3802742, "zero_in_every_leaf": 894648, "zero_colour_rows": 894651, "groups_of_64": 15625,
               "groups_of_64_wholly_dead": 13}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    args = ap.parse_args()
    O.set_threads(min(os.cpu_count() or 1, 32))
    sc, W, H = bench.make_workload(args.gaussians, "cpu")
    ref = rasterization_cpu(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["colors"], sc["viewmats"], sc["Ks"], W, H,
                            sh_degree=3)
    N = args.gaussians
    zero = {k: (g.reshape(N, -1) == 0).all(1) for k, g in ref["grads"].items()}
    dead = torch.stack(list(zero.values())).all(0)
    pad = (-N) % 64
    groups = torch.cat([dead, torch.ones(pad, dtype=torch.bool)]).reshape(-1, 64).all(1)
    out = {"gaussians": N, "n_isects": ref["n_isects"], "n_visible": ref["n_visible"],
           "zero_in_every_leaf": int(dead.sum()), "dead_share": round(float(dead.float().mean()), 6),
           "zero_colour_rows": int(zero["colors"].sum()), "zero_rows_per_leaf": {k: int(v.sum()) for k, v in zero.items()},
           "groups_of_64": int(groups.numel()), "groups_of_64_wholly_dead": int(groups.sum())}
    print(json.dumps(out))
    if N == 1_000_000:
        wrong = {k: (out[k], v) for k, v in EXPECTED_C3.items() if out[k] != v}
        if wrong:
            sys.exit(f"dead_row_share: c3 figures moved (got, expected): {wrong}")


if __name__ == "__main__":
    main()
