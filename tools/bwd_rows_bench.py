#!/usr/bin/env python
"""Times the two per-Gaussian backward kernels alone (gsx_sh_bwd, gsx_project_ewa_bwd_opac) on the c3 scene, HIP events around
each call, with the cotangents as columns of [R, 9] gradient rows of which a given share is zero - the rows of Gaussians that
compositing never reached. --dead 0 is the all-live control (dense random cotangents, no dead row): a row-granular liveness
test must cost it nothing. Select the library under test with GSPLAT_AMD_LIB, one process per library.

    python tools/bwd_rows_bench.py --dead 0 --dead 0.895"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import gsplat_amd  # noqa: E402
from gsplat_amd import _cabi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--dead", type=float, action="append", help="share of rows with all-zero cotangents (repeatable)")
    ap.add_argument("--reps", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sc, W, H = bench.make_workload(args.gaussians, dev)
    N, K = sc["colors"].shape[:2]
    radii, _, _, conics, _ = gsplat_amd.fully_fused_projection(sc["means"], None, sc["quats"], sc["scales"], sc["viewmats"],
                                                                sc["Ks"], W, H, opacities=sc["opacities"])
    radii, conics = radii.contiguous(), conics.contiguous()
    post = torch.clamp_min(gsplat_amd.spherical_harmonics(3, sc["means"], sc["viewmats"], sc["colors"]) + 0.5, 0.0).contiguous()
    g = torch.Generator().manual_seed(1)
    out = {"library": os.path.basename(_cabi.lib_path()), "gaussians": N, "reps": args.reps}
    p, ps = _cabi.ptr, _cabi.ptr_strided
    v_coeffs, v_means_sh = torch.empty_like(sc["colors"]), torch.empty_like(sc["means"])
    v_means, v_quats, v_scales = torch.empty_like(sc["means"]), torch.empty_like(sc["quats"]), torch.empty_like(sc["scales"])
    v_opac = torch.empty_like(sc["opacities"])
    for dead in args.dead or [0.0]:
        rows = torch.randn(N, 9, generator=g)
        rows[:, 2:5] *= 1e-2
        rows[torch.rand(N, generator=g) < dead] = 0.0
        rows = rows.to(dev)

        def sh():
            _cabi.call("gsx_sh_bwd", 3, p(sc["means"]), p(sc["viewmats"]), p(sc["colors"]), None, None, None, None, 1, 1, N, -1, 1,
                       K, 3, p(radii), p(post), ps(rows[:, 5:8]), 9, None, p(v_coeffs), p(v_means_sh), None)

        def proj():
            _cabi.call("gsx_project_ewa_bwd_opac", p(sc["means"]), None, p(sc["quats"]), p(sc["scales"]), p(sc["viewmats"]),
                       p(sc["Ks"]), 1, 1, N, W, H, 0.3, 0, p(radii), p(conics), None, ps(rows[:, 0:2]), 9, None, ps(rows[:, 2:5]),
                       9, None, ps(rows[:, 8]), 9, p(v_means), None, p(v_quats), p(v_scales), None, p(v_opac))

        for _ in range(10):
            sh(), proj()
        torch.cuda.synchronize()
        _cabi.profile_begin()
        for _ in range(args.reps):
            sh(), proj()
        rec = _cabi.profile_end()
        for name, ms in rec.items():
            us = sorted(1e3 * t for t in ms)
            out[f"{name} dead={dead}"] = {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
