#!/usr/bin/env python
"""Times the fused deformation network (csrc/deformation.hip) against its torch composition, which is what a user without the
kernels would run, and writes profiles/deformation.json.

Per size (N Gaussians; 64 plane features, width 64, three hidden layers, heads drawn uniform in +-0.125): `--windows`
alternating windows of fused and `deform_torch`, forward and forward + backward, each window the median of `--iters` calls
between device events after a warm-up. Recorded: the times, the ratio torch / fused per window (the fused form has to win every
window), the achieved fp32 matrix rate against the 155 TFLOP/s figure and the bytes the kernels must move against the time,
both computed from the shapes:
  forward   2 (3 * 64 * 64 + 8 * 64) FLOP; 256 B features + 32 B (means, quats, opacities) in + 32 B out per row
  backward  the forward again + 2 * 6 * 64 * 64 + 2 * 2 * 8 * 64 FLOP; 256 B features + 32 B cotangents + 256 B v_plane_features
Also the error figures of the fused gradients against a float64 composition at the first size.

`--kernels-only` makes a few fused calls and nothing else, for a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/deformation_bench.py --kernels-only`.

usage: python tools/deformation_bench.py [--iters 10] [--windows 5] [--out profiles/deformation.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsplat_amd import deformation as df  # noqa: E402

SIZES = (200_000, 1_000_000, 2_800_000)
DEV = "cuda"


def module(seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    m = df.DeformNetwork(64)
    with torch.no_grad():
        for head in (m.pos_head, m.quat_head, m.opacity_head):
            for p in head.parameters():
                p.uniform_(-0.125, 0.125)
    return m.to(DEV).to(dtype)


def inputs(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    leaves = [torch.randn(N, d, generator=g).to(DEV).requires_grad_(True) for d in (3, 4, 1)]
    leaves.append((torch.randn(N, 64, generator=g) * 0.5).to(DEV).requires_grad_(True))
    weights = [torch.randn(N, d, generator=g).to(DEV) for d in (3, 4, 1)]
    return leaves, weights


def loss(outs, weights):
    return sum((o * w).sum() for o, w in zip(outs, weights))


def timed(fn, iters):
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "deformation.json"))
    p.add_argument("--kernels-only", action="store_true")
    args = p.parse_args()
    if args.kernels_only:
        m = module()
        leaves, weights = inputs(SIZES[1])
        for _ in range(5):
            loss(df.deform(m, *leaves), weights).backward()
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "windows": args.windows, "sizes": []}
    for N in SIZES:
        m = module()
        leaves, weights = inputs(N)

        def fwd(fn):
            with torch.no_grad():
                fn(m, *leaves)

        def both(fn):
            for t in leaves:
                t.grad = None
            m.zero_grad(set_to_none=True)
            loss(fn(m, *leaves), weights).backward()

        rows = {"fused_fwd": [], "torch_fwd": [], "fused_fwd_bwd": [], "torch_fwd_bwd": []}
        for _ in range(args.windows):
            rows["fused_fwd"].append(timed(lambda: fwd(df.deform), args.iters))
            rows["torch_fwd"].append(timed(lambda: fwd(df.deform_torch), args.iters))
            rows["fused_fwd_bwd"].append(timed(lambda: both(df.deform), args.iters))
            rows["torch_fwd_bwd"].append(timed(lambda: both(df.deform_torch), args.iters))
        flop_f = 2 * (3 * 64 * 64 + 8 * 64) * N
        flop_b = flop_f + (2 * 6 * 64 * 64 + 2 * 2 * 8 * 64) * N
        bytes_f, bytes_b = 320 * N, 544 * N
        tf, tb = min(rows["fused_fwd"]), min(rows["fused_fwd_bwd"])
        entry = {"N": N, "ms": rows,
                 "ratio_fwd": [t / u for t, u in zip(rows["torch_fwd"], rows["fused_fwd"])],
                 "ratio_fwd_bwd": [t / u for t, u in zip(rows["torch_fwd_bwd"], rows["fused_fwd_bwd"])],
                 "fused_wins_every_window": all(t > u for t, u in zip(rows["torch_fwd"], rows["fused_fwd"]))
                 and all(t > u for t, u in zip(rows["torch_fwd_bwd"], rows["fused_fwd_bwd"])),
                 "fwd_tflops": flop_f / tf / 1e9, "fwd_share_of_155_tflops": flop_f / tf / 1e9 / 155.0,
                 "fwd_bwd_tflops": (flop_f + flop_b) / tb / 1e9, "fwd_gb_per_s": bytes_f / tf / 1e6,
                 "fwd_bwd_gb_per_s": (bytes_f + bytes_b) / tb / 1e6}
        result["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
        del m, leaves, weights
        torch.cuda.empty_cache()
    # error of the fused gradients against float64, next to the float32 composition's own
    N = SIZES[0]
    leaves, weights = inputs(N, seed=1)
    errs = {}
    for tag, fn, dt in (("f64", df.deform_torch, torch.float64), ("f32", df.deform_torch, torch.float32), ("fused", df.deform, torch.float32)):
        mm = module(seed=1, dtype=dt)
        ll = [t.detach().to(dt).requires_grad_(True) for t in leaves]
        outs = fn(mm, *ll)
        loss(outs, [w.to(dt) for w in weights]).backward()
        errs[tag] = {"means_new": outs[0].detach().double(), "quats_new": outs[1].detach().double(),
                     "opacities_new": outs[2].detach().double(), "v_plane_features": ll[3].grad.double(),
                     **{"v_" + k: q.grad.double() for k, q in mm.named_parameters()}}
    result["error_vs_float64"] = {"N": N, "note": "near-kink rows not dropped here: the summed gradients include them",
                                  "fused": {k: float((errs["fused"][k] - errs["f64"][k]).abs().max()) for k in errs["f64"]},
                                  "float32_composition": {k: float((errs["f32"][k] - errs["f64"][k]).abs().max()) for k in errs["f64"]},
                                  "max_abs": {k: float(errs["f64"][k].abs().max()) for k in errs["f64"]}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    lost = [e["N"] for e in result["sizes"] if not e["fused_wins_every_window"]]
    if lost:
        raise SystemExit(f"the fused form lost a window to the torch composition at N = {lost}")


if __name__ == "__main__":
    main()
