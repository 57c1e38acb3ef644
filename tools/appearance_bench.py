#!/usr/bin/env python
"""Times the fused appearance MLP (csrc/appearance.hip) against its torch composition, which is what a user without the
kernels would run, and writes profiles/appearance.json.

Per size (N Gaussians, C cameras; embed_dim 16, sh_degree 3): 5 alternating windows of fused and `appearance_torch`, forward
and forward + backward, each window the median of `--iters` calls between device events after a warm-up. Recorded: the times,
the ratio torch / fused per window (the fused form has to win every window), the achieved fp32 matrix rate against the 155
TFLOP/s figure and the bytes the kernels must move against the time, both computed from the shapes:
  forward   2 (48 * 64 + 64 * 64 + 3 * 64) FLOP and 128 B features / C + 12 B dirs + 12 B colours per row
  backward  the forward again + 2 * 4 * 64 * 64 FLOP per row; 128 B features + 128 B v_features per Gaussian, 36 B per row
Also the error figures of the fused gradients against a float64 composition at the first size.

`--kernels-only` makes a few fused calls and nothing else, for a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/appearance_bench.py --kernels-only`.

usage: python tools/appearance_bench.py [--iters 10] [--windows 5] [--out profiles/appearance.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsplat_amd import appearance as ap  # noqa: E402

SIZES = ((1_000_000, 1), (2_800_000, 1), (1_000_000, 4))
DEV = "cuda"


def inputs(N, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = ap.AppearanceOptModule(8, 32).to(DEV)
    f = (torch.randn(N, 32, generator=g) * 0.5).to(DEV).requires_grad_(True)
    d = torch.randn(C, N, 3, generator=g).to(DEV).requires_grad_(True)
    ids = torch.arange(C, device=DEV) % 8
    w = torch.randn(C, N, 3, generator=g).to(DEV)
    return m, f, ids, d, w


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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "appearance.json"))
    p.add_argument("--kernels-only", action="store_true")
    args = p.parse_args()
    if args.kernels_only:
        m, f, ids, d, w = inputs(*SIZES[0])
        for _ in range(5):
            (ap.appearance(m, f, ids, d, 3) * w).sum().backward()
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "sizes": []}
    for N, C in SIZES:
        m, f, ids, d, w = inputs(N, C)

        def fwd(fn):
            with torch.no_grad():
                fn(m, f, ids, d, 3)

        def both(fn):
            f.grad = d.grad = None
            m.zero_grad(set_to_none=True)
            (fn(m, f, ids, d, 3) * w).sum().backward()

        rows = {"fused_fwd": [], "torch_fwd": [], "fused_fwd_bwd": [], "torch_fwd_bwd": []}
        for _ in range(args.windows):
            rows["fused_fwd"].append(timed(lambda: fwd(ap.appearance), args.iters))
            rows["torch_fwd"].append(timed(lambda: fwd(ap.appearance_torch), args.iters))
            rows["fused_fwd_bwd"].append(timed(lambda: both(ap.appearance), args.iters))
            rows["torch_fwd_bwd"].append(timed(lambda: both(ap.appearance_torch), args.iters))
        R = N * C
        flop_f = 2 * (48 * 64 + 64 * 64 + 3 * 64) * R
        flop_b = flop_f + 2 * 4 * 64 * 64 * R
        bytes_f, bytes_b = 128 * N + 24 * R, 256 * N + 36 * R
        tf, tb = min(rows["fused_fwd"]), min(rows["fused_fwd_bwd"])
        entry = {"N": N, "C": C, "ms": rows,
                 "ratio_fwd": [t / u for t, u in zip(rows["torch_fwd"], rows["fused_fwd"])],
                 "ratio_fwd_bwd": [t / u for t, u in zip(rows["torch_fwd_bwd"], rows["fused_fwd_bwd"])],
                 "fused_wins_every_window": all(t > u for t, u in zip(rows["torch_fwd"], rows["fused_fwd"]))
                 and all(t > u for t, u in zip(rows["torch_fwd_bwd"], rows["fused_fwd_bwd"])),
                 "fwd_tflops": flop_f / tf / 1e9, "fwd_share_of_155_tflops": flop_f / tf / 1e9 / 155.0,
                 "fwd_bwd_tflops": (flop_f + flop_b) / tb / 1e9, "fwd_gb_per_s": bytes_f / tf / 1e6,
                 "fwd_bwd_gb_per_s": (bytes_f + bytes_b) / tb / 1e6}
        result["sizes"].append(entry)
        print(json.dumps(entry))
        del m, f, d, w
        torch.cuda.empty_cache()
    # error of the fused gradients against float64, next to the float32 composition's own
    N, C = 200_000, 2
    m, f, ids, d, w = inputs(N, C, seed=1)
    errs = {}
    for tag, fn, dt in (("f64", ap.appearance_torch, torch.float64), ("f32", ap.appearance_torch, torch.float32), ("fused", ap.appearance, torch.float32)):
        mm = ap.AppearanceOptModule(8, 32).to(DEV).to(dt)
        mm.load_state_dict({k: v.to(dt) for k, v in m.state_dict().items()})
        ff, dd = f.detach().to(dt).requires_grad_(True), d.detach().to(dt).requires_grad_(True)
        (fn(mm, ff, ids, dd, 3) * w.to(dt)).sum().backward()
        errs[tag] = {"v_features": ff.grad.double(), "v_dirs": dd.grad.double(), "v_embeds": mm.embeds.weight.grad.double(),
                     **{"v_" + k: p.grad.double() for k, p in mm.color_head.named_parameters()}}
    result["error_vs_float64"] = {"N": N, "C": C, "note": "near-kink rows not dropped here: the summed gradients include them",
                                  "fused": {k: float((errs["fused"][k] - errs["f64"][k]).abs().max()) for k in errs["f64"]},
                                  "float32_composition": {k: float((errs["f32"][k] - errs["f64"][k]).abs().max()) for k in errs["f64"]},
                                  "max_abs": {k: float(errs["f64"][k].abs().max()) for k in errs["f64"]}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    lost = [(e["N"], e["C"]) for e in result["sizes"] if not e["fused_wins_every_window"]]
    if lost:
        raise SystemExit(f"the fused form lost a window to the torch composition at (N, C) = {lost}")


if __name__ == "__main__":
    main()
