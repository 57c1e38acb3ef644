#!/usr/bin/env python
"""Times the fused colour correction (csrc/color_correct.hip) against its torch compositions (`*_torch`: per iteration a
[pixels, 10] feature matrix and one lstsq per channel, what runs without the kernels) on the same device, and writes
profiles/color_correct.json.

Input: one 1080p image, a smooth scene with a colour twist, a quadratic term and noise, about a tenth of img and of ref
saturated. Rows: quadratic (5 iterations, the default) and affine, both under no_grad as in the trainer's eval loop. Per row
`--windows` alternating windows of the two implementations; a window is the host time of a number of calls ending in a device
synchronise, per call; the number of calls is chosen per implementation after the warm-up so that a window lasts about
`--window-seconds`. Recorded: every window, the medians, torch / fused, the largest difference between the two outputs, and the
clock state the driver reports before and after.

usage: python tools/color_correct_bench.py [--windows 7] [--window-seconds 0.3] [--out profiles/color_correct.json]"""
import argparse
import glob
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsplat_amd import color_correct as C  # noqa: E402

DEV = "cuda"
H, W = 1080, 1920
WARMUP = 3  # calls per implementation before a row's windows


def clock_state():
    """What the driver reports, read only: the sclk / mclk tables with the active level starred."""
    out = {}
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_[sm]clk")):
        try:
            with open(path) as f:
                out[path] = f.read().strip().splitlines()
        except OSError as e:
            out[path] = f"unreadable: {e}"
    return out or "not exposed on this machine"


def scene():
    g = torch.Generator().manual_seed(0)
    v, u = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    s = torch.stack([0.5 + 0.42 * torch.sin(2 * math.pi * (a * u + b * v) + p) + 0.22 * torch.sin(2 * math.pi * (3.1 * b * u - 2.3 * a * v) + q)
                     for a, b, p, q in ((1.3, 0.7, 0.4, 2.0), (0.6, 1.5, 1.9, 0.3), (1.1, 1.2, 3.3, 4.4))], dim=-1)
    twist = torch.eye(3) + (torch.rand(3, 3, generator=g) - 0.5) * 0.3
    img = s @ twist + (s * s) @ ((torch.rand(3, 3, generator=g) - 0.5) * 0.24) + 0.02 + 0.01 * torch.randn(H, W, 3, generator=g)
    return img.clamp(0, 1).to(DEV), s.clamp(0, 1).to(DEV)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--window-seconds", type=float, default=0.3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_correct.json"))
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("color_correct_bench: needs a ROCm GPU; a CPU timing says nothing about these kernels")

    img, ref = scene()
    saturated = [float(((t <= 0) | (t >= 1)).float().mean()) for t in (img, ref)]
    rows_spec = [("quadratic", lambda: C.color_correct_quadratic(img, ref), lambda: C.color_correct_quadratic_torch(img, ref),
                  C._FusedColorCorrectQuadratic),
                 ("affine", lambda: C.color_correct_affine(img, ref), lambda: C.color_correct_affine_torch(img, ref),
                  C._FusedColorCorrectAffine)]
    result = {"device": torch.cuda.get_device_name(0), "image": [H, W, 3], "saturated_share_img_ref": saturated,
              "windows": args.windows, "window_seconds": args.window_seconds,
              "timing": "host clock around `iters` calls ending in a device synchronise, ms per call; windows alternate fused / torch",
              "clock_state_before": clock_state(), "rows": []}
    with torch.no_grad():
        for name, fused, composed, counter in rows_spec:
            impls = (("fused", fused), ("torch", composed))
            before, iters = counter.calls, {}
            for k, fn in impls:  # warm-up of the shape the timed windows use, then the calls a window takes
                for _ in range(WARMUP):
                    fn()
                iters[k] = max(1, math.ceil(args.window_seconds * 1e3 / window(fn, 2)))
            ms = {k: [] for k, _ in impls}
            for _ in range(args.windows):
                for k, fn in impls:
                    ms[k].append(window(fn, iters[k]))
            assert counter.calls - before == WARMUP + 2 + args.windows * iters["fused"], "the fused row did not take the kernels"
            med = {k: statistics.median(v) for k, v in ms.items()}
            row = {"method": name, "iters_per_window": iters, "ms_windows": ms, "ms_median": med,
                   "torch_over_fused": med["torch"] / med["fused"], "fused_faster_than_torch": med["fused"] < med["torch"],
                   "fused_faster_than_torch_in_every_window": all(a < b for a, b in zip(ms["fused"], ms["torch"])),
                   "max_abs_difference_of_outputs": float((fused() - composed()).abs().max())}
            result["rows"].append(row)
            print(json.dumps({k: row[k] for k in ("method", "iters_per_window", "ms_median", "torch_over_fused",
                                                  "max_abs_difference_of_outputs")}))
    result["clock_state_after"] = clock_state()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
