#!/usr/bin/env python
"""The training step's photometric loss lerp(L1, 1 - SSIM, 0.2) on the MI355X: gsplat_amd.photometric_loss (one fused kernel per
direction, csrc/ssim.hip) against the composed form that tools/train_step_bench.py uses without --fused-loss, with and without
a mask. Three parts, one JSON object:

  loss      1 x 3 x 1080 x 1920 in channels-last storage (the rasterizer's [B, H, W, C] output), forward + backward, device events
            around windows of --iters iterations, composed and fused windows alternating; the composed form is timed in two
            series (A, B) so that the spread between two timings of the SAME code is known before a difference is read.
            The masked composed form is the reference trainer's (examples/simple_trainer.py:946-961): boolean indexing for L1,
            colors * masks[..., None] for SSIM.
  step      tools/train_step_bench.py with and without fused_loss, alternating (--step-repeats pairs; 0 skips the part)
  kernels   --kernels only: a short run of the fused loss for `rocprofv3 --kernel-trace --stats -- python tools/photometric_bench.py
            --kernels`; --kernel-stats <csv> then joins that run's kernel times with the bytes below

Algorithmic bytes per launch, from the shapes (what the kernels must move once, not what the caches serve again):
  forward   read pred, target (2 images) + the mask, write the three derivative maps (3 images)
  backward  read pred, target, three derivative maps (5 images) + the mask, write the gradient (1 image)

usage: photometric_bench.py [--iters 200] [--windows 5] [--step-repeats 2] [--out profiles/photometric_loss.json]"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, C, H, W = 1, 3, 1080, 1920
HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, specification


def algorithmic_bytes(mask_shape=None, mask_itemsize=0):
    image = B * C * H * W * 4
    mask = 0 if mask_shape is None else mask_itemsize * mask_shape[0] * mask_shape[1] * mask_shape[2] * mask_shape[3]
    return {"image_bytes": image, "mask_bytes": mask, "forward": 2 * image + mask + 3 * image, "backward": 5 * image + mask + image}


def make_inputs(dev, mask_fraction=0.3):
    gen = torch.Generator().manual_seed(5)
    rc = torch.rand(B, H, W, C, generator=gen).to(dev)
    target = (rc + 0.05 * torch.randn(B, H, W, C, generator=gen).to(dev)).clamp(0, 1)
    masks = (torch.rand(B, H, W, generator=gen) >= mask_fraction).to(dev)
    return rc, target, masks


def loss_forms(rc, target, masks):
    """{name: f(leaf) -> loss}; rc-shaped leaf in [B, H, W, C] storage, as the rasterizer returns it."""
    from gsplat_amd.losses import photometric_loss, ssim_loss

    tp = target.permute(0, 3, 1, 2)
    mask4 = masks[:, None]

    def composed(x):  # tools/train_step_bench.py without --fused-loss
        return torch.lerp((x - target).abs().mean(), ssim_loss(x.permute(0, 3, 1, 2), tp), 0.2)

    def composed_masked(x):  # examples/simple_trainer.py:946-961
        l1 = (x[masks] - target[masks]).abs().mean()
        return torch.lerp(l1, ssim_loss((x * masks[..., None]).permute(0, 3, 1, 2), (target * masks[..., None]).permute(0, 3, 1, 2)), 0.2)

    return {
        "unmasked": (composed, lambda x: photometric_loss(x.permute(0, 3, 1, 2), tp, 0.2)),
        "masked": (composed_masked, lambda x: photometric_loss(x.permute(0, 3, 1, 2), tp, 0.2, mask4)),
    }


def time_window(fn, leaf, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        leaf.grad = None
        fn(leaf).backward()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def bench_loss(dev, iters, windows):
    rc, target, masks = make_inputs(dev)
    leaf = rc.clone().requires_grad_(True)
    out = {}
    for case, (composed, fused) in loss_forms(rc, target, masks).items():
        lc, lf = composed(leaf), fused(leaf)
        gc = torch.autograd.grad(lc, leaf)[0]
        gf = torch.autograd.grad(lf, leaf)[0]
        agree = {"loss_composed": float(lc.detach()), "loss_fused": float(lf.detach()),
                 "max_abs_grad_diff": float((gc - gf).abs().max()), "max_abs_grad": float(gc.abs().max())}
        series = {"composed_a": composed, "fused": fused, "composed_b": composed}
        for fn in series.values():  # warm-up of every form at the timed shape
            time_window(fn, leaf, 20)
        ms = {k: [] for k in series}
        for _ in range(windows):
            for k, fn in series.items():
                ms[k].append(time_window(fn, leaf, iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = abs(med["composed_a"] - med["composed_b"])
        composed_med = statistics.median(ms["composed_a"] + ms["composed_b"])
        out[case] = {
            "ms_windows": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "median_ms": {k: round(t, 4) for k, t in med.items()},
            "composed_median_ms": round(composed_med, 4), "fused_median_ms": round(med["fused"], 4),
            "composed_run_to_run_spread_ms": round(spread, 4),
            "fused_over_composed": round(med["fused"] / composed_med, 4),
            "fused_not_slower": bool(med["fused"] <= composed_med + spread),
            "agreement": agree,
        }
    return out


def bench_step(dev, repeats, steps):
    import train_step_bench

    out = {}
    for case, frac in (("unmasked", 0.0), ("masked", 0.3)):
        ms = {"composed": [], "fused": []}
        loss = {}
        for _ in range(repeats):
            for k, fused in (("composed", False), ("fused", True)):
                r = train_step_bench.run(steps=steps, device=dev, fused_loss=fused, mask_fraction=frac)
                ms[k].append(r["ms_per_step"])
                loss[k] = r["final_loss"]
        out[case] = {"ms_per_step": ms, "median_ms_per_step": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                     "final_loss": loss, "steps": steps}
    return out


def kernels_run(dev, iters=50):
    """What `rocprofv3 --kernel-trace --stats` wraps: the fused loss, masked ([B, 1, H, W] bool mask), forward + backward; then the
    composed unmasked form, whose gsx_ssim_* launches are the same kernel body without the photometric switch."""
    rc, target, masks = make_inputs(dev)
    leaf = rc.clone().requires_grad_(True)
    forms = loss_forms(rc, target, masks)
    time_window(forms["masked"][1], leaf, iters)
    time_window(forms["unmasked"][0], leaf, iters)


def kernel_stats(path):
    """Joins a rocprofv3 kernel_stats.csv of kernels_run() with the algorithmic bytes: time, bytes / s, share of the HBM peak."""
    byt = algorithmic_bytes((B, 1, H, W), 1)
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        kind = ("forward" if "ssim_kernelILb0ELb1" in name or "ssim_kernel<false, true>" in name else
                "backward" if "ssim_kernelILb1ELb1" in name or "ssim_kernel<true, true>" in name else
                "finish" if "photometric_finish" in name else
                "ssim_forward" if "ssim_kernelILb0ELb0" in name or "ssim_kernel<false, false>" in name else
                "ssim_backward" if "ssim_kernelILb1ELb0" in name or "ssim_kernel<true, false>" in name else None)
        if kind is None:
            continue
        us = float(r["AverageNs"]) / 1e3
        rows[kind] = {"kernel": name[:120], "calls": int(r["Calls"]), "average_us": round(us, 2)}
        if kind in byt:
            rate = byt[kind] / (us * 1e-6)
            rows[kind].update({"algorithmic_bytes": byt[kind], "bytes_per_s": round(rate, -9),
                               "share_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_S, 4)})
    return {"hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "mask": "[1, 1, 1080, 1920] bool", **rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--step-repeats", type=int, default=2)
    ap.add_argument("--step-steps", type=int, default=100)
    ap.add_argument("--kernels", action="store_true", help="only the short fused run that a kernel trace wraps")
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats.csv of a --kernels run: print kernel times over algorithmic bytes")
    ap.add_argument("--out", help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.kernel_stats:
        result = {"kernels": kernel_stats(a.kernel_stats)}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("photometric_bench.py measures on the GPU; none found")
        dev = torch.device("cuda", 0)
        import gsplat_amd  # noqa: F401

        if a.kernels:
            kernels_run(dev)
            return
        result = {"device": torch.cuda.get_device_name(0), "shape": [B, C, H, W], "storage": "[B, H, W, C]", "ssim_lambda": 0.2,
                  "mask_fraction": 0.3, "iters_per_window": a.iters, "windows": a.windows,
                  "algorithmic_bytes": {"unmasked": algorithmic_bytes(), "masked": algorithmic_bytes((B, 1, H, W), 1)},
                  "loss": bench_loss(dev, a.iters, a.windows)}
        if a.step_repeats > 0:
            result["step"] = bench_step(dev, a.step_repeats, a.step_steps)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
