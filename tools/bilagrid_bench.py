#!/usr/bin/env python
"""The bilateral-grid appearance model on the MI355X: gsplat_amd.bilagrid.slice_image (csrc/bilagrid.hip) against the torch
composition written below - F.grid_sample on the [1, 12, L, Hg, Wg] grid, the [1, H, W, 3, 4] matrices, a batched 3 x 4 product -
at 1080p, one image, default grid 16 x 16 x 8. One JSON object:

  slice     forward alone (no autograd graph) and forward + backward of sum(rgb_out * w); device events around windows of --iters
            iterations after a warm-up, torch and fused windows alternating; the torch form is timed in two series (a, b) so that
            the spread between two timings of the SAME code is known before a difference is read
  slice_xy  the fused kernels given the same coordinates as an explicit xy tensor (the backward is then the plain scatter of
            global atomics), forward + backward
  step_add  slice_image + photometric_loss + 10 x total variation of 200 grids, forward + backward: what a training step gains

usage: bilagrid_bench.py [--iters 100] [--windows 5] [--out profiles/bilagrid.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

I, H, W = 1, 1080, 1920
N_GRIDS = 200  # one per training image, as the trainer allocates them


def torch_slice(grids, xy, rgb, idx):
    """The torch path a user has without the kernels: grid_sample + affine product."""
    gray = (rgb * rgb.new_tensor([0.299, 0.587, 0.114])).sum(-1, keepdim=True)
    coords = torch.cat([(xy - 0.5) * 2.0, gray * 2.0 - 1.0], dim=-1).unsqueeze(1)  # [I, 1, H, W, 3]
    mats = F.grid_sample(grids[idx], coords, mode="bilinear", align_corners=True, padding_mode="border")  # [I, 12, 1, H, W]
    mats = mats.permute(0, 2, 3, 4, 1).reshape(*rgb.shape[:-1], 3, 4)
    return torch.matmul(mats[..., :3], rgb.unsqueeze(-1)).squeeze(-1) + mats[..., 3]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def compare(forms, iters, windows):
    """forms: {name: callable}; returns per-form windows and medians (alternating windows, warm-up first)."""
    for fn in forms.values():
        window(fn, 10)
    ms = {k: [] for k in forms}
    for _ in range(windows):
        for k, fn in forms.items():
            ms[k].append(window(fn, iters))
    return {"ms_windows": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()}}


def clock_state():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln or "Performance Level" in ln][:6]
    except Exception as e:  # the tool is optional
        return [f"unavailable: {e}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON object to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    from gsplat_amd import bilagrid
    from gsplat_amd.losses import photometric_loss

    gen = torch.Generator().manual_seed(5)
    model = bilagrid.BilateralGrid(N_GRIDS).to(dev)
    with torch.no_grad():
        model.grids += (0.05 * torch.randn(model.grids.shape, generator=gen)).to(dev)
    grids = model.grids
    rgb = torch.rand(I, H, W, 3, generator=gen).to(dev)
    target = (rgb + 0.05 * torch.randn(I, H, W, 3, generator=gen).to(dev)).clamp(0, 1)
    w = torch.randn(I, H, W, 3, generator=gen).to(dev)
    idx = torch.tensor([17], device=dev)
    xy = bilagrid.pixel_center_xy(I, H, W, device=dev).contiguous()
    leaf = rgb.clone().requires_grad_(True)

    def fwd_bwd(slicer):
        def run():
            leaf.grad = None
            grids.grad = None
            (slicer(leaf) * w).sum().backward()
        return run

    def fwd_only(slicer):
        def run():
            with torch.no_grad():
                slicer(rgb)
        return run

    t_slice = lambda x: torch_slice(grids, xy, x, idx)  # noqa: E731
    f_slice = lambda x: bilagrid.slice_image(model, x, idx)["rgb"]  # noqa: E731
    f_slice_xy = lambda x: bilagrid.slice(model, xy, x, idx.reshape(1, 1, 1, 1))["rgb"]  # noqa: E731

    # agreement of the two forms at the timed size
    fwd_bwd(t_slice)()
    ot, gt_rgb, gt_grid = t_slice(rgb).detach(), leaf.grad.clone(), grids.grad.clone()
    fwd_bwd(f_slice)()
    of = f_slice(rgb).detach()
    agree = {"max_abs_rgb_out_diff": float((ot - of).abs().max()),
             "max_abs_v_grids_diff": float((gt_grid - grids.grad).abs().max()), "max_abs_v_grids": float(gt_grid.abs().max()),
             "median_abs_v_rgb_diff": float((gt_rgb - leaf.grad).abs().median())}

    result = {"device": torch.cuda.get_device_name(0), "image": [I, H, W, 3], "grid": [N_GRIDS, 12, 8, 16, 16],
              "iters_per_window": a.iters, "windows": a.windows, "clock_state": clock_state(), "agreement": agree}
    fwd = compare({"torch_a": fwd_only(t_slice), "fused": fwd_only(f_slice), "torch_b": fwd_only(t_slice)}, a.iters, a.windows)
    both = compare({"torch_a": fwd_bwd(t_slice), "fused": fwd_bwd(f_slice), "torch_b": fwd_bwd(t_slice)}, a.iters, a.windows)
    for rec in (fwd, both):
        m = rec["median_ms"]
        torch_med = statistics.median(rec["ms_windows"]["torch_a"] + rec["ms_windows"]["torch_b"])
        rec.update({"torch_median_ms": round(torch_med, 4), "fused_median_ms": m["fused"],
                    "torch_run_to_run_spread_ms": round(abs(m["torch_a"] - m["torch_b"]), 4),
                    "fused_over_torch": round(m["fused"] / torch_med, 4), "fused_faster": bool(m["fused"] < torch_med)})
    result["slice"] = {"forward": fwd, "forward_backward": both}
    result["slice_xy"] = {"forward_backward": compare({"fused_xy": fwd_bwd(f_slice_xy)}, a.iters, a.windows)}

    tp = target.permute(0, 3, 1, 2)

    def step_add(slicer):
        def run():
            leaf.grad = None
            grids.grad = None
            loss = photometric_loss(slicer(leaf).permute(0, 3, 1, 2), tp, 0.2) + 10.0 * model.tv_loss()
            loss.backward()
        return run

    def loss_alone():
        leaf.grad = None
        photometric_loss(leaf.permute(0, 3, 1, 2), tp, 0.2).backward()

    result["step_add"] = compare({"photometric_loss_alone": loss_alone, "fused_slice_loss_tv": step_add(f_slice),
                                  "torch_slice_loss_tv": step_add(t_slice)}, a.iters, a.windows)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
