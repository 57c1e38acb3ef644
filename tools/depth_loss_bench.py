#!/usr/bin/env python
"""Times the fused depth-supervision losses (csrc/depth_loss.hip) against their torch compositions (`*_torch`, what runs without
the kernels) and against a restatement of the reference's formulas (gsplat/losses.py:209-320 with its boolean indexing;
examples/simple_trainer.py:962-980 for the sampled loss) on the same device, and writes profiles/depth_losses.json.

Inputs: one 1080p image; the predicted depth is channel 3 of a [1, 1080, 1920, 4] render (the `renders[..., 3:4]` view a trainer
passes), unmasked and with a uint8 mask that drops ~30 %; the sampled loss takes M = 5000 points. Rows: loss x mask x (forward,
forward + backward). Per row `--windows` alternating windows of the three implementations; a window is the host time of
`--iters` calls ending in a device synchronise, per call (the losses are launch-bound: the enqueue cost is what a step pays;
3000 calls make the shortest window about 0.1 s), after a warm-up of 200 calls of each. Recorded: every window, the median
per implementation, torch / fused and reference / fused, whether the fused form is no slower than the torch composition in every row, that a masked fused forward + backward makes no
host read (torch's synchronisation debug mode), and the clock state the driver reports before and after.

usage: python tools/depth_loss_bench.py [--iters 3000] [--windows 7] [--out profiles/depth_losses.json]"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsplat_amd import losses as L  # noqa: E402

DEV = "cuda"
H, W, M, SCALE = 1080, 1920, 5000, 1.75
WARMUP = 200  # calls per implementation before a row's windows


# ---- the reference's formulas restated: the same operations, with the boolean indexing (a count read back by the host) and the
# ---- host-side decisions that the fused and the `*_torch` forms avoid
def _inverse_where_positive(depth):
    return torch.where(depth > 0.0, depth.reciprocal(), torch.zeros_like(depth))  # NaN gradient at a depth of exactly 0


def ref_depth_l1(pred, gt, scale):
    return scale * F.l1_loss(_inverse_where_positive(pred), _inverse_where_positive(gt))


def _mean_of_indexed(values, keep):
    picked = values[keep.expand_as(values)]  # boolean indexing
    return picked.mean() if picked.numel() > 0 else values.sum() * 0.0  # decided on the host


def ref_binocular(pred, gt, mask=None, eps=1e-7):
    ok_pred, ok_gt = pred.abs() > eps, gt.abs() > eps
    one = torch.ones_like(pred)
    difference = (torch.where(ok_pred, pred, one).reciprocal() - torch.where(ok_gt, gt, one).reciprocal()).abs()
    weight = (ok_pred & ok_gt).to(pred.dtype)
    if mask is not None:
        weight = weight * mask.to(pred.dtype)
    return _mean_of_indexed(difference, weight != 0)


def ref_pearson(pred, gt, mask=None):
    p, g = pred.flatten(), gt.flatten()
    if mask is not None:
        keep = mask.flatten() != 0
        p, g = p[keep], g[keep]  # boolean indexing
    if p.numel() < 2:  # decided on the host
        return pred.sum() * 0.0
    dp, dg = p - p.mean(), g - g.mean()
    return 1.0 - (dp * dg).sum() / ((dp * dp).sum() * (dg * dg).sum()).clamp(min=1e-12).sqrt()


def ref_sampled(depth, points, depths_gt, scale):
    """The trainers' block: coordinates normalised to [-1, 1], F.grid_sample(align_corners=True), the disparity L1."""
    h, w = depth.shape[1:3]
    grid = (points / points.new_tensor([w - 1, h - 1]) * 2 - 1)[:, :, None, :]  # [C, M, 1, 2]
    sampled = F.grid_sample(depth.permute(0, 3, 1, 2), grid, align_corners=True)[:, 0, :, 0]
    return ref_depth_l1(sampled, depths_gt, scale)


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


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=3000)
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_losses.json"))
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_loss_bench: needs a ROCm GPU; a CPU timing says nothing about these kernels")

    g = torch.Generator().manual_seed(0)
    renders = torch.rand(1, H, W, 4, generator=g).to(DEV)
    renders[..., 3] = renders[..., 3] * 4 + 1  # depths 1 .. 5, positive everywhere: the reference's gradients are finite
    renders.requires_grad_(True)
    gt = (renders.detach()[..., 3:4] * (1 + 0.1 * torch.randn(1, H, W, 1, generator=g).to(DEV))).clamp_min(0.5).contiguous()
    mask = (torch.rand(1, H, W, 1, generator=g) > 0.3).to(torch.uint8).to(DEV)
    points = (torch.rand(1, M, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).to(DEV)
    depths_gt = (torch.rand(1, M, generator=g) * 4 + 1).to(DEV)

    def pred():
        return renders[..., 3:4]

    rows_spec = [
        ("depth_l1_loss", "none", lambda: L.depth_l1_loss(pred(), gt, SCALE), lambda: L.depth_l1_loss_torch(pred(), gt, SCALE),
         lambda: ref_depth_l1(pred(), gt, SCALE)),
        ("binocular_disparity_l1", "none", lambda: L.binocular_disparity_l1(pred(), gt), lambda: L.binocular_disparity_l1_torch(pred(), gt),
         lambda: ref_binocular(pred(), gt)),
        ("binocular_disparity_l1", "uint8", lambda: L.binocular_disparity_l1(pred(), gt, mask),
         lambda: L.binocular_disparity_l1_torch(pred(), gt, mask), lambda: ref_binocular(pred(), gt, mask)),
        ("pearson_depth_loss", "none", lambda: L.pearson_depth_loss(pred(), gt), lambda: L.pearson_depth_loss_torch(pred(), gt),
         lambda: ref_pearson(pred(), gt)),
        ("pearson_depth_loss", "uint8", lambda: L.pearson_depth_loss(pred(), gt, mask), lambda: L.pearson_depth_loss_torch(pred(), gt, mask),
         lambda: ref_pearson(pred(), gt, mask)),
        ("sampled_depth_l1_loss", "none", lambda: L.sampled_depth_l1_loss(pred(), points, depths_gt, SCALE),
         lambda: L.sampled_depth_l1_loss_torch(pred(), points, depths_gt, SCALE), lambda: ref_sampled(pred(), points, depths_gt, SCALE)),
    ]
    result = {"device": torch.cuda.get_device_name(0), "image": [1, H, W], "points": M, "iters": args.iters, "windows": args.windows,
              "timing": "host clock around `iters` calls ending in a device synchronise, ms per call; windows alternate fused / torch / reference",
              "clock_state_before": clock_state(), "rows": []}
    counters = (L._FusedDisparityL1, L._FusedPearsonDepth, L._FusedSampledDepthL1)
    for name, mask_kind, fused, composed, reference in rows_spec:
        values = {}
        for direction in ("fwd", "fwd_bwd"):
            def run(fn):
                if direction == "fwd":
                    with torch.no_grad():
                        fn()
                else:
                    renders.grad = None
                    fn().backward()

            impls = (("fused", fused), ("torch", composed), ("reference", reference))
            before = sum(c.calls for c in counters)
            for _, fn in impls:  # warm-up of every shape the timed windows use
                for _ in range(WARMUP):
                    run(fn)
            ms = {k: [] for k, _ in impls}
            for _ in range(args.windows):
                for k, fn in impls:
                    ms[k].append(window(lambda: run(fn), args.iters))
            assert sum(c.calls for c in counters) - before == WARMUP + args.windows * args.iters, "the fused row did not take the kernels"
            med = {k: statistics.median(v) for k, v in ms.items()}
            with torch.no_grad():
                values = {k: float(fn()) for k, fn in impls}
            row = {"loss": name, "mask": mask_kind, "direction": direction, "ms_windows": ms, "ms_median": med,
                   "torch_over_fused": med["torch"] / med["fused"], "reference_over_fused": med["reference"] / med["fused"],
                   "fused_no_slower_than_torch": med["fused"] <= med["torch"],
                   "fused_no_slower_than_torch_in_every_window": all(a <= b for a, b in zip(ms["fused"], ms["torch"])),
                   "loss_values": values}
            result["rows"].append(row)
            print(json.dumps({k: row[k] for k in ("loss", "mask", "direction", "ms_median", "torch_over_fused", "reference_over_fused")}))
    # the masked fused paths make no host read
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        renders.grad = None
        (L.binocular_disparity_l1(pred(), gt, mask) + L.pearson_depth_loss(pred(), gt, mask)).backward()
        result["masked_fused_host_reads"] = 0
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    result["clock_state_after"] = clock_state()
    result["fused_no_slower_than_torch_every_row"] = all(r["fused_no_slower_than_torch"] for r in result["rows"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out, "fused no slower than torch in every row:", result["fused_no_slower_than_torch_every_row"])


if __name__ == "__main__":
    main()
