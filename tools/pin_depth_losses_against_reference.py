#!/usr/bin/env python
"""Writes tests/golden/depth_losses_ref.npz: depth_l1_loss, binocular_disparity_l1 and pearson_depth_loss as the REFERENCE's
gsplat/losses.py evaluates them on the CPU, and the trainers' sampled form (examples/simple_trainer.py:962-980: normalise,
F.grid_sample(align_corners=True), depth_l1_loss), value and gradient in float32 and float64, for every case of
tests/_depth_cases.py. tests/test_depth_losses.py reads it and runs without a reference checkout. Checks gsplat_amd's torch
compositions against it on the way. TEST INFRASTRUCTURE; needs a checkout of the reference.

Keys per case: {name}/loss32, /loss64, /grad32, /grad64 and the inputs {name}/pred, /gt, /mask (dense) or /map, /points,
/depths_gt (sampled). Cases above SPAN + 1 elements keep every GRAD_STRIDE-th element of each gradient and no inputs (the
builders are seeded; {name}/sum holds the float64 sum of pred and of gt as a check on them). The reference's Pearson loss
flattens its mask without broadcasting it, so a broadcast mask is expanded before the call. Where a predicted depth is 0 the
reference's gradient is NaN; it is stored as it is.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_depth_losses_against_reference.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if not os.environ.get("GSPLAT_REFERENCE_PATH"):
    raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (its gsplat/losses.py is imported)")
sys.path.insert(0, os.environ["GSPLAT_REFERENCE_PATH"])

GRAD_STRIDE = 4099


def main():
    from gsplat import losses as ref  # the reference

    import _depth_cases as dc
    from gsplat_amd import losses as ours

    span = dc.launch_edges()[0]
    out = {}

    def run(fn, x, dtype):
        x = x.to(dtype).clone().requires_grad_(True)
        val = fn(x)
        val.backward()
        return val.detach(), x.grad

    def agree(name, a, b, dtype):
        (la, ga), (lb, gb) = a, b
        tol = 1e-5 if dtype == torch.float32 else 1e-13
        both_nan = bool(torch.isnan(la)) and bool(torch.isnan(lb))
        assert both_nan or abs(float(la) - float(lb)) <= tol * max(1.0, abs(float(la))), (name, dtype, float(la), float(lb))
        ok = torch.isfinite(ga)  # NaN where the reference back-propagates inf * 0
        assert bool(torch.isfinite(gb).all()), (name, dtype, "our gradient is not finite")
        if ok.any():
            assert float((ga - gb)[ok].abs().max()) <= tol * max(1e-30, float(ga[ok].abs().max())), (name, dtype)

    for case in dc.dense_cases():
        pred, gt, mask = dc.dense_inputs(case)
        small = pred.numel() <= span + 1
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            g = gt.to(dtype)
            if case.loss == "l1":
                theirs = run(lambda p: ref.depth_l1_loss(p, g, scene_scale=dc.SCALE), pred, dtype)
                mine = run(lambda p: ours.depth_l1_loss_torch(p, g, dc.SCALE), pred, dtype) if pred.numel() else theirs
            elif case.loss == "bin":
                theirs = run(lambda p: ref.binocular_disparity_l1(p, g, mask), pred, dtype)
                mine = run(lambda p: ours.binocular_disparity_l1_torch(p, g, mask), pred, dtype)
            else:
                full = None if mask is None else mask.expand(case.shape)
                theirs = run(lambda p: ref.pearson_depth_loss(p, g, full), pred, dtype)
                mine = run(lambda p: ours.pearson_depth_loss_torch(p, g, mask), pred, dtype)
            if not dc.degenerate(case):
                agree(case.name, theirs, mine, dtype)
            out[f"{case.name}/loss{tag}"] = theirs[0].numpy()
            out[f"{case.name}/grad{tag}"] = (theirs[1] if small else theirs[1].reshape(-1)[::GRAD_STRIDE]).numpy()
        if small:
            out[f"{case.name}/pred"], out[f"{case.name}/gt"] = pred.numpy(), gt.numpy()
            if mask is not None:
                out[f"{case.name}/mask"] = mask.numpy()
        else:
            out[f"{case.name}/sum"] = np.array([float(pred.double().sum()), float(gt.double().sum())])

    for case in dc.sampled_cases():
        dm, pts, dgt = dc.sampled_inputs(case)
        C, H, W = dm.shape
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            p, g = pts.to(dtype), dgt.to(dtype)

            def trainer(m):  # examples/simple_trainer.py:962-980 with depths = m[..., None]
                grid = torch.stack([p[:, :, 0] / (W - 1) * 2 - 1, p[:, :, 1] / (H - 1) * 2 - 1], dim=-1).unsqueeze(2)
                d = F.grid_sample(m[..., None].permute(0, 3, 1, 2), grid, align_corners=True).squeeze(3).squeeze(1)
                return ref.depth_l1_loss(d, g, scene_scale=dc.SCALE)

            theirs = run(trainer, dm, dtype)
            mine = run(lambda m: ours.sampled_depth_l1_loss_torch(m, p, g, dc.SCALE), dm, dtype)
            agree(case.name, theirs, mine, dtype)
            out[f"{case.name}/loss{tag}"], out[f"{case.name}/grad{tag}"] = theirs[0].numpy(), theirs[1].numpy()
        out[f"{case.name}/map"], out[f"{case.name}/points"], out[f"{case.name}/depths_gt"] = dm.numpy(), pts.numpy(), dgt.numpy()

    path = os.path.join(ROOT, "tests", "golden", "depth_losses_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "photometric_ref.npz")), size
    print("DEPTH LOSSES PINNED ->", path, size, "bytes,", len(dc.dense_cases()), "dense and", len(dc.sampled_cases()), "sampled cases")


if __name__ == "__main__":
    main()
