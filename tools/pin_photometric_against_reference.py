#!/usr/bin/env python
"""Writes tests/golden/photometric_ref.npz: the photometric loss lerp(l1, ssim_loss, ssim_lambda), with and without masks, as the
REFERENCE's gsplat/losses.py evaluates it on the CPU (masked_l1, masked_ssim, l1_loss, ssim_loss -> torch_ssim_loss), value,
parts and gradient, for tests/test_photometric_loss.py, which runs without a reference checkout. Checks gsplat_amd's torch
composition against it on the way. TEST INFRASTRUCTURE; needs a checkout of the reference.

Cases = shapes x masks x ssim_lambda:
  shapes  a (2, 3, 37, 53), b (1, 1, 16, 16), c (1, 3, 64, 96) - those of ssim_ref.npz: tile edges and a partial tile
  masks   none | b1: [B, 1, H, W] float, ~30 % zeros | bc: [B, C, H, W] float in {0, 0.5, 1} | zeros | ones ([B, 1, H, W])
  lambda  0, 0.2, 1
Keys: {shape}_x, {shape}_y, {shape}_mask_{mask}; per case {shape}_{mask}_{lambda}_loss / _l1 / _ssim / _grad. A gradient that is
bit-identical to one already stored (the all-ones mask repeats the unmasked case, the all-zeros mask gives zeros at every lambda)
is not stored twice: `aliases` is a JSON object {key: key that holds the array}.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_photometric_against_reference.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("GSPLAT_REFERENCE_PATH"):
    raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (its gsplat/losses.py is imported)")
sys.path.insert(0, os.environ["GSPLAT_REFERENCE_PATH"])

SHAPES = (("a", (2, 3, 37, 53)), ("b", (1, 1, 16, 16)), ("c", (1, 3, 64, 96)))
MASKS = ("none", "b1", "bc", "zeros", "ones")
LAMBDAS = (0.0, 0.2, 1.0)


def main():
    from gsplat import losses as ref  # the reference

    from gsplat_amd.losses import photometric_loss

    g = torch.Generator().manual_seed(3)
    out, aliases, seen = {}, {}, {}
    for tag, (B, C, H, W) in SHAPES:
        x = torch.rand(B, C, H, W, generator=g)
        y = (x + 0.1 * torch.randn(B, C, H, W, generator=g)).clamp(0, 1)
        masks = {
            "none": None,
            "b1": (torch.rand(B, 1, H, W, generator=g) >= 0.3).float(),
            "bc": torch.randint(0, 3, (B, C, H, W), generator=g).float() * 0.5,
            "zeros": torch.zeros(B, 1, H, W),
            "ones": torch.ones(B, 1, H, W),
        }
        out[f"{tag}_x"], out[f"{tag}_y"] = x.numpy(), y.numpy()
        for mname in MASKS:
            mask = masks[mname]
            if mask is not None:
                out[f"{tag}_mask_{mname}"] = mask.numpy()
            # conditions on the inputs: the L1 gradient is discontinuous at pred == target, so no selected element may tie;
            # every masked case selects something, except the all-zeros mask, which is there on purpose
            sel = torch.ones_like(x, dtype=torch.bool) if mask is None else (mask != 0).expand_as(x)
            assert int(((x == y) & sel).sum()) == 0, (tag, mname, "pred == target on a selected element")
            assert (int(sel.sum()) > 0) != (mname == "zeros"), (tag, mname, int(sel.sum()))
            for lam in LAMBDAS:
                xr = x.clone().requires_grad_(True)
                if mask is None:
                    l1, ss = ref.l1_loss(xr, y).mean(), ref.ssim_loss(xr, y)
                else:
                    l1, ss = ref.masked_l1(xr, y, mask), ref.masked_ssim(xr, y, mask)
                loss = torch.lerp(l1, ss, lam)
                loss.backward()
                xo = x.clone().requires_grad_(True)
                lo = photometric_loss(xo, y, lam, mask)
                lo.backward()
                dl, dg = abs(float(loss) - float(lo)), float((xr.grad - xo.grad).abs().max())
                assert dl < 2e-6 and dg <= 1e-6 + 1e-4 * float(xr.grad.abs().max()), (tag, mname, lam, dl, dg)
                if mask is not None:
                    assert bool((xr.grad[~sel] == 0).all()), (tag, mname, lam, "gradient under the mask")
                key = f"{tag}_{mname}_{lam:g}"
                out[f"{key}_loss"], out[f"{key}_l1"], out[f"{key}_ssim"] = (np.float32(v.item()) for v in (loss, l1, ss))
                grad = xr.grad.numpy()
                first = seen.setdefault(grad.tobytes(), f"{key}_grad")
                if first == f"{key}_grad":
                    out[first] = grad
                else:
                    aliases[f"{key}_grad"] = first
                print(f"{key:14s} loss {float(loss):.8f} l1 {float(l1):.8f} ssim {float(ss):.8f}  ours: |d loss| {dl:.1e} max |d grad| {dg:.1e}")
    out["aliases"] = np.array(json.dumps(aliases))
    path = os.path.join(ROOT, "tests", "golden", "photometric_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print("PHOTOMETRIC LOSS PINNED ->", path, size, "bytes,", len(aliases), "aliased gradients")


if __name__ == "__main__":
    main()
