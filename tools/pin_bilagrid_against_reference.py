#!/usr/bin/env python
"""Writes tests/golden/bilagrid_ref.npz: bilateral-grid slicing and the total-variation loss as the REFERENCE evaluates them on
the CPU (examples/lib_bilagrid.py: BilateralGrid, slice; gsplat/losses.py: total_variation_loss), forward and backward, for
tests/test_bilagrid.py and tests/test_gpu_bilagrid.py, which run without a reference checkout. Checks gsplat_amd's torch
composition against it on the way. TEST INFRASTRUCTURE; needs a checkout of the reference. `tensorly`, which lib_bilagrid.py
imports for its CP-decomposed 4-D grid only, is replaced by a stub module with a no-op set_backend.

Cases (`cases` = JSON list of {name, kind, grid: [Wg, Hg, L], mats, grids_of}):
  a  image  1 x 37 x 53, pixel-centre xy, default grid 16 x 16 x 8, three grids, the single index 2, colours in [0, 1]
  c  image  1 x 64 x 96, pixel-centre xy, the same three grids, the single index 1, colours in [-0.3, 1.3] (border clamp)
  s  image  2 x 37 x 53, pixel-centre xy, three grids 5 x 7 x 3, per-image indices (1, 2), colours in [-0.3, 1.3]; the
            matrices of its first image are stored
  p  points 2000 x 2 random xy in [0, 1] (some exactly 0 and 1), grid 5 x 7 x 3, a random grid per point, colours in [-0.3, 1.3]
Per case: {name}_rgb, _xy (float32, what the trainer computes: (arange + 0.5) / size), _idx (one int64 per leading entry), _grids,
_w and, under the loss sum(rgb_out * w): _rgb_out, _v_rgb, _v_grids (+ _mats). Everything is evaluated a second time in float64
from the same float32 inputs; err_{output} = max |float32 reference - float64 reference| is the reference's own spread, from
which the tests take their tolerance. v_rgb jumps where the guidance index iz crosses an integer (the derivative of a trilinear
weight), so pixels whose float64 iz lies within 1e-4 of an integer in [0, L - 1] are left out of err_v_rgb and flagged in
{name}_excl; the tool asserts that they are at most 1 % of the case. The perturbed grids and the weights take few distinct
values, and a case whose grids are those of an earlier case names it in `grids_of`, so that the archive stays small.
Total variation: tv{k}_x, tv{k}_loss, tv{k}_grad, tv{k}_err_loss, tv{k}_err_grad for three shapes.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_bilagrid_against_reference.py"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("GSPLAT_REFERENCE_PATH"):
    raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (examples/lib_bilagrid.py, gsplat/losses.py)")
REF = os.environ["GSPLAT_REFERENCE_PATH"]
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "examples"))

JUMP = 1e-4
TV_SHAPES = ((2, 12, 4, 8, 8), (2, 12, 3, 7, 5), (1, 4, 1, 6, 9))


def perturbed_grids(ref_lib, num, shape, g):
    Wg, Hg, L = shape
    m = ref_lib.BilateralGrid(num, grid_X=Wg, grid_Y=Hg, grid_W=L)
    with torch.no_grad():
        m.grids += torch.randint(-4, 5, m.grids.shape, generator=g).float() / 16.0  # up to +-0.25, multiples of 1/16
    return m


def colours(shape, wide, g):
    c = torch.rand(*shape, 3, generator=g)
    return c * 1.6 - 0.3 if wide else c


def centre_xy(I, H, W):
    ys, xs = (torch.arange(H, dtype=torch.float32) + 0.5) / H, (torch.arange(W, dtype=torch.float32) + 0.5) / W
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([gx, gy], dim=-1).unsqueeze(0).repeat(I, 1, 1, 1)


def run_reference(ref_lib, model, xy, rgb, idx, w, dtype):
    """slice + backward of sum(rgb_out * w) in `dtype`; idx [lead] -> the reference's grid_idx [lead, 1...]."""
    m = ref_lib.BilateralGrid(model.grids.shape[0], model.grid_width, model.grid_height, model.grid_guidance).to(dtype)
    with torch.no_grad():
        m.grids.copy_(model.grids.to(dtype))
    rgb = rgb.to(dtype).detach().clone().requires_grad_(True)
    grid_idx = idx.reshape(-1, *([1] * (rgb.dim() - 1))).expand(*rgb.shape[:-1], 1)
    out = ref_lib.slice(m, xy.to(dtype), rgb, grid_idx)
    (out["rgb"] * w.to(dtype)).sum().backward()
    return out["rgb"].detach(), out["rgb_affine_mats"].detach(), rgb.grad, m.grids.grad


def main():
    stub = types.ModuleType("tensorly")
    stub.set_backend = lambda *_a, **_k: None
    sys.modules.setdefault("tensorly", stub)
    import lib_bilagrid as ref_lib  # the reference
    from gsplat import losses as ref_losses

    from gsplat_amd import bilagrid as ours
    from gsplat_amd.losses import total_variation_loss

    g = torch.Generator().manual_seed(11)
    default, small = (16, 16, 8), (5, 7, 3)
    specs = (
        ("a", "image", default, (1, 37, 53), torch.tensor([2]), False, False),
        ("c", "image", default, (1, 64, 96), torch.tensor([1]), True, False),
        ("s", "image", small, (2, 37, 53), torch.tensor([1, 2]), True, True),
        ("p", "points", small, (2000,), None, True, False),
    )
    out, cases, models = {}, [], {}
    for name, kind, gshape, shape, idx, wide, keep_mats in specs:
        grids_of = name if kind == "points" or gshape not in models else models[gshape][0]
        model = perturbed_grids(ref_lib, 3, gshape, g) if grids_of == name else models[gshape][1]
        models.setdefault(gshape, (name, model))
        rgb = colours(shape, wide, g)
        if kind == "image":
            xy = centre_xy(*shape)
        else:
            xy = torch.rand(*shape, 2, generator=g)
            xy[:20] = torch.randint(0, 2, (20, 2), generator=g).float()  # exactly on the border
            idx = torch.randint(0, 3, shape, generator=g)
        w = torch.randint(-4, 5, rgb.shape, generator=g).float() / 4.0
        o32, m32, vr32, vg32 = run_reference(ref_lib, model, xy, rgb, idx, w, torch.float32)
        o64, m64, vr64, vg64 = run_reference(ref_lib, model, xy, rgb, idx, w, torch.float64)
        L = gshape[2]
        iz = (rgb.double() @ torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64)) * (L - 1)
        near = (iz - iz.round()).abs() < JUMP
        excl = near & (iz.round() >= 0) & (iz.round() <= L - 1)
        share = float(excl.float().mean())
        assert share <= 0.01, (name, share)
        keep = ~excl
        err = {"rgb_out": (o32.double() - o64).abs().max(), "v_rgb": (vr32.double() - vr64)[keep].abs().max(),
               "v_grids": (vg32.double() - vg64).abs().max(), "mats": (m32.double() - m64).abs().max()}
        # our torch composition against the reference, same inputs
        mine = ours.BilateralGrid(3, *gshape)
        mine.load_state_dict(model.state_dict())
        r = rgb.clone().requires_grad_(True)
        res = ours.slice_torch(mine, xy, r, idx, affine_mats=True)
        (res["rgb"] * w).sum().backward()
        for what, a, b in (("rgb_out", res["rgb"].detach(), o32), ("mats", res["rgb_affine_mats"].detach(), m32),
                           ("v_rgb", r.grad[keep], vr32[keep]), ("v_grids", mine.grids.grad, vg32)):
            d = float((a - b).abs().max())
            assert d <= 4 * float(err[what]) + 1.2e-7 * float(b.abs().max()), (name, what, d, float(err[what]))
        out.update({f"{name}_rgb": rgb.numpy(), f"{name}_xy": xy.numpy(), f"{name}_idx": idx.numpy().astype(np.int64),
                    f"{name}_w": w.numpy(), f"{name}_rgb_out": o32.numpy(),
                    f"{name}_v_rgb": vr32.numpy(), f"{name}_v_grids": vg32.numpy(), f"{name}_excl": excl.numpy()})
        for k in ("rgb_out", "v_rgb", "v_grids"):
            out[f"{name}_err_{k}"] = np.float64(err[k])
        if grids_of == name:
            out[f"{name}_grids"] = model.grids.detach().numpy()
        if keep_mats:
            out[f"{name}_mats"], out[f"{name}_err_mats"] = m32[0].numpy(), np.float64((m32[0].double() - m64[0]).abs().max())
        cases.append({"name": name, "kind": kind, "grid": list(gshape), "mats": keep_mats, "grids_of": grids_of})
        print(f"{name}: excluded {int(excl.sum())} of {excl.numel()} pixels; err " + " ".join(f"{k} {float(v):.2e}" for k, v in err.items()))
    for k, shape in enumerate(TV_SHAPES):
        x = torch.randn(*shape, generator=g)
        x32 = x.clone().requires_grad_(True)
        l32 = ref_losses.total_variation_loss(x32)
        l32.backward()
        x64 = x.double().requires_grad_(True)
        l64 = ref_losses.total_variation_loss(x64)
        l64.backward()
        xo = x.clone().requires_grad_(True)
        lo = total_variation_loss(xo)
        lo.backward()
        e_loss, e_grad = abs(float(l32) - float(l64)), float((x32.grad.double() - x64.grad).abs().max())
        assert abs(float(lo) - float(l32)) <= 4 * e_loss + 1.2e-7 * abs(float(l32)), (shape, float(lo), float(l32))
        assert float((xo.grad - x32.grad).abs().max()) <= 4 * e_grad + 1.2e-7 * float(x32.grad.abs().max()), shape
        out.update({f"tv{k}_x": x.numpy(), f"tv{k}_loss": np.float32(float(l32)), f"tv{k}_grad": x32.grad.numpy(),
                    f"tv{k}_err_loss": np.float64(e_loss), f"tv{k}_err_grad": np.float64(e_grad)})
        print(f"tv{k} {shape}: loss {float(l32):.8f} err loss {e_loss:.2e} err grad {e_grad:.2e}")
    out["cases"] = np.array(json.dumps(cases))
    out["n_tv"] = np.int64(len(TV_SHAPES))
    path = os.path.join(ROOT, "tests", "golden", "bilagrid_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print("BILATERAL GRID PINNED ->", path, size, "bytes")


if __name__ == "__main__":
    main()
