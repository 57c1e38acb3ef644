#!/usr/bin/env python
"""Writes tests/golden/hexplane_ref.npz (+ hexplane_ref_large.npz, hexplane_ref_pass.npz): the HexPlane field and its regularisers as the REFERENCE
evaluates them on the CPU (gsplat/contrib/dynamic/hexplane.py: HexPlaneField; regulation.py), forward and backward, for
tests/test_hexplane.py and tests/test_gpu_hexplane.py, which run without a reference checkout. Checks gsplat_amd's torch
composition against it on the way. TEST INFRASTRUCTURE; needs a checkout of the reference. The reference's two files are loaded
by path (they import only torch): `import gsplat` would pull in its CUDA backend.

Fields, all with bounds 1.0, 32 channels and resolution [5, 6, 7, 4] (a distinct size per axis catches an H / W or axis mix-up):
  m2  multires (1, 2), planes seeded uniform(-1, 1) (with the ones of a fresh module the time planes would test nothing);
      stored as m2_sd_{key}
  m1  multires (3,), seeded the same way; stored as m1_sd_{key}
  f2  multires (1, 2), a FRESH module as the reference initialises it (time planes one); stored as f2_sd_{key}

Points are continuous draws: three quarters inside the box, the rest up to 1.5 x bounds outside on either side of each axis
(each axis decides for itself, so a row mixes clamped and free axes); t uniform in [-1.5, 1.5]. The cotangent w is drawn from
nine values in [-1, 1] so that the archive stays small.

Cases (`cases` = JSON list of {name, field, N, dropped, drawn}); the fused forward gives a point to 8 lanes (8 points a wave, 32
a workgroup), the backward a point to a wave (4 a workgroup):
  a  N 1     m2  a single point
  b  N 3     m2  one backward workgroup minus one
  c  N 5     m2  one backward workgroup plus one
  d  N 7     m2  one forward wave minus one
  e  N 9     m2  one forward wave plus one
  f  N 31    m2  one forward workgroup minus one
  g  N 33    m2  one forward workgroup plus one
  h  N 2100  m2  many workgroups, the last one partial
  i  N 200   m1  one scale, factor 3
  j  N 200   f2  a fresh module
  k  N 200   m2  only columns 3..10 and 40..47 of the cotangent are non-zero
  l  N 8300  m2  more than one pass of the backward's persistent grid (2048 workgroups x 4 waves = 8192 points): the last 108
                 points are a wave's second trip. The cotangent repeats with a period of 64 rows, and of the features only the
                 rows l_feature_rows are stored (every 16th and all from 8192 on; the forward has no grid loop), so that the case
                 fits a committed file: a third archive, hexplane_ref_pass.npz. v_xyzt and the plane gradients are whole.
Per case: {name}_xyzt, {name}_w, and under the loss sum(features * w): {name}_features, _v_xyzt, _v_grids.{s}.{p}. Everything is
evaluated a second time in float64 from the same float32 inputs; {name}_err_{output} = max |float32 reference - float64
reference| is the reference's own spread, from which the tests take their tolerance. Arrays above 256 KiB, and the plane gradients
of the cases with N >= 200 (dense, so they do not compress), go to the second archive; each file stays under 1 MiB.

Kinks: v_xyzt jumps where a continuous index crosses an integer. Each case is drawn with spare rows, and a row is dropped when
for any axis at any scale the unclamped float64 index u = (c + 1) / 2 * (size - 1) has -TAU <= u <= size - 1 + TAU and
|u - round(u)| < TAU = 1e-4. Rows farther outside are kept: both precisions clamp them alike. The tool asserts that at most 5 %
are dropped and that the float32 reference's largest index error is at most TAU / 10.

Regularisers: on m2's planes, reg_{plane_smoothness, time_smoothness, time_l1, total} and, for `total` =
hexplane_regularization(field, 0.5, 0.25, 2.0), reg_v_grids.{s}.{p}; reg_err_* as above.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_hexplane_against_reference.py"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("GSPLAT_REFERENCE_PATH"):
    raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (gsplat/contrib/dynamic/hexplane.py)")
REF = os.environ["GSPLAT_REFERENCE_PATH"]

TAU = 1e-4
BOUNDS = 1.0
CONFIG = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [5, 6, 7, 4]}
FIELDS = {"m2": (1, 2), "m1": (3,), "f2": (1, 2)}
LAMBDAS = (0.5, 0.25, 2.0)


def load_reference(name):
    path = os.path.join(REF, "gsplat", "contrib", "dynamic", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def make_fields(ref, g):
    torch.manual_seed(13)
    fields = {}
    for name, multires in FIELDS.items():
        f = ref.HexPlaneField(bounds=BOUNDS, planes_config=CONFIG, multires=multires)
        if name != "f2":
            with torch.no_grad():
                for p in f.grids.parameters():
                    p.copy_(torch.rand(p.shape, generator=g) * 2.0 - 1.0)
        fields[name] = f
    return fields


def draw(n, g):
    """xyzt [n, 4] and the cotangent's value set."""
    inside = torch.rand(n, 4, generator=g) < 0.75
    u = torch.rand(n, 4, generator=g) * 2.0 - 1.0                      # inside: (-1, 1) x bounds
    far = (1.0 + 0.5 * torch.rand(n, 4, generator=g)) * torch.where(torch.rand(n, 4, generator=g) < 0.5, -1.0, 1.0)
    xyzt = torch.where(inside, u, far) * BOUNDS
    xyzt[:, 3] = torch.rand(n, generator=g) * 3.0 - 1.5
    return xyzt.contiguous()


def indices(xyzt, aabb, multires):
    """The unclamped continuous index of every (scale, axis), [n, scales * 4], and the sizes, in xyzt's dtype."""
    norm = (xyzt[:, :3] - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0
    pts = torch.cat([norm, xyzt[:, 3:]], dim=-1)
    cols, sizes = [], []
    for m in multires:
        for ax in range(4):
            size = CONFIG["resolution"][ax] * (m if ax < 3 else 1)
            cols.append(((pts[:, ax] + 1.0) / 2.0) * (size - 1))
            sizes.append(size)
    return torch.stack(cols, dim=1), torch.tensor(sizes, dtype=xyzt.dtype)


def near_kink(xyzt, aabb, multires):
    u, sizes = indices(xyzt.double(), aabb.double(), multires)
    return (((u >= -TAU) & (u <= sizes - 1 + TAU)) & ((u - u.round()).abs() < TAU)).any(dim=1)


def run(cls, multires, sd, xyzt, w, dtype):
    f = cls(bounds=BOUNDS, planes_config=CONFIG, multires=multires).to(dtype)
    f.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    x = xyzt.to(dtype).clone().requires_grad_(True)
    out = f(x)
    (out * w.to(dtype)).sum().backward()
    res = {"features": out.detach(), "v_xyzt": x.grad}
    for k, p in f.grids.named_parameters():
        res["v_grids." + k] = p.grad
    return res


def pin_regularisers(reg, ours, field, out):
    def evaluate(mod, dtype):
        f = type(field)(bounds=BOUNDS, planes_config=CONFIG, multires=FIELDS["m2"]).to(dtype)
        f.load_state_dict({k: v.to(dtype) for k, v in field.state_dict().items()}, strict=True)
        res = {"plane_smoothness": mod.plane_smoothness(f.spatial_planes()).detach(),
               "time_smoothness": mod.time_smoothness(f.temporal_planes()).detach(),
               "time_l1": mod.time_l1(f.temporal_planes()).detach()}
        total = mod.hexplane_regularization(f, *LAMBDAS)
        total.backward()
        res["total"] = total.detach()
        for k, p in f.grids.named_parameters():
            res["v_grids." + k] = p.grad
        return res

    r32, r64, got = evaluate(reg, torch.float32), evaluate(reg, torch.float64), evaluate(ours, torch.float32)
    for k in r32:
        err = amax(r32[k].double() - r64[k])
        assert amax(got[k] - r32[k]) <= 4 * err + 1.2e-7 * amax(r32[k]), ("regularisers", k)
        out["reg_" + k] = r32[k].numpy()
        out["reg_err_" + k] = np.float64(err)
    out["reg_lambdas"] = np.array(LAMBDAS)
    print("regularisers:", {k: float(v) for k, v in r32.items() if v.ndim == 0})


def main():
    ref, reg = load_reference("hexplane"), load_reference("regulation")
    from gsplat_amd import hexplane as ours

    g = torch.Generator().manual_seed(31)
    fields = make_fields(ref, g)
    specs = (("a", "m2", 1), ("b", "m2", 3), ("c", "m2", 5), ("d", "m2", 7), ("e", "m2", 9), ("f", "m2", 31), ("g", "m2", 33),
             ("h", "m2", 2100), ("i", "m1", 200), ("j", "f2", 200), ("k", "m2", 200), ("l", "m2", 8300))
    out, cases = {}, []
    for fname, f in fields.items():
        for k, v in f.state_dict().items():
            out[f"{fname}_sd_{k}"] = v.detach().numpy()
    for name, fname, N in specs:
        f, multires = fields[fname], FIELDS[fname]
        sd = f.state_dict()
        drawn = N + N // 4 + 40  # spare rows
        xyzt = draw(drawn, g)
        w = torch.randint(-4, 5, (drawn, 32 * len(multires)), generator=g).float() / 4.0
        if name == "k":
            mask = torch.zeros(w.shape[1], dtype=torch.bool)
            mask[3:11] = True
            mask[40:48] = True
            w = w * mask
        if name == "l":
            w = w[:64].repeat(drawn // 64 + 1, 1)[:drawn]
        near = near_kink(xyzt, f.aabb.detach(), multires)
        share = float(near.float().mean())
        assert share <= 0.05, (name, share)
        keep = torch.nonzero(~near).flatten()
        assert keep.numel() >= N, (name, keep.numel())
        keep = keep[:N]
        xyzt, w = xyzt[keep].contiguous(), w[keep].contiguous()
        u32, _ = indices(xyzt, f.aabb.detach(), multires)
        u64, _ = indices(xyzt.double(), f.aabb.detach().double(), multires)
        idx_err = amax(u32.double() - u64)
        assert idx_err <= TAU / 10, (name, idx_err)
        r32 = run(ref.HexPlaneField, multires, sd, xyzt, w, torch.float32)
        r64 = run(ref.HexPlaneField, multires, sd, xyzt, w, torch.float64)
        got = run(ours.HexPlaneField, multires, sd, xyzt, w, torch.float32)
        if name == "l":
            rows = torch.unique(torch.cat([torch.arange(0, N, 16), torch.arange(8192, N)]))
            out["l_feature_rows"] = rows.numpy().astype(np.int32)
            for r in (r32, r64, got):
                r["features"] = r["features"][rows]
        err = {k: amax(r32[k].double() - r64[k]) for k in r32}
        # our torch composition against the reference, same inputs, and the state dict the other way round
        for k in r32:
            dlt = amax(got[k] - r32[k])
            assert dlt <= 4 * err[k] + 1.2e-7 * amax(r32[k]), (name, k, dlt, err[k])
        ref.HexPlaneField(bounds=BOUNDS, planes_config=CONFIG, multires=multires).load_state_dict(
            ours.HexPlaneField(bounds=BOUNDS, planes_config=CONFIG, multires=multires).state_dict(), strict=True)
        out[f"{name}_xyzt"], out[f"{name}_w"] = xyzt.numpy(), w.numpy()
        for k in r32:
            out[f"{name}_{k}"] = r32[k].numpy()
            out[f"{name}_err_{k}"] = np.float64(err[k])
        cases.append({"name": name, "field": fname, "N": N, "dropped": int(near.sum()), "drawn": drawn})
        print(f"{name}: dropped {int(near.sum())} of {drawn} ({share:.1%}); index err {idx_err:.2e}; err "
              + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    pin_regularisers(reg, ours, fields["m2"], out)
    out["cases"] = np.array(json.dumps(cases))
    out["tau"] = np.float64(TAU)
    out["bounds"] = np.float64(BOUNDS)
    out["config"] = np.array(json.dumps({"planes_config": CONFIG, "multires": {k: list(v) for k, v in FIELDS.items()}}))
    dense = tuple(c["name"] + "_v_grids." for c in cases if c["N"] >= 200)
    beyond = {k: v for k, v in out.items() if k.startswith("l_")}
    large = {k: v for k, v in out.items() if k not in beyond and (v.nbytes > 256 * 1024 or k.startswith(dense))}
    for tag, part in (("", {k: v for k, v in out.items() if k not in large and k not in beyond}), ("_large", large),
                      ("_pass", beyond)):
        path = os.path.join(ROOT, "tests", "golden", f"hexplane_ref{tag}.npz")
        np.savez_compressed(path, **part)
        size = os.path.getsize(path)
        assert size < 1_000_000, (path, size)
        print("HEXPLANE PINNED ->", path, size, "bytes", sorted(part) if tag else "")


if __name__ == "__main__":
    main()
