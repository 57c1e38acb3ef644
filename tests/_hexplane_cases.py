"""The cases of tests/golden/hexplane_ref.npz, hexplane_ref_large.npz and hexplane_ref_pass.npz
(tools/pin_hexplane_against_reference.py; the second archive holds the arrays that did not fit the first, the third the case beyond
one pass of the backward's grid) for test_hexplane.py and test_gpu_hexplane.py: loading, running a field on a
case, and the comparison rule, which is _deformation_cases.py's."""
import functools
import json
import os

import numpy as np
import torch

from _deformation_cases import amax

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = tuple(os.path.join(_HERE, "golden", f) for f in ("hexplane_ref.npz", "hexplane_ref_large.npz", "hexplane_ref_pass.npz"))
TAU = 1e-4


@functools.lru_cache(maxsize=None)
def golden():
    out = {}
    for path in GOLDEN:
        z = np.load(path)
        out.update({k: z[k] for k in z.files})
    return out


def cases():
    return json.loads(str(golden()["cases"]))


def case_names():
    return [c["name"] for c in cases()]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def config():
    """{"planes_config": ..., "multires": {field name: factors}} of the fixture's fields."""
    return json.loads(str(golden()["config"]))


def state_dict(fname):
    """Field `fname`'s, as stored from the reference."""
    tag = fname + "_sd_"
    return {k[len(tag):]: torch.from_numpy(v.copy()) for k, v in golden().items() if k.startswith(tag)}


def make_field(fname, device="cpu", dtype=torch.float32):
    from gsplat_amd.hexplane import HexPlaneField

    cfg = config()
    f = HexPlaneField(bounds=float(golden()["bounds"]), planes_config=cfg["planes_config"], multires=cfg["multires"][fname])
    f.load_state_dict(state_dict(fname), strict=True)
    return f.to(device=device, dtype=dtype)


def grid_keys(field):
    return ["v_grids." + k for k, _ in field.grids.named_parameters()]


def outputs(field):
    return ["features", "v_xyzt"] + grid_keys(field)


def all_outputs(fn, field, xyzt, w):
    """features, v_xyzt and every v_grids.{s}.{p} of `fn(field, xyzt)` under the loss sum(features * w); xyzt is made a leaf and
    the planes' gradients are cleared first."""
    for p in field.parameters():
        p.grad = None
    x = xyzt.detach().clone().requires_grad_(True)
    out = fn(field, x)
    (out * w).sum().backward()
    res = {"features": out.detach(), "v_xyzt": x.grad}
    for k, p in field.grids.named_parameters():
        res["v_grids." + k] = p.grad
    return res


def case_inputs(name, device="cpu", dtype=torch.float32):
    z = golden()
    return tuple(torch.from_numpy(z[f"{name}_{k}"]).to(device=device, dtype=dtype) for k in ("xyzt", "w"))


def run_case(name, fn, device="cpu", dtype=torch.float32):
    field = make_field(case(name)["field"], device, dtype)
    return {k: v.detach().cpu() for k, v in all_outputs(fn, field, *case_inputs(name, device, dtype)).items()}


def check(tag, got, ref, err, key):
    """One output under the rule |got - ref| <= 4 * err + 1.2e-7 * max |ref|; returns None or (key, diff, tol)."""
    d, tol = amax(got.to(torch.float64) - ref.to(torch.float64)), 4.0 * err + 1.2e-7 * amax(ref)
    print(f"{tag} {key}: diff {d:.3e} tol {tol:.3e} (err {err:.3e}, max|ref| {amax(ref):.3e})")
    return None if d <= tol else (key, d, tol)


def check_case(name, got):
    """|got - reference| <= 4 * err + 1.2e-7 * max |reference| for every output, err the float32 reference's own distance from
    its float64 evaluation. Prints each figure before it asserts. A case with {name}_feature_rows stores those rows of the
    features only."""
    z = golden()
    if f"{name}_feature_rows" in z:
        got = dict(got, features=got["features"][torch.from_numpy(z[f"{name}_feature_rows"]).long()])
    keys = ["features", "v_xyzt"] + sorted(k[len(name) + 1:] for k in z if k.startswith(name + "_v_grids."))
    assert len(keys) == 2 + 6 * len(config()["multires"][case(name)["field"]])
    bad = [check(name, got[k], torch.from_numpy(z[f"{name}_{k}"]), float(z[f"{name}_err_{k}"]), k) for k in keys]
    assert not any(bad), (name, [b for b in bad if b])


def near_kink(field, xyzt):
    """Rows of xyzt for which, at some axis of some scale, the unclamped float64 index u has -TAU <= u <= size - 1 + TAU and
    |u - round(u)| < TAU (the pin tool's rule)."""
    aabb, x = field.aabb.detach().double(), xyzt.detach().double().reshape(-1, 4)
    pts = torch.cat([(x[:, :3] - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0, x[:, 3:]], dim=-1)
    near = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    for g in field.grids:
        for ax, size in enumerate((g[0].shape[3], g[0].shape[2], g[1].shape[2], g[2].shape[2])):
            u = ((pts[:, ax] + 1.0) / 2.0) * (size - 1)
            near |= (u >= -TAU) & (u <= size - 1 + TAU) & ((u - u.round()).abs() < TAU)
    return near
