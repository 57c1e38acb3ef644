"""The cases of tests/golden/deformation_ref.npz and deformation_ref_rows.npz (tools/pin_deformation_against_reference.py; the
second archive holds the arrays too large for the first) for test_deformation.py and test_gpu_deformation.py: loading, running a
module on a case, and the comparison rule."""
import functools
import json
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = tuple(os.path.join(_HERE, "golden", f) for f in ("deformation_ref.npz", "deformation_ref_rows.npz"))
PARAMS = ("trunk.0.weight", "trunk.0.bias", "trunk.2.weight", "trunk.2.bias", "trunk.4.weight", "trunk.4.bias",
          "pos_head.weight", "pos_head.bias", "quat_head.weight", "quat_head.bias", "opacity_head.weight", "opacity_head.bias")
TRUNK = PARAMS[:6]
NEW = ("means_new", "quats_new", "opacities_new")
INPUTS = ("means", "quats", "opacities", "plane_features")
WEIGHTS = ("w_means", "w_quats", "w_opac")
OUTPUTS = NEW + tuple("v_" + k for k in INPUTS) + tuple("v_" + p for p in PARAMS)
TAU = 2e-5


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


def state_dict():
    """d3's, as stored from the reference."""
    return {k[len("d3_sd_"):]: torch.from_numpy(v.copy()) for k, v in golden().items() if k.startswith("d3_sd_")}


def make_module(mname, device="cpu", dtype=torch.float32):
    """`d3`: the stored state_dict. `z3`: a fresh module, its zero heads untouched, with d3's trunk."""
    from gsplat_amd.deformation import DeformNetwork

    m = DeformNetwork(64)
    if mname == "d3":
        m.load_state_dict(state_dict(), strict=True)
    else:
        assert mname == "z3"
        m.trunk.load_state_dict({k[len("trunk."):]: v for k, v in state_dict().items() if k.startswith("trunk.")}, strict=True)
    return m.to(device=device, dtype=dtype)


def call_module(m, means, quats, opacities, x):
    return m(means, quats, opacities, None, x)


def all_outputs(fn, m, inputs, weights):
    """Every output of OUTPUTS for `fn(module, means, quats, opacities, plane_features)` under the loss
    sum(means_new * w_means) + sum(quats_new * w_quats) + sum(opacities_new * w_opac); `inputs` are made leaves."""
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    outs = fn(m, *leaves)
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    res = {k: o.detach() for k, o in zip(NEW, outs)}
    res.update({"v_" + k: t.grad for k, t in zip(INPUTS, leaves)})
    for p in PARAMS:  # a parameter that autograd left out (a head the loss does not use) has a zero gradient
        q = m.get_parameter(p)
        res["v_" + p] = q.grad if q.grad is not None else torch.zeros_like(q)
    return res


def run_case(name, fn, device="cpu", dtype=torch.float32):
    c, z = case(name), golden()
    m = make_module(c["module"], device, dtype)
    inputs = [torch.from_numpy(z[f"{name}_{k}"]).to(device=device, dtype=dtype) for k in INPUTS]
    weights = [torch.from_numpy(z[f"{name}_{k}"]).to(device=device, dtype=dtype) for k in WEIGHTS]
    return {k: v.detach().cpu() for k, v in all_outputs(fn, m, inputs, weights).items()}


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def check_case(name, got):
    """|got - reference| <= 4 * err + 1.2e-7 * max |reference| for every output, err the float32 reference's own distance from
    its float64 evaluation. Prints each figure before it asserts."""
    z, bad = golden(), []
    for k in OUTPUTS:
        ref, err = torch.from_numpy(z[f"{name}_{k}"]), float(z[f"{name}_err_{k}"])
        d, tol = amax(got[k].to(torch.float64) - ref.to(torch.float64)), 4.0 * err + 1.2e-7 * amax(ref)
        print(f"{name} {k}: diff {d:.3e} tol {tol:.3e} (err {err:.3e}, max|ref| {amax(ref):.3e})")
        if not d <= tol:
            bad.append((k, d, tol))
    assert not bad, (name, bad)


def compare(tag, got, r32, r64, keys=OUTPUTS):
    """The same rule where no fixture exists: truth is the float64 composition `r64`, the spread its own float32 run `r32`."""
    bad = []
    for k in keys:
        err = amax(r32[k].double() - r64[k])
        diff, tol = amax(got[k].double() - r64[k]), 4 * err + 1.2e-7 * amax(r64[k])
        print(f"{tag} {k}: fused-vs-f64 {diff:.3e} tol {tol:.3e} (float32 composition's own {err:.3e})")
        if not diff <= tol:
            bad.append((k, diff, tol))
    assert not bad, (tag, bad)
