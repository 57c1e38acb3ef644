"""The cases of tests/golden/appearance_ref.npz (tools/pin_appearance_against_reference.py) for test_appearance.py and
test_gpu_appearance.py: loading, running a module on a case, and the comparison rule."""
import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "appearance_ref.npz")
PARAMS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")
OUTPUTS = ("colors", "v_features", "v_dirs", "v_embeds") + tuple("v_" + p for p in PARAMS)
SUMMED = ("v_embeds",) + tuple("v_" + p for p in PARAMS)  # sums over all rows


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def cases():
    return json.loads(str(golden()["cases"]))


def case_names():
    return [c["name"] for c in cases()]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def state_dict(mname):
    pre = mname + "_sd_"
    return {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in golden().items() if k.startswith(pre)}


def make_module(mname, device="cpu", dtype=torch.float32):
    from gsplat_amd.appearance import AppearanceOptModule

    sd = state_dict(mname)
    m = AppearanceOptModule(sd["embeds.weight"].shape[0], 32, embed_dim=sd["embeds.weight"].shape[1], sh_degree=3)
    m.load_state_dict(sd, strict=True)
    return m.to(device=device, dtype=dtype)


def run_case(name, fn, device="cpu", dtype=torch.float32):
    """Every output of OUTPUTS for `fn(module, features, ids, dirs, degree)` on a case, under the loss sum(colors * w)."""
    c, z = case(name), golden()
    m = make_module(c["module"], device, dtype)
    f = torch.from_numpy(z[name + "_features"]).to(device=device, dtype=dtype).requires_grad_(True)
    d = torch.from_numpy(z[name + "_dirs"]).to(device=device, dtype=dtype).requires_grad_(True)
    w = torch.from_numpy(z[name + "_w"]).to(device=device, dtype=dtype)
    ids = None if c["ids"] is None else torch.tensor(c["ids"], dtype=torch.int64, device=device)
    colors = fn(m, f, ids, d, c["sh_degree"])
    (colors * w).sum().backward()
    out = {"colors": colors.detach(), "v_features": f.grad, "v_dirs": d.grad if d.grad is not None else torch.zeros_like(d),
           "v_embeds": m.embeds.weight.grad if m.embeds.weight.grad is not None else torch.zeros_like(m.embeds.weight)}
    for p in PARAMS:
        out["v_" + p] = m.color_head.get_parameter(p).grad
    return {k: v.detach().cpu() for k, v in out.items()}


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def check_case(name, got, factor=4.0, factor_summed=None):
    """|got - reference| <= factor * err + 1.2e-7 * max |reference| for every output, err the float32 reference's own distance
    from its float64 evaluation. Prints each figure before it asserts."""
    z, bad = golden(), []
    keys = list(OUTPUTS)
    if f"{name}_clamp" in z:  # rows under the normalise clamp (v_dirs ~ 1e12) are compared among themselves
        clamp = torch.from_numpy(z[f"{name}_clamp"])
        got = dict(got, v_dirs_clamp=got["v_dirs"][clamp], v_dirs=got["v_dirs"] * (~clamp)[..., None])
        keys.append("v_dirs_clamp")
    for k in keys:
        ref, err = torch.from_numpy(z[f"{name}_{k}"]), float(z[f"{name}_err_{k}"])
        fac = factor_summed if (factor_summed is not None and k in SUMMED) else factor
        d, tol = amax(got[k].to(torch.float64) - ref.to(torch.float64)), fac * err + 1.2e-7 * amax(ref)
        print(f"{name} {k}: diff {d:.3e} tol {tol:.3e} (err {err:.3e}, max|ref| {amax(ref):.3e})")
        if not d <= tol:
            bad.append((k, d, tol))
    assert not bad, (name, bad)
