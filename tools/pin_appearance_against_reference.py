#!/usr/bin/env python
"""Writes tests/golden/appearance_ref.npz: the per-Gaussian appearance MLP as the REFERENCE evaluates it on the CPU
(examples/utils.py: AppearanceOptModule), forward and backward, for tests/test_appearance.py and tests/test_gpu_appearance.py,
which run without a reference checkout. Checks gsplat_amd's torch composition against it on the way. TEST INFRASTRUCTURE; needs
a checkout of the reference (its examples/utils.py imports sklearn and matplotlib).

Two modules of 4 images, 32 features, module sh_degree 3, width 64, depth 2: `m16` (embed_dim 16) and `m0` (embed_dim 0), seeded
and perturbed so that every bias and embedding is non-zero; their state_dicts are stored as {m}_sd_{key}.

Cases (`cases` = JSON list of {name, module, N, C, ids (or null), sh_degree, dropped, drawn}); the fused kernel's row tile is 32
Gaussians per wave, four waves per workgroup:
  a  N 1     C 1  embed_ids None     degree 3  m16
  b  N 33    C 1  ids given          degree 0  m16   one tile plus one
  c  N 129   C 2  ids (2, 0)         degree 2  m16   one workgroup plus one
  d  N 2100  C 3  ids given          degree 3  m16   one dirs row exactly zero and one of length 1e-20 (the normalise clamp)
  e  N 200   C 2  ids given          degree 3  m0
  f  N 31    C 1  ids given          degree 3  m16   one tile minus one
  g  N 127   C 2  ids given          degree 1  m16   one workgroup minus one
Per case: {name}_features, _dirs, _w, and under the loss sum(colors * w): _colors, _v_features, _v_dirs, _v_embeds and
_v_{parameter} for every color_head parameter. Everything is evaluated a second time in float64 from the same float32 inputs;
{name}_err_{output} = max |float32 reference - float64 reference| is the reference's own spread, from which the tests take their
tolerance. The two rows of case d that take the normalise clamp have v_dirs = v_unit / 1e-12, twelve orders above the others:
{name}_clamp [C, N] flags them, _v_dirs holds zeros there, and their values and spread are _v_dirs_clamp / _err_v_dirs_clamp.

ReLU kinks: a pre-activation within rounding of zero flips a whole row's contribution to the summed weight gradients. Each case
is drawn with spare rows, and every Gaussian for which any float64 pre-activation of either hidden layer, in any camera, has
|z| < TAU = 1e-4 is dropped (N above is after dropping). The tool asserts that at most 10 % are dropped and that the float32
reference's largest pre-activation error is at most TAU / 10. Features and weights of the loss take few distinct values so that
the archive stays small.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_appearance_against_reference.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("GSPLAT_REFERENCE_PATH"):
    raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (examples/utils.py)")
REF = os.environ["GSPLAT_REFERENCE_PATH"]
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "examples"))

TAU = 1e-4
N_IMAGES, FEATURE_DIM = 4, 32


def amax(t):
    """max |t|, 0 for an empty tensor (the embeddings of embed_dim 0)."""
    return float(t.abs().max()) if t.numel() else 0.0


def make_module(ref_utils, embed_dim, g):
    torch.manual_seed(5 + embed_dim)
    m = ref_utils.AppearanceOptModule(N_IMAGES, FEATURE_DIM, embed_dim=embed_dim, sh_degree=3)
    with torch.no_grad():
        for p in m.parameters():
            p += torch.randint(1, 5, p.shape, generator=g).float() / 64.0  # nothing stays zero
    return m


def outputs(colors, f, d, m):
    """Every stored output after the backward pass; a gradient that autograd left out (dirs at degree 0, the embeddings with
    embed_ids=None) is zero."""
    out = {"colors": colors.detach(), "v_features": f.grad, "v_dirs": d.grad if d.grad is not None else torch.zeros_like(d),
           "v_embeds": m.embeds.weight.grad if m.embeds.weight.grad is not None else torch.zeros_like(m.embeds.weight)}
    for k, p in m.color_head.named_parameters():
        out["v_" + k] = p.grad
    return out


def run(module_cls, sd, embed_dim, features, ids, dirs, w, degree, dtype):
    """colors, the hidden pre-activations and every gradient under sum(colors * w), in `dtype` (made the default dtype for the
    call: the reference allocates its zero embeddings and its SH bases in the default one)."""
    torch.set_default_dtype(dtype)
    try:
        return _run(module_cls, sd, embed_dim, features, ids, dirs, w, degree, dtype)
    finally:
        torch.set_default_dtype(torch.float32)


def _run(module_cls, sd, embed_dim, features, ids, dirs, w, degree, dtype):
    m = module_cls(N_IMAGES, FEATURE_DIM, embed_dim=embed_dim, sh_degree=3).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    pre = []
    hooks = [m.color_head[i].register_forward_hook(lambda _m, _i, o: pre.append(o.detach().clone())) for i in (0, 2)]
    f = features.to(dtype).clone().requires_grad_(True)
    d = dirs.to(dtype).clone().requires_grad_(True)
    colors = m(f, ids, d, degree)
    (colors * w.to(dtype)).sum().backward()
    for hk in hooks:
        hk.remove()
    return outputs(colors, f, d, m), pre


def main():
    import utils as ref_utils  # the reference's examples/utils.py

    from gsplat_amd import appearance as ours

    g = torch.Generator().manual_seed(23)
    modules = {"m16": (16, make_module(ref_utils, 16, g)), "m0": (0, make_module(ref_utils, 0, g))}
    specs = (
        ("a", "m16", 1, 1, None, 3),
        ("b", "m16", 33, 1, (1,), 0),
        ("c", "m16", 129, 2, (2, 0), 2),
        ("d", "m16", 2100, 3, (3, 1, 2), 3),
        ("e", "m0", 200, 2, (0, 1), 3),
        ("f", "m16", 31, 1, (3,), 3),
        ("g", "m16", 127, 2, (1, 1), 1),
    )
    out, cases = {}, []
    for mname, (E, m) in modules.items():
        for k, v in m.state_dict().items():
            out[f"{mname}_sd_{k}"] = v.detach().numpy()
    for name, mname, N, C, ids, degree in specs:
        E, m = modules[mname]
        sd = m.state_dict()
        ids_t = None if ids is None else torch.tensor(ids, dtype=torch.int64)
        drawn = N + N // 4 + 40  # spare rows: the share dropped is 3-5 % by the count of 128 units per row and camera
        features = torch.randint(-32, 33, (drawn, FEATURE_DIM), generator=g).float() / 32.0
        dirs = torch.randn(C, drawn, 3, generator=g) * 2.0
        if name == "d":
            dirs[0, 5] = 0.0
            dirs[1, 7] = torch.tensor([6e-21, -8e-21, 0.0])  # length 1e-20
        w_all = torch.randint(-4, 5, (C, drawn, 3), generator=g).float() / 4.0
        # drop the Gaussians next to a ReLU kink (float64 pre-activations of both hidden layers, every camera)
        _, pre64 = run(ref_utils.AppearanceOptModule, sd, E, features, ids_t, dirs, w_all, degree, torch.float64)
        near = torch.zeros(drawn, dtype=torch.bool)
        for z in pre64:
            near |= (z.abs() < TAU).any(dim=-1).any(dim=0)
        share = float(near.float().mean())
        assert share <= 0.10, (name, share)
        keep = torch.nonzero(~near).flatten()
        assert keep.numel() >= N, (name, keep.numel())
        keep = keep[:N]
        if name == "d":
            assert 5 in keep.tolist() and 7 in keep.tolist(), "the clamp rows were dropped"
        features, dirs, w = features[keep].contiguous(), dirs[:, keep].contiguous(), w_all[:, keep].contiguous()
        r32, pre32 = run(ref_utils.AppearanceOptModule, sd, E, features, ids_t, dirs, w, degree, torch.float32)
        r64, pre64 = run(ref_utils.AppearanceOptModule, sd, E, features, ids_t, dirs, w, degree, torch.float64)
        pre_err = max(float((a.double() - b).abs().max()) for a, b in zip(pre32, pre64))
        assert pre_err <= TAU / 10, (name, pre_err)
        assert min(float(z.abs().min()) for z in pre64) >= TAU
        err = {k: amax(r32[k].double() - r64[k]) for k in r32}
        # our torch composition against the reference, same inputs
        mine = ours.AppearanceOptModule(N_IMAGES, FEATURE_DIM, embed_dim=E, sh_degree=3)
        mine.load_state_dict(sd, strict=True)
        f = features.clone().requires_grad_(True)
        d = dirs.clone().requires_grad_(True)
        colors = ours.appearance_torch(mine, f, ids_t, d, degree)
        (colors * w).sum().backward()
        got = outputs(colors, f, d, mine)
        # rows that take the normalise clamp have v_dirs = v_unit / 1e-12: they are compared among themselves
        clamp = dirs.double().norm(dim=-1) < 1e-12
        if bool(clamp.any()):
            for res in (r32, r64, got):
                res["v_dirs_clamp"], res["v_dirs"] = res["v_dirs"][clamp], res["v_dirs"] * (~clamp)[..., None]
            err = {k: amax(r32[k].double() - r64[k]) for k in r32}
            out[f"{name}_clamp"] = clamp.numpy()
        for k in r32:
            dlt = amax(got[k] - r32[k])
            assert dlt <= 4 * err[k] + 1.2e-7 * amax(r32[k]), (name, k, dlt, err[k])
        out.update({f"{name}_features": features.numpy(), f"{name}_dirs": dirs.numpy(), f"{name}_w": w.numpy()})
        for k in r32:
            out[f"{name}_{k}"] = r32[k].numpy()
            out[f"{name}_err_{k}"] = np.float64(err[k])
        cases.append({"name": name, "module": mname, "N": N, "C": C, "ids": None if ids is None else list(ids),
                      "sh_degree": degree, "dropped": int(near.sum()), "drawn": drawn})
        print(f"{name}: dropped {int(near.sum())} of {drawn} ({share:.1%}); pre-activation err {pre_err:.2e}; err "
              + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    out["cases"] = np.array(json.dumps(cases))
    out["tau"] = np.float64(TAU)
    path = os.path.join(ROOT, "tests", "golden", "appearance_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print("APPEARANCE PINNED ->", path, size, "bytes")


if __name__ == "__main__":
    main()
