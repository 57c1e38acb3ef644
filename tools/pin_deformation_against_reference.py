#!/usr/bin/env python
"""Writes tests/golden/deformation_ref.npz: the deformation network as the REFERENCE evaluates it on the CPU
(gsplat/contrib/dynamic/deformation.py: DeformNetwork, DeformationTable), forward and backward, for tests/test_deformation.py and
tests/test_gpu_deformation.py, which run without a reference checkout. Checks gsplat_amd's torch composition against it on the
way. TEST INFRASTRUCTURE; needs a checkout of the reference. The reference's file is loaded by path: `import gsplat` would pull
in its CUDA backend.

Two modules of 64 features, width 64, three hidden layers: `d3`, seeded, with head weights and biases drawn uniform in +-0.125
(with the zero heads of a fresh module the backward would test nothing), stored as d3_sd_{key}; and `z3`, a fresh module with
its zero heads untouched that takes d3's trunk (not stored a second time: tests build it the same way).

Cases (`cases` = JSON list of {name, module, N, dropped, drawn}); the fused kernel's row tile is 32 Gaussians per wave, four
waves per workgroup:
  a  N 1     d3  a single row
  b  N 31    d3  one tile minus one
  c  N 33    d3  one tile plus one
  d  N 127   d3  one workgroup minus one
  e  N 129   d3  one workgroup plus one
  f  N 2100  d3  more tiles than one pass of a small grid
  g  N 200   z3  zero heads
  h  N 200   d3  only w_means non-zero
Per case: {name}_means, _quats, _opacities, _plane_features, the loss weights _w_means, _w_quats, _w_opac, and under the loss
sum(means_new * w_means) + sum(quats_new * w_quats) + sum(opacities_new * w_opac): _means_new, _quats_new, _opacities_new,
_v_means, _v_quats, _v_opacities, _v_plane_features and _v_{parameter} for all twelve parameters. Everything is evaluated a
second time in float64 from the same float32 inputs; {name}_err_{output} = max |float32 reference - float64 reference| is the
reference's own spread, from which the tests take their tolerance. The float64 values themselves are not kept: they would double
an archive that has to stay under the size limit of a committed file (1 MiB). For the same reason every array above 256 KiB -
case f's plane_features and v_plane_features - goes to a second archive next to the first, tests/golden/deformation_ref_rows.npz; the tests read
the two as one.

ReLU kinks: a pre-activation within rounding of zero flips a whole row's contribution to the summed weight gradients. Each case
is drawn with spare rows, and every row for which any float64 pre-activation of the three hidden layers has |z| < TAU = 2e-5 is
dropped (N above is after dropping). The tool asserts that at most 5 % are dropped (the third layer's pre-activations are small:
at 1e-4 the share would be near 10 %) and that the float32 reference's largest pre-activation error is at most TAU / 10. Inputs
and weights of the loss take few distinct values so that the archive stays small.

DeformationTable: `table_ops` (JSON) is a list of [method, arguments] applied in order to tables of `table_n` Gaussians, each
split factor on a copy of the table after the earlier steps; table_mask_{i} is the reference's mask after step i.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_deformation_against_reference.py"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("GSPLAT_REFERENCE_PATH"):
    raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (gsplat/contrib/dynamic/deformation.py)")
REF = os.environ["GSPLAT_REFERENCE_PATH"]

TAU = 2e-5
FEATURE_DIM = 64
OUT = ("means_new", "quats_new", "opacities_new")
TABLE_N = 12
TABLE_OPS = (
    ("set_indices", {"indices": [1, 4, 7, 10]}),
    ("set_indices", {"indices": [4], "value": False}),
    ("prune", {"keep_mask": [1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1]}),
    ("duplicate", {"indices": [0, 1, 5, 8]}),
    ("split", {"indices": [1, 2, 8], "factor": 1}),
    ("split", {"indices": [1, 2, 8], "factor": 2}),
    ("split", {"indices": [1, 2, 8], "factor": 3}),
)


def load_reference():
    path = os.path.join(REF, "gsplat", "contrib", "dynamic", "deformation.py")
    spec = importlib.util.spec_from_file_location("reference_deformation", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def make_modules(ref, g):
    torch.manual_seed(11)
    d3, z3 = ref.DeformNetwork(FEATURE_DIM), ref.DeformNetwork(FEATURE_DIM)
    z3.trunk.load_state_dict(d3.trunk.state_dict())
    with torch.no_grad():
        for head in (d3.pos_head, d3.quat_head, d3.opacity_head):
            for p in head.parameters():
                p.copy_((torch.rand(p.shape, generator=g) * 2.0 - 1.0) * 0.125)
    assert all(float(p.abs().max()) == 0.0 for h in (z3.pos_head, z3.quat_head, z3.opacity_head) for p in h.parameters())
    return {"d3": d3, "z3": z3}


def run(module_cls, sd, inputs, weights, dtype):
    """The three outputs, the hidden pre-activations and every gradient under the weighted sum, in `dtype`."""
    m = module_cls(FEATURE_DIM).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    pre = []
    hooks = [m.trunk[i].register_forward_hook(lambda _m, _i, o: pre.append(o.detach().clone())) for i in (0, 2, 4)]
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in inputs]
    means, quats, opac, x = leaves
    outs = m(means, quats, opac, torch.zeros(means.shape[0], 1, dtype=dtype), x)
    sum((o * w.to(dtype)).sum() for o, w in zip(outs, weights)).backward()
    for hk in hooks:
        hk.remove()
    res = {k: o.detach() for k, o in zip(OUT, outs)}
    res.update({"v_means": means.grad, "v_quats": quats.grad, "v_opacities": opac.grad, "v_plane_features": x.grad})
    for k, p in m.named_parameters():
        res["v_" + k] = p.grad
    return res, pre


def pin_table(ref, out):
    tables = []
    t = ref.DeformationTable(TABLE_N)
    for i, (op, kw) in enumerate(TABLE_OPS):
        if op == "split":  # every factor on a copy of the table as the steps before the splits left it
            t = ref.DeformationTable(0)
            t.mask = base.clone()
        args = {k: (torch.tensor(v, dtype=torch.bool) if k == "keep_mask" else torch.tensor(v) if isinstance(v, list) else v)
                for k, v in kw.items()}
        getattr(t, op)(**args)
        if op != "split":
            base = t.mask.clone()
        out[f"table_mask_{i}"] = t.mask.numpy().copy()
        tables.append(int(t.mask.sum()))
    out["table_ops"] = np.array(json.dumps([[op, kw] for op, kw in TABLE_OPS]))
    out["table_n"] = np.int64(TABLE_N)
    print("table: dynamic counts after each step", tables)


def main():
    ref = load_reference()
    from gsplat_amd import deformation as ours

    g = torch.Generator().manual_seed(29)
    modules = make_modules(ref, g)
    specs = (("a", "d3", 1), ("b", "d3", 31), ("c", "d3", 33), ("d", "d3", 127), ("e", "d3", 129), ("f", "d3", 2100),
             ("g", "z3", 200), ("h", "d3", 200))
    out, cases = {}, []
    for k, v in modules["d3"].state_dict().items():
        out[f"d3_sd_{k}"] = v.detach().numpy()
    for name, mname, N in specs:
        sd = modules[mname].state_dict()
        drawn = N + N // 4 + 40  # spare rows
        dims = (3, 4, 1, FEATURE_DIM)
        inputs = [torch.randint(-32, 33, (drawn, d), generator=g).float() / 32.0 for d in dims]
        weights = [torch.randint(-4, 5, (drawn, d), generator=g).float() / 4.0 for d in dims[:3]]
        if name == "h":
            weights[1].zero_()
            weights[2].zero_()
        # drop the rows next to a ReLU kink (float64 pre-activations of the three hidden layers)
        _, pre64 = run(ref.DeformNetwork, sd, inputs, weights, torch.float64)
        near = torch.zeros(drawn, dtype=torch.bool)
        for z in pre64:
            near |= (z.abs() < TAU).any(dim=-1)
        share = float(near.float().mean())
        assert share <= 0.05, (name, share)
        keep = torch.nonzero(~near).flatten()
        assert keep.numel() >= N, (name, keep.numel())
        keep = keep[:N]
        inputs = [t[keep].contiguous() for t in inputs]
        weights = [t[keep].contiguous() for t in weights]
        r32, pre32 = run(ref.DeformNetwork, sd, inputs, weights, torch.float32)
        r64, pre64 = run(ref.DeformNetwork, sd, inputs, weights, torch.float64)
        pre_err = max(float((a.double() - b).abs().max()) for a, b in zip(pre32, pre64))
        assert pre_err <= TAU / 10, (name, pre_err)
        assert min(float(z.abs().min()) for z in pre64) >= TAU
        err = {k: amax(r32[k].double() - r64[k]) for k in r32}
        # our torch composition against the reference, same inputs
        got, _ = run(ours.DeformNetwork, sd, inputs, weights, torch.float32)
        for k in r32:
            dlt = amax(got[k] - r32[k])
            assert dlt <= 4 * err[k] + 1.2e-7 * amax(r32[k]), (name, k, dlt, err[k])
        for key, t in zip(("means", "quats", "opacities", "plane_features", "w_means", "w_quats", "w_opac"), inputs + weights):
            out[f"{name}_{key}"] = t.numpy()
        for k in r32:
            out[f"{name}_{k}"] = r32[k].numpy()
            out[f"{name}_err_{k}"] = np.float64(err[k])
        cases.append({"name": name, "module": mname, "N": N, "dropped": int(near.sum()), "drawn": drawn})
        print(f"{name}: dropped {int(near.sum())} of {drawn} ({share:.1%}); pre-activation err {pre_err:.2e}; err "
              + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    pin_table(ref, out)
    out["cases"] = np.array(json.dumps(cases))
    out["tau"] = np.float64(TAU)
    rows = {k: v for k, v in out.items() if v.nbytes > 256 * 1024}
    for tag, part in (("", {k: v for k, v in out.items() if k not in rows}), ("_rows", rows)):
        path = os.path.join(ROOT, "tests", "golden", f"deformation_ref{tag}.npz")
        np.savez_compressed(path, **part)
        size = os.path.getsize(path)
        assert size < 1_000_000, (path, size)
        print("DEFORMATION PINNED ->", path, size, "bytes", sorted(part) if tag else "")


if __name__ == "__main__":
    main()
