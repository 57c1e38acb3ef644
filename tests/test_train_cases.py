"""CPU tests of tests/_train_cases.py: the float64 references and per-element bounds that tests/test_gpu_train_kernels.py holds
the kernels of csrc/optim.hip to. A correct float32 implementation must pass them - the float32 torch restatements (the oracle's
adam_step and mcmc_perturb, a float32 evaluation of the relocation double loop and of the statistics sums, the strategy's own
tensor-op form) lie inside every bound on every case - and they must discriminate: one deliberately wrong restatement per family
falls outside on at least one case. Also: the regime table of the Adam host rule covers both kernels and every listed block edge,
and the relocation grid meets its condition. Runs without a GPU."""
import numpy as np
import pytest
import torch

import _train_cases as tc
from oracle import oracle as O


def _hyper32(case):
    """The scalars as the kernel receives them (float32): a float32 restatement that formed 1 - b2 from the float64 0.999 would
    be 1.3e-5 away from what the kernel computes."""
    return tuple(tc.f32(case[k]) for k in ("lr", "b1", "b2", "eps"))


# ---- Adam ------------------------------------------------------------------------------------------------------------------
def _oracle_adam(p, g, m, v, valid, *hyper):
    """oracle.adam_step; a 0-dim parameter is one row of one element, as the op treats it."""
    if p.dim() == 0:
        return tuple(t.reshape(()) for t in O.adam_step(*(t.reshape(1) for t in (p, g, m, v)), valid, *hyper))
    return O.adam_step(p, g, m, v, valid, *hyper)


def _adam_run(step):
    worst = {}
    for c in tc.ADAM_CASES:
        cs = tc.adam_case(c.name)
        hyper = _hyper32(cs)
        p, m, v = step(cs["p"], cs["g"], cs["m"], cs["v"], cs["valid"], *hyper)
        refs = tc.adam_ref(cs["p"], cs["g"], cs["m"], cs["v"], cs["valid"], *hyper)
        sel = tc._row_select(cs["valid"], cs["p"])
        worst[c.name] = max(tc.ratio(out[sel], ref[sel], tol[sel]) for out, ref, tol in zip((p, m, v), refs[:3], refs[3:]))
    return worst


def test_adam_float32_restatement_is_inside_every_bound():
    worst = 0.0
    for c in tc.ADAM_CASES:
        cs = tc.adam_case(c.name)
        hyper = _hyper32(cs)
        p, m, v = _oracle_adam(cs["p"], cs["g"], cs["m"], cs["v"], cs["valid"], *hyper)
        r = tc.adam_check(p, m, v, (cs["p"], cs["g"], cs["m"], cs["v"]), cs["valid"], cs["never"], hyper)
        assert r <= 1.0, (c.name, r)
        worst = max(worst, r)
    print(f"adam float32 restatement: worst error / bound {worst:.3f} over {len(tc.ADAM_CASES)} cases")


def _adam_wrong(kind):
    def step(p, g, m, v, valid, lr, b1, b2, eps):
        m2 = b1 * m + (1.0 - b1) * g
        v2 = b2 * v + (1.0 - b2) * g * g
        den = torch.sqrt(v2) if kind == "no-eps" else v2 + eps
        return p - lr * m2 / den, m2, v2
    return step


@pytest.mark.parametrize("kind", ["no-eps", "v-for-sqrt-v"])
def test_adam_bounds_catch_a_wrong_denominator(kind):
    worst = _adam_run(_adam_wrong(kind))
    caught = [n for n, r in worst.items() if not r <= 1.0]
    assert caught, f"Adam with {kind} passes every case"
    if kind == "no-eps":  # the eps-dominated hyperparameter set catches it by orders of magnitude
        assert any(tc.ADAM_BY_NAME[n].hyper == 2 and worst[n] > 1e3 for n in caught)


def test_adam_cases_cover_both_kernels_and_every_block_edge():
    vec_items, scalar_items, widths = set(), set(), set()
    for c in tc.ADAM_CASES:
        n_rows, D = tc.adam_rows_width(c.shape)
        widths.add(D)
        ptrs = [4 if off else 0 for off in c.misalign]  # what tc.place() produces: the allocation's start, or 4 bytes in
        vec4 = tc.adam_takes_vec4(D, ptrs)
        if any(c.misalign):
            assert D % 4 == 0 and not vec4, c.name  # the same data, forced onto the scalar kernel
        (vec_items if vec4 else scalar_items).add(tc.adam_launch_items(c.shape, vec4))
    assert widths >= set(tc.ADAM_WIDTHS) | {0}
    assert vec_items >= {1, 255, 256, 257, 252, 264, 258}, sorted(vec_items)
    assert 0 in vec_items | scalar_items  # no rows: nothing is launched
    assert scalar_items >= {1, 255, 256, 257, 258, 260, 270, 1025}, sorted(scalar_items)
    assert scalar_items >= {257 * 4, 129 * 8, 22 * 48}  # the misaligned twins of the vector cases
    for D in (4, 8, 48):
        for mis in tc.ADAM_MISALIGN[1:]:
            assert any(c.misalign == mis and tc.adam_rows_width(c.shape)[1] == D for c in tc.ADAM_CASES), (D, mis)
    assert {c.mask for c in tc.ADAM_CASES} == set(tc.ADAM_MASKS)
    assert {c.hyper for c in tc.ADAM_CASES} == {0, 1, 2}
    assert not tc.adam_takes_vec4(4, (0, 0, 8, 0)) and not tc.adam_takes_vec4(6, (0, 0, 0, 0)) and tc.adam_takes_vec4(48, (16, 32, 0, 64))


def test_adam_cases_hold_what_they_claim():
    for c in tc.ADAM_CASES:
        cs = tc.adam_case(c.name)
        sel = tc._row_select(cs["valid"], cs["p"])
        for k in "pgmv":
            assert cs[k].dtype == torch.float32 and bool(torch.isfinite(cs[k][sel]).all()), c.name
        if cs["valid"] is not None and cs["p"].numel() and not bool(cs["valid"].all()):
            assert all(not bool(torch.isfinite(cs[k][~sel]).all()) or cs[k][~sel].abs().max() > 1e29 for k in "pgmv"), c.name
        if cs["n_rows"] >= 3 and cs["p"].dim() > 0:
            rows = cs["never"] if cs["valid"] is None else cs["never"] & cs["valid"]
            assert bool(cs["never"].any()) and all(bool((cs[k][rows] == 0).all()) for k in "gmv")
            assert bool((cs["p"][rows] != 0).all())
    assert tc.strided_bool(torch.rand(50) < 0.5, "cpu").is_contiguous() is False


# ---- relocation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_opacity", tc.RELOC_MIN_OPACITIES)
def test_relocation_float32_loop_is_inside_the_bounds_and_the_grid_meets_its_condition(min_opacity):
    o, scales, ratios = tc.relocation_grid()
    assert len(o) >= tc.RELOC_MIN_ROWS and len(o) % (len(tc.RELOC_OPACITIES) * len(tc.RELOC_RATIOS)) == 0
    new_o, new_s = tc.relocation_f32(o, scales, ratios, tc.binoms(), min_opacity)
    r_o, r_s, ref = tc.relocation_check(o, scales, ratios, tc.binoms(), min_opacity, new_o, new_s)
    print(f"relocation float32 loop, min_opacity {min_opacity}: opacity {r_o:.3f}, scale {r_s:.3f} of the bound")
    assert r_o <= 1.0 and r_s <= 1.0
    # the condition: every row is value-checked under a bound below 2e-2; the largest is at opacity 0.999, ratio 51
    assert np.isfinite(ref["rel"]).all() and ref["rel"].max() < tc.RELOC_MAX_BOUND
    top = int(ref["rel"].argmax())
    assert float(o[top]) == pytest.approx(0.999) and int(ratios[top]) == 51
    assert ref["rel"][top] == pytest.approx(9.8e-3, rel=0.05) and ref["kappa"][top] == pytest.approx(115, rel=0.05)
    # ratio 1: the Gaussian is kept (coefficient o / o')
    one = ratios.numpy() == 1
    assert np.allclose(ref["coeff"][one] * new_o.double().numpy()[one], o.double().numpy()[one], rtol=1e-12)


def test_relocation_bounds_catch_a_clamp_after_the_scale():
    o, scales, ratios = tc.relocation_grid()
    new_o, new_s = tc.relocation_f32(o, scales, ratios, tc.binoms(), 0.005, clamp_first=False)
    r_o, r_s, _ = tc.relocation_check(o, scales, ratios, tc.binoms(), 0.005, new_o, new_s)
    assert r_o <= 1.0 and not r_s <= 1.0  # the opacities are right, the scales of the clamped rows are not
    # with nothing to clamp the two orders agree
    hi = o >= 0.3
    new_o, new_s = tc.relocation_f32(o[hi], scales[hi], ratios[hi], tc.binoms(), 0.0, clamp_first=False)
    assert tc.relocation_check(o[hi], scales[hi], ratios[hi], tc.binoms(), 0.0, new_o, new_s)[1] <= 1.0


def test_relocation_small_table_and_corners():
    o, scales, ratios, table = tc.relocation_small()
    assert table.shape == (12, 12) and table.is_contiguous() and set(ratios.tolist()) == set(tc.RELOC_SMALL_RATIOS)
    new_o, new_s = tc.relocation_f32(o, scales, ratios, table, 0.005)
    r_o, r_s, ref = tc.relocation_check(o, scales, ratios, table, 0.005, new_o, new_s)
    assert r_o <= 1.0 and r_s <= 1.0 and set(ref["n"].tolist()) == {1, 12}
    o, scales, ratios = tc.relocation_corners()
    new_o, new_s = tc.relocation_f32(o, scales, ratios, tc.binoms(), 0.005)
    r_o, _, ref = tc.relocation_check(o, scales, ratios, tc.binoms(), 0.005, new_o, new_s)
    assert r_o <= 1.0
    assert bool((new_o[ratios == 1] == np.float32(tc.RELOC_UPPER)).all())
    assert ref["kappa"][(ratios == 51).numpy() & (new_o.numpy() > 0.9)].min() > 3e4  # why nothing is said about those scales


# ---- SGLD perturb ----------------------------------------------------------------------------------------------------------
def _perturb_wrong(pos, quats, log_scales, logits, noise, noise_scale, t, k):
    R = O.quat_to_rotmat(quats)
    covars = R.transpose(-1, -2) @ torch.diag_embed(torch.exp(log_scales) ** 2) @ R  # R^T S^2 R
    w = torch.sigmoid(-float(k) * (torch.sigmoid(logits) - float(t))) * noise_scale
    return pos + torch.einsum("bij,bj->bi", covars, noise * w[:, None])


@pytest.mark.parametrize("n", tc.PERTURB_ROWS)
def test_perturb_float32_restatement_is_inside_the_bound(n):
    cs = tc.perturb_case(n)
    args = (cs["pos"], cs["quats"], cs["log_scales"], cs["logits"], cs["noise"])
    assert bool((cs["pos"] != 0).all())
    caught = False
    for ns, t, k in tc.PERTURB_PARAMS + (tc.PERTURB_ZERO_SCALE,):
        ns32, t32, k32 = tc.f32(ns), tc.f32(t), tc.f32(k)
        ref, tol, w = tc.perturb_ref(*args, ns, t, k)
        out = O.mcmc_perturb(*args, ns32, t32, k32)
        r = tc.ratio(out, ref, tol)
        print(f"perturb float32 restatement, {n} rows, {(ns, t, k)}: {r:.3f} of the bound")
        assert r <= 1.0
        if ns == 0.0:
            assert tc.bits_equal(out, cs["pos"])
        elif n >= 255:
            if tc.perturb_w_is_zero(t, k):
                assert tc.bits_equal(out[cs["hi"]], cs["pos"][cs["hi"]])
            lo_w = ns32 / (1.0 + np.exp(-k32 * t32))
            assert torch.allclose(w[cs["lo"]], torch.full_like(w[cs["lo"]], lo_w), rtol=1e-9)
            assert int(cs["hi"].sum()) == 2 and bool(cs["hi"][-1]) and int(cs["lo"].sum()) == 1
            caught = caught or not tc.ratio(_perturb_wrong(*args, ns32, t32, k32), ref, tol) <= 1.0
    assert caught or n < 255, "R^T S^2 R passes every parameter set"
    assert tc.perturb_w_is_zero(0.005, 100.0) and not tc.perturb_w_is_zero(0.25, 8.0)


# ---- statistics ------------------------------------------------------------------------------------------------------------
def _accumulate_f32(grad, radii, state, half_w, half_h, max_dim, select=True):
    """The kernel's loop in float32: views in ascending order. `select=False` multiplies by the visibility instead."""
    C, N = radii.shape[:2]
    hw, hh, inv = np.float32(half_w), np.float32(half_h), np.float32(1.0 / max_dim)
    total = torch.zeros(N)
    count = torch.zeros(N)
    rmax = torch.zeros(N)
    for c in range(C):
        seen = (radii[c] > 0).all(dim=-1)
        gx, gy = grad[c, :, 0] * float(hw), grad[c, :, 1] * float(hh)
        norm = torch.sqrt(gx * gx + gy * gy)
        total = total + (torch.where(seen, norm, torch.zeros(())) if select else norm * seen.float())
        count = count + seen.float()
        rmax = torch.maximum(rmax, torch.where(seen, radii[c].amax(dim=-1).float() * float(inv), torch.zeros(())))
    out = dict(grad2d=state["grad2d"] + total, count=state["count"] + count)
    if state.get("radii") is not None:
        out["radii"] = torch.maximum(state["radii"], rmax)
    return out


def _accumulate_strategy_cpu(case, inp, state):
    """DefaultStrategy._accumulate on CPU tensors: the tensor-op form that every refused input falls back to."""
    from gsplat_amd.strategy import DefaultStrategy

    strat = DefaultStrategy(refine_scale2d_stop_iter=100 if case.track else 0, absgrad=case.absgrad, verbose=False)
    st = {k: v.clone() for k, v in state.items()}
    info = tc.accumulate_info(tc.accumulate_layout(inp["grad"], case.layout, "cpu"), inp["radii"], case.C, case.absgrad)
    strat._accumulate({"means": torch.zeros(case.N, 3)}, st, info, packed=False)
    return st


def test_statistics_float32_restatements_are_inside_the_bounds_and_a_product_is_caught():
    assert {c.N for c in tc.ACC_CASES} == set(tc.ACC_N) and {c.C for c in tc.ACC_CASES} == set(tc.ACC_C)
    assert {(c.layout, c.absgrad) for c in tc.ACC_CASES} == {(l, a) for l in tc.ACC_LAYOUTS for a in (False, True)}
    worst, caught = 0.0, 0
    for case in tc.ACC_CASES:
        inp = tc.accumulate_inputs(case.N, case.C)
        hidden = ~(inp["radii"] > 0).all(dim=-1)
        pats = {tuple(p) for p in inp["radii"][hidden].tolist()}
        if case.N >= 255:
            assert pats == set(tc.ACC_HIDDEN) and not bool(torch.isfinite(inp["grad"][hidden]).any())
            assert case.C < 2 or bool(hidden[1].all())
        scal = tc.accumulate_scalars(case.C)
        state = inp["state"]
        ref = tc.accumulate_ref(inp["grad"], inp["radii"], state if case.track else {k: state[k] for k in ("grad2d", "count")}, *scal)
        assert (ref["radii"] is None) == (not case.track)
        for got in (_accumulate_f32(inp["grad"], inp["radii"], state if case.track else dict(state, radii=None), *scal),
                    _accumulate_strategy_cpu(case, inp, state)):
            r = tc.accumulate_check(got, ref)
            assert r <= 1.0, (case.name, r)
            worst = max(worst, r)
        if not case.track:  # the running radius is not tracked: the strategy leaves a tensor under that key alone
            assert tc.bits_equal(_accumulate_strategy_cpu(case, inp, state)["radii"], state["radii"])
        if bool(hidden.any()):
            bad = _accumulate_f32(inp["grad"], inp["radii"], dict(state, radii=None), *scal, select=False)
            assert not tc.ratio(bad["grad2d"], ref["grad2d"], ref["tol_grad2d"]) <= 1.0, case.name
            caught += 1
    assert caught >= len(tc.ACC_CASES) - 6
    print(f"statistics float32 restatements: worst error / bound {worst:.3f}")
