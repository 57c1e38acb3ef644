"""CPU: the cases, the float64 reference and the bounds of tests/_world_cases.py (from-world compositing, csrc/raster_world.hip)
without a GPU: (1) every case reaches the regime its name claims and stays under the undecided cap; (2) the float32 statement
of oracle/eval3d.py goes through the very comparisons the GPU test makes and stays at or below 0.5 of every bound; (3) every
deliberately wrong restatement falls outside a bound (or takes another sample) on its case - except the float32-assembled M,
which these bounds cannot tell from float32 rounding: that is stated as a test of its own.

Worst |err| / bound of the float32 statement per output, over all cases (this machine; the per-case figures are printed):
    render_colors 0.13   render_alphas 0.46   render_normals 0.06
    rows: v_mean 0.033  torque 0.003  v_scale 0.013  v_opacity 0.039  v_colors 0.059  v_rays 0.042
    v_means 0.033  v_quats 0.0006  v_scales 0.013  v_colors 0.059  v_opacities 0.039  v_rays 0.042  v_backgrounds 0.002
(The torque and v_quats bounds are wide because the kernel forms the torque as p x a + ray_d x b from terms that nearly cancel:
the bound follows the absolute terms. On the GPU the saturated cases come much closer to their bounds than here - 0.25..0.38 -
because the kernel's backward rebuilds T from 1 - alpha_f32, the u / T_final term, which float32 autograd does not do.)"""
import pytest
import torch

import _world_cases as wc

HALF = 0.5
# wrong restatement -> the case that exposes it
WRONG = {
    "batch0": "t8_b2c2", "camera0": "t8_b2c2", "stop_blended": "t16_cut", "clamp_geometry_on": "clamp",
    "hd_no_scale": "t12_hit5", "hd_raw_direction": "t12_hit5", "hd_channel3": "t12_hit5", "scale_no_direct_share": "t12_hit5",
    "normal_not_facing": "t8_b2c2", "bg_without_T": "t12_hit5", "v_alpha_without_bg": "t12_hit5",
    "v_alphas_every_chunk": "t12_hit5", "quats_without_inverse_norm": "nonunit", "masked_zero": "masked",
    "zero_ray_samples": "behind_zero",
}


def _run(name, dtype, variant=None):
    """The statement on a case -> ({output: ratio}, integer mismatches on decided pixels), every comparison of the GPU test."""
    cs, ref = wc.case(name), wc.reference(name)
    post = variant if variant == "quats_without_inverse_norm" else None
    r, lv = wc.statement(cs, dtype, variant=None if post else variant, requires_grad=cs.backward)
    P = cs.I * cs.H * cs.W
    got = dict(render_colors=r.renders.detach().reshape(P, cs.D), render_alphas=r.alphas.detach().reshape(P, 1),
               render_normals=(r.normals.detach().reshape(P, 3) if cs.normals else None))
    ratios = dict(wc.compare_forward(cs, ref, got))
    dec = ref.decided
    wrong_ids = int((r.last_ids.reshape(P)[dec] != ref.last_ids[dec]).sum()) + int((r.sample_counts.reshape(P)[dec] != ref.sample_counts[dec]).sum())
    if cs.backward:
        g = wc.gradients(cs, r, lv, ref.cot)
        grads = {k: getattr(g, k) for k in wc.GRADS}
        if post:
            grads["v_quats"] = grads["v_quats"] * cs.quats.to(dtype).norm(dim=-1, keepdim=True)
        ratios.update({f"rows.{k}": v for k, v in wc.compare_rows(cs, ref, g.rows, g.v_rays).items()})
        ratios.update(wc.compare_grads(cs, ref, grads))
    return ratios, wrong_ids


@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_case_reaches_its_regime(name):
    cs, ref, p = wc.case(name), wc.reference(name), wc.params(name)
    st, lens = ref.stats, wc.list_lengths(cs)
    print(name, "longest list", int(lens.max()), st)
    assert st["undecided"] <= wc.UNDECIDED_CAP
    assert int(cs.flatten_ids.min()) >= 0 and int(cs.flatten_ids.max()) < cs.I * cs.N and st["max_count"] > 0
    threads = 64 if cs.ts <= 8 else 256
    if name == "t16_deep":
        assert cs.ts == 16 and cs.W % 16 == 8 and cs.H % 16 == 12 and cs.D == 3 and cs.backgrounds is not None
        assert lens.max() > 3 * wc.BATCH and st["saturated"] > 0.5 and st["skipped_batches"] >= 1
    elif name == "t16_cut":
        assert cs.ts == 16 and set(p["cut"]) <= set(lens.tolist()) and set(p["cut"]) == {0, 1, 127, 128, 129, 256, 257}
        assert st["last_at_batch_edge"] > 0  # a pixel's last contributor sits in the first or last slot of a staging batch
    elif name == "t12_hit5":
        assert cs.ts == 12 and threads - cs.ts ** 2 == 112 and cs.D == 5 and cs.hit and cs.bwd_chunks == 2 and (cs.D - 1) % 4 == 0
        assert cs.backgrounds is not None and cs.want_rays
    elif name == "t8_b2c2":
        assert cs.ts == 8 and (cs.B, cs.C, cs.D) == (2, 2, 4) and cs.hit and cs.normals
        assert not torch.equal(cs.means[0], cs.means[1]) and not torch.equal(cs.colors[0], cs.colors[1])
        assert not torch.equal(cs.opacities[2], cs.opacities[3])
    elif name == "t5_d1":
        assert cs.ts == 5 and threads - 25 == 39 and cs.D == 1 and cs.backgrounds is None and ref.cot.v_alpha is None
    elif name == "wide35":
        assert cs.D == 35 and cs.fwd_chunks == 2 and cs.bwd_chunks == 9 and cs.hit and cs.normals and cs.want_rays
        assert cs.backgrounds is not None and (cs.W, cs.H, cs.ts) == (24, 16, 8)
    elif name in ("d9", "d17"):
        assert cs.D == int(name[1:]) and not cs.backward
    elif name in ("masked", "masked_nobg"):
        share = 1.0 - float(cs.masks.float().mean())
        assert 0.2 <= share <= 0.45 and (cs.backgrounds is None) == (name == "masked_nobg") and cs.want_rays
        listed = torch.bincount(cs.flatten_ids.long(), minlength=cs.I * cs.N) > 0
        assert bool((listed & (ref.bwd_bounds.rows_mag.sum(1) == 0)).any())  # Gaussians seen only by masked tiles
        assert bool((ref.grads.v_rays.reshape(-1, 6)[~ref.open_px] == 0).all())
    elif name == "behind_zero":
        assert st["behind"] > 0.2 and 0.03 <= st["zero_ray"] <= 0.08
        assert bool((ref.sample_counts[ref.zero_ray] == 0).all())
    elif name in ("clamp", "clamp_hit"):
        assert st["clamped"] > 0.1 and float(cs.opacities.min()) >= 0.992 and cs.hit == (name == "clamp_hit")
    elif name == "nonunit":
        n = cs.quats.norm(dim=-1)
        assert float(n.min()) < 0.5 and float(n.max()) > 2.0
    elif name == "aniso":
        ratio = cs.scales.max(-1).values / cs.scales.min(-1).values
        assert float(ratio.max()) >= 15.0 and float(cs.scales.min()) < 0.012 and float(ratio.max()) <= 25.0
    # image edges cut tiles in every case but the 24 x 16 ones
    if (cs.W, cs.H) != (24, 16):
        assert cs.W % cs.ts or cs.H % cs.ts


@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_float32_statement_stays_within_half_of_every_bound(name):
    ratios, wrong_ids = _run(name, torch.float32)
    print(name, {k: round(v, 4) for k, v in ratios.items()})
    assert wrong_ids == 0
    assert max(ratios.values()) <= HALF, ratios


def test_float64_statement_reproduces_the_reference_exactly():
    """The machinery itself: the reference against itself is inside every bound with ratio ~0 (and a zero bound means equal)."""
    ratios, wrong_ids = _run("t8_b2c2", torch.float64)
    assert wrong_ids == 0 and max(ratios.values()) < 1e-6


@pytest.mark.parametrize("variant", tuple(WRONG))
def test_wrong_restatement_falls_outside(variant):
    ratios, wrong_ids = _run(WRONG[variant], torch.float64, variant)
    worst = max(ratios, key=ratios.get)
    print(variant, WRONG[variant], "worst", worst, ratios[worst], "integer mismatches", wrong_ids)
    assert ratios[worst] > 1.0 or wrong_ids > 0


def test_float32_assembled_m_cannot_be_told_from_float32_rounding():
    """M = S^-1 R^T assembled in float32 moves o' by a few u |M| |p| - the size of E_o itself, which already charges 5 u to
    every product of M: on `aniso` (the conditioning the float64 M exists for) that restatement stays inside every bound, so no
    per-element float32 bound can expose it. What holds the float64 assembly in place is the golden test against the
    reference's own float64-assembled values (tests/test_gpu_eval3d.py)."""
    ratios, wrong_ids = _run("aniso", torch.float32, "m_f32")
    assert wrong_ids == 0 and max(ratios.values()) <= 1.0
