"""GPU: the from-world (3DGUT) compositing pair of csrc/raster_world.hip against the float64 statement of itself, element by
element, in every launch regime: tile sizes 16 / 12 / 8 / 5 (256 and 64 threads, surplus lanes, image edges that cut tiles),
lists from empty to 15 staging batches and cut at the batch boundaries, forward templates 8 / 16 / 32 and chunks above 32,
backward chunks of 4 channels with the hit distance in a later chunk, masks, B > 1 batches of Gaussians, the zero ray,
hit_t < 0, the 0.99 clamp, non-unit quaternions and anisotropic scales. tests/_world_cases.py builds the cases, the reference,
the per-element bounds and the decided mask on the CPU (derivations there); tests/test_world_cases.py checks them without a GPU.

Forward comparisons run on EVERY decided pixel; the cotangents are exactly zero on the undecided ones, so EVERY gradient
element is compared. Each test prints the worst |err| / bound per output and asserts <= 1, and recomputes the undecided share
(cap 5 %). The backward consumes the GPU's own forward outputs, as in production."""
import pytest
import torch

import _world_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
CABI_FWD_CASES = ("t16_cut", "wide35", "t8_b2c2", "masked")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd
    from gsplat_amd import _ops  # noqa: F401  (defines torch.ops.gsplat.*)

    return gsplat_amd


def _reference(name):
    cs, ref = wc.case(name), wc.reference(name)
    share = ref.stats["undecided"]
    print(f"{name}: undecided {share:.3%}")
    assert share <= wc.UNDECIDED_CAP
    return cs, ref


def _report(name, what, ratios):
    print(f"{name} {what}: " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    worst = max(ratios.values()) if ratios else 0.0
    assert worst <= 1.0, (name, what, ratios)


def _flat(cs):
    """The C entry points' arguments on the device: Gaussians [B,N,*], rows [I,N,*], rays [I,H,W,6], lists, bg, masks."""
    d = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    return dict(means=d(cs.means), quats=d(cs.quats), scales=d(cs.scales), colors=d(cs.colors), opacities=d(cs.opacities),
                rays=d(cs.rays), bg=d(cs.backgrounds), masks=d(cs.masks), off=d(cs.offsets), fl=d(cs.flatten_ids))


def _check_forward(cs, ref, name, what, renders, alphas, last_ids, counts, normals):
    P = cs.I * cs.H * cs.W
    got = dict(render_colors=renders.detach().cpu().reshape(P, cs.D), render_alphas=alphas.detach().cpu().reshape(P, 1),
               render_normals=(normals.detach().cpu().reshape(P, 3) if cs.normals else None))
    last, cnt, dec = last_ids.cpu().reshape(P), counts.cpu().reshape(P), ref.decided
    assert torch.isfinite(got["render_colors"]).all() and torch.isfinite(got["render_alphas"]).all()
    bad = last[dec] != ref.last_ids[dec]
    assert not bad.any(), f"{name}: last_ids differ on {int(bad.sum())} decided pixels, first {torch.nonzero(dec)[bad][:5].flatten()}"
    bad = cnt[dec] != ref.sample_counts[dec]
    assert not bad.any(), f"{name}: sample counts differ on {int(bad.sum())} decided pixels"
    # masked tiles and zero rays: bit-exact background (or 0), alpha 0, no sample
    blank = ref.blank
    if blank.any():
        fill = (cs.backgrounds.repeat_interleave(cs.H * cs.W, dim=0) if cs.backgrounds is not None
                else torch.zeros(P, cs.D))[blank]
        assert torch.equal(got["render_colors"][blank], fill)
        assert bool((got["render_alphas"][blank] == 0).all()) and bool((last[blank] == -1).all()) and bool((cnt[blank] == 0).all())
        if cs.normals:
            assert bool((got["render_normals"][blank] == 0).all())
    _report(name, what, wc.compare_forward(cs, ref, got))


def _op_forward(cs, requires_grad=False):
    B, C, N, D, I = cs.B, cs.C, cs.N, cs.D, cs.I
    lead = (B, C)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(requires_grad)  # noqa: E731
    lv = dict(means=leaf(cs.means), quats=leaf(cs.quats), scales=leaf(cs.scales), colors=leaf(cs.colors.reshape(lead + (N, D))),
              opacities=leaf(cs.opacities.reshape(lead + (N,))),
              rays=cs.rays.reshape(lead + (cs.H, cs.W, 6)).to(DEV).clone().requires_grad_(requires_grad and cs.want_rays))
    if cs.backgrounds is not None:
        lv["backgrounds"] = leaf(cs.backgrounds.reshape(lead + (D,)))
    masks = None if cs.masks is None else cs.masks.reshape(lead + (cs.th, cs.tw)).to(DEV)
    eye = torch.eye(4, device=DEV).expand(lead + (4, 4)).contiguous()  # the rays are given: the cameras are not read
    Ks = torch.eye(3, device=DEV).expand(lead + (3, 3)).contiguous()
    out = torch.ops.gsplat.rasterize_to_pixels_from_world_3dgs(
        lv["means"], lv["quats"], lv["scales"], lv["colors"], lv["opacities"], lv.get("backgrounds"), masks, cs.W, cs.H, cs.ts, eye,
        None, Ks, 0, torch.classes.gsplat.UnscentedTransformParameters(), 4, lv["rays"], None, None, None,
        torch.classes.gsplat.FThetaCameraDistortionParameters(), None, None, cs.offsets.reshape(lead + (cs.th, cs.tw)).to(DEV),
        cs.flatten_ids.to(DEV), True, cs.hit, cs.normals, 0, True)
    return out, lv


@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_forward_op_within_fp64_bounds(G, name):
    cs, ref = _reference(name)
    with torch.no_grad():
        (renders, alphas, last_ids, counts, normals), _ = _op_forward(cs)
    assert (normals is not None) == cs.normals and last_ids.dtype == torch.int32 and counts.dtype == torch.int32
    _check_forward(cs, ref, name, "forward (op)", renders, alphas, last_ids, counts, normals)


def _cabi_forward(cs, a):
    from gsplat_amd import _cabi

    I, H, W, D = cs.I, cs.H, cs.W, cs.D
    renders = torch.full((I, H, W, D), float("nan"), device=DEV)
    alphas = torch.full((I, H, W, 1), float("nan"), device=DEV)
    last_ids = torch.full((I, H, W), -7, device=DEV, dtype=torch.int32)
    counts = torch.full((I, H, W), -7, device=DEV, dtype=torch.int32)
    normals = torch.full((I, H, W, 3), float("nan"), device=DEV) if cs.normals else None
    _cabi.call("gsx_raster_world_fwd", a["means"], a["quats"], a["scales"], a["colors"], a["opacities"], a["rays"], a["bg"],
               a["masks"], a["off"], a["fl"], I, cs.C, cs.N, a["fl"].numel(), D, W, H, cs.ts, cs.tw, cs.th, int(cs.hit), renders,
               alphas, last_ids, counts, normals)
    return renders, alphas, last_ids, counts, normals


@pytest.mark.parametrize("name", CABI_FWD_CASES)
def test_forward_c_entry_within_fp64_bounds(G, name):
    """gsx_raster_world_fwd through _cabi.call, into outputs pre-filled with NaN / -7: every pixel is written."""
    cs, ref = _reference(name)
    out = _cabi_forward(cs, _flat(cs))
    _check_forward(cs, ref, name, "forward (C entry)", *out)


def _cabi_backward(cs, a, ref, alphas, last_ids, want_rays, plain=False):
    """gsx_raster_world_bwd; `plain`: v_render_normals = NULL, use_hit_distance = 0 (and no v_rays), whatever the case has."""
    from gsplat_amd import _cabi

    I, D = cs.I, cs.D
    cot = ref.cot
    v_r = cot.v_render.to(DEV)
    v_a = cot.v_alpha.to(DEV) if cot.v_alpha is not None else None
    rows = torch.zeros((I * cs.N, 10 + D), device=DEV)
    v_n = cot.v_normals.to(DEV) if cs.normals and not plain else None
    v_rays = torch.zeros((I, cs.H, cs.W, 6), device=DEV) if want_rays else None
    _cabi.call("gsx_raster_world_bwd", a["means"], a["quats"], a["scales"], a["colors"], a["opacities"], a["rays"], a["bg"],
               a["masks"], a["off"], a["fl"], alphas, last_ids, v_r, v_a, v_n, I, cs.C, cs.N, a["fl"].numel(), D, cs.W, cs.H, cs.ts,
               cs.tw, cs.th, 0 if plain else int(cs.hit), rows, 10 + D, v_rays)
    return rows.cpu(), (None if v_rays is None else v_rays.cpu())


@pytest.mark.parametrize("name", wc.BACKWARD_CASES)
def test_backward_rows_within_fp64_bounds(G, name):
    """The C-ABI rows [I N][10 + D] of gsx_raster_world_bwd per element, the rows that must stay exactly zero included (their
    bound is 0), with v_rays where the case asks for them; a second run into fresh zeroed rows agrees within the unordered sums'
    term, and so does - where the case has neither hit distance nor normals - the call with NULL v_render_normals, use_hit_distance
    0 and NULL v_rays."""
    cs, ref = _reference(name)
    a = _flat(cs)
    _, alphas, last_ids, _, _ = _cabi_forward(cs, a)
    rows, v_rays = _cabi_backward(cs, a, ref, alphas, last_ids, cs.want_rays)
    assert torch.isfinite(rows).all()
    _report(name, "rows", wc.compare_rows(cs, ref, rows, v_rays))
    if cs.masks is not None:  # Gaussians seen only by masked tiles keep zero rows, masked pixels zero v_rays
        assert bool((ref.bwd_bounds.rows_mag.sum(1) == 0).any())
        assert v_rays is not None and bool((v_rays.reshape(-1, 6)[~ref.open_px] == 0).all())
    if ref.zero_ray.any() and v_rays is not None:
        assert bool((v_rays.reshape(-1, 6)[ref.zero_ray] == 0).all())
    rows2, v_rays2 = _cabi_backward(cs, a, ref, alphas, last_ids, cs.want_rays)
    twice = 2.0 * ref.bwd_bounds.rows_sum
    assert wc.ratio(rows2 - rows, twice) <= 1.0, "a second run differs by more than the unordered sums allow"
    if v_rays is not None:
        assert torch.equal(v_rays, v_rays2)  # one lane owns a pixel: no unordered sum
    if not (cs.hit or cs.normals):
        rows3, _ = _cabi_backward(cs, a, ref, alphas, last_ids, False, plain=True)
        _report(name, "rows (no extras, no v_rays)", wc.compare_rows(cs, ref, rows3))
        assert wc.ratio(rows3 - rows, twice) <= 1.0, "the rows differ between a call with and a call without v_rays"


@pytest.mark.parametrize("name", wc.BACKWARD_CASES)
def test_autograd_gradients_within_fp64_bounds(G, name):
    """v_means / v_quats / v_scales / v_colors / v_opacities / v_rays / v_backgrounds of the op, per element, against float64
    autograd."""
    cs, ref = _reference(name)
    (renders, alphas, last_ids, counts, normals), lv = _op_forward(cs, requires_grad=True)
    cot = ref.cot
    loss = (renders * cot.v_render.to(DEV).reshape(renders.shape)).sum()
    if cot.v_alpha is not None:
        loss = loss + (alphas * cot.v_alpha.to(DEV).reshape(alphas.shape)).sum()
    if cs.normals:
        loss = loss + (normals * cot.v_normals.to(DEV).reshape(normals.shape)).sum()
    loss.backward()
    got = {f"v_{k}": (None if t.grad is None else t.grad.cpu()) for k, t in lv.items()}
    assert all(got[k] is not None for k in ("v_means", "v_quats", "v_scales", "v_colors", "v_opacities"))
    assert (got["v_rays"] is not None) == cs.want_rays and (got.get("v_backgrounds") is not None) == (cs.backgrounds is not None)
    _report(name, "gradients (autograd)", wc.compare_grads(cs, ref, got))
