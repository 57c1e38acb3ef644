"""GPU: the fused bilateral-grid kernels (csrc/bilagrid.hip) against tests/golden/bilagrid_ref.npz and against the torch
composition. Tolerances as in tests/test_bilagrid.py: 4 x the yardstick's own float32-vs-float64 spread plus one float32 ulp of
its largest magnitude; v_grids is an atomic sum and is only ever compared by tolerance. At 1080p, where no fixture exists, the
yardstick is the torch composition: its float64 run is the truth and its own float32 run gives the spread."""
import numpy as np
import pytest
import torch

from gsplat_amd import bilagrid
from gsplat_amd.bilagrid import _FusedSlice
from gsplat_amd.losses import _FusedTotalVariation, photometric_loss, total_variation_loss, total_variation_torch
from test_bilagrid import CASE_NAMES, Z, case_inputs, check_case, tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda"


def grid_idx_like(idx, rgb):
    return idx.reshape(-1, *([1] * (rgb.dim() - 1)))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fused_slice_matches_reference(name):
    """Explicit xy (every case): forward + the scatter backward."""
    spec, model, xy, rgb, idx, w = case_inputs(name, DEV)
    rgb = rgb.requires_grad_(True)
    before = _FusedSlice.calls
    res = bilagrid.slice(model, xy, rgb, grid_idx_like(idx, rgb), affine_mats=True)
    assert _FusedSlice.calls == before + 1
    (res["rgb"] * w).sum().backward()
    check_case(name, spec, res, rgb.grad, model.grids.grad)


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n != "p"])
def test_fused_slice_image_matches_reference(name):
    """Pixel-centre coordinates from the pixel index: forward + the cell-owner backward (gradient summed in LDS)."""
    spec, model, xy, rgb, idx, w = case_inputs(name, DEV)
    rgb = rgb.requires_grad_(True)
    before = _FusedSlice.calls
    res = bilagrid.slice_image(model, rgb, idx, affine_mats=True)
    assert _FusedSlice.calls == before + 1
    (res["rgb"] * w).sum().backward()
    check_case(name, spec, res, rgb.grad, model.grids.grad)


def test_slice_image_equals_slice_with_pixel_centres():
    spec, model, xy, rgb, idx, w = case_inputs("s", DEV)
    a = bilagrid.slice_image(model, rgb, idx)["rgb"]
    b = bilagrid.slice(model, bilagrid.pixel_center_xy(*rgb.shape[:3], device=DEV), rgb, idx.reshape(-1, 1, 1, 1))["rgb"]
    assert "rgb_affine_mats" not in bilagrid.slice_image(model, rgb, idx)
    # the same arithmetic on the same float32 coordinates: pixel_center_xy divides by a tensor, so on the device it holds the
    # correctly rounded (x + 0.5) / W that the kernel forms from the pixel index
    assert torch.equal(bilagrid.pixel_center_xy(*rgb.shape[:3], device=DEV), xy)
    assert torch.equal(a.detach(), b.detach())


def test_strided_rgb_view():
    """rgb = [..., :3] of a 4-channel render: read in place, and v_rgb lands in the first three channels of the render."""
    spec, model, xy, rgb, idx, w = case_inputs("a", DEV)
    render = torch.cat([rgb, torch.full_like(rgb[..., :1], 7.0)], dim=-1).requires_grad_(True)
    view = render[..., :3]
    assert not view.is_contiguous()
    before = _FusedSlice.calls
    out = bilagrid.slice_image(model, view, idx)["rgb"]
    assert _FusedSlice.calls == before + 1
    (out * w).sum().backward()
    g_view, g_grids = render.grad.clone(), model.grids.grad.clone()
    model.grids.grad = None
    dense = rgb.clone().requires_grad_(True)
    out_d = bilagrid.slice_image(model, dense, idx)["rgb"]
    (out_d * w).sum().backward()
    assert torch.equal(out, out_d)
    assert torch.equal(g_view[..., :3], dense.grad) and bool((g_view[..., 3] == 0).all())
    tol = tolerance(Z["a_err_v_grids"], Z["a_v_grids"])
    assert float((g_grids - model.grids.grad).abs().max()) <= tol  # two atomic sums of the same terms


def test_out_of_range_index_is_contained():
    model = bilagrid.BilateralGrid(2).to(DEV)
    rgb = torch.rand(2, 8, 9, 3, device=DEV, requires_grad=True)
    idx = torch.tensor([1, 5], device=DEV)
    out = bilagrid.slice_image(model, rgb, idx)["rgb"]
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isnan(out[1]).all())
    out[0].sum().backward()
    assert bool((rgb.grad[1] == 0).all()) and bool(torch.isfinite(model.grids.grad).all())
    with pytest.raises(IndexError):
        bilagrid.slice_image(model, rgb, idx, check_index=True)


def _compose(model, rgb, idx, w, dtype):
    m = bilagrid.BilateralGrid(model.grids.shape[0], model.grid_width, model.grid_height, model.grid_guidance).to(DEV).to(dtype)
    with torch.no_grad():
        m.grids.copy_(model.grids.to(dtype))
    r = rgb.detach().to(dtype).clone().requires_grad_(True)
    xy = bilagrid.pixel_center_xy(*rgb.shape[:3], device=DEV).to(dtype)  # the float32 coordinates, widened
    out = bilagrid.slice_torch(m, xy, r, idx)["rgb"]
    (out * w.to(dtype)).sum().backward()
    return out.detach(), r.grad, m.grids.grad


def test_fused_matches_torch_composition_at_1080p():
    g = torch.Generator().manual_seed(7)
    model = bilagrid.BilateralGrid(2).to(DEV)
    with torch.no_grad():
        model.grids += (0.1 * torch.randn(model.grids.shape, generator=g)).to(DEV)
    rgb = (torch.rand(1, 1080, 1920, 3, generator=g) * 1.6 - 0.3).to(DEV)
    w = torch.randn(1, 1080, 1920, 3, generator=g).to(DEV)
    idx = torch.tensor([1], device=DEV)
    o32, vr32, vg32 = _compose(model, rgb, idx, w, torch.float32)
    o64, vr64, vg64 = _compose(model, rgb, idx, w, torch.float64)
    leaf = rgb.clone().requires_grad_(True)
    before = _FusedSlice.calls
    out = bilagrid.slice_image(model, leaf, idx)["rgb"]
    assert _FusedSlice.calls == before + 1
    (out * w).sum().backward()
    iz = (rgb.double() @ torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64, device=DEV)) * 7
    excl = ((iz - iz.round()).abs() < 1e-4) & (iz.round() >= 0) & (iz.round() <= 7)
    assert float(excl.float().mean()) <= 0.01
    keep = ~excl
    failures = []
    for what, got, f32, f64 in (("rgb_out", out.detach(), o32, o64), ("v_rgb", leaf.grad[keep], vr32[keep], vr64[keep]),
                                ("v_grids", model.grids.grad, vg32, vg64)):
        err = float((f32.double() - f64).abs().max())
        d = float((got.double() - f64).abs().max())
        tol = tolerance(err, f64.abs().max().item())
        print(f"1080p {what}: max |fused - float64| {d:.3e} tolerance {tol:.3e} (torch float32 spread {err:.3e})")
        if not d <= tol:
            failures.append((what, d, tol))
    assert not failures, failures


@pytest.mark.parametrize("k", range(int(Z["n_tv"])))
def test_fused_total_variation_matches_reference(k):
    x = torch.from_numpy(Z[f"tv{k}_x"]).to(DEV).requires_grad_(True)
    before = _FusedTotalVariation.calls
    loss = total_variation_loss(x)
    assert _FusedTotalVariation.calls == before + 1
    loss.backward()
    d_loss = abs(float(loss.detach()) - float(Z[f"tv{k}_loss"]))
    d_grad = float(np.abs(x.grad.cpu().numpy() - Z[f"tv{k}_grad"]).max())
    print(f"tv{k}: |d loss| {d_loss:.3e} max |d grad| {d_grad:.3e}")
    assert d_loss <= tolerance(Z[f"tv{k}_err_loss"], Z[f"tv{k}_loss"])
    assert d_grad <= tolerance(Z[f"tv{k}_err_grad"], Z[f"tv{k}_grad"])


def test_fused_total_variation_on_the_default_grid():
    g = torch.Generator().manual_seed(3)
    model = bilagrid.BilateralGrid(5).to(DEV)
    with torch.no_grad():
        model.grids += (0.1 * torch.randn(model.grids.shape, generator=g)).to(DEV)
    before = _FusedTotalVariation.calls
    loss = model.tv_loss()
    assert _FusedTotalVariation.calls == before + 1
    loss.backward()
    x32 = model.grids.detach().clone().requires_grad_(True)
    l32 = total_variation_torch(x32)
    l32.backward()
    x64 = model.grids.detach().double().requires_grad_(True)
    l64 = total_variation_torch(x64)
    l64.backward()
    e_loss, e_grad = abs(float(l32) - float(l64)), float((x32.grad.double() - x64.grad).abs().max())
    d_loss, d_grad = abs(float(loss) - float(l64)), float((model.grids.grad.double() - x64.grad).abs().max())
    print(f"tv default grid: |d loss| {d_loss:.3e} (spread {e_loss:.3e}) max |d grad| {d_grad:.3e} (spread {e_grad:.3e})")
    assert d_loss <= tolerance(e_loss, float(l64))
    assert d_grad <= tolerance(e_grad, x64.grad.abs().max().item())
    again = model.tv_loss()
    assert torch.equal(again, loss)  # fixed summation order


def test_training_step_end_to_end():
    """rasterization -> slice_image -> photometric_loss + 10 TV -> backward: finite, non-zero gradients everywhere."""
    import gsplat_amd
    from _util import make_scene

    sc, W, H = make_scene(N=3000, C=2, width=160, height=112, seed=0)
    names = ("means", "quats", "scales", "opacities", "colors")
    leaves = {k: sc[k].to(DEV).clone().requires_grad_(True) for k in names}
    model = bilagrid.BilateralGrid(4).to(DEV)
    target = torch.rand(2, H, W, 3, device=DEV)
    rc, _ra, _meta = gsplat_amd.rasterization(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"],
                                             leaves["colors"], sc["viewmats"].to(DEV), sc["Ks"].to(DEV), W, H,
                                             render_mode="RGB+ED")
    before = _FusedSlice.calls
    colors = bilagrid.slice_image(model, rc[..., :3], torch.tensor([3, 1], device=DEV))["rgb"]
    assert _FusedSlice.calls == before + 1
    loss = photometric_loss(colors.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2), 0.2) + 10.0 * model.tv_loss()
    loss.backward()
    assert bool(torch.isfinite(loss))
    for k in names:
        gr = leaves[k].grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, k
    gg = model.grids.grad
    assert bool(torch.isfinite(gg).all())
    assert float(gg[3].abs().max()) > 0 and float(gg[1].abs().max()) > 0


def test_unwanted_gradients_are_skipped():
    """Frozen grids: only v_rgb, equal to the one of the full backward; a constant image: only v_grids."""
    spec, model, xy, rgb, idx, w = case_inputs("c", DEV)
    leaf = rgb.clone().requires_grad_(True)
    (bilagrid.slice_image(model, leaf, idx)["rgb"] * w).sum().backward()
    full_rgb, full_grids = leaf.grad.clone(), model.grids.grad.clone()
    model.grids.grad = None
    model.grids.requires_grad_(False)
    leaf2 = rgb.clone().requires_grad_(True)
    (bilagrid.slice_image(model, leaf2, idx)["rgb"] * w).sum().backward()
    assert model.grids.grad is None and torch.equal(leaf2.grad, full_rgb)
    model.grids.requires_grad_(True)
    (bilagrid.slice_image(model, rgb, idx)["rgb"] * w).sum().backward()
    assert float((model.grids.grad - full_grids).abs().max()) <= tolerance(Z["c_err_v_grids"], Z["c_v_grids"])
