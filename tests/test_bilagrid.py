"""CPU: gsplat_amd.bilagrid (torch composition) and losses.total_variation_loss against tests/golden/bilagrid_ref.npz, which
tools/pin_bilagrid_against_reference.py recorded from the reference's examples/lib_bilagrid.py and gsplat/losses.py.

Tolerance of every comparison: 4 x the reference's own float32-vs-float64 spread of that output (err_* in the fixture) plus one
float32 ulp of the largest reference magnitude. v_rgb is not compared on the pixels flagged in {case}_excl (float64 guidance
index within 1e-4 of an integer, where the derivative jumps); they are at most 1 % of a case, asserted here again."""
import json
import os

import numpy as np
import pytest
import torch

from gsplat_amd import bilagrid
from gsplat_amd.losses import total_variation_loss

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bilagrid_ref.npz")


def load_fixture():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"]))


Z, CASES = load_fixture()
CASE_NAMES = [c["name"] for c in CASES]


def tolerance(err, ref) -> float:
    return 4.0 * float(err) + float(np.spacing(np.float32(np.abs(np.asarray(ref)).max())))


def case_inputs(name, device="cpu"):
    spec = next(c for c in CASES if c["name"] == name)
    t = lambda k: torch.from_numpy(Z[f"{name}_{k}"]).to(device)  # noqa: E731
    model = bilagrid.BilateralGrid(3, *spec["grid"])
    with torch.no_grad():
        model.grids.copy_(torch.from_numpy(Z[f"{spec['grids_of']}_grids"]))
    return spec, model.to(device), t("xy"), t("rgb"), t("idx"), t("w")


def excluded(name, spec):
    """The v_rgb exclusion, recomputed from the inputs: float64 iz within 1e-4 of an integer of [0, L - 1]; at most 1 %."""
    L = spec["grid"][2]
    iz = (Z[f"{name}_rgb"].astype(np.float64) @ np.array([0.299, 0.587, 0.114])) * (L - 1)
    excl = (np.abs(iz - np.round(iz)) < 1e-4) & (np.round(iz) >= 0) & (np.round(iz) <= L - 1)
    assert np.array_equal(excl, Z[f"{name}_excl"])
    assert excl.mean() <= 0.01, (name, excl.mean())
    return excl


def check_case(name, spec, res, v_rgb, v_grids):
    """Compares one case's outputs (tensors on any device) with the fixture; prints each figure before it asserts."""
    keep = ~excluded(name, spec)
    got = {"rgb_out": res["rgb"].detach().cpu().numpy(), "v_rgb": v_rgb.cpu().numpy(), "v_grids": v_grids.cpu().numpy()}
    ref = {k: Z[f"{name}_{k}"] for k in got}
    if spec["mats"]:
        got["mats"], ref["mats"] = res["rgb_affine_mats"].detach().cpu().numpy()[0], Z[f"{name}_mats"]
    failures = []
    for k in got:
        assert got[k].shape == ref[k].shape, (name, k, got[k].shape, ref[k].shape)
        d = np.abs(got[k].astype(np.float64) - ref[k])
        if k == "v_rgb":
            d = d[keep]
        tol = tolerance(Z[f"{name}_err_{k}"], ref[k])
        print(f"{name} {k}: max |diff| {d.max():.3e} tolerance {tol:.3e} (err {float(Z[f'{name}_err_{k}']):.3e})")
        if not d.max() <= tol:
            failures.append((k, float(d.max()), tol))
    assert not failures, (name, failures)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_torch_composition_matches_reference(name):
    spec, model, xy, rgb, idx, w = case_inputs(name)
    rgb = rgb.requires_grad_(True)
    res = bilagrid.slice(model, xy, rgb, idx.reshape(-1, *([1] * (rgb.dim() - 1))), affine_mats=True)
    (res["rgb"] * w).sum().backward()
    check_case(name, spec, res, rgb.grad, model.grids.grad)


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n != "p"])
def test_slice_image_is_slice_at_pixel_centres(name):
    spec, model, xy, rgb, idx, w = case_inputs(name)
    assert torch.equal(bilagrid.pixel_center_xy(*rgb.shape[:3]), xy)  # the trainer's (arange + 0.5) / size
    rgb = rgb.requires_grad_(True)
    res = bilagrid.slice_image(model, rgb, idx, affine_mats=True)
    (res["rgb"] * w).sum().backward()
    check_case(name, spec, res, rgb.grad, model.grids.grad)


@pytest.mark.parametrize("k", range(int(Z["n_tv"])))
def test_total_variation_matches_reference(k):
    x = torch.from_numpy(Z[f"tv{k}_x"]).requires_grad_(True)
    loss = total_variation_loss(x)
    loss.backward()
    d_loss, d_grad = abs(float(loss.detach()) - float(Z[f"tv{k}_loss"])), float(np.abs(x.grad.numpy() - Z[f"tv{k}_grad"]).max())
    print(f"tv{k}: |d loss| {d_loss:.3e} max |d grad| {d_grad:.3e}")
    assert d_loss <= tolerance(Z[f"tv{k}_err_loss"], Z[f"tv{k}_loss"])
    assert d_grad <= tolerance(Z[f"tv{k}_err_grad"], Z[f"tv{k}_grad"])


def test_total_variation_definition():
    """[B, C, d1] by hand: sum of squared forward differences / (C (d1 - 1)) / B; any number of spatial axes is accepted."""
    x = torch.tensor([[[0.0, 1.0, 3.0], [2.0, 2.0, 5.0]]])
    assert float(total_variation_loss(x)) == pytest.approx((1 + 4 + 0 + 9) / 4.0)
    assert float(total_variation_loss(torch.ones(2, 3, 1, 1))) == 0.0
    with pytest.raises(ValueError):
        total_variation_loss(torch.ones(4, 4))


def test_state_dict_and_attributes():
    m = bilagrid.BilateralGrid(5, grid_X=6, grid_Y=7, grid_W=3)
    sd = m.state_dict()
    assert set(sd) == {"grids", "rgb2gray_weight"}
    assert tuple(sd["grids"].shape) == (5, 12, 3, 7, 6) and tuple(sd["rgb2gray_weight"].shape) == (1, 3)
    assert (m.grid_width, m.grid_height, m.grid_guidance) == (6, 7, 3)
    assert [n for n, _ in m.named_parameters()] == ["grids"] and [n for n, _ in m.named_buffers()] == ["rgb2gray_weight"]
    assert torch.equal(sd["rgb2gray_weight"], torch.tensor([[0.299, 0.587, 0.114]]))
    d = bilagrid.BilateralGrid(2)
    assert tuple(d.grids.shape) == (2, 12, 8, 16, 16)
    assert torch.equal(d.grids[1, :, 3, 4, 5], torch.eye(3, 4).reshape(12))
    assert float(d.tv_loss().detach()) == 0.0
    # a reference-shaped state dict loads, strictly
    m.load_state_dict({"grids": torch.randn(5, 12, 3, 7, 6), "rgb2gray_weight": torch.tensor([[0.299, 0.587, 0.114]])})


def test_identity_grids_return_the_input():
    m = bilagrid.BilateralGrid(2)
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand(2, 9, 11, 3, generator=g) * 1.6 - 0.3
    res = bilagrid.slice_image(m, rgb, torch.tensor([1, 0]))
    assert "rgb_affine_mats" not in res  # only on request
    assert float((res["rgb"] - rgb).abs().max()) <= 1e-6
    pts = torch.rand(50, 3, generator=g)
    res = bilagrid.slice(m, torch.rand(50, 2, generator=g), pts, torch.zeros(50, 1, dtype=torch.long), affine_mats=True)
    assert float((res["rgb"] - pts).abs().max()) <= 1e-6
    assert tuple(res["rgb_affine_mats"].shape) == (50, 3, 4)


def test_input_ranks_and_forward():
    m = bilagrid.BilateralGrid(3, 5, 7, 3)
    with torch.no_grad():
        m.grids += 0.1 * torch.randn(m.grids.shape, generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(2)
    xy, rgb = torch.rand(4, 6, 2, generator=g), torch.rand(4, 6, 3, generator=g)
    idx = torch.tensor([0, 2, 1, 1])
    out3 = bilagrid.slice(m, xy, rgb, idx.reshape(4, 1, 1).expand(4, 6, 1))["rgb"]
    out4 = bilagrid.slice(m, xy.reshape(4, 2, 3, 2), rgb.reshape(4, 2, 3, 3), idx.reshape(4, 1, 1, 1))["rgb"]
    assert torch.allclose(out3, out4.reshape(4, 6, 3), atol=1e-6)
    mats = m(xy, rgb, idx)
    assert tuple(mats.shape) == (4, 6, 3, 4)
    assert torch.allclose(bilagrid.color_affine_transform(mats, rgb), out3, atol=1e-6)
    # gradient reaches xy on the torch path
    xy_g = xy.clone().requires_grad_(True)
    bilagrid.slice(m, xy_g, rgb, idx.reshape(4, 1, 1))["rgb"].sum().backward()
    assert xy_g.grad is not None and float(xy_g.grad.abs().max()) > 0


def test_argument_errors():
    m = bilagrid.BilateralGrid(2)
    rgb, xy = torch.rand(4, 5, 3), torch.rand(4, 5, 2)
    with pytest.raises(ValueError):
        bilagrid.slice(m, xy.reshape(20, 2), rgb, torch.zeros(4, 1, 1, dtype=torch.long))  # rank mismatch
    with pytest.raises(ValueError):
        bilagrid.slice(m, xy[:, :4], rgb, torch.zeros(4, 1, 1, dtype=torch.long))  # leading shapes differ
    with pytest.raises(ValueError):
        bilagrid.slice_image(m, rgb, torch.zeros(4, dtype=torch.long))  # not [I, H, W, 3]
    with pytest.raises(ValueError):
        m(xy, rgb)  # idx is required below 5-D
    with pytest.raises(ValueError, match="slice_image"):
        bilagrid.slice(m, None, rgb, torch.zeros(4, 1, 1, dtype=torch.long))
    with pytest.raises(IndexError):
        bilagrid.slice(m, xy, rgb, torch.tensor([0, 1, 2, 0]).reshape(4, 1, 1), check_index=True)
    with pytest.raises(IndexError):
        bilagrid.slice_image(m, torch.rand(1, 4, 5, 3), torch.tensor([-1]), check_index=True)


def test_public_surface():
    import gsplat_amd

    assert gsplat_amd.BilateralGrid is bilagrid.BilateralGrid
    assert gsplat_amd.bilagrid is bilagrid
    assert gsplat_amd.total_variation_loss is total_variation_loss
