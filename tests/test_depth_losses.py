"""CPU: the depth-supervision losses without a GPU - the pinned reference (tests/golden/depth_losses_ref.npz, written by
tools/pin_depth_losses_against_reference.py from the reference's gsplat/losses.py and the trainers' grid_sample block) holds
every case of tests/_depth_cases.py; the `*_torch` compositions reproduce its losses and gradients; the float32 restatements
lie within half of every bound of _depth_cases and one wrong restatement per family falls outside; the gradient this project
defines at depths <= 0 is 0 where the reference's is NaN; the error contract, the exports and the argument checks of the
gsx_depth_* entry points, which run before any launch. tests/test_gpu_depth_losses.py holds the kernels to the same bounds."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _depth_cases as dc
from gsplat_amd import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_STRIDE = 4099  # of the pin tool: large cases keep every GRAD_STRIDE-th gradient element


@pytest.fixture(scope="module")
def pinned():
    return np.load(os.path.join(ROOT, "tests", "golden", "depth_losses_ref.npz"))


def _torch_composition(case, dtype):
    """(loss, grad) of the `*_torch` composition for `case` in `dtype`."""
    if isinstance(case, dc.SampledCase):
        dm, pts, dgt = dc.sampled_inputs(case)
        x = dm.to(dtype).clone().requires_grad_(True)
        val = L.sampled_depth_l1_loss_torch(x, pts.to(dtype), dgt.to(dtype), dc.SCALE)
    else:
        pred, gt, mask = dc.dense_inputs(case)
        x = pred.to(dtype).clone().requires_grad_(True)
        if case.loss == "l1":
            val = L.depth_l1_loss_torch(x, gt.to(dtype), dc.SCALE)
        elif case.loss == "bin":
            val = L.binocular_disparity_l1_torch(x, gt.to(dtype), mask)
        else:
            val = L.pearson_depth_loss_torch(x, gt.to(dtype), mask)
    val.backward()
    return val.detach(), x.grad


def test_launch_edges_come_from_the_library():
    span, cap, cap_n = dc.launch_edges()
    from gsplat_amd import _cabi

    blocks = _cabi._lib.gsx_depth_blocks
    assert blocks(span) == 1 and blocks(span + 1) == 2 and blocks(cap_n) == cap == blocks(cap_n + 1) == blocks(1 << 50)
    assert blocks(0) == 1 and blocks(-5) == 1
    counts = [blocks(n) for n in (0, 1, span, span + 1, 3 * span, cap_n - 1, cap_n, cap_n + 1, 1 << 31, 1 << 62)]
    assert counts == sorted(counts) and max(counts) == cap  # monotone and capped
    assert set(dc.dense_counts()) >= {0, 1, 2, 3, 63, 64, 65, span - 1, span, span + 1, cap_n + 1}


def test_the_fixture_holds_every_case(pinned):
    span = dc.launch_edges()[0]
    for case in dc.dense_cases():
        pred, gt, mask = dc.dense_inputs(case)
        for key in ("loss32", "loss64", "grad32", "grad64"):
            assert f"{case.name}/{key}" in pinned.files, (case.name, key)
        if pred.numel() <= span + 1:  # the seeded builders still give the tensors the reference was run on
            assert np.array_equal(pinned[f"{case.name}/pred"], pred.numpy()) and np.array_equal(pinned[f"{case.name}/gt"], gt.numpy(), equal_nan=True)
            assert (mask is None) == (f"{case.name}/mask" not in pinned.files)
            if mask is not None:
                assert np.array_equal(pinned[f"{case.name}/mask"], mask.numpy())
        else:
            sums = pinned[f"{case.name}/sum"]
            assert sums[0] == float(pred.double().sum()) and sums[1] == float(gt.double().sum())
    for case in dc.sampled_cases():
        for key, t in zip(("map", "points", "depths_gt"), dc.sampled_inputs(case)):
            assert np.array_equal(pinned[f"{case.name}/{key}"], t.numpy()), (case.name, key)


def test_the_cases_cover_what_they_claim():
    cases = dc.dense_cases()
    assert {c.family for c in cases} == {"d3", "d20", "d100", "const", "anti", "zeros", "tiny"}
    assert {c.mask for c in cases} == {"none"} | set(dc.MASKS3) and {c.layout for c in cases} == {"contiguous", "channel3"}
    by_name = {c.name: c for c in cases}
    assert dc.selected_count(by_name["pearson-2x7x9-d20-one-contiguous"]) == 1
    assert dc.selected_count(by_name["pearson-2x7x9-d20-two-contiguous"]) == 2
    assert dc.selected_count(by_name["pearson-2x7x9-d20-zeros-contiguous"]) == 0
    assert dc.dense_inputs(by_name["pearson-2x7x9-d20-bcast-contiguous"])[2].shape == (2, 1, 9)
    for c in cases:
        pred, gt, mask = dc.dense_inputs(c)
        if c.family == "const":  # the clamp of the Pearson denominator is active, in float64 too
            assert bool((pred == 3.0).all()) and float(dc.ref_dense(c)[0]) == 1.0 or pred.numel() < 2
        if c.family == "anti" and pred.numel() >= 63:
            assert float(dc.ref_dense(c)[0]) > 1.9
        if c.family in ("zeros", "tiny") and pred.numel() >= 63:
            special = 0.0 if c.family == "zeros" else 5e-8
            assert bool((pred == special).any()) and bool((pred < 0).any()) and bool((gt == -special).any())
        if c.loss != "pearson":  # no counted pair ties: the sign of 1/p - 1/g is settled in float32 as well
            d = 1.0 / pred.double() - 1.0 / gt.double()
            ok = (pred.abs() > 1e-7) & (gt.abs() > 1e-7)
            assert not ok.any() or float((d[ok].abs() / (1.0 / pred.double()[ok]).abs()).min()) > 64 * dc.EPS, c.name
    for c in dc.sampled_cases():
        dm, pts, dgt = dc.sampled_inputs(c)
        C, H, W = c.shape
        x, y = pts[..., 0], pts[..., 1]
        if c.family == "pos":
            assert bool((dm > 0).all()) and bool(((x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)).all())
            if c.M >= 64:
                assert bool(((x == W - 1) | (y == H - 1)).any()) and bool(((x == x.round()) & (y == y.round())).any())
                cell = (x.floor() == 0) & (y.floor() == 0) & (x > 0) & (y > 0)
                assert int(cell.sum()) >= 2  # several points share one pixel's taps
        else:
            by, bx = dc.zero_block(c.shape)
            assert bool((dm[:, by:by + 2, bx:bx + 2] == 0).all())
            assert bool(((x > bx) & (x < bx + 1) & (y > by) & (y < by + 1)).any())
            assert bool(((x < -1) | (x > W) | (y < -1) | (y > H)).any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_torch_compositions_match_the_pinned_reference(pinned, dtype):
    """Losses and gradients of the reference itself. Where the reference's gradient is NaN (a predicted depth of exactly 0) ours
    is 0; Pearson cases with fewer than three samples compare the loss only (r = +-1: the gradient is rounding noise)."""
    tag = "32" if dtype == torch.float32 else "64"
    tol = 1e-5 if dtype == torch.float32 else 1e-13
    span = dc.launch_edges()[0]
    for case in dc.dense_cases() + dc.sampled_cases():
        loss, grad = _torch_composition(case, dtype)
        ref_loss, ref_grad = float(pinned[f"{case.name}/loss{tag}"]), torch.from_numpy(pinned[f"{case.name}/grad{tag}"])
        if math.isnan(ref_loss):
            assert case.loss == "l1" and case.shape == (0,) and math.isnan(loss.item())
            continue
        dense = isinstance(case, dc.DenseCase)
        if dense and dc.degenerate(case):
            assert abs(loss.item() - ref_loss) <= (4e-7 if dtype == torch.float32 else 1e-13), (case.name, loss.item(), ref_loss)
            assert bool(torch.isfinite(grad).all())
            continue
        assert abs(loss.item() - ref_loss) <= tol * max(1.0, abs(ref_loss)), (case.name, loss.item(), ref_loss)
        if dense and grad.numel() > span + 1:
            grad = grad.reshape(-1)[::GRAD_STRIDE]
        nan = torch.isnan(ref_grad)
        assert bool(torch.isfinite(grad).all()) and bool((grad[nan] == 0).all()), case.name
        if dense:
            pred = dc.dense_inputs(case)[0]
            assert not nan.any() or (case.loss == "l1" and bool((pred[nan.reshape(pred.shape)] == 0).all())), case.name
        if (~nan).any():
            err = float((grad - ref_grad)[~nan].abs().max())
            assert err <= tol * max(1e-30, float(ref_grad[~nan].abs().max())), (case.name, err)


def test_float32_restatements_lie_within_half_of_every_bound():
    """The bounds are twice the reference's own float32 error per family, so this is their definition - and the check that no
    family's bound is empty where an error exists, and that the per-element bound has its factor 2 as well."""
    bounds = dc.family_bounds()
    assert set(bounds) == {dc.family_of(c) for c in dc.dense_cases() + dc.sampled_cases()}
    for case in dc.dense_cases() + dc.sampled_cases():
        loss, grad = dc.ref_sampled(case, torch.float32) if isinstance(case, dc.SampledCase) else dc.ref_dense(case, torch.float32)
        dc.check(case, loss, grad, share=0.5)
    for family, (lb, gb) in bounds.items():
        assert math.isfinite(lb) and math.isfinite(gb)
        assert lb > 0 or family == ("pearson", "const"), family  # that loss is exactly 1 in either precision
        assert lb < 1e-6 and gb < 2e-5, (family, lb, gb)


def test_one_wrong_restatement_per_family_falls_outside():
    by_name = {c.name: c for c in dc.dense_cases() + dc.sampled_cases()}
    span = dc.launch_edges()[0]
    # Pearson from raw float32 moments at depths of 20 +- 0.5
    case = by_name[f"pearson-{span + 1}-d20-none-contiguous"]
    loss, grad = dc.ref_dense(case, torch.float32, "raw")
    lb, gb = dc.family_bounds()[dc.family_of(case)]
    assert dc.loss_error(loss, case) > lb or dc.grad_error(grad, case) > gb
    with pytest.raises(AssertionError):
        dc.check(case, loss, grad)
    # align_corners=False sampling
    case = by_name["sampled-2x16x16-65-pos"]
    loss, grad = dc.ref_sampled(case, torch.float64, False)
    with pytest.raises(AssertionError):
        dc.check(case, loss, grad)
    assert dc.grad_error(grad, case) > dc.family_bounds()[dc.family_of(case)][1]
    # a masked mean divided by all elements
    case = by_name["bin-2x7x9-zeros-bool-contiguous"]
    loss, grad = dc.ref_dense(case, torch.float64, "all")
    assert dc.loss_error(loss, case) > dc.family_bounds()[dc.family_of(case)][0] and dc.element_ratio(grad, case) > 1
    with pytest.raises(AssertionError):
        dc.check(case, loss, grad)


def test_gradient_is_zero_where_the_reference_gives_nan():
    """The departure: d/dx where(x > 0, 1 / x, 0) is 0 at x <= 0. The loss values are the reference's."""
    pred = torch.tensor([0.0, 2.0, -1.0, 4.0, 0.0], requires_grad=True)
    gt = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0])
    loss = L.depth_l1_loss(pred, gt, 2.0)
    loss.backward()
    assert loss.item() == pytest.approx(2.0 * (1.0 + 0.5 + 1.0 + 0.25 + 0.0) / 5)
    assert pred.grad.tolist() == pytest.approx([0.0, 2.0 / 5 / 4, 0.0, -2.0 / 5 / 16, 0.0])
    # the reference's formula on the same input: the same value, NaN at the zeros
    x = pred.detach().clone().requires_grad_(True)
    disp = torch.where(x > 0.0, 1.0 / x, torch.zeros_like(x))
    disp_gt = torch.where(gt > 0.0, 1.0 / gt, torch.zeros_like(gt))
    ref = torch.nn.functional.l1_loss(disp, disp_gt) * 2.0
    ref.backward()
    assert ref.item() == loss.item() and torch.isnan(x.grad).tolist() == [True, False, False, False, True]
    # sampled: an uncovered pixel block and a point off the image
    dm = torch.full((1, 4, 4, 1), 2.0)
    dm[0, :2, :2] = 0.0
    dm.requires_grad_(True)
    pts = torch.tensor([[[0.5, 0.5], [2.5, 2.5], [9.0, 1.0]]])
    loss = L.sampled_depth_l1_loss(dm, pts, torch.ones(1, 3))
    loss.backward()
    assert loss.item() == pytest.approx((1.0 + 0.5 + 1.0) / 3) and bool(torch.isfinite(dm.grad).all())
    assert float(dm.grad[0, :2, :2].abs().sum()) == 0.0 and float(dm.grad[0, 2:, 2:].sum()) == pytest.approx(1.0 / 3 / 4)


def test_degenerate_inputs_and_broadcast_masks():
    x = torch.tensor([[3.0, 4.0, 6.0]], requires_grad=True)
    y = torch.tensor([[1.0, 2.0, 2.5]])
    for mask in (torch.zeros(1, 3), torch.tensor([[0, 1, 0]]), torch.zeros(1, 3, dtype=torch.bool)):
        loss = L.pearson_depth_loss(x, y, mask)  # fewer than two samples: 0 with zero gradient
        loss.backward()
        assert loss.item() == 0.0 and float(x.grad.abs().sum()) == 0.0
        loss = L.binocular_disparity_l1(x, y, torch.zeros_like(mask))  # nothing counts: a differentiable 0
        loss.backward()
        assert loss.item() == 0.0 and float(x.grad.abs().sum()) == 0.0
    assert float(L.pearson_depth_loss(torch.zeros(0), torch.zeros(0))) == 0.0
    assert float(L.binocular_disparity_l1(torch.zeros(0), torch.zeros(0))) == 0.0
    assert float(L.sampled_depth_l1_loss(torch.ones(1, 3, 3), torch.zeros(1, 0, 2), torch.zeros(1, 0)).isnan())  # M == 0: a mean of nothing
    p, g = torch.rand(2, 3, 5) + 1, torch.rand(2, 3, 5) + 1
    m = torch.rand(2, 1, 5) > 0.4
    assert float(L.pearson_depth_loss(p, g, m)) == pytest.approx(float(L.pearson_depth_loss(p, g, m.expand(2, 3, 5).float())))
    assert float(L.binocular_disparity_l1(p, g, m)) == pytest.approx(float(L.binocular_disparity_l1(p, g, m.expand(2, 3, 5).to(torch.uint8))))


def test_error_contract():
    a, b = torch.ones(2, 3), torch.ones(3, 2)
    with pytest.raises(ValueError, match=r"binocular_disparity_l1: pred_depth shape .* != gt_depth shape .*\. Shapes must match\."):
        L.binocular_disparity_l1(a, b)
    with pytest.raises(ValueError, match=r"pearson_depth_loss: pred_depth shape .* != gt_depth shape .*\. Shapes must match\."):
        L.pearson_depth_loss(a, b)
    with pytest.raises(ValueError, match="Shapes must match"):
        L.pearson_depth_loss_torch(a, b)
    with pytest.raises(ValueError, match="Shapes must match"):
        L.binocular_disparity_l1_torch(a, b)
    with pytest.raises(ValueError, match="depth map"):
        L.sampled_depth_l1_loss(torch.ones(2, 4, 4, 3), torch.zeros(2, 5, 2), torch.ones(2, 5))
    with pytest.raises(ValueError, match="points"):
        L.sampled_depth_l1_loss(torch.ones(2, 4, 4, 1), torch.zeros(1, 5, 2), torch.ones(2, 5))
    with pytest.raises(ValueError, match="depths_gt"):
        L.sampled_depth_l1_loss(torch.ones(2, 4, 4), torch.zeros(2, 5, 2), torch.ones(2, 4))


def test_package_exports_the_new_names():
    import gsplat_amd
    from gsplat_amd import _cabi

    for name in ("depth_l1_loss", "binocular_disparity_l1", "pearson_depth_loss", "sampled_depth_l1_loss", "depth_l1_loss_torch",
                 "binocular_disparity_l1_torch", "pearson_depth_loss_torch", "sampled_depth_l1_loss_torch"):
        assert getattr(gsplat_amd, name) is getattr(gsplat_amd.losses, name) and name in dir(gsplat_amd)
    assert {"gsx_depth_blocks", "gsx_depth_pearson_fwd", "gsx_depth_pearson_bwd", "gsx_depth_disparity_fwd",
            "gsx_depth_disparity_bwd", "gsx_depth_sampled_fwd", "gsx_depth_sampled_bwd"} <= set(_cabi.exported_symbols())
    assert gsplat_amd.build_config()["losses"] is False  # the reference's gaussian_losses op is not what this adds


def test_entry_points_refuse_bad_arguments():
    """GSX_REQUIRE of the gsx_depth_* entry points: reached before any launch, so this runs without a GPU."""
    from gsplat_amd import _cabi

    lib, err = _cabi._lib, _cabi._lib.gsx_last_error
    s, p = (ctypes.c_int64 * 4)(1, 1, 1, 1), 64  # p: a non-null address that is never read
    pf, pb, df, db = lib.gsx_depth_pearson_fwd, lib.gsx_depth_pearson_bwd, lib.gsx_depth_disparity_fwd, lib.gsx_depth_disparity_bwd
    assert pf(None, s, p, s, None, None, 0, 1, 1, 4, 4, p, p, p, None) == -1           # null pred
    assert pf(p, None, p, s, None, None, 0, 1, 1, 4, 4, p, p, p, None) == -1           # null strides
    assert pf(p, s, p, s, None, None, 0, 1, 1, 4, 4, p, p, None, None) == -1           # null record
    assert pf(p, s, p, s, None, None, 0, 1, 1, 4, 4, None, p, p, None) == -1           # null scratch
    assert pf(p, s, p, s, p, None, 0, 1, 1, 4, 4, p, p, p, None) == -1 and b"strides" in err()   # a mask without strides
    assert pf(p, s, p, s, p, s, 7, 1, 1, 4, 4, p, p, p, None) == -1 and b"mask dtype" in err()
    assert pf(p, s, p, s, None, None, 0, 1, 0, 4, 4, p, p, p, None) == -1 and b"empty" in err()
    assert pf(p, s, p, s, None, None, 0, 1 << 10, 1 << 10, 1 << 10, 2, p, p, p, None) == -1 and b"2^31" in err()
    assert pf(p, s, p, s, None, None, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, p, p, p, None) == -1 and b"2^31" in err()
    assert pb(p, s, p, s, None, None, 0, 1, 1, 4, 4, None, p, p, None) == -1           # null record
    assert pb(p, s, p, s, None, None, 0, 1, 1, 4, 4, p, None, p, None) == -1           # null incoming gradient
    assert pb(p, s, p, s, None, None, 0, 1, 1, 4, 4, p, p, None, None) == -1           # null gradient output
    assert df(p, s, p, s, None, None, 0, 1, 1, 4, 4, 2, 1.0, 1e-7, p, p, p, None) == -1 and b"mode" in err()
    assert df(p, s, p, s, p, s, 1, 1, 1, 4, 4, 0, 1.0, 0.0, p, p, p, None) == -1 and b"no mask" in err()  # depth_l1_loss with a mask
    assert df(p, s, p, s, None, None, 0, 1, 1, 4, 4, 0, float("inf"), 0.0, p, p, p, None) == -1
    assert df(p, s, p, s, None, None, 0, 1, 1, 4, 4, 1, 1.0, -1.0, p, p, p, None) == -1                  # eps < 0
    assert df(None, s, p, s, None, None, 0, 1, 1, 4, 4, 1, 1.0, 1e-7, p, p, p, None) == -1
    assert db(p, s, p, s, None, None, 0, 1, 1, 4, 4, 1, 1e-7, None, p, p, None) == -1
    assert db(p, s, p, s, None, None, 0, 1, 1, 4, 4, 3, 1e-7, p, p, p, None) == -1
    s3 = (ctypes.c_int64 * 3)(16, 4, 1)
    sf, sb = lib.gsx_depth_sampled_fwd, lib.gsx_depth_sampled_bwd
    assert sf(None, s3, 1, 4, 4, p, p, 5, 1.0, p, p, p, None) == -1                    # null map
    assert sf(p, s3, 1, 4, 4, None, p, 5, 1.0, p, p, p, None) == -1                    # null points
    assert sf(p, s3, 1, 4, 4, p, p, 0, 1.0, p, p, p, None) == -1 and b"empty" in err()  # M == 0 is the caller's (torch) case
    assert sf(p, s3, 1, 1 << 24, 4, p, p, 5, 1.0, p, p, p, None) == -1 and b"2^24" in err()
    assert sf(p, s3, 1 << 12, 1 << 10, 1 << 10, p, p, 5, 1.0, p, p, p, None) == -1 and b"2^31" in err()
    assert sf(p, s3, 1 << 16, 4, 4, p, p, 1 << 16, 1.0, p, p, p, None) == -1 and b"points" in err()
    assert sf(p, s3, 1, 4, 4, p, p, 5, float("nan"), p, p, p, None) == -1
    assert sb(p, s3, 1, 4, 4, p, p, 5, None, p, p, None) == -1                         # null record
    assert sb(p, s3, 1, 4, 4, p, p, 5, p, p, None, None) == -1                         # null gradient output
