"""GPU: the depth-supervision kernels of csrc/depth_loss.hip through their public entry points - depth_l1_loss,
binocular_disparity_l1, pearson_depth_loss, sampled_depth_l1_loss - on every case of tests/_depth_cases.py, against the float64
references and within the bounds derived there (per element for the disparity gradients, per family twice the reference's own
float32 error for the reduced scalars and the Pearson / sampled gradients). Also: the kernels ran (`calls`), gradients land only
where selected, a strided [C, H, W, 4] view gives the bits of its contiguous copy, losses and dense gradients repeat bit for
bit, a masked forward + backward reads nothing back, the torch fallbacks agree, and the trainer's combination with
rasterization(render_mode="RGB+ED") and photometric_loss back-propagates to the means. tests/test_depth_losses.py checks the
references, the bounds and the argument checks without a GPU.

Largest error observed on an MI355X: disparity gradients 0.062 of the per-element bound (the kernels form each term in double
and round once); losses at most 0.50 of their family's bound - a loss is the float64 value rounded once to float32, so its error
cannot exceed the float32 reference's own, which is half the bound (bin / zeros 2.8e-8 of 5.6e-8); Pearson loss error at most
9.3e-10, 4.8e-8 in the anti-correlated family; Pearson gradient at most 5.3e-8 of max |grad| (bounds 1.3e-7 to 1.1e-5); sampled
gradient at most 3.2e-7 (bound 2.8e-6; a float atomic sum, so the last digits move between runs)."""
import pytest
import torch

import _depth_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from gsplat_amd import losses

    return losses


def _leaf_and_view(case):
    """(leaf, pred, gt, mask): pred is what the loss receives - the leaf itself, or channel 3 of a NaN-filled [C, H, W, 4] leaf."""
    pred, gt, mask = dc.place_dense(case, DEV)
    if case.layout == "contiguous":
        pred.requires_grad_(True)
        return pred, pred, gt, mask
    wide = pred._base.requires_grad_(True)
    return wide, wide[..., 3:4], gt, mask


def _dense_loss(L, case, pred, gt, mask):
    if case.loss == "l1":
        return L.depth_l1_loss(pred, gt, dc.SCALE)
    if case.loss == "bin":
        return L.binocular_disparity_l1(pred, gt, mask)
    return L.pearson_depth_loss(pred, gt, mask)


def _run_dense(L, case):
    leaf, pred, gt, mask = _leaf_and_view(case)
    loss = _dense_loss(L, case, pred, gt, mask)
    loss.backward()
    grad = leaf.grad
    if case.layout == "channel3":
        assert bool((grad[..., :3] == 0).all())  # the NaN channels took no part
        grad = grad[..., 3:4]
    return loss.detach(), grad


def _fused_class(L, loss):
    return L._FusedPearsonDepth if loss == "pearson" else L._FusedDisparityL1


@pytest.mark.parametrize("loss_kind", ["l1", "bin", "pearson"])
def test_every_dense_case_against_float64(L, loss_kind):
    cases = [c for c in dc.dense_cases() if c.loss == loss_kind]
    cls = _fused_class(L, loss_kind)
    before, worst = cls.calls, {}
    for case in cases:
        loss, grad = _run_dense(L, case)
        le, ge = dc.check(case, loss.cpu(), grad.cpu())
        print(f"{case.name:48s} loss error {le:.2e}  gradient {ge:.2e}")
        worst[dc.family_of(case)] = tuple(max(a, b) for a, b in zip(worst.get(dc.family_of(case), (0.0, 0.0)), (le, ge)))
        pred, gt, mask = dc.dense_inputs(case)
        if mask is not None:  # gradients land only where selected
            assert bool((grad.cpu().reshape(case.shape)[(mask == 0).expand(case.shape)] == 0).all()), case.name
        if loss_kind == "bin":
            assert bool((grad.cpu().reshape(case.shape)[(pred.abs() <= dc.BIN_EPS) | (gt.abs() <= dc.BIN_EPS)] == 0).all())
        if loss_kind == "l1":
            assert bool((grad.cpu().reshape(case.shape)[pred <= 0] == 0).all()), case.name
    print("largest error per family (loss absolute, gradient as documented):", worst, dc.family_bounds())
    assert cls.calls - before == sum(1 for c in cases if c.shape != (0,))  # every non-empty case took the kernels


def _run_sampled(L, case, view=False):
    dm, pts, dgt = (t.to(DEV) for t in dc.sampled_inputs(case))
    if view:
        wide = torch.full(case.shape + (4,), float("nan"), device=DEV)
        wide[..., 3] = dm
        leaf = wide.requires_grad_(True)
        loss = L.sampled_depth_l1_loss(leaf[..., 3:4], pts, dgt, dc.SCALE)
    else:
        leaf = dm.clone().requires_grad_(True)
        loss = L.sampled_depth_l1_loss(leaf, pts, dgt, dc.SCALE)
    loss.backward()
    return loss.detach(), (leaf.grad[..., 3] if view else leaf.grad)


def test_every_sampled_case_against_float64(L):
    before = L._FusedSampledDepthL1.calls
    for case in dc.sampled_cases():
        loss, grad = _run_sampled(L, case)
        le, ge = dc.check(case, loss.cpu(), grad.cpu())
        print(f"{case.name:32s} loss error {le:.2e}  gradient error / max |grad| {ge:.2e}")
        if case.family == "defined":  # an unchanged loss value (checked above), finite gradients, 0 at the zero block's taps
            by, bx = dc.zero_block(case.shape)
            assert bool(torch.isfinite(grad).all()) and bool((grad[:, by:by + 2, bx:bx + 2] == 0).all()), case.name
    assert L._FusedSampledDepthL1.calls - before == len(dc.sampled_cases())


def test_strided_view_gives_the_bits_of_its_contiguous_copy(L):
    for case in dc.dense_cases():
        if case.layout != "channel3":
            continue
        loss_v, grad_v = _run_dense(L, case)
        loss_c, grad_c = _run_dense(L, case._replace(layout="contiguous"))
        assert dc.bits_equal(loss_v, loss_c) and dc.bits_equal(grad_v, grad_c), case.name
    for case in dc.sampled_cases():
        if case.M == 1:  # one point: no two atomic adds meet, so the scattered gradient is bit-exact as well
            loss_v, grad_v = _run_sampled(L, case, view=True)
            loss_c, grad_c = _run_sampled(L, case)
            assert dc.bits_equal(loss_v, loss_c) and dc.bits_equal(grad_v, grad_c), case.name
        else:
            assert dc.bits_equal(_run_sampled(L, case, view=True)[0], _run_sampled(L, case)[0]), case.name


def test_losses_and_dense_gradients_repeat_bit_for_bit(L):
    span, _, cap_n = dc.launch_edges()
    names = {f"{k}-{n}-d3-{m}-contiguous" for k, m in (("l1", "none"), ("bin", "bool"), ("pearson", "bool")) for n in (span + 1, cap_n + 1)}
    cases = [c for c in dc.dense_cases() if c.name in names]
    assert len(cases) == 6
    for case in cases:
        first = _run_dense(L, case)
        for _ in range(3):
            again = _run_dense(L, case)
            assert dc.bits_equal(first[0], again[0]) and dc.bits_equal(first[1], again[1]), case.name
    for case in dc.sampled_cases():  # the loss always; the scattered gradient is a float atomic sum where points share a tap
        assert dc.bits_equal(_run_sampled(L, case)[0], _run_sampled(L, case)[0]), case.name
    # no two points share a tap: one point in every fourth cell of a 37 x 53 map
    g = torch.Generator().manual_seed(5)
    ys, xs = torch.meshgrid(torch.arange(0, 35, 4), torch.arange(0, 51, 4), indexing="ij")
    pts = (torch.stack([xs, ys], -1).reshape(1, -1, 2) + 0.125 + 0.75 * torch.rand(1, xs.numel(), 2, generator=g)).to(DEV)
    dm = (3 + torch.rand(1, 37, 53, generator=g)).to(DEV)
    dgt = (3 + torch.rand(1, xs.numel(), generator=g)).to(DEV)
    grads = []
    for _ in range(4):
        x = dm.clone().requires_grad_(True)
        L.sampled_depth_l1_loss(x, pts, dgt, dc.SCALE).backward()
        grads.append(x.grad)
    assert int((grads[0] != 0).sum()) == 4 * xs.numel() and all(dc.bits_equal(grads[0], g2) for g2 in grads[1:])


def test_incoming_gradient_is_multiplied_on_the_device(L):
    by_name = {c.name: c for c in dc.dense_cases()}
    for name in ("l1-65-d3-none-contiguous", "bin-2x7x9-zeros-f32-contiguous", "pearson-2x7x9-d20-bcast-contiguous"):
        case = by_name[name]
        _, once = _run_dense(L, case)
        leaf, pred, gt, mask = _leaf_and_view(case)
        (-4.0 * _dense_loss(L, case, pred, gt, mask)).backward()
        assert torch.equal(leaf.grad, -4.0 * once), name  # a power of two: the same roundings (0 and -0 compare equal)
    with torch.no_grad():  # nothing is saved for a forward that needs no gradient; an unused loss gives no gradient
        pred, gt, mask = dc.place_dense(by_name["pearson-65-d3-bool-contiguous"], DEV)
        assert not L.pearson_depth_loss(pred, gt, mask).requires_grad


def test_nothing_is_read_back(L):
    """A masked forward + backward of every loss under torch's synchronisation debug mode: any device-to-host read raises."""
    by_name = {c.name: c for c in dc.dense_cases()}
    names = ["l1-1025-d3-none-contiguous", "bin-2x7x9-zeros-bool-contiguous", "bin-2x7x9-zeros-u8-contiguous",
             "bin-2x7x9-zeros-f32-contiguous", "bin-2x7x9-zeros-bcast-contiguous", "bin-2x7x9-zeros-zeros-contiguous",
             "pearson-2x7x9-d20-bool-contiguous", "pearson-2x7x9-d20-u8-contiguous", "pearson-2x7x9-d20-f32-contiguous",
             "pearson-2x7x9-d20-bcast-contiguous", "pearson-2x7x9-d20-one-contiguous", "pearson-2x7x9x1-d3-u8-channel3"]
    sampled = dc.sampled_cases()[5]
    placed = [(by_name[n],) + _leaf_and_view(by_name[n]) for n in names]
    dm, pts, dgt = (t.to(DEV) for t in dc.sampled_inputs(sampled))
    dm.requires_grad_(True)
    for case, leaf, pred, gt, mask in placed:  # first use outside the mode: code objects load here
        _dense_loss(L, case, pred, gt, mask).backward()
        leaf.grad = None
    L.sampled_depth_l1_loss(dm, pts, dgt).backward()
    dm.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = []
        for case, leaf, pred, gt, mask in placed:
            loss = _dense_loss(L, case, pred, gt, mask)
            (2.0 * loss).backward()
            losses.append(loss.detach())
        loss = L.sampled_depth_l1_loss(dm, pts, dgt, dc.SCALE)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(leaf.grad[..., 3:4] if case.layout == "channel3" else leaf.grad).all())
               for case, leaf, *_ in placed) and bool(torch.isfinite(dm.grad).all())
    with pytest.raises(RuntimeError):  # the mode does catch a host read on this build
        torch.cuda.set_sync_debug_mode("error")
        try:
            float(losses[0])
        finally:
            torch.cuda.set_sync_debug_mode("default")


def test_fallbacks_agree_with_the_fused_path(L):
    """float64 inputs and a gt / points that require grad take the torch compositions, on the GPU as well; they meet the same
    references. The float64 composition lies far inside the bounds. A float32 composition on the GPU is a second float32
    evaluation, summed in another order than the CPU one whose error defines the family bounds (with their factor 2): what
    carries a reduced quantity is held to twice the bound - each of the two float32 evaluations may be one reference error away
    from the float64 value. The disparity gradients are elementwise and keep their per-element bound."""
    by_name = {c.name: c for c in dc.dense_cases()}
    counters = (L._FusedPearsonDepth, L._FusedDisparityL1, L._FusedSampledDepthL1)
    before = [c.calls for c in counters]
    for name in ("l1-1025-zeros-none-contiguous", "bin-2x7x9-zeros-bcast-contiguous", "bin-1025-tiny-none-contiguous",
                 "pearson-1025-d20-none-contiguous", "pearson-2x7x9-d20-u8-contiguous", "pearson-2x7x9-d20-one-contiguous"):
        case = by_name[name]
        pred, gt, mask = dc.place_dense(case, DEV)
        x = pred.double().requires_grad_(True)
        loss = _dense_loss(L, case, x, gt.double(), mask)
        loss.backward()
        dc.check(case, loss.detach().cpu(), x.grad.cpu(), share=0.01 if dc.family_bounds()[dc.family_of(case)][0] > 0 else 1.0)
        x = pred.clone().requires_grad_(True)
        y = gt.clone().requires_grad_(True)
        loss = _dense_loss(L, case, x, y, mask)
        loss.backward()
        assert y.grad is not None
        dc.check(case, loss.detach().cpu(), x.grad.cpu(), share=2.0, element_share=1.0)
    case = dc.sampled_cases()[6]
    dm, pts, dgt = (t.to(DEV) for t in dc.sampled_inputs(case))
    for dtype, grad_points in ((torch.float64, False), (torch.float32, True)):
        x = dm.to(dtype).requires_grad_(True)
        p = pts.to(dtype).requires_grad_(grad_points)
        loss = L.sampled_depth_l1_loss(x, p, dgt.to(dtype), dc.SCALE)
        loss.backward()
        assert (p.grad is not None) == grad_points
        dc.check(case, loss.detach().cpu(), x.grad.cpu(), share=2.0 if dtype == torch.float32 else 1.0)
    assert [c.calls for c in counters] == before  # none of these took the kernels


def test_trainer_combination_with_an_expected_depth_render(L):
    """examples/simple_trainer.py with depth_loss=True: an RGB+ED render, photometric_loss on its colours plus
    sampled_depth_l1_loss on renders[..., 3:4], read in place. The gradients on the means are finite, and those of the depth
    term equal the torch composition's within the sampled-gradient bound propagated by the same backward: the two cotangents on
    the render differ by at most delta = bound * max |cotangent| per tap, and |B delta| <= delta * sum_j |B_ij| over the taps j,
    with B the (linear) backward of the render, evaluated one tap at a time."""
    import gsplat_amd
    from _util import make_scene

    sc, W, H = make_scene(N=400, C=1, width=64, height=48, seed=3, device=DEV)
    means = sc["means"].clone().requires_grad_(True)
    renders, alphas, _ = gsplat_amd.rasterization(means, sc["quats"], sc["scales"], sc["opacities"], sc["colors"], sc["viewmats"],
                                                 sc["Ks"], W, H, render_mode="RGB+ED")
    assert renders.shape == (1, H, W, 4)
    depth = renders[..., 3:4]
    assert not depth.is_contiguous()
    covered = (alphas[0, :-1, :-1, 0] > 0.5).nonzero().cpu()  # test set-up: points over covered pixels
    assert len(covered) >= 8
    pick = covered[torch.linspace(0, len(covered) - 1, 8).long()]
    pts = (torch.stack([pick[:, 1], pick[:, 0]], -1).float() + torch.tensor([0.25, 0.5])).reshape(1, 8, 2).to(DEV)
    dgt = L._sample_depth_torch(depth.detach()[..., 0], pts) * 1.1
    target = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
    before = L._FusedSampledDepthL1.calls
    loss = L.photometric_loss(renders[..., :3].permute(0, 3, 1, 2), target) + 0.1 * L.sampled_depth_l1_loss(depth, pts, dgt, dc.SCALE)
    assert L._FusedSampledDepthL1.calls == before + 1
    (g_full,) = torch.autograd.grad(loss, means, retain_graph=True)
    assert bool(torch.isfinite(g_full).all()) and float(g_full.abs().max()) > 0
    # the depth term alone, through both compositions, on the same graph
    (v_fused,) = torch.autograd.grad(L.sampled_depth_l1_loss(depth, pts, dgt, dc.SCALE), renders, retain_graph=True)
    (v_torch,) = torch.autograd.grad(L.sampled_depth_l1_loss_torch(depth.double(), pts.double(), dgt.double(), dc.SCALE), renders,
                                     retain_graph=True)
    assert bool((v_fused[..., :3] == 0).all()) and int((v_torch[..., 3] != 0).sum()) > 8
    delta = dc.family_bounds()[("sampled", "pos")][1] * float(v_torch.abs().max())
    assert float((v_fused - v_torch).abs().max()) <= delta
    (g_fused,) = torch.autograd.grad(renders, means, grad_outputs=v_fused, retain_graph=True)
    (g_torch,) = torch.autograd.grad(renders, means, grad_outputs=v_torch, retain_graph=True)
    reach = torch.zeros_like(g_torch)
    for y, x in (v_torch[0, :, :, 3] != 0).nonzero().tolist():
        tap = torch.zeros_like(renders)
        tap[0, y, x, 3] = 1.0
        reach += torch.autograd.grad(renders, means, grad_outputs=tap, retain_graph=True)[0].abs()
    assert float(g_torch.abs().max()) > 0 and bool(torch.isfinite(g_fused).all())
    excess = ((g_fused - g_torch).abs() - delta * reach).max()
    print("depth term on the means: max |fused - torch|", float((g_fused - g_torch).abs().max()), "max allowed", float((delta * reach).max()))
    assert float(excess) <= 0.0
