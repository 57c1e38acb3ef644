"""gsplat_amd/losses.py: photometric_loss (lerp(l1, ssim_loss, ssim_lambda) with an optional mask), masked_l1, masked_ssim and
mse_loss against values the REFERENCE's gsplat/losses.py produced on the CPU (tests/golden/photometric_ref.npz, written by
tools/pin_photometric_against_reference.py): the torch composition on the CPU, the fused kernels of csrc/ssim.hip
(gsx_photometric_fwd / _bwd) on the MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from gsplat_amd.losses import _FusedPhotometric, l1_loss, masked_l1, masked_ssim, mse_loss, photometric_loss, ssim_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("a", "b", "c")  # (2, 3, 37, 53), (1, 1, 16, 16), (1, 3, 64, 96)
MASKS = ("none", "b1", "bc", "zeros", "ones")
LAMBDAS = (0.0, 0.2, 1.0)


def _golden():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "photometric_ref.npz")))
    aliases = json.loads(str(g.pop("aliases")))
    for key, holder in aliases.items():  # gradients stored once (the all-ones mask repeats the unmasked case, ...)
        g[key] = g[holder]
    return g


def _cases(g):
    for tag in SHAPES:
        for mname in MASKS:
            mask = None if mname == "none" else torch.from_numpy(g[f"{tag}_mask_{mname}"])
            for lam in LAMBDAS:
                yield tag, mname, lam, mask, f"{tag}_{mname}_{lam:g}"


def test_fixture_holds_every_case():
    g = _golden()
    keys = [key for *_, key in _cases(g)]
    assert len(keys) == 45
    for key in keys:
        for part in ("loss", "l1", "ssim", "grad"):
            assert f"{key}_{part}" in g, key
    assert abs(float(g["a_b1_0.2_loss"]) - 0.06591) < 1e-5


def test_torch_composition_matches_the_reference_outputs():
    g = _golden()
    for tag, mname, lam, mask, key in _cases(g):
        x = torch.from_numpy(g[f"{tag}_x"]).requires_grad_(True)
        y = torch.from_numpy(g[f"{tag}_y"])
        loss, l1, ssim = photometric_loss(x, y, lam, mask, return_parts=True)
        assert not l1.requires_grad and not ssim.requires_grad
        loss.backward()
        ref = torch.from_numpy(g[f"{key}_grad"])
        d_loss, d_grad = abs(float(loss.detach()) - float(g[f"{key}_loss"])), float((x.grad - ref).abs().max())
        print(key, "loss", float(loss.detach()), "|d loss|", d_loss, "max |d grad|", d_grad, "max |ref grad|", float(ref.abs().max()))
        assert d_loss < 2e-6, key
        assert abs(float(l1.detach()) - float(g[f"{key}_l1"])) < 2e-6 and abs(float(ssim.detach()) - float(g[f"{key}_ssim"])) < 2e-6, key
        assert d_grad <= 1e-6 + 1e-4 * float(ref.abs().max()), key
        assert torch.equal(photometric_loss(x.detach(), y, lam, mask), loss.detach()), key  # return_parts only adds outputs
        if mask is not None:
            assert bool((x.grad[(mask == 0).expand_as(x)] == 0).all()), key


def test_masked_l1_masked_ssim_and_mse_match_the_reference_outputs():
    g = _golden()
    for tag in SHAPES:
        x, y = torch.from_numpy(g[f"{tag}_x"]), torch.from_numpy(g[f"{tag}_y"])
        assert torch.equal(mse_loss(x, y), (x - y) ** 2)
        for mname in MASKS[1:]:
            mask = torch.from_numpy(g[f"{tag}_mask_{mname}"])
            for m in (mask, mask != 0) if mname != "bc" else (mask,):  # a bool mask is the same mask where the values are 0 / 1
                a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
                l1, ssim = masked_l1(a, y, m), masked_ssim(b, y, m)
                assert abs(float(l1.detach()) - float(g[f"{tag}_{mname}_0_loss"])) < 2e-6, (tag, mname)    # lambda = 0: the loss is l1
                assert abs(float(ssim.detach()) - float(g[f"{tag}_{mname}_1_loss"])) < 2e-6, (tag, mname)  # lambda = 1: ssim_loss
                l1.backward()
                ssim.backward()
                for grad, lam in ((a.grad, 0), (b.grad, 1)):
                    ref = torch.from_numpy(g[f"{tag}_{mname}_{lam}_grad"])
                    assert float((grad - ref).abs().max()) <= 1e-6 + 1e-4 * float(ref.abs().max()), (tag, mname, lam)


def test_all_zero_mask_gives_zero_loss_and_zero_gradient():
    g = _golden()
    x = torch.from_numpy(g["a_x"]).requires_grad_(True)
    y = torch.from_numpy(g["a_y"])
    for mask in (torch.zeros(2, 1, 37, 53), torch.zeros(2, 3, 37, 53, dtype=torch.bool)):
        for fn in (lambda: photometric_loss(x, y, 0.2, mask), lambda: masked_l1(x, y, mask)):
            x.grad = None
            loss = fn()
            loss.backward()
            assert float(loss.detach()) == 0.0
            assert bool(torch.isfinite(x.grad).all()) and bool((x.grad == 0).all())


def test_error_contract():
    x, y = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 9)
    m = torch.ones(1, 1, 8, 8)
    with pytest.raises(ValueError, match=r"masked_l1: pred shape torch.Size\(\[1, 3, 8, 8\]\) != gt shape torch.Size\(\[1, 3, 8, 9\]\)\. "
                                         r"Shapes must match\."):
        masked_l1(x, y, m)
    with pytest.raises(ValueError, match=r"masked_ssim: pred shape torch.Size\(\[1, 3, 8, 8\]\) != gt shape torch.Size\(\[1, 3, 8, 9\]\)\. "
                                         r"Shapes must match\."):
        masked_ssim(x, y, m)
    with pytest.raises(ValueError, match="Shapes must match"):
        photometric_loss(x, y)
    for lam in (-0.1, 1.5):
        with pytest.raises(ValueError, match="ssim_lambda"):
            photometric_loss(x, x, lam)
    with pytest.raises(ValueError, match="does not broadcast"):
        photometric_loss(x, x, 0.2, torch.ones(1, 1, 8, 9))


def test_package_exports_the_new_names():
    import gsplat_amd

    for name in ("photometric_loss", "masked_l1", "masked_ssim", "mse_loss"):
        assert getattr(gsplat_amd, name) is getattr(gsplat_amd.losses, name)
    from gsplat_amd import _cabi

    assert {"gsx_photometric_blocks", "gsx_photometric_fwd", "gsx_photometric_bwd"} <= set(_cabi.exported_symbols())


def test_entry_points_refuse_bad_arguments():
    """GSX_REQUIRE of gsx_photometric_fwd / _bwd: reached before any launch, so this runs without a GPU."""
    import ctypes

    from gsplat_amd import _cabi

    s = (ctypes.c_int64 * 4)(1, 1, 1, 1)
    fwd, bwd, p = _cabi._lib.gsx_photometric_fwd, _cabi._lib.gsx_photometric_bwd, 64  # p: a non-null address that is never read
    assert fwd(None, s, p, s, None, None, 0, 1, 1, 4, 4, 0.2, p, None, p, None) == -1      # null pred
    assert fwd(p, s, p, s, None, None, 0, 1, 1, 4, 4, 0.2, p, None, None, None) == -1      # null record
    assert fwd(p, s, p, s, None, None, 0, 1, 1, 4, 4, 1.5, p, None, p, None) == -1         # ssim_lambda outside [0, 1]
    assert b"ssim_lambda" in _cabi._lib.gsx_last_error()
    assert fwd(p, s, p, s, None, None, 0, 256, 256, 4, 4, 0.2, p, None, p, None) == -1     # 65536 planes
    assert b"65535" in _cabi._lib.gsx_last_error()
    assert fwd(p, s, p, s, p, None, 0, 1, 1, 4, 4, 0.2, p, None, p, None) == -1            # a mask without strides
    assert fwd(p, s, p, s, p, s, 7, 1, 1, 4, 4, 0.2, p, None, p, None) == -1               # unknown mask dtype tag
    assert bwd(p, s, p, s, None, None, 0, 1, 1, 4, 4, -0.5, p, p, p, p, s, None) == -1     # ssim_lambda outside [0, 1]
    assert bwd(p, s, p, s, None, None, 0, 1, 1, 4, 4, 0.2, None, p, p, p, s, None) == -1   # null dmaps
    assert bwd(p, s, p, s, None, None, 0, 1, 1, 4, 4, 0.2, p, p, None, p, s, None) == -1   # null incoming gradient
    assert _cabi._lib.gsx_photometric_blocks(2, 3, 37, 53) == 2 * 3 * 3 * 2 == _cabi._lib.gsx_ssim_blocks(2, 3, 37, 53)


# ---- MI355X -------------------------------------------------------------------------------------------------------------

LAYOUTS = ["nchw", "nhwc_view"]


def _as_layout(t, layout):
    if layout == "nchw":
        return t.cuda()
    return t.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)  # [B, H, W, C] storage viewed as [B, C, H, W]


def _fused(*args, **kw):
    """photometric_loss, asserting that the kernels ran (not the torch composition)."""
    before = _FusedPhotometric.calls
    out = photometric_loss(*args, **kw)
    assert _FusedPhotometric.calls == before + 1, "photometric_loss did not take the fused path"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_kernels_match_the_reference_outputs(layout):
    """Every fixture case through gsx_photometric_fwd / _bwd. Tolerances: those tests/test_losses.py applies to gsx_ssim_*
    against the same reference (fp32 fmaf order inside the window); the L1 half adds one mean."""
    g = _golden()
    for tag, mname, lam, mask, key in _cases(g):
        x = _as_layout(torch.from_numpy(g[f"{tag}_x"]), layout).requires_grad_(True)
        y = _as_layout(torch.from_numpy(g[f"{tag}_y"]), layout)
        variants = [mask if mask is None else _as_layout(mask, layout)]
        if mname in ("b1", "zeros", "ones"):  # values 0 / 1: the bool and uint8 forms are the same mask
            variants += [variants[0] != 0, (variants[0] != 0).to(torch.uint8)]
        ref = torch.from_numpy(g[f"{key}_grad"])
        for m in variants:
            x.grad = None
            loss, l1, ssim = _fused(x, y, lam, m, return_parts=True)
            assert not l1.requires_grad and not ssim.requires_grad and l1.is_cuda and ssim.is_cuda
            loss.backward()
            grad = x.grad.cpu()
            assert x.grad.stride() == x.stride()
            d = [abs(float(v.detach()) - float(g[f"{key}_{n}"])) for v, n in ((loss, "loss"), (l1, "l1"), (ssim, "ssim"))]
            d_grad = float((grad - ref).abs().max())
            print(key, layout, None if m is None else m.dtype, "loss", float(loss.detach()), "|d loss, l1, ssim|", d, "max |d grad|", d_grad,
                  "max |ref grad|", float(ref.abs().max()))
            assert max(d) < 5e-6, (key, d)
            assert d_grad <= 2e-7 + 2e-4 * float(ref.abs().max()), (key, d_grad)
            if mask is not None:
                under = grad[(mask == 0).expand_as(grad)]
                assert under.numel() == 0 or bool((under.view(torch.int32) == 0).all()), key  # +0.0, bit for bit
            if mname == "zeros":
                assert float(loss.detach()) == 0.0 and bool(torch.isfinite(grad).all()) and bool((grad == 0).all()), key


def _render_pair(layout, seed=5, frac=0.3):
    gen = torch.Generator().manual_seed(seed)
    img = torch.rand(1, 1080, 1920, 3, generator=gen)
    tgt = (img + 0.05 * torch.randn(1, 1080, 1920, 3, generator=gen)).clamp(0, 1)
    mask = (torch.rand(1, 1, 1080, 1920, generator=gen) >= frac).float().cuda()
    img, tgt = img.permute(0, 3, 1, 2), tgt.permute(0, 3, 1, 2)
    return _as_layout(img, layout), _as_layout(tgt, layout), mask


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_kernels_match_the_torch_composition_at_1080p(layout):
    """A 1080p x 3 render-shaped pair with a 30 %-zero [1, 1, H, W] mask: the kernels against this repository's own torch
    composition on the same device, incoming gradient 3 rather than 1."""
    img, tgt, mask = _render_pair(layout)
    a = img.clone(memory_format=torch.preserve_format).requires_grad_(True)
    b = img.clone(memory_format=torch.preserve_format).requires_grad_(True)
    la, l1a, sa = _fused(a, tgt, 0.2, mask, return_parts=True)
    l1b, sb = masked_l1(b, tgt, mask), masked_ssim(b, tgt, mask)
    lb = torch.lerp(l1b, sb, 0.2)
    (3.0 * la).backward()
    (3.0 * lb).backward()
    d = [abs(float(p.detach()) - float(q.detach())) for p, q in ((la, lb), (l1a, l1b), (sa, sb))]
    d_grad, top = float((a.grad - b.grad).abs().max()), float(b.grad.abs().max())
    print(layout, "loss", float(la.detach()), float(lb.detach()), "|d loss, l1, ssim|", d, "max |d grad|", d_grad, "max |grad|", top)
    assert max(d) < 5e-6, d
    assert d_grad <= 2e-7 + 2e-4 * top
    assert bool((a.grad[(mask == 0).expand_as(a.grad)].view(torch.int32) == 0).all())
    assert a.grad.stride() == a.stride()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_kernels_repeat_bit_for_bit(layout):
    img, tgt, mask = _render_pair(layout, seed=6)
    runs = []
    for _ in range(2):
        x = img.clone(memory_format=torch.preserve_format).requires_grad_(True)
        loss, l1, ssim = _fused(x, tgt, 0.2, mask, return_parts=True)
        loss.backward()
        runs.append((loss.detach().clone(), l1.clone(), ssim.clone(), x.grad))
    for p, q in zip(*runs):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_step_does_not_read_the_device_from_the_host(layout):
    """A masked forward + backward under torch's synchronisation debug mode: any device-to-host read raises."""
    img, tgt, mask = _render_pair(layout, seed=7)
    x = img.clone(memory_format=torch.preserve_format).requires_grad_(True)
    _fused(x, tgt, 0.2, mask).backward()  # first use outside the mode: code objects load here
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, l1, ssim = _fused(x, tgt, 0.2, mask != 0, return_parts=True)
        (2.0 * loss).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(x.grad).all()) and float(loss.detach()) > 0.0
    with pytest.raises(RuntimeError):  # the mode does catch a host read on this build
        torch.cuda.set_sync_debug_mode("error")
        try:
            float(loss.detach())
        finally:
            torch.cuda.set_sync_debug_mode("default")


@pytest.mark.gpu
def test_fallbacks_and_unmasked_fused_path_agree():
    """window_size != 11, a target that requires grad: the torch composition, on the GPU as well; ssim_lambda = 0 and no mask is
    the plain L1 mean; ssim_loss through gsx_ssim_* is untouched by the new template switch."""
    gen = torch.Generator().manual_seed(8)
    x = torch.rand(2, 3, 70, 90, generator=gen).cuda()
    y = (x + 0.1 * torch.randn(2, 3, 70, 90, generator=gen).cuda()).clamp(0, 1)
    before = _FusedPhotometric.calls
    photometric_loss(x, y, 0.2, None, window_size=7)
    photometric_loss(x, y.clone().requires_grad_(True), 0.2)
    assert _FusedPhotometric.calls == before
    loss, l1, ssim = _fused(x, y, 0.2, None, return_parts=True)
    assert abs(float(l1.detach()) - float(l1_loss(x, y).mean())) < 5e-6
    assert abs(float(ssim.detach()) - float(ssim_loss(x, y))) < 5e-6
    assert abs(float(loss.detach()) - float(torch.lerp(l1_loss(x, y).mean(), ssim_loss(x, y), 0.2))) < 5e-6
