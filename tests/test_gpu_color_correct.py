"""GPU: the colour-correction kernels of csrc/color_correct.hip through color_correct_quadratic and color_correct_affine, on
every non-singular case of tests/_color_correct_cases.py against the reference's float64 output pinned in
tests/golden/color_correct_ref.npz:

    quadratic   max |out - out64| <= 2 e32 + num_iters 2^-24
    affine      max |out - out64| <= 2 e32 + 2^-24

e32 is the reference's own float32 error on the case (its float32 output against out64); 2^-24 per iteration is the one rounding
to float32 per iteration of a value <= 1 that the float64 evaluation does not make. Also: the kernels ran (`calls`), the output
repeats bit for bit, a [..., :3] view of a [1, H, W, 4] tensor gives the bits of its contiguous copy, the three singular inputs
are refused, float64 / four channels / an input that requires grad take the torch composition and agree with it, and the
correction of a twisted rasterization() render brings its PSNR back. tests/test_color_correct.py checks the cases, the
reference and the argument checks without a GPU.

Largest error observed on an MI355X: quadratic 0.148 of the bound (the thresholds input: 1.2e-7 of 8.1e-7; the other cases
0.05-0.11, 9e-8 to 1.2e-7 absolute), affine 0.076 (3.0e-8 in every case: the float64 value rounded once). PSNR of the twisted
render 22.1 dB, 36.4 dB after the affine and 51.5 dB after the quadratic correction."""
import numpy as np
import pytest
import torch

import _color_correct_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from gsplat_amd import color_correct

    return color_correct


@pytest.fixture(scope="module")
def pinned():
    return np.load(cc.FIXTURE)


def _on_device(pinned, case_or_key):
    return tuple(t.to(DEV) for t in cc.load_inputs(pinned, case_or_key))


def test_quadratic_every_case_against_float64(C, pinned):
    before, worst = C._FusedColorCorrectQuadratic.calls, 0.0
    for case in cc.cases():
        img, ref = _on_device(pinned, case)
        with torch.no_grad():
            out = C.color_correct_quadratic(img, ref, num_iters=case.num_iters, eps=case.eps)
        assert out.shape == img.shape and out.dtype == torch.float32 and (out.data_ptr() != img.data_ptr() or case.num_iters == 0)
        got, want, e32 = cc.expected(pinned, f"q/{case.name}", out)
        err, bound = float((got - want).abs().max()), 2 * e32 + case.num_iters * 2.0 ** -24
        print(f"q/{case.name:24s} error {err:.3e}  bound {bound:.3e}  ratio {err / bound if bound else 0.0:.3f}")
        worst = max(worst, err / bound if bound else 0.0)
        assert err <= bound, (case.name, err, bound)
    print(f"largest quadratic error / bound: {worst:.3f}")
    assert C._FusedColorCorrectQuadratic.calls - before == sum(1 for c in cc.cases() if c.num_iters)  # 0 iterations: img itself


def test_affine_every_case_against_float64(C, pinned):
    before, worst = C._FusedColorCorrectAffine.calls, 0.0
    for key in cc.inputs_table():
        img, ref = _on_device(pinned, key)
        out = C.color_correct_affine(img, ref)
        assert out.shape == img.shape and out.dtype == torch.float32
        got, want, e32 = cc.expected(pinned, f"a/{key}", out)
        err, bound = float((got - want).abs().max()), 2 * e32 + 2.0 ** -24
        print(f"a/{key:24s} error {err:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}")
        worst = max(worst, err / bound)
        assert err <= bound, (key, err, bound)
    print(f"largest affine error / bound: {worst:.3f}")
    assert C._FusedColorCorrectAffine.calls - before == len(cc.inputs_table())


@pytest.mark.parametrize("key", ["nat-37x53", "nat-span+1", "tiled-cap+1"])
def test_outputs_repeat_bit_for_bit(C, pinned, key):
    img, ref = _on_device(pinned, key)
    assert torch.equal(C.color_correct_quadratic(img, ref), C.color_correct_quadratic(img, ref))
    assert torch.equal(C.color_correct_affine(img, ref), C.color_correct_affine(img, ref))


def test_a_channel_view_gives_the_bits_of_its_contiguous_copy(C, pinned):
    img, ref = _on_device(pinned, "nat-37x53")
    wide_img = torch.full((1, 37, 53, 4), float("nan"), device=DEV)
    wide_ref = torch.full((1, 37, 53, 4), float("nan"), device=DEV)
    wide_img[0, ..., :3], wide_ref[0, ..., :3] = img, ref
    view_img, view_ref = wide_img[..., :3], wide_ref[..., :3]
    assert not view_img.is_contiguous()
    for fn in (C.color_correct_quadratic, C.color_correct_affine):
        out = fn(view_img, view_ref)
        assert out.shape == (1, 37, 53, 3) and out.is_contiguous() and torch.equal(out[0], fn(img, ref))
    assert bool(torch.isnan(wide_img[..., 3]).all())  # the inputs are left alone


def test_singular_systems_are_refused(C):
    before = C._FusedColorCorrectQuadratic.calls
    for name, (img, ref) in cc.singular_inputs().items():
        with pytest.raises(ValueError, match=r"^color_correct_quadratic: rank-deficient system"):
            C.color_correct_quadratic(img.to(DEV), ref.to(DEV))
        assert bool(torch.isfinite(C.color_correct_affine(img.to(DEV), ref.to(DEV))).all()), name  # the affine form has its clamps
    assert C._FusedColorCorrectQuadratic.calls - before == 3  # refused by the kernels' status word, not beforehand


def test_other_inputs_take_the_torch_composition(C, pinned):
    img, ref = _on_device(pinned, "nat-2x19x23")
    before = C._FusedColorCorrectQuadratic.calls, C._FusedColorCorrectAffine.calls
    # float64
    out = C.color_correct_quadratic(img.double(), ref.double())
    assert out.dtype == torch.float64 and float((out - C.color_correct_quadratic_torch(img.double(), ref.double())).abs().max()) < 1e-12
    got, want, _ = cc.expected(pinned, "q/nat-2x19x23-i5", out)
    assert float((got - want).abs().max()) < 1e-11
    out = C.color_correct_affine(img.double(), ref.double())
    assert float((out.cpu() - torch.from_numpy(pinned["a/nat-2x19x23/out64"])).abs().max()) < 1e-12
    # four channels
    img4 = torch.cat([img, 0.5 + 0.4 * torch.sin(3.0 * img[..., :1] + img[..., 1:2])], -1)
    ref4 = torch.cat([ref, ref[..., 2:] ** 2], -1)
    assert float((C.color_correct_quadratic(img4.double(), ref4.double(), 2)
                  - C.color_correct_quadratic_torch(img4.double(), ref4.double(), 2)).abs().max()) < 1e-12
    assert torch.equal(C.color_correct_affine(img4, ref4), C.color_correct_affine_torch(img4, ref4))
    # an input that requires grad, grad mode on: differentiable, and the value of the composition
    x = img.double().requires_grad_(True)
    out = C.color_correct_quadratic(x, ref.double(), 2)
    out.sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float((out.detach() - C.color_correct_quadratic_torch(x.detach(), ref.double(), 2)).abs().max()) < 1e-12
    y = img.clone().requires_grad_(True)
    out = C.color_correct_affine(y, ref)
    assert out.requires_grad and torch.equal(out, C.color_correct_affine_torch(y, ref))
    assert (C._FusedColorCorrectQuadratic.calls, C._FusedColorCorrectAffine.calls) == before
    with torch.no_grad():  # the trainer's eval loop: the same tensor takes the kernels
        assert not C.color_correct_affine(y, ref).requires_grad
        C.color_correct_quadratic(y, ref)
    assert (C._FusedColorCorrectQuadratic.calls, C._FusedColorCorrectAffine.calls) == (before[0] + 1, before[1] + 1)
    assert torch.equal(C.color_correct_quadratic(img, ref, num_iters=0), img)


def test_correcting_a_twisted_render_brings_its_psnr_back(C):
    import gsplat_amd
    from _util import make_scene

    sc, W, H = make_scene(N=1500, C=1, width=64, height=64, seed=3, device=DEV)
    with torch.no_grad():
        render, _alphas, _meta = gsplat_amd.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["colors"],
                                                          sc["viewmats"], sc["Ks"], W, H)
        gt = render.clamp(0.0, 1.0)
        twist = torch.tensor([[0.85, 0.10, -0.05], [0.05, 0.90, 0.12], [-0.08, 0.04, 1.10]], device=DEV)
        twisted = (gt @ twist + 0.03 + 0.08 * gt * gt).clamp(0.0, 1.0)
        psnr = lambda a: float(-10.0 * torch.log10(((a - gt) ** 2).mean()))
        base = psnr(twisted)
        quadratic, affine = psnr(C.color_correct_quadratic(twisted, gt)), psnr(C.color_correct_affine(twisted, gt))
    print(f"PSNR twisted {base:.2f} dB, affine {affine:.2f} dB, quadratic {quadratic:.2f} dB")
    assert gt.shape == (1, 64, 64, 3) and float(gt.std()) > 0.05
    assert affine > base and quadratic > base
