"""CPU: colour correction without a GPU - the pinned reference (tests/golden/color_correct_ref.npz, written by
tools/pin_color_correct_against_reference.py from the reference's gsplat/color_correct.py) holds every case of
tests/_color_correct_cases.py; the cases are what they claim (saturation, planted thresholds, poisoned ref, guard band, pivots);
the `*_torch` compositions reproduce the reference's float64 output to 1e-12 and lie within twice its own float32 error in
float32, while a fit that ignores the mask falls far outside; the error contract, the dispatch on the CPU, the exports, the
launch regimes of gsx_cc_blocks and the argument checks of the gsx_cc_* entry points, which run before any launch.
tests/test_gpu_color_correct.py holds the kernels to the same reference."""
import numpy as np
import pytest
import torch

import _color_correct_cases as cc
from gsplat_amd import color_correct as C


@pytest.fixture(scope="module")
def pinned():
    return np.load(cc.FIXTURE)


def test_launch_regimes_are_pinned():
    from gsplat_amd import _cabi

    blocks = _cabi._lib.gsx_cc_blocks
    span, cap, cap_n = cc.launch_edges()
    assert (span, cap, cap_n) == (1024, 512, 524288)
    assert blocks(span) == 1 and blocks(span + 1) == 2 and blocks(cap_n - span) == cap - 1
    assert blocks(cap_n) == cap == blocks(cap_n + 1) == blocks(1 << 50)
    assert blocks(0) == 1 and blocks(-5) == 1 and blocks(1) == 1
    counts = [blocks(n) for n in (0, 1, span, span + 1, 3 * span, cap_n - 1, cap_n, cap_n + 1, 1 << 31, 1 << 62)]
    assert counts == sorted(counts) and max(counts) == cap  # monotone and capped
    pixels = {int(np.prod(i.shape[:-1])) for i in cc.inputs_table().values()}
    assert pixels >= {37 * 53, 2 * 19 * 23, span - 1, span, span + 1, cap_n + 1}


def test_the_fixture_holds_every_case(pinned):
    table = cc.inputs_table()
    for key, inp in table.items():
        if inp.kind == "tiled":
            img, ref = cc.build(inp, (pinned["in/nat-37x53/img"], pinned["in/nat-37x53/ref"]))
            assert img.shape == inp.shape and pinned[f"in/{key}/sum"].tolist() == [img.astype(np.float64).sum(), ref.astype(np.float64).sum()]
            assert pinned[f"a/{key}/out64"].shape == (-(-img.size // cc.STRIDE),)
        else:  # the seeded builders still give the arrays the reference was run on
            img, ref = cc.build(inp)
            assert np.array_equal(pinned[f"in/{key}/img"], img) and np.array_equal(pinned[f"in/{key}/ref"], ref), key
            assert pinned[f"a/{key}/out64"].shape == inp.shape and pinned[f"a/{key}/out64"].dtype == np.float64
        assert 0 < float(pinned[f"a/{key}/e32"]) < 1e-6
    for case in cc.cases():
        out64, e32 = pinned[f"q/{case.name}/out64"], float(pinned[f"q/{case.name}/e32"])
        assert out64.dtype == np.float64 and np.isfinite(out64).all() and out64.min() >= 0.0 and out64.max() <= 1.0
        assert (0 < e32 < 1e-4) if case.num_iters else e32 == 0.0, (case.name, e32)
    assert {c.num_iters for c in cc.cases()} == {0, 1, 5} and {c.eps for c in cc.cases()} == {cc.EPS, cc.EPS2}
    assert {c.input for c in cc.cases()} == set(table)


def test_the_cases_are_what_they_claim(pinned):
    lo, hi = np.float32(cc.EPS), np.float32(1.0 - cc.EPS)
    assert (float(lo), float(hi)) == cc.thresholds(cc.EPS) and float(lo) != cc.EPS  # the float32 thresholds are not the doubles
    for key, inp in cc.inputs_table().items():
        if inp.kind == "tiled":
            continue
        img, ref = pinned[f"in/{key}/img"], pinned[f"in/{key}/ref"]
        for a in (img, ref):  # roughly a tenth saturated at 0 or 1, both ends present
            assert 0.05 < float(((a == 0) | (a == 1)).mean()) < 0.25 and (a == 0).any() and (a == 1).any(), key
            assert a.min() >= 0 and a.max() <= 1
        planted = [int((a == t).sum()) for a in (img, ref) for t in (lo, hi)]
        assert planted == ([cc.PLANTED] * 4 if inp.kind == "thresholds" else [0] * 4), (key, planted)
        for it, eps in {(c.num_iters, c.eps) for c in cc.cases() if c.input == key and c.num_iters}:
            gap, pivot = cc.guard_report(img, ref, it, eps)
            assert gap > cc.GUARD and pivot > cc.MIN_PIVOT, (key, it, eps, gap, pivot)
    ref = pinned["in/poison-23x19/ref"]
    sat = (ref == 0) | (ref == 1)
    clean = cc._natural((23, 19, 3), np.random.default_rng([cc.SEEDS["poison-23x19"], sum(map(ord, "poison-23x19"))]))[1]
    assert np.array_equal(ref[~sat], clean[~sat]) and 0.3 < float((ref[sat] != clean[sat]).mean()) < 0.7  # a coin where saturated
    for name, (img, ref) in cc.singular_inputs().items():
        assert cc.trace64(img.numpy(), ref.numpy(), 1, cc.EPS)[1] <= 1e-10, name


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_torch_compositions_match_the_pinned_reference(pinned, dtype):
    """float64: the reference's float64 output to 1e-12. float32: within twice the reference's own float32 error."""
    affine_done = set()
    for case in cc.cases():
        img, ref = (t.to(dtype) for t in cc.load_inputs(pinned, case))
        runs = [(f"q/{case.name}", C.color_correct_quadratic_torch(img, ref, case.num_iters, case.eps))]
        if case.input not in affine_done:
            affine_done.add(case.input)
            runs.append((f"a/{case.input}", C.color_correct_affine_torch(img, ref)))
        for name, out in runs:
            assert out.dtype == dtype and out.shape == img.shape
            got, want, e32 = cc.expected(pinned, name, out)
            err = float((got - want).abs().max())
            print(f"{name:28s} {dtype}: error {err:.3e} (e32 {e32:.3e})")
            assert err <= (1e-12 if dtype == torch.float64 else 2 * e32), (name, err, e32)


def test_a_fit_that_ignores_the_mask_falls_outside(pinned):
    """eps = -1 makes every row count. On the poisoned input that is off by orders of magnitude more than any bound here."""
    img, ref = cc.load_inputs(pinned, "poison-23x19")
    out = C.color_correct_quadratic_torch(img.double(), ref.double(), 5, -1.0)
    got, want, e32 = cc.expected(pinned, "q/poison-23x19-i5", out)
    assert float((got - want).abs().max()) > 1e4 * (2 * e32 + 5 * 2.0 ** -24)


def test_shape_rule_dispatch_and_num_iters_zero(pinned):
    img, ref = cc.load_inputs(pinned, "nat-2x19x23")
    before = C._FusedColorCorrectQuadratic.calls, C._FusedColorCorrectAffine.calls
    flat = C.color_correct_quadratic(img.reshape(-1, 3), ref.reshape(-1, 3))
    # the leading dimensions are one set of pixels (float32 lstsq on the CPU does not repeat bit for bit: a few ulp)
    assert float((C.color_correct_quadratic(img, ref) - flat.reshape(img.shape)).abs().max()) < 4e-6
    assert torch.equal(C.color_correct_affine(img, ref), C.color_correct_affine(img.reshape(-1, 3), ref.reshape(-1, 3)).reshape(img.shape))
    assert torch.equal(C.color_correct_quadratic(img, ref, num_iters=0), img)
    assert float((flat - C.color_correct_quadratic_torch(img.reshape(-1, 3), ref.reshape(-1, 3))).abs().max()) < 4e-6
    four = torch.rand(50, 4, dtype=torch.float64)
    assert C.color_correct_quadratic(four, four.flip(0), num_iters=1).shape == (50, 4)  # 4 channels: 15 features
    assert (C._FusedColorCorrectQuadratic.calls, C._FusedColorCorrectAffine.calls) == before  # CPU tensors never take the kernels
    x = img.clone().requires_grad_(True)
    C.color_correct_quadratic(x, ref, num_iters=1).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().sum()) > 0
    y = img.clone().requires_grad_(True)
    C.color_correct_affine(y, ref).sum().backward()
    assert bool(torch.isfinite(y.grad).all())


def test_error_contract():
    a, b = torch.rand(5, 7, 3), torch.rand(5, 7, 4)
    for fn in (C.color_correct_quadratic, C.color_correct_affine, C.color_correct_quadratic_torch, C.color_correct_affine_torch):
        with pytest.raises(ValueError, match=r"^img's 3 and ref's 4 channels must match$"):
            fn(a, b)
        with pytest.raises(ValueError, match=r"^img's 4 and ref's 3 channels must match$"):
            fn(b, a)


def test_package_exports_the_new_names():
    import gsplat_amd
    from gsplat_amd import _cabi

    assert gsplat_amd.color_correct is C
    for name in ("color_correct_affine", "color_correct_quadratic"):
        assert getattr(gsplat_amd, name) is getattr(C, name) and name in dir(gsplat_amd)
    assert {"gsx_cc_blocks", "gsx_cc_quadratic", "gsx_cc_affine"} <= set(_cabi.exported_symbols())
    assert gsplat_amd.build_config()["losses"] is False  # the reference's gaussian_losses op is not what this adds


def test_entry_points_refuse_bad_arguments():
    """GSX_REQUIRE of the gsx_cc_* entry points: reached before any HIP call, so this runs without a GPU."""
    from gsplat_amd import _cabi

    lib, err = _cabi._lib, _cabi._lib.gsx_last_error
    q, a, p = lib.gsx_cc_quadratic, lib.gsx_cc_affine, 64  # p: a non-null address that is never read
    assert q(None, p, 10, 5, cc.EPS, p, p, p, p, None) == -1 and b"null" in err()      # img
    assert q(p, None, 10, 5, cc.EPS, p, p, p, p, None) == -1                            # ref
    assert q(p, p, 10, 5, cc.EPS, None, p, p, p, None) == -1                            # scratch
    assert q(p, p, 10, 5, cc.EPS, p, None, p, p, None) == -1                            # warps
    assert q(p, p, 10, 5, cc.EPS, p, p, None, p, None) == -1                            # status
    assert q(p, p, 10, 5, cc.EPS, p, p, p, None, None) == -1                            # out
    assert q(p, p, 0, 5, cc.EPS, p, p, p, p, None) == -1 and b"empty" in err()
    assert q(p, p, -3, 5, cc.EPS, p, p, p, p, None) == -1 and b"empty" in err()
    assert q(p, p, (1 << 31) // 3 + 1, 5, cc.EPS, p, p, p, p, None) == -1 and b"2^31" in err()
    assert q(p, p, 1 << 40, 5, cc.EPS, p, p, p, p, None) == -1 and b"2^31" in err()
    assert q(p, p, 10, 0, cc.EPS, p, p, p, p, None) == -1 and b"num_iters" in err()    # the caller's case: img itself
    assert q(p, p, 10, 65, cc.EPS, p, p, p, p, None) == -1 and b"num_iters" in err()
    assert q(p, p, 10, 5, float("nan"), p, p, p, p, None) == -1 and b"NaN" in err()
    assert a(None, p, 10, p, p, p, None) == -1 and a(p, None, 10, p, p, p, None) == -1
    assert a(p, p, 10, None, p, p, None) == -1 and a(p, p, 10, p, None, p, None) == -1 and a(p, p, 10, p, p, None, None) == -1
    assert a(p, p, 0, p, p, p, None) == -1 and b"empty" in err()
    assert a(p, p, 1 << 30, p, p, p, None) == -1 and b"2^31" in err()
