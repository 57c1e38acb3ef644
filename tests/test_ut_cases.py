"""CPU: the float64 references and per-row bounds of tests/_ut_cases.py (the Unscented-Transform projection of
csrc/projection_ut.hip) hold what they promise before a GPU sees them - the float32 restatement of oracle/ut.py lies inside
every bound with a ratio <= 0.5, at most 2 % of a case's rows are undecided, wrong restatements fall outside - and the two new
pieces of the oracle (windshield rays, lidar projection) agree with the golden vectors of the reference's own statements."""
import os

import numpy as np
import pytest
import torch

import _ut_cases as U
from oracle import ut as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in U.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_lies_inside_every_bound(name):
    ref = U.reference(name)
    got = U.restate32(name)
    rep = U.compare(ref, got)
    print(name, {k: round(rep.get(k, 0.0), 3) for k in U.OUTPUTS}, "kept", rep["kept"], "of", rep["rows"])
    assert U.ok(rep, limit=0.5), (rep, [U.describe(ref, rep, got, k) for k in U.OUTPUTS if rep.get(k, 0.0) > 0.5])
    for g, shape in zip(got[:4], ((2,), (2,), (), (3,))):
        assert g.shape == ref.valid.shape + shape


@pytest.mark.parametrize("name", NAMES)
def test_undecided_rows_stay_under_the_cap(name):
    ref = U.reference(name)
    print(name, "undecided", round(ref.undecided_share, 4), "valid", int(ref.valid.sum()), "of", ref.valid.numel())
    assert ref.undecided_share <= U.UNDECIDED_CAP
    if ref.valid.numel() > 1:
        assert int(ref.valid.sum()) > 0.05 * ref.valid.numel() and int((~ref.valid).sum()) > 0  # both kinds of rows exist


def test_cases_cover_what_they_claim():
    """Distinct cameras (poses, Ks by >= 10 %, coefficient rows, fisheye limits), a batch, the row filters, the launch edges."""
    inp = U.inputs("fisheye_tight")
    Ks = inp["Ks"].reshape(-1, 3, 3).double()
    for a in range(6):
        for b in range(a + 1, 6):
            for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):
                r = float(Ks[a, i, j] / Ks[b, i, j])
                assert max(r, 1.0 / r) - 1.0 >= 0.1
            assert not torch.equal(inp["viewmats"].reshape(-1, 4, 4)[a], inp["viewmats"].reshape(-1, 4, 4)[b])
            assert not torch.equal(inp["coeffs"]["radial"].reshape(-1, 4)[a], inp["coeffs"]["radial"].reshape(-1, 4)[b])
    for name in ("fisheye_plain", "fisheye_k", "fisheye_k4", "fisheye_tight"):
        amax = U.reference(name).info["aux"]["amax"][:, :, 0, 0].reshape(-1)
        assert len(set(amax.tolist())) == 6 and float((amax[:, None] - amax[None, :]).abs()[~torch.eye(6, dtype=torch.bool)].min()) > 1e-3
    assert not torch.equal(inp["means"][0], inp["means"][1])
    ref, inp = U.reference("pinhole"), U.inputs("pinhole")
    I = ref.info
    assert bool((I["z"] < 0).any()) and float(inp["quats"][0, 5].abs().sum()) == 0.0 and float(inp["scales"][0, 9, 1]) == 0.0
    assert float(inp["scales"][0, 10, 2]) == U.F32_EPS and not bool(ref.valid[:, :, 10].any()) and not bool(ref.valid[:, :, 9].any())
    front = I["cam"][..., 2] > 0
    assert bool((front.any(-1) & ~front.all(-1)).any())  # some sigma points behind, some in front
    op = I["op"][:, 0]
    assert bool((op[:, 12] < O.ALPHA_THRESHOLD).all()) and bool((op[:, 13] > O.ALPHA_THRESHOLD).all())
    assert bool((op[:, 12:14] / O.ALPHA_THRESHOLD - 1.0).abs().max() < 6e-3)
    assert not bool(ref.valid[:, 0, 12].any()) and not bool(ref.decided_invalid[:, 0, 13].any())
    sharp = U.reference("pinhole-ut1-all0")  # weights of order 1: the bound of opacity * compensation is far below 5e-3
    assert bool(sharp.decided_invalid[:, 0, 12].all()) and not bool(sharp.decided_invalid[:, 0, 13].any())
    icd = U.reference("opencv_strong").info["aux"]["icd"]
    assert bool((icd < O.ICD_MIN).any()) and bool((icd > O.ICD_MIN).any())
    rows = sorted({c.B * c.C * c.N for c in U.CASES if "-edge-" in c.name})
    assert rows == [1, 255, 256, 257, 513, 771]
    assert {c.ut for c in U.CASES} == {0, 1, 2} and {c.require_all for c in U.CASES} == {False, True}
    assert {c.margin for c in U.CASES} == {0.05, 0.1}
    assert any(c.ext for c in U.CASES) and any(not c.gz for c in U.CASES) and any(not c.opac for c in U.CASES)


def _cam0(t):
    return t[:1, :1].expand_as(t).contiguous()


def _batch0(t):
    return None if t is None else t[:1].expand_as(t).contiguous()


def _wrong(name, what):
    """A wrong restatement of case `name` in float32."""
    inp = U.inputs(name)
    w_m0, w_c0, w_i, spread = inp["weights"]
    alpha, beta, kappa = U.UT_PARAMS[inp["case"].ut]
    if what == "camera 0's coefficient row for every camera":
        return U.restate32(name, coeffs={k: _cam0(v) for k, v in inp["coeffs"].items()})
    if what == "batch 0's Gaussians for every batch entry":
        return U.restate32(name, **{k: _batch0(inp[k]) for k in ("means", "quats", "scales", "opacities")})
    if what == "camera 0's fisheye angle limit for every camera":
        amax = U.reference(name).info["aux"]["amax"][:, :, 0, 0]
        return U.restate32(name, fisheye_limit=_cam0(amax))
    if what == "w_c0 = w_m0":
        return U.restate32(name, weights=(w_m0, w_m0, w_i, spread))
    if what == "kappa left out of the spread":
        assert kappa != 0.0
        return U.restate32(name, weights=(w_m0, w_c0, w_i, U.f32(abs(alpha) * 3.0 ** 0.5)))
    if what == "f-theta principal point without the half-pixel shift":
        Ks = inp["Ks"].clone()
        Ks[..., :2, 2] -= 0.5
        return U.restate32(name, Ks=Ks)
    if what == "p1 and p2 swapped":
        assert float(inp["coeffs"]["tangential"].abs().max()) < 2e-3
        return U.restate32(name, coeffs=dict(inp["coeffs"], tangential=inp["coeffs"]["tangential"].flip(-1).contiguous()))
    mutate = {"blur added before det0": "blur_before_det0", "radii from the largest eigenvalue alone": "radii_from_eigenvalue",
              "sums over all seven points under require_all": "sum_all_points",
              "windshield's vertical polynomial fed (theta, phi)": "windshield_swapped_angles",
              "lidar relative azimuth without the wrap": "lidar_no_wrap"}[what]
    return U.restate32(name, mutate=(mutate,))


WRONG = [  # (what, the cases it is tried on: at least one must catch it)
    ("camera 0's coefficient row for every camera", ("opencv_full", "fisheye_k")),
    ("batch 0's Gaussians for every batch entry", ("pinhole",)),
    ("camera 0's fisheye angle limit for every camera", ("fisheye_tight",)),
    ("w_c0 = w_m0", ("pinhole", "pinhole-ut1-all0")),
    ("kappa left out of the spread", ("pinhole-ut1-all0",)),
    ("blur added before det0", ("pinhole", "pinhole-comp_clip")),
    ("radii from the largest eigenvalue alone", ("pinhole",)),
    ("f-theta principal point without the half-pixel shift", ("ftheta_forward", "ftheta_inverse")),
    ("p1 and p2 swapped", ("opencv_full",)),
    ("windshield's vertical polynomial fed (theta, phi)", ("pinhole-windshield", "fisheye_k-windshield")),
    ("lidar relative azimuth without the wrap", ("lidar_cw_120", "lidar_ccw_90")),
]


@pytest.mark.parametrize("what,names", WRONG, ids=[w for w, _ in WRONG])
def test_wrong_restatement_falls_outside_a_bound(what, names):
    caught = []
    for name in names:
        ref = U.reference(name)
        got = _wrong(name, what)
        rep = U.compare(ref, got)
        old = U.old_tolerances_pass(ref, got)
        print(f"{what} on {name}: caught {not U.ok(rep)} "
              f"({ {k: rep.get(k) for k in ('validity', 'radii', 'nonzero') + U.OUTPUTS} }); the old tolerances "
              f"(2e-2 px, 3e-2, radii +- 1, 2 flips) would have {'LET IT THROUGH' if old else 'caught it'}")
        caught.append(not U.ok(rep))
    assert any(caught), what


def test_sums_past_the_first_invalid_point_cannot_be_seen():
    """Under require_all_sigma_points_valid the sums stop at the first invalid point - and the row is invalid then, so it is
    written as zeros either way: no output tells a kernel that stops from one that sums all seven points. Stated here so that
    nobody looks for a test that could."""
    for name in ("pinhole-ut0-all1", "opencv_full", "fisheye_k-ut1-all1"):
        assert U.BY_NAME[name].require_all
        a, b = U.restate32(name), _wrong(name, "sums over all seven points under require_all")
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("order", range(6))
def test_oracle_windshield_rays_match_reference(order):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "external_distortion_ref.npz"))
    rays = torch.from_numpy(gold[f"o{order}.rays"]).double()
    out = O.windshield_ray(rays, gold[f"o{order}.h"].tolist(), gold[f"o{order}.v"].tolist())
    torch.testing.assert_close(out, torch.from_numpy(gold[f"o{order}.ref.distorted"]), rtol=0, atol=1e-12)
    x, y = torch.from_numpy(gold[f"o{order}.x"]).double(), torch.from_numpy(gold[f"o{order}.y"]).double()
    torch.testing.assert_close(O.bivariate_poly(gold[f"o{order}.h"].tolist(), x, y), torch.from_numpy(gold[f"o{order}.ref.poly"]),
                               rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["cw_120", "ccw_periodic", "ccw_90"])
def test_oracle_lidar_projection_matches_reference(name):
    """oracle/ut.py's lidar model (global shutter) in float64 against the reference's float32 torch statement, within what that
    statement's own precision allows: angular pixels of magnitude up to 3200 (half an ulp = 1.2e-4) through UT weights of -99."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "lidar_ref.npz"))
    t = lambda k: torch.from_numpy(gold[f"{name}.cam.{k}"]).double()  # noqa: E731
    fv0, fvs, fh0, fhs, _, ccw = gold[f"{name}.scalars"][:6]
    got = O.fully_fused_projection_with_ut(
        t("pts"), t("quats"), t("scales"), t("opac"), t("viewmats"), t("Ks"), int(gold[f"{name}.column_azimuths_rad"].shape[0]),
        int(gold[f"{name}.row_elevations_rad"].shape[0]), camera_model="lidar", lidar=dict(h0=fh0, hs=fhs, v0=fv0, vs=fvs, ccw=int(ccw)))
    ref = {k: torch.from_numpy(gold[f"{name}.proj_global.{k}"]) for k in ("radii", "means2d", "depths", "conics")}
    vr, vg = (ref["radii"] > 0).all(-1), (got[0] > 0).all(-1)
    assert int((vr != vg).sum()) == 0 and int(vr.sum()) > 30
    assert int((got[0] - ref["radii"]).abs()[vr].max()) <= 2 and float(((got[0] - ref["radii"]).abs()[vr] > 1).float().mean()) < 0.01
    assert float((got[1] - ref["means2d"]).abs()[vr].max()) < 0.1
    torch.testing.assert_close(got[2][vr], ref["depths"][vr].double(), rtol=1e-6, atol=1e-6)
    rel = (got[3] - ref["conics"]).abs()[vr] / ref["conics"].abs()[vr].amax(-1, keepdim=True)
    assert float(rel.max()) < 1e-3
