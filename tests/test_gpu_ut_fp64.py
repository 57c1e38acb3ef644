"""GPU: the Unscented-Transform projection (project_ut_kernel of csrc/projection_ut.hip, through gsx_project_ut_fwd and the
lidar entry) against the float64 references, per-row bounds and decided masks of tests/_ut_cases.py - every camera model and
route, six cameras that all differ, a batch, the launch edges - and the ray generation of the same file (camera_rays_kernel)
against the same float64 forward models: every generated ray, sent back through the forward model, lands on its pixel centre.
The rolling shutter is not covered here (tests/_ut_cases.py says why); tests/test_gpu_ut.py and tests/test_gpu_lidar.py hold it
to the golden outputs."""
import math
import os

import numpy as np
import pytest
import torch

import _ut_cases as U
from _train_cases import place
from oracle import ut as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
MODEL_ID = {"pinhole": 0, "ortho": 1, "fisheye": 2, "ftheta": 3, "lidar": 4}
WORST = {}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd
    from gsplat_amd import _ops  # noqa: F401

    return gsplat_amd


def _windshield(h, v, hi=(0.0, 1.0, 0.0), vi=(0.0, 0.0, 1.0)):
    p = torch.classes.gsplat.BivariateWindshieldModelParameters()
    p.horizontal_poly, p.vertical_poly = torch.tensor(h, dtype=torch.float32), torch.tensor(v, dtype=torch.float32)
    p.horizontal_poly_inverse, p.vertical_poly_inverse = torch.tensor(hi, dtype=torch.float32), torch.tensor(vi, dtype=torch.float32)
    return p


def _ftheta(ft):
    return None if ft is None else torch.classes.gsplat.FThetaCameraDistortionParameters(**ft)


def _arguments(name):
    """The device tensors and records of a case, as the public call takes them."""
    inp = U.inputs(name)
    c = inp["case"]
    dev = lambda t: None if t is None else place(t, c.misaligned, DEV)  # noqa: E731
    alpha, beta, kappa = U.UT_PARAMS[c.ut]
    ut = torch.classes.gsplat.UnscentedTransformParameters(alpha=alpha, beta=beta, kappa=kappa, in_image_margin_factor=c.margin,
                                                           require_all_sigma_points_valid=c.require_all)
    lidar = None
    if inp["lidar"] is not None:
        from test_gpu_lidar import lidar_from_golden

        lidar = lidar_from_golden(dict(np.load(os.path.join(ROOT, "tests", "golden", "lidar_ref.npz"))), inp["lidar_name"], DEV)
    ext = None if inp["ext"] is None else _windshield(inp["ext"]["horizontal"], inp["ext"]["vertical"])
    tensors = {k: dev(inp[k]) for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}
    coeffs = {k: dev(inp["coeffs"].get(k)) for k in ("radial", "tangential", "thin_prism")}
    if c.misaligned:
        for t in list(tensors.values()) + list(coeffs.values()):
            assert t is None or (t.data_ptr() % 16 == 4 and t.is_contiguous())
    return inp, tensors, coeffs, ut, _ftheta(inp["ftheta"]), lidar, ext


def _check(name, route, got):
    ref = U.reference(name)
    c = U.BY_NAME[name]
    lead = ref.valid.shape
    assert got[0].dtype == torch.int32 and got[0].shape == lead + (2,)
    assert got[1].dtype == torch.float32 and got[1].shape == lead + (2,)
    assert got[2].dtype == torch.float32 and got[2].shape == lead
    assert got[3].dtype == torch.float32 and got[3].shape == lead + (3,)
    assert (got[4] is None) == (not c.comp) and (got[4] is None or (got[4].dtype == torch.float32 and got[4].shape == lead))
    got = tuple(None if t is None else t.cpu() for t in got)
    rep = U.compare(ref, got)
    print(f"{name} [{route}]: " + " ".join(f"{k} {rep.get(k, 0.0):.3f}" for k in U.OUTPUTS)
          + f" | kept {rep['kept']}/{rep['rows']} validity {rep['validity']} radii {rep['radii']} nonzero {rep['nonzero']}")
    for k in U.OUTPUTS:
        key = (route, k)
        WORST[key] = max(WORST.get(key, 0.0), rep.get(k, 0.0))
    assert U.ok(rep), (rep, [U.describe(ref, rep, got, k) for k in U.OUTPUTS if rep.get(k, 0.0) > 1.0])


def _route(inp):
    c = inp["case"]
    if inp["lidar"] is not None:
        return "lidar"
    if c.ext:
        return "ext"
    if not c.gz:
        return "rs(global)"
    return "ftheta" if inp["camera_model"] == "ftheta" else "fwd"


@pytest.mark.parametrize("name", [c.name for c in U.CASES])
def test_ut_projection_within_fp64_bounds(G, name):
    inp, t, co, ut, ft, lidar, ext = _arguments(name)
    c = inp["case"]
    got = G.fully_fused_projection_with_ut(
        t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"], t["Ks"], inp["width"], inp["height"],
        calc_compensations=c.comp, camera_model=inp["camera_model"], ut_params=ut, radial_coeffs=co["radial"],
        tangential_coeffs=co["tangential"], thin_prism_coeffs=co["thin_prism"], ftheta_coeffs=ft, lidar_coeffs=lidar,
        external_distortion_coeffs=ext, global_z_order=c.gz, **inp["kw"])
    _check(name, _route(inp), got)


@pytest.mark.parametrize("name", U.EDGE_CASES)
def test_ut_projection_op_within_fp64_bounds_at_launch_edges(G, name):
    inp, t, co, ut, ft, lidar, ext = _arguments(name)
    c, kw = inp["case"], inp["kw"]
    got = torch.ops.gsplat.projection_ut_3dgs_fused(
        t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"], None, t["Ks"], inp["width"], inp["height"], kw["eps2d"],
        kw["near_plane"], kw["far_plane"], kw["radius_clip"], c.comp, MODEL_ID[inp["camera_model"]], c.gz, ut, 4, co["radial"],
        co["tangential"], co["thin_prism"], ft, lidar, ext)
    _check(name, "op", got)


def test_ut_projection_worst_ratios_per_route(G):
    """Prints the worst |err| / bound per route and output over the cases run so far in this process (GPU numbers)."""
    for (route, k), v in sorted(WORST.items()):
        print(f"worst {route:10s} {k:14s} {v:.3f}")
        assert v <= 1.0


# ---- ray generation ---------------------------------------------------------------------------------------------------------------
RW, RH, RI = 33, 17, 3  # neither dimension a multiple of 16, 561 pixels per image: no multiple of 256
_RFT = dict(pixeldist_to_angle_poly=U.f32list([0.0, 1 / 26.0, 0.0, 2 / 26.0 ** 4, 0.0, 0.0]),
            angle_to_pixeldist_poly=U.f32list([0.0, 26.0, 0.0, -2.0, 0.0, 0.0]), linear_cde=U.f32list([1.002, 0.001, -0.0015]),
            max_angle=U.f32(1.4))
# phi' = 0.01 + 1.05 phi, theta' = -0.02 + 0.97 theta and the inverse pair (exact up to the float32 rounding of the coefficients)
_RWS = dict(horizontal=U.f32list([0.01, 1.05, 0.0]), vertical=U.f32list([-0.02, 0.0, 0.97]),
            horizontal_inverse=U.f32list([-0.01 / 1.05, 1 / 1.05, 0.0]), vertical_inverse=U.f32list([0.02 / 0.97, 0.0, 1 / 0.97]))
RAY_CASES = {
    # name: (camera model, coefficient rows of image 0 (scaled per image), f-theta record, windshield)
    "pinhole": ("pinhole", {}, None, None),
    "opencv": ("pinhole", dict(radial=[0.12, -0.06, 0.01, 0.02, -0.01, 0.004], tangential=[4e-3, -3e-3],
                               thin_prism=[0.002, -0.001, 0.0015, 0.0005]), None, None),
    "ortho": ("ortho", {}, None, None),
    "fisheye": ("fisheye", dict(radial=[-0.04, 0.012, -0.003, 0.0]), None, None),
    "fisheye_tight": ("fisheye", dict(radial=[-0.7, 0.0, 0.0, 0.0]), None, None),  # the angle limit falls inside the image
    "ftheta_forward": ("ftheta", {}, dict(_RFT, reference_poly=1), None),
    "ftheta_inverse": ("ftheta", {}, dict(_RFT, reference_poly=0), None),
    "pinhole-windshield": ("pinhole", {}, None, _RWS),
    "fisheye-windshield": ("fisheye", dict(radial=[-0.04, 0.012, -0.003, 0.0]), None, _RWS),
}


def _ray_inputs(name):
    model, rows, ft, ws = RAY_CASES[name]
    vm, _, scale = U._cameras(1, RI)
    vm, scale = vm[0], scale[0]
    Ks = torch.zeros(RI, 3, 3)
    for i in range(RI):
        Ks[i] = torch.tensor([[24.0 * 1.12 ** i, 0.0, RW / 2 * 0.85 * 1.11 ** i], [0.0, 30.0 / 1.12 ** i, RH / 2 * 1.2 / 1.11 ** i],
                              [0.0, 0.0, 1.0]])
    if model == "ortho":
        Ks[:, 0, 0] *= 0.3
        Ks[:, 1, 1] *= 0.3
    coeffs = {k: (torch.tensor(r)[None] * scale[:, None]).float().contiguous() for k, r in rows.items()}
    return model, vm, Ks, coeffs, ft, ws


@pytest.mark.parametrize("name", list(RAY_CASES))
def test_generated_rays_land_on_their_pixel_centres(G, name):
    """camera_rays_kernel with three images that differ in pose, Ks and coefficients: each ray, taken back to the camera frame in
    float64 and sent through the float64 forward model of oracle/ut.py, lands on (x + 0.5, y + 0.5) within
        |d forward / d ray| (32 EPS + the inverse windshield's own roundings + the mismatch of the float32 inverse pair)
        + 1e-6 sum |d forward / d ray|        (the stopping rule of the Newton inversions: a step below 1e-6 in normalised
                                               coordinates / in the angle, times the local magnification in pixels)
        + c_model EPS (|px - c| + |px|)       (the model's own roundings, counted as in tests/_ut_cases.py)
    (f-theta with the backward polynomial as the calibrated one has no Newton in the ray; the forward model's own Newton stops
    below 1e-6 px.) Origins against the float64 pose within 32 EPS sum |t| (+ |u| + |v| for the orthographic origin). Pixels the
    model cannot invert (beyond the fisheye angle limit, by more than 1e-4 relative) carry the zero ray."""
    from gsplat_amd import _ops

    model, vm, Ks, coeffs, ft, ws = _ray_inputs(name)
    ext = None if ws is None else _windshield(ws["horizontal"], ws["vertical"], ws["horizontal_inverse"], ws["vertical_inverse"])
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    rays = _ops.camera_pixel_rays(dev(vm), None, dev(Ks), RW, RH, MODEL_ID[model], 4, dev(coeffs.get("radial")),
                                  dev(coeffs.get("tangential")), dev(coeffs.get("thin_prism")), _ftheta(ft), ext)
    assert rays.shape == (RI, RH, RW, 6) and rays.dtype == torch.float32
    rays = rays.cpu().double()
    E = U.EPS
    vm64, K64 = vm.double(), Ks.double()
    R, t = vm64[:, :3, :3], vm64[:, :3, 3]
    o_w, d_w = rays[..., :3], rays[..., 3:]
    d_c = torch.einsum("iab,ihwb->ihwa", R, d_w)
    o_c = torch.einsum("iab,ihwb->ihwa", R, o_w) + t[:, None, None, :]
    xs, ys = torch.arange(RW, dtype=torch.float64) + 0.5, torch.arange(RH, dtype=torch.float64) + 0.5
    centre = torch.stack([xs[None, None, :].expand(RI, RH, RW), ys[None, :, None].expand(RI, RH, RW)], -1)
    par = lambda v: v[:, None]  # noqa: E731
    fx, fy, cx, cy = par(K64[:, 0, 0]), par(K64[:, 1, 1]), par(K64[:, 0, 2]), par(K64[:, 1, 2])
    co = {k: v.double() for k, v in coeffs.items()}
    fwd_ws = None if ws is None else dict(horizontal=ws["horizontal"], vertical=ws["vertical"])

    def forward(X):  # camera-frame points / rays [I,H,W,3] -> pixels
        if fwd_ws is not None:
            X = O.windshield_points(X, model, fwd_ws)[0]
        px, _ = O.project_points(X.reshape(RI, RH * RW, 3), model, fx, fy, cx, cy, RW, RH, 0.1, co.get("radial"),
                                 co.get("tangential"), co.get("thin_prism"), ft)
        return px.reshape(RI, RH, RW, 2)

    nonzero = (rays != 0).any(-1)
    decided_valid = torch.ones(RI, RH, RW, dtype=torch.bool)
    decided_invalid = torch.zeros(RI, RH, RW, dtype=torch.bool)
    landing = decided_valid.clone()
    if model == "fisheye":
        k = co["radial"]
        amax = O.fisheye_max_angle(k, K64[:, 0, 0], K64[:, 1, 1], K64[:, 0, 2], K64[:, 1, 2], RW, RH)
        assert len(set(amax.tolist())) == RI
        a2 = amax * amax
        reach = (amax * (1 + a2 * (k[:, 0] + a2 * (k[:, 1] + a2 * (k[:, 2] + a2 * k[:, 3])))))[:, None, None]  # |uv| at the limit
        delta = torch.sqrt(((centre[..., 0] - cx[:, :, None]) / fx[:, :, None]) ** 2 + ((centre[..., 1] - cy[:, :, None]) / fy[:, :, None]) ** 2)
        decided_valid, decided_invalid = delta < reach * (1 - 1e-4), delta > reach * (1 + 1e-4)
        landing = delta < reach * 0.98  # next to the limit the polynomial is flat: Newton's last step says little about the angle
        if name == "fisheye_tight":
            assert int(decided_invalid.sum()) > 50 and int(decided_valid.sum()) > 50
    assert bool(nonzero[decided_valid].all()) and not bool(nonzero[decided_invalid].any())
    check = decided_valid & landing & nonzero

    if model == "ortho":  # parallel rays: the pixel moves the origin
        assert float((d_c - torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).abs().max()) <= 32 * E
        got = torch.stack([o_c[..., 0] * fx[:, :, None] + cx[:, :, None], o_c[..., 1] * fy[:, :, None] + cy[:, :, None]], -1)
        uv = o_c[..., :2].abs().sum(-1)
        tol = (32 * E * (uv + t.abs().sum(-1)[:, None, None]))[..., None] * torch.stack([fx, fy], -1)[:, :, None, :].expand(RI, RH, RW, 2) \
            + 4 * E * (centre + torch.stack([cx, cy], -1)[:, :, None, :].abs())
        assert float(o_c[..., 2].abs().max()) <= float(32 * E * (uv.max() + t.abs().sum(-1).max()))
    else:
        o_ref = -torch.einsum("iba,ib->ia", R, t)
        tol_o = 32 * E * t.abs().sum(-1)
        assert bool(((o_w - o_ref[:, None, None, :]).abs()[check] <= tol_o[:, None, None, None].expand(RI, RH, RW, 3)[check]).all())
        assert float((d_w.norm(dim=-1)[check] - 1.0).abs().max()) <= 32 * E
        got = forward(d_c)
        J = U._fd_abs_jacobian(forward, d_c)                       # [I,H,W,2,3]
        dd = torch.full_like(d_c, 32 * E)
        if ws is not None:
            inv = dict(horizontal=ws["horizontal_inverse"], vertical=ws["vertical_inverse"])
            seen = O.windshield_points(d_c, model, fwd_ws)[0]      # the camera model's ray, as the kernel had it before the inverse
            dd = dd + U._windshield_rounding(seen, model, inv) + (O.windshield_ray(O.windshield_ray(seen, **inv), **fwd_ws) - seen).abs()
        newton = 0.0 if (model in ("pinhole", "ortho") and not coeffs) or (model == "ftheta" and ft["reference_poly"] == 0) else 1e-6
        kind = model if model != "pinhole" else ("opencv" if coeffs else "pinhole")
        pp = torch.stack([cx, cy], -1)[:, :, None, :] + (0.5 if model == "ftheta" else 0.0)
        tol = (J * dd[..., None, :]).sum(-1) + newton * J.sum(-1) + U.C_MODEL[kind] * E * ((centre - pp).abs() + centre.abs())
        if model == "ftheta" and ft["reference_poly"] == 0:
            tol = tol + 2e-6
    err = (got - centre).abs()
    ratio = (err / tol)[check]
    assert int(check.sum()) > RI * RH * RW // 4
    worst = int(torch.argmax(ratio.amax(-1)))
    where = torch.nonzero(check)[worst].tolist()
    print(f"rays {name}: checked {int(check.sum())}/{check.numel()}, zero rays {int((~nonzero).sum())}, worst |err| / bound "
          f"{float(ratio.max()):.3f} at (image, y, x) = {where}: err {err[tuple(where)].tolist()} bound {tol[tuple(where)].tolist()}")
    assert bool(torch.isfinite(ratio).all()) and float(ratio.max()) <= 1.0
