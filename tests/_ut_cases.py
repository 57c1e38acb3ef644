"""Cases, float64 references, per-row error bounds and decided masks for the Unscented-Transform projection of
csrc/projection_ut.hip (project_ut_kernel behind gsx_project_ut_fwd - plain, f-theta, the Euclidean depth with a global shutter, the windshield - and
gsx_project_ut_lidar_fwd). Shared by tests/test_ut_cases.py (CPU: the float32 restatement of oracle/ut.py lies inside every bound, the share of
undecided rows is capped, wrong restatements fall outside) and tests/test_gpu_ut_fp64.py (GPU: the kernel against the same
references and bounds). Everything here is seeded torch / numpy on the CPU; nothing imports the GPU package.

The ROLLING shutter is not covered: its read-out time is floor(pixel row), so a sigma point within rounding of a row boundary
jumps by one row's motion and no per-row bound exists there. The budgeted golden tests (tests/test_gpu_ut.py,
tests/test_gpu_lidar.py) remain its check.

Conventions. EPS = 2^-24 (half a float32 ulp, relative). Inputs are float32 values promoted to float64; scalar parameters
(eps2d, near / far, radius_clip, the UT weights and spread, the f-theta and windshield records, the lidar's fields of view) are
rounded to float32 first, and so are the literals the kernel carries (oracle/ut.py). The reference is oracle/ut.py in float64
with detail=True. A transcendental (atan2f, asinf, sinf, logf, rsqrtf) is allowed T = 4 ulp = 8 EPS relative: the ROCm math
documentation is not on the build machine, so this is the stated allowance, not a measured one. Inside the camera models
division and sqrtf are allowed D = 1 ulp = 2 EPS (after the UT sums they keep T): hipcc rounds both correctly by default
(-fhip-fp32-correctly-rounded-divide-sqrt) and this unit is built with the default flags; with 4 ulp on every division of a
sigma point the bound of a radius would leave more rows undecided than the cap allows. Every bound counts the roundings of the
kernel's own expression and holds with or without fma contraction (a contraction removes a rounding, never adds one).

  camera-frame point P_i = Rc (m +- o_k) + t, o_k = spread s_k Rq[:, k]:
      dP = sum_j |Rc_kj| (EPS |w_j| + 12 EPS spread s_k) + 4 EPS (sum_j |Rc_kj w_j| + |t_k|)
      (12: rsqrtf-normalised quaternion, two products and a sum per matrix entry, two more products; absolute in the offset's length.
      4: three products and three sums, in any order a term passes through at most four roundings)
  windshield Q = W(P): dQ = |dW/dP| dP (central differences of the float64 model) + its own roundings: the two asin (argument
      3 EPS through 1 / cos, T on the result), the two polynomials (14 EPS of their absolute-value sums) pushed through
      d(sin H, sin V) / d(phi, theta), T/2 on each sine, z = sqrt(1 - x^2 - y^2) through 1 / z.
  sigma-point pixel: delta_i = |d model / dQ| dQ (central differences of project_points in float64)
      + EPS (c_model |px - c| + |px|), c = principal point (the last addition rounds the pixel itself); c_model = D + 2 (perfect
      pinhole: a division and two products), 1 (orthographic), D + 14 (OpenCV pinhole: + the two cubic polynomials, their quotient
      and the tangential / thin-prism sums), 28 (fisheye: hypot 6, atan2 T + 3, degree-9 polynomial 4, quotient D + 6, two products),
      40 (f-theta: + the second polynomial or three Newton steps, the (c, d, e) map); lidar: 1024 EPS (T |az| + 4) and
      1024 EPS (T |el| + 4 |tan el|).
  mean2d: tol = sum |w_m,i| delta_i + 8 EPS sum |w_m,i p_i|
  covariance (before the blur), e = tol of mean2d: because sum w_m,i (p_i - mean2d) = 0 the kernel's error in mean2d enters only as
      2 e |w_c0 - w_m0| |p_0 - mean2d| + e^2 |sum w_c|; the rest is sum |w_c,i| (2 |d_i| delta_i + delta_i^2 + 2 delta_i e)
      + 12 EPS sum |w_c,i d_i d_i'|. The blur adds EPS |c + eps2d|.
  det0, det, idet = a b - c^2: tol = b ta + a tb + 2 |c| tc + 3 EPS (a b + c^2)   (the cancellation term; it dominates for
      elongated footprints)
  compensation = sqrt(max(det0 / det, 0.005^2)): tol of the ratio = t_det0 / det_lo + |ratio| t_det / det_lo + T EPS |ratio|, through
      the square root at the lower end of the interval, + T EPS.
  conics (iyy, -cxy, ixx) / idet: tol = t_num / idet_lo + |num| t_idet / (idet idet_lo) + T EPS |conic|, idet_lo = idet - t_idet.
  depth: z from dP of the centre; |mean_c| = (|x| dx + |y| dy + |z| dz) / |mean_c| + (T + 4) EPS |mean_c|.
  extend = min(3.33, sqrt(2 log(max(op / (1/255), 1)))), op = opacity comp: interval arithmetic on op, T on log and sqrt.
  radii before ceil = min(extend sqrt(cxx), extend sqrt(lambda_max)): first order through every step, T on each sqrt.
      A radius is DECIDED where the float64 value is further from an integer than its bound; decided radii must be equal, the
      others must lie in [ceil(value - bound), ceil(value + bound)]: they may differ by 1 as long as the bound is under a pixel
      (a Gaussian straddling z = 0 under a distorted pinhole has a footprint of 1e5 px and a bound to match).
  validity: every threshold quantity (near, far, det > 0, opacity comp >= 1/255, radius_clip, the four image-bounds tests, the
      quaternion norm; per sigma point: in front, icd > 0.8, angle < max_angle - the fisheye limit is host float32 code and gets
      1e-5 relative on top -, polynomial > 0, the image-with-margin box, the lidar's four field-of-view tests and the distance of
      the relative azimuth from its wrap) carries its own bound. A row is decided INVALID where one test fails by more than its
      bound and decided VALID where all pass by more; sigma points count one by one under require_all_sigma_points_valid and
      through "any point valid" otherwise. A perfect-pinhole / orthographic sigma point whose z is within its bound of 0 (its pixel
      jumps to (0, 0)) leaves the row undecided. At most UNDECIDED_CAP of a case's rows may be undecided, validity and radii
      together.

Every constant above carries a factor >= 2 over what the float32 restatement on the CPU needs: oracle/ut.py run in float32,
worst |err| / bound over all cases (tests/test_ut_cases.py asserts <= 0.5 and prints them; CPU numbers, not GPU numbers):
    means2d 0.24   depths 0.35   conics 0.22   compensations 0.03   (depths 0.42 on a second machine, whose float32 matrix
    products round in another order)
No constant is tuned against the kernel."""
import functools
import math
import os
from collections import namedtuple

import numpy as np
import torch

from oracle import ut as O

EPS = 2.0 ** -24
T = 8.0  # 4 ulp, in units of EPS: atan2f, asinf, sinf, logf, rsqrtf
D = 2.0  # 1 ulp: float32 division and sqrtf (hipcc rounds both correctly by default; twice that is allowed here)
UNDECIDED_CAP = 0.02
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
F32_EPS = float(np.finfo(np.float32).eps)
UT_PARAMS = ((0.1, 2.0, 0.0), (0.5, 1.0, 0.5), (1.0, 0.0, 0.0))
OUTPUTS = ("means2d", "depths", "conics", "compensations")


def f32(x):
    return float(np.float32(x))


def f32list(v):
    return [f32(x) for x in v]


_FT = dict(pixeldist_to_angle_poly=f32list([0.0, 1 / 76.8, 0.0, 2 / 76.8 ** 4, 0.0, 0.0]),
           angle_to_pixeldist_poly=f32list([0.0, 76.8, 0.0, -2.0, 0.0, 0.0]), linear_cde=f32list([1.002, 0.001, -0.0015]))
MODELS = {
    # name: (camera_model, coefficient rows of camera 0 (scaled per camera), f-theta record)
    "pinhole": ("pinhole", {}, None),
    "opencv_full": ("pinhole", dict(radial=[0.12, -0.06, 0.01, 0.02, -0.01, 0.004], tangential=[4e-4, -3e-4],
                                    thin_prism=[0.002, -0.001, 0.0015, 0.0005]), None),
    "opencv_radial4": ("pinhole", dict(radial=[-0.2, 0.05, 0.0, 0.0]), None),
    "opencv_strong": ("pinhole", dict(radial=[-0.45, 0.1, 0.0, 0.0, 0.0, 0.0], tangential=[0.01, 0.01]), None),  # icd < 0.8 at the rim
    "ortho": ("ortho", {}, None),
    "fisheye_plain": ("fisheye", {}, None),
    "fisheye_k": ("fisheye", dict(radial=[-0.04, 0.012, -0.003, 0.0]), None),        # k4 = 0: cubic branch of the limit
    "fisheye_k4": ("fisheye", dict(radial=[0.05, -0.02, 0.004, -0.0015]), None),     # k4 != 0: Newton branch
    "fisheye_tight": ("fisheye", dict(radial=[-0.7, 0.0, 0.0, 0.0]), None),          # monotonic only up to ~0.69 rad: inside the image
    "ftheta_forward": ("ftheta", {}, dict(_FT, reference_poly=1, max_angle=f32(1.2))),
    "ftheta_inverse": ("ftheta", {}, dict(_FT, reference_poly=0, max_angle=f32(0.9))),
    "lidar_cw_120": ("lidar", {}, None), "lidar_ccw_periodic": ("lidar", {}, None), "lidar_ccw_90": ("lidar", {}, None),
}
# phi' = 0.01 + 1.05 phi + 0.02 phi^2 - 0.015 theta + 0.01 phi theta + 0.03 theta^2 and a vertical twin (order 2, not the identity)
WINDSHIELD = dict(horizontal=f32list([0.01, 1.05, 0.02, -0.015, 0.01, 0.03]), vertical=f32list([-0.02, 0.012, -0.02, 0.97, 0.015, -0.01]))

Case = namedtuple("Case", "name model B C N ut require_all margin gz ext opac comp kw misaligned")


def _case_list():
    cases = []

    def add(name, model, ut=0, req=False, margin=0.1, B=2, C=3, N=320, gz=True, ext=False, opac=True, comp=False, kw=(), mis=False):
        cases.append(Case(name, model, B, C, N, ut, req, margin, gz, ext, opac, comp, tuple(kw), mis))

    ut_of = dict(pinhole=0, opencv_full=1, opencv_radial4=2, opencv_strong=0, ortho=1, fisheye_plain=2, fisheye_k=1, fisheye_k4=2,
                 fisheye_tight=1, ftheta_forward=2, ftheta_inverse=1, lidar_cw_120=1, lidar_ccw_periodic=2, lidar_ccw_90=1)
    for i, m in enumerate(MODELS):
        lid = m.startswith("lidar")
        add(m, m, ut=ut_of[m], req=(i % 2 == 1) and not lid, margin=(0.1, 0.05)[i % 2], comp=(i % 3 == 0),
            B=1 if lid else 2, C=2 if lid else 3, N=500 if lid else 320)
    for u in range(3):
        for req in (False, True):
            add(f"pinhole-ut{u}-all{int(req)}", "pinhole", ut=u, req=req, margin=(0.05, 0.1)[(u + req) % 2])
            # with alpha = 0.1 the bound of the opacity-aware extent alone would put > 2 % of the fisheye radii within their bound of
            # an integer: those two run without opacities (extent = 3.33 exactly)
            add(f"fisheye_k-ut{u}-all{int(req)}", "fisheye_k", ut=u, req=req, margin=(0.1, 0.05)[(u + req) % 2], comp=True, opac=u != 0)
    # (f-theta with alpha = 0.1 stays out: its pixel carries ~40 roundings and the share of undecided radii would be ~4 %)
    for m in ("pinhole", "ortho", "fisheye_k"):
        add(f"{m}-windshield", m, ext=True, ut=1, comp=True)
        add(f"{m}-distance", m, gz=False, ut=2)
    add("ftheta_forward-distance", "ftheta_forward", gz=False, ut=1, kw=(("near_plane", 0.5), ("far_plane", 5.0)))
    add("pinhole-no_opacity", "pinhole", opac=False, ut=1)
    add("pinhole-comp_clip", "pinhole", comp=True, kw=(("radius_clip", 2.0), ("eps2d", 0.1), ("near_plane", 0.5), ("far_plane", 5.0)))
    add("opencv_full-clip", "opencv_full", kw=(("radius_clip", 3.0), ("near_plane", 1.0), ("far_plane", 4.0)), ut=2)
    for m in ("pinhole", "opencv_full"):
        u = 0 if m == "pinhole" else 1
        for n in (1, 255, 256, 257, 513):
            add(f"{m}-edge-n{n}", m, B=1, C=1, N=n, comp=True, ut=u)
        add(f"{m}-edge-n257-c3", m, B=1, C=3, N=257, comp=True, ut=u)
        add(f"{m}-edge-n257-misaligned", m, B=1, C=1, N=257, comp=True, mis=True, ut=u)
    return tuple(cases)


CASES = _case_list()
BY_NAME = {c.name: c for c in CASES}
EDGE_CASES = tuple(c.name for c in CASES if "-edge-" in c.name)


def ut_weights32(alpha, beta, kappa):
    """(w_m0, w_c0, w_i, spread) as the host computes them: alpha, beta, kappa arrive as float32, the formulas run in double,
    the results are rounded to float32."""
    return tuple(f32(v) for v in O.ut_weights(f32(alpha), f32(beta), f32(kappa)))


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


def lidar_record(name):
    """dict(h0, hs, v0, vs, ccw) of a golden lidar, the fields of view rounded to float32 as the host passes them."""
    fv0, fvs, fh0, fhs, _, ccw = _golden("lidar_ref.npz")[f"{name}.scalars"][:6]
    return dict(h0=f32(fh0), hs=f32(fhs), v0=f32(fv0), vs=f32(fvs), ccw=int(ccw))


def _cameras(B, C):
    """Per-camera pose, Ks and a scale for the coefficient rows: every one of the B * C cameras differs (focal lengths and
    principal point by >= 10 % from camera to camera)."""
    n = B * C
    vm, Ks, scale = torch.eye(4).repeat(n, 1, 1), torch.zeros(n, 3, 3), torch.zeros(n)
    f = 0.8 * W
    for i in range(n):
        a, b = 0.06 * i - 0.15, 0.03 * i - 0.06
        Ry = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
        vm[i, :3, :3] = Rx @ Ry
        vm[i, :3, 3] = torch.tensor([0.1 * i - 0.25, 0.05 * i - 0.1, 0.02 * i])
        Ks[i] = torch.tensor([[f * 0.8 * 1.12 ** i, 0.0, W / 2 * 0.72 * 1.11 ** i],
                              [0.0, 0.9 * f * 1.35 / 1.12 ** i, H / 2 * 1.3 / 1.12 ** i], [0.0, 0.0, 1.0]])
        scale[i] = 1.0 + 0.15 * i
    return vm.reshape(B, C, 4, 4), Ks.reshape(B, C, 3, 3), scale.reshape(B, C)


def _gaussians(N, seed):
    g = torch.Generator().manual_seed(seed)
    f = 0.8 * W
    z = torch.rand(N, generator=g) * 5.6 + 0.4
    means = torch.stack([(torch.rand(N, generator=g) - 0.5) * 1.5 * W / f * z, (torch.rand(N, generator=g) - 0.5) * 1.5 * H / f * z, z], -1)
    quats = torch.randn(N, 4, generator=g)
    scales = torch.exp(torch.randn(N, 3, generator=g) * 0.5 + math.log(0.05))
    opac = torch.rand(N, generator=g) * 0.95 + 0.05
    idx = torch.arange(N)
    means[(idx % 23 == 22), 2] *= -1.0                       # behind the camera
    opac[idx % 31 == 30] = 0.002                             # far below 1/255
    if N > 24:
        for r, zz in ((1, 0.03), (2, 0.05), (3, 0.08)):     # straddling z = 0 / the near plane: some sigma points behind
            means[r] = torch.tensor([0.01 * r, -0.01, zz])
            scales[r] = 0.3
        quats[5] = 0.0                                       # no orientation
        for r in (12, 13):                                   # well inside every image: the opacity alone decides (see inputs())
            means[r] = torch.tensor([0.1 * (r - 12.5), 0.05, 3.0])
            scales[r] = 0.05
        scales[9, 1] = 0.0                                   # a scale of 0
        scales[10, 2] = F32_EPS                              # a scale of exactly float32 eps (the test is s > eps)
        for k, r in enumerate(range(14, 22)):                # at the image rim: left / right / top / bottom, two depths
            zz = 1.5 + 0.5 * (k // 4)
            means[r] = torch.tensor([(-0.5, 0.5, 0.0, 0.0)[k % 4] * W / f * zz, (0.0, 0.0, -0.5, 0.5)[k % 4] * H / f * zz, zz])
    return means, quats, scales, opac


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The float32 inputs and the parameters of a case: dict(means [B,N,3], quats, scales, opacities or None, viewmats [B,C,4,4],
    Ks, coeffs = dict(radial / tangential / thin_prism -> [B,C,k]), kw = scalar keywords (rounded to float32), weights, ...)."""
    c = BY_NAME[name]
    model, rows, ft = MODELS[c.model]
    kw = dict(eps2d=f32(0.3), near_plane=f32(0.01), far_plane=f32(1e10), radius_clip=0.0)
    kw.update({k: f32(v) for k, v in c.kw})
    out = dict(case=c, camera_model=model, ftheta=ft, lidar=None, kw=kw, coeffs={}, weights=ut_weights32(*UT_PARAMS[c.ut]),
               ext=WINDSHIELD if c.ext else None, width=W, height=H)
    if model == "lidar":
        lname = c.model[len("lidar_"):]
        g = _golden("lidar_ref.npz")
        t = lambda k: torch.from_numpy(g[f"{lname}.cam.{k}"])[None]  # noqa: E731
        out.update(means=t("pts"), quats=t("quats"), scales=t("scales"), opacities=t("opac"), viewmats=t("viewmats"), Ks=t("Ks"),
                   lidar=lidar_record(lname), lidar_name=lname, width=int(g[f"{lname}.column_azimuths_rad"].shape[0]),
                   height=int(g[f"{lname}.row_elevations_rad"].shape[0]))
        return out
    vm, Ks, scale = _cameras(c.B, c.C)
    if model == "ortho":  # a narrower scene at a third of the focal length: the rays (x, y, 1) of the windshield detour stay under ~60 degrees
        Ks[..., 0, 0] *= 0.3
        Ks[..., 1, 1] *= 0.3
    gs = [_gaussians(c.N, 100 * (len(name) + 7 * b) + c.N + b) for b in range(c.B)]
    means, quats, scales, opac = (torch.stack([g[i] for g in gs]) for i in range(4))
    if model == "ortho":
        means[..., :2] *= 0.33
    if c.ut == 0:  # alpha = 0.1: weights of -99 and +16.7 multiply every rounding by ~200, so the bound of a radius grows with the
        # footprint; smaller Gaussians keep the share of radii within their bound of an integer under the cap
        scales *= 0.5
        if c.N > 24:
            scales[:, 10, 2] = F32_EPS
    if c.N > 24:  # the straddling rows again, now that the spread is known: offsets of 0.3 * spread around z = 0.4 .. 0.95 of that
        for r, frac in ((1, 0.4), (2, 0.7), (3, 0.95)):
            scales[:, r] = 0.3
            means[:, r, 2] = frac * 0.3 * out["weights"][3]
        if model in ("fisheye", "ftheta"):  # (their pixel's own roundings grow with the distance from the principal point)
            means[..., 22:, :2] *= 0.5
    for k, row in rows.items():
        out["coeffs"][k] = (torch.tensor(row)[None, None, :] * scale[..., None]).float().contiguous()
    out.update(means=means, quats=quats, scales=scales, opacities=opac if c.opac else None, viewmats=vm, Ks=Ks)
    if c.opac and c.N > 24:  # rows 12 / 13: opacity * compensation just below / above 1/255 in camera (0, 0)
        comp = _run(out, torch.float64, detail=True)[5]["comp"][:, 0]
        for r, s in ((12, 1.0 - 5e-3), (13, 1.0 + 5e-3)):
            opac[:, r] = (O.ALPHA_THRESHOLD * s / comp[:, r]).float()
    return out


def _run(inp, dtype, detail=False, mutate=(), **override):
    """oracle/ut.py on a case's inputs in `dtype` (float64: the reference; float32: the restatement)."""
    a = dict(inp)
    a.update(override)
    c = a["case"]
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    coeffs = {k + "_coeffs": cast(v) for k, v in a["coeffs"].items()}
    limit = a.get("fisheye_limit")
    return O.fully_fused_projection_with_ut(
        cast(a["means"]), cast(a["quats"]), cast(a["scales"]), cast(a["opacities"]), cast(a["viewmats"]), cast(a["Ks"]),
        a["width"], a["height"], calc_compensations=c.comp, camera_model=a["camera_model"],
        in_image_margin_factor=f32(c.margin), require_all_sigma_points_valid=c.require_all, ftheta=a["ftheta"],
        global_z_order=c.gz, ext=a["ext"], lidar=a["lidar"], weights=a["weights"], fisheye_limit=cast(limit), detail=detail,
        mutate=mutate, **a["kw"], **coeffs)


def restate32(name, mutate=(), **override):
    """The float32 restatement (or, with `mutate` / overridden inputs, a wrong one): (radii, means2d, depths, conics, comps)."""
    return _run(inputs(name), torch.float32, mutate=mutate, **override)[:5]


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def _fd_abs_jacobian(fn, X):
    """|d fn / d X| [..., K, 3] by central differences in float64 (fn: [..., 3] -> [..., K])."""
    cols = []
    h = 1e-6 * X.abs().amax(-1, keepdim=True).clamp_min(1e-3)
    for j in range(3):
        e = torch.zeros(3, dtype=X.dtype)
        e[j] = 1.0
        cols.append(((fn(X + h * e) - fn(X - h * e)) / (2.0 * h)).abs())
    return torch.stack(cols, -1)


def _poly_abs(coeffs, x, y):
    return O.bivariate_poly([abs(v) for v in coeffs], x.abs(), y.abs())


def _windshield_rounding(P, model, ext):
    """Absolute error of the windshield's own float32 evaluation on its output Q [..., 3] (exact input)."""
    if model == "ortho":
        P = torch.stack([P[..., 0], P[..., 1], torch.ones_like(P[..., 2])], -1)
    n = P.norm(dim=-1).clamp_min(1e-30)
    sx, sy = (P[..., 0] / n).clamp(-1, 1), (P[..., 1] / n).clamp(-1, 1)
    phi, th = torch.asin(sx), torch.asin(sy)
    dphi = EPS * (3.0 * sx.abs() / torch.sqrt((1 - sx * sx).clamp_min(1e-30)) + T * phi.abs())
    dth = EPS * (3.0 * sy.abs() / torch.sqrt((1 - sy * sy).clamp_min(1e-30)) + T * th.abs())
    h, v = ext["horizontal"], ext["vertical"]
    G = lambda a, b: torch.stack([torch.sin(O.bivariate_poly(h, a, b)), torch.sin(O.bivariate_poly(v, a, b))], -1)  # noqa: E731
    s = 1e-6
    g_phi, g_th = ((G(phi + s, th) - G(phi - s, th)) / (2 * s)).abs(), ((G(phi, th + s) - G(phi, th - s)) / (2 * s)).abs()
    XY = G(phi, th)
    pabs = torch.stack([_poly_abs(h, phi, th), _poly_abs(v, phi, th)], -1)
    dXY = g_phi * dphi[..., None] + g_th * dth[..., None] + 14.0 * EPS * pabs + 0.5 * T * EPS * XY.abs()
    Z = torch.sqrt((1.0 - (XY * XY).sum(-1)).clamp_min(1e-30))
    dZ = ((XY.abs() * dXY).sum(-1) + 2.0 * EPS) / Z + T * EPS * Z
    if model != "ortho":
        return torch.stack([dXY[..., 0], dXY[..., 1], dZ], -1)
    q = XY / Z[..., None]
    dq = (dXY + q.abs() * dZ[..., None]) / Z[..., None] + T * EPS * q.abs()
    return torch.stack([dq[..., 0], dq[..., 1], torch.zeros_like(dZ)], -1), Z, dZ


C_OFFSET = 12.0
C_MODEL = {"pinhole": D + 2.0, "ortho": 1.0, "opencv": D + 14.0, "fisheye": 28.0, "ftheta": 40.0}
Ref = namedtuple("Ref", "radii means2d depths conics compensations info tol valid decided_valid decided_invalid radii_decided "
                        "radii_lo radii_hi undecided_share")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a case with its per-row bounds and decided masks (see the module docstring)."""
    inp = inputs(name)
    return _reference(inp)


def _reference(inp):
    c = inp["case"]
    model = inp["camera_model"]
    f64 = lambda t: None if t is None else t.double()  # noqa: E731
    limit = None
    if model == "fisheye":
        k = f64(inp["coeffs"]["radial"]) if "radial" in inp["coeffs"] else torch.zeros(c.B, c.C, 4, dtype=torch.float64)
        Ks = f64(inp["Ks"])
        limit = O.fisheye_max_angle(k, Ks[..., 0, 0], Ks[..., 1, 1], Ks[..., 0, 2], Ks[..., 1, 2], inp["width"], inp["height"])
    radii, means2d, depths, conics, comps, I = _run(inp, torch.float64, detail=True, fisheye_limit=limit)
    Wd, Hd, margin = inp["width"], inp["height"], f32(c.margin)
    w_m0, w_c0, w_i, spread = inp["weights"]
    means, scales, vm, Ks = f64(inp["means"]), f64(inp["scales"]), f64(inp["viewmats"]), f64(inp["Ks"])
    Rc, tc = vm[..., :3, :3].abs(), vm[..., :3, 3].abs()
    B, C, N = c.B, c.C, means.shape[-2]

    # camera-frame points
    sw = I["sigma_world"].abs()                                                     # [B,N,7,3]
    off = torch.cat([torch.zeros(B, N, 1, dtype=torch.float64), spread * scales, spread * scales], -1)  # [B,N,7]
    e_w = EPS * sw + C_OFFSET * EPS * off[..., None]
    dP = torch.einsum("bcij,bnkj->bcnki", Rc, e_w) + 4.0 * EPS * (torch.einsum("bcij,bnkj->bcnki", Rc, sw) + tc[:, :, None, None, :])
    P = I["cam"]                                                                    # [B,C,N,7,3]

    # windshield
    Q, dQ = I["seen"], dP
    ext_margin = []
    if inp["ext"] is not None:
        fn = lambda X: O.windshield_points(X, model, inp["ext"])[0]  # noqa: E731
        dQ = (_fd_abs_jacobian(fn, P) * dP[..., None, :]).sum(-1)
        own = _windshield_rounding(P, model, inp["ext"])
        if model == "ortho":
            own, Z, dZ = own
            ext_margin = [(P[..., 2], dP[..., 2]), (Z, dZ)]
        dQ = dQ + own

    # the camera model
    par = lambda t: t[:, :, None, None]  # noqa: E731
    fx, fy, cx, cy = par(Ks[..., 0, 0]), par(Ks[..., 1, 1]), par(Ks[..., 0, 2]), par(Ks[..., 1, 2])
    co = {k: f64(v) for k, v in inp["coeffs"].items()}                              # [B,C,k]
    ck = lambda key, i: co[key][..., i][:, :, None, None] if key in co and i < co[key].shape[-1] \
        else torch.zeros(B, C, 1, 1, dtype=torch.float64)  # noqa: E731

    def model_fn(X):  # [B,C,N,7,3] -> pixels
        flat = X.reshape(B, C, N * 7, 3)
        px, _ = O.project_points(flat, model, fx[..., 0], fy[..., 0], cx[..., 0], cy[..., 0], Wd, Hd, margin, co.get("radial"),
                                 co.get("tangential"), co.get("thin_prism"), inp["ftheta"], inp["lidar"],
                                 None if limit is None else limit[..., None])
        return px.reshape(B, C, N, 7, 2)

    J = _fd_abs_jacobian(model_fn, Q)                                               # [B,C,N,7,2,3]
    pix = I["pix"]
    aux = I["aux"]
    if model == "lidar":
        az, el = aux["az"], aux["el"]
        own = torch.stack([1024.0 * EPS * (T * az.abs() + 4.0), 1024.0 * EPS * (T * el.abs() + 4.0 * torch.tan(el).abs())], -1)
    else:
        kind = model if model != "pinhole" else ("opencv" if inp["coeffs"] else "pinhole")
        pp = torch.stack([cx.expand(B, C, N, 7), cy.expand(B, C, N, 7)], -1)
        if model == "ftheta":
            pp = pp + 0.5
        own = EPS * (C_MODEL[kind] * (pix - pp).abs() + pix.abs())
    delta = (J * dQ[..., None, :]).sum(-1) + own                                    # [B,C,N,7,2]
    delta = torch.nan_to_num(delta, nan=math.inf, posinf=math.inf)

    # mean2d and covariance
    wm, wc, d = I["wm"].abs()[..., None], I["wc"].abs()[..., None], I["d"].abs()
    t_mean = (wm * delta).sum(-2) + 8.0 * EPS * (wm * pix.abs()).sum(-2)            # [B,C,N,2]
    e = t_mean
    swc = abs(w_c0 + 6.0 * w_i)
    dw0 = abs(w_c0 - w_m0)
    dx, dy, ex, ey, tx, ty = d[..., 0], d[..., 1], e[..., 0], e[..., 1], delta[..., 0], delta[..., 1]
    wc1 = wc[..., 0]
    t_xx = (wc1 * (2 * dx * tx + tx * tx + 2 * tx * ex[..., None])).sum(-1) + 2 * ex * dw0 * dx[..., 0] + ex * ex * swc \
        + 12.0 * EPS * (wc1 * dx * dx).sum(-1)
    t_yy = (wc1 * (2 * dy * ty + ty * ty + 2 * ty * ey[..., None])).sum(-1) + 2 * ey * dw0 * dy[..., 0] + ey * ey * swc \
        + 12.0 * EPS * (wc1 * dy * dy).sum(-1)
    t_xy = (wc1 * (dx * ty + dy * tx + tx * ty + tx * ey[..., None] + ty * ex[..., None])).sum(-1) \
        + dw0 * (ex * dy[..., 0] + ey * dx[..., 0]) + ex * ey * swc + 12.0 * EPS * (wc1 * dx * dy).sum(-1)

    def t_det(a, b, cc, ta, tb, tcc):
        return b.abs() * ta + a.abs() * tb + 2 * cc.abs() * tcc + ta * tb + tcc * tcc + 3.0 * EPS * ((a * b).abs() + cc * cc)

    c0xx, c0xy, c0yy = I["cov0"].unbind(-1)
    cxx, cxy, cyy = I["cov"].unbind(-1)
    t_det0 = t_det(c0xx, c0yy, c0xy, t_xx, t_yy, t_xy)
    t_bxx, t_byy = t_xx + EPS * cxx.abs(), t_yy + EPS * cyy.abs()
    t_detb = t_det(cxx, cyy, cxy, t_bxx, t_byy, t_xy)
    det0, det, ratio = I["det0"], I["det"], I["ratio"]
    det_lo = (det - t_detb)
    bad = ~(det_lo > 0)
    det_lo = torch.where(bad, torch.ones_like(det_lo), det_lo)
    t_ratio = t_det0 / det_lo + ratio.abs() * t_detb / det_lo + T * EPS * ratio.abs()
    rmin = O.MIN_COMPENSATION ** 2
    rc = ratio.clamp_min(rmin)
    t_comp = t_ratio / (2.0 * torch.sqrt((rc - t_ratio).clamp_min(rmin))) + T * EPS * I["comp"]
    t_comp = torch.where(bad, torch.full_like(t_comp, math.inf), t_comp)

    ixx, iyy = cxx + O.CONIC_EPS, cyy + O.CONIC_EPS
    t_ixx, t_iyy = t_bxx + EPS * ixx.abs(), t_byy + EPS * iyy.abs()
    idet = I["idet"]
    t_idet = t_det(ixx, iyy, cxy, t_ixx, t_iyy, t_xy)
    idet_lo = idet - t_idet
    ibad = ~(idet_lo > 0)
    idet_lo = torch.where(ibad, torch.ones_like(idet_lo), idet_lo)
    con = I["conics"]
    t_con = torch.stack([t_iyy, t_xy, t_ixx], -1) / idet_lo[..., None] \
        + torch.stack([iyy, cxy, ixx], -1).abs() * (t_idet / (idet.abs() * idet_lo))[..., None] + T * EPS * con.abs()
    t_con = torch.where(ibad[..., None], torch.full_like(t_con, math.inf), t_con)

    # depth
    P0, dP0 = P[..., 0, :], dP[..., 0, :]
    t_z = dP0[..., 2]
    dist = I["dist"]
    t_dist = (P0.abs() * dP0).sum(-1) / dist.clamp_min(1e-30) + (T + 4.0) * EPS * dist
    t_depth = t_z if c.gz else t_dist
    t_cull = t_dist if (not c.gz and model in ("ftheta", "lidar")) else t_z

    # extent and radii
    ext_v = I["extend"]
    if I["op"] is not None:
        op = I["op"]
        t_op = f64(inp["opacities"])[:, None, :] * t_comp + EPS * op.abs()
        x = op / O.ALPHA_THRESHOLD
        t_x = t_op / O.ALPHA_THRESHOLD + T * EPS * x.abs()
        L2 = 2.0 * torch.log(x.clamp_min(1.0))
        x_lo = (x - t_x).clamp_min(1.0)
        t_L2 = 2.0 * (torch.log((x + t_x).clamp_min(1.0)) - torch.log(x_lo)) + (T + 1.0) * EPS * L2
        s = torch.sqrt(L2)
        t_s = torch.maximum(torch.sqrt(L2 + t_L2) - s, s - torch.sqrt((L2 - t_L2).clamp_min(0.0))) + T * EPS * s
        t_ext = torch.where(s - t_s > O.GAUSSIAN_EXTEND, torch.zeros_like(t_s), t_s)
        t_ext = torch.nan_to_num(t_ext, nan=math.inf)
    else:
        t_op = None
        t_ext = torch.zeros_like(ext_v)

    def t_sqrt(v, tv):
        return tv / (2.0 * torch.sqrt((v - tv).clamp_min(1e-30))) + T * EPS * torch.sqrt(v.clamp_min(0.0))

    hb = I["hb"]
    t_hb = 0.5 * (t_bxx + t_byy) + EPS * hb.abs()
    disc = (hb * hb - det).clamp_min(O.DISC_MIN)
    t_disc = 2 * hb.abs() * t_hb + t_hb * t_hb + t_detb + 2.0 * EPS * (hb * hb + det.abs())
    t_sq = t_disc / (2.0 * torch.sqrt((disc - t_disc).clamp_min(O.DISC_MIN))) + T * EPS * torch.sqrt(disc)
    lam = I["lam_max"]
    t_lam = t_hb + t_sq + EPS * lam.abs()
    r_eig = I["r_eig"]
    t_reig = ext_v * t_sqrt(lam, t_lam) + torch.sqrt(lam.clamp_min(0)) * t_ext + 2.0 * EPS * r_eig.abs()
    t_pre = []
    for v, tv in ((cxx, t_bxx), (cyy, t_byy)):
        t_ax = ext_v * t_sqrt(v.clamp_min(0), tv) + torch.sqrt(v.clamp_min(0)) * t_ext + 2.0 * EPS * (ext_v * torch.sqrt(v.clamp_min(0)))
        ax_v = ext_v * torch.sqrt(v.clamp_min(0))
        # |min(a, b) - min(a', b')| <= max of the two bounds; where one side wins by more than both bounds, its own bound
        t_pre.append(torch.where(ax_v + t_ax < r_eig - t_reig, t_ax, torch.where(r_eig + t_reig < ax_v - t_ax, t_reig,
                                                                               torch.maximum(t_ax, t_reig))))
    t_pre = torch.nan_to_num(torch.stack(t_pre, -1), nan=math.inf)
    pre = I["pre"]
    radii_decided = ((pre - torch.round(pre)).abs() > t_pre).all(-1) & torch.isfinite(pre).all(-1)
    r_lo, r_hi = torch.ceil(pre - t_pre), torch.ceil(pre + t_pre)

    # ---- validity: (decided true, decided false) per test
    def test(margin_v, tol):
        tol = torch.nan_to_num(tol, nan=math.inf)
        fin = torch.isfinite(margin_v)
        return fin & (margin_v > tol), fin & (margin_v < -tol)

    tests = []
    qn2 = I["qn2"]
    sc_ok = (f64(inp["scales"]) > F32_EPS).all(-1)                                   # exact in any precision
    a_t, a_f = test(qn2 - F32_EPS, 8.0 * EPS * qn2)
    tests.append(((a_t & sc_ok)[:, None, :].expand(B, C, N), (a_f | ~sc_ok)[:, None, :].expand(B, C, N)))
    cull = I["cull_depth"]
    tests.append(test(cull - inp["kw"]["near_plane"], t_cull))
    tests.append(test(inp["kw"]["far_plane"] - cull, t_cull))
    tests.append(test(det, t_detb))
    if I["op"] is not None:
        tests.append(test(I["op"] - O.ALPHA_THRESHOLD, t_op))
    clip = inp["kw"]["radius_clip"]
    tests.append((r_lo.amax(-1) > clip, r_hi.amax(-1) <= clip))
    m2 = I["mean2d"]
    if model != "lidar":
        for ax, size in ((0, Wd), (1, Hd)):
            tb = t_mean[..., ax] + EPS * (m2[..., ax].abs() + r_hi[..., ax])
            tests.append(((m2[..., ax] + r_lo[..., ax] > tb), (m2[..., ax] + r_hi[..., ax] < -tb)))
            tests.append(((size - (m2[..., ax] - r_lo[..., ax]) > tb), (size - (m2[..., ax] - r_hi[..., ax]) < -tb)))

    # per sigma point
    pt = []                                                                          # (margin, tol) [B,C,N,7]
    dQn = dQ.norm(dim=-1)
    zero_jump = None
    if model in ("pinhole", "ortho", "fisheye"):
        pt.append((Q[..., 2], dQ[..., 2]))
        if model != "fisheye" and not inp["coeffs"]:
            zero_jump = ~(Q[..., 2].abs() > dQ[..., 2])                              # the pixel jumps to (0, 0) at z = 0
    pt += ext_margin
    if "icd" in aux:
        u, v = aux["u"], aux["v"]
        zq = Q[..., 2].abs().clamp_min(1e-30)
        du = (dQ[..., 0] + u.abs() * dQ[..., 2]) / zq + T * EPS * u.abs()
        dv = (dQ[..., 1] + v.abs() * dQ[..., 2]) / zq + T * EPS * v.abs()
        r2 = u * u + v * v
        dr2 = 2 * (u.abs() * du + v.abs() * dv) + 3.0 * EPS * r2
        k = [ck("radial", i) for i in range(6)]
        num, den = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2])), 1 + r2 * (k[3] + r2 * (k[4] + r2 * k[5]))
        numa = 1 + r2 * (k[0].abs() + r2 * (k[1].abs() + r2 * k[2].abs()))
        dena = 1 + r2 * (k[3].abs() + r2 * (k[4].abs() + r2 * k[5].abs()))
        dnum = (k[0].abs() + 2 * r2 * k[1].abs() + 3 * r2 * r2 * k[2].abs()) * dr2 + 8.0 * EPS * numa
        dden = (k[3].abs() + 2 * r2 * k[4].abs() + 3 * r2 * r2 * k[5].abs()) * dr2 + 8.0 * EPS * dena
        t_icd = dnum / den.abs() + (num / den).abs() * dden / den.abs() + T * EPS * aux["icd"].abs()
        pt.append((aux["icd"] - O.ICD_MIN, t_icd))
    if "th_full" in aux:
        th = aux["th_full"]
        t_th = dQn / Q.norm(dim=-1).clamp_min(1e-30) + (T + 4.0) * EPS * th
        host = 1e-5 * aux["amax"].abs() if model == "fisheye" else EPS * aux["amax"].abs()
        pt.append((aux["amax"] - th, t_th + host))
        if "poly" in aux:
            kk = [ck("radial", i).abs() for i in range(4)]
            t2 = aux["th"] ** 2
            pabs = aux["th"] * (1 + t2 * (kk[0] + t2 * (kk[1] + t2 * (kk[2] + t2 * kk[3]))))
            pt.append((aux["poly"], 16.0 * EPS * pabs + 10.0 * pabs * t_th / aux["th"].clamp_min(1e-30)))
    if model == "lidar":
        L = inp["lidar"]
        t_az, t_el = delta[..., 0] / 1024.0 + EPS * (aux["az"].abs() + abs(L["h0"])), delta[..., 1] / 1024.0 + EPS * (aux["el"].abs() + abs(L["v0"]))
        m_el, m_az = margin * L["vs"], margin * L["hs"]
        ra, re = aux["rel_az"], aux["rel_el"]
        pt += [(L["vs"] + m_el - re, t_el + 2 * EPS * L["vs"]), (re + m_el, t_el + EPS * m_el),
               (L["hs"] + m_az - ra, t_az + 2 * EPS * L["hs"]), (ra + m_az, t_az + EPS * m_az)]
        if L["hs"] + m_az < O.TWO_PI:  # a relative azimuth next to its wrap jumps by a turn (harmless for a periodic field of view)
            pt.append((torch.minimum(ra, O.TWO_PI - ra), t_az + EPS * O.TWO_PI))
    else:
        mx, my = Wd * margin, Hd * margin
        for ax, size, mm in ((0, Wd, mx), (1, Hd, my)):
            tb = delta[..., ax] + 2.0 * EPS * (size + mm)
            pt += [(pix[..., ax] + mm, tb), (size + mm - pix[..., ax], tb)]
    p_true = torch.ones(B, C, N, 7, dtype=torch.bool)
    p_false = torch.zeros(B, C, N, 7, dtype=torch.bool)
    for mv, tol in pt:
        a, b = test(mv, tol)
        p_true, p_false = p_true & a, p_false | b
    if model in ("pinhole", "ortho") and not inp["coeffs"]:
        # a point behind the camera sits at pixel (0, 0): only "in front" decides it
        behind = test(Q[..., 2], dQ[..., 2])[1]
        p_false = p_false | behind
    if c.require_all:
        tests.append((p_true.all(-1), p_false.any(-1)))
    else:
        tests.append((p_true.any(-1), p_false.all(-1)))

    dec_valid = torch.ones(B, C, N, dtype=torch.bool)
    dec_invalid = torch.zeros(B, C, N, dtype=torch.bool)
    for a, b in tests:
        dec_valid, dec_invalid = dec_valid & a, dec_invalid | b
    if zero_jump is not None:  # the moments of such a row are discontinuous in the inputs: nothing about it is decided ...
        jump = zero_jump.any(-1) & ~dec_invalid  # ... unless another test throws the row out anyway
        dec_valid = dec_valid & ~jump
        radii_decided = radii_decided & ~jump
        for t in (t_mean, t_con):
            t[jump] = math.inf
        t_comp = torch.where(jump, torch.full_like(t_comp, math.inf), t_comp)
    valid = I["valid"]
    assert not bool((dec_valid & ~valid).any()) and not bool((dec_invalid & valid).any()), name_of(c)
    undecided = ~(dec_valid | dec_invalid) | (dec_valid & ~radii_decided)
    I["bounds"] = dict(dP=dP, dQ=dQ, delta=delta, cov0=torch.stack([t_xx, t_xy, t_yy], -1), det0=t_det0, det=t_detb, idet=t_idet,
                       extend=t_ext, pre=t_pre, tests=tests, points=pt)
    tol = dict(means2d=torch.nan_to_num(t_mean, nan=math.inf), depths=t_depth, conics=t_con, compensations=t_comp)
    return Ref(radii, means2d, depths, conics, comps, I, tol, valid, dec_valid, dec_invalid, radii_decided, r_lo, r_hi,
               float(undecided.double().mean()))


def name_of(c):
    return c.name


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def compare(ref, got):
    """`got` = (radii, means2d, depths, conics, comps) on the CPU against a Ref: dict with the worst |err| / bound per output over
    the rows both sides keep (inf for a NaN), and the counts of rows that break a rule: `validity` (a decided row on the wrong
    side), `radii` (a decided radius that differs, an undecided one off by more than 1), `nonzero` (an invalid row that is not
    all zeros). `ok(report)` is the verdict."""
    radii, m2, dep, con, comp = (None if t is None else t.detach().cpu() for t in got)
    vg = (radii > 0).all(-1)
    rep = dict(rows=vg.numel(), kept=int((vg & ref.valid).sum()))
    rep["validity"] = int((ref.decided_valid & ~vg).sum() + (ref.decided_invalid & vg).sum())
    both = vg & ref.valid
    dr = (radii.long() - ref.radii.long()).abs().amax(-1)
    outside = ((radii < ref.radii_lo) | (radii > ref.radii_hi)).any(-1)  # ceil(value -+ bound): one apart while the bound is < 1 px
    rep["radii"] = int((both & ref.radii_decided & (dr != 0)).sum() + (both & ~ref.radii_decided & outside).sum())
    nz = (radii != 0).any(-1) | (m2 != 0).any(-1) | (dep != 0) | (con != 0).any(-1)
    if comp is not None:
        nz = nz | (comp != 0)
    rep["nonzero"] = int((~vg & nz).sum())
    for k, g, r in (("means2d", m2, ref.means2d), ("depths", dep, ref.depths), ("conics", con, ref.conics),
                    ("compensations", comp, ref.compensations)):
        if g is None or r is None:
            assert g is None and r is None, k
            continue
        tol = ref.tol[k]
        mask = both if tol.dim() == both.dim() else both[..., None].expand_as(tol)
        err = (g.double() - r).abs()
        q = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        q = torch.where(torch.isfinite(err), q, torch.full_like(q, math.inf))
        q = torch.where(torch.isinf(tol) & torch.isfinite(err), torch.zeros_like(q), q)
        q = q[mask]
        rep[k] = float(q.max()) if q.numel() else 0.0
        if q.numel():
            i = int(torch.argmax(q))
            rep[k + "_at"] = tuple(int(v) for v in torch.nonzero(mask)[i])
    return rep


def ok(rep, limit=1.0):
    return rep["validity"] == 0 and rep["radii"] == 0 and rep["nonzero"] == 0 and all(rep.get(k, 0.0) <= limit for k in OUTPUTS)


def old_tolerances_pass(ref, got):
    """Would the tolerances the golden tests assert (means2d 2e-2 px, conics 3e-2 relative, radii +- 1, 2 validity flips) let
    `got` through?"""
    radii, m2, dep, con, comp = (None if t is None else t.detach().cpu() for t in got)
    vg = (radii > 0).all(-1)
    both = vg & ref.valid
    if int((vg != ref.valid).sum()) > 2:
        return False
    if not bool(both.any()):
        return True
    return (int((radii.long() - ref.radii.long()).abs()[both].max()) <= 1
            and float((m2.double() - ref.means2d).abs()[both].max()) < 2e-2
            and float(((con.double() - ref.conics).abs() / (ref.conics.abs() + 1e-3))[both].max()) < 3e-2)


def describe(ref, rep, got, key):
    """The row behind the worst ratio of output `key`: indices, both values, the bound and the row's intermediates."""
    at = rep.get(key + "_at")
    if at is None:
        return ""
    row = at[:3]
    g = dict(zip(("radii", "means2d", "depths", "conics", "compensations"), got))[key].detach().cpu()
    I = ref.info
    return (f"{key} at {at}: got {float(g[at]):.9g} ref {float(getattr(ref, key)[at]):.9g} bound {float(ref.tol[key][at]):.3g}; "
            f"pix {I['pix'][row].tolist()} mean2d {I['mean2d'][row].tolist()} cov {I['cov'][row].tolist()} det {float(I['det'][row]):.6g} "
            f"idet {float(I['idet'][row]):.6g}")
