"""CPU oracle for the Unscented-Transform projection of 3DGUT (TEST INFRASTRUCTURE ONLY; nothing under gsplat_amd/ may
import it).

Restates the behaviour of ``gsplat::projection_ut_3dgs_fused`` (reference kernel
``gsplat/cuda/csrc/ProjectionUT3DGSFused.cu``; the reference's own torch statement of it is
``gsplat/cuda/_torch_impl_ut.py:69-644`` with the camera models of ``gsplat/cuda/_torch_cameras.py``) for the camera
models built so far: perfect pinhole (``_torch_cameras.py:696-757``), OpenCV pinhole with radial / tangential / thin-prism
distortion (``:927-1086``), orthographic (``:793-848``) and OpenCV fisheye (``:1335-1697``: odd 9th-degree polynomial in
the ray angle, clamped at the angle where the polynomial stops being monotonic) and f-theta (``:1786-2056``: pixel distance
as a degree-5 polynomial of the ray angle, or the 3-step Newton inverse of the angle-of-pixel-distance polynomial; affine
(c, d, e) sensor map; principal point shifted by half a pixel), the spinning lidar (image point = (azimuth, elevation) * 1024,
validity from the fields of view grown by the margin, no image-bounds cull) and the bivariate windshield model in front of any
of the cameras (every sigma point is bent before the camera model sees it), all under a GLOBAL shutter; ``global_z_order=False``
(depths = |mean_c|, f-theta and lidar cull near / far on it). The rolling shutter is not restated: its read-out time is
floor(pixel row), so the result is discontinuous at row boundaries and no per-row error bound exists there; the budgeted golden
tests of tests/test_gpu_ut.py and tests/test_gpu_lidar.py remain its check.

The module follows the dtype of its inputs: float64 in, float64 arithmetic (the reference of tests/_ut_cases.py); float32 in,
the float32 restatement those tests hold inside the bounds. Constants the kernel carries as float32 literals (0.8, 1e-6, 3.33,
0.01, 1/255, 0.005, 2 pi) are rounded to float32 here too. ``detail=True`` also returns every intermediate per row; ``mutate``
names deliberate mistakes (MUTATIONS) that tests/test_ut_cases.py must see fall outside the bounds.

Pinned: ``oracle/pin_ut_against_reference.py`` runs the reference's ``_fully_fused_projection_with_ut`` on the CPU — its
parameter records (``torch.classes.gsplat.UnscentedTransformParameters``) come from this backend's
``libgsplat_amd_torch.so`` installed as ``gsplat.csrc`` — and writes ``tests/golden/ut_ref.npz``;
``tests/test_oracle_ut.py`` checks this module against those vectors.

The algorithm, per (camera, Gaussian):
  1. seven sigma points: the mean and mean +- sqrt(3 + lambda) * scale_i * R[:, i], lambda = alpha^2 (3 + kappa) - 3
     (``_torch_impl_ut.py:111-170``);
  2. each is moved to the camera frame and projected by the camera model, which also says whether the point is valid
     (in front, distortion factor > 0.8, inside the image grown by ``in_image_margin_factor``);
  3. mean2d = sum w_m p_i, cov2d = sum w_c (p_i - mean2d)(p_i - mean2d)^T with the UT weights (``:69-108``); when
     ``require_all_sigma_points_valid`` the sums stop at the first invalid point (the kernel's early exit, ``:222-262``);
  4. blur + compensation, determinant / diagonal checks, conic = inverse, opacity-aware extent, eigenvalue-bounded radii,
     radius clip, image-bounds cull (``:470-644``). Invalid rows are zero.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor



def _f32(x: float) -> float:
    """A literal as the kernel carries it: rounded to float32."""
    return float(torch.tensor(x, dtype=torch.float32))


ALPHA_THRESHOLD = _f32(1.0 / 255.0)
MIN_COMPENSATION = _f32(0.005)  # gsplat/cuda/_constants.py
GAUSSIAN_EXTEND, ICD_MIN, CONIC_EPS, DISC_MIN, TWO_PI = _f32(3.33), _f32(0.8), _f32(1e-6), _f32(0.01), _f32(2.0 * math.pi)
LIDAR_PIXELS_PER_RAD = 1024.0
# deliberate mistakes (test infrastructure: each must fall outside the per-row bounds of tests/_ut_cases.py)
MUTATIONS = ("blur_before_det0", "radii_from_eigenvalue", "sum_all_points", "windshield_swapped_angles", "lidar_no_wrap")


def ut_weights(alpha: float, beta: float, kappa: float) -> Tuple[float, float, float, float]:
    """(centre weight of the mean, centre weight of the covariance, weight of the six others, sigma-point spread)."""
    lam = alpha * alpha * (3.0 + kappa) - 3.0
    w0 = lam / (3.0 + lam)
    return w0, w0 + (1.0 - alpha * alpha + beta), 1.0 / (2.0 * (3.0 + lam)), math.sqrt(3.0 + lam)


def _rotmat(quats: Tensor) -> Tensor:
    """Unit quaternion (w, x, y, z) -> rotation matrix; zero-length quaternions stay zero (culled by the caller)."""
    n = quats.norm(dim=-1, keepdim=True)
    q = quats / torch.where(n > 0, n, torch.ones_like(n))
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(q.shape[:-1] + (3, 3))


def _smallest_positive_root(a: Tensor, b: Tensor, c: Tensor) -> Tensor:
    """Smallest positive root of 1 + a x + b x^2 + c x^3 (inf when there is none), branch by branch like the reference
    (``_torch_cameras.py:1531-1621``): linear, quadratic, one real cubic root (Cardano), three real roots (trigonometric)."""
    inf = torch.full_like(a, float("inf"))
    lin = torch.where(a >= 0.0, inf, -1.0 / a)
    dq = a * a - 4.0 * b
    dt = torch.sqrt(dq) - a
    quad = torch.where(dt > 0.0, 2.0 / dt, inf)
    boc = b / c
    t1 = (9.0 * a * boc - 2.0 * b * boc * boc - 27.0) / c
    t2 = 3.0 * a / c - boc * boc
    dc = t1 * t1 + 4.0 * t2 * t2 * t2
    h = (torch.sqrt(dc) + t1) / 2.0
    cr = torch.sign(h) * torch.abs(h) ** (1.0 / 3.0)
    one = torch.where(cr != 0, (cr - t2 / cr - boc) / 3.0, inf)
    one = torch.where(one > 0.0, one, inf)
    th = torch.atan2(torch.sqrt(-dc), t1) / 3.0
    t3 = 2.0 * torch.sqrt(-t2)
    three = inf
    for i in (-1, 0, 1):
        r = (t3 * torch.cos(th + i * (2.0 * math.pi / 3.0)) - boc) / 3.0
        three = torch.minimum(three, torch.where(r > 0.0, r, inf))
    c0, b0 = c.abs() < 1e-10, b.abs() < 1e-10
    out = torch.where(dc < 0.0, three, inf)
    out = torch.where(dc >= 0.0, one, out)
    out = torch.where(c0, torch.where(dq >= 0.0, quad, inf), out)
    return torch.where(c0 & b0, lin, out)


def fisheye_max_angle(k: Tensor, fx: Tensor, fy: Tensor, cx: Tensor, cy: Tensor, width: int, height: int) -> Tensor:
    """Largest ray angle the OpenCV fisheye model projects (``_torch_cameras.py:1344-1521``): where the derivative of
    theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) first vanishes - a cubic in theta^2 when k4 = 0, Newton
    from 1.57 otherwise (20 steps, |step| < 1e-6 = converged) - and never beyond the image corner. k [..., 4]."""
    k1, k2, k3, k4 = k.unbind(-1)
    cubic = torch.sqrt(_smallest_positive_root(3.0 * k1, 5.0 * k2, 7.0 * k3))
    x = torch.full_like(k1, 1.57)
    done = torch.zeros_like(k1, dtype=torch.bool)
    for _ in range(20):
        x2 = x * x
        f = 1.0 + x2 * (3.0 * k1 + x2 * (5.0 * k2 + x2 * (7.0 * k3 + x2 * 9.0 * k4)))
        df = x * (6.0 * k1 + x2 * (20.0 * k2 + x2 * (42.0 * k3 + x2 * 72.0 * k4)))
        dx = f / df
        x = torch.where(done, x, x - dx)
        done = done | (dx.abs() < 1e-6)
    newton = torch.where(done & (x > 0.0), x, torch.full_like(x, float("inf")))
    ang = torch.where(k4.abs() < 1e-10, cubic, newton)
    rx, ry = torch.maximum(width - cx, cx), torch.maximum(height - cy, cy)
    rmax = torch.sqrt(rx * rx + ry * ry)
    return torch.minimum(ang, torch.maximum(rmax / fx, rmax / fy))


def _polyval(coeffs, x: Tensor) -> Tensor:
    """c0 + c1 x + ... by Horner (coeffs: python floats, lowest degree first)."""
    y = torch.full_like(x, float(coeffs[-1]))
    for c in reversed(coeffs[:-1]):
        y = y * x + float(c)
    return y


def bivariate_poly(coeffs, x: Tensor, y: Tensor) -> Tensor:
    """sum_k y^k * (polynomial in x of degree order - k); coeffs: python floats, block k = the order - k + 1 coefficients of
    y^k, lowest power of x first; len(coeffs) = (order + 1)(order + 2) / 2."""
    n = len(coeffs)
    order = int(round((math.sqrt(8 * n + 1) - 3) / 2))
    assert (order + 1) * (order + 2) // 2 == n, "bivariate polynomial: 1, 3, 6, 10, 15 or 21 coefficients"
    outer, start = [], 0
    for k in range(order + 1):
        m = order - k + 1
        outer.append(_polyval(list(coeffs[start:start + m]), x))
        start += m
    r = torch.zeros_like(x)
    for o in reversed(outer):
        r = r * y + o
    return r


def windshield_ray(p: Tensor, horizontal, vertical, mutate=()) -> Tensor:
    """The bivariate windshield model on rays / points p [..., 3]: phi = asin(x / |p|), theta = asin(y / |p|), the two
    polynomials give the angles of the bent ray, x' = sin(H(phi, theta)), y' = sin(V(phi, theta)), z' = sqrt(1 - x'^2 - y'^2)
    with the sign of z. The output is a unit vector; a ray shorter than 1e-6 is returned unchanged."""
    n = p.norm(dim=-1)
    short = n < 1e-6
    safe = torch.where(short, torch.ones_like(n), n)
    phi = torch.asin((p[..., 0] / safe).clamp(-1.0, 1.0))
    theta = torch.asin((p[..., 1] / safe).clamp(-1.0, 1.0))
    x = torch.sin(bivariate_poly(horizontal, phi, theta))
    y = torch.sin(bivariate_poly(vertical, theta, phi) if "windshield_swapped_angles" in mutate
                  else bivariate_poly(vertical, phi, theta))
    z = torch.sqrt(1.0 - (x * x + y * y).clamp(max=1.0)) * torch.where(p[..., 2] < 0.0, -1.0, 1.0).to(p.dtype)
    return torch.where(short[..., None], p, torch.stack([x, y, z], -1))


def windshield_points(p: Tensor, camera_model: str, ext: dict, mutate=()):
    """Camera-frame points as the camera model sees them behind the windshield, and whether the detour itself keeps them: every
    model takes the bent ray, except the orthographic one, whose input is a point: it goes through the ray (x, y, 1) and back
    to (x'/z', y'/z', z) and is dropped when z <= 0 or the bent ray does not point forward."""
    if camera_model != "ortho":
        return windshield_ray(p, ext["horizontal"], ext["vertical"], mutate), torch.ones_like(p[..., 0], dtype=torch.bool)
    o = windshield_ray(torch.stack([p[..., 0], p[..., 1], torch.ones_like(p[..., 2])], -1), ext["horizontal"], ext["vertical"],
                       mutate)
    oz = torch.where(o[..., 2] > 0.0, o[..., 2], torch.ones_like(o[..., 2]))
    x, y = o[..., 0] / oz, o[..., 1] / oz
    ok = (p[..., 2] > 0.0) & (o[..., 2] > 0.0) & torch.isfinite(x) & torch.isfinite(y)
    return torch.stack([x, y, p[..., 2]], -1), ok


def _remainder(x: Tensor, period: float) -> Tensor:
    """torch.remainder for a positive period: the result lies in [0, period)."""
    m = torch.fmod(x, period)
    return torch.where(m < 0.0, m + period, m)


def lidar_project(p: Tensor, lidar: dict, margin: float, mutate=(), aux: Optional[dict] = None):
    """Spinning lidar, global shutter: image point = (atan2(y, x), asin(z / |p|)) * 1024 (angular pixels); valid where the
    azimuth relative to the start of the horizontal field of view (in the spinning direction, wrapped into [0, 2 pi)) and the
    elevation below the top of the vertical one lie inside the spans grown by margin * span. lidar: dict(h0, hs, v0, vs, ccw)."""
    n2 = (p * p).sum(-1)
    inv = torch.where(n2 > 0.0, 1.0 / torch.sqrt(torch.where(n2 > 0.0, n2, torch.ones_like(n2))), torch.zeros_like(n2))
    az, el = torch.atan2(p[..., 1] * inv, p[..., 0] * inv), torch.asin((p[..., 2] * inv).clamp(-1.0, 1.0))
    h0, hs, v0, vs = (float(lidar[k]) for k in ("h0", "hs", "v0", "vs"))
    raw = az - h0 if int(lidar["ccw"]) else h0 - az
    rel_az = raw if "lidar_no_wrap" in mutate else _remainder(raw, TWO_PI)
    rel_el = v0 - el
    m_el, m_az = margin * vs, margin * hs
    ok = (rel_el <= vs + m_el) & (rel_az <= hs + m_az) & (rel_el >= -m_el) & (rel_az >= -m_az)
    if aux is not None:
        aux.update(az=az, el=el, raw_az=raw, rel_az=rel_az, rel_el=rel_el)
    return torch.stack([az * LIDAR_PIXELS_PER_RAD, el * LIDAR_PIXELS_PER_RAD], -1), ok


def project_points(p: Tensor, camera_model: str, fx: Tensor, fy: Tensor, cx: Tensor, cy: Tensor, width: int, height: int,
                   margin: float, radial: Optional[Tensor], tangential: Optional[Tensor], thin_prism: Optional[Tensor],
                   ftheta: Optional[dict] = None, lidar: Optional[dict] = None, fisheye_limit: Optional[Tensor] = None,
                   mutate=(), aux: Optional[dict] = None):
    """Camera-frame points p [..., C, M, 3] -> (pixels [..., C, M, 2], valid [..., C, M]). Per-camera parameters are
    [..., C, 1] (broadcast over M). `fisheye_limit` [..., C, 1]: the fisheye angle limit as the caller computed it (default:
    fisheye_max_angle in this dtype). `aux` (a dict) receives the quantities the model compares with a threshold."""
    if aux is None:
        aux = {}
    if camera_model == "lidar":
        return lidar_project(p, lidar, margin, mutate, aux)
    front = p[..., 2] > 0.0
    if camera_model == "ftheta":
        ax_, ay_ = p[..., 0].abs(), p[..., 1].abs()
        big, small = torch.maximum(ax_, ay_), torch.minimum(ax_, ay_)
        ratio = torch.where(big > 0.0, small / big, torch.zeros_like(big))
        rxy = torch.where(big > 0.0, big * torch.sqrt(1.0 + ratio * ratio), torch.zeros_like(big))
        rxy = torch.where(rxy <= 0.0, torch.full_like(rxy, torch.finfo(torch.float32).eps), rxy)
        th_full = torch.atan2(rxy, p[..., 2])
        th = th_full.clamp(max=float(ftheta["max_angle"]))
        a2p, p2a = list(ftheta["angle_to_pixeldist_poly"]), list(ftheta["pixeldist_to_angle_poly"])
        if int(ftheta["reference_poly"]) == 0:  # the angle-of-distance polynomial is the calibrated one: invert it
            dist = _polyval(a2p, th)
            slope = [k * p2a[k] for k in range(1, 6)]
            done = torch.zeros_like(dist, dtype=torch.bool)
            for _ in range(3):
                step = (_polyval(p2a, dist) - th) / _polyval(slope, dist)
                dist = torch.where(done, dist, dist - step)
                done = done | (step.abs() < 1e-6)
        else:
            dist = _polyval(a2p, th)
        ix, iy = dist * p[..., 0] / rxy, dist * p[..., 1] / rxy
        c_, d_, e_ = (float(v) for v in ftheta["linear_cde"])
        px, py = c_ * ix + d_ * iy + (cx + 0.5), e_ * ix + iy + (cy + 0.5)
        inb = (px >= -width * margin) & (px < width + width * margin) & (py >= -height * margin) & (py < height + height * margin)
        aux.update(th_full=th_full, amax=torch.full_like(th_full, float(ftheta["max_angle"])))
        return torch.stack([px, py], -1), (th_full < float(ftheta["max_angle"])) & inb  # no "in front" test for this model
    if camera_model == "fisheye":
        k = radial if radial is not None else torch.zeros(fx.shape[:-1] + (4,), dtype=p.dtype)
        amax = fisheye_max_angle(k, fx[..., 0], fy[..., 0], cx[..., 0], cy[..., 0], width, height)[..., None] \
            if fisheye_limit is None else fisheye_limit
        ax_, ay_ = p[..., 0].abs(), p[..., 1].abs()
        big, small = torch.maximum(ax_, ay_), torch.minimum(ax_, ay_)
        ratio = torch.where(big > 0.0, small / big, torch.zeros_like(big))
        rxy = torch.where(big > 0.0, big * torch.sqrt(1.0 + ratio * ratio), torch.zeros_like(big))
        rxy = torch.where(rxy <= 0.0, torch.full_like(rxy, torch.finfo(torch.float32).eps), rxy)
        th_full = torch.atan2(rxy, p[..., 2])
        th = torch.minimum(th_full, amax)
        t2 = th * th
        poly = th * (1.0 + t2 * (k[..., 0:1] + t2 * (k[..., 1:2] + t2 * (k[..., 2:3] + t2 * k[..., 3:4]))))
        delta = poly / rxy
        aux.update(th_full=th_full, amax=amax.expand_as(th_full), poly=poly, th=th)
        px, py = delta * p[..., 0] * fx + cx, delta * p[..., 1] * fy + cy
        inb = (px >= -width * margin) & (px < width + width * margin) & (py >= -height * margin) & (py < height + height * margin)
        return torch.stack([px, py], -1), front & (delta > 0.0) & (th_full < amax) & inb
    if camera_model == "ortho":
        u, v = p[..., 0], p[..., 1]
        ok = front
    else:
        u, v = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
        ok = front
        if radial is not None or tangential is not None or thin_prism is not None:
            z = torch.zeros_like(fx)
            k = [z] * 6 if radial is None else [radial[..., i:i + 1] if i < radial.shape[-1] else z for i in range(6)]
            p1, p2 = (z, z) if tangential is None else (tangential[..., 0:1], tangential[..., 1:2])
            s = [z] * 4 if thin_prism is None else [thin_prism[..., i:i + 1] for i in range(4)]
            uu, vv = u * u, v * v
            r2 = uu + vv
            a1, a2, a3 = 2.0 * u * v, r2 + 2.0 * uu, r2 + 2.0 * vv
            icd = (1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) / (1.0 + r2 * (k[3] + r2 * (k[4] + r2 * k[5])))
            du = p1 * a1 + p2 * a2 + r2 * (s[0] + r2 * s[1])
            dv = p1 * a3 + p2 * a1 + r2 * (s[2] + r2 * s[3])
            u, v = icd * u + du, icd * v + dv
            aux.update(icd=icd, u=p[..., 0] / p[..., 2], v=p[..., 1] / p[..., 2])
            ok = ok & (icd > ICD_MIN)  # the distorted model does NOT zero points behind the camera (_torch_cameras.py:1052-1086)
            px, py = u * fx + cx, v * fy + cy
            inb = (px >= -width * margin) & (px < width + width * margin) & (py >= -height * margin) & (py < height + height * margin)
            return torch.stack([px, py], -1), ok & inb
    px, py = u * fx + cx, v * fy + cy
    px, py = torch.where(front, px, torch.zeros_like(px)), torch.where(front, py, torch.zeros_like(py))
    inb = (px >= -width * margin) & (px < width + width * margin) & (py >= -height * margin) & (py < height + height * margin)
    return torch.stack([px, py], -1), ok & inb


def fully_fused_projection_with_ut(
    means: Tensor, quats: Tensor, scales: Tensor, opacities: Optional[Tensor], viewmats: Tensor, Ks: Tensor, width: int,
    height: int, eps2d: float = 0.3, near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0,
    calc_compensations: bool = False, camera_model: str = "pinhole", alpha: float = 0.1, beta: float = 2.0,
    kappa: float = 0.0, in_image_margin_factor: float = 0.1, require_all_sigma_points_valid: bool = False,
    radial_coeffs: Optional[Tensor] = None, tangential_coeffs: Optional[Tensor] = None,
    thin_prism_coeffs: Optional[Tensor] = None, ftheta: Optional[dict] = None, global_z_order: bool = True,
    ext: Optional[dict] = None, lidar: Optional[dict] = None, weights: Optional[Tuple[float, float, float, float]] = None,
    fisheye_limit: Optional[Tensor] = None, detail: bool = False, mutate=(),
):
    """means [..., N, 3], quats [..., N, 4], scales [..., N, 3], opacities [..., N] or None, viewmats [..., C, 4, 4],
    Ks [..., C, 3, 3] -> radii int32 [..., C, N, 2], means2d [..., C, N, 2], depths [..., C, N], conics [..., C, N, 3],
    compensations [..., C, N] or None; with `detail` a sixth value, the dict of every intermediate per row.
    `global_z_order=False`: depths = |mean_c|, and the f-theta and lidar models cull near / far on it. `ext`:
    dict(horizontal, vertical) = the windshield's forward polynomials. `lidar`: dict(h0, hs, v0, vs, ccw). `weights`: the
    (w_m0, w_c0, w_i, spread) to use in place of ut_weights(alpha, beta, kappa) (the kernel receives them as float32).
    `fisheye_limit` [..., C]: the fisheye angle limits to use in place of fisheye_max_angle."""
    if camera_model not in ("pinhole", "ortho", "fisheye", "ftheta", "lidar"):
        raise NotImplementedError(f"oracle.ut: camera model '{camera_model}' is not restated yet")
    assert not set(mutate) - set(MUTATIONS), mutate
    dt = means.dtype
    w_m0, w_c0, w_i, spread = ut_weights(alpha, beta, kappa) if weights is None else weights
    R = _rotmat(quats)  # [..., N, 3, 3], columns = principal axes
    axes = (spread * R * scales[..., None, :]).transpose(-1, -2)  # rows = the three offsets
    sigma = torch.cat([means[..., None, :], means[..., None, :] + axes, means[..., None, :] - axes], dim=-2)  # [..., N, 7, 3]

    Rc, tc = viewmats[..., :3, :3], viewmats[..., :3, 3]
    cam = torch.einsum("...cij,...nkj->...cnki", Rc, sigma) + tc[..., None, None, :]  # [..., C, N, 7, 3]
    lead = cam.shape[:-3]
    N = means.shape[-2]
    par = lambda t: t[..., None]  # noqa: E731  [..., C] -> [..., C, 1]
    seen = cam.reshape(lead + (N * 7, 3))  # what the camera model sees: the points themselves, or the rays the windshield bent
    ext_ok = torch.ones_like(seen[..., 0], dtype=torch.bool)
    if ext is not None:
        seen, ext_ok = windshield_points(seen, camera_model, ext, mutate)
    aux = {}
    pts, ok = project_points(seen, camera_model, par(Ks[..., 0, 0]), par(Ks[..., 1, 1]),
                             par(Ks[..., 0, 2]), par(Ks[..., 1, 2]), width, height, in_image_margin_factor,
                             radial_coeffs, tangential_coeffs, thin_prism_coeffs, ftheta, lidar,
                             None if fisheye_limit is None else par(fisheye_limit), mutate, aux)
    pts = torch.where(ext_ok[..., None], pts, torch.zeros_like(pts))  # a point the orthographic detour drops lands on (0, 0)
    ok = ok & ext_ok
    pts, ok, seen = pts.reshape(lead + (N, 7, 2)), ok.reshape(lead + (N, 7)), seen.reshape(lead + (N, 7, 3))
    aux = {k: v.reshape(lead + (N, 7)) for k, v in aux.items()}

    wm = torch.tensor([w_m0] + [w_i] * 6, dtype=dt)
    wc = torch.tensor([w_c0] + [w_i] * 6, dtype=dt)
    if require_all_sigma_points_valid and "sum_all_points" in mutate:
        valid = ok.all(dim=-1)
    elif require_all_sigma_points_valid:
        upto = torch.cumprod(ok.to(dt), dim=-1)  # 1 until the first invalid point
        valid = upto[..., -1] > 0
        wm, wc = wm * upto, wc * upto
    else:
        valid = ok.any(dim=-1)
    mean2d = (wm[..., None] * pts).sum(dim=-2)
    d = pts - mean2d[..., None, :]
    cxx, cxy, cyy = (wc * d[..., 0] * d[..., 0]).sum(-1), (wc * d[..., 0] * d[..., 1]).sum(-1), (wc * d[..., 1] * d[..., 1]).sum(-1)

    centre = cam[..., 0, :]  # sigma point 0 is the mean
    z, dist = centre[..., 2], centre.norm(dim=-1)
    cull_depth = dist if (not global_z_order and camera_model in ("ftheta", "lidar")) else z  # models that accept z <= 0
    eps = torch.finfo(torch.float32).eps  # the kernel's constant, whatever this module computes in
    qn2 = (quats * quats).sum(-1)
    alive = (qn2 > eps) & (scales > eps).all(-1)  # [..., N]
    sigma_valid = valid
    valid = valid & (cull_depth >= near_plane) & (cull_depth <= far_plane) & alive[..., None, :]

    cov0 = torch.stack([cxx, cxy, cyy], -1)
    if "blur_before_det0" in mutate:
        cxx, cyy = cxx + eps2d, cyy + eps2d
    det0 = cxx * cyy - cxy * cxy
    if "blur_before_det0" not in mutate:
        cxx, cyy = cxx + eps2d, cyy + eps2d
    det = cxx * cyy - cxy * cxy
    ratio = det0 / det
    comp = torch.sqrt(torch.clamp(ratio, min=MIN_COMPENSATION * MIN_COMPENSATION))
    valid = valid & (det > 0.0) & (cxx > 0.0) & (cyy > 0.0)

    ixx, iyy = cxx + CONIC_EPS, cyy + CONIC_EPS  # the reference inverts cov + 1e-6 I (_torch_impl_ut.py:526-528)
    idet = ixx * iyy - cxy * cxy
    conics = torch.stack([iyy / idet, -cxy / idet, ixx / idet], dim=-1)

    extend = torch.full_like(det, GAUSSIAN_EXTEND)
    op = None
    if opacities is not None:
        op = opacities[..., None, :] * comp
        valid = valid & (op >= ALPHA_THRESHOLD)
        extend = torch.minimum(extend, torch.sqrt(2.0 * torch.log(torch.clamp(op / ALPHA_THRESHOLD, min=1.0))))
    b = 0.5 * (cxx + cyy)
    lam_max = b + torch.sqrt(torch.clamp(b * b - det, min=DISC_MIN))
    r_eig = extend * torch.sqrt(lam_max.clamp(min=0.0))
    if "radii_from_eigenvalue" in mutate:
        pre = torch.stack([r_eig, r_eig], -1)
    else:
        pre = torch.stack([torch.minimum(extend * torch.sqrt(cxx.clamp(min=0.0)), r_eig),
                           torch.minimum(extend * torch.sqrt(cyy.clamp(min=0.0)), r_eig)], -1)
    rx, ry = torch.ceil(pre[..., 0]), torch.ceil(pre[..., 1])
    valid = valid & (torch.maximum(rx, ry) > radius_clip)
    if camera_model != "lidar":  # (a lidar's sigma points were tested against its fields of view)
        valid = valid & (mean2d[..., 0] + rx > 0) & (mean2d[..., 0] - rx < width) & (mean2d[..., 1] + ry > 0) & (mean2d[..., 1] - ry < height)

    zero = torch.zeros_like(z)
    radii = torch.where(valid[..., None], torch.stack([rx, ry], -1), zero[..., None]).to(torch.int32)
    means2d = torch.where(valid[..., None], mean2d, zero[..., None])
    depth = z if global_z_order else dist
    depths = torch.where(valid, depth, zero)
    conics_out = torch.where(valid[..., None], conics, zero[..., None])
    comps = torch.where(valid, comp, zero) if calc_compensations else None
    if not detail:
        return radii, means2d, depths, conics_out, comps
    info = dict(sigma_world=sigma, cam=cam, seen=seen, pix=pts, ok=ok, wm=wm.expand(ok.shape), wc=wc.expand(ok.shape),
                mean2d=mean2d, d=d, cov0=cov0, cov=torch.stack([cxx, cxy, cyy], -1), det0=det0, det=det, ratio=ratio, comp=comp,
                idet=idet, conics=conics, op=op, extend=extend, hb=b, lam_max=lam_max, r_eig=r_eig, pre=pre, z=z, dist=dist,
                depth=depth, cull_depth=cull_depth, qn2=qn2, alive=alive, sigma_valid=sigma_valid, valid=valid, aux=aux,
                weights=(w_m0, w_c0, w_i, spread))
    return radii, means2d, depths, conics_out, comps, info
