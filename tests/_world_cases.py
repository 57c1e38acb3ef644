"""Cases, float64 reference, per-element error bounds and decided masks for the from-world (3DGUT) compositing pair of
csrc/raster_world.hip (gsx_raster_world_fwd / _bwd behind rasterize_to_pixels_from_world_3dgs). Shared by
tests/test_world_cases.py (CPU: every case reaches its regime, the float32 statement lies inside every bound, wrong
restatements fall outside) and tests/test_gpu_world_fp64.py (GPU: the kernels against the same reference and bounds).

Inputs are float32, made on the CPU (make_scene -> oracle.fully_fused_projection -> oracle.isect_tiles / isect_offset_encode,
rays from oracle.eval3d.pinhole_rays) and uploaded as they are. Any superset list is a valid input of these kernels, so a
builder may cut a tile's list to an exact length (t16_cut) or list every Gaussian in every tile (behind_zero).

The reference is oracle.eval3d.from_world in float64 on those float32 values; gradients are float64 autograd with the decisions
taken as they fell. Every image gets its own leaf copy of means / quats / scales, so the gradients are the kernel's per-(image,
Gaussian) rows before the sum over cameras; the torque column is recovered from the float64 v_q (which is orthogonal to q):
(0, torque) = (|q| / 2) v_q (x) conj(q_unit).

Bounds. u = 2^-24. Every bound counts the roundings of the kernel's own expressions, first order, per sample, and holds with or
without fma contraction (a contraction removes a rounding). |M| is the matrix of absolute values, abscross(a, b) the cross
product with every product taken absolute.
  p = ray_o - mean: u |p|.  o' = M p: E_o = 5 u |M| |p| (M rounded once, p, product, two sums).  u = M ray_d: E_u = 4 u |M| |ray_d|.
  1 / |u|: relative (|d'| . E_u) / |u| + 8 u (three products, two sums, square root, division).  d' = u / |u|: E_d = E_u / |u| +
  |d'| (that + u).  hit_t = -d' . o': E_t = |d'| . E_o + |o'| . E_d + 3 u |d'| . |o'|.
  c = d' x o': E_c = abscross(|d'|, E_o) + abscross(E_d, |o'|) + 2 u abscross(|d'|, |o'|).
  x = -|c|^2 / 2: E_x = |c| . E_c + |E_c|^2 / 2 + 2 u |c|^2. This is the RELATIVE error of G = exp(x) and of alpha; |o'| reaches
  distance / scale, which is why `aniso` has wider bounds than `t16_deep`.
  rho (relative, opacity G and alpha) = E_x + u |x| (the product with log2 e inside __expf) + 16 u (the hardware exponential:
  csrc/raster3d.hpp states ~1e-6 relative for the staged v_exp_f32 form; the guides give no figure) + 3 u (the product with the
  opacity; 0.99f and 1/255f against their decimal values).
  T before sample j: tau_j = sum over the kept samples before it of (alpha rho / (1 - alpha) + 2 u).
  hit distance |scale d' hit_t|: E_g = scale (|d'| E_t + |hit_t| E_d) + 3 u |g|, E_hd = |g| . E_g / hd + 3 u hd.
  facing normal: 7 u relative (three products, two sums, reciprocal square root, product, sign).
  pixel colour: sum_j w_j (|value| (rho + tau + 2 u) + E_value) + n u sum_j w_j |value| (n kept samples, running sum)
      + T_final |background| (tau_final + 2 u) + u |colour|;  alpha = 1 - T_final: T_final tau_final + u;  normals like colours.
  backward: T is rebuilt from T_final = 1 - alpha_f32 by v_rcp_f32 (1 ulp per the public CDNA ISA text = 2 u) products, so
      tau_b = u / T_final (the rounding of alpha near 1: the term a first derivation misses) + 2 sum over the kept samples of
      (alpha rho / (1 - alpha) + 3 u);  alpha T: rho + tau_b + 2 u.
  v_alpha of a sample = sum_k (value_k T - buffer_k / (1 - alpha)) v_c_k + normals likewise + T_final / (1 - alpha) (v_a - bg . v_c):
      every summand with its own factors' errors (1 / (1 - alpha): alpha rho / (1 - alpha) + 3 u; buffer_k: the later samples'
      alpha T errors + n u) + (D + 6) u times the sum of the absolute summands. NOT relative to v_alpha: the summands cancel.
  geometry terms: v_c = -ov v_ov c pushed through v_d = o' x v_c, v_o = v_c x d', v_u = (v_d - d' (d' . v_d)) / |u|, a = M^T v_o,
      b = M^T v_u, torque = -(p x a + ray_d x b), v_scale = -(v_o o' + v_u u) / scale with absolute values ("mag") and with the
      errors above entering one factor at a time ("err", + 3..5 u of each step's own roundings); a sample's bound is
      ov (mag (E_v_alpha + |v_ov| (rho + 4 u)) + |v_ov| err). The hit distance's share goes through the same chain from
      v_g = g / hd alpha T v_c[D - 1], with the direct scale share d' hit_t v_g; the normals' torque n x (alpha T v_n) is relative.
  a row element: the sum of its samples' bounds + (9 + adds) u sum of |terms| for the unordered sums (6 levels of the wave
      reduction, 3 LDS adds of the other waves, one global add per tile list and channel chunk that holds the row).
  v_rays: the same sums per pixel, (n + chunks) u for the running sum.  v_backgrounds = sum T_final v_c over the pixels:
      relative tau_final + u / T_final + 2 u per term, (pixels) u on the sum.  v_quats: the closed form of
      _FromWorldCompositing.backward applied to the torque bound + 10 u of its own; sums over cameras add C u.

A pixel is DECIDED when float64 is outside the sample's own bound on every decision among the samples it evaluates before it
stops, the stopping one included: hit_t against 0 (E_t), alpha against 1/255 (alpha (rho + u)), T (1 - alpha) against 1e-4 (its
relative tau + alpha rho / (1 - alpha) + 3 u), opacity G against 0.99 (ov (rho + u)), the hit distance against 1e-8 (E_hd) and -
where normals are returned - the sign of axis . ray_d (4 u of its absolute sum). Cotangents are zero on undecided pixels, so
every gradient element is compared. At most UNDECIDED_CAP of a case's pixels may be undecided.

Measured (worst |err| / bound; CPU = the float32 statement, tests/test_world_cases.py asserts <= 0.5; GPU = MI355X,
tests/test_gpu_world_fp64.py asserts <= 1):
                 colours  alpha  normals | rows: v_mean  torque  v_scale  v_opacity  v_colors  v_rays | v_quats  v_backgrounds
    CPU (f32)     0.13    0.46    0.06   |       0.033   0.003   0.013     0.039     0.059    0.042  | 0.0006      0.002
    GPU           0.13    0.46    0.03   |       0.31    0.02    0.30      0.32      0.38     0.04   | 0.007       0.02
(the autograd-level v_means / v_scales / v_colors / v_opacities / v_rays equal their row columns to the digits shown). The worst
forward figures are behind_zero's (alpha of saturated pixels: the final rounding of 1 - T is half of its own term u); the worst
GPU gradients are the saturated cases' (t16_deep 0.16..0.25, t16_cut 0.17..0.26, behind_zero 0.30..0.38) where the CPU's float32
autograd sits at 0.005: the kernel rebuilds T from 1 - alpha_f32, autograd does not. Regimes reached (asserted on the CPU):
    case         tiles  longest list  kept / pixel  saturated  behind  clamped  undecided  whole batches skipped
    t16_deep        6      1902         <= 96         100 %     0.9 %     -       0.45 %        10
    t16_cut        12       838         <= 97          29 %     0.6 %     -       0.22 %         4     (lists 0 1 127 128 129 256 257)
    t12_hit5       12       260         <= 29           0 %       -       -       0 %            0
    t8_b2c2        48       208         <= 21           0 %     0.2 %     -       0.13 %         1
    t5_d1          20       135         <= 17           0 %     0.1 %     -       0 %            1
    wide35          6       144         <= 17           0 %     0.3 %     -       0 %            0
    d9 / d17        6    103 / 101      <= 14           0 %     0.1 %     -       0 %            0
    masked(_nobg)  20       156         <= 24           0 %     0.2 %     -       0 %            0     (7 of 20 tiles masked)
    behind_zero     6       100         <= 33          96 %    54.6 %     -       0 %            0     (4.2 % zero rays)
    clamp(_hit)     6        60         <= 2          100 %       -     33.6 %    0.26 %         0
    nonunit         6       220         <= 23           0 %       -       -       0.26 %         0
    aniso           6       143         <= 10           0 %     4.7 %     -       0 %            1
No constant is tuned against the kernel."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from _util import make_scene

U = 2.0 ** -24
EXP_U = 16.0  # hardware exponential, in units of u
UNDECIDED_CAP = 0.05
BATCH = 128  # staging batch of both kernels

# N, W, H, tile; D channels; B batches, C cameras; hit / normals / rays / bg / va (v_render_alphas given) flags
_BASE = dict(N=300, W=40, H=28, ts=16, D=3, B=1, C=1, hit=False, normals=False, rays=False, bg=True, va=True, seed=1,
             scales=(0.05, 0.3), lists="proj", backward=True)
CASES = {
    "t16_deep": dict(N=2500, scales=(0.05, 0.4), seed=11),
    "t16_cut": dict(N=1500, C=2, scales=(0.05, 0.4), seed=12, cut=(0, 1, 127, 128, 129, 256, 257)),
    "t12_hit5": dict(N=400, ts=12, D=5, hit=True, rays=True, seed=13),
    "t8_b2c2": dict(N=300, W=28, H=20, ts=8, B=2, C=2, D=4, hit=True, normals=True, per_camera=True, seed=14),
    "t5_d1": dict(N=200, W=23, H=17, ts=5, D=1, bg=False, va=False, seed=15),
    "wide35": dict(N=200, W=24, H=16, ts=8, D=35, hit=True, normals=True, rays=True, seed=16),
    "d9": dict(N=150, W=24, H=16, ts=8, D=9, seed=17, backward=False),
    "d17": dict(N=150, W=24, H=16, ts=8, D=17, seed=18, backward=False),
    "masked": dict(N=300, ts=8, rays=True, seed=19, masked=True),
    "masked_nobg": dict(N=300, ts=8, rays=True, bg=False, seed=19, masked=True),
    "behind_zero": dict(N=100, W=24, H=16, ts=8, rays=True, seed=20, lists="all", zero_rays=0.05, scales=(0.3, 1.0)),
    "clamp": dict(N=60, W=24, H=16, ts=8, seed=21, scales=(4.0, 12.0), opacity=(0.992, 1.0)),
    "clamp_hit": dict(N=60, W=24, H=16, ts=8, D=4, hit=True, seed=21, scales=(4.0, 12.0), opacity=(0.992, 1.0)),
    "nonunit": dict(N=300, W=24, H=16, ts=8, seed=22, quat_norms=(0.3, 3.0)),
    "aniso": dict(N=300, W=24, H=16, ts=8, seed=23, aniso=True),
}
CASE_NAMES = tuple(CASES)
BACKWARD_CASES = tuple(n for n in CASE_NAMES if CASES[n].get("backward", True))
OUTPUTS_FWD = ("render_colors", "render_alphas", "render_normals")
GRADS = ("v_means", "v_quats", "v_scales", "v_colors", "v_opacities", "v_rays", "v_backgrounds")


def params(name):
    return dict(_BASE, **CASES[name])


def _oracle():
    from oracle import oracle

    return oracle


@functools.lru_cache(maxsize=None)
def case(name):
    """CPU float32 tensors of one case (shared: do not modify): means [B,N,3], quats [B,N,4], scales [B,N,3], colors [I,N,D],
    opacities [I,N], rays [I,H,W,6], offsets int32 [I,th,tw], flatten_ids int32 [M], backgrounds [I,D] / masks bool [I,th,tw]
    or None, and the geometry / flags of the case."""
    from oracle import eval3d as E

    O = _oracle()
    p = params(name)
    N, W, H, ts, D, B, C = (p[k] for k in ("N", "W", "H", "ts", "D", "B", "C"))
    I = B * C
    rng = np.random.default_rng(p["seed"])
    g = torch.Generator().manual_seed(1000 + p["seed"])
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    z_range = (-3.0, 6.0) if p["lists"] == "all" else (2.0, 8.0)
    means, quats, scales, colors, opac, rays, m2s, rads, deps = [], [], [], [], [], [], [], [], []
    for b in range(B):
        sc, _, _ = make_scene(N=N, C=C, width=W, height=H, seed=p["seed"] + 100 * b, scale_range=p["scales"], z_range=z_range)
        if p.get("aniso"):  # ratios up to 1 : 20 with the small axis around 0.01
            s = torch.rand(N, 3, generator=g) * 0.15 + 0.05
            small = torch.randint(0, 3, (N,), generator=g)
            s[torch.arange(N), small] = 0.01 * (0.8 + 0.4 * torch.rand(N, generator=g))
            sc["scales"] = s
        if p.get("quat_norms"):
            lo, hi = p["quat_norms"]
            sc["quats"] = sc["quats"] * (lo + (hi - lo) * torch.rand(N, 1, generator=g))
        if p.get("opacity"):
            lo, hi = p["opacity"]
            sc["opacities"] = lo + (hi - lo) * torch.rand(N, generator=g)
        means.append(sc["means"]); quats.append(sc["quats"]); scales.append(sc["scales"])
        col = torch.rand(C, N, D, generator=g) if p.get("per_camera") else torch.rand(N, D, generator=g)[None].expand(C, N, D)
        op = sc["opacities"][None].expand(C, N)
        if p.get("per_camera"):
            op = op * (0.5 + 0.5 * torch.rand(C, N, generator=g))
        colors.append(col); opac.append(op)
        rays.append(E.pinhole_rays(sc["viewmats"], sc["Ks"], W, H))
        if p["lists"] == "proj":
            rad, m2, d, _, _ = O.fully_fused_projection(sc["means"][None], None, sc["quats"][None], sc["scales"][None],
                                                        sc["viewmats"][None], sc["Ks"][None], W, H)
            m2s.append(m2[0]); rads.append(rad[0] * 2); deps.append(d[0])
        else:  # every Gaussian in every tile, nearest first: a superset of any footprint, behind the camera included
            cam_o = rays[-1][:, 0, 0, :3]
            deps.append((sc["means"][None] - cam_o[:, None]).norm(dim=-1))
    cat = lambda xs: torch.cat(list(xs), 0).contiguous()  # noqa: E731
    if p["lists"] == "proj":
        _, ids, fl = O.isect_tiles(cat(m2s), cat(rads), cat(deps), ts, tw, th)
        off = O.isect_offset_encode(ids, I, tw, th)
    else:
        order = torch.argsort(cat(deps), dim=1)  # [I, N]
        fl = (torch.arange(I)[:, None, None] * N + order[:, None, :]).expand(I, th * tw, N).reshape(-1).to(torch.int32).contiguous()
        off = (torch.arange(I * th * tw, dtype=torch.int32) * N).reshape(I, th, tw)
    if p.get("cut"):  # cut the lists of the longest tiles to exact lengths (any superset list is a valid input)
        start = off.reshape(-1).long().numpy()
        end = np.concatenate([start[1:], [fl.numel()]])
        lens = end - start
        want = lens.copy()
        longest = np.argsort(-lens, kind="stable")[:len(p["cut"])]
        for t, n in zip(longest[rng.permutation(len(longest))], p["cut"]):
            assert lens[t] >= n, (name, int(lens[t]), n)
            want[t] = n
        fl = torch.cat([fl[s:s + n] for s, n in zip(start, want)]).contiguous()
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(want)[:-1]]).astype(np.int32)).reshape(I, th, tw)
    rays = cat(rays).clone()
    if p.get("zero_rays"):
        zero = torch.from_numpy(rng.random((I, H, W)) < p["zero_rays"])
        rays[..., 3:][zero] = 0.0
    masks = None
    if p.get("masked"):
        closed = rng.permutation(I * th * tw)[:round(I * th * tw / 3)]  # a third of the tiles
        masks = torch.ones(I * th * tw, dtype=torch.bool)
        masks[torch.from_numpy(closed)] = False
        masks = masks.reshape(I, th, tw)
    bg = torch.rand(I, D, generator=g) if p["bg"] else None
    return SimpleNamespace(name=name, means=torch.stack(means), quats=torch.stack(quats), scales=torch.stack(scales),
                           colors=cat(colors), opacities=cat(opac), rays=rays.contiguous(), offsets=off, flatten_ids=fl,
                           backgrounds=bg, masks=masks, W=W, H=H, ts=ts, tw=tw, th=th, B=B, C=C, I=I, N=N, D=D, hit=p["hit"],
                           normals=p["normals"], want_rays=p["rays"], va=p["va"], backward=p["backward"],
                           fwd_chunks=(D + 31) // 32, bwd_chunks=(D + 3) // 4)


def list_lengths(cs):
    start = cs.offsets.reshape(-1).long().numpy()
    return np.concatenate([start[1:], [cs.flatten_ids.numel()]]) - start


def abscross(a, b):
    a, b = a.abs(), b.abs()
    ax, ay, az = a.unbind(-1)
    bx, by, bz = b.unbind(-1)
    return torch.stack([ay * bz + az * by, az * bx + ax * bz, ax * by + ay * bx], -1)


def _dot(a, b):
    return (a * b).sum(-1)


def statement(cs, dtype, variant=None, detail=True, requires_grad=True):
    """oracle.eval3d.from_world on the case in `dtype`, every image with its own leaf copy of the Gaussians. Returns (result,
    leaves)."""
    from oracle import eval3d as E

    per_image = lambda x: x.to(dtype).repeat_interleave(cs.C, dim=0).clone().requires_grad_(requires_grad)  # noqa: E731
    lv = dict(means=per_image(cs.means), quats=per_image(cs.quats), scales=per_image(cs.scales),
              colors=cs.colors.to(dtype).clone().requires_grad_(requires_grad),
              opacities=cs.opacities.to(dtype).clone().requires_grad_(requires_grad),
              rays=cs.rays.to(dtype).clone().requires_grad_(requires_grad))
    if cs.backgrounds is not None:
        lv["backgrounds"] = cs.backgrounds.to(dtype).clone().requires_grad_(requires_grad)
    means, quats, scales = lv["means"], lv["quats"], lv["scales"]
    if variant == "batch0":  # (the statement's group 0 is image 0's copy here: take batch 0 for every image instead)
        means, quats, scales = (x.reshape(cs.B, cs.C, cs.N, -1)[:1].expand(cs.B, -1, -1, -1).reshape(x.shape) for x in (means, quats, scales))
        variant = None
    colors, opacities = lv["colors"], lv["opacities"]
    if variant == "camera0":
        colors, opacities = (x.reshape((cs.B, cs.C) + x.shape[1:])[:, :1].expand((cs.B, cs.C) + x.shape[1:]).reshape(x.shape)
                             for x in (colors, opacities))
        variant = None
    r = E.from_world(means, quats, scales, colors, opacities, lv["rays"], cs.W, cs.H, cs.ts, cs.offsets,
                     cs.flatten_ids, backgrounds=lv.get("backgrounds"), masks=cs.masks, use_hit_distance=cs.hit,
                     return_normals=cs.normals, detail=detail, variant=variant)
    return r, lv


def torque_from_v_quats(quats, v_q):
    """(0, torque) = (|q| / 2) v_q (x) conj(q_unit): the inverse of the closed form in _FromWorldCompositing.backward."""
    qn = quats.norm(dim=-1, keepdim=True)
    qu = quats / qn
    qw, qv = qu[..., :1], qu[..., 1:]
    a0, av = v_q[..., :1], v_q[..., 1:]
    return 0.5 * qn * (-a0 * qv + qw * av - torch.linalg.cross(av, qv))


def v_quats_from_torque(quats, tq, absolute=False):
    """The closed form of _FromWorldCompositing.backward; absolute=True: the same map with every product taken absolute."""
    qn_inv = 1.0 / quats.norm(dim=-1, keepdim=True)
    qu = quats * qn_inv
    qw, qv = qu[..., :1], qu[..., 1:]
    if absolute:
        return 2.0 * qn_inv * torch.cat([_dot(tq.abs(), qv.abs())[..., None], qw.abs() * tq.abs() + abscross(tq, qv)], dim=-1)
    return 2.0 * qn_inv * torch.cat([-_dot(tq, qv)[..., None], qw * tq + torch.linalg.cross(tq, qv)], dim=-1)


def gradients(cs, r, lv, cot):
    """Backward of the statement under the cotangents `cot`; returns the rows [I*N, 10 + D] (v_mean | torque | v_scale |
    v_opacity | v_colors), v_rays, the autograd-level gradients (summed over the cameras) and the per-sample v_alpha."""
    loss = (r.renders * cot.v_render.to(r.renders.dtype)).sum()
    if cot.v_alpha is not None:
        loss = loss + (r.alphas * cot.v_alpha.to(r.renders.dtype)).sum()
    if cs.normals:
        loss = loss + (r.normals * cot.v_normals.to(r.renders.dtype)).sum()
    loss.backward()
    I, N, D, B, C = cs.I, cs.N, cs.D, cs.B, cs.C
    z = lambda k: lv[k].grad if lv[k].grad is not None else torch.zeros_like(lv[k])  # noqa: E731
    tq = torque_from_v_quats(lv["quats"].detach(), z("quats"))
    rows = torch.cat([z("means"), tq, z("scales"), z("opacities")[..., None], z("colors")], dim=-1).reshape(I * N, 10 + D)
    per_b = lambda x: x.reshape(B, C, N, -1).sum(1)  # noqa: E731
    out = SimpleNamespace(rows=rows.detach(), v_rays=z("rays").detach(), v_means=per_b(z("means")), v_quats=per_b(z("quats")),
                          v_scales=per_b(z("scales")), v_colors=z("colors").detach(), v_opacities=z("opacities").detach(),
                          v_backgrounds=(z("backgrounds").detach() if "backgrounds" in lv else None),
                          v_sample_alpha=(r.alpha.grad if getattr(r, "alpha", None) is not None and r.alpha.grad is not None else None))
    return out


def _suffix_excl(x):
    """sum over the later list entries (dim 1), exclusive."""
    return torch.flip(torch.cumsum(torch.flip(x, [1]), 1), [1]) - x


def _chain(r, e, Vo, Vo_e, Vd, Vd_e):
    """(v_o, v_d) magnitudes and errors -> mag / err of the mean, torque, scale and ray columns (module docstring)."""
    absM, d, o, u = r.M.abs(), r.d.abs(), r.o.abs(), r.u.abs()
    rn = 1.0 / e.un
    dd = _dot(d, Vd)[..., None]
    Vu = (Vd + d * dd) * rn
    Vu_e = (Vd_e + d * _dot(d, Vd_e)[..., None] + e.E_d * dd + d * _dot(e.E_d, Vd)[..., None]) * rn + Vu * (e.rn_rel[..., None] + 5 * U)
    MT = lambda v: torch.einsum("plij,pli->plj", absM, v)  # noqa: E731
    a_m, b_m = MT(Vo), MT(Vu)
    a_e, b_e = MT(Vo_e) + 4 * U * a_m, MT(Vu_e) + 4 * U * b_m
    p, rd = r.p.abs(), e.rd.abs()
    t_m = abscross(p, a_m) + abscross(rd, b_m)
    t_e = abscross(p, a_e) + abscross(rd, b_e) + 5 * U * t_m
    s_m = (Vo * o + Vu * u) / r.scale
    s_e = (Vo_e * o + Vo * e.E_o + Vu_e * u + Vu * e.E_u) / r.scale + 5 * U * s_m
    return dict(mean=(a_m, a_e), torque=(t_m, t_e), scale=(s_m, s_e), ray_o=(a_m, a_e), ray_d=(b_m, b_e))


def sample_errors(cs, r):
    """Per-sample error quantities of the forward expressions (module docstring), float64 [P, L(, 3)], and the decided mask."""
    P, L = r.rows.shape
    e = SimpleNamespace()
    absM = r.M.abs()
    e.rd = cs.rays.double().reshape(P, 1, 6)[..., 3:].expand(P, L, 3)
    mv = lambda v: torch.einsum("plij,plj->pli", absM, v.abs())  # noqa: E731
    e.E_o = 5 * U * mv(r.p)
    e.E_u = 4 * U * mv(e.rd)
    un = r.u.norm(dim=-1, keepdim=True)
    e.un = torch.where(un > 0, un, torch.ones_like(un))
    d, o = r.d.abs(), r.o.abs()
    e.rn_rel = _dot(d, e.E_u) / e.un[..., 0] + 8 * U
    e.E_d = e.E_u / e.un + d * (e.rn_rel[..., None] + U)
    e.E_t = _dot(d, e.E_o) + _dot(o, e.E_d) + 3 * U * _dot(d, o)
    e.E_c = abscross(d, e.E_o) + abscross(e.E_d, o) + 2 * U * abscross(d, o)
    c2 = _dot(r.c, r.c)
    E_x = _dot(r.c.abs(), e.E_c) + 0.5 * _dot(e.E_c, e.E_c) + 2 * U * c2
    e.rho = E_x + U * 0.5 * c2 + (EXP_U + 3) * U
    a, keep = r.alpha, r.keep
    ra = 1.0 / (1.0 - a)
    step = torch.where(keep, a * e.rho * ra + 2 * U, torch.zeros_like(a))
    e.tau = torch.cumsum(step, 1) - step
    e.tau_final = step.sum(1)
    e.n = keep.sum(1).double()
    e.T_final = (1.0 - r.alphas.reshape(P)).detach()
    # hit distance and the values blended per channel
    D = cs.D
    e.E_val = torch.zeros(P, L, D, dtype=torch.float64)
    if cs.hit:
        gv = r.scale * r.d * r.hit_t[..., None]
        e.g = gv
        e.E_g = r.scale * (d * e.E_t[..., None] + r.hit_t.abs()[..., None] * e.E_d) + 3 * U * gv.abs()
        hd = r.hd
        e.E_hd = torch.where(hd > 0, _dot(gv.abs(), e.E_g) / torch.where(hd > 0, hd, torch.ones_like(hd)), e.E_g.norm(dim=-1)) + 3 * U * hd
        e.E_val[..., D - 1] = e.E_hd
    # decisions of the walked samples
    from oracle.eval3d import ALPHA_THRESHOLD, MAX_ALPHA, TRANSMITTANCE_THRESHOLD

    front = r.hit_t >= 0
    und = r.hit_t.abs() <= e.E_t
    alpha_c = torch.clamp(r.ov, max=MAX_ALPHA)
    und |= front & ((alpha_c - ALPHA_THRESHOLD).abs() <= alpha_c * (e.rho + U))
    Tn = r.T * (1.0 - a)
    und |= r.live & ((Tn - TRANSMITTANCE_THRESHOLD).abs() <= Tn * (e.tau + a * e.rho * ra + 3 * U))
    und |= r.live & ((r.ov - MAX_ALPHA).abs() <= r.ov * (e.rho + U))
    if cs.hit:
        und |= r.keep & ((r.hd - 1e-8).abs() <= e.E_hd)
    if cs.normals:
        ax = r.M[..., 2, :]
        und |= r.keep & (_dot(ax, e.rd).abs() <= 4 * U * _dot(ax.abs(), e.rd.abs()))
    e.decided = ~(und & r.walked).any(1)
    return e


def forward_bounds(cs, r, e):
    P, L = r.rows.shape
    w = torch.where(r.keep, r.alpha * r.T, torch.zeros_like(r.alpha))
    rel = e.rho + e.tau + 2 * U
    val = r.value.abs()
    wv = w[..., None] * val
    col = (wv * rel[..., None] + w[..., None] * e.E_val).sum(1) + (e.n * U)[:, None] * wv.sum(1) + U * r.renders.reshape(P, -1).abs()
    if cs.backgrounds is not None:
        bg = cs.backgrounds.double().repeat_interleave(cs.H * cs.W, dim=0)
        col = col + (e.T_final * (e.tau_final + 2 * U))[:, None] * bg.abs()
    alp = e.T_final * e.tau_final + U
    out = dict(render_colors=col, render_alphas=alp[:, None])
    if cs.normals:
        wn = w[..., None] * r.normal.abs()
        out["render_normals"] = (wn * (rel[..., None] + 7 * U)).sum(1) + (e.n * U)[:, None] * wn.sum(1) + U * r.normals.reshape(P, 3).abs()
    return {k: v.detach() for k, v in out.items()}


def backward_bounds(cs, r, e, cot, v_sample_alpha):
    """Bounds of the rows [I*N, 10 + D], of v_rays [P, 6] and of v_backgrounds [I, D], with the sums of |terms| (mags)."""
    P, L = r.rows.shape
    D, I, N = cs.D, cs.I, cs.N
    keep, a, T = r.keep, r.alpha.detach(), r.T.detach()
    kf = keep.double()
    ra = 1.0 / (1.0 - a)
    v_c = cot.v_render.double().reshape(P, D)
    v_a = cot.v_alpha.double().reshape(P) if cot.v_alpha is not None else torch.zeros(P, dtype=torch.float64)
    Tf = e.T_final
    step = torch.where(keep, a * e.rho * ra + 3 * U, torch.zeros_like(a))
    tau_b = U / Tf + 2 * step.sum(1)  # [P]
    facrel = e.rho + tau_b[:, None] + 2 * U
    fac = a * T * kf
    nU = (e.n * U)[:, None]
    val = r.value.detach().abs()
    # v_alpha of every kept sample
    Bmag = _suffix_excl(fac[..., None] * val)
    Berr = _suffix_excl(fac[..., None] * (val * (facrel + nU)[..., None] + e.E_val))
    ra_rel = (a * e.rho * ra + 3 * U)[..., None]
    avc = v_c.abs()[:, None, :]
    E_va = (avc * ((val * (tau_b[:, None, None] + 2 * U) + e.E_val) * T[..., None] + ra[..., None] * (Bmag * ra_rel + Berr))).sum(-1)
    S_abs = (avc * (val * T[..., None] + ra[..., None] * Bmag)).sum(-1)
    if cs.normals:
        v_n = cot.v_normals.double().reshape(P, 3)
        nv = r.normal.detach().abs()
        nBmag = _suffix_excl(fac[..., None] * nv)
        nBerr = _suffix_excl(fac[..., None] * nv * (facrel + nU + 7 * U)[..., None])
        avn = v_n.abs()[:, None, :]
        E_va = E_va + (avn * (nv * (tau_b[:, None, None] + 9 * U) * T[..., None] + ra[..., None] * (nBmag * ra_rel + nBerr))).sum(-1)
        S_abs = S_abs + (avn * (nv * T[..., None] + ra[..., None] * nBmag)).sum(-1)
    if cs.backgrounds is not None:
        bg = cs.backgrounds.double().repeat_interleave(cs.H * cs.W, dim=0)
        bgdot, bgabs = (bg * v_c).sum(-1), (bg * v_c).abs().sum(-1)
    else:
        bgdot = bgabs = torch.zeros(P, dtype=torch.float64)
    tail = (Tf * (v_a - bgdot).abs())[:, None] * ra
    E_va = E_va + tail * (tau_b[:, None] + ra_rel[..., 0] + 4 * U) + (Tf * (D + 1) * U * (v_a.abs() + bgabs))[:, None] * ra
    S_abs = S_abs + tail
    E_va = (E_va + (D + 6) * U * S_abs) * kf
    from oracle.eval3d import MAX_ALPHA

    unclamped = keep & (r.ov.detach() <= MAX_ALPHA)
    v_alpha = torch.zeros_like(a) if v_sample_alpha is None else v_sample_alpha.detach()
    v_ov = torch.where(unclamped, v_alpha, torch.zeros_like(a)).abs()
    E_vov = torch.where(unclamped, E_va, torch.zeros_like(a))
    ov = r.ov.detach() * kf
    # geometry through alpha, per unit of ov v_ov
    d, o = r.d.abs(), r.o.abs()
    A, EA = r.c.abs(), e.E_c
    Vo = abscross(A, d)
    Vo_e = abscross(EA, d) + abscross(A, e.E_d) + 3 * U * Vo
    Vd = abscross(o, A)
    Vd_e = abscross(e.E_o, A) + abscross(o, EA) + 3 * U * Vd
    unit = _chain(r, e, Vo, Vo_e, Vd, Vd_e)
    scale_m = (ov * v_ov)[..., None]
    scale_e = (ov * (E_vov + v_ov * (e.rho + 4 * U)))[..., None]
    geo = {k: (m * scale_m, m * scale_e + err * scale_m) for k, (m, err) in unit.items()}
    if cs.hit:  # the hit distance's share: from v_g = g / hd * alpha T v_c[D - 1]
        ok = (keep & (r.hd.detach() > 1e-8)).double()
        hd = torch.where(r.hd > 0, r.hd, torch.ones_like(r.hd)).detach()
        v_hd = fac * v_c[:, None, D - 1].abs() * ok
        gabs = e.g.abs() / hd[..., None]
        vg = gabs * v_hd[..., None]
        E_vg = v_hd[..., None] * (e.E_g / hd[..., None] + gabs * (e.E_hd / hd)[..., None]) + vg * (facrel[..., None] + 4 * U)
        sc, t = r.scale, r.hit_t.abs()[..., None]
        mag_t = _dot(sc * d, vg)[..., None]
        E_vt = _dot(sc * e.E_d, vg)[..., None] + _dot(sc * d, E_vg)[..., None] + 5 * U * mag_t
        HVd = sc * t * vg + o * mag_t
        HVd_e = sc * (e.E_t[..., None] * vg + t * E_vg) + e.E_o * mag_t + o * E_vt + 4 * U * HVd
        HVo = d * mag_t
        HVo_e = e.E_d * mag_t + d * E_vt + 2 * U * HVo
        hc = _chain(r, e, HVo, HVo_e, HVd, HVd_e)
        HS = d * t * vg
        HS_e = e.E_d * t * vg + d * e.E_t[..., None] * vg + d * t * E_vg + 3 * U * HS
        hc["scale"] = (hc["scale"][0] + HS, hc["scale"][1] + HS_e)
        geo = {k: (geo[k][0] + hc[k][0], geo[k][1] + hc[k][1]) for k in geo}
    if cs.normals:  # torque of the normals: n x (alpha T v_n), relative
        nt = abscross(r.normal.detach(), fac[..., None] * v_n.abs()[:, None, :])
        geo["torque"] = (geo["torque"][0] + nt, geo["torque"][1] + nt * (facrel[..., None] + 9 * U))
    op_m = r.G.detach() * v_ov * kf
    op_e = r.G.detach() * kf * (E_vov + v_ov * (e.rho + 2 * U))
    col_m = fac[..., None] * avc
    if cs.hit:
        col_m = col_m.clone()
        col_m[..., D - 1] = 0.0  # the colour of that channel is never read
    col_e = col_m * (facrel[..., None] + 2 * U)
    mags = torch.cat([geo["mean"][0], geo["torque"][0], geo["scale"][0], op_m[..., None], col_m], -1)
    errs = torch.cat([geo["mean"][1], geo["torque"][1], geo["scale"][1], op_e[..., None], col_e], -1)
    sel = keep.reshape(-1)
    idx = r.rows.reshape(-1)[sel]
    row_mag = torch.zeros(I * N, 10 + D, dtype=torch.float64).index_add_(0, idx, mags.reshape(P * L, -1)[sel])
    row_err = torch.zeros(I * N, 10 + D, dtype=torch.float64).index_add_(0, idx, errs.reshape(P * L, -1)[sel])
    lists = torch.bincount(cs.flatten_ids.long(), minlength=I * N).double()  # tile lists that hold the row
    adds = 9 + lists * cs.bwd_chunks
    out = SimpleNamespace(rows=row_err + (adds * U)[:, None] * row_mag, rows_sum=(adds * U)[:, None] * row_mag, rows_mag=row_mag)
    ray_m = torch.cat([geo["ray_o"][0], geo["ray_d"][0]], -1) * kf[..., None]
    ray_e = torch.cat([geo["ray_o"][1], geo["ray_d"][1]], -1) * kf[..., None]
    out.v_rays = ray_e.sum(1) + ((e.n + cs.bwd_chunks) * U)[:, None] * ray_m.sum(1)
    if cs.backgrounds is not None:
        term = (Tf[:, None] * v_c.abs()).reshape(I, cs.H * cs.W, D)
        rel = (e.tau_final + U / Tf + 2 * U).reshape(I, cs.H * cs.W, 1)
        out.v_backgrounds = (term * rel).sum(1) + cs.H * cs.W * U * term.sum(1)
    else:
        out.v_backgrounds = None
    return out


def grad_bounds(cs, bb):
    """Bounds of the autograd-level gradients from those of the rows: sums over the C cameras (+ C u), v_quats through the
    closed form (+ 10 u)."""
    B, C, N, D = cs.B, cs.C, cs.N, cs.D
    rows, mag = bb.rows.reshape(B, C, N, -1), bb.rows_mag.reshape(B, C, N, -1)
    s = lambda x, lo, hi: x[..., lo:hi].sum(1)  # noqa: E731
    out = dict(v_means=s(rows, 0, 3) + C * U * s(mag, 0, 3), v_scales=s(rows, 6, 9) + C * U * s(mag, 6, 9),
               v_opacities=bb.rows[:, 9].reshape(B * C, N) + 0.0, v_colors=bb.rows[:, 10:].reshape(B * C, N, D) + 0.0,
               v_rays=bb.v_rays.reshape(cs.I, cs.H, cs.W, 6), v_backgrounds=bb.v_backgrounds)
    q = cs.quats.double()
    tq_b, tq_m = s(rows, 3, 6) + C * U * s(mag, 3, 6), s(mag, 3, 6)
    out["v_quats"] = v_quats_from_torque(q, tq_b, absolute=True) + 10 * U * v_quats_from_torque(q, tq_m, absolute=True)
    return out


def cotangents(cs, decided):
    """Seeded float32 cotangents, exactly zero on undecided pixels (every loc[] of the backward kernel is linear in them)."""
    g = torch.Generator().manual_seed(7000 + params(cs.name)["seed"])
    keep = decided.reshape(cs.I, cs.H, cs.W, 1).float()
    v_r = torch.randn(cs.I, cs.H, cs.W, cs.D, generator=g) * keep
    v_a = torch.randn(cs.I, cs.H, cs.W, 1, generator=g) * keep if cs.va else None
    v_n = torch.randn(cs.I, cs.H, cs.W, 3, generator=g) * keep if cs.normals else None
    return SimpleNamespace(v_render=v_r.contiguous(), v_alpha=v_a, v_normals=v_n)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of one case (shared: do not modify): fwd (renders, alphas, normals, last_ids, sample_counts),
    decided [P], fwd bounds, cotangents, and - for the backward cases - rows, v_rays, gradients and their bounds."""
    cs = case(name)
    r, lv = statement(cs, torch.float64, requires_grad=cs.backward)
    with torch.no_grad():
        e = sample_errors(cs, r)
        fb = forward_bounds(cs, r, e)
    P = cs.I * cs.H * cs.W
    ref = SimpleNamespace(
        render_colors=r.renders.detach().reshape(P, cs.D), render_alphas=r.alphas.detach().reshape(P, 1),
        render_normals=(r.normals.detach().reshape(P, 3) if cs.normals else None), last_ids=r.last_ids.reshape(P),
        sample_counts=r.sample_counts.reshape(P), decided=e.decided, fwd_bounds=fb, blank=~r.open_px | r.zero_ray,
        open_px=r.open_px, zero_ray=r.zero_ray, cot=cotangents(cs, e.decided), detail=None)
    # regime figures for tests/test_world_cases.py
    walked, keep = r.walked, r.keep
    nw = max(int(walked.sum()), 1)
    ref.stats = dict(undecided=1.0 - float(e.decided.double().mean()), behind=float((walked & (r.hit_t < 0)).sum()) / nw,
                     clamped=float((keep & (r.ov > 0.99)).sum()) / max(int(keep.sum()), 1),
                     saturated=float(r.stop.any(1).double().mean()), zero_ray=float(r.zero_ray.double().mean()),
                     masked_px=float((~r.open_px).double().mean()), max_count=int(keep.sum(1).max()),
                     last_batch=int(((r.last_ids.reshape(P) - r.first).clamp(min=0) // BATCH).max()))
    # whole staging batches behind a tile's last contributor (the backward's `t_first = batch_end - wave_bin_final` skip)
    lens = torch.from_numpy(list_lengths(cs))
    last_k = torch.where(ref.last_ids >= 0, ref.last_ids.long() - r.first, torch.full_like(r.first, -1))
    tile_last = torch.full((lens.numel(),), -1, dtype=torch.long).scatter_reduce(0, r.tile, last_k, "amax")
    skipped = torch.where(tile_last >= 0, (lens - 1) // BATCH - tile_last // BATCH, torch.zeros_like(lens))
    ref.stats["skipped_batches"] = int(skipped.max())
    ref.stats["last_at_batch_edge"] = int(((last_k >= 0) & ((last_k % BATCH == 0) | (last_k % BATCH == BATCH - 1))).sum())
    if cs.backward:
        g = gradients(cs, r, lv, ref.cot)
        with torch.no_grad():
            bb = backward_bounds(cs, r, e, ref.cot, g.v_sample_alpha)
        ref.grads, ref.bwd_bounds, ref.grad_bounds = g, bb, grad_bounds(cs, bb)
    return ref


def compare_forward(cs, ref, got):
    """got: dict render_colors [P, D], render_alphas [P, 1], render_normals [P, 3] or None (float tensors on the CPU). Returns
    {output: worst |err| / bound over the decided pixels}."""
    dec = ref.decided
    out = {}
    for k in OUTPUTS_FWD:
        want = getattr(ref, k)
        if want is None:
            continue
        out[k] = ratio((got[k].double().reshape(want.shape) - want)[dec], ref.fwd_bounds[k].expand_as(want)[dec])
    return out


def ratio(err, bound):
    """worst |err| / bound; an element whose bound is 0 must be exactly 0 (ratio inf otherwise)."""
    err, bound = err.double().abs().reshape(-1), bound.double().reshape(-1)
    if err.numel() == 0:
        return 0.0
    q = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max())


def compare_rows(cs, ref, rows, v_rays=None):
    """rows [I*N, 10 + D] (and v_rays [I,H,W,6]) against the reference: {part: worst |err| / bound}."""
    D = cs.D
    cols = dict(v_mean=(0, 3), torque=(3, 6), v_scale=(6, 9), v_opacity=(9, 10), v_colors=(10, 10 + D))
    err = rows.double() - ref.grads.rows
    out = {k: ratio(err[:, lo:hi], ref.bwd_bounds.rows[:, lo:hi]) for k, (lo, hi) in cols.items()}
    if v_rays is not None:
        out["v_rays"] = ratio(v_rays.double().reshape(-1, 6) - ref.grads.v_rays.reshape(-1, 6), ref.bwd_bounds.v_rays)
    return out


def compare_grads(cs, ref, got):
    """got: dict of the autograd-level gradients (missing / None entries are skipped) -> {name: worst |err| / bound}."""
    out = {}
    for k in GRADS:
        want, b = getattr(ref.grads, k), ref.grad_bounds[k]
        if got.get(k) is None or want is None or b is None:
            continue
        out[k] = ratio(got[k].double().reshape(want.shape) - want, b.reshape(want.shape))
    return out
