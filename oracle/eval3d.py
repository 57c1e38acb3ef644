"""CPU oracle for the from-world ("eval3d") compositing of 3DGUT (TEST INFRASTRUCTURE ONLY; nothing under gsplat_amd/ may
import it). The product kernels are csrc/raster_world.hip (gsx_raster_world_fwd / _bwd); this is the
statement they are held to (tests/test_gpu_eval3d.py on the golden vectors, tests/test_gpu_world_fp64.py per element).

Restates ``gsplat::rasterize_to_pixels_from_world_3dgs`` (reference kernels
``gsplat/cuda/csrc/RasterizeToPixelsFromWorld3DGS*.cu``; the reference's torch statement is
``gsplat/cuda/_torch_impl_eval3d.py:135-495``): instead of evaluating a projected 2D conic at the pixel, every sample is
the response of the 3D Gaussian along the pixel's ray,

    M      = S^-1 R^T                               (``_compute_gaussian_transform`` :135-170)
    o', d' = M (ray_o - mean),  M ray_d / |M ray_d| (``_compute_ray_gaussian_distance`` :173-223)
    hit_t  = -d' . o'          (a Gaussian whose closest point lies behind the ray origin contributes nothing)
    dist2  = |d' x o'|^2
    alpha  = min(opacity * exp(-dist2 / 2), 1 - sqrt(1e-4))          (``_compute_gaussian_alphas`` :226-261)

followed by the same front-to-back compositing as the classic path: samples with alpha < 1/255 are skipped, the pixel stops
before the sample that would take the transmittance to <= 1e-4 (``accumulate_eval3d`` :264-495). Gradients come from torch
autograd on this vectorised statement, as the reference obtains its own.

Pinned: ``oracle/pin_eval3d_against_reference.py`` drives the reference's ``accumulate_eval3d`` (with a restated nerfacc,
as ``pin_against_reference.py`` does for the classic ``accumulate``) on the same candidate lists and writes
``tests/golden/eval3d_ref.npz``; ``tests/test_oracle_eval3d.py`` checks this module against those vectors.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional, Tuple

import torch
from torch import Tensor

ALPHA_THRESHOLD = 1.0 / 255.0
TRANSMITTANCE_THRESHOLD = 1e-4
MAX_ALPHA = 1.0 - math.sqrt(TRANSMITTANCE_THRESHOLD)


def _rotmat(q: Tensor) -> Tensor:
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(q.shape[:-1] + (3, 3))


def pinhole_rays(viewmats: Tensor, Ks: Tensor, width: int, height: int) -> Tensor:
    """World-space rays through the pixel centres of perfect pinhole cameras: [C, H, W, 6] = origin | unit direction
    (``_generate_rays`` :91-132 for the pinhole model: direction = R^T K^-1 (x + 0.5, y + 0.5, 1), origin = -R^T t)."""
    C = viewmats.shape[0]
    ys, xs = torch.meshgrid(torch.arange(height, dtype=viewmats.dtype), torch.arange(width, dtype=viewmats.dtype), indexing="ij")
    fx, fy, cx, cy = (Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2])
    d = torch.stack([(xs[None] + 0.5 - cx[:, None, None]) / fx[:, None, None],
                     (ys[None] + 0.5 - cy[:, None, None]) / fy[:, None, None],
                     torch.ones(C, height, width, dtype=viewmats.dtype)], dim=-1)
    d = d / d.norm(dim=-1, keepdim=True)
    R, t = viewmats[:, :3, :3], viewmats[:, :3, 3]
    d_w = torch.einsum("cji,chwj->chwi", R, d)
    o_w = -torch.einsum("cji,cj->ci", R, t)
    return torch.cat([o_w[:, None, None, :].expand(C, height, width, 3), d_w], dim=-1)


def candidate_lists(isect_offsets: Tensor, flatten_ids: Tensor, width: int, height: int, tile_size: int) -> Tuple[Tensor, Tensor]:
    """Per pixel, the depth-sorted rows of its tile, padded: (rows int64 [I*H*W, L], present bool [I*H*W, L])."""
    I, th, tw = isect_offsets.shape
    off = torch.cat([isect_offsets.reshape(-1).long(), torch.tensor([flatten_ids.numel()])])
    lens = off[1:] - off[:-1]
    L = int(lens.max()) if lens.numel() else 0
    ys, xs = torch.meshgrid(torch.arange(height), torch.arange(width), indexing="ij")
    tile = (ys // tile_size) * tw + (xs // tile_size)  # [H, W]
    tile = (torch.arange(I)[:, None, None] * (th * tw) + tile[None]).reshape(-1)  # [I*H*W]
    k = torch.arange(max(L, 1))
    present = k[None, :] < lens[tile][:, None]
    idx = (off[tile][:, None] + k[None, :]).clamp(max=max(flatten_ids.numel() - 1, 0))
    rows = flatten_ids.long()[idx] if flatten_ids.numel() else torch.zeros_like(idx)
    return rows, present


def from_world(
    means: Tensor, quats: Tensor, scales: Tensor, colors: Tensor, opacities: Tensor, rays: Tensor, image_width: int,
    image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor, backgrounds: Optional[Tensor] = None,
    masks: Optional[Tensor] = None, use_hit_distance: bool = False, return_normals: bool = False, detail: bool = False,
    variant: Optional[str] = None,
):
    """The whole statement of gsx_raster_world_fwd, in the dtype of `means` (float32: M = S^-1 R^T assembled in float64 and
    rounded once, the kernel's contract; float64: nothing is rounded).

    means [G,N,3] / quats [G,N,4] / scales [G,N,3] (or without G): G groups of Gaussians shared by I / G consecutive images each
    (G = B batches of C cameras; G = I gives every image its own copy, whose gradients are the kernel's per-image rows);
    colors [I,N,D], opacities [I,N], rays [I,H,W,6] (a zero direction takes no samples), isect_offsets int32 [I,th,tw],
    flatten_ids int32 [M] (row = image * N + gaussian), backgrounds [I,D] or None, masks bool [I,th,tw] or None (a False tile
    shows its background - or 0 - and nothing else). use_hit_distance: the last channel of a sample is |scale * d' hit_t|
    instead of its colour; return_normals: sum of weight * the Gaussian's third axis turned to face the ray.
    Differentiable in means / quats / scales / colors / opacities / rays / backgrounds.

    Returns a namespace: renders [I,H,W,D], alphas [I,H,W,1], last_ids int32 [I,H,W] (position in flatten_ids, -1: none),
    sample_counts int32 [I,H,W], normals [I,H,W,3] or None; with detail=True also the per-sample intermediates, [P, L] over
    the pixels (image, row, column) and the padded list of the pixel's tile: rows, present, M [P,L,3,3], p = ray_o - mean,
    o (o'), u = M ray_d, d (d'), hit_t, c = d' x o', ov = opacity G, alpha (clamped, 0 where not live; retains its gradient),
    T (before the sample), live, keep, stop (the sample the pixel stopped at), walked (evaluated before or at the stop), hd,
    normal [P,L,3], value [P,L,D] (the blended channel values), tile [P] and first (position of the tile's list in flatten_ids).

    `variant` names a deliberately WRONG restatement (tests/test_world_cases.py shows each falls outside the bounds)."""
    dt = means.dtype
    I, N, D = colors.shape
    H, W = image_height, image_width
    P = I * H * W
    means, quats, scales = means.reshape(-1, N, 3), quats.reshape(-1, N, 4), scales.reshape(-1, N, 3)
    per_group = I // means.shape[0]
    rows, present = candidate_lists(isect_offsets, flatten_ids, W, H, tile_size)  # [P, L]
    L = rows.shape[1]
    g = rows % N
    img = torch.arange(I).repeat_interleave(H * W)[:, None].expand_as(rows)
    grp = img // per_group
    if variant == "batch0":
        grp = torch.zeros_like(grp)
    cam = img if variant != "camera0" else (img // per_group) * per_group
    _, th, tw = isect_offsets.shape
    off = torch.cat([isect_offsets.reshape(-1).long(), torch.tensor([flatten_ids.numel()])])
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tile = (torch.arange(I)[:, None, None] * (th * tw) + ((ys // tile_size) * tw + (xs // tile_size))[None]).reshape(-1)
    if masks is not None:
        open_px = masks.reshape(-1).bool()[tile]
        present = present & open_px[:, None]
    else:
        open_px = torch.ones(P, dtype=torch.bool)
    ray = rays.reshape(P, 6)
    zero_ray = (ray[:, 3:] == 0).all(-1)
    if variant != "zero_ray_samples":
        present = present & ~zero_ray[:, None]
    # [G,N,3,3] = S^-1 R^T: its entries reach 1 / min scale and every later product inherits their rounding, so the float32
    # statement assembles it in float64 and rounds once, as the reference (:158-165) and the kernel do
    if variant == "m_f32":
        Mg = torch.diag_embed(1.0 / scales) @ _rotmat(quats).transpose(-1, -2)
    else:
        Mg = (torch.diag_embed(1.0 / scales.double()) @ _rotmat(quats.double()).transpose(-1, -2)).to(dt)
    M = Mg[grp, g]  # [P, L, 3, 3]
    p = ray[:, None, :3] - means[grp, g]
    rd = ray[:, None, 3:].expand_as(p)
    o = torch.einsum("plij,plj->pli", M, p)
    u = torch.einsum("plij,plj->pli", M, rd)
    un = u.norm(dim=-1, keepdim=True)
    d = u / torch.where(un > 0, un, torch.ones_like(un))
    hit_t = -(d * o).sum(-1)
    c = torch.linalg.cross(d, o)
    G = torch.exp(-0.5 * (c * c).sum(-1))
    ov = opacities[cam, g] * G
    alpha = torch.clamp(ov, max=MAX_ALPHA)
    if variant == "clamp_geometry_on":
        alpha = ov + (alpha - ov).detach()
    live = present & (hit_t >= 0.0) & (alpha >= ALPHA_THRESHOLD)
    a = torch.where(live, alpha, torch.zeros_like(alpha))
    if detail and a.requires_grad:
        a.retain_grad()
    T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), 1.0 - a[:, :-1]], dim=1), dim=1)
    fails = live & ~(T * (1.0 - a) > TRANSMITTANCE_THRESHOLD)
    # a pixel STOPS at the first sample that fails the transmittance test: that sample and the later ones do not contribute
    n_fail = torch.cumsum(fails.long(), dim=1)
    stop = fails & (n_fail == 1)
    keep = live & (n_fail == 0)
    if variant == "stop_blended":
        keep = keep | stop
    wgt = torch.where(keep, a * T, torch.zeros_like(a))
    scl = scales[grp, g]
    scl_hd = scl.detach() if variant == "scale_no_direct_share" else scl
    value = colors[cam, g]
    hd = None
    if use_hit_distance:
        gv = (scl_hd if variant != "hd_no_scale" else torch.ones_like(scl)) * (d if variant != "hd_raw_direction" else u) \
            * hit_t[..., None]
        g2 = (gv * gv).sum(-1)
        # (the square root of an exact 0 has no gradient; the kernel gives such a sample none: `hd > 1e-8`)
        hd = torch.where(g2 > 1e-16, torch.sqrt(torch.where(g2 > 1e-16, g2, torch.ones_like(g2))), torch.zeros_like(g2))
        k_hd = D - 1 if variant != "hd_channel3" else min(3, D - 1)
        value = torch.cat([value[..., :k_hd], hd[..., None], value[..., k_hd + 1:]], dim=-1)
    renders = torch.einsum("pl,pld->pd", wgt, value)
    alphas = wgt.sum(-1, keepdim=True)
    T_final = torch.where(keep, 1.0 - a, torch.ones_like(a)).prod(dim=1, keepdim=True)
    if variant == "stop_blended":
        T_final = 1.0 - alphas
    normal = normals = None
    if return_normals:
        ax = M[..., 2, :]
        n0 = ax / ax.norm(dim=-1, keepdim=True)
        facing = torch.where((ax * rd).sum(-1, keepdim=True) > 0, -1.0, 1.0).to(dt)
        normal = n0 * facing if variant != "normal_not_facing" else n0
        normals = torch.einsum("pl,pli->pi", wgt, normal).reshape(I, H, W, 3)
    if backgrounds is not None:
        bg = backgrounds.repeat_interleave(H * W, dim=0)
        if variant == "masked_zero":
            bg = bg * open_px[:, None].to(dt)
        T_bg = {"bg_without_T": torch.ones_like(T_final), "v_alpha_without_bg": T_final.detach()}.get(variant, T_final)
        renders = renders + T_bg * bg
    # alpha = 1 - T_final, as the kernel writes it (the sum of the weights telescopes to the same value)
    alphas = 1.0 - T_final
    if variant == "v_alphas_every_chunk":  # the backward walks ceil(D / 4) channel chunks
        alphas = alphas.detach() + ((D + 3) // 4) * (alphas - alphas.detach())
    k = torch.arange(L)[None, :].expand_as(rows)
    last_k = torch.where(keep, k, torch.full_like(k, -1)).max(dim=1).values
    last_ids = torch.where(last_k >= 0, off[tile] + last_k, torch.full_like(last_k, -1)).to(torch.int32)
    out = SimpleNamespace(renders=renders.reshape(I, H, W, D), alphas=alphas.reshape(I, H, W, 1), last_ids=last_ids.reshape(I, H, W),
                          sample_counts=keep.sum(1).to(torch.int32).reshape(I, H, W), normals=normals)
    if detail:
        walked = present & (torch.cumsum(fails.long(), dim=1) - fails.long() == 0)
        out.__dict__.update(rows=rows, present=present, M=M, p=p, o=o, u=u, d=d, hit_t=hit_t, c=c, ov=ov, alpha=a, T=T, live=live,
                            keep=keep, stop=stop, walked=walked, hd=hd, normal=normal, value=value, first=off[tile], tile=tile,
                            open_px=open_px, zero_ray=zero_ray, scale=scl, opacity=opacities[cam, g], G=G)
    return out


def rasterize_to_pixels_eval3d(
    means: Tensor, quats: Tensor, scales: Tensor, colors: Tensor, opacities: Tensor, rays: Tensor, image_width: int,
    image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor, backgrounds: Optional[Tensor] = None,
):
    """means [N,3], quats [N,4], scales [N,3] (one batch), colors [I,N,D], opacities [I,N], rays [I,H,W,6],
    isect_offsets int32 [I,th,tw], flatten_ids int32 [M] (row = image * N + gaussian, depth-sorted per tile) ->
    (renders [I,H,W,D], alphas [I,H,W,1], last_ids int32 [I,H,W] = position in flatten_ids of the last sample, -1 if none).
    Differentiable in means / quats / scales / colors / opacities / rays / backgrounds. The plain form of `from_world`."""
    r = from_world(means, quats, scales, colors, opacities, rays, image_width, image_height, tile_size, isect_offsets,
                   flatten_ids, backgrounds=backgrounds)
    return r.renders, r.alphas, r.last_ids
