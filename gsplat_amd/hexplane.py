"""HexPlane feature field of the dynamic-scene trainer (examples/dynamic_surgical_trainer.py; semantics restated from
gsplat/contrib/dynamic/hexplane.py and regulation.py): `HexPlaneField`, the producer of `DeformNetwork`'s ``plane_features``, and
the three regularisers the trainer's loss adds every step.

Per scale the field holds six planes, one per pair of the axes (x, y, z, t) in the order of ``itertools.combinations``: xy, xz,
xt, yz, yt, zt; plane (a, b) is ``[1, C, reso[b], reso[a]]``, coordinate a runs along W and b along H. A point samples each plane
bilinearly (``align_corners=True``, border padding), multiplies the six samples element-wise and concatenates the scales.
x, y, z are mapped to [-1, 1] by ``(xyz - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0``; t is taken as it is.

Fused configuration: float32 CUDA tensors on one device, ``grid_dimensions == 2``, ``input_coordinate_dim == 4``,
``output_coordinate_dim == 32``, 1 to 4 scales, every scaled resolution in [2, 2048], ``0 < N < 2**31``. It takes the kernels of
csrc/hexplane.hip: the planes are packed into a channel-last arena on each forward (one launch per scale), one launch samples
all scales, the backward recomputes the samples, writes ``v_xyzt`` with a fixed-order sum and adds the plane gradients with float
atomics into a gradient arena that is unpacked into the ``[1, C, H, W]`` gradients. ``features`` and ``v_xyzt`` are bit-equal
between runs; the plane gradients are sums of float atomics and may differ in their last bits. Nothing is read back from the
device. A coordinate whose index is clamped at the border passes no gradient. Non-finite coordinates give finite border samples
(a NaN or -inf index samples cell 0 of its axis, +inf the last cell) where grid_sample leaves the result unspecified. Every other
configuration - CPU tensors, other dtypes, channel counts, more scales, an axis of resolution 1 - is evaluated by
`hexplane_torch`, the reference's composition of tensor operations. The fused backward is not itself differentiable.

The regularisers are plain tensor operations.
"""
from __future__ import annotations

import ctypes
import itertools
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

__all__ = ["HexPlaneField", "hexplane", "hexplane_torch", "plane_smoothness", "time_smoothness", "time_l1",
           "hexplane_regularization"]

_DEFAULT_CONFIG = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [64, 64, 64, 25]}
_DEFAULT_MULTIRES = (1, 2)
_MAX_SCALES, _MIN_RES, _MAX_RES, _CHANNELS = 4, 2, 2048, 32


def _make_planes(grid_nd: int, in_dim: int, out_dim: int, reso: Sequence[int], a: float = 0.1, b: float = 0.5) -> nn.ParameterList:
    """One scale: a plane per combination of `grid_nd` of the `in_dim` axes, the later axis outermost. Planes that contain the
    time axis start at one (the product then starts as the spatial planes' alone), the others uniform in [a, b]."""
    if in_dim != len(reso):
        raise ValueError(f"_init_grid_param: in_dim={in_dim} != len(reso)={len(reso)}.")
    if grid_nd > in_dim:
        raise ValueError(f"_init_grid_param: grid_nd={grid_nd} > in_dim={in_dim}.")
    planes = nn.ParameterList()
    for axes in itertools.combinations(range(in_dim), grid_nd):
        p = nn.Parameter(torch.empty([1, out_dim] + [reso[i] for i in reversed(axes)]))
        if in_dim == 4 and 3 in axes:
            nn.init.ones_(p)
        else:
            nn.init.uniform_(p, a=a, b=b)
        planes.append(p)
    return planes


def _check(xyzt: Tensor) -> None:
    if xyzt.shape[-1] != 4:
        raise ValueError(f"HexPlaneField.forward: xyzt last dim must be 4, got shape {tuple(xyzt.shape)}.")


def _sample(plane: Tensor, coords: Tensor) -> Tensor:
    """``plane [1, C, *sizes]`` at ``coords [N, d]`` (d = 2 or 3, first coordinate along the last axis) -> ``[N, C]``."""
    d = coords.shape[-1]
    if d not in (2, 3):
        raise NotImplementedError(f"_grid_sample_wrapper supports 2D / 3D coords only; got {d}D.")
    grid = coords.view([1] * d + [-1, d])
    out = F.grid_sample(plane, grid, align_corners=True, mode="bilinear", padding_mode="border")
    return out.view(plane.shape[1], -1).t()


def hexplane_torch(field: "HexPlaneField", xyzt: Tensor) -> Tensor:
    """`hexplane` composed of torch calls as the reference composes it (any device and dtype, differentiable as far as
    ``grid_sample`` is): the CPU path, the float64 yardstick and the route of every configuration outside the fused one."""
    _check(xyzt)
    aabb = field.aabb
    xyz = (xyzt[..., :3] - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0
    pts = torch.cat([xyz, xyzt[..., 3:]], dim=-1).reshape(-1, 4)
    combos = list(itertools.combinations(range(4), field.grid_config["grid_dimensions"]))
    scales = []
    for planes in field.grids:
        feature = 1.0
        for plane, axes in zip(planes, combos):
            feature = feature * _sample(plane, pts[..., list(axes)])
        scales.append(feature)
    return torch.cat(scales, dim=-1)


class _FusedHexPlane(torch.autograd.Function):
    """csrc/hexplane.hip. ``res`` is the tuple of the scales' (rx, ry, rz, rt); the planes follow scale by scale."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, xyzt, aabb, res, *planes):
        from . import _cabi

        N, S, dev = xyzt.shape[0], len(res), xyzt.device
        cells = [_cabi.query("gsx_hexplane_scale_cells", *r) for r in res]
        arena = torch.empty((sum(cells), _CHANNELS), device=dev, dtype=torch.float32)
        first = 0
        for s, r in enumerate(res):
            _cabi.call("gsx_hexplane_pack", *(p.contiguous() for p in planes[6 * s:6 * s + 6]), *r, arena[first:first + cells[s]])
            first += cells[s]
        x, box = xyzt.contiguous(), aabb.contiguous()
        features = torch.empty((N, S * _CHANNELS), device=dev, dtype=torch.float32)
        _cabi.call("gsx_hexplane_fwd", x, N, box, arena, (ctypes.c_int32 * (4 * S))(*itertools.chain(*res)), S, features)
        _FusedHexPlane.calls += 1
        ctx.save_for_backward(x, box, arena)
        ctx.res, ctx.cells = res, cells
        return features

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_features):
        from . import _cabi

        x, box, arena = ctx.saved_tensors
        res, cells, S = ctx.res, ctx.cells, len(ctx.res)
        want_x, want_planes = ctx.needs_input_grad[0], ctx.needs_input_grad[3:]
        v_x = torch.empty_like(x) if want_x else None
        v_arena = torch.empty_like(arena) if any(want_planes) else None  # zeroed on the stream by the entry point
        _cabi.call("gsx_hexplane_bwd", x, x.shape[0], box, arena, (ctypes.c_int32 * (4 * S))(*itertools.chain(*res)), S,
                   v_features.to(torch.float32).contiguous(), v_x, v_arena)
        v_planes: List[Optional[Tensor]] = [None] * (6 * S)
        first = 0
        for s, (rx, ry, rz, rt) in enumerate(res):
            if any(want_planes[6 * s:6 * s + 6]):
                r = (rx, ry, rz, rt)
                out = [torch.empty((1, _CHANNELS, r[b], r[a]), device=x.device, dtype=torch.float32)
                       for a, b in itertools.combinations(range(4), 2)]
                _cabi.call("gsx_hexplane_unpack", v_arena[first:first + cells[s]], *r, *out)
                for p in range(6):
                    if want_planes[6 * s + p]:
                        v_planes[6 * s + p] = out[p]
            first += cells[s]
        return (v_x, None, None, *v_planes)


def _fused_ok(field: "HexPlaneField", xyzt: Tensor) -> bool:
    cfg = field.grid_config
    if not (cfg.get("grid_dimensions") == 2 and cfg.get("input_coordinate_dim") == 4
            and cfg.get("output_coordinate_dim") == _CHANNELS and 1 <= len(field.grids) <= _MAX_SCALES):
        return False
    for planes in field.grids:
        if len(planes) != 6:
            return False
        r = (planes[0].shape[3], planes[0].shape[2], planes[1].shape[2], planes[2].shape[2])
        if not all(_MIN_RES <= v <= _MAX_RES for v in r):
            return False
        if not all(tuple(p.shape) == (1, _CHANNELS, r[b], r[a]) for p, (a, b) in zip(planes, itertools.combinations(range(4), 2))):
            return False
    tensors = [xyzt, field.aabb] + [p for planes in field.grids for p in planes]
    return (all(t.is_cuda and t.device == xyzt.device and t.dtype == torch.float32 for t in tensors)
            and tuple(field.aabb.shape) == (2, 3) and 0 < xyzt.numel() // 4 < 2 ** 31)


def hexplane(field: "HexPlaneField", xyzt: Tensor) -> Tensor:
    """``[prod(leading), feat_dim]`` plane features of ``xyzt [..., 4]``. The fused configuration (module docstring) runs
    gsx_hexplane_pack / _fwd / _bwd / _unpack; every other one is `hexplane_torch`. No points: an empty result, nothing launched."""
    _check(xyzt)
    if xyzt.numel() == 0:
        return xyzt.new_empty((0, field.feat_dim))
    if not _fused_ok(field, xyzt):
        return hexplane_torch(field, xyzt)
    res = tuple((g[0].shape[3], g[0].shape[2], g[1].shape[2], g[2].shape[2]) for g in field.grids)
    return _FusedHexPlane.apply(xyzt.reshape(-1, 4), field.aabb, res, *(p for g in field.grids for p in g))


class HexPlaneField(nn.Module):
    """The reference's multi-resolution six-plane field. Constructor, attribute and parameter names are the reference's
    (``aabb``, ``grids.{scale}.{plane}``), so a ``state_dict`` moves between the two in either direction with ``strict=True``.

    ``bounds``: half-extent of the spatial box. ``planes_config``: ``grid_dimensions``, ``input_coordinate_dim``,
    ``output_coordinate_dim`` and ``resolution``; default 2, 4, 32 and ``[64, 64, 64, 25]``. ``multires``: the factors on the three
    spatial resolutions, one scale each (the time resolution is the same at every scale); default ``(1, 2)``."""

    _SPATIAL_PLANE_IDXS: Tuple[int, ...] = (0, 1, 3)   # xy, xz, yz
    _TEMPORAL_PLANE_IDXS: Tuple[int, ...] = (2, 4, 5)  # xt, yt, zt

    def __init__(self, bounds: float = 1.6, planes_config: Optional[dict] = None, multires: Optional[Sequence[int]] = None) -> None:
        super().__init__()
        self.bounds = float(bounds)
        self.aabb = nn.Parameter(torch.tensor([[bounds] * 3, [-bounds] * 3], dtype=torch.float32), requires_grad=False)
        self.grid_config = dict(_DEFAULT_CONFIG if planes_config is None else planes_config)
        self.multires = list(_DEFAULT_MULTIRES if multires is None else multires)
        self.concat_features = True
        self.grids = nn.ModuleList()
        self.feat_dim = 0
        cfg = self.grid_config
        for factor in self.multires:
            base = list(cfg["resolution"])
            planes = _make_planes(cfg["grid_dimensions"], cfg["input_coordinate_dim"], cfg["output_coordinate_dim"],
                                  [r * factor for r in base[:3]] + base[3:])
            self.feat_dim += planes[-1].shape[1]
            self.grids.append(planes)

    def forward(self, xyzt: Tensor) -> Tensor:
        """``xyzt [..., 4]`` (world x, y, z and the time coordinate) -> ``[prod(leading), feat_dim]``."""
        return hexplane(self, xyzt)

    def spatial_planes(self) -> List[Tensor]:
        """The xy, xz, yz planes of every scale."""
        return [g[i] for g in self.grids for i in self._SPATIAL_PLANE_IDXS]

    def temporal_planes(self) -> List[Tensor]:
        """The xt, yt, zt planes of every scale."""
        return [g[i] for g in self.grids for i in self._TEMPORAL_PLANE_IDXS]


def _zero_like_first(planes: Sequence[Tensor]) -> Tensor:
    first = next(iter(planes), None)
    if first is None:
        return torch.zeros((), dtype=torch.float32)
    return torch.zeros((), dtype=first.dtype, device=first.device)


def _second_difference(planes: Sequence[Tensor]) -> Tensor:
    total = None
    for p in planes:
        if p.ndim != 4:
            raise ValueError(f"Expected 4D plane tensors (B, C, H, W); got {p.ndim}D shape {tuple(p.shape)}.")
        if p.shape[-2] < 3:
            continue
        d1 = p[..., 1:, :] - p[..., :-1, :]
        term = (d1[..., 1:, :] - d1[..., :-1, :]).pow(2).mean()
        total = term if total is None else total + term
    return _zero_like_first(planes) if total is None else total


def plane_smoothness(planes: Sequence[Tensor]) -> Tensor:
    """Mean squared second difference along H, summed over ``planes`` (``[B, C, H, W]`` each; H < 3 contributes nothing). For
    the spatial planes of a field."""
    return _second_difference(planes)


def time_smoothness(planes: Sequence[Tensor]) -> Tensor:
    """The same sum for the planes that contain the time axis, whose H is time."""
    return _second_difference(planes)


def time_l1(planes: Sequence[Tensor]) -> Tensor:
    """Mean ``|1 - p|``, summed over ``planes``: keeps the time planes near their initial value of one."""
    total = None
    for p in planes:
        term = (1.0 - p).abs().mean()
        total = term if total is None else total + term
    return _zero_like_first(planes) if total is None else total


def hexplane_regularization(field: HexPlaneField, lambda_plane_smooth: float = 1.0, lambda_time_smooth: float = 1.0,
                            lambda_time_l1: float = 1.0) -> Tensor:
    """The weighted sum of the three regularisers over the field's own spatial / temporal partition of its planes."""
    spatial, temporal = field.spatial_planes(), field.temporal_planes()
    return (lambda_plane_smooth * plane_smoothness(spatial) + lambda_time_smooth * time_smoothness(temporal)
            + lambda_time_l1 * time_l1(temporal))
