"""Bilateral-grid appearance model: the per-image colour correction that the reference trainer applies between the render and
the loss with ``post_processing="bilateral_grid"`` (examples/simple_trainer.py:571-577, 766-776, 981-984; semantics restated
from examples/lib_bilagrid.py:110-295).

Every training image owns a grid ``[12, L, Hg, Wg]`` of 3 x 4 affine colour matrices (row-major in the 12 channels), identity
at the start. A pixel of colour ``rgb`` at image position ``(x, y)`` in ``[0, 1]^2`` samples its image's grid trilinearly at
``(x (Wg - 1), y (Hg - 1), gray (L - 1))`` with ``gray = 0.299 r + 0.587 g + 0.114 b`` of its own colour - ``F.grid_sample`` with
``align_corners=True`` and ``padding_mode="border"``, so each index is clamped to its axis and a clamped index passes no
gradient - and leaves ``A[:, :3] @ rgb + A[:, 3]``.

float32 tensors on the GPU take the kernels of csrc/bilagrid.hip (gsx_bilagrid_slice_fwd / _bwd): one pass over the image per
direction, ``rgb`` read through its strides, the ``[..., 3, 4]`` matrices never materialised unless asked for, and the gradient
of the grid summed in LDS before it reaches memory when the coordinates are the pixel centres (`slice_image`). CPU tensors,
other dtypes and an ``xy`` that requires grad take the same composition in torch (`slice_torch`). The fused backward is not
itself differentiable (as with `photometric_loss`): a second derivative through the fused path raises, and a caller who needs
one calls `slice_torch`.

One deliberate difference from the reference's ``slice``: ``"rgb_affine_mats"`` is in the returned dict only with
``affine_mats=True`` - the trainer reads ``"rgb"`` alone, and the matrices of a 1080p image are 100 MB.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .losses import total_variation_loss

__all__ = ["BilateralGrid", "slice", "slice_image", "slice_torch", "color_affine_transform", "total_variation_loss"]


def color_affine_transform(affine_mats: Tensor, rgb: Tensor) -> Tensor:
    """``A[..., :3] @ rgb + A[..., 3]`` for matrices ``[..., 3, 4]`` and colours ``[..., 3]``."""
    return (affine_mats[..., :3] * rgb.unsqueeze(-2)).sum(-1) + affine_mats[..., 3]


class BilateralGrid(nn.Module):
    """``num`` bilateral grids ``[num, 12, grid_W, grid_Y, grid_X]`` (guidance, height, width), identity in every cell.
    Attribute, parameter and buffer names are the reference's, so a ``state_dict`` moves between the two in either direction."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        self.grid_width = grid_X
        self.grid_height = grid_Y
        self.grid_guidance = grid_W
        identity = torch.eye(3, 4, dtype=torch.float32).reshape(1, 12, 1, 1, 1)
        self.grids = nn.Parameter(identity.repeat(num, 1, grid_W, grid_Y, grid_X))
        self.register_buffer("rgb2gray_weight", torch.tensor([[0.299, 0.587, 0.114]], dtype=torch.float32))

    def rgb2gray(self, rgb: Tensor) -> Tensor:
        """Guidance in ``[-1, 1]`` of colours ``[..., 3]``, as ``[..., 1]``."""
        return (rgb @ self.rgb2gray_weight.T) * 2.0 - 1.0

    def tv_loss(self) -> Tensor:
        """Total variation of the grids (the trainer adds it with weight 10)."""
        return total_variation_loss(self.grids)

    def forward(self, grid_xy: Tensor, rgb: Tensor, idx=None) -> Tensor:
        """The sliced matrices ``[..., 3, 4]`` for coordinates ``grid_xy [..., 2]`` in ``[0, 1]`` and colours ``rgb [..., 3]``
        of 2 to 5 dimensions; the first dimension runs over the grids selected by ``idx`` (all of them, in order, for 5-D input
        without ``idx``). Evaluated in torch; `slice` / `slice_image` are the fused route to the colours."""
        nd = grid_xy.dim()
        if rgb.dim() != nd:
            raise ValueError(f"BilateralGrid: grid_xy has {nd} dimensions, rgb has {rgb.dim()}")
        if not 2 <= nd <= 5:
            raise ValueError("Bilateral grid slicing only takes either 2D, 3D, 4D and 5D inputs")
        if nd < 5 and idx is None:
            raise ValueError("BilateralGrid: idx is required for 2-D to 4-D input")
        for _ in range(5 - nd):
            grid_xy, rgb = grid_xy.unsqueeze(1), rgb.unsqueeze(1)
        grids = self.grids if idx is None else self.grids[idx]
        if grids.shape[0] != grid_xy.shape[0]:
            raise ValueError(f"BilateralGrid: {grids.shape[0]} grids selected for {grid_xy.shape[0]} leading entries")
        coords = torch.cat([(grid_xy - 0.5) * 2.0, self.rgb2gray(rgb)], dim=-1)  # [N, m, h, w, 3] in [-1, 1]
        mats = F.grid_sample(grids, coords, mode="bilinear", align_corners=True, padding_mode="border")  # [N, 12, m, h, w]
        mats = mats.permute(0, 2, 3, 4, 1)
        mats = mats.reshape(*mats.shape[:-1], 3, 4)
        for _ in range(5 - nd):
            mats = mats.squeeze(1)
        return mats


def _leading_index(grid_idx: Tensor, lead: int) -> Tensor:
    """The grid of each leading entry, ``[lead]`` int64: ``grid_idx`` is ``[lead, ..., 1]`` (the reference reads its first
    element per leading entry), ``[lead]``, or a single index for all."""
    if grid_idx.numel() == 1:
        return grid_idx.reshape(1).expand(lead).to(torch.int64)
    if grid_idx.shape[0] != lead:
        raise ValueError(f"bilagrid: grid_idx has {grid_idx.shape[0]} leading entries, the input has {lead}")
    return grid_idx.reshape(lead, -1)[:, 0].to(torch.int64)


def _check_inputs(bil_grids, xy, rgb, who: str) -> None:
    if rgb.dim() < 2 or rgb.dim() > 4 or rgb.shape[-1] != 3:
        raise ValueError(f"{who}: rgb must be [..., 3] with 2 to 4 dimensions, got {tuple(rgb.shape)}")
    if xy is not None and (xy.dim() != rgb.dim() or xy.shape[-1] != 2 or xy.shape[:-1] != rgb.shape[:-1]):
        raise ValueError(f"{who}: xy {tuple(xy.shape)} does not match rgb {tuple(rgb.shape)} (expected [..., 2] of the same "
                         "leading shape)")
    g = bil_grids.grids
    if g.dim() != 5 or g.shape[1] != 12:
        raise ValueError(f"{who}: grids must be [N, 12, L, Hg, Wg], got {tuple(g.shape)}")


def slice_torch(bil_grids: BilateralGrid, xy: Tensor, rgb: Tensor, grid_idx: Tensor, affine_mats: bool = False) -> dict:
    """`slice` composed of torch calls (any device and dtype, differentiable in everything, twice if need be)."""
    _check_inputs(bil_grids, xy, rgb, "slice")
    idx = _leading_index(grid_idx, rgb.shape[0])
    if not idx.is_cuda and idx.numel() > 1 and bool((idx == idx[0]).all()):
        # one grid for everything (host tensors: the comparison costs no device read): slice it once instead of gathering a
        # copy of it per leading entry
        mats = bil_grids(xy.unsqueeze(0), rgb.unsqueeze(0), idx[:1]).squeeze(0)
    else:
        mats = bil_grids(xy, rgb, idx)
    out = {"rgb": color_affine_transform(mats, rgb)}
    if affine_mats:
        out["rgb_affine_mats"] = mats
    return out


def _as_image(t: Tensor) -> Tensor:
    """[B, c] -> [B, 1, 1, c], [B, P, c] -> [B, 1, P, c]: a view, whatever the strides."""
    while t.dim() < 4:
        t = t.unsqueeze(1)
    return t


class _FusedSlice(torch.autograd.Function):
    """csrc/bilagrid.hip: rgb_out (and the matrices on request) in one pass; the backward writes v_rgb and adds v_grids."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, grids: Tensor, rgb: Tensor, xy, idx: Tensor, want_mats: bool):
        import ctypes

        from . import _cabi

        I, H, W, _ = rgb.shape
        N, _, L, Hg, Wg = grids.shape
        grids_c = grids.contiguous()
        rgb_out = torch.empty((I, H, W, 3), device=rgb.device, dtype=torch.float32)
        mats = torch.empty((I, H, W, 12), device=rgb.device, dtype=torch.float32) if want_mats else None
        sr = (ctypes.c_int64 * 4)(*rgb.stride())
        sx = (ctypes.c_int64 * 4)(*xy.stride()) if xy is not None else None
        _cabi.call("gsx_bilagrid_slice_fwd", grids_c, N, L, Hg, Wg, _cabi.strided(rgb), sr,
                   _cabi.strided(xy) if xy is not None else None, sx, idx, I, H, W, rgb_out, mats)
        _FusedSlice.calls += 1
        ctx.save_for_backward(grids_c, rgb, xy, idx)
        if mats is None:
            return rgb_out, None
        ctx.mark_non_differentiable(mats)  # a by-product for inspection; gradients flow through "rgb"
        return rgb_out, mats.view(I, H, W, 3, 4)

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_out, _v_mats):
        import ctypes

        from . import _cabi

        grids, rgb, xy, idx = ctx.saved_tensors
        if v_out is None:
            return None, None, None, None, None
        I, H, W, _ = rgb.shape
        N, _, L, Hg, Wg = grids.shape
        v_out = v_out.to(torch.float32)
        # a gradient nobody asked for (frozen grids, a constant image) is neither allocated nor computed. v_grids is dense over
        # all N grids, as autograd wants it for the parameter, although one step touches the I grids of its images only
        v_rgb = torch.empty((I, H, W, 3), device=rgb.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        v_grids = torch.zeros_like(grids) if ctx.needs_input_grad[0] else None
        if v_rgb is None and v_grids is None:
            return None, None, None, None, None
        sr, sv = (ctypes.c_int64 * 4)(*rgb.stride()), (ctypes.c_int64 * 4)(*v_out.stride())
        sx = (ctypes.c_int64 * 4)(*xy.stride()) if xy is not None else None
        _cabi.call("gsx_bilagrid_slice_bwd", grids, N, L, Hg, Wg, _cabi.strided(rgb), sr,
                   _cabi.strided(xy) if xy is not None else None, sx, idx, I, H, W, _cabi.strided(v_out), sv, v_rgb, v_grids)
        return v_grids, v_rgb, None, None, None


def _fused_ok(grids: Tensor, rgb: Tensor, xy, idx: Tensor) -> bool:
    return (grids.is_cuda and rgb.is_cuda and idx.device == rgb.device and grids.device == rgb.device
            and grids.dtype == torch.float32 and rgb.dtype == torch.float32 and rgb.numel() > 0
            and grids.numel() < 2 ** 31 and rgb.numel() // 3 < 2 ** 31 and max(rgb.shape[:-1]) < 2 ** 22
            and (xy is None or (xy.device == rgb.device and xy.dtype == torch.float32 and not xy.requires_grad)))


def _check_index(idx: Tensor, n: int, who: str) -> None:
    lo, hi = int(idx.min()), int(idx.max())  # reads the device: only on request
    if lo < 0 or hi >= n:
        raise IndexError(f"{who}: grid index {lo if lo < 0 else hi} is out of range for {n} grids")


def slice(bil_grids: BilateralGrid, xy: Tensor, rgb: Tensor, grid_idx: Tensor, affine_mats: bool = False,  # noqa: A001
          check_index: bool = False) -> dict:
    """Slices the bilateral grids at coordinates ``xy [..., 2]`` in ``[0, 1]`` with the guidance of colours ``rgb [..., 3]`` and
    applies the sliced matrices to ``rgb``. Inputs have 2 to 4 dimensions; the first runs over images, and image ``b`` uses grid
    ``grid_idx[b, ..., 0]`` (``grid_idx [..., 1]`` as in the reference, whose result this is also when all indices are equal).

    Returns ``{"rgb": [..., 3]}``, plus ``"rgb_affine_mats": [..., 3, 4]`` with ``affine_mats=True`` (detached on the fused
    path). ``check_index=True`` verifies the indices on the host (a device read) and raises ``IndexError``; without it an index
    outside the grids gives NaN colours on the fused path and torch's own error elsewhere."""
    if xy is None:
        raise ValueError("slice: xy is required; slice_image() is the call for whole images at their pixel centres")
    _check_inputs(bil_grids, xy, rgb, "slice")
    idx = _leading_index(grid_idx, rgb.shape[0])
    if check_index and idx.numel():
        _check_index(idx, bil_grids.grids.shape[0], "slice")
    if not _fused_ok(bil_grids.grids, rgb, xy, idx):
        return slice_torch(bil_grids, xy, rgb, idx, affine_mats)
    out, mats = _FusedSlice.apply(bil_grids.grids, _as_image(rgb), _as_image(xy), idx.contiguous(), bool(affine_mats))
    res = {"rgb": out.reshape(rgb.shape)}
    if affine_mats:
        res["rgb_affine_mats"] = mats.reshape(*rgb.shape[:-1], 3, 4)
    return res


def pixel_center_xy(I: int, H: int, W: int, device=None, dtype=torch.float32) -> Tensor:
    """``[I, H, W, 2]`` pixel-centre coordinates ``((x + 0.5) / W, (y + 0.5) / H)``: what `slice_image` uses implicitly."""
    # divided by a tensor, not a Python number: on the GPU torch turns division by a host scalar into a multiplication by its
    # reciprocal, which is an ulp off the correctly rounded quotient that the CPU and the kernels compute
    ys = (torch.arange(H, device=device, dtype=dtype) + 0.5) / torch.full((), H, device=device, dtype=dtype)
    xs = (torch.arange(W, device=device, dtype=dtype) + 0.5) / torch.full((), W, device=device, dtype=dtype)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([gx, gy], dim=-1).unsqueeze(0).expand(I, H, W, 2)


def slice_image(bil_grids: BilateralGrid, rgb: Tensor, grid_idx: Tensor, affine_mats: bool = False,
                check_index: bool = False) -> dict:
    """The trainer's case: whole images ``rgb [I, H, W, 3]`` (a ``[..., :3]`` view of a wider render is read in place), image
    ``i`` corrected by grid ``grid_idx[i]`` at its pixel centres. No ``xy`` tensor is built or read and nothing is read back
    from the device; the backward sums the grid's gradient on chip. Returns the dict of `slice`."""
    if rgb.dim() != 4:
        raise ValueError(f"slice_image: rgb must be [I, H, W, 3], got {tuple(rgb.shape)}")
    _check_inputs(bil_grids, None, rgb, "slice_image")
    I, H, W, _ = rgb.shape
    idx = _leading_index(grid_idx, I)
    if check_index and idx.numel():
        _check_index(idx, bil_grids.grids.shape[0], "slice_image")
    if not _fused_ok(bil_grids.grids, rgb, None, idx):
        return slice_torch(bil_grids, pixel_center_xy(I, H, W, rgb.device, rgb.dtype), rgb, idx, affine_mats)
    out, mats = _FusedSlice.apply(bil_grids.grids, rgb, None, idx.contiguous(), bool(affine_mats))
    res = {"rgb": out}
    if affine_mats:
        res["rgb_affine_mats"] = mats
    return res
