"""Image losses of the training step around the rasterizer.

`ssim_loss` mirrors ``gsplat/losses.py:150-200`` (``1 - SSIM`` with an 11 x 11 Gaussian window of sigma 1.5, zero padding,
constants C1 = 0.01^2 / C2 = 0.03^2, mean over batch, channels and pixels - the term the reference trainer blends with L1,
``examples/simple_trainer.py:951-961``: ``loss = lerp(l1, ssim_loss, 0.2)``). The reference evaluates five depthwise 11 x 11
convolutions (or the third-party ``fused_ssim`` CUDA extension, not available here); the window is an outer product, so this
version runs the five maps as ONE stacked tensor through a vertical and a horizontal 11-tap pass - the same sums, 22 taps per
output instead of 121. Plain torch ops: differentiable through autograd, runs on any device.

`photometric_loss` is that whole blend with an optional mask (``masked_l1`` / ``masked_ssim``, gsplat/losses.py:328-399): one
fused kernel pair on the GPU, the torch composition elsewhere.

`depth_l1_loss`, `binocular_disparity_l1`, `pearson_depth_loss` (gsplat/losses.py:209-320) and `sampled_depth_l1_loss` (the
trainers' ``depth_loss=True`` block, examples/simple_trainer.py:962-980) are the depth supervision: csrc/depth_loss.hip on the
GPU, the ``*_torch`` compositions elsewhere, neither with a host read. One departure from the reference, in both: where a
(sampled) predicted depth is ``<= 0`` the gradient of the disparity ``where(d > 0, 1 / d, 0)`` is 0, not NaN.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor

_WINDOW_CACHE: dict = {}


def _window_1d(window_size: int, sigma: float, device, dtype) -> Tensor:
    key = (window_size, sigma, str(device), dtype)
    w = _WINDOW_CACHE.get(key)
    if w is None:
        x = torch.arange(window_size, device=device, dtype=torch.float32)
        g = torch.exp(-((x - window_size // 2) ** 2) / (2 * sigma ** 2))
        w = (g / g.sum()).to(dtype)
        _WINDOW_CACHE[key] = w
    return w


def ssim_map(img1: Tensor, img2: Tensor, window_size: int = 11) -> Tensor:
    """SSIM map [B, C, H, W] of two image batches [B, C, H, W] in [0, 1] (gsplat/losses.py: torch_ssim_loss)."""
    if img1.shape != img2.shape or img1.dim() != 4:
        raise ValueError(f"ssim: expected two [B, C, H, W] batches of one shape, got {tuple(img1.shape)} / {tuple(img2.shape)}")
    B, C, H, W = img1.shape
    w = _window_1d(window_size, 1.5, img1.device, img1.dtype)
    pad = window_size // 2
    maps = torch.cat([img1, img2, img1 * img1, img2 * img2, img1 * img2], dim=1)  # [B, 5 C, H, W]
    G = 5 * C
    maps = F.conv2d(maps, w.view(1, 1, window_size, 1).expand(G, 1, window_size, 1), padding=(pad, 0), groups=G)
    maps = F.conv2d(maps, w.view(1, 1, 1, window_size).expand(G, 1, 1, window_size), padding=(0, pad), groups=G)
    mu1, mu2, s11, s22, s12 = maps.split(C, dim=1)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = s11 - mu1_sq, s22 - mu2_sq, s12 - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


class _FusedSsimMean(torch.autograd.Function):
    """mean(SSIM map) on the MI355X: csrc/ssim.hip (gsx_ssim_fwd / gsx_ssim_bwd), one kernel per direction, images read
    through their strides (a [B, H, W, C] render permuted to [B, C, H, W] is consumed in place). Differentiable in img1."""

    @staticmethod
    def forward(ctx, img1: Tensor, img2: Tensor):
        import ctypes

        from . import _cabi

        B, C, H, W = img1.shape
        img2 = img2.detach()
        dev = img1.device
        partial = torch.empty(_cabi.query("gsx_ssim_blocks", B, C, H, W), device=dev, dtype=torch.float32)
        need_grad = ctx.needs_input_grad[0]
        dmaps = torch.empty((B, C, H, W, 3), device=dev, dtype=torch.float32) if need_grad else None
        s1, s2 = (ctypes.c_int64 * 4)(*img1.stride()), (ctypes.c_int64 * 4)(*img2.stride())
        _cabi.call("gsx_ssim_fwd", _cabi.strided(img1), s1, _cabi.strided(img2), s2, B, C, H, W, partial, dmaps)
        ctx.save_for_backward(img1, img2, dmaps)
        return partial.sum() / float(B * C * H * W)

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_mean: Tensor):
        import ctypes

        from . import _cabi

        img1, img2, dmaps = ctx.saved_tensors
        if dmaps is None:  # forward ran without a gradient request for img1
            return None, None
        B, C, H, W = img1.shape
        v_img1 = torch.empty_like(img1)  # preserve_format: a dense permuted view (channels-last render) keeps its strides
        s1, s2, sv = ((ctypes.c_int64 * 4)(*t.stride()) for t in (img1, img2, v_img1))
        v_mean = v_mean.reshape(1).to(torch.float32).contiguous()  # stays on the device: the kernel multiplies by it
        _cabi.call("gsx_ssim_bwd", _cabi.strided(img1), s1, _cabi.strided(img2), s2, B, C, H, W, dmaps,
                   1.0 / float(B * C * H * W), v_mean, _cabi.strided(v_img1), sv)
        return v_img1, None


def ssim_loss(img1: Tensor, img2: Tensor, window_size: int = 11) -> Tensor:
    """``1 - mean(SSIM)`` (gsplat/losses.py:150-200). float32 images on the GPU with the default window take the fused
    kernels (what the reference gets from the third-party ``fused_ssim`` extension); anything else the torch evaluation.
    Zero ("same") padding like gsplat/losses.py's torch path; the reference's optional fused_ssim fast path defaults to
    padding="valid" and is a different loss value - not offered here."""
    if (img1.is_cuda and img2.is_cuda and window_size == 11 and img1.dtype == torch.float32 and img2.dtype == torch.float32
            and img1.dim() == 4 and img1.shape == img2.shape and not img2.requires_grad
            and img1.shape[0] * img1.shape[1] <= 65535):  # the kernels' grid: one z-slice per (batch, channel) plane
        return 1.0 - _FusedSsimMean.apply(img1, img2)
    return 1.0 - ssim_map(img1, img2, window_size).mean()


def l1_loss(pred: Tensor, target: Tensor) -> Tensor:
    """Per-element L1 (gsplat/losses.py:48-63)."""
    return (pred - target).abs()


def mse_loss(pred: Tensor, target: Tensor) -> Tensor:
    """Per-element squared error (gsplat/losses.py:66-76)."""
    return F.mse_loss(pred, target, reduction="none")


def masked_l1(pred: Tensor, gt: Tensor, mask: Tensor) -> Tensor:
    """Mean of ``|pred - gt|`` over the elements with ``mask != 0``; a differentiable 0 when nothing is selected
    (gsplat/losses.py:328-357). The reference gathers the selected elements by boolean indexing, which reads their number
    back from the device; here the selection is a ``where`` and two sums, so a training step on the GPU stays free of host
    reads. ``mask`` broadcasts to ``pred`` (a ``[B, 1, H, W]`` mask on ``[B, C, H, W]`` images)."""
    if pred.shape != gt.shape:
        raise ValueError(f"masked_l1: pred shape {pred.shape} != gt shape {gt.shape}. Shapes must match.")
    abs_diff = (pred - gt).abs()
    selected = (mask != 0).expand_as(abs_diff)
    count = selected.sum().clamp(min=1).to(abs_diff.dtype)  # nothing selected: 0 / 1
    return torch.where(selected, abs_diff, torch.zeros((), dtype=abs_diff.dtype, device=abs_diff.device)).sum() / count


def masked_ssim(pred: Tensor, gt: Tensor, mask: Tensor) -> Tensor:
    """``ssim_loss(pred * mask, gt * mask)`` (gsplat/losses.py:360-399): both images are zeroed where the mask is, and the
    mean still runs over the whole image, so the value scales with the mask's coverage - the reference's convention."""
    if pred.shape != gt.shape:
        raise ValueError(f"masked_ssim: pred shape {pred.shape} != gt shape {gt.shape}. Shapes must match.")
    return ssim_loss(pred * mask, gt * mask)


class _FusedPhotometric(torch.autograd.Function):
    """lerp(l1, ssim_loss, ssim_lambda) with an optional mask on the MI355X: csrc/ssim.hip (gsx_photometric_fwd / _bwd). One
    kernel per direction reads pred, target and the mask through their strides, a one-workgroup reduction leaves
    (loss, l1, ssim_loss, count) in device memory, and the backward writes the whole gradient of pred. Differentiable in pred."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, pred: Tensor, target: Tensor, mask, ssim_lambda: float):
        import ctypes

        from . import _cabi

        B, C, H, W = pred.shape
        target = target.detach()
        dev = pred.device
        if mask is not None:
            mask = mask.detach()
            if mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)
            elif mask.dtype not in (torch.uint8, torch.float32):
                mask = mask.to(torch.float32)
            mask = mask.expand(B, C, H, W)  # stride 0 along the broadcast dimensions: read in place
        tag = 1 if mask is not None and mask.dtype == torch.uint8 else 0  # GSX_MASK_U8 / GSX_MASK_F32
        partial = torch.empty(3 * _cabi.query("gsx_photometric_blocks", B, C, H, W), device=dev, dtype=torch.float32)
        record = torch.empty(4, device=dev, dtype=torch.float32)
        need_grad = ctx.needs_input_grad[0]
        dmaps = torch.empty((B, C, H, W, 3), device=dev, dtype=torch.float32) if need_grad else None
        sp, st = (ctypes.c_int64 * 4)(*pred.stride()), (ctypes.c_int64 * 4)(*target.stride())
        sm = (ctypes.c_int64 * 4)(*mask.stride()) if mask is not None else None
        _cabi.call("gsx_photometric_fwd", _cabi.strided(pred), sp, _cabi.strided(target), st,
                   _cabi.strided(mask) if mask is not None else None, sm, tag, B, C, H, W, float(ssim_lambda),
                   partial, dmaps, record)
        _FusedPhotometric.calls += 1
        ctx.save_for_backward(pred, target, mask, dmaps, record)
        ctx.ssim_lambda, ctx.mask_tag = float(ssim_lambda), tag
        ctx.set_materialize_grads(False)
        loss, l1, ssim = record[0], record[1], record[2]
        ctx.mark_non_differentiable(l1, ssim)
        return loss, l1, ssim

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_loss, _v_l1, _v_ssim):
        import ctypes

        from . import _cabi

        pred, target, mask, dmaps, record = ctx.saved_tensors
        if dmaps is None or v_loss is None:  # forward ran without a gradient request for pred / the loss was not used
            return None, None, None, None
        B, C, H, W = pred.shape
        v_pred = torch.empty_like(pred)  # preserve_format: a dense permuted view (channels-last render) keeps its strides
        sp, st, sv = ((ctypes.c_int64 * 4)(*t.stride()) for t in (pred, target, v_pred))
        sm = (ctypes.c_int64 * 4)(*mask.stride()) if mask is not None else None
        v_loss = v_loss.reshape(1).to(torch.float32).contiguous()  # stays on the device: the kernel multiplies by it
        _cabi.call("gsx_photometric_bwd", _cabi.strided(pred), sp, _cabi.strided(target), st,
                   _cabi.strided(mask) if mask is not None else None, sm, ctx.mask_tag, B, C, H, W, ctx.ssim_lambda,
                   dmaps, record, v_loss, _cabi.strided(v_pred), sv)
        return v_pred, None, None, None


def photometric_loss(pred: Tensor, target: Tensor, ssim_lambda: float = 0.2, mask=None, window_size: int = 11,
                     return_parts: bool = False):
    """The trainer's photometric loss ``lerp(l1, ssim_loss, ssim_lambda)`` (examples/simple_trainer.py:946-961) of two
    ``[B, C, H, W]`` batches, with an optional ``mask`` broadcastable to them (``[B, 1, H, W]`` or ``[B, C, H, W]``; float,
    bool or uint8): ``l1 = masked_l1(pred, target, mask)`` selects by ``mask != 0``, ``ssim_loss = masked_ssim(pred, target,
    mask)`` multiplies by the mask's value (gsplat/losses.py:328-399). Without a mask: ``l1_loss(pred, target).mean()`` and
    ``ssim_loss(pred, target)``.

    float32 images on the GPU with the default window take the fused kernels - each image read once per direction, no host
    read, one gradient image for autograd; anything else (CPU tensors, other dtypes or windows, a ``target`` that requires
    grad, more than 65535 planes) the same composition in torch. Returns the scalar loss, or with ``return_parts`` the tuple
    ``(loss, l1, ssim_loss)`` whose last two are detached device scalars for logging."""
    if pred.shape != target.shape:
        raise ValueError(f"photometric_loss: pred shape {pred.shape} != target shape {target.shape}. Shapes must match.")
    if pred.dim() != 4:
        raise ValueError(f"photometric_loss: expected [B, C, H, W] batches, got {tuple(pred.shape)}")
    if not 0.0 <= float(ssim_lambda) <= 1.0:
        raise ValueError(f"photometric_loss: ssim_lambda {ssim_lambda} outside [0, 1]")
    if mask is not None:
        if mask.dim() != 4 or any(m != p and m != 1 for m, p in zip(mask.shape, pred.shape)):
            raise ValueError(f"photometric_loss: mask shape {tuple(mask.shape)} does not broadcast to {tuple(pred.shape)}")
    if (pred.is_cuda and target.is_cuda and window_size == 11 and pred.dtype == torch.float32 and target.dtype == torch.float32
            and not target.requires_grad and 0 < pred.shape[0] * pred.shape[1] <= 65535 and pred.numel() > 0
            and (mask is None or (mask.device == pred.device and not mask.requires_grad))):
        loss, l1, ssim = _FusedPhotometric.apply(pred, target, mask, float(ssim_lambda))
    else:
        if mask is None:
            l1, ssim = l1_loss(pred, target).mean(), ssim_loss(pred, target, window_size)
        else:
            l1, ssim = masked_l1(pred, target, mask), ssim_loss(pred * mask, target * mask, window_size)  # = masked_ssim
        loss = torch.lerp(l1, ssim, float(ssim_lambda))
        l1, ssim = l1.detach(), ssim.detach()
    return (loss, l1, ssim) if return_parts else loss


def total_variation_torch(x: Tensor) -> Tensor:
    """`total_variation_loss` composed of torch calls (any device, dtype and number of spatial axes)."""
    if x.dim() < 3:
        raise ValueError(f"total_variation_loss: expected [B, C, d1, ...], got {tuple(x.shape)}")
    tv = x.new_zeros(())
    for axis in range(2, x.dim()):
        n = x.shape[axis] - 1
        if n <= 0:  # nothing to difference along this axis
            continue
        d = x.narrow(axis, 1, n) - x.narrow(axis, 0, n)
        tv = tv + d.pow(2).sum() / max(float(d.numel() // max(d.shape[0], 1)), 1.0)
    return tv / x.shape[0]


class _FusedTotalVariation(torch.autograd.Function):
    """Total variation of a [B, C, D1, D2, D3] tensor on the MI355X: csrc/bilagrid.hip (gsx_tv_fwd / gsx_tv_bwd). Per-workgroup
    sums added by one workgroup in a fixed order; the value stays in device memory and the backward reads its incoming
    gradient there."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, x: Tensor):
        from . import _cabi

        xc = x.contiguous()
        partial = torch.empty(_cabi.query("gsx_tv_blocks", *xc.shape), device=x.device, dtype=torch.float32)
        out = torch.empty(1, device=x.device, dtype=torch.float32)
        _cabi.call("gsx_tv_fwd", xc, *xc.shape, partial, out)
        _FusedTotalVariation.calls += 1
        ctx.save_for_backward(xc)
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_loss: Tensor):
        from . import _cabi

        (xc,) = ctx.saved_tensors
        v_x = torch.empty_like(xc)
        v_loss = v_loss.reshape(1).to(torch.float32).contiguous()  # stays on the device: the kernel multiplies by it
        _cabi.call("gsx_tv_bwd", xc, *xc.shape, v_loss, v_x)
        return v_x


def total_variation_loss(x: Tensor) -> Tensor:
    """Total variation of ``x [B, C, d1, ...]`` (gsplat/losses.py:642-667; the regulariser of the bilateral grids,
    examples/simple_trainer.py:981-984): for every spatial axis the sum of squared forward differences divided by the element
    count of the differenced tensor without its batch axis (at least 1), summed over the axes, divided by ``B``.

    A float32 5-D tensor on the GPU (a stack of bilateral grids ``[N, 12, L, Hg, Wg]``) takes the fused kernels: one pass and a
    one-workgroup reduction forward, one pass backward, no host read. Anything else the same sums in torch."""
    if x.dim() < 3:
        raise ValueError(f"total_variation_loss: expected [B, C, d1, ...], got {tuple(x.shape)}")
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and 0 < x.numel() < 2 ** 31:
        return _FusedTotalVariation.apply(x)
    return total_variation_torch(x)


# ---- depth supervision -----------------------------------------------------------------------------------------------------

def _disparity(depth: Tensor) -> Tensor:
    """``where(depth > 0, 1 / depth, 0)`` whose gradient is 0 where ``depth <= 0`` (the reference's is inf * 0 = NaN there)."""
    positive = depth > 0.0
    return torch.where(positive, 1.0 / torch.where(positive, depth, torch.ones_like(depth)), torch.zeros_like(depth))


def depth_l1_loss_torch(pred_depth: Tensor, gt_depth: Tensor, scene_scale: float = 1.0) -> Tensor:
    """`depth_l1_loss` composed of torch calls (any device and dtype)."""
    return (_disparity(pred_depth) - _disparity(gt_depth)).abs().mean() * scene_scale


def binocular_disparity_l1_torch(pred_depth: Tensor, gt_depth: Tensor, mask=None, eps: float = 1e-7) -> Tensor:
    """`binocular_disparity_l1` composed of torch calls: the selection is a ``where`` and two sums (`masked_l1`), no boolean
    indexing and no host read."""
    if pred_depth.shape != gt_depth.shape:
        raise ValueError(f"binocular_disparity_l1: pred_depth shape {pred_depth.shape} != gt_depth shape {gt_depth.shape}. "
                         "Shapes must match.")
    valid_pred, valid_gt = pred_depth.abs() > eps, gt_depth.abs() > eps
    ones = torch.ones_like(pred_depth)
    pred_inv, gt_inv = 1.0 / torch.where(valid_pred, pred_depth, ones), 1.0 / torch.where(valid_gt, gt_depth, ones)
    selected = valid_pred & valid_gt
    if mask is not None:
        selected = selected & (mask != 0)
    return masked_l1(pred_inv, gt_inv, selected)


def pearson_depth_loss_torch(pred_depth: Tensor, gt_depth: Tensor, mask=None) -> Tensor:
    """`pearson_depth_loss` composed of torch calls: centred sums over a ``where``, the count stays on the device."""
    if pred_depth.shape != gt_depth.shape:
        raise ValueError(f"pearson_depth_loss: pred_depth shape {pred_depth.shape} != gt_depth shape {gt_depth.shape}. "
                         "Shapes must match.")
    zero = torch.zeros((), dtype=pred_depth.dtype, device=pred_depth.device)
    if mask is None:
        selected = torch.ones_like(pred_depth, dtype=torch.bool)
    else:
        selected = (mask != 0).expand_as(pred_depth)
    count = selected.sum()
    n = count.clamp(min=1).to(pred_depth.dtype)
    pred_centered = torch.where(selected, pred_depth - torch.where(selected, pred_depth, zero).sum() / n, zero)
    gt_centered = torch.where(selected, gt_depth - torch.where(selected, gt_depth, zero).sum() / n, zero)
    num = (pred_centered * gt_centered).sum()
    denom = (pred_centered.pow(2).sum() * gt_centered.pow(2).sum()).clamp(min=1e-12).sqrt()
    return torch.where(count >= 2, 1.0 - num / denom, zero)


def _depth_map_3d(depth_map: Tensor, points: Tensor, depths_gt: Tensor) -> Tensor:
    if depth_map.dim() == 4 and depth_map.shape[-1] == 1:
        depth_map = depth_map[..., 0]
    if depth_map.dim() != 3:
        raise ValueError(f"sampled_depth_l1_loss: expected a [C, H, W, 1] or [C, H, W] depth map, got {tuple(depth_map.shape)}")
    C = depth_map.shape[0]
    if points.dim() != 3 or points.shape[0] != C or points.shape[2] != 2:
        raise ValueError(f"sampled_depth_l1_loss: expected points [{C}, M, 2], got {tuple(points.shape)}")
    if depths_gt.shape != points.shape[:2]:
        raise ValueError(f"sampled_depth_l1_loss: depths_gt shape {tuple(depths_gt.shape)} != points' {tuple(points.shape[:2])}")
    return depth_map


def _sample_depth_torch(depth_map: Tensor, points: Tensor) -> Tensor:
    """Bilinear samples ``[C, M]`` of ``depth_map [C, H, W]`` at pixel coordinates ``points [C, M, 2] = (x, y)``: what
    ``F.grid_sample(..., align_corners=True)`` returns for the coordinates normalised by ``(W - 1, H - 1)``, zeros outside."""
    C, H, W = depth_map.shape
    if H * W == 0 or points.shape[1] == 0:
        return depth_map.new_zeros(points.shape[:2]) + 0.0 * points.sum(-1).to(depth_map.dtype)
    points = torch.where(torch.isfinite(points), points, torch.full_like(points, -2.0)).to(depth_map.dtype)
    x, y = points[..., 0], points[..., 1]
    x0, y0 = x.detach().floor(), y.detach().floor()
    flat = depth_map.reshape(C, H * W)
    out = depth_map.new_zeros(points.shape[:2])
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            w = ((x - x0) if dx else (1.0 - (x - x0))) * ((y - y0) if dy else (1.0 - (y - y0)))
            inside = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
            out = out + torch.where(inside, flat.gather(1, idx) * w, torch.zeros_like(w))
    return out


def sampled_depth_l1_loss_torch(depth_map: Tensor, points: Tensor, depths_gt: Tensor, scene_scale: float = 1.0) -> Tensor:
    """`sampled_depth_l1_loss` composed of torch calls (any device and dtype; differentiable in ``points`` as well)."""
    depth_map = _depth_map_3d(depth_map, points, depths_gt)
    return depth_l1_loss_torch(_sample_depth_torch(depth_map, points), depths_gt, scene_scale)


def _as_4d(t: Tensor) -> Tensor:
    """`t` as the [d0, d1, d2, d3] tensor the kernels address through strides: leading axes of size 1 added, or the leading
    axes of a longer shape merged (a view wherever the strides allow one)."""
    if t.dim() < 4:
        return t[(None,) * (4 - t.dim())]
    return t if t.dim() == 4 else t.flatten(0, t.dim() - 4)


def _mask_4d(mask, shape):
    """(mask as the kernels read it - uint8 or float32, broadcast to `shape` with stride 0 - , its GSX_MASK_* tag)."""
    if mask is None:
        return None, 0
    mask = mask.detach()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    elif mask.dtype not in (torch.uint8, torch.float32):
        mask = (mask != 0).view(torch.uint8)
    return _as_4d(mask.expand(shape)), 1 if mask.dtype == torch.uint8 else 0  # GSX_MASK_U8 / GSX_MASK_F32


def _dense_depth_args(pred4: Tensor, gt4: Tensor, mask4, tag: int):
    import ctypes

    from . import _cabi

    sp, sg = (ctypes.c_int64 * 4)(*pred4.stride()), (ctypes.c_int64 * 4)(*gt4.stride())
    sm = (ctypes.c_int64 * 4)(*mask4.stride()) if mask4 is not None else None
    return (_cabi.strided(pred4), sp, _cabi.strided(gt4), sg, _cabi.strided(mask4) if mask4 is not None else None, sm,
            tag, *pred4.shape)


def _depth_scratch(n: int, device):
    from . import _cabi

    partial = torch.empty(6 * _cabi.query("gsx_depth_blocks", n), device=device, dtype=torch.float64)  # GSX_DEPTH_PARTIALS
    return partial, torch.empty(1, device=device, dtype=torch.float32), torch.empty(8, device=device, dtype=torch.float64)


class _FusedPearsonDepth(torch.autograd.Function):
    """``1 - Pearson r`` over the elements with ``mask != 0`` on the MI355X: csrc/depth_loss.hip (gsx_depth_pearson_fwd / _bwd).
    One pass reads pred, gt and the mask through their strides, a one-workgroup finish leaves the loss and the record (count,
    means, Spp, Sgg, Spg, denominator) in device memory, and the backward is one elementwise pass. Differentiable in pred."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, pred: Tensor, gt: Tensor, mask):
        from . import _cabi

        pred4, gt4 = _as_4d(pred), _as_4d(gt.detach())
        mask4, tag = _mask_4d(mask, pred.shape)
        partial, loss, record = _depth_scratch(pred4.numel(), pred.device)
        _cabi.call("gsx_depth_pearson_fwd", *_dense_depth_args(pred4, gt4, mask4, tag), partial, loss, record)
        _FusedPearsonDepth.calls += 1
        ctx.save_for_backward(pred4, gt4, mask4, record)
        ctx.mask_tag, ctx.shape = tag, pred.shape
        ctx.set_materialize_grads(False)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_loss):
        from . import _cabi

        pred4, gt4, mask4, record = ctx.saved_tensors
        if v_loss is None or not ctx.needs_input_grad[0]:
            return None, None, None
        v_pred = torch.empty(pred4.shape, device=pred4.device, dtype=torch.float32)
        v_loss = v_loss.reshape(1).to(torch.float32).contiguous()  # stays on the device: the kernel multiplies by it
        _cabi.call("gsx_depth_pearson_bwd", *_dense_depth_args(pred4, gt4, mask4, ctx.mask_tag), record, v_loss, v_pred)
        return v_pred.view(ctx.shape), None, None


class _FusedDisparityL1(torch.autograd.Function):
    """`depth_l1_loss` (mode 0, GSX_DEPTH_L1) and `binocular_disparity_l1` (mode 1, GSX_DEPTH_BINOCULAR) on the MI355X:
    csrc/depth_loss.hip (gsx_depth_disparity_fwd / _bwd), one pass per direction; the record (loss, count, L1 sum, gradient
    scale) stays in device memory. Differentiable in pred; the gradient is 0 where a pair does not count or pred <= 0."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, pred: Tensor, gt: Tensor, mask, mode: int, scale: float, eps: float):
        from . import _cabi

        pred4, gt4 = _as_4d(pred), _as_4d(gt.detach())
        mask4, tag = _mask_4d(mask, pred.shape)
        partial, loss, record = _depth_scratch(pred4.numel(), pred.device)
        _cabi.call("gsx_depth_disparity_fwd", *_dense_depth_args(pred4, gt4, mask4, tag), mode, scale, eps, partial,
                   loss, record)
        _FusedDisparityL1.calls += 1
        ctx.save_for_backward(pred4, gt4, mask4, record)
        ctx.mask_tag, ctx.shape, ctx.mode, ctx.eps = tag, pred.shape, mode, eps
        ctx.set_materialize_grads(False)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_loss):
        from . import _cabi

        pred4, gt4, mask4, record = ctx.saved_tensors
        if v_loss is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        v_pred = torch.empty(pred4.shape, device=pred4.device, dtype=torch.float32)
        v_loss = v_loss.reshape(1).to(torch.float32).contiguous()  # stays on the device: the kernel multiplies by it
        _cabi.call("gsx_depth_disparity_bwd", *_dense_depth_args(pred4, gt4, mask4, ctx.mask_tag), ctx.mode, ctx.eps,
                   record, v_loss, v_pred)
        return v_pred.view(ctx.shape), None, None, None, None, None


class _FusedSampledDepthL1(torch.autograd.Function):
    """`sampled_depth_l1_loss` on the MI355X: csrc/depth_loss.hip (gsx_depth_sampled_fwd / _bwd). One thread per point takes
    its four taps through the map's strides; the backward zero-fills a dense [C, H, W] gradient and scatters the taps with
    float atomics (points may share a pixel). Differentiable in the depth map."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def _args(depth_map, points, depths_gt):
        import ctypes

        from . import _cabi

        C, H, W = depth_map.shape
        return (_cabi.strided(depth_map), (ctypes.c_int64 * 3)(*depth_map.stride()), C, H, W, points,
                depths_gt, points.shape[1])

    @staticmethod
    def forward(ctx, depth_map: Tensor, points: Tensor, depths_gt: Tensor, scale: float):
        from . import _cabi

        map3 = depth_map[..., 0] if depth_map.dim() == 4 else depth_map
        points, depths_gt = points.detach().contiguous(), depths_gt.detach().contiguous()
        partial, loss, record = _depth_scratch(depths_gt.numel(), map3.device)
        _cabi.call("gsx_depth_sampled_fwd", *_FusedSampledDepthL1._args(map3, points, depths_gt), scale, partial, loss, record)
        _FusedSampledDepthL1.calls += 1
        ctx.save_for_backward(map3, points, depths_gt, record)
        ctx.shape = depth_map.shape
        ctx.set_materialize_grads(False)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_loss):
        from . import _cabi

        map3, points, depths_gt, record = ctx.saved_tensors
        if v_loss is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        v_map = torch.empty(map3.shape, device=map3.device, dtype=torch.float32)  # zero-filled by the entry point
        v_loss = v_loss.reshape(1).to(torch.float32).contiguous()  # stays on the device: the kernel multiplies by it
        _cabi.call("gsx_depth_sampled_bwd", *_FusedSampledDepthL1._args(map3, points, depths_gt), record, v_loss, v_map)
        return v_map.view(ctx.shape), None, None, None


def _dense_depth_fused_ok(pred: Tensor, gt: Tensor, mask) -> bool:
    if not (pred.is_cuda and gt.device == pred.device and pred.dtype == torch.float32 and gt.dtype == torch.float32
            and pred.shape == gt.shape and not gt.requires_grad and 0 < pred.numel() < 2 ** 31):
        return False
    if mask is None:
        return True
    if mask.device != pred.device or mask.requires_grad or mask.dim() > pred.dim():
        return False
    return all(m == p or m == 1 for m, p in zip(mask.shape[::-1], pred.shape[::-1]))


def depth_l1_loss(pred_depth: Tensor, gt_depth: Tensor, scene_scale: float = 1.0) -> Tensor:
    """L1 loss in disparity space (gsplat/losses.py:209-224): ``scene_scale * mean |disp(pred) - disp(gt)|`` over all
    elements, with ``disp(x) = where(x > 0, 1 / x, 0)`` on each side independently.

    Departure from the reference: where ``pred_depth <= 0`` the gradient is 0. The reference's ``torch.where(d > 0, 1 / d, 0)``
    back-propagates ``inf * 0 = NaN`` at ``d == 0``, which an expected-depth render is at every uncovered pixel. The loss
    value is the reference's.

    float32 tensors of one shape on the GPU take the fused kernels (one pass per direction, strided views such as
    ``renders[..., 3:4]`` read in place); anything else - CPU tensors, other dtypes, a ``gt_depth`` that requires grad, empty
    inputs - `depth_l1_loss_torch`."""
    if _dense_depth_fused_ok(pred_depth, gt_depth, None):
        return _FusedDisparityL1.apply(pred_depth, gt_depth, None, 0, float(scene_scale), 0.0)
    return depth_l1_loss_torch(pred_depth, gt_depth, scene_scale)


def binocular_disparity_l1(pred_depth: Tensor, gt_depth: Tensor, mask=None, eps: float = 1e-7) -> Tensor:
    """L1 loss in inverse-depth space with optional masking (gsplat/losses.py:227-276): the mean of ``|1 / pred - 1 / gt|``
    over the pairs with ``|pred| > eps``, ``|gt| > eps`` and, with a ``mask`` (broadcastable to ``pred_depth``; bool, uint8 or
    float), ``mask != 0``. A differentiable 0 when no pair counts.

    The reference gathers the counted pairs by boolean indexing - a device-to-host read per step; neither path here reads
    anything back. float32 tensors on the GPU take the fused kernels, anything else `binocular_disparity_l1_torch`."""
    if pred_depth.shape != gt_depth.shape:
        raise ValueError(f"binocular_disparity_l1: pred_depth shape {pred_depth.shape} != gt_depth shape {gt_depth.shape}. "
                         "Shapes must match.")
    if _dense_depth_fused_ok(pred_depth, gt_depth, mask) and eps >= 0:
        return _FusedDisparityL1.apply(pred_depth, gt_depth, mask, 1, 1.0, float(eps))
    return binocular_disparity_l1_torch(pred_depth, gt_depth, mask, eps)


def pearson_depth_loss(pred_depth: Tensor, gt_depth: Tensor, mask=None) -> Tensor:
    """Monocular depth loss ``1 - Pearson r`` over the elements with ``mask != 0`` (gsplat/losses.py:279-320; all elements
    without a mask). 0 with zero gradient when fewer than two elements remain; the denominator is
    ``sqrt(clamp(Spp * Sgg, min=1e-12))``, and the clamp passes its gradient where the product is ``>= 1e-12`` and blocks it
    otherwise, as torch's does.

    The reference selects by boolean indexing and tests ``numel() < 2`` on the host; here both are decided on the device.
    float32 tensors on the GPU take the fused kernels (centred moments in double, merged pairwise: accurate at depths of 100 +- 0.05),
    anything else `pearson_depth_loss_torch`."""
    if pred_depth.shape != gt_depth.shape:
        raise ValueError(f"pearson_depth_loss: pred_depth shape {pred_depth.shape} != gt_depth shape {gt_depth.shape}. "
                         "Shapes must match.")
    if _dense_depth_fused_ok(pred_depth, gt_depth, mask):
        return _FusedPearsonDepth.apply(pred_depth, gt_depth, mask)
    return pearson_depth_loss_torch(pred_depth, gt_depth, mask)


def sampled_depth_l1_loss(depth_map: Tensor, points: Tensor, depths_gt: Tensor, scene_scale: float = 1.0) -> Tensor:
    """The trainers' depth supervision as one call (examples/simple_trainer.py:962-980, simple_trainer_2dgs.py:639-657):
    ``depth_map`` (``[C, H, W, 1]`` or ``[C, H, W]``, e.g. ``renders[..., 3:4]`` of an ``RGB+ED`` render, read in place) is
    sampled bilinearly at ``points [C, M, 2]`` - pixel coordinates ``(x, y)`` - with ``F.grid_sample``'s ``align_corners=True``
    semantics and zeros outside the image, and `depth_l1_loss` is applied to the samples and ``depths_gt [C, M]``. Sampling in
    pixel coordinates equals the reference's normalise-then-``grid_sample`` round trip to 1e-15 in float64.

    Departure from the reference: where a sample is ``<= 0`` (uncovered pixels, points off the image) its gradient is 0, not
    NaN; the loss value is the reference's.

    A float32 map on the GPU takes the fused kernels (the dense gradient of the map is a float atomic sum: points may share a
    pixel); CPU tensors, other dtypes, ``points`` or ``depths_gt`` that require grad and ``M == 0`` take
    `sampled_depth_l1_loss_torch`."""
    map3 = _depth_map_3d(depth_map, points, depths_gt)
    if (map3.is_cuda and map3.dtype == torch.float32 and points.device == map3.device and depths_gt.device == map3.device
            and points.dtype == torch.float32 and depths_gt.dtype == torch.float32 and not points.requires_grad
            and not depths_gt.requires_grad and 0 < map3.numel() < 2 ** 31 and 0 < depths_gt.numel() < 2 ** 31
            and max(map3.shape[1:]) < 2 ** 24):
        return _FusedSampledDepthL1.apply(depth_map, points, depths_gt, float(scene_scale))
    return depth_l1_loss_torch(_sample_depth_torch(map3, points), depths_gt, scene_scale)
