"""Colour correction of a render against its ground truth before it is scored (gsplat/color_correct.py; the trainer's
``use_color_correction_metric`` block, examples/simple_trainer.py: ``cc_psnr`` / ``cc_ssim`` / ``cc_lpips`` of a run with
``post_processing="bilateral_grid"`` or ``app_opt=True``).

`color_correct_quadratic` fits, ``num_iters`` times and per channel, ``ref`` by the ten quadratic features of the current image
over the pixels that are unclipped in the original image, the current image and ``ref``, and warps the image by the fit.
`color_correct_affine` fits ``a * ref + b = img`` per channel and applies the inverse. Shapes are ``[..., C]``: all leading
dimensions form one set of pixels and one warp serves the whole call.

float32 tensors with three channels on the GPU, outside autograd, take csrc/color_correct.hip: the quadratic form sums the
10 x 10 normal equations of every channel in double in one pass per iteration (the earlier warps are re-applied in registers, no
intermediate image is stored), solves them in double on the device and writes the corrected image in a last pass -
``2 * num_iters + 1`` launches and one host read, where the reference builds a ``[pixels, 10]`` matrix and runs fifteen ``lstsq``
calls, each followed by a host read. A rank-deficient system (a grey image, a channel without unclipped rows, fewer than ten
distinct pixels) is refused with a ``ValueError``: the reference trips its assert or returns unstable values there. Everything
else - CPU tensors, float64, ``C != 3``, inputs that need a gradient - takes the ``*_torch`` compositions.
"""
from __future__ import annotations

import torch
from torch import Tensor

_MAX_ITERS = 64  # GSX_CC_MAX_ITERS


def _channels_match(img: Tensor, ref: Tensor) -> None:
    if img.shape[-1] != ref.shape[-1]:
        raise ValueError(f"img's {img.shape[-1]} and ref's {ref.shape[-1]} channels must match")


def _unclipped(z: Tensor, eps: float) -> Tensor:
    """``eps <= z <= 1 - eps`` with both thresholds rounded to float32, ``1 - eps`` formed in double first: what torch
    compares a float32 tensor with when given Python scalars. Kept in every dtype, so that a float64 evaluation selects the
    rows the float32 one does (a value lying exactly on a threshold included)."""
    lo, hi = (float(torch.tensor(t, dtype=torch.float32)) for t in (eps, 1 - eps))
    return (z >= lo) & (z <= hi)


def _quadratic_features(x: Tensor) -> Tensor:
    """``[n, C] -> [n, C (C + 1) / 2 + C + 1]``: the products ``x_i x_j`` (``i <= j``, row-major), ``x`` itself, 1."""
    C = x.shape[-1]
    i, j = torch.triu_indices(C, C, device=x.device)
    return torch.cat([x[:, i] * x[:, j], x, torch.ones_like(x[:, :1])], dim=-1)


def color_correct_quadratic_torch(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = 0.5 / 255) -> Tensor:
    """`color_correct_quadratic` composed of torch calls (any device, dtype and channel count; differentiable): per iteration
    one feature matrix and one ``lstsq`` per channel on its masked copy."""
    _channels_match(img, ref)
    C = img.shape[-1]
    x, r = img.reshape(-1, C), ref.reshape(-1, C)
    usable = _unclipped(x, eps) & _unclipped(r, eps)  # of the original image and of ref: fixed over the iterations
    for _ in range(num_iters):
        A = _quadratic_features(x)
        rows = usable & _unclipped(x, eps)
        columns = []
        for c in range(C):
            m = rows[:, c]
            masked_A, masked_b = torch.where(m[:, None], A, torch.zeros_like(A)), torch.where(m, r[:, c], torch.zeros_like(r[:, c]))
            columns.append(torch.linalg.lstsq(masked_A, masked_b, rcond=-1).solution)
        W = torch.stack(columns, dim=-1)
        if not bool(torch.isfinite(W).all()):
            raise ValueError("color_correct_quadratic: the least-squares fit returned a non-finite warp")
        x = (A @ W).clip(0, 1)
    return x.reshape(img.shape)


def color_correct_affine_torch(img: Tensor, ref: Tensor) -> Tensor:
    """`color_correct_affine` composed of torch calls (any device, dtype and channel count; differentiable)."""
    _channels_match(img, ref)
    C = img.shape[-1]
    x, r = img.reshape(-1, C), ref.reshape(-1, C)
    mean_r, mean_x = r.mean(dim=0), x.mean(dim=0)
    var_r = ((r * r).mean(dim=0) - mean_r * mean_r).clamp(min=1e-8)
    a = ((r * x).mean(dim=0) - mean_r * mean_x) / var_r
    b = mean_x - a * mean_r
    a = torch.where(a.abs() < 1e-8, torch.ones_like(a), a)
    return ((x - b) / a).clip(0, 1).reshape(img.shape)


def _fused_ok(img: Tensor, ref: Tensor) -> bool:
    if torch.is_grad_enabled() and (img.requires_grad or ref.requires_grad):
        return False
    return (img.is_cuda and ref.device == img.device and img.dtype == torch.float32 and ref.dtype == torch.float32
            and img.shape[-1] == 3 and ref.numel() == img.numel() and 0 < img.numel() < 2 ** 31)


def _scratch(n: int, device) -> Tensor:
    from . import _cabi

    return torch.empty(195 * _cabi.query("gsx_cc_blocks", n), device=device, dtype=torch.float64)  # GSX_CC_PARTIALS


class _FusedColorCorrectQuadratic:
    """`color_correct_quadratic` on the MI355X: csrc/color_correct.hip (gsx_cc_quadratic)."""

    calls = 0  # calls that took the kernels (tests assert on it)

    @staticmethod
    def apply(img: Tensor, ref: Tensor, num_iters: int, eps: float) -> Tensor:
        from . import _cabi

        x, r = img.detach().reshape(-1, 3).contiguous(), ref.detach().reshape(-1, 3).contiguous()
        n, dev = x.shape[0], x.device
        out = torch.empty_like(x)
        warps = torch.empty((num_iters, 10, 3), device=dev, dtype=torch.float64)
        status = torch.empty(1, device=dev, dtype=torch.int32)  # cleared by the entry point
        _cabi.call("gsx_cc_quadratic", x, r, n, num_iters, float(eps), _scratch(n, dev), warps, status, out)
        _FusedColorCorrectQuadratic.calls += 1
        bits = int(status.item())  # the one host read of the call
        if bits:
            channels = [c for c in range(3) if bits >> c & 1]
            raise ValueError(f"color_correct_quadratic: rank-deficient system in channel(s) {channels}: fewer than ten independent "
                             "rows are unclipped in img and ref (a grey image, a saturated channel, too few pixels)")
        return out.reshape(img.shape)


class _FusedColorCorrectAffine:
    """`color_correct_affine` on the MI355X: csrc/color_correct.hip (gsx_cc_affine), no host read."""

    calls = 0  # calls that took the kernels (tests assert on it)

    @staticmethod
    def apply(img: Tensor, ref: Tensor) -> Tensor:
        from . import _cabi

        x, r = img.detach().reshape(-1, 3).contiguous(), ref.detach().reshape(-1, 3).contiguous()
        n, dev = x.shape[0], x.device
        out = torch.empty_like(x)
        coef = torch.empty((3, 2), device=dev, dtype=torch.float64)
        _cabi.call("gsx_cc_affine", x, r, n, _scratch(n, dev), coef, out)
        _FusedColorCorrectAffine.calls += 1
        return out.reshape(img.shape)


def color_correct_quadratic(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = 0.5 / 255) -> Tensor:
    """Warp ``img`` towards the colours of ``ref`` by an iterated quadratic fit (gsplat/color_correct.py:
    color_correct_quadratic). ``img`` and ``ref``: ``[..., C]`` in [0, 1]; all leading dimensions form one set of pixels.

    Each of the ``num_iters`` rounds fits every channel of ``ref`` by the features ``(rr, rg, rb, gg, gb, bb, r, g, b, 1)`` of
    the current image, over the pixels whose value in that channel lies in ``[eps, 1 - eps]`` in the original image, in the
    current image and in ``ref``, then replaces the image by ``clip(features @ warp, 0, 1)``. ``num_iters == 0`` returns
    ``img`` reshaped.

    float32 tensors with ``C == 3`` on the GPU take the fused kernels when no gradient is wanted (under ``no_grad``, or when
    neither input requires one): a new tensor of ``img``'s shape, bit-equal between runs, one host read, and a ``ValueError`` for
    a rank-deficient system. Anything else takes `color_correct_quadratic_torch`."""
    _channels_match(img, ref)
    if 1 <= num_iters <= _MAX_ITERS and _fused_ok(img, ref):
        return _FusedColorCorrectQuadratic.apply(img, ref, int(num_iters), float(eps))
    return color_correct_quadratic_torch(img, ref, num_iters, eps)


def color_correct_affine(img: Tensor, ref: Tensor) -> Tensor:
    """Warp ``img`` towards the colours of ``ref`` by a per-channel affine fit (gsplat/color_correct.py: color_correct_affine):
    with ``a ref + b = img`` fitted over all pixels (``Var(ref)`` clamped to ``>= 1e-8``, ``a = 1`` where ``|a| < 1e-8``) the
    result is ``clip((img - b) / a, 0, 1)``. ``img`` and ``ref``: ``[..., C]``; all leading dimensions form one set of pixels.

    float32 tensors with ``C == 3`` on the GPU take the fused kernels when no gradient is wanted (moments in double, no host
    read, bit-equal between runs); anything else `color_correct_affine_torch`."""
    _channels_match(img, ref)
    if _fused_ok(img, ref):
        return _FusedColorCorrectAffine.apply(img, ref)
    return color_correct_affine_torch(img, ref)
