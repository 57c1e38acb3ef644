"""Per-Gaussian appearance model: the colour of every Gaussian as a small MLP over (per-image embedding, per-Gaussian feature,
SH basis of the view direction), which the reference trainer uses with ``app_opt=True`` (examples/simple_trainer.py:477,
547-566, 673-681; semantics restated from examples/utils.py:66-129).

For camera ``c`` and Gaussian ``n`` the input row is ``[embeds[embed_ids[c]] | features[n] | Y(normalize(dirs[c, n]))]`` with
``Y`` the ``(module sh_degree + 1)^2`` real SH bases, those beyond ``(sh_degree + 1)^2`` of the call zero; ``color_head`` is
``Linear, ReLU, (Linear, ReLU) x (mlp_depth - 1), Linear(., 3)``. ``embed_ids=None`` means zero embeddings, ``embed_dim == 0`` no
embedding part at all. ``dirs`` are normalised as ``F.normalize`` does (``d / max(|d|, 1e-12)``).

Fused configuration: float32 CUDA tensors, ``mlp_width == 64``, ``mlp_depth == 2``, ``feature_dim == 32``, module
``sh_degree == 3``, ``embed_dim`` in {0, 16}. It takes the kernels of csrc/appearance.hip (gsx_appearance_fwd / _bwd): the three
products on the fp32 matrix cores, the hidden activations never written to memory, the backward recomputing the forward, every
sum in a fixed order without float atomics (two runs are bit-equal), nothing read back from the device. Every other
configuration - CPU tensors, other dtypes, widths, depths, feature or embedding sizes - is evaluated by `appearance_torch`, the
reference's composition of tensor operations. The fused backward is not itself differentiable (as with `photometric_loss`); a
caller who needs a second derivative calls `appearance_torch`.

Gradients reach ``features``, ``embeds.weight``, every ``color_head`` parameter and ``dirs``: the trainer forms
``dirs = means[None] - camtoworlds[:, None, :3, 3]`` itself, and ``means`` and the poses are reached through ``v_dirs``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

__all__ = ["AppearanceOptModule", "appearance", "appearance_torch", "sh_bases_torch"]


def sh_bases_torch(degree: int, dirs: Tensor) -> Tensor:
    """The ``(degree + 1)^2`` real SH bases (Sloan, JCGT 2013, polynomial forms; degree <= 4) at unit directions
    ``dirs [..., 3]``."""
    if not 0 <= degree <= 4:
        raise ValueError(f"sh_bases_torch: degree {degree} outside 0..4")
    x, y, z = dirs.unbind(-1)
    out = [torch.full_like(x, 0.2820947917738781)]
    if degree >= 1:
        c1 = 0.48860251190292
        out += [-c1 * y, c1 * z, -c1 * x]
    if degree >= 2:
        z2 = z * z
        b = -1.092548430592079 * z
        C1, S1 = x * x - y * y, 2 * x * y
        out += [0.5462742152960395 * S1, b * y, 0.9461746957575601 * z2 - 0.3153915652525201, b * x, 0.5462742152960395 * C1]
    if degree >= 3:
        c = -2.285228997322329 * z2 + 0.4570457994644658
        b = 1.445305721320277 * z
        a = -0.5900435899266435
        C2, S2 = x * C1 - y * S1, x * S1 + y * C1
        out += [a * S2, b * S1, c * y, z * (1.865881662950577 * z2 - 1.119528997770346), c * x, b * C1, a * C2]
    if degree >= 4:
        d = z * (-4.683325804901025 * z2 + 2.007139630671868)
        c = 3.31161143515146 * z2 - 0.47308734787878
        b = -1.770130769779931 * z
        a = 0.6258357354491763
        C3, S3 = x * C2 - y * S2, x * S2 + y * C2
        out += [a * S3, b * S2, c * S1, d * y,
                1.984313483298443 * z2 * (1.865881662950577 * z2 - 1.119528997770346)
                - 1.006230589874905 * (0.9461746957575601 * z2 - 0.3153915652525201),
                d * x, c * C1, b * C2, a * C3]
    return torch.stack(out, dim=-1)


def _check(module: "AppearanceOptModule", features: Tensor, embed_ids, dirs: Tensor, sh_degree: int) -> None:
    if features.dim() != 2:
        raise ValueError(f"appearance: features must be [N, D], got {tuple(features.shape)}")
    if dirs.dim() != 3 or dirs.shape[1] != features.shape[0] or dirs.shape[2] != 3:
        raise ValueError(f"appearance: dirs must be [C, {features.shape[0]}, 3], got {tuple(dirs.shape)}")
    if embed_ids is not None and (embed_ids.dim() != 1 or embed_ids.shape[0] != dirs.shape[0]):
        raise ValueError(f"appearance: embed_ids must be [{dirs.shape[0]}], got {tuple(embed_ids.shape)}")
    if not 0 <= sh_degree <= module.sh_degree:
        raise ValueError(f"appearance: sh_degree {sh_degree} outside 0..{module.sh_degree} of the module")


def appearance_torch(module: "AppearanceOptModule", features: Tensor, embed_ids: Optional[Tensor], dirs: Tensor,
                     sh_degree: int) -> Tensor:
    """`appearance` composed of torch calls as the reference composes it (any device and dtype, differentiable in everything,
    twice if need be): the CPU path, the float64 yardstick and the route of every configuration outside the fused one."""
    _check(module, features, embed_ids, dirs, sh_degree)
    C, N = dirs.shape[:2]
    u = F.normalize(dirs, dim=-1)
    n_use, n_all = (sh_degree + 1) ** 2, (module.sh_degree + 1) ** 2
    bases = sh_bases_torch(sh_degree, u)
    if n_all > n_use:
        bases = torch.cat([bases, bases.new_zeros(C, N, n_all - n_use)], dim=-1)
    parts = [features[None].expand(C, -1, -1), bases.to(features.dtype)]
    if module.embed_dim > 0:
        if embed_ids is None:
            emb = features.new_zeros(C, module.embed_dim)
        else:
            emb = module.embeds(embed_ids)
        parts.insert(0, emb[:, None, :].expand(-1, N, -1))
    return module.color_head(torch.cat(parts, dim=-1))


class _FusedAppearance(torch.autograd.Function):
    """csrc/appearance.hip. `emb` is the [C, 16] embedding rows (or None); the embedding part of layer 1 is folded into a
    per-camera bias here and unfolded from the per-camera sums the backward kernel returns."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, features, dirs, emb, W1, b1, W2, b2, W3, b3, sh_degree: int, embed_dim: int):
        import ctypes

        from . import _cabi

        C, N = dirs.shape[:2]
        feats = features.contiguous()
        if feats.data_ptr() % 16:  # a contiguous view at an odd storage offset: the kernels read rows as 16-byte vectors
            feats = feats.clone()
        W1c, W2c, W3c, b2c, b3c = W1.contiguous(), W2.contiguous(), W3.contiguous(), b2.contiguous(), b3.contiguous()
        if emb is not None:
            bias1 = torch.addmm(b1, emb, W1c[:, :embed_dim].t())  # [C, 64]
        else:
            bias1 = b1[None].expand(C, -1).contiguous()
        colors = torch.empty((C, N, 3), device=features.device, dtype=torch.float32)
        sd = (ctypes.c_int64 * 3)(*dirs.stride())
        _cabi.call("gsx_appearance_fwd", feats, _cabi.strided(dirs), sd, bias1, W1c,
                   embed_dim, W2c, b2c, W3c, b3c, N, C, sh_degree, colors)
        _FusedAppearance.calls += 1
        ctx.save_for_backward(feats, dirs, emb, bias1, W1c, W2c, b2c, W3c, b3c)
        ctx.sh_degree, ctx.embed_dim = sh_degree, embed_dim
        return colors

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_colors):
        import ctypes

        from . import _cabi

        feats, dirs, emb, bias1, W1, W2, b2, W3, b3 = ctx.saved_tensors
        C, N = dirs.shape[:2]
        E = ctx.embed_dim
        dev = feats.device
        v_colors = v_colors.to(torch.float32).contiguous()
        work = torch.empty(_cabi.query("gsx_appearance_bwd_workspace_floats", N, C), device=dev, dtype=torch.float32)
        v_features = torch.empty_like(feats)
        v_dirs = torch.empty((C, N, 3), device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        v_W1x = torch.empty((64, 64), device=dev, dtype=torch.float32)
        v_W2 = torch.empty((64, 64), device=dev, dtype=torch.float32)
        v_small = torch.empty(260 + 64 * C, device=dev, dtype=torch.float32)
        sd = (ctypes.c_int64 * 3)(*dirs.stride())
        _cabi.call("gsx_appearance_bwd", feats, _cabi.strided(dirs), sd, emb, bias1, W1, E, W2, b2, W3, b3, N, C, ctx.sh_degree,
                   v_colors, work, v_features, v_dirs, v_W1x, v_W2, v_small)
        v_b2, v_W3, v_b3 = v_small[:64], v_small[64:256].view(3, 64), v_small[256:259]
        s = v_small[260:].view(C, 64)  # per camera: the sum over the Gaussians of the gradient at layer 1's pre-activation
        v_b1 = s.sum(0)
        v_emb = None
        if E == 0:
            v_W1 = v_W1x[:, :48]
        elif emb is None:  # zero embeddings: their columns of W1 saw zeros
            v_W1 = torch.cat([torch.zeros_like(v_W1x[:, 48:]), v_W1x[:, :48]], dim=1)
        else:
            v_W1 = torch.cat([v_W1x[:, 48:], v_W1x[:, :48]], dim=1)
            v_emb = s @ W1[:, :E]
        return v_features, v_dirs, v_emb, v_W1, v_b1, v_W2, v_b2.clone(), v_W3.clone(), v_b3.clone(), None, None


def _fused_ok(module: "AppearanceOptModule", features: Tensor, embed_ids, dirs: Tensor) -> bool:
    head = module.color_head
    if not (module.sh_degree == 3 and module.embed_dim in (0, 16) and len(head) == 5):
        return False
    if not (tuple(head[0].weight.shape) == (64, module.embed_dim + 48) and tuple(head[2].weight.shape) == (64, 64)
            and tuple(head[4].weight.shape) == (3, 64) and features.shape[1] == 32):
        return False
    tensors = [features, dirs] + [p for p in head.parameters()] + ([module.embeds.weight] if module.embed_dim else [])
    return (all(t.is_cuda and t.device == features.device and t.dtype == torch.float32 for t in tensors)
            and (embed_ids is None or embed_ids.device == features.device)
            and 0 < features.shape[0] < 2 ** 31 and 0 < dirs.shape[0] < 2 ** 16)


def appearance(module: "AppearanceOptModule", features: Tensor, embed_ids: Optional[Tensor], dirs: Tensor,
               sh_degree: int) -> Tensor:
    """Colours ``[C, N, 3]`` of ``features [N, D1]`` seen along ``dirs [C, N, 3]`` (not normalised) by the cameras with
    embeddings ``embed_ids [C]`` (``None``: zero embeddings), with the SH bases up to ``sh_degree``. The fused configuration
    (module docstring) runs gsx_appearance_fwd / _bwd; every other one is `appearance_torch`."""
    _check(module, features, embed_ids, dirs, sh_degree)
    if not _fused_ok(module, features, embed_ids, dirs):
        return appearance_torch(module, features, embed_ids, dirs, sh_degree)
    head = module.color_head
    emb = module.embeds(embed_ids) if module.embed_dim > 0 and embed_ids is not None else None
    return _FusedAppearance.apply(features, dirs, emb, head[0].weight, head[0].bias, head[2].weight, head[2].bias,
                                  head[4].weight, head[4].bias, int(sh_degree), int(module.embed_dim))


class AppearanceOptModule(nn.Module):
    """The reference's appearance module: ``embeds`` (``n`` images x ``embed_dim``) and ``color_head``. Constructor, attribute
    and parameter names are the reference's, so a ``state_dict`` moves between the two in either direction with ``strict=True``."""

    def __init__(self, n: int, feature_dim: int, embed_dim: int = 16, sh_degree: int = 3, mlp_width: int = 64,
                 mlp_depth: int = 2):
        super().__init__()
        self.embed_dim = embed_dim
        self.sh_degree = sh_degree
        self.embeds = nn.Embedding(n, embed_dim)
        layers = [nn.Linear(embed_dim + feature_dim + (sh_degree + 1) ** 2, mlp_width), nn.ReLU(inplace=True)]
        for _ in range(mlp_depth - 1):
            layers += [nn.Linear(mlp_width, mlp_width), nn.ReLU(inplace=True)]
        layers.append(nn.Linear(mlp_width, 3))
        self.color_head = nn.Sequential(*layers)

    def forward(self, features: Tensor, embed_ids: Optional[Tensor], dirs: Tensor, sh_degree: int) -> Tensor:
        """``features [N, D1]``, ``embed_ids [C]`` or ``None``, ``dirs [C, N, 3]`` -> colours ``[C, N, 3]``."""
        return appearance(self, features, embed_ids, dirs, sh_degree)
