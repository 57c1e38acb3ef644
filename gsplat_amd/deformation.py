"""Deformation model of the dynamic-scene trainer (examples/dynamic_surgical_trainer.py; semantics restated from
gsplat/contrib/dynamic/deformation.py): `DeformNetwork`, an MLP over per-Gaussian plane features that emits deltas on
``(means, quats, opacities)``, and `DeformationTable`, the per-Gaussian flag that says which Gaussians it animates.

``h = trunk(plane_features)`` with ``trunk = Linear, ReLU, (Linear, ReLU) x (num_layers - 1)``; the result is
``(means + pos_head(h), quats + quat_head(h), opacities + opacity_head(h))``. The heads start at zero, so a fresh module returns
its inputs. Who produced ``plane_features`` (the reference: a HexPlane lookup) is not this module's concern.

Fused configuration: float32 CUDA tensors on one device, ``feature_dim == 64`` (the reference HexPlaneField's default,
``32 x len((1, 2))``), ``hidden_dim == 64``, ``num_layers == 3``, ``0 < N < 2**31``. It takes the kernels of csrc/deformation.hip
(gsx_deform_fwd / _bwd): one launch for the three outputs, the products on the fp32 matrix cores, the hidden activations never
written to memory, the backward recomputing the forward, every sum over the Gaussians in a fixed order without float atomics
(two runs are bit-equal), nothing read back from the device. Every other configuration - CPU tensors, other dtypes, widths,
depths or feature sizes - is evaluated by `deform_torch`, the reference's composition of tensor operations. The fused backward
is not itself differentiable; a caller who needs a second derivative calls `deform_torch`.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

__all__ = ["DeformNetwork", "DeformationTable", "deform", "deform_torch"]


def _check(module: "DeformNetwork", means: Tensor, quats: Tensor, opacities: Tensor, plane_features: Tensor) -> None:
    n = means.shape[0]
    if quats.shape[0] != n or opacities.shape[0] != n or plane_features.shape[0] != n:
        raise ValueError(
            f"DeformNetwork: batch dim mismatch — means {means.shape[0]}, quats {quats.shape[0]}, "
            f"opacities {opacities.shape[0]}, plane_features {plane_features.shape[0]}."
        )
    if plane_features.shape[-1] != module.feature_dim:
        raise ValueError(
            f"DeformNetwork: plane_features last dim {plane_features.shape[-1]} != feature_dim {module.feature_dim}."
        )
    if not (means.dtype == quats.dtype == opacities.dtype == plane_features.dtype):
        raise ValueError(
            f"DeformNetwork: dtype mismatch — means {means.dtype}, quats {quats.dtype}, "
            f"opacities {opacities.dtype}, plane_features {plane_features.dtype}."
        )


def deform_torch(module: "DeformNetwork", means: Tensor, quats: Tensor, opacities: Tensor,
                 plane_features: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """`deform` composed of torch calls as the reference composes it (any device and dtype, differentiable in everything, twice
    if need be): the CPU path, the float64 yardstick and the route of every configuration outside the fused one."""
    _check(module, means, quats, opacities, plane_features)
    h = module.trunk(plane_features)
    return means + module.pos_head(h), quats + module.quat_head(h), opacities + module.opacity_head(h)


def _rows(t: Tensor) -> Tensor:
    """Contiguous, and at a 16-byte boundary (a contiguous view can start at an odd storage offset; the kernels read rows as
    16-byte vectors)."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class _FusedDeform(torch.autograd.Function):
    """csrc/deformation.hip. The three heads go to the kernels as one [8, 64] matrix and one [8] bias, in the order
    [position 3 | quaternion 4 | opacity 1], and their gradients come back that way."""

    calls = 0  # forwards that took the kernels (tests assert on it)

    @staticmethod
    def forward(ctx, means, quats, opacities, plane_features, W1, b1, W2, b2, W3, b3, Wp, bp, Wq, bq, Wo, bo):
        from . import _cabi

        N = means.shape[0]
        x = _rows(plane_features)
        W1c, b1c, W2c, b2c, W3c, b3c = (t.contiguous() for t in (W1, b1, W2, b2, W3, b3))
        Wh, bh = torch.cat([Wp, Wq, Wo], dim=0), torch.cat([bp, bq, bo], dim=0)
        outs = tuple(torch.empty((N, k), device=means.device, dtype=torch.float32) for k in (3, 4, 1))
        _cabi.call("gsx_deform_fwd", means.contiguous(), quats.contiguous(), opacities.contiguous(), x, W1c, b1c, W2c, b2c, W3c,
                   b3c, Wh, bh, N, *outs)
        _FusedDeform.calls += 1
        ctx.set_materialize_grads(False)  # the cotangent of an output the loss does not use stays None
        ctx.save_for_backward(x, W1c, b1c, W2c, b2c, W3c, b3c, Wh, bh)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward kernel is not itself differentiable
    def backward(ctx, v_means, v_quats, v_opacities):
        from . import _cabi

        x, W1, b1, W2, b2, W3, b3, Wh, bh = ctx.saved_tensors
        N, dev = x.shape[0], x.device
        # a missing cotangent (an output the loss does not use) is a null pointer: zeros to the kernel, None to the caller
        cot = [None if v is None else v.to(torch.float32).contiguous() for v in (v_means, v_quats, v_opacities)]
        work = torch.empty(_cabi.query("gsx_deform_bwd_workspace_floats", N), device=dev, dtype=torch.float32)
        v_x = torch.empty_like(x) if ctx.needs_input_grad[3] else None
        v_W = torch.empty((3, 64, 64), device=dev, dtype=torch.float32)
        v_small = torch.empty(712, device=dev, dtype=torch.float32)
        _cabi.call("gsx_deform_bwd", x, W1, b1, W2, b2, W3, b3, Wh, bh, N, *cot, work, v_x, v_W, v_small)
        v_b1, v_b2, v_b3 = v_small[:64], v_small[64:128], v_small[128:192]
        v_Wh, v_bh = v_small[192:704].view(8, 64), v_small[704:712]
        return (v_means, v_quats, v_opacities, v_x, v_W[0], v_b1.clone(), v_W[1], v_b2.clone(), v_W[2], v_b3.clone(),
                v_Wh[0:3].clone(), v_bh[0:3].clone(), v_Wh[3:7].clone(), v_bh[3:7].clone(), v_Wh[7:8].clone(), v_bh[7:8].clone())


def _fused_ok(module: "DeformNetwork", means: Tensor, quats: Tensor, opacities: Tensor, plane_features: Tensor) -> bool:
    if not (module.feature_dim == 64 and module.hidden_dim == 64 and module.num_layers == 3 and len(module.trunk) == 6):
        return False
    if not (means.dim() == 2 and quats.dim() == 2 and opacities.dim() == 2 and plane_features.dim() == 2
            and means.shape[1] == 3 and quats.shape[1] == 4 and opacities.shape[1] == 1):
        return False
    if not (all(tuple(module.trunk[i].weight.shape) == (64, 64) for i in (0, 2, 4))
            and tuple(module.pos_head.weight.shape) == (3, 64) and tuple(module.quat_head.weight.shape) == (4, 64)
            and tuple(module.opacity_head.weight.shape) == (1, 64)):
        return False
    tensors = [means, quats, opacities, plane_features] + list(module.parameters())
    return (all(t.is_cuda and t.device == means.device and t.dtype == torch.float32 for t in tensors)
            and 0 < means.shape[0] < 2 ** 31)


def deform(module: "DeformNetwork", means: Tensor, quats: Tensor, opacities: Tensor,
           plane_features: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """``(means [N, 3], quats [N, 4], opacities [N, 1])`` moved by the deltas that ``module`` reads from
    ``plane_features [N, F]``. The fused configuration (module docstring) runs gsx_deform_fwd / _bwd; every other one is
    `deform_torch`."""
    _check(module, means, quats, opacities, plane_features)
    if not _fused_ok(module, means, quats, opacities, plane_features):
        return deform_torch(module, means, quats, opacities, plane_features)
    t = module.trunk
    return _FusedDeform.apply(means, quats, opacities, plane_features, t[0].weight, t[0].bias, t[2].weight, t[2].bias,
                              t[4].weight, t[4].bias, module.pos_head.weight, module.pos_head.bias, module.quat_head.weight,
                              module.quat_head.bias, module.opacity_head.weight, module.opacity_head.bias)


class DeformNetwork(nn.Module):
    """The reference's deformation network. Constructor, attribute and parameter names are the reference's
    (``trunk.{0,2,4}``, ``pos_head``, ``quat_head``, ``opacity_head``), so a ``state_dict`` moves between the two in either
    direction with ``strict=True``."""

    def __init__(self, feature_dim: int, hidden_dim: int = 64, num_layers: int = 3) -> None:
        super().__init__()
        if num_layers < 1:
            raise ValueError(f"num_layers must be >= 1, got {num_layers}.")
        if feature_dim < 1:
            raise ValueError(f"feature_dim must be >= 1, got {feature_dim}.")
        self.feature_dim = feature_dim
        self.hidden_dim = hidden_dim
        self.num_layers = num_layers
        layers = [nn.Linear(feature_dim, hidden_dim), nn.ReLU()]
        for _ in range(num_layers - 1):
            layers += [nn.Linear(hidden_dim, hidden_dim), nn.ReLU()]
        self.trunk = nn.Sequential(*layers)
        self.pos_head = nn.Linear(hidden_dim, 3)
        self.quat_head = nn.Linear(hidden_dim, 4)
        self.opacity_head = nn.Linear(hidden_dim, 1)
        for head in (self.pos_head, self.quat_head, self.opacity_head):  # the initial deformation is the identity
            nn.init.zeros_(head.weight)
            nn.init.zeros_(head.bias)

    def forward(self, means: Tensor, quats: Tensor, opacities: Tensor, t: Tensor, plane_features: Tensor):
        """``means [N, 3]``, ``quats [N, 4]``, ``opacities [N, 1]``, ``plane_features [N, feature_dim]`` ->
        ``(means_new, quats_new, opacities_new)``. ``t`` is ignored, as in the reference: time is already in the features."""
        return deform(self, means, quats, opacities, plane_features)


class DeformationTable:
    """The reference's per-Gaussian bool table of which Gaussians are dynamic: a plain ``torch.bool`` tensor ``mask`` that is
    resized in lock-step with the densification operations."""

    def __init__(self, num_gaussians: int, device: Optional[torch.device] = None) -> None:
        if num_gaussians < 0:
            raise ValueError(f"DeformationTable: num_gaussians must be >= 0, got {num_gaussians}.")
        self.mask = torch.zeros(num_gaussians, dtype=torch.bool, device=device)

    def __len__(self) -> int:
        return int(self.mask.shape[0])

    def set_indices(self, indices: Tensor, value: bool = True) -> None:
        """Marks the given Gaussians dynamic (static with ``value=False``)."""
        self.mask[indices] = value

    def prune(self, keep_mask: Tensor) -> None:
        """Drops the Gaussians whose ``keep_mask [N]`` is False."""
        if keep_mask.shape != self.mask.shape:
            raise ValueError(
                f"DeformationTable.prune: keep_mask shape {tuple(keep_mask.shape)} != table shape {tuple(self.mask.shape)}."
            )
        self.mask = self.mask[keep_mask]

    def duplicate(self, indices: Tensor) -> None:
        """Appends one copy per index, with its parent's flag; the originals stay."""
        self.mask = torch.cat([self.mask, self.mask[indices]], dim=0)

    def split(self, indices: Tensor, factor: int = 2) -> None:
        """Removes the given Gaussians and appends ``factor`` children for each, with the parent's flag."""
        if factor < 1:
            raise ValueError(f"DeformationTable.split: factor must be >= 1, got {factor}.")
        keep = torch.ones(self.mask.shape[0], dtype=torch.bool, device=self.mask.device)
        keep[indices] = False
        self.mask = torch.cat([self.mask[keep], self.mask[indices].repeat_interleave(factor)], dim=0)
