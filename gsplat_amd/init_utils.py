"""Bringing up a scene: the nearest-neighbour scale initialisation every reference trainer starts with.

``knn(x, K)`` is the trainer's ``examples/utils.py:156`` (scikit-learn ``NearestNeighbors(n_neighbors=K).fit(x).kneighbors(x)``
on the host): the Euclidean distances from every point of ``x [N, 3]`` to its K nearest points of ``x``, itself included,
ascending - column 0 is 0 and ``knn(points, 4)[:, 1:]`` drops into ``simple_trainer.py:321``. ``knn_scale_init(xyz, k)`` is the
library's own statement, ``gsplat/init_utils.py:145``: ``log(max(rms of the distances to the k nearest OTHER points, eps))``.

Fused configuration: float32 CUDA points, ``K <= 16``, no gradient asked for. It takes the kernels of csrc/knn.hip
(gsx_knn_bin, one ``torch.sort`` of distinct int64 keys, gsx_knn_search): an exact search over a uniform grid with an all-points
scan for the rows the grid does not serve, distances from coordinate differences, nothing read back from the device, no float
atomics, bit-equal between runs and under a permutation of the rows. Every other input - CPU tensors, float64, ``K > 16``,
points that require grad while grad is enabled - is evaluated by ``knn_torch`` / ``knn_scale_init_torch``, a chunked
composition of tensor operations (O(N^2); differentiable). The fused path is not differentiable: initialisation runs without
grad.

Non-finite points (a NaN or infinite coordinate) are nobody's neighbour; their own row is NaN, index -1. Among equal distances
which index is reported is unspecified.

``multi_frame_depth_unprojection`` of the reference's module is not here.
"""
from __future__ import annotations

from typing import Tuple, Union

import torch
from torch import Tensor

__all__ = ["knn", "knn_scale_init", "knn_torch", "knn_scale_init_torch", "knn_last_stats"]

RING_CAP = 8  # rings of cells a query walks before it is handed to the all-points scan (csrc/knn.hip)
_FUSED_MAX_K = 16


def _check(x: Tensor, K: int, who: str) -> int:
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{who}: points must be [N, 3], got {tuple(x.shape)}")
    if K < 1:
        raise ValueError(f"{who}: K = {K} must be at least 1")
    if K > x.shape[0]:
        raise ValueError(f"{who}: K = {K} neighbours asked of {x.shape[0]} points")
    return x.shape[0]


def knn_torch(x: Tensor, K: int = 4, return_indices: bool = False, chunk_size: int = 1024) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """`knn` composed of tensor operations on any device and dtype, `chunk_size` query rows at a time against all N points
    (memory O(chunk_size * N)), squared distances from coordinate differences, ``(dx dx + dy dy) + dz dz``."""
    N = _check(x, K, "knn_torch")
    finite = torch.isfinite(x).all(dim=-1)
    inf = torch.tensor(float("inf"), dtype=x.dtype, device=x.device)
    cols = x.unbind(-1)
    chunk = max(1, min(int(chunk_size), N))
    rows_d, rows_i = [], []
    for s in range(0, N, chunk):
        d = [x[s:s + chunk, a:a + 1] - cols[a][None, :] for a in range(3)]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        d2 = torch.where(finite[None, :], d2, inf)
        v, i = torch.topk(d2, K, dim=-1, largest=False, sorted=True)
        pos = v > 0  # sqrt with a zero (not infinite) derivative at the zero self-distance
        v = torch.where(pos, torch.where(pos, v, torch.ones_like(v)).sqrt(), torch.zeros_like(v))
        rows_d.append(v)
        rows_i.append(torch.where(torch.isinf(v), torch.full_like(i, -1), i))
    dist, idx = torch.cat(rows_d), torch.cat(rows_i)
    dist = torch.where(finite[:, None], dist, torch.full_like(dist, float("nan")))
    idx = torch.where(finite[:, None], idx, torch.full_like(idx, -1))
    return (dist, idx) if return_indices else dist


def _rms_log(neighbor_dists: Tensor, eps: float) -> Tensor:
    return neighbor_dists.pow(2).mean(dim=-1).sqrt().clamp_min(eps).log()


def knn_scale_init_torch(xyz: Tensor, k: int = 3, eps: float = 1e-7, chunk_size: int = 1024) -> Tensor:
    """`knn_scale_init` through `knn_torch`."""
    n = xyz.shape[0]
    if n <= k:
        raise ValueError(f"knn_scale_init: need at least k+1={k + 1} points, got {n}.")
    return _rms_log(knn_torch(xyz, k + 1, chunk_size=chunk_size)[:, 1:], eps)


_last_work = None  # the workspace of the last fused call, for knn_last_stats


def _fused_ok(x: Tensor, K: int) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and K <= _FUSED_MAX_K and x.shape[0] < 2 ** 31 - 1
            and not (x.requires_grad and torch.is_grad_enabled()))


def _knn_fused(x: Tensor, K: int, return_indices: bool, ring_cap: int = RING_CAP):
    """csrc/knn.hip. Three launches, a sort of N distinct int64 keys, four more launches; the host reads nothing back."""
    global _last_work
    from . import _cabi

    x = x.detach().contiguous()
    N = x.shape[0]
    with torch.cuda.device(x.device):
        work = torch.empty(_cabi.query("gsx_knn_workspace_bytes", N, K), dtype=torch.uint8, device=x.device)
        keys = torch.empty(N, dtype=torch.int64, device=x.device)
        _cabi.call("gsx_knn_bin", x, N, work, keys)
        keys = torch.sort(keys).values
        dist = torch.empty((N, K), dtype=torch.float32, device=x.device)
        idx = torch.empty((N, K), dtype=torch.int64, device=x.device) if return_indices else None
        _cabi.call("gsx_knn_search", x, keys, N, K, int(ring_cap), work, dist, idx)
    _last_work = work
    return (dist, idx) if return_indices else dist


def knn_last_stats() -> dict:
    """What the last fused call on this process did, read back from its workspace (synchronises; for tests and
    tools/knn_bench.py): grid dims, cell count, and the number of rows that took the all-points scan."""
    if _last_work is None:
        raise RuntimeError("knn_last_stats: no fused call yet")
    head = _last_work[:64].cpu()
    ints = head.view(torch.int32)
    return {"dims": [int(v) for v in ints[9:12]], "deferred": int(ints[12]), "cells": int(ints[13]),
            "box_min": [float(v) for v in head.view(torch.float32)[0:3]],
            "cell_size": [float(v) for v in head.view(torch.float32)[6:9]]}


def knn(x: Tensor, K: int = 4, return_indices: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """Distances ``[N, K]`` from every point of ``x [N, 3]`` to its K nearest points of ``x``, itself included, ascending; with
    ``return_indices`` also their ``int64 [N, K]`` indices. ``K > N`` raises ``ValueError``."""
    _check(x, K, "knn")
    if _fused_ok(x, K):
        return _knn_fused(x, K, return_indices)
    return knn_torch(x, K, return_indices)


def knn_scale_init(xyz: Tensor, k: int = 3, eps: float = 1e-7, chunk_size: int = 1024) -> Tensor:
    """Per-point initial log-scale ``[N]``: ``log(max(rms of the distances to the k nearest other points, eps))``, the
    reference's signature and value (gsplat/init_utils.py:145). ``chunk_size`` only affects the torch path. ``N <= k`` raises
    ``ValueError``."""
    n = xyz.shape[0]
    if n <= k:
        raise ValueError(f"knn_scale_init: need at least k+1={k + 1} points, got {n}.")
    _check(xyz, k + 1, "knn_scale_init")
    if _fused_ok(xyz, k + 1):
        return _rms_log(_knn_fused(xyz, k + 1, False)[:, 1:], eps)
    return knn_scale_init_torch(xyz, k, eps, chunk_size)
