"""CPU dry run of the host side of the pipeline (no GPU in the build container).

The product path has no CPU fallback, so nothing can be COMPUTED here — but everything above the kernels can be
EXERCISED: with device pointers taken from CPU tensors and launch failures ("no ROCm-capable device") ignored, a call of
rasterization() runs its orchestration, the op implementations, the ctypes marshalling of every C-ABI call (argument
count / types against include/gsplat_amd.h) and the host-side checks of the entry points (GSX_REQUIRE) until something
needs a value that only a kernel could have produced. The compiled op bodies (csrc/torch_ops.cpp) run on the CPU tensors
through their CUDA-key kernel up to the point where they would touch the device; past it, the ones that would launch
(compositing, offsets) hand out outputs of the right shape. Outputs are garbage; errors are real. Used by
tests/test_host_dry_run.py for the empty-scene path, whose control flow does not depend on kernel results.

    python tools/dry_run.py            # empty 3DGS / 2DGS scenes, dense and packed, forward + backward
"""
import os
import sys
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def install():
    """Patch gsplat_amd for the dry run (this process only). Returns the list that collects the C-ABI calls made."""
    import gsplat_amd  # noqa: F401
    from gsplat_amd import _cabi, _ops

    calls = []
    _cabi._refuse_host_tensor = lambda t: None  # CPU tensors stand in for device tensors
    _cabi.current_stream = lambda: 0
    real_call = _cabi.call

    def call(name, *args):
        calls.append(name)
        try:
            real_call(name, *args)
        except _cabi.GsplatAmdError as e:  # a launch / memset without a device; host-side check failures are ValueError
            if not any(w in str(e) for w in ("device", "memset", "launch")):
                raise

    _cabi.call = call
    _ops.call = call  # its imported copy
    cpu = torch.library.Library("gsplat", "IMPL", "CPU")
    for name in _ops.SCHEMAS:
        cpu.impl(name, _ops.impl(name) if name in _ops._impls else _compiled_on_cpu(name))
    install.keep = cpu
    return calls


def _launch_outputs(name, a):
    """Outputs of the compiled bodies that would launch kernels even for an empty scene (fills of the images / offsets)."""
    if name == "intersect_offset":  # (isect_ids, I, tile_width, tile_height)
        return torch.zeros(a[1], a[3], a[2], dtype=torch.int32)
    means2d, colors = a[0], a[2]
    W, H, offsets = (a[6], a[7], a[9]) if name == "rasterize_to_pixels_3dgs" else (a[8], a[9], a[11])
    absgrad = a[12] if name == "rasterize_to_pixels_3dgs" else a[14]
    hw = tuple(offsets.shape[:-2]) + (H, W)
    img = lambda d: torch.empty(hw + (d,))  # noqa: E731
    holder = torch.zeros_like(means2d) if absgrad else torch.empty(0)
    ids = torch.empty(hw, dtype=torch.int32)
    if name == "rasterize_to_pixels_3dgs":
        return img(colors.shape[-1]), img(1), holder, ids
    return img(colors.shape[-1]), img(1), img(3), img(1), img(1), holder, ids, ids.clone()


def _compiled_on_cpu(name):
    op = getattr(torch.ops.gsplat, name).default
    cuda = torch._C.DispatchKeySet(torch._C.DispatchKey.CUDA)

    def body(*args):
        try:
            return op.redispatch(cuda, *args)
        except RuntimeError as e:  # the body's device guard / stream lookup, past its host-side checks
            if not any(w in str(e) for w in ("ROCm-capable device", "no CPU fallback")) or name not in (
                    "intersect_offset", "rasterize_to_pixels_3dgs", "rasterize_to_pixels_2dgs"):
                raise
            return _launch_outputs(name, args)

    return body


def empty_scene(fn: str, packed: bool):
    import gsplat_amd
    from _util import make_scene

    W, H, C = 96, 64, 2
    names = ("means", "quats", "scales", "opacities", "colors")
    sc, _, _ = make_scene(N=8, C=C, width=W, height=H, seed=2)
    leaves = {k: sc[k][:0].clone().requires_grad_(True) for k in names}
    bg = torch.rand(C, 3)
    if fn == "3dgs":
        rc, ra, meta = gsplat_amd.rasterization(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"],
                                                leaves["colors"], sc["viewmats"], sc["Ks"], W, H, packed=packed,
                                                backgrounds=bg, render_mode="RGB+ED", absgrad=True)
        (rc.sum() + ra.sum()).backward()
        assert rc.shape == (C, H, W, 4) and meta["isect_ids"].numel() == 0
    else:
        out = gsplat_amd.rasterization_2dgs(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"],
                                            leaves["colors"], sc["viewmats"], sc["Ks"], W, H, packed=packed,
                                            backgrounds=bg, render_mode="RGB+D", distloss=True)
        (out[0].sum() + out[1].sum() + out[2].sum() + out[4].sum()).backward()
        assert out[0].shape == (C, H, W, 4) and out[6]["isect_ids"].numel() == 0


def main() -> int:
    calls = install()
    bad = 0
    for fn in ("3dgs", "2dgs"):
        for packed in (False, True):
            n0 = len(calls)
            try:
                empty_scene(fn, packed)
                print(f"{fn} packed={packed}: OK ({len(calls) - n0} C-ABI calls: {sorted(set(calls[n0:]))})")
            except Exception as e:  # noqa: BLE001
                bad += 1
                print(f"{fn} packed={packed}: {type(e).__name__}: {str(e)[:300]}")
                for f in traceback.extract_tb(e.__traceback__)[-4:]:
                    print("    ", os.path.basename(f.filename), f.lineno, f.name)
    return bad


if __name__ == "__main__":
    sys.exit(main())
