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
    python tools/dry_run.py cameras    # the 3DGUT projection and ray-generation op bodies for every camera model
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


def ut_cameras(calls):
    """projection_ut_3dgs_fused and camera_pixel_rays for every camera model of the one entry each (pinhole, OpenCV pinhole,
    ortho, fisheye, f-theta) under a global and a rolling shutter, behind a windshield, with the Euclidean sort depth: B = 1,
    C = 2, N = 4, 5 x 3 pixels. call() checks every argument list against the header; the entries run their own checks and read
    the host records. Returns the entry points these op bodies reached."""
    from gsplat_amd import _ops

    n0 = len(calls)
    g = torch.Generator().manual_seed(3)
    B, C, N, W, H = 1, 2, 4, 5, 3
    means, quats = torch.randn(B, N, 3, generator=g), torch.randn(B, N, 4, generator=g)
    scales, opacities = torch.rand(B, N, 3, generator=g) * 0.1, torch.rand(B, N, generator=g)
    viewmats = torch.eye(4).expand(B, C, 4, 4).contiguous()
    viewmats_rs = viewmats.clone()
    viewmats_rs[..., 0, 3] = 0.1
    Ks = torch.tensor([[4.0, 0.0, 2.5], [0.0, 4.0, 1.5], [0.0, 0.0, 1.0]]).expand(B, C, 3, 3).contiguous()
    cls = torch.classes.gsplat
    ftheta = cls.FThetaCameraDistortionParameters(
        reference_poly=1, pixeldist_to_angle_poly=[0.0, 0.25, 0.0, 0.0, 0.0, 0.0], angle_to_pixeldist_poly=[0.0, 4.0, 0.0, 0.0, 0.0, 0.0],
        max_angle=1.2, linear_cde=[1.0, 0.0, 0.0])
    windshield = cls.BivariateWindshieldModelParameters()
    windshield.horizontal_poly = windshield.horizontal_poly_inverse = torch.tensor([0.0, 1.0, 0.0])
    windshield.vertical_poly = windshield.vertical_poly_inverse = torch.tensor([0.0, 0.0, 1.0])
    radial6, radial4 = torch.full((B, C, 6), 0.01), torch.full((B, C, 4), 0.01)
    tangential, thin_prism = torch.full((B, C, 2), 1e-3), torch.full((B, C, 4), 1e-3)
    cameras = {  # name: (camera model id, radial, tangential, thin prism, f-theta record)
        "pinhole": (0, None, None, None, None), "opencv": (0, radial6, tangential, thin_prism, None),
        "opencv-radial4": (0, radial4, None, None, None), "ortho": (1, None, None, None, None),
        "fisheye": (2, radial4, None, None, None), "fisheye-plain": (2, None, None, None, None),
        "ftheta": (3, None, None, None, ftheta)}
    runs = [(name, rs, True, None) for name in cameras for rs in (_ops.ROLLING_SHUTTER_GLOBAL, 1)]
    runs += [("pinhole", _ops.ROLLING_SHUTTER_GLOBAL, True, windshield), ("ftheta", _ops.ROLLING_SHUTTER_GLOBAL, False, None)]
    for name, rs, global_z, ext in runs:
        model, radial, tang, prism, ft = cameras[name]
        rolling = rs != _ops.ROLLING_SHUTTER_GLOBAL
        out = _ops.projection_ut_3dgs_fused(means, quats, scales, opacities, viewmats, viewmats_rs if rolling else None, Ks, W, H,
                                            0.3, 0.01, 1e10, 0.0, True, model, global_z, None, rs, radial, tang, prism, ft, None, ext)
        assert out[0].shape == (B, C, N, 2) and out[0].dtype == torch.int32 and out[4].shape == (B, C, N)
        rays = _ops.camera_pixel_rays(viewmats, viewmats_rs if rolling else None, Ks, W, H, model, rs, radial, tang, prism, ft, ext)
        assert rays.shape == (B, C, H, W, 6)
    assert len(calls) - n0 == 2 * len(runs)
    return sorted(set(calls[n0:]))


def main() -> int:
    calls = install()
    if sys.argv[1:] == ["cameras"]:
        print("cameras:", " ".join(ut_cameras(calls)))
        return 0
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
