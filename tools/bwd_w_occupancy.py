"""Workgroups per CU that the HIP runtime admits for the one-wave-per-tile compositing backward (variant W), read with
hipOccupancyMaxActiveBlocksPerMultiprocessor for each kernel's handle in the library, at one or several dynamic LDS sizes.

    python tools/bwd_w_occupancy.py [--lib path/to/libgsplat_amd*.so] [--lds 13312 12288 ...]

The kernel handles are exported symbols of the library, so this works on any build of it (GSPLAT_AMD_LIB or --lib).
Prints one JSON line per (kernel, LDS size). Needs a GPU (the runtime answers for the current device)."""
import argparse
import ctypes
import json
import os

KERNELS = {
    "raster3d_bwd_w_kernel<1>": "_ZN3gsx21raster3d_bwd_w_kernelILi1EEEvNS_12Raster3DArgsE",
    "raster3d_bwd_w_kernel<2>": "_ZN3gsx21raster3d_bwd_w_kernelILi2EEEvNS_12Raster3DArgsE",
    "raster3d_bwd_w_kernel<3>": "_ZN3gsx21raster3d_bwd_w_kernelILi3EEEvNS_12Raster3DArgsE",
    "raster3d_bwd_w4_kernel": "_ZN3gsx22raster3d_bwd_w4_kernelENS_12Raster3DArgsE",
    "raster3d_bwd_w_abs_kernel<3>": "_ZN3gsx25raster3d_bwd_w_abs_kernelILi3EEEvNS_12Raster3DArgsE",
}


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--lib", default=os.environ.get("GSPLAT_AMD_LIB") or os.path.join(here, "..", "gsplat_amd", "csrc", "libgsplat_amd.so"))
    ap.add_argument("--lds", type=int, nargs="+", default=[12288, 13312])
    args = ap.parse_args()
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    fn = hip.hipOccupancyMaxActiveBlocksPerMultiprocessor
    fn.argtypes, fn.restype = [ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t], ctypes.c_int
    assert hip.hipSetDevice(0) == 0, "no GPU"
    for name, sym in KERNELS.items():
        handle = ctypes.c_char.in_dll(lib, sym)  # the host-side kernel handle (a variable of the library)
        for lds in args.lds:
            n = ctypes.c_int(-1)
            rc = fn(ctypes.byref(n), ctypes.addressof(handle), 64, lds)
            print(json.dumps({"lib": os.path.basename(args.lib), "kernel": name, "block": 64, "dynamic_lds": lds,
                              "workgroups_per_cu": n.value, "hip_error": rc}))


if __name__ == "__main__":
    main()
