"""ctypes binding of the C-ABI in include/gsplat_amd.h (libgsplat_amd.so).

This is the only place that crosses from Python into native code. There is NO CPU fallback:
if the shared library is missing the import fails loudly, and every call targets HIP kernels.

call(name, *args) takes the tensors themselves and marshals them: it holds them until the launch is queued and launches
on their device's current stream. query(name, *ints) is the host-only twin for the size / capability queries.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_ENV = "GSPLAT_AMD_LIB"  # optional override of the library path (e.g. a debug build)


class GsplatAmdError(RuntimeError):
    pass


def lib_path() -> str:
    return os.environ.get(_LIB_ENV) or os.path.join(_HERE, "csrc", "libgsplat_amd.so")


def _load() -> ctypes.CDLL:
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"gsplat_amd: native library not found at {path}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C gsplat_amd/csrc` "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback."
        )
    return ctypes.CDLL(path)


_lib = _load()

# signature table: p = pointer (device pointer or NULL), u = uint32, i = int, l = int64, f = float, d = double
_P, _U, _I, _L, _F = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_CODES = {"p": _P, "u": _U, "i": _I, "l": _L, "f": _F, "d": ctypes.c_double}

_HEADER = os.path.join(os.path.dirname(_HERE), "include", "gsplat_amd.h")


def _parse_header(path: str):
    """Derive the ctypes signatures from include/gsplat_amd.h so that the header stays the single
    source of truth. Returns {name: (restype_code, [arg codes])} for every `gsx_*` prototype."""
    import re

    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    sigs = {}
    for m in re.finditer(r"\b(int64_t|int|const char \*|void \*|void)\s*(gsx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        codes = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                if "*" in a:
                    codes.append("p")
                elif a.startswith("uint32_t"):
                    codes.append("u")
                elif a.startswith("int64_t"):
                    codes.append("l")
                elif a.startswith("float"):
                    codes.append("f")
                elif a.startswith("double"):
                    codes.append("d")
                elif a.startswith("int "):
                    codes.append("i")
                else:
                    raise ImportError(f"gsplat_amd: cannot parse argument '{a}' of {name} in {path}")
        sigs[name] = ({"int": "i", "int64_t": "l", "void *": "p", "void": "v"}.get(ret, "s"), codes)
    return sigs


_SIG_TABLE = os.path.join(_HERE, "csrc", "abi_signatures.json")  # written by write_signature_table() at build time


def _load_signatures():
    """The header is the source of truth in a checkout; an installed copy of the package (no ../include) reads the table
    that build() generated from it next to the library."""
    if os.path.exists(_HEADER):
        return _parse_header(_HEADER)
    if os.path.exists(_SIG_TABLE):
        with open(_SIG_TABLE) as f:
            return {k: (v[0], list(v[1])) for k, v in json.load(f).items()}
    raise ImportError(f"gsplat_amd: neither {_HEADER} nor {_SIG_TABLE} found; rebuild with __graft_entry__.build()")


def write_signature_table() -> str:
    with open(_SIG_TABLE, "w") as f:
        json.dump({k: [v[0], v[1]] for k, v in _parse_header(_HEADER).items()}, f)
    return _SIG_TABLE


SIGNATURES = _load_signatures()


def _bind():
    for name, (ret, codes) in SIGNATURES.items():
        fn = getattr(_lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = {"i": ctypes.c_int, "l": _L, "s": ctypes.c_char_p, "p": ctypes.c_void_p, "v": None}[ret]
        fn.argtypes = [_CODES[c] for c in codes]


_bind()

ABI_VERSION = _lib.gsx_version()
ARCH = _lib.gsx_arch().decode()


def exported_symbols():
    return list(SIGNATURES)


def _refuse_host_tensor(t: torch.Tensor) -> None:
    """The one device rule of this module: a tensor handed to native code that is not on a ROCm device ends here.
    tools/dry_run.py replaces this function to exercise the host side with CPU tensors."""
    raise GsplatAmdError("gsplat_amd kernels only run on a ROCm device (got a CPU tensor); there is no CPU fallback")


class strided:
    """Marks a call() argument as a view whose layout the caller has already checked (row-strided views): the device
    check stays, the contiguity check is skipped."""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        self.t = t


def ptr(t: Optional[torch.Tensor]):
    """Checked data_ptr() of a contiguous device tensor (None -> NULL), for code that drives the library directly. The
    caller keeps the tensor alive; the launch goes to the current device. Product code passes the tensor to call()."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise GsplatAmdError("gsplat_amd: tensor must be contiguous")
    return ptr_strided(t)


def ptr_strided(t: torch.Tensor):
    """The same for a tensor whose layout the caller has already checked (row-strided views)."""
    if not t.is_cuda:
        _refuse_host_tensor(t)
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream() -> int:
    """Raw hipStream_t of torch's current stream on the current device. The private fast accessor costs ~0.3 us;
    torch.cuda.current_stream() builds a Stream object through several Python layers (~9 us, measured), which adds
    up to ~0.1 ms per step over the ~12 C-ABI calls of a step."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_profile = None  # list of (entry point, start event, end event) while profiling is on
_profile_only = None  # optional set of entry points to record (None = all)


def torch_lib_path() -> str:
    """libgsplat_amd_torch.so, linked against the kernel library in use: GSPLAT_AMD_TORCH_LIB, else the one named after
    GSPLAT_AMD_LIB (tools/mkvariant.sh: libgsplat_amd_<name>.so -> libgsplat_amd_torch_<name>.so next to it), else the
    default build's."""
    if os.environ.get("GSPLAT_AMD_TORCH_LIB"):
        return os.environ["GSPLAT_AMD_TORCH_LIB"]
    d, base = os.path.split(lib_path())
    if not (base.startswith("libgsplat_amd") and base.endswith(".so")):
        raise ImportError(f"gsplat_amd: {_LIB_ENV}={lib_path()} does not follow the naming rule libgsplat_amd*.so; set "
                          "GSPLAT_AMD_TORCH_LIB to the libgsplat_amd_torch*.so linked against it")
    return os.path.join(d, "libgsplat_amd_torch" + base[len("libgsplat_amd"):])


def check_single_kernel_library() -> None:
    """After libgsplat_amd_torch.so is loaded: its compiled op bodies must call the same kernel library as this module (an
    A/B build with a torch library linked against another one would silently run the other's kernels)."""
    with open("/proc/self/maps") as f:
        libs = {os.path.realpath(ln.split(None, 5)[5].strip()) for ln in f if len(ln.split(None, 5)) == 6}
    kernels = {p for p in libs if os.path.basename(p).startswith("libgsplat_amd") and "_torch" not in os.path.basename(p)}
    if kernels != {os.path.realpath(lib_path())}:
        raise ImportError(f"gsplat_amd: {torch_lib_path()} is linked against {sorted(kernels - {os.path.realpath(lib_path())})}, "
                          f"not {lib_path()}; build the matching torch library (tools/mkvariant.sh, make SUFFIX=... torch)")


_torch_lib = None


def torch_lib() -> ctypes.CDLL:
    """libgsplat_amd_torch.so (csrc/torch_ops.cpp; gsplat_amd._ops loads it at import): the segment length of its compositing
    body, and the event-pair hooks of its op bodies, which call the C-ABI without passing through call() below."""
    global _torch_lib
    if _torch_lib is None:
        lib = ctypes.CDLL(torch_lib_path())
        lib.gsx_torch_seg_len.argtypes, lib.gsx_torch_seg_len.restype = [], ctypes.c_int64
        lib.gsx_torch_profile_begin.argtypes, lib.gsx_torch_profile_begin.restype = [ctypes.c_char_p], None
        lib.gsx_torch_profile_end.restype = ctypes.c_char_p
        _torch_lib = lib
    return _torch_lib


def profile_begin(only=None) -> None:
    """Start recording a HIP-event pair around gsx_* calls (events go on the stream the kernels are launched on:
    torch's current stream). `only` = iterable of entry-point names restricts the recording (bench.py times just the
    dominant kernels inside its timed region so that event bookkeeping does not perturb the step time)."""
    global _profile, _profile_only
    _profile = []
    _profile_only = None if only is None else frozenset(only)
    torch_lib().gsx_torch_profile_begin(" ".join(sorted(_profile_only or ())).encode())


def profile_end() -> dict:
    """Stop recording; returns {entry point: [ms per call, ...]} (synchronises the device)."""
    global _profile
    rec, _profile = _profile or [], None
    torch.cuda.synchronize()
    out = {}
    for name, a, b in rec:
        out.setdefault(name, []).append(a.elapsed_time(b))
    for line in torch_lib().gsx_torch_profile_end().decode().splitlines():  # the calls made by the compiled op bodies
        name, ms = line.split()
        out.setdefault(name, []).append(float(ms))
    return out


_SCALARS = frozenset((int, float, bool))


def call(name: str, *args) -> None:
    """Invoke a gsx_* entry point on the current stream of the device that owns its tensor arguments; raise on a non-zero
    return code. A torch.Tensor (contiguous, on a ROCm device), None (NULL) or strided(view) stands at a pointer
    position; anything else (int, float, ctypes array, raw address) passes through. `args` references the tensors until
    the entry point has returned, i.e. until the launch is queued, so a temporary (`x.contiguous()`) in the argument list
    is safe. Device guard: tensors on two devices are an error; if their device is not the current one it becomes current
    for the duration of the launch; without tensor arguments the launch goes to the current device."""
    codes = SIGNATURES[name][1]  # the last one is the stream
    if len(args) + 1 != len(codes):
        raise TypeError(f"{name}: takes {len(codes) - 1} arguments before the stream, got {len(args)}")
    raw, dev = list(args), -1
    for i, a in enumerate(args):
        if type(a) in _SCALARS:  # the one test most arguments take
            continue
        if a is not None:
            if type(a) is strided:
                a = a.t
            elif not isinstance(a, torch.Tensor):
                continue  # a ctypes array or pointer
            elif not a.is_contiguous():
                raise GsplatAmdError("gsplat_amd: tensor must be contiguous")
            if not a.is_cuda:
                _refuse_host_tensor(a)
            d = a.get_device()
            if d != dev:
                if dev >= 0 and d >= 0:
                    raise GsplatAmdError(f"{name}: tensor arguments on two devices (cuda:{dev} and cuda:{d}, argument {i})")
                dev = d
            raw[i] = a.data_ptr()
        if codes[i] != "p":
            raise TypeError(f"{name}: argument {i} is a '{codes[i]}' scalar, got {type(args[i]).__name__}")
    if dev >= 0 and dev != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return _launch(name, raw)
    _launch(name, raw)


def _launch(name: str, args) -> None:
    fn = getattr(_lib, name)
    if _profile is not None and (_profile_only is None or name in _profile_only):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args, current_stream())
        b.record()
        _profile.append((name, a, b))
    else:
        rc = fn(*args, current_stream())
    if rc != 0:
        msg = _lib.gsx_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{name}: {msg}")
        raise GsplatAmdError(f"{name} failed (code {rc}): {msg}")


def query(name: str, *ints) -> int:
    """A size / capability query of the library (gsx_*_workspace_bytes, gsx_*_blocks, ...): host-only, no stream."""
    return int(getattr(_lib, name)(*ints))


# the workspace sizes that tests/test_gpu_sort_edges.py and tests/test_gpu_ops.py ask for by these names
def scan_workspace_bytes(n: int) -> int:
    return query("gsx_scan_workspace_bytes", n)


def sort_workspace_bytes(n: int) -> int:
    return query("gsx_sort_pairs_workspace_bytes", n)


def tile_sort_workspace_bytes(n: int, n_images: int, tile_w: int, tile_h: int) -> int:
    return query("gsx_isect_tile_sort_workspace_bytes", n, n_images, tile_w, tile_h)


def tile_sort_supported(n_images: int, tile_w: int, tile_h: int) -> bool:
    return bool(_lib.gsx_isect_tile_sort_supported(n_images, tile_w, tile_h))


def isect_fused_supported(n_images: int, tile_w: int, tile_h: int, packed: bool) -> bool:
    return bool(_lib.gsx_isect_fused_supported(n_images, tile_w, tile_h, int(packed)))


class IsectPathMemory:
    """The retry notes of the tile-owner-major intersection path, owned by ONE caller (include/gsplat_amd.h:
    gsx_isect_path_memory_*). Which intersection kernel runs depends on recent history (a clustered scene that was sent back is
    not tried again for 63 calls); `with memory:` makes that history this object's for the calls inside, on this thread - a
    trainer and a viewer, or two trainers, each hold their own. Without one, a thread uses a private default."""

    def __init__(self):
        self._h = _lib.gsx_isect_path_memory_create()
        if not self._h:
            raise MemoryError("gsx_isect_path_memory_create failed")
        self._prev = []

    def __enter__(self):
        self._prev.append(_lib.gsx_isect_path_memory_use(self._h))
        return self

    def __exit__(self, *exc):
        _lib.gsx_isect_path_memory_use(self._prev.pop())
        return False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.gsx_isect_path_memory_destroy(h)


def copy_column_groups(groups, rows: int) -> None:
    """One launch of gsx_copy_column_groups. `groups`: list of (src_ptr, src_row_stride, dst_ptr, dst_row_stride, width)
    in 32-bit words (device pointers as ints)."""
    n = len(groups)
    src = (ctypes.c_void_p * n)(*[g[0] for g in groups])
    dst = (ctypes.c_void_p * n)(*[g[2] for g in groups])
    ss = (ctypes.c_uint32 * n)(*[g[1] for g in groups])
    ds = (ctypes.c_uint32 * n)(*[g[3] for g in groups])
    w = (ctypes.c_uint32 * n)(*[g[4] for g in groups])
    call("gsx_copy_column_groups", n, src, ss, dst, ds, w, rows)


def copy_column_groups_mapped(groups, seg_rows, seg_n, map_dst: bool) -> None:
    """gsx_copy_column_groups_mapped: `groups` as in copy_column_groups; seg_rows[k] = C_local * N_k, seg_n[k] = N_k."""
    n, m = len(groups), len(seg_rows)
    src = (ctypes.c_void_p * n)(*[g[0] for g in groups])
    dst = (ctypes.c_void_p * n)(*[g[2] for g in groups])
    ss = (ctypes.c_uint32 * n)(*[g[1] for g in groups])
    ds = (ctypes.c_uint32 * n)(*[g[3] for g in groups])
    w = (ctypes.c_uint32 * n)(*[g[4] for g in groups])
    sr = (ctypes.c_int64 * m)(*[int(v) for v in seg_rows])
    sn = (ctypes.c_int64 * m)(*[int(v) for v in seg_n])
    call("gsx_copy_column_groups_mapped", n, src, ss, dst, ds, w, m, sr, sn, int(bool(map_dst)))


def copy_message_columns(msg_ptr: int, msg_stride: int, rows: int, groups, to_message: bool, seg_rows=None, seg_n=None) -> None:
    """gsx_copy_message_columns. `groups`: list of (column, width, field_ptr, field_row_stride) in 32-bit words."""
    n = len(groups)
    cols = (ctypes.c_uint32 * n)(*[g[0] for g in groups])
    w = (ctypes.c_uint32 * n)(*[g[1] for g in groups])
    fields = (ctypes.c_void_p * n)(*[g[2] for g in groups])
    fs = (ctypes.c_uint32 * n)(*[g[3] for g in groups])
    m = 0 if seg_rows is None else len(seg_rows)
    sr = (ctypes.c_int64 * max(m, 1))(*([int(v) for v in seg_rows] if m else [0]))
    sn = (ctypes.c_int64 * max(m, 1))(*([int(v) for v in seg_n] if m else [0]))
    call("gsx_copy_message_columns", ctypes.c_void_p(msg_ptr), msg_stride, rows, n, cols, w, fields, fs, int(bool(to_message)), m,
         sr, sn)


def sort_pairs(keys, vals, keys_alt, vals_alt, n: int, end_bit: int, workspace) -> bool:
    """Returns True when the sorted data ended up in the alt buffers."""
    flag = ctypes.c_int(0)
    call("gsx_sort_pairs", keys, vals, keys_alt, vals_alt, n, end_bit, workspace, workspace.numel() * workspace.element_size(),
         ctypes.addressof(flag))
    return bool(flag.value)
