"""CPU: what the C-ABI entry points of the projection, compositing and 3DGUT families answer to bad or empty arguments.

Every case leaves its entry through a GSX_REQUIRE or through an early return that precedes the first HIP runtime call, so the
test runs on a machine without a GPU. The library is called directly (gsplat_amd._cabi._lib): _cabi.call would ask torch for
the current device. A pointer that a case does not name is NULL; P is a non-null address that is never read. The expected
codes and texts are literals: the entry's own name, the wording and the ORDER of the checks are part of the published
behaviour (gsplat_amd/_ops.py turns GSX_ERR_ARG into ValueError with this text).
"""
import os
import re

import pytest

from gsplat_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG = 0, -1
P = 64  # a non-null address that is never read


def _parameter_names():
    """{entry point: [parameter names]} from include/gsplat_amd.h, in declaration order."""
    text = open(os.path.join(ROOT, "include", "gsplat_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gsx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = [] if args in ("", "void") else [re.findall(r"\w+", a)[-1] for a in args.split(",")]
    return out


_NAMES = _parameter_names()


def _call(entry, **kw):
    """(return code, gsx_last_error() text) of `entry` with every argument NULL / 0 except the named ones."""
    names, codes = _NAMES[entry], _cabi.SIGNATURES[entry][1]
    assert len(names) == len(codes)
    unknown = set(kw) - set(names)
    assert not unknown, f"{entry} has no parameter {sorted(unknown)}"
    args = [kw.get(n, None if c == "p" else 0) for n, c in zip(names, codes)]
    rc = getattr(_cabi._lib, entry)(*args)
    return rc, _cabi._lib.gsx_last_error().decode()


def _ptrs(*names):
    return {n: P for n in names}


def _drop(kw, name):
    """`kw` with the pointer `name` NULL again."""
    assert kw.pop(name) == P
    return kw


def _check(entry, kw, rc, msg):
    got_rc, got_msg = _call(entry, **kw)
    assert got_rc == rc, (entry, kw, got_rc, got_msg)
    if rc != OK:  # a successful call leaves the previous message in place
        assert got_msg == msg, (entry, kw)


# ---- EWA projection (projection.hip) ----------------------------------------------------------------------------------------
ONE = dict(B=1, C=1, N=1)
MVK = _ptrs("means", "viewmats", "Ks")
GEOM = dict(MVK, covars=P)  # passes the checks shared by the projection entries (pinhole = camera model 0)
EWA_FWD_OUT = _ptrs("radii", "means2d", "depths", "conics")
EWA_BWD_IN = _ptrs("radii", "conics", "v_means2d", "v_conics")
EWA_PACKED_BWD_IN = _ptrs("batch_ids", "camera_ids", "gaussian_ids", "conics", "v_means2d", "v_conics")
TOO_MANY = (1 << 31) - 256


def _common_cases(entry, base):
    """The checks shared by the EWA projection entries, reached with `base` (sizes and whatever precedes them)."""
    return [
        (entry, dict(base), ERR_ARG, f"{entry}: null means/viewmats/Ks"),
        (entry, dict(base, **_ptrs("means", "viewmats")), ERR_ARG, f"{entry}: null means/viewmats/Ks"),
        (entry, dict(base, **MVK), ERR_ARG, f"{entry}: need covars or (quats and scales)"),
        (entry, dict(base, **MVK, quats=P), ERR_ARG, f"{entry}: need covars or (quats and scales)"),
        (entry, dict(base, **GEOM, camera_model=3), ERR_ARG,
         f"{entry}: unsupported camera model 3 (pinhole/ortho/fisheye only)"),
        (entry, dict(base, **MVK, quats=P, scales=P, camera_model=-1), ERR_ARG,
         f"{entry}: unsupported camera model -1 (pinhole/ortho/fisheye only)"),
    ]


def _stride_cases(entry, base):
    return [
        (entry, dict(base, v_means2d_stride=1, v_conics_stride=3), ERR_ARG, f"{entry}: row strides must be >= 2 / >= 3"),
        (entry, dict(base, v_means2d_stride=2, v_conics_stride=2), ERR_ARG, f"{entry}: row strides must be >= 2 / >= 3"),
        (entry, dict(base), ERR_ARG, f"{entry}: row strides must be >= 2 / >= 3"),
    ]


EWA = []
for _e in ("gsx_project_ewa_fwd", "gsx_project_ewa_packed_count"):
    EWA += [(_e, dict(B=0, C=1, N=1), OK, ""), (_e, dict(B=1, C=0, N=1), OK, ""), (_e, dict(B=1, C=1, N=0), OK, "")]
    EWA += _common_cases(_e, ONE)
    EWA += [(_e, dict(ONE, **GEOM), ERR_ARG, f"{_e}: null output")]
EWA += [("gsx_project_ewa_fwd", dict(ONE, **GEOM, **_ptrs("radii", "means2d", "depths")), ERR_ARG,
         "gsx_project_ewa_fwd: null output")]

_e = "gsx_project_ewa_packed_write"
EWA += [(_e, dict(B=1, C=1, N=0), ERR_ARG, f"{_e}: null indptr"), (_e, dict(ONE), ERR_ARG, f"{_e}: null indptr")]
EWA += _common_cases(_e, dict(ONE, indptr=P))
EWA += [
    (_e, dict(ONE, **GEOM, indptr=P), ERR_ARG, f"{_e}: null row_offsets"),
    (_e, dict(ONE, **GEOM, indptr=P, row_offsets=P, nnz=1), ERR_ARG, f"{_e}: null output"),
    (_e, dict(ONE, **GEOM, indptr=P, row_offsets=P, nnz=1, **_ptrs("batch_ids", "camera_ids", "gaussian_ids", "radii", "means2d", "depths")),
     ERR_ARG, f"{_e}: null output"),
]

_e = "gsx_project_ewa_packed_count_blocks"
_bb = _ptrs("block_counts", "block_offsets")
EWA += [
    (_e, dict(B=1, C=1, N=TOO_MANY), ERR_ARG, f"{_e}: 2147483392 (image, Gaussian) pairs exceed int32 offsets"),
    (_e, dict(B=2, C=1, N=TOO_MANY, **_bb), ERR_ARG, f"{_e}: 4294966784 (image, Gaussian) pairs exceed int32 offsets"),
    (_e, dict(B=1, C=1, N=0), ERR_ARG, f"{_e}: null block buffer"),
    (_e, dict(ONE, block_counts=P), ERR_ARG, f"{_e}: null block buffer"),
]
EWA += _common_cases(_e, dict(ONE, **_bb))

_e = "gsx_project_ewa_packed_write_blocks"
_ib = _ptrs("indptr", "block_offsets")
EWA += [
    (_e, dict(B=1, C=1, N=0), ERR_ARG, f"{_e}: null indptr / block offsets"),
    (_e, dict(ONE, indptr=P), ERR_ARG, f"{_e}: null indptr / block offsets"),
    (_e, dict(B=1, C=1, N=TOO_MANY, **_ib), ERR_ARG, f"{_e}: too many (image, Gaussian) pairs"),
]
EWA += _common_cases(_e, dict(ONE, **_ib))
EWA += [(_e, dict(ONE, **GEOM, **_ib), ERR_ARG, f"{_e}: null output"),
        (_e, _drop(dict(ONE, **GEOM, **_ib, **_ptrs("batch_ids", "camera_ids", "gaussian_ids"), **EWA_FWD_OUT), "radii"), ERR_ARG,
         f"{_e}: null output")]

_e = "gsx_project_ewa_bwd"
EWA += [(_e, dict(B=0, C=1, N=1), OK, ""), (_e, dict(B=1, C=1, N=0), OK, ""), (_e, dict(B=1, C=0, N=1), OK, "")]
EWA += _common_cases(_e, ONE)
EWA += [(_e, dict(ONE, **GEOM), ERR_ARG, f"{_e}: null input"),
        (_e, _drop(dict(ONE, **GEOM, **EWA_BWD_IN), "radii"), ERR_ARG, f"{_e}: null input")]
EWA += _stride_cases(_e, dict(ONE, **GEOM, **EWA_BWD_IN))

_e = "gsx_project_ewa_bwd_opac"
_vo = dict(v_opacities=P, v_view_opacities=P, v_view_opacities_stride=1)
EWA += [
    (_e, dict(B=0, C=1, N=1), OK, ""), (_e, dict(B=1, C=1, N=0), OK, ""), (_e, dict(B=1, C=0, N=0), OK, ""),
    (_e, dict(ONE), ERR_ARG, f"{_e}: null v_opacities"),
    (_e, dict(B=1, C=0, N=1), ERR_ARG, f"{_e}: null v_opacities"),  # checked before the C == 0 fill
    (_e, dict(ONE, **GEOM, **EWA_BWD_IN, v_view_opacities=P, v_view_opacities_stride=1), ERR_ARG, f"{_e}: null v_opacities"),
    (_e, dict(ONE, v_opacities=P), ERR_ARG, f"{_e}: null opacity cotangent"),
    (_e, dict(ONE, **GEOM, v_opacities=P, v_view_opacities=P), ERR_ARG, f"{_e}: null opacity cotangent"),  # stride 0
]
EWA += _common_cases(_e, dict(ONE, **_vo))
EWA += [(_e, dict(ONE, **GEOM, **_vo), ERR_ARG, f"{_e}: null input")]
EWA += _stride_cases(_e, dict(ONE, **GEOM, **EWA_BWD_IN, **_vo))

for _e in ("gsx_project_ewa_packed_bwd", "gsx_project_ewa_packed_bwd_rows"):
    EWA += [(_e, dict(ONE, nnz=0), OK, ""), (_e, dict(ONE, nnz=-1), OK, ""), (_e, dict(nnz=0), OK, "")]
    EWA += _common_cases(_e, dict(ONE, nnz=1))
    EWA += [(_e, dict(ONE, nnz=1, **GEOM), ERR_ARG, f"{_e}: null input"),
            (_e, _drop(dict(ONE, nnz=1, **GEOM, **EWA_PACKED_BWD_IN), "camera_ids"), ERR_ARG, f"{_e}: null input")]
    EWA += _stride_cases(_e, dict(ONE, nnz=1, **GEOM, **EWA_PACKED_BWD_IN))

_e = "gsx_project_ewa_packed_bwd_opac"
EWA += [
    (_e, dict(B=0, C=1, N=1, nnz=1), OK, ""), (_e, dict(B=1, C=1, N=0, nnz=1), OK, ""), (_e, dict(nnz=0), OK, ""),
    (_e, dict(ONE, nnz=1), ERR_ARG, f"{_e}: null v_opacities"),
    (_e, dict(ONE, nnz=0), ERR_ARG, f"{_e}: null v_opacities"),  # checked before the nnz <= 0 fill
    (_e, dict(ONE, nnz=1, v_opacities=P), ERR_ARG, f"{_e}: null opacity cotangent"),
    (_e, dict(ONE, nnz=1, **GEOM, v_opacities=P, v_view_opacities=P), ERR_ARG, f"{_e}: null opacity cotangent"),  # stride 0
]
EWA += _common_cases(_e, dict(ONE, nnz=1, **_vo))
EWA += [(_e, dict(ONE, nnz=1, **GEOM, **_vo), ERR_ARG, f"{_e}: null input"),
        (_e, _drop(dict(ONE, nnz=1, **GEOM, **_vo, **EWA_PACKED_BWD_IN), "v_conics"), ERR_ARG, f"{_e}: null input")]
EWA += _stride_cases(_e, dict(ONE, nnz=1, **GEOM, **_vo, **EWA_PACKED_BWD_IN))

# ---- 2DGS projection (projection2d.hip) -------------------------------------------------------------------------------------
IN2 = _ptrs("means", "quats", "scales", "viewmats", "Ks")
BWD2_IN = _ptrs("radii", "ray_transforms", "v_means2d", "v_ray_transforms", "v_normals")
PACKED_BWD2_IN = _ptrs("batch_ids", "camera_ids", "gaussian_ids", "ray_transforms", "v_means2d", "v_ray_transforms", "v_normals")
OUT2 = _ptrs("v_means", "v_quats", "v_scales")

P2D = []
for _e in ("gsx_project_2dgs_fwd", "gsx_project_2dgs_packed_count", "gsx_project_2dgs_packed_write"):
    P2D += [(_e, dict(B=1, C=1, N=0), OK, ""), (_e, dict(B=0, C=1, N=1), OK, ""),
            (_e, dict(ONE), ERR_ARG, f"{_e}: null input"),
            (_e, _drop(dict(ONE, **IN2), "Ks"), ERR_ARG, f"{_e}: null input")]
P2D += [("gsx_project_2dgs_fwd", dict(ONE, **IN2), ERR_ARG, "gsx_project_2dgs_fwd: null output"),
        ("gsx_project_2dgs_packed_count", dict(ONE, **IN2), ERR_ARG, "gsx_project_2dgs_packed_count: null output"),
        ("gsx_project_2dgs_packed_write", dict(ONE, **IN2, indptr=P), ERR_ARG,
         "gsx_project_2dgs_packed_write: null row_offsets/indptr"),
        ("gsx_project_2dgs_packed_write", dict(ONE, **IN2, indptr=P, row_offsets=P, nnz=1), ERR_ARG,
         "gsx_project_2dgs_packed_write: null output")]

_e = "gsx_project_2dgs_bwd"
P2D += [
    (_e, dict(B=1, C=1, N=0), OK, ""), (_e, dict(B=0, C=1, N=1), OK, ""),
    (_e, dict(ONE), ERR_ARG, f"{_e}: null input"),
    (_e, dict(B=1, C=0, N=1), ERR_ARG, f"{_e}: null input"),
    (_e, dict(ONE, **IN2), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(ONE, **IN2, **BWD2_IN), "v_normals"), ERR_ARG, f"{_e}: null input"),
    (_e, dict(ONE, **IN2, **BWD2_IN), ERR_ARG, f"{_e}: null output"),
    (_e, dict(B=1, C=0, N=1, **IN2), ERR_ARG, f"{_e}: null output"),  # no views: the per-view inputs may be null
    (_e, _drop(dict(ONE, **IN2, **BWD2_IN, **OUT2), "v_scales"), ERR_ARG, f"{_e}: null output"),
]
_e = "gsx_project_2dgs_bwd_opac"
_vo2 = dict(v_view_opacities=P, v_view_opacities_stride=1)
P2D += [
    (_e, dict(B=1, C=1, N=0), OK, ""), (_e, dict(B=0, C=1, N=1), OK, ""),
    (_e, dict(ONE), ERR_ARG, f"{_e}: null v_opacities"),
    (_e, dict(ONE, **IN2, **BWD2_IN, **OUT2, **_vo2), ERR_ARG, f"{_e}: null v_opacities"),
    (_e, dict(ONE, v_opacities=P), ERR_ARG, f"{_e}: null input"),
    (_e, dict(ONE, **IN2, **BWD2_IN, v_opacities=P), ERR_ARG, f"{_e}: null input"),
    (_e, dict(ONE, **IN2, **BWD2_IN, v_opacities=P, v_view_opacities=P), ERR_ARG, f"{_e}: null input"),  # stride 0
    (_e, dict(ONE, **IN2, **BWD2_IN, **_vo2, v_opacities=P), ERR_ARG, f"{_e}: null output"),
    (_e, dict(B=1, C=0, N=1, **IN2, v_opacities=P), ERR_ARG, f"{_e}: null output"),
]
for _e in ("gsx_project_2dgs_packed_bwd", "gsx_project_2dgs_packed_bwd_rows"):
    P2D += [
        (_e, dict(ONE, nnz=0), OK, ""), (_e, dict(nnz=0), OK, ""),
        (_e, dict(ONE, nnz=1), ERR_ARG, f"{_e}: null input"),
        (_e, dict(ONE, nnz=-1), ERR_ARG, f"{_e}: null input"),  # only nnz == 0 returns early
        (_e, dict(ONE, nnz=1, **IN2), ERR_ARG, f"{_e}: null input"),
        (_e, _drop(dict(ONE, nnz=1, **IN2, **PACKED_BWD2_IN), "gaussian_ids"), ERR_ARG, f"{_e}: null input"),
        (_e, dict(ONE, nnz=1, **IN2, **PACKED_BWD2_IN), ERR_ARG, f"{_e}: null output"),
        (_e, _drop(dict(ONE, nnz=1, **IN2, **PACKED_BWD2_IN, **OUT2), "v_means"), ERR_ARG, f"{_e}: null output"),
    ]

# ---- 3DGS compositing (raster3d_fwd.hip, raster3d_bwd.hip, raster3d_seg.hip) ------------------------------------------------
T16 = dict(tile_size=16, cdim=3)
GRID = dict(n_images=1, tile_w=1, tile_h=1, width=16, height=16)
R3_IN = _ptrs("means2d", "conics", "colors", "opacities", "flatten_ids")
R3_OUT = _ptrs("render_colors", "render_alphas", "last_ids")
R3_BWD_IN = dict(R3_IN, **_ptrs("render_alphas", "last_ids", "v_render_colors", "isect_offsets"))
R3_SPARSE = _ptrs("active_tiles", "tile_offsets", "tile_pixel_mask", "tile_pixel_cumsum", "pixel_map")


def _tile_cdim_cases(entry, name, zero_cdim=None):
    zero_cdim = zero_cdim or f"{name}: channels must be >= 1"
    return [
        (entry, dict(tile_size=0, cdim=3), ERR_ARG, f"{name}: tile_size must be in [1,16], got 0"),
        (entry, dict(tile_size=17, cdim=3), ERR_ARG, f"{name}: tile_size must be in [1,16], got 17"),
        (entry, dict(tile_size=17, cdim=0), ERR_ARG, f"{name}: tile_size must be in [1,16], got 17"),
        (entry, dict(tile_size=16, cdim=0), ERR_ARG, zero_cdim),
    ]


R3D = []
_e = "gsx_raster3d_fwd"
R3D += _tile_cdim_cases(_e, _e)
R3D += [
    (_e, dict(T16), ERR_ARG, f"{_e}: null output"),
    (_e, _drop(dict(T16, **R3_OUT), "last_ids"), ERR_ARG, f"{_e}: null output"),
    (_e, dict(T16, **GRID, **R3_OUT, n_isects=1), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(T16, **GRID, **R3_OUT, **R3_IN, n_isects=1), "opacities"), ERR_ARG, f"{_e}: null input"),
    (_e, dict(T16, **GRID, **R3_OUT), ERR_ARG, f"{_e}: null isect_offsets"),
    (_e, dict(T16, **GRID, **R3_OUT, **R3_IN, n_isects=1), ERR_ARG, f"{_e}: null isect_offsets"),
    (_e, dict(T16, **R3_OUT), OK, ""),  # no images: no workgroup to launch
    (_e, dict(T16, **R3_OUT, n_images=1, tile_w=0, tile_h=1), OK, ""),
    (_e, dict(tile_size=8, cdim=40, **R3_OUT), OK, ""),  # two channel chunks, neither launches
]
_e = "gsx_raster3d_sparse_fwd"
R3D += _tile_cdim_cases(_e, _e)
R3D += [
    (_e, dict(T16), OK, ""),  # n_active == 0
    (_e, dict(T16, **GRID, n_isects=1, words_per_tile=4), OK, ""),
    (_e, dict(T16, n_active=1, words_per_tile=3), ERR_ARG, f"{_e}: pixel mask too narrow"),
    (_e, dict(tile_size=9, cdim=3, n_active=1, words_per_tile=1), ERR_ARG, f"{_e}: pixel mask too narrow"),
    (_e, dict(T16, n_active=1, words_per_tile=4), ERR_ARG, f"{_e}: null layout / output"),
    (_e, _drop(dict(T16, n_active=1, words_per_tile=4, **R3_SPARSE, **R3_OUT), "pixel_map"), ERR_ARG, f"{_e}: null layout / output"),
    (_e, dict(T16, n_active=1, words_per_tile=4, **R3_SPARSE), ERR_ARG, f"{_e}: null layout / output"),
    (_e, dict(tile_size=8, cdim=3, n_active=1, words_per_tile=1, **R3_SPARSE, **R3_OUT, n_isects=1), ERR_ARG, f"{_e}: null input"),
]
# the three spellings of the compositing backward share their checks and name themselves gsx_raster3d_bwd in them
for _e in ("gsx_raster3d_bwd", "gsx_raster3d_bwd_ws", "gsx_raster3d_bwd_fill"):
    _n = "gsx_raster3d_bwd"
    R3D += _tile_cdim_cases(_e, _n)
    R3D += [
        (_e, dict(T16), OK, ""),  # n_isects == 0, no rows to fill
        (_e, dict(T16, **GRID, v_rows=P, row_stride=9), OK, ""),
        (_e, dict(T16, n_isects=1), ERR_ARG, f"{_n}: null gradient output"),
        (_e, dict(T16, n_isects=1, **R3_BWD_IN, row_stride=9), ERR_ARG, f"{_n}: null gradient output"),
        (_e, dict(T16, n_isects=1, v_rows=P, row_stride=8), ERR_ARG, f"{_n}: row_stride 8 too small for 6 + 3 channels"),
        (_e, dict(T16, n_isects=1, v_rows=P, row_stride=10, has_abs=1), ERR_ARG,
         f"{_n}: row_stride 10 too small for 6 + 2 + 3 channels"),
        (_e, dict(tile_size=16, cdim=40, n_isects=1, v_rows=P, row_stride=45), ERR_ARG,
         f"{_n}: row_stride 45 too small for 6 + 40 channels"),
        (_e, dict(T16, n_isects=1, v_rows=P, row_stride=9), ERR_ARG, f"{_n}: null input"),
        (_e, _drop(dict(T16, n_isects=1, v_rows=P, row_stride=11, has_abs=1, **R3_BWD_IN), "isect_offsets"), ERR_ARG, f"{_n}: null input"),
        (_e, _drop(dict(T16, n_isects=1, v_rows=P, row_stride=9, **R3_BWD_IN), "v_render_colors"), ERR_ARG, f"{_n}: null input"),
    ]
for _e in ("gsx_raster3d_bwd_ws", "gsx_raster3d_bwd_fill"):
    R3D += [
        (_e, dict(T16, **GRID, n_isects=1, v_rows=P, row_stride=9, **R3_BWD_IN, v_colors_pixel_stride=0, v_colors_channel_stride=-1),
         ERR_ARG, "gsx_raster3d_bwd_ws: negative channel stride"),
        (_e, dict(T16, n_isects=1, v_rows=P, row_stride=9, v_colors_pixel_stride=0, v_colors_channel_stride=-1), ERR_ARG,
         "gsx_raster3d_bwd: null input"),  # the layout of the cotangent is looked at after the pointers
    ]
R3D += [("gsx_raster3d_bwd_fill", dict(T16, v_rows_to_fill=-5, v_rows=P, row_stride=9), OK, ""),  # nothing to fill
        ("gsx_raster3d_bwd_fill", dict(T16, v_rows_to_fill=7, row_stride=9), OK, "")]  # no rows to fill them into

_e = "gsx_raster3d_sparse_bwd"
R3D += _tile_cdim_cases(_e, _e)
R3D += [
    (_e, dict(T16), OK, ""),  # n_isects == 0
    (_e, dict(T16, n_active=1, words_per_tile=1), OK, ""),
    (_e, dict(T16, n_isects=1), ERR_ARG, f"{_e}: null gradient output"),
    (_e, dict(T16, n_isects=1, v_rows=P, row_stride=8), ERR_ARG, f"{_e}: row_stride 8 too small"),
    (_e, dict(T16, n_isects=1, v_rows=P, row_stride=10, has_abs=1), ERR_ARG, f"{_e}: row_stride 10 too small"),
    (_e, dict(T16, n_isects=1, v_rows=P, row_stride=9), OK, ""),  # n_active == 0, after the gradient rows were checked
    (_e, dict(T16, n_isects=1, v_rows=P, row_stride=11, has_abs=1, words_per_tile=1), OK, ""),
    (_e, dict(T16, n_isects=1, v_rows=P, row_stride=9, n_active=1, words_per_tile=3), ERR_ARG, f"{_e}: pixel mask too narrow"),
    (_e, dict(T16, n_isects=1, v_rows=P, row_stride=9, n_active=1, words_per_tile=4), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(T16, n_isects=1, v_rows=P, row_stride=9, n_active=1, words_per_tile=4, **R3_SPARSE,
                    **_drop(dict(R3_BWD_IN), "isect_offsets")), "last_ids"),
     ERR_ARG, f"{_e}: null input"),
]

_e = "gsx_raster3d_fwd_seg"
SEG = dict(T16, seg_len=256)
R3D += _tile_cdim_cases(_e, _e)
R3D += [
    (_e, dict(T16), ERR_ARG, f"{_e}: seg_len must be >= 256 (one staged batch), got 0"),
    (_e, dict(T16, seg_len=255, **R3_OUT), ERR_ARG, f"{_e}: seg_len must be >= 256 (one staged batch), got 255"),
    (_e, dict(SEG), ERR_ARG, f"{_e}: null output"),
    (_e, dict(SEG, **GRID, **R3_OUT, n_isects=1), ERR_ARG, f"{_e}: null input"),
    (_e, dict(SEG, **GRID, **R3_OUT), ERR_ARG, f"{_e}: null isect_offsets"),
    (_e, dict(SEG, **R3_OUT), OK, ""),  # no tiles
    (_e, dict(SEG, **R3_OUT, **R3_IN, n_isects=5, n_images=2, tile_w=3, tile_h=0), OK, ""),
]
# both spellings of the segmented backward name themselves gsx_raster3d_bwd_seg
for _e in ("gsx_raster3d_bwd_seg", "gsx_raster3d_bwd_seg_reuse"):
    _n = "gsx_raster3d_bwd_seg"
    _m = f"{_n}: needs 16 x 16 tiles and <= 4 channels (got tile %u, %u channels): use gsx_raster3d_bwd"
    R3D += [
        (_e, dict(tile_size=8, cdim=3, seg_len=256), ERR_ARG, _m % (8, 3)),
        (_e, dict(tile_size=16, cdim=5, seg_len=256), ERR_ARG, _m % (16, 5)),
        (_e, dict(tile_size=16, cdim=0, seg_len=256), ERR_ARG, _m % (16, 0)),
        (_e, dict(tile_size=17, cdim=3), ERR_ARG, _m % (17, 3)),
        (_e, dict(T16, seg_len=255), ERR_ARG, f"{_n}: seg_len must be >= 256, got 255"),
        (_e, dict(SEG), OK, ""),  # n_isects == 0
        (_e, dict(SEG, n_isects=1), ERR_ARG, f"{_n}: gradient rows missing / too narrow"),
        (_e, dict(SEG, n_isects=1, v_rows=P, row_stride=8), ERR_ARG, f"{_n}: gradient rows missing / too narrow"),
        (_e, dict(SEG, n_isects=1, v_rows=P, row_stride=9), ERR_ARG, f"{_n}: null input"),
        (_e, _drop(dict(SEG, n_isects=1, v_rows=P, row_stride=9, **R3_BWD_IN), "means2d"), ERR_ARG, f"{_n}: null input"),
        (_e, dict(SEG, n_isects=1, v_rows=P, row_stride=9, **R3_BWD_IN), OK, ""),  # no tiles
    ]

# ---- 2DGS compositing (raster2d.hip) ----------------------------------------------------------------------------------------
R2_IN = _ptrs("means2d", "ray_transforms", "colors", "opacities", "normals", "flatten_ids")
R2_OUT = _ptrs("render_colors", "render_alphas", "render_normals", "render_distort", "render_median", "last_ids", "median_ids")
R2_BWD_IN = dict(R2_IN, **_ptrs("render_colors", "render_alphas", "last_ids", "median_ids", "v_render_colors", "isect_offsets"))


def _cdim2_cases(entry, name):
    return _tile_cdim_cases(entry, name, f"{name}: unsupported number of channels 0 (1..32)") + [
        (entry, dict(tile_size=16, cdim=33), ERR_ARG, f"{name}: unsupported number of channels 33 (1..32)")]


R2D = []
_e = "gsx_raster2d_fwd"
R2D += _cdim2_cases(_e, _e)
R2D += [
    (_e, dict(T16), ERR_ARG, f"{_e}: null output"),
    (_e, _drop(dict(T16, **R2_OUT), "render_median"), ERR_ARG, f"{_e}: null output"),
    (_e, dict(T16, **GRID, **R2_OUT, n_isects=1), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(T16, **GRID, **R2_OUT, **R2_IN, n_isects=1), "normals"), ERR_ARG, f"{_e}: null input"),
    (_e, dict(T16, **GRID, **R2_OUT), ERR_ARG, f"{_e}: null isect_offsets"),
    (_e, dict(T16, **R2_OUT), OK, ""),  # no tiles
    (_e, dict(tile_size=8, cdim=32, **R2_OUT, **R2_IN, n_isects=3), OK, ""),
]
for _e in ("gsx_raster2d_bwd", "gsx_raster2d_bwd_ws", "gsx_raster2d_bwd_fill"):
    _n = "gsx_raster2d_bwd"
    R2D += _cdim2_cases(_e, _n)
    R2D += [
        (_e, dict(T16), OK, ""),  # n_isects == 0, no rows to fill
        (_e, dict(T16, **GRID, v_rows=P, row_stride=20), OK, ""),
        (_e, dict(T16, n_isects=1), ERR_ARG, f"{_n}: null gradient output"),
        (_e, dict(T16, n_isects=1, v_rows=P, row_stride=19), ERR_ARG, f"{_n}: row_stride 19 too small"),
        (_e, dict(T16, n_isects=1, v_rows=P, row_stride=21, has_abs=1), ERR_ARG, f"{_n}: row_stride 21 too small"),
        (_e, dict(T16, n_isects=1, v_rows=P, row_stride=20), ERR_ARG, f"{_n}: null input"),
        (_e, _drop(dict(T16, n_isects=1, v_rows=P, row_stride=22, has_abs=1, **R2_BWD_IN), "median_ids"), ERR_ARG, f"{_n}: null input"),
    ]
R2D += [("gsx_raster2d_bwd_fill", dict(T16, v_rows_to_fill=-5, v_rows=P, row_stride=20), OK, ""),
        ("gsx_raster2d_bwd_fill", dict(T16, v_rows_to_fill=7, row_stride=20), OK, "")]


# ---- 3DGUT: unscented projection and ray generation (projection_ut.hip), from-world compositing (raster_world.hip) -----------
# A case that names `ftheta` or `ext` must fail a check: past the checks the entry reads those HOST records.
UT_IN = _ptrs("means", "quats", "scales", "viewmats0", "Ks")
UT_OUT = _ptrs("radii", "means2d", "depths", "conics")
UT_OK = dict(ONE, **UT_IN, **UT_OUT, rs_type=4)  # passes everything up to the sigma-point weights (ut_alpha = 0)
_rs = "rolling shutter type %d (0 .. 3 rolling, 4 global)"
_models = "camera model %d is not built (pinhole = 0, orthographic = 1, fisheye = 2, f-theta = 3, lidar = 4 are)"
_ortho = "the orthographic model takes no distortion coefficients"
_fisheye = "the fisheye model needs fisheye_max_angle and takes radial coefficients only"
_ftheta = "the f-theta model needs its parameter record and takes no other coefficients"

UTP = []
_e = "gsx_project_ut_fwd"
UTP += [
    (_e, dict(B=0, C=1, N=1, rs_type=4), OK, ""), (_e, dict(B=1, C=0, N=1, rs_type=4), OK, ""),
    (_e, dict(B=1, C=1, N=0, rs_type=4), OK, ""),
    (_e, dict(B=0, C=1, N=1, rs_type=5), ERR_ARG, f"{_e}: {_rs % 5}"),  # the shutter checks precede the empty return
    (_e, dict(UT_OK, rs_type=5), ERR_ARG, f"{_e}: {_rs % 5}"),
    (_e, dict(UT_OK, rs_type=-1), ERR_ARG, f"{_e}: {_rs % -1}"),
    (_e, dict(UT_OK, rs_type=0), ERR_ARG, f"{_e}: a rolling shutter needs the end-of-frame poses"),
    (_e, dict(ONE, rs_type=4), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(UT_OK), "Ks"), ERR_ARG, f"{_e}: null input"),
    (_e, dict(ONE, **UT_IN, rs_type=4), ERR_ARG, f"{_e}: null output"),
    (_e, _drop(dict(UT_OK), "conics"), ERR_ARG, f"{_e}: null output"),
    (_e, dict(UT_OK, camera_model=5), ERR_ARG, f"{_e}: {_models % 5}"),
    (_e, dict(UT_OK, camera_model=-1), ERR_ARG, f"{_e}: {_models % -1}"),
    (_e, dict(UT_OK, camera_model=4), ERR_ARG, f"{_e}: the lidar model (4) goes through gsx_project_ut_lidar_fwd"),
    (_e, dict(UT_OK, camera_model=1, radial=P), ERR_ARG, f"{_e}: {_ortho}"),
    (_e, dict(UT_OK, camera_model=1, thin_prism=P), ERR_ARG, f"{_e}: {_ortho}"),
    (_e, dict(UT_OK, camera_model=2, radial=P), ERR_ARG, f"{_e}: {_fisheye}"),
    (_e, dict(UT_OK, camera_model=2, fisheye_max_angle=P, tangential=P), ERR_ARG, f"{_e}: {_fisheye}"),
    (_e, dict(UT_OK, camera_model=3), ERR_ARG, f"{_e}: {_ftheta}"),
    (_e, dict(UT_OK, camera_model=3, ftheta=P, radial=P), ERR_ARG, f"{_e}: {_ftheta}"),
    (_e, dict(UT_OK), ERR_ARG, f"{_e}: alpha^2 (3 + kappa) must be positive"),  # ut_alpha = 0: 3 + lambda = 0
    (_e, dict(UT_OK, rs_type=2, viewmats1=P, ut_alpha=1.0, ut_kappa=-3.0), ERR_ARG, f"{_e}: alpha^2 (3 + kappa) must be positive"),
]
_e = "gsx_project_ut_lidar_fwd"  # the same body: its messages carry the lidar entry's name
UTP += [
    (_e, dict(B=1, C=1, N=0, rs_type=4), OK, ""),
    (_e, dict(UT_OK, rs_type=5), ERR_ARG, f"{_e}: {_rs % 5}"),
    (_e, dict(UT_OK, rs_type=1), ERR_ARG, f"{_e}: a rolling shutter needs the end-of-frame poses"),
    (_e, dict(ONE, rs_type=4), ERR_ARG, f"{_e}: null input"),
    (_e, dict(ONE, **UT_IN, rs_type=4), ERR_ARG, f"{_e}: null output"),
    (_e, dict(UT_OK, rs_type=1, viewmats1=P), ERR_ARG, f"{_e}: a rolling shutter needs the angles_to_columns_map"),
    (_e, dict(UT_OK, rs_type=1, viewmats1=P, angles_to_columns_map=P, map_h=2, map_w=2, n_columns=1), ERR_ARG,
     f"{_e}: a rolling shutter needs the angles_to_columns_map"),
    (_e, dict(UT_OK, rs_type=1, viewmats1=P, angles_to_columns_map=P, map_h=2, map_w=2, n_columns=2), ERR_ARG,
     f"{_e}: alpha^2 (3 + kappa) must be positive"),
    (_e, dict(UT_OK), ERR_ARG, f"{_e}: alpha^2 (3 + kappa) must be positive"),
]

RAYS = []
_e = "gsx_camera_rays"
RAY_OK = dict(n_images=1, width=5, height=3, rs_type=4, **_ptrs("viewmats", "Ks", "rays"))
RAYS += [
    (_e, dict(n_images=0, width=5, height=3), OK, ""), (_e, dict(n_images=1, width=0, height=3), OK, ""),
    (_e, dict(n_images=1, width=5, height=0, rs_type=7, camera_model=9), OK, ""),  # no pixels: nothing is checked
    (_e, dict(n_images=1, width=5, height=3, rs_type=4), ERR_ARG, f"{_e}: null pointer"),
    (_e, _drop(dict(RAY_OK), "rays"), ERR_ARG, f"{_e}: null pointer"),
    (_e, dict(RAY_OK, camera_model=4), ERR_ARG, f"{_e}: camera model 4 is not built (pinhole 0, ortho 1, fisheye 2, f-theta 3)"),
    (_e, dict(RAY_OK, camera_model=-1), ERR_ARG, f"{_e}: camera model -1 is not built (pinhole 0, ortho 1, fisheye 2, f-theta 3)"),
    (_e, dict(RAY_OK, rs_type=5), ERR_ARG, f"{_e}: {_rs % 5}"),
    (_e, dict(RAY_OK, rs_type=-1), ERR_ARG, f"{_e}: {_rs % -1}"),
    (_e, dict(RAY_OK, rs_type=3), ERR_ARG, f"{_e}: a rolling shutter needs the end-of-frame poses"),
    (_e, dict(RAY_OK, camera_model=1, tangential=P), ERR_ARG, f"{_e}: {_ortho}"),
    (_e, dict(RAY_OK, camera_model=2, radial=P), ERR_ARG, f"{_e}: {_fisheye}"),
    (_e, dict(RAY_OK, camera_model=2, fisheye_max_angle=P, thin_prism=P), ERR_ARG, f"{_e}: {_fisheye}"),
    (_e, dict(RAY_OK, camera_model=3), ERR_ARG, f"{_e}: {_ftheta}"),
    (_e, dict(RAY_OK, camera_model=3, ftheta=P, tangential=P), ERR_ARG, f"{_e}: {_ftheta}"),
]

WORLD = []
_e = "gsx_raster_world_fwd"
W_CAM = dict(T16, cameras_per_batch=1)
W_OUT = _ptrs("render_colors", "render_alphas", "last_ids", "isect_offsets", "rays")  # what the entry needs without any list
W_IN = _ptrs("means", "quats", "scales", "colors", "opacities", "flatten_ids")
_dims = "channels and cameras_per_batch must be >= 1"
WORLD += [
    (_e, dict(tile_size=0, cdim=3, cameras_per_batch=1), ERR_ARG, f"{_e}: tile_size must be in [1,16], got 0"),
    (_e, dict(tile_size=17, cdim=3, cameras_per_batch=1), ERR_ARG, f"{_e}: tile_size must be in [1,16], got 17"),
    (_e, dict(tile_size=16, cdim=0, cameras_per_batch=1), ERR_ARG, f"{_e}: {_dims}"),
    (_e, dict(T16), ERR_ARG, f"{_e}: {_dims}"),  # cameras_per_batch = 0
    (_e, dict(W_CAM), ERR_ARG, f"{_e}: null pointer"),
    (_e, _drop(dict(W_CAM, **W_OUT), "last_ids"), ERR_ARG, f"{_e}: null pointer"),
    (_e, _drop(dict(W_CAM, **W_OUT), "rays"), ERR_ARG, f"{_e}: null pointer"),
    (_e, dict(W_CAM, **W_OUT, n_isects=1), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(W_CAM, **W_OUT, **W_IN, n_isects=1), "quats"), ERR_ARG, f"{_e}: null input"),
]
_e = "gsx_raster_world_bwd"
W_BWD_IN = dict(W_IN, **_ptrs("rays", "isect_offsets", "render_alphas", "last_ids", "v_render_colors"))
_rows = "gradient rows missing or too narrow (10 + cdim columns)"
WORLD += [
    (_e, dict(tile_size=0, cdim=3, cameras_per_batch=1), ERR_ARG, f"{_e}: tile_size must be in [1,16], got 0"),
    (_e, dict(tile_size=17, cdim=3, cameras_per_batch=1), ERR_ARG, f"{_e}: tile_size must be in [1,16], got 17"),
    (_e, dict(tile_size=16, cdim=0, cameras_per_batch=1), ERR_ARG, f"{_e}: {_dims}"),
    (_e, dict(T16), ERR_ARG, f"{_e}: {_dims}"),
    (_e, dict(W_CAM), OK, ""),  # n_isects == 0 returns before the row checks
    (_e, dict(W_CAM, use_hit_distance=1, v_render_normals=P, v_rays=P), OK, ""),
    (_e, dict(W_CAM, n_isects=1), ERR_ARG, f"{_e}: {_rows}"),
    (_e, dict(W_CAM, n_isects=1, v_rows=P, row_stride=12), ERR_ARG, f"{_e}: {_rows}"),  # 9 + cdim
    (_e, dict(W_CAM, n_isects=1, v_rows=P, row_stride=13), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(W_CAM, n_isects=1, v_rows=P, row_stride=13, **W_BWD_IN), "rays"), ERR_ARG, f"{_e}: null input"),
    (_e, _drop(dict(W_CAM, n_isects=1, v_rows=P, row_stride=13, **W_BWD_IN, use_hit_distance=1, v_render_normals=P), "last_ids"),
     ERR_ARG, f"{_e}: null input"),
]


def _ids(cases):
    return [f"{i}-{c[0][4:]}-{'ok' if c[2] == OK else c[3].split(': ', 1)[1][:28]}" for i, c in enumerate(cases)]


@pytest.mark.parametrize("entry,kw,rc,msg", EWA, ids=_ids(EWA))
def test_ewa_projection_entries(entry, kw, rc, msg):
    _check(entry, kw, rc, msg)


@pytest.mark.parametrize("entry,kw,rc,msg", P2D, ids=_ids(P2D))
def test_2dgs_projection_entries(entry, kw, rc, msg):
    _check(entry, kw, rc, msg)


@pytest.mark.parametrize("entry,kw,rc,msg", R3D, ids=_ids(R3D))
def test_3dgs_compositing_entries(entry, kw, rc, msg):
    _check(entry, kw, rc, msg)


@pytest.mark.parametrize("entry,kw,rc,msg", R2D, ids=_ids(R2D))
def test_2dgs_compositing_entries(entry, kw, rc, msg):
    _check(entry, kw, rc, msg)


@pytest.mark.parametrize("entry,kw,rc,msg", UTP, ids=_ids(UTP))
def test_ut_projection_entries(entry, kw, rc, msg):
    _check(entry, kw, rc, msg)
    assert rc == OK or msg.startswith(entry + ": ")


@pytest.mark.parametrize("entry,kw,rc,msg", RAYS, ids=_ids(RAYS))
def test_camera_ray_entries(entry, kw, rc, msg):
    _check(entry, kw, rc, msg)
    assert rc == OK or msg.startswith(entry + ": ")


@pytest.mark.parametrize("entry,kw,rc,msg", WORLD, ids=_ids(WORLD))
def test_from_world_entries(entry, kw, rc, msg):
    _check(entry, kw, rc, msg)
    assert rc == OK or msg.startswith(entry + ": ")


def test_a_successful_call_keeps_the_last_message():
    """gsx_last_error() is only written on failure: the OK cases above cannot be told from a stale message, so pin that too."""
    rc, msg = _call("gsx_project_ewa_fwd", B=1, C=1, N=1)
    assert (rc, msg) == (ERR_ARG, "gsx_project_ewa_fwd: null means/viewmats/Ks")
    assert _call("gsx_project_ewa_fwd", B=1, C=1, N=0) == (OK, msg)
