"""ctypes binding of libcrender_hip.so (C ABI: include/crender_hip.h).

There is no CPU fallback: if the shared library is missing or fails to load, importing
a symbol from here raises.  Device pointers are plain integers (``tensor.data_ptr()``).
"""
from __future__ import annotations

import ctypes as C
import os

from . import _build

ABI_VERSION = 6
OK, EINVAL, EHIP, ENOMEM, EBUSY, ESTATE = 0, 1, 2, 3, 4, 5
FUSED_CLEAR = 1
NO_DIRECT_BINS = 2
OVERLAPPED_FRAMES = 4
FUSED_GURO = 8
STATIC_INPUTS = 16
# raster kernels of a 32-pixel plan (crender_plan_set_raster_path): both exact on every tile
PATH_AUTO, PATH_GENERAL, PATH_OWNERS = -1, 0, 1

_vp, _i32, _i64, _u32, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint, C.c_size_t
_f32p = C.POINTER(C.c_float)

# name -> (restype, argtypes); mirrors include/crender_hip.h one to one
SIGNATURES = {
    "crender_abi_version": (_i32, []),
    "crender_last_error": (C.c_char_p, []),
    "crender_projection_matrix": (_i32, [C.c_double, C.c_double, C.c_double, _i32, _i32, _f32p]),
    "crender_project": (_i32, [_vp, _vp, _i64, _f32p, _i32, _i32, _vp]),
    "crender_clear": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "crender_plan_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i64, _i64, _i32]),
    "crender_plan_create": (_i32, [C.POINTER(_vp), _i32, _i32, _i32, _i32, _i64, _i64, _i32,
                                   _vp, _sz, _vp]),
    "crender_plan_destroy": (None, [_vp]),
    "crender_plan_last_bin_usage": (_i32, [_vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "crender_plan_last_frame_direct": (_i32, [_vp]),
    "crender_plan_last_frame_binning": (_i32, [_vp]),
    "crender_plan_frame_ticket": (C.c_uint64, [_vp]),
    "crender_plan_poll_bin_usage": (_i32, [_vp, C.c_uint64, C.POINTER(_i64), C.POINTER(_i64)]),
    "crender_plan_set_light": (_i32, [_vp, _f32p]),
    "crender_plan_debug_check": (_i32, [_vp, _vp, C.c_char_p, _sz]),
    "crender_plan_set_raster_path": (_i32, [_vp, _i32]),
    "crender_plan_last_raster_path": (_i32, [_vp]),
    "crender_set_default_raster_path": (_i32, [_i32]),
    "crender_plan_set_triangle_order": (_i32, [_vp, _vp, _vp]),
    "crender_plan_set_normal_z": (_i32, [_vp, _vp]),
    "crender_tile_order_keys": (_i32, [_vp, _i64, _f32p, _i32, _i32, _vp, _vp]),
    "crender_plan_timing_begin": (_i32, [_vp, _i32]),
    "crender_plan_timing_end": (_i32, [_vp, _vp, C.POINTER(_i32), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]),
    "crender_raster": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _u32, _vp]),
    "crender_render_model": (_i32, [_vp, _vp, _vp, _vp, _i64, _f32p, _vp, _vp, _vp, _vp, _u32, _vp]),
    "crender_prepare": (_i32, [_vp, _vp, _vp, _i64, _f32p, _u32, _vp]),
    "crender_draw": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _u32, _vp]),
    "crender_pipeline_create": (_i32, [C.POINTER(_vp), C.POINTER(_vp), _i32]),
    "crender_pipeline_destroy": (None, [_vp]),
    "crender_pipeline_frame": (_i32, [_vp, _vp, _vp, _vp, _i64, _f32p, _vp, _vp, _vp, _vp, _u32, _vp]),
    "crender_pipeline_join": (_i32, [_vp, _vp]),
    "crender_pipeline_bind": (_i32, [_vp, _i32, _vp, _vp, _vp, _i64, _f32p, _vp, _vp, _vp, _vp, _u32]),
    "crender_pipeline_submit": (_i32, [_vp, _vp]),
    "crender_pipeline_timing_begin": (_i32, [_vp, _i32]),
    "crender_pipeline_timing_end": (_i32, [_vp, C.POINTER(_i32), C.POINTER(C.c_double)]),
    "crender_atomic_scratch_bytes": (_sz, [_i32, _i32]),
    "crender_raster_atomic": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                                     _u32, _vp, _vp]),
    "crender_selfcheck_division": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "crender_present_u8": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "crender_guro_illumination": (_i32, [_vp, _vp, _f32p, _i32, _i32, _i32, _i32, _vp]),
    "crender_model_shift": (_i32, [_vp, _i64, C.POINTER(C.c_double), _i32, _vp]),
    "crender_model_scale": (_i32, [_vp, _i64, _vp, C.c_float, _i32, _vp]),
    "crender_model_scale3": (_i32, [_vp, _i64, _vp, C.POINTER(C.c_double), _i32, _i32, _vp]),
    "crender_model_stats": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "crender_pipeline_set_lookahead": (_i32, [_vp, _vp, _i32]),
    "crender_model_gather": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "crender_model_rotate": (_i32, [_vp, _i64, C.POINTER(C.c_double), _vp]),
    "crender_model_vertex_normals": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crender_model_texture_colors": (_i32, [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp]),
}

# The entry points of the library's other units, each bound from a table of its own beside its constants:
# unit -> {name: (restype, argtypes)}, keyed like _build.UNITS (whose "pass" is a header without entry points).
UNIT_SIGNATURES = {}

# the wireframe filler's entry points (include/crender_wire.h), bound from a table of their own
WIRE_DOTS, WIRE_FORCE_COLORS, WIRE_CLEAR = 1, 2, 4
WIRE_MAX_WIDTH = 64
WIRE_OUTLINE_MAX_RADIUS = 8
WIRE_CONTOUR_BORDERS = 1
WIRE_HIDDEN_USE_WINNER = 1
WIRE_MAX_DASH = 64
WIRE_RUNS_GROUP = 256
WIRE_RUNS_USE_WINNER = 1
UNIT_SIGNATURES["wire"] = {
    "crender_wire_key_bytes": (_sz, [_i32, _i32]),
    "crender_wire_draw": (_i32, [_vp, _vp, _i64, _f32p, _vp, _vp, _vp, _vp, _i32, _i32, _u32, _vp, _vp]),
    # the hidden-line overlay over the winner plane: a deferred pass (DeferredPasses.wire_pass)
    "crender_wire_overlay": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _f32p, _f32p, C.c_float, C.c_float, C.c_float, _vp,
                                    _i32, _i32, _i32, _i32, _u32, _vp]),
    # the same lines at full width, from the winners of a pixel's neighbourhood (DeferredPasses.wire_pass(outline=True)):
    # the overlay's arguments with d_z after d_winner, and depth_bias and radius_px after the opacity
    "crender_wire_outline": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _f32p, _f32p, C.c_float, C.c_float, C.c_float,
                                    C.c_float, _i32, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
    # the edge mask of a view for the two: contour edges from the model's partner table (DeferredPasses.contour_edges)
    "crender_wire_contours": (_i32, [_vp, _i64, _vp, _f32p, _vp, _vp, _vp, _vp, _i32, _i32, _u32, _vp]),
    # geometric edge anti-aliasing over the winner plane (DeferredPasses.edge_aa): the outline's planes and mask, the
    # result plane in front of the colour plane, which is only read
    "crender_wire_edge_aa": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
    # the edges behind the surface, dashed (DeferredPasses.hidden_line_pass): the outline's planes and mask, the line's
    # colour, opacity, dash and depth bias, the key plane in front of the colour plane
    "crender_wire_hidden": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _f32p, C.c_float, _i32, _i32, C.c_float, _vp, _vp,
                                   _i32, _i32, _i32, _i32, _u32, _vp]),
    # the same classification kept as vector segments (DeferredPasses.line_runs): the hidden pass's planes and mask, the
    # partner table and the bias; the counts per group of 256 segments, then their prefix, the total and the two results
    "crender_wire_runs_groups": (_i64, [_i64]),
    "crender_wire_runs_count": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _vp, C.c_float, _vp, _i32, _i32, _i32, _i32,
                                       _u32, _vp]),
    "crender_wire_runs_emit": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _vp, C.c_float, _vp, _i64, _vp, _vp, _i32, _i32,
                                      _i32, _i32, _u32, _vp]),
}

# bloom and tone mapping (include/crender_bloom.h), bound from a table of its own (DevicePlanes.bloom, bloom.bloom):
# any float32 image, the threshold, the HOST weights and the
# radius, intensity, exposure, 1 / white^2 and the clamp, the scratch plane and the result, then the frame and the rows
BLOOM_MAX_RADIUS = 32
BLOOM_U8, BLOOM_FLIP, BLOOM_REINHARD, BLOOM_GAMMA2 = 1, 2, 4, 8
UNIT_SIGNATURES["bloom"] = {
    "crender_bloom": (_i32, [_vp, C.c_float, _f32p, _i32, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp,
                             _i32, _i32, _i32, _i32, _u32, _vp]),
}

# transparency (include/crender_peel.h), bound from a table of its own (DeferredPasses.peel_layers,
# transparency_pass): the outline's frame of a given layer, then the normals,
# the key scratch and the next layer's winner plane, its z plane in the colour plane's place
PEEL_FIRST, PEEL_LAST = 1, 2
PEEL_MAX_LAYERS = 16
UNIT_SIGNATURES["peel"] = {
    "crender_peel_next": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
    # and a layer blended under what is in front of it: the overlay's frame, then the colours, normals and alpha, the
    # light, the front colours, the background, the transmittance plane, the sum in the colour plane's place
    "crender_peel_blend": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _vp, _vp, _f32p, _vp, _f32p, _vp, _vp, _i32, _i32, _i32,
                                  _i32, _u32, _vp]),
}

# depth of field (include/crender_dof.h), bound from a table of its own (DeferredPasses.depth_of_field):
# the outline's frame, then the colour plane, which is only read, the
# focus, the band, the aperture and the largest radius, the result plane
DOF_MAX_RADIUS = 12
UNIT_SIGNATURES["dof"] = {
    "crender_dof_blur": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, C.c_float, C.c_float, C.c_float, _i32, _vp,
                                _i32, _i32, _i32, _i32, _u32, _vp]),
}

# normal mapping (include/crender_nmap.h), bound from a table of its own (DeferredPasses.bind_normal_map,
# normal_map_pass): a tangent-space map from a height map, and the
# pass that perturbs the normal plane: the overlay's frame, then the uv, the map and its size, the strength, the plane
NMAP_WRAP = 1
NMAP_PERSPECTIVE, NMAP_BILINEAR, NMAP_CHAIN = 1, 2, 4
UNIT_SIGNATURES["nmap"] = {
    "crender_nmap_from_height": (_i32, [_vp, _i32, _i32, C.c_float, _u32, _vp, _vp]),
    "crender_nmap_shade": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _i32, C.c_float, _vp, _i32, _i32, _i32, _i32,
                                  _u32, _vp]),
}

# environment mapping (include/crender_env.h), bound from a table of its own (DeferredPasses.bind_environment,
# environment_pass): the overlay's frame, then the normal plane,
# the two levels' faces and sides and the second one's weight, the orientation, reflectivity, f0, the tint, the
# background's gain
ENV_REFLECT, ENV_BACKGROUND = 1, 2
ENV_MAX_SIDE = 8192
UNIT_SIGNATURES["env"] = {
    "crender_env_shade": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _vp, _i32, C.c_float, _f32p, C.c_float, C.c_float,
                                 _f32p, C.c_float, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
}

# the numpy filler's entry points (include/crender_py.h), bound from a table of their own
PY_CLEAR = 1
UNIT_SIGNATURES["py"] = {
    "crender_py_scratch_bytes": (_sz, [_i32, _i32, _i64]),
    "crender_py_draw": (_i32, [_vp, _vp, _vp, _i64, _f32p, _vp, _vp, _vp, _i32, _i32, _u32, _vp, _vp, _vp]),
    "crender_py_guro": (_i32, [_vp, _vp, _f32p, _i32, _i32, _vp]),
}

# the deferred texture pass (include/crender_tex.h), bound from a table of its own
TEX_PERSPECTIVE, TEX_BILINEAR = 1, 2
UNIT_SIGNATURES["tex"] = {
    "crender_tex_shade": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _i32, _vp, _f32p, _vp,
                                 _i32, _i32, _i32, _i32, _u32, _vp]),
}

# the mip chain and the trilinear texture pass (include/crender_mip.h), bound from a table of their own
MIP_PERSPECTIVE = 1
MIP_MAX_LEVELS = 16
_u64p = C.POINTER(C.c_uint64)
UNIT_SIGNATURES["mip"] = {
    "crender_mip_layout": (_i32, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _u64p, _u64p]),
    "crender_mip_build": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "crender_mip_shade": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _i32, _vp, _f32p, _vp,
                                 _i32, _i32, _i32, _i32, _u32, _vp]),
}

# the anisotropic texture pass (include/crender_aniso.h), bound from a table of its own: crender_mip_shade's
# arguments with max_aniso in front of the stream
ANISO_MAX = 16
UNIT_SIGNATURES["aniso"] = {
    "crender_aniso_shade": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _i32, _vp, _f32p, _vp,
                                   _i32, _i32, _i32, _i32, _u32, _i32, _vp]),
}

# the supersampling resolve (include/crender_ssaa.h), bound from a table of its own
SSAA_U8, SSAA_FLIP = 1, 2
SSAA_MAX = 8
UNIT_SIGNATURES["ssaa"] = {
    "crender_ssaa_resolve": (_i32, [_vp, _vp, _f32p, _i32, _i32, _i32, _i32, _i32, _vp, _u32, _vp]),
}

# the deferred shadow pass (include/crender_shadow.h), bound from a table of its own
SHADOW_PCF = (1, 3, 5)
UNIT_SIGNATURES["shadow"] = {
    "crender_shadow_shade": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _f32p, _vp, _vp, _i32, _i32, C.c_float, C.c_float,
                                    _i32, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
}

# the deferred Phong pass (include/crender_phong.h), bound from a table of its own
PHONG_MAX_LIGHTS = 4
PHONG_MAX_SHININESS = 1 << 12
UNIT_SIGNATURES["phong"] = {
    "crender_phong_shade": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, _f32p, _i32, _u32, C.c_float, _i32, _f32p, C.c_float,
                                   _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
}

# the deferred ambient-occlusion pass (include/crender_ao.h), bound from a table of its own
AO_ROTATE, AO_FACE_NORMALS = 1, 2
AO_MAX_TAPS = 64
AO_MAX_RADIUS_PX = 32
UNIT_SIGNATURES["ao"] = {
    "crender_ao_shade": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _i32, C.c_float, C.c_float, C.c_float,
                                C.c_float, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
}

# the swap chain's shared slot (include/crender_chain.h), bound from a table of its own
UNIT_SIGNATURES["chain"] = {
    "crender_pipeline_share_stream": (_i32, [_vp, _i32, _vp]),
    "crender_pipeline_unshare": (_i32, [_vp]),
    "crender_pipeline_shared_slot": (_i32, [_vp]),
    "crender_pipeline_owned_streams": (_i32, [_vp]),
}

# the swap chain's frame kernel for small scenes (include/crender_frame32.h), bound from a table of its own: it stands in
# for one path of k_frame
UNIT_SIGNATURES["frame32"] = {
    "crender_frame32_submit": (_i32, [_vp, _vp]),
    "crender_frame32_last": (_i32, [_vp]),
}

# motion vectors and motion blur (include/crender_motion.h), bound from a table of their own
# (DeferredPasses.motion_vectors, motion_blur): the overlay's frame, then the previous pose, the exposure and the velocity
# plane; and the lens's frame, then the colour and the velocity planes, the largest radius, the taps, the depth range, the result
MOTION_MAX_RADIUS = 12
MOTION_MAX_TAPS = 32
UNIT_SIGNATURES["motion"] = {
    "crender_motion_vectors": (_i32, [_vp, _vp, _i64, _vp, _f32p, _vp, C.c_float, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
    "crender_motion_blur": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _i32, C.c_float, _vp,
                                   _i32, _i32, _i32, _i32, _u32, _vp]),
}

# Provisional, keyed like _build.PENDING: the next refactor folds this table into UNIT_SIGNATURES, together with
# tests/util.py's two lists.  Temporal anti-aliasing (include/crender_taa.h; DeferredPasses.temporal_resolve): the frame's
# colour, the history, the velocity and the z plane or NULL, the blend, the result, then the frame, the rows and the flags
TAA_NO_CLAMP = 1
PENDING = {
    "taa": {
        "crender_taa_resolve": (_i32, [_vp, _vp, _vp, _vp, C.c_float, _vp, _i32, _i32, _i32, _i32, _u32, _vp]),
    },
}

_lib = None


class CrenderError(RuntimeError):
    pass


def lib_path() -> str:
    # CRENDER_LIB: load another build of the same ABI (diagnostic builds, A/B variants)
    return os.environ.get("CRENDER_LIB") or _build.LIB_PATH


def load():
    """Load the shared library (never builds it: see __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise CrenderError(
            f"{path} is missing: build it with `python -m cython3dmodelrenderer_amd._build` "
            "(or __graft_entry__.build()).  There is no CPU fallback for the rasterizer.")
    L = C.CDLL(path)
    for table in (SIGNATURES, *UNIT_SIGNATURES.values(), *PENDING.values()):
        for name, (res, args) in table.items():
            fn = getattr(L, name)      # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
    got = L.crender_abi_version()
    if got != ABI_VERSION:
        raise CrenderError(f"libcrender_hip.so ABI {got}, binding expects {ABI_VERSION}")
    _lib = L
    return L


def check(status: int, what: str):
    if status != OK:
        msg = load().crender_last_error()
        raise CrenderError(f"{what} failed (code {status}): {msg.decode() if msg else ''}")


def plan_debug_check(plan_handle, stream):
    """crender_plan_debug_check: raises CrenderError with the findings if the plan's cross-frame state is
    inconsistent (synchronises `stream`)."""
    buf = C.create_string_buffer(2048)
    rc = load().crender_plan_debug_check(plan_handle, stream, buf, len(buf))
    if rc == ESTATE:
        raise CrenderError("plan state: " + buf.value.decode(errors="replace"))
    check(rc, "crender_plan_debug_check")


def f32_16(mat):
    """Host float32[16] ctypes array from a 4x4 numpy matrix."""
    import numpy as np
    a = np.ascontiguousarray(mat, dtype=np.float32).reshape(16)
    return (C.c_float * 16)(*a.tolist())
