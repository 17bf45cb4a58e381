"""Compiles csrc/*.hip into the in-tree shared library with hipcc.

The library is plain HIP behind a C ABI (include/crender_hip.h): no torch headers, so
``hipcc -c`` per translation unit (in parallel) and one ``hipcc -shared`` are the whole build.
gfx950 only.
"""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_HERE, "libcrender_hip.so")
# binning.hip  K1 + the binning passes      raster.hip  K2 (tile rasterizer, k_frame, atomic path)
# model_ops.hip  rows f1-f4 of SURVEY 8f     abi.hip  plans, frames, swap chain (no kernels)
SOURCES = ["abi.hip", "binning.hip", "raster.hip", "model_ops.hip"]
HEADERS = ["common.h", "binning.h", "plan.h", "raster_math.h", os.path.join("..", "..", "include", "crender_hip.h")]
_INCLUDE = os.path.join("..", "..", "include")
# The other units of the library, in link order (which decides the library's bytes): name -> (sources, headers).  All are
# linked into the same library but kept out of source_sha16(): that fingerprint names the kernels the committed
# profiles/*.json were measured on, and these kernels are none of them.  _capi.UNIT_SIGNATURES is keyed alike.
UNITS = {
    # wireframe.hip  EdgeOnlyPixelBufferFiller, and the line passes over the winner plane: overlay, outline, edge
    # anti-aliasing, contours, hidden lines, runs (include/crender_wire.h)
    "wire": (["wireframe.hip"], [os.path.join(_INCLUDE, "crender_wire.h")]),
    # bloom.hip  bloom and tone mapping over any float32 image (include/crender_bloom.h)
    "bloom": (["bloom.hip"], [os.path.join(_INCLUDE, "crender_bloom.h")]),
    # peel.hip  transparency: depth peeling by depth key and the blend of a layer (include/crender_peel.h)
    "peel": (["peel.hip"], [os.path.join(_INCLUDE, "crender_peel.h")]),
    # dof.hip  depth of field: a gather blur by the circle of confusion over the z plane (include/crender_dof.h)
    "dof": (["dof.hip"], [os.path.join(_INCLUDE, "crender_dof.h")]),
    # normal_map.hip  a normal map from a height map, and the pass that perturbs the normal plane (include/crender_nmap.h)
    "nmap": (["normal_map.hip"], [os.path.join(_INCLUDE, "crender_nmap.h")]),
    # envmap.hip  cube-map reflections and the skybox over the winner plane (include/crender_env.h)
    "env": (["envmap.hip"], [os.path.join(_INCLUDE, "crender_env.h")]),
    # pyfill.hip  the numpy filler of crender/py (include/crender_py.h)
    "py": (["pyfill.hip"], [os.path.join(_INCLUDE, "crender_py.h")]),
    # texture.hip  the deferred texture pass over the winner plane (include/crender_tex.h)
    "tex": (["texture.hip"], [os.path.join(_INCLUDE, "crender_tex.h")]),
    # texmip.hip  the mip chain and the trilinear texture pass (include/crender_mip.h)
    "mip": (["texmip.hip"], [os.path.join(_INCLUDE, "crender_mip.h"), "mip_sample.h"]),
    # texaniso.hip  the anisotropic texture pass (include/crender_aniso.h).  mip_sample.h is what it shares with
    # texmip.hip: the chain's layout, the bilinear sample, uv at a pixel.
    "aniso": (["texaniso.hip"], [os.path.join(_INCLUDE, "crender_aniso.h"), "mip_sample.h"]),
    # resolve.hip  the supersampling resolve with the fused light and uint8 presentation (include/crender_ssaa.h)
    "ssaa": (["resolve.hip"], [os.path.join(_INCLUDE, "crender_ssaa.h")]),
    # shadow.hip  the deferred shadow-mapping pass over the winner plane (include/crender_shadow.h)
    "shadow": (["shadow.hip"], [os.path.join(_INCLUDE, "crender_shadow.h")]),
    # phong.hip  the deferred Blinn-Phong lighting pass over the winner plane (include/crender_phong.h)
    "phong": (["phong.hip"], [os.path.join(_INCLUDE, "crender_phong.h")]),
    # ao.hip  the deferred ambient-occlusion pass over the z, winner and normal planes (include/crender_ao.h)
    "ao": (["ao.hip"], [os.path.join(_INCLUDE, "crender_ao.h")]),
    # winner_pass.h  what the deferred passes over the winner plane share (texture.hip, texmip.hip, texaniso.hip,
    # shadow.hip, phong.hip, ao.hip, wireframe.hip, bloom.hip, peel.hip, dof.hip, normal_map.hip, envmap.hip,
    # motion.hip): the winner's triangle projected and the host's frame checks; the per-pixel frame, the store with the
    # fused light, the texel fetches and the launch geometry; the tile frame and the tile grid; a unit of its own,
    # without a source, so that each pass's header list stays its own.
    "pass": ([], ["winner_pass.h"]),
    # chain.hip  the swap chain's shared slot: one slot on the caller's stream (include/crender_chain.h; host code
    # only, over the pipeline handle of plan.h): it launches nothing.
    "chain": (["chain.hip"], [os.path.join(_INCLUDE, "crender_chain.h")]),
    # frame32.hip  the swap chain's frame kernel for small scenes on 32-pixel tiles (include/crender_frame32.h): it stands
    # in for one path of the fingerprinted k_frame, over the same plans and the arithmetic of raster_math.h
    "frame32": (["frame32.hip"], [os.path.join(_INCLUDE, "crender_frame32.h")]),
    # motion.hip  per-pixel motion vectors against an earlier pose, and the motion blur that gathers along them
    # (include/crender_motion.h)
    "motion": (["motion.hip"], [os.path.join(_INCLUDE, "crender_motion.h")]),
}
# Provisional: the units added since UNITS and library_sources() were pinned by their tests (tests/util.py's two lists),
# keyed like UNITS and linked behind it, outside source_sha16() like it.  The next refactor folds this table into UNITS,
# together with tests/util.py's UNIT_KEYS and LIBRARY_SOURCES.
#   temporal.hip  temporal anti-aliasing: a jittered frame resolved against its reprojected history (include/crender_taa.h)
PENDING = {
    "taa": (["temporal.hip"], [os.path.join(_INCLUDE, "crender_taa.h")]),
}

# Float parity with the reference depends on these (DESIGN.md "Numerics"):
#   -ffp-contract=off                           no FMA contraction (hipcc defaults to fast)
#   -fhip-fp32-correctly-rounded-divide-sqrt    IEEE division / sqrt
#   -fno-gpu-flush-denormals-to-zero            f32 denormals kept
# Speed only:
#   -fno-slp-vectorize   the SLP vectoriser pairs the barycentric arithmetic into v_pk_*_f32
#                        ops, which cost as much as two scalar ops each plus ~20 register moves
#                        per sample to line the operands up, and 10-25 more VGPRs; without it
#                        every workload is 3-10 % faster (r01 A/B, same box)
HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17",
    "-ffp-contract=off",
    "-fhip-fp32-correctly-rounded-divide-sqrt",
    "-fno-gpu-flush-denormals-to-zero",
    "-fno-slp-vectorize",
    "-fPIC", "-fvisibility=hidden", "-Wall", "-Wextra",
]
LINK_FLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-soname,libcrender_hip.so"]


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built")


def source_sha16() -> str:
    """Fingerprint of everything the kernels are built from — the translation units, their headers and
    the compiler flags: profiles/*.json carry it from profiling time, and bench.py quotes a committed
    profile figure only when it matches the sources it runs."""
    import hashlib
    h = hashlib.sha256()
    for name in sorted(SOURCES + HEADERS):
        with open(os.path.join(SRC_DIR, name), "rb") as fh:
            h.update(name.encode() + b"\0" + fh.read() + b"\0")
    h.update(" ".join(HIPCC_FLAGS).encode())
    return h.hexdigest()[:16]


def library_sources() -> list:
    """The translation units of the library, in link order (which decides the library's bytes)."""
    return SOURCES + [src for sources, _ in UNITS.values() for src in sources]


def build_inputs() -> list:
    """Paths of everything whose change makes the library stale: the fingerprinted sources and headers, every unit's
    sources and headers, and this file (the flags).  A header that two units list is named once."""
    names = SOURCES + HEADERS + [name for sources, headers in UNITS.values() for name in sources + headers]
    return [os.path.join(SRC_DIR, name) for name in dict.fromkeys(names)] + [os.path.abspath(__file__)]


def pending_sources() -> list:
    """The translation units of PENDING, linked behind library_sources()."""
    return [src for sources, _ in PENDING.values() for src in sources]


def pending_inputs() -> list:
    """Paths of PENDING's sources and headers: build() counts them like build_inputs()."""
    names = [name for sources, headers in PENDING.values() for name in sources + headers]
    return [os.path.join(SRC_DIR, name) for name in dict.fromkeys(names)]


def needs_build(inputs=None) -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    built = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > built for d in (build_inputs() if inputs is None else inputs))


def compile_library(out: str, extra_flags=(), sources=None, src_dir: str = SRC_DIR, verbose: bool = False,
                    quiet: bool = False) -> str:
    """hipcc -c every translation unit (side by side), then link them into `out`.  `extra_flags`:
    defines of diagnostic builds (-DCRENDER_STAMPS, ...)."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    sources = list(sources or library_sources() + pending_sources())
    err = subprocess.DEVNULL if quiet else None
    with tempfile.TemporaryDirectory(prefix="crender_build_") as tmp:
        objs = [os.path.join(tmp, os.path.splitext(s)[0] + ".o") for s in sources]

        def one(job):
            src, obj = job
            cmd = [_hipcc()] + HIPCC_FLAGS + list(extra_flags) + ["-c", "-o", obj, os.path.join(src_dir, src)]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd, stderr=err)

        with ThreadPoolExecutor(max_workers=min(4, len(sources))) as pool:
            list(pool.map(one, zip(sources, objs)))
        # link beside the target and rename onto it: ranks started together on a stale library all
        # build, and none may dlopen a half-written file
        part = f"{out}.{os.getpid()}.part"
        cmd = [_hipcc()] + LINK_FLAGS + ["-o", part] + objs
        if verbose:
            print(" ".join(cmd))
        try:
            subprocess.check_call(cmd, stderr=err)
            os.replace(part, out)
        finally:
            if os.path.exists(part):
                os.remove(part)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    """Build libcrender_hip.so if missing or stale; returns its path."""
    if not force and not needs_build() and not needs_build(pending_inputs()):
        return LIB_PATH
    return compile_library(LIB_PATH, verbose=verbose)


if __name__ == "__main__":
    print(build(force=True, verbose=True))
