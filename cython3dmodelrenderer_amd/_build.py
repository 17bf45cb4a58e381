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
# wireframe.hip  EdgeOnlyPixelBufferFiller (include/crender_wire.h).  Linked into the same library but
# kept out of source_sha16(): that fingerprint names the kernels the committed profiles/*.json were
# measured on, and the wireframe kernels are none of them.
WIRE_SOURCES = ["wireframe.hip"]
WIRE_HEADERS = [os.path.join("..", "..", "include", "crender_wire.h")]
# pyfill.hip  the numpy filler of crender/py (include/crender_py.h); kept out of source_sha16() likewise.
PY_SOURCES = ["pyfill.hip"]
PY_HEADERS = [os.path.join("..", "..", "include", "crender_py.h")]
# texture.hip  the deferred texture pass over the winner plane (include/crender_tex.h); kept out of
# source_sha16() likewise.
TEX_SOURCES = ["texture.hip"]
TEX_HEADERS = [os.path.join("..", "..", "include", "crender_tex.h")]
# texmip.hip  the mip chain and the trilinear texture pass (include/crender_mip.h); kept out of
# source_sha16() likewise.
MIP_SOURCES = ["texmip.hip"]
MIP_HEADERS = [os.path.join("..", "..", "include", "crender_mip.h"), "mip_sample.h"]
# texaniso.hip  the anisotropic texture pass (include/crender_aniso.h); kept out of source_sha16() likewise.
# mip_sample.h is what it shares with texmip.hip: the chain's layout, the bilinear sample, uv at a pixel.
ANISO_SOURCES = ["texaniso.hip"]
ANISO_HEADERS = [os.path.join("..", "..", "include", "crender_aniso.h"), "mip_sample.h"]
# resolve.hip  the supersampling resolve with the fused light and uint8 presentation (include/crender_ssaa.h);
# kept out of source_sha16() likewise.
SSAA_SOURCES = ["resolve.hip"]
SSAA_HEADERS = [os.path.join("..", "..", "include", "crender_ssaa.h")]
# shadow.hip  the deferred shadow-mapping pass over the winner plane (include/crender_shadow.h); kept out of
# source_sha16() likewise.
SHADOW_SOURCES = ["shadow.hip"]
SHADOW_HEADERS = [os.path.join("..", "..", "include", "crender_shadow.h")]
# phong.hip  the deferred Blinn-Phong lighting pass over the winner plane (include/crender_phong.h); kept out of
# source_sha16() likewise.
PHONG_SOURCES = ["phong.hip"]
PHONG_HEADERS = [os.path.join("..", "..", "include", "crender_phong.h")]
# ao.hip  the deferred ambient-occlusion pass over the z, winner and normal planes (include/crender_ao.h); kept out of
# source_sha16() likewise.
AO_SOURCES = ["ao.hip"]
AO_HEADERS = [os.path.join("..", "..", "include", "crender_ao.h")]
# winner_pass.h  what the deferred passes over the winner plane share (texture.hip, texmip.hip, texaniso.hip,
# shadow.hip, phong.hip): the pixel frame, the corner gather, the store with the fused light, the texel fetches and the launch
# geometry; a group of its own, so that each pass's header list stays its own; kept out of source_sha16() likewise.
PASS_HEADERS = ["winner_pass.h"]
# chain.hip  the swap chain's shared slot: one slot on the caller's stream (include/crender_chain.h; host code
# only, over the pipeline handle of plan.h); kept out of source_sha16() likewise: it launches nothing.
CHAIN_SOURCES = ["chain.hip"]
CHAIN_HEADERS = [os.path.join("..", "..", "include", "crender_chain.h")]

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


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    built = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(SRC_DIR, s) for s in SOURCES + HEADERS + WIRE_SOURCES + WIRE_HEADERS +
                                                PY_SOURCES + PY_HEADERS + TEX_SOURCES + TEX_HEADERS +
                                                MIP_SOURCES + MIP_HEADERS + ANISO_SOURCES + ANISO_HEADERS +
                                                SSAA_SOURCES + SSAA_HEADERS + SHADOW_SOURCES + SHADOW_HEADERS +
                                                PHONG_SOURCES + PHONG_HEADERS + AO_SOURCES + AO_HEADERS + CHAIN_SOURCES + CHAIN_HEADERS +
                                                PASS_HEADERS] + \
        [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > built for d in deps)


def compile_library(out: str, extra_flags=(), sources=None, src_dir: str = SRC_DIR, verbose: bool = False,
                    quiet: bool = False) -> str:
    """hipcc -c every translation unit (side by side), then link them into `out`.  `extra_flags`:
    defines of diagnostic builds (-DCRENDER_STAMPS, ...)."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    sources = list(sources or SOURCES + WIRE_SOURCES + PY_SOURCES + TEX_SOURCES + MIP_SOURCES + ANISO_SOURCES +
                   SSAA_SOURCES + SHADOW_SOURCES + PHONG_SOURCES + AO_SOURCES + CHAIN_SOURCES)
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
    if not force and not needs_build():
        return LIB_PATH
    return compile_library(LIB_PATH, verbose=verbose)


if __name__ == "__main__":
    print(build(force=True, verbose=True))
