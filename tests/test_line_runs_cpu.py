"""The drawing as vectors without a GPU: the header against the binding and the library, the two entry points' argument
checks and their order, the host model the GPU tests compare with (tests/runs_ref.py) pinned against a plain loop, by the
identity with ``hidden_ref.classes``, on the counts of the oracle's frames and against a float64 evaluation of the end
points; ``wireframe.half_edges_once`` and ``wireframe.write_svg``; ``AdvancedPixelBufferFiller.line_runs``'s protocol on CPU
tensors and ``Renderer(wireframe={"vector": ...})``."""
import ctypes as C
import inspect
import io
import os
import re
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

import contour_ref
import hidden_ref
import pass_edges
import runs_ref
import tex_ref
import wire_ref
from pass_scenes import Frame, capi, fake_filler_base, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import UNIT_KEYS, assert_bit_equal, other_symbols, random_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_float
VP = C.c_void_p
COUNT_ARGTYPES = [VP, VP, VP, C.c_int64, VP, C.POINTER(F), VP, VP, F, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, VP]
EMIT_ARGTYPES = [VP, VP, VP, C.c_int64, VP, C.POINTER(F), VP, VP, F, VP, C.c_int64, VP, VP, C.c_int, C.c_int, C.c_int, C.c_int,
                 C.c_uint, VP]
NAN, INF = float("nan"), float("inf")
T_MAX = (2 ** 31 - 1) // 3


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_runs_symbols_are_declared_exported_and_bound(capi):
    from cython3dmodelrenderer_amd import _build
    header = open(os.path.join(ROOT, "include", "crender_wire.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    new = {"crender_wire_runs_groups", "crender_wire_runs_count", "crender_wire_runs_emit"}
    assert new <= declared and declared == set(capi.UNIT_SIGNATURES["wire"])
    assert not declared & other_symbols(capi, "wire")
    assert capi.UNIT_SIGNATURES["wire"]["crender_wire_runs_groups"] == (C.c_int64, [C.c_int64])
    assert capi.UNIT_SIGNATURES["wire"]["crender_wire_runs_count"] == (C.c_int, COUNT_ARGTYPES)
    assert capi.UNIT_SIGNATURES["wire"]["crender_wire_runs_emit"] == (C.c_int, EMIT_ARGTYPES)
    L = capi.load()
    assert L.crender_wire_runs_count.argtypes == COUNT_ARGTYPES and L.crender_wire_runs_emit.argtypes == EMIT_ARGTYPES
    want = {
        "count": ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
                  "const float *P16", "const uint8_t *d_edges", "const int32_t *d_partners", "float depth_bias", "uint32_t *d_counts",
                  "int H", "int W", "int y0", "int y1", "unsigned flags", "void *stream"],
        "emit": ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
                 "const float *P16", "const uint8_t *d_edges", "const int32_t *d_partners", "float depth_bias",
                 "const int64_t *d_offsets", "int64_t N", "int32_t *d_runs", "float *d_ends", "int H", "int W", "int y0", "int y1",
                 "unsigned flags", "void *stream"],
    }
    by_type = {"float": F, "int": C.c_int, "int64_t": C.c_int64, "unsigned": C.c_uint}
    for name, args in (("count", COUNT_ARGTYPES), ("emit", EMIT_ARGTYPES)):
        decl = re.search(rf"CRENDER_API int crender_wire_runs_{name}\((.*?)\);", header, re.S).group(1)
        params = [" ".join(a.split()) for a in decl.split(",")]
        assert params == want[name] and len(params) == len(args)
        for p, a in zip(params, args):
            assert a in (VP, C.POINTER(F)) if "*" in p else a is by_type[p.rsplit(" ", 1)[0]], p
    # the operands the two share with crender_wire_hidden come in its order
    hidden = re.search(r"CRENDER_API int crender_wire_hidden\((.*?)\);", header, re.S).group(1)
    assert [" ".join(a.split()) for a in hidden.split(",")][:7] == want["count"][:7] == want["emit"][:7]
    assert re.search(r"#define CRENDER_WIRE_RUNS_GROUP 256\b", header) and capi.WIRE_RUNS_GROUP == runs_ref.GROUP == 256
    assert re.search(r"#define CRENDER_WIRE_RUNS_USE_WINNER 1u\b", header) and capi.WIRE_RUNS_USE_WINNER == 1
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert new <= set(re.findall(r" T (crender_\w+)", out))
    # the feature lives in the wire unit as it was: no new unit, no new source, no new ABI, the same fingerprint
    assert capi.ABI_VERSION == 6
    assert _build.source_sha16() == "35a9bf480abfca1e"
    assert _build.UNITS["wire"][0] == ["wireframe.hip"]
    assert list(_build.UNITS) == UNIT_KEYS
    unit = open(os.path.join(_build.SRC_DIR, "wireframe.hip")).read()
    # after the hidden pass, whose text is left alone; count and emit are ONE template, without atomics or assembly
    assert unit.index("void k_wire_hidden") < unit.index("int wire_window(") < unit.index("void k_wire_runs")
    body = unit[unit.index("void k_wire_runs"):unit.index("int runs_checks(")]
    assert unit.count("void k_wire_runs(") == 1 and "k_wire_runs<kRunsCount>" in unit and "k_wire_runs<kRunsEmit>" in unit
    assert body.count("seg_setup(") == 1 and body.count("seg_pixel(") == 1 and "winner_triangle(" in body
    assert "atomic" not in body and "asm" not in body and "printf" not in body and "assert" not in body
    assert "wave_rank(" in body and "__builtin_amdgcn_ballot_w64" in unit and body.count("__syncthreads()") == 4


def test_the_groups_of_a_count(capi):
    L = capi.load()
    for T, want in ((0, 0), (1, 1), (85, 1), (86, 2), (171, 3), (13814, 162), (T_MAX, 8388608), (T_MAX + 1, -1), (-1, -1),
                    (2 ** 40, -1), (-2 ** 40, -1)):
        assert L.crender_wire_runs_groups(T) == want == runs_ref.groups(T), T
    assert 3 * T_MAX <= 2 ** 31 - 1 < 3 * (T_MAX + 1)


def test_runs_argument_errors_and_their_order_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (F * 16)(*([0.0] * 16))
    fake = C.c_void_p(0x1000)            # never dereferenced: every call below fails its checks first

    def count(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, edges=None, partners=None, bias=1e-3, counts=fake, H=8, W=8, y0=0,
              y1=8, flags=1):
        return L.crender_wire_runs_count(win, z, tri, T, pos_of, P, edges, partners, bias, counts, H, W, y0, y1, flags, None)

    def emit(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, edges=None, partners=None, bias=1e-3, offsets=fake, N=5, runs=fake,
             ends=fake, H=8, W=8, y0=0, y1=8, flags=1):
        return L.crender_wire_runs_emit(win, z, tri, T, pos_of, P, edges, partners, bias, offsets, N, runs, ends, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    shared = [
        (dict(T=-1), "T is negative"), (dict(tri=None), "d_tri is NULL with T > 0"), (dict(W=-2), "H or W is below 1"),
        (dict(y0=3, y1=3), "rows outside the frame"), (dict(H=2 ** 20 + 1), "H or W is above 2^20"),
        (dict(bias=NAN), "depth_bias is not finite"), (dict(flags=2), "unknown flag bits"),
    ]
    last = [(dict(T=T_MAX + 1), "T is too large")]
    null_count = "d_winner, d_z, P16 or d_counts is NULL"
    null_emit = "d_winner, d_z, P16, d_offsets, d_runs or d_ends is NULL"
    cases = {
        "count": (count, [(dict(win=None), null_count), (dict(z=None), null_count), (dict(P=None), null_count),
                          (dict(counts=None), null_count)] + shared + last),
        "emit": (emit, [(dict(win=None), null_emit), (dict(z=None), null_emit), (dict(P=None), null_emit), (dict(offsets=None), null_emit),
                        (dict(runs=None), null_emit), (dict(ends=None), null_emit)] + shared + [(dict(N=-1), "N is negative")] + last),
    }
    for name, (call, checks) in cases.items():
        prefix = f"crender_wire_runs_{name}: "
        for kw, words in checks:
            assert call(**kw) == E and text() == prefix + words, (name, kw, text())
        # more values of each
        for kw in (dict(T=-2 ** 40), dict(H=0), dict(H=-2 ** 31), dict(y0=-1), dict(y1=9), dict(y0=5, y1=2), dict(W=2 ** 20 + 1),
                   dict(bias=INF), dict(bias=-INF), dict(flags=3), dict(flags=0x80000000), dict(T=2 ** 62)):
            assert call(**kw) == E and text().startswith(prefix), (name, kw)
        # every pair of two checks in one call reports the earlier one
        for a in range(len(checks)):
            for b in range(a + 1, len(checks)):
                (ka, wa), (kb, wb) = checks[a], checks[b]
                if set(ka) & set(kb) or wa == wb:
                    continue
                assert call(**ka, **kb) == E and text() == prefix + wa, (name, ka, kb, text())
        # what is no error, with T == 0, which returns before any launch (so without a device too)
        for kw in (dict(), dict(tri=None), dict(flags=0), dict(bias=-1.0), dict(bias=0.0), dict(H=2 ** 20, W=2 ** 20, y1=2 ** 20),
                   dict(y0=7), dict(edges=fake, pos_of=fake, partners=fake, H=1, W=1, y1=1)):
            assert call(T=0, **kw) == capi.OK, (name, kw)
    assert emit(N=-2 ** 40) == E and emit(T=0, N=0) == capi.OK and emit(T=0, N=2 ** 40) == capi.OK
    assert emit(N=0) == capi.OK                                          # no run to store: no launch either


# ---- the statements again, a segment at a time ------------------------------------------------------------------

def _loop_model(winner, z, tri, P, edges=None, pos_of=None, partners=None, depth_bias=1e-3, use_winner=True, y0=0, y1=None):
    """The contract read line by line in plain Python, np.float32 scalars throughout: the classes of ALL el + 1 steps of a
    segment (0 off the frame and the rows), then its runs from one serial pass.  (runs, ends)."""
    f32 = np.float32
    H, W = winner.shape
    y1 = H if y1 is None else y1
    T = len(tri)
    runs, ends = [], []
    if T:
        proj = tex_ref.project(np.ascontiguousarray(tri, np.float32), P, W, H)
    with np.errstate(all="ignore"):
        for i in range(T):
            q = i if pos_of is None else int(pos_of[i])
            if q >= T:
                continue
            for e in range(3):
                if edges is not None and not (int(edges[i]) >> e) & 1:
                    continue
                g = (e + 1) % 3
                if not (tri[q, e, 2] > 0 and tri[q, g, 2] > 0):
                    continue
                a, b = proj[q, e], proj[q, g]
                if not all(abs(c) < f32(2.0 ** 30) for c in (a[0], a[1], b[0], b[1])):
                    continue
                pa, pb = (int(np.rint(a[0])), int(np.rint(a[1]))), (int(np.rint(b[0])), int(np.rint(b[1])))
                if (pb[1], pb[0]) < (pa[1], pa[0]):
                    pa, pb, a, b = pb, pa, b, a
                assert max(abs(pb[0] - pa[0]), abs(pb[1] - pa[1])) < 4096          # (the loop is for lines near the frame)
                pts = wire_ref.line_pixels(pa, pb)
                el = len(pts) - 1
                dz = b[2] - a[2]
                cls = []
                for t, (x, y) in enumerate(pts):
                    if not (0 <= x < W and 0 <= y < H and y0 <= y < y1):
                        cls.append(0)
                        continue
                    lam = f32(t) / f32(el) if el else f32(0)
                    ze = a[2] + dz * lam
                    hidden = bool(z[y, x] < ze - f32(depth_bias))
                    if hidden and use_winner:
                        w = int(winner[y, x])
                        v = -1 if partners is None else int(partners[i, e])
                        if w == i or (v >= 0 and w == v >> 1):
                            hidden = False
                    cls.append(1 if hidden else 2)
                t = 0
                while t <= el:
                    if cls[t] == 0:
                        t += 1
                        continue
                    t1 = t
                    while t1 + 1 <= el and cls[t1 + 1] == cls[t]:
                        t1 += 1
                    if el == 0:
                        u0, u1 = f32(0), f32(1)
                    else:
                        u0 = max(f32(t) - f32(0.5), f32(0)) / f32(el)
                        u1 = min(f32(t1) + f32(0.5), f32(el)) / f32(el)
                    runs.append((3 * i + e, t, t1, cls[t]))
                    ends.append((a[0] * (f32(1) - u0) + b[0] * u0, a[1] * (f32(1) - u0) + b[1] * u0,
                                 a[0] * (f32(1) - u1) + b[0] * u1, a[1] * (f32(1) - u1) + b[1] * u1))
                    t = t1 + 1
    return np.array(runs, np.int32).reshape(-1, 4), np.array(ends, np.float32).reshape(-1, 4)


def test_the_vectorised_model_equals_the_loop(oracle):
    from cython3dmodelrenderer_amd.wireframe import edge_partners
    seed, T, H, W = 23, 200, 64, 64
    tri, col, nrm = random_soup(np.random.default_rng(seed), T, 64, size_px=(2.0, 30.0))
    cam = oracle.OracleFiller(H, W, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    rng = np.random.default_rng(seed + 1)
    mask = rng.integers(0, 256, T).astype(np.uint8)
    partners = rng.integers(-2, 2 * T, (T, 3)).astype(np.int32)          # (a soup has no partners of its own)
    perm = rng.permutation(T).astype(np.uint32)
    perm[::7] = T + 3
    moved = np.empty_like(tri)
    moved[perm[perm < T]] = tri[perm < T]
    total = 0
    for kw in (dict(), dict(partners=partners), dict(edges=mask, depth_bias=0.0), dict(use_winner=False, partners=partners),
               dict(edges=mask, partners=partners, y0=20, y1=47), dict(edges=mask, pos_of=perm, partners=partners)):
        arrays = moved if "pos_of" in kw else tri
        want = _loop_model(cam.winner, cam.z_buffer, arrays, cam.proj_mat, **kw)
        kw = dict(kw)
        got = runs_ref.line_runs(cam.winner, cam.z_buffer, arrays, kw.pop("pos_of", None), cam.proj_mat, **kw)
        assert got[0].dtype == np.int32 and got[1].dtype == np.float32
        assert_bit_equal(got[0], want[0], f"the soup, {sorted(kw)}: runs")
        assert_bit_equal(got[1], want[1], f"the soup, {sorted(kw)}: ends")
        assert (got[0][:, 3] == 1).sum() > 20 and (got[0][:, 3] == 2).sum() > 20
        order = got[0][:, 0].astype(np.int64) * 2 ** 32 + got[0][:, 1]
        assert (np.diff(order) > 0).all()                                # ordered by (s, t0), no two runs alike
        total += len(got[0])
    assert total > 1500
    assert edge_partners(tri).max() < 0
    # the hand-built set: lines of length 0, through every side of the frame, skipped ones (those near the frame)
    odd, _ = hidden_ref.odd_segments()
    short = np.array([k for k in range(len(odd)) if k not in hidden_ref.FAR_AWAY])
    P = pass_edges.P
    winner = rng.integers(-1, len(short) + 2, (64, 64)).astype(np.int32)
    z = rng.choice(np.float32([0.5, 0.7, 0.75, 0.8, 1e6, np.nan, np.inf, -np.inf]), (64, 64))
    part = rng.integers(-2, 2 * len(short), (len(short), 3)).astype(np.int32)
    for kw in (dict(), dict(partners=part, depth_bias=0.0), dict(y0=9, y1=41)):
        want = _loop_model(winner, z, odd[short], P, **kw)
        got = runs_ref.line_runs(winner, z, odd[short], None, P, **kw)
        assert_bit_equal(got[0], want[0], f"the odd segments, {sorted(kw)}: runs")
        assert_bit_equal(got[1], want[1], f"the odd segments, {sorted(kw)}: ends")
        assert len(got[0]) > 40
    # a line of length 0 is one run from A to B, whatever they round to
    runs, ends = runs_ref.line_runs(winner, z, odd[4:5], None, P)
    proj = tex_ref.project(odd[4:5], P, 64, 64)
    assert runs.tolist() == [[e, 0, 0, runs[e, 3]] for e in range(3)]
    assert_bit_equal(ends[0], np.float32([proj[0, 0, 0], proj[0, 0, 1], proj[0, 1, 0], proj[0, 1, 1]]), "el = 0: u0 = 0, u1 = 1")


# ---- on the oracle's frames ----------------------------------------------------------------------------------------

class _Frame(Frame):
    def runs(self, **kw):
        return runs_ref.line_runs(self.cam.winner, self.cam.z_buffer, self.tri, None, self.cam.proj_mat, **kw)


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}       # test_hidden_cpu.py's scenes

soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)

# (recorded from a CPU prototype of the contract on the oracle's frame: the figures the README quotes)
COUNTS = {
    "all edges, own triangle only": dict(segments=41442, steps=133478, runs=43763, visible=17339, hidden=26424, one_step=10366, longest=21),
    "once + partners": dict(segments=20721, steps=66739, runs=21876, visible=8668, hidden=13208, one_step=5181, longest=21),
    "30 degree mask, once + partners": dict(segments=5061, steps=13691, runs=5451, visible=2250, hidden=3201, one_step=1860, longest=17),
}


def test_the_counts_on_trex_and_on_the_picket_fence(trex, oracle):
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges, half_edges_once
    partners = edge_partners(trex.tri)
    got = {}
    for name, kw in (("all edges, own triangle only", dict()),
                     ("once + partners", dict(edges=half_edges_once(None, partners), partners=partners)),
                     ("30 degree mask, once + partners", dict(edges=half_edges_once(feature_edges(trex.tri, 30.0), partners), partners=partners))):
        c = {}
        trex.runs(counts=c, **kw)
        print(f"T-Rex 256^2, bias 1e-3, winner rule, {name}: {c}")
        got[name] = c
    assert got == COUNTS
    # the fence: one workgroup, 108 trips of 256 candidates, runs longer than a trip
    n = runs_ref.FENCE
    tri, col, nrm = runs_ref.picket_fence()
    cam = oracle.OracleFiller(n, n, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    proj = tex_ref.project(tri, cam.proj_mat, n, n)
    assert np.abs(proj[0, :, :2] - np.float32([[4.3, 20.2], [315.6, 24.7], [160.2, 300.4]])).max() < 1e-3
    c = {}
    runs, ends = runs_ref.line_runs(cam.winner, cam.z_buffer, tri, None, cam.proj_mat, counts=c)
    print(f"the picket fence: {c}")
    assert (c["segments"], c["steps"], c["runs"], c["visible"], c["hidden"], c["longest"]) == (132, 27614, 304, 218, 86, 309)
    assert [int((runs[:, 0] == e).sum()) for e in range(3)] == [87, 43, 45]
    c = {}
    runs_ref.line_runs(cam.winner, cam.z_buffer, tri, None, cam.proj_mat, counts=c, y0=30, y1=62)
    assert c["runs"] == 96


def _painted(f, runs, **kw):
    """The runs painted into a plane with max: every step of a run gives its pixel the run's class."""
    S = hidden_ref.segments(f.tri, f.cam.proj_mat, f.H, f.W, kw.get("edges"))
    n, x, y, t, el, xm = hidden_ref.steps(S, f.H, f.W)
    key = (3 * S["i"] + S["e"])[n] * 2 ** 32 + t
    first = runs[:, 0].astype(np.int64) * 2 ** 32 + runs[:, 1]
    k = np.searchsorted(first, key, side="right") - 1
    assert (k >= 0).all() and (runs[k, 0] == key >> 32).all() and (t <= runs[k, 2]).all()      # every step lies in a run
    assert (runs[:, 2] - runs[:, 1] + 1).sum() == len(n)                                        # and the runs hold nothing else
    plane = np.zeros((f.H, f.W), np.uint8)
    np.maximum.at(plane, (y, x), runs[k, 3].astype(np.uint8))
    return plane


def test_painting_the_runs_gives_the_hidden_passs_classes(trex, soups):
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    for name, f in (("trex", trex), ("soup71", soups[71])):
        for kw in (dict(), dict(depth_bias=0.0, use_winner=False), dict(edges=feature_edges(f.tri, 30.0))):
            runs, ends = f.runs(**kw)
            want = hidden_ref.classes(f.cam.winner, f.cam.z_buffer, f.tri, None, f.cam.proj_mat, dash=(1, 0), **kw)
            assert_bit_equal(_painted(f, runs, **kw), want, f"{name}, {sorted(kw)}: the runs painted with max")
            assert (want == 1).sum() > 100 and (want == 2).sum() > 100
            # clipped to the frame: a run's points lie on the UNROUNDED edge, within half a pixel of rounding at each end,
            # half a pixel of the line's minor axis and half a step beyond the first and last pixel of the frame
            assert (ends >= -1.5).all() and (ends[:, [0, 2]] <= f.W + 0.5).all() and (ends[:, [1, 3]] <= f.H + 0.5).all()


ENDS64_MEASURED = 2.670e-5           # pixels; measured with this model: see the docstring below


def test_the_ends_against_float64(trex, soups):
    """The end points of every run of the three frames, all edges, in float32 and in float64 from the same float32 projected
    corners.  u is a quotient of two exactly represented numbers (one rounding), 1 - u another, and a coordinate two
    products and a sum of values up to 256: a handful of roundings of 2^-24 relative on coordinates below 2^8 (and a little
    beyond the frame for edges that leave it) — differences of a few 2^-16 pixels are what the formats allow.  Measured with
    this model: 1.831e-05 on T-Rex, 2.077e-05 on seed 51, 2.670e-05 on seed 71.  The bound is ten times the largest: the
    margin is for frames not measured.  A check of the model's statements, not a bound on the kernel, which is held to bit
    equality with the float32 model."""
    worst = 0.0
    for name, f in (("trex", trex), ("soup51", soups[51]), ("soup71", soups[71])):
        r32, e32 = f.runs()
        r64, e64 = f.runs(dtype=np.float64)
        assert e32.dtype == np.float32 and e64.dtype == np.float64 and len(r32) > 5000 and np.isfinite(e64).all()
        assert_bit_equal(r32, r64, f"{name}: the runs are the float32 model's")
        diff = float(np.abs(e32.astype(np.float64) - e64).max())
        print(f"{name}: largest |ends - ends64| = {diff:.3e} pixels over {len(r32)} runs")
        worst = max(worst, diff)
    print(f"largest |ends - ends64| over the three frames = {worst:.3e} pixels (bound {10 * ENDS64_MEASURED:.3e})")
    assert 0 < worst <= 10 * ENDS64_MEASURED


# ---- half_edges_once -----------------------------------------------------------------------------------------------

def test_half_edges_once(trex):
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges, half_edges_once
    tri = trex.tri
    T = len(tri)
    partners = edge_partners(tri)
    once = half_edges_once(None, partners)
    assert once.dtype == np.uint8 and once.shape == (T,)
    assert int(np.unpackbits(once).sum()) == 20721 and 3 * T == 41442
    S = hidden_ref.segments(tri, trex.cam.proj_mat, 256, 256, once)
    assert len(S["i"]) == 20721
    # each edge once: the kept half-edges' end points, as unordered pairs of bit patterns, are all different and are
    # the mesh's edges
    def keys(mask):
        i, e = np.nonzero((mask[:, None] >> np.arange(3)) & 1)
        a, b = tri[i, e].view(np.uint32), tri[i, (e + 1) % 3].view(np.uint32)
        swap = np.zeros(len(i), bool)
        for c in (2, 1, 0):
            swap = np.where(a[:, c] != b[:, c], a[:, c] > b[:, c], swap)
        return np.concatenate([np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)], 1)
    kept, every = keys(once), keys(np.full(T, 7, np.uint8))
    assert len(np.unique(kept, axis=0)) == len(kept) == len(np.unique(every, axis=0))
    # idempotent; the statements in a plain loop; numpy against torch on the CPU
    for mask in (None, feature_edges(tri, 30.0), np.random.default_rng(3).integers(0, 256, T).astype(np.uint8)):
        got = half_edges_once(mask, partners)
        assert_bit_equal(got, runs_ref.half_edges_once(mask, partners), "against the loop")
        assert_bit_equal(half_edges_once(got, partners), got, "idempotent")
        t = half_edges_once(None if mask is None else torch.from_numpy(mask), torch.from_numpy(partners))
        assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device.type == "cpu"
        assert_bit_equal(t.numpy(), got, "torch against numpy")
        assert_bit_equal(half_edges_once(mask, torch.from_numpy(partners)).numpy(), got, "a numpy mask with a tensor table")
        assert (got & ~(np.uint8(7) if mask is None else mask & 7) == 0).all()       # bits are only cleared; 3 to 7 come out 0
    # a half-edge whose twin is not drawn stays; borders and edges of three faces stay
    lone = np.zeros(T, np.uint8)
    i = int(np.nonzero(partners[:, 0] >> 1 < np.arange(T))[0][0])
    lone[i] = 1
    assert_bit_equal(half_edges_once(lone, partners), lone, "the twin is not drawn")
    cyl = contour_ref.place(contour_ref.open_cylinder())
    pc = edge_partners(cyl)
    assert (pc == -1).any()
    oc = half_edges_once(None, pc)
    bits = ((oc[:, None] >> np.arange(3)) & 1).astype(bool)
    assert bits[pc < 0].all() and int(bits.sum()) == int((pc < 0).sum()) + int((pc >= 0).sum()) // 2
    assert half_edges_once(None, np.zeros((0, 3), np.int32)).shape == (0,)
    for bad in (partners.astype(np.int64), partners[:, :2]):
        with pytest.raises(ValueError, match="partners must be int32"):
            half_edges_once(None, bad)
    with pytest.raises(ValueError, match="edges must be uint8"):
        half_edges_once(np.zeros(T - 1, np.uint8), partners)


# ---- write_svg -----------------------------------------------------------------------------------------------------

SVG = "{http://www.w3.org/2000/svg}"


def _drawing(runs, ends, H, W):
    from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import LineDrawing
    return LineDrawing(torch.from_numpy(np.ascontiguousarray(runs)), torch.from_numpy(np.ascontiguousarray(ends)), H, W)


def test_write_svg(trex, tmp_path):
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges, half_edges_once, write_svg
    partners = edge_partners(trex.tri)
    runs, ends = trex.runs(edges=half_edges_once(feature_edges(trex.tri, 30.0), partners), partners=partners)
    d = _drawing(runs, ends, 256, 256)
    assert len(d) == 5451 and tuple(d.visible().shape) == (2250, 4) and tuple(d.hidden().shape) == (3201, 4)
    path = tmp_path / "trex.svg"
    assert write_svg(str(path), d, scale=2.0, background="#fff") is None
    root = ET.parse(str(path)).getroot()
    assert root.tag == SVG + "svg" and root.get("width") == "512.000" and root.get("viewBox") == "0 0 512.000 512.000"
    kids = list(root)
    assert [k.tag for k in kids] == [SVG + "rect", SVG + "g", SVG + "g"] and kids[0].get("fill") == "#fff"
    hidden, visible = kids[1], kids[2]                                  # the visible group paints over the hidden one
    assert (hidden.get("class"), visible.get("class")) == ("hidden", "visible")
    assert len(hidden) == 3201 and len(visible) == 2250 and {k.tag for k in hidden} | {k.tag for k in visible} == {SVG + "line"}
    assert hidden.get("stroke-dasharray") == "4,4" and hidden.get("stroke-opacity") == "0.5" and visible.get("stroke-dasharray") is None
    assert hidden.get("stroke") == visible.get("stroke") == "#000" and visible.get("stroke-width") == "1"
    # the centre of pixel (x, y) is at (x + 0.5, y + 0.5) * scale, three decimals
    first = ends[runs[:, 3] == 2][0].astype(np.float64)
    assert [visible[0].get(k) for k in ("x1", "y1", "x2", "y2")] == ["%.3f" % ((v + 0.5) * 2.0) for v in first]
    # a file object; hidden=False; the other arguments
    buf = io.StringIO()
    write_svg(buf, d, stroke="red", width=0.5, hidden=False)
    root = ET.fromstring(buf.getvalue().split("?>", 1)[1])
    assert [k.get("class") for k in root] == ["visible"] and len(root[0]) == 2250 and root[0].get("stroke") == "red"
    assert root[0].get("stroke-width") == "0.5" and root.get("width") == "256.000"
    buf = io.StringIO()
    write_svg(buf, d, hidden_dash=(2, 6.5), hidden_opacity=0.25, stroke='a"<b')
    root = ET.fromstring(buf.getvalue().split("?>", 1)[1])
    assert root[0].get("stroke-dasharray") == "2,6.5" and root[0].get("stroke-opacity") == "0.25" and root[0].get("stroke") == 'a"<b'
    with pytest.raises(ValueError, match="scale"):
        write_svg(io.StringIO(), d, scale=0)
    # an empty drawing is a valid picture
    buf = io.StringIO()
    write_svg(buf, _drawing(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), 8, 9))
    root = ET.fromstring(buf.getvalue().split("?>", 1)[1])
    assert [len(g) for g in root] == [0, 0] and root.get("height") == "8.000"
    assert inspect.signature(write_svg).parameters["hidden_dash"].default == (4, 4)


def test_a_closed_visible_loop_closes_exactly(oracle):
    """One triangle in front of nothing: three fully visible edges, each ONE run from A to B bit for bit, so that the text of
    every corner appears exactly twice, once in each of the two edges that meet there."""
    from cython3dmodelrenderer_amd.wireframe import write_svg
    tri = np.ascontiguousarray(pass_edges.unproject(np.float64([[10.3, 50.7, 30.2]]), np.float64([[11.9, 20.1, 55.6]]), 1.0, 64, 64))
    winner = np.full((64, 64), -1, np.int32)
    z = np.full((64, 64), 1e6, np.float32)
    runs, ends = runs_ref.line_runs(winner, z, tri, None, pass_edges.P)
    assert runs[:, [0, 1, 3]].tolist() == [[0, 0, 2], [1, 0, 2], [2, 0, 2]]
    proj = tex_ref.project(tri, pass_edges.P, 64, 64)[0, :, :2]
    corners = {c.tobytes() for c in proj}
    assert {ends[k, :2].tobytes() for k in range(3)} | {ends[k, 2:].tobytes() for k in range(3)} == corners      # A and B, bit for bit
    buf = io.StringIO()
    write_svg(buf, _drawing(runs, ends, 64, 64), scale=3.0)
    root = ET.fromstring(buf.getvalue().split("?>", 1)[1])
    lines = list(root[1])
    points = [(ln.get("x1"), ln.get("y1")) for ln in lines] + [(ln.get("x2"), ln.get("y2")) for ln in lines]
    assert len(lines) == 3 and len(set(points)) == 3 and all(points.count(p) == 2 for p in set(points))


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses, LineDrawing  # noqa: E402


class FakeFiller(fake_filler_base()):
    """The protocol of the two mixins on CPU tensors; the launches are the host model."""

    def _model(self, winner, z, tri, T, pos_of, P, edges, partners, bias, y0, y1, flags):
        return runs_ref.line_runs(winner.numpy(), z.numpy(), tri.numpy()[:T], pos_of, P, edges=None if edges is None else edges.numpy(),
                                  partners=None if partners is None else partners.numpy(), depth_bias=bias, use_winner=bool(flags & 1),
                                  y0=y0, y1=y1)

    def _launch_pass(self, entry, args):
        winner, z, tri, T, pos_of, P, edges, partners, bias = args[:9]
        h, w, y0, y1, flags = args[-5:]
        assert winner is self.winner_buffer and z is self.z_buffer and (h, w, y0, y1) == (self.h, self.w, self.y0, self.y1)
        assert type(bias) is float and type(T) is int
        runs, ends = self._model(winner, z, tri, T, pos_of, P, edges, partners, bias, y0, y1, flags)
        if entry == "crender_wire_runs_count":
            (counts,) = args[9:-5]
            assert counts.dtype == torch.int32 and tuple(counts.shape) == (runs_ref.groups(T),)
            counts.copy_(torch.from_numpy(runs_ref.group_counts(runs, T).view(np.int32)))
        else:
            assert entry == "crender_wire_runs_emit"
            offsets, N, d_runs, d_ends = args[9:-5]
            counts = runs_ref.group_counts(runs, T).astype(np.int64)
            assert offsets.dtype == torch.int64 and np.array_equal(offsets.numpy(), np.cumsum(counts) - counts) and N == len(runs)
            assert d_runs.dtype == torch.int32 and d_ends.dtype == torch.float32 and tuple(d_runs.shape) == (N, 4) == tuple(d_ends.shape)
            d_runs.copy_(torch.from_numpy(runs))
            d_ends.copy_(torch.from_numpy(ends))
        self.events.append((entry, T, None if edges is None else edges.numpy().copy(), partners is not None, flags))


def test_line_runs_runs_the_protocol_and_only_reads(soups):
    s = soups[71]
    T = len(s.tri)
    f = FakeFiller(s)
    view = f.get_color_buffer()
    assert f._host_fresh
    f.events.clear()
    d = f.line_runs()
    assert isinstance(d, LineDrawing) and (d.height, d.width) == (256, 256)
    assert f.events == ["push", "settle", ("crender_wire_runs_count", T, None, False, 1), ("crender_wire_runs_emit", T, None, False, 1)]
    assert f._host_fresh and f.get_color_buffer() is view                # the planes are only read: the views stay fresh
    runs, ends = s.runs()
    assert len(d) == len(runs) > 3000
    assert_bit_equal(d.runs.numpy(), runs, "the defaults: bias 1e-3, the winner rule")
    assert_bit_equal(d.ends.numpy(), ends, "the defaults: ends")
    assert_bit_equal(d.visible().numpy(), ends[runs[:, 3] == 2], "visible()")
    assert_bit_equal(d.hidden().numpy(), ends[runs[:, 3] == 1], "hidden()")
    assert_bit_equal(f.color_buffer.numpy(), s.cam.color_buffer, "the colours")
    mask = np.random.default_rng(5).integers(0, 256, T).astype(np.uint8)
    partners = np.random.default_rng(6).integers(-2, 2 * T, (T, 3)).astype(np.int32)
    d = f.line_runs(edges=mask, partners=torch.from_numpy(partners), depth_bias=0, use_winner=False)
    assert np.array_equal(f.events[-1][2], mask) and f.events[-1][3:] == (True, 0)
    assert_bit_equal(d.runs.numpy(), s.runs(edges=mask, partners=partners, depth_bias=0.0, use_winner=False)[0], "with operands")
    # a row strip, and a frame with nothing in its rows: no emit
    g = FakeFiller(s, row_strip=(37, 75))
    assert_bit_equal(g.line_runs().runs.numpy(), s.runs(y0=37, y1=75)[0], "the strip")
    g = FakeFiller(s)
    g.events.clear()
    d = g.line_runs(edges=np.zeros(T, np.uint8))
    assert [e[0] for e in g.events[2:]] == ["crender_wire_runs_count"]
    assert len(d) == 0 and tuple(d.runs.shape) == (0, 4) == tuple(d.ends.shape) and d.runs.dtype == torch.int32 and d.ends.dtype == torch.float32


def test_line_runs_refuses_before_anything_is_launched(soups):
    s = soups[71]
    T = len(s.tri)
    f = FakeFiller(s)
    f._pipeline = object()
    with pytest.raises(ValueError, match=r"line_runs is not available on a swap chain \(pipeline=True\)"):
        f.line_runs()
    with pytest.raises(ValueError, match="line_runs needs the winner plane"):
        FakeFiller(s, track_winner=False).line_runs()
    f = FakeFiller(s)
    f._inputs = None
    with pytest.raises(ValueError, match="line_runs: no frame has been rendered"):
        f.line_runs()
    f = FakeFiller(s)
    f._last_flags = 0
    with pytest.raises(ValueError, match="line_runs: the last frame did not start from cleared buffers"):
        f.line_runs()
    f = FakeFiller(s)
    for bias in (NAN, INF, None, True, "1"):
        with pytest.raises(ValueError, match="depth_bias"):
            f.line_runs(depth_bias=bias)
    for bad, word in ((np.zeros(T - 1, np.uint8), rf"T = {T}.*\({T - 1},\)"), (np.zeros(T, np.int32), rf"T = {T}.*int32")):
        with pytest.raises(ValueError, match=word):
            f.line_runs(edges=bad)
    for bad, word in ((np.zeros((T, 3), np.int64), "partners must be int32"), (np.zeros((T, 2), np.int32), "partners must be int32"),
                      (np.zeros((T + 1, 3), np.int32), rf"holds {T + 1} triangles, the last frame drew {T}")):
        with pytest.raises(ValueError, match=word):
            f.line_runs(partners=bad)
    assert f.events == []                                                # nothing was pushed, settled or launched
    sig = inspect.signature(DeferredPasses.line_runs)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("edges", None), ("partners", None), ("depth_bias", 1e-3), ("use_winner", True)]
    assert "extra synchronisation" in DeferredPasses.line_runs.__doc__       # the total's .item(), said where the caller reads
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    assert AdvancedPixelBufferFiller.line_runs is DeferredPasses.line_runs


# ---- the Renderer ----------------------------------------------------------------------------------------------

class _Mesh:
    def __init__(self, tri):
        self._vertices_by_triangles = tri


# a filler that records what the Renderer asks of it
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass hidden_line_pass line_runs shade_guro resolve contour_edges get_color_tensor",
    returns=dict(line_runs="drawing", resolve="resolved", contour_edges=lambda f, partners, **kw: np.full(len(partners), 5, np.uint8)),
    quiet="_push_host_edits synchronize")


def test_renderer_takes_the_drawing_after_the_wire_and_hidden_passes():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges, half_edges_once
    tri = contour_ref.place(contour_ref.open_cylinder())
    model = _Mesh(tri)
    partners = edge_partners(tri)
    guro = GuroIllumination((0.3, -0.2, 1.0))

    class Plain:
        def wire_pass(self, **kw):
            pass
    with pytest.raises(ValueError, match=r"Renderer\(wireframe=\{'vector': \.\.\.\}\) needs a filler that returns the drawing as vectors.*Plain has no line_runs"):
        Renderer(Plain(), None, wireframe=dict(vector=True))
    with pytest.raises(ValueError, match="takes True or a dict"):
        Renderer(_Recorder(), None, wireframe=dict(vector=3))
    assert Renderer(Plain(), None, wireframe=dict(vector=False)).wireframe == dict(vector=False)
    # True: after the wire pass and the hidden pass, with the view's mask once and a table made once per model
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(width=2.0, feature_angle=30, hidden=True, vector=True))
    assert r.line_drawing is None
    assert r.render(model) == "colour" and r.line_drawing == "drawing"
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "shade_guro", "wire_pass", "hidden_line_pass", "line_runs",
                                       "get_color_tensor"]
    wire, runs = f.calls[3], f.calls[5]
    assert set(wire[2]) == {"width", "edges"} and set(runs[2]) == {"edges", "partners"} and runs[1] == ()
    assert np.array_equal(runs[2]["partners"], partners)
    assert np.array_equal(runs[2]["edges"], half_edges_once(feature_edges(tri, 30), partners))
    table = runs[2]["partners"]
    r.render(model)
    assert f.calls[-2][2]["partners"] is table                           # once per model
    # with the contours the table is theirs, and the mask is the view's
    f = _Recorder()
    r = Renderer(f, guro, on_device="fused", wireframe=dict(contours=True, vector=dict(depth_bias=0.0)))
    r.render(model)
    names = [c[0] for c in f.calls]
    assert names == ["set_fused_illumination", "render_model", "contour_edges", "wire_pass", "line_runs", "get_color_tensor"]
    runs = f.calls[4]
    assert runs[2]["partners"] is f.calls[2][1][0] and runs[2]["depth_bias"] == 0.0
    assert np.array_equal(runs[2]["edges"], half_edges_once(np.full(len(tri), 5, np.uint8), partners))
    # an explicit mask or table of its own wins; without a mask every edge once
    own = np.full(len(tri), 3, np.uint8)
    f = _Recorder()
    Renderer(f, guro, on_device=True, wireframe=dict(feature_angle=30, vector=dict(edges=own, partners=partners))).render(model)
    assert f.calls[4][2]["edges"] is own and f.calls[4][2]["partners"] is partners
    f = _Recorder()
    Renderer(f, guro, on_device=True, wireframe=dict(vector={})).render(model)
    assert f.calls[3] == ("wire_pass", (), {}) and np.array_equal(f.calls[4][2]["edges"], half_edges_once(None, partners))
    # supersampled: on the supersampled frame, before the resolve
    f = _Recorder()
    assert Renderer(f, guro, on_device=True, supersample=2, wireframe=dict(vector=True)).render(model) == "resolved"
    assert [c[0] for c in f.calls][-3:] == ["wire_pass", "line_runs", "resolve"]
    # without the key nothing changes
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(width=2.0))
    r.render(model)
    assert "line_runs" not in [c[0] for c in f.calls] and r.line_drawing is None
