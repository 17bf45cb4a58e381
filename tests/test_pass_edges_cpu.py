"""Conditions on the hand-built scenes of tests/pass_edges.py, checked on the host model alone: the scenes take every
window decision of the passes both ways, often enough and within one wavefront, before tests/test_pass_edges_gpu.py
holds the kernels to them; and the float32 model of the scene is still the float64 form of its own statements where
the operands are ordinary."""
import inspect
import os
import re

import numpy as np
import pytest

import aniso_ref
import mip_ref
import pass_edges as E
import shadow_ref
import tex_ref
from test_texture_cpu import PERSPECTIVE_UV_BOUND

WAVE = 64


@pytest.fixture(scope="module")
def scene(oracle):
    return E.scene()


@pytest.fixture(scope="module")
def sides(scene):
    return E.classify(scene)


def _block(c, W=E.W):
    return (c["ys"] // E.BLOCK) * ((W + E.BLOCK - 1) // E.BLOCK) + c["xs"] // E.BLOCK


def test_the_frame_has_partial_blocks_and_every_kind_of_winner(scene):
    s = scene
    assert s.winner.shape == (E.H, E.W) and E.H <= 96 and E.W <= 128
    assert E.H % 8 and E.W % 8 and E.H % 32 and E.W % 32
    for bad in (-1, -7, s.T, s.T + 5, E.INT_MAX, E.INT_MIN):
        assert (s.winner == bad).any(), bad
    by, bx = -(-E.H // 8), -(-E.W // 8)
    blocks = [s.winner[r * 8:(r + 1) * 8, c * 8:(c + 1) * 8] for r in range(by) for c in range(bx)]
    covered = [(b >= 0) & (b < s.T) for b in blocks]
    assert sum(not c.any() for c in covered) >= 1                                         # background only
    uniform = {s.class_of[b[0, 0]] for b, c in zip(blocks, covered) if c.all() and (b == b[0, 0]).all()}
    assert uniform == set(s.classes), set(s.classes) - uniform
    assert max(len({s.class_of[t] for t in b[c]}) for b, c in zip(blocks, covered) if c.any()) >= len(s.classes) - 2
    # the partial blocks at the right and at the bottom hold covered pixels
    assert ((s.winner[:, 96:] >= 0) & (s.winner[:, 96:] < s.T)).any() and ((s.winner[80:] >= 0) & (s.winner[80:] < s.T)).any()
    # d_pos_of: a permutation but for one entry beyond T, whose triangle is on the frame
    assert s.pos_of[s.gone] >= s.T and (s.winner == s.gone).sum() >= WAVE
    rest = np.delete(s.pos_of, s.gone)
    assert len(set(rest.tolist())) == s.T - 1 and rest.max() < s.T
    assert (s.moved[np.delete(np.arange(s.T), s.gone)].view(np.uint32) != s.tri[np.delete(np.arange(s.T), s.gone)].view(np.uint32)).any()


@pytest.mark.parametrize("decision", E.DECISIONS)
def test_every_decision_is_taken_both_ways_by_a_wavefronts_worth_and_within_one_block(sides, decision):
    c = sides
    fast = c[decision][:, 0]                       # the point (x, y) itself: what every pass evaluates
    print(f"{decision}: {int(fast.sum())} fast, {int((~fast).sum())} slow of {len(fast)} covered pixels")
    assert fast.sum() >= WAVE and (~fast).sum() >= WAVE
    blk = _block(c)
    both = [b for b in np.unique(blk) if fast[blk == b].any() and (~fast[blk == b]).any()]
    assert len(both) >= 1
    # and at the two neighbours the mip and aniso passes evaluate
    for p in (1, 2):
        assert c[decision][:, p].sum() >= WAVE and (~c[decision][:, p]).sum() >= WAVE


def test_slow_after_fast(sides):
    c = sides
    total = 0
    for a, b in zip(E.DECISIONS[:-1], E.DECISIONS[1:]):
        n = int((c[a][:, 0] & ~c[b][:, 0]).sum())
        print(f"{a} fast, then {b} slow: {n} pixels")
        total += n
    assert total >= WAVE
    # the quotients' own pair: the denominators inside the window, a numerator outside it (zero on an edge)
    assert int((c["fast"][:, 0] & ~c["num"][:, 0]).sum()) >= WAVE
    # z_fast holds and s falls out of the window: the corners at z = 2^39 and 2^40
    s = E.scene()
    edge = np.isin(c["t"], s.classes["z_edge"])
    assert int((edge & c["z_fast"][:, 0] & c["b"][:, 0] & ~c["s"][:, 0]).sum()) >= WAVE
    assert int((edge & c["s"][:, 0]).sum()) >= WAVE              # (and the same corners leave s inside it as often)


def test_one_corner_z_alone_outside_the_window(scene, sides):
    """A window test forgotten for one corner's z shows only where the other two pass.  An infinite z cannot show it:
    crender_project turns it into a NaN screen position, so every such pixel is NaN on any path.  A finite one can,
    where uv is made of that corner's term alone: the "z_far" triangles (z_c = 10^38, uv live at c only)."""
    s, c = scene, sides
    z = s.tri[:, :, 2][c["t"]]
    ys, xs, t, u, v = tex_ref.pixel_uv(s.winner, s.tri, E.P, s.uv, perspective=True)
    inf = np.isin(t, s.classes["z_inf"])
    assert inf.sum() >= WAVE and np.isnan(u[inf]).all() and np.isnan(v[inf]).all()
    assert np.isnan(tex_ref.project(s.tri[s.classes["z_inf"]], E.P, E.W, E.H)[np.isinf(s.tri[s.classes["z_inf"]][:, :, 2])]).all()
    far = np.isin(t, s.classes["z_far"])
    for corner in range(3):
        others = [k for k in range(3) if k != corner]
        at = far & ~E.in_window(z[:, corner]) & E.in_window(z[:, others[0]]) & E.in_window(z[:, others[1]])
        live = at & c["b"][:, 0] & c["s"][:, 0] & (np.abs(u) < 4) & (np.abs(v) < 4) & ((u != 0) | (v != 0))
        print(f"z = 1e38 at corner {corner} alone: {int(at.sum())} pixels, {int(live.sum())} with a uv of the size of a texture")
        assert live.sum() >= (WAVE if corner == 2 else 16) and not c["z_fast"][at, 0].any()
    # and each corner alone below and above the window at a moderate distance (2^-43, 2^42)
    for name in ("z_low", "z_high"):
        zc = s.tri[s.classes[name]][:, :, 2]
        alone = (~E.in_window(zc)).sum(1) == 1
        assert {int(k) for k in np.argmax(~E.in_window(zc[alone]), 1)} == {0, 1, 2}, name


def test_the_small_frame_has_denominators_under_the_window_that_are_not_zero(oracle):
    m = E.mini_scene()
    assert m.H * m.W < 1024
    proj = tex_ref.project(m.tri, E.P, m.W, m.H)
    l = np.abs(np.stack(E.edge_terms(proj, np.zeros(m.T), np.zeros(m.T))[:3], 1))
    assert ((l[m.classes["tiny"]] > 0) & (l[m.classes["tiny"]] < E.DIV_LO)).all()
    c = E.classify(m)
    assert (~c["fast"][:, 0]).sum() >= WAVE and c["fast"][:, 0].sum() >= WAVE
    blk = _block(c, m.W)
    assert any(c["fast"][blk == b, 0].any() and (~c["fast"][blk == b, 0]).any() for b in np.unique(blk))


def test_levels_weights_and_sample_counts_cover_their_edges(scene):
    s = scene
    th, tw = 64, 97
    L = len(mip_ref.layout(th, tw)[0])
    for persp in (False, True):
        _, _, _, _, rho, l0, f = mip_ref.pixel_levels(s.winner, s.tri, E.P, s.uv, th, tw, persp)
        one = np.float32(1)
        assert (rho == one).sum() >= 16                                           # rho > 1 is false AT 1
        assert ((rho > one) & (rho < one + np.float32(1e-5))).sum() >= 16         # just over
        assert ((rho < one) & (rho > one - np.float32(1e-5))).sum() >= 16         # just under
        assert ((f == 0) & (l0 > 0) & (l0 < L - 1)).sum() >= 16                   # exactly a power of two
        assert ((f != 0) & (l0 < L - 1)).sum() >= WAVE
        assert (rho == np.float32(2.0 ** (L - 1))).sum() + (rho > np.float32(2.0 ** (L - 1))).sum() >= WAVE
        assert np.isnan(rho).sum() >= WAVE
        assert set(np.unique(l0)) == set(range(L))
        N = aniso_ref.pixel_footprints(s.winner, s.tri, E.P, s.uv, th, tw, persp, 16)[6]
        assert (np.bincount(N, minlength=17)[1:] >= 16).all(), np.bincount(N)
        for A in (2, 4):
            N = aniso_ref.pixel_footprints(s.winner, s.tri, E.P, s.uv, th, tw, persp, A)[6]
            assert N.max() == A and (N == A).sum() >= WAVE and (np.bincount(N)[1:] > 0).all()


def test_the_shadow_map_holds_each_pixels_own_depth_and_its_neighbours(scene):
    s = scene
    ys, xs, t, cx, cy, depth, behind = E.shadow_points(s, s.winner)
    inside = ~behind & (cx >= 0) & (cx < E.WL) & (cy >= 0) & (cy < E.HL)
    at = s.lz[np.where(inside, cy, 0), np.where(inside, cx, 0)]
    d = np.float32
    with np.errstate(all="ignore"):
        assert (inside & (depth == at)).sum() >= WAVE                             # depth > z is false AT z
        assert (inside & (np.nextafter(depth, d(np.inf), dtype=d) == at)).sum() >= WAVE
        assert (inside & (np.nextafter(depth, d(-np.inf), dtype=d) == at)).sum() >= WAVE
    assert (inside & np.isnan(at)).sum() >= 16 and (inside & np.isposinf(at)).sum() >= 16 and (inside & np.isneginf(at)).sum() >= 16
    assert behind.sum() >= WAVE                                                   # behind the light (or NaN)
    assert (~behind & ~inside).sum() >= WAVE                                      # off the map
    assert (~behind & ((np.abs(cx) >= 2 ** 31 - 1) | (cx == E.INT_MIN))).sum() >= 16      # beyond int32
    own = inside & (s.lwinner[np.where(inside, cy, 0), np.where(inside, cx, 0)] == t)
    assert own.sum() >= WAVE                                                      # the winner rule fires
    for K in (1, 3, 5):
        counts = {}
        shadow_ref.shadow_pass(s.color, s.winner, s.tri, E.P, s.ltri, E.P, s.lz, s.lwinner, bias=E.BIAS, pcf=K, counts=counts)
        assert counts["lit"] >= WAVE and counts["shadowed"] >= WAVE
        assert counts["covered"] - counts["lit"] - counts["shadowed"] >= (WAVE if K > 1 else 0)


def test_the_float32_model_of_the_scene_stays_within_the_bound_of_float64(scene, sides):
    """tests/test_texture_cpu.py's statement on this scene, twice.

    As it stands (the bound is absolute, measured on rasterized pixels of T-Rex): on the pixels whose operands are what
    a rasterizer hands over — every decision on its fast side, the winner at least 8 px across, the pixel inside it,
    uv within one texture and the corners' z within a factor of two.

    On EVERY finite pixel with all decisions on the fast side, against the bound times max(1, max |b|) times
    max(1, max |uv|): the error of u is that of the barycentrics times the size of the uv they weigh, and a pixel
    outside its winner has barycentrics beyond [0, 1].  One class is left out of this second part, the triangles of
    less than one px^2 ("small": a hundredth of a pixel across): float64 from the same float32 corners projects them
    again, and the two projections differ by a rounding of the screen coordinate, 4e-6 px, which is a thousandth of
    such a triangle — the disagreement there measures the scene's conditioning, not the model."""
    s, c = scene, sides
    ys, xs, t, u32, v32 = tex_ref.pixel_uv(s.winner, s.tri, E.P, s.uv, perspective=True)
    with np.errstate(all="ignore"):
        _, _, _, u64, v64 = tex_ref.pixel_uv(s.winner, s.tri, E.P, s.uv, perspective=True, dtype=np.float64)
        proj = tex_ref.project(s.tri, E.P, E.W, E.H, np.float64)[t]
        b = np.stack(tex_ref.barycentrics(proj, xs, ys), 1)
        size = np.abs(E.edge_terms(proj, xs, ys)[0])
        err = np.maximum(np.abs(u32 - u64), np.abs(v32 - v64))
    assert u32.dtype == np.float32 and u64.dtype == np.float64
    finite = np.all([c[k][:, 0] for k in E.DECISIONS], 0) & np.isfinite(u64) & np.isfinite(v64) & np.isfinite(u32) & np.isfinite(v32)
    uv_size = np.abs(s.uv[t]).max((1, 2))
    z = s.tri[:, :, 2][t]
    with np.errstate(all="ignore"):
        ordinary = finite & (size >= 64) & (b.min(1) >= 0) & (b.max(1) <= 1) & (uv_size <= 1) & (z.max(1) <= 2 * z.min(1)) & (z.min(1) > 0)
    assert ordinary.sum() >= 500, int(ordinary.sum())
    print(f"perspective uv, ordinary operands: max error {float(err[ordinary].max()):.3e} over {int(ordinary.sum())} pixels")
    assert err[ordinary].max() <= PERSPECTIVE_UV_BOUND
    every = finite & (size >= 1)
    scale = np.maximum(1, np.abs(b).max(1)) * np.maximum(1, uv_size)
    classes = {n for n in s.classes if (every & (s.class_of[t] == n)).any()}
    print(f"perspective uv, every finite in-window pixel: max error / scaled bound "
          f"{float((err[every] / (PERSPECTIVE_UV_BOUND * scale[every])).max()):.3f} over {int(every.sum())} pixels of {sorted(classes)}")
    assert every.sum() >= 4000 and (b[every].min(1) < 0).sum() >= 1000 and (uv_size[every] > 1).sum() >= 1000
    assert classes >= {"ordinary", "aligned", "z_edge", "pow2", "rho", "aniso", "uv_zero"}
    assert (err[every] <= PERSPECTIVE_UV_BOUND * scale[every]).all()


def test_the_tall_frame_needs_a_second_trip_of_the_row_block_loop(oracle):
    t = E.tall_scene()
    blocks = -(-(E.TALL_H - E.TALL_Y0) // 8)
    assert blocks > 65535 and (E.TALL_H - E.TALL_Y0) % 8                          # more than a grid is tall; the last one partial
    covered = np.nonzero(((t.winner >= 0) & (t.winner < t.T)).any(1))[0]
    second = covered[(covered - E.TALL_Y0) // 8 >= 65535]
    assert len(second) >= 8 and covered.min() < 24 and covered.max() == E.TALL_H - 1
    assert set(covered) <= set(t.rows.tolist())
    assert t.color.nbytes * 2 + t.winner.nbytes < 64 << 20


def test_the_passes_share_one_header_that_the_build_watches_and_the_fingerprint_does_not():
    from cython3dmodelrenderer_amd import _build
    assert os.path.exists(os.path.join(_build.SRC_DIR, "winner_pass.h"))
    assert "winner_pass.h" in _build.PASS_HEADERS
    assert "PASS_HEADERS" in inspect.getsource(_build.needs_build)
    assert "winner_pass.h" not in _build.SOURCES + _build.HEADERS
    assert _build.source_sha16() == "f3a47bfc1afb1a02"
    units = ["texture.hip", "texmip.hip", "texaniso.hip", "shadow.hip"]
    text = {n: open(os.path.join(_build.SRC_DIR, n)).read() for n in units + ["mip_sample.h", "winner_pass.h"]}
    for name in ("host_f32_to_i32", "texel", "bilinear"):
        found = [n for n, t in text.items() for _ in re.finditer(r"^CR_DEV [^\n;]*\b" + name + r"\(", t, re.M)]
        assert len(found) == 1, (name, found)
    for n in units:
        assert '#include "winner_pass.h"' in text[n], n
