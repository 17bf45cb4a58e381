"""Conditions on the hand-built scenes of tests/pass_edges.py, checked on the host model alone: the scenes take every
window decision of the passes, and every select of the Phong and occlusion passes, both ways, often enough and within one wavefront, before tests/test_pass_edges_gpu.py
holds the kernels to them; and the float32 model of the scene is still the float64 form of its own statements where
the operands are ordinary.

The two wire passes, at the end: floors on what the overlay's and the outline's models do on the painted scene; the
hand-built frame that holds the hidden-line test at equality, the clamp of s on its three sides and the depth at the
closest point, with three mutants of the model that it tells apart; and the frames of lone winners, where the model
lights the pixel exactly radius_px rows or columns from a winner and no nearer radius does."""
import os
import re

import numpy as np
import pytest

import aniso_ref
import ao_ref
import mip_ref
import outline_ref
import overlay_ref
import pass_edges as E
import phong_ref
import shadow_ref
import tex_ref
from test_texture_cpu import PERSPECTIVE_UV_BOUND
from util import unit_in_build

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
    unit_in_build(_build, "pass", [], ["winner_pass.h"])
    units = ["texture.hip", "texmip.hip", "texaniso.hip", "shadow.hip"]
    text = {n: open(os.path.join(_build.SRC_DIR, n)).read() for n in units + ["mip_sample.h", "winner_pass.h"]}
    for name in ("host_f32_to_i32", "texel", "bilinear"):
        found = [n for n, t in text.items() for _ in re.finditer(r"^CR_DEV [^\n;]*\b" + name + r"\(", t, re.M)]
        assert len(found) == 1, (name, found)
    for n in units:
        assert '#include "winner_pass.h"' in text[n], n


# ---- the Phong pass ---------------------------------------------------------------------------------------------------

PHONG_AMBIENT = 0.25


def _phong_floors(s, kind, floor, rows=None, unlit_floor=None, odd_floor=None):
    """The conditions on one scene under one light set.  `rows`: the rows anything is counted on."""
    lights = s.lights[kind]
    ys, xs, t, pt, inside = E.phong_points(s)
    keep = np.ones(len(t), bool) if rows is None else np.isin(ys, rows)
    counts = {}
    out = phong_ref.phong_pass(s.color, s.winner, s.tri, E.P, s.normals, lights, ambient=PHONG_AMBIENT, counts=counts)
    assert np.isfinite(out).all()                                                 # no NaN or inf reaches the colours
    changed = (out.view(np.uint32) != s.color.view(np.uint32)).any(2)
    assert changed[ys, xs].all() and changed.sum() == len(t) == counts["covered"]
    # per light: both sides of `lit`, often enough and inside one 8 x 8 block
    n = [s.normals[ys, xs, a] for a in range(3)]
    L5, mask = phong_ref.lights5(lights)
    with np.errstate(all="ignore"):
        V = [-pt[:, a] for a in range(3)]
        vl = phong_ref.length(V)
        Vu = [v / vl for v in V]
        F_dir = np.full(len(t), np.float32(PHONG_AMBIENT))
        blk = (ys // E.BLOCK) * 100000 + xs // E.BLOCK
        for j in range(len(lights)):
            d, _ = phong_ref.light_terms([pt[:, a] for a in range(3)], Vu, n, L5[j, :3], bool(mask >> j & 1), 5)
            lit = (d > 0) & keep
            unlit = ~(d > 0) & keep
            print(f"{kind}, light {j}: {int(lit.sum())} lit, {int(unlit.sum())} unlit")
            assert lit.sum() >= floor and unlit.sum() >= (floor if unlit_floor is None or not mask >> j & 1 else unlit_floor)
            assert any(lit[blk == b].any() and unlit[blk == b].any() for b in np.unique(blk[keep]))
            if mask >> j & 1:
                F_dir = F_dir + L5[j, 3] * d
    # a surface point that is not finite: no point light and no highlight reaches the pixel — its colour times the
    # ambient term, and the diffuse term of the DIRECTIONS, which need no point (under the clamp)
    odd = ~np.isfinite(pt).all(1)
    print(f"{kind}: {int((odd & keep).sum())} points that are not finite, {int((~odd & ~inside & keep).sum())} finite ones outside their winner")
    assert (odd & keep).sum() >= (floor if odd_floor is None else odd_floor)
    same = out[ys[odd], xs[odd]].view(np.uint32) == np.minimum(s.color[ys[odd], xs[odd]] * F_dir[odd, None], np.float32(255)).view(np.uint32)
    assert same.all()
    if not mask:
        assert (F_dir == np.float32(PHONG_AMBIENT)).all()
    return int((~odd & ~inside & keep).sum())


@pytest.mark.parametrize("kind", E.LIGHT_SETS)
def test_phong_on_the_edge_scene_takes_every_select_both_ways(scene, kind):
    """Lit and unlit under every light, surface points that are NaN or infinite ("zero", "z_inf", most of "z_bad"),
    finite ones far outside their winner, channels at the clamp."""
    s = scene
    outside = _phong_floors(s, kind, WAVE)
    assert outside >= 1000
    counts = {}
    phong_ref.phong_pass(s.color, s.winner, s.tri, E.P, s.normals, s.lights[kind], ambient=PHONG_AMBIENT, clamp=100.0, counts=counts)
    assert counts["clamped"] >= 16
    ys, xs, t, pt, _ = E.phong_points(s)
    odd = ~np.isfinite(pt).all(1)
    assert set(s.classes["zero"] + s.classes["z_inf"]) <= set(t[odd].tolist())
    assert odd[np.isin(t, s.classes["zero"] + s.classes["z_inf"])].all()
    assert odd[np.isin(t, s.classes["z_bad"])].sum() > (~odd)[np.isin(t, s.classes["z_bad"])].sum()


def test_the_light_sets_hold_what_they_are_for(scene):
    s = scene
    assert [len(s.lights[k]) for k in E.LIGHT_SETS] == [1, 1, 4]
    assert "position" in s.lights["point"][0] and s.lights["direction"][0]["direction"] == E.LIGHT
    z = s.tri[s.classes["ordinary"]][:, :, 2]
    assert z.min() < s.lights["point"][0]["position"][2] < z.max()               # inside the ordinary triangles' depths
    four = s.lights["four"]
    assert ["position" in l for l in four] == [True, False, True, True]
    assert four[3]["position"] == (0.0, 0.0, 0.0) and four[3]["diffuse"] == four[3]["specular"] == 0.0
    assert len({l["diffuse"] for l in four}) == 4                                 # (a light's own kd: none stands for another)
    # the third light is a corner of a triangle on the frame, and at some of its pixels the vector to it has no length
    t, c = s.on_corner
    on = np.float32(four[2]["position"]).view(np.uint32) == s.tri[t, c].view(np.uint32)
    assert on.all() and (s.winner == t).any()
    ys, xs, tt, pt, _ = E.phong_points(s)
    with np.errstate(all="ignore"):
        lv = [np.float32(four[2]["position"])[a] - pt[:, a] for a in range(3)]
        ll = phong_ref.length(lv)
    print(f"{int((ll == 0).sum())} pixels at no distance from the third light")
    assert (ll == 0).sum() >= 1
    # the origin: L = V at every pixel with a finite point
    with np.errstate(all="ignore"):
        V = [-pt[:, a] for a in range(3)]
        L = [np.float32(0) - pt[:, a] for a in range(3)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(V, L))        # (as values: 0 - 0 is +0)


@pytest.mark.parametrize("kind", E.LIGHT_SETS)
def test_phong_on_the_small_and_on_the_tall_frame(oracle, kind):
    """The same floors at 16.  The tall frame holds ordinary triangles only (its arrays stay as they are), so no point
    on it fails to be finite; and LIGHT leaves 13 of its rows' 129 covered pixels unlit, normals and direction both
    being given: the floor of the directions' unlit side is 8 there, one block's rows of one column."""
    _phong_floors(E.mini_scene(), kind, 16)
    t = E.tall_scene()
    _phong_floors(t, kind, 16, rows=t.rows, unlit_floor=8, odd_floor=0)


# ---- the occlusion pass -------------------------------------------------------------------------------------------------

def _ao(s, table=E.TABLE, radius_px=8, radius=None, pos_of=False, **kw):
    counts = {}
    out = ao_ref.ao_pass(s.color, s.z, s.winner, s.moved if pos_of else s.tri, E.P, s.normals, table,
                         radius=s.ao_radius if radius is None else radius, radius_px=radius_px,
                         pos_of=s.pos_of if pos_of else None, T=s.T, counts=counts, **kw)
    assert not np.isnan(out).any()
    return out, counts


def test_the_z_plane_and_the_tap_table(scene):
    import test_ao_gpu
    s = scene
    assert E.TABLE == test_ao_gpu.TABLE and len(E.TABLE) == 16
    assert abs(s.px - 0.01) < 1e-6 and abs(E.mini_scene().px - 1 / 28) < 1e-6
    c = ao_ref.constants(E.P, E.W, E.H, 1.0, 1)
    assert abs(float(c[2]) - 0.01) < 1e-6 and abs(float(c[3]) - 0.0119) < 1e-4
    P16 = E.P.reshape(16)                                                        # crender_ao_shade's shape check
    assert all(P16[i] == 0 for i in (1, 2, 4, 6, 8, 9, 12, 13)) and all(np.isfinite(P16[i]) and P16[i] != 0 for i in (0, 5, 14))
    for m in (s, E.mini_scene()):
        z = m.z
        assert z.shape == (m.H, m.W) and z.dtype == np.float32
        for v in (np.inf, -np.inf, np.float32(E.P[2, 2]), np.float32(1e6)):
            assert (z == v).sum() >= 3, v
        assert np.isnan(z).sum() >= 3
        with np.errstate(all="ignore"):
            zv = np.float32(E.P[3, 2]) / (z - np.float32(E.P[2, 2]))
        usual = np.isfinite(zv) & (np.abs(zv - 1) <= 3.001 * m.px)
        assert 0.04 < 1 - usual.mean() < 0.12 and (zv[usual].max() - zv[usual].min()) > 5.5 * m.px
    assert abs(s.ao_radius - 6 * s.px) < 1e-9


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("face", [False, True])
def test_ao_on_the_edge_scene_takes_every_select_both_ways(scene, face, rotate):
    s = scene
    got = {}
    for pos_of in (False, True):
        out, c = _ao(s, face=face, rotate=rotate, pos_of=pos_of)
        print(f"face={face} rotate={rotate} pos_of={pos_of}: {c['occluded']} occluded of {c['covered']}, {c['taps_taken']} taps taken")
        assert c["occluded"] >= WAVE and c["covered"] - c["occluded"] >= WAVE and c["taps_taken"] > 0
        got[pos_of] = out
    if face:                     # the triangle d_pos_of drops is not written, and still occludes
        assert (got[True] != got[False]).any()
        gone = s.winner == s.gone
        assert (got[True][gone] == s.color[gone]).all() and (got[False][gone] != s.color[gone]).any()
    else:
        assert (got[True] == got[False]).all()
    out, c = _ao(s, table=E.HALO_TABLE, radius_px=32, radius=s.halo_radius, face=face, rotate=rotate)
    assert c["taps_taken"] >= 100
    # a strip: rows 5 .. 77 with pixels just outside that WOULD occlude
    whole, _ = _ao(s, face=face, rotate=rotate)
    strip, _ = _ao(s, face=face, rotate=rotate, y0=5, y1=77)
    assert (strip[5:77] != whole[5:77]).any() and (strip[:5] == s.color[:5]).all() and (strip[77:] == s.color[77:]).all()


def test_ao_face_normals_meet_overflow_nothing_and_nan_and_a_flip_test_at_zero(scene):
    """The face mode's cross product overflows to inf ("huge", "z_high"), vanishes ("zero") and is NaN ("z_bad",
    "z_inf") on triangles the frame shows; and `s > 0` is told from `s >= 0`: at a z of +-inf the view depth is
    -+0, the pixel's point the origin and s exactly 0, and under a radius that takes every tap the other rule gives
    other colours."""
    s = scene
    ys, xs, t = tex_ref.covered(s.winner, s.T)
    c = s.tri[t]
    with np.errstate(all="ignore"):
        g = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    assert np.isinf(g).any(1).sum() >= WAVE and np.isnan(g).any(1).sum() >= WAVE and (g == 0).all(1).sum() >= WAVE
    at_zero = np.isinf(s.z[ys, xs]) & np.isfinite(g).all(1) & (g != 0).any(1)
    assert at_zero.sum() >= WAVE
    real = ao_ref.face_normals

    def other(tri_t, Pp):
        A, B, C = tri_t[:, 0], tri_t[:, 1], tri_t[:, 2]
        e1 = [B[:, k] - A[:, k] for k in range(3)]
        e2 = [C[:, k] - A[:, k] for k in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        sgn = (n[0] * Pp[0] + n[1] * Pp[1]) + n[2] * Pp[2]
        return [np.where(sgn >= 0, -v, v) for v in n]
    want, _ = _ao(s, face=True, radius=1e30)
    try:
        ao_ref.face_normals = other
        flipped, _ = _ao(s, face=True, radius=1e30)
    finally:
        ao_ref.face_normals = real
    differ = (want != flipped).any(2)
    print(f"{int(differ.sum())} pixels tell s > 0 from s >= 0")
    assert differ.sum() >= 16 and np.isinf(s.z[differ]).all()


def test_ao_on_the_small_frame(oracle):
    m = E.mini_scene()
    for R, table, radius in ((8, E.TABLE, m.ao_radius), (32, E.HALO_TABLE + E.TABLE, m.halo_radius)):
        for face in (False, True):
            counts = {}
            out = ao_ref.ao_pass(m.color, m.z, m.winner, m.tri, E.P, m.normals, table, radius=radius, radius_px=R, face=face,
                                 counts=counts)
            assert not np.isnan(out).any()
            assert counts["occluded"] >= 16 and counts["covered"] - counts["occluded"] >= 16 and counts["taps_taken"] > 0
    assert m.H < 32 and m.W < 32                                                 # inside one tile, smaller than the halo


# ---- the wire passes: the overlay and the outline -----------------------------------------------------------------------

def _overlay(s, **kw):
    counts = {}
    out = overlay_ref.wire_pass(s.color, s.winner, s.tri, E.P, counts=counts, **kw)
    assert not np.isnan(out).any()
    on = (out.view(np.uint32) != s.color.view(np.uint32)).any(2)
    return out, counts, on


def _outline(s, **kw):
    counts = {}
    out = E.outline_model(s, counts=counts, **kw)
    assert not np.isnan(out).any()
    return out, counts


def test_the_scenes_gain_an_edge_mask_and_the_tall_frame_a_z_plane(scene):
    """What `_wired` adds: an edge mask with every value of the three low bits and bits above them, and a z plane on
    the tall frame alone (the other two keep the occlusion pass's)."""
    for s in (scene, E.mini_scene(), E.tall_scene()):
        assert s.edges.dtype == np.uint8 and s.edges.shape == (s.T,) and s.z.shape == (s.H, s.W) and s.z.dtype == np.float32
    assert set((scene.edges & 7).tolist()) == set(range(8)) and (scene.edges > 7).sum() > scene.T // 2
    t = E.tall_scene()
    assert np.isnan(t.z[t.rows]).any() and np.isinf(t.z[t.rows]).any()


def test_the_overlay_on_the_edge_scene(scene):
    s = scene
    _, c, _ = _overlay(s)
    print(f"overlay, defaults: {c}")
    assert c["covered"] == 7844 and (c["full"], c["partial"], c["nan"]) == (84, 205, 1309)
    assert c["full"] + c["partial"] >= 200 and c["nan"] >= 1000
    ys, xs, t, m, _ = overlay_ref.distances(s.winner, s.tri, E.P)
    with np.errstate(all="ignore"):
        on = (np.float32(1.0) - m) / np.float32(1.0) > 0
    for name, ids in s.classes.items():
        mine = np.isin(t, ids)
        print(f"overlay, {name}: {int((mine & on).sum())} on, {int((mine & ~on).sum())} off")
        if name != "aniso":                  # (its corners lie 100 px outside the frame: no pixel is near an edge)
            assert (mine & on).any() and (mine & ~on).any(), name
    assert _overlay(s, width=3.0, feather=0.5)[1]["full"] + _overlay(s, width=3.0, feather=0.5)[1]["partial"] == 528
    out, c, on = _overlay(s, width=64.0, feather=64.0, fill=(30.0, 35.0, 40.0))
    assert (c["full"] + c["partial"], c["off"]) == (6450, 1394) and c["full"] == 85       # the ramp: hi / feather is 1, the cap is met ON a line alone
    _, c, _ = _overlay(s, edges=s.edges)
    assert 100 <= c["full"] + c["partial"] < 289                                           # the mask takes edges away
    # d_pos_of: the model on the winner plane without the triangle that is sent beyond T
    out, _, _ = _overlay(s)
    gone = overlay_ref.wire_pass(s.color, s.winner_without_gone, s.tri, E.P)
    assert (out != gone).any()


def test_the_outline_on_the_edge_scene(scene):
    s = scene
    background = ~((s.winner >= 0) & (s.winner < s.T))
    _, c = _outline(s, radius_px=2)
    print(f"outline, r = 2: {c}")
    assert (c["background_on"], c["covered_on"], c["nan"]) == (83, 668, 3559)
    assert c["background_on"] >= 50 and c["nan"] > 3000
    out, c = _outline(s, radius_px=0)
    assert (c["background_on"], c["covered_on"]) == (0, 218)
    assert (out[background] == s.color[background]).all()
    _, c = _outline(s, width=3.0, feather=0.5, radius_px=3)
    assert (c["background_on"], c["covered_on"]) == (176, 1556)
    _, c = _outline(s, width=3.0, radius_px=8, depth_bias=0.0, fill=(30.0, 35.0, 40.0))
    assert (c["background_on"], c["covered_on"], c["nan"]) == (331, 3129, 7815)
    out, c = _outline(s, width=64.0, feather=64.0, radius_px=8, fill=(30.0, 35.0, 40.0))
    assert 0 < c["full"] < 500 and c["covered_on"] > 6000          # the ramp; the cap at the segments' own pixels alone
    # the depth comparison falls both ways: against a bias under which every edge counts, and one under which no
    # foreign edge does
    m = outline_ref.distances(s.winner, s.z, s.tri, E.P, radius_px=3, depth_bias=1e-3)[0]
    every = outline_ref.distances(s.winner, s.z, s.tri, E.P, radius_px=3, depth_bias=1e6)[0]
    none = outline_ref.distances(s.winner, s.z, s.tri, E.P, radius_px=3, depth_bias=-1e6)[0]
    print(f"the distance field differs at {int((m != every).sum())} pixels from every edge counting, at {int((m != none).sum())} from none")
    assert ((m != every).sum(), (m != none).sum()) == (4376, 4607)
    assert (m != every).sum() > 2000 and (m != none).sum() > 2000
    _, c = _outline(s, radius_px=2, edges=s.edges)
    assert 0 < c["background_on"] < 83
    # the small frame: a halo wider than the frame is tall
    mini = E.mini_scene()
    _, c = _outline(mini, radius_px=8)
    assert c["background_on"] >= 8 and c["covered_on"] >= 16 and mini.H < 2 * 8 + 8
    t = E.tall_scene()
    out, c = _outline(t, radius_px=2, y0=E.TALL_Y0)
    changed = np.nonzero((out != t.color).any((1, 2)))[0]
    assert c["covered_on"] >= 16 and set(changed.tolist()) <= set(t.rows.tolist()) and changed.max() >= E.TALL_H - 16
    assert (-(-E.TALL_W // E.TILE)) * (-(-(E.TALL_H - E.TALL_Y0) // E.TILE)) == 16385      # a workgroup per tile


# ---- the tie of the hidden-line test, the clamp and the depth at the closest point ------------------------------------

def _tie_field(s, less=np.less, clamp=True, ze_at_corner=False):
    """The distance field of the outline on `tie_scene`, restated for what that frame is: B draws nothing, every window
    holds A or A2 beside B and never both, and the one drawn edge is edge 0.  A pixel of A (A2) takes the edge whatever
    the depths; a pixel of B within the radius of one takes it if it counts.  The mutants: `less` (the comparison of
    the depth test), `clamp` False (the distance to the LINE, s as it comes), `ze_at_corner` (the depth of corner a)."""
    d_ = np.float32
    m = np.full((s.H, s.W), np.inf, d_)
    ys, xs = np.mgrid[0:s.H, 0:s.W]
    for t, own, ring in ((E.TIE_A, s.is_a, s.ring), (E.TIE_A2, s.is_a2, s.ring2)):
        raw, _, d, ze, _ = E.tie_operands(s.proj, t, 0, xs.reshape(-1), ys.reshape(-1))
        a, b = s.proj[t, 0], s.proj[t, 1]
        with np.errstate(all="ignore"):
            if not clamp:
                qx, qy = a[0] + raw * (b[0] - a[0]), a[1] + raw * (b[1] - a[1])
                cx, cy = xs.reshape(-1).astype(d_) - qx, ys.reshape(-1).astype(d_) - qy
                d = np.sqrt(cx * cx + cy * cy)
                ze = a[2] + raw * (b[2] - a[2])
            if ze_at_corner:
                ze = np.broadcast_to(a[2], ze.shape)
            counts = less(ze - d_(np.float32(E.TIE_BIAS)), s.z.reshape(-1))
            take = (own.reshape(-1) | (ring.reshape(-1) & counts)) & (d < np.inf)
        m.reshape(-1)[take] = d[take]
    return m


def test_the_tie_frame_holds_the_depth_test_at_equality_and_the_clamp_on_three_sides(oracle):
    s = E.tie_scene()
    assert s.H <= 40 and s.W <= 40 and s.edges.tolist() == [1, 0, 1]
    assert s.is_a.sum() >= 64 and s.is_a2.sum() == 25 and s.ring2.sum() >= 40
    ry, rx = np.nonzero(s.ring)
    raw, sc, d, ze, at = E.tie_operands(s.proj, E.TIE_A, 0, rx, ry)
    kind = s.kind[ry, rx]
    z = s.z[ry, rx]
    f32 = np.float32
    assert (z[kind == 0] == at[kind == 0]).all()
    assert (z[kind == 1] == np.nextafter(at[kind == 1], f32(np.inf), dtype=f32)).all()
    assert (z[kind == 2] == np.nextafter(at[kind == 2], f32(-np.inf), dtype=f32)).all()
    sides = [(raw < 0), (raw >= 0) & (raw <= 1), (raw > 1)]
    print(f"ring: {np.bincount(kind).tolist()} pixels exact / above / below; s < 0, inside, > 1: {[int(v.sum()) for v in sides]}")
    assert (np.bincount(kind, minlength=3) >= 20).all() and all(v.sum() >= 10 for v in sides)
    for side in sides:                                         # every side of the clamp meets every kind of depth
        assert set(kind[side].tolist()) == {0, 1, 2}
    assert len(np.unique(ze)) > 50 and (sc[sides[0]] == 0).all() and (sc[sides[2]] == 1).all()
    # the model takes the edge at "one ulp above" only
    m, own, nan = outline_ref.distances(s.winner, s.z, s.tri, E.P, s.edges, E.TIE_RADIUS, E.TIE_BIAS)
    taken = np.isfinite(m[ry, rx])
    assert taken[kind == 1].all() and not taken[kind != 1].any()
    assert (m[ry, rx][taken] == d[taken]).all()
    assert np.isfinite(m[s.is_a]).all() and np.isinf(m[(own == E.TIE_B) & ~s.ring]).all()
    # the edge of no length: s is 0 / 0, its distance a NaN that is never taken, its depth one that never counts
    r2 = E.tie_operands(s.proj, E.TIE_A2, 0, *np.nonzero(s.ring2 | s.is_a2)[::-1])
    assert np.isnan(r2[0]).all() and np.isnan(r2[2]).all() and np.isnan(r2[3]).all()
    assert np.isinf(m[s.is_a2 | s.ring2]).all() and nan[s.is_a2 | s.ring2].all()
    # the restatement is the model on this frame, and each mutant is not
    assert np.array_equal(_tie_field(s), m)
    for name, kw, where in (("<= for <", dict(less=np.less_equal), s.kind == 0), ("no clamp", dict(clamp=False), None),
                            ("ze at corner a", dict(ze_at_corner=True), s.ring)):
        differ = _tie_field(s, **kw) != m
        print(f"mutant {name}: differs at {int(differ.sum())} pixels")
        assert differ.sum() >= 10, name
        if where is not None:
            assert not (differ & ~where).any(), name
    assert (_tie_field(s, less=np.less_equal) != m)[s.kind == 0].all()
    # and in the colours, under a line wide enough to reach every pixel that takes the edge
    for fill in (None, (30.0, 35.0, 40.0)):
        out, c = _outline(s, width=64.0, feather=64.0, radius_px=E.TIE_RADIUS, depth_bias=E.TIE_BIAS, edges=s.edges, fill=fill)
        lit = (out != s.color).any(2)
        assert lit[s.ring & (s.kind == 1)].all() and (fill is not None or not lit[s.ring & (s.kind != 1)].any())


# ---- lone winners: the rows a wavefront skips, and the seams of the tiles ----------------------------------------------

@pytest.mark.parametrize("radius", E.SPARSE_RADII)
def test_lone_winners_light_the_pixel_exactly_radius_px_away_and_no_nearer_radius_does(oracle, radius):
    frames = E.sparse_frames(radius)
    assert len(frames) <= 16 and (E.SPARSE_H, E.SPARSE_W) == (97, 101)
    rows, cols, crossing = set(), set(), set()
    residues = {ty: set() for ty in range(3)}
    taps = 0
    for s in frames:
        # what the packing promises: the rows one wavefront reaches hold at most one winner of the tiles that stage it
        for i, (x, y, _) in enumerate(s.lone):
            for x2, y2, _ in s.lone[i + 1:]:
                assert abs(y - y2) >= 2 * radius + 2 or not (E.tiles_that_stage(x, radius) & E.tiles_that_stage(x2, radius))
        assert ((s.winner >= 0).sum(), s.T) == (len(s.lone), len(s.lone))
        out, c = _outline(s, radius_px=radius, edges=s.edges)
        nearer, _ = _outline(s, radius_px=radius - 1, edges=s.edges)
        lit, lit_nearer = (out != s.color).any(2), (nearer != s.color).any(2)
        assert c["covered"] == s.T and c["nan"] == 0
        for t, x, y, px, py in E.extreme_taps(s, radius):
            assert lit[py, px] and not lit_nearer[py, px], (radius, s.lone[t], px, py)
            taps += 1
            if s.lone[t][2] == "v" and (px // E.TILE, py // E.TILE) != (x // E.TILE, y // E.TILE):
                crossing.add(y % E.TILE)
        # nothing beyond the radius: every lit pixel is within it of its winner, rows and columns both
        ys, xs = np.nonzero(lit)
        for py, px in zip(ys, xs):
            assert any(abs(py - y) <= radius and abs(px - x) <= radius for x, y, _ in s.lone)
        for x, y, direction in s.lone:
            if direction == "v":
                rows.add(y)
                if y < 96:
                    residues[y // E.TILE].add(y % E.TILE)
            else:
                cols.add(x)
    assert rows == set(range(E.SPARSE_H)) and cols == set(E.SPARSE_COLUMNS)
    assert all(r == set(range(E.TILE)) for r in residues.values())
    assert {x for s in frames for x, _, d in s.lone if d == "v"} == set(E.SPARSE_COLUMNS)
    assert crossing == set(range(E.TILE)), sorted(set(range(E.TILE)) - crossing)
    print(f"radius {radius}: {len(frames)} frames, {taps} extreme taps lit")
    assert taps >= 2 * (E.SPARSE_H - radius) + 8                 # (each row's winner both ways where the frame allows)


def test_the_strip_frame_keeps_its_outside_winners_out_of_sight(oracle):
    s = E.sparse_strip()
    y0, y1 = E.SPARSE_STRIP
    assert y0 % 32 and y1 % 32 and [w[1] for w in s.lone] == [y0 - 1, y1, (y0 + y1) // 2]
    for radius in E.SPARSE_RADII:
        whole, _ = _outline(s, radius_px=radius, edges=s.edges)
        strip, _ = _outline(s, radius_px=radius, edges=s.edges, y0=y0, y1=y1)
        seen, lit = (whole != s.color).any(2), (strip != s.color).any(2)
        (xa, ya, _), (xb, yb, _), (xc, yc, _) = s.lone
        assert seen[y0:y0 + radius, xa].all() and seen[y1 - radius:y1, xb].all()         # the whole frame sees them
        assert not lit[:, :xc - radius].any() and not lit[:, xc + radius + 1:].any()    # the strip does not
        assert lit[yc - radius:yc + radius + 1, xc].all() and not lit[:y0].any() and not lit[y1:].any()
