"""Seeded sessions of ONE AdvancedPixelBufferFiller through its deferred passes (tests/pass_sessions.py draws the
steps): cleared frames from numpy arrays, device tensors and a DeviceModel, render_frame, composites (after which a
pass must raise and change nothing), clear(), textures bound, rebound at another size and dropped, texture passes in
every mode, shadow passes against a second filler that renders the light's view first (or against the camera itself),
two passes on one frame, edits of a colour view carried into a pass, resolves and getters — against an oracle frame and
the host models of the passes (tests/tex_ref.py, mip_ref.py, aniso_ref.py, shadow_ref.py, ssaa_ref.py) applied to it
in the same order.  The sessions of the "lit" family draw Phong and occlusion passes among them (tests/phong_ref.py,
ao_ref.py), chain up to four passes on one frame and edit the z view under an occlusion pass.  Those of the "wired"
family draw the wire pass as well, overlay and outline (tests/overlay_ref.py, outline_ref.py): between other passes on
one frame, over edited colours and an edited z view, first on a frame whose bin lists overflowed, after clear(), and
refused after a composite or for its own arguments.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest

import aniso_ref
import ao_ref
import mip_ref
import outline_ref
import overlay_ref
import pass_sessions as S
import phong_ref
import shadow_ref
import ssaa_ref
import tex_ref
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

# CRENDER_FUZZ_SOAK=n: n times the seeds (tests/test_hip_parity_gpu.py's switch)
_SOAK = max(1, int(os.environ.get("CRENDER_FUZZ_SOAK", "1")))
LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with
CENTRE = np.float32([[[0.0, 0.0, 1.5]] * 3])          # what the light's poses turn about


class _Pool:
    """The soups — (tri, col, nrm) and uv, numpy — with device copies and the DeviceModel; made once, only read."""

    def __init__(self):
        import torch
        from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
        rng = np.random.default_rng(16000)
        self.host, self.uv, self.dev = {}, {}, {}
        self.host["mixed"] = random_soup(rng, S.count("mixed"), 128, size_px=(3.0, 30.0))
        self.host["large"] = random_soup(rng, S.count("large"), 128, size_px=(20.0, 90.0))
        self.host["none"] = tuple(np.zeros((0, 3, 3), np.float32) for _ in range(3))
        T = S.count("model")
        tri, _, nrm = random_soup(rng, T, 128, size_px=(8.0, 50.0))
        idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
        uv = rng.uniform(0, 1, (T, 3, 2)).astype(np.float32)
        tex = rng.integers(0, 256, (21, 34, 3), dtype=np.uint8)
        self.model = Model(tri.reshape(-1, 3), idx, uv.reshape(-1, 2), idx, tex, nrm.reshape(-1, 3), idx, recalculate_normals=False)
        m = self.model
        self.host["model"] = (m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles)
        assert_bit_equal(self.host["model"][0], tri, "the model's triangles")
        self.device_model = DeviceModel(m)
        for name, scale in (("mixed", 1.0), ("large", 6.0), ("none", 1.0), ("model", 25.0)):
            n = self.host[name][0].shape[0]
            assert n == S.count(name)
            self.uv[name] = (rng.uniform(0, 1, (n, 3, 2)) * scale).astype(np.float32)
            self.dev[name] = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in self.host[name])
        self.textures = [rng.integers(0, 256, (th, tw, 3), dtype=np.uint8) for th, tw in S.TEXTURES]
        self.chains = [mip_ref.build_chain(t) for t in self.textures]


@pytest.fixture(scope="module")
def pool(oracle):
    return _Pool()


_SESSIONS = [(family, seed) for family in S.FAMILIES for seed in range(S.SEEDS * _SOAK)]


@pytest.mark.parametrize("family,seed", _SESSIONS, ids=[str(k) if fam == "passes" else f"{fam}-{k}" for fam, k in _SESSIONS])
def test_fuzz_a_filler_through_its_passes(oracle, pool, family, seed):
    import torch
    from cython3dmodelrenderer_amd import ambient_occlusion, shadow
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    opt, steps = S.plan(seed, family=family)
    H, W, Hl, Wl = opt["H"], opt["W"], opt["Hl"], opt["Wl"]
    f = AdvancedPixelBufferFiller(H, W, fov=45, track_winner=True, **opt["kw"])
    g = AdvancedPixelBufferFiller(Hl, Wl, fov=45, track_winner=True, **opt["light_kw"])
    ref, lig = oracle.OracleFiller(H, W, fov=45.0), oracle.OracleFiller(Hl, Wl, fov=45.0)
    y0, y1 = opt["kw"].get("row_strip", (0, H))
    light3 = [float(v) for v in oracle.guro_light(LIGHT)]
    state = dict(soup=None, bound=None, view=None)
    # fillers whose bin lists are far too small: their frames stay unchecked until a pass (or another op) looks, and
    # the session counts the overflowed frames that a legal pass was the first to meet
    small = dict(camera=bool(opt["kw"].get("bin_capacity")), light=bool(opt["light_kw"].get("bin_capacity")))
    met = dict(camera=0, light=0)

    def overflowed(filler):
        if not filler._pending:
            return False
        need, cap = filler.bin_usage()
        return need > cap
    story = []

    def what(k, more=""):
        return f"pass session {family} {seed} ({H}x{W}, {opt['kw']}; light {Hl}x{Wl}, {opt['light_kw']}), step {k} {more}: {story}"

    def ref_clear():                    # (a strip filler clears, and renders, its own rows only)
        ref.z_buffer[y0:y1] = np.float32(1e6); ref.color_buffer[y0:y1] = 0; ref.normals_buffer[y0:y1] = 0
        ref.winner[y0:y1] = -1

    def planes_equal(k, more=""):
        """All four planes, as the device holds them, against the oracle's."""
        for name, get, want in (("colour", f.get_color_tensor, ref.color_buffer), ("z", f.get_z_tensor, ref.z_buffer),
                                ("normal", f.get_normals_tensor, ref.normals_buffer), ("winner", f.get_winner_tensor, ref.winner)):
            assert_bit_equal(get().cpu().numpy()[y0:y1], want[y0:y1], what(k, more) + f": {name}")

    def check(k, more=""):
        if k % 2 == 0:
            f.debug_check()             # (synchronises: on odd steps the getters are the first to meet the frame)
        planes_equal(k, more)
        if k % 2:
            f.debug_check()

    def wire_edges(mode):
        """The edge mask of a wire mode, in the caller's order: random bytes of the last frame's triangle count, or of
        another soup's."""
        e = mode["edges"]
        if e is None:
            return None
        T = S.count(state["soup"]) if state["soup"] is not None else 0
        if e["wrong"]:
            T = next(S.count(n) for n in S.SOUPS if S.count(n) != T)
        return np.random.default_rng(e["seed"]).integers(0, 256, T).astype(np.uint8)

    def host_pass(mode):
        """The host model of a legal pass, applied to the oracle's colour plane."""
        tri, col, nrm = pool.host[state["soup"]]
        if mode["kind"] == "texture":
            name, t = state["bound"]
            uv, tex, chain = pool.uv[name], pool.textures[t], pool.chains[t]
            lit = dict(normals=ref.normals_buffer, light_direction=LIGHT) if mode["light"] else {}
            if mode["filter"] == "trilinear" and mode["anisotropy"] > 1:
                out = aniso_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, None, mode["perspective"],
                                             mode["anisotropy"], y0=y0, y1=y1, chain=chain, **lit)
            elif mode["filter"] == "trilinear":
                out = mip_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, None, mode["perspective"],
                                           y0=y0, y1=y1, chain=chain, **lit)
            else:
                out = tex_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, mode["perspective"],
                                           mode["filter"] == "bilinear", y0=y0, y1=y1, **lit)
        elif mode["kind"] == "phong":
            out = phong_ref.phong_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, ref.normals_buffer, mode["lights"],
                                       ambient=mode["ambient"], shininess=mode["shininess"],
                                       specular_color=mode["specular_color"], clamp=mode["clamp"], y0=y0, y1=y1)
        elif mode["kind"] == "ao":
            taps = mode["taps"]
            table = ambient_occlusion.taps(mode["radius_px"], taps) if isinstance(taps, int) else list(taps)
            out = ao_ref.ao_pass(ref.color_buffer, ref.z_buffer, ref.winner, tri, ref.proj_mat, ref.normals_buffer, table,
                                 radius=mode["radius"], radius_px=mode["radius_px"], strength=mode["strength"],
                                 floor=mode["floor"], rotate=mode["rotate"], face=mode["normals"] == "face", y0=y0, y1=y1)
        elif mode["kind"] == "wire":
            kw = dict(width=mode["width"], line=mode["color"], feather=mode["feather"], opacity=mode["opacity"], fill=mode["fill"],
                      edges=wire_edges(mode), y0=y0, y1=y1)
            if len(tri) == 0:          # the empty soup: legal, and nothing is written
                out = ref.color_buffer.copy()
            elif mode["outline"]:
                out = outline_ref.wire_pass(ref.color_buffer, ref.winner, ref.z_buffer, tri, ref.proj_mat,
                                            depth_bias=mode["depth_bias"], radius_px=mode["radius_px"], **kw)
            else:
                out = overlay_ref.wire_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, **kw)
        else:
            if mode["own"]:
                ltri, PL, lz, lw = tri, ref.proj_mat, ref.z_buffer, ref.winner
            else:
                ltri, PL, lz, lw = state["ltri"], lig.proj_mat, lig.z_buffer, lig.winner
            out = shadow_ref.shadow_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, ltri, PL, lz,
                                         lw if mode["use_winner"] else None, bias=mode["bias"], ambient=mode["ambient"],
                                         pcf=mode["pcf"], y0=y0, y1=y1)
        assert not np.isnan(out).any()
        ref.color_buffer[:] = out

    def device_pass(mode):
        if mode["kind"] == "texture":
            f.texture_pass(perspective=mode["perspective"], filter=mode["filter"], anisotropy=mode["anisotropy"],
                           light_direction=light3 if mode["light"] else None)
        elif mode["kind"] == "phong":
            f.phong_pass(mode["lights"], ambient=mode["ambient"], shininess=mode["shininess"],
                         specular_color=mode["specular_color"], clamp=mode["clamp"])
        elif mode["kind"] == "ao":
            f.ao_pass(radius=mode["radius"], radius_px=mode["radius_px"], taps=mode["taps"], strength=mode["strength"],
                      floor=mode["floor"], rotate=mode["rotate"], normals=mode["normals"])
        elif mode["kind"] == "wire":
            edges = wire_edges(mode)
            if edges is not None and mode["edges"]["form"] == "tensor":
                edges = torch.from_numpy(edges).cuda()
            f.wire_pass(width=mode["width"], color=mode["color"], feather=mode["feather"], opacity=mode["opacity"],
                        fill=mode["fill"], edges=edges, outline=mode["outline"], depth_bias=mode["depth_bias"],
                        radius_px=mode["radius_px"])
        else:
            f.shadow_pass(bias=mode["bias"], pcf=mode["pcf"], ambient=mode["ambient"], use_winner=mode["use_winner"])

    def light_frame(mode):
        """What a shadow pass needs first: the light's view of the camera's soup from a random pose, and the binding."""
        tri, col, nrm = pool.host[state["soup"]]
        if mode["own"]:
            f.bind_shadow_map(f, tri)                  # the camera's own planes are the map
            bound_count = len(tri)
        else:
            R, t = shadow_ref.rotation_frame(CENTRE, mode["angles"])
            ltri, lnrm = shadow.light_arrays(tri, nrm, R, t)
            state["ltri"] = ltri
            g.render_arrays(ltri, col, lnrm, clear=True)
            lig.clear()
            lig.render_arrays(ltri, col, lnrm)
            f.bind_shadow_map(g, torch.from_numpy(ltri).cuda() if seed % 2 else ltri)
            bound_count = len(ltri)
        if mode["wrong"]:                              # light-frame vertices of another triangle count
            other = next(n for n in S.SOUPS if S.count(n) != bound_count)
            f.bind_shadow_map(f if mode["own"] else g, pool.host[other][0])

    def a_pass(k, mode, more=""):
        if mode["kind"] == "shadow":
            light_frame(mode)
        if mode["legal"]:
            if small["camera"]:
                met["camera"] += overflowed(f)
            if small["light"] and mode["kind"] == "shadow" and not mode["own"]:
                met["light"] += overflowed(g)
            device_pass(mode)
            host_pass(mode)
            assert not f._pending                      # settled before the pass: no later redo can undo it
        else:
            with pytest.raises(ValueError):
                device_pass(mode)
        check(k, more + f" after {'a' if mode['legal'] else 'a refused'} {mode['kind']} pass")
        if mode["kind"] == "shadow" and not mode["own"] and mode["legal"]:
            assert not g._pending
            for name, get, want in (("z", g.get_z_tensor, lig.z_buffer), ("winner", g.get_winner_tensor, lig.winner)):
                assert_bit_equal(get().cpu().numpy(), want, what(k, more) + f": the light's {name}")

    for k, step in enumerate(steps):
        op = step["op"]
        story.append({a: b for a, b in step.items() if a not in ("rows", "value")})
        if op in ("cleared frame", "composite"):
            name = step["soup"]
            if op == "cleared frame":
                ref_clear()
            ref.render_arrays(*pool.host[name], y0=y0, y1=y1)
            if step.get("form") == "model":
                f.render_model(pool.device_model, clear=True)
            else:
                arrays = pool.dev[name] if step.get("form") == "torch" else pool.host[name]
                f.render_arrays(*arrays, clear=op == "cleared frame")
            state["soup"] = name
            if op == "composite":
                check(k, "after the composite")
                a_pass(k, step["then"], "on a composite")
                continue
        elif op == "render_frame":
            for _ in range(step["frames"]):
                f.render_frame()
            ref_clear()
            ref.render_arrays(*pool.host[state["soup"]], y0=y0, y1=y1)
        elif op == "clear":
            f.clear()
            ref_clear()
        elif op == "bind":
            t = step["texture"]
            uv, tex = pool.uv[step["soup"]], pool.textures[t]
            if k % 2:
                uv, tex = torch.from_numpy(uv).cuda(), torch.from_numpy(tex).cuda()
            f.bind_texture(uv, tex, mipmaps=step["mipmaps"])
            state["bound"] = (step["soup"], t)
            if step["mipmaps"]:
                assert f.mip_levels() == [c.shape[:2] for c in pool.chains[t]]
                for lv, c in enumerate(pool.chains[t]):
                    assert_bit_equal(f.get_mip_level(lv).cpu().numpy(), c, what(k, f"mip level {lv}"))
            else:
                assert f.mip_levels() is None          # (a chain bound before is gone with its texture)
        elif op == "unbind":
            f.bind_texture(None, None)
            state["bound"] = None
        elif op in ("texture_pass", "shadow_pass", "phong_pass", "ao_pass", "wire_pass"):
            a_pass(k, step["mode"])
            continue
        elif op in ("two passes", "chain"):
            for n, mode in enumerate(step["modes"]):
                a_pass(k, mode, f"pass {n + 1} of {len(step['modes'])}")
            continue
        elif op == "edit then pass":
            view = f.get_color_buffer()
            assert state["view"] is None or view is state["view"]          # the array handed out earlier
            state["view"] = view
            assert_bit_equal(view[y0:y1], ref.color_buffer[y0:y1], what(k, "before the edit"))
            a = y0 + int(step["rows"][0] * (y1 - y0 - 1))
            b = min(y1, a + 1 + int(step["rows"][1] * 9))
            mode = step["mode"]
            if mode["kind"] == "shadow":
                light_frame(mode)
            zview = pushed = None
            if step.get("z_edit"):     # covered pixels of the rows, 2e-3 nearer the eye: they occlude what surrounds them
                zview = f.get_z_buffer()
                assert_bit_equal(zview[y0:y1], ref.z_buffer[y0:y1], what(k, "z before the edit"))
                pushed = np.where(ref.winner[a:b] >= 0, ref.z_buffer[a:b] - np.float32(2e-3), ref.z_buffer[a:b])
            if mode["legal"]:
                view[a:b] = np.float32(step["value"])
                ref.color_buffer[a:b] = np.float32(step["value"])
                if zview is not None:
                    zview[a:b] = pushed
                    ref.z_buffer[a:b] = pushed
                device_pass(mode)
                host_pass(mode)
                check(k, f"rows {a} .. {b} edited, then a pass")
                assert f.get_color_buffer() is view
                assert_bit_equal(view[y0:y1], ref.color_buffer[y0:y1], what(k, "the view after the pass"))
            else:
                keep = view[a:b].copy()
                view[a:b] = np.float32(step["value"])
                if zview is not None:
                    zkeep = zview[a:b].copy()
                    zview[a:b] = pushed
                with pytest.raises(ValueError):
                    device_pass(mode)
                check(k, "a refused pass after an edit: nothing is carried, nothing changes")
                view[a:b] = keep                       # (the caller takes the edit back)
                if zview is not None:
                    zview[a:b] = zkeep
            continue
        elif op == "resolve":
            s = max(d for d in range(1, step["factor"] + 1) if H % d == 0 and W % d == 0 and y0 % d == 0 and y1 % d == 0)
            got = f.resolve(s, light_direction=light3 if step["light"] else None).cpu().numpy()
            want = ssaa_ref.resolve(ref.color_buffer, s, normals=ref.normals_buffer,
                                    light_direction=LIGHT if step["light"] else None, Y0=y0 // s, Y1=y1 // s)
            assert_bit_equal(got, want, what(k, f"resolve({s})"))
        elif op == "getters":
            if k % 2 == 0:
                f.debug_check()
            for name, get, want in (("z", f.get_z_buffer, ref.z_buffer), ("colour", f.get_color_buffer, ref.color_buffer),
                                    ("normal", f.get_normals_buffer, ref.normals_buffer)):
                view = get()
                if name == "colour":
                    assert state["view"] is None or view is state["view"]
                    state["view"] = view
                assert_bit_equal(view[y0:y1], want[y0:y1], what(k) + f": {name}")
            assert_bit_equal(f.get_winner_tensor().cpu().numpy()[y0:y1], ref.winner[y0:y1], what(k) + ": winner")
            if k % 2:
                f.debug_check()
            continue
        if small["camera"] and op in ("cleared frame", "render_frame", "bind", "unbind"):
            continue                                   # (left pending: whatever looks next meets the frame as it is)
        check(k)
    torch.cuda.synchronize()
    for who in ("camera", "light"):
        assert met[who] > 0 or not small[who], what(len(steps), f"no legal pass met an overflowed frame of the {who}'s")
