"""The op generator of tests/test_pass_sessions_gpu.py: seeded sessions of one AdvancedPixelBufferFiller through its
deferred passes.  A pure function of the seed — `plan(seed)` returns the filler's options and a list of steps, each a
dict that says everything the runner does and whether a pass in it is legal — so that tests/test_pass_edges_cpu.py can
dry-run the default seeds without a GPU and hold the generator to its coverage floors.

Three families of sessions.  The default one, "passes", draws texture and shadow passes; "lit" draws the Phong and
the occlusion pass among them as well, from generators, ops, weights and instances of its own, and chains up to four
passes on one frame; "wired" adds the wire pass, overlay and outline, to those of "lit", again from a seed base, ops,
weights and instances of its own, and chains up to five.  The two older families are the same functions of the seed
they were before the third one existed: tests/test_pass_sessions_cpu.py pins a digest of every plan of theirs.

The generator keeps the little state that decides legality, as the filler documents it: a pass needs a last frame that
started from cleared buffers (``clear()`` afterwards empties the planes but leaves the pass legal: it finds background
only); a texture pass needs uv of the last frame's triangle count bound, and a mip chain for "trilinear"; a Phong or
an occlusion pass needs the frame alone, and its own arguments well formed; so does a wire pass, whose edge mask
must have the last frame's triangle count."""
import numpy as np

SEEDS = 12
STEPS = 32
SOUPS = ("mixed", "large", "model", "none")           # "model" is also handed over as a DeviceModel
FORMS = ("numpy", "torch", "model")
TEXTURES = ((37, 53), (8, 5), (1, 1), (64, 128), (3, 200))          # th x tw: a smaller one may follow a larger one
OPS = ("cleared frame", "render_frame", "composite", "clear", "bind", "unbind", "texture_pass", "shadow_pass",
       "two passes", "edit then pass", "resolve", "getters")
# (weights tuned on the dry run of the default seeds: tests/test_pass_sessions_cpu.py states the floors)
WEIGHTS = (4, 2, 1, 1, 3, 1, 13, 7, 5, 2, 2, 2)
# The sessions (seed modulo SEEDS) whose camera filler gets bin lists far too small; those of the light's filler are
# seed % 4 == 2.  plan() opens such a session with the steps that make a legal pass the first to meet an overflowed
# frame, on every seed of a soak as well.
CAMERA_OVERFLOWS = (4, 9)

FAMILIES = ("passes", "lit", "wired")
# The "lit" family: a pass of each kind as an op of its own, "chain" (two to four passes on one frame) for "two passes".
LIT_OPS = ("cleared frame", "render_frame", "composite", "clear", "bind", "unbind", "texture_pass", "shadow_pass",
           "phong_pass", "ao_pass", "chain", "edit then pass", "resolve", "getters")
# (tuned on the dry run of the default seeds, as WEIGHTS is)
LIT_WEIGHTS = (4, 3, 1, 3, 2, 2, 11, 4, 1, 4, 8, 2, 2, 3)
# In the "lit" family the session 4 (modulo SEEDS) opens with a Phong pass on its overflowed frame, the session 9 — a
# presorted filler, and there a row strip as well — with an occlusion pass in the face mode.
LIT_KINDS = (0.5, 0.03, 0.3, 0.17)                     # texture, shadow, phong, ao: what a pass of any kind is
LIT_SEED = 28000
LIT_OPENING = {4: "phong_pass", 9: "ao_pass"}
# The lights a Phong mode draws from: points inside the soups' depth range (0.5 .. 3), behind the camera and beyond the
# soups, directions, and a light that adds nothing.
LIGHT_POOL = (dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5),
              dict(position=(-0.4, 0.3, 0.9), diffuse=0.5, specular=0.25),
              dict(position=(-0.8, -0.5, -0.2), diffuse=0.9, specular=0.5),
              dict(position=(1.5, -2.0, 6.0), diffuse=0.6, specular=0.125),
              dict(direction=(0.3, -0.2, 1.0), diffuse=0.3, specular=0.25),
              dict(direction=(-1.0, 0.5, 0.25), diffuse=0.2, specular=0.125),
              dict(position=(0.5, 0.5, 1.0), diffuse=0.0, specular=0.0))
AO_RADIUS = {1: 0.03, 4: 0.05, 8: 0.1, 32: 0.4}       # the world radius grows with the halo, so that far taps are taken
AO_TAP_COUNTS = {1: (1, 8), 4: (4, 16, 64), 8: (1, 16, 64), 32: (16, 64)}


# The "wired" family: the ops of "lit" and the wire pass as an op of its own.
WIRED_OPS = LIT_OPS + ("wire_pass",)
# (tuned on the dry run of the default seeds, as WEIGHTS is)
WIRED_WEIGHTS = (16, 6, 1, 7, 3, 4, 18, 5, 1, 2, 58, 6, 4, 6, 9)
WIRED_KINDS = (0.41, 0.02, 0.23, 0.21, 0.13)          # texture, shadow, phong, ao, wire
WIRED_SEED = 38000
# The session 4 (modulo SEEDS) opens with an overlay on its overflowed frame, the session 9 — presorted, with a row
# strip — with an outline.
WIRED_OPENING = {4: False, 9: True}
WIRE_WIDTHS = (0.25, 1.0, 3.0, 10.0)
WIRE_FILLS = (None, (30.0, 35.0, 40.0), (0.0, 0.0, 0.0))
WIRE_LINES = ((255.0, 255.0, 255.0), (250.0, 240.0, 20.0), (0.0, 0.0, 0.0))
WIRE_RADII = (None, 0, 1, 3, 8)
WIRE_MALFORMED = ("width 0", "radius_px 9", "width + feather over 14", "edges of another length", "opacity 1.5")


def options(seed, family="passes"):
    """The filler's construction options and the frame's size."""
    rng = np.random.default_rng({"passes": 17000, "lit": 27000, "wired": 37000}[family] + seed)
    H = int(rng.choice([96, 128, 97, 111])) if seed % 3 else int(rng.choice([97, 111, 127]))
    W = int(rng.choice([160, 128, 131, 159])) if seed % 3 else int(rng.choice([131, 159, 105]))
    kw = {"tile": int(rng.choice([16, 32]))}
    if seed % 4 == 1:
        kw["presort"] = True
    if seed % 5 == 2:
        a = 4 * int(rng.integers(0, H // 8))
        kw["row_strip"] = (a, min(H, a + 4 * int(rng.integers(4, H // 4))))
    if family != "passes" and seed % SEEDS == 9:                          # a row strip, presorted and overflowing at once
        a = 4 * int(rng.integers(1, H // 8))
        kw["row_strip"] = (a, min(H, a + 4 * int(rng.integers(6, H // 4))))
    if seed % SEEDS in CAMERA_OVERFLOWS:
        kw.update(tile=32, bin_capacity=40, direct_bins=False)        # frames overflow; a pass settles and redraws them
    light = {"tile": int(rng.choice([0, 16, 32]))}
    if seed % 3 == 0:
        light["presort"] = True
    if seed % 4 == 2:
        light.update(tile=32, bin_capacity=40, direct_bins=False)     # the light's own pending overflow
    return dict(H=H, W=W, kw=kw, light_kw=light, Hl=int(rng.choice([64, 77])), Wl=int(rng.choice([64, 90])))


def _texture_mode(rng, mip, flat=False):
    """A random mode of texture_pass; `legal` is False for "trilinear" without a chain.  `flat` (the "lit" family, which
    has fewer texture passes to spend): every kernel instance as likely as any other."""
    filt = str(rng.choice(["nearest", "bilinear", "trilinear", "aniso"] if flat else
                          ["nearest", "bilinear", "trilinear", "trilinear", "aniso", "aniso"]))
    if filt in ("trilinear", "aniso") and not mip and rng.uniform() < 0.85:
        filt = str(rng.choice(["nearest", "bilinear"]))
    mode = dict(kind="texture", filter="trilinear" if filt == "aniso" else filt, perspective=bool(rng.integers(0, 2)),
                light=bool(rng.integers(0, 2)), anisotropy=int(rng.integers(2, 17)) if filt == "aniso" else 1)
    return mode, (mip or mode["filter"] != "trilinear")


def _shadow_mode(rng):
    return dict(kind="shadow", pcf=int(rng.choice([1, 3, 5])), use_winner=bool(rng.integers(0, 2)),
                bias=float(rng.choice([0.0, 1e-3])), ambient=float(rng.choice([0.0, 0.25, 0.6])),
                angles=[float(v) for v in rng.uniform(-25, 25, 3)], own=bool(rng.uniform() < 0.2),
                wrong=bool(rng.uniform() < 0.12))


def _phong_mode(rng):
    """A random mode of phong_pass; about one in eight is malformed: five lights, a shininess that is no power of two,
    or a light with both a position and a direction."""
    n = int(rng.choice([1, 1, 2, 3, 4]))
    lights = [dict(LIGHT_POOL[int(i)]) for i in rng.choice(len(LIGHT_POOL), n, replace=False)]
    mode = dict(kind="phong", lights=lights, shininess=int(rng.choice([1, 8, 256, 4096])),
                ambient=float(rng.choice([0.0, 0.1, 0.4])), clamp=float(rng.choice([255.0, np.inf, 100.0])),
                specular_color=tuple(float(v) for v in rng.choice([255.0, 200.0, 17.5, 3.0], 3)), malformed=None)
    if rng.uniform() < 0.125:
        mode["malformed"] = str(rng.choice(["five lights", "shininess 3", "position and direction"]))
        if mode["malformed"] == "five lights":
            mode["lights"] = [dict(LIGHT_POOL[i]) for i in range(5)]
        elif mode["malformed"] == "shininess 3":
            mode["shininess"] = 3
        else:
            mode["lights"][-1] = dict(mode["lights"][-1], position=(0.0, 0.0, 1.0), direction=(0.0, 0.0, 1.0))
    return mode


def _ao_mode(rng):
    """A random mode of ao_pass; about one in eight is malformed: radius_px = 33, a (0, 0) tap, or normals="vertex"."""
    R = int(rng.choice([1, 4, 8, 32], p=[0.3, 0.15, 0.2, 0.35]))
    if rng.uniform() < 0.3:                                             # an explicit table: a corner of the halo and others
        n = int(rng.integers(2, 13))
        pairs = {(R, -R)} | {(int(a), int(b)) for a, b in rng.integers(-R, R + 1, (n, 2))}
        taps = sorted(pairs - {(0, 0)})
    else:
        taps = int(rng.choice(AO_TAP_COUNTS[R]))
    mode = dict(kind="ao", radius_px=R, taps=taps, radius=AO_RADIUS[R], normals=str(rng.choice(["plane", "face"])),
                rotate=bool(rng.integers(0, 2)), strength=float(rng.choice([1.0, 3.0, 50.0])),
                floor=float(rng.choice([0.0, 0.25, 1.0])), malformed=None)
    if rng.uniform() < 0.125:
        mode["malformed"] = str(rng.choice(["radius_px 33", "a (0, 0) tap", "vertex normals"]))
        if mode["malformed"] == "radius_px 33":
            mode["radius_px"] = 33
        elif mode["malformed"] == "a (0, 0) tap":
            mode["taps"] = [(1, 0), (0, 0)]
        else:
            mode["normals"] = "vertex"
    return mode


def _wire_mode(rng, outline=None):
    """A random mode of wire_pass; about one in eight is malformed (WIRE_MALFORMED).  `edges`: None, or how the mask —
    random bytes drawn from `seed`, of the last frame's triangle count unless `wrong` — is handed over."""
    outline = bool(rng.integers(0, 2)) if outline is None else outline
    width = float(rng.choice(WIRE_WIDTHS))
    feather = float(rng.choice([0.25, 1.0, 3.0, 14.0 - width]))
    edges = [None, "numpy", "tensor"][int(rng.integers(0, 3))]
    mode = dict(kind="wire", outline=outline, fill=WIRE_FILLS[int(rng.integers(0, len(WIRE_FILLS)))],
                color=WIRE_LINES[int(rng.integers(0, len(WIRE_LINES)))], width=width, feather=feather,
                opacity=float(rng.choice([0.0, 0.5, 1.0])),
                edges=None if edges is None else dict(form=edges, seed=int(rng.integers(0, 2 ** 31)), wrong=False),
                depth_bias=float(rng.choice([0.0, 1e-3, -2e-3])), radius_px=WIRE_RADII[int(rng.integers(0, len(WIRE_RADII)))],
                malformed=None)
    if rng.uniform() < 0.125:
        mode["malformed"] = bad = str(rng.choice(WIRE_MALFORMED))
        if bad == "width 0":
            mode["width"] = 0.0
        elif bad == "radius_px 9":
            mode.update(outline=True, radius_px=9)
        elif bad == "width + feather over 14":
            mode.update(outline=True, radius_px=None, width=10.0, feather=4.5)
        elif bad == "edges of another length":
            mode["edges"] = dict(form=str(rng.choice(["numpy", "tensor"])), seed=int(rng.integers(0, 2 ** 31)), wrong=True)
        else:
            mode["opacity"] = 1.5
    return mode


def instance(mode):
    """The kernel instance a legal pass runs."""
    if mode["kind"] == "wire":
        return ("wire", mode["outline"], mode["fill"] is not None)
    if mode["kind"] == "phong":
        return ("phong", len(mode["lights"]) == 1, mode["shininess"] > 1)
    if mode["kind"] == "ao":
        R = mode["radius_px"]
        return ("ao", mode["normals"] == "face", mode["rotate"], 1 if R == 1 else 8 if R <= 8 else 32)
    if mode["kind"] == "shadow":
        return ("shadow", mode["pcf"], mode["use_winner"])
    if mode["filter"] == "trilinear":
        return ("aniso" if mode["anisotropy"] > 1 else "mip", mode["perspective"], mode["light"])
    return ("tex", mode["perspective"], mode["filter"] == "bilinear", mode["light"])


INSTANCES = [("tex", p, b, l) for p in (False, True) for b in (False, True) for l in (False, True)] + \
            [(k, p, l) for k in ("mip", "aniso") for p in (False, True) for l in (False, True)] + \
            [("shadow", K, w) for K in (1, 3, 5) for w in (False, True)]
LIT_INSTANCES = INSTANCES + [("phong", one, squared) for one in (False, True) for squared in (False, True)] + \
                [("ao", face, rotate, R) for face in (False, True) for rotate in (False, True) for R in (1, 8, 32)]
WIRED_INSTANCES = LIT_INSTANCES + [("wire", outline, fill) for outline in (False, True) for fill in (False, True)]


def plan(seed, steps=STEPS, family="passes"):
    """(options, [step]) of a session.  Each step: op, its parameters, and for every pass in it `legal`."""
    assert family in FAMILIES
    wired = family == "wired"
    lit = family == "lit" or wired                             # what "wired" shares with "lit"
    opt = options(seed, family)
    rng = np.random.default_rng({"passes": 18000, "lit": LIT_SEED, "wired": WIRED_SEED}[family] + seed)
    ops, weights = {"passes": (OPS, WEIGHTS), "lit": (LIT_OPS, LIT_WEIGHTS), "wired": (WIRED_OPS, WIRED_WEIGHTS)}[family]
    soup = None            # the soup of the last render
    cleared = False        # that render started from cleared buffers
    bound = None           # (soup whose uv are bound, mipmaps)
    out = []

    def a_pass(kind=None):
        if wired:
            kind = kind or str(rng.choice(["texture", "shadow", "phong", "ao", "wire"], p=WIRED_KINDS))
        elif lit:
            kind = kind or str(rng.choice(["texture", "shadow", "phong", "ao"], p=LIT_KINDS))
        else:
            kind = "texture" if rng.uniform() < 0.62 else "shadow"
        if kind == "texture":
            mode, ok = _texture_mode(rng, bound is not None and bound[1], flat=lit)
            legal = ok and soup is not None and cleared and bound is not None and count(bound[0]) == count(soup)
        elif kind == "shadow":
            mode = _shadow_mode(rng)
            legal = soup is not None and cleared and not mode["wrong"]
        else:                          # the frame alone: the empty soup is legal and writes nothing
            mode = _phong_mode(rng) if kind == "phong" else _ao_mode(rng) if kind == "ao" else _wire_mode(rng)
            legal = soup is not None and cleared and mode["malformed"] is None
        return dict(mode, legal=bool(legal))

    def bind_now(right):
        """A binding step: the uv of the last frame's soup (`right`) or of another triangle count."""
        nonlocal bound
        names = [s for s in SOUPS if (count(s) == count(soup)) == right] if soup is not None else list(SOUPS)
        name = str(rng.choice(names or SOUPS))
        step = dict(op="bind", soup=name, texture=int(rng.integers(0, len(TEXTURES))), mipmaps=bool(rng.uniform() < 0.75))
        bound = (name, step["mipmaps"])
        return step

    # A filler with small bin lists: a frame of a soup that is not empty, then — nothing looking at the frame in
    # between — the binding and a legal texture pass (the camera's lists), a legal shadow pass against the second
    # filler (the light's).  The rest of the session is drawn as everywhere.
    opening = []
    if opt["kw"].get("bin_capacity"):
        opening += ["wire_pass"] if wired else [LIT_OPENING[seed % SEEDS]] if lit else ["bind", "texture_pass"]
    if opt["light_kw"].get("bin_capacity"):
        opening += ["shadow_pass"]
    opening = ["cleared frame"] + opening if opening else []

    for k in range(steps):
        op = str(rng.choice(ops, p=np.array(weights) / sum(weights)))
        if k == 0:
            op = "cleared frame"
        if k < len(opening):
            op = opening[k]
            step = dict(op=op)
            if op == "cleared frame":
                soup, cleared = str(rng.choice(SOUPS[:3])), True
                step.update(soup=soup, form=str(rng.choice(FORMS)) if soup == "model" else str(rng.choice(FORMS[:2])))
            elif op == "bind":
                step.update(soup=soup, texture=int(rng.integers(0, len(TEXTURES))), mipmaps=True)
                bound = (soup, True)
            elif op == "texture_pass":
                step["mode"] = dict(_texture_mode(rng, True)[0], legal=True)
            elif op in ("phong_pass", "ao_pass"):
                mode = None
                while mode is None or mode["malformed"]:               # (a well-formed one)
                    mode = _phong_mode(rng) if op == "phong_pass" else dict(_ao_mode(rng), normals="face")
                step["mode"] = dict(mode, legal=True)
            elif op == "wire_pass":
                mode = None
                while mode is None or mode["malformed"]:
                    mode = _wire_mode(rng, WIRED_OPENING[seed % SEEDS])
                step["mode"] = dict(mode, legal=True)
            else:
                step["mode"] = dict(_shadow_mode(rng), own=False, wrong=False, legal=True)
            out.append(step)
            continue
        if op in ("texture_pass", "two passes", "edit then pass", "chain") and soup is not None and cleared and \
                (bound is None or count(bound[0]) != count(soup)) and rng.uniform() < 0.8:
            op = "bind"                                                 # (most sessions bind before they texture)
        step = dict(op=op)
        if op == "cleared frame":
            soup, cleared = str(rng.choice(SOUPS)), True
            step.update(soup=soup, form=str(rng.choice(FORMS)) if soup == "model" else str(rng.choice(FORMS[:2])))
        elif op == "render_frame":
            if soup is None:
                step["op"] = "getters"
            else:
                cleared = True
                step["frames"] = int(rng.integers(1, 4))
        elif op == "composite":
            soup, cleared = str(rng.choice(SOUPS)), False
            step.update(soup=soup, then=a_pass())                       # the pass afterwards must raise
        elif op == "bind":
            step = bind_now(right=bool(rng.uniform() < 0.85))
        elif op == "unbind":
            bound = None
        elif op in ("texture_pass", "shadow_pass"):
            p = a_pass()
            if (p["kind"] == "texture") != (op == "texture_pass"):
                p = a_pass() if rng.uniform() < 0.5 else p
            step.update(op="texture_pass" if p["kind"] == "texture" else "shadow_pass", mode=p)
        elif op in ("phong_pass", "ao_pass", "wire_pass"):
            step["mode"] = a_pass(op[:-5])
        elif op == "two passes":
            step["modes"] = [a_pass(), a_pass()]
        elif op == "chain":
            if rng.uniform() < 0.6:                                     # a texture first, a shadow last, lights between
                kinds = ["texture"] + [str(k) for k in rng.choice(["phong", "ao"], int(rng.integers(1, 3)))] + ["shadow"]
                if wired:                                               # (and the lines over the lit surface, under the shadow)
                    kinds[-1:] = ["wire", "shadow"] if rng.uniform() < 0.6 else ["wire"]
            else:
                kinds = [None] * int(rng.integers(2, 5))
            step["modes"] = [a_pass(kind) for kind in kinds]
        elif op == "edit then pass":
            step.update(rows=[float(v) for v in rng.uniform(0, 1, 2)], value=float(rng.uniform(1, 200)),
                        mode=a_pass("wire" if wired and rng.uniform() < 0.5 else None))
            if lit:                    # under an occlusion pass: covered pixels of the rows pushed towards the eye as well
                mode = step["mode"]
                step["z_edit"] = bool(rng.integers(0, 2)) and (mode["kind"] == "ao" or bool(mode.get("outline")))
        elif op == "resolve":
            step.update(factor=int(rng.integers(1, 5)), light=bool(rng.integers(0, 2)))
        out.append(step)
    return opt, out


def count(soup):
    return {"mixed": 300, "large": 60, "model": 120, "none": 0}[soup]


def passes(steps):
    """Every pass call of a session, in order."""
    for s in steps:
        if s["op"] == "composite":
            yield s["then"]
        elif s["op"] in ("texture_pass", "shadow_pass", "phong_pass", "ao_pass", "wire_pass", "edit then pass"):
            yield s["mode"]
        elif s["op"] in ("two passes", "chain"):
            yield from s["modes"]


def first_to_settle(steps):
    """What first settles a frame whose bin lists overflowed, on a filler whose lists are too small for every soup
    but the empty one: "pass" if a legal pass meets the frame still pending (the runner leaves such a filler's frames
    unchecked until something else looks), else the op that looked first, or None.  A frame that starts from cleared
    buffers, and clear(), drop what is pending without growing the lists: the next frame overflows again."""
    live = False
    for s in steps:
        op = s["op"]
        modes = [s["mode"]] if op in ("texture_pass", "shadow_pass", "phong_pass", "ao_pass", "wire_pass") else s.get("modes", [])
        if op == "cleared frame":
            live = count(s["soup"]) > 0
        elif op == "clear":
            live = False
        elif op == "composite" and (live or count(s["soup"]) > 0):
            return op
        elif op in ("edit then pass", "getters", "resolve") and live:
            return op
        for mode in modes:
            if live:
                return "pass" if mode["legal"] else "refused pass"      # (the runner compares the planes after either)
    return None


def light_meets_a_pass(steps):
    """A legal shadow pass against the second filler, over a soup that is not empty: the pass that settles the
    light's own overflowed frame, which its render just before the pass left pending."""
    soup = None
    for s in steps:
        if s["op"] in ("cleared frame", "composite"):
            soup = s["soup"]
        for mode in passes([s]):
            if mode["kind"] == "shadow" and mode["legal"] and not mode["own"] and count(soup) > 0:
                return True
    return False


def lit_between(steps, between=("phong", "ao")):
    """The chains of a session that hold a legal Phong or occlusion pass (or one of the kinds `between`) after a legal
    texture pass and before a legal shadow pass of the same chain, or before a resolve as the next step."""
    n = 0
    for k, s in enumerate(steps):
        if s["op"] != "chain":
            continue
        kinds = [m["kind"] if m["legal"] else None for m in s["modes"]]
        resolve_next = k + 1 < len(steps) and steps[k + 1]["op"] == "resolve"
        for i, kind in enumerate(kinds):
            if kind in between and "texture" in kinds[:i] and ("shadow" in kinds[i + 1:] or resolve_next):
                n += 1
                break
    return n
