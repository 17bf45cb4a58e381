"""The op generator of tests/test_pass_sessions_gpu.py: seeded sessions of one AdvancedPixelBufferFiller through its
deferred passes.  A pure function of the seed — `plan(seed)` returns the filler's options and a list of steps, each a
dict that says everything the runner does and whether a pass in it is legal — so that tests/test_pass_edges_cpu.py can
dry-run the default seeds without a GPU and hold the generator to its coverage floors.

The generator keeps the little state that decides legality, as the filler documents it: a pass needs a last frame that
started from cleared buffers (``clear()`` afterwards empties the planes but leaves the pass legal: it finds background
only); a texture pass needs uv of the last frame's triangle count bound, and a mip chain for "trilinear"."""
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


def options(seed):
    """The filler's construction options and the frame's size."""
    rng = np.random.default_rng(17000 + seed)
    H = int(rng.choice([96, 128, 97, 111])) if seed % 3 else int(rng.choice([97, 111, 127]))
    W = int(rng.choice([160, 128, 131, 159])) if seed % 3 else int(rng.choice([131, 159, 105]))
    kw = {"tile": int(rng.choice([16, 32]))}
    if seed % 4 == 1:
        kw["presort"] = True
    if seed % 5 == 2:
        a = 4 * int(rng.integers(0, H // 8))
        kw["row_strip"] = (a, min(H, a + 4 * int(rng.integers(4, H // 4))))
    if seed % SEEDS in CAMERA_OVERFLOWS:
        kw.update(tile=32, bin_capacity=40, direct_bins=False)        # frames overflow; a pass settles and redraws them
    light = {"tile": int(rng.choice([0, 16, 32]))}
    if seed % 3 == 0:
        light["presort"] = True
    if seed % 4 == 2:
        light.update(tile=32, bin_capacity=40, direct_bins=False)     # the light's own pending overflow
    return dict(H=H, W=W, kw=kw, light_kw=light, Hl=int(rng.choice([64, 77])), Wl=int(rng.choice([64, 90])))


def _texture_mode(rng, mip):
    """A random mode of texture_pass; `legal` is False for "trilinear" without a chain."""
    filt = str(rng.choice(["nearest", "bilinear", "trilinear", "trilinear", "aniso", "aniso"]))
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


def instance(mode):
    """The kernel instance a legal pass runs."""
    if mode["kind"] == "shadow":
        return ("shadow", mode["pcf"], mode["use_winner"])
    if mode["filter"] == "trilinear":
        return ("aniso" if mode["anisotropy"] > 1 else "mip", mode["perspective"], mode["light"])
    return ("tex", mode["perspective"], mode["filter"] == "bilinear", mode["light"])


INSTANCES = [("tex", p, b, l) for p in (False, True) for b in (False, True) for l in (False, True)] + \
            [(k, p, l) for k in ("mip", "aniso") for p in (False, True) for l in (False, True)] + \
            [("shadow", K, w) for K in (1, 3, 5) for w in (False, True)]


def plan(seed, steps=STEPS):
    """(options, [step]) of a session.  Each step: op, its parameters, and for every pass in it `legal`."""
    opt = options(seed)
    rng = np.random.default_rng(18000 + seed)
    soup = None            # the soup of the last render
    cleared = False        # that render started from cleared buffers
    bound = None           # (soup whose uv are bound, mipmaps)
    out = []

    def a_pass():
        if rng.uniform() < 0.62:
            mode, ok = _texture_mode(rng, bound is not None and bound[1])
            legal = ok and soup is not None and cleared and bound is not None and count(bound[0]) == count(soup)
        else:
            mode = _shadow_mode(rng)
            legal = soup is not None and cleared and not mode["wrong"]
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
        opening += ["bind", "texture_pass"]
    if opt["light_kw"].get("bin_capacity"):
        opening += ["shadow_pass"]
    opening = ["cleared frame"] + opening if opening else []

    for k in range(steps):
        op = str(rng.choice(OPS, p=np.array(WEIGHTS) / sum(WEIGHTS)))
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
            else:
                step["mode"] = dict(_shadow_mode(rng), own=False, wrong=False, legal=True)
            out.append(step)
            continue
        if op in ("texture_pass", "two passes", "edit then pass") and soup is not None and cleared and \
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
        elif op == "two passes":
            step["modes"] = [a_pass(), a_pass()]
        elif op == "edit then pass":
            step.update(rows=[float(v) for v in rng.uniform(0, 1, 2)], value=float(rng.uniform(1, 200)), mode=a_pass())
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
        elif s["op"] in ("texture_pass", "shadow_pass", "edit then pass"):
            yield s["mode"]
        elif s["op"] == "two passes":
            yield from s["modes"]


def first_to_settle(steps):
    """What first settles a frame whose bin lists overflowed, on a filler whose lists are too small for every soup
    but the empty one: "pass" if a legal pass meets the frame still pending (the runner leaves such a filler's frames
    unchecked until something else looks), else the op that looked first, or None.  A frame that starts from cleared
    buffers, and clear(), drop what is pending without growing the lists: the next frame overflows again."""
    live = False
    for s in steps:
        op = s["op"]
        modes = [s["mode"]] if op in ("texture_pass", "shadow_pass") else s.get("modes", [])
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
