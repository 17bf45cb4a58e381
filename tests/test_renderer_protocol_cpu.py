"""What the Renderer asks of its fillers, recorded: for every ``on_device``, three kinds of illumination and every option
alone and every pair of two, either the refusal or the calls of two ``render`` calls and what they returned, compared
with tests/golden/renderer_protocol.json (scripts/make_renderer_protocol_golden.py wrote it, from the Renderer of the
commit before its frame sequence and its option checks were folded).  Needs no GPU and no library: the fillers are
``pass_scenes.recording_filler``'s."""
import itertools
import json
import os

import numpy as np
import pytest

from pass_scenes import GOLDEN, LIGHT, recording_filler

FIXTURE = os.path.join(GOLDEN, "renderer_protocol.json")
ON_DEVICE = (None, False, True, "fused")
# {option: {variant: its value}}; "shadow" gets its filler per case
OPTIONS = {
    "texture_pass": {"empty": {}, "full": dict(perspective=True, filter="trilinear", anisotropy=4)},
    "shadow": {"": dict(R=np.eye(3, dtype=np.float32), t=np.float32([0.0, 0.0, -2.0]), bias=2e-3, pcf=1)},
    "ambient_occlusion": {"": dict(radius_px=4)},
    "antialias": {"empty": {}, "full": dict(feature_angle=30, contours=True)},
    "depth_of_field": {"": dict(focus=1.25, aperture=6.0)},
    "motion_blur": {"": dict(exposure=0.5, taps=8)},
    "normal_map": {"": dict(height=np.zeros((4, 4), np.float32), scale=2.0, strength=0.5, filter="trilinear")},
    "environment": {"": dict(faces=np.zeros((6, 2, 2, 3), np.uint8), level=1.5, background=True, reflectivity=0.5)},
    "bloom": {"": dict(threshold=200.0, radius=4)},
    "transparency": {"": dict(alpha=0.5, layers=3)},
    "wireframe": {"empty": {}, "full": dict(feature_angle=30, contours=True, hidden=True, vector=True, width=2.0)},
    "supersample": {"": 2},
}
# the method of the filler that is each option's pass
PASSES = {"texture_pass": "texture_pass", "shadow": "shadow_pass", "ambient_occlusion": "ao_pass", "antialias": "edge_aa",
          "depth_of_field": "depth_of_field", "motion_blur": "motion_blur", "normal_map": "normal_map_pass",
          "environment": "environment_pass", "bloom": "bloom", "transparency": "transparency_pass", "wireframe": "wire_pass",
          "supersample": "resolve"}
H, W = 8, 8


def _plane(f, *a, **kw):
    import torch
    return torch.zeros((f.h, f.w, 3))


Camera = recording_filler(
    "render_model set_fused_illumination shade_guro phong_pass _push_host_edits synchronize get_color_tensor get_color_buffer "
    "get_normals_buffer bind_texture bind_shadow_map bind_normal_map get_normal_map bind_normal_map_uv bind_environment "
    "contour_edges hidden_line_pass line_runs " + " ".join(PASSES.values()),
    returns=dict({n: _plane for n in ("get_color_tensor", "edge_aa", "depth_of_field", "motion_blur", "bloom", "transparency_pass")},
                 resolve=lambda f, s, **kw: _plane(f)[:f.h // s, :f.w // s], get_normal_map="bound", line_runs="drawing",
                 contour_edges=lambda f, partners, **kw: np.full(len(partners), 5, np.uint8)))
Light = recording_filler("render_arrays")


def illuminations():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination

    class HostOnly(GuroIllumination):
        """Overrides ``draw_illumination`` alone: the inherited device form is not its shading."""

        def draw_illumination(self, color_buffer, n_buffer):
            color_buffer *= 0.5
    return {"guro": lambda: GuroIllumination(LIGHT), "host_only": lambda: HostOnly(LIGHT),
            "phong": lambda: PhongIllumination(position=(0.0, 0.0, 1.0))}


def model():
    """Four triangles with uv and a texture: a tetrahedron."""
    from cython3dmodelrenderer_amd.data_structures.model import Model
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) * 3 + [2, 2, -6]
    faces = np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    uv = np.float32([[0, 0], [1, 0], [0, 1], [1, 1]])
    tex = np.arange(4 * 4 * 3, dtype=np.uint8).reshape(4, 4, 3)
    return Model(v, faces, uv, faces, tex, None, None)


def option_sets():
    """{name: {option: variant}}: none, every option alone in each of its variants, every pair of two options."""
    single = [(o, v) for o, variants in OPTIONS.items() for v in variants]
    sets = [()] + [(s,) for s in single] + [p for p in itertools.combinations(single, 2) if p[0][0] != p[1][0]]
    return {"+".join(o + (":" + v if v else "") for o, v in s) or "none": dict(s) for s in sets}


def cases():
    """{name: (on_device, the illumination's name, {option: variant})}."""
    return {f"{on_device!r}/{light}/{name}": (on_device, light, chosen)
            for on_device in ON_DEVICE for light in illuminations() for name, chosen in option_sets().items()}


def reduced(v):
    """`v` as JSON: arrays and tensors as their shape and dtype, other objects as their type's name."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (list, tuple)):
        return [reduced(x) for x in v]
    if isinstance(v, dict):
        return {str(k): reduced(x) for k, x in v.items()}
    if isinstance(v, np.generic):
        return reduced(v.item())
    if hasattr(v, "shape") and hasattr(v, "dtype"):
        return {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")}
    return type(v).__name__


def outcome(on_device, light, chosen, m):
    """{"raises": [the type's name, the text]}, or {"renders": [per ``render`` call: the camera's and the light's calls
    and what came back]}, once where the two calls are equal.  What the constructor asks is part of the first."""
    from cython3dmodelrenderer_amd.renderer import Renderer
    camera, lamp = Camera(H, W), Light(H, W)
    options = {o: OPTIONS[o][v] for o, v in chosen.items()}
    if "shadow" in options:
        options["shadow"] = dict(options["shadow"], filler=lamp)
    renders = []
    try:
        r = Renderer(camera, illuminations()[light](), None, H, W, on_device=on_device, **options)
        for _ in range(2):
            image = r.render(m)
            renders.append({"camera": [reduced(c) for c in camera.calls], "light": [reduced(c) for c in lamp.calls],
                            "returned": dict(reduced(image), type=type(image).__name__)})
            camera.calls.clear()
            lamp.calls.clear()
    except Exception as e:
        return {"raises": [type(e).__name__, str(e)]}
    return {"renders": renders[:1] if renders[0] == renders[1] else renders}


def outcomes():
    m = model()
    return {name: outcome(*case, m) for name, case in cases().items()}


def packed(got):
    """The document of `got`, {case: outcome}: every distinct call once, every distinct outcome once with its call lists
    as places among the calls, and each case's place among the outcomes."""
    text = lambda v: json.dumps(v, sort_keys=True)                # noqa: E731
    calls = sorted({text(c) for o in got.values() for r in o.get("renders", ()) for who in ("camera", "light") for c in r[who]})
    at = {c: i for i, c in enumerate(calls)}

    def short(o):
        if "raises" in o:
            return o
        return {"renders": [dict(r, camera=[at[text(c)] for c in r["camera"]], light=[at[text(c)] for c in r["light"]])
                            for r in o["renders"]]}
    distinct = sorted({text(short(o)) for o in got.values()})
    place = {o: i for i, o in enumerate(distinct)}
    return {"calls": [json.loads(c) for c in calls], "outcomes": [json.loads(o) for o in distinct],
            "cases": {k: place[text(short(o))] for k, o in got.items()}}


def unpacked(doc):
    """{case: outcome} of the document `doc`."""
    def whole(o):
        if "raises" in o:
            return o
        return {"renders": [dict(r, camera=[doc["calls"][i] for i in r["camera"]], light=[doc["calls"][i] for i in r["light"]])
                            for r in o["renders"]]}
    return {k: whole(doc["outcomes"][i]) for k, i in doc["cases"].items()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return unpacked(json.load(fh))


@pytest.fixture(scope="module")
def computed():
    return json.loads(json.dumps(outcomes()))


def test_the_cases_are_the_files_and_cover_what_they_should(recorded):
    assert set(cases()) == set(recorded) and len(recorded) == 4 * 3 * 118
    renders = [o for o in recorded.values() if "renders" in o]
    raises = [o["raises"] for o in recorded.values() if "raises" in o]
    assert len(renders) + len(raises) == len(recorded)
    assert len(renders) >= 900 and len(raises) >= 400
    assert all(kind == "ValueError" and text.startswith("Renderer") for kind, text in raises)
    seen = {c[0] for o in renders for r in o["renders"] for c in r["camera"]}
    assert set(PASSES.values()) <= seen
    assert "render_arrays" in {c[0] for o in renders for r in o["renders"] for c in r["light"]}


def test_every_case_does_what_was_recorded(recorded, computed):
    assert set(computed) == set(recorded)
    differing = [k for k in recorded if computed[k] != recorded[k]]
    for k in differing[:5]:
        print(k, "\n  recorded:", recorded[k], "\n  computed:", computed[k])
    assert not differing, (len(differing), differing[:20])
