"""Dry run of the session generator of tests/pass_sessions.py over the default seeds, without a GPU: the sessions that
tests/test_pass_sessions_gpu.py drives reach every op kind and every kernel instance of the passes, and most of their
pass calls are legal ones.  These are conditions on the generator; its weights are tuned until they hold."""
import collections
import hashlib

import pytest

import pass_sessions as S

# sha256(repr(plan(seed))) of the default family's twelve plans, as they were before the "lit" family existed
DEFAULT_PLANS = (
    "65f6ee4017ca84fd3ea16820b2c8e1b788003f2388fd19eca64398b2c264b32f",
    "d13a8122a9baaeedddf593532bdc1ae689e770689d3fcc0bdefe36e09a66bded",
    "f0d4d136bf6b481f6d0b4584e1bf9cf9b7f33f181db8074cd0a109854d7a96b5",
    "40144febb0069809168f4b3e6e25bf9e78511693a153b9a689d4a67ee5e22ca9",
    "04c8d2a7cb14ce3baa89ba6a3b60611d88d214ad6952e082e68b9ea14401d702",
    "24968c6c198ee47697c05bf4c2cc26d66d75ed2f5be593c1f690535834890e15",
    "f655e342a74bbec1b7ac878556eec9b7626e8ca1213c3883cdeb2090d77f63f5",
    "a572d0251001f188bc0f5d5510a2d8d2e7e8edfc50861b1d9755a2198e19282c",
    "bf5a73d40ac2d81b0610647b2b7865cda57d39af35d49894ee586bb692fb8905",
    "20c82854b35eeb78bcb1f7cb9d76c906677f07ec0fdd9869ae14364a90c19ec1",
    "8436d4e132669625e3a66ca634b8afbb5eccd3bfb67bd1fec082875a4f154477",
    "e87e6d1e01f062d7d9ce3cb5e11cd17dbca84b08957a645f9af1eea97d1d5a47",
)

# the same of the "lit" family's, as they were before the "wired" family existed
LIT_PLANS = (
    "2049251269fca9681a1246f2fa2f2f96d6d2c8884a5baf5331fb5d7e2eee6867",
    "e02704275999a3addab6782aa89d7de5351648b6dabeb6abeef577939adc3f75",
    "273dbbadc534b6b13af5c2d9604ba766938ffe5d602b704b88c22f19381ff23b",
    "99ab7e2c01dce808084b27a15bf7f5da5fe7b28f00848cf0b4784f825860861b",
    "173b9685c858d9aa381ec51b215637a289f6469026624525f7f7d4ccdd2a1597",
    "57ff2c386329be32702cd37bfada194b15045e5e292aae6c6d52986fff84b2ca",
    "a559f10db4ec294da69ef7924d9560765780671788742222163e6dad6fb50d3a",
    "deafa7169f071426bbf8a16af12901632c7057f3b791123c63508984c2a540ee",
    "92cd86a75c98bb5f6cca49f96096e6ce363ca4e55dc1fdcc47f4eec76e723235",
    "34cdd1bbcb52b2ed7a8d737eb64178fd6e110bba4d1304ab11eaa59c077a9119",
    "8fc25358937f3ccd34d8fe4e3cb096dd1436f20c3a3427d5c589fb8e3d1ac388",
    "e2b83a5cf407ec3499b2d9937c791754181111b7539b4fdc7e3a73339d5717f7",
)
OPS = {"passes": S.OPS, "lit": S.LIT_OPS, "wired": S.WIRED_OPS}
INSTANCES = {"passes": S.INSTANCES, "lit": S.LIT_INSTANCES, "wired": S.WIRED_INSTANCES}


def _dry(family="passes"):
    ops, inst, legal, calls, per_session = collections.Counter(), collections.Counter(), 0, 0, []
    for seed in range(S.SEEDS):
        _, steps = S.plan(seed, family=family)
        ops.update(s["op"] for s in steps)
        ps = list(S.passes(steps))
        per_session.append(sum(p["legal"] for p in ps))
        legal += per_session[-1]
        calls += len(ps)
        inst.update(S.instance(p) for p in ps if p["legal"])
    return ops, inst, legal, calls, per_session


def test_the_generator_is_a_pure_function_of_the_seed():
    assert S.SEEDS == 12 and 28 <= S.STEPS <= 36
    for family in S.FAMILIES:
        for seed in (0, 5, 11):
            assert S.plan(seed, family=family) == S.plan(seed, family=family)
        assert S.plan(1, family=family)[1] != S.plan(2, family=family)[1]
    assert S.plan(3) == S.plan(3, family="passes") and S.plan(3)[1] != S.plan(3, family="lit")[1]
    assert S.plan(3, family="wired")[1] != S.plan(3, family="lit")[1]


def test_the_default_family_draws_the_plans_it_always_drew():
    assert len(DEFAULT_PLANS) == S.SEEDS
    for seed, digest in enumerate(DEFAULT_PLANS):
        assert hashlib.sha256(repr(S.plan(seed)).encode()).hexdigest() == digest, seed


def test_the_lit_family_draws_the_plans_it_always_drew():
    assert len(LIT_PLANS) == S.SEEDS
    for seed, digest in enumerate(LIT_PLANS):
        assert hashlib.sha256(repr(S.plan(seed, family="lit")).encode()).hexdigest() == digest, seed


def test_every_op_kind_and_every_kernel_instance_occurs_three_times(family="passes"):
    ops, inst, _, _, _ = _dry(family)
    print(dict(ops))
    print({i: inst[i] for i in S.WIRED_INSTANCES})
    assert set(ops) == set(OPS[family])
    assert min(ops.values()) >= 3, ops
    assert len(S.INSTANCES) == 4 * 2 + 2 * 2 + 2 * 2 + 3 * 2 and len(S.LIT_INSTANCES) == 22 + 4 + 12
    assert len(S.WIRED_INSTANCES) == len(S.LIT_INSTANCES) + 4 and len(S.WIRED_OPS) == len(S.LIT_OPS) + 1
    instances = INSTANCES[family]
    assert set(inst) <= set(instances)
    assert all(inst[i] >= 3 for i in instances), {i: inst[i] for i in instances if inst[i] < 3}


def test_most_pass_calls_are_legal_and_every_session_has_four(family="passes"):
    _, _, legal, calls, per_session = _dry(family)
    print(f"{legal} legal pass calls of {calls}; per session {per_session}")
    assert legal >= 0.6 * calls and legal < calls
    assert min(per_session) >= 4


def test_the_lit_family_lights_and_occludes_between_a_texture_and_a_shadow_or_a_resolve():
    chains = [S.lit_between(S.plan(seed, family="lit")[1]) for seed in range(S.SEEDS)]
    print(chains)
    assert sum(chains) >= 6
    modes = [m for seed in range(S.SEEDS) for m in S.passes(S.plan(seed, family="lit")[1])]
    lights = [l for m in modes if m["kind"] == "phong" and m["legal"] for l in m["lights"]]
    z = [l["position"][2] for l in lights if "position" in l]
    assert any(0.5 < v < 3 for v in z) and any(v < 0.5 for v in z) and any(v > 3 for v in z)
    assert any("direction" in l for l in lights) and any(l["diffuse"] == l["specular"] == 0 for l in lights)
    for key, values in (("shininess", {1, 8, 256, 4096}), ("ambient", {0.0, 0.1, 0.4}), ("clamp", {255.0, float("inf"), 100.0})):
        assert {m[key] for m in modes if m["kind"] == "phong" and m["legal"]} == values, key
    assert {len(m["lights"]) for m in modes if m["kind"] == "phong" and m["legal"]} == {1, 2, 3, 4}
    ao = [m for m in modes if m["kind"] == "ao" and m["legal"]]
    for key, values in (("radius_px", {1, 4, 8, 32}), ("strength", {1.0, 3.0, 50.0}), ("floor", {0.0, 0.25, 1.0})):
        assert {m[key] for m in ao} == values, key
    assert any(isinstance(m["taps"], int) for m in ao) and any(isinstance(m["taps"], list) for m in ao)
    for kind, ways in (("phong", {"five lights", "shininess 3", "position and direction"}),
                       ("ao", {"radius_px 33", "a (0, 0) tap", "vertex normals"})):
        assert {m["malformed"] for m in modes if m["kind"] == kind and m["malformed"]} == ways
        share = sum(bool(m["malformed"]) for m in modes if m["kind"] == kind) / sum(m["kind"] == kind for m in modes)
        assert 0.05 < share < 0.25, (kind, share)
    # an edit of the z view under an occlusion pass, taken and not taken
    edits = [s for seed in range(S.SEEDS) for s in S.plan(seed, family="lit")[1] if s["op"] == "edit then pass"]
    under_ao = [s["z_edit"] for s in edits if s["mode"]["kind"] == "ao" and s["mode"]["legal"]]
    assert True in under_ao and False in under_ao


def test_options_cover_what_the_sessions_are_about(family="passes"):
    opts = [S.options(seed, family) for seed in range(S.SEEDS)]
    assert all(o["H"] <= 128 and o["W"] <= 160 for o in opts)
    assert sum(o["H"] % 2 and o["W"] % 2 for o in opts) >= 3                        # odd frames
    assert {o["kw"]["tile"] for o in opts} == {16, 32}
    assert sum("presort" in o["kw"] for o in opts) >= 2 and sum("row_strip" in o["kw"] for o in opts) >= 2
    assert sum(o["kw"].get("bin_capacity", 0) > 0 and o["kw"]["direct_bins"] is False for o in opts) == 2
    assert any(o["light_kw"].get("bin_capacity") for o in opts) and any(o["light_kw"].get("presort") for o in opts)
    for o in opts:
        if "row_strip" in o["kw"]:
            a, b = o["kw"]["row_strip"]
            assert 0 <= a < b <= o["H"]
    if family != "passes":             # a row strip, presorted and overflowing at once
        assert sum(bool(o["kw"].get("bin_capacity")) and "row_strip" in o["kw"] and "presort" in o["kw"] for o in opts) == 1


def test_a_legal_pass_is_the_first_to_meet_an_overflowed_frame(family="passes"):
    """The mechanism of test_a_frame_redrawn_after_a_bin_overflow_ends_textured, for the camera's frame and the light's:
    on every seed with small bin lists, of the default round and of five rounds of CRENDER_FUZZ_SOAK.  In the "lit"
    family the pass that meets the camera's frame is a Phong pass in one session and a face-mode occlusion pass in the
    other."""
    for soak in range(6):
        cameras = lights = 0
        first = set()
        for seed in range(soak * S.SEEDS, (soak + 1) * S.SEEDS):
            opt, steps = S.plan(seed, family=family)
            assert len(steps) == S.STEPS
            if opt["kw"].get("bin_capacity"):
                cameras += 1
                assert S.first_to_settle(steps) == "pass", (seed, S.first_to_settle(steps))
                mode = next(S.passes(steps))
                first.add((mode["kind"], mode.get("normals")))
            if opt["light_kw"].get("bin_capacity"):
                lights += 1
                assert S.light_meets_a_pass(steps), seed
        assert cameras == 2 and lights == 3
        if family == "lit":
            assert first == {("phong", None), ("ao", "face")}
        if family == "wired":          # an overlay in the session 4, an outline in the presorted strip of the session 9
            assert first == {("wire", None)}
            firsts = {seed % S.SEEDS: next(S.passes(S.plan(seed, family=family)[1])) for seed in range(soak * S.SEEDS, (soak + 1) * S.SEEDS)
                      if seed % S.SEEDS in S.CAMERA_OVERFLOWS}
            assert [firsts[k]["outline"] for k in (4, 9)] == [False, True] and all(m["legal"] for m in firsts.values())
            opt = S.options(soak * S.SEEDS + 9, family)
            assert "row_strip" in opt["kw"] and opt["kw"].get("presort")


def test_the_lit_family_meets_the_same_conditions():
    """Every condition above on the sessions of the "lit" family: its 14 op kinds, the 22 instances of the default
    family with 4 of the Phong and 12 of the occlusion kernel, the share of legal calls, the options, and the first pass
    on an overflowed frame."""
    test_every_op_kind_and_every_kernel_instance_occurs_three_times("lit")
    test_most_pass_calls_are_legal_and_every_session_has_four("lit")
    test_options_cover_what_the_sessions_are_about("lit")
    test_a_legal_pass_is_the_first_to_meet_an_overflowed_frame("lit")


def test_the_wired_family_meets_the_same_conditions():
    """Every condition above on the sessions of the "wired" family: its 15 op kinds, the 38 instances of the "lit"
    family with the 4 of the two wire kernels (overlay or outline, with and without a fill), the share of legal calls,
    the options, and a wire pass as the first on an overflowed frame."""
    test_every_op_kind_and_every_kernel_instance_occurs_three_times("wired")
    test_most_pass_calls_are_legal_and_every_session_has_four("wired")
    test_options_cover_what_the_sessions_are_about("wired")
    test_a_legal_pass_is_the_first_to_meet_an_overflowed_frame("wired")


def test_the_wired_family_draws_lines_between_a_texture_and_a_shadow_or_a_resolve():
    plans = [S.plan(seed, family="wired")[1] for seed in range(S.SEEDS)]
    chains = [S.lit_between(steps, between=("wire",)) for steps in plans]
    print(chains)
    assert sum(chains) >= 6
    # the order texture, Phong or occlusion, wire, then a shadow or a resolve, every pass of it legal
    full = 0
    for steps in plans:
        for k, s in enumerate(steps):
            kinds = [m["kind"] if m["legal"] else None for m in s.get("modes", [])] if s["op"] == "chain" else []
            if "wire" in kinds and "texture" in kinds[:kinds.index("wire")]:
                i, j = kinds.index("texture"), kinds.index("wire")
                after = "shadow" in kinds[j + 1:] or (k + 1 < len(steps) and steps[k + 1]["op"] == "resolve")
                full += bool({"phong", "ao"} & set(kinds[i:j])) and after
    assert full >= 3, full
    modes = [m for steps in plans for m in S.passes(steps)]
    wire = [m for m in modes if m["kind"] == "wire"]
    legal = [m for m in wire if m["legal"]]
    assert {m["malformed"] for m in wire if m["malformed"]} == set(S.WIRE_MALFORMED)
    share = sum(bool(m["malformed"]) for m in wire) / len(wire)
    assert 0.05 < share < 0.25, share
    assert all(m["malformed"] is None for m in legal)
    outlines = [m for m in legal if m["outline"]]
    assert {m["radius_px"] for m in outlines} == set(S.WIRE_RADII) and None in S.WIRE_RADII
    assert {m["depth_bias"] for m in outlines} == {0.0, 1e-3, -2e-3}
    for key, values in (("width", {0.25, 1.0, 3.0, 10.0}), ("opacity", {0.0, 0.5, 1.0})):
        assert {m[key] for m in legal} == values, key
    assert {0.25, 1.0, 3.0} <= {m["feather"] for m in legal} and any(m["width"] + m["feather"] == 14 for m in outlines)
    assert any(m["radius_px"] is None and m["width"] + m["feather"] == 14 for m in outlines)      # the default radius at its top
    for outline in (False, True):
        assert {None if m["edges"] is None else m["edges"]["form"] for m in legal if m["outline"] == outline} == {None, "numpy", "tensor"}
    # a wire pass after an edit of the colour view, and an outline after one of the z view, taken and not taken
    edits = [s for steps in plans for s in steps if s["op"] == "edit then pass" and s["mode"]["kind"] == "wire" and s["mode"]["legal"]]
    assert len(edits) >= 3
    under = [s["z_edit"] for s in edits if s["mode"]["outline"]]
    assert True in under and False in under and not any(s["z_edit"] for s in edits if not s["mode"]["outline"])
    # on a cleared last frame (clear() leaves the pass legal: it finds background only), on the empty soup, after a composite
    after_clear = on_none = refused = 0
    for steps in plans:
        soup = cleared_by_clear = None
        for s in steps:
            if s["op"] in ("cleared frame", "composite"):
                soup, cleared_by_clear = s["soup"], False
            elif s["op"] == "render_frame":
                cleared_by_clear = False
            elif s["op"] == "clear":
                cleared_by_clear = True
            for m in S.passes([s]):
                if m["kind"] == "wire" and m["legal"]:
                    after_clear += bool(cleared_by_clear)
                    on_none += soup == "none"
            if s["op"] == "composite" and s["then"]["kind"] == "wire":
                refused += not s["then"]["legal"]
    print(f"{after_clear} wire passes after clear(), {on_none} on the empty soup, {refused} refused on a composite")
    assert after_clear >= 1 and on_none >= 1 and refused >= 1
