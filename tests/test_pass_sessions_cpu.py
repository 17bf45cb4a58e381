"""Dry run of the session generator of tests/pass_sessions.py over the default seeds, without a GPU: the sessions that
tests/test_pass_sessions_gpu.py drives reach every op kind and every kernel instance of the passes, and most of their
pass calls are legal ones.  These are conditions on the generator; its weights are tuned until they hold."""
import collections

import pass_sessions as S


def _dry():
    ops, inst, legal, calls, per_session = collections.Counter(), collections.Counter(), 0, 0, []
    for seed in range(S.SEEDS):
        _, steps = S.plan(seed)
        ops.update(s["op"] for s in steps)
        ps = list(S.passes(steps))
        per_session.append(sum(p["legal"] for p in ps))
        legal += per_session[-1]
        calls += len(ps)
        inst.update(S.instance(p) for p in ps if p["legal"])
    return ops, inst, legal, calls, per_session


def test_the_generator_is_a_pure_function_of_the_seed():
    assert S.SEEDS == 12 and 28 <= S.STEPS <= 36
    for seed in (0, 5, 11):
        assert S.plan(seed) == S.plan(seed)
    assert S.plan(1)[1] != S.plan(2)[1]


def test_every_op_kind_and_every_kernel_instance_occurs_three_times():
    ops, inst, _, _, _ = _dry()
    print(dict(ops))
    assert set(ops) == set(S.OPS)
    assert min(ops.values()) >= 3, ops
    assert len(S.INSTANCES) == 4 * 2 + 2 * 2 + 2 * 2 + 3 * 2
    assert all(inst[i] >= 3 for i in S.INSTANCES), {i: inst[i] for i in S.INSTANCES if inst[i] < 3}


def test_most_pass_calls_are_legal_and_every_session_has_four():
    _, _, legal, calls, per_session = _dry()
    print(f"{legal} legal pass calls of {calls}; per session {per_session}")
    assert legal >= 0.6 * calls and legal < calls
    assert min(per_session) >= 4


def test_options_cover_what_the_sessions_are_about():
    opts = [S.options(seed) for seed in range(S.SEEDS)]
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


def test_a_legal_pass_is_the_first_to_meet_an_overflowed_frame():
    """The mechanism of test_a_frame_redrawn_after_a_bin_overflow_ends_textured, for the camera's frame and the light's:
    on every seed with small bin lists, of the default round and of five rounds of CRENDER_FUZZ_SOAK."""
    for soak in range(6):
        cameras = lights = 0
        for seed in range(soak * S.SEEDS, (soak + 1) * S.SEEDS):
            opt, steps = S.plan(seed)
            assert len(steps) == S.STEPS
            if opt["kw"].get("bin_capacity"):
                cameras += 1
                assert S.first_to_settle(steps) == "pass", (seed, S.first_to_settle(steps))
            if opt["light_kw"].get("bin_capacity"):
                lights += 1
                assert S.light_meets_a_pass(steps), seed
        assert cameras == 2 and lights == 3
