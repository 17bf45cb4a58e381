"""The ORDER of the argument checks of the seven deferred-pass entries that share their frame checks
(csrc/winner_pass.h: ``frame_checks``, ``rows_check``), without a GPU: for every entry, single bad arguments drawn from its own
``*_argument_errors_without_a_gpu`` test, one or two per check, and every pair of two of them in one call.  Which of
the two is reported says which check comes first.  tests/golden/pass_arg_order.json holds the return code and the whole
text of ``crender_last_error()`` of every single and every pair, recorded by scripts/make_pass_arg_order_golden.py
from the build before the checks were shared; the library must give the same.  Every call fails before any launch."""
import ctypes as C
import itertools
import json
import os

from pass_scenes import GOLDEN, capi  # noqa: F401 (fixture)

FIXTURE = os.path.join(GOLDEN, "pass_arg_order.json")
NAN, INF = float("nan"), float("inf")
FAKE = C.c_void_p(0x1000)              # never dereferenced: every call fails its checks first


def _f3(*v):
    return (C.c_float * 3)(*v)


def _frame_singles(rows=True):
    """The bad arguments of the checks every entry makes: (label, keywords)."""
    s = [("tri=NULL", dict(tri=None)), ("T=-1", dict(T=-1)), ("H=0", dict(H=0)), ("W=-2", dict(W=-2))]
    if rows:
        s += [("y0=-1", dict(y0=-1)), ("y1=9", dict(y1=9)), ("y0=y1=3", dict(y0=3, y1=3))]
    return s


def _nulls(*names):
    return [(f"{n}=NULL", {n: None}) for n in names]


def _style_singles():
    return [("width=nan", dict(width=NAN)), ("width=64.5", dict(width=64.5)), ("feather=0", dict(feather=0.0)),
            ("feather=inf", dict(feather=INF)), ("opacity=nan", dict(opacity=NAN)), ("opacity=1.001", dict(opacity=1.001)),
            ("line[0]=nan", dict(line=_f3(NAN, 255.0, 255.0))), ("fill[2]=inf", dict(fill=_f3(255.0, 255.0, INF)))]


def entries(capi):
    """{entry: (call(**keywords) -> return code, [(label, keywords of one bad argument)])}."""
    L = capi.load()
    zeros = (C.c_float * 16)(*([0.0] * 16))
    white = _f3(255.0, 255.0, 255.0)

    def lights(*rows):
        return (C.c_float * (5 * len(rows)))(*[v for r in rows for v in r])
    row = (0.0, 0.0, -1.0, 0.9, 0.5)

    def phong(win=FAKE, tri=FAKE, T=4, pos_of=None, P=zeros, nrm=FAKE, lights=lights(row), n=1, mask=0, ambient=0.1, k=5,
              spec=white, clamp=255.0, col=FAKE, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_phong_shade(win, tri, T, pos_of, P, nrm, lights, n, mask, ambient, k, spec, clamp, col, H, W, y0, y1,
                                     flags, None)

    def shadow(win=FAKE, tri=FAKE, T=4, pos_of=None, P=zeros, ltri=FAKE, PL=zeros, lz=FAKE, lwin=None, Hl=8, Wl=8, bias=1e-3,
               ambient=0.25, pcf=1, col=FAKE, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_shadow_shade(win, tri, T, pos_of, P, ltri, PL, lz, lwin, Hl, Wl, bias, ambient, pcf, col, H, W, y0, y1,
                                      flags, None)

    def projection(**changed):
        P = (C.c_float * 16)()
        assert L.crender_projection_matrix(45.0, 0.1, 1000.0, 8, 8, P) == capi.OK
        for i, v in changed.items():
            P[int(i[1:])] = v
        return P

    def table(*pairs):
        return (C.c_int8 * (2 * len(pairs)))(*[v for p in pairs for v in p])

    def ao(win=FAKE, z=FAKE, tri=FAKE, T=4, pos_of=None, P=projection(), nrm=FAKE, taps=table((1, 0)), n=1, R=8, radius=0.03,
           min_cos=0.1, strength=2.0, floor=0.0, col=FAKE, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_ao_shade(win, z, tri, T, pos_of, P, nrm, taps, n, R, radius, min_cos, strength, floor, col, H, W, y0,
                                  y1, flags, None)

    def overlay(win=FAKE, tri=FAKE, T=4, pos_of=None, P=zeros, edges=None, line=white, fill=None, width=1.0, feather=1.0,
                opacity=1.0, col=FAKE, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_wire_overlay(win, tri, T, pos_of, P, edges, line, fill, width, feather, opacity, col, H, W, y0, y1,
                                      flags, None)

    def outline(win=FAKE, z=FAKE, tri=FAKE, T=4, pos_of=None, P=zeros, edges=None, line=white, fill=None, width=1.0,
                feather=1.0, opacity=1.0, bias=1e-3, radius=2, col=FAKE, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_wire_outline(win, z, tri, T, pos_of, P, edges, line, fill, width, feather, opacity, bias, radius, col,
                                      H, W, y0, y1, flags, None)

    def edge_aa(win=FAKE, z=FAKE, tri=FAKE, T=4, pos_of=None, P=zeros, edges=None, out=C.c_void_p(0x2000), col=FAKE, H=8, W=8,
                y0=0, y1=8, flags=0):
        return L.crender_wire_edge_aa(win, z, tri, T, pos_of, P, edges, out, col, H, W, y0, y1, flags, None)

    def contours(tri=FAKE, T=4, pos_of=None, P=zeros, partners=FAKE, static=None, facing=FAKE, edges=FAKE, H=8, W=8, flags=0):
        return L.crender_wire_contours(tri, T, pos_of, P, partners, static, facing, edges, H, W, flags, None)

    flags12 = [("flags=1", dict(flags=1)), ("flags=0x80000000", dict(flags=0x80000000))]
    return {
        "crender_phong_shade": (phong, _nulls("win", "P", "nrm", "lights", "spec", "col") + _frame_singles() + [
            ("n=0", dict(n=0)), ("n=5", dict(n=5, lights=lights(*[row] * 5))), ("mask=2", dict(mask=2)), ("k=-1", dict(k=-1)),
            ("k=13", dict(k=13)), ("ambient=nan", dict(ambient=NAN)), ("light[0]=inf", dict(lights=lights((INF,) + row[1:]))),
            ("spec[1]=nan", dict(spec=_f3(255.0, NAN, 255.0))), ("ambient=-0.001", dict(ambient=-0.001)),
            ("kd=-0.5", dict(lights=lights(row[:3] + (-0.5, 0.5)))), ("clamp=nan", dict(clamp=NAN))] + flags12),
        "crender_shadow_shade": (shadow, _nulls("win", "P", "PL", "lz", "col") + [("ltri=NULL", dict(ltri=None))] +
                                 _frame_singles() + [
            ("Hl=0", dict(Hl=0)), ("Wl=-1", dict(Wl=-1)), ("pcf=2", dict(pcf=2)), ("pcf=-1", dict(pcf=-1)),
            ("ambient=1.001", dict(ambient=1.001)), ("ambient=nan", dict(ambient=NAN)), ("bias=nan", dict(bias=NAN)),
            ("bias=-inf", dict(bias=-INF))] + flags12),
        "crender_ao_shade": (ao, _nulls("win", "z", "P", "taps", "col", "nrm") + [
            ("tri=NULL,flags=2", dict(tri=None, flags=2)), ("T=-1", dict(T=-1)), ("H=0", dict(H=0)), ("W=-2", dict(W=-2)),
            ("y0=-1", dict(y0=-1)), ("y1=9", dict(y1=9)), ("y0=y1=3", dict(y0=3, y1=3)), ("n=0", dict(n=0)), ("n=65", dict(n=65)),
            ("R=0", dict(R=0)), ("R=33", dict(R=33)), ("tap=(9,0)", dict(taps=table((1, 1), (9, 0)), n=2)),
            ("tap=(0,0)", dict(taps=table((1, 0), (0, 0)), n=2)), ("radius=nan", dict(radius=NAN)), ("radius=0", dict(radius=0.0)),
            ("min_cos=nan", dict(min_cos=NAN)), ("floor=inf", dict(floor=INF)), ("strength=-0.5", dict(strength=-0.5)),
            ("floor=1.01", dict(floor=1.01)), ("P[1]=0.5", dict(P=projection(p1=0.5))), ("P[0]=0", dict(P=projection(p0=0.0))),
            ("P[14]=nan", dict(P=projection(p14=NAN))), ("flags=4", dict(flags=4)), ("flags=0x80000000", dict(flags=0x80000000))]),
        "crender_wire_overlay": (overlay, _nulls("win", "P", "line", "col") + _frame_singles() + _style_singles() + flags12),
        "crender_wire_outline": (outline, _nulls("win", "z", "P", "line", "col") + _frame_singles() + _style_singles() + [
            ("bias=nan", dict(bias=NAN)), ("bias=inf", dict(bias=INF)), ("radius=-1", dict(radius=-1)),
            ("radius=9", dict(radius=9))] + flags12),
        "crender_wire_edge_aa": (edge_aa, _nulls("win", "z", "P", "out", "col") + _frame_singles() + flags12 + [
            ("out=col", dict(out=FAKE))]),
        "crender_wire_contours": (contours, _nulls("P", "partners", "facing", "edges") + _frame_singles(rows=False) + [
            ("flags=2", dict(flags=2)), ("flags=0x80000000", dict(flags=0x80000000))]),
    }


def outcomes(capi):
    """{entry: {"a" or "a + b": [return code, text of crender_last_error()]}}: every single bad argument, and every pair
    of two that do not set the same keyword."""
    L = capi.load()
    found = {}
    for entry, (call, singles) in entries(capi).items():
        labels = [label for label, _ in singles]
        assert len(set(labels)) == len(labels), entry
        got = {}
        for label, kw in singles:
            got[label] = [call(**kw), L.crender_last_error().decode()]
        for (la, ka), (lb, kb) in itertools.combinations(singles, 2):
            if set(ka) & set(kb):
                continue
            got[f"{la} + {lb}"] = [call(**ka, **kb), L.crender_last_error().decode()]
        found[entry] = got
    return found


def test_every_pair_of_bad_arguments_reports_what_it_did_before_the_checks_were_shared(capi):
    with open(FIXTURE) as fh:
        want = {entry: {case: doc["outcomes"][k] for case, k in doc["cases"].items()} for entry, doc in json.load(fh).items()}
    got = outcomes(capi)
    assert set(got) == set(want) and len(got) == 7
    for entry in want:
        assert set(got[entry]) == set(want[entry]), entry
        pairs = [k for k in want[entry] if " + " in k]
        assert len(pairs) >= 40, (entry, len(pairs))
        for case, (rc, text) in want[entry].items():
            assert rc == capi.EINVAL and text.startswith(entry + ": "), (entry, case)
            assert got[entry][case] == [rc, text], (entry, case)
        # a pair reports one of its two singles' failures: the checks are the same, only their order is in question
        for case in pairs:
            a, b = case.split(" + ")
            assert want[entry][case] in (want[entry][a], want[entry][b]), (entry, case)
