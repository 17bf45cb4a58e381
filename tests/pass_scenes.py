"""What the per-pass tests share: the scenes (T-Rex, the random soups, their textured forms), the fillers, the oracle's
frame of a scene with the comparison of the planes a pass only reads, the test doubles of a filler (``recording_filler``,
``fake_filler_base``), and the module-scoped fixtures built from them.
Imported by name by the CPU and the GPU files alike, so torch and the package are imported inside the functions.

A fixture defined here is shared by importing it into the test module (``from pass_scenes import capi  # noqa: F401``):
its scope is then that module, one instance per importing file.  A pass's test file subclasses ``Scene`` (GPU) or
``Frame`` (CPU) with the ``want`` / ``check`` or ``run`` that call its own model and pass, and builds the fixtures of
its class with ``trex_fixture`` and ``soup_fixture``."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from util import assert_bit_equal, random_soup

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with


def host(t):
    return t.cpu().numpy()


def filler(H, W, fov=45.0, **kw):
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    kw.setdefault("track_winner", True)
    return AdvancedPixelBufferFiller(H, W, fov=fov, device="cuda:0", **kw)


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def light3(oracle):
    return (C.c_float * 3)(*[float(v) for v in oracle.guro_light(LIGHT)])


# ---- scenes --------------------------------------------------------------------------------------------------------

def trex_arrays():
    from cython3dmodelrenderer_amd import scenes
    return scenes.load_fixture("trex_inputs.npz")


def trex_textured():
    tri, col, nrm = trex_arrays()
    with np.load(os.path.join(GOLDEN, "trex_uv.npz")) as z:
        uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    return tri, col, nrm, uv


def soup_textured(seed, T, res, **kw):
    rng = np.random.default_rng(seed)
    tri, col, nrm = random_soup(rng, T, res, **kw)
    uv = rng.uniform(-1.5, 2.5, (T, 3, 2)).astype(np.float32)        # beyond [0, 1]: the clamp is part of the rule
    return tri, col, nrm, uv


def texture(seed, th, tw):
    return np.random.default_rng(seed).integers(0, 256, (th, tw, 3), dtype=np.uint8)


def textured_model(seed=8):
    from cython3dmodelrenderer_amd.data_structures.model import Model
    tri, col, nrm, uv = soup_textured(seed, 3000, 256, size_px=(3.0, 50.0))
    T = len(tri)
    idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    tex = texture(seed, 37, 53)
    m = Model(tri.reshape(-1, 3), idx, uv.reshape(-1, 2), idx, tex, nrm.reshape(-1, 3), idx, recalculate_normals=False)
    return m, tex


def edge_mask(kind, tri, seed=9):
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    if kind == "all":
        return None
    if kind == "feature":
        return feature_edges(tri, 30.0)
    return np.random.default_rng(seed).integers(0, 256, len(tri)).astype(np.uint8)       # bits 3 to 7 are ignored


class Soup:
    """What a filler reads off a model."""

    def __init__(self, seed=71, T=3000, res=256):
        self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = \
            random_soup(np.random.default_rng(seed), T, res, size_px=(3.0, 50.0))


class TriangleModel:
    """Three arrays as the model that the triangle iterators walk."""

    def __init__(self, tri, col, nrm):
        self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = tri, col, nrm

    def n_triangles(self):
        return len(self._vertices_by_triangles)

    def get_triangle(self, i):
        return (self._vertices_by_triangles[i],
                None if self._colors_by_triangles is None else self._colors_by_triangles[i],
                self._normals_by_triangles[i])


# ---- the oracle's frame of a scene ---------------------------------------------------------------------------------

def oracle_frame(oracle, tri, col, nrm, H, W, y0=0, y1=None):
    ref = oracle.OracleFiller(H, W, fov=45.0)
    ref.render_arrays(tri, col, nrm, y0=y0, y1=y1)
    return ref


def planes_only_read(f, ref, what):
    """z, normals and the winner plane of the filler `f` are the oracle frame's: a pass only reads them."""
    assert_bit_equal(host(f.get_z_tensor()), ref.z_buffer, f"{what}: z")
    assert_bit_equal(host(f.get_normals_tensor()), ref.normals_buffer, f"{what}: normals")
    assert_bit_equal(host(f.get_winner_tensor()), ref.winner, f"{what}: winner")


class Frame:
    """A model and the oracle's frame of it: computed once, only read afterwards.  `covered` is the mask of its
    pixels that show a triangle."""

    def __init__(self, oracle, arrays, H, W, y0=0, y1=None):
        self.tri, self.col, self.nrm = arrays
        self.H, self.W = H, W
        self.cam = oracle_frame(oracle, self.tri, self.col, self.nrm, H, W, y0, y1)
        self.covered = self.cam.winner >= 0


class Scene(Frame):
    """A Frame for the fillers of the GPU tests: `covered` is the count.  A pass's file adds ``want(...)``, the host
    model's colours, and ``check(...)``, which draws, runs the pass and compares."""

    def __init__(self, oracle, arrays, H, W, y0=0, y1=None):
        super().__init__(oracle, arrays, H, W, y0, y1)
        self.covered = int(self.covered.sum())

    def draw(self, f):
        f.render_arrays(self.tri, self.col, self.nrm, clear=True)

    def check_planes(self, f, what):
        planes_only_read(f, self.cam, what)

    def assert_changed(self, want, what):
        """-> the mask of the pixels whose colour the pass changed, which is not empty."""
        changed = (want.view(np.uint32) != self.cam.color_buffer.view(np.uint32)).any(2)
        assert changed.any(), (what, "the pass changed nothing")
        return changed


# ---- the test doubles: a filler that records, a filler of the two mixins on CPU tensors ----------------------------

class RecordingFiller:
    """A filler that records what the Renderer asks of it, as (name, args, kwargs) in ``calls``.  It has the methods
    that ``recording_filler`` is given and no others: the Renderer's constructor asks ``hasattr``."""
    device = None
    returns = {}
    copies = ()

    def __init__(self, h=8, w=8):
        self.calls = []
        self.h, self.w = h, w

    def names(self):
        return [c[0] for c in self.calls]

    def _answer(self, name, a, kw):
        """What the method `name` returns: ``returns[name]``, called with the filler and the arguments if it is a
        function; else a fresh zero plane for the two host views, "colour" for the colour tensor, and None."""
        if name in self.returns:
            r = self.returns[name]
            return r(self, *a, **kw) if callable(r) else r
        if name in ("get_color_buffer", "get_normals_buffer"):
            return np.zeros((self.h, self.w, 3), np.float32)
        return "colour" if name == "get_color_tensor" else None


def recording_filler(methods, returns=None, quiet=(), copies=(), **attributes):
    """-> a RecordingFiller class with the methods named in `methods` and `quiet` (lists, or one string of names).  A
    call of a method in `methods` is recorded, one in `quiet` is not.  `returns` is {name: what the method returns, or a
    function of the filler and the call's arguments that returns it}.  The methods in `copies` record a clone of each
    tensor among their positional arguments (for a caller that edits it in place afterwards).  `attributes` become
    class attributes, such as the tensor that the tests expect back."""
    def method(name, noted):
        def call(self, *a, **kw):
            if noted:
                seen = tuple(v.clone() if hasattr(v, "clone") else v for v in a) if name in self.copies else a
                self.calls.append((name, seen, kw))
            return self._answer(name, a, kw)
        call.__name__ = name
        return call
    methods, quiet = [m.split() if isinstance(m, str) else list(m) for m in (methods, quiet)]
    body = dict(attributes, returns=dict(returns or {}), copies=tuple(copies))
    body.update({n: method(n, True) for n in methods})
    body.update({n: method(n, False) for n in quiet})
    return type("RecordingFiller", (RecordingFiller,), body)


def fake_filler_base():
    """-> the base of a file's ``FakeFiller``: the protocol of the two mixins (DevicePlanes, DeferredPasses) on CPU
    tensors, with the planes of a ``Frame``.  ``events`` lists what happened: "push" for the host edits carried up,
    "settle" for the wait for the frame, and whatever the file's own ``_launch_pass``, the host model, appends."""
    import torch
    from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses
    from cython3dmodelrenderer_amd.pixel_buffer_filler._device_planes import DevicePlanes

    class FakeFillerBase(DevicePlanes, DeferredPasses):
        device = "cpu"
        _pipeline = None
        _order = None
        inputs = ("tri",)                  # the arrays of the frame that the last draw left resident

        def __init__(self, frame, row_strip=None, track_winner=True):
            super().__init__()
            self.frame = frame
            self.h, self.w = frame.cam.winner.shape
            self.y0, self.y1 = (0, self.h) if row_strip is None else row_strip
            self._P = frame.cam.proj_mat
            self.z_buffer = torch.from_numpy(frame.cam.z_buffer.copy())
            self.color_buffer = torch.from_numpy(frame.cam.color_buffer.copy())
            self.normals_buffer = torch.from_numpy(frame.cam.normals_buffer.copy())
            self.winner_buffer = torch.from_numpy(frame.cam.winner.copy()) if track_winner else None
            self._inputs = tuple(torch.from_numpy(np.ascontiguousarray(getattr(frame, n))) for n in self.inputs)
            self._last_flags = 1               # FUSED_CLEAR
            self.events = []

        def _ready_planes(self):
            pass

        def _wait_planes(self):
            return False

        def _check_bins(self):
            self.events.append("settle")

        def _push_host_edits(self):
            self.events.append("push")
            super()._push_host_edits()

        def _pinned_like(self, buf):
            return torch.empty(tuple(buf.shape), dtype=buf.dtype)
    return FakeFillerBase


# ---- fixtures: import them into the test module, or build them there from its own class ----------------------------

def trex_fixture(cls):
    """A module's fixture of T-Rex at 256 x 256 as `cls`, a Frame or a Scene."""
    @pytest.fixture(scope="module")
    def trex(oracle):
        s = cls(oracle, trex_arrays(), 256, 256)
        assert int(np.sum(s.covered)) == 15801
        return s
    return trex


def soup_fixture(cls):
    """A module's fixture of the default Soup at 256 x 256 as the Scene `cls`, the Soup itself as its ``model``."""
    @pytest.fixture(scope="module")
    def soup(oracle):
        m = Soup()
        s = cls(oracle, (m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles), 256, 256)
        s.model = m
        assert s.covered > 10000
        return s
    return soup


def soups_fixture(cls, soups):
    """A module's fixture of {seed: cls of the random soup} for `soups`, {seed: (T, H, W, size_px)}."""
    @pytest.fixture(scope="module")
    def frames(oracle):
        return {seed: cls(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), size_px=size), H, W)
                for seed, (T, H, W, size) in soups.items()}
    return frames


@pytest.fixture(scope="module")
def capi():
    from cython3dmodelrenderer_amd import _build, _capi
    _build.build()           # hipcc cross-compiles for gfx950 without a GPU
    return _capi


@pytest.fixture(scope="module")
def lib():
    import torch                     # (before the library: the two then share one HIP runtime, torch's)
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cython3dmodelrenderer_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def trex_uv():
    return trex_textured()


@pytest.fixture(scope="module")
def wire_golden():
    with open(os.path.join(GOLDEN, "wire_golden.json")) as fh:
        return json.load(fh)
