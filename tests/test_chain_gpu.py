"""The swap chain with its last slot on the caller's stream (include/crender_chain.h, _FramePipeline's `share`):
the same frames, bit for bit, as a filler that renders one frame at a time; ordered with the caller's own work;
following the caller from stream to stream; and gone cleanly with frames in flight.

Frames are 96 x 80 (no multiple of the 32-pixel tiles, 3 x 3 of them) with at most 300 triangles, so a case is
a few hundred launches of microseconds each.  The reference of every comparison is the plain filler
(``pipeline=False``) on the same inputs, rendered once per scene."""
import gc

import numpy as np
import pytest

from util import random_soup

pytestmark = pytest.mark.gpu

H, W = 80, 96
PLANES = ("z", "colour", "normal", "winner")


def _filler(**kw):
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    kw.setdefault("fov", 45.0)
    kw.setdefault("track_winner", True)
    h, w = kw.pop("h", H), kw.pop("w", W)
    return AdvancedPixelBufferFiller(h, w, **kw)


def _sharing(**kw):
    return _filler(pipeline=True, pipeline_depth=4, share_caller_stream=True, **kw)


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _planes(f):
    """Copies of a filler's four planes (through the getters: they join the chain)."""
    return tuple(t.clone() for t in (f.get_z_tensor(), f.get_color_tensor(), f.get_normals_tensor(), f.get_winner_tensor()))


def _same(got, want, what):
    import torch
    for g, w, name in zip(got, want, PLANES):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), f"{what}: {name} differs"


def _soup(seed, T=300, size=(2, 30)):
    return random_soup(np.random.default_rng(seed), T, W, size_px=size)


def _device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.fixture(scope="module")
def plain():
    """The plain filler, and the frame it renders from given inputs."""
    f = _filler()

    def frame(*inputs):
        if len(inputs) == 1:
            f.render_model(inputs[0], clear=True)
        else:
            f.render_arrays(*inputs, clear=True)
        return _planes(f)
    return frame


def _device_model(seed=3, V=150, T=300):
    from cython3dmodelrenderer_amd.data_structures import Model, DeviceModel
    from cython3dmodelrenderer_amd.scenes import fit_model
    rng = np.random.default_rng(seed)
    vertices = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (T, 3)).astype(np.int32)
    dm = DeviceModel(Model(vertices, faces))
    dm.set_uniform_color((40.0, 180.0, 250.0))
    fit_model(dm)
    return dm


def _check_sets(filler, wants, what):
    """Every framebuffer set of the chain against the frame it should hold (after a join)."""
    filler.join()
    pipe = filler._pipe
    assert len(pipe.sets) == len(wants) == 4
    for k, (fb, want) in enumerate(zip(pipe.sets, wants)):
        _same(fb, want, f"{what}, framebuffer set {k}")


@pytest.mark.parametrize("look", [True, False])
def test_shared_slot_frames_are_exact(plain, look):
    """Twelve consecutive frames of a depth-4 chain whose slot 3 runs on the caller's stream: bursts long enough
    to come round to every slot, a DeviceModel moved between frames, a frame without triangles, new arrays after
    a join.  Every framebuffer set holds, bit for bit, the plain filler's frame of the scene it was last given."""
    dm = _device_model()
    chain = _sharing(lookahead=look)
    chain.render_model(dm, clear=True)
    pose0 = plain(dm)
    for _ in range(5):                                 # slots 0 1 2 3 0
        chain.render_frame()
    pipe = chain._pipe
    assert pipe.depth == 4 and pipe.lookahead == look and pipe.shared_slot() == 3 and pipe.owned_streams() == 3
    _same(_planes(chain), pose0, "burst of five")
    _check_sets(chain, [pose0] * 4, "burst of five")
    dm.shift([0.06, -0.04, 0.1])                       # the model counts the rewrite: the chain joins and re-binds
    pose1 = plain(dm)
    chain.render_frame()
    chain.render_frame()                               # slots 0 1; 2 and 3 keep the old pose's frames
    _same(_planes(chain), pose1, "after a shift")
    _check_sets(chain, [pose1, pose1, pose0, pose0], "after a shift")
    none = _device(tuple(np.zeros((0, 3, 3), np.float32) for _ in range(3)))
    empty = plain(*none)
    chain.render_arrays(*none, clear=True)             # a plain frame: into the set of the last frame, set 1
    chain.render_frame()                               # slot 0
    _same(_planes(chain), empty, "no triangles")
    _check_sets(chain, [empty, empty, pose0, pose0], "no triangles")
    chain.join()
    soup = _device(_soup(21))
    want = plain(*soup)
    chain.render_arrays(*soup, clear=True)
    for _ in range(4):                                 # slots 0 1 2 3
        chain.render_frame()
    assert chain._pipe.shared_slot() == 3
    _same(_planes(chain), want, "new arrays after a join")
    _check_sets(chain, [want] * 4, "new arrays after a join")


def test_shared_slot_trex_256(plain):
    """T-Rex at 256 x 256 (8 x 8 tiles of 32): a burst that comes round twice."""
    from cython3dmodelrenderer_amd import scenes
    trex = _device(scenes.load_fixture("trex_inputs.npz"))
    ref = _filler(h=256, w=256)
    ref.render_arrays(*trex, clear=True)
    want = _planes(ref)
    chain = _sharing(h=256, w=256)
    chain.render_arrays(*trex, clear=True)
    for _ in range(9):
        chain.render_frame()
    assert chain._pipe.lookahead and chain._pipe.shared_slot() == 3
    _same(_planes(chain), want, "T-Rex 256")
    _check_sets(chain, [want] * 4, "T-Rex 256")


def test_frames_are_ordered_with_the_callers_own_work(plain):
    """The caller rewrites a resident input with torch kernels behind a join — behind a queue of other work of
    its own, so that the rewrite is still pending when the next frames are submitted — and reads the planes
    through the getters: nothing synchronises the host in between, and the frames are those of the new contents."""
    import torch
    old, new = _soup(31), _soup(32)
    want = plain(*_device(new))
    tri, col, nrm = _device(old)
    new_dev = _device(new)
    busy = torch.zeros(4096, 4096, device="cuda")
    chain = _sharing()
    chain.render_arrays(tri, col, nrm, clear=True)
    for _ in range(5):
        chain.render_frame()
    chain.join()
    torch.cuda.synchronize()
    for _ in range(20):                                # 20 passes over 64 MB: some hundreds of microseconds ahead of the rewrite
        busy.add_(1.0)
    for t, n in zip((tri, col, nrm), new_dev):
        t.copy_(n)
    chain.render_arrays(tri, col, nrm, clear=True)     # (bare tensors rewritten in place: handed in again)
    for _ in range(6):                                 # slots 0 1 2 3 0 1
        chain.render_frame()
    got = _planes(chain)                               # getters: a join, no host synchronisation
    bad = [int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)]
    assert bad == [0, 0, 0, 0], dict(zip(PLANES, bad))
    _check_sets(chain, [want] * 4, "rewritten inputs")


def test_the_shared_slot_follows_the_callers_stream(plain):
    import torch
    soup = _device(_soup(41))
    want = plain(*soup)
    chain = _sharing()
    chain.render_arrays(*soup, clear=True)
    default = torch.cuda.current_stream()
    for _ in range(5):
        chain.render_frame()
    pipe = chain._pipe
    assert pipe.shared_slot() == 3 and pipe._shared_raw == default.cuda_stream
    _same(_planes(chain), want, "burst on the default stream")
    side = torch.cuda.Stream()
    side_raw = side.cuda_stream
    assert side_raw != default.cuda_stream
    side.wait_stream(default)
    with torch.cuda.stream(side):
        for _ in range(6):
            chain.render_frame()
        assert pipe.shared_slot() == 3 and pipe._shared_raw == side_raw and pipe.owned_streams() == 3
        got = _planes(chain)
        _check_sets(chain, [want] * 4, "burst on a side stream")
    default.wait_stream(side)
    _same(got, want, "burst on a side stream")
    del side
    gc.collect()
    assert pipe._shared_raw == side_raw                # the chain keeps the stream it runs on alive
    for _ in range(5):
        chain.render_frame()
    assert pipe.shared_slot() == 3 and pipe._shared_raw == default.cuda_stream
    _same(_planes(chain), want, "back on the default stream")
    _check_sets(chain, [want] * 4, "back on the default stream")


def test_a_filler_deleted_with_frames_in_flight(plain):
    import torch
    soup = _device(_soup(51))
    want = plain(*soup)
    chain = _sharing()
    chain.render_arrays(*soup, clear=True)
    for _ in range(8):
        chain.render_frame()                           # two frames of the shared slot among them, none joined
    assert chain._pipe.pending
    del chain
    gc.collect()
    assert int(torch.arange(1000, device="cuda").sum().item()) == 499500
    again = _sharing()
    again.render_arrays(*soup, clear=True)
    for _ in range(5):
        again.render_frame()
    _same(_planes(again), want, "a new filler")


def test_depth_rule(monkeypatch):
    """GPU_MAX_HW_QUEUES is read by the constructor only (the runtime took its own reading when it started)."""
    def pick(**kw):
        f = _filler(pipeline=True, **kw)
        return f._pipeline_depth, f._share_caller_stream

    for queues in ("4", None, "2", "junk"):
        if queues is None:
            monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
        else:
            monkeypatch.setenv("GPU_MAX_HW_QUEUES", queues)
        assert pick() == pick(h=256, w=256) == pick(h=1024, w=1024) == (4, True), queues
        assert pick(share_caller_stream=False) == (3, False), queues       # the rule before the shared slot
        assert pick(share_caller_stream=True) == (4, True), queues
        assert pick(h=2048, w=2048) == (3, False), queues
        assert pick(pipeline_depth=4) == (4, False), queues                # an explicit depth: no sharing unless asked
        assert pick(pipeline_depth=2, share_caller_stream=True) == (2, True), queues
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")
    assert pick() == pick(h=1024, w=1024) == (4, False)
    assert pick(share_caller_stream=False) == (4, False)
    assert pick(share_caller_stream=True) == (4, True)
    assert pick(h=2048, w=2048) == (3, False)
    # and the chains those choices make: how many streams they own, which slot they share
    soup = _device(_soup(61))
    for queues, want in (("8", (4, 4, -1)), ("4", (4, 3, 3))):
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", queues)
        f = _filler(pipeline=True)
        f.render_arrays(*soup, clear=True)
        f.render_frame()
        f.join()
        assert (f._pipe.depth, f._pipe.owned_streams(), f._pipe.shared_slot()) == want, queues


def test_share_stream_argument_errors():
    import torch
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    soup = _device(_soup(71))
    chain = _sharing()
    chain.render_arrays(*soup, clear=True)
    chain.render_frame()
    handle = chain._pipe.handle
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.crender_pipeline_share_stream(handle, 2, stream) == _capi.EINVAL       # a frame in flight
    assert b"frames in flight" in lib.crender_last_error()
    chain.join()
    for slot in (-1, 4, 8):
        assert lib.crender_pipeline_share_stream(handle, slot, stream) == _capi.EINVAL, slot
        assert b"bad slot" in lib.crender_last_error()
    assert lib.crender_pipeline_shared_slot(handle) == 3 and lib.crender_pipeline_owned_streams(handle) == 3
    assert lib.crender_pipeline_share_stream(handle, 3, stream) == _capi.OK           # the same stream again
    assert lib.crender_pipeline_unshare(handle) == _capi.OK
    assert lib.crender_pipeline_shared_slot(handle) == -1 and lib.crender_pipeline_owned_streams(handle) == 4
    assert lib.crender_pipeline_unshare(handle) == _capi.OK                           # nothing left to do


def test_a_slot_handed_to_another_stream_stays_behind_its_earlier_frames(plain):
    """crender_pipeline_share_stream replacing a borrowed stream orders the new one behind the old one.  Slot 3
    renders scene A on the default stream, queued behind other work of the caller's; the join is the default
    stream's.  The slot is then handed to an IDLE side stream — nothing else orders that stream behind the default
    one, and the first frame after a join skips the hand-off from an idle caller — and renders scene B into the same
    framebuffer set with the same plan.  Without the event B would run first and A's frame would land on top of it."""
    import ctypes as C
    import torch
    from cython3dmodelrenderer_amd import _capi, lowlevel as L
    lib = _capi.load()
    a, b = _device(_soup(81)), _device(_soup(82))
    want = plain(*b)
    depth, T = 4, a[0].shape[0]
    P = _capi.f32_16(L.projection_matrix(45.0, 0.1, 1000.0, H, W))
    plans = [L.Plan(H, W, T) for _ in range(depth)]
    fbs = [L.FrameBuffers(H, W, winner=True) for _ in range(depth)]
    busy = torch.zeros(4096, 4096, device="cuda")
    side = torch.cuda.Stream()
    default = torch.cuda.current_stream().cuda_stream
    pipe = C.c_void_p()
    _capi.check(lib.crender_pipeline_create(C.byref(pipe), (C.c_void_p * depth)(*[p.handle.value for p in plans]), depth),
                "create")

    def burst(inputs, stream):
        t, c, n = inputs
        for fb in fbs:
            _capi.check(lib.crender_pipeline_frame(
                pipe, t.data_ptr(), c.data_ptr(), n.data_ptr(), T, P, fb.z.data_ptr(), fb.color.data_ptr(),
                fb.normals.data_ptr(), fb.winner.data_ptr(), _capi.FUSED_CLEAR | _capi.OVERLAPPED_FRAMES, stream), "frame")
    try:
        _capi.check(lib.crender_pipeline_share_stream(pipe, depth - 1, default), "share")
        torch.cuda.synchronize()
        for _ in range(20):                            # 20 passes over 64 MB ahead of scene A's frames
            busy.add_(1.0)
        burst(a, default)
        _capi.check(lib.crender_pipeline_join(pipe, default), "join")
        _capi.check(lib.crender_pipeline_share_stream(pipe, depth - 1, side.cuda_stream), "share again")
        assert lib.crender_pipeline_shared_slot(pipe) == depth - 1
        burst(b, side.cuda_stream)
        _capi.check(lib.crender_pipeline_join(pipe, side.cuda_stream), "join")
        torch.cuda.synchronize()
        for k, fb in enumerate(fbs):
            _same((fb.z, fb.color, fb.normals, fb.winner), want, f"scene B, framebuffer set {k}")
    finally:
        torch.cuda.synchronize()
        lib.crender_pipeline_unshare(pipe)
        lib.crender_pipeline_destroy(pipe)
