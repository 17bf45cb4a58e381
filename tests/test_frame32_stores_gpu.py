"""The small-scene frame kernel's stores (csrc/frame32.hip: resolve_tile_rows, resolve_tile): a covered tile's pixels leave
a wavefront as whole 16-byte-aligned rows where the frame allows it, pixel by pixel where it does not.

Every case runs on plans with 32-pixel tiles, asserts ``crender_frame32_last`` (no case passes by delegating) and
compares the three planes as uint32, bit for bit, against the oracle AND against the same frames through
crender_pipeline_submit (the general kernel): nothing here is a tolerance.  The planes of every case are views into
larger buffers filled with a sentinel word, rendered rows included: a frame must replace every word of its rows and
no word outside them, so a 16-byte store that reaches past a row's end, or a row that nobody stores, shows.

The harness is tests/test_frame32_gpu.py's chain with the framebuffers (and, for the row strip, the plans) replaced."""
import ctypes as C

import numpy as np
import pytest

from test_frame32_gpu import FOV, Chain, _capi, _device, _soup, _tile_scene, _want
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF          # (a NaN no arithmetic of a frame produces)
GUARD = 64                     # floats on either side of a plane: 256 bytes, so an aligned plane stays aligned


class GuardedPlanes:
    """z [H,W], colour [H,W,3], normal [H,W,3] as views into sentinel-filled buffers, `GUARD` floats on either side;
    plane i begins `skew[i]` more floats (4 bytes each) into its buffer."""

    def __init__(self, h, w, skew=(0, 0, 0)):
        import torch
        self.h, self.w, self.skew, self.bufs, views = h, w, skew, [], []
        for ch, s in zip((1, 3, 3), skew):
            n = h * w * ch
            buf = torch.empty(GUARD + s + n + GUARD, dtype=torch.float32, device="cuda")
            buf.view(torch.int32).fill_(SENTINEL)
            assert buf.data_ptr() % 16 == 0
            self.bufs.append(buf)
            views.append(buf[GUARD + s:GUARD + s + n].view((h, w) if ch == 1 else (h, w, ch)))
        self.z, self.color, self.normals = views
        self.winner = None

    def check(self, want, y0, y1, what):
        """Rows [y0, y1) are `want`'s, every other word of the buffers is still the sentinel."""
        for buf, s, ch, w_, name in zip(self.bufs, self.skew, (1, 3, 3), want, ("z", "colour", "normal")):
            got = buf.cpu().numpy().view(np.uint32)
            row = self.w * ch
            lo, hi = GUARD + s + y0 * row, GUARD + s + y1 * row
            assert_bit_equal(got[lo:hi].reshape(w_[y0:y1].shape), w_[y0:y1], f"{what}: {name}")
            out = np.concatenate([got[:lo], got[hi:]])
            bad = np.flatnonzero(out != SENTINEL)
            assert len(bad) == 0, (f"{what}: {name}: {len(bad)} words outside rows [{y0}, {y1}) were written; first at "
                                   f"buffer word {bad[0] if bad[0] < lo else bad[0] + hi - lo} (rows begin at {lo}, end at {hi})")


class GuardedChain(Chain):
    """Chain over GuardedPlanes; `rows` = (y0, y1): plans of a row strip."""

    def __init__(self, h, w, max_T, depth, frame32, rows=None, skew=(0, 0, 0)):
        import torch
        from cython3dmodelrenderer_amd import lowlevel as L
        capi = _capi()
        self.lib, self.capi, self.h, self.w, self.depth, self.frame32 = capi.load(), capi, h, w, depth, frame32
        self.y0, self.y1 = rows or (0, h)
        self.plans = [L.Plan(h, w, max_T, y0=self.y0, y1=self.y1, tile=32) for _ in range(2 * depth)]
        self.fbs = [GuardedPlanes(h, w, skew) for _ in range(depth)]
        self.P = capi.f32_16(L.projection_matrix(FOV, 0.1, 1000.0, h, w))
        self.stream = torch.cuda.current_stream().cuda_stream
        self.pipe = C.c_void_p()
        arr = lambda ps: (C.c_void_p * depth)(*[p.handle.value for p in ps])
        capi.check(self.lib.crender_pipeline_create(C.byref(self.pipe), arr(self.plans[:depth]), depth), "create")
        capi.check(self.lib.crender_pipeline_set_lookahead(self.pipe, arr(self.plans[depth:]), depth), "lookahead")
        self.inputs = None

    def check(self, want, what):
        for k, fb in enumerate(self.fbs):
            fb.check(want, self.y0, self.y1, f"{what} set {k}")


def _both(oracle, scene, h, w, depth, drive, what, static=False, **kw):
    """`drive(chain)` on a chain of the small-scene kernel and on one of the general kernel, over guarded planes:
    each against the oracle bit for bit with its guards intact, then the two against each other."""
    capi = _capi()
    want = _want(oracle, scene, h, w)
    dev = _device(scene)
    flags = capi.FUSED_CLEAR | capi.OVERLAPPED_FRAMES | (capi.STATIC_INPUTS if static else 0)
    new, old = (GuardedChain(h, w, len(scene[0]), depth, f32, **kw) for f32 in (True, False))
    for chain, name in ((new, "frame32"), (old, "general kernel")):
        chain.bind(dev, flags=flags)
        drive(chain)
        chain.check(want, f"{what}, {name} against the oracle")
    for k in range(depth):
        for a, b, name in zip(new.planes(k), old.planes(k), ("z", "colour", "normal")):
            assert_bit_equal(a[new.y0:new.y1], b[new.y0:new.y1], f"{what} set {k} against the general kernel: {name}")
    new.close(); old.close()
    return want


def _burst(chain):
    """Every slot twice and once more, nothing joined in between."""
    for _ in range(2 * chain.depth + 1):
        chain.submit(expect=True)
    chain.join()


def _settled(chain):
    """test_frame32_gpu._rounds(chain, 2): from the third frame on the bins are the kernel's own binning wavefronts',
    and a tile's split flag is what an earlier frame's lengths set."""
    for _ in range(2):
        for _ in range(chain.depth):
            chain.submit(expect=True)
        chain.join()
    chain.frame(expect=True)


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("hw, rows", [((64, 64), None), ((72, 100), None), ((72, 98), None), ((64, 64), (8, 56))],
                         ids=["64x64", "72x100", "72x98", "64x64-rows-8-56"])
def test_sizes_and_edges(oracle, hw, rows, depth):
    """64 x 64: full tiles, every covered one stored as rows.  72 x 100: 16-byte rows, the last tile column 4 pixels
    wide (stored pixel by pixel beside tiles stored as rows) and the last tile row cut after 8 rows.  72 x 98: no
    16-byte rows, the whole frame pixel by pixel.  Rows 8..56 of 64: tiles that begin at row 8, the second cut after
    16 rows, and the rows around the strip are nobody's."""
    h, w = hw
    scene = _soup(11, 300, w)
    _both(oracle, scene, h, w, depth, _burst, f"{h}x{w} rows {rows} depth {depth}", rows=rows)


@pytest.mark.parametrize("plane", [0, 1, 2], ids=["z", "colour", "normal"])
def test_a_plane_that_is_not_16_byte_aligned(oracle, plane):
    """One plane begins 4 bytes into its buffer: no plane of the frame is stored in 16-byte words."""
    skew = tuple(int(i == plane) for i in range(3))
    scene = _soup(12, 300, 64)
    new = GuardedChain(64, 64, 300, 2, True, skew=skew)
    assert [t.data_ptr() % 16 for t in (new.fbs[0].z, new.fbs[0].color, new.fbs[0].normals)] == [4 * s for s in skew]
    new.close()
    _both(oracle, scene, 64, 64, 2, _burst, f"plane {plane} skewed", skew=skew)


@pytest.mark.parametrize("n", [40, 100, 300])
def test_split_tiles(oracle, n):
    """A tile of 40 records is split into halves (rows of 32 pixels, 16 of them), one of 100 into quadrants (rows of
    16 pixels, four to a wavefront pass); with 300 the winners of the first batch are shaded from global memory, those
    of the second from the queue, and the rest of the tile is background: all three in one wavefront pass."""
    scene = _tile_scene(oracle, n)
    want = _both(oracle, scene, 64, 64, 2, _settled, f"{n} records", static=True)
    tile = want[0][32:, 32:]
    assert (tile < 1e6).any() and (tile == 1e6).any()


def test_words_whose_bits_matter(oracle):
    """Triangles whose interpolated colour is -0.0 and triangles with a NaN in the normal's x, in rows that also hold
    background pixels: the staged words are the shaded words, not equal-comparing ones."""
    h = w = 64
    scene = [a.copy() for a in _soup(13, 300, w, size=(2, 12), frac_backface=0.0)]
    scene[1][0::3] = -0.0
    scene[2][1::3, 0, 0] = np.nan
    want = _want(oracle, scene, h, w)
    bg = want[0] == 1e6
    neg0 = (want[1].view(np.uint32) == 0x80000000).all(axis=2) & ~bg
    nan = np.isnan(want[2][:, :, 0]) & ~bg
    assert (neg0.any(axis=1) & bg.any(axis=1)).any() and (nan.any(axis=1) & bg.any(axis=1)).any()
    _both(oracle, scene, h, w, 2, _burst, "-0.0 colours and NaN normals")


def test_a_join_mid_burst_and_inputs_rewritten_in_place(oracle):
    """The staging space is the queue's: a frame whose queue the stores overwrote is followed by fresh ones.  A burst
    cut by a join goes on with the same scene; then the arrays are rewritten in place behind a join and the next
    frames are the new contents' (test_frame32_gpu.test_inputs_rewritten_in_place_and_a_join_mid_burst)."""
    h, w, depth = 80, 96, 4
    a, b = _soup(41, 300, w), _soup(42, 300, w)
    want_a, want_b = _want(oracle, a, h, w), _want(oracle, b, h, w)
    dev, dev_b = _device(a), _device(b)
    chains = [GuardedChain(h, w, 300, depth, f32) for f32 in (True, False)]
    for chain in chains:
        chain.bind(dev)
        for _ in range(6):
            chain.submit(expect=True)
        chain.join()                                 # mid-burst: slots 0 and 1 have come round
        for _ in range(3):
            chain.submit(expect=True)
        chain.join()
        chain.check(want_a, "scene a")
    planes_a = [[chain.planes(k) for k in range(depth)] for chain in chains]
    for t, n in zip(dev, dev_b):
        t.copy_(n)
    for chain in chains:
        chain.bind(dev)
        for _ in range(depth + 1):
            chain.submit(expect=True)
        chain.join()
        chain.check(want_b, "rewritten in place")
    new, old = chains
    for k in range(depth):
        for x, y, name in zip(planes_a[0][k], planes_a[1][k], ("z", "colour", "normal")):
            assert_bit_equal(x, y, f"scene a set {k} against the general kernel: {name}")
        for x, y, name in zip(new.planes(k), old.planes(k), ("z", "colour", "normal")):
            assert_bit_equal(x, y, f"rewritten in place set {k} against the general kernel: {name}")
    new.close(); old.close()
