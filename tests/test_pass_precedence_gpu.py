"""Which refusal of a deferred pass wins when several apply: for each of texture_pass, shadow_pass, phong_pass,
ao_pass and wire_pass the state in which every precondition is violated at once (as far as they can coexist), then one violation
repaired at a time, down to a call that succeeds.  Every refusal is asserted by its whole message.  16 x 16 fillers,
one triangle, an 8 x 8 texture: the refused calls never reach the library, and each pass launches once at the end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRI = np.float32([[[-0.3, -0.3, 1.5], [0.3, -0.3, 1.5], [0.0, 0.3, 1.5]]])
COL = np.full((1, 3, 3), 100.0, np.float32)
NRM = np.float32([[[0.0, 0.0, -1.0]] * 3])
COMPOSITE = "did not start from cleared buffers (clear=True): the winner plane of a composite mixes the triangle indices of several models"


def _fillers():
    """A swap chain, a filler without the winner plane and one with it: none has rendered or bound anything."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    return (AdvancedPixelBufferFiller(16, 16, fov=45, pipeline=True), AdvancedPixelBufferFiller(16, 16, fov=45),
            AdvancedPixelBufferFiller(16, 16, fov=45, track_winner=True))


def _refused(message, call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    assert str(e.value) == message


def _frames(f, name, call, **kw):
    """The last two refusals of every pass, on a filler that has rendered nothing; leaves a cleared frame."""
    _refused(f"{name}: no frame has been rendered", call, **kw)
    f.render_arrays(TRI, COL, NRM)
    _refused(f"{name}: the last frame {COMPOSITE}", call, **kw)
    f.render_arrays(TRI, COL, NRM, clear=True)


def _covered(f):
    """The colours of the covered pixels; the background is as the clear left it."""
    color = f.get_color_tensor().cpu().numpy()
    covered = f.get_winner_tensor().cpu().numpy() >= 0
    assert covered.any() and not covered.all()
    assert (color[~covered] == 0).all()
    return color[covered]


def test_texture_pass_refusals_in_order():
    chain, nowin, f = _fillers()
    uv = np.float32([[[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]]])
    tex = np.random.default_rng(5).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    _refused("filter must be 'nearest', 'bilinear' or 'trilinear', got 'cubic'", chain.texture_pass, filter="cubic", anisotropy=17)
    _refused("anisotropy must be an int from 1 to 16, got 17", chain.texture_pass, filter="bilinear", anisotropy=17)
    _refused("anisotropy=2 needs filter=\"trilinear\" (and its mip chain), got 'bilinear'", chain.texture_pass,
             filter="bilinear", anisotropy=2)
    kw = dict(filter="trilinear", anisotropy=2)
    _refused("texture_pass is not available on a swap chain (pipeline=True): per-slot passes are not implemented",
             chain.texture_pass, **kw)
    _refused("texture_pass needs the winner plane: construct the filler with track_winner=True", nowin.texture_pass, **kw)
    _refused("texture_pass: no texture is bound (bind_texture)", f.texture_pass, **kw)
    f.bind_texture(np.concatenate([uv, uv]), tex)
    _refused("filter 'trilinear' needs a mip chain: bind_texture(..., mipmaps=True)", f.texture_pass, **kw)
    f.bind_texture(np.concatenate([uv, uv]), tex, mipmaps=True)
    _refused("texture_pass: no frame has been rendered", f.texture_pass, **kw)
    f.render_arrays(TRI, COL, NRM)
    _refused(f"texture_pass: the last frame {COMPOSITE}", f.texture_pass, **kw)
    f.render_arrays(TRI, COL, NRM, clear=True)
    _refused("texture_pass: 2 triangles of texture coordinates are bound, the last frame drew 1", f.texture_pass, **kw)
    f.bind_texture(uv, tex, mipmaps=True)
    before = _covered(f)
    f.texture_pass(**kw)
    assert (_covered(f) != before).any()


def test_shadow_pass_refusals_in_order():
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    chain, nowin, f = _fillers()
    g = AdvancedPixelBufferFiller(16, 16, fov=45, track_winner=True)
    composite = "did not start from cleared buffers (clear=True): the planes of a composite mix several models"
    _refused("shadow_pass is not available on a swap chain (pipeline=True): per-slot passes are not implemented",
             chain.shadow_pass, pcf=2)
    _refused("shadow_pass needs the winner plane: construct the filler with track_winner=True", nowin.shadow_pass, pcf=2)
    _refused("shadow_pass: no shadow map is bound (bind_shadow_map)", f.shadow_pass, pcf=2)
    f.bind_shadow_map(g, np.concatenate([TRI, TRI]))
    _refused("shadow_pass: no frame has been rendered by the camera's filler", f.shadow_pass, pcf=2)
    f.render_arrays(TRI, COL, NRM)
    _refused(f"shadow_pass: the last frame of the camera's filler {composite}", f.shadow_pass, pcf=2)
    f.render_arrays(TRI, COL, NRM, clear=True)
    _refused("shadow_pass: no frame has been rendered by the light's filler", f.shadow_pass, pcf=2)
    g.render_arrays(TRI, COL, NRM)
    _refused(f"shadow_pass: the last frame of the light's filler {composite}", f.shadow_pass, pcf=2)
    g.render_arrays(TRI, COL, NRM, clear=True)
    _refused("shadow_pass: 2 triangles of light-frame vertices are bound, the light's last frame drew 1, the camera's 1",
             f.shadow_pass, pcf=2)
    f.bind_shadow_map(g, TRI)
    _refused("pcf must be 1, 3 or 5, got 2", f.shadow_pass, pcf=2)
    before = _covered(f)
    f.shadow_pass(pcf=3)                                   # (the light sees what the camera sees: nothing is shadowed)
    assert np.array_equal(_covered(f), before)


def test_phong_pass_refusals_in_order():
    chain, nowin, f = _fillers()
    lights = [dict(direction=(0.0, 0.0, 1.0), diffuse=0.5, specular=0.0)]
    _refused("phong_pass is not available on a swap chain (pipeline=True): per-slot passes are not implemented",
             chain.phong_pass, [], shininess=3)
    _refused("phong_pass needs the winner plane: construct the filler with track_winner=True", nowin.phong_pass, [], shininess=3)
    _refused("lights must be a list of 1 to 4 dicts, got 0", f.phong_pass, [], shininess=3)
    _refused("shininess must be a power of two from 1 to 4096, got 3", f.phong_pass, lights, shininess=3)
    _frames(f, "phong_pass", f.phong_pass, lights=lights, shininess=4)
    before = _covered(f)
    f.phong_pass(lights, shininess=4)
    assert (_covered(f) != before).any()


def test_ao_pass_refusals_in_order():
    chain, nowin, f = _fillers()
    count = "taps must be a count from 1 to 64 or a list of (dx, dy) pairs, got "
    kw = dict(normals="vertex", radius_px=0, taps=0)
    _refused("ao_pass is not available on a swap chain (pipeline=True): per-slot passes are not implemented", chain.ao_pass, **kw)
    _refused("ao_pass needs the winner plane: construct the filler with track_winner=True", nowin.ao_pass, **kw)
    _refused("normals must be 'plane' or 'face', got 'vertex'", f.ao_pass, **kw)
    kw["normals"] = "face"
    _refused("radius_px must be an int from 1 to 32, got 0", f.ao_pass, **kw)
    kw["radius_px"] = 2
    for taps, message in ((0, count + "0"), (65, count + "65"), (1.5, count + "1.5"), (True, count + "True"),
                          ([(1, 0), 3], count + "[(1, 0), 3]"), ([], "taps must hold 1 to 64 pairs, got 0"),
                          ([(1, 0)] * 65, "taps must hold 1 to 64 pairs, got 65"),
                          ([(1, 0), (3, 0)], "the tap (3, 0) is (0, 0) or reaches beyond radius_px=2"),
                          ([(0, 0)], "the tap (0, 0) is (0, 0) or reaches beyond radius_px=2")):
        kw["taps"] = taps
        _refused(message, f.ao_pass, **kw)
    kw["taps"] = [(1, 0), (0, -2)]
    _frames(f, "ao_pass", f.ao_pass, **kw)
    before = _covered(f)
    f.ao_pass(**kw)                                        # (one flat triangle: nothing occludes it)
    assert np.array_equal(_covered(f), before)


def test_wire_pass_refusals_in_order():
    """wire_pass asks whom it serves first (the swap chain, the winner plane), then reads its own arguments in the order
    width, feather, opacity, depth_bias, radius_px — the last two with `outline` alone — then the frame, and `edges`
    last, as it is measured against the frame's triangle count."""
    chain, nowin, f = _fillers()
    number = "must be a number of pixels above 0 and at most 64, got "
    kw = dict(outline=True, width=0.0, feather=65.0, opacity=1.5, depth_bias=float("nan"), radius_px=9,
              edges=np.zeros(2, np.int32))
    _refused("wire_pass is not available on a swap chain (pipeline=True): per-slot passes are not implemented", chain.wire_pass, **kw)
    _refused("wire_pass needs the winner plane: construct the filler with track_winner=True", nowin.wire_pass, **kw)
    _refused("width " + number + "0.0", f.wire_pass, **kw)
    kw["width"] = 10.0
    _refused("feather " + number + "65.0", f.wire_pass, **kw)
    kw["feather"] = 4.5
    _refused("opacity must be a number from 0 to 1, got 1.5", f.wire_pass, **kw)
    kw["opacity"] = 0.5
    _refused("depth_bias must be a finite number, got nan", f.wire_pass, **kw)
    kw["depth_bias"] = 1e-3
    _refused("radius_px must be None or an int from 0 to 8, got 9", f.wire_pass, **kw)
    kw["radius_px"] = None
    _refused("outline=True: width + feather = 14.5 needs radius_px = 9, above the largest, 8: width + feather may be at most 14",
             f.wire_pass, **kw)
    kw["feather"] = 4.0                                    # (the widest line the default radius holds)
    # an overlay does not look at the outline's two arguments
    _refused("wire_pass: no frame has been rendered", f.wire_pass, **dict(kw, outline=False, depth_bias=float("nan"), radius_px=9))
    _frames(f, "wire_pass", f.wire_pass, **kw)
    _refused("edges must be uint8 [T] with T = 1, the triangles of the last frame, got torch.int32 (2,)", f.wire_pass, **kw)
    kw["edges"] = np.zeros(2, np.uint8)
    _refused("edges must be uint8 [T] with T = 1, the triangles of the last frame, got torch.uint8 (2,)", f.wire_pass, **kw)
    kw["edges"] = np.full(1, 7, np.uint8)
    before = _covered(f)
    f.wire_pass(**dict(kw, outline=False))
    assert (_covered(f) != before).any()
    f.render_arrays(TRI, COL, NRM, clear=True)
    f.wire_pass(**kw)                                      # (the outline writes the background too: the outer half of a line)
    color = f.get_color_tensor().cpu().numpy()
    covered = f.get_winner_tensor().cpu().numpy() >= 0
    assert (color[covered] != before).any() and (color[~covered] != 0).any()
