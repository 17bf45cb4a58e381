"""The host-view protocol of the fillers that keep their planes in HBM
(cython3dmodelrenderer_amd/pixel_buffer_filler/_device_planes.py), on a machine without a GPU and
without the built library: a fake filler derived from the shared class, whose planes are CPU tensors
and whose leaf methods (allocation, pinned buffers, the library calls) write into them directly.
Its ``render`` does around its "kernel" what ``render_model`` / ``render_arrays`` of the real
fillers do around their launch.  Every ``Tensor.copy_`` between a plane and the buffer behind a
view is logged as ("up" | "down", plane name).

Cases 3 and 4 are the two defects of this state machine that only random sessions on the GPU had found."""
import numpy as np
import pytest
import torch

from cython3dmodelrenderer_amd.illumination import GuroIllumination
from cython3dmodelrenderer_amd.pixel_buffer_filler._device_planes import DevicePlanes

H, W = 4, 5
INITIAL = {"z": 1e6, "color": 0.0, "normals": 0.0}


class FakeFiller(DevicePlanes):
    def __init__(self):
        super().__init__()
        self.h, self.w = H, W
        self.redo = []             # values a frame is "rendered again" with, one per _wait_planes call
        self.readied = self.waits = 0
        self.lights = []
        self._allocate_planes()

    # ---- hooks
    def _ready_planes(self):
        self.readied += 1

    def _wait_planes(self):
        self.waits += 1
        if not self.redo:
            return False
        self._fill(self.redo.pop(0))
        return True

    def synchronize(self):
        self._wait_planes()

    # ---- leaves
    def _allocate_planes(self, track_winner=False):
        self.z_buffer = torch.full((H, W), INITIAL["z"], dtype=torch.float32)
        self.color_buffer = torch.zeros((H, W, 3), dtype=torch.float32)
        self.normals_buffer = torch.zeros((H, W, 3), dtype=torch.float32)

    def _pinned_like(self, buf):
        return torch.full(tuple(buf.shape), -1.0, dtype=buf.dtype)

    def _clear_planes(self):
        for name, plane in self._planes().items():
            plane.fill_(INITIAL[name])

    def _shade_planes(self, light):
        self.lights.append(np.asarray(light))
        self.color_buffer.mul_(0.5)

    # ---- the "kernels"
    def _fill(self, value):
        for plane in self._planes().values():
            plane.fill_(value)

    def render(self, value, clear=False, refresh_views=True):
        """Composites by ADDING `value` to every plane (so that what the planes held before shows in
        the result); ``clear=True`` starts from cleared planes in the same pass (planes = value)."""
        if clear:
            self._host_exposed = False         # (a plain store in the real fillers' per-frame paths too)
            self._fill(0.0)
        else:
            self._push_host_edits()
        for plane in self._planes().values():
            plane.add_(value)
        self._host_fresh = False
        if self._host and refresh_views:
            self._refresh_mirrors()

    def render_frame(self, value):
        self.render(value, clear=True, refresh_views=False)


@pytest.fixture
def log(monkeypatch):
    """-> (make a filler, the list of copies between its planes and its views' buffers)."""
    copies, fillers = [], []
    real = torch.Tensor.copy_

    def copy_(dst, src, non_blocking=False):
        for f in fillers:
            for name, pin in f._host_pin.items():
                plane = f._planes()[name]
                if dst is pin and src is plane:
                    copies.append(("down", name))
                elif dst is plane and src is pin:
                    copies.append(("up", name))
        return real(dst, src, non_blocking=non_blocking)

    monkeypatch.setattr(torch.Tensor, "copy_", copy_)

    def make():
        fillers.append(FakeFiller())
        return fillers[-1]
    return make, copies


def test_only_planes_handed_out_are_copied_once_each_way_per_render(log):
    make, copies = log
    f = make()
    f.render(1.0)
    f.render(2.0, clear=True)
    f.clear()
    f.render_frame(3.0)
    assert copies == [] and not f._host and not f._host_pin and f.waits == 0
    view = f.get_color_buffer()
    assert copies == [("down", "color")] and (view == 3.0).all()
    for k in range(3):
        del copies[:]
        f.render(1.0)
        assert sorted(copies) == [("down", "color"), ("up", "color")], k
    del copies[:]
    f.render(1.0, refresh_views=False)
    f.render(1.0, refresh_views=False)
    assert copies == [("up", "color")]         # (the view was the caller's to edit once more, after the last refresh)
    assert (f.get_color_buffer() == 8.0).all() and copies == [("up", "color"), ("down", "color")]
    assert set(f._host) == set(f._host_pin) == {"color"}
    z = f.get_z_buffer()
    assert (z == 8.0).all() and copies[2:] == [("down", "z")]


def test_an_array_handed_out_earlier_shows_a_later_render(log):
    f = log[0]()
    f.render(1.0)
    color, z = f.get_color_buffer(), f.get_z_buffer()
    assert (color == 1.0).all() and (z == np.float32(1e6) + 1).all()
    f.render(2.0)
    assert (color == 3.0).all() and f.get_color_buffer() is color and f.get_z_buffer() is z
    f.render(5.0, clear=True)
    assert (color == 5.0).all() and (z == 5.0).all()


def test_an_edit_after_a_render_without_another_getter_call_reaches_the_planes(log):
    f = log[0]()
    view = f.get_color_buffer()
    f.render(1.0)                              # refreshes the view: it is the caller's to write into again
    assert (view == 1.0).all()
    view[0, 0] = 50.0
    f.render(2.0)
    assert (f.color_buffer[0, 0] == 52.0).all() and (f.color_buffer[1:] == 3.0).all()
    assert (view[0, 0] == 52.0).all() and (view[1:] == 3.0).all()


@pytest.mark.parametrize("frame", ["cleared in the same pass", "clear() then a render"])
def test_a_stale_view_is_not_written_over_a_frame_that_started_from_cleared_planes(log, frame):
    f = log[0]()
    view = f.get_color_buffer()
    view[:] = 99.0
    if frame == "cleared in the same pass":
        f.render_frame(5.0)
    else:
        f.clear()
        f.render(5.0, refresh_views=False)
    assert (view == 99.0).all()                # stale, and void
    f.render(1.0, refresh_views=False)
    assert (f.color_buffer == 6.0).all()
    assert f.get_color_buffer() is view and (view == 6.0).all()


def test_clear_voids_pending_edits_and_the_views_show_the_initial_state(log):
    make, copies = log
    f = make()
    f.render(4.0)
    color, z, normals = f.get_color_buffer(), f.get_z_buffer(), f.get_normals_buffer()
    color[:] = 9.0
    z[:] = 9.0
    del copies[:]
    f.clear()
    assert copies == [] and not f._host_exposed and not f._host_fresh
    assert (f.color_buffer == 0).all() and (f.z_buffer == 1e6).all()
    assert (color == 9.0).all()                # until the next getter call
    assert f.get_color_buffer() is color and (color == 0).all()
    assert (z == np.float32(1e6)).all() and (normals == 0).all()
    f.render(1.0)
    assert (color == 1.0).all()


def test_a_frame_rendered_again_is_copied_again(log):
    make, copies = log
    f = make()
    view = f.get_color_buffer()
    f.redo = [7.0, 8.0]
    del copies[:]
    f.waits = 0
    f.render(1.0)
    assert f.waits == 3 and not f.redo         # called until it reports False
    assert copies == [("up", "color")] + [("down", "color")] * 3
    assert (view == 8.0).all() and f._host_fresh
    f.redo = [2.0]
    z = f.get_z_buffer()                       # the first copy of a plane newly handed out, too
    assert (z == 2.0).all() and copies[4:] == [("down", "z")] * 2


def test_the_shading_call_leaves_the_views_stale(log):
    f = log[0]()
    f.render(4.0)
    view = f.get_color_buffer()
    view[0, 0] = 10.0
    light = GuroIllumination((0.3, -0.2, 1.0))
    assert light.draw_illumination_device(f) is True
    assert len(f.lights) == 1 and np.array_equal(f.lights[0], light.light_direction)
    assert not f._host_fresh
    assert (view[1:] == 4.0).all()             # stale until the next getter call
    assert f.get_color_buffer() is view
    assert (view[0, 0] == 5.0).all() and (view[1:] == 2.0).all()     # the edit was carried up first
    f.shade_guro(light.light_direction.tolist())
    assert not f._host_fresh and f.get_color_buffer() is view and (view[1:] == 1.0).all()
