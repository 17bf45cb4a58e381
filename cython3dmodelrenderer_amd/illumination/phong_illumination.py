"""Per-pixel Blinn-Phong lighting: an ambient term, up to four point or directional lights, a specular term.

    colour = min(colour * (ambient + sum kd_j * d_j) + (sum ks_j * sp_j ** shininess) * specular_color, clamp)

with d_j the Guro factor of a pixel's normal under the unit vector towards light j and sp_j that of the half vector
between it and the direction to the camera (include/crender_phong.h states every operation).  The model needs the
surface point a pixel shows, which the colour and normal planes do not carry: it exists as a device pass over the
filler's winner plane only (``AdvancedPixelBufferFiller.phong_pass``, the HIP kernel ``crender_phong_shade``), and
``draw_illumination`` on two host planes raises.
"""
import numpy as np

from .guro_illumination import GuroIllumination
from .illumination_drawer import IlluminationDrawer

MAX_LIGHTS = 4
MAX_SHININESS = 4096


def shininess_log2(shininess):
    """k of a specular exponent 2^k, 1 <= 2^k <= 4096."""
    ok = isinstance(shininess, (int, np.integer)) and not isinstance(shininess, bool) and \
        1 <= shininess <= MAX_SHININESS and shininess & (shininess - 1) == 0
    if not ok:
        raise ValueError(f"shininess must be a power of two from 1 to {MAX_SHININESS}, got {shininess!r}")
    return int(shininess).bit_length() - 1


def light_rows(lights):
    """([(x, y, z, kd, ks)] as Python floats holding float32 values, the mask whose bit j says that light j is a
    direction) of a list of light dicts; a direction goes through ``GuroIllumination``'s own statements."""
    if not isinstance(lights, (list, tuple)) or not 1 <= len(lights) <= MAX_LIGHTS:
        n = len(lights) if isinstance(lights, (list, tuple)) else repr(lights)
        raise ValueError(f"lights must be a list of 1 to {MAX_LIGHTS} dicts, got {n}")
    rows, mask = [], 0
    for j, light in enumerate(lights):
        extra = set(light) - {"position", "direction", "diffuse", "specular"}
        if extra:
            raise ValueError(f"light {j}: unknown keys {sorted(extra)}")
        if ("position" in light) == ("direction" in light):
            raise ValueError(f"light {j} needs exactly one of 'position' and 'direction'")
        if "diffuse" not in light or "specular" not in light:
            raise ValueError(f"light {j} needs 'diffuse' and 'specular'")
        if "direction" in light:
            vec = GuroIllumination(light["direction"]).light_direction
            mask |= 1 << j
        else:
            vec = np.asarray(light["position"], dtype="float32")
        if vec.shape != (3,):
            raise ValueError(f"light {j}: the vector must have three components, got shape {vec.shape}")
        rows.append([float(v) for v in vec] + [float(np.float32(light["diffuse"])), float(np.float32(light["specular"]))])
    return rows, mask


class PhongIllumination(IlluminationDrawer):
    def __init__(self, position=None, direction=None, ambient=0.1, diffuse=0.9, specular=0.5, shininess=32,
                 specular_color=(255, 255, 255), clamp=255.0, lights=None):
        if lights is not None:
            if position is not None or direction is not None:
                raise ValueError("PhongIllumination: give one light through position / direction or several through "
                                 "lights=[...], not both")
            lights = [dict(light) for light in lights]
        else:
            if (position is None) == (direction is None):
                raise ValueError("PhongIllumination needs exactly one of position and direction (or lights=[...])")
            which = {"position": position} if position is not None else {"direction": direction}
            lights = [dict(which, diffuse=diffuse, specular=specular)]
        light_rows(lights)
        shininess_log2(shininess)
        self.lights = lights
        self.ambient, self.shininess, self.clamp = ambient, shininess, clamp
        self.specular_color = tuple(specular_color)

    def draw_illumination(self, color_buffer, n_buffer):
        raise ValueError("PhongIllumination needs the winner plane and the triangles (the surface point a pixel shows), "
                         "which the colour and normal planes do not carry: render with Renderer(on_device=None) or "
                         "on_device=True, where the filler's phong_pass runs on the device")

    def draw_illumination_device(self, filler):
        if not hasattr(filler, "phong_pass"):
            raise ValueError(f"PhongIllumination needs a filler with a Phong pass (AdvancedPixelBufferFiller): "
                             f"{type(filler).__name__} has no phong_pass()")
        filler.phong_pass(self.lights, ambient=self.ambient, shininess=self.shininess,
                          specular_color=self.specular_color, clamp=self.clamp)
        return True
