"""Scene description types — the input data model of the render path.

Mirrors the reference's domain layer (`/root/reference/ray_tracer/domain.py:5-59`) name for name
so a scene written against the reference reads the same here:

* ``Vector3D`` / ``RGBColor``     — ``domain.py:5-11``
* ``Camera``                      — ``domain.py:14-23`` (position, width, height)
* ``PointLight``                  — ``domain.py:26-30``
* ``DomeLight``                   — ``domain.py:33-40``
* ``Shape`` (ABC)                 — ``domain.py:43-50``
* ``Scene3D``                     — ``domain.py:53-59``

These are plain host-side containers. The HIP backend flattens them into one float64 blob per
scene (see ``infrastructure/hip/scene_pack.py``); nothing here touches the GPU.
"""

from __future__ import annotations

from abc import ABC, abstractmethod
from dataclasses import dataclass


class Vector3D:
    """Three components, scalars or arrays (reference ``domain.py:5-7``)."""

    def __init__(self, x, y, z) -> None:
        (self.x, self.y, self.z) = (x, y, z)

    def components(self) -> tuple:
        return (self.x, self.y, self.z)

    def __repr__(self) -> str:
        return f"{type(self).__name__}({self.x!r}, {self.y!r}, {self.z!r})"


class RGBColor(Vector3D):
    """Reference ``domain.py:10-11``."""


@dataclass
class Camera:
    """Observation point; the screen is fixed at world z=0 (reference ``domain.py:14-23``,
    screen construction in ``infrastructure/numpy/base.py:123-141``)."""

    position: Vector3D
    width: int
    height: int


@dataclass
class PerspectiveCamera(Camera):
    """A camera that looks from ``position`` at ``target`` (no counterpart in the reference, whose
    camera always looks along +z through a screen fixed at z=0). ``position``, ``width`` and
    ``height`` mean what they mean for ``Camera``, so the scene packer and the shader's view vector
    (``scene.camera.position``) read them unchanged.

    ``up``: the direction that appears upwards in the frame (a Vector3D or three numbers; it need not
    be perpendicular to the view, only not parallel to it). ``fov``: the vertical field of view in
    degrees, 0 < fov < 180. ``lens_radius`` >= 0: the radius of a thin lens (0: a pinhole, everything
    in focus); with a lens each of a pixel's samples leaves through another point of it, so it needs
    a renderer with ``samples >= 2``. ``focus_distance``: the distance along the view direction of
    the plane that stays sharp, > 0; None: the target's distance. Validated and reduced to the
    kernel's camera record by ``python_ray_tracer_amd.camera``."""

    target: Vector3D
    up: object = (0.0, 1.0, 0.0)
    fov: float = 40.0
    lens_radius: float = 0.0
    focus_distance: float | None = None


@dataclass
class PointLight:
    """Reference ``domain.py:26-30``. Only ``scene.lights[0]`` is ever used as the point light
    (``shader.py:75``), unless the list holds a ``ColoredPointLight``."""

    position: Vector3D


@dataclass
class ColoredPointLight(PointLight):
    """A point light with a strength and a colour (no counterpart in the reference: ``domain.py`` says
    "class PointLight:  # TODO: add intensity", ``main.py`` "TODO: use multiple lights"). One of them in
    ``scene.lights`` makes the scene a multi-light scene: every point light of the list then lights
    it, in list order, each weighted per channel by ``intensity * color`` (a plain ``PointLight``
    counts as intensity 1 and white). ``color``: an ``RGBColor`` or three numbers. Validated and
    reduced to the kernel's table by ``python_ray_tracer_amd.lights``."""

    intensity: float = 1.0
    color: object = (1.0, 1.0, 1.0)


class EnvironmentLight:
    """An environment map: what a ray that meets no shape sees (no counterpart in the reference, whose
    ``raytrace_scene`` adds nothing on a miss, base.py:100-121; its render settings carry a "background"
    image that nothing reads). One of them in ``scene.lights`` makes the scene an environment scene:
    camera rays, reflected rays and rays that leave a glass ball then return the image's colour in
    their direction where they meet nothing. It lights no surface (the dome light and the shadows do
    not see it) and has no ``position``, so it cannot be ``lights[0]``.

    ``image``: an equirectangular picture, columns by longitude about +y and row 0 at the zenith: a
    path (opened with PIL, ``convert("RGB")``, ``/ 255.0``), an (H, W, 3) uint8 array (``/ 255.0``) or an
    (H, W, 3) float array, whose values may exceed 1 (an HDR sky). At most 2^23 texels, none negative
    or not finite (ValueError). The light keeps ``texels``, a read-only float32 copy [H, W, 4] (RGB and a
    zero word: one 128-bit load per tap on the device), and ``digest``, its content hash, computed
    once. ``intensity`` and ``color`` (an ``RGBColor`` or three numbers) scale the image per channel;
    ``rotation`` turns it about +y, in degrees. Validated and reduced to the kernel's arguments by
    ``python_ray_tracer_amd.environment``."""

    def __init__(self, image, intensity: float = 1.0, color=(1.0, 1.0, 1.0), rotation: float = 0.0) -> None:
        from python_ray_tracer_amd.environment import image_texels

        self.texels, self.digest = image_texels(image)
        self.intensity = intensity
        self.color = color
        self.rotation = rotation

    def __repr__(self) -> str:
        h, w = self.texels.shape[:2]
        return (f"EnvironmentLight(<{w} x {h} image {self.digest[:8]}>, intensity={self.intensity!r}, "
                f"color={self.color!r}, rotation={self.rotation!r})")


@dataclass
class DomeLight:
    """Sky light (reference ``domain.py:33-40``); every DomeLight in ``scene.lights`` adds its
    intensity, the colour of the last one wins (``shader.py:234-244``)."""

    intensity: float
    color: RGBColor


class Shape(ABC):
    """Reference ``domain.py:43-50``."""

    @abstractmethod
    def intersect(self, ray_origin, normalized_ray_direction):
        pass

    @abstractmethod
    def diffusecolor(self, intersection_point):
        pass


class TriangleMesh(Shape):
    """Triangles with one shader (no counterpart in the reference, whose only shape is the sphere:
    ``Shape`` is an ABC with one subclass). One of them in ``scene.shapes`` makes the scene a mesh scene
    (``python_ray_tracer_amd.meshes``, ``rtx_trace_mesh``).

    ``vertices``: float [V, 3]. ``faces``: int [F, 3], indices into ``vertices``. ``normals``: float
    [V, 3] for smooth shading (the shading normal is interpolated over a face), None for flat.
    ``uvs``: texture coordinates per corner, float [F, 3, 2]: ``(s, t)`` at ``v0, v1, v2`` of each face
    (OBJ's ``vt``: t = 0 is the image's bottom row; a closed surface can have a seam without split
    vertices), or float [V, 2] per vertex, expanded to ``uvs[faces]``; None for a mesh without any.
    ``shader``: the material of every face, a ``HipShader`` (a plain or a checker texture, or an
    ``ImageTexture`` on a mesh with ``uvs``, looked up bilinearly with repeat: include/rtx_hip.h,
    DESIGN.md §18; no transmission). The arrays are kept as float64 / int64 copies; they are validated
    where a table is built from them (``meshes.mesh_table``)."""

    def __init__(self, vertices, faces, shader, normals=None, uvs=None) -> None:
        import numpy as np

        self.vertices = np.array(vertices, dtype=np.float64)
        self.faces = np.array(faces, dtype=np.int64)
        self.shader = shader
        self.normals = None if normals is None else np.array(normals, dtype=np.float64)
        self.uvs = None if uvs is None else np.array(uvs, dtype=np.float64)
        if (self.uvs is not None and self.uvs.ndim == 2 and self.uvs.shape == (len(self.vertices), 2)
                and self.faces.ndim == 2 and self.faces.size and 0 <= self.faces.min()
                and self.faces.max() < len(self.vertices)):
            self.uvs = self.uvs[self.faces]  # per vertex -> per corner

    def intersect(self, ray_origin, normalized_ray_direction):
        """The distance to the nearest triangle of this mesh (the two-sided Möller–Trumbore test of
        include/rtx_hip.h, in NumPy, every face tried): float64, FARAWAY (1e39) where the ray misses."""
        from python_ray_tracer_amd import meshes

        return meshes.intersect_mesh(self, ray_origin, normalized_ray_direction)

    def diffusecolor(self, intersection_point):
        return self.shader.diffuse_color.get_color(intersection_point)

    def placed(self, scale=1.0, translation=(0.0, 0.0, 0.0)) -> TriangleMesh:
        """A copy with every vertex at ``vertex * scale + translation`` (``scale`` a number)."""
        import numpy as np

        v = self.vertices * float(scale) + np.asarray(translation, dtype=np.float64).reshape(1, 3)
        return TriangleMesh(v, self.faces, self.shader, self.normals, self.uvs)

    def __repr__(self) -> str:
        return (f"TriangleMesh(<{len(self.vertices)} vertices, {len(self.faces)} faces, "
                f"{'smooth' if self.normals is not None else 'flat'}{', uvs' if self.uvs is not None else ''}>)")


@dataclass
class Scene3D:
    """Reference ``domain.py:53-59``."""

    shapes: list
    lights: list
    camera: Camera
