"""Scene specifications used by the benchmarks, the tests and the golden-fixture generator.

A *scene spec* is a plain JSON-able dict, so the same scene can be instantiated with this
package's classes (``build_scene``), with the reference's classes (the fixture generator under
``tests/golden/``) and by the CPU oracle (``oracle/numpy_oracle.py``) without any of them
importing each other.

Scenes:

* ``main_spec``   — ``/root/reference/main.py:13-51`` verbatim (the scene that produced the
  committed ``render.png``). Python ints are kept as ints, exactly as main.py writes them.
* ``readme_spec`` — the README scene (``/root/reference/README.md:50-84``) translated to today's
  API: every shader ``NumpyShader(0.8, 1.0, 0.5, 0.05, 1.0, tex)``; ground ``TextureChecker``.
  This is BASELINE.json configs[0] / configs[1].
* ``random_spec`` — the seeded generator of SURVEY.md §8d (configs C3/C4/C5).
* ``orbit_position`` — C5's camera orbit.

Spec layout::

    {"spheres": [{"center": [x, y, z], "radius": r,
                  "shader": {"reflection_gain": .., "specular_gain": .., "specular_roughness": ..,
                             "iridescence_gain": .., "diffuse_gain": ..,
                             "texture": {"kind": "const" | "checker", "color": [r, g, b]}}}],
                  (or {"kind": "image", "texels": (H, W, 3) float colours} — ImageTexture)
                  (a shader may also carry "transmission_gain" and "specular_ior": glass, glass_spec)
     "lights": [{"kind": "point", "position": [x, y, z]},
                (a point entry may also carry "intensity" and/or "color": [r, g, b]; either makes it a
                 domain.ColoredPointLight and the scene a multi-light scene, lights_spec)
                {"kind": "dome", "intensity": i, "color": [r, g, b]},
                {"kind": "environment", "texels": (H, W, 3) colours, and, all optional, "intensity": i,
                 "color": [r, g, b], "rotation": degrees}: a domain.EnvironmentLight, env_spec],
     "meshes": [...] (optional: domain.TriangleMesh shapes after the spheres, a mesh scene, mesh_spec; each
                {"kind": "quad", "corners": four points} | {"kind": "box", "lo": .., "hi": ..} |
                {"kind": "icosphere", "level": n} | {"kind": "torus", "R": .., "r": .., "nu": .., "nv": ..} |
                {"kind": "triangles", "vertices": [V, 3], "faces": [F, 3], and optionally "normals": [V, 3]},
                with "shader" as a sphere's and, all optional, "smooth": bool, "scale": s,
                "translation": [x, y, z]; texture coordinates, for an image texture on the mesh
                (textured_mesh_spec): "uvs": [F, 3, 2] or [V, 2] for kind "triangles", "uv": true for
                "quad", "box" and "torus")
     "camera": {"position": [x, y, z], "width": W, "height": H}}
                (with "target": [x, y, z] a domain.PerspectiveCamera; then also, all optional,
                 "up": [x, y, z], "fov": degrees, "lens_radius": r, "focus_distance": d)
"""

from __future__ import annotations

import copy
import math

import numpy as np


def _shader(reflection_gain, specular_gain, specular_roughness, iridescence_gain, diffuse_gain, texture):
    return {
        "reflection_gain": reflection_gain,
        "specular_gain": specular_gain,
        "specular_roughness": specular_roughness,
        "iridescence_gain": iridescence_gain,
        "diffuse_gain": diffuse_gain,
        "texture": texture,
    }


def _const(r, g, b):
    return {"kind": "const", "color": [r, g, b]}


def _checker():
    # TextureChecker's own colour is ignored by get_color (shader.py:29-32)
    return {"kind": "checker", "color": [1, 1, 1]}


def main_spec(width: int = 960, height: int = 540) -> dict:
    """``/root/reference/main.py:13-51``; default size is main.py's ``int(1920/2) x int(1080/2)``."""
    return {
        "spheres": [
            {"center": [0.55, 0.5, 3], "radius": 1.0,
             "shader": _shader(0.0, 0, 0.01, 0, 0.0, _const(1, 1, 1))},
            {"center": [-0.45, 0.1, 1], "radius": 0.4,
             "shader": _shader(0, 1, 0.1, 0.0, 0.0, _const(1, 0, 0))},
            {"center": [0, -99999.5, 0], "radius": 99999,
             "shader": _shader(0.0, 0.1, 0.5, 0.0, 1.0, _checker())},
        ],
        "lights": [
            {"kind": "point", "position": [-2, 1, 2]},
            {"kind": "dome", "intensity": 0.1, "color": [1, 1, 1]},
        ],
        "camera": {"position": [0, 0.2, -2], "width": int(width), "height": int(height)},
    }


def readme_spec(width: int = 1920, height: int = 1080) -> dict:
    """README scene, translated."""
    gains = (0.8, 1.0, 0.5, 0.05, 1.0)
    return {
        "spheres": [
            {"center": [0.55, 0.5, 3], "radius": 1.0, "shader": _shader(*gains, _const(1, 0, 1))},
            {"center": [-0.45, 0.1, 1], "radius": 0.4, "shader": _shader(*gains, _const(0.5, 0.5, 0.5))},
            {"center": [0, -99999.5, 0], "radius": 99999, "shader": _shader(*gains, _checker())},
        ],
        "lights": [
            {"kind": "point", "position": [5, 10, -10]},
            {"kind": "dome", "intensity": 0.1, "color": [1, 1, 1]},
        ],
        "camera": {"position": [0, 0.2, -2], "width": int(width), "height": int(height)},
    }


def glass_spec(width: int = 1920, height: int = 1080) -> dict:
    """The README scene with the small sphere made of glass (``transmission_gain`` 0.9, ``diffuse_gain``
    0.1) and the large one half glass (``transmission_gain`` 0.5): the transmission frame of
    tools/glass_bench.py and the README. Both keep the default index of refraction, 1.5."""
    spec = readme_spec(width, height)
    spec["spheres"][1]["shader"].update(transmission_gain=0.9, diffuse_gain=0.1)
    spec["spheres"][0]["shader"].update(transmission_gain=0.5)
    return spec


def lights_spec(width: int = 1920, height: int = 1080) -> dict:
    """The README scene under three point lights: its own light stays ``lights[0]`` (a plain point light:
    intensity 1, white), a warm fill light stands on the other side, behind the spheres, and a blue one
    above them. The
    multi-light frame of tools/lights_bench.py, the README and the tests (``rtx_trace_lights``)."""
    spec = readme_spec(width, height)
    spec["lights"] += [
        {"kind": "point", "position": [-1.33, 8.16, 7.23], "intensity": 0.6, "color": [1.0, 0.7, 0.4]},
        {"kind": "point", "position": [0.18, 9.4, 3.89], "intensity": 0.4, "color": [0.4, 0.6, 1.0]},
    ]
    return spec


def mesh_spec(width: int = 1920, height: int = 1080, level: int = 2) -> dict:
    """The README scene with its ground sphere replaced by a checkered quad, and a smooth icosphere
    (``level`` subdivisions: 20 * 4**level triangles) and a torus added: the mesh frame of
    tools/mesh_bench.py, the README and the tests (``rtx_trace_mesh``)."""
    spec = readme_spec(width, height)
    ground = spec["spheres"].pop(2)
    gains = (0.8, 1.0, 0.5, 0.05, 1.0)
    spec["meshes"] = [
        {"kind": "quad", "corners": [[-40, -0.5, -10], [-40, -0.5, 60], [40, -0.5, 60], [40, -0.5, -10]],
         "shader": ground["shader"]},
        {"kind": "icosphere", "level": int(level), "smooth": True, "scale": 0.45, "translation": [-1.5, -0.05, 1.75],
         "shader": _shader(*gains, _const(0.2, 0.6, 1.0))},
        {"kind": "torus", "R": 0.5, "r": 0.17, "nu": 32, "nv": 16, "smooth": True, "translation": [0.7, -0.33, 0.9],
         "shader": _shader(*gains, _const(1.0, 0.6, 0.1))},
    ]
    return spec


def mesh_of(m: dict, shader=None):
    """The ``TriangleMesh`` of one entry of a spec's "meshes", placed by its "scale" and "translation"."""
    from python_ray_tracer_amd import meshes

    kind, smooth, uv = m["kind"], bool(m.get("smooth", False)), bool(m.get("uv", False))
    if kind == "quad":
        mesh = meshes.quad(m["corners"], shader, uv)
    elif kind == "box":
        mesh = meshes.box(m["lo"], m["hi"], shader, uv)
    elif kind == "icosphere":
        mesh = meshes.icosphere(m["level"], shader, smooth)
    elif kind == "torus":
        mesh = meshes.torus(m["R"], m["r"], m["nu"], m["nv"], shader, smooth, uv)
    elif kind == "triangles":
        mesh = meshes.TriangleMesh(m["vertices"], m["faces"], shader, m.get("normals"), m.get("uvs"))
    else:
        raise ValueError(f"unknown mesh kind {kind!r}")
    if smooth and mesh.normals is None:
        mesh.normals = meshes.vertex_normals(mesh.vertices, mesh.faces)
    return mesh.placed(m.get("scale", 1.0), m.get("translation", (0.0, 0.0, 0.0)))


def mesh_arrays(m: dict):
    """(vertices [V, 3], faces [F, 3], normals [V, 3] or None) of one entry of a spec's "meshes", placed
    by its "scale" and "translation"."""
    mesh = mesh_of(m)
    return mesh.vertices, mesh.faces, mesh.normals


def uv_grid_texels(width: int = 64, height: int = 64) -> np.ndarray:
    """A procedural texture as a float64 image (height, width, 3), so that nobody needs a file: red grows
    with the column and green with the row from the bottom (so s and t can be read off a render), over a
    grid of 8 x 8 cells whose every other cell is darker and whose blue tells the two kinds apart."""
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError(f"uv_grid_texels: width and height must be >= 1, got {width} x {height}")
    s = ((np.arange(w) + 0.5) / w).reshape(1, w)
    t = (1.0 - (np.arange(h) + 0.5) / h).reshape(h, 1)  # row 0 is the top of the image: t near 1
    dark = ((np.floor(s * 8.0) + np.floor(t * 8.0)) % 2.0) == 1.0
    shade = np.where(dark, 0.45, 1.0)
    return np.stack([(0.15 + 0.85 * s) * shade, (0.15 + 0.85 * t) * shade, np.where(dark, 0.6, 0.2)], axis=-1)


def textured_mesh_spec(width: int = 1920, height: int = 1080, level: int = 2, texels=None) -> dict:
    """``mesh_spec`` with an image (``texels``, default ``uv_grid_texels()``) on its ground quad and on its
    torus, both with texture coordinates ("uv": true): the textured frame of tools/meshuv_bench.py, the
    README and the tests (``rtx_trace_mesh_uv``). The quad's 0..1 spans its 80 x 70 units once."""
    spec = mesh_spec(width, height, level)
    image = {"kind": "image", "texels": uv_grid_texels() if texels is None else texels}
    for i in (0, 2):
        spec["meshes"][i]["uv"] = True
        spec["meshes"][i]["shader"] = {**spec["meshes"][i]["shader"], "texture": image}
    return spec


def sky_texels(width: int = 256, height: int = 128) -> np.ndarray:
    """A procedural sky as an equirectangular float64 image (height, width, 3), so that nobody needs a
    file: above the horizon a gradient from a pale horizon to a blue zenith, below it a darker ground,
    and a sun disk of 5 degrees radius brighter than 1 (an HDR value) in the direction of the README
    scene's light, (5, 10, -10). Row j, column i hold the colour of the direction at the texel's
    centre: v = (j + 0.5) / height from the zenith down, u = (i + 0.5) / width about +y."""
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError(f"sky_texels: width and height must be >= 1, got {width} x {height}")
    el = (0.5 - (np.arange(h) + 0.5) / h) * math.pi  # elevation of a row's centre
    az = ((np.arange(w) + 0.5) / w - 0.5) * (2.0 * math.pi)  # atan2(z, x) of a column's centre
    up = np.clip(np.sin(el), 0.0, 1.0)[:, None, None]
    horizon, zenith, ground = np.array([0.85, 0.9, 1.0]), np.array([0.15, 0.35, 0.9]), np.array([0.2, 0.17, 0.14])
    sky = horizon + (zenith - horizon) * np.sqrt(up)
    img = np.where((el > 0.0)[:, None, None], sky, ground * (1.0 - 0.5 * np.clip(-np.sin(el), 0.0, 1.0)[:, None, None]))
    img = np.broadcast_to(img, (h, w, 3)).copy()
    sun = np.array([5.0, 10.0, -10.0]) / 15.0
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (h, w)),
                  np.cos(el)[:, None] * np.sin(az)[None, :]], axis=-1)
    img[(d @ sun) > math.cos(math.radians(5.0))] = [16.0, 14.0, 10.0]
    return img


def env_spec(width: int = 1920, height: int = 1080, env_width: int = 256, env_height: int = 128) -> dict:
    """The README scene under the procedural sky (``sky_texels(env_width, env_height)``): every ray that
    meets no sphere, reflected ones included, sees the sky. The environment frame of tools/env_bench.py,
    the README and the tests (``rtx_trace_lights_env``)."""
    spec = readme_spec(width, height)
    spec["lights"].append({"kind": "environment", "texels": sky_texels(env_width, env_height)})
    return spec


def random_spec(n_spheres: int, seed: int = 0, width: int = 3840, height: int = 2160) -> dict:
    """Seeded random scene of SURVEY.md §8d: PCG64 draws per sphere, in this order,
    r~U(0.1,0.5), cx~U(-4,4), cz~U(0.5,14), colour~U(0,1)^3, then the shader gains
    reflection~U(0,1), specular~U(0,1), roughness~U(0.05,0.9), iridescence~U(0,0.1),
    diffuse~U(0.3,1). Centre (cx, r-0.5, cz) rests the sphere on the ground. A checker ground
    sphere is appended; lights [PointLight(-2,4,-1), DomeLight(0.1, white)]; camera (0,0.2,-2)."""
    rng = np.random.default_rng(seed)
    spheres = []
    for _ in range(int(n_spheres)):
        r = float(rng.uniform(0.1, 0.5))
        cx = float(rng.uniform(-4, 4))
        cz = float(rng.uniform(0.5, 14))
        col = [float(v) for v in rng.uniform(0, 1, 3)]
        refl = float(rng.uniform(0, 1))
        spec = float(rng.uniform(0, 1))
        rough = float(rng.uniform(0.05, 0.9))
        irid = float(rng.uniform(0, 0.1))
        diff = float(rng.uniform(0.3, 1))
        spheres.append({"center": [cx, r - 0.5, cz], "radius": r,
                        "shader": _shader(refl, spec, rough, irid, diff, _const(*col))})
    spheres.append({"center": [0, -99999.5, 0], "radius": 99999,
                    "shader": _shader(0.0, 0.1, 0.5, 0.0, 1.0, _checker())})
    return {
        "spheres": spheres,
        "lights": [
            {"kind": "point", "position": [-2, 4, -1]},
            {"kind": "dome", "intensity": 0.1, "color": [1, 1, 1]},
        ],
        "camera": {"position": [0, 0.2, -2], "width": int(width), "height": int(height)},
    }


def orbit_position(frame: int, n_frames: int = 256) -> list:
    """C5 camera orbit: frame k at (sin θ, 0.2, -2 - cos θ), θ = 2πk/n (z stays < 0 because the
    reference screen is fixed at z=0, ``base.py:131-141``)."""
    theta = 2.0 * math.pi * frame / n_frames
    return [math.sin(theta), 0.2, -2.0 - math.cos(theta)]


def path_position(spec: dict, frame: int, n_frames: int = 256) -> list:
    """Frame k of the camera path through a config's own camera (the ``bench.py --gpus N``
    headline: rank r renders frame r, so frame 0 — rank 0, and the N = 1 line — is the config's
    frame itself). A circle of radius 1 in the horizontal plane, frame 0 at the camera and the
    centre one unit behind it: (cx + sin θ, cy, cz - 1 + cos θ), θ = 2πk/n. z stays ≤ cz, so a
    config camera in front of the reference's fixed screen (z < 0, ``base.py:131-141``) stays there."""
    cx, cy, cz = (float(v) for v in spec["camera"]["position"])
    theta = 2.0 * math.pi * frame / n_frames
    return [cx + math.sin(theta), cy, (cz - 1.0) + math.cos(theta)]


def rank_frame_spec(spec: dict, rank: int, n_frames: int = 256) -> dict:
    """The frame a rank of the weak-scaling headline renders: the config's own spec at rank 0
    (unchanged, so the N = 1 line is the single-GPU line), frame ``rank`` of ``path_position``
    elsewhere — every rank a distinct frame of one camera path, as ``render_image_pipeline`` renders
    one frame per call (``application.py:43-52``)."""
    if rank % n_frames == 0:
        return spec
    return with_camera(spec, path_position(spec, rank, n_frames))


def with_camera(spec: dict, position=None, width=None, height=None, target=None, up=None, fov=None,
                lens_radius=None, focus_distance=None) -> dict:
    """Copy of ``spec`` with camera fields replaced. ``target`` (and ``up``, ``fov``, ``lens_radius``,
    ``focus_distance``) make it a perspective camera's spec (``build_scene``)."""
    out = copy.deepcopy(spec)
    if position is not None:
        out["camera"]["position"] = list(position)
    if width is not None:
        out["camera"]["width"] = int(width)
    if height is not None:
        out["camera"]["height"] = int(height)
    if target is not None:
        out["camera"]["target"] = list(target)
    if up is not None:
        out["camera"]["up"] = list(up)
    for key, value in (("fov", fov), ("lens_radius", lens_radius), ("focus_distance", focus_distance)):
        if value is not None:
            out["camera"][key] = value
    return out


CONFIGS = {
    # BASELINE.json configs, by index
    "C1": lambda: (readme_spec(960, 540), 3),
    "C2": lambda: (readme_spec(1920, 1080), 3),
    "C2main": lambda: (main_spec(1920, 1080), 3),
    "C3": lambda: (random_spec(16, 0, 3840, 2160), 4),
    "C4": lambda: (random_spec(64, 0, 7680, 4320), 5),
    "C5": lambda: (random_spec(16, 0, 1920, 1080), 3),
}


def build_scene(spec: dict):
    """Instantiate ``spec`` with this package's HIP-backend classes."""
    from python_ray_tracer_amd.domain import Camera, ColoredPointLight, DomeLight, EnvironmentLight, PointLight, Scene3D
    from python_ray_tracer_amd.infrastructure.hip import (
        HipRGBColor,
        HipShader,
        HipSphere,
        HipVector3D,
        ImageTexture,
        Texture,
        TextureChecker,
    )

    def shader_of(sh):
        tex = sh["texture"]
        if tex["kind"] == "checker":
            texture = TextureChecker()
        elif tex["kind"] == "image":
            texture = ImageTexture(np.asarray(tex["texels"], dtype=np.float64))
        else:
            texture = Texture(HipRGBColor(*tex["color"]))
        shader = HipShader(sh["reflection_gain"], sh["specular_gain"], sh["specular_roughness"],
                           sh["iridescence_gain"], sh["diffuse_gain"], texture)
        for key in ("transmission_gain", "specular_ior"):  # optional: glass (glass_spec)
            if key in sh:
                setattr(shader, key, sh[key])
        return shader

    shapes = [HipSphere(HipVector3D(*s["center"]), s["radius"], shader_of(s["shader"])) for s in spec["spheres"]]
    for m in spec.get("meshes", ()):  # optional: a mesh scene (mesh_spec)
        shapes.append(mesh_of(m, shader_of(m["shader"])))
    lights = []
    for li in spec["lights"]:
        if li["kind"] == "point":
            if "intensity" in li or "color" in li:  # optional: a multi-light scene (lights_spec)
                lights.append(ColoredPointLight(HipVector3D(*li["position"]), li.get("intensity", 1.0),
                                                HipRGBColor(*li.get("color", (1.0, 1.0, 1.0)))))
            else:
                lights.append(PointLight(HipVector3D(*li["position"])))
        elif li["kind"] == "environment":  # an environment scene (env_spec)
            lights.append(EnvironmentLight(li["texels"], li.get("intensity", 1.0),
                                           HipRGBColor(*li.get("color", (1.0, 1.0, 1.0))), li.get("rotation", 0.0)))
        else:
            lights.append(DomeLight(li["intensity"], HipRGBColor(*li["color"])))
    cam = spec["camera"]
    if "target" in cam:  # a camera that looks at a point (domain.PerspectiveCamera); the other keys are optional
        from python_ray_tracer_amd.domain import PerspectiveCamera

        extra = {k: cam[k] for k in ("fov", "lens_radius", "focus_distance") if k in cam}
        if "up" in cam:
            extra["up"] = HipVector3D(*cam["up"])
        camera = PerspectiveCamera(HipVector3D(*cam["position"]), cam["width"], cam["height"],
                                   HipVector3D(*cam["target"]), **extra)
    else:
        camera = Camera(HipVector3D(*cam["position"]), cam["width"], cam["height"])
    return Scene3D(shapes, lights, camera)
