"""The scenes of the path-truth tests (tests/path_ref.py): a few triangles each, written as Mitsuba XML +
OBJ and loaded through the product's loaders; what no loader sets (multiscattering, the lens' blades, a
point light, the environment cube, opacities, feature bits) is set through the scene API.

Every part is its own OBJ in world coordinates under an identity transform (no instance scaling: shading
QUIRK Q1), flat-shaded (the shading normal is the face's), with texcoords (0,0) (1,0) (1,1) (0,1) on quads,
and lies at least 1e-2 from every other part. Lamps are well above the 1e-6 area threshold.

Two shipped material states have a scene of their own: `coat` -- smooth plastic, the one vertex kind at which one
selection number chooses between a continuous lobe and a delta lobe -- and `frost` -- a rough dielectric with
multiscattering, whose sampler draws from another density than the pdf it reports (BSDF QUIRK Q1). A roughness
texture has none: no loader and no scene call can set it.

SCENES[name]: the B the scene runs at, the states of LIGHT_VISIBLE, the reference's path count, the
device's image count. The path counts make the reference's standard error at most the device side's on
every statistic (tests/test_gpu_path_ref.py asserts it; DESIGN.md section 3 has the measured ratios)."""
from pathlib import Path

import numpy as np

from directcomputeraytracing_amd.scenes import _sensor, _xml, env_cube, mitsuba_matrix

SIZE = 64
SEED = 20240607
ANYHIT = 0x10
LIGHT_VISIBLE = 0x04

SCENES = {
    "bleed": {"bounces": (0, 1, 3), "visible": (True, False), "paths": 12 << 20, "images": 16},
    "mixed": {"bounces": (0, 1, 3), "visible": (True,), "paths": 1 << 20, "images": 16},
    "glass": {"bounces": (1, 3, 6), "visible": (True,), "paths": 1 << 20, "images": 16},
    "sheet": {"bounces": (0, 1, 3), "visible": (True,), "paths": 1 << 20, "images": 16},
    "veil": {"bounces": (0, 1, 3), "visible": (True,), "paths": 4 << 20, "images": 16},
    "coat": {"bounces": (0, 1, 3), "visible": (True, False), "paths": 1 << 20, "images": 16},
    "frost": {"bounces": (1, 3, 6), "visible": (True,), "paths": 1 << 20, "images": 16},
}


def _write_faces(path, faces):
    """Flat-shaded polygons [(corners counter-clockwise about the normal, normal)] as an OBJ, fanned."""
    lines, n = ["# path-truth part"], 0
    for corners, normal in faces:
        uv = [(0, 0), (1, 0), (1, 1), (0, 1)] if len(corners) == 4 else [(0, 0), (1, 0), (0, 1)]
        for (x, y, z), (s, t) in zip(corners, uv):
            lines += [f"v {x:.6f} {y:.6f} {z:.6f}", f"vt {s} {t}", f"vn {normal[0]:.6f} {normal[1]:.6f} {normal[2]:.6f}"]
        idx = [f"{n + k + 1}/{n + k + 1}/{n + k + 1}" for k in range(len(corners))]
        for k in range(1, len(corners) - 1):
            lines.append(f"f {idx[0]} {idx[k]} {idx[k + 1]}")
        n += len(corners)
    Path(path).write_text("\n".join(lines) + "\n")


def _quad(centre, ex, ey):
    """The quad centre +- ex +- ey, counter-clockwise about ex x ey."""
    c, ex, ey = (np.asarray(a, np.float64) for a in (centre, ex, ey))
    n = np.cross(ex, ey)
    return [tuple(c - ex - ey), tuple(c + ex - ey), tuple(c + ex + ey), tuple(c - ex + ey)], tuple(n / np.linalg.norm(n))


def _box(lo, hi):
    """The six outward faces of an axis-aligned box."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    out = []
    for a in range(3):
        for sgn in (1.0, -1.0):
            n = np.zeros(3); n[a] = sgn
            ex = np.zeros(3); ex[(a + 1) % 3] = h[(a + 1) % 3]
            ey = np.zeros(3); ey[(a + 2) % 3] = h[(a + 2) % 3] * sgn
            out.append(_quad(c + n * h[a], ex, ey))
    return out


def _shape(name, bsdf="", emitter=None):
    e = f'<emitter type="area"><rgb name="radiance" value="{emitter}"/></emitter>' if emitter else ""
    return (f'  <shape type="obj" id="{name}"><string name="filename" value="{name}.obj"/>{bsdf}{e}'
            f'<transform name="to_world"><matrix value="{mitsuba_matrix()}"/></transform></shape>\n')


def _diffuse(c, two_sided=False):
    b = f'<bsdf type="diffuse"><rgb name="reflectance" value="{c}"/></bsdf>'
    return f'<bsdf type="twosided">{b}</bsdf>' if two_sided else b


def _pgm(path, img):
    img = np.asarray(img, np.uint8)
    Path(path).write_bytes(f"P5 {img.shape[1]} {img.shape[0]} 255\n".encode() + img.tobytes())


def _ppm(path, img):
    img = np.asarray(img, np.uint8)
    Path(path).write_bytes(f"P6 {img.shape[1]} {img.shape[0]} 255\n".encode() + img.tobytes())


def _integrator(b):
    return f'  <integrator type="path"><integer name="max_depth" value="{b}"/></integrator>\n'


def _camera(pos, yaw=0.0, pitch=0.0, fov=80):
    return _sensor("perspective", SIZE, SIZE, mitsuba_matrix(pos, yaw=yaw, pitch=pitch), f'    <float name="fov" value="{fov}"/>\n',
                   rfilter='<rfilter type="box"/>')


# ---- bleed (and the box veil stands in) ------------------------------------------------------------------
def _bleed_parts(d):
    """The open box x, z in [-1, 1], y in [0, 2] (no front wall), a lamp over a quarter of the ceiling."""
    rng = np.random.default_rng(5)
    _ppm(d / "back.ppm", rng.integers(30, 256, (4, 5, 3)))
    parts = {
        "floor": (_quad((0, 0, 0), (1, 0, 0), (0, 0, -1)), '<bsdf type="roughplastic"><rgb name="diffuse_reflectance" value="0.8, 0.7, 0.1"/>'
                  '<float name="alpha" value="0.3"/><float name="int_ior" value="1.5"/></bsdf>'),
        "ceiling": (_quad((0, 2, 0), (1, 0, 0), (0, 0, 1)), _diffuse("0.7, 0.1, 0.7")),
        "back": (_quad((0, 1, 1), (-1, 0, 0), (0, 1, 0)), '<bsdf type="diffuse"><texture name="reflectance" type="bitmap">'
                 '<string name="filename" value="back.ppm"/></texture></bsdf>'),
        "left": (_quad((-1, 1, 0), (0, 0, -1), (0, 1, 0)), _diffuse("0.85, 0.1, 0.1")),
        "right": (_quad((1, 1, 0), (0, 0, 1), (0, 1, 0)), _diffuse("0.1, 0.8, 0.15")),
    }
    body = ""
    for name, (face, bsdf) in parts.items():
        _write_faces(d / f"{name}.obj", [face])
        body += _shape(name, bsdf)
    _write_faces(d / "lamp.obj", [_quad((-0.3, 1.9, 0.2), (0.5, 0, 0), (0, 0, 0.5))])
    return body + _shape("lamp", emitter="6, 5, 4")


def _load(scene_cls, path):
    s = scene_cls((SIZE, SIZE))
    s.load_from_file(path)
    return s


def load(name, directory):
    """The scene `name`, loaded; max_bounce is the scene's largest B (set_max_bounce selects another)."""
    from directcomputeraytracing_amd import Scene
    d = Path(directory) / name
    d.mkdir(parents=True, exist_ok=True)
    return globals()["_" + name](Scene, d)


def _bleed(Scene, d):
    (d / "bleed.xml").write_text(_xml(_integrator(3) + _camera((0.1, 0.9, -0.95), yaw=-6, pitch=-4, fov=90) + _bleed_parts(d)))
    s = _load(Scene, d / "bleed.xml")
    assert len(s.enable_multiscattering()) == 1          # the floor's rough plastic
    return s


def _veil(Scene, d):
    """The bleed box with a veil of constant opacity 0.37 between the camera and the box's inside, a veil with
    an opacity bitmap between the floor and the lamp, and a fully opaque `mask` quad (its instance carries the
    OPAQUE flag, like the walls') beside it."""
    img = np.clip(np.add.outer(np.arange(4) * 50, np.arange(4) * 17) + 20, 0, 255)
    _pgm(d / "veil.pgm", img)
    veils = {
        "front": (_quad((0, 1, -0.5), (-0.7, 0, 0), (0, 0.7, 0)), '<bsdf type="mask"><float name="opacity" value="0.37"/>' + _diffuse("0.2, 0.3, 0.8", True) + "</bsdf>"),
        "under": (_quad((-0.3, 1.4, 0.2), (0.6, 0, 0), (0, 0, 0.6)), '<bsdf type="mask"><texture name="opacity" type="bitmap"><string name="filename" value="veil.pgm"/>'
                  "</texture>" + _diffuse("0.6, 0.6, 0.2", True) + "</bsdf>"),
        "solid": (_quad((0.6, 0.5, 0.3), (0.25, 0, 0), (0, 0, 0.25)), '<bsdf type="mask"><float name="opacity" value="1"/>' + _diffuse("0.5, 0.5, 0.5", True) + "</bsdf>"),
    }
    body = _bleed_parts(d)
    for name, (face, bsdf) in veils.items():
        _write_faces(d / f"{name}.obj", [face])
        body += _shape(name, bsdf)
    (d / "veil.xml").write_text(_xml(_integrator(3) + _camera((0.1, 0.9, -0.95), yaw=-6, pitch=-4, fov=90) + body))
    s = _load(Scene, d / "veil.xml")
    s.enable_multiscattering()
    s.features = s.features | ANYHIT
    return s


def _mixed(Scene, d):
    parts = {
        "matte": (_quad((-1, 0, 0), (1, 0, 0), (0, 0, -2)), _diffuse("0.6, 0.5, 0.4")),
        "metal": (_quad((1, 0, 0), (1, 0, 0), (0, 0, -2)), '<bsdf type="roughconductor"><rgb name="eta" value="0.2, 0.9, 1.1"/>'
                  '<rgb name="k" value="3.9, 2.4, 2.2"/><float name="alpha" value="0.3"/></bsdf>'),
        "blocker": (_quad((0.2, 0.6, 0.1), (0.5, 0, 0), (0, 0, -0.4)), _diffuse("0.3, 0.6, 0.7", True)),
    }
    body = ""
    for name, (face, bsdf) in parts.items():
        _write_faces(d / f"{name}.obj", [face])
        body += _shape(name, bsdf)
    _write_faces(d / "lamp.obj", [_quad((-0.6, 1.8, 0.4), (0.4, 0, 0), (0, 0, 0.4))])
    body += _shape("lamp", emitter="5, 6, 7")
    body += ('  <emitter type="constant"><rgb name="radiance" value="0.3, 0.35, 0.5"/></emitter>\n'
             '  <emitter type="directional"><vector name="direction" value="-0.3, -0.8, 0.5"/><rgb name="irradiance" value="2, 1.9, 1.7"/></emitter>\n')
    (d / "mixed.xml").write_text(_xml(_integrator(3) + _camera((0, 1.6, -3.0), pitch=28, fov=60) + body))
    s = _load(Scene, d / "mixed.xml")
    assert len(s.enable_multiscattering()) == 1          # the rough conductor
    s.add_point_light((0.5, 1.5, 0.3), (3.0, 2.5, 2.0))
    st = s.settings()
    s.set_lens(camera_type=1, fov_x=st.fov_x, focal_length=0.05, focal_distance=3.3, relative_aperture=0.5, blade_count=5,
               aperture_rotation=0.3, film_size=tuple(st.film_size[:]))
    frame = s.frame_params(0)
    assert frame.aperture_radius > 0 and frame.blade_count == 5
    return s


def _glass(Scene, d):
    """A closed smooth-dielectric slab and a smooth conductor mirror between the camera and a lamp, a matte
    floor, the 8-texel environment cube."""
    _write_faces(d / "slab.obj", _box((-0.9, 0.3, 0.4), (0.3, 1.5, 0.6)))
    _write_faces(d / "mirror.obj", [_quad((0.9, 0.9, 0.8), (0.35, 0, 0.35), (0, 0.6, 0))])
    _write_faces(d / "floor.obj", [_quad((0, 0, 0.5), (2, 0, 0), (0, 0, -2))])
    _write_faces(d / "lamp.obj", [_quad((-0.2, 0.9, 1.6), (-0.5, 0, 0), (0, 0.5, 0))])
    body = (_shape("slab", '<bsdf type="dielectric"><float name="int_ior" value="1.5"/></bsdf>')
            + _shape("mirror", '<bsdf type="twosided"><bsdf type="conductor"><rgb name="eta" value="0.15, 0.4, 1.4"/><rgb name="k" value="3.6, 2.6, 2.3"/></bsdf></bsdf>')
            + _shape("floor", _diffuse("0.7, 0.6, 0.5")) + _shape("lamp", emitter="4, 5, 3"))
    (d / "glass.xml").write_text(_xml(_integrator(6) + _camera((0, 0.9, -1.6), fov=70) + body))
    s = _load(Scene, d / "glass.xml")
    s.set_environment_light((1.0, 1.0, 1.0), env_cube(8))
    return s


def _sheet(Scene, d):
    """A thin-dielectric sheet and a closed rough-dielectric octahedron (alpha 0.6, multiscattering off) over a
    matte floor under the environment cube."""
    import ray_truth as RT
    V, F = RT.closed_polyhedron(np.random.default_rng(3), levels=0)
    assert RT.is_closed(F)
    V = V * 0.9 + np.array([0.45, 0.8, 0.6])
    faces = []
    for a, b, c in F:
        n = np.cross(V[b] - V[a], V[c] - V[a])
        faces.append(([tuple(V[a]), tuple(V[b]), tuple(V[c])], tuple(n / np.linalg.norm(n))))
    _write_faces(d / "solid.obj", faces)
    _write_faces(d / "pane.obj", [_quad((-0.6, 0.8, 0.3), (-0.45, 0, 0.2), (0, 0.6, 0))])
    _write_faces(d / "floor.obj", [_quad((0, 0, 0.5), (2, 0, 0), (0, 0, -2))])
    body = (_shape("solid", '<bsdf type="roughdielectric"><float name="int_ior" value="1.5"/><float name="alpha" value="0.6"/></bsdf>')
            + _shape("pane", '<bsdf type="thindielectric"><float name="int_ior" value="1.5"/></bsdf>')
            + _shape("floor", _diffuse("0.5, 0.6, 0.7")))
    (d / "sheet.xml").write_text(_xml(_integrator(3) + _camera((0, 0.9, -1.6), pitch=5, fov=70) + body))
    s = _load(Scene, d / "sheet.xml")
    s.set_environment_light((1.0, 1.0, 1.0), env_cube(8))
    return s


def _coat(Scene, d):
    """The bleed box's shape with a smooth-plastic floor (ior 1.5, internal scattering SINGLE: the loader's
    default for `plastic`), a smooth-plastic left wall (two-sided, ior 1.8, `nonlinear`: MULTIPLE) whose face
    looks OUT of the box, so that every path meets it from behind and takes the two-sided mirror branch, a
    bitmap back wall, plain right wall and ceiling, a lamp before the back wall that faces the camera -- seen
    directly and, below it, in the floor's coat -- and a point light, which a mixed vertex receives through
    its Lambert base alone."""
    rng = np.random.default_rng(9)
    _ppm(d / "back.ppm", rng.integers(30, 256, (4, 5, 3)))
    parts = {
        "floor": (_quad((0, 0, 0), (1, 0, 0), (0, 0, -1)), '<bsdf type="plastic"><rgb name="diffuse_reflectance" value="0.75, 0.6, 0.2"/>'
                  '<float name="int_ior" value="1.5"/></bsdf>'),
        "left": (_quad((-1, 1, 0), (0, 0, 1), (0, 1, 0)), '<bsdf type="twosided"><bsdf type="plastic"><rgb name="diffuse_reflectance" value="0.2, 0.5, 0.8"/>'
                 '<float name="int_ior" value="1.8"/><boolean name="nonlinear" value="true"/></bsdf></bsdf>'),
        "ceiling": (_quad((0, 2, 0), (1, 0, 0), (0, 0, 1)), _diffuse("0.7, 0.7, 0.6")),
        "back": (_quad((0, 1, 1), (-1, 0, 0), (0, 1, 0)), '<bsdf type="diffuse"><texture name="reflectance" type="bitmap">'
                 '<string name="filename" value="back.ppm"/></texture></bsdf>'),
        "right": (_quad((1, 1, 0), (0, 0, 1), (0, 1, 0)), _diffuse("0.8, 0.15, 0.1")),
    }
    body = ""
    for name, (face, bsdf) in parts.items():
        _write_faces(d / f"{name}.obj", [face])
        body += _shape(name, bsdf)
    _write_faces(d / "lamp.obj", [_quad((0.2, 0.7, 0.9), (-0.35, 0, 0), (0, 0.3, 0))])
    body += _shape("lamp", emitter="6, 5, 4")
    (d / "coat.xml").write_text(_xml(_integrator(3) + _camera((0.1, 0.9, -0.95), yaw=-6, pitch=12, fov=90) + body))
    s = _load(Scene, d / "coat.xml")
    s.add_point_light((-0.4, 1.5, -0.2), (1.5, 1.3, 1.0))
    return s


def _frost(Scene, d):
    """The sheet scene's closed rough-dielectric octahedron (alpha 0.6) with multiscattering ON (BSDF QUIRK Q1:
    the drawn density is not the reported pdf) over a matte floor, a lamp behind it that faces the camera, the
    environment cube."""
    import ray_truth as RT
    V, F = RT.closed_polyhedron(np.random.default_rng(3), levels=0)
    assert RT.is_closed(F)
    V = V * 0.9 + np.array([0.45, 0.8, 0.6])
    faces = []
    for a, b, c in F:
        n = np.cross(V[b] - V[a], V[c] - V[a])
        faces.append(([tuple(V[a]), tuple(V[b]), tuple(V[c])], tuple(n / np.linalg.norm(n))))
    _write_faces(d / "solid.obj", faces)
    _write_faces(d / "floor.obj", [_quad((0, 0, 0.5), (2, 0, 0), (0, 0, -2))])
    _write_faces(d / "lamp.obj", [_quad((0.45, 0.8, 1.6), (-0.8, 0, 0), (0, 0.6, 0))])
    body = (_shape("solid", '<bsdf type="roughdielectric"><float name="int_ior" value="1.5"/><float name="alpha" value="0.6"/></bsdf>')
            + _shape("floor", _diffuse("0.5, 0.6, 0.7")) + _shape("lamp", emitter="1.6, 2, 1.2"))
    (d / "frost.xml").write_text(_xml(_integrator(6) + _camera((0, 0.9, -1.6), pitch=5, fov=70) + body))
    s = _load(Scene, d / "frost.xml")
    changed = s.enable_multiscattering()
    assert len(changed) == 1 and s.material_setting(changed[0]).multiscattering          # the solid
    s.set_environment_light((1.0, 1.0, 1.0), env_cube(8))
    return s


def with_case(scene, bounce, visible=True):
    """The scene at max_bounce B with LIGHT_VISIBLE on or off."""
    scene.set_max_bounce(int(bounce))
    scene.features = (scene.features | LIGHT_VISIBLE) if visible else (scene.features & ~LIGHT_VISIBLE)
    return scene
