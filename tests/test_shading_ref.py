"""The CPU oracle's camera rays, hit reconstruction, texture / environment lookups and light sampling
against tests/shading_ref.py, a float64 reference written from definitions: values at seeded inputs
(|got - ref64| <= K e + 4 ulp, ref_tolerance.tolerance_ratio), inputs on a discontinuity of the operation
matched against either side, the samplers' draws against their stated densities (chi-square), and the
consistency of the sampler with the evaluation. The same checks run through the device entries in
tests/test_gpu_shading_ref.py, which imports the scenes, inputs and checks from here: every check takes
a `probe` (OracleProbe here, the device's there)."""
import ctypes as C

import numpy as np
import pytest

import random_scenes as RS
import shading_ref as R
from ref_tolerance import chi_square_quantile, tolerance_ratio

INPUTS = 4000
# K of |got - ref64| <= K e + 4 ulp per quantity: the project's 6 wherever the oracle's measured worst ratio and
# half as much again fits in it (the rule test_bsdf_ref documents), else that product rounded up. The oracle's
# worst ratios over all cases ("Shading reference", lists them per case): the tangent 9.27
# (the sheared instance; Gram-Schmidt cancels where the interpolated tangent lies near the normal, and one float32
# run is one draw of that error: 9.27 x 1.5 = 13.9), the mesh-light sampler's pdf 3.67, everything else at most 1.81.
# None of these numbers comes from the device.
TOLERANCE_K = 6
QUANTITY_K = {"tangent": 14}
AMBIGUOUS_CAP = 0.02
EPS = 2.0 ** -24
CHI_DRAWS = 200_000
INVALID = 0xFFFFFFFF


# ---- scenes -----------------------------------------------------------------------------------------
def _matrix(m):
    return " ".join(f"{v:.6g}" for v in np.asarray(m, np.float64).reshape(-1))


def _shear():
    m = np.eye(4)
    m[:3, :3] = np.array([[1.0, 0.45, 0.0], [0.0, 1.0, 0.3], [0.2, 0.0, 1.0]])
    m[:3, 3] = (-1.1, 0.2, 1.7)
    return _matrix(m)


def transforms():
    """The six instance transforms, by name (Mitsuba matrices)."""
    mm = RS.mitsuba_matrix
    return {"identity": mm(), "rigid": mm((1.3, 0.2, -0.7), yaw=37, pitch=-20), "uniform": mm((-1.6, 0.1, -1.2), yaw=115, pitch=10, scale=(1.7, 1.7, 1.7)),
            "nonuniform": mm((1.9, -0.1, 1.4), yaw=-50, pitch=25, scale=(0.6, 1.5, 2.2)), "shear": _shear(),
            "mirror": mm((-0.4, 0.3, 2.6), yaw=200, pitch=-15, scale=(-1.2, 1.2, 1.2))}


def _lamp_matrix(name, k):
    """The rectangle lamp of transform `name`: a 1 x 0.8 rectangle pitched by 35 degrees (so that its normal lies along
    no axis of a non-uniform scale) under that transform's linear part, lifted above the soups."""
    m = np.array([float(x) for x in transforms()[name].split(" ")]).reshape(4, 4)
    c, sn = np.cos(np.radians(35.0)), np.sin(np.radians(35.0))
    m[:3, :3] = m[:3, :3] @ np.array([[1, 0, 0], [0, c, -sn], [0, sn, c]]) @ np.diag([0.5, 0.4, 1.0])
    m[:3, 3] = (2.0 * (k % 3) - 2.0, 3.0 + 0.3 * k, 2.0 * (k // 3) - 1.0)
    return _matrix(m)


def _fan(path):
    """A mesh light of six triangles of unequal area (0.014 .. 0.39) around one vertex."""
    ang = np.cumsum([0.0, 0.1, 0.25, 0.5, 0.9, 1.4, 2.0])
    rad = np.array([0.4, 0.7, 0.9, 0.6, 1.0, 0.8, 0.5])
    V = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([rad * np.cos(ang), 0.05 * np.sin(3 * ang), rad * np.sin(ang)], 1)])
    F = [(0, k + 2, k + 1) for k in range(6)]
    N = np.tile([0.0, 1.0, 0.0], (len(V), 1))
    RS._write_soup(path, V, N, np.zeros((len(V), 2)), np.asarray(F))


def _bsdfs(rng):
    return "".join("  " + RS._BSDFS[k].format(id=f"b{i}", c=RS._c(rng), a=f"{rng.uniform(0.1, 0.8):.3f}") + "\n"
                   for i, k in enumerate((0, 1, 3, 5)))


def _write_common(d, rng):
    RS._write_soup(d / "soup.obj", *RS.soup(rng, 3, 6))          # 30 triangles, smooth normals, texcoords
    img = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)           # 5 x 3: odd, not square
    (d / "albedo.ppm").write_bytes(b"P6 5 3 255\n" + img.tobytes())
    return _bsdfs(rng) + ('  <bsdf type="roughplastic" id="bt"><texture name="diffuse_reflectance" type="bitmap"><string name="filename" '
                          'value="albedo.ppm"/></texture><float name="alpha" value="0.35"/></bsdf>\n')


def _shape(kind, ident, matrix, ref=None, radiance=None, filename=None):
    inner = f'<string name="filename" value="{filename}"/>' if filename else ""
    inner += f'<ref id="{ref}"/>' if ref else ""
    inner += f'<emitter type="area"><rgb name="radiance" value="{radiance}"/></emitter>' if radiance else ""
    return f'  <shape type="{kind}" id="{ident}">{inner}<transform name="to_world"><matrix value="{matrix}"/></transform></shape>\n'


def write_instances_scene(d):
    """The soup instanced six ways (the textured material on the rigid one) and a rectangle lamp under each of the
    six transforms: six mesh lights."""
    rng = np.random.default_rng(20240)
    d.mkdir(parents=True, exist_ok=True)
    body = '  <integrator type="path"><integer name="max_depth" value="4"/></integrator>\n'
    body += RS._sensor("perspective", 48, 36, RS.mitsuba_matrix((0.2, 1.4, -6.0), pitch=10), '    <float name="fov" value="50"/>\n')
    body += _write_common(d, rng)
    for k, (name, m) in enumerate(transforms().items()):
        body += _shape("obj", f"soup_{name}", m, ref="bt" if name == "rigid" else f"b{k % 4}", filename="soup.obj")
    for k, name in enumerate(transforms()):
        body += _shape("rectangle", f"lamp_{name}", _lamp_matrix(name, k), radiance=f"{3 + k}, {4 + 0.5 * k}, {9 - k}")
    (d / "instances.xml").write_text(RS._xml(body))
    return d / "instances.xml"


def write_lights_scene(d):
    """One soup, one rectangle lamp, the fan (two mesh lights); the environment cube, a point and a directional light
    are added through the scene API: five lights, every kind."""
    rng = np.random.default_rng(20241)
    d.mkdir(parents=True, exist_ok=True)
    _fan(d / "fan.obj")
    body = '  <integrator type="path"><integer name="max_depth" value="4"/></integrator>\n'
    body += RS._sensor("perspective", 48, 36, RS.mitsuba_matrix((0.2, 1.4, -6.0), pitch=10), '    <float name="fov" value="50"/>\n')
    body += _write_common(d, rng)
    body += _shape("obj", "soup", transforms()["rigid"], ref="bt", filename="soup.obj")
    body += _shape("rectangle", "lamp", _lamp_matrix("rigid", 1), radiance="5, 6, 7")
    body += _shape("obj", "fan", RS.mitsuba_matrix((-0.8, 2.8, 0.6), yaw=25, pitch=190, scale=(1.4, 1.4, 1.4)), radiance="8, 3, 2", filename="fan.obj")
    (d / "lights.xml").write_text(RS._xml(body))
    return d / "lights.xml"


class Case:
    """A flat scene with the arrays the reference reads, and frame parameters. `edit` returns a copy with some
    arrays replaced (the copy owns them)."""

    def __init__(self, flat, frame, keep=()):
        self.flat, self.frame_params, self._keep = flat, frame, list(keep)
        self.ref = R.from_flat(flat)

    def frame(self, light_count=None):
        f = type(self.frame_params).from_buffer_copy(self.frame_params)
        if light_count is not None:
            f.light_count = light_count
        return f

    def edit(self, vertices=None, materials=None, lights=None, transforms=None, overrides=None, material_ids=None, textures=None, frame=None):
        from directcomputeraytracing_amd import _abi
        f = type(self.flat).from_buffer_copy(self.flat)
        keep = [self] + self._keep

        def put(field, array, ctype, count_field=None, count=None):
            a = np.ascontiguousarray(array)
            keep.append(a)
            setattr(f, field, a.ctypes.data_as(C.POINTER(ctype)))
            if count_field:
                setattr(f, count_field, count)
        if vertices is not None:
            put("vertices", vertices.astype(np.float32), _abi.Vertex)
        if materials is not None:
            put("materials", materials.astype(np.uint32), _abi.Material, "material_count", len(materials))
        if lights is not None:
            put("lights", lights.astype(np.uint32), _abi.Light, "light_count", len(lights))
        if transforms is not None:      # (I, 3, 4) forward matrices; the inverses stay (the probes read none)
            I = f.instance_count
            both = R._array(self.flat.instance_transforms, C.c_float, (2 * I, 12))
            both[:I] = transforms.reshape(I, 12)
            put("instance_transforms", both.astype(np.float32), _abi.Float4x3)
        if overrides is not None:
            put("instance_material_overrides", overrides.astype(np.uint32), C.c_uint32)
        if material_ids is not None:
            put("material_ids", material_ids.astype(np.uint32), C.c_uint32)
        if textures is not None:        # [(format, pixels (h, w, channels) uint8)]
            arr = (_abi.Texture * len(textures))()
            for k, (fmt, px) in enumerate(textures):
                px = np.ascontiguousarray(px, np.uint8)
                keep.append(px)
                arr[k] = _abi.Texture(px.shape[1], px.shape[0], fmt, px.ctypes.data_as(C.POINTER(C.c_uint8)))
            keep.append(arr)
            f.textures, f.texture_count = arr, len(textures)
        fr = frame or self.frame()
        if lights is not None:
            fr.light_count = len(lights)
        return Case(f, fr, keep)


def _named(M, table):
    """The name of an instance from its forward matrix (column c, row r): the entry of `table` (name -> Mitsuba matrix)
    with its translation's y and z. (The loader turns Mitsuba's right-handed frame into the renderer's left-handed one
    by negating x: every instance written here reaches the flat scene with a negative determinant -- the one named
    "mirror" alone with a positive one. hit_cases adds an exact identity and a proper rotation.)"""
    for name, m in table.items():
        t = np.array([float(x) for x in m.split(" ")]).reshape(4, 4)[:3, 3]
        if np.allclose(M[1:, 3], t[1:], atol=1e-4):
            return name
    raise AssertionError(M)


class Scenes:
    """The scenes, loaded once per session."""

    def __init__(self, directory):
        from directcomputeraytracing_amd import Scene, scenes
        a = Scene((48, 36))
        a.load_from_file(write_instances_scene(directory / "instances"))
        self.instances = Case(a.flat(), a.frame_params(1), [a])
        b = Scene((48, 36))
        b.load_from_file(write_lights_scene(directory / "lights"))
        b.set_environment_light((0.9, 1.1, 0.7), scenes.env_cube(8))
        b.add_point_light((0.4, 2.6, -1.2), (9.0, 8.0, 7.0))
        b.add_directional_light((0.6, 0.3, 0.0), (1.5, 1.4, 1.2))
        self.lights = Case(b.flat(), b.frame_params(1), [b])
        self.scene_b = b
        s = self.instances.ref
        self.soup_triangles = np.arange(int(s["lights"][:, 3].min()))        # the soup is the first mesh
        P = s["vertices"][s["triangles"][self.soup_triangles]][..., :3].astype(np.float64)
        area = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
        self.solid_triangles = self.soup_triangles[area > 1e-6]
        uses = np.bincount(s["triangles"][self.soup_triangles].ravel(), minlength=len(s["vertices"]))
        alone = (uses[s["triangles"][self.solid_triangles]] == 1).all(1)
        self.loose_triangles = self.solid_triangles[alone]           # triangles that share no vertex with another
        assert len(self.loose_triangles) >= 6
        lamp = s["light_indices"] != INVALID
        lamps = {name: _lamp_matrix(name, k) for k, name in enumerate(transforms())}
        self.soup_instance = {_named(s["transforms"][i], transforms()): i for i in np.flatnonzero(~lamp)}
        self.lamp_light = {_named(s["transforms"][i], lamps): int(s["light_indices"][i]) for i in np.flatnonzero(lamp)}
        assert sorted(self.soup_instance) == sorted(transforms()) and sorted(self.lamp_light) == sorted(transforms())


@pytest.fixture(scope="session")
def shading_scenes(native_lib, tmp_path_factory):
    return Scenes(tmp_path_factory.mktemp("shading_ref"))


def cameras():
    """name -> a function of a Scene that sets the camera up."""
    return {
        "pinhole": lambda s: s.set_lens(camera_type=0, fov_x=1.0),
        "thin_disk": lambda s: s.set_lens(camera_type=1, focal_length=0.05, focal_distance=3.0, relative_aperture=1.8, blade_count=0),
        "thin_5_blades": lambda s: s.set_lens(camera_type=1, focal_length=0.05, focal_distance=2.5, relative_aperture=2.0, blade_count=5, aperture_rotation=0.7),
        "thin_6_blades": lambda s: s.set_lens(camera_type=1, focal_length=0.035, focal_distance=4.0, relative_aperture=1.4, blade_count=6, aperture_rotation=2.9),
        "turned_6_blades": lambda s: (s.set_camera((1.5, 2.0, -3.0), (0.35, -0.8, 0.2)),
                                      s.set_lens(camera_type=1, focal_length=0.05, focal_distance=3.5, relative_aperture=2.8, blade_count=6, aperture_rotation=1.3)),
    }


def camera_frame(shading_scenes, name):
    s = shading_scenes.scene_b
    s.set_camera((0.2, 1.4, -6.0), (0.1, 0.0, 0.0))
    cameras()[name](s)
    f = s.frame_params(1)
    assert (f.aperture_radius > 0) == (name != "pinhole"), (name, f.aperture_radius)
    if "blades" in name:
        n = int(name.split("_")[1])
        assert f.blade_count == n and f.aperture_base_angle != 0
        np.testing.assert_allclose(np.hypot(*f.blade_vertex_pos[:]), f.aperture_radius, rtol=1e-5)
    return f


# ---- probes -----------------------------------------------------------------------------------------
class OracleProbe:
    def __init__(self, oracle_mod):
        self.o = oracle_mod

    def camera(self, frame, film, ap):
        return self.o.camera_ray_at(frame, film, ap)

    def hit(self, case, records, use_table=False):
        return self.o.intersection_probe(case.flat, records)

    def sample(self, case, light_count, p, states):
        return self.o.light_sample(case.flat, light_count, p, states)

    def evaluate(self, case, light_count, light_triangle, nwd):
        return self.o.light_eval(case.flat, light_count, light_triangle, nwd)

    def env(self, case, d):
        return self.o.env_lookup(case.flat, d)


@pytest.fixture(scope="module")
def probe(oracle_mod):
    return OracleProbe(oracle_mod)


# ---- inputs -----------------------------------------------------------------------------------------
def numbers(seed, shape):
    """float32 numbers in [0, 1) with 24 random bits each."""
    return (np.random.default_rng(seed).integers(0, 1 << 24, shape) / float(1 << 24)).astype(np.float32)


def hit_inputs(seed, triangles, instance, n=INPUTS):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(size=n), rng.uniform(size=n)
    s = np.sqrt(a)
    u, v = (1 - s).astype(np.float32), (b * s).astype(np.float32)
    tri = rng.choice(triangles, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
    return u, v, tri, np.full(n, instance, np.uint32)


def light_points(seed, n=INPUTS, top=2.2):
    rng = np.random.default_rng(seed)
    return rng.uniform([-3, -0.5, -3], [3, top, 3], (n, 3)).astype(np.float32), rng.integers(1, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)


# ---- the tolerance ----------------------------------------------------------------------------------
def vector_ratio(got, ref64, ref32):
    """tolerance_ratio for the components of geometric vectors (N, 3) -- positions, directions, normals, tangents; colours
    (albedo, radiance, rgb), whose channels are independent products, take tolerance_ratio per element. The rounding of a component that a rotation, a
    matrix or a normalisation produced scales with the vector, not with the component: a direction's 1e-4
    component carries the 6e-8 of its unit vector. So the float32 run's error of a vector is its largest
    component error, and the ulps and the floor of tolerance_ratio refer to its largest component: the check
    runs on |got - ref64| and ref32's error, both taken per vector in the max norm, against that magnitude."""
    got, ref64, ref32 = (np.asarray(a, np.float64).reshape(len(ref64), -1) for a in (got, ref64, ref32))
    size = np.abs(ref64).max(1)
    err = np.abs(got - ref64).max(1)
    err32 = np.abs(ref32 - ref64).max(1)
    # (got = size + err and ref32 = size + err32 carry the same differences against ref64 = size; a component of got
    # that is not finite makes err, and so the ratio, infinite or NaN, which `worst` counts as a failure)
    with np.errstate(invalid="ignore"):
        r = tolerance_ratio(size + err, size, size + err32)
    return np.where(np.isfinite(ref64).all(1) & ~np.isfinite(got).all(1), np.inf, r)


def worst(label, ratios, report):
    ratios = np.asarray(ratios, np.float64)
    k = float(np.where(np.isnan(ratios), np.inf, ratios).max()) if ratios.size else 0.0      # (a NaN ratio fails)
    report[label] = max(report.get(label, 0.0), k)
    return k


def assert_ratios(report, where):
    print(where + ": " + ", ".join(f"{k} {v:.2f}" for k, v in report.items()))
    bad = {k: v for k, v in report.items() if not v <= QUANTITY_K.get(k, TOLERANCE_K)}
    assert not bad, (where, bad)


def test_vectorised_xoshiro_is_the_scalar_restatement():
    """shading_ref's numpy xoshiro128** against the scalar restatement test_oracle.py pins the oracle's with: 64 states, 8
    steps each, outputs and states."""
    from test_oracle import xoshiro_next
    states = np.random.default_rng(2).integers(0, 1 << 32, (64, 4), dtype=np.uint64).astype(np.uint32)
    scalar = [[int(x) for x in s] for s in states]
    for _ in range(8):
        out, states = R.xoshiro_next(states)
        assert [xoshiro_next(s) for s in scalar] == out.tolist() and scalar == states.tolist()


# ---- 1. camera --------------------------------------------------------------------------------------
CAMERA_CASES = list(cameras())


def check_camera_values(probe, frame, name):
    film, ap = numbers(sum(map(ord, name)), (INPUTS, 2)), numbers(sum(map(ord, name)) + 1, (INPUTS, 3))
    f = R.frame_dict(frame)
    o64, d64, _, _ = R.camera_ray(f, film, ap, np.float64)
    o32, d32, _, _ = R.camera_ray(f, film, ap, np.float32)
    o, d = probe.camera(frame, film, ap)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    report = {}
    worst("origin", vector_ratio(o, o64, o32), report)
    worst("direction", vector_ratio(d, d64, d32), report)
    assert_ratios(report, f"camera {name}")
    return report


@pytest.mark.parametrize("name", CAMERA_CASES)
def test_camera_rays_against_float64_reference(probe, shading_scenes, name):
    """generate_ray at 4 000 film points and aperture numbers per camera: origin and direction as vectors
    (vector_ratio) within K = 6."""
    check_camera_values(probe, camera_frame(shading_scenes, name), name)


def check_thin_lens_focus(probe, frame, name):
    """Every ray of one film point passes through one point of the plane z = focal_distance (camera space): 64 film
    points x 64 aperture numbers. Tolerance: origin and direction each carry at most 8 float32 roundings of their
    magnitude (a normalisation, the 4 x 4 product), so the point at parameter t = focal_distance / d.z is off
    by at most 8 eps (t + |origin|) from each, 16 eps (t + |origin|) in all; the way back to camera space is float64."""
    film = np.repeat(numbers(5, (64, 2)), 64, 0)
    ap = numbers(6, (64 * 64, 3))
    o, d = probe.camera(frame, film, ap)
    f = R.frame_dict(frame)
    M = f["camera"].astype(np.float64)
    inv = np.linalg.inv(M[:3, :3])
    oc, dc = (o.astype(np.float64) - M[3, :3]) @ inv, d.astype(np.float64) @ inv
    t = (float(f["focal_distance"]) - oc[:, 2]) / dc[:, 2]
    x = (oc + dc * t[:, None]).reshape(64, 64, 3)
    _, _, _, focus = R.camera_ray(f, film, ap)
    tol = 16 * EPS * (t + np.abs(o).max(1)).reshape(64, 64)
    dev = np.abs(x - focus.reshape(64, 64, 3)).max(2)
    assert (np.abs(oc[:, 2]) <= 8 * EPS * np.abs(o).max(1)).all()                        # the origin lies on the aperture plane
    r = np.hypot(oc[:, 0], oc[:, 1])
    assert (r <= float(f["aperture_radius"]) * (1 + 1e-5) + 8 * EPS * np.abs(o).max(1)).all()
    print(f"focus {name}: worst deviation / tolerance {np.max(dev / tol):.3f}")
    assert (dev <= tol).all(), np.max(dev / tol)


@pytest.mark.parametrize("name", [c for c in CAMERA_CASES if c != "pinhole"])
def test_thin_lens_rays_of_one_film_point_meet_on_the_focus_plane(probe, shading_scenes, name):
    check_thin_lens_focus(probe, camera_frame(shading_scenes, name), name)


def triangle_cells(u, v, k=4):
    """The index among k^2 equal-area cells (the k-fold barycentric subdivision) of barycentrics (u, v)."""
    a, b = np.clip(u * k, 0, k - 1e-9), np.clip(v * k, 0, k - 1e-9)
    i, j = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)
    upper = ((a - i) + (b - j) > 1).astype(np.int64)
    # row i holds 2 (k - i) - 1 cells: lower cells j = 0 .. k - i - 1, upper cells j = 0 .. k - i - 2
    start = np.array([sum(2 * (k - r) - 1 for r in range(q)) for q in range(k + 1)])
    j = np.minimum(j, k - 1 - i - upper)       # (points that rounding put across the hypotenuse)
    return start[i] + 2 * j + upper


def chi_square(counts, expected):
    counts, expected = np.asarray(counts, np.float64), np.asarray(expected, np.float64)
    assert expected.min() >= 20, expected.min()
    return float(((counts - expected) ** 2 / expected).sum()), len(counts) - 1


def check_aperture_distribution(probe, frame, name):
    """200 000 aperture points over equal-area cells: the disk in 8 rings x 16 sectors, an n-gon in n blades x 16
    sub-triangles (the 4-fold barycentric subdivision of the triangle centre - vertex - vertex), chi-square at 1e-6.
    The density is uniform over the shape."""
    film = np.full((CHI_DRAWS, 2), 0.5, np.float32)
    ap = numbers(77, (CHI_DRAWS, 3))
    o, _ = probe.camera(frame, film, ap)
    f = R.frame_dict(frame)
    M = f["camera"].astype(np.float64)
    oc = (o.astype(np.float64) - M[3, :3]) @ np.linalg.inv(M[:3, :3])
    x, y = oc[:, 0], oc[:, 1]
    n, radius = f["blade_count"], float(f["aperture_radius"])
    if n <= 2:
        ring = np.minimum((8 * (x * x + y * y) / radius ** 2).astype(np.int64), 7)
        sector = np.minimum(((np.arctan2(y, x) + np.pi) / (2 * np.pi) * 16).astype(np.int64), 15)
        counts = np.bincount(ring * 16 + sector, minlength=128)
    else:
        half = np.pi / n
        phi = np.mod(np.arctan2(y, x) - float(f["aperture_base_angle"]) + half, 2 * np.pi)
        blade = np.minimum((phi / (2 * half)).astype(np.int64), n - 1)
        turn = -(blade * 2 * half + float(f["aperture_base_angle"]))
        lx, ly = x * np.cos(turn) - y * np.sin(turn), x * np.sin(turn) + y * np.cos(turn)
        vx, vy = float(f["blade_vertex_pos"][0]), float(f["blade_vertex_pos"][1])
        u, v = 0.5 * (lx / vx + ly / vy), 0.5 * (lx / vx - ly / vy)            # (lx, ly) = u (vx, vy) + v (vx, -vy)
        assert (u > -1e-5).all() and (v > -1e-5).all() and (u + v < 1 + 1e-5).all()
        counts = np.bincount(blade * 16 + triangle_cells(u, v), minlength=16 * n)
    chi2, dof = chi_square(counts, np.full(len(counts), CHI_DRAWS / len(counts)))
    print(f"aperture {name}: chi2/dof {chi2 / dof:.3f} (dof {dof}, bound {chi_square_quantile(dof) / dof:.3f})")
    assert chi2 < chi_square_quantile(dof), (chi2, dof)


@pytest.mark.parametrize("name", ["thin_disk", "thin_5_blades", "thin_6_blades"])
def test_aperture_points_are_uniform_over_the_shape(probe, shading_scenes, name):
    check_aperture_distribution(probe, camera_frame(shading_scenes, name), name)


# ---- 2. hit reconstruction --------------------------------------------------------------------------
HIT_FLOATS = {"position": slice(0, 3), "normal": slice(3, 6), "tangent": slice(6, 9), "geometry_normal": slice(9, 12)}


def checker_edit(case, inst):
    """The override material of instance `inst` with the roughness checkerboard on."""
    m = case.ref["materials"].copy()
    k = case.ref["overrides"][inst]
    m[k, 11] |= R.ROUGHNESS_TEXTURE
    m[k].view(np.float32)[7] = 0.6
    return case.edit(materials=m)


def hit_cases(sc):
    """name -> (case, instance): the six instances, and the edited scenes."""
    base = sc.instances
    out = {name: (base, i) for name, i in sc.soup_instance.items()}
    rigid, s = sc.soup_instance["rigid"], base.ref
    T = s["transforms"].copy()
    T[sc.soup_instance["identity"]] = np.eye(4)[:3]
    T[rigid, :, :3] = T[rigid, :, :3] * np.array([-1.0, 1.0, 1.0])[:, None]      # the x row back: a proper rotation
    assert np.linalg.det(T[rigid, :, :3].astype(np.float64)) > 0.99
    out["exact_identity"], out["proper_rotation"] = (base.edit(transforms=T), sc.soup_instance["identity"]), (base.edit(transforms=T), rigid)
    textured = int(s["overrides"][rigid])
    assert s["materials"][textured, 3] == 0 and len(s["textures"]) == 1 and s["textures"][0][1].shape[:2] == (3, 5)
    m = s["materials"].copy()
    m[textured].view(np.float32)[8:10] = (2.5, -1.75)
    out["tiling"] = (base.edit(materials=m), rigid)
    m = s["materials"].copy()
    m[textured].view(np.float32)[8:10] = (2.5, -1.75)
    m[textured, 11] |= R.ROUGHNESS_TEXTURE
    out["checker_tiled"] = (base.edit(materials=m), rigid)
    out["checker"] = (checker_edit(base, sc.soup_instance["uniform"]), sc.soup_instance["uniform"])
    # an R8 texture (read as (r, 0, 0, 1)) and an RGBA one whose alpha varies, 3 x 7 and 5 x 3, on two materials;
    # the identity instance without an override takes its triangles' materials, all four of them
    rng = np.random.default_rng(9)
    tex = [s["textures"][0], (1, rng.integers(0, 256, (7, 3, 1), dtype=np.uint8)), (0, rng.integers(0, 256, (3, 5, 4), dtype=np.uint8))]
    m = s["materials"].copy()
    m[0, 3], m[1, 3] = 1, 2
    ov = s["overrides"].copy()
    ov[sc.soup_instance["identity"]] = R.NO_OVERRIDE
    ids = s["material_ids"].copy()
    ids[sc.soup_triangles] = rng.integers(0, 4, len(sc.soup_triangles))
    out["r8_and_material_ids"] = (base.edit(materials=m, textures=tex, overrides=ov, material_ids=ids), sc.soup_instance["identity"])
    v = s["vertices"].copy()
    v[:, 6:9] = 0
    out["zero_tangent"] = (base.edit(vertices=v), rigid)
    v = s["vertices"].copy()
    v[:, 3:6] = (0.0, 1.0, 0.0)
    v[:, 3:6] = (1e-7, 1.0, 0.0)            # (a hair off: the fallback cross product is tiny, not 0) ...
    v[s["triangles"][sc.loose_triangles[:3]].ravel(), 3:6] = (0.0, 1.0, 0.0)     # ... but for three triangles, where it is 0
    v[:, 6:9] = (0.0, 0.5, 0.0)             # parallel to the normal: Gram-Schmidt leaves nothing
    out["normal_up"] = (base.edit(vertices=v), sc.soup_instance["identity"])
    return out


HIT_CASES = ["exact_identity", "proper_rotation", "identity", "rigid", "uniform", "nonuniform", "shear", "mirror", "tiling", "checker_tiled", "checker", "r8_and_material_ids",
             "zero_tangent", "normal_up"]


def hit_ambiguity(ref):
    """Per input: on a checker cell edge, on a tangent length threshold (judged from the float64 run alone). A texcoord
    is the sum of three float32 products and a product with the tiling: 8 roundings of its terms' magnitude
    (checker_scale) bound the distance at which float32 may land across the edge; the tangent lengths likewise
    against 8 roundings of the interpolated tangent's terms; the fallback's length is a copy of the normal's components
    (8 roundings of itself)."""
    g = ref["margins"]
    checker = g["uses_checker"] & (g["checker"] <= 8 * EPS * g["checker_scale"]).any(1)
    tol = 8 * EPS * g["t_scale"]
    near = lambda x: np.abs(x - R.DEGENERATE) <= tol
    tangent = near(g["len0"]) | near(g["len1"]) | (g["fallback"] & (np.abs(g["lenf"] - R.DEGENERATE) <= 8 * EPS * np.maximum(g["lenf"], R.DEGENERATE)))
    return checker, tangent


def hit_ratios(f, case, u, v, tri, inst, side):
    r64, r32 = R.hit(case.ref, u, v, tri, inst, np.float64, side), R.hit(case.ref, u, v, tri, inst, np.float32, side)
    out = {k: vector_ratio(f[:, sl], r64[k], r32[k]) for k, sl in HIT_FLOATS.items()}
    out["albedo"] = tolerance_ratio(f[:, 12:15], r64["albedo"], r32["albedo"].astype(np.float64)).max(1)      # per channel
    out["alpha"] = tolerance_ratio(f[:, 15], r64["alpha"], r32["alpha"].astype(np.float64))
    return out, r64


def check_hit_values(probe, sc, name, use_table=False):
    case, inst = hit_cases(sc)[name]
    u, v, tri, insts = hit_inputs(sum(map(ord, name)), sc.solid_triangles, inst)
    return check_hit_records(probe, case, name, u, v, tri, insts, use_table)


def check_hit_records(probe, case, name, u, v, tri, insts, use_table=False, cap=AMBIGUOUS_CAP):
    f, w = probe.hit(case, R_records(u, v, tri, insts), use_table)
    ratios, ref = hit_ratios(f, case, u, v, tri, insts, None)
    for k, sl in {**HIT_FLOATS, "albedo": slice(12, 15), "alpha": slice(15, 16)}.items():      # finite wherever the reference is
        ok = np.isfinite(np.asarray(ref[k]).reshape(len(f), -1)).all(1)
        assert np.isfinite(f[ok][:, sl]).all(), k
    # the words are exact
    assert (w[:, 0] == ref["material_type"]).all()
    assert (w[:, 1] == (ref["flags"] | ((tri >> np.uint32(31)) << np.uint32(1)))).all()
    assert (w[:, 2] == ref["light_index"]).all()
    checker, tangent = hit_ambiguity(ref)
    ambiguous = checker | tangent
    assert ambiguous.mean() <= cap, ambiguous.mean()
    if ambiguous.any():       # an input on a discontinuity matches the reference on one side of it
        for flip in ({"checker": 1 - ref["checker"]}, {"keep": ~ref["keep"]}, {"cross": ~ref["cross"]}):
            alt, _ = hit_ratios(f, case, u, v, tri, insts, flip)
            both = np.maximum.reduce([alt[k] for k in alt])
            best = np.maximum.reduce([ratios[k] for k in ratios])
            take = ambiguous & (both < best)
            for k in ratios:
                ratios[k] = np.where(take, alt[k], ratios[k])
    finite = np.isfinite(ref["tangent"]).all(1)
    # QUIRK Q5: where the reference's tangent is not finite, so is the renderer's
    assert not np.isfinite(f[~finite, 6:9]).any()
    report = {}
    for k, r in ratios.items():
        worst(k, r[finite] if k == "tangent" else r, report)
    report["ambiguous %"] = 100 * ambiguous.mean()
    assert_ratios({k: v for k, v in report.items() if k != "ambiguous %"}, f"hit {name} (ambiguous {100 * ambiguous.mean():.2f} %, non-finite tangents {(~finite).sum()})")
    return report, ref


def R_records(u, v, tri, inst):
    rec = np.empty((len(u), 4), np.uint32)
    rec[:, 0], rec[:, 1] = np.asarray(u, np.float32).view(np.uint32), np.asarray(v, np.float32).view(np.uint32)
    rec[:, 2], rec[:, 3] = tri, inst
    return rec


@pytest.mark.parametrize("name", HIT_CASES)
def test_hit_reconstruction_against_float64_reference(probe, shading_scenes, name):
    """hit_to_intersection at 4 000 records per case -- the soup under each of the six transforms, tex_tiling
    (2.5, -1.75), the roughness checkerboard, an R8 texture and per-triangle materials, all-zero tangents, normals
    parallel to +y: position, normal, tangent, geometry normal and albedo as vectors and alpha within K = 6, the
    material type, flags and light index exact; inputs on a checker edge or a tangent threshold (at most 2 %) match
    one side."""
    report, ref = check_hit_values(probe, shading_scenes, name)
    if name == "zero_tangent":
        assert not ref["keep"].any() and ref["cross"].all()                # the first fallback, every time
    if name == "normal_up":
        assert not ref["keep"].any() and (~ref["cross"]).any()            # the second fallback (QUIRK Q5)
        assert (~np.isfinite(ref["tangent"]).all(1)).any() and np.isfinite(ref["tangent"]).all(1).any()
    if name.startswith("checker"):
        assert 0.2 < ref["checker"].mean() < 0.8 and (ref["alpha"] == 0).any() and (ref["alpha"] > 0).any()
    if name == "r8_and_material_ids":
        assert len(np.unique(ref["material"])) == 4 and (ref["albedo"][ref["material"] == 0][:, 1:] == 0).all()


def test_texcoords_on_checker_edges_are_classified_and_match_one_side(probe, shading_scenes):
    """The classifier and the two-sided match on inputs aimed at the discontinuity: texcoords on checker cell edges
    (multiples of 0.5) and one float32 step either side of them, where the alpha jumps between 0 and roughness^2. At least
    a quarter of these inputs are classified ambiguous (the exact multiples: their float32 and float64 texcoords agree, a
    neighbour's need not), and every one matches the reference on one side."""
    sc = shading_scenes
    case, inst = texcoord_case(sc)
    g = np.array([k * 0.5 for k in range(1, 8)] + [0.25, 0.75], np.float32)
    g = np.concatenate([g, np.nextafter(g, np.float32(9)), np.nextafter(g, np.float32(-9))])
    u, v = np.repeat(g, 3), np.tile(np.array([0.1, 0.3, 0.6], np.float32), len(g))
    tri = np.full(len(u), sc.loose_triangles[0], np.uint32)
    report, ref = check_hit_records(probe, case, "checker edges", u, v, tri, np.full(len(u), inst, np.uint32), cap=1.0)
    assert report["ambiguous %"] >= 25 and (ref["alpha"] == 0).any() and (ref["alpha"] > 0).any()


# ---- 3. the environment cube ------------------------------------------------------------------------
def sphere(seed, n):
    z = np.random.default_rng(seed).normal(size=(n, 3))
    return (z / np.linalg.norm(z, axis=1, keepdims=True)).astype(np.float32)


def check_env_values(probe, sc):
    case = sc.lights
    d = sphere(3, INPUTS) * np.random.default_rng(4).uniform(0.1, 20.0, (INPUTS, 1)).astype(np.float32)     # any length
    got = probe.env(case, d)
    r64, r32 = R.env_lookup(case.ref["env"], d, np.float64), R.env_lookup(case.ref["env"], d, np.float32)
    assert np.isfinite(r64).all() and np.isfinite(got).all()
    report = {}
    worst("rgb", tolerance_ratio(got, r64, r32.astype(np.float64)), report)
    assert_ratios(report, "env lookup")
    assert len(np.unique(R.cube_face(d))) == 6
    return report


def test_environment_lookup_against_float64_reference(probe, shading_scenes):
    """sample_env at 4 000 directions of any length over all six faces of the 8-texel cube: the face of a float32
    direction is decided by comparisons (no ambiguity), the bilinear value within K = 6."""
    check_env_values(probe, shading_scenes)


# ---- 4. lights --------------------------------------------------------------------------------------
def light_cases(sc):
    """name -> (case, light count): six lamps (one per transform), every kind at once, each kind alone, and the
    lamps shrunk below the area thresholds."""
    out = {"six_lamps": (sc.instances, 6), "every_kind": (sc.lights, 5)}
    L = sc.lights.ref["lights"]
    kinds = R.light_kind(L)
    assert sorted(kinds) == [1, 2, 2, 4, 8]
    fan = int(np.flatnonzero((kinds == R.MESH) & (L[:, 4] == 6))[0])
    for name, k in (("point", R.POINT), ("directional", R.DIRECTIONAL), ("environment", R.ENVIRONMENT)):
        out[name + "_alone"] = (sc.lights.edit(lights=L[kinds == k]), 1)
    out["fan_alone"] = (sc.lights.edit(lights=L[[fan]]), 1)
    out["lamp_alone"] = (sc.lights.edit(lights=L[(kinds == R.MESH) & (L[:, 4] == 2)]), 1)
    return out


LIGHT_CASES = ["six_lamps", "every_kind", "point_alone", "directional_alone", "environment_alone", "fan_alone", "lamp_alone"]


def light_ambiguity(ref, p):
    """Per input: a mesh light's cos within rounding of 0 (wi = (x - p) / d carries the cancellation of x - p: 8 roundings
    of (|x| + |p|) / d, and the dot product 8 more of 1), an environment direction within 8 roundings of a face boundary."""
    mesh, env = ref["kind"] == R.MESH, ref["kind"] == R.ENVIRONMENT
    with np.errstate(invalid="ignore", divide="ignore"):
        d = ref["distance"] / (1 - float(R.SHADOW_EPSILON))
        tol = 8 * EPS * (1 + (np.abs(ref["point"]).max(1) + np.abs(p).max(1)) / d)
        cos = mesh & (np.abs(ref["cos"]) <= tol)
        margin, other = R.face_margin(ref["wi"])
    return cos, env & (margin <= 8 * EPS), other, np.where(mesh, tol, np.nan)


def light_ratios(f, ref64, ref32):
    return {"radiance": tolerance_ratio(f[:, 0:3], ref64["radiance"], ref32["radiance"].astype(np.float64)).max(1), "wi": vector_ratio(f[:, 3:6], ref64["wi"], ref32["wi"]),
            "pdf": tolerance_ratio(f[:, 6], ref64["pdf"], ref32["pdf"].astype(np.float64)),
            "distance": np.where(np.isinf(ref64["distance"]), np.where(f[:, 7] == np.inf, 0.0, np.inf),
                                 tolerance_ratio(np.where(np.isinf(ref64["distance"]), 0, f[:, 7]), np.where(np.isinf(ref64["distance"]), 0, ref64["distance"]),
                                                 np.where(np.isinf(ref64["distance"]), 0, ref32["distance"].astype(np.float64))))}


def check_light_sample_values(probe, sc, name, n=INPUTS):
    case, count = light_cases(sc)[name]
    p, states = light_points(sum(map(ord, name)), n)
    return check_light_sample_records(probe, case, count, name, p, states)


def check_light_sample_records(probe, case, count, name, p, states, cap=AMBIGUOUS_CAP):
    f, w = probe.sample(case, count, p, states)
    r64 = R.sample_light(case.ref, count, p, states, np.float64)
    r32 = R.sample_light(case.ref, count, p, states, np.float32)
    # exact: the delta flag and the state after 1, 1, 4 or 3 draws
    assert (w[:, 0] == r64["delta"]).all()
    assert (w[:, 1:] == r64["state"]).all()
    for k, sl in (("radiance", slice(0, 3)), ("wi", slice(3, 6)), ("pdf", slice(6, 7))):          # finite wherever the reference is
        ok = np.isfinite(np.asarray(r64[k]).reshape(len(f), -1)).all(1)
        assert np.isfinite(f[ok][:, sl]).all(), k
    assert not np.isnan(f[:, 7]).any() and (np.isinf(f[:, 7]) == np.isinf(r64["distance"])).all()
    ratios = light_ratios(f, r64, r32)
    cos, face, other, tol = light_ambiguity(r64, p)
    ambiguous = cos | face
    assert ambiguous.mean() <= cap, ambiguous.mean()
    if cos.any():
        # the dark side of cos = 0: no radiance, no pdf. The lit side: the light's radiance, and a pdf that is d^2 / (A cos)
        # for some cos in (0, tol] -- a pole, so all that can be said of it is that it is no smaller than at cos = tol
        # (less 1e-3 for the float32 roundings of d^2 and A). Whichever side ref64 itself is on is already in `ratios`.
        dark = (f[:, 0:3] == 0).all(1) & (f[:, 6] == 0)
        lit64 = R.sample_light(case.ref, count, p, states, np.float64, cos_floor=np.where(cos, tol, np.nan))
        lit32 = R.sample_light(case.ref, count, p, states, np.float32, cos_floor=np.where(cos, tol, np.nan))
        lit_radiance = tolerance_ratio(f[:, 0:3], lit64["radiance"], lit32["radiance"].astype(np.float64)).max(1)
        lit = cos & (f[:, 6] >= lit64["pdf"] * (1 - 1e-3)) & np.isfinite(f[:, 6])
        ratios["radiance"] = np.where(cos & dark, 0.0, np.where(lit, np.minimum(ratios["radiance"], lit_radiance), ratios["radiance"]))
        ratios["pdf"] = np.where(cos & (dark | lit), 0.0, ratios["pdf"])
    if face.any():            # the other face's texels
        alt = R.sample_light(case.ref, count, p, states, np.float64, env_face=other)
        alt32 = R.sample_light(case.ref, count, p, states, np.float32, env_face=other)
        ratios["radiance"] = np.where(face, np.minimum(ratios["radiance"], tolerance_ratio(f[:, 0:3], alt["radiance"], alt32["radiance"].astype(np.float64)).max(1)), ratios["radiance"])
    report = {"ambiguous %": 100 * ambiguous.mean()}
    for k in np.unique(r64["kind"]):
        m = r64["kind"] == k
        for q, r in ratios.items():
            worst({1: "point", 2: "mesh", 4: "directional", 8: "env"}[int(k)] + " " + q, r[m], report)
    assert_ratios({k: v for k, v in report.items() if k != "ambiguous %"}, f"light sample {name} (ambiguous {100 * ambiguous.mean():.2f} %)")
    return report, r64, (f, w), (p, states)


@pytest.mark.parametrize("name", LIGHT_CASES)
def test_light_sampling_against_float64_reference(probe, shading_scenes, name):
    """sample_light from 4 000 points and xoshiro states per case: radiance and wi as vectors, pdf and distance within
    K = 6, the delta flag and the advanced state (1, 1, 4, 3 draws) exact; a cos within rounding of 0 or a direction
    within rounding of a cube-face boundary (at most 2 %) matches one side."""
    _, ref, _, _ = check_light_sample_values(probe, shading_scenes, name)
    if name == "every_kind":
        assert sorted(np.unique(ref["kind"])) == [1, 2, 4, 8] and len(np.unique(ref["light"])) == 5
    if name in ("six_lamps", "fan_alone", "lamp_alone", "every_kind"):
        mesh = ref["kind"] == R.MESH
        assert (ref["pdf"][mesh] > 0).mean() > 0.2, (ref["pdf"][mesh] > 0).mean()


def test_points_on_a_lamps_plane_are_classified_and_match_one_side(probe, shading_scenes):
    """The classifier and the two-sided match where cos is 0 up to rounding: 512 points in the plane of the lamp (outside
    the rectangle, rounded to float32), where the sampler's answer jumps between nothing and the lit side's radiance and
    pdf (the pdf itself has a pole there, which the float32 run's own error follows). Most are classified ambiguous, and
    every one matches one side."""
    case, count = light_cases(shading_scenes)["lamp_alone"]
    L = case.ref["lights"][0]
    _, W, _, _, _ = R.triangle_geometry(case.ref, np.array([int(L[3])]), np.array([int(L[5])]), np.float64)
    rng = np.random.default_rng(21)
    a, b = rng.uniform(2, 5, 512) * rng.choice([-1, 1], 512), rng.uniform(2, 5, 512) * rng.choice([-1, 1], 512)
    p = (W[0, 0] + a[:, None] * (W[0, 1] - W[0, 0]) + b[:, None] * (W[0, 2] - W[0, 0])).astype(np.float32)
    states = rng.integers(1, 1 << 32, (512, 4), dtype=np.uint64).astype(np.uint32)
    report, _, _, _ = check_light_sample_records(probe, case, count, "on the lamp's plane", p, states, cap=1.0)
    assert report["ambiguous %"] >= 50


def eval_inputs_from_samples(case, ref):
    """evaluate_light's inputs at sampled points: the light and triangle, the light's normal there as the renderer forms
    it (QUIRK Q1; float32), wi and the unshortened distance |x - p|."""
    mesh = ref["kind"] == R.MESH
    tri = np.where(mesh, ref["triangle"], 0)
    normal = np.zeros((len(tri), 3))
    if mesh.any():
        inst = case.ref["lights"][ref["light"][mesh], 5].astype(np.int64)
        normal[mesh] = R.triangle_geometry(case.ref, tri[mesh], inst, np.float64)[3]
    d = np.where(np.isinf(ref["distance"]), 1.0, ref["distance"] / (1 - float(R.SHADOW_EPSILON)))
    nwd = np.concatenate([normal, ref["wi"], d[:, None]], 1).astype(np.float32)
    return np.stack([ref["light"], tri], 1).astype(np.uint32), nwd


def check_light_eval_values(probe, sc, name):
    case, count = light_cases(sc)[name]
    p, states = light_points(sum(map(ord, name)) + 7)
    ref = R.sample_light(case.ref, count, p, states)
    lt, nwd = eval_inputs_from_samples(case, ref)
    got = probe.evaluate(case, count, lt, nwd)
    a = (lt[:, 0], lt[:, 1], nwd[:, 0:3], nwd[:, 3:6], nwd[:, 6])
    (c64, p64), (c32, p32) = R.evaluate_light(case.ref, count, *a, np.float64), R.evaluate_light(case.ref, count, *a, np.float32)
    assert np.isfinite(c64).all() and np.isfinite(p64).all() and np.isfinite(got).all()
    # cos within rounding of 0 (8 roundings of a dot product of unit vectors) may fall on either side
    cos = -(nwd[:, 3:6].astype(np.float64) * nwd[:, 0:3]).sum(1)
    ambiguous = (ref["kind"] == R.MESH) & (np.abs(cos) <= 8 * EPS)
    assert ambiguous.mean() <= AMBIGUOUS_CAP
    rr, rp = tolerance_ratio(got[:, :3], c64, c32.astype(np.float64)).max(1), tolerance_ratio(got[:, 3], p64, p32.astype(np.float64))
    dark = (got == 0).all(1)
    rr, rp = np.where(ambiguous & dark, 0.0, rr), np.where(ambiguous & dark, 0.0, rp)
    report = {}
    worst("radiance", rr, report)
    worst("pdf", rp, report)
    assert_ratios(report, f"light eval {name}")
    # the delta lights evaluate to nothing
    delta = ref["delta"]
    assert (got[delta] == 0).all()
    return report


@pytest.mark.parametrize("name", LIGHT_CASES)
def test_light_evaluation_against_float64_reference(probe, shading_scenes, name):
    """evaluate_light at the points, directions and distances the reference's sampler drew, with the light's normal there:
    radiance and pdf within K = 6; nothing for the delta lights."""
    check_light_eval_values(probe, shading_scenes, name)


def check_sampler_against_evaluation(probe, sc):
    """At a sampled point evaluate_light's pdf is half the sampler's for a mesh light (QUIRK Q3, pinned) and equal, to the
    bit, for the environment. Inputs with cos >= 0.05: the evaluation gets the float32 normal, wi and distance, whose
    roundings move cos by at most 4 eps (relative 4 eps / 0.05 = 4.8e-6) and d^2 by 4 eps; with the handful of products
    on either side the two agree within 1e-5 relative."""
    case, count = sc.lights, 5
    p, states = light_points(99)
    f, _ = probe.sample(case, count, p, states)
    ref = R.sample_light(case.ref, count, p, states)
    lt, nwd = eval_inputs_from_samples(case, ref)
    nwd[:, 3:6], nwd[:, 6] = f[:, 3:6], np.where(np.isinf(f[:, 7]), 1.0, f[:, 7].astype(np.float64) / (1 - float(R.SHADOW_EPSILON)))
    got = probe.evaluate(case, count, lt, nwd)
    mesh = (ref["kind"] == R.MESH) & (ref["cos"] >= 0.05)
    assert mesh.sum() > 300
    np.testing.assert_allclose(2.0 * got[mesh, 3].astype(np.float64), f[mesh, 6], rtol=1e-5)
    assert (got[mesh, :3] == f[mesh, :3]).all()
    env = ref["kind"] == R.ENVIRONMENT
    assert env.sum() > 300 and (got[env, 3].view(np.uint32) == f[env, 6].view(np.uint32)).all()
    assert (got[env, :3].view(np.uint32) == f[env, :3].view(np.uint32)).all()         # the same lookup of the same direction


def test_evaluation_reports_half_the_samplers_mesh_pdf_and_the_same_environment_pdf(probe, shading_scenes):
    check_sampler_against_evaluation(probe, shading_scenes)


def check_true_density(probe, sc):
    """evaluate_light's pdf against the true solid-angle density d^2 / (A cos_true) / triangles / lights, cos_true from the
    inverse-transpose normal: equal within 2e-5 relative at cos >= 0.3 under the identity, rigid, uniform-scale and
    mirrored lamps. Their matrices are written with six digits: entries off by 5e-7 relative, which a matrix of condition
    2.5 (the rectangle's own 0.5 x 0.4 scale is part of it) turns into at most 2 * sqrt(3) * 5e-7 * 2.5 = 4.3e-6 of angle
    between the forward and the inverse-transpose normal, 4.3e-6 tan <= 1.4e-5 relative in the cosine; the float32
    roundings add 4 eps / 0.3 = 8e-7 and d^2 and the area a few eps more;
    under the non-uniformly scaled and the sheared lamp the renderer's cos is another angle's (QUIRK Q1).
    Returns the departure, max and median of |pdf / true - 1| over the lit samples of those two lamps."""
    case, count = sc.instances, 6
    p, states = light_points(123, 8 * INPUTS, top=7.0)           # (below and above the lamps: either side may emit)
    ref = R.sample_light(case.ref, count, p, states)
    lt, nwd = eval_inputs_from_samples(case, ref)
    got = probe.evaluate(case, count, lt, nwd)[:, 3].astype(np.float64)
    d = nwd[:, 6].astype(np.float64)
    tris = case.ref["lights"][ref["light"], 4].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        true = d * d / (ref["area"] * ref["cos_true"]) / tris / count
    departure = {}
    for name, light in sc.lamp_light.items():
        m = (ref["light"] == light) & (ref["cos"] >= 0.3) & (ref["cos_true"] >= 0.3)
        assert m.sum() > 200, (name, m.sum())
        rel = np.abs(got[m] / true[m] - 1)
        if name in ("nonuniform", "shear"):
            departure[name] = (float(rel.max()), float(np.median(rel)))
            assert rel.max() > 0.01, (name, rel.max())                       # the departure is there, and the value check pins its size
        else:
            assert rel.max() <= 2e-5, (name, rel.max())
    print("pdf against the true density, |pdf / true - 1| (max, median): " + ", ".join(f"{k} {a:.3f} {b:.3f}" for k, (a, b) in departure.items()))
    return departure


def test_mesh_light_pdf_is_the_true_density_under_similarity_transforms_only(probe, shading_scenes):
    check_true_density(probe, shading_scenes)


def check_tiny_lamps(probe, sc):
    """Lamps shrunk to 7.2e-7 and 1.8e-7 of area per triangle: below 1e-6 the sampler returns no radiance and no pdf;
    the evaluation applies the threshold to twice the area (QUIRK Q4), so the first lamp still evaluates (1.44e-6) and
    the second does not (3.6e-7). Bit for bit the reference's zeros; the evaluated pdf within K = 6."""
    base = sc.instances
    T = base.ref["transforms"].copy()
    lamps = {name: int(np.flatnonzero(base.ref["light_indices"] == li)[0]) for name, li in sc.lamp_light.items()}
    for name, area in (("identity", 7.2e-7), ("rigid", 1.8e-7)):
        # the rectangle is 2 x 2 scaled by (0.5, 0.4): each triangle 0.4 of area before the shrink
        T[lamps[name], :, :3] *= np.sqrt(area / 0.4)
    L = base.ref["lights"][[sc.lamp_light["identity"], sc.lamp_light["rigid"]]]
    case = base.edit(transforms=T, lights=L)
    p, states = light_points(31, 512)
    p[:, 1] = -2.0                                                   # below the lamps, which face down or up: some lit
    f, _ = probe.sample(case, 2, p, states)
    ref = R.sample_light(case.ref, 2, p, states)
    np.testing.assert_allclose(np.unique(np.round(ref["area"] * 1e7, 1)), [1.8, 7.2])
    assert (f[:, 0:3] == 0).all() and (f[:, 6] == 0).all() and (ref["pdf"] == 0).all()
    lt, nwd = eval_inputs_from_samples(case, ref)
    got = probe.evaluate(case, 2, lt, nwd)
    a = (lt[:, 0], lt[:, 1], nwd[:, 0:3], nwd[:, 3:6], nwd[:, 6])
    (c64, p64), (_, p32) = R.evaluate_light(case.ref, 2, *a, np.float64), R.evaluate_light(case.ref, 2, *a, np.float32)
    first = lt[:, 0] == 0
    lit = first & (p64 > 0)
    assert lit.sum() > 20 and (p64[~first] == 0).all() and (got[~first, 3] == 0).all()
    k = tolerance_ratio(got[:, 3], p64, p32.astype(np.float64)).max()
    assert k <= TOLERANCE_K, k


def test_lamps_below_the_area_threshold(probe, shading_scenes):
    check_tiny_lamps(probe, shading_scenes)


# ---- 5. distributions -------------------------------------------------------------------------------
def check_env_directions(probe, sc):
    """200 000 environment directions over 16 x 32 equal-solid-angle cells (z x azimuth), chi-square at 1e-6: the
    direction density is 1 / 4 pi."""
    case, _ = light_cases(sc)["environment_alone"]
    states = np.random.default_rng(8).integers(1, 1 << 32, (CHI_DRAWS, 4), dtype=np.uint64).astype(np.uint32)
    f, _ = probe.sample(case, 1, np.zeros((CHI_DRAWS, 3), np.float32), states)
    wi = f[:, 3:6].astype(np.float64)
    assert (np.abs(np.linalg.norm(wi, axis=1) - 1) < 1e-5).all()
    zi = np.minimum(((wi[:, 2] + 1) * 8).astype(np.int64), 15)
    ai = np.minimum(((np.arctan2(wi[:, 1], wi[:, 0]) + np.pi) / (2 * np.pi) * 32).astype(np.int64), 31)
    chi2, dof = chi_square(np.bincount(zi * 32 + ai, minlength=512), np.full(512, CHI_DRAWS / 512))
    print(f"env directions: chi2/dof {chi2 / dof:.3f} (dof {dof}, bound {chi_square_quantile(dof) / dof:.3f})")
    assert chi2 < chi_square_quantile(dof), (chi2, dof)
    assert (f[:, 6] == np.float32(np.float32(1) / (np.float32(4) * np.float32(np.pi)))).all()


def test_environment_directions_are_uniform(probe, shading_scenes):
    check_env_directions(probe, shading_scenes)


def locate(case, lights, x):
    """The light, triangle (index within its light) and barycentrics of world-space points on the mesh lights."""
    s = case.ref
    out_light, out_tri = np.full(len(x), -1, np.int64), np.full(len(x), -1, np.int64)
    out_uv, best = np.zeros((len(x), 2)), np.full(len(x), np.inf)
    for li in lights:
        offset, count, inst = (int(a) for a in s["lights"][li, 3:6])
        for k in range(count):
            _, W, _, _, _ = R.triangle_geometry(s, np.array([offset + k]), np.array([inst]), np.float64)
            e1, e2, n = W[0, 1] - W[0, 0], W[0, 2] - W[0, 0], np.cross(W[0, 1] - W[0, 0], W[0, 2] - W[0, 0])
            r = x - W[0, 0]
            A = np.stack([e1, e2, n / np.linalg.norm(n)], 1)
            c = np.linalg.solve(A, r.T).T
            off = np.maximum.reduce([-c[:, 0], -c[:, 1], c[:, 0] + c[:, 1] - 1, np.abs(c[:, 2])])
            take = off < best
            best = np.where(take, off, best)
            out_light[take], out_tri[take] = li, k
            out_uv[take] = c[take, :2]
    return out_light, out_tri, out_uv, best


def check_mesh_light_distribution(probe, sc):
    """200 000 draws over the five lights of the every-kind scene from one point, chi-square at 1e-6 on three levels: the
    lights (uniform: 1/5 each; told apart by the delta flag, the distance and the triangle the point lies on), the
    triangles within the six-triangle fan (uniform BY COUNT, 1/6 each whatever their areas, which differ 28-fold: the
    renderer does not pick by area), and the 16 equal-area cells of every triangle."""
    case, count = sc.lights, 5
    states = np.random.default_rng(12).integers(1, 1 << 32, (CHI_DRAWS, 4), dtype=np.uint64).astype(np.uint32)
    p = np.tile(np.array([[0.3, 0.2, -0.4]], np.float32), (CHI_DRAWS, 1))
    f, w = probe.sample(case, count, p, states)
    L = case.ref["lights"]
    kinds = R.light_kind(L)
    delta, far = w[:, 0] == 1, np.isinf(f[:, 7])
    mesh = ~delta & ~far
    x = p[mesh].astype(np.float64) + f[mesh, 3:6].astype(np.float64) * (f[mesh, 7].astype(np.float64) / (1 - float(R.SHADOW_EPSILON)))[:, None]
    meshes = np.flatnonzero(kinds == R.MESH)
    light, tri, uv, off = locate(case, meshes, x)
    assert off.max() < 1e-4, off.max()                                    # every sampled point lies on its triangle
    which = np.full(CHI_DRAWS, -1, np.int64)
    which[mesh] = light
    which[delta & ~far] = np.flatnonzero(kinds == R.POINT)[0]
    which[delta & far] = np.flatnonzero(kinds == R.DIRECTIONAL)[0]
    which[~delta & far] = np.flatnonzero(kinds == R.ENVIRONMENT)[0]
    total = [chi_square(np.bincount(which, minlength=5), np.full(5, CHI_DRAWS / 5))]
    fan = int(meshes[L[meshes, 4] == 6][0])
    in_fan = light == fan
    total.append(chi_square(np.bincount(tri[in_fan], minlength=6), np.full(6, in_fan.sum() / 6)))
    for li in meshes:
        for k in range(int(L[li, 4])):
            m = (light == li) & (tri == k)
            total.append(chi_square(np.bincount(triangle_cells(uv[m, 0], uv[m, 1]), minlength=16), np.full(16, m.sum() / 16)))
    for label, (chi2, dof) in zip(["lights", "fan triangles"] + ["cells"] * 8, total):
        print(f"mesh lights, {label}: chi2/dof {chi2 / dof:.3f} (dof {dof}, bound {chi_square_quantile(dof) / dof:.3f})")
        assert chi2 < chi_square_quantile(dof), (label, chi2, dof)


def test_mesh_light_points_are_uniform_on_three_levels(probe, shading_scenes):
    check_mesh_light_distribution(probe, shading_scenes)


# ---- 6. edge families (the device file compares them with the oracle bit for bit) -------------------
def edge_hit_records(sc, name):
    """Barycentrics +-0 and u + v = 1, and (for the textured, tiled case) texcoords on texel centres and edges, negative
    ones and ones far outside [0, 1): the corner texcoords are set so that (u, v) is the texcoord."""
    NZ = np.float32(-0.0)
    uv = [(0.0, 0.0), (NZ, 0.0), (0.0, NZ), (NZ, NZ), (1.0, 0.0), (0.0, 1.0), (0.25, 0.75), (0.5, 0.5), (1.0, NZ), (np.float32(1) - np.float32(2.0 ** -24), np.float32(2.0 ** -24))]
    if name == "texcoords":
        g = [k / 10.0 for k in range(-25, 26)] + [k / 6.0 for k in range(-9, 10)] + [-1000.3, 997.7, 65536.5, -65535.5, 0.1, 0.3, 0.5, 0.7, 0.9]
        uv = [(a, b) for a in g for b in (0.0, 1.0 / 6.0, 0.5, -1.0 / 3.0, 2.5, 1000.5)]
    tris = sc.loose_triangles[:6]
    u = np.array([a for _ in tris for a, _ in uv], np.float32)
    v = np.array([b for _ in tris for _, b in uv], np.float32)
    tri = np.repeat(tris, len(uv)).astype(np.uint32)
    return u, v, tri


def texcoord_case(sc):
    """The rigid instance with the 5 x 3 bitmap, every triangle's corner texcoords (0, 0), (1, 0), (0, 1): a record's
    (u, v) is its texcoord; tiling 1, checkerboard on."""
    base = sc.instances
    v = base.ref["vertices"].copy()
    t = base.ref["triangles"][sc.loose_triangles[:6]]
    assert len(np.unique(t)) == t.size            # (the six triangles share no vertex: loose triangles of the soup)
    v[t[:, 0], 9:11], v[t[:, 1], 9:11], v[t[:, 2], 9:11] = (0, 0), (1, 0), (0, 1)
    m = base.ref["materials"].copy()
    m[int(base.ref["overrides"][sc.soup_instance["rigid"]]), 11] |= R.ROUGHNESS_TEXTURE
    return base.edit(vertices=v, materials=m), sc.soup_instance["rigid"]


def edge_directions():
    """Directions with two or three equal largest components and with zero components, of either sign."""
    out = []
    for a in (1.0, -1.0):
        for b in (1.0, -1.0):
            for c in (0.0, -0.0, 0.5, -0.5, 1.0, -1.0):
                out += [(a, b, c), (a, c, b), (c, a, b)]
    out += [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (0.0, -0.0, 3.0), (2.0, 1e-30, -2.0)]
    return np.array(out, np.float32)


def edge_light_inputs(sc):
    """(case, count, points, states): p on a lamp triangle's plane (cos = 0 up to rounding), p equal to the point light's
    position, and first draws on every light boundary k / 5 and one 24-bit step either side of it."""
    case, count = sc.lights, 5
    L = case.ref["lights"]
    kinds = R.light_kind(L)
    bits = sorted({min(max(int(round(k * (1 << 24) / 5)) + dk, 0), (1 << 24) - 1) for k in range(6) for dk in (-1, 0, 1)})
    states = R.states_with_draw(np.repeat(bits, 8), 5)
    lamp = int(np.flatnonzero((kinds == R.MESH) & (L[:, 4] == 2))[0])
    _, W, _, _, _ = R.triangle_geometry(case.ref, np.array([int(L[lamp, 3])]), np.array([int(L[lamp, 5])]), np.float64)
    on_plane = W[0, 0] + 3.0 * (W[0, 1] - W[0, 0]) - 2.0 * (W[0, 2] - W[0, 0])
    point = L[kinds == R.POINT][0].view(np.float32)[3:6]
    p = np.tile(np.array([on_plane, point, [0.1, 0.2, 0.3], W[0, 0]], np.float32), (len(states) // 4 + 1, 1))[:len(states)]
    return case, count, p, states


def edge_camera_inputs():
    """Film samples 0 and 1 - 2^-24; aperture numbers 0, 1 - 2^-24 and, for n blades, k / n and one step either side."""
    hi = float(np.float32(1) - np.float32(2.0 ** -24))
    film = [(a, b) for a in (0.0, hi, 0.5) for b in (0.0, hi, 0.5)]
    third = sorted({0.0, hi, 0.5} | {min(max(k / n + dk * 2.0 ** -24, 0.0), hi) for n in (5, 6) for k in range(n + 1) for dk in (-1, 0, 1)})
    ap = [(a, b, c) for a in (0.0, hi, 0.5, 0.25) for b in (0.0, hi, 0.5) for c in third]
    film_all = np.array([f for f in film for _ in ap], np.float32)
    return film_all, np.array(ap * len(film), np.float32)


def test_edge_inputs_select_what_the_reference_selects(probe, shading_scenes):
    """The discrete outputs at the edge inputs: a first draw on a light boundary selects the reference's light (the delta
    flag and the number of draws the state advanced by), -0 barycentrics and corners reconstruct finite frames, film
    samples 0 and 1 - 2^-24 give unit directions, a blade number on a blade boundary the reference's blade."""
    sc = shading_scenes
    case, count, p, states = edge_light_inputs(sc)
    f, w = probe.sample(case, count, p, states)
    ref = R.sample_light(case.ref, count, p, states)
    assert (w[:, 0] == ref["delta"]).all() and (w[:, 1:] == ref["state"]).all() and len(np.unique(ref["light"])) == 5
    at_light = (p == case.ref["lights"][R.light_kind(case.ref["lights"]) == R.POINT][0].view(np.float32)[3:6]).all(1) & (ref["kind"] == R.POINT)
    assert at_light.any() and not np.isfinite(f[at_light, 3:6]).any()              # d = 0: the direction is 0 / 0
    u, v, tri = edge_hit_records(sc, "barycentrics")
    g, _ = probe.hit(sc.instances, R_records(u, v, tri, np.full(len(u), sc.soup_instance["shear"], np.uint32)))
    assert np.isfinite(g).all()
    frame = camera_frame(sc, "thin_6_blades")
    film, ap = edge_camera_inputs()
    o, d = probe.camera(frame, film, ap)
    assert np.isfinite(o).all() and (np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) < 1e-6).all()
    o64, d64, _, _ = R.camera_ray(R.frame_dict(frame), film, ap)
    assert np.abs(o - o64).max() <= 16 * EPS * np.abs(o64).max() and np.abs(d - d64).max() <= 16 * EPS
