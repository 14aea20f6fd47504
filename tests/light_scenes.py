"""The scene of the light-selection tests (tests/test_gpu_light_table.py), in the style of tests/path_scenes.py and
within the limits tests/path_ref.py lists: every part its own OBJ in world coordinates under an identity transform,
flat-shaded, at least 1e-2 from every other part, lamps far above the 1e-6 area threshold.

`lamps`: a matte floor and a two-sided blocker over it; a small bright quad lamp (0.0576 of area, luminance 175), a
large dim quad lamp (1.68, luminance 0.12) and a two-triangle kite lamp whose triangles' areas are 1 : 7 (0.015 and
0.105; luminance 1.3); a dim point light, a dim directional light and a dim constant environment: six lights. The
bright lamp gives the floor some fifty times the light of the other five together. Under uniform selection a sixth of
the light samples goes to each light and half of the kite's to its small triangle; by power the bright lamp takes
four in five (P = 0.80).

SCENES[name]: the B the scene runs at, the states of LIGHT_VISIBLE, the reference's path count (tests/light_truth.py
writes tests/golden/path_truth_lights.json from it) and the device's image count. The path count makes the
reference's standard error at most the device's on every statistic (tests/test_gpu_light_table.py asserts it)."""
import numpy as np

import path_scenes as PS
from directcomputeraytracing_amd.scenes import _sensor, _xml, mitsuba_matrix

SIZE = PS.SIZE
SEED = 20241021
SCENES = {
    "lamps": {"bounces": (0, 2), "visible": (True, False), "paths": 96 << 20, "images": 4},
}
KITE = [(-0.5, 1.3, -0.9), (-0.2, 1.3, -0.95), (0.1, 1.3, -0.9), (-0.2, 1.3, -0.55)]      # (A, B, C, D): triangles ABC 0.015, ACD 0.105


def _lamps(Scene, d, width=SIZE, height=SIZE):
    parts = {
        "floor": (PS._quad((0, 0, 0), (2, 0, 0), (0, 0, -2)), PS._diffuse("0.6, 0.5, 0.4")),
        "blocker": (PS._quad((0.2, 0.6, 0.1), (0.5, 0, 0), (0, 0, -0.4)), PS._diffuse("0.3, 0.6, 0.7", True)),
    }
    body = ""
    for name, (face, bsdf) in parts.items():
        PS._write_faces(d / f"{name}.obj", [face])
        body += PS._shape(name, bsdf)
    PS._write_faces(d / "bright.obj", [PS._quad((-0.9, 1.6, 0.3), (0.12, 0, 0), (0, 0, 0.12))])
    PS._write_faces(d / "dim.obj", [PS._quad((0.8, 1.9, -0.2), (0.7, 0, 0), (0, 0, 0.6))])
    PS._write_faces(d / "kite.obj", [(KITE, (0.0, -1.0, 0.0))])
    body += PS._shape("bright", emitter="200, 170, 130") + PS._shape("dim", emitter="0.1, 0.12, 0.16") + PS._shape("kite", emitter="1.2, 1.4, 1")
    body += ('  <emitter type="constant"><rgb name="radiance" value="0.006, 0.007, 0.01"/></emitter>\n'
             '  <emitter type="directional"><vector name="direction" value="-0.3, -0.8, 0.5"/><rgb name="irradiance" value="0.04, 0.038, 0.034"/></emitter>\n')
    camera = _sensor("perspective", width, height, mitsuba_matrix((0, 1.6, -3.0), pitch=28), '    <float name="fov" value="60"/>\n', rfilter='<rfilter type="box"/>')
    (d / "lamps.xml").write_text(_xml(PS._integrator(2) + camera + body))
    s = Scene((width, height))
    s.load_from_file(d / "lamps.xml")
    s.add_point_light((0.5, 1.5, 0.3), (0.12, 0.1, 0.08))
    return s


def load(name, directory, width=SIZE, height=SIZE):
    """The scene `name`, loaded (the tests' 64 x 64, or the film a tool asks for); max_bounce is the scene's largest B
    (path_scenes.with_case selects a case)."""
    from pathlib import Path

    from directcomputeraytracing_amd import Scene
    d = Path(directory) / name
    d.mkdir(parents=True, exist_ok=True)
    return globals()["_" + name](Scene, d, width, height)


# ---- what the tests and tools/bench_light_sampling.py share ------------------------------------------------
# The float64 prototype of test_variance_falls' ratio: light_table_ref.direct_moments (the light sample alone, no
# occlusion) at 200 seeded floor points of `lamps`, the table's variance over uniform selection's.
VARIANCE_RATIO_PROTOTYPE = 0.109


def point_lights(count, seed):
    """`count` point lights with seeded random positions and intensities (spread over four decades)."""
    rng = np.random.default_rng(seed)
    L = np.zeros((count, 7), np.uint32)
    L[:, 0:3] = (10.0 ** rng.uniform(-2, 2, (count, 1)) * rng.uniform(0.2, 1.0, (count, 3))).astype(np.float32).view(np.uint32)
    L[:, 3:6] = rng.uniform(-2, 2, (count, 3)).astype(np.float32).view(np.uint32)
    L[:, 6] = 1
    return L


def device_samples(t, images, first=0):
    out = []
    for seed in range(first, first + images):
        t.clear_film()
        t.render_images(seed, 1)
        out.append(t.read_samples()[1][..., :3].copy())
    return np.stack(out)


def floor_pixels(t):
    """The pixels of `lamps` whose footprint sees the floor alone: the camera rays through their four corners and their
    centre meet y = 0 inside the floor without crossing the blocker's rectangle at y = 0.6 (grown by 0.02)."""
    g = np.arange(2 * SIZE + 1, dtype=np.float64) / (2 * SIZE)
    X, Y = np.meshgrid(g, g, indexing="xy")
    film = np.stack([X.ravel(), Y.ravel()], 1).astype(np.float32)
    o, d = t.camera_ray_at(film, np.zeros((len(film), 3), np.float32))
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        hit = o + (-o[:, 1] / d[:, 1])[:, None] * d
        at = o + ((0.6 - o[:, 1]) / d[:, 1])[:, None] * d
    blocked = (at[:, 0] > -0.32) & (at[:, 0] < 0.72) & (at[:, 2] > -0.32) & (at[:, 2] < 0.52)
    ok = ((d[:, 1] < 0) & (np.abs(hit[:, 0]) < 1.99) & (np.abs(hit[:, 2]) < 1.99) & ~blocked).reshape(2 * SIZE + 1, 2 * SIZE + 1)
    return ok[0:-2:2, 0:-2:2] & ok[2::2, 0:-2:2] & ok[0:-2:2, 2::2] & ok[2::2, 2::2] & ok[1::2, 1::2]
