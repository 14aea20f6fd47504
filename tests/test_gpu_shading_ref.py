"""The device's camera rays, hit reconstruction, texture / environment lookups and light sampling
(dcrt_device_camera_ray / _intersection_probe / _light_sample / _light_eval / _env_lookup: the path kernels'
own generate_ray, hit_to_intersection, sample_light, evaluate_light and sample_env): every probe output bit
for bit the CPU oracle's -- at the seeded inputs, the edge families and the chi-square draws of
tests/test_shading_ref.py, in batches of 1, 63, 65, 257 and 4 000, with and without the frame table -- and
the float64 and chi-square checks of that file on the device's own numbers."""
import ctypes as C

import numpy as np
import pytest

import shading_ref as R
import test_shading_ref as T
from test_gpu_parity import same_bits
from test_shading_ref import shading_scenes  # noqa: F401 (the session's scenes)

pytestmark = pytest.mark.gpu


class DeviceProbe:
    """The probes of one tracer; a case's flat scene is uploaded when it is not the one in place."""

    def __init__(self, tracer):
        self.t, self.case = tracer, None

    def _place(self, case, light_count=None):
        if self.case is not case:
            assert self.t._lib.dcrt_tracer_upload_scene(self.t._h, C.byref(case.flat)) == 0
            self.case = case
        self.t.set_frame_params(case.frame(light_count))

    def camera(self, frame, film, ap):
        f = type(frame).from_buffer_copy(frame)
        f.light_count = 0              # (no light is read; the scene in place may hold fewer than the frame's)
        self.t.set_frame_params(f)
        return self.t.camera_ray_at(film, ap)

    def hit(self, case, records, use_table=False):
        self._place(case)
        return self.t.intersection_probe(records, use_table)

    def sample(self, case, light_count, p, states):
        self._place(case, light_count)
        return self.t.light_sample(p, states)

    def evaluate(self, case, light_count, light_triangle, nwd):
        self._place(case, light_count)
        return self.t.light_eval(light_triangle, nwd)

    def env(self, case, d):
        self._place(case)
        return self.t.env_lookup(d)


def assert_same(label, got, want):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    for k, (g, w) in enumerate(zip(got, want)):
        ok = same_bits(g, w) if g.dtype == np.float32 else (g == w)
        assert ok.all(), (label, k, int((~ok).sum()), np.argwhere(~ok)[:3].tolist(), g[~ok][:3].tolist(), w[~ok][:3].tolist())


class BothProbe:
    """The device's outputs, each compared with the oracle's bit for bit (a NaN matches a NaN) on the way."""

    def __init__(self, device, oracle):
        self.device, self.oracle, self.calls = device, oracle, 0

    def _both(self, name, *args):
        got, want = getattr(self.device, name)(*args), getattr(self.oracle, name)(*args)
        assert_same(name, got, want)
        self.calls += 1
        return got

    def camera(self, *a):
        return self._both("camera", *a)

    def hit(self, *a):
        return self._both("hit", *a)

    def sample(self, *a):
        return self._both("sample", *a)

    def evaluate(self, *a):
        return self._both("evaluate", *a)

    def env(self, *a):
        return self._both("env", *a)


@pytest.fixture(scope="module")
def probe(native_lib, golden_luts, oracle_mod):
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=1 << 14, iterations_per_render=8)
    t.set_luts(golden_luts)
    yield BothProbe(DeviceProbe(t), T.OracleProbe(oracle_mod))
    t.destroy()


# ---- the float64 and chi-square checks on the device's numbers, every output compared with the oracle's ----
@pytest.mark.parametrize("name", T.CAMERA_CASES)
def test_camera_rays(probe, shading_scenes, name):
    frame = T.camera_frame(shading_scenes, name)
    T.check_camera_values(probe, frame, name)
    if name != "pinhole":
        T.check_thin_lens_focus(probe, frame, name)
    film, ap = T.edge_camera_inputs()       # film samples 0 and 1 - 2^-24, aperture numbers on blade boundaries
    o, d = probe.camera(frame, film, ap)
    assert np.isfinite(o).all() and np.isfinite(d).all()


@pytest.mark.parametrize("name", ["thin_disk", "thin_5_blades", "thin_6_blades"])
def test_aperture_points_are_uniform_over_the_shape(probe, shading_scenes, name):
    T.check_aperture_distribution(probe, T.camera_frame(shading_scenes, name), name)


@pytest.mark.parametrize("name", T.HIT_CASES)
def test_hit_reconstruction(probe, shading_scenes, name):
    T.check_hit_values(probe, shading_scenes, name)


def test_hit_reconstruction_with_and_without_the_frame_table(probe, shading_scenes):
    """The every-kind scene has one instance per mesh, so the frame table is built for it: the form of the hit reconstruction that
    takes it and the per-hit form give the oracle's bits at 4 000 records of the soup and at the +-0 and corner
    barycentrics."""
    sc = shading_scenes
    case = sc.lights
    inst = int(np.flatnonzero(case.ref["light_indices"] == T.INVALID)[0])
    tris = np.arange(int(case.ref["lights"][R.light_kind(case.ref["lights"]) == R.MESH][:, 3].min()))
    P = case.ref["vertices"][case.ref["triangles"][tris]][..., :3].astype(np.float64)
    tris = tris[np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1) > 1e-6]
    u, v, tri, insts = T.hit_inputs(77, tris, inst)
    eu, ev, etri = T.edge_hit_records(sc, "barycentrics")
    etri = tris[:6].astype(np.uint32)[np.arange(len(etri)) % 6]
    rec = np.concatenate([T.R_records(u, v, tri, insts), T.R_records(eu, ev, etri, np.full(len(eu), inst, np.uint32))])
    assert sc.scene_b.triangle_instances()[0]           # (the table is built for such a scene, whichever variant MATERIAL takes)
    on, off = probe.hit(case, rec, True), probe.hit(case, rec, False)
    assert_same("table on / off", on, off)
    # the six-times-instanced soup has none: the table form is refused
    from directcomputeraytracing_amd import DCRTError
    with pytest.raises(DCRTError):
        probe.device.hit(sc.instances, rec[:1] * 0, True)


def test_environment_lookup(probe, shading_scenes):
    T.check_env_values(probe, shading_scenes)
    d = T.edge_directions()             # two or three equal largest components, zero components
    got = probe.env(shading_scenes.lights, d)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("name", T.LIGHT_CASES)
def test_light_sampling_and_evaluation(probe, shading_scenes, name):
    T.check_light_sample_values(probe, shading_scenes, name)
    T.check_light_eval_values(probe, shading_scenes, name)


def test_sampler_evaluation_consistency_true_density_and_tiny_lamps(probe, shading_scenes):
    T.check_sampler_against_evaluation(probe, shading_scenes)
    T.check_true_density(probe, shading_scenes)
    T.check_tiny_lamps(probe, shading_scenes)


def test_inputs_aimed_at_the_discontinuities_match_one_side(probe, shading_scenes):
    T.test_texcoords_on_checker_edges_are_classified_and_match_one_side(probe, shading_scenes)
    T.test_points_on_a_lamps_plane_are_classified_and_match_one_side(probe, shading_scenes)


def test_environment_directions_are_uniform(probe, shading_scenes):
    T.check_env_directions(probe, shading_scenes)


def test_mesh_light_points_are_uniform_on_three_levels(probe, shading_scenes):
    T.check_mesh_light_distribution(probe, shading_scenes)


# ---- edge families: bit for bit the oracle's (BothProbe compares), no float64 reference ----------------
def test_edge_barycentrics_and_texcoords(probe, shading_scenes):
    """u, v = +-0, corners and u + v = 1 under every transform; texcoords on texel centres and edges of the 5 x 3 bitmap,
    negative ones and ones far outside [0, 1) (wrap), with the checkerboard on."""
    sc = shading_scenes
    u, v, tri = T.edge_hit_records(sc, "barycentrics")
    for name, inst in sc.soup_instance.items():
        for back in (0, 1 << 31):
            probe.hit(sc.instances, T.R_records(u, v, tri | np.uint32(back), np.full(len(u), inst, np.uint32)))
    case, inst = T.texcoord_case(sc)
    u, v, tri = T.edge_hit_records(sc, "texcoords")
    f, _ = probe.hit(case, T.R_records(u, v, tri, np.full(len(u), inst, np.uint32)))
    assert np.isfinite(f[:, 12:16]).all() and len(np.unique(f[:, 15])) == 2      # both checker cells


def test_edge_light_inputs(probe, shading_scenes):
    """p on a lamp's plane, p equal to the point light's position, first draws on every light boundary and one step either
    side; then second draws (the triangle selection) on the fan's triangle boundaries k / 6."""
    sc = shading_scenes
    case, count, p, states = T.edge_light_inputs(sc)
    f, w = probe.sample(case, count, p, states)
    lt, nwd = T.eval_inputs_from_samples(case, R.sample_light(case.ref, count, p, states))
    nwd[:, 3:6] = np.nan_to_num(f[:, 3:6])
    probe.evaluate(case, count, lt, nwd)
    fan, _ = T.light_cases(sc)["fan_alone"]
    bits = sorted({min(max(int(round(k * (1 << 24) / 6)) + dk, 0), (1 << 24) - 1) for k in range(7) for dk in (-1, 0, 1)})
    states = R.states_with_draw(np.repeat(bits, 4), 17, which=1)
    ref = R.sample_light(fan.ref, 1, np.zeros((len(states), 3), np.float32), states)
    assert len(np.unique(ref["triangle"])) == 6 and ((ref["draws"][:, 1] * 6) % 1 == 0).any()
    probe.sample(fan, 1, np.tile(np.array([[0.1, 0.2, 0.3]], np.float32), (len(states), 1)), states)


# ---- batch sizes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_batch_sizes(probe, shading_scenes, n):
    """Batches that end inside a wave, one past it and one past a workgroup: the first n items of the 4 000-item inputs give
    the first n results (BothProbe compares each with the oracle's)."""
    sc = shading_scenes
    frame = T.camera_frame(sc, "turned_6_blades")
    film, ap = T.numbers(1, (T.INPUTS, 2)), T.numbers(2, (T.INPUTS, 3))
    assert_same("camera", tuple(a[:n] for a in probe.camera(frame, film, ap)), probe.camera(frame, film[:n], ap[:n]))
    u, v, tri, insts = T.hit_inputs(3, sc.solid_triangles, sc.soup_instance["shear"])
    rec = T.R_records(u, v, tri, insts)
    assert_same("hit", tuple(a[:n] for a in probe.hit(sc.instances, rec)), probe.hit(sc.instances, rec[:n]))
    p, states = T.light_points(4)
    full = probe.sample(sc.lights, 5, p, states)
    assert_same("sample", tuple(a[:n] for a in full), probe.sample(sc.lights, 5, p[:n], states[:n]))
    lt, nwd = T.eval_inputs_from_samples(sc.lights, R.sample_light(sc.lights.ref, 5, p, states))
    assert_same("evaluate", probe.evaluate(sc.lights, 5, lt, nwd)[:n], probe.evaluate(sc.lights, 5, lt[:n], nwd[:n]))
    d = T.sphere(5, T.INPUTS)
    assert_same("env", probe.env(sc.lights, d)[:n], probe.env(sc.lights, d[:n]))


def test_indices_outside_the_scene_are_refused(probe, shading_scenes):
    """A triangle, instance or light index past the scene's, and a state whose draws select past the lights, come back as
    errors before anything is launched; a count of 0 is served."""
    from directcomputeraytracing_amd import DCRTError
    sc, dev = shading_scenes, probe.device
    case = sc.lights
    T_, I, Ln = case.flat.triangle_count, case.flat.instance_count, case.flat.light_count
    for rec in ([0, 0, T_, 0], [0, 0, 0, I], [0, 0, T_ | (1 << 31), 0]):
        with pytest.raises(DCRTError):
            dev.hit(case, np.array([rec], np.uint32))
    for lt in ([Ln, 0], [0, T_]):
        with pytest.raises(DCRTError):
            dev.evaluate(case, Ln, np.array([lt], np.uint32), np.zeros((1, 7), np.float32))
    f, w = dev.hit(case, np.zeros((0, 4), np.uint32))
    assert f.shape == (0, 16) and w.shape == (0, 3)
    assert dev.env(case, np.zeros((0, 3), np.float32)).shape == (0, 3)
    no_cube = case.edit(lights=case.ref["lights"])
    no_cube.flat.env_cube_rgb, no_cube.flat.env_cube_size = None, 0
    with pytest.raises(DCRTError):
        dev.env(no_cube, np.ones((1, 3), np.float32))
