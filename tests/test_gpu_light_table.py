"""Power-proportional light selection on the device (include/dcrt.h, "light selection") against
tests/light_table_ref.py: the table the upload builds, the sampler and the evaluator through the light probes, the
distribution of 200 000 draws over lights and lamp triangles, the renderer's mean on the `lamps` scene against
tests/golden/path_truth_lights.json (wavefront and megakernel), its variance against uniform selection, and the
plumbing of the mode."""
import copy
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import light_scenes as LS
import light_table_ref as LT
import light_truth
import path_ref as PR
import path_scenes as PS
import shading_ref as R
import test_shading_ref as T
from ref_tolerance import TOLERANCE_K, TOLERANCE_ULPS, chi_square_quantile, tolerance_ratio
from test_gpu_parity import same_bits
from test_path_ref import NAN_CAP, within, z_bound
from test_shading_ref import shading_scenes  # noqa: F401 (the session's scenes)

pytestmark = pytest.mark.gpu

STATES = 4000
CHI_DRAWS = LT.CHI_DRAWS     # 200 000
# The per-sample luminance variance over the floor's pixels of `lamps` at B = 0, power selection over uniform selection:
# measured on an MI355X, power 0.03276 over uniform 0.06087 (profiles/light_sampling_costs.txt). Uniform selection's samples are
# about half as bright on this scene -- its sampler reports twice the density it draws a lamp's point from (shading QUIRK Q3),
# which this mode does not -- so its variance is a quarter of an unbiased estimator's; the float64 prototype of the direct estimator alone
# (light_table_ref.direct_moments at 200 seeded floor points, no occlusion, the light sample only) gives VARIANCE_RATIO_PROTOTYPE.
# The bound is twice the measured ratio, as test_gpu_env_importance.test_variance_falls has it.
VARIANCE_RATIO_MEASURED = 0.5381
VARIANCE_RATIO_PROTOTYPE = LS.VARIANCE_RATIO_PROTOTYPE     # 0.109


@pytest.fixture(scope="module")
def tracer(native_lib, golden_luts):
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=1 << 16, iterations_per_render=8)
    t.set_luts(golden_luts)
    yield t
    t.destroy()


def place(t, case, mode, light_count=None):
    assert t._lib.dcrt_tracer_upload_scene(t._h, C.byref(case.flat)) == 0
    t.set_light_sampling(mode)               # (on an uploaded scene; it outlives the next upload)
    t.env_cube_size = int(case.flat.env_cube_size) if case.flat.env_cube_rgb else 0
    t.set_frame_params(case.frame(light_count))


def ulps_apart(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


def root_radius(flat):
    """R as the definition takes it: half the diagonal of the BVH root's float32 box, in float64."""
    lo, hi = np.array(flat.bvh_nodes[0].bbox_min[:], np.float64), np.array(flat.bvh_nodes[0].bbox_max[:], np.float64)
    return LT.scene_radius(lo, hi)


def device_table(t, case):
    """(the device's arrays, the reference Table for the library's own R, a copy of it carrying the device's arrays)."""
    d = t.light_distribution()
    ref = LT.Table(case.ref, d["radius"])
    dev = copy.copy(ref)
    dev.light_prob, dev.light_cdf, dev.tri_prob, dev.tri_cdf = d["light_prob"], d["light_cdf"], d["tri_prob"], d["tri_cdf"]
    return d, ref, dev


def check_table(t, case, label):
    """All five arrays within 2 float32 ulps of the float64 reference rounded to float32 -- the bound
    test_gpu_env_importance.py holds the environment table to, for the same reason: float64 sums that differ from the
    reference's by their order alone, one rounding -- with the library's reported R as the reference's input; tri_base
    exact; the last entry of every CDF exactly 1."""
    assert t.light_sampling() == ("power", True), label
    d, ref, _ = device_table(t, case)
    assert ref.active and d["n"] == ref.n and d["entries"] == ref.entries
    assert (d["tri_base"] == ref.tri_base).all()
    worst = {}
    for key in ("light_prob", "light_cdf", "tri_prob", "tri_cdf"):
        got, want = d[key], getattr(ref, key)
        assert got.shape == want.shape and np.isfinite(got).all(), key
        worst[key] = float(ulps_apart(got, want).max()) if got.size else 0.0
    print(f"{label}: n {ref.n}, E {ref.entries}, R {d['radius']:.6f}, total {d['total_weight']:.6g}, ulps {worst}, build {t.light_table_build_ms():.3f} ms")
    assert max(worst.values()) <= 2, (label, worst)
    assert abs(d["total_weight"] / ref.total - 1) < 1e-12
    assert d["light_cdf"][-1] == 1 and (np.diff(d["light_cdf"]) >= 0).all()
    for l in np.flatnonzero(ref.tri_count > 0):
        b, c = int(ref.tri_base[l]), int(ref.tri_count[l])
        assert d["tri_cdf"][b + c - 1] == (1 if ref.A[l] > 0 else 0) and (np.diff(d["tri_cdf"][b:b + c]) >= 0).all()
    return d, ref


# ---- 1. the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lights", "instances"])
def test_table_matches_the_float64_reference(tracer, shading_scenes, name):
    case = getattr(shading_scenes, name)
    place(tracer, case, "power")
    d, _ = check_table(tracer, case, name)
    # R is the root's box as uploaded (its formula restated here), and that box holds the float64 box of the instanced
    # triangles: a TLAS leaf's box is the box of the eight transformed corners of its BLAS's box, which contains the
    # instance's triangles and, for a turned instance, more -- at most sqrt(3) times the diagonal. Measured on the CPU on
    # these scenes, float32 box arithmetic included: R / R64 = 1.1384 (lights) and 1.0299 (instances). Below, the root
    # may fall short of the float64 box by float32 rounding alone: 4 roundings of a coordinate of up to 2 R, 8 * 2^-23.
    assert d["radius"] == root_radius(case.flat)
    r64 = LT.scene_radius(*LT.float64_bounds(case.flat))
    print(f"{name}: R {d['radius']:.9f}, float64 box {r64:.9f}, ratio {d['radius'] / r64:.6f}")
    assert 1 - 8 * 2.0 ** -23 <= d["radius"] / r64 <= np.sqrt(3.0)


@pytest.mark.parametrize("count", [2, 256, 257, 1000])
def test_point_light_tables_across_the_chunk_carry(tracer, shading_scenes, count):
    """n = 2, 256, 257 and 1000 point lights: the light-level kernel's scan in chunks of 256 with a carry."""
    case = shading_scenes.lights.edit(lights=LS.point_lights(count, 40 + count))
    place(tracer, case, "power")
    check_table(tracer, case, f"{count} point lights")


def test_one_lamp_alone_has_a_table(tracer, shading_scenes):
    case, _ = T.light_cases(shading_scenes)["fan_alone"]
    place(tracer, case, "power")
    d, ref = check_table(tracer, case, "the fan alone")
    assert d["n"] == 1 and d["entries"] == 6 and d["light_prob"][0] == 1


@pytest.fixture(scope="module")
def fans(native_lib, tmp_path_factory):
    """name -> Case: a floor and one lamp of 65, of 130 unequal triangles around one vertex (angles and radii seeded)."""
    from directcomputeraytracing_amd import Scene
    from directcomputeraytracing_amd.scenes import _xml
    out = {}
    for count in (65, 130):
        d = tmp_path_factory.mktemp(f"fan{count}")
        rng = np.random.default_rng(count)
        ang = np.concatenate([[0.0], np.cumsum(rng.uniform(0.01, 0.08, count))])
        rad = rng.uniform(0.3, 1.0, count + 1)
        rim = np.stack([rad * np.cos(ang), np.full(count + 1, 1.5), rad * np.sin(ang)], 1)
        faces = [([(0.0, 1.5, 0.0), tuple(rim[k]), tuple(rim[k + 1])], (0.0, -1.0, 0.0)) for k in range(count)]
        PS._write_faces(d / "fan.obj", faces)
        PS._write_faces(d / "floor.obj", [PS._quad((0, 0, 0), (2, 0, 0), (0, 0, -2))])
        body = PS._integrator(1) + PS._camera((0, 1.0, -3.0), pitch=10, fov=60) + PS._shape("floor", PS._diffuse("0.6, 0.5, 0.4")) + PS._shape("fan", emitter="3, 4, 5")
        (d / "fan.xml").write_text(_xml(body))
        s = Scene((PS.SIZE, PS.SIZE))
        s.load_from_file(d / "fan.xml")
        s.add_point_light((0.5, 1.0, 0.3), (1.0, 1.0, 1.0))
        out[count] = T.Case(s.flat(), s.frame_params(0), [s])
    return out


@pytest.mark.parametrize("count", [65, 130])
def test_lamp_fans_across_the_wave_carry(tracer, fans, count):
    """A lamp of 65 and of 130 unequal triangles: the per-light scan in chunks of 64 entries with a carry."""
    case = fans[count]
    place(tracer, case, "power")
    d, ref = check_table(tracer, case, f"fan of {count}")
    assert d["entries"] == count and ref.areas.max() / ref.areas.min() > 5


def test_degenerate_light_sets_stay_uniform(tracer, shading_scenes):
    """Zero-radiance lights, and one point light alone: the mode is on and no table stands; sampling is the uniform
    selection's, bit for bit."""
    from directcomputeraytracing_amd import DCRTError
    L = shading_scenes.lights.ref["lights"].copy()
    dark = L.copy()
    dark[:, 0:3] = 0
    point, _ = T.light_cases(shading_scenes)["point_alone"]
    p, states = T.light_points(3, 257)
    for label, case in (("dark", shading_scenes.lights.edit(lights=dark)), ("one point light", point)):
        place(tracer, case, "uniform")
        want = tracer.light_sample(p, states)
        place(tracer, case, "power")
        assert tracer.light_sampling() == ("power", False), label
        with pytest.raises(DCRTError):
            tracer.light_distribution()
        got = tracer.light_sample(p, states)
        assert same_bits(got[0], want[0]).all() and (got[1] == want[1]).all(), label
    tracer.set_light_sampling("uniform")


# ---- 2. sampler and evaluator -----------------------------------------------------------------------------
def allowance(ref64, ref32):
    """What ref_tolerance.tolerance_ratio allows an element at K = TOLERANCE_K: K e + TOLERANCE_ULPS ulps, e the float32
    run's own error but no less than the case's 99th-percentile relative float32 error times |ref64|."""
    err32 = np.abs(ref32 - ref64)
    floor = np.percentile(err32 / np.abs(ref64), 99)
    return TOLERANCE_K * np.maximum(err32, floor * np.abs(ref64)) + TOLERANCE_ULPS * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


SAMPLE_CASES = {"lights": 61, "instances": 62}      # name -> the seed of its points and states


def sample_inputs(name):
    return T.light_points(SAMPLE_CASES[name], STATES, top=1.2)


@pytest.mark.parametrize("name", list(SAMPLE_CASES))
def test_sampler_and_evaluator(tracer, shading_scenes, name):
    """4 000 states per scene through dcrt_device_light_sample, the two searches restated on the table read back: the
    draws taken are the kind's (1, 4 or 3); a point, directional or environment light reports lightProb[l] times its
    kind's factor, bit for bit; for a lamp the sampler's pdf and the evaluator's -- at the sampler's own wi with the
    reference's normal and unscaled distance -- both lie within the rule of ref_tolerance.py of the float64 density,
    and so does their ratio of 1 (with the mode off it is 2, which the existing tests pin). Inputs whose cos is within
    rounding of 0 (the existing classifier) are left out, at most 1 %."""
    case = getattr(shading_scenes, name)
    count = len(case.ref["lights"])
    p, states = sample_inputs(name)
    place(tracer, case, "power", count)
    f, w = tracer.light_sample(p, states)
    _, _, dev = device_table(tracer, case)
    r64 = LT.sample_light(case.ref, dev, p, states, np.float64)
    r32 = LT.sample_light(case.ref, dev, p, states, np.float32)
    li, kind = r64["light"], r64["kind"]
    assert len(np.unique(li)) == count
    assert (w[:, 0] == r64["delta"]).all() and (w[:, 1:] == r64["state"]).all()             # 1, 1, 4 or 3 draws
    delta = r64["delta"]
    assert same_bits(f[delta, 6], dev.light_prob[li[delta]]).all()
    env = kind == R.ENVIRONMENT
    sphere = np.float32(np.float32(1) / (np.float32(4) * np.float32(np.pi)))
    assert same_bits(f[env, 6], sphere * dev.light_prob[li[env]]).all()
    mesh = kind == R.MESH
    assert mesh.sum() > 300
    # the lamps: the triangle the device drew is the restated search's (its point lies on it)
    x = p[mesh].astype(np.float64) + f[mesh, 3:6].astype(np.float64) * (f[mesh, 7].astype(np.float64) / (1 - float(R.SHADOW_EPSILON)))[:, None]
    np.testing.assert_allclose(x, r64["point"][mesh], atol=2e-5)
    cos_amb, _, _, _ = T.light_ambiguity(r64, p)
    lit = mesh & ~cos_amb & (r64["pdf"] > 0)
    dark = mesh & ~cos_amb & (r64["pdf"] == 0)
    left_out = (mesh & cos_amb).sum() / mesh.sum()
    assert left_out <= 0.01, left_out
    assert lit.sum() > 200 and (f[dark, 6] == 0).all() and (f[dark, 0:3] == 0).all() and (f[lit, 6] > 0).all()
    inst = case.ref["lights"][li[mesh], 5].astype(np.int64)
    normal = np.zeros((len(p), 3))
    normal[mesh] = R.triangle_geometry(case.ref, r64["triangle"][mesh], inst, np.float64)[3]
    dist = np.where(np.isinf(r64["distance"]), 1.0, r64["distance"] / (1 - float(R.SHADOW_EPSILON)))
    nwd = np.concatenate([normal, f[:, 3:6].astype(np.float64), dist[:, None]], 1).astype(np.float32)
    lt = np.stack([li, np.where(mesh, r64["triangle"], 0)], 1).astype(np.uint32)
    ev = tracer.light_eval(lt, nwd)
    a = (lt[:, 0], lt[:, 1], nwd[:, 0:3], nwd[:, 3:6], nwd[:, 6])
    (c64, e64), (_, e32) = LT.evaluate_light(case.ref, dev, *a, np.float64), LT.evaluate_light(case.ref, dev, *a, np.float32)
    assert (ev[delta] == 0).all() and same_bits(ev[env, 3], f[env, 6]).all()
    assert same_bits(ev[lit, 0:3], f[lit, 0:3]).all()
    ks = tolerance_ratio(f[lit, 6], r64["pdf"][lit], r32["pdf"][lit].astype(np.float64), TOLERANCE_ULPS).max()
    ke = tolerance_ratio(ev[lit, 3], e64[lit], e32[lit].astype(np.float64), TOLERANCE_ULPS).max()
    # ... and so their ratio is 1 -- the float64 densities' own ratio, which carries the rounding of the evaluator's inputs --
    # within what the rule allows the two together: (K e_s + ulps) / pdf_s + (K e_e + ulps) / pdf_e, first order
    ratio = f[lit, 6].astype(np.float64) / ev[lit, 3].astype(np.float64)
    want = r64["pdf"][lit] / e64[lit]
    allowed = allowance(r64["pdf"][lit], r32["pdf"][lit].astype(np.float64)) / r64["pdf"][lit] + allowance(e64[lit], e32[lit].astype(np.float64)) / e64[lit]
    kr = (np.abs(ratio - want) / (allowed * want)).max()
    print(f"{name}: lamps {mesh.sum()}, lit {lit.sum()}, left out {left_out:.4%}, K needed: sampler {ks:.3f}, evaluator {ke:.3f}; "
          f"sampler / evaluator {ratio.min():.7f} .. {ratio.max():.7f}, the largest share of its allowance {kr:.3f}")
    assert ks <= TOLERANCE_K and ke <= TOLERANCE_K, (ks, ke)
    assert kr <= 1, (kr, ratio.min(), ratio.max())
    tracer.set_light_sampling("uniform")


# ---- 3. the distribution ----------------------------------------------------------------------------------
CHI_POINT = (0.3, 0.2, -0.4)


def drawn_counts(t, case, ref):
    """Draws per bin: the light by the delta flag and the distance, a lamp's triangle by the point's place
    (test_shading_ref.locate, the helper check_mesh_light_distribution uses)."""
    states = np.random.default_rng(12).integers(1, 1 << 32, (CHI_DRAWS, 4), dtype=np.uint64).astype(np.uint32)
    p = np.tile(np.array([CHI_POINT], np.float32), (CHI_DRAWS, 1))
    f, w = t.light_sample(p, states)
    kinds = ref.kind
    delta, far = w[:, 0] == 1, np.isinf(f[:, 7])
    mesh = ~delta & ~far
    x = p[mesh].astype(np.float64) + f[mesh, 3:6].astype(np.float64) * (f[mesh, 7].astype(np.float64) / (1 - float(R.SHADOW_EPSILON)))[:, None]
    light, tri, _, off = T.locate(case, np.flatnonzero(kinds == R.MESH), x)
    assert off.max() < 1e-4, off.max()
    counts = {}
    for k, m in ((R.POINT, delta & ~far), (R.DIRECTIONAL, delta & far), (R.ENVIRONMENT, ~delta & far)):
        if (kinds == k).any():
            counts[(int(np.flatnonzero(kinds == k)[0]), -1)] = int(m.sum())
        else:
            assert not m.any()
    for l, k in zip(*np.unique(np.stack([light, tri]), axis=1)):
        counts[(int(l), int(k))] = int(((light == l) & (tri == k)).sum())
    return counts


def chi_square(counts, expected):
    keys = sorted(expected)
    c, e = np.array([counts.get(k, 0) for k in keys], np.float64), np.array([expected[k] for k in keys])
    assert set(counts) <= set(keys) and c.sum() == CHI_DRAWS
    return float(((c - e) ** 2 / e).sum()), len(keys) - 1


@pytest.mark.parametrize("name", ["lights", "instances"])
def test_draws_follow_the_table(tracer, shading_scenes, name):
    """200 000 draws from one point, counted per light and, on the lamps, per triangle: chi-square at CHI_Z against
    N P(l) P(t | l) of the float64 reference (the smallest expected count is at least 20). Uniform selection fails it."""
    case = getattr(shading_scenes, name)
    count = len(case.ref["lights"])
    place(tracer, case, "power", count)
    _, ref, _ = device_table(tracer, case)
    expected = LT.expected_counts(ref, CHI_DRAWS)
    assert min(expected.values()) >= 20, min(expected.values())
    chi2, dof = chi_square(drawn_counts(tracer, case, ref), expected)
    place(tracer, case, "uniform", count)
    uniform, _ = chi_square(drawn_counts(tracer, case, ref), expected)
    print(f"{name}: chi2 {chi2:.1f}, dof {dof}, bound {chi_square_quantile(dof):.1f}, smallest expected count {min(expected.values()):.1f}; uniform selection {uniform:.0f}")
    assert chi2 < chi_square_quantile(dof), (chi2, dof)
    assert uniform > 10 * chi_square_quantile(dof), uniform


# ---- 4., 5. the renderer ----------------------------------------------------------------------------------
def lamp_cases():
    spec = LS.SCENES["lamps"]
    return [(vis, b) for vis in spec["visible"] for b in spec["bounces"]]


def comparisons():
    """The statistical comparisons of this file: both modes of every case of `lamps` (4 quadrants x 3 channels), and the
    all-on render against the table-only one."""
    return 2 * len(lamp_cases()) * 12 + 12


@pytest.mark.parametrize("mode", ["wavefront", "megakernel"])
def test_renderer_means_are_the_rendering_equations(native_lib, golden_luts, tmp_path, mode):
    """`lamps` at B = 0 and 2, LIGHT_VISIBLE on and off, 64 x 64: the quadrant means of the device's samples under power
    selection against tests/golden/path_truth_lights.json -- path_ref.py with mis_model=False: the light sampler
    reports the density it draws from, so the pair is unbiased -- by `within` and z_bound of test_path_ref.py, z from
    this file's own number of comparisons. The fixture's standard error is at most the device's."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    fixture = light_truth.load_fixture()
    assert fixture["scenes"]["lamps"]["paths"] == LS.SCENES["lamps"]["paths"]
    scene = LS.load("lamps", tmp_path)
    z = z_bound(comparisons())
    t = WavefrontPathTracer(path_pool_size=1 << 16)
    try:
        t.set_luts(golden_luts)
        for vis, b in lamp_cases():
            PS.with_case(scene, b, vis)
            t.on_scene_loaded(scene)
            t.set_mode(mode)
            t.set_light_sampling("power")
            assert t.light_sampling() == ("power", True)
            mean, sem, _, nan = PR.quadrant_statistics(LS.device_samples(t, LS.SCENES["lamps"]["images"]))
            want, want_sem = PR.fixture_entry(fixture, "lamps", vis, b)
            ok, worst = within(mean, sem, want, want_sem, z)
            ratio = float((want_sem[sem > 0] / sem[sem > 0]).max())
            print("lamps", mode, "visible" if vis else "hidden", "B", b, "mean", mean.mean(0).round(5), "sem", sem.max(0).round(5), "NaN share", nan,
                  "worst |difference| / bound", round(worst, 3), "sem ratio fixture / device", round(ratio, 3))
            assert nan <= NAN_CAP, (mode, vis, b, nan)
            assert ratio <= 1.0, (mode, vis, b, ratio)
            assert ok, (mode, vis, b, worst, mean, want)
    finally:
        t.destroy()


def test_variance_falls(native_lib, golden_luts, tmp_path):
    """`lamps` at B = 0, 32 images in both modes: the sample variance of the luminance over the floor's pixels under
    power selection against uniform selection's. Whatever the measurement, the ratio is below 1; and it is below twice
    the ratio measured on an MI355X."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    scene = PS.with_case(LS.load("lamps", tmp_path), 0, True)
    lum = np.array([0.299, 0.587, 0.114])
    var = {}
    t = WavefrontPathTracer(path_pool_size=1 << 16)
    try:
        t.set_luts(golden_luts)
        t.on_scene_loaded(scene)
        floor = LS.floor_pixels(t)
        assert floor.mean() > 0.3, floor.mean()
        for s in ("power", "uniform"):
            t.set_light_sampling(s)
            v = LS.device_samples(t, 32)
            var[s] = float((v[:, floor, :].reshape(-1, 3).astype(np.float64) @ lum).var())
    finally:
        t.destroy()
    ratio = var["power"] / var["uniform"]
    print(f"variance over {int(floor.sum())} floor pixels: power {var['power']:.5f}, uniform {var['uniform']:.5f}, ratio {ratio:.5f} "
          f"(measured {VARIANCE_RATIO_MEASURED}, float64 prototype {VARIANCE_RATIO_PROTOTYPE})")
    assert ratio < 1, ratio
    assert VARIANCE_RATIO_MEASURED is not None and ratio < 2 * VARIANCE_RATIO_MEASURED, ratio


# ---- 6. plumbing ------------------------------------------------------------------------------------------
def test_mode_off_is_the_oracles_film(native_lib, oracle_mod, golden_luts, tmp_path):
    """A tracer that had the mode on and off again renders the samples of the oracle, which never heard of it, bit
    for bit; the setter refuses what it should."""
    from directcomputeraytracing_amd import DCRTError, WavefrontPathTracer
    scene = PS.with_case(LS.load("lamps", tmp_path), 2, True)
    t = WavefrontPathTracer(path_pool_size=1 << 16, debug_rng=True)
    try:
        t.set_luts(golden_luts)
        with pytest.raises(DCRTError):           # (the mode is set on an uploaded scene, like the scene edits)
            t.set_light_sampling("power")
        t.on_scene_loaded(scene, frame_seed=1)
        assert t.light_sampling() == ("uniform", False)
        with pytest.raises(DCRTError):
            t.light_distribution()
        assert t._lib.dcrt_tracer_set_light_sampling(t._h, 2) != 0 and t.light_sampling() == ("uniform", False)
        want = oracle_mod.render(oracle_mod.flat_with_own_bvh(scene), golden_luts, oracle_mod.frame_params(scene, 1), oracle_mod.WAVEFRONT)[1]
        t.clear_film()
        t.render_images(1, 1)
        assert same_bits(t.read_samples()[1], want).all()
        # off -> on -> off: one graph drop per toggle, the uniform samples bit for bit the oracle's again
        drops = t.upload_stats()["graph_invalidations"]
        t.set_light_sampling("power")
        assert t.upload_stats()["graph_invalidations"] == drops + 1 and t.light_sampling() == ("power", True)
        t.set_light_sampling("power")
        assert t.upload_stats()["graph_invalidations"] == drops + 1
        t.clear_film()
        t.render_images(1, 1)
        lit = t.read_samples()[1].copy()
        assert np.isfinite(lit).all() and not same_bits(lit, want).all()
        t.set_light_sampling("uniform")
        assert t.upload_stats()["graph_invalidations"] == drops + 2
        t.clear_film()
        t.render_images(1, 1)
        assert same_bits(t.read_samples()[1], want).all()
    finally:
        t.destroy()


def test_uploads_edits_and_frames(native_lib, golden_luts, tmp_path):
    """The mode survives upload_scene; a colour edit through update_lights changes lightProb as the reference says and
    drops no graph; a light added or removed rebuilds the table and drops the graphs once; a frame with another
    light_count is refused while a table stands and accepted while none does."""
    from directcomputeraytracing_amd import DCRTError, WavefrontPathTracer
    scene = PS.with_case(LS.load("lamps", tmp_path / "a"), 0, True)
    t = WavefrontPathTracer(path_pool_size=1 << 16)

    def reference():
        flat = scene.flat()
        return LT.Table(R.from_flat(flat), t.light_distribution()["radius"])

    def agrees():
        d, ref = t.light_distribution(), reference()
        return d["n"] == ref.n and all(ulps_apart(d[k], getattr(ref, k)).max() <= 2 for k in ("light_prob", "light_cdf", "tri_prob", "tri_cdf"))

    try:
        t.set_luts(golden_luts)
        t.on_scene_loaded(scene)
        t.set_light_sampling("power")
        other = PS.with_case(LS.load("lamps", tmp_path / "b"), 0, True)
        t.on_scene_loaded(other)                                # the mode survives an upload
        assert t.light_sampling() == ("power", True) and agrees()
        t.clear_film()
        t.render_images(0, 1)
        before = t.light_distribution()
        drops = t.upload_stats()["graph_invalidations"]
        # a colour edit: the point light ten times as bright (the last light: add_point_light appended it)
        flat = scene.flat()
        lights = R._array(flat.lights, C.c_uint32, (flat.light_count, 7))
        point = int(np.flatnonzero(R.light_kind(lights) == R.POINT)[0])
        edited = lights.copy()
        edited[point, 0:3] = (lights[point, 0:3].view(np.float32) * np.float32(10)).view(np.uint32)
        arr = np.ascontiguousarray(edited)
        from directcomputeraytracing_amd import _abi
        assert t._lib.dcrt_tracer_update_lights(t._h, arr.ctypes.data_as(C.POINTER(_abi.Light)), len(arr)) == 0
        assert t.upload_stats()["graph_invalidations"] == drops
        after = t.light_distribution()
        s = dict(R.from_flat(flat), lights=edited)
        ref = LT.Table(s, after["radius"])
        assert after["light_prob"][point] > 2 * before["light_prob"][point]
        assert all(ulps_apart(after[k], getattr(ref, k)).max() <= 2 for k in ("light_prob", "light_cdf", "tri_prob", "tri_cdf"))
        assert same_bits(after["tri_prob"], before["tri_prob"]).all() and same_bits(after["tri_cdf"], before["tri_cdf"]).all()
        t.clear_film()
        t.render_images(0, 1)
        assert np.isfinite(t.read_film()).all()
        # a light removed, and added again: the table rebuilt, the graphs dropped once each time
        fewer = np.ascontiguousarray(np.delete(edited, point, 0))
        assert t._lib.dcrt_tracer_update_lights(t._h, fewer.ctypes.data_as(C.POINTER(_abi.Light)), len(fewer)) == 0
        assert t.upload_stats()["graph_invalidations"] == drops + 1 and t.light_distribution()["n"] == len(fewer)
        frame = scene.frame_params(0)
        assert frame.light_count == len(edited)
        t.set_frame_params(frame)                               # (names one light more than the table holds)
        t.clear_film()
        with pytest.raises(DCRTError):
            t.render_images(0, 1)
        with pytest.raises(DCRTError):
            t.light_sample(np.zeros((1, 3), np.float32), np.ones((1, 4), np.uint32))
        frame.light_count = len(fewer)
        t.set_frame_params(frame)
        t.render_images(0, 1)                                   # (graphs again, for the next edit to drop)
        assert t._lib.dcrt_tracer_update_lights(t._h, arr.ctypes.data_as(C.POINTER(_abi.Light)), len(arr)) == 0
        assert t.upload_stats()["graph_invalidations"] == drops + 2 and t.light_distribution()["n"] == len(arr)
        frame.light_count = len(arr)
        t.set_frame_params(frame)
        t.render_images(0, 1)
        frame.light_count = len(arr) - 1                        # fewer lights than are held: refused under the table ...
        t.set_frame_params(frame)
        with pytest.raises(DCRTError):
            t.render_images(0, 1)
        t.set_light_sampling("uniform")                         # ... and accepted without one, as it always was
        t.clear_film()
        t.render_images(0, 1)
        assert np.isfinite(t.read_film()).all()
    finally:
        t.destroy()


def test_everything_on_together(native_lib, golden_luts, tmp_path):
    """`lamps` under the 8-texel cube at B = 2 with light selection, environment importance sampling and the roulette
    all on, against light selection alone: neither of the other two changes the expectation, so the quadrant means
    agree within both standard errors by the rule of test_renderer_means_are_the_rendering_equations."""
    from directcomputeraytracing_amd import WavefrontPathTracer, scenes
    scene = PS.with_case(LS.load("lamps", tmp_path), 2, True)
    scene.set_environment_light((0.03, 0.035, 0.05), scenes.env_cube(8))
    t = WavefrontPathTracer(path_pool_size=1 << 16)
    try:
        t.set_luts(golden_luts)
        t.on_scene_loaded(scene)
        t.set_light_sampling("power")
        alone = PR.quadrant_statistics(LS.device_samples(t, 8))
        t.set_environment_sampling("importance")
        t.set_russian_roulette(True, start_bounce=1)
        assert t.light_sampling() == ("power", True) and t.environment_sampling() == ("importance", True)
        both = PR.quadrant_statistics(LS.device_samples(t, 8, first=100))
    finally:
        t.destroy()
    ok, worst = within(both[0], both[1], alone[0], alone[1], z_bound(comparisons()))
    print("all on against the table alone: worst |difference| / bound", round(worst, 3), "NaN shares", alone[3], both[3])
    assert alone[3] <= NAN_CAP and both[3] <= NAN_CAP and ok, (worst, alone[0], both[0])


@pytest.mark.parametrize("interleave", [False, True])
def test_make_pipelines_passes_the_mode_on(native_lib, tmp_path, interleave):
    from directcomputeraytracing_amd.tracer import make_pipelines
    scene = PS.with_case(LS.load("lamps", tmp_path), 0, True)
    pipes = make_pipelines(scene, 1 << 16, streams=2, interleave=interleave, light_sampling="power")
    try:
        assert len(pipes) == 2 and all(p.light_sampling() == ("power", True) for p in pipes)
    finally:
        for p in pipes:
            p.destroy()


def test_dcrt_render_light_power(native_lib, tmp_path):
    """examples/dcrt_render --light-power writes an image, and another one than without the flag."""
    from directcomputeraytracing_amd.build import build_examples
    exe = build_examples()
    LS.load("lamps", tmp_path)
    xml = tmp_path / "lamps" / "lamps.xml"
    out = {}
    for flag in ("--light-power", None):
        bmp = tmp_path / f"{flag or 'plain'}.bmp"
        args = [str(exe), str(xml), str(LS.SIZE), str(LS.SIZE), "4", "2", str(bmp)] + ([flag] if flag else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout.strip().splitlines()[-1])["images"] == 4
        out[flag] = bmp.read_bytes()
    assert len(out["--light-power"]) == len(out[None]) > LS.SIZE * LS.SIZE * 3 and out["--light-power"] != out[None]
