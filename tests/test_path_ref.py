"""The path-truth layer on the CPU ("Path truth"): tests/path_ref.py -- a float64
estimator of the expected sample radiance, written from the rendering equation -- against closed forms;
the fixture tests/golden/path_truth.json against a fresh run of it; and the oracle's quadrant means
against the fixture.

The bound of every statistical comparison is |a - b| <= z sqrt(sem_a^2 + sem_b^2), z the two-sided normal
quantile of a family-wise false-alarm rate of 1e-6, Bonferroni over every such comparison in this file
(`comparisons`). Samples with a NaN channel (the power heuristic's inf / inf, reference arithmetic) are
dropped under a cap of 0.1 % per case; nothing else is excluded. The oracle's NaN share is 0 in every
case of every scene here (measured; the emissive box's is 5e-5).

Measured on one core: the closed forms 8 s, the fixture check 105 s (bleed 59, veil 28, coat 8), the oracle
against the fixture 3 s; worst |difference| / bound 0.48 (fixture check) and 0.53 (oracle). DESIGN.md has the
table of oracle changes that this file catches."""
import math
from statistics import NormalDist

import numpy as np
import pytest

import path_ref as PR
import path_scenes as PS
import shading_ref as S
from conftest import GOLDEN

FAMILY_RATE = 1e-6
NAN_CAP = 1e-3
ORACLE_IMAGES = 16
BOX_PATHS = 1 << 16
VEIL_PATHS = 1 << 16


def cases(name):
    spec = PS.SCENES[name]
    return [(vis, b) for vis in spec["visible"] for b in spec["bounces"]]


def comparisons():
    """How many statistical comparisons this file makes: per scene and case 4 quadrants x 3 channels, once
    for the fixture's check and once for the oracle; the black veil; the two veils (both models against their
    closed forms, the oracle against the model); the emissive box against the oracle; the smooth-plastic plane
    at its two B."""
    return 2 * sum(len(cases(n)) * 12 for n in PS.SCENES) + 1 + 3 + 1 + 2


def z_bound(count=None):
    return NormalDist().inv_cdf(1.0 - FAMILY_RATE / (2.0 * (count or comparisons())))


def within(a, sem_a, b, sem_b, z):
    """(ok, the worst |a - b| / bound) over all statistics; a statistic that is exact on both sides must be equal."""
    bound = z * np.sqrt(np.asarray(sem_a) ** 2 + np.asarray(sem_b) ** 2)
    diff = np.abs(np.asarray(a) - np.asarray(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 1e-9, np.inf, 0.0))
    return bool((ratio <= 1.0).all()), float(ratio.max())


@pytest.fixture(scope="module")
def lut_arrays():
    return dict(np.load(GOLDEN / "bxdf_luts.npz"))


@pytest.fixture(scope="module")
def fixture():
    return PR.load_fixture()


def test_bound_comes_from_the_comparison_count():
    n = comparisons()
    assert n == 2 * 12 * (6 + 3 + 3 + 3 + 3 + 6 + 3) + 7
    z = z_bound()
    assert math.isclose(2 * (1 - NormalDist().cdf(z)) * n, FAMILY_RATE, rel_tol=1e-4) and 5.5 < z < 6.5


# ---- the reference against closed forms -----------------------------------------------------------------
def test_lit_plane_is_the_analytic_irradiance(native_lib, lut_arrays, tmp_path):
    """A diffuse plane (rho 0.6) under one point light, B = 0: every path's radiance is rho / pi C cos / d^2 at
    the point its camera ray meets the plane -- a deterministic term (no proposal enters), 1e-10 relative."""
    from directcomputeraytracing_amd import Scene, scenes
    rho, Cl, light = 0.6, np.array([3.0, 2.0, 1.0]), np.array([0.4, 1.2, 2.0])
    s = Scene((64, 64))
    s.load_from_file(scenes.write_lit_plane(tmp_path, 64, 64, albedo=rho))
    s.add_point_light(tuple(light), tuple(Cl))
    ref = PR.PathRef(s.flat(), s.frame_params(0), lut_arrays)
    rng = np.random.default_rng(1)
    film, ap = rng.random((4000, 2)), rng.random((4000, 3))
    L, L0 = ref.radiance(rng, film, ap, (0,))
    o, d, _, _ = S.camera_ray(ref.frame, film, ap)
    t = -o[:, 1] / d[:, 1]
    p = o + t[:, None] * d
    on = (d[:, 1] < 0) & (np.abs(p[:, 0]) < 4) & (np.abs(p[:, 2]) < 4)
    l = np.float32(light).astype(np.float64) - p
    d2 = (l * l).sum(1)
    want = np.where(on[:, None], np.float32(rho).astype(np.float64) / np.pi * np.float32(Cl).astype(np.float64) * (np.maximum(l[:, 1], 0) / np.sqrt(d2) / d2)[:, None], 0.0)
    assert on.mean() > 0.5 and not L0.any()
    np.testing.assert_allclose(L[:, 0], want, rtol=1e-10, atol=1e-300)


PLANE_PATHS = 1 << 16


def test_smooth_plastic_plane_is_its_closed_form(native_lib, lut_arrays, tmp_path):
    """The mixed vertex against a closed form that does not pass through the fixture: a smooth-plastic plane
    (ior 1.5 / 1.000277, albedo rho, internal scattering MULTIPLE) alone under a constant environment of 1.
    Every ray that leaves the plane reaches the environment (weight m = 1: both of the environment's pdfs are
    the true density, and s = q for the Lambert base; 1 after the coat), so a path that meets the plane at
    cos c carries, in expectation, the Lambert base's albedo plus the coat's reflectance,
        (1 - coat(c)) rho isf + F(c, 1, ior),
    coat the dielectric-BRDF table's weight and isf = (1 - R_in) / (1 - rho R_in), both looked up through
    bsdf_ref; a path that misses it carries the environment's 1. At B = 0 and at B = 1 (nothing is there to
    be met twice). Each path takes one of two values (coat or base), so the mean over the film is compared:
    the mean of (path - closed form) is 0 within z standard errors of it, z from `comparisons`."""
    import bsdf_ref as R
    from directcomputeraytracing_amd import Scene
    from directcomputeraytracing_amd.scenes import _xml
    rho = (0.9, 0.5, 0.1)
    PS._write_faces(tmp_path / "plane.obj", [PS._quad((0, 0, 0), (30, 0, 0), (0, 0, -30))])
    body = (PS._integrator(1) + PS._camera((0, 1.0, -1.0), pitch=25, fov=80)
            + PS._shape("plane", f'<bsdf type="plastic"><rgb name="diffuse_reflectance" value="{rho[0]}, {rho[1]}, {rho[2]}"/>'
                        '<float name="int_ior" value="1.5"/><boolean name="nonlinear" value="true"/></bsdf>')
            + '  <emitter type="constant"><rgb name="radiance" value="1, 1, 1"/></emitter>\n')
    (tmp_path / "plane.xml").write_text(_xml(body))
    s = Scene((64, 64))
    s.load_from_file(tmp_path / "plane.xml")
    ref = PR.PathRef(s.flat(), s.frame_params(0), lut_arrays)
    rng = np.random.default_rng(8)
    film, ap = rng.random((PLANE_PATHS, 2)), rng.random((PLANE_PATHS, 3))
    L, L0 = ref.radiance(rng, film, ap, (0, 1))
    o, d, _, _ = S.camera_ray(ref.frame, film, ap)
    with np.errstate(divide="ignore"):
        at = o - (o[:, 1] / d[:, 1])[:, None] * d
    on = (d[:, 1] < 0) & (np.abs(at[:, 0]) < 30) & (np.abs(at[:, 2]) < 30)
    c = np.where(on, -d[:, 1], 1.0)
    mat = R.material(R.PLASTIC, albedo=rho, alpha=0.0, ior=np.float32(1.5) / np.float32(1.000277), internal_scattering=R.ISF_MULTIPLE)
    luts = R.Luts(lut_arrays)
    coat = R.lut_brdf_dielectric(luts, c, 0.0, np.float64(mat["ior"][0]), False)
    want = (1.0 - coat)[:, None] * mat["albedo"].astype(np.float64) * R.internal_scattering_factor(luts, mat) \
        + R.fresnel_dielectric(c, 1.0, np.float64(mat["ior"][0]))[:, None]
    want = np.where(on[:, None], want, 0.0)
    assert 0.3 < on.mean() < 0.9 and 0.03 < coat[on].min() < 0.05 and coat[on].max() > 0.3
    assert (L0 == np.where(on[:, None], 0.0, 1.0)).all()
    z = z_bound()
    for j, b in enumerate((0, 1)):
        diff = L[:, j] - want
        mean, sem = diff.mean(0), diff.std(0) / np.sqrt(len(diff))
        ok, worst = within(mean, sem, 0.0, 0.0, z)
        print("smooth-plastic plane B", b, "mean radiance", L[:, j].mean(0).round(5), "closed form", want.mean(0).round(5), "sem", sem.round(5), "worst", round(worst, 3))
        assert ok and 0 < sem.max() < 2e-3, (mean, sem, worst)
    # (the resolution: a Lambert base weighted 1 instead of 1 - coat is outside the bound)
    base = np.where(on[:, None], coat[:, None] * mat["albedo"].astype(np.float64) * R.internal_scattering_factor(luts, mat), 0.0)
    assert not within(mean - base.mean(0), sem, 0.0, 0.0, z)[0]


@pytest.mark.parametrize("woz,ms", [(0.7, False), (-0.4, True), (0.15, True)])
def test_dielectric_proposal_follows_its_density(lut_arrays, woz, ms):
    """`dielectric_proposal` returns directions wi and a density g; the estimator divides by g, so the directions
    must follow it. For phi = the uniform density, the cosine density of the upper hemisphere and that of the
    lower one, each of integral 1, the mean of phi(wi) / g(wi) over 2^17 draws is 1 within 6 of its standard errors
    (g >= 1 / (8 pi) bounds every term; another density in the sampler than in g -- the Fresnel term of the wrong
    side, a reflection where g states a refraction -- moves at least one of the three)."""
    import bsdf_ref as R
    n = 1 << 17
    wo = np.tile(np.array([np.sqrt(1 - woz * woz), 0.0, woz]), (n, 1))
    mat = R.material(R.DIELECTRIC, alpha=0.6, ior=1.5, multiscattering=ms)
    wi, g = PR.dielectric_proposal(np.random.default_rng(12), R.Luts(lut_arrays), mat, wo)
    np.testing.assert_allclose((wi * wi).sum(1), 1.0, rtol=1e-12)
    assert (g >= 1 / (8 * np.pi)).all()
    for phi in (np.full(n, 1 / (4 * np.pi)), np.maximum(wi[:, 2], 0) / np.pi, np.maximum(-wi[:, 2], 0) / np.pi):
        x = phi / g
        assert abs(x.mean() - 1.0) <= 6.0 * x.std() / np.sqrt(n), (x.mean(), x.std() / np.sqrt(n))


def test_white_furnace_is_one(native_lib, lut_arrays, tmp_path):
    """An albedo-1 diffuse convex cube under a constant environment of 1: every path carries exactly 1 (the
    environment's pair of strategies is unbiased, m = 1), at every depth."""
    from directcomputeraytracing_amd import Scene, scenes
    s = Scene((64, 64))
    s.load_from_file(scenes.write_furnace(tmp_path, 64, 64))
    ref = PR.PathRef(s.flat(), s.frame_params(0), lut_arrays)
    st = ref.region_statistics(2, 1 << 14, (0, 2, 8), regions=1)
    np.testing.assert_allclose(st["visible"]["mean"], 1.0, rtol=1e-9)
    assert st["visible"]["sem"].max() < 1e-9


def _black_veils(tmp_path, opacities):
    """Black veils of the given opacities, one behind the other, across the whole view of a constant environment of 1."""
    from directcomputeraytracing_amd import Scene
    from directcomputeraytracing_amd.scenes import _xml
    body = PS._integrator(0) + PS._camera((0, 0, 0), fov=60)
    for k, a in enumerate(opacities):
        PS._write_faces(tmp_path / f"veil{k}.obj", [PS._quad((0, 0, 2 + k), (-30, 0, 0), (0, 30, 0))])
        body += PS._shape(f"veil{k}", f'<bsdf type="mask"><float name="opacity" value="{a}"/>' + PS._diffuse("0, 0, 0", True) + "</bsdf>")
    body += '  <emitter type="constant"><rgb name="radiance" value="1, 1, 1"/></emitter>\n'
    (tmp_path / "veils.xml").write_text(_xml(body))
    s = Scene((64, 64))
    s.load_from_file(tmp_path / "veils.xml")
    s.features = s.features | PS.ANYHIT
    return s


def test_black_veil_passes_its_transparency(native_lib, lut_arrays, tmp_path):
    """A black veil of opacity 0.37 across the whole view of a constant environment of 1: 0.63."""
    s = _black_veils(tmp_path, [0.37])
    ref = PR.PathRef(s.flat(), s.frame_params(0), lut_arrays)
    st = ref.region_statistics(3, VEIL_PATHS, (0,), regions=1)["visible"]
    want = 1.0 - float(np.float32(0.37))
    ok, worst = within(st["mean"], st["sem"], want, 0.0, z_bound())
    print("black veil", st["mean"].ravel(), st["sem"].ravel(), worst)
    assert ok and 0 < st["sem"].max() < 3e-3, (st["mean"], st["sem"], worst)


def test_two_veils_share_one_opacity_draw(native_lib, lut_arrays, oracle_mod, golden_luts, tmp_path):
    """QUIRK P1 pinned: behind veils of opacity 0.37 and 0.5 the renderer shows 1 - max = 0.5 of the environment (one
    draw per ray, tested at every crossing: WavefrontPathTracing.hlsl:224-225, BVHAccel.inc.hlsl:188), where
    independent crossings would show 0.63 x 0.5 = 0.315. The model with the switch on predicts the first, with
    it off the second, and the oracle follows the first."""
    s = _black_veils(tmp_path, [0.37, 0.5])
    z = z_bound()
    shared = PR.PathRef(s.flat(), s.frame_params(0), lut_arrays).region_statistics(7, VEIL_PATHS, (0,), regions=1)["visible"]
    apart = PR.PathRef(s.flat(), s.frame_params(0), lut_arrays, shared_opacity_draw=False).region_statistics(7, VEIL_PATHS, (0,), regions=1)["visible"]
    assert within(shared["mean"], shared["sem"], 0.5, 0.0, z)[0], shared["mean"]
    assert within(apart["mean"], apart["sem"], (1.0 - float(np.float32(0.37))) * 0.5, 0.0, z)[0], apart["mean"]
    mean, sem, _, nan = PR.quadrant_statistics(oracle_case(oracle_mod, golden_luts, s), 1)
    ok, worst = within(mean, sem, shared["mean"][0], shared["sem"][0], z)
    print("two veils: shared", shared["mean"].ravel()[0], "apart", apart["mean"].ravel()[0], "oracle", mean.ravel()[0], sem.ravel()[0], worst)
    assert nan == 0 and ok, (mean, shared["mean"], worst)
    assert not within(mean, sem, apart["mean"][0], apart["sem"][0], 2 * z)[0]


@pytest.fixture(scope="module")
def emissive_box(native_lib, tmp_path_factory):
    from directcomputeraytracing_amd import Scene, scenes
    s = Scene((64, 64))
    s.load_from_file(scenes.write_emissive_box(tmp_path_factory.mktemp("box"), 64, 64, albedo=0.5, radiance=1.0, max_bounce=8))
    return s


def test_emissive_box_without_the_model_is_the_geometric_series(emissive_box, lut_arrays):
    """mis_model=False (m = 1, an unbiased estimator): sum_{k=0}^{B+1} 0.5^k at B = 0, 2, 8, exactly -- every
    vertex is on an emitting wall, so no proposal enters either."""
    ref = PR.PathRef(emissive_box.flat(), emissive_box.frame_params(0), lut_arrays, mis_model=False)
    st = ref.region_statistics(4, 1 << 12, (0, 2, 8), regions=1)["visible"]
    np.testing.assert_allclose(st["mean"][:, 0, 0], [1.5, 1.875, sum(0.5 ** k for k in range(10))], rtol=1e-12)


def test_emissive_box_with_the_model_lands_on_the_oracle(emissive_box, lut_arrays, oracle_mod, golden_luts):
    """The first independent prediction of the 1.93-1.94 that the reference's halved triangle-light pdf gives
    (tests/test_physics.py pins it as a band): the m model (p_s = 2 p for mesh lights) against the oracle's mean
    of the same scene. Measured: 1.93503 +- 0.00015 (2^18 paths) against 1.93484 +- 0.00051."""
    s = emissive_box
    ref = PR.PathRef(s.flat(), s.frame_params(0), lut_arrays)
    st = ref.region_statistics(5, BOX_PATHS, (8,), regions=1)["visible"]
    flat = oracle_mod.flat_with_own_bvh(s)
    imgs = np.stack([oracle_mod.render(flat, golden_luts, oracle_mod.frame_params(s, k), oracle_mod.WAVEFRONT)[1][..., :3] for k in range(ORACLE_IMAGES)])
    mean, sem, _, nan = PR.quadrant_statistics(imgs, 1)
    ok, worst = within(st["mean"][0], st["sem"][0], mean, sem, z_bound())
    print("emissive box: reference", st["mean"][0, 0, 0], st["sem"][0, 0, 0], "oracle", mean[0, 0], sem[0, 0], "NaN share", nan, "worst", worst)
    assert nan <= NAN_CAP and ok, (st["mean"], mean, worst)
    assert 1.92 < st["mean"][0, 0, 0] < 1.95


def test_vectorised_delta_lobes_are_the_scalar_definition():
    import bsdf_ref as R
    rng = np.random.default_rng(6)
    wo = rng.normal(size=(200, 3))
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    wo[:20, 2] *= 0.02                                     # grazing: total internal reflection from inside
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    mats = [R.material(R.DIELECTRIC, alpha=0.0, ior=1.5), R.material(R.THIN, alpha=0.0, ior=1.5),
            R.material(R.CONDUCTOR, albedo=(3.6, 2.6, 2.3), alpha=0.0, ior=(0.15, 0.4, 1.4)),
            R.material(R.CONDUCTOR, albedo=(3.6, 2.6, 2.3), alpha=0.0, ior=(0.15, 0.4, 1.4), two_sided=True),
            R.material(R.PLASTIC, albedo=(0.7, 0.6, 0.5), alpha=0.0, ior=1.5, internal_scattering=1),
            R.material(R.PLASTIC, albedo=(0.7, 0.6, 0.5), alpha=0.0, ior=1.8, two_sided=True, internal_scattering=2)]
    luts = R.Luts(dict(np.load(GOLDEN / "bxdf_luts.npz")))
    tir = 0
    for mat in mats:
        many = PR.delta_lobes_many(mat, wo, luts)
        for i in range(len(wo)):
            one = R.delta_lobes(mat, wo[i], L=luts)
            present = [l for l in many if l[2][i] > 0]
            assert len(present) == len(one), (mat["type"], i)
            tir += mat["type"] == R.DIELECTRIC and len(one) == 1
            for (wi, fw, pr), (wi1, fw1, pr1) in zip(present, one):
                np.testing.assert_allclose(wi[i], wi1, rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(fw[i], fw1, rtol=1e-12)
                np.testing.assert_allclose(pr[i], pr1, rtol=1e-12)
    assert tir > 10
    # (a one-sided plastic has its coat from outside only, a two-sided one from both sides)
    assert [int((PR.delta_lobes_many(m, wo, luts)[0][2] > 0).sum()) for m in mats[-2:]] == [int((wo[:, 2] > 0).sum()), len(wo)]


# ---- the fixture is current ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PS.SCENES))
def test_fixture_is_current(native_lib, fixture, name):
    """The scene recomputed at a quarter of the fixture's path count with another seed agrees with the fixture."""
    entry = fixture["scenes"][name]
    assert entry["paths"] == PS.SCENES[name]["paths"] and fixture["regions"] == 2
    st = PR.scene_statistics(name, entry["paths"] // 4, entry["seed"] + 1000)
    z = z_bound()
    worst = 0.0
    for vis, b in cases(name):
        key = "visible" if vis else "hidden"
        j = PS.SCENES[name]["bounces"].index(b)
        mean, sem = PR.fixture_entry(fixture, name, vis, b)
        ok, w = within(st[key]["mean"][j], st[key]["sem"][j], mean, sem, z)
        worst = max(worst, w)
        assert ok, (name, key, b, w)
    print(name, "fixture check: worst |difference| / bound", round(worst, 3))


# ---- the oracle is held to the fixture --------------------------------------------------------------------
def oracle_case(oracle_mod, golden_luts, scene, images=ORACLE_IMAGES, mode=None):
    flat = oracle_mod.flat_with_own_bvh(scene)
    mode = oracle_mod.WAVEFRONT if mode is None else mode
    return np.stack([oracle_mod.render(flat, golden_luts, oracle_mod.frame_params(scene, k), mode)[1][..., :3] for k in range(images)])


@pytest.mark.parametrize("name", list(PS.SCENES))
def test_oracle_means_are_the_fixtures(native_lib, oracle_mod, golden_luts, fixture, name, tmp_path):
    scene = PS.load(name, tmp_path)
    z = z_bound()
    for vis, b in cases(name):
        PS.with_case(scene, b, vis)
        mean, sem, _, nan = PR.quadrant_statistics(oracle_case(oracle_mod, golden_luts, scene))
        want, want_sem = PR.fixture_entry(fixture, name, vis, b)
        ok, worst = within(mean, sem, want, want_sem, z)
        print(name, "visible" if vis else "hidden", "B", b, "NaN share", nan, "worst |difference| / bound", round(worst, 3),
              "sem ratio reference / oracle", round(float((want_sem / np.maximum(sem, 1e-300)).max()), 3))
        assert nan <= NAN_CAP, (name, vis, b, nan)
        assert ok, (name, vis, b, worst, mean, want)
