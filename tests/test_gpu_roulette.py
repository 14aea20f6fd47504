"""Russian roulette on the device (include/dcrt.h "Russian roulette"; tests/roulette_ref.py restates the rule).

a. dcrt_device_roulette -- the function shade_path and the megakernel call -- is roulette_ref bit for bit.
b. enable 1, start 0, min = max = 1 (q >= 1 at every vertex: no draw, no scaling) leaves image 0 of every
   path-truth scene the oracle's bit for bit, ray counts included, in both modes.
c. The setter's refusals, and the setting's life across uploads and edits without a dropped graph.
d. Unbiased: the rule of tests/test_gpu_path_ref.py unchanged -- quadrant means of PS.SCENES[name]["images"]
   images against tests/golden/path_truth.json with `within`, NAN_CAP and z_bound -- under a fixed coin at every
   vertex (start 0, min = max = 0.5: a missing / q halves every indirect term) in both modes, and under the
   throughput-driven form (start 1, min 0.1, max 0.95) in wavefront mode.
e. The survival frequency is Binomial(M, q) exactly (derivation at the test).
f. Pool size, image batch, the early-finish route and film bands do not change a bit.
g. Fewer extension rays than without it.

z is the two-sided normal quantile of a family-wise rate of 1e-6 over this file's own statistical comparisons
(`comparisons`): d's quadrant statistics and e's four counts. Films are 64 x 64, pools 2^10 to 2^16 slots."""
import os

import numpy as np
import pytest

import path_ref as PR
import path_scenes as PS
import roulette_ref as RR
from test_gpu_parity import same_bits
from test_path_ref import NAN_CAP, cases, within, z_bound

pytestmark = pytest.mark.gpu

SIZE = 64
COIN = dict(start_bounce=0, min_survival=0.5, max_survival=0.5)
THROUGHPUT = dict(start_bounce=1, min_survival=0.1, max_survival=0.95)
IDENTITY = dict(start_bounce=0, min_survival=1.0, max_survival=1.0)
RAYS = ("extension_rays", "shadow_rays", "new_paths", "images_completed")
E_COUNTS = 4          # test e: two settings x two early-finish routes


def comparisons():
    """d: the fixed coin in both modes and the throughput form in one, every case's 4 quadrants x 3 channels; e: 4 counts."""
    return 3 * sum(len(cases(n)) * 12 for n in PS.SCENES) + E_COUNTS


class env:
    """Environment variables for the length of a block (the knobs are read at creation, uploads and edits)."""

    def __init__(self, **values):
        self.values = {k: v for k, v in values.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.values}
        os.environ.update(self.values)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def same(a, b):
    """Bit-identical arrays (float32: test_gpu_parity's same_bits, a NaN matching any NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(same_bits(a, b).all()) if a.dtype == np.float32 else bool(np.array_equal(a, b))


def new_tracer(luts, scene, pool=1 << 16, early=None, roulette=None, mode="wavefront", batch=None, bands=None, seed=0):
    from directcomputeraytracing_amd import WavefrontPathTracer
    with env(DCRT_EARLY_FINISH=early):
        t = WavefrontPathTracer(path_pool_size=pool, iterations_per_render=8, debug_rng=True)
        try:
            t.set_luts(luts)
            t.on_scene_loaded(scene, seed)
            t.set_mode(mode)
            if batch is not None:
                t.set_image_batch(batch)
            if bands is not None:
                t.set_film_bands(bands, 2)
            if roulette is not None:
                t.set_russian_roulette(True, **roulette)
        except BaseException:
            t.destroy()
            raise
    return t


def lit_plane(directory, rho=0.6):
    from directcomputeraytracing_amd import Scene, scenes
    s = Scene((SIZE, SIZE))
    s.load_from_file(scenes.write_lit_plane(directory, SIZE, SIZE, albedo=rho))
    s.add_point_light((0.4, 1.2, 2.0), (3.0, 2.0, 1.0))
    return s


# ---- a. the probe ----------------------------------------------------------------------------------------
def test_probe_is_the_restatement_bit_for_bit(gpu_tracer):
    rng = np.random.default_rng(21)
    n = 4096
    T = (rng.random((n, 3)) ** 3 * 1.6).astype(np.float32)
    T[rng.random(n) < 0.1] *= np.float32(0.01)
    u = rng.random(n).astype(np.float32)
    ended = 0
    for lo, hi in [(0.05, 1.0), (0.1, 0.95), (0.5, 0.5), (1.0, 1.0)]:
        eT, eu = RR.edge_rows(lo, hi)
        for rows, draws in ((T, u), (eT, eu)):
            q, survive, scaled = gpu_tracer.device_roulette(rows, draws, lo, hi)
            q_ref, survive_ref, scaled_ref = RR.roulette(rows, draws, lo, hi)
            assert same_bits(q, q_ref).all(), (lo, hi)
            assert (survive == survive_ref).all(), (lo, hi, rows[survive != survive_ref][:4], draws[survive != survive_ref][:4])
            assert same_bits(scaled, scaled_ref).all(), (lo, hi)
            ended += int((~survive).sum())
        assert np.isfinite(q).all()
    assert ended > 1000
    q, survive, scaled = gpu_tracer.device_roulette(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), 0.05, 1.0)
    assert len(q) == len(survive) == len(scaled) == 0


# ---- b. identity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["wavefront", "megakernel"])
@pytest.mark.parametrize("name", list(PS.SCENES))
def test_survival_one_is_the_oracle_bit_for_bit(native_lib, oracle_mod, golden_luts, tmp_path, name, mode):
    scene = PS.load(name, tmp_path)
    vis, b = cases(name)[-1]                 # (the scene's largest B: the most vertices pass through the rule)
    PS.with_case(scene, b, vis)
    t = new_tracer(golden_luts, scene, roulette=IDENTITY, mode=mode)
    try:
        assert t.russian_roulette() == dict(enable=True, **IDENTITY)
        t.clear_film()
        t.reset_stats()
        t.render_images(0, 1)
        pos, val = t.read_samples()
        rng, c = t.read_rng(), t.counters()
    finally:
        t.destroy()
    p_ref, v_ref, r_ref, c_ref = oracle_mod.render(oracle_mod.flat_with_own_bvh(scene), golden_luts, oracle_mod.frame_params(scene, 0),
                                                   oracle_mod.MEGAKERNEL if mode == "megakernel" else oracle_mod.WAVEFRONT, rng=True)
    assert np.array_equal(pos.view(np.uint32), p_ref.view(np.uint32))
    bad = np.count_nonzero(~same_bits(val, v_ref).all(-1))
    assert bad == 0, f"{name} {mode}: {bad} samples differ from the oracle's"
    assert np.array_equal(rng, r_ref)        # (no draw was made: the terminal states are the oracle's)
    assert (c["extension_rays"], c["shadow_rays"]) == (c_ref["extension_rays"], c_ref["shadow_rays"])


# ---- c. the setter ---------------------------------------------------------------------------------------
def test_setter_refusals_and_the_settings_life(native_lib, golden_luts, tmp_path):
    import ctypes as C
    from conftest import cornell
    from directcomputeraytracing_amd import DCRTError, _abi
    scene = cornell(SIZE, SIZE, 3)
    t = new_tracer(golden_luts, scene, pool=1 << 12)
    try:
        assert t.russian_roulette() == dict(enable=False, start_bounce=2, min_survival=float(np.float32(0.05)), max_survival=1.0)
        t.set_russian_roulette(True, 3, 0.25, 0.75)
        kept = dict(enable=True, start_bounce=3, min_survival=0.25, max_survival=0.75)
        assert t.russian_roulette() == kept
        nan, inf = float("nan"), float("inf")
        for start, lo, hi in [(21, 0.25, 0.75), (1 << 31, 0.25, 0.75), (0, 0.0, 0.75), (0, -0.25, 0.75), (0, 0.8, 0.75), (0, 0.25, 1.5),
                              (0, nan, 0.75), (0, 0.25, nan), (0, nan, nan), (0, inf, inf), (0, 0.25, inf), (0, -inf, 0.75)]:
            assert not RR.valid(start, lo, hi)
            p = _abi.RouletteParams(1, start, lo, hi)
            assert t._lib.dcrt_tracer_set_roulette(t._h, C.byref(p)) == -1, (start, lo, hi)
            with pytest.raises(DCRTError, match="INVALID_ARG"):
                t.set_russian_roulette(True, start, lo, hi)
            assert t.russian_roulette() == kept
        assert t._lib.dcrt_tracer_set_roulette(t._h, None) == -1 and t._lib.dcrt_tracer_get_roulette(t._h, None) == -1
        # the limits themselves are fine
        t.set_russian_roulette(True, 20, 1e-30, 1e-30)
        t.set_russian_roulette(True, 0, 1.0, 1.0)
        t.set_russian_roulette(True, 3, 0.25, 0.75)
        # it lives on the tracer: uploads and partial updates keep it, and no graph depends on it
        t.clear_film()
        t.render_images(0, 2)                                  # (graphs exist)
        drops = t.upload_stats()["graph_invalidations"]
        t.set_russian_roulette(True, 1, 0.5, 0.5)
        t.set_russian_roulette(True, 3, 0.25, 0.75)
        assert t.upload_stats()["graph_invalidations"] == drops
        t.update_materials(scene)
        assert t.russian_roulette() == kept
        t.on_scene_loaded(scene)
        assert t.russian_roulette() == kept
        t.on_scene_loaded(lit_plane(tmp_path))
        assert t.russian_roulette() == kept
        # off again: the fields stay, the image is the plain one
        t.set_russian_roulette(False, 3, 0.25, 0.75)
        assert t.russian_roulette() == dict(kept, enable=False)
        # the probe checks its parameters the same way
        with pytest.raises(DCRTError, match="INVALID_ARG"):
            t.device_roulette(np.ones((1, 3), np.float32), np.zeros(1, np.float32), 0.8, 0.75)
    finally:
        t.destroy()


def test_off_after_on_is_the_plain_image(native_lib, golden_luts):
    from conftest import cornell
    scene = cornell(SIZE, SIZE, 4)
    plain = new_tracer(golden_luts, scene, pool=1 << 12)
    t = new_tracer(golden_luts, scene, pool=1 << 12, roulette=COIN)
    try:
        def run(tr):
            tr.clear_film()
            tr.reset_stats()
            tr.render_images(5, 2)
            return tr.read_film(), tr.read_samples()[1], tr.read_rng(), {k: tr.counters()[k] for k in RAYS}

        runs = [run(plain), run(t)]
        t.set_russian_roulette(False)          # (the same tracer, its graphs captured with the roulette on)
        runs.append(run(t))
        assert not same(runs[1][0], runs[0][0]) and runs[1][3]["extension_rays"] < runs[0][3]["extension_rays"]
        for a, b in zip(runs[2][:3], runs[0][:3]):
            assert same(a, b)
        assert runs[2][3] == runs[0][3]
    finally:
        plain.destroy()
        t.destroy()


# ---- d. unbiased -----------------------------------------------------------------------------------------
def _device_samples(t, images):
    out = []
    for seed in range(images):
        t.clear_film()
        t.render_images(seed, 1)
        out.append(t.read_samples()[1][..., :3].copy())
    return np.stack(out)


@pytest.mark.parametrize("form,mode", [("coin", "wavefront"), ("coin", "megakernel"), ("throughput", "wavefront")])
@pytest.mark.parametrize("name", list(PS.SCENES))
def test_device_means_stay_the_fixtures(native_lib, golden_luts, tmp_path, name, form, mode):
    fixture = PR.load_fixture()
    scene = PS.load(name, tmp_path)
    images = PS.SCENES[name]["images"]
    z = z_bound(comparisons())
    t = new_tracer(golden_luts, scene, roulette=COIN if form == "coin" else THROUGHPUT, mode=mode)
    try:
        for vis, b in cases(name):
            PS.with_case(scene, b, vis)
            t.on_scene_loaded(scene)
            t.set_mode(mode)
            assert t.russian_roulette()["enable"]
            v = _device_samples(t, images)
            mean, sem, _, nan = PR.quadrant_statistics(v)
            want, want_sem = PR.fixture_entry(fixture, name, vis, b)
            ok, worst = within(mean, sem, want, want_sem, z)
            ratio = float((want_sem[sem > 0] / sem[sem > 0]).max())
            print(name, mode, form, "visible" if vis else "hidden", "B", b, "mean", mean.mean(0).round(5), "sem", sem.max(0).round(5),
                  "NaN share", nan, "worst |difference| / bound", round(worst, 3), "sem ratio fixture / device", round(ratio, 3))
            assert nan <= NAN_CAP, (name, mode, form, vis, b, nan)
            assert ratio <= 1.0, (name, mode, form, vis, b, ratio)
            assert ok, (name, mode, form, vis, b, worst, mean, want)
    finally:
        t.destroy()


# ---- e. survival frequency -------------------------------------------------------------------------------
@pytest.mark.parametrize("early", [None, "0"])
def test_survivors_are_binomial(native_lib, golden_luts, tmp_path, early):
    """The lit plane (a Lambert plane of albedo 0.6, one point light) at max_bounce 0, seeds 0..15.

    Off. A camera ray that misses the plane ends its path; one that hits it is shaded at bounce 0, and where the
    BSDF sample is accepted the path casts exactly one more extension ray (its bounce index 1 exceeds max_bounce:
    that ray's hit adds nothing and ends it -- on the early-finish route the ray is the counted last ray, on the long
    way a ray like any other). So extension_rays - new_paths = M, the accepted samples.
    On, start 0. The draws in front of the roulette's (camera, light sample, BSDF sample) are the same numbers in
    both runs, so the same M paths reach the rule, each with its own next number u, uniform on the 2^24 lattice
    and independent between paths: a path casts its further ray iff u < q. With min = max = q0 the count
    k = extension_rays - new_paths is Binomial(M, q0) (q0 = 0.5 is on the lattice: P(u < q0) = q0 exactly), so
    |k - M q0| <= z sqrt(M q0 (1 - q0)). With min 0.05, max 1 the probability is the throughput's largest component:
    a cosine-sampled Lambert surface has T' = rho cos / pi / (cos / pi) = rho up to float32 rounding of a few
    ulp, so each path's q is float32(0.6) (1 +- 1e-6) and k is a sum of M independent Bernoulli(q_i) draws: its
    mean is within M 1e-6 of M p, p = float32(0.6), and its variance at most M p (1 - p) (1 + 1e-5), which the
    M 1e-6 covers as well. Shadow rays and new paths are as without the roulette."""
    scene = lit_plane(tmp_path)
    z = z_bound(comparisons())
    images = 16
    results = {}
    for label, roulette in (("off", None), ("coin", COIN), ("throughput", dict(start_bounce=0, min_survival=0.05, max_survival=1.0))):
        t = new_tracer(golden_luts, scene, early=early, roulette=roulette)
        try:
            assert t.info()["early_finish"] == (0 if early == "0" else 1)
            t.clear_film()
            t.reset_stats()
            t.render_images(0, images)
            results[label] = t.counters()
        finally:
            t.destroy()
    off = results["off"]
    paths = images * SIZE * SIZE
    M = off["extension_rays"] - off["new_paths"]
    assert off["new_paths"] == paths and M > paths / 2
    for label, p, slack in (("coin", 0.5, 0.0), ("throughput", float(np.float32(0.6)), M * 1e-6)):
        c = results[label]
        k = c["extension_rays"] - c["new_paths"]
        bound = z * np.sqrt(M * p * (1 - p)) + slack
        print("early finish", early, label, "M", M, "k", k, "M p", M * p, "|k - M p| / bound", abs(k - M * p) / bound)
        assert (c["new_paths"], c["shadow_rays"]) == (off["new_paths"], off["shadow_rays"])
        assert abs(k - M * p) <= bound, (label, M, k, p, bound)


# ---- f. determinism across routes ------------------------------------------------------------------------
def _run(luts, scene, images=4, **how):
    t = new_tracer(luts, scene, roulette=THROUGHPUT, seed=1, **how)
    try:
        t.clear_film()
        t.reset_stats()
        t.render_images(1, images)
        pos, val = t.read_samples()
        c = t.counters()
        return {"film": t.read_film(), "position": pos, "value": val, "rng": t.read_rng(), "rays": {k: c[k] for k in RAYS},
                "early_finished": c["early_finished"], "info": t.info()}
    finally:
        t.destroy()


def _assert_same(got, want, what, keys=("film", "position", "value", "rng")):
    for key in keys:
        assert same(got[key], want[key]), (what, key)
    assert got["rays"] == want["rays"], what


@pytest.mark.parametrize("which", ["bleed", "lit plane", "cornell"])
def test_routes_do_not_change_a_bit(native_lib, golden_luts, tmp_path, which):
    if which == "bleed":                      # (a mesh light: the any-scene variant, no early finish)
        scene = PS.with_case(PS.load("bleed", tmp_path), 3)
    elif which == "lit plane":                # (a point light alone: the early-finish variant; its paths leave after one
        scene = lit_plane(tmp_path)           #  vertex, so start 1 tests none of them: the routes with the setting on)
    else:                                     # (the early-finish variant with paths the roulette ends at every bounce
        from conftest import cornell          #  from 1 on, the last shaded one included: no last ray for those)
        scene = cornell(SIZE, SIZE, 3)
    base = _run(golden_luts, scene, batch=1)
    assert base["info"]["early_finish"] == (0 if which == "bleed" else 1)
    assert np.isfinite(base["film"]).all() and base["film"][..., :3].max() > 0
    # pool 2^10 (a quarter of an image: slots are claimed again while other paths are live) against 2^16
    _assert_same(_run(golden_luts, scene, batch=1, pool=1 << 10), base, "pool 2^10")
    # image batch 4 against 1 (the sample textures read back are another image's: the film holds all four)
    _assert_same(_run(golden_luts, scene, batch=4), base, "batch 4", keys=("film",))
    _assert_same(_run(golden_luts, scene, batch=4, pool=1 << 12), base, "batch 4, pool 2^12", keys=("film",))
    # the early-finish routes: the long way, and both routes mixed in a wave
    for early in ("0", "2"):
        got = _run(golden_luts, scene, batch=1, early=early, pool=1 << 12)
        _assert_same(got, base, ("DCRT_EARLY_FINISH", early))
        if which != "bleed":
            assert got["info"]["early_finish"] == int(early)
            assert (got["early_finished"] > 0) == (early == "2") and got["early_finished"] < base["early_finished"]
    if which == "cornell":
        # the roulette ended paths in front of their last ray: fewer early-finished paths than without it
        plain = new_tracer(golden_luts, scene, seed=1, batch=1)
        try:
            plain.reset_stats()
            plain.render_images(1, 4)
            assert 0 < base["early_finished"] < plain.counters()["early_finished"]
        finally:
            plain.destroy()
    # a two-band film: each band's owned rows are the full film's (its ray counts include the halo rows it traces)
    full = base
    total = None
    for y0, y1 in ((0, 24), (24, SIZE)):
        got = _run(golden_luts, scene, batch=1, bands=[(y0, y1)], pool=1 << 12)
        for key in ("position", "value", "rng"):
            assert same(got[key][y0:y1], full[key][y0:y1]), ("band", y0, y1, key)
        total = got["film"] if total is None else total + got["film"]
    assert same(total, full["film"])


# ---- g. fewer rays ---------------------------------------------------------------------------------------
def test_fewer_extension_rays(native_lib, golden_luts, tmp_path):
    scene = PS.with_case(PS.load("bleed", tmp_path), 3)
    rays = {}
    for label, roulette in (("off", None), ("on", THROUGHPUT)):
        t = new_tracer(golden_luts, scene, roulette=roulette)
        try:
            t.clear_film()
            t.reset_stats()
            t.render_images(0, 4)
            rays[label] = t.counters()
        finally:
            t.destroy()
    print("bleed B 3: extension rays on / off", rays["on"]["extension_rays"] / rays["off"]["extension_rays"],
          "shadow rays on / off", rays["on"]["shadow_rays"] / rays["off"]["shadow_rays"])
    assert rays["on"]["new_paths"] == rays["off"]["new_paths"]
    assert rays["on"]["extension_rays"] < rays["off"]["extension_rays"]
    assert rays["on"]["shadow_rays"] <= rays["off"]["shadow_rays"]
