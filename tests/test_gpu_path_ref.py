"""The device held to the path-truth fixture (tests/golden/path_truth.json, produced by tests/path_ref.py:
a float64 estimator of the expected sample radiance that shares no code with the kernels or the oracle), in
wavefront and in megakernel mode: per scene and mode, first one image bit-identical to the oracle's (parity
extended to delta chains, mixed lights and opacity draws inside paths), then the four quadrant means of
PS.SCENES[name]["images"] images of 64 x 64 per case against the fixture, by the rule of
tests/test_path_ref.py, z from this file's own number of comparisons. The fixture's standard error is asserted to be at most the device side's on every
statistic that has any. Nothing outside the repository tree is read."""
import numpy as np
import pytest

import path_ref as PR
import path_scenes as PS
from test_gpu_parity import same_bits
from test_path_ref import NAN_CAP, cases, within, z_bound

pytestmark = pytest.mark.gpu


def comparisons():
    """The statistical comparisons of this file: both modes of every case (4 quadrants x 3 channels), and the
    sheet's cases once more under importance sampling."""
    return 2 * sum(len(cases(n)) * 12 for n in PS.SCENES) + len(cases("sheet")) * 12


def _device_samples(t, images):
    out = []
    for seed in range(images):
        t.clear_film()
        t.render_images(seed, 1)
        out.append(t.read_samples()[1][..., :3].copy())
    return np.stack(out)


def _held_to_fixture(name, mode, oracle_mod, golden_luts, tmp_path, sampling=None):
    from directcomputeraytracing_amd import WavefrontPathTracer
    fixture = PR.load_fixture()
    scene = PS.load(name, tmp_path)
    images = PS.SCENES[name]["images"]
    z = z_bound(comparisons())
    t = WavefrontPathTracer(path_pool_size=1 << 16)
    try:
        t.set_luts(golden_luts)
        first = True
        for vis, b in cases(name):
            PS.with_case(scene, b, vis)
            t.on_scene_loaded(scene)
            t.set_mode(mode)
            if sampling:
                t.set_environment_sampling(sampling)
            v = _device_samples(t, images)
            if first and not sampling:             # (the oracle samples the environment uniformly)
                ref = oracle_mod.render(oracle_mod.flat_with_own_bvh(scene), golden_luts, oracle_mod.frame_params(scene, 0),
                                        oracle_mod.MEGAKERNEL if mode == "megakernel" else oracle_mod.WAVEFRONT)[1][..., :3]
                bad = np.count_nonzero(~same_bits(v[0], ref).all(-1))
                assert bad == 0, f"{name} {mode}: {bad} samples of image 0 differ from the oracle's"
                first = False
            mean, sem, _, nan = PR.quadrant_statistics(v)
            want, want_sem = PR.fixture_entry(fixture, name, vis, b)
            ok, worst = within(mean, sem, want, want_sem, z)
            ratio = float((want_sem[sem > 0] / sem[sem > 0]).max())
            print(name, mode, sampling or "", "visible" if vis else "hidden", "B", b, "mean", mean.mean(0).round(5), "sem", sem.max(0).round(5),
                  "NaN share", nan, "worst |difference| / bound", round(worst, 3), "sem ratio fixture / device", round(ratio, 3))
            assert nan <= NAN_CAP, (name, mode, vis, b, nan)
            assert sampling or ratio <= 1.0, (name, mode, vis, b, ratio)     # (the path counts were chosen for the default sampling)
            assert ok, (name, mode, vis, b, worst, mean, want)
    finally:
        t.destroy()


@pytest.mark.parametrize("mode", ["wavefront", "megakernel"])
@pytest.mark.parametrize("name", list(PS.SCENES))
def test_device_means_are_the_fixtures(native_lib, oracle_mod, golden_luts, tmp_path, name, mode):
    _held_to_fixture(name, mode, oracle_mod, golden_luts, tmp_path)


def test_sheet_with_environment_importance_sampling(native_lib, oracle_mod, golden_luts, tmp_path):
    """Importance sampling of the environment cube changes the light strategy, not the expectation (both of its
    pdfs are the true density: m = 1), so the uniform run's fixture holds it too."""
    _held_to_fixture("sheet", "wavefront", oracle_mod, golden_luts, tmp_path, sampling="importance")
