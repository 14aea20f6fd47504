"""The three ext_timing read-outs of the film stages (dcrt.h): denoise_timings, adaptive_timings and
film_pass_timing -- how many figures each reports, that they are finite and not negative while
ext_timing is on, and that they are empty or zero once it is off. The figures themselves are times:
nothing here holds them to a value."""
import math

import numpy as np
import pytest

from conftest import cornell
import adaptive_ref
import noise_ref

pytestmark = pytest.mark.gpu

W, H = 40, 24          # a multiple of neither the 16-pixel film / noise tile nor the 8-pixel block
BOUNCES = 2
POOL = 1 << 10


def new_tracer(golden_luts):
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=POOL, iterations_per_render=8)
    t.set_luts(golden_luts)
    t.on_scene_loaded(cornell(W, H, BOUNCES))
    return t


def is_time(ms) -> bool:
    return math.isfinite(ms) and ms >= 0.0


def test_denoise_timings(native_lib, golden_luts):
    from directcomputeraytracing_amd.tracer import denoise_default_params
    t = new_tracer(golden_luts)
    try:
        t.render_images(0, 2)
        t.render_guides(0, 1)
        p = denoise_default_params()
        p.iterations = 3
        t.set_instrumentation(False, True)
        t.denoise(p)
        ms = t.denoise_timings()
        print("denoise_timings", ms)
        assert len(ms) == 5, ms             # prologue, variance, 3 passes
        assert all(is_time(x) for x in ms), ms
        t.set_instrumentation(False, False)
        t.denoise(p)
        assert t.denoise_timings() == []
    finally:
        t.destroy()


def partial_threshold(oracle_mod, golden_luts, filt, images):
    """A threshold at which the block list of the film of `images` oracle images (margin 0) is neither
    empty nor full, from the CPU restatements alone."""
    film, half = noise_ref.films_of(oracle_mod, filt, noise_ref.cornell_images(oracle_mod, golden_luts, W, H, BOUNCES, range(images)))
    e, valid = noise_ref.pixel_error(film, half)
    total = len(adaptive_ref.all_blocks(W, H))
    # (a block leaves the list once the threshold reaches its largest error: the blocks' maxima, the middle one first)
    worst = np.where(valid & np.isfinite(e), e, np.inf)
    maxima = sorted({float(worst[y:y + 8, x:x + 8].max()) for y in range(0, H, 8) for x in range(0, W, 8)} - {math.inf})
    for threshold in sorted(maxima, key=lambda m: abs(maxima.index(m) - len(maxima) // 2)):
        _, active = adaptive_ref.active_blocks(film, half, threshold, 0)
        if 0 < len(active) < total:
            return threshold, active
    raise AssertionError("no threshold leaves a partial block list")


def test_adaptive_timings(native_lib, golden_luts, oracle_mod):
    t = new_tracer(golden_luts)
    try:
        filt = cornell(W, H, BOUNCES).filter_params()
        threshold, want = partial_threshold(oracle_mod, golden_luts, filt, 4)
        t.set_convergence(True)
        t.set_adaptive(True)
        t.set_instrumentation(False, True)
        t.render_images(0, 4, filt)
        assert t.update_sample_blocks(threshold, 0) == len(want)
        assert np.array_equal(t.get_sample_blocks(), want)
        ms = t.adaptive_timings()
        print("adaptive_timings (mask, compact)", ms)
        assert is_time(ms["mask_ms"]) and is_time(ms["compact_ms"]), ms
        t.render_images(4, 1, filt)         # a listed image: the sentinel fill runs first
        ms = t.adaptive_timings()
        print("adaptive_timings (fill)", ms)
        assert is_time(ms["fill_ms"]), ms
        t.set_instrumentation(False, False)
        assert 0 < t.update_sample_blocks(threshold, 0) < len(adaptive_ref.all_blocks(W, H))
        ms = t.adaptive_timings()
        assert ms["mask_ms"] == 0.0 and ms["compact_ms"] == 0.0, ms
        t.render_images(5, 1, filt)         # the list changed: the fill runs again, untimed
        assert t.adaptive_timings()["fill_ms"] == 0.0
    finally:
        t.destroy()


@pytest.mark.parametrize("convergence", [False, True])
def test_film_pass_timing(native_lib, golden_luts, convergence):
    """k accumulate_film calls are k timed launches, of film_kernel or (convergence on) of the kernel
    that also feeds the half film."""
    k = 3
    t = new_tracer(golden_luts)
    try:
        t.render_images(0, 1)               # samples in slot 0
        if convergence:
            t.set_convergence(True)
        t.set_instrumentation(False, True)
        t.reset_stats()
        for _ in range(k):
            t.accumulate_film()
        launches, ms = t.film_pass_timing()
        print("film_pass_timing", launches, ms)
        assert launches == k
        assert is_time(ms)
        assert t.film_image_count() == (k if convergence else k + 1)
    finally:
        t.destroy()
