"""MATERIAL's fused variant (material_kernel's FUSED: a shadow ray of a scene with direction cells is
tested beside the shading instead of travelling through the shadow queue) on the GPU: films and
counters are the unfused path's bit for bit -- with every ray inline (the default), with none
(DCRT_FUSED_SHADOW=0) and with both routes mixed in a wave (the test value) -- and the oracle's; the
variant is launched exactly with the CELLS cast, and follows the table across light edits."""
import os

import numpy as np
import pytest

import shadow_cell_rays as R
from conftest import cornell
from directcomputeraytracing_amd import _abi

pytestmark = pytest.mark.gpu

POOL = 1 << 12          # smaller than film x images: slots recycle, batches follow one another
RES = 32                # the build's default cube-map resolution (DCRT_SHADOW_CELLS)
NO_WATERTIGHT = _abi.FEATURE_DEFAULT & ~_abi.FEATURE_WATERTIGHT
DEFAULT, OFF, MIXED = None, "0", "2"     # DCRT_FUSED_SHADOW: unset, off, odd path slots take the queue


class env:
    """Environment variables for the length of a block (the knobs are read at uploads and edits)."""

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


def new_tracer(luts, scene, fused=DEFAULT, seed=1, bands=None, **knobs):
    """A fresh tracer with the scene loaded under DCRT_FUSED_SHADOW=`fused` (and further knobs)."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=POOL, iterations_per_render=8)
    try:
        t.set_luts(luts)
        with env(DCRT_FUSED_SHADOW=fused, **knobs):
            t.on_scene_loaded(scene, seed)
        if bands is not None:
            t.set_film_bands(bands, 2)
    except BaseException:
        t.destroy()
        raise
    return t


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def film_of(tracers, scene, images=3):
    """(the tracers' films summed, their counters) after `images` images from seed 1."""
    out = None
    for t in tracers:
        t.set_frame_params(scene.frame_params(1))
        t.clear_film()
        t.reset_stats()
        t.render_images(1, images)
        f = t.read_film()
        out = f if out is None else out + f
    return out, [t.counters() for t in tracers]


def render_fresh(luts, scene, fused, band_sets=(None,), images=3, prepare=None, **knobs):
    """Film, counters and info() of fresh tracers (one per band set) under one setting."""
    tracers = []
    try:
        for bands in band_sets:
            tracers.append(new_tracer(luts, scene, fused, bands=bands, **knobs))
        for t in tracers:
            t.set_frame_params(scene.frame_params(1))
            if prepare:
                prepare(t)
        infos = [t.info() for t in tracers]
        film, counters = film_of(tracers, scene, images)
        return film, counters, infos
    finally:
        for t in tracers:
            t.destroy()


@pytest.mark.parametrize("pipelines", [1, 2])
@pytest.mark.parametrize("watertight", [True, False])
@pytest.mark.parametrize("bounces", [1, 2, 8])
def test_films_and_counters_equal_the_unfused_path(bounces, watertight, pipelines, golden_luts):
    # (max bounce 1: every shadow ray belongs to a path that ends with it -- the finish queue's route)
    scene = cornell(96, 80, bounces)
    if not watertight:
        scene.features = NO_WATERTIGHT
    band_sets = (None,) if pipelines == 1 else ([(0, 40)], [(40, 80)])
    runs = {}
    for fused in (DEFAULT, OFF, MIXED):
        film, counters, infos = render_fresh(golden_luts, scene, fused, band_sets)
        assert all(i["shadow_cells"] == RES for i in infos), infos
        assert all(i["shadow_inline"] == (0 if fused == OFF else 1) for i in infos), (fused, infos)
        runs[fused] = (film, counters)
    for fused in (DEFAULT, MIXED):
        assert same_bits(runs[fused][0], runs[OFF][0]), fused
        assert runs[fused][1] == runs[OFF][1], fused
    assert all(c["shadow_rays"] > 0 and c["images_completed"] == 3 for c in runs[DEFAULT][1])
    assert np.isfinite(runs[DEFAULT][0]).all() and runs[DEFAULT][0][..., :3].max() > 0


def test_film_and_ray_counts_are_the_oracles(golden_luts, oracle_mod):
    from directcomputeraytracing_amd import FILTER_BOX, FilterParams
    scene = cornell(96, 80, 8)
    filt = FilterParams(FILTER_BOX, 1.0, 1.5, 1 / 3, 1 / 3, 3)
    flat = oracle_mod.flat_with_own_bvh(scene)
    ref, ext, shadow = None, 0, 0
    for seed in (1, 2, 3):
        p, v, _, c = oracle_mod.render(flat, golden_luts, oracle_mod.frame_params(scene, seed), oracle_mod.WAVEFRONT)
        if ref is None:
            ref = np.zeros((80, 96, 4), np.float32)
        oracle_mod.sample_convolution(filt, p, v, ref)
        ext += c["extension_rays"]
        shadow += c["shadow_rays"]
    for fused in (DEFAULT, MIXED):
        t = new_tracer(golden_luts, scene, fused)
        try:
            assert t.info()["shadow_inline"] == 1
            t.set_frame_params(scene.frame_params(1))
            t.clear_film()
            t.reset_stats()
            t.render_images(1, 3, filt)
            film, c = t.read_film(), t.counters()
        finally:
            t.destroy()
        assert film.shape == ref.shape
        assert same_bits(film, ref), fused
        assert (c["extension_rays"], c["shadow_rays"], c["new_paths"]) == (ext, shadow, 3 * 96 * 80), fused


def _second_light(scene):
    scene.add_point_light((0.7, 1.5, 2.0), (1.0, 0.9, 0.8))


def _anyhit(scene):
    scene.features = _abi.FEATURE_DEFAULT | _abi.FEATURE_ALLOW_ANYHIT


@pytest.mark.parametrize("what", ["second point light", "any-hit", "counters", "no cells"])
def test_ineligible_launches_keep_the_queue(what, golden_luts):
    scene = cornell(96, 80, 4)
    knobs, prepare = {}, None
    if what == "second point light":
        _second_light(scene)
    elif what == "any-hit":
        _anyhit(scene)
    elif what == "counters":
        prepare = lambda t: t.set_instrumentation(True, False)
    else:
        knobs["DCRT_SHADOW_CELLS"] = "0"
    runs = {}
    for fused in (DEFAULT, OFF):
        film, counters, infos = render_fresh(golden_luts, scene, fused, images=2, prepare=prepare, **knobs)
        assert infos[0]["shadow_inline"] == 0, (what, fused, infos[0])
        runs[fused] = (film, counters)
    assert same_bits(runs[DEFAULT][0], runs[OFF][0])
    assert runs[DEFAULT][1] == runs[OFF][1]
    assert runs[DEFAULT][1][0]["shadow_rays"] > 0 and runs[DEFAULT][0][..., :3].max() > 0


def test_light_edits_switch_the_variant(golden_luts):
    scene = cornell(96, 80, 6)
    t = new_tracer(golden_luts, scene)
    try:
        scene.acquire_dirty()
        assert t.info()["shadow_cells"] == RES and t.info()["shadow_inline"] == 1
        film_of([t], scene, 1)              # (graphs exist before the edits)

        def against_fresh(what, table):
            t.apply_edits(scene, scene.acquire_dirty(), 1)
            info = t.info()
            assert (info["shadow_cells"] != 0) == table and info["shadow_inline"] == (1 if table else 0), (what, info)
            got = film_of([t], scene, 2)
            for fused in (DEFAULT, OFF):
                f = new_tracer(golden_luts, scene, fused)
                try:
                    if fused == DEFAULT:
                        assert f.info() == info, what
                    else:
                        assert f.info()["shadow_inline"] == 0, what
                    want = film_of([f], scene, 2)
                finally:
                    f.destroy()
                assert same_bits(got[0], want[0]), (what, fused)
                assert got[1] == want[1], (what, fused)

        position, euler, color, directional = scene.punctual_lights()[0]
        scene.set_punctual_light(0, (-0.6, 1.7, 2.4), euler, color, directional)
        against_fresh("point light moved", True)
        _second_light(scene)
        against_fresh("second light added", False)
        scene.remove_punctual_light(1)
        against_fresh("second light removed", True)
    finally:
        t.destroy()


@pytest.mark.parametrize("which", [3, 12])
def test_random_rooms(which, tmp_path, golden_luts):
    # (two of test_cell_occlusion_bits_are_the_bvh_walks' rooms: 30 triangles, room 3 with its light
    # in the planes of a box's top and side)
    from directcomputeraytracing_amd import Scene
    groups, light, triangles = R.room_groups(which, boxes=2, quads=0)
    assert triangles == 30
    scene = Scene((64, 64))
    scene.reset(64, 64)
    scene.load_from_file(R.write_obj(tmp_path, groups))
    scene.add_point_light(light, (2.0, 2.0, 2.0))
    scene.set_max_bounce(4)
    runs = {}
    for fused in (DEFAULT, OFF, MIXED):
        film, counters, infos = render_fresh(golden_luts, scene, fused)
        assert infos[0]["shadow_cells"] == RES and infos[0]["shadow_inline"] == (0 if fused == OFF else 1), infos[0]
        runs[fused] = (film, counters)
    for fused in (DEFAULT, MIXED):
        assert same_bits(runs[fused][0], runs[OFF][0]), fused
        assert runs[fused][1] == runs[OFF][1], fused
    assert runs[DEFAULT][1][0]["shadow_rays"] > 0 and runs[DEFAULT][0][..., :3].max() > 0
