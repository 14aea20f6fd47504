"""The merged cast's streaming shadow section (cast_kernel<..., CELLS>) on the GPU: the direction-cell
answer is the BVH walk's, bit for bit -- per ray (trace_occlusion_cells against occluded), per film and
counter (the default build against DCRT_SHADOW_CELLS=0), and across light edits."""
import os

import numpy as np
import pytest

import shadow_cell_rays as R
from conftest import cornell
from directcomputeraytracing_amd import _abi

pytestmark = pytest.mark.gpu

POOL = 1 << 16
RES = 32                # the build's default cube-map resolution (DCRT_SHADOW_CELLS)
NO_WATERTIGHT = _abi.FEATURE_DEFAULT & ~_abi.FEATURE_WATERTIGHT


def new_tracer(luts, cells=True):
    """A fresh tracer; cells=False: one whose uploads read DCRT_SHADOW_CELLS=0."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=POOL, iterations_per_render=8)
    t.set_luts(luts)
    t.cells = cells
    return t


def load(t, scene, seed=0):
    old = os.environ.get("DCRT_SHADOW_CELLS")
    if not t.cells:
        os.environ["DCRT_SHADOW_CELLS"] = "0"
    try:
        t.on_scene_loaded(scene, seed)
    finally:
        if not t.cells:
            if old is None:
                del os.environ["DCRT_SHADOW_CELLS"]
            else:
                os.environ["DCRT_SHADOW_CELLS"] = old


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("which", ["cornell", 0, 3, 12, 15])
def test_cell_occlusion_bits_are_the_bvh_walks(which, tmp_path, gpu_tracer):
    # (rooms of the Cornell box's size, 30 triangles: the whole scene sits in the cast's LDS)
    scene, light = R.cornell_scene() if which == "cornell" else R.room_scene(tmp_path, which, boxes=2, quads=0)
    gpu_tracer.on_scene_loaded(scene)
    info = gpu_tracer.info()
    assert info["cast_identity"] == 2, info
    assert info["shadow_cells"] == RES, info
    assert 0.0 < info["shadow_cell_mean_leaves"] <= info["shadow_cell_max_leaves"] <= 64
    rays = R.ray_set(scene, light, 7 if which == "cornell" else which)
    for features in (_abi.FEATURE_DEFAULT, NO_WATERTIGHT):
        got, want = gpu_tracer.occluded_cells(rays, features), gpu_tracer.occluded(rays, features)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"features {features:#x}: {len(bad)} of {len(rays)} bits differ, first {bad[:5]}"
        assert 0.05 < want.mean() < 0.95


def test_no_table_is_an_error(gpu_tracer, tmp_path):
    scene, light = R.room_scene(tmp_path, 1, boxes=2, quads=0)
    scene.add_point_light((0.2, 1.2, 2.0), (1.0, 1.0, 1.0))
    gpu_tracer.on_scene_loaded(scene)
    assert gpu_tracer.info()["shadow_cells"] == 0
    with pytest.raises(_abi.DCRTError):
        gpu_tracer.occluded_cells(R.ray_set(scene, light, 1, 1000))


def _film(tracers, scene, images=3):
    out = None
    for t in tracers:
        t.set_frame_params(scene.frame_params(1))
        t.clear_film()
        t.reset_stats()
        t.render_images(1, images)
        f = t.read_film()
        out = f if out is None else out + f
    return out, [t.counters() for t in tracers]


@pytest.mark.parametrize("watertight", [True, False])
@pytest.mark.parametrize("pipelines", [1, 2])
def test_films_and_counters_equal_the_bvh_builds(watertight, pipelines, golden_luts):
    scene = cornell(128, 128, 8)
    if not watertight:
        scene.features = NO_WATERTIGHT
    bands = [[(0, 128)]] if pipelines == 1 else [[(0, 64)], [(64, 128)]]
    results = {}
    for cells in (True, False):
        tracers = [new_tracer(golden_luts, cells) for _ in bands]
        try:
            for t, b in zip(tracers, bands):
                load(t, scene, 1)
                if pipelines > 1:
                    t.set_film_bands(b, 2)
                assert (t.info()["shadow_cells"] != 0) == cells
            results[cells] = _film(tracers, scene)
        finally:
            for t in tracers:
                t.destroy()
    assert same_bits(results[True][0], results[False][0])
    assert results[True][1] == results[False][1]
    assert all(c["shadow_rays"] > 0 and c["images_completed"] == 3 for c in results[True][1])
    assert np.isfinite(results[True][0]).all() and results[True][0][..., :3].max() > 0


def test_light_edits_rebuild_and_drop_the_table(golden_luts):
    scene = cornell(96, 80, 6)
    t = new_tracer(golden_luts)
    try:
        load(t, scene, 1)
        scene.acquire_dirty()
        assert t.info()["shadow_cells"] == RES
        _film([t], scene, 1)              # (graphs exist before the edits)

        def against_fresh(what, cells_on):
            t.apply_edits(scene, scene.acquire_dirty(), 1)
            got = _film([t], scene, 2)
            for fresh_cells in (True, False):
                f = new_tracer(golden_luts, fresh_cells)
                try:
                    load(f, scene, 1)
                    assert (f.info()["shadow_cells"] != 0) == (fresh_cells and cells_on), what
                    if fresh_cells:
                        assert f.info() == t.info(), what
                    want = _film([f], scene, 2)
                finally:
                    f.destroy()
                assert same_bits(got[0], want[0]), what
                assert got[1] == want[1], what

        position, euler, color, directional = scene.punctual_lights()[0]
        scene.set_punctual_light(0, (-0.6, 1.7, 2.4), euler, color, directional)
        against_fresh("point light moved", True)
        scene.add_point_light((0.7, 1.5, 2.0), (1.0, 0.9, 0.8))
        against_fresh("second light added", False)
        assert t.info()["shadow_cells"] == 0
        scene.remove_punctual_light(1)
        against_fresh("second light removed", True)
        assert t.info()["shadow_cells"] == RES
    finally:
        t.destroy()
