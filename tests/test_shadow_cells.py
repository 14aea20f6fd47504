"""The point light's direction-cell table on the host (dcrt_shadow_cells_build, shadow_cells.h).

For the Cornell box and 20 seeded rooms, 2 * 10^5 shadow rays each (shadow_cell_rays.ray_set):
* every leaf whose own box and triangle a ray hits in float32 is in the mask of the ray's cell --
  zero misses;
* the OR over the masked leaves of (leaf box, guard boxes, triangle) is the oracle's any-hit
  traversal, ray for ray. (The guards carry weight: answered without them, 3 of the Cornell rays
  and 134 of the rooms' differ from the oracle -- rays that pass a leaf's box inside the ulp by which
  a rounded ancestor box misses it.)
Scenes outside the scheme build no table."""
import numpy as np
import pytest

import shadow_cell_rays as R
from directcomputeraytracing_amd import _abi

SEEDS = list(range(20))
RES = 32                # the build's default cube-map resolution (DCRT_SHADOW_CELLS)


def _check(scene, light, seed, oracle_mod, expect_reach=True):
    table = scene.shadow_cells()
    assert table is not None, _abi.load_library().dcrt_last_error()
    res = table["resolution"]
    assert res == RES and table["leaf_count"] <= 64
    rays = R.ray_set(scene, light, seed)
    assert len(rays) > 0.95 * R.RAYS_PER_SCENE
    o, d, t_max = rays["origin"], rays["direction"], rays["t_max"]
    assert (((d == 0).sum(1) == 1).sum() > 1000) and (((d == 0).sum(1) == 2).sum() > 1000)
    inv = R.inv_dir(d)
    masks = table["cells"].reshape(-1)[scene.shadow_cell_indices(res, -d)]
    tri = R.scene_triangles(scene)
    missed = 0
    reached = np.zeros(len(rays), bool)      # some leaf passes both tests
    answer = np.zeros(len(rays), bool)       # the table's answer: masked leaves, with their guards
    for k, (box, t, guards) in enumerate(R.leaves_of(table)):
        idx = np.nonzero(R.slab(o, inv, t_max, box))[0]
        idx = idx[R.watertight(o[idx], d[idx], inv[idx], t_max[idx], tri[t])]
        in_mask = (masks[idx] >> np.uint64(k)) & np.uint64(1) != 0
        missed += int((~in_mask).sum())
        reached[idx] = True
        idx = idx[in_mask]
        for g in guards:
            idx = idx[R.slab(o[idx], inv[idx], t_max[idx], g)]
        answer[idx] = True
    assert missed == 0, f"{missed} (ray, leaf) pairs pass the leaf's box and triangle outside the cell's mask"
    want, _ = oracle_mod.occluded(scene.flat(), rays, _abi.FEATURE_DEFAULT)
    bad = np.nonzero(answer != (want != 0))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(rays)} occlusion bits differ from the oracle's traversal, first {bad[:5]}"
    if expect_reach:
        assert 0.05 < answer.mean() < 0.95   # (both answers occur)
    return table, rays


def test_cornell_table_is_a_superset_and_answers_as_the_oracle(native_lib, oracle_mod):
    scene, light = R.cornell_scene()
    table, _ = _check(scene, light, 99, oracle_mod)
    assert table["leaf_count"] == 32
    assert table["mean_leaves"] < 8.0    # (the cost estimate's premise: a handful of leaves per cell)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_rooms_table_is_a_superset_and_answers_as_the_oracle(seed, tmp_path, native_lib, oracle_mod):
    scene, light = R.room_scene(tmp_path, seed)
    _check(scene, light, seed, oracle_mod)


def _no_table(scene):
    assert scene.shadow_cells() is None
    return _abi.load_library().dcrt_last_error().decode()


def test_ineligible_scenes_build_no_table(tmp_path, native_lib):
    scene, light = R.room_scene(tmp_path / "base", 1)
    assert scene.shadow_cells() is not None
    r0 = scene.shadow_cells()["r0"]
    scene.add_point_light((0.2, 1.2, 2.0), (1.0, 1.0, 1.0))
    scene.flatten()
    assert "one point light" in _no_table(scene)                            # two lights
    scene, _ = R.room_scene(tmp_path / "dir", 1)
    scene.remove_punctual_light(0)
    scene.add_directional_light((0.6, 0.3, 0.0), (1.0, 1.0, 1.0))
    scene.flatten()
    assert "one point light" in _no_table(scene)                            # not a point light
    groups, light, triangles = R.room_groups(2, boxes=5, quads=3)
    assert triangles > 64
    scene = R.Scene((32, 24))
    scene.load_from_file(R.write_obj(tmp_path / "many", groups))
    scene.add_point_light(light, (1.0, 1.0, 1.0))
    scene.flatten()
    assert "64" in _no_table(scene)                                         # 65 leaves or more
    # a triangle closer to the light than r0: the light just under the ceiling
    scene, _ = R.room_scene(tmp_path / "near", 3)
    y1 = float(R.scene_triangles(scene)[:, :, 1].max())
    scene.remove_punctual_light(0)
    scene.add_point_light((0.1, y1 - 0.5 * r0, 2.5), (1.0, 1.0, 1.0))
    scene.flatten()
    assert "r0" in _no_table(scene)
    scene.remove_punctual_light(0)
    scene.add_point_light((0.1, y1 - 4.0 * r0, 2.5), (1.0, 1.0, 1.0))
    scene.flatten()
    assert scene.shadow_cells() is not None


def test_triangle_emitter_and_rotated_instance_build_no_table(tmp_path, native_lib):
    import random_scenes
    from directcomputeraytracing_amd import Scene
    # an XML scene: an area emitter (a mesh light) and transformed instances
    scene = Scene((32, 24))
    scene.load_from_file(random_scenes.write_xml_scene(tmp_path, 5, 32, 24, n_grid=2, n_loose=2, n_instances=2))
    scene.flatten()
    assert scene.flat().light_count >= 1
    reason = _no_table(scene)
    assert "light" in reason or "identity" in reason
    # the same scene with its lights replaced by one point light: the rotated instances refuse it
    flat = scene.flat()
    light = (_abi.Light * 1)()
    light[0].radiance[:] = (1.0, 1.0, 1.0)
    light[0].position_or_triangle_range[:] = (0.0, 5.0, 0.0)
    light[0].flags = 1
    flat.lights, flat.light_count = light, 1
    info = _abi.ShadowCellsInfo()
    import ctypes as C
    _abi.check(_abi.load_library().dcrt_shadow_cells_build(C.byref(flat), 0, C.byref(info), None, None, None, 0))
    assert info.resolution == 0
    assert "identity" in _abi.load_library().dcrt_last_error().decode()
