"""Partial scene edits on the host: an edit re-flattens only its own arrays, reports the dirty
bits of the reference's UI (Scene.h:211-215, ImGui.cpp:322-372, 468-497, 596-657), and leaves
the flat scene byte for byte what a full flatten -- and the oracle's own flattening -- gives."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN, cornell

ARRAYS = ("vertices", "triangles", "bvh_nodes", "material_ids", "instance_transforms", "instance_light_indices",
          "instance_flags", "instance_material_overrides", "materials", "lights")
GEOMETRY = ("vertices", "triangles", "bvh_nodes")


def flat_arrays(f) -> dict:
    """Copies of every array of a dcrt_flat_scene as bytes-comparable uint32 arrays, with the scalars."""
    def copy(ptr, words):
        if not words or not ptr:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(words,)).copy()

    n = f.instance_count
    return {
        "vertices": copy(f.vertices, f.vertex_count * 11),
        "triangles": copy(f.triangles, f.triangle_count * 3),
        "bvh_nodes": copy(f.bvh_nodes, f.bvh_node_count * 8),
        "material_ids": copy(f.material_ids, f.triangle_count),
        "instance_transforms": copy(f.instance_transforms, n * 2 * 12),
        "instance_light_indices": copy(f.instance_light_indices, n),
        "instance_flags": copy(f.instance_flags, n),
        "instance_material_overrides": copy(f.instance_material_overrides, n),
        "materials": copy(f.materials, f.material_count * 13),
        "lights": copy(f.lights, f.light_count * 7),
        "scalars": (f.vertex_count, f.triangle_count, f.bvh_node_count, f.tlas_node_count, n, f.material_count, f.light_count,
                    f.environment_light_index, f.texture_count, f.env_cube_size, f.bvh_traversal_stack_size),
    }


def anyhit(resolution=(8, 8)):
    from directcomputeraytracing_amd import Scene
    s = Scene(resolution)
    s.load_from_file(GOLDEN / "anyhit" / "anyhit.xml")
    return s


def veil_index(s) -> int:
    opacity = s.arrays()["materials"][:, 10].view(np.float32)
    return int(np.flatnonzero(np.isclose(opacity, 0.4))[0])


def _material(s):
    s.set_material(3, 1, (0.8, 0.2, 0.2), 0.4, (1.5, 1.5, 1.5), None, False, True)


def _multiscattering(s):
    s.set_material(4, 2, (0.9, 0.6, 0.3), 0.3, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
    s.acquire_dirty()
    s.set_multiscattering(4, True)


def _opacity(s):
    s.set_material_opacity(2, 0.5)


def _add_point(s):
    s.add_point_light((0.3, 1.2, 2.0), (1.0, 2.0, 3.0))


def _add_directional(s):
    s.add_directional_light((0.6, 0.3, 0.0), (1.5, 1.4, 1.2))


def _move_point(s):
    s.set_punctual_light(0, (-0.4, 0.9, 3.1), (0, 0, 0), (3.0, 2.0, 1.0), False)


def _turn_directional(s):
    s.set_punctual_light(0, (0, 0, 0), (0.2, 0.7, 0.0), (1.0, 1.0, 1.0), True)


def _remove_point(s):
    s.remove_punctual_light(0)


def _environment_colour(s):
    s.set_environment_light((0.4, 0.5, 0.6))


def _environment_removed(s):
    s.set_environment_light((0.4, 0.5, 0.6))
    s.acquire_dirty()
    s.remove_environment_light()


def _camera(s):
    s.set_camera((0.1, 1.1, -2.5), (0.05, 0.1, 0.0))


def _lens(s):
    s.set_lens(0, 0.9, 0.05, 2.0, 8.0, 7, 0.0)


# the table of the issue (§1): edit -> the bits its setter leaves
L, M, F, CAM, SCENE = 0x01, 0x02, 0x04, 0x08, 0x10
EDITS = {
    "material": (_material, M), "multiscattering": (_multiscattering, M), "opacity": (_opacity, M | F),
    "add_point": (_add_point, L), "add_directional": (_add_directional, L), "move_point": (_move_point, L),
    "turn_directional": (_turn_directional, L), "remove_point": (_remove_point, L),
    "environment_colour": (_environment_colour, L), "environment_removed": (_environment_removed, L),
    "camera": (_camera, CAM), "lens": (_lens, CAM),
}


def test_dirty_constants_mirror_header(native_lib):
    from directcomputeraytracing_amd import Scene, _abi
    assert (Scene.DIRTY_LIGHTS, Scene.DIRTY_MATERIALS, Scene.DIRTY_INSTANCE_FLAGS, Scene.DIRTY_CAMERA, Scene.DIRTY_SCENE) == \
        (L, M, F, CAM, SCENE) == (_abi.DIRTY_LIGHTS, _abi.DIRTY_MATERIALS, _abi.DIRTY_INSTANCE_FLAGS, _abi.DIRTY_CAMERA,
                                  _abi.DIRTY_SCENE)


@pytest.mark.parametrize("kind", sorted(EDITS))
def test_edit_flattens_its_part_only_and_sets_its_bits(native_lib, oracle_mod, kind):
    edit, bits = EDITS[kind]
    s = cornell(48, 40, 4)
    assert s.acquire_dirty() & SCENE                      # (load and reset)
    before_flat = s.flat()
    before = flat_arrays(before_flat)
    geometry_ptrs = [C.cast(p, C.c_void_p).value for p in (before_flat.vertices, before_flat.triangles, before_flat.bvh_nodes,
                                                           before_flat.instance_transforms)]
    edit(s)
    assert s.acquire_dirty() == bits
    assert s.acquire_dirty() == 0
    f = s.flat()
    after = flat_arrays(f)
    # no vertex, triangle, node or transform was copied: same storage, same bytes
    assert geometry_ptrs == [C.cast(p, C.c_void_p).value for p in (f.vertices, f.triangles, f.bvh_nodes, f.instance_transforms)]
    for name in GEOMETRY + ("material_ids", "instance_transforms", "instance_light_indices", "instance_material_overrides"):
        assert np.array_equal(after[name], before[name]), name
    # the old way: the same edit on a freshly loaded scene, then every array flattened again
    old = cornell(48, 40, 4)
    edit(old)
    old.flatten()
    reference = flat_arrays(old.flat())
    for name in ARRAYS + ("scalars",):
        assert np.array_equal(after[name], reference[name]) if name != "scalars" else after[name] == reference[name], name
    # ... and the oracle's own flattening of the edited scene
    own = flat_arrays(oracle_mod.flatten_scene(s))
    for name in ARRAYS + ("scalars",):
        assert np.array_equal(after[name], own[name]) if name != "scalars" else after[name] == own[name], name
    if bits & (L | M | F):
        changed = [n for n in ARRAYS if not np.array_equal(after[n], before[n])]
        assert set(changed) <= {"materials", "lights", "instance_flags"}, changed
        assert changed or kind == "environment_removed"   # (that one adds the light, then removes it)


def test_opacity_edit_follows_into_instance_flags(native_lib, oracle_mod):
    s = anyhit()
    s.acquire_dirty()
    veil = veil_index(s)
    for opacity, opaque_instances in ((1.0, 4), (0.4, 3)):
        before = flat_arrays(s.flat())
        s.set_material_opacity(veil, opacity)
        assert s.acquire_dirty() == M | F
        after = flat_arrays(s.flat())
        assert int(np.count_nonzero(after["instance_flags"] & 1)) == opaque_instances
        own = flat_arrays(oracle_mod.flatten_scene(s))
        for name in ARRAYS:
            assert np.array_equal(after[name], own[name]), name
        for name in GEOMETRY:
            assert np.array_equal(after[name], before[name]), name
    # an opacity texture index is an opacity edit too
    s.set_material_opacity(veil, 1.0, 1)
    assert s.acquire_dirty() == M | F
    assert int(np.count_nonzero(flat_arrays(s.flat())["instance_flags"] & 1)) == 3


def test_cube_set_changed_or_cleared_is_dirty_scene(native_lib):
    from directcomputeraytracing_amd import DCRTError, scenes
    s = cornell(16, 16, 2)
    s.acquire_dirty()
    s.set_environment_light((1.0, 1.0, 1.0), scenes.env_cube(4))
    assert s.acquire_dirty() == SCENE                       # appears
    s.set_environment_light((1.0, 1.0, 1.0), scenes.env_cube(4, seed=7))
    assert s.acquire_dirty() == SCENE                       # changes
    s.set_environment_light((0.5, 0.5, 0.5))
    assert s.acquire_dirty() == SCENE                       # disappears (the light stays, constant)
    assert s.flat().env_cube_size == 0 and s.flat().light_count == 2
    s.set_environment_light((0.25, 0.5, 0.5))
    assert s.acquire_dirty() == L                           # the colour alone
    s.set_environment_light((1.0, 1.0, 1.0), scenes.env_cube(4))
    s.acquire_dirty()
    s.remove_environment_light()
    assert s.acquire_dirty() == SCENE                       # removed with its cube
    assert s.flat().light_count == 1 and s.flat().environment_light_index == 0xFFFFFFFF
    with pytest.raises(DCRTError, match="INVALID_ARG"):     # none left
        s.remove_environment_light()
    assert s.acquire_dirty() == 0
    s.reset(16, 16)
    assert s.acquire_dirty() == SCENE


def test_remove_first_of_three_punctual_lights_keeps_order(native_lib, oracle_mod):
    s = cornell(16, 16, 2)
    s.add_directional_light((0.6, 0.3, 0.0), (1.5, 1.4, 1.2))
    s.add_point_light((0.5, 0.5, 2.0), (0.1, 0.2, 0.3))
    three = s.punctual_lights()
    assert len(three) == 3
    lights = flat_arrays(s.flat())["lights"].reshape(3, 7)
    s.remove_punctual_light(0)
    assert s.punctual_lights() == three[1:]
    after = flat_arrays(s.flat())
    assert np.array_equal(after["lights"].reshape(2, 7), lights[1:])
    assert np.array_equal(after["lights"], flat_arrays(oracle_mod.flatten_scene(s))["lights"])
    assert s.frame_params(0).light_count == 2


def test_light_entry_points_refuse_bad_indices(native_lib):
    from directcomputeraytracing_amd import DCRTError
    s = cornell(16, 16, 2)
    s.acquire_dirty()
    for call in (lambda: s.set_punctual_light(1, (0, 0, 0), (0, 0, 0), (1, 1, 1)), lambda: s.remove_punctual_light(1),
                 lambda: s.remove_punctual_light(0xFFFFFFFF)):
        with pytest.raises(DCRTError, match="INVALID_ARG"):
            call()
    assert s.acquire_dirty() == 0 and len(s.punctual_lights()) == 1
    assert native_lib.dcrt_scene_acquire_dirty(s.handle, None) == -1
    assert native_lib.dcrt_scene_acquire_dirty(None, C.byref(C.c_uint32())) == -1
    assert native_lib.dcrt_scene_remove_environment_light(None) == -1
    assert native_lib.dcrt_scene_flatten(None) == -1
    from directcomputeraytracing_amd import Scene
    assert native_lib.dcrt_scene_flatten(Scene((8, 8)).handle) == -3   # no content yet


def test_tracer_update_calls_refuse_null_tracer_or_array(native_lib):
    """Checked before any device call: no GPU needed."""
    from directcomputeraytracing_amd import _abi
    s = cornell(16, 16, 2)
    f = s.flat()
    stats = _abi.UploadStats()
    assert native_lib.dcrt_tracer_update_materials(None, f.materials, f.material_count) == -1
    assert native_lib.dcrt_tracer_update_materials(None, None, f.material_count) == -1
    assert native_lib.dcrt_tracer_update_lights(None, f.lights, f.light_count) == -1
    assert native_lib.dcrt_tracer_update_lights(None, None, 1) == -1
    assert native_lib.dcrt_tracer_update_instance_flags(None, f.instance_flags, f.instance_count) == -1
    assert native_lib.dcrt_tracer_update_instance_flags(None, None, f.instance_count) == -1
    assert native_lib.dcrt_tracer_upload_stats(None, C.byref(stats)) == -1
