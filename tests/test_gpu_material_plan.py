"""How MATERIAL is launched, as dcrt_tracer_get_info and the upload statistics show it, held to a
recorded table (golden/material_plan_info.json): the variant, the bytes of its LDS sections, the
shading-table bits in force and whether the shadow rays are tested inline -- for five tiny scenes under
every shading knob, one at a time against the defaults, with the any-hit feature bit, the counters and
the row probe on and off -- and, on Cornell with captured graphs, the graph invalidations of a series
of material and light edits. The table was recorded before the launch got a single owner; a change
of the planning code must reproduce every entry, the invalidation counts included."""
import ctypes as C
import json

import numpy as np
import pytest

import random_scenes as RS
from conftest import GOLDEN, cornell
from directcomputeraytracing_amd import _abi
from test_gpu_fused_shadow import POOL, env
from test_gpu_shading_tables import _single_use_scene

pytestmark = pytest.mark.gpu

TABLE = GOLDEN / "material_plan_info.json"
FIELDS = ("material_generic", "material_lds", "shadow_inline", "shading_tables", "dielectric_row_bytes", "dielectric_row_lds",
          "frame_table_bytes")
ANYHIT = _abi.FEATURE_DEFAULT | _abi.FEATURE_ALLOW_ANYHIT
SCENES = ("cornell", "transformed instance", "blas used twice", "plastic obj", "65 materials")


def _scene(name, directory):
    """(scene, upload(tracer)) of one of SCENES."""
    from directcomputeraytracing_amd import Scene
    directory.mkdir(parents=True, exist_ok=True)
    scene, materials = None, None
    if name == "cornell":
        scene = cornell(16, 16, 4)
    elif name == "transformed instance":
        scene = _single_use_scene(directory, 7)
    elif name == "blas used twice":
        scene = Scene((48, 36))
        scene.load_from_file(RS.write_xml_scene(directory, 5, n_grid=2, n_loose=2, n_instances=2))
    else:
        scene = RS.setup_obj_scene(Scene((48, 36)), RS.write_obj_scene(directory, 11), 11)
        scene.set_material(0, _abi.MATERIAL_PLASTIC, (0.6, 0.4, 0.2), 0.3, (1.5, 1.5, 1.5))
        if name == "65 materials":
            flat = scene.flat()
            n = flat.material_count
            materials = (_abi.Material * 65)(*([flat.materials[i] for i in range(n)] + [flat.materials[0]] * (65 - n)))

    def upload(t):
        f = scene.flat()
        if materials is not None:
            f.materials, f.material_count = materials, 65
        assert t._lib.dcrt_tracer_upload_scene(t._h, C.byref(f)) == 0
        t.set_frame_params(scene.frame_params(1))
        t.filter = scene.filter_params()

    return scene, upload


def _knob_cases(scene, material_count):
    """The knob settings, one at a time against the defaults; the LDS budget between the scene's shading
    copy without and with the triangles (16 (9 T + 3 I) + 4 (2 I + 13 M + 7 L) bytes)."""
    f = scene.flat()
    rest = 48 * f.instance_count + 4 * (2 * f.instance_count + 13 * material_count + 7 * f.light_count)
    cases = {"defaults": {},
             "DCRT_MATERIAL_LDS=0": {"DCRT_MATERIAL_LDS": "0"},
             "DCRT_MATERIAL_LDS=between": {"DCRT_MATERIAL_LDS": str(rest + 72 * f.triangle_count)},
             "DCRT_MATERIAL_LDS_PARTIAL=0": {"DCRT_MATERIAL_LDS_PARTIAL": "0"},
             "DCRT_MATERIAL_LDS=between,PARTIAL=0": {"DCRT_MATERIAL_LDS": str(rest + 72 * f.triangle_count), "DCRT_MATERIAL_LDS_PARTIAL": "0"},
             "DCRT_MATERIAL_GENERIC=1": {"DCRT_MATERIAL_GENERIC": "1"},
             "DCRT_SHADOW_CELLS=0": {"DCRT_SHADOW_CELLS": "0"}}
    for v in (0, 1, 4):
        cases[f"DCRT_FUSED_SHADOW={v}"] = {"DCRT_FUSED_SHADOW": str(v)}
    for v in (0, 1, 2, 4, 7):
        cases[f"DCRT_SHADING_TABLES={v}"] = {"DCRT_SHADING_TABLES": str(v)}
    return cases


def _info(t):
    info = t.info()
    return {k: info[k] for k in FIELDS}


def collect_uploads(luts, directory):
    """{scene: {knob case: {launch case: info fields}}}: upload alone, no render."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    out = {}
    t = WavefrontPathTracer(path_pool_size=POOL, iterations_per_render=8)
    try:
        t.set_luts(luts)
        for name in SCENES:
            scene, upload = _scene(name, directory / name.replace(" ", "_"))
            material_count = 65 if name == "65 materials" else scene.material_count
            out[name] = {}
            for case, knobs in _knob_cases(scene, material_count).items():
                with env(**knobs):
                    upload(t)
                launches = {"plain": _info(t)}
                params = scene.frame_params(1)
                params.features = ANYHIT
                t.set_frame_params(params)
                launches["anyhit"] = _info(t)
                t.set_frame_params(scene.frame_params(1))
                t.set_instrumentation(True, False)
                launches["counters"] = _info(t)
                t.set_instrumentation(False, False)
                t.set_row_cost_probe(True)
                launches["row probe"] = _info(t)
                t.set_row_cost_probe(False)
                launches["plain again"] = _info(t)
                out[name][case] = launches
    finally:
        t.destroy()
    return out


def collect_edits(luts):
    """[(edit, graph invalidations it caused, info fields after it)] on Cornell with captured graphs."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    scene = cornell(16, 16, 4)
    mesh = _abi.Light()
    mesh.radiance[:] = (40.0, 36.0, 30.0)
    mesh.position_or_triangle_range[:] = np.array([0, 2, 0], np.uint32).view(np.float32).tolist()   # triangles [0, 2) of instance 0
    mesh.flags = 0x2                                                         # DCRT_LIGHT_FLAGS_MESH_LIGHT
    mesh_lights = (_abi.Light * 1)(mesh)
    out = []
    t = WavefrontPathTracer(path_pool_size=POOL, iterations_per_render=8)
    try:
        t.set_luts(luts)
        t.on_scene_loaded(scene, 1)
        scene.acquire_dirty()
        t.clear_film()
        t.render_images(1, 1)
        out.append(("uploaded and rendered", 0, _info(t)))

        def record(what, apply):
            before = t.upload_stats()["graph_invalidations"]
            apply()
            t.render_images(1, 1)      # (graphs exist again before the next edit)
            out.append((what, t.upload_stats()["graph_invalidations"] - before, _info(t)))

        def materials(*args):
            scene.set_material(*args)
            t.apply_edits(scene, scene.acquire_dirty(), 1)

        m = scene.material_setting(2)
        record("albedo of a plastic material", lambda: materials(2, _abi.MATERIAL_PLASTIC, (0.3, 0.5, 0.7), m.roughness, tuple(m.ior)))
        record("a material becomes glass", lambda: materials(3, _abi.MATERIAL_DIELECTRIC, (1.0, 1.0, 1.0), 0.2, (1.5, 1.5, 1.5)))
        record("roughness of a plastic material", lambda: materials(2, _abi.MATERIAL_PLASTIC, (0.3, 0.5, 0.7), 0.37, (1.9, 1.9, 1.9)))
        record("point light to mesh light", lambda: t._lib.dcrt_tracer_update_lights(t._h, mesh_lights, 1))
        record("mesh light back to the point light", lambda: t.update_lights(scene))
        record("the glass becomes diffuse again", lambda: materials(3, _abi.MATERIAL_DIFFUSE, (0.5, 0.5, 0.5), 1.0))
    finally:
        t.destroy()
    return [list(e) for e in out]


def collect(luts, directory):
    return {"uploads": collect_uploads(luts, directory), "edits": collect_edits(luts)}


@pytest.fixture(scope="module")
def recorded():
    return json.loads(TABLE.read_text())


def test_every_upload_plans_material_as_recorded(recorded, golden_luts, tmp_path):
    got = collect_uploads(golden_luts, tmp_path)
    assert sorted(got) == sorted(recorded["uploads"]) == sorted(SCENES)
    for name in SCENES:
        assert sorted(got[name]) == sorted(recorded["uploads"][name]), name
        for case, launches in got[name].items():
            assert launches == recorded["uploads"][name][case], (name, case)
    # (the table does cover what it is there for: each mode, the fused variant, rows and frames in and out of LDS)
    flat = [i for s in recorded["uploads"].values() for c in s.values() for i in c.values()]
    for field in FIELDS:
        assert len({i[field] for i in flat}) > 1, field
    assert any(i["dielectric_row_bytes"] and not i["dielectric_row_lds"] for i in flat)
    for case in recorded["uploads"]["cornell"].values():
        assert case["anyhit"]["shadow_inline"] == case["counters"]["shadow_inline"] == case["row probe"]["shadow_inline"] == 0
        assert case["plain again"] == case["plain"]


def test_edits_drop_the_graphs_exactly_as_recorded(recorded, golden_luts):
    got = collect_edits(golden_luts)
    assert len(got) == len(recorded["edits"]) == 7
    for g, want in zip(got, recorded["edits"]):
        assert g == want, g[0]
