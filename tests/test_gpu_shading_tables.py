"""Scene-constant shading work taken out of MATERIAL's per-hit path (DCRT_SHADING_TABLES: bit 1, no
BSDF pdf for a delta light's sample; bit 2, the plastic dielectric LUT read from per-material float
rows; bit 4, the hit's normal / tangent / geometry normal from a per-triangle table) on the GPU: films and counters are bit for bit those of the per-hit code (DCRT_SHADING_TABLES=0)
under every setting, the rows follow material and LUT edits, the pdf comes back when a light edit
brings an area light, and the film is the oracle's."""
import ctypes as C
import itertools

import numpy as np
import pytest

import random_scenes as RS
import test_gpu_bsdf as B
from conftest import cornell
from directcomputeraytracing_amd import _abi
from test_gpu_fused_shadow import NO_WATERTIGHT, POOL, env, film_of, same_bits

pytestmark = pytest.mark.gpu

DEFAULT, OFF, PDF, ROWS, FRAMES = None, "0", "1", "2", "4"      # DCRT_SHADING_TABLES: unset (every bit), off, each bit alone
SETTINGS = (DEFAULT, OFF, PDF, ROWS, FRAMES)
BITS = {DEFAULT: 7, OFF: 0, PDF: 1, ROWS: 2, FRAMES: 4}
ROW_BYTES = 4 * 132                                # kDielRowFloats floats per material


def new_tracer(luts, upload, tables, **knobs):
    """A fresh tracer with the scene uploaded (by `upload(tracer)`) under DCRT_SHADING_TABLES=`tables`."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=POOL, iterations_per_render=8)
    try:
        t.set_luts(luts)
        with env(DCRT_SHADING_TABLES=tables, **knobs):
            upload(t)
    except BaseException:
        t.destroy()
        raise
    return t


def render_fresh(luts, scene, tables, images=3, upload=None, **knobs):
    """(film, counters, info()) of a fresh tracer under one setting."""
    t = new_tracer(luts, upload or (lambda t: t.on_scene_loaded(scene, 1)), tables, **knobs)
    try:
        t.set_frame_params(scene.frame_params(1))
        info = t.info()
        film, counters = film_of([t], scene, images)
        return film, counters, info
    finally:
        t.destroy()


def assert_all_settings_equal(luts, scene, rows, frames, images=3, **knobs):
    """Every setting's film and counters are the OFF setting's; info() reports the bits in force
    (`rows`: the scene has rows, i.e. a plastic material and at most 64 materials; `frames`: it has the
    frame table, i.e. no BLAS with two instances and the whole shading data in MATERIAL's LDS) and the
    tables' sizes. Returns the runs."""
    runs = {}
    for tables in SETTINGS:
        film, counters, info = render_fresh(luts, scene, tables, images, **knobs)
        want = BITS[tables] & (1 | (2 if rows else 0) | (4 if frames else 0))
        assert info["shading_tables"] == want, (tables, info)
        assert info["frame_table_bytes"] == (48 * scene.flat().triangle_count if want & 4 else 0), (tables, info)
        assert info["dielectric_row_bytes"] == (ROW_BYTES * scene.material_count if want & 2 else 0), (tables, info)
        assert info["dielectric_row_lds"] in (0, info["dielectric_row_bytes"]), (tables, info)
        runs[tables] = (film, counters, info)
    for tables in SETTINGS:
        assert same_bits(runs[tables][0], runs[OFF][0]), tables
        assert runs[tables][1] == runs[OFF][1], tables
    assert np.isfinite(runs[OFF][0]).all() and runs[OFF][0][..., :3].max() > 0
    return runs


@pytest.mark.parametrize("watertight", [True, False])
@pytest.mark.parametrize("bounces", [1, 2, 8])
def test_cornell_films_and_counters_equal_the_per_hit_code(bounces, watertight, golden_luts):
    scene = cornell(96, 80, bounces)
    if not watertight:
        scene.features = NO_WATERTIGHT
    runs = assert_all_settings_equal(golden_luts, scene, rows=True, frames=True)
    info = runs[DEFAULT][2]
    # (every Cornell material is plastic; the LDS scene copy holds the rows: 6 materials' cost no workgroup)
    assert info["material_generic"] == 0 and info["material_lds"] != 0 and info["dielectric_row_lds"] == 6 * ROW_BYTES, info
    assert all(c["shadow_rays"] > 0 and c["images_completed"] == 3 for c in runs[DEFAULT][1])


def test_cornell_without_the_lds_copy_reads_the_rows_from_global_memory(golden_luts):
    scene = cornell(96, 80, 4)
    runs = assert_all_settings_equal(golden_luts, scene, rows=True, frames=False, images=2, DCRT_MATERIAL_LDS="0")
    assert runs[DEFAULT][2]["material_lds"] == 0 and runs[DEFAULT][2]["dielectric_row_lds"] == 0


def _single_use_scene(directory, seed):
    """random_scenes' soup (smooth normals; 14 triangles) once, rotated, scaled and moved, with a rough
    plastic bound to the shape (the instance's material override), under a point light: the BLAS has one
    instance, the whole shading data fits MATERIAL's LDS and the delta-only variant shades it."""
    from directcomputeraytracing_amd import Scene
    from directcomputeraytracing_amd.scenes import _sensor, _xml, mitsuba_matrix
    rng = np.random.default_rng(seed)
    RS._write_soup(directory / "soup.obj", *RS.soup(rng, 2, 2))
    body = ('  <integrator type="path"><integer name="max_depth" value="5"/></integrator>\n'
            + _sensor("perspective", 48, 36, mitsuba_matrix((0.2, 1.4, -4.2), pitch=15, yaw=4), '    <float name="fov" value="50"/>\n')
            + "  " + RS._BSDFS[1].format(id="b0", c="0.7, 0.4, 0.2", a="0.3") + "\n"
            + '  <shape type="obj" id="soup0"><string name="filename" value="soup.obj"/><ref id="b0"/><transform name="to_world">'
            + f'<matrix value="{mitsuba_matrix((0.3, 0.1, -0.4), yaw=37, pitch=-20, scale=(1.3, 1.3, 1.3))}"/></transform></shape>\n'
)
    (directory / "single.xml").write_text(_xml(body))
    scene = Scene((48, 36))
    scene.load_from_file(directory / "single.xml")
    scene.add_point_light((0.4, 2.6, -1.2), (9.0, 8.0, 7.0))
    return scene


def test_transformed_smooth_instance_with_an_override_in_lds(tmp_path, golden_luts):
    scene = _single_use_scene(tmp_path, 7)
    flat = scene.flat()
    assert flat.instance_count == 1 and flat.instance_material_overrides[0] != 0xFFFFFFFF
    assert [flat.instance_transforms[0].m[k] for k in (0, 5, 10)] != [1.0, 1.0, 1.0]
    runs = assert_all_settings_equal(golden_luts, scene, rows=True, frames=True)
    info = runs[DEFAULT][2]
    # (mode 1: the triangles are part of the LDS copy -- 144 B each -- and the rows and frames sit behind it)
    assert info["material_generic"] == 0 and info["material_lds"] >= 144 * flat.triangle_count, info
    assert info["dielectric_row_lds"] == info["dielectric_row_bytes"] != 0, info
    assert all(c["shadow_rays"] > 0 for c in runs[DEFAULT][1])


@pytest.mark.parametrize("case", ["mode 1", "mode 2"])
def test_blas_with_two_instances_has_no_frame_table(case, tmp_path, golden_luts):
    """random_scenes' XML scenes instance one soup mesh twice (and one rectangle mesh for the floor and the
    area light): no frame table, rows for their plastic materials -- in the whole-scene LDS copy of the
    small soup, behind the copy without triangles of the larger one -- and the area light's samples are
    weighted with the BSDF pdf under every setting."""
    from directcomputeraytracing_amd import Scene
    scene = Scene((48, 36))
    if case == "mode 1":
        scene.load_from_file(RS.write_xml_scene(tmp_path, 5, n_grid=2, n_loose=2, n_instances=2))
    else:
        scene.load_from_file(RS.write_xml_scene(tmp_path, 3, n_grid=8, n_loose=4, n_instances=2))
    flat = scene.flat()
    assert scene.settings().mesh_light_count >= 1 and flat.instance_count == 4
    runs = assert_all_settings_equal(golden_luts, scene, rows=True, frames=False)
    info = runs[DEFAULT][2]
    assert info["material_generic"] == 1 and info["frame_table_bytes"] == 0, info
    assert (info["material_lds"] >= 144 * flat.triangle_count) == (case == "mode 1") and info["material_lds"] != 0, info
    assert info["dielectric_row_lds"] == info["dielectric_row_bytes"] != 0, info
    assert all(c["shadow_rays"] > 0 for c in runs[DEFAULT][1])


def test_scene_without_a_plastic_material_has_no_rows(golden_luts):
    """No material reads the rows: none are built, and MATERIAL's launch keeps its LDS to the byte."""
    scene = cornell(96, 80, 3)
    for i in range(scene.material_count):
        scene.set_material(i, _abi.MATERIAL_CONDUCTOR if i % 2 else _abi.MATERIAL_DIFFUSE, (0.6, 0.5, 0.4), 0.3, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
    runs = assert_all_settings_equal(golden_luts, scene, rows=False, frames=True, images=2)
    assert runs[DEFAULT][2]["dielectric_row_lds"] == 0 and runs[DEFAULT][2]["material_lds"] == runs[OFF][2]["material_lds"]


def test_scene_with_more_materials_than_the_cap_keeps_the_per_hit_lut(golden_luts):
    """65 materials (the Cornell arrays with its first material repeated behind them): no rows."""
    scene = cornell(96, 80, 3)
    flat = scene.flat()
    n = flat.material_count
    materials = (_abi.Material * 65)(*([flat.materials[i] for i in range(n)] + [flat.materials[0]] * (65 - n)))

    def upload(t):
        f = scene.flat()
        f.materials, f.material_count = materials, 65
        assert t._lib.dcrt_tracer_upload_scene(t._h, C.byref(f)) == 0
        t.set_frame_params(scene.frame_params(1))
        t.filter = scene.filter_params()

    runs = {}
    for tables in (DEFAULT, OFF):
        film, counters, info = render_fresh(golden_luts, scene, tables, upload=upload)
        assert info["shading_tables"] == BITS[tables] & 5 and info["dielectric_row_bytes"] == 0, info
        runs[tables] = (film, counters)
    assert same_bits(runs[DEFAULT][0], runs[OFF][0]) and runs[DEFAULT][1] == runs[OFF][1]
    plain, _, _ = render_fresh(golden_luts, scene, OFF)
    assert same_bits(runs[OFF][0], plain)        # (the unused materials change nothing)


def test_film_and_ray_counts_are_the_oracles(golden_luts, oracle_mod):
    from directcomputeraytracing_amd import FILTER_BOX, FilterParams
    scene = cornell(96, 80, 8)
    filt = FilterParams(FILTER_BOX, 1.0, 1.5, 1 / 3, 1 / 3, 3)
    flat = oracle_mod.flat_with_own_bvh(scene)
    ref, ext, shadow = np.zeros((80, 96, 4), np.float32), 0, 0
    for seed in (1, 2, 3):
        p, v, _, c = oracle_mod.render(flat, golden_luts, oracle_mod.frame_params(scene, seed), oracle_mod.WAVEFRONT)
        oracle_mod.sample_convolution(filt, p, v, ref)
        ext += c["extension_rays"]
        shadow += c["shadow_rays"]
    t = new_tracer(golden_luts, lambda t: t.on_scene_loaded(scene, 1), DEFAULT)
    try:
        assert t.info()["shading_tables"] == 7 and t.info()["dielectric_row_lds"] != 0 and t.info()["frame_table_bytes"] == 48 * 32
        t.set_frame_params(scene.frame_params(1))
        t.clear_film()
        t.reset_stats()
        t.render_images(1, 3, filt)
        film, c = t.read_film(), t.counters()
    finally:
        t.destroy()
    assert same_bits(film, ref)
    assert (c["extension_rays"], c["shadow_rays"], c["new_paths"]) == (ext, shadow, 3 * 96 * 80)


def test_rows_equal_the_lut_on_plastic_edge_inputs(gpu_tracer, golden_luts):
    """dcrt_device_bsdf_eval / _sample of plastic over test_gpu_bsdf's edge inputs -- wo.z from 0 and
    1e-4 to 1 on either side, alpha 0 ... 1 around kAlphaThreshold and the first LUT rows, ior 1 ... 3.5
    (beyond the LUT) -- with the probe material's rows and with the LUT itself: every output bit."""
    saved = gpu_tracer.luts()
    gpu_tracer.set_luts(golden_luts)
    try:
        ref = B.R.Luts(dict(np.load(B.GOLDEN / "bxdf_luts.npz")))
        configs = 0
        for ior in B.IORS:
            wi, wo = B.edge_directions(ior)
            for alpha, two, ms, isf in itertools.product(B.ALPHAS, (False, True), (False, True), (0, 1, 2)):
                kw = B.material_kw(B.PLASTIC, alpha, ior, two, ms, isf)
                swo, su = B.edge_numbers(ref, dict(kw, ior=float(ior)))
                dm = B.device_material(kw)
                out = {}
                for tables in (ROWS, OFF):
                    with env(DCRT_SHADING_TABLES=tables):
                        out[tables] = gpu_tracer.bsdf_eval(dm, wi, wo, B.VNDF) + gpu_tracer.bsdf_sample(dm, swo, su, B.VNDF)
                for k, (a, b) in enumerate(zip(out[ROWS], out[OFF])):
                    assert same_bits(a, b), (kw, k)
                configs += 1
        assert configs == 5 * 7 * 2 * 2 * 3
    finally:
        gpu_tracer.set_luts(saved)


def test_material_and_lut_edits_rebuild_the_rows(golden_luts):
    scene = cornell(96, 80, 6)
    t = new_tracer(golden_luts, lambda t: t.on_scene_loaded(scene, 1), DEFAULT)
    try:
        scene.acquire_dirty()
        film_of([t], scene, 1)              # (graphs exist before the edits)

        def against_fresh(what):
            got = film_of([t], scene, 2)
            for tables in (DEFAULT, OFF):
                want = render_fresh(golden_luts, scene, tables, images=2)
                assert same_bits(got[0], want[0]), (what, tables)
                assert got[1] == want[1], (what, tables)
                if tables == DEFAULT:
                    assert t.info() == want[2], what

        m = scene.material_setting(2)
        scene.set_material(2, _abi.MATERIAL_PLASTIC, tuple(m.albedo), 0.37, (1.9, 1.9, 1.9))
        scene.set_material(4, _abi.MATERIAL_PLASTIC, (0.3, 0.5, 0.7), 0.05, (1.25, 1.25, 1.25))
        t.apply_edits(scene, scene.acquire_dirty(), 1)
        against_fresh("roughness and ior changed")
        # other LUTs, then the golden ones again: the rows hold the texels of the LUTs in place
        other = type(golden_luts).from_buffer_copy(golden_luts)
        texels = np.frombuffer(other, np.uint16)
        texels[:] = texels[::-1].copy()
        t.set_luts(other)
        reversed_film = film_of([t], scene, 2)
        t.set_luts(golden_luts)
        against_fresh("LUTs replaced and put back")
        assert not same_bits(reversed_film[0], film_of([t], scene, 2)[0])
    finally:
        t.destroy()


def test_light_edit_to_a_mesh_light_brings_the_pdf_back(golden_luts):
    """The only point light becomes a mesh light over two of the scene's triangles (UpdateLights with
    a hand-made light; the instance light indices are geometry and stay, so the triangles emit
    nothing when hit -- in the edited tracer and in the fresh ones alike): MATERIAL's variant becomes
    the any-scene one and its light samples are weighted with the BSDF pdf again."""
    scene = cornell(96, 80, 6)
    light = _abi.Light()
    light.radiance[:] = (40.0, 36.0, 30.0)
    light.position_or_triangle_range[:] = np.array([0, 2, 0], np.uint32).view(np.float32).tolist()   # triangles [0, 2) of instance 0
    light.flags = 0x2                                                                               # DCRT_LIGHT_FLAGS_MESH_LIGHT
    lights = (_abi.Light * 1)(light)

    def upload_with_mesh_light(t):
        f = scene.flat()
        f.lights, f.light_count = lights, 1
        assert t._lib.dcrt_tracer_upload_scene(t._h, C.byref(f)) == 0
        t.set_frame_params(scene.frame_params(1))
        t.filter = scene.filter_params()

    t = new_tracer(golden_luts, lambda t: t.on_scene_loaded(scene, 1), DEFAULT)
    try:
        assert t.info()["material_generic"] == 0
        point = film_of([t], scene, 2)
        assert t._lib.dcrt_tracer_update_lights(t._h, lights, 1) == 0
        assert t.info()["material_generic"] == 1 and t.info()["shading_tables"] == 3   # (no table in the any-scene variant)
        got = film_of([t], scene, 2)
    finally:
        t.destroy()
    assert not same_bits(got[0], point[0]) and got[0][..., :3].max() > 0 and got[1][0]["shadow_rays"] > 0
    for tables in SETTINGS:
        want = render_fresh(golden_luts, scene, tables, images=2, upload=upload_with_mesh_light)
        assert same_bits(got[0], want[0]), tables
        assert got[1] == want[1], tables


def test_sign_guard_of_the_frame_table_on_hits_with_negative_zero_barycentrics(golden_luts):
    """The one place where the table's exactness rests on reasoning: with bitwise-equal vertex normals
    bary3 forms (+0) u + n0 + (+0) v, and a -0 component of n0 survives exactly when both products are
    -0. MATERIAL's hit reconstruction (dcrt_device_frame_probe: hit_to_intersection in the form that takes
    the table) over chosen hit records of the Cornell scene -- the floor's vertex normals made
    (-0, -1, -0), every instance moved by a negative x so that the -0 survives the transform -- with
    u, v in {+0, -0, interior values}: table on and off agree in every bit, and the (-0, -0) record's
    normal differs from the (+0, +0) record's, so a table entry taken without the guard would be wrong."""
    from directcomputeraytracing_amd.scene import flat_triangle_instances
    scene = cornell(32, 32, 2)
    flat = scene.flat()
    T, I = flat.triangle_count, flat.instance_count
    vertices = (_abi.Vertex * flat.vertex_count)(*[flat.vertices[i] for i in range(flat.vertex_count)])
    changed = set()
    for i in range(flat.vertex_count):
        if tuple(vertices[i].normal) == (0.0, 1.0, 0.0):
            vertices[i].normal[:] = (-0.0, -1.0, -0.0)
            changed.add(i)
    target = [t for t in range(T) if all(flat.triangles[3 * t + k] in changed for k in range(3))]
    assert len(target) >= 2
    transforms = (_abi.Float4x3 * (2 * I))(*[flat.instance_transforms[i] for i in range(2 * I)])
    for i in range(I):
        transforms[i].m[3] = -0.25
    single, owners = flat_triangle_instances(scene._lib, flat)
    assert single

    def upload(t):
        f = scene.flat()
        f.vertices, f.instance_transforms = vertices, transforms
        assert t._lib.dcrt_tracer_upload_scene(t._h, C.byref(f)) == 0
        t.set_frame_params(scene.frame_params(1))

    NZ = np.float32(-0.0)
    uv = [(0.0, 0.0), (NZ, 0.0), (0.0, NZ), (NZ, NZ), (0.25, 0.5), (NZ, 0.3), (0.3, NZ)]
    u = np.array([a for _ in range(T) for a, _ in uv], np.float32)
    v = np.array([b for _ in range(T) for _, b in uv], np.float32)
    tri = np.repeat(np.arange(T, dtype=np.uint32), len(uv))
    signed = ((u.view(np.uint32) | v.view(np.uint32)) >> 31) != 0
    assert signed.sum() == 5 * T and (~signed).sum() == 2 * T       # (the records do carry the sign bit)
    t = new_tracer(golden_luts, upload, DEFAULT)
    try:
        assert t.info()["frame_table_bytes"] == 48 * T
        on = t.frame_probe(u, v, tri, owners[tri], True)
        off = t.frame_probe(u, v, tri, owners[tri], False)
    finally:
        t.destroy()
    assert same_bits(on, off), np.argwhere(on.view(np.uint32) != off.view(np.uint32))[:5].tolist()
    assert np.isfinite(off).all() and (np.abs(np.linalg.norm(off, axis=-1) - 1) < 1e-5).all()
    off = off.reshape(T, len(uv), 3, 3).view(np.uint32)
    for k in target:
        # normal.x: +0 from u = v = +0 (what the table holds), -0 where both products are -0
        assert off[k, 0, 0, 0] == 0 and off[k, 3, 0, 0] == 0x80000000, (k, off[k, :, 0].tolist())
        assert (off[k, 1, 0] == off[k, 0, 0]).all() and (off[k, 2, 0] == off[k, 0, 0]).all()
