"""The GPU ray casts against the float64 brute-force intersection reference (tests/ray_truth.py),
directly and not through the oracle. The assertions are those of tests/test_ray_truth.py, where the
tolerances and the ambiguous-ray caps are explained.

Two kinds of entry are held to it:

* `WavefrontPathTracer.trace_rays` and `.occluded`, i.e. the four `batch_trace_kernel` variants (closest /
  any hit x watertight / Moller-Trumbore), with the session tracer (LDS node cache, PackBVH's order) and
  with a tracer made under DCRT_NO_LDS_CACHE=1 + DCRT_PAIR_TRAVERSAL=1 (global memory, the pair order).

* `WavefrontPathTracer.cast_rays`: the caller's rays through the cast_kernel variant, scene copy, LDS bytes and
  workgroup size that a render of the uploaded scene launches (`cast_rays_kernel`, instantiated from the
  cast's own variant table), closest and any-hit rays mixed in one batch as in the merged cast. Every
  result is compared bit for bit with `oracle_cast_rays` and then, on its own numbers, with the reference.
  The variant that ran is asserted from the entry's `variant` output, never inferred:

      knobs (TRACERS)                                   small           obj                       soup, closed, large
      default                                           all_cached      all_cached ident flat     (global: partly cached)
      DCRT_FLAT_CAST=0                                  -               all_cached ident          -
      DCRT_NO_LDS_CACHE=1                               (global)        ident                     (global)
      ... + DCRT_PAIR_TRAVERSAL=1                       pair            pair                      pair
      ... + DCRT_STACK_RING=8                           ring            ring ident                ring
      ... + DCRT_STACK_RING=8 + DCRT_PAIR_TRAVERSAL=1   ring pair       ring pair                 ring pair

  (The cast's LDS cache holds about 17 KiB of a scene with the soup's stack depth; the soup needs 19 KiB, the
  closed meshes 42 KiB. The small soup and the small closed scene are the all-cached ones with instance
  transforms, where tri_watertight_rot on rotated LDS triangles replaces tri_watertight.)

  With FEATURE_ALLOW_ANYHIT (0x10: every ray carries an opacity sample into the any-hit test) the three
  opacity rows: all_cached on the veil scene and the small soup, global and pair on those two and on the soup,
  each with the opacity edits of tests/ray_truth.py, and the exact families float32 decides without tolerance
  (`exact_cards`) on the veil scene under all three.

Not reached by a ray-level entry (they keep resting on bit equality of renders with the oracle,
tests/test_gpu_parity.py and tests/test_random_scenes.py, which tests/test_ray_truth.py holds to this reference,
now under any-hit as well): the counting (INSTR) variants, the CELLS shadow section (its own entry:
tests/test_gpu_shadow_cells.py), the split extension_kernel / shadow_kernel, and the megakernel's and the view
kernel's trace_full<..., OPACITY>."""
import ctypes as C

import numpy as np
import pytest

import ray_truth as T
from test_ray_truth import check_exact_families, check_watertight, edited_flat, inside_rays

pytestmark = pytest.mark.gpu

_cases = {}
_opacity_cases = {}


@pytest.fixture(scope="module")
def case(native_lib, tmp_path_factory):
    from test_scene_pin import _flat_arrays

    def get(name):
        if name not in _cases:
            s = T.load_scene(name, tmp_path_factory.mktemp(name))
            _cases[name] = (T.Case(name, _flat_arrays(s.flat())), s)
        return _cases[name]
    return get


@pytest.fixture(scope="module")
def opacity_case(case):
    """name -> (the any-hit case over the product's flat scene with the opacity edits, that flat scene, the scene)."""
    from test_scene_pin import _flat_arrays

    def get(name):
        if name not in _opacity_cases:
            _, s = case(name)
            edited = edited_flat(name, s.flat(), s)
            _opacity_cases[name] = (T.Case(name, _flat_arrays(edited), T.Opacity(edited)), edited, s)
        return _opacity_cases[name]
    return get


# the upload knobs that reach the cast's variants
TRACERS = {
    "noflat": {"DCRT_FLAT_CAST": "0"},
    "nolds": {"DCRT_NO_LDS_CACHE": "1"},
    "pair": {"DCRT_NO_LDS_CACHE": "1", "DCRT_PAIR_TRAVERSAL": "1"},
    "ring": {"DCRT_NO_LDS_CACHE": "1", "DCRT_STACK_RING": "8"},
    "ring_pair": {"DCRT_NO_LDS_CACHE": "1", "DCRT_STACK_RING": "8", "DCRT_PAIR_TRAVERSAL": "1"},
}


@pytest.fixture
def knob_tracer(native_lib, golden_luts, monkeypatch, gpu_tracer):
    """knobs name -> a tracer made under TRACERS[name] ("default": the session tracer)."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    made = []

    def get(name):
        if name == "default":
            return gpu_tracer
        for k, v in TRACERS[name].items():
            monkeypatch.setenv(k, v)
        t = WavefrontPathTracer(path_pool_size=1 << 12, debug_rng=True)
        t.set_luts(golden_luts)
        made.append(t)
        return t
    yield get
    for t in made:
        t.destroy()


@pytest.fixture
def pair_tracer(knob_tracer):
    return knob_tracer("pair")


def _load(tracer, scene, pair):
    tracer.on_scene_loaded(scene)
    assert tracer.info()["pair_traversal"] == (1 if pair else 0)
    return tracer


def _upload(tracer, flat, scene):
    """An edited flat scene of `scene` into the tracer (on_scene_loaded takes a Scene)."""
    from directcomputeraytracing_amd.tracer import check
    check(tracer._lib.dcrt_tracer_upload_scene(tracer._h, C.byref(flat)), "OnSceneLoaded")
    tracer.set_frame_params(scene.frame_params(0))
    return tracer


def _check(tracer, c, families=None):
    msgs = []
    for features in (0x0D, 0x05):
        msgs += [f"{features:#x} {m}" for m in c.check(lambda r: tracer.trace_rays(r, features), lambda r: tracer.occluded(r, features),
                                                       families)]
    assert not msgs, "\n".join(msgs)


def _check_cast(tracer, c, flat, oracle_mod, feature_list):
    """Every family of the case through `cast_rays` under each of the features: bit-identical to
    oracle_cast_rays on the same flat scene, and the reference's checks on the device's own numbers.
    Returns the variant that ran (the same for every call)."""
    msgs, variants = [], []
    for features in feature_list:
        got = {}

        def device(rays, kinds, samples):
            hits, occ, variant = tracer.cast_rays(rays, kinds, samples, features)
            variants.append(frozenset(variant))
            return hits, occ

        def both(rays, samples=None):
            if id(rays) not in got:
                got[id(rays)] = T.cast_both(device, rays, samples)
                want = T.cast_both(lambda r, k, s: oracle_mod.cast_rays(flat, r, k, s, features)[:2], rays, samples)
                differ = np.flatnonzero((got[id(rays)][0] != want[0]) | (got[id(rays)][1] != want[1]))
                if len(differ):
                    msgs.append(f"{features:#x}: {len(differ)} of {len(rays)} rays differ from oracle_cast_rays, first {differ[:5]}: "
                                f"{got[id(rays)][0][differ[:3]]} {got[id(rays)][1][differ[:3]]} / {want[0][differ[:3]]} {want[1][differ[:3]]}")
            return got[id(rays)]
        msgs += [f"{features:#x} {m}" for m in c.check(lambda *a: both(*a)[0], lambda *a: both(*a)[1])]
    assert not msgs, "\n".join(msgs)
    assert len(set(variants)) == 1, set(variants)
    return set(variants[0])


@pytest.mark.parametrize("name", ["soup", "closed", "obj"])
def test_gpu_casts_match_reference(gpu_tracer, case, name):
    c, s = case(name)
    _check(_load(gpu_tracer, s, False), c)


@pytest.mark.parametrize("name", ["soup", "closed", "obj"])
def test_gpu_pair_traversal_casts_match_reference(pair_tracer, case, name):
    c, s = case(name)
    _check(_load(pair_tracer, s, True), c)


def test_gpu_large_soup_matches_reference(gpu_tracer, case):
    """3 x 5.2 k triangles: the BVH is deeper than the LDS node cache holds."""
    c, s = case("large")
    t = _load(gpu_tracer, s, False)
    assert t.info()["scene_in_lds"] == 0
    _check(t, c)


def test_gpu_large_soup_pair_traversal_matches_reference(pair_tracer, case):
    c, s = case("large")
    t = _load(pair_tracer, s, True)
    assert t.info()["scene_in_lds"] == 0
    _check(t, c)


@pytest.mark.parametrize("n", T.BATCH_SIZES)
def test_gpu_batch_sizes(gpu_tracer, case, n):
    """Batches shorter than a wave or a workgroup, and no multiple of either: the persistent
    cast's refill. The rays are a mix of every family of the small soup."""
    c, s = case("soup")
    t = _load(gpu_tracer, s, False)
    rays, _ = c.mixed(n)
    assert len(rays) == n
    an = c.truth.analyse(rays)
    for features in (0x0D, 0x05):
        h = t.trace_rays(rays, features)
        assert len(h) == n
        bad = T.compare_hits(c.truth, an, rays, h)
        assert not bad, (features, {k: T.describe(an, v) for k, v in bad.items()})
        idx, _ = T.compare_occluded(an, rays, t.occluded(rays, features))
        assert len(idx) == 0, (features, T.describe(an, idx))


@pytest.mark.parametrize("pair", [False, True])
def test_gpu_closed_meshes_are_watertight(request, case, pair):
    """The watertight casts from inside the closed meshes; the box test's leaks on exactly aimed
    rays are the reference's, pinned in test_ray_truth.BOX_LEAKS."""
    c, s = case("closed")
    t = _load(request.getfixturevalue("pair_tracer" if pair else "gpu_tracer"), s, pair)   # (pair_tracer sets the environment)
    rays, aimed = inside_rays(c.truth, 11)
    check_watertight(rays, aimed, c.truth.analyse(rays), lambda r, f: t.trace_rays(r, f))


def test_gpu_backface_convention(gpu_tracer, native_lib, tmp_path):
    """test_ray_truth.test_backface_convention on the GPU casts."""
    from test_ray_truth import _ray
    from test_scene_pin import _flat_arrays
    from directcomputeraytracing_amd import Scene
    (tmp_path / "one.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\nf 1/1/1 2/1/1 3/1/1\n")
    s = Scene((8, 8))
    s.load_from_file(tmp_path / "one.obj")
    gpu_tracer.on_scene_loaded(s)
    tr = T.Truth(_flat_arrays(s.flat()))
    c = tr.p_world[0].mean(0)
    n = np.cross(tr.p_world[0, 1] - tr.p_world[0, 0], tr.p_world[0, 2] - tr.p_world[0, 0])
    rays = np.concatenate([_ray(c + 2 * n, -n), _ray(c - 2 * n, n)])          # d . n < 0, then d . n > 0
    for features in (0x0D, 0x05):
        h = gpu_tracer.trace_rays(rays, features)
        assert np.isfinite(h["t"]).all()
        assert list(h["triangle_id"] >> 31) == ([1, 0] if T.BACKFACE_IS_NEGATIVE_FACING else [0, 1]), features


# ---- the render path's cast variants: cast_rays ----------------------------------------------------------------
def _expected_variant(knobs, name):
    """The cast_kernel row of the module docstring's table."""
    ident = name == "obj"               # (the OBJ scene's instances are all the identity)
    if knobs == "default":
        return {"all_cached", "ident", "flat"} if ident else {"all_cached"} if name == "small" else set()
    if knobs == "noflat":
        return {"all_cached", "ident"} if ident else {"all_cached"}
    want = {"nolds": set(), "pair": {"pair"}, "ring": {"ring"}, "ring_pair": {"ring", "pair"}}[knobs]
    return want | ({"ident"} if ident and "pair" not in want else set())


@pytest.mark.parametrize("name", ["soup", "closed", "obj", "large", "small"])
@pytest.mark.parametrize("knobs", ["default", "nolds", "pair", "ring", "ring_pair"])
def test_gpu_cast_variants_match_oracle_and_reference(knob_tracer, case, oracle_mod, knobs, name):
    """Opaque features (0x0D, 0x05): every family through the cast variant the knobs select."""
    c, s = case(name)
    t = knob_tracer(knobs)
    t.on_scene_loaded(s)
    assert t.info()["scene_in_lds"] == (1 if knobs == "default" and name in ("obj", "small") else 0)
    variant = _check_cast(t, c, s.flat(), oracle_mod, (0x0D, 0x05))
    assert variant == _expected_variant(knobs, name), (variant, knobs, name)
    if "ring" in variant and name == "large":
        assert t.ring_spills() > 0, "a stack 22 deep in a window of 8 rows: the ring kernel must have spilled"


def test_gpu_cast_all_cached_ident_variant(knob_tracer, case, oracle_mod):
    """The cache-only IDENT kernel on PackBVH's order (DCRT_FLAT_CAST=0): the row the entry-free order replaces."""
    c, s = case("obj")
    t = knob_tracer("noflat")
    t.on_scene_loaded(s)
    assert _check_cast(t, c, s.flat(), oracle_mod, (0x0D, 0x05)) == {"all_cached", "ident"}


@pytest.mark.parametrize("name", sorted(T.OPACITY_INSTANCES))
@pytest.mark.parametrize("knobs", ["default", "nolds", "pair"])
def test_gpu_any_hit_cast_variants_match_oracle_and_reference(knob_tracer, opacity_case, oracle_mod, knobs, name):
    """FEATURE_ALLOW_ANYHIT (0x1D, 0x15): the three opacity rows on the veil scene and the soups with opacity edits
    (all-cached: the veil scene and the small soup; the soup's default cast is the global row)."""
    c, flat, s = opacity_case(name)
    t = _upload(knob_tracer(knobs), flat, s)
    variant = _check_cast(t, c, flat, oracle_mod, (0x1D, 0x15))
    want = {"default": set() if name == "soup" else {"all_cached"}, "nolds": set(), "pair": {"pair"}}[knobs]
    assert variant == {"opacity"} | want, (variant, knobs, name)


@pytest.mark.parametrize("knobs", ["default", "nolds", "pair"])
def test_gpu_exact_opacity_families(knob_tracer, opacity_case, knobs):
    """Where float32 decides exactly (test_ray_truth.test_oracle_exact_opacity_families), no tolerance."""
    c, flat, s = opacity_case("veil")
    t = _upload(knob_tracer(knobs), flat, s)
    for features in (0x1D, 0x15):
        seen = []

        def cast(r, k, sm, f=features):
            h, o, v = t.cast_rays(r, k, sm, f)
            seen.append(v)
            return h, o
        check_exact_families(c, flat, cast)
        assert all(v == {"opacity"} | {"default": {"all_cached"}, "nolds": set(), "pair": {"pair"}}[knobs] for v in seen), seen


def test_gpu_any_hit_bit_with_opaque_materials_changes_nothing(gpu_tracer, case):
    """With every material opaque the any-hit kernels give the opaque kernels' results, whatever the samples."""
    c, s = case("small")
    gpu_tracer.on_scene_loaded(s)
    rays, _ = c.mixed(3000)
    samples = np.random.default_rng(3).random(len(rays), np.float32)
    for features in (0x0D, 0x05):
        seen = []

        def cast(r, k, sm, f=features | 0x10):
            h, o, v = gpu_tracer.cast_rays(r, k, sm, f)
            seen.append(v)
            return h, o
        hits, occ = T.cast_both(cast, rays, samples)
        assert all(v == {"opacity", "all_cached"} for v in seen), seen
        assert hits.tobytes() == gpu_tracer.trace_rays(rays, features).tobytes()
        assert np.array_equal(occ, gpu_tracer.occluded(rays, features))


@pytest.mark.parametrize("n", T.BATCH_SIZES)
def test_gpu_cast_batch_sizes(gpu_tracer, case, opacity_case, oracle_mod, n):
    """`test_gpu_batch_sizes` through cast_rays: kinds alternating per ray and in runs of 64 (`mixed_kinds`), opaque on
    the small soup and with opacity samples on the veil scene (the all-cached kernels both)."""
    for name, feature_list in (("small", (0x0D, 0x05)), ("veil", (0x1D, 0x15))):
        if name == "small":
            c, s = case(name)
            flat = s.flat()
            gpu_tracer.on_scene_loaded(s)
        else:
            c, flat, s = opacity_case(name)
            _upload(gpu_tracer, flat, s)
        rays = np.concatenate(list(c.families.values()))
        order = np.resize(np.random.default_rng(7).permutation(len(rays)), n)      # (10 007 is more than the case has: some rays twice)
        rays = rays[order]
        samples = None if c.samples is None else np.concatenate(list(c.samples.values()))[order]
        an = c.truth.analyse(rays, samples)
        for features in feature_list:
            hits, occ = T.cast_both(lambda r, k, sm: gpu_tracer.cast_rays(r, k, sm, features)[:2], rays, samples)
            want = T.cast_both(lambda r, k, sm: oracle_mod.cast_rays(flat, r, k, sm, features)[:2], rays, samples)
            assert len(hits) == n and hits.tobytes() == want[0].tobytes() and np.array_equal(occ, want[1]), (name, features)
            bad = T.compare_hits(c.truth, an, rays, hits)
            assert not bad, (name, features, {k: T.describe(an, v) for k, v in bad.items()})
            idx, _ = T.compare_occluded(an, rays, occ)
            assert len(idx) == 0, (name, features, T.describe(an, idx))


@pytest.mark.parametrize("name", ["closed", "closed_small"])
def test_gpu_cast_closed_meshes_are_watertight(gpu_tracer, case, tmp_path, name):
    """`check_watertight` and the pinned box leaks through cast_rays: the closed meshes (the global cast over the
    partly cached scene) and the small closed scene, which the LDS cache holds whole -- the all-cached variant, where
    tri_watertight_rot on the rotated LDS triangles replaces tri_watertight."""
    from test_ray_truth import BOX_LEAKS, SMALL_BOX_LEAKS
    from test_scene_pin import _flat_arrays
    if name == "closed":
        c, s = case(name)
        truth = c.truth
    else:
        s = T.load_scene(name, tmp_path)
        truth = T.Truth(_flat_arrays(s.flat()))
    gpu_tracer.on_scene_loaded(s)
    rays, aimed = inside_rays(truth, 11)
    seen = []

    def trace(r, f):
        h, _, v = gpu_tracer.cast_rays(r, np.zeros(len(r), np.uint32), None, f)
        seen.append(v)
        return h
    check_watertight(rays, aimed, truth.analyse(rays), trace, box_leaks=BOX_LEAKS if name == "closed" else SMALL_BOX_LEAKS)
    assert all(v == ({"all_cached"} if name == "closed_small" else set()) for v in seen), seen
