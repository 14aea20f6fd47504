"""The GPU ray casts against the float64 brute-force intersection reference (tests/ray_truth.py),
directly and not through the oracle: `WavefrontPathTracer.trace_rays` and `.occluded`, i.e. the four
`batch_trace_kernel` variants (closest / any hit x watertight / Moller-Trumbore), with the session
tracer (LDS node cache, PackBVH's order) and with a tracer made under DCRT_NO_LDS_CACHE=1 +
DCRT_PAIR_TRAVERSAL=1 (global memory, the child-pair order). The assertions are those of
tests/test_ray_truth.py, where the tolerances and the ambiguous-ray caps are explained.

The render path's cast kernels (the LDS-only, identity, ring and merged EXT + SHADOW variants) have no
ray-level entry point. They stay covered by their bit-equality with the oracle (tests/test_gpu_parity.py,
tests/test_random_scenes.py), and tests/test_ray_truth.py holds the oracle to this reference."""
import numpy as np
import pytest

import ray_truth as T
from test_ray_truth import check_watertight, inside_rays

pytestmark = pytest.mark.gpu

_cases = {}


@pytest.fixture(scope="module")
def case(native_lib, tmp_path_factory):
    from test_scene_pin import _flat_arrays

    def get(name):
        if name not in _cases:
            s = T.load_scene(name, tmp_path_factory.mktemp(name))
            _cases[name] = (T.Case(name, _flat_arrays(s.flat())), s)
        return _cases[name]
    return get


@pytest.fixture
def pair_tracer(native_lib, golden_luts, monkeypatch):
    from directcomputeraytracing_amd import WavefrontPathTracer
    monkeypatch.setenv("DCRT_NO_LDS_CACHE", "1")
    monkeypatch.setenv("DCRT_PAIR_TRAVERSAL", "1")
    t = WavefrontPathTracer(path_pool_size=1 << 12, debug_rng=True)
    t.set_luts(golden_luts)
    yield t
    t.destroy()


def _load(tracer, scene, pair):
    tracer.on_scene_loaded(scene)
    assert tracer.info()["pair_traversal"] == (1 if pair else 0)
    return tracer


def _check(tracer, c, families=None):
    msgs = []
    for features in (0x0D, 0x05):
        msgs += [f"{features:#x} {m}" for m in c.check(lambda r: tracer.trace_rays(r, features), lambda r: tracer.occluded(r, features),
                                                       families)]
    assert not msgs, "\n".join(msgs)


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
