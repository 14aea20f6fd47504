"""tests/light_table_ref.py, the float64 reference of power-proportional light selection (include/dcrt.h, "light
selection"), held to itself on the scenes of test_shading_ref.py: the probabilities sum to 1 and keep their uniform
share, a lamp's triangles follow their areas, the searches pick what the CDFs say, and the direct-light estimator has
the same mean under the table as under uniform selection."""
import numpy as np
import pytest

import light_table_ref as LT
import shading_ref as R
from test_shading_ref import shading_scenes  # noqa: F401 (the session's scenes)


def table_of(case):
    return LT.Table(case.ref, LT.scene_radius(*LT.float64_bounds(case.flat)))


@pytest.mark.parametrize("name", ["lights", "instances"])
def test_probabilities_sum_to_one_and_keep_their_uniform_share(shading_scenes, name):
    """`lights`: a rectangle lamp, the six-triangle fan, the cube, a point and a directional light; `instances`: six
    lamps under six transforms, whose world areas differ. P(l) sums to 1, every P(t | l) sums to 1, P(l) >= e / n."""
    case = getattr(shading_scenes, name)
    t = table_of(case)
    n = t.n
    assert t.active and n == (5 if name == "lights" else 6)
    assert abs(t.light_prob64.sum() - 1) < 1e-14 and abs(float(t.light_prob.astype(np.float64).sum()) - 1) < n * 2.0 ** -24
    assert (t.light_prob64 >= LT.EPSILON / n).all() and (t.light_prob >= np.float32(LT.EPSILON / n)).all()
    assert t.light_cdf[-1] == 1 and (np.diff(t.light_cdf) > 0).all()
    lamps = np.flatnonzero(t.kind == R.MESH)
    assert len(lamps) == (2 if name == "lights" else 6) and t.entries == int(case.ref["lights"][lamps, 4].sum())
    for l in lamps:
        b, c = int(t.tri_base[l]), int(t.tri_count[l])
        assert abs(t.tri_prob64[b:b + c].sum() - 1) < 1e-14 and t.tri_cdf[b + c - 1] == 1 and (np.diff(t.tri_cdf[b:b + c]) > 0).all()
        assert t.A[l] > 0 and (t.areas[b:b + c] > 0).all()
    if name == "instances":         # (the same rectangle under six transforms -- the identity and the rigid one keep its 0.8 -- and weights that follow the areas)
        assert len(np.unique(np.round(t.A, 4))) == 5 and t.A.max() / t.A.min() > 2.5
        y = LT.luminance(case.ref["lights"][:, 0:3].view(np.float32)).astype(np.float64)
        np.testing.assert_allclose(t.weights, np.pi * y * t.A, rtol=1e-15)
    print(name, "P(l)", t.light_prob, "A", t.A)


def test_the_float32_areas_are_the_float64_areas(shading_scenes):
    """a_t restated in float32 in the sampler's order against shading_ref.triangle_geometry's float64 area: a few float32
    roundings apart."""
    for case in (shading_scenes.lights, shading_scenes.instances):
        t = table_of(case)
        L = case.ref["lights"]
        for l in np.flatnonzero(t.kind == R.MESH):
            b, c = int(t.tri_base[l]), int(t.tri_count[l])
            _, _, area, _, _ = R.triangle_geometry(case.ref, int(L[l, 3]) + np.arange(c), np.full(c, int(L[l, 5])), np.float64)
            np.testing.assert_allclose(t.areas[b:b + c], area, rtol=2e-6)


def test_the_fans_triangles_follow_their_areas(shading_scenes):
    case = shading_scenes.lights
    t = table_of(case)
    L = case.ref["lights"]
    fan = int(np.flatnonzero((t.kind == R.MESH) & (L[:, 4] == 6))[0])
    b = int(t.tri_base[fan])
    _, _, area, _, _ = R.triangle_geometry(case.ref, int(L[fan, 3]) + np.arange(6), np.full(6, int(L[fan, 5])), np.float64)
    assert area.max() / area.min() > 20                      # (0.014 .. 0.39 before the instance's scale)
    np.testing.assert_allclose(t.tri_prob64[b:b + 6], area / area.sum(), rtol=2e-6)
    np.testing.assert_allclose(t.tri_prob[b:b + 6], area / area.sum(), rtol=2e-6)


def test_the_searches_pick_by_the_cdfs(shading_scenes):
    """Every 24-bit number's neighbours around each CDF entry: the light is the first with cdf > sel, so sel = cdf[l]
    itself already selects l + 1; no number selects past the arrays."""
    t = table_of(shading_scenes.lights)
    edges = t.light_cdf[:-1]
    below = np.nextafter(edges, np.float32(0))
    li, _ = LT.select(t, np.concatenate([below, edges, [np.float32(0), np.float32(1) - np.float32(2.0 ** -24)]]), np.zeros(2 * len(edges) + 2, np.float32))
    assert list(li) == list(range(len(edges))) + list(range(1, len(edges) + 1)) + [0, t.n - 1]
    fan = int(np.flatnonzero(t.tri_count == 6)[0])
    sel = np.full(1000, np.nextafter(t.light_cdf[fan], np.float32(0)), np.float32)
    tri_sel = (np.arange(1000) / 1000).astype(np.float32)
    li, k = LT.select(t, sel, tri_sel)
    c = t.tri_cdf[int(t.tri_base[fan]):][:6]
    assert (li == fan).all() and (k == np.searchsorted(c, tri_sel, side="right")).all() and k.max() == 5


def test_degenerate_tables_are_inactive(shading_scenes):
    case = shading_scenes.lights
    L = case.ref["lights"].copy()
    kinds = R.light_kind(L)
    dark = L.copy()
    dark[:, 0:3] = 0
    assert not LT.Table(dict(case.ref, lights=dark), 5.0).active
    assert not LT.Table(dict(case.ref, lights=L[kinds == R.POINT]), 5.0).active          # nothing to choose
    assert LT.Table(dict(case.ref, lights=L[(kinds == R.MESH) & (L[:, 4] == 6)]), 5.0).active   # one lamp: its triangles
    hot = L.copy()
    hot[0, 0:3] = np.array([np.inf, 1, 1], np.float32).view(np.uint32)
    assert not LT.Table(dict(case.ref, lights=hot), 5.0).active
    assert not LT.Table(dict(case.ref, lights=L[:0]), 5.0).active


POINTS = [((0.3, 0.2, -0.4), (0.0, 1.0, 0.0)), ((-1.5, 0.0, 1.0), (0.0, 1.0, 0.0)), ((1.0, 1.0, 0.5), (0.6, 0.8, 0.0)),
          ((-0.5, 4.5, 0.5), (0.0, -1.0, 0.0)), ((2.0, -0.3, -2.0), (0.0, 0.6, 0.8))]


@pytest.mark.parametrize("name", ["lights", "instances"])
def test_the_direct_estimator_keeps_its_mean(shading_scenes, name):
    """At five points, the first moment of the one-sample direct-light estimator -- summed exactly over lights and
    triangles, with a quadrature over every triangle and the sphere -- is the same under the table as under uniform
    selection with the evaluator's density, and both are the integral itself (computed without any pdf): selection
    probabilities and density cancel, whichever way the lights are picked. The second moments differ: the table's is
    printed beside uniform selection's."""
    case = getattr(shading_scenes, name)
    t = table_of(case)
    q, sph = LT.triangle_quadrature(12), LT.sphere_quadrature(24)
    for p, nrm in POINTS:
        mt, st, it = LT.direct_moments(case.ref, t, p, nrm, q, sph)
        mu, su, iu = LT.direct_moments(case.ref, None, p, nrm, q, sph)
        assert it == iu and it > 0
        assert abs(mt / it - 1) < 1e-6 and abs(mu / it - 1) < 1e-6, (p, mt, mu, it)     # (tri_prob and light_prob are float32)
        print(f"{name} {p}: mean {mt:.6f}, variance table {st - mt * mt:.4f} / uniform {su - mu * mu:.4f}")


@pytest.mark.parametrize("name", ["lights", "instances"])
def test_the_distribution_tests_draws_fill_every_bin(shading_scenes, name):
    """tests/test_gpu_light_table.py draws LT.CHI_DRAWS light samples and runs a chi-square per light and lamp triangle:
    with this N the smallest expected count is at least 20 -- by the reference alone, for R of the float64 box and for R
    of the uploaded BVH root's box, which is the one the library takes."""
    case = getattr(shading_scenes, name)
    root = case.flat.bvh_nodes[0]
    for radius in (LT.scene_radius(*LT.float64_bounds(case.flat)), LT.scene_radius(root.bbox_min[:], root.bbox_max[:])):
        e = LT.expected_counts(LT.Table(case.ref, radius), LT.CHI_DRAWS)
        assert len(e) == (11 if name == "lights" else 12) and abs(sum(e.values()) - LT.CHI_DRAWS) < 1e-6
        print(name, "R", radius, "smallest expected count", min(e.values()))
        assert min(e.values()) >= 20, min(e.values())
