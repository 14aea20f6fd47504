"""tests/env_importance_ref.py held to itself on the cubes of the device tests: the density integrates to 1
over the sphere, 200 000 sampled directions follow it (chi-square per texel), and the sampler's estimate of a
plane's direct irradiance agrees with uniform sampling's. No GPU."""
import numpy as np
import pytest

import env_importance_ref as E
import shading_ref as R
from ref_tolerance import chi_square_quantile

CHI_DRAWS = 200_000


@pytest.fixture(scope="module")
def cubes():
    return E.cubes()


def numbers(seed, count):
    """float32 numbers in [0, 1) with 24 random bits each, (count, 2)."""
    return (np.random.default_rng(seed).integers(0, 1 << 24, (count, 2)) / float(1 << 24)).astype(np.float32)


@pytest.mark.parametrize("name", E.ACTIVE_CUBES)
def test_table_is_a_distribution(cubes, name):
    t = E.Table(cubes[name])
    n = t.n
    assert t.active and t.prob.shape == (6 * n, n) and t.marginal.shape == (6 * n,)
    assert abs(t.prob64.sum() - 1) < 1e-12 and (t.prob >= 0).all()
    assert (np.diff(t.marginal) >= 0).all() and t.marginal[-1] == 1
    live = t.prob64.sum(1) > 0
    assert (np.diff(t.row_cdf, axis=1) >= 0).all() and (t.row_cdf[live, -1] == 1).all() and (t.row_cdf[~live] == 0).all()


@pytest.mark.parametrize("name", E.INACTIVE_CUBES)
def test_degenerate_cubes_have_no_table(cubes, name):
    assert not E.Table(cubes[name]).active


@pytest.mark.parametrize("name", ["n1", "n2", "n5_hot", "n8_sun"])
def test_density_integrates_to_one(cubes, name):
    """Per texel a k x k midpoint rule in face coordinates, the density taken at the DIRECTION of each node (so through
    the face table, the texel lookup and the Jacobian): the integrand pdf / (1 + sc^2 + tc^2)^(3/2) is constant for the table's
    share and smooth for the uniform share, whose midpoint error falls as 1 / (k n)^2."""
    t = E.Table(cubes[name])
    n = t.n
    k = max(24, 96 // n)       # (n k >= 96 nodes across a face: the n = 1 cube at 24 is off by 2.7e-5, a sixteenth of it at 96)
    g = (2.0 * (np.arange(n * k) + 0.5) / (n * k)) - 1.0
    SC, TC = np.meshgrid(g, g, indexing="xy")
    sc, tc = SC.ravel(), TC.ravel()
    one = np.ones_like(sc)
    total = 0.0
    for face in range(6):
        d = np.stack([[one, -one, sc, sc, sc, -sc][face], [-tc, -tc, one, -one, -tc, -tc][face], [-sc, sc, tc, -tc, one, -one][face]], -1)
        d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
        q = 1 + sc * sc + tc * tc
        total += (E.env_pdf(t, d) / (q * np.sqrt(q))).sum() * (2.0 / (n * k)) ** 2
    print(f"{name}: integral {total:.9f}")
    assert abs(total - 1) < 2e-5, total


@pytest.mark.parametrize("name", ["n2", "n5_hot", "n8_sun"])
def test_sampled_directions_follow_the_density(cubes, name):
    t = E.Table(cubes[name])
    u = numbers(11, CHI_DRAWS)
    d, r, c = E.sample_direction(t, u[:, 0], u[:, 1])
    assert (np.abs(np.linalg.norm(d, axis=1) - 1) < 1e-12).all()
    expected = E.expected_counts(t, CHI_DRAWS)
    chi2, dof = E.chi_square(E.texel_counts(d, t.n), expected)
    print(f"{name}: chi2 {chi2:.1f}, dof {dof}, bound {chi_square_quantile(dof):.1f}, smallest expected count {expected[expected > 0].min():.1f}")
    assert chi2 < chi_square_quantile(dof), (chi2, dof)
    # a direction drawn from the table lies in the texel chosen (away from its edges)
    face, iy, ix = E.texel_of(d.astype(np.float32), t.n)
    grid, gap = E.texel_margin(d.astype(np.float32), t.n)
    inner = (r >= 0) & (grid > 1e-4) & (gap > 1e-4)
    assert inner.mean() > 0.9 and ((face * t.n + iy == r) & (ix == c))[inner].all()


@pytest.mark.parametrize("name", ["n5_hot", "n8_sun"])
def test_irradiance_estimates_agree_with_uniform_sampling(cubes, name):
    """The direct irradiance of a horizontal plane, L cos / pdf averaged: the table's sampler and the uniform sphere agree
    within 3 combined standard errors, and the table's variance is the smaller."""
    cube = cubes[name]
    t = E.Table(cube)
    N = 400_000
    u = numbers(12, N)
    d, _, _ = E.sample_direction(t, u[:, 0], u[:, 1])
    d32 = d.astype(np.float32)
    lum = lambda x: x @ np.array([0.299, 0.587, 0.114])
    f_is = lum(R.env_lookup(cube, d32)) * np.maximum(d32[:, 1].astype(np.float64), 0) / E.env_pdf(t, d32)
    v = numbers(13, N)
    w = E.uniform_sphere(v[:, 0], v[:, 1]).astype(np.float32)
    f_un = lum(R.env_lookup(cube, w)) * np.maximum(w[:, 1].astype(np.float64), 0) * (4 * np.pi)
    se = np.sqrt(f_is.var() / N + f_un.var() / N)
    print(f"{name}: importance {f_is.mean():.4f} +- {np.sqrt(f_is.var() / N):.4f}, uniform {f_un.mean():.4f} +- {np.sqrt(f_un.var() / N):.4f}, "
          f"variance ratio {f_is.var() / f_un.var():.4f}")
    assert abs(f_is.mean() - f_un.mean()) < 3 * se
    assert f_is.var() < f_un.var()
    exact = lum(E.hemisphere_irradiance(cube, 256))
    assert abs(f_is.mean() - exact) < 4 * np.sqrt(f_is.var() / N) + 1e-3 * exact, (f_is.mean(), exact)


def test_solid_angles_tile_the_sphere():
    for n in (1, 2, 5, 8):
        assert abs(6 * E.texel_solid_angles(n).sum() - 4 * np.pi) < 1e-12
