"""The CPU oracle's BxDF stack and the golden LUTs against tests/bsdf_ref.py, a float64 reference
written from the literature: BSDF values and pdfs at seeded direction pairs, the samplers' draws
against the pdf (chi-square), and every table against a quadrature of the directional albedo. The
same checks run through the device entries in tests/test_gpu_bsdf.py."""
from statistics import NormalDist

import numpy as np
import pytest

import bsdf_ref as R
from conftest import GOLDEN
from ref_tolerance import CHI_Z, TOLERANCE_K, TOLERANCE_ULPS, chi_square_quantile, tolerance_ratio  # noqa: F401 (re-exported)

DIFFUSE, PLASTIC, CONDUCTOR, DIELECTRIC, THIN = 0, 1, 2, 3, 4
VNDF = 1   # DCRT_FEATURE_GGX_SAMPLE_VNDF

MATERIALS = [
    ("plastic_rough", dict(type=PLASTIC, albedo=(0.7, 0.6, 0.5), alpha=0.4, ior=1.5)),
    ("plastic_rough_ms", dict(type=PLASTIC, albedo=(0.7, 0.6, 0.5), alpha=0.6, ior=1.5, multiscattering=True)),
    ("conductor_rough", dict(type=CONDUCTOR, albedo=(3.9, 2.4, 1.6), alpha=0.35, ior=0.2)),
    ("conductor_rough_ms", dict(type=CONDUCTOR, albedo=(3.9, 2.4, 1.6), alpha=0.7, ior=0.2, multiscattering=True)),
    ("dielectric_rough", dict(type=DIELECTRIC, alpha=0.3, ior=1.5)),
    ("dielectric_rough_ms", dict(type=DIELECTRIC, alpha=0.5, ior=1.5, multiscattering=True)),
]
EVAL_MATERIALS = MATERIALS + [
    ("diffuse", dict(type=DIFFUSE, albedo=(0.8, 0.5, 0.2))),
    ("plastic_isf0", dict(type=PLASTIC, albedo=(0.9, 0.5, 0.1), alpha=0.25, ior=1.8, internal_scattering=0)),
    ("plastic_isf1", dict(type=PLASTIC, albedo=(0.9, 0.5, 0.1), alpha=0.25, ior=1.8, internal_scattering=1)),
    ("plastic_isf2", dict(type=PLASTIC, albedo=(0.9, 0.5, 0.1), alpha=0.25, ior=1.8, internal_scattering=2)),
    ("plastic_ms_isf2", dict(type=PLASTIC, albedo=(0.9, 0.5, 0.1), alpha=0.8, ior=1.3, multiscattering=True, internal_scattering=2)),
    ("conductor_rgb", dict(type=CONDUCTOR, albedo=(3.9, 2.4, 1.1), alpha=0.2, ior=(0.2, 0.9, 1.4))),
    ("conductor_rgb_ms", dict(type=CONDUCTOR, albedo=(5.0, 4.0, 3.0), alpha=0.55, ior=(1.0, 0.9, 0.8), multiscattering=True)),
    ("dielectric_1.33", dict(type=DIELECTRIC, alpha=0.3, ior=1.33)),
    ("dielectric_1.33_ms", dict(type=DIELECTRIC, alpha=0.45, ior=1.33, multiscattering=True)),
    ("dielectric_1.5", dict(type=DIELECTRIC, alpha=0.15, ior=1.5)),
    ("dielectric_2.4", dict(type=DIELECTRIC, alpha=0.6, ior=2.4)),
    ("dielectric_2.4_ms", dict(type=DIELECTRIC, alpha=0.35, ior=2.4, multiscattering=True)),
]
EVAL_CASES = [(n, kw, two, feat) for n, kw in EVAL_MATERIALS for two in (False, True) for feat in (VNDF, 0)]
# smooth plastic: the evaluator describes the Lambert base alone, weighted 1 - coat (the coat is a delta lobe)
SMOOTH_PLASTICS = [
    ("plastic_smooth", dict(type=PLASTIC, albedo=(0.7, 0.6, 0.5), alpha=0.0, ior=1.5), False),
    ("plastic_smooth_two_isf2", dict(type=PLASTIC, albedo=(0.9, 0.5, 0.1), alpha=0.0, ior=1.8, internal_scattering=2), True),
]
EVAL_CASES += [(n, kw, two, feat) for n, kw, two in SMOOTH_PLASTICS for feat in (VNDF, 0)]
EVAL_PAIRS = 4000


@pytest.fixture(scope="module")
def ref_luts():
    return R.Luts(dict(np.load(GOLDEN / "bxdf_luts.npz")))


def eval_inputs(name, kw, n=EVAL_PAIRS):
    """Seeded float32 unit direction pairs for one material: wo above the surface for one half and
    below it for the other; wi on wo's side for 4 in 5 pairs of a reflecting material and for every
    other pair of a dielectric (the rest are transmission pairs); |cos| >= 0.02 for both, and the pair's
    half vector (the reflection one on one side, the refraction one across) at least 0.02 in
    cosine away from perpendicular to either, transmission pairs off the critical angle. Returns wi,
    wo and the fraction of the n pairs kept."""
    rng = np.random.default_rng(abs(hash_name(name)))

    def hemi(k):
        z = rng.uniform(0.02, 1.0, k)
        phi = rng.uniform(0.0, 2.0 * np.pi, k)
        r = np.sqrt(1.0 - z * z)
        return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)

    wo, wi = hemi(n), hemi(n)
    dielectric = kw["type"] == DIELECTRIC
    across = rng.uniform(size=n) < (0.5 if dielectric else 0.2)
    if dielectric:
        # half of the transmission pairs are refractions of wo through a facet normal drawn around n,
        # so that enough of them have a facet that faces both directions
        ior = float(np.float32(kw["ior"]))
        m = hemi(n) * np.array([0.5, 0.5, 1.0])
        m /= np.linalg.norm(m, axis=1, keepdims=True)
        for inside in (False, True):
            eta = ior if inside else 1.0 / ior
            c = (wo * m).sum(1)
            k = 1.0 - eta * eta * (1.0 - c * c)
            wt = -eta * wo + (eta * c - np.sqrt(np.maximum(k, 0.0)))[:, None] * m
            use = across & (np.arange(n) % 2 == 0) & (k > 0.05) & (c > 0.05) & (wt[:, 2] < -0.02) & ((np.arange(n) % 4 < 2) == inside)
            wi[use] = wt[use] * np.array([1.0, 1.0, -1.0])     # (flipped below with the rest of `across`)
    wi[across, 2] = -wi[across, 2]
    below = np.arange(n) % 4 < 2
    wo[below, 2], wi[below, 2] = -wo[below, 2], -wi[below, 2]
    wi, wo = wi.astype(np.float32), wo.astype(np.float32)
    # conditioning, judged on the float32 inputs in float64
    a, b = wi.astype(np.float64), wo.astype(np.float64)
    same = a[:, 2] * b[:, 2] > 0
    keep = np.ones(n, bool)
    h = a + b
    h /= np.maximum(np.linalg.norm(h, axis=1, keepdims=True), 1e-30)
    keep &= ~same | ((np.abs((a * h).sum(1)) >= 0.02) & (np.abs((b * h).sum(1)) >= 0.02))
    if dielectric:
        ior = float(np.float32(kw["ior"]))
        n_o = np.where(b[:, 2] < 0, ior, 1.0)[:, None]
        n_i = np.where(b[:, 2] < 0, 1.0, ior)[:, None]
        ht = n_o * b + n_i * a
        ht /= np.maximum(np.linalg.norm(ht, axis=1, keepdims=True), 1e-30)
        keep &= same | ((np.abs((a * ht).sum(1)) >= 0.02) & (np.abs((b * ht).sum(1)) >= 0.02))
        # ... and transmission pairs away from the critical angle, where 1 - F has a square-root
        # singularity (its relative condition number is unbounded): sin^2 of the refracted angle
        # at least 0.02 from 1
        sin2_t = (n_o[:, 0] / n_i[:, 0]) ** 2 * (1.0 - (b * ht).sum(1) ** 2)
        keep &= same | (np.abs(sin2_t - 1.0) >= 0.02)
    return wi[keep], wo[keep], keep.mean()


def hash_name(name):
    return int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") % (1 << 31)


def ref_pair(L, kw, wi, wo, features):
    """bsdf_ref's (f, pdf) in float64 and in float32 on the same float32 inputs."""
    mat = R.material(**kw)
    vndf = bool(features & VNDF)
    r64 = R.evaluate(L, mat, wi, wo, vndf, np.float64)
    r32 = R.evaluate(L, mat, wi, wo, vndf, np.float32)
    return r64, tuple(x.astype(np.float64) for x in r32)


def check_values_and_pdfs(bsdf_eval, L, name, kw, two, feat):
    """One case of the value / pdf comparison for an evaluator bsdf_eval(kw, wi, wo, features) ->
    (f, pdf); returns the worst K needed (printed by the callers' -s runs)."""
    kw = dict(kw, two_sided=two)
    wi, wo, kept = eval_inputs(name, kw)
    r64, r32 = ref_pair(L, kw, wi, wo, feat)
    assert kept >= 0.95, kept
    assert (r64[0].max(1) > 0).mean() >= 0.25, (r64[0].max(1) > 0).mean()
    f, pdf = bsdf_eval(kw, wi, wo, feat)
    assert np.isfinite(f).all() and np.isfinite(pdf).all()
    kf, kp = tolerance_ratio(f, r64[0], r32[0]), tolerance_ratio(pdf, r64[1], r32[1])
    print(f"{name} two_sided={two} features={feat}: kept {kept:.3f} nonzero {(r64[0].max(1) > 0).mean():.3f} K f {kf.max():.2f} pdf {kp.max():.2f}")
    assert kf.max() <= TOLERANCE_K, (kf.max(), wi[kf.max(1).argmax()], wo[kf.max(1).argmax()])
    assert kp.max() <= TOLERANCE_K, (kp.max(), wi[kp.argmax()], wo[kp.argmax()])
    return max(kf.max(), kp.max())


@pytest.mark.parametrize("name,kw,two,feat", EVAL_CASES, ids=[f"{c[0]}-two{int(c[2])}-f{c[3]}" for c in EVAL_CASES])
def test_values_and_pdfs_against_float64_reference(oracle_mod, golden_luts, ref_luts, name, kw, two, feat):
    """EvaluateBSDF / EvaluateBSDFPdf of the oracle against bsdf_ref in float64 at the pairs of
    eval_inputs (at least 95 % of 4 000 kept, at least 25 % with a nonzero f; both asserted):
    per element |got - ref64| <= K e + 4 float32 ulps of ref64, e the float32 run's own error (see
    tolerance_ratio for its floor). K = 6: the worst ratio seen on the oracle over all cases is 3.95
    (a multiscattering dielectric's pdf; 3.80 for an f), and K covers the product's different
    order of the same operations with half as much again. Without the floor single elements at
    which the float32 run happens to land on the float64 value would ask for K in the tens of
    thousands, and without keeping transmission pairs off the critical angle for 26."""
    def ev(kw, wi, wo, features):
        return oracle_mod.bsdf_eval(golden_luts, oracle_mod.bsdf_material(**kw), wi, wo, features)
    check_values_and_pdfs(ev, ref_luts, name, kw, two, feat)


# ---- 2. the samplers draw from their pdf ------------------------------------------------------------
CHI_DRAWS = 200_000
CHI_BINS = (32, 64)     # cos(theta) in [-1, 1] x phi in [-pi, pi]: the horizon is a bin edge
CHI_SUB = (16, 8)       # sub-grid per bin in cos and in phi for the expected counts
CHI_CASES = [(n, kw, z) for n, kw in MATERIALS for z in (0.9, 0.3)]
# (the two-sided one once from below)
CHI_CASES += [(n, dict(kw, two_sided=two), z) for n, kw, two in SMOOTH_PLASTICS for z in (0.9, -0.3 if two else 0.3)]
DELTA_RATE = 1e-6       # the two-sided false-alarm rate of the delta-draw count, CHI_Z's 1e-6


def sampler_numbers(seed, n):
    """(n, 3) float32 numbers in [0, 1) with 24 random bits each (exact in float32, never 1)."""
    return (np.random.default_rng(seed).integers(0, 1 << 24, (n, 3)) / float(1 << 24)).astype(np.float32)


def expected_bin_mass(L, kw, wo1, sub=CHI_SUB):
    """Per (cos, phi) bin, the integral of bsdf_ref's sampled density (a midpoint rule on a sub-grid;
    finer in cos, where the refracted lobe ends sharply), and the same restricted to where the
    reported pdf is positive."""
    nc, nphi = CHI_BINS
    sc, sp = sub
    c = -1.0 + (np.arange(nc * sc) + 0.5) * (2.0 / (nc * sc))
    phi = -np.pi + (np.arange(nphi * sp) + 0.5) * (2.0 * np.pi / (nphi * sp))
    cc, pp = np.meshgrid(c, phi, indexing="ij")
    s = np.sqrt(1.0 - cc * cc)
    wi = np.stack([s * np.cos(pp), s * np.sin(pp), cc], -1).reshape(-1, 3)
    wo = np.broadcast_to(wo1.astype(np.float64), wi.shape)
    mat = R.material(**kw)
    d = R.sampled_density(L, mat, wi, wo)
    lit = R.evaluate(L, mat, wi, wo, True)[1] > 0
    cell = (2.0 / (nc * sc)) * (2.0 * np.pi / (nphi * sp))
    shape = (nc, sc, nphi, sp)
    return d.reshape(shape).sum((1, 3)) * cell, (d * lit).reshape(shape).sum((1, 3)) * cell


def check_sampler(bsdf_sample, L, name, kw, woz):
    """Chi-square of CHI_DRAWS draws of bsdf_sample(kw, wo, u) -> (wi, f, pdf, delta) against the
    expected bin masses, and the share of draws with a positive pdf against its integral. Returns
    chi-square per degree of freedom.

    A sampler with a delta lobe (smooth plastic's coat, probability c = the sum of `delta_lobes`'
    probabilities at wo; 0 for every rough material, which then may not flag a single draw): the
    draws that are not flagged delta follow sampled_density / (1 - c), by the same chi-square over
    their own number; the count of flagged draws is binomial(n, c), held to |k - n c| <=
    z sqrt(n c (1 - c)) + 1, z the two-sided normal quantile of DELTA_RATE (n c is in the
    thousands: the normal approximation is good) and the 1 for the sampler's own arithmetic: the
    numbers are multiples of 2^-24 and its float32 weight is a float32 ulp from c, which together
    move the expected count by n (2^-24 + 2^-23 c) < 0.04."""
    wo1 = np.array([np.sqrt(1.0 - woz * woz), 0.0, woz], np.float32)
    n = CHI_DRAWS
    u = sampler_numbers(hash_name(name) + int(woz * 10), n)
    wi, f, pdf, delta = bsdf_sample(kw, np.broadcast_to(wo1, (n, 3)), u)
    mat = R.material(**kw)
    c = float(sum(l[2] for l in R.delta_lobes(mat, wo1, L=L))) if R.is_smooth(mat) else 0.0
    assert 0.0 <= c < 1.0
    z = NormalDist().inv_cdf(1.0 - DELTA_RATE / 2.0)
    k_bound = z * np.sqrt(n * c * (1.0 - c)) + (1.0 if c else 0.0)
    assert abs(delta.sum() - n * c) <= k_bound, (int(delta.sum()), n * c, k_bound)
    mass, lit_mass = expected_bin_mass(L, kw, wo1)
    mass = mass / (1.0 - c)
    m = int((~delta).sum())                     # the chi-square is over the draws that are not delta
    drawn = ~delta & np.isfinite(wi).all(1) & (np.abs(wi).max(1) > 0)
    w = wi[drawn].astype(np.float64)
    obs, _, _ = np.histogram2d(w[:, 2], np.arctan2(w[:, 1], w[:, 0]), bins=CHI_BINS, range=[[-1, 1], [-np.pi, np.pi]])
    # merge bins in raster order until each group expects at least 5 draws; "no direction" is a group
    e = np.append(mass.ravel() * m, max(1.0 - mass.sum(), 0.0) * m)
    o = np.append(obs.ravel(), m - drawn.sum())
    ge, go, ae, ao = [], [], 0.0, 0.0
    for ei, oi in zip(e, o):
        ae, ao = ae + ei, ao + oi
        if ae >= 5.0:
            ge.append(ae); go.append(ao); ae, ao = 0.0, 0.0
    ge[-1] += ae; go[-1] += ao
    ge, go = np.array(ge), np.array(go)
    chi2, dof = ((go - ge) ** 2 / ge).sum(), len(ge) - 1
    valid = (~delta & (pdf > 0)).mean()
    lit = min(lit_mass.sum(), 1.0)
    print(f"{name} wo.z={woz}: chi2/dof {chi2 / dof:.3f} (dof {dof}, bound {chi_square_quantile(dof) / dof:.3f}), "
          f"valid {valid:.4f} against {lit:.4f}, density integral {mass.sum():.4f}, "
          f"delta draws {int(delta.sum())} against {n * c:.1f} +- {k_bound:.1f}")
    assert dof >= 100
    assert chi2 < chi_square_quantile(dof), (chi2, dof)
    assert abs(valid - lit) < 5.0 * np.sqrt(lit * (1.0 - lit) / n) + 1e-3, (valid, lit)
    return chi2 / dof


@pytest.mark.parametrize("name,kw,woz", CHI_CASES, ids=[f"{c[0]}-z{c[2]}" for c in CHI_CASES])
def test_samplers_draw_from_their_pdf(oracle_mod, golden_luts, ref_luts, name, kw, woz):
    """200 000 draws of the oracle's SampleBSDF (VNDF) per rough material and wo.z, binned on a
    32 x 64 (cos theta, phi) grid over the sphere, against bsdf_ref's sampled density integrated per
    bin; bins merged until each expects at least 5 draws; chi-square below the p = 1e-6 quantile.
    The seeds are fixed; observed chi-square per degree of freedom: 0.96 to 1.05 over the twelve
    cases (850 to 1 984 degrees of freedom, bounds 1.16 to 1.25). The share of draws with a
    positive pdf matches the density's integral over where the reported pdf is positive (the
    mass VNDF sampling sends below the horizon is drawn but invalid) within 5 standard errors +
    1e-3. Tried once on a scratch copy of the oracle: with sample_ggx always drawing from the NDF
    while the pdf stays the VNDF's, all twelve cases fail (chi-square per degree of freedom from
    1.9 for plastic_rough at wo.z = 0.9 to above 70 000). The four smooth-plastic cases (CHI_CASES' tail)
    draw their coat as a delta lobe: chi-square per degree of freedom 0.97 to 1.00 over the Lambert draws,
    and 8 093 to 50 386 delta draws, each within 0.3 of its binomial bound (see check_sampler)."""
    def smp(kw, wo, u):
        return oracle_mod.bsdf_sample(golden_luts, oracle_mod.bsdf_material(**kw), wo, u, VNDF)
    check_sampler(smp, ref_luts, name, kw, woz)


# ---- 3. the tables against a quadrature -----------------------------------------------------------------
# The table builder's compiled constants, as its "%f" formatting printed them (BxDFTexturesBuilding.cpp:
# 77-81): the cosine and alpha steps, the ior step, and -- the one that matters -- the sample weight
# 1 / samples printed as 0.000049 and 0.000010, so that weight x samples is not 1.
LUT_STEP_COS = np.float32(0.032258)
LUT_TABLES = {
    # name: (alpha step, samples, printed weight, has Fresnel, is BSDF)
    "brdf": (np.float32(0.032258), 20480, 0.000049, False, False),
    "brdf_dielectric": (np.float32(0.066667), 20480, 0.000049, True, False),
    "bsdf": (np.float32(0.066667), 98304, 0.000010, True, True),
}
LUT_STEP_IOR = np.float32(0.133333)
LUT_QUAD = {"brdf": 64, "brdf_dielectric": 128, "bsdf": 128}    # quadrature resolution n per table


def lut_texel_parameters(table, tx, ty, slice_):
    """(cos_o, alpha, eta_o, eta_i) of a texel in the builder's float32 arithmetic
    (BxDFTexturesBuilding.hlsl:42-45, 79-80): slices 16-31 see the boundary from the dense side."""
    cos_o = np.maximum(np.float32(tx) * LUT_STEP_COS, np.float32(0.0001))
    alpha = np.float32(ty) * LUT_TABLES[table][0]
    ior = np.float32(slice_ % 16) * LUT_STEP_IOR + np.float32(1.0)
    entering = slice_ >= 16
    return float(cos_o), float(alpha), float(ior if entering else 1.0), float(1.0 if entering else ior)


def _gauss(n, lo, hi):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (hi - lo) * x + 0.5 * (hi + lo), 0.5 * (hi - lo) * w


def _sign_changes(v):
    """Where consecutive rows (axis -2) of v differ in sign, both finite."""
    return (v[..., :-1, :] * v[..., 1:, :] < 0) & np.isfinite(v[..., :-1, :]) & np.isfinite(v[..., 1:, :])


def _kink_breaks(kinks, phi, grid=256, iters=40):
    """For each phi, the theta in (0, pi/2) at which one of the kink functions -- kinks(theta, phi)
    returns them stacked on axis 0 -- changes sign: found on a grid and refined by bisection,
    sorted and padded with pi/2 to one width: (len(phi), P)."""
    th = np.linspace(0.0, np.pi / 2, grid + 1)
    v = kinks(th[:, None], phi[None, :])
    kk, i, j = np.nonzero(_sign_changes(v))
    lo, hi, flo = th[i], th[i + 1], v[kk, i, j]
    pick = np.arange(len(kk))
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        left = kinks(mid, phi[j])[kk, pick] * flo > 0
        lo, hi = np.where(left, mid, lo), np.where(left, hi, mid)
    roots = [[] for _ in phi]
    for jj, r in zip(j, 0.5 * (lo + hi)):
        roots[jj].append(r)
    width = max(len(r) for r in roots)
    return np.array([sorted(r) + [np.pi / 2] * (width - len(r)) for r in roots]).reshape(len(phi), width)


def _smooth_gauss(n, lo, hi):
    """Gauss-Legendre in u on x = lo + (hi - lo) u^2 (3 - 2 u): nodes and weights in x. A function
    that starts like a square root at either end is smooth in u."""
    x, w = np.polynomial.legendre.leggauss(n)
    u, wu = 0.5 * (x + 1.0), 0.5 * w
    return lo + (hi - lo) * (u * u * (3.0 - 2.0 * u)), (hi - lo) * (6.0 * u * (1.0 - u)) * wu


def _azimuth_breaks(kinks, grid=96, theta_grid=256, iters=24):
    """The azimuths in (0, pi) at which the number of sign changes in theta of a kink function
    changes (a kink curve touches a line of constant azimuth, or leaves through theta = pi / 2):
    there the inner integral has a kink in phi. With 0, pi / 2 and pi, sorted."""
    th = np.linspace(0.0, np.pi / 2, theta_grid + 1)[:, None]

    def signature(phi):
        return _sign_changes(kinks(th, phi[None, :])).sum(1)

    phi = np.linspace(0.0, np.pi, grid + 1)
    sig = signature(phi)
    i = np.nonzero((sig[:, :-1] != sig[:, 1:]).any(0))[0]
    lo, hi, slo = phi[i], phi[i + 1], sig[:, i]
    for _ in range(iters if len(i) else 0):
        mid = 0.5 * (lo + hi)
        same = (signature(mid) == slo).all(0)
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    return np.unique(np.concatenate([[0.0, np.pi / 2, np.pi], 0.5 * (lo + hi)]))


def albedo_quadrature(table, cos_o, alpha, eta_o, eta_i, n=None):
    """E[w] and E[w^2] of the builder's estimator w = f |cos| / pdf over its visible-normal draws,
    in float64: the integral over the normals m of the visible-normal density G1(wo) max(0, wo.m)
    D(m) / wo.n times w, in m's own polar angle theta and azimuth phi about the surface normal
    (sample_vndf instead maps a disk onto the hemisphere seen from wo). The integrand is smooth
    between kinks (see `kinks`), so both directions are cut there and each stretch gets n / 4
    Gauss-Legendre nodes: phi over half the circle (the other half mirrors it: wo lies in the xz
    plane), cut where the number of kinks along theta changes; theta cut at the kinks and at 2, 6,
    18, ... alpha, D's peak being alpha wide. f and pdf are bsdf_ref's; for the BSDF table each
    normal reflects with probability F and refracts otherwise, and f is the builder's variant
    without the radiance scale."""
    _, _, _, fresnel, is_bsdf = LUT_TABLES[table]
    n = n or LUT_QUAD[table]
    if is_bsdf and eta_o == eta_i:           # the sampler passes straight through; the evaluator has no
        return 0.0, 0.0                      # half vector for wi = -wo and reports pdf 0
    wo1 = np.array([np.sqrt(1.0 - cos_o * cos_o), 0.0, cos_o])
    eta = eta_o / eta_i

    def normal(th, ph):
        th, ph = np.broadcast_arrays(th, ph)
        return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1)

    def branches(m):
        """wo.m, the refraction discriminant, and the mirrored and refracted directions."""
        c = m @ wo1
        k = 1.0 - eta * eta * (1.0 - c * c)
        return c, k, 2.0 * c[..., None] * m - wo1, -eta * wo1 + (eta * c - np.sqrt(np.maximum(k, 0.0)))[..., None] * m

    def kinks(th, ph):
        """The functions whose zero sets are the integrand's kinks, stacked: wo.m (the normal turns
        away), the mirrored direction's height (it crosses the horizon), the discriminant (the
        critical angle), and for the BSDF the refracted direction's height and, for either event,
        the two products with which the evaluator asks whether its own half vector of (wi, wo)
        faces both directions."""
        m = normal(th, ph)
        c, k, wi_r, wi_t = branches(m)
        out = [c, wi_r[..., 2]]
        if fresnel and eta > 1:
            out.append(k)
        if is_bsdf:
            live = (k > 0) & (c > 0)
            out.append(np.where(live, wi_t[..., 2], np.nan))
            for wi, ok in ((wi_r, c > 0), (wi_t, live)):
                h = R.generalized_half_vector(wi, np.broadcast_to(wo1, wi.shape), eta_o, eta_i)
                out += [np.where(ok, (h * wi).sum(-1) * wi[..., 2], np.nan), np.where(ok, (h @ wo1) * cos_o, np.nan)]
        return np.stack(out, 0)

    cuts = _azimuth_breaks(kinks)
    panels = [_smooth_gauss(max(n // 4, 8), a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    phi, wphi = np.concatenate([q[0] for q in panels]), np.concatenate([q[1] for q in panels])
    n = len(phi)
    graded = alpha * 2.0 * 3.0 ** np.arange(8)          # D's peak has width alpha: panels 2, 6, 18, ... alpha
    graded = np.broadcast_to(np.minimum(graded, np.pi / 2), (n, 8))
    edges = np.sort(np.concatenate([np.zeros((n, 1)), graded, _kink_breaks(kinks, phi), np.full((n, 1), np.pi / 2)], 1), 1)
    x, wx = np.polynomial.legendre.leggauss(max(n // 4, 8))
    lo, hi = edges[:, :-1, None], edges[:, 1:, None]
    # (on each stretch theta = lo + (hi - lo) u^2 (3 - 2 u): 1 - F starts like a square root at the
    # critical angle, which this substitution turns into a smooth function of u)
    u, wu = 0.5 * (x + 1.0), 0.5 * wx
    ps = (lo + (hi - lo) * (u * u * (3.0 - 2.0 * u))).reshape(n, -1)
    wq = (((hi - lo) * (6.0 * u * (1.0 - u)) * wu).reshape(n, -1) * wphi[:, None] * 2.0).ravel()
    ph = np.broadcast_to(phi[:, None], ps.shape).ravel()
    ps = ps.ravel()
    use = wq > 0
    ps, ph, wq = ps[use], ph[use], wq[use]
    m = normal(ps, ph)
    wo = np.broadcast_to(wo1, m.shape)
    wom, k, wi_r, wi_t = branches(m)
    a2 = alpha * alpha
    g1_over_cos = 2.0 / (np.sqrt(a2 + (1.0 - a2) * cos_o * cos_o) + cos_o)     # G1(wo) / wo.n, finite at grazing
    density = np.sin(ps) * R.ggx_d(m[:, 2], alpha) * g1_over_cos * np.maximum(wom, 0.0) * wq
    if not is_bsdf:
        val, pdf, woh = R.cook_torrance_brdf(wi_r, wo, alpha, True)
        if fresnel:
            val = val * R.fresnel_dielectric(woh, eta_o, eta_i)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(pdf > 0, val * np.abs(wi_r[:, 2]) / pdf, 0.0)
        return (density * w).sum(), (density * w * w).sum()
    F = R.fresnel_dielectric(np.maximum(wom, 0.0), eta_o, eta_i)
    e1 = e2 = 0.0
    for wi, p in ((wi_r, F), (wi_t, np.where(k > 0, 1.0 - F, 0.0))):
        val, pdf = R.rough_dielectric(wi, wo, alpha, eta_o, eta_i, True, False)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(pdf > 0, val * np.abs(wi[:, 2]) / pdf, 0.0)
        e1, e2 = e1 + (density * p * w).sum(), e2 + (density * p * w * w).sum()
    return e1, e2


def lut_texels(table):
    """The texels of a table the quadrature is run on: all of brdf above alpha row 0; of the two
    arrays a seeded spread that holds, for both halves (leaving / entering), ior slices 0 (ior 1)
    and 15, alpha rows 1 and 15 and cos columns 0, 1 and 31 in every combination, four texels
    beyond the critical angle, and 180 random ones."""
    if table == "brdf":
        return [(tx, ty, 0) for ty in range(1, 32) for tx in range(32)]
    rng = np.random.default_rng(7 if table == "bsdf" else 8)
    t = {(tx, ty, half * 16 + z) for half in (0, 1) for z in (0, 15) for ty in (1, 15) for tx in (0, 1, 31)}
    t |= {(3, 7, 31), (21, 8, 20), (21, 15, 20), (10, 2, 25)}
    while len(t) < 208:
        t.add((int(rng.integers(32)), int(rng.integers(1, 16)), int(rng.integers(32))))
    return sorted(t)


def lut_golden(table):
    g = np.load(GOLDEN / "bxdf_luts.npz")[table].astype(np.float64) / 65535.0
    return g.reshape((1, 32, 32) if table == "brdf" else (32, 16, 32))


@pytest.mark.parametrize("table", list(LUT_TABLES))
def test_lut_texels_against_quadrature(table):
    """Every golden texel (see lut_texels) lies within 5 sigma + 1/65535 of clip(k E, 0, 1): E the
    float64 directional albedo (albedo_quadrature), k the builder's printed sample weight times its
    sample count -- 0.000049 x 20480 = 1.00352 for brdf and brdf_dielectric, 0.000010 x 98304 =
    0.98304 for bsdf -- and sigma = k sqrt((E[w^2] - E[w]^2) / N) the Monte Carlo standard error of
    the table's N samples. Each texel is bounded on its own: all texels share their random numbers,
    so their errors are correlated. Worst z = |golden - expected| / (sigma + 1/65535/5) seen: brdf
    2.68, brdf_dielectric 2.47, bsdf 2.22; with k = 1 instead it is 11.5, 9.6 and 391."""
    alpha_step, samples, weight, fresnel, is_bsdf = LUT_TABLES[table]
    k = weight * samples
    assert abs(k - (0.98304 if is_bsdf else 1.00352)) < 1e-12
    golden = lut_golden(table)
    texels = lut_texels(table)
    assert len(texels) >= 200
    if table != "brdf":
        params = np.array([lut_texel_parameters(table, *t) for t in texels])
        tir = (params[:, 2] > 1) & (params[:, 0] < np.sqrt(1.0 - 1.0 / params[:, 2] ** 2))
        assert tir.sum() >= 20 and {t[2] % 16 for t in texels} >= {0, 15} and {t[2] // 16 for t in texels} == {0, 1}
    worst, worst_raw = 0.0, 0.0
    bad = []
    for tx, ty, sl in texels:
        e1, e2 = albedo_quadrature(table, *lut_texel_parameters(table, tx, ty, sl))
        sigma = k * np.sqrt(max(e2 - e1 * e1, 0.0) / samples)
        got = golden[sl, ty, tx]
        err = abs(got - np.clip(k * e1, 0.0, 1.0))
        z = err / (sigma + 0.2 / 65535.0)
        worst, worst_raw = max(worst, z), max(worst_raw, abs(got - np.clip(e1, 0.0, 1.0)) / (sigma + 0.2 / 65535.0))
        if err > 5.0 * sigma + 1.0 / 65535.0:
            bad.append((tx, ty, sl, got, k * e1, sigma))
    print(f"{table}: {len(texels)} texels, worst z {worst:.2f}; with k = 1 it would be {worst_raw:.2f}")
    assert not bad, bad[:10]


CONVERGENCE_TEXELS = [("brdf", 0, 1, 0), ("brdf", 31, 1, 0), ("brdf", 16, 8, 0), ("brdf", 1, 31, 0),
                      ("brdf_dielectric", 31, 1, 31), ("brdf_dielectric", 10, 15, 20), ("brdf_dielectric", 3, 7, 31),
                      ("bsdf", 0, 1, 15), ("bsdf", 1, 15, 31), ("bsdf", 12, 7, 20), ("bsdf", 17, 15, 8)]


@pytest.mark.parametrize("table,tx,ty,sl", CONVERGENCE_TEXELS, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in CONVERGENCE_TEXELS])
def test_quadrature_is_converged(table, tx, ty, sl):
    """Doubling the quadrature's resolution moves E[w] and E[w^2] by at most 1e-5: at grazing and
    at normal incidence, at the smallest and the largest alpha, beyond the critical angle."""
    p = lut_texel_parameters(table, tx, ty, sl)
    a, b = albedo_quadrature(table, *p), albedo_quadrature(table, *p, n=2 * LUT_QUAD[table])
    assert abs(a[0] - b[0]) <= 1e-5 and abs(a[1] - b[1]) <= 1e-5, (a, b)


def test_lut_smooth_rows():
    """Alpha row 0 is the smooth branch and has no noise: every sample of brdf weighs 1, of
    brdf_dielectric F(cos) and of bsdf 1 (F / F or T / T), so the texels are clip(k), clip(k F) and
    k = 0.98304, to one UNORM16 step. F is bsdf_ref's in float32, the builder's precision: at the
    first column's cos = 0.0001 the sine rounds to 1, and between equal indices (ior slice 0) the
    test "sin(theta_t) >= 1" of Fresnel.inc.hlsl:16-21 then reports total reflection where the
    exact F is 0; the table holds that 1."""
    lsb = 1.0 / 65535.0
    assert (lut_golden("brdf")[0, 0] == 1.0).all()
    bd, bs = lut_golden("brdf_dielectric"), lut_golden("bsdf")
    for sl in range(32):
        p = np.array([lut_texel_parameters("brdf_dielectric", tx, 0, sl) for tx in range(32)])
        F = R.fresnel_dielectric(p[:, 0], p[0, 2], p[0, 3], np.float32).astype(np.float64)
        assert sl % 16 or (F[0] == 1.0 and R.fresnel_dielectric(p[0, 0], 1.0, 1.0) < 1e-12)
        assert np.abs(bd[sl, 0] - np.clip(1.00352 * F, 0.0, 1.0)).max() <= lsb, sl
        assert np.abs(bs[sl, 0] - 0.98304).max() <= lsb, sl


def test_lut_averages():
    """The three *_avg tables are the builder's trapezoid rule over each row of their main table
    (BxDFTexturesBuilding.hlsl:127-160): 2 / 31 (f(0) 0.0001 / 2 + sum_{i=1}^{30} f(i) (i 0.032258)
    + f(31) / 2), written to [slice / 16][slice % 16][alpha]; recomputed in float64 from the golden
    main tables they agree to one UNORM16 step -- except that the builder averages its float
    tables before they are clamped to 1, so where the row's last texel (cos = 1, weight 1/2) is
    saturated the stored average may exceed the recomputed one by up to (k - 1) / 31 = 7.4 steps
    (seen: 5.2 steps on the three such rows of brdf; at most 0.6 steps everywhere else)."""
    arrays = np.load(GOLDEN / "bxdf_luts.npz")
    lsb = 1.0 / 65535.0
    w = np.arange(32) * float(LUT_STEP_COS)
    w[0], w[31] = 0.0001 / 2, 0.5

    def average(rows):
        return np.clip((rows * w).sum(-1) * 2.0 / 31.0, 0.0, 1.0)

    def check(got, rows):
        want = average(rows)
        over = np.where(rows[..., 31] >= 1.0, (1.00352 - 1.0) / 31.0, 0.0)
        assert (got >= want - lsb).all() and (got <= want + over + lsb).all(), np.abs(got - want).max()

    check(arrays["brdf_avg"].astype(np.float64) / 65535.0, lut_golden("brdf")[0])
    for name in ("brdf_dielectric", "bsdf"):
        got = (arrays[name + "_avg"].astype(np.float64) / 65535.0).reshape(2, 16, 16)      # [slice][ior][alpha]
        rows = lut_golden(name).reshape(2, 16, 16, 32)                                    # [half][ior][alpha][cos]
        check(got, rows)


DELTA_MATERIALS = [
    ("smooth_dielectric", dict(type=DIELECTRIC, alpha=0.0, ior=1.5)),
    ("smooth_dielectric_2.4", dict(type=DIELECTRIC, alpha=0.0, ior=2.4)),
    ("thin_dielectric", dict(type=THIN, alpha=0.0, ior=1.5)),
    ("smooth_conductor", dict(type=CONDUCTOR, albedo=(3.9, 2.4, 1.1), alpha=0.0, ior=(0.2, 0.9, 1.4), two_sided=True)),
    ("smooth_plastic", dict(type=PLASTIC, albedo=(0.7, 0.6, 0.5), alpha=0.0, ior=1.5, internal_scattering=0)),
    ("smooth_plastic_1.8_isf1", dict(type=PLASTIC, albedo=(0.9, 0.5, 0.1), alpha=0.0, ior=1.8, internal_scattering=1)),
    ("smooth_plastic_two_isf2", dict(type=PLASTIC, albedo=(0.9, 0.5, 0.1), alpha=0.0, ior=1.5, two_sided=True, internal_scattering=2)),
]
DELTA_DIRECTIONS = 64


def check_delta_lobes(bsdf_sample, bsdf_eval, L, name, kw):
    """One material of DELTA_MATERIALS for a sampler bsdf_sample(kw, wo, u) -> (wi, f, pdf, delta) and an
    evaluator bsdf_eval(kw, wi, wo, features) -> (f, pdf), at 64 seeded wo, alternately above and below.

    A smooth dielectric, thin sheet or conductor has delta lobes only: with the selection number at 0
    and just below 1 the sampler returns bsdf_ref's first and last lobe at that wo -- direction, f
    and probability to a relative 2e-5 (a refracted direction's float32 cancellation at grazing wo
    included) -- every draw flagged delta.

    A smooth plastic is mixed, and its delta lobe is the LAST interval of the selection number
    (`sel < w_l` is Lambert): at sel = 1 - 2^-24 the draw is the coat of `delta_lobes`, to the same
    2e-5 and flagged delta; at sel = 0 it is a Lambert draw, not flagged, whose f and pdf are
    `evaluate` at the returned direction within check_values_and_pdfs' tolerance. Every wo that has
    the coat has a coat weight strictly between 0 and 1 (asserted), so both branches are reached;
    from inside a one-sided plastic there is no lobe at all: f = 0, pdf = 0, not delta."""
    rng = np.random.default_rng(hash_name(name))
    n = DELTA_DIRECTIONS
    z = rng.uniform(0.05, 1.0, n) * np.where(np.arange(n) % 2, -1.0, 1.0)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    wo = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1).astype(np.float32)
    mat = R.material(**kw)
    lobes = [R.delta_lobes(mat, wo[i], L=L) for i in range(n)]
    if kw["type"] != PLASTIC:
        for sel, pick in ((0.0, 0), (1.0 - 2.0 ** -24, -1)):
            u = np.tile(np.array([0.3, 0.6, sel], np.float32), (n, 1))
            wi, f, pdf, delta = bsdf_sample(kw, wo, u)
            assert delta.all()
            for i in range(n):
                rwi, rf, rp = lobes[i][pick]
                np.testing.assert_allclose(wi[i], rwi, rtol=2e-5, atol=2e-6)
                np.testing.assert_allclose(f[i], rf, rtol=2e-5)
                np.testing.assert_allclose(pdf[i], rp, rtol=2e-5)
        return
    has = np.array([len(l) == 1 for l in lobes])
    assert (has == ((z > 0) | bool(kw.get("two_sided")))).all() and has.sum() >= n // 2
    coat = np.array([float(l[0][2]) if l else 0.0 for l in lobes])
    assert ((coat[has] > 0) & (coat[has] < 1)).all(), (coat[has].min(), coat[has].max())
    u = sampler_numbers(hash_name(name) + 1, n)
    # -- the last interval: the coat
    u[:, 2] = 1.0 - 2.0 ** -24
    wi, f, pdf, delta = bsdf_sample(kw, wo, u)
    assert (delta == has).all()
    assert not f[~has].any() and not pdf[~has].any()
    for i in np.flatnonzero(has):
        rwi, rf, rp = lobes[i][0]
        np.testing.assert_allclose(wi[i], rwi, rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(f[i], rf, rtol=2e-5)
        np.testing.assert_allclose(pdf[i], rp, rtol=2e-5)
    # -- the first: the Lambert base, described by `evaluate`
    u[:, 2] = 0.0
    wi, f, pdf, delta = bsdf_sample(kw, wo, u)
    assert not delta.any()
    assert not f[~has].any() and not pdf[~has].any()
    wi, wo_h, f, pdf = wi[has], wo[has], f[has], pdf[has]
    assert (wi[:, 2] * wo_h[:, 2] > 0).all() and (pdf > 0).all() and (f > 0).all()
    r64 = R.evaluate(L, mat, wi, wo_h, True, np.float64)
    r32 = tuple(x.astype(np.float64) for x in R.evaluate(L, mat, wi, wo_h, True, np.float32))
    kf, kp = tolerance_ratio(f, r64[0], r32[0]), tolerance_ratio(pdf, r64[1], r32[1])
    print(f"{name}: coat weight {coat[has].min():.4f} to {coat[has].max():.4f}; Lambert draw K f {kf.max():.2f} pdf {kp.max():.2f}")
    assert kf.max() <= TOLERANCE_K and kp.max() <= TOLERANCE_K, (kf.max(), kp.max())
    ef, ep = bsdf_eval(kw, wi, wo_h, VNDF)          # ... and the evaluator says the same of the pair
    assert tolerance_ratio(ef, r64[0], r32[0]).max() <= TOLERANCE_K and tolerance_ratio(ep, r64[1], r32[1]).max() <= TOLERANCE_K


@pytest.mark.parametrize("name,kw", DELTA_MATERIALS, ids=[m[0] for m in DELTA_MATERIALS])
def test_delta_lobes_against_float64_reference(oracle_mod, golden_luts, ref_luts, name, kw):
    """check_delta_lobes on the oracle's SampleBSDF / EvaluateBSDF: the smooth and thin materials' delta
    lobes, and both intervals of a smooth plastic's selection number."""
    def smp(kw, wo, u):
        return oracle_mod.bsdf_sample(golden_luts, oracle_mod.bsdf_material(**kw), wo, u, VNDF)

    def ev(kw, wi, wo, features):
        return oracle_mod.bsdf_eval(golden_luts, oracle_mod.bsdf_material(**kw), wi, wo, features)
    check_delta_lobes(smp, ev, ref_luts, name, kw)
