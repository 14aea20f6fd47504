"""tests/firefly_ref.py, the restatement of dcrt.h "firefly re-weighting", against itself in float64, against the
split's identities, against the oracle's film, and on the prototype's synthetic run. CPU only: the GPU kernels are
held to firefly_ref bit for bit in tests/test_gpu_firefly.py."""
import numpy as np
import pytest

import film_ref
import firefly_ref

EPS32 = float(np.finfo(np.float32).eps)


def make_filter(kind, radius):
    from directcomputeraytracing_amd import FilterParams
    return FilterParams(int(kind), float(radius), 1.5, 1 / 3, 1 / 3, 3)


def random_images(rng, W, H, count, lo=1 / 8, hi=8 * 32768.0):
    """Grey-ish non-negative samples, luminances log-uniform over [lo, hi]."""
    out = []
    for _ in range(count):
        pos = np.minimum(rng.uniform(0.0, 1.0, (H, W, 2)).astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))
        lum = np.exp(rng.uniform(np.log(lo), np.log(hi), (H, W, 1)))
        val = (lum * rng.uniform(0.5, 1.5, (H, W, 4))).astype(np.float32)
        val[..., 3] = 1.0
        out.append((pos, val))
    return out


def alpha_bound(params, eps):
    """|alpha error| of the split in arithmetic of unit roundoff eps on non-negative samples: Y has 5 operations
    and s_j at most K - 1 products, so s_j / Y carries (K + 5) eps relative and is < 1; r adds eps, the subtraction
    one more; d = 1 - r carries 1.5 eps absolute, 1.5 eps / d relative, and the division one more: in all at most
    (K + 10) eps / d."""
    d = 1.0 - 1.0 / float(params.base)
    return (int(params.cascades) + 10) * eps / d


# ---- float32 against float64 -----------------------------------------------------------------------
def test_cascades_float32_against_float64():
    """Per cascade pixel: |C32 - C64| <= mag * (alpha_bound + (taps + images + 3) eps), mag = sum |w| max|v|
    (film_model's magnitude sum): a share differs by at most |v| alpha_bound plus eps for its product, a tap adds
    one product and one addition, each image one more addition. The box filter with offsets in [0.01, 0.99] keeps
    every sample 0.01 from a support edge (r = 1.5: the edges sit at offsets 0 and 1), so the weights are the same
    0s and 1s in both precisions and the bound is the firefly arithmetic's alone; film_ref's own float32 weights
    are test_film_ref's subject."""
    W, H, n = 21, 19, 3
    params = firefly_ref.make_params(6, 1.0, 8.0, 3.0)
    filt = make_filter(film_ref.BOX, 1.5)
    images = [(np.clip(pos, 0.01, 0.99), val) for pos, val in random_images(np.random.default_rng(0), W, H, n)]
    K = int(params.cascades)
    c32 = firefly_ref.accumulate(np.zeros((K, H, W, 4), np.float32), filt, images, params, np.float32)
    c64 = firefly_ref.accumulate(np.zeros((K, H, W, 4), np.float64), filt, images, params, np.float64)
    mag = sum(film_ref.film_model(filt, pos, val, np.float64)[1] for pos, val in images)
    taps = (2 * 3 + 1) ** 2          # film_model's square window at r = 1.5
    bound = mag * (alpha_bound(params, EPS32) + (taps + n + 3) * EPS32)
    err = np.abs(c32[..., :3].astype(np.float64) - c64[..., :3]).max(-1)
    assert (err <= bound[None]).all(), float((err / bound[None]).max())
    assert err.max() > 0 and np.abs(c64[..., :3]).max() > 1.0 and not c32[..., 3].any()


def test_resolve_float32_against_float64():
    """The resolve over the same (float32-valued) film and cascades: a count carries 8 eps relative (5 for Y, two
    products, one division), T nine additions more, S two more and S - 1 one: with S < kappa + 1 wherever omega is
    not clamped to 1, |omega error| <= 21 eps (kappa + 1) / kappa + eps. out = (sum_j omega_j C_j) / W then differs
    by at most (sum_j |C_j| / W) * (that + (K + 2) eps)."""
    W, H, n = 23, 17, 5
    params = firefly_ref.make_params(6, 1.0, 8.0, 2.5)
    filt = make_filter(film_ref.TRIANGLE, 1.0)
    images = random_images(np.random.default_rng(3), W, H, n, hi=4096.0)
    K = int(params.cascades)
    cas = firefly_ref.accumulate(np.zeros((K, H, W, 4), np.float32), filt, images, params)
    film = sum(film_ref.film_model(filt, pos, val, np.float32)[0] for pos, val in images).astype(np.float32)
    o32, w32 = firefly_ref.resolve(film, cas, n, params, np.float32)
    o64, w64 = firefly_ref.resolve(film, cas, n, params, np.float64)
    kappa = float(params.min_support)
    omega_tol = EPS32 * (21 * (kappa + 1) / kappa + 1)
    assert np.abs(w32.astype(np.float64) - w64).max() <= omega_tol
    scale = np.abs(cas[..., :3].astype(np.float64)).sum(0) / film[..., 3:4].astype(np.float64)
    assert (np.abs(o32[..., :3].astype(np.float64) - o64[..., :3]) <= scale * (omega_tol + (K + 2) * EPS32)).all()
    mid = (w64 > 0) & (w64 < 1)
    assert mid.any() and (w64 == 0).any() and (w64[1:] == 1).any()


# ---- the split ---------------------------------------------------------------------------------------
def boundary_luminances(params):
    s = firefly_ref.constants(params, np.float32)[0]
    ys = [np.float32(0)]
    for x in s:
        ys += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))]
    return np.array(ys, np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cascades,start,base", [(2, 1.0, 8.0), (6, 1.0, 8.0), (8, 0.37, 3.3), (5, 2.0, 1.5)])
def test_split_identities(dtype, cascades, start, base):
    """alpha_j + alpha_{j+1} = 1 to one rounding of 1 - alpha and one of the sum (eps in all), and the once-only
    count alpha_j Y / s_j + alpha_{j+1} Y / s_{j+1} = 1 to base * (alpha_bound + 4 eps): Y / s_j <= base, and the
    two quotients, two products and the sum add 4 eps. Y at, just below and just above every s_j, and in between."""
    params = firefly_ref.make_params(cascades, start, base, 3.0)
    eps = float(np.finfo(dtype).eps)
    s = firefly_ref.constants(params, dtype)[0]
    K = len(s)
    rng = np.random.default_rng(cascades)
    Y = np.concatenate([boundary_luminances(params), np.exp(rng.uniform(np.log(start / 8), np.log(float(s[-1]) * 8), 4096)).astype(np.float32)])
    Y = Y.astype(dtype)
    band, alpha = firefly_ref.split(Y, params)
    one = dtype(1)
    beta = one - alpha
    assert (np.abs((alpha + beta).astype(np.float64) - 1.0) <= eps).all()
    assert (alpha >= 0).all() and (alpha <= 1).all() and (band >= 0).all() and (band < K).all()
    # exactly these comparisons
    assert (band[Y <= s[0]] == 0).all() and (alpha[Y <= s[0]] == 1).all()
    assert (band[Y > s[-1]] == K - 1).all() and (alpha[Y > s[-1]] == 1).all()
    inner = (Y > s[0]) & (Y <= s[-1])
    assert (s[band[inner]] < Y[inner]).all() and (Y[inner] <= s[band[inner] + 1]).all()
    j = band[inner]
    once = alpha[inner] * (Y[inner] / s[j]) + beta[inner] * (Y[inner] / s[j + 1])
    tol = float(base) * (alpha_bound(params, eps) + 4 * eps)
    assert (np.abs(once.astype(np.float64) - 1.0) <= tol).all(), float(np.abs(once.astype(np.float64) - 1.0).max() / tol)
    # and the shares of a sample sum to the sample, to the two products' and the sum's roundings
    v = np.stack([Y, Y, Y], -1)[None]
    total = firefly_ref.shares(v, params, dtype).sum(0)
    assert (np.abs(total.astype(np.float64) - v) <= 3 * eps * np.abs(v)).all()


# ---- against the oracle's film -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(5))
def test_cascades_sum_to_the_oracle_film(oracle_mod, kind):
    """sum_j C_j against sample_convolution's film on non-negative samples, the cascades convolved by the oracle too:
    per tap the two shares differ from v by 3 eps |v| in sum (two products, one of 1 - alpha), and the cascade sums
    and the film's add the same taps in other groupings: (taps + images + 2) eps mag on each side."""
    W, H, n = 37, 29, 3
    params = firefly_ref.make_params(6, 1.0, 8.0, 3.0)
    filt = make_filter(kind, 1.5)
    images = random_images(np.random.default_rng(40 + kind), W, H, n)
    film = np.zeros((H, W, 4), np.float32)
    for pos, val in images:
        oracle_mod.sample_convolution(filt, pos, val, film)
    cas = firefly_ref.accumulate(np.zeros((6, H, W, 4), np.float32), filt, images, params,
                                 convolve=lambda f, p, v: oracle_mod.sample_convolution(f, p, v))
    mag = sum(film_ref.film_model(filt, pos, val, np.float64)[1] for pos, val in images)
    taps = (2 * 3 + 1) ** 2
    bound = mag * EPS32 * (3 + 2 * (taps + n + 2))
    err = np.abs(cas[..., :3].astype(np.float64).sum(0) - film[..., :3]).max(-1)
    assert (err <= bound).all(), float((err / bound).max())
    assert (cas[..., :3] != 0).any(axis=(1, 2, 3)).all()      # every cascade took something


# ---- the prototype's synthetic run -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_synthetic_run_at_16_images(dtype):
    images, planted, lamp, rare = firefly_ref.synthetic_run(16)
    params = firefly_ref.make_params()
    filt = make_filter(film_ref.BOX, 0.5)
    cas = firefly_ref.accumulate(np.zeros((6, 32, 32, 4), dtype), filt, images, params, dtype)
    film = np.zeros((32, 32, 4), dtype)
    for pos, val in images:
        film = film + film_ref.film_model(filt, pos, val, dtype)[0]
    out, omega = firefly_ref.resolve(film, cas, 16, params, dtype)
    lum = lambda x: x[..., :3].astype(np.float64) @ np.array([0.299, 0.587, 0.114])
    plain = film[..., :3] / film[..., 3:4]
    print("film at the planted pixel", lum(plain)[planted], "re-weighted", lum(out)[planted], "lamp", lum(out)[lamp].mean(),
          "rare region film", lum(plain)[rare].mean(), "re-weighted", lum(out)[rare].mean())
    assert lum(plain)[planted] > 300.0
    assert lum(out)[planted] <= 0.8
    inner = (slice(5, 7), slice(5, 7))
    whole = cas[:, inner[0], inner[1], :3].astype(np.float64).sum(0) / film[inner][..., 3:4].astype(np.float64)
    assert np.allclose(out[inner][..., :3], whole, rtol=1e-6, atol=0)
    assert np.allclose(lum(out)[inner], 50.0, rtol=1e-5)
    assert lum(out).sum() <= lum(plain).sum()


# ---- adaptive sampling's sentinel ----------------------------------------------------------------------
def test_sentinel_sample_changes_no_cascade_bit():
    """A sentinel sample of adaptive sampling (position +inf, value 0) adds nothing to any cascade."""
    W, H = 16, 12
    params = firefly_ref.make_params()
    filt = make_filter(film_ref.BOX, 0.5)
    rng = np.random.default_rng(5)
    first = random_images(rng, W, H, 2)
    (pos, val), = random_images(rng, W, H, 1)
    masked_pos, masked_val = pos.copy(), val.copy()
    masked_pos[3:9, 2:10] = np.inf
    masked_val[3:9, 2:10] = 0.0
    before = firefly_ref.accumulate(np.zeros((6, H, W, 4), np.float32), filt, first, params)
    with np.errstate(invalid="ignore"):
        after = firefly_ref.accumulate(before.copy(), filt, [(masked_pos, masked_val)], params)
    untouched = np.zeros((H, W), bool)
    untouched[3:9, 2:10] = True
    assert np.array_equal(before[:, untouched].view(np.uint32), after[:, untouched].view(np.uint32))
    assert not np.array_equal(before[:, ~untouched], after[:, ~untouched])
