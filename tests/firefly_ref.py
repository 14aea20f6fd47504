"""The firefly re-weighting of include/dcrt.h ("firefly re-weighting": Zirr, Hanika, Dachsbacher 2018) restated in
numpy: the split of a sample over two cascades, the cascade films' accumulation and the resolve. With dtype
float32 every operation is the definition's, in its order, so the GPU's cascades and re-weighted image match bit
for bit; with float64 the same functions are the version the float32 one is held to (tests/test_firefly_ref.py).

The accumulation is built on film_ref's filter weights: film_model convolves one image's shares. film_ref's
float32 box and triangle weights are the kernels' own bits; its Gaussian, Mitchell and Lanczos weights are the
textbook formulas, a few ulp from the kernels' det_exp / coefficient-table / det_sin forms, so a caller that
wants the kernels' bits for those passes `convolve`, e.g. the oracle's sample_convolution (which the film kernel
is held to bit for bit): the shares, the per-image sums and their addition stay this module's.
"""
import numpy as np

import film_ref

MAX_CASCADES = 8


def make_params(cascades=6, start=1.0, base=8.0, min_support=3.0):
    from directcomputeraytracing_amd import FireflyParams
    return FireflyParams(int(cascades), float(start), float(base), float(min_support))


def constants(params, dtype=np.float32):
    """(s [K], r, d, kappa) in `dtype`: s_j by sequential products, r = 1 / base, d = 1 - r."""
    T = np.dtype(dtype).type
    s = np.empty(int(params.cascades), dtype)
    x = T(params.start)
    for j in range(len(s)):
        s[j] = x
        x = T(x * T(params.base))
    r = T(T(1) / T(params.base))
    return s, r, T(T(1) - r), T(params.min_support)


def luminance(rgb):
    """Y = fmaxf(0, r * 0.299 + g * 0.587 + b * 0.114) in rgb's dtype, summed left to right (a NaN reads 0)."""
    T = rgb.dtype.type
    return np.fmax(T(0), (rgb[..., 0] * T(0.299) + rgb[..., 1] * T(0.587)) + rgb[..., 2] * T(0.114))


def split(Y, params):
    """(band, alpha) of luminances Y (in Y's dtype): cascade `band` takes alpha, band + 1 takes 1 - alpha."""
    T = Y.dtype.type
    s, r, d, _ = constants(params, Y.dtype)
    K = len(s)
    band = np.zeros(Y.shape, np.int64)
    sj = np.full(Y.shape, s[0], Y.dtype)
    for i in range(1, K - 1):
        m = Y > s[i]
        band[m] = i
        sj[m] = s[i]
    with np.errstate(all="ignore"):
        alpha = np.fmin(np.fmax((sj / Y - r) / d, T(0)), T(1))
    low, high = Y <= s[0], Y > s[K - 1]
    alpha = np.where(low | high, T(1), alpha).astype(Y.dtype)
    band = np.where(low, 0, np.where(high, K - 1, band))
    return band, alpha


def shares(val, params, dtype=np.float32):
    """(K, H, W, 3): share_j(v) of every sample of one image, alpha v in `band`, (1 - alpha) v in band + 1, +0 elsewhere."""
    T = np.dtype(dtype).type
    rgb = np.asarray(val)[..., :3].astype(dtype)
    band, alpha = split(luminance(rgb), params)
    lo = rgb * alpha[..., None]
    hi = rgb * (T(1) - alpha)[..., None]
    out = np.zeros((int(params.cascades),) + rgb.shape, dtype)
    for j in range(int(params.cascades)):
        out[j] = np.where((band == j)[..., None], lo, np.where((band + 1 == j)[..., None], hi, T(0)))
    return out


def model_convolve(dtype):
    def convolve(filter_params, pos, val4):
        return film_ref.film_model(filter_params, pos, val4, dtype)[0]
    return convolve


def accumulate(cascades, filter_params, images, params, dtype=np.float32, convolve=None):
    """One film pass over `images` [(pos, val)] into `cascades` (K, H, W, 4), in place: per image and cascade the
    per-image sum of share * w (convolve(filter, pos, share as RGBA) from a zero film), then C.rgb = C.rgb + sum.
    C.w is left alone."""
    convolve = convolve or model_convolve(dtype)
    for pos, val in images:
        sh = shares(val, params, dtype)
        for j in range(sh.shape[0]):
            v4 = np.concatenate([sh[j], np.zeros(sh[j].shape[:2] + (1,), dtype)], -1)
            cascades[j, ..., :3] = cascades[j, ..., :3] + convolve(filter_params, pos, v4)[..., :3].astype(dtype)
    return cascades


def neighbourhood_sum(c):
    """The 3 x 3 sum around every pixel of (H, W) `c`, sequential from 0, rows then columns; outside counts 0."""
    H, W = c.shape
    padded = np.zeros((H + 2, W + 2), c.dtype)
    padded[1:-1, 1:-1] = c
    total = np.zeros((H, W), c.dtype)
    for dy in range(3):
        for dx in range(3):
            total = total + padded[dy:dy + H, dx:dx + W]
    return total


def resolve(film, cascades, image_count, params, dtype=np.float32):
    """(out (H, W, 4), omega (K, H, W)) of the resolve over `film` (H, W, 4) and `cascades` (K, H, W, 4)."""
    T = np.dtype(dtype).type
    s, _, _, kappa = constants(params, dtype)
    K = len(s)
    film = np.asarray(film).astype(dtype)
    cas = np.asarray(cascades).astype(dtype)
    Wt = film[..., 3]
    valid = Wt > 0
    N = T(image_count)
    sums = []
    with np.errstate(all="ignore"):
        for i in range(K):
            count = np.where(valid, (N * luminance(cas[i, ..., :3])) / (Wt * s[i]), T(0)).astype(dtype)
            sums.append(neighbourhood_sum(count))
        omega = np.ones((K,) + Wt.shape, dtype)
        acc = cas[0, ..., :3].copy()
        for j in range(1, K):
            S = sums[j - 1] + sums[j]
            if j + 1 < K:
                S = S + sums[j + 1]
            omega[j] = np.fmin(np.fmax((S - T(1)) / kappa, T(0)), T(1))
            acc = acc + cas[j, ..., :3] * omega[j][..., None]
        rgb = acc / Wt[..., None]
    out = np.zeros(film.shape, dtype)
    out[..., :3] = np.where(valid[..., None], rgb, T(0))
    out[..., 3] = np.where(valid, T(1), T(0))
    return out, omega


# ---- the prototype's synthetic run (the issue's table) --------------------------------------------
def synthetic_run(images, seed=1):
    """`images` images of a 32 x 32 film for the box filter of radius 0.5: a background in [0.2, 0.8], a 4 x 4 lamp
    block where every sample is 50, a 16 x 16 region where 2 % of the samples are 40, and one planted sample of
    5000 (image 0, pixel (5, 25)). Returns ([(pos, val)], planted (y, x), lamp slice, rare slice)."""
    rng = np.random.default_rng(seed)
    H = W = 32
    lamp = (slice(4, 8), slice(4, 8))
    rare = (slice(14, 30), slice(2, 18))
    planted = (5, 25)
    out = []
    for k in range(images):
        pos = np.minimum(rng.uniform(0.0, 1.0, (H, W, 2)).astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))
        grey = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32)
        val = np.repeat(grey[..., None], 4, -1)
        val[lamp] = 50.0
        hot = rng.uniform(0.0, 1.0, (16, 16)) < 0.02
        region = val[rare]
        region[hot] = 40.0
        val[rare] = region
        if k == 0:
            val[planted] = 5000.0
        val[..., 3] = 1.0
        out.append((pos, val))
    return out, planted, lamp, rare
