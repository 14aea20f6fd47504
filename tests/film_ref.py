"""Independent numpy models of the image-space passes: film reconstruction (SampleConvolution)
and post-processing (SumLuminance + PostProcessings + the sRGB encode).

Nothing here comes from the oracle or the library: the filter weights are the textbook formulas
(Mitchell & Netravali 1988 eq. 8 from B and C, not the host-made coefficient table; numpy's
normalised sinc), gathered over a square window instead of the shader's per-pixel bounds, and
evaluated in float64 or float32. tests/test_film_ref.py holds the oracle to these models; the GPU
is then held to the oracle bit for bit (tests/test_gpu_film_kernels.py).
"""
import numpy as np

BOX, TRIANGLE, GAUSSIAN, MITCHELL, LANCZOS = range(5)


def mitchell_netravali(x, B, C):
    """k(x) of Mitchell & Netravali, "Reconstruction Filters in Computer Graphics", eq. 8
    (support |x| < 2, k(0) = (6 - 2B) / 6)."""
    x = np.abs(x)
    one = x.dtype.type(1)
    near = (12 - 9 * B - 6 * C) * x ** 3 + (-18 + 12 * B + 6 * C) * x ** 2 + (6 - 2 * B)
    far = (-B - 6 * C) * x ** 3 + (6 * B + 30 * C) * x ** 2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C)
    return np.where(x < one, near, np.where(x < 2 * one, far, 0 * one)) / x.dtype.type(6)


def weight_1d(fp, d):
    """The 1-D reconstruction weight at signed distance d (an array of the evaluation dtype)."""
    T = d.dtype.type
    r = T(fp.radius)
    a = np.abs(d)
    if fp.filter == BOX:
        return (a <= r).astype(d.dtype)
    if fp.filter == TRIANGLE:
        return np.maximum(T(0), r - a)
    if fp.filter == GAUSSIAN:
        alpha = T(fp.gaussian_alpha)
        return np.maximum(T(0), np.exp(-alpha * d * d) - np.exp(-alpha * r * r))
    if fp.filter == MITCHELL:
        return mitchell_netravali(T(2) * a / r, T(fp.mitchell_b), T(fp.mitchell_c))
    if fp.filter == LANCZOS:
        tau = T(fp.lanczos_tau or 3)    # 0 reads as the default 3
        return np.where(a <= r, np.sinc(d) * np.sinc(d / tau), T(0))
    raise ValueError(f"unknown filter {fp.filter}")


def film_model(filter_params, pos, val, dtype=np.float64):
    """The film contribution of one image: pos (H, W, 2) sub-pixel offsets (a sample's position is
    its pixel's corner plus its offset), val (H, W, >= 3). Pixel centre c gathers every sample s
    with weight w(cx - sx) * w(cy - sy): rgb = sum w * v.rgb, w = sum w. Returns the (H, W, 4) film
    in `dtype` and the (H, W) magnitude sum |w| * |v| (float64, |v| the largest of |r|, |g|, |b| and
    the 1 the weight sum adds), the scale of a pixel's rounding error."""
    T = np.dtype(dtype).type
    H, W = pos.shape[:2]
    sx = pos[..., 0].astype(dtype) + np.arange(W, dtype=dtype)[None, :]
    sy = pos[..., 1].astype(dtype) + np.arange(H, dtype=dtype)[:, None]
    rgb = val[..., :3].astype(dtype)
    mag_v = np.maximum(np.abs(val[..., :3].astype(np.float64)).max(-1), 1.0)   # (the weight sum's "value" is 1)
    cx = np.arange(W, dtype=dtype) + T(0.5)
    cy = np.arange(H, dtype=dtype) + T(0.5)
    reach = int(min(max(W, H), np.floor(float(filter_params.radius) + 0.5) + 1))   # one wider than floor(r + 0.5)
    film = np.zeros((H, W, 4), dtype)
    mag = np.zeros((H, W), np.float64)
    for dy in range(-reach, reach + 1):
        # destination rows [y0, y1) gather from source rows [y0 + dy, y1 + dy)
        y0, y1 = max(0, -dy), min(H, H - dy)
        if y0 >= y1:
            continue
        for dx in range(-reach, reach + 1):
            x0, x1 = max(0, -dx), min(W, W - dx)
            if x0 >= x1:
                continue
            src = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            dst = (slice(y0, y1), slice(x0, x1))
            w = weight_1d(filter_params, cx[None, x0:x1] - sx[src]) * weight_1d(filter_params, cy[y0:y1, None] - sy[src])
            film[dst + (slice(0, 3),)] += w[..., None] * rgb[src]
            film[dst + (3,)] += w
            mag[dst] += np.abs(w.astype(np.float64)) * mag_v[src]
    return film, mag


# Radii with the sub-pixel offsets that put a sample exactly on a pixel centre's support edge,
# |d| == r, exactly so in float32 and float64 (all dyadic): at offset o the distance to the centre
# k pixels on is k + 0.5 - o.
SUPPORT_EDGE_CASES = [(0.75, (0.75, 0.25)), (1.25, (0.25, 0.75)), (2.0, (0.5, 0.5))]


def pairs_on_support_edge(pos, radius):
    """(pixel, sample) pairs of the gather windows whose weight is decided on the support edge:
    |dx| == r with |dy| <= r or the other way round, in the kernels' float32 arithmetic."""
    H, W = pos.shape[:2]
    r = np.float32(radius)
    f = np.float32
    sx = pos[..., 0] + np.arange(W, dtype=f)[None, :]
    sy = pos[..., 1] + np.arange(H, dtype=f)[:, None]
    cx, cy = np.arange(W, dtype=f) + f(0.5), np.arange(H, dtype=f) + f(0.5)
    dx = np.abs(cx[:, None, None] - sx[None])                                   # (pixel x, sample y, sample x)
    dy = np.abs(cy[:, None, None] - sy[None])                                   # (pixel y, sample y, sample x)
    ix, iy = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    in_x = (ix >= np.floor(cx - r)[:, None, None]) & (ix <= np.floor(cx + r)[:, None, None])
    in_y = (iy >= np.floor(cy - r)[:, None, None]) & (iy <= np.floor(cy + r)[:, None, None])
    on_x, on_y = (dx == r) & in_x, (dy == r) & in_y
    return int(((on_x[None] & ((dy <= r) & in_y)[:, None]) | (on_y[:, None] & ((dx <= r) & in_x)[None])).sum())


# ---- post-processing ------------------------------------------------------------------------------
# Film sizes (W, H) by the partial sums of the first reduction pass, (((W + 7) / 8 + 1) / 2) *
# (((H + 7) / 8 + 1) / 2): up to 128 the second pass is one group, 256 x 128 gives exactly 128,
# 2049 x 9 gives 129 (two passes), and beyond 16384 (8200 x 520: 16929; every 4K film) three.
POSTFX_SIZES = [(1, 1), (8, 8), (16, 16), (17, 16), (16, 17), (33, 19), (256, 128), (2049, 9), (8200, 520)]

# (enabled, auto_exposure, ev100, luminance_white): auto exposure, manual exposure at EV100 -10,
# 0, 6 and 20, luminance_white 0, 0.5, 1 and 1e3, post-FX off
POSTFX_PARAMETERS = ([(1, 1, 0.0, 1.0)] + [(1, 0, ev, 1.0) for ev in (-10.0, 0.0, 6.0, 20.0)]
                     + [(1, 1, 0.0, lw) for lw in (0.0, 0.5, 1e3)] + [(1, 0, 0.0, 0.5), (1, 0, 0.0, 0.0), (0, 0, 0.0, 1.0)])


def partial_sums(W, H):
    return (((W + 7) // 8 + 1) // 2) * (((H + 7) // 8 + 1) // 2)


def synthetic_film(W, H, seed):
    """A seeded random film with weights other than 1 (rgb already multiplied by the weight)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 3.0, (H, W, 1))
    rgb = rng.uniform(0.0, 1.0, (H, W, 3)) ** 3 * 4.0     # (dark-heavy: most of the sRGB range at EV100 0)
    return np.concatenate([rgb * w, w], -1).astype(np.float32)


def srgb_encode(x):
    """IEC 61966-2-1 encode of a linear value clamped to [0, 1] (NaN reads as 0)."""
    x = np.clip(np.nan_to_num(x, nan=0.0), 0.0, 1.0)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055)


def sum_log_luminance_model(film):
    """SumLuminance in float64: sum of log(1e-4 + luminance) over the reduction's padded domain
    (16 x 16-texel cells; texels outside the film, and texels of weight <= 0, count as black)."""
    film = np.asarray(film, np.float64)
    H, W = film.shape[:2]
    bx, by = ((W + 7) // 8 + 1) // 2, ((H + 7) // 8 + 1) // 2
    with np.errstate(all="ignore"):
        rgb = np.where(film[..., 3:4] > 0, film[..., :3] / film[..., 3:4], 0.0)
    lum = np.zeros((16 * by, 16 * bx))
    lum[:H, :W] = np.clip(rgb, 0, 65000) @ np.array([0.299, 0.587, 0.114])
    return float(np.log(1e-4 + lum).sum())


def postfx_model(film, params):
    """Post-processing in float64: (codes (H, W, 3) as real numbers in [0, 255] before rounding to
    the sRGB8 code, sum of log luminance). Exposure 1 / (1.2 * 2^EV100), EV100 given or, with auto
    exposure, log2(100 / 12.5 * the log-average luminance); Reinhard c (1 + c / white^2) / (1 + c);
    both skipped with post-FX off."""
    film = np.asarray(film, np.float64)
    H, W = film.shape[:2]
    total = sum_log_luminance_model(film)
    with np.errstate(all="ignore"):
        c = film[..., :3] / film[..., 3:4]
        if params.enabled:
            ev = np.log2(np.exp(total / (W * H)) * 100 / 12.5) if params.auto_exposure else float(params.ev100)
            c = c / (1.2 * 2.0 ** ev)
            c = c * (1 + c / float(params.luminance_white) ** 2) / (1 + c)
        return srgb_encode(c) * 255, total
