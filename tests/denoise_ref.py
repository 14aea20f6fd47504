"""The film denoiser of include/dcrt.h ("film denoiser") restated in numpy float32, operation for
operation: every product, sum, quotient and square root below is one float32 operation in the
order the header states, and exp is the library's det_exp polynomial through the oracle's own
export (oracle.math_eval(2, .)). The library is built without FMA contraction and with correctly
rounded division and square root, so the GPU result equals this one bit for bit
(tests/test_gpu_denoise.py); tests/test_denoise_ref.py pins this restatement by itself.

A helper module in the style of tests/random_scenes.py: no tests here.
"""
import numpy as np

F = np.float32
H5 = [F(1.0) / F(16.0), F(1.0) / F(4.0), F(3.0) / F(8.0), F(1.0) / F(4.0), F(1.0) / F(16.0)]
G3 = [F(1.0) / F(4.0), F(1.0) / F(2.0), F(1.0) / F(4.0)]
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.2, sigma_albedo=0.1, demodulate=1)


def same_bits(a, b):
    """Bit-identical, except that a NaN matches any NaN (as in tests/test_gpu_output_views.py)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def det_exp(x):
    import oracle
    x = np.ascontiguousarray(x, np.float32)
    return oracle.math_eval(2, x.ravel()).reshape(x.shape)


def resolve(film):
    """f.w > 0 ? f.rgb / f.w : 0"""
    film = np.asarray(film, np.float32)
    w = film[..., 3:4]
    pos = w > 0
    return np.where(pos, film[..., :3] / np.where(pos, w, F(1.0)), F(0.0)).astype(np.float32)


def lum(x):
    return x[..., 0] * F(0.299) + x[..., 1] * F(0.587) + x[..., 2] * F(0.114)


def dist2(q, p):
    d = q - p
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _tap(img, dx, dy):
    """img at p + (dx, dy) for every pixel p, and which of those taps lie inside the image
    (the others hold some pixel's finite values and are never added)."""
    Hh, Ww = img.shape[:2]
    ys, xs = np.arange(Hh) + dy, np.arange(Ww) + dx
    vy, vx = (ys >= 0) & (ys < Hh), (xs >= 0) & (xs < Ww)
    out = img[np.clip(ys, 0, Hh - 1)][:, np.clip(xs, 0, Ww - 1)]
    return out, vy[:, None] & vx[None, :]


def _add(acc, term, valid):
    return np.where(valid if acc.ndim == 2 else valid[..., None], acc + term, acc)


def variance0(c0, n, a, kn, ka):
    l = lum(c0)
    m1, m2, ws = (np.zeros(l.shape, np.float32) for _ in range(3))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            nq, valid = _tap(n, dx, dy)
            aq, _ = _tap(a, dx, dy)
            lq, _ = _tap(l, dx, dy)
            wg = det_exp(-(dist2(nq, n) * kn + dist2(aq, a) * ka))
            m1 = _add(m1, lq * wg, valid)
            m2 = _add(m2, lq * lq * wg, valid)
            ws = _add(ws, wg, valid)
    mean = m1 / ws
    return np.maximum(m2 / ws - mean * mean, F(0.0))


def atrous_pass(c, var, n, a, step, sigma_l, kn, ka):
    gs, gw = np.zeros(var.shape, np.float32), np.zeros(var.shape, np.float32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            vq, valid = _tap(var, dx, dy)
            w = G3[dy + 1] * G3[dx + 1]
            gs = _add(gs, vq * w, valid)
            gw = _add(gw, np.full(var.shape, w, np.float32), valid)
    gv = gs / gw
    if sigma_l > 0:
        kl = F(1.0) / (F(sigma_l) * np.sqrt(gv) + F(1e-6))
    else:
        kl = np.zeros(var.shape, np.float32)
    l = lum(c)
    total = np.zeros(c.shape, np.float32)
    sv, ws = np.zeros(var.shape, np.float32), np.zeros(var.shape, np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, valid = _tap(c, dx * step, dy * step)
            vq, _ = _tap(var, dx * step, dy * step)
            nq, _ = _tap(n, dx * step, dy * step)
            aq, _ = _tap(a, dx * step, dy * step)
            e = np.abs(lum(cq) - l) * kl + dist2(nq, n) * kn + dist2(aq, a) * ka
            w = (H5[dy + 2] * H5[dx + 2]) * det_exp(-e)
            total = _add(total, cq * w[..., None], valid)
            sv = _add(sv, vq * (w * w), valid)
            ws = _add(ws, w, valid)
    return total / ws[..., None], sv / (ws * ws)


def denoise(color, normal, albedo, iterations=5, sigma_luminance=4.0, sigma_normal=0.2, sigma_albedo=0.1, demodulate=1):
    """Three H x W x 4 float32 films (sum w*L, sum w) -> the denoised H x W x 4 image (c_N * d, 1)."""
    assert 1 <= iterations <= 8
    sn, sa = F(sigma_normal), F(sigma_albedo)
    kn = F(1.0) / (sn * sn) if sn > 0 else F(0.0)
    ka = F(1.0) / (sa * sa) if sa > 0 else F(0.0)
    c, a = resolve(color), resolve(albedo)
    n = F(2.0) * resolve(normal) - F(1.0)
    d = np.maximum(a, F(1e-3)) if demodulate else np.ones(a.shape, np.float32)
    with np.errstate(all="ignore"):
        c = c / d
        var = variance0(c, n, a, kn, ka)
        for i in range(iterations):
            c, var = atrous_pass(c, var, n, a, 1 << i, F(sigma_luminance), kn, ka)
        out = np.empty(c.shape[:2] + (4,), np.float32)
        out[..., :3] = c * d
    out[..., 3] = F(1.0)
    return out


def film(rgb, weight=None):
    """An H x W x 3 image as a film: (w * rgb, w), w = 1 unless given."""
    rgb = np.asarray(rgb, np.float32)
    w = np.ones(rgb.shape[:2], np.float32) if weight is None else np.asarray(weight, np.float32)
    return np.concatenate([rgb * w[..., None], w[..., None]], axis=-1).astype(np.float32)


def encode_normal(n):
    """The Shading Normal view's encoding, n * 0.5 + 0.5."""
    return np.asarray(n, np.float32) * F(0.5) + F(0.5)


def piecewise_guides(rng, W, H):
    """Guide films whose normal and albedo are constant on a few rectangles (so the edge-stopping
    terms are exactly 0 inside a region and large across), with random film weights."""
    nrm = np.zeros((H, W, 3), np.float32)
    alb = np.zeros((H, W, 3), np.float32)
    xs = sorted({0, W, *rng.integers(0, W + 1, 2).tolist()})
    ys = sorted({0, H, *rng.integers(0, H + 1, 2).tolist()})
    for y0, y1 in zip(ys[:-1], ys[1:]):
        for x0, x1 in zip(xs[:-1], xs[1:]):
            v = rng.normal(size=3)
            nrm[y0:y1, x0:x1] = (v / np.linalg.norm(v)).astype(np.float32)
            alb[y0:y1, x0:x1] = rng.uniform(0.05, 0.95, 3).astype(np.float32)
    # a little variation inside the regions, so the guide weights are not all 0 or 1
    nrm += rng.normal(0.0, 0.02, nrm.shape).astype(np.float32)
    alb = np.clip(alb + rng.normal(0.0, 0.01, alb.shape), 0.0, 1.0).astype(np.float32)
    w = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    return film(encode_normal(nrm), w), film(alb, w)


def random_inputs(seed, W, H):
    """Seeded finite films for the bit-for-bit cases: colour of any film weight (a few pixels with
    w = 0), piecewise guides."""
    rng = np.random.default_rng(seed)
    rgb = rng.gamma(2.0, 0.4, (H, W, 3)).astype(np.float32)
    w = rng.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    w[rng.random((H, W)) < 0.02] = 0.0
    color = film(rgb, w)
    normal, albedo = piecewise_guides(rng, W, H)
    return color, normal, albedo


def synthetic_scene(noise_sigma=0.5, seed=7, W=48, H=40):
    """The noise-reduction image: two halves with different normal and albedo, a 4-pixel albedo
    checker of +-25 %, a vertical irradiance ramp 0.3 .. 1.0 with a x0.25 shadow rectangle that
    appears in no guide, multiplicative log-normal noise of unit mean.
    Returns (clean rgb, noisy colour film, normal film, albedo film)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    left = xx < W // 2
    nrm = np.where(left[..., None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])).astype(np.float32)
    base = np.where(left[..., None], np.array([0.7, 0.5, 0.3]), np.array([0.3, 0.5, 0.7]))
    checker = np.where(((xx // 4) + (yy // 4)) % 2 == 0, 1.25, 0.75)
    alb = (base * checker[..., None]).astype(np.float32)
    irradiance = 0.3 + 0.7 * yy / (H - 1.0)
    irradiance = np.where((xx >= 10) & (xx < 30) & (yy >= 12) & (yy < 28), irradiance * 0.25, irradiance)
    clean = (alb * irradiance[..., None]).astype(np.float32)
    noise = rng.lognormal(-0.5 * noise_sigma * noise_sigma, noise_sigma, clean.shape)
    noisy = (clean * noise).astype(np.float32)
    return clean, film(noisy), film(encode_normal(nrm)), film(alb)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
