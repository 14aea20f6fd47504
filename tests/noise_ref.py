"""The film noise estimate of include/dcrt.h ("film noise estimate") restated in numpy float32,
operation by operation: per pixel, the 16 x 16 tile tree, the 128-group tree over the tile sums,
the statistics. The GPU kernels must match it bit for bit (tests/test_gpu_noise.py);
tests/test_noise_ref.py holds it to a plain float64 model of the same formulas.

Every float32 operation below is one correctly rounded IEEE operation on float32 arrays (numpy
does not contract), in the order the header gives.
"""
import numpy as np

TILE = 16
F = np.float32


def same_bits(a, b):
    """Bit-identical, except that a NaN matches any NaN (the default NaN's sign differs between
    x86 and gfx950)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def pixel_error(film, half):
    """(e H x W float32, valid H x W bool)."""
    f, h = np.asarray(film, np.float32), np.asarray(half, np.float32)
    with np.errstate(all="ignore"):
        valid = (f[..., 3] > 0) & (h[..., 3] > 0)            # (a NaN weight compares false)
        c = f[..., :3] / f[..., 3:4]
        a = h[..., :3] / h[..., 3:4]
        d = (np.abs(c[..., 0] - a[..., 0]) + np.abs(c[..., 1] - a[..., 1])) + np.abs(c[..., 2] - a[..., 2])
        s = (c[..., 0] + c[..., 1]) + c[..., 2]
        n = np.sqrt(np.fmax(s, F(0)))                        # (fmaxf: a NaN s gives 0)
        e = d / (n + F(1e-4))
    e = np.where(valid, e, F(0)).astype(np.float32)
    return e, valid


def tree(values, width):
    """acc[t] = acc[t] + acc[t + k] for k = width / 2 .. 1 over the last axis (width a power of 2)."""
    acc = np.array(values, np.float32)
    assert acc.shape[-1] == width
    k = width // 2
    with np.errstate(all="ignore"):
        while k >= 1:
            acc[..., :k] = acc[..., :k] + acc[..., k:2 * k]
            k //= 2
    return acc[..., 0]


def tiles_of(image, fill):
    """H x W -> tilesY x tilesX x 256 (t = ty * 16 + tx), padded with `fill`."""
    H, W = image.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    pad = np.full((ty * TILE, tx * TILE), fill, image.dtype)
    pad[:H, :W] = image
    return pad.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)


def reduce_groups(values):
    """Groups of 128 consecutive values, zero padded, tree 64 .. 1, until one value remains
    (luminance_single_kernel's passes); a single value takes no pass."""
    v = np.asarray(values, np.float32).ravel()
    while v.size != 1:
        groups = -(-v.size // 128)
        pad = np.zeros(groups * 128, np.float32)
        pad[:v.size] = v
        v = tree(pad.reshape(groups, 128), 128)
    return v[0]


def noise(film, half, threshold):
    """(stats dict without `images`, per-pixel map, tile map), as dcrt_tracer_noise_device gives them."""
    threshold = F(threshold)
    e, valid = pixel_error(film, half)
    with np.errstate(all="ignore"):
        converged = valid & (e <= threshold)
        tile_sum = tree(tiles_of(e, F(0)), TILE * TILE)
        tile_valid = tiles_of(valid, False).sum(-1).astype(np.uint32)
        tile_conv = tiles_of(converged, False).sum(-1).astype(np.uint32)
        tile_max = np.fmax.reduce(np.fmax(tiles_of(e, F(0)), F(0)), axis=-1)
        tile_err = np.where(tile_valid > 0, tile_sum / np.maximum(tile_valid, 1).astype(np.float32), F(0)).astype(np.float32)
        total = reduce_groups(tile_sum)
        n_valid, n_conv = int(tile_valid.sum()), int(tile_conv.sum())
        mean = total / F(n_valid) if n_valid else F(0)
    stats = {"valid_pixels": n_valid, "converged_pixels": n_conv, "mean_error": F(mean),
             "max_error": F(np.fmax.reduce(np.fmax(tile_max.ravel(), F(0)))),
             "max_tile_error": F(np.fmax.reduce(np.fmax(tile_err.ravel(), F(0))))}
    return stats, e, tile_err


def noise_f64(film, half, threshold):
    """The same formulas in plain float64, flat sums: (stats, per-pixel e)."""
    f, h = np.asarray(film, np.float64), np.asarray(half, np.float64)
    with np.errstate(all="ignore"):
        valid = (f[..., 3] > 0) & (h[..., 3] > 0)
        c, a = f[..., :3] / f[..., 3:4], h[..., :3] / h[..., 3:4]
        e = np.abs(c - a).sum(-1) / (np.sqrt(np.fmax(c.sum(-1), 0.0)) + float(F(1e-4)))
        e = np.where(valid, e, 0.0)
        H, W = e.shape
        ty, tx = -(-H // TILE), -(-W // TILE)
        tile_err = np.zeros((ty, tx))
        for j in range(ty):
            for i in range(tx):
                win = (slice(j * TILE, (j + 1) * TILE), slice(i * TILE, (i + 1) * TILE))
                n = valid[win].sum()
                tile_err[j, i] = e[win].sum() / n if n else 0.0
    n_valid = int(valid.sum())
    stats = {"valid_pixels": n_valid, "converged_pixels": int((valid & (e <= float(F(threshold)))).sum()),
             "mean_error": e.sum() / n_valid if n_valid else 0.0,
             "max_error": float(np.fmax.reduce(np.fmax(e.ravel(), 0.0))),
             "max_tile_error": float(np.fmax.reduce(np.fmax(tile_err.ravel(), 0.0)))}
    return stats, e


# ---- oracle films of the Cornell box (shared by the CPU and the GPU tests: rendered once) ----------
_images = {}


def cornell_images(oracle_mod, luts, W, H, bounces, seeds):
    """[(sample positions, sample values)] of the oracle's images of these frame seeds."""
    from conftest import cornell
    key = (W, H, bounces)
    if key not in _images:
        s = cornell(W, H, bounces)
        _images[key] = (s, oracle_mod.flat_with_own_bvh(s), {})
    s, flat, done = _images[key]
    for seed in seeds:
        if seed not in done:
            p, v, _, _ = oracle_mod.render(flat, luts, oracle_mod.frame_params(s, seed), oracle_mod.WAVEFRONT)
            done[seed] = (p, v)
    return [done[seed] for seed in seeds]


def films_of(oracle_mod, filt, images, film=None, half=None, first_index=0):
    """(film, half film) after convolving `images` in order: image k has film image count
    first_index + k and goes into the half film when that is even."""
    H, W = images[0][0].shape[:2]
    film = np.zeros((H, W, 4), np.float32) if film is None else film
    half = np.zeros((H, W, 4), np.float32) if half is None else half
    for k, (pos, val) in enumerate(images):
        oracle_mod.sample_convolution(filt, pos, val, film)
        if (first_index + k) % 2 == 0:
            oracle_mod.sample_convolution(filt, pos, val, half)
    return film, half


def target_met(stats, fraction) -> bool:
    """dcrt_tracer_render_converged's stopping rule (compared in double; the fraction is a float)."""
    return float(stats["converged_pixels"]) >= float(F(fraction)) * float(stats["valid_pixels"])


def stats_equal(got, want) -> bool:
    """The statistics of a GPU call against noise()'s, bit for bit (`images` aside)."""
    return (int(got["valid_pixels"]) == want["valid_pixels"] and int(got["converged_pixels"]) == want["converged_pixels"]
            and all(bool(same_bits(F(got[k]), want[k])) for k in ("mean_error", "max_error", "max_tile_error")))
