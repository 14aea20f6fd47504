"""Adaptive sampling (include/dcrt.h "adaptive sampling") restated in numpy: which 8 x 8 film blocks
stay active for a film and its half film, the sentinel sample that stands in a pixel no path was
started in, and dcrt_tracer_render_adaptive's host loop replayed on the oracle's images. The GPU is
held to these bit for bit (tests/test_gpu_adaptive.py); tests/test_adaptive_ref.py holds them to
plainer models.
"""
import numpy as np

import noise_ref
from noise_ref import F

BLOCK = 8


def block_grid(W, H):
    """(blocksX, blocksY) of a W x H film."""
    return -(-W // BLOCK), -(-H // BLOCK)


def all_blocks(W, H):
    bx, by = block_grid(W, H)
    return np.arange(bx * by, dtype=np.uint32)


def block_pixels(blocks, W, H):
    """The pixels of the listed blocks that lie inside the film: the paths one image starts."""
    bx, _ = block_grid(W, H)
    b = np.asarray(blocks, np.int64)
    return int((np.minimum(BLOCK, W - (b % bx) * BLOCK) * np.minimum(BLOCK, H - (b // bx) * BLOCK)).sum())


def active_blocks(film, half, threshold, margin):
    """(flags blocksY x blocksX uint32, ascending list uint32): block (bx, by) is active when some
    film pixel with bx*8 - margin <= x <= bx*8 + 7 + margin, by*8 - margin <= y <= by*8 + 7 + margin
    is invalid or has !(e <= threshold) -- a NaN e counts -- with e and valid of noise_ref.pixel_error."""
    e, valid = noise_ref.pixel_error(film, half)
    with np.errstate(all="ignore"):
        noisy = ~(valid & (e <= F(threshold)))
    H, W = noisy.shape
    bx, by = block_grid(W, H)
    m = int(margin)
    total = np.zeros((H + 1, W + 1), np.int64)          # total[y, x] = noisy pixels in [0, y) x [0, x)
    total[1:, 1:] = noisy.cumsum(0).cumsum(1)
    x0 = np.maximum(0, np.arange(bx) * BLOCK - m)
    x1 = np.minimum(W - 1, np.arange(bx) * BLOCK + BLOCK - 1 + m) + 1
    y0 = np.maximum(0, np.arange(by) * BLOCK - m)[:, None]
    y1 = (np.minimum(H - 1, np.arange(by) * BLOCK + BLOCK - 1 + m) + 1)[:, None]
    count = total[y1, x1] - total[y0, x1] - total[y1, x0] + total[y0, x0]
    flags = (count > 0).astype(np.uint32)
    return flags, np.flatnonzero(flags.ravel()).astype(np.uint32)


def inactive_pixels(blocks, W, H):
    """H x W bool: the pixels of the blocks that are not listed."""
    bx, by = block_grid(W, H)
    active = np.zeros(bx * by, bool)
    active[np.asarray(blocks, np.int64)] = True
    return ~np.repeat(np.repeat(active.reshape(by, bx), BLOCK, 0), BLOCK, 1)[:H, :W]


def mask_samples(pos, val, blocks):
    """Copies of one image's sample textures with the sentinel sample -- position (+inf, +inf),
    value 0 -- in the pixels of the blocks that are not listed."""
    H, W = pos.shape[:2]
    off = inactive_pixels(blocks, W, H)
    pos, val = np.array(pos, np.float32), np.array(val, np.float32)
    pos[off] = np.inf
    val[off] = 0.0
    return pos, val


def replay(oracle_mod, filt, images, params, margin):
    """dcrt_tracer_render_adaptive's loop on the oracle's images (images[i]: the sample textures of
    the image with film image count i, frame seed first_seed + i) from an empty film: (film, half
    film, the list after every check point that went on, report dict, last stats, converged)."""
    H, W = images[0][0].shape[:2]
    film, half = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    blocks = all_blocks(W, H)
    lists = []
    report = {"images": 0, "check_points": 0, "pixel_samples": 0, "active_blocks": len(blocks), "total_blocks": len(blocks)}
    n, point, converged = 0, int(params.min_images), False
    while True:
        target = min(point, int(params.max_images))
        if n < target:
            masked = [mask_samples(*images[i], blocks) for i in range(n, target)]
            film, half = noise_ref.films_of(oracle_mod, filt, masked, film, half, first_index=n)
            report["images"] += target - n
            report["pixel_samples"] += (target - n) * block_pixels(blocks, W, H)
            n = target
        stats = noise_ref.noise(film, half, params.threshold)[0]
        report["check_points"] += 1
        if noise_ref.target_met(stats, params.target_fraction):
            converged = True
            break
        if n >= int(params.max_images):
            break
        blocks = active_blocks(film, half, params.threshold, margin)[1]
        lists.append(blocks)
        report["active_blocks"] = len(blocks)
        if len(blocks) == 0:
            converged = True
            break
        point += int(params.check_interval)
    return film, half, lists, report, stats, converged


# ---- synthetic films for the mask tests (shared by the CPU and the GPU tests) ----------------------
MASK_SIZES = [(8, 8), (9, 9), (33, 17)]      # one block; partial edge blocks of one pixel; 5 x 3 blocks
MASK_MARGINS = [0, 1, 4, 40]                 # (40: wider than every film above)


def synthetic_films(W, H, seed):
    """A seeded film and half film that agree to well under the threshold nearly everywhere, with a
    noisy pixel per 150 or so. Returns (film, half, threshold)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 40.0, (H, W, 1))
    hw = w * rng.uniform(0.3, 0.7, (H, W, 1))
    c = rng.uniform(0.5, 4.0, (H, W, 3))
    a = c * (1.0 + rng.uniform(-0.002, 0.002, (H, W, 3)))                    # quiet nearly everywhere
    for _ in range(max(1, W * H // 150)):
        y, x = int(rng.integers(H)), int(rng.integers(W))
        a[y, x] = c[y, x] * rng.uniform(1.5, 2.0)                            # a noisy pixel
    film = np.concatenate([c * w, w], -1).astype(np.float32)
    half = np.concatenate([a * hw, hw], -1).astype(np.float32)
    return film, half, F(0.05)


def mask_cases(W, H):
    """{name: (film, half, threshold)}: the seeded film, with an invalid pixel in the last block,
    with a NaN e in the first, and with the threshold exactly at and just below the largest e."""
    film, half, thr = synthetic_films(W, H, W * 31 + H)
    cases = {"plain": (film, half, thr)}
    f2 = film.copy()
    f2[H - 1, W - 1, 3] = 0.0
    cases["invalid"] = (f2, half, thr)
    f3, h3 = film.copy(), half.copy()
    f3[0, 0, :3] = np.inf                    # inf - inf: a NaN e, valid and not converged
    h3[0, 0, :3] = np.inf
    assert np.isnan(noise_ref.pixel_error(f3, h3)[0][0, 0])
    cases["nan"] = (f3, h3, thr)
    top = noise_ref.pixel_error(film, half)[0].max()
    cases["at the threshold"] = (film, half, top)            # converged everywhere ...
    cases["below the threshold"] = (film, half, np.nextafter(top, F(0)))   # ... and not
    return cases
