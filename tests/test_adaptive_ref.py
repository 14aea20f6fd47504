"""tests/adaptive_ref.py against plainer models, CPU only: the sentinel sample through the oracle's
sample_convolution against a float64 gather that skips the samples it replaces, active_blocks
against a per-pixel loop, and the replay of render_adaptive at its two extremes."""
from types import SimpleNamespace

import numpy as np
import pytest

import adaptive_ref
import film_ref
import noise_ref
from noise_ref import F

FILM_W, FILM_H = 27, 20


def make_filter(kind, radius, alpha=1.5):
    from directcomputeraytracing_amd import FilterParams
    return FilterParams(int(kind), float(radius), float(alpha), 1 / 3, 1 / 3, 3)


def skipping_gather(filt, pos, val, skip, dtype):
    """film_ref.film_model over the samples that `skip` (H x W bool) does not mark: the skipped
    samples are left out of every sum, never evaluated. Returns (film, magnitude sum)."""
    T = np.dtype(dtype).type
    H, W = pos.shape[:2]
    film = np.zeros((H, W, 4), dtype)
    mag = np.zeros((H, W), np.float64)
    reach = int(min(max(W, H), np.floor(float(filt.radius) + 0.5) + 1))
    for sy in range(H):
        for sx in range(W):
            if skip[sy, sx]:
                continue
            px = T(pos[sy, sx, 0]) + T(sx)
            py = T(pos[sy, sx, 1]) + T(sy)
            y0, y1 = max(0, sy - reach), min(H, sy + reach + 1)
            x0, x1 = max(0, sx - reach), min(W, sx + reach + 1)
            cx = np.arange(x0, x1, dtype=dtype) + T(0.5)
            cy = np.arange(y0, y1, dtype=dtype) + T(0.5)
            w = film_ref.weight_1d(filt, cy - py)[:, None] * film_ref.weight_1d(filt, cx - px)[None, :]
            film[y0:y1, x0:x1, :3] += w[..., None] * val[sy, sx, :3].astype(dtype)
            film[y0:y1, x0:x1, 3] += w
            mag[y0:y1, x0:x1] += np.abs(w.astype(np.float64)) * max(float(np.abs(val[sy, sx, :3]).max()), 1.0)
    return film, mag


# two inactive rectangles of whole blocks on a 4 x 3 block grid (27 x 20: partial last column and row)
INACTIVE = [0, 1, 4, 5, 7, 11]
SENTINEL_CASES = ([(kind, r, 1.5) for kind in range(5) for r in (0.5, 1.3, 2.0, 5.5)]
                  + [(film_ref.GAUSSIAN, r, 0.0) for r in (0.5, 2.0, 5.5)])


@pytest.mark.parametrize("kind,radius,alpha", SENTINEL_CASES)
def test_sentinel_samples_add_nothing(oracle_mod, kind, radius, alpha):
    """sample_convolution over sentinel-masked samples against the float64 gather that skips them:
    within 4 x the float32 gather's own error + 2^-22 of the largest sum |w| |v| (the bound of
    tests/test_film_ref.py), every value finite, no -0, and a preloaded film unchanged bit for bit
    where a pixel's whole window is inactive."""
    rng = np.random.default_rng(int(kind * 100 + radius * 10 + alpha))
    filt = make_filter(kind, radius, alpha)
    pos = np.minimum(rng.uniform(0.0, 1.0, (FILM_H, FILM_W, 2)).astype(np.float32), np.nextafter(F(1), F(0)))
    val = rng.uniform(0.0, 4.0, (FILM_H, FILM_W, 4)).astype(np.float32)
    val[..., 3] = 1.0
    blocks = np.setdiff1d(adaptive_ref.all_blocks(FILM_W, FILM_H), INACTIVE).astype(np.uint32)
    skip = adaptive_ref.inactive_pixels(blocks, FILM_W, FILM_H)
    mpos, mval = adaptive_ref.mask_samples(pos, val, blocks)
    assert np.isinf(mpos[skip]).all() and not mval[skip].any() and np.array_equal(mpos[~skip], pos[~skip])
    got = oracle_mod.sample_convolution(filt, mpos, mval)
    m64, mag = skipping_gather(filt, pos, val, skip, np.float64)
    m32, _ = skipping_gather(filt, pos, val, skip, np.float32)
    assert np.isfinite(got).all()
    assert not (np.signbit(got) & (got == 0)).any()
    scale = mag.max()
    if scale == 0.0:        # (a Gaussian with alpha 0 weighs nothing: every film is exactly zero)
        assert alpha == 0.0 and not got.any() and not m32.any()
    else:
        err, err32 = float(np.abs(got - m64).max() / scale), float(np.abs(m32 - m64).max() / scale)
        print(f"filter {kind} r {radius} alpha {alpha}: oracle {err:.3e} float32 gather {err32:.3e}")
        assert err <= 4 * err32 + 2.0 ** -22
    # pixels whose whole window is inactive: an empty film stays exactly 0, a preloaded one as it was
    reach = int(np.floor(radius + 0.5)) + 1
    alone = np.ones((FILM_H, FILM_W), bool)
    for y, x in np.argwhere(~skip):
        alone[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = False
    if radius <= 2.0:
        assert alone.any()
    assert not got[alone].any()
    preload = rng.uniform(-3.0, 3.0, (FILM_H, FILM_W, 4)).astype(np.float32)
    preload[0, 0] = 0.0
    film = preload.copy()
    oracle_mod.sample_convolution(filt, mpos, mval, film)
    assert np.array_equal(film[alone].view(np.uint32), preload[alone].view(np.uint32))


# ---- active_blocks against a per-pixel loop ------------------------------------------------------
def active_blocks_loop(film, half, threshold, margin):
    H, W = film.shape[:2]
    bx, by = adaptive_ref.block_grid(W, H)
    flags = np.zeros((by, bx), np.uint32)
    thr = F(threshold)
    for y in range(H):
        for x in range(W):
            f, h = film[y, x], half[y, x]
            with np.errstate(all="ignore"):
                if f[3] > 0 and h[3] > 0:
                    c, a = f[:3] / f[3], h[:3] / h[3]
                    d = (abs(c[0] - a[0]) + abs(c[1] - a[1])) + abs(c[2] - a[2])
                    e = d / (np.sqrt(np.fmax((c[0] + c[1]) + c[2], F(0))) + F(1e-4))
                    if e <= thr:
                        continue
            for j in range(by):
                for i in range(bx):
                    if i * 8 - margin <= x <= i * 8 + 7 + margin and j * 8 - margin <= y <= j * 8 + 7 + margin:
                        flags[j, i] = 1
    return flags


@pytest.mark.parametrize("W,H", adaptive_ref.MASK_SIZES)
@pytest.mark.parametrize("margin", adaptive_ref.MASK_MARGINS)
def test_active_blocks_matches_pixel_loop(W, H, margin):
    cases = adaptive_ref.mask_cases(W, H)
    for name, (f, h, t) in cases.items():
        flags, blocks = adaptive_ref.active_blocks(f, h, t, margin)
        want = active_blocks_loop(f, h, t, margin)
        assert np.array_equal(flags, want), name
        assert np.array_equal(blocks, np.flatnonzero(want.ravel())) and blocks.dtype == np.uint32, name
    assert not adaptive_ref.active_blocks(*cases["at the threshold"], margin)[0].any()
    assert adaptive_ref.active_blocks(*cases["below the threshold"], margin)[0].any()
    assert adaptive_ref.active_blocks(*cases["invalid"], margin)[0][-1, -1] == 1
    assert adaptive_ref.active_blocks(*cases["nan"], margin)[0][0, 0] == 1
    if margin >= max(W, H):
        assert adaptive_ref.active_blocks(*cases["plain"], margin)[0].all()


def test_block_pixels_and_mask():
    W, H = 33, 17
    assert adaptive_ref.block_grid(W, H) == (5, 3)
    assert adaptive_ref.block_pixels(adaptive_ref.all_blocks(W, H), W, H) == W * H
    assert adaptive_ref.block_pixels([14], W, H) == 1 and adaptive_ref.block_pixels([0, 4, 10], W, H) == 64 + 8 + 8
    off = adaptive_ref.inactive_pixels([14], W, H)
    assert off.sum() == W * H - 1 and not off[16, 32]


# ---- replay extremes -------------------------------------------------------------------------------
def test_replay_extremes(oracle_mod, golden_luts):
    """Threshold 0: nothing ever converges, every block stays listed and the film is films_of's bit
    for bit. A huge threshold: the target is met at the first check point."""
    from conftest import cornell
    W, H, bounces = 33, 17, 2
    filt = cornell(W, H, bounces).filter_params()
    images = noise_ref.cornell_images(oracle_mod, golden_luts, W, H, bounces, range(8))
    total = len(adaptive_ref.all_blocks(W, H))
    params = SimpleNamespace(threshold=0.0, target_fraction=0.5, min_images=2, max_images=8, check_interval=3)
    film, half, lists, report, stats, converged = adaptive_ref.replay(oracle_mod, filt, images, params, 1)
    want = noise_ref.films_of(oracle_mod, filt, images)
    assert np.array_equal(film.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(half.view(np.uint32), want[1].view(np.uint32))
    assert not converged and all(len(b) == total for b in lists) and len(lists) == 2
    assert report == {"images": 8, "check_points": 3, "pixel_samples": 8 * W * H, "active_blocks": total, "total_blocks": total}
    params.threshold = 1e30
    film, half, lists, report, stats, converged = adaptive_ref.replay(oracle_mod, filt, images, params, 1)
    want = noise_ref.films_of(oracle_mod, filt, images[:2])
    assert converged and lists == [] and report["images"] == 2 and report["check_points"] == 1
    assert np.array_equal(film.view(np.uint32), want[0].view(np.uint32))
