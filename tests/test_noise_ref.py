"""tests/noise_ref.py (the float32 restatement of dcrt.h's film noise estimate, which the GPU
kernels must match bit for bit) pinned by itself: against a plain float64 model of the same
formulas on seeded random films, on the special cases, and -- as a check that the estimator is a
usable stopping statistic -- on oracle films of the Cornell box. CPU only."""
import numpy as np
import pytest

import noise_ref
from noise_ref import F

EPS = 2.0 ** -24


def random_films(rng, W, H, gap=0.1):
    """A film and a half film whose colours differ by at least `gap` of the larger one per channel
    (so |c - a| loses at most a factor 1 / gap of relative precision), positive weights."""
    w = rng.uniform(0.5, 40.0, (H, W, 1))
    hw = w * rng.uniform(0.3, 0.7, (H, W, 1))
    c = rng.uniform(0.05, 4.0, (H, W, 3))
    a = c * np.where(rng.random((H, W, 3)) < 0.5, rng.uniform(0.5, 1.0 - gap, (H, W, 3)), rng.uniform(1.0 + gap, 1.6, (H, W, 3)))
    film = np.concatenate([c * w, w], -1).astype(np.float32)
    half = np.concatenate([a * hw, hw], -1).astype(np.float32)
    return film, half


def off_threshold(e64, valid, want):
    """A float32 threshold near `want` that no valid pixel's e comes within 1e-4 relative of."""
    t = F(want)
    for _ in range(1000):
        if not (np.abs(e64[valid] - float(t)) <= 1e-4 * float(t)).any():
            return t
        t = F(float(t) * 1.001)
    raise AssertionError("no threshold off every pixel")


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (16, 16), (17, 16), (33, 17), (130, 70), (300, 200)])
def test_restatement_against_float64(W, H):
    """Counts equal; every e, the maxima and the tile errors within 64 * 2^-24 relative: c and a
    carry one rounding each and their difference amplifies that by at most 1 / gap = 10 (<= 20 *
    2^-24 per channel), the three-term sums, the square root, the + 1e-4 and the quotient add <= 8
    more, the tile mean its sum's bound; the mean within (ceil(log2(pixels)) + 2) * 2^-24 of the
    float64 mean of the same float32 e (pairwise sums of non-negative terms)."""
    rng = np.random.default_rng(W * 1000 + H)
    film, half = random_films(rng, W, H)
    s64, e64 = noise_ref.noise_f64(film, half, 1.0)
    valid = np.ones((H, W), bool)
    thr = off_threshold(e64, valid, np.median(e64))
    s64, e64 = noise_ref.noise_f64(film, half, thr)
    s32, e32, tile32 = noise_ref.noise(film, half, thr)
    assert e32.dtype == np.float32 and tile32.dtype == np.float32 and tile32.shape == (-(-H // 16), -(-W // 16))
    assert s32["valid_pixels"] == s64["valid_pixels"] == W * H
    assert s32["converged_pixels"] == s64["converged_pixels"]
    assert 0 < s32["converged_pixels"] < W * H or W * H == 1
    assert np.abs(e32 - e64).max() <= 64 * EPS * e64.max()
    assert np.all(np.abs(e32 - e64) <= 64 * EPS * e64)
    assert s32["max_error"] == e32.max()                       # the maximum of its own map, exactly
    assert np.unravel_index(e32.argmax(), e32.shape) == np.unravel_index(e64.argmax(), e64.shape)
    assert abs(float(s32["max_error"]) - s64["max_error"]) <= 64 * EPS * s64["max_error"]
    assert s32["max_tile_error"] == tile32.max()
    bound = 64 * EPS + (8 + 2) * EPS
    assert abs(float(s32["max_tile_error"]) - s64["max_tile_error"]) <= bound * s64["max_tile_error"]
    mean64 = e32.astype(np.float64).sum() / (W * H)
    assert abs(float(s32["mean_error"]) - mean64) <= (int(np.ceil(np.log2(W * H))) + 2) * EPS * mean64


def test_reduction_order():
    """The trees are the header's: t + k pairs from k = width / 2 down, groups of 128 zero padded."""
    v = (np.arange(256, dtype=np.float32) * F(1.0000001) + F(1e-3)) ** 2
    acc = v.copy()
    for k in (128, 64, 32, 16, 8, 4, 2, 1):
        for t in range(k):
            acc[t] = F(acc[t] + acc[t + k])
    assert noise_ref.tree(v, 256) == acc[0]
    rng = np.random.default_rng(3)
    sums = rng.uniform(0, 10, 8385).astype(np.float32)          # 129 x 65 tiles: 66 groups, the last of 65 values
    first = np.array([noise_ref.tree(np.concatenate([sums[g * 128:(g + 1) * 128], np.zeros(128, np.float32)])[:128], 128)
                      for g in range(66)], np.float32)
    want = noise_ref.tree(np.concatenate([first, np.zeros(62, np.float32)]), 128)
    assert noise_ref.reduce_groups(sums) == want
    assert noise_ref.reduce_groups(np.array([F(2.5)])) == F(2.5)   # one tile: no pass


def test_special_cases():
    film = np.zeros((5, 7, 4), np.float32)
    half = np.zeros((5, 7, 4), np.float32)
    film[...] = (2.0, 4.0, 6.0, 2.0)       # c = (1, 2, 3)
    half[...] = (1.0, 1.0, 1.0, 1.0)       # a = (1, 1, 1): d = 3, s = 6
    e_plain = F(F(3.0) / F(np.sqrt(F(6.0)) + F(1e-4)))
    film[0, 0, 3] = 0.0                    # weight 0
    half[0, 1, 3] = -1.0                   # a negative weight
    film[0, 2, 3] = np.nan                 # a NaN weight
    film[1, 0] = (-2.0, -4.0, 1.0, 2.0)    # c = (-1, -2, 0.5): a negative colour sum, n = 0
    film[1, 1, 0] = np.inf                 # an inf texel: e = inf / inf
    half[1, 2, 1] = np.nan                 # a NaN texel
    stats, e, tile = noise_ref.noise(film, half, 2.0)
    assert tile.shape == (1, 1)
    assert stats["valid_pixels"] == 35 - 3
    assert (e[0, :3] == 0).all()
    assert e[2, 2] == e_plain
    assert e[1, 0] == F(F(F(2.0) + F(3.0)) + F(0.5)) / F(1e-4)
    assert np.isnan(e[1, 1]) and np.isnan(e[1, 2])
    assert stats["converged_pixels"] == 35 - 3 - 3          # the NaN pixels and the large one are not converged
    assert stats["max_error"] == e[1, 0]                    # fmaxf ignores the NaNs
    assert np.isnan(stats["mean_error"]) and stats["max_tile_error"] == 0 and np.isnan(tile[0, 0])
    # every pixel invalid; a 1 x 1 film
    stats, e, tile = noise_ref.noise(np.zeros((5, 7, 4), np.float32), half, 2.0)
    assert stats == {"valid_pixels": 0, "converged_pixels": 0, "mean_error": 0, "max_error": 0, "max_tile_error": 0}
    assert not e.any() and not tile.any()
    stats, e, tile = noise_ref.noise(film[2:3, 2:3], half[2:3, 2:3], e_plain)
    assert stats["valid_pixels"] == 1 and stats["converged_pixels"] == 1      # e == threshold converges
    assert stats["mean_error"] == stats["max_error"] == stats["max_tile_error"] == tile[0, 0] == e_plain
    below = np.nextafter(e_plain, F(0))
    assert noise_ref.noise(film[2:3, 2:3], half[2:3, 2:3], below)[0]["converged_pixels"] == 0


def test_stopping_rule_in_double():
    assert noise_ref.target_met({"converged_pixels": 3, "valid_pixels": 4}, 0.75)
    assert not noise_ref.target_met({"converged_pixels": 2, "valid_pixels": 4}, 0.75)
    # the fraction is a float32: 0.95f = 0.949999988079071
    assert noise_ref.target_met({"converged_pixels": 19, "valid_pixels": 20}, 0.95)


def test_estimator_on_oracle_films(oracle_mod, golden_luts):
    """Cornell 64 x 48, 4 bounces, the scene's filter. The estimate falls as 1 / sqrt(images): mean
    e at 64 images / mean e at 16 in [0.40, 0.70] (theory 0.5; measured 0.533), and it tracks the
    measured error: mean e at 64 within [0.5, 1.5] of the same expression against a separate
    768-image film, seeds 1000 .. 1767 (measured 0.709: mean e 0.0367 against 0.0518)."""
    from conftest import cornell
    W, H = 64, 48
    filt = cornell(W, H, 4).filter_params()
    images = noise_ref.cornell_images(oracle_mod, golden_luts, W, H, 4, range(64))
    film16, half16 = noise_ref.films_of(oracle_mod, filt, images[:16])
    film64, half64 = noise_ref.films_of(oracle_mod, filt, images)
    m16 = float(noise_ref.noise(film16, half16, 0.05)[0]["mean_error"])
    s64 = noise_ref.noise(film64, half64, 0.05)[0]
    m64 = float(s64["mean_error"])
    print(f"mean e: 16 images {m16:.4f}, 64 images {m64:.4f}, ratio {m64 / m16:.3f}; "
          f"converged at 64: {s64['converged_pixels'] / s64['valid_pixels']:.3f}")
    assert 0.40 <= m64 / m16 <= 0.70
    truth = np.zeros((H, W, 4), np.float32)
    for pos, val in noise_ref.cornell_images(oracle_mod, golden_luts, W, H, 4, range(1000, 1768)):
        oracle_mod.sample_convolution(filt, pos, val, truth)
    measured = float(noise_ref.noise(film64, truth, 0.05)[0]["mean_error"])
    print(f"mean e at 64 against the 768-image film {measured:.4f}, ratio {m64 / measured:.3f}")
    assert 0.5 <= m64 / measured <= 1.5
