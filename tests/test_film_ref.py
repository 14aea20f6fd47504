"""The oracle's image-space passes (sample_convolution, sum_log_luminance, resolve_image) against
the independent numpy models of tests/film_ref.py, on synthetic inputs. CPU only: the GPU kernels
are held to the oracle bit for bit in tests/test_gpu_film_kernels.py."""
import numpy as np
import pytest

import film_ref

FILM_W, FILM_H = 37, 29
RADIUS_RANGES = ((0.001, 0.5), (0.3, 6.0), (6.0, 16.0))   # the reference UI's limits (ImGui.cpp:215)
EDGE_MARGIN = 1e-3


def _frac_distance(a, b):
    d = np.abs(a - b) % 1.0
    return np.minimum(d, 1.0 - d)


def film_case(case):
    """Seeded case -> (FilterParams, pos, val): the five kinds in rotation, the three radius ranges,
    cases 30.. with signed values. For box and Lanczos no offset lies within EDGE_MARGIN of
    frac(0.5 -/+ r), the offsets that put a sample on a pixel centre's support edge."""
    from directcomputeraytracing_amd import FilterParams
    rng = np.random.default_rng(1000 + case)
    kind = case % 5
    lo, hi = RADIUS_RANGES[(case // 5) % 3]
    filt = FilterParams(kind, float(rng.uniform(lo, hi)), float(rng.uniform(0.5, 3.0)), float(rng.uniform(0, 1)),
                        float(rng.uniform(0, 1)), int(rng.integers(1, 5)))
    pos = rng.uniform(0.0, 1.0, (FILM_H, FILM_W, 2)).astype(np.float32)
    edges = support_edge_offsets(filt)
    if edges:
        for _ in range(100):
            bad = near_support_edge(pos, edges)
            if not bad.any():
                break
            pos[bad] = rng.uniform(0.0, 1.0, int(bad.sum())).astype(np.float32)
    pos = np.minimum(pos, np.nextafter(np.float32(1), np.float32(0)))      # [0, 1) after the float32 rounding
    val = rng.uniform(0.0, 4.0, (FILM_H, FILM_W, 4)).astype(np.float32)
    if case >= 30:
        val = (val - 2.0).astype(np.float32)
    val[..., 3] = 1.0
    return filt, pos, val


def support_edge_offsets(filt):
    if filt.filter not in (film_ref.BOX, film_ref.LANCZOS):
        return ()
    r = float(filt.radius)
    return ((0.5 - r) % 1.0, (0.5 + r) % 1.0)


def near_support_edge(pos, edges):
    p = pos.astype(np.float64)
    return (_frac_distance(p, edges[0]) < EDGE_MARGIN) | (_frac_distance(p, edges[1]) < EDGE_MARGIN)


def film_errors(oracle_mod, filt, pos, val):
    """(oracle's error, float32 model's error) against the float64 model, both relative to the
    case's largest magnitude."""
    m64, mag = film_ref.film_model(filt, pos, val, np.float64)
    m32, _ = film_ref.film_model(filt, pos, val, np.float32)
    got = oracle_mod.sample_convolution(filt, pos, val)
    scale = mag.max()
    if scale == 0.0:        # no sample reaches any pixel centre: every film is exactly zero
        assert not got.any() and not m32.any()
        return 0.0, 0.0
    return float(np.abs(got - m64).max() / scale), float(np.abs(m32 - m64).max() / scale)


@pytest.mark.parametrize("case", range(60))
def test_film_oracle_matches_model(oracle_mod, case):
    """sample_convolution against the textbook-formula model, no pixel excluded. Bound: 4x the
    error of the model's own float32 run (it covers the summation order and the det_* polynomials)
    plus 2^-22. Measured over the 60 cases: oracle / float32-model error ratio 0.82 .. 1.11 (worst:
    case 13, Mitchell r 13.9), errors 3e-8 .. 4e-5 of the largest magnitude; in 5 small-radius box
    cases every film is exact (at most one sample per pixel)."""
    filt, pos, val = film_case(case)
    edges = support_edge_offsets(filt)
    if edges:
        assert not near_support_edge(pos, edges).any()
    assert (pos >= 0).all() and (pos < 1).all()
    err_oracle, err_f32 = film_errors(oracle_mod, filt, pos, val)
    print(f"case {case} filter {filt.filter} r {filt.radius:.4f}: oracle {err_oracle:.3e} float32 model {err_f32:.3e} "
          f"ratio {err_oracle / err_f32 if err_f32 else float('nan'):.3f}")
    assert err_oracle <= 4 * err_f32 + 2.0 ** -22


@pytest.mark.parametrize("radius,offsets", film_ref.SUPPORT_EDGE_CASES)
def test_support_edge_samples_belong_to_the_window(oracle_mod, radius, offsets):
    """Samples exactly on the support edge count: |d| <= r for box, and Lanczos cuts only x > r.
    The offsets are dyadic, so |d| == r holds exactly in float32 and in float64 and nothing else
    comes near an edge; the bound is the one of the random cases."""
    from directcomputeraytracing_amd import FILTER_BOX, FILTER_LANCZOS, FilterParams
    rng = np.random.default_rng(int(radius * 100))
    choices = np.array(list(offsets) + [0.5, 0.125, 0.625], np.float32)
    pos = choices[rng.integers(0, len(choices), (FILM_H, FILM_W, 2))]
    val = rng.uniform(-2.0, 2.0, (FILM_H, FILM_W, 4)).astype(np.float32)
    on_edge = film_ref.pairs_on_support_edge(pos, radius)
    assert on_edge > 100
    for kind, tau in ((FILTER_BOX, 3), (FILTER_LANCZOS, 1), (FILTER_LANCZOS, 3)):
        filt = FilterParams(kind, radius, 1.5, 1 / 3, 1 / 3, tau)
        err_oracle, err_f32 = film_errors(oracle_mod, filt, pos, val)
        print(f"r {radius} filter {kind} tau {tau}: {on_edge} pairs on the edge, oracle {err_oracle:.3e} float32 model {err_f32:.3e}")
        assert err_oracle <= 4 * err_f32 + 2.0 ** -22


def test_lanczos_tau_zero_reads_as_three(oracle_mod):
    """dcrt.h: lanczos_tau 0 is the default 3, in the oracle as in the library."""
    from directcomputeraytracing_amd import FILTER_LANCZOS, FilterParams
    _, pos, val = film_case(4)
    films = [oracle_mod.sample_convolution(FilterParams(FILTER_LANCZOS, 2.3, 1.5, 1 / 3, 1 / 3, tau), pos, val)
             for tau in (0, 3, 2)]
    assert np.isfinite(films[0]).all()
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))
    assert not np.array_equal(films[1], films[2])


def test_scene_set_filter_takes_the_tracers_rule():
    """dcrt_scene_set_filter refuses what a film pass refuses (dcrt.h, dcrt_filter_params): an
    unknown kind, a radius that is NaN, negative, infinite or 2^30 and more; the scene keeps its
    filter, and tau 0 is stored as 3."""
    from conftest import cornell
    from directcomputeraytracing_amd import DCRTError, FILTER_GAUSSIAN, FILTER_LANCZOS
    s = cornell(8, 8, 1)
    s.set_filter(FILTER_GAUSSIAN, 1.25, 2.0)
    for kind, radius, text in ((5, 1.0, "unknown"), (0xFFFFFFFF, 1.0, "unknown"), (0, float("nan"), "NaN"), (0, -0.5, "negative"),
                               (0, float("inf"), "2\\^30"), (0, 2.0 ** 30, "2\\^30"), (4, float("-inf"), "negative")):
        with pytest.raises(DCRTError, match="INVALID_ARG.*" + text):
            s.set_filter(kind, radius)
        f = s.filter_params()
        assert (f.filter, f.radius, f.gaussian_alpha) == (FILTER_GAUSSIAN, 1.25, 2.0)
    s.set_filter(FILTER_LANCZOS, float(np.nextafter(np.float32(2.0 ** 30), np.float32(0))), lanczos_tau=0)
    assert s.filter_params().lanczos_tau == 3


def test_filter_models_hold_their_own_identities():
    """The models' formulas against what defines them, so that a slip here is not mistaken for
    one in the oracle: Mitchell-Netravali is a partition of unity, continuous, zero from 2 on, for
    any B and C; the gaussian and the tent reach zero at the radius; Lanczos is 1 at 0 and zero at
    the integers."""
    from directcomputeraytracing_amd import FilterParams
    x = np.linspace(0.0, 1.0, 101)
    for B, C in ((1 / 3, 1 / 3), (1.0, 0.0), (0.0, 0.5), (0.2, 0.9)):
        total = sum(film_ref.mitchell_netravali(x - k, B, C) for k in range(-2, 4))
        assert np.abs(total - 1.0).max() < 1e-14
        k = film_ref.mitchell_netravali(np.array([1.0 - 1e-12, 1.0, 2.0 - 1e-12, 2.0, 0.0]), B, C)
        assert abs(k[0] - k[1]) < 1e-10 and abs(k[2]) < 1e-10 and k[3] == 0.0 and abs(k[4] - (6 - 2 * B) / 6) < 1e-15
    r = 1.75
    d = np.array([0.0, r, -r, np.nextafter(r, 2 * r), 1.0, 2.0, 0.5])
    for kind in range(5):
        w = film_ref.weight_1d(FilterParams(kind, r, 1.5, 1 / 3, 1 / 3, 2), d)
        assert w[0] > 0 and w[3] == 0.0 and w[1] == w[2]
        assert (w[1] == 1.0) if kind == film_ref.BOX else (abs(w[1]) < 0.2)
    lanczos = film_ref.weight_1d(FilterParams(film_ref.LANCZOS, 3.0, 1.5, 1 / 3, 1 / 3, 2), d)
    assert lanczos[0] == 1.0 and abs(lanczos[4]) < 1e-15 and abs(lanczos[5]) < 1e-15
    assert abs(lanczos[6] - (2 / np.pi) * (np.sin(np.pi / 4) / (np.pi / 4))) < 1e-15


@pytest.mark.parametrize("W,H", film_ref.POSTFX_SIZES, ids=[f"{w}x{h}" for w, h in film_ref.POSTFX_SIZES])
def test_postfx_oracle_matches_model(oracle_mod, W, H):
    """sum_log_luminance within 1e-4 relative and resolve_image within one sRGB8 code of the
    float64 model (the tolerances of test_postfx_matches_float64_model), at the film sizes that take
    one, two and three reduction passes."""
    from directcomputeraytracing_amd import PostFxParams, srgb_thresholds
    film = film_ref.synthetic_film(W, H, 7 * W + H)
    th = srgb_thresholds()
    n = film_ref.partial_sums(W, H)
    if (W, H) in ((256, 128), (2049, 9)):
        assert n == (128 if W == 256 else 129)      # the last one-pass count, the first two-pass count
    else:
        assert n > 16384 if W == 8200 else n < 128
    got = oracle_mod.sum_log_luminance(film)
    params = [PostFxParams(*p) for p in film_ref.POSTFX_PARAMETERS]
    for prm in params[:1] if W * H > 1 << 20 else params:     # (the oracle resolves 4 M pixels in seconds: once)
        codes, total = film_ref.postfx_model(film, prm)
        assert abs(got - total) <= 1e-4 * abs(total), (got, total)
        out = oracle_mod.resolve_image(film, prm, th)
        diff = np.abs(out[..., :3].astype(int) - np.rint(codes))
        assert diff.max() <= 1 and np.all(out[..., 3] == 255), \
            f"{prm.enabled} {prm.auto_exposure} {prm.ev100} {prm.luminance_white}: {diff.max()} codes"
    print(f"{W}x{H}: {n} partial sums, sum relative error {abs(got - total) / abs(total):.2e}")


def test_postfx_model_sees_the_whole_code_range():
    """The synthetic films are not all black or all white (or the one-code bound above would hold
    for any tone curve): under auto exposure where the film fills the reduction's padded domain
    (a ragged film's padding counts as black and drives the exposure up, as in the reference), and
    under manual exposure on a ragged one."""
    from directcomputeraytracing_amd import PostFxParams
    for (W, H), prm in (((256, 128), PostFxParams(1, 1, 0.0, 1.0)), ((33, 19), PostFxParams(1, 0, 0.0, 1.0))):
        codes, _ = film_ref.postfx_model(film_ref.synthetic_film(W, H, 7 * W + H), prm)
        assert codes.min() < 40 and codes.max() > 200 and np.unique(np.rint(codes)).size > 100
