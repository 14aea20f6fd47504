"""tests/roulette_ref.py held to itself on the CPU: the float32 restatement against the same rule in float64,
its expectation over the draw (mean_u(scaled * survive) = T: the estimator's mean is untouched), the totality
of q, and the defaults dcrt_roulette_default_params hands out.

Tolerances. q is a maximum and two clamps of float32 values: exact in either precision, so equal. T / q in
float32 is the correctly rounded quotient: within 2^-24 relative of the float64 quotient. Over the grid
u = k / N, k < N, the survivors are the k < q N, ceil(q N) of them: the mean is T / q * ceil(q N) / N, which is
T within 1 / (q N) relative (+ 2^-23 for the division and the product), and within 2^-23 alone where q N is a
whole number."""
import ctypes as C

import numpy as np

import roulette_ref as RR

F = np.float32
SETTINGS = [(0.05, 1.0), (0.1, 0.95), (0.5, 0.5), (1.0, 1.0), (0.25, 0.25)]


def _random_rows(rng, n):
    T = (rng.random((n, 3)) ** 3 * 1.6).astype(F)       # mostly small, some above 1
    T[rng.random(n) < 0.1] *= F(0.01)
    return T, rng.random(n).astype(F)


def _float64_rule(T, u, lo, hi):
    T, u = T.astype(np.float64), u.astype(np.float64)
    lo, hi = float(F(lo)), float(F(hi))
    q = np.minimum(np.maximum(T.max(1), lo), hi)
    drawn = q < 1
    survive = ~drawn | (u < q)
    scaled = np.where((drawn & survive)[:, None], T / q[:, None], T)
    return q, survive, scaled


def test_restatement_is_the_float64_rule():
    rng = np.random.default_rng(11)
    T, u = _random_rows(rng, 20000)
    for lo, hi in SETTINGS:
        q, survive, scaled = RR.roulette(T, u, lo, hi)
        q64, survive64, scaled64 = _float64_rule(T, u, lo, hi)
        assert q.dtype == F and scaled.dtype == F
        assert (q.astype(np.float64) == q64).all()
        assert (survive == survive64).all()
        assert (np.abs(scaled.astype(np.float64) - scaled64) <= 2.0 ** -24 * np.abs(scaled64)).all()
        assert (q >= F(lo)).all() and (q <= F(hi)).all()
        both = survive.mean()
        assert (lo == hi == 1.0 and both == 1.0) or 0.0 < both < 1.0


def test_q_is_total_and_edges_fall_where_the_header_says():
    for lo, hi in SETTINGS:
        T, u = RR.edge_rows(lo, hi)
        q, survive, scaled = RR.roulette(T, u, lo, hi)
        assert np.isfinite(q).all() and (q >= F(lo)).all() and (q <= F(hi)).all()
        assert ((u < q) | (q >= 1) == survive).all()
        untouched = (q >= 1) | ~survive
        assert (scaled.view(np.uint32)[untouched] == T.view(np.uint32)[untouched]).all()
    lo, hi = F(0.05), F(0.9)
    nan, inf = F(np.nan), F(np.inf)
    q = RR.survival(np.array([(nan, nan, nan), (nan, 0.3, nan), (inf, 0, 0), (-inf, -1, nan), (0, 0, 0), (nan, inf, 0.2)], F), lo, hi)
    assert q.tolist() == [lo, F(0.3), hi, lo, lo, hi]
    # u just below q survives, u at q does not
    one = np.array([(0.4, 0.1, 0.2)], F)
    assert RR.roulette(one, np.nextafter(F(0.4), F(0)), lo, hi)[1][0]
    assert not RR.roulette(one, F(0.4), lo, hi)[1][0]
    # q >= 1: no draw decides anything
    assert RR.roulette(np.array([(1.0, 0.2, 0.3), (7.0, 0, 0)], F), np.array([0.999, 0.999], F), 0.05, 1.0)[1].all()


def test_expectation_over_the_draw_is_the_throughput():
    N = 1 << 16
    u = (np.arange(N, dtype=np.float64) / N).astype(F)            # (k / 2^16: exact in float32)
    rng = np.random.default_rng(12)
    T, _ = _random_rows(rng, 48)
    T = np.abs(T) + F(1e-3)
    # rows whose q N is whole: the largest component a multiple of 1 / 256 inside [min, max]
    whole = T.copy()
    whole[:, 0] = (rng.integers(32, 240, len(T)) / 256.0).astype(F)
    whole[:, 1:] *= F(0.1)
    for lo, hi in SETTINGS:
        for rows, exact in ((T, False), (whole, True)):
            q = RR.survival(rows, lo, hi).astype(np.float64)
            if exact:
                keep = (q * N == np.floor(q * N)) & (rows.max(1) >= F(lo)) & (rows.max(1) <= F(hi))
                rows, q = rows[keep], q[keep]
                assert len(rows) > 8 or lo == hi
            for t, qq in zip(rows, q):
                _, survive, scaled = RR.roulette(np.broadcast_to(t, (N, 3)), u, lo, hi)
                mean = (scaled.astype(np.float64) * survive[:, None]).mean(0)
                tol = 2.0 ** -23 + (0.0 if exact or qq >= 1 else 1.0 / (qq * N))
                assert (np.abs(mean - t.astype(np.float64)) <= tol * t.astype(np.float64)).all(), (lo, hi, t, qq, mean)


def test_validity_is_the_setters_rule():
    assert RR.valid(0, 0.05, 1.0) and RR.valid(20, 1.0, 1.0) and RR.valid(2, 1e-30, 1e-30)
    for start, lo, hi in [(21, 0.05, 1.0), (0, 0.0, 1.0), (0, -0.1, 1.0), (0, 0.6, 0.5), (0, 0.5, 1.5), (0, np.nan, 1.0), (0, 0.5, np.nan),
                          (0, np.inf, np.inf), (0, 0.5, np.inf)]:
        assert not RR.valid(start, lo, hi), (start, lo, hi)


def test_defaults_come_from_the_library(native_lib):
    from directcomputeraytracing_amd import _abi
    from directcomputeraytracing_amd.tracer import roulette_defaults
    p = roulette_defaults()
    assert (p.enable, p.start_bounce) == (0, 2)
    assert F(p.min_survival) == F(0.05) and F(p.max_survival) == F(1.0)
    assert RR.valid(p.start_bounce, p.min_survival, p.max_survival)
    assert C.sizeof(_abi.RouletteParams) == 16
    assert native_lib.dcrt_roulette_default_params(None) == -1        # DCRT_E_INVALID_ARG
