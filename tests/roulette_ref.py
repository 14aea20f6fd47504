"""Russian roulette as include/dcrt.h ("Russian roulette") pins it, restated in numpy float32: the survival
probability of a throughput, and what one draw u does to the path. Shares no code with the kernels;
tests/test_roulette_ref.py holds it to float64 and to its own expectation, tests/test_gpu_roulette.py holds
dcrt_device_roulette to it bit for bit.

    q = fminf(fmaxf(fmaxf(fmaxf(T.x, T.y), T.z), min_survival), max_survival)
    q >= 1: the path goes on with T, no draw; else u < q: it goes on with T / q; else it ends.

np.fmax / np.fmin are C's fmaxf / fminf (a NaN operand is ignored), so q is total: always within [min, max]."""
import numpy as np

F = np.float32


def valid(start_bounce, min_survival, max_survival, max_ray_bounce=20):
    """What dcrt_tracer_set_roulette accepts: 0 < min <= max <= 1 (a NaN fails a comparison), start <= DCRT_MAX_RAY_BOUNCE."""
    lo, hi = F(min_survival), F(max_survival)
    return bool(lo > 0 and lo <= hi and hi <= 1 and 0 <= start_bounce <= max_ray_bounce)


def survival(T, min_survival, max_survival):
    """q [n] float32 of the throughputs T [n, 3]."""
    T = np.asarray(T, F).reshape(-1, 3)
    m = np.fmax(np.fmax(T[:, 0], T[:, 1]), T[:, 2])
    return np.fmin(np.fmax(m, F(min_survival)), F(max_survival)).astype(F)


def roulette(T, u, min_survival, max_survival):
    """(q [n], survive [n] bool, scaled [n, 3]): scaled is T / q where the draw was made and passed, T where no
    draw was made (q >= 1) or the path ends."""
    T = np.asarray(T, F).reshape(-1, 3)
    u = np.asarray(u, F).reshape(-1)
    q = survival(T, min_survival, max_survival)
    drawn = ~(q >= 1)
    survive = ~drawn | (u < q)
    with np.errstate(all="ignore"):
        divided = (T / q[:, None]).astype(F)
    scaled = np.where((drawn & survive)[:, None], divided, T).astype(F)
    return q, survive, scaled


def edge_rows(min_survival, max_survival):
    """(T [n, 3], u [n]) float32: a zero, a negative, a NaN and an infinite component (alone and throughout), the
    largest component exactly at min, at max and at 1 and one step either side, and u one step below q, at q
    and one step above for each of those."""
    lo, hi, one = F(min_survival), F(max_survival), F(1)
    nan, inf = F(np.nan), F(np.inf)
    step = lambda x, to: np.nextafter(F(x), F(to))
    rows = [(0, 0, 0), (0.3, 0, 0.2), (-1, -2, -3), (-1, 0.4, 0.2), (nan, 0.3, 0.2), (0.3, nan, 0.2), (0.3, 0.2, nan),
            (nan, nan, 0.7), (nan, nan, nan), (inf, 0.1, 0.2), (0.1, -inf, 0.2), (inf, inf, inf), (nan, inf, 0.5),
            (1e-30, 1e-38, 1e-45), (3e38, 1, 1)]
    for edge in (lo, hi, one):
        for m in (step(edge, 0), edge, step(edge, 2)):
            rows += [(m, m * F(0.5), 0), (0, m, m), (m * F(0.25), 0, m)]
    T = np.array(rows, F)
    q = survival(T, lo, hi)
    Ts, us = [], []
    for t, qq in zip(T, q):
        for u in (step(qq, 0), qq, step(qq, 2), F(0), step(1, 0)):
            Ts.append(t)
            us.append(min(max(u, F(0)), step(1, 0)))   # (a draw lies in [0, 1))
    return np.array(Ts, F), np.array(us, F)
