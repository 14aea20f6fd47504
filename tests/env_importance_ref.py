"""A float64 reference of environment importance sampling, written from the definition in include/dcrt.h
("environment importance sampling") and not from the kernels: the table of a cube, the density of a direction
and the sampler. tests/test_env_importance_ref.py holds it to itself (the density integrates to 1, the sampler
follows it, its estimates agree with uniform sampling's); tests/test_gpu_env_importance.py holds the device to it.

Definitions (n = the cube's size, faces and signs as shading_ref.env_lookup has them)
  * texel (f, y, x): face coordinates sc = (2x + 1) / n - 1, tc = (2y + 1) / n - 1.
  * Y = max(0, 0.299 r + 0.587 g + 0.114 b) in float32, products summed left to right, a NaN counting 0;
    M = the largest Y over the texel's 3 x 3 neighbourhood clamped inside the face;
    w = M (4 / n^2) (1 + sc^2 + tc^2)^(-3/2) in float64.
  * P = w / sum(w), rows r = f n + y; the row CDFs and the marginal CDF over rows are float64 sums in ascending
    index order, normalised, stored as float32 with the last entry exactly 1; an empty row's CDF is zeros.
    sum(w) zero or not finite: no table.
  * pdf(wi) = (1 - e) P(texel(wi)) (n^2 / 4) (1 + sc^2 + tc^2)^(3/2) + e / (4 pi), e = 1/16, at the face
    coordinates (sc, tc) of wi; texel(wi) = the face, clamp(floor(u n)), clamp(floor(v n)) of the lookup's u, v.
  * the sampler: a < e -> the uniform sphere's direction of (a / e, b); else a' = (a - e) / (1 - e), the first
    row with marginal > a', the first column with cdf > b, the remainders inside the texel, the inverse face map.

As in shading_ref.py, discrete decisions -- the face and the texel of a float32 direction, the row and the column
of float32 numbers against the stored float32 CDFs -- are evaluated as float32 does; everything continuous is
`dtype` (np.float64 the reference, np.float32 the same formulas in single precision)."""
import numpy as np

import shading_ref as R

EPSILON = 1.0 / 16.0
BELOW_ONE = np.float32(1) - np.float32(2.0 ** -24)


def luminance(cube):
    """Y per texel, float32 (fmaxf: a NaN gives 0)."""
    c = np.asarray(cube, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (c[..., 0] * np.float32(0.299) + c[..., 1] * np.float32(0.587)) + c[..., 2] * np.float32(0.114)
    return np.where(y > 0, y, np.float32(0)).astype(np.float32)


def texel_weights(cube):
    """w (6, n, n) float64."""
    y = luminance(cube)
    n = y.shape[1]
    p = np.pad(y, ((0, 0), (1, 1), (1, 1)), mode="edge")
    m = np.zeros_like(y)
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, p[:, dy:dy + n, dx:dx + n])
    c = (2.0 * np.arange(n) + 1.0) / n - 1.0
    q = 1.0 + c[None, None, :] ** 2 + c[None, :, None] ** 2          # sc along x, tc along y
    with np.errstate(over="ignore", invalid="ignore"):
        return m.astype(np.float64) * (4.0 / (float(n) * float(n))) / (q * np.sqrt(q))


class Table:
    """The table of a cube: prob, row_cdf (6n, n) and marginal (6n) as stored (float32), and `active`."""

    def __init__(self, cube):
        w = texel_weights(cube)
        self.n = n = w.shape[1]
        rows = w.reshape(6 * n, n)
        sums = np.zeros_like(rows)
        acc = np.zeros(6 * n)
        for x in range(n):                       # ascending order, float64
            with np.errstate(over="ignore", invalid="ignore"):
                acc = acc + rows[:, x]
            sums[:, x] = acc
        row_total = sums[:, -1]
        marg = np.zeros(6 * n)
        t = 0.0
        for r in range(6 * n):
            with np.errstate(over="ignore", invalid="ignore"):
                t = t + row_total[r]
            marg[r] = t
        self.total = t
        self.active = bool(np.isfinite(t) and t > 0)
        if not self.active:
            self.prob = self.row_cdf = self.marginal = None
            return
        self.prob64 = rows / t
        self.prob = self.prob64.astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            cdf = np.where(row_total[:, None] > 0, sums / row_total[:, None], 0.0)
        cdf[row_total > 0, -1] = 1.0
        self.row_cdf = cdf.astype(np.float32)
        m = marg / t
        m[-1] = 1.0
        self.marginal = m.astype(np.float32)


def face_coordinates(d, dtype=np.float64, face=None):
    """(face, sc, tc): the face as float32 comparisons decide it, the face coordinates in dtype."""
    face = R.cube_face(np.asarray(d, np.float32)) if face is None else face
    d = np.asarray(d).astype(dtype)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    sc = np.choose(face, [-z, z, x, x, x, -x])
    tc = np.choose(face, [-y, -y, z, -z, -y, -y])
    ma = np.abs(np.choose(face, [x, x, y, y, z, z]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return face, sc / ma, tc / ma


def texel_of(d, n):
    """(face, iy, ix) of float32 directions, as float32 evaluates u n and v n."""
    face, fs, ft = face_coordinates(d, np.float32)
    one, half = np.float32(1), np.float32(0.5)
    with np.errstate(invalid="ignore"):
        ix = np.clip(np.floor(np.nan_to_num((fs + one) * half * np.float32(n))), 0, n - 1).astype(np.int64)
        iy = np.clip(np.floor(np.nan_to_num((ft + one) * half * np.float32(n))), 0, n - 1).astype(np.int64)
    return face, iy, ix


def texel_margin(d, n):
    """How near float32 directions are to a jump of the density: the distance of u n and v n from an integer, and the
    relative gap between the two largest components' magnitudes."""
    _, fs, ft = face_coordinates(d, np.float64)
    un, vn = (fs + 1) * 0.5 * n, (ft + 1) * 0.5 * n
    grid = np.minimum(np.abs(un - np.round(un)), np.abs(vn - np.round(vn)))
    # (the cube's outer edges u n = 0 and n are face boundaries, which the second measure covers)
    gap, _ = R.face_margin(np.asarray(d, np.float32))
    return grid, gap


def env_pdf(table, d, dtype=np.float64):
    """The density of directions d (float32 inputs), per solid angle."""
    n = table.n
    face, iy, ix = texel_of(d, n)
    _, fs, ft = face_coordinates(np.asarray(d, np.float32), dtype, face)
    p = table.prob[face * n + iy, ix].astype(dtype)
    q = dtype(1) + fs * fs + ft * ft
    e = dtype(EPSILON)
    return (dtype(1) - e) * p * (dtype(n) * dtype(n) * dtype(0.25)) * (q * np.sqrt(q)) + e * dtype(1 / (4 * np.pi))


def _first_above(cdf, x):
    """Per element the first index i with cdf[..., i] > x (cdf (N, K) or (K,), float32 compared with float32)."""
    c = np.asarray(cdf, np.float32)
    x = np.asarray(x, np.float32)
    if c.ndim == 1:
        return np.minimum(np.searchsorted(c, x, side="right"), len(c) - 1)
    return np.minimum((c <= x[:, None]).sum(1), c.shape[1] - 1)


def uniform_sphere(s0, s1, dtype=np.float64):
    z = dtype(1) - dtype(2) * s0.astype(dtype)
    r = np.sqrt(np.maximum(dtype(0), dtype(1) - z * z))
    phi = dtype(2 * np.pi) * s1.astype(dtype)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def sample_direction(table, a, b, dtype=np.float64):
    """Directions (N, 3) in dtype from float32 numbers a, b in [0, 1), and per element the texel chosen (row, column; -1 for
    the uniform share)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n = table.n
    e32 = np.float32(EPSILON)
    uni = a < e32
    out = uniform_sphere(a / e32, b, dtype)
    a1 = (a - e32) / (np.float32(1) - e32)                 # (float32: it selects the row)
    r = _first_above(table.marginal, a1)
    c = _first_above(table.row_cdf[r], b)
    m_lo = np.where(r > 0, table.marginal[np.maximum(r - 1, 0)], np.float32(0)).astype(dtype)
    m_hi = table.marginal[r].astype(dtype)
    c_lo = np.where(c > 0, table.row_cdf[r, np.maximum(c - 1, 0)], np.float32(0)).astype(dtype)
    c_hi = table.row_cdf[r, c].astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        fa = np.minimum(np.maximum(np.nan_to_num((a1.astype(dtype) - m_lo) / (m_hi - m_lo)), 0), dtype(BELOW_ONE))
        fb = np.minimum(np.maximum(np.nan_to_num((b.astype(dtype) - c_lo) / (c_hi - c_lo)), 0), dtype(BELOW_ONE))
    face, y = r // n, r % n
    sc = dtype(2) * (c.astype(dtype) + fb) / dtype(n) - dtype(1)
    tc = dtype(2) * (y.astype(dtype) + fa) / dtype(n) - dtype(1)
    one = np.ones_like(sc)
    d = np.stack([np.choose(face, [one, -one, sc, sc, sc, -sc]),
                  np.choose(face, [-tc, -tc, one, -one, -tc, -tc]),
                  np.choose(face, [-sc, sc, tc, -tc, one, -one])], -1)
    d = d / np.sqrt((d * d).sum(-1))[:, None]
    out = np.where(uni[:, None], out, d)
    return out, np.where(uni, -1, r), np.where(uni, -1, c)


def texel_solid_angles(n):
    """The exact solid angle of every texel of a face, (n, n) [y, x]: omega = A(x1, y1) - A(x0, y1) - A(x1, y0) + A(x0, y0)
    with A(x, y) = atan2(x y, sqrt(x^2 + y^2 + 1)) (the solid angle of a rectangle seen from unit distance)."""
    g = 2.0 * np.arange(n + 1) / n - 1.0
    X, Y = np.meshgrid(g, g, indexing="xy")
    A = np.arctan2(X * Y, np.sqrt(X * X + Y * Y + 1.0))
    return A[1:, 1:] - A[:-1, 1:] - A[1:, :-1] + A[:-1, :-1]


def expected_counts(table, draws):
    """Expected draws per texel (6n, n): N [(1 - e) P + e omega / (4 pi)]."""
    n = table.n
    omega = np.tile(texel_solid_angles(n), (6, 1))
    return draws * ((1 - EPSILON) * table.prob.astype(np.float64) + EPSILON * omega / (4 * np.pi))


def texel_counts(d, n):
    face, iy, ix = texel_of(np.asarray(d, np.float32), n)
    return np.bincount((face * n + iy) * n + ix, minlength=6 * n * n).reshape(6 * n, n)


def chi_square(counts, expected):
    """(chi^2, degrees of freedom) over the bins with a positive expectation; a draw in a bin of expectation 0 is inf."""
    counts, expected = counts.ravel().astype(np.float64), expected.ravel()
    m = expected > 0
    if counts[~m].sum() > 0:
        return np.inf, int(m.sum()) - 1
    return float(((counts[m] - expected[m]) ** 2 / expected[m]).sum()), int(m.sum()) - 1


# ---- the cubes of the tests ---------------------------------------------------------------------------
def cubes():
    """name -> cube (6, n, n, 3) float32: the eight cubes of the issue's table, built from scenes.env_cube(n)."""
    from directcomputeraytracing_amd import scenes
    out = {f"n{n}": scenes.env_cube(n) for n in (1, 2, 65, 96)}
    hot5 = scenes.env_cube(5)
    hot5[2, 1, 4] = 1e6
    sun8 = scenes.env_cube(8)
    sun8[2, 2, 7] = 5000.0
    zero = np.zeros_like(scenes.env_cube(4))
    inf4 = scenes.env_cube(4)
    inf4[3, 1, 2, 1] = np.inf
    out.update({"n5_hot": hot5, "n8_sun": sun8, "n4_zero": zero, "n4_inf": inf4})
    return out


ACTIVE_CUBES = ["n1", "n2", "n5_hot", "n8_sun", "n65", "n96"]
INACTIVE_CUBES = ["n4_zero", "n4_inf"]


def hemisphere_irradiance(cube, step_count):
    """E = the integral of L cos over the upper hemisphere (normal +y), rgb, by a midpoint rule over (cos theta, phi) with
    step_count x 4 step_count cells of equal solid angle."""
    k = step_count
    mu = (np.arange(k) + 0.5) / k
    phi = (np.arange(4 * k) + 0.5) / (4 * k) * 2 * np.pi
    MU, PHI = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1 - MU * MU)
    d = np.stack([s * np.cos(PHI), MU, s * np.sin(PHI)], -1).reshape(-1, 3)
    L = R.env_lookup(cube, d.astype(np.float32), np.float64)
    return (L * d[:, 1:2]).sum(0) * (2 * np.pi / (4 * k * k))
