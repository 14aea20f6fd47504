"""A float64 reference of power-proportional light selection, written from the definition in include/dcrt.h
("light selection") and not from the kernels: the table of a scene's lights, the two searches, the sampler and
the evaluator under the table, and the exact moments of the direct-light estimator. tests/test_light_table_ref.py
holds it to itself; tests/test_gpu_light_table.py holds the device to it.

Definitions (n = the lights uploaded, e = 1/16)
  * Y(c) = max(0, 0.299 r + 0.587 g + 0.114 b) in float32, products summed left to right, a NaN counting 0.
  * a_t: the world-space area of a lamp triangle as light sampling computes it, in float32 and in its order of
    operations: w = ((v.x m0 + v.y m1) + v.z m2) + m3 per component of the three transformed vertices, c =
    cross(w2 - w0, w1 - w0) with components a.y b.z - a.z b.y, a_t = sqrt((c.x^2 + c.y^2) + c.z^2) * 0.5; counted 0
    below 1e-6 or when not finite. A_l = the float64 sum of a lamp's a_t in ascending order.
  * weights (float64): point 4 pi Y; directional pi R^2 Y; mesh pi Y A; environment 4 pi . pi R^2 Y Ybar, Ybar = 1
    without a cube, else sum(Y omega) / sum(omega) over the texels in index order with omega = (4 / n^2) (1 + sc^2 +
    tc^2)^(-3/2). R is an input: half the diagonal of the scene's bounds (the library reports the one it took).
  * P(l) = (1 - e) w_l / sum(w) + e / n; P(t | l) = a_t / A_l. Stored float32: light_prob, light_cdf [n], tri_base [n],
    tri_prob, tri_cdf [E] in light order; CDFs are float64 sums in ascending order, rounded once, last entry exactly 1.
    A lamp with A = 0 has w = 0 and a CDF of zeros. sum(w) zero or not finite, no lights, or one light that is no lamp:
    no table.
  * sampling: the light is the first l with light_cdf[l] > sel, the triangle the first k with tri_cdf[tri_base[l] + k]
    > triSel, both clamped to the last index; the kinds draw what they draw under uniform selection.
  * density: the kind's own pdf times light_prob[l] for point, directional and environment lights; for a lamp
    (light_prob[l] * tri_prob[tri_base[l] + k]) / a_t * (d^2 / cos), zero where a_t counts 0. The sampler reports it
    for the point it drew and the evaluator for the point it is given: the same function (no doubled sampler pdf).

As in shading_ref.py, discrete decisions are evaluated as float32 does and everything continuous is `dtype`."""
import numpy as np

import shading_ref as R

EPSILON = 1.0 / 16.0
AREA_FLOOR = np.float32(1e-6)
CHI_DRAWS = 200_000          # the draws of the distribution test; test_light_table_ref.py checks the smallest expected count


def luminance(rgb):
    """Y of (..., 3) float32 colours, float32 (fmaxf: a NaN gives 0)."""
    c = np.asarray(rgb, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (c[..., 0] * np.float32(0.299) + c[..., 1] * np.float32(0.587)) + c[..., 2] * np.float32(0.114)
    return np.where(y > 0, y, np.float32(0)).astype(np.float32)


def cube_mean_luminance(cube):
    """Ybar of a cube (6, n, n, 3), or 1 without one: float64 sums over the texels in index order."""
    if cube is None:
        return 1.0
    y = luminance(cube).astype(np.float64)
    n = y.shape[1]
    c = (2.0 * np.arange(n) + 1.0) / n - 1.0
    q = 1.0 + c[None, :] ** 2 + c[:, None] ** 2                       # sc along x, tc along y
    omega = np.broadcast_to((4.0 / (float(n) * float(n))) / (q * np.sqrt(q)), y.shape)
    sum_y = sum_o = 0.0
    for a, b in zip((y * omega).ravel(), omega.ravel()):
        sum_y, sum_o = sum_y + a, sum_o + b
    return sum_y / sum_o


def triangle_areas32(s, tri, instance):
    """a_t of triangles `tri` under instances `instance`, float32, in the sampler's order of operations; 0 where the
    sampler's threshold rejects it."""
    f = np.float32
    P = s["vertices"][s["triangles"][tri]][..., 0:3].astype(f)        # (N, 3 vertices, 3)
    M = s["transforms"][instance].astype(f)                            # (N, 3 columns, 4 rows)
    with np.errstate(invalid="ignore", over="ignore"):
        W = [np.stack([((P[:, k, 0] * M[:, c, 0] + P[:, k, 1] * M[:, c, 1]) + P[:, k, 2] * M[:, c, 2]) + f(1) * M[:, c, 3] for c in range(3)], 1)
             for k in range(3)]
        a, b = W[2] - W[0], W[1] - W[0]
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        area = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(f) * f(0.5)
    return np.where(np.isfinite(area) & (area >= AREA_FLOOR), area, f(0)).astype(f)


def scene_radius(bounds_min, bounds_max):
    """R of a box: half its diagonal."""
    d = np.asarray(bounds_max, np.float64) - np.asarray(bounds_min, np.float64)
    return 0.5 * float(np.sqrt((d * d).sum()))


def _running(values):
    """Float64 sums in ascending order."""
    out, t = np.zeros(len(values)), 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for i, v in enumerate(values):
            t = t + float(v)
            out[i] = t
    return out


class Table:
    """The light table of a scene `s` (shading_ref.from_flat) with the scene radius R: the five stored arrays, their
    float64 originals (light_prob64, tri_prob64), the areas (a_t float32 per entry, A float64 per light), the weights,
    and `active`."""

    def __init__(self, s, radius):
        L = s["lights"]
        self.n = n = len(L)
        self.kind = kind = R.light_kind(L) if n else np.zeros(0, np.int64)
        self.radius = float(radius)
        mesh = kind == R.MESH
        counts = np.where(mesh, L[:, 4].astype(np.int64), 0) if n else np.zeros(0, np.int64)
        self.tri_count = counts
        self.tri_base = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32) if n else np.zeros(0, np.uint32)
        self.entries = E = int(counts.sum())
        self.areas = np.zeros(E, np.float32)
        self.A = np.zeros(n)
        sums = np.zeros(E)
        for l in np.flatnonzero(mesh):
            b, c = int(self.tri_base[l]), int(counts[l])
            tri = int(L[l, 3]) + np.arange(c)
            self.areas[b:b + c] = triangle_areas32(s, tri, np.full(c, int(L[l, 5])))
            sums[b:b + c] = _running(self.areas[b:b + c])
            self.A[l] = sums[b + c - 1] if c else 0.0
        y = luminance(L[:, 0:3].view(np.float32)).astype(np.float64) if n else np.zeros(0)
        ybar = cube_mean_luminance(s["env"])
        Rr = self.radius
        with np.errstate(over="ignore", invalid="ignore"):
            w = np.select([kind == R.POINT, kind == R.DIRECTIONAL, mesh, kind == R.ENVIRONMENT],
                          [4.0 * np.pi * y, np.pi * Rr * Rr * y, np.pi * y * self.A, 4.0 * np.pi * (np.pi * Rr * Rr) * y * ybar], 0.0)
        self.weights = w
        running = _running(w)
        self.total = total = float(running[-1]) if n else 0.0
        self.active = bool(n > 0 and np.isfinite(total) and total > 0 and not (n == 1 and not mesh[0]))
        if not self.active:
            self.light_prob = self.light_cdf = self.tri_prob = self.tri_cdf = None
            return
        self.light_prob64 = (1 - EPSILON) * w / total + EPSILON / n
        cdf = _running(self.light_prob64)
        cdf[-1] = 1.0
        self.light_prob, self.light_cdf = self.light_prob64.astype(np.float32), cdf.astype(np.float32)
        self.tri_prob64, tcdf = np.zeros(E), np.zeros(E)
        for l in np.flatnonzero(mesh):
            b, c = int(self.tri_base[l]), int(counts[l])
            if self.A[l] > 0:
                self.tri_prob64[b:b + c] = self.areas[b:b + c].astype(np.float64) / self.A[l]
                tcdf[b:b + c] = sums[b:b + c] / self.A[l]
                tcdf[b + c - 1] = 1.0
        self.tri_prob, self.tri_cdf = self.tri_prob64.astype(np.float32), tcdf.astype(np.float32)


def first_above(cdf, x):
    """Per element of x the first index i with cdf[i] > x (float32 against float32), clamped to the last index."""
    return np.minimum(np.searchsorted(np.asarray(cdf, np.float32), np.asarray(x, np.float32), side="right"), len(cdf) - 1).astype(np.int64)


def select(table, sel, tri_sel):
    """(light, triangle within the light or -1) of float32 numbers sel and tri_sel against the stored CDFs of `table`
    (a Table, or any object with light_cdf, tri_cdf, tri_base, tri_count -- the device's arrays read back)."""
    li = first_above(table.light_cdf, sel)
    k = np.full(len(li), -1, np.int64)
    for l in np.unique(li):
        c = int(table.tri_count[l])
        if c:
            m = li == l
            b = int(table.tri_base[l])
            k[m] = first_above(table.tri_cdf[b:b + c], np.asarray(tri_sel, np.float32)[m])
    return li, k


def mesh_factor(table, li, k, dtype=np.float64):
    """P(l) P(t | l) / a_t per element from the stored float32 arrays, in the definition's order; 0 where a_t counts 0."""
    e = table.tri_base[li].astype(np.int64) + k
    a = table.areas[e].astype(dtype)
    sel = table.light_prob[li].astype(dtype) * table.tri_prob[e].astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(a > 0, sel / a, 0)


def sample_light(s, table, p, states, dtype=np.float64):
    """shading_ref.sample_light under the table: the same dict, with `light`, `triangle` and `pick` (the triangle's index
    within its lamp) chosen by the two searches and `pdf` the table's density."""
    N = len(p)
    p = np.asarray(p, np.float32).astype(dtype)
    u, _ = R.draws(states, 4)
    li, pick = select(table, u[:, 0], u[:, 1])
    L = s["lights"][li]
    Lf = L.view(np.float32)
    kind = R.light_kind(L)
    state = np.zeros((N, 4), np.uint32)
    for k, c in R.DRAWS.items():
        m = kind == k
        if m.any():
            state[m] = R.draws(np.asarray(states, np.uint32).reshape(-1, 4)[m], c)[1]
    out = {"radiance": np.zeros((N, 3), dtype), "wi": np.zeros((N, 3), dtype), "pdf": np.zeros(N, dtype), "distance": np.zeros(N, dtype),
           "delta": (kind == R.POINT) | (kind == R.DIRECTIONAL), "state": state, "light": li, "kind": kind, "pick": pick,
           "triangle": np.full(N, -1, np.int64), "point": np.full((N, 3), np.nan), "cos": np.full(N, np.nan), "area": np.full(N, np.nan), "draws": u}
    radiance = Lf[:, 0:3].astype(dtype)
    P_l = table.light_prob[li].astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = kind == R.POINT
        if m.any():
            w = Lf[m, 3:6].astype(dtype) - p[m]
            d = R._norm(w)
            out["wi"][m], out["distance"][m] = w / d[:, None], d
            out["radiance"][m] = radiance[m] / (d * d)[:, None]
            out["pdf"][m] = P_l[m]
        m = kind == R.DIRECTIONAL
        if m.any():
            out["wi"][m], out["distance"][m] = -Lf[m, 3:6].astype(dtype), np.inf
            out["radiance"][m] = radiance[m]
            out["pdf"][m] = P_l[m]
        m = kind == R.MESH
        if m.any():
            offset, instance = L[m, 3].astype(np.int64), L[m, 5].astype(np.int64)
            tri = offset + pick[m]
            Pv, W, area, n_q, _ = R.triangle_geometry(s, tri, instance, dtype)
            sq = np.sqrt(u[m, 2].astype(dtype))
            bu, bv = dtype(1) - sq, u[m, 3].astype(dtype) * sq
            x = R.to_world(s["transforms"][instance], R._bary(Pv[:, 0], Pv[:, 1], Pv[:, 2], bu, bv), 1, dtype)
            w = x - p[m]
            d = R._norm(w)
            wi = w / d[:, None]
            cos = -R._dot(wi, n_q)
            pdf = mesh_factor(table, li[m], pick[m], dtype) * (d * d / cos)
            lit = (cos > 0) & (pdf > 0)
            out["wi"][m], out["distance"][m] = wi, d
            out["radiance"][m] = np.where(lit[:, None], radiance[m], 0)
            out["pdf"][m] = np.where(cos > 0, pdf, 0)
            out["triangle"][m], out["point"][m], out["cos"][m], out["area"][m] = tri, x, cos, area
        m = kind == R.ENVIRONMENT
        if m.any():
            z = dtype(1) - dtype(2) * u[m, 1].astype(dtype)
            r = np.sqrt(np.maximum(dtype(0), dtype(1) - z * z))
            phi = dtype(2 * np.pi) * u[m, 2].astype(dtype)
            wi = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)
            out["wi"][m], out["distance"][m] = wi, np.inf
            out["pdf"][m] = dtype(1 / (4 * np.pi)) * P_l[m]
            out["radiance"][m] = radiance[m] * (R.env_lookup(s["env"], wi, dtype, R.cube_face64(wi)) if s["env"] is not None else 1)
    finite = np.isfinite(out["distance"])
    out["distance"] = np.where(finite, out["distance"] * dtype(np.float32(1) - R.SHADOW_EPSILON), out["distance"])
    return out


def evaluate_light(s, table, li, tri, normal, wi, distance, dtype=np.float64):
    """shading_ref.evaluate_light under the table: radiance and pdf of light li seen along wi."""
    li, tri = np.asarray(li, np.int64), np.asarray(tri, np.int64)
    normal, wi, distance = (np.asarray(a, np.float32).astype(dtype) for a in (normal, wi, distance))
    L = s["lights"][li]
    Lf = L.view(np.float32)
    kind = R.light_kind(L)
    N = len(li)
    radiance, pdf = np.zeros((N, 3), dtype), np.zeros(N, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = kind == R.MESH
        if m.any():
            k = tri[m] - L[m, 3].astype(np.int64)
            cos = -R._dot(wi[m], normal[m])
            radiance[m] = np.where((cos > 0)[:, None], Lf[m, 0:3].astype(dtype), 0)
            pdf[m] = mesh_factor(table, li[m], k, dtype) * np.where(cos > 0, distance[m] * distance[m] / cos, 0)
        m = kind == R.ENVIRONMENT
        if m.any():
            radiance[m] = Lf[m, 0:3].astype(dtype) * (R.env_lookup(s["env"], wi[m].astype(np.float32), dtype) if s["env"] is not None else 1)
            pdf[m] = dtype(1 / (4 * np.pi)) * table.light_prob[li[m]].astype(dtype)
    return radiance, pdf


# ---- the direct-light estimator's moments, exactly -------------------------------------------------------
def triangle_quadrature(m=24):
    """Barycentric midpoints (u, v) of the m^2 congruent sub-triangles of a triangle, each of weight 1 / m^2."""
    pts = []
    for i in range(m):
        for j in range(m - i):
            pts.append(((i + 1 / 3) / m, (j + 1 / 3) / m))
            if j < m - i - 1:
                pts.append(((i + 2 / 3) / m, (j + 2 / 3) / m))
    return np.array(pts)


def sphere_quadrature(k=48):
    """Directions of k x 4k cells of equal solid angle (midpoints in z and azimuth), each of weight 4 pi / (4 k^2)."""
    z = 1 - 2 * (np.arange(k) + 0.5) / k
    phi = (np.arange(4 * k) + 0.5) / (4 * k) * 2 * np.pi
    Z, PHI = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1 - Z * Z)
    return np.stack([r * np.cos(PHI), r * np.sin(PHI), Z], -1).reshape(-1, 3)


def direct_moments(s, table, p, normal, quadrature=None, sphere=None):
    """The first and second moment of the one-sample direct-light estimator X = Y(radiance) max(0, n . wi) / pdf at the
    point p with the normal n (no occlusion), by summing over the lights and the lamps' triangles with a quadrature over
    every triangle and over the sphere: E[X^k] = sum over (l, t) of sel(l, t) times the mean over the triangle of X^k,
    with sel and pdf those of the table -- or, for table None, of uniform selection (1 / n, 1 / triangle count) with the
    undoubled density 1 / a_t d^2 / cos the evaluator reports. Returns (mean, second moment, the integral itself)."""
    q = triangle_quadrature() if quadrature is None else quadrature
    sph = sphere_quadrature() if sphere is None else sphere
    L = s["lights"]
    n = len(L)
    kind = R.light_kind(L)
    p, normal = np.asarray(p, np.float64), np.asarray(normal, np.float64)
    lum = np.array([np.float32(0.299), np.float32(0.587), np.float32(0.114)], np.float64)
    m1 = m2 = integral = 0.0
    for l in range(n):
        P_l = float(table.light_prob[l]) if table is not None else 1.0 / n
        rad = L[l, 0:3].view(np.float32).astype(np.float64)
        if kind[l] == R.POINT:
            w = L[l, 3:6].view(np.float32).astype(np.float64) - p
            d = np.linalg.norm(w)
            f = float(rad @ lum) / (d * d) * max(0.0, float(normal @ w) / d)
            m1, m2, integral = m1 + P_l * (f / P_l), m2 + P_l * (f / P_l) ** 2, integral + f
        elif kind[l] == R.DIRECTIONAL:
            f = float(rad @ lum) * max(0.0, float(normal @ -L[l, 3:6].view(np.float32).astype(np.float64)))
            m1, m2, integral = m1 + P_l * (f / P_l), m2 + P_l * (f / P_l) ** 2, integral + f
        elif kind[l] == R.ENVIRONMENT:
            Le = (R.env_lookup(s["env"], sph.astype(np.float32), np.float64) if s["env"] is not None else np.ones((len(sph), 3))) * rad
            f = (Le @ lum) * np.maximum(0.0, sph @ normal)
            pdf = P_l / (4 * np.pi)
            m1 += P_l * float((f / pdf).mean())
            m2 += P_l * float(((f / pdf) ** 2).mean())
            integral += float(f.mean()) * 4 * np.pi
        elif kind[l] == R.MESH:
            offset, count, inst = (int(a) for a in L[l, 3:6])
            for k in range(count):
                _, W, area, n_q, _ = R.triangle_geometry(s, np.array([offset + k]), np.array([inst]), np.float64)
                x = W[0, 0] + q[:, 0:1] * (W[0, 1] - W[0, 0]) + q[:, 1:2] * (W[0, 2] - W[0, 0])
                w = x - p
                d = np.linalg.norm(w, axis=1)
                wi = w / d[:, None]
                cos_l = -(wi @ n_q[0])
                if table is not None:
                    sel = P_l * float(table.tri_prob[int(table.tri_base[l]) + k])
                    a_t = float(table.areas[int(table.tri_base[l]) + k])
                    per_area = sel / a_t if a_t > 0 else 0.0
                else:
                    sel = P_l / count
                    per_area = sel / float(area[0]) if float(area[0]) >= R.DEGENERATE else 0.0
                with np.errstate(divide="ignore", invalid="ignore"):
                    pdf = np.where(cos_l > 0, per_area * d * d / cos_l, 0.0)
                    f = np.where(pdf > 0, float(rad @ lum) * np.maximum(0.0, wi @ normal), 0.0)
                    x1 = np.where(pdf > 0, f / pdf, 0.0)
                m1 += sel * float(x1.mean())
                m2 += sel * float((x1 * x1).mean())
                with np.errstate(divide="ignore", invalid="ignore"):
                    integral += float(np.where(cos_l > 0, f * cos_l / (d * d), 0.0).mean()) * float(area[0])
    return m1, m2, integral


def float64_bounds(flat):
    """The float64 box of every instanced triangle's world-space vertices (ray_truth.instance_triangles names the
    triangles of each instance from the BVH's structure): (min, max)."""
    import ctypes as C

    import ray_truth as RT
    s = R.from_flat(flat)
    nodes = R._array(flat.bvh_nodes, C.c_uint32, (flat.bvh_node_count, 8))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst, prims in RT.instance_triangles(nodes):
        P = s["vertices"][s["triangles"][prims]][..., 0:3].astype(np.float64).reshape(-1, 3)
        W = R.to_world(np.broadcast_to(s["transforms"][inst], (len(P), 3, 4)), P, 1, np.float64)
        lo, hi = np.minimum(lo, W.min(0)), np.maximum(hi, W.max(0))
    return lo, hi


def expected_counts(ref, draws):
    """Per bin -- a light that is no lamp, or a (lamp, triangle) pair -- N P(l) P(t | l) from the float64 reference."""
    out = {}
    for l in range(ref.n):
        c, b = int(ref.tri_count[l]), int(ref.tri_base[l])
        if c == 0:
            out[(l, -1)] = draws * ref.light_prob64[l]
        for k in range(c):
            out[(l, k)] = draws * ref.light_prob64[l] * ref.tri_prob64[b + k]
    return out
