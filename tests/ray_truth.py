"""A float64 brute-force ray-cast reference (test infrastructure, numpy only).

It calls no product or oracle intersection code and never reads a BVH box: the triangle list of
every instance comes from the structure of the two-level BVH alone (so a box that is too small
makes the traversal visibly miss a hit this reference finds), and every (instance, triangle) pair
is intersected with a textbook Moller-Trumbore in float64 -- in object space, with the ray taken
through the uploaded inverse matrix (what the kernels are given), and again in world space with
the vertices taken through the forward matrix; the two must agree, which holds the inverse
matrices to the forward ones.

A Float4x3 is three columns of four floats (`mul43`, csrc/device/dscene.h): the matrix that a row
vector (x, y, z, w) multiplies is `xf[i].reshape(3, 4).T`.

Tolerances are not fixed in advance. For every candidate hit the float64 intersection is rerun
with the ray's origin and direction, the triangle's vertices and the inverse matrix's entries
each moved by one float32 ulp (PERTURBATIONS random sign patterns); the largest change of t, times
8 for the roughly ten rounded operations between a ray and its t in either triangle test, plus
4 ulps of t, is that candidate's tolerance on t; u and v likewise (plus 4 ulps of 1).

Every ray is classified as clear or ambiguous (`Analysis.reason`, the R_* bits). Equality with a
float32 cast is only asserted on clear rays; an ambiguous ray must still miss or report a t near
one of the reference's candidates (`compare_hits`).

With the any-hit feature a ray carries an opacity sample and a hit counts only if the sample is below
the hit's opacity (`Opacity`: float64, from the definition, the texel addressing imported from
tests/shading_ref.py). `Truth.analyse(rays, samples)` then keeps every candidate, takes the nearest
accepted one, and derives a tolerance on each candidate's opacity the same way (u, v moved by the
candidate's own tolerance, every float32 input by one ulp, times 8, plus 4 ulps); a candidate whose
sample lies within it of its opacity is undecided, and a ray with an undecided candidate -- or one
ambiguous by the reasons above -- at or before its result is ambiguous (R_OPACITY).

The generators below write the scenes (Mitsuba XML + OBJ, as tests/random_scenes.py does) and the
ray families the ray-truth tests use."""
from pathlib import Path

import numpy as np

EPS32 = 2.0 ** -23
BARY_MARGIN = 1e-3      # barycentric margin below which the nearest hit (or a near miss) is ambiguous
GRAZING_COS = 1e-3      # |cos| between ray and face below which a hit is ambiguous
SLIVER_RATIO = 1e-4     # area / longest edge^2 below which a triangle is a sliver
PERTURBATIONS = 4
PREFILTER_MARGIN = 0.05   # near misses are looked for this far outside a triangle; tol_uv must stay below it
COUNT_MASK = 0x1FFFFFFF

# why a ray is ambiguous for the closest hit (`Analysis.occluded` decides separately, for a given t_max)
R_MARGIN, R_GRAZING, R_GAP, R_NEAR_MISS, R_T_ZERO, R_SLIVER, R_CONDITION, R_OPACITY = 1, 2, 4, 8, 16, 32, 64, 128
REASONS = {R_MARGIN: "margin", R_GRAZING: "grazing", R_GAP: "gap", R_NEAR_MISS: "near-miss", R_T_ZERO: "t~0",
           R_SLIVER: "sliver", R_CONDITION: "ill-conditioned", R_OPACITY: "opacity"}
NO_OVERRIDE = 0xFFFFFFFF
FLAG_OPAQUE = 1


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a * b).sum(-1)


def moller_trumbore(o, d, p0, p1, p2):
    """t, u, v of the line o + t d against the plane of (p0, p1, p2), float64, no acceptance test:
    the hit point is (1 - u - v) p0 + u p1 + v p2. Non-finite where the ray is parallel to the
    plane or the triangle has no area."""
    e1, e2 = p1 - p0, p2 - p0
    pv = _cross(d, e2)
    det = _dot(e1, pv)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / det
        tv = o - p0
        u = _dot(tv, pv) * inv
        qv = _cross(tv, e1)
        v = _dot(d, qv) * inv
        t = _dot(e2, qv) * inv
    return t, u, v


def instance_triangles(nodes):
    """[(instance index, primitive indices)] from the BVH's structure only: a TLAS leaf has
    misc & 4 (instance (misc >> 3) & COUNT_MASK, `right` the absolute BLAS root), a BLAS leaf has a
    count (misc >> 3) & COUNT_MASK > 0 of primitives from `right`, an interior node has the
    children n + 1 and `right`."""
    right, misc = nodes[:, 6].astype(np.int64), nodes[:, 7].astype(np.int64)
    blas = {}

    def prims(root):
        if root not in blas:
            out, stack = [], [root]
            while stack:
                n = stack.pop()
                count = (misc[n] >> 3) & COUNT_MASK
                if count:
                    out.extend(range(right[n], right[n] + count))
                else:
                    stack += [right[n], n + 1]
            blas[root] = np.asarray(out, np.int64)
        return blas[root]

    out, stack = [], [0]
    while stack:
        n = stack.pop()
        if misc[n] & 4:
            out.append((int((misc[n] >> 3) & COUNT_MASK), prims(int(right[n]))))
        else:
            assert (misc[n] >> 3) & COUNT_MASK == 0, "a TLAS node with primitives"
            stack += [right[n], n + 1]
    return sorted(out, key=lambda e: e[0])


def _ulp(x32):
    return np.spacing(np.abs(x32)).astype(np.float64)


class Opacity:
    """The any-hit opacity test of a flat scene (a dcrt_flat_scene), in float64 and from its definition: the
    material of a candidate is its instance's override if it has one, else its triangle's; the value is the
    material's opacity, times the red channel of its opacity texture -- bilinear, wrapped, at tex_tiling x the
    texcoord interpolated at (u, v) -- if it has one; a candidate counts iff sample < value, and always on an
    instance flagged OPAQUE. The texture addressing (texel centres, wrap, R8 / sRGB decode) is
    tests/shading_ref.py's."""

    def __init__(self, flat):
        import ctypes as C
        import shading_ref as S
        s = S.from_flat(flat)
        self.S = S
        self.tc32 = s["vertices"][:, 9:11].astype(np.float32)[s["triangles"]]              # (T, 3, 2)
        self.material_ids = s["material_ids"].astype(np.int64)
        self.overrides = s["overrides"].astype(np.int64)
        self.opaque = (S._array(flat.instance_flags, C.c_uint32, (flat.instance_count,)) & FLAG_OPAQUE) != 0
        m = s["materials"]
        self.tiling32 = m[:, 8:10].copy().view(np.float32)
        self.opacity32 = m[:, 10].copy().view(np.float32)
        self.texture = m[:, 12].copy().view(np.int32).astype(np.int64)
        self.textures = s["textures"]

    def material(self, inst, prim):
        ov = self.overrides[inst]
        return np.where(ov != NO_OVERRIDE, ov, self.material_ids[prim])

    def value(self, mat, u, v, tc, tiling, opacity):
        """The opacity of candidates with material `mat` at (u, v): float64 from the given texcoords (n, 3, 2),
        tilings (n, 2) and material opacities (n)."""
        out = np.asarray(opacity, np.float64).copy()
        w = np.stack([1.0 - u - v, u, v], -1)
        at = np.einsum("nk,nkc->nc", w, tc) * tiling
        for k in np.unique(self.texture[mat]):
            if k < 0:
                continue
            rows = np.flatnonzero(self.texture[mat] == k)
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(at[rows]).all(1)
                red = np.full(len(rows), np.nan)
                red[ok] = self.S.sample_texture(self.textures[k], at[rows][ok], np.float64)[:, 0]
            out[rows] = out[rows] * red
        return out

    def decide(self, rng, inst, prim, u, v, tol_uv, sample):
        """Per candidate: (value, tolerance, accepted, undecided). The tolerance is the largest change of the
        value when u and v move by the candidate's tol_uv and the float32 texcoords, tiling and material opacity
        by one ulp each (PERTURBATIONS sign patterns), times 8, plus 4 float32 ulps of the value."""
        mat = self.material(inst, prim)
        tc, tiling, op = self.tc32[prim], self.tiling32[mat], self.opacity32[mat]
        val = self.value(mat, u, v, tc.astype(np.float64), tiling.astype(np.float64), op.astype(np.float64))
        dv = np.zeros(len(val))
        for _ in range(PERTURBATIONS):
            def move(x32):
                return x32.astype(np.float64) + rng.choice([-1.0, 1.0], x32.shape) * _ulp(x32)
            with np.errstate(invalid="ignore"):
                moved = self.value(mat, u + rng.choice([-1.0, 1.0], u.shape) * tol_uv, v + rng.choice([-1.0, 1.0], v.shape) * tol_uv,
                                   move(tc), move(tiling), move(op))
                dv = np.fmax(dv, np.abs(moved - val))
        with np.errstate(invalid="ignore"):
            tol = 8.0 * dv + 4.0 * _ulp(val.astype(np.float32))
        tol[~np.isfinite(tol) | ~np.isfinite(val)] = np.inf
        s = np.asarray(sample, np.float64)
        opaque = self.opaque[inst]
        with np.errstate(invalid="ignore"):
            accepted = opaque | (s < val)
            undecided = ~opaque & ~(np.abs(s - val) > tol)
        return val, tol, accepted, undecided


class Analysis:
    """What `Truth.analyse` found for a batch of rays. Per ray: hit, t, u, v, inst, prim (the
    nearest hit, object-space intersection), facing (sign of d_obj . (p1 - p0) x (p2 - p0)), cos,
    tol_t, tol_uv and reason (0: clear). Per candidate (a hit, a near miss within BARY_MARGIN, or a
    sliver / zero-area triangle the ray passes close to): c_ray, c_inst, c_prim, c_t, c_u, c_v,
    c_tol_t, c_tol_uv, c_true (a hit in float64). With opacity samples (`Truth.analyse(rays, samples)`:
    every ray carries one into the any-hit test, `Opacity`) also c_opacity, c_tol_opacity, c_accept
    (sample < opacity, or an OPAQUE instance) and c_undecided (|sample - opacity| within the tolerance);
    the nearest hit is then the nearest accepted one, and crossed[ray] says that the ray passes a clearly
    rejected hit before it. Without samples every candidate is accepted and none undecided."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def clear(self):
        return self.reason == 0

    def tie_keys(self):
        """Sorted keys ray * n_pairs + pair of the candidates that tie with the nearest hit."""
        best = self.t[self.c_ray]
        tie = self.c_true & (self.c_accept | self.c_undecided) & (self.c_t - best <= 2.0 * np.maximum(self.c_tol_t, self.tol_t[self.c_ray]))
        return np.sort(self.c_ray[tie] * self.n_keys + self.c_inst[tie] * self.n_prims + self.c_prim[tie])

    def occluded(self, t_max):
        """(occluded, ambiguous) for the rays' t_max: any accepted hit with 0 <= t < t_max. Clear when
        one hit is robust (inside its triangle by BARY_MARGIN, not grazing, not a sliver, further
        than its tolerance from 0 and from t_max, and clearly accepted), or when no candidate that is
        accepted or undecided lies in range."""
        n = len(self.t)
        tm = np.asarray(t_max, np.float64)[self.c_ray]
        occ = np.zeros(n, bool)
        occ[self.c_ray[self.c_true & self.c_accept & (self.c_t >= 0) & (self.c_t < tm)]] = True
        robust = self.c_robust & self.c_accept & ~self.c_undecided & (self.c_t > self.c_tol_t) & (self.c_t < tm - self.c_tol_t)
        sure = np.zeros(n, bool)
        sure[self.c_ray[robust]] = True
        near = (self.c_t > -self.c_tol_t) & (self.c_t - self.c_tol_t < tm) & (self.c_accept | self.c_undecided)
        maybe = np.zeros(n, bool)
        maybe[self.c_ray[near]] = True
        return occ, maybe & ~sure

    def crossed_before(self, t_max):
        """Per ray: a clearly rejected float64 hit lies below t_max (an any-hit ray passes through it)."""
        tm = np.asarray(t_max, np.float64)[self.c_ray]
        out = np.zeros(len(self.t), bool)
        out[self.c_ray[self.c_true & ~self.c_accept & ~self.c_undecided & (self.c_t >= 0) & (self.c_t < tm)]] = True
        return out


class Truth:
    """The float64 reference over one flat scene (`test_scene_pin._flat_arrays`)."""

    def __init__(self, fa, seed=0, opacity=None):
        self.rng = np.random.default_rng(seed)
        self.opacity = opacity                     # an `Opacity` over the same flat scene: `analyse` takes samples
        self.opacity_rng = np.random.default_rng(seed + 1)     # (its own draws: the tolerances on t, u, v are the same with and without samples)
        pos = np.ascontiguousarray(fa["vertices"][:, :3]).view(np.float32)
        tri = fa["triangles"].astype(np.int64)
        xf = np.ascontiguousarray(fa["instance_transforms"]).view(np.float32)
        self.n_inst = len(xf) // 2
        per_inst = instance_triangles(fa["bvh_nodes"])
        assert [i for i, _ in per_inst] == list(range(self.n_inst)), "every instance is one TLAS leaf"
        self.inst = np.concatenate([np.full(len(p), i, np.int64) for i, p in per_inst])
        self.prim = np.concatenate([p for _, p in per_inst])
        self.n_prims = len(tri)
        self.xf32 = xf.reshape(2 * self.n_inst, 3, 4).transpose(0, 2, 1).copy()      # (2 n, 4, 3): reshape(3, 4).T
        fwd = self.xf32[:self.n_inst].astype(np.float64)
        self.inv = self.xf32[self.n_inst:].astype(np.float64)
        self.fwd = fwd
        self.p32 = pos[tri[self.prim]]                                               # (M, 3, 3) float32
        self.p_obj = self.p32.astype(np.float64)
        self.p_world = np.einsum("mkj,mjc->mkc", self.p_obj, fwd[self.inst][:, :3]) + fwd[self.inst][:, None, 3]
        thin = np.zeros(len(self.prim), bool)
        for p in (self.p_obj, self.p_world):
            e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], 1)
            longest2 = (e * e).sum(-1).max(1)
            area = 0.5 * np.linalg.norm(_cross(e[:, 0], -e[:, 2]), axis=1)
            thin |= area < SLIVER_RATIO * longest2
        self.thin = thin
        n_obj = _cross(self.p_obj[:, 1] - self.p_obj[:, 0], self.p_obj[:, 2] - self.p_obj[:, 0])
        self.zero_area = (n_obj == 0).all(1)
        self.normal_obj = n_obj
        e = np.stack([self.p_obj[:, 1] - self.p_obj[:, 0], self.p_obj[:, 2] - self.p_obj[:, 1], self.p_obj[:, 0] - self.p_obj[:, 2]], 1)
        k = (e * e).sum(-1).argmax(1)
        m = np.arange(len(k))
        self.seg_a = self.p_obj[m, k]                                                # the longest edge, object space
        self.seg_b = self.p_obj[m, (k + 1) % 3]
        self.box = (self.p_world.reshape(-1, 3).min(0), self.p_world.reshape(-1, 3).max(0))

    # ---- the intersection -------------------------------------------------------------------
    def _object_rays(self, o, d, inv):
        return (np.einsum("rk,rkc->rc", o, inv[:, :3]) + inv[:, 3], np.einsum("rk,rkc->rc", d, inv[:, :3]))

    def _tolerances(self, o32, d32, pair):
        """Per candidate: the change of (t, u, v) under one-ulp moves of every float32 input."""
        o, d = o32.astype(np.float64), d32.astype(np.float64)
        inv32 = self.xf32[self.n_inst + self.inst[pair]]
        p32 = self.p32[pair]
        oo, dd = self._object_rays(o, d, inv32.astype(np.float64))
        t, u, v = moller_trumbore(oo, dd, *(self.p_obj[pair][:, k] for k in range(3)))
        dt = np.zeros(len(pair))
        duv = np.zeros(len(pair))
        for _ in range(PERTURBATIONS):
            def move(x32):
                return x32.astype(np.float64) + self.rng.choice([-1.0, 1.0], x32.shape) * _ulp(x32)
            oo, dd = self._object_rays(move(o32), move(d32), move(inv32))
            p = move(p32)
            t1, u1, v1 = moller_trumbore(oo, dd, p[:, 0], p[:, 1], p[:, 2])
            with np.errstate(invalid="ignore"):
                dt = np.fmax(dt, np.abs(t1 - t))
                duv = np.fmax(duv, np.fmax(np.abs(u1 - u), np.abs(v1 - v)))
        tol_t = 8.0 * dt + 4.0 * _ulp(t.astype(np.float32))
        tol_uv = 8.0 * duv + 4.0 * EPS32
        bad = ~np.isfinite(tol_t) | ~np.isfinite(tol_uv)
        tol_t[bad] = np.inf
        tol_uv[bad] = np.inf
        return tol_t, tol_uv

    def _near_thin(self, oo, dd, a, b):
        """Distance between the ray oo + s dd (s >= 0) and the segment a..b, and s."""
        u, v, w = dd, b - a, oo - a
        A, B, Cc, D, E = _dot(u, u), _dot(u, v), _dot(v, v), _dot(u, w), _dot(v, w)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(A * Cc - B * B > 0, (A * E - B * D) / (A * Cc - B * B), 0.0)
            for _ in range(2):
                q = np.clip(np.nan_to_num(q), 0.0, 1.0)
                s = np.maximum((q * B - D) / A, 0.0)
                q = np.where(Cc > 0, (E + s * B) / Cc, 0.0)
            q = np.clip(np.nan_to_num(q), 0.0, 1.0)
        return np.linalg.norm(w + s[..., None] * u - q[..., None] * v, axis=-1), s

    def analyse(self, rays, samples=None):
        """`samples`: one opacity sample per ray (needs `self.opacity`): the any-hit test decides which
        candidates count; None: every one does."""
        o32 = np.ascontiguousarray(rays["origin"], np.float32)
        d32 = np.ascontiguousarray(rays["direction"], np.float32)
        n, M = len(rays), len(self.prim)
        P = [self.p_obj[:, k] for k in range(3)]
        W = [self.p_world[:, k] for k in range(3)]
        thin_pairs = np.flatnonzero(self.thin)
        solid = ~self.zero_area
        norm_n = np.linalg.norm(self.normal_obj, axis=1)
        best_w = np.full(n, np.inf)
        cr, cm, ct, cu, cv, cthin = [], [], [], [], [], []

        def add(r, m, t, u=None, v=None):
            nan = np.full(len(r), np.nan)
            cr.append(r), cm.append(m), ct.append(t), cu.append(nan if u is None else u), cv.append(nan if v is None else v)
            cthin.append(np.full(len(r), u is None))

        # Every ray against every triangle, in two steps: the distance of the ray's line from the triangle's
        # bounding sphere (world space, float64, every pair), then the intersection for the pairs that
        # pass within 1.25 radii (a near miss by PREFILTER_MARGIN lies well inside that).
        centre = self.p_world.mean(1)
        radius = np.linalg.norm(self.p_world - centre[:, None], axis=-1).max(1)
        reach2 = (1.25 * radius + 1e-6 * (1.0 + np.abs(centre).max(1))) ** 2
        c2 = _dot(centre, centre)
        step = max(1, 4_000_000 // M)
        for lo in range(0, n, step):
            o, d = o32[lo:lo + step].astype(np.float64), d32[lo:lo + step].astype(np.float64)
            dn = d / np.linalg.norm(d, axis=1, keepdims=True)
            along_ray = dn @ centre.T - _dot(o, dn)[:, None]
            dist2 = c2[None] - 2.0 * (o @ centre.T) + _dot(o, o)[:, None] - along_ray ** 2
            r, m = np.nonzero((dist2 <= reach2[None]) & solid[None])
            oo, dd = self._object_rays(o[r], d[r], self.inv[self.inst[m]])
            t, u, v = moller_trumbore(oo, dd, P[0][m], P[1][m], P[2][m])
            with np.errstate(invalid="ignore"):
                margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
                cand = np.isfinite(t) & (margin > -PREFILTER_MARGIN) & (t > -1e-3 * (1.0 + np.abs(oo).max(-1)))
            add(r[cand] + lo, m[cand], t[cand], u[cand], v[cand])
            tw, uw, vw = moller_trumbore(o[r], d[r], W[0][m], W[1][m], W[2][m])
            with np.errstate(invalid="ignore"):
                hit_w = np.isfinite(tw) & (uw >= 0) & (vw >= 0) & (uw + vw <= 1) & (tw >= 0)
            np.minimum.at(best_w, r[hit_w] + lo, tw[hit_w])
            # triangles the ray runs along (nearly in their plane): a float32 test may hit them anywhere along the overlap
            with np.errstate(invalid="ignore", divide="ignore"):
                along = np.abs(_dot(dd, self.normal_obj[m])) < GRAZING_COS * np.linalg.norm(dd, axis=-1) * norm_n[m]
            ra, ma, oa, da = r[along], m[along], oo[along], dd[along]
            for k in range(3):
                a, b = P[k][ma], P[(k + 1) % 3][ma]
                dist, s_ = self._near_thin(oa, da, a, b)
                close = dist < 1e-3 * np.linalg.norm(b - a, axis=-1) + 64 * EPS32 * (np.abs(oa).max(-1) + np.abs(a).max(-1))
                add(ra[close] + lo, ma[close], s_[close])
            if len(thin_pairs):   # slivers and zero-area triangles the ray passes close to (every ray against each)
                r, k = np.nonzero(np.ones((len(o), len(thin_pairs)), bool))
                m = thin_pairs[k]
                oo, dd = self._object_rays(o[r], d[r], self.inv[self.inst[m]])
                a, b = self.seg_a[m], self.seg_b[m]
                dist, s_ = self._near_thin(oo, dd, a, b)
                close = dist < 1e-3 * np.linalg.norm(b - a, axis=-1) + 64 * EPS32 * (np.abs(oo).max(-1) + np.abs(a).max(-1))
                add(r[close] + lo, m[close], s_[close])
        cr, cm, ct, cu, cv, cthin = (np.concatenate(x) for x in (cr, cm, ct, cu, cv, cthin))
        tol_t, tol_uv = self._tolerances(o32[cr], d32[cr], cm)
        seg = np.linalg.norm(self.seg_b[cm] - self.seg_a[cm], axis=-1)
        tol_t = np.where(cthin, seg, tol_t)            # (a float32 hit on a sliver may lie anywhere along it)
        with np.errstate(invalid="ignore"):
            margin = np.minimum(np.minimum(cu, cv), 1.0 - cu - cv)
        c_true = ~cthin & (margin >= 0) & (ct >= 0)
        _, dd = self._object_rays(o32[cr].astype(np.float64), d32[cr].astype(np.float64), self.inv[self.inst[cm]])
        nrm = self.normal_obj[cm]
        dn = _dot(dd, nrm)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = np.abs(dn) / (np.linalg.norm(dd, axis=1) * np.linalg.norm(nrm, axis=1))
        # the margin a candidate needs: BARY_MARGIN, or its own tolerance on u, v where that is more (a float32
        # u or v that is off by less cannot change sides; the instance 1e3 units away needs it: its object-space
        # origins carry the rounding of 1e3)
        need = np.maximum(BARY_MARGIN, tol_uv)
        c_robust = c_true & (margin >= need) & (cos >= GRAZING_COS) & ~self.thin[cm] & (need <= PREFILTER_MARGIN)

        # the any-hit test: which candidates count (every one without samples)
        c_accept, c_undecided = np.ones(len(cr), bool), np.zeros(len(cr), bool)
        c_opacity, c_tol_opacity = np.ones(len(cr)), np.zeros(len(cr))
        if samples is not None:
            s32 = np.ascontiguousarray(samples, np.float32)
            assert self.opacity is not None and len(s32) == n
            c_opacity, c_tol_opacity, c_accept, c_undecided = self.opacity.decide(
                self.opacity_rng, self.inst[cm], self.prim[cm], cu, cv, np.where(np.isfinite(tol_uv), tol_uv, 0.0), s32[cr])
            c_undecided |= ~self.opacity.opaque[self.inst[cm]] & (cthin | ~np.isfinite(tol_uv))

        # the nearest (accepted) hit of every ray
        order = np.lexsort((ct, cr))
        order = order[(c_true & c_accept)[order]]
        first = order[np.unique(cr[order], return_index=True)[1]]
        hit = np.zeros(n, bool)
        hit[cr[first]] = True
        res = {k: np.zeros(n) for k in ("t", "u", "v", "cos", "facing", "tol_t", "tol_uv")}
        res["t"][:] = np.inf
        inst, prim = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        rr = cr[first]
        res["t"][rr], res["u"][rr], res["v"][rr] = ct[first], cu[first], cv[first]
        res["cos"][rr], res["facing"][rr] = cos[first], np.sign(dn[first])
        res["tol_t"][rr], res["tol_uv"][rr] = tol_t[first], tol_uv[first]
        inst[rr], prim[rr] = self.inst[cm[first]], self.prim[cm[first]]

        reason = np.zeros(n, np.int64)

        def flag(mask, code):
            np.bitwise_or.at(reason, cr[mask], code)

        is_first = np.zeros(len(cr), bool)
        is_first[first] = True
        best = res["t"][cr]                                # (inf where the ray misses: every candidate is in range)
        in_range = (ct > -tol_t) & (ct - tol_t < best + 2.0 * res["tol_t"][cr])
        flag(is_first & (margin < need), R_MARGIN)
        flag(in_range & ~cthin & (cos < GRAZING_COS), R_GRAZING)
        flag(in_range & c_true & ~is_first & (ct - best > 1e-9 * (1.0 + best)), R_GAP)
        flag(in_range & ~c_true & ~cthin & (margin > -need), R_NEAR_MISS)
        flag(np.abs(ct) <= tol_t, R_T_ZERO)
        flag(in_range & (cthin | self.thin[cm]), R_SLIVER)
        flag(in_range & ~cthin & ((need > PREFILTER_MARGIN) | (tol_t > 1e-2 * (1.0 + np.abs(ct)))), R_CONDITION)
        if samples is not None:
            # every candidate at or before the nearest accepted hit decides the result: an undecided any-hit
            # test, or a hit on an edge (a float32 cast may take its neighbour, with another material)
            flag(in_range & c_undecided, R_OPACITY)
            flag(in_range & c_true & (margin < need), R_MARGIN)
        crossed = np.zeros(n, bool)
        crossed[cr[c_true & ~c_accept & ~c_undecided & (ct < best)]] = True

        # world space against object space: the uploaded inverse matrices belong to the forward ones
        # (the world-space pass knows no opacity: checked on the analyses without samples)
        ok = (reason == 0) & (samples is None)
        assert np.array_equal(np.isfinite(best_w[ok]), hit[ok]), "world- and object-space hit / miss differ on clear rays"
        both = ok & hit
        worst = np.abs(best_w[both] - res["t"][both]) / res["tol_t"][both]
        assert worst.size == 0 or worst.max() <= 1.0, f"world- and object-space t differ by {worst.max():.2f} tolerances"
        return Analysis(n_prims=self.n_prims, n_keys=self.n_inst * self.n_prims, hit=hit, inst=inst, prim=prim, reason=reason,
                        c_ray=cr, c_inst=self.inst[cm], c_prim=self.prim[cm], c_pair=cm, c_t=ct, c_u=cu, c_v=cv, c_tol_t=tol_t,
                        c_tol_uv=tol_uv, c_true=c_true, c_robust=c_robust, world_t=best_w, c_accept=c_accept, c_undecided=c_undecided,
                        c_opacity=c_opacity, c_tol_opacity=c_tol_opacity, crossed=crossed, **res)

    def closest(self, rays):
        return self.analyse(rays)

    def occluded(self, rays):
        return self.analyse(rays).occluded(rays["t_max"])


# ---- a float32 cast against the reference -----------------------------------------------------
BACKFACE_IS_NEGATIVE_FACING = True
"""The sign convention of the hit's backface bit (bit 31 of triangle_id), fixed once by
test_ray_truth.test_backface_convention on a hand-placed triangle: the bit is set when
d . ((p1 - p0) x (p2 - p0)) < 0 in the instance's space, with (p0, p1, p2) in the flat scene's
winding -- 'backface is clock-wise' in RayPrimitiveIntersect.inc.hlsl's left-handed frame."""


def compare_hits(truth, an, rays, hits, exact_aim=False):
    """A float32 cast's hits against the analysis. Returns {check: indices of failing rays}.
    Clear rays: hit / miss equal, (instance, triangle) in the tie set, t, u, v within the derived
    tolerances, the hit point rebuilt from u, v within tolerance of o + t d, the backface bit the
    reference's facing. Ambiguous rays: a miss, or a hit that names one of the ray's candidates (a
    hit, a near miss, a sliver or a triangle the ray runs along; with opacity samples: one that is
    accepted or undecided) at that candidate's distance.
    `exact_aim`: the family is aimed at vertices and edges, where ambiguity is the point: every
    ray is held to the ambiguous rays' rule only (no hit / miss equality, the candidates at the
    nearest distance stand in for the id)."""
    t = hits["t"].astype(np.float64)
    got = np.isfinite(t)
    tid = (hits["triangle_id"] & 0x7FFFFFFF).astype(np.int64)
    back = (hits["triangle_id"] >> 31).astype(bool)
    ins = hits["instance_index"].astype(np.int64)
    clear = an.clear & (not exact_aim)
    bad = {}
    bad["hit/miss"] = np.flatnonzero(clear & (got != an.hit))
    c = clear & got & an.hit
    # the candidate the cast names
    keys = an.c_ray * an.n_keys + an.c_inst * an.n_prims + an.c_prim
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    mine = np.arange(len(t)) * an.n_keys + ins * an.n_prims + tid
    assert len(skeys), "no ray of the batch comes near any triangle"
    pos = np.clip(np.searchsorted(skeys, mine), 0, len(skeys) - 1)
    k = order[pos]
    ties = an.tie_keys()
    in_ties = np.isin(mine, ties)
    bad["id not in tie set"] = np.flatnonzero(c & ~in_ties)
    c &= in_ties
    bad["t"] = np.flatnonzero(c & ~(np.abs(t - an.c_t[k]) <= an.c_tol_t[k]))
    for name, ref in (("u", an.c_u), ("v", an.c_v)):
        bad[name] = np.flatnonzero(c & ~(np.abs(hits[name].astype(np.float64) - ref[k]) <= an.c_tol_uv[k]))
    # the hit point, in the instance's space: (1 - u - v) p0 + u p1 + v p2 against o + t d
    pair = an.c_pair[k]
    p = truth.p_obj[pair]
    u, v = hits["u"].astype(np.float64), hits["v"].astype(np.float64)
    oo, dd = truth._object_rays(rays["origin"].astype(np.float64), rays["direction"].astype(np.float64), truth.inv[truth.inst[pair]])
    with np.errstate(invalid="ignore", over="ignore"):
        gap = np.linalg.norm((1 - u - v)[:, None] * p[:, 0] + u[:, None] * p[:, 1] + v[:, None] * p[:, 2]
                             - (oo + np.where(got, t, 0.0)[:, None] * dd), axis=1)
    edge = np.linalg.norm(p[:, 1] - p[:, 0], axis=1) + np.linalg.norm(p[:, 2] - p[:, 0], axis=1)
    bad["hit point"] = np.flatnonzero(c & ~(gap <= an.c_tol_t[k] * np.linalg.norm(dd, axis=1) + an.c_tol_uv[k] * edge))
    dn = _dot(dd, truth.normal_obj[pair])
    bad["backface"] = np.flatnonzero(c & (back != ((dn < 0) == BACKFACE_IS_NEGATIVE_FACING)))
    # ambiguous rays: a miss, or a hit that names one of the ray's candidates, at that candidate's distance
    with np.errstate(invalid="ignore"):
        ok = ((mine[an.c_ray] == keys) & (an.c_accept | an.c_undecided)
              & (np.abs(t[an.c_ray] - an.c_t) <= 2.0 * np.maximum(an.c_tol_t, an.tol_t[an.c_ray])))
    on_candidate = np.zeros(len(t), bool)
    on_candidate[an.c_ray[ok]] = True
    bad["ambiguous hit not on a candidate"] = np.flatnonzero(~clear & got & ~on_candidate)
    return {k_: v_ for k_, v_ in bad.items() if len(v_)}


def compare_occluded(an, rays, occ):
    want, ambiguous = an.occluded(rays["t_max"])
    return np.flatnonzero(~ambiguous & (want != (np.asarray(occ) != 0))), ambiguous


def describe(an, idx):
    return [(int(i), [REASONS[b] for b in REASONS if an.reason[i] & b], float(an.t[i]), int(an.inst[i]), int(an.prim[i]))
            for i in idx[:5]]


# ---- scenes --------------------------------------------------------------------------------------
def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.sign(np.linalg.det(q))


def transform_set(rng, spacing=0.0):
    """Six 4x4 matrices (column-vector convention): identity, uniform scale, non-uniform scale,
    mirrored (negative determinant), sheared (arbitrary entries) and one translated by 1e3 units
    (float32 cancellation in o - v). `spacing` > 0 lays them out that far apart."""
    lin = [np.eye(3),
           0.7 * _rotation(rng),
           _rotation(rng) @ np.diag([1.6, 0.5, 1.1]),
           _rotation(rng) @ np.diag([-1.0, 1.0, 0.9]),
           np.eye(3) + rng.uniform(-0.45, 0.45, (3, 3)),
           _rotation(rng)]
    assert np.linalg.det(lin[3]) < 0 and abs(np.linalg.det(lin[4])) > 0.2
    out = []
    for k, a in enumerate(lin):
        m = np.eye(4)
        m[:3, :3] = a
        if k:
            m[:3, 3] = rng.uniform([-1.5, -0.3, -1.5], [1.5, 0.5, 1.5]) if not spacing else (spacing * (k % 3), 0.0, spacing * (k // 3))
        if k == 5:
            m[0, 3] += 1000.0
        out.append(m)
    return out


def _matrix(m):
    return " ".join(f"{v:.9g}" for v in np.asarray(m).reshape(-1))     # (single spaces: the loader needs 16 fields)


def _write_xml(d, meshes):
    """meshes: [(obj file name, [4x4 matrices])]."""
    from directcomputeraytracing_amd.scenes import _sensor, _xml, mitsuba_matrix
    shapes = "".join(f'  <shape type="obj" id="s{i}_{k}"><string name="filename" value="{name}"/><ref id="b0"/>'
                     f'<transform name="to_world"><matrix value="{_matrix(m)}"/></transform></shape>\n'
                     for i, (name, ms) in enumerate(meshes) for k, m in enumerate(ms))
    body = ('  <integrator type="path"><integer name="max_depth" value="3"/></integrator>\n'
            + _sensor("perspective", 48, 36, mitsuba_matrix((0.0, 1.4, -4.2), pitch=15.0), '    <float name="fov" value="50"/>\n')
            + '  <bsdf type="diffuse" id="b0"><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>\n' + shapes
            + '  <emitter type="constant"><rgb name="radiance" value="1, 1, 1"/></emitter>\n')
    p = Path(d) / "truth.xml"
    p.write_text(_xml(body))
    return p


def write_soup_scene(directory, seed, n_grid=6, n_loose=12, n_instances=6):
    """A random soup (tests/random_scenes.soup: its slivers, zero-area triangles and coincident
    duplicates stay in as hazards) under the first `n_instances` transforms of `transform_set`."""
    import random_scenes as R
    rng = np.random.default_rng(seed)
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    R._write_soup(d / "soup.obj", *R.soup(rng, n_grid, n_loose))
    return _write_xml(d, [("soup.obj", transform_set(rng)[:n_instances])])


def _weld(V, F):
    """Vertices merged by the position an OBJ line keeps of them (six decimals)."""
    key, inverse = np.unique(np.round(np.asarray(V, np.float64), 6) + 0.0, axis=0, return_inverse=True)
    F = inverse.reshape(-1)[np.asarray(F)]
    return key, F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])]


def is_closed(F):
    """Every edge is shared by exactly two triangles (and in opposite directions)."""
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    _, count = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    _, directed = np.unique(e, axis=0, return_counts=True)
    return bool((count == 2).all() and (directed == 1).all())


def closed_lathe(segments=12):
    from directcomputeraytracing_amd.scenes import lathe
    V, _, _, F = lathe([(0.0, 0.0), (0.5, 0.0), (0.62, 0.45), (0.4, 1.0), (0.0, 1.0)], segments)   # capped at both ends
    return _weld(V, F)


def closed_polyhedron(rng, levels=2):
    """An octahedron subdivided `levels` times, every vertex moved along its own radius."""
    V = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    F = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    V = [np.asarray(v, np.float64) for v in V]
    for _ in range(levels):
        mid, out = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                V.append((V[a] + V[b]) / np.linalg.norm(V[a] + V[b]))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        F = out
    V = np.asarray(V) * rng.uniform(0.55, 0.8, (len(V), 1))
    return _weld(V, np.asarray(F))


def write_closed_scene(directory, seed):
    """A capped lathe and a jittered closed polyhedron, each closed by construction (verified:
    every edge is shared by exactly two triangles), each under `transform_set`, laid out apart."""
    from directcomputeraytracing_amd.scenes import write_obj
    rng = np.random.default_rng(seed)
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    meshes = []
    for name, (V, F) in (("lathe.obj", closed_lathe()), ("poly.obj", closed_polyhedron(rng))):
        assert is_closed(F), name
        N = V / np.maximum(np.linalg.norm(V, axis=1, keepdims=True), 1e-9) + [0.0, 1e-3, 0.0]
        write_obj(d / name, V, N, rng.uniform(0, 1, (len(V), 2)), F)
        ms = transform_set(rng, spacing=3.0)
        if name == "poly.obj":
            for m in ms:
                m[1, 3] += 3.0
        meshes.append((name, ms))
    return _write_xml(d, meshes)


# ---- any-hit opacity: the veil scene and the edit that gives a flat scene its materials -----------------
VEIL_LAYERS, VEIL_SPACING = 4, 0.25
VEIL_GRID, WALL_GRID = 2, 1           # quads along a side: 62 triangles in all, so that the scene fits the cast's LDS cache whole
CARD_STEP, CARD_GAP = 0.5, 1.0       # the cards' pitch along x and the distance from a front card to its back card
CARD_ORIGIN = (6.0, -2.0, 0.8)       # (away from the veils and the wall; no card's plane through the world's origin)


def _grid(n, size, z, rng, jitter=0.0):
    """An n x n grid of quads over [-size, size]^2 at height z: vertices (jittered in the plane) and triangles."""
    g = np.linspace(-size, size, n + 1)
    V = np.stack([*np.meshgrid(g, g, indexing="ij"), np.full((n + 1, n + 1), z)], -1).reshape(-1, 3)
    V[:, :2] += rng.uniform(-jitter, jitter, (len(V), 2)) * (2.0 * size / n)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
    return V, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])


def card_count():
    return len(CARDS)


def write_veil_scene(directory, seed):
    """VEIL_LAYERS translucent layers (VEIL_GRID x VEIL_GRID quads each, VEIL_SPACING apart) as one mesh under three adjacent
    instances -- mirrored, sheared and uniformly scaled (`transform_set`) --, an opaque back wall behind them, and
    the exact families' cards: per card a front quad and, CARD_GAP behind it, a back quad (`exact_cards`)."""
    from directcomputeraytracing_amd.scenes import write_obj
    rng = np.random.default_rng(seed)
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    up = np.array([0.0, 0.0, -1.0])

    def put(name, parts):
        V = np.concatenate([p[0] for p in parts])
        F = np.concatenate([p[1] + off for p, off in zip(parts, np.cumsum([0] + [len(p[0]) for p in parts[:-1]]))])
        write_obj(d / name, V, np.repeat(up[None], len(V), 0), rng.uniform(0.0, 1.0, (len(V), 2)), F)
    put("veil.obj", [_grid(VEIL_GRID, 1.0, k * VEIL_SPACING, rng, 0.2) for k in range(VEIL_LAYERS)])
    put("wall.obj", [_grid(WALL_GRID, 4.0, 0.0, rng, 0.2)])
    cards = []
    for k in range(card_count()):
        for z in (0.0, CARD_GAP):
            V, F = _grid(1, 0.2, z, rng)
            cards.append((V + [k * CARD_STEP, 0.0, 0.0], F))
    put("cards.obj", cards)
    ms = transform_set(rng)
    wall, card = np.eye(4), np.eye(4)
    wall[:3, 3] = (0.0, 0.0, 2.5)
    card[:3, 3] = CARD_ORIGIN
    return _write_xml(d, [("veil.obj", [ms[3], ms[4], ms[1]]), ("wall.obj", [wall]), ("cards.obj", [card])])


# The materials every opacity case gets (`opacity_edit`): (opacity, opacity texture or -1, tex_tiling)
M_OPAQUE, M_ZERO, M_CONST, M_R8, M_RGBA, M_DYADIC, M_HALF = range(7)
CONST_OPACITY = np.float32(0.37)
MATERIALS = [(1.0, -1, (1.0, 1.0)), (0.0, -1, (1.0, 1.0)), (CONST_OPACITY, -1, (1.0, 1.0)), (0.8, 0, (2.5, -1.5)),
             (1.0, 1, (-0.75, 3.0)), (1.0, 2, (1.0, 1.0)), (0.5, 2, (2.0, -1.0))]
ONE_BELOW = np.float32(1.0 - 2.0 ** -24)


# The exact families' cards: (front quad's material, the texel (x, y) of the dyadic texture its constant texcoord names)
CARDS = [(M_CONST, None), (M_ZERO, None), (M_OPAQUE, None), (M_DYADIC, (1, 2)), (M_DYADIC, (2, 2)), (M_HALF, (3, 0)), (M_HALF, (0, 1))]


def exact_cards():
    """The aimed families float32 decides exactly: (card, opacity sample, accepted). `<` is strict: a sample
    equal to the opacity passes through, the float just below it is accepted."""
    c, zero = CONST_OPACITY, np.float32(0.0)
    return [(0, c, False), (0, np.nextafter(c, zero), True),          # a constant opacity
            (1, zero, False),                                          # opacity 0, sample 0
            (2, ONE_BELOW, True),                                      # opacity 1, sample 1 - 2^-24
            (3, ONE_BELOW, True), (3, zero, True),                     # a texel of 1
            (4, zero, False),                                          # a texel of 0
            (5, np.float32(0.5), False), (5, np.nextafter(np.float32(0.5), zero), True),   # opacity 1/2 x a texel of 1, a negative tiling
            (6, zero, False)]


def opacity_textures(rng):
    """[(format, pixels)]: an R8 texture, an RGBA one whose red and alpha differ, and an R8 one of 0 and 255
    alone (texel values 0 and 1: the dyadic texture of the exact families)."""
    r8 = rng.integers(0, 256, (8, 8, 1)).astype(np.uint8)
    rgba = rng.integers(0, 256, (4, 8, 4)).astype(np.uint8)
    rgba[..., 3] = 255 - rgba[..., 0]
    dyadic = (((np.add.outer(np.arange(4), np.arange(4)) % 3) == 0) * 255).astype(np.uint8)[..., None]   # [y][x]
    return [(1, r8), (0, rgba), (1, dyadic)]


def opacity_edit(flat, frame, seed, instances, cards=False, keep=()):
    """A copy of `flat` (a dcrt_flat_scene; `frame` its frame parameters, `keep` what owns it) with MATERIALS,
    the three textures, a random material per triangle, texcoords stretched to [-1, 2) and, per instance,
    `instances[i]` = (OPAQUE flag, override or NO_OVERRIDE). `cards`: the last 4 * card_count() triangles are
    the veil scene's cards and get the exact families' materials and constant texel-centre texcoords
    (`.cards`: {triangle: (card, is front)}). The fields no loader sets (tex_tiling, the textures) are edited
    in the flat scene, as tests/test_shading_ref.py does. The copy keeps its arrays alive."""
    import ctypes as C
    import shading_ref as S
    from test_shading_ref import Case as FlatCase
    rng = np.random.default_rng(seed)
    s = S.from_flat(flat)
    n_tri, n_inst = len(s["triangles"]), flat.instance_count
    assert len(instances) == n_inst, (len(instances), n_inst)
    base = s["materials"][0].copy()
    mats = np.repeat(base[None], len(MATERIALS), 0)
    for k, (op, tex, tiling) in enumerate(MATERIALS):
        mats[k, 8:10] = np.asarray(tiling, np.float32).view(np.uint32)
        mats[k, 10] = np.asarray([op], np.float32).view(np.uint32)[0]
        mats[k, 12] = np.asarray([tex], np.int32).view(np.uint32)[0]
    ids = rng.choice([M_OPAQUE, M_ZERO, M_ZERO, M_CONST, M_R8, M_R8, M_RGBA, M_RGBA], n_tri).astype(np.uint32)
    V = s["vertices"].copy()
    V[:, 9:11] = V[:, 9:11] * np.float32(3.0) - np.float32(1.0)
    textures = opacity_textures(rng)
    where = {}
    if cards:
        # (a BVH build orders a mesh's triangles its own way: a card's are found by where they lie)
        table = CARDS
        first = n_tri - 4 * len(table)
        centre = np.abs(s["vertices"][s["triangles"][first:]][..., :3].astype(np.float64).mean(1))
        card, front = np.rint(centre[:, 0] / CARD_STEP).astype(int), centre[:, 2] < 0.5 * CARD_GAP
        assert all(((card == k) & (front == f)).sum() == 2 for k in range(len(table)) for f in (False, True))
        for tri, k, f in zip(range(first, n_tri), card, front):
            mat, texel = table[k]
            where[tri] = (int(k), bool(f))
            ids[tri] = mat if f else M_OPAQUE
            if f and texel is not None:                           # tiling x texcoord = the texel's centre, some periods away
                tc = ((np.asarray(texel, np.float64) + 0.5) / 4.0 + (3.0, -2.0)) / np.asarray(MATERIALS[mat][2], np.float64)
                V[s["triangles"][tri], 9:11] = tc.astype(np.float32)
    case = FlatCase(flat, frame, list(keep)).edit(vertices=V, materials=mats, material_ids=ids, textures=textures,
                                                  overrides=np.asarray([o for _, o in instances], np.uint32))
    flags = np.asarray([FLAG_OPAQUE if f else 0 for f, _ in instances], np.uint32)
    case.flat.instance_flags = flags.ctypes.data_as(C.POINTER(C.c_uint32))
    case._keep.append(flags)
    case.flat.owner = case           # (the struct keeps the arrays it points into alive)
    case.flat.cards = where
    return case.flat


CLOSED_SMALL_SEED = 2


def write_closed_small_scene(directory, seed=CLOSED_SMALL_SEED):
    """One jittered closed polyhedron of 32 triangles under `transform_set`, laid out apart: closed meshes
    small enough for the cast's LDS cache to hold the scene whole."""
    from directcomputeraytracing_amd.scenes import write_obj
    rng = np.random.default_rng(seed)
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    V, F = closed_polyhedron(rng, levels=1)
    assert is_closed(F) and len(F) == 32
    write_obj(d / "poly.obj", V, V / np.linalg.norm(V, axis=1, keepdims=True), rng.uniform(0, 1, (len(V), 2)), F)
    return _write_xml(d, [("poly.obj", transform_set(rng, spacing=3.0))])


def point_triangle_distance(p, a, b, c):
    """Distance from points p (N, 3) to triangles (M, 3) each: (N, M). Ericson, Real-Time
    Collision Detection 5.1.5, vectorised."""
    p = p[:, None]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        den = 1.0 / (va + vb + vc)
        q = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]   # the face region

        def put(mask, value):
            nonlocal q
            q = np.where(mask[..., None], value, q)
        put((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None])
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[..., None])
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[..., None])
        put((d6 >= 0) & (d5 <= d6), np.broadcast_to(c, q.shape))
        put((d3 >= 0) & (d4 <= d3), np.broadcast_to(b, q.shape))
        put((d1 <= 0) & (d2 <= 0), np.broadcast_to(a, q.shape))
    return np.linalg.norm(p - q, axis=-1)


# ---- rays -----------------------------------------------------------------------------------------
def _rays(O, T, rng, d=None):
    """Rays from O towards T (or along d), float32, a quarter of them with a finite t_max around
    the distance to the target."""
    from directcomputeraytracing_amd import make_rays
    O, T = np.asarray(O, np.float64), np.asarray(T, np.float64)
    dist = np.linalg.norm(T - O, axis=1)
    if d is None:
        keep = dist > 1e-6
        O, T, dist = O[keep], T[keep], dist[keep]
        d = (T - O) / dist[:, None]
    r = make_rays(O.astype(np.float32), np.asarray(d).astype(np.float32), 0.0, np.inf)
    k = len(r) // 4
    r["t_max"][:k] = (dist[:k] * rng.uniform(0.3, 1.7, k)).astype(np.float32)
    return r[rng.permutation(len(r))]


def _origins(truth, targets, rng, reach=(0.3, 2.0), outside=0.5):
    """Origins `reach` away from their targets, strictly inside the scene's root box, and a share
    `outside` of them moved out of it (above or below)."""
    lo, hi = truth.box
    n = len(targets)
    step = rng.normal(size=(n, 3))
    O = targets + step / np.linalg.norm(step, axis=1, keepdims=True) * rng.uniform(*reach, (n, 1))
    inside = rng.random(n) >= outside
    O[inside] = np.clip(O[inside], lo + 1e-3 * (hi - lo), hi - 1e-3 * (hi - lo))
    out = ~inside
    O[out, 1] = np.where(rng.random(out.sum()) < 0.5, hi[1] + rng.uniform(0.3, 2.0, out.sum()), lo[1] - rng.uniform(0.3, 2.0, out.sum()))
    return O


def ray_families(truth, seed, per_family=1500, reach=(0.3, 2.0), outside=0.5):
    """{family: rays}. interior: random interior points of non-sliver triangles; near_vertex: points
    2 % of the way in from a vertex; grazing: onto faces at 0.3-3 degrees; axis: axis-aligned rays
    (exactly zero direction components, infinite 1 / d) through interior points; zero_origin:
    origins with exactly zero components; exact: aimed exactly at world-space vertices and
    edge midpoints, and leaving from the vertices themselves."""
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero(~truth.thin)
    P = truth.p_world
    # fewer aims at an instance far from the origin: float32 leaves its rays a coarser t, u and v, so more
    # of them are ambiguous, and the caps on the ambiguous share are a condition on these aims
    weight = np.where(np.abs(truth.fwd[truth.inst[ok], 3]).max(1) > 100.0, 0.3, 1.0)
    weight /= weight.sum()

    def interior(n, lowest=0.1):
        m = rng.choice(ok, n, p=weight)
        b = rng.dirichlet([1.0, 1.0, 1.0], n) * (1.0 - 3.0 * lowest) + lowest
        return m, np.einsum("nk,nkc->nc", b, P[m])

    fam = {}
    n = per_family
    m, T = interior(n)
    T[: n // 5] += rng.normal(size=(n // 5, 3))         # (a fifth aimed nowhere: misses, and hits at any angle)
    fam["interior"] = _rays(_origins(truth, T, rng, reach, outside), T, rng)
    m = rng.choice(ok, n, p=weight)
    b = np.full((n, 3), 0.02)
    b[np.arange(n), rng.integers(0, 3, n)] = 0.96
    T = np.einsum("nk,nkc->nc", b, P[m])
    fam["near_vertex"] = _rays(_origins(truth, T, rng, reach, outside), T, rng)
    m, T = interior(n, 0.2)        # grazing: the direction is a tangent tilted by 0.3-3 degrees towards the face
    nw = _cross(P[m, 1] - P[m, 0], P[m, 2] - P[m, 0])
    nw /= np.linalg.norm(nw, axis=1, keepdims=True)
    tang = _cross(nw, rng.normal(size=(n, 3)))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(0.3, 3.0, (n, 1))) * rng.choice([-1.0, 1.0], (n, 1))
    D = np.cos(ang) * tang - np.sin(ang) * nw
    fam["grazing"] = _rays(T - D * rng.uniform(0.1, 0.3, (n, 1)) * reach[1], T, rng)
    m, T = interior(n)
    nw = _cross(P[m, 1] - P[m, 0], P[m, 2] - P[m, 0])
    axis = np.abs(nw).argmax(1)                          # (the axis the face is steepest to: not along a flat patch)
    D = np.zeros((n, 3))
    D[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
    fam["axis"] = _rays(T - D * rng.uniform(*reach, (n, 1)), T, rng, d=D)
    m, T = interior(n)
    O = _origins(truth, T, rng, reach, outside)
    O[np.arange(n), np.abs(O).argmin(1)] = 0.0            # (the component that moves the origin least)
    O[: n // 4][rng.random((n // 4, 3)) < 0.5] = 0.0
    O[: n // 16] = 0.0
    fam["zero_origin"] = _rays(O, T, rng)
    m = rng.choice(len(P), n)
    k = rng.integers(0, 3, n)
    verts = P[m, k]
    mids = 0.5 * (P[m, k] + P[m, (k + 1) % 3])
    T = np.concatenate([verts[: n // 3], mids[n // 3: 2 * n // 3]])
    O = np.concatenate([_origins(truth, T, rng, reach, outside), verts[2 * n // 3:]])
    T = np.concatenate([T, P[rng.choice(ok, n - len(T)), 0] * 0.5 + 0.5 * P[rng.choice(ok, n - len(T)), 1]])
    fam["exact"] = _rays(O, T, rng)
    return fam


CAPS = {"interior": 0.02, "axis": 0.02, "zero_origin": 0.02, "near_vertex": 0.05, "grazing": 0.05, "exact": None}
BATCH_SIZES = (1, 63, 65, 257, 10007)

# scene -> how it is generated and aimed at. The seeds and reaches are chosen so that the reference alone
# meets CAPS (the cap is a condition on the aims, asserted by the tests, not a measurement of the cast).
SCENES = {
    "soup": dict(seed=4, per_family=1700),                                    # 6 x 90 triangles, every transform
    "closed": dict(seed=1, per_family=700),                                   # 12 closed meshes
    "large": dict(seed=1003, per_family=600, reach=(0.05, 0.3), outside=0.1),  # 3 x 5.2 k triangles: deeper than the LDS node cache
    "obj": dict(seed=2, per_family=700),                                      # identity-only OBJ scene, 44 triangles
    "veil": dict(seed=4, per_family=1200),                                    # 3 x 32 veil triangles, a wall, the cards
    "small": dict(seed=5, per_family=700),                                    # a soup small enough for the cast's LDS cache, every transform
}
CAPPED = ("soup", "large", "obj", "veil", "small")
# the any-hit cases: scene -> per instance (OPAQUE flag, material override). Adjacent instances differ in both, so
# a flag or an override carried over from the previous TLAS leaf shows.
OPACITY_INSTANCES = {
    # by mesh (the flat scene's instances come in the TLAS builder's order): the veil's three instances in that order,
    # the wall (its triangles' random materials overridden by the opaque one, without the flag), the cards
    "veil": {"veil": [(True, M_OPAQUE), (False, M_R8), (False, NO_OVERRIDE)], "wall": [(False, M_OPAQUE)], "cards": [(False, NO_OVERRIDE)]},
    # (an OPAQUE instance whose override says opacity 0: the flag wins)
    "soup": {"soup": [(True, M_ZERO), (False, M_R8), (False, NO_OVERRIDE), (False, M_RGBA), (True, NO_OVERRIDE), (False, NO_OVERRIDE)]},
}
OPACITY_INSTANCES["small"] = OPACITY_INSTANCES["soup"]


def opacity_instances(name, flat):
    """Per instance of the flat scene (OPAQUE flag, material override): OPACITY_INSTANCES[name], its meshes told
    apart by their triangle counts."""
    import ctypes as C
    import shading_ref as S
    roles = {k: list(v) for k, v in OPACITY_INSTANCES[name].items()}
    if len(roles) == 1:
        return next(iter(roles.values()))
    size = {VEIL_LAYERS * 2 * VEIL_GRID ** 2: "veil", 2 * WALL_GRID ** 2: "wall", 4 * card_count(): "cards"}
    nodes = S._array(flat.bvh_nodes, C.c_uint32, (flat.bvh_node_count, 8))
    return [roles[size[len(p)]].pop(0) for _, p in instance_triangles(nodes)]
# the seed of a case's materials per triangle, texture bytes and opacity samples: chosen, like SCENES', so that the
# reference alone meets CAPS with the samples in
OPACITY_SEEDS = {"veil": 1, "soup": 7, "small": 1}
CROSSING_SHARE = 0.30      # interior rays that pass a clearly rejected hit before their result, at least


def load_scene(name, directory):
    import random_scenes as R
    from directcomputeraytracing_amd import Scene
    s = Scene((48, 36))
    if name == "closed_small":
        s.load_from_file(write_closed_small_scene(directory))
        return s
    seed = SCENES[name]["seed"]
    if name == "soup":
        s.load_from_file(write_soup_scene(directory, seed))
    elif name == "closed":
        s.load_from_file(write_closed_scene(directory, seed))
    elif name == "large":
        s.load_from_file(write_soup_scene(directory, seed, n_grid=48, n_loose=600, n_instances=3))
    elif name == "veil":
        s.load_from_file(write_veil_scene(directory, seed))
    elif name == "small":
        s.load_from_file(write_soup_scene(directory, seed, n_grid=3, n_loose=5))
    else:
        R.setup_obj_scene(s, R.write_obj_scene(directory, seed), seed)
    return s


class Case:
    """One scene's reference: the families' rays and their analyses, computed once."""

    def __init__(self, name, flat_arrays, opacity=None):
        """`opacity`: an `Opacity` over the same flat scene: every ray carries a uniform opacity sample
        (`samples`), and the analyses are those of the any-hit test."""
        cfg = dict(SCENES[name])
        self.name = name
        self.truth = Truth(flat_arrays, cfg["seed"], opacity)
        self.families = ray_families(self.truth, cfg.pop("seed"), **cfg)
        self.samples = None
        if opacity is not None:
            rng = np.random.default_rng(OPACITY_SEEDS[name])
            self.samples = {k: rng.random(len(r), np.float32) for k, r in self.families.items()}
        self.analyses = {k: self.truth.analyse(r, None if self.samples is None else self.samples[k]) for k, r in self.families.items()}

    def shares(self):
        return {k: float((~a.clear).mean()) for k, a in self.analyses.items()}

    def largest_tolerances(self):
        """(absolute tol_t, tol_t relative to max(t, 1), tol_uv) over the clear hits of every family."""
        out = np.zeros(3)
        for a in self.analyses.values():
            c = a.clear & a.hit
            if c.any():
                out = np.maximum(out, [a.tol_t[c].max(), (a.tol_t[c] / np.maximum(a.t[c], 1.0)).max(), a.tol_uv[c].max()])
        return out

    def check(self, trace, occluded, families=None):
        """Every family through `trace(rays)` and `occluded(rays)` -- with opacity samples:
        `trace(rays, samples)` and `occluded(rays, samples)` --; a list of failure messages."""
        msgs = []
        for fam in families or self.families:
            rays, an = self.families[fam], self.analyses[fam]
            args = (rays,) if self.samples is None else (rays, self.samples[fam])
            for what, idx in compare_hits(self.truth, an, rays, trace(*args), exact_aim=(fam == "exact")).items():
                msgs.append(f"{self.name}/{fam}: {what}: {len(idx)} of {len(rays)} rays, first {describe(an, idx)}")
            idx, _ = compare_occluded(an, rays, occluded(*args))
            if len(idx):
                msgs.append(f"{self.name}/{fam}: occluded: {len(idx)} of {len(rays)} rays differ, first {describe(an, idx)}")
        return msgs

    def mixed(self, n):
        """The first n rays of all families interleaved, with the analysis rows that go with them."""
        rays = np.concatenate(list(self.families.values()))
        order = np.random.default_rng(7).permutation(len(rays))[:n]
        return rays[order], order


def mixed_kinds(n):
    """0 (closest hit) / 1 (any hit) per ray: alternating over the first half of the batch, in runs of 64
    over the second, so that a cast's waves are both mixed and pure."""
    i = np.arange(n)
    return np.where(i < n // 2, i & 1, (i >> 6) & 1).astype(np.uint32)


def cast_both(cast, rays, samples=None):
    """(closest hits, occlusion words) of every ray through `cast(rays, kinds, samples) -> (hits, occluded)`:
    two batches with complementary `mixed_kinds`, so each ray is cast as both kinds and every batch mixes them.
    A ray's unused output must be the miss record / 0."""
    kinds = mixed_kinds(len(rays))
    h0, o0 = cast(rays, kinds, samples)
    h1, o1 = cast(rays, 1 - kinds, samples)
    for h, o, k in ((h0, o0, kinds), (h1, o1, 1 - kinds)):
        assert np.isinf(h["t"][k == 1]).all() and not h["triangle_id"][k == 1].any() and not o[k == 0].any()
    closest = kinds == 0
    hits = h1.copy()
    hits[closest] = h0[closest]
    return hits, np.where(closest, o1, o0)


def largest_opacity_tolerance(case):
    """The largest tolerance on the opacity among the decided candidates of the clear rays of every family."""
    out = 0.0
    for a in case.analyses.values():
        m = a.clear[a.c_ray] & ~a.c_undecided & np.isfinite(a.c_tol_opacity) & ~case.truth.opacity.opaque[a.c_inst]
        out = max(out, float(a.c_tol_opacity[m].max()) if m.any() else 0.0)
    return out


def exact_opacity_rays(truth, cards):
    """The aimed families of `exact_cards`, one ray per sample and front triangle of its card: straight through an
    interior point of the front triangle (0.7 in front of it) towards the back card CARD_GAP behind. Returns
    (rays, samples, accepted, front triangle, card): a closest-hit ray must name the front triangle when
    accepted and a triangle of the card's back quad otherwise; with t_max between the two quads (the rays'
    t_max) an any-hit ray is occluded iff accepted."""
    from directcomputeraytracing_amd import make_rays
    O, D, S, A, F, K = [], [], [], [], [], []
    pair_of = {int(p): m for m, p in enumerate(truth.prim) if int(p) in cards}      # (the cards' instance is the only one of its mesh)
    centre = {kf: np.mean([truth.p_world[pair_of[t]].mean(0) for t, v in cards.items() if v == kf], 0) for kf in set(cards.values())}
    for tri, (k, front) in sorted(cards.items()):
        if not front:
            continue
        p = truth.p_world[pair_of[tri]]
        d = centre[(k, False)] - centre[(k, True)]
        d /= np.linalg.norm(d)
        target = 0.5 * p[0] + 0.3 * p[1] + 0.2 * p[2]
        for card, sample, accepted in exact_cards():
            if card == k:
                O.append(target - 0.7 * d), D.append(d), S.append(sample), A.append(accepted), F.append(tri), K.append(k)
    rays = make_rays(np.asarray(O, np.float32), np.asarray(D, np.float32), 0.0, np.float32(0.7 + 0.5 * CARD_GAP))
    return rays, np.asarray(S, np.float32), np.asarray(A, bool), np.asarray(F), np.asarray(K)


def hand_scene(triangles, matrices=(np.eye(4),)):
    """Flat-scene arrays made by hand: `triangles` (n, 3, 3) in one BLAS leaf, one instance of it
    per 4x4 matrix (column-vector convention), a TLAS chain over them. Every box is zero: the
    reference does not read them."""
    tri = np.asarray(triangles, np.float32).reshape(-1, 3, 3)
    n = len(matrices)
    vertices = np.zeros((3 * len(tri), 11), np.uint32)
    vertices[:, :3] = tri.reshape(-1, 3).view(np.uint32)
    nodes = np.zeros((2 * n, 8), np.uint32)
    for i in range(n - 1):
        nodes[2 * i, 6] = 2 * i + 2                        # interior: children 2 i + 1 and 2 i + 2
        nodes[2 * i + 1, 6:] = (2 * n - 1, 4 | (i << 3))   # TLAS leaf: instance i, BLAS root
    nodes[2 * n - 2, 6:] = (2 * n - 1, 4 | ((n - 1) << 3))
    nodes[2 * n - 1, 6:] = (0, len(tri) << 3)              # BLAS leaf: every triangle
    xf = [np.asarray(m, np.float64)[:3].reshape(-1) for m in matrices]     # three columns of four: rows of the 3x4
    xf += [np.linalg.inv(np.asarray(m, np.float64))[:3].reshape(-1) for m in matrices]
    return {"vertices": vertices, "triangles": np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3), "bvh_nodes": nodes,
            "instance_transforms": np.asarray(xf, np.float32).view(np.uint32)}
