"""A float64 reference of the path integrator's EXPECTED sample radiance, written from the rendering
equation: it calls neither the CPU oracle nor the product and shares no code with either's path loop.
tests/test_path_ref.py holds the oracle to it, tests/test_gpu_path_ref.py the device (wavefront and
megakernel), both through the fixture tests/golden/path_truth.json that `python tests/path_ref.py --write`
produces (a few minutes; the seed is recorded in the file).

What it builds on (each independent of the renderer and pinned by its own tests): tests/ray_truth.py --
`instance_triangles`, `moller_trumbore` and `Opacity` (brute-force float64 intersection of every
(instance, triangle) pair, and the any-hit opacity value); tests/shading_ref.py -- `from_flat`,
`camera_ray`, `hit`, `env_lookup`, `evaluate_light`; tests/bsdf_ref.py -- `evaluate`, `sampled_density`,
the Fresnel terms and the LUT lookups (`delta_lobes` is the scalar definition the vectorised
`delta_lobes_many` here is held to, tests/test_path_ref.py; a smooth plastic's coat included).

The estimand. Vertex k = 0 is the camera ray's first hit, B = max_bounce.
  * Cast: the nearest hit. Under the any-hit feature (0x10) a crossing of opacity a is accepted with
    probability a (see QUIRK P1 for how the crossings of one ray depend on each other).
  * Emission at vertex k -- the environment on a miss, or a lamp triangle seen from its emitting side
    (`evaluate_light`) -- is added times W: W = 1 at k = 0 with LIGHT_VISIBLE (0x04) and 0 without;
    W = 1 after a delta lobe; W = m otherwise (below).
  * The path stops on a miss or when k > B: vertices 0..B are shaded, emission is seen at 0..B + 1.
  * Delta lights (point, directional) add sum f(wi, wo) |n_s.wi| Le Tr at every shaded vertex, exactly
    (no sampling; the light count cancels, shading QUIRK Q8). Tr is 0 or 1, or the chance that the
    shadow ray passes every crossing under 0x10.
  * Continuation: the integral over the sphere of f |n_s.wi| (s / q) L_{k+1}, plus the delta lobes; q
    is the pdf the sampler reports (`evaluate`), s the density it draws from (`sampled_density`).
  * The MIS model -- the one place where the renderer's documented quirks enter, as data: for a
    direction that reaches an emitter, p = `evaluate_light`'s pdf, p_s the pdf the light sampler
    reports (2 p for mesh lights, shading QUIRK Q3; p for the environment), ph(a, b) = a^2 / (a^2 + b^2),
        m = ph(p_s, q) p / p_s + ph(q, p) s / q
    -- the expected weight of the two strategies together: light samples are drawn with density p and
    carry ph(p_s, q) / p_s, BSDF samples are drawn with density s and carry ph(q, p) / q. An unbiased
    pair (p_s = p, s = q) has m = 1; `mis_model=False` forces m = 1.

How it integrates: its own generator (np.random.default_rng) and its own proposals -- a cosine
direction about the shading normal on wo's side at reflecting vertices, at a rough dielectric a uniform
direction on the sphere or one of Walter's single-scattering sampler, half and half
(`dielectric_proposal`), a lobe chosen by its probability at delta vertices, at a mixed vertex (smooth
plastic) the coat's delta lobe with a probability of its own choosing and the cosine direction otherwise -- and NO next-event
estimation towards area lights or the environment: the strategy differs from the product's on purpose,
only the expectation is shared. One run serves every B of a scene (the terms of vertex k count for
every B >= k, its emission for every B >= k - 1) and both states of LIGHT_VISIBLE (the k = 0 emission
is kept apart).

QUIRK P1 (data, switch `shared_opacity_draw`): the renderer draws ONE opacity number per cast ray and
tests every crossing of that ray against it (WavefrontPathTracing.hlsl:109, :166, :224-225 hand the
path's single g_OpacitySamples entry to the traversal; BVHAccel.inc.hlsl:188, :331 pass it to every
AnyHitShader call), so a ray that crosses opacities a1, a2 passes both with probability
1 - max(a1, a2), not (1 - a1)(1 - a2), and stops at the first crossing whose opacity exceeds the draw.
`shared_opacity_draw=False` draws per crossing.

Mixed vertices. A smooth plastic has a continuous lobe (its Lambert base, which `evaluate` and
`sampled_density` describe, weighted 1 - coat) next to a delta lobe (the coat, `delta_lobes`): delta lights
reach it through `evaluate`; the continuation picks the coat with a probability P of this reference's
choosing (the coat weight) and weights it 1 / P, delta = True, q = s = 1, or else proposes a cosine
direction weighted 1 / (1 - P) with q and s as at any reflecting vertex. A rough dielectric with
multiscattering (BSDF QUIRK Q1) needs nothing of its own here: s / q is in the continuation and in m.

Kept out of the scenes, because this reference does not cover them:
  * roughness textures (the checkerboard of alphas): no loader and no scene call sets has_roughness_texture,
    so only a hand-edited flat scene reaches it, and tests/shading_ref.py pins the per-hit alpha it gives;
  * non-rigid or non-uniformly scaled instances (shading QUIRK Q1: the renderer's normals are then
    not the true ones);
  * lamps near the 1e-6 area threshold (shading QUIRK Q4);
  * geometry closer than 1e-2 to other geometry: the renderer offsets ray origins along the geometry
    normal (offset_ray_origin), this reference starts rays at the hit point and ignores hits with
    t <= T_MIN, and the two agree only when nothing lies in between.
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

import bsdf_ref as R
import ray_truth as RT
import shading_ref as S

T_MIN = 1e-6                 # a ray leaving a surface ignores hits nearer than this (its own triangle)
NO_LIGHT = 0xFFFFFFFF
ALLOW_ANYHIT = 0x10
CHUNK = 1 << 16              # paths traced together
FIXTURE = Path(__file__).resolve().parent / "golden" / "path_truth.json"


def _dot(a, b):
    return (a * b).sum(-1)


def _ph(a, b):
    """The power heuristic a^2 / (a^2 + b^2); 0 where both are 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        w = a * a / (a * a + b * b)
    return np.where((a == 0) & (b == 0), 0.0, w)


def delta_lobes_many(mat, wo, L=None):
    """`bsdf_ref.delta_lobes` for (N, 3) wo of one material: a list of (wi (N, 3), f-weight (N, 3),
    probability (N,)); a lobe that does not exist for a row has probability 0 there. Built from the
    same Fresnel terms (and, for a smooth plastic's coat weight, the same table lookup: L are the
    tables); tests/test_path_ref.py holds it to the scalar definition row by row."""
    wo = np.asarray(wo, np.float64)
    t = mat["type"]
    inside = wo[:, 2] < 0
    c = np.abs(wo[:, 2])
    mirror = wo * np.array([-1.0, -1.0, 1.0])
    ior = np.float64(mat["ior"][0])
    if t == R.CONDUCTOR:
        ok = ~inside | mat["two_sided"]
        with np.errstate(invalid="ignore", divide="ignore"):
            fw = R.fresnel_conductor(c, mat["ior"], mat["albedo"]) / c[:, None]
        return [(mirror, np.where(ok[:, None], fw, 0.0), ok.astype(np.float64))]
    if t == R.PLASTIC and R.is_smooth(mat):
        ok = ~inside | mat["two_sided"]
        coat = R.lut_brdf_dielectric(L, c, np.float64(mat["alpha"]), ior, False)
        with np.errstate(invalid="ignore", divide="ignore"):
            fw = R.fresnel_dielectric(c, 1.0, ior) / c
        return [(mirror, np.where(ok[:, None], np.repeat(fw[:, None], 3, 1), 0.0), np.where(ok, coat, 0.0))]
    if t not in (R.DIELECTRIC, R.THIN):
        return []
    thin = t == R.THIN
    swap = inside & (not thin)
    n_o, n_i = np.where(swap, ior, 1.0), np.where(swap, 1.0, ior)
    F = R.fresnel_dielectric(c, n_o, n_i)
    if thin:
        with np.errstate(invalid="ignore", divide="ignore"):
            F = np.where(F < 1, F + (1 - F) * (1 - F) * F / (1 - F * F), F)
    T = 1 - F
    with np.errstate(invalid="ignore", divide="ignore"):
        out = [(mirror, np.repeat((F / c)[:, None], 3, 1), F)]
        if thin:
            out.append((-wo, np.repeat(np.where(T > 0, T / c, 0.0)[:, None], 3, 1), T))
        else:
            eta = n_o / n_i
            ct = np.sqrt(np.maximum(1 - eta * eta * (1 - c * c), 0.0))
            wt = np.stack([-eta * wo[:, 0], -eta * wo[:, 1], np.where(inside, 1.0, -1.0) * ct], -1)
            out.append((wt, np.repeat(np.where(T > 0, T * eta * eta / ct, 0.0)[:, None], 3, 1), np.where(T > 0, T, 0.0)))
    return out


def visible_normal(wo, alpha, u):
    """A GGX normal drawn from the distribution of normals visible from wo (N, 3), wo.n > 0, with the numbers
    u (N, 2): Heitz 2018, listing 1 (stretch the view, draw a point of the projected disk, unstretch)."""
    vh = np.stack([alpha * wo[:, 0], alpha * wo[:, 1], wo[:, 2]], -1)
    vh /= np.sqrt(_dot(vh, vh))[:, None]
    lensq = vh[:, 0] ** 2 + vh[:, 1] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        t1 = np.where((lensq > 0)[:, None], np.stack([-vh[:, 1], vh[:, 0], 0 * lensq], -1) / np.sqrt(lensq)[:, None], np.array([1.0, 0.0, 0.0]))
    t2 = np.cross(vh, t1)
    r, phi = np.sqrt(u[:, 0]), 2 * np.pi * u[:, 1]
    a, b = r * np.cos(phi), r * np.sin(phi)
    sh = 0.5 * (1 + vh[:, 2])
    b = (1 - sh) * np.sqrt(np.maximum(0.0, 1 - a * a)) + sh * b
    nh = a[:, None] * t1 + b[:, None] * t2 + np.sqrt(np.maximum(0.0, 1 - a * a - b * b))[:, None] * vh
    m = np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.maximum(0.0, nh[:, 2])], -1)
    return m / np.sqrt(_dot(m, m))[:, None]


def dielectric_proposal(rng, luts, mat, wo):
    """This reference's proposal at a rough dielectric, wo (N, 3) all on one side: (wi, its density g). Half
    of the directions are uniform on the sphere (so g > 0 wherever any lobe is), half follow Walter's sampler
    of the single-scattering BSDF -- a visible normal, reflected about with probability F and refracted
    through otherwise -- whose density bsdf_ref states (`sampled_density` of the material without
    multiscattering: no QUIRK Q1 in it, F and 1 - F). f |cos| / g then stays bounded along a chain of
    vertices inside a solid, where the uniform proposal alone leaves a heavy tail. tests/test_path_ref.py
    checks that the directions follow g."""
    n = len(wo)
    z = rng.random((n, 4))
    cz = 1 - 2 * z[:, 0]
    sr = np.sqrt(np.maximum(0.0, 1 - cz * cz))
    wi = np.stack([sr * np.cos(2 * np.pi * z[:, 1]), sr * np.sin(2 * np.pi * z[:, 1]), cz], -1)
    inside = bool((wo[:, 2] < 0).all())
    flip = np.array([1.0, 1.0, -1.0 if inside else 1.0])
    w = wo * flip
    ior = np.float64(mat["ior"][0])
    n_o, n_i = (ior, 1.0) if inside else (1.0, ior)
    m = visible_normal(w, np.float64(mat["alpha"]), z[:, 0:2])
    c = _dot(w, m)
    eta = n_o / n_i
    k = 1 - eta * eta * (1 - c * c)
    reflect = z[:, 3] < R.fresnel_dielectric(c, n_o, n_i)              # (1 beyond the critical angle)
    walter = np.where(reflect[:, None], 2 * c[:, None] * m - w, -eta * w + (eta * c - np.sqrt(np.maximum(k, 0.0)))[:, None] * m) * flip
    wi = np.where((z[:, 2] < 0.5)[:, None], wi, walter)
    single = dict(mat, multiscattering=False)
    return wi, 0.5 / (4 * np.pi) + 0.5 * R.sampled_density(luts, single, wi, wo)


class PathRef:
    """The estimator over one flat scene (a dcrt_flat_scene), one frame (a dcrt_frame_params) and the
    BxDF tables (the arrays of tests/golden/bxdf_luts.npz)."""

    def __init__(self, flat, frame, lut_arrays, mis_model=True, shared_opacity_draw=True):
        import ctypes as C
        self.s = S.from_flat(flat)
        self.frame = S.frame_dict(frame)
        self.features = int(frame.features)
        self.light_count = int(frame.light_count)
        self.env_light = int(frame.environment_light_index)
        self.luts = R.Luts(lut_arrays)
        self.mis_model, self.shared = mis_model, shared_opacity_draw
        nodes = S._array(flat.bvh_nodes, C.c_uint32, (flat.bvh_node_count, 8))
        per_inst = RT.instance_triangles(nodes)
        self.inst = np.concatenate([np.full(len(p), i, np.int64) for i, p in per_inst])
        self.prim = np.concatenate([np.asarray(p, np.int64) for _, p in per_inst])
        P = self.s["vertices"][self.s["triangles"][self.prim]][..., 0:3].astype(np.float64)
        M = self.s["transforms"][self.inst]
        self.W = np.stack([S.to_world(M, P[:, k], 1, np.float64) for k in range(3)], 1)       # (pairs, 3, 3)
        self.anyhit = bool(self.features & ALLOW_ANYHIT)
        self.opacity = RT.Opacity(flat) if self.anyhit else None
        kinds = S.light_kind(self.s["lights"][:self.light_count]) if self.light_count else np.zeros(0, np.int64)
        self.delta_lights = [int(i) for i in np.flatnonzero((kinds == S.POINT) | (kinds == S.DIRECTIONAL))]
        self.kinds = kinds

    # ---- casts --------------------------------------------------------------------------------------
    def _candidates(self, o, d, t_max):
        """t, u, v (N, pairs) of every pair, inf where the ray does not hit inside (T_MIN, t_max)."""
        t, u, v = RT.moller_trumbore(o[:, None], d[:, None], self.W[None, :, 0], self.W[None, :, 1], self.W[None, :, 2])
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(t) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > T_MIN) & (t < t_max[:, None])
        return np.where(ok, t, np.inf), u, v

    def _opacities(self, t, u, v):
        """The opacity of every finite candidate (N, pairs); 1 on OPAQUE instances."""
        O = self.opacity
        a = np.ones(t.shape)
        r, c = np.nonzero(np.isfinite(t))
        if len(r):
            inst, prim = self.inst[c], self.prim[c]
            mat = O.material(inst, prim)
            val = O.value(mat, u[r, c], v[r, c], O.tc32[prim].astype(np.float64), O.tiling32[mat].astype(np.float64),
                          O.opacity32[mat].astype(np.float64))
            a[r, c] = np.where(O.opaque[inst], 1.0, val)
        return a

    def nearest(self, rng, o, d):
        """The accepted nearest hit: (hit, t, u, v, pair)."""
        t, u, v = self._candidates(o, d, np.full(len(o), np.inf))
        if self.anyhit:
            a = self._opacities(t, u, v)
            draw = rng.random((len(o), 1)) if self.shared else rng.random(t.shape)
            t = np.where(draw < a, t, np.inf)
        k = t.argmin(1)
        rows = np.arange(len(o))
        tt = t[rows, k]
        return np.isfinite(tt), tt, u[rows, k], v[rows, k], k

    def transmittance(self, o, d, t_max):
        """The chance that a shadow ray passes every crossing before t_max."""
        t, u, v = self._candidates(o, d, t_max)
        if not self.anyhit:
            return (~np.isfinite(t).any(1)).astype(np.float64)
        a = np.where(np.isfinite(t), self._opacities(t, u, v), 0.0)
        return 1.0 - a.max(1) if self.shared else np.prod(1.0 - a, 1)

    # ---- materials ----------------------------------------------------------------------------------
    def _material(self, mid, h, rows):
        """The bsdf_ref material of hits `rows` (all of material mid; one alpha: no roughness texture here)."""
        matf = self.s["materials"][mid].view(np.float32)
        flags = int(self.s["materials"][mid][11])
        assert not flags & S.ROUGHNESS_TEXTURE, "roughness textures are not covered"
        t = flags & 0xF
        # (a diffuse material has no alpha; bsdf_ref's probe materials give it one, and `sampled_density` reads it)
        alpha = np.float32(1.0 if t == R.DIFFUSE else h["alpha"][rows[0]])
        m = R.material(t, albedo=(1, 1, 1), alpha=alpha, ior=matf[4:7], two_sided=bool(flags & S.TWO_SIDED),
                       multiscattering=bool(flags & S.MULTISCATTERING), internal_scattering=(flags >> 8) & 3)
        m["albedo"] = h["albedo"][rows]          # per hit: the texture is in it (a conductor's k is constant)
        if t == R.CONDUCTOR:
            m["albedo"] = matf[0:3].copy()
        return m

    # ---- the estimator -------------------------------------------------------------------------------
    def radiance(self, rng, film, aperture, bounces):
        """Per path and per B of `bounces`: (N, len(bounces), 3) radiance without the k = 0 emission,
        and that emission (N, 3)."""
        N = len(film)
        bounces = np.asarray(bounces)
        L = np.zeros((N, len(bounces), 3))
        L0 = np.zeros((N, 3))
        o, d, _, _ = S.camera_ray(self.frame, film, aperture, np.float64)
        alive = np.arange(N)
        T = np.ones((N, 3))                       # throughput of what is not emission at the next vertex
        Te = np.ones((N, 3))                      # throughput without the factor that W replaces
        q = np.zeros(N)                           # the previous vertex's reported pdf, its sampled density,
        sdens = np.zeros(N)                       # and whether its lobe was a delta
        delta = np.ones(N, bool)
        s, lc = self.s, self.light_count
        for k in range(int(bounces.max()) + 2):
            if not len(alive):
                break
            emits = bounces >= k - 1              # the B for which vertex k's emission counts
            shades = bounces >= k                 # and for which vertex k is shaded
            hit, t, u, v, pair = self.nearest(rng, o, d)
            # -- emission
            li = np.full(len(alive), NO_LIGHT, np.int64)
            inst, prim = self.inst[pair], self.prim[pair]
            h = S.hit(s, u, v, prim, inst, np.float64) if len(alive) else None
            li[hit] = h["light_index"][hit]
            if self.env_light != NO_LIGHT:
                li[~hit] = self.env_light
            e = np.flatnonzero(li != NO_LIGHT)
            if len(e) and lc:
                rad, p = S.evaluate_light(s, lc, li[e], prim[e], h["geometry_normal"][e], d[e], np.where(hit[e], t[e], np.inf), np.float64)
                if k == 0:
                    L0[alive[e]] = rad
                else:
                    if self.mis_model:
                        ps = np.where(self.kinds[li[e]] == S.MESH, 2.0 * p, p)
                        with np.errstate(invalid="ignore", divide="ignore"):
                            m = _ph(ps, q[e]) * np.where(ps > 0, p / ps, 0.0) + np.where(q[e] > 0, _ph(q[e], p) * sdens[e] / q[e], 0.0)
                    else:
                        m = np.ones(len(e))
                    W = np.where(delta[e], 1.0, m)
                    L[alive[e][:, None], np.flatnonzero(emits)[None, :]] += (Te[e] * rad * W[:, None])[:, None, :]
            if not shades.any():
                break
            keep = np.flatnonzero(hit)
            alive, o, d, T, t = alive[keep], o[keep], d[keep], T[keep], t[keep]
            h = {key: val[keep] for key, val in h.items() if isinstance(val, np.ndarray)}
            n = len(alive)
            if not n:
                break
            # (the point on the ray: `hit` takes its barycentrics as the float32 of a hit record, 1e-7 away)
            pos, ns, tg = o + t[:, None] * d, h["normal"], h["tangent"]
            bt = np.cross(ns, tg)
            local = lambda w: np.stack([_dot(w, tg), _dot(w, bt), _dot(w, ns)], -1)
            world = lambda w: w[:, 0:1] * tg + w[:, 1:2] * bt + w[:, 2:3] * ns
            wo = local(-d)
            new_d, fcos_g = np.zeros((n, 3)), np.zeros((n, 3))
            q, sdens, delta = np.zeros(n), np.zeros(n), np.zeros(n, bool)
            direct = np.zeros((n, 3))
            for mid in np.unique(h["material"]):
                for side in (wo[:, 2] > 0, wo[:, 2] < 0):
                    rows = np.flatnonzero((h["material"] == mid) & side)
                    if not len(rows):
                        continue
                    mat = self._material(int(mid), h, rows)
                    smooth = mat["type"] == R.THIN or (mat["type"] in (R.CONDUCTOR, R.DIELECTRIC) and R.is_smooth(mat))
                    if smooth:
                        lobes = delta_lobes_many(mat, wo[rows])
                        if not lobes:
                            continue
                        prob = np.stack([l[2] for l in lobes], 1)
                        pick = (rng.random(len(rows))[:, None] >= np.cumsum(prob, 1)[:, :-1]).sum(1) if prob.shape[1] > 1 else np.zeros(len(rows), np.int64)
                        r = np.arange(len(rows))
                        wi = np.stack([l[0] for l in lobes], 1)[r, pick]
                        fw = np.stack([l[1] for l in lobes], 1)[r, pick]
                        pr = prob[r, pick]
                        with np.errstate(invalid="ignore", divide="ignore"):
                            fcos_g[rows] = np.where(pr[:, None] > 0, fw * np.abs(wi[:, 2:3]) / pr[:, None], 0.0)
                        new_d[rows], delta[rows], q[rows], sdens[rows] = wi, True, 1.0, 1.0
                        continue
                    # -- delta lights, exactly (a delta lobe sees none)
                    for dl in self.delta_lights:
                        Lf = s["lights"][dl].view(np.float32)
                        if self.kinds[dl] == S.POINT:
                            w = Lf[3:6].astype(np.float64) - pos[rows]
                            dist = np.sqrt(_dot(w, w))
                            w = w / dist[:, None]
                            Le = Lf[0:3].astype(np.float64) / (dist * dist)[:, None]
                            reach = dist * (1.0 - float(S.SHADOW_EPSILON))
                        else:
                            w = np.repeat(-Lf[3:6].astype(np.float64)[None], len(rows), 0)
                            Le = np.repeat(Lf[0:3].astype(np.float64)[None], len(rows), 0)
                            reach = np.full(len(rows), np.inf)
                        wl = np.stack([_dot(w, tg[rows]), _dot(w, bt[rows]), _dot(w, ns[rows])], -1)
                        f, _ = R.evaluate(self.luts, mat, wl, wo[rows])
                        lit = f.any(1)
                        tr = np.zeros(len(rows))
                        if lit.any():
                            tr[lit] = self.transmittance(pos[rows][lit], w[lit], reach[lit])
                        direct[rows] += f * np.abs(wl[:, 2:3]) * Le * tr[:, None]
                    # -- the continuation's proposal
                    mixed = mat["type"] == R.PLASTIC and R.is_smooth(mat)
                    if mat["type"] == R.DIELECTRIC:
                        wi, g = dielectric_proposal(rng, self.luts, mat, wo[rows])
                    else:
                        z = rng.random((len(rows), 2))
                        sr = np.sqrt(z[:, 0])
                        cz = np.sqrt(np.maximum(0.0, 1 - z[:, 0])) * np.sign(wo[rows, 2])
                        wi = np.stack([sr * np.cos(2 * np.pi * z[:, 1]), sr * np.sin(2 * np.pi * z[:, 1]), cz], -1)
                        g = np.abs(cz) / np.pi
                    f, qq = R.evaluate(self.luts, mat, wi, wo[rows])
                    ss = R.sampled_density(self.luts, mat, wi, wo[rows])
                    with np.errstate(invalid="ignore", divide="ignore"):
                        fc = np.where(g[:, None] > 0, f * np.abs(wi[:, 2:3]) / g[:, None], 0.0)
                    if mixed:
                        # a mixed vertex: the coat's delta lobe with a probability P of this reference's choosing
                        # (its weight in the sampler will do: 0 where there is no coat, never 1), the Lambert
                        # base by the cosine proposal otherwise
                        (cwi, cfw, P), = delta_lobes_many(mat, wo[rows], self.luts)
                        coat = rng.random(len(rows)) < P
                        with np.errstate(invalid="ignore", divide="ignore"):
                            fc = np.where(coat[:, None], cfw * np.abs(cwi[:, 2:3]) / P[:, None], fc / (1.0 - P)[:, None])
                        wi, qq, ss = np.where(coat[:, None], cwi, wi), np.where(coat, 1.0, qq), np.where(coat, 1.0, ss)
                        delta[rows] = coat
                    fcos_g[rows] = fc
                    new_d[rows], q[rows], sdens[rows] = wi, qq, ss
            L[alive[:, None], np.flatnonzero(shades)[None, :]] += (T * direct)[:, None, :]
            Te = T * fcos_g
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(delta, 1.0, np.where(q > 0, sdens / q, 0.0))
            T = Te * ratio[:, None]
            go = np.flatnonzero(Te.any(1))
            alive, T, Te, q, sdens, delta = alive[go], T[go], Te[go], q[go], sdens[go], delta[go]
            o, d = pos[go], world(new_d)[go]
        return L, L0

    def region_statistics(self, seed, paths, bounces, regions=2, log=None):
        """Paths spread uniformly over the film; per region (regions x regions, row-major), B and channel
        the mean, its standard error and the path count, with and without LIGHT_VISIBLE's k = 0 term:
        {"visible": {...}, "hidden": {...}}, arrays (len(bounces), regions^2, 3)."""
        rng = np.random.default_rng(seed)
        nb, nr = len(bounces), regions * regions
        s1 = {v: np.zeros((nb, nr, 3)) for v in ("visible", "hidden")}
        s2 = {v: np.zeros((nb, nr, 3)) for v in ("visible", "hidden")}
        count = np.zeros(nr, np.int64)
        done = 0
        while done < paths:
            n = min(CHUNK, paths - done)
            film, ap = rng.random((n, 2)), rng.random((n, 3))
            L, L0 = self.radiance(rng, film, ap, bounces)
            reg = np.minimum((film[:, 1] * regions).astype(np.int64), regions - 1) * regions + np.minimum((film[:, 0] * regions).astype(np.int64), regions - 1)
            count += np.bincount(reg, minlength=nr)
            for name, x in (("hidden", L), ("visible", L + L0[:, None, :])):
                for r in range(nr):
                    sel = x[reg == r]
                    s1[name][:, r] += sel.sum(0)
                    s2[name][:, r] += (sel * sel).sum(0)
            done += n
            if log:
                log(f"  {done} / {paths}")
        out = {}
        for name in s1:
            c = count[None, :, None]
            mean = s1[name] / c
            var = np.maximum(s2[name] / c - mean * mean, 0.0)
            out[name] = {"mean": mean, "sem": np.sqrt(var / c), "count": count.copy()}
        return out


def quadrant_statistics(samples, regions=2):
    """The device / oracle side: samples (images, H, W, 3) -> mean, standard error (regions^2, 3), sample
    counts and the NaN share. A sample with a NaN channel is dropped (the caller caps the share)."""
    v = np.asarray(samples, np.float64)
    _, H, W, _ = v.shape
    mean, sem, count = np.zeros((regions * regions, 3)), np.zeros((regions * regions, 3)), np.zeros(regions * regions, np.int64)
    bad = np.isnan(v).any(-1)
    for r in range(regions * regions):
        ry, rx = divmod(r, regions)
        ys, xs = slice(ry * H // regions, (ry + 1) * H // regions), slice(rx * W // regions, (rx + 1) * W // regions)
        x = v[:, ys, xs][~bad[:, ys, xs]]
        mean[r], sem[r], count[r] = x.mean(0), x.std(0) / np.sqrt(len(x)), len(x)
    return mean, sem, count, bad.mean()


def load_fixture():
    return json.loads(FIXTURE.read_text())


def fixture_entry(fx, scene, visible, bounce):
    """(mean, sem) arrays (regions^2, 3) of one case."""
    e = fx["scenes"][scene]["cases"]["visible" if visible else "hidden"][str(bounce)]
    return np.array(e["mean"]), np.array(e["sem"])


def scene_statistics(name, paths, seed):
    """`region_statistics` of one scene of tests/path_scenes.py, every B and LIGHT_VISIBLE state of it."""
    import tempfile
    import path_scenes as PS
    luts = dict(np.load(FIXTURE.parent / "bxdf_luts.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        scene = PS.load(name, tmp)
        ref = PathRef(scene.flat(), scene.frame_params(0), luts)
        return ref.region_statistics(seed, paths, PS.SCENES[name]["bounces"])


def _fixture_scene(name):
    import path_scenes as PS
    spec = PS.SCENES[name]
    seed = PS.SEED + list(PS.SCENES).index(name)
    t0 = time.time()
    st = scene_statistics(name, spec["paths"], seed)
    cases = {}
    for vis in spec["visible"]:
        key = "visible" if vis else "hidden"
        cases[key] = {str(b): {"mean": st[key]["mean"][j].round(9).tolist(), "sem": st[key]["sem"][j].round(9).tolist()}
                      for j, b in enumerate(spec["bounces"])}
    return name, {"paths": spec["paths"], "seed": seed, "count": st["visible"]["count"].tolist(), "seconds": round(time.time() - t0, 1),
                  "cases": cases}


def main(argv):
    """python tests/path_ref.py --write [scene ...]: recompute tests/golden/path_truth.json (all scenes, or
    the named ones, keeping the others), one process per scene."""
    if "--write" not in argv:
        print(main.__doc__)
        return 1
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import multiprocessing
    import path_scenes as PS
    names = [a for a in argv if not a.startswith("--")] or list(PS.SCENES)
    fx = load_fixture() if FIXTURE.exists() else {"seed": PS.SEED, "regions": 2, "resolution": [PS.SIZE, PS.SIZE], "scenes": {}}
    with multiprocessing.get_context("spawn").Pool(min(len(names), 8)) as pool:
        for name, entry in pool.imap_unordered(_fixture_scene, names):
            print(name, entry["seconds"], "s", flush=True)
            fx["scenes"][name] = entry
    fx["scenes"] = {n: fx["scenes"][n] for n in PS.SCENES if n in fx["scenes"]}
    FIXTURE.write_text(json.dumps(fx, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
