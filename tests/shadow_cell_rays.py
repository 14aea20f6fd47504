"""Scenes and shadow rays for the direction-cell tests (test infrastructure, not part of the product).

Scenes: the Cornell box, and seeded rooms of axis-aligned and rotated boxes and loose quads (at
most 64 triangles, identity instances, one point light). Rays: built the way MATERIAL builds a
shadow ray -- P, OffsetRayOrigin(P), wi = (L - P) / |L - P|, tMax = |L - P|, every step in float32 --
from points on random triangles, from points aimed within 0..4 ulps of every triangle edge and
vertex (the boxes' silhouettes among them), and from points that give one or two direction
components exactly 0. The float32 slab and watertight tests restate dscene.h ray_aabb_raw /
tri_watertight_rot operation for operation (numpy rounds every operation; no contraction)."""
import math
from pathlib import Path

import numpy as np

from directcomputeraytracing_amd import Scene, scenes
from directcomputeraytracing_amd.tracer import RAY_DTYPE

F = np.float32
RAYS_PER_SCENE = 200_000

_MTL = "newmtl a\nKd 0.7 0.7 0.7\nNi 1.0\nnewmtl b\nKd 0.6 0.2 0.2\nNi 1.5\nPr 0.3\n"


def _quad(p, e0, e1, normal):
    p, e0, e1 = np.asarray(p, float), np.asarray(e0, float), np.asarray(e1, float)
    return [([tuple(p), tuple(p + e0), tuple(p + e0 + e1), tuple(p + e1)], tuple(normal))]


def room_groups(seed: int, boxes: int | None = None, quads: int | None = None):
    """(groups as scenes.cornell_groups, light position, triangle count)."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1, z0, z1 = -1.5, 1.5, 0.0, float(rng.choice([2.0, 2.25])), 1.0, 4.5
    groups = [
        ("floor", "a", _quad((x0, y0, z0), (x1 - x0, 0, 0), (0, 0, z1 - z0), (0, 1, 0))),
        ("ceiling", "a", _quad((x0, y1, z0), (0, 0, z1 - z0), (x1 - x0, 0, 0), (0, -1, 0))),
        ("back", "a", _quad((x0, y0, z1), (x1 - x0, 0, 0), (0, y1 - y0, 0), (0, 0, -1))),
        ("left", "b", _quad((x0, y0, z0), (0, 0, z1 - z0), (0, y1 - y0, 0), (1, 0, 0))),
        ("right", "b", _quad((x1, y0, z0), (0, y1 - y0, 0), (0, 0, z1 - z0), (-1, 0, 0))),
    ]
    n_boxes = int(rng.integers(1, 5)) if boxes is None else boxes
    tops = []
    for k in range(n_boxes):
        cx, cz = float(rng.uniform(-1.0, 1.0)), float(rng.uniform(1.8, 4.0))
        sx, sy, sz = (float(v) for v in rng.uniform([0.3, 0.3, 0.3], [0.9, 1.5, 0.9]))
        aligned = rng.random() < 0.4
        angle = 0.0 if aligned else math.radians(float(rng.uniform(-40, 40)))
        groups.append((f"box{k}", "b" if k & 1 else "a", scenes._box_faces(cx, cz, sx, sy, sz, angle)))
        if aligned:
            tops.append((cx, cz, sx, sy, sz))
    n_quads = int(rng.integers(0, 5)) if quads is None else quads
    for k in range(n_quads):
        p = rng.uniform([-1.2, 0.2, 1.4], [0.8, 1.6, 3.9])
        e0, e1 = rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.5, 0.5, 3)
        groups.append((f"quad{k}", "a", _quad(p, e0, e1, np.cross(e0, e1) / max(np.linalg.norm(np.cross(e0, e1)), 1e-9))))
    light = rng.uniform([-1.0, 1.0, 1.5], [1.0, y1 - 0.15, 4.0])
    if tops and seed % 3 == 0:
        # a light in the plane of an axis-aligned box's top and on the line of one of its sides,
        # beside the box: rays with a zero direction component then run in those planes
        cx, cz, sx, sy, sz = tops[0]
        light = np.array([float(f"{cx + sx / 2:.6f}"), float(f"{sy:.6f}"), float(f"{cz + sz / 2:.6f}") + 0.4])   # (as the OBJ's text)
    light = np.asarray(light, np.float32)
    triangles = 2 * sum(len(q) for _, _, q in groups)
    return groups, tuple(float(v) for v in light), triangles


def write_obj(directory, groups) -> Path:
    """The groups in the OBJ dialect of scenes.cornell_obj_text (x mirrored on import)."""
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    lines = ["mtllib room.mtl"]
    vi = vti = vni = 0
    for name, mat, quads in groups:
        lines += [f"g {name}", f"usemtl {mat}"]
        for quad, normal in quads:
            for (x, y, z) in quad:
                lines.append(f"v {-x:.6f} {y:.6f} {z:.6f}")
            lines += [f"vt {s} {t}" for s, t in ((0, 0), (1, 0), (1, 1), (0, 1))]
            nx, ny, nz = normal
            lines.append(f"vn {-nx:.6f} {ny:.6f} {nz:.6f}")
            idx = [f"{vi + k + 1}/{vti + k + 1}/{vni + 1}" for k in range(4)]
            lines += [f"f {idx[0]} {idx[2]} {idx[1]}", f"f {idx[0]} {idx[3]} {idx[2]}"]
            vi += 4; vti += 4; vni += 1
    (d / "room.mtl").write_text(_MTL)
    (d / "room.obj").write_text("\n".join(lines) + "\n")
    return d / "room.obj"


def room_scene(directory, seed: int, **kw):
    """(scene, light position) of seeded room `seed`."""
    groups, light, _ = room_groups(seed, **kw)
    s = Scene((32, 24))
    s.reset(32, 24)
    s.load_from_file(write_obj(directory, groups))
    s.add_point_light(light, (2.0, 2.0, 2.0))
    s.set_max_bounce(3)
    s.flatten()
    return s, light


def cornell_scene():
    s = Scene((32, 24))
    scenes.setup_cornell(s, 32, 24, 3)
    s.flatten()
    return s, scenes.POINT_LIGHT_POSITION


def scene_triangles(scene) -> np.ndarray:
    """[T, 3, 3] float32 world positions (identity instances)."""
    a = scene.arrays()
    return a["vertices"][:, :3][a["triangles"].astype(np.int64)].astype(F)


# ---- MATERIAL's shadow ray, float32 -------------------------------------------------------------
def offset_ray_origin(p, n, d):
    """dmath.h offset_ray_origin on [n, 3] float32 arrays."""
    dot = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    n = (n * np.sign(dot).astype(F)[:, None]).astype(F)
    of = (F(256.0) * n).astype(np.int32)                      # (truncates, as the C cast)
    moved = (p.view(np.uint32) + np.where(p < 0, -of, of).astype(np.uint32)).view(F)
    return np.where(np.abs(p) < F(1.0 / 32.0), p + F(1.0 / 65536.0) * n, moved).astype(F)


def shadow_rays(p, n, light) -> np.ndarray:
    p, n = np.ascontiguousarray(p, F), np.ascontiguousarray(n, F)
    wi = (np.asarray(light, F)[None, :] - p).astype(F)
    dist = np.sqrt((wi[:, 0] * wi[:, 0] + wi[:, 1] * wi[:, 1]) + wi[:, 2] * wi[:, 2]).astype(F)
    wi = (wi / dist[:, None]).astype(F)
    keep = np.isfinite(wi).all(1) & (dist > 0)
    p, n, wi, dist = p[keep], n[keep], wi[keep], dist[keep]
    r = np.zeros(len(p), RAY_DTYPE)
    r["origin"] = offset_ray_origin(p, n, wi)
    r["direction"] = wi
    r["t_max"] = dist
    return r


def _normals(tri):
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
    return (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)).astype(F)


def ray_set(scene, light, seed: int, count: int = RAYS_PER_SCENE) -> np.ndarray:
    rng = np.random.default_rng(seed)
    tri = scene_triangles(scene)
    nrm = _normals(tri)
    L = np.asarray(light, F)
    n_surface, n_edge = int(count * 0.6), int(count * 0.3)
    # points on random triangles
    t = rng.integers(0, len(tri), n_surface)
    u, v = rng.random(n_surface), rng.random(n_surface)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u).astype(F), np.where(flip, 1 - v, v).astype(F)
    p = (tri[t, 0] + (tri[t, 1] - tri[t, 0]) * u[:, None] + (tri[t, 2] - tri[t, 0]) * v[:, None]).astype(F)
    sets = [shadow_rays(p, nrm[t], L)]
    # points on the line from the light through a spot within 0..4 ulps of an edge or a vertex
    t = rng.integers(0, len(tri), n_edge)
    e = rng.integers(0, 3, n_edge)
    w = np.where(rng.random(n_edge) < 0.3, rng.integers(0, 2, n_edge).astype(float), rng.random(n_edge)).astype(F)
    a, b = tri[t, e], tri[t, (e + 1) % 3]
    q = (a + (b - a) * w[:, None]).astype(F)
    q = (q + rng.integers(-4, 5, q.shape).astype(F) * np.spacing(np.abs(q))).astype(F)
    s = np.where(rng.random(n_edge) < 0.25, 1.0, rng.uniform(1.0, 2.5, n_edge)).astype(F)
    p = (L[None, :] + (q - L[None, :]) * s[:, None]).astype(F)
    sets.append(shadow_rays(p, nrm[rng.integers(0, len(tri), n_edge)], L))
    # one or two direction components exactly 0: P differs from the light along one or two axes
    n_zero = count - n_surface - n_edge
    axes = np.zeros((n_zero, 3))
    first = rng.integers(0, 3, n_zero)
    axes[np.arange(n_zero), first] = rng.choice([-1.0, 1.0], n_zero) * rng.uniform(0.1, 3.0, n_zero)
    second = (first + rng.integers(1, 3, n_zero)) % 3
    two = rng.random(n_zero) < 0.6
    axes[np.arange(n_zero)[two], second[two]] = (rng.choice([-1.0, 1.0], n_zero) * rng.uniform(0.1, 3.0, n_zero))[two]
    p = (L[None, :] + axes.astype(F)).astype(F)
    n = (axes / np.linalg.norm(axes, axis=1, keepdims=True)).astype(F)
    sets.append(shadow_rays(p, n, L))
    return np.concatenate(sets)


# ---- dscene.h ray_aabb_raw / tri_watertight_rot, float32 ------------------------------------------
def inv_dir(d):
    with np.errstate(divide="ignore"):
        return (F(1.0) / d).astype(F)


def slab(o, inv, t_max, box):
    """ray_aabb_raw with tMin = 0 on [n, 3] rays and one box (min xyz, max xyz)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = t1 = None
        for a in range(3):
            ta = ((box[a] - o[:, a]) * inv[:, a]).astype(F)
            tb = ((box[3 + a] - o[:, a]) * inv[:, a]).astype(F)
            lo, hi = np.fmin(ta, tb), np.fmax(ta, tb)
            t0 = lo if t0 is None else np.fmax(t0, lo)
            t1 = hi if t1 is None else np.fmin(t1, hi)
        return (t1 >= t0) & (t0 < t_max) & (t1 >= 0)


def shear(d, inv):
    ad = np.abs(d)
    z = np.where(ad[:, 0] >= ad[:, 1], 0, 1)
    z = np.where(np.where(z == 0, ad[:, 0], ad[:, 1]) >= ad[:, 2], z, 2)
    x = (z + 1) % 3
    y = (x + 1) % 3
    i = np.arange(len(d))
    inv_z = inv[i, z]
    with np.errstate(invalid="ignore", over="ignore"):
        return x, y, z, (-d[i, x] * inv_z).astype(F), (-d[i, y] * inv_z).astype(F), inv_z


def watertight(o, d, inv, t_max, tri):
    """tri_watertight_rot (tMin = 0) on [n, 3] rays and one triangle [3, 3]; the degenerate flag as
    build_tri_verts_kernel computes it."""
    e1, e2 = (tri[1] - tri[0]).astype(F), (tri[2] - tri[0]).astype(F)
    cp = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], F)
    if F(F(cp[0] * cp[0] + cp[1] * cp[1]) + cp[2] * cp[2]) == 0:
        return np.zeros(len(o), bool)
    o = (o + F(0.0)).astype(F)
    d = (d + F(0.0)).astype(F)
    x, y, z, sx, sy, sz = shear(d, inv)
    i = np.arange(len(o))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = [(tri[k][None, :] - o).astype(F) for k in range(3)]
        px = [(p[k][i, x] + sx * p[k][i, z]).astype(F) for k in range(3)]
        py = [(p[k][i, y] + sy * p[k][i, z]).astype(F) for k in range(3)]
        pz = [p[k][i, z] for k in range(3)]
        e0 = (px[1] * py[2] - px[2] * py[1]).astype(F)
        e1 = (px[2] * py[0] - px[0] * py[2]).astype(F)
        e2 = (px[0] * py[1] - px[1] * py[0]).astype(F)
        mixed = ((e0 < 0) | (e1 < 0) | (e2 < 0)) & ((e0 > 0) | (e1 > 0) | (e2 > 0))
        det = ((e0 + e1) + e2).astype(F)
        pz = [(pz[k] * sz).astype(F) for k in range(3)]
        t_scaled = ((e0 * pz[0] + e1 * pz[1]) + e2 * pz[2]).astype(F)
        t = (t_scaled * (F(1.0) / det).astype(F)).astype(F)
        return ~mixed & (det != 0) & (t >= 0) & (t < t_max)


def leaves_of(table):
    """Per leaf of the table: (box [6], triangle index, [guard boxes])."""
    nodes = table["nodes"]
    boxes = nodes[:, :6].view(F)
    words = table["leaf_words"]
    out = []
    for k in range(table["leaf_count"]):
        w = int(words[k])
        node, count, first = w & 1023, (w >> 10) & 63, w >> 16
        out.append((boxes[node], int(nodes[node, 6]), [boxes[int(g)] for g in words[first:first + count]]))
    return out
