"""A float64 reference of the stages between the ray casts and the BSDF -- camera rays, hit
reconstruction with its texture and environment lookups, light sampling and evaluation -- written
from definitions and not from the product's code (csrc/device/kernels.h, dscene.h) or the CPU oracle:
tests/test_shading_ref.py holds the oracle to it, and tests/test_gpu_shading_ref.py the device.

Definitions
  * Camera: a film of film_size at distance film_distance behind a pinhole at the camera-space origin,
    looking down +z; film sample (sx, sy) in [0, 1]^2 is the film point ((0.5 - sx) W, (sy - 0.5) H,
    -film_distance), and its ray leaves the pinhole away from it. A thin lens (aperture_radius > 0)
    sends every ray of one film point through the point where the pinhole ray meets the plane
    z = focal_distance; the ray starts at a point of the aperture in the plane z = 0. The aperture is
    the disk of radius aperture_radius (blade_count <= 2; Shirley & Chiu's concentric map of the unit
    square, "A Low Distortion Map Between Disk and Square", 1997: density 1 / (pi R^2)) or the regular
    n-gon whose vertices lie at the polar angles aperture_base_angle + (2k +- 1) pi / n on the circle
    through blade_vertex_pos (density 1 / (n/2 R^2 sin(2 pi / n))): blade k = floor(a2 n) is the
    triangle (centre, vertex at -pi/n, vertex at +pi/n) turned by k 2 pi / n + base angle, and the
    point in it has the uniform-triangle barycentrics of (a0, a1) below. Camera to world:
    camera_transform as include/dcrt.h lays it out, a row-major 4x4 with the translation in row 3,
    applied to row vectors.
  * Uniform triangle sampling (Osada et al. 2002; PBRT 13.6.5): (u, v) = (1 - sqrt(s0), s1 sqrt(s0)),
    the point p0 + u (p1 - p0) + v (p2 - p0), density 1 / area.
  * Uniform sphere: z = 1 - 2 s0, phi = 2 pi s1, density 1 / (4 pi).
  * Hit reconstruction: barycentric position p0 + u (p1 - p0) + v (p2 - p0); the interpolated,
    renormalised normal; the interpolated tangent made orthogonal to it (Gram-Schmidt) and normalised;
    the geometry normal cross(p2 - p0, p1 - p0) normalised (the winding's); all moved to world space
    with the instance's forward float4x3 (include/dcrt.h: m[c * 4 + r], row-vector convention).
    The material is the instance's override, or the triangle's; the texcoord is interpolated and
    multiplied by tex_tiling; the albedo is multiplied by the bilinear, wrap-addressed texel (D3D
    functional spec 7.18.8: texel centres at (i + 0.5) / size), sRGB texels decoded before filtering
    (IEC 61966-2-1), an R8 texture read as (r, 0, 0, 1); alpha = roughness^2, the roughness
    multiplied by the checkerboard (floor(2 tcx) + floor(2 tcy)) & 1 where the material asks for it.
  * Environment cube: the D3D functional spec's face table (7.18.11): the face of the component of
    largest magnitude, (sc, tc, ma) = +x (-z, -y, x), -x (z, -y, x), +y (x, z, y), -y (x, -z, y),
    +z (x, -y, z), -z (-x, -y, z), (s, t) = ((sc / |ma| + 1) / 2, (tc / |ma| + 1) / 2), bilinear.
  * Lights: a point light's radiance / d^2 from direction (position - p) / d, density 1 (delta); a
    directional light's radiance from -direction at infinity (delta); the environment's lookup times
    its radiance from a uniform direction; a mesh light's radiance from a point drawn uniformly on a
    triangle picked uniformly BY COUNT (not by area) among the light's, at the solid-angle density
    d^2 / (A cos) / triangle count, A the world-space area and cos the angle at the light. Every
    density is divided by the light count (one light is picked uniformly), and a finite distance is
    shortened by the shadow epsilon 1e-3.

Where the reference renderer's arithmetic departs from the above, the renderer settles the behaviour
and this file states the departure (search for "QUIRK"):
  Q1  normals, tangents and light normals reach world space through the forward instance matrix,
      normalize(M n), not the inverse transpose (RayTracingCommon.inc.hlsl:112-115, Light.inc.hlsl:63):
      exact for rigid motions and uniform scale; off under non-uniform scale and shear (the shading
      frame and the cosine of the area-light pdf; `true_normal` gives the right one); under a mirror
      the emitting side follows the instance-space winding.
  Q2  bilinear taps of the environment cube are clamped inside the selected face (a Texture2D-style
      fetch per face), where D3D12 filters across face edges: the lookup is discontinuous at face
      boundaries. Ties between components go to x, then y, then z (the spec: z, y, x).
  Q3  the mesh-light sampler reports twice the solid-angle density: it halves the triangle's area
      twice (Light.inc.hlsl:51, :59); EvaluateLightDirect reports it once (Light.inc.hlsl:37-38).
  Q4  the "no area" threshold 1e-6 is applied to the area A by the sampler (Light.inc.hlsl:51, :59)
      and to 2 A by the evaluation (Light.inc.hlsl:37-38).
  Q5  the last tangent fallback divides (1, 0, 0) by the degenerate length it replaces
      (HitShader.inc.hlsl:49, :51): a normal exactly parallel to y with a degenerate tangent gives a
      non-finite tangent, and one within 1e-6 of it a tangent of the right direction.
  Q6  float -> uint of the checkerboard saturates: a negative texcoord is cell 0 (HitShader.inc.hlsl:11,
      D3D conversion rules).
  Q7  the selected light and triangle are floor(draw * count) evaluated in float32, the triangle index
      as float(offset) + floor(.) (RayTracingCommon.inc.hlsl:147, :166).
  Q8  every density, the delta lights' too, is divided by the light count (RayTracingCommon.inc.hlsl:182).

Discrete decisions -- the light, the triangle, the blade, the cube face of a given float32 direction --
are evaluated exactly as float32 does (one multiplication and a floor, or comparisons); everything
continuous is `dtype`. Bilinear filtering is continuous in the texcoord, so the texels are chosen in
`dtype`. Every function takes `dtype`: np.float64 is the reference, np.float32 runs the same formulas
in single precision and measures how much rounding the formulas themselves cost.
"""
import ctypes as C

import numpy as np

POINT, MESH, DIRECTIONAL, ENVIRONMENT = 1, 2, 4, 8
DRAWS = {POINT: 1, DIRECTIONAL: 1, MESH: 4, ENVIRONMENT: 3}     # numbers a light sample consumes
SHADOW_EPSILON = np.float32(1e-3)
DEGENERATE = 1e-6            # tangent lengths and light areas below it count as none
NO_OVERRIDE = 0xFFFFFFFF
ROUGHNESS_TEXTURE, TWO_SIDED, MULTISCATTERING = 0x20, 0x40, 0x80
U24 = 2.0 ** -24


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _normalize(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / _norm(a)[..., None]


# ---- xoshiro128** 1.0 (Blackman & Vigna), vectorised over (N, 4) uint32 states ----------------------
def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def xoshiro_next(states):
    """(outputs (N,), next states (N, 4)) of (N, 4) uint32 states."""
    s = np.array(states, np.uint32).reshape(-1, 4).T.copy()
    with np.errstate(over="ignore"):
        out = _rotl(s[0] * np.uint32(5), 7) * np.uint32(9)
        t = s[1] << np.uint32(9)
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 11)
    return out, s.T.copy()


def draws(states, count):
    """`count` uniform numbers per state, (N, count) float32 with 24 bits each, and the states after."""
    out = np.zeros((len(states), count), np.float32)
    for k in range(count):
        bits, states = xoshiro_next(states)
        out[:, k] = (bits >> np.uint32(8)).astype(np.float32) * np.float32(U24)
    return out, states


def states_with_draw(bits24, seed, which=0):
    """States whose first (which = 0) or second (1) number is bits24 / 2^24: the output function rotl(s0 * 5, 7) * 9
    inverted (9 and 5 are units modulo 2^32) gives the s0 that draws it; one step turns s0 into s0 ^ s1 ^ s3, so the second
    draw is chosen through s0 = wanted ^ s1 ^ s3. The other words are random."""
    rng = np.random.default_rng(seed)
    bits24 = np.asarray(bits24, np.uint64)
    out = ((bits24 << np.uint64(8)) | rng.integers(0, 256, len(bits24)).astype(np.uint64)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = out * np.uint32(0x38E38E39)                    # / 9
        x = (x >> np.uint32(7)) | (x << np.uint32(25))     # rotr 7
        s0 = x * np.uint32(0xCCCCCCCD)                     # / 5
    s = rng.integers(1, 1 << 32, (len(bits24), 4), dtype=np.uint64).astype(np.uint32)
    s[:, 0] = s0 if which == 0 else s0 ^ s[:, 1] ^ s[:, 3]
    return s


# ---- the scene as arrays (layouts: include/dcrt.h) ------------------------------------------------------
def _array(ptr, ctype, shape):
    n = int(np.prod(shape))
    if n == 0 or not ptr:
        return np.zeros(shape, ctype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).reshape(shape).copy()


def from_flat(flat):
    """A dcrt_flat_scene as numpy arrays."""
    I, T = flat.instance_count, flat.triangle_count
    s = {"vertices": _array(flat.vertices, C.c_float, (flat.vertex_count, 11)),
         "triangles": _array(flat.triangles, C.c_uint32, (T, 3)),
         "material_ids": _array(flat.material_ids, C.c_uint32, (T,)),
         "transforms": _array(flat.instance_transforms, C.c_float, (2 * I, 3, 4))[:I],   # [instance][column c][row r]
         "light_indices": _array(flat.instance_light_indices, C.c_uint32, (I,)),
         "overrides": _array(flat.instance_material_overrides, C.c_uint32, (I,)),
         "materials": _array(flat.materials, C.c_uint32, (flat.material_count, 13)),
         "lights": _array(flat.lights, C.c_uint32, (flat.light_count, 7)),
         "textures": [], "env": None}
    for k in range(flat.texture_count):
        t = flat.textures[k]
        ch = 1 if t.format == 1 else 4
        s["textures"].append((t.format, _array(t.pixels, C.c_uint8, (t.height, t.width, ch))))
    if flat.env_cube_rgb and flat.env_cube_size:
        n = flat.env_cube_size
        s["env"] = _array(flat.env_cube_rgb, C.c_float, (6, n, n, 3))
    return s


def frame_dict(frame):
    return {"camera": np.array(frame.camera_transform[:], np.float32).reshape(4, 4),
            "film_size": np.array(frame.film_size[:], np.float32), "aperture_radius": np.float32(frame.aperture_radius),
            "focal_distance": np.float32(frame.focal_distance), "film_distance": np.float32(frame.film_distance),
            "blade_count": int(frame.blade_count), "blade_vertex_pos": np.array(frame.blade_vertex_pos[:], np.float32),
            "aperture_base_angle": np.float32(frame.aperture_base_angle)}


def to_world(M, v, w, dtype):
    """Row vector (v, w) through instance matrices M (N, 3, 4) [column][row]."""
    M = M.astype(dtype)
    return np.einsum("ncr,nr->nc", M[:, :, :3], v) + M[:, :, 3] * dtype(w)


def true_normal(M, n):
    """The world-space normal of an instance-space normal: the inverse transpose (float64)."""
    A = np.transpose(M[:, :, :3].astype(np.float64), (0, 2, 1))     # A[r][c]: world = v A
    return _normalize(np.einsum("nrc,nc->nr", np.linalg.inv(A), n.astype(np.float64)))


# ---- camera -----------------------------------------------------------------------------------------
def concentric_disk(sx, sy, dtype):
    """Shirley & Chiu: the unit square to the unit disk, area-preserving."""
    x, y = dtype(2) * sx.astype(dtype) - dtype(1), dtype(2) * sy.astype(dtype) - dtype(1)
    wide = np.abs(x) > np.abs(y)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(wide, x, y)
        theta = np.where(wide, dtype(np.pi / 4) * (y / x), dtype(np.pi / 2) - dtype(np.pi / 4) * (x / y))
    zero = (x == 0) & (y == 0)
    theta = np.where(zero, 0, theta).astype(dtype)
    return np.where(zero, 0, r * np.cos(theta)).astype(dtype), np.where(zero, 0, r * np.sin(theta)).astype(dtype)


def blade_index(a2, n):
    """QUIRK-free but discrete: floor(a2 n) as float32 evaluates it."""
    return np.floor(a2.astype(np.float32) * np.float32(n)).astype(np.int64)


def aperture_point(f, ap, dtype):
    """The point of the aperture (camera space, z = 0) of aperture numbers (N, 3)."""
    a0, a1, a2 = (ap[:, k].astype(dtype) for k in range(3))
    n = f["blade_count"]
    if n <= 2:
        x, y = concentric_disk(a0, a1, dtype)
        return x * dtype(f["aperture_radius"]), y * dtype(f["aperture_radius"])
    vx, vy = dtype(f["blade_vertex_pos"][0]), dtype(f["blade_vertex_pos"][1])
    s = np.sqrt(a0)
    u, v = dtype(1) - s, a1 * s
    px, py = u * vx + v * vx, u * vy + v * -vy             # u A + v B + (1 - u - v) 0, A = (vx, vy), B = (vx, -vy)
    theta = blade_index(ap[:, 2], n).astype(dtype) * dtype(2 * np.pi / n) + dtype(f["aperture_base_angle"])
    c, sn = np.cos(theta), np.sin(theta)
    return px * c - py * sn, px * sn + py * c


def camera_ray(f, film, ap, dtype=np.float64):
    """World-space origin and direction, and the camera-space aperture point and focus point."""
    sx, sy = film[:, 0].astype(dtype), film[:, 1].astype(dtype)
    W, H = dtype(f["film_size"][0]), dtype(f["film_size"][1])
    d = _normalize(np.stack([(sx - dtype(0.5)) * W, (dtype(0.5) - sy) * H, np.full_like(sx, dtype(f["film_distance"]))], -1))
    o = np.zeros_like(d)
    focus = None
    if f["aperture_radius"] > 0:
        focus = d * (dtype(f["focal_distance"]) / d[:, 2])[:, None]
        x, y = aperture_point(f, ap, dtype)
        o = np.stack([x, y, np.zeros_like(x)], -1)
        d = _normalize(focus - o)
    M = f["camera"].astype(dtype)
    return o @ M[:3, :3] + M[3, :3], d @ M[:3, :3], o, focus


# ---- textures and the environment cube --------------------------------------------------------------
def srgb_decode(c8, dtype):
    c = c8.astype(np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(dtype)


def texture_rgba(texture, dtype):
    fmt, px = texture
    if fmt == 1:
        r = px[..., 0].astype(dtype) / dtype(255)
        return np.stack([r, np.zeros_like(r), np.zeros_like(r), np.ones_like(r)], -1)
    return np.concatenate([srgb_decode(px[..., :3], dtype), px[..., 3:].astype(dtype) / dtype(255)], -1)


def bilinear(img, x, y, wrap, dtype):
    """Bilinear fetch of img (h, w, C) at texel-space coordinates (texel centres at integers)."""
    h, w = img.shape[:2]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    ix = (lambda i: i % w) if wrap else (lambda i: np.clip(i, 0, w - 1))
    iy = (lambda i: i % h) if wrap else (lambda i: np.clip(i, 0, h - 1))
    top = img[iy(y0), ix(x0)] * (dtype(1) - fx) + img[iy(y0), ix(x0 + 1)] * fx
    bot = img[iy(y0 + 1), ix(x0)] * (dtype(1) - fx) + img[iy(y0 + 1), ix(x0 + 1)] * fx
    return top * (dtype(1) - fy) + bot * fy


def sample_texture(texture, tc, dtype):
    img = texture_rgba(texture, dtype)
    h, w = img.shape[:2]
    if h == 0 or w == 0:
        return np.zeros((len(tc), 4), dtype)
    return bilinear(img, tc[:, 0] * dtype(w) - dtype(0.5), tc[:, 1] * dtype(h) - dtype(0.5), True, dtype)


def cube_face(d):
    """The face (0..5: +x -x +y -y +z -z) of float32 directions as comparisons decide it (QUIRK Q2's ties)."""
    a = np.abs(d.astype(np.float32))
    axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    comp = np.take_along_axis(d, axis[:, None], 1)[:, 0]
    return 2 * axis + (~(comp >= 0)).astype(np.int64)


def env_lookup(env, d, dtype=np.float64, face=None):
    """The cube's rgb at directions d; `face` forces the faces (the other side of a boundary)."""
    face = cube_face(d.astype(np.float32)) if face is None else face
    d = d.astype(dtype)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    sc = np.choose(face, [-z, z, x, x, x, -x])
    tc = np.choose(face, [-y, -y, z, -z, -y, -y])
    ma = np.abs(np.choose(face, [x, x, y, y, z, z]))
    n = env.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        s, t = (sc / ma + dtype(1)) * dtype(0.5), (tc / ma + dtype(1)) * dtype(0.5)
    out = np.zeros((len(d), 3), dtype)
    for k in range(6):
        m = face == k
        if m.any():
            out[m] = bilinear(env[k].astype(dtype), s[m] * dtype(n) - dtype(0.5), t[m] * dtype(n) - dtype(0.5), False, dtype)   # QUIRK Q2
    return out


def face_margin(d):
    """How far a direction is from a face boundary: (largest - second largest magnitude) / largest, and the
    face on the other side."""
    a = np.abs(d.astype(np.float64))
    order = np.argsort(-a, axis=1)
    first, second = np.take_along_axis(a, order[:, :1], 1)[:, 0], np.take_along_axis(a, order[:, 1:2], 1)[:, 0]
    axis2 = order[:, 1]
    comp = np.take_along_axis(d, axis2[:, None], 1)[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (first - second) / first, 2 * axis2 + (~(comp >= 0)).astype(np.int64)


# ---- hit reconstruction -----------------------------------------------------------------------------
def _bary(p0, p1, p2, u, v):
    return p0 + (p1 - p0) * u[:, None] + (p2 - p0) * v[:, None]


def hit(s, u, v, tri, inst, dtype=np.float64, side=None):
    """The intersection of hit records. `side`: None, or a dict of forced decisions for the inputs that sit on
    a discontinuity -- "checker" (N,) cells, "keep" (N,) bool: the interpolated tangent survives both length
    tests, "cross" (N,) bool: the first fallback survives its test. Returns a dict; `margins` in it holds what
    the ambiguity classes are judged by."""
    tri = np.asarray(tri, np.int64) & 0x7FFFFFFF
    inst = np.asarray(inst, np.int64)
    u, v = np.asarray(u, np.float32).astype(dtype), np.asarray(v, np.float32).astype(dtype)
    V = s["vertices"][s["triangles"][tri]].astype(dtype)               # (N, 3, 11)
    M = s["transforms"][inst]
    P, Nn, Tt, UV = V[..., 0:3], V[..., 3:6], V[..., 6:9], V[..., 9:11]
    pos = _bary(P[:, 0], P[:, 1], P[:, 2], u, v)
    n = _normalize(_bary(Nn[:, 0], Nn[:, 1], Nn[:, 2], u, v))
    t0 = _bary(Tt[:, 0], Tt[:, 1], Tt[:, 2], u, v)
    len0 = _norm(t0)
    t1 = t0 - n * _dot(t0, n)[:, None]
    len1 = np.where(len0 >= DEGENERATE, _norm(t1), len0)
    keep = (len0 >= DEGENERATE) & (len1 >= DEGENERATE)
    fb = np.cross(n, np.array([0, 1, 0], dtype))
    lenf = _norm(fb)
    use_cross = lenf >= DEGENERATE
    if side is not None:
        keep = side.get("keep", keep)
        use_cross = side.get("cross", use_cross)
    with np.errstate(invalid="ignore", divide="ignore"):
        kept = np.where((len0 >= DEGENERATE)[:, None], t1, t0) / np.where(len0 >= DEGENERATE, _norm(t1), len0)[:, None]
        fallback = np.where(use_cross[:, None], fb, np.array([1, 0, 0], dtype)) / lenf[:, None]      # QUIRK Q5
    tangent = np.where(keep[:, None], kept, fallback)
    gn = _normalize(np.cross(P[:, 2] - P[:, 0], P[:, 1] - P[:, 0]))
    ov = s["overrides"][inst]
    mid = np.where(ov != NO_OVERRIDE, ov, s["material_ids"][tri]).astype(np.int64)
    mat = s["materials"][mid]
    matf = mat.view(np.float32)
    tc_raw = _bary(UV[:, 0], UV[:, 1], UV[:, 2], u, v)
    tiling = matf[:, 8:10].astype(dtype)
    tc = tc_raw * tiling
    albedo = matf[:, 0:3].astype(dtype)
    tex = mat[:, 3].astype(np.int32)
    for k in np.unique(tex[tex != -1]):
        m = tex == k
        albedo[m] = albedo[m] * sample_texture(s["textures"][k], tc[m], dtype)[:, :3]
    cell = np.where(tc > 0, np.floor(np.minimum(tc * dtype(2), dtype(4294967295.0))), 0).astype(np.uint64)     # QUIRK Q6
    checker = ((cell[:, 0] + cell[:, 1]) & 1).astype(np.int64)
    if side is not None and "checker" in side:
        checker = side["checker"]
    flags = mat[:, 11]
    rough = matf[:, 7].astype(dtype) * np.where((flags & ROUGHNESS_TEXTURE) != 0, checker.astype(dtype), dtype(1))
    # what the ambiguity classes are judged by (float64 runs): the distance of 2 tc from a cell edge against the
    # rounding of its terms; the tangent lengths against the rounding of theirs
    tc_scale = (np.abs(UV[:, 0]) + np.abs(UV[:, 1] - UV[:, 0]) * np.abs(u)[:, None] + np.abs(UV[:, 2] - UV[:, 0]) * np.abs(v)[:, None]) * np.abs(tiling) * 2
    t_scale = (np.abs(Tt[:, 0]) + np.abs(Tt[:, 1] - Tt[:, 0]) * np.abs(u)[:, None] + np.abs(Tt[:, 2] - Tt[:, 0]) * np.abs(v)[:, None]).max(1)
    return {"position": to_world(M, pos, 1, dtype),
            "normal": _normalize(to_world(M, n, 0, dtype)),                                   # QUIRK Q1
            "tangent": _normalize(to_world(M, tangent, 0, dtype)),
            "geometry_normal": _normalize(to_world(M, gn, 0, dtype)),
            "albedo": albedo, "alpha": rough * rough,
            "material_type": (flags & 0xF).astype(np.uint32),
            "flags": (((flags & TWO_SIDED) != 0) * 1 | ((flags & MULTISCATTERING) != 0) * 4 | ((flags >> 8) & 3) << 4).astype(np.uint32),
            "light_index": s["light_indices"][inst], "material": mid, "checker": checker, "keep": keep, "cross": use_cross,
            "margins": {"checker": np.where(tc * 2 > -1, np.abs(tc * 2 - np.round(np.maximum(tc * 2, 0))), np.inf), "checker_scale": tc_scale,
                        "uses_checker": (flags & ROUGHNESS_TEXTURE) != 0,
                        "len0": len0, "len1": len1, "lenf": lenf, "t_scale": t_scale, "fallback": ~keep}}


# ---- lights -----------------------------------------------------------------------------------------
def light_kind(lights):
    f = lights[:, 6]
    return np.where(f & POINT, POINT, np.where(f & DIRECTIONAL, DIRECTIONAL, np.where(f & MESH, MESH, np.where(f & ENVIRONMENT, ENVIRONMENT, 0))))


def select(draw, count):
    """QUIRK Q7: floor(draw * count) as float32 evaluates it."""
    return np.floor(draw.astype(np.float32) * np.asarray(count).astype(np.float32)).astype(np.int64)


def triangle_geometry(s, tri, instance, dtype):
    """World-space vertices, world-space area, the renderer's light normal (QUIRK Q1) and the true one."""
    P = s["vertices"][s["triangles"][tri]][..., 0:3].astype(dtype)
    M = s["transforms"][instance]
    W = np.stack([to_world(M, P[:, k], 1, dtype) for k in range(3)], 1)
    area = _norm(np.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0])) * dtype(0.5)
    n_inst = _normalize(np.cross(P[:, 2] - P[:, 0], P[:, 1] - P[:, 0]))
    return P, W, area, _normalize(to_world(M, n_inst, 0, dtype)), true_normal(M, n_inst)


def sample_light(s, light_count, p, states, dtype=np.float64, env_face=None, cos_floor=None):
    """Light sampling from points p (N, 3) with xoshiro states (N, 4). Returns a dict: radiance, wi, pdf,
    distance, delta, state (after the kind's draws), light, kind, and for mesh lights triangle, point, cos
    (the renderer's), cos_true, area. `cos_floor` (N,), NaN where unused: the mesh light's cos is taken as this positive
    number -- the lit side of an input whose cos is 0 up to rounding, with the smallest pdf that side can report."""
    N = len(p)
    p = np.asarray(p, np.float32).astype(dtype)
    u, _ = draws(states, 4)
    li = select(u[:, 0], light_count)
    L = s["lights"][li]
    Lf = L.view(np.float32)
    kind = light_kind(L)
    state = np.zeros((N, 4), np.uint32)
    for k, c in DRAWS.items():
        m = kind == k
        if m.any():
            state[m] = draws(np.asarray(states, np.uint32).reshape(-1, 4)[m], c)[1]
    out = {"radiance": np.zeros((N, 3), dtype), "wi": np.zeros((N, 3), dtype), "pdf": np.zeros(N, dtype), "distance": np.zeros(N, dtype),
           "delta": (kind == POINT) | (kind == DIRECTIONAL), "state": state, "light": li, "kind": kind,
           "triangle": np.full(N, -1, np.int64), "point": np.full((N, 3), np.nan), "cos": np.full(N, np.nan), "cos_true": np.full(N, np.nan),
           "area": np.full(N, np.nan), "draws": u}
    radiance = Lf[:, 0:3].astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = kind == POINT
        if m.any():
            w = Lf[m, 3:6].astype(dtype) - p[m]
            d = _norm(w)
            out["wi"][m], out["distance"][m] = w / d[:, None], d
            out["radiance"][m] = radiance[m] / (d * d)[:, None]
            out["pdf"][m] = 1
        m = kind == DIRECTIONAL
        if m.any():
            out["wi"][m], out["distance"][m] = -Lf[m, 3:6].astype(dtype), np.inf
            out["radiance"][m] = radiance[m]
            out["pdf"][m] = 1
        m = kind == MESH
        if m.any():
            offset, count, instance = L[m, 3].astype(np.int64), L[m, 4].astype(np.int64), L[m, 5].astype(np.int64)
            tri = (offset.astype(np.float32) + select(u[m, 1], count).astype(np.float32)).astype(np.int64)      # QUIRK Q7
            P, W, area, n_q, n_true = triangle_geometry(s, tri, instance, dtype)
            sq = np.sqrt(u[m, 2].astype(dtype))
            bu, bv = dtype(1) - sq, u[m, 3].astype(dtype) * sq
            x = to_world(s["transforms"][instance], _bary(P[:, 0], P[:, 1], P[:, 2], bu, bv), 1, dtype)
            w = x - p[m]
            d = _norm(w)
            wi = w / d[:, None]
            cos = -_dot(wi, n_q)
            if cos_floor is not None:
                cos = np.where(np.isnan(cos_floor[m]), cos, cos_floor[m].astype(dtype))
            pdf = np.where(area >= DEGENERATE, dtype(2) / area, 0) * (d * d / cos)      # QUIRK Q3, Q4
            lit = (cos > 0) & (pdf > 0)
            out["wi"][m], out["distance"][m] = wi, d
            out["radiance"][m] = np.where(lit[:, None], radiance[m], 0)
            out["pdf"][m] = np.where(cos > 0, pdf, 0) / count.astype(dtype)
            out["triangle"][m], out["point"][m], out["cos"][m], out["area"][m] = tri, x, cos, area
            out["cos_true"][m] = -_dot(wi.astype(np.float64), n_true)
        m = kind == ENVIRONMENT
        if m.any():
            z = dtype(1) - dtype(2) * u[m, 1].astype(dtype)
            r = np.sqrt(np.maximum(dtype(0), dtype(1) - z * z))
            phi = dtype(2 * np.pi) * u[m, 2].astype(dtype)
            wi = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)
            out["wi"][m], out["distance"][m] = wi, np.inf
            out["pdf"][m] = dtype(1 / (4 * np.pi))
            face = cube_face64(wi) if env_face is None else env_face[m]      # (of the run's own direction)
            out["radiance"][m] = radiance[m] * (env_lookup(s["env"], wi, dtype, face) if s["env"] is not None else 1)
    out["pdf"] = out["pdf"] / dtype(light_count)                                        # QUIRK Q8
    finite = np.isfinite(out["distance"])
    out["distance"] = np.where(finite, out["distance"] * dtype(np.float32(1) - SHADOW_EPSILON), out["distance"])
    return out


def cube_face64(d):
    a = np.abs(d)
    axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    comp = np.take_along_axis(d, axis[:, None], 1)[:, 0]
    return 2 * axis + (~(comp >= 0)).astype(np.int64)


def evaluate_light(s, light_count, li, tri, normal, wi, distance, dtype=np.float64):
    """Radiance and pdf of light li seen along wi at `distance`, the light's normal there `normal`."""
    li, tri = np.asarray(li, np.int64), np.asarray(tri, np.int64)
    normal, wi, distance = (np.asarray(a, np.float32).astype(dtype) for a in (normal, wi, distance))
    L = s["lights"][li]
    Lf = L.view(np.float32)
    kind = light_kind(L)
    N = len(li)
    radiance, pdf = np.zeros((N, 3), dtype), np.zeros(N, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = kind == MESH
        if m.any():
            _, _, area, _, _ = triangle_geometry(s, tri[m], L[m, 5].astype(np.int64), dtype)
            cos = -_dot(wi[m], normal[m])
            a = np.where(area * dtype(2) >= DEGENERATE, dtype(1) / area, 0)              # QUIRK Q3 (once), Q4
            radiance[m] = np.where((cos > 0)[:, None], Lf[m, 0:3].astype(dtype), 0)
            pdf[m] = a * np.where(cos > 0, distance[m] * distance[m] / cos, 0) / L[m, 4].astype(dtype)
        m = kind == ENVIRONMENT
        if m.any():
            radiance[m] = Lf[m, 0:3].astype(dtype) * (env_lookup(s["env"], wi[m].astype(np.float32), dtype) if s["env"] is not None else 1)
            pdf[m] = dtype(1 / (4 * np.pi))
    return radiance, pdf / dtype(light_count)
