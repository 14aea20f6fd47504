"""The first-hit "Output" views (dcrt_tracer_set_output: Shading Normal, Shading Tangent, Albedo,
Negative NdotV, Backface, Iteration Count -- MegakernelPathTracing.hlsl:212-291) on the GPU,
bit for bit against values built from the oracle's existing entry points alone:

* oracle.camera_ray: a pixel's camera ray and its RNG state after the five draws;
* oracle.render(...)[0]: the sample positions (the same first two draws);
* oracle.trace_rays: the ray's closest hit (t, u, v, triangle | backface << 31, instance), and,
  called with one ray at a time, that ray's node visits (iterationCounter);
* oracle.sample_convolution: the film of the expected samples.

What the views show of a hit is restated here in numpy float32, operation by operation, from
HitShader.inc.hlsl:31-83 (interpolation, the tangent's orthonormalisation and fall-backs, the
material override, the albedo texture) and RayTracingCommon.inc.hlsl:88-116 (the instance
transform): the library is built without FMA contraction and with correctly rounded division,
square root and reciprocal, so the restatement matches to the bit, and must.

oracle_trace_rays strips the any-hit bit, and these expectations are built from it: with
ALLOW_ANYHIT_SHADER on, the values of pixels whose first hit is masked are not rebuilt here, and that
case asserts the RNG state (one more draw than the opaque build: IntersectScene's opacity sample) and
the sample positions only. The any-hit test itself -- oracle_cast_rays and the cast kernels' OPACITY
variants, each ray with its opacity sample -- is held to a float64 reference by tests/test_ray_truth.py
and tests/test_gpu_ray_truth.py; the view kernel's trace_full<..., OPACITY> has no ray-level entry and
rests on its renders' bit equality with the oracle.
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GOLDEN, cornell

pytestmark = pytest.mark.gpu

F = np.float32
VIEWS = ["normal", "tangent", "albedo", "negative_ndotv", "backface", "iteration_count"]
DEFAULT, MOLLER, NO_F2B = 0x0D, 0x05, 0x0F   # VNDF | LIGHT_VISIBLE | WATERTIGHT; without WATERTIGHT; with NO_FRONT_TO_BACK
NONE = 0xFFFFFFFF


def same_bits(a, b):
    """Bit-identical, except that a NaN matches any NaN (the default NaN's sign differs between
    x86 and gfx950)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- the numpy float32 restatement -------------------------------------------------------------
def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _length(a):
    return np.sqrt(_dot(a, a))


def _normalize(a):   # a * (1 / sqrt(dot)): sqrt and the reciprocal correctly rounded
    s = F(1.0) / np.sqrt(_dot(a, a))
    return a * s[:, None]


def _bary(p0, p1, p2, u, v):   # VectorBaryCentric2 / 3 (Math.inc.hlsl:23-43)
    r1 = p1 - p0
    r2 = p2 - p0
    r1 = r1 * u[:, None]
    r2 = r2 * v[:, None]
    r1 = r1 + p0
    return r1 + r2


def _mul43(v, w, M):   # mul(float4(v, w), float4x3): three columns of four floats per instance
    out = []
    for c in range(3):
        col = M[:, 4 * c:4 * c + 4]
        out.append(v[:, 0] * col[:, 0] + v[:, 1] * col[:, 1] + v[:, 2] * col[:, 2] + F(w) * col[:, 3])
    return np.stack(out, axis=1)


def _srgb_table():
    return np.array([c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4) for c in (i / 255.0 for i in range(256))],
                    np.float64).astype(np.float32)


def _sample_texture_wrap(tex, u, v):
    """SampleLevel(UVWrapSampler, texcoord, 0): sRGB decode per texel, then the bilinear filter in
    sample_texture_wrap's order (top and bottom rows along x, then along y), wrap addressing."""
    w, h = int(tex.width), int(tex.height)
    assert w > 0 and h > 0
    px = np.ctypeslib.as_array(tex.pixels, (h * w * (1 if tex.format == 1 else 4),))
    table = _srgb_table()
    x = u * F(w) - F(0.5)
    y = v * F(h) - F(0.5)
    fx0, fy0 = np.floor(x), np.floor(y)
    fx, fy = x - fx0, y - fy0
    x0, x1 = fx0.astype(np.int64) % w, (fx0.astype(np.int64) + 1) % w
    y0, y1 = fy0.astype(np.int64) % h, (fy0.astype(np.int64) + 1) % h

    def texel(xx, yy):
        if tex.format == 1:   # R8_UNORM
            r = px[yy * w + xx].astype(np.float32) / F(255.0)
            return np.stack([r, np.zeros_like(r), np.zeros_like(r)], axis=1)
        p = px.reshape(h * w, 4)[yy * w + xx]
        return np.stack([table[p[:, 0]], table[p[:, 1]], table[p[:, 2]]], axis=1)

    a, b, c, d = texel(x0, y0), texel(x1, y0), texel(x0, y1), texel(x1, y1)
    one = F(1.0)
    top = a * (one - fx)[:, None] + b * fx[:, None]
    bot = c * (one - fx)[:, None] + d * fx[:, None]
    return top * (one - fy)[:, None] + bot * fy[:, None]


def _intersections(flat, hits):
    """HitInfoToIntersection for every hit: (normal, tangent, albedo), world space."""
    keep = flat._keep[0]
    V, T = keep["vertices"], keep["triangles"].reshape(-1, 3)
    tri = hits["triangle_id"] & np.uint32(0x7FFFFFFF)
    inst = hits["instance_index"]
    u, v = hits["u"].astype(np.float32), hits["v"].astype(np.float32)
    v0, v1, v2 = V[T[tri, 0]], V[T[tri, 1]], V[T[tri, 2]]
    thr = F(0.000001)
    with np.errstate(all="ignore"):
        normal = _normalize(_bary(v0[:, 3:6], v1[:, 3:6], v2[:, 3:6], u, v))
        tangent = _bary(v0[:, 6:9], v1[:, 6:9], v2[:, 6:9], u, v)
        tl = _length(tangent)
        ortho = tangent - normal * _dot(tangent, normal)[:, None]
        keepT = tl >= thr
        tangent = np.where(keepT[:, None], ortho, tangent)
        tl = np.where(keepT, _length(ortho), tl)
        up = np.broadcast_to(np.array([0.0, 1.0, 0.0], np.float32), normal.shape)
        picked = _cross(normal, up)
        pl = _length(picked)
        picked = np.where((pl >= thr)[:, None], picked, np.array([1.0, 0.0, 0.0], np.float32))
        degenerate = tl < thr
        tangent = np.where(degenerate[:, None], picked, tangent)
        tl = np.where(degenerate, pl, tl)
        tangent = tangent / tl[:, None]
        # the material: the instance's override, or the triangle's own
        ov = keep["overrides"][inst]
        mid = np.where(ov != NONE, ov, keep["material_ids"][tri])
        mats = keep["materials"][mid]
        mf = mats.view(np.float32)
        tc = _bary(v0[:, 9:11], v1[:, 9:11], v2[:, 9:11], u, v) * mf[:, 8:10]
        albedo = mf[:, 0:3].copy()
        texIndex = mats[:, 3].view(np.int32)
        for ti in np.unique(texIndex[texIndex != -1]):
            sel = texIndex == ti
            albedo[sel] = albedo[sel] * _sample_texture_wrap(flat.textures[int(ti)], tc[sel, 0], tc[sel, 1])
        M = keep["transforms"][inst]
        normal = _normalize(_mul43(normal, 0.0, M))
        tangent = _normalize(_mul43(tangent, 0.0, M))
    return normal.astype(np.float32), tangent.astype(np.float32), albedo.astype(np.float32)


# ---- expectations, from the oracle ---------------------------------------------------------------
class Expected:
    """One image's camera rays, first hits, per-ray node visits and sample positions."""

    def __init__(self, oracle, luts, scene, seed, resolution=None):
        self.oracle = oracle
        self.frame = oracle.frame_params(scene, seed)
        if resolution:
            self.frame.resolution[0], self.frame.resolution[1] = resolution
        self.features = self.frame.features
        self.flat = oracle.flat_with_own_bvh(scene)
        W, H = self.frame.resolution[0], self.frame.resolution[1]
        self.W, self.H = W, H
        from directcomputeraytracing_amd import make_rays
        o, d = np.zeros((H * W, 3), np.float32), np.zeros((H * W, 3), np.float32)
        self.rng = np.zeros((H, W, 4), np.uint32)
        for py in range(H):
            for px in range(W):
                o[py * W + px], d[py * W + px], self.rng[py, px] = oracle.camera_ray(self.frame, px, py)
        self.d = d
        self.rays = make_rays(o, d, 0.0, np.inf)
        self.pos = oracle.render(self.flat, luts, self.frame, oracle.MEGAKERNEL)[0]
        self.hits, _ = oracle.trace_rays(self.flat, self.rays, self.features)
        self.found = np.isfinite(self.hits["t"])
        self._visits = None
        self._its = None

    def visits(self):
        """Node visits per ray: the oracle's counter for a one-ray batch."""
        if self._visits is None:
            self._visits = np.array([self.oracle.trace_rays(self.flat, self.rays[i:i + 1], self.features)[1]["node_visits"]
                                     for i in range(len(self.rays))], np.int64)
        return self._visits

    def values(self, view, threshold=20):
        n = self.W * self.H
        val = np.zeros((n, 4), np.float32)
        green, red = np.array([0, 1, 0], np.float32), np.array([1, 0, 0], np.float32)
        if view == "iteration_count":
            c = self.visits()
            grey = (c.astype(np.float32) / F(threshold)).astype(np.float32)
            val[:, :3] = np.where((c <= threshold)[:, None], grey[:, None], red)
            return val.reshape(self.H, self.W, 4)
        f = self.found
        if self._its is None:
            self._its = _intersections(self.flat, self.hits[f])
        normal, tangent, albedo = self._its
        if view == "normal":
            val[f, :3] = normal * F(0.5) + F(0.5)
        elif view == "tangent":
            val[f, :3] = tangent * F(0.5) + F(0.5)
        elif view == "albedo":
            val[f, :3] = albedo
        elif view == "negative_ndotv":
            val[f, :3] = np.where((_dot(-self.d[f], normal) < F(0.0))[:, None], green, red)
        elif view == "backface":
            val[f, :3] = np.where(((self.hits["triangle_id"][f] >> 31) != 0)[:, None], green, red)
        else:
            raise KeyError(view)
        return val.reshape(self.H, self.W, 4)


_cache = {}


def expected(oracle, luts, key, make_scene, seed, features=None, resolution=None):
    k = (key, seed, features, resolution)
    if k not in _cache:
        s = make_scene()
        if features is not None:
            s.features = features
        _cache[k] = (s, Expected(oracle, luts, s, seed, resolution))
    return _cache[k]


def _cornell():
    return cornell(64, 48, 2)


def _xml_mix():
    from directcomputeraytracing_amd import Scene
    s = Scene((64, 48))
    s.load_from_file(GOLDEN / "xml_mix" / "scene.xml")
    return s


def _spaceship():
    from test_oracle import load_fixture_scene
    return load_fixture_scene("spaceship")


def _anyhit_off():
    from test_oracle import anyhit_scene
    return anyhit_scene()


def _anyhit_on():
    from test_gpu_parity import _anyhit_scenes
    return _anyhit_scenes()["mask_xml"]


@pytest.fixture(scope="module")
def view_tracer(native_lib, golden_luts):
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=1 << 14, debug_rng=True)
    t.set_luts(golden_luts)
    yield t
    t.destroy()


def _load(t, s, e, seed):
    """The scene on the tracer, with the expectation's resolution."""
    t.on_scene_loaded(s, frame_seed=seed)
    fp = s.frame_params(seed)
    if (fp.resolution[0], fp.resolution[1]) != (e.W, e.H):
        fp.resolution[0], fp.resolution[1] = e.W, e.H
        t.set_frame_params(fp)


def _check_view(t, oracle, s, e, seed, view, threshold=20, rng_draws=0):
    """render_images of one view image: sample positions, sample values, film and RNG state."""
    want = e.values(view, threshold)
    t.set_output(view, threshold)
    assert t.output() == (view, threshold)
    t.clear_film()
    t.render_images(seed, 1)
    pos, val = t.read_samples()
    assert np.array_equal(pos.view(np.uint32), e.pos.view(np.uint32)), "sample positions"
    bad = ~same_bits(val, want).all(-1)
    assert not bad.any(), f"{view}: {int(bad.sum())} of {bad.size} sample values differ, first at {np.argwhere(bad)[:3].tolist()}"
    film = oracle.sample_convolution(s.filter_params(), e.pos, want)
    assert same_bits(t.read_film(), film).all(), "film"
    state = e.rng.copy()
    for _ in range(rng_draws):
        for row in state:
            for st in row:
                oracle.rng_next(st)
    assert np.array_equal(t.read_rng(), state), "RNG state"


# ---- 1. Cornell ------------------------------------------------------------------------------------
_CORNELL_CASES = [(v, f) for v in ("normal", "backface", "iteration_count") for f in (DEFAULT, MOLLER, NO_F2B)] + \
                 [(v, DEFAULT) for v in ("tangent", "albedo", "negative_ndotv")]


@pytest.mark.parametrize("seed", [0, 5])
@pytest.mark.parametrize("view,features", _CORNELL_CASES)
def test_cornell_views_bit_exact(view_tracer, golden_luts, oracle_mod, view, features, seed):
    """Cornell 64x48: every view with the default features; Normal, Backface and Iteration Count
    also with the Moller-Trumbore test and without front-to-back order. No draw after the camera
    ray's five in an opaque build."""
    s, e = expected(oracle_mod, golden_luts, "cornell", _cornell, seed, features)
    assert e.features == features
    t = view_tracer
    try:
        _load(t, s, e, seed)
        _check_view(t, oracle_mod, s, e, seed, view)
    finally:
        t.set_output("path_tracing")


# ---- 2. transformed instances with material overrides ----------------------------------------------
@pytest.mark.parametrize("view", ["normal", "tangent", "albedo", "backface"])
def test_xml_mix_views_bit_exact(view_tracer, golden_luts, oracle_mod, view):
    """xml_mix: rectangle instances under transforms, with material overrides -- a view that
    skipped the instance transform or the override differs here."""
    s, e = expected(oracle_mod, golden_luts, "xml_mix", _xml_mix, 1)
    keep = e.flat._keep[0]
    assert (keep["overrides"] != NONE).any()
    t = view_tracer
    try:
        _load(t, s, e, 1)
        _check_view(t, oracle_mod, s, e, 1, view)
    finally:
        t.set_output("path_tracing")


# ---- 3. the heat map on instanced hulls, in every node order ---------------------------------------
@pytest.mark.parametrize("env", [{}, {"DCRT_NO_LDS_CACHE": "1"}, {"DCRT_NO_LDS_CACHE": "1", "DCRT_PAIR_TRAVERSAL": "1"}],
                         ids=["default", "no_lds_cache", "pair_order"])
def test_spaceship_iteration_count_bit_exact(native_lib, golden_luts, oracle_mod, monkeypatch, env):
    """The spaceship fixture (8 instanced hulls) on a 48x32 film, threshold = the median of the
    oracle's per-pixel counts: both branches of the heat map hold at least a tenth of the pixels.
    The counts are the oracle's whether the nodes sit in the LDS cache or in memory, in PackBVH's
    order or in the device's child-pair order."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    s, e = expected(oracle_mod, golden_luts, "spaceship", _spaceship, 2, resolution=(48, 32))
    assert e.flat.instance_count == 8
    counts = e.visits()
    threshold = int(np.median(counts))
    assert 1 <= threshold <= 10000
    below = int(np.count_nonzero(counts <= threshold))
    assert below >= counts.size // 10 and counts.size - below >= counts.size // 10, (threshold, below, counts.size)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = WavefrontPathTracer(path_pool_size=1 << 14, debug_rng=True)
    try:
        t.set_luts(golden_luts)
        _load(t, s, e, 2)
        info = t.info()
        if "DCRT_NO_LDS_CACHE" in env:
            assert info["cached_nodes"] == 0
        assert info["pair_traversal"] == (1 if "DCRT_PAIR_TRAVERSAL" in env else 0)
        _check_view(t, oracle_mod, s, e, 2, "iteration_count", threshold)
    finally:
        t.destroy()


# ---- 4. textured albedo -----------------------------------------------------------------------------
def test_textured_albedo_bit_exact(view_tracer, golden_luts, oracle_mod):
    """The any-hit fixture's textured floor with the any-hit shader off: the albedo view shows
    albedo * the wrap-addressed bilinear sRGB fetch."""
    s, e = expected(oracle_mod, golden_luts, "anyhit_off", _anyhit_off, 4)
    assert not (e.features & 0x10)
    keep = e.flat._keep[0]
    tri = e.hits["triangle_id"][e.found] & np.uint32(0x7FFFFFFF)
    ov = keep["overrides"][e.hits["instance_index"][e.found]]
    mid = np.where(ov != NONE, ov, keep["material_ids"][tri])
    textured = keep["materials"][mid][:, 3].view(np.int32) != -1
    assert np.count_nonzero(textured) >= e.found.size // 10, "the textured floor fills part of the frame"
    t = view_tracer
    try:
        _load(t, s, e, 4)
        _check_view(t, oracle_mod, s, e, 4, "albedo")
    finally:
        t.set_output("path_tracing")


# ---- 5. ALLOW_ANYHIT_SHADER -------------------------------------------------------------------------
def test_anyhit_view_draws_one_opacity_sample(view_tracer, golden_luts, oracle_mod):
    """With ALLOW_ANYHIT_SHADER the view draws IntersectScene's opacity sample: the RNG state is
    camera_ray's advanced by one draw, the sample positions are the oracle's. (The oracle's ray
    entry points strip the any-hit bit, so the values of masked pixels have no oracle here.)"""
    s = _anyhit_on()
    frame = oracle_mod.frame_params(s, 3)
    assert frame.features & 0x10
    W, H = frame.resolution[0], frame.resolution[1]
    state = np.zeros((H, W, 4), np.uint32)
    for py in range(H):
        for px in range(W):
            st = oracle_mod.camera_ray(frame, px, py)[2]
            oracle_mod.rng_next(st)
            state[py, px] = st
    p_ref = oracle_mod.render(oracle_mod.flat_with_own_bvh(s), golden_luts, frame, oracle_mod.MEGAKERNEL)[0]
    t = view_tracer
    try:
        t.on_scene_loaded(s, frame_seed=3)
        t.set_output("normal")
        t.clear_film()
        t.render_images(3, 1)
        pos, val = t.read_samples()
        assert np.array_equal(t.read_rng(), state)
        assert np.array_equal(pos.view(np.uint32), p_ref.view(np.uint32))
        assert np.isfinite(val).all() and (val[..., 3] == 0).all()
    finally:
        t.set_output("path_tracing")


# ---- 6. film bands ------------------------------------------------------------------------------------
def test_banded_view_matches_unbanded_rows(native_lib, golden_luts, oracle_mod):
    """Two film bands with two halo rows: the owned rows are the unbanded film's, all others zero."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    s, e = expected(oracle_mod, golden_luts, "cornell", _cornell, 0, DEFAULT)
    bands = [(5, 17), (30, 41)]
    full = oracle_mod.sample_convolution(s.filter_params(), e.pos, e.values("normal"))
    t = WavefrontPathTracer(path_pool_size=1 << 14)
    try:
        t.set_luts(golden_luts)
        _load(t, s, e, 0)
        t.set_film_bands(bands, 2)
        t.set_output("normal")
        t.clear_film()
        t.render_images(0, 1)
        film = t.read_film()
    finally:
        t.destroy()
    owned = np.zeros(e.H, bool)
    for y0, y1 in bands:
        owned[y0:y1] = True
    assert same_bits(film[owned], full[owned]).all()
    assert (film[~owned].view(np.uint32) == 0).all()
    assert np.count_nonzero(full[~owned]) > 0


# ---- 7. image sequencing ---------------------------------------------------------------------------------
def test_view_accumulates_images_in_seed_order(view_tracer, golden_luts, oracle_mod):
    """render_images(3, 4) in the albedo view: the sum of the four images' convolutions, seeds 3..6."""
    t = view_tracer
    film = None
    for seed in range(3, 7):
        s, e = expected(oracle_mod, golden_luts, "cornell", _cornell, seed, DEFAULT)
        film = oracle_mod.sample_convolution(s.filter_params(), e.pos, e.values("albedo"), film=film)
    try:
        _load(t, s, e, 3)
        t.set_output("albedo")
        t.clear_film()
        t.render_images(3, 4)
        assert same_bits(t.read_film(), film).all()
        pos, val = t.read_samples()   # the last image's
        assert np.array_equal(pos.view(np.uint32), e.pos.view(np.uint32))
        assert same_bits(val, e.values("albedo")).all()
    finally:
        t.set_output("path_tracing")


# ---- 8. the selector ------------------------------------------------------------------------------------
def test_selector_validation_trigger_and_return_to_path_tracing(native_lib, golden_luts, oracle_mod):
    from directcomputeraytracing_amd import WavefrontPathTracer, _abi
    s = _cornell()
    filt = s.filter_params()

    def path_traced(t):
        t.clear_film()
        t.render_images(0, 1)
        return t.read_samples() + (t.read_film(),)

    t = WavefrontPathTracer(path_pool_size=1 << 14)
    fresh = WavefrontPathTracer(path_pool_size=1 << 14)
    try:
        for x in (t, fresh):
            x.set_luts(golden_luts)
            x.on_scene_loaded(s)
        assert t.output() == ("path_tracing", 20)
        lib, h = t._lib, t._h

        def rc(kind, threshold):
            p = _abi.OutputParams(kind, threshold)
            return lib.dcrt_tracer_set_output(h, C.byref(p))

        assert rc(7, 20) == -1
        assert rc(_abi.OUTPUT_ITERATION_COUNT, 0) == -1
        assert rc(_abi.OUTPUT_ITERATION_COUNT, 10001) == -1
        assert t.output() == ("path_tracing", 20)          # a refused call changes nothing
        t.acquire_film_clear_trigger()
        assert not t.acquire_film_clear_trigger()
        t.set_output("normal")
        assert t.acquire_film_clear_trigger() and not t.acquire_film_clear_trigger()   # exactly once
        t.set_output("normal")
        assert not t.acquire_film_clear_trigger()          # no change, no trigger
        t.set_output("iteration_count", 10000)
        assert t.acquire_film_clear_trigger()
        t.set_output("iteration_count", 1)
        assert t.acquire_film_clear_trigger() and not t.acquire_film_clear_trigger()
        t.clear_film()
        t.render_images(0, 1)
        t.set_output("path_tracing")
        assert t.acquire_film_clear_trigger()
        got, want = path_traced(t), path_traced(fresh)
        for a, b in zip(got, want):
            assert same_bits(a, b).all()
        assert np.count_nonzero(want[1][..., :3]) > 0
        with pytest.raises(Exception):
            t.set_output("normal")
            t.render_images(0, 1, filt, convolve=False)    # kept sample slots: out of scope, refused
    finally:
        t.destroy()
        fresh.destroy()


# ---- 9. the frame loop -------------------------------------------------------------------------------------
def test_frame_loop_render_completes_a_view_image_in_one_call(view_tracer, golden_luts, oracle_mod):
    """render() with a view selected: the whole image of the frame seed in one call, complete, in
    the sample textures -- the caller's accumulate_film then convolves it as any other image."""
    s, e = expected(oracle_mod, golden_luts, "cornell", _cornell, 5, DEFAULT)
    want = e.values("backface")
    t = view_tracer
    try:
        _load(t, s, e, 5)
        t.set_output("backface")
        t.reset_image()
        assert not t.is_image_complete()
        t.clear_film()
        t.render()
        assert t.is_image_complete()
        pos, val = t.read_samples()
        assert np.array_equal(pos.view(np.uint32), e.pos.view(np.uint32))
        assert same_bits(val, want).all()
        t.accumulate_film()
        assert same_bits(t.read_film(), oracle_mod.sample_convolution(s.filter_params(), e.pos, want)).all()
    finally:
        t.set_output("path_tracing")


# ---- 10. the C++ host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["frame", "batch"])
def test_cpp_host_output_option(native_lib, golden_luts, oracle_mod, tmp_path, mode):
    """examples/dcrt_render --output normal, in the frame loop (CMI355XPathTracer::SetOutputType,
    render() per frame) and in --batch mode (render_images): the film of Cornell 64x48, seed 0."""
    import subprocess
    from directcomputeraytracing_amd import scenes
    from directcomputeraytracing_amd.build import build_examples
    exe = build_examples()
    s, e = expected(oracle_mod, golden_luts, "cornell", _cornell, 0, DEFAULT)
    film = tmp_path / "normal.film"
    args = [str(exe), str(scenes.CORNELL_OBJ), "64", "48", "1", "2", str(tmp_path / "normal.bmp"), "--output", "normal",
            "--film", str(film), "--pool", str(1 << 14)] + (["--batch"] if mode == "batch" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = oracle_mod.sample_convolution(s.filter_params(), e.pos, e.values("normal"))
    assert same_bits(np.fromfile(film, np.float32).reshape(48, 64, 4), want).all()
    assert (tmp_path / "normal.bmp").stat().st_size > 64 * 48 * 3
    bad = subprocess.run(args + ["--output", "depth"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2   # (not a view of the reference's: usage)
