"""Firefly re-weighting on the GPU (dcrt.h "firefly re-weighting"): film_cascade_kernel through accumulate_images on
synthetic samples, firefly_resolve_kernel through the device entry point on synthetic cascades, the render chain
on the oracle's sample textures, the re-weighted image into the denoiser, and the feature's lifetime and refusals
-- everything bit for bit against tests/firefly_ref.py."""
import numpy as np
import pytest

from conftest import cornell
from device_buffers import DeviceBuffers
import denoise_ref
import film_ref
import firefly_ref
import noise_ref
from noise_ref import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
BOUNCES = 2


def make_filter(kind, radius):
    from directcomputeraytracing_amd import FilterParams
    return FilterParams(int(kind), float(radius), 0.7, 0.2, 0.6, 2)


@pytest.fixture(scope="module")
def bare_tracer(native_lib):
    """A tracer without a scene: the film passes and the resolve need none."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=1 << 14)
    yield t
    t.destroy()


@pytest.fixture
def bufs():
    b = DeviceBuffers()
    yield b
    b.release()


def new_tracer(golden_luts, scene):
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=1 << 16, iterations_per_render=8)
    t.set_luts(golden_luts)
    t.on_scene_loaded(scene)
    return t


_frames = {}


def size_film(t, W, H):
    if (W, H) not in _frames:
        _frames[(W, H)] = cornell(W, H, 1).frame_params(0)
    t.set_frame_params(_frames[(W, H)])
    assert (t.width, t.height) == (W, H)


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~same_bits(got, want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[bad][:2].tolist()} != {want[bad][:2].tolist()}"


def oracle_convolve(oracle_mod):
    return lambda filt, pos, val4: oracle_mod.sample_convolution(filt, pos, val4)


def convolve_for(oracle_mod, kind):
    """film_ref's float32 box and triangle weights are the kernels' bits, so those two kinds run on the independent
    model; the other three take the oracle's convolution (firefly_ref's module text says why)."""
    return None if kind in (film_ref.BOX, film_ref.TRIANGLE) else oracle_convolve(oracle_mod)


# ---- 1. the cascade pass ------------------------------------------------------------------------------
CASCADE_PARAMS = {2: (2, 1.0, 8.0), 6: (6, 0.37, 3.3), 8: (8, 1.0, 8.0)}


def green_with_luminance(target):
    """A sample (r, g, 0), mostly green, whose luminance is exactly `target` in float32: g's product alone steps over
    some targets, so a little red makes up the difference."""
    target = F(target)
    g = F(target / F(0.587))
    for _ in range(8):
        g = np.nextafter(g, F(0))
    for _ in range(17):
        rest = F(target - F(g * F(0.587)))
        r = np.nextafter(F(rest / F(0.299)), F(0)) if rest > 0 else F(0)
        for _ in range(3 if rest > 0 else 1):
            v = np.array([r, g, 0.0], F)
            if rest >= 0 and firefly_ref.luminance(v) == target:
                return v
            r = np.nextafter(r, F(np.inf))
        g = np.nextafter(g, F(np.inf))
    raise AssertionError(f"no float32 sample of luminance {target!r}")


def cascade_images(params, seed, W, H, count):
    """Luminances log-uniform over [s_0 / 8, 8 s_{K-1}] in random non-negative colours, a few samples with a
    negative channel, and planted ones: luminance exactly 0, exactly every s_j, and their float32 neighbours."""
    rng = np.random.default_rng(seed)
    s = firefly_ref.constants(params)[0]
    planted = [np.zeros(3, F)]
    for x in s:
        planted += [green_with_luminance(y) for y in (np.nextafter(x, F(0)), x, np.nextafter(x, F(np.inf)))]
    images = []
    for _ in range(count):
        pos = np.minimum(rng.uniform(0.0, 1.0, (H, W, 2)).astype(F), np.nextafter(F(1), F(0)))
        lum = np.exp(rng.uniform(np.log(float(s[0]) / 8), np.log(float(s[-1]) * 8), (H, W, 1)))
        mix = rng.uniform(0.2, 1.0, (H, W, 3))
        val = np.zeros((H, W, 4), F)
        val[..., :3] = (lum * mix / (mix @ np.array([0.299, 0.587, 0.114]))[..., None]).astype(F)
        neg = rng.uniform(0, 1, (H, W)) < 0.05
        val[neg, 2] = -val[neg, 2] * F(6.0)            # (some of these clamp to luminance 0)
        where = rng.permutation(W * H)[:len(planted)]
        for k, v in zip(where, planted):
            val[k // W, k % W, :3] = v
        val[..., 3] = 1.0
        images.append((pos, val))
    return images


@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("K", [2, 6, 8])
def test_cascade_pass(bare_tracer, bufs, oracle_mod, K, kind):
    """37 x 29 (3 x 2 tiles, cut by both edges), radius 0.5 and 1.0 (staged) and 5.0 (the direct gather): two images,
    then a second call of one image onto the non-zero cascades; after each call the cascades are firefly_ref's and
    the film is the film of the same calls with the feature off, bit for bit."""
    W, H = 37, 29
    t = bare_tracer
    params = firefly_ref.make_params(*CASCADE_PARAMS[K], 3.0)
    images = cascade_images(params, 100 * K + kind, W, H, 3)
    lum = firefly_ref.luminance(np.stack([v for _, v in images])[..., :3])
    s = firefly_ref.constants(params)[0]
    assert (lum == 0).any() and all((lum == x).any() and (lum == np.nextafter(x, F(0))).any() and
                                    (lum == np.nextafter(x, F(np.inf))).any() for x in s)
    ptrs = [(bufs.upload(p), bufs.upload(v)) for p, v in images]
    size_film(t, W, H)
    for radius in (0.5, 1.0, 5.0):
        filt = make_filter(kind, radius)
        what = f"K {K} kind {kind} r {radius}"
        t.set_firefly_filter(None)
        plain = []
        for call in ((0, 1), (2,)):
            t.accumulate_images([ptrs[k][0] for k in call], [ptrs[k][1] for k in call], filt)
            plain.append(t.read_film())
        t.set_firefly_filter(params)
        ref = np.zeros((K, H, W, 4), F)
        for call, film in zip(((0, 1), (2,)), plain):
            t.accumulate_images([ptrs[k][0] for k in call], [ptrs[k][1] for k in call], filt)
            firefly_ref.accumulate(ref, filt, [images[k] for k in call], params, convolve=convolve_for(oracle_mod, kind))
            assert_same(t.read_cascades(), ref, what + f": cascades after images {call}")
            assert_same(t.read_film(), film, what + f": film after images {call}")
        assert t.film_image_count() == 3
        assert (ref[..., :3] != 0).any(axis=(1, 2, 3)).all(), what
    t.set_firefly_filter(None)


def test_adaptive_sentinel_through_the_cascade_pass(bare_tracer, bufs, oracle_mod):
    """Adaptive sampling's sentinel sample (position +inf, value 0) in a checkerboard of 8 x 8 blocks: the cascades
    are still firefly_ref's bit for bit, finite, at radius 0.5 and 2 (staged) and 5.5 (the direct gather)."""
    import adaptive_ref
    W, H = 64, 48
    t = bare_tracer
    params = firefly_ref.make_params(6, 0.37, 3.3, 3.0)
    bx, by = adaptive_ref.block_grid(W, H)
    blocks = np.array([j * bx + i for j in range(by) for i in range(bx) if (i + j) % 2 == 0], np.uint32)
    images = [adaptive_ref.mask_samples(p, v, blocks) for p, v in cascade_images(params, 9, W, H, 2)]
    assert np.isinf(images[0][0]).any() and np.isfinite(images[0][0]).any()
    ptrs = [(bufs.upload(p), bufs.upload(v)) for p, v in images]
    size_film(t, W, H)
    for kind, radius in ((film_ref.BOX, 0.5), (film_ref.GAUSSIAN, 2.0), (film_ref.MITCHELL, 5.5)):
        filt = make_filter(kind, radius)
        t.set_firefly_filter(params)
        t.accumulate_images([p for p, _ in ptrs], [v for _, v in ptrs], filt)
        ref = firefly_ref.accumulate(np.zeros((6, H, W, 4), F), filt, images, params, convolve=oracle_convolve(oracle_mod))
        got = t.read_cascades()
        assert np.isfinite(got).all()
        assert_same(got, ref, f"kind {kind} r {radius}")
    t.set_firefly_filter(None)


# ---- 2. the resolve through the device entry point -----------------------------------------------------
RESOLVE_SIZES = [(1, 1), (1, 5), (17, 16)]            # (W, H): corners only; edges; a tile cut
RESOLVE_CASES = [(K, kappa, n) for K in (2, 6, 8) for kappa, n in ((0.25, 1), (3.0, 1), (3.0, 7), (40.0, 64))]


def synthetic_cascades(W, H, params, image_count, seed):
    """A film and cascades whose counts put S_j around 1 + kappa / 2 in the interior: per pixel and cascade a count u
    in [0, a), a cut by a third of the entries to 0 and a tenth negative (Mitchell lobes: Y clamps to 0); a tenth of
    the weights 0 and a twentieth negative."""
    rng = np.random.default_rng(seed)
    s, _, _, kappa = firefly_ref.constants(params)
    K = len(s)
    terms = 3 * min(9, W * H)
    a = 2.0 * (1.0 + float(kappa) / 2) / terms * 1.6
    weight = rng.uniform(0.5, 3.0, (H, W))
    u = rng.uniform(0.0, a, (K, H, W))
    u[rng.uniform(0, 1, u.shape) < 0.33] = 0.0
    grey = u * s[:, None, None].astype(np.float64) * weight[None] / image_count
    mix = rng.uniform(0.2, 1.0, (K, H, W, 3))
    cas = np.zeros((K, H, W, 4), F)
    cas[..., :3] = (grey[..., None] * mix / (mix @ np.array([0.299, 0.587, 0.114]))[..., None]).astype(F)
    negative = rng.uniform(0, 1, (K, H, W)) < 0.1
    cas[negative, :3] *= F(-1.0)
    film = np.zeros((H, W, 4), F)
    film[..., :3] = rng.uniform(0.0, 4.0, (H, W, 3))
    film[..., 3] = weight
    if W * H > 1:
        r = rng.uniform(0, 1, (H, W))
        film[r < 0.10, 3] = 0.0
        film[r < 0.05, 3] = -1.5
    return film, cas


def test_resolve_device(bare_tracer, bufs):
    """firefly_resolve_device on synthetic cascades at 1 x 1, 1 x 5 and 17 x 16, K 2, 6 and 8, kappa small and large,
    image counts 1, 7 and 64: bit for bit the reference's image. The reference's own omega (j >= 1, valid pixels) take
    0, 1 and values in between, with no more than 90 % of them at either end -- checked before the GPU runs."""
    t = bare_tracer
    omegas = []
    runs = []
    for W, H in RESOLVE_SIZES:
        for K, kappa, n in RESOLVE_CASES:
            params = firefly_ref.make_params(K, 0.37, 3.3, kappa)
            film, cas = synthetic_cascades(W, H, params, n, seed=W * 1000 + H * 10 + K)
            want, omega = firefly_ref.resolve(film, cas, n, params)
            omegas.append(omega[1:][:, film[..., 3] > 0].ravel())
            runs.append((W, H, params, n, film, cas, want))
    omega = np.concatenate(omegas)
    at_zero, at_one = float((omega == 0).mean()), float((omega == 1).mean())
    print(f"omega: {omega.size} values, {at_zero:.3f} at 0, {at_one:.3f} at 1")
    assert at_zero > 0 and at_one > 0 and ((omega > 0) & (omega < 1)).any()
    assert at_zero <= 0.9 and at_one <= 0.9 and at_zero + at_one <= 0.9
    invalid = 0
    for W, H, params, n, film, cas, want in runs:
        d_out = bufs.filled((H, W, 4), np.nan)
        t.firefly_resolve_device(W, H, n, bufs.upload(film), [bufs.upload(c) for c in cas], d_out, params)
        assert_same(bufs.download(d_out), want, f"{W}x{H} K {params.cascades} kappa {params.min_support} N {n}")
        invalid += int((~(film[..., 3] > 0)).sum())
        assert not want[~(film[..., 3] > 0)].any()
        bufs.release()
    assert invalid > 10


# ---- 3. the render chain -------------------------------------------------------------------------------
RW, RH = 48, 32
RENDER_PARAMS = (6, 0.01, 3.0, 1.0)        # s = 0.01 .. 2.43: Cornell's samples put some into every cascade


@pytest.fixture(scope="module")
def render_reference(oracle_mod, golden_luts):
    """(scene, filter, film, cascades, re-weighted image) of six oracle images of the Cornell box, computed once."""
    s = cornell(RW, RH, BOUNCES)
    filt = s.filter_params()
    params = firefly_ref.make_params(*RENDER_PARAMS)
    images = noise_ref.cornell_images(oracle_mod, golden_luts, RW, RH, BOUNCES, range(6))
    film, _ = noise_ref.films_of(oracle_mod, filt, images)
    cas = firefly_ref.accumulate(np.zeros((6, RH, RW, 4), F), filt, images, params, convolve=oracle_convolve(oracle_mod))
    out, omega = firefly_ref.resolve(film, cas, 6, params)
    assert (cas[..., :3] != 0).any(axis=(1, 2, 3)).all() and ((omega > 0) & (omega < 1)).any()
    for a in (film, cas, out):
        a.setflags(write=False)
    return s, filt, params, film, cas, out


@pytest.mark.parametrize("mode", ["wavefront", "megakernel"])
def test_render_chain(native_lib, golden_luts, render_reference, mode):
    """48 x 32, 6 images, max bounce 2: cascades and re-weighted image are firefly_ref's over the oracle's sample
    textures of the same seeds, the film is the oracle's, and a batch of 6 gives the bits of 6 batches of 1."""
    s, filt, params, film, cas, out = render_reference
    t = new_tracer(golden_luts, s)
    try:
        t.set_mode(mode)
        t.set_firefly_filter(params)
        for batch in (6, 1):
            t.clear_film()
            t.set_image_batch(batch)
            t.render_images(0, 6, filt)
            what = f"{mode}, batches of {batch}"
            assert t.film_image_count() == 6
            assert_same(t.read_film(), film, what + ": film")
            assert_same(t.read_cascades(), cas, what + ": cascades")
            assert_same(t.firefly_filtered(), out, what + ": re-weighted image")
    finally:
        t.destroy()


# ---- 4. feeding the denoiser -----------------------------------------------------------------------------
def test_reweighted_image_feeds_the_denoiser(bare_tracer, bufs):
    """denoise_device with the re-weighted image (film convention, w = 1) as its colour input is denoise_ref on it."""
    t = bare_tracer
    W, H = 40, 33
    params = firefly_ref.make_params(6, 0.37, 3.3, 3.0)
    film, cas = synthetic_cascades(W, H, params, 4, seed=77)
    want, _ = firefly_ref.resolve(film, cas, 4, params)
    _, normal, albedo = denoise_ref.random_inputs(5, W, H)
    d_color, d_out = bufs.filled((H, W, 4), np.nan), bufs.filled((H, W, 4), np.nan)
    t.firefly_resolve_device(W, H, 4, bufs.upload(film), [bufs.upload(c) for c in cas], d_color, params)
    t.denoise_device(W, H, d_color, bufs.upload(normal), bufs.upload(albedo), d_out)
    assert_same(bufs.download(d_color), want, "re-weighted image")
    assert_same(bufs.download(d_out), denoise_ref.denoise(want, normal, albedo, **denoise_ref.DEFAULTS), "denoised")


# ---- 5. lifetime and refusals ----------------------------------------------------------------------------
def test_lifetime(native_lib, golden_luts, bufs):
    from directcomputeraytracing_amd import DCRTError
    W, H = 48, 32
    s = cornell(W, H, BOUNCES)
    ref, t = new_tracer(golden_luts, s), new_tracer(golden_luts, s)
    try:
        ref.render_images(0, 3)
        want = ref.read_film()
        t.render_images(0, 3)
        assert t.firefly_filter() is None
        with pytest.raises(DCRTError, match="firefly re-weighting is off"):
            t.read_cascades()
        with pytest.raises(DCRTError, match="firefly re-weighting is off"):
            t.firefly_filtered()
        # toggling drops the captured graphs once; min_support alone drops none, but clears as every set does
        drops = t.upload_stats()["graph_invalidations"]
        p = firefly_ref.make_params(*RENDER_PARAMS)
        t.set_firefly_filter(p)
        assert t.upload_stats()["graph_invalidations"] == drops + 1 and t.film_image_count() == 0
        assert not t.read_film().any() and not t.read_cascades().any()
        with pytest.raises(DCRTError, match="INVALID_ARG.*no image reached the film"):
            t.firefly_filtered()
        t.render_images(0, 3)
        assert_same(t.read_film(), want, "film with the feature on")
        ptrs = t.cascade_device_ptrs()
        first = t.firefly_filtered()
        drops = t.upload_stats()["graph_invalidations"]
        p2 = firefly_ref.make_params(*RENDER_PARAMS[:3], 7.0)
        t.set_firefly_filter(p2)
        assert t.upload_stats()["graph_invalidations"] == drops and t.cascade_device_ptrs() == ptrs
        assert t.firefly_filter().min_support == 7.0 and t.film_image_count() == 0 and not t.read_cascades().any()
        with pytest.raises(DCRTError, match="no re-weighted image"):
            t.resolve_image(firefly=True)
        t.render_images(0, 3)
        cas = t.read_cascades()
        assert cas[..., :3].any() and not cas[..., 3].any()
        assert_same(t.firefly_filtered(), firefly_ref.resolve(want, cas, 3, p2)[0], "min_support 7")
        assert not np.array_equal(first, t.firefly_filtered())
        assert t.resolve_image(firefly=True).shape == (H, W, 4)
        # clear_film zeroes the cascades; a resolution change resizes them; the params persist across upload_scene
        t.clear_film()
        assert not t.read_cascades().any() and t.film_image_count() == 0
        t.on_scene_loaded(cornell(37, 29, BOUNCES))
        assert t.read_cascades().shape == (6, 29, 37, 4) and not t.read_cascades().any()
        assert t.firefly_filter().min_support == 7.0
        t.render_images(0, 1)
        assert t.read_cascades()[..., :3].any()
        # refusals while it is on
        for call in (lambda: t.set_film_bands([(0, 8)], 2), lambda: t.set_film_partition(2, 0),
                     lambda: t.add_film_device(bufs.upload(np.zeros((29, 37, 4), F)))):
            with pytest.raises(DCRTError, match="INVALID_ARG.*firefly"):
                call()
        for bad in ((1, 1.0, 8.0, 3.0), (9, 1.0, 8.0, 3.0), (6, 0.0, 8.0, 3.0), (6, -1.0, 8.0, 3.0), (6, 1.0, 1.0, 3.0),
                    (6, 1.0, 8.0, 0.0), (6, np.nan, 8.0, 3.0), (6, 1.0, np.inf, 3.0), (6, 1.0, 8.0, np.nan), (8, 1e30, 1e3, 3.0)):
            with pytest.raises(DCRTError, match="INVALID_ARG.*firefly"):
                t.set_firefly_filter(firefly_ref.make_params(*bad))
            with pytest.raises(DCRTError, match="INVALID_ARG.*firefly"):
                t.firefly_resolve_device(4, 4, 1, 1, [1] * int(np.clip(bad[0], 0, 9)), 1, firefly_ref.make_params(*bad))
        assert t.firefly_filter().min_support == 7.0
        banded = new_tracer(golden_luts, s)
        try:
            banded.set_film_bands([(0, 8)], 2)
            with pytest.raises(DCRTError, match="INVALID_ARG.*banded or partitioned"):
                banded.set_firefly_filter(p)
        finally:
            banded.destroy()
        # off again: the tracer is the one that never had it on (the graph drops aside, which the toggles count)
        t.on_scene_loaded(s)
        t.set_firefly_filter(None)
        assert t.firefly_filter() is None
        t.add_film_device(bufs.upload(np.zeros((H, W, 4), F)))
        t.clear_film()
        t.render_images(0, 3)
        assert_same(t.read_film(), want, "film with the feature off again")
        ref.on_scene_loaded(cornell(37, 29, BOUNCES))       # (the same uploads as `t` made)
        ref.on_scene_loaded(s)
        a, b = t.upload_stats(), ref.upload_stats()
        for key in a:
            if key != "graph_invalidations":
                assert a[key] == b[key], key
    finally:
        ref.destroy()
        t.destroy()


# ---- 6. dcrt_render --firefly ------------------------------------------------------------------------------
def test_cpp_host_firefly_option(native_lib, tmp_path):
    """examples/dcrt_render --firefly (frame loop and --batch) writes the BMP of the Python host's render_images +
    firefly_filtered + resolve_image(firefly=True), and with --denoise that of denoise(firefly=True)."""
    import json
    import subprocess
    from directcomputeraytracing_amd import WavefrontPathTracer, save_bmp, scenes
    from directcomputeraytracing_amd.build import build_examples
    exe = build_examples()
    w, h, spp, bounces = 48, 32, 3, 3
    px, col = scenes.POINT_LIGHT_POSITION, scenes.POINT_LIGHT_COLOR
    fields = "6:0.01:3:1"
    out, removed = {}, {}
    for tag, extra in (("frame", []), ("batch", ["--batch"]), ("denoise", ["--batch", "--denoise"])):
        bmp = tmp_path / f"{tag}.bmp"
        cmd = [str(exe), str(scenes.CORNELL_OBJ), str(w), str(h), str(spp), str(bounces), str(bmp), "--pool", "16384",
               "--point", *map(str, px), *map(str, col), "--firefly", fields, *extra]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        out[tag] = bmp.read_bytes()
        removed[tag] = json.loads(res.stdout.strip().splitlines()[-1])["firefly"]["removed"]
    s = cornell(w, h, bounces)
    t = WavefrontPathTracer(path_pool_size=1 << 14)
    try:
        t.on_scene_loaded(s)
        t.set_firefly_filter(firefly_ref.make_params(6, 0.01, 3.0, 1.0))
        t.render_images(0, spp)
        save_bmp(tmp_path / "plain.bmp", t.resolve_image(s.postfx_params()))
        kept = t.firefly_filtered()
        save_bmp(tmp_path / "py.bmp", t.resolve_image(s.postfx_params(), firefly=True))
        t.render_guides(0, spp)
        denoised = t.denoise(firefly=True)
        save_bmp(tmp_path / "py_denoised.bmp", t.resolve_image(s.postfx_params(), denoised=True))
        assert np.array_equal(kept, t.firefly_filtered())      # (the guides and the denoiser left film and cascades alone)
        # denoise(firefly=True) is the filter over the re-weighted image and the film's guides
        nrm, alb = t.read_guides()
        assert_same(denoised, denoise_ref.denoise(kept, nrm, alb, **denoise_ref.DEFAULTS), "denoise(firefly=True)")
        for bad in ("6:1:8", "6:1:8:x", "six:1:8:3", "out.bmp"):
            res = subprocess.run([str(exe), str(scenes.CORNELL_OBJ), str(w), str(h), "1", "1", str(tmp_path / "no.bmp"), "--firefly", bad],
                                 capture_output=True, text=True, timeout=60)
            assert res.returncode == 2 and "usage" in res.stderr, bad
    finally:
        t.destroy()
    assert out["frame"] == out["batch"] == (tmp_path / "py.bmp").read_bytes()
    assert out["denoise"] == (tmp_path / "py_denoised.bmp").read_bytes()
    assert out["frame"] != (tmp_path / "plain.bmp").read_bytes()
    assert 0.0 < removed["frame"] == removed["batch"] < 0.5
