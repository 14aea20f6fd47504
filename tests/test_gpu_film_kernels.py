"""The image-space kernels on synthetic inputs, bit for bit against the oracle: film_kernel through
accumulate_images (device pointers to arbitrary sample textures), add_film_kernel and
copy_film_device, and the luminance reduction + postfx_kernel through resolve_image of a film
loaded with clear_film + add_film_device. The oracle's side of each pass is held to independent
numpy models in tests/test_film_ref.py.

No render is needed: set_frame_params sizes the film, tests/device_buffers.py holds the inputs.
"""
import numpy as np
import pytest

from conftest import cornell
from device_buffers import DeviceBuffers
import film_ref
from test_gpu_parity import same_bits

pytestmark = pytest.mark.gpu

ALL_KINDS = range(5)
BELOW_4_5 = float(np.nextafter(np.float32(4.5), np.float32(0)))
# staged with 1, 2 and 3 staging elements per thread (spans up to 16, 22 and 24), then the direct gather
RADII = (0.001, 0.49, 0.5, 1.0, 2.5, 3.0, 3.5, 4.0, BELOW_4_5, 4.5, 5.0, 16.0)


def make_filter(kind, radius, tau=3, alpha=1.5, B=1 / 3, C=1 / 3):
    from directcomputeraytracing_amd import FilterParams
    return FilterParams(int(kind), float(radius), alpha, B, C, int(tau))


@pytest.fixture(scope="module")
def film_tracer(native_lib):
    from directcomputeraytracing_amd import WavefrontPathTracer
    t = WavefrontPathTracer(path_pool_size=1 << 14)
    yield t
    t.destroy()


@pytest.fixture
def bufs():
    b = DeviceBuffers()
    yield b
    b.release()


_frames = {}


def size_film(t, W, H):
    """Size the tracer's film without a scene or a render (SetFrame calls EnsureFilm)."""
    if (W, H) not in _frames:
        _frames[(W, H)] = cornell(W, H, 1).frame_params(0)
    t.set_frame_params(_frames[(W, H)])
    assert (t.width, t.height) == (W, H)


def random_images(rng, W, H, count):
    """`count` images of sub-pixel offsets in [0, 1) and signed values (alpha 1)."""
    out = []
    for _ in range(count):
        pos = np.minimum(rng.uniform(0.0, 1.0, (H, W, 2)).astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))
        val = rng.uniform(-1.0, 3.0, (H, W, 4)).astype(np.float32)
        val[..., 3] = 1.0
        out.append((pos, val))
    return out


def prior_film(W, H, seed=99):
    """A non-zero film to accumulate onto, so that film + sum is computed and not 0 + sum."""
    return np.random.default_rng(seed).uniform(0.5, 2.0, (H, W, 4)).astype(np.float32)


def load_film(t, bufs, film):
    t.clear_film()
    t.add_film_device(bufs.upload(film))


def gpu_accumulate(t, bufs, filt, images, prior=None, order=None):
    """The film after accumulate_images of `images` (in list order, or images[k] for k in `order`)
    onto `prior`."""
    H, W = images[0][0].shape[:2]
    size_film(t, W, H)
    load_film(t, bufs, np.zeros((H, W, 4), np.float32) if prior is None else prior)
    ptrs = [(bufs.upload(p), bufs.upload(v)) for p, v in images]
    order = range(len(images)) if order is None else order
    t.accumulate_images([ptrs[k][0] for k in order], [ptrs[k][1] for k in order], filt)
    return t.read_film()


def oracle_accumulate(oracle_mod, filt, images, prior=None, row_runs=None):
    H, W = images[0][0].shape[:2]
    ref = np.zeros((H, W, 4), np.float32) if prior is None else prior.copy()
    for pos, val in images:
        for rows in (row_runs or [None]):
            oracle_mod.sample_convolution(filt, pos, val, ref, rows=rows)
    return ref


def assert_same_film(film, ref, what):
    bad = ~same_bits(film, ref).all(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at (y, x) {tuple(np.argwhere(bad)[0])}"


# ---- film reconstruction -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_kinds_and_radii(film_tracer, bufs, oracle_mod, kind):
    """Every kind on 37 x 29 (3 x 2 tiles, cut by both edges) at radii through the staged path's
    1, 2 and 3 staging elements per thread and into the direct gather; two images onto a
    non-zero film."""
    W, H = 37, 29
    images = random_images(np.random.default_rng(10 + kind), W, H, 2)
    prior = prior_film(W, H)
    for radius in RADII:
        filt = make_filter(kind, radius, tau=2, alpha=0.7, B=0.2, C=0.6)
        film = gpu_accumulate(film_tracer, bufs, filt, images, prior)
        assert_same_film(film, oracle_accumulate(oracle_mod, filt, images, prior), f"kind {kind} r {radius!r}")
        assert not np.array_equal(film, prior) or radius < 0.5


@pytest.mark.parametrize("W,H", [(24, 24), (25, 24), (24, 25), (23, 40)])
def test_span_boundary(film_tracer, bufs, oracle_mod, W, H):
    """Radius 16: the whole film is every pixel's window, and a tile's span is the film. 24 wide
    is exactly the staged span's limit, 25 takes the direct gather."""
    images = random_images(np.random.default_rng(W * 100 + H), W, H, 2)
    prior = prior_film(W, H)
    for kind in ALL_KINDS:
        filt = make_filter(kind, 16.0, alpha=0.01)
        film = gpu_accumulate(film_tracer, bufs, filt, images, prior)
        assert_same_film(film, oracle_accumulate(oracle_mod, filt, images, prior), f"{W}x{H} kind {kind}")


@pytest.mark.parametrize("W,H", [(1, 40), (40, 1), (15, 15), (16, 16), (17, 17)])
def test_narrow_films(film_tracer, bufs, oracle_mod, W, H):
    images = random_images(np.random.default_rng(W * 100 + H), W, H, 2)
    prior = prior_film(W, H)
    for kind in ALL_KINDS:
        for radius in (0.5, 2.0):
            filt = make_filter(kind, radius)
            film = gpu_accumulate(film_tracer, bufs, filt, images, prior)
            assert_same_film(film, oracle_accumulate(oracle_mod, filt, images, prior), f"{W}x{H} kind {kind} r {radius}")


@pytest.mark.parametrize("radius,offsets", film_ref.SUPPORT_EDGE_CASES)
def test_support_edges(film_tracer, bufs, oracle_mod, radius, offsets):
    """Samples exactly on a pixel centre's support edge (|d| == r in float32: box takes them with
    |d| <= r, Lanczos with its x > r test), offsets 0 and the last float below 1, and a few outside
    [0, 1): the operation is defined by position, and both sides must agree."""
    from directcomputeraytracing_amd import FILTER_BOX, FILTER_LANCZOS
    W, H = 37, 29
    rng = np.random.default_rng(int(radius * 100))
    choices = np.array(list(offsets) * 3 + [0.0, float(np.nextafter(np.float32(1), np.float32(0))), -0.3, 1.7], np.float32)
    images = []
    for _ in range(2):
        pos = choices[rng.integers(0, len(choices), (H, W, 2))]
        val = rng.uniform(-1.0, 3.0, (H, W, 4)).astype(np.float32)
        images.append((pos, val))
        assert film_ref.pairs_on_support_edge(pos, radius) > 100
    prior = prior_film(W, H)
    for kind, tau in ((FILTER_BOX, 3), (FILTER_LANCZOS, 1), (FILTER_LANCZOS, 3)):
        filt = make_filter(kind, radius, tau=tau)
        film = gpu_accumulate(film_tracer, bufs, filt, images, prior)
        assert_same_film(film, oracle_accumulate(oracle_mod, filt, images, prior), f"kind {kind} tau {tau} r {radius}")


def windows_containing(W, H, radius, x0, y0):
    """Pixels whose gather window holds sample texel (x0, y0) (film_pixel_window, float32)."""
    r, f = np.float32(radius), np.float32
    cx, cy = np.arange(W, dtype=f) + f(0.5), np.arange(H, dtype=f) + f(0.5)
    in_x = (np.floor(cx - r) <= x0) & (x0 <= np.floor(cx + r))
    in_y = (np.floor(cy - r) <= y0) & (y0 <= np.floor(cy + r))
    return in_y[:, None] & in_x[None, :]


@pytest.mark.parametrize("kind,radius", [(2, 1.5), (0, 5.0), (4, 2.0)])
def test_sample_values(film_tracer, bufs, oracle_mod, kind, radius):
    """Negative values, denormals and 1e30; one inf and one NaN sample, which reach exactly the
    windows that hold them (a weight of 0 included: 0 * inf and 0 * nan are nan, as in the oracle)
    and leave every weight sum finite; and the samples' fourth channel is never read."""
    W, H = 37, 29
    rng = np.random.default_rng(7)
    (pos, val), = random_images(rng, W, H, 1)
    val[3, 4, :3] = (1e-40, -1e-42, 1.4e-45)
    val[10, 11, :3] = (1e30, -1e30, 1e30)
    val[25, 2, :3] = (1e30, 1e30, 0.0)
    val[5, 7, 1] = np.inf
    val[20, 30, 0] = np.nan
    prior = prior_film(W, H)
    filt = make_filter(kind, radius)
    film = gpu_accumulate(film_tracer, bufs, filt, [(pos, val)], prior)
    assert_same_film(film, oracle_accumulate(oracle_mod, filt, [(pos, val)], prior), f"kind {kind}")
    expected = windows_containing(W, H, radius, 7, 5) | windows_containing(W, H, radius, 30, 20)
    assert 0 < expected.sum() < W * H
    assert np.array_equal(~np.isfinite(film[..., :3]).all(-1), expected)
    assert np.isfinite(film[..., 3]).all()
    garbage = val.copy()
    garbage[..., 3] = rng.uniform(-1e30, 1e30, (H, W)).astype(np.float32)
    garbage[::3, ::2, 3] = np.nan
    garbage[1::3, 1::2, 3] = np.inf
    again = gpu_accumulate(film_tracer, bufs, filt, [(pos, garbage)], prior)
    assert_same_film(again, film, f"kind {kind}, fourth channel")


@pytest.mark.parametrize("kind,radius", [(2, 1.5), (0, 5.0)])
def test_image_counts(film_tracer, bufs, oracle_mod, kind, radius):
    """Pointer lists of 1, 2, 3, 4, 7 and 65 distinct buffers through the film pass's software
    pipeline (prologue, steady state, epilogue; staged path) and the direct gather's image loop,
    against the oracle applied image by image in list order; and a list that repeats a pointer."""
    W, H = 37, 29
    images = random_images(np.random.default_rng(3), W, H, 65)
    prior = prior_film(W, H)
    filt = make_filter(kind, radius)
    for count in (1, 2, 3, 4, 7, 65):
        film = gpu_accumulate(film_tracer, bufs, filt, images[:count], prior)
        assert_same_film(film, oracle_accumulate(oracle_mod, filt, images[:count], prior), f"kind {kind}: {count} images")
        bufs.release()
    order = [0, 1, 0, 0, 2, 1]
    film = gpu_accumulate(film_tracer, bufs, filt, images[:3], prior, order=order)
    assert_same_film(film, oracle_accumulate(oracle_mod, filt, [images[k] for k in order], prior), f"kind {kind}: repeated")


@pytest.mark.parametrize("kind,radius", [(2, 1.5), (3, 3.0), (0, 5.0)])
def test_row_ownership(native_lib, bufs, oracle_mod, kind, radius):
    """Bands and stripes that cut tiles on a 37 x 45 film: the owned rows get the oracle's
    convolution of exactly those rows, every other row keeps the prior film's bits."""
    from directcomputeraytracing_amd import WavefrontPathTracer
    from directcomputeraytracing_amd.partition import band_owned_rows, halo_for_radius, owned_rows, row_runs
    W, H = 37, 45
    images = random_images(np.random.default_rng(5), W, H, 3)
    prior = prior_film(W, H)
    filt = make_filter(kind, radius)
    halo = halo_for_radius(radius, H)
    bands = [(5, 21), (30, 45)]
    t = WavefrontPathTracer(path_pool_size=1 << 14)
    try:
        size_film(t, W, H)
        for what, owned in (("bands", band_owned_rows(H, bands)), ("stripes", owned_rows(H, 3, 1, 16))):
            if what == "bands":
                t.set_film_bands(bands, halo)
            else:
                t.set_film_partition(3, 1, 16, halo)
            assert 0 < owned.sum() < H
            film = gpu_accumulate(t, bufs, filt, images, prior)
            ref = oracle_accumulate(oracle_mod, filt, images, prior, row_runs=row_runs(np.nonzero(owned)[0]))
            assert_same_film(film, ref, f"{what} kind {kind}")
            assert np.array_equal(film[~owned].view(np.uint32), prior[~owned].view(np.uint32))
            assert not np.array_equal(film[owned], prior[owned])
    finally:
        t.destroy()


def test_lanczos_tau_zero_is_tau_three(film_tracer, bufs, oracle_mod):
    from directcomputeraytracing_amd import FILTER_LANCZOS
    images = random_images(np.random.default_rng(11), 37, 29, 2)
    films = [gpu_accumulate(film_tracer, bufs, make_filter(FILTER_LANCZOS, 2.3, tau=tau), images) for tau in (0, 3, 2)]
    assert np.isfinite(films[0]).all()
    assert_same_film(films[0], films[1], "tau 0 against tau 3")
    assert_same_film(films[0], oracle_accumulate(oracle_mod, make_filter(FILTER_LANCZOS, 2.3, tau=0), images), "tau 0")
    assert not np.array_equal(films[1], films[2])


def test_invalid_filters_are_refused(native_lib, bufs, golden_luts, oracle_mod):
    """Every entry point that takes a filter refuses an unknown kind and a radius that is NaN,
    negative or 2^30 and more, with INVALID_ARG and a text; the film is untouched and the tracer
    still renders."""
    from directcomputeraytracing_amd import DCRTError, WavefrontPathTracer
    W, H = 32, 24
    s = cornell(W, H, 2)
    (pos, val), = random_images(np.random.default_rng(1), W, H, 1)
    p, v = bufs.upload(pos), bufs.upload(val)
    t = WavefrontPathTracer(path_pool_size=1 << 14)
    try:
        t.set_luts(golden_luts)
        t.on_scene_loaded(s)
        good = t.filter
        t.clear_film()
        t.render_images(0, 1)
        before = t.read_film()
        for kind, radius, text in ((5, 1.0, "unknown"), (0xFFFFFFFF, 1.0, "unknown"), (0, float("nan"), "NaN"),
                                   (2, -1.0, "negative"), (0, float("inf"), r"2\^30"), (4, 2.0 ** 30, r"2\^30")):
            bad = make_filter(kind, radius)
            for call in (lambda: t.render_images(1, 1, bad), lambda: t.render_images(1, 2, bad, seed_stride=2),
                         lambda: t.render_images(1, 1, bad, convolve=False), lambda: t.accumulate_film(bad),
                         lambda: t.accumulate_images([p], [v], bad)):
                with pytest.raises(DCRTError, match="INVALID_ARG.*" + text):
                    call()
        assert np.array_equal(t.read_film().view(np.uint32), before.view(np.uint32))
        t.render_images(1, 1)
        film = t.read_film()
    finally:
        t.destroy()
    flat = oracle_mod.flat_with_own_bvh(s)
    ref = np.zeros_like(film)
    for seed in (0, 1):
        sp, sv, _, _ = oracle_mod.render(flat, golden_luts, oracle_mod.frame_params(s, seed), oracle_mod.WAVEFRONT)
        oracle_mod.sample_convolution(good, sp, sv, ref)
        if seed == 0:
            assert_same_film(before, ref, "before the refusals")
    assert_same_film(film, ref, "after the refusals")


# ---- film sum and copy ---------------------------------------------------------------------------
def awkward_film(W, H, seed):
    """Random values with inf, -inf, nan, denormals, -0 and huge values among them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4.0, 4.0, (H, W, 4)).astype(np.float32)
    flat = x.reshape(-1)
    specials = np.array([np.inf, -np.inf, np.nan, 1e-40, -1e-45, -0.0, 0.0, 3e38, -3e38, 1.1754944e-38], np.float32)
    where = rng.permutation(flat.size)[:20 * len(specials)]
    flat[where] = np.tile(specials, 20)
    return x


def test_film_sum_and_copy(film_tracer, bufs):
    """clear_film + add_film_device(x) loads x (0 + x in float32: -0 becomes +0), a second
    add_film_device(y) gives float32 x + y (inf + -inf included), copy_film_device returns the
    film's bits; 37 x 29 = 1073 float4, no multiple of a block."""
    W, H = 37, 29
    size_film(film_tracer, W, H)
    x, y = awkward_film(W, H, 1), awkward_film(W, H, 2)
    # specials meet specials: inf + -inf, denormal + denormal, overflow, nan + inf, x + -x, -0 + -0
    x[0, 0], y[0, 0] = (np.inf, 1e-40, 3e38, np.nan), (-np.inf, 2e-41, 3e38, np.inf)
    x[-1, -1], y[-1, -1] = (1.5, -0.0, -np.inf, 1e-45), (-1.5, -0.0, -np.inf, -1e-45)
    load_film(film_tracer, bufs, x)
    loaded = film_tracer.read_film()
    zero = np.zeros_like(x)
    assert same_bits(loaded, zero + x).all()
    plain = ~np.isnan(x) & ~((x == 0) & np.signbit(x))
    assert np.array_equal(loaded.view(np.uint32)[plain], x.view(np.uint32)[plain])
    assert not np.signbit(loaded[x == 0]).any()
    film_tracer.add_film_device(bufs.upload(y))
    total = film_tracer.read_film()
    with np.errstate(invalid="ignore", over="ignore"):
        expected = (zero + x) + y
    assert same_bits(total, expected).all()
    assert np.isnan(expected[0, 0, 0]) and 1.1e-40 < expected[0, 0, 1] < 1.3e-40 and np.isinf(expected[0, 0, 2])
    dst = bufs.filled((H, W, 4), -7.0)
    film_tracer.copy_film_device(dst)
    assert np.array_equal(bufs.download(dst).view(np.uint32), total.view(np.uint32))


# ---- luminance reduction and tone mapping --------------------------------------------------------
def resolve_and_compare(t, oracle_mod, film, params, what):
    from directcomputeraytracing_amd import PostFxParams, srgb_thresholds
    th = srgb_thresholds()
    want_sum = np.float32(oracle_mod.sum_log_luminance(film))
    for p in params:
        prm = PostFxParams(*p)
        img, lum = t.resolve_image(prm, with_luminance=True)
        assert same_bits(np.float32(lum), want_sum), f"{what}: sum of log luminance {lum!r} against {want_sum!r}"
        ref = oracle_mod.resolve_image(film, prm, th)
        bad = (img != ref).any(-1)
        assert not bad.any(), f"{what} {p}: {int(bad.sum())} pixels differ, first at {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("W,H", film_ref.POSTFX_SIZES, ids=[f"{w}x{h}" for w, h in film_ref.POSTFX_SIZES])
def test_resolve_sizes(film_tracer, bufs, oracle_mod, W, H):
    """One, two and three passes of the luminance reduction (up to 128, up to 16384, more partial
    sums) and ragged films, random films with weights other than 1, every parameter set (one at
    the three-pass size, where the oracle takes seconds)."""
    size_film(film_tracer, W, H)
    load_film(film_tracer, bufs, film_ref.synthetic_film(W, H, 7 * W + H))
    film = film_tracer.read_film()
    params = film_ref.POSTFX_PARAMETERS[:1] if W * H > 1 << 20 else film_ref.POSTFX_PARAMETERS
    resolve_and_compare(film_tracer, oracle_mod, film, params, f"{W}x{H}")


def test_resolve_cleared_film(film_tracer, bufs, oracle_mod):
    """The film right after clear_film (every weight 0), an ordinary state of a frame loop."""
    size_film(film_tracer, 33, 19)
    film_tracer.clear_film()
    film = film_tracer.read_film()
    assert not film.any()
    resolve_and_compare(film_tracer, oracle_mod, film, film_ref.POSTFX_PARAMETERS, "cleared film")


def test_resolve_awkward_texels(film_tracer, bufs, oracle_mod):
    """Zero and negative weights, negative lobes, inf, nan, overflowing and tiny colours."""
    W, H = 33, 19
    texels = np.array([(0, 0, 0, 0), (1, 2, 3, 0), (-1, -2, 0.5, 1), (np.inf, 1, 1, 1), (np.nan, 1, 1, 1),
                       (1e30, 1e30, 1e30, 1e-8), (1, 1, 1, -1), (1e-30, 1e-30, 1e-30, 1)], np.float32)
    film = film_ref.synthetic_film(W, H, 5)
    flat = film.reshape(-1, 4)
    for k, texel in enumerate(texels):
        flat[k * 3::41] = texel
    flat[0], flat[-1] = texels[4], texels[3]
    size_film(film_tracer, W, H)
    load_film(film_tracer, bufs, film)
    loaded = film_tracer.read_film()
    assert same_bits(loaded, film).all()
    resolve_and_compare(film_tracer, oracle_mod, loaded, [(1, 1, 0.0, 1.0), (1, 0, 0.0, 1.0), (1, 0, 6.0, 0.5), (0, 0, 0.0, 1.0)],
                        "awkward texels")
