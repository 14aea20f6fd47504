"""The numpy float32 restatement of the film denoiser (tests/denoise_ref.py) pinned by itself, so
the GPU tests' yardstick is not only "what the kernel does": against a float64 B3-spline
convolution, on constant and zero images, across a guide edge, and on a synthetic noisy image
where a purely colour-weighted a-trous filter does far worse. No GPU needed; the library's
parameter defaults are checked here too."""
import ctypes as C

import numpy as np

import denoise_ref as ref

F = np.float32
OFF = dict(sigma_luminance=0.0, sigma_normal=0.0, sigma_albedo=0.0)


def _flat_guides(W, H, normal=(0.0, 0.0, 1.0), albedo=(0.5, 0.5, 0.5)):
    n = np.broadcast_to(np.asarray(normal, np.float32), (H, W, 3))
    a = np.broadcast_to(np.asarray(albedo, np.float32), (H, W, 3))
    return ref.film(ref.encode_normal(n)), ref.film(a)


def test_plain_b3_convolution(oracle_mod):
    """All sigmas 0, one pass, no demodulation: interior pixels are the 5 x 5 B3-spline
    convolution (float64) to 1e-6 absolute."""
    rng = np.random.default_rng(1)
    W, H = 23, 17
    rgb = rng.random((H, W, 3)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, (H, W)).astype(np.float32)
    normal, albedo = _flat_guides(W, H)
    out = ref.denoise(ref.film(rgb, w), normal, albedo, iterations=1, demodulate=0, **OFF)
    c = ref.resolve(ref.film(rgb, w)).astype(np.float64)
    h = np.array([1, 4, 6, 4, 1], np.float64) / 16.0
    want = np.zeros((H - 4, W - 4, 3))
    for dy in range(5):
        for dx in range(5):
            want += h[dy] * h[dx] * c[dy:dy + H - 4, dx:dx + W - 4]
    err = np.abs(out[2:-2, 2:-2, :3].astype(np.float64) - want).max()
    print("B3 convolution: max abs error", err)
    assert err <= 1e-6
    assert (out[..., 3] == 1).all()


def test_constant_image_stays_constant(oracle_mod):
    """A constant image (zero variance) stays constant to 1e-6 relative, and finite."""
    W, H = 21, 13
    value = np.array([0.37, 1.5, 0.004], np.float32)
    w = np.random.default_rng(2).uniform(0.5, 3.0, (H, W)).astype(np.float32)
    normal, albedo = _flat_guides(W, H, albedo=(0.8, 0.25, 0.0))   # (one channel below the demodulation floor)
    out = ref.denoise(ref.film(np.broadcast_to(value, (H, W, 3)), w), normal, albedo, **ref.DEFAULTS)
    assert np.isfinite(out).all()
    c = ref.resolve(ref.film(np.broadcast_to(value, (H, W, 3)), w))   # (w * v / w: the constant to an ulp)
    rel = np.abs(out[..., :3].astype(np.float64) / c.astype(np.float64) - 1.0).max()
    print("constant image: max relative error", rel)
    assert rel <= 1e-6


def test_zero_image_and_empty_pixels(oracle_mod):
    """All-zero colour -> all zero; pixels without weight resolve to 0 and make no NaN."""
    W, H = 9, 7
    normal, albedo = _flat_guides(W, H)
    zero = np.zeros((H, W, 4), np.float32)
    out = ref.denoise(zero, normal, albedo, **ref.DEFAULTS)
    assert (out[..., :3] == 0).all() and (out[..., 3] == 1).all()
    # guides without weight as well (a miss everywhere)
    out = ref.denoise(zero, zero, zero, **ref.DEFAULTS)
    assert np.isfinite(out).all() and (out[..., :3] == 0).all()
    rng = np.random.default_rng(3)
    color = ref.film(rng.random((H, W, 3)), np.where(rng.random((H, W)) < 0.3, 0.0, 1.0))
    out = ref.denoise(color, normal, albedo, **ref.DEFAULTS)
    assert np.isfinite(out).all()


def test_edge_isolation(oracle_mod):
    """sigma_luminance = 0, sigma_normal = 0.1, perpendicular unit normals in the two halves:
    |dn|^2 * kn = 200 and det_exp(-200) is exactly 0, so the left half's output does not depend
    on the right half's colours -- bit for bit. (With sigma_luminance > 0 it would: the 3 x 3
    variance prefilter is unguided.)"""
    assert ref.det_exp(np.array([-200.0], np.float32))[0] == 0.0
    rng = np.random.default_rng(4)
    W, H = 26, 15
    nrm = np.zeros((H, W, 3), np.float32)
    nrm[:, :W // 2] = (1.0, 0.0, 0.0)
    nrm[:, W // 2:] = (0.0, 1.0, 0.0)
    normal = ref.film(ref.encode_normal(nrm))
    _, albedo = _flat_guides(W, H)
    rgb = rng.random((H, W, 3)).astype(np.float32)
    other = rgb.copy()
    other[:, W // 2:] = rng.uniform(0.0, 50.0, (H, W - W // 2, 3))
    prm = dict(iterations=4, sigma_luminance=0.0, sigma_normal=0.1, sigma_albedo=0.1, demodulate=1)
    a = ref.denoise(ref.film(rgb), normal, albedo, **prm)
    b = ref.denoise(ref.film(other), normal, albedo, **prm)
    assert ref.same_bits(a[:, :W // 2], b[:, :W // 2]).all()
    assert not ref.same_bits(a[:, W // 2:], b[:, W // 2:]).all()


def test_noise_reduction_on_synthetic_image(oracle_mod):
    """48 x 40, log-normal noise of sigma 0.5: the denoised RMSE against the clean image is below
    half the noisy one with the default parameters (measured 0.22; a colour-only a-trous filter
    gives 0.75 - 0.97 on this image, and a regression to it fails here)."""
    clean, color, normal, albedo = ref.synthetic_scene(noise_sigma=0.5, seed=7)
    out = ref.denoise(color, normal, albedo, **ref.DEFAULTS)
    noisy = ref.rmse(ref.resolve(color), clean)
    ratio = ref.rmse(out[..., :3], clean) / noisy
    print("synthetic image: noisy RMSE", noisy, "denoised / noisy", ratio)
    assert ratio < 0.5


def test_default_params(native_lib):
    """dcrt_denoise_default_params: the documented defaults, without a device."""
    from directcomputeraytracing_amd import _abi, denoise_default_params
    assert C.sizeof(_abi.DenoiseParams) == 20
    p = _abi.DenoiseParams(9, -1.0, -1.0, -1.0, 7)
    assert native_lib.dcrt_denoise_default_params(C.byref(p)) == 0
    assert (p.iterations, p.demodulate) == (5, 1)
    assert (F(p.sigma_luminance), F(p.sigma_normal), F(p.sigma_albedo)) == (F(4.0), F(0.2), F(0.1))
    assert native_lib.dcrt_denoise_default_params(None) == -1
    q = denoise_default_params()
    assert {k: getattr(q, k) for k, _ in q._fields_} == {k: getattr(p, k) for k, _ in p._fields_}
    assert {k: F(v) for k, v in ref.DEFAULTS.items()} == {k: F(getattr(p, k)) for k in ref.DEFAULTS}


def test_null_tracer_is_refused(native_lib):
    from directcomputeraytracing_amd import _abi
    p = _abi.DenoiseParams(5, 4.0, 0.2, 0.1, 1)
    assert native_lib.dcrt_tracer_render_guides(None, 0, 1) == -1
    assert native_lib.dcrt_tracer_denoise(None, C.byref(p)) == -1
    assert native_lib.dcrt_tracer_read_denoised(None, None) == -1
    assert native_lib.dcrt_tracer_denoise_device(None, C.byref(p), 4, 4, None, None, None, None) == -1
