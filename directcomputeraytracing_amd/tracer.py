"""``CWavefrontPathTracer`` (Source/WavefrontPathTracer.h:7-101) on MI355X.

A thin host mirror over the C ABI: every call goes to ``libdcrt.so`` (gfx950
kernels). Method names follow the reference's ``CPathTracer`` interface
(Source/PathTracer.h:3-31): ``create``/``destroy``/``on_scene_loaded``/
``render``/``reset_image``/``is_image_complete``/``acquire_film_clear_trigger``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check
from .scene import Scene

RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("t_min", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("triangle_id", "<u4"), ("instance_index", "<u4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 20

MATH_SIN, MATH_COS, MATH_EXP, MATH_ATAN = range(4)

# set_output's names for the DCRT_OUTPUT_* views (s_OutputNames, MegakernelPathTracer.cpp:360)
OUTPUT_NAMES = {"path_tracing": _abi.OUTPUT_PATH_TRACING, "normal": _abi.OUTPUT_SHADING_NORMAL,
                "tangent": _abi.OUTPUT_SHADING_TANGENT, "albedo": _abi.OUTPUT_ALBEDO,
                "negative_ndotv": _abi.OUTPUT_NEGATIVE_NDOTV, "backface": _abi.OUTPUT_BACKFACE,
                "iteration_count": _abi.OUTPUT_ITERATION_COUNT}


def make_rays(origins, directions, t_min=0.0, t_max=np.inf) -> np.ndarray:
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    r = np.zeros(len(o), RAY_DTYPE)
    r["origin"], r["direction"] = o, d
    r["t_min"], r["t_max"] = t_min, t_max
    return r


class WavefrontPathTracer:
    """CWavefrontPathTracer: path pool, queues and kernels resident in HBM."""

    def __init__(self, path_pool_size: int = 0, iterations_per_render: int = 0, device: int = 0,
                 stream: int | None = None, debug_rng: bool = False):
        self._lib = _abi.load_library()
        self._h = None
        self.create(path_pool_size, iterations_per_render, device, stream, debug_rng)

    # ---- CPathTracer --------------------------------------------------------
    def create(self, path_pool_size=0, iterations_per_render=0, device=0, stream=None, debug_rng=False):
        cfg = _abi.TracerConfig(int(path_pool_size), int(iterations_per_render), int(device),
                                C.c_void_p(stream or 0), 1 if debug_rng else 0)
        h = C.c_void_p()
        check(self._lib.dcrt_tracer_create(C.byref(cfg), C.byref(h)), "Create")
        self._h = h
        self.width = self.height = 0
        self.env_cube_size = 0
        self.filter = _abi.FilterParams(_abi.FILTER_BOX, 1.0, 1.5, 1 / 3, 1 / 3, 3)

    def destroy(self):
        if self._h:
            self._lib.dcrt_tracer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def on_scene_loaded(self, scene: Scene, frame_seed: int = 0) -> None:
        """Upload the flattened scene and the camera/film constants (OnSceneLoaded)."""
        flat = scene.flat()
        check(self._lib.dcrt_tracer_upload_scene(self._h, C.byref(flat)), "OnSceneLoaded")
        self.env_cube_size = int(flat.env_cube_size) if flat.env_cube_rgb else 0
        self.set_frame_params(scene.frame_params(frame_seed))
        self.filter = scene.filter_params()

    # ---- partial scene updates (UpdateMaterial / Light / InstanceFlagsGPUData, Scene.cpp:672-807)
    def update_materials(self, scene: Scene) -> None:
        f = scene.flat()
        check(self._lib.dcrt_tracer_update_materials(self._h, f.materials, f.material_count), "UpdateMaterials")

    def update_lights(self, scene: Scene) -> None:
        f = scene.flat()
        check(self._lib.dcrt_tracer_update_lights(self._h, f.lights, f.light_count), "UpdateLights")

    def update_instance_flags(self, scene: Scene) -> None:
        f = scene.flat()
        check(self._lib.dcrt_tracer_update_instance_flags(self._h, f.instance_flags, f.instance_count), "UpdateInstanceFlags")

    def upload_stats(self) -> dict:
        s = _abi.UploadStats()
        check(self._lib.dcrt_tracer_upload_stats(self._h, C.byref(s)), "UploadStats")
        return {k: getattr(s, k) for k, _ in _abi.UploadStats._fields_}

    def apply_edits(self, scene: Scene, bits: int, frame_seed: int = 0) -> None:
        """Bring the tracer up to the scene's edits: `bits` from scene.acquire_dirty() (an
        argument, so every pipeline of make_pipelines applies the same acquired bits). DIRTY_SCENE
        is the full on_scene_loaded; otherwise only the arrays the bits name are sent. The frame
        parameters (camera, light count) are always re-sent. The image is the caller's to restart
        (reset_image), as in the reference's frame loop."""
        if bits & _abi.DIRTY_SCENE:
            self.on_scene_loaded(scene, frame_seed)
            return
        if bits & _abi.DIRTY_MATERIALS:
            self.update_materials(scene)
        if bits & _abi.DIRTY_LIGHTS:
            self.update_lights(scene)
        if bits & _abi.DIRTY_INSTANCE_FLAGS:
            self.update_instance_flags(scene)
        self.set_frame_params(scene.frame_params(frame_seed))

    def set_frame_params(self, params: _abi.FrameParams) -> None:
        check(self._lib.dcrt_tracer_set_frame_params(self._h, C.byref(params)), "SetFrameParams")
        self.width, self.height = params.resolution[0], params.resolution[1]

    def set_film_partition(self, world_size: int, rank: int, stripe_height: int = 64, halo_rows: int = 0) -> None:
        p = _abi.FilmPartition(world_size, rank, stripe_height, halo_rows)
        check(self._lib.dcrt_tracer_set_film_partition(self._h, C.byref(p)), "SetFilmPartition")

    def set_film_bands(self, bands, halo_rows: int = 0) -> None:
        """Own the rows of the (y0, y1) bands (ascending, disjoint), path-trace them plus halo_rows
        beyond each and convolve only them (dcrt_tracer_set_film_bands)."""
        flat = np.asarray([y for b in bands for y in b], np.uint32)
        check(self._lib.dcrt_tracer_set_film_bands(self._h, flat.ctypes.data_as(C.POINTER(C.c_uint32)), len(bands),
                                                   int(halo_rows)), "SetFilmBands")

    def set_row_cost_probe(self, enable: bool) -> None:
        """Count the rays cast per film row from now on (cleared when turned on)."""
        check(self._lib.dcrt_tracer_set_row_cost_probe(self._h, 1 if enable else 0), "SetRowCostProbe")

    def read_row_cost(self) -> np.ndarray:
        out = np.empty(self.height, np.uint32)
        check(self._lib.dcrt_tracer_read_row_cost(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))), "ReadRowCost")
        return out

    def render(self, max_iterations: int = 0) -> None:
        check(self._lib.dcrt_tracer_render(self._h, int(max_iterations)), "Render")

    def render_images(self, first_seed: int, count: int, filter_params: _abi.FilterParams | None = None,
                      seed_stride: int = 1, convolve: bool = True) -> None:
        """Images first_seed + k * seed_stride, k < count; convolve=False keeps every image's
        samples (slot k) for accumulate_images instead of running the film pass."""
        f = filter_params or self.filter
        if seed_stride == 1 and convolve:
            check(self._lib.dcrt_tracer_render_images(self._h, int(first_seed), int(count), C.byref(f)), "RenderImages")
        else:
            check(self._lib.dcrt_tracer_render_images_strided(self._h, int(first_seed), int(seed_stride), int(count),
                                                              1 if convolve else 0, C.byref(f)), "RenderImagesStrided")

    def image_sample_ptrs(self, image: int) -> tuple[int, int]:
        pos, val = C.c_void_p(), C.c_void_p()
        check(self._lib.dcrt_tracer_image_sample_ptrs(self._h, int(image), C.byref(pos), C.byref(val)), "ImageSamplePtrs")
        return pos.value or 0, val.value or 0

    def accumulate_images(self, positions, values, filter_params: _abi.FilterParams | None = None) -> None:
        """SampleConvolution of the images whose sample textures sit at these device pointers, in order."""
        f = filter_params or self.filter
        n = len(positions)
        P = (C.c_void_p * max(1, n))(*positions)
        V = (C.c_void_p * max(1, n))(*values)
        check(self._lib.dcrt_tracer_accumulate_images(self._h, P, V, n, C.byref(f)), "AccumulateImages")

    def prepare_images(self, count: int) -> None:
        """Allocate / capture what render_images(count) would on its first call."""
        check(self._lib.dcrt_tracer_prepare_images(self._h, int(count)), "PrepareImages")

    def set_image_batch(self, images: int = 0) -> None:
        """Images per render_images batch (0 = automatic)."""
        check(self._lib.dcrt_tracer_set_image_batch(self._h, int(images)), "SetImageBatch")

    def set_mode(self, mode: str) -> None:
        """"wavefront" (CWavefrontPathTracer) or "megakernel" (CMegakernelPathTracer) for render_images."""
        check(self._lib.dcrt_tracer_set_mode(self._h, {"wavefront": 0, "megakernel": 1}[mode]), "SetMode")

    def set_output(self, output, iteration_threshold: int = 20) -> None:
        """The "Output" view: an OUTPUT_NAMES key or a DCRT_OUTPUT_* int. Anything but
        "path_tracing" makes render / render_images draw the camera rays' first hits (normal,
        tangent, albedo, facing flags) or their BVH node visits over iteration_threshold."""
        kind = OUTPUT_NAMES[output] if isinstance(output, str) else int(output)
        p = _abi.OutputParams(kind, int(iteration_threshold))
        check(self._lib.dcrt_tracer_set_output(self._h, C.byref(p)), "SetOutput")

    def output(self) -> tuple[str, int]:
        """(view name, iteration threshold) as set_output takes them."""
        p = _abi.OutputParams()
        check(self._lib.dcrt_tracer_get_output(self._h, C.byref(p)), "GetOutput")
        return {v: k for k, v in OUTPUT_NAMES.items()}[p.output_type], int(p.iteration_threshold)

    def reset_image(self) -> None:
        check(self._lib.dcrt_tracer_reset_image(self._h), "ResetImage")

    def is_image_complete(self) -> bool:
        v = C.c_int()
        check(self._lib.dcrt_tracer_is_image_complete(self._h, C.byref(v)), "IsImageComplete")
        return bool(v.value)

    def acquire_film_clear_trigger(self) -> bool:
        v = C.c_int()
        check(self._lib.dcrt_tracer_acquire_film_clear_trigger(self._h, C.byref(v)), "AcquireFilmClearTrigger")
        return bool(v.value)

    # ---- film --------------------------------------------------------------
    def clear_film(self) -> None:
        check(self._lib.dcrt_tracer_clear_film(self._h), "ClearFilm")

    def accumulate_film(self, filter_params: _abi.FilterParams | None = None) -> None:
        f = filter_params or self.filter
        check(self._lib.dcrt_tracer_accumulate_film(self._h, C.byref(f)), "SampleConvolution")

    def read_film(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), np.float32)
        check(self._lib.dcrt_tracer_read_film(self._h, out.ctypes.data_as(_abi._FP)), "ReadFilm")
        return out

    def read_samples(self):
        pos = np.empty((self.height, self.width, 2), np.float32)
        val = np.empty((self.height, self.width, 4), np.float32)
        check(self._lib.dcrt_tracer_read_samples(self._h, pos.ctypes.data_as(_abi._FP), val.ctypes.data_as(_abi._FP)),
              "ReadSamples")
        return pos, val

    def read_rng(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), np.uint32)
        check(self._lib.dcrt_tracer_read_rng(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))), "ReadRng")
        return out

    def film_device_ptr(self) -> int:
        p = C.c_void_p()
        check(self._lib.dcrt_tracer_film_device_ptr(self._h, C.byref(p)), "FilmDevicePtr")
        return p.value or 0

    def sample_device_ptrs(self) -> tuple[int, int]:
        """Device pointers of the current image's sample textures (R32G32F positions, RGBA32F
        values): what the reference's SampleConvolution pass reads."""
        pos, val = C.c_void_p(), C.c_void_p()
        check(self._lib.dcrt_tracer_sample_device_ptrs(self._h, C.byref(pos), C.byref(val)), "SampleDevicePtrs")
        return pos.value or 0, val.value or 0

    def copy_film_device(self, d_dst: int) -> None:
        check(self._lib.dcrt_tracer_copy_film_device(self._h, C.c_void_p(d_dst)), "CopyFilmDevice")

    def add_film_device(self, d_src: int) -> None:
        """film += the RGBA32F film at device address d_src (another partition's film)."""
        check(self._lib.dcrt_tracer_add_film_device(self._h, C.c_void_p(d_src)), "AddFilmDevice")

    def resolve_image(self, params: _abi.PostFxParams | None = None, with_luminance: bool = False, denoised: bool = False,
                      firefly: bool = False):
        """Post-processing (exposure + Reinhard) into sRGB8 RGBA, H x W x 4 uint8: of the film, or
        with denoised=True of the last denoise()'s image, or with firefly=True of the last
        firefly_filtered()'s."""
        p = params or _abi.PostFxParams(1, 1, 15.0, 1.0)
        out = np.empty((self.height, self.width, 4), np.uint8)
        lum = C.c_float()
        fn, what = (self._lib.dcrt_tracer_resolve_image, "ResolveImage")
        if denoised:
            fn, what = (self._lib.dcrt_tracer_resolve_denoised, "ResolveDenoised")
        elif firefly:
            fn, what = (self._lib.dcrt_tracer_resolve_firefly, "ResolveFirefly")
        check(fn(self._h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(lum)), what)
        return (out, lum.value) if with_luminance else out

    # ---- film denoiser ---------------------------------------------------------
    def render_guides(self, first_seed: int, count: int) -> None:
        """The denoiser's guide films of images first_seed .. first_seed + count - 1 (the seeds the
        film was rendered with): first-hit shading normal and albedo, convolved with the film's
        filter. Overwrites the sample textures; the film and the selected output stay."""
        check(self._lib.dcrt_tracer_render_guides(self._h, int(first_seed), int(count)), "RenderGuides")

    def read_guides(self):
        """(normal film, albedo film), H x W x 4 float32 each, in film convention."""
        nrm = np.empty((self.height, self.width, 4), np.float32)
        alb = np.empty((self.height, self.width, 4), np.float32)
        check(self._lib.dcrt_tracer_read_guides(self._h, nrm.ctypes.data_as(_abi._FP), alb.ctypes.data_as(_abi._FP)), "ReadGuides")
        return nrm, alb

    def guide_device_ptrs(self) -> tuple[int, int]:
        nrm, alb = C.c_void_p(), C.c_void_p()
        check(self._lib.dcrt_tracer_guide_device_ptrs(self._h, C.byref(nrm), C.byref(alb)), "GuideDevicePtrs")
        return nrm.value or 0, alb.value or 0

    def denoise(self, params: _abi.DenoiseParams | None = None, firefly: bool = False) -> np.ndarray:
        """Filter the film -- with firefly=True the re-weighted image of the last firefly_filtered() -- with the
        rendered guides; returns the denoised image (H x W x 4 float32, film convention with w = 1), which
        resolve_image(denoised=True) tone-maps."""
        p = params or denoise_default_params()
        if firefly:
            check(self._lib.dcrt_tracer_denoise_firefly(self._h, C.byref(p)), "DenoiseFirefly")
        else:
            check(self._lib.dcrt_tracer_denoise(self._h, C.byref(p)), "Denoise")
        out = np.empty((self.height, self.width, 4), np.float32)
        check(self._lib.dcrt_tracer_read_denoised(self._h, out.ctypes.data_as(_abi._FP)), "ReadDenoised")
        return out

    def denoised_device_ptr(self) -> int:
        p = C.c_void_p()
        check(self._lib.dcrt_tracer_denoised_device_ptr(self._h, C.byref(p)), "DenoisedDevicePtr")
        return p.value or 0

    def denoise_images(self, color, normal, albedo, params: _abi.DenoiseParams | None = None) -> np.ndarray:
        """The same filter over host images (H x W x 4 float32, film convention)."""
        p = params or denoise_default_params()
        c, n, a = (np.ascontiguousarray(x, np.float32) for x in (color, normal, albedo))
        if c.ndim != 3 or c.shape[2] != 4 or n.shape != c.shape or a.shape != c.shape:
            raise ValueError("denoise_images: three H x W x 4 images of one shape")
        out = np.empty_like(c)
        check(self._lib.dcrt_tracer_denoise_images(self._h, C.byref(p), c.shape[1], c.shape[0], c.ctypes.data_as(_abi._FP),
                                                   n.ctypes.data_as(_abi._FP), a.ctypes.data_as(_abi._FP),
                                                   out.ctypes.data_as(_abi._FP)), "DenoiseImages")
        return out

    def denoise_device(self, width: int, height: int, d_color: int, d_normal: int, d_albedo: int, d_out: int,
                       params: _abi.DenoiseParams | None = None) -> None:
        """... over device images, e.g. the reduced films of a multi-GPU render; d_out may not overlap an input."""
        p = params or denoise_default_params()
        check(self._lib.dcrt_tracer_denoise_device(self._h, C.byref(p), int(width), int(height), C.c_void_p(d_color),
                                                   C.c_void_p(d_normal), C.c_void_p(d_albedo), C.c_void_p(d_out)), "DenoiseDevice")

    def denoise_timings(self) -> list:
        """ms per kernel of the last denoise (prologue, variance, passes) with ext_timing on."""
        ms = (C.c_float * 16)()
        n = C.c_uint32()
        check(self._lib.dcrt_tracer_denoise_timings(self._h, ms, 16, C.byref(n)), "DenoiseTimings")
        return [float(ms[i]) for i in range(min(16, n.value))]

    # ---- firefly re-weighting (include/dcrt.h) ------------------------------------------
    def set_firefly_filter(self, params: _abi.FireflyParams | None) -> None:
        """Firefly re-weighting (off by default): with params, keep K cascade films beside the film and feed them in
        every film pass; None switches it off and frees them. Either way the film, the half film and the cascades
        are cleared and the film image count is reset. Needs the frame parameters (a film)."""
        check(self._lib.dcrt_tracer_set_firefly(self._h, C.byref(params) if params is not None else None), "SetFirefly")

    def firefly_filter(self) -> _abi.FireflyParams | None:
        """The parameters while firefly re-weighting is on, else None."""
        on, p = C.c_int(), _abi.FireflyParams()
        check(self._lib.dcrt_tracer_get_firefly(self._h, C.byref(on), C.byref(p)), "GetFirefly")
        return p if on.value else None

    def firefly_filtered(self) -> np.ndarray:
        """Resolve the film and its cascades; returns the re-weighted image (H x W x 4 float32, film convention
        with w = 1), which resolve_image(firefly=True) tone-maps and denoise_device takes as its colour input."""
        check(self._lib.dcrt_tracer_firefly_resolve(self._h), "FireflyResolve")
        out = np.empty((self.height, self.width, 4), np.float32)
        check(self._lib.dcrt_tracer_read_firefly(self._h, out.ctypes.data_as(_abi._FP)), "ReadFirefly")
        return out

    def firefly_device_ptr(self) -> int:
        p = C.c_void_p()
        check(self._lib.dcrt_tracer_firefly_device_ptr(self._h, C.byref(p)), "FireflyDevicePtr")
        return p.value or 0

    def read_cascades(self) -> np.ndarray:
        """The cascade films, K x H x W x 4 float32 (rgb: the band's share of sum w * L; w: 0)."""
        p = self.firefly_filter()
        if p is None:
            raise _abi.DCRTError("ReadCascades failed (DCRT_E_INVALID_ARG): firefly re-weighting is off")
        out = np.empty((int(p.cascades), self.height, self.width, 4), np.float32)
        check(self._lib.dcrt_tracer_read_cascades(self._h, out.ctypes.data_as(_abi._FP)), "ReadCascades")
        return out

    def cascade_device_ptrs(self) -> list:
        ptrs = (C.c_void_p * 8)()
        n = C.c_uint32()
        check(self._lib.dcrt_tracer_cascade_device_ptrs(self._h, ptrs, 8, C.byref(n)), "CascadeDevicePtrs")
        return [ptrs[i] or 0 for i in range(n.value)]

    def firefly_resolve_device(self, width: int, height: int, image_count: int, d_film: int, d_cascades, d_out: int,
                               params: _abi.FireflyParams | None = None) -> None:
        """The resolve over device images, e.g. the reduced film and cascades of a multi-GPU render: d_cascades holds
        params.cascades device addresses; d_out may not overlap an input."""
        p = params or firefly_default_params()
        ptrs = (C.c_void_p * len(d_cascades))(*[C.c_void_p(int(x)) for x in d_cascades])
        if len(d_cascades) != int(p.cascades):
            raise ValueError("firefly_resolve_device: one device image per cascade")
        check(self._lib.dcrt_tracer_firefly_resolve_device(self._h, C.byref(p), int(width), int(height), int(image_count),
                                                           C.c_void_p(d_film), ptrs, C.c_void_p(d_out)), "FireflyResolveDevice")

    def firefly_timings(self) -> tuple[float, float]:
        """(cascade pass ms, resolve ms) of the last ones that ran with ext_timing on (0: none did)."""
        a, b = C.c_float(), C.c_float()
        check(self._lib.dcrt_tracer_firefly_timings(self._h, C.byref(a), C.byref(b)), "FireflyTimings")
        return float(a.value), float(b.value)

    # ---- film noise estimate, render until converged --------------------------------
    def set_convergence(self, enable: bool) -> None:
        """Keep a half film (every other image of the film's) for noise(); clears the film, the
        half film and the film image count. Needs the frame parameters (a film)."""
        check(self._lib.dcrt_tracer_set_convergence(self._h, 1 if enable else 0), "SetConvergence")

    def film_image_count(self) -> int:
        """Images convolved into the film since the last clear."""
        n = C.c_uint32()
        check(self._lib.dcrt_tracer_film_image_count(self._h, C.byref(n)), "FilmImageCount")
        return int(n.value)

    def half_film_device_ptr(self) -> int:
        p = C.c_void_p()
        check(self._lib.dcrt_tracer_half_film_device_ptr(self._h, C.byref(p)), "HalfFilmDevicePtr")
        return p.value or 0

    def read_half_film(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), np.float32)
        check(self._lib.dcrt_tracer_read_half_film(self._h, out.ctypes.data_as(_abi._FP)), "ReadHalfFilm")
        return out

    def add_half_film_device(self, d_src: int) -> None:
        """half film += the RGBA32F half film at device address d_src (another partition's)."""
        check(self._lib.dcrt_tracer_add_half_film_device(self._h, C.c_void_p(d_src)), "AddHalfFilmDevice")

    def noise(self, threshold: float, maps: bool = False):
        """The half-film noise estimate of the film: a dict of dcrt_noise_stats; with maps=True
        (stats, per-pixel e H x W, tile errors ceil(H / 16) x ceil(W / 16))."""
        s = _abi.NoiseStats()
        check(self._lib.dcrt_tracer_noise(self._h, float(threshold), C.byref(s)), "Noise")
        stats = noise_stats_dict(s)
        return (stats, *self.read_noise_maps()) if maps else stats

    def read_noise_maps(self):
        """(per-pixel e, tile errors) of the last noise()."""
        pix = np.empty((self.height, self.width), np.float32)
        tile = np.empty((-(-self.height // 16), -(-self.width // 16)), np.float32)
        check(self._lib.dcrt_tracer_read_noise_maps(self._h, pix.ctypes.data_as(_abi._FP), tile.ctypes.data_as(_abi._FP)),
              "ReadNoiseMaps")
        return pix, tile

    def noise_map_device_ptrs(self) -> tuple[int, int]:
        pix, tile = C.c_void_p(), C.c_void_p()
        check(self._lib.dcrt_tracer_noise_map_device_ptrs(self._h, C.byref(pix), C.byref(tile)), "NoiseMapDevicePtrs")
        return pix.value or 0, tile.value or 0

    def noise_device(self, width: int, height: int, d_film: int, d_half: int, threshold: float, d_pixel_map: int = 0,
                     d_tile_map: int = 0) -> dict:
        """The estimate over device images (e.g. the reduced film and half film of a multi-GPU
        render); the map destinations are optional."""
        s = _abi.NoiseStats()
        check(self._lib.dcrt_tracer_noise_device(self._h, int(width), int(height), C.c_void_p(d_film), C.c_void_p(d_half),
                                                 float(threshold), C.c_void_p(d_pixel_map or None),
                                                 C.c_void_p(d_tile_map or None), C.byref(s)), "NoiseDevice")
        return noise_stats_dict(s)

    def film_pass_timing(self) -> tuple[int, float]:
        """(launches, ms) of the film passes into the film since reset_stats, with ext_timing on."""
        n, ms = C.c_uint64(), C.c_double()
        check(self._lib.dcrt_tracer_film_pass_timing(self._h, C.byref(n), C.byref(ms)), "FilmPassTiming")
        return int(n.value), float(ms.value)

    def render_converged(self, first_seed: int, params: _abi.ConvergeParams, filter_params: _abi.FilterParams | None = None):
        """Render images first_seed, first_seed + 1, ... until the estimate meets params' target or
        max_images sit in the film: (stats of the last check, converged). The film is not cleared."""
        f = filter_params or self.filter
        s = _abi.NoiseStats()
        done = C.c_int()
        check(self._lib.dcrt_tracer_render_converged(self._h, int(first_seed), C.byref(params), C.byref(f), C.byref(s),
                                                     C.byref(done)), "RenderConverged")
        return noise_stats_dict(s), bool(done.value)

    # ---- adaptive sampling: trace only the film blocks that are still noisy ---------
    FILTER_MARGIN = 0xFFFFFFFF   # margin: the filter's window rows

    def set_adaptive(self, enable: bool) -> None:
        """Keep a list of active 8 x 8 film blocks (index by * ceil(W / 8) + bx) that render_images
        starts paths in; set to every block. Needs a film; not on a partitioned or banded tracer."""
        check(self._lib.dcrt_tracer_set_adaptive(self._h, 1 if enable else 0), "SetAdaptive")

    def set_sample_blocks(self, blocks) -> None:
        """The active blocks: strictly ascending indices; an empty list leaves nothing to sample."""
        b = np.ascontiguousarray(blocks, np.uint32).ravel()
        check(self._lib.dcrt_tracer_set_sample_blocks(self._h, b.ctypes.data_as(C.POINTER(C.c_uint32)), b.size), "SetSampleBlocks")

    def get_sample_blocks(self) -> np.ndarray:
        n = C.c_uint32()
        check(self._lib.dcrt_tracer_get_sample_blocks(self._h, None, 0, C.byref(n)), "GetSampleBlocks")
        out = np.empty(n.value, np.uint32)
        check(self._lib.dcrt_tracer_get_sample_blocks(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)),
              "GetSampleBlocks")
        return out

    def update_sample_blocks(self, threshold: float, margin: int = FILTER_MARGIN) -> int:
        """Rebuild the list from the film and the half film: the blocks with a pixel within `margin`
        pixels that is invalid or whose error is not <= threshold. Returns the list's length."""
        n = C.c_uint32()
        check(self._lib.dcrt_tracer_update_sample_blocks(self._h, float(threshold), int(margin), C.byref(n)), "UpdateSampleBlocks")
        return int(n.value)

    def sample_blocks_device(self, width: int, height: int, d_film: int, d_half: int, threshold: float, margin: int,
                             d_list: int, d_flags: int = 0) -> int:
        """The same over device images: the ascending list at d_list (room for every block), one
        uint32 flag per block at d_flags if given. Returns the count."""
        n = C.c_uint32()
        check(self._lib.dcrt_tracer_sample_blocks_device(self._h, int(width), int(height), C.c_void_p(d_film), C.c_void_p(d_half),
                                                         float(threshold), int(margin), C.c_void_p(d_flags or None),
                                                         C.c_void_p(d_list), C.byref(n)), "SampleBlocksDevice")
        return int(n.value)

    def adaptive_timings(self) -> dict:
        """HIP-event ms of the last mask, compaction and sentinel-fill kernels, with ext_timing on."""
        ms = [C.c_float(), C.c_float(), C.c_float()]
        check(self._lib.dcrt_tracer_adaptive_timings(self._h, *[C.byref(m) for m in ms]), "AdaptiveTimings")
        return {"mask_ms": ms[0].value, "compact_ms": ms[1].value, "fill_ms": ms[2].value}

    def render_adaptive(self, first_seed: int, params: _abi.ConvergeParams, margin: int = FILTER_MARGIN,
                        filter_params: _abi.FilterParams | None = None):
        """render_converged that rebuilds the block list at every check point and renders only the
        listed blocks: (stats of the last check, converged, report dict). Starts on every block;
        the film is not cleared, and the list stays as the last check point left it."""
        f = filter_params or self.filter
        s = _abi.NoiseStats()
        done = C.c_int()
        r = _abi.AdaptiveReport()
        check(self._lib.dcrt_tracer_render_adaptive(self._h, int(first_seed), C.byref(params), int(margin), C.byref(f), C.byref(s),
                                                    C.byref(done), C.byref(r)), "RenderAdaptive")
        return noise_stats_dict(s), bool(done.value), {k: int(getattr(r, k)) for k, _ in _abi.AdaptiveReport._fields_}

    # ---- environment importance sampling (include/dcrt.h) ----------------------------
    ENV_SAMPLING = ("uniform", "importance")

    def set_environment_sampling(self, mode: str) -> None:
        """"uniform" (the default, the reference's sampling) or "importance": light samples follow the
        environment cube's power. Needs an uploaded scene; kept across later uploads; the caller restarts the image."""
        if mode not in self.ENV_SAMPLING:
            raise ValueError(f"environment sampling {mode!r}: one of {self.ENV_SAMPLING}")
        check(self._lib.dcrt_tracer_set_environment_sampling(self._h, self.ENV_SAMPLING.index(mode)), "SetEnvironmentSampling")

    def environment_sampling(self) -> tuple[str, bool]:
        """(mode, active): active while the mode is on and a table stands for the uploaded scene's cube."""
        mode, active = C.c_int(), C.c_int()
        check(self._lib.dcrt_tracer_get_environment_sampling(self._h, C.byref(mode), C.byref(active)), "GetEnvironmentSampling")
        return self.ENV_SAMPLING[mode.value], bool(active.value)

    # ---- Russian roulette (include/dcrt.h) -------------------------------------------
    def set_russian_roulette(self, enable: bool = True, start_bounce: int | None = None, min_survival: float | None = None,
                             max_survival: float | None = None) -> None:
        """Russian roulette path termination (off by default); a value left None is dcrt_roulette_default_params'.
        Lives on the tracer (kept across uploads and edits), takes effect with the next image: the caller
        restarts the image. Refused unless 0 < min_survival <= max_survival <= 1 and start_bounce <= 20."""
        p = roulette_defaults()
        p.enable = 1 if enable else 0
        if start_bounce is not None:
            if not 0 <= int(start_bounce) <= 0xFFFFFFFF:
                raise ValueError(f"Russian roulette start bounce {start_bounce!r}")
            p.start_bounce = int(start_bounce)
        if min_survival is not None:
            p.min_survival = float(min_survival)
        if max_survival is not None:
            p.max_survival = float(max_survival)
        check(self._lib.dcrt_tracer_set_roulette(self._h, C.byref(p)), "SetRoulette")

    def russian_roulette(self) -> dict:
        """The setting: {"enable", "start_bounce", "min_survival", "max_survival"}."""
        p = _abi.RouletteParams()
        check(self._lib.dcrt_tracer_get_roulette(self._h, C.byref(p)), "GetRoulette")
        return {"enable": bool(p.enable), "start_bounce": int(p.start_bounce), "min_survival": float(p.min_survival),
                "max_survival": float(p.max_survival)}

    def device_roulette(self, throughputs, u, min_survival: float, max_survival: float):
        """dcrt_device_roulette: (q [n], survive [n] bool, scaled [n, 3]) of the kernels' roulette on throughputs [n, 3]
        with u [n] in place of the paths' draws."""
        T = np.ascontiguousarray(throughputs, np.float32).reshape(-1, 3)
        uu = np.ascontiguousarray(u, np.float32).reshape(-1)
        if len(uu) != len(T):
            raise ValueError("device_roulette: one u per throughput")
        n = len(T)
        q, alive, scaled = np.empty(n, np.float32), np.empty(n, np.uint32), np.empty((n, 3), np.float32)
        p = _abi.RouletteParams(1, 0, float(min_survival), float(max_survival))
        fp = _abi._FP
        check(self._lib.dcrt_device_roulette(self._h, C.byref(p), T.ctypes.data_as(fp), uu.ctypes.data_as(fp), n, q.ctypes.data_as(fp),
                                             alive.ctypes.data_as(C.POINTER(C.c_uint32)), scaled.ctypes.data_as(fp)), "DeviceRoulette")
        return q, alive != 0, scaled

    def environment_distribution(self):
        """The stored table of the uploaded cube (size n): P [6n, n], the per-row CDF [6n, n], the marginal CDF [6n].
        Raises (no scene) while inactive."""
        n = max(1, self.env_cube_size)
        prob, cdf, marginal = np.empty((6 * n, n), np.float32), np.empty((6 * n, n), np.float32), np.empty(6 * n, np.float32)
        fp = _abi._FP
        check(self._lib.dcrt_tracer_read_environment_distribution(self._h, prob.ctypes.data_as(fp), cdf.ctypes.data_as(fp),
                                                                  marginal.ctypes.data_as(fp)), "ReadEnvironmentDistribution")
        return prob, cdf, marginal

    def environment_build_ms(self) -> float:
        ms = C.c_float()
        check(self._lib.dcrt_tracer_environment_build_timing(self._h, C.byref(ms)), "EnvironmentBuildTiming")
        return float(ms.value)

    # ---- light selection (include/dcrt.h) ---------------------------------------------
    LIGHT_SAMPLING = ("uniform", "power")

    def set_light_sampling(self, mode: str) -> None:
        """"uniform" (the default, the reference's selection) or "power": lights are picked in proportion to their power
        and a lamp's triangles in proportion to their area. Needs an uploaded scene; kept across later uploads; the caller
        restarts the image."""
        if mode not in self.LIGHT_SAMPLING:
            raise ValueError(f"light sampling {mode!r}: one of {self.LIGHT_SAMPLING}")
        check(self._lib.dcrt_tracer_set_light_sampling(self._h, self.LIGHT_SAMPLING.index(mode)), "SetLightSampling")

    def light_sampling(self) -> tuple[str, bool]:
        """(mode, active): active while the mode is on and a table stands for the lights as they are."""
        mode, active = C.c_int(), C.c_int()
        check(self._lib.dcrt_tracer_get_light_sampling(self._h, C.byref(mode), C.byref(active)), "GetLightSampling")
        return self.LIGHT_SAMPLING[mode.value], bool(active.value)

    def light_distribution(self) -> dict:
        """The stored light table: light_prob, light_cdf [n], tri_base [n] (uint32), tri_prob, tri_cdf [E], and n, E, the
        scene radius R and the total weight. Raises (no scene) while inactive."""
        info = _abi.LightTableInfo()
        check(self._lib.dcrt_tracer_read_light_distribution(self._h, C.byref(info), None, None, None, None, None), "ReadLightDistribution")
        n, e = int(info.light_count), int(info.triangle_entries)
        out = {"light_prob": np.empty(n, np.float32), "light_cdf": np.empty(n, np.float32), "tri_base": np.empty(n, np.uint32),
               "tri_prob": np.empty(e, np.float32), "tri_cdf": np.empty(e, np.float32)}
        fp = _abi._FP
        check(self._lib.dcrt_tracer_read_light_distribution(self._h, C.byref(info), out["light_prob"].ctypes.data_as(fp),
                                                            out["light_cdf"].ctypes.data_as(fp),
                                                            out["tri_base"].ctypes.data_as(C.POINTER(C.c_uint32)),
                                                            out["tri_prob"].ctypes.data_as(fp), out["tri_cdf"].ctypes.data_as(fp)),
              "ReadLightDistribution")
        out.update(n=n, entries=e, radius=float(info.scene_radius), total_weight=float(info.total_weight))
        return out

    def light_table_build_ms(self) -> float:
        ms = C.c_float()
        check(self._lib.dcrt_tracer_light_table_build_timing(self._h, C.byref(ms)), "LightTableBuildTiming")
        return float(ms.value)

    # ---- statistics ----------------------------------------------------------
    def counters(self) -> dict:
        s = _abi.RayStats()
        check(self._lib.dcrt_tracer_counters(self._h, C.byref(s)), "Counters")
        return {k: getattr(s, k) for k, _ in _abi.RayStats._fields_}

    def set_instrumentation(self, counters: bool, ext_timing: bool) -> None:
        check(self._lib.dcrt_tracer_set_instrumentation(self._h, int(counters), int(ext_timing)), "SetInstrumentation")

    def traversal_stats(self) -> dict:
        s = _abi.TraversalStats()
        check(self._lib.dcrt_tracer_traversal_stats(self._h, C.byref(s)), "TraversalStats")
        return {k: getattr(s, k) for k, _ in _abi.TraversalStats._fields_}

    def info(self) -> dict:
        """What the tracer chose for the uploaded scene (pool, LDS scene cache, variants)."""
        s = _abi.TracerInfo()
        check(self._lib.dcrt_tracer_get_info(self._h, C.byref(s)), "GetInfo")
        return {k: getattr(s, k) for k, _ in _abi.TracerInfo._fields_}

    def ring_spills(self) -> int:
        """Stack entries the spilling-stack cast kernel moved to its global columns (test hook)."""
        n = C.c_uint64(0)
        check(self._lib.dcrt_tracer_debug_ring_spills(self._h, C.byref(n)), "DebugRingSpills")
        return int(n.value)

    def reset_stats(self) -> None:
        check(self._lib.dcrt_tracer_reset_stats(self._h), "ResetStats")

    def synchronize(self) -> None:
        check(self._lib.dcrt_tracer_synchronize(self._h), "Synchronize")

    def luts(self) -> _abi.BxDFLuts:
        l = _abi.BxDFLuts()
        check(self._lib.dcrt_tracer_get_luts(self._h, C.byref(l)), "GetLuts")
        return l

    def set_luts(self, luts: _abi.BxDFLuts) -> None:
        check(self._lib.dcrt_tracer_set_luts(self._h, C.byref(luts)), "SetLuts")

    # ---- kernel-level entry points -------------------------------------------
    def trace_rays(self, rays: np.ndarray, features: int = _abi.FEATURE_DEFAULT) -> np.ndarray:
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        check(self._lib.dcrt_tracer_trace_rays(self._h, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays),
                                               hits.ctypes.data_as(C.POINTER(_abi.RayHit)), int(features)), "TraceRays")
        return hits

    def occluded(self, rays: np.ndarray, features: int = _abi.FEATURE_DEFAULT) -> np.ndarray:
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros(len(rays), np.uint32)
        check(self._lib.dcrt_tracer_occluded(self._h, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays),
                                             out.ctypes.data_as(C.POINTER(C.c_uint32)), int(features)), "Occluded")
        return out

    def cast_rays(self, rays: np.ndarray, kinds, opacity_samples=None, features: int = _abi.FEATURE_DEFAULT):
        """A ray batch through the cast a render of the uploaded scene with `features` launches
        (dcrt_tracer_cast_rays): kinds[i] == 0 a closest-hit ray, else an any-hit ray below its t_max, each
        with opacity_samples[i] under FEATURE_ALLOW_ANYHIT. Returns (hits, occluded, variant): `variant`
        names the flags of the kernel that ran ({"opacity", "all_cached", "pair", "ident", "ring", "flat"})."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        kinds = np.ascontiguousarray(kinds, np.uint32)
        if len(kinds) != len(rays):
            raise ValueError("one kind per ray")
        samples = None
        if opacity_samples is not None:
            samples = np.ascontiguousarray(opacity_samples, np.float32)
            if len(samples) != len(rays):
                raise ValueError("one opacity sample per ray")
        hits, occ, variant = np.zeros(len(rays), HIT_DTYPE), np.zeros(len(rays), np.uint32), C.c_uint32(0)
        check(self._lib.dcrt_tracer_cast_rays(self._h, rays.ctypes.data_as(C.POINTER(_abi.Ray)), kinds.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              None if samples is None else samples.ctypes.data_as(_abi._FP), len(rays), int(features),
                                              hits.ctypes.data_as(C.POINTER(_abi.RayHit)), occ.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              C.byref(variant)), "CastRays")
        return hits, occ, {k for k, bit in _abi.CAST_VARIANT.items() if variant.value & bit}

    def occluded_cells(self, rays: np.ndarray, features: int = _abi.FEATURE_DEFAULT) -> np.ndarray:
        """Occlusion bits of shadow rays towards the scene's point light through the merged cast's
        direction-cell section (dcrt_tracer_trace_occlusion_cells); `occluded` is its comparison
        partner. Raises when the scene has no table (info()["shadow_cells"] == 0)."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros(len(rays), np.uint32)
        check(self._lib.dcrt_tracer_trace_occlusion_cells(self._h, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays),
                                                          out.ctypes.data_as(C.POINTER(C.c_uint32)), int(features)),
              "TraceOcclusionCells")
        return out

    def trace_rays_device(self, d_rays: int, count: int, d_hits: int, features: int = _abi.FEATURE_DEFAULT) -> None:
        check(self._lib.dcrt_tracer_trace_rays_device(self._h, C.c_void_p(d_rays), int(count), C.c_void_p(d_hits),
                                                      int(features)), "TraceRaysDevice")

    def math_eval(self, function: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        check(self._lib.dcrt_device_math_eval(self._h, int(function), x.ctypes.data_as(_abi._FP), x.size,
                                              y.ctypes.data_as(_abi._FP)), "MathEval")
        return y

    def bsdf_eval(self, material: _abi.BsdfProbeMaterial, wi: np.ndarray, wo: np.ndarray,
                  features: int = _abi.FEATURE_DEFAULT):
        """MATERIAL's evaluate_bsdf / evaluate_bsdf_pdf of one material in the frame n = (0,0,1),
        t = (1,0,0) with the current LUTs: (N, 3) f and (N,) pdf for (N, 3) direction pairs."""
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        if len(wi) != len(wo):
            raise ValueError("bsdf_eval: wi and wo differ in length")
        f = np.zeros_like(wi)
        pdf = np.zeros(len(wi), np.float32)
        fp = _abi._FP
        check(self._lib.dcrt_device_bsdf_eval(self._h, C.byref(material), int(features), wi.ctypes.data_as(fp),
                                              wo.ctypes.data_as(fp), len(wi), f.ctypes.data_as(fp), pdf.ctypes.data_as(fp)),
              "BsdfEval")
        return f, pdf

    def frame_probe(self, u, v, triangles, instances, use_table: bool) -> np.ndarray:
        """The world-space normal, tangent and geometry normal (N, 3, 3) of hit records (u, v, triangle,
        instance) of the uploaded scene, as MATERIAL reconstructs them with the per-triangle frame table
        (use_table) or without it (dcrt_device_frame_probe)."""
        rec = np.empty((len(u), 4), np.uint32)
        rec[:, 0] = np.asarray(u, np.float32).view(np.uint32)
        rec[:, 1] = np.asarray(v, np.float32).view(np.uint32)
        rec[:, 2] = np.asarray(triangles, np.uint32)
        rec[:, 3] = np.asarray(instances, np.uint32)
        out = np.zeros((len(rec), 3, 3), np.float32)
        check(self._lib.dcrt_device_frame_probe(self._h, rec.ctypes.data_as(C.POINTER(C.c_uint32)), len(rec), int(bool(use_table)),
                                                out.ctypes.data_as(_abi._FP)), "FrameProbe")
        return out

    # -- the shading probes (tests): the path kernels' own stages on the uploaded scene and the current frame
    # parameters; layouts in dcrt.h --
    def camera_ray_at(self, film, aperture):
        """generate_ray at (N, 2) film samples and (N, 3) aperture numbers: origins, directions (N, 3)."""
        film = np.ascontiguousarray(film, np.float32).reshape(-1, 2)
        aperture = np.ascontiguousarray(aperture, np.float32).reshape(-1, 3)
        if len(film) != len(aperture):
            raise ValueError("camera_ray_at: film and aperture samples differ in length")
        o, d = np.zeros((len(film), 3), np.float32), np.zeros((len(film), 3), np.float32)
        fp = _abi._FP
        check(self._lib.dcrt_device_camera_ray(self._h, film.ctypes.data_as(fp), aperture.ctypes.data_as(fp), len(film),
                                               o.ctypes.data_as(fp), d.ctypes.data_as(fp)), "CameraRay")
        return o, d

    def intersection_probe(self, records, use_table: bool = False):
        """hit_to_intersection of (N, 4) uint32 hit records (u, v bits, triangle | backface bit 31, instance):
        (N, 16) floats -- position, normal, tangent, geometry normal, albedo, alpha -- and (N, 3) words --
        material type, flags, light index."""
        records = np.ascontiguousarray(records, np.uint32).reshape(-1, 4)
        f, w = np.zeros((len(records), 16), np.float32), np.zeros((len(records), 3), np.uint32)
        up = C.POINTER(C.c_uint32)
        check(self._lib.dcrt_device_intersection_probe(self._h, records.ctypes.data_as(up), len(records), int(bool(use_table)),
                                                       f.ctypes.data_as(_abi._FP), w.ctypes.data_as(up)), "IntersectionProbe")
        return f, w

    def light_sample(self, points, states):
        """sample_light from (N, 3) points and (N, 4) xoshiro states: (N, 8) floats -- radiance, wi, pdf,
        distance -- and (N, 5) words -- delta flag, advanced state."""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        states = np.ascontiguousarray(states, np.uint32).reshape(-1, 4)
        if len(points) != len(states):
            raise ValueError("light_sample: points and states differ in length")
        f, w = np.zeros((len(points), 8), np.float32), np.zeros((len(points), 5), np.uint32)
        up = C.POINTER(C.c_uint32)
        check(self._lib.dcrt_device_light_sample(self._h, points.ctypes.data_as(_abi._FP), states.ctypes.data_as(up), len(points),
                                                 f.ctypes.data_as(_abi._FP), w.ctypes.data_as(up)), "LightSample")
        return f, w

    def light_eval(self, light_triangle, normal_wi_distance):
        """evaluate_light of (N, 2) (light, triangle) and (N, 7) (normal, wi, distance): (N, 4) radiance, pdf."""
        lt = np.ascontiguousarray(light_triangle, np.uint32).reshape(-1, 2)
        a = np.ascontiguousarray(normal_wi_distance, np.float32).reshape(-1, 7)
        if len(lt) != len(a):
            raise ValueError("light_eval: index pairs and vectors differ in length")
        out = np.zeros((len(lt), 4), np.float32)
        check(self._lib.dcrt_device_light_eval(self._h, lt.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(_abi._FP), len(lt),
                                               out.ctypes.data_as(_abi._FP)), "LightEval")
        return out

    def env_lookup(self, directions):
        """sample_env at (N, 3) directions: rgb (N, 3)."""
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        out = np.zeros_like(d)
        check(self._lib.dcrt_device_env_lookup(self._h, d.ctypes.data_as(_abi._FP), len(d), out.ctypes.data_as(_abi._FP)), "EnvLookup")
        return out

    def bsdf_sample(self, material: _abi.BsdfProbeMaterial, wo: np.ndarray, u: np.ndarray,
                    features: int = _abi.FEATURE_DEFAULT):
        """MATERIAL's sample_bsdf likewise: for (N, 3) wo and (N, 3) numbers (sx, sy, sel), the
        sampled wi (N, 3), f (N, 3), pdf (N,) and delta flags (N,)."""
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 3)
        if len(wo) != len(u):
            raise ValueError("bsdf_sample: wo and u differ in length")
        wi = np.zeros_like(wo)
        f = np.zeros_like(wo)
        pdf = np.zeros(len(wo), np.float32)
        delta = np.zeros(len(wo), np.uint32)
        fp = _abi._FP
        check(self._lib.dcrt_device_bsdf_sample(self._h, C.byref(material), int(features), wo.ctypes.data_as(fp),
                                                u.ctypes.data_as(fp), len(wo), wi.ctypes.data_as(fp), f.ctypes.data_as(fp),
                                                pdf.ctypes.data_as(fp), delta.ctypes.data_as(C.POINTER(C.c_uint32))),
              "BsdfSample")
        return wi, f, pdf, delta.astype(bool)


def bsdf_probe_material(type, albedo=(1.0, 1.0, 1.0), alpha=0.5, ior=1.5, two_sided=False, multiscattering=False,
                        internal_scattering=0) -> _abi.BsdfProbeMaterial:
    """A probe material for bsdf_eval / bsdf_sample; a scalar ior fills all three channels."""
    ior3 = (float(ior),) * 3 if np.isscalar(ior) else tuple(float(x) for x in ior)
    return _abi.BsdfProbeMaterial(int(type), (C.c_float * 3)(*albedo), (C.c_float * 3)(*ior3), float(alpha), int(two_sided),
                                  int(multiscattering), int(internal_scattering))


def denoise_default_params() -> _abi.DenoiseParams:
    """dcrt_denoise_default_params: 5 iterations, sigmas 4 / 0.2 / 0.1, demodulation on (no device needed)."""
    p = _abi.DenoiseParams()
    check(_abi.load_library().dcrt_denoise_default_params(C.byref(p)), "DenoiseDefaultParams")
    return p


def firefly_default_params() -> _abi.FireflyParams:
    """dcrt_firefly_default_params: 6 cascades from luminance 1 in steps of 8, support 3 (no device needed). The
    defaults come from a prototype on a synthetic run, not from a render."""
    p = _abi.FireflyParams()
    check(_abi.load_library().dcrt_firefly_default_params(C.byref(p)), "FireflyDefaultParams")
    return p


def roulette_defaults() -> _abi.RouletteParams:
    """dcrt_roulette_default_params: off, start bounce 2, survival within [0.05, 1] (no device needed)."""
    p = _abi.RouletteParams()
    check(_abi.load_library().dcrt_roulette_default_params(C.byref(p)), "RouletteDefaultParams")
    return p


def noise_stats_dict(s: _abi.NoiseStats) -> dict:
    return {k: getattr(s, k) for k, _ in _abi.NoiseStats._fields_}


def srgb_thresholds() -> np.ndarray:
    out = np.empty(255, np.float32)
    check(_abi.load_library().dcrt_srgb_encode_thresholds(out.ctypes.data_as(_abi._FP)), "SrgbThresholds")
    return out


def save_bmp(path, rgba8: np.ndarray) -> None:
    """24-bit BMP (SaveImageToFile.cpp:92-182)."""
    a = np.ascontiguousarray(rgba8, np.uint8)
    h, w = a.shape[:2]
    check(_abi.load_library().dcrt_write_bmp(str(path).encode(), w, h, a.ctypes.data_as(C.POINTER(C.c_uint8))), "WriteBmp")


def device_count() -> int:
    lib = _abi.load_library()
    n = C.c_int()
    check(lib.dcrt_device_count(C.byref(n)))
    return n.value


def make_pipelines(scene, pool: int, streams: int = 2, images: int = 1, iterations: int = 16, world: int = 1,
                   rank: int = 0, stripe: int = 64, mode: str = "wavefront", image_batch: int = 0, device: int = 0,
                   debug_rng: bool = False, row_cost=None, fixed_pool: bool = False, interleave: bool = False,
                   bands_per_rank: int = 0, env_sampling: str = "uniform", roulette: dict | None = None,
                   light_sampling: str = "uniform") -> list:
    """The concurrent wavefront pipelines bench.py renders with, each a tracer with its share of
    `pool` slots (grown to whole batches of `images` images, partition.pipeline_pool), the
    filter's halo rows, its own stream. With `row_cost` (rays per film row, probe_row_cost) the
    film is cut into world x streams contiguous equal-cost bands (partition.balanced_bands) and
    pipeline s of rank r takes band s * world + r -- dealt round-robin, so every rank holds one
    band of each 1/streams of the film and a cost trend down the image evens out; without it, one GPU splits the film into
    `streams` equal horizontal bands and N GPUs deal this rank's round-robin stripes to its
    pipelines (partition.stream_partition). Their films have disjoint supports: add_film_device
    sums them into the rank's film bit for bit. `roulette`: set_russian_roulette's arguments, given to every pipeline;
    `light_sampling`: set_light_sampling's mode, likewise."""
    from .partition import balanced_bands, band_render_rows, halo_for_radius, pipeline_pool, render_rows, stream_partition
    W, H = scene.resolution
    halo = max(1, halo_for_radius(scene.filter_params().radius, H))
    K = max(1, streams)
    if interleave:
        return _make_interleaved(scene, pool, K, images, iterations, world, rank, stripe, mode, image_batch, device, debug_rng,
                                 row_cost, fixed_pool, bands_per_rank or K, halo, env_sampling, roulette, light_sampling)
    bands = balanced_bands(row_cost, world * K, halo) if row_cost is not None and world * K > 1 else None
    tracers = []
    try:
        for s_ in range(K):
            part = stream_partition(H, world, rank, K, s_, stripe) if (K > 1 or world > 1) and bands is None else None
            band = [bands[s_ * world + rank]] if bands is not None else None
            rows = (len(band_render_rows(H, band, halo)) if band is not None
                    else len(render_rows(H, *part, halo)) if part is not None else H)
            p = pipeline_pool(pool // K, rows, W, images) if not (image_batch or fixed_pool) else pool // K
            t = WavefrontPathTracer(path_pool_size=p, iterations_per_render=iterations, device=device, debug_rng=debug_rng)
            tracers.append(t)
            t.on_scene_loaded(scene)
            t.set_environment_sampling(env_sampling)
            t.set_light_sampling(light_sampling)
            if roulette is not None:
                t.set_russian_roulette(**roulette)
            t.set_mode(mode)
            t.set_image_batch(image_batch)
            if band is not None:
                t.set_film_bands(band, halo)
            elif part is not None:
                t.set_film_partition(*part, halo)
    except BaseException:
        for t in tracers:
            t.destroy()
        raise
    return tracers


def _make_interleaved(scene, pool, K, images, iterations, world, rank, stripe, mode, image_batch, device, debug_rng, row_cost,
                      fixed_pool, bands_per_rank, halo, env_sampling="uniform", roulette=None,
                      light_sampling="uniform") -> list:
    """make_pipelines(interleave=True): K tracers over the SAME rows -- the whole film on one GPU,
    the rank's share of it on N (`bands_per_rank` cost-balanced bands dealt round-robin, or the
    round-robin stripes without a row cost) -- that split the images instead of the rows
    (render_images_concurrently deals image j to pipeline j mod K). No halo rows between the
    pipelines of one GPU, and the pipelines carry statistically equal work."""
    from .partition import balanced_bands, band_render_rows, pipeline_pool, render_rows
    W, H = scene.resolution
    bands = part = None
    if world > 1:
        if row_cost is not None:
            B = max(1, bands_per_rank)
            bands = balanced_bands(row_cost, world * B, halo)[rank::world]
        else:
            part = (world, rank, stripe)
    rows = (len(band_render_rows(H, bands, halo)) if bands is not None
            else len(render_rows(H, *part, halo)) if part is not None else H)
    per = -(-images // K)
    px = max(1, -(-rows // 8) * 8 * -(-W // 8) * 8)
    p = pipeline_pool(pool // K, rows, W, per) if not (image_batch or fixed_pool) else pool // K
    tracers = []
    try:
        for _ in range(K):
            t = WavefrontPathTracer(path_pool_size=p, iterations_per_render=iterations, device=device, debug_rng=debug_rng)
            tracers.append(t)
            t.on_scene_loaded(scene)
            t.set_environment_sampling(env_sampling)
            t.set_light_sampling(light_sampling)
            if roulette is not None:
                t.set_russian_roulette(**roulette)
            t.set_mode(mode)
            t.set_image_batch(image_batch)
            if bands is not None:
                t.set_film_bands(bands, halo)
            elif part is not None:
                t.set_film_partition(*part, halo)
            t.interleaved = True
            t.pool_images = max(1, p // px)
            t.rank_bands = bands
    except BaseException:
        for t in tracers:
            t.destroy()
        raise
    return tracers


def _run_threads(tracers, fn) -> None:
    """fn(index, tracer) on every tracer at once (one host thread each; the C ABI runs with the
    GIL released and every tracer owns its stream). An error in any tracer is raised here,
    after every thread has finished."""
    import threading
    errors = []

    def run(i, t):
        try:
            fn(i, t)
        except BaseException as e:   # re-raised in the caller's thread
            errors.append(e)

    if len(tracers) == 1:
        run(0, tracers[0])
    else:
        th = [threading.Thread(target=run, args=(i, t)) for i, t in enumerate(tracers)]
        for x in th:
            x.start()
        for x in th:
            x.join()
    if errors:
        raise errors[0]


def render_images_concurrently(tracers, first_seed: int, count: int, filter_params=None) -> None:
    """render_images on several tracers at once, then synchronize them all. Pipelines built
    with interleaved images (make_pipelines(interleave=True)) share their rows: tracer s renders
    images s, s + K, ... of each chunk without the film pass, and tracer 0 then convolves the
    chunk's images in image order from all K pipelines' sample textures (accumulate_images), so
    its film is the one-pipeline film bit for bit and the others' stay empty."""
    K = len(tracers)
    if K > 1 and getattr(tracers[0], "interleaved", False):
        # chunks the pipelines' pools hold whole (one batch each, with its virtual start)
        chunk = K * max(1, min(getattr(t, "pool_images", 1) for t in tracers))
        for c0 in range(0, count, chunk):
            n = min(chunk, count - c0)
            _run_threads(tracers, lambda s, t: t.render_images(first_seed + c0 + s, len(range(s, n, K)), filter_params,
                                                               seed_stride=K, convolve=False) if s < n else None)
            for t in tracers:
                t.synchronize()
            # image k of a pipeline's call sits in its sample slot k: slot 0's pointers plus k
            # whole-film strides (one ABI call per pipeline, not one per image)
            W, H = tracers[0].width, tracers[0].height
            base = [t.image_sample_ptrs(0) for t in tracers[:min(K, n)]]
            pos = [base[j % K][0] + (j // K) * W * H * 8 for j in range(n)]
            val = [base[j % K][1] + (j // K) * W * H * 16 for j in range(n)]
            tracers[0].accumulate_images(pos, val, filter_params)
        return
    _run_threads(tracers, lambda i, t: t.render_images(first_seed, count, filter_params))
    for t in tracers:
        t.synchronize()


def prepare_pipelines(tracers, count: int) -> None:
    """prepare_images on every pipeline for a render_images_concurrently of `count` images: the
    whole count on banded pipelines, the largest per-pipeline share of a chunk on interleaved
    ones (each keeps only the images it renders)."""
    K = len(tracers)
    if K > 1 and getattr(tracers[0], "interleaved", False):
        chunk = min(count, K * max(1, min(getattr(t, "pool_images", 1) for t in tracers)))
        count = -(-chunk // K)
    for t in tracers:
        t.prepare_images(count)


def probe_row_cost(scene, first_seed: int = 1 << 20, images: int = 1, pool: int = 1 << 22, device: int = 0) -> np.ndarray:
    """Rays cast per film row over `images` images (seeds first_seed ..) of the whole film, from
    the tracer's row-cost probe: exact and schedule-independent, so every rank that probes the
    same scene gets the same vector and cuts the same balanced bands without communicating.
    (The default seeds lie outside any render's: the probe's image is not one of the film's.)"""
    t = WavefrontPathTracer(path_pool_size=pool, iterations_per_render=16, device=device)
    try:
        t.on_scene_loaded(scene)
        t.set_row_cost_probe(True)
        t.clear_film()
        t.render_images(first_seed, images)
        return t.read_row_cost().astype(np.int64)
    finally:
        t.destroy()
