#!/usr/bin/env python3
"""Cost and effect of firefly re-weighting (dcrt.h "firefly re-weighting") on one GPU, into profiles/firefly_costs.txt:

  1. the cascade pass per image beside the film pass of the same launch pair (HIP events: dcrt_tracer_firefly_timings
     and dcrt_tracer_film_pass_timing around accumulate_film of a Cornell image), at 1080p and 4K, K = 6;
  2. the resolve (HIP events) and the memory the cascades hold, K * W * H * 16 B;
  3. Cornell 64 x 64 with Russian roulette on: the share of the film's summed luminance the resolve removes after 4,
     16, 64 and 256 images, and the denoiser's output with the film and with the re-weighted image as its colour
     input (mean luminance of each, and their RMS difference) -- evidence of how fast the bias vanishes, not a check.

    python tools/bench_firefly.py [--repeat 9] [--out profiles/firefly_costs.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LUM = np.array([0.299, 0.587, 0.114])


def cornell(width, height, bounces):
    from directcomputeraytracing_amd import Scene, scenes
    s = Scene((width, height))
    scenes.setup_cornell(s, width, height, bounces)
    return s


def pass_costs(width, height, repeat, lines):
    from directcomputeraytracing_amd import WavefrontPathTracer, firefly_default_params
    t = WavefrontPathTracer()
    try:
        t.on_scene_loaded(cornell(width, height, 2))
        params = firefly_default_params()
        t.set_instrumentation(False, True)
        t.set_mode("megakernel")          # (one image, its samples left in slot 0 for accumulate_film)

        def film_ms():
            t.reset_stats()
            t.accumulate_film()
            launches, ms = t.film_pass_timing()
            assert launches == 1
            return ms

        t.render_images(0, 1)
        off = [film_ms() for _ in range(repeat + 1)][1:]
        t.set_firefly_filter(params)
        t.render_images(0, 1)
        film, cascade, resolve = [], [], []
        for _ in range(repeat + 1):
            film.append(film_ms())
            cascade.append(t.firefly_timings()[0])
            t.firefly_filtered()
            resolve.append(t.firefly_timings()[1])
        med = lambda v: statistics.median(v[1:])
        mib = int(params.cascades) * width * height * 16 / 2 ** 20
        lines.append(f"{width}x{height}, K = {params.cascades}: film pass {statistics.median(off):.3f} ms with the feature off, "
                     f"{med(film):.3f} ms on; cascade pass {med(cascade):.3f} ms per image ({med(cascade) / med(film):.1f}x the film pass); "
                     f"resolve {med(resolve):.3f} ms; cascades hold {mib:.0f} MiB")
    finally:
        t.destroy()


def bias_run(lines):
    from directcomputeraytracing_amd import WavefrontPathTracer, firefly_default_params, denoise_default_params
    W = H = 64
    t = WavefrontPathTracer(path_pool_size=1 << 16)
    try:
        t.on_scene_loaded(cornell(W, H, 8))
        t.set_russian_roulette(True)
        t.set_firefly_filter(firefly_default_params())
        lum = lambda img: np.maximum(img[..., :3].astype(np.float64) @ LUM, 0.0)
        done = 0
        for count in (4, 16, 64, 256):
            t.render_images(done, count - done)
            done = count
            film = t.read_film()
            kept = t.firefly_filtered()
            plain = lum(film[..., :3] / film[..., 3:4])
            lines.append(f"Cornell {W}x{H}, 8 bounces, roulette on, defaults: after {count:3d} images the resolve removes "
                         f"{1.0 - lum(kept).sum() / plain.sum():.4%} of the film's summed luminance "
                         f"(largest pixel {plain.max():.3f} -> {lum(kept).max():.3f})")
        t.render_guides(0, done)
        a = t.denoise(denoise_default_params())
        b = t.denoise(denoise_default_params(), firefly=True)
        lines.append(f"denoiser at {done} images: mean luminance {lum(a).mean():.5f} with the film as colour input, {lum(b).mean():.5f} "
                     f"with the re-weighted image; RMS difference {np.sqrt(((lum(a) - lum(b)) ** 2).mean()):.2e}")
    finally:
        t.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "firefly_costs.txt"))
    args = ap.parse_args()
    from directcomputeraytracing_amd import version
    lines = [f"firefly re-weighting: costs and bias (tools/bench_firefly.py; {version()})",
             f"HIP events around the kernels (ext_timing), medians of {args.repeat} accumulate_film / resolve calls after a warm-up call; "
             "one Cornell image in the sample textures, the scene's reconstruction filter"]
    pass_costs(1920, 1080, args.repeat, lines)
    pass_costs(3840, 2160, args.repeat, lines)
    bias_run(lines)
    lines.append("not measured: other K and base values, megakernel timing, anything on more than one GPU")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
