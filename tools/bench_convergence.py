#!/usr/bin/env python3
"""What the film noise estimate costs on one GPU, and what render_converged does with it.

* The film pass's HIP-event time per image with convergence off and on (the half film's second
  accumulator), Cornell at 1080p and 4K with the scene's filter: ext_timing launches,
  dcrt_tracer_film_pass_timing.
* The noise kernels (tile pass, reduction passes, totals) at both sizes: the median wall time of
  noise(), which includes the copy of the statistics.
* Cornell 1080p, 8 bounces: the images render_converged takes at thresholds 0.05 and 0.02 with a
  target fraction of 0.95, and its wall time against render_images of the same count.

    python tools/bench_convergence.py [--images 8] [--repeat 9] [--max-images 4096]

The last line is JSON.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def film_pass_ms(t, images, convergence):
    """HIP-event ms per image of the film pass over `images` images."""
    t.set_instrumentation(False, False)
    t.set_convergence(convergence)
    t.render_images(0, images)            # warm-up: sample textures, code objects
    t.set_instrumentation(False, True)
    t.clear_film()
    t.reset_stats()
    t.render_images(0, images)
    _, ms = t.film_pass_timing()
    t.set_instrumentation(False, False)
    return ms / images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8, help="images per film-pass measurement")
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--max-images", type=int, default=4096)
    a = ap.parse_args()
    from directcomputeraytracing_amd import ConvergeParams, Scene, WavefrontPathTracer, scenes
    result = {"film_pass_ms_per_image": {}, "noise_ms": {}, "render_converged": {}}
    for name, (W, H) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        s = Scene((W, H))
        scenes.setup_cornell(s, W, H, 8)
        t = WavefrontPathTracer(path_pool_size=1 << 22)
        try:
            t.on_scene_loaded(s)
            off = statistics.median(film_pass_ms(t, a.images, False) for _ in range(3))
            on = statistics.median(film_pass_ms(t, a.images, True) for _ in range(3))
            result["film_pass_ms_per_image"][name] = {"off": off, "on": on}
            print(f"{name}: film pass {off:.4f} ms per image with convergence off, {on:.4f} on ({(on / off - 1) * 100:+.1f} %)")
            t.noise(0.05)                 # (convergence is on, the film holds a.images images)
            wall = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                t.noise(0.05)
                wall.append((time.perf_counter() - t0) * 1e3)
            result["noise_ms"][name] = statistics.median(wall)
            print(f"{name}: noise() {statistics.median(wall):.4f} ms wall (median of {a.repeat})")
            if name != "1080p":
                continue
            for threshold in (0.05, 0.02):
                p = ConvergeParams(threshold, 0.95, 16, a.max_images, 16)
                t.clear_film()
                t.prepare_images(16)      # (the batch's sample textures and graphs, outside the timed region)
                t.synchronize()
                t0 = time.perf_counter()
                stats, converged = t.render_converged(0, p)
                wall_converged = time.perf_counter() - t0
                n = stats["images"]
                t.set_convergence(False)
                t.prepare_images(n)
                t.synchronize()
                t0 = time.perf_counter()
                t.render_images(0, n)
                t.synchronize()
                wall_plain = time.perf_counter() - t0
                t.set_convergence(True)
                result["render_converged"][str(threshold)] = {
                    "images": n, "converged": converged, "converged_fraction": stats["converged_pixels"] / max(1, stats["valid_pixels"]),
                    "mean_error": stats["mean_error"], "seconds": wall_converged, "render_images_seconds": wall_plain}
                print(f"1080p threshold {threshold}: {n} images, converged {converged}, "
                      f"{stats['converged_pixels'] / max(1, stats['valid_pixels']):.4f} of the pixels, mean e {stats['mean_error']:.4f}; "
                      f"{wall_converged:.3f} s against render_images({n}) {wall_plain:.3f} s ({(wall_converged / wall_plain - 1) * 100:+.1f} %)")
        finally:
            t.destroy()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
