#!/usr/bin/env python3
"""What Russian roulette costs and buys on one GPU (dcrt.h "Russian roulette").

For each config (BASELINE.json's Cornell at 1080p and 8 bounces, and coffee) and each setting -- off, then on from
bounce `start` in {1, 2, 3} with dcrt_roulette_default_params' min_survival and max_survival:

* milliseconds per image on bench.py's pipelines (make_pipelines: 3 for Cornell, 2 otherwise; render_images over
  `--images` images, the median of `--repeat` runs after one warm-up run);
* extension and shadow rays per image (the counters of the last run);
* the per-sample luminance variance: per pixel, the variance of the sample's luminance over `--variance-images`
  single-image renders (seeds 0, 1, ...), averaged over the film;
* time x variance relative to off: the cost of a given noise level, below 1 where the roulette pays.

    python tools/bench_roulette.py [--configs cornell,coffee] [--images 16] [--repeat 5] [--variance-images 16] [--out FILE]

The text goes to stdout and to `--out` (default profiles/roulette_costs.txt); the last stdout line is JSON.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LUM = np.array([0.299, 0.587, 0.114])


def settings():
    from directcomputeraytracing_amd.tracer import roulette_defaults
    d = roulette_defaults()
    out = [("off", None)]
    for start in (1, 2, 3):
        out.append((f"start {start}", dict(enable=True, start_bounce=start, min_survival=float(d.min_survival), max_survival=float(d.max_survival))))
    return out


def timed(scene, config, roulette, images, repeat):
    from directcomputeraytracing_amd import make_pipelines, prepare_pipelines, render_images_concurrently, scenes
    W, H = scene.resolution
    K = 3 if config == "cornell" else 2
    filt = scene.filter_params()
    tracers = make_pipelines(scene, scenes.default_pool(W, H, K), streams=K, images=images, iterations=16, roulette=roulette)
    try:
        for t in tracers:
            t.clear_film()
        prepare_pipelines(tracers, images)
        ms = []
        for _ in range(repeat + 1):                    # (the first run warms up: graphs, caches)
            for t in tracers:
                t.clear_film()
                t.reset_stats()
                t.synchronize()
            t0 = time.perf_counter()
            render_images_concurrently(tracers, 0, images, filt)
            for t in tracers:
                t.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / images)
        c = [t.counters() for t in tracers]
        return {"ms_per_image": statistics.median(ms[1:]), "ms_runs": [round(x, 4) for x in ms[1:]],
                "extension_rays_per_image": sum(x["extension_rays"] for x in c) / images,
                "shadow_rays_per_image": sum(x["shadow_rays"] for x in c) / images}
    finally:
        for t in tracers:
            t.destroy()


def variance(scene, roulette, images):
    from directcomputeraytracing_amd import WavefrontPathTracer
    W, H = scene.resolution
    t = WavefrontPathTracer(path_pool_size=1 << 22)
    try:
        t.on_scene_loaded(scene)
        if roulette is not None:
            t.set_russian_roulette(**roulette)
        s1, s2 = np.zeros((H, W)), np.zeros((H, W))
        for seed in range(images):
            t.clear_film()
            t.render_images(seed, 1)
            y = np.nan_to_num(t.read_samples()[1][..., :3].astype(np.float64) @ LUM, nan=0.0, posinf=0.0, neginf=0.0)
            s1 += y
            s2 += y * y
        mean = s1 / images
        var = (s2 / images - mean * mean) * images / max(1, images - 1)
        return {"mean_luminance": float(mean.mean()), "variance": float(var.mean())}
    finally:
        t.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cornell,coffee")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--variance-images", type=int, default=16)
    ap.add_argument("--scene-dir", default="/tmp/dcrt_scenes")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "roulette_costs.txt"))
    a = ap.parse_args()
    from directcomputeraytracing_amd import Scene, scenes
    lines, result = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# Russian roulette: costs and effect (tools/bench_roulette.py)")
    say(f"# {a.images} images per run, median of {a.repeat} runs; variance: per-pixel sample luminance over {a.variance_images} seeds, film mean")
    for config in a.configs.split(","):
        scene = Scene((1920, 1080))
        say(f"## {config}: {scenes.setup_config(scene, config, Path(a.scene_dir))}")
        rows = {}
        for label, roulette in settings():
            row = timed(scene, config, roulette, a.images, a.repeat)
            row.update(variance(scene, roulette, a.variance_images))
            rows[label] = row
            off = rows["off"]
            row["time_x_variance"] = (row["ms_per_image"] / off["ms_per_image"]) * (row["variance"] / off["variance"]) if off["variance"] > 0 else float("nan")
            say(f"{label:8s}  {row['ms_per_image']:.4f} ms/image (runs {min(row['ms_runs']):.4f} .. {max(row['ms_runs']):.4f})   "
                f"extension rays {row['extension_rays_per_image'] / 1e6:.3f} M   shadow rays {row['shadow_rays_per_image'] / 1e6:.3f} M   "
                f"mean luminance {row['mean_luminance']:.5f}   variance {row['variance']:.5f}   "
                f"time {row['ms_per_image'] / off['ms_per_image']:.3f} x variance {row['variance'] / off['variance'] if off['variance'] > 0 else float('nan'):.3f} "
                f"= {row['time_x_variance']:.3f} of off")
        result[config] = rows
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
