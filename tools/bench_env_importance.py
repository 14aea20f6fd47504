#!/usr/bin/env python3
"""What environment importance sampling costs and buys on one GPU (dcrt.h "environment importance sampling").

The scene is the test suite's: a diffuse plane (rho 0.6, no bounce) under scenes.env_cube(8) with the texel
(face 2, y 2, x 7) set to 5000, at 1080p. For uniform and for importance sampling:

* milliseconds per image (render_images over `--images` images, the median of `--repeat` runs);
* the mean noise estimate (noise()["mean_error"]) after the same `--images` images;
* the images render_converged needs for `--threshold` at fraction 0.95, checked every 16 images, at most `--max-images`;
* the per-sample variance over the pixels that see the plane, from `--variance-images` single-image renders at 128 x 128
  (what tests/test_gpu_env_importance.py::test_variance_falls bounds), and the ratio of the two.

Then the table's build time (the HIP-event time of its three kernels, the median of `--repeat` uploads) for cubes of
n = 8, 256 and 1024.

    python tools/bench_env_importance.py [--images 32] [--repeat 5] [--threshold 0.05] [--max-images 512] [--out FILE]

The text goes to stdout and to `--out` (default profiles/env_importance_costs.txt); the last stdout line is JSON.
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COLOUR = (0.9, 1.1, 0.7)
MODES = ("uniform", "importance")


def sun_cube():
    from directcomputeraytracing_amd import scenes
    cube = scenes.env_cube(8)
    cube[2, 2, 7] = 5000.0
    return cube


def plane_scene(width, height, cube, directory):
    from directcomputeraytracing_amd import Scene, scenes
    s = Scene((width, height))
    s.load_from_file(scenes.write_lit_plane(directory, width, height, albedo=0.6))
    s.set_environment_light(COLOUR, cube)
    return s


def plane_pixels(t, size):
    """The pixels whose four corner rays hit the plane [-4, 4]^2 at y = 0."""
    g = np.arange(size + 1, dtype=np.float64) / size
    X, Y = np.meshgrid(g, g, indexing="xy")
    film = np.stack([X.ravel(), Y.ravel()], 1).astype(np.float32)
    o, d = t.camera_ray_at(film, np.zeros((len(film), 3), np.float32))
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        hit = o + (-o[:, 1] / d[:, 1])[:, None] * d
    ok = ((d[:, 1] < 0) & (np.abs(hit[:, 0]) < 3.99) & (np.abs(hit[:, 2]) < 3.99)).reshape(size + 1, size + 1)
    return ok[:-1, :-1] & ok[1:, :-1] & ok[:-1, 1:] & ok[1:, 1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--max-images", type=int, default=512)
    ap.add_argument("--variance-images", type=int, default=32)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "env_importance_costs.txt"))
    a = ap.parse_args()
    from directcomputeraytracing_amd import ConvergeParams, WavefrontPathTracer, scenes
    lines, result = [], {"render": {}, "variance": {}, "build_ms": {}}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# Environment importance sampling: costs and effect (tools/bench_env_importance.py)")
    say(f"# scene: the lit plane (rho 0.6, max_depth 0) under scenes.env_cube(8) with texel (2, 2, 7) = 5000, colour {COLOUR}")
    with tempfile.TemporaryDirectory() as tmp:
        W, H = 1920, 1080
        scene = plane_scene(W, H, sun_cube(), Path(tmp) / "hd")
        say(f"## {W} x {H}, {a.images} images per run, median of {a.repeat}")
        for mode in MODES:
            t = WavefrontPathTracer(path_pool_size=1 << 22)
            try:
                t.on_scene_loaded(scene)
                t.set_environment_sampling(mode)
                t.set_convergence(True)
                t.prepare_images(a.images)
                ms = []
                for _ in range(a.repeat + 1):          # (the first run warms up)
                    t.clear_film()
                    t.synchronize()
                    t0 = time.perf_counter()
                    t.render_images(0, a.images)
                    t.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3 / a.images)
                stats = t.noise(a.threshold)
                t.clear_film()
                conv, done = t.render_converged(0, ConvergeParams(a.threshold, 0.95, 16, a.max_images, 16))
                row = {"ms_per_image": statistics.median(ms[1:]), "mean_error": stats["mean_error"],
                       "converged_fraction": stats["converged_pixels"] / max(1, stats["valid_pixels"]),
                       "converge_images": conv["images"], "converged": bool(done)}
                result["render"][mode] = row
                say(f"{mode:10s}  {row['ms_per_image']:.4f} ms/image   mean noise estimate after {a.images} images {row['mean_error']:.5f} "
                    f"({row['converged_fraction']:.4f} of the pixels under {a.threshold})   render_converged: {row['converge_images']} images, "
                    f"converged {row['converged']} (cap {a.max_images})")
            finally:
                t.destroy()
        size = 128
        small = plane_scene(size, size, sun_cube(), Path(tmp) / "small")
        lum = np.array([0.299, 0.587, 0.114])
        for mode in MODES:
            t = WavefrontPathTracer(path_pool_size=1 << 16)
            try:
                t.on_scene_loaded(small)
                t.set_environment_sampling(mode)
                plane = plane_pixels(t, size)
                v = []
                for seed in range(a.variance_images):
                    t.clear_film()
                    t.render_images(seed, 1)
                    v.append(t.read_samples()[1][..., :3][plane].astype(np.float64) @ lum)
                v = np.concatenate(v)
                result["variance"][mode] = {"mean": float(v.mean()), "variance": float(v.var()), "samples": int(v.size)}
            finally:
                t.destroy()
        ratio = result["variance"]["importance"]["variance"] / result["variance"]["uniform"]["variance"]
        result["variance"]["ratio"] = ratio
        say(f"## per-sample variance over the plane's pixels, {size} x {size}, {a.variance_images} images (luminance)")
        for mode in MODES:
            r = result["variance"][mode]
            say(f"{mode:10s}  mean {r['mean']:.4f}   variance {r['variance']:.4f}   ({r['samples']} samples)")
        say(f"ratio importance / uniform: {ratio:.5f}")
        say(f"## table build: HIP-event ms of env_rows_kernel + env_marginal_kernel + env_finish_kernel, median of {a.repeat} uploads")
        for n in (8, 256, 1024):
            s = plane_scene(64, 64, scenes.env_cube(n), Path(tmp) / f"n{n}")
            t = WavefrontPathTracer(path_pool_size=1 << 14)
            try:
                t.on_scene_loaded(s)
                t.set_environment_sampling("importance")     # (kept: every later upload builds the table)
                ms = []
                for _ in range(a.repeat + 1):
                    t.on_scene_loaded(s)
                    ms.append(t.environment_build_ms())
                result["build_ms"][str(n)] = statistics.median(ms[1:])
                say(f"n = {n:5d}  {result['build_ms'][str(n)]:.4f} ms   ({6 * n * n} texels)")
            finally:
                t.destroy()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
