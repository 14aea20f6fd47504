#!/usr/bin/env python3
"""Time the film denoiser on one GPU: render_guides, denoise() in total, and every kernel of it
(HIP events through dcrt_tracer_denoise_timings: prologue, variance estimate, one entry per
a-trous pass), for the default choice of pass kernel and with each variant forced
(DCRT_DENOISE_PASS=global|tile|latticeN|lattice, all 8 steps) -- the A/B behind
DenoisePassLattice in tracer.hip.
Medians of --repeat runs after a warm-up. Next to each pass: its compulsory traffic (64 B per
pixel: the working image and the two guides read once, the result written once) as a fraction
of the HBM peak.

    python tools/bench_denoise.py [--width 1920 --height 1080 --spp 4 --iterations 5 --repeat 5]
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_PEAK = 8.0e12   # bytes/s, MI355X


def median_kernels(t, params, repeat):
    t.denoise(params)   # warm-up (allocations, code objects)
    runs, wall = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        t.denoise(params)
        wall.append((time.perf_counter() - t0) * 1e3)
        runs.append(t.denoise_timings())
    return [statistics.median(k) for k in zip(*runs)], statistics.median(wall)


def stride(variant, step):
    """What DenoisePassLattice (tracer.hip) picks: the default, or the forced stride where its span fits."""
    default = 1 if step <= 4 else step if step in (16, 32) else 0
    want = {"default": default, "global": 0, "tile": 1, "lattice": step}.get(variant)
    if want is None:
        want = min(step, int(variant[len("lattice"):]))
    L = want if want == 0 or (step % want == 0 and step // want <= 4) else default
    return "global" if L == 0 else f"L={L} taps {step // L} apart"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    from directcomputeraytracing_amd import Scene, WavefrontPathTracer, denoise_default_params, scenes
    s = Scene((a.width, a.height))
    scenes.setup_cornell(s, a.width, a.height, 8)
    t = WavefrontPathTracer(path_pool_size=1 << 22)
    try:
        t.on_scene_loaded(s)
        t.clear_film()
        t.render_images(0, a.spp)
        t.render_guides(0, 1)
        guide_ms = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            t.render_guides(0, 1)
            guide_ms.append((time.perf_counter() - t0) * 1e3)
        t.render_guides(0, a.spp)
        p = denoise_default_params()
        p.iterations = a.iterations
        px = a.width * a.height
        t.set_instrumentation(False, True)
        result = {"width": a.width, "height": a.height, "spp": a.spp, "iterations": a.iterations,
                  "render_guides_1_ms": statistics.median(guide_ms), "variants": {}}
        for variant in ("default", "global", "tile", "lattice2", "lattice4", "lattice8", "lattice"):
            if variant == "default":
                os.environ.pop("DCRT_DENOISE_PASS", None)
            else:
                os.environ["DCRT_DENOISE_PASS"] = variant
                p.iterations = 8   # (the A/B covers every step; a pass's time does not depend on the count)
            kernels, wall = median_kernels(t, p, a.repeat)
            result["variants"][variant] = {"denoise_wall_ms": wall, "kernel_ms": kernels, "kernel_sum_ms": sum(kernels)}
            print(f"{variant:8s} denoise {wall:7.3f} ms wall, kernels {sum(kernels):7.3f} ms: prologue {kernels[0]:.3f}  variance {kernels[1]:.3f}")
            for i, ms in enumerate(kernels[2:]):
                print(f"    pass {i} step {1 << i:3d} [{stride(variant, 1 << i)}]: {ms:7.3f} ms  {64 * px / (ms * 1e-3) / HBM_PEAK * 100:5.1f} % of HBM peak at 64 B/px")
        os.environ.pop("DCRT_DENOISE_PASS", None)
        print(json.dumps(result))
    finally:
        t.destroy()


if __name__ == "__main__":
    main()
