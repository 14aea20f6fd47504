#!/usr/bin/env python3
"""What adaptive sampling costs on one GPU, and what render_adaptive does against render_converged.

* The HIP-event time of the mask kernel, the compaction kernel and the sentinel fill of the sample
  slots, Cornell at 1080p and 4K with the scene's filter (ext_timing, dcrt_tracer_adaptive_timings):
  the film holds `--images` images, the list is rebuilt at the median of the blocks' largest
  errors (so about half of the blocks hold a noisy pixel), and one listed image is rendered so
  that the fill runs.
* Cornell 1080p, 8 bounces, the scene's filter, check points every 16 images: render_adaptive
  against render_converged on the same tracer at threshold 0.05 / fraction 0.95 (the README's
  convergence line) and at a harder threshold that render_converged does not meet within
  `--max-images`. For both: wall time, images, pixel samples against images x pixels, and the
  converged fraction at the end.

    python tools/bench_adaptive.py [--images 16] [--repeat 5] [--max-images 512] [--hard 0.02]

The last line is JSON.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def kernel_times(t, images, repeat):
    """Median HIP-event ms of the mask, compaction and fill kernels; the blocks left active."""
    t.set_convergence(True)
    t.set_adaptive(True)
    t.render_images(0, images)
    stats, pix, _ = t.noise(0.05, maps=True)
    H, W = pix.shape
    pad = np.zeros((-(-H // 8) * 8, -(-W // 8) * 8), np.float32)
    pad[:H, :W] = pix
    worst = pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).max((1, 3))
    threshold = float(np.median(worst))        # half of the blocks hold a pixel over it (more are active: the margin)
    t.set_instrumentation(False, True)
    rows = []
    active = 0
    for _ in range(repeat):
        active = t.update_sample_blocks(threshold)
        if active:
            t.render_images(images, 1)         # (a listed image: the fill runs first)
        rows.append(t.adaptive_timings())
    t.set_instrumentation(False, False)
    out = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    out["active_blocks"] = active
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16, help="images in the film when the kernels are timed")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-images", type=int, default=512)
    ap.add_argument("--hard", type=float, default=0.02, help="the harder threshold")
    a = ap.parse_args()
    from directcomputeraytracing_amd import ConvergeParams, Scene, WavefrontPathTracer, scenes
    result = {"kernels_ms": {}, "render": {}}
    for name, (W, H) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        s = Scene((W, H))
        scenes.setup_cornell(s, W, H, 8)
        t = WavefrontPathTracer(path_pool_size=1 << 22)
        try:
            t.on_scene_loaded(s)
            k = kernel_times(t, a.images, a.repeat)
            k["total_blocks"] = -(-W // 8) * -(-H // 8)
            result["kernels_ms"][name] = k
            print(f"{name}: mask {k['mask_ms']:.4f} ms, compaction {k['compact_ms']:.4f} ms, fill {k['fill_ms']:.4f} ms "
                  f"({k['active_blocks']} of {k['total_blocks']} blocks active, median of {a.repeat})")
            if name != "1080p":
                continue
            for threshold in (0.05, a.hard):
                p = ConvergeParams(threshold, 0.95, 16, a.max_images, 16)
                row = {}
                for which in ("render_converged", "render_adaptive"):
                    t.set_adaptive(which == "render_adaptive")
                    t.clear_film()
                    t.prepare_images(16)      # (the batch's sample textures and graphs, outside the timed region)
                    t.synchronize()
                    t0 = time.perf_counter()
                    if which == "render_converged":
                        stats, converged = t.render_converged(0, p)
                        samples = stats["images"] * W * H
                    else:
                        stats, converged, report = t.render_adaptive(0, p)
                        samples = report["pixel_samples"]
                    t.synchronize()
                    wall = time.perf_counter() - t0
                    row[which] = {"seconds": wall, "images": stats["images"], "converged": converged, "pixel_samples": samples,
                                  "full_samples": stats["images"] * W * H,
                                  "converged_fraction": stats["converged_pixels"] / max(1, stats["valid_pixels"])}
                    r = row[which]
                    print(f"1080p threshold {threshold} {which}: {wall:.3f} s, {r['images']} images, converged {converged}, "
                          f"{samples / 1e6:.1f} M pixel samples of {r['full_samples'] / 1e6:.1f} M, "
                          f"{r['converged_fraction']:.4f} of the pixels under the threshold")
                result["render"][str(threshold)] = row
        finally:
            t.destroy()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
