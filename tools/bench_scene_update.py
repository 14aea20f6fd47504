#!/usr/bin/env python3
"""Edit-to-next-sample latency of a material edit: the partial update against the full reload.

    python tools/bench_scene_update.py [--config spaceship] [--runs 5] [--out profiles/scene_update_latency.txt]
                                       [--commit ID] [--box NAME] [--small]

On the spaceship config (8 instances of the 261 k-triangle hull) a roughness edit is timed, wall
clock, from the setter to synchronize() after the first following render(), two ways:

  partial  set_material (re-flattens the materials only) -> acquire_dirty -> apply_edits
           (dcrt_tracer_update_materials + frame parameters) -> reset_image -> render
  full     what the edit cost before the partial paths: set_material + the full flatten
           (dcrt_scene_flatten) -> on_scene_loaded (dcrt_tracer_upload_scene + frame parameters)
           -> reset_image -> render

Median of --runs runs after one warm-up each. The upload counters of each way are printed with
the times: the partial way sends no geometry byte. Recorded, not gated.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def box() -> str:
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown device"


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or "unknown"
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="spaceship")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pool", type=int, default=1 << 22)
    ap.add_argument("--iterations", type=int, default=2, help="iterations of the render() that follows the edit")
    ap.add_argument("--scene-dir", default="/tmp/dcrt_scenes")
    ap.add_argument("--small", action="store_true", help="the reduced meshes (a quick check of the tool)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--box", default=None, help="the machine, where the device-name query gives nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from directcomputeraytracing_amd import Scene, WavefrontPathTracer, scenes
    scene = Scene((1920, 1080))
    what = scenes.setup_config(scene, args.config, args.scene_dir, small=args.small)
    tracer = WavefrontPathTracer(path_pool_size=args.pool, iterations_per_render=args.iterations)
    try:
        tracer.on_scene_loaded(scene)
        scene.acquire_dirty()
        tracer.render()
        tracer.synchronize()
        flat = scene.flat()
        index = 0
        setting = scene.material_setting(index)

        def edit(k):
            # the roughness slider: every other field as it is
            scene.set_material(index, setting.material_type, tuple(setting.albedo), 0.05 + 0.9 * ((k % 7) / 7.0), tuple(setting.ior),
                               tuple(setting.k), bool(setting.multiscattering), bool(setting.is_two_sided))

        def partial(k):
            t0 = time.perf_counter()
            edit(k)
            tracer.apply_edits(scene, scene.acquire_dirty())
            tracer.reset_image()
            tracer.render()
            tracer.synchronize()
            return time.perf_counter() - t0

        def full(k):
            t0 = time.perf_counter()
            edit(k)
            scene.flatten()
            scene.acquire_dirty()
            tracer.on_scene_loaded(scene)
            tracer.reset_image()
            tracer.render()
            tracer.synchronize()
            return time.perf_counter() - t0

        results = {}
        for name, fn in (("partial", partial), ("full", full)):
            fn(0)                                                   # warm-up
            s0 = tracer.upload_stats()
            times = [fn(k + 1) for k in range(args.runs)]
            s1 = tracer.upload_stats()
            results[name] = (statistics.median(times), times, {k: s1[k] - s0[k] for k in s1})
        lines = [
            f"scene update latency: a roughness edit to synchronize() after the first following render() ({args.iterations} iterations)",
            f"box: {args.box or box()}   commit: {args.commit or commit()}",
            f"scene: {what}; {flat.triangle_count} triangles, {flat.bvh_node_count} nodes, {flat.material_count} materials, "
            f"{flat.light_count} lights; pool {args.pool}",
        ]
        for name, (med, times, d) in results.items():
            lines.append(f"{name:8s} median {med * 1e3:10.3f} ms of {args.runs} ({', '.join(f'{t * 1e3:.3f}' for t in times)}); per run: "
                         f"scene uploads {d['scene_uploads'] / args.runs:g}, geometry bytes {d['geometry_bytes'] // args.runs}, "
                         f"shading bytes {d['shading_bytes'] // args.runs}, graph invalidations {d['graph_invalidations'] / args.runs:g}")
        lines.append(f"ratio full / partial: {results['full'][0] / results['partial'][0]:.1f}x")
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text)
    finally:
        tracer.destroy()


if __name__ == "__main__":
    main()
