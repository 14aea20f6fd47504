#!/usr/bin/env python3
"""What power-proportional light selection costs and buys on one GPU (dcrt.h "light selection").

The scene is the test suite's `lamps` (tests/light_scenes.py): a matte floor and a blocker under a small bright lamp,
a large dim lamp, a two-triangle kite lamp, a point light, a directional light and a constant environment, at 1080p,
max_depth 2. For uniform and for power selection:

* milliseconds per image (render_images over `--images` images, the median of `--repeat` runs);
* the mean noise estimate (noise()["mean_error"]) after the same `--images` images;
* the images render_converged needs for `--threshold` at fraction 0.95, checked every 16 images, at most `--max-images`;
* the per-sample variance of the luminance over the floor's pixels at B = 0, from `--variance-images` single-image
  renders at 64 x 64 (what tests/test_gpu_light_table.py::test_variance_falls bounds), and the ratio of the two.

Then the table's build time (the HIP-event time of its kernels, the median of `--repeat` uploads) for `lamps` itself
(6 lights, 6 lamp triangles), for 1000 point lights in its place, and for one lamp of 2 * 512 * 255 = 261 120 triangles (scenes.hull_mesh(512, 256) made emissive), with the time of
the light-level kernel alone after a colour edit.

    python tools/bench_light_sampling.py [--images 32] [--repeat 5] [--threshold 0.05] [--max-images 512] [--out FILE]

The text goes to stdout and to `--out` (default profiles/light_sampling_costs.txt); the last stdout line is JSON.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

MODES = ("uniform", "power")


def lamps_scene(width, height, bounce, directory):
    import light_scenes as LS
    import path_scenes as PS
    return PS.with_case(LS.load("lamps", directory, width, height), bounce, True)


def hull_lamp_scene(directory):
    from directcomputeraytracing_amd import Scene, scenes
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    scenes.write_obj(d / "hull.obj", *scenes.hull_mesh(512, 256))
    body = ('  <integrator type="path"><integer name="max_depth" value="1"/></integrator>\n'
            + scenes._sensor("perspective", 64, 64, scenes.mitsuba_matrix((0, 0, -30)), '    <float name="fov" value="40"/>\n')
            + f'  <shape type="obj" id="hull"><string name="filename" value="hull.obj"/><emitter type="area"><rgb name="radiance" value="1, 1, 1"/></emitter>'
              f'<transform name="to_world"><matrix value="{scenes.mitsuba_matrix()}"/></transform></shape>\n')
    (d / "hull.xml").write_text(scenes._xml(body))
    s = Scene((64, 64))
    s.load_from_file(d / "hull.xml")
    s.add_point_light((0.0, 20.0, 0.0), (1.0, 1.0, 1.0))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--max-images", type=int, default=512)
    ap.add_argument("--variance-images", type=int, default=32)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "light_sampling_costs.txt"))
    a = ap.parse_args()
    from directcomputeraytracing_amd import ConvergeParams, WavefrontPathTracer, _abi
    import light_scenes as LS
    import shading_ref as R
    lines, result = [], {"render": {}, "variance": {}, "build_ms": {}}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# Power-proportional light selection: costs and effect (tools/bench_light_sampling.py)")
    say("# scene: `lamps` of tests/light_scenes.py (six lights: three lamps, a point light, a directional light, a constant environment)")
    with tempfile.TemporaryDirectory() as tmp:
        W, H = 1920, 1080
        scene = lamps_scene(W, H, 2, Path(tmp) / "hd")
        say(f"## {W} x {H}, max_depth 2, {a.images} images per run, median of {a.repeat}")
        for mode in MODES:
            t = WavefrontPathTracer(path_pool_size=1 << 22)
            try:
                t.on_scene_loaded(scene)
                t.set_light_sampling(mode)
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
                say(f"{mode:8s}  {row['ms_per_image']:.4f} ms/image   mean noise estimate after {a.images} images {row['mean_error']:.5f} "
                    f"({row['converged_fraction']:.4f} of the pixels under {a.threshold})   render_converged: {row['converge_images']} images, "
                    f"converged {row['converged']} (cap {a.max_images})")
            finally:
                t.destroy()
        small = lamps_scene(LS.SIZE, LS.SIZE, 0, Path(tmp) / "small")
        lum = np.array([0.299, 0.587, 0.114])
        for mode in MODES:
            t = WavefrontPathTracer(path_pool_size=1 << 16)
            try:
                t.on_scene_loaded(small)
                t.set_light_sampling(mode)
                floor = LS.floor_pixels(t)
                v = LS.device_samples(t, a.variance_images)[:, floor, :].reshape(-1, 3).astype(np.float64) @ lum
                result["variance"][mode] = {"mean": float(v.mean()), "variance": float(v.var()), "samples": int(v.size)}
            finally:
                t.destroy()
        ratio = result["variance"]["power"]["variance"] / result["variance"]["uniform"]["variance"]
        result["variance"]["ratio"] = ratio
        say(f"## per-sample variance over the floor's pixels, {LS.SIZE} x {LS.SIZE}, B = 0, {a.variance_images} images (luminance)")
        for mode in MODES:
            r = result["variance"][mode]
            say(f"{mode:8s}  mean {r['mean']:.5f}   variance {r['variance']:.5f}   ({r['samples']} samples)")
        say(f"ratio power / uniform: {ratio:.5f}   (float64 prototype of the light sample alone: {LS.VARIANCE_RATIO_PROTOTYPE})")
        say(f"## table build: HIP-event ms of the table's kernels, median of {a.repeat} uploads; `edit`: the light-level kernel alone after a colour edit")
        hull = hull_lamp_scene(Path(tmp) / "hull")
        base = small.flat()
        many = type(base).from_buffer_copy(base)                  # (`lamps` with 1000 point lights in place of its six lights)
        points = np.ascontiguousarray(LS.point_lights(1000, 1040))
        many.lights, many.light_count = points.ctypes.data_as(C.POINTER(_abi.Light)), len(points)
        flats = {"lamps": base, "1000 point lights": many, "261 120-triangle lamp": hull.flat()}
        for name, flat in flats.items():
            t = WavefrontPathTracer(path_pool_size=1 << 14)
            try:
                assert t._lib.dcrt_tracer_upload_scene(t._h, C.byref(flat)) == 0
                t.set_light_sampling("power")              # (kept: every later upload builds the table)
                ms, edit = [], []
                for _ in range(a.repeat + 1):
                    assert t._lib.dcrt_tracer_upload_scene(t._h, C.byref(flat)) == 0
                    ms.append(t.light_table_build_ms())
                    lights = np.ascontiguousarray(R._array(flat.lights, C.c_uint32, (flat.light_count, 7)))
                    lights[0, 0] = (lights[0, 0:1].view(np.float32) * np.float32(1.5)).view(np.uint32)[0]
                    assert t._lib.dcrt_tracer_update_lights(t._h, lights.ctypes.data_as(C.POINTER(_abi.Light)), len(lights)) == 0
                    edit.append(t.light_table_build_ms())
                d = t.light_distribution()
                result["build_ms"][name] = {"build": statistics.median(ms[1:]), "edit": statistics.median(edit[1:]), "lights": d["n"], "entries": d["entries"]}
                say(f"{name:22s}  build {result['build_ms'][name]['build']:.4f} ms   edit {result['build_ms'][name]['edit']:.4f} ms   ({d['n']} lights, {d['entries']} lamp triangles)")
            finally:
                t.destroy()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
