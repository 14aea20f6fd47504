"""`python tests/light_truth.py --write`: tests/golden/path_truth_lights.json, the expected sample radiance of the
scenes of tests/light_scenes.py from tests/path_ref.py with mis_model=False -- under power-proportional light
selection (include/dcrt.h, "light selection") the light sampler reports the density it draws from, so the MIS pair is
unbiased and the rendering equation alone is the estimand. (tests/golden/path_truth.json models the doubled sampler pdf
of uniform selection and does not apply to this mode on mesh-lit scenes.) The layout is path_truth.json's, so
path_ref.fixture_entry reads it; the paths are split over processes, each with its own seed, and pooled."""
import json
import sys
import time
from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent / "golden" / "path_truth_lights.json"
PARTS = 8


def load_fixture():
    return json.loads(FIXTURE.read_text())


def _part(args):
    import tempfile

    import light_scenes as LS
    import path_ref as PR
    name, paths, seed = args
    luts = dict(np.load(FIXTURE.parent / "bxdf_luts.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        scene = LS.load(name, tmp)
        ref = PR.PathRef(scene.flat(), scene.frame_params(0), luts, mis_model=False)
        return ref.region_statistics(seed, paths, LS.SCENES[name]["bounces"])


def scene_statistics(name, paths, seed, pool=None):
    """region_statistics of `paths` paths in PARTS independent parts (seeds seed, seed + 1, ...), pooled: per case the
    count-weighted mean and the standard error of the pooled sample."""
    jobs = [(name, paths // PARTS, seed + k) for k in range(PARTS)]
    parts = pool.map(_part, jobs) if pool else [_part(j) for j in jobs]
    out = {}
    for key in ("visible", "hidden"):
        c = np.stack([p[key]["count"] for p in parts]).astype(np.float64)[:, None, :, None]       # (parts, 1, regions, 1)
        mean = np.stack([p[key]["mean"] for p in parts])
        second = np.stack([p[key]["sem"] for p in parts]) ** 2 * c + mean ** 2                        # E[x^2] per part
        n = c.sum(0)
        m = (mean * c).sum(0) / n
        var = np.maximum((second * c).sum(0) / n - m * m, 0.0)
        out[key] = {"mean": m, "sem": np.sqrt(var / n), "count": n[0, :, 0].astype(np.int64)}
    return out


def main(argv):
    if "--write" not in argv:
        print(__doc__)
        return 1
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import multiprocessing

    import light_scenes as LS
    fx = {"seed": LS.SEED, "regions": 2, "resolution": [LS.SIZE, LS.SIZE], "scenes": {}}
    with multiprocessing.get_context("spawn").Pool(PARTS) as pool:
        for i, (name, spec) in enumerate(LS.SCENES.items()):
            t0 = time.time()
            seed = LS.SEED + 1000 * i
            st = scene_statistics(name, spec["paths"], seed, pool)
            cases = {}
            for vis in spec["visible"]:
                key = "visible" if vis else "hidden"
                cases[key] = {str(b): {"mean": st[key]["mean"][j].round(9).tolist(), "sem": st[key]["sem"][j].round(9).tolist()}
                              for j, b in enumerate(spec["bounces"])}
            fx["scenes"][name] = {"paths": spec["paths"], "seed": seed, "parts": PARTS, "count": st["visible"]["count"].tolist(),
                                  "seconds": round(time.time() - t0, 1), "cases": cases}
            print(name, fx["scenes"][name]["seconds"], "s", flush=True)
    FIXTURE.write_text(json.dumps(fx, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
