"""rrt_render_passes timed beside rrt_render_moments on one handle: config 4 at 1024^2 (100 352 triangles, three point lights, depth 8, fixed BVH), default
fp32 handle, device buffers, 32 samples per pixel. Both frames render with the per-slot radiance layout (film_records 0), so the ratio is the cost of
the pass masks, the radiance planes and one more film kernel and merge per pass - against a frame that pays for one more plane itself.

  1 pass     everything (the frame's own bits)
  4 passes   one per light, and the indirect light of all three
  16 passes  every light at vertices 0, 1, 2, 3 and >= 4, and everything: an unoccluded shadow record is added to two planes beside L

After a warm-up (tile trees, pools, the planes of the largest call), `reps` alternating rounds moments / 1 / 4 / 16 on a synchronised host clock (every
call returns with the stream drained): medians, spread and the ratio of the medians. rrt_render_stats::ms_film of further frames gives the film kernels'
own share.

Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/passes_time.json.
Usage: python tools/passes_time.py [reps] [spp]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

W = H = 1024
RECT = (0, 0, W, H)
ALL = 0xFFFFFFFF
SETS = {
    1: [(ALL, 0, 0)],
    4: [(1, 0, 0), (2, 0, 0), (4, 0, 0), (ALL, 1, 0)],
    16: [(1 << i, b, b + 1 if b < 4 else 0) for i in range(3) for b in range(5)] + [(ALL, 0, 0)],
}


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args else 10
    spp = int(args[1]) if len(args) > 1 else 32
    cfg, root = scenes.cfg4(tempfile.mkdtemp(), xres=W, yres=H, nsamp=spp + 1, max_depth=8)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    bufs = torch.zeros((18, H, W, 4), dtype=torch.float32, device="cuda:0")
    film, mom = bufs[16].data_ptr(), bufs[17].data_ptr()
    calls = {"moments": lambda stats=False: r.render_moments_device(RECT, film, mom, stats=stats)}
    for n, passes in SETS.items():
        assert len(passes) == n
        calls[f"passes_{n}"] = lambda stats=False, passes=passes: r.render_passes_device(RECT, passes, [bufs[k].data_ptr() for k in range(len(passes))], film_ptr=film, stats=stats)
    for name in ("passes_16", "moments", "passes_1", "passes_4", "passes_16", "moments"):      # warm-up, the largest call first
        calls[name]()
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {"reps": reps, "film": [W, H], "spp": spp, "config": "cfg4"}
    for name, v in ms.items():
        out[name + "_ms"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    for n in SETS:
        out[f"passes_{n}_over_moments"] = out[f"passes_{n}_ms"]["median"] / out["moments_ms"]["median"]
    for name, fn in calls.items():
        st = [fn(True) for _ in range(3)]
        out[name + "_stats"] = dict(ms_film=float(np.median([s.ms_film for s in st])), ms_shade=float(np.median([s.ms_shade for s in st])),
                                    ms_any=float(np.median([s.ms_any for s in st])), ms_total=float(np.median([s.ms_total for s in st])))
    r.close()
    line = json.dumps(out)
    print(line)
    if os.environ.get("RRT_RESULTS_DIR"):
        os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "passes_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
