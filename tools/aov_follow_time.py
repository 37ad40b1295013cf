"""rrt_render_aov_follow timed beside rrt_render_aov, default fp32 handle, device planes, fixed BVH. Two scenes in one visit: config 5 at its own
size (2048^2, 103 488 triangles) with its floor set to Mirror, and unmodified config 4 (1024^2, no specular material: every chain ends on its
first surface). Per scene rrt_render_aov(max_samples 32) and rrt_render_aov_follow(32, max_follow 4) alternate, REPS pairs after a warm-up of
each, on a synchronised host clock (both calls return with the stream drained); medians, and the spread of each column. No frame is rendered
first, so level 0 runs without tile trees in both columns. Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as
<dir>/aov_follow_time.json.
Usage: python tools/aov_follow_time.py [reps]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 10
SAMPLES, FOLLOW = 32, 4


def measure(cfg, root, W, H):
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    planes = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    aov = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, *[p.data_ptr() for p in planes])
    rect = (C.c_int32 * 4)(0, 0, W, H)

    def first_hit():
        rc = A.lib().rrt_render_aov(r._h, rect, 0, 1, SAMPLES, C.byref(aov))
        assert rc == A.RRT_OK, A.lib().rrt_last_error()

    def follow():
        rc = A.lib().rrt_render_aov_follow(r._h, rect, 0, 1, SAMPLES, FOLLOW, C.byref(aov))
        assert rc == A.RRT_OK, A.lib().rrt_last_error()

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):      # warm-up: pools, record buffers, code objects
        first_hit(); follow()
    ms = {"aov": [], "follow": []}
    for _ in range(reps):
        ms["aov"].append(once(first_hit))
        ms["follow"].append(once(follow))
    r.close()
    out = {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}
    out["follow_over_aov"] = out["follow"]["median"] / out["aov"]["median"]
    return out


wd = tempfile.mkdtemp()
cfg5, root5 = scenes.cfg5(os.path.join(wd, "cfg5"))
cfg5["Aggregate"]["primitives"][0]["material_name"] = "mat_mirror"       # the floor
cfg4, root4 = scenes.cfg4(os.path.join(wd, "cfg4"))
out = {"reps": reps, "max_samples": SAMPLES, "max_follow": FOLLOW,
       "cfg5_mirror_floor_2048": measure(cfg5, root5, 2048, 2048), "cfg4_1024": measure(cfg4, root4, 1024, 1024)}
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "aov_follow_time.json"), "w") as f:
        f.write(line + "\n")
