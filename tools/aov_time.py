"""rrt_render_aov timed beside the frame: config 4 at 1024^2 (100 352 triangles, 256 spp, depth 8, fixed BVH), default fp32 handle, device planes.
render_aov for max_samples 8, 32 and 256 and the full frame, each after a warm-up, REPS repetitions on a synchronised host clock (both calls return
with the stream drained). Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/aov_time.json.
Usage: python tools/aov_time.py [reps] [key=value ...] (handle options)."""
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
W = H = 1024
cfg, root = scenes.cfg4(tempfile.mkdtemp(), xres=W, yres=H, nsamp=257, max_depth=8)
r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
for k, v in (a.split("=") for a in args):
    r.set_option(k, float(v))
film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
planes = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
torch.cuda.synchronize()
aov = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, *[p.data_ptr() for p in planes])
rect = (C.c_int32 * 4)(0, 0, W, H)


def frame():
    return r.render_device((0, 0, W, H), film.data_ptr(), stats=True)


def aov_pass(k):
    rc = A.lib().rrt_render_aov(r._h, rect, 0, 1, k, C.byref(aov))
    assert rc == A.RRT_OK, A.lib().rrt_last_error()


def timed(fn):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


for _ in range(2):      # warm-up: the first frame builds the tile trees and sizes the pools
    st = frame()
out = {"reps": reps, "frame_ms": timed(frame), "frame_ms_raygen_closest": [st.ms_raygen, st.ms_closest], "camera_rays_per_frame": int(st.camera_rays)}
for k in (8, 32, 256):
    for _ in range(2):
        aov_pass(k)
    out[f"aov_ms_{k}"] = timed(lambda: aov_pass(k))
w_live = float(planes[0][..., 3].sum().item())
out["live_weight_accumulated"] = w_live
r.close()
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "aov_time.json"), "w") as f:
        f.write(line + "\n")
