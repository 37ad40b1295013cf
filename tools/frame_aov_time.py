"""rrt_render_frame_aov against the pair it replaces: config 4 at 1024^2 (100 352 triangles, depth 8, fixed BVH), default fp32 handle, device buffers.
Per sample count (8, 32 and 256 spp: scenes with nsamp 9, 33, 257) rrt_render_moments + rrt_render_aov(max_samples 32) and
rrt_render_frame_aov(aov_max_samples 32) on ONE handle, after a warm-up, REPS rounds that alternate the two routes, each call timed on a synchronised
host clock (every call returns with the stream drained); medians. Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as
<dir>/frame_aov_time.json.
Usage: python tools/frame_aov_time.py [reps] [spp=8,32,256] [key=value ...] (handle options)

The split between the first-hit shading and the gather comes from a kernel trace of its own (the timed run carries no profiler):
    rocprofv3 --kernel-trace --output-format csv -d results/frame_aov_prof -- python3 tools/frame_aov_time.py 3 spp=32
    python tools/frame_aov_time.py --split results/frame_aov_prof
sums, over the LAST fused call of the trace, the dispatches by family."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def split(trace_dir):
    import csv
    import glob
    f = sorted(glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the last fused call is the last call of the run (rounds end with it): everything after the merge kernels of the call before it
    shade = [i for i, r in enumerate(rows) if "k_aov_shade_frame" in r["Kernel_Name"]]
    before = [i for i, r in enumerate(rows) if i < shade[-1] and ("k_aov_merge" in r["Kernel_Name"] or "k_film_add" in r["Kernel_Name"])]
    first = before[-1] + 1 if before else 0
    per_call = len([i for i in shade if i >= first])
    families = (("k_aov_shade_frame", ("k_aov_shade_frame",)), ("gather", ("k_gather_box", "k_gather_wide")), ("merge", ("k_aov_merge", "k_film_add")),
                ("camera", ("k_pixel_offsets", "k_raygen")), ("traversal", ("k_trace_", "k_closest", "k_tt_snapshot")), ("shading", ("k_shade_",)),
                ("film", ("k_film_",)))
    total = {}
    for r in rows[first:]:
        fam = next((k for k, keys in families if any(s in r["Kernel_Name"] for s in keys)), "other")
        total[fam] = total.get(fam, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    span = (int(rows[-1]["End_Timestamp"]) - int(rows[first]["Start_Timestamp"])) / 1e6
    out = {"last_fused_call_kernel_ms": {k: round(v, 4) for k, v in total.items()}, "first_launch_to_last_end_ms": round(span, 4), "passes": per_call}
    print(json.dumps(out))


if len(sys.argv) > 2 and sys.argv[1] == "--split":
    split(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 10
spps = (8, 32, 256)
if args and args[0].startswith("spp="):
    spps = tuple(int(v) for v in args.pop(0)[4:].split(","))
W = H = 1024
K = 32      # the feature buffers' samples: what rrt_render and deploy_render hand the denoiser
wd = tempfile.mkdtemp()
bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(5)]      # film, moments, albedo, normal, depth
torch.cuda.synchronize()
film, mom, planes = bufs[0].data_ptr(), bufs[1].data_ptr(), [b.data_ptr() for b in bufs[2:]]
aov = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, *planes)
rect = (C.c_int32 * 4)(0, 0, W, H)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


out = {"reps": reps, "aov_max_samples": K}
for spp in spps:
    cfg, root = scenes.cfg4(wd, xres=W, yres=H, nsamp=spp + 1, max_depth=8)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    for k, v in (a.split("=") for a in args):
        r.set_option(k, float(v))

    def moments():
        r.render_moments_device((0, 0, W, H), film, mom, stats=False)

    def aov_pass():
        rc = A.lib().rrt_render_aov(r._h, rect, 0, 1, K, C.byref(aov))
        assert rc == A.RRT_OK, A.lib().rrt_last_error()

    def fused():
        r.render_frame_aov_device((0, 0, W, H), film, mom, *planes, max_samples=K, stats=False)

    for _ in range(2):      # warm-up: the first frame builds the tile trees and sizes the pools
        moments(); aov_pass(); fused()
    t = {"moments": [], "aov": [], "fused": []}
    for _ in range(reps):   # alternating rounds
        t["moments"].append(clock(moments))
        t["aov"].append(clock(aov_pass))
        t["fused"].append(clock(fused))
    pair = [a + b for a, b in zip(t["moments"], t["aov"])]
    out[f"spp_{spp}"] = {"moments_ms": stat(t["moments"]), "aov_ms": stat(t["aov"]), "two_calls_ms": stat(pair), "fused_ms": stat(t["fused"]),
                         "feature_cost_two_calls_ms": float(np.median(t["aov"])), "feature_cost_fused_ms": float(np.median(t["fused"]) - np.median(t["moments"]))}
    r.close()
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "frame_aov_time.json"), "w") as f:
        f.write(line + "\n")
