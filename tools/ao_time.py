"""rrt_render_ao timed beside rrt_render_aov: config 4 at 1024^2 (100 352 triangles, fixed BVH), default fp32 handle, planes in device memory,
max_samples 8, 16 draws per hit (cosine). Both calls on one handle in one run, alternating, every shape warmed first, device events on the handle's
stream around each call; median, min and max over REPS repetitions. The frame's own any-hit figure comes from the same handle: one frame with the
option frame_stats on (any_queries / ms_any: what `bench.py --full` reports one frame at a time).

The per-kernel split comes from a run of its own: this script starts `rocprofv3 --kernel-trace --stats` (no counters) over a child process of itself
that makes the rrt_render_ao call reps + 1 times (the warm-up included), and reads k_ao_gen, the any-hit launches (the k_trace_* instantiations whose
first template argument is true) and k_gather_box (the gather over AoAcc) from the stats table; any-hit rays per second = hit samples x draws / any-hit kernel time.
--no-profile skips it.

Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/ao_time.json.
Usage: python tools/ao_time.py [reps] [--no-profile]"""
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

W = H = 1024
SPP, DRAWS = 8, 16
RECT = (0, 0, W, H)


def make(wd):
    cfg, root = scenes.cfg4(wd, xres=W, yres=H, nsamp=257, max_depth=8)
    return Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)


def calls(r):
    """{name: a function that makes the call once, into device planes that run on (+=)}, and the planes"""
    planes = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(5)]
    torch.cuda.synchronize()
    rect = (C.c_int32 * 4)(*RECT)
    aov_d = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, *[b.data_ptr() for b in planes[:3]])
    ao_d = A.Ao(A.RRT_MEM_DEVICE, RRT_F32, planes[3].data_ptr(), planes[4].data_ptr())
    prm = A.AoParams(DRAWS, 1)

    def aov():
        assert A.lib().rrt_render_aov(r._h, rect, 0, 1, SPP, C.byref(aov_d)) == A.RRT_OK, A.lib().rrt_last_error()

    def ao():
        assert A.lib().rrt_render_ao(r._h, rect, 0, 1, SPP, C.byref(prm), C.byref(ao_d)) == A.RRT_OK, A.lib().rrt_last_error()

    return {"aov_ms": aov, "ao_ms": ao}, planes


def child(reps):
    """the profiled process: the rrt_render_ao call, reps + 1 times"""
    r = make(tempfile.mkdtemp())
    fns, _ = calls(r)
    for _ in range(reps + 1): fns["ao_ms"]()
    r.close()


def kernel_split(reps):
    out_dir = tempfile.mkdtemp()
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child", str(reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("rocprofv3 run failed: " + p.stderr[-2000:])
    f = sorted(glob.glob(out_dir + "/**/*kernel_stats.csv", recursive=True))[0]
    split = {}
    for row in csv.DictReader(open(f)):
        m = re.search(r"(k_\w+)", row["Name"])
        if not m: continue
        name = m.group(1)
        t = re.search(r"k_trace_\w+<(true|false)", row["Name"])
        if t: name += "<any>" if t.group(1) == "true" else "<closest>"
        e = split.setdefault(name, dict(calls=0, total_us=0.0))
        e["calls"] += int(row["Calls"]); e["total_us"] += float(row["TotalDurationNs"]) / 1e3
    for e in split.values(): e["avg_us"] = e["total_us"] / max(1, e["calls"])
    return split


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    if "--child" in sys.argv:
        return child(reps)
    r = make(tempfile.mkdtemp())
    fns, planes = calls(r)
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):      # warm-up: the first frame builds the tile trees and sizes the pools
        r.render_device(RECT, film.data_ptr(), stats=True)
    r.set_option("frame_stats", 1)
    st = r.render_device(RECT, film.data_ptr(), stats=True)
    r.set_option("frame_stats", 0)
    for fn in fns.values():
        for _ in range(2): fn()
    stream = torch.cuda.ExternalStream(r.stream)
    ms = {name: [] for name in fns}
    for _ in range(reps):       # alternating
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    n_calls = reps + 2
    hit_samples = float(planes[3][..., 2].sum().item()) / n_calls      # box filter: one unit of weight per hit sample
    out = {"reps": reps, "film": [W, H], "max_samples": SPP, "n_samples": DRAWS, "hit_samples_per_call": hit_samples, "any_rays_per_call": hit_samples * DRAWS}
    for name in fns:
        out[name] = dict(median=float(np.median(ms[name])), min=float(min(ms[name])), max=float(max(ms[name])))
    out["ao_over_aov"] = out["ao_ms"]["median"] / out["aov_ms"]["median"]
    out["frame_any"] = {"any_queries": int(st.any_queries), "ms_any": float(st.ms_any), "any_rays_per_s": float(st.any_queries) / (float(st.ms_any) * 1e-3) if st.ms_any > 0 else None}
    r.close()
    if "--no-profile" not in sys.argv:
        split = kernel_split(reps)
        out["kernel_split_us"] = split
        any_us = sum(e["total_us"] for k, e in split.items() if k.endswith("<any>"))
        out["ao_kernels_ms_per_call"] = {k: split[k]["total_us"] / 1e3 / (reps + 1) for k in ("k_ao_gen", "k_gather_box") if k in split}
        out["ao_kernels_ms_per_call"]["any_hit"] = any_us / 1e3 / (reps + 1)
        out["ao_any_rays_per_s"] = hit_samples * DRAWS * (reps + 1) / (any_us * 1e-6) if any_us > 0 else None
    line = json.dumps(out)
    print(line)
    if os.environ.get("RRT_RESULTS_DIR"):
        os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "ao_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
