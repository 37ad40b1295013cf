"""rrt_render_mattes timed beside rrt_render_aov: config 5 at 1024^2 (100 802 triangles, two objects, fixed BVH), 32 samples per pixel, default fp32
handle, device buffers, K = 6 slots, "object" ids (two per frame) and "prim" ids (one per triangle: the last-slot fast path mostly misses). On the
same handle in the same run rrt_render_aov with all three planes - the call whose rays the mattes pass repeats. Each after a warm-up call, REPS
repetitions on a synchronised host clock (every call returns with the stream drained); median, min and max.

The per-kernel split comes from a run of its own: this script starts `rocprofv3 --kernel-trace --stats` (no counters) over a child process of
itself per call (reps + 1 calls each, the warm-up included), and reads the kernels' launches and total times from the stats table. --no-profile skips it.

Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/mattes_time.json.
Usage: python tools/mattes_time.py [reps] [--no-profile]"""
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

W = H = 1024
SPP, K = 32, 6
RECT = (0, 0, W, H)


def make(wd):
    cfg, root = scenes.cfg5(wd, xres=W, yres=H, nsamp=SPP + 1, max_depth=8)
    return Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def calls(r):
    """{name: a function that makes the call once on zeroed device buffers}"""
    planes = [zeros(H, W, 4) for _ in range(3)]
    ids, cov, wgt = zeros(H, W, K, dtype=torch.int32), zeros(H, W, K), zeros(H, W, 4)
    rect = (C.c_int32 * 4)(*RECT)
    prim_ids = {by: r.scene.prim_ids(by) for by in ("object", "prim")}

    def aov():
        for b in planes: b.zero_()
        d = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, *[b.data_ptr() for b in planes])
        assert A.lib().rrt_render_aov(r._h, rect, 0, 1, 0, C.byref(d)) == A.RRT_OK, A.lib().rrt_last_error()

    def mattes(by):
        def run():
            ids.zero_(); cov.zero_(); wgt.zero_()
            r.render_mattes_device(RECT, ids.data_ptr(), cov.data_ptr(), wgt.data_ptr(), K, ids=prim_ids[by])
        return run

    return {"aov_ms": aov, "mattes_object_ms": mattes("object"), "mattes_prim_ms": mattes("prim")}, (ids, cov, wgt)


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def child(reps, which):
    """the profiled process: one of the calls, reps + 1 times"""
    r = make(tempfile.mkdtemp())
    fns, _ = calls(r)
    for _ in range(reps + 1): fns[which]()
    r.close()


def kernel_split(reps, which):
    """per kernel of one call: launches and total time over reps + 1 calls (the warm-up included), from a profiled child process"""
    out_dir = tempfile.mkdtemp()
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child=" + which, str(reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("rocprofv3 run failed: " + p.stderr[-2000:])
    f = sorted(glob.glob(out_dir + "/**/*kernel_stats.csv", recursive=True))[0]
    split = {}
    for row in csv.DictReader(open(f)):
        m = re.search(r"(k_\w+)<", row["Name"]) or re.search(r"(k_\w+)", row["Name"])
        if not m: continue
        e = split.setdefault(m.group(1), dict(calls=0, total_us=0.0))
        e["calls"] += int(row["Calls"]); e["total_us"] += float(row["TotalDurationNs"]) / 1e3
    for e in split.values(): e["avg_us"] = e["total_us"] / max(1, e["calls"])
    return split


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 5
    for a in sys.argv[1:]:
        if a.startswith("--child="):
            return child(reps, a.split("=", 1)[1])
    r = make(tempfile.mkdtemp())
    fns, (ids, cov, wgt) = calls(r)
    out = {"reps": reps, "film": [W, H], "spp": SPP, "slots": K}
    for name, fn in fns.items():
        fn()      # warm-up: the first call sizes the pools and allocates the records and the table
        out[name] = timed(fn, reps)
        if name.startswith("mattes"):
            w = wgt.cpu().numpy()
            hit = w[..., 1] > 0
            out[name.replace("_ms", "_table")] = {"hit_pixels": int(hit.sum()), "overflow_share_of_hit_pixels": float((w[..., 2][hit] > 0).mean()),
                                                  "mean_used_slots": float((cov.cpu().numpy()[hit] != 0).sum(-1).mean())}
    r.close()
    for by in ("object", "prim"):
        out[f"mattes_{by}_over_aov"] = out[f"mattes_{by}_ms"]["median"] / out["aov_ms"]["median"]
    if "--no-profile" not in sys.argv:
        out["kernel_split_us"] = {name: kernel_split(reps, name) for name in fns}
    line = json.dumps(out)
    print(line)
    if os.environ.get("RRT_RESULTS_DIR"):
        os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "mattes_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
