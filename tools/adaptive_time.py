"""rrt_render_adaptive timed beside the uniform moments frame it shortens: configs 4 and 5 (depth 8, fixed BVH) at 1024^2, K = 256 samples per pixel,
default fp32 handle, device buffers.

listed_pass:  the price of losing tile trees. The uniform frame (rrt_render_moments, 256 samples in rect passes) gives the cost per sample of a full
              pass; rrt_render_adaptive with threshold 0, min_samples 16 and batch 240 renders the same frame as 16 samples of rect passes and ONE
              listed round of 240 samples over every tile, so (its time - 16 x the full cost per sample) / 240 is the cost per sample of a listed pass.
rounds:       threshold 0 with batch 16 is the same frame in 15 listed rounds: (that time - the one-round time) / 14 is what a round costs beyond its
              samples - k_tile_error, k_tile_select, the 4-byte read-back with its synchronisation, and the shorter passes. The two kernels' own times
              come from a run of its own: `rocprofv3 --kernel-trace --stats` (no counters) over a child process of this script (--no-profile skips it).
thresholds:   samples taken and frame time at a few thresholds (defaults otherwise: min_samples 16, batch 16), and the same with batch 240: one listed
              round that takes the tiles above the threshold straight to K.
equal_time:   RGB RMSE against a 1024-sample frame of the adaptive frame at each threshold and of the uniform frame whose sample count costs the same
              time (the adaptive frame's time / the full cost per sample, rounded down, at least 2), both also after rrt_denoise_moments under the planes of at most
              32 samples per pixel. Reported, not barred.

Each timing after a warm-up, REPS repetitions on a synchronised host clock (every call returns with the stream drained).
Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/adaptive_time.json.
Usage: python tools/adaptive_time.py [reps] [--no-profile] [--configs cfg4,cfg5]"""
import argparse
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
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes
from rs_ray_toy_amd import _abi as A

W = H = 1024
RECT = (0, 0, W, H)
K = 256
REFERENCE_SPP = 1024
THRESHOLDS = (0.02, 0.05, 0.1, 0.2)
RGB_FROM_XYZ = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])


def make(config, spp, wd):
    cfg, root = (scenes.cfg4 if config == "cfg4" else scenes.cfg5)(wd, xres=W, yres=H, nsamp=spp + 1, max_depth=8)
    return Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)


def buffers(n):
    return [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(n)]


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def rgb(film):
    f = film.cpu().numpy().astype(np.float64)
    return np.where(f[..., 3:4] > 0, (f[..., :3] / np.maximum(f[..., 3:4], 1e-300)) @ RGB_FROM_XYZ.T, 0.0)


def denoised(r, film, mom, spp):
    a, n, d, out = buffers(4)
    aov = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, a.data_ptr(), n.data_ptr(), d.data_ptr())
    rc = A.lib().rrt_render_aov(r._h, (C.c_int32 * 4)(*RECT), 0, 1, min(spp, 32), C.byref(aov))
    assert rc == A.RRT_OK, A.lib().rrt_last_error()
    r.denoise_device(film.data_ptr(), [a.data_ptr(), n.data_ptr(), d.data_ptr()], out.data_ptr(), moments_ptr=mom.data_ptr())
    return out


def measure(config, wd, reps):
    out = {}
    r = make(config, REFERENCE_SPP, wd)
    ref_film, = buffers(1)
    r.render_device(RECT, ref_film.data_ptr(), stats=False)
    clean = rgb(ref_film)
    r.close()
    del ref_film
    rmse = lambda film: float(np.sqrt(((rgb(film) - clean) ** 2).mean()))

    r = make(config, K, wd)
    film, mom = buffers(2)
    tiles = torch.zeros((H // 8, W // 8), dtype=torch.int32, device="cuda:0")

    def fresh():
        film.zero_(); mom.zero_()

    uniform = lambda: r.render_moments_device(RECT, film.data_ptr(), mom.data_ptr(), stats=False)
    adaptive = lambda **p: r.render_adaptive_device(RECT, film.data_ptr(), mom.data_ptr(), tiles.data_ptr(), stats=True, **p)
    for _ in range(2):      # warm-up: the first frame builds the tile trees and sizes the pools, the first adaptive frame allocates its lists
        uniform(); adaptive(threshold=0.0, min_samples=16, batch=240)
    t_uniform = timed(uniform, reps)
    t_one = timed(lambda: adaptive(threshold=0.0, min_samples=16, batch=240), reps)
    t_many = timed(lambda: adaptive(threshold=0.0, min_samples=16, batch=16), reps)
    full = t_uniform["median"] / K
    out["uniform_ms"] = t_uniform
    out["listed_pass"] = dict(adaptive_threshold0_one_round_ms=t_one, full_pass_ms_per_sample=full, listed_pass_ms_per_sample=(t_one["median"] - 16 * full) / 240)
    out["rounds"] = dict(adaptive_threshold0_15_rounds_ms=t_many, ms_per_round_beyond_its_samples=(t_many["median"] - t_one["median"]) / 14)
    out["thresholds"] = {}
    plans = []
    for T in THRESHOLDS:
        adaptive(threshold=T)
        t = timed(lambda: adaptive(threshold=T), reps)
        fresh()
        st = adaptive(threshold=T)
        counts = tiles.cpu().numpy()
        res = dict(frame_ms=t, camera_samples=int(st.camera_samples), share_of_uniform=float(st.camera_samples) / (W * H * K), mean_samples=float(counts.mean()),
                   tiles_at_min=float((counts == 16).mean()), tiles_at_K=float((counts == K).mean()), rgb_rmse=rmse(film), rgb_rmse_denoised=rmse(denoised(r, film, mom, 16)))
        # the same threshold with ONE listed round up to K (batch = K - 16): what the rounds themselves cost at this threshold
        adaptive(threshold=T, batch=K - 16)
        t1 = timed(lambda: adaptive(threshold=T, batch=K - 16), reps)
        fresh()
        st1 = adaptive(threshold=T, batch=K - 16)
        res["one_round_to_K"] = dict(frame_ms=t1, camera_samples=int(st1.camera_samples), share_of_uniform=float(st1.camera_samples) / (W * H * K), rgb_rmse=rmse(film),
                                     rgb_rmse_denoised=rmse(denoised(r, film, mom, 16)))
        out["thresholds"][str(T)] = res
        plans.append((T, max(2, int(t["median"] / full))))
    fresh()
    uniform()
    out["uniform_rgb_rmse"] = dict(rgb_rmse=rmse(film), rgb_rmse_denoised=rmse(denoised(r, film, mom, K)))
    r.close()
    for T, spp in plans:      # the uniform frame that costs the adaptive frame's time
        r = make(config, spp, wd)
        fresh()
        uniform = lambda: r.render_moments_device(RECT, film.data_ptr(), mom.data_ptr(), stats=False)
        uniform()
        t = timed(uniform, max(2, reps // 2))
        fresh()
        uniform()
        out["thresholds"][str(T)]["uniform_at_equal_time"] = dict(spp=spp, frame_ms=t, rgb_rmse=rmse(film), rgb_rmse_denoised=rmse(denoised(r, film, mom, spp)))
        r.close()
    return out


def child(reps):
    """the profiled process: config 4, threshold 0, 15 listed rounds a frame"""
    r = make("cfg4", K, tempfile.mkdtemp())
    film, mom = buffers(2)
    for _ in range(reps + 1):
        r.render_adaptive_device(RECT, film.data_ptr(), mom.data_ptr(), None, stats=False, threshold=0.0, min_samples=16, batch=16)
    r.close()


def kernel_split(reps):
    out_dir = tempfile.mkdtemp()
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), str(reps), "--child"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    if p.returncode != 0:
        raise RuntimeError("rocprofv3 run failed: " + p.stderr[-2000:])
    f = sorted(glob.glob(out_dir + "/**/*kernel_stats.csv", recursive=True))[0]
    split = {}
    for row in csv.DictReader(open(f)):
        m = re.search(r"(k_tile_error|k_tile_select|k_film_box_moments<\w+, true>|k_film_box_moments|k_pixel_offsets_list|k_pixel_offsets)", row["Name"])
        if m: split[m.group(1)] = dict(calls=int(row["Calls"]), avg_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3)
    return split


def keep(line):
    print(line)
    if os.environ.get("RRT_RESULTS_DIR"):
        os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "adaptive_time.json"), "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 run over a child process")
    ap.add_argument("--configs", default="cfg4,cfg5", help="comma-separated: cfg4, cfg5")
    ap.add_argument("--child", action="store_true", help="(internal) the profiled process")
    args = ap.parse_args()
    reps, configs = args.reps, [c for c in args.configs.split(",") if c]
    if args.child:
        return child(reps)
    out = {"reps": reps, "film": [W, H], "K": K, "reference_spp": REFERENCE_SPP}
    for config in configs:
        out[config] = measure(config, tempfile.mkdtemp(), reps)
        keep(json.dumps(out))      # kept as it grows: a later step that runs out of time loses nothing
    if not args.no_profile:
        out["kernel_split_us_cfg4_threshold0_15_rounds"] = kernel_split(2)
        keep(json.dumps(out))


if __name__ == "__main__":
    main()
