"""rrt_render_moments and rrt_denoise_moments timed beside the calls they extend: config 4 at 1024^2 (100 352 triangles, depth 8, fixed BVH), default
fp32 handle, device buffers, frames of 8, 32 and 256 samples per pixel (one scene each).

Cost of the plane, split two ways: rrt_render_rect with film_records 1 (the default: k_film_box_runs) against film_records 0 (k_film_box, the
layout a moments frame renders with) against rrt_render_moments (k_film_box_moments and one more merge). Each after a warm-up, REPS repetitions
on a synchronised host clock (every call returns with the stream drained); the film kernels' own share is rrt_render_stats::ms_film (HIP events
around the film launches) of REPS further frames that ask for statistics.

rrt_denoise against rrt_denoise_moments: the 8 spp frame, five iterations (the default), the same clock.

Quality on the device: the 8 spp frame of config 4 and of config 5 (depth 8) at 1024^2 denoised both ways, RGB RMSE against the 256 spp frame.

The per-kernel split of rrt_denoise_moments comes from a run of its own: this script starts `rocprofv3 --kernel-trace --stats` (no counters)
over a child process of itself that denoises the 8 spp frame with the plane, and reads the k_dn_* kernels' average and minimum times from the
stats table. k_dn_sample_variance's time is the most that folding the rule into k_dn_moments could save. --no-profile skips it; --split-only
runs nothing else.

Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/moments_time.json (moments_split.json for --split-only).
Usage: python tools/moments_time.py [reps] [--no-profile | --split-only]"""
import csv
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

W = H = 1024
RECT = (0, 0, W, H)
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


def film_ms(fn, reps):
    """median rrt_render_stats::ms_film and ms_total of `reps` frames that ask for statistics"""
    st = [fn() for _ in range(reps)]
    return dict(ms_film=float(np.median([s.ms_film for s in st])), ms_total=float(np.median([s.ms_total for s in st])))


def aov(r, bufs, spp):
    import ctypes as C
    from rs_ray_toy_amd import _abi as A
    d = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, *[b.data_ptr() for b in bufs])
    rc = A.lib().rrt_render_aov(r._h, (C.c_int32 * 4)(*RECT), 0, 1, min(spp, 32), C.byref(d))
    assert rc == A.RRT_OK, A.lib().rrt_last_error()


def rgb(film):
    f = film.cpu().numpy().astype(np.float64)
    return np.where(f[..., 3:4] > 0, (f[..., :3] / np.maximum(f[..., 3:4], 1e-300)) @ RGB_FROM_XYZ.T, 0.0)


def cost_of_the_plane(spp, wd, reps):
    r = make("cfg4", spp, wd)
    film, mom = buffers(2)
    plain = lambda stats=False: r.render_device(RECT, film.data_ptr(), stats=stats)
    moments = lambda stats=False: r.render_moments_device(RECT, film.data_ptr(), mom.data_ptr(), stats=stats)
    for _ in range(2):      # warm-up: the first frame builds the tile trees and sizes the pools, the first moments frame allocates its running sums
        plain(); moments()
    res = {}
    # interleaved A / B / C rounds, so that a drift of the clocks falls on all three alike
    rounds = {"frame_ms_film_records_1": [], "frame_ms_film_records_0": [], "moments_ms": []}
    for _ in range(3):
        r.set_option("film_records", 1)
        plain()
        rounds["frame_ms_film_records_1"].append(timed(plain, reps))
        r.set_option("film_records", 0)
        plain()
        rounds["frame_ms_film_records_0"].append(timed(plain, reps))
        r.set_option("film_records", 1)
        moments()
        rounds["moments_ms"].append(timed(moments, reps))
    for key, rs in rounds.items():
        res[key] = dict(median=float(np.median([x["median"] for x in rs])), min=min(x["min"] for x in rs), max=max(x["max"] for x in rs),
                        round_medians=[x["median"] for x in rs])
    r.set_option("film_records", 1)
    res["film_kernels_film_records_1"] = film_ms(lambda: plain(True), reps)
    r.set_option("film_records", 0)
    res["film_kernels_film_records_0"] = film_ms(lambda: plain(True), reps)
    r.set_option("film_records", 1)
    res["film_kernels_moments"] = film_ms(lambda: moments(True), reps)
    r.close()
    return res


def denoise_and_quality(config, wd, reps, want_times):
    """the 8 spp frame denoised both ways against the 256 spp frame; with want_times, both calls timed (five iterations)"""
    out = {}
    r = make(config, 256, wd)
    clean_film, = buffers(1)
    r.render_device(RECT, clean_film.data_ptr(), stats=False)
    clean = rgb(clean_film)
    r.close()
    r = make(config, 8, wd)
    film, mom, a, n, d, o1, o2 = buffers(7)
    r.render_moments_device(RECT, film.data_ptr(), mom.data_ptr(), stats=False)
    aov(r, (a, n, d), 8)
    planes = [a.data_ptr(), n.data_ptr(), d.data_ptr()]
    spatial = lambda: r.denoise_device(film.data_ptr(), planes, o1.data_ptr())
    sample = lambda: r.denoise_device(film.data_ptr(), planes, o2.data_ptr(), moments_ptr=mom.data_ptr())
    spatial(); sample()
    if want_times:
        rs = {"denoise_ms": [], "denoise_moments_ms": []}
        for _ in range(3):
            rs["denoise_ms"].append(timed(spatial, reps)); rs["denoise_moments_ms"].append(timed(sample, reps))
        for key, v in rs.items():
            out[key] = dict(median=float(np.median([x["median"] for x in v])), min=min(x["min"] for x in v), max=max(x["max"] for x in v))
    rmse = lambda x: float(np.sqrt(((x - clean) ** 2).mean()))
    m = mom.cpu().numpy().astype(np.float64)
    n_eff = np.where(m[..., 3] > 0, m[..., 2] ** 2 / np.maximum(m[..., 3], 1e-300), 0.0)
    out["rgb_rmse_against_256spp"] = {"noisy": rmse(rgb(film)), "spatial_variance": rmse(rgb(o1)), "sample_variance": rmse(rgb(o2))}
    out["share_of_pixels_on_the_sample_variance"] = float(((n_eff >= 2) & (m[..., 0] > 0)).mean())
    r.close()
    return out


def child(reps):
    """the profiled process: the 8 spp frame of config 4, rrt_denoise_moments with default parameters"""
    r = make("cfg4", 8, tempfile.mkdtemp())
    film, mom, a, n, d, o = buffers(6)
    r.render_moments_device(RECT, film.data_ptr(), mom.data_ptr(), stats=False)
    aov(r, (a, n, d), 8)
    for _ in range(reps + 2):
        r.denoise_device(film.data_ptr(), [a.data_ptr(), n.data_ptr(), d.data_ptr()], o.data_ptr(), moments_ptr=mom.data_ptr())
    r.close()


def kernel_split(reps):
    out_dir = tempfile.mkdtemp()
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child", str(reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    if p.returncode != 0:
        raise RuntimeError("rocprofv3 run failed: " + p.stderr[-2000:])
    f = sorted(glob.glob(out_dir + "/**/*kernel_stats.csv", recursive=True))[0]
    split = {}
    for row in csv.DictReader(open(f)):
        m = re.search(r"(k_dn_\w+)<float(?:, (\d+))?>", row["Name"])
        if not m: continue
        name = m.group(1) + (f"_s{m.group(2)}" if m.group(2) else "")
        split[name] = dict(calls=int(row["Calls"]), avg_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3)
    return split


def keep(line, name):
    print(line)
    if os.environ.get("RRT_RESULTS_DIR"):
        os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["RRT_RESULTS_DIR"], name), "w") as f:
            f.write(line + "\n")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 10
    if "--child" in sys.argv:
        return child(reps)
    if "--split-only" in sys.argv:
        return keep(json.dumps({"reps": reps, "film": [W, H], "denoise_moments_kernel_split_us": kernel_split(reps)}), "moments_split.json")
    wd = tempfile.mkdtemp()
    out = {"reps": reps, "film": [W, H]}
    for spp in (8, 32, 256):
        out[f"spp_{spp}"] = cost_of_the_plane(spp, wd, reps)
    out["cfg4_8spp"] = denoise_and_quality("cfg4", wd, reps, True)
    out["cfg5_8spp"] = denoise_and_quality("cfg5", tempfile.mkdtemp(), reps, False)
    keep(json.dumps(out), "moments_time.json")      # the timings are kept before the profiled child starts
    if "--no-profile" not in sys.argv:
        out["denoise_moments_kernel_split_us"] = kernel_split(reps)
        keep(json.dumps(out), "moments_time.json")


if __name__ == "__main__":
    main()
