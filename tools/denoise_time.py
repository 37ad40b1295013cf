"""rrt_denoise timed beside the frame and the feature-buffer pass: config 4 at 1024^2 (100 352 triangles, depth 8, fixed BVH), default fp32 handle,
device buffers; frames of 8, 32 and 256 samples per pixel (one scene each), rrt_render_aov with max_samples min(spp, 32) as the command line runs it,
rrt_denoise with default parameters. Each after a warm-up, REPS repetitions on a synchronised host clock (every call returns with the stream
drained). Also: RGB RMSE of the noisy and the denoised 8 and 32 spp frames against the 256 spp frame, and the samples per pixel whose noisy RMSE
the denoised 8 spp frame matches (1 / sqrt(spp) law through the two noisy points) with the frame time interpolated there.

The per-kernel split comes from a run of its own: this script starts `rocprofv3 --kernel-trace --stats` (no counters) over a child process of
itself that denoises the 8 spp frame with six iterations (steps 1 .. 32) under dn_lds 0 (direct gathers at every step) and dn_lds 1 (the LDS
tiles), and reads the kernels' average and minimum times from the stats table: the kernel names carry the form and the step. --no-profile skips it.

Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/denoise_time.json.
Usage: python tools/denoise_time.py [reps] [--no-profile]"""
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
RGB_FROM_XYZ = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])


def make(spp, wd):
    cfg, root = scenes.cfg4(wd, xres=W, yres=H, nsamp=spp + 1, max_depth=8)
    return Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)


def buffers():
    return [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(5)]     # film, albedo, normal, depth, out


def render_into(r, bufs, spp):
    for b in bufs: b.zero_()
    torch.cuda.synchronize()
    r.render_device((0, 0, W, H), bufs[0].data_ptr(), stats=False)
    aov(r, bufs, spp)


def aov(r, bufs, spp):
    import ctypes as C
    from rs_ray_toy_amd import _abi as A
    d = A.Aov(A.RRT_MEM_DEVICE, RRT_F32, *[b.data_ptr() for b in bufs[1:4]])
    rect = (C.c_int32 * 4)(0, 0, W, H)
    rc = A.lib().rrt_render_aov(r._h, rect, 0, 1, min(spp, 32), C.byref(d))
    assert rc == A.RRT_OK, A.lib().rrt_last_error()


def denoise(r, bufs, **params):
    r.denoise_device(bufs[0].data_ptr(), [b.data_ptr() for b in bufs[1:4]], bufs[4].data_ptr(), **params)


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


def child(reps):
    """the profiled process: the 8 spp frame, six iterations, direct gathers against the LDS tiles"""
    r = make(8, tempfile.mkdtemp())
    bufs = buffers()
    render_into(r, bufs, 8)
    for mode in (0, 1):
        r.set_option("dn_lds", mode)
        for _ in range(reps + 2):
            denoise(r, bufs, iterations=6)
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
        m = re.search(r"(k_dn_\w+)<float(?:, (\d+))?>", row["Name"])
        if not m: continue
        name = m.group(1) + (f"_s{m.group(2)}" if m.group(2) else "")
        split[name] = dict(calls=int(row["Calls"]), avg_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3)
    return split


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 10
    if "--child" in sys.argv:
        return child(reps)
    wd = tempfile.mkdtemp()
    out = {"reps": reps, "film": [W, H]}
    frames = {}
    for spp in (8, 32, 256):
        r = make(spp, wd)
        bufs = buffers()
        for _ in range(2):      # warm-up: the first frame builds the tile trees and sizes the pools, the first denoise allocates the records
            render_into(r, bufs, spp)
            denoise(r, bufs)
        res = {"frame_ms": timed(lambda: r.render_device((0, 0, W, H), bufs[0].data_ptr(), stats=False), reps),
               "aov_ms": timed(lambda: aov(r, bufs, spp), reps)}
        render_into(r, bufs, spp)      # one frame's sums again (the timed calls added to them)
        for mode, key in ((1, "denoise_ms"), (0, "denoise_ms_dn_lds_0")):
            r.set_option("dn_lds", mode)
            denoise(r, bufs)
            res[key] = timed(lambda: denoise(r, bufs), reps)
        r.set_option("dn_lds", 1)
        denoise(r, bufs)
        frames[spp] = (rgb(bufs[0]), rgb(bufs[4]))
        out[f"spp_{spp}"] = res
        r.close()
    clean = frames[256][0]
    rmse = lambda a: float(np.sqrt(((a - clean) ** 2).mean()))
    q = {"noisy_8": rmse(frames[8][0]), "denoised_8": rmse(frames[8][1]), "noisy_32": rmse(frames[32][0]), "denoised_32": rmse(frames[32][1])}
    out["rgb_rmse_against_256spp"] = q
    # noisy RMSE ~ a / spp^b through the 8 and 32 spp points; the spp at which it equals the denoised 8 spp frame's
    b = np.log(q["noisy_8"] / q["noisy_32"]) / np.log(4.0)
    spp_eq = float(8.0 * (q["noisy_8"] / q["denoised_8"]) ** (1.0 / b))
    f8, f32, f256 = (out[f"spp_{k}"]["frame_ms"]["median"] for k in (8, 32, 256))
    lo, hi = ((8, f8), (32, f32)) if spp_eq <= 32 else ((32, f32), (256, f256))
    out["denoised_8_matches_noisy_spp"] = spp_eq
    out["denoised_32_matches_noisy_spp"] = float(32.0 * (q["noisy_32"] / q["denoised_32"]) ** (1.0 / b))
    out["noise_exponent"] = float(b)
    out["frame_ms_at_that_spp_interpolated"] = float(lo[1] + (hi[1] - lo[1]) * (spp_eq - lo[0]) / (hi[0] - lo[0]))
    s8 = out["spp_8"]
    out["denoise_share_of_8spp_frame_plus_aov"] = s8["denoise_ms"]["median"] / (s8["frame_ms"]["median"] + s8["aov_ms"]["median"])
    if "--no-profile" not in sys.argv:
        out["kernel_split_us_8spp_6_iterations"] = kernel_split(reps)
        # algorithmic bytes of an a-trous launch: 25 taps x 32 B read + 32 B written per pixel (cache-served: the three record planes are 48 MB)
        out["atrous_algorithmic_bytes_per_launch"] = W * H * (25 * 32 + 32)
    line = json.dumps(out)
    print(line)
    if os.environ.get("RRT_RESULTS_DIR"):
        os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "denoise_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
