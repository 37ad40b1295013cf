"""rrt_render_rays timed beside the frame: config 4 at 1024^2 (100 352 triangles, 32 spp, depth 8, fixed BVH), default fp32 handle, device film.
The handle's own camera samples (rrt_camera_samples, fetched in strips of rows and uploaded once as fp32 SoA arrays) go back in through
rrt_render_rays from device memory; rrt_render_rect renders the same frame. Both after a warm-up, REPS alternating rounds on a synchronised host
clock (both calls return with the stream drained), and the kernel-category split of one call each from rrt_render_stats.
parent_lib=<librrt.so of the parent commit>: the frame is also timed on that build, in a child process of its own (RRT_LIBRARY), the same way.
Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/render_rays_time.json.
Usage: python tools/render_rays_time.py [reps] [parent_lib=path] [key=value ...] (handle options)."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 10
frame_only = "--frame-only" in args
args = [a for a in args if a != "--frame-only"]
parent_lib = next((a.split("=", 1)[1] for a in args if a.startswith("parent_lib=")), None)
args = [a for a in args if not a.startswith("parent_lib=")]
if frame_only:      # the parent's build has fewer entry points than this tree's ctypes table: bind what it exports
    import ctypes
    from rs_ray_toy_amd import _abi as A
    older = ctypes.CDLL(A.LIB_PATH)
    for name in [k for k in A.PROTOTYPES if not hasattr(older, k)]:
        del A.PROTOTYPES[name]
W = H = 1024
NSAMP, STRIP = 33, 128
cfg, root = scenes.cfg4(tempfile.mkdtemp(), xres=W, yres=H, nsamp=NSAMP, max_depth=8)
r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
for k, v in (a.split("=") for a in args):
    r.set_option(k, float(v))
film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
RECT = (0, 0, W, H)


def frame():
    return r.render_device(RECT, film.data_ptr(), stats=True)


def timed(fns):
    """the calls in turn, reps rounds: {name: ms statistics}"""
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}


def split(st):
    return dict(total=st.ms_total, camera_or_ingest=st.ms_raygen, closest=st.ms_closest, any=st.ms_any, shade=st.ms_shade, film=st.ms_film,
                camera_rays=int(st.camera_rays), closest_queries=int(st.closest_queries), tile_launches=int(st.tile_launches), root_culled=int(st.root_culled))


for _ in range(2):      # warm-up: the first frame builds the tile trees and sizes the pools
    st_frame = frame()
if frame_only:
    print(json.dumps({"frame_ms": timed({"frame": frame})["frame"], "frame_split_ms": split(st_frame)}))
    r.close()
    sys.exit(0)

# the handle's own samples of sample numbers 1 .. 32, [pixel][sample] over the whole film = the strips' layouts one after the other
cols = [[] for _ in range(9)]      # ox oy oz dx dy dz weight pfx pfy
for y0 in range(0, H, STRIP):
    dims, rays, w = r.camera_samples((0, y0, W, y0 + STRIP), 1, NSAMP)
    ys, xs = np.mgrid[y0:y0 + STRIP, 0:W]
    px = np.repeat(xs.ravel(), NSAMP - 1).astype(np.float32) + dims[:, 0].astype(np.float32)
    py = np.repeat(ys.ravel(), NSAMP - 1).astype(np.float32) + dims[:, 1].astype(np.float32)
    for c, a in zip(cols, [rays[:, k] for k in range(6)] + [w, px, py]):
        c.append(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0"))
    del dims, rays, w
soa = [torch.cat(c) for c in cols[:7]]
p_film = torch.stack([torch.cat(cols[7]), torch.cat(cols[8])], 1).contiguous()
del cols
torch.cuda.synchronize()
film_rays = torch.zeros_like(film)


def rays_call(dst=film):
    return r.render_rays_device(RECT, 1, NSAMP, [t.data_ptr() for t in soa[:6]], soa[6].data_ptr(), p_film.data_ptr(), dst.data_ptr(), stats=True)


film.zero_(); frame(); ref = film.clone()
rays_call(film_rays)
same = bool(torch.equal(ref, film_rays))
for _ in range(2):
    st_rays = rays_call()
    st_frame = frame()
out = {"what": "config 4, 1024^2, 32 spp, depth 8, fp32, device buffers, one MI355X: rrt_render_rays fed the handle's own camera samples against rrt_render_rect, "
               "alternating rounds, host clock around synchronised calls, ms", "reps": reps, "bit_identical_films": same}
t = timed({"frame": frame, "render_rays": rays_call})
out.update(frame_ms=t["frame"], render_rays_ms=t["render_rays"], ratio_render_rays_over_frame=t["render_rays"]["median"] / t["frame"]["median"],
           frame_split_ms=split(st_frame), render_rays_split_ms=split(st_rays))
r.close()
if parent_lib:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--frame-only"] + args, env=dict(os.environ, RRT_LIBRARY=os.path.abspath(parent_lib)),
                           capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stderr[-2000:]
    parent = json.loads(child.stdout.strip().splitlines()[-1])
    out.update(parent_frame_ms=parent["frame_ms"], parent_frame_split_ms=parent["frame_split_ms"],
               ratio_render_rays_over_parent_frame=t["render_rays"]["median"] / parent["frame_ms"]["median"])
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "render_rays_time.json"), "w") as f:
        f.write(line + "\n")
