"""rrt_irradiance timed beside the route a caller had before it: config 4 (100 352 triangles, Path depth 8, fixed BVH) on a 256 x 256 film with nsamp raised
to 65, default fp32 handle. The points are the first hits of the camera rays of samples 1 .. 3 of every pixel (the live ones that hit), with their
geometric normals turned towards the camera; 64 cosine draws per point; every array in device memory.

  irradiance       rrt_irradiance: rays made on the device, sums reduced there
  torch_route      the same draws built in torch on the device from the same u (dims5[0:2] of the pixel's samples, uploaded once), rrt_radiance over them
                   (radiance_device), a torch reduction to the same four sums per point
  radiance_only    radiance_device alone over the same ray count (the rays of the last torch_route call)

After a warm-up, REPS alternating rounds on a host clock around synchronised calls; medians. The sums of the two routes are compared point by point
(torch's sin, cos and divisions are not the device's: most points agree to fp32 rounding, a few differ by a draw that landed elsewhere; the bit-for-bit
statement is tests/test_irradiance.py's, over rrt_irradiance_rays' own rays).
parent_lib=<librrt.so of the parent commit>: torch_route and radiance_only are also timed on that build, in a child process of its own (RRT_LIBRARY).
--irradiance-only: nothing but warm-up and a few rrt_irradiance calls, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/irradiance_time.py 3 --irradiance-only).
Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/irradiance_time.json.
Usage: python tools/irradiance_time.py [reps] [parent_lib=path] [--irradiance-only]"""
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes
from rs_ray_toy_amd import _abi as A

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 20
route_only = "--route-only" in args
irr_only = "--irradiance-only" in args
parent_lib = next((a.split("=", 1)[1] for a in args if a.startswith("parent_lib=")), None)
if route_only:      # the parent's build has fewer entry points than this tree's ctypes table: bind what it exports
    import ctypes
    older = ctypes.CDLL(A.LIB_PATH)
    for name in [k for k in A.PROTOTYPES if not hasattr(older, k)]:
        del A.PROTOTYPES[name]
import oracle_lib as O

W = H = 256
NSAMP, GRID_SAMPLES = 65, 3
ND = NSAMP - 1
DEV = "cuda:0"
cfg, root = scenes.cfg4(tempfile.mkdtemp(), xres=W, yres=H, nsamp=NSAMP, max_depth=8)
sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
r = Renderer(sc, 0, RRT_F32)

# the points: first hits of the grid's camera rays (the f64 oracle's traversal gives the geometric normal with the hit)
dims, rays, w = r.camera_samples((0, 0, W, H), 1, 1 + GRID_SAMPLES)
alive = np.flatnonzero(w > 0)
hit = O.trace_closest(sc, rays[alive, :3], rays[alive, 3:], np.full(len(alive), np.inf), want_geometry=True)
ok = np.flatnonzero(hit["prim"] >= 0)
sel = alive[ok]
nrm = hit["n"][ok] / np.linalg.norm(hit["n"][ok], axis=1, keepdims=True)
nrm = np.where((np.sum(nrm * rays[sel, 3:], 1) > 0)[:, None], -nrm, nrm)
pix = sel // GRID_SAMPLES                                      # [pixel][sample] layout: the pixel of each point
n_pts = len(sel)
OFFSET = 1e-3


def dev(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to(DEV)


P = [dev(hit["p"][ok][:, k]) for k in range(3)]
N = [dev(nrm[:, k]) for k in range(3)]
pixel_word = (((pix // W).astype(np.uint32) << 16) | (pix % W).astype(np.uint32)).astype(np.uint32)
PIXEL = dev(pixel_word, np.uint32)
sums = torch.zeros((n_pts, 4), dtype=torch.float32, device=DEV)
torch.cuda.synchronize()


def irradiance():
    sums.zero_()
    r.irradiance_device([t.data_ptr() for t in P], [t.data_ptr() for t in N], n_pts, 1, NSAMP, sums.data_ptr(), pixel_ptr=PIXEL.data_ptr(), offset=OFFSET)


def timed(fns):
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}


if irr_only:
    for _ in range(2 + reps):
        irradiance()
    torch.cuda.synchronize()
    r.close()
    sys.exit(0)

# today's route: u of every draw of every pixel once (host, then device), the rays in torch, rrt_radiance, a torch reduction
u_all = np.concatenate([r.camera_samples((0, y0, W, y0 + 64), 1, NSAMP)[0][:, :2] for y0 in range(0, H, 64)]).reshape(W * H, ND, 2)
U = dev(u_all[pix])                                                                  # (n, ND, 2)
PIX_RAYS = PIXEL.repeat_interleave(ND).contiguous()
SNUM = torch.arange(1, NSAMP, dtype=torch.int32, device=DEV).repeat(n_pts).contiguous()
rgb4 = torch.zeros((n_pts * ND, 4), dtype=torch.float32, device=DEV)
Pt, Nt = torch.stack(P, 1), torch.stack(N, 1)
YW = torch.tensor([0.212671, 0.715160, 0.072169], dtype=torch.float32, device=DEV)
last_rays = []


def build_rays():
    nn = Nt / Nt.norm(dim=1, keepdim=True)
    x, y, z = nn[:, 0], nn[:, 1], nn[:, 2]
    zero = torch.zeros_like(x)
    a = torch.stack([-z, zero, x], 1) / torch.sqrt(x * x + z * z)[:, None]
    b = torch.stack([zero, z, -y], 1) / torch.sqrt(y * y + z * z)[:, None]
    s = torch.where((x.abs() > y.abs())[:, None], a, b)
    t = torch.linalg.cross(nn, s)
    ox, oy = 2.0 * U[..., 0] - 1.0, 2.0 * U[..., 1] - 1.0
    first = ox.abs() > oy.abs()
    rr = torch.where(first, ox, oy)
    theta = torch.where(first, (math.pi / 4) * (oy / ox), math.pi / 2 - (math.pi / 4) * (ox / oy))
    centre = (ox == 0) & (oy == 0)
    dx = torch.where(centre, zero[:, None], rr * torch.cos(theta))
    dy = torch.where(centre, zero[:, None], rr * torch.sin(theta))
    dz = torch.sqrt(torch.clamp(1.0 - dx * dx - dy * dy, min=0.0))
    d = s[:, None, :] * dx[..., None] + t[:, None, :] * dy[..., None] + nn[:, None, :] * dz[..., None]
    d = d / d.norm(dim=-1, keepdim=True)
    o = (Pt + nn * OFFSET)[:, None, :].expand(-1, ND, -1)
    return [o[..., k].reshape(-1).contiguous() for k in range(3)] + [d[..., k].reshape(-1).contiguous() for k in range(3)], (dz != 0).reshape(-1).to(torch.float32)


def radiance_only():
    soa, wgt = last_rays
    r.radiance_device([t.data_ptr() for t in soa], PIX_RAYS.data_ptr(), SNUM.data_ptr(), n_pts * ND, rgb4.data_ptr(), weight_ptr=wgt.data_ptr())


def torch_route():
    global last_rays
    last_rays = build_rays()
    radiance_only()
    L = rgb4.view(n_pts, ND, 4)[..., :3]
    y = L @ YW
    return torch.cat([L.sum(1), (y * y).sum(1, keepdim=True)], 1)


for _ in range(2):      # warm-up: pools, code objects, torch's kernels
    route_sums = torch_route()
    radiance_only()
    if not route_only:
        irradiance()
torch.cuda.synchronize()
if route_only:
    print(json.dumps(timed({"torch_route": torch_route, "radiance_only": radiance_only})))
    r.close()
    sys.exit(0)

# the two routes point by point: torch's sin / cos / division are not the device's, so a ray can land on another triangle and a draw change its value -
# most points agree to fp32 rounding, a few differ by a draw
is_lit = (sums[:, :3] > 0).any(1)
lit = int(is_lit.sum())
per_point = ((sums[:, :3] - route_sums[:, :3]).abs().max(1).values / route_sums[:, :3].abs().max(1).values.clamp(min=1e-30))[is_lit]
agree = dict(median=float(per_point.median()), share_within_1e_4=float((per_point < 1e-4).float().mean()), share_within_1e_2=float((per_point < 1e-2).float().mean()),
             mean_E_ratio=float(sums[:, :3].sum() / route_sums[:, :3].sum()))
t = timed({"irradiance": irradiance, "torch_route": torch_route, "radiance_only": radiance_only})
out = {"what": "config 4 (100 352 triangles, Path depth 8), 256 x 256 film, fp32, one MI355X: irradiance sums of 64 cosine draws at the first hits of the camera rays "
               "of samples 1..3, device arrays; rrt_irradiance against rays built in torch + rrt_radiance + a torch reduction, and rrt_radiance alone; alternating "
               "rounds, host clock around synchronised calls, ms",
       "reps": reps, "points": n_pts, "draws": ND, "rays": n_pts * ND, "points_lit": lit, "per_point_difference_of_the_routes_over_the_points_largest_sum": agree,
       "irradiance_ms": t["irradiance"], "torch_route_ms": t["torch_route"], "radiance_only_ms": t["radiance_only"],
       "ratio_irradiance_over_torch_route": t["irradiance"]["median"] / t["torch_route"]["median"],
       "ratio_irradiance_over_radiance_only": t["irradiance"]["median"] / t["radiance_only"]["median"]}
r.close()
if parent_lib:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--route-only"], env=dict(os.environ, RRT_LIBRARY=os.path.abspath(parent_lib)),
                           capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stderr[-2000:]
    parent = json.loads(child.stdout.strip().splitlines()[-1])
    out.update(parent_torch_route_ms=parent["torch_route"], parent_radiance_only_ms=parent["radiance_only"])
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "irradiance_time.json"), "w") as f:
        f.write(line + "\n")
