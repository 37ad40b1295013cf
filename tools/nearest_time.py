"""rrt_nearest timed: config 4 (100 352 triangles, fixed BVH), default fp32 handle, everything device resident.

  workloads   (a) the points of a 1024 x 1024 atlas (rrt_atlas_sites -> rrt_surface_at over the 224 x 224 grid mesh with vt = the grid), lifted 0.01 of the
                  scene extent off their surfaces along the normal;
              (b) the cell centres of a 128^3 grid over the world bound.
  variants    per workload, alternated in one process, three rounds each: rrt_nearest on the pair-node tree (k_nearest_pairs_f32, option nearest_pairs
              = 1), rrt_nearest on the linear tree (k_nearest<float>, the default), and the yardstick, rrt_trace_closest over as many rays:
              (a) from the lifted points back along -n, (b) from the grid points straight down. The two rrt_nearest variants' outputs are compared bit
              for bit.
  kernels     the kernels' own times, read from the kernel statistics of a trace of `--nearest-only` (stats=<csv or directory>).

Times are device events on the handle's stream around `reps` repetitions (the calls return with their work done). Prints one JSON line;
RRT_RESULTS_DIR=<dir> also keeps it as <dir>/nearest_time.json.
Usage: python tools/nearest_time.py [reps] [stats=path] [--nearest-only]"""
import csv
import glob
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 10
nearest_only = "--nearest-only" in args
stats_path = next((a.split("=", 1)[1] for a in args if a.startswith("stats=")), None)

DEV = "cuda:0"
GRID = 224
ATLAS = 1024
FIELD = 128
LIFT = 0.01
wd = tempfile.mkdtemp()


def event_ms(r, fn, n=None):
    """ms per call: device events on the handle's stream around n calls"""
    n = n or reps
    st = torch.cuda.ExternalStream(r.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    e0.record(st)
    for _ in range(n): fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_stats(path):
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)) if os.path.isdir(path) else [path]
    out = {}
    for p in files:
        with open(p) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in ("k_nearest_pairs_f32", "k_nearest"):
                    if "rrtd::" + k + "<" in name:
                        out.setdefault(k, []).append(dict(name=name, calls=int(row["Calls"]), average_ns=float(row["AverageNs"])))
                        break
    return out


def charted_scene():
    """config 4's mesh with vt = the grid (tools/surface_time.py's)"""
    scenes.write_heightfield(wd, n=GRID)
    lines = open(os.path.join(wd, "heightfield.obj")).read().splitlines()
    g = GRID + 1
    v = [ln for ln in lines if ln.startswith("v ")]
    f = [ln.split()[1:] for ln in lines if ln.startswith("f ")]
    vt = [f"vt {i / GRID:.9f} {j / GRID:.9f}" for i in range(g) for j in range(g)]
    with open(os.path.join(wd, "charted.obj"), "w") as o:
        o.write("\n".join(v + vt + ["f " + " ".join(f"{k}/{k}" for k in tri) for tri in f]) + "\n")
    cfg, root = scenes.cfg4(wd, xres=64, yres=64, nsamp=2, max_depth=8, n=GRID)
    cfg["objs"] = [{"filename": "charted.obj", "obj_name": "hf"}]
    return Scene.loads(cfg, root, flags=RRT_FIXED_BVH)


def workloads(sc, r):
    """{name: (points (m, 3) tensor, ray directions (m, 3) tensor)}"""
    wb = np.ctypeslib.as_array(sc.desc.world_bound).astype(np.float64)
    ext = float(np.linalg.norm(wb[3:] - wb[:3]))
    nt = ATLAS * ATLAS
    t_prim = torch.zeros(nt, dtype=torch.int32, device=DEV)
    t_b1, t_b2 = torch.zeros(nt, dtype=torch.float32, device=DEV), torch.zeros(nt, dtype=torch.float32, device=DEV)
    rec = {k: torch.zeros(nt, dtype=torch.float32, device=DEV) for k in ("px", "py", "pz", "nx", "ny", "nz")}
    torch.cuda.synchronize()
    r.atlas_sites_device((ATLAS, ATLAS), t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr())
    r.surface_at_device(t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr(), nt, {k: t.data_ptr() for k, t in rec.items()})
    torch.cuda.synchronize()
    live = t_prim >= 0
    p = torch.stack([rec[k] for k in ("px", "py", "pz")], 1)[live]
    n = torch.stack([rec[k] for k in ("nx", "ny", "nz")], 1)[live]
    atlas = ((p + (LIFT * ext) * n).contiguous(), (-n).contiguous())
    ax = [wb[k] + (np.arange(FIELD) + 0.5) * ((wb[3 + k] - wb[k]) / FIELD) for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    g = torch.from_numpy(np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)).to(DEV)
    down = torch.zeros_like(g); down[:, 1] = -1.0
    return {"atlas_1024": atlas, "grid_128": (g, down)}, ext


def main():
    sc = charted_scene()
    r = Renderer(sc, 0, RRT_F32)
    loads, ext = workloads(sc, r)
    res = {}
    for name, (p, d) in loads.items():
        m = len(p)
        cols = [p[:, k].contiguous() for k in range(3)]
        dcols = [d[:, k].contiguous() for k in range(3)]
        tmax = torch.full((m,), float("inf"), dtype=torch.float32, device=DEV)
        outs = {v: {k: torch.zeros(m, dtype=torch.int32 if k == "prim" else torch.float32, device=DEV) for k in ("prim", "b1", "b2", "dist")} for v in ("pairs", "linear")}
        hit = {k: torch.zeros(m, dtype=torch.int32 if k == "prim" else torch.float32, device=DEV) for k in ("t", "prim", "u", "v")}
        torch.cuda.synchronize()
        ptrs7 = [t.data_ptr() for t in cols + dcols + [tmax]]

        def nearest(variant):
            r.set_option("nearest_pairs", 1 if variant == "pairs" else 0)
            r.nearest_device(dict(px=cols[0].data_ptr(), py=cols[1].data_ptr(), pz=cols[2].data_ptr(), **{k: t.data_ptr() for k, t in outs[variant].items()}), m)

        trace = lambda: r.trace_closest_device(ptrs7, m, hit["t"].data_ptr(), hit["prim"].data_ptr(), hit["u"].data_ptr(), hit["v"].data_ptr())
        if nearest_only:
            for _ in range(2 + reps): nearest("pairs")
            for _ in range(2 + reps): nearest("linear")
            torch.cuda.synchronize()
            continue
        for _ in range(2): nearest("pairs"); nearest("linear"); trace()      # warm-up
        rounds = {"nearest_pairs": [], "nearest_linear": [], "trace_closest": []}
        for _ in range(3):
            rounds["nearest_pairs"].append(event_ms(r, lambda: nearest("pairs")))
            rounds["nearest_linear"].append(event_ms(r, lambda: nearest("linear")))
            rounds["trace_closest"].append(event_ms(r, trace))
        torch.cuda.synchronize()
        same = all(bool(torch.equal(outs["pairs"][k].view(torch.int32), outs["linear"][k].view(torch.int32))) for k in ("prim", "b1", "b2", "dist"))
        dist = outs["pairs"]["dist"]
        res[name] = {"points": m, "ms": {k: dict(median=float(np.median(v)), rounds=v) for k, v in rounds.items()}, "pairs_and_linear_same_bits": same,
                     "found": int((outs["pairs"]["prim"] >= 0).sum()), "rays_that_hit": int((hit["prim"] >= 0).sum()),
                     "dist_over_extent": {"median": float(dist.median()) / ext, "max": float(dist.max()) / ext}}
        med = {k: res[name]["ms"][k]["median"] for k in rounds}
        res[name]["ns_per_query"] = {k: v * 1e6 / m for k, v in med.items()}
        res[name]["nearest_linear_over_trace_closest"] = med["nearest_linear"] / med["trace_closest"]
        res[name]["nearest_pairs_over_linear"] = med["nearest_pairs"] / med["nearest_linear"]
    r.close()
    return res


out = main()
if nearest_only:
    sys.exit(0)
out = {"what": "config 4 (100 352 triangles, fixed BVH), fp32, one MI355X, device arrays, device events on the handle's stream, ms per call", "reps": reps, **out}
if stats_path:
    out["kernel_average_ns"] = kernel_stats(stats_path)
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "nearest_time.json"), "w") as f:
        f.write(line + "\n")
