"""rrt_surface_rays, rrt_surface_at and rrt_atlas_sites timed: config 4 (100 352 triangles, fixed BVH), default fp32 handle, everything device resident.

  record cost   rrt_surface_rays with all groups and with p, n only against rrt_trace_closest over the live camera rays of sample 1 of a 1024 x 1024
                film; the difference is the record cost
  kernel        k_surface's own time, read from the kernel statistics of a trace of `--surface-only` (stats=<csv or directory>), beside the bytes it must
                move: 48 in (ray origin, ray direction, hit record) + the 48-byte triangle record of a hit + 4 per produced element out, against the
                6.3 TB/s a streaming kernel reaches on this part
  the gate      parent_tree=<a built checkout of the parent commit>: rrt_trace_closest over those rays (this tool, RRT_LIBRARY = the parent's librrt.so)
                and `python bench.py` (the parent's own, in its tree) on this build and on the parent's, alternated in child processes, with the
                run-to-run spread of each
  the chain     atlas_sites(1024 x 1024) over the 224 x 224 grid mesh with a uv chart (vt = the grid) -> surface_at -> irradiance with 16 draws, each
                stage timed, against the first two stages done in numpy from the description (a rasteriser over each triangle's bounding box, then
                points and normals from the vertices), which is what a caller writes today

Times are device events on the handle's stream around `reps` repetitions (the calls return with their work done). Prints one JSON line;
RRT_RESULTS_DIR=<dir> also keeps it as <dir>/surface_time.json.
Usage: python tools/surface_time.py [reps] [parent_tree=path] [stats=path] [--surface-only | --chain-only | --trace-only]"""
import csv
import glob
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
from rs_ray_toy_amd import _abi as A

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 20
mode = next((a for a in args if a in ("--surface-only", "--chain-only", "--trace-only")), None)
parent_tree = next((a.split("=", 1)[1] for a in args if a.startswith("parent_tree=")), None)
stats_path = next((a.split("=", 1)[1] for a in args if a.startswith("stats=")), None)
if mode == "--trace-only":      # the parent's build has fewer entry points than this tree's ctypes table: bind what it exports
    import ctypes
    older = ctypes.CDLL(A.LIB_PATH)
    for name in [k for k in A.PROTOTYPES if not hasattr(older, k)]:
        del A.PROTOTYPES[name]

DEV = "cuda:0"
W = H = 1024
GRID = 224
ATLAS = 1024
DRAWS = 16
STREAM_TBS = 6.3
wd = tempfile.mkdtemp()


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


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
    """{short kernel name: [(full name, calls, average ns)]} from a *kernel_stats.csv, or from every one below a directory"""
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)) if os.path.isdir(path) else [path]
    out = {}
    for p in files:
        with open(p) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in ("k_surface", "k_atlas_owner", "k_atlas_emit", "k_sites_check"):
                    if "rrtd::" + k + "<" in name:
                        out.setdefault(k, []).append((name, int(row["Calls"]), float(row["AverageNs"])))
    return out


# ---- the rays: live camera rays of sample 1 -------------------------------------------------------------------------------------------------------------
def camera_rays():
    cfg, root = scenes.cfg4(wd, xres=W, yres=H, nsamp=2, max_depth=8, n=GRID)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    parts = [r.camera_samples((0, y0, W, y0 + 64), 1, 2) for y0 in range(0, H, 64)]
    rays = np.concatenate([p[1] for p in parts]); w = np.concatenate([p[2] for p in parts])
    live = w > 0
    cols = [dev(rays[live, k]) for k in range(6)] + [torch.full((int(live.sum()),), float("inf"), dtype=torch.float32, device=DEV)]
    return sc, r, cols, int(live.sum())


def record_cost():
    sc, r, cols, m = camera_rays()
    ptrs7 = [t.data_ptr() for t in cols]
    t_out = torch.zeros(m, dtype=torch.float32, device=DEV); prim_out = torch.zeros(m, dtype=torch.int32, device=DEV)
    u_out, v_out = torch.zeros(m, dtype=torch.float32, device=DEV), torch.zeros(m, dtype=torch.float32, device=DEV)
    members = [k for g in A.SURFACE_GROUPS.values() for k in g] if hasattr(A, "SURFACE_GROUPS") else []
    outs = {k: torch.zeros(m, dtype=torch.int32 if k in ("prim", "material") else torch.float32, device=DEV) for k in members}
    torch.cuda.synchronize()
    trace = lambda: r.trace_closest_device(ptrs7, m, t_out.data_ptr(), prim_out.data_ptr(), u_out.data_ptr(), v_out.data_ptr())
    if mode == "--trace-only":
        ms = [event_ms(r, trace) for _ in range(3)]
        print(json.dumps({"trace_closest_ms": ms}))
        r.close()
        return None
    all_ptrs = {k: t.data_ptr() for k, t in outs.items()}
    pn_ptrs = {k: outs[k].data_ptr() for k in ("px", "py", "pz", "nx", "ny", "nz")}
    surf_all = lambda: r.surface_device(ptrs7, m, all_ptrs)
    surf_pn = lambda: r.surface_device(ptrs7, m, pn_ptrs)
    if mode == "--surface-only":
        for _ in range(2 + reps): surf_all()
        for _ in range(2 + reps): surf_pn()
        torch.cuda.synchronize(); r.close()
        return None
    res = {"rays": m, "hits": 0}
    for _ in range(2): trace(); surf_all(); surf_pn()
    rounds = {"trace_closest": [], "surface_all": [], "surface_p_n": []}
    for _ in range(3):
        rounds["trace_closest"].append(event_ms(r, trace)); rounds["surface_all"].append(event_ms(r, surf_all)); rounds["surface_p_n"].append(event_ms(r, surf_pn))
    res["hits"] = int((outs["prim"] >= 0).sum())
    res["ms"] = {k: dict(median=float(np.median(v)), rounds=v) for k, v in rounds.items()}
    res["record_cost_ms"] = {"all_groups": res["ms"]["surface_all"]["median"] - res["ms"]["trace_closest"]["median"],
                             "p_n": res["ms"]["surface_p_n"]["median"] - res["ms"]["trace_closest"]["median"]}
    # the bytes k_surface must move: per record 48 in, per hit the 48-byte triangle record, 4 per produced element out (17 arrays / 6 arrays)
    hits = res["hits"]
    res["bytes_model"] = {"all_groups": 48 * m + 48 * hits + 4 * 17 * m, "p_n": 48 * m + 48 * hits + 4 * 6 * m}
    res["streaming_floor_us_at_6.3_TB_s"] = {k: v / (STREAM_TBS * 1e12) * 1e6 for k, v in res["bytes_model"].items()}
    r.close()
    return res


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------------
def charted_scene():
    """config 4's mesh with vt = the grid: the heightfield's own vertices and faces, a uv chart added"""
    scenes.write_heightfield(wd, n=GRID)
    lines = open(os.path.join(wd, "heightfield.obj")).read().splitlines()
    g = GRID + 1
    v = [ln for ln in lines if ln.startswith("v ")]
    f = [ln.split()[1:] for ln in lines if ln.startswith("f ")]
    vt = [f"vt {i / GRID:.9f} {j / GRID:.9f}" for i in range(g) for j in range(g)]
    with open(os.path.join(wd, "charted.obj"), "w") as o:
        o.write("\n".join(v + vt + ["f " + " ".join(f"{k}/{k}" for k in tri) for tri in f]) + "\n")
    cfg, root = scenes.cfg4(wd, xres=256, yres=256, nsamp=DRAWS + 1, max_depth=8, n=GRID)
    cfg["objs"] = [{"filename": "charted.obj", "obj_name": "hf"}]
    return Scene.loads(cfg, root, flags=RRT_FIXED_BVH)


def numpy_route(sc):
    """What a caller writes today: the owner and barycentrics per texel by a rasteriser over each triangle's bounding box, then points and normals from
    the description's vertices (one mesh, no instance)"""
    d = sc.desc
    n = int(d.n_prim_order)
    t0 = time.perf_counter()
    order = np.ctypeslib.as_array(d.prim_order, shape=(n,))
    prims = np.frombuffer((A.Prim * int(d.n_prims)).from_address(__import__("ctypes").addressof(d.prims.contents)), dtype=np.dtype(A.Prim))
    tris = np.frombuffer((A.Tri * int(d.n_tris)).from_address(__import__("ctypes").addressof(d.tris.contents)), dtype=np.dtype(A.Tri))
    pos = np.ctypeslib.as_array(d.positions, shape=(int(d.n_positions) * 3,)).reshape(-1, 3)
    uvs = np.ctypeslib.as_array(d.uvs, shape=(int(d.n_uvs) * 2,)).reshape(-1, 2)
    tr = tris[prims["shape"][order]]
    UV = uvs[tr["uv"]]; P = pos[tr["v"]]
    owner = np.full((ATLAS, ATLAS), -1, np.int32); b1 = np.zeros((ATLAS, ATLAS)); b2 = np.zeros((ATLAS, ATLAS))
    for k in range(n):
        a, b, c3 = UV[k]
        x0, x1 = max(0, int(np.floor(min(a[0], b[0], c3[0]) * ATLAS)) - 1), min(ATLAS, int(np.ceil(max(a[0], b[0], c3[0]) * ATLAS)) + 1)
        y0, y1 = max(0, int(np.floor(min(a[1], b[1], c3[1]) * ATLAS)) - 1), min(ATLAS, int(np.ceil(max(a[1], b[1], c3[1]) * ATLAS)) + 1)
        if x1 <= x0 or y1 <= y0: continue
        cx, cy = np.meshgrid((np.arange(x0, x1) + 0.5) / ATLAS, (np.arange(y0, y1) + 0.5) / ATLAS)
        bax, bay, cax, cay = b[0] - a[0], b[1] - a[1], c3[0] - a[0], c3[1] - a[1]
        area = bax * cay - bay * cax
        if area == 0: continue
        px, py = cx - a[0], cy - a[1]
        e1 = (px * cay - py * cax) / area; e2 = (bax * py - bay * px) / area
        take = (e1 >= 0) & (e2 >= 0) & (e1 + e2 <= 1) & (owner[y0:y1, x0:x1] < 0)
        owner[y0:y1, x0:x1][take] = k; b1[y0:y1, x0:x1][take] = e1[take]; b2[y0:y1, x0:x1][take] = e2[take]
    t1 = time.perf_counter()
    q = np.maximum(owner.ravel(), 0)
    p = P[q, 0] + ((P[q, 1] - P[q, 0]) * b1.ravel()[:, None] + (P[q, 2] - P[q, 0]) * b2.ravel()[:, None])
    nrm = np.cross(P[q, 0] - P[q, 2], P[q, 1] - P[q, 2])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dead = owner.ravel() < 0
    p[dead] = 0; nrm[dead] = 0
    t2 = time.perf_counter()
    return dict(owner=owner, b1=b1, b2=b2, p=p, n=nrm, atlas_s=t1 - t0, records_s=t2 - t1)


def chain():
    sc = charted_scene()
    r = Renderer(sc, 0, RRT_F32)
    nt = ATLAS * ATLAS
    t_prim = torch.zeros(nt, dtype=torch.int32, device=DEV)
    t_b1, t_b2 = torch.zeros(nt, dtype=torch.float32, device=DEV), torch.zeros(nt, dtype=torch.float32, device=DEV)
    rec = {k: torch.zeros(nt, dtype=torch.float32, device=DEV) for k in ("px", "py", "pz", "nx", "ny", "nz")}
    sums = torch.zeros((nt, 4), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    covered = [0]

    def atlas(): covered[0] = r.atlas_sites_device((ATLAS, ATLAS), t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr())
    def records(): r.surface_at_device(t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr(), nt, {k: t.data_ptr() for k, t in rec.items()})
    def irradiance(): r.irradiance_device([rec[k].data_ptr() for k in ("px", "py", "pz")], [rec[k].data_ptr() for k in ("nx", "ny", "nz")], nt, 1, DRAWS + 1, sums.data_ptr(), offset=1e-3)

    if mode == "--chain-only":
        for _ in range(2 + reps): atlas(); records()
        torch.cuda.synchronize(); r.close()
        return None
    atlas(); records(); irradiance()
    res = {"texels": nt, "triangles": int(sc.desc.n_prim_order), "draws": DRAWS,
           "ms": {"atlas_sites": event_ms(r, atlas), "surface_at": event_ms(r, records), "irradiance": event_ms(r, irradiance, max(2, reps // 4))}}
    res["covered"] = covered[0]
    ref = numpy_route(sc)
    res["numpy_route_s"] = {"atlas": ref["atlas_s"], "records": ref["records_s"]}
    got_owner = t_prim.cpu().numpy().reshape(ATLAS, ATLAS)
    res["owner_differs_from_numpy_on_texels"] = int((got_owner != ref["owner"]).sum())
    same = (got_owner == ref["owner"]).ravel() & (ref["owner"].ravel() >= 0)
    res["largest_p_difference_from_numpy"] = float(np.abs(np.stack([rec[k].cpu().numpy() for k in ("px", "py", "pz")], 1)[same] - ref["p"][same]).max())
    r.close()
    return res


if mode in ("--surface-only", "--trace-only"):
    record_cost()
    sys.exit(0)
if mode == "--chain-only":
    chain()
    sys.exit(0)

out = {"what": "config 4 (100 352 triangles, fixed BVH), fp32, one MI355X, device arrays, device events on the handle's stream, ms per call",
       "reps": reps, "record_cost": record_cost(), "chain": chain()}
if stats_path:
    ks = kernel_stats(stats_path)
    out["kernel_average_ns"] = {k: [dict(name=n, calls=c, average_ns=a) for n, c, a in v] for k, v in ks.items()}
if parent_tree:
    me = os.path.abspath(__file__)
    parent_tree = os.path.abspath(parent_tree)
    parent_lib = os.path.join(parent_tree, "rs_ray_toy_amd", "csrc", "librrt.so")
    trees = {"branch": ROOT, "parent": parent_tree}
    envs = {"branch": dict(os.environ), "parent": dict(os.environ, RRT_LIBRARY=parent_lib)}
    gate = {"trace_closest_ms": {"branch": [], "parent": []}, "bench_ms_per_step": {"branch": [], "parent": []}, "bench_value": {"branch": [], "parent": []}}
    for _ in range(2):
        for who in ("parent", "branch"):
            c = subprocess.run([sys.executable, me, str(reps), "--trace-only"], env=envs[who], capture_output=True, text=True, timeout=300)
            assert c.returncode == 0, c.stderr[-2000:]
            gate["trace_closest_ms"][who] += json.loads(c.stdout.strip().splitlines()[-1])["trace_closest_ms"]
            c = subprocess.run([sys.executable, os.path.join(trees[who], "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=trees[who], env=dict(os.environ),
                               capture_output=True, text=True, timeout=300)
            assert c.returncode == 0, c.stderr[-2000:]
            b = json.loads(c.stdout.strip().splitlines()[-1])
            gate["bench_ms_per_step"][who].append(b["ms_per_step"]); gate["bench_value"][who].append(b["value"])
    for k in ("trace_closest_ms", "bench_ms_per_step"):
        for who in ("branch", "parent"):
            v = gate[k][who]
            gate[k][who] = dict(median=float(np.median(v)), min=min(v), max=max(v), spread=max(v) - min(v), rounds=v)
        # the medians differ by no more than the larger run-to-run spread (max - min of a build's own rounds)
        gate[k]["inside_the_spread"] = bool(abs(gate[k]["branch"]["median"] - gate[k]["parent"]["median"]) <= max(gate[k]["parent"]["spread"], gate[k]["branch"]["spread"]))
    out["gate"] = gate
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "surface_time.json"), "w") as f:
        f.write(line + "\n")
