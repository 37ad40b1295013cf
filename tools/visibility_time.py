"""rrt_visibility timed: config 4 (100 352 triangles, fixed BVH, vt = the grid), default fp32 handle, everything device resident.

  workloads   (a) points x points: 4 096 x 4 096 sites of a 128 x 128 atlas (rrt_atlas_sites -> rrt_surface_at; every fourth texel for A, the texels two
                  further on for B), lifted 1e-3 of the extent along their normals by the call's own offsets;
              (b) points x directions: the 65 536 sites of a 256 x 256 atlas x 256 directions spread over the upper (+y) hemisphere, RRT_VIS_FACING_A.
  routes      alternated in one process, `rounds` rounds of `reps` calls each, medians over the rounds:
              visibility   one rrt_visibility call, bits and count;
              parent       the only route the parent commit offers: torch builds the same segments by the header's formulas (o = a + nn offset, w, len,
                           d = w / len, tmax) for a chunk of rows, rrt_trace_all with k = 0 counts, torch packs count == 0 into the same words and row counts;
                           chunks of 2^22 rays (117 MB of rays). A pair that fails FACING_A is given a zero direction - a dead ray, no walk - and masked.
              trace_any    one rrt_trace_any pass over the same segments, as a speed landmark only: it is the reference's shadow ray (another triangle,
                           Q11; boxes pruned at 1 - 1e-4, Q9; no t_max in the primitive test, Q10), so its answers differ - the share is reported.
  The bits of the two exact routes are compared (torch's float32 division and square root need not be the IEEE ones, so equality is reported, not assumed).

Times are device events on the handle's stream around `reps` calls (the calls return with their work done); `wall_ms` is the host clock around the same
calls, and device_share = the event time of the rrt_visibility call alone (its memset and its kernel launches) over that wall time.
bench_this=<file> / bench_parent=<file>: files of `python bench.py` JSON lines from this commit's and the parent commit's build, run alternately in the
same session, copied into the result. Prints one JSON line; RRT_RESULTS_DIR=<dir> also keeps it as <dir>/visibility_time.json.
Usage: python tools/visibility_time.py [reps] [rounds=N] [bench_this=FILE] [bench_parent=FILE]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 5
opts = dict(a.split("=", 1) for a in args)
rounds_n = int(opts.get("rounds", 3))

DEV = "cuda:0"
GRID = 224
LIFT = 1e-3
CHUNK = 1 << 22
wd = tempfile.mkdtemp()


def charted_scene():
    """config 4's mesh with vt = the grid (tools/nearest_time.py's)"""
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


def atlas_points(r, res):
    """(p (m, 3), n (m, 3)) float32 tensors: the covered sites of a res x res atlas"""
    nt = res * res
    t_prim = torch.zeros(nt, dtype=torch.int32, device=DEV)
    t_b1, t_b2 = torch.zeros(nt, dtype=torch.float32, device=DEV), torch.zeros(nt, dtype=torch.float32, device=DEV)
    rec = {k: torch.zeros(nt, dtype=torch.float32, device=DEV) for k in ("px", "py", "pz", "nx", "ny", "nz")}
    torch.cuda.synchronize()
    r.atlas_sites_device((res, res), t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr())
    r.surface_at_device(t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr(), nt, {k: t.data_ptr() for k, t in rec.items()})
    torch.cuda.synchronize()
    live = t_prim >= 0
    return torch.stack([rec[k] for k in ("px", "py", "pz")], 1)[live].contiguous(), torch.stack([rec[k] for k in ("nx", "ny", "nz")], 1)[live].contiguous()


def cols(t):
    return [t[:, k].contiguous() for k in range(3)]


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def unit(n):
    return n / torch.sqrt(dot(n, n))[:, None]


class Workload:
    def __init__(self, r, a, na, b, nb, offset, directions, facing_a):
        self.r, self.directions, self.facing_a, self.offset = r, directions, facing_a, float(np.float32(offset))
        self.n_a, self.n_b, self.words = len(a), len(b), (len(b) + 63) // 64
        self.a, self.na, self.b, self.nb = a, na, b, nb
        self._held = []
        self.ptrs = {"a": tuple(c.data_ptr() for c in self._keep(cols(a))), "na": tuple(c.data_ptr() for c in self._keep(cols(na))), "b": tuple(c.data_ptr() for c in self._keep(cols(b)))}
        if nb is not None: self.ptrs["nb"] = tuple(c.data_ptr() for c in self._keep(cols(nb)))
        i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)
        self.bits, self.count = i64(self.n_a, self.words), i32(self.n_a)
        self.p_bits, self.p_count = i64(self.n_a, self.words), i32(self.n_a)
        self.any_vis = torch.zeros(self.n_a, self.n_b, dtype=torch.bool, device=DEV)
        self.rows = max(1, CHUNK // self.n_b)
        self.ray_count = i32(self.rows * self.n_b)
        self.ray_occ = torch.zeros(self.rows * self.n_b, dtype=torch.uint8, device=DEV)
        self.shifts = torch.arange(64, dtype=torch.int64, device=DEV)
        self.st = torch.cuda.ExternalStream(r.stream)

    def _keep(self, ts):
        self._held.extend(ts)      # (the column tensors behind the raw pointers)
        return ts

    def visibility(self):
        self.r.visibility_device({**self.ptrs, "bits": self.bits.data_ptr(), "count": self.count.data_ptr()}, self.n_a, self.n_b, offset_a=self.offset,
                                 offset_b=0.0 if self.directions else self.offset, facing_a=self.facing_a, directions=self.directions)

    def _segments(self, i0, i1):
        """the rays of rows i0 .. i1 by the header's formulas, and the pairs that are traced at all"""
        off = torch.tensor(self.offset, dtype=torch.float32, device=DEV)
        nna = unit(self.na[i0:i1])
        o = (self.a[i0:i1] + nna * off)[:, None, :].expand(i1 - i0, self.n_b, 3)
        if self.directions:
            w = self.b[None, :, :].expand(i1 - i0, self.n_b, 3)
        else:
            w = (self.b + unit(self.nb) * off)[None, :, :] - o
        ln = torch.sqrt(dot(w, w))
        d = w / ln[..., None]
        tmax = torch.full_like(ln, float("inf")) if self.directions else ln
        traced = ln > 0
        if self.facing_a:
            traced = traced & (dot(nna[:, None, :].expand_as(w), w) > 0)
        d = torch.where(traced[..., None], d, torch.zeros_like(d))      # a pair that is not traced: a dead ray
        soa = [o[..., k].reshape(-1).contiguous() for k in range(3)] + [d[..., k].reshape(-1).contiguous() for k in range(3)] + [tmax.reshape(-1).contiguous()]
        return soa, traced

    def _rows(self, fn):
        with torch.cuda.stream(self.st):      # (the handle's stream: torch's work and the library's calls are ordered on it)
            for i0 in range(0, self.n_a, self.rows):
                i1 = min(self.n_a, i0 + self.rows)
                soa, traced = self._segments(i0, i1)
                fn(i0, i1, soa, traced)

    def parent(self):
        def one(i0, i1, soa, traced):
            m = (i1 - i0) * self.n_b
            self.r.trace_all_device([t.data_ptr() for t in soa], m, {"count": self.ray_count.data_ptr()}, 0)
            vis = (self.ray_count[:m].view(i1 - i0, self.n_b) == 0) & traced
            pad = torch.zeros(i1 - i0, self.words * 64, dtype=torch.int64, device=DEV)
            pad[:, :self.n_b] = vis
            self.p_bits[i0:i1] = (pad.view(i1 - i0, self.words, 64) << self.shifts).sum(-1)
            self.p_count[i0:i1] = vis.sum(1)
        self._rows(one)

    def trace_any(self):
        def one(i0, i1, soa, traced):
            m = (i1 - i0) * self.n_b
            self.r.trace_any_device([t.data_ptr() for t in soa], m, self.ray_occ.data_ptr())
            self.any_vis[i0:i1] = (self.ray_occ[:m].view(i1 - i0, self.n_b) == 0) & traced
        self._rows(one)

    def timed(self, fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(self.st)
        for _ in range(n): fn()
        e1.record(self.st)
        e1.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n

    def run(self):
        routes = {"visibility": self.visibility, "parent": self.parent, "trace_any": self.trace_any}
        for fn in routes.values(): fn()      # warm-up
        torch.cuda.synchronize()
        ev = {k: [] for k in routes}; wall = {k: [] for k in routes}
        for _ in range(rounds_n):
            for name, fn in routes.items():
                e, w = self.timed(fn, reps if name == "visibility" else max(1, reps // 2))
                ev[name].append(e); wall[name].append(w)
        med = {k: float(np.median(v)) for k, v in ev.items()}
        wmed = {k: float(np.median(v)) for k, v in wall.items()}
        vis = ((self.bits[:, :, None] >> self.shifts) & 1).view(self.n_a, -1)[:, :self.n_b].bool()
        pairs = self.n_a * self.n_b
        return {"n_a": self.n_a, "n_b": self.n_b, "pairs": pairs, "directions": self.directions, "facing_a": self.facing_a,
                "ms": {k: dict(median=med[k], rounds=ev[k]) for k in routes}, "wall_ms": {k: dict(median=wmed[k], rounds=wall[k]) for k in routes},
                "ns_per_pair": {k: med[k] * 1e6 / pairs for k in routes}, "visibility_over_parent": med["visibility"] / med["parent"],
                "visibility_over_trace_any": med["visibility"] / med["trace_any"], "device_share_of_the_call": med["visibility"] / wmed["visibility"],
                "visible_share": float(vis.double().mean()), "bits_equal_parent": bool(torch.equal(self.bits, self.p_bits)),
                "pairs_differing_from_parent": int((vis != ((self.p_bits[:, :, None] >> self.shifts) & 1).view(self.n_a, -1)[:, :self.n_b].bool()).sum()),
                "count_equal_parent": bool(torch.equal(self.count, self.p_count)), "count_is_popcount": bool(torch.equal(self.count.long(), vis.sum(1))),
                "share_where_trace_any_says_otherwise": float((self.any_vis != vis).double().mean())}


def main():
    sc = charted_scene()
    r = Renderer(sc, 0, RRT_F32)
    wb = np.ctypeslib.as_array(sc.desc.world_bound).astype(np.float64)
    ext = float(np.linalg.norm(wb[3:] - wb[:3]))
    p, n = atlas_points(r, 128)
    a_idx = torch.arange(0, len(p), 4, device=DEV)[:4096]
    b_idx = torch.arange(2, len(p), 4, device=DEV)[:4096]
    res = {"extent": ext, "lift": LIFT}
    res["points_4096_x_points_4096"] = Workload(r, p[a_idx].contiguous(), n[a_idx].contiguous(), p[b_idx].contiguous(), n[b_idx].contiguous(), LIFT * ext, False, False).run()
    p, n = atlas_points(r, 256)
    k = np.arange(256) + 0.5
    y = k / 256.0                                                   # a Fibonacci spiral over the upper hemisphere
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    rad = np.sqrt(1.0 - y * y)
    dirs = torch.from_numpy(np.stack([rad * np.cos(phi), y, rad * np.sin(phi)], 1).astype(np.float32)).to(DEV)
    res["points_65536_x_directions_256_facing_a"] = Workload(r, p[:65536].contiguous(), n[:65536].contiguous(), dirs, None, LIFT * ext, True, True).run()
    r.close()
    return res


out = {"what": "config 4 (100 352 triangles, fixed BVH), fp32, one MI355X, device arrays, device events on the handle's stream, ms per call; medians over the rounds",
       "reps": reps, "rounds": rounds_n,
       "trace_any_note": "rrt_trace_any is the reference's shadow ray (Q9 - Q11): a speed landmark whose answers differ from the geometric test", **main()}
for key in ("bench_this", "bench_parent"):
    if key in opts:
        runs = [json.loads(ln) for ln in open(opts[key]) if ln.strip().startswith("{")]
        out[key] = runs
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "visibility_time.json"), "w") as f:
        f.write(line + "\n")
