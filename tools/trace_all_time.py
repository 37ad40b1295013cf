"""rrt_trace_all timed: config 4 (100 352 triangles, fixed BVH), default fp32 handle, everything device resident.

  workload    2^20 rays between uniform random points of 1.2 x the world bound (unit directions, unbounded): a ray crosses the height field 0 to a few times.
  variants    alternated in one process, three rounds each: rrt_trace_all at k = 1, 4 and 16, with and without `count`, and the count-only form (k = 0);
              the yardsticks: (a) one rrt_trace_closest over the same rays, (b) a peel of k rrt_trace_closest calls - each followed by the device
              arithmetic that advances the origin to the hit and sets skip_prim to the primitive just found - for k = 1, 4 and 16.
              The slots of the calls without `count` are compared bit for bit with those of the calls with it, and the slots of a smaller k with the
              first planes of k = 16.

Times are device events on the handle's stream around `reps` repetitions (the calls return with their work done). Prints one JSON line;
RRT_RESULTS_DIR=<dir> also keeps it as <dir>/trace_all_time.json.
Usage: python tools/trace_all_time.py [reps]"""
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

DEV = "cuda:0"
GRID = 224
N = 1 << 20
KS = (1, 4, 16)
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


def main():
    cfg, root = scenes.cfg4(wd, xres=64, yres=64, nsamp=2, max_depth=8, n=GRID)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    wb = np.ctypeslib.as_array(sc.desc.world_bound).astype(np.float64)
    rng = np.random.default_rng(41)
    centre, half = 0.5 * (wb[:3] + wb[3:]), 0.6 * (wb[3:] - wb[:3])
    a, b = (centre + half * (2.0 * rng.random((N, 3)) - 1.0) for _ in range(2))
    d = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
    o_cols = [torch.from_numpy(np.ascontiguousarray(a[:, k], np.float32)).to(DEV) for k in range(3)]
    d_cols = [torch.from_numpy(np.ascontiguousarray(d[:, k], np.float32)).to(DEV) for k in range(3)]
    tmax = torch.full((N,), float("inf"), dtype=torch.float32, device=DEV)
    ptrs7 = [t.data_ptr() for t in o_cols + d_cols + [tmax]]
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    outs = {(k, c): dict(t=f32(k, N), prim=i32(k, N), b1=f32(k, N), b2=f32(k, N), **({"count": i32(N)} if c else {})) for k in KS for c in (True, False)}
    count0 = i32(N)
    hit = dict(t=f32(N), prim=i32(N), u=f32(N), v=f32(N))
    peel_o = [t.clone() for t in o_cols]
    peel_skip = i32(N)
    torch.cuda.synchronize()

    def trace_all(k, c):
        r.trace_all_device(ptrs7, N, {f: t.data_ptr() for f, t in outs[(k, c)].items()}, k)

    def count_only():
        r.trace_all_device(ptrs7, N, {"count": count0.data_ptr()}, 0)

    def closest():
        r.trace_closest_device(ptrs7, N, hit["t"].data_ptr(), hit["prim"].data_ptr(), hit["u"].data_ptr(), hit["v"].data_ptr())

    def peel(k):
        st = torch.cuda.ExternalStream(r.stream)
        with torch.cuda.stream(st):
            for j in range(3): peel_o[j].copy_(o_cols[j])
            peel_skip.fill_(-1)
            p7 = [t.data_ptr() for t in peel_o + d_cols + [tmax]]
            for _ in range(k):
                r.trace_closest_device(p7, N, hit["t"].data_ptr(), hit["prim"].data_ptr(), hit["u"].data_ptr(), hit["v"].data_ptr(), skip_ptr=peel_skip.data_ptr())
                live = hit["prim"] >= 0
                for j in range(3): peel_o[j].add_(torch.where(live, d_cols[j] * hit["t"], torch.zeros_like(hit["t"])))
                peel_skip.copy_(hit["prim"])

    variants = {f"trace_all_k{k}_{'count' if c else 'nocount'}": (lambda k=k, c=c: trace_all(k, c)) for k in KS for c in (True, False)}
    variants["trace_all_k0_count_only"] = count_only
    variants["trace_closest"] = closest
    variants.update({f"peel_k{k}": (lambda k=k: peel(k)) for k in KS})
    for fn in variants.values(): fn()      # warm-up
    rounds = {name: [] for name in variants}
    for _ in range(3):
        for name, fn in variants.items():
            rounds[name].append(event_ms(r, fn, max(1, reps // 4) if name.startswith("peel") else reps))
    torch.cuda.synchronize()
    big = outs[(16, True)]
    same_nocount = all(bool(torch.equal(outs[(k, False)][f].view(torch.int32), outs[(k, True)][f].view(torch.int32))) for k in KS for f in ("t", "prim", "b1", "b2"))
    prefixes = all(bool(torch.equal(outs[(k, True)][f].view(torch.int32), big[f][:k].view(torch.int32))) for k in KS for f in ("t", "prim", "b1", "b2"))
    counts_same = all(bool(torch.equal(outs[(k, True)]["count"], count0)) for k in KS)
    closest(); torch.cuda.synchronize()
    both = (hit["prim"] >= 0) & (big["prim"][0] >= 0)
    cnt = big["count"].to(torch.int64)
    med = {name: float(np.median(v)) for name, v in rounds.items()}
    res = {"rays": N, "ms": {name: dict(median=med[name], rounds=v) for name, v in rounds.items()}, "ns_per_ray": {name: v * 1e6 / N for name, v in med.items()},
           "slots_without_count_same_bits": same_nocount, "smaller_k_are_prefixes": prefixes, "count_same_at_every_k": counts_same,
           "hits_per_ray": {"mean": float(cnt.double().mean()), "max": int(cnt.max()), "rays_with_none": int((cnt == 0).sum()), "rays_with_more_than_16": int((cnt > 16).sum())},
           "trace_closest_names_slot_0": float((hit["prim"][both] == big["prim"][0][both]).double().mean()),
           "trace_all_over_trace_closest": {name: med[name] / med["trace_closest"] for name in med if name.startswith("trace_all")},
           "peel_over_trace_all": {f"k{k}": med[f"peel_k{k}"] / med[f"trace_all_k{k}_count"] for k in KS}}
    r.close()
    return res


out = {"what": "config 4 (100 352 triangles, fixed BVH), fp32, one MI355X, device arrays, device events on the handle's stream, ms per call", "reps": reps, **main()}
line = json.dumps(out)
print(line)
if os.environ.get("RRT_RESULTS_DIR"):
    os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
    with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "trace_all_time.json"), "w") as f:
        f.write(line + "\n")
