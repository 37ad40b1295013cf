"""The numpy side of test_trace_all.py (f64): rrt_trace_all restated as a brute force over all (ray, triangle entry) pairs, its scenes and its rays.

Per entry of prim_order the world-space vertices come from nearest_reference.world_triangles() (surface_reference.geometry(): the mesh's raw vertices
through the primitive's instance transform). For fp32 handles the world vertices and the rays are rounded to float32 first, then everything is
computed in f64. A pair is accepted by include/rrt.h's three rules - Moller-Trumbore in the written-down order, t < tmax, the slab test of the
candidate's own box with the far factor of the handle's type -, and the accepted pairs of a ray are sorted by (t, entry).

Every pair is looked at; the three rules run on the pairs an exact test cannot rule out: a ray whose line passes farther from a triangle's centroid
than 1.05 x the triangle's largest centroid-to-vertex distance plus 1e-3 of the scene's size meets the triangle's plane outside the triangle by far
more than any band below, so such a pair is neither accepted nor marginal (brute_all_pairs() is the same without the cull; the CPU tests hold the
two against each other).

The reference's own margins. Each rule's decision has a margin - how far the quantity is from the value at which the decision flips: min(u, 1 - u),
v, 1 - u - v (absolute), t - 1e-7, tmax - t and the slab test's min(fars, tmax) - max(nears, 0) (relative to the scene extent; the rays' directions
have unit length, so t is a distance), | |det| - 1e-7 | (relative to 1e-7). A pair's margin is the smallest of them: >= 0 iff accepted. A pair is
MARGINAL when its margin lies within the band (-band, band): a rounding of that size flips the decision. A ray is marginal when one of its pairs is,
or when two of its accepted hits lie within the band (x extent) of each other in t: their order is then the rounding's. Two entries of prim_order
with the same vertices are excepted from the second rule (the reference's own builder lists a primitive twice where its treelets overlap, Q26: 4 of
the 24 entries of `rigid`): they are judged on identical operands, get identical bits in t, and their order is the index's, not the rounding's.
"""
import os

import numpy as np

import nearest_reference as NR
import surface_reference as SR
from rs_ray_toy_amd import RRT_FIXED_BVH, Scene, scenes

CASES = ("cfg5", "rigid", "scaled", "rigid_sphere", "hand_closed")
BAND = {True: 1e-4, False: 1e-9}      # [f32]
K = 8
N_RAYS = 4097 + 65                     # crosses the 4 096-ray boundary of max_paths = 4096 and the 64-lane boundary

# ---- the closed hand-built scene: a unit cube and a tetrahedron, small integer coordinates, no two faces coplanar and overlapping ----------------------
CUBE_V = np.array([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], np.float64)
CUBE_F = {"X0a": (0, 2, 6), "X0b": (0, 6, 4), "X1a": (1, 3, 7), "X1b": (1, 7, 5), "Y0a": (0, 1, 5), "Y0b": (0, 5, 4), "Y1a": (2, 3, 7), "Y1b": (2, 7, 6),
          "Z0a": (0, 1, 3), "Z0b": (0, 3, 2), "Z1a": (4, 5, 7), "Z1b": (4, 7, 6)}
TET_V = np.array([[4, 0, 0], [6, 0, 0], [4, 2, 0], [4, 0, 2]], np.float64)
TET_F = {"TA": (0, 2, 3), "TB": (0, 1, 3), "TC": (0, 1, 2), "TD": (1, 2, 3)}
HAND_TRIS = {**{k: CUBE_V[list(f)] for k, f in CUBE_F.items()}, **{k: TET_V[list(f)] for k, f in TET_F.items()}}

_scenes = {}


def _hand_closed(wd):
    with open(os.path.join(wd, "closed.obj"), "w") as f:
        for t in HAND_TRIS.values():
            for v in t:
                f.write(f"v {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}\n")
        for k in range(len(HAND_TRIS)):
            f.write(f"f {3 * k + 1} {3 * k + 2} {3 * k + 3}\n")
    cfg = scenes._base(16, 16, SR.NSAMP, {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 2})
    cfg["objs"] = [{"filename": "closed.obj", "obj_name": "closed"}]
    cfg["lights"] = [{"light_type": "distant", "l": {"values": [1.0, 1.0, 1.0]}, "from": [0.3, 1.0, 0.2], "to": [0.0, 0.0, 0.0]}]
    cfg["Aggregate"]["primitives"] = [{"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "closed"}]
    return cfg, wd


def scene(workdir, name):
    if name != "hand_closed":
        return NR.scene(workdir, name)
    if name not in _scenes:
        wd = os.path.join(workdir, "trace_all_" + name)
        os.makedirs(wd, exist_ok=True)
        cfg, root = _hand_closed(wd)
        _scenes[name] = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    return _scenes[name]


def hand_entries(sc):
    """{face name: entry of prim_order} of the hand-built scene"""
    P, _, _ = SR.geometry(sc, "hand_closed")
    return {k: int(np.flatnonzero((P == t).all((1, 2)))[0]) for k, t in HAND_TRIS.items()}


def hand_inside(p):
    """analytic: inside the unit cube or the tetrahedron, and the distance to the nearest face plane of either (for keeping away from the faces)"""
    p = np.asarray(p, np.float64)
    cube = np.stack([p[:, 0], 1 - p[:, 0], p[:, 1], 1 - p[:, 1], p[:, 2], 1 - p[:, 2]], 1)
    q = p - TET_V[0]
    tet = np.stack([q[:, 0], q[:, 1], q[:, 2], (2 - q.sum(1)) / np.sqrt(3.0)], 1)
    inside = (cube.min(1) > 0) | (tet.min(1) > 0)
    # distance to the surfaces: inside a solid the smallest plane distance; outside, the distance to the clamped point (cube) / a lower bound (tetrahedron)
    d_cube = np.where(cube.min(1) > 0, cube.min(1), np.linalg.norm(p - np.clip(p, 0, 1), axis=1))
    d_tet = np.where(tet.min(1) > 0, tet.min(1), np.maximum(-tet.min(1), 0))      # outside: at least the largest violated plane distance
    return inside, np.minimum(d_cube, d_tet)


# ---- the rules --------------------------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def far_factor(f32):
    eps = 2.0 ** -24 if f32 else 2.0 ** -53
    return 1.0 + 2.0 * ((3.0 * eps) / (1.0 - 3.0 * eps))


def judge(o, d, tmax, a, b, c, f32, ext):
    """The three rules on pairs (broadcast): (accepted, t, u, v, margin) - margin as the module text defines it (in band units: absolute for the
    barycentrics, relative to ext for distances)"""
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        P = _cross(d, e2)
        det = _dot(e1, P)
        f = 1.0 / det
        T = o - a
        u = f * _dot(T, P)
        Q = _cross(T, e1)
        v = f * _dot(d, Q)
        t = f * _dot(e2, Q)
        ok = ~((det > -1e-7) & (det < 1e-7)) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 1e-7) & (t < tmax)
        lo = np.minimum(np.minimum(a, b), c); hi = np.maximum(np.maximum(a, b), c)
        inv = 1.0 / d
        n0, f0 = (lo - o) * inv, (hi - o) * inv
        near = np.where(inv < 0, f0, n0); far = np.where(inv < 0, n0, f0) * far_factor(f32)
        near = np.where(np.isnan(near), -np.inf, near); far = np.where(np.isnan(far), np.inf, far)
        tn = np.maximum(near.max(-1), 0.0)
        tf = np.minimum(far.min(-1), tmax)
        ok &= tn <= tf
        # the slab decision's margin: the smallest far_i - near_j over DIFFERENT axes i != j, far_i - 0 and tmax - near_j. An axis' own far - near is no
        # margin: both come from the same o and inv by a monotone function of lo <= hi, so far_i >= near_i whatever the rounding (a flat box has
        # far_i - near_i ~ 0 by construction and is safe all the same)
        pairs = [far[..., i] - near[..., j] for i in range(3) for j in range(3) if i != j] + [far.min(-1), tmax - near.max(-1)]
        slab = np.stack([np.where(np.isnan(q), np.inf, q) for q in pairs], -1).min(-1)
        margins = np.stack([u, 1 - u, v, 1 - u - v, (t - 1e-7) / ext, np.where(np.isinf(tmax), np.inf, (tmax - t) / ext), slab / ext, (np.abs(det) - 1e-7) / 1e-7], -1)
        margin = np.where(np.isnan(margins), -np.inf, margins).min(-1)
        return ok, t, u, v, margin


def _prepare(sc, name, o, d, tmax, f32):
    ent, V = NR.world_triangles(sc, name, f32)
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64); tmax = np.asarray(tmax, np.float64)
    if f32:
        o = o.astype(np.float32).astype(np.float64); d = d.astype(np.float32).astype(np.float64)
        with np.errstate(over="ignore"):
            tmax = tmax.astype(np.float32).astype(np.float64)
    live = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.isfinite(tmax) | (tmax == np.inf)) & (d != 0).any(1)
    return ent, V, o, d, tmax, live


def _collect(m, k, band, ext, rows, cols, ent, gid, ok, t, u, v, margin, tmax):
    """From the judged pairs (rows = ray, cols = position in ent): the slots, the counts, the marginal rays and the near-candidates"""
    out = dict(t=np.repeat(tmax[None, :], k, 0), prim=np.full((k, m), -1, np.int32), b1=np.zeros((k, m)), b2=np.zeros((k, m)), count=np.zeros(m, np.uint32))
    acc = np.flatnonzero(ok)
    order = acc[np.lexsort((cols[acc], t[acc], rows[acc]))]
    r = rows[order]
    out["count"] = np.bincount(r, minlength=m).astype(np.uint32)
    first = np.r_[0, np.flatnonzero(r[1:] != r[:-1]) + 1] if len(r) else np.zeros(0, np.int64)
    rank = np.arange(len(r)) - np.repeat(first, np.diff(np.r_[first, len(r)]))
    keep = rank < k
    out["t"][rank[keep], r[keep]] = t[order][keep]; out["prim"][rank[keep], r[keep]] = ent[cols[order]][keep]
    out["b1"][rank[keep], r[keep]] = u[order][keep]; out["b2"][rank[keep], r[keep]] = v[order][keep]
    near = np.abs(margin) < band                                        # a marginal pair
    n_marginal = np.bincount(rows[near], minlength=m)
    close = np.zeros(m, bool)                                            # two accepted hits within the band of each other
    if len(r) > 1:
        g = gid[cols[order]]
        same = (r[1:] == r[:-1]) & (np.diff(t[order]) < band * ext) & (g[1:] != g[:-1])
        close[r[1:][same]] = True
        n_marginal += np.bincount(r[1:][same], minlength=m) * 2         # (either of the two may be the one that moves)
    cand = margin > -band                                                # accepted, or rejected within the band: what a rounding may report
    key = rows[cand].astype(np.int64) * (int(ent.max()) + 1) + ent[cols[cand]]
    srt = np.argsort(key)
    out.update(marginal=(n_marginal > 0) | close, n_marginal=n_marginal, cand_key=key[srt], cand_t=t[cand][srt], key_base=int(ent.max()) + 1)
    return out


def brute(sc, name, o, d, tmax, f32, skip=None, k=K, chunk=128, cull=True):
    """rrt_trace_all restated: dict(t, prim, b1, b2 (k, m), count (m,), marginal (m,) bool, n_marginal (m,), and the near-candidates of every ray as
    (cand_key = ray * key_base + entry, sorted; cand_t))"""
    ent, V, o, d, tmax, live = _prepare(sc, name, o, d, tmax, f32)
    m = len(o)
    ext = SR.extent(sc)
    band = BAND[bool(f32)]
    cent = V.mean(1)
    rad = np.linalg.norm(V - cent[:, None, :], axis=2).max(1)
    slack = 1e-3 * max(float(np.abs(V).max()), ext)
    idx = np.flatnonzero(live)
    parts = []
    for s in range(0, len(idx), chunk):
        ii = idx[s:s + chunk]
        if cull:
            w = cent[None, :, :] - o[ii, None, :]
            dist = np.linalg.norm(_cross(w, d[ii, None, :]), axis=2) / np.linalg.norm(d[ii], axis=1)[:, None]
            rr, cc = np.nonzero(dist <= 1.05 * rad[None, :] + slack)
        else:
            rr, cc = np.divmod(np.arange(len(ii) * len(ent)), len(ent))
        rows = ii[rr]
        if skip is not None:
            keep = ent[cc] != np.asarray(skip)[rows]
            rows, cc = rows[keep], cc[keep]
        ok, t, u, v, margin = judge(o[rows], d[rows], tmax[rows], V[cc, 0], V[cc, 1], V[cc, 2], f32, ext)
        sel = margin > -1.0                                              # (keeps every accepted and every near pair; drops the bulk)
        parts.append((rows[sel], cc[sel], ok[sel], t[sel], u[sel], v[sel], margin[sel]))
    rows, cols, ok, t, u, v, margin = (np.concatenate([p[j] for p in parts]) if parts else np.zeros(0, np.int64 if j < 2 else np.float64) for j in range(7))
    gid = np.unique(V.reshape(len(V), -1), axis=0, return_inverse=True)[1].reshape(-1)      # entries with the same vertices share a group
    return _collect(m, k, band, ext, rows.astype(np.int64), cols.astype(np.int64), ent, gid, ok.astype(bool), t, u, v, margin, tmax)


def brute_all_pairs(sc, name, o, d, tmax, f32, skip=None, k=K):
    """brute() without the cull (slow: the CPU test runs it on a subset)"""
    return brute(sc, name, o, d, tmax, f32, skip, k, chunk=32, cull=False)


# ---- rays -------------------------------------------------------------------------------------------------------------------------------------------
def rays(sc, name, seed=17, total=N_RAYS, n_through=1800, n_edge=250, n_vertex=250):
    """(o, d (m, 3), tmax (m,), kinds (m,)) - float32-representable, so that both precisions are asked the same rays; d of unit length (then rounded).
    "uniform": between random points of 1.5 x the world bound; "through": from such a point at a random interior point of a random triangle; "edge",
    "vertex": at edge midpoints and vertices (ties). Every second ray has a finite tmax, between 0.3 and 1.6 times the distance to the target."""
    rng = np.random.default_rng(seed)
    wb = np.ctypeslib.as_array(sc.desc.world_bound).astype(np.float64)
    centre, half = 0.5 * (wb[:3] + wb[3:]), 0.75 * (wb[3:] - wb[:3])
    ent, V = NR.world_triangles(sc, name, False)
    uni = lambda n: centre + half * (2.0 * rng.random((n, 3)) - 1.0)
    n_edge = min(n_edge, 3 * len(V)); n_vertex = min(n_vertex, 3 * len(V))
    tri = V[rng.integers(0, len(V), n_through)]
    u, v = rng.random(n_through), rng.random(n_through)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    u, v = 0.05 + 0.85 * u, 0.05 + 0.85 * v                             # interior: every barycentric at least 0.05
    through = tri[:, 0] + (tri[:, 1] - tri[:, 0]) * u[:, None] + (tri[:, 2] - tri[:, 0]) * v[:, None]
    pick = V[rng.integers(0, len(V), n_edge)]
    e = rng.integers(0, 3, n_edge)
    edge = 0.5 * (pick[np.arange(n_edge), e] + pick[np.arange(n_edge), (e + 1) % 3])
    vert = V[rng.integers(0, len(V), n_vertex), rng.integers(0, 3, n_vertex)]
    n_uniform = total - n_through - n_edge - n_vertex
    target = np.concatenate([uni(n_uniform), through, edge, vert])
    kinds = np.concatenate([np.full(n_uniform, "uniform"), np.full(n_through, "through"), np.full(n_edge, "edge"), np.full(n_vertex, "vertex")])
    o = uni(total)
    dist = np.linalg.norm(target - o, axis=1)
    d = (target - o) / dist[:, None]
    tmax = np.where(np.arange(total) % 2 == 0, np.inf, dist * (0.3 + 1.3 * rng.random(total)))
    o = o.astype(np.float32).astype(np.float64); d = d.astype(np.float32).astype(np.float64); tmax = tmax.astype(np.float32).astype(np.float64)
    for a in (o, d, tmax): a.setflags(write=False)
    return o, d, tmax, kinds
