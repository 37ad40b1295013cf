"""The numpy side of test_nearest.py (f64): rrt_nearest restated as a brute force over all triangle entries, its scenes and its query points.

Per entry of prim_order the world-space vertices come from surface_reference.geometry(): the mesh's raw vertices through the primitive's instance
transform M. For fp32 handles the world vertices and the points are rounded to float32 first, then everything is computed in f64. The closest point of
a candidate is include/rrt.h's region algorithm (Ericson 5.1.5), vectorised over candidates; the winner is the smallest d2, the smallest index among
equal ones, never a NaN.

The region algorithm checks itself (self_check) against an independent formulation: project the point onto the triangle's plane and keep the
projection if it is inside, else take the smallest distance to the three edge segments.
"""
import os

import numpy as np

import surface_reference as SR
from rs_ray_toy_amd import RRT_FIXED_BVH, Scene, scenes


# ---- the region algorithm ---------------------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest_on_triangles(p, a, b, c):
    """p (..., 3) against triangles a, b, c (..., 3), broadcast: (b1, b2, d2) by the region rules of include/rrt.h, first matching rule wins"""
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2; vb = d5 * d2 - d1 * d6; va = d3 * d6 - d5 * d4
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        rules = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        b1 = np.select(rules, [zero, one, d1 / (d1 - d3), zero, zero, 1.0 - w], vb * den)
        b2 = np.select(rules, [zero, zero, zero, one, d2 / (d2 - d6), w], vc * den)
        b1 = np.where(b1 < 0, 0.0, np.where(b1 > 1, 1.0, b1))      # (NaN passes through)
        b2 = np.where(b2 < 0, 0.0, np.where(b2 > 1, 1.0, b2))
        q = a + (ab * b1[..., None] + ac * b2[..., None])
        e = p - q
        return b1, b2, _dot(e, e)


def _segment_d2(p, u, v):
    with np.errstate(all="ignore"):
        uv = v - u
        l2 = _dot(uv, uv)
        t = np.where(l2 > 0, np.clip(_dot(p - u, uv) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0), 0.0)
        e = p - (u + uv * t[..., None])
        return _dot(e, e)


def independent_d2(p, a, b, c):
    """The squared distance by another route: the projection onto the plane where it falls inside the triangle, else the nearest of the three segments"""
    with np.errstate(all="ignore"):
        n = np.cross(b - a, c - a)
        nn = _dot(n, n)
        ok = nn > 0
        nn1 = np.where(ok, nn, 1.0)
        h = _dot(p - a, n)
        proj = p - n * (h / nn1)[..., None]
        # inside iff the three sub-triangle areas have the triangle's orientation
        s0 = _dot(np.cross(b - a, proj - a), n); s1 = _dot(np.cross(c - b, proj - b), n); s2 = _dot(np.cross(a - c, proj - c), n)
        inside = ok & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
        seg = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, b, c)), _segment_d2(p, c, a))
        return np.where(inside, np.minimum(h * h / nn1, seg), seg)


def self_check(seed=5):
    """dict(kind -> (n, n_nan, largest |d_region - d_independent| / scale)) over random triangles, points on vertices, on edges and in the plane, and
    zero-area triangles (two equal vertices; three collinear vertices). scale = the largest coordinate difference of the case."""
    rng = np.random.default_rng(seed)
    n = 4000
    a, b, c = (rng.normal(size=(n, 3)) * 3.0 + 10.0 for _ in range(3))
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    inplane = a + (b - a) * (rng.random(n) * 3 - 1)[:, None] + (c - a) * (rng.random(n) * 3 - 1)[:, None]
    t = rng.random(n)[:, None]
    cases = {
        "random": (rng.normal(size=(n, 3)) * 6.0 + 10.0, a, b, c),
        "vertex": (np.where((np.arange(n) % 3 == 0)[:, None], a, np.where((np.arange(n) % 3 == 1)[:, None], b, c)), a, b, c),
        "edge": (np.where((np.arange(n) % 3 == 0)[:, None], a + (b - a) * t, np.where((np.arange(n) % 3 == 1)[:, None], b + (c - b) * t, c + (a - c) * t)), a, b, c),
        "inside": (a + (b - a) * u[:, None] + (c - a) * v[:, None], a, b, c),
        "plane": (inplane, a, b, c),
        "two_equal": (rng.normal(size=(n, 3)) * 6.0 + 10.0, a, np.where((np.arange(n) % 2 == 0)[:, None], a, b), np.where((np.arange(n) % 2 == 0)[:, None], c, b)),
        "collinear": (rng.normal(size=(n, 3)) * 6.0 + 10.0, a, a + (b - a) * 0.5, a + (b - a) * (rng.random(n) * 4 - 2)[:, None]),
    }
    # collinear in exact arithmetic: small integers, so that va = vb = vc = 0 exactly and an edge rule decides ("collinear" above is collinear up to
    # rounding: a sliver whose area is noise, where the face rule may divide noise by noise - its site is on the triangle but need not be the nearest)
    ia = rng.integers(-8, 9, size=(n, 3)).astype(np.float64); idir = rng.integers(-4, 5, size=(n, 3)).astype(np.float64)
    idir[(idir == 0).all(1)] = (1.0, 2.0, -1.0)
    k1, k2 = rng.integers(1, 6, size=(n, 1)).astype(np.float64), rng.integers(-6, 7, size=(n, 1)).astype(np.float64)
    cases["collinear_exact"] = (rng.integers(-12, 13, size=(n, 3)).astype(np.float64), ia, ia + idir * k1, ia + idir * k2)
    out = {}
    for kind, (p, ta, tb, tc) in cases.items():
        b1, b2, d2 = closest_on_triangles(p, ta, tb, tc)
        ref = independent_d2(p, ta, tb, tc)
        nan = np.isnan(d2)
        scale = max(np.ptp(np.concatenate([p, ta, tb, tc])), 1.0)
        dev = np.abs(np.sqrt(d2[~nan]) - np.sqrt(ref[~nan])).max() / scale if (~nan).any() else 0.0
        inside_ok = bool(((b1[~nan] >= 0) & (b2[~nan] >= 0) & (b1[~nan] + b2[~nan] <= 1 + 1e-15)).all())
        out[kind] = dict(n=n, nan=int(nan.sum()), dev=float(dev), inside=inside_ok, beyond=int((np.sqrt(d2[~nan]) < np.sqrt(ref[~nan]) - 1e-9 * scale).sum()))
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------------------
CASES = ("cfg5", "rigid", "scaled", "rigid_sphere")
_scenes = {}

HAND_TRIS = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]],             # T0: the right triangle
                      [[4, 0, 0], [0, 4, 0], [2, 2, -4]],            # T1: shares T0's hypotenuse and hangs straight down from it
                      [[100, 100, 100], [100, 100, 100], [104, 100, 100]],      # two equal vertices
                      [[100, 200, 100], [102, 200, 100], [104, 200, 100]]], np.float64)   # collinear


def _hand(wd):
    with open(os.path.join(wd, "hand.obj"), "w") as f:
        for t in HAND_TRIS:
            for v in t:
                f.write(f"v {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}\n")
        for k in range(len(HAND_TRIS)):
            f.write(f"f {3 * k + 1} {3 * k + 2} {3 * k + 3}\n")
    cfg = scenes._base(16, 16, SR.NSAMP, {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 2})
    cfg["objs"] = [{"filename": "hand.obj", "obj_name": "hand"}]
    cfg["lights"] = [{"light_type": "distant", "l": {"values": [1.0, 1.0, 1.0]}, "from": [0.3, 1.0, 0.2], "to": [0.0, 0.0, 0.0]}]
    cfg["Aggregate"]["primitives"] = [{"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "hand"}]
    return cfg, wd


def scene(workdir, name):
    """surface_reference's scenes, plus "rigid_sphere" (rigid with a sphere primitive added: no candidate) and "hand" (HAND_TRIS)"""
    if name in SR._BUILD:
        return SR.scene(workdir, name)
    if name not in _scenes:
        wd = os.path.join(workdir, "nearest_" + name)
        os.makedirs(wd, exist_ok=True)
        if name == "rigid_sphere":
            cfg, root = SR._cfg3_tilted(wd)
            cfg["Aggregate"]["primitives"].append({"primitive_type": "sphere", "material_name": "mat_matte", "radius": 0.75, "instances": [{"world_pos": [33.0, 2.0, 1.0]}]})
        elif name == "hand":
            cfg, root = _hand(wd)
        else:
            raise KeyError(name)
        # (the fixed builder: the reference-exact one drops primitives inside its treelets (Q26), here the sphere)
        _scenes[name] = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    return _scenes[name]


_world = {}


def world_triangles(sc, name, f32):
    """(entries (k,) int32: the triangle entries of prim_order, V (k, 3, 3): their world-space vertices, rounded to float32 for fp32 handles)"""
    key = (name, bool(f32))
    if key not in _world:
        P, M, _ = SR.geometry(sc, name)
        ent = SR.triangle_entries(sc, name)
        V = np.einsum("kij,kvj->kvi", M[ent][:, :3, :3], P[ent]) + M[ent][:, None, :3, 3]
        if f32:
            V = V.astype(np.float32).astype(np.float64)
        V.setflags(write=False)
        _world[key] = (ent, V)
    return _world[key]


def site_point(V_of_entry, b1, b2):
    """a + ((b - a) b1 + (c - a) b2) on the world vertices (m, 3, 3) of the reported entries"""
    a, b, c = V_of_entry[:, 0], V_of_entry[:, 1], V_of_entry[:, 2]
    return a + ((b - a) * np.asarray(b1, np.float64)[:, None] + (c - a) * np.asarray(b2, np.float64)[:, None])


def brute(sc, name, p, f32, chunk=512):
    """rrt_nearest with max_dist = inf restated: dict(prim (m,) int32 index into prim_order, b1, b2, dist (m,)), -1 / 0 / 0 / inf for a point with a
    non-finite coordinate. The points are rounded to float32 for fp32 handles.
    Every (point, triangle) pair is looked at; the region algorithm runs on the pairs that an exact test cannot rule out: with D the distance from the
    point to the triangle's centroid and r the triangle's largest centroid-to-vertex distance, the triangle lies between D - r and D + r away, so a
    pair with D - r above the smallest D + r of its point (plus 1e-9 of the scene's size) cannot hold the smallest distance, nor tie it."""
    ent, V = world_triangles(sc, name, f32)
    p = np.asarray(p, np.float64)
    if f32:
        p = p.astype(np.float32).astype(np.float64)
    m = len(p)
    prim = np.full(m, -1, np.int32); ob1 = np.zeros(m); ob2 = np.zeros(m); dist = np.full(m, np.inf)
    live = np.flatnonzero(np.isfinite(p).all(1))
    cent = V.mean(1)
    r = np.linalg.norm(V - cent[:, None, :], axis=2).max(1)
    slack = 1e-9 * max(float(np.abs(V).max()), 1.0)
    for s in range(0, len(live), chunk):
        idx = live[s:s + chunk]
        D = np.linalg.norm(p[idx, None, :] - cent[None, :, :], axis=2)      # (chunk, k)
        upper = (D + r).min(1)
        rows, cols = np.nonzero(D - r <= (upper + slack + 1e-9 * upper)[:, None])
        b1, b2, d2 = closest_on_triangles(p[idx][rows], V[cols, 0], V[cols, 1], V[cols, 2])
        d2 = np.where(np.isnan(d2), np.inf, d2)
        order = np.lexsort((cols, d2, rows))      # per point: the smallest d2 first, the smallest entry among equal ones (entries ascend with cols)
        first = order[np.r_[True, rows[order][1:] != rows[order][:-1]]]
        got = np.isfinite(d2[first])
        at = idx[rows[first]]
        prim[at] = np.where(got, ent[cols[first]], -1)
        ob1[at] = np.where(got, b1[first], 0.0); ob2[at] = np.where(got, b2[first], 0.0)
        dist[at] = np.where(got, np.sqrt(d2[first]), np.inf)
    return dict(prim=prim, b1=ob1, b2=ob2, dist=dist)


def brute_all_pairs(sc, name, p, f32, chunk=64):
    """brute() without the cull: the region algorithm on every pair (slow; the CPU test holds the two against each other on a subset)"""
    ent, V = world_triangles(sc, name, f32)
    p = np.asarray(p, np.float64)
    if f32:
        p = p.astype(np.float32).astype(np.float64)
    m = len(p)
    prim = np.full(m, -1, np.int32); ob1 = np.zeros(m); ob2 = np.zeros(m); dist = np.full(m, np.inf)
    live = np.flatnonzero(np.isfinite(p).all(1))
    a, b, c = V[None, :, 0], V[None, :, 1], V[None, :, 2]
    for s in range(0, len(live), chunk):
        idx = live[s:s + chunk]
        b1, b2, d2 = closest_on_triangles(p[idx, None, :], a, b, c)      # (chunk, k)
        d2 = np.where(np.isnan(d2), np.inf, d2)
        win = np.argmin(d2, axis=1)      # the first smallest: entries ascend, so the smallest index among equal d2
        rows = np.arange(len(idx))
        got = np.isfinite(d2[rows, win])
        prim[idx] = np.where(got, ent[win], -1)
        ob1[idx] = np.where(got, b1[rows, win], 0.0); ob2[idx] = np.where(got, b2[rows, win], 0.0)
        dist[idx] = np.where(got, np.sqrt(d2[rows, win]), np.inf)
    return dict(prim=prim, b1=ob1, b2=ob2, dist=dist)


# ---- query points ---------------------------------------------------------------------------------------------------------------------------------------------
def points(sc, name, n_uniform=1000, n_hits=300, n_tris=250, seed=11, with_hits=True, total=4000):
    """About 4 000 points (float32-representable, so that both precisions are asked the same ones): uniform in 1.5 x the world bound; the
    oracle's first-hit points themselves and those moved by +-1e-3 of the extent along the normal; the vertices and edge midpoints of up to n_tris
    triangles (ties); eight points 100 extents away. Returns (p (m, 3), kinds (m,) of "uniform", "hit", "lifted", "vertex", "mid", "far")."""
    rng = np.random.default_rng(seed)
    wb = np.ctypeslib.as_array(sc.desc.world_bound).astype(np.float64)
    ext = SR.extent(sc)
    centre, half = 0.5 * (wb[:3] + wb[3:]), 0.75 * (wb[3:] - wb[:3])
    parts = []
    if with_hits:
        ref = SR.reference(sc, name)
        hi = np.flatnonzero(ref["hit"])
        hi = hi[rng.permutation(len(hi))[:n_hits]]
        parts.append(("hit", ref["p"][hi]))
        parts.append(("lifted", np.concatenate([ref["p"][hi] + 1e-3 * ext * ref["n"][hi], ref["p"][hi] - 1e-3 * ext * ref["n"][hi]])))
    ent, V = world_triangles(sc, name, False)
    pick = V[rng.permutation(len(V))[:n_tris]]
    parts.append(("vertex", pick.reshape(-1, 3)))
    parts.append(("mid", (0.5 * (pick + np.roll(pick, -1, axis=1))).reshape(-1, 3)))
    corners = np.array([[(i >> k) & 1 for k in range(3)] for i in range(8)], np.float64) * 2.0 - 1.0
    parts.append(("far", centre + corners * 100.0 * ext))
    n_uniform = max(n_uniform, total - sum(len(q) for _, q in parts))      # small scenes have few vertices: uniform points make up the number
    parts.insert(0, ("uniform", centre + half * (2.0 * rng.random((n_uniform, 3)) - 1.0)))
    p = np.concatenate([q for _, q in parts]).astype(np.float32).astype(np.float64)
    kinds = np.concatenate([np.full(len(q), k) for k, q in parts])
    p.setflags(write=False)
    return p, kinds
