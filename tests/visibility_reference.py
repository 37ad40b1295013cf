"""The numpy side of test_visibility.py: rrt_visibility restated.

segments() makes the rays of include/rrt.h's definition in numpy IN THE HANDLE'S TYPE, operation by operation (numpy's float32 + - * / sqrt are the
IEEE ones and nothing is fused): the unit normals, the moved ends, w, len, d, tmax, and the verdict that needs no candidate (dead, coincident,
facing). Sent through rrt_trace_all with k = 0 they give the call's bits exactly: pair visible iff count == 0.

brute() is the f64 brute force over every (pair, triangle entry): those rays taken to f64 and judged by trace_all_reference.judge against the world
vertices of nearest_reference.world_triangles (rounded to float32 for fp32 handles), with trace_all_reference's cull and margin bands (BAND). A pair
is blocked where a candidate is accepted. It is MARGINAL where one of its candidate decisions lies inside the band, or - with a FACING flag - where
the facing dot product relative to |w| does: a rounding of that size flips the bit.

pairs() are the inputs: 70 A and 131 B points (131 crosses the 64 and 128 column boundaries) at interior barycentrics of random triangle entries with
the geometric normal, the last 30 B points free in 1.5 x the world bound with the z axis as their normal (lifted along z), all float32-representable so
that both precisions are asked the same; offset_a = offset_b = 1e-3 x extent.
"""
import numpy as np

import nearest_reference as NR
import surface_reference as SR
import trace_all_reference as TR

N_A, N_B, N_FREE = 70, 131, 30
FACING_A, FACING_B = 1, 2
NO, YES, TRACE = 0, 1, 2      # the verdict before any candidate: not visible / visible untraced (coincident) / visible iff not blocked

_pairs = {}


def pairs(sc, name, seed=23):
    """dict(a, na (70, 3), b, nb (131, 3), ent_a (70,), ent_b (131,) the entry of prim_order a point lies on (-1: a free point), offset)"""
    key = (name, seed)
    if key in _pairs:
        return _pairs[key]
    rng = np.random.default_rng(seed)
    ent, V = NR.world_triangles(sc, name, False)
    ext = SR.extent(sc)

    def on_surface(n):
        pick = rng.integers(0, len(V), n)
        tri = V[pick]
        u, v = rng.random(n), rng.random(n)
        flip = u + v > 1
        u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
        u, v = 0.05 + 0.85 * u, 0.05 + 0.85 * v                         # interior: every barycentric at least 0.05
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        p = tri[:, 0] + e1 * u[:, None] + e2 * v[:, None]
        g = np.cross(e1, e2)
        return p, g / np.linalg.norm(g, axis=1)[:, None], ent[pick].astype(np.int32)

    a, na, ent_a = on_surface(N_A)
    b, nb, ent_b = on_surface(N_B - N_FREE)
    wb = np.ctypeslib.as_array(sc.desc.world_bound).astype(np.float64)
    centre, half = 0.5 * (wb[:3] + wb[3:]), 0.75 * (wb[3:] - wb[:3])
    b = np.concatenate([b, centre + half * (2.0 * rng.random((N_FREE, 3)) - 1.0)])
    nb = np.concatenate([nb, np.tile([0.0, 0.0, 1.0], (N_FREE, 1))])
    ent_b = np.concatenate([ent_b, np.full(N_FREE, -1, np.int32)])
    P = dict(a=a, na=na, b=b, nb=nb)
    P = {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}
    P.update(ent_a=ent_a, ent_b=ent_b, offset=float(np.float32(1e-3 * ext)))
    for v in P.values():
        if isinstance(v, np.ndarray): v.setflags(write=False)
    _pairs[key] = P
    return P


# ---- the definition, in the handle's type ----------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def ends(p, n, offset, dtype):
    """(q, nn, live): the points moved by offset along their unit normals (n None: q = p, nn = 0)"""
    with np.errstate(all="ignore"):
        p = np.asarray(p).astype(dtype)
        live = np.isfinite(p).all(1)
        if n is None:
            return p, np.zeros_like(p), live
        n = np.asarray(n).astype(dtype)
        nn = n / np.sqrt(_dot(n, n))[:, None]
        q = p + nn * dtype(offset)
        live = live & np.isfinite(n).all(1) & (n != 0).any(1) & np.isfinite(nn).all(1) & np.isfinite(q).all(1)
        return q, nn, live


def segments(a, b, dtype, na=None, nb=None, offset_a=0.0, offset_b=0.0, flags=0, directions=False, pairs=False):
    """The rays of pairs (i, j), row-major over (n_a, n_b) - or of the pairs (i, i) -, in dtype: dict(o, d (m, 3), tmax (m,), verdict (m,) of NO, YES,
    TRACE, facing (m,): the smaller facing dot product relative to |w| in f64 where a flag is set, else +inf; shape (n_a, n_b) or (n_a,))"""
    dtype = np.dtype(dtype).type
    qa, nna, la = ends(a, na, offset_a, dtype)
    qb, nnb, lb = ends(b, nb, offset_b, dtype)
    if pairs:
        ii = jj = np.arange(len(qa))
        shape = (len(qa),)
    else:
        ii, jj = (x.ravel() for x in np.meshgrid(np.arange(len(qa)), np.arange(len(qb)), indexing="ij"))
        shape = (len(qa), len(qb))
    with np.errstate(all="ignore"):
        o = qa[ii]
        w = qb[jj] if directions else qb[jj] - o
        ln = np.sqrt(_dot(w, w))
        d = w / ln[:, None]
        tmax = np.full(len(ii), np.inf, dtype) if directions else ln
        verdict = np.full(len(ii), TRACE, np.int8)
        facing = np.full(len(ii), np.inf)
        if flags & FACING_A:
            fa = _dot(nna[ii], w)
            verdict[~(fa > 0)] = NO
            facing = np.minimum(facing, fa.astype(np.float64) / ln.astype(np.float64))
        if flags & FACING_B:
            fb = _dot(nnb[jj], w)
            verdict[~(fb < 0)] = NO
            facing = np.minimum(facing, -fb.astype(np.float64) / ln.astype(np.float64))
        verdict[ln == 0] = YES if (not directions and flags == 0) else NO
        verdict[~np.isfinite(ln)] = NO
        verdict[~(la[ii] & lb[jj])] = NO
    return dict(o=o, d=d, tmax=tmax, verdict=verdict, facing=facing, shape=shape, ii=ii, jj=jj)


def pack(vis):
    """bool (n_a, n_b) -> uint64 (n_a, words) as rrt_visibility packs a row; bool (n,) -> (words,)"""
    vis = np.asarray(vis, bool)
    n = vis.shape[-1]
    words = (n + 63) // 64
    padded = np.zeros(vis.shape[:-1] + (words * 64,), np.uint64)
    padded[..., :n] = vis
    shifts = np.arange(64, dtype=np.uint64)
    return (padded.reshape(vis.shape[:-1] + (words, 64)) << shifts).sum(-1, dtype=np.uint64)


# ---- the f64 brute force ---------------------------------------------------------------------------------------------------------------------------------
def brute(sc, name, seg, f32, skip_a=None, skip_b=None, chunk=128):
    """dict(visible (shape) bool, marginal (shape) bool) of the segments `seg` (segments() in the handle's dtype): every traced pair against every
    triangle entry other than its skip entries, by trace_all_reference.judge in f64"""
    ent, V = NR.world_triangles(sc, name, f32)
    ext = SR.extent(sc)
    band = TR.BAND[bool(f32)]
    o, d, tmax = (seg[k].astype(np.float64) for k in ("o", "d", "tmax"))
    m = len(o)
    cent = V.mean(1)
    rad = np.linalg.norm(V - cent[:, None, :], axis=2).max(1)
    slack = 1e-3 * max(float(np.abs(V).max()), ext)
    blocked = np.zeros(m, bool)
    marginal = np.zeros(m, bool)
    idx = np.flatnonzero(seg["verdict"] == TRACE)
    for s in range(0, len(idx), chunk):
        sel = idx[s:s + chunk]
        w = cent[None, :, :] - o[sel, None, :]
        dist = np.linalg.norm(np.cross(w, d[sel, None, :]), axis=2) / np.linalg.norm(d[sel], axis=1)[:, None]
        rr, cc = np.nonzero(dist <= 1.05 * rad[None, :] + slack)      # (trace_all_reference.brute's cull: farther pairs are neither accepted nor marginal)
        rows = sel[rr]
        keep = np.ones(len(rows), bool)
        if skip_a is not None: keep &= ent[cc] != np.asarray(skip_a)[seg["ii"][rows]]
        if skip_b is not None: keep &= ent[cc] != np.asarray(skip_b)[seg["jj"][rows]]
        rows, cc = rows[keep], cc[keep]
        ok, _, _, _, margin = TR.judge(o[rows], d[rows], tmax[rows], V[cc, 0], V[cc, 1], V[cc, 2], f32, ext)
        blocked[rows[ok]] = True
        marginal[rows[np.abs(margin) < band]] = True
    marginal |= (seg["verdict"] != YES) & (np.abs(seg["facing"]) < band)
    visible = (seg["verdict"] == YES) | ((seg["verdict"] == TRACE) & ~blocked)
    return dict(visible=visible.reshape(seg["shape"]), marginal=marginal.reshape(seg["shape"]))
