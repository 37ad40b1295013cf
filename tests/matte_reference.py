"""numpy reference (f64) of the ID mattes of rrt_render_mattes, derived from the oracle alone, built like tests/aov_reference.py:
oracle_camera_samples gives every sample's film point, ray and weight, oracle_trace_closest its first-hit primitive, aov_reference._splat
the (pixel, sample, fw) pairs of the film's filter, and the table rule of include/rrt.h is applied literally, pair by pair.
Test infrastructure only (tests/test_mattes.py)."""
import numpy as np

import aov_reference as AR
import oracle_lib as O


def samples(scene, rect=None, rank=0, world=1, max_samples=0, flat=False):
    """The camera samples rrt_render_mattes takes for `rect` (rank / world: its interleaved 16-row bands), as aov_reference.samples lays them out
    ([pixel][sample], pixels row by row): dict(p_film, px, py, weight, live, hit, prim) - prim indexes prim_order, -1 where nothing is hit."""
    d = scene.desc
    W, H = scene.resolution
    x0, y0, x1, y1 = rect or (0, 0, W, H)
    nsamp = int(d.sampler.samples_per_pixel)
    s1 = nsamp if max_samples == 0 else min(nsamp, 1 + max_samples)
    ns = s1 - 1
    dims, rays, w = O.camera_samples(scene, (x0, y0, x1, y1), 1, s1)
    ys, xs = np.mgrid[y0:y1, x0:x1]
    px, py = np.repeat(xs.ravel(), ns), np.repeat(ys.ravel(), ns)
    keep = ((py - y0) // 16) % world == rank if world > 1 else np.ones(len(px), bool)
    px, py, dims, rays, w = px[keep], py[keep], dims[keep], rays[keep], w[keep]
    p_film = np.stack([px + dims[:, 0], py + dims[:, 1]], -1)
    live = w > 0
    prim = np.full(len(w), -1, np.int64)
    li = np.nonzero(live)[0]
    if len(li):
        h = O.trace_closest(scene, rays[li, :3], rays[li, 3:], np.full(len(li), np.inf), flat=flat)
        prim[li] = h["prim"]
    return dict(p_film=p_film, px=px, py=py, weight=w, live=live, hit=prim >= 0, prim=prim)


def order_ids(scene, prim_id=None):
    """The id of every entry of prim_order: prim_id[prim_order[i]], or prims[prim_order[i]].material + 1 for prim_id None."""
    d = scene.desc
    order = np.array([d.prim_order[i] for i in range(d.n_prim_order)], np.int64)
    if prim_id is None:
        return np.array([d.prims[int(j)].material + 1 for j in order], np.uint32)
    return np.asarray(prim_id, np.uint32)[order]


def empty(scene, K):
    W, H = scene.resolution
    return dict(ids=np.zeros((H, W, K), np.uint32), coverage=np.zeros((H, W, K)), weight=np.zeros((H, W, 4)))


def rank(table):
    """Slots sorted by coverage descending, ties by ascending id, empty slots last as (0, 0) - in place."""
    ids, cov = table["ids"], table["coverage"]
    H, W, K = ids.shape
    for y in range(H):
        for x in range(W):
            slots = sorted(((-c, i) for i, c in zip(ids[y, x].tolist(), cov[y, x].tolist()) if c != 0))
            ids[y, x] = [i for _, i in slots] + [0] * (K - len(slots))
            cov[y, x] = [-c for c, _ in slots] + [0.0] * (K - len(slots))
    return table


def pairs(scene, s, prim_id=None):
    """(pixel index y * W + x, fw, hit, id) of every (live sample, film pixel) pair with fw != 0, grouped by pixel, a pixel's pairs in arrival
    order (box filter: sample-number order)."""
    W, _ = scene.resolution
    y, x, i, fw = AR._splat(scene, s)
    keep = fw != 0
    y, x, i, fw = y[keep], x[keep], i[keep], fw[keep]
    pix = y * W + x
    o = np.argsort(pix, kind="stable")
    ids = order_ids(scene, prim_id)
    hit = s["hit"][i]
    sid = np.where(hit, ids[np.maximum(s["prim"][i], 0)], 0).astype(np.uint32)
    return pix[o], fw[o], hit[o], sid[o]


def apply(scene, table, s, prim_id=None):
    """The table rule of rrt.h, literally: continues `table` (dict ids (H, W, K), coverage (H, W, K), weight (H, W, 4), f64) with the samples
    `s`, then ranks it. Returns the table."""
    W, H = scene.resolution
    K = table["ids"].shape[2]
    ids, cov, wgt = table["ids"].reshape(H * W, K), table["coverage"].reshape(H * W, K), table["weight"].reshape(H * W, 4)
    pix, fw, hit, sid = pairs(scene, s, prim_id)
    cur, row_i, row_c, w = -1, None, None, None

    def flush():
        if cur >= 0:
            ids[cur], cov[cur], wgt[cur, :3] = row_i, row_c, w

    for p, f, h, i in zip(pix.tolist(), fw.tolist(), hit.tolist(), sid.tolist()):
        if p != cur:
            flush()
            cur, row_i, row_c, w = p, ids[p].tolist(), cov[p].tolist(), wgt[p, :3].tolist()
        w[0] += f
        if not h:
            continue
        w[1] += f
        for k in range(K):
            if row_c[k] != 0 and row_i[k] == i:
                row_c[k] += f
                break
        else:
            for k in range(K):
                if row_c[k] == 0:
                    row_i[k], row_c[k] = i, f
                    break
            else:
                w[2] += f
    flush()
    return rank(table)


def mattes(scene, K, prim_id=None, rect=None, rank_=0, world=1, max_samples=0, table=None, with_samples=False):
    """The table rrt_render_mattes leaves for one call (on `table`, or on zeroed buffers)."""
    s = samples(scene, rect, rank_, world, max_samples)
    out = apply(scene, table if table is not None else empty(scene, K), s, prim_id)
    return (out, s) if with_samples else out


def complete_sums(scene, s, prim_id=None):
    """{pixel index: {id: the id's complete coverage sum}} over the hit pairs - what a table without a slot limit would hold."""
    pix, fw, hit, sid = pairs(scene, s, prim_id)
    out = {}
    for p, f, h, i in zip(pix.tolist(), fw.tolist(), hit.tolist(), sid.tolist()):
        if h:
            d = out.setdefault(p, {})
            d[i] = d.get(i, 0.0) + f
    return out
