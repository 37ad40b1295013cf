"""numpy reference (f64) of the first-hit feature buffers of rrt_render_aov, derived from the oracle alone:
oracle_camera_samples gives every sample's film point, ray and weight, oracle_trace_closest(want_geometry) its first hit
(t, primitive, barycentrics, p, n), oracle_texture_eval any texture at a point, and the desc holds the materials and the
film's filter table. Test infrastructure only (tests/test_aov.py)."""
import numpy as np

import oracle_lib as O

# RRT_MAT_* of include/rrt.h and the rrt_material::tex slots rho reads
MATTE, PLASTIC, METAL, MIRROR, DEBUG, GLASS, TRANSLUCENT = range(7)
P_KD, P_KR, P_ETA, P_K = 0, 2, 3, 4


def _prim_tables(scene):
    """Per entry of prim_order: material, primitive type, and the triangle's three texture coordinates (get_uvs: (0,0), (1,0), (1,1) without a mesh uv)."""
    d = scene.desc
    n = d.n_prim_order
    mat = np.zeros(n, np.int64); is_tri = np.zeros(n, bool); uv = np.zeros((n, 3, 2))
    for i in range(n):
        p = d.prims[d.prim_order[i]]
        mat[i] = p.material
        is_tri[i] = p.type == 0
        if not is_tri[i]:
            continue
        t = d.tris[p.shape]
        if t.mesh_has_uv:
            for k in range(3):
                uv[i, k] = (d.uvs[2 * t.uv[k]], d.uvs[2 * t.uv[k] + 1])
        else:
            uv[i] = ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0))
    return mat, is_tri, uv


def _rho(scene, tables, hit):
    """First-hit reflectance of every hit (rrt.h, rrt_render_aov): the material's own parameter, a textured one evaluated at the hit with zero
    differentials, clamped to >= 0 where the material clamps."""
    d = scene.desc
    mat_of, is_tri, uvs = tables
    prim, b1, b2, p = hit["prim"], hit["u"], hit["v"], hit["p"]
    n = len(prim)
    rho = np.zeros((n, 3))
    mats = mat_of[prim]
    uv = (uvs[prim, 0] * (1.0 - b1 - b2)[:, None] + uvs[prim, 1] * b1[:, None]) + uvs[prim, 2] * b2[:, None]

    def param(m, slot, const, idx):
        if m.tex[slot] < 0:
            return np.broadcast_to(np.array(list(const), np.float64), (len(idx), 3))
        assert is_tri[prim[idx]].all(), "the reference evaluates textures on triangle hits only"
        return np.array([O.texture_eval(scene, m.tex[slot], p=p[i], uv=uv[i]) for i in idx])

    for mi in np.unique(mats):
        m = d.materials[mi]
        idx = np.nonzero(mats == mi)[0]
        if m.type in (MATTE, PLASTIC, TRANSLUCENT):
            v = np.maximum(param(m, P_KD, m.kd, idx), 0.0)
        elif m.type == MIRROR:
            v = np.maximum(param(m, P_KR, m.kr, idx), 0.0)
        elif m.type == GLASS:
            v = np.ones((len(idx), 3))
        elif m.type == METAL:
            eta, k = param(m, P_ETA, m.eta, idx), param(m, P_K, m.k, idx)
            v = ((eta - 1.0) ** 2 + k * k) / ((eta + 1.0) ** 2 + k * k)
        else:
            v = np.broadcast_to(np.array([0.0, 1.0, 1.0]), (len(idx), 3))
        rho[idx] = v
    return rho


def samples(scene, rect, rank=0, world=1, max_samples=0, flat=False):
    """The camera samples rrt_render_aov takes for `rect` (rank / world: its interleaved 16-row bands) as flat arrays:
    dict(p_film (n, 2), weight, live, hit, t, n (unit), rho) - hit, t, n, rho are meaningful where live."""
    d = scene.desc
    x0, y0, x1, y1 = rect
    nsamp = int(d.sampler.samples_per_pixel)
    s1 = nsamp if max_samples == 0 else min(nsamp, 1 + max_samples)
    ns = s1 - 1
    dims, rays, w = O.camera_samples(scene, rect, 1, s1)       # [pixel][sample], pixels row by row
    ys, xs = np.mgrid[y0:y1, x0:x1]
    px, py = np.repeat(xs.ravel(), ns), np.repeat(ys.ravel(), ns)
    keep = ((py - y0) // 16) % world == rank if world > 1 else np.ones(len(px), bool)
    px, py, dims, rays, w = px[keep], py[keep], dims[keep], rays[keep], w[keep]
    p_film = np.stack([px + dims[:, 0], py + dims[:, 1]], -1)
    live = w > 0
    n_all = len(w)
    hit = np.zeros(n_all, bool); t = np.zeros(n_all); nrm = np.zeros((n_all, 3)); rho = np.zeros((n_all, 3))
    li = np.nonzero(live)[0]
    if len(li):
        h = O.trace_closest(scene, rays[li, :3], rays[li, 3:], np.full(len(li), np.inf), want_geometry=True, flat=flat)
        hh = h["prim"] >= 0
        hi = li[hh]
        hit[hi] = True
        t[hi] = h["t"][hh]
        nn = h["n"][hh]
        nrm[hi] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
        rho[hi] = _rho(scene, _prim_tables(scene), {k: h[k][hh] for k in ("prim", "u", "v", "p")})
    return dict(p_film=p_film, px=px, py=py, weight=w, live=live, hit=hit, t=t, n=nrm, rho=rho)


def _splat(scene, s):
    """(pixel y, pixel x, sample index, filter weight) of every (live sample, film pixel) pair the film's filter joins."""
    f = scene.desc.film
    W, H = f.xres, f.yres
    li = np.nonzero(s["live"])[0]
    rx, ry = f.filter_radius[0], f.filter_radius[1]
    if f.filter_type == 0 and rx == 0.5 and ry == 0.5:       # the box filter of radius 0.5: weight 1 in the sample's own pixel
        return s["py"][li], s["px"][li], li, np.ones(len(li))
    table = np.array(list(f.filter_table)).reshape(16, 16)
    inv_rx, inv_ry = 1.0 / rx, 1.0 / ry
    dx, dy = s["p_film"][li, 0] - 0.5, s["p_film"][li, 1] - 0.5
    # FilmTile::add_sample film.rs:77-130: p0 = ceil(d - r), p1 = trunc(d + r) + 1, clipped to the film
    p0x, p0y = np.ceil(dx - rx), np.ceil(dy - ry)
    p1x, p1y = np.trunc(dx + rx) + 1.0, np.trunc(dy + ry) + 1.0
    reach_x, reach_y = int(np.ceil(rx + 0.5)), int(np.ceil(ry + 0.5))
    out = [[], [], [], []]
    for oy in range(-reach_y, reach_y + 1):
        for ox in range(-reach_x, reach_x + 1):
            x, y = s["px"][li] + ox, s["py"][li] + oy
            ok = (x >= p0x) & (x < p1x) & (y >= p0y) & (y < p1y) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            fx = np.abs((x - dx) * inv_rx * 16.0); fy = np.abs((y - dy) * inv_ry * 16.0)
            ifx = np.minimum(np.floor(fx), 15.0).astype(int); ify = np.minimum(np.floor(fy), 15.0).astype(int)
            fw = table[ify, ifx]
            out[0].append(y[ok]); out[1].append(x[ok]); out[2].append(li[ok]); out[3].append(fw[ok])
    return tuple(np.concatenate(a) for a in out)


def planes(scene, rect=None, rank=0, world=1, max_samples=0, flat=False, with_samples=False):
    """dict(albedo, normal, depth) as rrt_aov defines them ((H, W, 4) f64 each), + hit_weight: per pixel the sum of the CAMERA
    weights of the hit samples that land in it (what the Debug integrator's frame holds, times 0.1)."""
    W, H = scene.resolution
    rect = rect or (0, 0, W, H)
    s = samples(scene, rect, rank, world, max_samples, flat)
    y, x, i, fw = _splat(scene, s)
    alb, nrm, dep, hw = np.zeros((H, W, 4)), np.zeros((H, W, 4)), np.zeros((H, W, 4)), np.zeros((H, W))
    np.add.at(alb[..., 3], (y, x), fw)
    h = s["hit"][i]
    y, x, i, fw = y[h], x[h], i[h], fw[h]
    for c in range(3):
        np.add.at(alb[..., c], (y, x), fw * s["rho"][i, c])
        np.add.at(nrm[..., c], (y, x), fw * s["n"][i, c])
    np.add.at(nrm[..., 3], (y, x), fw)
    np.add.at(dep[..., 0], (y, x), fw * s["t"][i])
    np.add.at(dep[..., 1], (y, x), fw * s["t"][i] * s["t"][i])
    np.add.at(dep[..., 2], (y, x), fw)
    np.add.at(hw, (y, x), fw * s["weight"][i])
    out = dict(albedo=alb, normal=nrm, depth=dep, hit_weight=hw)
    if with_samples:
        out["samples"] = s
    return out
