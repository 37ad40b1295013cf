"""numpy reference (f64) of rrt_render_ao (include/rrt.h): AOIntegrator::li (ao.rs:65-96) per camera sample, derived from the oracle alone.
oracle_camera_samples gives every sample's film point, ray and weight, oracle_trace_closest(want_geometry, flat) its first hit (t, primitive,
barycentrics, p, n), oracle_halton_index / oracle_halton_dim the draws' 2D values, oracle_trace_any(o = p, d, t_max = inf, flat) each
hemisphere ray's verdict and the margin of its closest decision. dpdu is restated here from the desc's vertices, uvs and transforms
(triangle.rs:268-293, sphere.rs:192-200, transform.rs:628-655). The splat is aov_reference._splat. Test infrastructure only (tests/test_ao.py)."""
import numpy as np

import aov_reference as AR
import oracle_lib as O

INV_PI = 0.31830988618379067154


def _xform(d, idx):
    return np.array(list(d.xforms[idx].m)).reshape(4, 4), np.array(list(d.xforms[idx].m_inv)).reshape(4, 4)


def _dpdu(scene, prim, p):
    """The interaction's geometric dpdu, in world space, of hits on prim_order entries `prim` at world points `p`."""
    d = scene.desc
    out = np.zeros((len(prim), 3))
    for k, (pi, pw) in enumerate(zip(prim, p)):
        pr = d.prims[d.prim_order[pi]]
        if pr.type == 0:
            t = d.tris[pr.shape]
            P = np.array([[d.positions[3 * t.v[j] + c] for c in range(3)] for j in range(3)])
            if t.mesh_has_uv == 1: uv = np.array([[d.uvs[2 * t.uv[j]], d.uvs[2 * t.uv[j] + 1]] for j in range(3)])
            elif t.mesh_has_uv == 2: uv = np.array([[d.uvs[0], d.uvs[1]]] * 3)
            else: uv = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])
            duv02, duv12 = uv[0] - uv[2], uv[1] - uv[2]
            dp02, dp12 = P[0] - P[2], P[1] - P[2]
            det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
            assert abs(det) >= 1e-8, "the reference scenes keep non-degenerate uvs"
            v = (dp02 * duv12[1] - dp12 * duv02[1]) * (1.0 / det)
        else:
            s = d.spheres[pr.shape]
            m, mi = _xform(d, s.xform)
            po = pw
            if pr.instance >= 0: po = _xform(d, pr.instance)[1][:3, :3] @ po + _xform(d, pr.instance)[1][:3, 3]
            ph = mi[:3, :3] @ po + mi[:3, 3]
            v = m[:3, :3] @ np.array([-s.phi_max * ph[1], s.phi_max * ph[0], 0.0])
        if pr.instance >= 0: v = _xform(d, pr.instance)[0][:3, :3] @ v
        out[k] = v
    return out


def _hemisphere(u, cos_sample):
    """(wi_local (n, 3), pdf (n,)) of sampling.rs:245-303 for the 2D values u (n, 2)."""
    if not cos_sample:
        z = u[:, 0]
        r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        phi = 2.0 * np.pi * u[:, 1]
        return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1), np.full(len(u), 1.0 / (2.0 * np.pi))
    ox, oy = u[:, 0] * 2.0 - 1.0, u[:, 1] * 2.0 - 1.0
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(all="ignore"):
        r = np.where(first, ox, oy)
        theta = np.where(first, (np.pi / 4) * (oy / ox), np.pi / 2 - (np.pi / 4) * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    dx, dy = np.where(zero, 0.0, np.cos(theta) * r), np.where(zero, 0.0, np.sin(theta) * r)
    z = np.sqrt(np.maximum(0.0, 1.0 - dx * dx - dy * dy))
    return np.stack([dx, dy, z], -1), np.abs(z) * INV_PI


def samples(scene, rect, rank=0, world=1, max_samples=0, n_samples=4, cos_sample=True):
    """The camera samples rrt_render_ao takes, as aov_reference.samples lists them, with per sample a (sum a_i), b (sum a_i d_i) and margin (the
    smallest any-hit margin of its draws; inf for misses), and the draws' rays themselves (ray_o, ray_d (n_hit, N, 3), free, a_i (n_hit, N), hit_index)."""
    d = scene.desc
    x0, y0, x1, y1 = rect
    nsamp = int(d.sampler.samples_per_pixel)
    s1 = nsamp if max_samples == 0 else min(nsamp, 1 + max_samples)
    ns = s1 - 1
    dims, rays, w = O.camera_samples(scene, rect, 1, s1)       # [pixel][sample], pixels row by row
    ys, xs = np.mgrid[y0:y1, x0:x1]
    px, py = np.repeat(xs.ravel(), ns), np.repeat(ys.ravel(), ns)
    snum = np.tile(np.arange(1, s1), (x1 - x0) * (y1 - y0))
    keep = ((py - y0) // 16) % world == rank if world > 1 else np.ones(len(px), bool)
    px, py, snum, dims, rays, w = px[keep], py[keep], snum[keep], dims[keep], rays[keep], w[keep]
    p_film = np.stack([px + dims[:, 0], py + dims[:, 1]], -1)
    live = w > 0
    n_all, N = len(w), int(n_samples)
    hit = np.zeros(n_all, bool); a = np.zeros(n_all); b = np.zeros((n_all, 3)); margin = np.full(n_all, np.inf)
    out = dict(p_film=p_film, px=px, py=py, weight=w, live=live, hit=hit, a=a, b=b, margin=margin)
    li = np.nonzero(live)[0]
    if not len(li): return out
    h = O.trace_closest(scene, rays[li, :3], rays[li, 3:], np.full(len(li), np.inf), want_geometry=True, flat=True)
    hh = h["prim"] >= 0
    hi = li[hh]
    hit[hi] = True
    if not len(hi): return out
    n_g, p, cam_d = h["n"][hh], h["p"][hh], rays[hi, 3:]
    n = np.where((np.einsum("ij,ij->i", n_g, -cam_d) < 0)[:, None], -n_g, n_g)     # faceforward(n_g, -ray.d)
    s = _dpdu(scene, h["prim"][hh], p)
    s = s / np.linalg.norm(s, axis=1, keepdims=True)
    t = np.cross(n_g, s)
    index = [O.halton_index(scene, int(x), int(y), int(k)) for x, y, k in zip(px[hi], py[hi], snum[hi])]
    u = np.array([[[O.halton_dim(scene, ix, 5 + 2 * i), O.halton_dim(scene, ix, 6 + 2 * i)] for i in range(N)] for ix in index])   # (n_hit, N, 2)
    wl, pdf = _hemisphere(u.reshape(-1, 2), cos_sample)
    wl, pdf = wl.reshape(len(hi), N, 3), pdf.reshape(len(hi), N)
    wi = (s[:, None, :] * wl[..., 0:1] + t[:, None, :] * wl[..., 1:2]) + n[:, None, :] * wl[..., 2:3]
    ok = pdf != 0                                                                  # ao.rs would form 0 / 0: the draw is dropped
    with np.errstate(all="ignore"):
        a_i = np.where(ok, np.einsum("ijk,ik->ij", wi, n) / (pdf * N), 0.0)
    length = np.linalg.norm(wi, axis=-1, keepdims=True)
    dirs = wi / np.where(length > 0, length, 1.0)
    ro = np.repeat(p[:, None, :], N, 1)
    v = O.trace_any(scene, ro.reshape(-1, 3), dirs.reshape(-1, 3), np.full(len(hi) * N, np.inf), flat=True)
    free = ~v["occluded"].reshape(len(hi), N) & ok
    for i in range(N):                                                             # summed in draw order
        a[hi] += np.where(free[:, i], a_i[:, i], 0.0)
        b[hi] += np.where(free[:, i, None], a_i[:, i, None] * dirs[:, i], 0.0)
    margin[hi] = np.where(ok, v["margin"].reshape(len(hi), N), np.inf).min(1)
    out.update(ray_o=ro, ray_d=dirs, free=free, a_i=a_i, ok=ok, hit_index=hi, prim=h["prim"][hh])
    return out


def planes_of(scene, s, a=None, b=None):
    """dict(ao, bent, risky) from the samples `s` (a / b: other per-sample sums in place of the reference's own): ao and bent as rrt_ao defines them
    ((H, W, 4) f64), risky (H, W) bool = the pixels that receive a sample one of whose draws has an any-hit margin below 1e-9."""
    W, H = scene.resolution
    a = s["a"] if a is None else a
    b = s["b"] if b is None else b
    y, x, i, fw = AR._splat(scene, s)
    ao, bent, risky = np.zeros((H, W, 4)), np.zeros((H, W, 4)), np.zeros((H, W), bool)
    np.add.at(ao[..., 3], (y, x), fw)
    h = s["hit"][i]
    y, x, i, fw = y[h], x[h], i[h], fw[h]
    np.add.at(ao[..., 0], (y, x), fw * a[i])
    np.add.at(ao[..., 1], (y, x), fw * a[i] * a[i])
    np.add.at(ao[..., 2], (y, x), fw)
    for c in range(3):
        np.add.at(bent[..., c], (y, x), fw * b[i, c])
    np.add.at(bent[..., 3], (y, x), fw)
    r = s["margin"][i] < 1e-9
    risky[y[r], x[r]] = True
    return dict(ao=ao, bent=bent, risky=risky)


def planes(scene, rect=None, rank=0, world=1, max_samples=0, n_samples=4, cos_sample=True, with_samples=False):
    W, H = scene.resolution
    s = samples(scene, rect or (0, 0, W, H), rank, world, max_samples, n_samples, cos_sample)
    out = planes_of(scene, s)
    if with_samples:
        out["samples"] = s
    return out
