"""numpy reference (f64) of rrt_render_aov_follow (include/rrt.h): the feature buffers of the first non-specular surface along the chain of
perfectly specular bounces a camera ray starts. Built on aov_reference.py from the oracle alone: oracle_camera_samples gives the camera rays,
oracle_trace_closest(want_geometry) every segment's hit (t, primitive, barycentrics, p, geometric n - which is the shading normal on meshes
without vertex normals, the only specular surfaces of the test scenes), oracle_texture_eval any textured parameter at the hit with zero
differentials, and the desc holds the materials. Test infrastructure only (tests/test_aov_follow*.py)."""
import numpy as np

import aov_reference as AR
import oracle_lib as O

P_KR, P_UROUGH, P_VROUGH, P_KT, P_INDEX = 2, 7, 8, 9, 12      # rrt_material::tex slots the follow rules read


def reflect(d, sn):
    """d' = d - 2 (d . sn) sn, row by row"""
    return d - 2.0 * np.sum(d * sn, -1, keepdims=True) * sn


def refract(wo, n, eta):
    """refract() of reflection.rs:122-134, row by row: (exists, wt) for unit wo, the normal n on wo's side and the ratio eta = eta_i / eta_t"""
    cos_i = np.sum(n * wo, -1)
    sin2_i = np.maximum(0.0, 1.0 - cos_i * cos_i)
    sin2_t = eta * eta * sin2_i
    ok = sin2_t < 1.0
    cos_t = np.sqrt(np.where(ok, 1.0 - sin2_t, 0.0))
    wt = -wo * eta[:, None] + n * (eta * cos_i - cos_t)[:, None]
    return ok, wt


def glass_direction(d, sn, index):
    """The refracted continuation of the rule for smooth Glass: wo = -d, entering = wo . sn > 0, ratio 1 / index entering and index leaving, the
    normal turned towards wo -> (exists, d', entering)."""
    wo = -d
    entering = np.sum(wo * sn, -1) > 0
    ratio = np.where(entering, 1.0 / index, index)
    nf = np.where(entering[:, None], sn, -sn)
    ok, wt = refract(wo, nf, ratio)
    return ok, wt, entering


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _param(scene, tables, m, slot, const, hit, idx, scalar=False):
    """A material parameter at the hits `idx`: its constant, or its texture at the hit with zero differentials"""
    _, is_tri, uvs = tables
    if m.tex[slot] < 0:
        c = np.array([const] if scalar else list(const), np.float64)
        return np.broadcast_to(c, (len(idx), len(c))).copy()
    prim, b1, b2, p = hit["prim"][idx], hit["u"][idx], hit["v"][idx], hit["p"][idx]
    assert is_tri[prim].all(), "the reference evaluates textures on triangle hits only"
    uv = (uvs[prim, 0] * (1.0 - b1 - b2)[:, None] + uvs[prim, 1] * b1[:, None]) + uvs[prim, 2] * b2[:, None]
    v = np.array([O.texture_eval(scene, m.tex[slot], p=p[i], uv=uv[i]) for i in range(len(idx))]).reshape(len(idx), 3)
    return v[:, :1] if scalar else v


def follow_rules(scene, tables, hit, d):
    """The rules of the prototype at every hit of one level: (follow, d' (unit), tint, event) with event in
    '' (not followed), 'mirror', 'enter', 'leave', 'tir' (glass reflecting for want of a refracted direction), 'glass_reflect' (Kt black)."""
    n = len(hit["prim"])
    follow = np.zeros(n, bool); dn = np.zeros((n, 3)); tint = np.ones((n, 3)); event = np.full(n, "", dtype=object)
    mat_of = tables[0]
    mats = mat_of[hit["prim"]]
    sn = _normalize(hit["n"])
    for mi in np.unique(mats):
        m = scene.desc.materials[mi]
        idx = np.nonzero(mats == mi)[0]
        if m.type not in (AR.MIRROR, AR.GLASS):
            continue
        kr = np.maximum(_param(scene, tables, m, P_KR, m.kr, hit, idx), 0.0)
        refl_ok = np.any(kr != 0.0, -1)
        d_refl = reflect(d[idx], sn[idx])
        if m.type == AR.MIRROR:
            follow[idx] = refl_ok; dn[idx] = d_refl; tint[idx] = kr
            event[idx[refl_ok]] = "mirror"
            continue
        ur = _param(scene, tables, m, P_UROUGH, m.u_roughness, hit, idx, scalar=True)[:, 0]
        vr = _param(scene, tables, m, P_VROUGH, m.v_roughness, hit, idx, scalar=True)[:, 0]
        smooth = (ur == 0.0) & (vr == 0.0)
        kt = np.maximum(_param(scene, tables, m, P_KT, m.kt, hit, idx), 0.0)
        index = _param(scene, tables, m, P_INDEX, m.index, hit, idx, scalar=True)[:, 0]
        exists, wt, entering = glass_direction(d[idx], sn[idx], index)
        through = smooth & exists & np.any(kt != 0.0, -1)
        back = smooth & ~through & refl_ok
        follow[idx] = through | back
        dn[idx] = np.where(through[:, None], wt, d_refl)
        tint[idx] = np.where(through[:, None], kt, kr)
        event[idx[through & entering]] = "enter"
        event[idx[through & ~entering]] = "leave"
        event[idx[back & ~exists]] = "tir"
        event[idx[back & exists]] = "glass_reflect"
    dn[follow] = _normalize(dn[follow])
    return follow, dn, tint, event


def chain(scene, o, d, max_follow, flat=False):
    """The chains of the rays (o, d): dict(hit, rho (= thr * rho of the last surface), n, t (= path length T), levels (surfaces on the chain),
    end ('miss0' a miss of the first segment, 'surface' the last surface is not followed, 'miss' a later segment missed, 'exhausted' the last
    surface would be followed but max_follow is used up), events (per ray, the list of follow events), segments (rays traced in all))."""
    n = len(o)
    tables = AR._prim_tables(scene)
    hit = np.zeros(n, bool); rho = np.zeros((n, 3)); nrm = np.zeros((n, 3)); T = np.zeros(n)
    thr = np.ones((n, 3)); levels = np.zeros(n, int)
    end = np.full(n, "miss0", dtype=object)
    events = [[] for _ in range(n)]
    act = np.arange(n)
    o, d = np.array(o, np.float64), np.array(d, np.float64)
    segments = 0
    for k in range(max_follow + 1):
        if len(act) == 0:
            break
        segments += len(act)
        h = O.trace_closest(scene, o[act], d[act], np.full(len(act), np.inf), want_geometry=True, flat=flat)
        hh = h["prim"] >= 0
        if k > 0:
            end[act[~hh]] = "miss"
        hi = act[hh]
        hsub = {key: h[key][hh] for key in ("prim", "u", "v", "p", "n", "t")}
        if len(hi) == 0:
            break
        hit[hi] = True
        T[hi] += hsub["t"]
        nrm[hi] = _normalize(hsub["n"])
        rho[hi] = thr[hi] * AR._rho(scene, tables, hsub)
        levels[hi] += 1
        follow, dn, tint, event = follow_rules(scene, tables, hsub, d[hi])
        end[hi] = np.where(follow, "exhausted", "surface")
        if k == max_follow:
            break
        fi = hi[follow]
        for i, e in zip(fi, event[follow]):
            events[i].append(e)
        thr[fi] *= tint[follow]
        o[fi] = hsub["p"][follow]       # spawn_ray applies no offset (Q8)
        d[fi] = dn[follow]
        act = fi
    return dict(hit=hit, rho=rho, n=nrm, t=T, levels=levels, end=end, events=events, segments=segments)


def samples(scene, rect, max_follow, rank=0, world=1, max_samples=0, flat=False):
    """aov_reference.samples with the chain's final record in hit, t, n, rho; + end, levels, events per sample ('' / 0 / [] where not live)"""
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
    end = np.full(n_all, "", dtype=object); levels = np.zeros(n_all, int); events = [[] for _ in range(n_all)]
    li = np.nonzero(live)[0]
    segments = 0
    if len(li):
        c = chain(scene, rays[li, :3], rays[li, 3:], max_follow, flat)
        hit[li], t[li], nrm[li], rho[li], end[li], levels[li] = c["hit"], c["t"], c["n"], c["rho"], c["end"], c["levels"]
        for i, e in zip(li, c["events"]):
            events[i] = e
        segments = c["segments"]
    return dict(p_film=p_film, px=px, py=py, weight=w, live=live, hit=hit, t=t, n=nrm, rho=rho, end=end, levels=levels, events=events,
                segments=segments)


def planes(scene, max_follow, rect=None, rank=0, world=1, max_samples=0, flat=False):
    """dict(albedo, normal, depth) as rrt_render_aov_follow defines them ((H, W, 4) f64 each) + samples: the per-sample chains"""
    W, H = scene.resolution
    rect = rect or (0, 0, W, H)
    s = samples(scene, rect, max_follow, rank, world, max_samples, flat)
    y, x, i, fw = AR._splat(scene, s)
    alb, nrm, dep = np.zeros((H, W, 4)), np.zeros((H, W, 4)), np.zeros((H, W, 4))
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
    return dict(albedo=alb, normal=nrm, depth=dep, samples=s)
