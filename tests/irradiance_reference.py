"""The numpy side of test_irradiance.py (f64): the scenes, the points, and rrt_irradiance's definition restated.

Draw j of point i (include/rrt.h): u = the first two sampler values of sample j of the point's pixel (the oracle's camera_samples dims5[0:2]), nn = n / |n|,
(s, t) = coordinate_system(nn) (geometry.rs:1146-1161), wl = cosine_sample_hemisphere(u) (sampling.rs:270-304, the concentric disk) or
uniform_sample_sphere(u) (sampling.rs:233-243), d = normalize(s wl.x + t wl.y + nn wl.z), o = p + nn * offset. A point with a zero or non-finite normal is
dead, and so is a cosine draw with wl.z == 0. The nine SH basis functions are rrt.h's, at the local direction wl.

The points of the integrator cases are first hits of the oracle's camera rays, with the geometric normal turned towards the camera, all rounded to fp32
once so that both precisions are given the same values. The closed-form scene is a 10 x 10 matte plane under one distant light.
"""
import copy
import os

import numpy as np

import oracle_lib as O
import passes_reference as PR
import texture_shapes as TS
from rs_ray_toy_amd import Scene

FILM = (24, 16)
NSAMP = 17                   # 16 draws
N_POINTS = 37                # a prime, less than a wave
DEAD, LONG, REPEAT = 5, 9, 11     # the point with a zero normal, the one with |n| = 3, the one that shares point 10's pixel
OFFSET = 1.0 / 1024.0        # exact in fp32

SH_C = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
Y_WEIGHTS = np.array([0.212671, 0.715160, 0.072169])

CASES = ("path", "direct", "texture")
_scenes = {}


def _config(workdir, name):
    wd = os.path.join(workdir, "irradiance_" + name)
    os.makedirs(wd, exist_ok=True)
    if name == "texture":
        cfg, root = TS.scene(wd, "shared")
        cfg = copy.deepcopy(cfg)
    elif name == "plane":
        return _plane_config(wd)
    else:
        cfg, root = PR.config(wd, "base")
        if name == "direct":
            cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 4}
        elif name == "ao":
            cfg["Integrator"] = {"integrator_type": "AO"}
        elif name == "stratified":
            cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 2, "jitter": True, "dimension": 4}
            return cfg, root
    cfg["Film"]["xres"], cfg["Film"]["yres"] = FILM
    cfg["Sampler"] = {"sampler_type": "HaltonSampler", "nsamp": NSAMP}
    return cfg, root


def scene(workdir, name):
    if name not in _scenes:
        cfg, root = _config(workdir, name)
        _scenes[name] = PR.load(cfg, root) if name != "texture" else Scene.loads(cfg, root)
    return _scenes[name]


def extent(sc):
    wb = np.ctypeslib.as_array(sc.desc.world_bound)
    return float(np.linalg.norm(wb[3:] - wb[:3]))


# ---- the closed-form scene ----------------------------------------------------------------------------------------------------------------------------
PLANE_KD = [0.6, 0.4, 0.2]
PLANE_L = [2.0, 2.5, 3.0]
PLANE_FROM = [0.3, 1.0, 0.2]
PLANE_CENTRE = (35.0, -1.0, 0.0)


def _plane_config(wd):
    from rs_ray_toy_amd import scenes
    cx, cy, cz = PLANE_CENTRE
    with open(os.path.join(wd, "plane.obj"), "w") as f:      # 10 x 10, normal +y (counter-clockwise seen from +y, as write_heightfield winds)
        for x, z in ((-5, -5), (5, -5), (5, 5), (-5, 5)):
            f.write(f"v {cx + x:.6f} {cy:.6f} {cz + z:.6f}\n")
        f.write("f 1 3 2\nf 1 4 3\n")
    cfg = scenes._base(FILM[0], FILM[1], NSAMP, {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 2})
    cfg["objs"] = [{"filename": "plane.obj", "obj_name": "plane"}]
    cfg["rgb_texture"] = [TS.cr("plane_kd", PLANE_KD)]
    cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_plane", "kd": "plane_kd"}]
    cfg["lights"] = [{"light_type": "distant", "l": {"values": PLANE_L}, "from": PLANE_FROM, "to": [0.0, 0.0, 0.0]}]
    cfg["Aggregate"]["primitives"] = [{"primitive_type": "triangle", "material_name": "m_plane", "obj_name": "plane"}]
    return cfg, wd


def plane_points():
    """Eight sensor points 0.01 above the plane, n towards it; dict(p, n, pixel)."""
    cx, cy, cz = PLANE_CENTRE
    xz = np.array([(-2.0, -2.0), (-1.0, 1.5), (0.0, 0.0), (0.5, -1.25), (1.0, 2.0), (2.0, -0.5), (-1.5, -0.75), (1.75, 1.0)])
    p = np.stack([cx + xz[:, 0], np.full(8, cy + 0.01), cz + xz[:, 1]], 1).astype(np.float32).astype(np.float64)
    n = np.tile(np.array([0.0, -1.0, 0.0]), (8, 1))
    pixel = np.stack([np.arange(8) * 3, np.arange(8) * 2], 1)
    return dict(p=p, n=n, pixel=pixel)


def plane_irradiance():
    """Kd L cos(theta_light): pi / N x the sums of a sensor whose every draw hits the lit plane (each draw carries Kd / pi x L x cos)"""
    w = np.asarray(PLANE_FROM, np.float64)
    cos_l = (w / np.linalg.norm(w))[1]
    return np.asarray(PLANE_KD) * np.asarray(PLANE_L) * cos_l


# ---- the points of the integrator cases ------------------------------------------------------------------------------------------------------------------
_points = {}


def points(sc, key):
    """37 first hits of the oracle's camera rays (sample 1 of pixels spread over the film) with the geometric normal facing the camera; then point DEAD
    gets a zero normal, point LONG a normal of length 3, point REPEAT the pixel of the point before it. dict(p (m, 3), n (m, 3), pixel (m, 2))."""
    if key not in _points:
        W, H = sc.resolution
        dims, rays, w = O.camera_samples(sc, (0, 0, W, H), 1, 2)
        alive = np.flatnonzero(w > 0)
        hit = O.trace_closest(sc, rays[alive, :3], rays[alive, 3:], np.full(len(alive), np.inf), want_geometry=True)
        ok = np.flatnonzero(hit["prim"] >= 0)
        assert len(ok) >= N_POINTS, f"only {len(ok)} camera rays of sample 1 hit the scene"
        ok = ok[np.linspace(0, len(ok) - 1, N_POINTS).astype(int)]
        sel = alive[ok]                                                   # pixel-linear: sample 1 of every pixel
        n = hit["n"][ok]
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where((np.sum(n * rays[sel, 3:], 1) > 0)[:, None], -n, n)
        p = hit["p"][ok].astype(np.float32).astype(np.float64)
        n = n.astype(np.float32).astype(np.float64)
        n[DEAD] = 0.0
        n[LONG] = (3.0 * n[LONG]).astype(np.float32).astype(np.float64)
        pixel = np.stack([sel % W, sel // W], 1)
        pixel[REPEAT] = pixel[REPEAT - 1]
        for a in (p, n, pixel): a.setflags(write=False)
        _points[key] = dict(p=p, n=n, pixel=pixel)
    return _points[key]


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------------
def coordinate_system(v):
    """geometry.rs:1146-1161 on (m, 3)"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    zero = np.zeros_like(x)
    with np.errstate(all="ignore"):
        a = np.stack([-z, zero, x], 1) / np.sqrt(x * x + z * z)[:, None]
        b = np.stack([zero, z, -y], 1) / np.sqrt(y * y + z * z)[:, None]
    v2 = np.where((np.abs(x) > np.abs(y))[:, None], a, b)
    return v2, np.cross(v, v2)


def cosine_sample_hemisphere(u):
    """sampling.rs:270-304 (concentric_sample_disk :246-268) on (..., 2)"""
    ox, oy = 2.0 * u[..., 0] - 1.0, 2.0 * u[..., 1] - 1.0
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(all="ignore"):
        r = np.where(first, ox, oy)
        theta = np.where(first, (np.pi / 4) * (oy / ox), np.pi / 2 - (np.pi / 4) * (ox / oy))
    centre = (ox == 0) & (oy == 0)
    dx, dy = np.where(centre, 0.0, r * np.cos(theta)), np.where(centre, 0.0, r * np.sin(theta))
    return np.stack([dx, dy, np.sqrt(np.maximum(0.0, 1.0 - dx * dx - dy * dy))], -1)


def uniform_sample_sphere(u):
    """sampling.rs:233-243 on (..., 2)"""
    z = 1.0 - 2.0 * u[..., 0]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = 2.0 * np.pi * u[..., 1]
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def sh9(w):
    """(..., 9): the basis of rrt.h at unit vectors (..., 3)"""
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    c0, c1, c2, c3, c4 = SH_C
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3.0 * z * z - 1.0), c2 * x * z, c4 * (x * x - y * y)], -1)


_u = {}


def draw_u(sc, key, pixel, s0, s1):
    """(m, s1 - s0, 2): the oracle's first two sampler values of samples s0 .. s1-1 of each point's pixel"""
    out = np.zeros((len(pixel), s1 - s0, 2))
    for i, (x, y) in enumerate(np.asarray(pixel)):
        k = (key, int(x), int(y), s0, s1)
        if k not in _u:
            _u[k] = O.camera_samples(sc, (int(x), int(y), int(x) + 1, int(y) + 1), s0, s1)[0][:, :2].copy()
        out[i] = _u[k]
    return out


def rays(sc, key, pts, s0, s1, offset, mode):
    """dict(od (m, ns, 6) with dead draws zero, wl (m, ns, 3) local directions, live (m, ns))"""
    p, n = np.asarray(pts["p"], np.float64), pts["n"]
    m = len(p)
    n = np.tile(np.array([0.0, 0.0, 1.0]), (m, 1)) if n is None else np.asarray(n, np.float64)
    u = draw_u(sc, key, pts["pixel"], s0, s1)
    alive = np.isfinite(n).all(1) & (n != 0).any(1)
    with np.errstate(all="ignore"):
        nn = n / np.sqrt(np.sum(n * n, 1))[:, None]
    nn = np.where(alive[:, None], nn, np.array([0.0, 0.0, 1.0]))
    s, t = coordinate_system(nn)
    wl = cosine_sample_hemisphere(u) if mode == "cosine" else uniform_sample_sphere(u)
    d = (s[:, None, :] * wl[..., 0:1] + t[:, None, :] * wl[..., 1:2]) + nn[:, None, :] * wl[..., 2:3]
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to((p + nn * offset)[:, None, :], d.shape)
    live = alive[:, None] & ((wl[..., 2] != 0) if mode == "cosine" else np.ones(wl.shape[:-1], bool))
    od = np.where(live[..., None], np.concatenate([o, d], -1), 0.0)
    return dict(od=od, wl=wl, live=live)


def sums_in_order(L, dtype, start=None):
    """(m, 3): L (m, ns, 3) added in draw order in `dtype`, from `start` - what k_irr_reduce's plain adds leave"""
    L = np.asarray(L, dtype)
    acc = np.zeros((L.shape[0], 3), dtype) if start is None else np.array(start, dtype)
    for j in range(L.shape[1]):
        acc = (acc + L[:, j]).astype(dtype)
    return acc


def sum_y2(L):
    """(m,) f64: the sum of the squared luminances of L (m, ns, 3)"""
    y = np.asarray(L, np.float64) @ Y_WEIGHTS
    return np.sum(y * y, 1)


def sh_sums(L, wl):
    """(m, 27) f64: sum_j L_j.c Y_k(wl_j) at [3 k + c]"""
    Y = sh9(wl)                                                  # (m, ns, 9)
    return np.einsum("mjk,mjc->mkc", Y, np.asarray(L, np.float64)).reshape(len(Y), 27)
