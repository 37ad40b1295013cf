"""numpy reference (f64) of rrt_denoise (include/rrt.h): the edge-avoiding a-trous wavelet filter guided by the planes of rrt_render_aov, written from the
definition on the prototype, not from the kernels. Test infrastructure only (tests/test_denoise.py).

denoise(film, albedo, normal, depth, ...) takes the sums as rrt_render_rect / rrt_render_aov leave them, (H, W, 4) each, and returns the filtered film.
record_dtype=np.float32 rounds the per-pixel records (c, v, n, z, sd and d) to fp32 where the fp32 device mode stores them for the first time and goes on in
f64, so that a comparison with the fp32 device starts from the same records."""
import numpy as np

DEFAULTS = dict(iterations=5, demodulate=1, sigma_color=4.0, sigma_normal=32.0, sigma_depth=8.0)
B3 = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0])
K3 = np.array([1.0, 2.0, 1.0])


def xyz_to_rgb(xyz):
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return np.stack([3.240479 * x - 1.537150 * y - 0.498535 * z, -0.969256 * x + 1.875991 * y + 0.041556 * z, 0.055648 * x - 0.204043 * y + 1.057311 * z], -1)


def rgb_to_xyz(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return np.stack([0.412453 * r + 0.357580 * g + 0.180423 * b, 0.212671 * r + 0.715160 * g + 0.072169 * b, 0.019334 * r + 0.119193 * g + 0.950227 * b], -1)


def luminance(c):
    return 0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2]


def _shift(a, ox, oy, fill=0.0):
    """b[y, x] = a[y + oy, x + ox], `fill` where that is outside the frame"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys0, ys1 = max(0, -oy), min(H, H - oy)
    xs0, xs1 = max(0, -ox), min(W, W - ox)
    if ys0 < ys1 and xs0 < xs1:
        b[ys0:ys1, xs0:xs1] = a[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return b


def _round(a, dtype):
    return a if dtype is None else a.astype(dtype).astype(np.float64)


def prepare(film, albedo, normal, depth, demodulate=1, record_dtype=None):
    film, albedo, normal, depth = (np.asarray(a, np.float64) for a in (film, albedo, normal, depth))
    with np.errstate(all="ignore"):
        w = film[..., 3]
        data = w > 0
        rgb = xyz_to_rgb(film[..., :3] / w[..., None])
        w_live = albedo[..., 3]
        a = np.where((w_live != 0)[..., None], albedo[..., :3] / w_live[..., None], 0.0)
        w_hit = depth[..., 2]
        hit = w_hit > 0
        z = depth[..., 0] / w_hit
        sd = np.sqrt(np.maximum(0.0, depth[..., 1] / w_hit - z * z))
        length = np.sqrt((normal[..., :3] ** 2).sum(-1))
        n = np.where((length > 0)[..., None], normal[..., :3] / length[..., None], 0.0)
        d = np.maximum(a, 1e-3) if demodulate else np.ones_like(a)
        c = rgb / d
    c = np.where(data[..., None], c, 0.0)
    z = np.where(hit, z, -1.0)
    sd = np.where(hit, sd, 0.0)
    n = np.where(hit[..., None], n, 0.0)
    return dict(w=w, data=data, hit=hit, c=_round(c, record_dtype), n=_round(n, record_dtype), z=_round(z, record_dtype), sd=_round(sd, record_dtype),
                d=_round(d, record_dtype))


def _surface_weight(rec, ox, oy, sigma_normal):
    """(g(p, q), usable) for q = p + (ox, oy)"""
    usable = _shift(rec["data"], ox, oy, False)
    hit_q = _shift(rec["hit"], ox, oy, False)
    n_q = _shift(rec["n"], ox, oy)
    dot = np.maximum(0.0, (rec["n"] * n_q).sum(-1))
    g = np.where(rec["hit"] != hit_q, 0.0, np.where(rec["hit"], dot ** sigma_normal, 1.0))
    return g, usable, hit_q


def initial_variance(rec, sigma_normal):
    l = luminance(rec["c"])
    sg = np.zeros_like(l); s1 = np.zeros_like(l); s2 = np.zeros_like(l)
    for oy in range(-3, 4):
        for ox in range(-3, 4):
            g, usable, _ = _surface_weight(rec, ox, oy, sigma_normal)
            g = np.where(usable, g, 0.0)
            l_q = _shift(l, ox, oy)
            sg += g; s1 += g * l_q; s2 += g * l_q * l_q
    with np.errstate(all="ignore"):
        v = np.maximum(0.0, s2 / sg - (s1 / sg) ** 2)
    return np.where(sg > 0, v, 0.0)


def iteration(rec, c, v, step, sigma_color, sigma_normal, sigma_depth):
    data, hit, z, sd = rec["data"], rec["hit"], rec["z"], rec["sd"]
    l = luminance(c)
    # the variance, prefiltered over the 3 x 3 neighbourhood
    sk = np.zeros_like(l); sv = np.zeros_like(l)
    for oy in range(-1, 2):
        for ox in range(-1, 2):
            g, usable, _ = _surface_weight(rec, ox, oy, sigma_normal)
            kg = np.where(usable, K3[oy + 1] * K3[ox + 1] * g, 0.0)
            sk += kg; sv += kg * _shift(v, ox, oy)
    with np.errstate(all="ignore"):
        gv = np.where(sk > 0, sv / sk, v)
    sw = np.zeros_like(l); sc = np.zeros_like(c); sv2 = np.zeros_like(l)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ox, oy = step * dx, step * dy
            hh = B3[dy + 2] * B3[dx + 2]
            if dx == 0 and dy == 0:
                wgt = np.full_like(l, hh)
            else:
                g, usable, hit_q = _surface_weight(rec, ox, oy, sigma_normal)
                with np.errstate(all="ignore"):
                    w_z = np.where(hit & hit_q, np.exp(-np.abs(z - _shift(z, ox, oy)) / (sigma_depth * (max(abs(dx), abs(dy)) * step * sd + 1e-3 * z))), 1.0)
                    if sigma_color > 0:
                        w_l = np.exp(-np.abs(l - _shift(l, ox, oy)) / (sigma_color * np.sqrt(gv) + 1e-3 * np.abs(l) + 1e-30))
                    else:
                        w_l = 1.0
                    wgt = np.where(usable & (g > 0), hh * g * w_z * w_l, 0.0)
            sw += wgt
            sc += wgt[..., None] * _shift(c, ox, oy)
            sv2 += wgt * wgt * _shift(v, ox, oy)
    with np.errstate(all="ignore"):
        c_new = np.where(data[..., None], sc / sw[..., None], c)
        v_new = np.where(data, sv2 / (sw * sw), v)
    return c_new, v_new


def denoise(film, albedo, normal, depth, iterations=5, demodulate=1, sigma_color=4.0, sigma_normal=32.0, sigma_depth=8.0, record_dtype=None):
    film = np.asarray(film, np.float64)
    rec = prepare(film, albedo, normal, depth, demodulate, record_dtype)
    c = rec["c"]
    v = _round(np.where(rec["data"], initial_variance(rec, sigma_normal), 0.0), record_dtype)
    for i in range(iterations):
        c, v = iteration(rec, c, v, 1 << i, sigma_color, sigma_normal, sigma_depth)
    out = film.copy()
    xyz = rgb_to_xyz(c * rec["d"]) * rec["w"][..., None]
    out[..., :3] = np.where(rec["data"][..., None], xyz, film[..., :3])
    return out


def synthetic(W, H, seed, spp=8):
    """Film and planes as the render calls leave them (f64 sums): three planar regions with normals 90 degrees apart that vary smoothly by < 5 degrees
    inside a region, depth ramps with a consistent sum t^2, gamma-distributed radiance noise over a per-region albedo and irradiance, a block of pixels
    without weight, a block without hits, and a band of partly covered pixels (0 < w_hit < w_live). Film weight = 3 x the sample count (Q3)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    region = np.where(xs < 0.45 * W + 0.2 * ys, 0, np.where(ys < 0.55 * H - 0.1 * xs, 1, 2))
    base = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])[region]
    tilt = 0.03 * np.stack([np.sin(xs / 7.0), np.cos(ys / 5.0), np.sin((xs + ys) / 9.0)], -1)       # < 0.052 rad off the region's axis
    n = base + tilt
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    z = np.array([6.0, 9.0, 14.0])[region] + np.array([0.02, -0.03, 0.05])[region] * xs + np.array([0.01, 0.04, -0.02])[region] * ys
    sd = 0.02 * z / 10.0
    rho = np.array([[0.7, 0.6, 0.5], [0.2, 0.5, 0.8], [0.9, 0.9, 0.1]])[region] * (1.0 + 0.2 * np.sin(xs / 3.0)[..., None])
    irr = np.array([0.8, 2.5, 0.3])[region] * (1.0 + 0.3 * np.cos(ys / 11.0))
    noise = rng.gamma(shape=2.0, scale=0.5, size=(H, W, 3))
    rgb = rho * irr[..., None] * noise
    w_live = np.full((H, W), float(spp))
    w_hit = w_live.copy()
    hole = (slice(H // 5, H // 5 + max(2, H // 6)), slice(W // 6, W // 6 + max(2, W // 5)))             # no weight at all
    sky = (slice(H // 2, H // 2 + max(2, H // 4)), slice(W // 2, W // 2 + max(2, W // 4)))              # live samples, none hits
    w_hit[sky] = 0.0
    band = (slice(max(0, H // 2 - 2), H // 2), slice(W // 2, W // 2 + max(2, W // 4)))                  # partly covered
    w_hit[band] = np.floor(spp / 2.0)
    rgb[sky] = 0.05 * noise[sky]
    film = np.zeros((H, W, 4)); albedo = np.zeros((H, W, 4)); normal = np.zeros((H, W, 4)); depth = np.zeros((H, W, 4))
    film[..., 3] = 3.0 * w_live
    film[..., :3] = rgb_to_xyz(rgb) * film[..., 3:4]
    albedo[..., :3] = rho * w_hit[..., None]
    albedo[..., 3] = w_live
    normal[..., :3] = n * w_hit[..., None]
    normal[..., 3] = w_hit
    depth[..., 0] = z * w_hit
    depth[..., 1] = (z * z + sd * sd) * w_hit
    depth[..., 2] = w_hit
    for a in (film, albedo, normal, depth):
        a[hole] = 0.0
    return film, dict(albedo=albedo, normal=normal, depth=depth)
