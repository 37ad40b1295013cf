"""numpy references (f64) of rrt_render_moments and rrt_denoise_moments (include/rrt.h), written from the definitions on the prototypes, not from the
kernels. Test infrastructure only (tests/test_moments.py).

moments(): Halton sample k of a pixel does not depend on nsamp, so the oracle's frame of ONE pixel with nsamp = k + 1 minus the same with nsamp = k
is exactly the splat of sample k of that pixel onto the film: fw = dW / 3 per touched pixel (Q3), y = dY / fw where fw > 0. Nothing but the oracle's
own frame path is needed.

denoise(): denoise_reference's prepare, initial_variance and iteration with the sample-variance rule in between."""
import numpy as np

import denoise_reference as DR
import oracle_lib as O


def band_mask(H, rect, band):
    """rows of the frame that render_moments(rect, rank, world) takes: the rect's interleaved 16-row bands b % world == rank"""
    rows = np.zeros(H, bool)
    for y in range(rect[1], rect[3]):
        rows[y] = band is None or ((y - rect[1]) // 16) % band[1] == band[0]
    return rows


def moments(scene_factory, nsamp, rect=None, band=None):
    """scene_factory(n) -> the Scene with samples_per_pixel = n. -> dict(moments (H, W, 4) = {S1, S2, S0, S3}, film (H, W, 4) = the summed differences:
    what the frame path adds for the rect / band)"""
    scs = [scene_factory(n) for n in range(1, nsamp + 1)]     # scs[k]: samples 1 .. k
    W, H = scs[0].resolution
    rect = rect or (0, 0, W, H)
    rows = band_mask(H, rect, band)
    S = np.zeros((H, W, 4)); film = np.zeros((H, W, 4))
    for y in range(rect[1], rect[3]):
        if not rows[y]:
            continue
        for x in range(rect[0], rect[2]):
            prev = np.zeros((H, W, 4))
            for k in range(1, nsamp):
                cur = O.render(scs[k], (x, y, x + 1, y + 1), n_threads=1)
                d = cur - prev
                prev = cur
                fw = d[..., 3] / 3.0
                assert (fw >= 0).all()
                with np.errstate(all="ignore"):
                    lum = np.where(fw > 0, d[..., 1] / fw, 0.0)
                S[..., 0] += fw * lum; S[..., 1] += fw * lum * lum; S[..., 2] += fw; S[..., 3] += fw * fw
                film += d
    return dict(moments=S, film=film)


def sample_variance(rec, m):
    """(v, use): the rule of rrt_denoise_moments per pixel and where it applies"""
    m = np.asarray(m, np.float64)
    s1, s2, s0, s3 = m[..., 0], m[..., 1], m[..., 2], m[..., 3]
    l = DR.luminance(rec["c"])
    with np.errstate(all="ignore"):
        n_eff = np.where(s3 > 0, s0 * s0 / s3, 0.0)
        use = rec["data"] & (n_eff >= 2) & (s1 > 0)
        rel = np.maximum(0.0, (s2 / s1) * (s0 / s1) - 1.0)      # = S2 S0 / S1^2 - 1; S1^2 of a tiny S1 would underflow
        v = l * l * rel / (n_eff - 1.0)
    return np.where(use, v, 0.0), use


def denoise(film, albedo, normal, depth, moments, iterations=5, demodulate=1, sigma_color=4.0, sigma_normal=32.0, sigma_depth=8.0, record_dtype=None,
            variance="sample"):
    """variance="spatial" ignores the plane: denoise_reference.denoise through this function's own steps"""
    film = np.asarray(film, np.float64)
    rec = DR.prepare(film, albedo, normal, depth, demodulate, record_dtype)
    c = rec["c"]
    v = np.where(rec["data"], DR.initial_variance(rec, sigma_normal), 0.0)
    if variance == "sample":
        vs, use = sample_variance(rec, moments)
        v = np.where(use, vs, v)
    v = DR._round(v, record_dtype)
    for i in range(iterations):
        c, v = DR.iteration(rec, c, v, 1 << i, sigma_color, sigma_normal, sigma_depth)
    out = film.copy()
    xyz = DR.rgb_to_xyz(c * rec["d"]) * rec["w"][..., None]
    out[..., :3] = np.where(rec["data"][..., None], xyz, film[..., :3])
    return out


def synthetic_moments(film, seed, spp=8):
    """A plane for the film of denoise_reference.synthetic: S1 = the film's Y, S0 = S3 = spp, S2 from a gamma-distributed relative variance; a block
    with n_eff = 1.5, a block with S1 = 0 over data, and the film's hole left zero - every branch of the rule."""
    film = np.asarray(film, np.float64)
    H, W = film.shape[:2]
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W, 4))
    data = film[..., 3] > 0
    s1 = np.where(data, film[..., 1], 0.0)
    rel = rng.gamma(shape=2.0, scale=0.4, size=(H, W))      # S2 S0 / S1^2 - 1
    m[..., 0] = s1
    m[..., 2] = np.where(data, float(spp), 0.0)
    m[..., 3] = m[..., 2]
    with np.errstate(all="ignore"):
        m[..., 1] = np.where(data, (1.0 + rel) * s1 * s1 / float(spp), 0.0)
    few = (slice(H // 8, H // 8 + max(2, H // 7)), slice(W // 2 + 1, W // 2 + 1 + max(2, W // 6)))      # S0 = 3, S3 = 6: n_eff = 1.5
    m[few + (2,)] = np.where(data[few], 3.0, 0.0)
    m[few + (3,)] = np.where(data[few], 6.0, 0.0)
    black = (slice(2 * H // 3, 2 * H // 3 + max(2, H // 8)), slice(W // 10, W // 10 + max(2, W // 5)))    # every sample black: S1 = S2 = 0
    m[black + (0,)] = 0.0
    m[black + (1,)] = 0.0
    return m
