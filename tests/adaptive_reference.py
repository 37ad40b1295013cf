"""numpy references (f64) of rrt_tile_error and of the stopping rule of rrt_render_adaptive (include/rrt.h), written from the definitions on the
prototypes, not from the kernels. Test infrastructure only (tests/test_adaptive.py).

tile_error(): per pixel n_eff, m, v as the header states them; per 8 x 8 tile of the rect E = sqrt(V / 64) / (M / 64).
prefix_moments(): moments_reference.moments's per-sample differences of the oracle's one-pixel frames, with the running sums copied at the sample counts
asked for: Halton sample k of a pixel does not depend on nsamp, so the plane after k samples is the plane of a frame with nsamp = k + 1.
loop(): the rounds. It only needs `moments_at(k)`, the plane a k-sample frame leaves - the oracle's for the CPU tests, the device's own bit-equal
k-sample frames for the replay of the stopping rule."""
import numpy as np

import oracle_lib as O

TILE = 8


def tile_error(m, rect=None):
    """m (H, W, 4) = {S1, S2, S0, S3} -> (rh / 8, rw / 8) float64, tiles anchored at the rect's origin"""
    m = np.asarray(m, np.float64)
    H, W = m.shape[:2]
    x0, y0, x1, y1 = rect or (0, 0, W, H)
    assert (x1 - x0) % TILE == 0 and (y1 - y0) % TILE == 0
    m = m[y0:y1, x0:x1]
    s1, s2, s0, s3 = m[..., 0], m[..., 1], m[..., 2], m[..., 3]
    with np.errstate(all="ignore"):
        n_eff = np.where(s3 > 0, s0 * s0 / s3, 0.0)
        mean = np.where(s0 > 0, s1 / s0, 0.0)
        v = np.where(n_eff >= 2, np.maximum(0.0, s2 / s0 - mean * mean) / (n_eff - 1.0), 0.0)
        ty, tx = (y1 - y0) // TILE, (x1 - x0) // TILE
        tiles = lambda a: a.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)
        M, V = tiles(mean).sum(-1), tiles(v).sum(-1)
        return np.where(M > 0, np.sqrt(V / 64.0) / (np.where(M > 0, M, 1.0) / 64.0), 0.0)


def prefix_moments(scene_factory, ks, K):
    """scene_factory(n) -> the Scene with samples_per_pixel = n (box filter of radius 0.5). -> {k: (moments, film) after sample numbers 1 .. k} for k in ks,
    whole frame, from the oracle's one-pixel frames"""
    scs = [scene_factory(n) for n in range(1, K + 2)]     # scs[k]: samples 1 .. k
    W, H = scs[0].resolution
    S, film = np.zeros((K + 1, H, W, 4)), np.zeros((K + 1, H, W, 4))
    for y in range(H):
        for x in range(W):
            prev = np.zeros((H, W, 4))
            for k in range(1, K + 1):
                cur = O.render(scs[k], (x, y, x + 1, y + 1), n_threads=1)
                d = (cur - prev)[y, x]
                prev = cur
                fw = d[3] / 3.0
                assert fw == 1.0      # the box filter of radius 0.5: the sample's own pixel, weight 1 (Q3 triples it in the film)
                lum = d[1] / fw
                S[k, y, x] = S[k - 1, y, x] + np.array([fw * lum, fw * lum * lum, fw, fw * fw])
                film[k, y, x] = cur[y, x]
    return {k: (S[k], film[k]) for k in ks}


def loop(moments_at, rect, K, min_samples, batch, threshold):
    """-> (tile_samples (rh / 8, rw / 8) int, {k: E of the tiles active at checkpoint k, NaN elsewhere})"""
    k = min(min_samples, K)
    E = tile_error(moments_at(k), rect)
    active = np.ones(E.shape, bool)
    samples = np.zeros(E.shape, np.int64)
    seen = {}
    while True:
        E = tile_error(moments_at(k), rect)
        seen[k] = np.where(active, E, np.nan)
        stop = active & ((E < threshold) | (k == K))
        samples[stop] = k
        active &= ~stop
        if not active.any():
            return samples, seen
        k += min(batch, K - k)
