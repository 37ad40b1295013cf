"""Cameras other than the scene's RealisticCamera, as inputs of Renderer.render_rays: the rays are built on the host, the film
samples stay the frame's own (the first two of the five dimensions Renderer.camera_samples reports per sample)."""
import numpy as np


def rect_pixels(rect, ns):
    """(x, y) of every sample of a rect in the [pixel][sample] layout of rrt_camera_samples: (npix * ns, 2) int64."""
    x0, y0, x1, y1 = rect
    ys, xs = np.mgrid[y0:y1, x0:x1]
    return np.repeat(np.stack([xs.ravel(), ys.ravel()], 1), ns, axis=0)


def pinhole_rays(renderer, rect, s0, s1, eye, look, up, fov_deg):
    """An ideal pinhole at `eye` looking at `look`, vertical field of view `fov_deg`, image y pointing down as the film's does.
    Returns (rays (n, 6), weight (n,) = 1, p_film (n, 2)) for sample numbers [s0, s1) of the rect's pixels, in the renderer's precision:
    p_film = pixel + the frame's own film sample, so the pixel filter sees what it sees in a frame. No sample is dead."""
    W, H = renderer.scene.resolution
    dims, _, _ = renderer.camera_samples(rect, s0, s1)
    p_film = (rect_pixels(rect, s1 - s0) + dims[:, :2]).astype(renderer.dtype)
    eye = np.asarray(eye, np.float64)
    w = np.asarray(look, np.float64) - eye
    w /= np.linalg.norm(w)
    u = np.cross(w, np.asarray(up, np.float64))
    u /= np.linalg.norm(u)
    v = np.cross(w, u)                      # image down
    half_h = np.tan(np.radians(fov_deg) / 2.0)
    half_w = half_h * W / H
    sx = (2.0 * p_film[:, 0].astype(np.float64) / W - 1.0) * half_w
    sy = (2.0 * p_film[:, 1].astype(np.float64) / H - 1.0) * half_h
    d = w[None, :] + sx[:, None] * u[None, :] + sy[:, None] * v[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.broadcast_to(eye, d.shape), d], 1).astype(renderer.dtype)
    if renderer.dtype == np.float32:        # unit length in the precision the kernels read
        d32 = rays[:, 3:].astype(np.float64)
        rays[:, 3:] = (d32 / np.linalg.norm(d32, axis=1, keepdims=True)).astype(np.float32)
    return rays, np.ones(len(rays), renderer.dtype), p_film
