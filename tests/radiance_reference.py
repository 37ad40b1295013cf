"""The numpy side of test_radiance.py: the scenes, the handle's own camera samples as inputs of rrt_render_rays / rrt_radiance, and the box film
restated from per-sample radiance.

film_from_radiance() is FilmTile::add_sample + merge_film_tile for the box filter of radius 0.5 (film.rs:77-130, 248-263): per pixel the sum of
w * L over its samples in sample order, converted with the RGB-to-XYZ table of passes_reference.py, and 3 of filter weight per sample, dead ones
included (Q2, Q3). It is evaluated in f64 on the device's per-sample values; the device sums in its own precision, so the two differ by summation
order and the rounding of the conversion only.
"""
import copy
import os

import numpy as np

import passes_reference as PR
import texture_shapes as TS
from rs_ray_toy_amd import Scene
from rs_ray_toy_amd.cameras import rect_pixels

STRATIFIED = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 2, "jitter": True, "dimension": 4}
TEXTURE_CASE = "shared"      # UV leaf under Scale and Mix, DirectLighting: no node of the graph reads the footprint, the differential pools are live

# name -> (variant of passes_reference.config or None for the texture scene, edits of the scene document)
CASES = {
    "base": ("base", {}),
    "glass": ("glass", {}),
    "depth6": ("depth6", {}),
    "gauss": ("gauss", {}),
    "direct_all": ("base", {"Integrator": {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 4}}),
    "debug": ("base", {"Integrator": {"integrator_type": "Debug", "max_depth": 4}}),
    "stratified": ("base", {"Sampler": STRATIFIED}),
    "texture": (None, {}),
}
BOX_CASES = [k for k in CASES if k != "gauss"]

_scenes = {}


def scene(workdir, name):
    if name not in _scenes:
        variant, edits = CASES[name]
        wd = os.path.join(workdir, "radiance_" + name)
        os.makedirs(wd, exist_ok=True)
        if variant is None:
            _scenes[name] = Scene.loads(*TS.scene(wd, TEXTURE_CASE))
        else:
            cfg, root = PR.config(wd, variant)
            cfg.update(copy.deepcopy(edits))
            _scenes[name] = PR.load(cfg, root)
    return _scenes[name]


def nsamp(sc):
    return int(sc.desc.sampler.samples_per_pixel)


def full_rect(sc):
    W, H = sc.resolution
    return (0, 0, W, H)


def own_samples(r, rect=None):
    """The handle's own camera samples of the frame's sample numbers 1 .. nsamp-1, as inputs of render_rays and radiance:
    dict(rays (n, 6), weight (n,), p_film (n, 2), pixel (n, 2), sample_num (n,)) in the handle's precision, layout [pixel][sample]."""
    sc = r.scene
    rect = rect or full_rect(sc)
    ns = nsamp(sc) - 1
    dims, rays, w = r.camera_samples(rect, 1, ns + 1)
    pix = rect_pixels(rect, ns)
    p_film = pix.astype(r.dtype) + dims[:, :2].astype(r.dtype)      # k_raygen: (R)px + to_real<R>(d0)
    return dict(rays=rays.astype(r.dtype), weight=w.astype(r.dtype), p_film=p_film, pixel=pix, sample_num=np.tile(np.arange(1, ns + 1), len(pix) // ns))


def film_from_radiance(L, w, pixel, resolution):
    """(H, W, 4) f64 film of the box filter from per-sample radiance L (n, 3), weights w (n,) and pixels (n, 2), samples of a pixel in sample order."""
    W, H = resolution
    rgb = np.zeros((H, W, 3))
    wsum = np.zeros((H, W))
    L = np.asarray(L, np.float64) * np.asarray(w, np.float64)[:, None]
    for k in range(len(L)):      # in order: a pixel's samples are added one by one
        x, y = pixel[k]
        rgb[y, x] += L[k]
        wsum[y, x] += 3.0
    film = np.zeros((H, W, 4))
    film[..., :3] = rgb @ PR.RGB_TO_XYZ.T
    film[..., 3] = wsum
    return film
