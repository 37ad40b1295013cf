"""Oracle frames for the passes of rrt_render_passes (include/rrt.h), from two identities of the unchanged f64 oracle.

Lights.  estimate_direct draws the same sampler dimensions whatever the light's spectrum is; a black `li` only skips the shadow ray
         (integrator/mod.rs:403-558). So the oracle frame of the same scene with every other light's spectrum set to 0 is the pass of the lights that
         stayed, and a scene whose spectra are scaled by gains is the relit frame.
Bounces. NEE at path vertex b uses sampler dimensions and Russian-roulette decisions that do not depend on max_depth, and emission is 0 (Q18). So
         oracle(max_depth = hi) - oracle(max_depth = lo) is the sum of the NEE terms at vertices lo .. hi - 1, and oracle(max_depth = 0) is black.

A pass (groups, lo, hi) of a scene of depth D is therefore
    O.render(spectra of the lights outside the groups set to 0, max_depth = min(hi, D)) - O.render(same, max_depth = lo),
the second term 0 for lo = 0 and hi <= 0 read as D. A distant light's spectrum key is `l`, every other light's `spectrum`.

The test scene (config()) is cfg4's heightfield at n = 32 under four lights of four kinds - a point light, two distant lights and a sphere area light -
at 24 x 16 (whole 8 x 8 tiles: the tiled camera path runs), nsamp 5, depth 4; VARIANTS changes one thing at a time.
"""
import copy

import numpy as np

import oracle_lib as O
from rs_ray_toy_amd import RRT_FIXED_BVH, Scene, scenes

RGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])      # spectrum.rs:2084-2090

GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}      # test_frame_shapes.py's

LIGHTS = [
    {"light_type": "point", "world_pos": [25.66, 8.69, 4.00], "spectrum": {"values": [800, 700, 600]}},
    {"light_type": "distant", "l": {"values": [2.0, 2.5, 3.0]}, "from": [0.3, 1.0, 0.2], "to": [0.0, 0.0, 0.0]},
    {"light_type": "distant", "l": {"values": [3.0, 1.0, 0.5]}, "from": [-0.5, 1.0, -0.4], "to": [0.0, 0.0, 0.0]},
    {"light_type": "diffuse", "spectrum": {"values": [40, 40, 40]}, "light_shape": {"shape_type": "sphere", "radius": 1.0, "world_pos": [33.0, 6.0, 2.0]}},
]

# name -> (film, depth, filter, extra geometry)
VARIANTS = {
    "base": ((24, 16), 4, None, None),
    # Russian roulette draws at vertices > 3. Under the open sky no path of this film gets that far (the oracle's depth-5 and depth-6 frames equal its
    # depth-4 frame), so this variant stands inside cfg3's matte box: vertices 4 and 5 then add 0.022 and 0.011 of the frame's largest value
    "depth6": ((24, 16), 6, None, "box"),
    "glass": ((24, 16), 4, None, "glass"),         # specular vertices: they count and have no NEE term (16 pixels see the wall)
    "gauss": ((24, 16), 4, GAUSS, None),
    "wide": ((128, 40), 4, None, None),            # bands of 16 rows with world 3: 16 + 8, 16, 8 rows
}


def _glass_wall(cfg, workdir):
    """cfg2's cube at its first instance, the wall x = +1 as GlassMaterial (smooth: FresnelSpecular), the other five faces matte."""
    import os
    v = [l for l in scenes.CUBE_OBJ.splitlines() if l.startswith("v ")]
    faces = [l for l in scenes.CUBE_OBJ.splitlines() if l.startswith("f ")]
    on_wall = lambda f: all(float(v[int(t.split("/")[0]) - 1].split()[1]) > 0 for t in f.split()[1:])
    for name, keep in (("cube_wall.obj", True), ("cube_rest.obj", False)):
        with open(os.path.join(workdir, name), "w") as f:
            f.write("\n".join(v + [re_f(l) for l in faces if on_wall(l) == keep]) + "\n")
    cfg["objs"] += [{"filename": "cube_wall.obj", "obj_name": "cube_wall"}, {"filename": "cube_rest.obj", "obj_name": "cube_rest"}]
    cfg["rgb_texture"] += [{"texture_type": "BilerpTexture", "texture_name": f"gl_{k}", "v00": {"values": val}, "v01": {"values": val}}
                           for k, val in (("kr", [1.0, 1.0, 1.0]), ("kt", [0.9, 0.9, 0.9]))]
    cfg["float_texture"] += [{"texture_type": "BilerpTexture", "texture_name": "gl_eta", "v00": 1.5, "v01": 1.5}]
    cfg["materials"].append({"material_type": "GlassMaterial", "material_name": "gl", "kr": "gl_kr", "kt": "gl_kt", "eta": "gl_eta"})
    inst = [copy.deepcopy(scenes.SCENE_JSON_INSTANCES[0])]
    cfg["Aggregate"]["primitives"] += [
        {"primitive_type": "triangle", "material_name": "gl", "obj_name": "cube_wall", "instances": copy.deepcopy(inst)},
        {"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "cube_rest", "instances": copy.deepcopy(inst)},
    ]


def re_f(line):
    """A face line without its normal indices (the part files carry no vn lines)."""
    return "f " + " ".join(t.split("/")[0] for t in line.split()[1:])


def config(workdir, variant="base"):
    """(cfg, root) of a variant: a scene.json document the tests may edit further."""
    (W, H), depth, filt, extra = VARIANTS[variant]
    cfg, root = scenes.cfg4(workdir, xres=W, yres=H, nsamp=5, max_depth=depth, n=32)
    cfg["lights"] = copy.deepcopy(LIGHTS)
    if filt: cfg["Film"]["Filter"] = dict(filt)
    if extra == "glass": _glass_wall(cfg, workdir)
    if extra == "box":
        scenes.write_box(workdir, center=(35.0, 0.0, 0.0), half=(40.0, 20.0, 40.0))
        cfg["objs"].append({"filename": "box.obj", "obj_name": "box_01"})
        cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "box_01"})
    return cfg, root


def spectrum_key(light):
    return "l" if light["light_type"] == "distant" else "spectrum"


def edited(cfg, gains=None, max_depth=None):
    """A copy of cfg with light i's spectrum scaled by gains[i] (a number or an RGB triple; None: unchanged) and the integrator's depth replaced."""
    out = copy.deepcopy(cfg)
    if gains is not None:
        assert len(gains) == len(out["lights"])
        for light, g in zip(out["lights"], gains):
            sp = light[spectrum_key(light)]
            sp["values"] = [float(x) for x in np.asarray(sp["values"], np.float64) * np.broadcast_to(np.asarray(g, np.float64), (3,))]
    if max_depth is not None: out["Integrator"]["max_depth"] = int(max_depth)
    return out


def load(cfg, root):
    return Scene.loads(cfg, root, flags=RRT_FIXED_BVH)


def oracle_frame(cfg, root, gains=None, max_depth=None, rect=None):
    """One thread: the oracle merges its tiles in the order its threads finish, and under a wide filter the weight sums of two runs then differ in
    the last bit - the frames here are compared with each other, weight channels included."""
    return O.render(load(edited(cfg, gains, max_depth), root), rect, n_threads=1)


def pass_frame(cfg, root, groups, lo=0, hi=0, light_group=None, rect=None):
    """The oracle's frame of one pass (module docstring); light_group None: light i is in group min(i, 31)."""
    D = int(cfg["Integrator"]["max_depth"])
    n = len(cfg["lights"])
    lg = [min(i, 31) for i in range(n)] if light_group is None else list(light_group)
    keep = [1.0 if (groups >> lg[i]) & 1 else 0.0 for i in range(n)]
    top = D if hi <= 0 else min(hi, D)
    if top <= lo:      # an empty vertex range: the frame's weights, no colour
        out = oracle_frame(cfg, root, keep, 0, rect)
        assert not out[..., :3].any()
        return out
    out = oracle_frame(cfg, root, keep, top, rect)
    if lo > 0:
        low = oracle_frame(cfg, root, keep, lo, rect)
        assert np.array_equal(out[..., 3], low[..., 3])
        out[..., :3] -= low[..., :3]
    return out


def combine(films, gains):
    """rrt_combine_passes restated: out[:3] = sum_k rgb_to_xyz(gains[k] * xyz_to_rgb(films[k][:3])) in f64, the operations in the kernel's order;
    out[3] = films[0][3]. rgb_to_xyz is the table the films were merged with (spectrum.rs:2084-2090), xyz_to_rgb its inverse in f64 (rrt.h)."""
    to_rgb = np.linalg.inv(RGB_TO_XYZ)
    out = np.zeros(films[0].shape, np.float64)
    g_all = np.asarray(gains, np.float64)
    if g_all.ndim == 1: g_all = g_all[:, None]
    for f, g in zip(films, np.broadcast_to(g_all, (len(films), 3))):
        x, y, z = (f[..., c].astype(np.float64) for c in range(3))
        r = (to_rgb[0, 0] * x + to_rgb[0, 1] * y + to_rgb[0, 2] * z) * g[0]
        gg = (to_rgb[1, 0] * x + to_rgb[1, 1] * y + to_rgb[1, 2] * z) * g[1]
        b = (to_rgb[2, 0] * x + to_rgb[2, 1] * y + to_rgb[2, 2] * z) * g[2]
        out[..., 0] += 0.412453 * r + 0.357580 * gg + 0.180423 * b
        out[..., 1] += 0.212671 * r + 0.715160 * gg + 0.072169 * b
        out[..., 2] += 0.019334 * r + 0.119193 * gg + 0.950227 * b
    out[..., 3] = films[0][..., 3]
    return out
