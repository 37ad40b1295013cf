"""First-hit feature buffers (rrt_render_aov, include/rrt.h): albedo, normal and depth planes beside the film.

CPU tests: the C layout of rrt_aov, the argument checks that need no device, and the numpy reference (tests/aov_reference.py) pinned to the
oracle's own frame path - a Debug frame without lights holds 0.1 x the camera weight of every sample that hits, so the pixels it lights are the
pixels the reference has hit weight in, with that value.

GPU tests, against that reference (built per scene from oracle_camera_samples, oracle_trace_closest(want_geometry), oracle_texture_eval with zero
differentials, the desc's materials and film.filter_table):
  test_f64_planes_match_reference     f64 device mode; the project's f64 bar: every value channel within 1e-9 of its plane's largest magnitude
                                      (depth: of its own channel's - sum t and sum t^2 have different units), box-filter weight channels equal
                                      exactly (integers), wide-filter weight channels equal support and rtol 1e-12.
  test_fp32_planes_close_to_reference the default fp32 mode, the fp32 frame bars of test_frame_shapes.py::test_default_fp32_frame_close_to_oracle per
                                      plane: >= 0.975 of the covered pixels within 1e-4, mean < 1e-4, max < 3e-2 x 256 / spp, live samples within 2e-5.
                                      One plane of one case has a bar of its own, measured and explained at SPHERE_NORMAL_SHARE below.
  test_parts_sum_to_the_whole, test_max_samples_is_a_shorter_scene, test_shortcuts_change_no_bit, test_frame_is_untouched,
  test_error_paths, test_resolve_aov, test_cli_writes_three_pngs.
The scenes are tie-free, as test_frame_shapes.py requires of its own: heightfields, and generic rotation axes for the cubes and the enclosure.
"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import aov_reference as AR
import oracle_lib as O
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, Scene, resolve_aov, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PLANES = ("albedo", "normal", "depth")
GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
ROT = {"rotation_axis": [1.0, 2.0, 0.5], "rotation_angle": 25.0}
SHORTCUTS = ("tile_trees", "tile_order", "quad_nodes", "lens_cull", "aux_margin")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_aov_struct_matches_c_layout(tmp_path):
    fields = [name for name, _ in A.Aov._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("size %zu\\n", sizeof(rrt_aov));']
    src += [f'printf("{f} %zu\\n", offsetof(rrt_aov, {f}));' for f in fields]
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", str(c), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert fields == ["mem", "precision", "albedo", "normal", "depth"]
    assert int(out["size"]) == C.sizeof(A.Aov)
    for f in fields:
        assert int(out[f]) == getattr(A.Aov, f).offset, f


def test_render_aov_refuses_null_arguments():
    """No device is needed to be told so: a NULL handle, a NULL rrt_aov, and an rrt_aov that asks for no plane are RRT_EINVAL, each with its own message."""
    lib = A.lib()
    plane = np.zeros(4, np.float32)
    rect = (C.c_int32 * 4)(0, 0, 1, 1)
    good = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, plane.ctypes.data, None, None)
    assert lib.rrt_render_aov(None, rect, 0, 1, 0, C.byref(good)) == A.RRT_EINVAL
    assert b"null handle" in lib.rrt_last_error()
    assert lib.rrt_render_aov(None, rect, 0, 1, 0, None) == A.RRT_EINVAL
    assert b"rrt_aov" in lib.rrt_last_error()
    empty = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, None, None, None)
    assert lib.rrt_render_aov(None, rect, 0, 1, 0, C.byref(empty)) == A.RRT_EINVAL
    assert b"no plane" in lib.rrt_last_error()
    assert np.all(plane == 0)


XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])


def test_reference_matches_the_oracles_debug_frame(workdir):
    """The reference builder against the oracle's frame path: under Integrator {Debug, max_depth 1} without lights a sample that hits adds 0.1 x its
    camera weight to each RGB channel and a sample that misses adds nothing, so the frame is the reference's hit-weight plane."""
    cfg, root = scenes.cfg5(workdir, xres=64, yres=48, nsamp=25, n=64)
    cfg["Integrator"] = {"integrator_type": "Debug", "max_depth": 1}
    cfg["lights"] = []
    sc = Scene.loads(cfg, root)
    ref = AR.planes(sc, with_samples=True)
    s = ref["samples"]
    assert 0.2 < s["live"].mean() < 0.5 and 0.1 < s["hit"][s["live"]].mean() < 0.9
    film = O.render(sc)
    lit = film[..., 1] > 0
    assert lit.any() and not lit.all()
    assert np.array_equal(lit, ref["depth"][..., 2] > 0)
    rgb = film[..., :3] @ np.linalg.inv(XYZ_FROM_RGB).T
    want = 0.1 * ref["hit_weight"]
    np.testing.assert_allclose(rgb[lit], np.repeat(want[lit][:, None], 3, 1), rtol=1e-12, atol=0)
    # both materials of the scene are in the albedo plane: the plastic's Kd and the metal's normal-incidence reflectance
    d = sc.desc
    kinds = {d.materials[m].type for m in AR._prim_tables(sc)[0]}
    assert kinds == {A.RRT_MAT_PLASTIC, A.RRT_MAT_METAL}
    assert len(np.unique(s["rho"][s["hit"]].round(9), axis=0)) == 2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

def _bands(world):
    return tuple(("band", k, world) for k in range(world))


def _cfg5(wd, film, nsamp):
    return scenes.cfg5(wd, xres=film[0], yres=film[1], nsamp=nsamp, max_depth=8, n=64)


def _cfg3_tilted(wd, nsamp=9):
    """cfg3 with the enclosure and the cube instanced under generic rotations (no exact box / face ties)."""
    cfg, root = scenes.cfg3(wd, xres=64, yres=64, nsamp=nsamp, max_depth=5)
    cfg["Aggregate"]["primitives"][0]["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
    cfg["Aggregate"]["primitives"][1]["instances"] = [{"world_pos": [0.0, 0.0, 0.0], "rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}]
    return cfg, root


def _const_rgb(name, v):
    return {"texture_name": name, "texture_type": "BilerpTexture", "v00": {"values": v}, "v01": {"values": v}}


def _textured(wd):
    """A uv checkerboard whose second child is Scale(UV, constant), Mix of that checkerboard and the UV texture on the instanced cube, and a 3D
    checkerboard (rotated, scaled world_to_texture) on the instanced enclosure: hard edges everywhere, evaluated with zero differentials."""
    cfg, root = _cfg3_tilted(wd)
    cube, box = cfg["Aggregate"]["primitives"]
    cfg["rgb_texture"] = [_const_rgb("w", [0.8, 0.8, 0.7]), _const_rgb("k", [0.15, 0.1, 0.3]),
                          {"texture_name": "uvt", "texture_type": "UVTexture", "mapping": {"mapping": "uv", "su": 2.0, "sv": 3.0}},
                          {"texture_name": "uvs", "texture_type": "ScaleTexture", "t1": "uvt", "t2": "w"},
                          {"texture_name": "chk", "texture_type": "CheckerBoardTexture", "t1": "w", "t2": "uvs",
                           "mapping": {"mapping": "uv", "su": 6.0, "sv": 6.0, "du": 0.0, "dv": 0.0}},
                          {"texture_name": "mixc", "texture_type": "MixTexture", "t1": "chk", "t2": "uvt"},
                          {"texture_name": "chk3", "texture_type": "CheckerBoardTexture", "dimension": 3, "t1": "w", "t2": "k", **ROT, "scale": [0.1, 0.1, 0.1]}]
    cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_box", "kd": "chk3"},
                                           {"material_type": "MirrorMaterial", "material_name": "m_cube", "kr": "mixc"}]
    cube["material_name"], box["material_name"] = "m_cube", "m_box"
    return cfg, root


def _scaled_instance(wd):
    cfg, root = _cfg3_tilted(wd)
    cfg["Aggregate"]["primitives"][0]["instances"][0]["scale"] = [1.5, 0.7, 1.2]       # non-rigid: the device keeps it, n comes back un-normalised
    return cfg, root


def _stratified(wd):
    cfg, root = _cfg5(wd, (48, 40), 5)
    cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 3, "ysamp": 4, "jitter": True, "dimension": 4}
    return cfg, root


def _case(build, parts=(None,), filt=None, max_paths=None, max_samples=0, flags=RRT_FIXED_BVH, fp32_share=None):
    """fp32_share: {plane: share of the covered pixels within 1e-4} where a plane cannot hold the frame's 0.975 (see SPHERE_NORMAL_SHARE)."""
    return dict(build=build, parts=tuple(parts), filt=filt, max_paths=max_paths, max_samples=max_samples, flags=flags, fp32_share=fp32_share or {})


# The one fp32 bar a plane could not hold: the NORMAL plane of config 1's spheres, 85.7 % of the covered pixels within 1e-4 against the bar's 97.5 %
# (mean 6.1e-5 and max 1.9e-3 hold their bars, albedo and depth hold all of theirs: 100 %, and the live and hit samples are the reference's exactly).
# No sample flips here - no silhouette or checker edge: every sphere sample is a little off. Sphere::intersect solves |o + t d|^2 = r^2 with the
# coefficients formed at the camera's distance D = 45 from spheres of radius r = 0.75 (sphere.rs:124-191, the device replays it operation by
# operation in the handle's format): b^2 and 4ac are both 4 D^2 = 8 000 and carry ~3 ulp each, so the discriminant 4 (r^2 - h^2) <= 2.25 (h: the
# ray's distance from the centre) is known to 6 x 2^-24 x 4 D^2 = 2.9e-3 only; t = (-b +- sqrt(disc)) / 2a moves by 2.9e-3 / (8 sqrt(r^2 - h^2)), the
# hit point p = o + t d (not re-projected on the first root, as in the reference) slides along the ray, and the normal p / r turns by that times
# h / r^2: averaged over the sphere's disc 2.9e-3 x (pi / 2) / (8 r^2) = 1.0e-3 per sample as a bound, a third of it with random rounding - over
# a pixel's two hit samples on average, relative to the plane's largest sum (4.8): about 1e-4, the bar itself. Depth does not show it (t is 45) and
# albedo does not read p. So this bar is set as the issue says for a plane that cannot hold one: from the measured share against the
# oracle-derived plane with a factor 2 on the share that misses: 1 - 2 x (1 - 0.857) = 0.714. DESIGN.md section 4 has both numbers.
SPHERE_NORMAL_SHARE = 1.0 - 2.0 * (1.0 - 0.857)


CASES = {
    "cfg5_whole": _case(lambda wd: _cfg5(wd, (64, 48), 25)),                                        # Plastic + Metal
    "rect_off_tile": _case(lambda wd: _cfg5(wd, (136, 104), 25), parts=[(5, 3, 101, 67)]),
    "bands_world3": _case(lambda wd: _cfg5(wd, (128, 104), 9), parts=_bands(3)),
    "gauss_rect_off": _case(lambda wd: _cfg5(wd, (136, 104), 9), parts=[(5, 3, 101, 67)], filt=GAUSS),   # halo outside the rect included
    "small_pools": _case(lambda wd: _cfg5(wd, (64, 48), 9), max_paths=1000),                        # four pixel groups x eight sample chunks
    "max_samples_8": _case(lambda wd: _cfg5(wd, (64, 48), 25), max_samples=8),
    "stratified": _case(_stratified),
    "textured_cfg3": _case(_textured, flags=0),
    "cfg1_spheres": _case(lambda wd: scenes.cfg1(wd, xres=64, yres=64, nsamp=9), flags=0, fp32_share={"normal": SPHERE_NORMAL_SHARE}),
    "scaled_instance": _case(_scaled_instance, flags=0),
}

_scenes, _refs = {}, {}


def _scene(name, workdir):
    if name not in _scenes:
        c = CASES[name]
        cfg, root = c["build"](workdir)
        if c["filt"]: cfg["Film"]["Filter"] = dict(c["filt"])
        _scenes[name] = Scene.loads(cfg, root, flags=c["flags"])
    return _scenes[name]


def _part_args(part):
    if part is not None and part[0] == "band": return dict(rect=None, rank=part[1], world=part[2])
    return dict(rect=part, rank=0, world=1)


def _reference(name, workdir):
    if name not in _refs:
        sc, c = _scene(name, workdir), CASES[name]
        total = None
        for part in c["parts"]:
            p = AR.planes(sc, max_samples=c["max_samples"], **_part_args(part))
            total = p if total is None else {k: total[k] + p[k] for k in p}
        assert total["depth"][..., 2].max() > 0
        if "cfg3" not in name and name != "scaled_instance":      # (the enclosure of cfg3 leaves no misses)
            assert (total["albedo"][..., 3] > total["depth"][..., 2]).any()
        _refs[name] = total
    return _refs[name]


def _device(name, workdir, prec, options=()):
    sc, c = _scene(name, workdir), CASES[name]
    r = Renderer(sc, 0, prec)
    if c["max_paths"]: r.set_option("max_paths", c["max_paths"])
    for k in options: r.set_option(k, 0)
    total = None
    for part in c["parts"]:
        p = r.render_aov(max_samples=c["max_samples"], **_part_args(part))
        total = p if total is None else {k: total[k] + p[k] for k in p}
    r.close()
    return total


def _channels(plane):
    """(value channels, weight channel, the magnitude each value channel is measured against) of a plane of rrt_aov."""
    if plane == "depth": return (0, 1), 2, "own"       # sum t, sum t^2 | sum fw
    return (0, 1, 2), 3, "plane"


def _value_diff(plane, got, ref):
    """per pixel: the largest difference over the plane's value channels, relative to the plane's (depth: the channel's) largest magnitude"""
    vals, _, scale = _channels(plane)
    g, r = got[..., vals].astype(np.float64), ref[..., vals]
    mag = np.abs(r).max() if scale == "plane" else np.abs(r).reshape(-1, len(vals)).max(0)
    assert np.all(mag > 0)
    return (np.abs(g - r) / mag).max(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_f64_planes_match_reference(name, workdir):
    ref = _reference(name, workdir)
    got = _device(name, workdir, RRT_F64)
    for plane in PLANES:
        _, wc, _ = _channels(plane)
        w, w_ref = got[plane][..., wc], ref[plane][..., wc]
        diff = _value_diff(plane, got[plane], ref[plane])
        print(f"{name}: f64 {plane}: values max {diff.max():.3e}, weights max {np.abs(w - w_ref).max():.3e}, support equal {np.array_equal(w != 0, w_ref != 0)}")
        if CASES[name]["filt"] is None:
            assert np.array_equal(w, w_ref), plane      # integers
        else:
            assert np.array_equal(w != 0, w_ref != 0), plane
            np.testing.assert_allclose(w, w_ref, rtol=1e-12, atol=0)
        assert diff.max() < 1e-9, (plane, diff.max())
        if plane == "depth": assert np.all(got[plane][..., 3] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_planes_close_to_reference(name, workdir):
    ref = _reference(name, workdir)
    got = _device(name, workdir, RRT_F32)
    sc = _scene(name, workdir)
    spp = int(sc.desc.sampler.samples_per_pixel) - 1
    if CASES[name]["max_samples"]: spp = min(spp, CASES[name]["max_samples"])
    live, live_ref = float(got["albedo"][..., 3].astype(np.float64).sum()), float(ref["albedo"][..., 3].sum())
    print(f"{name}: fp32 live weight {live} against {live_ref}")
    failures = []
    for plane in PLANES:
        _, wc, _ = _channels(plane)
        covered = ref[plane][..., wc] != 0
        w_diff = np.abs(got[plane][..., wc].astype(np.float64) - ref[plane][..., wc]) / ref[plane][..., wc].max()
        diff = np.maximum(_value_diff(plane, got[plane], ref[plane]), w_diff)
        assert np.all(got[plane][~covered & (got[plane][..., wc] == 0)] == 0)
        d = diff[covered | (got[plane][..., wc] != 0)]
        print(f"{name}: fp32 {plane} at {spp} spp: within 1e-4: {(d < 1e-4).mean():.4f}, mean {d.mean():.3e}, max {d.max():.3e}")
        if not (d < 1e-4).mean() >= CASES[name]["fp32_share"].get(plane, 0.975): failures.append((plane, "share", (d < 1e-4).mean()))
        if not d.mean() < 1e-4: failures.append((plane, "mean", d.mean()))
        if not d.max() < 3e-2 * 256 / spp: failures.append((plane, "max", d.max()))
    assert abs(live - live_ref) <= 2e-5 * live_ref, (live, live_ref)
    assert not failures, failures


def _sum_parts(r, parts, **kw):
    total = None
    for part in parts:
        p = r.render_aov(**_part_args(part), **kw)
        total = p if total is None else {k: total[k] + p[k] for k in p}
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("filt", [None, GAUSS], ids=["box", "gauss"])
def test_parts_sum_to_the_whole(prec, filt, workdir):
    """Rects that tile the film, and the bands of three ranks, add up to the whole call: bit for bit under the box filter (a pixel's samples are
    all in one part, summed in sample order), to the rounding of the differently ordered sums under a wide filter (test_frame_shapes.py::_check_weights' bars)."""
    cfg, root = _cfg5(workdir, (128, 104), 9)
    if filt: cfg["Film"]["Filter"] = dict(filt)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, prec)
    whole = r.render_aov()
    rects = _sum_parts(r, [(0, 0, 61, 50), (61, 0, 128, 50), (0, 50, 128, 104)])
    bands = _sum_parts(r, _bands(3))
    r.close()
    assert whole["depth"][..., 2].max() > 0
    rtol = 1e-12 if prec == RRT_F64 else 1e-5
    for plane in PLANES:
        for parts in (rects, bands):
            if filt is None:
                assert np.array_equal(parts[plane], whole[plane]), plane
            else:
                _, wc, _ = _channels(plane)
                assert np.array_equal(parts[plane][..., wc] != 0, whole[plane][..., wc] != 0)
                np.testing.assert_allclose(parts[plane][..., wc], whole[plane][..., wc], rtol=rtol, atol=0)
                np.testing.assert_allclose(parts[plane], whole[plane], rtol=rtol, atol=rtol * np.abs(whole[plane]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_max_samples_is_a_shorter_scene(prec, workdir):
    """render_aov(max_samples=8) of a 25-sample Halton scene = render_aov() of the same scene loaded with nsamp 9, bit for bit."""
    planes = []
    for nsamp, k in ((25, 8), (9, 0)):
        cfg, root = _cfg5(workdir, (64, 48), nsamp)
        r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, prec)
        planes.append(r.render_aov(max_samples=k))
        r.close()
    assert planes[0]["albedo"][..., 3].max() > 0
    for plane in PLANES:
        assert np.array_equal(planes[0][plane], planes[1][plane]), plane


@pytest.mark.gpu
def test_shortcuts_change_no_bit(workdir):
    """tile_trees, tile_order, quad_nodes, lens_cull and aux_margin off together: the same planes. The frame rendered first builds the tile trees, so
    the default pass is the one that uses them."""
    cfg, root = _cfg5(workdir, (128, 96), 25)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    _, st = r.render(stats=True)
    assert st.tile_launches > 0
    fast = r.render_aov()
    for k in SHORTCUTS: r.set_option(k, 0)
    plain = r.render_aov()
    r.close()
    assert fast["depth"][..., 2].max() > 0
    for plane in PLANES:
        assert np.array_equal(fast[plane], plain[plane]), plane


@pytest.mark.gpu
def test_frame_is_untouched(workdir):
    """render, render_aov, render on one default fp32 handle (tile trees, film records, root and horizon cull all on): the same frame twice."""
    cfg, root = _cfg5(workdir, (128, 96), 25)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    a, sa = r.render(stats=True)
    aov = r.render_aov()
    b, sb = r.render(stats=True)
    r.close()
    assert aov["depth"][..., 2].max() > 0 and a[..., :3].max() > 0
    assert sa.tile_launches > 0 and sa.root_culled > 0
    assert np.array_equal(a, b)
    for key in ("camera_rays", "closest_queries", "any_queries", "tile_launches", "root_culled"):
        assert getattr(sa, key) == getattr(sb, key), key


@pytest.mark.gpu
def test_error_paths(workdir):
    import torch
    cfg, root = _cfg5(workdir, (64, 48), 9)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    lib = A.lib()
    for rect in ((0, 0, 65, 48), (-1, 0, 64, 48), (10, 10, 10, 20)):
        with pytest.raises(RrtError, match="rect outside the film"):
            r.render_aov(rect=rect)
    for rank, world in ((0, 0), (2, 2), (-1, 1)):
        with pytest.raises(RrtError, match="rank/world"):
            r.render_aov(rank=rank, world=world)
    plane = np.zeros((48, 64, 4), np.float64)
    wrong = A.Aov(A.RRT_MEM_HOST, A.RRT_F64, plane.ctypes.data, None, None)
    full = (C.c_int32 * 4)(0, 0, 64, 48)
    assert lib.rrt_render_aov(r._h, full, 0, 1, 0, C.byref(wrong)) == A.RRT_EINVAL and b"precision" in lib.rrt_last_error()
    assert lib.rrt_render_aov(r._h, None, 0, 1, 0, C.byref(wrong)) == A.RRT_EINVAL
    film = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, film.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_aov()
    r.render_end()
    assert np.all(plane == 0)
    # device planes, and a single plane
    dev = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    only = A.Aov(A.RRT_MEM_DEVICE, A.RRT_F32, None, None, dev.data_ptr())
    assert lib.rrt_render_aov(r._h, full, 0, 1, 0, C.byref(only)) == A.RRT_OK, lib.rrt_last_error()
    assert lib.rrt_render_aov(r._h, full, 0, 1, 0, C.byref(only)) == A.RRT_OK       # += : twice the sums
    host = r.render_aov(planes=("depth",))
    assert set(host) == {"depth"}
    assert np.array_equal(dev.cpu().numpy(), host["depth"] + host["depth"])
    r.close()


@pytest.mark.gpu
def test_resolve_aov(workdir):
    cfg, root = _cfg5(workdir, (64, 48), 25)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    res = resolve_aov(r.render_aov())
    r.close()
    hit = res["coverage"] > 0
    assert hit.any() and not hit.all()
    assert np.all((res["coverage"] >= 0) & (res["coverage"] <= 1))
    np.testing.assert_allclose(np.linalg.norm(res["normal"][hit], axis=-1), 1.0, rtol=1e-12)
    assert np.all(res["normal"][~hit] == 0) and np.all(res["depth"][~hit] == 0)
    assert np.all(res["depth"][hit] > 0) and np.all(res["albedo"] >= 0) and np.all(res["albedo"] <= 1)


def _png_size(path):
    with open(path, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", head[16:24])


@pytest.mark.gpu
def test_cli_writes_three_pngs(tmp_path):
    """RRT_AOV=<prefix>: rrt_render and `python -m rs_ray_toy_amd` write <prefix>_albedo / _normal / _depth.png of the film's size after the frame."""
    cfg, root = _cfg5(str(tmp_path), (64, 48), 9)
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
        prefix = str(tmp_path / f"aov_{tag}")
        env = dict(os.environ, RRT_AOV=prefix, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        p = subprocess.run(cmd + [str(scene), str(tmp_path / f"{tag}.png")], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr
        assert _png_size(tmp_path / f"{tag}.png") == (64, 48)
        for plane in PLANES:
            assert _png_size(f"{prefix}_{plane}.png") == (64, 48), plane
    # without the variable nothing is written beside the frame
    p = subprocess.run([exe, str(scene), str(tmp_path / "plain.png")], capture_output=True, text=True, timeout=600, env={k: v for k, v in os.environ.items() if k != "RRT_AOV"})
    assert p.returncode == 0 and not [f for f in os.listdir(tmp_path) if f.startswith("plain_")]
