"""Ambient occlusion and bent normals beside the film (rrt_render_ao, include/rrt.h).

CPU tests: the C layout of rrt_ao / rrt_ao_params, the argument checks that need no device, the numpy reference (tests/ao_reference.py) on the
floor case - every hit sample has a == pi in cosine mode - and the cap on the pixels the f64 test may leave out, which is a property of the
reference alone.

GPU tests, against that reference:
  test_f64_planes_match_reference      the project's f64 bar: every value channel within 1e-9 of its largest magnitude (ao: the channel's own,
                                       as depth; bent: the plane's), box-filter weight channels equal exactly, wide ones equal support and rtol
                                       1e-12. A pixel is left out only where one of its draws has an oracle any-hit margin below 1e-9 (device and
                                       numpy sin / cos differ in the last bits, which can turn such a ray): at most 0.5 % of a case's covered pixels.
  test_fp32_planes_close_to_reference  weights and live weight: test_aov.py's bars. Values: the bar is measured against existing code - the
                                       reference's own rays, rounded to fp32, through Renderer.trace_any in fp32, the planes rebuilt in numpy from
                                       those verdicts; the pass stays within 1.5 x that baseline's share beyond 1e-4, mean and max, and is never
                                       asked for better than the fp32 frame bars (0.975 within 1e-4, mean 1e-4, max 3e-2 x 256 / spp).
                                       Figures: profiles/ao_gpu_tests.txt.
  test_parts_sum_to_the_whole, test_max_samples_is_a_shorter_scene, test_draw_rounds_do_not_depend_on_the_pool, test_shortcuts_change_no_bit,
  test_frame_is_untouched, test_error_paths, test_resolve_ao, test_cli_writes_png.
The scenes are tie-free, as test_frame_shapes.py requires of its own: generic rotation axes, heightfields, a tilted floor.
"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ao_reference as AO
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError, RrtUnsupported, Scene, resolve_ao, scenes
from scene_util import write_patch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PLANES = ("ao", "bent")
GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
AXES = ([1.0, 2.0, 3.0], [3.0, 1.0, 2.0], [2.0, 3.0, 1.0])
SHORTCUTS = ("tile_trees", "tile_order", "quad_nodes", "lens_cull", "aux_margin", "halton_tables")
EXCLUDED_CAP = 0.005


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------------------

def _write_floor(wd):
    """Two triangles of one tilted plane (no box face is a triangle's plane), counter-clockwise seen from +y."""
    y = lambda x, z: -2.0 + 0.013 * (x - 35.0) + 0.021 * z
    v = [(25.0, -10.0), (45.0, -10.0), (45.0, 10.0), (25.0, 10.0)]
    with open(os.path.join(wd, "floor.obj"), "w") as f:
        for x, z in v: f.write(f"v {x:.6f} {y(x, z):.9f} {z:.6f}\n")
        f.write("f 1 3 2\nf 1 4 3\n")


def _floor(wd, film=(32, 32), nsamp=5):
    os.makedirs(wd, exist_ok=True)
    _write_floor(wd)
    cfg = scenes._base(film[0], film[1], nsamp, {"integrator_type": "Path", "max_depth": 3})
    cfg["objs"] = [{"filename": "floor.obj", "obj_name": "floor"}]
    cfg["lights"] = [{"light_type": "point", "world_pos": [30.0, 8.0, 0.0], "spectrum": {"values": [500, 500, 500]}}]
    cfg["Aggregate"]["primitives"] = [{"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "floor"}]
    return cfg, wd


def _cubes(wd, film=(48, 40), nsamp=5):
    """scene.json's 36 instanced triangles (three cubes, generic rotation axes) over an 8 x 8 x 2 heightfield."""
    cfg, root = scenes.cfg2(wd, xres=film[0], yres=film[1], nsamp=nsamp, max_depth=4)
    scenes.write_heightfield(wd, n=8, name="hf8.obj")
    for inst, axis in zip(cfg["Aggregate"]["primitives"][0]["instances"], AXES): inst["rotation_axis"] = axis
    cfg["objs"].append({"filename": "hf8.obj", "obj_name": "hf8"})
    cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "mat_plastic", "obj_name": "hf8"})
    return cfg, root


def _spheres(wd):
    cfg, root = _floor(wd)
    inst = [{"world_pos": [33.0, -1.1, -2.5]}, {"world_pos": [36.0, -0.9, 0.4]}, {"world_pos": [34.5, -1.0, 3.1]}]
    cfg["Aggregate"]["primitives"].append({"primitive_type": "sphere", "material_name": "mat_matte", "radius": 1.0, "instances": inst})
    return cfg, root


def _scaled(wd):
    cfg, root = _cubes(wd, film=(32, 32))
    cfg["Aggregate"]["primitives"][0]["instances"][0]["scale"] = [1.5, 0.7, 1.2]      # non-rigid: the device keeps it, n_g comes back un-normalised
    return cfg, root


def _uv(wd):
    """The floor and a curved patch with vt (dpdu runs along u = x, not along the default's p1 - p0) and smooth vn (shading.dpdu is not dpdu)."""
    cfg, root = _floor(wd)
    write_patch(wd, half=4.0, bend=0.03)
    cfg["objs"].append({"filename": "patch.obj", "obj_name": "patch_01"})
    cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "mat_plastic", "obj_name": "patch_01",
                                           "instances": [{"world_pos": [34.0, -1.2, 0.5], "rotation_axis": [0.2, 1.0, 0.1], "rotation_angle": 20}]})
    return cfg, root


def _bands(world):
    return tuple(("band", k, world) for k in range(world))


def _case(build, draws, cos=(True,), parts=(None,), filt=None, max_paths=None):
    return dict(build=build, draws=tuple(draws), cos=tuple(cos), parts=tuple(parts), filt=filt, max_paths=max_paths)


RECTS, BANDS = ((0, 0, 29, 23), (29, 0, 48, 23), (0, 23, 48, 40)), _bands(3)
CASES = {
    "floor": _case(_floor, (4,), cos=(True, False)),
    "cubes": _case(_cubes, (1, 16), max_paths=1024),
    "cubes_rects": _case(_cubes, (16,), parts=RECTS[:2], max_paths=1024),           # two uneven rects
    "cubes_bands": _case(_cubes, (16,), parts=BANDS, max_paths=1024),
    "n32": _case(_cubes, (32,), parts=((16, 12, 32, 28),)),                          # dimensions cross the 64 tabulated ones
    "spheres": _case(_spheres, (3,), cos=(False,)),
    "scaled": _case(_scaled, (3,)),
    "uv": _case(_uv, (3,)),
    "gauss": _case(lambda wd: _cubes(wd, film=(32, 32)), (2,), parts=((3, 2, 20, 30), (20, 2, 32, 30)), filt=GAUSS),   # splats across the rects' border
}
# every (case, draws, cos) the planes are compared for
RUNS = [(name, n, cos) for name in sorted(CASES) for n in CASES[name]["draws"] for cos in CASES[name]["cos"]]
_ids = [f"{name}-N{n}-{'cos' if cos else 'uniform'}" for name, n, cos in RUNS]

_scenes, _refs = {}, {}


def _scene(name, workdir):
    if name not in _scenes:
        c = CASES[name]
        cfg, root = c["build"](os.path.join(workdir, "ao_" + name))
        if c["filt"]: cfg["Film"]["Filter"] = dict(c["filt"])
        _scenes[name] = Scene.loads(cfg, root, flags=0)
    return _scenes[name]


def _part_args(part):
    if part is not None and part[0] == "band": return dict(rect=None, rank=part[1], world=part[2])
    return dict(rect=part, rank=0, world=1)


def _reference(name, n, cos, workdir):
    """dict(ao, bent, risky, parts = the per-part samples) of a run, computed once and left unchanged"""
    key = (name, n, cos)
    if key not in _refs:
        sc, c = _scene(name, workdir), CASES[name]
        total, parts = None, []
        for part in c["parts"]:
            p = AO.planes(sc, n_samples=n, cos_sample=cos, with_samples=True, **_part_args(part))
            parts.append(p.pop("samples"))
            total = p if total is None else {k: (total[k] | p[k]) if k == "risky" else total[k] + p[k] for k in p}
        assert total["ao"][..., 2].max() > 0 and total["ao"][..., 0].max() > 0
        total["parts"] = parts
        _refs[key] = total
    return _refs[key]


def _device(name, n, cos, workdir, prec, options=(), max_paths="case", set_options=None):
    sc, c = _scene(name, workdir), CASES[name]
    r = Renderer(sc, 0, prec)
    if max_paths == "case": max_paths = c["max_paths"]
    if max_paths: r.set_option("max_paths", max_paths)
    for k in options: r.set_option(k, 0)
    for k, v in (set_options or {}).items(): r.set_option(k, v)
    total = None
    for part in c["parts"]:
        p = r.render_ao(n_samples=n, cos_sample=cos, **_part_args(part))
        total = p if total is None else {k: total[k] + p[k] for k in p}
    r.close()
    return total


def _channels(plane):
    """(value channels, weight channels, the magnitude each value channel is measured against) of a plane of rrt_ao."""
    if plane == "ao": return (0, 1), (2, 3), "own"       # sum a, sum a^2 | sum fw over hits, over live samples
    return (0, 1, 2), (3,), "plane"


def _value_diff(plane, got, ref):
    vals, _, scale = _channels(plane)
    g, r = got[..., vals].astype(np.float64), ref[..., vals]
    mag = np.abs(r).max() if scale == "plane" else np.abs(r).reshape(-1, len(vals)).max(0)
    assert np.all(mag > 0)
    return (np.abs(g - r) / mag).max(-1)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------------------------

def test_ao_structs_match_c_layout(tmp_path):
    want = {"rrt_ao": (A.Ao, ["mem", "precision", "ao", "bent"]), "rrt_ao_params": (A.AoParams, ["n_samples", "cos_sample"])}
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cname, (cls, fields) in want.items():
        assert [name for name, _ in cls._fields_] == fields
        src.append(f'printf("{cname}.size %zu\\n", sizeof({cname}));')
        src += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", str(c), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, (cls, fields) in want.items():
        assert int(out[f"{cname}.size"]) == C.sizeof(cls)
        for f in fields:
            assert int(out[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_render_ao_refuses_bad_arguments():
    """No device is needed to be told so: a NULL handle, a NULL rrt_ao, an rrt_ao that asks for no plane, n_samples 0 and 257 are RRT_EINVAL, each
    with its own message; rrt_ao_defaults of no handle is 64 draws, cosine."""
    lib = A.lib()
    plane = np.zeros(4, np.float32)
    rect = (C.c_int32 * 4)(0, 0, 1, 1)
    good = A.Ao(A.RRT_MEM_HOST, A.RRT_F32, plane.ctypes.data, None)
    assert lib.rrt_render_ao(None, rect, 0, 1, 0, None, C.byref(good)) == A.RRT_EINVAL
    assert b"null handle" in lib.rrt_last_error()
    assert lib.rrt_render_ao(None, rect, 0, 1, 0, None, None) == A.RRT_EINVAL
    assert b"rrt_ao" in lib.rrt_last_error() and b"null output" in lib.rrt_last_error()
    empty = A.Ao(A.RRT_MEM_HOST, A.RRT_F32, None, None)
    assert lib.rrt_render_ao(None, rect, 0, 1, 0, None, C.byref(empty)) == A.RRT_EINVAL
    assert b"no plane" in lib.rrt_last_error()
    for n, word in ((0, b"at least 1"), (257, b"at most 256")):
        prm = A.AoParams(n, 1)
        assert lib.rrt_render_ao(None, rect, 0, 1, 0, C.byref(prm), C.byref(good)) == A.RRT_EINVAL
        assert word in lib.rrt_last_error(), lib.rrt_last_error()
    prm = A.AoParams(0, 0)
    lib.rrt_ao_defaults(None, C.byref(prm))
    assert (prm.n_samples, prm.cos_sample) == (64, 1)
    assert np.all(plane == 0)


def test_reference_floor_is_fully_open(workdir):
    """Nothing but one plane: every ray of every hit sample is free, so a = sum (pi / N) = pi in cosine mode, and b runs along n."""
    ref = _reference("floor", 4, True, workdir)
    s = ref["parts"][0]
    hit = s["hit"]
    assert hit.sum() > 200 and (s["live"] & ~hit).sum() > 0
    assert s["free"].all()
    np.testing.assert_allclose(s["a"][hit], np.pi, rtol=1e-12, atol=0)
    n = np.array([-0.013, 1.0, -0.021]); n /= np.linalg.norm(n)
    b = s["b"][hit]
    np.testing.assert_allclose(b, (np.pi / 4) * s["ray_d"].sum(1), rtol=0, atol=1e-12)      # every a_i is pi / N: b is the mean direction times pi
    assert np.all(b @ n > 0)
    # uniform mode on the same points: a_i = 2 pi z / N, not pi
    assert np.abs(_reference("floor", 4, False, workdir)["parts"][0]["a"][hit] - np.pi).max() > 0.1


@pytest.mark.parametrize("name,n,cos", RUNS, ids=_ids)
def test_reference_keeps_the_exclusion_cap(name, n, cos, workdir):
    """The f64 test may leave out the pixels that receive a draw whose oracle any-hit margin is below 1e-9: at most 0.5 % of the covered pixels.
    A property of the scenes and the reference alone."""
    ref = _reference(name, n, cos, workdir)
    covered = ref["ao"][..., 2] != 0
    share = (ref["risky"] & covered).sum() / covered.sum()
    print(f"{name} N {n}: {int((ref['risky'] & covered).sum())} of {int(covered.sum())} covered pixels hold a draw with margin < 1e-9")
    assert share <= EXCLUDED_CAP
    occluded = np.concatenate([~s["free"][s["ok"]] for s in ref["parts"] if "free" in s])
    if name != "floor": assert 0.02 < occluded.mean() < 0.98, occluded.mean()      # the case does test occlusion


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,n,cos", RUNS, ids=_ids)
def test_f64_planes_match_reference(name, n, cos, workdir):
    ref = _reference(name, n, cos, workdir)
    got = _device(name, n, cos, workdir, RRT_F64)
    covered = ref["ao"][..., 2] != 0
    keep = ~ref["risky"]
    left_out = int((ref["risky"] & covered).sum())
    print(f"{name} N {n}: {left_out} of {int(covered.sum())} covered pixels left out (a draw with any-hit margin < 1e-9)")
    assert left_out <= EXCLUDED_CAP * covered.sum()
    for plane in PLANES:
        _, wcs, _ = _channels(plane)
        diff = _value_diff(plane, got[plane], ref[plane])
        print(f"{name} N {n}: f64 {plane}: values max {diff[keep].max():.3e} (left-out pixels: {diff[~keep].max() if (~keep).any() else 0.0:.3e})")
        for wc in wcs:
            w, w_ref = got[plane][..., wc], ref[plane][..., wc]
            if CASES[name]["filt"] is None:
                assert np.array_equal(w, w_ref), (plane, wc)      # integers
            else:
                assert np.array_equal(w != 0, w_ref != 0), (plane, wc)
                np.testing.assert_allclose(w, w_ref, rtol=1e-12, atol=0)
        assert diff[keep].max() < 1e-9, (plane, diff[keep].max())


def _fp32_stats(plane, got, ref):
    """(share beyond 1e-4, mean, max) of a plane's value differences over the covered pixels"""
    _, wcs, _ = _channels(plane)
    covered = (ref[..., wcs[0]] != 0) | (np.asarray(got)[..., wcs[0]] != 0)
    d = _value_diff(plane, np.asarray(got), ref)[covered]
    return float((d >= 1e-4).mean()), float(d.mean()), float(d.max())


def check_fp32_planes(name, n, cos, workdir, set_options=None):
    """test_fp32_planes_close_to_reference's comparison (module docstring) of the fp32 pass rendered under `set_options` (option -> value; None: the
    default handle). The baseline is always the default handle's trace_any."""
    ref = _reference(name, n, cos, workdir)
    sc = _scene(name, workdir)
    spp = int(sc.desc.sampler.samples_per_pixel) - 1
    # the baseline: the reference's own rays, rounded to fp32, through the existing fp32 any-hit entry point (start triangle excluded, as
    # test_gpu_parity.py does for spawned rays), and the planes rebuilt in numpy from those verdicts
    r = Renderer(sc, 0, RRT_F32)
    base = None
    for s in ref["parts"]:
        a, b = np.zeros_like(s["a"]), np.zeros_like(s["b"])
        if "free" in s:
            nh, N = s["free"].shape
            occ = r.trace_any(s["ray_o"].reshape(-1, 3), s["ray_d"].reshape(-1, 3), np.full(nh * N, np.inf), skip_prim=np.repeat(s["prim"], N)).reshape(nh, N)
            free = ~occ & s["ok"]
            for i in range(N):
                a[s["hit_index"]] += np.where(free[:, i], s["a_i"][:, i], 0.0)
                b[s["hit_index"]] += np.where(free[:, i, None], s["a_i"][:, i, None] * s["ray_d"][:, i], 0.0)
        p = AO.planes_of(sc, s, a, b)
        base = p if base is None else {k: base[k] + p[k] for k in ("ao", "bent")}
    r.close()
    got = _device(name, n, cos, workdir, RRT_F32, set_options=set_options)
    live, live_ref = float(got["ao"][..., 3].astype(np.float64).sum()), float(ref["ao"][..., 3].sum())
    print(f"{name} N {n}: fp32 live weight {live} against {live_ref}")
    failures = []
    for plane in PLANES:
        _, wcs, _ = _channels(plane)
        for wc in wcs:
            w_ref = ref[plane][..., wc]
            w_diff = (np.abs(got[plane][..., wc].astype(np.float64) - w_ref) / w_ref.max())[(w_ref != 0) | (got[plane][..., wc] != 0)]
            if not ((w_diff < 1e-4).mean() >= 0.975 and w_diff.mean() < 1e-4 and w_diff.max() < 3e-2 * 256 / spp): failures.append((plane, "weight", wc, w_diff.max()))
        b_share, b_mean, b_max = _fp32_stats(plane, base[plane], ref[plane])
        g_share, g_mean, g_max = _fp32_stats(plane, got[plane], ref[plane])
        print(f"{name} N {n} {plane} at {spp} spp: baseline beyond 1e-4: {b_share:.4f}, mean {b_mean:.3e}, max {b_max:.3e} | pass beyond 1e-4: {g_share:.4f}, mean {g_mean:.3e}, max {g_max:.3e}")
        if not g_share <= max(1.5 * b_share, 1.0 - 0.975): failures.append((plane, "share", g_share, b_share))
        if not g_mean <= max(1.5 * b_mean, 1e-4): failures.append((plane, "mean", g_mean, b_mean))
        if not g_max <= max(1.5 * b_max, 3e-2 * 256 / spp): failures.append((plane, "max", g_max, b_max))
    assert abs(live - live_ref) <= 2e-5 * live_ref, (live, live_ref)
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,cos", RUNS, ids=_ids)
def test_fp32_planes_close_to_reference(name, n, cos, workdir):
    check_fp32_planes(name, n, cos, workdir)


def _sum_parts(r, parts, **kw):
    total = None
    for part in parts:
        p = r.render_ao(**_part_args(part), **kw)
        total = p if total is None else {k: total[k] + p[k] for k in p}
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("filt", [None, GAUSS], ids=["box", "gauss"])
def test_parts_sum_to_the_whole(prec, filt, workdir):
    """Rects that tile the film, and the bands of three ranks, add up to the whole call: bit for bit under the box filter (a pixel's samples are
    all in one part, summed in sample order), to the rounding of the differently ordered sums under a wide filter (test_aov.py's rtol)."""
    cfg, root = _cubes(os.path.join(workdir, "ao_parts"))
    if filt: cfg["Film"]["Filter"] = dict(filt)
    r = Renderer(Scene.loads(cfg, root, flags=0), 0, prec)
    whole = r.render_ao(n_samples=4)
    rects = _sum_parts(r, RECTS, n_samples=4)
    bands = _sum_parts(r, BANDS, n_samples=4)
    r.close()
    assert whole["ao"][..., 0].max() > 0
    rtol = 1e-12 if prec == RRT_F64 else 1e-5
    for plane in PLANES:
        for parts in (rects, bands):
            if filt is None:
                assert np.array_equal(parts[plane], whole[plane]), plane
            else:
                for wc in _channels(plane)[1]:
                    assert np.array_equal(parts[plane][..., wc] != 0, whole[plane][..., wc] != 0)
                    np.testing.assert_allclose(parts[plane][..., wc], whole[plane][..., wc], rtol=rtol, atol=0)
                np.testing.assert_allclose(parts[plane], whole[plane], rtol=rtol, atol=rtol * np.abs(whole[plane]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_max_samples_is_a_shorter_scene(prec, workdir):
    """render_ao(max_samples=4) of a 9-sample Halton scene = render_ao() of the same scene loaded with nsamp 5, bit for bit."""
    planes = []
    for nsamp, k in ((9, 4), (5, 0)):
        cfg, root = _cubes(os.path.join(workdir, "ao_short"), nsamp=nsamp)
        r = Renderer(Scene.loads(cfg, root, flags=0), 0, prec)
        planes.append(r.render_ao(max_samples=k, n_samples=4))
        r.close()
    assert planes[0]["ao"][..., 0].max() > 0
    for plane in PLANES:
        assert np.array_equal(planes[0][plane], planes[1][plane]), plane


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_draw_rounds_do_not_depend_on_the_pool(prec, workdir):
    """max_paths 1024 (a pass is cut into pixel groups and sample chunks) against the default pool: the same bits."""
    small = _device("cubes", 16, True, workdir, prec, max_paths=1024)
    large = _device("cubes", 16, True, workdir, prec, max_paths=None)
    assert small["ao"][..., 0].max() > 0
    for plane in PLANES:
        assert np.array_equal(small[plane], large[plane]), plane


@pytest.mark.gpu
def test_shortcuts_change_no_bit(workdir):
    """tile_trees, tile_order, quad_nodes, lens_cull, aux_margin and halton_tables off together: the same planes (32 draws: dimensions on both sides
    of the tabulated 64). The frame rendered first builds the tile trees where the scene takes them."""
    cfg, root = _cubes(os.path.join(workdir, "ao_short_cuts"), film=(64, 48), nsamp=9)
    r = Renderer(Scene.loads(cfg, root, flags=0), 0, RRT_F32)
    r.render()
    fast = r.render_ao(n_samples=32)
    for k in SHORTCUTS: r.set_option(k, 0)
    plain = r.render_ao(n_samples=32)
    r.close()
    assert fast["ao"][..., 0].max() > 0
    for plane in PLANES:
        assert np.array_equal(fast[plane], plain[plane]), plane


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [0, 1])
def test_n32_halton_tables_give_the_same_bits(tables, workdir):
    """Draw dimensions 5 .. 68 cross the 64 tabulated ones: option halton_tables 0 / 1 gives the bits of the default handle."""
    sc = _scene("n32", workdir)
    want = _device("n32", 32, True, workdir, RRT_F32)
    r = Renderer(sc, 0, RRT_F32)
    r.set_option("halton_tables", tables)
    got = r.render_ao(rect=CASES["n32"]["parts"][0], n_samples=32)
    r.close()
    for plane in PLANES:
        assert np.array_equal(got[plane], want[plane]), plane


@pytest.mark.gpu
def test_frame_is_untouched(workdir):
    """render, render_ao, render on one default fp32 handle: the same film and counts; render_aov before and after: the same planes."""
    cfg, root = scenes.cfg5(os.path.join(workdir, "ao_frame"), xres=128, yres=96, nsamp=25, max_depth=8, n=64)
    r = Renderer(Scene.loads(cfg, root, flags=A.RRT_FIXED_BVH), 0, RRT_F32)
    a, sa = r.render(stats=True)
    aov_a = r.render_aov()
    ao = r.render_ao(n_samples=4, max_samples=8)
    aov_b = r.render_aov()
    b, sb = r.render(stats=True)
    r.close()
    assert ao["ao"][..., 0].max() > 0 and a[..., :3].max() > 0
    assert sa.tile_launches > 0 and sa.root_culled > 0
    assert np.array_equal(a, b)
    for key in ("camera_rays", "closest_queries", "any_queries", "tile_launches", "root_culled"):
        assert getattr(sa, key) == getattr(sb, key), key
    for plane in aov_a:
        assert np.array_equal(aov_a[plane], aov_b[plane]), plane


@pytest.mark.gpu
def test_error_paths(workdir):
    import torch
    sc = _scene("cubes", workdir)
    r = Renderer(sc, 0, RRT_F32)
    lib = A.lib()
    for rect in ((0, 0, 49, 40), (-1, 0, 48, 40), (10, 10, 10, 20)):
        with pytest.raises(RrtError, match="rect outside the film"):
            r.render_ao(rect=rect)
    for rank, world in ((0, 0), (2, 2), (-1, 1)):
        with pytest.raises(RrtError, match="rank/world"):
            r.render_ao(rank=rank, world=world)
    plane = np.zeros((40, 48, 4), np.float64)
    wrong = A.Ao(A.RRT_MEM_HOST, A.RRT_F64, plane.ctypes.data, None)
    full = (C.c_int32 * 4)(0, 0, 48, 40)
    assert lib.rrt_render_ao(r._h, full, 0, 1, 0, None, C.byref(wrong)) == A.RRT_EINVAL and b"precision" in lib.rrt_last_error()
    assert lib.rrt_render_ao(r._h, None, 0, 1, 0, None, C.byref(wrong)) == A.RRT_EINVAL
    film = torch.zeros((40, 48, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, film.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_ao()
    r.render_end()
    assert np.all(plane == 0)
    # device planes, a single plane, += : twice the sums; NULL params = the defaults (64 draws, cosine, on a Path scene)
    dev = torch.zeros((40, 48, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    only = A.Ao(A.RRT_MEM_DEVICE, A.RRT_F32, None, dev.data_ptr())
    assert lib.rrt_render_ao(r._h, full, 0, 1, 0, None, C.byref(only)) == A.RRT_OK, lib.rrt_last_error()
    assert lib.rrt_render_ao(r._h, full, 0, 1, 0, None, C.byref(only)) == A.RRT_OK
    host = r.render_ao(planes=("bent",))
    assert set(host) == {"bent"}
    assert np.array_equal(dev.cpu().numpy(), host["bent"] + host["bent"])
    r.close()
    # the StratifiedSampler is refused by name
    cfg, root = _cubes(os.path.join(workdir, "ao_strat"))
    cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 2, "jitter": True, "dimension": 4}
    r = Renderer(Scene.loads(cfg, root, flags=0), 0, RRT_F32)
    with pytest.raises(RrtUnsupported, match="StratifiedSampler"):
        r.render_ao(n_samples=4)
    r.close()


@pytest.mark.gpu
def test_ao_defaults_follow_the_scene(workdir):
    """An AO scene's own n_samples / cos_sample are the defaults; every other integrator type gives 64 / cosine. The pass itself ignores the type."""
    cfg, root = _floor(os.path.join(workdir, "ao_defaults"))
    cfg["Integrator"] = {"integrator_type": "AO", "n_samples": 8, "cos_sample": False}
    r = Renderer(Scene.loads(cfg, root, flags=0), 0, RRT_F32)
    prm = A.AoParams()
    A.lib().rrt_ao_defaults(r._h, C.byref(prm))
    got = r.render_ao()
    want = r.render_ao(n_samples=prm.n_samples, cos_sample=prm.cos_sample)
    r.close()
    assert (prm.n_samples, prm.cos_sample) == (8, 0)
    assert got["ao"][..., 0].max() > 0
    for plane in PLANES:
        assert np.array_equal(got[plane], want[plane])


@pytest.mark.gpu
def test_resolve_ao(workdir):
    # the floor: fully open, bent normal = the plane's normal (fp32 sums: |a_i d_i| recovers a_i to a few ulp, 2^-23 each)
    r = Renderer(_scene("floor", workdir), 0, RRT_F32)
    res = resolve_ao(r.render_ao(n_samples=16))
    r.close()
    hit = res["coverage"] > 0
    assert hit.any() and not hit.all()
    np.testing.assert_allclose(res["ao"][hit], 1.0, rtol=0, atol=16 * 2.0 ** -22)
    n = np.array([-0.013, 1.0, -0.021]); n /= np.linalg.norm(n)
    # >= 16 cosine-weighted directions per pixel: their mean is (2 / 3) n with a tangent part of standard deviation 1 / (2 sqrt 16) per axis; 0.7 is 3 sigma
    assert np.all(res["bent"][hit] @ n > 0.7) and (res["bent"][hit] @ n).mean() > 0.95
    np.testing.assert_allclose(res["ao_var"][hit], 0.0, atol=1e-5)
    assert np.all(res["ao"][~hit] == 0) and np.all(res["bent"][~hit] == 0)
    # the cubes: values in [0, 1], unit bent normals, some occlusion
    r = Renderer(_scene("cubes", workdir), 0, RRT_F32)
    res = resolve_ao(r.render_ao(n_samples=16))
    r.close()
    hit = res["coverage"] > 0
    assert hit.any()
    assert np.all((res["ao"] >= 0) & (res["ao"] <= 1)) and np.all((res["coverage"] >= 0) & (res["coverage"] <= 1))
    assert res["ao"][hit].min() < 0.7 and res["ao"][hit].max() > 0.95
    lit = hit & (res["ao"] > 0)
    np.testing.assert_allclose(np.linalg.norm(res["bent"][lit], axis=-1), 1.0, rtol=1e-12)
    assert np.all(res["ao_var"] >= 0)


def _png_size(path):
    with open(path, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", head[16:24])


@pytest.mark.gpu
def test_cli_writes_png(tmp_path):
    """RRT_AO=<path.png>: rrt_render and `python -m rs_ray_toy_amd` write the resolved occlusion of the film's size after the frame."""
    cfg, root = _cubes(str(tmp_path))
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
        out = str(tmp_path / f"ao_{tag}.png")
        env = dict(os.environ, RRT_AO=out, RRT_AO_SAMPLES="4", RRT_AO_SPP="2", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        p = subprocess.run(cmd + [str(scene), str(tmp_path / f"{tag}.png")], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr
        assert _png_size(tmp_path / f"{tag}.png") == (48, 40)
        assert _png_size(out) == (48, 40)
    p = subprocess.run([exe, str(scene), str(tmp_path / "plain.png")], capture_output=True, text=True, timeout=600, env={k: v for k, v in os.environ.items() if not k.startswith("RRT_AO")})
    assert p.returncode == 0 and not [f for f in os.listdir(tmp_path) if f.startswith("plain_")]
