"""The moments frame and its feature buffers from one camera pass (rrt_render_frame_aov, include/rrt.h).

Every GPU comparison here is between two runs of the device library on one handle - the fused call against rrt_render_moments followed by
rrt_render_aov - so there is no tolerance anywhere: np.array_equal on the film, the moments plane, the three feature planes, and == on the
statistics. The scenes are the ones tests/test_aov.py renders, at its sizes.

  test_fused_equals_the_two_calls   the cases of CASES in fp32 and f64 (a case that needs the fp32 shortcuts is fp32 only).
                                    "cfg5_root_cull" has the root cull and the tile trees at work: a live camera ray that misses the root box never
                                    enters the queue, so nothing writes its record and the gather must read it as a miss.
  test_fused_after_a_stale_pass     a rect full of hits, then a rect of the same shape full of misses on the same handle: the first call's hit
                                    records lie in the very slots the second call's culled samples own. A gather that trusts an unwritten record
                                    fails here (in the case above the records left behind by rrt_render_aov happen to say "miss" for those slots).
  test_handle_is_left_as_it_was, test_shortcuts_change_no_bit, test_error_paths, test_cli_route.

On "small_pools": with max_paths 1000 the 3072 pixels of the 64 x 48 film are cut into four pixel groups and every pass holds ONE sample (samples
per pass = pool slots / pixels of the group, at least 1), so there every prefix of the samples ends on a pass border: max_samples 5 and 3 are both
of that kind. A prefix that ends INSIDE a pass needs passes of several samples: "chunked_pools" has max_paths 3 x 3072, one pixel group and passes
of samples {1-3, 4-6, 7-8}; max_samples 5 ends inside the second pass, 6 on its border.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, RrtPanic, Scene, resolve_rgba8, scenes, write_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PLANES = ("albedo", "normal", "depth")
GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
ROT = {"rotation_axis": [1.0, 2.0, 0.5], "rotation_angle": 25.0}
STATS = ("camera_samples", "camera_rays", "closest_queries", "any_queries", "root_culled", "sky_culled", "tile_launches", "list_launches")
SHORTCUTS = ("tile_trees", "tile_order", "quad_nodes", "lens_cull", "aux_margin", "root_cull")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_prototype_is_in_the_header_and_the_abi_version_stays():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    assert "int rrt_render_frame_aov(rrt_handle*, const int32_t rect[4], int rank, int world, void* film_xyzw, void* moments" in flat
    assert "uint64_t aov_max_samples, rrt_aov* aov, rrt_render_stats* stats" in flat
    assert "#define RRT_ABI_VERSION 11" in flat
    assert "rrt_render_frame_aov" in A.PROTOTYPES
    assert hasattr(A.lib(), "rrt_render_frame_aov")


def test_render_frame_aov_refuses_bad_arguments_without_a_device():
    """No device is needed to be told so: each NULL argument, an rrt_aov that asks for no plane, a bad mem and planes in another memory kind than
    the film are RRT_EINVAL, each with its own message, and nothing is written."""
    lib = A.lib()
    film, plane = np.zeros(4, np.float32), np.zeros(4, np.float32)
    rect = (C.c_int32 * 4)(0, 0, 1, 1)
    good = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, plane.ctypes.data, None, None)
    fake = None            # the caller's own arguments are judged before the handle is

    def call(h, r, f, mem, aov):
        return lib.rrt_render_frame_aov(h, r, 0, 1, f, None, mem, 0, aov, None)

    assert call(fake, None, film.ctypes.data, A.RRT_MEM_HOST, C.byref(good)) == A.RRT_EINVAL and b"null rect" in lib.rrt_last_error()
    assert call(fake, rect, None, A.RRT_MEM_HOST, C.byref(good)) == A.RRT_EINVAL and b"null film" in lib.rrt_last_error()
    assert call(fake, rect, film.ctypes.data, A.RRT_MEM_HOST, None) == A.RRT_EINVAL and b"rrt_aov" in lib.rrt_last_error()
    empty = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, None, None, None)
    assert call(fake, rect, film.ctypes.data, A.RRT_MEM_HOST, C.byref(empty)) == A.RRT_EINVAL and b"no plane" in lib.rrt_last_error()
    assert call(fake, rect, film.ctypes.data, 2, C.byref(good)) == A.RRT_EINVAL and b"bad mem" in lib.rrt_last_error()
    assert call(fake, rect, film.ctypes.data, A.RRT_MEM_DEVICE, C.byref(good)) == A.RRT_EINVAL and b"aov->mem != mem" in lib.rrt_last_error()
    assert call(None, rect, film.ctypes.data, A.RRT_MEM_HOST, C.byref(good)) == A.RRT_EINVAL and b"null handle" in lib.rrt_last_error()
    assert np.all(film == 0) and np.all(plane == 0)


# ---- GPU: scenes -------------------------------------------------------------------------------------------------------------------------------------

def _bands(world):
    return tuple(("band", k, world) for k in range(world))


def _cfg5(wd, film, nsamp):
    return scenes.cfg5(wd, xres=film[0], yres=film[1], nsamp=nsamp, max_depth=8, n=64)


def _cfg3_tilted(wd, nsamp=9):
    cfg, root = scenes.cfg3(wd, xres=64, yres=64, nsamp=nsamp, max_depth=5)
    cfg["Aggregate"]["primitives"][0]["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
    cfg["Aggregate"]["primitives"][1]["instances"] = [{"world_pos": [0.0, 0.0, 0.0], "rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}]
    return cfg, root


def _const_rgb(name, v):
    return {"texture_name": name, "texture_type": "BilerpTexture", "v00": {"values": v}, "v01": {"values": v}}


def _textured(wd):
    """tests/test_aov.py's textured cfg3: uv and 3D checkerboards, Scale and Mix, on the instanced cube (Mirror) and enclosure (Matte)."""
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


def _textured_direct(wd):
    """the same under DirectLighting: the per-sample recursion kernel, no camera queue - the call runs rrt_render_aov's own pass after the frame"""
    cfg, root = _textured(wd)
    cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3}
    return cfg, root


def _stratified(wd):
    cfg, root = _cfg5(wd, (48, 40), 5)
    cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 3, "ysamp": 4, "jitter": True, "dimension": 4}
    return cfg, root


def _ao(wd):
    cfg, root = _cfg5(wd, (64, 48), 9)
    cfg["Integrator"] = {"integrator_type": "AO"}
    return cfg, root


def _case(build, parts=(None,), filt=None, max_paths=None, max_samples=(0,), flags=RRT_FIXED_BVH, precs=("f32", "f64"), misses=True, culled=False, lit=True):
    """misses: the planes hold live samples that hit nothing; culled: the frame's root cull and tile trees are at work; lit: the frame is not black"""
    return dict(build=build, parts=tuple(parts), filt=filt, max_paths=max_paths, max_samples=tuple(max_samples), flags=flags, precs=precs, misses=misses, culled=culled, lit=lit)


CASES = {
    "cfg5_whole": _case(lambda wd: _cfg5(wd, (64, 48), 25)),
    # a default fp32 handle: tile trees and the root cull are fp32 shortcuts
    "cfg5_root_cull": _case(lambda wd: _cfg5(wd, (128, 96), 25), precs=("f32",), culled=True),
    "rect_off_tile": _case(lambda wd: _cfg5(wd, (136, 104), 25), parts=[(5, 3, 101, 67)]),
    "bands_world3": _case(lambda wd: _cfg5(wd, (128, 104), 9), parts=_bands(3)),
    "gauss_rect_off": _case(lambda wd: _cfg5(wd, (136, 104), 9), parts=[(5, 3, 101, 67)], filt=GAUSS),
    "small_pools": _case(lambda wd: _cfg5(wd, (64, 48), 9), max_paths=1000, max_samples=(0, 5, 3)),
    "chunked_pools": _case(lambda wd: _cfg5(wd, (64, 48), 9), max_paths=3 * 64 * 48, max_samples=(5, 6)),
    "max_samples_8": _case(lambda wd: _cfg5(wd, (64, 48), 25), max_samples=(8,)),
    "stratified": _case(_stratified),
    "textured_cfg3": _case(_textured, flags=0, misses=False),       # (the enclosure of cfg3 leaves no misses)
    "cfg1_spheres": _case(lambda wd: scenes.cfg1(wd, xres=64, yres=64, nsamp=9), flags=0),      # DirectLighting: the level loop's queue
    "fallback_ao": _case(_ao, lit=False),       # (an AO frame traces nothing on the device: its film holds the filter weights and no radiance, in every call)
    "fallback_direct_tree": _case(_textured_direct, flags=0, misses=False),
}
PARAMS = [pytest.param(name, prec, id=f"{name}-{prec}") for name in sorted(CASES) for prec in CASES[name]["precs"]]
PREC = {"f32": RRT_F32, "f64": RRT_F64}

_scenes = {}


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


def _two_calls(r, max_samples=0, **part):
    film, mom, st = r.render_moments(stats=True, **part)
    return film, mom, r.render_aov(max_samples=max_samples, **part), st


def _assert_same(fused, two, what):
    film, mom, aov, st = fused
    film2, mom2, aov2, st2 = two
    assert np.array_equal(film, film2), (what, "film")
    assert np.array_equal(mom, mom2), (what, "moments")
    for plane in PLANES:
        assert np.array_equal(aov[plane], aov2[plane]), (what, plane)
    for key in STATS:
        assert getattr(st, key) == getattr(st2, key), (what, key, getattr(st, key), getattr(st2, key))


# ---- GPU: tests --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,prec", PARAMS)
def test_fused_equals_the_two_calls(name, prec, workdir):
    c = CASES[name]
    r = Renderer(_scene(name, workdir), 0, PREC[prec])
    if c["max_paths"]: r.set_option("max_paths", c["max_paths"])
    for k in c["max_samples"]:
        for part in c["parts"]:
            args = _part_args(part)
            two = _two_calls(r, max_samples=k, **args)
            fused = r.render_frame_aov(max_samples=k, stats=True, **args)
            what = (name, prec, k, part)
            aov, st = two[2], two[3]
            assert aov["depth"][..., 2].max() > 0 and two[0][..., 3].max() > 0, what        # neither the planes nor the frame are empty
            if c["lit"]: assert two[0][..., :3].max() > 0, what
            if c["misses"]: assert (aov["albedo"][..., 3] > aov["depth"][..., 2]).any(), what
            if c["culled"]: assert st.root_culled > 0 and st.tile_launches > 0, what
            print(f"{what}: live {aov['albedo'][..., 3].sum()}, hit {aov['depth'][..., 2].sum()}, root_culled {st.root_culled}, tile_launches {st.tile_launches}")
            _assert_same(fused, two, what)
    r.close()


@pytest.mark.gpu
def test_moments_plane_and_feature_planes_are_optional(workdir):
    """moments=False: the film is still the moments frame's; one plane asked for: that plane alone; arrays handed in are added to."""
    r = Renderer(_scene("cfg5_whole", workdir), 0, RRT_F32)
    film2, _, aov2, _ = _two_calls(r)
    film, mom, aov = r.render_frame_aov(moments=False, planes=("depth",))
    assert mom is None and set(aov) == {"depth"}
    assert np.array_equal(film, film2) and np.array_equal(aov["depth"], aov2["depth"])
    seven = np.full_like(film2, 7.0)
    film3, _, _ = r.render_frame_aov(film=seven, moments=False)
    r.close()
    assert film3 is seven and np.array_equal(seven, np.float32(7.0) + film2)


@pytest.mark.gpu
def test_fused_after_a_stale_pass(workdir):
    """One handle: a fused call over the rows richest in hits, then one over rows of the same shape whose camera rays mostly leave the scene (sky
    rows of cfg5, root-culled on a default fp32 handle). The second call's culled samples own slots the first call wrote hit records into."""
    r = Renderer(_scene("cfg5_root_cull", workdir), 0, RRT_F32)
    whole = r.render_aov()      # the existing call picks the rows: 16-row strips by their hit and miss weights
    hit = whole["depth"][..., 2].reshape(6, 16, -1).sum((1, 2))
    live = whole["albedo"][..., 3].reshape(6, 16, -1).sum((1, 2))
    full, sky = int(np.argmax(hit)), int(np.argmax(live - hit))
    print(f"hit weight per strip {hit}, live weight per strip {live}: strips {full} and {sky}")
    assert full != sky and hit[full] > hit[sky] and (live - hit)[sky] > 0.5 * live[sky], (hit, live)
    rects = [(0, 16 * k, 128, 16 * k + 16) for k in (full, sky)]
    got = [r.render_frame_aov(rect=rc, stats=True) for rc in rects]
    want = [_two_calls(r, rect=rc) for rc in rects]
    r.close()
    assert want[1][3].root_culled > 0
    for g, w, rc in zip(got, want, rects):
        _assert_same(g, w, rc)


@pytest.mark.gpu
def test_handle_is_left_as_it_was(workdir):
    """render, render_frame_aov, render on one default fp32 handle (tile trees, film records, root and horizon cull all on): the same frame twice."""
    r = Renderer(_scene("cfg5_root_cull", workdir), 0, RRT_F32)
    a, sa = r.render(stats=True)
    film, _, aov = r.render_frame_aov()
    b, sb = r.render(stats=True)
    r.close()
    assert aov["depth"][..., 2].max() > 0 and a[..., :3].max() > 0
    assert sa.tile_launches > 0 and sa.root_culled > 0
    assert np.array_equal(a, b) and np.array_equal(a, film)
    for key in STATS:
        assert getattr(sa, key) == getattr(sb, key), key


@pytest.mark.gpu
def test_shortcuts_change_no_bit(workdir):
    """tile_trees, tile_order, quad_nodes, lens_cull, aux_margin and root_cull off together: the same planes from the fused call."""
    r = Renderer(_scene("cfg5_root_cull", workdir), 0, RRT_F32)
    _, _, fast, st = r.render_frame_aov(stats=True)
    assert st.tile_launches > 0 and st.root_culled > 0
    for k in SHORTCUTS: r.set_option(k, 0)
    _, _, plain, st0 = r.render_frame_aov(stats=True)
    r.close()
    assert st0.tile_launches == 0 and st0.root_culled == 0
    assert fast["depth"][..., 2].max() > 0
    for plane in PLANES:
        assert np.array_equal(fast[plane], plain[plane]), plane


@pytest.mark.gpu
def test_error_paths(workdir):
    import torch
    cfg, root = _cfg5(workdir, (64, 48), 9)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    lib = A.lib()
    for rect in ((0, 0, 65, 48), (-1, 0, 64, 48), (10, 10, 10, 20)):
        with pytest.raises(RrtError, match="rect outside the film"):
            r.render_frame_aov(rect=rect)
    for rank, world in ((0, 0), (2, 2), (-1, 1)):
        with pytest.raises(RrtError, match="rank/world"):
            r.render_frame_aov(rank=rank, world=world)
    film = np.zeros((48, 64, 4), np.float32)
    plane = np.zeros((48, 64, 4), np.float64)
    wrong = A.Aov(A.RRT_MEM_HOST, A.RRT_F64, plane.ctypes.data, None, None)
    full = (C.c_int32 * 4)(0, 0, 64, 48)
    assert lib.rrt_render_frame_aov(r._h, full, 0, 1, film.ctypes.data, None, A.RRT_MEM_HOST, 0, C.byref(wrong), None) == A.RRT_EINVAL
    assert b"precision" in lib.rrt_last_error()
    frame = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, frame.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_frame_aov(film=film)
    r.render_end()
    assert np.all(film == 0) and np.all(plane == 0)
    # device buffers, += : two calls leave twice the sums of the host call
    dev = [torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0") for _ in range(5)]
    torch.cuda.synchronize()
    for _ in range(2):
        r.render_frame_aov_device((0, 0, 64, 48), *[d.data_ptr() for d in dev])
    f, m, aov = r.render_frame_aov()
    r.close()
    for d, h in zip(dev, (f, m, aov["albedo"], aov["normal"], aov["depth"])):
        assert np.array_equal(d.cpu().numpy(), h + h)
    # a scene rrt_render_rect refuses: DirectLighting without lights panics on a miss (Q20), though rrt_render_aov alone renders it
    cfg, root = scenes.cfg2(workdir, xres=32, yres=32, nsamp=3)
    cfg["Integrator"] = {"integrator_type": "DirectLighting"}
    cfg["lights"] = []
    r = Renderer(Scene.loads(cfg, root), 0, RRT_F32)
    with pytest.raises(RrtPanic):
        r.render()
    with pytest.raises(RrtPanic):
        r.render_frame_aov()
    r.close()


@pytest.mark.gpu
def test_cli_route(tmp_path):
    """RRT_DENOISE + RRT_DENOISE_MOMENTS on one GPU go through rrt_render_frame_aov: rrt_render and `python -m rs_ray_toy_amd` write, byte for byte, the
    frame and the denoised frame that the two-call route (render_moments, render_aov(max_samples=32), denoise) writes from Python."""
    import sys
    cfg, root = _cfg5(str(tmp_path), (64, 48), 41)       # more samples than the 32 the planes take
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    sc = Scene.loads(cfg, root)
    r = Renderer(sc, 0, RRT_F32)
    film, mom = r.render_moments()
    dn = r.denoise(film, r.render_aov(max_samples=32), moments=mom)
    r.close()
    write_png(str(tmp_path / "want.png"), resolve_rgba8(film, sc.desc.film.scale))
    write_png(str(tmp_path / "want_dn.png"), resolve_rgba8(dn, sc.desc.film.scale))
    want = ((tmp_path / "want.png").read_bytes(), (tmp_path / "want_dn.png").read_bytes())
    assert want[0] != want[1]
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    base = {k: v for k, v in os.environ.items() if k not in ("RRT_DENOISE", "RRT_DENOISE_MOMENTS", "RRT_AOV", "RRT_GPUS", "RRT_ADAPTIVE", "RRT_PRECISION", "RRT_FIXED_BVH")}
    base["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
        frame, out = tmp_path / f"{tag}.png", tmp_path / f"{tag}_dn.png"
        p = subprocess.run(cmd + [str(scene), str(frame)], capture_output=True, text=True, timeout=600, env=dict(base, RRT_DENOISE=str(out), RRT_DENOISE_MOMENTS="1"))
        assert p.returncode == 0, p.stderr
        assert frame.read_bytes() == want[0], tag
        assert out.read_bytes() == want[1], tag
