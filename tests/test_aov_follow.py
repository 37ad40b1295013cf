"""Feature buffers through mirrors and glass (rrt_render_aov_follow, include/rrt.h): the planes of rrt_render_aov with the record of the first
non-specular surface along the chain of perfectly specular bounces.

CPU tests: the prototype, the argument checks that need no device, the numpy reference (tests/aov_follow_reference.py) pinned to the oracle's own
frame path - in a scene whose every surface is a Mirror of Kr = 1, without lights, the Path integrator of max_depth K with rr_threshold 0 traces
exactly the segments the chain traces with max_follow = K - and known answers of the refraction rule.

GPU tests, against that reference (scenes: tests/aov_follow_scenes.py; every case's reference asserts that it holds the chains the case is about):
  test_f64_planes_match_reference      the bars of test_aov.py::test_f64_planes_match_reference
  test_fp32_planes_close_to_reference  the bars of test_aov.py::test_fp32_planes_close_to_reference
  bit for bit in both precisions: max_follow 0 and a scene without specular materials against rrt_render_aov, the weight channels at every
  max_follow, rects and bands against the whole, the shortcuts off, persistent_traversal 0 against 3; the handle left as it was; the error
  paths; the CLI variable RRT_AOV_FOLLOW on both hosts; and the reason for the feature: rrt_denoise guided by followed planes is closer to the
  converged frame on the mirror's pixels than guided by first-hit planes.
"""
import collections
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_follow_reference as FR
import aov_follow_scenes as FS
import oracle_lib as O
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PLANES = ("albedo", "normal", "depth")
GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
SHORTCUTS = ("tile_trees", "tile_order", "quad_nodes", "lens_cull", "aux_margin")
PRECS = pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_prototype_is_declared_and_exported():
    with open(HEADER) as f:
        text = f.read()
    assert "#define RRT_ABI_VERSION 11" in text
    assert "int rrt_render_aov_follow(rrt_handle*, const int32_t rect[4], int rank, int world, uint64_t max_samples, uint32_t max_follow, rrt_aov* out);" in text
    assert "rrt_render_aov_follow" in A.PROTOTYPES
    restype, argtypes = A.PROTOTYPES["rrt_render_aov_follow"]
    assert restype is C.c_int and argtypes[4:6] == [C.c_uint64, C.c_uint32] and len(argtypes) == 7
    assert A.lib().rrt_render_aov_follow is not None


def test_refuses_bad_arguments_without_a_device():
    """A NULL rrt_aov, an rrt_aov that asks for no plane, a NULL rect, a NULL handle and max_follow = 17 are RRT_EINVAL, each with its own
    message, before any device work; nothing is written."""
    lib = A.lib()
    plane = np.zeros(4, np.float32)
    rect = (C.c_int32 * 4)(0, 0, 1, 1)
    good = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, plane.ctypes.data, None, None)
    empty = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, None, None, None)
    fake = C.c_void_p(1)       # never dereferenced: max_follow is refused first
    seen = []
    for args, word in (((None, rect, 0, 1, 0, 4, None), b"rrt_aov"), ((None, rect, 0, 1, 0, 4, C.byref(empty)), b"no plane"),
                       ((None, None, 0, 1, 0, 4, C.byref(good)), b"null rect"), ((None, rect, 0, 1, 0, 4, C.byref(good)), b"null handle"),
                       ((fake, rect, 0, 1, 0, 17, C.byref(good)), b"max_follow")):
        assert lib.rrt_render_aov_follow(*args) == A.RRT_EINVAL
        msg = lib.rrt_last_error()
        assert word in msg and b"rrt_render_aov_follow" in msg, msg
        seen.append(msg)
    assert len(set(seen)) == len(seen)
    assert np.all(plane == 0)


@pytest.mark.parametrize("K", [1, 4])
def test_reference_chain_is_the_oracles_path(K, workdir):
    """Every surface a Mirror of Kr = 1, no lights, Path {max_depth K, rr_threshold 0}: beta stays 1, nothing is sampled but the specular lobe, no
    path is terminated early, so the closest-hit queries of the oracle's frame are the segments of the reference's chains with max_follow = K."""
    cfg, root = FS.all_mirrors(workdir)
    cfg["Integrator"] = {"integrator_type": "Path", "max_depth": K, "rr_threshold": 0.0}
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    _, st = O.render(sc, stats=True)
    s = FR.planes(sc, K)["samples"]
    live = s["live"]
    assert st.camera_rays == live.sum() and st.any_queries == 0
    assert (s["levels"][live] == K + 1).sum() > 20 and (s["levels"][live] == 0).sum() > 20      # whole chains and plain misses
    if K > 1: assert ((s["levels"][live] > 1) & (s["levels"][live] <= K)).sum() > 20             # chains that leave the mirrors
    assert st.closest_queries == s["segments"]


def test_refraction_known_answers():
    """Snell's ratio sin(theta_t) = sin(theta_i) / eta entering and sin(theta_i) x eta leaving, at two angles each, the refracted ray in the plane
    of incidence on the far side; beyond the critical angle of eta = 1.5 (41.81 degrees) no refracted direction when leaving."""
    eta = 1.5
    sn = np.array([[0.0, 1.0, 0.0]])
    for deg in (20.0, 55.0):
        th = np.radians(deg)
        d_in = np.array([[np.sin(th), -np.cos(th), 0.0]])        # from above, against sn
        ok, wt, entering = FR.glass_direction(d_in, sn, np.array([eta]))
        assert ok[0] and entering[0]
        np.testing.assert_allclose(np.linalg.norm(wt[0]), 1.0, rtol=1e-14)
        np.testing.assert_allclose(wt[0, 0], np.sin(th) / eta, rtol=1e-14)
        assert wt[0, 1] < 0 and wt[0, 2] == 0
    for deg in (20.0, 40.0):
        th = np.radians(deg)
        d_out = np.array([[np.sin(th), np.cos(th), 0.0]])        # from below, along sn
        ok, wt, entering = FR.glass_direction(d_out, sn, np.array([eta]))
        assert ok[0] and not entering[0]
        np.testing.assert_allclose(wt[0, 0], np.sin(th) * eta, rtol=1e-14)
        assert wt[0, 1] > 0 and wt[0, 2] == 0
    for deg in (42.0, 60.0, 85.0):
        th = np.radians(deg)
        ok, _, entering = FR.glass_direction(np.array([[np.sin(th), np.cos(th), 0.0]]), sn, np.array([eta]))
        assert not ok[0] and not entering[0]
    assert FR.glass_direction(np.array([[np.sin(np.radians(41.5)), np.cos(np.radians(41.5)), 0.0]]), sn, np.array([eta]))[0][0]
    # the mirror rule on the same normal
    np.testing.assert_allclose(FR.reflect(np.array([[0.6, -0.8, 0.0]]), sn), [[0.6, 0.8, 0.0]], rtol=1e-15)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

def _bands(world):
    return tuple(("band", k, world) for k in range(world))


def _case(build, follow, expect, parts=(None,), filt=None, max_paths=None):
    """expect: what the case is about - ends of chains ('surface+': a chain of two or more surfaces that ends on one that is not followed, 'miss',
    'exhausted') and follow events ('mirror', 'enter', 'leave', 'tir') that its reference must hold; textured: the TEX kernels"""
    return dict(build=build, follow=follow, expect=tuple(expect), parts=tuple(parts), filt=filt, max_paths=max_paths)


CASES = {
    "mirror_floor_1": _case(FS.mirror_floor, 1, ("surface+", "miss", "mirror")),
    "mirror_floor_4": _case(FS.mirror_floor, 4, ("surface+", "miss", "mirror")),
    "facing_mirrors": _case(FS.facing_mirrors, 4, ("surface+", "miss", "exhausted", "mirror", "deep")),
    "glass_cube": _case(FS.glass_cube, 4, ("surface+", "miss", "enter", "leave", "tir")),
    "textured_kr": _case(FS.textured_kr, 4, ("surface+", "miss", "mirror", "tints")),
    "gauss_rect_off": _case(lambda wd: FS.mirror_floor(wd, (136, 104)), 4, ("surface+", "miss"), parts=[(5, 3, 101, 67)], filt=GAUSS),
    "bands_world3": _case(lambda wd: FS.facing_mirrors(wd, (128, 104)), 4, ("surface+", "miss", "exhausted"), parts=_bands(3)),
    "small_pools": _case(FS.mirror_floor, 4, ("surface+", "miss"), max_paths=1000),       # four pixel groups x eight sample chunks: slots reused
}

_scenes, _refs = {}, {}


def _scene(name, workdir):
    if name not in _scenes:
        c = CASES[name]
        cfg, root = c["build"](workdir)
        if c["filt"]: cfg["Film"]["Filter"] = dict(c["filt"])
        _scenes[name] = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    return _scenes[name]


def _part_args(part):
    if part is not None and part[0] == "band": return dict(rect=None, rank=part[1], world=part[2])
    return dict(rect=part, rank=0, world=1)


def _assert_holds(name, samples_list):
    """the reference of a case holds the chains the case is about"""
    ends, events, levels, tints = collections.Counter(), collections.Counter(), collections.Counter(), set()
    for s in samples_list:
        live = s["live"]
        ends.update(s["end"][live])
        ends["surface+"] += int(((s["end"] == "surface") & (s["levels"] >= 2) & live).sum())
        levels.update(s["levels"][live])
        for e in s["events"]: events.update(e)
        tints.update(map(tuple, np.unique(s["rho"][live & (s["levels"] >= 2)].round(6), axis=0)))
    print(f"{name}: ends {dict(ends)}, events {dict(events)}, surfaces per chain {dict(levels)}")
    for key in CASES[name]["expect"]:
        if key == "deep": assert sum(v for k, v in levels.items() if k >= 3) >= 10, levels
        elif key == "tints": assert len(tints) >= 4, tints      # two checker colours of the mirror's Kr times the surfaces behind it
        elif key in ("mirror", "enter", "leave", "tir"): assert events[key] >= 10, (key, events)
        else: assert ends[key] >= 10, (key, ends)


def _reference(name, workdir):
    if name not in _refs:
        sc, c = _scene(name, workdir), CASES[name]
        total, samples = None, []
        for part in c["parts"]:
            p = FR.planes(sc, c["follow"], **_part_args(part))
            samples.append(p.pop("samples"))
            total = p if total is None else {k: total[k] + p[k] for k in p}
        _assert_holds(name, samples)
        assert total["depth"][..., 2].max() > 0 and (total["albedo"][..., 3] > total["depth"][..., 2]).any()
        _refs[name] = total
    return _refs[name]


def _follow(r, follow, rect=None, rank=0, world=1, max_samples=0):
    """rrt_render_aov_follow into new host planes (Renderer.render_aov(follow=) takes rrt_render_aov at 0: here 0 goes through the new call too)"""
    W, H = r.scene.resolution
    out = {k: np.zeros((H, W, 4), r.dtype) for k in PLANES}
    aov = A.Aov(A.RRT_MEM_HOST, r.precision, *(out[k].ctypes.data for k in PLANES))
    rc = A.lib().rrt_render_aov_follow(r._h, (C.c_int32 * 4)(*(rect or (0, 0, W, H))), rank, world, max_samples, follow, C.byref(aov))
    assert rc == A.RRT_OK, A.lib().rrt_last_error()
    return out


def _device(name, workdir, prec):
    sc, c = _scene(name, workdir), CASES[name]
    r = Renderer(sc, 0, prec)
    if c["max_paths"]: r.set_option("max_paths", c["max_paths"])
    total = None
    for part in c["parts"]:
        p = r.render_aov(follow=c["follow"], **_part_args(part))
        total = p if total is None else {k: total[k] + p[k] for k in p}
    r.close()
    return total


def _channels(plane):
    """(value channels, weight channel, the magnitude each value channel is measured against) of a plane of rrt_aov."""
    if plane == "depth": return (0, 1), 2, "own"       # sum T, sum T^2 | sum fw
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
    spp = int(_scene(name, workdir).desc.sampler.samples_per_pixel) - 1
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
        if not (d < 1e-4).mean() >= 0.975: failures.append((plane, "share", (d < 1e-4).mean()))
        if not d.mean() < 1e-4: failures.append((plane, "mean", d.mean()))
        if not d.max() < 3e-2 * 256 / spp: failures.append((plane, "max", d.max()))
    assert abs(live - live_ref) <= 2e-5 * live_ref, (live, live_ref)
    assert not failures, failures


def _equal(a, b):
    for plane in PLANES:
        assert np.array_equal(a[plane], b[plane]), plane


@pytest.mark.gpu
@PRECS
def test_follow_0_and_no_specular_are_render_aov(prec, workdir):
    """max_follow = 0 adds the bits of rrt_render_aov (a mirror, glass and textured scene each), and so does max_follow = 4 on a scene without a
    specular material."""
    for build, follow in ((FS.textured_kr, 0), (FS.glass_cube, 0), (FS.facing_mirrors, 0), (FS.no_specular, 4)):
        cfg, root = build(workdir)
        r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, prec)
        first = r.render_aov()
        got = _follow(r, follow)
        r.close()
        assert first["depth"][..., 2].max() > 0
        _equal(got, first)


@pytest.mark.gpu
@PRECS
def test_weight_channels_are_render_aovs(prec, workdir):
    """albedo[3], normal[3] and depth[2] at every max_follow: the same fw in the same order as rrt_render_aov's - under a wide filter too"""
    for build, filt in ((FS.facing_mirrors, None), (FS.glass_cube, GAUSS)):
        cfg, root = build(workdir)
        if filt: cfg["Film"]["Filter"] = dict(filt)
        r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, prec)
        first = r.render_aov()
        changed = False
        for follow in (1, 2, 4, 16):
            got = _follow(r, follow)
            for plane in PLANES:
                wc = _channels(plane)[1]
                assert np.array_equal(got[plane][..., wc], first[plane][..., wc]), (plane, follow)
            changed = changed or not np.array_equal(got["depth"], first["depth"])
        r.close()
        assert changed      # (the values do move)


def _sum_parts(r, parts, follow):
    total = None
    for part in parts:
        p = _follow(r, follow, **_part_args(part))
        total = p if total is None else {k: total[k] + p[k] for k in p}
    return total


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("filt", [None, GAUSS], ids=["box", "gauss"])
def test_parts_sum_to_the_whole(prec, filt, workdir):
    """test_aov.py::test_parts_sum_to_the_whole with chains: bit for bit under the box filter, to the rounding of the differently ordered sums
    under a wide one."""
    cfg, root = FS.facing_mirrors(workdir, (128, 104))
    if filt: cfg["Film"]["Filter"] = dict(filt)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, prec)
    whole = _follow(r, 4)
    rects = _sum_parts(r, [(0, 0, 61, 50), (61, 0, 128, 50), (0, 50, 128, 104)], 4)
    bands = _sum_parts(r, _bands(3), 4)
    r.close()
    assert whole["depth"][..., 2].max() > 0
    rtol = 1e-12 if prec == RRT_F64 else 1e-5
    for plane in PLANES:
        for parts in (rects, bands):
            if filt is None:
                assert np.array_equal(parts[plane], whole[plane]), plane
            else:
                wc = _channels(plane)[1]
                assert np.array_equal(parts[plane][..., wc] != 0, whole[plane][..., wc] != 0)
                np.testing.assert_allclose(parts[plane][..., wc], whole[plane][..., wc], rtol=rtol, atol=0)
                np.testing.assert_allclose(parts[plane], whole[plane], rtol=rtol, atol=rtol * np.abs(whole[plane]).max())


@pytest.mark.gpu
def test_shortcuts_change_no_bit(workdir):
    """tile_trees, tile_order, quad_nodes, lens_cull and aux_margin off together: the same planes. The frame rendered first builds the tile trees,
    so the default call is the one whose level 0 uses them."""
    cfg, root = FS.facing_mirrors(workdir, (128, 96))
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    _, st = r.render(stats=True)
    assert st.tile_launches > 0
    fast = _follow(r, 4)
    for k in SHORTCUTS: r.set_option(k, 0)
    plain = _follow(r, 4)
    r.close()
    assert fast["depth"][..., 2].max() > 0
    _equal(fast, plain)


@pytest.mark.gpu
def test_persistent_traversal_changes_no_bit(workdir):
    planes = []
    for mode in (0, 3):
        cfg, root = FS.glass_cube(workdir)
        r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
        r.set_option("persistent_traversal", mode)
        planes.append(_follow(r, 4))
        r.close()
    assert planes[0]["depth"][..., 2].max() > 0
    _equal(planes[0], planes[1])


@pytest.mark.gpu
def test_handle_is_untouched(workdir):
    """frame, follow call, frame on one default fp32 handle: the same frame and statistics; and rrt_render_aov after a follow call is
    rrt_render_aov on a fresh handle."""
    cfg, root = FS.facing_mirrors(workdir, (128, 96))
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    a, sa = r.render(stats=True)
    followed = _follow(r, 3)       # an odd number of queue swaps per pass
    b, sb = r.render(stats=True)
    after = r.render_aov()
    r.close()
    assert followed["depth"][..., 2].max() > 0 and a[..., :3].max() > 0 and sa.tile_launches > 0
    assert np.array_equal(a, b)
    for key in ("camera_rays", "closest_queries", "any_queries", "tile_launches", "root_culled"):
        assert getattr(sa, key) == getattr(sb, key), key
    fresh = Renderer(sc, 0, RRT_F32)
    want = fresh.render_aov()
    fresh.close()
    _equal(after, want)


@pytest.mark.gpu
def test_error_paths(workdir):
    import torch
    cfg, root = FS.mirror_floor(workdir)
    r = Renderer(Scene.loads(cfg, root, flags=RRT_FIXED_BVH), 0, RRT_F32)
    lib = A.lib()
    for rect in ((0, 0, 65, 48), (-1, 0, 64, 48), (10, 10, 10, 20)):
        with pytest.raises(RrtError, match="rect outside the film"):
            r.render_aov(rect=rect, follow=2)
    with pytest.raises(RrtError, match="rank/world"):
        r.render_aov(rank=2, world=2, follow=2)
    plane = np.zeros((48, 64, 4), np.float64)
    wrong = A.Aov(A.RRT_MEM_HOST, A.RRT_F64, plane.ctypes.data, None, None)
    full = (C.c_int32 * 4)(0, 0, 64, 48)
    assert lib.rrt_render_aov_follow(r._h, full, 0, 1, 0, 2, C.byref(wrong)) == A.RRT_EINVAL and b"precision" in lib.rrt_last_error()
    with pytest.raises(RrtError, match="max_follow"):
        r.render_aov(follow=17)
    film = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, film.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_aov(follow=2)
    r.render_end()
    assert np.all(plane == 0)
    # device planes, and a single plane: += twice
    dev = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    only = A.Aov(A.RRT_MEM_DEVICE, A.RRT_F32, None, None, dev.data_ptr())
    for _ in range(2):
        assert lib.rrt_render_aov_follow(r._h, full, 0, 1, 0, 16, C.byref(only)) == A.RRT_OK, lib.rrt_last_error()
    host = r.render_aov(planes=("depth",), follow=16)
    assert set(host) == {"depth"}
    assert np.array_equal(dev.cpu().numpy(), host["depth"] + host["depth"])
    r.close()


def _mean_xyz(film):
    f = film.astype(np.float64)
    return f[..., :3] / np.where(f[..., 3:] > 0, f[..., 3:], 1.0)


@pytest.mark.gpu
def test_followed_planes_denoise_the_mirror_better(workdir):
    """The reason for the call. mirror_floor with a checker wall seen in the mirror, one fp32 handle: an 8-sample frame (rrt_render_adaptive
    stopped at 8 samples holds the bits of an 8-sample frame) filtered by rrt_denoise under first-hit planes and under max_follow = 4 planes, each
    against the handle's undenoised 1024-sample frame, RMS over the pixels whose live samples all meet the mirror first. Only the order of the
    two errors is asserted (measured: DESIGN.md section 6)."""
    cfg, root = FS.mirror_floor(workdir, (64, 48), 1025, wall_mat="m_chk")
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    s = FR.samples(sc, (0, 0, 64, 48), 1, max_samples=8)
    first_mirror = np.array([bool(e) and e[0] == "mirror" for e in s["events"]])
    n_live, n_mirror = np.zeros((48, 64)), np.zeros((48, 64))
    np.add.at(n_live, (s["py"], s["px"]), s["live"])
    np.add.at(n_mirror, (s["py"], s["px"]), s["live"] & first_mirror)
    mask = (n_live > 0) & (n_mirror == n_live)
    assert mask.sum() > 150
    r = Renderer(sc, 0, RRT_F32)
    noisy = r.render_adaptive(min_samples=8, max_samples=8, threshold=0.0)[0]
    converged = _mean_xyz(r.render())
    rms = {}
    for follow in (0, 4):
        out = r.denoise(noisy, r.render_aov(max_samples=8, follow=follow))
        err = (_mean_xyz(out) - converged)[mask]
        rms[follow] = float(np.sqrt((err * err).mean()))
    rms["noisy"] = float(np.sqrt((((_mean_xyz(noisy) - converged)[mask]) ** 2).mean()))
    r.close()
    print(f"mirror pixels {int(mask.sum())}: RMS error against 1024 spp: undenoised {rms['noisy']:.4e}, first-hit planes {rms[0]:.4e}, followed planes {rms[4]:.4e}")
    assert rms[4] < rms[0], rms


@pytest.mark.gpu
@pytest.mark.parametrize("host", ["cli", "py"])
def test_cli_follow_variable(host, tmp_path):
    """RRT_AOV_FOLLOW=4 on both hosts: RRT_AOV's albedo and depth images change (the mirror shows what it reflects), the frame does not, and the
    RRT_DENOISE / RRT_DENOISE_MOMENTS route writes its frame."""
    cfg, _ = FS.mirror_floor(str(tmp_path))
    scene = tmp_path / "aov_follow" / "scene.json"
    scene.write_text(json.dumps(cfg))
    cmd = [os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")] if host == "cli" else [sys.executable, "-m", "rs_ray_toy_amd"]
    base = {k: v for k, v in os.environ.items() if not k.startswith("RRT_")}
    base["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    out = {}
    for tag, extra in (("first", {}), ("follow", {"RRT_AOV_FOLLOW": "4", "RRT_DENOISE": str(tmp_path / "dn.png"), "RRT_DENOISE_MOMENTS": "1"})):
        env = dict(base, RRT_AOV=str(tmp_path / tag), **extra)
        p = subprocess.run(cmd + [str(scene), str(tmp_path / f"{tag}.png")], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr
        out[tag] = {k: (tmp_path / f"{tag}{k}.png").read_bytes() for k in ("", "_albedo", "_normal", "_depth")}
    assert out["first"][""] == out["follow"][""]
    assert out["first"]["_albedo"] != out["follow"]["_albedo"] and out["first"]["_depth"] != out["follow"]["_depth"]
    assert (tmp_path / "dn.png").stat().st_size > 0
    if host != "cli": return
    bad = subprocess.run(cmd + [str(scene), str(tmp_path / "bad.png")], capture_output=True, text=True, timeout=600,
                         env=dict(base, RRT_AOV=str(tmp_path / "bad"), RRT_AOV_FOLLOW="17"))
    assert bad.returncode != 0 and "max_follow" in bad.stderr + bad.stdout
