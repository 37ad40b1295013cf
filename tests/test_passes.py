"""Light-group and bounce passes beside the film (rrt_render_passes) and relighting from them (rrt_combine_passes), include/rrt.h.

The reference frames come from the unchanged f64 oracle through two identities (tests/passes_reference.py): a light's pass is the frame of the scene
with every other light black, a vertex range's pass is the difference of two frames of different depth. The scene is cfg4's heightfield (n = 32) under a
point light, two distant lights and a sphere area light, 24 x 16 px, nsamp 5; the variants change one thing each (passes_reference.VARIANTS) and CASES adds
how the frame is cut: two pool passes, bands with world 3 on the 128 x 40 film, device memory.

CPU tests: the exports and prototypes, every RRT_EINVAL that needs no handle, the reference pinned (single-light frames sum to the frame within 1e-13 of
its largest value, depth increments >= 0, weight channels equal), the combine formula on hand-made films.
GPU tests:
  test_plain_frame_holds_the_bars   rrt_render_rect's own frame of every test scene against the oracle at the bars the passes are held to
  test_passes_match_oracle          per-light, direct / indirect, a two-group and a light x bounce pass; colour within 1e-9 (f64) / 1e-4 (fp32, 4 spp) of the
                                    full oracle frame's largest value (test_frame_shapes.py's bars), weights equal (box) or equal support and rtol 1e-12 /
                                    1e-5 (Gaussian)
  test_frame_film_and_full_pass     film and the six statistics equal rrt_render_rect's, the full pass holds the film's bits, the handle is untouched
  test_partitions_sum_to_the_frame  per-light passes and {vertex 0, vertices >= 1}. Bound: a pixel's film value is a sum of n <= spp x D x (pixels under the
                                    filter) non-negative terms, added in another association by the passes: each order is within (n - 1) eps of the exact
                                    sum, the RGB -> XYZ rows add 3 products (4 eps), summing the pass films in f64 adds nothing in fp32 and (passes) eps
                                    in f64: |sum - frame| <= (2 n + 8) eps x frame, per pixel and channel
  test_cuts_give_the_same_passes    rects, bands and two pool passes: rtol 1e-12 (f64) / 1e-5 (fp32, test_gpu_parity.py's pass-sum bar)
  test_shortcuts_change_no_bit      INVARIANT_OPTIONS all off together, and overlap_shadow 0 / 1: identical pass bits (fp32)
  test_relighting_matches_the_formula  rrt_combine_passes of the four light passes under RGB gains against the numpy restatement (rtol 1e-12 / 1e-6), host
                                    and device memory, in place
  test_relighting_matches_oracle    the same film against the oracle frame of the scene with its spectra scaled, at the same bars
  test_device_side_errors, test_command_lines_write_the_passes
One RRT_EINVAL cannot be raised without a device: a light_group entry >= 32 is found by walking the handle's n_lights entries, and a handle needs a
device. It is checked in test_device_side_errors, before the handle does any device work (the buffers stay untouched).
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import passes_reference as PR
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError, RrtUnsupported
from test_frame_shapes import INVARIANT_OPTIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
ALL = 0xFFFFFFFF
STATS = ("camera_samples", "camera_rays", "closest_queries", "any_queries", "root_culled", "sky_culled")
# (groups, bounce_lo, bounce_hi): the four lights, direct, indirect, the two distant lights together, the area light at vertices 1 and 2, everything
PASSES = [(1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 0, 0), (ALL, 0, 1), (ALL, 1, 0), (0b0110, 0, 0), (8, 1, 3), (ALL, 0, 0)]
LIGHT, DIRECT, INDIRECT, FULL = (0, 1, 2, 3), 4, 5, 8
# name -> (variant, how the frame is rendered)
CASES = {"base": ("base", "whole"), "depth6": ("depth6", "whole"), "glass": ("glass", "whole"), "gauss": ("gauss", "whole"),
         "two_pool_passes": ("base", "max_paths"), "bands_world3": ("wide", "bands"), "device_memory": ("base", "device")}
PRECS = [RRT_F32, RRT_F64]
IDS = ["f32", "f64"]

_cfgs, _scenes, _refs, _films = {}, {}, {}, {}


def _cfg(variant, workdir):
    if variant not in _cfgs: _cfgs[variant] = PR.config(workdir, variant)
    return _cfgs[variant]


def _scene(variant, workdir):
    if variant not in _scenes: _scenes[variant] = PR.load(*_cfg(variant, workdir))
    return _scenes[variant]


def _ref(variant, workdir, k):
    """The oracle's frame of PASSES[k], computed once."""
    if (variant, k) not in _refs:
        cfg, root = _cfg(variant, workdir)
        _refs[(variant, k)] = PR.oracle_frame(cfg, root) if k == FULL else PR.pass_frame(cfg, root, *PASSES[k])
    return _refs[(variant, k)]


def _render_case(name, prec, workdir):
    """(frame film, [pass films], [stats of each call]) of a case, rendered once per precision."""
    if (name, prec) in _films: return _films[(name, prec)]
    variant, how = CASES[name]
    sc = _scene(variant, workdir)
    W, H = sc.resolution
    r = Renderer(sc, 0, prec)
    if how == "max_paths": r.set_option("max_paths", 24 * 16 * 2)      # 4 samples of 384 pixels: two pool passes
    if how == "bands":
        film, films, stats = np.zeros((H, W, 4), r.dtype), [np.zeros((H, W, 4), r.dtype) for _ in PASSES], []
        for rank in range(3):
            f, fs, st = r.render_passes(PASSES, rank=rank, world=3, stats=True)
            film += f; stats.append(st)
            for a, b in zip(films, fs): a += b
    elif how == "device":
        import torch
        dev = torch.zeros((len(PASSES) + 1, H, W, 4), dtype=torch.float32 if prec == RRT_F32 else torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        st = r.render_passes_device((0, 0, W, H), PASSES, [dev[1 + k].data_ptr() for k in range(len(PASSES))], film_ptr=dev[0].data_ptr())
        host = dev.cpu().numpy()
        film, films, stats = host[0], [host[1 + k] for k in range(len(PASSES))], [st]
    else:
        film, films, st = r.render_passes(PASSES, stats=True)
        stats = [st]
    r.close()
    _films[(name, prec)] = (film, films, stats)
    return _films[(name, prec)]


def _check_weights(variant, w, w_ref):
    """test_frame_shapes.py's _check_weights: equal for the box filter, equal support and rtol 1e-12 / 1e-5 for the Gaussian."""
    if PR.VARIANTS[variant][2] is None:
        assert np.array_equal(w.astype(np.float64), w_ref)
    else:
        assert np.array_equal(w != 0, w_ref != 0)
        np.testing.assert_allclose(w.astype(np.float64), w_ref, rtol=1e-12 if w.dtype == np.float64 else 1e-5, atol=0)


def _colour_bar(prec):
    return 1e-9 if prec == RRT_F64 else 1e-4      # test_frame_shapes.py:183, 218 (4 spp)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_and_abi_declares_both_calls():
    header = open(HEADER).read()
    for name in ("rrt_render_passes", "rrt_combine_passes"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in A.PROTOTYPES, name
        assert hasattr(A.lib(), name), name
    assert "#define RRT_ABI_VERSION 11" in header and "#define RRT_MAX_PASSES 16" in header
    assert A.RRT_MAX_PASSES == 16 and C.sizeof(A.Pass) == 24
    res, args = A.PROTOTYPES["rrt_render_passes"]
    assert res is C.c_int and len(args) == 10
    res, args = A.PROTOTYPES["rrt_combine_passes"]
    assert res is C.c_int and len(args) == 6


def test_render_passes_refuses_bad_arguments_without_a_device():
    """Each RRT_EINVAL with its own message, before the handle is used (`fake` is never dereferenced); the buffers stay untouched."""
    lib = A.lib()
    film = np.full((2, 2, 4), 7.0, np.float32)
    rect = (C.c_int32 * 4)(0, 0, 2, 2)
    fake = C.c_void_p(1)
    tab = lambda n=1, lo=0, ptr=film.ctypes.data: (A.Pass * 17)(*[A.Pass(ALL, lo, 0, ptr) for _ in range(n)])
    call = lambda h, rc, ps, n, mem=A.RRT_MEM_HOST: lib.rrt_render_passes(h, rc, 0, 1, None, ps, n, film.ctypes.data, mem, None)
    for args, msg in (((None, rect, tab(), 1), b"null handle"), ((fake, None, tab(), 1), b"null rect"), ((fake, rect, None, 1), b"null passes"),
                      ((fake, rect, tab(), 0), b"n_passes"), ((fake, rect, tab(17), 17), b"n_passes"), ((fake, rect, tab(2, 0, None), 2), b"null pass film"),
                      ((fake, rect, tab(), 1, 5), b"bad mem"), ((fake, rect, tab(3, -1), 3), b"bounce_lo")):
        assert call(*args) == A.RRT_EINVAL and msg in lib.rrt_last_error(), (msg, lib.rrt_last_error())
    assert np.all(film == 7.0)


def test_combine_passes_refuses_bad_arguments_without_a_device():
    lib = A.lib()
    film = np.full((2, 2, 4), 7.0, np.float32)
    fake = C.c_void_p(1)
    ptrs = lambda n, p=film.ctypes.data: (C.c_void_p * 17)(*[p] * n)
    gains = (C.c_double * 51)(*[1.0] * 51)
    call = lambda h, fs, g, n, out=film.ctypes.data, mem=A.RRT_MEM_HOST: lib.rrt_combine_passes(h, fs, g, n, out, mem)
    for args, msg in (((None, ptrs(1), gains, 1), b"null handle"), ((fake, None, gains, 1), b"null films"), ((fake, ptrs(1), None, 1), b"null gains"),
                      ((fake, ptrs(1), gains, 1, None), b"null output"), ((fake, ptrs(1), gains, 0), b"n must be"), ((fake, ptrs(17), gains, 17), b"n must be"),
                      ((fake, ptrs(2, None), gains, 2), b"null film ("), ((fake, ptrs(1), gains, 1, film.ctypes.data, 5), b"bad mem")):
        assert call(*args) == A.RRT_EINVAL and msg in lib.rrt_last_error(), (msg, lib.rrt_last_error())
    assert np.all(film == 7.0)


@pytest.mark.parametrize("variant", sorted(PR.VARIANTS))
def test_reference_is_pinned(variant, workdir):
    """The two identities on the oracle itself: the single-light frames sum to the frame within 1e-13 of its largest value with equal weight channels, and
    every extra unit of depth adds a non-negative increment in every pixel and channel, with equal weight channels."""
    cfg, root = _cfg(variant, workdir)
    full = _ref(variant, workdir, FULL)
    top = np.abs(full[..., :3]).max()
    assert top > 0
    lights = [_ref(variant, workdir, k) for k in LIGHT]
    for f in lights: assert np.array_equal(f[..., 3], full[..., 3])
    err = np.abs(sum(f[..., :3] for f in lights) - full[..., :3]).max() / top
    print(f"{variant}: single-light frames sum to the frame within {err:.3e}; shares {[float(f[..., :3].max() / top) for f in lights]}")
    assert err < 1e-13
    assert all(f[..., :3].max() > 0.01 * top for f in lights)
    prev = PR.oracle_frame(cfg, root, None, 0)
    assert not prev[..., :3].any() and np.array_equal(prev[..., 3], full[..., 3])
    for d in range(1, int(cfg["Integrator"]["max_depth"]) + 1):
        f = PR.oracle_frame(cfg, root, None, d)
        inc = f[..., :3] - prev[..., :3]
        print(f"{variant}: depth {d} adds {inc.max() / top:.4f} of the largest value, smallest increment {inc.min():.3e}")
        assert inc.min() >= 0 and np.array_equal(f[..., 3], full[..., 3])
        prev = f
    assert np.array_equal(prev, full)
    if variant == "depth6": assert inc.max() > 0      # vertex 5 is reached: Russian roulette has drawn on the way


def test_combine_reference_on_hand_made_films():
    """Unit gains give the sum of the films up to f64 rounding (the way back to RGB is the inverse of the way there); a gain on one film moves only
    that film's share; the weight channel is the first film's."""
    rng = np.random.default_rng(5)
    films = [rng.random((3, 5, 4)) for _ in range(3)]
    one = PR.combine(films, [[1, 1, 1]] * 3)
    np.testing.assert_allclose(one[..., :3], sum(f[..., :3] for f in films), rtol=1e-12, atol=1e-13)
    assert np.array_equal(one[..., 3], films[0][..., 3])
    two = PR.combine(films, [[1, 1, 1], [2, 2, 2], [1, 1, 1]])
    np.testing.assert_allclose(two[..., :3] - one[..., :3], films[1][..., :3], rtol=1e-12, atol=1e-13)
    assert not PR.combine(films, [0, 0, 0])[..., :3].any()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
@pytest.mark.parametrize("variant", sorted(PR.VARIANTS))
def test_plain_frame_holds_the_bars(variant, prec, workdir):
    """rrt_render_rect's own frame of every test scene holds the bars the passes are held to (a scene that did not would be changed, not the bar)."""
    ref = _ref(variant, workdir, FULL)
    r = Renderer(_scene(variant, workdir), 0, prec)
    film = r.render()
    r.close()
    _check_weights(variant, film[..., 3], ref[..., 3])
    diff = np.abs(film[..., :3].astype(np.float64) - ref[..., :3]).max() / np.abs(ref[..., :3]).max()
    print(f"{variant} {film.dtype}: plain frame vs oracle, max {diff:.3e}")
    assert diff < _colour_bar(prec), diff


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_passes_match_oracle(name, prec, workdir):
    variant = CASES[name][0]
    film, films, _ = _render_case(name, prec, workdir)
    full = _ref(variant, workdir, FULL)
    top = np.abs(full[..., :3]).max()
    for k, p in enumerate(PASSES):
        ref = _ref(variant, workdir, k)
        _check_weights(variant, films[k][..., 3], full[..., 3])
        diff = np.abs(films[k][..., :3].astype(np.float64) - ref[..., :3]).max() / top
        print(f"{name} {film.dtype}: pass {p} vs oracle, max {diff:.3e} of the frame's largest value; the pass's own largest {ref[..., :3].max() / top:.4f}")
        assert diff < _colour_bar(prec), (p, diff)
    assert all(_ref(variant, workdir, k)[..., :3].max() > 0 for k in range(len(PASSES)))      # no pass is compared with a black frame


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
@pytest.mark.parametrize("name", ["base", "gauss", "two_pool_passes", "bands_world3", "device_memory"])
def test_frame_film_and_full_pass(name, prec, workdir):
    """The frame film and the six statistics are rrt_render_rect's / rrt_render_bands'; the full pass holds the film's bits; a frame rendered before
    and after the call has the same bits; a NULL frame film gives the same passes."""
    variant, how = CASES[name]
    sc = _scene(variant, workdir)
    film, films, stats = _render_case(name, prec, workdir)
    r = Renderer(sc, 0, prec)
    if how == "max_paths": r.set_option("max_paths", 24 * 16 * 2)
    parts = [r.render_bands(k, 3, stats=True) for k in range(3)] if how == "bands" else [r.render(stats=True)]
    _, only, st2 = r.render_passes(PASSES[:2], rank=0, world=3 if how == "bands" else 1, film=None, stats=True)
    again = [r.render_bands(k, 3) for k in range(3)] if how == "bands" else [r.render()]
    r.close()
    plain = sum(p[0] for p in parts)
    assert plain[..., :3].max() > 0
    assert np.array_equal(film, plain)
    assert np.array_equal(films[FULL], plain)
    for st, (_, ref_st) in zip(stats, parts):
        assert [getattr(st, k) for k in STATS] == [getattr(ref_st, k) for k in STATS], [(k, getattr(st, k), getattr(ref_st, k)) for k in STATS]
    assert [getattr(st2, k) for k in STATS] == [getattr(parts[0][1], k) for k in STATS]
    for a, (b, _) in zip(again, parts): assert np.array_equal(a, b)
    if how != "bands":
        for k in range(2): assert np.array_equal(only[k], films[k])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_partitions_sum_to_the_frame(name, prec, workdir):
    variant = CASES[name][0]
    film, films, _ = _render_case(name, prec, workdir)
    cfg, _ = _cfg(variant, workdir)
    spp, D = int(cfg["Sampler"]["nsamp"]) - 1, int(cfg["Integrator"]["max_depth"])
    under_filter = 1 if PR.VARIANTS[variant][2] is None else 16      # a Gaussian of radius 1.5 reaches the samples of at most 4 x 4 pixels
    n = spp * D * under_filter
    bound = (2 * n + 8) * float(np.finfo(film.dtype).eps) * film[..., :3].astype(np.float64)
    assert film[..., :3].min() >= 0
    for what, ks in (("lights", LIGHT), ("direct + indirect", (DIRECT, INDIRECT))):
        total = sum(films[k][..., :3].astype(np.float64) for k in ks)
        over = np.abs(total - film[..., :3].astype(np.float64)) - bound
        used = np.abs(total - film[..., :3].astype(np.float64))[bound > 0] / bound[bound > 0]
        print(f"{name} {film.dtype}: {what} sum to the frame; at most {used.max():.3f} of the bound is used (bound up to {bound.max():.3e})")
        assert over.max() <= 0, (what, over.max())
        for k in ks: assert np.array_equal(films[k][..., 3], film[..., 3])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_cuts_give_the_same_passes(prec, workdir):
    """Rects, bands and two pool passes against the whole frame in one pool pass."""
    rtol = 1e-12 if prec == RRT_F64 else 1e-5      # test_gpu_parity.py:652's fp32 pass-sum bar
    _, whole, _ = _render_case("base", prec, workdir)
    _, pooled, _ = _render_case("two_pool_passes", prec, workdir)
    r = Renderer(_scene("base", workdir), 0, prec)
    rects = [np.zeros_like(whole[0]) for _ in PASSES]
    for rect in ((0, 0, 8, 16), (8, 0, 24, 8), (8, 8, 24, 16)):      # a tiled rect off the origin among them
        _, fs = r.render_passes(PASSES, rect=rect, film=None)
        for a, b in zip(rects, fs): a += b
    r.close()
    _, banded, _ = _render_case("bands_world3", prec, workdir)
    r = Renderer(_scene("wide", workdir), 0, prec)
    _, wide_whole = r.render_passes(PASSES, film=None)
    r.close()
    for what, got, want in (("two pool passes", pooled, whole), ("rects", rects, whole), ("bands", banded, wide_whole)):
        for k in range(len(PASSES)):
            assert want[k][..., :3].max() > 0
            np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=0, err_msg=f"{what}, pass {PASSES[k]}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base", "glass"])
def test_shortcuts_change_no_bit(name, workdir):
    """Every result-invariant shortcut off together, and one or two shadow queues: the pass films keep their bits (fp32)."""
    sc = _scene(CASES[name][0], workdir)
    _, films, _ = _render_case(name, RRT_F32, workdir)
    for options in (INVARIANT_OPTIONS, ("overlap_shadow",)):
        r = Renderer(sc, 0, RRT_F32)
        for key in options: r.set_option(key, 0)
        frame, plain = r.render_passes(PASSES)
        r.close()
        assert np.array_equal(frame, plain[FULL])
        for k in range(len(PASSES)): assert np.array_equal(plain[k], films[k]), (options, PASSES[k])


GAINS = [[0.25, 0.5, 1.0], [2.0, 1.0, 0.0], [0.0, 0.0, 0.0], [3.0, 3.0, 1.5]]
_relit = {}


def _relight(prec, workdir):
    """The four light passes of the base case combined under GAINS: host call, device call in place, unit gains - once per precision."""
    if prec not in _relit:
        import torch
        film, films, _ = _render_case("base", prec, workdir)
        lights = [films[k] for k in LIGHT]
        r = Renderer(_scene("base", workdir), 0, prec)
        out = r.combine_passes(lights, GAINS)
        dev = torch.from_numpy(np.stack(lights)).to("cuda:0")
        torch.cuda.synchronize()
        r.combine_passes_device([dev[k].data_ptr() for k in range(4)], GAINS, dev[2].data_ptr())      # in place, over an input that is not the first
        after = dev.cpu().numpy()
        unit = r.combine_passes(lights, 1.0)
        r.close()
        _relit[prec] = (film, lights, out, after, unit)
    return _relit[prec]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_relighting_matches_the_formula(prec, workdir):
    """rrt_combine_passes against the numpy restatement of its formula (rtol 1e-12 / 1e-6), host and device memory, in place, the weight channel."""
    film, lights, out, after, unit = _relight(prec, workdir)
    assert out.dtype == film.dtype and np.array_equal(out, after[2])
    for k in (0, 1, 3): assert np.array_equal(after[k], lights[k])      # the other inputs are read only
    assert np.array_equal(out[..., 3], film[..., 3])
    rtol = 1e-12 if prec == RRT_F64 else 1e-6
    np.testing.assert_allclose(out, PR.combine(lights, GAINS), rtol=rtol, atol=0)
    np.testing.assert_allclose(unit, PR.combine(lights, 1.0), rtol=rtol, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_relighting_matches_oracle(prec, workdir):
    """The reason for the call: the four light passes under RGB gains against the oracle's frame of the scene whose light spectra are scaled by them,
    at the frame's own bars (1e-9 in f64, 1e-4 in fp32).

    The way back to RGB is the f64 inverse of the rgb_to_xyz table the films were merged with: through the six-digit xyz_to_rgb table of
    spectrum.rs:2075-2082, an inverse of it only to 1.43e-6, the formula evaluated in numpy on the ORACLE's own single-light frames is 5.139e-7 away
    from the oracle's frame of the scaled scene, and a first version of the kernel measured the same 5.139e-7 in f64; with the inverse the same oracle
    frames give 2.3e-16."""
    cfg, root = _cfg("base", workdir)
    ref = PR.oracle_frame(cfg, root, GAINS)
    top = np.abs(_ref("base", workdir, FULL)[..., :3]).max()
    _, _, out, _, _ = _relight(prec, workdir)
    diff = np.abs(out[..., :3].astype(np.float64) - ref[..., :3]).max() / top
    print(f"{out.dtype}: relit frame vs the oracle's frame of the scaled scene, max {diff:.3e} of the unscaled frame's largest value")
    assert ref[..., :3].max() > 0 and diff < _colour_bar(prec), diff


@pytest.mark.gpu
def test_device_side_errors(workdir):
    import torch
    cfg, root = _cfg("base", workdir)
    r = Renderer(_scene("base", workdir), 0, RRT_F32)
    lib = A.lib()
    W, H = 24, 16
    film = np.full((H, W, 4), 7.0, np.float32)
    tab = (A.Pass * 1)(A.Pass(ALL, 0, 0, film.ctypes.data))
    call = lambda rect, rank, world, lg=None: lib.rrt_render_passes(r._h, (C.c_int32 * 4)(*rect), rank, world, lg, tab, 1, film.ctypes.data, A.RRT_MEM_HOST, None)
    groups = np.array([0, 1, 32, 3], np.uint8)
    assert call((0, 0, W, H), 0, 1, groups.ctypes.data) == A.RRT_EINVAL and b"light_group[2]" in lib.rrt_last_error()
    assert call((0, 0, W, H), 2, 2) == A.RRT_EINVAL and b"rank" in lib.rrt_last_error()
    assert call((0, 0, W, H), 0, 0) == A.RRT_EINVAL and b"rank" in lib.rrt_last_error()
    assert call((0, 0, W + 1, H), 0, 1) == A.RRT_EINVAL and b"outside the film" in lib.rrt_last_error()
    assert call((4, 4, 4, 8), 0, 1) == A.RRT_EINVAL and b"outside the film" in lib.rrt_last_error()
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, frame.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_passes([(ALL, 0, 0)])
    r.render_end()
    assert np.all(film == 7.0)
    # groups are a call argument: all four lights in group 5, and a pass that asks for group 5, is the frame
    _, (five, none) = r.render_passes([(1 << 5, 0, 0), (1 << 4, 0, 0)], light_group=[5, 5, 5, 5], film=None)
    plain = r.render()
    r.close()
    assert np.array_equal(five, plain) and not none[..., :3].any() and np.array_equal(none[..., 3], plain[..., 3])
    for edit, msg in ((lambda c: c["Integrator"].update(integrator_type="DirectLighting", light_strategy="all"), "Path integrator"),
                      (lambda c: c["Film"].update(max_sample_luminance=10.0), "max_sample_luminance")):
        c2 = PR.edited(cfg)
        edit(c2)
        r = Renderer(PR.load(c2, root), 0, RRT_F32)
        with pytest.raises(RrtUnsupported, match=msg):
            r.render_passes([(ALL, 0, 0)])
        assert r.render()[..., :3].max() > 0      # the handle still renders
        r.close()


@pytest.mark.gpu
def test_command_lines_write_the_passes(tmp_path):
    """RRT_PASSES=<prefix> in both command lines: direct, indirect and one PNG per light beside an unchanged frame; the light PNGs differ from each other."""
    cfg, _ = PR.config(str(tmp_path), "base")
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    base = {k: v for k, v in os.environ.items() if k not in ("RRT_PASSES", "RRT_DENOISE", "RRT_DENOISE_MOMENTS", "RRT_AOV", "RRT_GPUS", "RRT_ADAPTIVE", "RRT_FIXED_BVH", "RRT_PRECISION")}
    base["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    names = ["direct", "indirect"] + [f"light{i}" for i in range(4)]
    written = {}
    for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
        plain, frame, prefix = tmp_path / f"{tag}_plain.png", tmp_path / f"{tag}.png", tmp_path / f"{tag}_pass"
        for out, env in ((plain, {}), (frame, {"RRT_PASSES": str(prefix)})):
            p = subprocess.run(cmd + [str(scene), str(out)], capture_output=True, text=True, timeout=600, env=dict(base, **env))
            assert p.returncode == 0, p.stderr
        assert frame.read_bytes() == plain.read_bytes()
        written[tag] = [(tmp_path / f"{tag}_pass_{n}.png").read_bytes() for n in names]
        assert all(b[:8] == b"\x89PNG\r\n\x1a\n" for b in written[tag])
        assert len(set(written[tag])) == len(names)
        assert not (tmp_path / f"{tag}_pass_light4.png").exists()
    assert written["cli"] == written["py"]
