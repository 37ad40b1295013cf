"""Sample-variance plane beside the film (rrt_render_moments) and the denoiser that reads it (rrt_denoise_moments), include/rrt.h.

CPU tests: the exports and prototypes, the argument checks that need no device, the numpy references (tests/moments_reference.py) pinned to the
oracle's own frame path, the fallback to the spatial estimate, and the definition's quality on the oracle frames of test_denoise.py.

GPU tests. The render shapes are the smallest that reach each path of the film kernels (SHAPES below); the scene is the tilted config 3 of test_aov.py
(generic rotation axes, no exact ties; at 16 x 12 and nsamp 9, 189 of 192 pixels are lit and 69 % of the samples are dead, so both kinds of sample
are in every pixel), Path integrator, depth 5.
  test_f64_moments_match_reference      f64 mode, the project's f64 bar: every channel within 1e-9 of its own channel's largest magnitude; box S0, S3 equal
                                        exactly; wide S0, S3 equal support and rtol 1e-12
  test_film_is_the_plain_frames         both modes, every shape: np.array_equal with render / render_bands on a fresh buffer, the five statistics equal
  test_parts_sum_to_the_whole           box: bit-equal in both modes for rects, bands and the max_paths 256 case; Gaussian f64: rtol 1e-12
  test_shortcuts_change_no_bit          tile_trees, tile_order, film_records, shade_compact all on / all off (fp32)
  test_fp32_moments_close_to_reference  the film bar of test_frame_shapes.py::test_default_fp32_frame_close_to_oracle on the test's own film (max < 1e-4 of
                                        the plane's largest magnitude), then S1 at the same bar (the same numbers), S2 at twice that (an error eps in y
                                        relative to the largest y is at most 2 eps in y^2 relative to the largest y^2), box S0 and S3 exact
  test_large_pass_consistency           512 x 512, one and eight samples per pixel: k_film_box's path for passes of 2^18 pixels or more; no oracle
  test_handle_is_untouched, test_denoise_moments_*, test_end_to_end_f64, test_device_side_error_paths, test_cli_denoise_moments
The fp32 bar of rrt_denoise_moments against the numpy reference with fp32 records is test_denoise.py's, 4 x 1.234e-6 = 4.94e-6: only the once-rounded
v records are new arithmetic. Measured worst case on an MI355X: 1.385e-6 (131 x 77), 2.3e-7 (20 x 6) - inside that bar, which therefore stays.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aov_reference as AR
import denoise_reference as DR
import moments_reference as MR
import oracle_lib as O
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError, Scene, resolve_moments, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PLANES = ("albedo", "normal", "depth")
GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
STATS = ("camera_rays", "closest_queries", "any_queries", "root_culled", "sky_culled")
NEW = ("rrt_render_moments", "rrt_denoise_moments")


def _cfg3_tilted(wd, film, nsamp, filt=None):
    """test_aov.py's scene: cfg3 with the enclosure and the cube instanced under generic rotations (no exact box / face ties)."""
    cfg, root = scenes.cfg3(wd, xres=film[0], yres=film[1], nsamp=nsamp, max_depth=5)
    cfg["Aggregate"]["primitives"][0]["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
    cfg["Aggregate"]["primitives"][1]["instances"] = [{"world_pos": [0.0, 0.0, 0.0], "rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}]
    if filt: cfg["Film"]["Filter"] = dict(filt)
    return cfg, root


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_and_abi_declares_both_calls():
    header = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in A.PROTOTYPES, name
        assert hasattr(A.lib(), name), name
    assert "#define RRT_ABI_VERSION 11" in header
    res, args = A.PROTOTYPES["rrt_render_moments"]
    assert res is C.c_int and len(args) == 8
    res, args = A.PROTOTYPES["rrt_denoise_moments"]
    assert res is C.c_int and len(args) == 6


def test_render_moments_refuses_null_arguments():
    """No device is needed to be told so: a NULL handle, rect, film or moments is RRT_EINVAL, each with its own message; the buffers stay untouched."""
    lib = A.lib()
    film, mom = np.full(4, 7.0, np.float32), np.full(4, 7.0, np.float32)
    rect = (C.c_int32 * 4)(0, 0, 1, 1)
    fake = C.c_void_p(1)      # never dereferenced: every case below fails on a check before the handle is used
    assert lib.rrt_render_moments(None, rect, 0, 1, film.ctypes.data, mom.ctypes.data, A.RRT_MEM_HOST, None) == A.RRT_EINVAL
    assert b"null handle" in lib.rrt_last_error()
    assert lib.rrt_render_moments(fake, None, 0, 1, film.ctypes.data, mom.ctypes.data, A.RRT_MEM_HOST, None) == A.RRT_EINVAL
    assert b"null rect" in lib.rrt_last_error()
    assert lib.rrt_render_moments(fake, rect, 0, 1, None, mom.ctypes.data, A.RRT_MEM_HOST, None) == A.RRT_EINVAL
    assert b"null film" in lib.rrt_last_error()
    assert lib.rrt_render_moments(fake, rect, 0, 1, film.ctypes.data, None, A.RRT_MEM_HOST, None) == A.RRT_EINVAL
    assert b"null moments" in lib.rrt_last_error()
    assert lib.rrt_render_moments(fake, rect, 0, 1, film.ctypes.data, mom.ctypes.data, 5, None) == A.RRT_EINVAL
    assert b"bad mem" in lib.rrt_last_error()
    assert np.all(film == 7.0) and np.all(mom == 7.0)


def test_denoise_moments_refuses_bad_arguments_without_a_device():
    """rrt_denoise's checks under the new name, and one more: a NULL moments plane."""
    lib = A.lib()
    a = np.zeros(4, np.float32)
    out = np.full(4, 7.0, np.float32)
    good = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, a.ctypes.data, a.ctypes.data, a.ctypes.data)
    call = lambda film, aov, mom, p, o: lib.rrt_denoise_moments(None, film, aov, mom, p, o)
    assert call(a.ctypes.data, None, a.ctypes.data, None, out.ctypes.data) == A.RRT_EINVAL and b"rrt_aov" in lib.rrt_last_error()
    missing = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, a.ctypes.data, None, a.ctypes.data)
    assert call(a.ctypes.data, C.byref(missing), a.ctypes.data, None, out.ctypes.data) == A.RRT_EINVAL and b"three planes" in lib.rrt_last_error()
    bad = A.DenoiseParams(7, 1, 4.0, 32.0, 8.0)
    assert call(a.ctypes.data, C.byref(good), a.ctypes.data, C.byref(bad), out.ctypes.data) == A.RRT_EINVAL and b"iterations" in lib.rrt_last_error()
    assert call(None, C.byref(good), a.ctypes.data, None, out.ctypes.data) == A.RRT_EINVAL and b"null film" in lib.rrt_last_error()
    assert call(a.ctypes.data, C.byref(good), None, None, out.ctypes.data) == A.RRT_EINVAL and b"null moments" in lib.rrt_last_error()
    assert call(a.ctypes.data, C.byref(good), a.ctypes.data, None, out.ctypes.data) == A.RRT_EINVAL and b"null handle" in lib.rrt_last_error()
    assert b"rrt_denoise_moments" in lib.rrt_last_error()
    assert np.all(out == 7.0)


@pytest.mark.parametrize("filt", [None, GAUSS], ids=["box", "gauss"])
def test_reference_is_pinned_to_the_oracles_frame(filt, workdir):
    """The per-sample differences sum to the oracle's whole frame; S1 is the film's Y, S0 the film's weight / 3."""
    factory = lambda n: Scene.loads(*_cfg3_tilted(workdir, (16, 12), n, filt))
    ref = MR.moments(factory, 9)
    whole = O.render(factory(9))
    m, film = ref["moments"], ref["film"]
    for ch in range(4):
        err = np.abs(film[..., ch] - whole[..., ch]).max() / np.abs(whole[..., ch]).max()
        print(f"summed differences against the frame, channel {ch}: {err:.3e}")
        assert err < 1e-12
    assert whole[..., 1].max() > 0 and (whole[..., 1] > 0).sum() >= 180
    np.testing.assert_allclose(m[..., 0], whole[..., 1], rtol=0, atol=1e-12 * whole[..., 1].max())
    if filt is None:
        assert np.array_equal(m[..., 2], whole[..., 3] / 3.0) and np.array_equal(m[..., 2], m[..., 3]) and np.all(m[..., 2] == 8.0)
    else:
        np.testing.assert_allclose(m[..., 2], whole[..., 3] / 3.0, rtol=1e-12, atol=0)
        assert np.all(m[..., 3] > 0) and np.all(m[..., 3] < m[..., 2] ** 2)
    res = resolve_moments(m)
    assert np.all(res["n_eff"] >= 2) and np.all(res["variance_of_mean"] >= 0) and res["variance_of_mean"].max() > 0
    np.testing.assert_allclose(res["mean"] * m[..., 2], m[..., 0], rtol=1e-12, atol=0)


def test_reference_falls_back_to_the_spatial_estimate():
    film, aov = DR.synthetic(40, 24, seed=5)
    want = DR.denoise(film, **aov)
    few = np.zeros_like(film)
    few[..., 0] = film[..., 1]; few[..., 1] = film[..., 1] ** 2; few[..., 2] = 3.0; few[..., 3] = 6.0      # n_eff = 1.5 everywhere
    for plane in (np.zeros_like(film), few):
        assert np.array_equal(MR.denoise(film, **aov, moments=plane), want)
    assert np.array_equal(MR.denoise(film, **aov, moments=few, variance="spatial"), want)
    assert not np.array_equal(MR.denoise(film, **aov, moments=MR.synthetic_moments(film, 6)), want)


def test_synthetic_plane_reaches_every_branch():
    film, aov = DR.synthetic(131, 77, seed=1131)
    m = MR.synthetic_moments(film, 7)
    rec = DR.prepare(film, **aov)
    v, use = MR.sample_variance(rec, m)
    data = rec["data"]
    n_eff = np.where(m[..., 3] > 0, m[..., 2] ** 2 / np.where(m[..., 3] > 0, m[..., 3], 1.0), 0.0)
    assert use.any() and (data & ~use).any() and (~data).any()
    assert (data & (n_eff == 1.5)).any() and (data & (n_eff >= 2) & (m[..., 0] == 0)).any() and np.all(m[~data] == 0)
    assert np.all(np.isfinite(v)) and np.all(v >= 0)


ORACLE_CASES = {"cfg5": lambda wd, ns: scenes.cfg5(wd, xres=96, yres=64, nsamp=ns, max_depth=5, n=64),      # the three cases of test_denoise.py
                "cfg4": lambda wd, ns: scenes.cfg4(wd, xres=96, yres=64, nsamp=ns, max_depth=5, n=64),
                "cfg3": lambda wd, ns: scenes.cfg3(wd, xres=96, yres=64, nsamp=ns, max_depth=5)}


def _rgb(film):
    with np.errstate(all="ignore"):
        return np.where(film[..., 3:4] > 0, DR.xyz_to_rgb(film[..., :3] / film[..., 3:4]), 0.0)


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_definition_denoises_oracle_frames(name, workdir):
    """8 spp oracle frames against the 128 spp frame: RGB RMSE with the sample variance below the noisy frame's and not above the spatial variant's."""
    factory = lambda n: Scene.loads(*ORACLE_CASES[name](workdir, n))
    sc8, sc128 = factory(9), factory(129)
    noisy, clean = O.render(sc8), O.render(sc128)
    p = AR.planes(sc8)
    m = MR.moments(factory, 9)["moments"]
    planes = {k: p[k] for k in PLANES}
    spatial = MR.denoise(noisy, **planes, moments=m, variance="spatial")
    sample = MR.denoise(noisy, **planes, moments=m)
    rmse = lambda f: float(np.sqrt(((_rgb(f) - _rgb(clean)) ** 2).mean()))
    _, use = MR.sample_variance(DR.prepare(noisy, **planes), m)
    print(f"{name}: RGB RMSE against 128 spp: noisy {rmse(noisy):.4g}, spatial variance {rmse(spatial):.4g}, sample variance {rmse(sample):.4g}; "
          f"share of pixels on the sample variance {use.mean():.3f}")
    assert np.array_equal(spatial, DR.denoise(noisy, **planes))
    assert np.all(np.isfinite(sample))
    assert rmse(sample) < rmse(noisy)
    assert rmse(sample) <= rmse(spatial)


# ---- GPU: rrt_render_moments -------------------------------------------------------------------------------------------------------------------------

def _bands(world):
    return tuple(("band", k, world) for k in range(world))


def _shape(film, nsamp, parts=(None,), filt=None, max_paths=None):
    return dict(film=film, nsamp=nsamp, parts=tuple(parts), filt=filt, max_paths=max_paths)


SHAPES = {
    "box_16x12": _shape((16, 12), 9),                                              # 8 samples: exactly one batch of k_film_box
    "box_40x24_rect_off": _shape((40, 24), 12, parts=[(5, 3, 37, 21)]),            # batch + tail of 3; a rect that is not whole tiles
    "box_40x24_rect_tiles": _shape((40, 24), 12, parts=[(8, 8, 40, 24)]),          # a whole-tile rect: tile-order / tile-tree passes
    "gauss_16x12": _shape((16, 12), 9, filt=GAUSS),                                # k_film_wide
    "gauss_16x12_rect": _shape((16, 12), 9, parts=[(3, 2, 13, 9)], filt=GAUSS),    # splats across the rect border into this call's plane
    "box_16x40_bands": _shape((16, 40), 5, parts=_bands(2)),                       # bands with a short last band
    "gauss_16x40_bands": _shape((16, 40), 5, parts=_bands(2), filt=GAUSS),
    "box_16x12_passes": _shape((16, 12), 9, max_paths=256),                        # several passes that cut pixels and samples
}
_scenes, _refs = {}, {}


def _factory(name, workdir):
    s = SHAPES[name]
    def make(n):
        key = (s["film"], n, s["filt"] is not None)
        if key not in _scenes:
            _scenes[key] = Scene.loads(*_cfg3_tilted(workdir, s["film"], n, s["filt"]))
        return _scenes[key]
    return make


def _scene(name, workdir):
    return _factory(name, workdir)(SHAPES[name]["nsamp"])


def _reference(name, workdir):
    """(moments, film) of the shape in f64, the parts summed; computed once, read-only"""
    if name not in _refs:
        s = SHAPES[name]
        W, H = s["film"]
        m, film = np.zeros((H, W, 4)), np.zeros((H, W, 4))
        for part in s["parts"]:
            band = (part[1], part[2]) if part is not None and part[0] == "band" else None
            ref = MR.moments(_factory(name, workdir), s["nsamp"], None if band or part is None else part, band)
            m += ref["moments"]; film += ref["film"]
        assert film[..., 1].max() > 0
        m.setflags(write=False); film.setflags(write=False)
        _refs[name] = (m, film)
    return _refs[name]


def _handle(name, workdir, prec):
    r = Renderer(_scene(name, workdir), 0, prec)
    if SHAPES[name]["max_paths"]: r.set_option("max_paths", SHAPES[name]["max_paths"])
    return r


def _render_part(r, part, moments=True):
    """one part on handle r, fresh buffers: (film, moments or None, stats)"""
    band = part is not None and part[0] == "band"
    if moments:
        return r.render_moments(None, part[1], part[2], stats=True) if band else r.render_moments(part, stats=True)
    film, st = r.render_bands(part[1], part[2], stats=True) if band else r.render(part, stats=True)
    return film, None, st


def _render(r, name):
    """the shape's parts summed: (film, moments)"""
    W, H = SHAPES[name]["film"]
    film, mom = np.zeros((H, W, 4), r.dtype), np.zeros((H, W, 4), r.dtype)
    for part in SHAPES[name]["parts"]:
        f, m, _ = _render_part(r, part)
        film += f; mom += m
    return film, mom


def _channel_errors(got, ref):
    return [float(np.abs(got[..., ch].astype(np.float64) - ref[..., ch]).max() / np.abs(ref[..., ch]).max()) for ch in range(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_f64_moments_match_reference(name, workdir):
    ref, _ = _reference(name, workdir)
    r = _handle(name, workdir, RRT_F64)
    _, mom = _render(r, name)
    r.close()
    errs = _channel_errors(mom, ref)
    print(f"{name}: f64 S1, S2, S0, S3 against the reference, of each channel's largest magnitude: {['%.3e' % e for e in errs]}")
    if SHAPES[name]["filt"] is None:
        assert np.array_equal(mom[..., 2], ref[..., 2]) and np.array_equal(mom[..., 3], ref[..., 3])
    else:
        for ch in (2, 3):
            assert np.array_equal(mom[..., ch] != 0, ref[..., ch] != 0)
            np.testing.assert_allclose(mom[..., ch], ref[..., ch], rtol=1e-12, atol=0)
    assert max(errs) < 1e-9, errs


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_film_is_the_plain_frames(name, prec, workdir):
    r = _handle(name, workdir, prec)
    for part in SHAPES[name]["parts"]:
        film, mom, st = _render_part(r, part)
        plain, _, st_plain = _render_part(r, part, moments=False)
        assert film[..., :3].max() > 0 and mom[..., 1].max() > 0
        assert np.array_equal(film, plain), (name, part)      # all four channels
        for key in STATS:
            assert getattr(st, key) == getattr(st_plain, key), (name, part, key)
        assert st.camera_rays > 0 and st.any_queries > 0
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_parts_sum_to_the_whole(prec, workdir):
    """Rects are the whole frame's pixels inside them, the ranks' bands sum to it, and the cut into passes does not matter: box filter bit for bit in both
    modes; Gaussian in f64 to rtol 1e-12 (a pixel's sum is then added up in another order)."""
    for name in ("box_40x24_rect_off", "box_40x24_rect_tiles", "box_16x40_bands", "box_16x12_passes", "gauss_16x40_bands"):
        s = SHAPES[name]
        if s["filt"] is not None and prec == RRT_F32: continue
        r = _handle(name, workdir, prec)
        film, mom = _render(r, name)
        r.set_option("max_paths", 2 ** 28)
        whole_film, whole = r.render_moments()
        r.close()
        if s["parts"][0] is not None and s["parts"][0][0] != "band":      # a rect: the whole frame's pixels inside it, nothing outside
            x0, y0, x1, y1 = s["parts"][0]
            inside = np.zeros(whole.shape[:2], bool); inside[y0:y1, x0:x1] = True
            whole, whole_film = np.where(inside[..., None], whole, 0), np.where(inside[..., None], whole_film, 0)
        assert mom[..., 1].max() > 0
        if s["filt"] is None:
            assert np.array_equal(mom, whole), name
            assert np.array_equal(film, whole_film), name
        else:
            np.testing.assert_allclose(mom, whole, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_shortcuts_change_no_bit(workdir):
    for name in ("box_40x24_rect_tiles", "box_16x12", "gauss_16x12_rect"):
        r = _handle(name, workdir, RRT_F32)
        out = []
        for mode in (1, 0):
            for key in ("tile_trees", "tile_order", "film_records", "shade_compact"): r.set_option(key, mode)
            out.append(_render(r, name))
        r.close()
        assert out[0][1][..., 1].max() > 0
        assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0]), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fp32_moments_close_to_reference(name, workdir):
    ref, ref_film = _reference(name, workdir)
    r = _handle(name, workdir, RRT_F32)
    film, mom = _render(r, name)
    r.close()
    lit = ref_film[..., 3] != 0
    film_err = float((np.abs(film[..., :3].astype(np.float64) - ref_film[..., :3]).max(-1) / np.abs(ref_film[..., :3]).max())[lit].max())
    errs = _channel_errors(mom, ref)
    print(f"{name}: fp32 film max {film_err:.3e}; S1, S2, S0, S3: {['%.3e' % e for e in errs]}")
    assert np.all(mom[~lit] == 0)
    assert film_err < 1e-4      # the film bar first: a scene that misses it has ties, and is replaced, not excused
    assert errs[0] < 1e-4
    assert errs[1] < 2e-4
    if SHAPES[name]["filt"] is None:
        assert np.array_equal(mom[..., 2], ref[..., 2]) and np.array_equal(mom[..., 3], ref[..., 3])
    else:      # the weights of an fp32 table, summed in the kernel's order: test_frame_shapes.py's bar for the film's own weight channel
        assert np.array_equal(mom[..., 2] != 0, ref[..., 2] != 0)
        np.testing.assert_allclose(mom[..., 2], ref[..., 2], rtol=1e-5, atol=0)
        np.testing.assert_allclose(mom[..., 3], ref[..., 3], rtol=2e-5, atol=0)


def _large_frame(workdir, nsamp):
    """512 x 512 on a default fp32 handle whose pools are pinned to the default 2^28 slots: the whole frame is ONE pass of 2^18 pixels and all its samples.
    -> (film, moments, stats, plain film, the same frame as two half-frame rects summed: passes of 2^17 pixels)"""
    sc = Scene.loads(*_cfg3_tilted(workdir, (512, 512), nsamp))
    r = Renderer(sc, 0, RRT_F32)
    r.set_option("max_paths", 2 ** 28)
    film, mom, st = r.render_moments(stats=True)
    plain = r.render()
    halves = [r.render_moments(rect) for rect in ((0, 0, 512, 256), (0, 256, 512, 512))]
    r.close()
    assert st.camera_samples == 512 * 512 * (nsamp - 1)
    return film, mom, st, plain, (halves[0][0] + halves[1][0], halves[0][1] + halves[1][1])


@pytest.mark.gpu
def test_large_pass_consistency(workdir):
    """512 x 512 in one pass of 2^18 pixels: k_film_box's path for passes of that size or more. No oracle at this size; the plane against its own film.
    One sample per pixel (S2 S0 = S1^2), and eight: with fewer than eight samples neither path batches, so only the eight-sample frame tells the
    large-pass loop from the ordinary tail - its half-frame rects (2^17 pixels a pass) take the batched-by-8 loop and must give the same bits."""
    film, mom, st, plain, _ = _large_frame(workdir, 2)
    assert np.array_equal(film, plain)
    m = mom.astype(np.float64)
    assert np.array_equal(m[..., 2], film[..., 3].astype(np.float64) / 3.0) and np.array_equal(m[..., 2], m[..., 3]) and np.all(m[..., 2] == 1.0)
    assert (m[..., 0] > 0).mean() > 0.1
    np.testing.assert_allclose(m[..., 0], film[..., 1].astype(np.float64), rtol=1e-5, atol=0)
    np.testing.assert_allclose(m[..., 1] * m[..., 2], m[..., 0] ** 2, rtol=1e-6, atol=0)
    film, mom, st, plain, (half_film, half_mom) = _large_frame(workdir, 9)
    assert np.array_equal(film, plain)
    assert np.array_equal(mom, half_mom) and np.array_equal(film, half_film)      # the unbatched and the batched loop: one sample order, the same bits
    m = mom.astype(np.float64)
    assert np.array_equal(m[..., 2], film[..., 3].astype(np.float64) / 3.0) and np.array_equal(m[..., 2], m[..., 3]) and np.all(m[..., 2] == 8.0)
    assert (m[..., 0] > 0).mean() > 0.1
    np.testing.assert_allclose(m[..., 0], film[..., 1].astype(np.float64), rtol=1e-5, atol=0)
    assert np.all(m[..., 1] * m[..., 2] >= m[..., 0] ** 2 * (1 - 1e-5))      # Cauchy-Schwarz, to fp32 rounding of eight-term sums
    assert (m[..., 1] * m[..., 2] > m[..., 0] ** 2 * 1.01).mean() > 0.1          # and a real spread among the samples of many pixels


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box_40x24_rect_tiles", "gauss_16x12"])
def test_handle_is_untouched(name, workdir):
    r = _handle(name, workdir, RRT_F32)
    part = SHAPES[name]["parts"][0]
    a, sa = r.render(part, stats=True)
    _render_part(r, part)
    b, sb = r.render(part, stats=True)
    r.close()
    assert a[..., :3].max() > 0 and np.array_equal(a, b)
    for key in STATS + ("tile_launches", "list_launches"):
        assert getattr(sa, key) == getattr(sb, key), key


# ---- GPU: rrt_denoise_moments ------------------------------------------------------------------------------------------------------------------------

DN_SHAPES = ((131, 77), (20, 6))
DN_FP32_BAR = 4 * 1.234e-6      # test_denoise.py's: 4 x the worst case measured there against the numpy reference; measured here: 1.385e-6
_dn_inputs, _dn_refs, _dn_scenes = {}, {}, {}


def _dn_renderer(W, H, prec, workdir):
    """config 3 with the film's size: the filter takes the frame size from the handle"""
    if (W, H) not in _dn_scenes:
        _dn_scenes[(W, H)] = Scene.loads(*scenes.cfg3(workdir, xres=W, yres=H, nsamp=3, max_depth=5))
    return Renderer(_dn_scenes[(W, H)], 0, prec)


def _dn_input(W, H, dtype):
    """the synthetic film, planes and moments of a size, rounded to the handle's type once"""
    key = (W, H, np.dtype(dtype).name)
    if key not in _dn_inputs:
        film, aov = DR.synthetic(W, H, seed=1000 + W)
        mom = MR.synthetic_moments(film, 2000 + W)
        _dn_inputs[key] = (np.ascontiguousarray(film, dtype), {k: np.ascontiguousarray(v, dtype) for k, v in aov.items()}, np.ascontiguousarray(mom, dtype))
    return _dn_inputs[key]


def _dn_reference(W, H, dtype):
    key = (W, H, np.dtype(dtype).name)
    if key not in _dn_refs:
        film, aov, mom = _dn_input(W, H, dtype)
        _dn_refs[key] = MR.denoise(film, **aov, moments=mom, record_dtype=np.float32 if dtype == np.float32 else None)
        _dn_refs[key].setflags(write=False)
    return _dn_refs[key]


def _rel_err(got, ref):
    return float(np.abs(got[..., :3].astype(np.float64) - ref[..., :3]).max() / np.abs(ref[..., :3]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("size", DN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_moments_matches_reference(size, prec, workdir):
    W, H = size
    dtype = np.float32 if prec == RRT_F32 else np.float64
    film, aov, mom = _dn_input(W, H, dtype)
    r = _dn_renderer(W, H, prec, workdir)
    got = r.denoise(film, aov, moments=mom)
    spatial = r.denoise(film, aov)
    r.close()
    ref = _dn_reference(W, H, dtype)
    err = _rel_err(got, ref)
    print(f"{W} x {H}: {np.dtype(dtype).name} max error {err:.3e} of the output's largest magnitude")
    assert np.all(np.isfinite(got)) and not np.array_equal(got, spatial)
    assert np.array_equal(got[..., 3], film[..., 3])
    assert np.array_equal(got[film[..., 3] == 0], film[film[..., 3] == 0])
    assert err < (1e-9 if prec == RRT_F64 else DN_FP32_BAR)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_denoise_moments_lds_memory_kinds_and_in_place_agree(prec, workdir):
    import torch
    dtype = np.float32 if prec == RRT_F32 else np.float64
    for W, H in DN_SHAPES:
        film, aov, mom = _dn_input(W, H, dtype)
        r = _dn_renderer(W, H, prec, workdir)
        host = r.denoise(film, aov, moments=mom, iterations=6)
        r.set_option("dn_lds", 0)
        gathers = r.denoise(film, aov, moments=mom, iterations=6)
        r.set_option("dn_lds", 1)
        in_place = film.copy()
        assert r.denoise(in_place, aov, out=in_place, moments=mom, iterations=6) is in_place
        dev = [torch.from_numpy(a).to("cuda:0") for a in (film, aov["albedo"], aov["normal"], aov["depth"], mom)]
        dev_out = torch.zeros_like(dev[0])
        torch.cuda.synchronize()
        r.denoise_device(dev[0].data_ptr(), [d.data_ptr() for d in dev[1:4]], dev_out.data_ptr(), moments_ptr=dev[4].data_ptr(), iterations=6)
        assert np.array_equal(dev[0].cpu().numpy(), film) and np.array_equal(dev[4].cpu().numpy(), mom)      # read only
        r.denoise_device(dev[0].data_ptr(), [d.data_ptr() for d in dev[1:4]], dev[0].data_ptr(), moments_ptr=dev[4].data_ptr(), iterations=6)
        empty = r.denoise(film, aov, moments=np.zeros_like(mom))
        spatial = r.denoise(film, aov)
        r.close()
        assert not np.array_equal(host, film)
        assert np.array_equal(host, gathers)
        assert np.array_equal(host, in_place)
        assert np.array_equal(host, dev_out.cpu().numpy())
        assert np.array_equal(host, dev[0].cpu().numpy())
        assert np.array_equal(empty, spatial)      # an empty plane: rrt_denoise


@pytest.mark.gpu
def test_end_to_end_f64(workdir):
    """render_moments, render_aov, denoise(moments=...) on the 40 x 24 scene against the numpy reference fed the device's own planes."""
    sc = Scene.loads(*_cfg3_tilted(workdir, (40, 24), 12))
    r = Renderer(sc, 0, RRT_F64)
    film, mom = r.render_moments()
    aov = r.render_aov()
    got = r.denoise(film, aov, moments=mom)
    spatial = r.denoise(film, aov)
    r.close()
    ref = MR.denoise(film, **aov, moments=mom)
    _, use = MR.sample_variance(DR.prepare(film, **aov), mom)
    err = _rel_err(got, ref)
    print(f"tilted config 3 at 40 x 24, 11 spp: f64 max error {err:.3e}; {use.mean():.3f} of the pixels on the sample variance")
    assert use.mean() > 0.5 and not np.array_equal(got, spatial)
    assert np.array_equal(got[..., 3], film[..., 3])
    assert err < 1e-9


# ---- GPU: error paths and the command lines ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_device_side_error_paths(workdir):
    import torch
    name = "box_16x12"
    W, H = SHAPES[name]["film"]
    r = _handle(name, workdir, RRT_F32)
    lib = A.lib()
    film, mom = np.full((H, W, 4), 7.0, np.float32), np.full((H, W, 4), 7.0, np.float32)
    call = lambda rect, rank, world, mem: lib.rrt_render_moments(r._h, (C.c_int32 * 4)(*rect), rank, world, film.ctypes.data, mom.ctypes.data, mem, None)
    assert call((0, 0, W, H), 0, 1, 2) == A.RRT_EINVAL and b"bad mem" in lib.rrt_last_error()
    assert call((0, 0, W, H), 2, 2, A.RRT_MEM_HOST) == A.RRT_EINVAL and b"rank" in lib.rrt_last_error()
    assert call((0, 0, W, H), 0, 0, A.RRT_MEM_HOST) == A.RRT_EINVAL and b"rank" in lib.rrt_last_error()
    assert call((0, 0, W + 1, H), 0, 1, A.RRT_MEM_HOST) == A.RRT_EINVAL and b"outside the film" in lib.rrt_last_error()
    assert call((4, 4, 4, 8), 0, 1, A.RRT_MEM_HOST) == A.RRT_EINVAL and b"outside the film" in lib.rrt_last_error()
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, frame.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_moments(film=film, moments=mom)
    r.render_end()
    assert np.all(film == 7.0) and np.all(mom == 7.0)
    f2, m2 = r.render_moments(film=film, moments=mom)      # and the handle still works: += onto the caller's values
    fresh_f, fresh_m = r.render_moments()
    r.close()
    assert f2 is film and m2 is mom
    assert np.array_equal(film, np.float32(7.0) + fresh_f) and np.array_equal(mom, np.float32(7.0) + fresh_m)


@pytest.mark.gpu
def test_cli_denoise_moments(tmp_path):
    """RRT_DENOISE_MOMENTS=1 beside RRT_DENOISE: both command lines write a denoised PNG that differs from the spatial one; the ordinary PNG stays byte for
    byte; without RRT_DENOISE the variable changes nothing."""
    cfg, _ = _cfg3_tilted(str(tmp_path), (40, 24), 9)
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    base = {k: v for k, v in os.environ.items() if k not in ("RRT_DENOISE", "RRT_DENOISE_MOMENTS", "RRT_AOV", "RRT_GPUS")}
    base["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
        out = {}
        for kind, env in (("spatial", {}), ("moments", {"RRT_DENOISE_MOMENTS": "1"})):
            frame, dn = tmp_path / f"{tag}_{kind}.png", tmp_path / f"{tag}_{kind}_dn.png"
            p = subprocess.run(cmd + [str(scene), str(frame)], capture_output=True, text=True, timeout=600, env=dict(base, RRT_DENOISE=str(dn), **env))
            assert p.returncode == 0, p.stderr
            out[kind] = (frame.read_bytes(), dn.read_bytes(), p.stdout)
        assert out["moments"][0] == out["spatial"][0]
        assert out["moments"][2] == out["spatial"][2]      # the "N rays generated" line
        assert out["moments"][1][:8] == b"\x89PNG\r\n\x1a\n" and out["moments"][1][16:24] == out["spatial"][1][16:24]
        assert out["moments"][1] != out["spatial"][1]
    alone = tmp_path / "alone.png"
    p = subprocess.run([exe, str(scene), str(alone)], capture_output=True, text=True, timeout=600, env=dict(base, RRT_DENOISE_MOMENTS="1"))
    assert p.returncode == 0, p.stderr
    assert alone.read_bytes() == out["spatial"][0]
