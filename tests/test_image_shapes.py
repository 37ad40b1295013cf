"""The device's MIPMap lookup (dtexture.hpp: mip_texel, mip_triangle, mip_ewa, mip_lookup_d) on hand-built images (tests/image_shapes.py), against the
f64 oracle.

Every other GPU test looks up one square 256 x 256 image, `clamp` in the trilinear form, `repeat` with every coordinate inside [0, 1) in the EWA form.
The images and mappings of image_shapes.py walk the lookup through what that never reaches: wrap `black` with its quirk that an in-range texel reads
(0, 0), texels out of range under EWA, levels with u_res != v_res, a pyramid resampled from a source that is no power of two, one-level pyramids,
negative coordinates, and EWA results that are 0 / 0 - all of them and part of them. image_shapes.py says which case reaches what, and the oracle's
lookup census (oracle_lib.mip_census) proves per case that the frame does reach it: the proof is counted on the reference side.

CPU tests (the host loader and the oracle alone):
  test_case_loads_and_reaches_its_branches    the pyramid's level sizes are oracle/host_ref.py build_mipmap's; the oracle's frame is finite and lit
                                              on the enclosure (ewa_all_nan: lit on the cube only, weight plane full); the census has the structure
                                              image_shapes.census_problems asks of the case's tag
  test_wrap_modes_give_three_frames           the oracle's repeat / black / clamp frames differ pairwise in more than a quarter of the pixels
                                              (2 249 to 3 297 of 4 096): a device that took one wrap mode for another cannot pass
  test_one_level_ewa_panics_in_the_oracle     EWA on a one-level pyramid asks for pyramid[1]
GPU tests, a 64 x 64 film at nsamp 5 each:
  test_f64_frame_matches_oracle               weights and the three counters equal, colour within 1e-9 of the brightest pixel; the frames with 0 / 0
                                              lookups finite and dark exactly where the oracle's are
  test_fp32_frame_close_to_oracle             test_gpu_parity.py::test_textured_materials' fp32 bars
  test_one_level_ewa_panics                   RrtPanic in both precisions; the trilinear form on the same handle type renders
  test_albedo_plane_reads_level_zero          rrt_render_aov evaluates textures with zero differentials: triangle(0) of every image shape under every
                                              wrap mode against tests/aov_reference.py, with test_aov.py's f64 and fp32 bars
  test_shortcuts_change_no_bit                shade compaction, shading-kernel specialisation and tile order off: the fp32 frame keeps its bits
"""
import os
import sys

import numpy as np
import pytest

import image_shapes as IS
import oracle_lib as O
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtPanic, Scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

ALL = sorted(IS.CASES)
NAN_TAGS = ("ewa_all_nan", "ewa_some_nan")
# the cube (plain matte) alone lights 68 of the 4 096 pixels; the enclosure fills the rest of the lens's image circle (82 % of the film)
CUBE_ONLY = 0.05

_scenes, _refs, _pyramids = {}, {}, {}


def _scene(name, workdir):
    if name not in _scenes:
        _scenes[name] = Scene.loads(*IS.scene(workdir, name))
    return _scenes[name]


def _ref(name, workdir):
    """(frame, stats, census) of the oracle for the case, rendered once and never written to"""
    if name not in _refs:
        sc = _scene(name, workdir)
        O.mip_census()
        film, st = O.render(sc, stats=True)
        census = O.mip_census()
        film.setflags(write=False)
        _refs[name] = (film, (int(st.camera_rays), int(st.closest_queries), int(st.any_queries)), census)
    return _refs[name]


def _level_sizes(h, w):
    """[(u_res, v_res)] of the pyramid host_ref.build_mipmap builds of the image (the sizes do not depend on the wrap mode: it was built under repeat)"""
    if (h, w) not in _pyramids:
        import host_ref as HR
        _pyramids[(h, w)] = [(L.u_res, L.v_res) for L in HR.build_mipmap(IS.image(h, w), wrap=0)]
    return _pyramids[(h, w)]


def _lit(film):
    return float((film[..., :3].max(-1) > 0).mean())


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_case_loads_and_reaches_its_branches(name, workdir):
    c = IS.CASES[name]
    sc = _scene(name, workdir)
    assert sc.desc.n_images == 1 and sc.desc.n_textures == 1
    im = sc.desc.images[0]
    assert (im.do_trilinear, im.wrap, im.max_aniso) == (1 if c.trilinear else 0, IS.WRAP_CODE[c.wrap], c.max_aniso)
    sizes = _level_sizes(c.h, c.w)
    assert im.n_levels == len(sizes)
    assert [(im.levels[k].u_res, im.levels[k].v_res) for k in range(im.n_levels)] == sizes
    if (c.h, c.w) in IS.ONE_LEVEL: assert im.n_levels == 1
    if (c.h, c.w) == (100, 130): assert sizes == [(256, 128), (128, 64)]
    if (c.h, c.w) == (128, 512): assert sizes == [(512, 128), (256, 64)]
    if (c.h, c.w) == (512, 128): assert sizes == [(128, 512), (64, 256)]
    film, _, census = _ref(name, workdir)
    print(f"{name}: lit {_lit(film):.4f}, brightest {film[..., :3].max():.4f}, census {census}")
    assert np.all(np.isfinite(film))
    assert np.all(film[..., 3] > 0)
    if c.tag == "ewa_all_nan":
        # every sample on the enclosure is dropped: the cube alone is lit, and the weight plane is the one of a frame that drops nothing
        assert 0 < _lit(film) < CUBE_ONLY
        assert np.array_equal(film[..., 3], _ref(IS.find("tri_magnified", 256, 256)[0], workdir)[0][..., 3])
    else:
        assert _lit(film) > CUBE_ONLY
    assert not IS.census_problems(c, census), (IS.census_problems(c, census), census)


WRAP_GROUPS = {f"{tag}-{h}x{w}": [IS.find(tag, h, w, wrap)[0] for wrap in IS.WRAPS]
               for tag, h, w in [("tri_all_levels", 256, 256), ("tri_all_levels", 128, 512), ("tri_all_levels", 512, 128), ("tri_all_levels", 100, 130),
                                 ("ewa_edge", 256, 256)]}


@pytest.mark.parametrize("group", sorted(WRAP_GROUPS))
def test_wrap_modes_give_three_frames(group, workdir):
    films = [_ref(name, workdir)[0][..., :3] for name in WRAP_GROUPS[group]]
    for a in range(3):
        for b in range(a + 1, 3):
            scale = max(films[a].max(), films[b].max())
            differ = int((np.abs(films[a] - films[b]).max(-1) > 1e-6 * scale).sum())
            print(f"{group}: {IS.WRAPS[a]} against {IS.WRAPS[b]}: {differ} of {films[a].shape[0] * films[a].shape[1]} pixels differ")
            assert differ > films[a].shape[0] * films[a].shape[1] // 4


def _one_level_scene(workdir, hw, trilinear):
    c = IS.Case("one_level", *hw, "repeat", trilinear, IS.MAP_ALL_LEVELS, 8.0)
    return Scene.loads(*IS.scene(workdir, c))


@pytest.mark.parametrize("hw", IS.ONE_LEVEL, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_one_level_ewa_panics_in_the_oracle(hw, workdir):
    """lod = max(levels - 1 + log2(minor_length), 0) with levels - 1 == 0: ewa(0) and ewa(1) = pyramid[1], index out of bounds (mipmap.rs:217). No EWA
    frame of such an image exists; the panic is the expected result."""
    sc = _one_level_scene(workdir, hw, False)
    assert sc.desc.images[0].n_levels == 1
    with pytest.raises(O.OracleError, match="out of bounds"):
        O.render(sc)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_f64_frame_matches_oracle(name, workdir):
    ref, counters, _ = _ref(name, workdir)
    r = Renderer(_scene(name, workdir), 0, RRT_F64)
    film, st = r.render(stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert (st.camera_rays, st.closest_queries, st.any_queries) == counters
    if IS.CASES[name].tag in NAN_TAGS:
        # the 0 / 0 lookups are dropped at the film as the reference drops them: nothing of them arrives, and the same pixels stay dark
        assert np.all(np.isfinite(film))
        assert np.array_equal(film[..., :3].max(-1) > 0, ref[..., :3].max(-1) > 0)
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    print(f"{name}: f64 max {diff.max():.3e}")
    assert diff.max() < 1e-9, (diff.max(), int((diff > 1e-9).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_fp32_frame_close_to_oracle(name, workdir):
    ref, _, _ = _ref(name, workdir)
    r = Renderer(_scene(name, workdir), 0, RRT_F32)
    f32 = r.render().astype(np.float64)
    r.close()
    assert np.array_equal(f32[..., 3], ref[..., 3])
    assert np.all(np.isfinite(f32))
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    mean_rel = abs(f32[..., :3].mean() / ref[..., :3].mean() - 1)
    print(f"{name}: f32 within 1e-4: {(d32 < 1e-4).mean():.4f}, median {np.median(d32):.3e}, max {d32.max():.3e}, mean rel {mean_rel:.3e}")
    assert (d32 < 1e-4).mean() > 0.97 and np.median(d32) < 1e-5, ((d32 < 1e-4).mean(), np.median(d32), d32.max())
    assert mean_rel < 0.02, mean_rel


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
def test_one_level_ewa_panics(prec, workdir):
    for hw in ((16, 16), (16, 256)):
        r = Renderer(_one_level_scene(workdir, hw, False), 0, prec)
        with pytest.raises(RrtPanic, match="index out of bounds"):
            r.render()
        r.close()
        r = Renderer(_one_level_scene(workdir, hw, True), 0, prec)
        film = r.render()
        r.close()
        assert np.all(np.isfinite(film)) and _lit(film) > CUBE_ONLY


# The one fp32 bar a case cannot hold: the share of the albedo plane's pixels within 1e-4 for 128 x 512 under `repeat`. Its level 0 is 512 texels wide and
# su = 3 repeats it, so one unit of the triangle's u spans 1 536 texels of an image whose neighbouring texels differ by a third of the range on average
# (noise in B, x ^ y in R) - twice the texels of every other case, and under `repeat` no lookup is spared (clamp and black read one texel, or none, for
# the 9 in 10 lookups past the last column). With zero differentials every lookup is the bilinear triangle(0), whose value moves by that texel
# difference times the error of sx = s u_res - 0.5 in texels. What fp32 can know of sx, worked out on the oracle alone: with the camera rays, the hit's
# barycentrics, uv and s each only ROUNDED to fp32 and every operation between them exact, the plane already moves by 7.6e-6 in the mean and 7.5e-5 at most
# (of its largest value) - s near 2 has a spacing of 2.4e-7, 1.2e-4 texels, and sx near 1 024 the same again. The device's fp32 chain from the ray to sx is
# some fifteen rounded operations, not four roundings, and lands at 3.7 times that floor: mean 2.8e-5 (the bar is 1e-4), largest 4.4e-4 (the bar is 1.9),
# live weight exact, and 96.25 % of the pixels within 1e-4 where the bar asks 97.5 %; the f64 plane of the same case equals the reference to the bit
# (0.0), so the lookup itself is the reference's. The error is in texels, so it grows with the texels per unit of u: this case keeps every bar of
# test_fp32_planes_close_to_reference with the per-pixel threshold scaled by its level 0 against the others', 512 / 256: 97.5 % within 2e-4. 256 x 256 and
# 100 x 130 (256 wide) under repeat hold the bar as it is (99.8 % and 99.9 %).
FP32_ALBEDO_PIXEL_BAR = {"tri_all_levels-128x512-repeat": 1e-4 * 512 / 256}

ALBEDO_CASES = [IS.find("tri_all_levels", h, w, wrap)[0] for h, w in ((256, 256), (128, 512), (100, 130)) for wrap in IS.WRAPS] + \
               [IS.find("tri_one_level", 16, 16, wrap)[0] for wrap in IS.WRAPS]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALBEDO_CASES)
def test_albedo_plane_reads_level_zero(name, workdir):
    """The albedo plane's textures are evaluated with zero differentials: width 0, level = levels - 1 + log2(1e-8) < 0, triangle(0) - also on the
    one-level image. The f64 plane holds test_aov.py::test_f64_planes_match_reference's bar, the fp32 plane test_fp32_planes_close_to_reference's
    (one case with the per-pixel threshold of FP32_ALBEDO_PIXEL_BAR, for the reason given there)."""
    import aov_reference as AR
    from test_aov import _value_diff
    sc = _scene(name, workdir)
    O.mip_census()
    ref = AR.planes(sc)["albedo"]
    census = O.mip_census()
    assert census["tri_below"] > 4000 and census["tri_last"] == 0 and census["tri_between"] == 0, census
    assert census["texel_out"] > 0 and census["texel_in"] > 0, census
    assert ref[..., :3].max() > 0
    got = {}
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        got[prec] = r.render_aov(planes=("albedo",))["albedo"]
        r.close()
    diff = _value_diff("albedo", got[RRT_F64], ref)
    print(f"{name}: f64 albedo max {diff.max():.3e}")
    assert np.array_equal(got[RRT_F64][..., 3], ref[..., 3])
    assert diff.max() < 1e-9, diff.max()
    spp = int(sc.desc.sampler.samples_per_pixel) - 1
    f32 = got[RRT_F32].astype(np.float64)
    live, live_ref = float(f32[..., 3].sum()), float(ref[..., 3].sum())
    covered = ref[..., 3] != 0
    w_diff = np.abs(f32[..., 3] - ref[..., 3]) / ref[..., 3].max()
    d = np.maximum(_value_diff("albedo", f32, ref), w_diff)
    assert np.all(f32[~covered & (f32[..., 3] == 0)] == 0)
    d = d[covered | (f32[..., 3] != 0)]
    bar = FP32_ALBEDO_PIXEL_BAR.get(name, 1e-4)
    print(f"{name}: fp32 albedo at {spp} spp: within 1e-4: {(d < 1e-4).mean():.4f}, within 2e-4: {(d < 2e-4).mean():.4f}, mean {d.mean():.3e}, max {d.max():.3e}, "
          f"live {live} against {live_ref}")
    assert (d < bar).mean() >= 0.975 and d.mean() < 1e-4 and d.max() < 3e-2 * 256 / spp, (bar, (d < bar).mean(), d.mean(), d.max())
    assert abs(live - live_ref) <= 2e-5 * live_ref, (live, live_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [IS.find("tri_all_levels", 128, 512, "black")[0], IS.find("ewa_edge", 256, 256, "clamp")[0]])
def test_shortcuts_change_no_bit(name, workdir):
    """The shading-side options (test_gpu_parity.py: test_shade_compaction_changes_nothing, test_shading_kernel_specialisation,
    test_tile_order_of_the_pixels_changes_nothing) reorder or specialise the work around the texture lookup and must not touch it."""
    r = Renderer(_scene(name, workdir), 0, RRT_F32)
    base, st0 = r.render(stats=True)
    assert base[..., :3].max() > 0
    for opt in ("shade_compact", "shade_spec", "tile_order"):
        r.set_option(opt, 0)
        film, st = r.render(stats=True)
        r.set_option(opt, 1)
        assert np.array_equal(film, base), opt
        assert (st.camera_rays, st.closest_queries, st.any_queries) == (st0.camera_rays, st0.closest_queries, st0.any_queries), opt
    r.close()
