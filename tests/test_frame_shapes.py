"""The fp32 frame against the f64 oracle over rect, pass and band shapes, on the GPU.

The fast path of the fp32 path integrator - k_raygen_main_f32 with 8 x 8 tile x 8 samples per camera workgroup, k_trace_tiles_f32, k_film_box_runs -
is guarded elsewhere by A/B tests that switch one option and share everything else between the two sides. Here one table of frame shapes (rects whose
origin is off the tile and patch grids, more than 64 record runs per tile, frames whose passes are partly record passes, bands with a short last
band, wide filters at a nonzero origin) is held to the oracle, and every shape says which kernels it must have gone through (rrt_render_stats).

Three tests over the table:
  test_f64_frame_matches_oracle              the shared enumeration and film code, in the f64 device mode: weights and rays generated equal, colour within 1e-9
  test_default_fp32_frame_equals_plain_frame the defaults against the same handle with every result-invariant shortcut switched off TOGETHER: identical bits
  test_default_fp32_frame_close_to_oracle    the default fp32 frame within the fp32 bars of DESIGN.md section 4

The options switched off together, each pinned bit-identical (np.array_equal on frames, on and off) on its own by an existing test:
  tile_order     test_gpu_parity.py::test_tile_order_of_the_pixels_changes_nothing
  tile_trees     test_gpu_parity.py::test_tile_trees_change_nothing
  quad_nodes     test_gpu_parity.py::test_quad_nodes_change_nothing
  shade_compact  test_gpu_parity.py::test_shade_compaction_changes_nothing
  horizon_cull   test_gpu_parity.py::test_horizon_cull_changes_nothing
  root_cull      test_gpu_parity.py::test_root_cull_changes_nothing
  shadow_lists   test_gpu_parity.py::test_shadow_candidate_lists_change_nothing
  aux_margin     test_gpu_parity.py::test_aux_margins_change_nothing
  lens_cull      test_lens_cull.py::test_lens_cull_changes_nothing
  film_records   test_film_records.py::test_film_records_change_nothing
  halton_tables  test_gpu_parity.py::test_halton_block_tables_change_nothing
  cam_tables     test_gpu_parity.py::test_camera_halton_block_tables_change_nothing
  any_entry      test_gpu_parity.py::test_any_hit_entry_nodes_change_nothing
raygen_lean, persistent_traversal and pt_split_* stay as they are: the code documents those as equal to rounding only (the compiler contracts multiply-adds
differently in the kernels they choose between), so bits are compared within one split setting only.

The heightfield scenes used here are not tie-prone: for every shape the oracle's reference-order and flattened evaluations agree to 4e-17 or exactly, so a
difference is the device's.
"""
import numpy as np
import pytest

import oracle_lib as O
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, Scene, scenes

pytestmark = pytest.mark.gpu

INVARIANT_OPTIONS = ("tile_order", "tile_trees", "quad_nodes", "shade_compact", "horizon_cull", "root_cull", "shadow_lists", "aux_margin", "lens_cull",
                     "film_records", "halton_tables", "cam_tables", "any_entry")

GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}


def _shape(scene="cfg4", film=(128, 96), nsamp=25, parts=(None,), tile=(1,), max_paths=None, filt=None):
    """parts: the render calls that are summed into one film - None (the whole film), a rect (x0, y0, x1, y1), or ("band", rank, world);
    tile: rrt_render_stats::tile_launches expected of each part with the defaults (the number of passes that qualify for k_trace_tiles_f32)."""
    assert len(parts) == len(tile)
    return dict(scene=scene, film=film, nsamp=nsamp, parts=tuple(parts), tile=tuple(tile), max_paths=max_paths, filt=filt)


def _bands(world):
    return tuple(("band", k, world) for k in range(world))


SHAPES = {
    # rect origins: off the 8-pixel tile grid, tile-aligned but off the 32-pixel patch grid, and a rect that is not made of whole tiles (row-order camera kernel)
    "rect_off_tile": _shape(film=(136, 104), parts=[(5, 3, 101, 67)]),                       # 96 x 64: tiled, three runs per tile
    "rect_off_tile_8spp": _shape(film=(136, 104), nsamp=9, parts=[(5, 3, 101, 67)]),
    "rect_off_patch": _shape(film=(136, 104), parts=[(8, 24, 104, 88)]),
    "rect_untiled": _shape(film=(136, 104), parts=[(5, 3, 98, 60)], tile=[0]),               # 93 x 57
    # record runs per tile: k_film_box_runs hands out {first, count} for 64 runs at a time; 6 tiles do not fill its four-tile workgroups
    "runs_64": _shape(film=(24, 16), nsamp=513),
    "runs_65": _shape(film=(24, 16), nsamp=521),
    "runs_128": _shape(film=(24, 16), nsamp=1025),
    "cfg5_runs_65": _shape(scene="cfg5", film=(64, 48), nsamp=521),
    # mixed frames: record passes and per-slot passes add into one internal film
    "mixed_passes_tail4": _shape(nsamp=29, max_paths=128 * 96 * 8, tile=[3]),                 # passes of 8, 8, 8 and 4 samples
    "mixed_passes_tail12": _shape(nsamp=45, max_paths=128 * 96 * 16, tile=[2]),               # passes of 16, 16 and 12 samples: the last is no multiple of 8
    "odd_samples": _shape(nsamp=30, tile=[0]),                                                # one pass of 29 samples: no tile-tree pass
    "pixel_groups": _shape(nsamp=9, max_paths=1000, tile=[0]),                                # groups that are not whole tiles, one sample per pass
    # bands of 16 rows, world 3: 104 rows leave rank 0 with 16 + 16 + 8 rows (tiled), 100 rows with 36 (row order) beside two tiled ranks
    "bands_short_last": _shape(film=(128, 104), parts=_bands(3), tile=[1, 1, 1]),
    "bands_mixed_order": _shape(film=(128, 100), parts=_bands(3), tile=[0, 1, 1]),
    # the wide film's halo and inverse enumeration at a nonzero origin, and the halo clipped by the film's edges
    "gauss_rect_off": _shape(film=(136, 104), nsamp=9, parts=[(5, 3, 101, 67)], filt=GAUSS),
    "gauss_rect_corner": _shape(film=(136, 104), nsamp=9, parts=[(0, 0, 96, 64), (40, 40, 136, 104)], tile=[1, 1], filt=GAUSS),
}

_scenes, _refs, _defaults = {}, {}, {}


def _scene(name, workdir):
    if name not in _scenes:
        s = SHAPES[name]
        W, H = s["film"]
        if s["scene"] == "cfg4": cfg, root = scenes.cfg4(workdir, xres=W, yres=H, nsamp=s["nsamp"], max_depth=5, n=64)
        else: cfg, root = scenes.cfg5(workdir, xres=W, yres=H, nsamp=s["nsamp"], max_depth=8, n=64)
        if s["filt"]: cfg["Film"]["Filter"] = dict(s["filt"])
        _scenes[name] = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    return _scenes[name]


def _oracle(name, workdir):
    """(film, rays generated) of the f64 oracle: the parts summed (the bands of all ranks are the whole film)."""
    if name not in _refs:
        sc, s = _scene(name, workdir), SHAPES[name]
        W, H = s["film"]
        film, rays = np.zeros((H, W, 4)), 0
        if isinstance(s["parts"][0], tuple) and s["parts"][0][0] == "band":
            film, st = O.render(sc, stats=True)
            rays = int(st.camera_rays)
        else:
            for part in s["parts"]:
                f, st = O.render(sc, part, stats=True)
                film += f; rays += int(st.camera_rays)
        assert film[..., :3].max() > 0
        _refs[name] = (film, rays)
    return _refs[name]


def _render(r, name):
    """The shape's parts on handle r: (film summed over the parts, [stats of each part])."""
    s = SHAPES[name]
    W, H = s["film"]
    film, stats = np.zeros((H, W, 4), r.dtype), []
    for part in s["parts"]:
        if part is not None and part[0] == "band": f, st = r.render_bands(part[1], part[2], stats=True)
        else: f, st = r.render(part, stats=True)
        film += f; stats.append(st)
    return film, stats


def _handle(name, workdir, prec, split0=False):
    r = Renderer(_scene(name, workdir), 0, prec)
    if SHAPES[name]["max_paths"]: r.set_option("max_paths", SHAPES[name]["max_paths"])
    if split0:      # the tile / persistent kernels at every queue size (the product hands queues below 100 000 rays to the grid-stride kernel)
        r.set_option("pt_split_closest", 0); r.set_option("pt_split_any", 0)
    return r


def _counts(stats):
    return [(s.camera_rays, s.closest_queries, s.any_queries) for s in stats]


def _check_default_stats(name, stats):
    """What the table says of the shape: no case may pass through a path other than the one it names."""
    for st, tile in zip(stats, SHAPES[name]["tile"]):
        assert st.tile_launches == tile, (name, st.tile_launches, tile)
        assert 0 < st.root_culled < st.camera_rays
        assert st.sky_culled > 0
        assert st.list_launches == st.any_launches > 0


def _check_weights(name, film, ref):
    """Filter-weight sums against the oracle's, the zeros outside the rect included. Box filter of radius 0.5: a pixel's sum is 3 per sample (Q3), an
    integer in both formats - equal. Gaussian: a pixel adds ~72 table weights, in fp32 those of an fp32 table, and the device adds them in its own
    order (k_film_wide: pixel by pixel; the oracle: sample by sample, tile by tile), so the sums cannot be equal bit for bit in either format
    (measured: 7.5e-16 relative in f64, 3.6e-7 in fp32). There the SUPPORT is equal exactly - which pixels of the halo, clipped by the rect and the
    film's edges, hold weight at all - and the values hold test_wide_filters' bars (rtol 1e-12 in f64, 1e-5 in fp32)."""
    w, w_ref = film[..., 3].astype(np.float64), ref[..., 3]
    rel = np.abs(w - w_ref).max() / w_ref.max()
    print(f"{name}: {film.dtype} weights: support equal {np.array_equal(w != 0, w_ref != 0)}, largest difference {rel:.3e} of the largest sum")
    if SHAPES[name]["filt"] is None:
        assert np.array_equal(w, w_ref)
    else:
        assert np.array_equal(w != 0, w_ref != 0)
        np.testing.assert_allclose(w, w_ref, rtol=1e-12 if film.dtype == np.float64 else 1e-5, atol=0)


def _default_frame(name, workdir, split0, handle=None):
    key = (name, split0)
    if key not in _defaults:
        r = handle or _handle(name, workdir, RRT_F32, split0)
        _defaults[key] = _render(r, name)
        if handle is None: r.close()
    return _defaults[key]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_f64_frame_matches_oracle(name, workdir):
    ref, ref_rays = _oracle(name, workdir)
    r = _handle(name, workdir, RRT_F64)
    film, stats = _render(r, name)
    r.close()
    _check_weights(name, film, ref)
    if name == "gauss_rect_off": assert int((ref[..., 3] != 0).sum()) == 98 * 66
    assert sum(int(s.camera_rays) for s in stats) == ref_rays
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    print(f"{name}: f64 device vs oracle, max {diff.max():.3e}")
    assert diff.max() < 1e-9, diff.max()       # the f64 mode's bar


@pytest.mark.parametrize("split0", [False, True], ids=["product_split", "split_0"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_default_fp32_frame_equals_plain_frame(name, split0, workdir):
    r = _handle(name, workdir, RRT_F32, split0)
    film, stats = _default_frame(name, workdir, split0, handle=r)
    for key in INVARIANT_OPTIONS: r.set_option(key, 0)
    plain, st_plain = _render(r, name)
    r.close()
    print(f"{name}: tile launches {[s.tile_launches for s in stats]}, rays generated {[s.camera_rays for s in stats]}, root culled {[s.root_culled for s in stats]}, "
          f"sky culled {[s.sky_culled for s in stats]}")
    _check_default_stats(name, stats)
    for st in st_plain:
        assert st.tile_launches == 0 and st.root_culled == 0 and st.sky_culled == 0 and st.list_launches == 0
    assert _counts(stats) == _counts(st_plain)
    assert film[..., :3].max() > 0
    assert np.array_equal(film, plain)       # all four channels


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_default_fp32_frame_close_to_oracle(name, workdir):
    ref, ref_rays = _oracle(name, workdir)
    film, stats = _default_frame(name, workdir, True)
    _check_default_stats(name, stats)
    spp = SHAPES[name]["nsamp"] - 1
    _check_weights(name, film, ref)
    rays = sum(int(s.camera_rays) for s in stats)
    assert abs(rays - ref_rays) <= 2e-5 * ref_rays, (rays, ref_rays)       # aperture-edge samples (test_full_size_frame_properties)
    lit = ref[..., 3] != 0
    diff = (np.abs(film[..., :3].astype(np.float64) - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max())[lit]
    print(f"{name}: fp32 vs oracle at {spp} spp: within 1e-4: {(diff < 1e-4).mean():.4f}, max {diff.max():.3e}, mean {diff.mean():.3e}")
    assert np.all(film[~lit] == 0)
    if spp <= 8:
        assert diff.max() < 1e-4, diff.max()       # DESIGN.md section 4, as test_render_f32_close_to_oracle
    else:      # the statistical form of test_full_size_frame_properties; one sample's share scaled from its 3e-2 at 256 spp
        assert (diff < 1e-4).mean() >= 0.975, (diff < 1e-4).mean()
        assert diff.mean() < 1e-4, diff.mean()
        assert diff.max() < 3e-2 * 256 / spp, diff.max()
