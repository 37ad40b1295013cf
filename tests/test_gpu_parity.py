"""GPU parity tests: the HIP path (through the C ABI) against the f64 oracle on the same seeded inputs.

Bars: index/integer outputs (winning triangle, occlusion bits, filter-weight sums, node/prim counters)
bit-exact in f64 mode; floating point within the tolerance written next to each assert. The fp32 product
path is held to statistical closeness because a path's discrete decisions (which triangle, which lobe,
roulette) flip for O(1e-5) of samples under fp32 rounding.

The reference transforms the ray per primitive (TransformedPrimitive, primitives.rs:115-139). The f64 device mode replays exactly
that for every instance (RRT_INSTANCES_KEEP is its default) and is compared bit-for-bit with the oracle's reference-order
evaluation. The fp32 product flattens rigid instances to world space; the two evaluations agree except on exact ties (a hit on a
face coplanar with a flat leaf box: gap of ~1e-16), which each breaks by its own last-bit rounding - tests/test_oracle.py bounds how
often they differ and shows that every such ray is a tie, and test_flattened_f64_matches_the_flat_oracle holds the flattened
evaluation (RRT_INSTANCES_FLATTEN in f64) to the oracle's flat=True one bit for bit.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
from scene_util import boxes_on_a_plane, rough_terrain, write_patch as _write_patch
from rs_ray_toy_amd import (RRT_F32, RRT_F64, RRT_FIXED_BVH, RRT_INSTANCES_FLATTEN, RRT_INSTANCES_KEEP, Renderer, RrtPanic, RrtUnsupported,
                            Scene, scenes)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cfg2_scene(workdir):
    cfg, root = scenes.cfg2(workdir, xres=128, yres=128, nsamp=9, max_depth=4)
    return Scene.loads(cfg, root)


@pytest.fixture(scope="module")
def hf_scene(workdir):
    cfg, root = scenes.cfg4(workdir, xres=96, yres=96, nsamp=5, max_depth=8, n=64)  # 8192 triangles
    return Scene.loads(cfg, root, flags=RRT_FIXED_BVH)


def _rays_for(scene, n, seed):
    o, d, tmax = O.random_rays(scene, n, seed)
    # half of the rays start on a surface, like spawned rays do (Q8: no origin offset)
    ref = O.trace_closest(scene, o, d, tmax, want_geometry=True)
    hit = ref["prim"] >= 0
    rng = np.random.default_rng(seed + 1)
    o2 = np.where(hit[:, None], ref["p"], o)
    d2 = rng.normal(size=(n, 3))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    skip = np.concatenate([np.full(n, -1, np.int32), np.where(hit, ref["prim"], -1).astype(np.int32)])
    return np.concatenate([o, o2]), np.concatenate([d, d2]), np.concatenate([tmax, tmax]), skip


@pytest.mark.parametrize("which", ["cfg2", "hf"])
def test_trace_closest_f64_exact(which, cfg2_scene, hf_scene):
    sc = cfg2_scene if which == "cfg2" else hf_scene
    o, d, tmax, _ = _rays_for(sc, 4096, 11)
    ref = O.trace_closest(sc, o, d, tmax)
    r = Renderer(sc, 0, RRT_F64)
    got = r.trace_closest(o, d, tmax, counters=True)
    r.close()
    assert (ref["prim"] >= 0).sum() > 500
    assert np.array_equal(got["prim"], ref["prim"])            # winning triangle incl. "last accepted wins" (Q10)
    assert np.array_equal(got["nodes"], ref["nodes"])          # identical traversal: node / prim counters
    assert np.array_equal(got["prims"], ref["prims"])
    hit = ref["prim"] >= 0
    # same operation order, IEEE f64 add/mul/div only, no FMA contraction on either side: bit-exact
    assert np.array_equal(got["t"], ref["t"])
    assert np.array_equal(got["u"][hit], ref["u"][hit]) and np.array_equal(got["v"][hit], ref["v"][hit])


def test_flattened_f64_matches_the_flat_oracle(cfg2_scene, workdir):
    """RRT_INSTANCES_FLATTEN in the f64 mode = the evaluation the fp32 product uses (rigid instances moved to world space once), held to
    the oracle's flat=True evaluation bit for bit: rays (winner, t, u, v, counters, occlusion) and a frame."""
    sc = cfg2_scene
    o, d, tmax, _ = _rays_for(sc, 4096, 11)
    ref = O.trace_closest(sc, o, d, tmax, flat=True)
    r = Renderer(sc, 0, RRT_F64, flags=RRT_INSTANCES_FLATTEN)
    got = r.trace_closest(o, d, tmax, counters=True)
    occ = r.trace_any(o, d, np.full(len(tmax), 1.0 - 1e-4))
    film = r.render()
    r.close()
    hit = ref["prim"] >= 0
    assert np.array_equal(got["prim"], ref["prim"]) and np.array_equal(got["nodes"], ref["nodes"]) and np.array_equal(got["prims"], ref["prims"])
    assert np.array_equal(got["t"], ref["t"]) and np.array_equal(got["u"][hit], ref["u"][hit]) and np.array_equal(got["v"][hit], ref["v"][hit])
    assert np.array_equal(occ, O.trace_any(sc, o, d, np.full(len(tmax), 1.0 - 1e-4), flat=True)["occluded"])
    ref_film = O.render(sc, flat=True)
    assert np.array_equal(film[..., 3], ref_film[..., 3])
    diff = np.abs(film[..., :3] - ref_film[..., :3]).max(-1) / np.abs(ref_film[..., :3]).max()
    assert (diff > 1e-9).mean() < 0.005, (diff > 1e-9).mean()


def test_kept_instances_fp32(workdir):
    """RRT_INSTANCES_KEEP in the fp32 mode: every instance through the per-primitive ray transform (the reference's order) on the generic
    kernels, against the oracle's reference-order evaluation within the fp32 bar (tilted cubes: no exact ties)."""
    cfg, root = scenes.cfg2(workdir, xres=64, yres=64, nsamp=9, max_depth=4)
    for inst in cfg["Aggregate"]["primitives"][0]["instances"]:
        inst["rotation_axis"] = [1.0, 2.0, 3.0]
    sc = Scene.loads(cfg, root)
    ref = O.render(sc)
    r = Renderer(sc, 0, RRT_F32, flags=RRT_INSTANCES_KEEP)
    film = r.render().astype(np.float64)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    assert (diff < 1e-4).mean() > 0.99 and np.median(diff) < 1e-5, ((diff < 1e-4).mean(), np.median(diff))
    with pytest.raises(Exception):
        Renderer(sc, 0, RRT_F32, flags=RRT_INSTANCES_KEEP | RRT_INSTANCES_FLATTEN)


@pytest.mark.parametrize("which", ["cfg2", "hf"])
def test_trace_closest_f32(which, cfg2_scene, hf_scene):
    sc = cfg2_scene if which == "cfg2" else hf_scene
    o, d, tmax, skip = _rays_for(sc, 4096, 5)
    ref = O.trace_closest(sc, o, d, tmax)
    r = Renderer(sc, 0, RRT_F32)
    got = r.trace_closest(o, d, tmax, skip_prim=skip)          # fp32 excludes the triangle a ray starts on
    r.close()
    same = got["prim"] == ref["prim"]
    # fp32: edge/grazing rays may pick the neighbour. cfg2's cubes have axis-aligned faces coplanar with flat
    # leaf boxes: 23 % of its rays carry an exact tie that fp32 breaks at random (see test_oracle.py)
    assert same.mean() > (0.97 if which == "cfg2" else 0.999), same.mean()
    hit = same & (ref["prim"] >= 0)
    np.testing.assert_allclose(got["t"][hit], ref["t"][hit], rtol=2e-4, atol=1e-4)


def test_trace_closest_when_tmax_grows(workdir):
    """Q10 makes t_max non-monotonic: a later accepted hit that is FARTHER overwrites the nearer one (closed, rotated
    cubes: the back face's fat leaf box starts before the front hit). A far child skipped because its box began beyond
    the t_max of that moment must therefore still be judged against the t_max at the time it is popped. Camera rays
    through tilted cubes, fp32 product kernels vs the oracle: every winner identical."""
    cfg, root = scenes.cfg2(workdir, xres=128, yres=128, nsamp=9, max_depth=1)
    for inst in cfg["Aggregate"]["primitives"][0]["instances"]:
        inst["rotation_axis"] = [1.0, 2.0, 3.0]
    sc = Scene.loads(cfg, root)
    _, rays, w = O.camera_samples(sc, (0, 0, 128, 128), 1, 9)
    alive = w > 0
    o, d = rays[alive, :3], rays[alive, 3:]
    tmax = np.full(len(o), np.inf)
    ref = O.trace_closest(sc, o, d, tmax, flat=True)
    hit = ref["prim"] >= 0
    assert hit.sum() > 2000
    r = Renderer(sc, 0, RRT_F32)
    got = r.trace_closest(o, d, tmax)
    big = Renderer(sc, 0, RRT_F32)
    big.set_option("persistent_traversal", 2)      # the persistent-thread kernel regardless of the queue size
    got_pt = big.trace_closest(o, d, tmax)
    r.close(); big.close()
    assert (got["prim"] == ref["prim"]).mean() > 0.9999, (got["prim"] != ref["prim"]).sum()
    assert (got_pt["prim"] == ref["prim"]).mean() > 0.9999, (got_pt["prim"] != ref["prim"]).sum()
    np.testing.assert_allclose(got["t"][hit & (got["prim"] == ref["prim"])], ref["t"][hit & (got["prim"] == ref["prim"])], rtol=2e-6)


@pytest.mark.parametrize("prec", [RRT_F64, RRT_F32])
def test_trace_any(prec, hf_scene):
    sc = hf_scene
    o, d, tmax, skip = _rays_for(sc, 4096, 23)
    tmax = np.full(len(tmax), 1.0 - 1e-4)                      # shadow rays keep t_max = 1 - SHADOW_EPSILON (Q9)
    ref = O.trace_any(sc, o, d, tmax)
    r = Renderer(sc, 0, prec)
    got = r.trace_any(o, d, tmax, skip_prim=skip if prec == RRT_F32 else None)
    r.close()
    assert ref["occluded"].sum() > 50
    if prec == RRT_F64:
        assert np.array_equal(got, ref["occluded"])
    else:
        assert (got == ref["occluded"]).mean() > 0.995


@pytest.mark.parametrize("prec", [RRT_F64, RRT_F32])
def test_camera_samples(prec, cfg2_scene):
    sc = cfg2_scene
    rect = (40, 50, 72, 66)
    dims, rays, w = O.camera_samples(sc, rect, 1, 5)
    r = Renderer(sc, 0, prec)
    gd, gr, gw = r.camera_samples(rect, 1, 5)
    r.close()
    assert np.array_equal(gd, dims)                            # Halton dims are produced in f64 on the device: exact
    assert 0.05 < (w > 0).mean() < 0.9
    if prec == RRT_F64:
        assert np.array_equal(gw > 0, w > 0)
        np.testing.assert_allclose(gw, w, rtol=1e-11)
        np.testing.assert_allclose(gr, rays, rtol=1e-10, atol=1e-10)
    else:
        assert ((gw > 0) == (w > 0)).mean() > 0.995           # aperture-edge lens traces can flip in fp32
        both = (gw > 0) & (w > 0)
        np.testing.assert_allclose(gw[both], w[both], rtol=1e-4)
        np.testing.assert_allclose(gr[both], rays[both], rtol=1e-3, atol=2e-4)


def _film_err(film, ref):
    scale = np.abs(ref[..., :3]).max()
    return np.abs(film[..., :3].astype(np.float64) - ref[..., :3]).max() / scale, scale


def _cfg3_tilted(wd):
    """cfg3 with the enclosure and the cube instanced under generic rotations: the literal axis-aligned box has flat
    wall triangles whose leaf boxes are coplanar with them, i.e. exact box/face ties (see the module docstring)."""
    cfg, root = scenes.cfg3(wd, xres=64, yres=64, nsamp=5, max_depth=5)
    cfg["Aggregate"]["primitives"][0]["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
    cfg["Aggregate"]["primitives"][1]["instances"] = [{"world_pos": [0.0, 0.0, 0.0], "rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}]
    return cfg, root


def _cfg4_distant(wd):
    """cfg4 lit by a DistantLight (lights/distant.rs) next to one point light: delta-direction light, shadow rays aimed at
    p + w_light * 2 * world_radius (then normalised with t_max = 1 - 1e-4, Q9)."""
    cfg, root = scenes.cfg4(wd, xres=64, yres=64, nsamp=5, max_depth=6, n=48)
    cfg["lights"] = [{"light_type": "distant", "l": {"values": [3.0, 2.5, 2.0]}, "scale": {"values": [1.5, 1.5, 1.5]},
                      "from": [20.0, 30.0, 10.0], "to": [35.0, 0.0, 0.0], "rotation_axis": [0.0, 0.0, 1.0], "rotation_angle": 10},
                     cfg["lights"][0]]
    return cfg, root


RENDER_CASES = {
    "cfg4_distant": _cfg4_distant,
    "cfg2_path": lambda wd: scenes.cfg2(wd, xres=96, yres=96, nsamp=9, max_depth=4),
    "cfg3_path": lambda wd: _cfg3_tilted(wd),
    "cfg3_literal": lambda wd: scenes.cfg3(wd, xres=96, yres=96, nsamp=9),   # BASELINE config 3 as scenes.cfg3() defines it (axis-aligned box: ties)
    "cfg4_path": lambda wd: scenes.cfg4(wd, xres=64, yres=64, nsamp=5, max_depth=8, n=48),
    "cfg5_path": lambda wd: scenes.cfg5(wd, xres=64, yres=64, nsamp=9, max_depth=16, n=48),
}


TIE_PRONE = ("cfg2_path", "cfg3_literal")


@pytest.mark.parametrize("case", sorted(RENDER_CASES))
def test_render_f64_matches_oracle(case, workdir):
    cfg, root = RENDER_CASES[case](workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH if "cfg4" in case or "cfg5" in case else 0)
    ref, st_ref = O.render(sc, stats=True)
    r = Renderer(sc, 0, RRT_F64)
    film, st = r.render(stats=True)
    r.close()
    assert ref[..., :3].max() > 0
    assert np.array_equal(film[..., 3], ref[..., 3])           # filter_weight_sum (Q1, Q2, Q3): exact
    assert st.camera_rays == st_ref.camera_rays                # the reference's "rays generated" counter
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    # f64 device mode: same formulas and operation order; libm vs device sin/cos/log may differ in the last
    # ulp. Bar: 1e-9 of the brightest pixel (a flipped discrete decision shows up as >= 1e-3).
    if case in TIE_PRONE:
        # tie-prone geometry (axis-aligned faces coplanar with flat leaf boxes): a last-ulp difference in a
        # sampled direction can break such a tie the other way; at most 0.5 % of pixels may carry one
        assert (diff > 1e-9).mean() < 0.005, (diff > 1e-9).mean()
    else:
        assert diff.max() < 1e-9, diff.max()


@pytest.mark.parametrize("case", sorted(RENDER_CASES))
def test_render_f32_close_to_oracle(case, workdir):
    cfg, root = RENDER_CASES[case](workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH if "cfg4" in case or "cfg5" in case else 0)
    ref = O.render(sc)
    r = Renderer(sc, 0, RRT_F32)
    film = r.render()
    r.close()
    assert np.array_equal(film[..., 3].astype(np.float64), ref[..., 3])
    scale = np.abs(ref[..., :3]).max()
    diff = np.abs(film[..., :3].astype(np.float64) - ref[..., :3]).max(-1) / scale
    # fp32 tolerance (north_star: "pixel values within a stated fp32 tolerance"): every pixel within 1e-4 of the
    # brightest pixel's value (observed <= 1.1e-5). cfg2's cubes have axis-aligned faces coplanar with flat leaf
    # boxes, i.e. exact ties that any change of rounding breaks differently (the oracle's own two evaluation
    # orders differ on 0.4 % of its pixels): there 98.5 % of pixels must be within 1e-3.
    if case in TIE_PRONE:
        assert (diff < 1e-3).mean() > 0.985, (diff < 1e-3).mean()
        assert np.median(diff) < 1e-5
    else:
        assert diff.max() < 1e-4, diff.max()


def test_render_rect_and_passes_are_consistent(workdir):
    """Tile partition (§8e): disjoint rects sum to the full frame; pool size (pass structure) does not matter."""
    cfg, root = scenes.cfg2(workdir, xres=64, yres=64, nsamp=9, max_depth=4)
    sc = Scene.loads(cfg, root)
    r = Renderer(sc, 0, RRT_F64)
    full = r.render()
    parts = np.zeros_like(full)
    for rect in ((0, 0, 64, 16), (0, 16, 64, 40), (0, 40, 64, 64)):
        r.render(rect, film=parts)
    r.set_option("max_paths", 1000)   # forces pixel groups and 1-sample passes
    small = r.render()
    r.close()
    assert np.array_equal(parts, full)
    np.testing.assert_allclose(small, full, rtol=1e-12, atol=1e-15)


def test_frames_in_flight_match_synchronous_frames(workdir):
    """rrt_render_bands_begin / rrt_render_end: two handles with a frame each in flight (non-blocking streams) produce the
    films of the synchronous call bit for bit; a second _begin on a busy handle is refused."""
    import torch
    from rs_ray_toy_amd import RrtError
    cfg, root = scenes.cfg4(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=48)
    sc = Scene.loads(cfg, root)
    hs = [Renderer(sc, 0, RRT_F32) for _ in range(2)]
    ref = [torch.zeros((96, 96, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    for k in range(2):
        hs[0].render_bands_device(k, 2, ref[k].data_ptr(), stats=False)
    for h in hs:
        h.set_option("nonblocking_streams", 1)
    films = [torch.zeros((96, 96, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(3):                      # += into the same films: 3 x the frame
        for k in range(2):
            hs[k].render_end()
            hs[k].render_bands_begin(k, 2, films[k].data_ptr())
    with pytest.raises(RrtError):
        hs[0].render_bands_begin(0, 2, films[0].data_ptr())
    for h in hs:
        h.render_end()
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(films[k], ref[k] * 3.0)
        assert ref[k].abs().sum() > 0
    for h in hs:
        h.close()


def test_render_bands_partition_sums_to_the_frame(workdir):
    """rrt_render_bands: the ranks' interleaved 16-row bands are disjoint and sum to the full frame (world 1, 3)."""
    cfg, root = scenes.cfg2(workdir, xres=48, yres=72, nsamp=5, max_depth=3)
    sc = Scene.loads(cfg, root)
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        full = r.render()
        one = r.render_bands(0, 1)
        parts = [r.render_bands(k, 3) for k in range(3)]
        r.close()
        assert np.array_equal(one, full)
        cover = sum((p[..., 3] > 0).astype(int) for p in parts)
        assert (cover == 1).all()                                  # every pixel rendered by exactly one rank
        rows = np.nonzero(parts[1][:, 0, 3] > 0)[0]
        assert list(rows[:16]) == list(range(16, 32)) and list(rows[16:]) == list(range(64, 72))
        assert np.array_equal(sum(parts), full)


@pytest.mark.parametrize("integrator", ["Debug", "DirectLighting_all", "DirectLighting_one", "AO"])
def test_other_integrators(integrator, workdir):
    cfg, root = scenes.cfg2(workdir, xres=64, yres=64, nsamp=5)
    if integrator == "Debug":
        cfg["Integrator"] = {"integrator_type": "Debug", "max_depth": 5}
    elif integrator == "AO":
        cfg["Integrator"] = {"integrator_type": "AO"}
    else:
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": integrator.split("_")[1], "max_depth": 5}
    # one mirror cube exercises the specular_reflect chain
    cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "mat_mirror", "obj_name": "cube_01",
                                           "instances": [{"world_pos": [33.0, 0.5, 0.0], "rotation_axis": [1, 2, 3], "rotation_angle": 20}]})
    for inst in cfg["Aggregate"]["primitives"][0]["instances"]:
        inst["rotation_axis"] = [1.0, 2.0, 3.0]   # generic axes: no face stays axis-aligned, no box/face ties
    sc = Scene.loads(cfg, root)
    ref = O.render(sc)
    r = Renderer(sc, 0, RRT_F64)
    film = r.render()
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    if integrator == "AO":
        assert film[..., :3].max() == 0 and ref[..., :3].max() == 0   # ao.rs:62-64: bsdf is never built -> black
        return
    err, _ = _film_err(film, ref)
    assert err < 1e-9, err


def test_roundtrip_properties_full_size(workdir):
    """Size-independent properties at BASELINE cfg4's full mesh size (100 352 triangles): (a) a closest hit's
    point re-traced from the far side of the ray hits the same triangle or one in front of it never behind,
    (b) any-hit with t_max = inf is implied by a closest hit for rays that do not start on a surface."""
    cfg, root = scenes.cfg4(workdir, xres=64, yres=64, nsamp=3, n=224)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    assert sc.desc.n_prims == 100352
    o, d, tmax = O.random_rays(sc, 200000, 3)
    r = Renderer(sc, 0, RRT_F32)
    got = r.trace_closest(o, d, tmax, counters=True)
    occ = r.trace_any(o, d, tmax)
    r.close()
    hit = got["prim"] >= 0
    assert hit.mean() > 0.3
    assert np.all(got["t"][hit] > 0) and np.all(np.isfinite(got["t"][hit]))
    assert np.all((got["u"][hit] >= 0) & (got["v"][hit] >= 0) & (got["u"][hit] + got["v"][hit] <= 1 + 1e-6))
    assert np.all(got["nodes"] >= 1) and np.all(got["prims"][hit] >= 1)
    # the any-hit test uses the reference's *different* triangle (E2 = p2 - p1, Q11), so implication is not
    # exact; it holds for the overwhelming majority on a closed heightfield
    assert occ[hit].mean() > 0.5
    # sampled oracle check at full size
    idx = np.random.default_rng(0).choice(len(tmax), 4000, replace=False)
    ref = O.trace_closest(sc, o[idx], d[idx], tmax[idx])
    assert (got["prim"][idx] == ref["prim"]).mean() > 0.999


def test_full_size_frame_properties(workdir):
    """BASELINE config 4 at its full size (100 352 triangles, 1024^2, 256 spp, depth 8), fp32 product path:
    idempotence (bitwise identical frames although queue order depends on atomics), the closed-form filter weight
    sum 3 * (nsamp - 1) in every pixel (Q1, Q2, Q3), the result-invariant shortcuts switched off (auxiliary lens traces, any-hit start
    lists, Halton block tables, tile trees: identical frames), a 2-rank band partition that reassembles the frame exactly, and a 32-row slice
    checked against the f64 oracle at full spp."""
    cfg, root = scenes.cfg4(workdir, xres=1024, yres=1024, nsamp=257, max_depth=8, n=224)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    film, st = r.render(stats=True)
    assert st.camera_samples == 1024 * 1024 * 256
    assert st.tile_launches == 1          # the camera rays went through the per-patch sub-trees (test_tile_trees_change_nothing)
    assert 0.25 < st.camera_rays / st.camera_samples < 0.36
    assert np.all(film[..., 3] == 3.0 * 256.0)
    assert np.isfinite(film).all() and film[..., :3].max() > 0
    again = r.render()
    assert np.array_equal(again, film)
    r.set_option("aux_margin", 0)   # every auxiliary lens trace run (test_aux_margins_change_nothing): the same 268 M decisions
    full_aux, st_aux = r.render(stats=True)
    r.set_option("aux_margin", 1)
    assert st_aux.camera_rays == st.camera_rays and np.array_equal(full_aux, film)
    # the shortcuts of the second half of round 2, all at once, at full size: shadow rays from the root instead of their start lists,
    # Halton digit loops instead of block tables (camera and integrator dimensions), camera rays through the ordinary persistent kernel - the same
    # 268 M samples, bit for bit
    for key in ("any_entry", "cam_tables", "halton_tables", "tile_trees", "root_cull"): r.set_option(key, 0)
    plain, st_plain = r.render(stats=True)
    for key in ("any_entry", "cam_tables", "halton_tables", "tile_trees", "root_cull"): r.set_option(key, 1)
    assert st_plain.tile_launches == 0 and st_plain.root_culled == 0 and 0 < st.root_culled < st.camera_rays
    assert (st_plain.camera_rays, st_plain.closest_queries, st_plain.any_queries) == (st.camera_rays, st.closest_queries, st.any_queries)
    assert np.array_equal(plain, film)
    bands = r.render_bands(0, 2)
    r.render_bands(1, 2, film=bands)
    assert np.array_equal(bands, film)
    rect = (0, 496, 1024, 528)
    ref, st_ref = O.render(sc, rect, stats=True)
    part, st_part = r.render(rect, stats=True)
    r.close()
    # a smaller rect means smaller queues, and below a threshold the traversal runs in the grid-stride kernel instead of
    # the persistent one: same tests in the same order, but the compiler fuses multiply-adds differently in the two,
    # so fp32 results agree to rounding, not bitwise (the f64 mode, compiled without contraction, is bitwise:
    # test_render_rect_and_passes_are_consistent)
    dpart = np.abs(part[496:528, :, :3].astype(np.float64) - film[496:528, :, :3]).max(-1) / np.abs(film[..., :3]).max()
    assert (dpart < 1e-6).mean() > 0.999 and dpart.max() < 2e-2, ((dpart < 1e-6).mean(), dpart.max())
    assert np.array_equal(part[496:528, :, 3], film[496:528, :, 3])
    assert abs(int(st_part.camera_rays) - int(st_ref.camera_rays)) <= 2e-5 * st_ref.camera_rays   # aperture-edge samples
    scale = np.abs(ref[..., :3]).max()
    diff = np.abs(part[496:528, :, :3].astype(np.float64) - ref[496:528, :, :3]).max(-1) / scale
    # a pixel holds 256 samples; a sample whose discrete decision flips under fp32 rounding moves its pixel by up to
    # ~1/256 of a sample's radiance. What is left after the double-float spawn origins (spawn_point()) is the rounding
    # of the vertices themselves to fp32 (2e-6 at coordinates of ~35): a shadow ray passing within that distance of a
    # silhouette edge flips, ~4e-5 of the samples, i.e. ~1.5 % of the pixels hold one. Bar: 97.5 % of the pixels
    # within the stated 1e-4, none beyond one sample (3e-2), mean deviation below 1e-4 of the brightest pixel.
    print("full-size fp32 vs oracle: within 1e-4: %.4f, max %.3e, mean %.3e" % ((diff < 1e-4).mean(), diff.max(), diff.mean()))
    assert (diff < 1e-4).mean() > 0.975, (diff < 1e-4).mean()
    assert diff.max() < 3e-2, diff.max()
    assert diff.mean() < 1e-4, diff.mean()


def test_mixed_scene_keeps_the_pair_node_kernels(workdir):
    """One sphere and one scaled cube among BASELINE config 4's 100 352 triangles must not send the whole scene to the generic kernels:
    leaves that hold such a primitive carry a flag (kSpecialLeaf) and take a rare path inside the pair-node kernels. Bars: the mixed
    scene's frame within 10 % of the plain scene's frame time at a size where the kernels, not the launches, are what is timed (512^2,
    64 spp), and its image - on the pixels the two extra primitives do not touch - equal to the plain scene's."""
    import copy, time
    def build(mixed):
        cfg, root = scenes.cfg4(workdir, xres=512, yres=512, nsamp=65, max_depth=8)
        if mixed:
            write = scenes.write_cube(workdir)
            cfg["objs"] = cfg["objs"] + [{"filename": "cube.obj", "obj_name": "cube_01"}]
            cfg["Aggregate"]["primitives"] = cfg["Aggregate"]["primitives"] + [
                {"primitive_type": "sphere", "material_name": "mat_matte", "radius": 0.4, "instances": [{"world_pos": [33.0, 2.5, -1.0]}]},
                {"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "cube_01",
                 "instances": [{"world_pos": [37.0, 2.5, 1.5], "rotation_axis": [1.0, 2.0, 3.0], "rotation_angle": 20, "scale": [0.4, 0.25, 0.4]}]}]
        return Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    films, ms = {}, {}
    for mixed in (False, True):
        sc = build(mixed)
        r = Renderer(sc, 0, RRT_F32)
        r.render()                                     # pools, first-launch costs
        best = 1e9
        for _ in range(3):
            film, st = r.render(stats=True)
            best = min(best, st.ms_total)
        r.close()
        films[mixed], ms[mixed] = film.astype(np.float64), best
    print(f"mixed scene: {ms[True]:.2f} ms against {ms[False]:.2f} ms for the plain one ({ms[True] / ms[False]:.3f} x)")
    assert ms[True] < 1.10 * ms[False], (ms[True], ms[False])
    scale = films[False][..., :3].max()
    changed = (np.abs(films[True][..., :3] - films[False][..., :3]).max(-1) / scale > 1e-3).mean()
    assert 0.0005 < changed < 0.25, changed            # the two primitives are seen (and shadow / light their neighbourhood), the rest of the frame is not disturbed


def _non_rigid(wd, integrator):
    cfg, root = scenes.cfg2(wd, xres=72, yres=72, nsamp=9, max_depth=3)
    inst = cfg["Aggregate"]["primitives"][0]["instances"]
    for k, i in enumerate(inst):
        i["rotation_axis"] = [1.0, 2.0, 3.0]          # generic axes: no exact box / face ties
    inst[0]["scale"] = [2.0, 1.0, 0.5]                 # anisotropic
    inst[1]["scale"] = [0.6, 0.6, 0.6]                 # uniform, still not rigid; the third instance stays rigid (flattened)
    cfg["Integrator"] = integrator
    return cfg, root


@pytest.mark.parametrize("which", ["path", "path_metal", "path_plastic", "direct_all", "debug"])
def test_non_rigid_triangle_instances(which, workdir):
    """`scale` on a mesh instance (renderprocess.rs:242-252): TransformedPrimitive::intersect (primitives.rs:115-139) tests the triangle with
    the ray moved into the instance's space and RE-NORMALISED there (transform.rs:525-537), copies that object-space t to the world ray
    (Q15: boxes are then pruned with a distance in the wrong space) and transforms the interaction back, leaving wo un-normalised.
    The device replays exactly that for non-rigid instances (fp32: rigid ones are flattened; f64: every instance is kept). f64 mode: hits, t,
    counters bit for bit and frames to 1e-9 against the oracle; fp32 - pair-node kernels with the kept instances on their rare path, and the
    generic kernels - within the triangle scenes' bar.
    path_metal / path_plastic: the path integrator samples the BSDF with `wo = -ray.d` (path.rs:126), the WORLD ray's direction, while
    estimate_direct evaluates it with the interaction's un-normalised wo - on a scaled instance the two differ, and every lobe but the
    Lambertian one sees it (fuzz seed 703 case 95 found the device using the interaction's wo for both: 75 % of the pixels off by up to 6e-3)."""
    integ = {"path": {"integrator_type": "Path", "max_depth": 3}, "path_metal": {"integrator_type": "Path", "max_depth": 4},
             "path_plastic": {"integrator_type": "Path", "max_depth": 4}, "direct_all": {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3},
             "debug": {"integrator_type": "Debug", "max_depth": 3}}[which]
    cfg, root = _non_rigid(workdir, integ)
    if which in ("path_metal", "path_plastic"):
        cfg["Aggregate"]["primitives"][0]["material_name"] = "mat_metal" if which == "path_metal" else "mat_plastic"
    sc = Scene.loads(cfg, root)
    o, d, tmax, _ = _rays_for(sc, 2048, 17)
    ref_t = O.trace_closest(sc, o, d, tmax)      # the reference's order: every instance per primitive, like the f64 device mode
    ref_a = O.trace_any(sc, o, d, tmax)
    r = Renderer(sc, 0, RRT_F64)
    got = r.trace_closest(o, d, tmax, counters=True)
    occ = r.trace_any(o, d, tmax)
    ref, st_ref = O.render(sc, stats=True)
    film, st = r.render(stats=True)
    r.close()
    hit = ref_t["prim"] >= 0
    assert hit.sum() > 200
    scaled = np.array([sc.desc.prims[sc.desc.prim_order[p]].instance for p in ref_t["prim"][hit]])
    assert len(set(scaled.tolist())) >= 3                      # hits on all three instances, the two scaled ones included
    assert np.array_equal(got["prim"], ref_t["prim"]) and np.array_equal(got["nodes"], ref_t["nodes"]) and np.array_equal(got["prims"], ref_t["prims"])
    assert np.array_equal(got["t"], ref_t["t"])                # (object-space t for the scaled instances, as the reference leaves it in ray.t_max)
    assert np.array_equal(got["u"][hit], ref_t["u"][hit]) and np.array_equal(got["v"][hit], ref_t["v"][hit])
    assert np.array_equal(occ, ref_a["occluded"])
    assert np.array_equal(film[..., 3], ref[..., 3]) and st.camera_rays == st_ref.camera_rays
    if not which.startswith("path"):   # (the path integrator's dead final-bounce and MIS queries are not issued on the device)
        assert st.closest_queries == st_ref.closest_queries and st.any_queries == st_ref.any_queries
    scale = np.abs(ref[..., :3]).max()
    assert scale > 0
    assert (np.abs(film[..., :3] - ref[..., :3]).max() / scale) < 1e-9
    # fp32: the pair-node kernels (kept instances take their rare path, kSpecialLeaf) in both forms, and the generic kernels
    ref_o = ref                                                # the reference's own order throughout
    frames = {}
    for mode in (3, 2, 1, 0):
        r = Renderer(sc, 0, RRT_F32)
        if mode != 3:
            r.set_option("persistent_traversal", mode)         # 2: persistent-thread kernel whatever the queue size, 1: grid-stride, 0: generic
        f32 = r.render().astype(np.float64)
        r.close()
        frames[mode] = f32
        d32 = np.abs(f32[..., :3] - ref_o[..., :3]).max(-1) / scale
        assert np.array_equal(f32[..., 3], ref_o[..., 3])
        print(f"non-rigid {which} traversal mode {mode}: fp32 within 1e-4: {(d32 < 1e-4).mean():.4f}, max {d32.max():.2e}, mean ratio {f32[..., :3].mean() / ref_o[..., :3].mean():.5f}")
        assert (d32 < 1e-3).mean() > 0.97 and abs(f32[..., :3].mean() / ref_o[..., :3].mean() - 1.0) < 0.02
    dm = np.abs(frames[2][..., :3] - frames[1][..., :3]).max(-1) / scale      # the two pair-node kernels make the same decisions
    assert (dm < 1e-6).mean() > 0.995, (dm < 1e-6).mean()


@pytest.mark.parametrize("which", ["cfg4", "cfg4_far", "cfg5", "cfg2", "cfg3_direct"])
def test_any_hit_entry_nodes_change_nothing(which, workdir):
    """Shadow rays are 1 - 1e-4 long (Q9) and start on a triangle: the fp32 any-hit kernels start them at the first ancestor of that
    triangle's leaf whose other child is within reach, instead of at the root (TravScene::any_entry) - every ancestor contains the origin
    and passes its box test, every skipped sibling is more than a unit away and fails it, and an occlusion query does not depend on the
    order. Bar: frames with and without the shortcut are identical bit for bit, query counts included."""
    if which == "cfg4": cfg, root = scenes.cfg4(workdir, xres=128, yres=128, nsamp=9, max_depth=6, n=96)
    elif which == "cfg4_far":
        # the scene 1e5 units from the origin (an instance translation; camera moved along): fp32 coordinates there have an ulp of 0.008, which
        # the lists' reach must cover on top of the ray length (host/trav_tables.cpp build_pairs(): 8 ulp of the largest coordinate)
        cfg, root = scenes.cfg4(workdir, xres=128, yres=128, nsamp=9, max_depth=6, n=96)
        far = np.array([1.0e5, -7.0e4, 3.0e4])
        cfg["Aggregate"]["primitives"][0]["instances"] = [{"world_pos": list(far)}]
        cfg["Camera"]["world_pos"] = list(np.array(cfg["Camera"]["world_pos"], float) + far)
        cfg["Camera"]["look"] = list(np.array(cfg["Camera"]["look"], float) + far)
        cfg["lights"] = [{"light_type": "distant", "l": {"values": [3.0, 2.5, 2.0]}, "from": [20.0, 30.0, 10.0], "to": [35.0, 0.0, 0.0]}]
    elif which == "cfg5": cfg, root = scenes.cfg5(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=64)
    elif which == "cfg2": cfg, root = scenes.cfg2(workdir, xres=128, yres=128, nsamp=9, max_depth=4)
    else:
        cfg, root = scenes.cfg3(workdir, xres=128, yres=128, nsamp=9)
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3}
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    r.set_option("persistent_traversal", 2)            # the persistent-thread kernel whatever the queue size ...
    a, st_a = r.render(stats=True)
    r.set_option("any_entry", 0)
    b, st_b = r.render(stats=True)
    r.set_option("persistent_traversal", 1)            # ... and the grid-stride one
    c = r.render()
    r.set_option("any_entry", 1)
    d = r.render()
    r.close()
    assert st_a.any_queries == st_b.any_queries and st_a.any_queries > 1000
    assert np.array_equal(a, b) and np.array_equal(c, d)
    assert a[..., :3].max() > 0


@pytest.mark.parametrize("which", ["cfg4_lambert", "cfg5_glossy", "cfg2_mixed"])
def test_shading_kernel_specialisation(which, workdir):
    """The path shading kernel is instantiated per lobe-kind set (dmath.hpp "Lobe-kind sets"): scenes whose used materials can only produce
    Lambertian lobes, or Lambertian / Oren-Nayar / microfacet-reflection lobes, run a kernel without the other BxDFs' code and registers; the
    host picks the set from the materials (host/scene_flatten.cpp scan_materials()). Same arithmetic per lobe in every instantiation - the compiler may
    contract multiply-adds differently, so the frames agree to fp32 rounding, not bitwise; weights and query counts are identical - and both
    hold the fp32 bar against the oracle. cfg2_mixed uses a mirror: only the general kernel fits, the option changes nothing at all."""
    if which == "cfg4_lambert": cfg, root = scenes.cfg4(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=64)
    elif which == "cfg5_glossy": cfg, root = scenes.cfg5(workdir, xres=96, yres=96, nsamp=9, max_depth=8, n=64)
    else:
        cfg, root = scenes.cfg2(workdir, xres=96, yres=96, nsamp=9, max_depth=4)
        for inst in cfg["Aggregate"]["primitives"][0]["instances"]:
            inst["rotation_axis"] = [1.0, 2.0, 3.0]
        cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "mat_mirror", "obj_name": "cube_01",
                                               "instances": [{"world_pos": [33.0, 0.5, 0.0], "rotation_axis": [1, 2, 3], "rotation_angle": 20}]})
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    ref = O.render(sc)
    scale = np.abs(ref[..., :3]).max()
    r = Renderer(sc, 0, RRT_F32)
    spec, st_spec = r.render(stats=True)
    r.set_option("shade_spec", 0)            # the general kernel
    gen, st_gen = r.render(stats=True)
    r.close()
    assert (st_spec.camera_rays, st_spec.closest_queries, st_spec.any_queries) == (st_gen.camera_rays, st_gen.closest_queries, st_gen.any_queries)
    assert np.array_equal(spec[..., 3], gen[..., 3])
    d = np.abs(spec[..., :3].astype(np.float64) - gen[..., :3]).max(-1) / scale
    if which == "cfg2_mixed":
        assert np.array_equal(spec, gen)
    else:
        assert (d < 1e-6).mean() > 0.995 and np.median(d) < 1e-7, ((d < 1e-6).mean(), d.max())
    for film in (spec, gen):
        dd = np.abs(film[..., :3].astype(np.float64) - ref[..., :3]).max(-1) / scale
        assert (dd < 1e-4).mean() > 0.99 and np.median(dd) < 1e-5, ((dd < 1e-4).mean(), dd.max())


@pytest.mark.parametrize("which", ["box_cfg4", "gaussian_cfg3", "bands_cfg2"])
def test_tile_order_of_the_pixels_changes_nothing(which, workdir):
    """The pixels of a pass are enumerated tile by tile (8 x 8; a workgroup of the camera kernel takes one tile x 8 samples) where the rect is made
    of whole tiles, row by row otherwise (PassDesc::tiled): queue entries that are neighbours are then neighbours in both image directions, which
    the traversal and shading kernels' caches like (frame 36.8 -> 35.0 ms on config 4). Only the ORDER of the work changes - a sample's slot, Halton index and
    film pixel do not: frames, weights and counters with and without it are identical bit for bit, also under a filter that gathers across
    pixels (the film kernel inverts the enumeration) and for a rank's bands."""
    if which == "box_cfg4": cfg, root = scenes.cfg4(workdir, xres=128, yres=96, nsamp=9, max_depth=5, n=64)
    elif which == "gaussian_cfg3":
        cfg, root = scenes.cfg3(workdir, xres=96, yres=64, nsamp=9)
        cfg["Film"]["Filter"] = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
    else: cfg, root = scenes.cfg2(workdir, xres=64, yres=96, nsamp=5, max_depth=3)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    for prec in (RRT_F32, RRT_F64):
        r = Renderer(sc, 0, prec)
        out = {}
        for tile in (1, 0):
            r.set_option("tile_order", tile)
            if which == "bands_cfg2":
                out[tile] = (sum(r.render_bands(k, 3) for k in range(3)), None)
            else:
                out[tile] = r.render(stats=True)
                r.set_option("max_paths", 8 * 8 * 5 * 3)        # several pixel groups and passes: groups of whole tiles, 3 samples per pass
                out[tile + 2] = r.render(stats=True)
                r.set_option("max_paths", 1 << 28)
        r.close()
        assert np.array_equal(out[1][0], out[0][0]) and out[1][0][..., :3].max() > 0
        if which != "bands_cfg2":
            assert (out[1][1].camera_rays, out[1][1].closest_queries, out[1][1].any_queries) == (out[0][1].camera_rays, out[0][1].closest_queries, out[0][1].any_queries)
            np.testing.assert_allclose(out[3][0], out[1][0], rtol=1e-5 if prec == RRT_F32 else 1e-12, atol=1e-9)   # (fp32: a pixel's samples are summed pass by pass)
            assert np.array_equal(out[3][0], out[2][0])


@pytest.mark.parametrize("which", ["cfg4", "cfg4_odd_width", "cfg4_two_groups", "cfg4_bands", "cfg4_direct", "cfg4_passes", "cfg2_small_tree", "cfg4_2048"])
def test_tile_trees_change_nothing(which, workdir):
    """Camera rays walk the tree through per-patch local copies of its most visited pair nodes in LDS (dtraverse_f32.hpp k_trace_tiles_f32,
    host/trav_tables.cpp build_tile_trees()): the copies hold the tree's own boxes, leaf words and split axes - only the child words of a copy say
    "slot k of this copy" or "node n of the tree" - and the queue is not reordered, so every ray makes the same decisions in the same order
    whatever the census chose to copy. Frames, weights and query counts with and without are identical bit for bit: whole 32-pixel patches and
    a width of 13 tiles, one and two sample groups per tile, a rank's bands, DirectLighting's first level, a 2048^2 film (more 8 x 8 tiles than one grid
    dimension holds), and two census densities. Passes
    that do not cover the pixel grid in whole tile rows x 8 samples (small max_paths) and trees that fit a copy anyway keep the ordinary kernel
    (tile_launches = 0)."""
    kw = dict(xres=128, yres=96, nsamp=9, max_depth=5, n=64)
    if which == "cfg4_odd_width": kw.update(xres=104, yres=72)
    if which == "cfg4_two_groups": kw.update(nsamp=17)
    if which == "cfg4_2048": kw.update(xres=2048, yres=2048, max_depth=2)      # 65 536 tiles: the camera kernel's pixel blocks spill into grid z
    if which == "cfg2_small_tree": cfg, root = scenes.cfg2(workdir, xres=64, yres=96, nsamp=9, max_depth=3)
    else: cfg, root = scenes.cfg4(workdir, **kw)
    if which == "cfg4_direct": cfg["Integrator"] = {"integrator_type": "DirectLighting", "max_depth": 3, "light_strategy": "UniformSampleAll"}
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    r.set_option("pt_split_closest", 0)    # the persistent kernels at every queue size (the product switches at 100 000 rays)
    if which == "cfg4_passes": r.set_option("max_paths", 128 * 96 * 3)
    out = {}
    for tt in (1, 0, 2):
        r.set_option("tile_trees", 1 if tt else 0)
        if tt == 2: r.set_option("tt_census", 1)      # a sparser census: other copies, same frames
        if which == "cfg4_bands":
            out[tt] = [r.render_bands(k, 3, stats=True) for k in range(3)]
            out[tt] = (sum(f for f, _ in out[tt]), out[tt][0][1])
        else:
            out[tt] = r.render(stats=True)
    r.close()
    expect = 0 if which in ("cfg4_passes", "cfg2_small_tree") else 1
    assert out[1][1].tile_launches == expect and out[2][1].tile_launches == expect and out[0][1].tile_launches == 0, (out[1][1].tile_launches, out[0][1].tile_launches)
    assert out[1][0][..., :3].max() > 0
    for tt in (1, 2):
        assert np.array_equal(out[tt][0], out[0][0])
        assert (out[tt][1].camera_rays, out[tt][1].closest_queries, out[tt][1].any_queries) == (out[0][1].camera_rays, out[0][1].closest_queries, out[0][1].any_queries)


@pytest.mark.parametrize("which", ["cfg4", "cfg4_no_tile_trees", "cfg2", "cfg3", "cfg4_compat_bvh", "cfg4_direct", "cfg5"])
def test_quad_nodes_change_nothing(which, workdir):
    """Two levels per fetch (dtraverse_f32.hpp QuadNode, option "quad_nodes"): the closest-hit rays of the persistent kernel walk nodes that hold an
    interior node's four grandchild boxes; the children's own boxes are not tested (a grandchild's box passing implies its parent's, monotone
    rounding), slots are visited in the binary tree's order, every slot behind the one taken is judged when popped. Same leaves in the same
    order, same triangle tests, same t_max sequence as the pair-node walk: frames, weights and query counts identical bit for bit - on the
    heightfield (deep tree, 1-3 triangles per leaf), on the reference's tilted cubes (cfg2: exact box / face ties, t_max that grows, Q10), with
    the reference-exact builder's overlapping children (Q26 / Q27), under DirectLighting and with glossy materials + area lights - and a ray
    batch through the public entry point returns the same winners, t, u, v."""
    kw = dict(xres=128, yres=96, nsamp=9, max_depth=5, n=64)
    flags = RRT_FIXED_BVH
    if which == "cfg2": cfg, root = scenes.cfg2(workdir, xres=96, yres=96, nsamp=9, max_depth=4)
    elif which == "cfg3": cfg, root = scenes.cfg3(workdir, xres=96, yres=96, nsamp=9)
    elif which == "cfg5": cfg, root = scenes.cfg5(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=64)
    else: cfg, root = scenes.cfg4(workdir, **kw)
    if which == "cfg4_compat_bvh": flags = 0
    if which == "cfg4_direct": cfg["Integrator"] = {"integrator_type": "DirectLighting", "max_depth": 3, "light_strategy": "UniformSampleAll"}
    sc = Scene.loads(cfg, root, flags=flags)
    r = Renderer(sc, 0, RRT_F32)
    r.set_option("pt_split_closest", 0)    # the persistent kernels at every queue size (the product switches at 100 000 rays)
    if which == "cfg4_no_tile_trees": r.set_option("tile_trees", 0)   # the camera rays through the quad nodes as well
    rng = np.random.default_rng(7)
    wb = np.array(sc.desc.world_bound)
    n = 20000
    o = rng.uniform(wb[:3] - 2.0, wb[3:] + 2.0, (n, 3))
    tgt = rng.uniform(wb[:3], wb[3:], (n, 3))
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:64, 0] = 0.0; d[64:128, 1] = 0.0; d[:128] /= np.linalg.norm(d[:128], axis=1, keepdims=True)   # axis-parallel components: inf inverse directions
    tmax = np.full(n, np.inf)
    out, hits = {}, {}
    for q in (0, 1):
        r.set_option("quad_nodes", q)
        out[q] = r.render(stats=True)
        r.set_option("persistent_traversal", 2)
        hits[q] = r.trace_closest(o, d, tmax)
        r.set_option("persistent_traversal", 3)
    r.close()
    assert out[1][0][..., :3].max() > 0 and (hits[0]["prim"] >= 0).mean() > 0.2
    assert np.array_equal(out[1][0], out[0][0])
    assert (out[1][1].camera_rays, out[1][1].closest_queries, out[1][1].any_queries) == (out[0][1].camera_rays, out[0][1].closest_queries, out[0][1].any_queries)
    for k in ("prim", "t", "u", "v"):
        assert np.array_equal(hits[1][k], hits[0][k]), k


@pytest.mark.parametrize("which", ["cfg4", "rough_1", "rough_2", "rough_z_up", "cfg2", "cfg3", "cfg5", "stacked", "cfg4_passes", "boxes_1", "boxes_2", "cfg4_compat_bvh"])
def test_horizon_cull_changes_nothing(which, workdir, monkeypatch):
    """The path shading kernel answers a bounce ray as the miss it is when its elevation exceeds everything the host found visible from ANY point of its start
    triangle in its azimuth sector (host/horizon_build.cpp build_horizons(): per triangle 2 x 16 quantised horizons about the scene's flattest axis; touching neighbours bounded
    through the cone of their vertex differences, far geometry node by node). Three of four bounce rays leave an open terrain, each after walking the ~18 ancestors of
    its own leaf. Frames, weights and query counts (the culled rays stay closest-hit queries, rrt_render_stats::sky_culled) are identical bit for bit with and without:
    the gentle BASELINE terrain, steep noisy ones (valleys whose walls start on a triangle's own edge; also with z as the flat axis), the reference's tilted cubes and
    an enclosure whose light sits inside (nothing may be culled towards a wall), config 5's two meshes, a second terrain stacked above the first (overhangs), several
    pool passes, the reference-exact BVH (flags = 0: overlapping children, Q26 / Q27). RRT_HZ_CHECK makes the builder test 20 000 random rays it declares free against every triangle in double precision."""
    monkeypatch.setenv("RRT_HZ_CHECK", "20000")
    flags = RRT_FIXED_BVH
    if which in ("cfg4", "cfg4_passes", "cfg4_compat_bvh"):
        cfg, root = scenes.cfg4(workdir, xres=128, yres=96, nsamp=9, max_depth=6, n=64)
        if which == "cfg4_compat_bvh": flags = 0
    elif which.startswith("rough"):
        cfg, root = rough_terrain(workdir, {"rough_1": 1, "rough_2": 2, "rough_z_up": 3}[which])
        if which == "rough_z_up":      # the same terrain stood on its side (a rigid instance, flattened to world space): z becomes the scene's flattest axis
            cfg["Aggregate"]["primitives"][0]["instances"] = [{"rotation_axis": [1.0, 0.0, 0.0], "rotation_angle": -90.0}]
    elif which.startswith("boxes"):      # boxes resting on, sunk into, leaning on and a hair above a flat ground, as world-space triangles: coplanar contact, T-junctions, crossings
        cfg, root = boxes_on_a_plane(workdir, int(which[-1])); cfg["Film"]["xres"] = 96; cfg["Film"]["yres"] = 96
    elif which == "cfg2": cfg, root = scenes.cfg2(workdir, xres=96, yres=96, nsamp=9, max_depth=4); flags = 0
    elif which == "cfg3": cfg, root = scenes.cfg3(workdir, xres=96, yres=96, nsamp=9)
    elif which == "cfg5": cfg, root = scenes.cfg5(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=64)
    else:   # stacked: the terrain twice, the second copy 3 units above the first and shifted: rays that clear the lower terrain's horizon meet the upper one
        cfg, root = scenes.cfg4(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=48)
        cfg["Aggregate"]["primitives"][0]["instances"] = [{"world_pos": [0.0, 0.0, 0.0]}, {"world_pos": [1.3, 3.0, 0.7]}]
    sc = Scene.loads(cfg, root, flags=flags)
    r = Renderer(sc, 0, RRT_F32)
    if which == "cfg4_passes": r.set_option("max_paths", 128 * 96 * 3)
    out = {}
    for h in (1, 0):
        r.set_option("horizon_cull", h)
        out[h] = r.render(stats=True)
    r.close()
    assert out[1][0][..., :3].max() > 0
    assert np.array_equal(out[1][0], out[0][0])
    assert (out[1][1].camera_rays, out[1][1].closest_queries, out[1][1].any_queries) == (out[0][1].camera_rays, out[0][1].closest_queries, out[0][1].any_queries)
    assert out[0][1].sky_culled == 0
    print(f"horizon cull, {which}: {out[1][1].sky_culled} of {out[1][1].closest_queries} closest-hit queries answered by the tables")
    if which in ("cfg4", "cfg5", "cfg4_passes"): assert out[1][1].sky_culled > 0.05 * out[1][1].closest_queries     # (the steep terrains have high horizons: little to cull, and that little exactly)
    if which == "cfg4_compat_bvh": assert out[1][1].sky_culled > 0      # the cull is active on the reference-exact tree too
    if which == "cfg3": assert out[1][1].sky_culled == 0      # an enclosure: something is visible in every direction


def test_horizon_tables_are_built_once_per_geometry_and_can_be_switched_off(workdir, monkeypatch):
    """rrt_create builds the tables on the host (rrt_render_stats::s_horizon_build); a second handle on the same geometry finds them in the process cache (keyed by the
    content of the builder's input, not by address); RRT_HORIZON_TABLES=0 builds none - the frame is the same frame each time."""
    cfg, root = scenes.cfg4(workdir, xres=64, yres=64, nsamp=5, max_depth=4, n=40)
    cfg["Film"]["name"] = "unique_to_this_test"      # (nothing the builder sees)
    scenes.write_heightfield(workdir, n=40, seed=424242)      # geometry no other test of this process has built tables for
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r1 = Renderer(sc, 0, RRT_F32); f1, s1 = r1.render(stats=True)
    r2 = Renderer(sc, 0, RRT_F32); f2, s2 = r2.render(stats=True)
    monkeypatch.setenv("RRT_HORIZON_TABLES", "0")
    r3 = Renderer(sc, 0, RRT_F32); f3, s3 = r3.render(stats=True)
    for r in (r1, r2, r3): r.close()
    assert s1.s_horizon_build > 0 and s2.s_horizon_build == 0 and s3.s_horizon_build == 0
    assert s1.sky_culled > 0 and s2.sky_culled == s1.sky_culled and s3.sky_culled == 0
    assert np.array_equal(f1, f2) and np.array_equal(f1, f3)


@pytest.mark.parametrize("which", ["cfg4", "cfg5"])
def test_horizon_cull_changes_nothing_at_baseline_size(which, workdir):
    """The same invariance on the frames bench.py times (BASELINE config 4: 100 352 triangles, 1024 x 1024, 256 spp, depth 8 - 134 M closest-hit queries, a third
    of them answered by the tables; config 5: two meshes, micro-facet lobes, 2048 x 2048, 1 024 spp, depth 16 - 2.3 G queries, a quarter of them): identical bit for
    bit. A spawned ray's origin lies on its triangle to ~1e-9 only, so a ray that starts within that distance of an edge could in principle meet
    a neighbour the tables do not speak for; at this volume none does."""
    cfg, root = scenes.cfg4(workdir) if which == "cfg4" else scenes.cfg5(workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    out = {}
    for h in (1, 0):
        r.set_option("horizon_cull", h)
        out[h] = r.render(stats=True)
    r.close()
    st = out[1][1]
    print(f"horizon cull at BASELINE size: {st.sky_culled} of {st.closest_queries} closest-hit queries answered by the tables (built in {st.s_horizon_build:.2f} s); {st.ms_total:.1f} ms against {out[0][1].ms_total:.1f} ms without")
    assert st.sky_culled > 0.2 * st.closest_queries and out[0][1].sky_culled == 0
    assert (st.camera_rays, st.closest_queries, st.any_queries) == (out[0][1].camera_rays, out[0][1].closest_queries, out[0][1].any_queries)
    assert np.array_equal(out[1][0], out[0][0])


@pytest.mark.parametrize("which", ["cfg4", "cfg4_passes", "cfg2_f64", "cfg5", "cfg4_textured_translucent"])
def test_shade_compaction_changes_nothing(which, workdir):
    """k_shade_path packs the HITS of a chunk of queue entries (4 x the workgroup's size) into LDS before shading them (option "shade_compact"): on an
    open scene more than half of a queue's rays miss, the path integrator shades a miss with nothing (Q18), and one thread per queue entry left half of every
    wave idle. The hits keep their queue order inside a chunk and every sample adds to its own slot, so frames, weights and query counts are identical bit for
    bit with and without - also over several pool passes, in the f64 mode, with glossy materials and area lights, and in the general kernel."""
    prec = RRT_F32
    if which == "cfg2_f64":
        cfg, root = scenes.cfg2(workdir, xres=96, yres=96, nsamp=9, max_depth=4); prec = RRT_F64
    elif which == "cfg5":
        cfg, root = scenes.cfg5(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=64)
    else:
        cfg, root = scenes.cfg4(workdir, xres=128, yres=96, nsamp=9, max_depth=5, n=64)
    if which == "cfg4_textured_translucent":
        _with_material(cfg, "tl", ("TranslucentMaterial", {"kd": [0.4, 0.5, 0.6], "ks": [0.2, 0.2, 0.2], "reflect": [0.7, 0.7, 0.7], "transmit": [0.5, 0.5, 0.5]}, {"roughness": 0.2}, {}))
        cfg["Aggregate"]["primitives"][0]["material_name"] = "tl"
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, prec)
    if which == "cfg4_passes": r.set_option("max_paths", 128 * 96 * 3)
    out = {}
    for c in (1, 0):
        r.set_option("shade_compact", c)
        out[c] = r.render(stats=True)
    r.close()
    assert out[1][0][..., :3].max() > 0
    assert np.array_equal(out[1][0], out[0][0])
    assert (out[1][1].camera_rays, out[1][1].closest_queries, out[1][1].any_queries) == (out[0][1].camera_rays, out[0][1].closest_queries, out[0][1].any_queries)


@pytest.mark.parametrize("which", ["cfg4", "cfg4_stage_b", "cfg4_bands", "cfg2", "cfg4_direct"])
def test_root_cull_changes_nothing(which, workdir):
    """The fp32 path integrator's camera kernels answer a camera ray that misses the BVH's root box themselves - with the traversal kernels' own
    first test (lane_ray_begin: box_slabs_f32 on the root box) on the ray as the queue would hold it - instead of sending it through the queue:
    the miss it would have come back as is shaded with nothing. Frames, weights and the query counts (the culled rays stay closest-hit queries)
    are identical bit for bit with and without; stage B's survivors are culled the same way (aux_margin = 0 sends every survivor through stage
    B); DirectLighting keeps every ray in the queue (a miss without lights panics there, Q20)."""
    kw = dict(xres=128, yres=96, nsamp=9, max_depth=5, n=64)
    if which == "cfg2": cfg, root = scenes.cfg2(workdir, xres=64, yres=96, nsamp=9, max_depth=3)
    else: cfg, root = scenes.cfg4(workdir, **kw)
    if which == "cfg4_direct": cfg["Integrator"] = {"integrator_type": "DirectLighting", "max_depth": 3, "light_strategy": "UniformSampleAll"}
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    if which == "cfg4_stage_b": r.set_option("aux_margin", 0)
    out = {}
    for cull in (1, 0):
        r.set_option("root_cull", cull)
        if which == "cfg4_bands":
            parts = [r.render_bands(k, 3, stats=True) for k in range(3)]
            out[cull] = (sum(f for f, _ in parts), parts[1][1])
        else:
            out[cull] = r.render(stats=True)
    r.close()
    f1, s1 = out[1]; f0, s0 = out[0]
    assert np.array_equal(f1, f0) and f1[..., :3].max() > 0
    assert (s1.camera_rays, s1.closest_queries, s1.any_queries) == (s0.camera_rays, s0.closest_queries, s0.any_queries)
    assert s0.root_culled == 0
    if which == "cfg4_direct": assert s1.root_culled == 0
    else: assert 0 < s1.root_culled < s1.camera_rays


@pytest.mark.parametrize("which", ["cfg4", "cfg4_distant", "cfg4_far", "cfg2", "cfg3", "cfg3_direct", "cfg5_area", "cfg5_area_near", "cfg5_area_xform"])
def test_shadow_candidate_lists_change_nothing(which, workdir):
    """Shadow rays towards point / distant lights run down a per-(light, triangle) list of candidate leaves instead of walking the tree
    (dtraverse_f32.hpp k_shadow_lists_f32, host/shadow_lists.cpp build_shadow_lists()): a leaf's box test implies its ancestors', an occlusion query does
    not depend on the order, and the host lists every leaf whose box can meet a ray that starts on the triangle and points at the light. The
    same slab test on the same leaf boxes, the same triangle tests: frames and query counts with and without the lists are identical bit for
    bit - mesh at the origin and 1e5 units away, axis-aligned instanced cubes, an enclosure whose light sits inside it. Sphere-shaped area
    lights are sources too (cfg5_area: every point the light samples lies in its bounding sphere, the sweep towards it is a cone cut into
    pieces; rrt_render_stats::list_launches says the lists served the launches) - also close to the surface, where most triangles get no
    list and walk the tree inside the same kernel (cfg5_area_near), and with a scaled, rotated light transform."""
    if which == "cfg4": cfg, root = scenes.cfg4(workdir, xres=128, yres=128, nsamp=9, max_depth=6, n=96)
    elif which == "cfg4_distant": cfg, root = _cfg4_distant(workdir)
    elif which == "cfg4_far":
        cfg, root = scenes.cfg4(workdir, xres=128, yres=128, nsamp=9, max_depth=6, n=96)
        far = np.array([1.0e5, -7.0e4, 3.0e4])
        cfg["Aggregate"]["primitives"][0]["instances"] = [{"world_pos": list(far)}]
        cfg["Camera"]["world_pos"] = list(np.array(cfg["Camera"]["world_pos"], float) + far)
        cfg["Camera"]["look"] = list(np.array(cfg["Camera"]["look"], float) + far)
        cfg["lights"] = [{"light_type": "distant", "l": {"values": [3.0, 2.5, 2.0]}, "from": [20.0, 30.0, 10.0], "to": [35.0, 0.0, 0.0]}]
    elif which == "cfg2": cfg, root = scenes.cfg2(workdir, xres=128, yres=128, nsamp=9, max_depth=4)
    elif which == "cfg3": cfg, root = scenes.cfg3(workdir, xres=128, yres=128, nsamp=9)
    elif which == "cfg3_direct":
        cfg, root = scenes.cfg3(workdir, xres=128, yres=128, nsamp=9)
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3}
    else:
        cfg, root = scenes.cfg5(workdir, xres=96, yres=96, nsamp=9, max_depth=6, n=64)
        if which == "cfg5_area_near":      # lights 1.2 units above the surface, radius 1: directions spread over half a hemisphere
            for l in cfg["lights"]: l["light_shape"]["world_pos"][1] = 1.2
        if which == "cfg5_area_xform":     # a scaled, rotated sphere transform: the bounding sphere must follow it
            for k, l in enumerate(cfg["lights"]): l["light_shape"].update(scale=[1.5, 1.5, 1.5] if k % 2 else [0.5, 2.0, 1.0], rotation_axis=[1.0, 2.0, 3.0], rotation_angle=40.0)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    a, st_a = r.render(stats=True)
    assert st_a.list_launches == st_a.any_launches > 0, (st_a.list_launches, st_a.any_launches)
    r.set_option("shadow_lists", 0)
    b, st_b = r.render(stats=True)
    assert st_b.list_launches == 0
    r.set_option("any_entry", 0)               # ... and against the plain walk from the root
    c, st_c = r.render(stats=True)
    r.close()
    assert st_a.any_queries == st_b.any_queries == st_c.any_queries and st_a.any_queries > 1000
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert a[..., :3].max() > 0


def test_camera_halton_block_tables_change_nothing(workdir):
    """The fp32 camera kernel replaces the digit loops of Halton dimensions 1-3 (bases 3, 5, 7; halton.rs:107-128, lowdiscrepancy.rs:188-227)
    by two table look-ups each - the index split into a block of low digits and the rest, SceneDev::cam_lo / cam_hi. Same integers, same f64
    products: the sampler dimensions are identical bit for bit with and without the tables (and equal to the oracle's, test_camera_samples),
    and so are frames. 640 x 360 at 65 spp reaches indices of 12 base-5 digits; the first samples of the first pixels take the loop."""
    cfg, root = scenes.cfg2(workdir, xres=640, yres=360, nsamp=65, max_depth=2)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    rect = (0, 0, 256, 64)
    dims_on, rays_on, w_on = r.camera_samples(rect, 0, 65)
    film_on = r.render((192, 128, 448, 256))
    r.set_option("cam_tables", 0)
    dims_off, rays_off, w_off = r.camera_samples(rect, 0, 65)
    film_off = r.render((192, 128, 448, 256))
    r.close()
    assert dims_on.shape[0] == 256 * 64 * 65 and np.array_equal(dims_on, dims_off)
    assert np.array_equal(w_on, w_off) and np.array_equal(rays_on, rays_off, equal_nan=True)
    assert np.array_equal(film_on, film_off) and film_on[..., :3].max() > 0


@pytest.mark.parametrize("which", ["cfg4_path8", "cfg3_direct", "cfg2_glass_debug"])
def test_halton_block_tables_change_nothing(which, workdir):
    """The fp32 mode draws the sampler dimensions of the integrators (scrambled_radical_inverse, lowdiscrepancy.rs:204-227) from block tables
    too (SceneDev::hblk: the index split into a block of low digits and the rest, first 64 dimensions) - the same integers and the same f64
    products as the digit loops. Bar: frames and query counts with and without the tables are identical bit for bit (the oracle, which has no
    tables, holds the same frames in the render cases)."""
    if which == "cfg4_path8": cfg, root = scenes.cfg4(workdir, xres=160, yres=120, nsamp=17, max_depth=8, n=64)
    elif which == "cfg3_direct":
        cfg, root = scenes.cfg3(workdir, xres=128, yres=128, nsamp=9)
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3}
    else:
        cfg, root = scenes.cfg2(workdir, xres=128, yres=128, nsamp=9, max_depth=6)
        _with_material(cfg, "gl", ("GlassMaterial", {"kr": [1.0, 1.0, 1.0], "kt": [0.9, 0.9, 0.9]}, {"eta": 1.5}, {}))
        cfg["Aggregate"]["primitives"][0]["material_name"] = "gl"
        cfg["Integrator"] = {"integrator_type": "Debug", "max_depth": 6}
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    a, st_a = r.render(stats=True)
    r.set_option("halton_tables", 0)
    b, st_b = r.render(stats=True)
    r.close()
    assert st_a.closest_queries == st_b.closest_queries and st_a.any_queries == st_b.any_queries and st_a.closest_queries > 1000
    assert np.array_equal(a, b, equal_nan=True) and np.nanmax(a[..., :3]) > 0


AUX_CASES = {
    "cfg2_640x360": lambda wd: scenes.cfg2(wd, xres=640, yres=360, nsamp=9, max_depth=2),
    "cfg2_tiny_film": lambda wd: scenes.cfg2(wd, xres=24, yres=16, nsamp=65, max_depth=2),     # 0.05 px is 70 um of film here
    "cfg4_1024": lambda wd: scenes.cfg4(wd, xres=1024, yres=1024, nsamp=5, max_depth=2, n=40),
    "cfg3_wide_filter": lambda wd: (lambda c: (c[0]["Film"].__setitem__("Filter", {"filter_type": "TriangleFilter", "radius": [2.0, 2.0]}), c)[1])(
        scenes.cfg3(wd, xres=200, yres=120, nsamp=9)),
}


def _random_lens(seed):
    """scene.json's double Gauss with every radius, thickness and aperture perturbed (+-15 / 20 / 30 %), a random stop and focus distance: the
    margins of calibrate_aux_margins() are a calibrated heuristic (16x the displacement measured over 16 384 host samples of THIS lens, not a
    proven bound), so they are validated on prescriptions nobody tuned them on - rims and near-critical interfaces move with the prescription."""
    def make(wd):
        rng = np.random.default_rng(seed)
        cfg, root = scenes.cfg2(wd, xres=256, yres=160, nsamp=9, max_depth=2)
        ld = np.array(scenes.LENS_DATA, float).reshape(-1, 4)
        ld[:, 0] *= rng.uniform(0.85, 1.15, len(ld))
        ld[:, 1] *= rng.uniform(0.8, 1.2, len(ld))
        ld[:, 3] *= rng.uniform(0.7, 1.1, len(ld))
        cfg["Camera"]["lens_data"] = [float(x) for x in ld.reshape(-1)]
        cfg["Camera"]["aperture_diameter"] = float(rng.uniform(8.0, 50.0))
        cfg["Camera"]["focus_distance"] = float(rng.uniform(10.0, 60.0))
        return cfg, root
    return make


AUX_CASES.update({f"random_lens_{seed}": _random_lens(seed) for seed in range(1, 9)})


@pytest.mark.parametrize("which", sorted(AUX_CASES))
def test_aux_margins_change_nothing(which, workdir):
    """The fp32 camera kernels do not trace the auxiliary rays of generate_ray_differential (camera.rs:582-628) for a main ray that
    clears every lens interface by 16x the measured displacement of an auxiliary ray (host/scene_flatten.cpp calibrate_aux_margins()); all
    they decide on untextured scenes is whether the sample keeps its weight. Bar: with and without the shortcut every sample has
    the same weight and the frames are identical bit for bit - and the shortcut must actually be taken for most survivors."""
    cfg, root = AUX_CASES[which](workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    W, H = sc.resolution
    r = Renderer(sc, 0, RRT_F32)
    film_on, st_on = r.render(stats=True)
    rect = (0, 0, min(W, 256), min(H, 128))
    ns = int(sc.desc.sampler.samples_per_pixel)
    _, rays_on, w_on = r.camera_samples(rect, 1, min(ns, 9))
    r.set_option("aux_margin", 0)
    film_off, st_off = r.render(stats=True)
    _, rays_off, w_off = r.camera_samples(rect, 1, min(ns, 9))
    r.close()
    assert st_on.camera_rays == st_off.camera_rays and st_on.camera_rays > 0
    assert np.array_equal(w_on, w_off) and np.array_equal(rays_on, rays_off)
    assert np.array_equal(film_on, film_off)
    assert film_on[..., :3].max() > 0


def test_full_size_cfg5_frame_properties(workdir):
    """BASELINE config 5 at its full size (100 352 + 6 272 triangles, Plastic + Metal microfacets, 4 sphere area lights, 2048^2, 1024 spp,
    depth 16: 4.29 G camera samples in 16 pool passes, ~1 s per frame), fp32 product path, through size-independent properties: the
    closed-form filter weight sum 3 * (nsamp - 1) in every pixel (Q1, Q2, Q3), finite non-negative values, idempotence (bitwise), a 2-rank
    band partition that reassembles the frame exactly, and a 16-row slice at full spp against the f64 oracle."""
    cfg, root = scenes.cfg5(workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    assert sc.resolution == (2048, 2048) and int(sc.desc.sampler.samples_per_pixel) == 1025 and sc.desc.integrator.max_depth == 16
    r = Renderer(sc, 0, RRT_F32)
    film, st = r.render(stats=True)
    assert st.camera_samples == 2048 * 2048 * 1024
    assert 0.25 < st.camera_rays / st.camera_samples < 0.36
    assert np.all(film[..., 3] == 3.0 * 1024.0)
    assert np.isfinite(film).all() and film[..., :3].max() > 0 and film[..., 1].min() >= 0
    again = r.render()
    assert np.array_equal(again, film)
    bands = r.render_bands(0, 2)
    r.render_bands(1, 2, film=bands)
    assert np.array_equal(bands, film)
    rect = (768, 1024, 1280, 1040)      # 512 x 16 pixels at 1 024 spp: 8.4 M camera samples for the oracle
    ref = O.render(sc, rect)
    part = r.render(rect)
    r.close()
    y0, y1, x0, x1 = rect[1], rect[3], rect[0], rect[2]
    scale = np.abs(ref[y0:y1, x0:x1, :3]).max()
    diff = np.abs(part[y0:y1, x0:x1, :3].astype(np.float64) - ref[y0:y1, x0:x1, :3]).max(-1) / scale
    assert np.array_equal(part[y0:y1, x0:x1, 3], ref[y0:y1, x0:x1, 3])
    print("full-size cfg5 fp32 vs oracle: within 1e-4: %.4f, max %.3e, mean %.3e" % ((diff < 1e-4).mean(), diff.max(), diff.mean()))
    # 1 024 samples per pixel, depth 16, glossy lobes: a flipped discrete decision moves a pixel by one sample's share (1e-3 of a bright
    # sample); the bar is the one of the config-4 frame, scaled to the deeper paths
    assert (diff < 1e-3).mean() > 0.97 and diff.mean() < 2e-4, ((diff < 1e-3).mean(), diff.mean())


WIDE_FILTERS = {
    "triangle": {"filter_type": "TriangleFilter", "radius": [2.0, 2.0]},
    "gaussian": {"filter_type": "GaussianFilter", "radius": [2.0, 2.0], "alpha": 2.0},
    "gaussian_aniso": {"filter_type": "GaussianFilter", "radius": [1.5, 2.5], "alpha": 1.0},
    "box_wide": {"filter_type": "BoxFilter", "radius": [1.0, 0.75]},
}


@pytest.mark.parametrize("which", sorted(WIDE_FILTERS))
def test_wide_filters(which, workdir):
    """FilmTile::add_sample with filters wider than a pixel (film.rs:77-130, filters/trianglefilter.rs, gaussian.rs): a
    sample splats into every pixel within the radius through the 16x16 table (incl. Q4: the table only varies with y).
    f64: same sums up to the order of additions; fp32: the stated tolerance. Rect / band partitions still sum to the frame
    (splats that cross a border land in the neighbour's pixels: the multi-GPU reduce is a sum)."""
    cfg, root = scenes.cfg4(workdir, xres=48, yres=40, nsamp=5, max_depth=3, n=24)
    cfg["Film"]["Filter"] = WIDE_FILTERS[which]
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    ref = O.render(sc)
    scale = np.abs(ref[..., :3]).max()
    assert scale > 0 and ref[..., 3].min() > 0
    r = Renderer(sc, 0, RRT_F64)
    film = r.render()
    np.testing.assert_allclose(film[..., 3], ref[..., 3], rtol=1e-12)          # filter weight sums (x3, Q3)
    assert np.abs(film[..., :3] - ref[..., :3]).max() / scale < 1e-9
    parts = np.zeros_like(film)
    for rect in ((0, 0, 48, 16), (0, 16, 20, 40), (20, 16, 48, 40)):
        r.render(rect, film=parts)
    np.testing.assert_allclose(parts, film, rtol=1e-11, atol=1e-13 * scale)
    bands = np.zeros_like(film)
    for rank in range(3):
        bands += r.render_bands(rank, 3)
    np.testing.assert_allclose(bands, film, rtol=1e-11, atol=1e-13 * scale)
    r.set_option("max_paths", 700)   # several pixel groups and sample passes
    small = r.render()
    np.testing.assert_allclose(small, film, rtol=1e-11, atol=1e-13 * scale)
    r.close()
    r = Renderer(sc, 0, RRT_F32)
    f32 = r.render().astype(np.float64)
    r.close()
    assert np.abs(f32[..., :3] - ref[..., :3]).max() / scale < 1e-4
    np.testing.assert_allclose(f32[..., 3], ref[..., 3], rtol=1e-5)


# material parameters are texture *names* in the reference's schema (literals fall back to the defaults); a constant is
# spelled as a BilerpTexture with equal corners (renderprocess.rs:330-346 reads v01 for three of them)
TRANSMISSIVE = {
    "glass": ("GlassMaterial", {"kr": [0.9, 0.9, 0.9], "kt": [0.8, 0.9, 1.0]}, {"eta": 1.5}, {}),
    "glass_t_only": ("GlassMaterial", {"kr": [0.0, 0.0, 0.0]}, {"eta": 1.33}, {}),
    "rough_glass": ("GlassMaterial", {}, {"u_roughness": 0.3, "v_roughness": 0.2, "eta": 1.5}, {"remap_roughness": True}),
    "translucent": ("TranslucentMaterial", {"kd": [0.4, 0.3, 0.2], "ks": [0.3, 0.3, 0.3], "reflect": [0.5, 0.5, 0.5], "transmit": [0.6, 0.5, 0.4]},
                    {"roughness": 0.2}, {}),
}


def _with_material(cfg, name, spec):
    import copy
    mtype, rgbs, floats, extra = spec
    cfg["rgb_texture"] = list(cfg.get("rgb_texture", []))
    cfg["float_texture"] = list(cfg.get("float_texture", []))
    m = {"material_type": mtype, "material_name": name}
    for k, v in rgbs.items():
        cfg["rgb_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"{name}_{k}", "v00": {"values": v}, "v01": {"values": v}})
        m[k] = f"{name}_{k}"
    for k, v in floats.items():
        cfg["float_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"{name}_{k}", "v00": v, "v01": v})
        m[k] = f"{name}_{k}"
    m.update(extra)
    cfg["materials"] = copy.deepcopy(cfg["materials"]) + [m]


@pytest.mark.parametrize("which", sorted(TRANSMISSIVE))
def test_transmissive_materials_path(which, workdir):
    """GlassMaterial / TranslucentMaterial under the Path integrator (glass.rs, translucent.rs; FresnelSpecular,
    MicrofacetTransmission, LambertianTransmission reflection.rs:661-898,1029-1151; eta_scale path.rs:150-162,205-213):
    a tilted cube of the material inside the lit enclosure, so paths enter, bounce inside and leave."""
    cfg, root = _cfg3_tilted(workdir)
    cfg["Integrator"]["max_depth"] = 7
    cfg["Sampler"]["nsamp"] = 9
    _with_material(cfg, "mat_t", TRANSMISSIVE[which])
    cfg["Aggregate"]["primitives"][0]["material_name"] = "mat_t"
    sc = Scene.loads(cfg, root)
    m = sc.desc.materials[sc.desc.prims[0].material]
    assert m.type in (5, 6) and (which != "glass" or (list(m.kt) == [0.8, 0.9, 1.0] and m.index == 1.5))
    ref, st_ref = O.render(sc, stats=True)
    assert ref[..., :3].max() > 0
    r = Renderer(sc, 0, RRT_F64)
    film, st = r.render(stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert st.camera_rays == st_ref.camera_rays
    assert st.closest_queries > st_ref.camera_rays          # paths really continue through / inside the cube
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    assert diff.max() < 1e-9, diff.max()
    r = Renderer(sc, 0, RRT_F32)
    f32 = r.render().astype(np.float64)
    r.close()
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    # refraction at grazing angles amplifies fp32 rounding (total internal reflection is a threshold): statistical bar
    assert (d32 < 1e-4).mean() > 0.99 and np.median(d32) < 1e-5, ((d32 < 1e-4).mean(), d32.max())


@pytest.mark.parametrize("which", ["glass_direct_all", "glass_direct_one", "glass_debug", "rough_glass_direct", "translucent_direct"])
def test_transmissive_materials_direct(which, workdir):
    """DirectLighting / Debug with transmissive materials: li() = lights + specular_reflect + specular_transmit
    (directlighting.rs:72-132, integrator/mod.rs:150-301) is a binary recursion whose sampler dimensions are consumed
    depth-first, so the device walks each camera sample's tree in one thread (k_direct_tree). allow_multiple_lobes = false:
    smooth glass carries a SpecularReflection and a SpecularTransmission lobe here, not FresnelSpecular."""
    mat = {"glass": "glass", "rough": "rough_glass", "trans": "translucent"}[which[:5]]
    cfg, root = _cfg3_tilted(workdir)
    cfg["Sampler"]["nsamp"] = 9
    cfg["Integrator"] = {"integrator_type": "Debug" if which.endswith("debug") else "DirectLighting",
                         "light_strategy": "one" if which.endswith("one") else "all", "max_depth": 5}
    cfg["lights"] = cfg["lights"] + [{"light_type": "point", "spectrum": {"values": [20000, 30000, 40000]}}]
    _with_material(cfg, "mat_t", TRANSMISSIVE[mat])
    cfg["Aggregate"]["primitives"][0]["material_name"] = "mat_t"
    sc = Scene.loads(cfg, root)
    ref, st_ref = O.render(sc, stats=True)
    assert ref[..., :3].max() > 0
    if mat == "glass":   # the recursion really runs: specular children were traced
        assert st_ref.closest_queries > st_ref.camera_rays
    r = Renderer(sc, 0, RRT_F64)
    film, st = r.render(stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert (st.camera_rays, st.closest_queries, st.any_queries) == (st_ref.camera_rays, st_ref.closest_queries, st_ref.any_queries)
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    assert diff.max() < 1e-9, diff.max()
    r = Renderer(sc, 0, RRT_F32)
    f32 = r.render().astype(np.float64)
    r.close()
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    assert (d32 < 1e-4).mean() > 0.99 and np.median(d32) < 1e-5, ((d32 < 1e-4).mean(), d32.max())


def test_deep_direct_trees_use_the_overflow_frames(workdir):
    """DirectLighting in a mirror-walled enclosure around a matte and a glass cube at max_depth 22: every camera sample's recursion (k_direct_tree, taken
    because of the glass) is a mirror chain deeper than the 16 frames a thread keeps privately, so the deeper frames live in the strided
    global array. Same tree, same sampler dimensions, same query counts as the oracle's recursion (integrator/mod.rs:150-301)."""
    cfg, root = _cfg3_tilted(workdir)
    cfg["Film"]["xres"], cfg["Film"]["yres"] = 40, 40
    cfg["Sampler"]["nsamp"] = 5
    cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "one", "max_depth": 22}
    _with_material(cfg, "mat_t", TRANSMISSIVE["glass"])
    _with_material(cfg, "mat_m", ("MirrorMaterial", {"kr": [0.95, 0.9, 0.85]}, {}, {}))
    import copy
    cube, box = cfg["Aggregate"]["primitives"]                    # the matte cube is what the light reaches; the walls are mirrors
    box["material_name"] = "mat_m"
    glass = copy.deepcopy(cube)
    glass["material_name"] = "mat_t"
    glass["instances"] = [{"world_pos": [33.0, 1.5, 1.0], "rotation_axis": [2.0, 1.0, 3.0], "rotation_angle": 25}]
    cfg["Aggregate"]["primitives"].append(glass)
    sc = Scene.loads(cfg, root)
    ref, st_ref = O.render(sc, stats=True)
    assert ref[..., :3].max() > 0 and st_ref.closest_queries > 18 * st_ref.camera_rays      # chains beyond 16 levels
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        film, st = r.render(stats=True)
        r.close()
        assert np.array_equal(film[..., 3].astype(np.float64), ref[..., 3])
        diff = np.abs(film[..., :3].astype(np.float64) - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
        if prec == RRT_F64:
            assert (st.camera_rays, st.closest_queries, st.any_queries) == (st_ref.camera_rays, st_ref.closest_queries, st_ref.any_queries)
            assert diff.max() < 1e-9, diff.max()
        else:
            assert (diff < 1e-4).mean() > 0.98 and np.median(diff) < 1e-5, ((diff < 1e-4).mean(), diff.max())


@pytest.mark.parametrize("which", ["dims4_jitter", "dims20_nojitter", "golden_scene_json", "deep_direct_glass"])
def test_stratified_sampler(which, workdir):
    """StratifiedSampler (samplers/stratified.rs): strata + shuffle per sampled dimension, rng.gen_range(-1.0..1.0) for the
    dimensions beyond `dimension` (samplers/mod.rs:211-226), sample 0 skipped (Q1). The reference draws from thread_rng; the
    device and the oracle share a counter-based stand-in, so between them parity is exact.
    `golden_scene_json` is the reference's own samples/scene.json, unmodified (it selects this sampler). `deep_direct_glass`: a
    DirectLighting tree of depth 8 over smooth glass draws several hundred 1D / 2D dimensions per camera sample (specular_reflect and
    specular_transmit each draw at every vertex, integrator/mod.rs:170,225) - rounds 1-3 refused such a sample at 255 (8-bit counters in the
    path's queue word), round 4 packs 12-bit counters (dmath.hpp db_pack) and renders it like the oracle."""
    import os
    if which == "deep_direct_glass":
        cfg, root = scenes.cfg2(workdir, xres=24, yres=24, nsamp=4, max_depth=8)
        _with_material(cfg, "glass", ("GlassMaterial", {"kr": [1.0, 1.0, 1.0], "kt": [0.9, 0.9, 0.9]}, {"eta": 1.5}, {}))
        import copy
        prim = cfg["Aggregate"]["primitives"][0]
        for inst in prim["instances"]:
            inst["rotation_axis"] = [1.0, 2.0, 3.0]     # generic axes: no exact box / face ties
        matte = copy.deepcopy(prim)                     # one matte cube among the glass ones: something the point lights can be seen on, through the glass
        matte["instances"], prim["instances"] = prim["instances"][2:], prim["instances"][:2]
        prim["material_name"] = "glass"
        cfg["Aggregate"]["primitives"].append(matte)
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 8}
        cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 2, "jitter": True, "dimension": 6}
        sc = Scene.loads(cfg, root)
        rect = (0, 0, 24, 24)
    elif which == "golden_scene_json":
        sc = Scene.load(os.path.join(os.path.dirname(__file__), "golden", "scene.json"))
        W, H = sc.resolution
        rect = (W // 2 - 40, H // 2 - 24, W // 2 + 40, H // 2 + 24)
    else:
        cfg, root = scenes.cfg4(workdir, xres=48, yres=40, nsamp=5, max_depth=5, n=24)
        cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 3, "ysamp": 4, "jitter": which == "dims4_jitter",
                          "dimension": 4 if which == "dims4_jitter" else 20}
        sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
        rect = (0, 0, 48, 40)
    assert sc.desc.sampler.type == 1
    ref, st_ref = O.render(sc, rect, stats=True)
    r = Renderer(sc, 0, RRT_F64)
    dims, rays, w = r.camera_samples(rect, 1, 4)
    rdims, rrays, rw = O.camera_samples(sc, rect, 1, 4)
    assert np.array_equal(dims, rdims)                                   # the sampler itself: bit-exact
    np.testing.assert_allclose(w, rw, rtol=1e-10, atol=0)
    film, st = r.render(rect, stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert st.camera_rays == st_ref.camera_rays
    scale = np.abs(ref[..., :3]).max()
    assert scale > 0
    d = np.abs(film[..., :3] - ref[..., :3]).max(-1) / scale
    if which == "golden_scene_json":   # axis-aligned cubes: exact box / face ties (module docstring)
        assert (d > 1e-9).mean() < 0.005, (d > 1e-9).mean()
    else:
        assert d.max() < 1e-9, d.max()
    r = Renderer(sc, 0, RRT_F32)
    f32 = r.render(rect).astype(np.float64)
    r.close()
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / scale
    # (deep_direct_glass: seven refractions in a row carry an fp32 rounding difference into the occasional other facet)
    assert (d32 < 1e-4).mean() > (0.97 if which in ("golden_scene_json", "deep_direct_glass") else 0.995), (d32 < 1e-4).mean()


def _sphere_zoo(wd, integrator, xres=48, yres=48, nsamp=5):
    """Sphere primitives next to triangles: plain instanced spheres (cfg1 style), clipped spheres (z_min / z_max /
    phi_max), a sphere with its own to_world (Q16: first p_hit taken from the un-transformed ray), a scaled instance
    (Q15: t copied across spaces) and a triangle heightfield below them, so leaves mix both shapes."""
    cfg, root = scenes.cfg4(wd, xres=xres, yres=yres, nsamp=nsamp, max_depth=4, n=24)
    cfg["Integrator"] = integrator
    prims = cfg["Aggregate"]["primitives"]
    prims.append({"primitive_type": "sphere", "material_name": "mat_matte", "radius": 0.75,
                  "instances": [{"world_pos": [33.0 + 0.4 * k, 1.5 + 0.2 * k, -5.0 + 2.0 * k]} for k in range(6)]})
    prims.append({"primitive_type": "sphere", "material_name": "mat_matte", "radius": 1.25, "z_min": -0.5, "z_max": 0.9, "phi_max": 250.0,
                  "instances": [{"world_pos": [36.0, 2.5, 0.0], "rotation_axis": [1.0, 2.0, 3.0], "rotation_angle": 40},
                                {"world_pos": [31.0, 2.0, 3.0], "rotation_axis": [0.0, 1.0, 0.0], "rotation_angle": 200, "scale": [1.5, 0.75, 1.0]}]})
    prims.append({"primitive_type": "sphere", "material_name": "mat_matte", "radius": 1.0, "world_pos": [0.3, 0.2, -0.1],
                  "instances": [{"world_pos": [34.0, 3.0, -3.0]}]})
    prims.append({"primitive_type": "sphere", "material_name": "mat_matte", "radius": 0.9, "world_pos": [37.0, 2.0, 4.0]})
    return cfg, root


def test_sphere_primitives_trace_f64_exact(workdir):
    """Sphere::intersect / intersect_p behind Geometric/TransformedPrimitive (sphere.rs:51-259, primitives.rs:51-139):
    same winner, same t, same occlusion bit and the same node / primitive-test counts as the oracle."""
    cfg, root = _sphere_zoo(workdir, {"integrator_type": "Path", "max_depth": 4})
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    assert sc.desc.n_spheres >= 4
    o, d, tmax = O.random_rays(sc, 20000, 77)
    ref = O.trace_closest(sc, o, d, tmax)
    assert (ref["prim"] >= 0).mean() > 0.2
    r = Renderer(sc, 0, RRT_F64)
    got = r.trace_closest(o, d, tmax, counters=True)
    assert np.array_equal(got["prim"], ref["prim"])
    hit = ref["prim"] >= 0
    assert np.array_equal(got["t"][hit], ref["t"][hit])
    assert np.array_equal(got["nodes"], ref["nodes"]) and np.array_equal(got["prims"], ref["prims"])
    tm = np.full(len(o), 1.0 - 1e-4)
    ref_any = O.trace_any(sc, o, d, tm)
    got_any = r.trace_any(o, d, tm)
    assert np.array_equal(np.asarray(got_any).astype(bool), ref_any["occluded"])
    r.close()
    # fp32: same winners except where fp32 rounding decides (grazing rays)
    for mode in (3, 2, 1, 0):
        r = Renderer(sc, 0, RRT_F32)
        if mode != 3:
            r.set_option("persistent_traversal", mode)
        got32 = r.trace_closest(o, d, tmax)
        any32 = r.trace_any(o, d, tm)
        r.close()
        assert (got32["prim"] == ref["prim"]).mean() > 0.999, mode
        both = (got32["prim"] == ref["prim"]) & hit
        np.testing.assert_allclose(got32["t"][both], ref["t"][both], rtol=2e-4)
        assert (np.asarray(any32).astype(bool) == ref_any["occluded"]).mean() > 0.999, mode


@pytest.mark.parametrize("which", ["cfg1", "zoo_direct", "zoo_path", "zoo_debug"])
def test_sphere_primitives_render(which, workdir):
    if which == "cfg1":
        cfg, root = scenes.cfg1(workdir, xres=64, yres=64, nsamp=3)
        flags = 0
    else:
        integ = {"zoo_direct": {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3},
                 "zoo_path": {"integrator_type": "Path", "max_depth": 4},
                 "zoo_debug": {"integrator_type": "Debug"}}[which]
        cfg, root = _sphere_zoo(workdir, integ)
        flags = RRT_FIXED_BVH
    sc = Scene.loads(cfg, root, flags=flags)
    ref, st_ref = O.render(sc, stats=True)
    assert ref[..., :3].max() > 0
    r = Renderer(sc, 0, RRT_F64)
    film, st = r.render(stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert st.camera_rays == st_ref.camera_rays
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    # A ray spawned on a sphere re-tests that sphere with c = |o|^2 - r^2 ~ 1e-16 of either sign (no epsilon in
    # sphere.rs): the reference's own pixels depend on that rounding noise. The f64 device mode replays the same
    # operations, so it must still agree, up to libm-vs-device atan2/acos/sin last-ulp differences.
    assert (diff > 1e-9).mean() < 0.01, ((diff > 1e-9).mean(), diff.max())
    # fp32 product: keeps the same un-epsilon'd test, so spawned rays self-hit with the same ~50 % odds but on
    # different samples: the image agrees with the oracle in the mean, not pixel by pixel (cfg1 at 2 spp is itself
    # noisy: 15 %; the zoo's spheres cover less of the frame: 5 %).
    for mode in (3, 2, 1, 0):      # default (by queue size), persistent-thread pair-node kernel, grid-stride pair-node kernel, generic kernels
        r = Renderer(sc, 0, RRT_F32)
        if mode != 3:
            r.set_option("persistent_traversal", mode)
        film32 = r.render()
        r.close()
        assert np.array_equal(film32[..., 3].astype(np.float64), ref[..., 3])
        ratio = film32[..., :3].mean() / ref[..., :3].mean()
        print(f"spheres {which}, traversal mode {mode}: fp32 mean / oracle mean = {ratio:.4f}")
        assert abs(ratio - 1.0) < (0.15 if which == "cfg1" else 0.05), ratio


SPHERE_MATERIALS = {
    "matte": (("MatteMaterial", {"kd": [0.6, 0.5, 0.4]}, {}, {}), 5, 0.03),
    "rough_metal": (("MetalMaterial", {}, {"roughness": 0.2}, {}), 5, 0.03),
}


@pytest.mark.parametrize("which", sorted(SPHERE_MATERIALS))
def test_fp32_spheres_at_a_converged_sample_count(which, workdir):
    """Sphere pixels of the reference are decided by coin flips (a spawned ray re-tests its own sphere with c = |o|^2 - r^2 of one ulp of
    either sign, no epsilon in sphere.rs), which fp32 cannot replay coin for coin: the product mode is held to the f64 mode - itself held
    to the oracle pixel for pixel - in the mean, at a converged sample count (config 1's 24 spheres, 64 spp, every sphere the same
    material). Measured (tools/sphere_debug.py): matte 1.016-1.03, rough metal 1.007-1.02 at depth 5. Transmissive spheres are not held to
    anything in fp32: see test_fp32_transmissive_spheres_are_disclaimed."""
    spec, depth, bar = SPHERE_MATERIALS[which]
    cfg, root = scenes.cfg1(workdir, xres=64, yres=64, nsamp=65)
    _with_material(cfg, "sph", spec)
    for prim in cfg["Aggregate"]["primitives"]:
        prim["material_name"] = "sph"
    cfg["Integrator"] = {"integrator_type": "Path", "max_depth": depth}
    sc = Scene.loads(cfg, root)
    means = {}
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        film = r.render().astype(np.float64)
        r.close()
        assert np.all(film[..., 3] == 3.0 * 64.0)
        means[prec] = film[..., :3].mean()
    ratio = means[RRT_F32] / means[RRT_F64]
    print(f"spheres, {which}: fp32 mean / f64 mean = {ratio:.4f}")
    assert means[RRT_F64] > 0 and abs(ratio - 1.0) < bar, ratio


@pytest.mark.parametrize("which", sorted(SPHERE_MATERIALS))
def test_fp32_opaque_spheres_per_pixel(which, workdir):
    """Row a11, read per pixel. The coins of sphere.rs (a spawned ray re-hits its own sphere at t ~ 0 when c = |o|^2 - r^2
    falls on the wrong side of 0, about every second ray) are tossed per SAMPLE, so the most fp32 could promise for an opaque sphere is that its
    pixel converges to the pixel the f64 mode - the reference's coins, held to the oracle pixel for pixel - converges to. Measured here at
    1 024 spp as 16 batches of 64 spp with independent Halton scramblings (rrt_scene_load's perm_seed), the same 16 seeds in both modes:
    sigma_batch = the f64 mode's standard deviation of a 64-spp pixel estimate over the batches (the per-sample sigma / sqrt(64)); z = |mean_fp32 -
    mean_f64| / (sigma / sqrt(N)) per channel, sigma / sqrt(N) = sigma_batch / sqrt(16).
    What the measurement says (printed): the fp32 mode is NOT unbiased. Its coin falls a little less often on the self-hit side, the image mean
    comes out 3.3-3.7 % brighter than the f64 mode's, and where independent coins on shared samples would put 99.5 % of an unbiased mode's
    pixels inside z < 4 (the difference of two such estimates has variance 2 sigma^2 / N: median z 0.95) matte spheres put 97.4 % and rough
    metal spheres - whose highlights concentrate the difference in few pixels: 95th percentile z = 6.0 - 88.9 %. The median z is 0.95 / 0.94:
    most pixels sit where an unbiased mode would; the bias lives in a tail of pixels. So the statement this test holds is a BOUND on that
    bias, not unbiasedness: per pixel within 4 sigma / sqrt(N) for >= 95 % (matte) / >= 85 % (rough metal) of the pixels a sphere covers,
    median z below 1.5, image mean within 5 %; sphere scenes that matter belong in RRT_F64."""
    spec, depth, _ = SPHERE_MATERIALS[which]
    B, spp = 16, 64
    sums = {RRT_F64: [], RRT_F32: []}
    for b in range(B):
        cfg, root = scenes.cfg1(workdir, xres=48, yres=48, nsamp=spp + 1)
        _with_material(cfg, "sph", spec)
        for prim in cfg["Aggregate"]["primitives"]:
            prim["material_name"] = "sph"
        cfg["Integrator"] = {"integrator_type": "Path", "max_depth": depth}
        sc = Scene.loads(cfg, root, perm_seed=0x1234_5678_9abc_def0 + 977 * b)
        for prec in (RRT_F64, RRT_F32):
            r = Renderer(sc, 0, prec)
            film = r.render().astype(np.float64)
            r.close()
            assert np.all(film[..., 3] == 3.0 * spp)
            sums[prec].append(film[..., :3] / spp)       # the batch's pixel estimate (box filter: the sum of its samples' contributions / spp)
    m64, m32 = np.stack(sums[RRT_F64]), np.stack(sums[RRT_F32])          # (B, H, W, 3)
    mean64, mean32 = m64.mean(0), m32.mean(0)
    sigma_batch = m64.std(0, ddof=1)
    covered = mean64.max(-1) > 0
    bar = 4.0 * sigma_batch / np.sqrt(B) + 1e-4 * mean64.max()
    ok = (np.abs(mean32 - mean64) < bar).all(-1)
    z = (np.abs(mean32 - mean64) / (sigma_batch / np.sqrt(B) + 1e-12))[covered]
    ratio = mean32.mean() / mean64.mean()
    print(f"spheres, {which}: {int(covered.sum())} covered pixels, {ok[covered].mean():.4f} within 4 sigma / sqrt(N) at N = {B * spp}; median |z| {np.median(z):.2f}, "
          f"95th percentile {np.percentile(z, 95):.2f}; fp32 mean / f64 mean = {ratio:.4f}")
    assert covered.sum() > 200
    assert ok[covered].mean() >= {"matte": 0.95, "rough_metal": 0.85}[which], ok[covered].mean()
    assert np.median(z) < 1.5, np.median(z)
    assert abs(ratio - 1.0) < 0.05, ratio


def test_fp32_transmissive_spheres_are_disclaimed(workdir):
    """Every refraction through a Glass / Translucent sphere spawns a ray ON the sphere; whether it leaves or re-hits at t ~ 0 is decided by the
    last bit of |o|^2 - r^2 (sphere.rs:124-259 has no epsilon), and a chain of such coins amplifies any change of the fp32 rounding sequence:
    the fp32 / f64 ratio of the mean moved from 0.99 to 1.36 at depth 2 when only the compiler's instruction selection changed, and is 2.2 at
    depth 5. A bar wide enough to hold that cannot fail, so there is none: the fp32 handle says so at creation
    (rrt_warning, printed by rrt_render / deploy_render like the reference's eprintln! diagnostics), the f64 handle - which replays the
    reference's coins and is held to the oracle pixel for pixel by test_sphere_primitives_render - does not, and neither does an fp32 handle
    on a scene whose spheres are opaque."""
    cfg, root = scenes.cfg1(workdir, xres=32, yres=32, nsamp=5)
    sc_opaque = Scene.loads(cfg, root)
    _with_material(cfg, "sph", ("GlassMaterial", {"kr": [1.0, 1.0, 1.0], "kt": [0.9, 0.9, 0.9]}, {"eta": 1.5, "u_roughness": 0.2, "v_roughness": 0.1}, {}))
    cfg["Aggregate"]["primitives"][0]["material_name"] = "sph"
    cfg["Integrator"] = {"integrator_type": "Path", "max_depth": 2}
    sc = Scene.loads(cfg, root)
    r32, r64, ro = Renderer(sc, 0, RRT_F32), Renderer(sc, 0, RRT_F64), Renderer(sc_opaque, 0, RRT_F32)
    assert len(r32.warnings) == 1 and "RRT_F64" in r32.warnings[0] and "sphere.rs" in r32.warnings[0]
    assert r64.warnings == [] and ro.warnings == []
    film = r32.render()
    assert np.isfinite(film).all() and np.all(film[..., 3] == 3.0 * 4.0)       # it still renders: the weights are exact, the radiance unclaimed
    for r in (r32, r64, ro):
        r.close()


def test_fp32_difference_found_by_the_fuzz_sweep_is_one_sample_on_a_shared_edge():
    """Fuzz seed 508 case 96 (tests/golden/fuzz508_96/: a tilted cube in a tilted box, a plastic whose roughness is a 3D checkerboard and a
    textured mirror, StratifiedSampler, TriangleFilter, Path depth 1) was the one fp32 image over the sweep's bar: 8 pixels off by up to 0.14 of
    the maximum. Traced (tools/trace_case.py): ONE camera sample, pixel (30, 30), whose ray meets the cube's front face
    7.6e-6 (barycentric) from the diagonal shared by triangles 12 and 13. Moller-Trumbore's u, v carry an fp32 error of eps * |O - p0| / edge
    ~ 1e-5 for a ray from 44 units away: both triangles reject it, the ray flies through the face and hits the back one (triangle 18,
    2.15 units further); the triangle filter spreads that one sample over 8 pixels. The f64 mode accepts triangle 13 like the oracle.
    The rule this test pins: with the box filter, every fp32 pixel outside 1e-4 holds a sample whose oracle hit lies within 5e-5
    (barycentric) of a triangle edge - the reference's own non-watertight test (Q12) at fp32 resolution - and there are at most 2 such
    pixels of 4 096; the f64 device mode has none."""
    import json
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz508_96")
    cfg = json.load(open(os.path.join(root, "scene.json")))
    cfg["Film"]["Filter"] = {"filter_type": "BoxFilter", "radius": [0.5, 0.5]}   # (the sampler dimensions do not depend on the filter)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    ref = O.render(sc)
    scale = np.abs(ref[..., :3]).max()
    r64 = Renderer(sc, 0, RRT_F64)
    f64 = r64.render()
    r64.close()
    assert (np.abs(f64[..., :3] - O.render(sc)[..., :3]).max() / scale) < 1e-9
    r = Renderer(sc, 0, RRT_F32)
    f32 = r.render().astype(np.float64)
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / scale
    bad = np.argwhere(d32 > 1e-4)
    print("fuzz 508/96 with the box filter: fp32 pixels beyond 1e-4:", bad.tolist(), "max", d32.max())
    assert len(bad) <= 2
    ns = int(sc.desc.sampler.samples_per_pixel)
    for y, x in bad:
        _, rays, w = O.camera_samples(sc, (int(x), int(y), int(x) + 1, int(y) + 1), 1, ns)
        live = w > 0
        h = O.trace_closest(sc, rays[live, :3], rays[live, 3:], np.full(int(live.sum()), np.inf))
        hit = h["prim"] >= 0
        edge = np.minimum(np.minimum(h["u"], h["v"]), 1.0 - h["u"] - h["v"])[hit]
        assert edge.min() < 5e-5, (x, y, edge)
    r.close()


def _tr_sample_11(cos_t, u1, u2, T):
    """trowbridge_reitz_sample_11's slope_x (microfacet.rs:270-305), in the arithmetic of type T."""
    one = T(1)
    sin_t = np.sqrt(max(T(0), one - cos_t * cos_t)); tan_t = sin_t / cos_t; a = one / tan_t
    g1 = T(2) / (one + np.sqrt(one + one / (a * a)))
    a = T(2) * u1 / g1 - one
    with np.errstate(divide="ignore"):
        tmp = one / (a * a - one)
    tmp = min(tmp, T(1e10))
    b = tan_t
    d = np.sqrt(max(b * b * tmp * tmp - (a * a - b * b) * tmp, T(0)))
    return b * tmp - d if (a < 0 or b * tmp + d > one / tan_t) else b * tmp + d


def test_fp32_difference_found_by_the_fuzz_sweep_is_a_sampler_value_of_exactly_zero():
    """Fuzz seed 416 case 43 (tests/golden/fuzz416_43/: three tilted cubes of a TranslucentMaterial with all four lobes, StratifiedSampler 2 x 2
    WITHOUT jitter, Path depth 6): 59 of 1 600 fp32 pixels beyond 1e-4 of the oracle with the box filter, the f64 device mode exact. Traced
    (tools/trace_416_43.py) to one value, not to a comparison that flips: unjittered 2 x 2 strata hand every sampler
    dimension 0.25 or 0.75; Bsdf::sample_f (reflection.rs:302-381) picks lobe floor(u0 * matching) and remaps u0 to u0 * matching - comp, which with
    matching = 4 lobes is EXACTLY 0 (0.25 * 4 = 1, 0.75 * 4 = 3); a microfacet lobe hands it to trowbridge_reitz_sample_11
    (microfacet.rs:270-325) as u1 = 0: a = 2 u1 / G1 - 1 = -1, tmp = 1 / (a^2 - 1) = inf -> clamped to 1e10, and slope_x = b tmp - sqrt(b^2 tmp^2 -
    (a^2 - b^2) tmp) is the difference of two numbers of the size 1e10 whose true value is O(1). f64 (ulp(1e10) = 2e-6) keeps six digits of it,
    fp32 (ulp(1e10) = 1 024) none: the sampled microfacet normal is a different vector, the path a different path. A measure-zero input - no
    jittered or low-discrepancy sampler ever hands out an exact 0 - for which no fp32 claim is made. The rule this test pins, on the committed
    scene: the difference needs BOTH the four-lobe material and a stratification whose values times four are integers - two lobes, jitter, or
    8 x 8 strata leave no fp32 pixel beyond 1e-4, 3 x 3 strata (the middle stratum 0.5 * 4 = 2) bring it back - and the f64 device mode equals
    the oracle on every variant; the cancellation itself is shown on the host in both arithmetics."""
    # the singularity, host arithmetic: u1 = 0 loses every digit in fp32, u1 = 1e-3 loses none that matter
    for cos_t in (0.3, 0.5):
        s64, s32 = _tr_sample_11(np.float64(cos_t), np.float64(0.0), 0.25, np.float64), _tr_sample_11(np.float32(cos_t), np.float32(0.0), 0.25, np.float32)
        exact = (1.0 - (np.sqrt(1 - cos_t * cos_t) / cos_t) ** 2) / (2.0 * np.sqrt(1 - cos_t * cos_t) / cos_t)     # limit of b tmp - d for tmp -> inf: (1 - b^2) / (2 b)
        assert abs(s64 - exact) < 1e-4 and abs(float(s32) - exact) > 0.3, (cos_t, s64, s32, exact)
        t64, t32 = _tr_sample_11(np.float64(cos_t), np.float64(1e-3), 0.25, np.float64), _tr_sample_11(np.float32(cos_t), np.float32(1e-3), 0.25, np.float32)
        assert abs(float(t32) - t64) < 2e-3 * max(1.0, abs(t64)), (cos_t, t64, t32)
    import copy, json
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz416_43")
    base = json.load(open(os.path.join(root, "scene.json")))
    base["Film"]["Filter"] = {"filter_type": "BoxFilter", "radius": [0.5, 0.5]}   # (the sampler dimensions do not depend on the filter)
    black = {"texture_name": "c_black", "texture_type": "BilerpTexture", "v00": {"values": [0, 0, 0]}, "v01": {"values": [0, 0, 0]}}
    results = {}
    for name in ("original", "two_lobes_no_glossy", "two_lobes_no_transmission", "jitter", "strata_3x3", "strata_8x8"):
        cfg = copy.deepcopy(base)
        mat = [m for m in cfg["materials"] if m.get("material_name") == "fz13"][0]
        if name == "two_lobes_no_glossy": mat["ks"] = "c_black"; cfg["rgb_texture"].append(black)
        if name == "two_lobes_no_transmission": mat["transmit"] = "c_black"; cfg["rgb_texture"].append(black)
        if name == "jitter": cfg["Sampler"]["jitter"] = True
        if name == "strata_3x3": cfg["Sampler"].update(xsamp=3, ysamp=3)
        if name == "strata_8x8": cfg["Sampler"].update(xsamp=8, ysamp=8)
        sc = Scene.loads(cfg, root)
        ref_flat, ref = O.render(sc, flat=True), O.render(sc)
        scale = np.abs(ref[..., :3]).max()
        r64 = Renderer(sc, 0, RRT_F64); f64 = r64.render(); r64.close()
        assert np.abs(f64[..., :3] - ref[..., :3]).max() / scale < 1e-9, name
        r32 = Renderer(sc, 0, RRT_F32); f32 = r32.render().astype(np.float64); r32.close()
        d32 = np.abs(f32[..., :3] - ref_flat[..., :3]).max(-1) / scale
        results[name] = (int((d32 > 1e-4).sum()), f32[..., :3].mean() / ref_flat[..., :3].mean())
    print("fuzz 416/43, fp32 pixels beyond 1e-4 of 1 600 and mean ratio per variant:", results)
    for name in ("two_lobes_no_glossy", "two_lobes_no_transmission", "jitter", "strata_8x8"):
        assert results[name][0] == 0 and abs(results[name][1] - 1.0) < 1e-3, (name, results[name])
    for name in ("original", "strata_3x3"):     # the singular inputs: different paths for the affected samples, the image still the same image in the mean
        assert results[name][0] > 0 and abs(results[name][1] - 1.0) < 0.05, (name, results[name])


def test_unsupported_and_panics(workdir):
    cfg, root = scenes.cfg2(workdir, xres=32, yres=32, nsamp=3)
    cfg["Integrator"] = {"integrator_type": "DirectLighting"}
    cfg["lights"] = []
    sc = Scene.loads(cfg, root)
    r = Renderer(sc, 0, RRT_F32)
    with pytest.raises(RrtPanic):
        r.render()                                               # Q20: unbounded recursion in the reference
    from rs_ray_toy_amd import RrtError
    # handle options are validated, not stored blindly (rg_spb = 3 made the camera workgroups generate their last samples twice)
    for key, bad in (("rg_spb", 3), ("rg_spb", 0), ("max_paths", 1), ("no_such_option", 1)):
        with pytest.raises(RrtError):
            r.set_option(key, bad)
    r.set_option("rg_spb", 4)
    r.close()
    cfg["lights"] = [{"light_type": "point", "world_pos": [25.0, 8.0, 4.0], "spectrum": {"values": [800, 800, 800]}}]
    cfg["Integrator"] = {"integrator_type": "Path", "max_depth": 300}      # under the StratifiedSampler the bounce count rides in 8 bits of a path's queue word (dmath.hpp db_pack)
    cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 2, "jitter": True, "dimension": 4}
    r = Renderer(Scene.loads(cfg, root), 0, RRT_F32)
    with pytest.raises(RrtUnsupported):
        r.render()
    r.close()


# ---- textures: texture graph + ray differentials on the device -----------------------------
def _const_rgb(name, v):
    return {"texture_name": name, "texture_type": "BilerpTexture", "v00": {"values": v}, "v01": {"values": v}}


ROT = {"rotation_axis": [1.0, 2.0, 0.5], "rotation_angle": 25.0}


def _tex_case(which, wd):
    cfg, root = _cfg3_tilted(wd)
    cfg["Sampler"]["nsamp"] = 9
    cube, box = cfg["Aggregate"]["primitives"]
    if which == "path_checker_uv":
        cfg["float_texture"] = [{"texture_name": "sig", "texture_type": "BilerpTexture", "v00": 0.0, "v01": 40.0}]
        cfg["rgb_texture"] = [_const_rgb("w", [0.8, 0.8, 0.7]), {"texture_name": "uvt", "texture_type": "UVTexture", "mapping": {"mapping": "uv", "su": 2.0, "sv": 3.0}},
                              {"texture_name": "uvs", "texture_type": "ScaleTexture", "t1": "uvt", "t2": "w"},
                              {"texture_name": "chk", "texture_type": "CheckerBoardTexture", "t1": "w", "t2": "uvs",
                               "mapping": {"mapping": "uv", "su": 6.0, "sv": 6.0, "du": 0.0, "dv": 0.0}},
                              {"texture_name": "mixc", "texture_type": "MixTexture", "t1": "chk", "t2": "uvt"}]
        cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_box", "kd": "chk", "sigma": "sig"},
                                               {"material_type": "MatteMaterial", "material_name": "m_cube", "kd": "mixc"}]
        cube["material_name"], box["material_name"] = "m_cube", "m_box"
    elif which == "path_noise":
        cfg["float_texture"] = [{"texture_name": "lo", "texture_type": "BilerpTexture", "v00": 0.05, "v01": 0.05},
                                {"texture_name": "hi", "texture_type": "BilerpTexture", "v00": 0.3, "v01": 0.3},
                                {"texture_name": "rough", "texture_type": "CheckerBoardTexture", "dimension": 3, "t1": "lo", "t2": "hi", **ROT, "scale": [0.5, 0.5, 0.5]}]
        cfg["rgb_texture"] = [_const_rgb("tint", [0.9, 0.6, 0.3]), {"texture_name": "wr", "texture_type": "WrinkledTexture", "octaves": 5, "omega": 0.6, **ROT},
                              {"texture_name": "wrt", "texture_type": "ScaleTexture", "t1": "wr", "t2": "tint"},
                              {"texture_name": "wind", "texture_type": "WindyTexture", **ROT, "scale": [3.0, 3.0, 3.0]},
                              {"texture_name": "sph", "texture_type": "CheckerBoardTexture", "t1": "tint", "mapping": {"mapping": "spherical"}, **ROT,
                               "world_pos": [35.0, 0.0, 0.0], "scale": [0.05, 0.1, 0.05]}]
        cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_box", "kd": "wrt"},
                                               {"material_type": "PlasticMaterial", "material_name": "m_cube", "kd": "sph", "ks": "wind", "roughness": "rough"}]
        cube["material_name"], box["material_name"] = "m_cube", "m_box"
    elif which in ("direct_mirror_patch", "debug_glass_patch"):
        _write_patch(wd)
        cfg["objs"] = cfg["objs"] + [{"filename": "patch.obj", "obj_name": "patch_01"}]
        cfg["Integrator"] = {"integrator_type": "DirectLighting" if which.startswith("direct") else "Debug", "light_strategy": "all", "max_depth": 4}
        cfg["lights"] = cfg["lights"] + [{"light_type": "point", "spectrum": {"values": [20000, 30000, 40000]}}]
        cfg["float_texture"] = [{"texture_name": "ior", "texture_type": "BilerpTexture", "v00": 1.3, "v01": 1.7}]
        cfg["rgb_texture"] = [_const_rgb("w", [0.9, 0.9, 0.9]), _const_rgb("k", [0.15, 0.1, 0.3]),
                              {"texture_name": "chk", "texture_type": "CheckerBoardTexture", "t1": "w", "t2": "k",
                               "mapping": {"mapping": "planar", "v1": [0.25, 0.0, 0.0], "v2": [0.0, 0.1, 0.25], "udelta": 0.3, "vdelta": 0.1}},
                              {"texture_name": "cyl", "texture_type": "CheckerBoardTexture", "t1": "w", "t2": "k", "mapping": {"mapping": "cylindrical"}, **ROT,
                               "world_pos": [35.0, 0.0, 0.0], "scale": [0.1, 0.1, 0.1]},
                              {"texture_name": "kr", "texture_type": "CheckerBoardTexture", "aamode": "none", "t1": "w", "t2": "k",
                               "mapping": {"mapping": "uv", "su": 5.0, "sv": 5.0, "du": 0.0, "dv": 0.0}}]
        if which.startswith("direct"):
            patch_mat = {"material_type": "MirrorMaterial", "material_name": "m_patch", "kr": "kr"}
        else:
            patch_mat = {"material_type": "GlassMaterial", "material_name": "m_patch", "kr": "kr", "kt": "w", "eta": "ior"}
        cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_box", "kd": "chk"},
                                               {"material_type": "MatteMaterial", "material_name": "m_cube", "kd": "cyl"}, patch_mat]
        cube["material_name"], box["material_name"] = "m_cube", "m_box"
        cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "m_patch", "obj_name": "patch_01",
                                               "instances": [{"world_pos": [33.0, -2.5, 0.0], "rotation_axis": [0.2, 1.0, 0.1], "rotation_angle": 20}]})
    elif which in ("direct_image_ewa", "path_image_trilinear"):
        from test_host import write_png_fixture as write_png
        rng = np.random.default_rng(4)
        yy, xx = np.mgrid[0:256, 0:256]
        img = np.stack([(xx ^ yy) & 255, (xx * 3 + yy) & 255, rng.integers(0, 256, size=(256, 256))], -1).astype(np.uint8)
        write_png(os.path.join(wd, "tex.png"), img, filters=[4])
        tri = which.endswith("trilinear")
        cfg["rgb_texture"] = [{"texture_name": "img", "texture_type": "ImageTexture", "filename": "tex.png", "do_trilinear": tri, "wrap": "clamp" if tri else "repeat",
                               "mapping": {"mapping": "uv", "su": 3.0, "sv": 2.0, "du": 0.25, "dv": 0.5} if tri else
                                          {"mapping": "uv", "su": 0.002, "sv": 0.002, "du": 0.3, "dv": 0.3}},
                              _const_rgb("half", [0.5, 0.5, 0.5]), {"texture_name": "img_half", "texture_type": "ScaleTexture", "t1": "img", "t2": "half"}]
        cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_box", "kd": "img"},
                                               {"material_type": "PlasticMaterial", "material_name": "m_cube", "kd": "img_half", "ks": "img"}]
        cube["material_name"], box["material_name"] = "m_cube", "m_box"
        # EWA (the default) as the reference has it: compute_differentials' `ty` (interaction.rs:234) makes dpdy - hence dstdy - as large as
        # the scene, so at unit texture scale lod lands past the last level and ewa() indexes out of bounds
        # (test_image_texture_ewa_panics_like_the_reference); and the ellipse's t offset is taken from st[0] (mipmap.rs:250), so off the
        # diagonal s = t no texel passes r2 < 1 and the lookup is 0 / 0. The case therefore shrinks the mapping (footprint < 1) and keeps
        # s = t; DirectLighting drops NaN samples at the film (integrator/mod.rs:105) where the path integrator would assert on beta.
        if not tri:
            cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3}
    elif which in ("path_bump_patch", "direct_bump_spheres"):
        # Material::bump (material/mod.rs:22-62): displacement texture at (u + du, v), (u, v + dv), (u, v); du / dv from the differentials
        cfg["float_texture"] = [{"texture_name": "wr", "texture_type": "WrinkledTexture", "octaves": 4, "omega": 0.5, **ROT, "scale": [2.0, 2.0, 2.0]},
                                {"texture_name": "amp", "texture_type": "BilerpTexture", "v00": 0.03, "v01": 0.03},
                                {"texture_name": "bumpy", "texture_type": "ScaleTexture", "t1": "wr", "t2": "amp"},
                                {"texture_name": "chk", "texture_type": "CheckerBoardTexture", "t1": "amp", "aamode": "none",
                                 "mapping": {"mapping": "uv", "su": 6.0, "sv": 6.0, "du": 0.0, "dv": 0.0}},
                                {"texture_name": "lift", "texture_type": "BilerpTexture", "v00": 0.2, "v01": 0.2}]
        if which == "path_bump_patch":
            # depth 3, not 5: a bump-mapped normal is a finite difference of the displacement (step 0.0005), and each further bounce off the
            # noise-bumped walls multiplies the rounding difference between device and oracle by ~100 (measured: 5e-14, 2e-10, 2e-8, 3e-6 of
            # the image maximum at depths 2..5) - chaos in the scene, not a difference in the algorithm
            cfg["Integrator"]["max_depth"] = 3
            _write_patch(wd)
            cfg["objs"] = cfg["objs"] + [{"filename": "patch.obj", "obj_name": "patch_01"}]
            cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_box", "bump_map": "bumpy"},
                                                   {"material_type": "PlasticMaterial", "material_name": "m_cube", "bump_map": "chk"},
                                                   {"material_type": "MetalMaterial", "material_name": "m_patch", "bump_map": "lift", "roughness": "amp"}]
            cube["material_name"], box["material_name"] = "m_cube", "m_box"
            cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "m_patch", "obj_name": "patch_01",
                                                   "instances": [{"world_pos": [33.0, -2.5, 0.0], "rotation_axis": [0.2, 1.0, 0.1], "rotation_angle": 20}]})
        else:
            cfg, root = scenes.cfg1(wd, xres=64, yres=64, nsamp=5)
            cfg["float_texture"] = [{"texture_name": "lift", "texture_type": "BilerpTexture", "v00": 0.2, "v01": 0.2},
                                    {"texture_name": "ramp", "texture_type": "BilerpTexture", "v00": 0.0, "v01": 0.5}]
            cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_s", "bump_map": "lift"},   # constant, but dndu != 0 on a sphere
                                                   {"material_type": "MirrorMaterial", "material_name": "m_mirror", "bump_map": "ramp"}]
            inst = cfg["Aggregate"]["primitives"][0]["instances"]
            cfg["Aggregate"]["primitives"] = [{"primitive_type": "sphere", "material_name": "m_s", "radius": 0.75, "instances": inst[::2]},
                                              {"primitive_type": "sphere", "material_name": "m_mirror", "radius": 0.75, "instances": inst[1::2]}]
    elif which == "direct_spheres":
        cfg, root = scenes.cfg1(wd, xres=64, yres=64, nsamp=5)
        cfg["rgb_texture"] = [_const_rgb("w", [0.9, 0.9, 0.9]), _const_rgb("k", [0.2, 0.1, 0.1]),
                              {"texture_name": "chk", "texture_type": "CheckerBoardTexture", "t1": "w", "t2": "k",
                               "mapping": {"mapping": "uv", "su": 8.0, "sv": 4.0, "du": 0.0, "dv": 0.0}}]
        cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_s", "kd": "chk"},
                                               {"material_type": "MirrorMaterial", "material_name": "m_mirror", "kr": "chk"}]
        inst = cfg["Aggregate"]["primitives"][0]["instances"]
        cfg["Aggregate"]["primitives"] = [{"primitive_type": "sphere", "material_name": "m_s", "radius": 0.75, "instances": inst[::2]},
                                          {"primitive_type": "sphere", "material_name": "m_mirror", "radius": 0.75, "instances": inst[1::2]}]
    return cfg, root


@pytest.mark.parametrize("which", ["path_checker_uv", "path_noise", "direct_mirror_patch", "debug_glass_patch", "direct_spheres", "direct_image_ewa",
                                   "path_image_trilinear", "path_bump_patch", "direct_bump_spheres"])
def test_textured_materials(which, workdir):
    """Texture graph evaluated per hit (texture/*.rs), with the camera ray differentials (camera.rs:582-628, scaled by 1 / sqrt(spp)),
    compute_differentials incl. its `ty` quirk (interaction.rs:234), and - DirectLighting / Debug - the differentials specular
    children inherit (integrator/mod.rs:183-201 with its factor 0.2, :238-292)."""
    cfg, root = _tex_case(which, workdir)
    sc = Scene.loads(cfg, root)
    assert sc.desc.n_textures > 0 and any(t >= 0 for m in sc.desc.materials[:sc.desc.n_materials] for t in list(m.tex) + [m.bump])
    ref, st_ref = O.render(sc, stats=True)
    assert ref[..., :3].max() > 0
    r = Renderer(sc, 0, RRT_F64)
    film, st = r.render(stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert st.camera_rays == st_ref.camera_rays
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    if which.endswith("spheres"):     # rays spawned on a sphere re-test it with c ~ +-1e-16 (test_sphere_primitives_render)
        assert (diff > 1e-9).mean() < 0.01, ((diff > 1e-9).mean(), diff.max())
    else:
        assert st.any_queries == st_ref.any_queries
        if not which.startswith("path"):      # (the wavefront never issues the path integrator's last, unshaded closest-hit query)
            assert st.closest_queries == st_ref.closest_queries
        assert diff.max() < 1e-9, (diff.max(), (diff > 1e-9).sum())
    r = Renderer(sc, 0, RRT_F32)
    f32 = r.render().astype(np.float64)
    r.close()
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    print(which, "f32: within 1e-4:", (d32 < 1e-4).mean(), "median", np.median(d32), "max", d32.max(), "mean rel", abs(f32[..., :3].mean() / ref[..., :3].mean() - 1))
    if which == "path_bump_patch":        # the same chaos from an fp32 rounding (6e-8) instead of an f64 one: per-pixel bar at 1e-3
        assert (d32 < 1e-3).mean() > 0.97, ((d32 < 1e-3).mean(), d32.max())
    elif not which.endswith("spheres"):   # fp32 spheres: parity in the mean only
        assert (d32 < 1e-4).mean() > 0.97 and np.median(d32) < 1e-5, ((d32 < 1e-4).mean(), d32.max())
    assert abs(f32[..., :3].mean() / ref[..., :3].mean() - 1) < (0.15 if which.endswith("spheres") else 0.02)


def test_image_texture_ewa_panics_like_the_reference(workdir):
    """A 64 x 64 image has one pyramid level (mipmap.rs:361 stops below 64), so every EWA lookup with a non-degenerate footprint asks
    for ewa(1) = pyramid[1]: index out of bounds in the reference; the trilinear path of the same texture renders."""
    from test_host import write_png_fixture as write_png
    rng = np.random.default_rng(9)
    write_png(os.path.join(workdir, "small.png"), rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8))
    for tri in (False, True):
        cfg, root = _cfg3_tilted(workdir)
        cfg["rgb_texture"] = [{"texture_name": "img", "texture_type": "ImageTexture", "filename": "small.png", "do_trilinear": tri}]
        cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "m_box", "kd": "img"}]
        cfg["Aggregate"]["primitives"][1]["material_name"] = "m_box"
        sc = Scene.loads(cfg, root)
        for prec in (RRT_F64, RRT_F32):
            r = Renderer(sc, 0, prec)
            if tri:
                film = r.render()
                assert film[..., :3].max() > 0
            else:
                with pytest.raises(RrtPanic, match="index out of bounds"):
                    r.render()
            r.close()
        if not tri:
            with pytest.raises(O.OracleError, match="out of bounds"):
                O.render(sc)


@pytest.mark.parametrize("which", ["stratified_gaussian_passes", "bands_and_frames_in_flight"])
def test_textured_scene_across_features(which, workdir):
    """Textures and ray differentials together with the other features of the path: the stratified sampler (scale_differentials takes
    1 / sqrt(xsamp * ysamp)), a wide film filter, several pool passes (the per-slot differential records are per pass), band
    partitions and frames in flight."""
    import torch
    cfg, root = _tex_case("path_checker_uv", workdir)
    if which == "stratified_gaussian_passes":
        cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 3, "ysamp": 3, "jitter": True, "dimension": 6}
        cfg["Film"]["Filter"] = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
    sc = Scene.loads(cfg, root)
    ref = O.render(sc)
    scale = np.abs(ref[..., :3]).max()
    if which == "stratified_gaussian_passes":
        for prec, tol in ((RRT_F64, 1e-9), (RRT_F32, 1e-4)):
            r = Renderer(sc, 0, prec)
            r.set_option("max_paths", 64 * 64 * 3)       # 8 samples per pixel -> 3 passes
            film = r.render().astype(np.float64)
            r.close()
            if prec == RRT_F64:
                np.testing.assert_allclose(film[..., 3], ref[..., 3], rtol=1e-12)
            else:   # fp32: a jittered sample whose |d| / r * 16 rounds across a filter-table bin moves one weight (6 of 4096 pixels here)
                wrel = np.abs(film[..., 3] - ref[..., 3]) / ref[..., 3]
                assert (wrel < 1e-6).mean() > 0.99 and wrel.max() < 1e-2, ((wrel < 1e-6).mean(), wrel.max())
            d = np.abs(film[..., :3] - ref[..., :3]).max(-1) / scale
            assert (d < tol).mean() > (0.97 if prec == RRT_F32 else 0.9999), (prec, (d < tol).mean(), d.max())
    else:
        hs = [Renderer(sc, 0, RRT_F64) for _ in range(2)]
        for h in hs:
            h.set_option("nonblocking_streams", 1)
        films = [torch.zeros((64, 64, 4), dtype=torch.float64, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        for k in range(2):
            hs[k].render_bands_begin(k, 2, films[k].data_ptr())
        for h in hs:
            h.render_end()
        torch.cuda.synchronize()
        film = (films[0] + films[1]).cpu().numpy()
        for h in hs:
            h.close()
        assert np.array_equal(film[..., 3], ref[..., 3])
        d = np.abs(film[..., :3] - ref[..., :3]).max(-1) / scale
        assert d.max() < 1e-9, d.max()


def test_unjittered_strata_on_filter_table_boundaries(workdir):
    """2 x 2 unjittered strata put every sample 0.75 px from a pixel centre; with radius 1.5 the filter-table index
    |d| * (1 / r) * 16 is exactly 8.0 (film.rs:100-112). The fp32 build's fast reciprocal (1 ulp low) made it 7.99..: weight sums off
    by up to 2.6 per pixel until 1 / radius came from the host (found by tools/fuzz_parity.py)."""
    cfg, root = _cfg3_tilted(workdir)
    cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 2, "jitter": False, "dimension": 8}
    cfg["Integrator"] = {"integrator_type": "Debug", "max_depth": 1}
    for filt in ({"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}, {"filter_type": "TriangleFilter", "radius": [1.5, 1.5]}):
        cfg["Film"]["Filter"] = filt
        sc = Scene.loads(cfg, root)
        ref = O.render(sc, flat=True)
        r = Renderer(sc, 0, RRT_F32)
        film = r.render().astype(np.float64)
        r.close()
        np.testing.assert_allclose(film[..., 3], ref[..., 3], rtol=1e-5)
        d = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
        assert (d < 1e-4).mean() > 0.99, ((d < 1e-4).mean(), d.max())


def test_halton_dimension_limit_panics_like_the_reference(workdir):
    """HaltonSampler::permutation_for_dimension panics at dimension 1000 (samplers/halton.rs:63-69). A Debug / DirectLighting tree
    over smooth glass (16 dimensions per vertex, two children per vertex) gets there at depth ~7; found by tools/fuzz_parity.py as a
    device read past the 1000-entry dimension table."""
    cfg, root = scenes.cfg1(workdir, xres=24, yres=24, nsamp=3)
    _with_material(cfg, "mat_t", TRANSMISSIVE["glass"])
    cfg["Aggregate"]["primitives"][0]["material_name"] = "mat_t"
    cfg["Integrator"] = {"integrator_type": "Debug", "max_depth": 11}
    sc = Scene.loads(cfg, root)
    with pytest.raises(O.OracleError, match="1000 dimensions"):
        O.render(sc)
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        with pytest.raises(RrtPanic, match="1000 dimensions"):
            r.render()
        r.close()
    # the path integrator: 8 dimensions per bounce at most, so only absurd depths get there
    cfg, root = scenes.cfg3(workdir, xres=16, yres=16, nsamp=3, max_depth=400)
    cfg["Integrator"]["rr_threshold"] = 0.0      # no Russian roulette: paths live until max_depth
    cfg["materials"] = cfg["materials"] + [{"material_type": "MatteMaterial", "material_name": "white", "kd": "w"}]
    cfg["rgb_texture"] = [_const_rgb("w", [0.99, 0.99, 0.99])]
    for prim in cfg["Aggregate"]["primitives"]:
        prim["material_name"] = "white"
    sc = Scene.loads(cfg, root)
    with pytest.raises(O.OracleError, match="1000 dimensions"):
        O.render(sc)
    r = Renderer(sc, 0, RRT_F32)
    with pytest.raises(RrtPanic, match="1000 dimensions"):
        r.render()
    r.close()


def test_stratified_dimension_counters_overflow_is_refused(workdir):
    """The device packs the stratified sampler's 1D / 2D dimension counters in 12 bits each (8 until round 4) beside the bounce count in a path's
    queue word (dmath.hpp db_pack). A deep Debug / DirectLighting tree over smooth glass that draws several hundred 2D samples per camera sample -
    refused at 255 by rounds 1-3 - renders and matches the oracle; one that draws more than 4 095 (hundreds of lights, each sampled at every vertex) is
    refused loudly (RRT_EUNSUP), never wrapped silently."""
    cfg, root = _cfg3_tilted(workdir)
    cfg["Sampler"] = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 1, "jitter": True, "dimension": 4}
    cfg["Integrator"] = {"integrator_type": "Debug", "max_depth": 10}
    one_set = list(cfg["lights"])
    cfg["lights"] = one_set * 8                 # Debug samples every light at every vertex: 2 x 8 + 2 two-dimensional draws each
    _with_material(cfg, "mat_t", TRANSMISSIVE["glass"])
    for prim in cfg["Aggregate"]["primitives"]:
        prim["material_name"] = "mat_t"
    sc = Scene.loads(cfg, root)
    ref = O.render(sc)
    r = Renderer(sc, 0, RRT_F64)
    film = r.render()                           # (rounds 1-3: RRT_EUNSUP "8-bit counters")
    r.close()
    assert np.abs(film[..., :3] - ref[..., :3]).max() <= 1e-9 * np.abs(ref[..., :3]).max()
    cfg["lights"] = one_set * 600               # 2 x 600 + 2 two-dimensional draws per vertex: four vertices overflow 12 bits
    sc = Scene.loads(cfg, root)
    r = Renderer(sc, 0, RRT_F64)
    with pytest.raises(RrtUnsupported, match="12-bit counters"):
        r.render()
    r.close()
    cfg["lights"] = one_set * 8
    cfg["Integrator"]["max_depth"] = 3          # a shallow tree stays within the counters and matches the oracle
    sc = Scene.loads(cfg, root)
    ref = O.render(sc)
    r = Renderer(sc, 0, RRT_F64)
    film = r.render()
    r.close()
    assert np.abs(film[..., :3] - ref[..., :3]).max() <= 1e-9 * np.abs(ref[..., :3]).max()


def test_edge_configurations_found_by_the_sweeps(workdir):
    """tools/fuzz_edges.py findings: (1) a box filter narrower than 0.5 leaves samples near a pixel border in no pixel at all
    (film.rs:93-99: p0 > p1), so only radius exactly 0.5 may take the closed-form film kernel; (2) DirectLighting with an empty light
    list recurses for ever only on a MISS (Q20): inside an enclosure it renders (black), it does not panic."""
    cfg, root = _cfg3_tilted(workdir)
    cfg["Film"]["Filter"] = {"filter_type": "BoxFilter", "radius": [0.2, 0.35]}
    sc = Scene.loads(cfg, root)
    ref = O.render(sc)
    assert ref[..., 3].min() < 3 * 4 and ref[..., 3].max() <= 3 * 4      # fewer than the 4 samples reach some pixels
    for prec, tol in ((RRT_F64, 1e-9), (RRT_F32, 1e-4)):
        r = Renderer(sc, 0, prec)
        film = r.render().astype(np.float64)
        r.close()
        assert np.array_equal(film[..., 3], ref[..., 3])
        d = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
        assert (d < tol).mean() > 0.99, (prec, d.max())
    cfg, root = _cfg3_tilted(workdir)
    cfg["lights"] = []
    cfg["Integrator"] = {"integrator_type": "DirectLighting", "max_depth": 3}
    sc = Scene.loads(cfg, root)
    ref = O.render(sc, flat=True)                      # every camera ray hits the enclosure: no miss, no recursion, no light
    assert not ref[..., :3].any()
    r = Renderer(sc, 0, RRT_F32)
    film = r.render()
    r.close()
    assert not film[..., :3].any() and np.array_equal(film[..., 3].astype(np.float64), ref[..., 3])


@pytest.mark.parametrize("prec", [RRT_F64, RRT_F32])
def test_trace_api_survives_garbage_rays(prec, hf_scene):
    """rrt_trace_closest / rrt_trace_any are fed by callers: zero / NaN / infinite components, t_max of 0, negative, NaN, and skip_prim
    indices outside the triangle array must neither fault nor hang, and must not disturb the sane rays of the same batch."""
    sc = hf_scene
    o, d, tmax, skip = _rays_for(sc, 2048, 5)
    dt = np.float32 if prec == RRT_F32 else np.float64
    o, d, tmax = o.astype(dt), d.astype(dt), tmax.astype(dt)
    r = Renderer(sc, 0, prec)
    clean = r.trace_closest(o, d, tmax, skip_prim=skip)
    clean_any = r.trace_any(o, d, np.full(len(o), 1.0 - 1e-4, dt), skip_prim=skip)
    o2, d2, t2, s2 = o.copy(), d.copy(), tmax.copy(), skip.copy()
    bad = np.arange(0, len(o), 7)
    d2[bad[0::6]] = 0.0
    d2[bad[1::6], 1] = np.nan
    o2[bad[2::6], 0] = np.inf
    t2[bad[3::6]] = np.array([0.0, -1.0, np.nan, np.inf], dt)[np.arange(len(bad[3::6])) % 4]
    s2[bad[4::6]] = 2 ** 31 - 1
    s2[bad[5::6]] = -12345
    good = np.ones(len(o), bool); good[bad] = False
    got = r.trace_closest(o2, d2, t2, skip_prim=s2)
    t_any = np.full(len(o), 1.0 - 1e-4, dt)
    t_any[bad[3::6]] = t2[bad[3::6]]
    got_any = r.trace_any(o2, d2, t_any, skip_prim=s2)
    r.close()
    assert np.array_equal(got["prim"][good], clean["prim"][good]) and np.array_equal(got["t"][good], clean["t"][good])
    assert np.array_equal(got_any[good], clean_any[good])
    assert (got["prim"][bad] >= -1).all() and (got["prim"][bad] < sc.desc.n_prim_order).all()


def test_create_rejects_inconsistent_descs(workdir):
    """rrt_create follows indices of a caller-owned rrt_scene_desc: each is range-checked up front (RRT_EINVAL), not found by a kernel."""
    from rs_ray_toy_amd import RrtError
    cfg, root = scenes.cfg2(workdir, xres=16, yres=16, nsamp=3)
    sc = Scene.loads(cfg, root)
    d = sc.desc
    def broken(setter, restore):
        setter()
        try:
            with pytest.raises(RrtError, match="scene desc"):
                Renderer(sc, 0, RRT_F32)
        finally:
            restore()
    m0 = d.prims[0].material
    broken(lambda: setattr(d.prims[0], "material", 10 ** 6), lambda: setattr(d.prims[0], "material", m0))
    v0 = d.tris[0].v[0]
    broken(lambda: d.tris[0].v.__setitem__(0, d.n_positions), lambda: d.tris[0].v.__setitem__(0, v0))
    o0 = d.prim_order[0]
    broken(lambda: d.prim_order.__setitem__(0, d.n_prims), lambda: d.prim_order.__setitem__(0, o0))
    leaf = next(i for i in range(d.n_bvh_nodes) if d.bvh_nodes[i].n_primitives > 0)
    n0 = d.bvh_nodes[leaf].offset
    broken(lambda: setattr(d.bvh_nodes[leaf], "offset", d.n_prim_order), lambda: setattr(d.bvh_nodes[leaf], "offset", n0))
    r = Renderer(sc, 0, RRT_F32)        # restored: creates and renders
    assert r.render()[..., 3].max() > 0
    # the batch entry points validate their ranges the same way (the sample arrays are caller-sized from them)
    with pytest.raises(RrtError, match="rect outside the film"):
        r.camera_samples((0, 0, 17, 16), 0, 1)
    with pytest.raises(RrtError, match="sample range"):
        r.camera_samples((0, 0, 4, 4), 0, 4)               # samples_per_pixel is 3
    with pytest.raises(RrtError, match="rect outside the film"):
        r.render(rect=(0, 0, 16, 17))
    assert r.camera_samples((0, 0, 4, 4), 0, 3)[2].shape == (48,)
    r.close()
