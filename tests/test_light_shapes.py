"""The device's direct-lighting code (dkernels.hpp: light_sample_li, estimate_direct_light, sample_light_discrete, the `v * n_lights` choice; host/scene_loader.cpp
make_light, host/scene_flatten.cpp's Light<R> records and light cdf, host/shadow_lists.cpp's sources) on hand-built light tables (tests/light_shapes.py),
against the f64 oracle.

Every other GPU test lights its scene with 1 to 4 point, distant or unit sphere lights. The table of light_shapes.py walks the code through what that
never reaches: triangle emitters (with and without vertex normals, with `vn` lines and no normal indices, the last face of a mesh, near and far from the
origin, of zero area), tables of 2 to 17 lights under both light choosers, every early out of estimate_direct, sphere emitters that are scaled and rotated,
clipped, of negative radius, around the geometry, below it and far away, and tables that mix all of it. light_shapes.py says which case reaches what,
and the oracle's light census (oracle_lib.light_census) proves per case that the frame does reach it: the proof is counted on the reference side.

CPU tests (the host loader and the oracle alone):
  test_case_loads_and_reaches_its_branches      the loaded rrt_light records hold the table's constants; the oracle's outcome is the recorded one; a
                                                frame is finite and lit; the census has what the case's tags ask and every light index was chosen
  test_loader_refuses_what_the_reference_refuses  tri_num out of range, an unknown obj_name, a missing light_shape, an unknown shape_type
  test_pairs_are_one_light                      a clipped sphere emitter is the full one: bit-equal oracle frames and counters
  test_normals_turn_the_emitter                 tri_normals_flipped against tri_plain: more than a tenth of the lit pixels differ
  test_closed_forms                             through oracle_lib.light_sample: the point light's inverse square, the distant light's tester, the sphere
                                                emitter's point on the sphere and its back face, the triangle emitter's point off the triangle (Q19) and
                                                its normal, and the pdf without an area in it
GPU tests, a 64 x 64 film each:
  test_f64_frame_matches_oracle                 weights and the three counters equal, colour within 1e-9 of the brightest pixel, black where the oracle is
  test_fp32_frame_close_to_oracle               test_gpu_parity.py's fp32 bar
  test_light_choice_in_fp32                     the count cases under Path and DirectLighting `one`: the bar, less twice the share of the oracle's choices
                                                that lie on a cdf boundary
  test_candidate_lists_change_nothing           the shadow candidate lists on and off on the terrain: 15 / 16 / 17 sources, duplicates, the scaled and
                                                the inside-out sphere emitter, sphere emitters beside a triangle emitter
  test_passes_partition_the_mixed_table         rrt_render_passes, one pass per light of mixed_all_four
"""
import copy

import numpy as np
import pytest

import light_shapes as LS
import oracle_lib as O
import passes_reference as PR
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, RRT_SKIP_MIS_BSDF_RAY, Renderer, RrtPanic, Scene

ALL = sorted(LS.CASES)
F64_ONLY = [k for k in ALL if LS.CASES[k].fp32.startswith("f64_only")]
# at most three, and never a plain, mixed, count or triangle-normal case
assert len(F64_ONLY) <= 3 and not any(k.startswith(("point-", "sphere_plain", "tri_plain", "mixed_", "count_", "tri_normals", "two_equal")) for k in F64_ONLY)
COUNTS = [k for k in ALL if k.startswith("count_") and LS.CASES[k].integrator in (LS.PATH, LS.ONE)]

_scenes, _refs, _f32 = {}, {}, {}


def _flags(name):
    # under an area light the oracle traces estimate_direct's BSDF-sampled ray, which can only add 0 and which the device leaves out (DESIGN.md section 3,
    # dead work 1): with the flag the oracle leaves it out too and the query counters compare
    return RRT_SKIP_MIS_BSDF_RAY if LS.has_area_light(name) else 0


def _scene(name, workdir):
    if name not in _scenes: _scenes[name] = Scene.loads(*LS.scene(workdir, name), flags=_flags(name))
    return _scenes[name]


def _ref(name, workdir):
    """(frame, (camera rays, closest queries the device issues, any queries), light census) of the oracle for the case, rendered once and never written to;
    (None, panic message, census) where the oracle panics"""
    if name not in _refs:
        sc = _scene(name, workdir)
        O.bsdf_census(); O.light_census()
        try:
            film, st = O.render(sc, stats=True)
            film.setflags(write=False)
            # the device leaves out the path integrator's closest-hit query at bounces == max_depth (dead work 2; test_material_shapes.py)
            _refs[name] = (film, (int(st.camera_rays), int(st.closest_queries) - O.bsdf_census()["path_last_query"], int(st.any_queries)), O.light_census())
        except O.OracleError as e:
            _refs[name] = (None, str(e), O.light_census())
    return _refs[name]


def _lit(film):
    return film[..., :3].max(-1) > 0


def _outcome(film):
    """What the oracle did with a case, in light_shapes.py's words"""
    if film is None: return "panic"
    if not film[..., :3].any(): return "black"
    return "frame"


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_case_loads_and_reaches_its_branches(name, workdir):
    c = LS.CASES[name]
    sc = _scene(name, workdir)
    want = LS.expected_constants(c)
    assert sc.desc.n_lights == len(want)
    for i, w in enumerate(want):
        l = sc.desc.lights[i]
        assert l.type == w["type"] and list(l.spectrum) == w["spectrum"], (i, l.type, list(l.spectrum))
        if "p_light" in w: assert list(l.p_light) == w["p_light"]
        if "shape_type" in w: assert l.shape_type == w["shape_type"]
        if "w_light" in w:
            assert np.allclose(list(l.w_light), w["w_light"], rtol=0, atol=4e-16), (list(l.w_light), w["w_light"])
            assert l.world_radius > 0
        if "area" in w: assert abs(l.area - w["area"]) <= 1e-14 * abs(w["area"]), (l.area, w["area"])
    film, counters, census = _ref(name, workdir)
    # a NaN sample the film drops (integrator/mod.rs:105) leaves a frame; no case of the table has one, and "drops" would be recorded as such
    assert _outcome(film) == c.oracle, (_outcome(film), counters)
    if film is None: return
    print(f"{name}: lit {_lit(film).mean():.4f}, brightest {film[..., :3].max():.4f}, counters {counters}, census { {k: v for k, v in census.items() if v and k != 'chosen'} }, "
          f"chosen {census['chosen'][:len(c.lights)]}")
    assert np.all(np.isfinite(film)) and np.all(film[..., 3] > 0)
    if c.oracle == "frame": assert _lit(film).mean() > 0.01
    assert not LS.census_problems(c, census), (LS.census_problems(c, census), census)
    if name.startswith("distant_grazing"):      # within half a degree of the floor's plane, above it
        up = LS._rotate((0.0, 1.0, 0.0), LS.FLOOR_TILT["rotation_axis"], LS.FLOOR_TILT["rotation_angle"])
        s = float(np.dot(up, list(sc.desc.lights[0].w_light)))
        assert 0 < s < np.sin(np.radians(0.5)), s
    if name.startswith("sphere_swallows_floor"): assert census["emitter_backface"] > 500


@pytest.mark.parametrize("what", ["tri_num", "obj_name", "light_shape", "shape_type"])
def test_loader_refuses_what_the_reference_refuses(what, workdir):
    """make_light's panics (renderprocess.rs:968-1095), raised by the loader before anything is built"""
    cfg, root = LS.scene(workdir, "tri_last_of_mesh-path")
    cfg = copy.deepcopy(cfg)
    shape = cfg["lights"][0]["light_shape"]
    if what == "tri_num": shape["tri_num"] = 12; msg = r"renderprocess\.rs:1090 mesh\[tri_num\] out of bounds"      # one past the last face of the mesh of 12
    elif what == "obj_name": shape["obj_name"] = "nobody"; msg = r"renderprocess\.rs:1087 triangle_mesh\[\"nobody\"\] missing"
    elif what == "light_shape": del cfg["lights"][0]["light_shape"]; msg = r"renderprocess\.rs:1013 Shape Required for a DiffuseLight"
    else: shape["shape_type"] = "disk"; msg = r"renderprocess\.rs:1095 Failed to parse a Shape"
    with pytest.raises(RrtPanic, match=msg):
        Scene.loads(cfg, root)
    shape_ok = LS.scene(workdir, "tri_last_of_mesh-path")
    assert Scene.loads(*shape_ok).desc.n_lights == 1      # ... and the unedited document loads


PAIRS = sorted((k, c.pair) for k, c in LS.CASES.items() if c.pair)


@pytest.mark.parametrize("name,partner", PAIRS, ids=[a for a, _ in PAIRS])
def test_pairs_are_one_light(name, partner, workdir):
    (a, ca, na), (b, cb, nb) = _ref(name, workdir), _ref(partner, workdir)
    assert _scene(name, workdir).desc.lights[0].area != _scene(partner, workdir).desc.lights[0].area      # two spellings ...
    assert np.array_equal(a, b) and ca == cb and na == nb                                                   # ... of one light


@pytest.mark.parametrize("integ", [LS.PATH, LS.ALL, LS.ONE])
def test_normals_turn_the_emitter(integ, workdir):
    """faceforward (triangle.rs:405-408) against the file's normals turns the emitter round for the samples whose `barycentrics` give ns the other sign: the
    frames with and without the normals differ, so a device that dropped tri_has_n cannot pass"""
    plain, flipped, agree = (_ref(f"{n}-{integ}", workdir)[0][..., :3] for n in ("tri_plain", "tri_normals_flipped", "tri_normals_agree"))
    lit = _lit(plain) | _lit(flipped)
    for other, tag in ((flipped, "flipped"), (agree, "agree")):
        scale = max(plain.max(), other.max())
        differ = int((np.abs(plain - other).max(-1) > 1e-6 * scale)[lit].sum())
        print(f"tri_plain against tri_normals_{tag} ({integ}): {differ} of {int(lit.sum())} lit pixels differ")
        assert differ > int(lit.sum()) // 10, (tag, differ)
    if integ == LS.PATH:      # the first normal of the mesh three times is not the three normals
        assert not np.array_equal(_ref("tri_normals_mode2-path", workdir)[0], _ref("tri_normals_flipped-path", workdir)[0])


def _affine(sc, light):
    sp = sc.desc.spheres[sc.desc.lights[light].shape]
    x = sc.desc.xforms[sp.xform]
    return np.array(list(x.m)).reshape(4, 4), np.array(list(x.m_inv)).reshape(4, 4), sp.radius


REFS = [np.array(p) for p in ((35.0, -19.0, 0.0), (20.0, 3.0, -7.5), (70.0, 11.0, 30.0), (-3.0, -2.0, 1.0), (33.0, 1.5, 0.5))]
US = [(0.07, 0.31), (0.5, 0.5), (0.93, 0.77), (0.33, 0.02), (0.61, 0.95), (0.18, 0.64)]


def test_closed_forms(workdir):
    # point light (point.rs:55-77): li = I / d^2, the tester ends at the origin whatever world_pos says (Q17)
    sc = _scene("point-path", workdir)
    for ref in REFS:
        e = O.light_sample(sc, 0, ref)
        assert np.allclose(e["li"] * np.dot(ref, ref), 60000.0, rtol=4e-16, atol=0) and e["pdf"] == 1.0
        assert np.array_equal(e["p1"], [0.0, 0.0, 0.0]) and np.allclose(e["wi"], -ref / np.linalg.norm(ref), rtol=0, atol=2e-16)
    # distant light (distant.rs:67-92): wi = w_light, the tester ends 2 world_radius along it
    sc = _scene("distant_scaled_rotated-path", workdir)
    L = sc.desc.lights[0]
    w = np.array(list(L.w_light))
    for ref in REFS:
        e = O.light_sample(sc, 0, ref)
        assert np.array_equal(e["wi"], w) and e["pdf"] == 1.0 and np.array_equal(e["li"], list(L.spectrum))
        assert np.allclose(e["p1"] - ref, 2.0 * L.world_radius * w, rtol=0, atol=1e-13 * L.world_radius)
    # sphere emitters: the sampled point is on the sphere in object space, and the emitter is black exactly where it shows its back
    for name in ("sphere_plain-path", "sphere_scaled_rotated-path", "sphere_clipped-path", "sphere_negative_radius-path", "sphere_swallows_floor-path", "sphere_far_tiny-path"):
        sc = _scene(name, workdir)
        m, mi, radius = _affine(sc, 0)
        seen = set()
        for ref in REFS:
            outside = np.linalg.norm((mi @ np.append(ref, 1.0))[:3]) > abs(radius)
            for u0, u1 in US:
                e = O.light_sample(sc, 0, ref, u0, u1)
                p_obj = (mi @ np.append(e["p1"], 1.0))[:3]
                tol = 1e-12 * max(1.0, np.abs(e["p1"]).max())      # (what M^-1 M costs at the emitter's distance from the origin)
                assert abs(np.linalg.norm(p_obj) - abs(radius)) <= tol, (name, np.linalg.norm(p_obj))
                back = np.dot(e["n1"], -e["wi"]) <= 0
                assert (not e["li"].any()) == bool(back), (name, ref, u0, u1)
                if not back: assert np.array_equal(e["li"], list(sc.desc.lights[0].spectrum))
                d2 = np.dot(e["p1"] - ref, e["p1"] - ref)
                assert np.isclose(e["pdf"], d2 / abs(np.dot(-e["wi"], e["n1"])), rtol=1e-12, atol=0)      # no area in it (Shape::sample_ref shape/mod.rs:33-48)
                if outside: seen.add(bool(back))
        if name != "sphere_far_tiny-path": assert seen == {True, False}, name      # (a ten-thousandth of a degree wide: one face from every REFS)
    # ... a clipped sphere samples what the full one samples
    for ref in REFS:
        for u0, u1 in US:
            a, b = O.light_sample(_scene("sphere_plain-path", workdir), 0, ref, u0, u1), O.light_sample(_scene("sphere_clipped-path", workdir), 0, ref, u0, u1)
            assert all(np.array_equal(a[k], b[k]) for k in a)
    # ... and from inside the emitter every sample shows its back
    sc = _scene("sphere_swallows_floor-path", workdir)
    assert not any(O.light_sample(sc, 0, (35.0, -19.0, 0.0), u0, u1)["li"].any() for u0, u1 in US)
    # triangle emitters (triangle.rs:393-418, Q19): p = sum b_k q_k with |b| = 1 - on an ellipsoid around the origin, not on the triangle
    flips = set()
    for name in ("tri_plain-path", "tri_normals_flipped-path", "tri_near_origin-path", "tri_far_from_origin-path", "tri_last_of_mesh-path"):
        sc = _scene(name, workdir)
        q = np.array(LS.emitter_vertices(name, 0)).T      # columns q0 q1 q2
        ng = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
        ng /= np.linalg.norm(ng)
        off_triangle = 0
        for ref in REFS:
            for u0, u1 in US:
                e = O.light_sample(sc, 0, ref, u0, u1)
                b = np.linalg.solve(q, e["p1"])
                assert abs(np.linalg.norm(b) - 1.0) < 1e-14 * np.linalg.cond(q) + 1e-12, (name, b, np.linalg.norm(b))      # (the solve costs cond(q) ulp)
                off_triangle += bool(b.min() < -1e-3 or abs(b.sum() - 1.0) > 1e-3)
                assert np.allclose(np.abs(e["n1"]), np.abs(ng), rtol=0, atol=1e-14)
                back = np.dot(e["n1"], -e["wi"]) <= 0
                assert (not e["li"].any()) == bool(back)
                d2 = np.dot(e["p1"] - ref, e["p1"] - ref)
                assert np.isclose(e["pdf"], d2 / abs(np.dot(-e["wi"], e["n1"])), rtol=1e-12, atol=0)      # no area in it
                if name == "tri_plain-path":
                    assert np.allclose(e["n1"], ng, rtol=0, atol=1e-14)
                    f = O.light_sample(_scene("tri_normals_flipped-path", workdir), 0, ref, u0, u1)
                    assert np.array_equal(f["p1"], e["p1"])
                    # the file's normals are -TRI_VN: ns = -sum b_k vn_k, and faceforward turns n exactly when ns and n disagree
                    turned = sum(b[k] * np.dot(LS.TRI_VN[k] / np.linalg.norm(LS.TRI_VN[k]), ng) for k in range(3)) > 0
                    assert np.array_equal(f["n1"], -e["n1"] if turned else e["n1"]), (u0, u1)
                    flips.add(bool(turned))
        assert off_triangle == len(REFS) * len(US), (name, off_triangle)
    assert flips == {True, False}
    # zero area: pdf 0 and black, not NaN
    e = O.light_sample(_scene("tri_degenerate-path", workdir), 0, REFS[0], 0.3, 0.6)
    assert e["pdf"] == 0.0 and not e["li"].any()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

def _counters(st):
    return (st.camera_rays, st.closest_queries, st.any_queries)


def _render_f32(name, workdir):
    """(frame as f64, counters) of the fp32 device for the case, rendered once"""
    if name not in _f32:
        r = Renderer(_scene(name, workdir), 0, RRT_F32)
        film, st = r.render(stats=True)
        r.close()
        film = film.astype(np.float64)
        film.setflags(write=False)
        _f32[name] = (film, _counters(st))
    return _f32[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_f64_frame_matches_oracle(name, workdir):
    ref, counters, _ = _ref(name, workdir)
    r = Renderer(_scene(name, workdir), 0, RRT_F64)
    if LS.CASES[name].oracle == "panic":
        with pytest.raises(RrtPanic):
            r.render()
        r.close()
        return
    film, st = r.render(stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert _counters(st) == counters
    assert np.all(np.isfinite(film))
    if LS.CASES[name].oracle == "drops": assert np.array_equal(_lit(film), _lit(ref))
    scale = np.abs(ref[..., :3]).max()
    if scale == 0:      # every light sample of the frame takes an early out
        assert LS.CASES[name].oracle == "black" and not film[..., :3].any()
        return
    assert not film[..., :3][~_lit(ref)].any()      # exactly black where the oracle is
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / scale
    print(f"{name}: f64 max {diff.max():.3e}")
    assert diff.max() < 1e-9, (diff.max(), int((diff > 1e-9).sum()))


def _fp32_bar(name, f32, ref, allowance=0.0):
    """test_gpu_parity.py's fp32 bar: more than 99 % of the pixels within 1e-4 of the brightest pixel (less `allowance`), the median below 1e-5"""
    scale = np.abs(ref[..., :3]).max()
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / scale
    print(f"{name}: f32 within 1e-4: {(d32 < 1e-4).mean():.4f} ({int((d32 >= 1e-4).sum())} pixels beyond), median {np.median(d32):.3e}, max {d32.max():.3e}")
    if name not in F64_ONLY: O.fp32_bar(d32, allowance)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_fp32_frame_close_to_oracle(name, workdir):
    """The cases the table marks f64-only (F64_ONLY; light_shapes.py argues each beside the case) keep everything here but the bar on the colour."""
    ref, _, _ = _ref(name, workdir)
    if LS.CASES[name].oracle == "panic":
        r = Renderer(_scene(name, workdir), 0, RRT_F32)
        with pytest.raises(RrtPanic):
            r.render()
        r.close()
        return
    f32, _ = _render_f32(name, workdir)
    assert np.array_equal(f32[..., 3], ref[..., 3])
    assert np.all(np.isfinite(f32))
    if not ref[..., :3].any():
        assert not f32[..., :3].any()
        return
    _fp32_bar(name, f32, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNTS)
def test_light_choice_in_fp32(name, workdir):
    """sample_light_discrete compares an fp32 u with the f64 cdf cast to fp32, DirectLighting `one` multiplies u by n in fp32: a sample within an fp32 ulp of a
    cdf entry may choose the neighbouring light, and its pixel then leaves the bar. How many samples that is, is counted by the oracle (choice_boundary: u
    within 2^-23 of an inner cdf entry); twice that share of the pixels is allowed beyond the bar's own 1 %. The counts are in
    profiles/light_shapes_gpu_tests.txt: none of the table's frames has such a sample, so the allowance is 0 and the bar is the bar."""
    ref, counters, census = _ref(name, workdir)
    choices = census["choose_distrib"] + census["choose_plain"]
    share = census["choice_boundary"] / choices
    f32, got = _render_f32(name, workdir)
    print(f"{name}: {census['choice_boundary']} of {choices} light choices of the oracle lie within 2^-23 of a cdf entry, {census['choice_clamped']} were clamped: "
          f"allowance {2.0 * share:.2e} of the pixels")
    assert got[0] == counters[0] and got[2] == counters[2]      # (a choice that went to the neighbour would still trace its shadow ray: the colour is what tells)
    assert np.array_equal(f32[..., 3], ref[..., 3]) and np.all(np.isfinite(f32))
    _fp32_bar(name, f32, ref, allowance=2.0 * share)


# name -> the candidate lists exist (host/shadow_lists.cpp: up to 15 distinct sources, every one a point, distant or sphere light)
LISTS = {"count_15-path": True, "count_16-path": False, "count_17-path": False, "count_15-all": True, "count_17-one": False, "two_equal_points-path": True,
         "sphere_scaled_rotated-path": True, "sphere_negative_radius-path": True, "spheres_plus_triangle-path": False}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LISTS))
def test_candidate_lists_change_nothing(name, workdir):
    """test_gpu_parity.py::test_shadow_candidate_lists_change_nothing on the table's lights over the terrain: the lists on and off give the same bits and the
    same counters; rrt_render_stats::list_launches says whether the handle has lists at all - it has for 15 sources and for duplicates of one, it has none
    for 16 and 17 (shadow_lists.cpp:61) nor beside a triangle emitter (shadow_lists.cpp:57)."""
    sc = Scene.loads(*LS.scene(workdir, name, carrier="field"), flags=RRT_FIXED_BVH | _flags(name))
    r = Renderer(sc, 0, RRT_F32)
    a, st_a = r.render(stats=True)
    r.set_option("shadow_lists", 0)
    b, st_b = r.render(stats=True)
    r.close()
    print(f"{name}: {st_a.list_launches} of {st_a.any_launches} any-hit launches by the lists, {st_a.any_queries} shadow rays")
    assert st_a.any_launches > 0 and st_a.any_queries > 500 and st_b.list_launches == 0
    assert st_a.list_launches == (st_a.any_launches if LISTS[name] else 0), (st_a.list_launches, st_a.any_launches)
    assert _counters(st_a) == _counters(st_b)
    assert np.array_equal(a, b) and a[..., :3].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_passes_partition_the_mixed_table(prec, workdir):
    """rrt_render_passes with one pass per light of mixed_all_four (point, distant, sphere, triangle): the passes sum to the frame within
    test_passes.py::test_partitions_sum_to_the_frame's bound, each holds the frame's weights, and in f64 each is the oracle's frame of the scene with the
    other lights black (tests/passes_reference.py)."""
    name = "mixed_all_four-path"
    cfg, root = LS.scene(workdir, name)
    passes = [(1 << k, 0, 0) for k in range(4)]
    r = Renderer(_scene(name, workdir), 0, prec)
    film, films = r.render_passes(passes)
    plain = r.render()
    r.close()
    assert np.array_equal(film, plain) and film[..., :3].min() >= 0
    n = (LS.NSAMP - 1) * LS.DEPTH
    bound = (2 * n + 8) * float(np.finfo(film.dtype).eps) * film[..., :3].astype(np.float64)
    total = sum(f[..., :3].astype(np.float64) for f in films)
    over = np.abs(total - film[..., :3].astype(np.float64)) - bound
    used = np.abs(total - film[..., :3].astype(np.float64))[bound > 0] / bound[bound > 0]
    print(f"mixed_all_four {film.dtype}: the four light passes sum to the frame; at most {used.max():.3f} of the bound is used (bound up to {bound.max():.3e})")
    assert over.max() <= 0, over.max()
    top = np.abs(_ref(name, workdir)[0][..., :3]).max()
    for k, f in enumerate(films):
        assert np.array_equal(f[..., 3], film[..., 3]) and f[..., :3].max() > 0
        if prec == RRT_F64:
            # passes_reference.py's light identity (a black spectrum only skips the shadow ray) on this scene, loaded as the case is: pass_frame() itself
            # loads with RRT_FIXED_BVH, which is another tree and, by Q26, another frame
            ref = O.render(Scene.loads(PR.edited(cfg, [1.0 if j == k else 0.0 for j in range(4)]), root, flags=_flags(name)))
            diff = np.abs(f[..., :3] - ref[..., :3]).max() / top
            print(f"mixed_all_four: pass of light {k} against the oracle, max {diff:.3e}")
            assert diff < 1e-9, (k, diff)
