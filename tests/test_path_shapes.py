"""The device's integrator loops and the host code that drives them bounce by bounce (rrt_impl.hpp run_pass and dkernels.hpp: k_shade_path under the
`for (b < max_depth)` loop with its queue swap, its two alternating shadow queues and the horizon cull; the k_shade_nee / k_shade_specular chain; k_direct_tree's
explicit stack) on hand-built path tables (tests/path_shapes.py), against the f64 oracle.

Every other Path test runs at max_depth 2 to 8 under rr_threshold 1 or 0, and at max_depth 5 - the depth of most of them - what Russian roulette decides cannot
reach the film; every other DirectLighting / Debug test runs at depth 1, 3, 5, 8 or 22. The table of path_shapes.py walks max_depth from 0 to 64, rr_threshold from
-1 to 1e9 over walls that put q on its floor, end nearly every path and separate the largest component from the luminance, glass that moves eta_scale both ways,
vertices that draw differently, and the recursive integrators across the depths 2 | 3 and 16 | 17 | 18 on the queue chain and on the tree. path_shapes.py says
which case reaches what, and the oracle's path census (oracle_lib.path_census) proves per case that the frame does reach it: the proof is counted on the
reference side.

CPU tests (the host loader and the oracle alone):
  test_case_loads_and_reaches_its_states        the loaded integrator and sampler are the table's; the oracle's outcome is the recorded one; the census has
                                                what the case's tags ask; a Path frame's ends by cause sum to the paths started
  test_closed_forms_*                           depth 0 is black with the depth-5 frame's weights; rr_threshold 0 and 1 are one frame at max_depth 5 and two at 6;
                                                -1 is 0; 1e9 draws at every vertex with bounces > 3; DirectLighting and Debug are one frame at max_depth 0, 1, 2
                                                and another at 3; 64 bounces draw 5 + 7 x 64 dimensions
  test_refusals_on_the_oracle                   the reference refuses what the table says it refuses, and renders what only the device refuses
  test_roulette_ties_are_counted                the census's proximity counter on path_shapes.NEAR_CASE, a frame whose roulette tests compare 1 with 1
  test_f64_only_cases_are_argued                what the table says of its f64-only cases, on the oracle's two evaluation orders
GPU tests, a 64 x 64 film each:
  test_f64_frame_matches_oracle                 weights, camera rays, closest-hit and any-hit queries equal, colour within 1e-9 of the brightest pixel
  test_refusals_on_the_device                   the error the table records
  test_fp32_frame_close_to_oracle               test_material_shapes.py's fp32 bar (oracle_lib.fp32_bar), less twice the share of the pixels whose sample the
                                                oracle counts as a roulette decision within 2^-20 of flipping
  test_overlap_shadow_changes_no_bit            the two alternating shadow queues on the second stream against one queue on the main stream
  test_shortcuts_change_no_bit                  the defaults against test_frame_shapes.INVARIANT_OPTIONS all off together
  test_horizon_cull_meets_the_depth_guard       the terrain cases: the horizon tables on and off; none of a max_depth 1 frame's rays is answered by them
"""
import time

import numpy as np
import pytest

import oracle_lib as O
import path_shapes as PS
import rs_ray_toy_amd as RRT
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, Scene
from test_frame_shapes import INVARIANT_OPTIONS

ALL = sorted(PS.CASES)
F64_ONLY = [k for k in ALL if PS.CASES[k].fp32.startswith("f64_only")]
# at most three, none at max_depth <= 6, none a DirectLighting or Debug case at depth <= 4
assert len(F64_ONLY) <= 3 and not any(PS.CASES[k].max_depth <= (6 if PS.CASES[k].integrator == PS.PATH else 4) for k in F64_ONLY)
INVARIANT = [f"depth{d}-walls" for d in (1, 2, 3, 4, 6, 9)] + PS.find("depth", carrier="field")
INTEGRATOR_TYPE = {PS.PATH: 0, PS.ALL: 1, PS.ONE: 1, PS.DEBUG: 2}      # RRT_INT_* of include/rrt.h

_scenes, _refs, _f32 = {}, {}, {}


def _scene(name, workdir):
    if name not in _scenes: _scenes[name] = Scene.loads(*PS.scene(workdir, name))
    return _scenes[name]


def _ref(name, workdir):
    """(frame, (camera rays, closest queries the device issues, any queries), path census, seconds) of the oracle for the case, rendered once and never
    written to"""
    if name not in _refs:
        sc = _scene(name, workdir)
        O.bsdf_census(); O.path_census()
        t0 = time.perf_counter()
        film, st = O.render(sc, PS.CASES[name].frame["rect"], stats=True)
        dt = time.perf_counter() - t0
        film.setflags(write=False)
        # the device leaves out the path integrator's closest-hit query at bounces == max_depth (dead work 2; test_material_shapes.py)
        _refs[name] = (film, (int(st.camera_rays), int(st.closest_queries) - O.bsdf_census()["path_last_query"], int(st.any_queries)), O.path_census(), dt)
    return _refs[name]


def _outcome(film):
    return "frame" if film[..., :3].any() else "black"


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_case_loads_and_reaches_its_states(name, workdir):
    c = PS.CASES[name]
    sc = _scene(name, workdir)
    integ = sc.desc.integrator
    assert integ.type == INTEGRATOR_TYPE[c.integrator] and integ.max_depth == c.max_depth
    if c.integrator == PS.PATH: assert integ.rr_threshold == (1.0 if c.rr is None else c.rr)
    assert sc.desc.sampler.type == (1 if c.frame["sampler"] == "stratified" else 0)      # RRT_SAMPLER_*
    film, counters, census, dt = _ref(name, workdir)
    flat = {k: v for k, v in census.items() if v and k not in ("ends", "li_depth")}
    print(f"{name}: oracle {dt:.2f} s, lit {(film[..., :3].max(-1) > 0).mean():.4f}, brightest {film[..., :3].max():.4f}, counters {counters}, census {flat}, "
          f"ends { {k: {b: v for b, v in enumerate(h) if v} for k, h in census['ends'].items() if any(h)} }, li { {d: v for d, v in enumerate(census['li_depth']) if v} }")
    assert _outcome(film) == c.oracle
    assert np.all(np.isfinite(film)) and film[..., 3].max() > 0
    x0, y0, x1, y1 = c.frame["rect"] or (0, 0, PS.XRES, PS.YRES)
    assert np.all(film[y0:y1, x0:x1, 3] > 0) and film[..., 3].sum() == film[y0:y1, x0:x1, 3].sum()
    if c.oracle == "frame": assert (film[..., :3].max(-1) > 0).mean() > 0.01
    assert not PS.census_problems(c, census), (PS.census_problems(c, census), flat)
    # no roulette decision of the table's frames is a tie an fp32 rounding could flip (path_shapes.NEAR_CASE is one that has them)
    assert census["rr_test_near"] == 0 and census["rr_draw_near"] == 0
    if c.integrator == PS.PATH:      # ends by cause sum to the paths started, and every path is a camera ray
        assert sum(census["end_" + k] for k in O.PATH_ENDS) == census["started"] == counters[0]
        assert all(sum(census["ends"][k]) == census["end_" + k] for k in O.PATH_ENDS)
    else:
        assert census["li_depth"][1] == counters[0] and sum(census["li_depth"]) == census["li_calls"] == census["li_depth"][1] + census["reflect_taken"] + census["transmit_taken"]


def test_roulette_ties_are_counted(workdir):
    """path_shapes.NEAR_CASE: with light_shapes.py's Plastic on the walls a tenth of a frame's roulette tests compare 1 +- 1e-16 with the threshold 1, and the
    census says so - the counter test_fp32_frame_close_to_oracle takes its allowance from"""
    O.path_census()
    O.render(Scene.loads(*PS.scene(workdir, PS.NEAR_CASE)))
    n = O.path_census()
    print(f"near case: {n['rr_test_near']} of {n['rr_tests']} roulette tests within 2^-20 of the threshold")
    assert not PS.census_problems(PS.NEAR_CASE, n) and n["rr_test_near"] > n["rr_tests"] // 20


@pytest.mark.parametrize("name", F64_ONLY)
def test_f64_only_cases_are_argued(name, workdir):
    """What path_shapes.py says of the cases it makes no fp32 claim for, on the oracle alone: its two f64 evaluation orders, which differ by roundings of 2^-53,
    are further apart than 1e-4 x 2^-29 of the brightest pixel in more than 1 % of the pixels - an fp32 rounding is 2^29 times as large, the bar lets 1 % go"""
    ref = _ref(name, workdir)[0]
    flat = O.render(_scene(name, workdir), PS.CASES[name].frame["rect"], flat=True)
    d = np.abs(flat[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    print(f"{name}: the oracle's two evaluation orders: {(d > 1e-4 * 2.0 ** -29).mean():.4f} of the pixels beyond 1e-4 x 2^-29, max {d.max():.3e}")
    assert (d > 1e-4 * 2.0 ** -29).mean() > 0.01
    # ... and the same scene at 17 bounces is not such a case
    ref17 = _ref("depth17_bright-walls", workdir)[0]
    d17 = np.abs(O.render(_scene("depth17_bright-walls", workdir), flat=True)[..., :3] - ref17[..., :3]).max(-1) / np.abs(ref17[..., :3]).max()
    assert (d17 > 1e-4 * 2.0 ** -29).mean() < 0.01


def test_closed_forms_depth_zero(workdir):
    """max_depth 0: `bounces >= max_depth` ends every path at its first hit. A black film with the weights of any other depth"""
    for carrier in ("walls", "field"):
        black, lit = _ref(f"depth0-{carrier}", workdir), _ref(f"depth5-{carrier}", workdir)
        assert not black[0][..., :3].any() and lit[0][..., :3].any()
        assert np.array_equal(black[0][..., 3], lit[0][..., 3]) and black[1][0] == lit[1][0]
        assert black[1][1:] == (0, 0)      # the one query of such a path is the dead last one, and nothing is shaded


def test_closed_forms_roulette_reaches_the_film_at_depth_six(workdir):
    """Roulette runs at vertices with bounces > 3, after their light sample: at max_depth 5 the survivor's next vertex is the break on `bounces >= max_depth`,
    so neither the draw's outcome nor beta / (1 - q) reaches the film. At 6 both do."""
    for d, same in ((5, True), (6, False)):
        on, off = _ref(f"depth{d}-walls", workdir), _ref(f"depth{d}_rr0-walls", workdir)
        assert on[2]["rr_draws"] > PS.TAG_MIN and off[2]["rr_draws"] == 0
        assert np.array_equal(on[0], off[0]) == same, d
        assert (on[1][2] == off[1][2]) == same      # (shadow rays)
    # ... and rr_threshold -1 is rr_threshold 0: no beta is below either
    for walls in ("bright", "dark", "red"):
        a, b = _ref(f"rrm1_{walls}-walls", workdir), _ref(f"rr0_{walls}-walls", workdir)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    # ... and under 1e9 every vertex with bounces > 3 draws
    for walls in ("bright", "dark", "red"):
        n = _ref(f"rr1e9_{walls}-walls", workdir)[2]
        assert n["rr_draws"] == n["rr_tests"] > PS.TAG_MIN
    # the largest component against the luminance: red walls of y() = 0.27 kd.r keep the paths a grey wall of that luminance would lose
    red, dark = _ref("rr1_red-walls", workdir)[2], _ref("rr1_dark-walls", workdir)[2]
    assert red["rr_survivors"] > 10 * max(1, dark["rr_survivors"])


@pytest.mark.parametrize("integ", [PS.ALL, PS.ONE, PS.DEBUG])
def test_closed_forms_first_recursion_at_depth_three(integ, workdir):
    """li recurses while depth + 1 < max_depth from depth 1: max_depth 0, 1 and 2 are one frame, 3 is another wherever a specular lobe is hit"""
    for carrier in ("hall", "glass"):
        f0, f1, f2, f3 = (_ref(f"{carrier}{d}-{integ}", workdir) for d in (0, 1, 2, 3))
        assert np.array_equal(f0[0], f1[0]) and np.array_equal(f1[0], f2[0]) and f0[1] == f1[1] == f2[1]
        assert f2[2]["recursion_refused"] > PS.TAG_MIN and f3[2]["reflect_taken"] > PS.TAG_MIN
        assert f3[1][1] == f2[1][1] + f3[2]["reflect_taken"] + f3[2]["transmit_taken"]      # one closest-hit query per recursion
        differ = int((np.abs(f3[0][..., :3] - f2[0][..., :3]).max(-1) > 0).sum())
        print(f"{carrier} {integ}: max_depth 3 against 2: {differ} pixels differ, {f3[2]['reflect_taken']} + {f3[2]['transmit_taken']} recursions")
        assert differ > 100
    # the overflow frames of the tree: every level up to max_depth - 1 is reached on the glass, 16 | 17 | 18
    for d in (16, 17, 18):
        n = _ref(f"glass{d}-{integ}", workdir)[2]
        assert n["level_max"] == d - 1 and all(n["li_depth"][k] > PS.TAG_MIN for k in range(1, d)) and not any(n["li_depth"][d:])


def test_closed_forms_dimensions_of_64_bounces(workdir):
    """5 camera dimensions, then 5 for the light sample and 2 for the lobe at each of 64 vertices: the deepest draw is dimension 453, below the 1 000 at which
    the reference's Halton sampler panics (halton.rs:63-69)"""
    n = _ref("depth64_bright-walls", workdir)[2]
    assert n["dim_max"] == 5 + 7 * 64 < 1000 and n["end_depth"] == n["started"]


@pytest.mark.parametrize("name", sorted(PS.REFUSALS))
def test_refusals_on_the_oracle(name, workdir):
    r = PS.REFUSALS[name]
    sc = Scene.loads(*PS.refusal_scene(workdir, name))
    if r.oracle is None:
        assert np.all(np.isfinite(O.render(sc)))      # the limit is the device's own
        return
    with pytest.raises(O.OracleError, match=r.oracle):
        O.render(sc)
    if name == "halton_depth143":      # ... and one bounce less renders
        cfg, root = PS.refusal_scene(workdir, name)
        cfg["Integrator"]["max_depth"] = 142
        O.path_census()
        assert np.all(np.isfinite(O.render(Scene.loads(cfg, root))))
        assert O.path_census()["dim_max"] == 5 + 7 * 142 == 999


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

def _counters(st):
    return (st.camera_rays, st.closest_queries, st.any_queries)


def _handle(name, workdir, prec):
    r = Renderer(_scene(name, workdir), 0, prec)
    if PS.CASES[name].frame["max_paths"]: r.set_option("max_paths", PS.CASES[name].frame["max_paths"])
    return r


def _render_f32(name, workdir):
    """(frame as f64, counters, seconds) of the fp32 device for the case, rendered once"""
    if name not in _f32:
        r = _handle(name, workdir, RRT_F32)
        t0 = time.perf_counter()
        film, st = r.render(PS.CASES[name].frame["rect"], stats=True)
        dt = time.perf_counter() - t0
        r.close()
        film = film.astype(np.float64)
        film.setflags(write=False)
        _f32[name] = (film, _counters(st), dt)
    return _f32[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_f64_frame_matches_oracle(name, workdir):
    ref, counters, _, _ = _ref(name, workdir)
    t0 = time.perf_counter()
    r = _handle(name, workdir, RRT_F64)
    film, st = r.render(PS.CASES[name].frame["rect"], stats=True)
    r.close()
    dt = time.perf_counter() - t0
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert _counters(st) == counters, (_counters(st), counters)
    assert np.all(np.isfinite(film))
    scale = np.abs(ref[..., :3]).max()
    if scale == 0:
        assert PS.CASES[name].oracle == "black" and not film[..., :3].any()
        print(f"PROFILE {name} f64 black {dt:.2f}s")
        return
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / scale
    print(f"PROFILE {name} f64 max {diff.max():.3e} {dt:.2f}s")
    assert diff.max() < 1e-9, (diff.max(), int((diff > 1e-9).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PS.REFUSALS))
def test_refusals_on_the_device(name, workdir):
    ref = PS.REFUSALS[name]
    sc = Scene.loads(*PS.refusal_scene(workdir, name))
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        with pytest.raises(getattr(RRT, ref.device), match=ref.device_match):
            r.render()
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_fp32_frame_close_to_oracle(name, workdir):
    """A roulette test whose rr_max lies within 2^-20 of the threshold, or a draw within 2^-20 of q, may go the other way in fp32: the path then ends or lives
    against the oracle, and every later dimension of a path whose test flipped shifts by one. How many samples of a frame that is, is counted by the oracle
    (rr_test_near, rr_draw_near); each is one pixel at most, and twice their share of the frame's pixels is allowed beyond the bar's own 1 %. The counts are in
    profiles/path_shapes_gpu_tests.txt: zero for every case of the table (test_case_loads_and_reaches_its_states asserts it), so the allowance is 0 and the bar is the bar; path_shapes.NEAR_CASE
    is a frame that has them."""
    c = PS.CASES[name]
    ref, counters, census, _ = _ref(name, workdir)
    f32, got, dt = _render_f32(name, workdir)
    assert np.array_equal(f32[..., 3], ref[..., 3])
    assert np.all(np.isfinite(f32))
    if not ref[..., :3].any():
        assert not f32[..., :3].any()
        assert got == counters      # no shading decision, no rounding: the counters of a black frame compare in fp32 too
        print(f"PROFILE {name} f32 black near 0+0 {dt:.2f}s")
        return
    pixels = ref[..., 3] > 0
    near = census["rr_test_near"] + census["rr_draw_near"]
    allowance = 2.0 * near / int(pixels.sum())
    d32 = (np.abs(f32[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max())[pixels]
    print(f"PROFILE {name} f32 within 1e-4 {(d32 < 1e-4).mean():.4f} median {np.median(d32):.3e} max {d32.max():.3e} near {census['rr_test_near']}+{census['rr_draw_near']} "
          f"allowance {allowance:.4f} {dt:.2f}s")
    if name not in F64_ONLY: O.fp32_bar(d32, allowance)


@pytest.mark.gpu
@pytest.mark.parametrize("name", INVARIANT)
def test_overlap_shadow_changes_no_bit(name, workdir):
    """overlap_shadow runs the shadow rays of bounce b on a second stream, from the queue b & 1, while the main stream shades bounce b + 1 into the other; it is
    off by itself at max_depth <= 1. Depths 1, 2, 3 are the first three states of the alternation (no wait; one queue each; the first refill of queue 0)."""
    base, counters, _ = _render_f32(name, workdir)
    r = _handle(name, workdir, RRT_F32)
    r.set_option("overlap_shadow", 0)
    film, st = r.render(stats=True)
    r.set_option("overlap_shadow", 1)
    again, st2 = r.render(stats=True)
    r.close()
    assert np.array_equal(film, base) and np.array_equal(again, base)
    assert _counters(st) == counters == _counters(st2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", INVARIANT)
def test_shortcuts_change_no_bit(name, workdir):
    base, counters, _ = _render_f32(name, workdir)
    r = _handle(name, workdir, RRT_F32)
    for key in INVARIANT_OPTIONS: r.set_option(key, 0)
    plain, st = r.render(stats=True)
    r.close()
    assert (st.closest_queries, st.any_queries) == counters[1:]
    assert st.sky_culled == 0 and st.root_culled == 0 and st.list_launches == 0
    assert np.array_equal(plain, base)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PS.find("depth", carrier="field"))
def test_horizon_cull_meets_the_depth_guard(name, workdir):
    """The horizon tables answer a bounce ray only while bounces < max_depth (dkernels.hpp k_shade_path): the ray a path would trace at bounces == max_depth is
    never issued, so it is not counted as answered either. At max_depth 0 nothing is shaded, at 1 every bounce ray is such a ray: sky_culled is 0; from 2 on
    the tables answer escaping rays and the frame keeps its bits."""
    d = PS.CASES[name].max_depth
    r = _handle(name, workdir, RRT_F32)
    out = {}
    for h in (1, 0):
        r.set_option("horizon_cull", h)
        out[h] = r.render(stats=True)
    r.close()
    print(f"horizon cull, {name}: {out[1][1].sky_culled} of {out[1][1].closest_queries} closest-hit queries answered by the tables")
    assert np.array_equal(out[1][0], out[0][0])
    assert _counters(out[1][1]) == _counters(out[0][1])
    assert out[0][1].sky_culled == 0
    if d <= 1: assert out[1][1].sky_culled == 0
    else: assert out[1][1].sky_culled > 0
