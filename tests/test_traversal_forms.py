"""The traversal-kernel instantiations that no other test gives work ("Traversal launches": the coverage table).

At the other tests' sizes every queue is below pt_split_* = 100 000, so the persistent-thread kernel's any-hit instantiations with a sink (AO, PASSES)
only ever ran as the launch that returns at once; no frame was rendered under count_traversal, and the generic any-hit kernel never ran as an AO
launch in fp32 or on a tree deeper than 64 levels. The regime is forced with persistent_traversal / pt_split_* as test_bvh_shapes.py::FORMS does, never by a large queue.
No bar is new:
  test_ao_per_form                     test_ao.py::test_fp32_planes_close_to_reference's comparison (check_fp32_planes), its floor and spheres cases
                                       (all-triangle and MIXED trees) and a chain of 96 levels (the generic kernel's DEEP form)
  test_passes_per_form                 test_passes.py::test_passes_match_oracle's bars, on its base scene
  test_counting_frames_keep_the_bits   count_traversal 1 and the generic kernels run the same arithmetic (COUNT only adds the counters): films, pass films
                                       and the statistics other than the traversal totals are equal bit for bit
  test_f64_ao_on_a_deep_tree           test_ao.py::test_f64_planes_match_reference's 1e-9 and its cap of 0.5 % of the covered pixels left out
"""
import numpy as np
import pytest

import test_ao as TA
import test_passes as TP
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer
from test_bvh_shapes import FORMS, _shape

gpu = pytest.mark.gpu
FORM = {name: options for name, options, _ in FORMS}
DEEP = "chain_first_96"
ALL = 0xFFFFFFFF


def _deep_ao_case(workdir):
    """The chain of 96 levels over the 512-triangle heightfield as a case of test_ao.py, so that its reference and its comparison take it."""
    if "deep96" not in TA.CASES:
        TA.CASES["deep96"] = TA._case(None, (4,))
        TA._scenes["deep96"] = _shape(DEEP, workdir, film=(32, 24), nsamp=5)
    return "deep96"


# generic: k_shadow<float, DEEP, false, false, true>; persistent: k_trace_pt_f32<true, MIXED, false, false, true>
AO_RUNS = [(name, n, cos, form) for name, n, cos in (("floor", 4, True), ("floor", 4, False), ("spheres", 3, False)) for form in ("generic", "persistent")]
AO_RUNS.append(("deep96", 4, True, "generic"))      # the pair-node kernels have no deep form: the other forms are what the default handle runs


@gpu
@pytest.mark.parametrize("name,n,cos,form", AO_RUNS, ids=[f"{a}-N{b}-{'cos' if c else 'uniform'}-{d}" for a, b, c, d in AO_RUNS])
def test_ao_per_form(name, n, cos, form, workdir):
    if name == "deep96": _deep_ao_case(workdir)
    TA.check_fp32_planes(name, n, cos, workdir, set_options=FORM[form])


# persistent_traversal 2 with shadow_lists 0: the shadow launch of a passes frame is k_trace_pt_f32<true, false, false, true>, not
# k_shadow_lists_f32<true> (under grid_stride: test_passes.py::test_shortcuts_change_no_bit runs it). A MIXED case is missing: with a sphere added
# to that scene the plain fp32 frame misses the oracle in every form, which is no matter of the launch ("Traversal launches")
@gpu
def test_passes_per_form(workdir):
    r = Renderer(TP._scene("base", workdir), 0, RRT_F32)
    for k, v in dict(FORM["persistent"], shadow_lists=0).items(): r.set_option(k, v)
    film, films = r.render_passes(TP.PASSES)
    r.close()
    full = TP._ref("base", workdir, TP.FULL)
    top = np.abs(full[..., :3]).max()
    assert np.array_equal(film, films[TP.FULL])
    for k, p in enumerate(TP.PASSES):
        ref = TP._ref("base", workdir, k)
        assert ref[..., :3].max() > 0
        TP._check_weights("base", films[k][..., 3], full[..., 3])
        diff = np.abs(films[k][..., :3].astype(np.float64) - ref[..., :3]).max() / top
        print(f"base persistent: pass {p} vs oracle, max {diff:.3e} of the frame's largest value")
        assert diff < TP._colour_bar(RRT_F32), (p, diff)


# k_shadow<R, DEEP, true, PASSES> and k_closest<R, DEEP, true> over a frame's queues: no other test renders under count_traversal
@gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("tree", ["builder", DEEP])
def test_counting_frames_keep_the_bits(tree, prec, workdir):
    sh = _shape(tree, workdir, film=(32, 24), nsamp=5)
    passes = [(1, 0, 0), (ALL, 0, 1), (ALL, 0, 0)]
    out = []
    for options in ({"persistent_traversal": 0}, {"count_traversal": 1}):
        r = Renderer(sh, 0, prec)
        for k, v in options.items(): r.set_option(k, v)
        out.append(r.render(stats=True) + r.render_passes(passes, stats=True))
        r.close()
    (plain_a, pst_a, film_a, films_a, st_a), (plain_b, pst_b, film_b, films_b, st_b) = out
    assert plain_a[..., :3].max() > 0 and all(f[..., :3].max() > 0 for f in films_a)
    assert np.array_equal(plain_a, plain_b) and np.array_equal(film_a, film_b) and np.array_equal(plain_a, film_a)
    for a, b in zip(films_a, films_b): assert np.array_equal(a, b)
    for a, b in ((pst_a, pst_b), (st_a, st_b)):
        assert [getattr(a, k) for k in TP.STATS] == [getattr(b, k) for k in TP.STATS]
        assert b.any_queries > 0 and b.any_nodes > 0 and b.closest_nodes > 0 and a.any_nodes == 0      # the counting kernels counted


def _deep_ao_reference(workdir):
    return TA._reference(_deep_ao_case(workdir), 4, True, workdir)


def test_deep_ao_reference_keeps_the_exclusion_cap(workdir):
    """The shape is chosen so that the reference alone stays under test_ao.py's cap (no GPU)."""
    ref = _deep_ao_reference(workdir)
    covered = ref["ao"][..., 2] != 0
    print(f"deep96: {int((ref['risky'] & covered).sum())} of {int(covered.sum())} covered pixels hold a draw with margin < 1e-9")
    assert covered.sum() > 200 and (ref["risky"] & covered).sum() <= TA.EXCLUDED_CAP * covered.sum()
    occluded = np.concatenate([~s["free"][s["ok"]] for s in ref["parts"]])
    assert 0.02 < occluded.mean() < 0.98      # the case does test occlusion


# k_shadow<double, true, false, false, true>
@gpu
def test_f64_ao_on_a_deep_tree(workdir):
    ref = _deep_ao_reference(workdir)
    got = TA._device("deep96", 4, True, workdir, RRT_F64)
    keep = ~ref["risky"]
    for plane in TA.PLANES:
        _, wcs, _ = TA._channels(plane)
        for wc in wcs: assert np.array_equal(got[plane][..., wc], ref[plane][..., wc]), (plane, wc)
        diff = TA._value_diff(plane, got[plane], ref[plane])
        print(f"deep96: f64 {plane}: values max {diff[keep].max():.3e}")
        assert diff[keep].max() < 1e-9, (plane, diff[keep].max())
