"""ID mattes beside the film (rrt_render_mattes, rrt_matte_extract, include/rrt.h): per pixel a ranked table of (id, coverage) slots.

CPU tests: the C layout of rrt_mattes, the prototypes, the argument checks that need no handle, Scene.prim_ids, the numpy reference
(tests/matte_reference.py) pinned to tests/aov_reference.py, and the conditions the GPU cases rely on (that the overflow case overflows, that the
complete cases do not, ...), asserted on the reference alone so that a case cannot pass by having nothing to show.

GPU tests, against that reference (the table rule of rrt.h applied literally to the oracle's camera samples and first hits):
  test_f64_box_tables_match_reference        ids, coverages and all weight channels equal exactly (box filter: integers, arrival order specified)
  test_f64_gauss_object_matches_reference    no overflow: the same (id, coverage) lists at the wide-filter f64 bar (equal support, rtol 1e-12)
  test_f64_gauss_prim_identities             overflow: only the identities of rrt.h hold, and pixels the reference does not overflow in match fully
  test_fp32_object_tables_close_to_reference the fp32 bar of test_aov.py::test_fp32_planes_close_to_reference: >= 0.975 of the covered pixels identical
  test_fp32_prim_identities                  the identities against the device's own complete sums; the share of identical pixels is printed, no bar
  test_weights_are_render_aovs, test_cuts_change_nothing, test_small_pools_change_nothing, test_device_memory, test_continuing_a_table,
  test_shortcuts_change_no_bit, test_frame_is_untouched, test_matte_extract, test_error_paths, test_cli_previews_are_identical.
The scenes are tie-free, as test_aov.py requires of its own.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_reference as AR
import matte_reference as MR
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, Scene, resolve_mattes, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
GAUSS = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
SHORTCUTS = ("tile_trees", "tile_order", "quad_nodes", "lens_cull", "aux_margin")
PRECS = pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])


def _cfg5(wd, film=(64, 48), nsamp=25, filt=None):
    cfg, root = scenes.cfg5(wd, xres=film[0], yres=film[1], nsamp=nsamp, max_depth=8, n=64)
    if filt: cfg["Film"]["Filter"] = dict(filt)
    return cfg, root


def _cfg3_tilted(wd):
    """cfg3 with the enclosure and the cube instanced under generic rotations (no exact box / face ties), as test_aov.py tilts it"""
    cfg, root = scenes.cfg3(wd, xres=64, yres=64, nsamp=9, max_depth=5)
    cfg["Aggregate"]["primitives"][0]["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
    cfg["Aggregate"]["primitives"][1]["instances"] = [{"world_pos": [0.0, 0.0, 0.0], "rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}]
    return cfg, root


SCENES = {
    "cfg5": (lambda wd: _cfg5(wd), RRT_FIXED_BVH),                       # 64 x 48, 24 samples, box
    "cfg5_gauss": (lambda wd: _cfg5(wd, filt=GAUSS), RRT_FIXED_BVH),
    "cfg5_gauss8": (lambda wd: _cfg5(wd, nsamp=9, filt=GAUSS), RRT_FIXED_BVH),   # 8 samples: see test_reference_shows_what_the_gpu_cases_rely_on
    "cfg5_20x12": (lambda wd: _cfg5(wd, film=(20, 12)), RRT_FIXED_BVH),  # not whole tiles
    "cfg5_one": (lambda wd: _cfg5(wd, nsamp=2), RRT_FIXED_BVH),          # one sample per pixel
    "cfg5_16x12": (lambda wd: _cfg5(wd, film=(16, 12), nsamp=9), RRT_FIXED_BVH),
    "cfg5_16x12_gauss": (lambda wd: _cfg5(wd, film=(16, 12), nsamp=9, filt=GAUSS), RRT_FIXED_BVH),
    "cfg5_frame": (lambda wd: _cfg5(wd, film=(128, 96)), RRT_FIXED_BVH),
    "cfg1": (lambda wd: scenes.cfg1(wd, xres=64, yres=64, nsamp=9), 0),
    "cfg3": (_cfg3_tilted, 0),
}
_scenes, _samples, _refs = {}, {}, {}


def _scene(name, workdir):
    if name not in _scenes:
        build, flags = SCENES[name]
        cfg, root = build(workdir)
        _scenes[name] = Scene.loads(cfg, root, flags=flags)
    return _scenes[name]


def _ref_samples(name, workdir):
    if name not in _samples:
        _samples[name] = MR.samples(_scene(name, workdir))
    return _samples[name]


def _reference(name, by, K, workdir):
    """The reference table of one whole-film call on zeroed buffers, computed once and never changed."""
    key = (name, by, K)
    if key not in _refs:
        sc = _scene(name, workdir)
        ref = MR.apply(sc, MR.empty(sc, K), _ref_samples(name, workdir), sc.prim_ids(by))
        for a in ref.values(): a.flags.writeable = False
        _refs[key] = ref
    return _refs[key]


def _overflow_share(ref):
    hit = ref["weight"][..., 1] > 0
    return float((ref["weight"][..., 2][hit] > 0).mean())


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_mattes_struct_matches_c_layout(tmp_path):
    fields = [name for name, _ in A.Mattes._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("size %zu\\n", sizeof(rrt_mattes));']
    src += [f'printf("{f} %zu\\n", offsetof(rrt_mattes, {f}));' for f in fields]
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", str(c), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert fields == ["mem", "precision", "n_slots", "pad", "ids", "coverage", "weight"]
    assert int(out["size"]) == C.sizeof(A.Mattes)
    for f in fields:
        assert int(out[f]) == getattr(A.Mattes, f).offset, f


def test_header_declares_the_calls_and_keeps_the_abi():
    header = open(HEADER).read()
    flat = " ".join(header.split())
    assert "#define RRT_ABI_VERSION 11" in header and "#define RRT_MAX_MATTE_SLOTS 16" in header
    assert A.RRT_MAX_MATTE_SLOTS == 16
    assert "int rrt_render_mattes(rrt_handle*, const int32_t rect[4], int rank, int world, uint64_t max_samples, const uint32_t* prim_id" in flat
    assert "int rrt_matte_extract(rrt_handle*, const rrt_mattes* m, const uint32_t* ids, int n_ids" in flat
    lib = A.lib()
    assert hasattr(lib, "rrt_render_mattes") and hasattr(lib, "rrt_matte_extract")


def test_calls_refuse_bad_arguments_without_a_handle():
    """Every RRT_EINVAL that needs no handle, each with its own message; nothing is written."""
    lib = A.lib()
    ids = np.zeros(4, np.uint32); cov = np.zeros(4, np.float32); w = np.zeros(4, np.float32); alpha = np.full(1, 7.0, np.float32)
    rect = (C.c_int32 * 4)(0, 0, 1, 1)
    want = (C.c_uint32 * 2)(1, 2)

    def m(**kw):
        f = dict(mem=A.RRT_MEM_HOST, precision=A.RRT_F32, n_slots=4, pad=0, ids=ids.ctypes.data, coverage=cov.ctypes.data, weight=w.ctypes.data)
        f.update(kw)
        return A.Mattes(*[f[k] for k, _ in A.Mattes._fields_])

    def render(mm, r=rect):
        return lib.rrt_render_mattes(None, r, 0, 1, 0, None, 0, None if mm is None else C.byref(mm))

    def extract(mm, lst=want, n=2, out=alpha.ctypes.data):
        return lib.rrt_matte_extract(None, None if mm is None else C.byref(mm), lst, n, out)

    shared = ((None, b"rrt_mattes"), (m(ids=None), b"null ids"), (m(coverage=None), b"null coverage"), (m(weight=None), b"null weight"),
              (m(n_slots=0), b"n_slots"), (m(n_slots=17), b"n_slots"), (m(mem=2), b"bad mem"))
    for call, name in ((render, b"rrt_render_mattes"), (extract, b"rrt_matte_extract")):
        for mm, msg in shared:
            assert call(mm) == A.RRT_EINVAL
            assert msg in lib.rrt_last_error() and name in lib.rrt_last_error(), lib.rrt_last_error()
        assert call(m()) == A.RRT_EINVAL and b"null handle" in lib.rrt_last_error()
    assert render(m(), None) == A.RRT_EINVAL and b"null rect" in lib.rrt_last_error()
    assert extract(m(), None) == A.RRT_EINVAL and b"null id list" in lib.rrt_last_error()
    for n in (0, -1, 257):
        assert extract(m(), n=n) == A.RRT_EINVAL and b"n_ids" in lib.rrt_last_error()
    assert extract(m(), out=None) == A.RRT_EINVAL and b"null alpha" in lib.rrt_last_error()
    assert not ids.any() and not cov.any() and not w.any() and alpha[0] == 7.0


def test_prim_ids(workdir):
    sc = _scene("cfg1", workdir)     # 24 instanced spheres of one material
    n = sc.desc.n_prims
    assert n == 24
    assert np.array_equal(sc.prim_ids("material"), np.full(n, sc.desc.prims[0].material + 1, np.uint32))
    assert len(np.unique(sc.prim_ids("object"))) == 24 and len(np.unique(sc.prim_ids("instance"))) == 24
    assert sc.prim_ids("instance").min() >= 2 and np.array_equal(np.sort(sc.prim_ids("object")), np.arange(1, 25))
    assert np.array_equal(sc.prim_ids("prim"), np.arange(1, n + 1))
    sc = _scene("cfg3", workdir)     # cube and enclosure: one material, two instances
    inst = np.array([sc.desc.prims[i].instance for i in range(sc.desc.n_prims)])
    assert len(np.unique(sc.prim_ids("material"))) == 1 and len(np.unique(sc.prim_ids("object"))) == 2 == len(np.unique(inst))
    assert np.array_equal(sc.prim_ids("instance"), (inst + 2).astype(np.uint32))
    sc = _scene("cfg5", workdir)     # two uninstanced meshes, two materials
    mat = np.array([sc.desc.prims[i].material for i in range(sc.desc.n_prims)])
    assert sc.desc.n_prims == 8704 and np.all(sc.prim_ids("instance") == 1)
    assert np.array_equal(sc.prim_ids("material"), (mat + 1).astype(np.uint32))
    assert np.array_equal(sc.prim_ids("object"), (np.unique(mat, return_inverse=True)[1].reshape(-1) + 1).astype(np.uint32))
    assert sc.prim_ids("object").dtype == np.uint32 and sc.prim_ids("prim")[-1] == 8704
    with pytest.raises(ValueError):
        sc.prim_ids("colour")


@pytest.mark.parametrize("name", ["cfg5", "cfg5_gauss"])
def test_reference_is_pinned_to_the_aov_reference(name, workdir):
    """weight[0] and weight[1] are the live and hit weight planes of aov_reference; slots plus overflow are weight[1]; one id for every primitive
    puts all of weight[1] into slot 0."""
    sc = _scene(name, workdir)
    aov = AR.planes(sc)
    box = name == "cfg5"
    for by, K in (("prim", 2), ("object", 4)):
        ref = _reference(name, by, K, workdir)
        assert ref["weight"][..., 1].max() > 0 and (ref["weight"][..., 0] > ref["weight"][..., 1]).any()
        total = ref["coverage"].sum(-1) + ref["weight"][..., 2]
        if box:
            assert np.array_equal(ref["weight"][..., 0], aov["albedo"][..., 3]) and np.array_equal(ref["weight"][..., 1], aov["depth"][..., 2])
            assert np.array_equal(total, ref["weight"][..., 1])
        else:
            np.testing.assert_allclose(ref["weight"][..., 0], aov["albedo"][..., 3], rtol=1e-12, atol=0)
            np.testing.assert_allclose(ref["weight"][..., 1], aov["depth"][..., 2], rtol=1e-12, atol=0)
            np.testing.assert_allclose(total, ref["weight"][..., 1], rtol=1e-12, atol=0)
        assert np.all(ref["weight"][..., 3] == 0)
    one = MR.apply(sc, MR.empty(sc, 3), _ref_samples(name, workdir), np.full(sc.desc.n_prims, 77, np.uint32))
    hit = one["weight"][..., 1] > 0
    assert np.all(one["ids"][..., 0][hit] == 77) and np.all(one["ids"][..., 1:] == 0) and np.all(one["weight"][..., 2] == 0)
    np.testing.assert_allclose(one["coverage"][..., 0], one["weight"][..., 1], rtol=0 if box else 1e-12, atol=0)


def test_reference_shows_what_the_gpu_cases_rely_on(workdir):
    """The conditions of the GPU cases, on the reference alone."""
    # the overflow case (box, "prim", K = 2) overflows in at least a quarter of the hit pixels
    share = _overflow_share(_reference("cfg5", "prim", 2, workdir))
    print(f"box prim K=2: overflow in {share:.3f} of the hit pixels")
    assert share >= 0.25
    # the exactly-full case: pixels with exactly K = 3 ids
    sums = MR.complete_sums(_scene("cfg5", workdir), _ref_samples("cfg5", workdir), _scene("cfg5", workdir).prim_ids("prim"))
    n_ids = np.array([len(v) for v in sums.values()])
    print(f"box prim: ids per hit pixel max {n_ids.max()}, mean {n_ids.mean():.2f}, exactly 3: {(n_ids == 3).sum()}")
    assert (n_ids == 3).sum() >= 20 and (n_ids > 3).any()
    # the complete cases overflow nowhere
    assert n_ids.max() <= 8
    for name in ("cfg5", "cfg5_gauss"):
        assert _overflow_share(_reference(name, "object", 4, workdir)) == 0
    assert _overflow_share(_reference("cfg5", "prim", 8, workdir)) == 0
    assert _overflow_share(_reference("cfg1", "instance", 4, workdir)) == 0
    # the Gaussian "prim" K = 16 case overflows in some pixels and not in most. Its shape is 8 samples per pixel, not the 24 of the other cases:
    # measured on this reference, 24 samples meet more than 16 ids in 0.649 of the covered pixels (mean 19.3 ids), 12 in 0.394, 8 in 0.102 (mean 12.5)
    share = _overflow_share(_reference("cfg5_gauss8", "prim", 16, workdir))
    print(f"gauss prim K=16: overflow in {share:.3f} of the covered pixels")
    assert 0.05 < share < 0.5
    # the small films have something to show, and K = 1 overflows
    for name in ("cfg5_20x12", "cfg5_16x12"):
        assert _overflow_share(_reference(name, "prim", 2, workdir)) > 0
    one = _reference("cfg5_one", "prim", 2, workdir)     # one sample per pixel: one id, hits and misses
    assert one["weight"][..., 1].sum() > 50 and (one["weight"][..., 0] > one["weight"][..., 1]).any() and np.all(one["coverage"][..., 1] == 0)
    assert _overflow_share(_reference("cfg5", "prim", 1, workdir)) > 0.25


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

def _device(name, workdir, prec, by, K, **kw):
    r = Renderer(_scene(name, workdir), 0, prec)
    m = r.render_mattes(ids=by, slots=K, **kw)
    r.close()
    return m


def _assert_ranked(m):
    """coverage descending, ties by ascending id, empty slots last as (0, 0), ids distinct within a pixel"""
    ids, cov = m["ids"].astype(np.int64), m["coverage"].astype(np.float64)
    a, b = cov[..., :-1], cov[..., 1:]
    assert np.all(a >= b) and np.all(cov >= 0)
    assert np.all((a != b) | (b == 0) | (ids[..., :-1] < ids[..., 1:]))
    assert np.all(ids[cov == 0] == 0)
    K = ids.shape[-1]
    for i in range(K):
        for j in range(i + 1, K):
            assert not np.any((ids[..., i] == ids[..., j]) & (cov[..., j] != 0))


BOX_CASES = [("cfg5", "object", 4), ("cfg5", "prim", 8), ("cfg5", "prim", 3), ("cfg5", "prim", 2), ("cfg5", "prim", 1), ("cfg1", "instance", 4),
             ("cfg5_20x12", "prim", 2), ("cfg5_one", "prim", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,by,K", BOX_CASES, ids=[f"{n}-{b}-{k}" for n, b, k in BOX_CASES])
def test_f64_box_tables_match_reference(name, by, K, workdir):
    ref = _reference(name, by, K, workdir)
    got = _device(name, workdir, RRT_F64, by, K)
    assert ref["weight"][..., 1].max() > 0
    print(f"{name} {by} K={K}: overflow share {_overflow_share(ref):.3f}, ids equal {np.array_equal(got['ids'], ref['ids'])}, "
          f"coverage max diff {np.abs(got['coverage'] - ref['coverage']).max()}, weight max diff {np.abs(got['weight'] - ref['weight']).max()}")
    assert np.array_equal(got["ids"], ref["ids"])
    assert np.array_equal(got["coverage"], ref["coverage"])
    assert np.array_equal(got["weight"], ref["weight"])
    _assert_ranked(got)


def _lists(m):
    """per pixel {id: coverage} of the non-empty slots"""
    H, W, K = m["ids"].shape
    ids, cov = m["ids"].reshape(-1, K).tolist(), m["coverage"].reshape(-1, K).astype(np.float64).tolist()
    return [{i: c for i, c in zip(ri, rc) if c != 0} for ri, rc in zip(ids, cov)]


def _assert_same_order_up_to_near_ties(got, ref, rtol):
    """the slots hold the same ids in the same order, except where the reference coverages of the swapped slots agree to rtol (sums of the same
    filter weights in another order)"""
    diff = got["ids"] != ref["ids"]
    for y, x in zip(*np.nonzero(diff.any(-1))):
        c = ref["coverage"][y, x][diff[y, x]]
        assert c.max() - c.min() <= rtol * c.max(), (y, x, got["ids"][y, x], ref["ids"][y, x], ref["coverage"][y, x])


@pytest.mark.gpu
def test_f64_gauss_object_matches_reference(workdir):
    ref = _reference("cfg5_gauss", "object", 4, workdir)
    got = _device("cfg5_gauss", workdir, RRT_F64, "object", 4)
    assert np.array_equal(got["weight"] != 0, ref["weight"] != 0) and np.all(got["weight"][..., 2:] == 0)
    np.testing.assert_allclose(got["weight"], ref["weight"], rtol=1e-12, atol=0)
    gl, rl = _lists(got), _lists(ref)
    for g, r in zip(gl, rl):
        assert g.keys() == r.keys()
        for i in g: assert abs(g[i] - r[i]) <= 1e-12 * r[i]
    _assert_same_order_up_to_near_ties(got, ref, 1e-12)
    _assert_ranked(got)


@pytest.mark.gpu
def test_f64_gauss_prim_identities(workdir):
    """Where a pixel meets more than K ids, which K are kept is the implementation's: each stored coverage is its id's complete sum, slots plus
    overflow are weight[1], the ranking holds, and pixels the reference does not overflow in match fully."""
    sc = _scene("cfg5_gauss8", workdir)
    ref = _reference("cfg5_gauss8", "prim", 16, workdir)
    got = _device("cfg5_gauss8", workdir, RRT_F64, "prim", 16)
    sums = MR.complete_sums(sc, _ref_samples("cfg5_gauss8", workdir), sc.prim_ids("prim"))
    np.testing.assert_allclose(got["weight"][..., :2], ref["weight"][..., :2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["coverage"].sum(-1) + got["weight"][..., 2], got["weight"][..., 1], rtol=1e-12, atol=0)
    _assert_ranked(got)
    gl, rl = _lists(got), _lists(ref)
    full = 0
    for p, (g, r) in enumerate(zip(gl, rl)):
        for i, c in g.items():
            assert abs(c - sums[p][i]) <= 1e-12 * sums[p][i], (p, i)
        if ref["weight"].reshape(-1, 4)[p, 2] == 0:
            assert g.keys() == r.keys() and got["weight"].reshape(-1, 4)[p, 2] == 0
            full += 1
        else:
            assert len(g) == 16 and got["weight"].reshape(-1, 4)[p, 2] > 0
    assert 0 < full < len(gl)


def _share_identical(got, ref):
    covered = ref["weight"][..., 0] != 0
    same = np.all(got["ids"] == ref["ids"], -1) & np.all(got["coverage"].astype(np.float64) == ref["coverage"], -1)
    return float(same[covered].mean())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg5", "cfg3"])
def test_fp32_object_tables_close_to_reference(name, workdir):
    """A list differs only where a first hit crosses a silhouette, which also moves rrt_render_aov's albedo: that test's share of the covered pixels."""
    ref = _reference(name, "object", 4, workdir)
    got = _device(name, workdir, RRT_F32, "object", 4)
    share = _share_identical(got, ref)
    print(f"{name}: fp32 object K=4: {share:.4f} of the covered pixels hold the reference's table")
    assert np.array_equal(got["weight"][..., 0].astype(np.float64), ref["weight"][..., 0])
    assert share >= 0.975
    assert np.array_equal(got["coverage"].sum(-1) + got["weight"][..., 2], got["weight"][..., 1])
    _assert_ranked(got)


@pytest.mark.gpu
def test_fp32_prim_identities(workdir):
    """fp32 may take the neighbouring triangle of the heightfield: the identities are asserted against the device's own complete sums (K = 16 holds
    every id of every pixel), the share of pixels identical to the reference is printed and, under RRT_RESULTS_DIR=<dir>, written to <dir>/mattes_gpu_tests.txt
    (profiles/mattes_gpu_tests.txt holds a run's copy), without a bar."""
    full = _device("cfg5", workdir, RRT_F32, "prim", 16)
    assert np.all(full["weight"][..., 2] == 0)
    fl = _lists(full)
    lines = []
    for K in (2, 3, 8):
        got = _device("cfg5", workdir, RRT_F32, "prim", K)
        assert np.array_equal(got["weight"][..., :2], full["weight"][..., :2])
        assert np.array_equal(got["coverage"].sum(-1) + got["weight"][..., 2], got["weight"][..., 1])
        _assert_ranked(got)
        for p, g in enumerate(_lists(got)):
            assert len(g) == min(K, len(fl[p]))
            for i, c in g.items(): assert fl[p][i] == c, (p, i)
        lines.append(f"cfg5 n=64, 64x48, 24 samples, box, fp32, prim ids, K={K}: {_share_identical(got, _reference('cfg5', 'prim', K, workdir)):.4f} of the covered pixels hold the f64 reference's table")
        print(lines[-1])
    if os.environ.get("RRT_RESULTS_DIR"):      # as the timing tools keep their output; profiles/mattes_gpu_tests.txt is a copy of such a run
        os.makedirs(os.environ["RRT_RESULTS_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["RRT_RESULTS_DIR"], "mattes_gpu_tests.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("name", ["cfg5", "cfg5_gauss"])
def test_weights_are_render_aovs(name, prec, workdir):
    """weight[0] and weight[1] against albedo[3] and depth[2] of rrt_render_aov on the same handle"""
    r = Renderer(_scene(name, workdir), 0, prec)
    m = r.render_mattes(ids="prim", slots=3)
    aov = r.render_aov()
    r.close()
    assert m["weight"][..., 1].max() > 0
    if name == "cfg5":
        assert np.array_equal(m["weight"][..., 0], aov["albedo"][..., 3]) and np.array_equal(m["weight"][..., 1], aov["depth"][..., 2])
    else:
        rtol = 1e-12 if prec == RRT_F64 else 1e-5
        np.testing.assert_allclose(m["weight"][..., 0], aov["albedo"][..., 3], rtol=rtol, atol=0)
        np.testing.assert_allclose(m["weight"][..., 1], aov["depth"][..., 2], rtol=rtol, atol=0)


def _equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("ids", "coverage", "weight"))


@pytest.mark.gpu
@PRECS
def test_cuts_change_nothing(prec, workdir):
    """Four rects, and the bands of three ranks as three calls into one table: bit for bit the whole call (box filter), the overflow case included."""
    r = Renderer(_scene("cfg5", workdir), 0, prec)
    for by, K in (("prim", 2), ("prim", 8), ("object", 4)):
        whole = r.render_mattes(ids=by, slots=K)
        assert whole["weight"][..., 1].max() > 0
        rects = None
        for rect in ((0, 0, 29, 20), (29, 0, 64, 20), (0, 20, 64, 33), (0, 33, 64, 48)):
            rects = r.render_mattes(ids=by, slots=K, rect=rect, mattes=rects)
        bands = None
        for k in range(3):
            bands = r.render_mattes(ids=by, slots=K, rank=k, world=3, mattes=bands)
        assert _equal(rects, whole) and _equal(bands, whole), (by, K)
        if prec == RRT_F64:
            assert _equal(whole, _reference("cfg5", by, K, workdir))
    r.close()


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("max_paths", [256, 100])
def test_small_pools_change_nothing(prec, max_paths, workdir):
    """max_paths 256 on a 16 x 12 film with 8 samples: one pixel group, one sample per pool pass, so a pixel's table lives across eight passes;
    max_paths 100 also cuts the pixels into two groups. The pools never shrink, so the small handle is a fresh one with the option set before its
    first call (its frame's launch count shows the cut is in effect); the uncut tables come from a second handle. The overflow case (K = 2)
    still holds the reference's table exactly, and a Gaussian table without overflow the same lists to the rounding of the re-ordered sums."""
    sc = _scene("cfg5_16x12", workdir)
    small = Renderer(sc, 0, prec)
    small.set_option("max_paths", max_paths)
    _, st = small.render(stats=True)
    assert st.closest_launches >= 8      # at least one launch per sample number: the pools hold max_paths slots
    plain = Renderer(sc, 0, prec)
    for K in (2, 8):
        cut, whole = small.render_mattes(ids="prim", slots=K), plain.render_mattes(ids="prim", slots=K)
        assert cut["weight"][..., 2].max() > 0 or K == 8
        assert _equal(cut, whole), K
        if prec == RRT_F64:
            assert _equal(cut, _reference("cfg5_16x12", "prim", K, workdir)), K
    small.close(); plain.close()
    # the wide kernel across passes: every film pixel within reach reloads and stores its table per pass
    sc = _scene("cfg5_16x12_gauss", workdir)
    small = Renderer(sc, 0, prec)
    small.set_option("max_paths", max_paths)
    cut = small.render_mattes(ids="object", slots=4)
    small.close()
    ref = _reference("cfg5_16x12_gauss", "object", 4, workdir)
    rtol = 1e-12 if prec == RRT_F64 else 1e-5
    assert len(np.unique(ref["ids"])) == 3 and np.all(cut["weight"][..., 2] == 0)      # both objects and the empty slot
    np.testing.assert_allclose(cut["weight"], ref["weight"], rtol=rtol, atol=0)
    for g, r in zip(_lists(cut), _lists(ref)):
        assert g.keys() == r.keys()
        for i in g: assert abs(g[i] - r[i]) <= rtol * r[i]
    _assert_same_order_up_to_near_ties(cut, ref, rtol)
    _assert_ranked(cut)


@pytest.mark.gpu
@PRECS
def test_device_memory(prec, workdir):
    import torch
    sc = _scene("cfg5", workdir)
    r = Renderer(sc, 0, prec)
    dt = torch.float32 if prec == RRT_F32 else torch.float64
    for K in (2, 6):
        host = r.render_mattes(ids="prim", slots=K)
        ids = torch.zeros((48, 64, K), dtype=torch.int32, device="cuda:0")
        cov = torch.zeros((48, 64, K), dtype=dt, device="cuda:0")
        w = torch.zeros((48, 64, 4), dtype=dt, device="cuda:0")
        torch.cuda.synchronize()
        r.render_mattes_device((0, 0, 64, 32), ids.data_ptr(), cov.data_ptr(), w.data_ptr(), K, ids="prim")
        r.render_mattes_device((0, 32, 64, 48), ids.data_ptr(), cov.data_ptr(), w.data_ptr(), K, ids="prim")
        dev = dict(ids=ids.cpu().numpy().view(np.uint32), coverage=cov.cpu().numpy(), weight=w.cpu().numpy())
        assert host["weight"][..., 2].max() > 0 or K == 6
        assert _equal(dev, host), K
    r.close()


@pytest.mark.gpu
def test_continuing_a_table(workdir):
    """Two calls with max_samples 8 and different id tables into the same buffers equal the reference applied twice; a call on buffers that
    already hold K foreign ids adds only overflow."""
    sc = _scene("cfg5", workdir)
    s8 = MR.samples(sc, max_samples=8)
    r = Renderer(sc, 0, RRT_F64)
    for K in (3, 6):
        ref = MR.apply(sc, MR.empty(sc, K), s8, sc.prim_ids("object"))
        ref = MR.apply(sc, ref, s8, sc.prim_ids("prim"))
        got = r.render_mattes(ids="object", slots=K, max_samples=8)
        got = r.render_mattes(ids="prim", slots=K, max_samples=8, mattes=got)
        assert ref["weight"][..., 2].max() > 0 or K == 6
        assert _equal(got, ref), K
    K = 3
    foreign = dict(ids=np.tile(np.array([1000001, 1000002, 1000003], np.uint32), (48, 64, 1)), coverage=np.ones((48, 64, K)), weight=np.zeros((48, 64, 4)))
    got = r.render_mattes(ids="prim", mattes={k: v.copy() for k, v in foreign.items()})
    r.close()
    ref = _reference("cfg5", "prim", 8, workdir)
    assert np.array_equal(got["ids"], foreign["ids"]) and np.array_equal(got["coverage"], foreign["coverage"])
    assert np.array_equal(got["weight"][..., :2], ref["weight"][..., :2]) and np.array_equal(got["weight"][..., 2], ref["weight"][..., 1])


@pytest.mark.gpu
def test_shortcuts_change_no_bit(workdir):
    """tile_trees, tile_order, quad_nodes, lens_cull and aux_margin off together: the same table. The frame rendered first builds the tile trees."""
    r = Renderer(_scene("cfg5_frame", workdir), 0, RRT_F32)
    _, st = r.render(stats=True)
    assert st.tile_launches > 0
    fast = r.render_mattes(ids="prim", slots=3)
    for k in SHORTCUTS: r.set_option(k, 0)
    plain = r.render_mattes(ids="prim", slots=3)
    r.close()
    assert fast["weight"][..., 2].max() > 0
    assert _equal(fast, plain)


@pytest.mark.gpu
def test_frame_is_untouched(workdir):
    """render, render_mattes, render on one default fp32 handle: the same frame twice, bits and statistics."""
    r = Renderer(_scene("cfg5_frame", workdir), 0, RRT_F32)
    a, sa = r.render(stats=True)
    m = r.render_mattes(ids="object")
    b, sb = r.render(stats=True)
    r.close()
    assert m["weight"][..., 1].max() > 0 and a[..., :3].max() > 0
    assert sa.tile_launches > 0 and sa.root_culled > 0
    assert np.array_equal(a, b)
    for key in ("camera_rays", "closest_queries", "any_queries", "tile_launches", "root_culled"):
        assert getattr(sa, key) == getattr(sb, key), key


def _alpha(m, ids):
    cov, w0 = m["coverage"].astype(np.float64), m["weight"][..., 0].astype(np.float64)
    s = np.where(np.isin(m["ids"], ids) & (cov != 0), cov, 0.0).sum(-1)
    return np.where(w0 != 0, s / np.where(w0 != 0, w0, 1.0), 0.0)


@pytest.mark.gpu
@PRECS
def test_matte_extract(prec, workdir):
    import torch
    sc = _scene("cfg5", workdir)
    r = Renderer(sc, 0, prec)
    rtol = 1e-12 if prec == RRT_F64 else 1e-6
    m = r.render_mattes(ids="prim", slots=4)
    present = np.unique(m["ids"][m["coverage"] != 0])
    lst = np.concatenate([present[::3], present[:5], [0xFFFFFFFF, 0, 123456789]]).astype(np.uint32)[:256]     # duplicates and absent ids
    want = _alpha(m, lst)
    assert 0 < (want > 0).mean() < 1
    got = r.matte_extract(m, lst)
    assert got.dtype == r.dtype and np.array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)
    dt = torch.float32 if prec == RRT_F32 else torch.float64
    dev = {k: torch.from_numpy(v.view(np.int32) if k == "ids" else v).to("cuda:0") for k, v in m.items()}
    out = torch.full((48, 64), -1.0, dtype=dt, device="cuda:0")
    torch.cuda.synchronize()
    r.matte_extract_device(dev["ids"].data_ptr(), dev["coverage"].data_ptr(), dev["weight"].data_ptr(), 4, lst, out.data_ptr())
    assert np.array_equal(out.cpu().numpy(), got)
    # a complete table: the objects' alphas and the miss share partition 1
    m = r.render_mattes(ids="object", slots=4)
    assert np.all(m["weight"][..., 2] == 0)
    objects = np.unique(sc.prim_ids("object"))
    assert len(objects) == 2
    alphas = [r.matte_extract(m, [i]).astype(np.float64) for i in objects]
    assert all(a.max() > 0 for a in alphas)
    live = m["weight"][..., 0] != 0
    miss = 1.0 - m["weight"][..., 1].astype(np.float64)[live] / m["weight"][..., 0].astype(np.float64)[live]
    assert miss.max() > 0
    np.testing.assert_allclose(sum(a[live] for a in alphas) + miss, 1.0, rtol=rtol, atol=0)
    assert all(np.all(a[~live] == 0) for a in alphas)
    np.testing.assert_allclose(resolve_mattes(m).sum(-1)[live] + miss, 1.0, rtol=1e-12, atol=0)
    r.close()


@pytest.mark.gpu
def test_error_paths(workdir):
    import torch
    sc = _scene("cfg5", workdir)
    r = Renderer(sc, 0, RRT_F32)
    lib = A.lib()
    m = dict(ids=np.full((48, 64, 3), 5, np.uint32), coverage=np.full((48, 64, 3), 2.0, np.float32), weight=np.full((48, 64, 4), 3.0, np.float32))
    keep = {k: v.copy() for k, v in m.items()}
    with pytest.raises(RrtError, match="n_prim_id"):
        r.render_mattes(ids=np.arange(sc.desc.n_prims - 1), mattes=m)
    for rect in ((0, 0, 65, 48), (-1, 0, 64, 48), (10, 10, 10, 20)):
        with pytest.raises(RrtError, match="rect outside the film"):
            r.render_mattes(rect=rect, mattes=m)
    for rank, world in ((0, 0), (2, 2), (-1, 1)):
        with pytest.raises(RrtError, match="rank/world"):
            r.render_mattes(rank=rank, world=world, mattes=m)
    m64 = dict(ids=np.zeros((48, 64, 3), np.uint32), coverage=np.zeros((48, 64, 3), np.float64), weight=np.zeros((48, 64, 4), np.float64))
    wrong = A.Mattes(A.RRT_MEM_HOST, A.RRT_F64, 3, 0, m64["ids"].ctypes.data, m64["coverage"].ctypes.data, m64["weight"].ctypes.data)
    full = (C.c_int32 * 4)(0, 0, 64, 48)
    assert lib.rrt_render_mattes(r._h, full, 0, 1, 0, None, 0, C.byref(wrong)) == A.RRT_EINVAL and b"precision" in lib.rrt_last_error()
    alpha = np.full((48, 64), 9.0, np.float64)
    want = (C.c_uint32 * 1)(5)
    assert lib.rrt_matte_extract(r._h, C.byref(wrong), want, 1, alpha.ctypes.data) == A.RRT_EINVAL and b"precision" in lib.rrt_last_error()
    film = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, film.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_mattes(mattes=m)
    with pytest.raises(RrtError, match="in flight"):
        r.matte_extract(m, [5])
    r.render_end()
    r.close()
    assert _equal(m, keep) and not any(v.any() for v in m64.values()) and np.all(alpha == 9.0)


@pytest.mark.gpu
def test_cli_previews_are_identical(tmp_path):
    """RRT_MATTES=<path.png>: rrt_render and `python -m rs_ray_toy_amd` write the same bytes, for the default ids and for RRT_MATTE_BY / RRT_MATTE_SLOTS."""
    cfg, _ = _cfg5(str(tmp_path), (64, 48), 9)
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    for case, extra in (("default", {}), ("material", {"RRT_MATTE_BY": "material", "RRT_MATTE_SLOTS": "2"})):
        files = []
        for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
            path = tmp_path / f"mattes_{case}_{tag}.png"
            env = dict(os.environ, RRT_MATTES=str(path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **extra)
            p = subprocess.run(cmd + [str(scene), str(tmp_path / f"{tag}.png")], capture_output=True, text=True, timeout=600, env=env)
            assert p.returncode == 0, p.stderr
            files.append(path.read_bytes())
        assert files[0][:8] == b"\x89PNG\r\n\x1a\n" and len(files[0]) > 200
        assert files[0] == files[1], case
