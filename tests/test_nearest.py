"""Nearest-surface point queries (rrt_nearest, include/rrt.h).

CPU tests: the exports and prototypes (header, library, A.PROTOTYPES), the ABI version, the C layout of rrt_nearest_out, the refusals that need no
device, the numpy reference (tests/nearest_reference.py) checking itself against an independent formulation, and tools/nearest_check.cpp - the
generic walk on the CPU against a scan - built and run.

GPU tests, in both precisions:
  test_by_hand        seven regions of a right triangle, a vertex, a tie on a shared edge, a point in the plane, a dead point; expectations by hand
  test_is_a_nearest   four scenes, ~4 000 points each: the distance is the brute force's, and the reported site lies that far away
  test_tree_shapes    chains, combs, a fat leaf and the builder's tree return, bit for bit, what a single-leaf tree over the same prim_order returns
In fp32 the pair-node kernel (option "nearest_pairs": not the default, it measured slower) runs beside the generic one in test_by_hand,
test_is_a_nearest, test_tree_shapes and test_invariances and must return the same bits.
  test_max_dist       a finite search radius keeps every bit of the accepted points and reads -1, 0, 0, max_dist elsewhere
  test_chain          points lifted off known sites come back to them; nearest_records' point lies `dist` away
  test_invariances    memory kind, batch sizes, max_paths, pre-filled outputs, dist = NULL, ignored members, the frame before and after
  test_refusals       each by its message; a sphere-only scene is RRT_EUNSUP
The winner's index is never compared with the reference's argmin: a point on a shared edge or vertex is a tie between neighbours, which the two
arithmetics break differently (a float32 emulation agreed with the f64 argmin on 94.5 % of such a point set). What is asserted instead holds for
every point: the distance is the smallest one, and the reported site is at that distance.

test_tree_shapes compares each shape with a SINGLE-LEAF TREE OVER THE SHAPE'S OWN prim_order, not with bvh_shapes.one_leaf (prim_order = identity): the
rule "among equal d2 the smallest prim_order index wins" names a different triangle when prim_order differs, and vertices and edge midpoints are
ties. Against bvh_shapes.one_leaf itself the distance must still agree bit for bit, and so must the triangle wherever the two orders agree on it.

The bars (BARS) are 16 x the largest deviation measured on an MI355X against the numpy reference, per field and precision, recorded in
profiles/nearest_gpu_tests.txt; distances and positions relative to the scene extent, barycentrics absolute. Where the measurement is 0, the bar is 0.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bvh_shapes as B
import nearest_reference as NR
import surface_reference as SR
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, RrtUnsupported, Scene, scenes
from rs_ray_toy_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
CSRC = os.path.join(ROOT, "rs_ray_toy_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PRECS = pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
MEMBERS = ["mem", "precision", "prim", "b1", "b2", "dist"]

# 16 x the largest value measured (profiles/nearest_gpu_tests.txt): {key: (f64, f32)}. The fp32 distance figures are those of the points 100 extents
# away: a float32 distance of 100 extents is good to 6e-6 of the extent.
#   dist:     |dist - d_ref| / extent                                  test_is_a_nearest
#   site:     | |p - site_point(prim, b1, b2)| - d_ref | / extent      test_is_a_nearest
#   hand_b:   |b - expected|, hand_dist: |dist - expected|             test_by_hand (coordinates are small integers: no extent)
#   chain_b:  |b - the site's|, chain_dist: |dist - h| / extent        test_chain on the flat patch
#   records:  | |nearest_records(p).p - p| - dist | / extent           test_chain on every scene
BARS = {
    "dist": (16 * 1.077e-16, 16 * 9.245e-06), "site": (16 * 1.077e-16, 16 * 5.971e-08), "hand_b": (16 * 0.0, 16 * 0.0), "hand_dist": (16 * 0.0, 16 * 0.0),
    "chain_b": (16 * 0.0, 16 * 5.960e-08), "chain_dist": (16 * 0.0, 16 * 0.0), "records": (16 * 1.615e-16, 16 * 9.245e-06),
}


def _name(prec):
    return "f64" if prec == RRT_F64 else "f32"


def _check_bars(prec, case, devs):
    """Print every figure, then assert each against its bar"""
    for key, v in devs.items():
        print(f"BAR {key} {_name(prec)} {case} {v:.3e}")
    for key, v in devs.items():
        bar = BARS[key][0 if prec == RRT_F64 else 1]
        assert v <= bar, (key, case, v, bar)


def _same(a, b, fields=("prim", "b1", "b2", "dist")):
    for f in fields:
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)), f


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    return None if m is None else [a.strip() for a in m.group(1).split(",")]


def test_exports_header_and_prototypes_agree():
    lib = A.lib()
    assert hasattr(lib, "rrt_nearest"), "librrt.so does not export rrt_nearest"
    args = _header_prototype("rrt_nearest")
    assert args is not None, "include/rrt.h does not declare rrt_nearest"
    assert "rrt_nearest" in A.PROTOTYPES
    restype, argtypes = A.PROTOTYPES["rrt_nearest"]
    assert restype is C.c_int and len(argtypes) == len(args) == 5
    assert argtypes[1] is C.POINTER(A.Points) and "rrt_points" in args[1] and argtypes[2] is C.c_size_t and "size_t" in args[2]
    assert argtypes[3] is C.c_double and args[3].startswith("double") and argtypes[4] is C.POINTER(A.NearestOut) and "rrt_nearest_out" in args[4]


def test_abi_version_stays_11():
    assert "#define RRT_ABI_VERSION 11" in " ".join(open(HEADER).read().split())


def test_struct_mirror_matches_the_c_layout(tmp_path):
    assert [name for name, _ in A.NearestOut._fields_] == MEMBERS
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("size %zu\\n", sizeof(rrt_nearest_out));']
    src += [f'printf("{f} %zu\\n", offsetof(rrt_nearest_out, {f}));' for f in MEMBERS]
    src.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c11", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(A.NearestOut)
    for f in MEMBERS:
        assert int(out[f]) == getattr(A.NearestOut, f).offset, f


def _host_io(m, dtype, prec, mem=A.RRT_MEM_HOST):
    cols = [np.zeros(m, dtype) for _ in range(3)]
    pts = A.Points(mem, prec, *[c.ctypes.data for c in cols], None, None, None, None)
    arrs = dict(prim=np.full(m, 35, np.int32), b1=np.full(m, 3.5, dtype), b2=np.full(m, 3.5, dtype), dist=np.full(m, 3.5, dtype))
    out = A.NearestOut(mem, prec, *[arrs[k].ctypes.data for k in ("prim", "b1", "b2", "dist")])
    return pts, out, arrs, cols


def _untouched(arrs):
    for k, v in arrs.items():
        assert np.all(v == (35 if v.dtype == np.int32 else 3.5)), k


def test_refusals_that_need_no_device():
    """The structs are checked before the handle is looked at: every call here has a NULL handle, and only the last one gets as far as saying so"""
    lib = A.lib()
    inf = float("inf")
    pts, out, arrs, cols = _host_io(4, np.float64, RRT_F64)

    def refused(rc, substr):
        assert rc == A.RRT_EINVAL and substr in lib.rrt_last_error(), lib.rrt_last_error()
        _untouched(arrs)

    refused(lib.rrt_nearest(None, None, 4, inf, C.byref(out)), b"rrt_points")
    refused(lib.rrt_nearest(None, C.byref(pts), 4, inf, None), b"rrt_nearest_out")
    for member in ("px", "py", "pz"):
        bad = A.Points.from_buffer_copy(pts); setattr(bad, member, None)
        refused(lib.rrt_nearest(None, C.byref(bad), 4, inf, C.byref(out)), b"null point array")
    for member in ("prim", "b1", "b2"):
        bad = A.NearestOut.from_buffer_copy(out); setattr(bad, member, None)
        refused(lib.rrt_nearest(None, C.byref(pts), 4, inf, C.byref(bad)), b"null output array")
    bad = A.Points.from_buffer_copy(pts); bad.mem = 7
    refused(lib.rrt_nearest(None, C.byref(bad), 4, inf, C.byref(out)), b"bad mem")
    bad = A.NearestOut.from_buffer_copy(out); bad.mem = A.RRT_MEM_DEVICE
    refused(lib.rrt_nearest(None, C.byref(pts), 4, inf, C.byref(bad)), b"same memory kind")
    refused(lib.rrt_nearest(None, C.byref(pts), 0, inf, C.byref(out)), b"n must be > 0")
    refused(lib.rrt_nearest(None, C.byref(pts), 1 << 31, inf, C.byref(out)), b"batch too large")
    refused(lib.rrt_nearest(None, C.byref(pts), 4, float("nan"), C.byref(out)), b"max_dist")
    refused(lib.rrt_nearest(None, C.byref(pts), 4, -1.0, C.byref(out)), b"max_dist")
    nodist = A.NearestOut.from_buffer_copy(out); nodist.dist = None
    for md in (inf, 0.0):      # dist = NULL, +inf and 0 are legal: the call gets as far as the handle
        refused(lib.rrt_nearest(None, C.byref(pts), 4, md, C.byref(nodist)), b"null handle")


def test_reference_checks_itself():
    """The region algorithm against projection-or-segments. Proper triangles and exactly collinear ones: the same distance to 1e-12 of the case's size, no
    NaN. Two equal vertices: NaN where the point faces the doubled vertex's side (0 / 0 in an edge rule: such a candidate never wins), the same distance
    elsewhere. Collinear up to rounding (a sliver whose area is noise): the site is on the triangle and never nearer than the true distance."""
    res = NR.self_check()
    for kind, r in res.items():
        print(f"{kind}: {r['n']} cases, {r['nan']} NaN, largest deviation {r['dev']:.3e} x size, barycentrics inside: {r['inside']}, nearer than the truth: {r['beyond']}")
    assert set(res) == {"random", "vertex", "edge", "inside", "plane", "two_equal", "collinear", "collinear_exact"}
    for kind, r in res.items():
        assert r["inside"] and r["beyond"] == 0, kind
        if kind != "collinear":
            assert r["dev"] <= 1e-12, kind
        assert (r["nan"] > 0) == (kind == "two_equal"), kind
    assert res["two_equal"]["nan"] < res["two_equal"]["n"]


def test_nearest_check_on_the_golden_scenes():
    """tools/nearest_check.cpp: the walk of k_nearest on the CPU against a scan, on the golden scenes, a single-leaf root and a 96-deep chain (no sanitizer
    here: the program builds with -fsanitize=address,undefined as it stands)"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "nearest_check"])
    paths = [os.path.join(GOLDEN, p, "scene.json") for p in ("", "fuzz416_43", "fuzz508_96")]
    run = subprocess.run([os.path.join(ROOT, "build", "nearest_check", "nearest_check")] + paths, capture_output=True, text=True, timeout=120)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stderr
    assert "nearest_check: ok" in run.stdout and "96-deep chain" in run.stdout and "single-leaf root" in run.stdout


def test_hand_expectations_are_the_brute_force(workdir):
    """The expectations test_by_hand writes down are what the numpy brute force finds on the hand-built triangles (f64), whichever of the two tied
    triangles comes first in prim_order"""
    sc = NR.scene(workdir, "hand")
    idx = _hand_entries(sc)
    assert sorted(idx) == [0, 1, 2, 3]
    ref = NR.brute(sc, "hand", HAND_P, False)
    for k, exp in enumerate(_hand_expected(idx)):
        assert (ref["prim"][k], ref["b1"][k], ref["b2"][k]) == exp[:3], (k, exp)
        assert ref["dist"][k] == (np.inf if exp[0] < 0 else exp[3]), k


@pytest.mark.parametrize("case", ("cfg5", "scaled", "hand"))
def test_reference_cull_changes_nothing(case, workdir):
    """nearest_reference.brute rules pairs out by an exact centroid bound before the region algorithm: every seventh point against all pairs"""
    sc = NR.scene(workdir, case)
    p = HAND_P if case == "hand" else NR.points(sc, case)[0][::7]
    for f32 in (False, True):
        a, b = NR.brute(sc, case, p, f32), NR.brute_all_pairs(sc, case, p, f32)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, f32)


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------------------------------
# T0 = (0,0,0), (4,0,0), (0,4,0); T1 = (4,0,0), (0,4,0), (2,2,-4) hangs straight down from T0's hypotenuse, so for points with z >= 0 its nearest point is
# on that edge: every point whose nearest point of T0 lies on the hypotenuse or at its ends is a TIE, which goes to the smaller prim_order index.
# Per point: the answer on T0 and, where T1 ties, the answer on T1.
HAND_P = np.array([[-2, -1, 2],            # region of vertex a
                   [6, -1, 2],             # vertex b          (tie)
                   [-1, 6, 2],             # vertex c          (tie)
                   [2, -3, 4],             # edge ab
                   [-3, 2, 4],             # edge ac
                   [5, 3, 1],              # edge bc           (tie)
                   [1, 1, 5],              # the face
                   [0, 0, 0],              # exactly on vertex a
                   [2, 2, 0],              # exactly on the shared edge (tie at distance 0)
                   [1, 2, 0],              # in the plane, inside
                   [np.nan, 1, 1]], np.float64)      # dead
HAND_T0 = [(0, 0, 3), (1, 0, 3), (0, 1, 3), (0.5, 0, 5), (0, 0.5, 5), (0.75, 0.25, 3), (0.25, 0.25, 5), (0, 0, 0), (0.5, 0.5, 0), (0.25, 0.5, 0), None]
HAND_T1 = [None, (0, 0, 3), (1, 0, 3), None, None, (0.25, 0, 3), None, None, (0.5, 0, 0), None, None]
HAND_MAX_DIST = 1000.0


def _hand_entries(sc):
    """prim_order entry of each of NR.HAND_TRIS"""
    P, _, _ = SR.geometry(sc, "hand")
    return [int(np.flatnonzero((P == t).all((1, 2)))[0]) for t in NR.HAND_TRIS]


def _hand_expected(idx):
    out = []
    for t0, t1 in zip(HAND_T0, HAND_T1):
        if t0 is None: out.append((-1, 0.0, 0.0, HAND_MAX_DIST))
        elif t1 is not None and idx[1] < idx[0]: out.append((idx[1],) + tuple(float(x) for x in t1))
        else: out.append((idx[0],) + tuple(float(x) for x in t0))
    return out


@pytest.mark.gpu
@PRECS
def test_by_hand(prec, workdir):
    sc = NR.scene(workdir, "hand")
    exp = _hand_expected(_hand_entries(sc))
    r = Renderer(sc, 0, prec)
    got = r.nearest(HAND_P, HAND_MAX_DIST)
    if prec == RRT_F32:      # the pair-node kernel (not the default) returns the same bits
        r.set_option("nearest_pairs", 1)
        _same(r.nearest(HAND_P, HAND_MAX_DIST), got)
    r.close()
    for f in ("b1", "b2", "dist"):
        assert np.isfinite(got[f]).all(), f
    assert got["prim"].tolist() == [e[0] for e in exp]
    assert (got["b1"] >= 0).all() and (got["b2"] >= 0).all()
    devs = {"hand_b": float(max(np.abs(got["b1"] - [e[1] for e in exp]).max(), np.abs(got["b2"] - [e[2] for e in exp]).max())),
            "hand_dist": float(np.abs(got["dist"] - [e[3] for e in exp]).max())}
    _check_bars(prec, "hand", devs)
    assert got["dist"][7] == 0 and got["dist"][8] == 0 and got["dist"][9] == 0      # on a vertex, on the shared edge, in the plane


# ---- is a nearest -------------------------------------------------------------------------------------------------------------------------------------------------
_runs, _refs = {}, {}


def _ref(case, prec, workdir):
    key = (case, prec)
    if key not in _refs:
        sc = NR.scene(workdir, case)
        p, kinds = NR.points(sc, case)
        ref = NR.brute(sc, case, p, prec == RRT_F32)
        for a in ref.values(): a.setflags(write=False)
        _refs[key] = (p, kinds, ref)
    return _refs[key]


def _run(case, prec, workdir):
    key = (case, prec)
    if key not in _runs:
        sc = NR.scene(workdir, case)
        p, _, _ = _ref(case, prec, workdir)
        r = Renderer(sc, 0, prec)
        out = r.nearest(p)
        md = float(np.median(out["dist"]))
        # for max_dist = 0: the points, and the vertices of 40 triangles as the handle stores them (the float32-representable points are not ON an f64 handle's vertices)
        pz = np.concatenate([p, NR.world_triangles(sc, case, prec == RRT_F32)[1][:40].reshape(-1, 3)])
        _runs[key] = dict(inf=out, md=md, cut=r.nearest(p, md), zero_full=r.nearest(pz), zero=r.nearest(pz, 0.0), rec=r.nearest_records(p, fields=("p", "prim")))
        if prec == RRT_F32:      # the pair-node kernel (option "nearest_pairs"; spheres and kept instances take its rare leaf path)
            r.set_option("nearest_pairs", 1)
            _runs[key].update(inf_pairs=r.nearest(p), cut_pairs=r.nearest(p, md))
        r.close()
    return _runs[key]


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("case", NR.CASES)
def test_is_a_nearest(case, prec, workdir):
    sc = NR.scene(workdir, case)
    p, kinds, ref = _ref(case, prec, workdir)
    got = _run(case, prec, workdir)["inf"]
    if prec == RRT_F32:
        _same(_run(case, prec, workdir)["inf_pairs"], got)
        _same(_run(case, prec, workdir)["cut_pairs"], _run(case, prec, workdir)["cut"])
    ext = SR.extent(sc)
    ent, V = NR.world_triangles(sc, case, prec == RRT_F32)
    assert len(p) >= 1000 and set(kinds) == {"uniform", "hit", "lifted", "vertex", "mid", "far"}
    assert np.isin(got["prim"], ent).all()                                        # a triangle entry on every point: the sphere is no candidate
    if case == "rigid_sphere":
        assert len(ent) < int(sc.desc.n_prim_order)
    b1, b2 = got["b1"].astype(np.float64), got["b2"].astype(np.float64)
    assert (got["b1"] >= 0).all() and (got["b2"] >= 0).all()
    eps = np.finfo(got["b1"].dtype).eps
    assert (b1 + b2 <= 1 + eps).all()
    pq = p.astype(np.float32).astype(np.float64) if prec == RRT_F32 else p
    site = NR.site_point(V[np.searchsorted(ent, got["prim"])], b1, b2)
    devs = {"dist": float(np.abs(got["dist"] - ref["dist"]).max() / ext),
            "site": float(np.abs(np.linalg.norm(pq - site, axis=1) - ref["dist"]).max() / ext)}
    agree = float((got["prim"] == ref["prim"]).mean())
    print(f"{case} {_name(prec)}: {len(p)} points, the winner is the reference's argmin on {100 * agree:.1f} % (not asserted: ties)")
    _check_bars(prec, case, devs)


# ---- tree shapes ----------------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = ("chain_first_9", "chain_alt_10", "chain_second_65", "chain_alt_96", "comb_10", "comb_96", "fat_2048", "builder")
_shape_base, _shape_pts, _shape_runs = {}, {}, {}


def _heightfield(workdir, n):
    if n not in _shape_base:
        wd = os.path.join(workdir, f"nearest_hf{n}")
        os.makedirs(wd, exist_ok=True)
        cfg, root = scenes.cfg4(wd, xres=32, yres=32, nsamp=5, max_depth=3, n=n)
        _shape_base[n] = Scene.loads(cfg, root, flags=RRT_FIXED_BVH if n > 16 else 0)
    return _shape_base[n]


def _leaf_in_order(scene, order):
    """A root that is a leaf holding every primitive in the given order: the scan over that prim_order"""
    return B.ShapedScene(scene, ("leaf", [int(i) for i in order]), "one_leaf_in_order")


def _shape_run(name, prec, workdir):
    """(result on the shape, result on the single leaf over the shape's prim_order, result on bvh_shapes.one_leaf, the shape's prim_order) over the 2 000
    points of the shape's scene"""
    n = 48 if name.startswith("fat_") else 16      # fat_2048 needs more than 2 048 triangles: the 4 608-triangle heightfield, as test_bvh_shapes.py
    base = _heightfield(workdir, n)
    if n not in _shape_pts:
        _shape_pts[n] = NR.points(base, f"hf{n}", n_uniform=800, n_tris=190, with_hits=False, total=0)[0]
        wb = np.ctypeslib.as_array(base.desc.world_bound).astype(np.float64)
        # (no oracle here: "hit" points are points of the surface itself - random barycentric points of random triangles - and those lifted off it)
        ent, V = NR.world_triangles(base, f"hf{n}", False)
        rng = np.random.default_rng(3)
        t = V[rng.integers(0, len(V), 30)]
        u, v = rng.random(30) * 0.5, rng.random(30) * 0.5
        on = t[:, 0] + (t[:, 1] - t[:, 0]) * u[:, None] + (t[:, 2] - t[:, 0]) * v[:, None]
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        lift = 1e-3 * SR.extent(base)
        _shape_pts[n] = np.concatenate([_shape_pts[n], on, on + lift * nrm, on - lift * nrm]).astype(np.float32).astype(np.float64)
    p = _shape_pts[n]

    def run(sh):
        key = (id(sh), prec)
        if key not in _shape_runs:
            r = Renderer(sh, 0, prec)
            out = r.nearest(p)
            if prec == RRT_F32:      # the pair-node kernel on the same tree (where the tree has pair nodes: not with a leaf of more than 2 047 primitives)
                r.set_option("nearest_pairs", 1)
                _same(r.nearest(p), out)
            _shape_runs[key] = (out, sh)      # (the shape is kept alive: id() is the key)
            r.close()
        return _shape_runs[key][0]

    def cached(key, make):
        if key not in _shape_base: _shape_base[key] = make()
        return _shape_base[key]

    if name == "builder":
        sh, order = base, base.prim_order()
    else:
        sh = cached((name, n), lambda: B.fat(base, int(name[4:])) if name.startswith("fat_") else B.comb(base, int(name.split("_")[1])) if name.startswith("comb_")
                    else B.chain(base, int(name.split("_")[2]), name.split("_")[1]))
        order = np.array(sh._order[:], np.int64)
    leaf = cached(("leaf", name, n), lambda: _leaf_in_order(base, order))
    plain = cached(("one_leaf", n), lambda: B.one_leaf(base))
    return run(sh), run(leaf), run(plain), np.asarray(order, np.int64), p


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("name", SHAPES)
def test_tree_shapes(name, prec, workdir):
    got, leaf, plain, order, p = _shape_run(name, prec, workdir)
    assert len(p) >= 2000 and (got["prim"] >= 0).all()
    _same(got, leaf)                                                   # the walk is the scan over the same prim_order, bit for bit
    _same(got, plain, ("dist",))                                       # the smallest distance does not depend on the order
    mapped = order[got["prim"]]                                        # the primitive behind the shape's entry; one_leaf's prim_order is the identity
    same = mapped == plain["prim"]
    print(f"{name} {_name(prec)}: {len(p)} points, {int((~same).sum())} ties resolved differently under the identity prim_order")
    _same({k: v[same] for k, v in got.items()}, {k: v[same] for k, v in plain.items()}, ("b1", "b2"))


# ---- max_dist -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("case", ("cfg5", "scaled"))
def test_max_dist(case, prec, workdir):
    run = _run(case, prec, workdir)
    full, cut, zero, md = run["inf"], run["cut"], run["zero"], run["md"]
    md_r = full["dist"].dtype.type(md)
    keep = full["dist"] <= md_r
    assert 0.3 < keep.mean() < 0.7
    _same({k: v[keep] for k, v in cut.items()}, {k: v[keep] for k, v in full.items()})
    out = ~keep
    assert (cut["prim"][out] == -1).all() and not cut["b1"][out].any() and not cut["b2"][out].any() and (cut["dist"][out] == md_r).all()
    full = run["zero_full"]
    keep0 = full["dist"] == 0
    # (exact zeros: a vertex the handle stores as it is. The f64 handle of `scaled` takes the cube's vertices through the kept instance's transform in its own
    # operation order, which numpy's need not match to the last bit: there the count may be 0)
    assert keep0.sum() > 0 or (case == "scaled" and prec == RRT_F64)
    print(f"{case} {_name(prec)}: {int(keep0.sum())} of {len(keep0)} points at distance 0")
    _same({k: v[keep0] for k, v in zero.items()}, {k: v[keep0] for k, v in full.items()})
    assert (zero["prim"][~keep0] == -1).all() and not zero["b1"][~keep0].any() and not zero["b2"][~keep0].any() and not zero["dist"].any()


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
def test_chain(prec, workdir):
    """On the flat patch a site's point plus h times the normal comes back to that site; on every scene nearest_records' point lies `dist` away"""
    sc = SR.scene(workdir, "patch")
    ext = SR.extent(sc)
    ent, V = NR.world_triangles(sc, "patch", prec == RRT_F32)
    rng = np.random.default_rng(9)
    k = rng.integers(0, len(ent), 400)
    b1 = 0.1 + 0.35 * rng.random(400); b2 = 0.1 + 0.35 * rng.random(400)      # well inside: the nearest site is unique
    h = np.where(np.arange(400) % 2 == 0, 0.25, 0.05)
    site = NR.site_point(V[k], b1, b2)
    nrm = np.cross(V[k, 1] - V[k, 0], V[k, 2] - V[k, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = (site + h[:, None] * nrm).astype(np.float32).astype(np.float64)
    # what the rounded point asks for, exactly: the patch is the plane y = const, and barycentrics are affine in the point
    hq = np.abs(p[:, 1] - V[k, 0, 1])
    A2 = np.stack([V[k, 1] - V[k, 0], V[k, 2] - V[k, 0]], 2)[:, [0, 2], :]
    bq = np.linalg.solve(A2, (p - V[k, 0])[:, [0, 2], None])[..., 0]
    r = Renderer(sc, 0, prec)
    got = r.nearest(p)
    r.close()
    assert np.array_equal(got["prim"], ent[k])
    devs = {"chain_b": float(max(np.abs(got["b1"] - bq[:, 0]).max(), np.abs(got["b2"] - bq[:, 1]).max())), "chain_dist": float(np.abs(got["dist"] - hq).max() / ext)}
    _check_bars(prec, "patch", devs)
    for case in NR.CASES:
        scn = NR.scene(workdir, case)
        pts, _, _ = _ref(case, prec, workdir)
        run = _run(case, prec, workdir)
        rec, near = run["rec"], run["inf"]
        assert np.array_equal(rec["prim"], near["prim"]) and np.array_equal(rec["dist"], near["dist"])
        pq = pts.astype(np.float32).astype(np.float64) if prec == RRT_F32 else pts
        d = np.linalg.norm(rec["p"].astype(np.float64) - pq, axis=1)
        _check_bars(prec, case, {"records": float(np.abs(d - near["dist"]).max() / SR.extent(scn))})


# ---- invariances ----------------------------------------------------------------------------------------------------------------------------------------------------
def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_nearest(r, p, max_dist=np.inf, dist=True, extras=False):
    import torch
    m = len(p)
    cols = [_torch(np.asarray(p[:, k], r.dtype)) for k in range(3)]
    tdt = torch.float32 if r.dtype == np.float32 else torch.float64
    outs = dict(prim=torch.full((m,), 35, dtype=torch.int32, device="cuda:0"), b1=torch.full((m,), 3.5, dtype=tdt, device="cuda:0"),
                b2=torch.full((m,), 3.5, dtype=tdt, device="cuda:0"))
    if dist: outs["dist"] = torch.full((m,), 3.5, dtype=tdt, device="cuda:0")
    ptrs = dict(px=cols[0].data_ptr(), py=cols[1].data_ptr(), pz=cols[2].data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})
    torch.cuda.synchronize()
    if extras:      # normals and pixel set: ignored (the pixel words are outside every film)
        junk = torch.full((m,), float("nan"), dtype=tdt, device="cuda:0")
        pix = torch.full((m,), -1, dtype=torch.int32, device="cuda:0")
        pts = A.Points(A.RRT_MEM_DEVICE, r.precision, ptrs["px"], ptrs["py"], ptrs["pz"], junk.data_ptr(), junk.data_ptr(), junk.data_ptr(), pix.data_ptr())
        out = A.NearestOut(A.RRT_MEM_DEVICE, r.precision, ptrs["prim"], ptrs["b1"], ptrs["b2"], ptrs.get("dist"))
        assert A.lib().rrt_nearest(r._h, C.byref(pts), m, float(max_dist), C.byref(out)) == A.RRT_OK
    else:
        r.nearest_device(ptrs, m, max_dist)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in outs.items()}


@pytest.mark.gpu
@PRECS
def test_invariances(prec, workdir):
    """Bit for bit, on the scaled scene (a kept instance: the rare leaf path in fp32)"""
    case = "scaled"
    sc = NR.scene(workdir, case)
    p, _, _ = _ref(case, prec, workdir)
    p = np.concatenate([p, p[:300] + 0.125])[:4097 + 65]      # more than 4 097 points, NaN-free
    assert len(p) == 4097 + 65
    r = Renderer(sc, 0, prec)
    frame0 = r.render()
    full = r.nearest(p)
    md = float(np.median(full["dist"]))
    cut = r.nearest(p, md)
    # host and device memory; device outputs pre-filled with 3.5 / 35 are overwritten, rejected points included
    _same(full, _device_nearest(r, p))
    _same(cut, _device_nearest(r, p, md))
    # dist = NULL changes no other array; normals and pixel are ignored
    _same(_device_nearest(r, p, md, dist=False), cut, ("prim", "b1", "b2"))
    _same(_device_nearest(r, p, md, extras=True), cut)
    # host outputs pre-filled are overwritten
    pts, out, arrs, cols = _host_io(len(p), r.dtype, prec)
    for k in range(3): cols[k][:] = p[:, k]
    assert A.lib().rrt_nearest(r._h, C.byref(pts), len(p), md, C.byref(out)) == A.RRT_OK
    _same(arrs, cut)
    # batches of 1, 63, 64, 65 and 4 097 points against slices of the large batch
    for n, at in ((1, 0), (1, 777), (63, 0), (64, 100), (65, 31), (4097, 0), (4097, 65)):
        _same(r.nearest(p[at:at + n], md), {k: v[at:at + n] for k, v in cut.items()})
    # a small max_paths cuts the points into many passes
    r.set_option("max_paths", 64)
    _same(r.nearest(p), full)
    _same(r.nearest(p, md), cut)
    r.close()
    # the generic kernel and the pair-node kernel return the same bits (fp32; f64 has the generic one alone), also cut into many passes
    if prec == RRT_F32:
        r = Renderer(sc, 0, prec)
        r.set_option("nearest_pairs", 1)
        _same(r.nearest(p), full)
        _same(_device_nearest(r, p, md), cut)
        r.set_option("max_paths", 64)
        _same(r.nearest(p, md), cut)
        r.close()
    # a frame rendered before and after the call is the same frame
    r = Renderer(sc, 0, prec)
    r.nearest(p); r.nearest(p, md)
    frame1 = r.render()
    r.close()
    assert np.array_equal(frame0, frame1) and frame0[..., :3].max() > 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
def test_refusals(prec, workdir):
    import torch
    lib = A.lib()
    spheres = SR.scene(workdir, "cfg1")
    tri = SR.scene(workdir, "rigid")
    rs, rt = Renderer(spheres, 0, prec), Renderer(tri, 0, prec)
    other = RRT_F32 if prec == RRT_F64 else RRT_F64
    inf = float("inf")
    pts, out, arrs, cols = _host_io(4, rt.dtype, prec)

    def refused(rc, substr, code=A.RRT_EINVAL):
        assert rc == code and substr in lib.rrt_last_error(), lib.rrt_last_error()
        _untouched(arrs)

    bad = A.Points.from_buffer_copy(pts); bad.precision = other
    refused(lib.rrt_nearest(rt._h, C.byref(bad), 4, inf, C.byref(out)), b"point precision must match the handle")
    bad = A.NearestOut.from_buffer_copy(out); bad.precision = other
    refused(lib.rrt_nearest(rt._h, C.byref(pts), 4, inf, C.byref(bad)), b"output precision must match the handle")
    bad = A.Points.from_buffer_copy(pts); bad.py = None
    refused(lib.rrt_nearest(rt._h, C.byref(bad), 4, inf, C.byref(out)), b"null point array")
    bad = A.NearestOut.from_buffer_copy(out); bad.b2 = None
    refused(lib.rrt_nearest(rt._h, C.byref(pts), 4, inf, C.byref(bad)), b"null output array")
    bad = A.NearestOut.from_buffer_copy(out); bad.mem = 5
    refused(lib.rrt_nearest(rt._h, C.byref(pts), 4, inf, C.byref(bad)), b"same memory kind")
    bad = A.Points.from_buffer_copy(pts); bad.mem = 5
    refused(lib.rrt_nearest(rt._h, C.byref(bad), 4, inf, C.byref(out)), b"bad mem")
    refused(lib.rrt_nearest(rt._h, C.byref(pts), 0, inf, C.byref(out)), b"n must be > 0")
    refused(lib.rrt_nearest(rt._h, C.byref(pts), (1 << 31), inf, C.byref(out)), b"batch too large")
    refused(lib.rrt_nearest(rt._h, C.byref(pts), 4, float("nan"), C.byref(out)), b"max_dist must be >= 0")
    refused(lib.rrt_nearest(rt._h, C.byref(pts), 4, -0.5, C.byref(out)), b"max_dist must be >= 0")
    refused(lib.rrt_nearest(None, C.byref(pts), 4, inf, C.byref(out)), b"null handle")
    # a sphere-only scene
    refused(lib.rrt_nearest(rs._h, C.byref(pts), 4, inf, C.byref(out)), b"no triangle entry", A.RRT_EUNSUP)
    with pytest.raises(RrtUnsupported, match="no triangle entry"):
        rs.nearest(np.zeros((4, 3)))
    # a frame in flight
    W, H = tri.resolution
    film = torch.zeros((H, W, 4), dtype=torch.float32 if prec == RRT_F32 else torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rt.render_bands_begin(0, 1, film.data_ptr())
    refused(lib.rrt_nearest(rt._h, C.byref(pts), 4, inf, C.byref(out)), b"a frame is in flight")
    rt.render_end()
    assert lib.rrt_nearest(rt._h, C.byref(pts), 4, inf, C.byref(out)) == A.RRT_OK and (arrs["prim"] >= 0).all()      # +inf is legal, and the handle is as it was
    assert lib.rrt_nearest(rt._h, C.byref(pts), 4, 0.0, C.byref(out)) == A.RRT_OK                                    # so is 0
    with pytest.raises(RrtError):
        rt.nearest(np.zeros((4, 3)), -1.0)
    rs.close(); rt.close()
