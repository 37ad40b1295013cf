"""All hits along a ray, in order (rrt_trace_all, include/rrt.h).

CPU tests: the exports and prototypes (header, library, A.PROTOTYPES), the ABI version, the C layout of rrt_multi_hits, the refusals that need no
device, tools/trace_all_check.cpp - the walk on the CPU against the scan - built and run, and the numpy reference (tests/trace_all_reference.py)
on its own: its cull changes nothing, it finds what test_by_hand writes down, and at most 2 % of the `uniform` and `through` rays of every case are
marginal (a condition on the cases, not a measurement: the comparison below is exact on the other 98 %).

GPU tests, in both precisions:
  test_by_hand                  a unit cube and a tetrahedron: through both, missing, starting inside, tmax between two hits, exactly at a shared edge,
                                a dead ray, skip_prim; expectations by hand, exact
  test_is_the_scan              five scenes, 4 162 rays each: count and the slots' prim are the brute force's on every non-marginal ray, t, b1, b2 within
                                BARS; on marginal and tie rays every reported hit is a candidate the reference has within its band
  test_tree_shapes              chains, a comb, a fat leaf and the builder's tree return, bit for bit, what a single-leaf tree over the same prim_order returns
  test_k_and_count              k = 1, 4, 16 are prefixes of one another; count = NULL and k = 0 change nothing else; the empty slots
  test_chain                    plane s of (prim, b1, b2) through surface_at is the point o + d t[s]; slot 0 against rrt_trace_closest
  test_inside_and_signed_field  Renderer.inside against the analytic solids; distance_field(signed=True); the unsigned default unchanged
  test_invariances              memory kind, batch sizes, max_paths, pre-filled outputs, b1 = b2 = NULL, the frame before and after
  test_refusals                 each by its message; a sphere-only scene is RRT_EUNSUP; a frame in flight

The bars (BARS) are 16 x the largest deviation measured on an MI355X against the numpy reference, per field and precision, recorded in
profiles/trace_all_gpu_tests.txt; t and positions relative to the scene extent, barycentrics absolute. Where the measurement is 0, the bar is 0.
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
import trace_all_reference as TR
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, RrtUnsupported, Scene, scenes
from rs_ray_toy_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
CSRC = os.path.join(ROOT, "rs_ray_toy_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PRECS = pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
MEMBERS = ["mem", "precision", "k", "pad", "t", "prim", "b1", "b2", "count"]
SLOTS = ("t", "prim", "b1", "b2")
FIELDS = SLOTS + ("count",)

# 16 x the largest value measured (profiles/trace_all_gpu_tests.txt): {key: (f64, f32)}
#   t:        |t - t_ref| / extent on the filled slots of the non-marginal rays      test_is_the_scan
#   b:        |b - b_ref| there                                                      test_is_the_scan
#   hand_t, hand_b: |t - expected|, |b - expected|                                   test_by_hand (coordinates are small integers: no extent)
#   chain_p:  |surface_at(plane s).p - (o + d t[s])| / extent                        test_chain
BARS = {
    "t": (16 * 4.129e-14, 16 * 1.451e-05), "b": (16 * 5.445e-12, 16 * 1.329e-03), "hand_t": (16 * 0.0, 16 * 0.0), "hand_b": (16 * 0.0, 16 * 0.0),
    "chain_p": (16 * 8.622e-14, 16 * 7.639e-05),
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


def _same(a, b, fields=FIELDS):
    for f in fields:
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)), f


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    return None if m is None else [a.strip() for a in m.group(1).split(",")]


def test_exports_header_and_prototypes_agree():
    lib = A.lib()
    assert hasattr(lib, "rrt_trace_all"), "librrt.so does not export rrt_trace_all"
    args = _header_prototype("rrt_trace_all")
    assert args is not None, "include/rrt.h does not declare rrt_trace_all"
    assert "rrt_trace_all" in A.PROTOTYPES
    restype, argtypes = A.PROTOTYPES["rrt_trace_all"]
    assert restype is C.c_int and len(argtypes) == len(args) == 4
    assert argtypes[1] is C.POINTER(A.Rays) and "rrt_rays" in args[1] and argtypes[2] is C.c_size_t and "size_t" in args[2]
    assert argtypes[3] is C.POINTER(A.MultiHits) and "rrt_multi_hits" in args[3]
    assert re.search(r"#define\s+RRT_MAX_HITS\s+16\b", open(HEADER).read()) and A.RRT_MAX_HITS == 16


def test_abi_version_stays_11():
    assert "#define RRT_ABI_VERSION 11" in " ".join(open(HEADER).read().split())


def test_struct_mirror_matches_the_c_layout(tmp_path):
    assert [name for name, _ in A.MultiHits._fields_] == MEMBERS
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("size %zu\\n", sizeof(rrt_multi_hits));']
    src += [f'printf("{f} %zu\\n", offsetof(rrt_multi_hits, {f}));' for f in MEMBERS]
    src.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c11", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(A.MultiHits)
    for f in MEMBERS:
        assert int(out[f]) == getattr(A.MultiHits, f).offset, f


def _host_io(m, dtype, prec, k=4, mem=A.RRT_MEM_HOST):
    cols = [np.zeros(m, dtype) for _ in range(7)]
    cols[3][:] = 1.0; cols[6][:] = np.inf
    rays = A.Rays(mem, prec, *[c.ctypes.data for c in cols], None)
    arrs = dict(t=np.full((k, m), 3.5, dtype), prim=np.full((k, m), 35, np.int32), b1=np.full((k, m), 3.5, dtype), b2=np.full((k, m), 3.5, dtype), count=np.full(m, 35, np.uint32))
    out = A.MultiHits(mem, prec, k, 0, *[arrs[f].ctypes.data for f in FIELDS])
    return rays, out, arrs, cols


def _untouched(arrs):
    for k, v in arrs.items():
        assert np.all(v == (35 if v.dtype.kind in "iu" else 3.5)), k


def _struct_refusals(lib, h, rays, out, refused):
    """The refusals that are decided on the structs alone, with handle h (None: a NULL handle, looked at last)"""
    call = lambda r, n, o: lib.rrt_trace_all(h, None if r is None else C.byref(r), n, None if o is None else C.byref(o))
    refused(call(None, 4, out), b"rrt_rays")
    refused(call(rays, 4, None), b"rrt_multi_hits")
    for member in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax"):
        bad = A.Rays.from_buffer_copy(rays); setattr(bad, member, None)
        refused(call(bad, 4, out), b"null ray array")
    for k in (-1, 17):
        bad = A.MultiHits.from_buffer_copy(out); bad.k = k
        refused(call(rays, 4, bad), b"k must be 0 .. RRT_MAX_HITS")
    for member in ("t", "prim"):
        bad = A.MultiHits.from_buffer_copy(out); setattr(bad, member, None)
        refused(call(rays, 4, bad), b"null slot array")
    for member in ("b1", "b2"):
        bad = A.MultiHits.from_buffer_copy(out); setattr(bad, member, None)
        refused(call(rays, 4, bad), b"b1 and b2 must both be NULL or both be set")
    bad = A.MultiHits.from_buffer_copy(out); bad.k = 0; bad.count = None
    refused(call(rays, 4, bad), b"k == 0 needs count")
    bad = A.Rays.from_buffer_copy(rays); bad.mem = 7
    refused(call(bad, 4, out), b"bad mem")
    bad = A.MultiHits.from_buffer_copy(out); bad.mem = A.RRT_MEM_DEVICE
    refused(call(rays, 4, bad), b"same memory kind")
    refused(call(rays, 0, out), b"n must be > 0")
    refused(call(rays, 1 << 31, out), b"batch too large")


def test_refusals_that_need_no_device():
    """The structs are checked before the handle is looked at: every call here has a NULL handle, and only the last ones get as far as saying so"""
    lib = A.lib()
    rays, out, arrs, cols = _host_io(4, np.float64, RRT_F64)

    def refused(rc, substr):
        assert rc == A.RRT_EINVAL and substr in lib.rrt_last_error(), lib.rrt_last_error()
        _untouched(arrs)

    _struct_refusals(lib, None, rays, out, refused)
    legal = [A.MultiHits.from_buffer_copy(out) for _ in range(3)]      # count = NULL, b1 = b2 = NULL, k = 0 with count: legal, the call gets as far as the handle
    legal[0].count = None; legal[1].b1 = None; legal[1].b2 = None; legal[2].k = 0; legal[2].t = None; legal[2].prim = None
    for ok in legal:
        refused(lib.rrt_trace_all(None, C.byref(rays), 4, C.byref(ok)), b"null handle")


def test_trace_all_check_on_the_golden_scenes():
    """tools/trace_all_check.cpp: the walk of k_trace_all on the CPU against the scan, on the golden scenes, a single-leaf root and a 96-deep chain (no
    sanitizer here: the program builds with -fsanitize=address,undefined as it stands)"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "trace_all_check"])
    paths = [os.path.join(GOLDEN, p, "scene.json") for p in ("", "fuzz416_43", "fuzz508_96")]
    run = subprocess.run([os.path.join(ROOT, "build", "trace_all_check", "trace_all_check")] + paths, capture_output=True, text=True, timeout=120)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stderr
    assert "trace_all_check: ok" in run.stdout and "96-deep chain" in run.stdout and "single-leaf root" in run.stdout


_refs = {}


def _ref(case, prec, workdir):
    key = (case, prec)
    if key not in _refs:
        sc = TR.scene(workdir, case)
        o, d, tmax, kinds = TR.rays(sc, case)
        ref = TR.brute(sc, case, o, d, tmax, prec == RRT_F32)
        for a in ref.values():
            if isinstance(a, np.ndarray): a.setflags(write=False)
        _refs[key] = (o, d, tmax, kinds, ref)
    return _refs[key]


@pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", TR.CASES)
def test_reference_margins(case, prec, workdir):
    """The reference alone: at most 2 % of the uniform and through rays are marginal at the precision's band"""
    o, d, tmax, kinds, ref = _ref(case, prec, workdir)
    assert len(o) == TR.N_RAYS and set(kinds) == {"uniform", "through", "edge", "vertex"}
    assert 0.4 < np.isfinite(tmax).mean() < 0.6
    for kind in ("uniform", "through"):
        sel = kinds == kind
        share = float(ref["marginal"][sel].mean())
        print(f"{case} {_name(prec)} {kind}: {int(sel.sum())} rays, {100 * share:.2f} % marginal, {float(ref['count'][sel].mean()):.2f} hits per ray")
        assert sel.sum() >= 1500 and share <= 0.02, (case, kind, share)
    assert ref["count"][kinds == "through"].mean() >= 0.5      # (half of them are cut short by a finite tmax)


@pytest.mark.parametrize("case", ("cfg5", "scaled", "hand_closed"))
def test_reference_cull_changes_nothing(case, workdir):
    """trace_all_reference.brute rules pairs out by the distance of the ray's line from the centroid before the three rules: every 41st ray against all pairs"""
    sc = TR.scene(workdir, case)
    o, d, tmax, _ = TR.rays(sc, case)
    for f32 in (False, True):
        a, b = TR.brute(sc, case, o[::41], d[::41], tmax[::41], f32), TR.brute_all_pairs(sc, case, o[::41], d[::41], tmax[::41], f32)
        for k in FIELDS + ("marginal", "n_marginal", "cand_key", "cand_t"):
            assert np.array_equal(a[k], b[k]), (k, f32)


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------------------------------
# trace_all_reference.HAND_TRIS: the unit cube (faces X0, X1, Y0, ... of two triangles a, b each; X0a = (0,0,0), (0,1,0), (0,1,1), X0b = (0,0,0), (0,1,1), (0,0,1):
# the diagonal of the faces x = 0 and x = 1 is y = z) and the tetrahedron (4,0,0), (6,0,0), (4,2,0), (4,0,2) (TA: the face x = 4, TD: the slanted face x + y + z = 6).
# All rays run along +x. Per ray: o, tmax, the face to skip, and the hits (face, t, b1, b2) in order; among equal t the smaller entry goes first.
INF = np.inf
HAND_RAYS = [
    # through both solids: x = 0 and x = 1 above the diagonal (z > y), x = 4, and the slanted face at x = 6 - 0.75
    ((-1, 0.25, 0.5), INF, None, [("X0b", 1, 0.25, 0.25), ("X1b", 2, 0.25, 0.25), ("TA", 5, 0.125, 0.25), ("TD", 6.25, 0.125, 0.25)]),
    ((-1, 5, 5), INF, None, []),                                                                                          # missing everything
    ((0.5, 0.25, 0.5), INF, None, [("X1b", 0.5, 0.25, 0.25), ("TA", 3.5, 0.125, 0.25), ("TD", 4.75, 0.125, 0.25)]),       # starting inside the cube
    ((-1, 0.25, 0.5), 3, None, [("X0b", 1, 0.25, 0.25), ("X1b", 2, 0.25, 0.25)]),                                         # tmax between the second and the third hit
    # exactly at the shared diagonal y = z of the faces x = 0 and x = 1: both neighbours report, u = 0 on one and v = 0 on the other
    ((-1, 0.5, 0.5), INF, None, [("X0a", 1, 0, 0.5), ("X0b", 1, 0.5, 0), ("X1a", 2, 0, 0.5), ("X1b", 2, 0.5, 0), ("TA", 5, 0.25, 0.25), ("TD", 6, 0.25, 0.25)]),
    ((np.nan, 0.25, 0.5), INF, None, []),                                                                                 # dead
    ((-1, 0.25, 0.5), INF, "X0b", [("X1b", 2, 0.25, 0.25), ("TA", 5, 0.125, 0.25), ("TD", 6.25, 0.125, 0.25)]),           # skip_prim removes the first hit
]


def _hand_io(idx, dtype=np.float64):
    o = np.array([r[0] for r in HAND_RAYS], dtype)
    d = np.tile(np.array([1.0, 0.0, 0.0], dtype), (len(HAND_RAYS), 1))
    tmax = np.array([r[1] for r in HAND_RAYS], dtype)
    skip = np.array([-1 if r[2] is None else idx[r[2]] for r in HAND_RAYS], np.int32)
    return o, d, tmax, skip


def _hand_expected(idx, k=TR.K):
    m = len(HAND_RAYS)
    exp = dict(t=np.zeros((k, m)), prim=np.full((k, m), -1, np.int32), b1=np.zeros((k, m)), b2=np.zeros((k, m)), count=np.zeros(m, np.uint32))
    for i, (_, tmax, _, hits) in enumerate(HAND_RAYS):
        exp["t"][:, i] = tmax
        exp["count"][i] = len(hits)
        for s, (face, t, b1, b2) in enumerate(sorted(hits, key=lambda h: (h[1], idx[h[0]]))):
            exp["t"][s, i], exp["prim"][s, i], exp["b1"][s, i], exp["b2"][s, i] = t, idx[face], b1, b2
    return exp


def test_hand_expectations_are_the_brute_force(workdir):
    """The expectations test_by_hand writes down are what the numpy brute force finds on the hand-built solids (f64), exactly"""
    sc = TR.scene(workdir, "hand_closed")
    idx = TR.hand_entries(sc)
    assert sorted(idx.values()) == list(range(16))
    o, d, tmax, skip = _hand_io(idx)
    ref = TR.brute(sc, "hand_closed", o, d, tmax, False, skip=skip)
    exp = _hand_expected(idx)
    for f in FIELDS:
        assert np.array_equal(ref[f], exp[f]), f
    assert idx["X0a"] != idx["X0b"] and exp["prim"][0, 4] == min(idx["X0a"], idx["X0b"]) and exp["prim"][1, 4] == max(idx["X0a"], idx["X0b"])


@pytest.mark.gpu
@PRECS
def test_by_hand(prec, workdir):
    sc = TR.scene(workdir, "hand_closed")
    idx = TR.hand_entries(sc)
    exp = _hand_expected(idx)
    o, d, tmax, skip = _hand_io(idx)
    r = Renderer(sc, 0, prec)
    got = r.trace_all(o, d, tmax, k=TR.K, skip_prim=skip)
    r.close()
    assert got["count"].tolist() == exp["count"].tolist()
    assert np.array_equal(got["prim"], exp["prim"])
    filled = exp["prim"] >= 0
    assert np.array_equal(got["t"][~filled], exp["t"][~filled].astype(r.dtype))      # empty slots: tmax (inf, 3) - the dead ray's too
    assert not got["b1"][~filled].any() and not got["b2"][~filled].any()
    devs = {"hand_t": float(np.abs(got["t"][filled] - exp["t"][filled]).max()),
            "hand_b": float(max(np.abs(got["b1"][filled] - exp["b1"][filled]).max(), np.abs(got["b2"][filled] - exp["b2"][filled]).max()))}
    _check_bars(prec, "hand_closed", devs)


# ---- is the scan --------------------------------------------------------------------------------------------------------------------------------------------------
_runs = {}


def _run(case, prec, workdir):
    key = (case, prec)
    if key not in _runs:
        sc = TR.scene(workdir, case)
        o, d, tmax, _, _ = _ref(case, prec, workdir)
        r = Renderer(sc, 0, prec)
        run = dict(k8=r.trace_all(o, d, tmax, k=TR.K))
        if case == "cfg5":      # test_k_and_count
            run.update({f"k{k}": r.trace_all(o, d, tmax, k=k) for k in (1, 4, 16)})
            run.update(k4_nocount=r.trace_all(o, d, tmax, k=4, count=False), k16_nocount=r.trace_all(o, d, tmax, k=16, count=False), k0=r.trace_all(o, d, tmax, k=0))
        planes = [r.surface_at(run["k8"]["prim"][s], run["k8"]["b1"][s], run["k8"]["b2"][s], fields=("p",))["p"] for s in range(TR.K)]      # test_chain
        run.update(planes=planes, closest=r.trace_closest(o, d, tmax))
        r.close()
        _runs[key] = run
    return _runs[key]


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("case", TR.CASES)
def test_is_the_scan(case, prec, workdir):
    sc = TR.scene(workdir, case)
    o, d, tmax, kinds, ref = _ref(case, prec, workdir)
    got = _run(case, prec, workdir)["k8"]
    ext = SR.extent(sc)
    band = TR.BAND[prec == RRT_F32]
    ent, _ = NR.world_triangles(sc, case, prec == RRT_F32)
    m = len(o)
    assert m == TR.N_RAYS
    filled = got["prim"] >= 0
    held = filled.sum(0)
    assert np.array_equal(held, np.minimum(got["count"], TR.K)) and (filled[1:] <= filled[:-1]).all()      # the slots fill from 0, count says how many
    assert np.isin(got["prim"][filled], ent).all()                                                          # triangle entries only: a sphere is never reported
    if case == "rigid_sphere":
        assert len(ent) < int(sc.desc.n_prim_order)
    tq = tmax.astype(got["t"].dtype)
    assert np.array_equal(got["t"][~filled], np.broadcast_to(tq, filled.shape)[~filled]) and not got["b1"][~filled].any() and not got["b2"][~filled].any()
    t = np.where(filled, got["t"].astype(np.float64), np.inf)
    assert (t[1:] >= t[:-1]).all()                                                                # t is non-decreasing along the slots of every ray
    tie = np.isin(kinds, ("edge", "vertex"))
    strong = ~ref["marginal"] & ~tie
    assert strong.mean() > 0.8
    # non-marginal rays: the reference's count and prims, t and barycentrics within the bars
    assert np.array_equal(got["count"][strong], ref["count"][strong])
    assert np.array_equal(got["prim"][:, strong], ref["prim"][:, strong])
    f = filled & strong[None, :]
    devs = {"t": float(np.abs(got["t"][f] - ref["t"][f]).max() / ext),
            "b": float(max(np.abs(got["b1"][f] - ref["b1"][f]).max(), np.abs(got["b2"][f] - ref["b2"][f]).max()))}
    # marginal and tie rays: every reported hit is a candidate the reference has within its band, at that t; count is off by at most the marginal candidates
    weak = ~strong
    ss, ii = np.nonzero(filled & weak[None, :])
    key = ii.astype(np.int64) * ref["key_base"] + got["prim"][ss, ii]
    assert len(ref["cand_key"]) > 0
    at = np.minimum(np.searchsorted(ref["cand_key"], key), len(ref["cand_key"]) - 1)
    assert np.array_equal(ref["cand_key"][at], key)
    assert (np.abs(got["t"][ss, ii] - ref["cand_t"][at]) <= band * ext).all()
    off = np.abs(got["count"][weak].astype(np.int64) - ref["count"][weak].astype(np.int64))
    assert (off <= ref["n_marginal"][weak]).all()
    print(f"{case} {_name(prec)}: {m} rays, {int(strong.sum())} compared exactly, {int(weak.sum())} marginal or tie rays of which {int((off > 0).sum())} count differently, "
          f"{int(filled.sum())} hits, {int((got['count'] > TR.K).sum())} rays with more than {TR.K}")
    _check_bars(prec, case, devs)


# ---- tree shapes ----------------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = ("chain_first_9", "chain_alt_96", "comb_96", "fat_2048", "builder")
_shape_base, _shape_rays, _shape_runs = {}, {}, {}


def _heightfield(workdir, n):
    if n not in _shape_base:
        wd = os.path.join(workdir, f"trace_all_hf{n}")
        os.makedirs(wd, exist_ok=True)
        cfg, root = scenes.cfg4(wd, xres=32, yres=32, nsamp=5, max_depth=3, n=n)
        _shape_base[n] = Scene.loads(cfg, root, flags=RRT_FIXED_BVH if n > 16 else 0)
    return _shape_base[n]


def _shape_run(name, prec, workdir):
    """(result on the shape, result on the single leaf over the shape's prim_order) over 2 000 rays of the shape's scene, k = 8 with count"""
    n = 48 if name.startswith("fat_") else 16      # fat_2048 needs more than 2 048 triangles: the 4 608-triangle heightfield, as test_bvh_shapes.py
    base = _heightfield(workdir, n)
    if n not in _shape_rays:
        _shape_rays[n] = TR.rays(base, f"trace_all_hf{n}", seed=23, total=2000, n_through=900, n_edge=150, n_vertex=150)
    o, d, tmax, _ = _shape_rays[n]

    def run(sh):
        key = (id(sh), prec)
        if key not in _shape_runs:
            r = Renderer(sh, 0, prec)
            _shape_runs[key] = (r.trace_all(o, d, tmax, k=TR.K), sh)      # (the shape is kept alive: id() is the key)
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
    leaf = cached(("leaf", name, n), lambda: B.ShapedScene(base, ("leaf", [int(i) for i in order]), "one_leaf_in_order"))
    return run(sh), run(leaf)


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("name", SHAPES)
def test_tree_shapes(name, prec, workdir):
    """The walk is the scan: bit for bit in every output array against a root that is one leaf over the same prim_order"""
    got, leaf = _shape_run(name, prec, workdir)
    assert got["count"].sum() > 1000 and (got["count"] > 1).sum() > 100
    print(f"{name} {_name(prec)}: {len(got['count'])} rays, {int(got['count'].sum())} hits, at most {int(got['count'].max())} on a ray")
    _same(got, leaf)


# ---- k and count ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
def test_k_and_count(prec, workdir):
    run = _run("cfg5", prec, workdir)
    o, d, tmax, _, _ = _ref("cfg5", prec, workdir)
    k16 = run["k16"]
    assert (k16["count"] > 8).sum() > 0 and (k16["count"] == 0).sum() > 0
    for k in (1, 4, 8):      # prefixes of one another, bit for bit, and the same count
        _same(run[f"k{k}"], {**{f: k16[f][:k] for f in SLOTS}, "count": k16["count"]})
    for k in (4, 16):        # count = NULL changes no slot
        assert "count" not in run[f"k{k}_nocount"]
        _same(run[f"k{k}_nocount"], run[f"k{k}"], SLOTS)
    _same(run["k0"], k16, ("count",))                                       # the count-only form
    assert run["k0"]["t"].shape == (0, len(o))
    empty = np.arange(16)[:, None] >= k16["count"][None, :]
    assert np.array_equal(k16["prim"] == -1, empty)
    assert np.array_equal(k16["t"][empty], np.broadcast_to(tmax.astype(k16["t"].dtype), empty.shape)[empty])
    assert not k16["b1"][empty].any() and not k16["b2"][empty].any()


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------------------
def _rigid_entries(sc, case):
    """per entry of prim_order: a triangle whose instance transform is rigid (what the handle flattens into world space)"""
    _, M, _ = SR.geometry(sc, case)
    is_tri = SR.tables(sc, case)[1]
    lin = M[:, :3, :3]
    return is_tri & (np.abs(np.einsum("kij,klj->kil", lin, lin) - np.eye(3)).max((1, 2)) < 1e-9)


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("case", TR.CASES)
def test_chain(case, prec, workdir):
    """Plane s of (prim, b1, b2) goes into surface_at as it is and gives the point o + d t[s]; where rrt_trace_closest found the nearest hit on a rigid
    triangle, slot 0 names the same primitive"""
    sc = TR.scene(workdir, case)
    o, d, tmax, kinds, ref = _ref(case, prec, workdir)
    run = _run(case, prec, workdir)
    got = run["k8"]
    ext = SR.extent(sc)
    oq, dq = (o.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64)) if prec == RRT_F32 else (o, d)
    dev = 0.0
    for s in range(TR.K):
        f = got["prim"][s] >= 0
        if f.any():
            p = oq[f] + dq[f] * got["t"][s][f].astype(np.float64)[:, None]
            dev = max(dev, float(np.linalg.norm(run["planes"][s][f].astype(np.float64) - p, axis=1).max() / ext))
    _check_bars(prec, case, {"chain_p": dev})
    # rrt_trace_closest returns the LAST accepted hit (Q10): compared only where that is the nearest one, on non-marginal, non-tie rays
    cl = run["closest"]
    order = np.asarray(sc.prim_order(), np.int64)
    rigid = _rigid_entries(sc, case)
    bar_t = max(BARS["t"][0 if prec == RRT_F64 else 1], 4 * np.finfo(cl["t"].dtype).eps) * ext
    sel = (cl["prim"] >= 0) & (ref["count"] > 0) & ~ref["marginal"] & ~np.isin(kinds, ("edge", "vertex"))
    sel[sel] &= rigid[cl["prim"][sel]] & (np.abs(cl["t"][sel].astype(np.float64) - ref["t"][0][sel]) <= bar_t)
    # (f64 handles keep rigid instances too and replay the reference's ray transform: their t is the object-space one of a re-normalised direction, Q15,
    # which differs from the world t by the 6e-8 the float32-rounded directions are off unit length - few rays of the instanced scenes qualify there)
    assert sel.sum() > (200 if case in ("cfg5", "hand_closed") or prec == RRT_F32 else 0)
    assert np.array_equal(order[cl["prim"][sel]], order[got["prim"][0][sel]])
    same_entry = cl["prim"][sel] == got["prim"][0][sel]
    bits = [float((cl[a][sel][same_entry] == got[b][0][sel][same_entry]).mean()) for a, b in (("t", "t"), ("u", "b1"), ("v", "b2"))]
    print(f"{case} {_name(prec)}: {int(sel.sum())} rays where rrt_trace_closest found the nearest hit; bitwise equal t {100 * bits[0]:.1f} %, u {100 * bits[1]:.1f} %, "
          f"v {100 * bits[2]:.1f} % (not asserted: the two calls contract differently)")


# ---- inside, thickness and the signed field -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
def test_inside_and_signed_field(prec, workdir):
    sc = TR.scene(workdir, "hand_closed")
    ext = SR.extent(sc)
    rng = np.random.default_rng(31)
    p = np.concatenate([rng.random((150, 3)), TR.TET_V[0] + rng.random((150, 3)) * 0.6, rng.random((3000, 3)) * [8.0, 3.5, 3.5] - [1.0, 0.75, 0.75]])
    p = p.astype(np.float32).astype(np.float64)
    inside, dist = TR.hand_inside(p)
    p, inside = p[dist >= 1e-3 * ext][:500], inside[dist >= 1e-3 * ext][:500]
    assert len(p) == 500 and 50 < inside.sum() < 450
    r = Renderer(sc, 0, prec)
    assert np.array_equal(r.inside(p), inside)
    # thickness along +x through both solids: 1 in the cube, and x from 4 to 6 - y - z in the tetrahedron
    th = r.thickness(np.array([[-1, 0.25, 0.5]]), np.array([[1.0, 0, 0]]), np.array([np.inf]))
    assert th.tolist() == [1.0 + 1.25]
    lo, hi, res = (-0.5, -0.5, -0.5), (6.5, 2.5, 2.5), (14, 6, 6)      # cell centres at quarters: none nearer than 0.14 to a face
    ax = [lo[k] + (np.arange(n) + 0.5) * ((hi[k] - lo[k]) / n) for k, n in enumerate(res)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    cells = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    cin, cdist = TR.hand_inside(cells)
    assert (cdist >= 1e-3 * ext).all() and cin.sum() > 3
    unsigned = r.distance_field(lo, hi, res)
    signed = r.distance_field(lo, hi, res, signed=True)
    direct = r.nearest(cells)["dist"].reshape(res[2], res[1], res[0])
    r.close()
    assert np.array_equal(unsigned.view(np.uint8), direct.view(np.uint8)) and (unsigned > 0).all()      # the default is bit for bit what it was
    assert np.array_equal(signed, np.where(cin.reshape(unsigned.shape), -unsigned, unsigned))


# ---- invariances ----------------------------------------------------------------------------------------------------------------------------------------------------
def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_trace_all(r, o, d, tmax, k, bary=True, count=True):
    import torch
    m = len(tmax)
    cols = [_torch(np.asarray(a, r.dtype)) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
    tdt = torch.float32 if r.dtype == np.float32 else torch.float64
    outs = dict(t=torch.full((k, m), 3.5, dtype=tdt, device="cuda:0"), prim=torch.full((k, m), 35, dtype=torch.int32, device="cuda:0"))
    if bary: outs.update(b1=torch.full((k, m), 3.5, dtype=tdt, device="cuda:0"), b2=torch.full((k, m), 3.5, dtype=tdt, device="cuda:0"))
    if count: outs["count"] = torch.full((m,), 35, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    r.trace_all_device([c.data_ptr() for c in cols], m, {f: t.data_ptr() for f, t in outs.items()}, k)
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in outs.items()}
    if count: res["count"] = res["count"].view(np.uint32)
    return res


@pytest.mark.gpu
@PRECS
def test_invariances(prec, workdir):
    """Bit for bit, on the scaled scene (a kept instance: the grown node boxes)"""
    case = "scaled"
    sc = TR.scene(workdir, case)
    o, d, tmax, _, _ = _ref(case, prec, workdir)
    m = len(o)
    assert m == 4097 + 65
    r = Renderer(sc, 0, prec)
    frame0 = r.render()
    full = r.trace_all(o, d, tmax, k=TR.K)
    assert (full["count"] > 0).mean() > 0.5
    # host and device memory; device outputs pre-filled with 3.5 / 35 are overwritten, empty slots and rays without a hit included
    _same(full, _device_trace_all(r, o, d, tmax, TR.K))
    # b1 = b2 = NULL and count = NULL change no other array
    _same(_device_trace_all(r, o, d, tmax, TR.K, bary=False), full, ("t", "prim", "count"))
    _same(_device_trace_all(r, o, d, tmax, TR.K, count=False), full, SLOTS)
    # host outputs pre-filled are overwritten
    rays, out, arrs, cols = _host_io(m, r.dtype, prec, k=TR.K)
    for j, a in enumerate((o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)): cols[j][:] = a
    assert A.lib().rrt_trace_all(r._h, C.byref(rays), m, C.byref(out)) == A.RRT_OK
    _same(arrs, full)
    # batches of 1, 63, 64, 65 and 4 097 rays against slices of the large batch
    for n, at in ((1, 0), (1, 777), (63, 0), (64, 100), (65, 31), (4097, 0), (4097, 65)):
        _same(r.trace_all(o[at:at + n], d[at:at + n], tmax[at:at + n], k=TR.K), {f: (v[at:at + n] if f == "count" else v[:, at:at + n]) for f, v in full.items()})
    # a small max_paths cuts the rays into many passes
    r.set_option("max_paths", 64)
    _same(r.trace_all(o, d, tmax, k=TR.K), full)
    r.close()
    # a frame rendered before and after the call is the same frame
    r = Renderer(sc, 0, prec)
    r.trace_all(o, d, tmax, k=TR.K); r.trace_all(o, d, tmax, k=0)
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
    rays, out, arrs, cols = _host_io(4, rt.dtype, prec)

    def refused(rc, substr, code=A.RRT_EINVAL):
        assert rc == code and substr in lib.rrt_last_error(), lib.rrt_last_error()
        _untouched(arrs)

    _struct_refusals(lib, rt._h, rays, out, refused)
    bad = A.Rays.from_buffer_copy(rays); bad.precision = other
    refused(lib.rrt_trace_all(rt._h, C.byref(bad), 4, C.byref(out)), b"ray precision must match the handle")
    bad = A.MultiHits.from_buffer_copy(out); bad.precision = other
    refused(lib.rrt_trace_all(rt._h, C.byref(rays), 4, C.byref(bad)), b"output precision must match the handle")
    refused(lib.rrt_trace_all(None, C.byref(rays), 4, C.byref(out)), b"null handle")
    # a sphere-only scene
    refused(lib.rrt_trace_all(rs._h, C.byref(rays), 4, C.byref(out)), b"no triangle entry", A.RRT_EUNSUP)
    with pytest.raises(RrtUnsupported, match="no triangle entry"):
        rs.trace_all(np.zeros((4, 3)), np.ones((4, 3)), np.full(4, np.inf))
    # a frame in flight
    W, H = tri.resolution
    film = torch.zeros((H, W, 4), dtype=torch.float32 if prec == RRT_F32 else torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rt.render_bands_begin(0, 1, film.data_ptr())
    refused(lib.rrt_trace_all(rt._h, C.byref(rays), 4, C.byref(out)), b"a frame is in flight")
    rt.render_end()
    assert lib.rrt_trace_all(rt._h, C.byref(rays), 4, C.byref(out)) == A.RRT_OK and (arrs["prim"] != 35).all() and (arrs["count"] != 35).all()
    with pytest.raises(RrtError):
        rt.trace_all(np.zeros((4, 3)), np.ones((4, 3)), np.full(4, np.inf), k=17)
    rs.close(); rt.close()
