"""Mutual visibility of two point sets as a packed bit matrix (rrt_visibility, include/rrt.h).

CPU tests: the export and prototype (header, library, A.PROTOTYPES), the ABI version, the C layout of rrt_vis_params and rrt_vis_out, the refusals that
need no device, tools/visibility_check.cpp - the walk on the CPU against the scan - built and run, the numpy reference (tests/visibility_reference.py)
on its own - at most 2 % of the 9 170 pairs of every case are marginal (the project's bar for rrt_trace_all's rays) and between 5 % and 95 % are
visible -, and the hand expectations held equal to the brute force.

GPU tests, in both precisions:
  test_by_hand        a unit cube and a tetrahedron: a point inside the cube, two points across the gap, a point behind the tetrahedron; the FACING_A,
                      FACING_B and DIRECTIONS variants; expectations by hand, exact
  test_is_trace_all   five scenes, 70 x 131 pairs: every bit equals count == 0 of rrt_trace_all (k = 0) over the segments built in numpy in the
                      handle's type - no band, no exclusion -, with and without skip_a; count is the popcount of the row, the padding bits are 0
  test_is_the_scan    against the f64 brute force: equal on every non-marginal pair
  test_variants       DIRECTIONS, FACING_A / _B / both, PAIRS against the diagonal, skip_b, dead points, coincident points - bit for bit against the same
                      rrt_trace_all construction
  test_tree_shapes    deep (global stack), lopsided and fat-leaf trees against the same construction on the same shape
  test_invariances    n_b in {1, 63, 64, 65, 131}, max_paths cutting the matrix into launches, host against device memory, count == NULL, the frame
                      before and after
  test_refusals       a frame in flight, a scene with no triangle entry, a wrong precision

Every comparison on the device is exact: there are no bars. Measured (profiles/visibility_gpu_tests.txt): the marginal share of the 9 170 pairs is
0.0010 / 0.0003 / 0.0003 / 0.0002 / 0.0001 in fp32 for cfg5 / rigid / scaled / rigid_sphere / hand_closed and 0 in f64, the visible share runs from
0.11 (cfg5) to 0.53 (rigid), and on an MI355X none of the marginal pairs differed from the brute force either.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bvh_shapes as B
import surface_reference as SR
import trace_all_reference as TR
import visibility_reference as VR
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, RrtUnsupported, Scene, scenes, unpack_visibility
from rs_ray_toy_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
CSRC = os.path.join(ROOT, "rs_ray_toy_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PRECS = pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
PARAM_MEMBERS = ["mode", "b_kind", "flags", "pad", "offset_a", "offset_b", "skip_a", "skip_b"]
OUT_MEMBERS = ["mem", "pad", "bits", "count"]


def _name(prec):
    return "f64" if prec == RRT_F64 else "f32"


def _dtype(prec):
    return np.float64 if prec == RRT_F64 else np.float32


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    return None if m is None else [a.strip() for a in m.group(1).split(",")]


def test_exports_header_prototypes_and_layout(tmp_path):
    lib = A.lib()
    assert hasattr(lib, "rrt_visibility"), "librrt.so does not export rrt_visibility"
    args = _header_prototype("rrt_visibility")
    assert args is not None, "include/rrt.h does not declare rrt_visibility"
    assert "rrt_visibility" in A.PROTOTYPES
    restype, argtypes = A.PROTOTYPES["rrt_visibility"]
    assert restype is C.c_int and len(argtypes) == len(args) == 7
    assert argtypes[1] is C.POINTER(A.Points) and "rrt_points" in args[1] and argtypes[2] is C.c_size_t and "size_t" in args[2]
    assert argtypes[3] is C.POINTER(A.Points) and "rrt_points" in args[3] and argtypes[4] is C.c_size_t and "size_t" in args[4]
    assert argtypes[5] is C.POINTER(A.VisParams) and "rrt_vis_params" in args[5] and argtypes[6] is C.POINTER(A.VisOut) and "rrt_vis_out" in args[6]
    assert "#define RRT_ABI_VERSION 11" in " ".join(open(HEADER).read().split())
    assert (A.RRT_VIS_MATRIX, A.RRT_VIS_PAIRS, A.RRT_VIS_POINTS, A.RRT_VIS_DIRECTIONS, A.RRT_VIS_FACING_A, A.RRT_VIS_FACING_B) == (0, 1, 0, 1, 1, 2)
    # the C layout: an offsetof printer
    assert [n for n, _ in A.VisParams._fields_] == PARAM_MEMBERS and [n for n, _ in A.VisOut._fields_] == OUT_MEMBERS
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
           'printf("p.size %zu\\n", sizeof(rrt_vis_params));', 'printf("o.size %zu\\n", sizeof(rrt_vis_out));',
           'printf("enums %d %d %d %d %d %d\\n", RRT_VIS_MATRIX, RRT_VIS_PAIRS, RRT_VIS_POINTS, RRT_VIS_DIRECTIONS, RRT_VIS_FACING_A, RRT_VIS_FACING_B);']
    src += [f'printf("p.{f} %zu\\n", offsetof(rrt_vis_params, {f}));' for f in PARAM_MEMBERS]
    src += [f'printf("o.{f} %zu\\n", offsetof(rrt_vis_out, {f}));' for f in OUT_MEMBERS]
    src.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c11", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = dict(line.split(None, 1) for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(out["p.size"]) == C.sizeof(A.VisParams) and int(out["o.size"]) == C.sizeof(A.VisOut)
    assert out["enums"].split() == ["0", "1", "0", "1", "1", "2"]
    for f in PARAM_MEMBERS:
        assert int(out["p." + f]) == getattr(A.VisParams, f).offset, f
    for f in OUT_MEMBERS:
        assert int(out["o." + f]) == getattr(A.VisOut, f).offset, f


class _Io:
    """Host arrays of n_a x n_b points with normals, pre-filled outputs, and the structs over them"""

    def __init__(self, n_a, n_b, dtype, prec, mem=A.RRT_MEM_HOST):
        self.cols = {s: [np.zeros(n, dtype) for _ in range(6)] for s, n in (("a", n_a), ("b", n_b))}
        for s in "ab":
            self.cols[s][5][:] = 1.0                                   # normals: the z axis
        self.cols["b"][0][:] = 1.0                                     # b = a + x
        self.skip = {"a": np.full(n_a, -1, np.int32), "b": np.full(n_b, -1, np.int32)}
        self.a = A.Points(mem, prec, *[c.ctypes.data for c in self.cols["a"]], None)
        self.b = A.Points(mem, prec, *[c.ctypes.data for c in self.cols["b"]], None)
        self.bits = np.full((n_a, (n_b + 63) // 64), 35, np.uint64)
        self.count = np.full(n_a, 35, np.uint32)
        self.prm = A.VisParams(A.RRT_VIS_MATRIX, A.RRT_VIS_POINTS, 0, 0, 0.0, 0.0, None, None)
        self.out = A.VisOut(mem, 0, self.bits.ctypes.data, self.count.ctypes.data)

    def untouched(self):
        assert (self.bits == 35).all() and (self.count == 35).all()


def _struct_refusals(lib, h, io, refused, n_a=4, n_b=5):
    """The refusals that are decided on the structs alone, with handle h (None: a NULL handle, looked at last)"""
    ref = lambda x: None if x is None else C.byref(x)
    call = lambda a=io.a, b=io.b, prm=io.prm, out=io.out, na=n_a, nb=n_b: lib.rrt_visibility(h, ref(a), na, ref(b), nb, ref(prm), ref(out))
    pts = lambda p, **kw: _with(A.Points, p, **kw)
    prm = lambda **kw: _with(A.VisParams, io.prm, **kw)
    out = lambda **kw: _with(A.VisOut, io.out, **kw)
    refused(call(a=None), b"point description a")
    refused(call(b=None), b"point description b")
    refused(call(out=None), b"rrt_vis_out")
    refused(call(out=out(bits=None)), b"null bits")
    for member in ("px", "py", "pz"):
        refused(call(a=pts(io.a, **{member: None})), b"coordinate array of a")
        refused(call(b=pts(io.b, **{member: None})), b"coordinate array of b")
    refused(call(a=pts(io.a, ny=None)), b"normals of a")
    refused(call(b=pts(io.b, nz=None)), b"normals of b")
    refused(call(a=pts(io.a, mem=7)), b"bad mem")
    refused(call(b=pts(io.b, mem=A.RRT_MEM_DEVICE)), b"same memory kind")
    refused(call(out=out(mem=A.RRT_MEM_DEVICE)), b"same memory kind")
    refused(call(na=0), b"n_a and n_b must be > 0")
    refused(call(nb=0), b"n_a and n_b must be > 0")
    refused(call(na=1 << 31), b"n_a or n_b too large")
    refused(call(nb=1 << 31), b"n_a or n_b too large")
    refused(call(na=(1 << 20) + 1, nb=1 << 20), b"n_a * n_b too large")
    refused(call(prm=prm(mode=2)), b"bad mode")
    refused(call(prm=prm(b_kind=-1)), b"bad b_kind")
    refused(call(prm=prm(flags=4)), b"bad flags")
    refused(call(prm=prm(offset_a=float("nan"))), b"offset_a must be finite")
    refused(call(prm=prm(offset_b=float("inf"))), b"offset_b must be finite")
    no_na, no_nb = pts(io.a, nx=None, ny=None, nz=None), pts(io.b, nx=None, ny=None, nz=None)
    refused(call(a=no_na, prm=prm(offset_a=0.5)), b"offset_a needs the normals of a")
    refused(call(a=no_na, prm=prm(flags=A.RRT_VIS_FACING_A)), b"RRT_VIS_FACING_A needs the normals of a")
    refused(call(b=no_nb, prm=prm(offset_b=0.5)), b"offset_b needs the normals of b")
    refused(call(b=no_nb, prm=prm(flags=A.RRT_VIS_FACING_B)), b"RRT_VIS_FACING_B needs the normals of b")
    dirs = dict(b_kind=A.RRT_VIS_DIRECTIONS)
    refused(call(prm=prm(**dirs)), b"RRT_VIS_DIRECTIONS: b is a set of directions")
    refused(call(b=no_nb, prm=prm(offset_b=0.5, **dirs)), b"RRT_VIS_DIRECTIONS: offset_b must be 0")
    refused(call(b=no_nb, prm=prm(flags=A.RRT_VIS_FACING_B, **dirs)), b"RRT_VIS_DIRECTIONS: RRT_VIS_FACING_B")
    refused(call(b=no_nb, prm=prm(skip_b=io.skip["b"].ctypes.data, **dirs)), b"RRT_VIS_DIRECTIONS: skip_b must be NULL")
    refused(call(prm=prm(mode=A.RRT_VIS_PAIRS), out=out(count=None)), b"RRT_VIS_PAIRS: n_b must equal n_a")
    refused(call(prm=prm(mode=A.RRT_VIS_PAIRS), nb=n_a), b"RRT_VIS_PAIRS: count must be NULL")
    return call, prm, out, no_na, no_nb


def _with(cls, struct, **members):
    s = cls.from_buffer_copy(struct)
    for k, v in members.items():
        setattr(s, k, v)
    return s


def test_refusals_that_need_no_device():
    """The structs are checked before the handle is looked at: every call here has a NULL handle, and only the last ones get as far as saying so"""
    lib = A.lib()
    io = _Io(4, 5, np.float64, RRT_F64)

    def refused(rc, substr):
        assert rc == A.RRT_EINVAL and substr in lib.rrt_last_error(), lib.rrt_last_error()
        io.untouched()

    call, prm, out, no_na, no_nb = _struct_refusals(lib, None, io, refused)
    # legal forms get as far as the handle: NULL params, count == NULL, no normals, DIRECTIONS, PAIRS, the flags, skip arrays
    for kw in (dict(prm=None), dict(out=out(count=None)), dict(a=no_na, b=no_nb), dict(b=no_nb, prm=prm(b_kind=A.RRT_VIS_DIRECTIONS, flags=A.RRT_VIS_FACING_A, offset_a=0.5)),
               dict(prm=prm(mode=A.RRT_VIS_PAIRS), out=out(count=None), nb=4), dict(prm=prm(flags=3, offset_a=0.5, offset_b=-0.5)),
               dict(prm=prm(skip_a=io.skip["a"].ctypes.data, skip_b=io.skip["b"].ctypes.data)), dict(na=1 << 20, nb=1 << 20)):
        refused(call(**kw), b"null handle")


def test_visibility_check_on_the_golden_scenes():
    """tools/visibility_check.cpp: the walk of k_visibility on the CPU against the scan, on the golden scenes, a single-leaf root and a 96-deep chain (no
    sanitizer here: the program builds with -fsanitize=address,undefined as it stands)"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "visibility_check"])
    paths = [os.path.join(GOLDEN, p, "scene.json") for p in ("", "fuzz416_43", "fuzz508_96")]
    run = subprocess.run([os.path.join(ROOT, "build", "visibility_check", "visibility_check")] + paths, capture_output=True, text=True, timeout=120)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stderr
    assert "visibility_check: ok" in run.stdout and "96-deep chain" in run.stdout and "single-leaf root" in run.stdout


_refs = {}


def _seg(case, prec, workdir, **kw):
    """The case's pairs as segments in the handle's type, with the case's offsets unless the caller says otherwise"""
    P = VR.pairs(TR.scene(workdir, case), case)
    kw.setdefault("na", P["na"]); kw.setdefault("nb", None if kw.get("directions") else P["nb"])
    kw.setdefault("offset_a", P["offset"]); kw.setdefault("offset_b", 0.0 if kw.get("directions") else P["offset"])
    return P, VR.segments(P["a"], kw.pop("b", P["b"]), _dtype(prec), **kw)


def _ref(case, prec, workdir):
    key = (case, prec)
    if key not in _refs:
        P, seg = _seg(case, prec, workdir)
        ref = VR.brute(TR.scene(workdir, case), case, seg, prec == RRT_F32)
        for a in ref.values(): a.setflags(write=False)
        _refs[key] = (P, seg, ref)
    return _refs[key]


@PRECS
@pytest.mark.parametrize("case", TR.CASES)
def test_reference_margins(case, prec, workdir):
    """The reference alone: at most 2 % of the 9 170 pairs are marginal at the precision's band, and between 5 % and 95 % are visible"""
    P, seg, ref = _ref(case, prec, workdir)
    assert ref["visible"].shape == (70, 131) and ref["visible"].size == 9170
    assert (P["ent_b"][-30:] == -1).all() and (P["ent_b"][:-30] >= 0).all() and (P["ent_a"] >= 0).all()
    marginal, visible = float(ref["marginal"].mean()), float(ref["visible"].mean())
    print(f"{case} {_name(prec)}: marginal share {marginal:.4f}, visible share {visible:.3f}")
    assert marginal <= 0.02, (case, marginal)
    assert 0.05 <= visible <= 0.95, (case, visible)


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------------------------------
# trace_all_reference.HAND_TRIS: the unit cube and the tetrahedron (4,0,0), (6,0,0), (4,2,0), (4,0,2) (face x = 4 and the slanted face x + y + z = 6).
# A: a point inside the cube, one in the gap next to the cube, one behind the tetrahedron. B: a point in the gap next to the tetrahedron, one on the far
# side of the cube, one high above the gap (its segments to the second and third A pass over both solids: x + y + z >= 6 all along the third's).
HAND_A = np.array([[0.5, 0.25, 0.5], [1.5, 0.25, 0.5], [7.0, 0.25, 0.5]])
HAND_B = np.array([[3.5, 0.25, 0.5], [-1.0, 0.25, 0.5], [3.5, 0.25, 5.0]])
HAND_NA = np.array([[1.0, 0, 0.5], [1.0, 0, 1.0], [0.5, 0, -1.0]])      # (none of unit length)
HAND_NB = np.array([[-1.0, 0, 0], [1.0, 0, 0], [0, 0, 1.0]])
HAND_DIRS = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 0, 1.0]])
HAND = {      # variant: (keyword arguments of Renderer.visibility beyond a, b; the matrix)
    # the inside point sees nothing; across the gap: yes; through the cube: no; behind the tetrahedron to in front of it: no; over the top: yes
    "plain": (dict(), [[0, 0, 0], [1, 0, 1], [0, 0, 1]]),
    "normals_unused": (dict(na=HAND_NA, nb=HAND_NB), [[0, 0, 0], [1, 0, 1], [0, 0, 1]]),
    # the third A looks down: the point above it is behind its surface
    "facing_a": (dict(na=HAND_NA, nb=HAND_NB, facing_a=True), [[0, 0, 0], [1, 0, 1], [0, 0, 0]]),
    # the third B faces up (+z): both segments arrive from below, on its back
    "facing_b": (dict(na=HAND_NA, nb=HAND_NB, facing_b=True), [[0, 0, 0], [1, 0, 0], [0, 0, 0]]),
    "facing_both": (dict(na=HAND_NA, nb=HAND_NB, facing_a=True, facing_b=True), [[0, 0, 0], [1, 0, 0], [0, 0, 0]]),
    # directions +x, -x, +z: from the gap +x runs into the tetrahedron and -x into the cube; from behind the tetrahedron +x and +z are free
    "directions": (dict(directions=True), [[0, 0, 0], [0, 0, 1], [1, 0, 1]]),
    # the third A looks down and a little towards +x: +z is behind it
    "directions_facing_a": (dict(na=HAND_NA, directions=True, facing_a=True), [[0, 0, 0], [0, 0, 1], [1, 0, 0]]),
}


def _hand_b(kw):
    return HAND_DIRS if kw.get("directions") else HAND_B


def test_hand_expectations_are_the_brute_force(workdir):
    """What test_by_hand writes down is what the numpy brute force finds on the hand-built solids, in both types, with no marginal pair"""
    sc = TR.scene(workdir, "hand_closed")
    for name, (kw, expected) in HAND.items():
        flags = (VR.FACING_A if kw.get("facing_a") else 0) | (VR.FACING_B if kw.get("facing_b") else 0)
        for dtype in (np.float64, np.float32):
            seg = VR.segments(HAND_A, _hand_b(kw), dtype, na=kw.get("na"), nb=kw.get("nb"), flags=flags, directions=bool(kw.get("directions")))
            ref = VR.brute(sc, "hand_closed", seg, dtype is np.float32)
            assert ref["visible"].astype(int).tolist() == expected, (name, dtype)
            assert not ref["marginal"].any(), (name, dtype)


@pytest.mark.gpu
@PRECS
def test_by_hand(prec, workdir):
    sc = TR.scene(workdir, "hand_closed")
    r = Renderer(sc, 0, prec)
    for name, (kw, expected) in HAND.items():
        got = r.visibility(HAND_A, _hand_b(kw), **kw)
        assert got["bits"].shape == (3, 1) and got["bits"].dtype == np.uint64
        assert unpack_visibility(got["bits"], 3).astype(int).tolist() == expected, name
        assert got["count"].tolist() == [sum(row) for row in expected], name
        assert np.array_equal(got["bits"], VR.pack(np.array(expected, bool))), name      # (the padding bits are 0)
    sky = r.sky_view(HAND_A, HAND_NA, HAND_DIRS)
    r.close()
    assert sky.tolist() == [0.0, 1 / 3, 1 / 3]


# ---- is rrt_trace_all ---------------------------------------------------------------------------------------------------------------------------------------------
def _by_trace_all(r, seg, skip=None):
    """The call's bits by its definition: the segments through rrt_trace_all with k = 0, visible iff count == 0 (and the untraced verdicts as they are)"""
    live = seg["verdict"] == VR.TRACE
    count = r.trace_all(seg["o"][live], seg["d"][live], seg["tmax"][live], k=0, skip_prim=None if skip is None else np.asarray(skip, np.int32)[live])["count"]
    vis = seg["verdict"] == VR.YES
    vis[live] = count == 0
    return vis.reshape(seg["shape"])


def _check_matrix(got, expected, n_b, count=True):
    """bits bit for bit - the padding included - and count = popcount(row)"""
    assert got["bits"].dtype == np.uint64 and got["bits"].shape == (len(expected), (n_b + 63) // 64)
    assert np.array_equal(unpack_visibility(got["bits"], n_b), expected)
    assert np.array_equal(got["bits"], VR.pack(expected))
    if count:
        assert got["count"].dtype == np.uint32 and np.array_equal(got["count"], expected.sum(1))


_runs = {}


def _run(case, prec, workdir):
    key = (case, prec)
    if key not in _runs:
        sc = TR.scene(workdir, case)
        P, seg, _ = _ref(case, prec, workdir)
        r = Renderer(sc, 0, prec)
        kw = dict(na=P["na"], nb=P["nb"], offset_a=P["offset"], offset_b=P["offset"])
        _runs[key] = dict(got=r.visibility(P["a"], P["b"], **kw), expected=_by_trace_all(r, seg),
                          got_skip=r.visibility(P["a"], P["b"], skip_a=P["ent_a"], **kw), expected_skip=_by_trace_all(r, seg, skip=P["ent_a"][seg["ii"]]))
        r.close()
    return _runs[key]


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("case", TR.CASES)
def test_is_trace_all(case, prec, workdir):
    """Every one of the 9 170 bits is rrt_trace_all's count == 0 over the segment built by the header's formulas: no band, no exclusion"""
    run = _run(case, prec, workdir)
    assert run["expected"].size == 9170 and 0.05 <= run["expected"].mean() <= 0.95
    print(f"{case} {_name(prec)}: {int(run['expected'].sum())} of 9170 pairs visible, {int(run['expected_skip'].sum())} with skip_a")
    _check_matrix(run["got"], run["expected"], VR.N_B)
    _check_matrix(run["got_skip"], run["expected_skip"], VR.N_B)


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("case", TR.CASES)
def test_is_the_scan(case, prec, workdir):
    """Against the f64 brute force: equal on every non-marginal pair; the marginal ones are printed (test_reference_margins bounds their share)"""
    _, _, ref = _ref(case, prec, workdir)
    got = unpack_visibility(_run(case, prec, workdir)["got"]["bits"], VR.N_B)
    strong = ~ref["marginal"]
    differ = got != ref["visible"]
    print(f"{case} {_name(prec)}: {int(strong.sum())} pairs compared exactly, {int((~strong).sum())} marginal of which {int((differ & ~strong).sum())} differ: "
          f"{np.argwhere(~strong).tolist()}")
    assert not (differ & strong).any(), np.argwhere(differ & strong).tolist()


# ---- variants -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
def test_variants(prec, workdir):
    case = "scaled"
    sc = TR.scene(workdir, case)
    P = VR.pairs(sc, case)
    # DIRECTIONS: the B points as directions (tmax = inf), without and with FACING_A - on cfg5, which is open to the sky (the instanced scenes are
    # closed rooms: every unbounded ray is blocked there, which the second round holds as well)
    for open_case in ("cfg5", case):
        Q = VR.pairs(TR.scene(workdir, open_case), open_case)
        r = Renderer(TR.scene(workdir, open_case), 0, prec)
        for flags in (0, VR.FACING_A):
            _, seg = _seg(open_case, prec, workdir, directions=True, flags=flags)
            expected = _by_trace_all(r, seg)
            assert 0.02 < expected.mean() < 0.98 if open_case == "cfg5" else not expected.any()
            _check_matrix(r.visibility(Q["a"], Q["b"], na=Q["na"], offset_a=Q["offset"], directions=True, facing_a=bool(flags)), expected, VR.N_B)
            if flags:
                assert np.array_equal(r.sky_view(Q["a"], Q["na"], Q["b"], offset=Q["offset"]), expected.sum(1) / VR.N_B)
        if open_case == "cfg5":      # a zero or non-finite direction is a dead column; the others are unchanged
            dirs = Q["b"].copy(); dirs[7] = 0.0; dirs[70, 0] = np.inf
            plain_dirs = unpack_visibility(r.visibility(Q["a"], Q["b"], directions=True)["bits"], VR.N_B)
            dead = plain_dirs.copy(); dead[:, [7, 70]] = False
            assert plain_dirs[:, [7, 70]].any()
            _check_matrix(r.visibility(Q["a"], dirs, directions=True), dead, VR.N_B)
        r.close()
    r = Renderer(sc, 0, prec)
    # FACING_A, FACING_B and both: a pair that fails is 0 and the others are the plain call's
    plain = _by_trace_all(r, _seg(case, prec, workdir)[1])
    for flags in (VR.FACING_A, VR.FACING_B, VR.FACING_A | VR.FACING_B):
        _, seg = _seg(case, prec, workdir, flags=flags)
        expected = _by_trace_all(r, seg)
        failed = seg["verdict"].reshape(seg["shape"]) == VR.NO
        assert 0.1 < failed.mean() < 0.95 and not expected[failed].any() and np.array_equal(expected[~failed], plain[~failed])
        got = r.visibility(P["a"], P["b"], na=P["na"], nb=P["nb"], offset_a=P["offset"], offset_b=P["offset"], facing_a=bool(flags & 1), facing_b=bool(flags & 2))
        _check_matrix(got, expected, VR.N_B)
    # PAIRS is the diagonal of the MATRIX call over n_a == n_b == 131
    kw = dict(na=P["nb"], nb=P["nb"][::-1], offset_a=P["offset"], offset_b=P["offset"])
    matrix = r.visibility(P["b"], P["b"][::-1], **kw)
    diag = np.diagonal(unpack_visibility(matrix["bits"], VR.N_B))
    got = r.visibility(P["b"], P["b"][::-1], pairs=True, **kw)
    assert got["count"] is None and got["bits"].shape == (3,) and 5 < diag.sum() < 126
    assert np.array_equal(got["bits"], VR.pack(diag))
    seg = VR.segments(P["b"], P["b"][::-1], _dtype(prec), na=P["nb"], nb=P["nb"][::-1], offset_a=P["offset"], offset_b=P["offset"], pairs=True)
    assert np.array_equal(_by_trace_all(r, seg), diag)
    # dead points (a NaN coordinate, a zero normal) give zero rows and columns; the rest is unchanged
    a, na, b, nb = (P[k].copy() for k in ("a", "na", "b", "nb"))
    a[3, 1] = np.nan; na[9] = 0.0; b[64, 2] = np.nan; nb[130] = 0.0; na[11, 0] = np.inf
    got = r.visibility(a, b, na=na, nb=nb, offset_a=P["offset"], offset_b=P["offset"])
    expected = plain.copy()
    expected[[3, 9, 11], :] = False; expected[:, [64, 130]] = False
    _check_matrix(got, expected, VR.N_B)
    assert got["count"][[3, 9, 11]].tolist() == [0, 0, 0] and plain[[3, 9, 11]].any() and plain[:, [64, 130]].any()
    # coincident points: nothing lies between them - visible without a FACING flag, not visible with one
    same = r.visibility(P["a"], P["a"], pairs=True)
    assert np.array_equal(same["bits"], VR.pack(np.ones(VR.N_A, bool)))
    same = r.visibility(P["a"], P["a"], na=P["na"], nb=P["na"], facing_a=True, pairs=True)
    assert not same["bits"].any()
    same = r.visibility(P["a"], P["a"], na=P["na"], nb=P["na"], facing_b=True)
    assert not np.diagonal(unpack_visibility(same["bits"], VR.N_A)).any()
    r.close()
    # skip_b on the hand-built solids: B on the cube face x = 1 with offset_b = 0 and its own entry skipped - seen from in front and from inside the cube
    # (only the skipped face lies on that segment), not seen from behind the cube; a NULL skip_a beside it, and skip_a naming the same entry
    sc = TR.scene(workdir, "hand_closed")
    idx = TR.hand_entries(sc)
    r = Renderer(sc, 0, prec)
    a3 = np.array([[2.0, 0.5, 0.75], [0.5, 0.25, 0.5], [-1.0, 0.25, 0.5]])
    b1 = np.array([[1.0, 0.25, 0.5]])
    own = np.array([idx["X1b"]], np.int32)
    got = r.visibility(a3, b1, nb=np.array([[1.0, 0, 0]]), offset_b=0.0, skip_b=own)
    assert unpack_visibility(got["bits"], 1)[:, 0].tolist() == [True, True, False] and got["count"].tolist() == [1, 1, 0]
    for i in range(3):      # against the construction: rrt_trace_all with skip_prim
        seg = VR.segments(a3[i:i + 1], b1, _dtype(prec), nb=np.array([[1.0, 0, 0]]))
        assert _by_trace_all(r, seg, skip=own)[0, 0] == [True, True, False][i]
    got = r.visibility(b1, a3, skip_a=own)      # the same segments the other way round
    assert unpack_visibility(got["bits"], 3)[0].tolist() == [True, True, False]
    got = r.visibility(a3, b1, skip_a=np.array([idx["X0b"], -1, idx["X0b"]], np.int32), skip_b=own)      # both skips: the cube's far face removed too
    assert unpack_visibility(got["bits"], 1)[:, 0].tolist() == [True, True, True]
    r.close()


# ---- tree shapes ----------------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = ("chain_first_9", "chain_alt_96", "comb_96", "fat_2048", "builder")
_shape_base = {}


def _shape(name, workdir):
    """(the shaped scene, its heightfield, the heightfield's name) as test_trace_all.test_tree_shapes builds them"""
    n = 48 if name.startswith("fat_") else 16      # fat_2048 needs more than 2 048 triangles
    hf = f"visibility_hf{n}"
    if n not in _shape_base:
        wd = os.path.join(workdir, hf)
        os.makedirs(wd, exist_ok=True)
        cfg, root = scenes.cfg4(wd, xres=32, yres=32, nsamp=5, max_depth=3, n=n)
        _shape_base[n] = Scene.loads(cfg, root, flags=RRT_FIXED_BVH if n > 16 else 0)
    base = _shape_base[n]
    if (name, n) not in _shape_base:
        _shape_base[(name, n)] = (base if name == "builder" else B.fat(base, int(name[4:])) if name.startswith("fat_") else B.comb(base, int(name.split("_")[1]))
                                  if name.startswith("comb_") else B.chain(base, int(name.split("_")[2]), name.split("_")[1]))
    return _shape_base[(name, n)], base, hf


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("name", SHAPES)
def test_tree_shapes(name, prec, workdir):
    """The walk is the definition on every tree: bit for bit the rrt_trace_all construction on the same shape (chain_alt_96 and comb_96 are deeper than
    64: the global stack)"""
    sh, base, hf = _shape(name, workdir)
    P = VR.pairs(base, hf)
    seg = VR.segments(P["a"], P["b"], _dtype(prec), na=P["na"], nb=P["nb"], offset_a=P["offset"], offset_b=P["offset"])
    r = Renderer(sh, 0, prec)
    expected = _by_trace_all(r, seg)
    got = r.visibility(P["a"], P["b"], na=P["na"], nb=P["nb"], offset_a=P["offset"], offset_b=P["offset"])
    r.close()
    print(f"{name} {_name(prec)}: {int(expected.sum())} of {expected.size} pairs visible")
    assert expected.any() and not expected.all()
    _check_matrix(got, expected, VR.N_B)


# ---- invariances ----------------------------------------------------------------------------------------------------------------------------------------------------
def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_visibility(r, P, count=True, fill=35):
    import torch
    cols = {k: [_torch(P[k][:, c].astype(r.dtype)) for c in range(3)] for k in ("a", "na", "b", "nb")}
    n_a, n_b = len(P["a"]), len(P["b"])
    bits = torch.full((n_a, (n_b + 63) // 64), fill, dtype=torch.int64, device="cuda:0")
    cnt = torch.full((n_a,), fill, dtype=torch.int32, device="cuda:0")
    ptrs = {k: tuple(c.data_ptr() for c in v) for k, v in cols.items()}
    ptrs["bits"] = bits.data_ptr()
    if count: ptrs["count"] = cnt.data_ptr()
    torch.cuda.synchronize()
    r.visibility_device(ptrs, n_a, n_b, offset_a=P["offset"], offset_b=P["offset"])
    torch.cuda.synchronize()
    return dict(bits=bits.cpu().numpy().view(np.uint64), count=cnt.cpu().numpy().view(np.uint32))


@pytest.mark.gpu
@PRECS
def test_invariances(prec, workdir):
    """Bit for bit, on the scaled scene (a kept instance: the grown node boxes)"""
    case = "scaled"
    sc = TR.scene(workdir, case)
    P = VR.pairs(sc, case)
    kw = dict(na=P["na"], offset_a=P["offset"], offset_b=P["offset"])
    r = Renderer(sc, 0, prec)
    frame0 = r.render()
    full = r.visibility(P["a"], P["b"], nb=P["nb"], **kw)
    vis = unpack_visibility(full["bits"], VR.N_B)
    assert 0.05 < vis.mean() < 0.95
    # n_b in {1, 63, 64, 65, 131}: the leading columns, and a window that starts elsewhere
    for n_b, at in ((1, 0), (1, 77), (63, 0), (64, 0), (64, 67), (65, 0), (65, 3), (131, 0)):
        _check_matrix(r.visibility(P["a"], P["b"][at:at + n_b], nb=P["nb"][at:at + n_b], **kw), vis[:, at:at + n_b], n_b)
    # host against device memory; pre-filled device outputs are overwritten, the padding included
    dev = _device_visibility(r, P)
    assert np.array_equal(dev["bits"], full["bits"]) and np.array_equal(dev["count"], full["count"])
    # count == NULL changes no bit, and the count plane is not touched
    dev = _device_visibility(r, P, count=False)
    assert np.array_equal(dev["bits"], full["bits"]) and (dev["count"] == 35).all()
    assert np.array_equal(r.visibility(P["a"], P["b"], nb=P["nb"], count=False, **kw)["bits"], full["bits"])
    # pre-filled host outputs are overwritten
    io = _Io(VR.N_A, VR.N_B, r.dtype, prec)
    for s, n in (("a", "na"), ("b", "nb")):
        for c in range(3):
            io.cols[s][c][:] = P[s][:, c]; io.cols[s][3 + c][:] = P[n][:, c]
    io.prm.offset_a = io.prm.offset_b = P["offset"]
    assert A.lib().rrt_visibility(r._h, C.byref(io.a), VR.N_A, C.byref(io.b), VR.N_B, C.byref(io.prm), C.byref(io.out)) == A.RRT_OK
    assert np.array_equal(io.bits, full["bits"]) and np.array_equal(io.count, full["count"])
    # a small max_paths cuts the 210 words into as many launches
    r.set_option("max_paths", 64)
    cut = r.visibility(P["a"], P["b"], nb=P["nb"], **kw)
    assert np.array_equal(cut["bits"], full["bits"]) and np.array_equal(cut["count"], full["count"])
    r.set_option("max_paths", 64 * 7)      # 7 words a launch: launches that end inside a row
    cut = r.visibility(P["a"], P["b"], nb=P["nb"], **kw)
    assert np.array_equal(cut["bits"], full["bits"]) and np.array_equal(cut["count"], full["count"])
    r.close()
    # a frame rendered before and after the call is the same frame
    r = Renderer(sc, 0, prec)
    r.visibility(P["a"], P["b"], nb=P["nb"], **kw); r.visibility(P["a"], P["a"], pairs=True)
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
    io = _Io(4, 5, rt.dtype, prec)

    def refused(rc, substr, code=A.RRT_EINVAL):
        assert rc == code and substr in lib.rrt_last_error(), lib.rrt_last_error()
        io.untouched()

    call, prm, out, no_na, no_nb = _struct_refusals(lib, rt._h, io, refused)
    # a wrong precision, of either set
    refused(call(a=_with(A.Points, io.a, precision=other), b=_with(A.Points, io.b, precision=other)), b"a precision must match the handle")
    refused(call(b=_with(A.Points, io.b, precision=other)), b"precision")
    # a scene with no triangle entry
    refused(lib.rrt_visibility(rs._h, C.byref(io.a), 4, C.byref(io.b), 5, None, C.byref(io.out)), b"no triangle entry", A.RRT_EUNSUP)
    with pytest.raises(RrtUnsupported, match="no triangle entry"):
        rs.visibility(np.zeros((4, 3)), np.ones((5, 3)))
    # a frame in flight
    W, H = tri.resolution
    film = torch.zeros((H, W, 4), dtype=torch.float32 if prec == RRT_F32 else torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rt.render_bands_begin(0, 1, film.data_ptr())
    refused(call(), b"a frame is in flight")
    rt.render_end()
    assert call() == A.RRT_OK and (io.bits < 32).all() and (io.count <= 5).all()
    with pytest.raises(RrtError):
        rt.visibility(np.zeros((4, 3)), np.ones((5, 3)), offset_a=1.0)      # an offset without normals
    rs.close(); rt.close()
