"""Surface records (rrt_surface_rays, rrt_surface_at, include/rrt.h).

CPU tests: the exports and prototypes, the C layout of rrt_surface and rrt_sites, the refusals that need no device, and the numpy reference
(tests/surface_reference.py) checking itself - its restatement of the sites form at the oracle's (prim, u, v) gives the oracle's own p and n.

GPU tests, in both precisions, on five scenes (surface_reference.CASES) over the oracle's camera rays of samples 1 and 2 of every live pixel:
  test_rays_form_is_the_trace            t and prim equal rrt_trace_closest's bit for bit: infinite t_max, a finite one on every third ray, skip_prim
  test_rays_form_against_the_reference   every field within its bar; fp32 may leave out a ray only where its prim differs from the oracle's (<= 1 %)
  test_against_the_planes                rho, n, t over the handle's own camera rays against rrt_render_aov's planes at one sample per pixel
  test_sites_form_is_the_rays_form       fed (prim, u, v) of the triangle hits
  test_sites_by_hand                     vertices, centroids, outside points and a dead site against the restatement
  test_invariances                       memory kind, NULL groups, pre-filled outputs, batch sizes, max_paths, the frame before and after
  test_refusals                          each by its message
The bars (BARS) are 16 x the largest deviation measured on an MI355X against that reference, per field and precision, recorded in
profiles/surface_gpu_tests.txt; positions and t relative to the scene extent, the other fields absolute. Where the measurement is 0, the bar is 0.
The sphere scene (cfg1) has bars of its own and does not widen the triangles' (fp32 sphere normals: test_aov.py, SPHERE_NORMAL_SHARE).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import surface_reference as SR
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError
from rs_ray_toy_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PRECS = pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
CASES = pytest.mark.parametrize("case", SR.CASES)
TRI_CASES = pytest.mark.parametrize("case", SR.TRI_CASES)
FIELDS = ("p", "n", "s", "uv", "rho", "t")
SYMBOLS = ("rrt_surface_rays", "rrt_surface_at", "rrt_atlas_sites")
SURFACE_MEMBERS = ["mem", "precision", "px", "py", "pz", "nx", "ny", "nz", "sx", "sy", "sz", "tu", "tv", "rho_r", "rho_g", "rho_b", "t", "prim", "material"]

# 16 x the largest value measured (profiles/surface_gpu_tests.txt): {key: {field: (f64, f32)}}.
#   rays_tri / rays_sphere: rrt_surface_rays against the reference on the four triangle scenes / on cfg1
#   planes:                 rrt_surface_rays against rrt_render_aov's planes (zero expected)
#   at_rays:                rrt_surface_at at the trace's (prim, u, v) against rrt_surface_rays on those rays
#   at_hand:                rrt_surface_at against the restatement from the description
BARS = {
    "rays_tri": {"p": (16 * 0.0, 16 * 8.940e-07), "n": (16 * 0.0, 16 * 8.112e-07), "s": (16 * 1.388e-17, 16 * 1.025e-06), "uv": (16 * 0.0, 16 * 8.146e-05),
                 "rho": (16 * 0.0, 16 * 6.361e-06), "t": (16 * 0.0, 16 * 1.955e-06)},
    "rays_sphere": {"p": (16 * 0.0, 16 * 3.498e-04), "n": (16 * 3.331e-16, 16 * 6.915e-03), "s": (16 * 0.0, 16 * 6.691e-03), "uv": (16 * 1.665e-16, 16 * 2.209e-03),
                    "rho": (16 * 0.0, 16 * 0.0), "t": (16 * 0.0, 16 * 4.555e-04)},
    "planes": {"rho": (16 * 0.0, 16 * 0.0), "n": (16 * 0.0, 16 * 0.0), "t": (16 * 0.0, 16 * 0.0)},
    # f64 p: the rays form is o + d t, the sites form the barycentric point; fp32: both are the barycentric point, the same statements
    "at_rays": {"p": (16 * 1.871e-15, 16 * 0.0), "n": (16 * 0.0, 16 * 0.0), "s": (16 * 0.0, 16 * 0.0), "uv": (16 * 0.0, 16 * 0.0), "rho": (16 * 0.0, 16 * 0.0)},
    "at_hand": {"p": (16 * 4.206e-19, 16 * 4.453e-08), "n": (16 * 0.0, 16 * 2.673e-07), "s": (16 * 0.0, 16 * 2.846e-07), "uv": (16 * 0.0, 16 * 0.0), "rho": (16 * 0.0, 16 * 3.874e-08)},
}


def _name(prec):
    return "f64" if prec == RRT_F64 else "f32"


def _bar(key, field, prec):
    return BARS[key][field][0 if prec == RRT_F64 else 1]


def _dev(a, b, scale=1.0):
    """the largest |a - b| / scale over the arrays (0 for empty ones)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / scale) if a.size else 0.0


def _check_fields(key, case, prec, got, want, ext, sel=slice(None), fields=None):
    """Print every field's deviation, then assert each against its bar"""
    devs = {}
    for f in fields or BARS[key]:
        devs[f] = _dev(got[f][sel], want[f][sel], ext if f in ("p", "t") else 1.0)
        print(f"BAR {key} {f} {_name(prec)} {case} {devs[f]:.3e}")
    for f, v in devs.items():
        assert v <= _bar(key, f, prec), (key, case, f, v)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    lib = A.lib()
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"librrt.so does not export {name}"
        assert name in A.PROTOTYPES and name + "(" in header
    assert "#define RRT_ABI_VERSION 11" in " ".join(header.split())


def test_struct_mirrors_match_the_c_layout(tmp_path):
    structs = {"rrt_surface": (A.Surface, SURFACE_MEMBERS), "rrt_sites": (A.Sites, ["mem", "precision", "prim", "b1", "b2"])}
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cname, (mirror, fields) in structs.items():
        assert [name for name, _ in mirror._fields_] == fields
        src.append(f'printf("{cname}.size %zu\\n", sizeof({cname}));')
        src += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c11", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for cname, (mirror, fields) in structs.items():
        assert int(out[cname + ".size"]) == C.sizeof(mirror)
        for f in fields:
            assert int(out[f"{cname}.{f}"]) == getattr(mirror, f).offset, (cname, f)


def _host_surface(m, dtype, prec, fields=A.SURFACE_GROUPS, fill=3.5):
    out = A.Surface(A.RRT_MEM_HOST, prec)
    arrs = {}
    for f in fields:
        for k in A.SURFACE_GROUPS[f]:
            arrs[k] = np.full(m, 35 if f == "prim" else fill, np.int32 if f == "prim" else dtype)
            setattr(out, k, arrs[k].ctypes.data)
    return out, arrs


def test_null_arguments_are_refused_before_a_handle_is_looked_at():
    lib = A.lib()
    a = np.zeros(4)
    i4 = np.zeros(4, np.int32)
    rays = A.Rays(A.RRT_MEM_HOST, RRT_F64, *([a.ctypes.data] * 7), None)
    sites = A.Sites(A.RRT_MEM_HOST, RRT_F64, i4.ctypes.data, a.ctypes.data, a.ctypes.data)
    out, arrs = _host_surface(4, np.float64, RRT_F64)
    calls = [(lambda: lib.rrt_surface_rays(None, None, 4, C.byref(out)), b"rrt_rays"),
             (lambda: lib.rrt_surface_at(None, None, 4, C.byref(out)), b"rrt_sites"),
             (lambda: lib.rrt_surface_rays(None, C.byref(rays), 4, None), b"rrt_surface"),
             (lambda: lib.rrt_surface_at(None, C.byref(sites), 4, None), b"rrt_surface"),
             (lambda: lib.rrt_surface_rays(None, C.byref(rays), 4, C.byref(out)), b"null handle"),
             (lambda: lib.rrt_surface_at(None, C.byref(sites), 4, C.byref(out)), b"null handle"),
             (lambda: lib.rrt_surface_rays(None, C.byref(rays), 0, C.byref(out)), b"n must be > 0"),
             (lambda: lib.rrt_surface_at(None, C.byref(sites), 1 << 31, C.byref(out)), b"batch too large"),
             (lambda: lib.rrt_atlas_sites(None, 4, 4, None, 0, A.RRT_MEM_HOST, None, a.ctypes.data, a.ctypes.data, None), b"null output"),
             (lambda: lib.rrt_atlas_sites(None, 4, 4, None, 0, A.RRT_MEM_HOST, i4.ctypes.data, a.ctypes.data, a.ctypes.data, None), b"null handle")]
    for call, substr in calls:
        assert call() == A.RRT_EINVAL and substr in lib.rrt_last_error(), lib.rrt_last_error()
    rays.dy = None
    assert lib.rrt_surface_rays(None, C.byref(rays), 4, C.byref(out)) == A.RRT_EINVAL and b"null ray array" in lib.rrt_last_error()
    sites.b2 = None
    assert lib.rrt_surface_at(None, C.byref(sites), 4, C.byref(out)) == A.RRT_EINVAL and b"null site array" in lib.rrt_last_error()
    for k, v in arrs.items():
        assert np.all(v == (35 if v.dtype == np.int32 else 3.5)), k


@CASES
def test_reference_checks_itself(case, workdir):
    """The sites restatement at the oracle's (prim, u, v) is the oracle's own p and n, to 1e-9 x extent and 1e-9, on every triangle hit."""
    sc = SR.scene(workdir, case)
    ref = SR.reference(sc, case)
    is_tri = SR.tables(sc, case)[1]
    sel = np.flatnonzero(ref["hit"] & is_tri[np.maximum(ref["prim"], 0)])
    if case == "cfg1":
        assert len(sel) == 0 and ref["hit"].any()
        return
    assert len(sel) > 500
    at = SR.site_records(sc, case, ref["prim"][sel], ref["u"][sel], ref["v"][sel])
    dp = _dev(at["p"], ref["p"][sel], SR.extent(sc)); dn = _dev(at["n"], ref["n"][sel])
    print(f"{case}: {len(sel)} triangle hits, restated p off by {dp:.3e} x extent, n by {dn:.3e}")
    assert dp <= 1e-9 and dn <= 1e-9
    assert np.array_equal(at["material"], ref["material"][sel])
    assert _dev(at["uv"], ref["uv"][sel]) == 0.0 and _dev(at["s"], ref["s"][sel]) <= 1e-9


def test_the_margins_the_comparisons_rest_on(workdir):
    """No ray's box or triangle decision margin is below 1e-9: the f64 comparisons leave out nothing."""
    for case in SR.CASES:
        ref = SR.reference(SR.scene(workdir, case), case)
        print(f"{case}: {len(ref['margin'])} rays, {int((ref['margin'] < 1e-4).sum())} with a margin below 1e-4, smallest {ref['margin'].min():.3e}")
        assert ref["margin"].min() >= 1e-9


# ---- GPU: one shared set of calls per (case, precision), never written to --------------------------------------------------------------------------------
_runs = {}


def _tmax_every_third(ref):
    """a finite t_max on every third ray: half the hit distance (the ray becomes a miss that keeps its t_max), 100 where the oracle misses"""
    tmax = np.full(len(ref["t"]), np.inf)
    third = np.arange(len(tmax)) % 3 == 0
    tmax[third] = np.where(ref["hit"][third], 0.5 * ref["t"][third], 100.0)
    return tmax


def _run(case, prec, workdir):
    key = (case, prec)
    if key not in _runs:
        sc = SR.scene(workdir, case)
        ref = SR.reference(sc, case)
        o, d = SR.rays(sc, case)
        m = len(o)
        r = Renderer(sc, 0, prec)
        out = dict(trace={}, rec={})
        inf = np.full(m, np.inf)
        first = r.trace_closest(o, d, inf)
        variants = {"inf": (inf, None), "third": (_tmax_every_third(ref), None), "skip": (inf, first["prim"].copy())}
        for name, (tmax, skip) in variants.items():
            out["trace"][name] = first if name == "inf" else r.trace_closest(o, d, tmax, skip_prim=skip)
            out["rec"][name] = r.surface(o, d, tmax, skip_prim=skip)
        tr = out["trace"]["inf"]
        is_tri = SR.tables(sc, case)[1]
        tri_hit = (tr["prim"] >= 0) & is_tri[np.maximum(tr["prim"], 0)]
        out["tri_hit"] = tri_hit
        if tri_hit.any():
            out["at"] = r.surface_at(np.where(tri_hit, tr["prim"], -1), tr["u"], tr["v"])
        r.close()
        _runs[key] = out
    return _runs[key]


@pytest.mark.gpu
@PRECS
@CASES
def test_rays_form_is_the_trace(case, prec, workdir):
    run = _run(case, prec, workdir)
    for name in ("inf", "third", "skip"):
        tr, rec = run["trace"][name], run["rec"][name]
        assert np.array_equal(tr["prim"], rec["prim"]), name
        assert np.array_equal(tr["t"].view(np.uint8), rec["t"].view(np.uint8)), name
        dead = rec["prim"] < 0
        assert np.array_equal(rec["material"] < 0, dead)
        for f in ("p", "n", "s", "uv", "rho"):
            assert not rec[f][dead].any(), (name, f)
    third = run["rec"]["third"]
    assert np.isfinite(third["t"][::3]).all() and (third["prim"][::3] < 0).sum() > 0          # the cut rays keep their t_max
    sk = run["rec"]["skip"]
    hit0 = run["trace"]["inf"]["prim"] >= 0
    if case != "cfg1":   # (skip_prim names a triangle a ray starts on; a sphere is not skipped, by either call)
        assert not (sk["prim"][hit0] == run["trace"]["inf"]["prim"][hit0]).any()               # the second surface is recorded
        assert (sk["prim"] >= 0).sum() > 0


@pytest.mark.gpu
@PRECS
@CASES
def test_rays_form_against_the_reference(case, prec, workdir):
    sc = SR.scene(workdir, case)
    ref = SR.reference(sc, case)
    rec = _run(case, prec, workdir)["rec"]["inf"]
    differ = rec["prim"] != ref["prim"]
    print(f"{case} {_name(prec)}: {int(differ.sum())} of {len(differ)} rays left out (the device's prim is not the oracle's)")
    if prec == RRT_F64:
        assert not differ.any()
    assert differ.sum() <= 0.01 * len(differ)
    keep = ~differ
    assert np.array_equal(rec["material"][keep], ref["material"][keep])
    hit = keep & ref["hit"]
    want = dict(ref)
    _check_fields("rays_sphere" if case == "cfg1" else "rays_tri", case, prec, rec, want, SR.extent(sc), sel=hit)
    miss = keep & ~ref["hit"]
    assert np.isinf(rec["t"][miss]).all()


@pytest.mark.gpu
@PRECS
def test_against_the_planes(prec, workdir, tmp_path):
    """One sample per pixel under the box filter of radius 0.5 (fw = 1): the planes of rrt_render_aov ARE the records of the handle's own camera rays."""
    from rs_ray_toy_amd import RRT_FIXED_BVH, Scene, scenes
    cfg, root = scenes.cfg5(str(tmp_path), xres=64, yres=48, nsamp=2, max_depth=8, n=64)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    W, H = sc.resolution
    r = Renderer(sc, 0, prec)
    dims, rays, w = r.camera_samples((0, 0, W, H), 1, 2)
    planes = r.render_aov()
    live = np.flatnonzero(w > 0)
    rec = r.surface(rays[live, :3], rays[live, 3:], fields=("rho", "n", "t", "prim"))
    r.close()
    hit = rec["prim"] >= 0
    y, x = live[hit] // W, live[hit] % W
    assert hit.sum() > 300 and np.array_equal(planes["depth"][..., 2] > 0, np.bincount(live[hit], minlength=W * H).reshape(H, W) > 0)
    got = dict(rho=rec["rho"][hit], n=rec["n"][hit], t=rec["t"][hit])
    want = dict(rho=planes["albedo"][y, x, :3], n=planes["normal"][y, x, :3], t=planes["depth"][y, x, 0])
    _check_fields("planes", "cfg5_1spp", prec, got, want, SR.extent(sc))


@pytest.mark.gpu
@PRECS
@TRI_CASES
def test_sites_form_is_the_rays_form(case, prec, workdir):
    sc = SR.scene(workdir, case)
    run = _run(case, prec, workdir)
    rec, at, sel = run["rec"]["inf"], run["at"], run["tri_hit"]
    assert sel.sum() > 500
    assert np.array_equal(at["prim"][sel], rec["prim"][sel]) and np.array_equal(at["material"][sel], rec["material"][sel])
    assert not at["t"].any()
    dead = ~sel
    assert (at["prim"][dead] == -1).all() and (at["material"][dead] == -1).all()
    for f in ("p", "n", "s", "uv", "rho"):
        assert not at[f][dead].any(), f
    _check_fields("at_rays", case, prec, at, rec, SR.extent(sc), sel=sel)


def _hand_sites(sc, case):
    """12 sites over three primitives: vertices and centroid of two, centroid and two outside points of the third, one dead site"""
    ref = SR.reference(sc, case)
    is_tri = SR.tables(sc, case)[1]
    prims = np.unique(ref["prim"][ref["hit"] & is_tri[np.maximum(ref["prim"], 0)]])
    a, b, c = prims[0], prims[len(prims) // 2], prims[-1]
    third = 1.0 / 3.0
    sites = [(a, 0, 0), (a, 1, 0), (a, 0, 1), (a, third, third), (b, third, third), (b, -0.25, 0.5), (b, 1.5, -0.25), (c, 0, 0), (c, 1, 0), (c, 0, 1), (c, 0.25, 0.5), (-1, 0.5, 0.25)]
    return np.array([s[0] for s in sites], np.int32), np.array([s[1] for s in sites], np.float64), np.array([s[2] for s in sites], np.float64)


@pytest.mark.gpu
@PRECS
@TRI_CASES
def test_sites_by_hand(case, prec, workdir):
    sc = SR.scene(workdir, case)
    prim, b1, b2 = _hand_sites(sc, case)
    assert len(prim) == 12 and len(set(prim[prim >= 0])) == 3
    r = Renderer(sc, 0, prec)
    at = r.surface_at(prim, b1, b2)
    r.close()
    want = SR.site_records(sc, case, prim, b1.astype(r.dtype), b2.astype(r.dtype))
    assert np.array_equal(at["prim"], prim) and np.array_equal(at["material"], want["material"])
    assert at["prim"][-1] == -1 and at["material"][-1] == -1 and not at["t"].any()
    for f in ("p", "n", "s", "uv", "rho"):
        assert not at[f][-1].any(), f
    _check_fields("at_hand", case, prec, at, want, SR.extent(sc), sel=slice(0, 11))


def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_records(r, o, d, fields, sites=None):
    """the records through device memory (torch tensors): {member: array}"""
    import torch
    m = len(o) if sites is None else len(sites[0])
    outs = {k: torch.full((m,), 35 if f == "prim" else 3.5, dtype=torch.int32 if f == "prim" else (torch.float32 if r.dtype == np.float32 else torch.float64), device="cuda:0")
            for f in fields for k in A.SURFACE_GROUPS[f]}
    ptrs = {k: t.data_ptr() for k, t in outs.items()}
    if sites is None:
        cols = [_torch(np.asarray(a, r.dtype)) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], np.full(m, np.inf))]
        torch.cuda.synchronize()
        r.surface_device([t.data_ptr() for t in cols], m, ptrs)
    else:
        cols = [_torch(np.asarray(sites[0], np.int32)), _torch(np.asarray(sites[1], r.dtype)), _torch(np.asarray(sites[2], r.dtype))]
        torch.cuda.synchronize()
        r.surface_at_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), m, ptrs)
    torch.cuda.synchronize()
    return Renderer._surface_dict({k: t.cpu().numpy() for k, t in outs.items()})


def _same(a, b, fields=None):
    for f in fields or a:
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)), f


@pytest.mark.gpu
@PRECS
def test_invariances(prec, workdir):
    """Bit for bit, on the textured scene (instanced, vn on the cube, TEX kernels): both forms"""
    case = "textured"
    sc = SR.scene(workdir, case)
    o, d = SR.rays(sc, case)
    m = len(o)
    r = Renderer(sc, 0, prec)
    frame0 = r.render()
    full = r.surface(o, d)
    tri = full["prim"] >= 0
    sites = (np.where(tri, full["prim"], -1), np.where(tri, r.trace_closest(o, d, np.full(m, np.inf))["u"], 0), np.where(tri, r.trace_closest(o, d, np.full(m, np.inf))["v"], 0))
    full_at = r.surface_at(*sites)
    # host and device memory; device outputs pre-filled with 3.5 / 35 are overwritten, dead records included
    _same(full, _device_records(r, o, d, A.SURFACE_GROUPS))
    _same(full_at, _device_records(r, o, d, A.SURFACE_GROUPS, sites=sites))
    # any group set to NULL changes no other array
    for g in A.SURFACE_GROUPS:
        rest = tuple(f for f in A.SURFACE_GROUPS if f != g)
        part = r.surface(o, d, fields=rest)
        assert set(part) == set(full) - ({"prim", "material"} if g == "prim" else {g})
        _same(part, full, part)
        part = r.surface_at(*sites, fields=rest)
        _same(part, full_at, part)
    # host outputs pre-filled with 3.5 are overwritten
    out, arrs = _host_surface(m, r.dtype, prec)
    st = [np.ascontiguousarray(a) for a in (sites[0].astype(np.int32), sites[1].astype(r.dtype), sites[2].astype(r.dtype))]
    cs = A.Sites(A.RRT_MEM_HOST, prec, *[a.ctypes.data for a in st])
    assert A.lib().rrt_surface_at(r._h, C.byref(cs), m, C.byref(out)) == A.RRT_OK
    _same(Renderer._surface_dict(arrs), full_at)
    # n = 1, 63, 257 and the full batch
    for n in (1, 63, 257):
        _same(r.surface(o[:n], d[:n]), {k: v[:n] for k, v in full.items()})
        _same(r.surface_at(*[a[:n] for a in sites]), {k: v[:n] for k, v in full_at.items()})
    # max_paths 64 against the default
    r.set_option("max_paths", 64)
    _same(r.surface(o, d), full)
    _same(r.surface_at(*sites), full_at)
    r.close()
    # a frame rendered before and after the calls is the same frame
    r = Renderer(sc, 0, prec)
    r.surface(o, d); r.surface_at(*sites)
    frame1 = r.render()
    r.close()
    assert np.array_equal(frame0, frame1) and frame0[..., :3].max() > 0


@pytest.mark.gpu
@PRECS
def test_refusals(prec, workdir):
    import torch
    lib = A.lib()
    sc = SR.scene(workdir, "cfg1")
    tri = SR.scene(workdir, "rigid")
    r, rt = Renderer(sc, 0, prec), Renderer(tri, 0, prec)
    dt = r.dtype
    other = RRT_F32 if prec == RRT_F64 else RRT_F64
    m = 4
    a = np.zeros(m, dt); one = np.ones(m, dt); i4 = np.zeros(m, np.int32)
    n_order = int(tri.desc.n_prim_order)

    def rays(mem=A.RRT_MEM_HOST, p=prec):
        return A.Rays(mem, p, a.ctypes.data, a.ctypes.data, a.ctypes.data, one.ctypes.data, a.ctypes.data, a.ctypes.data, one.ctypes.data, None)

    def refused(rc, substr, arrs=None):
        assert rc == A.RRT_EINVAL and substr in lib.rrt_last_error(), lib.rrt_last_error()
        for k, v in (arrs or {}).items():
            assert np.all(v == (35 if v.dtype == np.int32 else 3.5)), k

    out, arrs = _host_surface(m, dt, prec)
    part = A.Surface.from_buffer_copy(out); part.ny = None
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays()), m, C.byref(part)), b"partly set", arrs)
    part = A.Surface.from_buffer_copy(out); part.material = None
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays()), m, C.byref(part)), b"partly set", arrs)
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays()), m, C.byref(A.Surface(A.RRT_MEM_HOST, prec))), b"all NULL")
    wrong = A.Surface.from_buffer_copy(out); wrong.precision = other
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays()), m, C.byref(wrong)), b"record precision must match the handle", arrs)
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays(p=other)), m, C.byref(out)), b"ray precision must match the handle", arrs)
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays(mem=A.RRT_MEM_DEVICE)), m, C.byref(out)), b"same memory kind", arrs)
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays()), 0, C.byref(out)), b"n must be > 0", arrs)

    def sites(h, prim, b1=None, b2=None):
        prim = np.ascontiguousarray(prim, np.int32)
        b1 = np.ascontiguousarray(a if b1 is None else b1, dt); b2 = np.ascontiguousarray(a if b2 is None else b2, dt)
        s = A.Sites(A.RRT_MEM_HOST, prec, prim.ctypes.data, b1.ctypes.data, b2.ctypes.data)
        return lib.rrt_surface_at(h, C.byref(s), m, C.byref(out))

    refused(sites(r._h, [0, -1, -1, -1]), b"names a sphere", arrs)
    refused(sites(rt._h, [0, 1, n_order, 2]), b"outside [0, n_prim_order) (site 2)", arrs)
    refused(sites(rt._h, [0, 1, -2, 2]), b"outside [0, n_prim_order)", arrs)
    refused(sites(rt._h, [0, 1, 2, 3], b2=[0, np.nan, 0, 0]), b"non-finite barycentric (site 1)", arrs)
    refused(sites(rt._h, [0, 1, 2, 3], b1=[0, 0, 0, np.inf]), b"non-finite barycentric (site 3)", arrs)
    assert sites(rt._h, [0, 1, -1, 3]) == A.RRT_OK and arrs["prim"].tolist() == [0, 1, -1, 3]
    # device-resident bad sites leave the pre-filled outputs untouched
    for handle, prim, b1 in ((rt, [0, 1, n_order, 2], [0, 0, 0, 0]), (rt, [0, 1, 2, 3], [0, np.nan, 0, 0]), (r, [-1, 0, -1, -1], [0, 0, 0, 0])):
        tp, t1, t2 = _torch(np.asarray(prim, np.int32)), _torch(np.asarray(b1, dt)), _torch(np.zeros(m, dt))
        outs = {k: _torch(np.full(m, 35, np.int32) if k in ("prim", "material") else np.full(m, 3.5, dt)) for g in A.SURFACE_GROUPS.values() for k in g}
        torch.cuda.synchronize()
        with pytest.raises(RrtError, match="a refused site"):
            handle.surface_at_device(tp.data_ptr(), t1.data_ptr(), t2.data_ptr(), m, {k: t.data_ptr() for k, t in outs.items()})
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert (t.cpu().numpy() == (35 if k in ("prim", "material") else 3.5)).all(), k
        handle.surface_at([0 if handle is rt else -1] * m, a, a)       # the handle's error word was put back: the next call passes
    # a frame in flight
    W, H = tri.resolution
    film = torch.zeros((H, W, 4), dtype=torch.float32 if prec == RRT_F32 else torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rt.render_bands_begin(0, 1, film.data_ptr())
    out2, arrs2 = _host_surface(m, dt, prec)
    refused(lib.rrt_surface_rays(rt._h, C.byref(rays()), m, C.byref(out2)), b"a frame is in flight", arrs2)
    s = A.Sites(A.RRT_MEM_HOST, prec, i4.ctypes.data, a.ctypes.data, a.ctypes.data)
    refused(lib.rrt_surface_at(rt._h, C.byref(s), m, C.byref(out2)), b"a frame is in flight", arrs2)
    rt.render_end()
    r.close(); rt.close()
