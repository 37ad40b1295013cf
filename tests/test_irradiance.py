"""rrt_irradiance and rrt_irradiance_rays (include/rrt.h): irradiance and SH sums at caller-supplied points, rays made on the device.

Scenes and points: irradiance_reference.py - 24 x 16 films at 17 samples per pixel (16 draws), Halton; Path, DirectLighting and a textured material; 37
points (first hits of the oracle's camera rays) of which one has a zero normal, one a normal of length 3 and one shares its neighbour's pixel.

CPU: the symbols are exported, the ctypes mirrors have the C layout, NULL arguments are refused before a handle is looked at. Everything else needs the
GPU: (1) the rays against the numpy restatement of the definition; (2) the sums are rrt_radiance over those very rays, bit for bit; (3) split, chunk,
memory-kind and pre-fill invariance, bit for bit; (4) a closed form that neither the device code nor rrt_radiance judges; (5) sphere mode and its SH
sums; (6) refusals and the handle's state.

The measured bars (BARS) are 16 x the largest deviation seen on an MI355X, recorded in profiles/irradiance_gpu_tests.txt.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import irradiance_reference as IR
import oracle_lib as O
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError, RrtUnsupported, resolve_irradiance, resolve_sh
from rs_ray_toy_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PRECS = pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
CASES = pytest.mark.parametrize("case", IR.CASES)
NS = IR.NSAMP - 1

# 16 x the largest value measured (profiles/irradiance_gpu_tests.txt), per precision
BARS = {
    "direction": {RRT_F64: 16 * 4.441e-16, RRT_F32: 16 * 4.047e-7},     # largest |component| deviation of a unit direction from the reference
    # largest origin deviation / scene extent. f64: measured 0 - p + nn * offset is the same IEEE operations in the same order on either side
    "origin": {RRT_F64: 16 * 0.0, RRT_F32: 16 * 6.506e-8},
    "y2": {RRT_F64: 16 * 5.488e-16, RRT_F32: 16 * 3.009e-7},            # sums4[:, 3] against numpy's f64 sum of y^2, relative
    "sh": {RRT_F64: 16 * 2.668e-16, RRT_F32: 16 * 6.314e-7},            # sh27 against numpy's sum L Y(wl), relative to the row's largest value
    "closed_form_f32": 16 * 1.352e-7,                                   # fp32 E against the f64 E of the closed-form scene, relative
}


def _name(prec):
    return "f64" if prec == RRT_F64 else "f32"


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    lib = A.lib()
    for name in ("rrt_irradiance", "rrt_irradiance_rays"):
        assert hasattr(lib, name), f"librrt.so does not export {name}"
        assert name in A.PROTOTYPES and name in open(HEADER).read()


def test_null_arguments_are_refused_before_a_handle_is_looked_at():
    lib = A.lib()
    assert lib.rrt_irradiance(None, None, 1, 1, 2, None, None, None) == A.RRT_EINVAL and b"rrt_points" in lib.rrt_last_error()
    assert lib.rrt_irradiance_rays(None, None, 1, 1, 2, None, None) == A.RRT_EINVAL and b"rrt_points" in lib.rrt_last_error()
    a = np.zeros(4)
    pts = A.Points(A.RRT_MEM_HOST, RRT_F64, *([a.ctypes.data] * 6), None)
    out = np.full(16, 3.5)
    for call, substr in ((lambda: lib.rrt_irradiance(None, C.byref(pts), 4, 1, 2, None, None, None), b"null output"),
                         (lambda: lib.rrt_irradiance_rays(None, C.byref(pts), 4, 1, 2, None, None), b"null output"),
                         (lambda: lib.rrt_irradiance(None, C.byref(pts), 4, 1, 2, None, out.ctypes.data, None), b"null handle"),
                         (lambda: lib.rrt_irradiance_rays(None, C.byref(pts), 4, 1, 2, None, out.ctypes.data), b"null handle")):
        assert call() == A.RRT_EINVAL and substr in lib.rrt_last_error(), lib.rrt_last_error()
    pts.py = None
    assert lib.rrt_irradiance(None, C.byref(pts), 4, 1, 2, None, out.ctypes.data, None) == A.RRT_EINVAL and b"null point array" in lib.rrt_last_error()
    assert np.all(out == 3.5)


def test_struct_mirrors_match_the_c_layout(tmp_path):
    structs = {"rrt_points": (A.Points, ["mem", "precision", "px", "py", "pz", "nx", "ny", "nz", "pixel"]), "rrt_irr_params": (A.IrrParams, ["mode", "pad", "offset"])}
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cname, (mirror, fields) in structs.items():
        assert [name for name, _ in mirror._fields_] == fields
        src.append(f'printf("{cname}.size %zu\\n", sizeof({cname}));')
        src += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    src += ['printf("modes %d %d\\n", RRT_IRR_COSINE, RRT_IRR_SPHERE);', "return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c11", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    lines = subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines()
    out = dict(line.split() for line in lines[:-1])
    for cname, (mirror, fields) in structs.items():
        assert int(out[cname + ".size"]) == C.sizeof(mirror)
        for f in fields:
            assert int(out[f"{cname}.{f}"]) == getattr(mirror, f).offset, (cname, f)
    assert lines[-1].split() == ["modes", str(A.RRT_IRR_COSINE), str(A.RRT_IRR_SPHERE)]


def test_resolvers():
    sums = np.array([[4.0, 8.0, 2.0, 30.0]])
    out = resolve_irradiance(sums, 4)
    assert np.allclose(out["E"], np.pi / 4 * sums[:, :3])
    mean_y = (sums[0, :3] @ IR.Y_WEIGHTS) / 4
    assert np.allclose(out["stderr"], np.pi * np.sqrt((30.0 / 4 - mean_y ** 2) / 3))
    sh = np.arange(27.0)[None]
    assert resolve_sh(sh, 8).shape == (1, 9, 3) and np.allclose(resolve_sh(sh, 8)[0, 2, 1], 4 * np.pi / 8 * 7.0)


# ---- GPU: one shared set of calls per (case, precision), never written to ------------------------------------------------------------------------------
_runs = {}


def _sample_nums(m, s0=1, s1=IR.NSAMP):
    return np.tile(np.arange(s0, s1), m)


def _radiance_over(r, od, pixel):
    """rrt_radiance over the rays of irradiance_rays, (m, ns, 3): the points' own streams, dead draws (six zeros) with weight 0"""
    m, ns = od.shape[:2]
    flat = od.reshape(m * ns, 6)
    live = flat[:, 3:].any(1)
    L = r.radiance(flat[:, :3], flat[:, 3:], np.repeat(np.asarray(pixel), ns, axis=0), _sample_nums(m, 1, ns + 1), weight=live.astype(r.dtype))
    return L.reshape(m, ns, 3).copy()


def _run(case, prec, workdir):
    key = (case, prec)
    if key not in _runs:
        sc = IR.scene(workdir, case)
        pts = IR.points(sc, case)
        p, n, pixel = pts["p"], pts["n"], pts["pixel"]
        r = Renderer(sc, 0, prec)
        out = dict(pts=pts)
        out["od"] = r.irradiance_rays(p, n, pixel=pixel, offset=IR.OFFSET)
        out["sums"] = r.irradiance(p, n, pixel=pixel, offset=IR.OFFSET)
        out["L"] = _radiance_over(r, out["od"], pixel)
        out["od_s"] = r.irradiance_rays(p, n, pixel=pixel, offset=IR.OFFSET, mode="sphere")
        out["sums_s"], out["sh"] = r.irradiance(p, n, pixel=pixel, offset=IR.OFFSET, mode="sphere", sh=True)
        out["L_s"] = _radiance_over(r, out["od_s"], pixel)
        r.close()
        for v in out.values():
            if isinstance(v, np.ndarray): v.setflags(write=False)
        _runs[key] = out
    return _runs[key]


_refs = {}


def _ref(case, mode, workdir):
    if (case, mode) not in _refs:
        sc = IR.scene(workdir, case)
        _refs[(case, mode)] = IR.rays(sc, case, IR.points(sc, case), 1, IR.NSAMP, IR.OFFSET, mode)
    return _refs[(case, mode)]


# ---- 1. the rays ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
@CASES
@pytest.mark.parametrize("mode", ["cosine", "sphere"])
def test_rays_match_the_definition(case, prec, mode, workdir):
    run = _run(case, prec, workdir)
    od = run["od" if mode == "cosine" else "od_s"].astype(np.float64)
    ref = _ref(case, mode, workdir)
    assert od.shape == (IR.N_POINTS, NS, 6)
    live = ref["live"]
    assert not live[IR.DEAD].any() and live[IR.LONG].all() and live.sum() >= (IR.N_POINTS - 1) * NS - 4
    assert not od[~live].any()                                                # dead draws: six zeros
    assert np.array_equal(od[..., 3:].any(-1), live)
    d_dev = np.abs(od[..., 3:] - ref["od"][..., 3:])[live].max()
    o_dev = np.abs(od[..., :3] - ref["od"][..., :3])[live].max() / IR.extent(IR.scene(workdir, case))
    print(f"rays {case} {mode} {_name(prec)}: direction deviation {d_dev:.3e}, origin deviation / extent {o_dev:.3e}")
    np.testing.assert_allclose(np.linalg.norm(od[..., 3:], axis=-1)[live], 1.0, rtol=0, atol=4e-7 if prec == RRT_F32 else 1e-15)
    assert d_dev <= BARS["direction"][prec], d_dev
    assert o_dev <= BARS["origin"][prec], o_dev
    # the point with |n| = 3 shoots the rays of its unit normal; the two points of one pixel share their local directions
    assert np.array_equal(ref["wl"][IR.REPEAT], ref["wl"][IR.REPEAT - 1])


# ---- 2. the sums are rrt_radiance over those very rays ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
@CASES
@pytest.mark.parametrize("mode", ["cosine", "sphere"])
def test_sums_are_radiance_over_the_rays(case, prec, mode, workdir):
    run = _run(case, prec, workdir)
    sums, L = (run["sums"], run["L"]) if mode == "cosine" else (run["sums_s"], run["L_s"])
    assert sums.dtype == L.dtype == (np.float32 if prec == RRT_F32 else np.float64)
    expect = IR.sums_in_order(L, sums.dtype)
    assert (expect > 0).any(1).sum() >= 1 and (sums[:, :3] > 0).any(), "every point is black"
    print(f"sums {case} {mode} {_name(prec)}: {int((sums[:, :3] != expect).sum())} of {expect.size} values differ, {int((expect > 0).any(1).sum())} points lit")
    assert np.array_equal(sums[:, :3], expect)
    assert not sums[IR.DEAD].any()
    y2 = IR.sum_y2(L)
    lit = y2 > 0
    assert np.array_equal(sums[:, 3] > 0, lit)
    rel = (np.abs(sums[:, 3].astype(np.float64) - y2)[lit] / y2[lit]).max()
    print(f"sums {case} {mode} {_name(prec)}: sum y^2 deviation {rel:.3e}")
    assert rel <= BARS["y2"][prec], rel


# ---- 3. split, chunk, memory kind, pre-fill -----------------------------------------------------------------------------------------------------------------------
def _device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _packed(pixel):
    pixel = np.asarray(pixel)
    return ((pixel[:, 1].astype(np.uint32) << 16) | pixel[:, 0].astype(np.uint32)).astype(np.uint32)


def _device_call(r, pts, s0, s1, mode, sums0, sh0):
    """irradiance_device on copies of the points in device memory; returns (sums, sh) as host arrays"""
    import torch
    m = len(pts["p"])
    tp = [_device(pts["p"][:, k].astype(r.dtype)) for k in range(3)]
    tn = [_device(pts["n"][:, k].astype(r.dtype)) for k in range(3)]
    tpix = _device(_packed(pts["pixel"]))
    tsums = _device(sums0)
    tsh = _device(sh0) if sh0 is not None else None
    torch.cuda.synchronize()
    r.irradiance_device([t.data_ptr() for t in tp], [t.data_ptr() for t in tn], m, s0, s1, tsums.data_ptr(), None if tsh is None else tsh.data_ptr(),
                        pixel_ptr=tpix.data_ptr(), offset=IR.OFFSET, mode=mode)
    torch.cuda.synchronize()
    return tsums.cpu().numpy(), None if tsh is None else tsh.cpu().numpy()


@pytest.mark.gpu
@PRECS
@CASES
def test_split_chunk_memory_and_prefill_change_no_bit(case, prec, workdir):
    run = _run(case, prec, workdir)
    pts = run["pts"]
    p, n, pixel = pts["p"], pts["n"], pts["pixel"]
    m = IR.N_POINTS
    r = Renderer(IR.scene(workdir, case), 0, prec)
    kw = dict(pixel=pixel, offset=IR.OFFSET)
    whole = {"cosine": (run["sums"], None), "sphere": (run["sums_s"], run["sh"])}
    assert (run["sh"] != 0).any()
    for mode, (sums_w, sh_w) in whole.items():
        sphere = mode == "sphere"

        def call(s0, s1, sums=None, sh=None):
            out = r.irradiance(p, n, s0, s1, mode=mode, sums=sums, sh=(True if sh is None else sh) if sphere else None, **kw)
            return out if sphere else (out, None)

        # [1, 6) then [6, 17) into one buffer
        a, b = call(1, 6)
        a, b = call(6, IR.NSAMP, a, b)
        assert np.array_equal(a, sums_w) and (not sphere or np.array_equal(b, sh_w)), f"{mode}: split draw ranges"
        # device arrays
        a, b = _device_call(r, pts, 1, IR.NSAMP, mode, np.zeros((m, 4), r.dtype), np.zeros((m, 27), r.dtype) if sphere else None)
        assert np.array_equal(a, sums_w) and (not sphere or np.array_equal(b, sh_w)), f"{mode}: device arrays"
        # a pre-filled buffer: pre-fill plus the draws, added one by one onto it. The three colour sums are plain adds that numpy repeats bit for
        # bit; sum y^2 and the SH sums add products the device may fuse, so they are held to the split (bit for bit) and to the whole call's values
        # within the 17 roundings of 16 adds onto a start of the sums' own size (64 eps of the largest magnitude involved)
        pre, pre_sh = np.full((m, 4), 0.75, r.dtype), np.full((m, 27), -0.5, r.dtype)
        a, b = call(1, IR.NSAMP, pre.copy(), pre_sh.copy())
        L = run["L_s"] if sphere else run["L"]
        assert np.array_equal(a[:, :3], IR.sums_in_order(L, r.dtype, start=pre[:, :3])), f"{mode}: pre-filled sums"
        assert np.all(a[IR.DEAD] == 0.75) and (not sphere or np.all(b[IR.DEAD] == -0.5))
        a2, b2 = call(1, 6, pre.copy(), pre_sh.copy())
        a2, b2 = call(6, IR.NSAMP, a2, b2)
        assert np.array_equal(a2, a) and (not sphere or np.array_equal(b2, b)), f"{mode}: pre-filled, split"
        eps = np.finfo(r.dtype).eps
        for got, start, total in ((a, pre, sums_w),) + (((b, pre_sh, sh_w),) if sphere else ()):
            got, start, total = got.astype(np.float64), start.astype(np.float64), total.astype(np.float64)
            assert np.all(np.abs(got - (start + total)) <= 64 * eps * (np.abs(start) + np.abs(total).max(1, keepdims=True))), f"{mode}: pre-fill plus sums"
        # the rays too
        od = r.irradiance_rays(p, n, 6, IR.NSAMP, mode=mode, **kw)
        assert np.array_equal(od, (run["od_s"] if sphere else run["od"])[:, 5:])
    # pools of 64 slots: 37 points x 16 draws in ten passes of four points (one point in the last)
    r.set_option("max_paths", 64)
    for mode, (sums_w, sh_w) in whole.items():
        out = r.irradiance(p, n, mode=mode, sh=True if mode == "sphere" else None, **kw)
        a, b = out if mode == "sphere" else (out, None)
        assert np.array_equal(a, sums_w) and (b is None or np.array_equal(b, sh_w)), f"{mode}: max_paths 64"
    r.close()


@pytest.mark.gpu
@PRECS
def test_a_draw_range_longer_than_the_pools_is_cut(prec, workdir):
    """129 samples per pixel: 128 draws against pools of 64 slots, so every point's range is cut in two and each pass holds one point."""
    import copy
    cfg, root = IR._config(workdir, "path")
    cfg = copy.deepcopy(cfg)
    cfg["Sampler"]["nsamp"] = 129
    sc = IR.PR.load(cfg, root)
    pts = IR.points(IR.scene(workdir, "path"), "path")
    sel = [0, IR.DEAD, 20]
    p, n, pixel = pts["p"][sel], pts["n"][sel], pts["pixel"][sel]
    r = Renderer(sc, 0, prec)
    whole, sh = r.irradiance(p, n, pixel=pixel, offset=IR.OFFSET, mode="sphere", sh=True)
    r.set_option("max_paths", 64)
    cut, sh_cut = r.irradiance(p, n, pixel=pixel, offset=IR.OFFSET, mode="sphere", sh=True)
    od = r.irradiance_rays(p, n, pixel=pixel, offset=IR.OFFSET, mode="sphere")
    r.close()
    assert whole[:, :3].max() > 0 and np.array_equal(cut, whole) and np.array_equal(sh_cut, sh)
    assert od.shape == (3, 128, 6) and not od[1].any() and od[0, :, 3:].any(1).all() and od[2, :, 3:].any(1).all()


# ---- 4. closed form ---------------------------------------------------------------------------------------------------------------------------------------------
_plane = {}


def _plane_run(prec, workdir):
    if prec not in _plane:
        sc = IR.scene(workdir, "plane")
        pts = IR.plane_points()
        r = Renderer(sc, 0, prec)
        sums = r.irradiance(pts["p"], pts["n"], pixel=pts["pixel"])
        r.close()
        _plane[prec] = sums
    return _plane[prec]


@pytest.mark.gpu
@PRECS
def test_sensor_above_a_lit_plane_reads_the_closed_form(prec, workdir):
    """Every draw of a sensor 0.01 above a 10 x 10 matte plane, looking down, hits the plane (asserted on the reference's rays with the oracle's
    traversal) and carries Li = Kd / pi x L x cos(theta_light): pi / N x sums = Kd L cos(theta_light) with no Monte-Carlo error."""
    sc = IR.scene(workdir, "plane")
    pts = IR.plane_points()
    ref = IR.rays(sc, "plane", pts, 1, IR.NSAMP, 0.0, "cosine")
    assert ref["live"].all()
    flat = ref["od"].reshape(-1, 6)
    hit = O.trace_closest(sc, flat[:, :3], flat[:, 3:], np.full(len(flat), np.inf))
    assert (hit["prim"] >= 0).all(), "a draw of the reference misses the plane"
    E = resolve_irradiance(_plane_run(prec, workdir), NS)["E"]
    expect = IR.plane_irradiance()
    rel = np.abs(E - expect).max() / expect.max()
    print(f"closed form {_name(prec)}: E[0] = {E[0]}, expected {expect}, deviation {rel:.3e}")
    if prec == RRT_F64:
        assert rel < 1e-9, rel       # the project's f64 frame bar
    else:
        E64 = resolve_irradiance(_plane_run(RRT_F64, workdir), NS)["E"]
        rel32 = np.abs(E - E64).max() / E64.max()
        print(f"closed form f32 against f64: {rel32:.3e}")
        assert rel32 <= BARS["closed_form_f32"], rel32
    assert resolve_irradiance(_plane_run(prec, workdir), NS)["stderr"].max() <= 1e-3 * expect.max()      # every draw carries the same value


# ---- 5. sphere mode ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
@CASES
def test_sh_sums(case, prec, workdir):
    run = _run(case, prec, workdir)
    ref = _ref(case, "sphere", workdir)
    sh, sums, L = run["sh"].astype(np.float64), run["sums_s"].astype(np.float64), run["L_s"]
    expect = IR.sh_sums(L, ref["wl"])
    scale = np.abs(expect).max(1)
    lit = scale > 0
    assert lit.any() and not sh[~lit].any() and not sh[IR.DEAD].any()
    rel = (np.abs(sh - expect)[lit] / scale[lit, None]).max()
    print(f"sh {case} {_name(prec)}: deviation {rel:.3e} of a row's largest value, {int(lit.sum())} points lit")
    assert rel <= BARS["sh"][prec], rel
    # band 0 is a constant: sum (L c) against c sum L, non-negative terms, 16 adds and one product each way - 32 roundings at the most
    eps = np.finfo(run["sh"].dtype).eps
    np.testing.assert_allclose(sh[:, 0:3], IR.SH_C[0] * sums[:, :3], rtol=32 * eps, atol=0)
    assert resolve_sh(run["sh"], NS).shape == (IR.N_POINTS, 9, 3)


@pytest.mark.gpu
@PRECS
def test_null_normals_are_the_z_axis(prec, workdir):
    sc = IR.scene(workdir, "path")
    pts = IR.points(sc, "path")
    p, pixel = pts["p"], pts["pixel"]
    r = Renderer(sc, 0, prec)
    z = np.tile(np.array([0.0, 0.0, 1.0]), (len(p), 1))
    od_null = r.irradiance_rays(p, None, pixel=pixel, mode="sphere")
    od_z = r.irradiance_rays(p, z, pixel=pixel, mode="sphere")
    s_null, sh_null = r.irradiance(p, None, pixel=pixel, mode="sphere", sh=True)
    s_z, sh_z = r.irradiance(p, z, pixel=pixel, mode="sphere", sh=True)
    # pixel = NULL: point i takes the stream of pixel (i % xres, (i / xres) % yres)
    W, H = sc.resolution
    i = np.arange(len(p))
    od_auto = r.irradiance_rays(p, None, mode="sphere")
    od_named = r.irradiance_rays(p, None, pixel=np.stack([i % W, (i // W) % H], 1), mode="sphere")
    r.close()
    assert od_null[..., 3:].any(-1).all()
    assert np.array_equal(od_null, od_z) and np.array_equal(s_null, s_z) and np.array_equal(sh_null, sh_z)
    assert np.array_equal(od_auto, od_named) and not np.array_equal(od_auto, od_null)
    # the local frame of the z axis: local (x, y, z) = world (y, -x, z)
    ref = IR.rays(sc, "path", dict(p=p, n=None, pixel=pixel), 1, IR.NSAMP, 0.0, "sphere")
    wl = ref["wl"]
    np.testing.assert_allclose(od_null[..., 3:], np.stack([-wl[..., 1], wl[..., 0], wl[..., 2]], -1), rtol=0, atol=BARS["direction"][prec])


# ---- 6. refusals and the handle's state ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@PRECS
def test_bad_arguments_are_refused_and_write_nothing(prec, workdir):
    import torch
    lib = A.lib()
    sc = IR.scene(workdir, "path")
    W, H = sc.resolution
    pts = IR.points(sc, "path")
    m = IR.N_POINTS
    r = Renderer(sc, 0, prec)
    sums = np.full((m, 4), 3.5, r.dtype)
    sh = np.full((m, 27), 3.5, r.dtype)
    od = np.full((m, NS, 6), 3.5, r.dtype)

    def fresh(pixel=pts["pixel"]):
        return r._points(pts["p"], pts["n"], pixel)

    def refused(ps, substr, count=m, s0=1, s1=IR.NSAMP, params=None, h=r._h, sums_ptr=sums.ctypes.data, sh_ptr=None, code=A.RRT_EINVAL, rays=True):
        prm = C.byref(params) if params is not None else None
        calls = [lambda: lib.rrt_irradiance(h, C.byref(ps) if ps is not None else None, count, s0, s1, prm, sums_ptr, sh_ptr)]
        if rays: calls.append(lambda: lib.rrt_irradiance_rays(h, C.byref(ps) if ps is not None else None, count, s0, s1, prm, od.ctypes.data))
        for call in calls:
            rc = call()
            assert rc == code, (rc, lib.rrt_last_error())
            assert substr in lib.rrt_last_error().decode(), lib.rrt_last_error()
        assert np.all(sums == 3.5) and np.all(sh == 3.5) and np.all(od == 3.5)

    refused(None, "rrt_points")
    ps, keep = fresh(); refused(ps, "null handle", h=None)
    ps, keep = fresh(); refused(ps, "null output", sums_ptr=None, rays=False)
    for field in ("px", "pz"):
        ps, keep = fresh(); setattr(ps, field, None); refused(ps, "null point array")
    ps, keep = fresh(); ps.ny = None; refused(ps, "normals partly set")
    ps, keep = fresh(); ps.mem = 7; refused(ps, "bad mem")
    ps, keep = fresh(); ps.precision = RRT_F32 if prec == RRT_F64 else RRT_F64; refused(ps, "precision")
    ps, keep = fresh(); refused(ps, "n must be", count=0)
    ps, keep = fresh(); refused(ps, "batch too large", count=1 << 31)
    for s0, s1 in ((0, 5), (3, 3), (5, 2), (1, IR.NSAMP + 1)):
        ps, keep = fresh(); refused(ps, "draw range", s0=s0, s1=s1)
    ps, keep = fresh(); refused(ps, "bad mode", params=A.IrrParams(2, 0, 0.0))
    for bad in (np.inf, -np.inf, np.nan):
        ps, keep = fresh(); refused(ps, "offset must be finite", params=A.IrrParams(A.RRT_IRR_COSINE, 0, bad))
    ps, keep = fresh(); refused(ps, "sphere-mode output", sh_ptr=sh.ctypes.data, rays=False)
    ps, keep = fresh(); refused(ps, "sphere-mode output", params=A.IrrParams(A.RRT_IRR_COSINE, 0, 0.0), sh_ptr=sh.ctypes.data, rays=False)
    ps, keep = fresh(); ps.nx = ps.ny = ps.nz = None; refused(ps, "null normals in cosine mode")
    # a pixel outside the film, host memory: the host sees it
    packed = _packed(pts["pixel"])
    for k, word in ((17, (3 << 16) | W), (m - 1, (H << 16) | 2)):
        q = packed.copy(); q[k] = word
        ps, keep = fresh(pixel=q); refused(ps, "pixel outside the film")
    # a frame in flight
    dev_film = torch.zeros((H, W, 4), dtype=torch.float32 if prec == RRT_F32 else torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, dev_film.data_ptr())
    ps, keep = fresh(); refused(ps, "in flight")
    r.render_end()

    # the same pixel in device memory: the generating kernel's check, before anything is traced, and nothing is written
    for k, word in ((17, (3 << 16) | W), (m - 1, (H << 16) | 2)):
        q = packed.copy(); q[k] = word
        bad_pts = dict(p=pts["p"], n=pts["n"], pixel=np.stack([q & 0xffff, q >> 16], 1))
        with pytest.raises(RrtError) as e:
            _device_call(r, bad_pts, 1, IR.NSAMP, "sphere", sums, sh)
        assert e.value.code == A.RRT_EINVAL and type(e.value) is RrtError and "pixel outside the film" in str(e.value)
    # (_device_call copies back only after a call that returned; a refused one is looked at here)
    tp = [_device(pts["p"][:, k].astype(r.dtype)) for k in range(3)]
    tn = [_device(pts["n"][:, k].astype(r.dtype)) for k in range(3)]
    q = packed.copy(); q[3] = (H << 16)
    tpix, tsums, tsh = _device(q), _device(sums), _device(sh)
    torch.cuda.synchronize()
    with pytest.raises(RrtError):
        r.irradiance_device([t.data_ptr() for t in tp], [t.data_ptr() for t in tn], m, 1, IR.NSAMP, tsums.data_ptr(), tsh.data_ptr(), pixel_ptr=tpix.data_ptr(), mode="sphere")
    torch.cuda.synchronize()
    assert bool((tsums == 3.5).all()) and bool((tsh == 3.5).all())
    # and the handle still answers
    run = _run("path", prec, workdir)
    assert np.array_equal(r.irradiance(pts["p"], pts["n"], pixel=pts["pixel"], offset=IR.OFFSET), run["sums"])
    r.close()


@pytest.mark.gpu
@PRECS
def test_the_stratified_sampler_is_unsupported(prec, workdir):
    r = Renderer(IR.scene(workdir, "stratified"), 0, prec)
    p = np.zeros((4, 3)); n = np.tile(np.array([0.0, 1.0, 0.0]), (4, 1))
    for call in (lambda: r.irradiance(p, n, 1, 3), lambda: r.irradiance_rays(p, n, 1, 3)):
        with pytest.raises(RrtUnsupported) as e:
            call()
        assert "StratifiedSampler" in str(e.value)
    r.close()


@pytest.mark.gpu
@PRECS
def test_an_ao_scene_adds_zeros(prec, workdir):
    pts = IR.points(IR.scene(workdir, "path"), "path")
    r = Renderer(IR.scene(workdir, "ao"), 0, prec)
    pre, pre_sh = np.full((IR.N_POINTS, 4), 0.75, r.dtype), np.full((IR.N_POINTS, 27), -0.5, r.dtype)
    sums, sh = r.irradiance(pts["p"], pts["n"], pixel=pts["pixel"], offset=IR.OFFSET, mode="sphere", sums=pre.copy(), sh=pre_sh.copy())
    od = r.irradiance_rays(pts["p"], pts["n"], pixel=pts["pixel"], offset=IR.OFFSET, mode="sphere")
    r.close()
    assert np.array_equal(sums, pre) and np.array_equal(sh, pre_sh)
    assert np.array_equal(od, _run("path", prec, workdir)["od_s"])      # the rays are the scene's geometry and sampler, not its integrator


@pytest.mark.gpu
@PRECS
def test_the_handle_is_left_as_it_was(prec, workdir):
    sc = IR.scene(workdir, "path")
    pts = IR.points(sc, "path")
    W, H = sc.resolution
    run = _run("path", prec, workdir)
    r = Renderer(sc, 0, prec)
    before = r.render((0, 0, W, H))
    sums = r.irradiance(pts["p"], pts["n"], pixel=pts["pixel"], offset=IR.OFFSET)
    od = r.irradiance_rays(pts["p"], pts["n"], pixel=pts["pixel"], offset=IR.OFFSET)
    s_s, sh = r.irradiance(pts["p"], pts["n"], pixel=pts["pixel"], offset=IR.OFFSET, mode="sphere", sh=True)
    after = r.render((0, 0, W, H))
    r.close()
    assert before[..., :3].max() > 0 and np.array_equal(after, before)
    assert np.array_equal(sums, run["sums"]) and np.array_equal(od, run["od"]) and np.array_equal(s_s, run["sums_s"]) and np.array_equal(sh, run["sh"])
