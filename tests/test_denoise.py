"""rrt_denoise (include/rrt.h): the edge-avoiding a-trous wavelet filter over the film, guided by the planes of rrt_render_aov.

CPU tests: the C layout and defaults of rrt_denoise_params, the refusals that need no device, properties of the numpy reference
(tests/denoise_reference.py, written from the definition on the prototype), and that the definition denoises oracle frames.

GPU tests, against that reference on synthetic films (DR.synthetic: three planar regions 90 degrees apart, depth ramps, gamma noise, a hole without
weight, a block without hits, a partly covered band - no pixel is excluded from any comparison):
  f64 handle: xyz within 1e-9 of the output's largest magnitude (the project's f64 bar), weight channel equal.
  fp32 handle: against the reference started from the fp32 records (record_dtype). FP32_BAR is 4 x the largest error measured on an MI355X
               (FP32_MEASURED, relative to the output's largest magnitude; DESIGN.md section 4 has the table).
  dn_lds 0 / 1, device and host memory, in place and out of place, a second call, bands summed by the caller: identical bits.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_reference as AR
import denoise_reference as DR
import oracle_lib as O
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtError, Scene, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
PLANES = ("albedo", "normal", "depth")

# fp32 device mode against the reference on the same fp32 records: largest |difference| / largest |output| over the cases of SHAPES, measured on an
# MI355X (ROCm 7), and the bar at 4 x that (exp / log differ between ROCm versions). The frame's fp32 bar is 1e-4.
FP32_MEASURED = 1.234e-6
FP32_BAR = 4.0 * FP32_MEASURED


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_denoise_params_match_c_layout_and_defaults(tmp_path):
    fields = [name for name, _ in A.DenoiseParams._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("size %zu\\n", sizeof(rrt_denoise_params));']
    src += [f'printf("{f} %zu\\n", offsetof(rrt_denoise_params, {f}));' for f in fields]
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", str(c), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert fields == ["iterations", "demodulate", "sigma_color", "sigma_normal", "sigma_depth"]
    assert int(out["size"]) == C.sizeof(A.DenoiseParams)
    for f in fields:
        assert int(out[f]) == getattr(A.DenoiseParams, f).offset, f
    p = A.DenoiseParams(-1, -1, -1.0, -1.0, -1.0)
    A.lib().rrt_denoise_defaults(C.byref(p))
    assert (p.iterations, p.demodulate, p.sigma_color, p.sigma_normal, p.sigma_depth) == (5, 1, 4.0, 32.0, 8.0)
    assert {k: getattr(p, k) for k in fields} == DR.DEFAULTS
    A.lib().rrt_denoise_defaults(None)


def test_denoise_refuses_bad_arguments_without_a_device():
    """NULL arguments and parameters out of range are RRT_EINVAL before anything touches a device, each with its own message; the output is untouched."""
    lib = A.lib()
    film = np.ones(4, np.float32); out = np.full(4, 7.0, np.float32)
    planes = [np.ones(4, np.float32) for _ in range(3)]
    ptr = [p.ctypes.data for p in planes]
    good = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, *ptr)

    def params(**kw):
        p = A.DenoiseParams()
        lib.rrt_denoise_defaults(C.byref(p))
        for k, v in kw.items(): setattr(p, k, v)
        return C.byref(p)

    def refused(msg, h, f, aov, p, o):
        assert lib.rrt_denoise(h, f, aov, p, o) == A.RRT_EINVAL
        assert msg in lib.rrt_last_error(), lib.rrt_last_error()

    refused(b"rrt_aov", None, film.ctypes.data, None, None, out.ctypes.data)
    for k in range(3):
        q = list(ptr); q[k] = None
        refused(b"three planes", None, film.ctypes.data, C.byref(A.Aov(A.RRT_MEM_HOST, A.RRT_F32, *q)), None, out.ctypes.data)
    refused(b"bad mem", None, film.ctypes.data, C.byref(A.Aov(7, A.RRT_F32, *ptr)), None, out.ctypes.data)
    for it in (0, 7, -3):
        refused(b"iterations", None, film.ctypes.data, C.byref(good), params(iterations=it), out.ctypes.data)
    for bad in (0.0, -1.0, float("nan")):
        refused(b"sigma_normal", None, film.ctypes.data, C.byref(good), params(sigma_normal=bad), out.ctypes.data)
        refused(b"sigma_depth", None, film.ctypes.data, C.byref(good), params(sigma_depth=bad), out.ctypes.data)
    refused(b"null film", None, None, C.byref(good), None, out.ctypes.data)
    refused(b"null film", None, film.ctypes.data, C.byref(good), None, None)
    refused(b"null handle", None, film.ctypes.data, C.byref(good), None, out.ctypes.data)
    refused(b"null handle", None, film.ctypes.data, C.byref(good), params(iterations=6, sigma_color=0.0), out.ctypes.data)
    assert np.all(out == 7.0) and np.all(film == 1.0)


def _two_surfaces(W=40, H=24, seed=3):
    """Two flat surfaces with perpendicular normals meeting at x = W / 2, noisy radiance"""
    rng = np.random.default_rng(seed)
    left = np.arange(W) < W // 2
    n = np.where(left[None, :, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])) * np.ones((H, W, 1))
    z = np.where(left, 5.0, 7.0) * np.ones((H, W))
    spp = 8.0
    film = np.zeros((H, W, 4)); alb = np.zeros((H, W, 4)); nrm = np.zeros((H, W, 4)); dep = np.zeros((H, W, 4))
    film[..., 3] = 3.0 * spp
    film[..., :3] = DR.rgb_to_xyz(rng.gamma(2.0, 0.5, (H, W, 3))) * film[..., 3:4]
    alb[..., :3] = 0.5 * spp; alb[..., 3] = spp
    nrm[..., :3] = n * spp; nrm[..., 3] = spp
    dep[..., 0] = z * spp; dep[..., 1] = (z * z + 1e-4) * spp; dep[..., 2] = spp
    return film, dict(albedo=alb, normal=nrm, depth=dep), left


def test_reference_leaks_no_bit_across_a_perpendicular_edge():
    film, aov, left = _two_surfaces()
    a = DR.denoise(film, **aov)
    loud = film.copy()
    loud[:, ~left, :3] *= 100.0
    b = DR.denoise(loud, **aov)
    assert np.array_equal(a[:, left], b[:, left])
    assert not np.array_equal(a[:, ~left], b[:, ~left])
    assert not np.array_equal(a[:, left], film[:, left])      # and the filter did something on the quiet side


def test_reference_keeps_a_constant_image():
    H, W = 24, 40
    film, aov = DR.synthetic(W, H, seed=5)
    data = film[..., 3] > 0
    film[..., :3] = np.where(data[..., None], DR.rgb_to_xyz(np.array([0.3, 0.7, 0.2])) * film[..., 3:4], 0.0)
    for demodulate in (0, 1):
        if demodulate == 0:
            out = DR.denoise(film, **aov, demodulate=0)
        else:      # c = rgb / albedo is constant where the albedo is
            flat = {k: v.copy() for k, v in aov.items()}
            flat["albedo"][..., :3] = 0.5 * flat["albedo"][..., 3:4]
            out = DR.denoise(film, **flat)
        rel = np.abs(out[..., :3] - film[..., :3]).max() / np.abs(film[..., :3]).max()
        print(f"constant image, demodulate {demodulate}: {rel:.3e} relative")
        assert rel < 2e-6


def test_reference_is_finite_and_copies_holes_and_weights():
    film, aov = DR.synthetic(53, 37, seed=7)
    out = DR.denoise(film, **aov)
    hole = film[..., 3] == 0
    assert hole.any() and (aov["depth"][..., 2] == 0)[~hole].any()
    assert (0 < aov["depth"][..., 2])[aov["depth"][..., 2] < aov["albedo"][..., 3]].any()
    assert np.all(np.isfinite(out))
    assert np.array_equal(out[..., 3], film[..., 3])
    assert np.array_equal(out[hole], film[hole])
    assert not np.array_equal(out[~hole], film[~hole])
    film[hole] = [1.0, 2.0, 3.0, 0.0]      # whatever a pixel without weight holds comes back
    out = DR.denoise(film, **aov)
    assert np.array_equal(out[hole], film[hole]) and np.all(np.isfinite(out))


def test_reference_one_flat_iteration_is_the_b3_blur():
    film, aov, _ = _two_surfaces(W=30, H=20)
    for k in ("normal", "depth"):      # one flat surface
        aov[k][...] = aov[k][:, :1]
    out = DR.denoise(film, **aov, iterations=1, sigma_color=0.0, demodulate=0)
    rgb = DR.xyz_to_rgb(film[..., :3] / film[..., 3:4])
    blur = sum(DR.B3[dy + 2] * DR.B3[dx + 2] * np.roll(rgb, (-dy, -dx), (0, 1)) for dy in range(-2, 3) for dx in range(-2, 3))
    want = DR.rgb_to_xyz(blur) * film[..., 3:4]
    inner = (slice(2, -2), slice(2, -2))
    np.testing.assert_allclose(out[inner][..., :3], want[inner], rtol=1e-12, atol=0)


ORACLE_CASES = {"cfg5": lambda wd, ns: scenes.cfg5(wd, xres=96, yres=64, nsamp=ns, max_depth=5, n=64),
                "cfg4": lambda wd, ns: scenes.cfg4(wd, xres=96, yres=64, nsamp=ns, max_depth=5, n=64),
                "cfg3": lambda wd, ns: scenes.cfg3(wd, xres=96, yres=64, nsamp=ns, max_depth=5)}


def _rgb(film):
    with np.errstate(all="ignore"):
        return np.where(film[..., 3:4] > 0, DR.xyz_to_rgb(film[..., :3] / film[..., 3:4]), 0.0)


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_definition_denoises_oracle_frames(name, workdir):
    """8 spp oracle frames, filtered under the planes of the same 8 samples, against the 128 spp frame: RGB RMSE strictly below the noisy frame's."""
    sc8 = Scene.loads(*ORACLE_CASES[name](workdir, 9))
    sc128 = Scene.loads(*ORACLE_CASES[name](workdir, 129))
    noisy, clean = O.render(sc8), O.render(sc128)
    p = AR.planes(sc8)
    out = DR.denoise(noisy, p["albedo"], p["normal"], p["depth"])
    rmse = lambda f: float(np.sqrt(((_rgb(f) - _rgb(clean)) ** 2).mean()))
    print(f"{name}: RGB RMSE against 128 spp: noisy {rmse(noisy):.4g}, denoised {rmse(out):.4g}, ratio {rmse(out) / rmse(noisy):.3f}")
    assert np.all(np.isfinite(out))
    assert rmse(out) < rmse(noisy)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

# (W, H, parameters): partial tiles both ways; a last step whose reach of 32 exceeds the frame; a film smaller than one workgroup; the iteration range;
# no demodulation; no luminance stop
SHAPES = {
    "131x77_defaults": (131, 77, {}),
    "37x21_reach": (37, 21, {"iterations": 5}),
    "20x6_small": (20, 6, {}),
    "iterations_1": (67, 35, {"iterations": 1}),
    "iterations_6": (67, 35, {"iterations": 6}),
    "demodulate_0": (67, 35, {"demodulate": 0}),
    "sigma_color_0": (67, 35, {"sigma_color": 0.0}),
}
_handles_scenes, _inputs, _refs = {}, {}, {}


def _renderer(W, H, prec, workdir, nsamp=3):
    """config 3 (12 + 12 triangles: created at once) with the film's size: rrt_denoise takes the frame size from the handle"""
    key = (W, H, nsamp)
    if key not in _handles_scenes:
        _handles_scenes[key] = Scene.loads(*scenes.cfg3(workdir, xres=W, yres=H, nsamp=nsamp, max_depth=5))
    return Renderer(_handles_scenes[key], 0, prec)


def _input(W, H, dtype):
    """the synthetic film and planes of a size, rounded to the handle's type once (both sides then start from the same numbers)"""
    key = (W, H, np.dtype(dtype).name)
    if key not in _inputs:
        film, aov = DR.synthetic(W, H, seed=1000 + W)
        _inputs[key] = (np.ascontiguousarray(film, dtype), {k: np.ascontiguousarray(v, dtype) for k, v in aov.items()})
    return _inputs[key]


def _reference(name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _refs:
        W, H, params = SHAPES[name]
        film, aov = _input(W, H, dtype)
        _refs[key] = DR.denoise(film, **aov, **params, record_dtype=np.float32 if dtype == np.float32 else None)
        _refs[key].setflags(write=False)
    return _refs[key]


def _rel_err(got, ref):
    return float(np.abs(got[..., :3].astype(np.float64) - ref[..., :3]).max() / np.abs(ref[..., :3]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_f64_matches_reference(name, workdir):
    W, H, params = SHAPES[name]
    film, aov = _input(W, H, np.float64)
    r = _renderer(W, H, RRT_F64, workdir)
    got = r.denoise(film, aov, **params)
    r.close()
    ref = _reference(name, np.float64)
    err = _rel_err(got, ref)
    print(f"{name}: f64 max error {err:.3e} of the output's largest magnitude")
    assert np.array_equal(got[..., 3], ref[..., 3])
    assert np.array_equal(got[film[..., 3] == 0], film[film[..., 3] == 0])
    assert err < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fp32_close_to_reference(name, workdir):
    W, H, params = SHAPES[name]
    film, aov = _input(W, H, np.float32)
    r = _renderer(W, H, RRT_F32, workdir)
    got = r.denoise(film, aov, **params)
    r.close()
    ref = _reference(name, np.float32)
    err = _rel_err(got, ref)
    print(f"{name}: fp32 max error {err:.3e} of the output's largest magnitude (bar {FP32_BAR:.1e})")
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[..., 3], film[..., 3])
    assert np.array_equal(got[film[..., 3] == 0], film[film[..., 3] == 0])
    assert err < FP32_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_denoise_lds_changes_nothing(prec, workdir):
    """dn_lds 1 (the default: LDS tiles at the steps where they are faster) and 0 (direct gathers at every step): the same bits."""
    dtype = np.float32 if prec == RRT_F32 else np.float64
    for W, H in ((131, 77), (20, 6)):
        film, aov = _input(W, H, dtype)
        r = _renderer(W, H, prec, workdir)
        outs = []
        for mode in (1, 0):
            r.set_option("dn_lds", mode)
            outs.append(r.denoise(film, aov, iterations=6))
        r.close()
        assert not np.array_equal(outs[0], film)
        assert np.array_equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_memory_kinds_in_place_and_repeats_agree(prec, workdir):
    import torch
    dtype = np.float32 if prec == RRT_F32 else np.float64
    W, H = 131, 77
    film, aov = _input(W, H, dtype)
    r = _renderer(W, H, prec, workdir)
    host = r.denoise(film, aov)
    again = r.denoise(film, aov)
    in_place = film.copy()
    assert r.denoise(in_place, aov, out=in_place) is in_place
    dev = [torch.from_numpy(a).to("cuda:0") for a in (film, aov["albedo"], aov["normal"], aov["depth"])]
    dev_out = torch.zeros_like(dev[0])
    torch.cuda.synchronize()
    r.denoise_device(dev[0].data_ptr(), [d.data_ptr() for d in dev[1:]], dev_out.data_ptr())
    assert np.array_equal(dev[0].cpu().numpy(), film)      # out of place: the film is read only
    r.denoise_device(dev[0].data_ptr(), [d.data_ptr() for d in dev[1:]], dev[0].data_ptr())
    r.close()
    assert not np.array_equal(host, film)
    assert np.array_equal(host, again)
    assert np.array_equal(host, in_place)
    assert np.array_equal(host, dev_out.cpu().numpy())
    assert np.array_equal(host, dev[0].cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])
def test_bands_summed_by_the_caller(prec, workdir):
    """The planes of three ranks' bands (box filter), summed by the caller, guide the filter to the same bits as the planes of the whole frame."""
    r = _renderer(128, 104, prec, workdir, nsamp=9)
    film = r.render()
    whole = r.render_aov()
    parts = [r.render_aov(rank=k, world=3) for k in range(3)]
    summed = {p: parts[0][p] + parts[1][p] + parts[2][p] for p in PLANES}
    a, b = r.denoise(film, whole), r.denoise(film, summed)
    r.close()
    assert film[..., :3].max() > 0 and not np.array_equal(a, film)
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_end_to_end_on_rendered_data(workdir):
    """render + render_aov + denoise on config 5 against the reference on the same arrays (f64: 1e-9); and render, denoise, render on one default
    fp32 handle: the same frame and the same counts."""
    cfg, root = scenes.cfg5(workdir, xres=96, yres=64, nsamp=9, max_depth=5, n=64)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F64)
    film = r.render()
    aov = r.render_aov()
    got = r.denoise(film, aov)
    r.close()
    ref = DR.denoise(film, **aov)
    err = _rel_err(got, ref)
    print(f"config 5 at 96 x 64, 8 spp: f64 max error {err:.3e}")
    assert (aov["albedo"][..., 3] > aov["depth"][..., 2]).any() and film[..., :3].max() > 0
    assert np.array_equal(got[..., 3], film[..., 3]) and not np.array_equal(got, film)
    assert err < 1e-9
    r = Renderer(sc, 0, RRT_F32)
    a, sa = r.render(stats=True)
    out = r.denoise(a, r.render_aov())
    b, sb = r.render(stats=True)
    r.close()
    assert np.all(np.isfinite(out)) and not np.array_equal(out, a)
    assert np.array_equal(a, b)
    for key in ("camera_rays", "closest_queries", "any_queries"):
        assert getattr(sa, key) == getattr(sb, key), key


@pytest.mark.gpu
def test_device_side_error_paths(workdir):
    import torch
    W, H = 64, 48
    film, aov = _input(W, H, np.float32)
    r = _renderer(W, H, RRT_F32, workdir)
    lib = A.lib()
    out = np.full((H, W, 4), 7.0, np.float32)
    planes64 = [np.zeros((H, W, 4)) for _ in range(3)]
    wrong = A.Aov(A.RRT_MEM_HOST, A.RRT_F64, *[p.ctypes.data for p in planes64])
    assert lib.rrt_denoise(r._h, film.ctypes.data, C.byref(wrong), None, out.ctypes.data) == A.RRT_EINVAL and b"precision" in lib.rrt_last_error()
    missing = A.Aov(A.RRT_MEM_HOST, A.RRT_F32, aov["albedo"].ctypes.data, None, aov["depth"].ctypes.data)
    assert lib.rrt_denoise(r._h, film.ctypes.data, C.byref(missing), None, out.ctypes.data) == A.RRT_EINVAL and b"three planes" in lib.rrt_last_error()
    with pytest.raises(RrtError, match="iterations"):
        r.denoise(film, aov, out=out, iterations=7)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, frame.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.denoise(film, aov, out=out)
    r.render_end()
    assert np.all(out == 7.0)
    assert r.denoise(film, aov, out=out) is out and not np.all(out == 7.0)      # and the handle still works
    r.close()


@pytest.mark.gpu
def test_cli_writes_the_denoised_png(tmp_path):
    """RRT_DENOISE=<path.png>: rrt_render and `python -m rs_ray_toy_amd` write the filtered frame beside the ordinary one, which stays byte for byte."""
    cfg, root = scenes.cfg5(str(tmp_path), xres=64, yres=48, nsamp=9, max_depth=5, n=64)
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    base = {k: v for k, v in os.environ.items() if k not in ("RRT_DENOISE", "RRT_AOV")}
    base["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
        plain, frame, dn = tmp_path / f"{tag}_plain.png", tmp_path / f"{tag}.png", tmp_path / f"{tag}_dn.png"
        p = subprocess.run(cmd + [str(scene), str(plain)], capture_output=True, text=True, timeout=600, env=base)
        assert p.returncode == 0, p.stderr
        assert not dn.exists()
        p = subprocess.run(cmd + [str(scene), str(frame)], capture_output=True, text=True, timeout=600, env=dict(base, RRT_DENOISE=str(dn)))
        assert p.returncode == 0, p.stderr
        assert frame.read_bytes() == plain.read_bytes()
        assert dn.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and dn.read_bytes()[16:24] == frame.read_bytes()[16:24]
        assert dn.read_bytes() != frame.read_bytes()
