"""Adaptive sampling (rrt_render_adaptive) and the error map it stops on (rrt_tile_error), include/rrt.h.

Scenes. A = test_moments.py's tilted config 3 (Path, depth 5) at 32 x 16, nsamp 13, min_samples 4, batch 4, threshold 0.95: the oracle's tile
errors put every decision at least 4 % from the threshold on the whole frame and on rect (8, 0, 32, 16), 1.5 % on rect (4, 4, 28, 12), whose tiles
are not aligned to the film. B = the smoke test's tilted config 2 at 32 x 16, nsamp 13: tile columns 0 and 3 are black in all 12 samples.

CPU tests: exports and prototypes, the refusals that need no device, the numpy reference loop (tests/adaptive_reference.py) on the oracle's frames.

GPU tests. No tolerance but two: rrt_tile_error against numpy at rtol 1e-12 (both sides compute in double from the same input bits; a 64-term
non-negative sum in any order differs by at most 64 x 2^-53) and the f64 film against the oracle at the project's f64 bar (1e-9 of each channel's
largest magnitude). Everything else is np.array_equal: Halton sample k of a pixel does not depend on nsamp and a pixel's sums are added in sample
order, so a tile that stopped at k holds the bits of a frame with nsamp = k + 1.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adaptive_reference as AD
import denoise_reference as DR
import moments_reference as MR
import oracle_lib as O
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError, RrtUnsupported, Scene, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt.h")
STATS = ("camera_rays", "closest_queries", "any_queries", "root_culled", "sky_culled")      # test_moments.py::STATS
NEW = ("rrt_tile_error", "rrt_render_adaptive")
FILM, NSAMP, K = (32, 16), 13, 12
PARAMS = dict(min_samples=4, batch=4, threshold=0.95)
CHECKPOINTS = (4, 8, 12)
RECTS = {"whole": (0, 0, 32, 16), "right": (8, 0, 32, 16), "inner": (4, 4, 28, 12)}
MAPS_A = {"whole": [[8, 8, 12, 4], [12, 8, 12, 4]], "right": [[8, 12, 4], [8, 12, 4]], "inner": [[12, 12, 4]]}
PRECS = pytest.mark.parametrize("prec", [RRT_F32, RRT_F64], ids=["f32", "f64"])


def _cfg_a(wd, nsamp, film=FILM, integrator=None, sampler=None, filt=None):
    """test_moments.py's scene: cfg3 with the enclosure and the cube instanced under generic rotations (no exact box / face ties)."""
    cfg, root = scenes.cfg3(wd, xres=film[0], yres=film[1], nsamp=nsamp, max_depth=5)
    cfg["Aggregate"]["primitives"][0]["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
    cfg["Aggregate"]["primitives"][1]["instances"] = [{"world_pos": [0.0, 0.0, 0.0], "rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}]
    if integrator: cfg["Integrator"] = dict(integrator)
    if sampler: cfg["Sampler"] = dict(sampler)
    if filt: cfg["Film"]["Filter"] = dict(filt)
    return cfg, root


def _cfg_b(wd, nsamp):
    """__graft_entry__.smoke()'s scene at 32 x 16"""
    cfg, root = scenes.cfg2(wd, xres=FILM[0], yres=FILM[1], nsamp=nsamp, max_depth=4)
    for inst in cfg["Aggregate"]["primitives"][0]["instances"]:
        inst["rotation_axis"] = [1.0, 2.0, 3.0]
    return cfg, root


DIRECT = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 5}
SCENES = {"A": lambda wd, n: _cfg_a(wd, n), "B": _cfg_b,
          "A_direct": lambda wd, n: _cfg_a(wd, n, integrator=DIRECT), "A_ao": lambda wd, n: _cfg_a(wd, n, integrator={"integrator_type": "AO"})}
_scenes, _prefix, _kframes = {}, {}, {}


def _scene(name, workdir, nsamp=NSAMP):
    if (name, nsamp) not in _scenes:
        _scenes[(name, nsamp)] = Scene.loads(*SCENES[name](workdir, nsamp))
    return _scenes[(name, nsamp)]


def _oracle_prefix(name, workdir):
    """{k: (moments, film)} of the oracle after k samples, whole frame; computed once, read-only"""
    if name not in _prefix:
        _prefix[name] = AD.prefix_moments(lambda n: _scene(name, workdir, n), CHECKPOINTS, K)
        for m, f in _prefix[name].values():
            m.setflags(write=False); f.setflags(write=False)
    return _prefix[name]


def _tiles(mask_tiles, rect, shape):
    """(H, W) pixel mask of the tiles of `rect` selected by the boolean map mask_tiles"""
    out = np.zeros(shape, bool)
    for ty, tx in zip(*np.nonzero(mask_tiles)):
        out[rect[1] + 8 * ty:rect[1] + 8 * ty + 8, rect[0] + 8 * tx:rect[0] + 8 * tx + 8] = True
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_and_abi_declares_the_calls():
    header = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in A.PROTOTYPES, name
        assert hasattr(A.lib(), name), name
    assert re.search(r"\bvoid\s+rrt_adaptive_defaults\s*\(", header) and "rrt_adaptive_defaults" in A.PROTOTYPES and hasattr(A.lib(), "rrt_adaptive_defaults")
    assert "#define RRT_ABI_VERSION 11" in header
    res, args = A.PROTOTYPES["rrt_tile_error"]
    assert res is C.c_int and len(args) == 5
    res, args = A.PROTOTYPES["rrt_render_adaptive"]
    assert res is C.c_int and len(args) == 8
    p = A.AdaptiveParams()
    A.lib().rrt_adaptive_defaults(C.byref(p))
    assert (p.min_samples, p.batch, p.max_samples, p.threshold) == (16, 16, 0, 0.05)
    assert C.sizeof(A.AdaptiveParams) == 24      # three uint32, padding, one double


def test_render_adaptive_refuses_bad_arguments_without_a_device():
    """RRT_EINVAL, each with its own message, before the handle is looked at; the buffers stay untouched."""
    lib = A.lib()
    film, mom = np.full(8 * 8 * 4, 7.0, np.float32), np.full(8 * 8 * 4, 7.0, np.float32)
    tiles = np.full(1, 7, np.uint32)
    rect = (C.c_int32 * 4)(0, 0, 8, 8)
    fake = C.c_void_p(1)      # never dereferenced: every case below fails on a check before the handle is used

    def call(h=fake, rect=rect, params=None, film=film.ctypes.data, mom=mom.ctypes.data, mem=A.RRT_MEM_HOST):
        return lib.rrt_render_adaptive(h, rect, C.byref(params) if params is not None else None, film, mom, tiles.ctypes.data, mem, None)

    cases = [(dict(rect=None), b"null rect"), (dict(film=None), b"null film"), (dict(mom=None), b"null moments"), (dict(mem=5), b"bad mem"),
             (dict(params=A.AdaptiveParams(1, 16, 0, 0.05)), b"min_samples"), (dict(params=A.AdaptiveParams(16, 0, 0, 0.05)), b"batch"),
             (dict(params=A.AdaptiveParams(16, 16, 0, -1.0)), b"threshold"), (dict(params=A.AdaptiveParams(16, 16, 0, float("nan"))), b"threshold"),
             (dict(rect=(C.c_int32 * 4)(0, 0, 12, 8)), b"whole 8 x 8 tiles"), (dict(rect=(C.c_int32 * 4)(0, 0, 8, 7)), b"whole 8 x 8 tiles"),
             (dict(rect=(C.c_int32 * 4)(8, 0, 8, 8)), b"whole 8 x 8 tiles"), (dict(h=None), b"null handle")]
    seen = set()
    for kw, word in cases:
        assert call(**kw) == A.RRT_EINVAL, kw
        msg = lib.rrt_last_error()
        assert word in msg and b"rrt_render_adaptive" in msg, (kw, msg)
        seen.add(msg)
    assert len(seen) == 9      # the two thresholds and the three rects share a message, every other refusal has its own
    assert np.all(film == 7.0) and np.all(mom == 7.0) and tiles[0] == 7


def test_tile_error_refuses_bad_arguments_without_a_device():
    lib = A.lib()
    mom, out = np.full(8 * 8 * 4, 7.0, np.float32), np.full(1, 7.0)
    rect = (C.c_int32 * 4)(0, 0, 8, 8)
    fake = C.c_void_p(1)
    call = lambda h=fake, m=mom.ctypes.data, mem=A.RRT_MEM_HOST, rect=rect, o=out.ctypes.data: lib.rrt_tile_error(h, m, mem, rect, o)
    cases = [(dict(m=None), b"null moments"), (dict(rect=None), b"null rect"), (dict(o=None), b"null output"), (dict(mem=-1), b"bad mem"),
             (dict(rect=(C.c_int32 * 4)(0, 0, 9, 8)), b"whole 8 x 8 tiles"), (dict(h=None), b"null handle")]
    seen = set()
    for kw, word in cases:
        assert call(**kw) == A.RRT_EINVAL, kw
        msg = lib.rrt_last_error()
        assert word in msg and b"rrt_tile_error" in msg, (kw, msg)
        seen.add(msg)
    assert len(seen) == len(cases)
    assert np.all(mom == 7.0) and out[0] == 7.0


def test_reference_tile_error_on_hand_made_tiles():
    """E by hand: a tile of constant pixels has E = 0; 64 pixels with mean 2 and variance of the mean 0.25 give E = 0.5 / 2; black and empty give 0;
    n_eff < 2 contributes its mean and no variance."""
    m = np.zeros((8, 40, 4))
    m[:, 0:8] = [8.0 * 3.0, 8.0 * 9.0, 8.0, 8.0]                 # 8 samples, all 3: variance 0
    n, mean, var_of_mean = 5.0, 2.0, 0.25                        # S2 / S0 - mean^2 = var_of_mean (n - 1) = 1
    m[:, 8:16] = [n * mean, n * (1.0 + mean * mean), n, n]
    m[:, 16:24] = [0.0, 0.0, 8.0, 8.0]                            # every sample black
    m[:, 32:40] = [3.0 * mean, 3.0 * 9.0, 3.0, 6.0]               # n_eff = 1.5
    E = AD.tile_error(m)
    assert E.shape == (1, 5)
    assert E[0, 0] == 0.0 and E[0, 2] == 0.0 and E[0, 3] == 0.0 and E[0, 4] == 0.0
    np.testing.assert_allclose(E[0, 1], np.sqrt(var_of_mean) / mean, rtol=1e-14)
    np.testing.assert_allclose(AD.tile_error(m, (8, 0, 24, 8)), E[:, 1:3], rtol=0, atol=0)


def test_reference_loop_reproduces_the_oracles_maps(workdir):
    pre = _oracle_prefix("A", workdir)
    E4, E8 = AD.tile_error(pre[4][0]), AD.tile_error(pre[8][0])
    np.testing.assert_allclose(E4, [[1.323, 1.047, 0.989, 0.772], [2.175, 1.215, 3.438, 0.723]], atol=5e-4)
    np.testing.assert_allclose(E8, [[0.903, 0.849, 1.054, 1.181], [1.396, 0.824, 2.302, 1.131]], atol=5e-4)
    for name, rect in RECTS.items():
        samples, seen = AD.loop(lambda k: pre[k][0], rect, K, **PARAMS)
        print(name, samples.tolist(), {k: np.round(e, 3).tolist() for k, e in seen.items()})
        assert samples.tolist() == MAPS_A[name], name
        margin = min(np.nanmin(np.abs(e / PARAMS["threshold"] - 1.0)) for k, e in seen.items() if k < K)
        assert margin > (0.04 if name != "inner" else 0.0149), (name, margin)      # 0.9642 / 0.95 = 1.0149: the nearest decision of all


def test_reference_loop_stops_black_tiles_at_min_samples(workdir):
    pre = _oracle_prefix("B", workdir)
    full = pre[K][0]
    assert np.all(full[:, 0:8, :2] == 0) and np.all(full[:, 24:32, :2] == 0) and np.all(full[..., 2] == K)      # columns 0 and 3: black in all 12 samples
    assert full[:, 8:24, 0].max() > 0
    samples, seen = AD.loop(lambda k: pre[k][0], RECTS["whole"], K, **PARAMS)
    assert np.all(samples[:, [0, 3]] == PARAMS["min_samples"]) and np.all(samples[:, 1:3] > PARAMS["min_samples"])
    assert np.all(seen[4][:, [0, 3]] == 0.0)
    tiny, _ = AD.loop(lambda k: pre[k][0], RECTS["whole"], K, 4, 4, 1e-300)      # E = 0 stops for ANY positive threshold
    assert np.all(tiny[:, [0, 3]] == 4) and np.all(tiny[:, 1:3] == K)


# ---- GPU: rrt_tile_error ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@PRECS
def test_tile_error_matches_numpy(prec, workdir):
    import torch
    dtype = np.float32 if prec == RRT_F32 else np.float64
    planes = []
    for (W, H), seed in (((136, 80), 7), ((24, 8), 8)):      # many workgroups with a last one of two tiles; three tiles
        film, _ = DR.synthetic(W, H, seed=1000 + W)
        planes.append((W, H, np.ascontiguousarray(MR.synthetic_moments(film, seed), dtype), ((0, 0, W, H), (8, 0, W, H)) + (((3, 5, 131, 69),) if W > 100 else ())))
    for W, H, m, rects in planes:
        sc = Scene.loads(*_cfg_a(workdir, 3, film=(W, H)))
        r = Renderer(sc, 0, prec)
        n_eff = np.where(m[..., 3] > 0, m[..., 2].astype(np.float64) ** 2 / np.where(m[..., 3] > 0, m[..., 3], 1), 0.0)
        if W > 100: assert (n_eff == 1.5).any() and ((m[..., 0] == 0) & (m[..., 2] > 0)).any() and (m[..., 2] == 0).any()      # every branch of the definition
        for rect in rects:
            want = AD.tile_error(m, rect)
            got = r.tile_error(m, rect)
            dev_m = torch.from_numpy(m).to("cuda:0")
            dev_out = torch.full(want.shape, -1.0, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            r.tile_error_device(dev_m.data_ptr(), rect, dev_out.data_ptr())
            err = np.abs(got - want).max() / want.max()
            print(f"{W} x {H} rect {rect}: {np.dtype(dtype).name} E in [{want.min():.3g}, {want.max():.3g}], largest difference {err:.3e}")
            assert got.shape == want.shape and want.max() > 0
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
            assert np.array_equal(dev_out.cpu().numpy(), got)
            assert np.array_equal(dev_m.cpu().numpy(), m)      # read only
        r.close()
    # a rendered plane with black tiles (B)
    r = Renderer(_scene("B", workdir), 0, prec)
    _, m = r.render_moments()
    got = r.tile_error(m)
    r.close()
    np.testing.assert_allclose(got, AD.tile_error(m), rtol=1e-12, atol=0)
    assert np.all(got[:, [0, 3]] == 0.0) and np.all(got[:, 1:3] > 0)


# ---- GPU: rrt_render_adaptive ------------------------------------------------------------------------------------------------------------------------

_adaptive = {}


def _run(name, rect_name, prec, workdir, **over):
    """(film, moments, tile_samples, stats) of the scene's adaptive frame on a fresh handle; cached for the default parameters, read-only"""
    key = (name, rect_name, prec)
    if over or key not in _adaptive:
        r = Renderer(_scene(name, workdir), 0, prec)
        out = r.render_adaptive(RECTS[rect_name], stats=True, **dict(PARAMS, **over))
        r.close()
        if over: return out
        for a in out[:3]: a.setflags(write=False)
        _adaptive[key] = out
    return _adaptive[key]


def _kframe(name, rect_name, prec, k, workdir):
    """render_moments(rect) of a fresh handle whose scene has nsamp = k + 1; computed once, read-only"""
    key = (name, rect_name, prec, k)
    if key not in _kframes:
        r = Renderer(_scene(name, workdir, k + 1), 0, prec)
        _kframes[key] = r.render_moments(RECTS[rect_name])
        r.close()
        for a in _kframes[key]: a.setflags(write=False)
    return _kframes[key]


def _check_bit_equality(name, rect_name, prec, workdir, run=None):
    """check 3: over the tiles that stopped at k, film and moments are those of the k-sample frame; nothing outside the rect is written"""
    film, mom, samples, st = run or _run(name, rect_name, prec, workdir)
    rect = RECTS[rect_name]
    counts = sorted(set(samples.ravel().tolist()))
    covered = np.zeros(film.shape[:2], bool)
    for k in counts:
        kf, km = _kframe(name, rect_name, prec, k, workdir)
        px = _tiles(samples == k, rect, film.shape[:2])
        covered |= px
        assert np.array_equal(film[px], kf[px]), (name, rect_name, k)
        assert np.array_equal(mom[px], km[px]), (name, rect_name, k)
        assert np.all(mom[px][:, 2] == k)
    inside = np.zeros(film.shape[:2], bool); inside[rect[1]:rect[3], rect[0]:rect[2]] = True
    assert np.array_equal(covered, inside)
    assert np.all(film[~inside] == 0) and np.all(mom[~inside] == 0)
    assert st.camera_samples == 64 * int(samples.sum())
    return counts


@pytest.mark.gpu
def test_f64_handle_takes_the_oracles_decisions(workdir):
    for rect_name, rect in RECTS.items():
        film, mom, samples, st = _run("A", rect_name, RRT_F64, workdir)
        assert samples.tolist() == MAPS_A[rect_name], rect_name
        assert st.camera_samples == 64 * int(samples.sum())
        for k in sorted(set(samples.ravel().tolist())):      # the oracle's frame of the rect at the tiles' own nsamp
            ref = O.render(_scene("A", workdir, k + 1), rect)
            px = _tiles(samples == k, rect, film.shape[:2])
            for ch in range(4):
                err = np.abs(film[..., ch] - ref[..., ch])[px].max() / np.abs(ref[..., ch]).max()
                assert err < 1e-9, (rect_name, k, ch, err)


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("case", ["A-whole", "A-right", "A-inner", "B-whole"])
def test_stopped_tiles_hold_the_shorter_frames_bits(case, prec, workdir):
    name, rect_name = case.split("-")
    counts = _check_bit_equality(name, rect_name, prec, workdir)
    film = _run(name, rect_name, prec, workdir)[0]
    assert film[..., :3].max() > 0
    if prec == RRT_F32: assert len(counts) >= 2, counts
    if name == "B":
        samples = _run(name, rect_name, prec, workdir)[2]
        assert np.all(samples[:, [0, 3]] == PARAMS["min_samples"])      # the black tile columns


@pytest.mark.gpu
@PRECS
def test_stopping_rule_replays_on_the_shorter_frames(prec, workdir):
    """The decisions, replayed in numpy on the bit-equal k-sample planes: E >= T at every checkpoint before a tile's count, E < T at its count where that is
    below K. A decision within 1e-9 T of T would be exempt (device and numpy sum in different orders); there is none."""
    T = PARAMS["threshold"]
    for name, rect_name in (("A", "whole"), ("A", "right"), ("A", "inner"), ("B", "whole")):
        rect = RECTS[rect_name]
        samples = _run(name, rect_name, prec, workdir)[2]
        E = {k: AD.tile_error(_kframe(name, rect_name, prec, k, workdir)[1], rect) for k in CHECKPOINTS}
        for k in CHECKPOINTS:
            looked = samples >= k      # the tiles that were still active at checkpoint k
            assert not (np.abs(E[k][looked] - T) <= 1e-9 * T).any()
            assert np.all(E[k][samples > k] >= T), (name, rect_name, k)
            if k < K: assert np.all(E[k][samples == k] < T), (name, rect_name, k)
        assert set(samples.ravel().tolist()) <= set(CHECKPOINTS)
        want, _ = AD.loop(lambda k: _kframe(name, rect_name, prec, k, workdir)[1], rect, K, **PARAMS)
        assert np.array_equal(samples, want)


@pytest.mark.gpu
@PRECS
def test_threshold_extremes(prec, workdir):
    r = Renderer(_scene("A", workdir), 0, prec)
    film, mom, samples, st = r.render_adaptive(stats=True, **dict(PARAMS, threshold=0.0))
    uf, um, ust = r.render_moments(stats=True)
    assert np.all(samples == K) and film[..., :3].max() > 0
    assert np.array_equal(film, uf) and np.array_equal(mom, um)
    for key in STATS:
        assert getattr(st, key) == getattr(ust, key), key
    assert st.camera_samples == 64 * int(samples.sum()) == ust.camera_samples
    film, mom, samples, st = r.render_adaptive(stats=True, **dict(PARAMS, threshold=1e30))
    assert np.all(samples == PARAMS["min_samples"]) and st.camera_samples == 64 * int(samples.sum())
    capped = r.render_adaptive(stats=True, **dict(PARAMS, threshold=0.0, max_samples=6))      # K = 6: rounds of 4 and 2
    r.close()
    assert np.all(capped[2] == 6) and capped[3].camera_samples == 64 * int(capped[2].sum())
    kf, km = _kframe("A", "whole", prec, 4, workdir)
    assert np.array_equal(film, kf) and np.array_equal(mom, km)


@pytest.mark.gpu
@PRECS
def test_pass_cutting_changes_no_bit(prec, workdir):
    """max_paths 256: listed passes cut into groups of four tiles and single-sample chunks"""
    want = _run("A", "whole", prec, workdir)
    r = Renderer(_scene("A", workdir), 0, prec)
    r.set_option("max_paths", 256)
    film, mom, samples, st = r.render_adaptive(stats=True, **PARAMS)
    r.close()
    assert np.array_equal(samples, want[2]) and np.array_equal(film, want[0]) and np.array_equal(mom, want[1])
    for key in STATS + ("camera_samples",):
        assert getattr(st, key) == getattr(want[3], key), key


def _cut(n_units, unit_px, n_samples, cap):
    """(groups, sample chunks per group) of the driver's cutter for n_units units of unit_px pixels and n_samples samples in pools of cap slots"""
    group = max(1, min(n_units, cap // unit_px))
    s_chunk = max(1, cap // (group * unit_px))
    return -(-n_units // group), -(-n_samples // s_chunk)


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("side,max_paths,batch,listed_cut", [(8, 256, 8, (1, 2)), (16, 128, 2, (2, 2))], ids=["one-group-two-chunks", "two-groups-one-sample-chunks"])
def test_listed_cut_corners_change_no_bit(side, max_paths, batch, listed_cut, prec, workdir):
    """The two other corners of the listed cut, beside test_pass_cutting_changes_no_bit's groups of four tiles and single-sample chunks. Threshold 0 is
    met by no tile, so every tile stays listed until K = 12 (min_samples 4).
    Rect 8 x 8 (one tile), max_paths 256, batch 8: one listed round of one group and two chunks of four samples.
    Rect 16 x 16 (four tiles), max_paths 128, batch 2: four listed rounds of two groups of two tiles and two single-sample chunks.
    Film, moments and tile_samples are those of the same call at max_paths = 2**28, bit for bit.
    The pool capacity is not rounded: a fresh handle's pools hold min(max_paths, the call's pixels x samples) slots exactly (768 and 3072 wanted
    here), so the cuts are computed from max_paths itself; the frame's closest-hit launch count - max_depth = 5 per pass of the Path integrator -
    shows that they happened."""
    rect, T = (0, 0, side, side), dict(PARAMS, batch=batch, threshold=0.0)
    out = {}
    for cap in (max_paths, 2 ** 28):
        r = Renderer(_scene("A", workdir), 0, prec)
        r.set_option("max_paths", cap)
        out[cap] = r.render_adaptive(rect, stats=True, **T)
        r.close()
    (film, mom, samples, st), want = out[max_paths], out[2 ** 28]
    n_tiles, rounds = (side // 8) ** 2, (K - T["min_samples"]) // batch
    groups, chunks = _cut(n_tiles, 64, batch, max_paths)
    assert (groups, chunks) == listed_cut
    g0, c0 = _cut(side * side, 1, T["min_samples"], max_paths)
    print(f"rect {side} x {side}, max_paths {max_paths}: round 0 {g0} x {c0} passes, {rounds} listed rounds of {groups} x {chunks}; closest launches {st.closest_launches}, {want[3].closest_launches} uncut")
    assert st.closest_launches == 5 * (g0 * c0 + rounds * groups * chunks) and want[3].closest_launches == 5 * (1 + rounds)
    assert np.all(samples == K) and film[..., :3].max() > 0
    assert np.array_equal(samples, want[2]) and np.array_equal(film, want[0]) and np.array_equal(mom, want[1])
    for key in STATS + ("camera_samples",):
        assert getattr(st, key) == getattr(want[3], key), key


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("min_samples,batch", [(4, 8), (2, 10)], ids=["8", "8+2"])
def test_listed_passes_of_eight_samples_or_more(min_samples, batch, prec, workdir):
    """A listed pass of fewer than 2^18 pixels and 8 samples or more takes the batched-by-8 loop of k_film_box_moments in its listed form (batch 8: exactly one batch;
    batch 10: a batch and the tail of 2) - the loop the default batch of 16 runs. Threshold 0: the moments frame's bits; threshold 0.95: the tiles
    that stopped at min_samples and those that went on to K, each equal to the shorter frame."""
    r = Renderer(_scene("A", workdir), 0, prec)
    film, mom, samples, st = r.render_adaptive(stats=True, min_samples=min_samples, batch=batch, threshold=0.0)
    uf, um = r.render_moments()
    mixed = r.render_adaptive(stats=True, min_samples=min_samples, batch=batch, threshold=PARAMS["threshold"])
    r.close()
    assert np.all(samples == K) and st.camera_samples == 64 * int(samples.sum()) and film[..., :3].max() > 0
    assert np.array_equal(film, uf) and np.array_equal(mom, um)
    counts = _check_bit_equality("A", "whole", prec, workdir, run=mixed)
    assert set(counts) <= {min_samples, K} and K in counts
    if min_samples == 4: assert counts == [4, K]      # the oracle's E at 4 samples: two tiles below 0.95 by 19 % and more, the nearest above by 4 %


@pytest.mark.gpu
def test_large_listed_pass(workdir):
    """512 x 512, nsamp 17, min 8, batch 8, threshold 0: the second round is ONE listed pass of 2^18 pixels (k_film_box_moments' path for passes of that
    size or more), bit-equal to the moments frame"""
    sc = Scene.loads(*_cfg_a(workdir, 17, film=(512, 512)))
    r = Renderer(sc, 0, RRT_F32)
    r.set_option("max_paths", 2 ** 28)
    film, mom, samples, st = r.render_adaptive(stats=True, min_samples=8, batch=8, threshold=0.0)
    uf, um = r.render_moments()
    r.close()
    assert samples.shape == (64, 64) and np.all(samples == 16) and st.camera_samples == 512 * 512 * 16
    assert film[..., :3].max() > 0 and np.array_equal(film, uf) and np.array_equal(mom, um)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A_direct", "A_ao"])
def test_other_integrators(name, workdir):
    for prec in (RRT_F32, RRT_F64):
        _check_bit_equality(name, "whole", prec, workdir)
        film, mom, samples, _ = _run(name, "whole", prec, workdir)
        if name == "A_ao": assert np.all(film[..., :3] == 0) and np.all(samples == PARAMS["min_samples"])      # ao.rs:62-64 returns black: E = 0 everywhere
        else: assert film[..., :3].max() > 0


@pytest.mark.gpu
@PRECS
def test_handle_is_untouched_and_calls_repeat(prec, workdir):
    r = Renderer(_scene("A", workdir), 0, prec)
    a, sa = r.render(stats=True)
    one = r.render_adaptive(RECTS["inner"], stats=True, **PARAMS)
    b, sb = r.render(stats=True)
    two = r.render_adaptive(RECTS["inner"], stats=True, **PARAMS)
    seven = np.full(a.shape, 7.0, a.dtype), np.full(a.shape, 7.0, a.dtype)
    r.render_adaptive(RECTS["inner"], film=seven[0], moments=seven[1], **PARAMS)      # += onto the caller's values
    r.close()
    assert a[..., :3].max() > 0 and np.array_equal(a, b)
    for key in STATS + ("tile_launches", "list_launches"):
        assert getattr(sa, key) == getattr(sb, key), key
    for x, y in zip(one[:3], two[:3]):
        assert np.array_equal(x, y)
    for key in STATS + ("camera_samples",):
        assert getattr(one[3], key) == getattr(two[3], key), key
    assert np.array_equal(seven[0], a.dtype.type(7.0) + one[0]) and np.array_equal(seven[1], a.dtype.type(7.0) + one[1])
    want = _run("A", "inner", prec, workdir)
    assert np.array_equal(one[0], want[0]) and np.array_equal(one[2], want[2])


@pytest.mark.gpu
def test_device_memory_form(workdir):
    import torch
    r = Renderer(_scene("A", workdir), 0, RRT_F32)
    film = torch.zeros((FILM[1], FILM[0], 4), dtype=torch.float32, device="cuda:0")
    mom, tiles = torch.zeros_like(film), torch.zeros((2, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = r.render_adaptive_device(RECTS["whole"], film.data_ptr(), mom.data_ptr(), tiles.data_ptr(), **PARAMS)
    r.render_adaptive_device(RECTS["whole"], film.data_ptr(), mom.data_ptr(), None, stats=False, **PARAMS)      # tile_samples may be NULL; += again
    r.close()
    want = _run("A", "whole", RRT_F32, workdir)
    assert np.array_equal(tiles.cpu().numpy().astype(np.uint32), want[2]) and st.camera_samples == want[3].camera_samples
    assert np.array_equal(film.cpu().numpy(), want[0] + want[0]) and np.array_equal(mom.cpu().numpy(), want[1] + want[1])


@pytest.mark.gpu
def test_device_side_error_paths(workdir):
    import torch
    W, H = FILM
    lib = A.lib()
    film, mom = np.full((H, W, 4), 7.0, np.float32), np.full((H, W, 4), 7.0, np.float32)
    strat = Renderer(Scene.loads(*_cfg_a(workdir, NSAMP, sampler={"sampler_type": "StratifiedSampler", "xsamp": 3, "ysamp": 4, "jitter": True, "dimension": 4})), 0, RRT_F32)
    with pytest.raises(RrtUnsupported, match="StratifiedSampler"):
        strat.render_adaptive(film=film, moments=mom, **PARAMS)
    strat.close()
    gauss = Renderer(Scene.loads(*_cfg_a(workdir, NSAMP, filt={"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0})), 0, RRT_F32)
    with pytest.raises(RrtUnsupported, match="box filter of radius 0.5"):
        gauss.render_adaptive(film=film, moments=mom, **PARAMS)
    gauss.close()
    r = Renderer(_scene("A", workdir), 0, RRT_F32)
    out = np.full((2, 4), 7.0)
    with pytest.raises(RrtError, match="whole 8 x 8 tiles"):
        r.render_adaptive((0, 0, 12, 16), film=film, moments=mom, **PARAMS)
    with pytest.raises(RrtError, match="outside the film"):
        r.render_adaptive((8, 8, 40, 16), film=film, moments=mom, **PARAMS)
    with pytest.raises(RrtError, match="whole 8 x 8 tiles"):
        r.tile_error(mom, (0, 0, 12, 16))
    with pytest.raises(RrtError, match="outside the film"):
        r.tile_error(mom, (0, 8, 32, 24))
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, frame.data_ptr())
    with pytest.raises(RrtError, match="in flight"):
        r.render_adaptive(film=film, moments=mom, **PARAMS)
    assert lib.rrt_tile_error(r._h, mom.ctypes.data, A.RRT_MEM_HOST, (C.c_int32 * 4)(0, 0, W, H), out.ctypes.data) == A.RRT_EINVAL and b"in flight" in lib.rrt_last_error()
    r.render_end()
    assert np.all(film == 7.0) and np.all(mom == 7.0) and np.all(out == 7.0)
    f2, m2, samples = r.render_adaptive(film=film, moments=mom, **PARAMS)      # and the handle still works
    r.close()
    assert f2 is film and samples.tolist() == _run("A", "whole", RRT_F32, workdir)[2].tolist()


@pytest.mark.gpu
def test_cli_adaptive(tmp_path, workdir):
    """RRT_ADAPTIVE=<threshold>: both command lines write byte-identical PNGs (frame and denoised frame) and print the same sample counts; the frame
    differs from the uniform one."""
    cfg, _ = _cfg_a(str(tmp_path), NSAMP)
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    exe = os.path.join(ROOT, "rs_ray_toy_amd", "csrc", "rrt_render")
    base = {k: v for k, v in os.environ.items() if k not in ("RRT_DENOISE", "RRT_DENOISE_MOMENTS", "RRT_AOV", "RRT_GPUS") and not k.startswith("RRT_ADAPTIVE")}
    base["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    out = {}
    for tag, cmd in (("cli", [exe]), ("py", [sys.executable, "-m", "rs_ray_toy_amd"])):
        frame, dn = tmp_path / f"{tag}.png", tmp_path / f"{tag}_dn.png"
        env = dict(base, RRT_ADAPTIVE="0.95", RRT_ADAPTIVE_MIN="4", RRT_ADAPTIVE_BATCH="4", RRT_DENOISE=str(dn), RRT_DENOISE_MOMENTS="1")
        p = subprocess.run(cmd + [str(scene), str(frame)], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr
        # the loader's diagnostics (rrt_scene_warning: here the OBJ parser's "unsupported Element" lines) go to stderr in rrt_render and to stdout in the
        # Python mirror; they are taken out by their content, every other line is compared
        out[tag] = (frame.read_bytes(), dn.read_bytes(), [l for l in p.stdout.splitlines() if not l.startswith("ParseObjError:")])
    uniform = tmp_path / "uniform.png"
    p = subprocess.run([exe, str(scene), str(uniform)], capture_output=True, text=True, timeout=600, env=base)
    assert p.returncode == 0, p.stderr
    assert out["cli"][0] == out["py"][0] and out["cli"][1] == out["py"][1] and out["cli"][2] == out["py"][2]
    assert out["cli"][0][:8] == b"\x89PNG\r\n\x1a\n" and out["cli"][0] != uniform.read_bytes()
    taken = 64 * int(_run("A", "whole", RRT_F32, workdir)[2].sum())
    assert len(out["cli"][2]) == 2 and out["cli"][2][0] == f"{taken} of {32 * 16 * K} camera samples taken (adaptive)" and out["cli"][2][1].endswith("rays generated")
