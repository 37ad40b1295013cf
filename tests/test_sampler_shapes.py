"""The samplers on hand-built sampler tables (tests/sampler_shapes.py): film, index, dimension.

Three statements of the HaltonSampler are held to each other bit for bit: the device's (rrt_sampler_values, the unit-test surface over
halton_pixel_offset / draw_1d / draw_2d of device/dmath.hpp; rrt_camera_samples for the camera kernels' own route, halton_cam4 and the pix_off
kernels; rrt_irradiance_rays for k_irr_gen), the oracle's (oracle_sampler_values) and a plain Python one written from the reference alone
(tests/sampler_reference.py). The StratifiedSampler's counter-based generator has no reference to replay (the reference draws from thread_rng), so
the oracle's restatement is held to the structure samplers/stratified.rs promises, and the device to the oracle.

There is no tolerance in this file: every comparison is array_equal.

CPU: reference against oracle and the description's fields over every Halton shape; the host's division magics and block tables at the points no
probe reaches (tools/sampler_tables_check.cpp); the Stratified structure. GPU: both handles against both, the fp32
handle as created, with "halton_tables" off and with "cam_tables" off; the camera dimensions probe by probe; the refusals.

The one place where the issue's wording could not be taken literally: rrt_irradiance_rays hands out normalize(wl), and the length of wl rounds to
1 - 2^-53 or 1 + 2^-52 for some draws, so d.z is 1 - 2 u0 to within an ulp, not to the bit. Dimension 0 is a multiple of 2^-32 (a reversed 32-bit
word), so the test recovers that integer from d.z - exact for an error below 2^-34, a million ulps - and compares integers with array_equal.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import sampler_reference as SR
import sampler_shapes as SS
from rs_ray_toy_amd import _abi as A
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError, RrtUnsupported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs_ray_toy_amd", "csrc")

PRECS = pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
HALTON = pytest.mark.parametrize("name", list(SS.HALTON))
STRATIFIED = pytest.mark.parametrize("name", list(SS.STRATIFIED))

_halton = {}
_stratified = {}


def _halton_case(name, workdir):
    """scene, probes, and per range the reference's answer - computed once, read-only, shared by every test of the shape"""
    if name not in _halton:
        s = SS.HALTON[name]
        sc = SS.halton_scene(workdir, name)
        ref = SR.Halton.of_scene(sc)
        px, sn = SS.probes(*s["film"], s["nsamp"])
        want = {rg: ref.values(px, sn, *rg) for rg in SS.RANGES}
        for arrs in want.values():
            for a in arrs: a.setflags(write=False)
        _halton[name] = dict(scene=sc, ref=ref, px=px, sn=sn, want=want)
    return _halton[name]


def _stratified_case(name, workdir):
    if name not in _stratified:
        s = SS.STRATIFIED[name]
        sc = SS.stratified_scene(workdir, name)
        px, sn = SS.st_probes(s)
        want = O.sampler_values(sc, px, sn, *SS.ST_RANGE)
        for a in want: a.setflags(write=False)
        _stratified[name] = dict(scene=sc, px=px, sn=sn, want=want)
    return _stratified[name]


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- CPU: the table itself ------------------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_what_it_says():
    assert len(SS.HALTON) == 2 * len(SS.FILMS) + len(SS.LARGEST) + 1 and len(SS.STRATIFIED) == 30
    assert SS.HALTON["128x82_n138083"]["nsamp"] == 138083 and SS.HALTON["128x1_n33554430"]["nsamp"] == 33554430
    assert (SS.table_block(5), SS.table_block(7), SS.table_block(11), SS.table_block(311)) == (5 ** 7, 7 ** 6, 11 ** 4, 311 ** 2)
    # the largest-nsamp shapes reach every edge, the 21st base-3 digit of dimension 1 included, and stop short of 2^32
    for name, scale1 in (("128x82_n138083", 243), ("128x1_n33554430", 1)):
        s = SS.HALTON[name]
        stride = 128 * scale1
        sn = SS.sample_numbers(*s["film"], s["nsamp"])
        for e in SS.edges(scale1):
            if e < stride * s["nsamp"]: assert any(k * stride < e for k in sn) and any(e <= k * stride < e + 2 * stride for k in sn), (name, e)
        assert stride * (s["nsamp"] + 1) < 2 ** 32 <= stride * (s["nsamp"] + 2)
    assert 3 ** 20 < 128 * 33554429 and 3 ** 21 > 2 ** 32      # 128x1: the reversed digits of dimension 1 pass 2^32
    for w, h in SS.FILMS:
        px = SS.pixels(w, h)
        assert {(0, 0), (w - 1, h - 1)} <= set(px) and len(px) <= 32
        if w > 128: assert {(127, 0), (128, 0)} <= set(px)
        if h > 128: assert {(0, 127), (0, 128)} <= set(px)
    films = {s["film"] for s in SS.STRATIFIED.values()}
    assert films == set(SS.ST_FILMS) and {s["seed"] for s in SS.STRATIFIED.values()} == set(SS.ST_SEEDS)
    assert max(y * 2048 + x for x, y in SS.st_pixels(2048, 2048)) == 2 ** 22 - 1


# ---- CPU: HaltonSampler, the Python reference against the oracle and the description --------------------------------------------------------------------
@HALTON
def test_reference_equals_oracle_and_desc(name, workdir):
    c = _halton_case(name, workdir)
    sc, ref, px, sn = c["scene"], c["ref"], c["px"], c["sn"]
    ref.check_desc(sc.desc)
    assert len(sn) <= 600
    for rg in SS.RANGES:
        index, v1, v2 = c["want"][rg]
        assert _same(O.sampler_values(sc, px, sn, *rg), (index, v1, v2)), rg
        assert v1.min() >= 0.0 and v1.max() < 1.0 and v2.min() >= 0.0 and v2.max() < 1.0
        assert int(index.max()) < 2 ** 32
    # the single-value surfaces the older tests use say the same
    for i in range(0, len(sn), 7):
        assert O.halton_index(sc, int(px[i, 0]), int(px[i, 1]), int(sn[i])) == int(c["want"][SS.RANGES[0]][0][i])
    # Dimensions 0 and 1 name the pixel (modulo 128, modulo the base scale) where the reference's own numbers let them: get_index_for_sample takes
    # base_exponents[1] digits for x too (Q24), enough only if base_exponents[0] <= base_exponents[1]; and multiplicative_inverse's `x as u64` turns a
    # negative x into 2^64 + x, which is no inverse modulo a power of 3 (1x7: the "inverse" of 1 modulo 9 is 8). Where either fails the reference
    # itself does not name the pixel: counted, not asserted.
    if not SS.HALTON[name]["center"]:
        # (the radical inverse of the whole index times the base scale, floored, is the reversed low digits of the index - the digits that
        # sample_dimension strips before it makes the offset inside the pixel - so the integers are compared: no float sits on a cell edge)
        index = [int(i) for i in c["want"][SS.RANGES[0]][0]]
        s0, s1 = ref.base_scales
        e0, e1 = ref.base_exponents
        inverse = [n == 1 or a * m % n == 1 for a, n, m in ((s1, s0, ref.mult_inverse[0]), (s0, s1, ref.mult_inverse[1]))]
        names = [np.array([SR.inverse_radical_inverse(2, i % s0, e0) for i in index]) == (px[:, 0] % 128) % s0,
                 np.array([SR.inverse_radical_inverse(3, i % s1, e1) for i in index]) == (px[:, 1] % 128) % s1]
        for i, enough in enumerate((ref.base_exponents[0] <= ref.base_exponents[1], True)):
            if enough and inverse[i]: assert names[i].all(), i
            else: print(f"{name}: base_exponents {ref.base_exponents}, mult_inverse {ref.mult_inverse} (true inverses: {inverse}): dimension {i} names its "
                        f"pixel coordinate for {int(names[i].sum())} of {len(names[i])} probes")
    else:
        assert np.all(c["want"][SS.RANGES[0]][1][:, :2] == 0.5)


def test_reference_permutations_and_primes(workdir):
    c = _halton_case("2x3_n2", workdir)
    c["ref"].check_perms()
    assert SR.PRIMES[:5] == [2, 3, 5, 7, 11] and SR.PRIMES[63] == 311 and SR.PRIMES[998] == 7907 and SR.PRIMES[999] == 7919
    assert SR.PRIME_SUMS[:4] == [0, 2, 5, 10] and SR.PRIME_SUMS[999] + 7919 == len(c["ref"].perms)
    assert SR.multiplicative_inverse(243, 128) == 59 and SR.multiplicative_inverse(128, 243) == 131      # DESIGN.md's cfg films
    for a, n in ((243, 128), (81, 128), (27, 64), (3, 4), (1, 8)):      # 2^64 is a multiple of a power of 2: the u64 cast of a negative x does no harm
        assert a * SR.multiplicative_inverse(a, n) % n == 1, (a, n)
    # extended_gcd(1, 9) gives x = -8; as u64 that is 2^64 - 8, and 2^64 = 7 (mod 9): 8, where the inverse of 1 is 1 (worked by hand from halton.rs:131-150)
    assert SR.extended_gcd(1, 9)[0] == -8 and SR.multiplicative_inverse(1, 9) == 8


def test_host_tables_divide_exactly():
    """tools/sampler_tables_check.cpp, built and run on every (base scales, nsamp) of the table: the division magics of all 1000 bases and of every
    table block at the points where a wrong magic number shows first (the probes above cannot see one that is off by a few units), the block tables'
    reach and their entries against the digit loop. No GPU and no sanitizer: a plain program over the host objects."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "sampler_tables_check"])
    films = sorted({(*SS.scales(*s["film"]), s["nsamp"]) for s in SS.HALTON.values()})
    run = subprocess.run([os.path.join(ROOT, "build", "sampler_tables_check", "sampler_tables_check")] + [str(v) for f in films for v in f], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0 and "sampler_tables_check: ok" in run.stdout, run.stdout[-3000:] + run.stderr[-1000:]
    assert run.stdout.count("1000 dividers") == len(films) and "62 block tables" in run.stdout


# ---- CPU: StratifiedSampler, the oracle's generator against the structure stratified.rs promises ---------------------------------------------------------
def _strata_of(name, workdir, seed=None):
    """per probed pixel: the stratum each sample number lands in, 1D (pixels, spp, dimension) and 2D, and the values"""
    s = SS.STRATIFIED[name]
    if seed is None:
        c = _stratified_case(name, workdir)
        px, sn, (index, v1, v2) = c["px"], c["sn"], c["want"]
    else:
        px, sn = SS.st_probes(s)
        index, v1, v2 = O.sampler_values(SS.stratified_scene(workdir, name, seed=seed), px, sn, *SS.ST_RANGE)
    nx, ny = s["strata"]
    spp, npx = nx * ny, len(sn) // (nx * ny)
    v1 = v1.reshape(npx, spp, -1); v2 = v2.reshape(npx, spp, -1, 2)
    return index.reshape(npx, spp), v1, v2, px.reshape(npx, spp, 2)[:, 0]


@STRATIFIED
def test_stratified_structure(name, workdir):
    s = SS.STRATIFIED[name]
    (nx, ny), dim, (w, h) = s["strata"], s["dimension"], s["film"]
    spp = nx * ny
    index, v1, v2, pix = _strata_of(name, workdir)
    assert np.array_equal(index, ((pix[:, 1] * w + pix[:, 0])[:, None] << 10) | np.arange(spp)[None, :])
    below1, below2 = v1[:, :, :dim], v2[:, :, :dim]
    j1 = np.floor(below1 * spp).astype(np.int64)
    jx, jy = np.floor(below2[..., 0] * nx).astype(np.int64), np.floor(below2[..., 1] * ny).astype(np.int64)
    every = np.arange(spp)[None, :, None]
    # within a dimension below `dimension`, the nx * ny samples of a pixel hit every stratum exactly once, and each value lies in its cell
    assert np.array_equal(np.sort(j1, axis=1), np.broadcast_to(every, j1.shape))
    assert np.array_equal(np.sort(jy * nx + jx, axis=1), np.broadcast_to(every, jx.shape))
    assert below1.min() >= 0.0 and below1.max() < 1.0 and below2.min() >= 0.0 and below2.max() < 1.0
    assert np.all(j1 <= below1 * spp) and np.all(below1 * spp < j1 + 1) and np.all(jx <= below2[..., 0] * nx) and np.all(below2[..., 0] * nx < jx + 1)
    assert np.all(jy <= below2[..., 1] * ny) and np.all(below2[..., 1] * ny < jy + 1)
    if not s["jitter"]:      # cell centres, by the generator's own two operations
        assert np.array_equal(below1, (j1 + 0.5) * (1.0 / spp))
        assert np.array_equal(below2[..., 0], (jx + 0.5) * (1.0 / nx)) and np.array_equal(below2[..., 1], (jy + 0.5) * (1.0 / ny))
    elif spp > 1:
        assert len(np.unique(below1 * spp - j1)) > below1.size // 2      # the jitter is not one number
    # counters at and past `dimension`: rng.gen_range(-1.0..1.0)
    past1, past2 = v1[:, :, dim:], v2[:, :, dim:]
    assert past1.shape[2] == SS.ST_RANGE[1] - dim and past1.min() >= -1.0 and past1.max() < 1.0 and past2.min() >= -1.0 and past2.max() < 1.0
    if past1.size >= 64: assert past1.min() < 0.0 < past1.max() and past2.min() < 0.0 < past2.max()
    # two pixels, two counters, two seeds, and the 1D and the 2D counter of one number, do not share a permutation (nor, past `dimension`, a value)
    # (7 strata have 5040 orders, so single permutations may coincide by chance: a pixel's, a counter's and a seed's permutations are compared as sets)
    other = _strata_of(name, workdir, seed=SS.ST_SEEDS[0] if s["seed"] == SS.ST_SEEDS[1] else SS.ST_SEEDS[1])
    if spp > 1:
        J = np.concatenate([j1, jy * nx + jx], axis=2)      # (pixels, sample numbers, 1D counters then 2D counters)
        o2 = other[2][:, :, :dim]
        JO = np.concatenate([np.floor(other[1][:, :, :dim] * spp), np.floor(o2[..., 1] * ny) * nx + np.floor(o2[..., 0] * nx)], axis=2).astype(np.int64)
        assert not any(np.array_equal(J[p], J[q]) for p in range(len(J)) for q in range(p))
        assert not any(np.array_equal(J[:, :, a], J[:, :, b]) for a in range(2 * dim) for b in range(a))
        assert not np.array_equal(J, JO) and np.array_equal(np.sort(JO, axis=1), np.broadcast_to(every, JO.shape))
    flat = np.concatenate([past1.ravel(), past2.ravel(), other[1][:, :, dim:].ravel(), other[2][:, :, dim:].ravel()])
    assert len(np.unique(flat)) > 0.99 * flat.size      # 32-bit hashes: a handful of birthday collisions at most


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
def _settings(prec):
    """the ways a handle is run: (label, options to set first)"""
    if prec == RRT_F64: return (("as created", ()),)
    return (("as created", ()), ("halton_tables off", (("halton_tables", 0),)), ("cam_tables off", (("halton_tables", 1), ("cam_tables", 0))))


@pytest.mark.gpu
@PRECS
@HALTON
def test_halton_values_on_the_device(name, prec, workdir):
    c = _halton_case(name, workdir)
    sc, px, sn = c["scene"], c["px"], c["sn"]
    oracle = {rg: O.sampler_values(sc, px, sn, *rg) for rg in SS.RANGES}
    r = Renderer(sc, 0, prec)
    got = {(label, rg): (_set(r, opts), r.sampler_values(px, sn, *rg))[1] for label, opts in _settings(prec) for rg in SS.RANGES}
    r.close()
    for (label, rg), g in got.items():
        for what, a, w, o in zip(("index", "v1", "v2"), g, c["want"][rg], oracle[rg]):
            assert np.array_equal(a, w), f"{name} {label} {rg}: {what} differs from the Python reference at {np.argwhere(a != w)[:4].tolist()}"
            assert np.array_equal(a, o), f"{name} {label} {rg}: {what} differs from the oracle"


def _set(r, opts):
    for k, v in opts: r.set_option(k, v)


def _camera_dims(r, px, sn):
    out = np.zeros((len(sn), 5))
    for i, ((x, y), s) in enumerate(zip(px.tolist(), sn.tolist())):
        out[i] = r.camera_samples((x, y, x + 1, y + 1), s, s + 1)[0][0]
    return out


@pytest.mark.gpu
@PRECS
@HALTON
def test_camera_dimensions_on_the_device(name, prec, workdir):
    """rrt_camera_samples' dims5 = dimensions 0 .. 4 of the reference, one 1 x 1 rect and one sample number per probe: the fp32 handle's camera
    kernels (halton_cam4, the pix_off kernels) with their tables on and off, the f64 handle's k_raygen"""
    c = _halton_case(name, workdir)
    want = c["want"][SS.RANGES[0]][1][:, :5]
    r = Renderer(c["scene"], 0, prec)
    got = {}
    for label, opts in _settings(prec):
        if label == "halton_tables off": continue
        _set(r, opts)
        got[label] = _camera_dims(r, c["px"], c["sn"])
    r.close()
    for label, g in got.items():
        bad = np.argwhere(g != want)
        assert np.array_equal(g, want), (f"{name} {label}: {len(bad)} values differ, first (probe, dimension) {bad[:4].tolist()}: pixel {c['px'][bad[0, 0]].tolist()} "
                                         f"sample {int(c['sn'][bad[0, 0]])} got {g[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")


@pytest.mark.gpu
@PRECS
@STRATIFIED
def test_stratified_values_on_the_device(name, prec, workdir):
    c = _stratified_case(name, workdir)
    sc, px, sn = c["scene"], c["px"], c["sn"]
    s = SS.STRATIFIED[name]
    spp = s["strata"][0] * s["strata"][1]
    r = Renderer(sc, 0, prec)
    got = r.sampler_values(px, sn, *SS.ST_RANGE)
    dims = np.concatenate([r.camera_samples((x, y, x + 1, y + 1), 0, spp)[0] for x, y in px.reshape(-1, spp, 2)[:, 0].tolist()])
    r.close()
    for what, a, w in zip(("index", "v1", "v2"), got, c["want"]):
        assert np.array_equal(a, w), f"{name}: {what} differs from the oracle"
    # get_camerasample: film 2D, lens 2D, time 1D = 2D counters 0 and 1, 1D counter 0
    index, v1, v2 = c["want"]
    assert np.array_equal(dims, np.concatenate([v2[:, 0], v2[:, 1], v1[:, :1]], 1))


@pytest.mark.gpu
def test_irradiance_rays_draw_from_the_same_table(workdir):
    """k_irr_gen, the third user of halton_pixel_offset: the sphere-mode direction of draw j of a point with pixel P is uniform_sample_sphere of
    dimensions 0 and 1 of stream (P, j), so d.z = 1 - 2 u0 before the normalisation (see the module docstring for what that leaves of it)"""
    name = "64x27_n65"
    c = _halton_case(name, workdir)
    ref, nsamp = c["ref"], SS.HALTON[name]["nsamp"]
    pix = np.array(SS.pixels(*SS.HALTON[name]["film"]), np.int64)
    r = Renderer(c["scene"], 0, RRT_F64)
    od = r.irradiance_rays(np.zeros((len(pix), 3)), None, 1, nsamp, pixel=pix, mode="sphere")
    r.close()
    assert od.shape == (len(pix), nsamp - 1, 6)
    u0 = np.array([[ref.dim(ref.index(int(x), int(y), s), 0) for s in range(1, nsamp)] for x, y in pix])
    want = u0 * 2.0 ** 32
    assert np.array_equal(want, np.round(want)) and len(np.unique(want)) > want.size // 2
    z = od[..., 5]
    print(f"irradiance z: {int((z == 1.0 - 2.0 * u0).sum())} of {z.size} draws equal 1 - 2 u0 to the bit; largest difference {np.abs(z - (1.0 - 2.0 * u0)).max():.3e}")
    assert np.array_equal(np.round((1.0 - z) * 0.5 * 2.0 ** 32), want)
    assert np.abs(np.linalg.norm(od[..., 3:], axis=-1) - 1.0).max() < 1e-15


@pytest.mark.gpu
@PRECS
@pytest.mark.parametrize("name", [n for n, s in SS.HALTON.items() if s["nsamp"] > 65])
def test_one_more_sample_is_unsupported(name, prec, workdir):
    """stride * (nsamp + 1) < 2^32 is the host's rule: the largest shape's film with one sample more is RRT_EUNSUP, from the host"""
    sc = SS.halton_scene(workdir, name, extra_samples=1)
    assert int(sc.desc.sampler.sample_stride) * (int(sc.desc.sampler.samples_per_pixel) + 1) >= 2 ** 32
    r = Renderer(sc, 0, prec)
    for call in (lambda: r.sampler_values(np.zeros((1, 2), np.int64), np.zeros(1, np.int64), 0, 4), lambda: r.camera_samples((0, 0, 1, 1), 0, 1)):
        with pytest.raises(RrtUnsupported) as e:
            call()
        assert "Halton sample index exceeds 32 bits" in str(e.value)
    r.close()


@pytest.mark.gpu
@PRECS
def test_refusals_and_the_handle_is_left_as_it_was(prec, workdir):
    lib = A.lib()
    c = _halton_case("64x27_n65", workdir)
    sc, nsamp = c["scene"], 65
    r = Renderer(sc, 0, prec)
    before = r.render()
    assert before[..., 3].max() > 0
    pixel = np.array([5 << 16 | 9, 26 << 16 | 63], np.uint32); sample = np.array([0, nsamp - 1], np.uint32)
    index = np.full(2, 7, np.uint64); v1 = np.full((2, 70), 3.5); v2 = np.full((2, 70, 2), 3.5)

    def call(h=r._h, pixel=pixel, sample=sample, n=2, first=0, count=4, index=index, v1=v1, v2=v2):
        ptr = lambda a: None if a is None else a.ctypes.data
        return lib.rrt_sampler_values(h, ptr(pixel), ptr(sample), n, first, count, ptr(index), ptr(v1), ptr(v2))

    for kw, substr in ((dict(h=None), "null handle"), (dict(pixel=None), "null argument"), (dict(sample=None), "null argument"), (dict(v1=None), "null argument"),
                       (dict(v2=None), "null argument"), (dict(n=0), "n must be > 0"), (dict(count=0), "count must be > 0"),
                       (dict(pixel=np.array([5 << 16 | 9, 26 << 16 | 64], np.uint32)), "pixel outside the film (stream 1)"),
                       (dict(pixel=np.array([27 << 16 | 9, 0], np.uint32)), "pixel outside the film (stream 0)"),
                       (dict(sample=np.array([0, nsamp], np.uint32)), "sample_num outside 0 .. nsamp-1 (stream 1)"),
                       (dict(first=930, count=70), "reaches Halton dimension 1000"), (dict(first=999, count=1), "reaches Halton dimension 1000"),
                       (dict(first=0xffffffff, count=2), "reaches Halton dimension 1000")):
        assert call(**kw) == A.RRT_EINVAL, kw
        assert substr in lib.rrt_last_error().decode(), (kw, lib.rrt_last_error())
    assert np.all(index == 7) and np.all(v1 == 3.5) and np.all(v2 == 3.5)      # nothing was written
    assert call(index=None) == A.RRT_OK and np.all(index == 7) and not np.any(v1[0, :4] == 3.5)
    assert call(first=930, count=69, v1=np.zeros((2, 69)), v2=np.zeros((2, 69, 2))) == A.RRT_OK      # up to the pair (998, 999)
    got = r.sampler_values(c["px"], c["sn"], *SS.RANGES[0])
    after = r.render()      # a frame raises on any device error bit: none was set, and nothing of the handle's state moved
    r.close()
    assert _same(got, c["want"][SS.RANGES[0]]) and np.array_equal(after, before)

    # StratifiedSampler: a counter of 4095 is the device's limit (ERR_ST_DIMS)
    cs = _stratified_case("3x5_j1_d4", workdir)
    r = Renderer(cs["scene"], 0, prec)
    before = r.render()
    px, sn = cs["px"][:15], cs["sn"][:15]
    with pytest.raises(RrtError) as e:
        r.sampler_values(px, sn, 4072, 24)
    assert type(e.value) is RrtError and "reaches Stratified counter 4095" in str(e.value)
    with pytest.raises(RrtError) as e:
        r.sampler_values(px, np.full(15, 15), 0, 4)
    assert "sample_num outside 0 .. nsamp-1 (stream 0)" in str(e.value)
    _, v1, v2 = r.sampler_values(px, sn, 4071, 24)      # counters 4071 .. 4094: past `dimension`, gen_range(-1.0..1.0)
    after = r.render()
    r.close()
    assert v1.min() >= -1.0 and v1.max() < 1.0 and v2.min() < 0.0 < v2.max() and np.array_equal(after, before)
