"""Lens cull table of the fp32 camera kernel (csrc/host/lens_cull.cpp), on the CPU alone.

The camera kernel drops a sample before any lens arithmetic when its cell over (r_film, p_lens) is marked dead. The builder decides that from f64
traces at the cell corners with an erosion by one cell; these tests hold it to the promise with an independent f64 restatement of
trace_lenses_from_film (camera.rs:163-211, the reference's operation order, numpy): every point of a lattice 4x denser than the builder's inside
every dead cell, cell edges included, is stopped by the lens - on the scene.json lens, perturbed copies of it and hand-built prescriptions of 2 to 64
interfaces (tests/lens_shapes.py) - and of 4 M uniform random samples per lens none that gets through lies in a dead cell. The GPU side of the promise is
tests/test_lens_cull.py and tests/test_lens_shapes.py (frames identical bit for bit).
"""
import ctypes as C
import time

import numpy as np
import pytest

import lens_shapes as LS
from rs_ray_toy_amd import RRT_FIXED_BVH, Scene, scenes
from rs_ray_toy_amd import _abi as A

KR, KX, KY = 32, 96, 96      # host/lens_cull.hpp kLcR / kLcX / kLcY
WORDS = (KX + 31) // 32


def lens_cull(scene):
    """(dead [2, KR, KY, KX] bool, r_max, inv_dr, dead share, traces, seconds) through the library's test hook, or None without a table."""
    fn = A.lib().rrt_internal_lens_cull
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    bits = np.zeros(2 * KR * KY * WORDS, np.uint32)
    info = np.zeros(5)
    rc = fn(C.addressof(scene.desc), bits.ctypes.data, info.ctypes.data)
    if rc == 1:
        return None
    assert rc == 0
    dead = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(2, KR, KY, WORDS * 32)[..., :KX].astype(bool)
    return dead, info[0], info[1], info[2], int(info[3]), info[4]


def _nrm(x, y, z):
    l = np.sqrt(x * x + y * y + z * z)
    l = np.where(l == 0.0, 1.0, l)
    return x / l, y / l, z / l


def trace_through(elems, rf, plx, ply):
    """f64 trace_lenses_from_film of film point (rf, 0, 0) towards the rear point (plx, ply, rear_z) (the frame turned by the film point's polar
    angle, camera.rs:505-513): True where the ray gets through every interface."""
    with np.errstate(all="ignore"):
        return _trace_through(elems, rf, plx, ply)


def _trace_through(elems, rf, plx, ply):
    n = len(elems)
    ox, oy, oz = rf.copy(), np.zeros_like(rf), np.zeros_like(rf)
    dx, dy, dz = _nrm(plx - rf, ply, np.full_like(rf, elems[n - 1][1]))
    dz = -dz
    idx = np.arange(rf.size)
    element_z = 0.0
    for i in range(n - 1, -1, -1):
        cr, th, eta_i, ap = elems[i]
        element_z -= th
        if cr == 0.0:
            keep = dz < 0.0
            t = np.where(keep, (element_z - oz) / np.where(keep, dz, -1.0), -1.0)
        else:
            zc = element_z + cr
            ocx, ocy, ocz = ox, oy, oz - zc
            a = dx * dx + dy * dy + dz * dz
            b = 2.0 * (dx * ocx + dy * ocy + dz * ocz)
            c = ocx * ocx + ocy * ocy + ocz * ocz - cr * cr
            disc = b * b - 4.0 * a * c
            keep = disc >= 0.0
            root = np.sqrt(np.where(keep, disc, 0.0))
            q = np.where(b < 0.0, -0.5 * (b - root), -0.5 * (b + root))
            t0 = q / a
            t1 = c / q
            closer = (dz > 0.0) ^ (cr < 0.0)
            t = np.where(closer, np.fmin(t0, t1), np.fmax(t0, t1))
            t = np.where(keep, t, -1.0)
        keep = t >= 0.0
        px, py, pz = ox + dx * t, oy + dy * t, oz + dz * t
        keep &= px * px + py * py < ap * ap
        if cr != 0.0:
            nx, ny, nz = _nrm(ocx + dx * t, ocy + dy * t, ocz + dz * t)
            flip = nx * -dx + ny * -dy + nz * -dz < 0.0
            nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
            eta_t = elems[i - 1][2] if i > 0 and elems[i - 1][2] != 0.0 else 1.0
            eta = eta_i / eta_t
            wx, wy, wz = _nrm(-dx, -dy, -dz)
            cos_i = nx * wx + ny * wy + nz * wz
            sin2_t = eta * eta * np.fmax(0.0, 1.0 - cos_i * cos_i)
            keep &= sin2_t < 1.0
            cos_tt = np.sqrt(np.where(keep, 1.0 - sin2_t, 0.0))
            k = eta * cos_i - cos_tt
            dx, dy, dz = -wx * eta + nx * k, -wy * eta + ny * k, -wz * eta + nz * k
        ox, oy, oz = px[keep], py[keep], pz[keep]
        dx, dy, dz = dx[keep], dy[keep], dz[keep]
        idx = idx[keep]
        if idx.size == 0:
            break
    out = np.zeros(rf.size, bool)
    out[idx] = True
    return out


def _elems(scene):
    cam = scene.desc.camera
    return [(cam.elems[i].curvature_radius, cam.elems[i].thickness, cam.elems[i].eta, cam.elems[i].aperture_radius) for i in range(cam.n_elems)]


def _random_lens_cfg(wd, seed):
    """scene.json's double Gauss with every radius, thickness and aperture perturbed, a random stop and focus distance (as
    tests/test_gpu_parity.py's random prescriptions)."""
    rng = np.random.default_rng(seed)
    cfg, root = scenes.cfg2(wd, xres=256, yres=160, nsamp=9, max_depth=2)
    ld = np.array(scenes.LENS_DATA, float).reshape(-1, 4)
    ld[:, 0] *= rng.uniform(0.85, 1.15, len(ld))
    ld[:, 1] *= rng.uniform(0.8, 1.2, len(ld))
    ld[:, 3] *= rng.uniform(0.7, 1.1, len(ld))
    cfg["Camera"]["lens_data"] = [float(x) for x in ld.reshape(-1)]
    cfg["Camera"]["aperture_diameter"] = float(rng.uniform(8.0, 50.0))
    cfg["Camera"]["focus_distance"] = float(rng.uniform(10.0, 60.0))
    return cfg, root


CASES = {
    "scene_json_lens": lambda wd: scenes.cfg4(wd, xres=1024, yres=1024, nsamp=5, max_depth=2, n=8),
    "tiny_film": lambda wd: scenes.cfg2(wd, xres=24, yres=16, nsamp=9, max_depth=2),
    "random_lens_1": lambda wd: _random_lens_cfg(wd, 1),
    "random_lens_5": lambda wd: _random_lens_cfg(wd, 5),
}
# hand-built prescriptions (tests/lens_shapes.py): 2, 3, 5 and 64 rows, a stop at index 0, total internal reflection inside the rim
CASES.update({name: (lambda wd, name=name: LS.sample_scene(wd, name, xres=256, yres=160)) for name in ("singlet_2", "stop_front_3", "two_singlets_5", "strong_singlet_2", "padded_64")})


@pytest.mark.parametrize("which", sorted(CASES))
def test_dead_cells_are_dead_on_a_denser_lattice(which, workdir):
    cfg, root = CASES[which](workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    got = lens_cull(sc)
    assert got is not None
    dead, r_max, inv_dr, share, traces, secs = got
    print(f"{which}: lens cull table in {secs * 1e3:.1f} ms ({traces} f64 traces), {share:.3f} of the cells dead")
    assert np.float32(inv_dr) == np.float32(KR / r_max)
    elems = _elems(sc)
    assert dead.any(), "no cell culled"
    cam, film = sc.desc.camera, sc.desc.film
    dr = r_max / KR
    sub = np.linspace(0.0, 1.0, 5)                      # 4x the builder's lattice (the cell corners), edges included
    su, sv, sw = np.meshgrid(sub, sub, sub, indexing="ij")
    su, sv, sw = su.ravel(), sv.ravel(), sw.ravel()
    for b in range(2):
        pb = list(cam.exit_pupil_bounds[0 if b == 0 else 63])
        cells = np.argwhere(dead[b])                    # (cr, cy, cx)
        if cells.size == 0:
            continue
        # the kernel chooses box 63 at r_film >= diagonal / 2: a dead cell of a box lies (up to the builder's 1e-4 tolerance) where that box is chosen
        r_lo, r_hi = cells[:, 0] * dr, (cells[:, 0] + 1) * dr
        if b == 0:
            assert np.all(r_lo < film.diagonal / 2 * (1 + 1e-4))
        else:
            assert np.all(r_hi > film.diagonal / 2 * (1 - 1e-4))
        for c0 in range(0, len(cells), 16384):
            cc = cells[c0:c0 + 16384]
            rf = ((cc[:, 0:1] + su[None]) * dr).ravel()
            lx = (0.5 + (cc[:, 2:3] + sv[None]) / KX).ravel()
            ly = (0.5 + (cc[:, 1:2] + sw[None]) / KY).ravel()
            plx = pb[0] * (1.0 - lx) + pb[2] * lx
            ply = pb[1] * (1.0 - ly) + pb[3] * ly
            through = trace_through(elems, rf, plx, ply)
            assert not through.any(), f"box {b}: {int(through.sum())} lattice points of dead cells get through, e.g. cell {cc[np.argmax(through) // su.size]}"
    if which == "padded_64":      # open stop planes behind the real stop: the builder traces the same lens, and the table is the double Gauss's bit for bit
        cfg13, root13 = LS.sample_scene(workdir, "double_gauss_13", xres=256, yres=160)
        dead13, r_max13, inv_dr13, *_ = lens_cull(Scene.loads(cfg13, root13, flags=RRT_FIXED_BVH))
        assert r_max13 == r_max and inv_dr13 == inv_dr and np.array_equal(dead13, dead)


def test_the_table_culls_what_it_should(workdir):
    """The table is worth its load: on the scene.json lens about two thirds of the (r_film, p_lens) cells are dead (69 % of the samples die in the
    lens, Q5), and the cells the f64 trace finds open on their whole lattice are never marked dead."""
    cfg, root = CASES["scene_json_lens"](workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    t0 = time.perf_counter()
    dead, r_max, inv_dr, share, traces, secs = lens_cull(sc)
    assert time.perf_counter() - t0 < 5.0
    assert 0.55 < share < 0.8, share
    # open cells: the centre of each cell of box 0 below the switch radius; a dead cell's centre must be dead
    dr = r_max / KR
    cr, cy, cx = np.meshgrid(np.arange(KR), np.arange(KY), np.arange(KX), indexing="ij")
    use = (cr + 1) * dr < sc.desc.film.diagonal / 2
    pb = list(sc.desc.camera.exit_pupil_bounds[0])
    lx, ly = 0.5 + (cx[use] + 0.5) / KX, 0.5 + (cy[use] + 0.5) / KY
    through = trace_through(_elems(sc), (cr[use] + 0.5) * dr, pb[0] * (1.0 - lx) + pb[2] * lx, pb[1] * (1.0 - ly) + pb[3] * ly)
    assert not (through & dead[0][use]).any()
    assert through.mean() > 0.2 and (~dead[0][use]).mean() > through.mean()


RANDOM_CASES = {
    "double_gauss_13": {},
    "double_gauss_13_diagonal_70": dict(diagonal=70),
    "double_gauss_13_aperture_2": dict(aperture_diameter=2),
    "singlet_2": {},
    "two_singlets_5": {},
    "stop_front_3_aperture_3": dict(aperture_diameter=3),
}


@pytest.mark.parametrize("which", sorted(RANDOM_CASES))
def test_no_random_sample_passes_in_a_dead_cell(which, workdir):
    """4 M uniform (r_film, p_lens) samples over the table's domain, the exit-pupil box chosen as the kernel chooses it, traced in f64: none that gets
    through lies in a dead cell. The lattice test above cannot see a passing sliver thinner than a quarter cell; this one can."""
    name = which.split("_diagonal")[0].split("_aperture")[0]
    cfg, root = LS.sample_scene(workdir, name, xres=256, yres=160, **RANDOM_CASES[which])
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    dead, r_max, inv_dr, share, traces, secs = lens_cull(sc)
    assert dead.any(), "no cell culled"
    elems, cam, film = _elems(sc), sc.desc.camera, sc.desc.film
    rng = np.random.default_rng(20)
    n_through = n_dead = 0
    for _ in range(8):
        n = 500_000
        rf, lx, ly = rng.random(n) * r_max, 0.5 + rng.random(n), 0.5 + rng.random(n)
        box = (rf / (film.diagonal / 2.0) >= 1.0).astype(int)      # rg_begin_lean's choice (Q6)
        pb = np.array([list(cam.exit_pupil_bounds[0]), list(cam.exit_pupil_bounds[63])])[box]
        through = trace_through(elems, rf, pb[:, 0] * (1.0 - lx) + pb[:, 2] * lx, pb[:, 1] * (1.0 - ly) + pb[:, 3] * ly)
        cr, cx, cy = np.minimum((rf * (KR / r_max)).astype(int), KR - 1), np.minimum(((lx - 0.5) * KX).astype(int), KX - 1), np.minimum(((ly - 0.5) * KY).astype(int), KY - 1)
        in_dead = dead[box, cr, cy, cx]
        n_through += int(through.sum()); n_dead += int(in_dead.sum())
        bad = through & in_dead
        assert not bad.any(), f"{int(bad.sum())} passing samples in dead cells, e.g. r_film {rf[bad][0]}, p_lens ({lx[bad][0]}, {ly[bad][0]}), box {box[bad][0]}"
    print(f"{which}: {share:.3f} of the cells dead; of 4 M samples {n_through} get through, {n_dead} lie in dead cells, none does both")
    assert n_through > 0 and n_dead > 0
