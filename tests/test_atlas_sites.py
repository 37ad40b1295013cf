"""Lightmap sites (rrt_atlas_sites, include/rrt.h) and the chain atlas -> sites -> records -> irradiance.

CPU: the brute-force reference (surface_reference.atlas_brute) on the dyadic patch - a flat 8 x 8-quad patch with vt = (i / 8, j / 8) - covers every
texel of a 16 x 16 atlas, reconstructs each texel centre from (owner, beta) to 1e-15, and gives the lower index on every diagonal tie.
GPU, both precisions:
  test_atlas_against_brute_force   16 x 16: centres fall exactly on quad diagonals and every product is exact - owner and beta identical; 24 x 16: nothing
                                   is dyadic - owner identical wherever the reference's smallest |edge value| exceeds 1e-12 (it leaves out none at this
                                   shape), beta within its bar; n_covered; a list of every second triangle; the cube of the cfg3 case, whose 12 entries
                                   without vt all cover the same half square: the first list entry owns it, and reversing the list reverses it
  test_the_chain_composes          atlas_sites -> surface_at -> irradiance with every intermediate in device memory equals, bit for bit, the three
                                   calls through host arrays; uncovered texels give dead records and zero sums; bake_irradiance resolves those numbers
  test_atlas_refusals              each by its message
BETA_BAR is 16 x the largest deviation of b1 / b2 measured on an MI355X against the reference rounded once to the handle's type
(profiles/surface_gpu_tests.txt): the kernels' doubles are not contracted, so they form the reference's own bits.
"""
import ctypes as C

import numpy as np
import pytest

import surface_reference as SR
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtError, resolve_irradiance
from rs_ray_toy_amd import _abi as A

PRECS = pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
BETA_BAR = {RRT_F64: 16 * 0.0, RRT_F32: 16 * 0.0}     # measured 0 in both modes at 24 x 16


def _name(prec):
    return "f64" if prec == RRT_F64 else "f32"


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------
def test_brute_force_on_the_dyadic_patch(workdir):
    sc = SR.scene(workdir, "patch")
    assert int(sc.desc.n_prim_order) == 2 * SR.PATCH_N ** 2
    uvs = SR.tables(sc, "patch")[2]
    at = SR.atlas_brute(sc, "patch", 16, 16)
    assert at["covered"] == 256 and (at["prim"] >= 0).all()
    k = at["prim"]
    a, b, c3 = uvs[k, 0], uvs[k, 1], uvs[k, 2]
    centre = a + (b - a) * at["b1"][..., None] + (c3 - a) * at["b2"][..., None]
    cx, cy = np.meshgrid((np.arange(16) + 0.5) / 16, (np.arange(16) + 0.5) / 16)
    assert np.abs(centre - np.stack([cx, cy], -1)).max() <= 1e-15
    # a quad holds 2 x 2 texels: the centres of the two with x % 2 == y % 2 lie exactly on its diagonal, both triangles of the quad cover them, and the
    # lower index owns them; the other two lie a quarter inside one triangle
    ys, xs = np.mgrid[0:16, 0:16]
    diag = xs % 2 == ys % 2
    assert (at["edge"][diag] == 0).all() and (at["edge"][~diag] == 0.25).all()
    rev = SR.atlas_brute(sc, "patch", 16, 16, prims=SR.triangle_entries(sc, "patch")[::-1])
    assert (at["prim"][diag] < rev["prim"][diag]).all() and np.array_equal(at["prim"][~diag], rev["prim"][~diag])
    # nothing is dyadic at 24 x 16, and no centre comes near an edge
    at = SR.atlas_brute(sc, "patch", 24, 16)
    assert at["covered"] == 24 * 16 and at["edge"].min() > 1e-12


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
def _compare(got, ref, prec, dtype, what, stable=None):
    stable = np.ones(ref["prim"].shape, bool) if stable is None else stable
    assert np.array_equal(got["prim"][stable], ref["prim"][stable]), what
    dev = max(float(np.abs(got[k][stable].astype(np.float64) - ref[k][stable].astype(dtype).astype(np.float64)).max()) for k in ("b1", "b2"))
    print(f"BAR atlas beta {_name(prec)} {what} {dev:.3e}")
    return dev


@pytest.mark.gpu
@PRECS
def test_atlas_against_brute_force(prec, workdir):
    sc = SR.scene(workdir, "patch")
    r = Renderer(sc, 0, prec)
    # 16 x 16: exact
    ref = SR.atlas_brute(sc, "patch", 16, 16)
    got = r.atlas_sites((16, 16))
    assert got["prim"].shape == (16, 16) and got["prim"].dtype == np.int32 and got["b1"].dtype == r.dtype
    assert _compare(got, ref, prec, r.dtype, "16x16") == 0.0
    assert got["covered"] == ref["covered"] == 256
    # 24 x 16: nothing dyadic
    ref = SR.atlas_brute(sc, "patch", 24, 16)
    stable = ref["edge"] > 1e-12
    assert stable.all()
    got = r.atlas_sites((24, 16))
    assert _compare(got, ref, prec, r.dtype, "24x16", stable) <= BETA_BAR[prec]
    assert got["covered"] == ref["covered"] == int((got["prim"] >= 0).sum())
    # every second triangle: the others' texels stay -1
    lst = SR.triangle_entries(sc, "patch")[::2]
    ref = SR.atlas_brute(sc, "patch", 24, 16, prims=lst)
    got = r.atlas_sites((24, 16), prims=lst)
    assert 0 < ref["covered"] < 24 * 16 and got["covered"] == ref["covered"]
    assert _compare(got, ref, prec, r.dtype, "24x16 every second") <= BETA_BAR[prec]
    assert not got["b1"][got["prim"] < 0].any() and not got["b2"][got["prim"] < 0].any()
    r.close()
    # the cube of the cfg3 case: 12 entries without vt, all on the half square u >= v
    sc = SR.scene(workdir, "rigid")
    mat_of, is_tri, uvs = SR.tables(sc, "rigid")
    cube = np.flatnonzero((uvs == np.array([[0, 0], [1, 0], [1, 1]])).all((1, 2)) & is_tri).astype(np.int32)[:12]
    assert len(cube) == 12
    r = Renderer(sc, 0, prec)
    for lst in (cube, cube[::-1].copy()):
        got = r.atlas_sites((13, 11), prims=lst)
        ref = SR.atlas_brute(sc, "rigid", 13, 11, prims=lst)
        assert np.array_equal(got["prim"], ref["prim"]) and got["covered"] == ref["covered"]
        assert set(np.unique(got["prim"])) == {-1, int(lst[0])}
    r.close()


def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.gpu
@PRECS
def test_the_chain_composes(prec, workdir):
    import torch
    sc = SR.scene(workdir, "patch_lit")
    r = Renderer(sc, 0, prec)
    aw, ah, n = 16, 16, 256
    mat_of, is_tri, uvs = SR.tables(sc, "patch_lit")
    charted = np.flatnonzero(is_tri & ~(uvs == np.array([[0, 0], [1, 0], [1, 1]])).all((1, 2))).astype(np.int32)     # the patch, not the roof
    assert len(charted) == 2 * SR.PATCH_N ** 2
    lst = charted[::2]                                               # half the texels stay uncovered
    # through host arrays
    sites = r.atlas_sites((aw, ah), prims=lst)
    rec = r.surface_at(sites["prim"].ravel(), sites["b1"].ravel(), sites["b2"].ravel(), fields=("p", "n"))
    flip = bool(rec["n"][sites["prim"].ravel() >= 0][0, 1] < 0)
    nrm = -rec["n"] if flip else rec["n"]
    sums = r.irradiance(rec["p"], nrm, 1, 5, offset=1.0 / 1024.0)
    dead = sites["prim"].ravel() < 0
    assert dead.sum() == n - sites["covered"] and 0 < dead.sum() < n
    assert not rec["p"][dead].any() and not rec["n"][dead].any() and not sums[dead].any()
    assert (sums[~dead, :3] > 0).all()
    # every intermediate in device memory
    tdt = torch.float32 if prec == RRT_F32 else torch.float64
    t_prim = torch.full((n,), 35, dtype=torch.int32, device="cuda:0")
    t_b1, t_b2 = (torch.full((n,), 3.5, dtype=tdt, device="cuda:0") for _ in range(2))
    t_rec = {k: torch.full((n,), 3.5, dtype=tdt, device="cuda:0") for k in ("px", "py", "pz", "nx", "ny", "nz")}
    t_sums = torch.zeros((n, 4), dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    covered = r.atlas_sites_device((aw, ah), t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr(), prims=lst)
    r.surface_at_device(t_prim.data_ptr(), t_b1.data_ptr(), t_b2.data_ptr(), n, {k: t.data_ptr() for k, t in t_rec.items()})
    if flip:
        torch.cuda.synchronize()
        for k in ("nx", "ny", "nz"): t_rec[k].neg_()
        torch.cuda.synchronize()
    r.irradiance_device([t_rec[k].data_ptr() for k in ("px", "py", "pz")], [t_rec[k].data_ptr() for k in ("nx", "ny", "nz")], n, 1, 5, t_sums.data_ptr(), offset=1.0 / 1024.0)
    torch.cuda.synchronize()
    assert covered == sites["covered"]
    assert np.array_equal(t_prim.cpu().numpy(), sites["prim"].ravel())
    assert np.array_equal(t_b1.cpu().numpy(), sites["b1"].ravel()) and np.array_equal(t_b2.cpu().numpy(), sites["b2"].ravel())
    for c, k in enumerate(("px", "py", "pz")):
        assert np.array_equal(t_rec[k].cpu().numpy(), rec["p"][:, c]), k
    assert np.array_equal(t_sums.cpu().numpy().view(np.uint8), sums.view(np.uint8))
    # bake_irradiance: those numbers, resolved
    bake = r.bake_irradiance((aw, ah), prims=lst, s0=1, s1=5, offset=1.0 / 1024.0, flip=flip)
    want = resolve_irradiance(sums, 4)
    assert bake["E"].shape == (ah, aw, 3) and np.array_equal(bake["E"], want["E"].reshape(ah, aw, 3)) and np.array_equal(bake["stderr"], want["stderr"].reshape(ah, aw))
    assert np.array_equal(bake["covered"], sites["prim"] >= 0)
    r.close()


@pytest.mark.gpu
@PRECS
def test_atlas_refusals(prec, workdir):
    import torch
    lib = A.lib()
    sc, sph = SR.scene(workdir, "patch"), SR.scene(workdir, "cfg1")
    r, rs = Renderer(sc, 0, prec), Renderer(sph, 0, prec)
    n_order = int(sc.desc.n_prim_order)
    prim = np.full(16, 35, np.int32); b1 = np.full(16, 3.5, r.dtype); b2 = np.full(16, 3.5, r.dtype)

    def call(h, aw, ah, lst=None, n_list=None, mem=A.RRT_MEM_HOST):
        lst = None if lst is None else np.ascontiguousarray(lst, np.int32)
        return lib.rrt_atlas_sites(h, aw, ah, None if lst is None else lst.ctypes.data, (0 if lst is None else len(lst)) if n_list is None else n_list, mem,
                                   prim.ctypes.data, b1.ctypes.data, b2.ctypes.data, None)

    for rc, substr in ((lambda: call(r._h, 0, 4), b"outside 1 .. 16384"), (lambda: call(r._h, 4, 16385), b"outside 1 .. 16384"), (lambda: call(r._h, 4, 4, mem=7), b"bad mem"),
                       (lambda: call(r._h, 4, 4, lst=[0], n_list=0), b"empty candidate list"), (lambda: call(r._h, 4, 4, lst=[0, n_order]), b"outside [0, n_prim_order) (entry 1)"),
                       (lambda: call(r._h, 4, 4, lst=[-1]), b"outside [0, n_prim_order)"), (lambda: call(rs._h, 4, 4, lst=[0]), b"names a sphere")):
        assert rc() == A.RRT_EINVAL and substr in lib.rrt_last_error(), lib.rrt_last_error()
    # a scene of spheres has no candidate: nothing is covered
    got = rs.atlas_sites((4, 4))
    assert got["covered"] == 0 and (got["prim"] == -1).all()
    W, H = sc.resolution
    film = torch.zeros((H, W, 4), dtype=torch.float32 if prec == RRT_F32 else torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    r.render_bands_begin(0, 1, film.data_ptr())
    assert call(r._h, 4, 4) == A.RRT_EINVAL and b"a frame is in flight" in lib.rrt_last_error()
    r.render_end()
    assert (prim == 35).all() and (b1 == 3.5).all() and (b2 == 3.5).all()
    assert call(r._h, 4, 4) == A.RRT_OK and (prim >= 0).all()
    with pytest.raises(RrtError):
        r.atlas_sites((4, 4), prims=[n_order])
    r.close(); rs.close()
