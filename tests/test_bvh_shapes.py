"""Traversal on hand-built BVH shapes (tests/bvh_shapes.py): deep, lopsided and fat-leaf trees over the cfg4 heightfield.

Every traversal kernel walks whatever tree the scene description carries, and the builder's trees reach only part of that code. The shapes here reach,
on purpose: the strided global stack of trees deeper than 64 (deep_, GlobStack, its reallocation when the pools grow), the spill of the fp32 kernels'
8-entry LDS stacks, the leaf-size limits of build_quads (511) and build_pairs (2047), and a root that is itself a leaf. Each shape is compared with the
oracle ON THE SAME DESCRIPTION, never with another tree: the reference's winner depends on the visiting order (Q10, last accepted wins).

CPU tests (no gpu mark): every shape passes validate_desc and has the depth it was built for; its closest-hit hit/miss set is the builder's tree's; the
ray batches reach what they are for BY THE ORACLE ALONE (shares of rays whose stack held more than 8 / more than 64 entries); at most 10 % of a
batch's rays are unstable. The oracle pushes the other child unconditionally; the fp32 pair-node kernels test both children's boxes at the parent and
push a far child only when its slabs are hit, so the oracle's occupancy is an upper bound of theirs. The probe therefore reports a second peak, over the
entries whose box the ray hits, and the batches are held to minimum shares under both (test_batches_spill_by_the_oracle).

Stable rays: rays from outside the scene whose oracle box margin and triangle margin are both >= 1e-3 - no comparison of the whole walk was closer
than that to flipping. On those the fp32 kernels must return the oracle's winner and occlusion bit on EVERY ray, in every traversal form. The shares
the filter leaves out (a condition of the test, at most 10 %) are what a leaf of hundreds of triangles costs: every ray that enters it makes hundreds
of triangle tests, each with its own edge lines to come near. Batches for the fat shapes therefore hold more near-vertical rays, for which the
regular grid's edge lines coincide row after row.

The u / v bar of the fp32 kernels is derived, not measured: the inputs are rounded to 2^-24 relative to M, the largest root-box coordinate;
Moeller-Trumbore is a few dozen operations on differences of the size of l, the shortest triangle edge; bound = 64 * 2^-24 * M / l, absolute
(1.37e-4 for the 512-triangle heightfield, 4.12e-4 for the 4608-triangle one).

Measured on an MI355X, every form of the fp32 traversal on every shape: no wrong winner and no wrong occlusion bit on any ray, stable or not; largest
u / v error on stable rays 8.9e-5 (comb_9) of 1.37e-4 on the 512-triangle shapes, 1.28e-4 of 4.12e-4 on the fat ones. test_f32_stable_rays prints
the figures per shape and form.
"""
import ctypes as C

import numpy as np
import pytest

import bvh_shapes as B
import oracle_lib as O
from rs_ray_toy_amd import RRT_F32, RRT_F64, RRT_FIXED_BVH, Renderer, RrtUnsupported, Scene, scenes
from rs_ray_toy_amd import _abi as A
from test_frame_shapes import INVARIANT_OPTIONS

gpu = pytest.mark.gpu

N_RAYS = 4096
STABLE = 1e-3
SIDES = ("first", "second", "alt")
DEPTHS_F64 = (8, 9, 10, 63, 64, 65, 200)
DEPTHS_F32 = (8, 9, 10, 64, 96)
FAT = (511, 512, 2047, 2048)
DEPTH_SHAPES = sorted({f"chain_{s}_{d}" for s in SIDES for d in DEPTHS_F64 + DEPTHS_F32} | {f"comb_{d}" for d in DEPTHS_F64 + DEPTHS_F32},
                      key=lambda n: (int(n.rsplit("_", 1)[1]), n))
FLAT_SHAPES = ["one_leaf"] + [f"fat_{b}" for b in FAT]
ALL_SHAPES = DEPTH_SHAPES + FLAT_SHAPES
F64_SHAPES = [n for n in DEPTH_SHAPES if int(n.rsplit("_", 1)[1]) in DEPTHS_F64] + FLAT_SHAPES
F32_SHAPES = [n for n in DEPTH_SHAPES if int(n.rsplit("_", 1)[1]) in DEPTHS_F32] + FLAT_SHAPES

_scenes, _shapes, _rays, _refs = {}, {}, {}, {}


def _depth_of(name):
    return int(name.rsplit("_", 1)[1]) if name.startswith(("chain", "comb")) else None


def _base(workdir, n, film=(32, 32), nsamp=5, max_depth=3, integrator="Path", flags=0):
    """The cfg4 heightfield with n x n x 2 plain triangles: not tie-prone (test_frame_shapes.py), reference-order and flattened evaluation coincide."""
    key = (n, film, nsamp, max_depth, integrator, flags)
    if key not in _scenes:
        cfg, root = scenes.cfg4(workdir, xres=film[0], yres=film[1], nsamp=nsamp, max_depth=max_depth, n=n)
        if integrator != "Path":
            cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": max_depth}
        _scenes[key] = Scene.loads(cfg, root, flags=flags)      # flags = 0: the builder's own tree is the reference-exact one
    return _scenes[key]


def _make(name, scene):
    if name == "builder": return scene
    if name == "one_leaf": return B.one_leaf(scene)
    if name.startswith("fat_"): return B.fat(scene, int(name[4:]))
    if name.startswith("comb_"): return B.comb(scene, _depth_of(name))
    _, side, depth = name.split("_")
    return B.chain(scene, int(depth), side)


def _shape(name, workdir, **scene_args):
    """The named shape over the 512-triangle heightfield (fat_*: the 4608-triangle one); "builder" / "builder48" = the loaded scenes themselves."""
    key = (name, tuple(sorted(scene_args.items())))
    if key not in _shapes:
        n = 48 if name.startswith("fat_") or name == "builder48" else 16
        # builder48: the fixed builder. At 4608 triangles the reference-exact one (flags = 0) drops primitives inside its treelets (Q26), so its tree does
        # not hold the whole scene; at 512 triangles it does, and "builder" is the reference-exact tree
        if name == "builder48": scene_args = dict(scene_args, flags=RRT_FIXED_BVH)
        _shapes[key] = _make("builder" if name.startswith("builder") else name, _base(workdir, n, **scene_args))
    return _shapes[key]


def _outside_rays(shape, scene, n, seed):
    """Rays from outside the scene.
    Depth shapes: half random_rays; a quarter aimed from a scene diagonal away at the box of the deepest interior node, all three direction signs equal -
    positive on even rays, negative on odd ones (a chain's stack grows only under one sign of each split axis, and only for rays that reach its far
    end); a quarter along the axis the chain's primitives are sorted by, both ways, through the middle of the field's height range: those pass
    through the boxes of many of the chain's leaves, which is what fills the stack of a walk that pushes a child only when its box is hit.
    Fat shapes (no depth to reach, hundreds of triangle tests per ray): a quarter random_rays, a quarter within ~1e-2 and half within ~1e-3 of the
    vertical, from above and from below (see the module docstring). The builder's own trees: random_rays alone."""
    wb = np.array(list(scene.desc.world_bound))
    diag = np.linalg.norm(wb[3:] - wb[:3])
    rng = np.random.default_rng(seed + 7)
    if not isinstance(shape, B.ShapedScene):
        return O.random_rays(scene, n, seed)
    if shape.axis is not None:
        m, m2 = n // 2, n // 4
        o, d, _ = O.random_rays(scene, n - m, seed)
        box = shape.last_interior_box
        tgt = box[:3] + rng.random((m, 3)) * (box[3:] - box[:3])
        dd = np.abs(rng.normal(size=(m, 3))) + 0.05
        lo, hi = wb[:3].copy(), wb[3:].copy()
        lo[1], hi[1] = wb[1] + 0.4 * (wb[4] - wb[1]), wb[1] + 0.6 * (wb[4] - wb[1])
        tgt[m - m2:] = lo + rng.random((m2, 3)) * (hi - lo)
        dd[m - m2:] = rng.normal(size=(m2, 3)) * 0.02
        dd[m - m2:, shape.axis] = 1.0
    else:
        m = n - n // 4
        o, d, _ = O.random_rays(scene, n - m, seed)
        tgt = wb[:3] + rng.random((m, 3)) * (wb[3:] - wb[:3])
        dd = rng.normal(size=(m, 3)) * np.where(np.arange(m) % 3 == 0, 1e-2, 1e-3)[:, None]
        dd[:, 1] = 1.0
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    dd *= np.where(np.arange(m) % 2 == 0, 1.0, -1.0)[:, None]
    # interleave the kinds, so that every prefix and every strided subset of the batch holds all of them
    o_all, d_all = np.concatenate([o, tgt - dd * diag]), np.concatenate([d, dd])
    perm = np.random.default_rng(seed + 13).permutation(n)
    return np.ascontiguousarray(o_all[perm]), np.ascontiguousarray(d_all[perm]), np.full(n, np.inf)


def _batch(name, workdir):
    """dict(o, d, tmax, skip, tmax_any): N_RAYS rays from outside followed by N_RAYS spawned on the surfaces the first half hit, in random directions, as
    test_gpu_parity._rays_for makes them (Q8: no origin offset; skip = the triangle a spawned ray starts on, which the fp32 kernels exclude).
    tmax_any: what any-hit queries use - unbounded for the rays from outside, 1 - 1e-4 for the spawned ones (shadow rays, Q9)."""
    if name not in _rays:
        sh = _shape(name, workdir)
        scene = sh.base if isinstance(sh, B.ShapedScene) else sh
        o, d, tmax = _outside_rays(sh, scene, N_RAYS, 3)
        ref = O.trace_closest(sh, o, d, tmax, want_geometry=True)
        hit = ref["prim"] >= 0
        rng = np.random.default_rng(4)
        d2 = rng.normal(size=(N_RAYS, 3))
        d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
        _rays[name] = dict(o=np.concatenate([o, np.where(hit[:, None], ref["p"], o)]), d=np.concatenate([d, d2]), tmax=np.concatenate([tmax, tmax]),
                           skip=np.concatenate([np.full(N_RAYS, -1, np.int32), np.where(hit, ref["prim"], -1).astype(np.int32)]),
                           tmax_any=np.concatenate([tmax, np.full(N_RAYS, 1.0 - 1e-4)]))
    return _rays[name]


def _ref(name, workdir):
    """The oracle on the shape's own description, computed once and shared: closest-hit and any-hit probes over the whole batch."""
    if name not in _refs:
        sh, b = _shape(name, workdir), _batch(name, workdir)
        _refs[name] = (O.trace_closest_probe(sh, b["o"], b["d"], b["tmax"]), O.trace_any_probe(sh, b["o"], b["d"], b["tmax_any"]))
    return _refs[name]


def _stable(ref):
    return (ref["margin"] >= STABLE) & (ref["tri_margin"] >= STABLE)


# ---- CPU: the shapes are what they claim, and the batches reach what they are for -----------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SHAPES)
def test_shape_is_valid_and_has_its_depth(name, workdir):
    """validate_desc accepts the description: rrt_create gets as far as the device (RRT_EDEVICE without one, a handle with one), never RRT_EINVAL."""
    sh = _shape(name, workdir)
    d = sh.desc
    if _depth_of(name) is not None: assert d.bvh_depth == sh.depth == _depth_of(name)
    elif name == "one_leaf": assert d.bvh_depth == 1 and d.n_bvh_nodes == 1 and d.bvh_nodes[0].n_primitives == d.n_prims == 512
    else: assert max(sh.leaf_sizes) == int(name[4:]) and d.n_prims == 4608 and sorted(sh.leaf_sizes)[-2] <= 320
    assert sum(sh.leaf_sizes) == d.n_prims == d.n_prim_order and d.n_bvh_nodes == 2 * len(sh.leaf_sizes) - 1
    lib = A.lib()
    h = C.c_void_p()
    rc = lib.rrt_create(0, C.byref(d), RRT_F64, C.byref(h))
    assert rc == (A.RRT_OK if lib.rrt_device_count() > 0 else A.RRT_EDEVICE), (rc, lib.rrt_last_error())
    if rc == A.RRT_OK: lib.rrt_destroy(h)
    less = A.SceneDesc.from_buffer_copy(d)      # and the depth is exact: one less is refused (on a copy: the shape is shared by the tests that follow)
    less.bvh_depth -= 1
    rc = lib.rrt_create(0, C.byref(less), RRT_F64, C.byref(h))
    assert rc == A.RRT_EINVAL and b"understates" in lib.rrt_last_error()


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_hit_miss_set_is_the_builders(name, workdir):
    """Which rays hit anything does not depend on the tree (the winner does: Q10). Rays from outside; the triangles' own boxes are padded, so no hit is lost to a box."""
    b, (ref, _) = _batch(name, workdir), _ref(name, workdir)
    builder = _shape("builder48" if name.startswith("fat_") else "builder", workdir)
    base = O.trace_closest(builder, b["o"], b["d"], b["tmax"])
    hit = ref["prim"] >= 0
    assert 0.3 < hit[:N_RAYS].mean() and hit[N_RAYS:].sum() > 50
    assert np.array_equal(hit, base["prim"] >= 0)


def _spill_minimum(name):
    """(least share of the batch whose ORACLE stack held more than 8 entries, more than 64), by the shape's construction: a chain of depth D with its leaves
    on one side holds D - 1 entries for a ray that reaches its end under the growing signs - half of the aimed rays, an eighth of the batch; an
    alternating chain grows on exactly three of every six levels for every ray that reaches the end, (D - 1) / 2 entries; a comb is an alternating chain
    above a balanced subtree of depth <= 10."""
    kind, D = name.split("_")[0], _depth_of(name)
    if name.startswith(("chain_first", "chain_second")): peak, share = D - 1, 0.12
    elif kind == "chain": peak, share = (D - 1) // 2, 0.4
    else: peak, share = (D - 10) // 2, 0.4
    return (share if peak > 8 else 0.0), (share if peak > 64 else 0.0)


def _spill_minimum_hit(name):
    """Least share of the batch whose stack held more than 8 entries under the fp32 pair-node kernels' push policy (peak_hit: a child is pushed only when
    the ray's slabs hit its box - the oracle pushes the other child unconditionally, so its occupancy is only an upper bound of theirs). What fills such
    a stack is a ray through the boxes of many leaves: the quarter of the batch that runs along the chain's sort axis, half of it the growing way.
    Chains of 63 levels and more: a tenth of the batch; chains with their leaves on one side at depth 10 (nine leaves to cross, all of them): 2 %; combs of
    63 levels and more (an alternating chain: every other level can grow): 1 %. Nothing is claimed for the alternating chain and the comb at depth 10
    and below: under this policy they never hold nine entries."""
    kind, D = name.split("_")[0], _depth_of(name)
    if kind == "chain" and D >= 63: return 0.1
    if name.startswith(("chain_first", "chain_second")) and D >= 10: return 0.02
    if kind == "comb" and D >= 63: return 0.01
    return 0.0


@pytest.mark.parametrize("name", DEPTH_SHAPES)
def test_batches_spill_by_the_oracle(name, workdir):
    """The oracle's own stack (the f64 kernels walk exactly like it: their node counters are compared bit for bit) and the occupancy under the fp32 pair-node
    kernels' push policy, both from the oracle's walk alone."""
    sh, (ref, ref_any) = _shape(name, workdir), _ref(name, workdir)
    D = sh.depth
    min8, min64 = _spill_minimum(name)
    min_hit = _spill_minimum_hit(name)
    for what, r in (("closest", ref), ("any", ref_any)):
        peak, peak_hit = r["peak"][:N_RAYS], r["peak_hit"][:N_RAYS]
        s8, s64, h8 = float((peak > 8).mean()), float((peak > 64).mean()), float((peak_hit > 8).mean())
        print(f"{name}: {what}-hit rays from outside: peak stack {peak.max()}, share beyond 8 entries {s8:.3f} (>= {min8}), beyond 64 {s64:.3f} (>= {min64}); "
              f"pushing only boxes that are hit: peak {peak_hit.max()}, share beyond 8 entries {h8:.3f} (>= {min_hit}), exactly 8: {(peak_hit == 8).mean():.3f}")
        assert peak_hit.max() <= peak.max() <= D - 1 and np.all(peak_hit <= peak)
        assert s8 >= min8 and s64 >= min64 and h8 >= min_hit
        if name.startswith(("chain_first", "chain_second")):
            assert (peak == D - 1).mean() >= 0.12      # depth 8, 9: the oracle's stack holds at most 8 entries; depth 10: a ninth
            if D == 9: assert (peak_hit == 8).mean() >= 0.02      # the 8 LDS entries exactly full, nothing spilled
    if D >= 64: assert ref["peak"][N_RAYS:].max() > 8      # the spawned rays spill too


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_stable_ray_cap(name, workdir):
    """At most 10 % of the rays from outside may be unstable, for closest-hit and for any-hit walks. A condition on the batch, not a measurement."""
    ref, ref_any = _ref(name, workdir)
    for what, r in (("closest", ref), ("any", ref_any)):
        unstable = 1.0 - _stable(r)[:N_RAYS].mean()
        print(f"{name}: {what}-hit: unstable share {unstable:.4f} (box margin alone {(r['margin'][:N_RAYS] < STABLE).mean():.4f})")
        assert unstable <= 0.10, (name, what, unstable)


def _tri_margin_numpy(shape, o, d, any_hit):
    """The definition of WalkProbe::tri_margin written out again: every triangle of a one-leaf tree is tested in prim_order; a test makes the comparisons
    up to its first failing one. Closest-hit: all triangles (Q10). Any-hit: E2 = p2 - p1 (Q11), and the walk stops at the first accepted triangle."""
    ds = shape.desc
    pos = np.ctypeslib.as_array(ds.positions, (ds.n_positions, 3))
    out = np.full(len(o), np.inf)
    for i in range(len(o)):
        for k in range(ds.n_prim_order):
            t = ds.tris[ds.prims[ds.prim_order[k]].shape]
            p0, p1, p2 = pos[t.v[0]], pos[t.v[1]], pos[t.v[2]]
            e1, e2 = p1 - p0, (p2 - p1 if any_hit else p2 - p0)
            pv = np.cross(d[i], e2)
            a = e1 @ pv
            out[i] = min(out[i], abs(abs(a) - 1e-7) / max(abs(a), 1e-7))
            if -1e-7 < a < 1e-7: continue
            f = 1.0 / a
            tv = o[i] - p0
            u = f * (tv @ pv)
            out[i] = min(out[i], abs(u), abs(u - 1.0))
            if u < 0.0 or u > 1.0: continue
            q = np.cross(tv, e1)
            v = f * (d[i] @ q)
            out[i] = min(out[i], abs(v), abs(u + v - 1.0))
            if v < 0.0 or u + v > 1.0: continue
            tt = f * (e2 @ q)
            out[i] = min(out[i], abs(tt - 1e-7) / max(abs(tt), 1e-7))
            if tt >= 1e-7 and any_hit: break
    return out


def test_triangle_margin_is_the_smallest_gap(workdir):
    """The probe against its definition written out in numpy, on the one-leaf tree (every ray tests every triangle, no box in the way), and at rays placed
    at known barycentrics of one triangle: its own gaps bound the walk's smallest from above."""
    sh = _shape("one_leaf", workdir)
    b = _batch("one_leaf", workdir)
    sel = np.arange(24) * 170
    o, d = b["o"][sel], b["d"][sel]
    r = O.trace_closest_probe(sh, o, d, b["tmax"][sel])
    a = O.trace_any_probe(sh, o, d, b["tmax"][sel])
    assert np.all(r["peak"] == 0) and np.all(r["prims"] == 512) and np.all(a["peak"] == 0) and np.all(r["margin"] > 0)
    np.testing.assert_allclose(r["tri_margin"], _tri_margin_numpy(sh, o, d, False), rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(a["tri_margin"], _tri_margin_numpy(sh, o, d, True), rtol=1e-6, atol=1e-12)
    ds = sh.desc
    t0 = ds.tris[ds.prims[ds.prim_order[0]].shape]
    p = np.array([[ds.positions[3 * t0.v[k] + c] for c in range(3)] for k in range(3)])
    nrm = np.cross(p[1] - p[0], p[2] - p[0])
    nrm /= np.linalg.norm(nrm)
    uv = np.array([[0.25, 0.25], [0.0005, 0.3], [0.3, 0.0002], [0.6, 0.3999]])
    tgt = p[0] + uv[:, :1] * (p[1] - p[0]) + uv[:, 1:] * (p[2] - p[0])
    r = O.trace_closest_probe(sh, tgt + nrm * 5.0, np.tile(-nrm, (len(uv), 1)), np.full(len(uv), np.inf))
    own = np.minimum.reduce([uv[:, 0], 1 - uv[:, 0], uv[:, 1], 1 - uv.sum(1)])
    assert np.all(r["tri_margin"] <= own + 1e-9) and np.all(r["tri_margin"][1:] < STABLE) and np.all(r["prim"] >= 0)


# ---- GPU, f64 handle: bit-exact ---------------------------------------------------------------------------------------------------------------------
def _assert_closest_exact(got, ref, sel=slice(None)):
    hit = ref["prim"][sel] >= 0
    assert np.array_equal(got["prim"], ref["prim"][sel])
    assert np.array_equal(got["nodes"], ref["nodes"][sel]) and np.array_equal(got["prims"], ref["prims"][sel])
    assert np.array_equal(got["t"], ref["t"][sel])
    assert np.array_equal(got["u"][hit], ref["u"][sel][hit]) and np.array_equal(got["v"][hit], ref["v"][sel][hit])


@gpu
@pytest.mark.parametrize("name", F64_SHAPES)
def test_f64_trace_matches_oracle_bit_for_bit(name, workdir):
    sh, b, (ref, ref_any) = _shape(name, workdir), _batch(name, workdir), _ref(name, workdir)
    r = Renderer(sh, 0, RRT_F64)
    try:
        _assert_closest_exact(r.trace_closest(b["o"], b["d"], b["tmax"], counters=True), ref)
        assert np.array_equal(r.trace_any(b["o"], b["d"], b["tmax_any"]), ref_any["occluded"])
        assert ref_any["occluded"][:N_RAYS].sum() > 500 and ref_any["occluded"][N_RAYS:].sum() > 20
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("name", ["chain_first_64", "chain_second_200", "comb_64", "comb_200"])
def test_f64_deep_stack_follows_the_pools_and_renders(name, workdir):
    """deep_stack_ is sized stack_depth x pool slots and strided by the slot count: 100 rays first, 5000 afterwards on the same handle (ensure_pools
    reallocates it), then a frame (the pools grow again: 32 x 32 x 4 slots... or stay, the stride is the pools' either way)."""
    sh, b, (ref, ref_any) = _shape(name, workdir), _batch(name, workdir), _ref(name, workdir)
    pick = np.arange(5000) * 8192 // 5000      # rays of both halves
    r = Renderer(sh, 0, RRT_F64)
    try:
        for sel in (pick[:100], pick, pick[:100]):
            _assert_closest_exact(r.trace_closest(b["o"][sel], b["d"][sel], b["tmax"][sel], counters=True), ref, sel)
            assert np.array_equal(r.trace_any(b["o"][sel], b["d"][sel], b["tmax_any"][sel]), ref_any["occluded"][sel])
        film, st = r.render(stats=True)
    finally:
        r.close()
    frame, st_ref = O.render(sh, stats=True)
    assert frame[..., :3].max() > 0
    assert np.array_equal(film[..., 3], frame[..., 3]) and st.camera_rays == st_ref.camera_rays
    assert st.any_queries == st_ref.any_queries
    diff = np.abs(film[..., :3] - frame[..., :3]).max(-1) / np.abs(frame[..., :3]).max()
    print(f"{name}: f64 frame vs oracle, max {diff.max():.3e}; closest-hit queries {st.closest_queries} (oracle {st_ref.closest_queries})")
    assert diff.max() < 1e-9, diff.max()       # test_render_f64_matches_oracle's bar


@gpu
def test_f64_direct_lighting_on_a_deep_tree(workdir):
    """DirectLighting on the depth-64 chain: the level loop's closest-hit and shadow launches with the strided global stack. (The per-sample recursion
    kernel k_direct_tree is taken for transmissive or textured scenes only, and check_renderable refuses those on a tree deeper than 64: second half.)"""
    sh = B.chain(_base(workdir, 16, integrator="DirectLighting"), 64, "first")
    frame, st_ref = O.render(sh, stats=True)
    r = Renderer(sh, 0, RRT_F64)
    try:
        film, st = r.render(stats=True)
    finally:
        r.close()
    assert frame[..., :3].max() > 0 and np.array_equal(film[..., 3], frame[..., 3])
    assert (st.camera_rays, st.closest_queries, st.any_queries) == (st_ref.camera_rays, st_ref.closest_queries, st_ref.any_queries)
    assert np.abs(film[..., :3] - frame[..., :3]).max() / np.abs(frame[..., :3]).max() < 1e-9
    from test_gpu_parity import TRANSMISSIVE, _with_material
    cfg, root = scenes.cfg4(workdir, xres=16, yres=16, nsamp=3, max_depth=3, n=16)
    cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3}
    _with_material(cfg, "mat_t", TRANSMISSIVE["glass"])
    cfg["Aggregate"]["primitives"][0]["material_name"] = "mat_t"
    glass = Scene.loads(cfg, root)
    for depth, refused in ((63, False), (64, True)):
        r = Renderer(B.chain(glass, depth, "first"), 0, RRT_F64)
        try:
            if refused:
                with pytest.raises(RrtUnsupported): r.render()
            else: r.render()
        finally:
            r.close()


# ---- GPU, fp32 handle: exact on the rays that can be exact ----------------------------------------------------------------------------------------
FORMS = (("generic", {"persistent_traversal": 0}, None),
         ("grid_stride", {"persistent_traversal": 1}, None),
         ("persistent", {"persistent_traversal": 2, "quad_nodes": 0}, None),
         ("persistent_quad", {"persistent_traversal": 2, "quad_nodes": 1}, None),
         ("split_below", {"persistent_traversal": 3, "quad_nodes": 0, "pt_split_closest": 1000, "pt_split_any": 1000}, 999),
         ("split_above", {"persistent_traversal": 3, "quad_nodes": 0, "pt_split_closest": 1000, "pt_split_any": 1000}, 1001))


def _uv_bound(shape):
    wb = np.abs(np.array(list(shape.desc.world_bound)))
    return 64.0 * 2.0 ** -24 * wb.max() / B.shortest_edge(shape)


@gpu
@pytest.mark.parametrize("name", F32_SHAPES)
def test_f32_stable_rays(name, workdir):
    """Every form of the fp32 traversal on the rays from outside: the oracle's winner and occlusion bit on every stable ray, t within the project's bar
    (test_trace_closest_f32), u and v within the derived bound."""
    sh, b, (ref, ref_any) = _shape(name, workdir), _batch(name, workdir), _ref(name, workdir)
    bound = _uv_bound(sh)
    worst = 0.0
    r = Renderer(sh, 0, RRT_F32)
    try:
        assert r.warnings == []      # nothing these shapes switch off is reported as a warning (build_pairs / build_quads drop their kernels silently)
        for form, options, count in FORMS:
            for k, v in options.items(): r.set_option(k, v)
            sel = np.arange(N_RAYS) if count is None else np.arange(count) * 4      # a strided subset: both kinds of rays, more than one workgroup
            o, d, tmax = b["o"][sel], b["d"][sel], b["tmax"][sel]
            got = r.trace_closest(o, d, tmax)
            occ = r.trace_any(o, d, tmax)
            st, st_any = _stable(ref)[sel], _stable(ref_any)[sel]
            hit = st & (ref["prim"][sel] >= 0)
            assert st.mean() >= 0.9 and hit.sum() > 300
            wrong, wrong_any = int((got["prim"] != ref["prim"][sel])[st].sum()), int((occ != ref_any["occluded"][sel])[st_any].sum())
            du = max(np.abs(got["u"][hit] - ref["u"][sel][hit]).max(), np.abs(got["v"][hit] - ref["v"][sel][hit]).max())
            worst = max(worst, float(du))
            print(f"{name} {form}: {st.sum()} stable of {len(sel)} rays: wrong winners {wrong}, wrong occlusion bits {wrong_any} (all rays: "
                  f"{int((got['prim'] != ref['prim'][sel]).sum())}, {int((occ != ref_any['occluded'][sel]).sum())}), largest u / v error {du:.3e} (bound {bound:.3e})")
            assert wrong == 0 and wrong_any == 0, (name, form, wrong, wrong_any)
            np.testing.assert_allclose(got["t"][hit], ref["t"][sel][hit], rtol=2e-4, atol=1e-4)
            assert du <= bound, (name, form, du, bound)
    finally:
        r.close()
    print(f"{name}: largest u / v error over all forms {worst:.3e}, bound {bound:.3e}")


@gpu
@pytest.mark.parametrize("name", F32_SHAPES)
def test_f32_quad_nodes_change_nothing(name, workdir):
    """On ALL rays, stable or not, spawned rays with their skip words included: quad_nodes 0 / 1 within the persistent kernel - winner, t, u, v."""
    sh, b = _shape(name, workdir), _batch(name, workdir)
    r = Renderer(sh, 0, RRT_F32)
    try:
        r.set_option("persistent_traversal", 2)
        res = {}
        for q in (0, 1):
            r.set_option("quad_nodes", q)
            res[q] = r.trace_closest(b["o"], b["d"], b["tmax"], skip_prim=b["skip"])
    finally:
        r.close()
    hit = res[0]["prim"] >= 0
    assert hit[:N_RAYS].sum() > 1000 and hit[N_RAYS:].sum() > 50
    assert np.array_equal(res[0]["prim"], res[1]["prim"]) and np.array_equal(res[0]["t"], res[1]["t"])
    assert np.array_equal(res[0]["u"][hit], res[1]["u"][hit]) and np.array_equal(res[0]["v"][hit], res[1]["v"][hit])


@gpu
@pytest.mark.parametrize("name", ["chain_first_96", "chain_second_96", "chain_alt_96", "comb_96", "chain_first_64", "comb_10"])
def test_f32_any_entry_changes_nothing(name, workdir):
    """any_entry 0 / 1 alone, as test_gpu_parity.py::test_any_hit_entry_nodes_change_nothing toggles it: frames (64 x 48, 9 spp, Path depth 4) identical bit
    for bit, query counts included, under the persistent and the grid-stride kernel. The any-hit start lists are taken by the pool's shadow rays only
    (lane_ray_begin: rrt_trace_any walks from the root whatever the option says), so a frame is the only way to them. Shadow candidate lists would
    serve these rays first: they are not built for trees deeper than 64 levels and are switched off for the others, and any_launches > list_launches says
    that the pair-node kernels had the shadow rays. On a chain every ancestor's off-path child is a leaf beside the start triangle's own: the lists are
    full (kAnyList = 6) and the ordinary walk takes over below the sixth entry, on a stack that already holds six."""
    sh = _shape(name, workdir, film=(64, 48), nsamp=10, max_depth=4)
    r = Renderer(sh, 0, RRT_F32)
    try:
        r.set_option("shadow_lists", 0)
        out = {}
        for mode in (2, 1):
            r.set_option("persistent_traversal", mode)
            for e in (1, 0):
                r.set_option("any_entry", e)
                out[mode, e] = r.render(stats=True)
    finally:
        r.close()
    for mode in (2, 1):
        (a, st_a), (b, st_b) = out[mode, 1], out[mode, 0]
        assert st_a.any_launches > st_a.list_launches == 0 and st_b.any_launches > st_b.list_launches == 0
        assert st_a.any_queries == st_b.any_queries > 1000 and (st_a.camera_rays, st_a.closest_queries) == (st_b.camera_rays, st_b.closest_queries)
        assert a[..., :3].max() > 0
        assert np.array_equal(a, b), (name, mode)


FRAME_SHAPES = ("comb_10", "comb_96", "one_leaf", "fat_2048")
_frame_refs = {}


def _frame_ref(name, nsamp, workdir):
    if (name, nsamp) not in _frame_refs:
        sh = _shape(name, workdir, film=(64, 48), nsamp=nsamp, max_depth=4)
        film, st = O.render(sh, stats=True)
        assert film[..., :3].max() > 0
        _frame_refs[name, nsamp] = (film, int(st.camera_rays))
    return _frame_refs[name, nsamp]


@gpu
@pytest.mark.parametrize("split0", [False, True], ids=["product_split", "split_0"])
@pytest.mark.parametrize("name,spp", [(n, 9) for n in FRAME_SHAPES] + [("comb_10", 8), ("comb_96", 8)])
def test_f32_frames(name, spp, split0, workdir):
    """64 x 48, Path depth 4, 9 samples per pixel: the default frame equals the frame with every result-invariant shortcut off together, bit for bit, and
    lies within test_default_fp32_frame_close_to_oracle's bars of the oracle's frame of the same description. split_0: the tile / persistent kernels at
    this queue size. 9 samples are no multiple of the camera workgroup's 8, so no pass of such a frame qualifies for the tile trees: the two combs, whose
    trees have more pair nodes than a tile-tree copy holds, are rendered at 8 samples per pixel as well (k_trace_tiles_f32 on a depth-96 tree; whether a
    camera ray of this frame fills its RRT_TT_STACK entries is not shown by anything here). A root leaf and a tree without pair nodes have no tile trees."""
    sh = _shape(name, workdir, film=(64, 48), nsamp=spp + 1, max_depth=4)
    ref, ref_rays = _frame_ref(name, spp + 1, workdir)
    r = Renderer(sh, 0, RRT_F32)
    try:
        if split0: r.set_option("pt_split_closest", 0); r.set_option("pt_split_any", 0)
        film, st = r.render(stats=True)
        for key in INVARIANT_OPTIONS: r.set_option(key, 0)
        plain, st_plain = r.render(stats=True)
    finally:
        r.close()
    print(f"{name} {spp} spp: tile launches {st.tile_launches}, list launches {st.list_launches} of {st.any_launches} any-hit launches, root culled {st.root_culled}, sky culled {st.sky_culled}")
    assert st_plain.tile_launches == 0 and st_plain.root_culled == 0 and st_plain.sky_culled == 0 and st_plain.list_launches == 0
    if name == "fat_2048":       # a leaf beyond kLeafCountMask: no pair-node kernels, hence none of the shortcuts that ride on them
        assert st.tile_launches == 0 and st.list_launches == 0 and st.root_culled == 0
    else:
        assert st.root_culled > 0
    if name == "comb_96": assert st.list_launches == 0                    # shadow candidate lists are built for trees of at most 64 levels
    if name == "comb_10": assert st.list_launches == st.any_launches > 0
    if name.startswith("comb") and spp == 8: assert st.tile_launches == 1     # more pair nodes than a tile-tree copy holds, one pass of 8 samples
    if spp == 9: assert st.tile_launches == 0
    assert (st.camera_rays, st.closest_queries, st.any_queries) == (st_plain.camera_rays, st_plain.closest_queries, st_plain.any_queries)
    assert np.array_equal(film, plain)       # all four channels
    assert np.array_equal(film[..., 3].astype(np.float64), ref[..., 3])
    assert abs(int(st.camera_rays) - ref_rays) <= 2e-5 * ref_rays, (st.camera_rays, ref_rays)       # test_default_fp32_frame_close_to_oracle's bar: equal at this size
    lit = ref[..., 3] != 0
    diff = (np.abs(film[..., :3].astype(np.float64) - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max())[lit]
    print(f"{name}: fp32 vs oracle at {spp} spp: within 1e-4: {(diff < 1e-4).mean():.4f}, max {diff.max():.3e}, mean {diff.mean():.3e}")
    assert np.all(film[~lit] == 0)
    if spp <= 8:
        assert diff.max() < 1e-4, diff.max()
    else:
        assert (diff < 1e-4).mean() >= 0.975, (diff < 1e-4).mean()
        assert diff.mean() < 1e-4, diff.mean()
        assert diff.max() < 3e-2 * 256 / spp, diff.max()


# ---- GPU, the public batch entry points: device memory, odd sizes ---------------------------------------------------------------------------------
PAD = 16
SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 513)


class _Raw:
    """rrt_trace_closest / rrt_trace_any on buffers this test owns, in host (numpy) or device (torch) memory, every output PAD elements longer than the batch
    and pre-filled with a canary."""

    def __init__(self, r, mem):
        self.r, self.mem = r, mem
        if mem == A.RRT_MEM_DEVICE:
            import torch
            self.torch = torch

    def _in(self, a):
        if self.mem == A.RRT_MEM_HOST: return np.ascontiguousarray(a)
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def _out(self, n, dtype, canary):
        a = np.full(n + PAD, canary, dtype)
        if self.mem == A.RRT_MEM_HOST: return a
        return self.torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to("cuda:0")

    @staticmethod
    def _ptr(a):
        return None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())

    def _np(self, a):
        return a if isinstance(a, np.ndarray) else a.cpu().numpy()

    def _rays(self, o, d, tmax, skip, mem=None):
        dt = self.r.dtype
        self.keep = [self._in(np.asarray(a, dt)) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
        self.keep.append(None if skip is None else self._in(np.asarray(skip, np.int32)))
        return A.Rays(self.mem if mem is None else mem, self.r.precision, *[self._ptr(a) for a in self.keep])

    def closest(self, o, d, tmax, n, skip=None, uv=True, counters=False, rays_mem=None):
        """-> (rc, dict of the n results, dict of the PAD-element tails)"""
        dt = self.r.dtype
        rays = self._rays(o, d, tmax, skip, rays_mem)
        outs = dict(t=self._out(n, dt, -7.5), prim=self._out(n, np.int32, -77))
        if uv: outs.update(u=self._out(n, dt, -7.5), v=self._out(n, dt, -7.5))
        if counters: outs.update(nodes=self._out(n, np.uint32, 0xdeadbeef), prims=self._out(n, np.uint32, 0xdeadbeef))
        hits = A.Hits(self.mem, self.r.precision, *[self._ptr(outs.get(k)) for k in ("t", "prim", "u", "v", "nodes", "prims")])
        rc = A.lib().rrt_trace_closest(self.r._h, C.byref(rays), n, C.byref(hits))
        if self.mem == A.RRT_MEM_DEVICE: self.torch.cuda.synchronize()
        res = {k: self._np(v) for k, v in outs.items()}
        for k in ("nodes", "prims"):
            if k in res: res[k] = res[k].view(np.uint32)
        return rc, {k: v[:n] for k, v in res.items()}, {k: v[n:] for k, v in res.items()}

    def any(self, o, d, tmax, n, skip=None):
        rays = self._rays(o, d, tmax, skip)
        occ = self._out(n, np.uint8, 0xa5)
        rc = A.lib().rrt_trace_any(self.r._h, C.byref(rays), n, self._ptr(occ))
        if self.mem == A.RRT_MEM_DEVICE: self.torch.cuda.synchronize()
        occ = self._np(occ)
        return rc, occ[:n], occ[n:]


def _tails_untouched(tails):
    for k, v in tails.items():
        canary = {"t": -7.5, "u": -7.5, "v": -7.5, "prim": -77, "nodes": 0xdeadbeef, "prims": 0xdeadbeef, "occ": 0xa5}[k]
        assert len(v) == PAD and np.all(v == canary), k


def _same(a, b, n=None):
    hit = a["prim"][:n] >= 0
    for k in a:
        x, y = a[k][:n], b[k][:n]
        if k in ("u", "v"): x, y = x[hit], y[hit]      # u and v of a miss are not defined
        assert np.array_equal(x, y), k


@gpu
@pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("tree", ["builder", "deep"])
def test_public_batch_forms(tree, prec, workdir):
    """rrt_trace_closest / rrt_trace_any on device-memory rays and hits against the host-memory call, bit for bit (k_pack_rays / k_unpack_hits straight on
    caller pointers): with and without u / v, with a device skip_prim, with device counters; batch sizes around the wave, the workgroup and two
    workgroups: every prefix of one batch equals the same rays inside the full batch, and nothing is written past the end of any output array."""
    name = "builder" if tree == "builder" else ("comb_200" if prec == RRT_F64 else "comb_96")
    sh, b = _shape(name, workdir), _batch(name, workdir)
    sel = np.arange(1024) * 8                      # rays from outside and spawned rays, with their skip words
    o, d, tmax, tmax_any, skip = b["o"][sel], b["d"][sel], b["tmax"][sel], b["tmax_any"][sel], b["skip"][sel].copy()
    win = _ref(name, workdir)[0]["prim"][sel]
    skip[::2] = np.where(skip[::2] < 0, win[::2], skip[::2])      # every other ray from outside skips the oracle's winner: a skip word that must change the answer
    n = len(sel)
    r = Renderer(sh, 0, prec)
    try:
        host, dev = _Raw(r, A.RRT_MEM_HOST), _Raw(r, A.RRT_MEM_DEVICE)
        full = {}
        for uv in (True, False):
            for with_skip in (False, True):
                for counters in (False, True):
                    sk = skip if with_skip else None
                    rc_h, res_h, tail_h = host.closest(o, d, tmax, n, sk, uv, counters)
                    rc_d, res_d, tail_d = dev.closest(o, d, tmax, n, sk, uv, counters)
                    assert rc_h == A.RRT_OK and rc_d == A.RRT_OK, A.lib().rrt_last_error()
                    assert (res_h["prim"] >= 0).sum() > 100
                    _same(res_h, res_d)
                    _tails_untouched(tail_h); _tails_untouched(tail_d)
                    full[uv, with_skip, counters] = res_d
        _same({k: v for k, v in full[True, True, False].items() if k in ("t", "prim")}, full[False, True, False])       # u / v asked for or not: the same hits
        if prec == RRT_F32:      # the skip words were read, in both memory kinds (the fp32 kernels exclude the named triangle)
            for counters in (False, True):
                got = full[True, True, counters]["prim"]
                assert (skip >= 0).sum() > 300 and np.all(got[skip >= 0] != skip[skip >= 0])
                assert not np.array_equal(got, full[True, False, counters]["prim"])
        full_any = {}
        for with_skip in (False, True):
            sk = skip if with_skip else None
            rc_h, occ_h, tail_h = host.any(o, d, tmax_any, n, sk)
            rc_d, occ_d, tail_d = dev.any(o, d, tmax_any, n, sk)
            assert rc_h == A.RRT_OK and rc_d == A.RRT_OK, A.lib().rrt_last_error()
            assert 20 < occ_h.sum() < n and np.array_equal(occ_h, occ_d)
            _tails_untouched({"occ": tail_h}); _tails_untouched({"occ": tail_d})
            full_any[with_skip] = occ_d
        for m in SIZES:
            for raw in (host, dev):
                rc, res, tail = raw.closest(o[:m], d[:m], tmax[:m], m, skip[:m], True, True)
                assert rc == A.RRT_OK
                _same(res, full[True, True, True], m)
                _tails_untouched(tail)
                rc, occ, tail = raw.any(o[:m], d[:m], tmax_any[:m], m, skip[:m])
                assert rc == A.RRT_OK and np.array_equal(occ, full_any[True][:m])
                _tails_untouched({"occ": tail})
        # n = 0: RRT_OK, nothing written
        for raw in (host, dev):
            rc, _, tail = raw.closest(o[:1], d[:1], tmax[:1], 0, skip[:1], True, True)
            assert rc == A.RRT_OK
            _tails_untouched(tail)
            rc, _, tail = raw.any(o[:1], d[:1], tmax_any[:1], 0)
            assert rc == A.RRT_OK
            _tails_untouched({"occ": tail})
        # rays and hits in different memory kinds: refused before anything is launched
        rc, _, tail = host.closest(o, d, tmax, n, rays_mem=A.RRT_MEM_DEVICE)
        assert rc == A.RRT_EINVAL and b"same memory kind" in A.lib().rrt_last_error()
        _tails_untouched(tail)
        rc, _, tail = dev.closest(o, d, tmax, n, rays_mem=A.RRT_MEM_HOST)
        assert rc == A.RRT_EINVAL
        _tails_untouched(tail)
        # the Python wrapper's device form, counters and skip included
        import torch
        t7 = [torch.from_numpy(np.ascontiguousarray(a, r.dtype)).to("cuda:0") for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
        tsk = torch.from_numpy(np.ascontiguousarray(skip)).to("cuda:0")
        tdt = torch.float32 if prec == RRT_F32 else torch.float64
        tt, tu, tv = (torch.zeros(n, dtype=tdt, device="cuda:0") for _ in range(3))
        tp = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        tn, tq = (torch.zeros(n, dtype=torch.int32, device="cuda:0") for _ in range(2))
        r.trace_closest_device([t.data_ptr() for t in t7], n, tt.data_ptr(), tp.data_ptr(), tu.data_ptr(), tv.data_ptr(), skip_ptr=tsk.data_ptr(),
                               nodes_ptr=tn.data_ptr(), prims_ptr=tq.data_ptr())
        torch.cuda.synchronize()
        want = full[True, True, True]
        _same(dict(t=tt.cpu().numpy(), prim=tp.cpu().numpy(), u=tu.cpu().numpy(), v=tv.cpu().numpy(), nodes=tn.cpu().numpy().view(np.uint32),
                   prims=tq.cpu().numpy().view(np.uint32)), want)
        assert want["nodes"].min() >= 1 and want["prims"].max() > 0
    finally:
        r.close()
