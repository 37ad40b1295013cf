"""The procedural half of the device's texture code (dtexture.hpp: TexEval's node types, tex_map_2d, map_round, the Perlin noise, noise_sum and the saturating
casts, compute_differentials, solve_2x2; dkernels.hpp: Material::bump and the triangle's uv set-up in SurfExt) and the host side that flattens the graph,
on hand-built graphs, mappings and footprints (tests/texture_shapes.py), against the f64 oracle.

test_gpu_parity.py::test_textured_materials' procedural cases sit where the closed-form checkerboard filter is mostly bypassed and never cross a seam, a
pole, a negative lattice coordinate, a saturated cast, a fallback constant, a mirrored or degenerate uv, or the depth limit. texture_shapes.py says which
case reaches what, and the oracle's texture census (oracle_lib.tex_census) proves per case that the frame does reach it: the proof is counted on the
reference side.

CPU tests (the host loader and the oracle alone):
  test_case_loads_and_reaches_its_branches    the oracle's frame is finite, the weight plane full, the frame lit, the census has what the case's tags ask;
                                              the slot cases bind the slots they name; a mirror case evaluates more checkerboards than its walls twin
  test_cases_are_distinct                     within each group that differs by one parameter the oracle's frames differ pairwise in more than 2 % of the
                                              lit pixels: a device that ignored the parameter cannot pass
  test_bump_differs_from_a_constant_displacement   every bump case's frame differs from the frames of three constant displacements: its finite
                                              difference is exercised
  test_the_later_texture_owns_a_duplicated_name   the child indices of the loaded graph
  test_depth_six_loads_and_the_oracle_walks_it   the loader and the oracle have no depth limit; the refusal is the device's (test_depth_six_is_refused)
  test_point_values                           oracle_lib.texture_eval against a numpy restatement: bump_int at negative arguments, the folds on both
                                              sides of the seam, noise at saturated coordinates, octaves 0
GPU tests, a 64 x 64 film at nsamp 5 each:
  test_f64_frame_matches_oracle               weights and the three counters equal, colour within 1e-9 of the brightest pixel; RrtPanic where the oracle panics
  test_fp32_frame_close_to_oracle             test_textured_materials' fp32 bars (its path_bump_patch bar for the bump-mapped Path cases)
  test_albedo_plane                           rrt_render_aov's albedo for one case per group against tests/aov_reference.py, test_aov.py's bars
  test_followed_plane                         rrt_render_aov_follow on the mirror carrier against tests/aov_follow_reference.py
  test_shortcuts_change_no_bit                shade compaction, kernel specialisation and tile order off: the fp32 frame keeps its bits
  test_depth_six_is_refused                   RrtUnsupported from every render call in both precisions (the handle is made: the check is check_renderable's);
                                              the depth-5 chain renders on the same handle type
"""
import numpy as np
import pytest

import oracle_lib as O
import texture_shapes as TS
from rs_ray_toy_amd import RRT_F32, RRT_F64, Renderer, RrtPanic, RrtUnsupported, Scene

ALL = sorted(TS.CASES)
FRAMES = [k for k in ALL if TS.CASES[k].oracle == "frame"]
# the cube (plain matte) alone lights 68 of the 4 096 pixels (test_image_shapes.py)
CUBE_ONLY = 0.05

_scenes, _refs = {}, {}


def _scene(name, workdir):
    if name not in _scenes:
        _scenes[name] = Scene.loads(*TS.scene(workdir, name))
    return _scenes[name]


def _ref(name, workdir):
    """(frame, (camera rays, closest queries the device issues, any queries), census) of the oracle for the case, rendered once and never written to;
    (None, panic message, census) where the oracle panics"""
    if name not in _refs:
        sc = _scene(name, workdir)
        O.tex_census(); O.bsdf_census()
        try:
            film, st = O.render(sc, stats=True)
            film.setflags(write=False)
            # (the device leaves out the path integrator's closest-hit query at bounces == max_depth: test_material_shapes.py::_ref)
            _refs[name] = (film, (int(st.camera_rays), int(st.closest_queries) - O.bsdf_census()["path_last_query"], int(st.any_queries)), O.tex_census())
        except O.OracleError as e:
            _refs[name] = (None, str(e), O.tex_census())
    return _refs[name]


def _lit(film):
    return float((film[..., :3].max(-1) > 0).mean())


def _counters(st):
    return int(st.camera_rays), int(st.closest_queries), int(st.any_queries)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_the_table_has_its_size():
    assert 50 <= len(ALL) <= 90 and len(TS.F64_ONLY) <= 4
    assert {c.group for c in TS.CASES.values()} == {"checker", "round", "noise", "graph", "slots", "diff", "bump"}
    # every textured slot of resolve_material is claimed by some case (and test_case_loads_and_reaches_its_branches holds each case to its claim)
    claimed = {k for c in TS.CASES.values() for tag in c.tags if tag.startswith("slots:") for k in tag[6:].split(",")}
    assert claimed == set(TS.SLOTS) and len(TS.SLOTS) == 13, sorted(set(TS.SLOTS) - claimed)
    assert any("bump" in c.tags for c in TS.CASES.values())


@pytest.mark.parametrize("name", ALL)
def test_case_loads_and_reaches_its_branches(name, workdir):
    c = TS.CASES[name]
    sc = _scene(name, workdir)
    bound = {k for m in sc.desc.materials[:sc.desc.n_materials] for k in range(13) if m.tex[k] >= 0}
    for tag in c.tags:
        if tag.startswith("slots:"):
            assert {TS.SLOTS[k] for k in tag[6:].split(",")} <= bound, (tag, bound)
    if "bump" in c.tags: assert any(m.bump >= 0 for m in sc.desc.materials[:sc.desc.n_materials])
    film, counters, census = _ref(name, workdir)
    if c.oracle == "panic":
        assert film is None and "path.rs:147 assert!(beta.y().is_finite())" in counters, counters
        return
    assert film is not None, counters
    print(f"{name}: lit {_lit(film):.4f}, brightest {film[..., :3].max():.4g}, counters {counters}, census { {k: v for k, v in census.items() if v} }")
    assert np.all(np.isfinite(film)) and np.all(film[..., 3] > 0)
    assert _lit(film) > CUBE_ONLY
    assert not TS.census_problems(c, census), (TS.census_problems(c, census), census)
    if c.carrier == "mirror":      # the enclosure is evaluated again behind the mirror, with the differentials the specular child inherits
        O.tex_census()
        O.render(Scene.loads(*TS.scene(workdir, c._replace(carrier="walls"))))
        twin = O.tex_census()
        assert census["node_checker2d"] > twin["node_checker2d"] and census["chk_filtered"] > twin["chk_filtered"], (census, twin)


DISTINCT = {
    "aamode-su0.5": ["chk-su0.5-closedform", "chk-su0.5-none"], "aamode-su2": ["chk-su2-closedform", "chk-su2-none"],
    "aamode-su6": ["chk-su6-closedform", "chk-su6-none"], "aamode-su40": ["chk-su40-closedform", "chk-su40-none"],
    "su-closedform": [f"chk-su{su}-closedform" for su in ("0.5", "2", "6", "40")], "su-none": [f"chk-su{su}-none" for su in ("0.5", "2", "6", "40")],
    "planar": ["chk-planar-generic", "chk-planar-parallel"],
    "octaves": [f"wrinkled-o{o}-w0.5" for o in (0, 1, 8, 12)], "omega": [f"wrinkled-o8-w{w}" for w in ("0", "0.5", "1", "1.5")],
    "windy-scale": ["windy-s0.05", "windy-s3", "windy-s200"], "chk3-scale": ["chk3-s0.1-negative", "chk3-s3-negative"],
    "rotation-spherical": [f"round-spherical-{r}-uv" for r in ("identity", "rotated", "squashed")],
    "rotation-cylindrical": [f"round-cylindrical-{r}-uv" for r in ("identity", "rotated", "squashed")],
    "mapping-kind": ["round-spherical-identity-uv", "round-cylindrical-identity-uv"],
    "missing-mix": ["fallback-mix-t1", "fallback-mix-t2"], "missing-scale": ["fallback-scale-t1", "fallback-scale-t2"],
    "missing-checker": ["fallback-checker-t1", "fallback-checker-t2"],
    "depth": [f"depth-{d}" for d in range(1, 6)],
    "uvmesh-texture": ["uvmesh-chk", "uvmesh-uv"],
    # (a Matte's frame does not read vn: set_shading_geometry keeps the geometric normal. Under a bump map displace * dndu does)
    "uvmesh-vn": ["bump-ramp-uvmesh", "bump-ramp-uvmesh-vn"],
    "bump-patch": ["bump-wrinkled", "bump-windy", "bump-chk3", "bump-checker-closedform", "bump-depth5"],
}


@pytest.mark.parametrize("group", sorted(DISTINCT))
def test_cases_are_distinct(group, workdir):
    names = DISTINCT[group]
    films = [_ref(n, workdir)[0][..., :3] for n in names]
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            lit = (films[a].max(-1) > 0) | (films[b].max(-1) > 0)
            scale = max(films[a].max(), films[b].max())
            differ = int((np.abs(films[a] - films[b]).max(-1) > 1e-6 * scale)[lit].sum())
            print(f"{group}: {names[a]} against {names[b]}: {differ} of {int(lit.sum())} lit pixels differ")
            assert differ > 0.02 * lit.sum(), (names[a], names[b], differ)


BUMPED = [k for k in ALL if any(t in ("bump", "bump_some") for t in TS.CASES[k].tags)]


@pytest.mark.parametrize("name", BUMPED)
def test_bump_differs_from_a_constant_displacement(name, workdir):
    """Material::bump is a finite difference: a displacement that does not vary over the hit tests none of it. Every bump case's oracle frame differs, in
    more than 2 % of the lit pixels, from the frames of the same scene under constant displacements (0, and the case's own largest value scale 0.03 / 0.5)."""
    c = TS.CASES[name]
    film = _ref(name, workdir)[0][..., :3]
    for const in (0.0, 0.03, 0.5):
        twin = c._replace(floats=[TS.cf0("bumpy", const)])
        flat = O.render(Scene.loads(*TS.scene(workdir, twin)))[..., :3]
        lit = (film.max(-1) > 0) | (flat.max(-1) > 0)
        differ = int((np.abs(film - flat).max(-1) > 1e-6 * max(film.max(), flat.max()))[lit].sum())
        print(f"{name}: against a constant {const}: {differ} of {int(lit.sum())} lit pixels differ")
        assert differ > 0.02 * lit.sum(), (const, differ)


def test_the_later_texture_owns_a_duplicated_name(workdir):
    """duplicate-names: `dup` is declared twice (a constant, then a UV texture) with the Scale `early` between them. The oracle and the device read the same
    loaded graph, so the owner is asserted on it: `early` holds the first `dup`, the root's t2 the second (renderprocess.rs inserts into a HashMap)."""
    BILERP, UV = 2, 8      # RRT_TEX_* of include/rrt.h
    sc = _scene("duplicate-names", workdir)
    t = sc.desc.textures
    names = [x["texture_name"] for x in TS.CASES["duplicate-names"].rgbs]      # node i is the i-th declared texture: none is skipped here
    assert sc.desc.n_textures == len(names) == 5
    first, early, second, root = names.index("dup"), names.index("early"), len(names) - 1 - names[::-1].index("dup"), names.index("root")
    assert (first, early, second, root) == (1, 2, 3, 4)
    assert t[first].type == BILERP and t[second].type == UV
    assert (t[early].child[0], t[early].child[1]) == (first, names.index("tint"))
    assert (t[root].child[0], t[root].child[1]) == (early, second)
    assert sc.desc.materials[sc.desc.n_materials - 1].tex[0] == root


def test_depth_six_loads_and_the_oracle_walks_it(workdir):
    """Neither the loader nor the reference has a depth limit: the six-level chain loads and the oracle evaluates six levels. The refusal is the device's
    (kTexDepth, raised by the render calls of a handle and not without a device: test_depth_six_is_refused)."""
    sc = Scene.loads(*TS.refused_scene(workdir))
    O.tex_census()
    film = O.render(sc)
    census = O.tex_census()
    assert census["depth_max"] == 6 and census["node_uv"] > 1000 and np.all(np.isfinite(film)) and _lit(film) > CUBE_ONLY


PERM = [151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240, 21, 10, 23, 190, 6, 148,
        247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88, 237, 149, 56, 87, 174, 20, 125, 136, 171, 168, 68, 175,
        74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231, 83, 111, 229, 122, 60, 211, 133, 230, 220, 105, 92, 41, 55, 46, 245, 40, 244, 102, 143, 54,
        65, 25, 63, 161, 1, 216, 80, 73, 209, 76, 132, 187, 208, 89, 18, 169, 200, 196, 135, 130, 116, 188, 159, 86, 164, 100, 109, 198, 173, 186, 3, 64,
        52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118, 126, 255, 82, 85, 212, 207, 206, 59, 227, 47, 16, 58, 17, 182, 189, 28, 42, 223, 183, 170, 213,
        119, 248, 152, 2, 44, 154, 163, 70, 221, 153, 101, 155, 167, 43, 172, 9, 129, 22, 39, 253, 19, 98, 108, 110, 79, 113, 224, 232, 178, 185, 112, 104,
        218, 246, 97, 228, 251, 34, 242, 193, 238, 210, 144, 12, 191, 179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31, 181, 199, 106, 157,
        184, 84, 204, 176, 115, 121, 50, 45, 127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243, 141, 128, 195, 78, 66, 215, 61, 156, 180] * 2


def _as_i32(v):
    """Rust's `as i32`: saturating"""
    return int(min(max(v, -2147483648.0), 2147483647.0))


def _perlin_sat(x, y, z):
    """texture/mod.rs:73-130 with its `as i32` casts (test_oracle.py::_perlin takes int(floor()), which does not saturate): past 2^31 the lattice
    coordinate stops at i32::MAX and dx = x - ix is as large as x"""
    def grad(ix, iy, iz, dx, dy, dz):
        h = PERM[PERM[PERM[ix] + iy] + iz] & 15
        u = dx if (h < 8 or h in (12, 13)) else dy
        v = dy if (h < 4 or h in (12, 13)) else dz
        return (-u if h & 1 else u) + (-v if h & 2 else v)

    ix, iy, iz = _as_i32(np.floor(x)), _as_i32(np.floor(y)), _as_i32(np.floor(z))
    dx, dy, dz = x - ix, y - iy, z - iz
    ix &= 255; iy &= 255; iz &= 255

    def w(t):
        t3 = t * t * t; t4 = t3 * t
        return 6.0 * t4 * t - 15.0 * t4 + 10.0 * t3
    lerp = lambda t, a, b: a * (1.0 - t) + b * t
    c = [[[grad(ix + i, iy + j, iz + k, dx - i, dy - j, dz - k) for k in (0, 1)] for j in (0, 1)] for i in (0, 1)]
    x00, x10 = lerp(w(dx), c[0][0][0], c[1][0][0]), lerp(w(dx), c[0][1][0], c[1][1][0])
    x01, x11 = lerp(w(dx), c[0][0][1], c[1][0][1]), lerp(w(dx), c[0][1][1], c[1][1][1])
    return lerp(w(dz), lerp(w(dy), x00, x10), lerp(w(dy), x01, x11))


def test_point_values(tmp_path):
    from test_oracle import _perlin, _texture_scene
    rot = {"rotation_axis": [0.0, 0.0, 1.0], "rotation_angle": 0.0}
    ft = [TS.wrinkled("wr0", 0, 0.5, **rot), TS.wrinkled("wr3", 3, 1.5, **rot), TS.wrinkled("wr_big", 2, 0.5, **rot, **TS.s3(1e9)), TS.windy("wind_big", **rot, **TS.s3(1e9))]
    rt = [TS.cr("a", [0.9, 0.1, 0.2]), TS.cr("b", [0.0, 0.5, 1.0]), TS.checker("chk", "a", "b", TS.uvmap(4.0, 4.0, -5.2, -5.2)),
          {"texture_type": "CheckerBoardTexture", "texture_name": "sph", "t1": "a", "t2": "b", "mapping": {"mapping": "spherical"}, **rot, "world_pos": [1.0, 2.0, 3.0]},
          {"texture_type": "CheckerBoardTexture", "texture_name": "cyl", "t1": "a", "t2": "b", "mapping": {"mapping": "cylindrical"}, **rot, "world_pos": [1.0, 2.0, 3.0]}]
    sc, ix = _texture_scene(tmp_path, ft, rt)
    ev = lambda name, **kw: O.texture_eval(sc, ix[name], **kw)
    A, B = np.array([0.9, 0.1, 0.2]), np.array([0.0, 0.5, 1.0])
    bump = lambda x: np.floor(x / 2) + 2 * max(x / 2 - np.floor(x / 2) - 0.5, 0.0)

    def filtered(s, t, ds, dt):
        """checkerboard.rs:54-97 past aamode none"""
        if np.floor(s - ds) == np.floor(s + ds) and np.floor(t - dt) == np.floor(t + dt):
            return A if (int(np.floor(s)) + int(np.floor(t))) % 2 == 0 else B      # (Python's % is not Rust's, but even is even)
        sint, tint = (bump(s + ds) - bump(s - ds)) / (2 * ds), (bump(t + dt) - bump(t - dt)) / (2 * dt)
        area2 = 0.5 if (ds > 1 or dt > 1) else sint + tint - 2 * sint * tint
        return A * (1 - area2) + B * area2

    # bump_int at negative arguments: floor(x / 2) is negative and the fractional part still lies in [0, 1)
    assert bump(-0.5) == -0.5 and bump(-1.5) == -1.0 and bump(-2.5) == -1.5      # (the integral of the square wave: flat on [-2, -1], rising on [-1, 0])
    O.tex_census()
    for u, v, duv in ((0.255, 0.1, (0.01, 0.002, 0.001, 0.004)), (0.9, 0.77, (0.03, 0.0, 0.0, 0.05)), (0.55, 1.0, (0.1, 0.0, 0.0, 0.2)), (1.29, 1.28, (0.02, 0.01, 0.01, 0.03))):
        s, t, ds, dt = 4 * u - 5.2, 4 * v - 5.2, 4 * max(abs(duv[0]), abs(duv[1])), 4 * max(abs(duv[2]), abs(duv[3]))
        assert s - ds < 0 and t - dt < 0
        np.testing.assert_allclose(ev("chk", uv=(u, v), duv=duv), filtered(s, t, ds, dt), rtol=1e-12, atol=1e-15)
    census = O.tex_census()
    assert census["chk_bump_int_negative"] == census["chk_filtered"] == 3 and census["chk_same_cell"] == 1 and census["chk_negative_sum"] == 4, census      # (the first: one cell)

    # the folds on both sides of the seam: a checkerboard over a round mapping returns the filtered value of (st, folded dst)
    centre = np.array([1.0, 2.0, 3.0])

    def sphere(p):
        q = (p - centre) / np.linalg.norm(p - centre)
        phi = np.arctan2(q[1], q[0])
        return np.array([np.arccos(np.clip(q[2], -1, 1)) / np.pi, (phi + 2 * np.pi if phi < 0 else phi) / (2 * np.pi)])

    def cylinder(p):
        q = (p - centre) / np.linalg.norm(p - centre)
        return np.array([(np.pi + np.arctan2(q[1], q[0])) / (2 * np.pi), q[2]])

    def round_value(f, p, dpdx, dpdy):
        st = f(p)
        dx, dy = (f(p + 0.1 * dpdx) - st) / 0.1, (f(p + 0.1 * dpdy) - st) / 0.1
        for d in (dx, dy):
            if d[1] > 0.5: d[1] = 1.0 - d[1]
            elif d[1] < -0.5: d[1] = -(d[1] + 1.0)
        return filtered(st[0], st[1], max(abs(dx[0]), abs(dx[1])), max(abs(dy[0]), abs(dy[1])))

    O.tex_census()
    for f, name in ((sphere, "sph"), (cylinder, "cyl")):
        # the spherical seam is the half plane y = 0, x > 0 in texture space (phi wraps there); for the cylinder the fold reads [1] = v.z, so the step runs
        # along z there. A step of 0.1 * 4 across either, from both sides, and a short one that crosses nothing
        along = np.array([0.0, 4.0, 0.5]) if f is sphere else np.array([0.3, 0.2, 9.0])
        for side in (1.0, -1.0):
            p = centre + np.array([2.0, 0.0, 0.3]) - side * 0.2 * along / np.linalg.norm(along)
            for dpdx, dpdy in ((side * along, np.array([0.01, 0.02, 0.0])), (np.array([0.02, 0.0, 0.01]), side * along), (np.array([0.01, 0.0, 0.0]), np.array([0.0, 0.0, 0.01]))):
                np.testing.assert_allclose(ev(name, p=p, dpdx=dpdx, dpdy=dpdy), round_value(f, p, dpdx, dpdy), rtol=1e-10, atol=1e-13)
    census = O.tex_census()
    for k in ("fold_dx_high", "fold_dx_low", "fold_dy_high", "fold_dy_low"): assert census[k] >= 1, census
    assert census["round_phi_wrapped"] > 0

    # octaves 0: n = 0 = octaves, no full term, the partial term lerp(smooth_step(0) = 0, 0.2, |noise|) = 0.2, no tail
    p = (0.37, 1.31, -0.4)
    np.testing.assert_allclose(ev("wr0", p=p), [0.2] * 3, rtol=1e-15)
    np.testing.assert_allclose(ev("wr0", p=p, dpdx=(0.5, 0, 0)), [0.2] * 3, rtol=1e-15)
    # omega above 1 with all three octaves (zero footprint): sum omega^i |noise(1.99^i p)| + omega^3 * 0.2
    want = sum(1.5 ** i * abs(_perlin(*(np.array(p) * 1.99 ** i))) for i in range(3)) + 1.5 ** 3 * 0.2
    np.testing.assert_allclose(ev("wr3", p=p)[0], want, rtol=1e-13)

    # saturated coordinates (scale 1e9): the restatement with saturating casts agrees, and an fp32 world_to_texture would not: the entry 1e9 itself is
    # representable, but a ROTATED placement's entries are not, and rounding one to fp32 (a relative 6e-8, up to 32 in 1e9) moves the argument by
    # hundreds of lattice cells at scene coordinates - where dx is not even the fractional part any more
    q = np.array([12.5, -3.25, 40.0])
    O.tex_census()
    got = ev("wr_big", p=q)[0]
    assert O.tex_census()["noise_saturated"] == 3
    want = sum(0.5 ** i * abs(_perlin_sat(*(q * 1e9 * 1.99 ** i))) for i in range(2)) + 0.5 ** 2 * 0.2
    assert np.isfinite(got) and got > 1e100
    np.testing.assert_allclose(got, want, rtol=1e-9)
    assert _perlin_sat(*(q * 1e9)) != _perlin(*(q * 1e9))
    got = ev("wind_big", p=q)[0]

    def fbm(pt, octaves):
        return sum(0.5 ** i * _perlin_sat(*(pt * 1.99 ** i)) for i in range(octaves))      # zero footprint: n = octaves, the partial term is smooth_step(0) = 0
    with np.errstate(over="ignore"):
        want = abs(fbm(q * 1e9 * 0.1, 3)) * fbm(q * 1e9, 6)
    assert (np.isinf(want) and np.isinf(got) and np.sign(want) == np.sign(got)) or np.isclose(got, want, rtol=1e-9)
    fp32_entry = float(np.float32(0.9063077870366499e9))      # cos(25 degrees) * 1e9: an entry of the rotated placement
    assert abs(fp32_entry - 0.9063077870366499e9) * 40.0 > 100.0


@pytest.mark.parametrize("name", ["axes-walls", "bump-du-fallback", "uvmesh-vn-chk"])
def test_degenerate_uv_faces_are_not_flattened(name, workdir):
    """The fp32 product moves the triangles of a rigid instance to world space. A degenerate-uv triangle takes dpdu / dpdv (and dndu / dndv) from
    coordinate_system() of an object-space vector, which does not commute with the instance's rotation: flattened, axes-walls differed from the reference in
    239 pixels by up to 1.1e-2 of the brightest, bump-du-fallback in 134. The host keeps such triangles as instances (scene_flatten.cpp uv_degenerate) and the
    oracle's flat mode restates that: its frame is the reference-order frame up to rounding."""
    ref = _ref(name, workdir)[0]
    flat = O.render(_scene(name, workdir), flat=True)
    assert np.array_equal(flat[..., 3], ref[..., 3])
    diff = np.abs(flat[..., :3] - ref[..., :3]).max() / ref[..., :3].max()
    print(f"{name}: flat against reference order {diff:.3e}")
    assert diff < 1e-9, diff


def test_f64_only_arguments(workdir):
    """What texture_shapes.py says of windy-s200, on the oracle alone: the texture's values at the camera's hit points on the walls, against the values
    at the same points ROUNDED to fp32. At scale 200 a large share moves by more than the bar's 1e-4 of the largest value, at scale 3 none does. (The
    scale-1e9 cases: test_point_values.)"""
    share = {}
    for name in ("windy-s200", "windy-s3"):
        sc = _scene(name, workdir)
        root = sc.desc.n_textures - 1
        _, rays, w = O.camera_samples(sc, (0, 0, TS.XRES, TS.YRES), 0, TS.NSAMP)
        o, d = rays[w != 0, :3], rays[w != 0, 3:]
        hit = O.trace_closest(sc, o, d, np.full(len(o), np.inf))
        found = hit["prim"] >= 0
        p = (o[found] + d[found] * hit["t"][found][:, None])[::10]
        exact = np.array([O.texture_eval(sc, root, p=q) for q in p])
        rounded = np.array([O.texture_eval(sc, root, p=q.astype(np.float32).astype(np.float64)) for q in p])
        rel = np.abs(exact - rounded).max(-1) / np.abs(exact).max()
        share[name] = float((rel > 1e-4).mean())
        print(f"{name}: {len(p)} hit points, {share[name]:.3f} of the values move by more than 1e-4 under an fp32 hit point, median {np.median(rel):.3e}")
    assert share["windy-s200"] > 0.25 and share["windy-s3"] < 0.01, share


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_f64_frame_matches_oracle(name, workdir):
    ref, counters, _ = _ref(name, workdir)
    r = Renderer(_scene(name, workdir), 0, RRT_F64)
    if TS.CASES[name].oracle == "panic":
        with pytest.raises(RrtPanic, match="path.rs:146 .*is_finite"):      # (the device reports the asserts of :146 and :147 as one)
            r.render()
        r.close()
        return
    film, st = r.render(stats=True)
    r.close()
    assert np.array_equal(film[..., 3], ref[..., 3])
    assert _counters(st) == counters
    diff = np.abs(film[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    print(f"{name}: f64 max {diff.max():.3e}")
    assert diff.max() < 1e-9, (diff.max(), int((diff > 1e-9).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in ALL if k != "wrinkled-saturated"])      # (its tint of 1e-200 is 0 in fp32, and 0 times a noise above FLT_MAX is no frame)
def test_fp32_frame_close_to_oracle(name, workdir):
    """The cases the table marks f64-only (texture_shapes.py argues each beside the case) keep everything here but the bars on the colour."""
    c = TS.CASES[name]
    ref, _, _ = _ref(name, workdir)
    r = Renderer(_scene(name, workdir), 0, RRT_F32)
    if c.oracle == "panic":
        assert c.fp32 == "panic"
        with pytest.raises(RrtPanic, match="path.rs:146"):
            r.render()
        r.close()
        return
    f32 = r.render().astype(np.float64)
    r.close()
    assert np.array_equal(f32[..., 3], ref[..., 3])
    assert np.all(np.isfinite(f32))
    d32 = np.abs(f32[..., :3] - ref[..., :3]).max(-1) / np.abs(ref[..., :3]).max()
    mean_rel = abs(f32[..., :3].mean() / ref[..., :3].mean() - 1)
    print(f"{name}: f32 within 1e-4: {(d32 < 1e-4).mean():.4f}, within 1e-3: {(d32 < 1e-3).mean():.4f}, median {np.median(d32):.3e}, max {d32.max():.3e}, mean rel {mean_rel:.3e}")
    if name in TS.F64_ONLY:
        print(f"{name}: f64 only ({c.fp32})")
    elif c.fp32 == "bump":
        assert "bump" in c.tags and c.carrier.endswith("_path")
        assert (d32 < 1e-3).mean() > 0.97, ((d32 < 1e-3).mean(), d32.max())
    else:
        assert (d32 < 1e-4).mean() > 0.97 and np.median(d32) < 1e-5, ((d32 < 1e-4).mean(), np.median(d32), d32.max())
    assert mean_rel < 0.02, mean_rel


ALBEDO_CASES = ["chk-su2-closedform", "round-spherical-identity-uv", "round-spherical-squashed-chk", "wrinkled-negative", "chk3-s3-negative", "depth-5", "shared",
                "slots-plastic", "uvmesh-uv"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALBEDO_CASES)
def test_albedo_plane(name, workdir):
    """The albedo plane's textures are evaluated with zero differentials: the census shows the point branches only (a closed-form checkerboard returns at
    "same cell", the noise keeps every octave). test_aov.py::test_f64_planes_match_reference's bar and test_fp32_planes_close_to_reference's."""
    import aov_reference as AR
    from test_aov import _value_diff
    sc = _scene(name, workdir)
    O.tex_census()
    ref = AR.planes(sc)["albedo"]
    census = O.tex_census()
    assert census["chk_filtered"] == 0 and census["chk_half"] == 0 and census["noise_partial"] == 0, census
    assert census["noise_all_octaves"] == census["noise_sums"] and sum(v for k, v in census.items() if k.startswith("node_")) > 1000, census
    assert ref[..., :3].max() > 0
    got = {}
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        got[prec] = r.render_aov(planes=("albedo",))["albedo"]
        r.close()
    diff = _value_diff("albedo", got[RRT_F64], ref)
    assert np.array_equal(got[RRT_F64][..., 3], ref[..., 3])
    spp = int(sc.desc.sampler.samples_per_pixel) - 1
    f32 = got[RRT_F32].astype(np.float64)
    live, live_ref = float(f32[..., 3].sum()), float(ref[..., 3].sum())
    covered = ref[..., 3] != 0
    w_diff = np.abs(f32[..., 3] - ref[..., 3]) / ref[..., 3].max()
    d = np.maximum(_value_diff("albedo", f32, ref), w_diff)
    assert np.all(f32[~covered & (f32[..., 3] == 0)] == 0)
    d = d[covered | (f32[..., 3] != 0)]
    print(f"{name}: albedo f64 max {diff.max():.3e}; fp32 at {spp} spp: within 1e-4: {(d < 1e-4).mean():.4f}, mean {d.mean():.3e}, max {d.max():.3e}, live {live} against {live_ref}")
    assert diff.max() < 1e-9, diff.max()
    assert (d < 1e-4).mean() >= 0.975 and d.mean() < 1e-4 and d.max() < 3e-2 * 256 / spp, ((d < 1e-4).mean(), d.mean(), d.max())
    assert abs(live - live_ref) <= 2e-5 * live_ref, (live, live_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TS.find(carrier="mirror"))
def test_followed_plane(name, workdir):
    """rrt_render_aov_follow through the mirror cube onto the textured enclosure, test_aov_follow.py's bars"""
    import aov_follow_reference as FR
    from test_aov_follow import PLANES, _channels, _value_diff
    sc = _scene(name, workdir)
    ref = FR.planes(sc, 2)
    spp = int(sc.desc.sampler.samples_per_pixel) - 1
    for prec in (RRT_F64, RRT_F32):
        r = Renderer(sc, 0, prec)
        got = r.render_aov(follow=2)
        r.close()
        for plane in PLANES:
            _, wc, _ = _channels(plane)
            diff = _value_diff(plane, got[plane], ref[plane])
            if prec == RRT_F64:
                print(f"{name}: followed f64 {plane}: max {diff.max():.3e}")
                assert np.array_equal(got[plane][..., wc], ref[plane][..., wc]), plane
                assert diff.max() < 1e-9, (plane, diff.max())
            else:
                covered = ref[plane][..., wc] != 0
                w_diff = np.abs(got[plane][..., wc].astype(np.float64) - ref[plane][..., wc]) / ref[plane][..., wc].max()
                d = np.maximum(diff, w_diff)[covered | (got[plane][..., wc] != 0)]
                print(f"{name}: followed fp32 {plane} at {spp} spp: within 1e-4: {(d < 1e-4).mean():.4f}, mean {d.mean():.3e}, max {d.max():.3e}")
                assert (d < 1e-4).mean() >= 0.975 and d.mean() < 1e-4 and d.max() < 3e-2 * 256 / spp, (plane, (d < 1e-4).mean(), d.mean(), d.max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chk-su2-closedform", "round-spherical-squashed-uv", "bump-wrinkled"])
def test_shortcuts_change_no_bit(name, workdir):
    """The shading-side options reorder or specialise the work around the texture evaluation and must not touch it (test_image_shapes.py)."""
    r = Renderer(_scene(name, workdir), 0, RRT_F32)
    base, st0 = r.render(stats=True)
    assert base[..., :3].max() > 0
    for opt in ("shade_compact", "shade_spec", "tile_order"):
        r.set_option(opt, 0)
        film, st = r.render(stats=True)
        r.set_option(opt, 1)
        assert np.array_equal(film, base), opt
        assert _counters(st) == _counters(st0), opt
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [RRT_F64, RRT_F32], ids=["f64", "f32"])
def test_depth_six_is_refused(prec, workdir):
    """kTexDepth = 5 levels are evaluated; a material whose graph has six is RRT_EUNSUP from render, render_aov and render_aov_follow, and five render"""
    r = Renderer(Scene.loads(*TS.refused_scene(workdir)), 0, prec)
    for call in (r.render, lambda: r.render_aov(planes=("albedo",)), lambda: r.render_aov(follow=2)):
        with pytest.raises(RrtUnsupported, match="texture graphs deeper than 5 levels"):
            call()
    r.close()
    r = Renderer(_scene("depth-5", workdir), 0, prec)
    film = r.render()
    r.close()
    assert np.all(np.isfinite(film)) and _lit(film) > CUBE_ONLY
