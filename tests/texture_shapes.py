"""Hand-built texture graphs, mappings and footprints for the procedural half of the device's texture code (dtexture.hpp: TexEval's node types, tex_map_2d,
map_round, the Perlin noise with noise_sum and the saturating casts, compute_differentials, solve_2x2; dkernels.hpp: Material::bump in build_bsdf_tex and
the triangle's uv / dpdu / dpdv / dndu / dndv in SurfExt) and for the host side that flattens the graph. Test infrastructure only.

A texture graph is caller-supplied data, as a tree (tests/bvh_shapes.py), a lens table (tests/lens_shapes.py), an image (tests/image_shapes.py) and a
material (tests/material_shapes.py) are. The six procedural cases of test_gpu_parity.py::test_textured_materials sit where the closed-form checkerboard
filter is mostly bypassed, use one placement of the round mappings with the centre far outside the walls' texture range, and noise at 4 to 5 octaves;
the table here walks the code through the rest, each case on a carrier where its branch is reached by many hits.

Carriers (64 x 64 films, nsamp 5; material_shapes.py's enclosure, slab and patch placement, scene_util.write_patch):
  walls        image_shapes.scene's frame (tilted cfg3, DirectLighting all, depth 1), the graph on the enclosure's material. The enclosure has no vt: every
               triangle has uv (0, 0), (1, 0), (1, 1), and the camera sees u >= 0.53 only (image_shapes.py)
  walls_path   the same under Path at depth 3: the bounces carry no auxiliary rays, so their footprint is zero
  mirror       walls at depth 3 with the cube a MirrorMaterial: the enclosure is hit a second time through k_direct_tree's inherited differentials.
               The census cannot tell a camera hit from an inherited one; test_texture_shapes.py compares the evaluation count with the walls case's
  patch        walls with write_patch's curved 6 x 6 patch (vt, smooth vn) carrying the material; patch_path the same under Path at depth 3
  uvmesh       walls with a flat 4 x 4 quad grid (write_uvmesh) where the patch is, whose vt are made per face: regular, mirrored (negative determinant),
               degenerate (three equal vt), collinear (|det| < 1e-8) and scaled to [-2, 3] - each kind on three or four sixteenths of the mesh.
               uvmesh_vn has smooth vn as well (dndu / dndv through coordinate_system(dn) on the degenerate faces); uvmesh_x / uvmesh_z stand the
               mesh up so that its normal's largest component is x / z
  uvmesh_huge  uvmesh_vn with a sixth kind: huge, uv from -2e5 to 2e5 over the quad, dpdu and dpdv so short that solve_2x2's |det| < 1e-10 refuses
               them. That refusal needs |dpdu x dpdv| < 1e-10, i.e. a uv area of 1e10 times the face's own: on any face large enough to be hit, uv
               beyond 1e4, where an fp32 barycentric (one ulp 6e-8, times 2e5: 0.012) no longer places u within a hundredth of a unit. So the cases
               on this mesh use textures that do not read uv at unit frequency (a checkerboard with cells of 1e5, a 3D noise, constants with a
               zero mapping: cf0 / cr0 below), and the other meshes leave the kind out
  slab         material_shapes.py's slab under Path (depth 5), for the transmissive materials of the slot cases

A case is (group, tags, carrier, floats, rgbs, materials, fp32, oracle). `floats` / `rgbs` are the scene's float_texture / rgb_texture lists, `materials` the
material on the carrier (and, where there are two, on the cube). A tag names what the oracle's texture census (oracle_lib.tex_census, counted by the oracle
and not by the code under test) must show for ONE frame of the case; census_problems() states it and test_texture_shapes.py asserts it on the CPU for every
case. `fp32` is "bar" (test_textured_materials' fp32 bars), "bump" (its path_bump_patch bar, bump-mapped Path cases only) or "f64_only: <finding>".
`oracle` records what the reference's own arithmetic does with the case: "frame", or "panic" where it asserts - recorded from the oracle, never from the
code under test.

What the carriers give and do not give (measured on the oracle, placements chosen on the CPU):
  noise on walls   compute_differentials keeps the reference's `ty` quirk (interaction.rs:234), so dpdy is as long as the scene and a camera hit has
                   l2 >> 1: n = 0 at every texture scale above some 0.01. The camera footprints therefore give noise_none at scale 0.3 to 200 and
                   noise_partial only at scale 0.002; noise_all_octaves comes from walls_path's bounces (l2 = 0, n = octaves)
  round_seam       the cylindrical mapping has no `phi < 0` wrap (texture/mod.rs: cylinder() adds pi instead): round_seam (the wrap and all four folds)
                   is asked of the spherical squashed placement, round_fold (the four folds, no wrap) of the cylindrical one - ROUND_PLACES below says
                   why an isotropic placement cannot give the folds; the identity placements give the poles and the wrapped half
  bump_du_fallback a degenerate-uv face does NOT reach `du == 0` under DirectLighting: its dpdu / dpdv come from coordinate_system and solve_2x2
                   succeeds. The face that does is the huge one (solve_2x2 refuses, dudx = dudy = 0); the tag is met there
  diff_not_finite  tx or ty infinite needs dot(n, rxd) == 0 exactly; no placement of these carriers under a thin-lens camera gives it, and no case
                   claims it (tests/test_oracle.py covers the branch through oracle_lib.surface_differentials)
"""
import collections
import copy
import os

import material_shapes as MS

Case = collections.namedtuple("Case", "group tags carrier floats rgbs materials fp32 oracle")

XRES = YRES = 64
NSAMP = 5
ROT = {"rotation_axis": [1.0, 2.0, 0.5], "rotation_angle": 25.0}      # test_gpu_parity.py's generic texture rotation
NO_ROT = {"rotation_axis": [0.0, 0.0, 1.0], "rotation_angle": 0.0}    # (make_to_world normalises the axis: an absent one is a NaN matrix)
FAR_NEGATIVE = [-300.0, -200.0, -100.0]                                # texture space = R S p + world_pos: the scene at negative coordinates
TINT, DARK, LIGHT = [0.9, 0.6, 0.3], [0.15, 0.1, 0.3], [0.8, 0.8, 0.7]
# Where the round mappings sit. The camera sees the enclosure's corner near (76, -18, 37): the floor (x 45 to 77, z 1 to 36), the back wall (y -18 to 0,
# z 12 to 37) and a side wall (x 60 to 77, y -20 to -1).
#   identity   the axis along world z through the side wall's visible middle: the pole (68, -10, 37) and the plane y = -10 are in view
#   rotated    the generic rotation about the generic centre
#   squashed   a step of 0.1 dpdx is some 0.08 world units, and a fold needs dst[1] to move by more than 0.05 over it: with an isotropic placement that
#              happens on a handful of hits beside the seam, in one direction only (dpdx points one way on a wall). A scale of 0.003 along one
#              texture axis compresses the change of phi (spherical: texture y, turned onto world z, so the plane z = 18 with its seam half crosses
#              floor and back wall) or of v.z (cylindrical: texture z, turned onto world (1, 0, 1), along which dpdx points one way on the floor and
#              the other way on the side wall) into a thin wedge that many hits straddle, from either side
ROUND_PLACES = {
    "spherical": {"identity": {"world_pos": [68.0, -10.0, 15.0], **NO_ROT}, "rotated": {"world_pos": [60.0, -9.0, 20.0], **ROT},
                  "squashed": {"world_pos": [62.0, -8.0, 18.0], "rotation_axis": [1.0, 0.0, 0.0], "rotation_angle": 90.0, "scale": [1.0, 0.003, 1.0]}},
    "cylindrical": {"identity": {"world_pos": [68.0, -10.0, 15.0], **NO_ROT}, "rotated": {"world_pos": [60.0, -9.0, 20.0], **ROT},
                    "squashed": {"world_pos": [68.0, -10.0, 32.0], "rotation_axis": [0.0, 1.0, 0.0], "rotation_angle": 45.0, "scale": [1.0, 1.0, 0.003]}},
}
# the huge quad's uv run from -2e5 to 2e5 over its 3.5 units: |dpdu| = |dpdv| = 8.75e-6, so the 2 x 2 determinant is at most 7.7e-11 < 1e-10 whatever the
# dominant axis, with a quarter to spare in either precision; an fp32 uv of 2e5 still resolves 1 / 64 of a unit
HUGE_UV = 4e5
FALLBACK_STEP_HEIGHT = 0.0005
BUMP_CHECKER = (0.3, 0.5, 0.5)      # (su = sv, du = dv, height) of bump-checker-closedform: 82 % of its evaluations filtered, none on the shortcut
UVMESH_KINDS = ("regular", "mirrored", "degenerate", "collinear", "scaled")
UVMESH_INSTANCES = {
    "uvmesh": MS.PATCH_INSTANCE, "uvmesh_vn": MS.PATCH_INSTANCE, "uvmesh_huge": MS.PATCH_INSTANCE,
    # the mesh's normal is +y in object space: turned about z towards the camera (normal mostly -x), and about x (normal mostly +-z)
    "uvmesh_x": {"world_pos": [30.0, -0.5, -5.0], "rotation_axis": [0.1, 0.2, 1.0], "rotation_angle": 70},
    "uvmesh_z": {"world_pos": [26.0, -0.5, -5.0], "rotation_axis": [1.0, 0.3, 0.1], "rotation_angle": 65},
}


def cf(name, v): return {"texture_type": "BilerpTexture", "texture_name": name, "v00": v, "v01": v}
def cr(name, v): return {"texture_type": "BilerpTexture", "texture_name": name, "v00": {"values": list(v)}, "v01": {"values": list(v)}}
# a constant whose mapping is (0, 0, 0, 0): s = t = 0 and the bilerp expression is v00 itself. The loader does not fold a constant CHILD: it is evaluated
# through v00 (1 - s)(1 - t) + v01 (1 - s) t + .. at the hit's (u, v), and on the huge quad (u, v up to 2e5) those are four terms of 4e10 that cancel to
# the constant - to 4e-6 in f64, not at all in fp32
def cf0(name, v): return {**cf(name, v), "mapping": uvmap(0.0, 0.0, 0.0, 0.0)}
def cr0(name, v): return {**cr(name, v), "mapping": uvmap(0.0, 0.0, 0.0, 0.0)}
def uvmap(su, sv=None, du=0.0, dv=0.0): return {"mapping": "uv", "su": su, "sv": su if sv is None else sv, "du": du, "dv": dv}
def uvtex(name, mapping=None, **kw): return {"texture_type": "UVTexture", "texture_name": name, "mapping": mapping or uvmap(2.0, 3.0), **kw}
def scale(name, t1, t2): return {"texture_type": "ScaleTexture", "texture_name": name, "t1": t1, "t2": t2}
def mix(name, t1, t2): return {"texture_type": "MixTexture", "texture_name": name, "t1": t1, "t2": t2}


def checker(name, t1, t2, mapping, aamode="closedform", **kw):
    return {"texture_type": "CheckerBoardTexture", "texture_name": name, "t1": t1, "t2": t2, "aamode": aamode, "mapping": mapping, **kw}


def checker3(name, t1, t2, **kw): return {"texture_type": "CheckerBoardTexture", "texture_name": name, "dimension": 3, "t1": t1, "t2": t2, **kw}
def wrinkled(name, octaves, omega, **kw): return {"texture_type": "WrinkledTexture", "texture_name": name, "octaves": octaves, "omega": omega, **kw}
def windy(name, **kw): return {"texture_type": "WindyTexture", "texture_name": name, **kw}
def matte(**kw): return {"material_type": "MatteMaterial", **kw}
def s3(v): return {"scale": [v, v, v]}


def _cases():
    out = {}

    def add(name, group, tags, carrier, floats=(), rgbs=(), materials=None, fp32="bar", oracle="frame"):
        assert name not in out, name
        if isinstance(tags, str): tags = (tags,)
        out[name] = Case(group, tuple(tags), carrier, list(floats), list(rgbs), list(materials or [matte(kd="root")]), fp32, oracle)

    two = [cr("a", LIGHT), cr("b", DARK)]

    # ---- checker: s = su (u - 1.3) and t = su (v - 1.3) are negative on every hit (u, v <= 1), and so is every cell sum
    for su in (0.5, 2.0, 6.0, 40.0):
        for aamode in ("closedform", "none"):
            tags = {0.5: ["chk_closedform"], 2.0: ["chk_filtered"], 6.0: ["chk_closedform"], 40.0: ["chk_half"]}[su] if aamode == "closedform" else ["chk_none"]
            add(f"chk-su{su:g}-{aamode}", "checker", tags + ["chk_negative"], "walls", rgbs=two + [checker("root", "a", "b", uvmap(su, su, -1.3 * su, -1.3 * su), aamode)])
    add("chk-su6-point", "checker", ["chk_point", "chk_negative"], "walls_path", rgbs=two + [checker("root", "a", "b", uvmap(6.0, 6.0, -7.8, -7.8))])
    add("chk-planar-generic", "checker", ["chk_closedform", "chk_negative"], "walls",
        rgbs=two + [checker("root", "a", "b", {"mapping": "planar", "v1": [0.05, 0.02, 0.01], "v2": [-0.01, 0.02, 0.06], "udelta": -3.3, "vdelta": -1.1})])
    add("chk-planar-parallel", "checker", ["chk_closedform"], "walls",
        rgbs=two + [checker("root", "a", "b", {"mapping": "planar", "v1": [0.02, 0.04, 0.03], "v2": [0.04, 0.08, 0.06], "udelta": 0.3, "vdelta": 0.1})])
    add("chk-children", "checker", ["chk_filtered", "chk_negative", "node_uv"], "walls",
        rgbs=two + [uvtex("uvt"), checker("inner", "a", "b", uvmap(3.0, 5.0, 0.25, 0.5), "none"), checker("root", "uvt", "inner", uvmap(2.0, 2.0, -2.6, -2.6))])

    # ---- round: centre inside the enclosure, scale 1; the identity rotation puts the seam plane y = 0, x < 0 and the poles +-z on walls
    for kind in ("spherical", "cylindrical"):
        for rot_name, place in ROUND_PLACES[kind].items():
            place = {"mapping": {"mapping": kind}, **place}
            tags = {"identity": ["round_pole"], "rotated": [], "squashed": ["round_seam" if kind == "spherical" else "round_fold"]}[rot_name]
            tags = tags + (["round_wrap"] if kind == "spherical" else ["round_no_wrap"])
            add(f"round-{kind}-{rot_name}-uv", "round", tags, "walls", rgbs=[{"texture_type": "UVTexture", "texture_name": "root", **place}])
            add(f"round-{kind}-{rot_name}-chk", "round", tags + ["node_checker2d"], "walls",
                rgbs=two + [{"texture_type": "CheckerBoardTexture", "texture_name": "root", "t1": "a", "t2": "b", **place}])

    # ---- noise (the module docstring: camera hits have n = 0 unless the scale is tiny; walls_path's bounces have n = octaves)
    tinted = lambda tex: [cr("tint", TINT), tex, scale("root", "n", "tint")]
    for octaves in (0, 1, 8, 12):
        add(f"wrinkled-o{octaves}-w0.5", "noise", ["noise_all_octaves", "noise_none"], "walls_path", rgbs=tinted(wrinkled("n", octaves, 0.5, **ROT, **s3(0.3))))
    for omega in (0.0, 1.0, 1.5):
        add(f"wrinkled-o8-w{omega:g}", "noise", ["noise_all_octaves", "noise_none"], "walls_path", rgbs=tinted(wrinkled("n", 8, omega, **ROT, **s3(0.3))))
    add("wrinkled-partial", "noise", ["noise_partial"], "walls", rgbs=tinted(wrinkled("n", 8, 0.5, **ROT, **s3(0.002), world_pos=[7.3, 2.1, 5.9])))
    add("wrinkled-camera", "noise", ["noise_none"], "walls", rgbs=tinted(wrinkled("n", 8, 0.5, **ROT)))
    add("wrinkled-negative", "noise", ["noise_negative", "noise_all_octaves"], "walls_path", rgbs=tinted(wrinkled("n", 8, 0.5, **ROT, **s3(0.3), world_pos=FAR_NEGATIVE)))
    # Windy is signed (|fbm| * fbm) and a negative kd is a black surface: an rgb Mix with a constant lifts it to 0.25 + 0.5 windy (the amount is the
    # fallback 0.5: no float texture is named `n`)
    lifted = lambda tex: [cr("half", [0.5, 0.5, 0.5]), tex, mix("root", "half", "n")]
    # scale 200 is f64 only: one fp32 ulp of a hit point at x = 50 (3.8e-6) is 7.6e-4 texture units at the first octave and 0.024 at the sixth, where
    # the noise changes by order one per unit. Shown on the oracle alone (test_texture_shapes.py::test_f64_only_arguments): with nothing but the hit
    # point ROUNDED to fp32, 41 % of the texture's values on the walls move by more than 1e-4 of the largest (none at scale 3), while rounding
    # world_to_texture alone moves 0.05 % of the frame's pixels that far. Measured: 94.4 % of the pixels within 1e-4 where the bar asks 97 %, median
    # 5.7e-6, largest 5.5e-3, mean within 1.6e-5; the f64 frame equals the oracle's, weights exact
    for sc_ in (0.05, 3.0, 200.0):
        add(f"windy-s{sc_:g}", "noise", ["noise_windy", "noise_all_octaves"], "walls_path", rgbs=lifted(windy("n", **ROT, **s3(sc_))),
            fp32="bar" if sc_ < 200.0 else "f64_only: an fp32 hit point resolves 7.6e-4 texture units at scale 200, 0.024 at the sixth octave")
    add("windy-partial", "noise", ["noise_windy", "noise_partial"], "walls", rgbs=lifted(windy("n", **ROT, **s3(0.004), world_pos=[7.3, 2.1, 5.9])))
    add("windy-negative", "noise", ["noise_windy", "noise_negative"], "walls_path", rgbs=lifted(windy("n", **ROT, **s3(3.0), world_pos=FAR_NEGATIVE)))
    # scale 1e9: every coordinate past 2^31, f2i_sat saturates and dx = x - ix is as large as x. f64 only: world_to_texture is stored in the mode's
    # precision, and an fp32 matrix entry of 1e9 carries a rounding of up to 32, which times a scene coordinate moves the noise argument by whole lattice
    # cells - any fp32 storage of the matrix does that, whatever the evaluation (shown on the oracle alone: test_texture_shapes.py::test_point_values)
    # Past 2^31 the weights 6 dx^5 are astronomic (noise() of some 1e170 at the first octave, 1e210 at the eighth): a tint of 1e-200 brings Wrinkled back
    # into range, and the frame is decided by its few largest pixels. Windy multiplies two such sums, the product overflows, and path.rs:147 asserts on
    # beta: the device has to panic with it
    tiny = lambda tex: [cr("tint", [1e-200, 6e-201, 3e-201]), tex, scale("root", "n", "tint")]
    add("wrinkled-saturated", "noise", ["noise_saturated"], "walls_path", rgbs=tiny(wrinkled("n", 8, 0.5, **ROT, **s3(1e9))),
        fp32="f64_only: world_to_texture at scale 1e9 rounds by whole lattice cells in fp32")
    add("windy-saturated", "noise", ["noise_saturated", "noise_windy"], "walls_path", rgbs=tiny(windy("n", **ROT, **s3(1e9))),
        fp32="panic", oracle="panic")
    for sc_ in (0.1, 3.0):
        add(f"chk3-s{sc_:g}-negative", "noise", ["chk3_negative"], "walls", rgbs=two + [checker3("root", "a", "b", **ROT, **s3(sc_), world_pos=[-80.0 * sc_, -30.0 * sc_, -60.0 * sc_])])
    bump_of = lambda tex, amp: [tex, cf("amp", amp), scale("bumpy", "n", "amp")]
    bumped = [matte(bump_map="bumpy")]
    # Under DirectLighting the footprint of a camera hit takes every octave away above scale 0.01 (module docstring), and a noise without octaves is a
    # constant (Wrinkled) or 0 (Windy): Material::bump's three evaluations would agree and its finite difference be 0. So the camera-footprint bumps sit
    # at the scales where octaves survive, with an amplitude that makes up for the slow change; `bump` asks that the difference is not 0 on most hits
    add("bump-wrinkled", "noise", ["bump", "noise_partial"], "patch", floats=bump_of(wrinkled("n", 8, 0.5, **ROT, **s3(0.002), world_pos=[7.3, 2.1, 5.9]), 30.0), materials=bumped)
    add("bump-windy", "noise", ["bump", "noise_windy", "noise_partial"], "patch", floats=bump_of(windy("n", **ROT, **s3(0.004), world_pos=[7.3, 2.1, 5.9]), 40.0), materials=bumped)
    add("bump-chk3", "noise", ["bump", "node_checker3d"], "patch", floats=[cf("lo", 0.0), cf("hi", 0.04), checker3("bumpy", "lo", "hi", **ROT, **s3(0.7))], materials=bumped)
    add("bump-wrinkled-path", "noise", ["bump", "bump_du_fallback", "noise_all_octaves"], "walls_path",
        floats=bump_of(wrinkled("n", 4, 0.5, **ROT, **s3(2.0)), 0.03), materials=bumped, fp32="bump")

    # ---- graph: chains of depth 1 to 5 over a UV leaf (depth 6: refused_scene below)
    for depth in range(1, 6):
        add(f"depth-{depth}", "graph", [f"depth_{depth}", "node_uv"], "walls", floats=[cf("tint", 0.3)], rgbs=chain(depth), materials=[matte(kd=f"L{depth}")])
    # a diamond: one leaf under two parents, the parents under one Mix, the root on two materials
    add("shared", "graph", ["shared", "depth_3"], "walls",
        rgbs=[cr("tint", TINT), cr("dark", DARK), uvtex("leaf"), scale("p1", "leaf", "tint"), mix("p2", "leaf", "dark"), mix("root", "p1", "p2")],
        materials=[matte(kd="root"), {"material_type": "PlasticMaterial", "kd": "root", "ks": "root"}])
    base = [cr("tint", TINT), uvtex("uvt"), uvtex("uvt2", uvmap(5.0, 1.0, 0.5, 0.0))]
    add("fallback-mix-t1", "graph", ["fb_mix_t1", "fb_mix_amount"], "walls", rgbs=base + [mix("root", "nope", "uvt")])
    add("fallback-mix-t2", "graph", ["fb_mix_t2", "fb_mix_amount"], "walls", rgbs=base + [mix("root", "uvt", "nope")])
    add("fallback-scale-t1", "graph", ["fb_scale_t1"], "walls", rgbs=base + [scale("root", "nope", "uvt2")])
    add("fallback-scale-t2", "graph", ["fb_scale_t2"], "walls", rgbs=base + [scale("root", "uvt", "nope")])
    add("fallback-checker-t1", "graph", ["fb_checker_t1"], "walls", rgbs=base + [checker("root", "nope", "uvt", uvmap(4.0), "none")])
    add("fallback-checker-t2", "graph", ["fb_checker_t2"], "walls", rgbs=base + [checker("root", "uvt", "nope", uvmap(4.0), "none")])
    # the Mix quirks (renderprocess.rs:318 and :412-414): the float Mix reads the `t2` name for its amount, the rgb Mix takes its amount from the FLOAT
    # texture that `t2` names
    add("mix-rgb-amount", "graph", ["mix_amount_textured"], "walls", floats=[{"texture_type": "BilerpTexture", "texture_name": "tint", "v00": 0.0, "v01": 1.0, "mapping": uvmap(1.0)}],
        rgbs=base + [mix("root", "uvt", "tint")])
    add("mix-float-amount", "graph", ["mix_amount_textured", "slots:sigma"], "walls",
        floats=[cf("lo", 10.0), {"texture_type": "BilerpTexture", "texture_name": "ramp", "v00": 0.0, "v01": 1.0, "mapping": uvmap(1.0)}, mix("sig", "lo", "ramp"), cf("s60", 60.0), scale("sigma", "sig", "s60")],
        rgbs=[cr("kd", LIGHT)], materials=[matte(kd="kd", sigma="sigma")])
    add("amount-outside", "graph", ["amount_outside"], "walls",
        floats=[{"texture_type": "BilerpTexture", "texture_name": "ramp", "v00": -0.2, "v01": 0.8, "mapping": uvmap(1.0)}, cf("c2.5", 2.5), scale("tint", "ramp", "c2.5")],
        rgbs=base + [mix("root", "uvt", "tint")])
    add("negative-kd", "graph", ["negative_value"], "walls", rgbs=[cr("neg", [-1.0, 0.5, -0.2]), uvtex("uvt"), scale("root", "uvt", "neg")])
    add("negative-sigma", "graph", ["negative_value", "slots:sigma"], "walls",
        floats=[{"texture_type": "BilerpTexture", "texture_name": "ramp", "v00": -1.0, "v01": 1.0, "mapping": uvmap(1.0)}, cf("m40", -40.0), scale("sigma", "ramp", "m40")],
        rgbs=[cr("kd", LIGHT)], materials=[matte(kd="kd", sigma="sigma")])
    # the later texture owns the name; a parent made before it keeps the earlier one
    add("duplicate-names", "graph", ["node_uv", "node_scale"], "walls", rgbs=[cr("tint", TINT), cr("dup", DARK), scale("early", "dup", "tint"), uvtex("dup"), checker("root", "early", "dup", uvmap(4.0), "none")])

    # ---- slots: every textured parameter of resolve_material driven per hit by a two-constant aamode-none checkerboard, as material_shapes.py does it
    def per_hit(rgb=(), flt=()):
        fl, rg = [], []
        for k, (a, b) in flt:
            fl += [cf(f"{k}_a", a), cf(f"{k}_b", b), checker(f"p_{k}", f"{k}_a", f"{k}_b", dict(MS.CHECKER), "none")]
        for k, (a, b) in rgb:
            rg += [cr(f"{k}_a", a), cr(f"{k}_b", b), checker(f"p_{k}", f"{k}_a", f"{k}_b", dict(MS.CHECKER), "none")]
        return fl, rg

    fl, rg = per_hit(rgb=[("kd", (LIGHT, DARK)), ("ks", (DARK, LIGHT))], flt=[("roughness", (0.05, 0.4))])
    add("slots-plastic", "slots", ["slots:kd,ks,roughness"], "walls_path", floats=fl, rgbs=rg,
        materials=[{"material_type": "PlasticMaterial", "kd": "p_kd", "ks": "p_ks", "roughness": "p_roughness"}])
    fl, rg = per_hit(rgb=[("eta", ([0.2, 0.9, 1.1], [1.5, 0.6, 0.3])), ("k", ([3.9, 2.4, 2.2], [0.5, 1.0, 3.0]))], flt=[("u_roughness", (0.05, 0.4)), ("v_roughness", (0.3, 0.08))])
    add("slots-metal", "slots", ["slots:eta,k,u_roughness,v_roughness"], "patch_path", floats=fl, rgbs=rg,
        materials=[{"material_type": "MetalMaterial", "eta": "p_eta", "k": "p_k", "u_roughness": "p_u_roughness", "v_roughness": "p_v_roughness"}])
    fl, rg = per_hit(rgb=[("kr", (LIGHT, DARK)), ("kt", (TINT, LIGHT))], flt=[("eta", (1.3, 1.7))])
    add("slots-glass", "slots", ["slots:kr,kt,index"], "slab", floats=fl, rgbs=rg, materials=[{"material_type": "GlassMaterial", "kr": "p_kr", "kt": "p_kt", "eta": "p_eta"}])
    fl, rg = per_hit(rgb=[("kd", (LIGHT, DARK)), ("ks", (DARK, TINT)), ("reflect", (LIGHT, TINT)), ("transmit", (TINT, LIGHT))], flt=[("roughness", (0.2, 0.5))])
    add("slots-translucent", "slots", ["slots:kd,ks,reflect,transmit,roughness"], "slab", floats=fl, rgbs=rg,
        materials=[{"material_type": "TranslucentMaterial", "kd": "p_kd", "ks": "p_ks", "reflect": "p_reflect", "transmit": "p_transmit", "roughness": "p_roughness"}])
    add("slots-mirror-kr", "slots", ["slots:kr", "chk_closedform"], "walls", rgbs=two + [checker("root", "a", "b", uvmap(2.0, 2.0, -2.6, -2.6))],
        materials=[matte(kd="root"), {"material_type": "MirrorMaterial", "kr": "root"}])

    # ---- diff: the triangle's uv kinds, the three dominant-axis branches, solve_2x2 refusing, inherited differentials
    mesh_chk = two + [checker("root", "a", "b", uvmap(2.0, 2.0, 0.3, 0.3))]
    add("uvmesh-chk", "diff", ["tri_degenerate", "tri_negative_det", "chk_closedform"], "uvmesh", rgbs=mesh_chk)
    add("uvmesh-vn-chk", "diff", ["tri_degenerate", "tri_negative_det", "tri_coord_dn", "chk_closedform"], "uvmesh_vn", rgbs=mesh_chk)
    add("uvmesh-huge-chk", "diff", ["tri_degenerate", "tri_coord_dn", "solve_failed", "node_checker2d"], "uvmesh_huge",
        rgbs=[cr0("a", LIGHT), cr0("b", DARK), checker("root", "a", "b", uvmap(1e-5, 1e-5, 0.3, 0.3))])
    add("uvmesh-vn-mirror", "diff", ["tri_degenerate", "tri_coord_dn", "slots:kr"], "uvmesh_vn", rgbs=mesh_chk, materials=[{"material_type": "MirrorMaterial", "kr": "root"}])
    add("uvmesh-uv", "diff", ["tri_degenerate", "tri_negative_det", "node_uv"], "uvmesh", rgbs=[uvtex("root", uvmap(1.0, 1.0, 0.0, 0.0))])
    add("axes-walls", "diff", ["diff_axes"], "uvmesh_x", rgbs=mesh_chk, materials=[matte(kd="root"), None, matte(kd="root")])
    add("axes-z", "diff", ["diff_axis_xy"], "uvmesh_z", rgbs=mesh_chk)
    for su in (1.0, 2.0):
        add(f"mirror-su{su:g}", "diff", ["chk_filtered_some", "chk_negative"], "mirror", rgbs=two + [checker("root", "a", "b", uvmap(su, su, -1.3 * su, -1.3 * su))])

    # ---- bump
    # The du == 0 fallback steps 0.0005 along the unit shading dpdu (the mesh has vn). A displacement that is linear over that step gives the same slope for
    # any step, and a device with another fallback would pass; a 3D checkerboard with cells of 0.001 (not filtered, evaluated on the double hit point) is
    # 0 or FALLBACK_STEP_HEIGHT apart over it, so that the slope is 0 on some fallback hits and +-1 on the others (bump_fallback_mixed) - which hits, and
    # how steep, both depend on the 0.0005. (A uv texture cannot serve: on the huge face u + 0.0005 is u in fp32.) Off the fallback the step is as long as
    # the scene and the slope is nothing
    add("bump-du-fallback", "bump", ["bump_some", "bump_du_fallback", "bump_fallback_mixed", "solve_failed"], "uvmesh_huge",
        floats=[cf0("lo", 0.0), cf0("hi", FALLBACK_STEP_HEIGHT), checker3("bumpy", "lo", "hi", **ROT, **s3(1000.0))], materials=bumped)
    ramp = lambda name, top: {"texture_type": "BilerpTexture", "texture_name": name, "v00": 0.0, "v01": top, "mapping": uvmap(1.0)}
    # the displacement is the closed-form filter's own output: the filtered branch has to dominate in Material::bump's evaluations too
    add("bump-checker-closedform", "bump", ["bump", "chk_filtered"], "patch", floats=[cf("amp", BUMP_CHECKER[2]), checker("bumpy", "amp", "nope", uvmap(BUMP_CHECKER[0], BUMP_CHECKER[0], BUMP_CHECKER[1], BUMP_CHECKER[1]))], materials=bumped)
    add("bump-depth5", "bump", ["bump", "depth_5"], "patch",
        floats=[cf("lo", 0.01), cf("hi", 0.3), cf("amp", 0.7), ramp("B5", 2.0), scale("B4", "B5", "amp"), checker("B3", "B4", "lo", uvmap(5.0), "none"),
                mix("B2", "B3", "hi"), scale("bumpy", "B2", "amp")], materials=bumped)
    # the same uv ramp on the quad mesh without and with vn: displace * dndu enters with vn only, and the mirrored, degenerate and collinear faces take
    # their du, dv and dpdu from their own uv
    add("bump-ramp-uvmesh", "bump", ["bump", "tri_degenerate", "tri_negative_det"], "uvmesh", floats=[ramp("bumpy", 2.0)], materials=bumped)
    add("bump-ramp-uvmesh-vn", "bump", ["bump", "tri_degenerate", "tri_negative_det", "tri_coord_dn"], "uvmesh_vn", floats=[ramp("bumpy", 2.0)], materials=bumped)
    return out


def chain(depth):
    """rgb textures L1 .. L<depth>: L1 a UV leaf, then Scale, Checkerboard (aamode none), Mix, Scale, Checkerboard over it in turn. L<depth> is the root and
    evaluates `depth` levels. (The rgb Mix's amount is the float texture named `tint`.)"""
    out = [cr("tint", TINT), cr("dark", DARK), uvtex("L1")]
    makers = [lambda n, c: scale(n, c, "tint"), lambda n, c: checker(n, c, "dark", uvmap(4.0, 4.0, 0.0, 0.0), "none"), lambda n, c: mix(n, c, "tint")]
    for level in range(2, depth + 1):
        out.append(makers[(level - 2) % 3](f"L{level}", f"L{level - 1}"))
    return out


CASES = _cases()
F64_ONLY = [k for k, c in CASES.items() if c.fp32.startswith("f64_only")]
assert len(F64_ONLY) <= 4


def find(group=None, tag=None, carrier=None):
    return [k for k, c in CASES.items() if (group is None or c.group == group) and (tag is None or tag in c.tags) and (carrier is None or c.carrier == carrier)]


def write_uvmesh(wd, with_vn, huge=False, half=7.0, bend=0.02):
    """The flat 4 x 4 quad grid of the module docstring (y = 0, normal +y, write_patch's winding and extent) as uvmesh.obj / uvmesh_vn.obj / uvmesh_huge.obj.
    Quad q (row-major) is of kind q modulo the number of kinds (UVMESH_KINDS, and "huge" after them if asked for); every face has vt of its own. The vn are those of write_patch's curved surface: they vary over a face, which is what
    coordinate_system(dn) needs."""
    import numpy as np
    n = 4
    xs = [-half + 2.0 * half * i / n for i in range(n + 1)]
    lines = [f"v {x:.6f} 0.000000 {z:.6f}" for z in xs for x in xs]
    if with_vn:
        for z in xs:
            for x in xs:
                g = np.array([-2.0 * bend * x, 1.0, -bend * z]); g /= np.linalg.norm(g)
                lines.append(f"vn {g[0]:.6f} {g[1]:.6f} {g[2]:.6f}")
    faces, n_vt = [], 0
    for j in range(n):
        for i in range(n):
            kinds = UVMESH_KINDS + (("huge",) if huge else ())
            kind = kinds[(j * n + i) % len(kinds)]
            corners = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]      # a, b, c, d
            if kind == "regular": uv = [(ci / n, cj / n) for ci, cj in corners]
            elif kind == "mirrored": uv = [(1.0 - ci / n, cj / n) for ci, cj in corners]
            elif kind == "degenerate": uv = [(0.3, 0.6)] * 4
            elif kind == "collinear": uv = [(0.125, 0.125), (0.25, 0.25), (0.5, 0.5), (0.375, 0.375)]      # (dyadic: the determinant is 0 in either precision)
            elif kind == "scaled": uv = [(-2.0 + 5.0 * (ci - i), -2.0 + 5.0 * (cj - j)) for ci, cj in corners]
            else: uv = [(HUGE_UV * (ci - i - 0.5), HUGE_UV * (cj - j - 0.5)) for ci, cj in corners]
            for u, v in uv: lines.append(f"vt {u:.9g} {v:.9g}")
            a, b, c, d = [cj * (n + 1) + ci + 1 for ci, cj in corners]
            ta, tb, tc, td = n_vt + 1, n_vt + 2, n_vt + 3, n_vt + 4
            n_vt += 4
            ref = (lambda p, t: f"{p}/{t}/{p}") if with_vn else (lambda p, t: f"{p}/{t}")
            faces.append(f"f {ref(a, ta)} {ref(d, td)} {ref(c, tc)}")
            faces.append(f"f {ref(a, ta)} {ref(c, tc)} {ref(b, tb)}")
    name = "uvmesh_huge.obj" if huge else ("uvmesh_vn.obj" if with_vn else "uvmesh.obj")
    with open(os.path.join(wd, name), "w") as f:
        f.write("\n".join(lines + faces) + "\n")
    return name


def _frame(wd, carrier):
    """(cfg, root, the primitives that carry materials[0], the cube) of a carrier, textures and materials not yet added"""
    from scene_util import write_patch
    path = carrier in ("walls_path", "patch_path", "slab")
    cfg, root = MS._enclosure(wd, NSAMP, 5 if carrier == "slab" else 3)
    if not path:
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 3 if carrier == "mirror" else 1}
    cube, box = cfg["Aggregate"]["primitives"]
    if carrier in ("walls", "walls_path", "mirror"):
        return cfg, root, box, cube
    if carrier == "slab":
        MS._slab(wd, cfg)
        return cfg, root, cfg["Aggregate"]["primitives"][0], None
    if carrier in ("patch", "patch_path"):
        write_patch(wd)
        obj, inst = "patch.obj", MS.PATCH_INSTANCE
    else:
        obj, inst = write_uvmesh(wd, carrier in ("uvmesh_vn", "uvmesh_huge"), carrier == "uvmesh_huge"), UVMESH_INSTANCES[carrier]
    cfg["objs"] = cfg["objs"] + [{"filename": obj, "obj_name": "carrier_01"}]
    prim = {"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "carrier_01", "instances": [copy.deepcopy(inst)]}
    cfg["Aggregate"]["primitives"].append(prim)
    return cfg, root, prim, cube


def scene(wd, name):
    """The frame of the module docstring for the case (a Case or an id); returns (cfg, root) for Scene.loads. materials[0] goes on the carrier as m_case,
    materials[1] (if any) on the cube as m_cube, materials[2] (if any) on the enclosure as m_box."""
    c = CASES[name] if isinstance(name, str) else name
    cfg, root, target, cube = _frame(wd, c.carrier)
    cfg["float_texture"] = copy.deepcopy(c.floats)
    cfg["rgb_texture"] = copy.deepcopy(c.rgbs)
    mats = list(c.materials)
    if c.carrier == "mirror" and len(mats) == 1:
        cfg["rgb_texture"].append(cr("mirror_kr", [0.9, 0.9, 0.9]))
        mats.append({"material_type": "MirrorMaterial", "kr": "mirror_kr"})
    added = []
    box = cfg["Aggregate"]["primitives"][1] if c.carrier != "slab" else None
    for m, prim, mname in zip(mats, (target, cube, box), ("m_case", "m_cube", "m_box")):
        if m is None: continue
        added.append({**m, "material_name": mname})
        prim["material_name"] = mname
    cfg["materials"] = copy.deepcopy(cfg["materials"]) + added
    return cfg, root


def refused_scene(wd, depth=6):
    """walls with the chain of `depth` levels as kd: depth 6 is one more than the device evaluates (kTexDepth) and is refused with RRT_EUNSUP at the first render"""
    return scene(wd, Case("graph", (f"depth_{depth}",), "walls", [cf("tint", 0.3)], chain(depth), [matte(kd=f"L{depth}")], "bar", "frame"))


# RRT_P_* of include/rrt.h, by the name the census tag uses
SLOTS = MS.TEX_SLOT


def census_problems(c, n):
    """What the census n (oracle_lib.tex_census of ONE oracle frame of case c) lacks of what c's tags promise; an empty list if nothing. Structure, not
    numbers: which counters are zero, which are not, which dominates. A share is of the calls the counter belongs to. The checkerboard shares (chk_filtered
    30 %, chk_half 50 %) are taken of the evaluations that get past aamode none, not of all 2D checkerboard evaluations: the same number wherever the
    graph's checkerboards are all closed-form, and the only meaningful one for chk-children, whose inner aamode-none checkerboard can reach no filter
    branch (of all its evaluations the filtered ones are 25 %)."""
    if isinstance(c, str): c = CASES[c]
    bad = []

    def need(cond, what):
        if not cond: bad.append(what)

    chk2 = n["node_checker2d"]
    nodes = sum(v for k, v in n.items() if k.startswith("node_"))
    with_aux = n["diff_calls"] - n["diff_no_aux"]
    closed = chk2 - n["chk_aa_none"]      # the 2D checkerboard evaluations that get past aamode none
    need(nodes > 1000, "a frame evaluates some thousand texture nodes")
    need(n["diff_not_finite"] == 0, "no case claims tx / ty not finite (module docstring)")
    for tag in c.tags:
        if tag == "chk_filtered": need(closed > 0 and n["chk_filtered"] >= 0.3 * closed, "the bump_int branch holds at least 30 % of the closed-form 2D checkerboard evaluations")
        elif tag == "chk_filtered_some": need(closed > 0 and n["chk_filtered"] >= 0.05 * closed, "the bump_int branch holds at least 5 % of the closed-form 2D checkerboard evaluations")
        elif tag == "chk_half": need(closed > 0 and n["chk_half"] >= 0.5 * closed, "the area2 = 0.5 shortcut holds at least 50 %")
        elif tag == "chk_closedform":
            need(n["chk_aa_none"] == 0, "closedform: no aamode-none return")
            need(n["chk_filtered"] + n["chk_half"] >= 0.05 * chk2 > 0, "at least 5 % of the evaluations pass the same-cell test")
        elif tag == "chk_none": need(n["chk_aa_none"] == chk2 > 0 and n["chk_filtered"] + n["chk_half"] + n["chk_same_cell"] == 0, "aamode none: every evaluation returns at once")
        elif tag == "chk_point":
            need(n["diff_no_aux"] > 0 and n["chk_same_cell"] >= 0.05 * chk2 > 0, "zero footprints: at least 5 % same-cell returns")
        elif tag == "chk_negative":
            need(n["chk_negative_sum"] >= 0.05 * chk2 > 0, "at least 5 % negative cell sums")
            if "chk_point" not in c.tags and c.carrier != "mirror" and n["chk_aa_none"] == 0:
                need(n["chk_bump_int_negative"] >= 0.05 * chk2, "bump_int of a negative argument in at least 5 % of the evaluations")
        elif tag == "round_seam":
            need(n["round_phi_wrapped"] >= 1, "phi < 0 wrapped")
            for k in ("fold_dx_high", "fold_dx_low", "fold_dy_high", "fold_dy_low"): need(n[k] >= 1, f"{k} at least once")
        elif tag == "round_fold":
            for k in ("fold_dx_high", "fold_dx_low", "fold_dy_high", "fold_dy_low"): need(n[k] >= 1, f"{k} at least once")
        elif tag == "round_pole": need(n["round_pole"] >= 1, "a call within 0.05 rad of a pole")
        elif tag == "noise_all_octaves": need(n["noise_all_octaves"] >= 0.05 * n["noise_sums"] > 0, "n == octaves in at least 5 % of the sums")
        elif tag == "noise_none": need(n["noise_n_int_0"] >= 0.05 * n["noise_sums"] > 0, "n_int == 0 in at least 5 % of the sums")
        elif tag == "noise_partial": need(n["noise_partial"] >= 0.05 * n["noise_sums"] > 0, "0 < n < octaves in at least 5 % of the sums")
        elif tag == "noise_negative": need(n["noise_negative_lattice"] >= 0.05 * n["noise_calls"] > 0, "a negative lattice coordinate in at least 5 % of the noise() calls")
        elif tag == "noise_saturated": need(n["noise_saturated"] >= 0.05 * n["noise_calls"] > 0, "a saturated cast in at least 5 % of the noise() calls")
        elif tag == "noise_windy": need(n["node_windy"] > 0 and n["noise_sums"] == 2 * n["node_windy"], "two fbm calls per Windy evaluation")
        elif tag == "chk3_negative": need(n["chk3_negative_sum"] >= 0.05 * n["node_checker3d"] > 0, "at least 5 % negative 3D cell sums")
        elif tag.startswith("depth_"): need(n["depth_max"] == int(tag[6:]), f"the deepest level reached is {tag[6:]}, not {n['depth_max']}")
        elif tag == "shared": need(n["node_uv"] == 2 * n["node_scale"] > 0 and n["node_mix"] == 2 * n["node_scale"], "the shared leaf is evaluated through both parents of every root")
        elif tag == "round_wrap": need(0.05 * n["round_calls"] <= n["round_phi_wrapped"] <= 0.95 * n["round_calls"], "phi < 0 wrapped in 5 % to 95 % of the sphere() calls")
        elif tag == "round_no_wrap": need(n["round_calls"] > 0 and n["round_phi_wrapped"] == 0, "cylinder() wraps no phi")
        elif tag.startswith("fb_"):
            need(n[tag] > 0, f"{tag} used")
            for k in n:
                if k.startswith("fb_") and k != tag and k not in c.tags: need(n[k] == 0, f"{k} must stay zero")
        elif tag == "mix_amount_textured": need(n["node_mix"] > 0 and n["fb_mix_amount"] == 0 and n["mix_amount_outside"] == 0, "the amount comes from a texture and stays in [0, 1]")
        elif tag == "amount_outside": need(n["mix_amount_outside"] >= 0.05 * n["node_mix"] > 0, "the amount leaves [0, 1] in at least 5 % of the Mix evaluations")
        elif tag == "negative_value": need(n["mat_negative_value"] >= 0.05 * with_aux, "a negative value reaches the material in at least 5 % of the hits")
        elif tag.startswith("node_"): need(n[tag] > 0, f"{tag} evaluated")
        elif tag.startswith("slots:"): pass      # checked on the loaded material (test_texture_shapes.py)
        elif tag == "tri_degenerate": need(n["tri_degenerate_uv"] >= 1, "a degenerate-uv face hit")
        elif tag == "tri_negative_det": need(n["tri_negative_det"] >= 1, "a mirrored face hit")
        elif tag == "tri_coord_dn": need(n["tri_coord_dn"] >= 1, "coordinate_system(dn) on a degenerate face with vertex normals")
        elif tag == "solve_failed": need(n["diff_solve_failed"] >= 1, "solve_2x2 refused")
        elif tag == "diff_axes":
            for k in ("diff_axis_yz", "diff_axis_xz", "diff_axis_xy"): need(n[k] >= 0.05 * with_aux, f"{k} holds at least 5 % of the hits with differentials")
        elif tag == "diff_axis_xy": need(n["diff_axis_xy"] >= 0.05 * with_aux, "diff_axis_xy holds at least 5 %")
        elif tag == "bump": need(n["bump_calls"] > 100 and n["bump_slope"] >= 0.5 * n["bump_calls"], "Material::bump runs, with a finite difference that is not 0 on at least half of its calls")
        elif tag == "bump_some": need(n["bump_calls"] > 100 and n["bump_slope"] >= 1, "Material::bump runs, with a finite difference that is not 0")
        elif tag == "bump_fallback_mixed":
            need(0.05 * n["bump_du_fallback"] <= n["bump_fallback_slope"] <= 0.95 * n["bump_du_fallback"], "on the du fallback the slope is 0 on some hits and not on others")
        elif tag == "bump_du_fallback": need(n["bump_du_fallback"] >= 1 and n["bump_dv_fallback"] >= 1, "the du == 0 and dv == 0 fallbacks")
        else: bad.append(f"unknown tag {tag}")
    return bad
