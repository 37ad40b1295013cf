"""Hand-built material tables for the device's BSDF code (dmath.hpp: build_lobes, Bsdf::f / pdf / sample_f, lobe_f / lobe_pdf / lobe_sample_f, the
Trowbridge-Reitz helpers, fr_dielectric, fr_conductor, roughness_to_alpha). Test infrastructure only.

A material is caller-supplied data, as a tree (tests/bvh_shapes.py), a lens table (tests/lens_shapes.py) and an image (tests/image_shapes.py) are. Every
other GPU test shades materials with all their lobes present and mid-range parameters; the table here walks the lobe sets with gaps (a Translucent whose
`reflect` is black fills slots 1 and 3 of the device's fixed lobe slots), the empty sets (a black Matte, Q31's Plastic with a black kd), the edges of the
parameters (roughness_to_alpha's clamp, alpha_x != alpha_y, alpha 0, sigma beyond its clamp, an index of 1 and below 1, a conductor with k = 0) and
materials whose lobe set is decided per hit by a checkerboard, each on a carrier where the case's branch is reached by many paths.

Carriers (64 x 64 films, built from rs_ray_toy_amd/scenes.py):
  walls   test_gpu_parity.py's tilted cfg3 (a matte cube inside a 12-triangle enclosure, both under generic rotations, one point light) with the material on
          the enclosure: the opaque cases
  slab    the same enclosure, and instead of the cube a thin box (scenes.write_box, half height 0.25) under its own generic rotation between the camera
          and the back wall, carrying the material: the camera's first hits land on it for more than a third of the rays that hit anything
          (slab_coverage(), asserted on the CPU: 79 %), and a path that enters it meets the far face from inside. Under DirectLighting a distant light
          shines from behind the slab as well: every point light of the reference sits at the origin (Q17), on the camera's side, where a transmissive
          lobe alone would leave the slab dark
  area    slab, lit by one of cfg5's sphere area lights instead of the point light: the MIS weight reads bsdf.pdf
  patch   walls with a curved 6 x 6 patch with smooth vertex normals carrying the material: real dpdu, which is what alpha_x != alpha_y needs. The
          reference's set_shading_geometry (interaction.rs:183-202) keeps the geometric normal's direction, so ns = +-ng here all the same
  bump    patch with a smooth bump map on the material: ns != ng (the general kernel, as for every textured material)
  field   cfg4's heightfield at n = 20 with its point lights: the Lambert and Glossy kernel classes and the horizon tables apply here
  field_cube   field with one of cfg2's plain matte cubes above the terrain: a terrain of an empty BSDF alone is a black frame

Constants are spelled as BilerpTextures with equal corners, which the loader folds: a constant material reaches the specialised kernels in fp32. A per-hit
parameter is a 2D CheckerBoardTexture (aamode none) over two constants.

A case is (material, carrier, integrator, tags, oracle, fp32, pair, per_hit). `tags` name counters of the oracle's BSDF census (oracle_lib.bsdf_census,
counted by the oracle and not by the code under test) that the case's frame must raise, "!name" one that must stay zero; census_problems() checks them and
test_material_shapes.py asserts it on the CPU for every case. `oracle` records what the reference's own arithmetic does with the case: "frame", or "panic"
where it asserts (alpha 0 makes D = 0 / 0 and path.rs:146 asserts on beta), or "drops" where DirectLighting drops the NaN samples at the film - recorded
from the oracle, never from the code under test. `fp32` is "bar" (test_transmissive_materials_path's fp32 bar), "panic", or
"f64_only: <finding>". `pair` names the case that is the same material by clamping.
"""
import collections
import copy
import os

import numpy as np

Case = collections.namedtuple("Case", "material carrier integrator tags oracle fp32 pair per_hit")

XRES = YRES = 64
PATH, DIRECT = "path", "direct"
BLACK = [0.0, 0.0, 0.0]
WHITE = [1.0, 1.0, 1.0]
# the slab: half extents and instance (tilted 35 degrees off the viewing direction, generic axis)
SLAB_HALF = (4.5, 0.25, 4.5)
SLAB_INSTANCE = {"world_pos": [21.0, 5.5, -9.5], "rotation_axis": [-0.55, 0.1, 0.75], "rotation_angle": 52.0}
SLAB_COVERAGE = 1.0 / 3.0
BACK_LIGHT = {"light_type": "distant", "l": {"values": [3.0, 2.5, 2.0]}, "scale": {"values": [1.5, 1.5, 1.5]}, "from": [50.0, -8.0, 12.0], "to": [21.0, 5.5, -9.5]}
PATCH_INSTANCE = {"world_pos": [26.0, -0.5, -5.0], "rotation_axis": [0.2, 1.0, 0.1], "rotation_angle": 20}
FIELD_N = 20
BUMP = {"v00": 0.0, "v01": 2.0}      # a displacement that rises by 2 over the patch's 14 units: a smooth tilt of the shading normal, no noise
CHECKER = {"mapping": "uv", "su": 9.0, "sv": 7.0, "du": 0.0, "dv": 0.0}

# Translucent lobe subsets by slot (0 LambertianReflection, 1 LambertianTransmission, 2 MicrofacetReflection, 3 MicrofacetTransmission; translucent.rs:50-107)
# as (kd, ks, reflect, transmit). Colours differ between the four parameters so that no two subsets give one frame.
_KD, _KS, _R, _T = [0.7, 0.5, 0.3], [0.4, 0.6, 0.8], [0.9, 0.8, 0.7], [0.6, 0.8, 0.9]
TRANSLUCENT_SUBSETS = {
    "s0": (_KD, BLACK, _R, BLACK), "s1": (_KD, BLACK, BLACK, _T), "s2": (BLACK, _KS, _R, BLACK), "s3": (BLACK, _KS, BLACK, _T),
    "s01": (_KD, BLACK, _R, _T), "s23": (BLACK, _KS, _R, _T), "s02": (_KD, _KS, _R, BLACK), "s13": (_KD, _KS, BLACK, _T),
    "s_none": (BLACK, BLACK, _R, _T), "s0123": (_KD, _KS, _R, _T),
}
SUBSET_SLOTS = {"s0": (0,), "s1": (1,), "s2": (2,), "s3": (3,), "s01": (0, 1), "s23": (2, 3), "s02": (0, 2), "s13": (1, 3), "s_none": (), "s0123": (0, 1, 2, 3)}
SLOT_LOBE = ("lobe_lambert", "lobe_lambert_trans", "lobe_microfacet", "lobe_microfacet_trans")
ALL_LOBES = ("lobe_lambert", "lobe_oren_nayar", "lobe_microfacet", "lobe_spec_refl", "lobe_spec_trans", "lobe_fresnel_spec", "lobe_lambert_trans",
             "lobe_microfacet_trans")


def _only(*lobes):
    """tags: these lobe kinds are added, no other kind is"""
    return tuple(lobes) + tuple("!" + k for k in ALL_LOBES if k not in lobes)


def _translucent(subset, remap=False, roughness=0.4):
    kd, ks, r, t = TRANSLUCENT_SUBSETS[subset]
    return ("TranslucentMaterial", {"kd": kd, "ks": ks, "reflect": r, "transmit": t}, {"roughness": roughness}, {"remap_roughness": True} if remap else {})


def _translucent_tags(subset, carrier, integrator):
    slots = SUBSET_SLOTS[subset]
    # (everything but `field` has plain matte surfaces beside the material: Lambertian lobes and one-lobe BSDFs are always there)
    tags = ["built_%d" % len(slots)] + [SLOT_LOBE[s] for s in slots] + ["!" + SLOT_LOBE[s] for s in range(4) if s not in slots and (s != 0 or carrier == "field")]
    if carrier in ("walls", "slab", "area"): tags += ["!lobe_oren_nayar", "!lobe_spec_refl", "!lobe_fresnel_spec", "!lobe_spec_trans"]
    if not slots: tags += ["sample_no_match"]
    if integrator == PATH:
        if len(slots) >= 1: tags += ["sample_comp0"]
        if len(slots) >= 2: tags += ["sample_comp1"]
        if len(slots) == 4: tags += ["sample_comp2", "sample_comp3"]
        if len(slots) < 4: tags += ["!sample_comp%d" % k for k in range(max(len(slots), 1), 4)]
        if len(slots) >= 2 and (1 in slots or 3 in slots): tags += ["sample_other_pdfs"]      # a transmissive lobe chosen among several (Q21)
        if len(slots) < 2 or not (1 in slots or 3 in slots): tags += ["!sample_other_pdfs"]
        if 3 in slots: tags += ["fr_swap"]
    return tuple(tags)


def _glass(kr=None, kt=None, eta=1.5, u=None, v=None, remap=False):
    rgbs, floats = {}, {"eta": eta}
    if kr is not None: rgbs["kr"] = kr
    if kt is not None: rgbs["kt"] = kt
    if u is not None: floats["u_roughness"] = u
    if v is not None: floats["v_roughness"] = v
    return ("GlassMaterial", rgbs, floats, {"remap_roughness": True} if remap else {})


def _metal(floats=None, rgbs=None, remap=False):
    return ("MetalMaterial", dict(rgbs or {}), dict(floats or {}), {"remap_roughness": True} if remap else {})


def _cases():
    out = {}

    def add(name, material, carrier, integrator, tags, oracle="frame", fp32="bar", pair=None, per_hit=None):
        assert name not in out, name
        out[name] = Case(material, carrier, integrator, tuple(tags), oracle, fp32, pair, per_hit)

    # ---- empty and one-lobe sets
    matte = lambda kd, sigma=None: ("MatteMaterial", {"kd": kd}, {} if sigma is None else {"sigma": sigma}, {})
    plastic = lambda kd, ks, rough=None, remap=False: ("PlasticMaterial", {"kd": kd, "ks": ks}, {} if rough is None else {"roughness": rough},
                                                       {"remap_roughness": True} if remap else {})
    # (the cube keeps its plain matte on `walls`: Lambertian lobes and one-lobe BSDFs are always there)
    add("matte_black-walls", matte(BLACK), "walls", PATH, ["built_0", "sample_no_match", "built_1", "!lobe_oren_nayar", "!lobe_microfacet"])
    add("matte_black-field", matte(BLACK), "field_cube", PATH, ["built_0", "sample_no_match", "built_1", "!built_2"] + list(_only("lobe_lambert")))
    add("matte_one_channel-walls", matte([0.6, 0.0, 0.0]), "walls", PATH, ["!built_0", "built_1"] + list(_only("lobe_lambert")))
    add("matte_negative-walls", matte([-1.0, 0.5, 0.2]), "walls", PATH, ["!built_0", "built_1"] + list(_only("lobe_lambert")))
    add("mirror_black-walls", ("MirrorMaterial", {"kr": BLACK}, {}, {}), "walls", PATH, ["built_0", "sample_no_match", "!lobe_spec_refl"])
    add("plastic_kd_black-walls", plastic(BLACK, [0.5, 0.5, 0.5]), "walls", PATH, ["built_0", "sample_no_match", "!built_2", "!lobe_microfacet"])
    add("plastic_kd_black-field", plastic(BLACK, [0.5, 0.5, 0.5]), "field_cube", PATH, ["built_0", "sample_no_match", "built_1", "!built_2"] + list(_only("lobe_lambert")))
    add("plastic_ks_black-walls", plastic([0.6, 0.5, 0.4], BLACK), "walls", PATH, ["built_2", "lobe_microfacet", "sample_comp0", "sample_comp1"])

    # ---- Oren-Nayar with a constant sigma
    for sigma, pair in ((20.0, None), (90.0, None), (200.0, "sigma90"), (-5.0, "sigma0")):
        tag = "sigma%g" % sigma
        for carrier in ("walls", "field"):
            lobes = ["lobe_lambert", "!lobe_oren_nayar", "!oren_max_cos"] if sigma < 0 else ["lobe_oren_nayar", "oren_max_cos"]
            if carrier == "field" and sigma > 0: lobes += ["!lobe_lambert"]
            add(f"matte_{tag}-{carrier}", matte([0.7, 0.6, 0.5], sigma), carrier, PATH, ["built_1", "!lobe_microfacet"] + lobes,
                pair=None if pair is None else f"matte_{pair}-{carrier}")
    for carrier in ("walls", "field"):      # the partner of sigma -5
        add(f"matte_sigma0-{carrier}", matte([0.7, 0.6, 0.5], 0.0), carrier, PATH, ["built_1", "lobe_lambert", "!lobe_oren_nayar", "!lobe_microfacet"])

    # ---- alpha
    micro = ["built_1", "lobe_microfacet", "sample_comp0"]
    # alpha 1e-4 (no remap): f64 only. tr_d reads tan^2 = (1 - wh.z^2) / wh.z^2 against alpha^2 = 1e-8, and fp32 resolves 1 - wh.z^2 in steps of 6e-8.
    # Worked out on the formula alone, with nothing but wh.z ROUNDED to fp32 and every operation exact: D moves by up to 600 % at theta_h = 1e-4, 12 % at
    # 1e-3, 1.3 % at 3e-3 and 0.1 % at 1e-2, where D is still 0.3 - so every path vertex whose half vector towards the light lies within a hundredth of a
    # radian of the normal carries an error beyond the bar's 1e-4, in any fp32 evaluation of the reference's formula. Measured: 98.51 % of the pixels
    # within 1e-4 where the bar asks 99 % (median 3.8e-8, largest 0.14); the f64 frame equals the oracle's to 2.2e-16, the specialised and the general
    # fp32 kernels agree to 4.5e-8, weights and query counters are exact. Roughness 1.0 and 2.0 and the remapped 1e-3 clamp (alpha 0.047) hold the bar.
    add("metal_rough1e-4-walls", _metal({"roughness": 1e-4}), "walls", PATH, micro + ["!alpha_clamp"],
        fp32="f64_only: D at alpha 1e-4 needs 1 - wh.z^2 to 1e-8, fp32 has 6e-8")
    add("metal_rough1-walls", _metal({"roughness": 1.0}), "walls", PATH, micro + ["!alpha_clamp", "micro_reject_hemi"])
    add("metal_rough2-walls", _metal({"roughness": 2.0}), "walls", PATH, micro + ["!alpha_clamp", "micro_reject_hemi"])
    add("metal_remap0-walls", _metal({"roughness": 0.0}, remap=True), "walls", PATH, micro + ["alpha_clamp"], pair="metal_remap1e-3-walls")
    add("metal_remap1e-3-walls", _metal({"roughness": 1e-3}, remap=True), "walls", PATH, micro + ["alpha_clamp"])
    add("metal_remap2-walls", _metal({"roughness": 2.0}, remap=True), "walls", PATH, micro + ["!alpha_clamp"])      # the polynomial above 1
    add("plastic_remap-walls", plastic([0.5, 0.4, 0.3], [0.5, 0.5, 0.5], 0.3, remap=True), "walls", PATH,
        ["built_2", "lobe_microfacet", "sample_comp0", "sample_comp1", "!alpha_clamp"])
    # (f_leak stays zero on the patch: set_shading_geometry, interaction.rs:183-202, keeps the geometric normal's direction and only faces it towards the
    # interpolated one, so ns = +-ng on a triangle and the patch's vertex normals reach the BSDF through ss / ts alone - which is what alpha_x != alpha_y reads)
    add("metal_aniso_uv-patch", _metal({"u_roughness": 0.02, "v_roughness": 0.5}), "patch", PATH, micro + ["!f_leak"])
    add("metal_aniso_vu-patch", _metal({"u_roughness": 0.5, "v_roughness": 0.02}), "patch", PATH, micro + ["!f_leak"])
    add("metal_k0-walls", _metal({"roughness": 0.2}, {"k": BLACK}), "walls", PATH, micro)
    # eta = 1, k = 0: F = 0 up to the rounding of fr_conductor's square roots (a few 1e-17, of either sign), so every f is black or as good as black. Under
    # the path integrator the reference asserts beta.y() > 0 on such an f wherever its sign comes out negative: DirectLighting, which only sums f
    add("metal_eta1_k0-walls", _metal({"roughness": 0.2}, {"eta": WHITE, "k": BLACK}), "walls", DIRECT, ["built_1", "lobe_microfacet", "direct_f_black"])
    # alpha 0: tr_d is 0 / 0 at the pole and 0 elsewhere, tr_sample_11 divides by zero - the reference asserts (recorded from the oracle, see the module docstring)
    add("metal_rough0-walls", _metal({"roughness": 0.0}), "walls", PATH, [], oracle="panic", fp32="panic")

    # ---- glass on the slab, under both integrators
    for integ in (PATH, DIRECT):
        p = integ == PATH
        smooth = ["lobe_fresnel_spec", "!lobe_spec_refl", "!lobe_spec_trans"] if p else ["!lobe_fresnel_spec"]
        add(f"glass_index1-{integ}", _glass([0.9, 0.9, 0.9], [0.8, 0.9, 1.0], 1.0), "slab", integ,
            smooth + (["fresnel_spec_transmit", "!fresnel_spec_reflect", "!fr_tir", "!refract_fail_specular"] if p else ["lobe_spec_refl", "lobe_spec_trans", "built_2", "!fr_tir"]))
        add(f"glass_index0.75-{integ}", _glass([0.9, 0.9, 0.9], [0.8, 0.9, 1.0], 0.75), "slab", integ,
            smooth + ["fr_tir"] + (["fresnel_spec_transmit", "fresnel_spec_reflect"] if p else ["refract_fail_specular", "built_2"]))
        add(f"glass_index2.4-{integ}", _glass([0.9, 0.9, 0.9], [0.8, 0.9, 1.0], 2.4), "slab", integ,
            smooth + ["fr_tir"] + (["fresnel_spec_transmit", "fresnel_spec_reflect"] if p else ["refract_fail_specular", "built_2"]))
        # (Path: FresnelSpecular carries both colours, one lobe either way. DirectLighting: the one-slot sets 0 and 1)
        # (index 2.4: F is 0.17 at normal incidence, so that under the path integrator most pixels have a sample that took the reflect branch - kt only and
        # both differ in nothing else)
        add(f"glass_kr_only-{integ}", _glass([0.9, 0.8, 0.7], BLACK,  2.4), "slab", integ,
            smooth + (["fresnel_spec_reflect", "fresnel_spec_transmit"] if p else ["lobe_spec_refl", "!lobe_spec_trans", "!built_2"]))
        add(f"glass_kt_only-{integ}", _glass(BLACK, [0.7, 0.8, 0.9],  2.4), "slab", integ,
            smooth + (["fresnel_spec_reflect", "fresnel_spec_transmit"] if p else ["!lobe_spec_refl", "lobe_spec_trans", "!built_2"]))
        add(f"glass_both-{integ}", _glass([0.9, 0.8, 0.7], [0.7, 0.8, 0.9],  2.4), "slab", integ,
            smooth + (["fresnel_spec_reflect", "fresnel_spec_transmit"] if p else ["lobe_spec_refl", "lobe_spec_trans", "built_2"]))
        rough = ["!lobe_fresnel_spec", "!lobe_spec_refl", "!lobe_spec_trans"]
        add(f"rough_glass_kr_only-{integ}", _glass([0.9, 0.8, 0.7], BLACK, 1.5, 0.3, 0.2), "slab", integ, rough + ["lobe_microfacet", "!lobe_microfacet_trans", "!built_2", "!alpha_clamp"])
        add(f"rough_glass_kt_only-{integ}", _glass(BLACK, [0.7, 0.8, 0.9], 1.5, 0.3, 0.2), "slab", integ,
            rough + ["!lobe_microfacet", "lobe_microfacet_trans", "!built_2", "!alpha_clamp"] + (["fr_swap"] if p else []))
        # u 0.3 / v 0 is not specular (glass.rs tests before it remaps); with the remap alpha_y comes from the 1e-3 clamp
        add(f"rough_glass_v0_remap-{integ}", _glass([0.9, 0.8, 0.7], [0.7, 0.8, 0.9], 1.5, 0.3, 0.0, remap=True), "slab", integ,
            rough + ["lobe_microfacet", "lobe_microfacet_trans", "built_2", "alpha_clamp"] + (["sample_comp0", "sample_comp1", "sample_other_pdfs"] if p else []))
        # ... and without it alpha_y = 0: D is 0 or 0 / 0 (recorded from the oracle: Path asserts on beta, DirectLighting drops the NaN samples at the film)
        add(f"rough_glass_v0-{integ}", _glass([0.9, 0.8, 0.7], [0.7, 0.8, 0.9], 1.5, 0.3, 0.0), "slab", integ, [] if p else rough + ["lobe_microfacet", "lobe_microfacet_trans"],
            oracle="panic" if p else "drops", fp32="panic" if p else "bar")

    # ---- Translucent lobe subsets on the slab, under both integrators
    for integ in (PATH, DIRECT):
        for subset in TRANSLUCENT_SUBSETS:
            remap = subset == "s0123"
            add(f"translucent_{subset}-{integ}", _translucent(subset, remap), "slab", integ, _translucent_tags(subset, "slab", integ) + (("!alpha_clamp",) if remap else ()))
    for subset in ("s13", "s02"):
        add(f"translucent_{subset}-area", _translucent(subset), "area", PATH, _translucent_tags(subset, "area", PATH))
    for subset in ("s0123", "s13"):
        add(f"translucent_{subset}-patch", _translucent(subset, subset == "s0123"), "patch", PATH, tuple(t for t in _translucent_tags(subset, "patch", PATH) if t != "!lobe_lambert") + ("!f_leak",))
    # the same two under a bump map (Material::bump, material/mod.rs:22-62, is NOT authoritative: ns really leaves ng): Bsdf::f chooses reflection or
    # transmission by ng and evaluates the lobes in the ns frame, and the light at the origin grazes the patch - the light-leak case
    for subset in ("s0123", "s13"):
        add(f"translucent_{subset}-bump", _translucent(subset, subset == "s0123"), "bump", PATH, tuple(t for t in _translucent_tags(subset, "patch", PATH) if t != "!lobe_lambert") + ("f_leak",))
    # ---- horizon: transmitted bounce rays leave below the surface
    for subset in ("s0123", "s13"):
        add(f"translucent_{subset}-field", _translucent(subset, subset == "s0123"), "field", PATH, _translucent_tags(subset, "field", PATH))

    # ---- lobe set decided per hit: a checkerboard over two constants drives one parameter (the general kernel; lanes of one wave disagree)
    add("per_hit_matte_kd-walls", matte(None), "walls", PATH, ["built_0", "built_1", "sample_no_match", "lobe_lambert"], per_hit={"kd": (BLACK, WHITE)})
    add("per_hit_plastic_kd-walls", plastic(None, [0.5, 0.5, 0.5]), "walls", PATH, ["built_0", "built_2", "sample_no_match", "lobe_microfacet"], per_hit={"kd": (BLACK, WHITE)})
    add("per_hit_translucent-slab", ("TranslucentMaterial", {"kd": _KD, "ks": _KS}, {"roughness": 0.4}, {}), "slab", PATH,
        ["built_2", "!built_4", "!built_0", "lobe_lambert", "lobe_lambert_trans", "lobe_microfacet", "lobe_microfacet_trans", "sample_other_pdfs"],
        per_hit={"reflect": (BLACK, WHITE), "transmit": (WHITE, BLACK)})
    add("per_hit_glass_kt-slab", _glass([0.9, 0.8, 0.7], None, 1.5), "slab", DIRECT, ["built_1", "built_2", "lobe_spec_refl", "lobe_spec_trans", "!lobe_fresnel_spec"],
        per_hit={"kt": (BLACK, WHITE)})
    return out


CASES = _cases()
# RRT_P_* of include/rrt.h: the slot of a material's tex[] that a textured parameter binds
TEX_SLOT = {"kd": 0, "ks": 1, "kr": 2, "eta": 3, "k": 4, "sigma": 5, "roughness": 6, "u_roughness": 7, "v_roughness": 8, "kt": 9, "reflect": 10, "transmit": 11,
            "index": 12}
MATERIAL_TYPE = {"MatteMaterial": 0, "PlasticMaterial": 1, "MetalMaterial": 2, "MirrorMaterial": 3, "GlassMaterial": 5, "TranslucentMaterial": 6}


def find(carrier=None, integrator=None, mtype=None, prefix=None, constant=None):
    """ids of the cases on this carrier / under this integrator / of this material type / whose name starts so / with constant parameters only"""
    return [k for k, c in CASES.items() if (carrier is None or c.carrier == carrier) and (integrator is None or c.integrator == integrator) and
            (mtype is None or c.material[0] == mtype) and (prefix is None or k.startswith(prefix)) and (constant is None or (c.per_hit is None) == constant)]


def expected_constants(c):
    """{rrt_material field: value} the loaded material must hold for the case (a Case or an id): the table's constants"""
    if isinstance(c, str): c = CASES[c]
    mtype, rgbs, floats, extra = c.material
    out = {k: list(v) for k, v in rgbs.items() if v is not None}
    for k, v in floats.items():
        if mtype == "GlassMaterial" and k == "eta": out["index"] = v
        elif mtype == "MetalMaterial" and k == "roughness": out.update(roughness=v, u_roughness=v, v_roughness=v)      # metal.rs:60-71
        else: out[k] = v
    out["remap_roughness"] = 1 if extra.get("remap_roughness") else 0
    return out


def _add_material(cfg, name, c):
    mtype, rgbs, floats, extra = c.material
    m = {"material_type": mtype, "material_name": name}
    for k, v in rgbs.items():
        if v is None: continue
        cfg["rgb_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"{name}_{k}", "v00": {"values": list(v)}, "v01": {"values": list(v)}})
        m[k] = f"{name}_{k}"
    for k, v in floats.items():
        cfg["float_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"{name}_{k}", "v00": v, "v01": v})
        m[k] = f"{name}_{k}"
    for k, (a, b) in (c.per_hit or {}).items():
        for tag, v in (("a", a), ("b", b)):
            cfg["rgb_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"{name}_{k}_{tag}", "v00": {"values": list(v)}, "v01": {"values": list(v)}})
        cfg["rgb_texture"].append({"texture_type": "CheckerBoardTexture", "texture_name": f"{name}_{k}", "aamode": "none", "t1": f"{name}_{k}_a", "t2": f"{name}_{k}_b",
                                   "mapping": dict(CHECKER)})
        m[k] = f"{name}_{k}"
    if c.carrier == "bump":
        cfg["float_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"{name}_bump", **BUMP})
        m["bump_map"] = f"{name}_bump"
    m.update(extra)
    cfg["materials"] = copy.deepcopy(cfg["materials"]) + [m]


def _enclosure(wd, nsamp, max_depth):
    """test_gpu_parity.py::_cfg3_tilted: generic rotations, no exact box / face ties"""
    from rs_ray_toy_amd import scenes
    cfg, root = scenes.cfg3(wd, xres=XRES, yres=YRES, nsamp=nsamp, max_depth=max_depth)
    cube, box = cfg["Aggregate"]["primitives"]
    cube["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
    box["instances"] = [{"world_pos": [0.0, 0.0, 0.0], "rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}]
    return cfg, root


def _slab(wd, cfg):
    """replaces the cube by the slab (written as slab.obj; box.obj is written again as the enclosure)"""
    from rs_ray_toy_amd import scenes
    scenes.write_box(wd, center=(0.0, 0.0, 0.0), half=SLAB_HALF)
    os.replace(os.path.join(wd, "box.obj"), os.path.join(wd, "slab.obj"))
    scenes.write_box(wd, center=(35.0, 0.0, 0.0), half=(40.0, 20.0, 40.0))
    cfg["objs"] = [o for o in cfg["objs"] if o["obj_name"] != "cube_01"] + [{"filename": "slab.obj", "obj_name": "slab_01"}]
    prims = cfg["Aggregate"]["primitives"]
    prims[0] = {"primitive_type": "triangle", "material_name": "m_case", "obj_name": "slab_01", "instances": [copy.deepcopy(SLAB_INSTANCE)]}


def scene(wd, name):
    """The frame of the module docstring for the case (a Case or an id); returns (cfg, root) for Scene.loads. The material under test is named m_case and
    is the last of the scene's materials."""
    from rs_ray_toy_amd import scenes
    from scene_util import write_patch
    c = CASES[name] if isinstance(name, str) else name
    if c.carrier in ("field", "field_cube"):
        cfg, root = scenes.cfg4(wd, xres=XRES, yres=YRES, nsamp=5, max_depth=6, n=FIELD_N)
        _add_material(cfg, "m_case", c)
        cfg["Aggregate"]["primitives"][0]["material_name"] = "m_case"
        if c.carrier == "field_cube":
            scenes.write_cube(wd)
            cfg["objs"] = cfg["objs"] + [{"filename": "cube.obj", "obj_name": "cube_01"}]
            cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "cube_01",
                                                   "instances": [{"world_pos": [35.2, 1.0, 2.8], "rotation_axis": [1.0, 2.0, 3.0], "rotation_angle": 15}]})
    else:
        cfg, root = _enclosure(wd, 9 if c.carrier in ("slab", "area") else 5, 7 if c.carrier in ("slab", "area") else 5)
        _add_material(cfg, "m_case", c)
        cube, box = cfg["Aggregate"]["primitives"]
        if c.carrier == "walls":
            box["material_name"] = "m_case"
        elif c.carrier in ("patch", "bump"):
            write_patch(wd)
            cfg["objs"] = cfg["objs"] + [{"filename": "patch.obj", "obj_name": "patch_01"}]
            cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "m_case", "obj_name": "patch_01", "instances": [copy.deepcopy(PATCH_INSTANCE)]})
        else:
            _slab(wd, cfg)
            if c.carrier == "area":      # one of scenes.cfg5's sphere area lights, brighter: the enclosure is larger than cfg5's terrain
                cfg["lights"] = [{"light_type": "diffuse", "spectrum": {"values": [4000, 4000, 4000]},
                                  "light_shape": {"shape_type": "sphere", "radius": 1.0, "world_pos": [30.0, 6.0, -5.0]}}]
    if c.integrator == DIRECT:
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": "all", "max_depth": 5}
        if c.carrier == "slab":      # every point light sits at the origin (Q17), on the camera's side of the slab: a distant light from behind it, for the transmissive lobes
            cfg["lights"] = cfg["lights"] + [dict(BACK_LIGHT)]
    return cfg, root


def slab_coverage(sc, O):
    """The share of the camera rays that hit anything whose first hit (the oracle's, O = oracle_lib) is on a primitive carrying the scene's last material"""
    W, H = sc.resolution
    nsamp = int(sc.desc.sampler.samples_per_pixel)
    _, rays, w = O.camera_samples(sc, (0, 0, W, H), 0, nsamp)
    live = w != 0
    hit = O.trace_closest(sc, rays[live, :3], rays[live, 3:], np.full(int(live.sum()), np.inf))
    found = hit["prim"] >= 0      # (an index into the BVH's primitive order)
    order = np.array([sc.desc.prim_order[i] for i in range(sc.desc.n_prim_order)])
    mats = np.array([sc.desc.prims[i].material for i in range(sc.desc.n_prims)])
    return float((mats[order[hit["prim"][found]]] == sc.desc.n_materials - 1).mean()), int(found.sum())


def census_problems(c, n):
    """What the census n (oracle_lib.bsdf_census of ONE oracle frame of case c) lacks of what c's tags promise; an empty list if nothing. Structure, not
    numbers: which counters are zero and which are not."""
    if isinstance(c, str): c = CASES[c]
    bad = []
    for tag in c.tags:
        if tag.startswith("!"):
            if n[tag[1:]] != 0: bad.append(f"{tag[1:]} must stay zero, is {n[tag[1:]]}")
        elif n[tag] == 0: bad.append(f"{tag} must be raised")
    if c.oracle != "panic" and n["built_0"] + n["built_1"] + n["built_2"] + n["built_4"] < 1000: bad.append("a frame builds some thousand BSDFs")
    return bad
