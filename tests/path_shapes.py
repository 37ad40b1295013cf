"""Hand-built path tables for the device's three integrator loops and the host code that drives them bounce by bounce (rrt_impl.hpp run_pass: the
`for (b < max_depth)` loop of k_shade_path with its queue swap, its two alternating shadow queues and the horizon cull; the k_shade_nee / k_shade_specular
chain of DirectLighting and Debug over opaque scenes; k_direct_tree's per-sample stack over transmissive ones). Test infrastructure only.

A path table is caller-supplied data, as a tree (tests/bvh_shapes.py), a lens table (tests/lens_shapes.py), an image (tests/image_shapes.py), a material
(tests/material_shapes.py), a texture graph (tests/texture_shapes.py) and a light table (tests/light_shapes.py) are. Every other Path test runs at max_depth
2 to 8 with rr_threshold 1 or 0, every other DirectLighting / Debug test at depth 1, 3, 5, 8 or 22; the table here walks max_depth from 0 to 64 (the
shadow-queue alternation's first states, the depths 5 | 6 where Russian roulette first reaches the film, the depths 16 | 17 | 18 around k_direct_tree's
first overflow frame), rr_threshold from -1 to 1e9 over walls that put q on its floor, kill nearly every path and separate max_component from y(),
glass that moves eta_scale both ways, and vertices that draw differently (specular only, black f, no lights, thirteen lights).

Films are 64 x 64, HaltonSampler nsamp 5 (4 samples per pixel) or 9. Carriers (built from rs_ray_toy_amd/scenes.py, as material_shapes.py's):
  walls   material_shapes._enclosure: test_gpu_parity.py's tilted cfg3 (a matte cube inside a 12-triangle enclosure, both under generic rotations, one point
          light at the origin) with the case's material on the enclosure: light_shapes.py's rough Plastic, or a Matte of the case's kd
  slab    the same enclosure with material_shapes.py's thin box instead of the cube, between the camera and the back wall, of smooth glass. Under
          DirectLighting and Debug (`walls` = "mirror": the glass hall) the walls are mirrors, a matte block stands behind the slab for the light to land
          on and material_shapes.BACK_LIGHT shines from behind it as well: in the plain enclosure the recursion ends at level 3 (a ray leaves the slab
          and meets a matte wall), the mirrors carry it to any max_depth, and the glass makes it k_direct_tree's
  field   cfg4's heightfield at n = 20 under the open sky with its three point lights: most bounce rays escape, the horizon tables apply
  hall    the enclosure as a mirror hall: its walls are MirrorMaterial, the cube is a mirror too (`cube` = "mirror") or matte; beside a matte cube stands a
          matte block in the far corner the camera looks into (the cube alone fills a sixtieth of the frame and catches none of a frame's first
          reflections), and under DirectLighting and Debug material_shapes.BACK_LIGHT shines as well

A case is (carrier, integrator, max_depth, rr, params, frame, tags, oracle, fp32). `rr` is the Path integrator's rr_threshold (None: the default 1). `params`
holds what the carrier takes: wall (a kd, or None for the Plastic), slab (an eta, or "matte"), cube, lights (a list replacing the carrier's). `frame` is how
the frame is rendered: nsamp, sampler ("halton" / "stratified": 2 x 2, dimension 4, jitter on), max_paths (the device option, for several pixel groups and
sample passes), rect. `tags` name what the oracle's path census (oracle_lib.path_census, counted by the oracle and not by the code under test) must show
for ONE frame of the case:
  name          the counter is raised at least TAG_MIN times          name>=N       at least N times (a rare event, or a maximum such as dim_max)
  !name         the counter stays zero                                name<=N       at most N
  cause@b       the end-cause histogram has TAG_MIN paths (or >=N) that ended by `cause` with bounces == b; li@d: li calls at reference depth d
  !cause@b      none
`oracle` records what the reference's own arithmetic does with the case: "frame" or "black" (every pixel exactly 0). `fp32` is "bar"
(test_material_shapes.py's fp32 bar) or "f64_only: <finding>", argued from the oracle alone.

REFUSALS are recorded, not rendered as frames: configurations that must fail, with the error the oracle gives (None: the reference renders them, the limit
is the device's own packing of a path's queue word) and the error the device must give.

What the reference does with the carriers, recorded from the oracle's census and not from the code under test:
  - a ray that starts on a face of the slab misses the opposite face more often than not (triangle.rs:167-205 takes E2 = p2 - p1), so in the
    plain enclosure a path that enters the glass leaves it a hundred times per frame and the recursive integrators end at level 3: hence the glass hall
  - a MatteMaterial with kd = 0 has no lobe at all, so its vertices draw no light sample before f.is_black() ends the path; the vertices that draw and then
    end on a black f are the Plastic's, a fifth of every frame on the `walls` carrier
  - under the default rr_threshold no path over the Plastic walls lives longer than 23 bounces, and on the terrain none reaches bounce 5: the frames of
    max_depth 40 and 64 there (9 and up on the terrain) are one frame, and the depths 17, 40 and 64 are live only on the bright walls without roulette
  - beyond `dimension` the StratifiedSampler hands out values of (-1, 1) (samplers/mod.rs:211-226), which ends two thirds of the paths over the walls at
    their first lobe sample; the mirror hall's paths need no sample and carry the 40 bounces
"""
import collections
import copy

import light_shapes as LS
import material_shapes as MS

Case = collections.namedtuple("Case", "carrier integrator max_depth rr params frame tags oracle fp32")

XRES = YRES = 64
PATH, ALL, ONE, DEBUG = "path", "all", "one", "debug"
TAG_MIN = 500
FIELD_N = MS.FIELD_N
# The walls' Plastic. Where its glossy lobe is negligible, a sample of the two-lobe BSDF multiplies beta by 2 kd (f = kd / pi against the average of the two
# pdfs), and after a survived roulette draw beta's largest component is 1: with light_shapes.py's kd of 0.5 a tenth of a frame's roulette tests then compare
# 1 +- 1e-7 with the default threshold of 1 (NEAR_PLASTIC, the case depth6_near-walls). This kd keeps the tests of every other case away from it.
PLASTIC = ("PlasticMaterial", {"kd": [0.45, 0.4, 0.3], "ks": [0.5, 0.5, 0.5]}, {"roughness": 0.3})
NEAR_PLASTIC = LS.ROUGH_PLASTIC
# the matte block of the glass hall: half extents and instance
BLOCK_HALF = (7.0, 5.0, 7.0)
BLOCK_INSTANCE = {"world_pos": [40.0, -6.0, 8.0], "rotation_axis": [1.0, 2.0, 3.0], "rotation_angle": 25.0}
# ... and of the mirror hall: in the far corner the camera looks into, where a fifth of the first reflections land on it
HALL_BLOCK_HALF = (5.0, 4.0, 5.0)
HALL_BLOCK_INSTANCE = {"world_pos": [62.0, -12.0, 22.0], "rotation_axis": [1.0, 2.0, 3.0], "rotation_angle": 25.0}
STRATIFIED = {"sampler_type": "StratifiedSampler", "xsamp": 2, "ysamp": 2, "jitter": True, "dimension": 4}
RECT = (5, 3, 53, 44)      # 48 x 41, origin and size off the 8 x 8 tile grid
GLASS_KR, GLASS_KT = [0.9, 0.9, 0.9], [0.8, 0.9, 1.0]      # material_shapes.py's glass_index* colours
PATH_DEPTHS = (0, 1, 2, 3, 4, 5, 6, 7, 9, 17, 40, 64)
DIRECT_DEPTHS = (0, 1, 2, 3, 4, 16, 17, 18, 40)
TREE_CAP = 18      # the glass tree's work grows with every level (two children per vertex inside the slab)
RR_DEPTH = 9
RR_THRESHOLDS = (("m1", -1.0), ("0", 0.0), ("1e-3", 1e-3), ("0.25", 0.25), ("1", None), ("1e9", 1e9))
# the threshold of the two eta_scale cases, chosen from the oracle's census: of 0.05 to 3 these have the most vertices whose test eta_scale decides (609 and 1 000
# of 11 000) with none within 2^-20 of the threshold - 0.5 has 800 of those, it is the enclosure's matte kd
ETA_THRESHOLD = {1.5: 0.3, 0.75: 0.6}


def _frame(nsamp=5, sampler="halton", max_paths=None, rect=None):
    return {"nsamp": nsamp, "sampler": sampler, "max_paths": max_paths, "rect": rect}


def _cases():
    out = {}

    def add(name, carrier, integrator, max_depth, tags, rr=None, oracle="frame", fp32="bar", frame=None, **params):
        assert name not in out, name
        out[name] = Case(carrier, integrator, max_depth, rr, params, frame or _frame(), tuple(tags), oracle, fp32)

    def depth_tags(d, rr_on=True):
        """what a Path frame of max_depth d over surfaces that mostly scatter must show"""
        if d == 0: return ["started", "depth@0>=5000", "!vertex_nee", "!rr_tests", "!end_escaped", "!end_roulette"]
        t = ["started", "vertex_nee", f"!depth@{min(d + 1, 65)}", "!end_pdf_zero"] + ([f"depth@{d}>=1"] if d <= 9 else ["roulette@9>=1"])
        t += ["!rr_tests", "!end_roulette"] if d <= 4 else ["rr_tests"]
        if d == 5 and rr_on: t += ["rr_draws", "roulette@4", "rr_survivors>=100", "!roulette@5"]
        if d >= 6 and rr_on: t += ["rr_draws", "roulette@4", "roulette@5>=50"]
        return t

    # ---- Path, depth: the enclosure with plastic walls, and the terrain under the open sky
    for d in PATH_DEPTHS:
        # (the Plastic's glossy lobe samples below the surface now and then: f.is_black() ends such a path after its light sample has drawn)
        add(f"depth{d}-walls", "walls", PATH, d, depth_tags(d) + (["!end_escaped", "black_f@0>=100"] if d else []), oracle="black" if d == 0 else "frame")
        # (the terrain: most bounce rays escape; the horizon cull answers them while bounces < max_depth)
        add(f"depth{d}-field", "field", PATH, d, [t for t in depth_tags(d) if not t.startswith(("rr_", "roulette@", f"depth@{d}"))] +
            (["end_escaped", "escaped@0", "escaped@1"] if d > 1 else ["end_escaped"] if d == 1 else []) + ([f"depth@{d}>=1"] if 0 < d <= 4 else []),
            oracle="black" if d == 0 else "frame")
    # depth 5 | 6 with roulette off: the partners of test_path_shapes.py's closed form (5: bit-equal to the default, 6: not)
    for d in (5, 6):
        add(f"depth{d}_rr0-walls", "walls", PATH, d, ["rr_tests", "!rr_draws", "!end_roulette", f"depth@{d}"], rr=0.0)
    # 64 bounces over bright walls without roulette: every path lives to the end and draws 7 dimensions per bounce, below the Halton sampler's 1 000
    # f64 only at 40 and 64 bounces, argued from the oracle alone: its two f64 evaluation orders of one frame (the reference's per-primitive ray transform
    # and the flattened instances, oracle_lib.render(flat=True)) differ by roundings of 2^-53 and nothing else, and after 40 (64) bounces that all survive they
    # are apart by more than 1e-4 x 2^-29 of the brightest pixel in 6.5 % (20 %) of the pixels, by up to 7.6e-10 (4.2e-8): a hit point's rounding error grows
    # with every bounce off the tilted walls and the cube. An fp32 rounding is 2^29 times as large, which puts those pixels beyond the bar's 1e-4 - more than
    # the 1 % the bar lets go. At 17 bounces it is 0.3 % of the pixels and the bar holds. test_f64_only_cases_are_argued asserts the oracle's side of this;
    # measured on the device: 93.7 % and 78.9 % of the pixels within 1e-4, medians 7.5e-7 and 3.5e-6.
    drift = "f64_only: after %d live bounces the oracle's own two f64 evaluation orders are 1e-4 x 2^-29 apart in more than 1 %% of the pixels"
    for d in (17, 40, 64):
        add(f"depth{d}_bright-walls", "walls", PATH, d, ["started", "vertex_nee", f"depth@{d}>=5000", "!rr_draws", "!end_roulette"] + (["dim_max>=440", "dim_max<=999"] if d == 64 else []),
            rr=0.0, wall=[0.95] * 3, fp32="bar" if d == 17 else drift % d)

    # ---- Path, roulette at max_depth 9
    for tag, thr in RR_THRESHOLDS:
        off = thr is not None and thr <= 0.0
        everyone = thr == 1e9
        # kd 0.95: rr_max stays above 0.95 for a bounce or two and q = max(1 - rr_max, 0.05) sits on its floor
        none = off or thr == 1e-3      # 0.95^9 = 0.63: beta never comes near 1e-3
        add(f"rr{tag}_bright-walls", "walls", PATH, RR_DEPTH, ["rr_tests"] + (["!rr_draws", "!end_roulette", "depth@9"] if none else ["rr_draws>=1"]) +
            (["rr_floor", "rr_draws", "rr_survivors", "depth@9"] if everyone else []) + (["rr_draws", "rr_survivors", "roulette@4"] if thr is None else []),
            rr=thr, wall=[0.95] * 3)
        # kd 0.05: beta is below 1e-5 at bounce 4, q is 1 to five digits and nearly every path dies there
        add(f"rr{tag}_dark-walls", "walls", PATH, RR_DEPTH, ["rr_tests"] + (["!rr_draws", "!end_roulette", "depth@9"] if off else ["rr_draws", "roulette@4", "rr_survivors<=50", "depth@9<=50", "!rr_floor"]),
            rr=thr, wall=[0.05] * 3)
        # kd (0.9, 0.1, 0.1): max_component is the red channel's, y() is a quarter of it
        add(f"rr{tag}_red-walls", "walls", PATH, RR_DEPTH, ["rr_tests"] + (["!rr_draws", "!end_roulette", "depth@9"] if none else ["rr_draws>=1"]) +
            (["rr_draws", "rr_survivors", "roulette@4", "depth@9>=100"] if thr is None or everyone else []), rr=thr, wall=[0.9, 0.1, 0.1])
    # glass in front of the camera: eta_scale leaves 1 both ways (entering multiplies it by eta^2, leaving divides), and at the chosen threshold some
    # vertices with bounces > 3 have their roulette test decided by it
    for eta in (1.5, 0.75):
        add(f"rr_eta{eta}-slab", "slab", PATH, RR_DEPTH, ["rr_tests", "rr_draws", "eta_enter", "eta_leave>=50", "rr_eta_decided>=100", "vertex_specular_only", "vertex_nee"],
            rr=ETA_THRESHOLD[eta], slab=eta, frame=_frame(nsamp=9))

    # ---- Path, vertices that draw differently
    # a mirror hall around one matte cube: a specular-only vertex skips next-event estimation and its five dimensions
    add("mirror_hall-path", "hall", PATH, RR_DEPTH, ["vertex_specular_only", "vertex_nee", "rr_tests", "depth@9"], cube="matte", frame=_frame(nsamp=9))
    # ... and around a mirror cube: nothing but specular vertices, a black frame whose paths all live to max_depth
    add("mirror_hall_all-path", "hall", PATH, 17, ["vertex_specular_only", "!vertex_nee", "!vertex_no_lights", "depth@17", "rr_tests"], cube="mirror", oracle="black")
    # kd 0 on the walls: MatteMaterial adds no lobe at all (matte.rs, material_shapes.py's matte_black), so num_components(non-specular) is 0, no light
    # sample is drawn and sample_f's black f ends the path two dimensions later - not after a light sample, as a black lobe would. (The vertices that do
    # draw and then end on a black f are the Plastic's, above.)
    add("matte_black-path", "walls", PATH, RR_DEPTH, ["vertex_specular_only", "vertex_nee>=100", "end_black_f", "black_f@0", "black_f@1>=50"], wall=[0.0] * 3)
    # no lights: n_lights == 0 skips the light draws. A black frame whose counters and weights still compare
    add("no_lights-path", "walls", PATH, RR_DEPTH, ["vertex_no_lights", "!vertex_nee", "rr_tests", "rr_draws", "roulette@4"], lights=[], oracle="black")
    # thirteen lights with roulette on: the light choice and the roulette draw are both live
    add("lights13-path", "walls", PATH, RR_DEPTH, ["vertex_nee", "rr_tests", "rr_draws", "roulette@4", "depth@9>=50"], lights=LS._distant_fan(13))

    # ---- DirectLighting `all` / `one` and Debug: the queue chain over the mirror hall, k_direct_tree over the glass slab
    for integ in (ALL, ONE, DEBUG):
        for d in DIRECT_DEPTHS:
            levels = max(1, d - 1)      # li recurses while depth + 1 < max_depth: reference depths 1 .. levels
            tags = ["li_calls", f"li@{levels}>=1", f"!li@{levels + 1}", f"level_max>={levels}", f"level_max<={levels}"]
            tags += ["reflect_taken", "recursion_refused>=1"] if d >= 3 else ["!reflect_taken", "!transmit_taken", "recursion_refused"]
            add(f"hall{d}-{integ}", "hall", integ, d, tags + ["!transmit_taken"], cube="matte")
            if d <= TREE_CAP:
                add(f"glass{d}-{integ}", "slab", integ, d, tags + (["transmit_taken"] if d >= 3 else []), slab=1.5, walls="mirror")
    # Debug without lights: k_shade_specular's grey_only path
    for d in (1, 3, 17):
        add(f"hall{d}_no_lights-debug", "hall", DEBUG, d, ["li_calls", f"li@{max(1, d - 1)}>=1"] + (["reflect_taken"] if d >= 3 else ["!reflect_taken"]), cube="matte", lights=[])

    # ---- across samplers and frame shapes
    # (beyond `dimension` the sampler hands out values of (-1, 1), samplers/mod.rs:211-226: half of the lobe samples land outside the unit disk and most
    # paths end on a black f at once. The mirror hall needs no sample to go on: without roulette every path there lives for 40 bounces)
    for d in (9, 40):
        add(f"stratified_depth{d}-walls", "walls", PATH, d, ["started", "vertex_nee", "black_f@0", "rr_tests>=10"], frame=_frame(sampler="stratified"))
    add("stratified_depth40-hall", "hall", PATH, 40, ["vertex_specular_only", "depth@40", "rr_tests"], rr=0.0, cube="matte", frame=_frame(sampler="stratified"))
    add("stratified_glass8-all", "slab", ALL, 8, ["li_calls", "reflect_taken", "transmit_taken", "li@7>=1", "!li@8"], slab=1.5, walls="mirror", frame=_frame(sampler="stratified"))
    # max_paths 1000: the 4 096 pixels go in five groups, one sample per pass
    add("small_pools_depth6-walls", "walls", PATH, 6, depth_tags(6), frame=_frame(max_paths=1000))
    add("small_pools_depth3-field", "field", PATH, 3, ["end_escaped", "depth@3>=1"], frame=_frame(max_paths=1000))
    add("small_pools_hall4-all", "hall", ALL, 4, ["li_calls", "reflect_taken", "li@3>=1", "!li@4"], cube="matte", frame=_frame(max_paths=1000))
    add("small_pools_glass17-debug", "slab", DEBUG, 17, ["li_calls", "transmit_taken", "li@16>=1", "!li@17"], slab=1.5, walls="mirror", frame=_frame(max_paths=1000))
    # a rect off the tile grid
    add("rect_depth9-walls", "walls", PATH, 9, ["vertex_nee", "rr_tests", "rr_draws"], frame=_frame(nsamp=9, rect=RECT))
    add("rect_depth2-field", "field", PATH, 2, ["end_escaped", "depth@2>=1"], frame=_frame(nsamp=9, rect=RECT))
    add("rect_glass17-one", "slab", ONE, 17, ["li_calls", "transmit_taken", "li@16>=1"], slab=1.5, walls="mirror", frame=_frame(rect=RECT))
    return out


CASES = _cases()
# Not a case of the table: roulette tests that compare 1 +- 1e-16 with the threshold 1 (NEAR_PLASTIC above). Such a test is a tie that any rounding decides, the
# f64 device's as much as an fp32 one's (4 pixels of its f64 frame leave the oracle's by 3e-3), so no frame of it is held to the oracle; it stands here for
# the census's rr_test_near counter, which test_path_shapes.py shows to be 0 for every case of the table and not 0 for this one.
NEAR_CASE = Case("walls", PATH, 6, None, {"wall": "near"}, _frame(), ("rr_draws", "roulette@5>=50", "rr_test_near>=100"), "frame", "none")

Refusal = collections.namedtuple("Refusal", "integrator max_depth sampler oracle device device_match")
REFUSALS = {
    # the bounce count rides in 8 bits of a path's queue word under the StratifiedSampler (dmath.hpp db_pack): the reference has no such limit
    "stratified_depth256": Refusal(PATH, 256, "stratified", None, "RrtUnsupported", "max_depth above 255"),
    # 3 * 1364 + 4 = 4096 two-dimensional draws would pass the 12-bit dimension counters
    "stratified_counters": Refusal(PATH, 1364, "stratified", None, "RrtUnsupported", "dimension counters are 12 bits"),
    # 5 camera dimensions and 7 per bounce: bounce 143 would draw dimension 1 000 (halton.rs:63-69). test_gpu_parity.py's
    # test_halton_dimension_limit_panics_like_the_reference holds the device to it at depth 400; here it is the first depth that can get there
    "halton_depth143": Refusal(PATH, 143, "halton", "1000 dimensions", "RrtPanic", "1000 dimensions"),
}


def find(prefix=None, integrator=None, carrier=None):
    return [k for k, c in CASES.items() if (prefix is None or k.startswith(prefix)) and (integrator is None or c.integrator == integrator) and (carrier is None or c.carrier == carrier)]


def _material(cfg, name, material):
    """material_shapes.py's way of spelling a material with constant parameters"""
    MS._add_material(cfg, name, MS.Case(tuple(material) + ({},) * (4 - len(material)), "walls", None, (), None, None, None, None))


def _block(wd, cfg, half=BLOCK_HALF, instance=BLOCK_INSTANCE):
    """adds the matte block (written as block.obj; box.obj is written again as the enclosure, as material_shapes._slab does)"""
    import os
    from rs_ray_toy_amd import scenes
    scenes.write_box(wd, center=(0.0, 0.0, 0.0), half=half)
    os.replace(os.path.join(wd, "box.obj"), os.path.join(wd, "block.obj"))
    scenes.write_box(wd, center=(35.0, 0.0, 0.0), half=(40.0, 20.0, 40.0))
    cfg["objs"] = cfg["objs"] + [{"filename": "block.obj", "obj_name": "block_01"}]
    cfg["Aggregate"]["primitives"].append({"primitive_type": "triangle", "material_name": "mat_matte", "obj_name": "block_01", "instances": [copy.deepcopy(instance)]})


def _integrator(cfg, integrator, max_depth, rr):
    if integrator == PATH:
        cfg["Integrator"] = {"integrator_type": "Path", "max_depth": max_depth}
        if rr is not None: cfg["Integrator"]["rr_threshold"] = rr
    elif integrator == DEBUG: cfg["Integrator"] = {"integrator_type": "Debug", "max_depth": max_depth}
    else: cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": integrator, "max_depth": max_depth}


def scene(wd, name):
    """The frame of the module docstring for the case (a Case or an id); returns (cfg, root) for Scene.loads."""
    from rs_ray_toy_amd import scenes
    c = CASES[name] if isinstance(name, str) else name
    p = c.params
    if c.carrier == "field":
        cfg, root = scenes.cfg4(wd, xres=XRES, yres=YRES, nsamp=c.frame["nsamp"], max_depth=c.max_depth, n=FIELD_N)
    else:
        cfg, root = MS._enclosure(wd, c.frame["nsamp"], c.max_depth)
        cube, box = cfg["Aggregate"]["primitives"]
        if c.carrier == "walls":
            wall = p.get("wall")
            _material(cfg, "m_wall", PLASTIC if wall is None else NEAR_PLASTIC if wall == "near" else ("MatteMaterial", {"kd": list(wall)}, {}))
            box["material_name"] = "m_wall"
        elif c.carrier == "slab":
            slab = p["slab"]
            _material(cfg, "m_case", ("MatteMaterial", {"kd": [0.6, 0.5, 0.4]}, {}) if slab == "matte" else ("GlassMaterial", {"kr": GLASS_KR, "kt": GLASS_KT}, {"eta": slab}))
            MS._slab(wd, cfg)
            if p.get("walls") == "mirror":      # the glass hall: mirror walls, and a matte block for the light to land on
                box["material_name"] = "mat_mirror"
                _block(wd, cfg)
            if c.integrator != PATH: cfg["lights"] = cfg["lights"] + [dict(MS.BACK_LIGHT)]
        else:
            box["material_name"] = "mat_mirror"
            cube["material_name"] = "mat_mirror" if p["cube"] == "mirror" else "mat_matte"
            if p["cube"] == "matte": _block(wd, cfg, HALL_BLOCK_HALF, HALL_BLOCK_INSTANCE)
            if c.integrator != PATH: cfg["lights"] = cfg["lights"] + [dict(MS.BACK_LIGHT)]      # (the first reflections see the block from behind)
    if "lights" in p: cfg["lights"] = copy.deepcopy(p["lights"])
    _integrator(cfg, c.integrator, c.max_depth, c.rr)
    if c.frame["sampler"] == "stratified": cfg["Sampler"] = dict(STRATIFIED)
    return cfg, root


def refusal_scene(wd, name):
    """A 16 x 16 film of the enclosure with white walls and no roulette, under the refusal's sampler and depth"""
    r = REFUSALS[name]
    c = Case("walls", r.integrator, r.max_depth, 0.0, {"wall": [0.99] * 3}, _frame(nsamp=3, sampler=r.sampler), (), None, None)
    cfg, root = scene(wd, c)
    cfg["Film"]["xres"] = cfg["Film"]["yres"] = 16
    return cfg, root


def _value(n, key):
    if "@" in key:
        what, b = key.split("@")
        return (n["li_depth"] if what == "li" else n["ends"][what])[int(b)]
    return n[key] if key in n else n["end_" + key]


def census_problems(c, n):
    """What the census n (oracle_lib.path_census of ONE oracle frame of case c) lacks of what c's tags promise; an empty list if nothing."""
    if isinstance(c, str): c = CASES[c]
    bad = []
    for tag in c.tags:
        if tag.startswith("!"):
            if _value(n, tag[1:]) != 0: bad.append(f"{tag[1:]} must stay zero, is {_value(n, tag[1:])}")
        elif "<=" in tag:
            key, lim = tag.split("<=")
            if _value(n, key) > int(lim): bad.append(f"{key} must stay within {lim}, is {_value(n, key)}")
        else:
            key, lim = tag.split(">=") if ">=" in tag else (tag, TAG_MIN)
            if _value(n, key) < int(lim): bad.append(f"{key} must be raised {lim} times, is {_value(n, key)}")
    if c.integrator == PATH:
        ends = sum(n["end_" + k] for k in ("escaped", "depth", "black_f", "pdf_zero", "roulette"))
        if ends != n["started"]: bad.append(f"ends by cause sum to {ends}, {n['started']} paths started")
        if n["li_calls"]: bad.append("a Path frame makes no li call of the recursive integrators")
    elif n["started"]: bad.append("a DirectLighting / Debug frame starts no path")
    return bad
