"""Hand-built light tables for the device's direct-lighting code (dkernels.hpp: light_sample_li, estimate_direct_light, sample_light_discrete and the
`v * n_lights` choice of DirectLighting `one`; host/scene_loader.cpp make_light, host/scene_flatten.cpp's Light<R> records and light cdf,
host/shadow_lists.cpp's sources). Test infrastructure only.

A light table is caller-supplied data, as a tree (tests/bvh_shapes.py), a lens table (tests/lens_shapes.py), an image (tests/image_shapes.py), a material
(tests/material_shapes.py) and a texture graph (tests/texture_shapes.py) are. Every other GPU test lights its scene with 1 to 4 point, distant or unit
sphere lights above the geometry; the table here walks the three light kinds through triangle emitters (never built anywhere else), the light counts up
to and beyond the 15 sources of the shadow candidate lists, every early out of estimate_direct, and sphere emitters that are scaled, clipped, turned
inside out, far away or around the geometry.

Films are 64 x 64 at 4 samples per pixel, depth 3. Lights are not geometry (Q18: no primitive carries an area light), so no carrier has a sphere
primitive and fp32 stays free of the sphere self-hit coin. Carriers (built from rs_ray_toy_amd/scenes.py, as material_shapes.py's):
  walls   test_gpu_parity.py's tilted cfg3 (a cube inside a 12-triangle enclosure, both under generic rotations) with a rough Plastic on the cube: the
          MIS weight of an area light reads a non-Lambertian bsdf.pdf there. A shadow ray is one unit long (Ray::new normalises d and keeps
          t_max = 1 - SHADOW_EPSILON, Q9), so the enclosure shuts no light out: distant lights and emitters beyond the walls light it, and only the
          cube and the corners occlude
  field   cfg4's heightfield at n = 20: world-space triangles only, which is what the shadow candidate lists need (host/shadow_lists.cpp)

Every point light of the reference sits at the world origin (Q17), which is inside the enclosure and beside the terrain.

A triangle emitter is a face of an OBJ mesh named by `obj_name` / `tri_num`; its vertices are the file's, no instance moves them. scene() writes the
file a light's "_obj" entry holds into the work directory. Triangle::sample takes its "barycentrics" from a point b of the unit SPHERE (Q19): the sampled
point is b.x q0 + b.y q1 + b.z q2, on an ellipsoid around the world origin and not on the triangle, and with vertex normals ns = sum b_k n_k changes
sign with b - faceforward turns the emitter round for half of the samples whichever way the file's normals point.

A case is (lights, carrier, integrator, tags, oracle, fp32, pair). `tags` name counters of the oracle's light census (oracle_lib.light_census, counted by
the oracle and not by the code under test) that the case's frame must raise at least TAG_MIN times, "!name" one that must stay zero; census_problems()
checks them, and that every light index was chosen, and test_light_shapes.py asserts it on the CPU for every case. `oracle` records what the reference's
own arithmetic does with the case: "frame", "black" (every pixel exactly 0), "drops" (NaN samples dropped at the film, integrator/mod.rs:105) or "panic" -
recorded from the oracle, never from the code under test. Every case of the table came out as "frame" or "black": Vector3::normalize (geometry.rs:925) leaves a
zero vector as it is, so neither `from == to` nor a zero-area emitter puts a NaN anywhere. `fp32` is "bar" (test_gpu_parity.py's fp32 bar) or "f64_only: <finding>". `pair` names the
case that is the same light table spelled differently.
"""
import collections
import copy
import os

import numpy as np

Case = collections.namedtuple("Case", "lights carrier integrator tags oracle fp32 pair")

XRES = YRES = 64
NSAMP, DEPTH = 5, 3      # (HaltonSampler nsamp 5: 4 samples per pixel)
PATH, ALL, ONE = "path", "all", "one"
TAG_MIN = 500
FIELD_N = 20
ROUGH_PLASTIC = ("PlasticMaterial", {"kd": [0.5, 0.4, 0.3], "ks": [0.5, 0.5, 0.5]}, {"roughness": 0.3})
POINT, DIFFUSE, DISTANT = 0, 1, 2      # RRT_LIGHT_* of include/rrt.h
TRIANGLE, SPHERE = 0, 1                # RRT_PRIM_*
FLOOR_TILT = {"rotation_axis": [3.0, 1.0, 2.0], "rotation_angle": 7}      # _enclosure()'s instance of the box


def _rotate(v, axis, angle_deg):
    """Rodrigues' rotation of v about axis (transform.rs rotate(): counter-clockwise seen against the axis)"""
    v, a = np.asarray(v, np.float64), np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(angle_deg)
    return v * np.cos(t) + np.cross(a, v) * np.sin(t) + a * np.dot(a, v) * (1.0 - np.cos(t))


def point(spectrum=(60000.0, 60000.0, 60000.0)):
    return {"light_type": "point", "spectrum": {"values": list(spectrum)}}


def distant(frm, to=(0.0, 0.0, 0.0), l=(3.0, 2.5, 2.0), **extra):
    return {"light_type": "distant", "l": {"values": list(l)}, "from": list(frm), "to": list(to), **extra}


def sphere(pos=(30.0, 6.0, -5.0), radius=1.0, spectrum=(4000.0, 4000.0, 4000.0), **shape):
    return {"light_type": "diffuse", "spectrum": {"values": list(spectrum)}, "light_shape": {"shape_type": "sphere", "radius": radius, "world_pos": list(pos), **shape}}


def tri_obj(verts, faces, normals=None, face_normals=None):
    """OBJ text: `v` lines, `vn` lines if normals is given, `f a b c` faces, or `f a//n b//n c//n` where face_normals gives each face's normal indices"""
    lines = ["v %r %r %r" % tuple(float(x) for x in v) for v in verts]
    lines += ["vn %r %r %r" % tuple(float(x) for x in n) for n in (normals or [])]
    for k, f in enumerate(faces):
        if face_normals is None: lines.append("f %d %d %d" % tuple(i + 1 for i in f))
        else: lines.append("f " + " ".join("%d//%d" % (i + 1, j + 1) for i, j in zip(f, face_normals[k])))
    return "\n".join(lines) + "\n"


def triangle(obj_text, tri_num=0, spectrum=(20000.0, 20000.0, 20000.0)):
    """A DiffuseAreaLight on face tri_num of the mesh obj_text describes"""
    return {"light_type": "diffuse", "spectrum": {"values": list(spectrum)}, "light_shape": {"shape_type": "triangle", "tri_num": tri_num}, "_obj": obj_text}


# The plain triangle emitter: the sampled points b.x q0 + b.y q1 + b.z q2 range over an ellipsoid with half axes of some 50, 9 and 7 units around the
# origin, about half of it inside the enclosure. Its geometric normal is (0.11, -0.99, -0.06): the emitter faces down.
TRI = [(30.0, 12.0, -6.0), (40.0, 13.0, -4.0), (36.0, 12.0, 6.0)]
TRI_N = np.cross(np.subtract(TRI[1], TRI[0]), np.subtract(TRI[2], TRI[0]))
TRI_N = TRI_N / np.linalg.norm(TRI_N)
# ... vertex normals that are not parallel: within 30 degrees of the geometric normal
TRI_VN = [TRI_N + 0.3 * np.array(d) for d in ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, -1.0))]
# near the origin: the ellipsoid has half axes below 2 units and stays inside the enclosure, 5 units from its nearest wall; far from it: q0 ~ q1 ~ q2 = c,
# so the sampled point is (b.x + b.y + b.z) c + O(1): a needle through the origin that reaches 1.7 |c| = 120 units out, most of it beyond the walls
TRI_NEAR = [(1.0, 0.5, 0.0), (0.0, 1.2, 0.8), (-0.5, 0.3, -1.0)]
TRI_FAR = [(60.0, 14.0, 30.0), (61.0, 14.0, 30.5), (60.5, 15.0, 29.0)]
TRI_DEGENERATE = [(30.0, 12.0, -6.0), (33.0, 12.0, 0.0), (36.0, 12.0, 6.0)]      # collinear: cross = 0 exactly


def _box_obj(center=(30.0, 10.0, -4.0), half=(3.0, 1.0, 2.0)):
    """scenes.write_box's 12-triangle box as OBJ text"""
    order = [(1, 1, -1), (1, -1, -1), (1, 1, 1), (1, -1, 1), (-1, 1, -1), (-1, -1, -1), (-1, 1, 1), (-1, -1, 1)]
    faces = [(5, 3, 1), (3, 8, 4), (7, 6, 8), (2, 8, 6), (1, 4, 2), (5, 2, 6), (5, 7, 3), (3, 7, 8), (7, 5, 6), (2, 4, 8), (1, 3, 4), (5, 1, 2)]
    verts = [tuple(c + s * h for c, s, h in zip(center, sg, half)) for sg in order]
    return tri_obj(verts, [(a - 1, c - 1, b - 1) for a, b, c in faces])


def _distant_fan(n):
    """n distinct distant lights from the upper hemisphere (a golden-angle spiral between 25 and 80 degrees of elevation), each of its own colour, n in all as bright as three"""
    out = []
    for k in range(n):
        el, az = np.radians(25.0 + 55.0 * (k + 0.5) / n), 2.399963 * k
        g = 3.0 / n
        out.append(distant((np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)), l=(g * (2.0 + (k % 3)), g * (2.0 + ((k + 1) % 3)), g * (2.0 + ((k + 2) % 3)))))
    return out


def _cases():
    out = {}

    def add(name, lights, carrier, tags=(), oracle="frame", fp32="bar", pair=None, direct=False, oracle_by=None):
        for integ in (PATH, ALL, ONE) if direct else (PATH,):
            assert f"{name}-{integ}" not in out, name
            t = list(tags) + (["choose_distrib", "!choose_plain"] if integ == PATH else ["!choose_distrib", "choose_plain"] if integ == ONE else ["!choose_distrib", "!choose_plain"])
            out[f"{name}-{integ}"] = Case(lights, carrier, integ, tuple(t), (oracle_by or {}).get(integ, oracle), fp32, None if pair is None else f"{pair}-{integ}")

    only = lambda *kinds: list(kinds) + ["!" + k for k in ("point", "distant", "sphere_emitter", "tri_emitter") if k not in kinds]
    # ---- delta lights
    # the point.rs branch: li = I / d^2, pdf 1, no MIS
    add("point", [point()], "walls", only("point") + ["unoccluded", "!li_black", "!pdf_zero"], direct=True)
    # a black spectrum: li.is_black() returns before bsdf.f is evaluated and before any shadow ray
    add("point_black", [point((0.0, 0.0, 0.0))], "walls", only("point") + ["li_black", "!unoccluded", "!occluded", "!f_black"], oracle="black")
    # distant.rs with `scale` (a spectrum: l * scale) and a rotation on the light (w = normalize(light_to_world(from - to)))
    add("distant_scaled_rotated", [distant((20.0, 30.0, 10.0), (35.0, 0.0, 0.0), scale={"values": [1.5, 0.5, 2.0]}, rotation_axis=[1.0, 2.0, 3.0], rotation_angle=25.0)],
        "walls", only("distant") + ["unoccluded"], direct=True)
    # w within half a degree of the floor's plane: |cos| at the floor is below 0.009, the walls are lit at full strength
    add("distant_grazing", [distant(_rotate(_rotate((1.0, 0.0, 0.3), (0.0, 0.0, 1.0), 0.4), FLOOR_TILT["rotation_axis"], FLOOR_TILT["rotation_angle"]))], "walls",
        only("distant") + ["unoccluded"])
    # from == to: Vector3::normalize (geometry.rs:925) leaves a zero vector as it is, so w = wi = 0, cos = 0 and f is black: no NaN, a black frame
    add("distant_from_eq_to", [distant((3.0, 4.0, 5.0), (3.0, 4.0, 5.0))], "walls", only("distant") + ["f_black", "!unoccluded", "!occluded"], oracle="black")
    # duplicates: one source, one candidate table (shadow_lists.cpp:59), two entries of the cdf
    add("two_equal_points", [point((30000.0, 30000.0, 30000.0)), point((30000.0, 30000.0, 30000.0))], "field", only("point") + ["unoccluded", "occluded"], direct=True)
    # ---- counts: sample_light_discrete / v * n_lights among n lights, the fp32 cdf, the 15 sources of the candidate lists
    # (13 is the base of the Halton dimension that chooses the light at the first vertex: the radical inverse has the cdf's own denominator)
    for n in (2, 3, 5, 13, 15, 16, 17):
        add(f"count_{n}", _distant_fan(n), "field", only("distant") + ["unoccluded"], direct=True)
    add("count_3_mixed", [point((30000.0, 20000.0, 10000.0))] + _distant_fan(2), "field", only("point", "distant") + ["unoccluded"], direct=True)
    # ---- triangle emitters (the L.shape_type != 1 branch of light_sample_li, Q19)
    tri = only("tri_emitter") + ["unoccluded", "emitter_backface"]
    no_n = ["!tri_normals_kept", "!tri_normals_flipped", "!tri_normals_mode2"]
    # (the emitter faces down and most of its sampled points are above the first hits: few samples show their back at the first vertex)
    add("tri_plain", [triangle(tri_obj(TRI, [(0, 1, 2)]))], "walls", [t for t in tri if t != "emitter_backface"] + no_n, direct=True)
    # (ns = sum b_k n_k changes sign with b: both branches of faceforward whichever way the normals point)
    add("tri_normals_agree", [triangle(tri_obj(TRI, [(0, 1, 2)], TRI_VN, [(0, 1, 2)]))], "walls", tri + ["tri_normals_kept", "tri_normals_flipped", "!tri_normals_mode2"], direct=True)
    add("tri_normals_flipped", [triangle(tri_obj(TRI, [(0, 1, 2)], [-n for n in TRI_VN], [(0, 1, 2)]))], "walls",
        tri + ["tri_normals_kept", "tri_normals_flipped", "!tri_normals_mode2"], direct=True)
    # `vn` lines and faces without normal indices: mesh_has_n = 2, Triangle::new's n = [0, 0, 0] - the FIRST normal of the mesh three times
    add("tri_normals_mode2", [triangle(tri_obj(TRI, [(0, 1, 2)], [-n for n in TRI_VN]))], "walls", tri + ["tri_normals_mode2", "tri_normals_kept", "tri_normals_flipped"])
    # the last face of a mesh of 12: first_tri + tri_num reaches the mesh's end and not past it
    add("tri_last_of_mesh", [triangle(_box_obj(), 11)], "walls", tri + no_n)
    add("tri_near_origin", [triangle(tri_obj(TRI_NEAR, [(0, 1, 2)]), spectrum=(60000.0, 60000.0, 60000.0))], "walls", tri + no_n)
    add("tri_far_from_origin", [triangle(tri_obj(TRI_FAR, [(0, 1, 2)]))], "walls", tri + no_n)
    # zero area: the cross product is 0 and Vector3::normalize leaves it, |dot(-wi, n)| = 0, pdf = d^2 / 0 = inf, which Shape::sample_ref turns into 0
    add("tri_degenerate", [triangle(tri_obj(TRI_DEGENERATE, [(0, 1, 2)]))], "walls", only("tri_emitter") + no_n + ["pdf_zero", "!unoccluded", "!occluded", "!li_black", "!pdf_not_positive"],
        oracle="black")
    # ---- sphere emitters
    sph = only("sphere_emitter") + ["unoccluded", "emitter_backface"]
    add("sphere_plain", [sphere()], "walls", sph, direct=True)
    # a non-uniform scale under a rotation: n comes from aff_nrm (the inverse transpose); the lists bound the emitter by the Frobenius stretch
    add("sphere_scaled_rotated", [sphere(scale=[0.5, 2.0, 1.0], rotation_axis=[1.0, 2.0, 3.0], rotation_angle=40.0)], "walls", sph, direct=True)
    # z_min / z_max / phi_max change `area` alone, and light_sample_li overwrites the pdf that read it: Sphere::sample ignores the clip
    add("sphere_clipped", [sphere(z_min=-0.3, z_max=0.6, phi_max=200.0)], "walls", sph, pair="sphere_plain")
    # radius < 0: p_obj = radius * u is scaled by radius / |p_obj| < 0 - the point lands opposite, and its normal points inwards
    add("sphere_negative_radius", [sphere(radius=-1.0)], "walls", sph)
    # the floor below the cube is inside the emitter (radius 15 around a point of the floor): from inside every sample shows its back
    add("sphere_swallows_floor", [sphere(pos=(35.0, -20.0, 0.0), radius=15.0)], "walls", sph)
    # below the floor and outside the enclosure: at the floor wi is below the horizon and f is black; the walls see the emitter (Q9)
    add("sphere_below_floor", [sphere(pos=(35.0, -30.0, 0.0), radius=2.0)], "walls", only("sphere_emitter") + ["f_black", "unoccluded"])
    # radius 1e-3 at 1e4: in fp32 p has an ulp of 1e-3, the whole emitter is one or two values of p; p - ref_p cancels nothing that matters (|p - ref| ~ 1e4)
    add("sphere_far_tiny", [sphere(pos=(6.0e3, 7.0e3, -4.0e3), radius=1.0e-3, spectrum=(3.0e8, 3.0e8, 3.0e8))], "walls", sph)
    # ---- mixed tables: the AREA = true kernels with delta lights passing through them
    add("mixed_all_four", [point((30000.0, 30000.0, 30000.0)), distant((20.0, 30.0, 10.0), (35.0, 0.0, 0.0)), sphere(spectrum=(2000.0, 2000.0, 2000.0)),
                           triangle(tri_obj(TRI, [(0, 1, 2)], TRI_VN, [(0, 1, 2)]), spectrum=(10000.0, 10000.0, 10000.0))], "walls",
        ["point", "distant", "sphere_emitter", "tri_emitter", "unoccluded", "tri_normals_kept", "tri_normals_flipped"], direct=True)
    # sphere emitters and one triangle emitter: shadow_lists.cpp has no bound for what Triangle::sample returns and builds no list for the whole scene
    add("spheres_plus_triangle", [sphere(), sphere(pos=(40.0, 6.0, 5.0)), triangle(tri_obj(TRI, [(0, 1, 2)]))], "field", ["sphere_emitter", "tri_emitter", "!point", "!distant", "unoccluded"])
    add("mixed_delta_plus_black_sphere", [point(), sphere(spectrum=(0.0, 0.0, 0.0))], "walls", ["point", "sphere_emitter", "!distant", "!tri_emitter", "li_black", "unoccluded"])
    return out


CASES = _cases()
NAMES = sorted({k.rsplit("-", 1)[0] for k in CASES})


def find(prefix=None, integrator=None, carrier=None):
    return [k for k, c in CASES.items() if (prefix is None or k.startswith(prefix)) and (integrator is None or c.integrator == integrator) and (carrier is None or c.carrier == carrier)]


def has_area_light(c):
    if isinstance(c, str): c = CASES[c]
    return any(l["light_type"] == "diffuse" for l in c.lights)


def expected_constants(c):
    """Per light of the case (a Case or an id): {rrt_light field: value} the loaded record must hold - the table's constants. `w_light` and `area` are computed
    here in f64 from the table (compare to a few ulp), the rest is exact."""
    if isinstance(c, str): c = CASES[c]
    out = []
    for l in c.lights:
        if l["light_type"] == "point":
            out.append({"type": POINT, "spectrum": list(l["spectrum"]["values"]), "p_light": [0.0, 0.0, 0.0]})      # Q17
        elif l["light_type"] == "distant":
            sp = np.asarray(l["l"]["values"], np.float64) * np.asarray(l.get("scale", {"values": [1.0, 1.0, 1.0]})["values"], np.float64)
            w = np.subtract(l["from"], l["to"]).astype(np.float64)
            if "rotation_axis" in l: w = _rotate(w, l["rotation_axis"], l.get("rotation_angle", 0.0))
            if np.linalg.norm(w) != 0.0: w = w / np.linalg.norm(w)      # (Vector3::normalize leaves a zero vector as it is)
            out.append({"type": DISTANT, "spectrum": list(sp), "w_light": list(w), "world_radius": "positive"})
        else:
            sh = l["light_shape"]
            e = {"type": DIFFUSE, "spectrum": list(l["spectrum"]["values"])}
            if sh["shape_type"] == "sphere":
                r = sh["radius"]
                phi = np.radians(min(max(sh.get("phi_max", 360.0), 0.0), 360.0))
                e.update(shape_type=SPHERE, area=float(phi * r * (sh.get("z_max", r) - sh.get("z_min", -r))))      # Sphere::area sphere.rs:261-263
            else:
                q = _face(l["_obj"], sh["tri_num"])
                e.update(shape_type=TRIANGLE, area=float(0.5 * np.linalg.norm(np.cross(q[1] - q[0], q[2] - q[0]))))      # Triangle::area triangle.rs:420-425
            out.append(e)
    return out


def _face(obj_text, tri_num):
    """The three vertices of face tri_num of the OBJ text"""
    v = [np.array([float(x) for x in ln.split()[1:4]]) for ln in obj_text.splitlines() if ln.startswith("v ")]
    f = [ln.split()[1:4] for ln in obj_text.splitlines() if ln.startswith("f ")][tri_num]
    return [v[int(t.split("/")[0]) - 1] for t in f]


def emitter_vertices(c, light):
    if isinstance(c, str): c = CASES[c]
    return _face(c.lights[light]["_obj"], c.lights[light]["light_shape"]["tri_num"])


def _add_plastic(cfg):
    mtype, rgbs, floats = ROUGH_PLASTIC
    m = {"material_type": mtype, "material_name": "m_rough"}
    for k, v in rgbs.items():
        cfg["rgb_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"m_rough_{k}", "v00": {"values": list(v)}, "v01": {"values": list(v)}})
        m[k] = f"m_rough_{k}"
    for k, v in floats.items():
        cfg["float_texture"].append({"texture_type": "BilerpTexture", "texture_name": f"m_rough_{k}", "v00": v, "v01": v})
        m[k] = f"m_rough_{k}"
    cfg["materials"] = copy.deepcopy(cfg["materials"]) + [m]


def scene(wd, name, carrier=None):
    """The frame of the module docstring for the case (a Case or an id), on its own carrier or on `carrier`; returns (cfg, root) for Scene.loads."""
    from rs_ray_toy_amd import scenes
    c = CASES[name] if isinstance(name, str) else name
    tag = name if isinstance(name, str) else "case"
    carrier = carrier or c.carrier
    if carrier == "field":
        cfg, root = scenes.cfg4(wd, xres=XRES, yres=YRES, nsamp=NSAMP, max_depth=DEPTH, n=FIELD_N)
    else:
        cfg, root = scenes.cfg3(wd, xres=XRES, yres=YRES, nsamp=NSAMP, max_depth=DEPTH)      # material_shapes.py::_enclosure
        cube, box = cfg["Aggregate"]["primitives"]
        cube["instances"][0]["rotation_axis"] = [1.0, 2.0, 3.0]
        box["instances"] = [{"world_pos": [0.0, 0.0, 0.0], **FLOOR_TILT}]
        _add_plastic(cfg)
        cube["material_name"] = "m_rough"
    lights = []
    for i, l in enumerate(copy.deepcopy(c.lights)):
        text = l.pop("_obj", None)
        if text is not None:
            fn = f"emitter_{tag}_{i}.obj"
            with open(os.path.join(wd, fn), "w") as f: f.write(text)
            cfg["objs"] = cfg["objs"] + [{"filename": fn, "obj_name": f"emitter_{i}"}]
            l["light_shape"]["obj_name"] = f"emitter_{i}"
        lights.append(l)
    cfg["lights"] = lights
    if c.integrator != PATH:
        cfg["Integrator"] = {"integrator_type": "DirectLighting", "light_strategy": c.integrator, "max_depth": DEPTH}
    return cfg, root


def census_problems(c, n):
    """What the census n (oracle_lib.light_census of ONE oracle frame of case c) lacks of what c's tags promise; an empty list if nothing."""
    if isinstance(c, str): c = CASES[c]
    bad = []
    for tag in c.tags:
        if tag.startswith("!"):
            if n[tag[1:]] != 0: bad.append(f"{tag[1:]} must stay zero, is {n[tag[1:]]}")
        elif n[tag] < TAG_MIN: bad.append(f"{tag} must be raised {TAG_MIN} times, is {n[tag]}")
    if c.integrator != ALL:      # the choosers: every light index is chosen, none beyond the table
        nl = len(c.lights)
        if any(v == 0 for v in n["chosen"][:nl]): bad.append(f"every light is chosen: {n['chosen'][:nl]}")
        if any(n["chosen"][nl:]): bad.append(f"no index beyond the table is chosen: {n['chosen']}")
    elif any(n["chosen"]): bad.append("`all` chooses nothing")
    return bad

