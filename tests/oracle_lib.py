"""ctypes binding of oracle/liboracle.so — the f64 CPU checker. Test infrastructure only."""
import ctypes as C
import os

import numpy as np

from rs_ray_toy_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
        L.oracle_last_error.restype = C.c_char_p
        L.oracle_halton_index.restype = C.c_uint64
        L.oracle_halton_index.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64]
        L.oracle_halton_dim.restype = C.c_double
        L.oracle_halton_dim.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
        L.oracle_radical_inverse.restype = C.c_double
        L.oracle_radical_inverse.argtypes = [C.c_int, C.c_uint64]
        L.oracle_vec3_ops.argtypes = [C.c_void_p] * 5
        L.oracle_sphere_intersect_p.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.oracle_bsdf_eval.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        L.oracle_bsdf_eval.restype = C.c_int
        L.oracle_texture_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.oracle_surface_differentials.argtypes = [C.c_void_p, C.c_void_p]
        L.oracle_trace_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p]
        L.oracle_trace_any.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.oracle_trace_closest_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4
        L.oracle_trace_any_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.oracle_camera_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_sampler_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_render_rect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.oracle_mip_census.restype = None
        L.oracle_mip_census.argtypes = [C.c_void_p, C.c_int]
        L.oracle_bsdf_census.restype = None
        L.oracle_bsdf_census.argtypes = [C.c_void_p, C.c_int]
        L.oracle_tex_census.restype = None
        L.oracle_tex_census.argtypes = [C.c_void_p, C.c_int]
        L.oracle_light_census.restype = None
        L.oracle_light_census.argtypes = [C.c_void_p, C.c_int]
        L.oracle_path_census.restype = None
        L.oracle_path_census.argtypes = [C.c_void_p, C.c_int]
        L.oracle_light_sample.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        L.oracle_light_sample.restype = C.c_int
        _lib = L
    return _lib


class OracleError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise OracleError(f"[{rc}] {lib().oracle_last_error().decode()}")


def _d(scene):
    return C.byref(scene.desc)


def halton_index(scene, px, py, sample_num):
    return lib().oracle_halton_index(_d(scene), px, py, sample_num)


def halton_dim(scene, index, dim):
    return lib().oracle_halton_dim(_d(scene), index, dim)


def trace_closest(scene, o, d, tmax, want_geometry=False, flat=False):
    """flat=False: the reference's per-primitive ray transform; flat=True: world-space flattened instances,
    the evaluation order of the HIP kernels (bit-comparable with the device's f64 mode)."""
    n = len(tmax)
    o = np.ascontiguousarray(o, np.float64); d = np.ascontiguousarray(d, np.float64); tmax = np.ascontiguousarray(tmax, np.float64)
    t = np.empty(n); prim = np.empty(n, np.int32); u = np.empty(n); v = np.empty(n)
    nodes = np.empty(n, np.uint32); prims = np.empty(n, np.uint32)
    p = np.zeros((n, 3)); nn = np.zeros((n, 3)); margin = np.zeros(n)
    _check(lib().oracle_trace_closest(_d(scene), o.ctypes.data, d.ctypes.data, tmax.ctypes.data, n, t.ctypes.data, prim.ctypes.data,
                                      u.ctypes.data, v.ctypes.data, nodes.ctypes.data, prims.ctypes.data,
                                      p.ctypes.data if want_geometry else None, nn.ctypes.data if want_geometry else None,
                                      1 if flat else 0, margin.ctypes.data))
    out = dict(t=t, prim=prim, u=u, v=v, nodes=nodes, prims=prims, margin=margin)
    if want_geometry:
        out.update(p=p, n=nn)
    return out


def trace_any(scene, o, d, tmax, flat=False):
    n = len(tmax)
    o = np.ascontiguousarray(o, np.float64); d = np.ascontiguousarray(d, np.float64); tmax = np.ascontiguousarray(tmax, np.float64)
    occ = np.zeros(n, np.uint8); nodes = np.empty(n, np.uint32); prims = np.empty(n, np.uint32); margin = np.zeros(n)
    _check(lib().oracle_trace_any(_d(scene), o.ctypes.data, d.ctypes.data, tmax.ctypes.data, n, occ.ctypes.data, nodes.ctypes.data, prims.ctypes.data,
                                  1 if flat else 0, margin.ctypes.data))
    return dict(occluded=occ.astype(bool), nodes=nodes, prims=prims, margin=margin)


def trace_closest_probe(scene, o, d, tmax, flat=False):
    """trace_closest and two more per-ray outputs: peak = the largest number of entries the walk's stack held, peak_hit = the same
    counting only entries whose box the ray's slabs hit (what a walk holds that tests a child's box before it pushes it: the fp32 pair-node kernels), tri_margin = the smallest
    gap of every comparison of every triangle test the walk made (WalkProbe in rrt_oracle.cpp; inf where it tested none)."""
    n = len(tmax)
    o = np.ascontiguousarray(o, np.float64); d = np.ascontiguousarray(d, np.float64); tmax = np.ascontiguousarray(tmax, np.float64)
    t = np.empty(n); prim = np.empty(n, np.int32); u = np.empty(n); v = np.empty(n)
    nodes = np.empty(n, np.uint32); prims = np.empty(n, np.uint32)
    margin = np.zeros(n); peak = np.zeros(n, np.uint32); tri_margin = np.zeros(n); peak_hit = np.zeros(n, np.uint32)
    _check(lib().oracle_trace_closest_probe(_d(scene), o.ctypes.data, d.ctypes.data, tmax.ctypes.data, n, t.ctypes.data, prim.ctypes.data, u.ctypes.data,
                                            v.ctypes.data, nodes.ctypes.data, prims.ctypes.data, 1 if flat else 0, margin.ctypes.data, peak.ctypes.data,
                                            tri_margin.ctypes.data, peak_hit.ctypes.data))
    return dict(t=t, prim=prim, u=u, v=v, nodes=nodes, prims=prims, margin=margin, peak=peak, tri_margin=tri_margin, peak_hit=peak_hit)


def trace_any_probe(scene, o, d, tmax, flat=False):
    n = len(tmax)
    o = np.ascontiguousarray(o, np.float64); d = np.ascontiguousarray(d, np.float64); tmax = np.ascontiguousarray(tmax, np.float64)
    occ = np.zeros(n, np.uint8); nodes = np.empty(n, np.uint32); prims = np.empty(n, np.uint32)
    margin = np.zeros(n); peak = np.zeros(n, np.uint32); tri_margin = np.zeros(n); peak_hit = np.zeros(n, np.uint32)
    _check(lib().oracle_trace_any_probe(_d(scene), o.ctypes.data, d.ctypes.data, tmax.ctypes.data, n, occ.ctypes.data, nodes.ctypes.data, prims.ctypes.data,
                                        1 if flat else 0, margin.ctypes.data, peak.ctypes.data, tri_margin.ctypes.data, peak_hit.ctypes.data))
    return dict(occluded=occ.astype(bool), nodes=nodes, prims=prims, margin=margin, peak=peak, tri_margin=tri_margin, peak_hit=peak_hit)


def camera_samples(scene, rect, s0, s1):
    x0, y0, x1, y1 = rect
    n = (x1 - x0) * (y1 - y0) * (s1 - s0)
    dims = np.zeros((n, 5)); rays = np.zeros((n, 6)); w = np.zeros(n)
    r = (C.c_int32 * 4)(*rect)
    _check(lib().oracle_camera_samples(_d(scene), r, s0, s1, dims.ctypes.data, rays.ctypes.data, w.ctypes.data))
    return dims, rays, w


def sampler_values(scene, pixel, sample_num, first, count):
    """Renderer.sampler_values over the oracle's Sampler: pixel (n, 2) of (x, y), sample_num (n,); returns index (n,) uint64, v1 (n, count), v2 (n, count, 2)."""
    pixel = np.asarray(pixel)
    word = np.ascontiguousarray((pixel[:, 1].astype(np.uint32) << 16) | pixel[:, 0].astype(np.uint32), np.uint32)
    sample_num = np.ascontiguousarray(sample_num, np.uint32)
    n = len(sample_num)
    index = np.zeros(n, np.uint64); v1 = np.zeros((n, count)); v2 = np.zeros((n, count, 2))
    _check(lib().oracle_sampler_values(_d(scene), word.ctypes.data, sample_num.ctypes.data, n, first, count, index.ctypes.data, v1.ctypes.data, v2.ctypes.data))
    return index, v1, v2


def render(scene, rect=None, n_threads=0, faithful_sampler_rebuild=False, stats=False, flat=False):
    W, H = scene.resolution
    rect = rect or (0, 0, W, H)
    film = np.zeros((H, W, 4))
    st = A.RenderStats()
    r = (C.c_int32 * 4)(*rect)
    _check(lib().oracle_render_rect(_d(scene), r, film.ctypes.data, C.byref(st), n_threads, 1 if faithful_sampler_rebuild else 0,
                                    1 if flat else 0))
    return (film, st) if stats else film


def random_rays(scene, n, seed=0):
    """Rays from points around the scene bound towards points inside it (normalised d, tmax = inf)."""
    rng = np.random.default_rng(seed)
    wb = np.array(list(scene.desc.world_bound))
    lo, hi = wb[:3], wb[3:]
    c, ext = (lo + hi) / 2, np.maximum(hi - lo, 1e-3)
    o = c + (rng.random((n, 3)) - 0.5) * ext * 3.0
    tgt = lo + rng.random((n, 3)) * ext
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d, np.full(n, np.inf)


def texture_eval(scene, tex, p=(0, 0, 0), uv=(0, 0), dpdx=(0, 0, 0), dpdy=(0, 0, 0), duv=(0, 0, 0, 0)):
    """Texture::evaluate of scene.desc.textures[tex] at a hand-made interaction; duv = (dudx, dvdx, dudy, dvdy)."""
    si = np.array(list(p) + list(uv) + list(dpdx) + list(dpdy) + list(duv), np.float64)
    out = np.zeros(3)
    _check(lib().oracle_texture_eval(_d(scene), tex, si.ctypes.data, out.ctypes.data))
    return out


MIP_CENSUS = ("tri_below", "tri_last", "tri_between", "ewa_degenerate", "ewa_clamped", "ewa_plain", "ewa_nan", "ewa_ok", "texel_out", "texel_in",
              "triangle_negative")


def mip_census(reset=True):
    """What the oracle's MIPMap lookups did since the last reset (MipCensus in rrt_oracle.cpp), process-wide: trilinear lookups with level < 0
    (tri_below), level >= levels - 1 (tri_last) and between two levels; EWA lookups with minor_length == 0, with the anisotropy clamp applied and
    plain; ewa() results that are 0 / 0 (ewa_nan) and that have sum_wts > 0 (two ewa() calls per lookup); texel() calls with s >= u_res or
    t >= v_res and in range; triangle() calls with a negative s or t. Call it once to reset, render, call it again to read."""
    out = (C.c_uint64 * len(MIP_CENSUS))()
    lib().oracle_mip_census(out, 1 if reset else 0)
    return dict(zip(MIP_CENSUS, (int(v) for v in out)))


BSDF_CENSUS = ("built_0", "built_1", "built_2", "built_4",
               "lobe_lambert", "lobe_oren_nayar", "lobe_microfacet", "lobe_spec_refl", "lobe_debug_diffuse", "lobe_debug_specular", "lobe_spec_trans",
               "lobe_fresnel_spec", "lobe_lambert_trans", "lobe_microfacet_trans",
               "sample_no_match", "sample_comp0", "sample_comp1", "sample_comp2", "sample_comp3", "sample_pdf0", "sample_other_pdfs",
               "refract_fail_specular", "refract_fail_microfacet", "fresnel_spec_reflect", "fresnel_spec_transmit", "fr_swap", "fr_tir",
               "tr11_normal", "tr11_clamp", "micro_reject_back", "micro_reject_hemi",
               "alpha_clamp", "oren_max_cos", "oren_skip", "f_leak", "direct_f_black", "path_last_query")


def bsdf_census(reset=True):
    """What the oracle's material and BxDF code did since the last reset (BsdfCensus in rrt_oracle.cpp), process-wide: BSDFs built with 0 / 1 / 2 / 4
    lobes and the lobes added per kind; Bsdf::sample_f calls with no matching lobe, by the index of the chosen component, that returned pdf 0 and
    that added the other lobes' pdfs (a non-reflective lobe chosen among several); refract() failures in SpecularTransmission / FresnelSpecular
    and in MicrofacetTransmission; FresnelSpecular's two branches; fr_dielectric calls that swapped the indices (cos_i <= 0) and that met total
    internal reflection; tr_sample_11's cos_t > 0.9999 branch and its 1e10 clamp; microfacet samples rejected by dot(wo, wh) < 0 and by
    !same_hemisphere; roughness_to_alpha calls at or below its 1e-3 clamp; Oren-Nayar evaluations with max_cos computed and skipped; Bsdf::f calls
    where the shading frame and the geometric normal disagree on reflection against transmission; estimate_direct returns on a black f; closest-hit queries the path integrator
    issued at bounces == max_depth (the device leaves them out: DESIGN.md section 3, dead work 2). Call it
    once to reset, render, call it again to read."""
    out = (C.c_uint64 * len(BSDF_CENSUS))()
    lib().oracle_bsdf_census(out, 1 if reset else 0)
    return dict(zip(BSDF_CENSUS, (int(v) for v in out)))


TEX_CENSUS = ("node_constant", "node_mix", "node_bilerp", "node_checker2d", "node_checker3d", "node_scale", "node_windy", "node_wrinkled", "node_uv",
              "node_image", "depth_max",
              "fb_mix_t1", "fb_mix_t2", "fb_mix_amount", "fb_scale_t1", "fb_scale_t2", "fb_checker_t1", "fb_checker_t2",
              "chk_aa_none", "chk_same_cell", "chk_filtered", "chk_half", "chk_negative_sum", "chk_bump_int_negative", "chk3_negative_sum",
              "round_calls", "round_phi_wrapped", "fold_dx_high", "fold_dx_low", "fold_dy_high", "fold_dy_low", "round_pole",
              "noise_sums", "noise_n_int_0", "noise_partial", "noise_all_octaves", "noise_calls", "noise_negative_lattice", "noise_saturated",
              "diff_calls", "diff_no_aux", "diff_not_finite", "diff_axis_yz", "diff_axis_xz", "diff_axis_xy", "diff_solve_failed",
              "bump_calls", "bump_du_fallback", "bump_dv_fallback", "bump_slope", "bump_fallback_slope",
              "tri_hits", "tri_degenerate_uv", "tri_negative_det", "tri_coord_dn",
              "mix_amount_outside", "mat_negative_value")


def tex_census(reset=True):
    """What the oracle's texture code did since the last reset (TexCensus in rrt_oracle.cpp), process-wide: nodes evaluated per type and the deepest
    level reached (depth_max: a maximum, the root is level 1); fallback constants used per type and slot (a 3D checkerboard counts with the 2D one); 2D
    checkerboard evaluations that returned at aamode none, at "same cell", from the bump_int expression (filtered) and from the area2 = 0.5 shortcut
    (half), those whose cell sum floor(s) + floor(t) is negative and those whose bump_int saw a negative argument; 3D checkerboard evaluations with a
    negative cell sum; sphere() / cylinder() calls (three per mapping), those with phi < 0 wrapped, those within 0.05 rad of a pole, and the folds of
    dst[1] > 0.5 / < -0.5 for dstdx and dstdy; fbm / turbulence calls (noise_sums) with n_int == 0, with 0 < n < octaves and with n == octaves,
    noise() calls, those with a negative lattice coordinate and those with a coordinate past 2^31 (a saturated cast); compute_differentials calls,
    those without an auxiliary ray, with tx or ty not finite, per dominant-axis branch (the pair of axes kept) and solve_2x2 failures (two solves per
    call); Material::bump calls, its du / dv == 0 fallbacks, the calls whose
    displaced evaluations differ from the one at the hit (bump_slope: a finite difference that is not 0) and those of them on the du fallback; successful triangle intersection tests (every candidate the traversal accepts, not
    only the closest), those with a degenerate uv, with a negative uv determinant, and with dndu / dndv from coordinate_system(dn); Mix amounts
    outside [0, 1]; texture values with a negative channel handed to a material parameter. Call it once to reset, render, call it again to read."""
    out = (C.c_uint64 * len(TEX_CENSUS))()
    lib().oracle_tex_census(out, 1 if reset else 0)
    return dict(zip(TEX_CENSUS, (int(v) for v in out)))


LIGHT_CENSUS = ("point", "distant", "sphere_emitter", "tri_emitter", "tri_normals_kept", "tri_normals_flipped", "tri_normals_mode2",
                "li_black", "pdf_zero", "pdf_not_positive", "emitter_backface", "f_black", "occluded", "unoccluded",
                "choose_distrib", "choose_plain", "choice_clamped", "choice_boundary")
LIGHT_CHOSEN = 32


def light_census(reset=True):
    """What the oracle's light code did since the last reset (LightCensus in rrt_oracle.cpp), process-wide: Light::sample_li calls per kind (point, distant,
    and Shape::sample of a sphere and of a triangle emitter); triangle emitters with vertex normals whose faceforward kept and turned the geometric
    normal, and those of a mesh with `vn` lines and no normal indices (mode 2; they count as kept or flipped too); estimate_direct calls whose light
    sample had pdf > 0 and a black li, pdf == 0, a pdf that is neither (NaN); area-light samples with dot(n, -wi) <= 0; estimate_direct calls that
    returned on a black f, whose shadow ray was occluded and was not; uniform_sample_one_light calls that chose by the light distribution (Path) and by
    v * n_lights (DirectLighting `one`), those of either whose index had to be clamped to the last light, and those whose sample lies within 2^-23 of an inner entry of the light
    cdf (v = u * n_lights within n_lights * 2^-23 of an inner integer): the choices an fp32 rounding can hand to the neighbouring light. `chosen` is the list of how often each
    light index was chosen (indices past 31 count as 31). Call it once to reset, render, call it again to read."""
    out = (C.c_uint64 * (len(LIGHT_CENSUS) + LIGHT_CHOSEN))()
    lib().oracle_light_census(out, 1 if reset else 0)
    n = dict(zip(LIGHT_CENSUS, (int(v) for v in out)))
    n["chosen"] = [int(v) for v in out[len(LIGHT_CENSUS):]]
    return n


PATH_CENSUS = ("started", "end_escaped", "end_depth", "end_black_f", "end_pdf_zero", "end_roulette",
               "vertex_nee", "vertex_specular_only", "vertex_no_lights",
               "rr_tests", "rr_draws", "rr_floor", "rr_survivors", "rr_eta_decided", "eta_enter", "eta_leave", "dim_max",
               "rr_draw_near", "rr_test_near",
               "li_calls", "reflect_taken", "transmit_taken", "recursion_refused", "level_max")
PATH_ENDS = ("escaped", "depth", "black_f", "pdf_zero", "roulette")
PATH_BINS = 66


def path_census(reset=True):
    """What the oracle's integrator loops did since the last reset (PathCensus in rrt_oracle.cpp), process-wide. Path: camera samples that entered li_path
    (started); ends by cause - the closest-hit query missed while bounces < max_depth (escaped), bounces reached max_depth (depth), sample_f returned a
    black f, a pdf of 0, Russian roulette ended the path; vertices that drew for next-event estimation, that did not because no lobe is non-specular (all specular, or a BSDF without lobes), and
    that have a non-specular lobe in a scene without lights (no draw either); vertices with bounces > 3, where the roulette test compares (rr_tests),
    those of them that took the draw (rr_draws), draws whose q = max(1 - rr_max, 0.05) sits on the floor, draws survived; tests that `beta` alone
    would have decided the other way than `beta * eta_scale` did (rr_eta_decided); eta_scale updates at a specular transmission from outside
    (eta_enter) and from inside; the largest Halton dimension counter after a draw (dim_max, a maximum); roulette draws with |u - q| < 2^-20 and tests
    with |rr_max - threshold| < 2^-20 |threshold|: the decisions an fp32 rounding can flip. DirectLighting and Debug: li calls, specular_reflect and
    specular_transmit recursions taken, li calls that did not recurse because depth + 1 >= max_depth at a hit with a specular lobe, and the deepest
    reference depth reached (level_max, a maximum; the camera ray is depth 1). `ends` maps each cause to its histogram over the value of `bounces` at
    the end (bins 0 .. 64 and an overflow bin), `li_depth` is the histogram of li calls over the reference depth. Call it once to reset, render, call it
    again to read."""
    n_flat = len(PATH_CENSUS)
    out = (C.c_uint64 * (n_flat + (len(PATH_ENDS) + 1) * PATH_BINS))()
    lib().oracle_path_census(out, 1 if reset else 0)
    n = dict(zip(PATH_CENSUS, (int(v) for v in out)))
    n["ends"] = {c: [int(v) for v in out[n_flat + k * PATH_BINS:n_flat + (k + 1) * PATH_BINS]] for k, c in enumerate(PATH_ENDS)}
    n["li_depth"] = [int(v) for v in out[n_flat + len(PATH_ENDS) * PATH_BINS:]]
    return n


def light_sample(scene, light, ref_p, u0=0.5, u1=0.5):
    """Light::sample_li of scene.desc.lights[light] for the reference point ref_p: dict(li, wi, pdf, p1, n1); p1 / n1 are the far end of the visibility tester."""
    ref_p = np.ascontiguousarray(ref_p, np.float64)
    out = np.zeros(13)
    _check(lib().oracle_light_sample(_d(scene), light, ref_p.ctypes.data, u0, u1, out.ctypes.data))
    return dict(li=out[0:3].copy(), wi=out[3:6].copy(), pdf=out[6], p1=out[7:10].copy(), n1=out[10:13].copy())


def fp32_bar(d32, allowance=0.0):
    """test_gpu_parity.py::test_transmissive_materials_path's fp32 bar on d32, the per-pixel difference of an fp32 frame from the oracle's relative to the
    oracle's brightest pixel: more than 99 % of the pixels within 1e-4 (less `allowance`, the share of the pixels a test can show from the oracle alone to
    hold a decision that an fp32 rounding may flip), the median below 1e-5. The table tests (test_material_shapes.py, test_light_shapes.py,
    test_path_shapes.py) share it from here."""
    assert (d32 < 1e-4).mean() > 0.99 - allowance and np.median(d32) < 1e-5, ((d32 < 1e-4).mean(), np.median(d32), d32.max())


def surface_differentials(n, p, dpdu, dpdv, rxo, rxd, ryo, ryd):
    """compute_differentials (interaction.rs:223-284): dict(dpdx, dpdy, duv = (dudx, dvdx, dudy, dvdy))."""
    a = np.ascontiguousarray(np.concatenate([n, p, dpdu, dpdv, rxo, rxd, ryo, ryd]), np.float64)
    out = np.zeros(10)
    _check(lib().oracle_surface_differentials(a.ctypes.data, out.ctypes.data))
    return dict(dpdx=out[0:3].copy(), dpdy=out[3:6].copy(), duv=out[6:10].copy())


def bsdf_eval(scene, material, wo, wi, u0=0.5, u1=0.5, allow_multiple_lobes=True):
    """Bsdf of `material` in its local frame (n = +z): dict with f, pdf and one sample_f draw."""
    wo = np.ascontiguousarray(wo, np.float64); wi = np.ascontiguousarray(wi, np.float64)
    out = np.zeros(16)
    _check(lib().oracle_bsdf_eval(_d(scene), material, 1 if allow_multiple_lobes else 0, wo.ctypes.data, wi.ctypes.data, u0, u1, out.ctypes.data))
    return dict(f=out[0:3].copy(), pdf=out[3], s_wi=out[4:7].copy(), s_f=out[7:10].copy(), s_pdf=out[10], s_flags=int(out[11]), eta=out[12],
                n_lobes=int(out[13]), n_nonspecular=int(out[14]))
