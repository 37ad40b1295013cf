"""Film records of the fp32 path integrator (option film_records; dtraverse_f32.hpp k_raygen_main_f32, k_raygen_aux2_f32, k_film_box_runs), on the GPU.

On the tile-tree passes (8 x 8 tile x 8 samples per camera workgroup) with the box filter of radius 0.5 on untextured scenes, a sample's
radiance lives in a record of its camera workgroup's run instead of in its slot, and the box film walks the runs. Each pixel makes the same
sequence of film_box_add() calls as k_film_box (see the kernel's header comment), so frames, filter-weight sums, rays generated and query
counts with the option on and off must be identical bit for bit - over several pool passes, in bands, through stage B, with the root and
lens culls on or off. Wide filters and textured scenes keep the per-slot state: there the option changes nothing at all.
"""
import numpy as np
import pytest

from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

pytestmark = pytest.mark.gpu

SMALL = dict(xres=128, yres=96, nsamp=25, max_depth=5, n=64)


def _textured(wd):
    cfg, root = scenes.cfg4(wd, **SMALL)
    cfg["rgb_texture"] = list(cfg.get("rgb_texture", [])) + [
        {"texture_type": "BilerpTexture", "texture_name": "kd_ramp", "v00": {"values": [0.2, 0.3, 0.4]}, "v01": {"values": [0.7, 0.5, 0.3]}}]
    cfg["materials"] = list(cfg["materials"]) + [{"material_type": "MatteMaterial", "material_name": "mat_ramp", "kd": "kd_ramp"}]
    cfg["Aggregate"]["primitives"][0]["material_name"] = "mat_ramp"
    return cfg, root


def _wide_filter(wd):
    cfg, root = scenes.cfg4(wd, **SMALL)
    cfg["Film"]["Filter"] = {"filter_type": "GaussianFilter", "radius": [1.5, 1.5], "alpha": 1.0}
    return cfg, root


# name: (scene, options set on the handle, whether the pass writes film records)
CASES = {
    "cfg4_full_size": (lambda wd: scenes.cfg4(wd), {}, True),                                     # 1024^2, 256 spp, depth 8: the bench frame
    "cfg4_24x16": (lambda wd: scenes.cfg4(wd, xres=24, yres=16, nsamp=65, max_depth=5, n=64), {}, True),
    "cfg4_bands": (lambda wd: scenes.cfg4(wd, **SMALL), {}, True),
    "cfg4_passes": (lambda wd: scenes.cfg4(wd, **SMALL), {"max_paths": 128 * 96 * 8}, True),      # three pool passes of 8 samples
    "cfg4_stage_b": (lambda wd: scenes.cfg4(wd, **SMALL), {"aux_margin": 0}, True),               # every survivor goes through stage B
    "cfg4_no_root_cull": (lambda wd: scenes.cfg4(wd, **SMALL), {"root_cull": 0}, True),
    "cfg4_no_lens_cull": (lambda wd: scenes.cfg4(wd, **SMALL), {"lens_cull": 0}, True),
    "cfg5_small": (lambda wd: scenes.cfg5(wd, xres=256, yres=256, nsamp=33, max_depth=8, n=64), {}, True),
    "wide_filter": (_wide_filter, {}, False),
    "textured": (_textured, {}, False),
}


@pytest.mark.parametrize("which", sorted(CASES))
def test_film_records_change_nothing(which, workdir):
    make, opts, records = CASES[which]
    cfg, root = make(workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    r = Renderer(sc, 0, RRT_F32)
    for k, v in opts.items():
        r.set_option(k, v)
    out = {}
    for on in (1, 0):
        r.set_option("film_records", on)
        if which == "cfg4_bands":
            parts = [r.render_bands(k, 3, stats=True) for k in range(3)]
            films, st = [f for f, _ in parts], [s for _, s in parts]
        else:
            film, s = r.render(stats=True)
            films, st = [film], [s]
        stats = [(s.camera_rays, s.closest_queries, s.any_queries, s.root_culled, s.tile_launches) for s in st]
        out[on] = (films, stats)
    r.close()
    (films1, st1), (films0, st0) = out[1], out[0]
    print(f"{which}: rays generated {[s[0] for s in st1]}, closest {[s[1] for s in st1]}, any {[s[2] for s in st1]}, tile launches {[s[4] for s in st1]}")
    assert st1 == st0 and all(s[0] > 0 for s in st1)
    if records:   # the passes are tile-tree passes, the ones that write film records
        assert all(s[4] > 0 for s in st1)
    for f1, f0 in zip(films1, films0):
        assert np.array_equal(f1, f0, equal_nan=True)   # XYZ sums and filter-weight sums
        assert np.nanmax(f1[..., :3]) > 0
