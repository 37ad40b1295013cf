"""Lens cull table of the fp32 camera kernel (csrc/host/lens_cull.cpp, dtraverse_f32.hpp k_raygen_main_f32), on the GPU.

With the table the camera kernel drops the samples of dead (r_film, p_lens) cells before any lens arithmetic and packs the survivors into whole
waves before the first interface instead of after the third. The lens arithmetic itself is unchanged (rg_begin_lean / rg_step_lean on the same
values, the state carried through LDS as before), and a culled sample is one the lens would have stopped: frames, weights, rays generated and
query counts with and without the table (option lens_cull) must be identical bit for bit. The table's own promise is checked on the CPU by
tests/test_lens_cull_table.py.
"""
import numpy as np
import pytest

from rs_ray_toy_amd import RRT_F32, RRT_FIXED_BVH, Renderer, Scene, scenes

pytestmark = pytest.mark.gpu


def _random_lens(seed):
    """scene.json's double Gauss with every radius, thickness and aperture perturbed, a random stop and focus distance (as
    tests/test_gpu_parity.py's random prescriptions)."""
    def make(wd):
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
    return make


def _direct(wd):
    cfg, root = scenes.cfg4(wd, xres=128, yres=96, nsamp=9, max_depth=3, n=64)
    cfg["Integrator"] = {"integrator_type": "DirectLighting", "max_depth": 3, "light_strategy": "UniformSampleAll"}
    return cfg, root


CASES = {
    "cfg4_full_size": lambda wd: scenes.cfg4(wd),                                            # 1024^2, 256 spp, depth 8: the bench frame
    "cfg4_small": lambda wd: scenes.cfg4(wd, xres=128, yres=96, nsamp=17, max_depth=5, n=64),
    "cfg4_passes": lambda wd: scenes.cfg4(wd, xres=128, yres=96, nsamp=17, max_depth=5, n=64),
    "cfg4_bands": lambda wd: scenes.cfg4(wd, xres=128, yres=96, nsamp=17, max_depth=5, n=64),
    "cfg4_spb1": lambda wd: scenes.cfg4(wd, xres=128, yres=96, nsamp=17, max_depth=5, n=64),
    "cfg4_direct": _direct,
    "cfg2_tiny_film": lambda wd: scenes.cfg2(wd, xres=24, yres=16, nsamp=65, max_depth=2),   # 0.05 px is 70 um of film: the aux-margin case
    "cfg2_640x360": lambda wd: scenes.cfg2(wd, xres=640, yres=360, nsamp=9, max_depth=2),
}
CASES.update({f"random_lens_{seed}": _random_lens(seed) for seed in range(1, 9)})


@pytest.mark.parametrize("which", sorted(CASES))
def test_lens_cull_changes_nothing(which, workdir):
    cfg, root = CASES[which](workdir)
    sc = Scene.loads(cfg, root, flags=RRT_FIXED_BVH)
    W, H = sc.resolution
    ns = int(sc.desc.sampler.samples_per_pixel)
    r = Renderer(sc, 0, RRT_F32)
    if which == "cfg4_passes": r.set_option("max_paths", 128 * 96 * 3)      # several pool passes per frame
    if which == "cfg4_spb1": r.set_option("rg_spb", 1)                      # one sample of 512 pixels per camera workgroup
    out = {}
    for on in (1, 0):
        r.set_option("lens_cull", on)
        if which == "cfg4_bands":
            parts = [r.render_bands(k, 3, stats=True) for k in range(3)]
            film, st = sum(f for f, _ in parts), [s for _, s in parts]
            stats = [(s.camera_rays, s.closest_queries, s.any_queries) for s in st]
        else:
            film, st = r.render(stats=True)
            stats = [(st.camera_rays, st.closest_queries, st.any_queries)]
        rect = (0, 0, 64, 64) if which == "cfg4_passes" else (0, 0, min(W, 256), min(H, 128))   # (camera_samples takes one pool pass)
        _, rays, w = r.camera_samples(rect, 1, min(ns, 9))
        out[on] = (film, stats, rays, w)
    r.close()
    (film1, st1, rays1, w1), (film0, st0, rays0, w0) = out[1], out[0]
    print(f"{which}: rays generated {[s[0] for s in st1]}, closest {[s[1] for s in st1]}, any {[s[2] for s in st1]}")
    assert st1 == st0 and all(s[0] > 0 for s in st1)
    assert np.array_equal(w1, w0) and np.array_equal(rays1, rays0)
    assert np.array_equal(film1, film0, equal_nan=True)
    assert np.nanmax(film1[..., :3]) > 0
