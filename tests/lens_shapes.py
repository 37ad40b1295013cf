"""Hand-built lens prescriptions for the camera kernels. Test infrastructure only.

A lens table is caller-supplied data (Camera.lens_data of a scene document, rrt_camera::elems of a description), as a tree is (tests/bvh_shapes.py).
Every other camera test of the suite runs the 13-interface double Gauss of scenes.LENS_DATA, at most with its numbers perturbed: 13 interfaces, the
stop at index 5, simple_weighting on, a film diagonal of 20. The prescriptions here are chosen for what they reach in the fp32 camera kernels
(dtraverse_f32.hpp) and their host builders that such a lens never does. Rows are mm, front to rear: [curvature radius, thickness, eta, aperture
diameter]. The loader treats EVERY row with radius 0 as the stop: it keeps its own diameter only while Camera.aperture_diameter exceeds it.

  double_gauss_13   scenes.LENS_DATA: the baseline every other shape is read against
  singlet_2         k_raygen_main_f32's k_pack = -1 with the cull table off (no re-pack at all), k_pack = 1 with it on; no stop row
  stop_rear_3       rear_z = lens[n - 1].thickness comes from a stop row; the first interface traced is the stop
  stop_front_3      a stop at index 0: rg_lens_to_lds' tid == 0 (no eta_prev) on a stop row
  doublet_stop_4    k_pack = 0: the re-pack runs and exactly one interface follows it; a cemented surface with eta_t != 1
  two_singlets_5    k_pack = 1; an inner stop
  strong_singlet_2  steep incidence and total internal reflection inside the rim
  weak_surface_2    cancellation in c = |oc|^2 - R^2 at a nearly flat face (R = 5 m)
  padded_32         the last index of RgLensLds::a / ::b and of safe_s[32]
  padded_33         one past it: the dense kernels do not apply (pt_ok), the generic fp32 k_raygen / k_raygen_aux run
  padded_64         the ABI's limit (validate_desc)
padded_n is the double Gauss with n - 13 open stop planes (diameter 20, above the real stop's 17.512 and every ray that passed it) 0.05 mm apart in
the first 2.6 mm of the air gap behind the real stop, clear of the sag of the next surface: the same lens, through more rows.

Modifiers (a shape name's suffix, applied to double_gauss_13 and singlet_2):
  +weighted   simple_weighting false with the shutter open from 0.25 to 0.75: the weight (close - open) cos^4 area / rear_z * rear_z, coded in
              rg_begin_lean, dmath.hpp and the oracle
  +diag43     a film diagonal of 43 mm: the lens cull table's r domain and the exit-pupil boxes of a larger film

Negative cases:
  stop_in_thin_gap_14  the double Gauss with row 7's 0.23012 mm air gap split in half by an open stop: the stop plane lies behind the hit point on
                       the neighbouring curved surface for rim rays, and the loader panics as the reference does (camera.rs:186)
  padded_65            one row more than include/rrt.h allows: loads, and rrt_create refuses it before any device work
"""
import copy

from rs_ray_toy_amd import scenes

_DG = [list(scenes.LENS_DATA[4 * i:4 * i + 4]) for i in range(len(scenes.LENS_DATA) // 4)]

_SINGLET = [[60, 6, 1.5, 30], [-60, 0, 1, 30]]


def padded(n):
    """The double Gauss through n rows (n >= 14): k = n - 13 open stops behind the real one, inside the first 0.05 (k + 1) mm of its 4.55532 mm gap."""
    k = n - 13
    assert k >= 1 and 0.05 * (k + 1) < 2.7, "the extra planes stay clear of the sag of the next surface"
    rows = [list(r) for r in _DG[:5]]
    rows.append([0, 0.05, 0, 17.512])
    rows += [[0, 0.05, 0, 20.0] for _ in range(k)]
    rows[-1][1] = 4.55532 - 0.05 * k
    rows += [list(r) for r in _DG[6:]]
    assert len(rows) == n
    return rows


def _thin_gap():
    rows = [list(r) for r in _DG]
    rows[7][1] = 0.11506
    rows.insert(8, [0, 0.11506, 0, 20])
    return rows


LENSES = {
    "double_gauss_13": _DG,
    "singlet_2": _SINGLET,
    "stop_rear_3": [[60, 6, 1.5, 30], [-60, 5, 1, 30], [0, 0, 0, 12]],
    "stop_front_3": [[0, 5, 0, 12]] + _SINGLET,
    "doublet_stop_4": [[61.47, 6, 1.517, 30], [-43.47, 2.5, 1.649, 30], [-125, 4, 1, 30], [0, 0, 0, 14]],
    "two_singlets_5": [[80, 5, 1.5, 30], [-80, 6, 1, 30], [0, 6, 0, 12], [80, 5, 1.6, 28], [-80, 0, 1, 28]],
    "strong_singlet_2": [[22, 14, 1.7, 30], [-22, 0, 1, 30]],
    "weak_surface_2": [[31, 6, 1.5, 30], [-5000, 0, 1, 30]],
    "padded_32": padded(32),
    "padded_33": padded(33),
    "padded_64": padded(64),
}
NEGATIVE = {"stop_in_thin_gap_14": _thin_gap(), "padded_65": padded(65)}

MODIFIERS = ("weighted", "diag43")
SHAPES = sorted(LENSES)                                                                                   # every prescription
MODIFIED = [f"{base}+{mod}" for base in ("double_gauss_13", "singlet_2") for mod in MODIFIERS]          # both modifiers on two of them
ALL = SHAPES + MODIFIED


def n_rows(name):
    return len({**LENSES, **NEGATIVE}[name.split("+")[0]])


def apply(cfg, name, aperture_diameter=None, diagonal=None):
    """Put the prescription `name` (with its +modifier, if any) into a scene document of rs_ray_toy_amd.scenes; returns cfg."""
    base, _, mod = name.partition("+")
    rows = {**LENSES, **NEGATIVE}[base]
    cam = cfg["Camera"]
    cam["lens_data"] = [float(x) for r in rows for x in r]
    if mod == "weighted":
        cam["simple_weighting"] = False
        cam["shutter_open"], cam["shutter_close"] = 0.25, 0.75
    elif mod == "diag43":
        cfg["Film"]["diagonal"] = 43
    else:
        assert mod == "", mod
    if aperture_diameter is not None: cam["aperture_diameter"] = float(aperture_diameter)
    if diagonal is not None: cfg["Film"]["diagonal"] = diagonal
    return cfg


def sample_scene(wd, name, xres=128, yres=96, **kw):
    """cfg2 with the prescription: the scene of the camera-sample tests (samples 1..8 of every pixel)."""
    cfg, root = scenes.cfg2(wd, xres=xres, yres=yres, nsamp=9, max_depth=2)
    return apply(cfg, name, **kw), root


def frame_scene(wd, name, filt=None, **kw):
    """cfg4 with 8192 triangles at 128 x 96, 8 samples per pixel, depth 4: the smallest frame that qualifies for tile trees, film records and the
    lens cull table at once (tests/test_lens_cull.py cfg4_small)."""
    cfg, root = scenes.cfg4(wd, xres=128, yres=96, nsamp=9, max_depth=4, n=64)
    if filt: cfg["Film"]["Filter"] = copy.deepcopy(filt)
    return apply(cfg, name, **kw), root
