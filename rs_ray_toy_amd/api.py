"""Python host mirror of the reference's render entry points, over the C ABI in include/rrt.h.

Names follow the reference (`deploy_render` = renderprocess.rs:92; `Scene`, `Integrator.render`,
`Film.write_image`); errors the reference raises as panics surface as `RrtPanic`, out-of-scope features
as `RrtUnsupported`. There is no CPU fallback: every compute call goes to the HIP kernels in librrt.so.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

from . import _abi as A


class RrtError(RuntimeError):
    code = A.RRT_EINVAL


class RrtPanic(RrtError):
    """The reference would panic here (assert!/unwrap/index); message cites the reference line."""
    code = A.RRT_EPANIC


class RrtUnsupported(RrtError):
    code = A.RRT_EUNSUP


class RrtDeviceError(RrtError):
    code = A.RRT_EDEVICE


_ERR = {A.RRT_EPANIC: RrtPanic, A.RRT_EUNSUP: RrtUnsupported, A.RRT_EDEVICE: RrtDeviceError}


def _check(rc):
    if rc != A.RRT_OK:
        msg = A.lib().rrt_last_error().decode("utf-8", "replace")
        raise _ERR.get(rc, RrtError)(f"[{rc}] {msg}")


DEFAULT_PERM_SEED = 0x853C49E6748FEA9B


class Scene:
    """Scene + BVHAccel + RealisticCamera + Film/Sampler/Integrator parameters (host memory)."""

    def __init__(self, handle):
        self._h = handle
        self.desc = A.lib().rrt_scene_desc_of(handle).contents

    @classmethod
    def load(cls, path, flags=0, perm_seed=DEFAULT_PERM_SEED):
        h = C.c_void_p()
        _check(A.lib().rrt_scene_load(os.fsencode(path), flags, perm_seed, C.byref(h)))
        return cls(h)

    @classmethod
    def loads(cls, cfg, root_dir=".", flags=0, perm_seed=DEFAULT_PERM_SEED):
        text = cfg if isinstance(cfg, str) else json.dumps(cfg)
        h = C.c_void_p()
        _check(A.lib().rrt_scene_load_str(text.encode(), os.fsencode(root_dir), flags, perm_seed, C.byref(h)))
        return cls(h)

    @property
    def warnings(self):
        L = A.lib()
        return [L.rrt_scene_warning(self._h, i).decode() for i in range(L.rrt_scene_warning_count(self._h))]

    @property
    def resolution(self):
        return self.desc.film.xres, self.desc.film.yres

    def prim_ids(self, by="object"):
        """One uint32 id per entry of rrt_scene_desc.prims, for Renderer.render_mattes: "material" = material index + 1; "instance" =
        rrt_prim.instance + 2 (uninstanced primitives get 1); "object" = 1 + the dense index of the distinct (instance, material) pairs in
        ascending order; "prim" = index + 1."""
        d = self.desc
        n = int(d.n_prims)
        if n == 0:
            return np.zeros(0, np.uint32)
        prims = np.frombuffer((A.Prim * n).from_address(C.addressof(d.prims.contents)), dtype=np.dtype(A.Prim))     # a view of the scene's own records
        inst, mat = prims["instance"].astype(np.int64), prims["material"].astype(np.int64)
        if by == "material":
            ids = mat + 1
        elif by == "instance":
            ids = inst + 2
        elif by == "object":
            _, dense = np.unique(np.stack([inst, mat], -1), axis=0, return_inverse=True)
            ids = dense.reshape(-1) + 1
        elif by == "prim":
            ids = np.arange(n, dtype=np.int64) + 1
        else:
            raise ValueError(f'prim_ids: by is "material", "instance", "object" or "prim", not {by!r}')
        return np.ascontiguousarray(ids, np.uint32)

    def prim_order(self):
        """rrt_scene_desc.prim_order as an array: entry i (the index rrt_hits.prim, rrt_surface.prim and rrt_atlas_sites speak) -> index into prims,
        so scene.prim_ids(by)[scene.prim_order()] selects list entries by object, instance or material."""
        d = self.desc
        n = int(d.n_prim_order)
        if n == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(d.prim_order, shape=(n,)).copy()

    def __del__(self):
        try:
            if self._h:
                A.lib().rrt_scene_free(self._h)
                self._h = None
        except Exception:
            pass


def _np_dtype(precision):
    return np.float32 if precision == A.RRT_F32 else np.float64


class Renderer:
    """Device executor (`Integrator::render`, integrator/mod.rs:21-23) for one GPU."""

    def __init__(self, scene, device=0, precision=A.RRT_F32, flags=0):
        """`flags`: device-side flags OR-ed into a copy of the scene's desc (RRT_INSTANCES_KEEP / RRT_INSTANCES_FLATTEN)."""
        self.scene = scene
        self.precision = precision
        self.dtype = _np_dtype(precision)
        desc = scene.desc
        if flags:
            desc = A.SceneDesc.from_buffer_copy(scene.desc)   # shallow: the arrays stay the scene's
            desc.flags |= flags
        h = C.c_void_p()
        _check(A.lib().rrt_create(device, C.byref(desc), precision, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            A.lib().rrt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return A.lib().rrt_stream(self._h)

    @property
    def warnings(self):
        """rrt_warning(): what this handle's precision mode does not claim for the scene (fp32 + transmissive spheres ...)."""
        L = A.lib()
        return [L.rrt_warning(self._h, i).decode() for i in range(L.rrt_warning_count(self._h))]

    def set_option(self, key, value):
        _check(A.lib().rrt_set_option(self._h, key.encode(), float(value)))

    # BVHAccel::intersect (bvh.rs:183): o, d (n,3), tmax (n,) host arrays
    def trace_closest(self, o, d, tmax, counters=False, skip_prim=None):
        n = len(tmax)
        soa = [np.ascontiguousarray(a, self.dtype) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
        skip = None if skip_prim is None else np.ascontiguousarray(skip_prim, np.int32)
        rays = A.Rays(A.RRT_MEM_HOST, self.precision, *[a.ctypes.data for a in soa], None if skip is None else skip.ctypes.data)
        t = np.empty(n, self.dtype); u = np.empty(n, self.dtype); v = np.empty(n, self.dtype)
        prim = np.empty(n, np.int32)
        nodes = np.zeros(n, np.uint32); prims = np.zeros(n, np.uint32)
        hits = A.Hits(A.RRT_MEM_HOST, self.precision, t.ctypes.data, prim.ctypes.data, u.ctypes.data, v.ctypes.data,
                      nodes.ctypes.data if counters else None, prims.ctypes.data if counters else None)
        _check(A.lib().rrt_trace_closest(self._h, C.byref(rays), n, C.byref(hits)))
        out = dict(t=t, prim=prim, u=u, v=v)
        if counters:
            out.update(nodes=nodes, prims=prims)
        return out

    # BVHAccel::intersect_p (bvh.rs:124)
    def trace_any(self, o, d, tmax, skip_prim=None):
        n = len(tmax)
        soa = [np.ascontiguousarray(a, self.dtype) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
        skip = None if skip_prim is None else np.ascontiguousarray(skip_prim, np.int32)
        rays = A.Rays(A.RRT_MEM_HOST, self.precision, *[a.ctypes.data for a in soa], None if skip is None else skip.ctypes.data)
        occ = np.zeros(n, np.uint8)
        _check(A.lib().rrt_trace_any(self._h, C.byref(rays), n, occ.ctypes.data))
        return occ.astype(bool)

    # device-resident variants (raw pointers, e.g. torch tensors' data_ptr()) used by bench.py
    def trace_closest_device(self, ptrs7, n, t_ptr, prim_ptr, u_ptr=None, v_ptr=None, skip_ptr=None, nodes_ptr=None, prims_ptr=None):
        """nodes_ptr and prims_ptr (both or neither): n uint32 each, the per-ray node / primitive-test counters (rrt_hits::nodes_visited, prims_tested)."""
        rays = A.Rays(A.RRT_MEM_DEVICE, self.precision, *ptrs7, skip_ptr)
        hits = A.Hits(A.RRT_MEM_DEVICE, self.precision, t_ptr, prim_ptr, u_ptr, v_ptr, nodes_ptr, prims_ptr)
        _check(A.lib().rrt_trace_closest(self._h, C.byref(rays), n, C.byref(hits)))

    def trace_any_device(self, ptrs7, n, occluded_ptr, skip_ptr=None):
        rays = A.Rays(A.RRT_MEM_DEVICE, self.precision, *ptrs7, skip_ptr)
        _check(A.lib().rrt_trace_any(self._h, C.byref(rays), n, occluded_ptr))

    def camera_samples(self, rect, s0, s1):
        x0, y0, x1, y1 = rect
        n = (x1 - x0) * (y1 - y0) * (s1 - s0)
        dims = np.zeros((n, 5)); rays = np.zeros((n, 6)); w = np.zeros(n)
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_camera_samples(self._h, r, s0, s1, dims.ctypes.data, rays.ctypes.data, w.ctypes.data))
        return dims, rays, w

    def sampler_values(self, pixel, sample_num, first, count):
        """rrt_sampler_values: what the kernels' sampler draws for the streams (pixel, sample_num) with the counter at first .. first + count - 1.
        pixel (n, 2) of (x, y) or (n,) packed y << 16 | x; sample_num (n,) in 0 .. nsamp-1. Returns index (n,) uint64, v1 (n, count) and
        v2 (n, count, 2) float64."""
        pixel = np.asarray(pixel)
        if pixel.ndim == 2:
            pixel = (pixel[:, 1].astype(np.uint32) << 16) | pixel[:, 0].astype(np.uint32)
        pixel = np.ascontiguousarray(pixel, np.uint32); sample_num = np.ascontiguousarray(sample_num, np.uint32)
        n = len(sample_num)
        assert pixel.shape == (n,)
        index = np.zeros(n, np.uint64); v1 = np.zeros((n, max(count, 0))); v2 = np.zeros((n, max(count, 0), 2))
        _check(A.lib().rrt_sampler_values(self._h, pixel.ctypes.data, sample_num.ctypes.data, n, first, count, index.ctypes.data, v1.ctypes.data, v2.ctypes.data))
        return index, v1, v2

    # SamplerIntegrator::si_render (integrator/mod.rs:48) over a pixel rect; returns (H, W, 4) XYZ+weight film
    def render(self, rect=None, film=None, stats=False):
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        if film is None:
            film = np.zeros((H, W, 4), self.dtype)
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_rect(self._h, r, film.ctypes.data, A.RRT_MEM_HOST, C.byref(st) if stats else None))
        return (film, st) if stats else film

    # radiance along caller-supplied rays (rrt_radiance, rrt_render_rays)
    def _ray_samples(self, o, d, weight, diffs, pixel=None, sample_num=None):
        """rrt_ray_samples over host arrays: o, d (n, 3); weight (n,) or None; diffs None or (rxo, rxd, ryo, ryd), (n, 3) each. Returns the
        struct and the arrays it points into (keep them alive for the call)."""
        o = np.asarray(o); d = np.asarray(d)
        keep = [np.ascontiguousarray(a, self.dtype) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2])]
        rs = A.RaySamples(A.RRT_MEM_HOST, self.precision, *[a.ctypes.data for a in keep])
        if weight is not None:
            keep.append(np.ascontiguousarray(weight, self.dtype))
            rs.weight = keep[-1].ctypes.data
        if diffs is not None:
            for name, a in zip(("rxo", "rxd", "ryo", "ryd"), diffs):
                cols = [np.ascontiguousarray(np.asarray(a)[:, k], self.dtype) for k in range(3)]
                keep += cols
                setattr(rs, name, (C.c_void_p * 3)(*[c.ctypes.data for c in cols]))
        if pixel is not None:
            pixel = np.asarray(pixel)
            if pixel.ndim == 2:   # (n, 2) of (x, y) -> y << 16 | x
                pixel = (pixel[:, 1].astype(np.uint32) << 16) | pixel[:, 0].astype(np.uint32)
            keep += [np.ascontiguousarray(pixel, np.uint32), np.ascontiguousarray(sample_num, np.uint32)]
            rs.pixel, rs.sample_num = keep[-2].ctypes.data, keep[-1].ctypes.data
        return rs, keep

    def radiance(self, o, d, pixel, sample_num, weight=None, diffs=None, out=None):
        """Li of the scene's integrator along each ray (rrt_radiance): o, d (n, 3) host arrays, d unit length; pixel (n, 2) of (x, y) or (n,)
        packed y << 16 | x, and sample_num (n,) in 1 .. nsamp-1 name the sampler stream of each ray; weight 0 = dead ray (result 0).
        Returns (n, 3) RGB, a view of `out` where a C-contiguous (>= n, 4) array of the renderer's dtype is given to write into."""
        n = len(np.asarray(sample_num))
        rs, keep = self._ray_samples(o, d, weight, diffs, pixel, sample_num)
        if out is None:
            out = np.zeros((n, 4), self.dtype)
        assert out.dtype == self.dtype and out.flags.c_contiguous and out.shape[0] >= n and out.shape[1:] == (4,)
        _check(A.lib().rrt_radiance(self._h, C.byref(rs), n, out.ctypes.data))
        return out[:n, :3]

    def render_rays(self, rect, s0, s1, rays, weight, p_film, film=None, stats=False, diffs=None):
        """rrt_render_rays: the frame's film for sample numbers [s0, s1) of the rect's pixels, the camera replaced by the caller's samples in
        camera_samples' layout [pixel][sample]: rays (n, 6) origin + unit direction, weight (n,) or None (= 1), p_film (n, 2) raster
        coordinates. Returns the (H, W, 4) XYZ + weight film (+= into `film` where given)."""
        W, H = self.scene.resolution
        if film is None:
            film = np.zeros((H, W, 4), self.dtype)
        rays = np.asarray(rays)
        rs, keep = self._ray_samples(rays[:, :3], rays[:, 3:6], weight, diffs)
        pf = np.ascontiguousarray(p_film, self.dtype)
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_rays(self._h, r, s0, s1, C.byref(rs), pf.ctypes.data, film.ctypes.data, A.RRT_MEM_HOST, C.byref(st) if stats else None))
        return (film, st) if stats else film

    def radiance_device(self, ptrs6, pixel_ptr, sample_num_ptr, n, rgb4_ptr, weight_ptr=None, diff_ptrs12=None):
        """rrt_radiance on device-resident arrays (raw pointers): ptrs6 = ox, oy, oz, dx, dy, dz; rgb4_ptr: n * 4 values, device memory."""
        rs = A.RaySamples(A.RRT_MEM_DEVICE, self.precision, *ptrs6, weight_ptr)
        if diff_ptrs12 is not None:
            for k, name in enumerate(("rxo", "rxd", "ryo", "ryd")):
                setattr(rs, name, (C.c_void_p * 3)(*diff_ptrs12[3 * k:3 * k + 3]))
        rs.pixel, rs.sample_num = pixel_ptr, sample_num_ptr
        _check(A.lib().rrt_radiance(self._h, C.byref(rs), n, rgb4_ptr))

    # irradiance and SH probes at caller-supplied points (rrt_irradiance, rrt_irradiance_rays)
    _IRR_MODES = {"cosine": A.RRT_IRR_COSINE, "sphere": A.RRT_IRR_SPHERE}

    def _irr_params(self, mode, offset):
        if mode not in self._IRR_MODES:
            raise ValueError(f'irradiance: mode is "cosine" or "sphere", not {mode!r}')
        return A.IrrParams(self._IRR_MODES[mode], 0, float(offset))

    def _points(self, p, n, pixel):
        """rrt_points over host arrays: p (m, 3); n (m, 3) or None; pixel None, (m, 2) of (x, y) or (m,) packed y << 16 | x. Returns the struct and
        the arrays it points into (keep them alive for the call)."""
        p = np.asarray(p)
        keep = [np.ascontiguousarray(p[:, k], self.dtype) for k in range(3)]
        if n is not None:
            n = np.asarray(n)
            keep += [np.ascontiguousarray(n[:, k], self.dtype) for k in range(3)]
        pts = A.Points(A.RRT_MEM_HOST, self.precision, *[a.ctypes.data for a in keep])
        if pixel is not None:
            pixel = np.asarray(pixel)
            if pixel.ndim == 2:
                pixel = (pixel[:, 1].astype(np.uint32) << 16) | pixel[:, 0].astype(np.uint32)
            keep.append(np.ascontiguousarray(pixel, np.uint32))
            pts.pixel = keep[-1].ctypes.data
        return pts, keep

    def _draw_range(self, s0, s1):
        return int(s0), int(self.scene.desc.sampler.samples_per_pixel if s1 is None else s1)

    def irradiance(self, p, n, s0=1, s1=None, pixel=None, offset=0.0, mode="cosine", sums=None, sh=None):
        """rrt_irradiance over host arrays: the sums of draws [s0, s1) (s1 None = nsamp) of the scene's integrator at points p (m, 3) with normals
        n (m, 3; None in sphere mode = the z axis), rays made on the device. mode "cosine": returns sums (m, 4) = {sum L.rgb, sum y^2}; mode
        "sphere": returns (sums, sh) with sh (m, 27) where sh is True or an array. `sums` / `sh` arrays of the renderer's dtype are added to
        (+=, draw ranges can be split over calls); see resolve_irradiance and resolve_sh for the scaling."""
        m = len(np.asarray(p))
        s0, s1 = self._draw_range(s0, s1)
        pts, keep = self._points(p, n, pixel)
        prm = self._irr_params(mode, offset)
        if sums is None:
            sums = np.zeros((m, 4), self.dtype)
        if sh is True:
            sh = np.zeros((m, 27), self.dtype)
        assert sums.dtype == self.dtype and sums.flags.c_contiguous and sums.shape == (m, 4)
        assert sh is None or (sh.dtype == self.dtype and sh.flags.c_contiguous and sh.shape == (m, 27))
        _check(A.lib().rrt_irradiance(self._h, C.byref(pts), m, s0, s1, C.byref(prm), sums.ctypes.data, None if sh is None else sh.ctypes.data))
        return sums if sh is None else (sums, sh)

    def irradiance_rays(self, p, n, s0=1, s1=None, pixel=None, offset=0.0, mode="cosine"):
        """rrt_irradiance_rays: the rays rrt_irradiance traces, (m, s1 - s0, 6) origin + unit direction in the renderer's dtype; a dead draw is
        six zeros."""
        m = len(np.asarray(p))
        s0, s1 = self._draw_range(s0, s1)
        pts, keep = self._points(p, n, pixel)
        prm = self._irr_params(mode, offset)
        od = np.zeros((m, max(0, s1 - s0), 6), self.dtype)
        _check(A.lib().rrt_irradiance_rays(self._h, C.byref(pts), m, s0, s1, C.byref(prm), od.ctypes.data))
        return od

    def irradiance_device(self, p_ptrs3, n_ptrs3, m, s0, s1, sums_ptr, sh_ptr=None, pixel_ptr=None, offset=0.0, mode="cosine"):
        """rrt_irradiance on device-resident arrays (raw pointers): p_ptrs3 = px, py, pz; n_ptrs3 = nx, ny, nz or None; sums_ptr: m * 4 values,
        sh_ptr: m * 27 values or None; both are added to."""
        pts = A.Points(A.RRT_MEM_DEVICE, self.precision, *p_ptrs3, *(n_ptrs3 if n_ptrs3 is not None else (None, None, None)), pixel_ptr)
        prm = self._irr_params(mode, offset)
        _check(A.lib().rrt_irradiance(self._h, C.byref(pts), m, s0, s1, C.byref(prm), sums_ptr, sh_ptr))

    # surface records and lightmap sites (rrt_surface_rays, rrt_surface_at, rrt_atlas_sites)
    SURFACE_FIELDS = tuple(A.SURFACE_GROUPS)

    def _surface_out(self, m, fields):
        """rrt_surface over fresh host arrays for the groups `fields` (names of A.SURFACE_GROUPS: "p", "n", "s", "uv", "rho", "t", "prim"); returns
        the struct and {member name: array}."""
        out = A.Surface(A.RRT_MEM_HOST, self.precision)
        arrs = {}
        for f in fields:
            if f not in A.SURFACE_GROUPS:
                raise ValueError(f"surface: fields are {', '.join(A.SURFACE_GROUPS)}, not {f!r}")
            for k in A.SURFACE_GROUPS[f]:
                arrs[k] = np.zeros(m, np.int32 if f == "prim" else self.dtype)
                setattr(out, k, arrs[k].ctypes.data)
        return out, arrs

    @staticmethod
    def _surface_dict(arrs):
        """{member: (m,)} -> dict(p (m, 3), n, s, uv (m, 2), rho (m, 3), t (m,), prim, material) of the groups that were produced"""
        res = {}
        for f, members in A.SURFACE_GROUPS.items():
            if members[0] not in arrs:
                continue
            if f == "prim":
                res["prim"], res["material"] = arrs["prim"], arrs["material"]
            elif f == "t":
                res["t"] = arrs["t"]
            else:
                res[f] = np.stack([arrs[k] for k in members], 1)
        return res

    def surface(self, o, d, tmax=None, skip_prim=None, fields=SURFACE_FIELDS):
        """rrt_surface_rays over host arrays: the rays o, d (m, 3), tmax (m,; None = inf), skip_prim (m,) or None, traced as trace_closest traces them;
        returns a dict of the record groups `fields`: p, n, s, rho (m, 3), uv (m, 2), t (m,), prim and material (m,) int32 (-1 = a miss: a dead
        record, zeros everywhere else but t)."""
        o = np.asarray(o); d = np.asarray(d)
        m = len(o)
        tmax = np.full(m, np.inf) if tmax is None else tmax
        soa = [np.ascontiguousarray(a, self.dtype) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
        skip = None if skip_prim is None else np.ascontiguousarray(skip_prim, np.int32)
        rays = A.Rays(A.RRT_MEM_HOST, self.precision, *[a.ctypes.data for a in soa], None if skip is None else skip.ctypes.data)
        out, arrs = self._surface_out(m, fields)
        _check(A.lib().rrt_surface_rays(self._h, C.byref(rays), m, C.byref(out)))
        return self._surface_dict(arrs)

    def surface_at(self, prim, b1, b2, fields=SURFACE_FIELDS):
        """rrt_surface_at over host arrays: the records of the sites (prim, b1, b2) - prim as rrt_hits.prim (-1 = no site: a dead record), b1, b2 the
        barycentrics of rrt_hits.u / .v. Returns a dict as surface() does, t = 0."""
        prim = np.ascontiguousarray(prim, np.int32)
        b1 = np.ascontiguousarray(b1, self.dtype); b2 = np.ascontiguousarray(b2, self.dtype)
        m = len(prim)
        sites = A.Sites(A.RRT_MEM_HOST, self.precision, prim.ctypes.data, b1.ctypes.data, b2.ctypes.data)
        out, arrs = self._surface_out(m, fields)
        _check(A.lib().rrt_surface_at(self._h, C.byref(sites), m, C.byref(out)))
        return self._surface_dict(arrs)

    def atlas_sites(self, res, prims=None):
        """rrt_atlas_sites into host arrays: res = (aw, ah); prims None = every triangle entry of prim_order, else the candidate list in the caller's
        order (the first covering entry owns a texel). Returns dict(prim (ah, aw) int32 with -1 = uncovered, b1, b2 (ah, aw), covered: int)."""
        aw, ah = int(res[0]), int(res[1])
        n = max(0, aw) * max(0, ah)
        prim = np.zeros(max(n, 1), np.int32); b1 = np.zeros(max(n, 1), self.dtype); b2 = np.zeros(max(n, 1), self.dtype)
        lst = None if prims is None else np.ascontiguousarray(prims, np.int32)
        covered = C.c_uint64(0)
        _check(A.lib().rrt_atlas_sites(self._h, aw, ah, None if lst is None else lst.ctypes.data, 0 if lst is None else len(lst), A.RRT_MEM_HOST,
                                       prim.ctypes.data, b1.ctypes.data, b2.ctypes.data, C.byref(covered)))
        return dict(prim=prim[:n].reshape(ah, aw), b1=b1[:n].reshape(ah, aw), b2=b2[:n].reshape(ah, aw), covered=int(covered.value))

    def _surface_device(self, ptrs):
        """rrt_surface over device arrays: ptrs = {member name of rrt_surface: raw pointer}; members left out are NULL (their group is not produced)"""
        out = A.Surface(A.RRT_MEM_DEVICE, self.precision)
        for k, v in ptrs.items():
            setattr(out, k, v)
        return out

    def surface_device(self, ptrs7, m, out_ptrs, skip_ptr=None):
        """rrt_surface_rays on device-resident arrays (raw pointers): ptrs7 = ox, oy, oz, dx, dy, dz, tmax; out_ptrs = {member name of rrt_surface
        ("px", ..., "rho_b", "t", "prim", "material"): pointer to m values}, whole groups."""
        rays = A.Rays(A.RRT_MEM_DEVICE, self.precision, *ptrs7, skip_ptr)
        out = self._surface_device(out_ptrs)
        _check(A.lib().rrt_surface_rays(self._h, C.byref(rays), m, C.byref(out)))

    def surface_at_device(self, prim_ptr, b1_ptr, b2_ptr, m, out_ptrs):
        """rrt_surface_at on device-resident arrays (raw pointers); out_ptrs as surface_device takes them."""
        sites = A.Sites(A.RRT_MEM_DEVICE, self.precision, prim_ptr, b1_ptr, b2_ptr)
        out = self._surface_device(out_ptrs)
        _check(A.lib().rrt_surface_at(self._h, C.byref(sites), m, C.byref(out)))

    def atlas_sites_device(self, res, prim_ptr, b1_ptr, b2_ptr, prims=None):
        """rrt_atlas_sites into device arrays of aw * ah values each (raw pointers; the candidate list stays a host array); returns the covered count."""
        lst = None if prims is None else np.ascontiguousarray(prims, np.int32)
        covered = C.c_uint64(0)
        _check(A.lib().rrt_atlas_sites(self._h, int(res[0]), int(res[1]), None if lst is None else lst.ctypes.data, 0 if lst is None else len(lst), A.RRT_MEM_DEVICE,
                                       prim_ptr, b1_ptr, b2_ptr, C.byref(covered)))
        return int(covered.value)

    def bake_irradiance(self, res, prims=None, s0=1, s1=None, offset=0.0, flip=False):
        """A lightmap: atlas_sites -> surface_at -> irradiance composed over host arrays. res = (aw, ah), prims as atlas_sites takes it, draws
        [s0, s1) (s1 None = nsamp), offset along the (flipped) normal. The record's normal is not turned towards anything: flip=True lights
        the -n side. Returns dict(E (ah, aw, 3), stderr (ah, aw), covered (ah, aw) bool) through resolve_irradiance; uncovered texels are 0."""
        aw, ah = int(res[0]), int(res[1])
        sites = self.atlas_sites((aw, ah), prims)
        rec = self.surface_at(sites["prim"].ravel(), sites["b1"].ravel(), sites["b2"].ravel(), fields=("p", "n"))
        s0, s1 = self._draw_range(s0, s1)
        sums = self.irradiance(rec["p"], -rec["n"] if flip else rec["n"], s0, s1, offset=offset)
        out = resolve_irradiance(sums, s1 - s0)
        return dict(E=out["E"].reshape(ah, aw, 3), stderr=out["stderr"].reshape(ah, aw), covered=sites["prim"] >= 0)

    # nearest-surface point queries (rrt_nearest)
    def nearest(self, p, max_dist=np.inf):
        """rrt_nearest over host arrays: p (m, 3) points; returns dict(prim (m,) int32 - index into prim_order as trace_closest's prim, -1 = nothing
        within max_dist -, b1, b2 (m,) barycentrics, dist (m,)). (prim, b1, b2) go into surface_at as they are. Spheres are not candidates."""
        p = np.asarray(p)
        m = len(p)
        cols = [np.ascontiguousarray(p[:, k], self.dtype) for k in range(3)]
        pts = A.Points(A.RRT_MEM_HOST, self.precision, *[c.ctypes.data for c in cols], None, None, None, None)
        prim = np.zeros(m, np.int32)
        b1 = np.zeros(m, self.dtype); b2 = np.zeros(m, self.dtype); dist = np.zeros(m, self.dtype)
        out = A.NearestOut(A.RRT_MEM_HOST, self.precision, prim.ctypes.data, b1.ctypes.data, b2.ctypes.data, dist.ctypes.data)
        _check(A.lib().rrt_nearest(self._h, C.byref(pts), m, float(max_dist), C.byref(out)))
        return dict(prim=prim, b1=b1, b2=b2, dist=dist)

    def nearest_device(self, ptrs, n, max_dist=np.inf):
        """rrt_nearest on device-resident arrays (raw pointers): ptrs = {"px", "py", "pz", "prim", "b1", "b2" and optionally "dist": pointer to n values}."""
        pts = A.Points(A.RRT_MEM_DEVICE, self.precision, ptrs["px"], ptrs["py"], ptrs["pz"], None, None, None, None)
        out = A.NearestOut(A.RRT_MEM_DEVICE, self.precision, ptrs["prim"], ptrs["b1"], ptrs["b2"], ptrs.get("dist"))
        _check(A.lib().rrt_nearest(self._h, C.byref(pts), n, float(max_dist), C.byref(out)))

    def nearest_records(self, p, max_dist=np.inf, fields=SURFACE_FIELDS):
        """nearest composed with surface_at: the surface records (dict as surface_at returns it) of the sites nearest to the points p, plus
        "dist", "b1" and "b2"; a point with nothing within max_dist gets the dead record (prim = -1)."""
        near = self.nearest(p, max_dist)
        rec = self.surface_at(near["prim"], near["b1"], near["b2"], fields=fields)
        rec.update(dist=near["dist"], b1=near["b1"], b2=near["b2"])
        rec.setdefault("prim", near["prim"])
        return rec

    def distance_field(self, lo, hi, res, max_dist=np.inf, signed=False):
        """The distances at the cell centres of a (rx, ry, rz) grid over the box lo .. hi, as an array (rz, ry, rx): nearest() over points built in
        numpy; cells with nothing within max_dist hold max_dist. signed=True negates the distances of the cells inside() finds inside (closed
        surfaces only)."""
        lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64)
        rx, ry, rz = (int(r) for r in res)
        ax = [lo[k] + (np.arange(r) + 0.5) * ((hi[k] - lo[k]) / r) for k, r in enumerate((rx, ry, rz))]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        dist = self.nearest(p, max_dist)["dist"]
        if signed:
            dist = np.where(self.inside(p), -dist, dist)
        return dist.reshape(rz, ry, rx)

    # all hits along a ray, in order (rrt_trace_all)
    def trace_all(self, o, d, tmax, k=8, count=True, skip_prim=None):
        """rrt_trace_all over host arrays: o, d (m, 3), tmax (m,); returns dict(t, prim, b1, b2 of shape (k, m) - slot s of ray i at [s, i], the accepted
        triangle hits sorted by (t, prim), prim = index into prim_order as trace_closest's prim, -1 / tmax / 0 / 0 in the empty slots - and, with
        count=True, count (m,) uint32: ALL accepted hits of the ray, not clipped at k). Plane s of (prim, b1, b2) goes into surface_at as it is.
        k = 0 is the count-only form. Spheres are not candidates."""
        o = np.asarray(o); d = np.asarray(d)
        m = len(tmax)
        soa = [np.ascontiguousarray(a, self.dtype) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
        skip = None if skip_prim is None else np.ascontiguousarray(skip_prim, np.int32)
        rays = A.Rays(A.RRT_MEM_HOST, self.precision, *[a.ctypes.data for a in soa], None if skip is None else skip.ctypes.data)
        k = int(k)
        t = np.zeros((k, m), self.dtype); b1 = np.zeros((k, m), self.dtype); b2 = np.zeros((k, m), self.dtype)
        prim = np.zeros((k, m), np.int32)
        cnt = np.zeros(m, np.uint32) if count else None
        slots = [a.ctypes.data if k > 0 else None for a in (t, prim, b1, b2)]
        out = A.MultiHits(A.RRT_MEM_HOST, self.precision, k, 0, *slots, None if cnt is None else cnt.ctypes.data)
        _check(A.lib().rrt_trace_all(self._h, C.byref(rays), m, C.byref(out)))
        res = dict(t=t, prim=prim, b1=b1, b2=b2)
        if count:
            res["count"] = cnt
        return res

    def trace_all_device(self, ptrs7, n, out_ptrs, k, skip_ptr=None):
        """rrt_trace_all on device-resident arrays (raw pointers): ptrs7 = ox, oy, oz, dx, dy, dz, tmax (n values each); out_ptrs = {"t", "prim" and
        optionally "b1" and "b2": pointer to k * n values, slot-major; optionally "count": pointer to n uint32}."""
        rays = A.Rays(A.RRT_MEM_DEVICE, self.precision, *ptrs7, skip_ptr)
        out = A.MultiHits(A.RRT_MEM_DEVICE, self.precision, int(k), 0, out_ptrs.get("t"), out_ptrs.get("prim"), out_ptrs.get("b1"), out_ptrs.get("b2"), out_ptrs.get("count"))
        _check(A.lib().rrt_trace_all(self._h, C.byref(rays), n, C.byref(out)))

    # mutual visibility of two point sets as a packed bit matrix (rrt_visibility)
    @staticmethod
    def _vis_params(offset_a, offset_b, facing_a, facing_b, directions, pairs, skip_a_ptr, skip_b_ptr):
        flags = (A.RRT_VIS_FACING_A if facing_a else 0) | (A.RRT_VIS_FACING_B if facing_b else 0)
        return A.VisParams(A.RRT_VIS_PAIRS if pairs else A.RRT_VIS_MATRIX, A.RRT_VIS_DIRECTIONS if directions else A.RRT_VIS_POINTS, flags, 0, float(offset_a), float(offset_b),
                           skip_a_ptr, skip_b_ptr)

    def visibility(self, a, b, na=None, nb=None, offset_a=0, offset_b=0, facing_a=False, facing_b=False, directions=False, pairs=False, skip_a=None, skip_b=None, count=True):
        """rrt_visibility over host arrays: points a (n_a, 3) and b (n_b, 3; with directions=True the directions themselves), optional normals na, nb
        of the same shapes - the ends are moved offset_a / offset_b along the unit normals, facing_a / facing_b require the segment to leave a's side
        and arrive on b's -, skip_a / skip_b one entry of prim_order per point to leave out (-1 = none). Returns dict(bits (n_a, words) uint64,
        words = (n_b + 63) // 64, bit j & 63 of word j // 64 of row i = a_i sees b_j; count (n_a,) uint32 = the set bits of each row, with
        count=True); pairs=True (n_b == n_a): bits (words,) for the pairs (i, i) and no count. unpack_visibility() turns bits into a bool array.
        Blocked = a triangle accepted by trace_all's rules lies on the segment; spheres are not candidates."""
        n_a, n_b = len(np.asarray(a)), len(np.asarray(b))
        pa, keep_a = self._points(a, na, None)
        pb, keep_b = self._points(b, nb, None)
        sa = None if skip_a is None else np.ascontiguousarray(skip_a, np.int32)
        sb = None if skip_b is None else np.ascontiguousarray(skip_b, np.int32)
        prm = self._vis_params(offset_a, offset_b, facing_a, facing_b, directions, pairs, None if sa is None else sa.ctypes.data, None if sb is None else sb.ctypes.data)
        bits = np.zeros((n_a + 63) // 64 if pairs else (n_a, (n_b + 63) // 64), np.uint64)
        cnt = np.zeros(n_a, np.uint32) if count and not pairs else None
        out = A.VisOut(A.RRT_MEM_HOST, 0, bits.ctypes.data, None if cnt is None else cnt.ctypes.data)
        _check(A.lib().rrt_visibility(self._h, C.byref(pa), n_a, C.byref(pb), n_b, C.byref(prm), C.byref(out)))
        return dict(bits=bits, count=cnt)

    def visibility_device(self, ptrs, n_a, n_b, offset_a=0, offset_b=0, facing_a=False, facing_b=False, directions=False, pairs=False):
        """rrt_visibility on device-resident arrays (raw pointers): ptrs = {"a": (px, py, pz), "b": (px, py, pz), "bits": pointer to the uint64 words,
        and optionally "na", "nb": (nx, ny, nz), "skip_a", "skip_b": int32 arrays, "count": n_a uint32}."""
        none3 = (None, None, None)
        pa = A.Points(A.RRT_MEM_DEVICE, self.precision, *ptrs["a"], *(ptrs.get("na") or none3), None)
        pb = A.Points(A.RRT_MEM_DEVICE, self.precision, *ptrs["b"], *(ptrs.get("nb") or none3), None)
        prm = self._vis_params(offset_a, offset_b, facing_a, facing_b, directions, pairs, ptrs.get("skip_a"), ptrs.get("skip_b"))
        out = A.VisOut(A.RRT_MEM_DEVICE, 0, ptrs["bits"], ptrs.get("count"))
        _check(A.lib().rrt_visibility(self._h, C.byref(pa), n_a, C.byref(pb), n_b, C.byref(prm), C.byref(out)))

    def sky_view(self, p, n, directions, offset=0.0):
        """The share of `directions` (m, 3) each point p (k, 3) with normal n sees unblocked and in front of its surface: visibility(directions=True,
        facing_a=True) count / m, as (k,) float64 - a sky-view factor for directions spread evenly over the sky, sun hours for sun positions."""
        directions = np.asarray(directions)
        return self.visibility(p, directions, na=n, offset_a=offset, facing_a=True, directions=True)["count"].astype(np.float64) / len(directions)

    # three fixed, mutually skew directions (no two parallel, none along an axis or a face diagonal of an axis-aligned mesh)
    INSIDE_DIRECTIONS = ((0.8164, 0.4082, 0.4083), (-0.3015, 0.9045, 0.3016), (0.2673, -0.5345, 0.8018))

    def inside(self, p):
        """Whether the points p (m, 3) lie inside the scene's closed triangle surfaces: the parity of trace_all's count (k = 0, unbounded rays) along
        INSIDE_DIRECTIONS, decided by majority - a ray through a shared edge or a vertex counts every triangle around it, which one vote absorbs.
        Returns (m,) bool."""
        p = np.asarray(p, np.float64)
        m = len(p)
        votes = np.zeros(m, np.int32)
        tmax = np.full(m, np.inf)
        for d in self.INSIDE_DIRECTIONS:
            votes += (self.trace_all(p, np.broadcast_to(np.asarray(d, np.float64), (m, 3)), tmax, k=0)["count"] & 1).astype(np.int32)
        return votes >= 2

    def thickness(self, o, d, tmax, k=A.RRT_MAX_HITS):
        """The length of the rays inside the scene's closed surfaces, in units of |d|: the sum of t[2j + 1] - t[2j] over the pairs of the first k hits
        (an unpaired last hit adds nothing). Returns (m,) in the handle's type."""
        hits = self.trace_all(o, d, tmax, k=k)
        held = np.minimum(hits["count"], k)
        total = np.zeros(len(held), self.dtype)
        for j in range(k // 2):
            with np.errstate(invalid="ignore"):      # (empty slots hold tmax: inf - inf where nothing is held)
                total += np.where(held >= 2 * j + 2, hits["t"][2 * j + 1] - hits["t"][2 * j], 0)
        return total

    def render_rays_device(self, rect, s0, s1, ptrs6, weight_ptr, p_film_ptr, film_ptr, stats=True):
        """rrt_render_rays on device-resident samples into a device film (+=)."""
        rs = A.RaySamples(A.RRT_MEM_DEVICE, self.precision, *ptrs6, weight_ptr)
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_rays(self._h, r, s0, s1, C.byref(rs), p_film_ptr, film_ptr, A.RRT_MEM_DEVICE, C.byref(st) if stats else None))
        return st

    def render_bands_device(self, rank, world, film_ptr, stats=True):
        """This rank's interleaved 16-row bands (partition.py) into a device film (+=)."""
        st = A.RenderStats()
        _check(A.lib().rrt_render_bands(self._h, rank, world, film_ptr, A.RRT_MEM_DEVICE, C.byref(st) if stats else None))
        return st

    def render_bands_begin(self, rank, world, film_ptr):
        """Enqueue render_bands_device and return (frames in flight, see rrt_render_bands_begin); pair with render_end()."""
        _check(A.lib().rrt_render_bands_begin(self._h, rank, world, film_ptr))

    def render_end(self, stats=False):
        if not stats:
            _check(A.lib().rrt_render_end(self._h))
            return None
        st = A.RenderStats()
        _check(A.lib().rrt_render_end_stats(self._h, C.byref(st)))
        return st

    def render_bands(self, rank, world, film=None, stats=False):
        W, H = self.scene.resolution
        if film is None:
            film = np.zeros((H, W, 4), self.dtype)
        st = A.RenderStats()
        _check(A.lib().rrt_render_bands(self._h, rank, world, film.ctypes.data, A.RRT_MEM_HOST, C.byref(st) if stats else None))
        return (film, st) if stats else film

    # first-hit feature buffers (rrt_render_aov): the raw filtered sums, (H, W, 4) each; resolve_aov() divides them out
    # follow > 0 (rrt_render_aov_follow): the planes of the first non-specular surface along chains of up to `follow` mirror / smooth-glass bounces
    def render_aov(self, rect=None, max_samples=0, rank=0, world=1, planes=("albedo", "normal", "depth"), follow=0):
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        out = {k: np.zeros((H, W, 4), self.dtype) for k in planes}
        ptr = {k: (out[k].ctypes.data if k in out else None) for k in ("albedo", "normal", "depth")}
        aov = A.Aov(A.RRT_MEM_HOST, self.precision, ptr["albedo"], ptr["normal"], ptr["depth"])
        r = (C.c_int32 * 4)(*rect)
        if follow > 0:
            _check(A.lib().rrt_render_aov_follow(self._h, r, rank, world, max_samples, follow, C.byref(aov)))
        else:
            _check(A.lib().rrt_render_aov(self._h, r, rank, world, max_samples, C.byref(aov)))
        return out

    # ambient occlusion and bent normals (rrt_render_ao): the raw filtered sums, (H, W, 4) each; resolve_ao() divides them out
    def render_ao(self, rect=None, max_samples=0, rank=0, world=1, n_samples=None, cos_sample=None, planes=("ao", "bent")):
        """n_samples / cos_sample: None = rrt_ao_defaults (the scene's own where its integrator is AO, else 64 / cosine)."""
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        out = {k: np.zeros((H, W, 4), self.dtype) for k in planes}
        ptr = {k: (out[k].ctypes.data if k in out else None) for k in ("ao", "bent")}
        ao = A.Ao(A.RRT_MEM_HOST, self.precision, ptr["ao"], ptr["bent"])
        prm = A.AoParams()
        A.lib().rrt_ao_defaults(self._h, C.byref(prm))
        if n_samples is not None: prm.n_samples = int(n_samples)
        if cos_sample is not None: prm.cos_sample = 1 if cos_sample else 0
        _check(A.lib().rrt_render_ao(self._h, (C.c_int32 * 4)(*rect), rank, world, max_samples, C.byref(prm), C.byref(ao)))
        return out

    # rrt_render_moments: the frame of render() / render_bands() and the sample-variance plane {S1, S2, S0, S3} beside it; resolve_moments() divides it out
    def render_moments(self, rect=None, rank=0, world=1, film=None, moments=None, stats=False):
        """-> (film, moments[, stats]): both (H, W, 4) host arrays of the handle's precision, added to (+=) where given."""
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        if film is None:
            film = np.zeros((H, W, 4), self.dtype)
        if moments is None:
            moments = np.zeros((H, W, 4), self.dtype)
        for a in (film, moments):
            if a.dtype != self.dtype or a.shape != (H, W, 4) or not a.flags.c_contiguous:
                raise ValueError("render_moments: film and moments are C-contiguous (H, W, 4) arrays of the handle's precision")
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_moments(self._h, r, rank, world, film.ctypes.data, moments.ctypes.data, A.RRT_MEM_HOST, C.byref(st) if stats else None))
        return (film, moments, st) if stats else (film, moments)

    def render_moments_device(self, rect, film_ptr, moments_ptr, rank=0, world=1, stats=True):
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_moments(self._h, r, rank, world, film_ptr, moments_ptr, A.RRT_MEM_DEVICE, C.byref(st) if stats else None))
        return st

    # rrt_render_passes: the frame of render() / render_bands() and, beside it, one film per pass of the Path integrator's next-event terms
    @staticmethod
    def _pass_table(passes, film_ptrs):
        tab = (A.Pass * max(1, len(passes)))()
        for k, (p, ptr) in enumerate(zip(passes, film_ptrs)):
            groups, lo, hi = p
            tab[k] = A.Pass(int(groups) & 0xFFFFFFFF, int(lo), int(hi), ptr)
        return tab

    @staticmethod
    def _light_groups(light_group):
        if light_group is None:
            return None, None
        lg = np.ascontiguousarray(light_group, np.uint8)
        return lg, lg.ctypes.data

    def render_passes(self, passes, light_group=None, rect=None, rank=0, world=1, film=True, stats=False):
        """passes: a list of (groups, bounce_lo, bounce_hi) - a bit mask of light groups and the path vertices lo <= b < hi (hi <= 0: no upper end);
        light_group: one group (< 32) per light, None = light i is in group min(i, 31). film: True = a new frame film, None / False = none, or an
        (H, W, 4) array added to (+=). -> (film or None, [pass films][, stats]): (H, W, 4) host arrays of the handle's precision."""
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        if film is True:
            film = np.zeros((H, W, 4), self.dtype)
        elif film is False:
            film = None
        if film is not None and (film.dtype != self.dtype or film.shape != (H, W, 4) or not film.flags.c_contiguous):
            raise ValueError("render_passes: film is a C-contiguous (H, W, 4) array of the handle's precision")
        films = [np.zeros((H, W, 4), self.dtype) for _ in passes]
        tab = self._pass_table(passes, [f.ctypes.data for f in films])
        lg, lg_ptr = self._light_groups(light_group)
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_passes(self._h, r, rank, world, lg_ptr, tab, len(passes), film.ctypes.data if film is not None else None, A.RRT_MEM_HOST,
                                         C.byref(st) if stats else None))
        return (film, films, st) if stats else (film, films)

    def render_passes_device(self, rect, passes, film_ptrs, light_group=None, film_ptr=None, rank=0, world=1, stats=True):
        """render_passes into device films: film_ptrs[k] is pass k's film (+=), film_ptr the frame's or None."""
        tab = self._pass_table(passes, film_ptrs)
        lg, lg_ptr = self._light_groups(light_group)
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_passes(self._h, r, rank, world, lg_ptr, tab, len(passes), film_ptr, A.RRT_MEM_DEVICE, C.byref(st) if stats else None))
        return st

    @staticmethod
    def _gains(gains, n):
        """(n, 3) doubles from one number for all films, one number per film, or one RGB triple per film."""
        g = np.asarray(gains, np.float64)
        if g.ndim == 1: g = g[:, None]
        return np.ascontiguousarray(np.broadcast_to(g, (n, 3)))

    # rrt_combine_passes: relighting - sum_k rgb_to_xyz(gains[k] * xyz_to_rgb(films[k])), the weight channel films[0]'s
    def combine_passes(self, films, gains, out=None):
        """films: (H, W, 4) host arrays as render_passes returns them; gains: one RGB triple (or one number) per film. -> the combined film."""
        W, H = self.scene.resolution
        for f in films:
            if f.dtype != self.dtype or f.shape != (H, W, 4) or not f.flags.c_contiguous:
                raise ValueError("combine_passes: films are C-contiguous (H, W, 4) arrays of the handle's precision")
        if out is None:
            out = np.empty((H, W, 4), self.dtype)
        g = self._gains(gains, len(films))
        ptrs = (C.c_void_p * max(1, len(films)))(*[f.ctypes.data for f in films])
        _check(A.lib().rrt_combine_passes(self._h, ptrs, g.ctypes.data_as(C.POINTER(C.c_double)), len(films), out.ctypes.data, A.RRT_MEM_HOST))
        return out

    def combine_passes_device(self, film_ptrs, gains, out_ptr):
        g = self._gains(gains, len(film_ptrs))
        ptrs = (C.c_void_p * max(1, len(film_ptrs)))(*film_ptrs)
        _check(A.lib().rrt_combine_passes(self._h, ptrs, g.ctypes.data_as(C.POINTER(C.c_double)), len(film_ptrs), out_ptr, A.RRT_MEM_DEVICE))

    # rrt_render_mattes: per pixel the K best-covered ids of the camera rays' first hits; resolve_mattes() divides the coverages out
    def _prim_id_arg(self, ids):
        """None (material index + 1), a Scene.prim_ids key, or one id per entry of rrt_scene_desc.prims -> (array kept alive, pointer, count)"""
        if ids is None:
            return None, None, 0
        arr = self.scene.prim_ids(ids) if isinstance(ids, str) else np.ascontiguousarray(ids, np.uint32)
        return arr, arr.ctypes.data, arr.size

    def render_mattes(self, ids=None, slots=6, rect=None, rank=0, world=1, max_samples=0, mattes=None):
        """-> dict(ids (H, W, K) uint32, coverage (H, W, K), weight (H, W, 4)): host arrays, the table ranked by coverage. mattes: such a dict,
        continued in place (its K is the table's)."""
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        if mattes is None:
            mattes = dict(ids=np.zeros((H, W, slots), np.uint32), coverage=np.zeros((H, W, slots), self.dtype), weight=np.zeros((H, W, 4), self.dtype))
        m = self._mattes_struct(mattes, "render_mattes")
        arr, ptr, n = self._prim_id_arg(ids)
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_mattes(self._h, r, rank, world, max_samples, ptr, n, C.byref(m)))
        return mattes

    def _mattes_struct(self, mattes, who):
        W, H = self.scene.resolution
        i, c, w = mattes["ids"], mattes["coverage"], mattes["weight"]
        K = i.shape[-1] if i.ndim == 3 else 0
        ok = (i.dtype == np.uint32 and i.shape == (H, W, K) and c.dtype == self.dtype and c.shape == (H, W, K) and w.dtype == self.dtype and w.shape == (H, W, 4)
              and i.flags.c_contiguous and c.flags.c_contiguous and w.flags.c_contiguous)
        if not ok:
            raise ValueError(f"{who}: ids (H, W, K) uint32, coverage (H, W, K) and weight (H, W, 4) of the handle's precision, all C-contiguous")
        return A.Mattes(A.RRT_MEM_HOST, self.precision, K, 0, i.ctypes.data, c.ctypes.data, w.ctypes.data)

    def render_mattes_device(self, rect, ids_ptr, coverage_ptr, weight_ptr, slots, ids=None, rank=0, world=1, max_samples=0):
        """The same on device buffers (raw pointers of the W*H*slots ids, W*H*slots coverages and W*H*4 weights), continued in place."""
        m = A.Mattes(A.RRT_MEM_DEVICE, self.precision, slots, 0, ids_ptr, coverage_ptr, weight_ptr)
        arr, ptr, n = self._prim_id_arg(ids)
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_mattes(self._h, r, rank, world, max_samples, ptr, n, C.byref(m)))

    # rrt_matte_extract: alpha = the coverage of the listed ids / the live weight
    def matte_extract(self, mattes, ids, out=None):
        """mattes: the dict of render_mattes; ids: 1 .. 256 ids -> (H, W) alpha of the handle's precision"""
        W, H = self.scene.resolution
        m = self._mattes_struct(mattes, "matte_extract")
        lst = np.ascontiguousarray(np.atleast_1d(ids), np.uint32)
        if out is None:
            out = np.empty((H, W), self.dtype)
        if out.dtype != self.dtype or out.shape != (H, W) or not out.flags.c_contiguous:
            raise ValueError("matte_extract: out is a C-contiguous (H, W) array of the handle's precision")
        _check(A.lib().rrt_matte_extract(self._h, C.byref(m), lst.ctypes.data, lst.size, out.ctypes.data))
        return out

    def matte_extract_device(self, ids_ptr, coverage_ptr, weight_ptr, slots, ids, out_ptr):
        m = A.Mattes(A.RRT_MEM_DEVICE, self.precision, slots, 0, ids_ptr, coverage_ptr, weight_ptr)
        lst = np.ascontiguousarray(np.atleast_1d(ids), np.uint32)
        _check(A.lib().rrt_matte_extract(self._h, C.byref(m), lst.ctypes.data, lst.size, out_ptr))

    # rrt_render_frame_aov: the frame of render_moments() and the planes of render_aov() from one camera pass - every input of denoise(..., moments=)
    def render_frame_aov(self, rect=None, rank=0, world=1, max_samples=0, film=None, moments=True, planes=("albedo", "normal", "depth"), stats=False):
        """-> (film, moments_or_None, aov_dict[, stats]): film and moments as render_moments gives them (moments: True = a new plane, False / None =
        not produced, an array = added to), aov_dict as render_aov(rect, max_samples, rank, world, planes) gives it."""
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        if film is None:
            film = np.zeros((H, W, 4), self.dtype)
        if moments is True:
            moments = np.zeros((H, W, 4), self.dtype)
        elif moments is False:
            moments = None
        for a in (film, moments):
            if a is not None and (a.dtype != self.dtype or a.shape != (H, W, 4) or not a.flags.c_contiguous):
                raise ValueError("render_frame_aov: film and moments are C-contiguous (H, W, 4) arrays of the handle's precision")
        out = {k: np.zeros((H, W, 4), self.dtype) for k in planes}
        ptr = {k: (out[k].ctypes.data if k in out else None) for k in ("albedo", "normal", "depth")}
        aov = A.Aov(A.RRT_MEM_HOST, self.precision, ptr["albedo"], ptr["normal"], ptr["depth"])
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_frame_aov(self._h, r, rank, world, film.ctypes.data, None if moments is None else moments.ctypes.data, A.RRT_MEM_HOST,
                                            max_samples, C.byref(aov), C.byref(st) if stats else None))
        return (film, moments, out, st) if stats else (film, moments, out)

    def render_frame_aov_device(self, rect, film_ptr, moments_ptr, albedo_ptr, normal_ptr, depth_ptr, max_samples=0, rank=0, world=1, stats=True):
        """The same on device buffers (raw pointers; moments_ptr and any plane but one may be None)."""
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        aov = A.Aov(A.RRT_MEM_DEVICE, self.precision, albedo_ptr, normal_ptr, depth_ptr)
        _check(A.lib().rrt_render_frame_aov(self._h, r, rank, world, film_ptr, moments_ptr, A.RRT_MEM_DEVICE, max_samples, C.byref(aov), C.byref(st) if stats else None))
        return st

    # rrt_render_adaptive: the moments frame with 8 x 8 tiles that stop once their error estimate (rrt_tile_error) is below the threshold
    def _adaptive_params(self, params):
        p = A.AdaptiveParams()
        A.lib().rrt_adaptive_defaults(C.byref(p))
        for k, v in params.items():
            if k not in ("min_samples", "batch", "max_samples", "threshold"):
                raise TypeError(f"render_adaptive: unknown parameter {k}")
            setattr(p, k, float(v) if k == "threshold" else int(v))
        return p

    def render_adaptive(self, rect=None, film=None, moments=None, stats=False, **params):
        """-> (film, moments, tile_samples[, stats]): film and moments as render_moments gives them, tile_samples (rh / 8, rw / 8) uint32 = the
        samples each 8 x 8 tile of the rect took. params: min_samples, batch, max_samples, threshold (rrt_adaptive_params)."""
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        if film is None:
            film = np.zeros((H, W, 4), self.dtype)
        if moments is None:
            moments = np.zeros((H, W, 4), self.dtype)
        for a in (film, moments):
            if a.dtype != self.dtype or a.shape != (H, W, 4) or not a.flags.c_contiguous:
                raise ValueError("render_adaptive: film and moments are C-contiguous (H, W, 4) arrays of the handle's precision")
        tiles = np.zeros((max(0, rect[3] - rect[1]) // 8, max(0, rect[2] - rect[0]) // 8), np.uint32)
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        p = self._adaptive_params(params)
        _check(A.lib().rrt_render_adaptive(self._h, r, C.byref(p), film.ctypes.data, moments.ctypes.data, tiles.ctypes.data, A.RRT_MEM_HOST, C.byref(st) if stats else None))
        return (film, moments, tiles, st) if stats else (film, moments, tiles)

    def render_adaptive_device(self, rect, film_ptr, moments_ptr, tile_samples_ptr=None, stats=True, **params):
        """The same on device buffers (raw pointers; tile_samples_ptr: (rh / 8) * (rw / 8) uint32, or None)."""
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        p = self._adaptive_params(params)
        _check(A.lib().rrt_render_adaptive(self._h, r, C.byref(p), film_ptr, moments_ptr, tile_samples_ptr, A.RRT_MEM_DEVICE, C.byref(st) if stats else None))
        return st

    # rrt_tile_error: per 8 x 8 tile of the rect, the RMS standard error of the pixels' means relative to the tile's mean luminance
    def tile_error(self, moments, rect=None):
        """moments (H, W, 4): the plane of render_moments / render_adaptive -> (rh / 8, rw / 8) float64"""
        W, H = self.scene.resolution
        rect = rect or (0, 0, W, H)
        if moments.dtype != self.dtype or moments.shape != (H, W, 4) or not moments.flags.c_contiguous:
            raise ValueError("tile_error: moments is a C-contiguous (H, W, 4) array of the handle's precision")
        out = np.zeros((max(0, rect[3] - rect[1]) // 8, max(0, rect[2] - rect[0]) // 8), np.float64)
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_tile_error(self._h, moments.ctypes.data, A.RRT_MEM_HOST, r, out.ctypes.data))
        return out

    def tile_error_device(self, moments_ptr, rect, out_ptr):
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_tile_error(self._h, moments_ptr, A.RRT_MEM_DEVICE, r, out_ptr))

    # rrt_denoise: the edge-avoiding wavelet filter over a film, guided by the planes of render_aov (the definition is on the prototype in rrt.h)
    def _denoise_params(self, params):
        p = A.DenoiseParams()
        A.lib().rrt_denoise_defaults(C.byref(p))
        for k, v in params.items():
            if k not in ("iterations", "demodulate", "sigma_color", "sigma_normal", "sigma_depth"):
                raise TypeError(f"denoise: unknown parameter {k}")
            setattr(p, k, int(v) if k in ("iterations", "demodulate") else float(v))
        return p

    def denoise(self, film, aov, out=None, moments=None, **params):
        """film (H, W, 4) and aov = the dict of render_aov (all three planes), host arrays of the handle's precision -> the filtered film
        (`out`, which may be `film`, or a new array). params: iterations, demodulate, sigma_color, sigma_normal, sigma_depth.
        moments: the plane of render_moments; the filter then starts from the pixels' sample variance (rrt_denoise_moments)."""
        W, H = self.scene.resolution
        arrs = [film] + [aov[k] for k in ("albedo", "normal", "depth")] + ([] if moments is None else [moments])
        for a in arrs:
            if a.dtype != self.dtype or a.shape != (H, W, 4) or not a.flags.c_contiguous:
                raise ValueError("denoise: film and planes are C-contiguous (H, W, 4) arrays of the handle's precision")
        if out is None:
            out = np.empty((H, W, 4), self.dtype)
        if out.dtype != self.dtype or out.shape != (H, W, 4) or not out.flags.c_contiguous:
            raise ValueError("denoise: out is a C-contiguous (H, W, 4) array of the handle's precision")
        d = A.Aov(A.RRT_MEM_HOST, self.precision, *[a.ctypes.data for a in arrs[1:4]])
        p = self._denoise_params(params)
        if moments is None:
            _check(A.lib().rrt_denoise(self._h, film.ctypes.data, C.byref(d), C.byref(p), out.ctypes.data))
        else:
            _check(A.lib().rrt_denoise_moments(self._h, film.ctypes.data, C.byref(d), moments.ctypes.data, C.byref(p), out.ctypes.data))
        return out

    def denoise_device(self, film_ptr, aov_ptrs, out_ptr, moments_ptr=None, **params):
        """The same on device buffers: raw pointers of the film, the (albedo, normal, depth) planes and the output (which may be the film);
        moments_ptr: the plane of rrt_render_moments (rrt_denoise_moments)."""
        d = A.Aov(A.RRT_MEM_DEVICE, self.precision, *aov_ptrs)
        p = self._denoise_params(params)
        if moments_ptr is None:
            _check(A.lib().rrt_denoise(self._h, film_ptr, C.byref(d), C.byref(p), out_ptr))
        else:
            _check(A.lib().rrt_denoise_moments(self._h, film_ptr, C.byref(d), moments_ptr, C.byref(p), out_ptr))

    def render_device(self, rect, film_ptr, stats=True):
        st = A.RenderStats()
        r = (C.c_int32 * 4)(*rect)
        _check(A.lib().rrt_render_rect(self._h, r, film_ptr, A.RRT_MEM_DEVICE, C.byref(st) if stats else None))
        return st


class Comm:
    """RCCL communicator behind the C ABI (rrt_comm_*): one per rank, one process per GPU. Rank 0 draws the id
    (`Comm.new_id()`) and ships the 128 bytes to the others over whatever channel the host has (torch.distributed
    broadcast in bench.py); creation is collective."""

    def __init__(self, comm_id, rank, world, device):
        buf = (C.c_uint8 * A.RRT_COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
        h = C.c_void_p()
        _check(A.lib().rrt_comm_create(buf, rank, world, device, C.byref(h)))
        self._h, self.rank, self.world = h, rank, world

    @staticmethod
    def new_id():
        buf = (C.c_uint8 * A.RRT_COMM_ID_BYTES)()
        _check(A.lib().rrt_comm_id(buf))
        return bytes(buf)

    def gather(self, renderer, film_ptr, root=0):
        """rrt_film_gather: this rank's bands -> root (box filter) / sum of the films on root (wide filters); enqueued on the
        renderer's stream."""
        _check(A.lib().rrt_film_gather(renderer._h, self._h, film_ptr, root))

    def close(self):
        if getattr(self, "_h", None):
            A.lib().rrt_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def band_rows(yres, rank, world):
    """[(y0, y1)] of the 16-row bands `rank` owns (rrt_band_rows: the C ABI's own partition arithmetic)."""
    n = A.lib().rrt_band_rows(yres, rank, world, None, 0)
    if n < 0:
        _check(n)
    buf = (C.c_int32 * (2 * max(n, 1)))()
    A.lib().rrt_band_rows(yres, rank, world, buf, n)
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


def resolve_rgba8(film, scale=1.0):
    """Film::write_image (film.rs:323-366) + gamma/quantise of renderprocess::write_image (:1501-1530)."""
    film = np.ascontiguousarray(film)
    H, W, _ = film.shape
    prec = A.RRT_F32 if film.dtype == np.float32 else A.RRT_F64
    rgba = np.zeros((H, W, 4), np.uint8)
    _check(A.lib().rrt_resolve_rgba8(film.ctypes.data, prec, W, H, float(scale), rgba.ctypes.data))
    return rgba


def resolve_aov(aov):
    """The sums of Renderer.render_aov -> dict(albedo (H, W, 3) = rgb / w_live, normal (H, W, 3) unit length (0 where nothing
    is hit), depth (H, W) mean first-hit distance (0 where nothing is hit), coverage (H, W) = w_hit / w_live)."""
    alb, nrm, dep = (np.asarray(aov[k], np.float64) for k in ("albedo", "normal", "depth"))
    w_live, w_hit = alb[..., 3], dep[..., 2]
    live, hit = w_live != 0, w_hit != 0
    albedo = np.where(live[..., None], alb[..., :3] / np.where(live, w_live, 1.0)[..., None], 0.0)
    length = np.linalg.norm(nrm[..., :3], axis=-1)
    normal = np.where((length > 0)[..., None], nrm[..., :3] / np.where(length > 0, length, 1.0)[..., None], 0.0)
    depth = np.where(hit, dep[..., 0] / np.where(hit, w_hit, 1.0), 0.0)
    coverage = np.where(live, w_hit / np.where(live, w_live, 1.0), 0.0)
    return dict(albedo=albedo, normal=normal, depth=depth, coverage=coverage)


def resolve_ao(planes):
    """The sums of Renderer.render_ao -> dict(ao (H, W) in [0, 1]: the mean of a / pi over the hit samples (1 = fully open, 0 where nothing
    is hit; the uniform mode's estimate can pass 1 and is clipped), ao_var (H, W): the weighted sample variance of a / pi over the hit
    samples, bent (H, W, 3): the unit bent normal (0 where nothing is hit or no ray is free; only with the "bent" plane), coverage (H, W) =
    w_hit / w_live)."""
    ao = np.asarray(planes["ao"], np.float64)
    w_hit, w_live = ao[..., 2], ao[..., 3]
    hit, live = w_hit != 0, w_live != 0
    wh = np.where(hit, w_hit, 1.0)
    mean = np.where(hit, ao[..., 0] / wh, 0.0) / np.pi
    var = np.where(hit, np.maximum(0.0, ao[..., 1] / wh / (np.pi * np.pi) - mean * mean), 0.0)
    out = dict(ao=np.clip(mean, 0.0, 1.0), ao_var=var, coverage=np.where(live, w_hit / np.where(live, w_live, 1.0), 0.0))
    if "bent" in planes:
        b = np.asarray(planes["bent"], np.float64)[..., :3]
        length = np.linalg.norm(b, axis=-1)
        out["bent"] = np.where((length > 0)[..., None], b / np.where(length > 0, length, 1.0)[..., None], 0.0)
    return out


def write_ao_png(path, planes):
    """The resolved occlusion as grey - what rrt_render writes under RRT_AO=<path.png>."""
    grey = resolve_ao(planes)["ao"]
    rgba = np.empty(grey.shape + (4,), np.uint8)
    rgba[..., :3] = np.clip(np.nan_to_num(grey) * 255.0 + 0.5, 0.0, 255.0).astype(np.uint8)[..., None]
    rgba[..., 3] = 255
    write_png(path, rgba)


def resolve_irradiance(sums, n_draws):
    """The sums of Renderer.irradiance (cosine mode) over n_draws draws per point -> dict(E (m, 3) = pi / N * sum L: the irradiance, stderr (m,):
    the standard error of E's luminance, pi * sqrt((sum y^2 / N - mean_y^2) / (N - 1)) (0 where N < 2)). Dead draws count: they are draws
    that carried nothing."""
    s = np.asarray(sums, np.float64)
    N = float(n_draws)
    E = np.pi / N * s[..., :3]
    mean_y = (s[..., :3] @ np.array([0.212671, 0.715160, 0.072169])) / N
    var = np.maximum(0.0, s[..., 3] / N - mean_y * mean_y)
    stderr = np.pi * np.sqrt(var / (N - 1.0)) if N >= 2 else np.zeros_like(mean_y)
    return dict(E=E, stderr=stderr)


def resolve_sh(sh, n_draws):
    """The sh sums of Renderer.irradiance (sphere mode) over n_draws draws per point -> (m, 9, 3): the coefficients 4 pi / N * sum L Y_k of the
    radiance around each point, bands 0 .. 2 in rrt.h's order, in the point's local frame."""
    s = np.asarray(sh, np.float64)
    return (4.0 * np.pi / float(n_draws)) * s.reshape(s.shape[:-1] + (9, 3))


def unpack_visibility(bits, n_b):
    """The packed words of Renderer.visibility -> bool: bits (n_a, words) -> (n_a, n_b), bit j & 63 of word j // 64 of a row; a pairs=True result
    (words,) -> (n_b,)."""
    b = np.ascontiguousarray(bits, np.uint64)
    j = np.arange(int(n_b))
    return ((b[..., j // 64] >> (j % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def resolve_moments(m):
    """The sums of Renderer.render_moments -> dict(mean (H, W) = S1 / S0: the pixel's mean sample luminance, variance_of_mean (H, W) =
    (S2 / S0 - mean^2) / (n_eff - 1) (0 where n_eff < 2), n_eff (H, W) = S0^2 / S3: Kish's effective sample count)."""
    m = np.asarray(m, np.float64)
    s1, s2, s0, s3 = m[..., 0], m[..., 1], m[..., 2], m[..., 3]
    with np.errstate(all="ignore"):
        n_eff = np.where(s3 > 0, s0 * s0 / s3, 0.0)
        mean = np.where(s0 > 0, s1 / s0, 0.0)
        var = np.where(n_eff >= 2, np.maximum(0.0, s2 / s0 - mean * mean) / (n_eff - 1.0), 0.0)
    return dict(mean=mean, variance_of_mean=var, n_eff=n_eff)


def write_aov_pngs(prefix, aov):
    """<prefix>_albedo.png, <prefix>_normal.png (n * 0.5 + 0.5), <prefix>_depth.png (mean depth scaled to its own min .. max
    over the covered pixels) from the sums of Renderer.render_aov - what rrt_render writes under RRT_AOV=<prefix>."""
    res = resolve_aov(aov)
    hit = res["coverage"] > 0
    d = res["depth"]
    lo, hi = (float(d[hit].min()), float(d[hit].max())) if hit.any() else (0.0, 0.0)
    grey = np.where(hit, (d - lo) / (hi - lo) if hi > lo else 0.0, 0.0)
    images = {"albedo": res["albedo"], "normal": np.where(hit[..., None], res["normal"] * 0.5 + 0.5, 0.0), "depth": np.repeat(grey[..., None], 3, -1)}
    for name, rgb in images.items():
        rgba = np.empty(rgb.shape[:2] + (4,), np.uint8)
        rgba[..., :3] = np.clip(np.nan_to_num(rgb) * 255.0 + 0.5, 0.0, 255.0).astype(np.uint8)
        rgba[..., 3] = 255
        write_png(f"{prefix}_{name}.png", rgba)


def resolve_mattes(m):
    """The table of Renderer.render_mattes -> (H, W, K) float64 shares coverage / weight[..., 0] (0 where no live sample covers the pixel)."""
    cov, w0 = np.asarray(m["coverage"], np.float64), np.asarray(m["weight"], np.float64)[..., 0]
    live = w0 != 0
    return np.where(live[..., None], cov / np.where(live, w0, 1.0)[..., None], 0.0)


def matte_colour(ids):
    """(..., 3) float64: the three low bytes of id * 2654435761 (mod 2^32), each / 255 - the preview colour of an id"""
    h = (np.asarray(ids).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return np.stack([(h >> np.uint64(s)) & np.uint64(0xFF) for s in (0, 8, 16)], -1).astype(np.float64) / 255.0


def write_matte_png(path, m):
    """One preview image of a matte table: per pixel sum_k colour(id_k) * coverage_k / weight[0], the slots added in stored order, quantised as
    write_aov_pngs quantises - what rrt_render writes under RRT_MATTES=<path.png>."""
    share = resolve_mattes(m)
    col = matte_colour(m["ids"])
    rgb = np.zeros(share.shape[:2] + (3,))
    for k in range(share.shape[2]):
        rgb += col[:, :, k, :] * share[:, :, k, None]
    rgba = np.empty(rgb.shape[:2] + (4,), np.uint8)
    rgba[..., :3] = np.clip(np.nan_to_num(rgb) * 255.0 + 0.5, 0.0, 255.0).astype(np.uint8)
    rgba[..., 3] = 255
    write_png(path, rgba)


def write_pass_pngs(prefix, renderer, n_lights, scale=1.0):
    """<prefix>_direct.png (path vertex 0), <prefix>_indirect.png (vertices >= 1) and <prefix>_light<i>.png for the first 14 lights, from one
    Renderer.render_passes call - what rrt_render writes under RRT_PASSES=<prefix>."""
    shown = min(int(n_lights), A.RRT_MAX_PASSES - 2)
    if n_lights > shown:
        print(f"RRT_PASSES writes the passes of the first {shown} of the scene's {n_lights} lights", file=sys.stderr, flush=True)
    names = ["direct", "indirect"] + [f"light{i}" for i in range(shown)]
    passes = [(0xFFFFFFFF, 0, 1), (0xFFFFFFFF, 1, 0)] + [(1 << i, 0, 0) for i in range(shown)]
    _, films = renderer.render_passes(passes, light_group=[min(i, 31) for i in range(n_lights)], film=None)
    for name, f in zip(names, films):
        write_png(f"{prefix}_{name}.png", resolve_rgba8(f, scale))


def write_png(path, rgba):
    rgba = np.ascontiguousarray(rgba, np.uint8)
    H, W, _ = rgba.shape
    _check(A.lib().rrt_write_png(os.fsencode(path), rgba.ctypes.data, W, H))


def deploy_render(filepath, save_to, device=0, precision=A.RRT_F32, flags=0, overrides=None):
    """renderprocess::deploy_render(filepath, save_to): load scene.json, render, write the PNG.

    `overrides` (dict) is merged into the top level of the scene config before loading, e.g. to swap the
    StratifiedSampler of samples/scene.json for the HaltonSampler or to change the resolution."""
    with open(filepath) as f:
        cfg = json.load(f)
    if overrides:
        cfg.update(overrides)
    root = os.path.dirname(os.path.realpath(filepath)) or "."
    scene = Scene.loads(cfg, root, flags)
    for w in scene.warnings:
        print(w, flush=True)
    r = Renderer(scene, device, precision)
    for w in r.warnings:
        print(w, flush=True)
    moments = aov = None
    with_moments = bool(os.environ.get("RRT_DENOISE")) and os.environ.get("RRT_DENOISE_MOMENTS", "0") not in ("", "0")
    follow = int(os.environ.get("RRT_AOV_FOLLOW") or 0)   # as rrt_render: > 0 takes the planes of RRT_AOV / RRT_DENOISE from rrt_render_aov_follow
    if os.environ.get("RRT_ADAPTIVE"):   # as rrt_render: rrt_render_adaptive in the frame's place
        params = {"threshold": float(os.environ["RRT_ADAPTIVE"])}
        for key, var in (("min_samples", "RRT_ADAPTIVE_MIN"), ("batch", "RRT_ADAPTIVE_BATCH")):
            if os.environ.get(var):
                params[key] = int(os.environ[var])
        film, plane, _, st = r.render_adaptive(stats=True, **params)
        moments = plane if with_moments else None
        W, H = scene.resolution
        print(f"{st.camera_samples} of {W * H * max(0, scene.desc.sampler.samples_per_pixel - 1)} camera samples taken (adaptive)")
    elif with_moments and follow > 0:   # as rrt_render: the moments frame; the followed planes come from their own call below
        film, moments, st = r.render_moments(stats=True)
    elif with_moments:   # as rrt_render: the same frame, its sample-variance plane and the denoiser's feature planes from one camera pass
        film, moments, aov, st = r.render_frame_aov(max_samples=32, stats=True)
    else:
        film, st = r.render(stats=True)
    print(f"{st.camera_rays} rays generated")
    rgba = resolve_rgba8(film, scene.desc.film.scale)
    write_png(save_to, rgba)
    if os.environ.get("RRT_AOV"):   # as rrt_render: three PNGs after the frame
        write_aov_pngs(os.environ["RRT_AOV"], r.render_aov(follow=follow))
    if os.environ.get("RRT_AO"):   # as rrt_render: the resolved occlusion as grey after the frame
        write_ao_png(os.environ["RRT_AO"], r.render_ao(max_samples=int(os.environ.get("RRT_AO_SPP") or 0),
                                                       n_samples=int(os.environ["RRT_AO_SAMPLES"]) if os.environ.get("RRT_AO_SAMPLES") else None, planes=("ao",)))
    if os.environ.get("RRT_PASSES"):   # as rrt_render: direct, indirect and one PNG per light (the first 14) after the frame
        write_pass_pngs(os.environ["RRT_PASSES"], r, scene.desc.n_lights, scene.desc.film.scale)
    if os.environ.get("RRT_MATTES"):   # as rrt_render: one preview image of the ID mattes after the frame
        by = os.environ.get("RRT_MATTE_BY") or "object"
        if by not in ("material", "instance", "object"):
            raise ValueError("RRT_MATTE_BY must be material, instance or object")
        write_matte_png(os.environ["RRT_MATTES"], r.render_mattes(ids=by, slots=int(os.environ.get("RRT_MATTE_SLOTS") or 6)))
    if os.environ.get("RRT_DENOISE"):   # as rrt_render: the filtered frame, guided by the planes of at most 32 samples per pixel
        write_png(os.environ["RRT_DENOISE"], resolve_rgba8(r.denoise(film, aov if aov is not None else r.render_aov(max_samples=32, follow=follow), moments=moments), scene.desc.film.scale))
    r.close()
    return film, st
