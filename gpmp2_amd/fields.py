"""The field calls of Engine: signed distance field handles and their updates in place (include/gpmp2mi.h "signed distance
fields", "live map", "sensor map", "scene")."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import dptr, f64, iptr
from .marshalling import _dev_arg, _Handle


class FieldCalls:
    """Mixed into Engine, which brings self.lib and self._ck."""

    def sdf(self, origin, cell_size, data, layout=_capi.SDF_LAYOUT_ZYX):
        data = f64(data)
        dim = data.ndim
        if dim == 2:
            ny, nx, nz = data.shape[0], data.shape[1], 1
        else:
            nz, ny, nx = data.shape
        org = f64(list(origin) + [0.0] * (3 - len(origin)))
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_sdf_create(C.c_int(dim), dptr(org), C.c_double(cell_size), nx, ny, nz,
                                             dptr(data), C.c_int(layout), C.byref(out)))
        h = _Handle(out, self.lib.gpmp2mi_sdf_destroy)
        h.dim, h.shape = dim, data.shape
        return h

    def sdf_field_from_occupancy(self, occ, cell_size):
        """occupancy [ny][nx] or [nz][ny][nx] -> signed field of the same shape (computed on the GPU)"""
        occ = f64(occ)
        dim = occ.ndim
        nz, ny, nx = ((1,) + occ.shape) if dim == 2 else occ.shape
        field = np.zeros_like(occ)
        self._ck(self.lib.gpmp2mi_sdf_field_from_occupancy(C.c_int(dim), nx, ny, nz, dptr(occ), C.c_double(cell_size),
                                                           dptr(field)))
        return field

    def sdf_from_occupancy(self, origin, cell_size, occ, layout=_capi.SDF_LAYOUT_ZYX):
        occ = f64(occ)
        dim = occ.ndim
        nz, ny, nx = ((1,) + occ.shape) if dim == 2 else occ.shape
        org = f64(list(origin) + [0.0] * (3 - len(origin)))
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_sdf_create_from_occupancy(C.c_int(dim), dptr(org), C.c_double(cell_size), nx, ny, nz,
                                                            dptr(occ), C.c_int(layout), C.byref(out)))
        h = _Handle(out, self.lib.gpmp2mi_sdf_destroy)
        h.dim, h.shape = dim, occ.shape
        return h

    def sdf_read_vol(self, filename_pre):
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_sdf_read_vol(str(filename_pre).encode(), C.byref(out)))
        h = _Handle(out, self.lib.gpmp2mi_sdf_destroy)
        h.dim = 3
        return h

    def sdf_field(self, sdf):
        """-> dict(dim, origin, cell_size, data [nz][ny][nx] or [ny][nx])"""
        dim, nx, ny, nz = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        org, cell = np.zeros(3), C.c_double()
        self._ck(self.lib.gpmp2mi_sdf_get_field(sdf.ptr, C.byref(dim), C.byref(nx), C.byref(ny), C.byref(nz), dptr(org),
                                                C.byref(cell), None))
        data = np.zeros((nz.value, ny.value, nx.value))
        self._ck(self.lib.gpmp2mi_sdf_get_field(sdf.ptr, None, None, None, None, None, None, dptr(data)))
        return dict(dim=dim.value, origin=org[:dim.value].copy(), cell_size=cell.value,
                    data=data[0] if dim.value == 2 else data)

    # ---------------------------------------------------------------- live map (include/gpmp2mi.h "live map")
    def _sdf_shape(self, sdf):
        """The voxel shape of a field handle, [nz][ny][nx] or [ny][nx]: kept by the calls that made it from an array, asked
        of the library once otherwise."""
        if getattr(sdf, "shape", None) is None:
            nx, ny, nz = C.c_int(), C.c_int(), C.c_int()
            self._ck(self.lib.gpmp2mi_sdf_get_field(sdf.ptr, None, C.byref(nx), C.byref(ny), C.byref(nz), None, None, None))
            sdf.shape = (nz.value, ny.value, nx.value)[3 - sdf.dim:]
        return tuple(sdf.shape)

    def _grid_arg(self, sdf, name, a, layout):
        a, shape = f64(a), self._sdf_shape(sdf)
        if layout not in (_capi.SDF_LAYOUT_ZYX, _capi.SDF_LAYOUT_GTSAM):
            raise ValueError("unknown voxel layout")
        if a.ndim != len(shape) or a.size != int(np.prod(shape)) or (layout == _capi.SDF_LAYOUT_ZYX and a.shape != shape):
            raise ValueError(f"{name}: expected {list(shape)} (the handle's grid), got {list(a.shape)}")
        return a

    def _points_args(self, sdf, robot, conf, margin):
        margin = float(margin)
        if np.isnan(margin):
            raise ValueError("margin must not be NaN")
        if robot is not None and conf is None:
            raise ValueError("the self filter needs the robot's configuration")
        return margin

    def sdf_reserve_update(self, sdf):
        """Takes the update workspace of the handle now, so that the first `_dev` update does not allocate."""
        self._ck(self.lib.gpmp2mi_sdf_reserve_update(sdf.ptr))

    def sdf_update(self, sdf, data, layout=_capi.SDF_LAYOUT_ZYX):
        """New voxels of the handle's own shape, in place; the handle then equals Engine.sdf of the same data."""
        data = self._grid_arg(sdf, "data", data, layout)
        self._ck(self.lib.gpmp2mi_sdf_update(sdf.ptr, dptr(data), C.c_int(layout)))

    def sdf_update_dev(self, sdf, data, stream=None):
        """The same from a device buffer in [nz][ny][nx] order (torch tensor or raw pointer), enqueued on `stream`."""
        self._ck(self.lib.gpmp2mi_sdf_update_dev(sdf.ptr, _dev_arg("data", data, self._sdf_shape(sdf)),
                                                 C.c_void_p(stream or 0)))

    def sdf_update_from_occupancy(self, sdf, occ, layout=_capi.SDF_LAYOUT_ZYX):
        """The handle's field from an occupancy grid of its own shape, in place (as Engine.sdf_from_occupancy); the
        obstacle set becomes the handle's base."""
        occ = self._grid_arg(sdf, "occ", occ, layout)
        self._ck(self.lib.gpmp2mi_sdf_update_from_occupancy(sdf.ptr, dptr(occ), C.c_int(layout)))

    def sdf_update_from_occupancy_dev(self, sdf, occ, stream=None):
        self._ck(self.lib.gpmp2mi_sdf_update_from_occupancy_dev(sdf.ptr, _dev_arg("occ", occ, self._sdf_shape(sdf)),
                                                                C.c_void_p(stream or 0)))

    def sdf_update_from_points(self, sdf, points, use_base=True, robot=None, conf=None, margin=0.0):
        """The handle's field from a point cloud [M][dim] (and the base when use_base), in place.  robot / conf: drop the
        points inside the robot's body spheres grown by `margin`.  -> dict(kept, non_finite, self, outside)."""
        margin = self._points_args(sdf, robot, conf, margin)
        p = f64(points)
        if p.size == 0:
            p = p.reshape(0, sdf.dim)
        if p.ndim != 2 or p.shape[1] != sdf.dim:
            raise ValueError(f"points: expected [M][{sdf.dim}], got {list(p.shape)}")
        q = None
        if robot is not None:
            q = f64(conf).reshape(-1)
            if q.size != robot.dof:
                raise ValueError(f"conf: expected [{robot.dof}], got {list(np.shape(conf))}")
        stats = np.zeros(4, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_update_from_points(sdf.ptr, p.shape[0], dptr(p), int(bool(use_base)),
                                                         None if robot is None else robot.ptr, dptr(q), margin,
                                                         iptr(stats)))
        return dict(zip(("kept", "non_finite", "self", "outside"), (int(x) for x in stats)))

    def sdf_update_from_points_dev(self, sdf, M, points, use_base=True, robot=None, conf=None, margin=0.0, stats=None,
                                   stream=None):
        """The same from device buffers (torch tensors or raw pointers): points [M][dim], conf [dof], stats [4] int32 or
        None; enqueued on `stream`, no host synchronisation."""
        margin, M = self._points_args(sdf, robot, conf, margin), int(M)
        if M < 0:
            raise ValueError("M must be >= 0")
        args = [_dev_arg("points", points, (M, sdf.dim)), int(bool(use_base)), None if robot is None else robot.ptr,
                None if robot is None else _dev_arg("conf", conf, (robot.dof,)), margin,
                _dev_arg("stats", stats, (4,), True)]
        self._ck(self.lib.gpmp2mi_sdf_update_from_points_dev(sdf.ptr, M, *args, C.c_void_p(stream or 0)))

    def sdf_update_timing(self, sdf, on=True, read=False):
        """Stage timer of the updates (gpmp2mi_debug_sdf_update_timing): read = True returns the device times in ms of the
        last recorded update as dict(seed_mark, passes, finish, pack)."""
        ms = np.zeros(4) if read else None
        self._ck(self.lib.gpmp2mi_debug_sdf_update_timing(sdf.ptr, int(bool(on)), dptr(ms)))
        return None if ms is None else dict(zip(("seed_mark", "passes", "finish", "pack"), (float(x) for x in ms)))

    # ---------------------------------------------------------------- sensor map (include/gpmp2mi.h "sensor map")
    EVIDENCE_DEFAULTS = dict(hit=2, miss=1, lo=-4, hi=8, occupied_at=1, use_base=False, refresh=True)
    EVIDENCE_STATS = ("hit", "invalid", "max_range", "self", "outside", "occupied")

    @classmethod
    def _evidence_opts(cls, opts):
        unknown = set(opts) - set(cls.EVIDENCE_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown evidence options: {sorted(unknown)}")
        o = _capi.EvidenceOpts()
        for k, v in dict(cls.EVIDENCE_DEFAULTS, **opts).items():
            setattr(o, k, int(v))
        return o

    @staticmethod
    def _camera(camera):
        """dict(width, height, fx, fy, cx, cy, depth_min, depth_max, pose [3][4] camera -> world) -> DepthCamera"""
        pose = f64(camera["pose"])
        if pose.size != 12:
            raise ValueError(f"camera pose: expected [3][4], got {list(pose.shape)}")
        cam = _capi.DepthCamera()
        cam.width, cam.height = int(camera["width"]), int(camera["height"])
        for k in ("fx", "fy", "cx", "cy", "depth_min", "depth_max"):
            setattr(cam, k, float(camera[k]))
        for k, v in enumerate(pose.reshape(12)):
            cam.pose[k] = float(v)
        return cam

    def _sensor_origin(self, sdf, sensor_origin):
        o = f64(sensor_origin).reshape(-1)
        if o.size != sdf.dim:
            raise ValueError(f"sensor_origin: expected [{sdf.dim}], got {list(np.shape(sensor_origin))}")
        return o

    def _conf_arg(self, robot, conf):
        if robot is None:
            return None
        q = f64(conf).reshape(-1)
        if q.size != robot.dof:
            raise ValueError(f"conf: expected [{robot.dof}], got {list(np.shape(conf))}")
        return q

    def sdf_reserve_evidence(self, sdf):
        """Takes the evidence workspace of the handle now, so that the first `_dev` integrate call does not allocate."""
        self._ck(self.lib.gpmp2mi_sdf_reserve_evidence(sdf.ptr))

    def sdf_integrate_points(self, sdf, points, sensor_origin, robot=None, conf=None, margin=0.0, **opts):
        """One frame of rays from sensor_origin [dim] to points [M][dim] into the handle's evidence: +hit where a ray
        ends, -miss where rays pass, clamped; then (refresh) the field again from the cells with evidence >= occupied_at.
        opts: hit, miss, lo, hi, occupied_at, use_base, refresh (EVIDENCE_DEFAULTS).  robot / conf / margin: rays that
        end inside the robot's body spheres carve and do not mark.
        -> dict(hit, invalid, max_range, self, outside, occupied)."""
        margin = self._points_args(sdf, robot, conf, margin)
        p = f64(points)
        if p.size == 0:
            p = p.reshape(0, sdf.dim)
        if p.ndim != 2 or p.shape[1] != sdf.dim:
            raise ValueError(f"points: expected [M][{sdf.dim}], got {list(p.shape)}")
        o, q, eo = self._sensor_origin(sdf, sensor_origin), self._conf_arg(robot, conf), self._evidence_opts(opts)
        stats = np.zeros(6, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_integrate_points(sdf.ptr, p.shape[0], dptr(p), dptr(o),
                                                       None if robot is None else robot.ptr, dptr(q), margin,
                                                       C.byref(eo), iptr(stats)))
        return dict(zip(self.EVIDENCE_STATS, (int(x) for x in stats)))

    def sdf_integrate_points_dev(self, sdf, M, points, sensor_origin, robot=None, conf=None, margin=0.0, stats=None,
                                 stream=None, **opts):
        """The same from device buffers (torch tensors or raw pointers): points [M][dim], conf [dof], stats [6] int32 or
        None; sensor_origin is a host array.  Enqueued on `stream`, no host synchronisation."""
        margin, M = self._points_args(sdf, robot, conf, margin), int(M)
        if M < 0:
            raise ValueError("M must be >= 0")
        o, eo = self._sensor_origin(sdf, sensor_origin), self._evidence_opts(opts)
        self._ck(self.lib.gpmp2mi_sdf_integrate_points_dev(
            sdf.ptr, M, _dev_arg("points", points, (M, sdf.dim)), dptr(o), None if robot is None else robot.ptr,
            None if robot is None else _dev_arg("conf", conf, (robot.dof,)), margin, C.byref(eo),
            _dev_arg("stats", stats, (6,), True), C.c_void_p(stream or 0)))

    def sdf_integrate_depth(self, sdf, camera, depth, robot=None, conf=None, margin=0.0, **opts):
        """One depth image [height][width] (float32 metres along the optical axis) of `camera` (a dict: width, height,
        fx, fy, cx, cy, depth_min, depth_max, pose [3][4] camera -> world) into the evidence of a 3-D handle, as
        sdf_integrate_points; pixels beyond depth_max carve up to depth_max and mark no end."""
        margin = self._points_args(sdf, robot, conf, margin)
        cam = self._camera(camera)
        z = np.ascontiguousarray(depth, dtype=np.float32)
        if sdf.dim != 3:
            raise ValueError("the depth form needs a 3-D field")
        if z.shape != (cam.height, cam.width):
            raise ValueError(f"depth: expected [{cam.height}][{cam.width}], got {list(z.shape)}")
        q, eo = self._conf_arg(robot, conf), self._evidence_opts(opts)
        stats = np.zeros(6, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_integrate_depth(sdf.ptr, C.byref(cam), z.ctypes.data_as(C.POINTER(C.c_float)),
                                                      None if robot is None else robot.ptr, dptr(q), margin,
                                                      C.byref(eo), iptr(stats)))
        return dict(zip(self.EVIDENCE_STATS, (int(x) for x in stats)))

    def sdf_integrate_depth_dev(self, sdf, camera, depth, robot=None, conf=None, margin=0.0, stats=None, stream=None,
                                **opts):
        """The same from device buffers: depth a contiguous float32 cuda tensor [height][width] or a raw pointer."""
        margin = self._points_args(sdf, robot, conf, margin)
        cam, eo = self._camera(camera), self._evidence_opts(opts)
        if hasattr(depth, "data_ptr"):
            if (str(depth.dtype) != "torch.float32" or not depth.is_contiguous() or depth.device.type != "cuda"
                    or tuple(depth.shape) != (cam.height, cam.width)):
                raise ValueError(f"depth: expected a contiguous torch.float32 cuda tensor of shape "
                                 f"{[cam.height, cam.width]}, got {depth.dtype} {list(depth.shape)} on {depth.device}")
            depth = depth.data_ptr()
        self._ck(self.lib.gpmp2mi_sdf_integrate_depth_dev(
            sdf.ptr, C.byref(cam), C.c_void_p(int(depth)), None if robot is None else robot.ptr,
            None if robot is None else _dev_arg("conf", conf, (robot.dof,)), margin, C.byref(eo),
            _dev_arg("stats", stats, (6,), True), C.c_void_p(stream or 0)))

    def sdf_refresh_from_evidence(self, sdf, occupied_at=1, use_base=False, stream=None, dev=False):
        """The field again from the evidence as it stands: the cells with evidence >= occupied_at, united with the base
        when use_base.  dev = True: enqueued on `stream` without a host synchronisation."""
        if dev:
            self._ck(self.lib.gpmp2mi_sdf_refresh_from_evidence_dev(sdf.ptr, int(occupied_at), int(bool(use_base)),
                                                                    C.c_void_p(stream or 0)))
        else:
            self._ck(self.lib.gpmp2mi_sdf_refresh_from_evidence(sdf.ptr, int(occupied_at), int(bool(use_base))))

    def sdf_evidence_reset(self, sdf, stream=None, dev=False):
        """Evidence 0 everywhere; the field stays as it is."""
        if dev:
            self._ck(self.lib.gpmp2mi_sdf_evidence_reset_dev(sdf.ptr, C.c_void_p(stream or 0)))
        else:
            self._ck(self.lib.gpmp2mi_sdf_evidence_reset(sdf.ptr))

    def sdf_evidence(self, sdf):
        """-> the handle's evidence, int16 [nz][ny][nx] or [ny][nx] (all 0 before the first integrate call)"""
        E = np.zeros(self._sdf_shape(sdf), dtype=np.int16)
        self._ck(self.lib.gpmp2mi_sdf_get_evidence(sdf.ptr, E.ctypes.data_as(C.POINTER(C.c_int16))))
        return E

    def sdf_integrate_timing(self, sdf, on=True, read=False):
        """Stage timer of the integrate calls (gpmp2mi_debug_sdf_integrate_timing): read = True returns the device times
        in ms of the last recorded call with refresh as dict(deproject, walk, apply_seed, passes, finish, pack)."""
        ms = np.zeros(6) if read else None
        self._ck(self.lib.gpmp2mi_debug_sdf_integrate_timing(sdf.ptr, int(bool(on)), dptr(ms)))
        names = ("deproject", "walk", "apply_seed", "passes", "finish", "pack")
        return None if ms is None else dict(zip(names, (float(x) for x in ms)))

    # ---------------------------------------------------------------- scene (include/gpmp2mi.h "scene")
    def scene(self, objects):
        """A scene handle of Box / Sphere / Cylinder / Mesh objects (gpmp2_amd.scene) on the current device."""
        from . import scene as _scene
        return _scene.Scene(objects, self)

    def sdf_update_from_scene(self, sdf, scene, use_base=False, use_evidence=False, occupied_at=1):
        """The handle's field from the scene's enabled objects, united with the base (use_base) and with the cells whose
        evidence is >= occupied_at (use_evidence), in place.  -> cells [K] int32: the count of each object alone
        (0 disabled, -1 a mesh out of range)."""
        cells = np.zeros(scene.K, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_update_from_scene(sdf.ptr, scene.ptr, int(bool(use_base)), int(bool(use_evidence)),
                                                        int(occupied_at), iptr(cells)))
        return cells

    def sdf_update_from_scene_dev(self, sdf, scene, use_base=False, use_evidence=False, occupied_at=1, cells=None,
                                  stream=None):
        """The same enqueued on `stream` without a host synchronisation; cells: a device buffer [K] int32 or None."""
        self._ck(self.lib.gpmp2mi_sdf_update_from_scene_dev(sdf.ptr, scene.ptr, int(bool(use_base)),
                                                            int(bool(use_evidence)), int(occupied_at),
                                                            _dev_arg("cells", cells, (scene.K,), True),
                                                            C.c_void_p(stream or 0)))

    def scene_rasterize_dev(self, scene, origin, cell_size, shape, mask, cells=None, stream=None):
        """The scene alone into a device byte mask of `shape` ([nz][ny][nx] or [ny][nx]; a contiguous torch.uint8 cuda
        tensor or a raw pointer) on `stream`; cells: a device buffer [K] int32 or None."""
        shape = tuple(int(x) for x in shape)
        dim = len(shape)
        origin = f64(origin).reshape(-1)
        if dim not in (2, 3) or origin.size != dim:
            raise ValueError(f"a shape of 2 or 3 sizes and an origin of as many numbers, got {shape}, {origin.size}")
        if hasattr(mask, "data_ptr"):
            if (str(mask.dtype) != "torch.uint8" or not mask.is_contiguous() or mask.device.type != "cuda"
                    or tuple(mask.shape) != shape):
                raise ValueError(f"mask: expected a contiguous torch.uint8 cuda tensor of shape {list(shape)}, got "
                                 f"{mask.dtype} {list(mask.shape)} on {mask.device}")
            mask = mask.data_ptr()
        nz, ny, nx = ((1,) + shape) if dim == 2 else shape
        org = f64(list(origin) + [0.0] * (3 - dim))
        self._ck(self.lib.gpmp2mi_scene_rasterize_dev(scene.ptr, dim, dptr(org), float(cell_size), nx, ny, nz,
                                                      C.c_void_p(int(mask)), _dev_arg("cells", cells, (scene.K,), True),
                                                      C.c_void_p(stream or 0)))

    def scene_timing(self, scene, on=True, read=False):
        """Stage timer of the rasterisation (gpmp2mi_debug_scene_timing): read = True returns the device times in ms of
        the last recorded call as dict(primitives, meshes)."""
        ms = np.zeros(2) if read else None
        self._ck(self.lib.gpmp2mi_debug_scene_timing(scene.ptr, int(bool(on)), dptr(ms)))
        return None if ms is None else dict(zip(("primitives", "meshes"), (float(x) for x in ms)))
