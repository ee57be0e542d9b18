"""ctypes binding of liblisflood_amd.so (C ABI: include/lisflood_amd.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "liblisflood_amd.so"
_lib = None

LF_OK = 0
LF_E_INVALID, LF_E_CYCLE, LF_E_NO_DEVICE, LF_E_HIP, LF_E_SECTION, LF_E_COMM = -1, -2, -3, -4, -5, -6
SECTION = {"main_channel": 0, "floodplains": 1}


# Every function of include/lisflood_amd.h by signature: one letter per parameter (p pointer or array, i int, u unsigned
# int, q int64_t, z size_t, d double), then ">" and the return kind where it is not int (q, v void, s const char *);
# names without their lf_ prefix.  lib() declares them all to ctypes, so call sites pass plain Python values and a value
# of the wrong kind is an ArgumentError instead of a truncated argument.  tests/test_host_cpu.py holds the table to the
# header, prototype by prototype.
_KIND = {"p": C.c_void_p, "i": C.c_int, "u": C.c_uint, "q": C.c_int64, "z": C.c_size_t, "d": C.c_double,
         "v": None, "s": C.c_char_p}
_SIGNATURES = {
    "": "version",
    "i": "side_stream_begin side_stream_end side_stream_join lane_fork lane_join device_trim "
         "device_synchronize timer_start soil_last_form",
    "ii": "upload_begin upload_end upload_wait compute_acquire compute_release lane_select module_last_form "
          "report_acquire download_begin download_end download_wait",
    "iippppppppqd": "pack_rasters_device",
    "iippq": "calibration_streams",
    "iiqp": "substep_stage",
    "ip": "device_free host_free timer_stop canopy_device soil_pf_device inloop_structures "
          "pixel_aggregates_device interception_host soil_columns_host interception_device soil_columns_device "
          "soil_columns_device_derived soil_last_deferred",
    "ipi": "soil_substep_histogram",
    "ipiiqq": "soil_columns_members_device",
    "ipiqqdpqipp": "members_order_statistics_device",
    "ipiqqdiiqpppipqpp": "members_track_device",
    "ipiqqdpqpppipqp": "members_summary_device",
    "ipiqdqppqppq": "members_zonal_device",
    "ipiqqippppdpd": "members_regress_device",
    "ipiqqp": "members_resample_device",
    "ipiqqpipqpipdpd": "members_perturb_device upload_perturb_rows",
    "ipiqqpppdpd": "members_transform_device",
    "ipiqqq": "pixel_aggregates_members_device snow_frost_members_device",
    "ipiz": "memset",
    "ippii": "lddrepair_raster_device",
    "ipppi": "land_columns_device",
    "ipppiiqq": "land_columns_members_device",
    "ipppii": "router_route_device_multi upstream_sum_raster_device lddmask_raster_device ldd_raster_host",
    "ipppqq": "scale_rows_device",
    "ipppiqi": "router_route_ordered_members_multi",
    "ippqi": "calibration_copy",
    "ippz": "memcpy_h2d memcpy_h2d_staged upload_copy upload_copy_f32 memcpy_d2h memcpy_d2d download_copy",
    "ipqipiiqp": "upload_rows",
    "ipqp": "count_nonfinite",
    "ipz": "device_name",
    "iqppp": "gather_device",
    "iqppqpqi": "gather_rows_device",
    "iup": "xcd_contiguous_order",
    "izp": "device_alloc host_alloc",
    "p": "struct_sizes device_count graph_max_upstream router_device router_reset_site_cache router_last_fused_form "
         "dist_router_last_fused_form dist_graph_local_num_phases dist_graph_num_phases comm_unique_id comm_close",
    "pi": "router_profile_enable dist_graph_finalize",
    "piiip": "comm_create",
    "piip": "dist_graph_round_send_positions dist_fused_halo_block dist_graph_part_range",
    "pip": "dist_graph_phase_range dist_graph_round_counts dist_fused_slab",
    "pipp": "catchment_totals_multi_device catchment_totals_multi_host accuflux_ordered_multi_device "
            "dist_router_recv_slots",
    "piqip": "graph_block_plan_stats graph_block_plan_check",
    "pp": "graph_get_links router_last_launches router_route_plan_stats routing_substep dist_graph_counts "
          "dist_graph_slab_layout dist_graph_block_stats dist_graph_get_ups_base",
    "ppdpddpip": "router_create dist_router_create",
    "ppi": "router_profile_read dist_fused_prepare",
    "ppiiii": "dist_fused_exchange",
    "ppiip": "graph_create graph_create_raster",
    "ppiipp": "graph_create_ex",
    "ppiippppp": "dist_graph_create",
    "ppiiq": "routing_model_steps_fused",
    "ppiiqi": "dist_fused_phase_model_steps",
    "ppipp": "dist_router_pack",
    "ppiq": "routing_substeps_fused",
    "ppiqi": "dist_fused_phase",
    "ppiqiqq": "routing_substeps_fused_members",
    "ppp": "graph_get_orders router_to_engine_order router_from_engine_order upstream_sum_device "
           "upstream_sum_host accuflux_host accuflux_ordered_device downstream_device downstream_host "
           "catchments_device catchments catchment_totals_device catchment_totals_host "
           "dist_graph_get_export_phases dist_graph_get_layout dist_router_to_engine_order "
           "dist_router_from_engine_order dist_graph_get_fused_tables",
    "pppi": "router_route_host router_route_device router_route_ordered routing_substeps_fused_structures",
    "pppii": "dist_routing_substep dist_router_compute_phase router_route_members_host",
    "pppiii": "dist_router_compute_part dist_router_exchange",
    "pppiiqqqq": "routing_substeps_fused_structures_members",
    "pppiiqii": "dist_routing_model_steps_fused",
    "pppiqi": "router_route_ordered_members",
    "pppiqii": "dist_routing_substeps_fused",
    "pppp": "graph_get_lookups graph_get_layout surface_step surface_step_ordered dist_graph_set_ghost_phases "
            "dist_graph_get_csr",
    "ppppiii": "dist_router_route dist_router_compute_part_io",
    "ppppiqq": "surface_step_members",
    "ppppiiii": "dist_router_route_many",
    "ppppppp": "dist_graph_get_fused_plan",
    "pppppppp": "dist_graph_get_route_plan",
    "qipqpppqppppppp": "site_plan",
    "qiqpp": "land_members_unit module_members_unit",
    "p>q": "graph_num_pixels graph_num_levels router_num_pixels dist_graph_num_pixels dist_graph_state_size "
           "dist_graph_num_launch_units dist_graph_num_noncontiguous dist_router_state_size "
           "dist_router_last_launches",
    "pii>q": "dist_graph_round_recv_slot",
    "iqiiqi>q": "fused_members_slice",
    ">s": "last_error",
    "p>v": "graph_destroy router_destroy dist_graph_destroy comm_destroy dist_router_destroy",
}


class LisfloodAmdError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("lisflood_amd error %d: %s" % (code, message))
        self.code = code


def library_path():
    """In-tree build by default; LISFLOOD_AMD_LIBRARY overrides (an alternative build of the same C ABI)."""
    return os.environ.get("LISFLOOD_AMD_LIBRARY") or os.path.join(_HERE, _LIBNAME)


def lib():
    """The loaded HIP library.  Fails loudly when it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise LisfloodAmdError(LF_E_NO_DEVICE, "%s not found - build it with `make -C lisflood-code_amd` "
                                   "(or __graft_entry__.build()); lisflood_amd has no CPU fallback" % path)
        L = C.CDLL(path)
        for sig, names in _SIGNATURES.items():
            args, _, ret = sig.partition(">")
            for name in names.split():
                try:
                    f = getattr(L, "lf_" + name)
                except AttributeError:
                    raise LisfloodAmdError(LF_E_INVALID, "%s does not export lf_%s" % (path, name)) from None
                f.argtypes, f.restype = [_KIND[k] for k in args], _KIND[ret or "i"]
        _lib = L
    return _lib


def check(rc):
    if rc != LF_OK:
        raise LisfloodAmdError(rc, lib().lf_last_error().decode("utf-8", "replace"))


def ptr(a):
    """void* of a numpy array (keeps the array alive through the returned object) or None."""
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def u8(a):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8) if a.flags.c_contiguous else a.astype(np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def _host(a):
    """C-contiguous host array as the device holds it: flags go up as uint8 (a view, no copy)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a


def _shape(shape):
    return shape if isinstance(shape, tuple) else tuple(np.atleast_1d(shape).tolist())


def device_count():
    n = C.c_int(0)
    check(lib().lf_device_count(C.byref(n)))
    return n.value


def device_name(device=0):
    buf = C.create_string_buffer(256)
    check(lib().lf_device_name(device, buf, 256))
    return buf.value.decode()


class PinnedArray:
    """numpy array in page-locked host memory (lf_host_alloc): `.a` is an ordinary ndarray to fill in place; uploads from
    it are asynchronous DMA.  Keep the object alive as long as `.a` is in use."""

    def __init__(self, shape, dtype=np.float64, device=0):
        self.device = device
        shape = _shape(shape)
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(lib().lf_host_alloc(device, n, C.byref(p)))
        self.ptr = C.c_void_p(p.value)
        self.a = np.frombuffer((C.c_char * max(n, 1)).from_address(p.value), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            self.a = None
            lib().lf_host_free(self.device, self.ptr)
            self.ptr = C.c_void_p(None)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceArray:
    """fp64 / uint8 vector resident in HBM (thin RAII wrapper over lf_device_alloc)."""

    def __init__(self, shape, dtype=np.float64, device=0):
        self.shape = _shape(shape)
        self.dtype = np.dtype(dtype)
        self.device = device
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().lf_device_alloc(device, self.nbytes, C.byref(p)))
        self.ptr = C.c_void_p(p.value)

    @classmethod
    def from_host(cls, a, device=0):
        a = _host(a)
        return cls(a.shape, a.dtype, device).upload(a)

    def upload(self, a, staged=False, prefix=False):
        """host array -> device.  prefix: a shorter `a` goes into the first entries and the rest stays as it is.  staged: do
        not wait for the device (lf_memcpy_h2d_staged): `a` is copied to a page-locked staging slot of the library before the
        call returns; the DMA runs in order on the stream the library calls currently go to"""
        a = _host(a)
        assert a.dtype == self.dtype and (a.nbytes == self.nbytes or prefix and a.nbytes < self.nbytes), \
            (a.shape, a.dtype, self.shape, self.dtype)
        copy = lib().lf_memcpy_h2d_staged if staged else lib().lf_memcpy_h2d
        check(copy(self.device, self.ptr, ptr(a), a.nbytes))
        return self

    def download(self, out=None):
        if out is None:
            out = np.empty(self.shape, self.dtype)
        assert out.nbytes == self.nbytes and out.flags.c_contiguous
        check(lib().lf_memcpy_d2h(self.device, ptr(out), self.ptr, self.nbytes))
        return out

    def copy_from(self, other):
        assert other.nbytes == self.nbytes
        check(lib().lf_memcpy_d2d(self.device, self.ptr, other.ptr, self.nbytes))
        return self

    def zero(self):
        check(lib().lf_memset(self.device, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            lib().lf_device_free(self.device, self.ptr)
            self.ptr = C.c_void_p(None)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BufferCache:
    """Device buffers of a module instance, kept between calls: `put(name, host)` uploads into the buffer of that name
    (allocated once, re-allocated only when shape or dtype change), `zeros(name, shape)` hands out a scratch buffer.
    The drop-in module classes stage their `var` arrays through the host on every call, as the reference's contract
    requires (other modules may have changed them); the allocations themselves are not repeated."""

    def __init__(self, device=0):
        self.device, self.buf = device, {}

    def get(self, name, shape, dtype=np.float64):
        shape = _shape(shape)
        d = self.buf.get(name)
        if d is None or d.shape != shape or d.dtype != np.dtype(dtype):
            if d is not None:
                d.free()
            d = self.buf[name] = DeviceArray(shape, dtype, self.device)
        return d

    def put(self, name, host):
        host = _host(host)
        return self.get(name, host.shape, host.dtype).upload(host)

    @staticmethod
    def _fingerprint(host):
        """identity of a host array's CONTENT: shape, dtype and a position-sensitive checksum over EVERY byte (CRC-32 and
        Adler-32 of the buffer, zlib: one pass each, cheaper than the staging copy and the PCIe transfer they save).  An
        in-place edit of any element changes it, and so does any reordering of the same values (a map re-compressed in
        another pixel order, two elements swapped) -- the order-blind sum / xor pair of round 4 did not see those."""
        import zlib
        b = memoryview(host.reshape(-1).view(np.uint8))
        return (host.shape, host.dtype.str, zlib.crc32(b), zlib.adler32(b))

    def put_static(self, name, host):
        """`put` for parameters that do not change between calls (soil and crop parameter maps, calibration constants):
        the upload is skipped while the array's content checksum is the one of the last upload.  Maps the reference
        itself rewrites during a run (the land-use fractions: landusechange.py:107-139, evapowater.py:108-119) do not
        come through here at all.  static_uploads = False switches the check off."""
        host = _host(host)
        if not getattr(self, "static_uploads", True):
            return self.put(name, host)
        fp = self._fingerprint(host)
        seen = self.__dict__.setdefault("_static_fp", {})
        d = self.buf.get(name)
        if d is not None and seen.get(name) == fp and d.shape == host.shape and d.dtype == host.dtype:
            return d
        d = self.put(name, host)
        seen[name] = fp
        return d

    def invalidate_static(self):
        self.__dict__["_static_fp"] = {}

    def free(self):
        for d in self.buf.values():
            d.free()
        self.buf = {}
        self.invalidate_static()


def synchronize(device=0):
    check(lib().lf_device_synchronize(device))


def timer_start(device=0):
    check(lib().lf_timer_start(device))


def timer_stop(device=0):
    ms = C.c_double(0.0)
    check(lib().lf_timer_stop(device, C.byref(ms)))
    return ms.value
