"""sdr-server_amd -- MI355X-native implementation of sdr-server's frequency-xlating FIR hot path.

The product is the C-ABI shared library `lib/libxlating_hip.so` (sources in csrc/, headers in ../include/):
hand-written HIP kernels for gfx950 behind the reference's own `xlating.h` / `lpf.h` API plus the batched
fan-out API of `xlating_batch.h`.  This Python package is only a thin ctypes host used by the tests and by
bench.py; it mirrors the reference interface one to one (same names, argument meaning, error behaviour):

    code, taps = create_low_pass_filter(1.0, 2016000, 24000, 9600)          # src/lpf.h:6
    f = XlatingFilter(42, taps, -12000, 2016000, 262144)                    # create_frequency_xlating_filter
    y = f.process("native", "cu8", "cf32", block)                           # process_native_cu8_cf32
    f.close()                                                               # destroy_xlating

There is NO CPU arithmetic path: if the library or a HIP device is missing, construction raises.
(The directory name contains '-'; import it through the top-level alias module `sdr_server_amd`.)
"""
import ctypes as C
import os

import numpy as np

from .build import build_library, library_path


class WireRequest(C.Structure):
    """include/xlating_wire.h xlating_wire_request"""
    _fields_ = [("center_freq", C.c_uint32), ("sampling_rate", C.c_uint32), ("band_freq", C.c_uint32), ("destination", C.c_uint8)]


class WireAdmission(C.Structure):
    """include/xlating_wire.h xlating_wire_admission"""
    _fields_ = [("decimation", C.c_uint32), ("center_offset", C.c_int32), ("lpf_cutoff", C.c_uint32), ("lpf_transition", C.c_uint32)]


class WireResample(C.Structure):
    """include/xlating_wire.h xlating_wire_resample"""
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("virtual_rate", C.c_uint32)]


_c_float_p = C.POINTER(C.c_float)
_c_i16_p = C.POINTER(C.c_int16)

FMT = {"cu8": 0, "cs8": 1, "cs16": 2, "cf32": 3}
MODE = {"native": 0, "optimized": 1, "q15": 2, "optimized_x86": 3, "optimized_x86_fma": 4}
_NP = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16, "cf32": np.float32}
_CT = {"cu8": C.c_uint8, "cs8": C.c_int8, "cs16": C.c_int16, "cf32": C.c_float}

# every symbol include/xlating.h, include/lpf.h and include/xlating_batch.h declare
EXPORTED_SYMBOLS = (
    ["SIMD_STATUS", "create_frequency_xlating_filter", "destroy_xlating", "create_low_pass_filter"]
    + [f"process_{v}_{i}_{o}" for v in ("native", "optimized") for i in ("cu8", "cs8", "cs16") for o in ("cf32", "cs16")]
    + ["process_native_cf32_cf32", "process_optimized_cf32_cf32", "xlating_set_optimized_x86"]
    + ["xlating_batch_create", "xlating_batch_create_grouped", "xlating_batch_set_option", "xlating_batch_q15_matrix_admits", "xlating_batch_process_host_group",
       "xlating_batch_process_device_group", "xlating_batch_process_device_group_ev", "xlating_batch_output_len_block", "xlating_batch_add_client", "xlating_batch_remove_client", "xlating_batch_num_clients",
       "xlating_batch_process_host", "xlating_batch_process_device", "xlating_batch_output_len", "xlating_batch_fetch",
       "xlating_batch_output_host", "xlating_batch_output_host_cs16", "xlating_batch_output_device", "xlating_batch_outputs_device", "xlating_batch_client_phase", "xlating_batch_client_phase_q15", "xlating_batch_sync",
       "xlating_batch_query", "xlating_batch_record_event", "xlating_batch_timing", "xlating_batch_timing_read", "xlating_batch_timing_polyphase", "xlating_batch_timing_stride", "xlating_batch_describe", "xlating_batch_destroy",
       "xlating_hip_device_info"]
    + ["xlating_sinks_create", "xlating_sinks_attach_fd", "xlating_sinks_attach_file", "xlating_sinks_write",
       "xlating_sinks_submit", "xlating_sinks_failed", "xlating_sinks_flush", "xlating_sinks_detach", "xlating_sinks_stats",
       "xlating_sinks_destroy", "xlating_sinks_attach_file_as", "xlating_sinks_write_bytes"]
    + ["xlating_wire_parse_header", "xlating_wire_parse_request", "xlating_wire_build_request", "xlating_wire_build_response",
       "xlating_wire_build_header", "xlating_wire_parse_response", "xlating_wire_admit", "xlating_wire_add_client",
       "xlating_wire_admit_any_rate", "xlating_wire_resample_taps"]
)

MULTI_SYMBOLS = ["xlating_multi_unique_id", "xlating_multi_create_rank", "xlating_multi_create_local", "xlating_multi_world",
                 "xlating_multi_local", "xlating_multi_add_client", "xlating_multi_engine", "xlating_multi_feed",
                 "xlating_multi_feed_done", "xlating_multi_feed_query", "xlating_multi_feed_wait_on_stream",
                 "xlating_multi_feed_timing", "xlating_multi_feed_timing_read", "xlating_multi_comm_count",
                 "xlating_multi_sync", "xlating_multi_destroy"]

_lib = None
_mlib = None


def multi_library_path():
    return os.path.join(os.path.dirname(library_path()), "libxlating_multi.so")


def multi_lib():
    """include/xlating_multi.h: the C host of the multi-GPU path (engines + RCCL broadcast).  Loads librccl."""
    global _mlib
    if _mlib is not None:
        return _mlib
    lib()
    path = multi_library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    M = C.CDLL(path)
    M.xlating_multi_unique_id.argtypes = [C.c_void_p]
    M.xlating_multi_unique_id.restype = C.c_int
    M.xlating_multi_create_rank.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint, C.c_int,
                                            C.POINTER(C.c_void_p)]
    M.xlating_multi_create_rank.restype = C.c_int
    M.xlating_multi_create_local.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_uint32, C.c_int, C.c_uint32, C.c_uint,
                                             C.POINTER(C.c_void_p)]
    M.xlating_multi_create_local.restype = C.c_int
    M.xlating_multi_world.argtypes = [C.c_void_p]
    M.xlating_multi_world.restype = C.c_int
    M.xlating_multi_local.argtypes = [C.c_void_p]
    M.xlating_multi_local.restype = C.c_int
    M.xlating_multi_add_client.argtypes = [C.c_void_p, C.c_int, C.c_uint32, _c_float_p, C.c_size_t, C.c_int32]
    M.xlating_multi_add_client.restype = C.c_int
    M.xlating_multi_engine.argtypes = [C.c_void_p, C.c_int]
    M.xlating_multi_engine.restype = C.c_void_p
    M.xlating_multi_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int]
    M.xlating_multi_feed.restype = C.c_int
    M.xlating_multi_sync.argtypes = [C.c_void_p]
    M.xlating_multi_sync.restype = C.c_int
    for name in ("xlating_multi_feed_done", "xlating_multi_feed_query"):
        getattr(M, name).argtypes = [C.c_void_p]
        getattr(M, name).restype = C.c_int
    M.xlating_multi_feed_wait_on_stream.argtypes = [C.c_void_p, C.c_void_p]
    M.xlating_multi_feed_wait_on_stream.restype = C.c_int
    M.xlating_multi_feed_timing.argtypes = [C.c_void_p, C.c_int]
    M.xlating_multi_feed_timing.restype = C.c_int
    M.xlating_multi_feed_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    M.xlating_multi_feed_timing_read.restype = C.c_int
    M.xlating_multi_comm_count.argtypes = [C.c_void_p]
    M.xlating_multi_comm_count.restype = C.c_int
    M.xlating_multi_destroy.argtypes = [C.c_void_p]
    M.xlating_multi_destroy.restype = None
    _mlib = M
    return M


def lib():
    """Load (never build) the in-tree shared library and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    # PyTorch bundles its own copy of the HIP runtime.  If this library (linked against /opt/rocm's) initialises HIP first
    # and torch is imported later in the same process, torch ends up on a second runtime that sees no GPU ("No HIP GPUs are
    # available"); with torch's copy loaded first both share it.  Tests and bench.py use torch for device buffers, so:
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional for this host; a pure C deployment never has this problem
        pass
    L = C.CDLL(path)
    L.create_low_pass_filter.argtypes = [C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_c_float_p), C.POINTER(C.c_size_t)]
    L.create_low_pass_filter.restype = C.c_int
    L.create_frequency_xlating_filter.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.create_frequency_xlating_filter.restype = C.c_int
    L.destroy_xlating.argtypes = [C.c_void_p]
    L.destroy_xlating.restype = None
    L.xlating_set_optimized_x86.argtypes = [C.c_void_p, C.c_int]
    L.xlating_set_optimized_x86.restype = C.c_int
    for v in ("native", "optimized"):
        for i in ("cu8", "cs8", "cs16", "cf32"):
            fn = getattr(L, f"process_{v}_{i}_cf32")
            fn.argtypes = [C.POINTER(_CT[i]), C.c_size_t, C.POINTER(_c_float_p), C.POINTER(C.c_size_t), C.c_void_p]
            fn.restype = None
            if i != "cf32":
                fn = getattr(L, f"process_{v}_{i}_cs16")
                fn.argtypes = [C.POINTER(_CT[i]), C.c_size_t, C.POINTER(_c_i16_p), C.POINTER(C.c_size_t), C.c_void_p]
                fn.restype = None
    L.xlating_batch_create.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    L.xlating_batch_create.restype = C.c_int
    L.xlating_batch_create_grouped.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_uint, C.c_int, C.POINTER(C.c_void_p)]
    L.xlating_batch_create_grouped.restype = C.c_int
    L.xlating_batch_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    L.xlating_batch_set_option.restype = C.c_int
    L.xlating_batch_q15_matrix_admits.argtypes = [C.c_uint32, _c_float_p, C.c_size_t, C.c_int32, C.c_uint32]
    L.xlating_batch_q15_matrix_admits.restype = C.c_int
    L.xlating_batch_process_host_group.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int]
    L.xlating_batch_process_host_group.restype = C.c_int
    L.xlating_batch_process_device_group.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p]
    L.xlating_batch_process_device_group.restype = C.c_int
    L.xlating_batch_output_len_block.argtypes = [C.c_void_p, C.c_int, C.c_uint]
    L.xlating_batch_output_len_block.restype = C.c_size_t
    L.xlating_batch_add_client.argtypes = [C.c_void_p, C.c_uint32, _c_float_p, C.c_size_t, C.c_int32]
    L.xlating_batch_add_client.restype = C.c_int
    L.xlating_batch_remove_client.argtypes = [C.c_void_p, C.c_int]
    L.xlating_batch_remove_client.restype = C.c_int
    L.xlating_batch_num_clients.argtypes = [C.c_void_p]
    L.xlating_batch_num_clients.restype = C.c_int
    L.xlating_batch_process_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.xlating_batch_process_host.restype = C.c_int
    L.xlating_batch_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.xlating_batch_process_device.restype = C.c_int
    L.xlating_batch_output_len.argtypes = [C.c_void_p, C.c_int]
    L.xlating_batch_output_len.restype = C.c_size_t
    L.xlating_batch_fetch.argtypes = [C.c_void_p]
    L.xlating_batch_fetch.restype = C.c_int
    L.xlating_batch_output_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(_c_float_p), C.POINTER(C.c_size_t)]
    L.xlating_batch_output_host.restype = C.c_int
    L.xlating_batch_output_host_cs16.argtypes = [C.c_void_p, C.c_int, C.POINTER(_c_i16_p), C.POINTER(C.c_size_t)]
    L.xlating_batch_output_host_cs16.restype = C.c_int
    L.xlating_batch_output_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.xlating_batch_output_device.restype = C.c_int
    L.xlating_batch_outputs_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.xlating_batch_outputs_device.restype = C.c_int
    L.xlating_batch_client_phase.argtypes = [C.c_void_p, C.c_int, _c_float_p, _c_float_p]
    L.xlating_batch_client_phase.restype = C.c_int
    L.xlating_batch_client_phase_q15.argtypes = [C.c_void_p, C.c_int, _c_i16_p, _c_i16_p]
    L.xlating_batch_client_phase_q15.restype = C.c_int
    L.xlating_batch_sync.argtypes = [C.c_void_p]
    L.xlating_batch_sync.restype = C.c_int
    L.xlating_batch_timing.argtypes = [C.c_void_p, C.c_int]
    L.xlating_batch_timing.restype = C.c_int
    L.xlating_batch_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    L.xlating_batch_timing_read.restype = C.c_int
    L.xlating_sinks_create.argtypes = [C.c_uint, C.c_size_t, C.POINTER(C.c_void_p)]
    L.xlating_sinks_create.restype = C.c_int
    L.xlating_sinks_attach_fd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.xlating_sinks_attach_fd.restype = C.c_int
    L.xlating_sinks_attach_file.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    L.xlating_sinks_attach_file.restype = C.c_int
    L.xlating_sinks_write.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.xlating_sinks_write.restype = C.c_int
    L.xlating_sinks_attach_file_as.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    L.xlating_sinks_attach_file_as.restype = C.c_int
    L.xlating_sinks_write_bytes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.xlating_sinks_write_bytes.restype = C.c_int
    L.xlating_sinks_submit.argtypes = [C.c_void_p, C.c_void_p]
    L.xlating_sinks_submit.restype = C.c_int
    L.xlating_sinks_failed.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t]
    L.xlating_sinks_failed.restype = C.c_size_t
    L.xlating_sinks_flush.argtypes = [C.c_void_p]
    L.xlating_sinks_flush.restype = C.c_int
    L.xlating_sinks_detach.argtypes = [C.c_void_p, C.c_int]
    L.xlating_sinks_detach.restype = C.c_int
    L.xlating_sinks_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.xlating_sinks_stats.restype = None
    L.xlating_sinks_destroy.argtypes = [C.c_void_p]
    L.xlating_sinks_destroy.restype = None
    L.xlating_wire_parse_header.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8)]
    L.xlating_wire_parse_header.restype = C.c_int
    L.xlating_wire_parse_request.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(WireRequest)]
    L.xlating_wire_parse_request.restype = C.c_int
    L.xlating_wire_build_request.argtypes = [C.POINTER(WireRequest), C.c_char_p]
    L.xlating_wire_build_request.restype = C.c_size_t
    L.xlating_wire_build_response.argtypes = [C.c_uint8, C.c_uint32, C.c_char_p]
    L.xlating_wire_build_response.restype = C.c_size_t
    L.xlating_wire_build_header.argtypes = [C.c_uint8, C.c_char_p]
    L.xlating_wire_build_header.restype = C.c_size_t
    L.xlating_wire_parse_response.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    L.xlating_wire_parse_response.restype = C.c_int
    L.xlating_wire_admit.argtypes = [C.POINTER(WireRequest), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(WireAdmission),
                                     C.POINTER(C.c_uint32)]
    L.xlating_wire_admit.restype = C.c_int
    L.xlating_wire_admit_any_rate.argtypes = [C.POINTER(WireRequest), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(WireAdmission),
                                              C.POINTER(WireResample), C.POINTER(C.c_uint32)]
    L.xlating_wire_admit_any_rate.restype = C.c_int
    L.xlating_wire_resample_taps.argtypes = [C.POINTER(WireRequest), C.POINTER(WireResample), C.c_uint32, C.POINTER(_c_float_p),
                                             C.POINTER(C.c_size_t)]
    L.xlating_wire_resample_taps.restype = C.c_int
    L.xlating_wire_add_client.argtypes = [C.c_void_p, C.POINTER(WireAdmission), C.c_uint32]
    L.xlating_wire_add_client.restype = C.c_int
    L.xlating_batch_timing_stride.argtypes = [C.c_void_p, C.c_uint]
    L.xlating_batch_timing_stride.restype = C.c_int
    L.xlating_batch_timing_polyphase.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.xlating_batch_timing_polyphase.restype = C.c_int
    L.xlating_batch_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.xlating_batch_describe.restype = C.c_int
    L.xlating_batch_destroy.argtypes = [C.c_void_p]
    L.xlating_batch_destroy.restype = None
    L.xlating_hip_device_info.argtypes = []
    L.xlating_hip_device_info.restype = C.c_char_p
    _lib = L
    return L


_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]
_libc.free.argtypes = [C.c_void_p]


def simd_status():
    """The exported SIMD_STATUS string (reference src/xlating.c:145-268; printed by src/main.c:23)."""
    return C.c_char_p.in_dll(lib(), "SIMD_STATUS").value.decode()


def device_info():
    return lib().xlating_hip_device_info().decode()


def create_low_pass_filter(gain, sampling_freq, cutoff_freq, transition_width):
    """reference src/lpf.h:6 -> (code, float32 taps | None)"""
    p = _c_float_p()
    n = C.c_size_t(0)
    code = lib().create_low_pass_filter(gain, sampling_freq, cutoff_freq, transition_width, C.byref(p), C.byref(n))
    if code != 0:
        return code, None
    taps = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    _libc.free(p)
    return 0, taps


class XlatingError(RuntimeError):
    def __init__(self, what, code):
        super().__init__(f"{what} failed with code {code}")
        self.code = code


def q15_matrix_admits(decimation, taps, center_freq, sampling_freq):
    """Would a Q15 call of an engine with option "q15_kernel" = 1 filter this client on the matrix cores?  (Host code only: no device.)"""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    return bool(lib().xlating_batch_q15_matrix_admits(int(decimation), taps.ctypes.data_as(_c_float_p), taps.size, int(center_freq),
                                                      int(sampling_freq)))


class XlatingFilter:
    """One `xlating *` handle (reference src/xlating.h:8-38)."""

    def __init__(self, decimation, taps, center_freq, sampling_freq, max_input_buffer_length):
        L = lib()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        # create() takes ownership of a malloc'd taps array (xlating.c:508, freed at :600-602)
        buf = _libc.malloc(max(4, taps.nbytes))
        C.memmove(buf, taps.ctypes.data, taps.nbytes)
        h = C.c_void_p()
        code = L.create_frequency_xlating_filter(decimation, buf, taps.size, center_freq, sampling_freq,
                                                 max_input_buffer_length, C.byref(h))
        if code != 0:
            if code == -1:  # taps_len == 0: taps not consumed (xlating.c:496-498)
                _libc.free(buf)
            raise XlatingError("create_frequency_xlating_filter", code)
        self.h = h
        self.D = decimation

    def process(self, variant, in_fmt, out_fmt, x):
        """process_<variant>_<in_fmt>_<out_fmt>(x) -> complex64[K] (cf32) or int16[K, 2] (cs16).
        x: 1-D array of scalar elements (I,Q interleaved); len(x) is the C API's input_len."""
        x = np.ascontiguousarray(x, dtype=_NP[in_fmt])
        fn = getattr(lib(), f"process_{variant}_{in_fmt}_{out_fmt}")
        n = C.c_size_t(0)
        if out_fmt == "cf32":
            p = _c_float_p()
            fn(x.ctypes.data_as(C.POINTER(_CT[in_fmt])), x.size, C.byref(p), C.byref(n), self.h)
            if n.value == 0:
                return np.zeros(0, np.complex64)
            return np.ctypeslib.as_array(p, shape=(2 * n.value,)).copy().view(np.complex64)
        p = _c_i16_p()
        fn(x.ctypes.data_as(C.POINTER(_CT[in_fmt])), x.size, C.byref(p), C.byref(n), self.h)
        if n.value == 0:
            return np.zeros((0, 2), np.int16)
        return np.ctypeslib.as_array(p, shape=(n.value, 2)).copy()

    def set_optimized_x86(self, on=1):
        """process_optimized_* follows the reference's x86 AVX build: the phase is never renormalised (xlating.c:338-339);
        on = 2: the build compiled with FMA (its contracted phase step)."""
        code = lib().xlating_set_optimized_x86(self.h, int(on))
        if code != 0:
            raise XlatingError("xlating_set_optimized_x86", code)

    def close(self):
        if getattr(self, "h", None):
            lib().destroy_xlating(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchEngine:
    """`xlating_batch *` (include/xlating_batch.h): one IQ stream, many clients, one GPU."""

    def __init__(self, sampling_freq, in_fmt, max_input_buffer_length, device=-1, group_blocks=1):
        h = C.c_void_p()
        code = lib().xlating_batch_create_grouped(sampling_freq, FMT[in_fmt], max_input_buffer_length, group_blocks, device,
                                                  C.byref(h))
        if code != 0:
            raise XlatingError("xlating_batch_create", code)
        self.h = h
        self.in_fmt = in_fmt

    def set_option(self, name, value):
        code = lib().xlating_batch_set_option(self.h, name.encode(), int(value))
        if code != 0:
            raise XlatingError(f"xlating_batch_set_option({name})", code)

    def process_host_group(self, x, nblocks, variant="native"):
        """x holds nblocks equal blocks back to back; results == nblocks successive process_host calls."""
        x = np.ascontiguousarray(x, dtype=_NP[self.in_fmt])
        assert x.size % nblocks == 0
        code = lib().xlating_batch_process_host_group(self.h, x.ctypes.data, x.size // nblocks, nblocks, MODE[variant])
        if code != 0:
            raise XlatingError("xlating_batch_process_host_group", code)

    def process_device_group(self, d_ptr, input_len, nblocks, variant="native", stream=0):
        """stream: a hipStream_t value, 0 (HIP's default stream) or "engine" (XL_STREAM_ENGINE: the engine's own compute
        stream, CU-masked for calls whose NCO chain runs on the side stream; wait with sync())."""
        sp = C.c_void_p(-1) if stream == "engine" else (C.c_void_p(stream) if stream else None)
        code = lib().xlating_batch_process_device_group(self.h, C.c_void_p(d_ptr), input_len, nblocks, MODE[variant], sp)
        if code != 0:
            raise XlatingError("xlating_batch_process_device_group", code)

    def output_len_block(self, cid, block):
        return lib().xlating_batch_output_len_block(self.h, cid, block)

    def add_client(self, decimation, taps, center_freq):
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        cid = lib().xlating_batch_add_client(self.h, decimation, taps.ctypes.data_as(_c_float_p), taps.size, center_freq)
        if cid < 0:
            raise XlatingError("xlating_batch_add_client", cid)
        return cid

    def remove_client(self, cid):
        code = lib().xlating_batch_remove_client(self.h, cid)
        if code != 0:
            raise XlatingError("xlating_batch_remove_client", code)

    @property
    def num_clients(self):
        return lib().xlating_batch_num_clients(self.h)

    def process_host(self, x, variant="native"):
        x = np.ascontiguousarray(x, dtype=_NP[self.in_fmt])
        code = lib().xlating_batch_process_host(self.h, x.ctypes.data, x.size, MODE[variant])
        if code != 0:
            raise XlatingError("xlating_batch_process_host", code)

    def process_device(self, d_ptr, input_len, variant="native", stream=0):
        code = lib().xlating_batch_process_device(self.h, C.c_void_p(d_ptr), input_len, MODE[variant],
                                                  C.c_void_p(stream) if stream else None)
        if code != 0:
            raise XlatingError("xlating_batch_process_device", code)

    def fetch(self):
        code = lib().xlating_batch_fetch(self.h)
        if code != 0:
            raise XlatingError("xlating_batch_fetch", code)

    def output(self, cid):
        p = _c_float_p()
        n = C.c_size_t(0)
        code = lib().xlating_batch_output_host(self.h, cid, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError("xlating_batch_output_host", code)
        if n.value == 0:
            return np.zeros(0, np.complex64)
        return np.ctypeslib.as_array(p, shape=(2 * n.value,)).copy().view(np.complex64)

    def output_cs16(self, cid):
        """After a "q15" call + fetch(): int16[K, 2]."""
        p = _c_i16_p()
        n = C.c_size_t(0)
        code = lib().xlating_batch_output_host_cs16(self.h, cid, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError("xlating_batch_output_host_cs16", code)
        if n.value == 0:
            return np.zeros((0, 2), np.int16)
        return np.ctypeslib.as_array(p, shape=(n.value, 2)).copy()

    def output_len(self, cid):
        return lib().xlating_batch_output_len(self.h, cid)

    def output_device(self, cid):
        p = C.c_void_p()
        n = C.c_size_t(0)
        code = lib().xlating_batch_output_device(self.h, cid, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError("xlating_batch_output_device", code)
        return p.value, n.value

    def outputs_device(self, cids):
        """-> (device pointers uint64 [n], lengths uint64 [n]): output_device of every listed client, in one call"""
        a = np.ascontiguousarray(cids, dtype=np.intc)
        p, n = np.zeros(a.size, np.uint64), np.zeros(a.size, np.uint64)
        code = lib().xlating_batch_outputs_device(self.h, a.size, a.ctypes.data, p.ctypes.data, n.ctypes.data)
        if code != 0:
            raise XlatingError("xlating_batch_outputs_device", code)
        return p, n

    def phase(self, cid):
        a, b = C.c_float(), C.c_float()
        code = lib().xlating_batch_client_phase(self.h, cid, C.byref(a), C.byref(b))
        if code != 0:
            raise XlatingError("xlating_batch_client_phase", code)
        return np.float32(a.value), np.float32(b.value)

    def phase_q15(self, cid):
        """The client's committed Q15 phase (re, im) after the latest processed call."""
        a, b = C.c_int16(), C.c_int16()
        code = lib().xlating_batch_client_phase_q15(self.h, cid, C.byref(a), C.byref(b))
        if code != 0:
            raise XlatingError("xlating_batch_client_phase_q15", code)
        return int(a.value), int(b.value)

    def sync(self):
        code = lib().xlating_batch_sync(self.h)
        if code != 0:
            raise XlatingError("xlating_batch_sync", code)

    def record_event(self, event):
        """Record `event` (a hipEvent_t value, e.g. torch.cuda.Event().cuda_event after a first record) behind the latest call's
        launches, on the stream(s) they ran on: how another stream waits for a call made on stream="engine"."""
        L = lib()
        L.xlating_batch_record_event.argtypes = [C.c_void_p, C.c_void_p]
        L.xlating_batch_record_event.restype = C.c_int
        code = L.xlating_batch_record_event(self.h, C.c_void_p(event))
        if code != 0:
            raise XlatingError("xlating_batch_record_event", code)

    def timing(self, enable):
        """False/0 off, True/1 bracket every block's launches, 2 also time the three polyphase launches separately."""
        lib().xlating_batch_timing(self.h, int(enable))

    def timing_stride(self, every_n):
        """Bracket only every n-th block with events (an event pair costs a few us of stream time)."""
        lib().xlating_batch_timing_stride(self.h, int(every_n))

    def timing_polyphase(self, reset=True):
        """-> (n_timed_blocks, [forward_ms_total, mix_ms_total, inverse_ms_total]) -- needs timing(2)"""
        a = (C.c_double * 3)()
        n = lib().xlating_batch_timing_polyphase(self.h, a, 1 if reset else 0)
        if n < 0:
            raise XlatingError("xlating_batch_timing_polyphase", n)
        return n, [a[0], a[1], a[2]]

    def describe(self):
        """The resident plan in one line (which classes take which arithmetic path)."""
        buf = C.create_string_buffer(1024)
        n = lib().xlating_batch_describe(self.h, buf, 1024)
        if n < 0:
            raise XlatingError("xlating_batch_describe", n)
        return buf.value.decode()

    def timing_read(self, reset=True):
        """-> (n_timed_blocks, fir_ms_total, nco_ms_total)"""
        a, b = C.c_double(0), C.c_double(0)
        n = lib().xlating_batch_timing_read(self.h, C.byref(a), C.byref(b), 1 if reset else 0)
        if n < 0:
            raise XlatingError("xlating_batch_timing_read", n)
        return n, a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            lib().xlating_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiHost:
    """`xlating_multi *` (include/xlating_multi.h): the C host of the multi-GPU path.  One process per GPU
    (rank / world / 128-byte id from `MultiHost.unique_id()` on rank 0) or one process driving `ngpus` GPUs."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        code = multi_lib().xlating_multi_unique_id(buf)
        if code != 0:
            raise XlatingError("xlating_multi_unique_id", code)
        return buf.raw

    def __init__(self, sampling_freq, in_fmt, max_input_buffer_length, group_blocks=1, rank=0, world=1, uid=None, device=-1,
                 ngpus=None):
        h = C.c_void_p()
        M = multi_lib()
        if ngpus is not None:
            code = M.xlating_multi_create_local(ngpus, None, sampling_freq, FMT[in_fmt], max_input_buffer_length, group_blocks,
                                                C.byref(h))
        else:
            idbuf = C.create_string_buffer(uid, 128) if uid is not None else None
            code = M.xlating_multi_create_rank(rank, world, idbuf, sampling_freq, FMT[in_fmt], max_input_buffer_length,
                                               group_blocks, device, C.byref(h))
        if code != 0:
            raise XlatingError("xlating_multi_create", code)
        self.h = h
        self.in_fmt = in_fmt
        self.world = M.xlating_multi_world(h)

    def engine(self, gpu):
        """The BatchEngine of job GPU `gpu` if this process drives it (owned by the host: do not close it)."""
        p = multi_lib().xlating_multi_engine(self.h, gpu)
        if not p:
            return None
        e = BatchEngine.__new__(BatchEngine)
        e.h = C.c_void_p(p)
        e.in_fmt = self.in_fmt
        e.close = lambda: None
        return e

    def add_client(self, global_client, decimation, taps, center_freq):
        """-> engine-local client id, or None when another process drives the client's GPU (global_client mod world)."""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        cid = multi_lib().xlating_multi_add_client(self.h, global_client, decimation, taps.ctypes.data_as(_c_float_p), taps.size,
                                                   center_freq)
        if cid == -2:
            return None
        if cid < 0:
            raise XlatingError("xlating_multi_add_client", cid)
        return cid

    def feed(self, d_src, input_len, nblocks, variant="optimized"):
        code = multi_lib().xlating_multi_feed(self.h, C.c_void_p(d_src) if d_src else None, input_len, nblocks, MODE[variant])
        if code != 0:
            raise XlatingError("xlating_multi_feed", code)

    def feed_done(self):
        """Block until the source buffer of the latest feed may be overwritten (xlating_multi_feed_done)."""
        code = multi_lib().xlating_multi_feed_done(self.h)
        if code != 0:
            raise XlatingError("xlating_multi_feed_done", code)

    def feed_query(self):
        code = multi_lib().xlating_multi_feed_query(self.h)
        if code < 0:
            raise XlatingError("xlating_multi_feed_query", code)
        return bool(code)

    def feed_wait_on_stream(self, stream=0):
        code = multi_lib().xlating_multi_feed_wait_on_stream(self.h, C.c_void_p(stream) if stream else None)
        if code != 0:
            raise XlatingError("xlating_multi_feed_wait_on_stream", code)

    def feed_timing(self, enable=True):
        """Bracket every broadcast with HIP events on the communication stream (xlating_multi_feed_timing)."""
        code = multi_lib().xlating_multi_feed_timing(self.h, 1 if enable else 0)
        if code != 0:
            raise XlatingError("xlating_multi_feed_timing", code)

    def feed_timing_read(self, reset=True):
        """-> (feeds measured, broadcast ms in total, of which hidden behind the previous feed's filtering)."""
        b, hd = C.c_double(0.0), C.c_double(0.0)
        n = multi_lib().xlating_multi_feed_timing_read(self.h, C.byref(b), C.byref(hd), 1 if reset else 0)
        if n < 0:
            raise XlatingError("xlating_multi_feed_timing_read", n)
        return n, b.value, hd.value

    def comm_count(self):
        """Ranks of the RCCL communicator the host broadcasts over (0: none)."""
        n = multi_lib().xlating_multi_comm_count(self.h)
        if n < 0:
            raise XlatingError("xlating_multi_comm_count", n)
        return n

    def sync(self):
        code = multi_lib().xlating_multi_sync(self.h)
        if code != 0:
            raise XlatingError("xlating_multi_sync", code)

    def close(self):
        if getattr(self, "h", None):
            multi_lib().xlating_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sinks:
    """ctypes mirror of include/xlating_sinks.h (per-client output delivery of the batched path; host-only)."""

    def __init__(self, writer_threads=4, queue_bytes=16 * 25600):
        h = C.c_void_p()
        code = lib().xlating_sinks_create(writer_threads, queue_bytes, C.byref(h))
        if code != 0:
            raise XlatingError("xlating_sinks_create", code)
        self.h = h

    def attach_fd(self, client_id, fd, close_on_detach=False):
        return lib().xlating_sinks_attach_fd(self.h, client_id, fd, 1 if close_on_detach else 0)

    def attach_file(self, client_id, base_path, use_gzip=False):
        return lib().xlating_sinks_attach_file(self.h, client_id, str(base_path).encode(), 1 if use_gzip else 0)

    def attach_file_as(self, client_id, base_path, ext, use_gzip=False):
        """<base_path>/<client_id>.<ext>[.gz]; ext: "cf32" or "cs16" (any other: -EINVAL)"""
        return lib().xlating_sinks_attach_file_as(self.h, client_id, str(base_path).encode(), ext.encode(), 1 if use_gzip else 0)

    def write(self, client_id, samples):
        a = np.ascontiguousarray(samples, dtype=np.complex64)
        return lib().xlating_sinks_write(self.h, client_id, a.ctypes.data_as(C.c_void_p), a.size)

    def write_bytes(self, client_id, data):
        """data: bytes, or an array whose bytes are queued as they are"""
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        return lib().xlating_sinks_write_bytes(self.h, client_id, a.ctypes.data_as(C.c_void_p) if a.size else None, a.size)

    def submit(self, engine):
        return lib().xlating_sinks_submit(self.h, engine.h)

    def failed(self, cap=4096):
        ids = (C.c_int * cap)()
        n = lib().xlating_sinks_failed(self.h, ids, cap)
        return [ids[i] for i in range(n)]

    def flush(self):
        return lib().xlating_sinks_flush(self.h)

    def detach(self, client_id):
        return lib().xlating_sinks_detach(self.h, client_id)

    def stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        lib().xlating_sinks_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            lib().xlating_sinks_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- include/xlating_wire.h (client wire format + admission rules; host-only)
def wire_build_request(center_freq, sampling_rate, band_freq, destination):
    req = WireRequest(center_freq & 0xFFFFFFFF, sampling_rate, band_freq, destination)
    buf = C.create_string_buffer(15)
    n = lib().xlating_wire_build_request(C.byref(req), buf)
    return buf.raw[:n]


def wire_build_response(status, details):
    buf = C.create_string_buffer(7)
    n = lib().xlating_wire_build_response(status, details, buf)
    return buf.raw[:n]


def wire_build_header(mtype):
    buf = C.create_string_buffer(2)
    n = lib().xlating_wire_build_header(mtype, buf)
    return buf.raw[:n]


def wire_parse_header(data):
    t = C.c_uint8(0)
    return lib().xlating_wire_parse_header(bytes(data), len(data), C.byref(t)), t.value


def wire_parse_request(data):
    req = WireRequest()
    code = lib().xlating_wire_parse_request(bytes(data), len(data), C.byref(req))
    return code, req


def wire_parse_response(data):
    st, det = C.c_uint8(0), C.c_uint32(0)
    code = lib().xlating_wire_parse_response(bytes(data), len(data), C.byref(st), C.byref(det))
    return code, st.value, det.value


def wire_admit(req, band_sampling_rate, current_band_freq=0, lpf_cutoff_rate=5):
    """-> (code, WireAdmission, failure_details)"""
    adm, why = WireAdmission(), C.c_uint32(0)
    code = lib().xlating_wire_admit(C.byref(req), band_sampling_rate, current_band_freq, lpf_cutoff_rate, C.byref(adm), C.byref(why))
    return code, adm, why.value


def wire_add_client(engine, adm, band_sampling_rate):
    return lib().xlating_wire_add_client(engine.h, C.byref(adm), band_sampling_rate)


def wire_admit_any_rate(req, band_sampling_rate, current_band_freq=0, lpf_cutoff_rate=5):
    """-> (code, WireAdmission, WireResample, failure_details); L == M == 1: the rate divides the band rate, no second stage"""
    adm, rs, why = WireAdmission(), WireResample(), C.c_uint32(0)
    code = lib().xlating_wire_admit_any_rate(C.byref(req), band_sampling_rate, current_band_freq, lpf_cutoff_rate, C.byref(adm),
                                             C.byref(rs), C.byref(why))
    return code, adm, rs, why.value


def wire_resample_taps(req, rs, lpf_cutoff_rate=5):
    """-> (code, float32 taps | None): the second stage's prototype of an admitted request"""
    p = _c_float_p()
    n = C.c_size_t(0)
    code = lib().xlating_wire_resample_taps(C.byref(req), C.byref(rs), lpf_cutoff_rate, C.byref(p), C.byref(n))
    if code != 0:
        return code, None
    taps = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    _libc.free(p)
    return 0, taps


# ------------------------------------------------------------------------------------------------- spectrogram (libxlating_spectrum.so)
SPECTRUM_SYMBOLS = ["xlating_spectrum_create", "xlating_spectrum_feed_host", "xlating_spectrum_feed_device", "xlating_spectrum_take_rows",
                    "xlating_spectrum_destroy", "spectrogram_main", "spectrogram_sighandler",
                    "xlating_spectrum_create_wide", "spectrogram_main_wide",
                    "xlating_spectrum_bank_create", "xlating_spectrum_bank_add", "xlating_spectrum_bank_remove",
                    "xlating_spectrum_bank_feed_device", "xlating_spectrum_bank_take_rows", "xlating_spectrum_bank_rows_pending",
                    "xlating_spectrum_bank_last_feed_ops", "xlating_spectrum_bank_destroy", "xlating_spectrum_bank_create_wide"]
SPECTRUM_FMT = {"cu8": 0, "cs16": 2, "cf32": 3}
_SPEC_NP = {"cu8": np.uint8, "cs16": np.int16, "cf32": np.float32}
_slib = None


def spectrum_library_path():
    return os.path.join(os.path.dirname(library_path()), "libxlating_spectrum.so")


def spectrum_lib():
    """include/xlating_spectrum.h and include/spectrogram.h: the GPU spectrogram."""
    global _slib
    if _slib is not None:
        return _slib
    lib()  # (torch's HIP runtime first, see lib())
    path = spectrum_library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    S = C.CDLL(path)
    S.xlating_spectrum_create.argtypes = [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    S.xlating_spectrum_create.restype = C.c_int
    S.xlating_spectrum_create_wide.argtypes = [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    S.xlating_spectrum_create_wide.restype = C.c_int
    S.xlating_spectrum_feed_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    S.xlating_spectrum_feed_host.restype = C.c_int
    S.xlating_spectrum_feed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    S.xlating_spectrum_feed_device.restype = C.c_int
    S.xlating_spectrum_take_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    S.xlating_spectrum_take_rows.restype = C.c_int
    S.xlating_spectrum_destroy.argtypes = [C.c_void_p]
    S.xlating_spectrum_destroy.restype = None
    S.spectrogram_main.argtypes = [C.c_void_p]
    S.spectrogram_main.restype = C.c_int
    S.spectrogram_main_wide.argtypes = [C.c_void_p]
    S.spectrogram_main_wide.restype = C.c_int
    S.xlating_spectrum_bank_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    S.xlating_spectrum_bank_create.restype = C.c_int
    S.xlating_spectrum_bank_create_wide.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    S.xlating_spectrum_bank_create_wide.restype = C.c_int
    S.xlating_spectrum_bank_add.argtypes = [C.c_void_p, C.c_uint32]
    S.xlating_spectrum_bank_add.restype = C.c_int
    S.xlating_spectrum_bank_remove.argtypes = [C.c_void_p, C.c_int]
    S.xlating_spectrum_bank_remove.restype = C.c_int
    S.xlating_spectrum_bank_feed_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    S.xlating_spectrum_bank_feed_device.restype = C.c_int
    S.xlating_spectrum_bank_take_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    S.xlating_spectrum_bank_take_rows.restype = C.c_int
    S.xlating_spectrum_bank_rows_pending.argtypes = [C.c_void_p, C.c_int]
    S.xlating_spectrum_bank_rows_pending.restype = C.c_int
    S.xlating_spectrum_bank_last_feed_ops.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    S.xlating_spectrum_bank_last_feed_ops.restype = C.c_int
    S.xlating_spectrum_bank_destroy.argtypes = [C.c_void_p]
    S.xlating_spectrum_bank_destroy.restype = None
    _slib = S
    return S


class Spectrum:
    """One `xlating_spectrum *` (include/xlating_spectrum.h): feed samples in pieces, take completed waterfall rows.
    wide=True creates it with xlating_spectrum_create_wide: widths up to 1048576 instead of 8192."""

    def __init__(self, sampling_rate, width, fmt="cu8", wide=False):
        S = spectrum_lib()
        name = "xlating_spectrum_create_wide" if wide else "xlating_spectrum_create"
        if fmt not in SPECTRUM_FMT:
            raise XlatingError(name, -22)
        h = C.c_void_p()
        code = getattr(S, name)(sampling_rate, width, SPECTRUM_FMT[fmt], C.byref(h))
        if code != 0:
            raise XlatingError(name, code)
        self.h, self.W, self.fmt = h, width, fmt

    def feed(self, x, n=None, stream=0):
        """x: a numpy array of scalar elements (I, Q interleaved; cu8 uint8, cs16 int16, cf32 float32), or a device pointer (int)
        with n = its number of complex samples, read in place on `stream`."""
        if isinstance(x, int):
            code = spectrum_lib().xlating_spectrum_feed_device(self.h, x, n, stream)
        else:
            x = np.ascontiguousarray(x, dtype=_SPEC_NP[self.fmt])
            code = spectrum_lib().xlating_spectrum_feed_host(self.h, x.ctypes.data, x.size // 2)
        if code != 0:
            raise XlatingError("xlating_spectrum_feed", code)

    def take_rows(self, max_rows=1 << 20):
        """-> (db float32 [R, W], pixels uint8 [R, W]): every completed row not taken yet, oldest first."""
        S, parts_db, parts_px = spectrum_lib(), [], []
        while True:
            n = max(4, min(256, (1 << 26) // self.W))  # (256 rows a round up to width 262144; fewer of a wider row)
            db = np.empty((n, self.W), np.float32)
            px = np.empty((n, self.W), np.uint8)
            got = S.xlating_spectrum_take_rows(self.h, db.ctypes.data, px.ctypes.data, min(n, max_rows))
            if got < 0:
                raise XlatingError("xlating_spectrum_take_rows", got)
            parts_db.append(db[:got])
            parts_px.append(px[:got])
            max_rows -= got
            if got < n or max_rows <= 0:
                break
        return np.concatenate(parts_db), np.concatenate(parts_px)

    def close(self):
        if getattr(self, "h", None):
            spectrum_lib().xlating_spectrum_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpectrumBank:
    """One `xlating_spectrum_bank *` (include/xlating_spectrum.h): many streams of one width and format, each with its own
    sampling_rate, advanced together by one feed of device buffers; rows are taken per stream.
    wide=True creates it with xlating_spectrum_bank_create_wide: widths up to 1048576 instead of 8192."""

    def __init__(self, width, fmt="cf32", wide=False):
        S = spectrum_lib()
        name = "xlating_spectrum_bank_create_wide" if wide else "xlating_spectrum_bank_create"
        if fmt not in SPECTRUM_FMT:
            raise XlatingError(name, -22)
        h = C.c_void_p()
        code = getattr(S, name)(width, SPECTRUM_FMT[fmt], C.byref(h))
        if code != 0:
            raise XlatingError(name, code)
        self.h, self.W, self.fmt = h, width, fmt

    def add(self, sampling_rate):
        sid = spectrum_lib().xlating_spectrum_bank_add(self.h, sampling_rate)
        if sid < 0:
            raise XlatingError("xlating_spectrum_bank_add", sid)
        return sid

    def remove(self, stream_id):
        code = spectrum_lib().xlating_spectrum_bank_remove(self.h, stream_id)
        if code != 0:
            raise XlatingError("xlating_spectrum_bank_remove", code)

    def feed(self, ids, ptrs, counts, stream=0):
        """stream ids[i] consumes counts[i] complex samples from device address ptrs[i], in place, ordered on `stream`."""
        a = np.ascontiguousarray(ids, dtype=np.intc)
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        assert a.size == p.size == c.size
        code = spectrum_lib().xlating_spectrum_bank_feed_device(self.h, a.size, a.ctypes.data, p.ctypes.data, c.ctypes.data, stream)
        if code != 0:
            raise XlatingError("xlating_spectrum_bank_feed_device", code)

    def feed_engine(self, engine, streams, stream=0):
        """streams: {client id of `engine`: stream id}.  Feeds every listed client's output of the engine's latest call
        (xlating_batch_output_device: a host-side lookup) in one call.  The caller orders `stream` behind the engine's call (the
        same stream, or BatchEngine.record_event and a wait when the call ran on stream="engine") and feeds before the next call,
        which reuses the rows."""
        self.feed(*self.gather_engine(engine, streams), stream)

    @staticmethod
    def gather_engine(engine, streams):
        """-> (stream ids, device pointers, counts) of the listed clients' outputs of the engine's latest call"""
        ptrs, counts = engine.outputs_device(list(streams.keys()))  # (one call: xlating_batch_outputs_device)
        return list(streams.values()), ptrs, counts

    def take_rows(self, stream_id, max_rows=1 << 20):
        """-> (db float32 [R, W], pixels uint8 [R, W]): the stream's completed rows not taken yet, oldest first."""
        S = spectrum_lib()
        n = self.rows_pending(stream_id)
        n = min(max(n, 0), max_rows)
        db = np.empty((n, self.W), np.float32)
        px = np.empty((n, self.W), np.uint8)
        got = S.xlating_spectrum_bank_take_rows(self.h, stream_id, db.ctypes.data, px.ctypes.data, n) if n else 0
        if got < 0:
            raise XlatingError("xlating_spectrum_bank_take_rows", got)
        return db[:got], px[:got]

    def rows_pending(self, stream_id):
        n = spectrum_lib().xlating_spectrum_bank_rows_pending(self.h, stream_id)
        if n < 0:
            raise XlatingError("xlating_spectrum_bank_rows_pending", n)
        return n

    def last_feed_ops(self):
        """-> (kernel launches, memory copies) the latest feed issued"""
        a, b = C.c_uint(0), C.c_uint(0)
        spectrum_lib().xlating_spectrum_bank_last_feed_ops(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            spectrum_lib().xlating_spectrum_bank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpectrogramRequest(C.Structure):
    """include/spectrogram.h `spectrogram` (the reference's six request fields, then reserved space)"""
    _fields_ = [("sampling_rate", C.c_uint32), ("width", C.c_int), ("data_format", C.c_char_p), ("input_file", C.c_char_p),
                ("output_file", C.c_char_p), ("fftw_flags", C.c_char_p), ("xl_private", C.c_void_p * 6)]


def spectrogram_main(input_file, output_file, width=1024, sampling_rate=48000, data_format="cu8", fftw_flags="FFTW_MEASURE", wide=False):
    """spectrogram_main() of include/spectrogram.h (wide=True: spectrogram_main_wide()) -> its return code.  None leaves a pointer
    field NULL."""
    enc = lambda v: None if v is None else str(v).encode()  # noqa: E731
    req = SpectrogramRequest(sampling_rate, width, enc(data_format), enc(input_file), enc(output_file), enc(fftw_flags))
    S = spectrum_lib()
    return (S.spectrogram_main_wide if wide else S.spectrogram_main)(C.byref(req))


# ------------------------------------------------------------------------------------------------- resampler bank (libxlating_resample.so)
RESAMPLE_SYMBOLS = ["xlating_resample_bank_create", "xlating_resample_bank_add", "xlating_resample_bank_remove",
                    "xlating_resample_bank_feed_device", "xlating_resample_bank_output_device", "xlating_resample_bank_fetch",
                    "xlating_resample_bank_output_host", "xlating_resample_bank_produced", "xlating_resample_bank_last_feed_ops",
                    "xlating_resample_bank_stats", "xlating_resample_bank_destroy"]
_rlib = None


def resample_library_path():
    return os.path.join(os.path.dirname(library_path()), "libxlating_resample.so")


def resample_lib():
    """include/xlating_resample.h: the rational resampler bank behind the engine."""
    global _rlib
    if _rlib is not None:
        return _rlib
    lib()  # (torch's HIP runtime first, see lib())
    path = resample_library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    R = C.CDLL(path)
    R.xlating_resample_bank_create.argtypes = [C.POINTER(C.c_void_p)]
    R.xlating_resample_bank_create.restype = C.c_int
    R.xlating_resample_bank_add.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
    R.xlating_resample_bank_add.restype = C.c_int
    R.xlating_resample_bank_remove.argtypes = [C.c_void_p, C.c_int]
    R.xlating_resample_bank_remove.restype = C.c_int
    R.xlating_resample_bank_feed_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    R.xlating_resample_bank_feed_device.restype = C.c_int
    R.xlating_resample_bank_output_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    R.xlating_resample_bank_output_device.restype = C.c_int
    R.xlating_resample_bank_fetch.argtypes = [C.c_void_p]
    R.xlating_resample_bank_fetch.restype = C.c_int
    R.xlating_resample_bank_output_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(_c_float_p), C.POINTER(C.c_size_t)]
    R.xlating_resample_bank_output_host.restype = C.c_int
    R.xlating_resample_bank_produced.argtypes = [C.c_void_p, C.c_int]
    R.xlating_resample_bank_produced.restype = C.c_uint64
    R.xlating_resample_bank_last_feed_ops.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    R.xlating_resample_bank_last_feed_ops.restype = C.c_int
    R.xlating_resample_bank_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_size_t)]
    R.xlating_resample_bank_stats.restype = C.c_int
    R.xlating_resample_bank_destroy.argtypes = [C.c_void_p]
    R.xlating_resample_bank_destroy.restype = None
    _rlib = R
    return R


class ResamplerBank:
    """One `xlating_resample_bank *` (include/xlating_resample.h): many complex float32 streams, each resampled by its own L / M
    with its own prototype, advanced together by one feed of device buffers; the latest feed's outputs are read per stream."""

    _prefix = "xlating_resample_bank_"  # (ResamplerBankQ15: the other header's functions, the same signatures)
    _lib = staticmethod(resample_lib)

    def _call(self, name, *args):
        return getattr(self._lib(), self._prefix + name)(self.h, *args)

    def __init__(self):
        h = C.c_void_p()
        code = getattr(self._lib(), self._prefix + "create")(C.byref(h))
        if code != 0:
            raise XlatingError(self._prefix + "create", code)
        self.h = h

    def add(self, L, M, taps):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        sid = self._call("add", L, M, t.ctypes.data, t.size)
        if sid < 0:
            raise XlatingError(self._prefix + "add", sid)
        return sid

    def remove(self, stream_id):
        code = self._call("remove", stream_id)
        if code != 0:
            raise XlatingError(self._prefix + "remove", code)

    def feed(self, ids, ptrs, counts, stream=0):
        """stream ids[i] consumes counts[i] complex samples from device address ptrs[i], in place, ordered on `stream`."""
        a = np.ascontiguousarray(ids, dtype=np.intc)
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        assert a.size == p.size == c.size
        code = self._call("feed_device", a.size, a.ctypes.data, p.ctypes.data, c.ctypes.data, stream)
        if code != 0:
            raise XlatingError(self._prefix + "feed_device", code)

    def feed_engine(self, engine, streams, stream=0):
        """streams: {client id of `engine`: stream id}.  Feeds every listed client's output of the engine's latest call in one call;
        ordering and lifetime as SpectrumBank.feed_engine."""
        self.feed(*SpectrumBank.gather_engine(engine, streams), stream)

    def fetch(self):
        code = self._call("fetch")
        if code != 0:
            raise XlatingError(self._prefix + "fetch", code)

    def output(self, stream_id):
        """-> complex64 [n]: the stream's outputs of the latest feed as of the latest fetch (a copy)"""
        p, n = _c_float_p(), C.c_size_t(0)
        code = self._call("output_host", stream_id, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError(self._prefix + "output_host", code)
        if n.value == 0:
            return np.zeros(0, np.complex64)
        return np.ctypeslib.as_array(p, shape=(2 * n.value,)).copy().view(np.complex64)

    def output_device(self, stream_id):
        """-> (device pointer | None, complex samples) of the stream's outputs of the latest feed; valid until the next feed"""
        p, n = C.c_void_p(), C.c_size_t(0)
        code = self._call("output_device", stream_id, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError(self._prefix + "output_device", code)
        return p.value, n.value

    def produced(self, stream_id):
        return self._call("produced", stream_id)

    def last_feed_ops(self):
        """-> (kernel launches, memory copies) the latest feed issued"""
        a, b = C.c_uint(0), C.c_uint(0)
        self._call("last_feed_ops", C.byref(a), C.byref(b))
        return a.value, b.value

    def stats(self):
        """-> (live streams, device tap tables, their bytes)"""
        a, b, c = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
        self._call("stats", C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def close(self):
        if getattr(self, "h", None):
            self._call("destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------- Q15 resampler bank (the same library)
RESAMPLE_Q15_SYMBOLS = ["xlating_resample_q15_quantize"] + [s.replace("xlating_resample_bank_", "xlating_resample_q15_bank_")
                                                            for s in RESAMPLE_SYMBOLS]
_rqlib = None


def resample_q15_lib():
    """include/xlating_resample_q15.h: the resampler bank of the cs16 output family (libxlating_resample.so, bound once)."""
    global _rqlib
    if _rqlib is not None:
        return _rqlib
    R = resample_lib()
    R.xlating_resample_q15_quantize.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    R.xlating_resample_q15_quantize.restype = C.c_int
    for name in RESAMPLE_SYMBOLS:  # the float bank's signatures, one for one; output_host gives int16
        f, q = getattr(R, name), getattr(R, name.replace("xlating_resample_bank_", "xlating_resample_q15_bank_"))
        q.argtypes, q.restype = list(f.argtypes), f.restype
    R.xlating_resample_q15_bank_output_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(_c_i16_p), C.POINTER(C.c_size_t)]
    _rqlib = R
    return R


def resample_q15_quantize(taps):
    """xlating_resample_q15_quantize: float32 taps -> int16 array, c = trunc(h * 32768); XlatingError(-ERANGE) for a tap that is
    not finite or does not fit, XlatingError(-EINVAL) for no taps"""
    t = np.ascontiguousarray(taps, dtype=np.float32)
    out = np.zeros(t.size, np.int16)
    code = resample_q15_lib().xlating_resample_q15_quantize(t.ctypes.data if t.size else None, t.size, out.ctypes.data if t.size else None)
    if code != 0:
        raise XlatingError("xlating_resample_q15_quantize", code)
    return out


class ResamplerBankQ15(ResamplerBank):
    """One `xlating_resample_q15_bank *` (include/xlating_resample_q15.h): many streams of int16 (re, im) pairs -- the engine's rows
    after a "q15" call -- each resampled by its own L / M in exact Q15 arithmetic.  ResamplerBank's methods; counts are complex samples
    of 4 bytes, output() is int16 [n, 2]."""
    _prefix = "xlating_resample_q15_bank_"
    _lib = staticmethod(resample_q15_lib)

    def output(self, stream_id):
        """-> int16 [n, 2]: the stream's outputs of the latest feed as of the latest fetch (a copy)"""
        p, n = _c_i16_p(), C.c_size_t(0)
        code = self._call("output_host", stream_id, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError(self._prefix + "output_host", code)
        if n.value == 0:
            return np.zeros((0, 2), np.int16)
        return np.ctypeslib.as_array(p, shape=(n.value, 2)).copy()


# ------------------------------------------------------------------------------------------------- delivery and serve (libxlating_serve.so)
DELIVERY_SYMBOLS = ["xlating_delivery_create", "xlating_delivery_pack_device", "xlating_delivery_pack_device_cs16", "xlating_delivery_query",
                    "xlating_delivery_wait", "xlating_delivery_row", "xlating_delivery_release", "xlating_delivery_last_ops",
                    "xlating_delivery_chunk_bytes", "xlating_delivery_destroy", "xlating_delivery_pack_device_cs16_gain",
                    "xlating_delivery_row_level"]
# ------------------------------------------------------------------------------------------------- tuner bank (libxlating_tune.so)
TUNE_SYMBOLS = ["xlating_tune_bank_create", "xlating_tune_bank_add", "xlating_tune_bank_remove", "xlating_tune_bank_set",
                "xlating_tune_bank_feed_device", "xlating_tune_bank_output_device", "xlating_tune_bank_state",
                "xlating_tune_bank_last_feed_ops", "xlating_tune_bank_destroy", "xlating_tune_cs", "xlating_tune_from_hz",
                "xlating_tune_chunk_samples"]
_tlib = None


def tune_library_path():
    return os.path.join(os.path.dirname(library_path()), "libxlating_tune.so")


def tune_lib():
    """include/xlating_tune.h: the phase-continuous rotator bank behind the engine."""
    global _tlib
    if _tlib is not None:
        return _tlib
    lib()  # (torch's HIP runtime first, see lib())
    path = tune_library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    T = C.CDLL(path)
    T.xlating_tune_bank_create.argtypes = [C.POINTER(C.c_void_p)]
    T.xlating_tune_bank_create.restype = C.c_int
    T.xlating_tune_bank_add.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64]
    T.xlating_tune_bank_add.restype = C.c_int
    T.xlating_tune_bank_remove.argtypes = [C.c_void_p, C.c_int]
    T.xlating_tune_bank_remove.restype = C.c_int
    T.xlating_tune_bank_set.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64]
    T.xlating_tune_bank_set.restype = C.c_int
    T.xlating_tune_bank_feed_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    T.xlating_tune_bank_feed_device.restype = C.c_int
    T.xlating_tune_bank_output_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    T.xlating_tune_bank_output_device.restype = C.c_int
    T.xlating_tune_bank_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_uint64)]
    T.xlating_tune_bank_state.restype = C.c_int
    T.xlating_tune_bank_last_feed_ops.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    T.xlating_tune_bank_last_feed_ops.restype = C.c_int
    T.xlating_tune_bank_destroy.argtypes = [C.c_void_p]
    T.xlating_tune_bank_destroy.restype = None
    T.xlating_tune_cs.argtypes = [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    T.xlating_tune_cs.restype = None
    T.xlating_tune_from_hz.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    T.xlating_tune_from_hz.restype = C.c_int
    T.xlating_tune_chunk_samples.argtypes = []
    T.xlating_tune_chunk_samples.restype = C.c_uint
    _tlib = T
    return T


def tune_cs(p):
    """-> (cos, sin) of 2 pi p / 2^32 as float32, by the tuner bank's rule (csrc/xl_tune_rule.h); p: 0 .. 2^32 - 1"""
    c, s = C.c_float(0), C.c_float(0)
    tune_lib().xlating_tune_cs(int(p) & 0xFFFFFFFF, C.byref(c), C.byref(s))
    return np.float32(c.value), np.float32(s.value)


def tune_from_hz(shift_hz, ramp_hz_per_s, rate):
    """-> (F, R): the steps of a shift in Hz and a ramp in Hz per second at a sample rate (XlatingError -EINVAL: a quotient that is
    not finite or not below 0.5 in magnitude)"""
    F, R = C.c_int64(0), C.c_int64(0)
    code = tune_lib().xlating_tune_from_hz(float(shift_hz), float(ramp_hz_per_s), float(rate), C.byref(F), C.byref(R))
    if code != 0:
        raise XlatingError("xlating_tune_from_hz", code)
    return F.value, R.value


def tune_chunk_samples():
    return tune_lib().xlating_tune_chunk_samples()


class TuneBank:
    """One `xlating_tune_bank *` (include/xlating_tune.h): many complex float32 streams, each rotated by its own phase-continuous
    shift (P, F, R), advanced together by one feed of device buffers; the latest feed's rows are read per stream on the device."""

    def __init__(self):
        h = C.c_void_p()
        code = tune_lib().xlating_tune_bank_create(C.byref(h))
        if code != 0:
            raise XlatingError("xlating_tune_bank_create", code)
        self.h = h

    def add(self, P=0, F=0, R=0):
        sid = tune_lib().xlating_tune_bank_add(self.h, int(P) & 0xFFFFFFFFFFFFFFFF, int(F), int(R))
        if sid < 0:
            raise XlatingError("xlating_tune_bank_add", sid)
        return sid

    def remove(self, stream_id):
        code = tune_lib().xlating_tune_bank_remove(self.h, stream_id)
        if code != 0:
            raise XlatingError("xlating_tune_bank_remove", code)

    def set(self, stream_id, F, R=0):
        """new steps from the next sample fed on; the phase is untouched"""
        code = tune_lib().xlating_tune_bank_set(self.h, stream_id, int(F), int(R))
        if code != 0:
            raise XlatingError("xlating_tune_bank_set", code)

    def feed(self, ids, ptrs, counts, stream=0):
        """stream ids[i] rotates counts[i] complex samples at device address ptrs[i], read in place, ordered on `stream`."""
        a = np.ascontiguousarray(ids, dtype=np.intc)
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        assert a.size == p.size == c.size
        code = tune_lib().xlating_tune_bank_feed_device(self.h, a.size, a.ctypes.data, p.ctypes.data, c.ctypes.data, stream)
        if code != 0:
            raise XlatingError("xlating_tune_bank_feed_device", code)

    def output_device(self, stream_id):
        """-> (device pointer | None, complex samples) of the stream's row of the latest feed; valid until the next feed"""
        p, n = C.c_void_p(), C.c_size_t(0)
        code = tune_lib().xlating_tune_bank_output_device(self.h, stream_id, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError("xlating_tune_bank_output_device", code)
        return p.value, n.value

    def state(self, stream_id):
        """-> (P, F, R, consumed) as the next sample fed will see them: Python integers, host state, no waiting"""
        P, F, R, n = C.c_uint64(0), C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        code = tune_lib().xlating_tune_bank_state(self.h, stream_id, C.byref(P), C.byref(F), C.byref(R), C.byref(n))
        if code != 0:
            raise XlatingError("xlating_tune_bank_state", code)
        return P.value, F.value, R.value, n.value

    def last_feed_ops(self):
        """-> (kernel launches, memory copies) the latest feed issued"""
        a, b = C.c_uint(0), C.c_uint(0)
        tune_lib().xlating_tune_bank_last_feed_ops(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            tune_lib().xlating_tune_bank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------- power meter (libxlating_meter.so)
METER_SYMBOLS = ["xlating_meter_create", "xlating_meter_measure_device", "xlating_meter_query", "xlating_meter_wait",
                 "xlating_meter_power", "xlating_meter_partials", "xlating_meter_last_ops", "xlating_meter_piece_samples",
                 "xlating_meter_destroy"]
METER_FMT = {"cf32": 0, "cs16": 1}
_meterlib = None


def meter_library_path():
    return os.path.join(os.path.dirname(library_path()), "libxlating_meter.so")


def meter_lib():
    """include/xlating_meter.h: the mean power of many device rows in one launch."""
    global _meterlib
    if _meterlib is not None:
        return _meterlib
    lib()  # (torch's HIP runtime first, see lib())
    path = meter_library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    M = C.CDLL(path)
    M.xlating_meter_create.argtypes = [C.POINTER(C.c_void_p)]
    M.xlating_meter_create.restype = C.c_int
    M.xlating_meter_measure_device.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    M.xlating_meter_measure_device.restype = C.c_int
    for name in ("xlating_meter_query", "xlating_meter_wait"):
        getattr(M, name).argtypes = [C.c_void_p]
        getattr(M, name).restype = C.c_int
    M.xlating_meter_power.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    M.xlating_meter_power.restype = C.c_int
    M.xlating_meter_partials.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    M.xlating_meter_partials.restype = C.c_int
    M.xlating_meter_last_ops.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    M.xlating_meter_last_ops.restype = C.c_int
    M.xlating_meter_piece_samples.argtypes = []
    M.xlating_meter_piece_samples.restype = C.c_uint
    M.xlating_meter_destroy.argtypes = [C.c_void_p]
    M.xlating_meter_destroy.restype = None
    _meterlib = M
    return M


def meter_piece_samples():
    return meter_lib().xlating_meter_piece_samples()


class Meter:
    """One `xlating_meter *` (include/xlating_meter.h): the mean power of many device rows of one format by one launch, one table copy
    and one copy back; one measurement outstanding at a time."""

    def __init__(self):
        h = C.c_void_p()
        code = meter_lib().xlating_meter_create(C.byref(h))
        if code != 0:
            raise XlatingError("xlating_meter_create", code)
        self.h = h

    def measure(self, fmt, ptrs, counts, stream=0):
        """row i: counts[i] samples of `fmt` ("cf32" | "cs16") at device address ptrs[i], read in place, ordered on `stream`"""
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        assert p.size == c.size
        code = meter_lib().xlating_meter_measure_device(self.h, METER_FMT[fmt], p.size, p.ctypes.data, c.ctypes.data, stream)
        if code != 0:
            raise XlatingError("xlating_meter_measure_device", code)

    def query(self):
        code = meter_lib().xlating_meter_query(self.h)
        if code < 0:
            raise XlatingError("xlating_meter_query", code)
        return bool(code)

    def wait(self):
        code = meter_lib().xlating_meter_wait(self.h)
        if code != 0:
            raise XlatingError("xlating_meter_wait", code)

    def power(self, i):
        """-> (mean power as a Python float, samples) of row i of the latest measurement, which is done"""
        p, n = C.c_double(0), C.c_uint64(0)
        code = meter_lib().xlating_meter_power(self.h, i, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError("xlating_meter_power", code)
        return p.value, n.value

    def partials(self, i):
        """-> uint64 [pieces]: row i's partials as the kernel left them (cf32: the float32's bits in the low half)"""
        n = meter_lib().xlating_meter_partials(self.h, i, 0, None)
        if n < 0:
            raise XlatingError("xlating_meter_partials", n)
        out = np.zeros(n, np.uint64)
        if n > 0:
            n = meter_lib().xlating_meter_partials(self.h, i, n, out.ctypes.data)
            if n < 0:
                raise XlatingError("xlating_meter_partials", n)
        return out

    def last_ops(self):
        """-> (kernel launches, memory copies) the latest measurement issued"""
        a, b = C.c_uint(0), C.c_uint(0)
        meter_lib().xlating_meter_last_ops(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            meter_lib().xlating_meter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SERVE_SYMBOLS = ["xlating_serve_create", "xlating_serve_request", "xlating_serve_remove", "xlating_serve_blocks_host",
                 "xlating_serve_blocks_device", "xlating_serve_flush", "xlating_serve_outputs_device", "xlating_serve_dropped",
                 "xlating_serve_engine", "xlating_serve_last_ops", "xlating_serve_sink_stats", "xlating_serve_destroy",
                 "xlating_serve_set_gain", "xlating_serve_set_auto_gain", "xlating_serve_enable_levels", "xlating_serve_levels",
                 "xlating_serve_gain_log", "xlating_serve_set_tune", "xlating_serve_tune_log", "xlating_serve_set_squelch",
                 "xlating_serve_clear_squelch", "xlating_serve_squelch_state", "xlating_serve_squelch_log"]
SERVE_FAMILY = {"cf32": 0, "cs16": 1, "cf32-cs16": 2}  # (2: the cf32 family, narrowed to cs16 by the delivery)
_vlib = None


class ServeConfig(C.Structure):
    """include/xlating_serve.h xlating_serve_config"""
    _fields_ = [("band_sampling_rate", C.c_uint32), ("input_format", C.c_int), ("buffer_size", C.c_uint32), ("group_blocks", C.c_uint),
                ("device", C.c_int), ("family", C.c_int), ("native", C.c_int), ("any_rate", C.c_int), ("lpf_cutoff_rate", C.c_uint32),
                ("base_path", C.c_char_p), ("use_gzip", C.c_int), ("writer_threads", C.c_uint), ("queue_bytes", C.c_size_t),
                ("delivery_slots", C.c_uint), ("overlap", C.c_int)]


def serve_library_path():
    return os.path.join(os.path.dirname(library_path()), "libxlating_serve.so")


def serve_lib():
    """include/xlating_delivery.h and include/xlating_serve.h: delivery of device rows, and the whole loop in one object."""
    global _vlib
    if _vlib is not None:
        return _vlib
    resample_lib()  # (torch's HIP runtime first, see lib(); the libraries this one links)
    tune_lib()
    meter_lib()
    path = serve_library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    V = C.CDLL(path)
    V.xlating_delivery_create.argtypes = [C.c_uint, C.POINTER(C.c_void_p)]
    V.xlating_delivery_create.restype = C.c_int
    V.xlating_delivery_pack_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    V.xlating_delivery_pack_device.restype = C.c_int
    V.xlating_delivery_pack_device_cs16.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    V.xlating_delivery_pack_device_cs16.restype = C.c_int
    V.xlating_delivery_pack_device_cs16_gain.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    V.xlating_delivery_pack_device_cs16_gain.restype = C.c_int
    V.xlating_delivery_row_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    V.xlating_delivery_row_level.restype = C.c_int
    for name in ("xlating_delivery_query", "xlating_delivery_wait", "xlating_delivery_release"):
        getattr(V, name).argtypes = [C.c_void_p, C.c_int]
        getattr(V, name).restype = C.c_int
    V.xlating_delivery_row.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    V.xlating_delivery_row.restype = C.c_int
    V.xlating_delivery_last_ops.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
    V.xlating_delivery_last_ops.restype = C.c_int
    V.xlating_delivery_chunk_bytes.argtypes = []
    V.xlating_delivery_chunk_bytes.restype = C.c_uint
    V.xlating_delivery_destroy.argtypes = [C.c_void_p]
    V.xlating_delivery_destroy.restype = None
    V.xlating_serve_create.argtypes = [C.POINTER(ServeConfig), C.POINTER(C.c_void_p)]
    V.xlating_serve_create.restype = C.c_int
    V.xlating_serve_request.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    V.xlating_serve_request.restype = C.c_int
    V.xlating_serve_remove.argtypes = [C.c_void_p, C.c_int]
    V.xlating_serve_remove.restype = C.c_int
    V.xlating_serve_blocks_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint]
    V.xlating_serve_blocks_host.restype = C.c_int
    V.xlating_serve_blocks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p]
    V.xlating_serve_blocks_device.restype = C.c_int
    V.xlating_serve_flush.argtypes = [C.c_void_p]
    V.xlating_serve_flush.restype = C.c_int
    V.xlating_serve_outputs_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    V.xlating_serve_outputs_device.restype = C.c_int
    V.xlating_serve_dropped.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t]
    V.xlating_serve_dropped.restype = C.c_size_t
    V.xlating_serve_engine.argtypes = [C.c_void_p]
    V.xlating_serve_engine.restype = C.c_void_p
    V.xlating_serve_last_ops.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
    V.xlating_serve_last_ops.restype = C.c_int
    V.xlating_serve_sink_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    V.xlating_serve_sink_stats.restype = C.c_int
    for name in ("xlating_serve_set_gain", "xlating_serve_set_auto_gain"):
        getattr(V, name).argtypes = [C.c_void_p, C.c_int, C.c_int]
        getattr(V, name).restype = C.c_int
    V.xlating_serve_enable_levels.argtypes = [C.c_void_p, C.c_int]
    V.xlating_serve_enable_levels.restype = C.c_int
    V.xlating_serve_levels.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 6
    V.xlating_serve_levels.restype = C.c_int
    V.xlating_serve_gain_log.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    V.xlating_serve_gain_log.restype = C.c_int
    V.xlating_serve_set_tune.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
    V.xlating_serve_set_tune.restype = C.c_int
    V.xlating_serve_tune_log.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    V.xlating_serve_tune_log.restype = C.c_int
    V.xlating_serve_set_squelch.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_uint]
    V.xlating_serve_set_squelch.restype = C.c_int
    V.xlating_serve_clear_squelch.argtypes = [C.c_void_p, C.c_int]
    V.xlating_serve_clear_squelch.restype = C.c_int
    V.xlating_serve_squelch_state.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    V.xlating_serve_squelch_state.restype = C.c_int
    V.xlating_serve_squelch_log.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    V.xlating_serve_squelch_log.restype = C.c_int
    V.xlating_serve_destroy.argtypes = [C.c_void_p]
    V.xlating_serve_destroy.restype = None
    _vlib = V
    return V


def delivery_chunk_bytes():
    return serve_lib().xlating_delivery_chunk_bytes()


class Delivery:
    """One `xlating_delivery *` (include/xlating_delivery.h): batches of device rows packed by one launch and moved to pinned host
    memory by one copy each; tickets are waited for, read per key and released."""

    def __init__(self, slots=2):
        h = C.c_void_p()
        code = serve_lib().xlating_delivery_create(slots, C.byref(h))
        if code != 0:
            raise XlatingError("xlating_delivery_create", code)
        self.h = h

    def pack(self, keys, ptrs, nbytes, stream=0):
        """row i: nbytes[i] bytes at device address ptrs[i], tagged keys[i] -> a ticket (XlatingError: -EAGAIN, -EINVAL, ...)"""
        k = np.ascontiguousarray(keys, dtype=np.intc)
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        b = np.ascontiguousarray(nbytes, dtype=np.uint64)
        assert k.size == p.size == b.size
        t = serve_lib().xlating_delivery_pack_device(self.h, k.size, k.ctypes.data, p.ctypes.data, b.ctypes.data, stream)
        if t < 0:
            raise XlatingError("xlating_delivery_pack_device", t)
        return t

    def pack_cs16(self, keys, ptrs, n_complex, stream=0):
        """row i: n_complex[i] cf32 samples at the 8-byte aligned device address ptrs[i], delivered as cs16 (round to nearest even of
        y * 32768, saturated; NaN -> 0) -> a ticket"""
        k = np.ascontiguousarray(keys, dtype=np.intc)
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        c = np.ascontiguousarray(n_complex, dtype=np.uint64)
        assert k.size == p.size == c.size
        t = serve_lib().xlating_delivery_pack_device_cs16(self.h, k.size, k.ctypes.data, p.ctypes.data, c.ctypes.data, stream)
        if t < 0:
            raise XlatingError("xlating_delivery_pack_device_cs16", t)
        return t

    def pack_device_cs16_gain(self, keys, ptrs, n_complex, gain_log2, stream=0):
        """pack_cs16 with a power-of-two gain per row, -48 .. 48 (y * 2^(15 + gain), rounded once, saturated; NaN -> 0), and every
        row's level recorded (row_level) -> a ticket"""
        k = np.ascontiguousarray(keys, dtype=np.intc)
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        c = np.ascontiguousarray(n_complex, dtype=np.uint64)
        g = np.ascontiguousarray(np.clip(np.asarray(gain_log2, dtype=np.int64), -128, 127), dtype=np.int8)  # (the library refuses)
        assert k.size == p.size == c.size == g.size
        t = serve_lib().xlating_delivery_pack_device_cs16_gain(self.h, k.size, k.ctypes.data, p.ctypes.data, c.ctypes.data, g.ctypes.data, stream)
        if t < 0:
            raise XlatingError("xlating_delivery_pack_device_cs16_gain", t)
        return t

    def row_level(self, ticket, key):
        """-> (peak_bits, clipped, nans) of the row tagged `key` of a pack_device_cs16_gain ticket that is done (XlatingError -ENODATA
        for a ticket of pack or pack_cs16)"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        code = serve_lib().xlating_delivery_row_level(self.h, ticket, key, C.byref(a), C.byref(b), C.byref(c))
        if code != 0:
            raise XlatingError("xlating_delivery_row_level", code)
        return a.value, b.value, c.value

    def query(self, ticket):
        code = serve_lib().xlating_delivery_query(self.h, ticket)
        if code < 0:
            raise XlatingError("xlating_delivery_query", code)
        return bool(code)

    def wait(self, ticket):
        code = serve_lib().xlating_delivery_wait(self.h, ticket)
        if code != 0:
            raise XlatingError("xlating_delivery_wait", code)

    def row(self, ticket, key):
        """-> uint8 [bytes]: a copy of the row tagged `key` (the ticket is done)"""
        p, n = C.c_void_p(), C.c_size_t(0)
        code = serve_lib().xlating_delivery_row(self.h, ticket, key, C.byref(p), C.byref(n))
        if code != 0:
            raise XlatingError("xlating_delivery_row", code)
        if n.value == 0:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()

    def release(self, ticket):
        code = serve_lib().xlating_delivery_release(self.h, ticket)
        if code != 0:
            raise XlatingError("xlating_delivery_release", code)

    def last_ops(self):
        """-> (kernel launches, memory copies, bytes of the device-to-host copy) of the latest pack"""
        a, b, c = C.c_uint(0), C.c_uint(0), C.c_uint64(0)
        serve_lib().xlating_delivery_last_ops(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def close(self):
        if getattr(self, "h", None):
            serve_lib().xlating_delivery_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Serve:
    """One `xlating_serve *` (include/xlating_serve.h): one band on one GPU, from wire requests to files and sockets."""

    def __init__(self, band_rate, in_fmt, buffer_size, base_path, family="cf32", native=False, any_rate=True, gzip=False, overlap=False,
                 group_blocks=1, lpf_cutoff_rate=5, writer_threads=2, queue_bytes=0, delivery_slots=2, device=-1):
        self._base = str(base_path).encode()
        cfg = ServeConfig(band_rate, FMT[in_fmt], buffer_size, group_blocks, device, SERVE_FAMILY[family], 1 if native else 0,
                          1 if any_rate else 0, lpf_cutoff_rate, self._base, 1 if gzip else 0, writer_threads, queue_bytes, delivery_slots,
                          1 if overlap else 0)
        h = C.c_void_p()
        code = serve_lib().xlating_serve_create(C.byref(cfg), C.byref(h))
        if code != 0:
            raise XlatingError("xlating_serve_create", code)
        self.h, self.in_fmt, self.family = h, in_fmt, family

    def request(self, msg, socket_fd=-1):
        """msg: header + request bytes -> (code, response bytes, client id | None); code 0 admitted, 1 refused"""
        resp, n, cid = C.create_string_buffer(7), C.c_size_t(0), C.c_int(-1)
        code = serve_lib().xlating_serve_request(self.h, bytes(msg), len(msg), socket_fd, resp, C.byref(n), C.byref(cid))
        if code < 0:
            raise XlatingError("xlating_serve_request", code)
        return code, resp.raw[:n.value], (cid.value if code == 0 else None)

    def remove(self, client_id):
        code = serve_lib().xlating_serve_remove(self.h, client_id)
        if code != 0:
            raise XlatingError("xlating_serve_remove", code)

    def blocks_host(self, x, nblocks=1):
        x = np.ascontiguousarray(x, dtype=_NP[self.in_fmt])
        assert x.size % nblocks == 0
        code = serve_lib().xlating_serve_blocks_host(self.h, x.ctypes.data, x.size // nblocks, nblocks)
        if code != 0:
            raise XlatingError("xlating_serve_blocks_host", code)

    def blocks_device(self, d_ptr, input_len, nblocks=1, stream=0):
        sp = C.c_void_p(-1) if stream == "engine" else (C.c_void_p(stream) if stream else None)
        code = serve_lib().xlating_serve_blocks_device(self.h, C.c_void_p(d_ptr), input_len, nblocks, sp)
        if code != 0:
            raise XlatingError("xlating_serve_blocks_device", code)

    def flush(self):
        code = serve_lib().xlating_serve_flush(self.h)
        if code != 0:
            raise XlatingError("xlating_serve_flush", code)

    def outputs_device(self, cids):
        """-> (device pointers uint64 [n], complex samples uint64 [n]) of the latest call's final rows"""
        a = np.ascontiguousarray(cids, dtype=np.intc)
        p, n = np.zeros(a.size, np.uint64), np.zeros(a.size, np.uint64)
        code = serve_lib().xlating_serve_outputs_device(self.h, a.size, a.ctypes.data, p.ctypes.data, n.ctypes.data)
        if code != 0:
            raise XlatingError("xlating_serve_outputs_device", code)
        return p, n

    def set_gain(self, client_id, gain_log2):
        """family "cf32-cs16": the client's rows as y * 2^(15 + gain_log2) from the next blocks call on; ends automatic gain"""
        code = serve_lib().xlating_serve_set_gain(self.h, client_id, int(gain_log2))
        if code != 0:
            raise XlatingError("xlating_serve_set_gain", code)

    def set_auto_gain(self, client_id, on=True):
        code = serve_lib().xlating_serve_set_auto_gain(self.h, client_id, 1 if on else 0)
        if code != 0:
            raise XlatingError("xlating_serve_set_auto_gain", code)

    def enable_levels(self, on=True):
        code = serve_lib().xlating_serve_enable_levels(self.h, 1 if on else 0)
        if code != 0:
            raise XlatingError("xlating_serve_enable_levels", code)

    def levels(self, cids):
        """-> dict of arrays [n]: peak_bits, clipped, nans (uint32), gain_log2 (int8) of the latest call queued to the sinks, and
        clipped_total (uint64) since each client joined"""
        a = np.ascontiguousarray(cids, dtype=np.intc)
        out = {"peak_bits": np.zeros(a.size, np.uint32), "clipped": np.zeros(a.size, np.uint32), "nans": np.zeros(a.size, np.uint32),
               "gain_log2": np.zeros(a.size, np.int8), "clipped_total": np.zeros(a.size, np.uint64)}
        code = serve_lib().xlating_serve_levels(self.h, a.size, a.ctypes.data, *[v.ctypes.data for v in out.values()])
        if code != 0:
            raise XlatingError("xlating_serve_levels", code)
        return out

    def gain_log(self, client_id, cap=64):
        """-> [(first_sample, gain_log2)]: the client's latest gain changes, oldest first"""
        f, g = np.zeros(cap, np.uint64), np.zeros(cap, np.int8)
        n = serve_lib().xlating_serve_gain_log(self.h, client_id, cap, f.ctypes.data, g.ctypes.data)
        if n < 0:
            raise XlatingError("xlating_serve_gain_log", n)
        return [(int(f[i]), int(g[i])) for i in range(n)]

    def set_tune(self, client_id, shift_hz, ramp_hz_per_s=0.0):
        """families "cf32" and "cf32-cs16": the client's final row rotated, phase-continuously, by shift_hz ramping by ramp_hz_per_s
        from the next blocks call on (include/xlating_serve.h; the rotation follows the client's filters)"""
        code = serve_lib().xlating_serve_set_tune(self.h, client_id, float(shift_hz), float(ramp_hz_per_s))
        if code != 0:
            raise XlatingError("xlating_serve_set_tune", code)

    def tune_log(self, client_id, cap=64):
        """-> [(first_sample, F, R)]: the client's latest changes of rotation, oldest first"""
        f, F, R = np.zeros(cap, np.uint64), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        n = serve_lib().xlating_serve_tune_log(self.h, client_id, cap, f.ctypes.data, F.ctypes.data, R.ctypes.data)
        if n < 0:
            raise XlatingError("xlating_serve_tune_log", n)
        return [(int(f[i]), int(F[i]), int(R[i])) for i in range(n)]

    def set_squelch(self, client_id, open_power, close_power=None, hang_calls=0):
        """every family: the client's rows are delivered only while its gate is open (mean power of its final row against the two
        marks, with hysteresis and a hang time in calls; include/xlating_serve.h), from the next blocks call on"""
        close_power = open_power if close_power is None else close_power
        code = serve_lib().xlating_serve_set_squelch(self.h, client_id, float(open_power), float(close_power), int(hang_calls))
        if code != 0:
            raise XlatingError("xlating_serve_set_squelch", code)

    def clear_squelch(self, client_id):
        code = serve_lib().xlating_serve_clear_squelch(self.h, client_id)
        if code != 0:
            raise XlatingError("xlating_serve_clear_squelch", code)

    def squelch_state(self, cids):
        """-> dict of arrays [n]: power (float64), open (uint8) of the latest blocks call, withheld_samples (uint64) since each joined"""
        a = np.ascontiguousarray(cids, dtype=np.intc)
        out = {"power": np.zeros(a.size, np.float64), "open": np.zeros(a.size, np.uint8), "withheld_samples": np.zeros(a.size, np.uint64)}
        code = serve_lib().xlating_serve_squelch_state(self.h, a.size, a.ctypes.data, *[v.ctypes.data for v in out.values()])
        if code != 0:
            raise XlatingError("xlating_serve_squelch_state", code)
        return out

    def squelch_log(self, client_id, cap=64):
        """-> [(stream_sample, delivered_sample, open)]: the client's latest gate changes, oldest first"""
        a, b, o = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
        n = serve_lib().xlating_serve_squelch_log(self.h, client_id, cap, a.ctypes.data, b.ctypes.data, o.ctypes.data)
        if n < 0:
            raise XlatingError("xlating_serve_squelch_log", n)
        return [(int(a[i]), int(b[i]), int(o[i])) for i in range(n)]

    def dropped(self, cap=4096):
        ids = (C.c_int * cap)()
        n = serve_lib().xlating_serve_dropped(self.h, ids, cap)
        return [ids[i] for i in range(n)]

    def engine(self):
        """The object's BatchEngine (owned by it: do not close it, add or remove clients through it)."""
        e = BatchEngine.__new__(BatchEngine)
        e.h = C.c_void_p(serve_lib().xlating_serve_engine(self.h))
        e.in_fmt = self.in_fmt
        e.close = lambda: None
        return e

    def last_ops(self):
        """-> (launches behind the engine call, copies behind it, bytes of the device-to-host copy) of the latest blocks call"""
        a, b, c = C.c_uint(0), C.c_uint(0), C.c_uint64(0)
        serve_lib().xlating_serve_last_ops(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def sink_stats(self):
        """-> (bytes handed to the OS / zlib, rows refused by a failed sink) since creation: Sinks.stats of the object's sinks"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        serve_lib().xlating_serve_sink_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            serve_lib().xlating_serve_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
