"""ctypes binding of libadapted_hip.so (include/adapted_hip.h) and the row <-> DetectResults
conversion shared by the operators and the CSV writer.

There is no CPU fallback: if the HIP library cannot be loaded the import of this module's
``load()`` fails loudly, and every operator of the package goes through it.
"""
from __future__ import annotations

import ctypes as C
import operator
import os
import sys
from typing import List, Optional, Sequence

import numpy as np

from . import build as _build
from .container_types import DetectResults

_LIB = None

NCOL = 39
MAX_CAND = 16
MAX_OPEN_PORES = 16

ADP_IN_DEVICE, ADP_OUT_DEVICE, ADP_WITH_START_PEAK, ADP_TOPK_NONE, ADP_BOUNDS_HOST, ADP_TAILS_NAN = 1, 2, 4, 8, 16, 32
ADP_CNN_FALLBACK = 1 << 17  # adp_detect_cnn: the short-read LLR fallback inside the call
ADP_CNN_SECOND_LLR = 1 << 18  # adp_detect_cnn: reads that fail get the LLR path's row where that one passes (row["reserved_"] bit 0)
ADP_FLAG_TRUNCATED = 1 << 19  # adp_detect_llr / adp_detect_cnn: flag poly(A) tails cut off by the preload window (row["reserved_"] bits 1, 2)
ADP_POLYA_TRUNCATED = 1 << 20  # adp_validate_candidates: Boundaries.polya_truncated is True -- no RNA partition
ADP_LLR_RESEGMENT = 1 << 21  # adp_detect_llr: re-segment failed reads behind their first change point (row["reserved_"] bits 5-9)
ADP_CNN_SECOND_RESEGMENT = 1 << 23  # adp_detect_cnn(_i16), with ADP_CNN_SECOND_LLR: re-segment the reads the second opinion fails too
ROW_FROM_SECOND_LLR = 1  # bits of row["reserved_"]
ROW_POLYA_TRUNCATED = 2  # the poly(A) runs into the end of the preloaded window
ROW_TRUNC_LOOKED = 4  # the call looked for that (every row of a call made with ADP_FLAG_TRUNCATED)
ROW_ADAPTER_FRONT = 8  # adp_adapter_front moved adapter_start: adapter_start / _len / _mean / _std / _med / _mad are the trimmed adapter's
ROW_REVALIDATED = 16  # adp_adapter_front_revalidate replaced the row by the validation from the trimmed start (beside ROW_ADAPTER_FRONT)
ROW_RESEGMENTED = 32  # the row is the validation of the second segmentation (ADP_LLR_RESEGMENT, include/adapted_hip_resegment.h)
ROW_FIRST_FAIL_SHIFT, ROW_FIRST_FAIL_MASK = 6, 15 << 6  # ... and bits 6-9 hold the fail_code of the row it replaced
ADP_ERR_UNSUPPORTED = -4
MB_OK, MB_MAD_ZERO, MB_EMPTY_TRACE = 0, 1, 2

COLS = ["signal_len", "preloaded", "adapter_start", "adapter_end", "adapter_len", "adapter_mean",
        "adapter_std", "adapter_med", "adapter_mad", "polya_start", "polya_end", "polya_len",
        "polya_mean", "polya_std", "polya_med", "polya_mad", "rna_preloaded_start",
        "rna_preloaded_len", "rna_preloaded_mean", "rna_preloaded_std", "rna_preloaded_med",
        "rna_preloaded_mad", "start_peak_idx", "start_peak_pa", "start_peak_next_max_idx",
        "start_peak_next_max_pa", "start_peak_open_pore_idx", "adapter_rna_median_shift",
        "{primary}_adapter_end", "{primary}_polya_end", "mvs_detect_mean_at_loc",
        "mvs_detect_var_at_loc", "mvs_detect_polya_med", "mvs_detect_polya_local_range",
        "mvs_detect_med_shift", "real_adapter_mean_start", "real_adapter_mean_end",
        "real_adapter_local_range", "mvs_adapter_end"]
assert len(COLS) == NCOL
_INT_COLS = {0, 1, 2, 3, 4, 9, 10, 11, 16, 17, 22, 24, 26, 28, 29, 38}
# columns the reference holds as numpy float32 scalars (kept as float32 so that the CSV
# writer rounds them like pandas does)
_F32_COLS = {23, 25, 27}

ROW_DTYPE = np.dtype([("col", "<f8", (NCOL,)), ("present", "<u8"), ("success", "<i4"), ("fail_code", "<i4"),
                      ("mvs_fail_mask", "<i4"), ("start_peak_type", "<i4"), ("n_cand", "<i4"),
                      ("n_open_pores", "<i4"), ("cand", "<i8", (MAX_CAND,)), ("open_pores", "<i4", (MAX_OPEN_PORES,)),
                      ("open_pores_more", "<i4"), ("reserved_", "<i4")])

# open_pores lists longer than a row holds (the reference's list has no length limit): host rows carry a token into this
# registry in `open_pores_more` (Engine._attach_open_pores swaps the arena offset of the call for it), so that rows can be
# sliced, concatenated and gathered freely before they become DetectResults
_OPEN_PORES_MORE: dict = {}
_open_pores_token = [0]


def register_open_pores(arr) -> int:
    _open_pores_token[0] += 1
    _OPEN_PORES_MORE[_open_pores_token[0]] = np.asarray(arr, dtype=np.int64)
    return _open_pores_token[0]


def clear_open_pores():
    _OPEN_PORES_MORE.clear()


def empty_rows(n: int) -> np.ndarray:
    """n zeroed result rows (the all-None rows of exceptions and dropped minibatches)"""
    rows = np.zeros(n, dtype=ROW_DTYPE)
    rows["n_cand"] = -1
    rows["n_open_pores"] = -1
    rows["open_pores_more"] = -1
    return rows


FAIL_REASONS = {
    0: None,
    1: "No adapter detected (primary)",
    2: "adapter MAD check failed",
    3: "Open pore too close to boundary",
    4: "Real signal check failed",
    5: "No polya detected (primary)",
    6: "MVS polya check failed: not enough signal",
    7: "MVS polya check failed: ",
    8: "Median shift check failed",
    9: "'NoneType' object is not iterable",
    10: "slice indices must be integers or None or have an __index__ method",
    11: "Moving window must between 1 and n, inclusive",
    12: "pA_mean_range is not specified",
    13: "attempt to get argmin of an empty sequence",
    14: "MAD normalization failed: scale is 0",
    15: "No adapter detected in range (mvs_detect)",
}
_MVS_NAMES = ["mean", "var", "med", "range", "shift"]
START_PEAK_TYPES = {0: None, 1: "open pore in adapter", 2: "potential concatemer adapter-only read"}
PRIMARY_CODE = {"llr": 0, "cnn": 1, "start_peak": 2}


class AdpCfg(C.Structure):
    _fields_ = [
        ("min_obs_adapter", C.c_int32), ("max_obs_adapter", C.c_int32), ("min_obs_polya", C.c_int32),
        ("downscale_factor", C.c_int32), ("max_obs_trace", C.c_int32), ("primary_method", C.c_int32),
        ("sig_norm_outlier_thresh", C.c_double),
        ("adapter_peak_prominence", C.c_double), ("adapter_peak_rel_height", C.c_double),
        ("adapter_peak_width", C.c_int32),
        ("mvs_detect_check", C.c_int32), ("mvs_detect_overwrite", C.c_int32), ("search_window", C.c_int32),
        ("pA_mean_window", C.c_int32), ("pA_var_window", C.c_int32), ("median_shift_window", C.c_int32),
        ("polyA_window", C.c_int32),
        ("pA_mean_range", C.c_double * 2), ("pA_var_range", C.c_double * 2),
        ("median_shift_range", C.c_double * 2), ("polyA_med_range", C.c_double * 2),
        ("polyA_local_range", C.c_double * 2), ("pA_mean_adapter_med_scale_range", C.c_double * 2),
        ("detect_open_pores", C.c_int32), ("real_signal_check", C.c_int32), ("mean_window", C.c_int32),
        ("max_obs_local_range", C.c_int32),
        ("mean_start_range", C.c_double * 2), ("mean_end_range", C.c_double * 2),
        ("local_range", C.c_double * 2), ("adapter_mad_range", C.c_double * 2),
        ("detect_med_shift", C.c_int32), ("med_shift_window", C.c_int32), ("med_shift_range", C.c_double * 2),
        ("sp_downscale_factor", C.c_int32), ("start_peak_max_idx", C.c_int32), ("sp_offset1", C.c_int32),
        ("sp_offset2", C.c_int32), ("open_pore_pa", C.c_double),
        ("polya_cand_k", C.c_int32), ("fallback_to_llr_short_reads", C.c_int32),
    ]


class HipLibraryError(RuntimeError):
    pass


def hip_runtimes() -> List[str]:
    """paths of every HIP runtime (libamdhip64) mapped into this process -- one entry is the healthy state"""
    seen = []
    try:
        with open("/proc/self/maps") as fh:
            for ln in fh:
                path = ln.split(None, 5)[-1].strip() if ln.count("/") else ""
                if "libamdhip64" in os.path.basename(path) and path not in seen:
                    seen.append(path)
    except OSError:
        pass
    return seen


def _elf_dynamic(path: str):
    """(SONAME or None, [DT_NEEDED names]) of a little-endian ELF64 shared object -- read from the file, nothing is loaded
    (the ELF header, the program headers, the dynamic section and the strings it names: a few KB of a multi-MB runtime)"""
    import struct

    with open(path, "rb") as fh:
        def at(off, size):
            fh.seek(off)
            return fh.read(size)

        head = at(0, 0x40)
        if head[:6] != b"\x7fELF\x02\x01":
            raise ValueError("not a little-endian ELF64 file: %s" % path)
        e_phoff, = struct.unpack_from("<Q", head, 0x20)
        e_phentsize, e_phnum = struct.unpack_from("<HH", head, 0x36)
        ph = at(e_phoff, e_phentsize * e_phnum)
        loads, dyn = [], None
        for i in range(e_phnum):
            p_type, _flags, p_offset, p_vaddr, _paddr, p_filesz = struct.unpack_from("<IIQQQQ", ph, i * e_phentsize)
            if p_type == 1:
                loads.append((p_vaddr, p_offset, p_filesz))
            elif p_type == 2:
                dyn = (p_offset, p_filesz)
        if dyn is None:
            return None, []

        def off_of(vaddr):
            for va, off, sz in loads:
                if va <= vaddr < va + sz:
                    return off + (vaddr - va)
            raise ValueError("address outside the file's segments")

        tags = []
        dsec = at(dyn[0], dyn[1])
        for o in range(0, len(dsec) - 15, 16):
            tag, val = struct.unpack_from("<qQ", dsec, o)
            if tag == 0:
                break
            tags.append((tag, val))
        strtab = off_of(next(v for t, v in tags if t == 5))

        def name(v):
            buf = b""
            while b"\0" not in buf:  # (names are short: one or two reads)
                more = at(strtab + v + len(buf), 256)
                if not more:
                    break
                buf += more
            return buf.split(b"\0", 1)[0].decode()

        return next((name(v) for t, v in tags if t == 14), None), [name(v) for t, v in tags if t == 1]


def _share_torch_runtime(lib_path: Optional[str] = None):
    """One process, ONE HIP runtime, whatever the import order.  PyTorch-ROCm wheels bundle a libamdhip64.so; when its SONAME is
    the one libadapted_hip.so was linked against (libamdhip64.so.7 with this image's wheel and /opt/rocm), this library loaded
    after torch binds to torch's copy by itself, and loaded BEFORE torch it would bind to /opt/rocm's and a later `import torch`
    would map a second runtime beside it (two runtimes = two device contexts: RCCL, events and allocations of one are invisible to
    the other).  So when no runtime is mapped yet and a torch wheel is installed whose bundled runtime carries exactly that
    SONAME, map that copy first (by path, without importing torch); the dynamic loader then resolves both this library and a
    later torch to it.  A wheel whose runtime has another SONAME (another ROCm major) is left alone: this library then runs on the
    system runtime it was built against, as it did before.  ADAPTED_HIP_RUNTIME=system keeps /opt/rocm's runtime in any case
    (fine for processes that never import torch)."""
    if os.environ.get("ADAPTED_HIP_RUNTIME", "auto") == "system" or hip_runtimes():
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if not os.path.exists(cand):
            return
        want = [n for n in _elf_dynamic(lib_path or _build.LIB)[1] if n.startswith("libamdhip64")]
        have = _elf_dynamic(cand)[0]
        if want and have == want[0]:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:  # noqa: BLE001 -- no torch, or an unusual install: the system runtime it is
        pass


def assert_one_runtime():
    """Raise HipLibraryError when two HIP runtimes are mapped into this process AND torch is imported: torch's device context and
    this library's would not see each other (RCCL, events, allocations).  Without torch a second mapped copy is idle and harmless.
    Checked when the library is loaded and again at every entry point that hands torch's device memory to the library or the
    library's rows to torch.distributed (Engine calls with device pointers, parallel.gather_rows, bench.py's process group): a
    torch imported AFTER the library was loaded on another runtime is caught there instead of failing silently."""
    rts = hip_runtimes()
    if len(rts) > 1 and "torch" in sys.modules:
        raise HipLibraryError("two HIP runtimes are mapped into this process (%s) and torch is imported: import torch BEFORE anything "
                              "that links /opt/rocm's libamdhip64, or -- for a process that does not need torch on the GPU -- set "
                              "ADAPTED_HIP_RUNTIME=system before adapted_amd.lib is loaded and do not import torch" % ", ".join(rts))


_RUNTIME_CHECKED_WITH_TORCH = False


def _check_runtime_once_torch_is_here():
    """assert_one_runtime, once per process after torch has appeared (reading /proc/self/maps per call would cost a detect call ~1 ms)"""
    global _RUNTIME_CHECKED_WITH_TORCH
    if not _RUNTIME_CHECKED_WITH_TORCH and "torch" in sys.modules:
        assert_one_runtime()
        _RUNTIME_CHECKED_WITH_TORCH = True


def load():
    """Load (building if needed) libadapted_hip.so.  Raises HipLibraryError if impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    try:
        path = os.environ.get("ADAPTED_HIP_LIB") or _build.build()  # (override: a developer's experimental build)
        _share_torch_runtime(path)
        lib = C.CDLL(path)
    except Exception as e:  # no CPU fallback by design
        raise HipLibraryError("libadapted_hip.so is required (hipcc build or load failed): %s" % e) from e
    assert_one_runtime()
    try:
        for name, proto in (list(PROTOTYPES.items()) + list(MODULE_PROTOTYPES.items()) + list(I16_PROTOTYPES.items())
                            + list(EVENT_PROTOTYPES.items()) + list(FINGERPRINT_PROTOTYPES.items())
                            + list(EVENT_PACKED_PROTOTYPES.items())
                            + list(ADAPTER_FRONT_PROTOTYPES.items()) + list(REVALIDATE_PROTOTYPES.items())
                            + list(TEMPLATE_PROTOTYPES.items()) + list(RESEGMENT_PROTOTYPES.items()) + list(CSV_PROTOTYPES.items())
                            + list(CLUSTER_PROTOTYPES.items()) + list(KNN_PROTOTYPES.items())
                            + list(SECOND_RESEGMENT_PROTOTYPES.items())):
            ret, params = proto.split(":")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _RETURNS[ret], [_argtype(kind) for kind in params.split()]
    except AttributeError as e:
        raise HipLibraryError("libadapted_hip.so does not export what include/adapted_hip.h declares: %s" % e) from e
    if (lib.adp_sizeof_cfg() != C.sizeof(AdpCfg) or lib.adp_sizeof_row() != ROW_DTYPE.itemsize
            or lib.adp_sizeof_peak_args() != C.sizeof(AdpPeakArgs) or lib.adp_sizeof_spike_args() != C.sizeof(AdpSpikeArgs)
            or lib.adp_sizeof_mvs_args() != C.sizeof(AdpMvsArgs) or lib.adp_sizeof_seg() != SEG_DTYPE.itemsize
            or lib.adp_sizeof_real_range_args() != C.sizeof(AdpRealRangeArgs)
            or lib.adp_sizeof_start_peak_args() != C.sizeof(AdpStartPeakArgs)
            or lib.adp_sizeof_adapter_start_args() != C.sizeof(AdpAdapterStartArgs)
            or lib.adp_sizeof_event_args() != C.sizeof(AdpEventArgs)
            or lib.adp_sizeof_adapter_front_args() != C.sizeof(AdpAdapterFrontArgs)):
        raise HipLibraryError("ABI mismatch between adapted_amd/lib.py and libadapted_hip.so")
    _LIB = lib
    return lib


class AdpTraceArgs(C.Structure):
    """struct adp_trace_args (include/adapted_hip.h): the keyword arguments of the reference's c_llr_trace"""
    _fields_ = [(k, C.c_int32) for k in ("min_obs", "border_trim", "stride", "adapter_early_stopping", "adapter_early_stop_window",
                                         "adapter_early_stop_stride", "polya_early_stopping", "polya_early_stop_window",
                                         "polya_early_stop_stride")]


class AdpPeakArgs(C.Structure):
    """struct adp_peak_args (include/adapted_hip.h): find_peaks_in_trace's and the two corrections' parameters"""
    _fields_ = [(k, C.c_double) for k in ("prominence", "width", "rel_height", "plateau_t", "split_t", "split_prominence")] + \
               [(k, C.c_int32) for k in ("plateau_on", "plateau_s", "plateau_window", "split_on", "split_s", "split_window")]


class AdpSpikeArgs(C.Structure):
    """struct adp_spike_args (include/adapted_hip.h): detect_full_polya_trace_peak_with_spike's parameters"""
    _fields_ = [(k, C.c_double) for k in ("min_peak_distance", "prominence_threshold", "min_width", "threshold_prominence_ratio",
                                          "threshold_r_squared")]


class AdpMvsArgs(C.Structure):
    """struct adp_mvs_args (include/adapted_hip.h): the [mvs_polya] and [streaming] parameters of the MVS module, plus its flags"""
    _fields_ = [(k, C.c_double * 2) for k in ("pA_mean_range", "pA_var_range", "median_shift_range", "polyA_med_range", "polyA_local_range")] + \
               [(k, C.c_int32) for k in ("search_window", "pA_mean_window", "pA_var_window", "median_shift_window", "polyA_window",
                                         "less_signal_ok", "windowed_stats", "min_obs_adapter", "min_obs_post_loc", "search_increment_step",
                                         "s_pA_mean_window", "s_pA_var_window", "s_median_shift_window", "s_polyA_window", "pad")] + \
               [(k, C.c_double * 2) for k in ("s_pA_mean_range", "s_pA_var_range", "s_median_shift_range", "s_polyA_med_range",
                                              "s_polyA_local_range")]


class AdpRealRangeArgs(C.Structure):
    """struct adp_real_range_args (include/adapted_hip.h): the [real_range] parameters real_range_check reads"""
    _fields_ = [(k, C.c_double * 2) for k in ("mean_start_range", "mean_end_range", "local_range")] + \
               [(k, C.c_int32) for k in ("mean_window", "max_obs_local_range")]


class AdpStartPeakArgs(C.Structure):
    """struct adp_start_peak_args (include/adapted_hip.h): the [rna_start_peak] parameters detect_rna_start_peak reads"""
    _fields_ = [("open_pore_pa", C.c_double)] + [(k, C.c_int32) for k in ("downscale_factor", "start_peak_max_idx", "offset1", "offset2")]


class AdpAdapterStartArgs(C.Structure):
    """struct adp_adapter_start_args (include/adapted_hip.h): MMAdapterStartConfig's parameters"""
    _fields_ = [(k, C.c_double) for k in ("min_shift", "min_pA_current")] + [(k, C.c_int32) for k in ("window", "min_obs_adapter")]


class AdpAdapterFrontArgs(C.Structure):
    """struct adp_adapter_front_args (include/adapted_hip_adapter_front.h): adp_adapter_start_args, then the least adapter a patched
    row may be left with"""
    _fields_ = AdpAdapterStartArgs._fields_ + [(k, C.c_int32) for k in ("min_adapter_len", "pad")]


class AdpEventArgs(C.Structure):
    """struct adp_event_args (include/adapted_hip_events.h): the parameters of the event segmentation"""
    _fields_ = [(k, C.c_double) for k in ("threshold", "var_floor")] + [(k, C.c_int32) for k in ("window", "min_distance")]


# the event segmentation's tile (EV_TILE: positions per workgroup of k_ev_scores) and the default byte budget, in MiB, of a call's batch
# of slots (EV_SCRATCH_MIB; ADP_EVENTS_SCRATCH_MIB in the environment replaces it, read per call) -- adapted_amd/csrc/events_api.h;
# tests/test_events_cpu.py holds both against that header
EVENTS_TILE = 1024
EVENTS_SCRATCH_MIB = 512


def events_slot_bytes(longest: int) -> int:
    """the scratch one segment takes in adp_segment_events when the call's longest clipped segment has ``longest`` samples"""
    stride = (max(int(longest), 1) + 1) & ~1
    return stride * 8 + (stride // 2 + 1) * 8


# the widest event table of adp_event_levels, the longest query / template and the most templates of adp_dtw_assign, and the default
# byte budget, in MiB, of that call's distance matrix (ADP_DTW_SCRATCH_MIB in the environment replaces it, read per call) --
# FP_EMAX, DTW_NT_MAX and DTW_SCRATCH_MIB of adapted_amd/csrc/fingerprint_api.h; tests/test_fingerprint_cpu.py holds them against it
FINGERPRINT_MAX_EVENTS = 512
DTW_MAX_TEMPLATES = 4096
DTW_SCRATCH_MIB = 512

# the chunk length of k_adapter_start's LDS staging (ASC_CHUNK, adapted_amd/csrc/startmods_api.h): its chains change path there
ADAPTER_START_CHUNK = 512

# struct adp_seg (include/adapted_hip.h): a segment signal[row, start:end] of a batch
SEG_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("row", "<i4"), ("pad", "<i4")])

ADP_TRACE_FROM_SUMS = 64
ADP_LLR_INTERP = 512
ADP_LLR_GIVEN_PEAK = 1024
ADP_CLLR_POLYA = 128
ADP_CLLR_F32 = 256
ADP_MVS_F64 = 2048
ADP_SS_NANSKIP = 4096
ADP_SS_WHOLE = 8192
ADP_SS_CLIP = 16384
ADP_SS_FORCE_GRID = 32768
ADP_SS_FORCE_WAVE = 65536
ADP_SS_GRID_MIN = 16384


# -- the C ABI, declared once -------------------------------------------------------------------------------------------------
# include/adapted_hip.h as "return: parameters", in header order.  Scalars: int, int32, uint32, uint64, float, double.  T* points
# to elements T: a number type, adp_row (ROW_DTYPE), adp_seg (SEG_DTYPE), void (anything), one of the structs above, or a handle.
# load() turns every line into restype / argtypes; tests/test_host_cpu.py holds the table against the header.
PROTOTYPES = {
    "adp_abi_version": "int:",
    "adp_sizeof_cfg": "int:",
    "adp_sizeof_row": "int:",
    "adp_last_error": "char*:",
    "adp_device_count": "int:",
    "adp_create": "int: int adp_cfg* int int adp_handle**",
    "adp_destroy": "int: adp_handle*",
    "adp_set_config": "int: adp_handle* adp_cfg*",
    "adp_set_layout": "int: adp_handle* int",
    "adp_stream": "void*: adp_handle*",
    "adp_synchronize": "int: adp_handle*",
    "adp_detect_llr": "int: adp_handle* float* int32* int int int int adp_row* int32*",
    "adp_detect_llr_i16": "int: adp_handle* int16* int32* float* float* int int int int adp_row* int32*",
    "adp_detect_start_peak": "int: adp_handle* float* int32* int int int int adp_row*",
    "adp_cnn_prepare": "int: adp_handle* float* int int int float*",
    "adp_cnn_set_weights": "int: adp_handle* float* float* float* float* float* float* float* float*",
    "adp_cnn_forward": "int: adp_handle* float* int int float*",
    "adp_cnn_predict": "int: adp_handle* float* int int int int64*",
    "adp_cnn_topk": "int: adp_handle* float* int64* int64* int int int int32* int32*",
    "adp_detect_cnn": "int: adp_handle* float* int32* int int int int adp_row* int64*",
    "adp_validate_candidates": "int: adp_handle* float* int32* int int int64* int int adp_row*",
    "adp_llr_refine_polya": "int: adp_handle* float* int32* int int int64* int int64* int32*",
    "adp_open_pores_arena": "int: adp_handle* int32* uint64 uint64*",
    "adp_synth_fill": "int: adp_handle* float* int32* int int uint32 uint32 int",
    "adp_dev_alloc": "int: adp_handle* uint64 void**",
    "adp_dev_free": "int: adp_handle* void*",
    "adp_memcpy_h2d": "int: adp_handle* void* void* uint64",
    "adp_memcpy_d2h": "int: adp_handle* void* void* uint64",
    "adp_calibrate_i16": "int: adp_handle* int16* int32* float* float* int int float*",
    "adp_expand_ragged": "int: adp_handle* void* int int64* int32* float* float* int int float*",
    "adp_expand_ragged_i16": "int: adp_handle* int16* int64* int32* int int int16*",
    "adp_host_alloc": "int: adp_handle* uint64 void**",
    "adp_host_free": "int: adp_handle* void*",
    "adp_memcpy_h2d_async": "int: adp_handle* void* void* uint64",
    "adp_copy_mark": "int: adp_handle* int",
    "adp_copy_wait": "int: adp_handle* int",
    "adp_c_llr_trace": "int: adp_handle* double* int32* int32* int32* int int adp_trace_args* int double* double* double*",
    "adp_c_llr_best_split": "int: adp_handle* double* double* int32* int32* int32* int32* int32* int int int int64* double*",
    "adp_c_llr_detect": "int: adp_handle* void* int32* int int int32 int32 int32 int int64* int64* double*",
    "adp_sizeof_peak_args": "int:",
    "adp_sizeof_spike_args": "int:",
    "adp_llr_trace_bounds": "int: adp_handle* double* int32* int32* int32* int int int int int32* int32* int32*",
    "adp_llr_trace_peaks": "int: adp_handle* double* int32* int32* int32* int int adp_peak_args* int int int64* int64*",
    "adp_llr_spike_peak": "int: adp_handle* double* int32* int int adp_spike_args* int int64*",
    "adp_sizeof_mvs_args": "int:",
    "adp_mvs_check": "int: adp_handle* void* int32* int64* int64* int int adp_mvs_args* int int32* double*",
    "adp_mvs_detect_at_loc": "int: adp_handle* void* int32* int64* int int adp_mvs_args* int int32* int64* double*",
    "adp_mvs_detect": "int: adp_handle* void* int32* int int adp_mvs_args* int int64*",
    "adp_sizeof_seg": "int:",
    "adp_seg_stats": "int: adp_handle* void* int32* int int adp_seg* int int double* int64*",
    "adp_sizeof_real_range_args": "int:",
    "adp_med_mad": "int: adp_handle* void* int32* int int int double*",
    "adp_normalize": "int: adp_handle* void* int32* int int double int double* void* int32*",
    "adp_pool_mean": "int: adp_handle* void* int int int int void*",
    "adp_real_range": "int: adp_handle* void* int32* int int adp_seg* int adp_real_range_args* int int32* double*",
    "adp_open_pores": "int: adp_handle* void* int32* int int adp_seg* int double double double int int int64* int64*",
    "adp_set_profiling": "int: adp_handle* int",
    "adp_kernel_times": "int: adp_handle* char** float* int",
    "adp_debug_fetch": "int: adp_handle* int void* uint64",
    "adp_debug_llr_upto": "int: adp_handle* float* int32* int int int int int",
    "adp_debug_divcheck": "int: adp_handle* float uint32 uint32 uint64*",
    "adp_debug_log": "int: adp_handle* double* double* int",
}
EXPORTS = list(PROTOTYPES)
# include/adapted_hip_startmods.h (the header adapted_hip.h includes for the start-peak and adapter-start modules), in the same
# vocabulary; load() binds both tables, tests/test_startmods_module_cpu.py holds this one against its header
MODULE_PROTOTYPES = {
    "adp_sizeof_start_peak_args": "int:",
    "adp_sizeof_adapter_start_args": "int:",
    "adp_start_peak": "int: adp_handle* void* int32* int int adp_start_peak_args* int int32* double*",
    "adp_adapter_start": "int: adp_handle* void* int32* int int adp_adapter_start_args* int int32* int64* int64* double*",
}
# include/adapted_hip_i16.h (the header adapted_hip.h includes for the CNN primary over raw int16 rows; adp_detect_llr_i16, the LLR
# primary's twin, stays in PROTOTYPES); tests/test_cnn_i16_cpu.py holds this table against its header
I16_PROTOTYPES = {
    "adp_detect_cnn_i16": "int: adp_handle* int16* int32* float* float* int int int int adp_row* int64*",
}

# include/adapted_hip_events.h (the header adapted_hip.h includes for the event segmentation, an extension);
# tests/test_events_cpu.py holds this table against its header
EVENT_PROTOTYPES = {
    "adp_sizeof_event_args": "int:",
    "adp_segment_events": "int: adp_handle* void* int32* int int adp_seg* int adp_event_args* int int int64* int64* double*",
}

# include/adapted_hip_fingerprint.h (the header adapted_hip.h includes for the adapter event fingerprints and their DTW
# distances to templates, an extension); tests/test_fingerprint_cpu.py holds this table against its header
FINGERPRINT_PROTOTYPES = {
    "adp_event_levels": "int: adp_handle* void* int32* int int adp_seg* int adp_event_args* int int int64* double* int32* int32* int32* "
                        "double* double* double*",
    "adp_dtw_assign": "int: adp_handle* double* int32* int int double* int32* int int int int double* int32* double*",
}

# include/adapted_hip_events_packed.h (the header adapted_hip.h includes for the packed forms of the two event calls -- segments back
# to back in one array, float32 pA or raw int16 samples with a calibration per segment --, an extension);
# tests/test_events_packed_cpu.py holds this table and the flag against its header
EVENT_PACKED_PROTOTYPES = {
    "adp_segment_events_packed": "int: adp_handle* void* int64* float* float* int adp_event_args* int int int64* int64* double*",
    "adp_event_levels_packed": "int: adp_handle* void* int64* float* float* int adp_event_args* int int int64* double* int32* int32* "
                               "int32* double* double* double*",
}
ADP_PACKED_I16 = 1 << 24  # the two packed event calls: raw int16 samples with a calibration per segment

# include/adapted_hip_adapter_front.h (the header adapted_hip.h includes for the adapter-front post-pass over the rows of a detect
# call, an extension); tests/test_adapter_front_cpu.py holds this table against its header
ADAPTER_FRONT_PROTOTYPES = {
    "adp_sizeof_adapter_front_args": "int:",
    "adp_adapter_front": "int: adp_handle* float* int32* int int adp_row* adp_adapter_front_args* int int32* int64* int64* double*",
    "adp_adapter_front_i16": "int: adp_handle* int16* int32* float* float* int int adp_row* adp_adapter_front_args* int int32* int64* "
                             "int64* double*",
}

# include/adapted_hip_revalidate.h (the header adapted_hip.h includes for the validation from a given adapter start and the
# adapter-front pass that validates its trimmed rows again, an extension); tests/test_revalidate_cpu.py holds this table against it
REVALIDATE_PROTOTYPES = {
    "adp_validate_candidates_from": "int: adp_handle* float* int32* int int int64* int64* int int adp_row*",
    "adp_adapter_front_revalidate": "int: adp_handle* float* int32* int int adp_row* adp_adapter_front_args* int int32* int64* int64* "
                                    "double* int32*",
    "adp_adapter_front_revalidate_i16": "int: adp_handle* int16* int32* float* float* int int adp_row* adp_adapter_front_args* int int32* "
                                        "int64* int64* double* int32*",
}

# include/adapted_hip_templates.h (the header adapted_hip.h includes for the warping path of a DTW alignment and the DBA iteration
# that build barcode templates, an extension); tests/test_dtw_align_cpu.py holds this table against its header
TEMPLATE_PROTOTYPES = {
    "adp_dtw_align": "int: adp_handle* double* int32* int32* int int double* int32* int int int int double* int32* int32* int32* double*",
    "adp_dba_step": "int: adp_handle* double* int32* int32* int int double* int32* int int int int double* int32* double* double*",
}

# include/adapted_hip_clusters.h (the header adapted_hip.h includes for the clustering of fingerprints without labels -- the
# all-pairs DTW matrix, PAM's BUILD, alternating k-medoids, the silhouette --, an extension); tests/test_clusters_cpu.py holds this
# table against its header
CLUSTER_PROTOTYPES = {
    "adp_dtw_pairwise": "int: adp_handle* double* int32* int int int int double*",
    "adp_kmedoids_build": "int: adp_handle* double* int int int int32* double*",
    "adp_kmedoids": "int: adp_handle* double* int int int int int32* int32* double* double* int32*",
    "adp_silhouette": "int: adp_handle* double* int int32* int int double*",
}
CLUSTER_MAX_ROWS = 16384  # CL_NMAX of adapted_amd/csrc/dtw_cluster_api.h
CLUSTER_MAX_K = 4096  # CL_KMAX

# include/adapted_hip_knn.h (the header adapted_hip.h includes for the k nearest labelled fingerprints of every query under DTW, an
# extension); tests/test_knn_cpu.py holds this table and the three constants against its header
KNN_PROTOTYPES = {
    "adp_dtw_knn": "int: adp_handle* double* int32* int int double* int32* int int int int int int32* int32* double* int64*",
}
ADP_KNN_NO_PRUNE = 1 << 22  # adp_dtw_knn: every pair runs to the end
KNN_KMAX = 32
KNN_NR_MAX = 262144

# include/adapted_hip_resegment.h (the header adapted_hip.h includes for the re-segmentation of reads the LLR primary fails, an
# extension): a flag of adp_detect_llr, row bits and a selector of adp_debug_fetch -- it declares no entry point;
# tests/test_resegment_cpu.py holds this table against its header
RESEGMENT_PROTOTYPES: dict = {}

# include/adapted_hip_second_resegment.h (the header adapted_hip.h includes for the same re-segmentation behind the CNN primary's LLR
# second opinion, an extension): a flag of adp_detect_cnn(_i16) and a selector of adp_debug_fetch -- no entry point, no row bit;
# tests/test_cnn_second_resegment_cpu.py holds this table against its header
SECOND_RESEGMENT_PROTOTYPES: dict = {}

# include/adapted_hip_csv.h (the header adapted_hip.h includes for the CSV text of one output file's rows, an extension);
# tests/test_native_csv_cpu.py holds this table against its header
CSV_PROTOTYPES = {
    "adp_format_rows": "int: adp_handle* adp_row* int int int void* int64* int64* int64* void* int32* int void* uint64 uint64* int32*",
}

_VoidP = C.c_void_p  # a handle, and what an adp_handle ** / void ** out-parameter points to
_RETURNS = {"int": C.c_int, "char*": C.c_char_p, "void*": _VoidP}
_SCALARS = {"int": C.c_int, "int32": C.c_int32, "uint32": C.c_uint32, "uint64": C.c_uint64, "float": C.c_float, "double": C.c_double}
_POINTEES = {"adp_cfg": AdpCfg, "adp_trace_args": AdpTraceArgs, "adp_peak_args": AdpPeakArgs, "adp_spike_args": AdpSpikeArgs,
            "adp_mvs_args": AdpMvsArgs, "adp_real_range_args": AdpRealRangeArgs, "adp_start_peak_args": AdpStartPeakArgs,
            "adp_adapter_start_args": AdpAdapterStartArgs, "adp_event_args": AdpEventArgs,
            "adp_adapter_front_args": AdpAdapterFrontArgs, "adp_handle*": _VoidP, "void*": _VoidP,
            "char*": C.c_char_p}
_ELEMENTS = {"float": np.float32, "double": np.float64, "int16": np.int16, "int32": np.int32, "int64": np.int64, "uint32": np.uint32,
             "uint64": np.uint64, "void": None, "adp_row": ROW_DTYPE, "adp_seg": SEG_DTYPE}
_CTYPES_ARGUMENT = (C._SimpleCData, C.Array, C._Pointer, type(C.byref(C.c_int())))


class _Pointer:
    """argtypes entry of a pointer to numbers, rows or segments -- the one place where an argument becomes an address.  Takes a
    device pointer (int) or None; a ctypes object (c_void_p, byref(...), a ctypes array) as it is; a numpy array only when it is
    C-contiguous and of the element type the header names (``void``: of any).  The array is an argument of the call and lives as
    long as it does."""

    def __init__(self, element):
        self.element, self.dtype = element, _ELEMENTS[element]

    def from_param(self, v):
        if isinstance(v, np.ndarray):
            if not v.flags.c_contiguous or (self.dtype is not None and v.dtype != self.dtype):
                raise TypeError("%s *: a C-contiguous %s array, not %s%s" % (self.element, np.dtype(self.dtype or np.void).name, v.dtype,
                                                                            "" if v.flags.c_contiguous else " with strides"))
            return C.c_void_p(v.ctypes.data)
        if isinstance(v, _CTYPES_ARGUMENT):
            return v
        return C.c_void_p(v if v is None else operator.index(v))


def _argtype(kind):
    """the ctypes side of one parameter kind of PROTOTYPES"""
    if kind in _SCALARS:
        return _SCALARS[kind]
    if kind == "adp_handle*":
        return _VoidP
    element = kind[:-1]
    return C.POINTER(_POINTEES[element]) if element in _POINTEES else _Pointer(element)


# a detect call's options -> their bits of its flag word (include/adapted_hip.h)
_OPTION_FLAGS = {"with_start_peak": ADP_WITH_START_PEAK, "tails_nan": ADP_TAILS_NAN, "flag_truncated": ADP_FLAG_TRUNCATED,
                 "fallback": ADP_CNN_FALLBACK, "second_opinion": ADP_CNN_SECOND_LLR, "resegment": ADP_LLR_RESEGMENT}


# what a CNN call's ``second_opinion`` argument may say: nothing, the LLR second opinion, or that with the re-segmentation of the
# reads it fails too (ADP_CNN_SECOND_RESEGMENT, include/adapted_hip_second_resegment.h)
SECOND_OPINIONS = ("llr", "llr_resegment")


def second_opinion_flags(value) -> int:
    """a ``second_opinion`` argument -> its bits: False / None 0, True / "llr" ADP_CNN_SECOND_LLR, "llr_resegment" that and
    ADP_CNN_SECOND_RESEGMENT; anything else is a ValueError"""
    if value is None or value is False:
        return 0
    if value is True or value == "llr":
        return ADP_CNN_SECOND_LLR
    if value == "llr_resegment":
        return ADP_CNN_SECOND_LLR | ADP_CNN_SECOND_RESEGMENT
    raise ValueError("second_opinion: one of False, True, %s, not %r" % (", ".join(repr(v) for v in SECOND_OPINIONS), value))


def _flag_word(**options) -> int:
    return sum(second_opinion_flags(on) if name == "second_opinion" else _OPTION_FLAGS[name] for name, on in options.items() if on)


class MinibatchDropped(RuntimeError):
    """batch-level failure of one minibatch (the reference drops it and logs): status = ADP_MB_*"""

    def __init__(self, status: int):
        super().__init__("minibatch dropped (status %d)" % status)
        self.status = status


def bounds(r, nan_ok=False):
    """a (min, max) range with None for an open end -> (float, float)"""
    lo, hi = (None, None) if r is None else r
    lo, hi = (-np.inf if lo is None else float(lo), np.inf if hi is None else float(hi))
    if not nan_ok and (lo != lo or hi != hi):
        raise ValueError("a range bound must be a number or None")
    return lo, hi


def make_cfg(spc) -> AdpCfg:
    c = AdpCfg()
    co = spc.core
    c.min_obs_adapter, c.max_obs_adapter, c.min_obs_polya = int(co.min_obs_adapter), int(co.max_obs_adapter), int(co.min_obs_polya)
    c.downscale_factor, c.max_obs_trace = int(co.downscale_factor), int(co.max_obs_trace)
    c.primary_method = PRIMARY_CODE[spc.primary_method]
    c.sig_norm_outlier_thresh = float(co.sig_norm_outlier_thresh)
    L = spc.llr_boundaries
    c.adapter_peak_prominence, c.adapter_peak_rel_height = float(L.adapter_peak_prominence), float(L.adapter_peak_rel_height)
    c.adapter_peak_width = int(L.adapter_peak_width)
    M = spc.mvs_polya
    for k in ("mvs_detect_check", "mvs_detect_overwrite", "search_window", "pA_mean_window", "pA_var_window",
              "median_shift_window", "polyA_window"):
        setattr(c, k, int(getattr(M, k)))
    for k in ("pA_mean_range", "pA_var_range", "median_shift_range", "polyA_med_range", "polyA_local_range",
              "pA_mean_adapter_med_scale_range"):
        setattr(c, k, bounds(getattr(M, k), nan_ok=True))
    R = spc.real_range
    for k in ("detect_open_pores", "real_signal_check", "mean_window", "max_obs_local_range"):
        setattr(c, k, int(getattr(R, k)))
    for k in ("mean_start_range", "mean_end_range", "local_range", "adapter_mad_range"):
        setattr(c, k, bounds(getattr(R, k), nan_ok=True))
    c.detect_med_shift, c.med_shift_window = int(spc.med_shift.detect_med_shift), int(spc.med_shift.med_shift_window)
    c.med_shift_range = bounds(spc.med_shift.med_shift_range, nan_ok=True)
    S = spc.rna_start_peak
    c.sp_downscale_factor, c.start_peak_max_idx = int(S.downscale_factor), int(S.start_peak_max_idx)
    c.sp_offset1, c.sp_offset2, c.open_pore_pa = int(S.offset1), int(S.offset2), float(S.open_pore_pa)
    c.polya_cand_k = int(spc.cnn_boundaries.polya_cand_k)
    c.fallback_to_llr_short_reads = int(spc.cnn_boundaries.fallback_to_llr_short_reads)
    return c


def fail_reason_of(row) -> Optional[str]:
    fc = int(row["fail_code"])
    fr = FAIL_REASONS[fc]
    if fc == 7:
        fr += " ".join(n for b, n in enumerate(_MVS_NAMES) if int(row["mvs_fail_mask"]) >> b & 1)
    return fr


_RNA_FIELDS = ("rna_preloaded_start", "rna_preloaded_len", "rna_preloaded_mean", "rna_preloaded_std", "rna_preloaded_med",
               "rna_preloaded_mad")


def truncation_unsupported(spc) -> Optional[str]:
    """why the truncation look (ADP_FLAG_TRUNCATED) does not go with this configuration, or None (what the library refuses with
    ADP_ERR_UNSUPPORTED, said without a GPU)"""
    M = spc.mvs_polya
    W = int(M.median_shift_window)
    if not M.mvs_detect_check:
        return "it needs mvs_polya.mvs_detect_check (its tests are the MVS check's)"
    if M.mvs_detect_overwrite:
        return "it does not go with mvs_polya.mvs_detect_overwrite"
    if W > 4096:
        return "mvs_polya.median_shift_window is longer than 4096"
    if not (1 <= int(M.pA_var_window) <= W - 3 and 1 <= int(M.pA_mean_window) <= W - 3):
        return "mvs_polya.pA_mean_window and pA_var_window must lie in [1, median_shift_window - 3]"
    return None


def resegment_unsupported(spc, flag_truncated: bool = False) -> Optional[str]:
    """why the re-segmentation (ADP_LLR_RESEGMENT) does not go with this configuration, or None (what the library refuses with
    ADP_ERR_UNSUPPORTED, said without a GPU)"""
    if spc.primary_method != "llr":
        return "it belongs to the LLR primary (the configuration selects %s)" % spc.primary_method
    if flag_truncated:
        return "it does not go with the truncation look (which validates from start 0)"
    if spc.mvs_polya.mvs_detect_overwrite:
        return "it does not go with mvs_polya.mvs_detect_overwrite"
    return None


def second_resegment_unsupported(spc, flag_truncated: bool = False) -> Optional[str]:
    """why the re-segmentation behind the CNN primary's second opinion (ADP_CNN_SECOND_RESEGMENT) does not go with this
    configuration, or None (what the library refuses with ADP_ERR_UNSUPPORTED, said without a GPU)"""
    if spc.primary_method != "cnn":
        return "it belongs to the CNN primary's second opinion (the configuration selects %s)" % spc.primary_method
    if flag_truncated:
        return "it does not go with the truncation look (which validates from start 0)"
    if spc.mvs_polya.mvs_detect_overwrite:
        return "it does not go with mvs_polya.mvs_detect_overwrite"
    return None


def first_fail_text(code: int) -> str:
    """the fail_reason text of a first row's fail_code as a re-segmented row keeps it (the MVS check's names are not kept)"""
    return FAIL_REASONS[int(code)].rstrip(": ")


def resegmented_row_log(code: int) -> str:
    """the llr_detect_log of a row the re-segmentation made, by the fail_code of the row it replaced"""
    return "resegmented: first pass failed (%s)" % first_fail_text(code)


# the magnitudes below which Engine.format_csv's text is known to be pandas' (CSV_F64_BOUND, CSV_F32_BOUND of
# adapted_amd/csrc/csv_api.h; tests/test_native_csv_cpu.py holds them against that header and against pandas)
CSV_F64_BOUND = 2.0 ** 43
CSV_F32_BOUND = 2.0 ** 14
_CSV_STRINGS = None


def csv_string_table():
    """the texts adp_format_rows prints for a row's codes, packed (include/adapted_hip_csv.h: 69 entries) -> (uint8 bytes, int32
    offsets [70]).  They are stated here and nowhere else: FAIL_REASONS, START_PEAK_TYPES, resegmented_row_log, the MVS check's
    names as fail_reason_of joins them, and the two header lines from output.CSV_COLUMNS."""
    global _CSV_STRINGS
    if _CSV_STRINGS is None:
        from .output import CSV_COLUMNS

        texts = [FAIL_REASONS[c] or "" for c in range(16)] + [START_PEAK_TYPES[c] or "" for c in range(3)]
        texts += [resegmented_row_log(c) if FAIL_REASONS[c] else "" for c in range(16)]
        texts += [" ".join(n for b, n in enumerate(_MVS_NAMES) if mask >> b & 1) for mask in range(32)]
        assert not any(ch in name for name in CSV_COLUMNS for ch in ',"\r\n')  # (a header cell that would need quotes)
        texts += [",".join(CSV_COLUMNS) + "\n", ",".join(CSV_COLUMNS + ["fail_reason"]) + "\n"]
        raw = [t.encode() for t in texts]
        off = np.zeros(len(raw) + 1, dtype=np.int32)
        np.cumsum([len(b) for b in raw], out=off[1:])
        _CSV_STRINGS = (np.frombuffer(b"".join(raw), dtype=np.uint8), off)
    return _CSV_STRINGS


def rows_csv_text(rows: np.ndarray, read_ids, primary: str, fail: bool = False, consume: bool = False) -> bytes:
    """the text of one output file as the pandas writer makes it (output.save_detected_boundaries on rows_to_results of the rows):
    the specification of Engine.format_csv, and what it returns for a file with a value outside its bounds"""
    import io

    from .container_types import ReadResult
    from .output import save_detected_boundaries

    res = rows_to_results(rows, primary, consume=consume)
    buf = io.StringIO()
    save_detected_boundaries([ReadResult(read_id=str(rid), success=r.success, fail_reason=r.fail_reason, detect_results=r)
                              for rid, r in zip(read_ids, res)], buf, save_fail_reasons=fail)
    return buf.getvalue().encode()


def resegment_log(reserved: np.ndarray) -> str:
    """the log line of a run: how many rows the re-segmentation kept, by the first row's fail_reason (reserved: the rows' ``reserved_``)"""
    reserved = np.asarray(reserved, dtype=np.int64)
    kept = reserved[(reserved & ROW_RESEGMENTED) != 0]
    codes = (kept & ROW_FIRST_FAIL_MASK) >> ROW_FIRST_FAIL_SHIFT
    by = ", ".join("%s: %d" % (first_fail_text(c), int((codes == c).sum())) for c in np.unique(codes))
    return "LLR re-segmentation: %d reads kept%s" % (kept.size, " (first failure: %s)" % by if kept.size else "")


def rows_to_results(rows: np.ndarray, primary: str, consume: bool = False) -> List[DetectResults]:
    """adp_row[] -> DetectResults, value for value what the reference's validate_boundaries
    returns (types: python int / float, np.float32 where the reference keeps numpy scalars).
    consume: the rows are not needed again -- their overflow open_pores lists leave the registry (a long run converts
    every row exactly once: adapted_amd/main.py).
    A row made by the CNN path's LLR second opinion (``reserved_`` bit 0) is named as the LLR path names it, whatever ``primary``.
    ``polya_truncated`` (an extension: the reference never sets it): True for a row the truncation look replaced (bit 1; its six
    ``rna_preloaded_*`` fields are None), False for a passing row of a call that looked (bit 2), None otherwise.
    A row the re-segmentation made (bit 5) says so in ``llr_detect_log``, the reference's column for the LLR detector's messages:
    "resegmented: first pass failed (<the fail_reason text of the first row's code>)"; every other LLR row keeps ""."""
    out = []
    names_of = {primary: [c.format(primary=primary) for c in COLS]}
    if rows.size and (rows["reserved_"] & ROW_FROM_SECOND_LLR).any():
        names_of["llr"] = [c.format(primary="llr") for c in COLS]
    row_primary = primary
    for r in rows:
        primary = "llr" if int(r["reserved_"]) & ROW_FROM_SECOND_LLR else row_primary
        names = names_of[primary]
        fc = int(r["fail_code"])
        if 9 <= fc <= 14:  # the reference raised inside its per-read try block
            out.append(DetectResults(success=False, fail_reason=fail_reason_of(r)))
            continue
        d = DetectResults(success=bool(r["success"]))
        pres = int(r["present"])
        col = r["col"]
        for i, name in enumerate(names):
            if pres >> i & 1:
                v = col[i]
                if i in _INT_COLS:
                    v = int(v)
                elif i in _F32_COLS:
                    v = np.float32(v)
                else:
                    v = float(v)
                setattr(d, name, v)
        nc = int(r["n_cand"])
        if nc >= 0:
            d.polya_candidates = np.asarray(r["cand"][:nc], dtype=np.int64)
        no = int(r["n_open_pores"])
        if no >= 0:
            if no <= MAX_OPEN_PORES:
                d.open_pores = np.asarray(r["open_pores"][:no], dtype=np.int64)
            else:  # the whole list was fetched from the call's arena (Engine._attach_open_pores)
                more = (_OPEN_PORES_MORE.pop if consume else _OPEN_PORES_MORE.get)(int(r["open_pores_more"]), None)
                if more is None or more.size != no:
                    raise HipLibraryError("a row with %d open pores lost its overflow list (rows from a device buffer? fetch them "
                                          "through Engine.attach_open_pores)" % no)
                d.open_pores = more
        res = int(r["reserved_"])
        if res & ROW_POLYA_TRUNCATED:
            d.polya_truncated = True
            for name in _RNA_FIELDS:
                setattr(d, name, None)
        elif res & ROW_TRUNC_LOOKED and d.success:
            d.polya_truncated = False
        d.mvs_llr_polya_end_adjust_ignored = False
        d.mvs_llr_polya_end_to_early_stop = bool(int(r["mvs_fail_mask"]) >> 8 & 1)  # (mvs_detect_overwrite only)
        fr = fail_reason_of(r)
        spt = START_PEAK_TYPES[int(r["start_peak_type"])]
        d.start_peak_open_pore_type = spt
        if primary == "start_peak":
            if fr is not None and spt is not None:
                fr = fr + "+" + spt
        else:
            d.llr_detect_log = "" if primary == "llr" else None
            if res & ROW_RESEGMENTED:
                d.llr_detect_log = resegmented_row_log((res & ROW_FIRST_FAIL_MASK) >> ROW_FIRST_FAIL_SHIFT)
        d.fail_reason = fr
        out.append(d)
    return out


def open_pore_float_column(results: List[DetectResults]) -> List[DetectResults]:
    """The start-peak primary's results of ONE minibatch as the reference returns them: detect_rna_start_peak keeps `open_pore_idx`
    in a DataFrame column (adapted/detect/start_peak.py:86-116) and combined_detect_start_peak copies the cell (combined.py:337) --
    all None: every row keeps None; one flagged read in the minibatch: the column is float64, the flagged rows read back as
    floats, the others as NaN.  (The CSV text is the same either way.)  Pinned by tests/golden/rna004_start_peak_200k."""
    if any(r.start_peak_open_pore_idx is not None for r in results):
        for r in results:
            if r.signal_len is None and r.start_peak_idx is None:
                continue  # (a row that only carries a raised exception)
            r.start_peak_open_pore_idx = float(r.start_peak_open_pore_idx) if r.start_peak_open_pore_idx is not None else float("nan")
    return results


class Engine:
    """One GPU's detect engine: a handle of libadapted_hip.so sized for (max_reads, m).  The library's functions carry their
    prototypes (PROTOTYPES): ints, floats, device pointers and numpy arrays are passed as they are, and checked there."""

    def __init__(self, spc, max_reads: int, m: int, device: int = 0, single_read_layout: bool = False):
        """single_read_layout: the engine of combined_detect_llr (adapted/detect/combined.py:39-119): pooled from sample 0, every
        read its own minibatch (detect_llr_rows with minibatch = 1)"""
        self.lib = load()
        self.spc = spc
        self.cfg = make_cfg(spc)
        self.max_reads, self.m, self.device = int(max_reads), int(m), int(device)
        self._h = _VoidP()
        self._pinned = {}
        self._check(self.lib.adp_create(self.device, C.byref(self.cfg), self.max_reads, self.m, C.byref(self._h)))
        if single_read_layout:
            self._check(self.lib.adp_set_layout(self._h, 1))

    # -- plumbing ---------------------------------------------------------------------
    def _check(self, rc):
        if rc < 0:
            raise HipLibraryError("libadapted_hip: error %d: %s" % (rc, self.lib.adp_last_error().decode()))
        return rc

    def close(self):
        if self._h:
            self.lib.adp_destroy(self._h)
            self._h = _VoidP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, spc):
        self.spc = spc
        self.cfg = make_cfg(spc)
        self._check(self.lib.adp_set_config(self._h, C.byref(self.cfg)))

    @property
    def stream(self) -> int:
        return int(self.lib.adp_stream(self._h) or 0)

    def set_profiling(self, on: bool):
        self._check(self.lib.adp_set_profiling(self._h, int(on)))

    def kernel_times(self):
        cap = 4096  # (a grouped call reports every group's launches)
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        k = self._check(self.lib.adp_kernel_times(self._h, names, ms, cap))
        return [(names[i].decode(), float(ms[i])) for i in range(k)]

    # -- device memory ------------------------------------------------------------------
    def dev_alloc(self, nbytes: int) -> int:
        p = _VoidP()
        self._check(self.lib.adp_dev_alloc(self._h, nbytes, C.byref(p)))
        return int(p.value)

    def dev_free(self, ptr: int):
        self._check(self.lib.adp_dev_free(self._h, ptr))

    def calibrate_i16(self, raw_dev: int, len_dev: int, scale_dev: int, offset_dev: int, n: int, out_dev: int):
        """int16 ADC samples [n, m] + per-read (scale, offset) -> float32 [n, m] NaN-padded, on the device (asynchronous
        on the handle's stream: the detect call that follows is ordered behind it)"""
        self._check(self.lib.adp_calibrate_i16(self._h, raw_dev, len_dev, scale_dev, offset_dev, int(n), self.m, out_dev))

    def expand_ragged(self, packed_dev: int, is_int16: bool, offs_dev: int, len_dev: int, n: int, out_dev: int,
                      scale_dev: int = 0, offset_dev: int = 0):
        """reads packed back to back (float32 pA, or int16 ADC + per-read calibration) -> float32 [n, m] NaN-padded, on the
        device (asynchronous on the handle's stream)"""
        self._check(self.lib.adp_expand_ragged(self._h, packed_dev, bool(is_int16), offs_dev, len_dev, scale_dev or None,
                                               offset_dev or None, int(n), self.m, out_dev))

    def expand_ragged_i16(self, packed_dev: int, offs_dev: int, len_dev: int, n: int, out_dev: int):
        """packed raw int16 reads -> raw int16 [n, m] on the device (what detect_llr_rows_i16 reads); asynchronous"""
        self._check(self.lib.adp_expand_ragged_i16(self._h, packed_dev, offs_dev, len_dev, int(n), self.m, out_dev))

    def host_alloc(self, shape, dtype) -> np.ndarray:
        """page-locked host array (staging for h2d_async); release with host_free(arr)"""
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        p = _VoidP()
        self._check(self.lib.adp_host_alloc(self._h, max(1, n * dt.itemsize), C.byref(p)))
        buf = (C.c_char * (n * dt.itemsize)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dt).reshape(shape)
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr: np.ndarray):
        self._check(self.lib.adp_host_free(self._h, self._pinned.pop(arr.ctypes.data)))

    def h2d_async(self, dst: int, arr: np.ndarray, nbytes: Optional[int] = None):
        """copy from a PINNED host array on the handle's copy stream; copy_mark(slot) then copy_wait(slot) before use"""
        self._check(self.lib.adp_memcpy_h2d_async(self._h, dst, arr, arr.nbytes if nbytes is None else nbytes))

    def copy_mark(self, slot: int):
        self._check(self.lib.adp_copy_mark(self._h, int(slot)))

    def copy_wait(self, slot: int = -1):
        self._check(self.lib.adp_copy_wait(self._h, int(slot)))

    def h2d(self, dst: int, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        self._check(self.lib.adp_memcpy_h2d(self._h, dst, a, a.nbytes))

    def d2h(self, arr: np.ndarray, src: int):
        assert arr.flags.c_contiguous
        self._check(self.lib.adp_memcpy_d2h(self._h, arr, src, arr.nbytes))

    def synth_fill(self, dev_signals: int, dev_full_len: Optional[int], n: int, seed: int, first_read: int,
                   decorate: bool = True):
        self._check(self.lib.adp_synth_fill(self._h, dev_signals, dev_full_len or None, int(n), self.m, seed, first_read, int(decorate)))

    # -- operators ------------------------------------------------------------------------
    def attach_open_pores(self, rows: Optional[np.ndarray]):
        """rows (host) of the LAST call: reads with more open pores than a row holds get their whole list out of the
        call's arena (the offset in `open_pores_more` becomes a registry token)"""
        if rows is None or rows.size == 0:
            return rows
        big = np.flatnonzero(rows["n_open_pores"] > MAX_OPEN_PORES)
        if big.size:
            used = np.zeros(1, dtype=np.uint64)
            self._check(self.lib.adp_open_pores_arena(self._h, None, 0, used))
            arena = np.zeros(int(used[0]), dtype=np.int32)
            self._check(self.lib.adp_open_pores_arena(self._h, arena, arena.size, used))
            for i in big:
                off, no = int(rows[i]["open_pores_more"]), int(rows[i]["n_open_pores"])
                if off < 0 or off + no > arena.size:
                    raise HipLibraryError("open-pore arena inconsistent (offset %d, %d entries, %d in use)" % (off, no, arena.size))
                rows[i]["open_pores_more"] = register_open_pores(arena[off:off + no])
        return rows

    def _in(self, signals, full_lens, n, device_ptrs):
        """a detect call's minibatch -> (signals, full_lens, flags): device pointers, or float32 [n, m] and int32 [n] host arrays"""
        if device_ptrs:
            _check_runtime_once_torch_is_here()  # (device pointers come from torch: its runtime must be this library's)
            return int(signals), int(full_lens), ADP_IN_DEVICE
        sig = np.ascontiguousarray(signals, dtype=np.float32)
        lens = np.ascontiguousarray(full_lens, dtype=np.int32)
        if sig.ndim != 2 or sig.shape != (n, self.m) or lens.shape != (n,):
            raise ValueError("signals must be float32 [n, %d] and full_lens int32 [n]" % self.m)
        return sig, lens, 0

    @staticmethod
    def _out(dev, shape, dtype=ROW_DTYPE):
        """a call's main output -> (host array or None, what the call is given, flags): a zeroed host array, or the caller's
        device buffer ``dev`` with ADP_OUT_DEVICE"""
        if dev is not None:
            return None, dev, ADP_OUT_DEVICE
        out = np.zeros(shape, dtype=dtype)
        return out, out, 0

    def _detect_llr(self, fn, head, n, minibatch, flags, rows_dev):
        """adp_detect_llr / adp_detect_llr_i16 (fn) behind the batch's leading arguments (head)"""
        rows, rows_arg, out_flag = self._out(rows_dev, n)
        mbs = np.zeros((n + minibatch - 1) // minibatch, dtype=np.int32)
        self._check(fn(self._h, *head, n, self.m, minibatch, flags | out_flag, rows_arg, mbs))
        return self.attach_open_pores(rows), mbs

    def detect_llr_rows(self, signals, full_lens, n: int, minibatch: int, with_start_peak: bool = False,
                        device_ptrs: bool = False, rows_dev: Optional[int] = None, tails_nan: bool = False, flag_truncated: bool = False,
                        resegment: bool = False):
        """-> (rows ndarray[ROW_DTYPE] or None when rows_dev is given, mb_status int32[n_mb]).
        tails_nan: the caller guarantees that every row is NaN from min(full_len, m) on (the reference's own padding,
        adapted/file_proc.py:170-174); the streaming passes then skip the padding (ADP_TAILS_NAN).
        flag_truncated: the call ends with the truncation look (ADP_FLAG_TRUNCATED, an extension): a read whose poly(A) runs into
        the end of the preloaded window gets the row of the validation with (adapter end, window end) and polya_truncated
        (reserved_ bit 1); every row carries reserved_ bit 2.
        resegment: reads whose first row fails behind a first change point are segmented once more from their "poly(A) end" and
        validated from the first adapter end (ADP_LLR_RESEGMENT, an extension, untuned; include/adapted_hip_resegment.h): a
        validation that passes replaces the row (reserved_ bit 5, the first fail_code in bits 6-9)."""
        sig, lens, flags = self._in(signals, full_lens, n, device_ptrs)
        flags |= _flag_word(with_start_peak=with_start_peak, tails_nan=tails_nan, flag_truncated=flag_truncated, resegment=resegment)
        return self._detect_llr(self.lib.adp_detect_llr, (sig, lens), n, minibatch, flags, rows_dev)

    def detect_llr_rows_i16(self, raw_dev: int, len_dev: int, scale_dev: int, offset_dev: int, n: int, minibatch: int,
                            with_start_peak: bool = False, rows_dev: Optional[int] = None):
        """adp_detect_llr over RAW int16 samples resident on the device (per-read calibration applied in registers):
        -> (rows or None when rows_dev is given, mb_status)"""
        head = (int(raw_dev), int(len_dev), int(scale_dev), int(offset_dev))
        flags = ADP_IN_DEVICE | _flag_word(with_start_peak=with_start_peak)
        return self._detect_llr(self.lib.adp_detect_llr_i16, head, n, minibatch, flags, rows_dev)

    def detect_start_peak_rows(self, signals, full_lens, n: int, minibatch: int, device_ptrs: bool = False):
        """adp_detect_start_peak over n reads in ONE library call: the pandas float-column quirk couples the reads of a minibatch
        (the library walks the minibatches), the open-pore arena belongs to the call (offsets of every minibatch index it)"""
        sig, lens, flags = self._in(signals, full_lens, n, device_ptrs)
        rows = np.zeros(n, dtype=ROW_DTYPE)
        self._check(self.lib.adp_detect_start_peak(self._h, sig, lens, n, self.m, int(minibatch), flags, rows))
        return self.attach_open_pores(rows)

    def validate_rows(self, signals, full_lens, n: int, bounds: np.ndarray, device_ptrs: bool = False,
                      topk_none: bool = False, polya_truncated: bool = False):
        """bounds int64 [n, 1+k] (host) -> rows.  polya_truncated: Boundaries.polya_truncated is True for every read -- the RNA
        partition is all None (ADP_POLYA_TRUNCATED)"""
        sig, lens, flags = self._in(signals, full_lens, n, device_ptrs)
        if topk_none:
            flags |= ADP_TOPK_NONE
        if polya_truncated:
            flags |= ADP_POLYA_TRUNCATED
        b = np.ascontiguousarray(bounds, dtype=np.int64)
        rows = np.zeros(n, dtype=ROW_DTYPE)
        if device_ptrs:
            flags |= ADP_BOUNDS_HOST  # the signals are resident, the candidate table comes from the host
        self._check(self.lib.adp_validate_candidates(self._h, sig, lens, n, self.m, b, b.shape[1] - 1, flags, rows))
        return self.attach_open_pores(rows)

    def validate_rows_from(self, signals, full_lens, n: int, bounds: np.ndarray, starts, device_ptrs: bool = False,
                           topk_none: bool = False, polya_truncated: bool = False):
        """validate_rows with Boundaries.adapter_start = starts[r] (adp_validate_candidates_from): starts int64 [n] (host), or None
        for 0 everywhere -- the bytes of validate_rows"""
        sig, lens, flags = self._in(signals, full_lens, n, device_ptrs)
        if topk_none:
            flags |= ADP_TOPK_NONE
        if polya_truncated:
            flags |= ADP_POLYA_TRUNCATED
        b = np.ascontiguousarray(bounds, dtype=np.int64)
        st = None
        if starts is not None:
            st = np.ascontiguousarray(starts, dtype=np.int64)
            if st.shape != (n,):
                raise ValueError("starts: int64 [n]")
        rows = np.zeros(n, dtype=ROW_DTYPE)
        if device_ptrs:
            flags |= ADP_BOUNDS_HOST  # the signals are resident, the candidate table and the starts come from the host
        self._check(self.lib.adp_validate_candidates_from(self._h, sig, lens, n, self.m, b, st, b.shape[1] - 1, flags, rows))
        return self.attach_open_pores(rows)

    # -- the reference's modules (adp_c_llr_*, adp_llr_*, adp_mvs_*): one input path ----------------------------------------
    def _rows_in(self, x, n=None, L=None, dtypes=(np.float64,), convert=False, what="signals"):
        """a module call's [n, L] input: a device pointer (int) with n and L given, or a host C-contiguous array of one of
        ``dtypes`` (``convert``: made so, other dtypes widened to dtypes[0]) -> (the pointer or the array, flags, n, L)"""
        if isinstance(x, int):
            if n is None or L is None:
                raise ValueError("a device pointer needs n and L")
            _check_runtime_once_torch_is_here()  # (device pointers come from torch: its runtime must be this library's)
            return x, ADP_IN_DEVICE, int(n), int(L)
        a = np.asarray(x)
        if convert:
            a = np.ascontiguousarray(a, dtype=a.dtype if a.dtype in dtypes else dtypes[0])
        if a.dtype not in dtypes or not a.flags.c_contiguous or a.ndim != 2:
            raise ValueError("%s: a C-contiguous %s [n, L] array" % (what, " or ".join(np.dtype(d).name for d in dtypes)))
        return a, 0, a.shape[0], a.shape[1]

    def _sig_in(self, sig, n, L, f64):
        """signals float32 / float64 [n, L] (a device pointer: float64 with ``f64``) -> (the pointer or the array, flags with
        ADP_MVS_F64 for float64, n, L, dtype)"""
        sig, flags, n, L = self._rows_in(sig, n, L, (np.float32, np.float64))
        dt = np.dtype(np.float64 if f64 else np.float32) if isinstance(sig, int) else sig.dtype
        return sig, flags | (ADP_MVS_F64 if dt == np.float64 else 0), n, L, dt

    @staticmethod
    def _per_read(a, n, what, dtype=np.int32):
        """a per-read host array as the library takes it: C-contiguous ``dtype`` [n]"""
        a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        if a.size != n:
            raise ValueError("%s needs one entry per read" % what)
        return a

    def c_llr_trace(self, raw, lens, starts, ends, args: "AdpTraceArgs", sums=None, return_c_c2: bool = False):
        """adp_c_llr_trace: the reference's `c_llr_trace` (`c_llr_trace_gains` with ``sums=(c, c2)``) for a batch -- raw float64
        [n, L], per-read lens / starts / ends -> gains float64 [n, L] (and c, c2)"""
        flags = 0
        if sums is not None:
            c, c2 = (self._rows_in(s, convert=True, what="sums")[0] for s in sums)
            n, L = c.shape
            raw = None
            flags |= ADP_TRACE_FROM_SUMS
        else:
            raw, _, n, L = self._rows_in(raw, convert=True, what="raw signals")
            c, c2 = (np.zeros((n, L)), np.zeros((n, L))) if return_c_c2 else (None, None)
        lens, starts, ends = (self._per_read(a, n, w) for a, w in ((lens, "lens"), (starts, "starts"), (ends, "ends")))
        g = np.zeros((n, L))
        self._check(self.lib.adp_c_llr_trace(self._h, raw, lens, starts, ends, n, L, C.byref(args), flags, g, c, c2))
        return (g, c, c2) if return_c_c2 else g

    def c_llr_best_split(self, c, c2, lens, starts, ends, offset_heads, offset_tails):
        """adp_c_llr_best_split: the reference's `_best_split` for a batch -- sums float64 [n, L], per-row lens / starts / ends /
        offsets -> (x int64 [n], gain float64 [n])"""
        c, c2 = (self._rows_in(s, convert=True, what="sums")[0] for s in (c, c2))
        n, L = c.shape
        if c2.shape != c.shape:
            raise ValueError("c, c2 [n, L] and one entry per row of lens / starts / ends / offsets")
        arrs = [self._per_read(a, n, w) for a, w in ((lens, "lens"), (starts, "starts"), (ends, "ends"), (offset_heads, "offset_heads"),
                                                     (offset_tails, "offset_tails"))]
        x = np.zeros(n, dtype=np.int64)
        g = np.zeros(n)
        self._check(self.lib.adp_c_llr_best_split(self._h, c, c2, *arrs, n, L, 0, x, g))
        return x, g

    def c_llr_detect(self, raw, lens, min_obs_adapter: int, border_trim: int, min_obs_polya: int = 0, polya: bool = False,
                     n: Optional[int] = None, L: Optional[int] = None, float32: bool = False, details: bool = False):
        """adp_c_llr_detect: `c_llr_detect_adapter` / `c_llr_detect_adapter_polya` for a batch.  raw: float64 or float32 [n, L]
        host array, or a device pointer (int) with n, L and ``float32`` given.  -> rows int64 [n, 4] (adapter_start, adapter_end,
        polya_end, tuple length 2 or 3); with ``details`` also (splits int64 [n, 4], stats float64 [n, 8])"""
        raw, flags, n, L = self._rows_in(raw, n, L, (np.float64, np.float32), convert=True, what="raw signals")
        if float32 if isinstance(raw, int) else raw.dtype == np.float32:
            flags |= ADP_CLLR_F32
        if polya:
            flags |= ADP_CLLR_POLYA
        lens = self._per_read(lens, n, "lens")
        rows = np.zeros((n, 4), dtype=np.int64)
        splits = np.zeros((n, 4), dtype=np.int64) if details else None
        stats = np.zeros((n, 8)) if details else None
        self._check(self.lib.adp_c_llr_detect(self._h, raw, lens, n, L, int(min_obs_adapter), int(border_trim), int(min_obs_polya),
                                              flags, rows, splits, stats))
        return (rows, splits, stats) if details else rows

    def llr_trace_bounds(self, trace, lens, min_obs, tail_trim, stride: int, interp: bool, n: Optional[int] = None, L: Optional[int] = None):
        """adp_llr_trace_bounds: LLRTrace's start / end / early_stop, and with ``interp`` interp_stride IN PLACE (trace: a writable
        host float64 [n, L] array, or a device pointer with n, L) -> (start, end, early_stop) int32 [n] (early_stop bit 1: the
        knot set was empty)"""
        trace, flags, n, L = self._rows_in(trace, n, L, what="traces")
        ins = [self._per_read(a, n, w) for a, w in ((lens, "lens"), (min_obs, "min_obs"), (tail_trim, "tail_trim"))]
        outs = [np.zeros(n, dtype=np.int32) for _ in range(3)]
        if interp:
            flags |= ADP_LLR_INTERP
        self._check(self.lib.adp_llr_trace_bounds(self._h, trace, *ins, int(stride), n, L, flags, *outs))
        return tuple(outs)

    def llr_trace_peaks(self, trace, lens, clip_lo, clip_hi, args: "AdpPeakArgs", cap: int = 16, n: Optional[int] = None,
                        L: Optional[int] = None, given_peak: bool = False):
        """adp_llr_trace_peaks -> (peaks int64 [n, cap] padded with -1, counts int64 [n]: the true counts, also past cap).
        ``given_peak``: clip_lo holds one peak per read, only corrected (ADP_LLR_GIVEN_PEAK)"""
        trace, flags, n, L = self._rows_in(trace, n, L, what="traces")
        if given_peak:
            flags |= ADP_LLR_GIVEN_PEAK
        ins = [self._per_read(a, n, w) for a, w in ((lens, "lens"), (clip_lo, "clip_lo"), (clip_hi, "clip_hi"))]
        pk = np.zeros((n, int(cap)), dtype=np.int64)
        cnt = np.zeros(n, dtype=np.int64)
        self._check(self.lib.adp_llr_trace_peaks(self._h, trace, *ins, n, L, C.byref(args), flags, int(cap), pk, cnt))
        return pk, cnt

    def llr_spike_peak(self, trace, lens, args: "AdpSpikeArgs", n: Optional[int] = None, L: Optional[int] = None):
        """adp_llr_spike_peak -> int64 [n]"""
        trace, flags, n, L = self._rows_in(trace, n, L, what="traces")
        lens = self._per_read(lens, n, "lens")
        out = np.zeros(n, dtype=np.int64)
        self._check(self.lib.adp_llr_spike_peak(self._h, trace, lens, n, L, C.byref(args), flags, out))
        return out

    def _mvs_call(self, fn, sig, lens, positions, args, n, L, f64, outs):
        """adp_mvs_*: signals float32 / float64 [n, L] (a device pointer: float64 with ``f64``), lens, the int64 positions, then
        the outputs ``outs(n)`` -> those outputs"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        ins = [self._per_read(lens, n, "lens")] + [self._per_read(v, n, w, np.int64) for v, w in positions]
        res = outs(n)
        self._check(fn(self._h, sig, *ins, n, L, C.byref(args), flags, *res))
        return res

    def mvs_check(self, sig, lens, adapter_ends, polya_ends, args: "AdpMvsArgs", n: Optional[int] = None, L: Optional[int] = None,
                  f64: bool = False):
        """adp_mvs_check -> (info int32 [n, 8], vals float64 [n, 5])"""
        return self._mvs_call(self.lib.adp_mvs_check, sig, lens, ((adapter_ends, "adapter_ends"), (polya_ends, "polya_ends")), args, n, L,
                              f64, lambda n: (np.zeros((n, 8), dtype=np.int32), np.zeros((n, 5))))

    def mvs_detect_at_loc(self, sig, lens, locs, args: "AdpMvsArgs", n: Optional[int] = None, L: Optional[int] = None, f64: bool = False):
        """adp_mvs_detect_at_loc -> (info int32 [n, 8], idx int64 [n], vals float64 [n, 5])"""
        return self._mvs_call(self.lib.adp_mvs_detect_at_loc, sig, lens, ((locs, "locs"),), args, n, L, f64,
                              lambda n: (np.zeros((n, 8), dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros((n, 5))))

    def mvs_detect(self, sig, lens, args: "AdpMvsArgs", n: Optional[int] = None, L: Optional[int] = None, f64: bool = False):
        """adp_mvs_detect -> int64 [n] (0: no poly(A) found)"""
        return self._mvs_call(self.lib.adp_mvs_detect, sig, lens, (), args, n, L, f64, lambda n: (np.zeros(n, dtype=np.int64),))[0]

    def _segs(self, rows, starts, ends):
        """struct adp_seg [n_seg] of per-segment rows, starts and ends"""
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        segs = np.zeros(rows.size, dtype=SEG_DTYPE)
        segs["row"] = rows
        segs["start"] = self._per_read(starts, rows.size, "starts", np.int64)
        segs["end"] = self._per_read(ends, rows.size, "ends", np.int64)
        return segs

    def seg_stats(self, sig, lens, rows, starts, ends, n: Optional[int] = None, L: Optional[int] = None, f64: bool = False):
        """adp_seg_stats: signals float32 / float64 [n, L] (a device pointer: float64 with ``f64``), lens, and per segment its
        row, start and end -> (stats float64 [n_seg, 4]: mean, std, median, MAD; counts int64 [n_seg]: the clipped sizes)"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        lens, segs = self._per_read(lens, n, "lens"), self._segs(rows, starts, ends)
        stats = np.zeros((segs.size, 4))
        cnt = np.zeros(segs.size, dtype=np.int64)
        self._check(self.lib.adp_seg_stats(self._h, sig, lens, n, L, segs, segs.size, flags, stats, cnt))
        return stats, cnt

    @staticmethod
    def _ss_flags(with_nan, whole, regime):
        return ((ADP_SS_NANSKIP if with_nan else 0) | (ADP_SS_WHOLE if whole else 0)
                | {None: 0, "grid": ADP_SS_FORCE_GRID, "wave": ADP_SS_FORCE_WAVE}[regime])

    def med_mad(self, sig, lens=None, with_nan: bool = False, whole: bool = False, n: Optional[int] = None, L: Optional[int] = None,
                f64: bool = False, regime: Optional[str] = None):
        """adp_med_mad -> float64 [n, 2] (median, MAD of every row's [0, lens[r])), or with ``whole`` [1, 2] of the whole array as
        one population.  ``regime``: "grid" / "wave" force the many-workgroup / the one-workgroup selection of a whole population"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        flags |= self._ss_flags(with_nan, whole, regime)
        lens = None if whole else self._per_read(lens, n, "lens")
        out = np.zeros((1 if whole else n, 2))
        self._check(self.lib.adp_med_mad(self._h, sig, lens, n, L, flags, out))
        return out

    def normalize(self, sig, lens=None, outlier_thresh: float = 5.0, with_nan: bool = False, whole: bool = False, clip_medmad=None,
                  n: Optional[int] = None, L: Optional[int] = None, f64: bool = False, out_ptr: Optional[int] = None,
                  regime: Optional[str] = None):
        """adp_normalize -> (out [n, L] of the input's type (None with ``out_ptr``, a device pointer the rows are written to),
        medmad float64 [n, 2] or [1, 2], status int32 [n] or [1]: 1 where the MAD is 0).  ``clip_medmad``: the clip alone, about
        the given (median, MAD) rows"""
        sig, flags, n, L, dt = self._sig_in(sig, n, L, f64)
        flags |= self._ss_flags(with_nan, whole, regime)
        rows = 1 if whole else n
        lens = None if whole else self._per_read(lens, n, "lens")
        if clip_medmad is not None:
            flags |= ADP_SS_CLIP
            mm = np.ascontiguousarray(clip_medmad, dtype=np.float64).reshape(-1, 2)
            if mm.shape[0] != rows:
                raise ValueError("clip_medmad needs one (median, MAD) per row, or one with whole")
        else:
            mm = np.zeros((rows, 2))
        status = np.zeros(rows, dtype=np.int32)
        out, out_arg, out_flag = self._out(out_ptr, (n, L), dt)
        self._check(self.lib.adp_normalize(self._h, sig, lens, n, L, outlier_thresh, flags | out_flag, mm, out_arg, status))
        return out, mm, status

    def pool_mean(self, data, pool_size: int, n: Optional[int] = None, L: Optional[int] = None, f64: bool = False,
                  out_ptr: Optional[int] = None):
        """adp_pool_mean: data [n, L] -> [n, ceil(L / pool_size)] of the input's type (None with ``out_ptr``)"""
        data, flags, n, L, dt = self._sig_in(data, n, L, f64)
        out, out_arg, out_flag = self._out(out_ptr, (n, -(-L // int(pool_size))), dt)
        self._check(self.lib.adp_pool_mean(self._h, data, n, L, int(pool_size), flags | out_flag, out_arg))
        return out

    def real_range(self, sig, lens, rows, starts, ends, args: "AdpRealRangeArgs", n: Optional[int] = None, L: Optional[int] = None,
                   f64: bool = False):
        """adp_real_range -> (info int32 [n_seg, 2]: result, stage; vals float64 [n_seg, 3]: mean_start, mean_end, local range)"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        lens, segs = self._per_read(lens, n, "lens"), self._segs(rows, starts, ends)
        info = np.zeros((segs.size, 2), dtype=np.int32)
        vals = np.zeros((segs.size, 3))
        self._check(self.lib.adp_real_range(self._h, sig, lens, n, L, segs, segs.size, C.byref(args), flags, info, vals))
        return info, vals

    def open_pores(self, sig, lens, rows, starts, ends, lo: float, hi: float, min_obs_diff: float, cap: int = 16,
                   n: Optional[int] = None, L: Optional[int] = None, f64: bool = False):
        """adp_open_pores -> (pos int64 [n_seg, cap'] padded with -1, counts int64 [n_seg, 3]: kept, in range, the last in range).
        cap' >= cap: the call is repeated with the largest count when a list did not fit, so no list is cut short"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        lens, segs = self._per_read(lens, n, "lens"), self._segs(rows, starts, ends)
        cnt = np.zeros((segs.size, 3), dtype=np.int64)
        cap = max(int(cap), 1)
        while True:
            pos = np.zeros((segs.size, cap), dtype=np.int64)
            self._check(self.lib.adp_open_pores(self._h, sig, lens, n, L, segs, segs.size, lo, hi, min_obs_diff, flags, cap, pos, cnt))
            if cnt[:, 0].max() <= cap:
                return pos, cnt
            cap = int(cnt[:, 0].max())

    def start_peak(self, sig, full_lens, args: "AdpStartPeakArgs", n: Optional[int] = None, m: Optional[int] = None, f64: bool = False):
        """adp_start_peak: signals float32 / float64 [n, m] (a device pointer: float64 with ``f64``), the full lengths (they may
        exceed m) -> (info int32 [n, 5]: valid, start_peak_idx, next_greater_idx, open_pore_idx or -1, flagged type -- pooled
        indices; vals float64 [n, 2]: start_peak_pa, next_greater_pa)"""
        sig, flags, n, m, _ = self._sig_in(sig, n, m, f64)
        info, vals = np.zeros((n, 5), dtype=np.int32), np.zeros((n, 2))
        self._check(self.lib.adp_start_peak(self._h, sig, self._per_read(full_lens, n, "full_signal_lens"), n, m, C.byref(args), flags,
                                            info, vals))
        return info, vals

    def adapter_start(self, sig, lens, args: "AdpAdapterStartArgs", n: Optional[int] = None, L: Optional[int] = None, f64: bool = False):
        """adp_adapter_start -> (info int32 [n, 4]: status, the exception's window and slice size, accepted; adapter_start int64
        [n]; cand int64 [n]; difference[cand] float64 [n])"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        info = np.zeros((n, 4), dtype=np.int32)
        out, cand, diff = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
        self._check(self.lib.adp_adapter_start(self._h, sig, self._per_read(lens, n, "lens"), n, L, C.byref(args), flags, info, out,
                                               cand, diff))
        return info, out, cand, diff

    def _adapter_front(self, fn, head, rows, args, n, m):
        """adp_adapter_front / adp_adapter_front_i16 (fn) behind the batch's leading arguments (head); rows: a host ROW_DTYPE array
        [n], patched in place, or a device pointer (ADP_OUT_DEVICE) -> (info int32 [n, 4], shift, cand int64 [n], diff float64 [n])"""
        flags = ADP_IN_DEVICE if isinstance(head[0], int) else 0  # (the signals: a device pointer, or a host array)
        if isinstance(rows, int):
            flags |= ADP_OUT_DEVICE
        elif not (isinstance(rows, np.ndarray) and rows.dtype == ROW_DTYPE and rows.flags.c_contiguous and rows.flags.writeable
                  and rows.shape == (n,)):
            raise ValueError("rows: a writable C-contiguous ROW_DTYPE array with one row per read, or a device pointer")
        info = np.zeros((n, 4), dtype=np.int32)
        shift, cand, diff = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
        self._check(fn(self._h, *head, n, int(m), rows, C.byref(args), flags, info, shift, cand, diff))
        return info, shift, cand, diff

    def adapter_front(self, sig, full_lens, rows, args: "AdpAdapterFrontArgs", n: Optional[int] = None, m: Optional[int] = None):
        """adp_adapter_front: the adapter-front post-pass over the rows of a detect call on ``sig``, the float32 [n, m] minibatch
        that call took (a host array, or a device pointer with ``n``; ``m``: the engine's unless given).  full_lens is not read
        (None will do).  rows: see _adapter_front -> (info, shift, cand, diff)"""
        sig, _, n, m = self._rows_in(sig, n, self.m if m is None else m, (np.float32,), what="signals")
        return self._adapter_front(self.lib.adp_adapter_front, (sig, None), rows, args, n, m)

    def adapter_front_i16(self, raw_dev: int, len_dev: int, scale_dev: int, offset_dev: int, rows, args: "AdpAdapterFrontArgs", n: int,
                          m: Optional[int] = None):
        """adp_adapter_front_i16: the same over RAW int16 samples resident on the device with their per-read calibration, as
        detect_llr_rows_i16 takes them (device pointers only; m a multiple of 4)"""
        _check_runtime_once_torch_is_here()
        head = (int(raw_dev), int(len_dev), int(scale_dev), int(offset_dev))
        return self._adapter_front(self.lib.adp_adapter_front_i16, head, rows, args, int(n), self.m if m is None else int(m))

    def _adapter_front_revalidate(self, fn, head, rows, args, n, m):
        """adp_adapter_front_revalidate / _i16 (fn) behind the batch's leading arguments (head); rows: a host ROW_DTYPE array [n]
        -> (info, shift, cand, diff, reval int32 [n, 2]).  The REPLACED rows alone get their whole open-pore lists out of this
        call's arena, and their old lists leave the registry: every other row's open_pores_more is a registry token already."""
        flags = ADP_IN_DEVICE if isinstance(head[0], int) else 0
        if not (isinstance(rows, np.ndarray) and rows.dtype == ROW_DTYPE and rows.flags.c_contiguous and rows.flags.writeable
                and rows.shape == (n,)):
            raise ValueError("rows: a writable C-contiguous ROW_DTYPE array with one row per read (host rows only)")
        info, reval = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
        shift, cand, diff = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
        n_before, token_before = rows["n_open_pores"].copy(), rows["open_pores_more"].copy()
        self._check(fn(self._h, *head, n, int(m), rows, C.byref(args), flags, info, shift, cand, diff, reval))
        replaced = np.flatnonzero(reval[:, 0] == 1)
        for i in replaced[n_before[replaced] > MAX_OPEN_PORES]:
            _OPEN_PORES_MORE.pop(int(token_before[i]), None)
        big = replaced[rows["n_open_pores"][replaced] > MAX_OPEN_PORES]
        if big.size:
            sub = rows[big]  # (a copy: attach_open_pores swaps offsets for tokens in it)
            rows[big] = self.attach_open_pores(sub)
        return info, shift, cand, diff, reval

    def adapter_front_revalidate(self, sig, full_lens, rows, args: "AdpAdapterFrontArgs", n: Optional[int] = None,
                                 m: Optional[int] = None):
        """adp_adapter_front_revalidate: adapter_front whose accepted reads are validated again from the trimmed start; a read whose
        validation fails keeps its row (the trim is rejected).  full_lens IS read: int32 [n] on the host beside host signals, a
        device pointer beside a device pointer -> (info, shift, cand, diff, reval)"""
        sig, _, n, m = self._rows_in(sig, n, self.m if m is None else m, (np.float32,), what="signals")
        lens = int(full_lens) if isinstance(sig, int) else np.ascontiguousarray(full_lens, dtype=np.int32)
        if not isinstance(lens, int) and lens.shape != (n,):
            raise ValueError("full_lens must be int32 [n]")
        return self._adapter_front_revalidate(self.lib.adp_adapter_front_revalidate, (sig, lens), rows, args, n, m)

    def adapter_front_revalidate_i16(self, raw_dev: int, len_dev: int, scale_dev: int, offset_dev: int, rows,
                                     args: "AdpAdapterFrontArgs", n: int, m: Optional[int] = None):
        """adp_adapter_front_revalidate_i16: the same over RAW int16 samples resident on the device (device pointers only)"""
        _check_runtime_once_torch_is_here()
        head = (int(raw_dev), int(len_dev), int(scale_dev), int(offset_dev))
        return self._adapter_front_revalidate(self.lib.adp_adapter_front_revalidate_i16, head, rows, args, int(n),
                                              self.m if m is None else int(m))

    def segment_events(self, sig, lens, rows, starts, ends, args: "AdpEventArgs", cap: int = 0, n: Optional[int] = None,
                       L: Optional[int] = None, f64: bool = False):
        """adp_segment_events: signals float32 / float64 [n, L] (a device pointer: float64 with ``f64``), lens, and per segment its
        row, start and end -> (pos int64 [n_seg, cap]: the boundaries between the events, from the clipped segment's start,
        padded with -1; info int64 [n_seg, 2]: the number of boundaries (also past cap), status (0; 1 a NaN in the slice; 2 the
        slice is shorter than two windows); stats float64 [n_seg, 2]: median and MAD of the gaps between boundaries)"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        lens, segs = self._per_read(lens, n, "lens"), self._segs(rows, starts, ends)
        cap = int(cap)
        if segs.size == 0:  # (the library wants a segment: an empty batch has an empty answer)
            return np.zeros((0, cap), dtype=np.int64), np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2))
        pos = np.zeros((segs.size, cap), dtype=np.int64)
        info = np.zeros((segs.size, 2), dtype=np.int64)
        stats = np.zeros((segs.size, 2))
        self._check(self.lib.adp_segment_events(self._h, sig, lens, n, L, segs, segs.size, C.byref(args), flags, cap,
                                                pos if cap > 0 else None, info, stats))
        return pos, info, stats

    def event_levels(self, sig, lens, rows, starts, ends, args: "AdpEventArgs", max_events: int, n: Optional[int] = None,
                     L: Optional[int] = None, f64: bool = False, fp_ptr: Optional[int] = None, count_ptr: Optional[int] = None):
        """adp_event_levels: the inputs of segment_events -> a dict: info int64 [n_seg, 2] and stats float64 [n_seg, 2] as
        segment_events'; count int32 [n_seg]; status int32 [n_seg] (0; 1 / 2 as the segmentation's; 4: the MAD of the levels is 0,
        or median / MAD are not finite); lengths int32 / levels float64 / fingerprints float64 [n_seg, max_events] (0 / NaN at and
        beyond count); norm float64 [n_seg, 2]: median and MAD of the levels.  With ``fp_ptr`` and ``count_ptr`` (device buffers
        of n_seg * max_events * 8 and n_seg * 4 bytes, dev_alloc) the fingerprints and counts stay on the device for dtw_assign and
        are None here"""
        sig, flags, n, L, _ = self._sig_in(sig, n, L, f64)
        lens, segs = self._per_read(lens, n, "lens"), self._segs(rows, starts, ends)
        E, ns = int(max_events), segs.size
        if (fp_ptr is None) != (count_ptr is None):
            raise ValueError("fp_ptr and count_ptr go together")
        on_dev = fp_ptr is not None
        out = {"info": np.zeros((ns, 2), dtype=np.int64), "stats": np.zeros((ns, 2)), "count": None if on_dev else np.zeros(ns, dtype=np.int32),
               "status": np.zeros(ns, dtype=np.int32), "lengths": np.zeros((ns, max(E, 0)), dtype=np.int32), "levels": np.zeros((ns, max(E, 0))),
               "fingerprints": None if on_dev else np.zeros((ns, max(E, 0))), "norm": np.zeros((ns, 2))}
        if ns == 0:  # (the library wants a segment: an empty batch has an empty answer)
            return out
        self._check(self.lib.adp_event_levels(self._h, sig, lens, n, L, segs, ns, C.byref(args), flags | (ADP_OUT_DEVICE if on_dev else 0), E,
                                              out["info"], out["stats"], int(count_ptr) if on_dev else out["count"], out["status"],
                                              out["lengths"], out["levels"], int(fp_ptr) if on_dev else out["fingerprints"], out["norm"]))
        return out

    def _packed_in(self, packed, offsets, scale, offset):
        """the packed calls' input: segment g is packed[offsets[g]:offsets[g + 1]] -- a host float32 or int16 array, or a device
        pointer (int16 when ``scale`` is given); offsets int64 [n_seg + 1] on the host; with int16 samples scale / offset float32
        [n_seg], host arrays beside a host array, device pointers beside a device pointer -> (packed, offsets, scale, offset, n_seg,
        flags)"""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.size < 1:
            raise ValueError("offsets: int64 [n_seg + 1]")
        ns = offsets.size - 1
        if (scale is None) != (offset is None):
            raise ValueError("scale and offset go together")
        if isinstance(packed, int):
            _check_runtime_once_torch_is_here()
            if scale is not None and not (isinstance(scale, int) and isinstance(offset, int)):
                raise ValueError("a device pointer to int16 samples needs device pointers to scale and offset")
            return packed, offsets, scale, offset, ns, ADP_IN_DEVICE | (ADP_PACKED_I16 if scale is not None else 0)
        a = np.asarray(packed)
        if a.dtype not in (np.float32, np.int16) or not a.flags.c_contiguous or a.ndim != 1:
            raise ValueError("packed: a C-contiguous float32 or int16 [samples] array")
        if ns and (offsets[0] < 0 or offsets[-1] > a.size or (np.diff(offsets) < 0).any()):
            raise ValueError("offsets must lie in [0, packed.size] and must not decrease")
        if a.dtype == np.int16:
            if scale is None:
                raise ValueError("int16 samples need a scale and an offset per segment")
            return (a if a.size else np.zeros(1, dtype=np.int16), offsets, self._per_read(scale, ns, "scale", np.float32),
                    self._per_read(offset, ns, "offset", np.float32), ns, ADP_PACKED_I16)
        return a if a.size else np.zeros(1, dtype=np.float32), offsets, None, None, ns, 0

    def segment_events_packed(self, packed, offsets, args: "AdpEventArgs", cap: int = 0, scale=None, offset=None):
        """adp_segment_events_packed: segment_events of the segments packed[offsets[g]:offsets[g + 1]] -- float32 pA, or raw int16
        samples with ``scale`` / ``offset`` float32 [n_seg] (pA = scale * (float32(adc) + offset), calibrate_i16's bits); a host
        array or a device pointer (_packed_in) -> segment_events' (pos, info, stats)"""
        packed, offsets, scale, offset, ns, flags = self._packed_in(packed, offsets, scale, offset)
        cap = int(cap)
        if ns == 0:  # (the library wants a segment: an empty batch has an empty answer)
            return np.zeros((0, cap), dtype=np.int64), np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2))
        pos = np.zeros((ns, cap), dtype=np.int64)
        info = np.zeros((ns, 2), dtype=np.int64)
        stats = np.zeros((ns, 2))
        self._check(self.lib.adp_segment_events_packed(self._h, packed, offsets, scale, offset, ns, C.byref(args), flags, cap,
                                                       pos if cap > 0 else None, info, stats))
        return pos, info, stats

    def event_levels_packed(self, packed, offsets, args: "AdpEventArgs", max_events: int, scale=None, offset=None,
                            fp_ptr: Optional[int] = None, count_ptr: Optional[int] = None):
        """adp_event_levels_packed: event_levels of the segments segment_events_packed takes -> event_levels' dict; ``fp_ptr`` and
        ``count_ptr`` as there"""
        packed, offsets, scale, offset, ns, flags = self._packed_in(packed, offsets, scale, offset)
        E = int(max_events)
        if (fp_ptr is None) != (count_ptr is None):
            raise ValueError("fp_ptr and count_ptr go together")
        on_dev = fp_ptr is not None
        out = {"info": np.zeros((ns, 2), dtype=np.int64), "stats": np.zeros((ns, 2)), "count": None if on_dev else np.zeros(ns, dtype=np.int32),
               "status": np.zeros(ns, dtype=np.int32), "lengths": np.zeros((ns, max(E, 0)), dtype=np.int32), "levels": np.zeros((ns, max(E, 0))),
               "fingerprints": None if on_dev else np.zeros((ns, max(E, 0))), "norm": np.zeros((ns, 2))}
        if ns == 0:  # (the library wants a segment: an empty batch has an empty answer)
            return out
        self._check(self.lib.adp_event_levels_packed(self._h, packed, offsets, scale, offset, ns, C.byref(args),
                                                     flags | (ADP_OUT_DEVICE if on_dev else 0), E, out["info"], out["stats"],
                                                     int(count_ptr) if on_dev else out["count"], out["status"], out["lengths"],
                                                     out["levels"], int(fp_ptr) if on_dev else out["fingerprints"], out["norm"]))
        return out

    def _fp_rows(self, q, q_count, n, E, noun: str, sizes: str, shape: Optional[str] = None):
        """fingerprint rows with their counts: a float64 [n, E] host array and a count per row, or two device pointers with ``n``
        and ``E`` (the refusals call those arguments ``sizes`` and the array's shape ``shape``) -> (q, q_count, n, E, flags)"""
        if isinstance(q, int):
            if n is None or E is None or not isinstance(q_count, int):
                raise ValueError("device %s need a device pointer to their counts, %s" % (noun, sizes))
            _check_runtime_once_torch_is_here()
            return q, q_count, int(n), int(E), ADP_IN_DEVICE
        q = np.ascontiguousarray(q, dtype=np.float64)
        if q.ndim != 2:
            raise ValueError("%s: a float64 [%s] array" % (noun, shape or sizes.replace(" and ", ", ")))
        n, E = q.shape
        return q, self._per_read(q_count, n, "q_count"), n, E, 0

    def _fp_table(self, t, t_count, noun: str, sizes: str, count_name: str):
        """a host table with its counts: float64 [rows, E] and a count per row -> (t, t_count, rows, E)"""
        t = np.ascontiguousarray(t, dtype=np.float64)
        if t.ndim != 2:
            raise ValueError("%s: a float64 [%s] array" % (noun, sizes))
        return t, self._per_read(t_count, t.shape[0], count_name), t.shape[0], t.shape[1]

    def dtw_assign(self, q, q_count, t, t_count, band: int = 0, nq: Optional[int] = None, Eq: Optional[int] = None,
                   want_dist: bool = True):
        """adp_dtw_assign: queries float64 [nq, Eq] with their counts (host arrays, or two device pointers with ``nq`` and ``Eq``:
        event_levels' fp_ptr and count_ptr), templates float64 [nt, Et] with their counts (host) -> (dist float64 [nq, nt], or
        None without ``want_dist``; best int32 [nq, 2]: the nearest and the second nearest template, -1 where there is none;
        bestdist float64 [nq, 2], NaN where -1)"""
        t, t_count, nt, Et = self._fp_table(t, t_count, "templates", "nt, Et", "t_count")
        q, q_count, nq, Eq, flags = self._fp_rows(q, q_count, nq, Eq, "queries", "nq and Eq")
        dist = np.zeros((nq, nt)) if want_dist else None
        best = np.full((nq, 2), -1, dtype=np.int32)
        bestdist = np.full((nq, 2), np.nan)
        if nq == 0:  # (the library wants a query: an empty batch has an empty answer)
            return dist, best, bestdist
        self._check(self.lib.adp_dtw_assign(self._h, q, q_count, nq, Eq, t, t_count, nt, Et, int(band), flags, dist, best, bestdist))
        return dist, best, bestdist

    def _align_in(self, q, q_count, which, t, t_count, nq, Eq):
        """the inputs adp_dtw_align and adp_dba_step share: dtw_assign's and ``which`` -> (q, q_count, which, nq, Eq, t, t_count, nt,
        Et, flags)"""
        t, t_count, nt, Et = self._fp_table(t, t_count, "templates", "nt, Et", "t_count")
        q, q_count, nq, Eq, flags = self._fp_rows(q, q_count, nq, Eq, "queries", "nq and Eq")
        return q, q_count, self._per_read(which, nq, "which"), nq, Eq, t, t_count, nt, Et, flags

    def dtw_align(self, q, q_count, which, t, t_count, band: int = 0, nq: Optional[int] = None, Eq: Optional[int] = None,
                  want_path: bool = True):
        """adp_dtw_align: queries and templates as dtw_assign takes them, which int32 [nq] (host): every query's template, -1 to
        skip it -> a dict: dist float64 [nq]; status int32 [nq] (0; 1 a count outside [1, Eq] or a value that is not finite; 2 a
        distance that is not finite; 3 skipped); with ``want_path`` lo, hi int32 [nq, Et] (the first and the last query index of
        every template position, -1 where there is none) and sum float64 [nq, Et] (the query summed over that run), else None"""
        q, q_count, which, nq, Eq, t, t_count, nt, Et, flags = self._align_in(q, q_count, which, t, t_count, nq, Eq)
        out = {"dist": np.full(nq, np.nan), "status": np.full(nq, 3, dtype=np.int32),
               "lo": np.full((nq, Et), -1, dtype=np.int32) if want_path else None,
               "hi": np.full((nq, Et), -1, dtype=np.int32) if want_path else None, "sum": np.full((nq, Et), np.nan) if want_path else None}
        if nq == 0:  # (the library wants a query: an empty batch has an empty answer)
            return out
        self._check(self.lib.adp_dtw_align(self._h, q, q_count, which, nq, Eq, t, t_count, nt, Et, int(band), flags, out["dist"],
                                           out["status"], out["lo"], out["hi"], out["sum"]))
        return out

    def dba_step(self, q, q_count, which, t, t_count, band: int = 0, nq: Optional[int] = None, Eq: Optional[int] = None,
                 want_dist: bool = False):
        """adp_dba_step: one iteration of DTW barycentre averaging over dtw_align's inputs (the queries may stay on the device
        over the iterations: two device pointers with ``nq`` and ``Eq``) -> (t_new float64 [nt, Et]: per position the mean of the
        query values aligned to it, NaN at and beyond the count, the old values of a template without a member; members int32 [nt];
        inertia float64 [nt]: the members' distances added up; dist float64 [nq], or None without ``want_dist``)"""
        q, q_count, which, nq, Eq, t, t_count, nt, Et, flags = self._align_in(q, q_count, which, t, t_count, nq, Eq)
        t_new, members, inertia = np.full((nt, Et), np.nan), np.zeros(nt, dtype=np.int32), np.zeros(nt)
        dist = np.full(nq, np.nan) if want_dist else None
        if nq == 0:
            for k in range(nt):
                t_new[k, :t_count[k]] = t[k, :t_count[k]]
            return t_new, members, inertia, dist
        self._check(self.lib.adp_dba_step(self._h, q, q_count, which, nq, Eq, t, t_count, nt, Et, int(band), flags, t_new, members,
                                          inertia, dist))
        return t_new, members, inertia, dist

    def dtw_pairwise(self, q, q_count, band: int = 0, n: Optional[int] = None, E: Optional[int] = None, out_ptr: Optional[int] = None):
        """adp_dtw_pairwise: fingerprints float64 [n, E] with their counts (host arrays, or two device pointers with ``n`` and
        ``E``) -> the symmetric DTW matrix float64 [n, n]; with ``out_ptr`` (device memory of n * n doubles) it is written there
        and None is returned"""
        q, q_count, n, E, flags = self._fp_rows(q, q_count, n, E, "fingerprints", "n and E")
        if n == 0:
            raise ValueError("no fingerprints")
        out = np.zeros((n, n)) if out_ptr is None else None
        self._check(self.lib.adp_dtw_pairwise(self._h, q, q_count, n, E, int(band), flags | (0 if out_ptr is None else ADP_OUT_DEVICE),
                                              out if out_ptr is None else int(out_ptr)))
        return out

    @staticmethod
    def _matrix_in(dist, n):
        """a distance matrix: a float64 [n, n] host array, or a device pointer with ``n`` -> (dist, n, flags)"""
        if isinstance(dist, int):
            if n is None:
                raise ValueError("a device matrix needs n")
            _check_runtime_once_torch_is_here()
            return dist, int(n), ADP_IN_DEVICE
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        if dist.ndim != 2 or dist.shape[0] != dist.shape[1] or dist.shape[0] == 0:
            raise ValueError("distances: a float64 [n, n] array")
        return dist, dist.shape[0], 0

    def kmedoids_build(self, dist, kmax: int, n: Optional[int] = None):
        """adp_kmedoids_build: PAM's BUILD on a distance matrix (host [n, n], or a device pointer with ``n``) -> (medoids int32
        [kmax]: the first K are BUILD's answer for every K <= kmax; gain float64 [kmax])"""
        dist, n, flags = self._matrix_in(dist, n)
        kmax = int(kmax)
        medoids, gain = np.zeros(max(kmax, 0), dtype=np.int32), np.zeros(max(kmax, 0))
        self._check(self.lib.adp_kmedoids_build(self._h, dist, n, kmax, flags, medoids, gain))
        return medoids, gain

    def kmedoids(self, dist, medoids, max_iter: int = 50, n: Optional[int] = None, want_sums: bool = False):
        """adp_kmedoids: alternating k-medoids from ``medoids`` int32 [k] -> a dict: medoids int32 [k], assign int32 [n], sums
        float64 [n, k] (None without ``want_sums``), cost float64 [iters + 1], iters"""
        dist, n, flags = self._matrix_in(dist, n)
        med = np.array(medoids, dtype=np.int32).reshape(-1)
        k, max_iter = med.size, int(max_iter)
        assign, sums = np.zeros(n, dtype=np.int32), (np.zeros((n, k)) if want_sums else None)
        cost, iters = np.zeros(max(max_iter, 0) + 1), np.zeros(1, dtype=np.int32)
        self._check(self.lib.adp_kmedoids(self._h, dist, n, k, max_iter, flags, med, assign, sums, cost, iters))
        return {"medoids": med, "assign": assign, "sums": sums, "cost": cost[:int(iters[0]) + 1].copy(), "iters": int(iters[0])}

    def silhouette(self, dist, assign, k: int, n: Optional[int] = None):
        """adp_silhouette: the silhouette float64 [n] of every row under ``assign`` int32 [n] with values in [0, k)"""
        dist, n, flags = self._matrix_in(dist, n)
        assign = self._per_read(assign, n, "assign")
        sil = np.zeros(n)
        self._check(self.lib.adp_silhouette(self._h, dist, n, assign, int(k), flags, sil))
        return sil

    def dtw_knn(self, q, q_count, r, r_count, k: int, band: int = 0, exclude=None, prune: bool = True, n: Optional[int] = None,
                E: Optional[int] = None, want_work: bool = False):
        """adp_dtw_knn: queries float64 [nq, Eq] with their counts (host arrays, or two device pointers with ``n`` and ``E``),
        references float64 [nr, Er] with their counts (host), ``exclude`` int32 [nq] (the reference that does not count for a query,
        -1 for none) or None -> (idx int32 [nq, k]: the k nearest references in the order (distance, index), -1 where there is none;
        dist float64 [nq, k], NaN where -1; with ``want_work`` work int64 [nq, 3]: pairs finished, pairs abandoned, DP steps).
        ``prune=False``: every pair runs to the end (the same idx and dist)"""
        r, r_count, nr, Er = self._fp_table(r, r_count, "references", "nr, Er", "r_count")
        q, q_count, nq, Eq, flags = self._fp_rows(q, q_count, n, E, "queries", "n and E", shape="nq, Eq")
        k = int(k)
        if exclude is not None:
            exclude = self._per_read(exclude, nq, "exclude")
        idx = np.full((nq, max(k, 0)), -1, dtype=np.int32)
        dist = np.full((nq, max(k, 0)), np.nan)
        work = np.zeros((nq, 3), dtype=np.int64) if want_work else None
        if nq > 0:  # (the library wants a query: an empty batch has an empty answer)
            self._check(self.lib.adp_dtw_knn(self._h, q, q_count, nq, Eq, r, r_count, nr, Er, k, int(band),
                                             flags | (0 if prune else ADP_KNN_NO_PRUNE), exclude, idx, dist, work))
        return (idx, dist, work) if want_work else (idx, dist)

    # the files Engine.format_csv made, and those among them that went through the pandas writer (a value outside the bounds)
    csv_files = 0
    csv_fallback_files = 0

    @staticmethod
    def _overflow_open_pores(rows, pop: bool = False):
        """the rows whose open_pores list lies in the registry (more entries than a row holds; an exception row prints none) and
        those lists, as rows_to_results finds them"""
        exc = (rows["fail_code"] >= 9) & (rows["fail_code"] <= 14)
        big = np.flatnonzero((rows["n_open_pores"] > MAX_OPEN_PORES) & ~exc)
        lists = []
        for i in big:
            more = (_OPEN_PORES_MORE.pop if pop else _OPEN_PORES_MORE.get)(int(rows["open_pores_more"][i]), None)
            if more is None or more.size != int(rows["n_open_pores"][i]):
                raise HipLibraryError("a row with %d open pores lost its overflow list (rows from a device buffer? fetch them "
                                      "through Engine.attach_open_pores)" % int(rows["n_open_pores"][i]))
            lists.append(more)
        return big, lists

    def format_csv_native(self, rows, read_ids, primary: str, fail: bool = False):
        """adp_format_rows (include/adapted_hip_csv.h): the rows of ONE output file (host, ROW_DTYPE, in file order) and their read
        ids -> (the file's text as the GPU printed it, the number of rows with a value outside the bounds within which that text
        is the pandas writer's).  With a count other than 0 the text is not the file's: format_csv is the call that always is."""
        rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        n = int(rows.shape[0])
        ids = [str(x).encode() for x in read_ids]
        if rows.ndim != 1 or len(ids) != n:
            raise ValueError("one read id per row")
        id_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.fromiter(map(len, ids), dtype=np.int64, count=n), out=id_off[1:])
        blob = np.frombuffer(b"".join(ids) or b"\0", dtype=np.uint8)
        more_off, more = np.zeros(n + 1, dtype=np.int64), None
        big, lists = self._overflow_open_pores(rows)
        if big.size:
            count = np.zeros(n, dtype=np.int64)
            count[big] = [a.size for a in lists]
            np.cumsum(count, out=more_off[1:])
            more = np.ascontiguousarray(np.concatenate(lists), dtype=np.int64)
        strings, str_off = csv_string_table()
        text = np.empty(int(id_off[n]) + 640 * n + 2048, dtype=np.uint8)
        size, bad = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int32)
        for _ in range(2):  # (a text longer than the first guess: once more with the length the first call reported)
            self._check(self.lib.adp_format_rows(self._h, rows, n, int(bool(fail)), PRIMARY_CODE[primary], blob, id_off, more, more_off,
                                                 strings, str_off, str_off.size - 1, text, text.size, size, bad))
            if int(size[0]) <= text.size:
                break
            text = np.empty(int(size[0]), dtype=np.uint8)
        return text[:int(size[0])].tobytes(), int(bad[0])

    def format_csv(self, rows, read_ids, primary: str, fail: bool = False, consume: bool = False) -> bytes:
        """the text of detected_boundaries_<k>.csv (``fail``: of failed_reads_<k>.csv) for the rows of that ONE file, byte for byte
        what output.save_detected_boundaries writes for rows_to_results of them -- printed on the GPU, without a DetectResults or a
        DataFrame.  A file that holds a value outside the printer's verified bounds (CSV_F64_BOUND, CSV_F32_BOUND) is not
        approximated: it goes through that pandas writer (csv_fallback_files counts such files, csv_files all).
        consume: as in rows_to_results"""
        text, bad = self.format_csv_native(rows, read_ids, primary, fail)
        self.csv_files += 1
        if bad:
            self.csv_fallback_files += 1
            return rows_csv_text(rows, read_ids, primary, fail, consume=consume)
        if consume:
            self._overflow_open_pores(rows, pop=True)
        return text

    def cnn_topk(self, scores_ptr: int, adapter_pos_ptr: int, polya_pos_ptr: int, n: int, Lo: int, k: int):
        """the k > 1 part of C3 behind given arg-maxes (tests): (cand int32 [n, k], n_peaks int32 [n]); device pointers in"""
        cand = np.zeros((n, k), dtype=np.int32)
        cnt = np.zeros(n, dtype=np.int32)
        self._check(self.lib.adp_cnn_topk(self._h, int(scores_ptr), int(adapter_pos_ptr), int(polya_pos_ptr), n, int(Lo), k, cand, cnt))
        return cand, cnt

    def cnn_predict(self, scores_ptr: int, n: int, minibatch: int, Lo: int) -> np.ndarray:
        """C3 + the scaling of cnn_detect on the device: int64 [n, 1 + max(k, 1)] (adapter end, poly(A) candidates; samples)"""
        k = max(1, int(self.cfg.polya_cand_k))
        out = np.zeros((n, 1 + k), dtype=np.int64)
        self._check(self.lib.adp_cnn_predict(self._h, int(scores_ptr), n, int(minibatch), int(Lo), out))
        return out

    def _detect_cnn(self, fn, head, n, minibatch, flags, rows_dev, want_bounds):
        """adp_detect_cnn / adp_detect_cnn_i16 (fn) behind the batch's leading arguments (head)"""
        k = max(1, int(self.cfg.polya_cand_k))
        bounds = np.zeros((n, 1 + k), dtype=np.int64) if want_bounds else None
        rows, rows_arg, out_flag = self._out(rows_dev, n)
        self._check(fn(self._h, *head, n, self.m, int(minibatch), flags | out_flag, rows_arg, bounds))
        return self.attach_open_pores(rows), bounds

    def detect_cnn_rows(self, signals, full_lens, n: int, minibatch: int, device_ptrs: bool = False, rows_dev: Optional[int] = None,
                        want_bounds: bool = True, flag_truncated: bool = False, with_start_peak: bool = False, fallback: bool = False,
                        second_opinion: bool = False):
        """combined_detect_cnn -> (rows or None when rows_dev is given, bounds int64 [n, 1 + k]).  fallback: with the short-read
        fallback applied on the device (ADP_CNN_FALLBACK; where the configuration has it on); without it the rows are those in
        front of the fallback.  bounds: what cnn_detect returned, either way.  second_opinion: reads whose row fails get the
        row of the LLR path on their minibatch where that one passes (True / "llr": ADP_CNN_SECOND_LLR; such rows carry reserved_
        bit 0); "llr_resegment": and where it fails behind a first change point, the row of its re-segmentation where that one
        passes (ADP_CNN_SECOND_RESEGMENT, an extension, untuned; reserved_ bits 0 and 5-9; not with flag_truncated).
        flag_truncated: the truncation look behind all of that, as in detect_llr_rows (ADP_FLAG_TRUNCATED).
        with_start_peak: the start-peak columns of detect_rna_start_peak overlaid on the row the call delivers, whichever phase
        made it, as in detect_llr_rows (ADP_WITH_START_PEAK); nothing else of any row changes."""
        sig, lens, flags = self._in(signals, full_lens, n, device_ptrs)
        flags |= _flag_word(with_start_peak=with_start_peak, fallback=fallback, flag_truncated=flag_truncated, second_opinion=second_opinion)
        return self._detect_cnn(self.lib.adp_detect_cnn, (sig, lens), n, minibatch, flags, rows_dev, want_bounds)

    def detect_cnn_rows_i16(self, raw_dev: int, len_dev: int, scale_dev: int, offset_dev: int, n: int, minibatch: int,
                            rows_dev: Optional[int] = None, want_bounds: bool = True, with_start_peak: bool = False, fallback: bool = False,
                            second_opinion: bool = False):
        """detect_cnn_rows over RAW int16 samples resident on the device (adp_detect_cnn_i16: the per-read calibration applied in
        registers, no float32 matrix) -> (rows or None when rows_dev is given, bounds int64 [n, 1 + k] or None).  The options
        are detect_cnn_rows'; the rows are those of calibrate_i16 + detect_cnn_rows, byte for byte.  m must be a multiple of 4;
        the truncation look has no int16 form."""
        _check_runtime_once_torch_is_here()
        flags = ADP_IN_DEVICE | _flag_word(with_start_peak=with_start_peak, fallback=fallback, second_opinion=second_opinion)
        head = (int(raw_dev), int(len_dev), int(scale_dev), int(offset_dev))
        return self._detect_cnn(self.lib.adp_detect_cnn_i16, head, n, minibatch, flags, rows_dev, want_bounds)

    def cnn_set_weights(self, state):
        """state: mapping with the reference's state-dict keys ("0.weight" ... "6.bias") -> float32 arrays (numpy, or anything
        np.asarray takes: torch CPU tensors included)"""
        arrs = []
        for key, shape in (("0.weight", (64, 1, 7)), ("0.bias", (64,)), ("2.weight", (64, 64, 7)), ("2.bias", (64,)),
                           ("4.weight", (64, 64, 7)), ("4.bias", (64,)), ("6.weight", (64, 2, 7)), ("6.bias", (2,))):
            a = state[key]
            if hasattr(a, "detach"):
                a = a.detach().cpu().numpy()
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError("CNN weight %s has shape %s, expected %s" % (key, a.shape, shape))
            arrs.append(a)
        self._check(self.lib.adp_cnn_set_weights(self._h, *arrs))
        self._cnn_weights_id = id(state)

    def cnn_forward(self, prepared_dev: int, n: int, Lc: int, scores_dev: int):
        """C2 on the device (hand-written conv stack): prepared float32 [n, Lc] -> scores float32 [n, 2, Lo]"""
        self._check(self.lib.adp_cnn_forward(self._h, int(prepared_dev), int(n), int(Lc), int(scores_dev)))

    def cnn_prepare(self, signals, n: int, out_dev_ptr: int, device_ptrs: bool = False):
        """C1 into a device buffer float32 [n, Lc] (e.g. a torch tensor's data_ptr)."""
        sig, flags = (int(signals), ADP_IN_DEVICE) if device_ptrs else (np.ascontiguousarray(signals, dtype=np.float32), 0)
        self._check(self.lib.adp_cnn_prepare(self._h, sig, int(n), self.m, flags | ADP_OUT_DEVICE, int(out_dev_ptr)))

    def llr_refine_polya(self, signals, full_lens, n: int, ranges: np.ndarray):
        sig, lens, flags = self._in(signals, full_lens, n, False)
        rg = np.ascontiguousarray(ranges, dtype=np.int64)
        out = np.zeros(n, dtype=np.int64)
        st = np.zeros(n, dtype=np.int32)
        self._check(self.lib.adp_llr_refine_polya(self._h, sig, lens, n, self.m, rg, flags, out, st))
        return out, st

    # -- debug (tests) ------------------------------------------------------------------------
    def debug_divcheck(self, d: float, first_bits: int, count: int) -> int:
        out = np.zeros(1, dtype=np.uint64)
        self._check(self.lib.adp_debug_divcheck(self._h, d, first_bits, count, out))
        return int(out[0])

    def debug_log(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._check(self.lib.adp_debug_log(self._h, x, y, x.size))
        return y

    def debug_llr_upto(self, signals, full_lens, n, minibatch, stage, tails_nan: bool = False):
        sig, lens, flags = self._in(signals, full_lens, n, False)
        flags |= _flag_word(tails_nan=tails_nan)
        self._check(self.lib.adp_debug_llr_upto(self._h, sig, lens, n, self.m, int(minibatch), flags, int(stage)))

    def debug_fetch(self, what: int, n: int):
        lp = np.zeros(1, dtype=np.int32)
        self._check(self.lib.adp_debug_fetch(self._h, 6, lp, 4))
        Lp = int(lp[0])
        if what == 6:
            return Lp
        # (the selectors are listed in include/adapted_hip.h; n: reads, or minibatches for 21)
        shapes = {1: ((n,), np.int32), 2: ((n, Lp), np.float32), 3: ((n, Lp), np.float64), 4: ((n,), np.int32),
                  5: ((n,), np.int32), 7: ((n, 2), np.int32), 9: ((n,), np.int8),
                  13: ((n, Lp // 16, 2), np.float64), 14: ((n, 2), np.float64), 15: ((n, Lp // 64), np.float64),
                  16: ((n, Lp // 64), np.float64), 17: ((n, 3), np.float64), 18: ((n,), np.int32),
                  19: ((n, Lp // 2 + 1), np.int32), 20: ((n, Lp // 2 + 1), np.float64), 21: ((n,), np.int32),
                  22: ((n,), np.int32), 23: ((n + 1,), np.int32)}
        if what == 0:
            raise ValueError("use debug_norm_params")
        shp, dt = shapes[what]
        a = np.zeros(shp, dtype=dt)
        self._check(self.lib.adp_debug_fetch(self._h, what, a, a.nbytes))
        return a

    def debug_cnn_fallback(self):
        """the fallback of the last detect_cnn_rows call: (reads selected, exception rows made, rows re-validated)"""
        a = np.zeros(3, dtype=np.int32)
        self._check(self.lib.adp_debug_fetch(self._h, 10, a, a.nbytes))
        return tuple(int(v) for v in a)

    def debug_cnn_second_opinion(self):
        """the LLR second opinion of the last detect_cnn_rows call: (reads selected, rows replaced, rows re-validated and still
        failing, minibatches with a selected read that gave none)"""
        a = np.zeros(4, dtype=np.int32)
        self._check(self.lib.adp_debug_fetch(self._h, 11, a, a.nbytes))
        return tuple(int(v) for v in a)

    def debug_truncated(self):
        """the truncation look of the last detect_llr_rows / detect_cnn_rows call made with flag_truncated: (eligible reads, reads
        whose tail window passed T1, rows replaced)"""
        a = np.zeros(3, dtype=np.int32)
        self._check(self.lib.adp_debug_fetch(self._h, 12, a, a.nbytes))
        return tuple(int(v) for v in a)

    def debug_resegment(self):
        """the re-segmentation of the last detect_llr_rows call: (eligible reads, reads whose second segmentation found a poly(A)
        end, rows replaced); (0, 0, 0) behind a call without ``resegment``"""
        a = np.zeros(3, dtype=np.int32)
        self._check(self.lib.adp_debug_fetch(self._h, 25, a, a.nbytes))
        return tuple(int(v) for v in a)

    def debug_second_resegment(self):
        """the re-segmentation behind the second opinion of the last detect_cnn_rows(_i16) call: (eligible reads, reads whose
        second segmentation found a poly(A) end, rows replaced); (0, 0, 0) behind a call whose second_opinion is not "llr_resegment" """
        a = np.zeros(3, dtype=np.int32)
        self._check(self.lib.adp_debug_fetch(self._h, 26, a, a.nbytes))
        return tuple(int(v) for v in a)

    def debug_counters(self, n: int = 8):
        a = np.zeros(n, dtype=np.uint64)
        self._check(self.lib.adp_debug_fetch(self._h, 8, a, 8 * n))
        return a

    def debug_n1_fused(self, n_mb: int):
        """what the single-pass N1 of the last plain call left per minibatch (adp_debug_fetch 24; an error when the call did not
        take that route): a list of dicts -- the brackets as float32 (med_s, A0, A1, D0, D1, eps, D0w, D1w) with ok / wide_ok,
        fused, status, nh, sample_in (sample points inside the brackets), keys uint32[nh] and counts uint32[nh]"""
        W = 78
        a = np.zeros((n_mb, W), dtype=np.uint32)
        self._check(self.lib.adp_debug_fetch(self._h, 24, a, a.nbytes))
        out = []
        for w in a:
            f = w[:10].view(np.float32)
            nh = int(w[12])
            d = {k: f[i] for i, k in ((0, "med_s"), (1, "A0"), (2, "A1"), (3, "D0"), (4, "D1"), (5, "eps"), (8, "D0w"), (9, "D1w"))}
            d.update(ok=int(w[6]), wide_ok=int(w[7]), fused=int(w[10]), status=int(w[11].view(np.int32)), nh=nh, sample_in=int(w[13]),
                     keys=w[14:14 + 32].copy(), counts=w[46:46 + 32].copy())
            out.append(d)
        return out

    def debug_norm_params(self, n_mb: int):
        a = np.zeros((n_mb, 4), dtype=np.float64)
        self._check(self.lib.adp_debug_fetch(self._h, 0, a, a.nbytes))
        return a
