"""Host-side streaming pipeline for `adapted detect`.

The reference moves minibatches between processes through pickling Manager queues
(adapted/file_proc.py:612-823); at MI355X speeds the detect step takes ~1.5 ms per 1000 reads, so the
host side is all that is left: assembling the float32 [N, m] minibatch and getting it across PCIe
(806 KB per read at the 200 k window -> about 78 k reads/s per GPU at 63 GB/s).  This module keeps that
path busy and nothing else in the way:

  producer thread   fills pinned (page-locked) staging slots in place -- no intermediate copy -- from any
                    iterator of (signals, lengths, ids) writers (io_utils.yield_minibatches(buffers=...));
  transfer/compute  (caller's thread) per slot: one asynchronous H2D copy on a copy stream, the detect call
                    on device pointers, the 544-byte result rows back; the H2D of slot k+1 is started
                    BEFORE the detect call of slot k, so copies and kernels overlap;
  consumer          `on_rows(ids, rows)` (CSV writer) runs in a third thread.

Pinned memory, device buffers and the copy stream come from the HIP library itself (adp_host_alloc,
adp_dev_alloc, adp_memcpy_h2d_async on the handle's copy stream): the LLR / start-peak path needs no PyTorch.
"""
from __future__ import annotations

import queue
import threading
from typing import Callable, Iterable, Optional, Tuple

import numpy as np

from . import lib


def native_int16_plan(primary: str, int16_input, m: int, flag_truncated: bool) -> bool:
    """Do the detect kernels read the raw int16 rows themselves (no float32 matrix on the device)?  int16_input: False, True
    (the LLR primary natively, the CNN primary through the calibrated float32 matrix) or "native" (the CNN primary natively as
    well: adp_detect_cnn_i16).  Never for rows that are not 8-byte aligned (m % 4), with the truncation look or the LLR
    re-segmentation (float32-row phases: callers pass ``flag_truncated or resegment``) or for the start-peak primary."""
    if not int16_input or m % 4 != 0 or flag_truncated:
        return False
    if primary == "llr":
        return True
    return primary == "cnn" and int16_input == "native"


# what enable_polya_length adds to a slot's rows, one entry per read (-1 / NaN for a read that did not pass): the boundaries
# between the events of its adapter, the segmentation's status, median and MAD of the event lengths (adp_segment_events)
EVENT_DTYPE = np.dtype([("n_bound", "<i8"), ("status", "<i8"), ("med", "<f8"), ("mad", "<f8")])


class AdapterFingerprints:
    """What enable_fingerprints adds to a slot's rows, one entry per read (count / status -1, lengths 0, NaN for a read that did
    not pass): the event table and fingerprint of its adapter (adp_event_levels) and, with templates, the nearest two templates
    and their DTW distances (adp_dtw_assign; best None without templates).  Sliced as the rows are."""
    FIELDS = ("count", "status", "lengths", "levels", "fingerprints", "best", "bestdist")

    def __init__(self, n: int, E: int, templates: bool):
        self.count, self.status = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
        self.lengths = np.zeros((n, E), dtype=np.int32)
        self.levels, self.fingerprints = np.full((n, E), np.nan), np.full((n, E), np.nan)
        self.best = np.full((n, 2), -1, dtype=np.int32) if templates else None
        self.bestdist = np.full((n, 2), np.nan) if templates else None

    def __len__(self):
        return self.count.size

    def __getitem__(self, sl):
        out = AdapterFingerprints.__new__(AdapterFingerprints)
        for k in self.FIELDS:
            v = getattr(self, k)
            setattr(out, k, None if v is None else v[sl])
        return out


class HostPipeline:
    def __init__(self, spc, minibatch: int, m: int, device: int = 0, n_slots: int = 3, primary: str = "llr",
                 with_start_peak: bool = False, model=None, int16_input: bool = False, group: int = 1, ragged: bool = False,
                 flag_truncated: bool = False, resegment: bool = False, second_opinion: Optional[str] = None):
        """with_start_peak: the start-peak columns on every row of the LLR and CNN primaries (an extension; the start-peak primary
        fills them anyway).
        second_opinion: None, or "llr" with the CNN primary -- reads the CNN path fails get the LLR path's row on their
        minibatch where that one passes, in the same library call (an extension; adapted_amd/detect/cnn.py); or "llr_resegment"
        -- and where that one fails behind a first change point, the row of its re-segmentation where that passes
        (ADP_CNN_SECOND_RESEGMENT, an extension, untuned; not with flag_truncated or mvs_detect_overwrite; it runs on raw int16
        rows as well, so the native int16 plan stays).
        flag_truncated: every detect call ends with the truncation look (ADP_FLAG_TRUNCATED, an extension; LLR and CNN
        primaries).  It reads float32 rows: int16 input then takes the calibrate + float32 route, not the native int16 one.
        resegment: every LLR detect call re-segments the reads its first pass fails behind a first change point (ADP_LLR_RESEGMENT,
        an extension, untuned; LLR primary only, not with flag_truncated).  Like the truncation look it reads float32 rows.
        int16_input: the staging slots hold raw ADC samples (int16) plus per-read (scale, offset); they are calibrated
        to float32 pA on the device (adp_calibrate_i16), so only 2 bytes per sample cross PCIe.  get_buffers() then hands
        out (raw, lengths, scale, offset) instead of (signals, lengths).  True: the LLR primary reads the raw rows itself, the
        CNN primary the calibrated matrix; "native": the CNN primary reads them itself as well (native_int16_plan).
        group: minibatches per staging slot and per detect call (a call over several minibatches fills the GPU better
        than one over 1000 reads; normalisation stays per minibatch).
        ragged: the staging slots hold the reads packed back to back (flat array + offsets int64 [N + 1]); only the samples
        that exist cross PCIe and the NaN-padded [N, m] minibatch is laid out on the device (adp_expand_ragged).  With
        heavy-tailed read lengths most of the padded matrix is padding.  get_buffers() hands out (flat, lengths, offsets)
        -- plus (scale, offset) with int16_input."""
        self.spc, self.mb, self.m, self.device = spc, int(minibatch), int(m), int(device)
        self.N = self.mb * max(1, int(group))  # reads per slot
        self.primary, self.with_start_peak, self.model, self.i16 = primary, with_start_peak, model, bool(int16_input)
        self.ragged = bool(ragged)
        if int16_input not in (False, True, "native"):
            raise ValueError('int16_input must be False, True or "native"')
        if second_opinion not in (None,) + lib.SECOND_OPINIONS:
            raise ValueError('second_opinion must be None, "llr" or "llr_resegment"')
        if second_opinion and primary != "cnn":
            raise ValueError("second_opinion needs the CNN primary")
        self.second_opinion = second_opinion
        self.flag_truncated = bool(flag_truncated)
        if second_opinion == "llr_resegment":
            why = lib.second_resegment_unsupported(spc, self.flag_truncated)
            if why:
                raise ValueError("second_opinion llr_resegment: " + why)
        if self.flag_truncated:
            if primary not in ("llr", "cnn"):
                raise ValueError("flag_truncated goes with the LLR and CNN primaries")
            why = lib.truncation_unsupported(spc)
            if why:
                raise ValueError("flag_truncated: " + why)
        self.resegment = bool(resegment)
        if self.resegment:
            if primary != "llr":
                raise ValueError("resegment goes with the LLR primary")
            why = lib.resegment_unsupported(spc, self.flag_truncated)
            if why:
                raise ValueError("resegment: " + why)
        self.eng = lib.Engine(spc, self.N, self.m, device=self.device)
        self.slots = []
        # int16 input + LLR primary (or the CNN primary with "native"): the kernels read the raw samples themselves
        # (adp_detect_llr_i16, adp_detect_cnn_i16) -- no float32 matrix is made
        self.native_i16 = native_int16_plan(primary, int16_input, self.m, self.flag_truncated or self.resegment)
        # the float32 minibatch made on the device (calibrated and / or laid out from packed reads); one: detect is serial
        # (native int16 + packed reads: the raw int16 matrix instead)
        self.dsig16 = None
        if self.native_i16:
            self.dsig16 = self.eng.dev_alloc(self.N * self.m * 2) if self.ragged else None
        elif self.i16 or self.ragged:
            self.dsig16 = self.eng.dev_alloc(self.N * self.m * 4)
        # staging slots are made when first handed out (page-locking a 3.2 GB slot takes about a second: a short run pins only
        # the slots it uses, and the second and third are pinned by the producer thread while the first is being processed)
        self.slots = [None] * min(16, max(2, n_slots))
        self.free: "queue.Queue[int]" = queue.Queue()
        for i in range(len(self.slots)):
            self.free.put(i)

    def enable_polya_length(self, params=None):
        """(extension) After every detect call, while the slot's float32 matrix is still resident, segment the adapter
        [adapter_start, adapter_end) of every passing read into events in one adp_segment_events call
        (adapted_amd/polya_length.py); run() then hands on_rows a third argument, an EVENT_DTYPE array beside the rows.
        params: polya_length.EventParams (None: its untuned defaults).  Not on the native int16 plan (no float32 matrix
        exists there) and not with the start-peak primary."""
        from .polya_length import EventParams

        if self.native_i16:
            raise ValueError("polya_length needs the float32 matrix on the device: not with int16 input read natively")
        if self.primary not in ("llr", "cnn"):
            raise ValueError("polya_length goes with the LLR and CNN primaries")
        params = params or EventParams()
        params.check()
        other = getattr(self, "fp_args", None)
        if other is not None and bytes(other) != bytes(params.args()):
            raise ValueError("fingerprints and polya_length share one segmentation: give both the same event parameters")
        self.event_args = params.args()

    def enable_fingerprints(self, params=None, templates=None):
        """(extension) After every detect call, while the slot's float32 matrix is still resident, the event table and the
        fingerprint of the adapter [adapter_start, adapter_end) of every passing read in one adp_event_levels call and, with
        ``templates`` (fingerprint.Templates), their DTW distances to the templates in one adp_dtw_assign call on the fingerprints
        the first call left on the device (adapted_amd/fingerprint.py); run() then hands on_rows a third and a fourth argument:
        the EVENT_DTYPE array of enable_polya_length, or None without it, and an AdapterFingerprints.  With enable_polya_length
        as well there is still one segmentation per detect call: both take the same event parameters.
        params: fingerprint.FingerprintParams (None: its untuned defaults).  Not on the native int16 plan and not with the
        start-peak primary."""
        from .fingerprint import FingerprintParams, template_arrays

        if self.native_i16:
            raise ValueError("fingerprints need the float32 matrix on the device: not with int16 input read natively")
        if self.primary not in ("llr", "cnn"):
            raise ValueError("fingerprints go with the LLR and CNN primaries")
        params = params or FingerprintParams()
        params.check()
        args = params.events.args()
        other = getattr(self, "event_args", None)
        if other is not None and bytes(other) != bytes(args):
            raise ValueError("fingerprints and polya_length share one segmentation: give both the same event parameters")
        self.fp_templates = template_arrays(templates) if templates is not None else None
        self.fp_params, self.fp_args = params, args
        self._fp_dev = None  # (fingerprints and counts of a slot's passing reads, on the device between the two calls)

    def enable_adapter_front(self, params=None):
        """(extension) After every detect call, while the slot's signal is still resident, trim the front of every passing read's
        adapter with the moving-mean start detector in one adp_adapter_front call on the call's rows (adapted_amd/adapter_front.py):
        a patched row carries the new adapter_start, adapter_len and adapter statistics and reserved_ bit 3; validation is not
        repeated.  It runs before the event segmentation of enable_polya_length / enable_fingerprints, which read the row's
        adapter_start and so segment the trimmed adapter.  Every input plan: float32 padded or packed, int16 calibrated on the
        device, int16 read natively (adp_adapter_front_i16).  params: adapter_front.AdapterFrontParams (None: the reference's
        defaults, untuned for RNA004).  Not with the start-peak primary.
        With ``params.revalidate`` the accepted reads are validated again from the trimmed start in the same call
        (adp_adapter_front_revalidate / _i16): a row whose validation passes is replaced (reserved_ bits 3 and 4), a read whose
        validation fails keeps its row -- counted in front_rejected.  Not with mvs_detect_overwrite; min_adapter_len >= 1."""
        from .adapter_front import AdapterFrontParams

        if self.primary not in ("llr", "cnn"):
            raise ValueError("adapter_front goes with the LLR and CNN primaries")
        params = params or AdapterFrontParams()
        params.check()
        self.front_revalidate = bool(getattr(params, "revalidate", False))
        if self.front_revalidate:
            if int(params.min_adapter_len) < 1:
                raise ValueError("adapter_front with revalidate needs min_adapter_len >= 1")
            if bool(getattr(self.spc.mvs_polya, "mvs_detect_overwrite", False)):
                raise ValueError("adapter_front with revalidate does not go with mvs_detect_overwrite")
        self.front_args = params.args()
        self.front_patched = 0  # rows patched so far
        self.front_rejected = 0  # (revalidate) trims the validation rejected so far

    def _adapter_front(self, j: int, n: int, rows: np.ndarray):
        """the adapter-front pass over the rows of slot j's detect call, on the signal that call just read; rows are patched in
        place (rows of a dropped minibatch have success 0: they are not looked at)"""
        if getattr(self, "front_revalidate", False):  # (the full lengths: the slot's, on the device beside the signal)
            if self.native_i16:
                raw, dlen, scale, offset = self._resident_i16
                out = self.eng.adapter_front_revalidate_i16(raw, dlen, scale, offset, rows, self.front_args, n=n, m=self.m)
            else:
                out = self.eng.adapter_front_revalidate(self._resident, self.slots[j]["dl"], rows, self.front_args, n=n, m=self.m)
            self.front_patched += int(out[0][:, 3].sum())
            self.front_rejected += int((out[4][:, 0] == 0).sum())
            return rows
        if self.native_i16:
            raw, dlen, scale, offset = self._resident_i16
            info = self.eng.adapter_front_i16(raw, dlen, scale, offset, rows, self.front_args, n=n, m=self.m)[0]
        else:
            info = self.eng.adapter_front(self._resident, None, rows, self.front_args, n=n, m=self.m)[0]
        self.front_patched += int(info[:, 3].sum())
        return rows

    def _passing_adapters(self, j: int, n: int, rows: np.ndarray, mbs):
        """the passing reads of undropped minibatches of slot j -> (their indices, adapter starts, adapter ends)"""
        ok = rows["success"][:n] != 0
        if mbs is not None:  # (the rows of a dropped minibatch mean nothing)
            ok &= np.repeat(np.asarray(mbs) == lib.MB_OK, self.mb)[:n]
        idx = np.flatnonzero(ok)
        col, present = rows["col"][idx], rows["present"][idx]
        starts = np.where(present >> np.uint64(2) & np.uint64(1), col[:, 2], 0).astype(np.int64)
        ends = np.where(present >> np.uint64(3) & np.uint64(1), col[:, 3], 0).astype(np.int64)
        return idx, starts, ends

    @staticmethod
    def _no_events(n: int) -> np.ndarray:
        ev = np.zeros(n, dtype=EVENT_DTYPE)
        ev["n_bound"], ev["status"], ev["med"], ev["mad"] = -1, -1, np.nan, np.nan
        return ev

    def _adapter_events(self, j: int, n: int, rows: np.ndarray, mbs) -> np.ndarray:
        """the events of the passing reads' adapters, from the matrix the detect call of slot j just read"""
        ev = self._no_events(n)
        idx, starts, ends = self._passing_adapters(j, n, rows, mbs)
        if idx.size:
            lens = np.minimum(self.slots[j]["lens"][:n], self.m).astype(np.int32)
            _, info, stats = self.eng.segment_events(self._resident, lens, idx, starts, ends, self.event_args, cap=0, n=n, L=self.m)
            ev["n_bound"][idx], ev["status"][idx] = info[:, 0], info[:, 1]
            ev["med"][idx], ev["mad"][idx] = stats[:, 0], stats[:, 1]
        return ev

    def _adapter_fingerprints(self, j: int, n: int, rows: np.ndarray, mbs):
        """-> (the EVENT_DTYPE array of _adapter_events, or None without enable_polya_length; AdapterFingerprints): one
        adp_event_levels call -- its info / stats are adp_segment_events' --, then adp_dtw_assign on what it left on the device"""
        E, tm = int(self.fp_params.max_events), self.fp_templates
        ev = self._no_events(n) if getattr(self, "event_args", None) is not None else None
        fp = AdapterFingerprints(n, E, tm is not None)
        idx, starts, ends = self._passing_adapters(j, n, rows, mbs)
        if idx.size:
            lens = np.minimum(self.slots[j]["lens"][:n], self.m).astype(np.int32)
            if tm is not None and self._fp_dev is None:
                self._fp_dev = (self.eng.dev_alloc(self.N * E * 8), self.eng.dev_alloc(self.N * 4))
            dev = dict(fp_ptr=self._fp_dev[0], count_ptr=self._fp_dev[1]) if tm is not None else {}
            r = self.eng.event_levels(self._resident, lens, idx, starts, ends, self.fp_args, E, n=n, L=self.m, **dev)
            if tm is not None:
                _, best, bestdist = self.eng.dtw_assign(self._fp_dev[0], self._fp_dev[1], tm[0], tm[1], int(self.fp_params.band),
                                                        nq=idx.size, Eq=E, want_dist=False)
                fp.best[idx], fp.bestdist[idx] = best, bestdist
                r["fingerprints"], r["count"] = np.zeros((idx.size, E)), np.zeros(idx.size, dtype=np.int32)
                self.eng.d2h(r["fingerprints"], self._fp_dev[0])
                self.eng.d2h(r["count"], self._fp_dev[1])
            for k in ("count", "status", "lengths", "levels", "fingerprints"):
                getattr(fp, k)[idx] = r[k]
            if ev is not None:
                ev["n_bound"][idx], ev["status"][idx] = r["info"][:, 0], r["info"][:, 1]
                ev["med"][idx], ev["mad"][idx] = r["stats"][:, 0], r["stats"][:, 1]
        return ev, fp

    def _slot(self, j: int):
        if self.slots[j] is None:
            sig = self.eng.host_alloc((self.N * self.m,) if self.ragged else (self.N, self.m), np.int16 if self.i16 else np.float32)
            lens = self.eng.host_alloc((self.N,), np.int32)
            slot = {"sig": sig, "lens": lens, "ds": self.eng.dev_alloc(self.N * self.m * (2 if self.i16 else 4)),
                    "dl": self.eng.dev_alloc(self.N * 4)}
            if self.ragged:
                slot["offs"] = self.eng.host_alloc((self.N + 1,), np.int64)
                slot["do"] = self.eng.dev_alloc((self.N + 1) * 8)
            if self.i16:
                slot["cal"] = self.eng.host_alloc((2, self.N), np.float32)  # scale, offset
                slot["dcal"] = self.eng.dev_alloc(2 * self.N * 4)
            self.slots[j] = slot
        return self.slots[j]

    def close(self):
        for s in self.slots:
            if s is None:
                continue
            self.eng.host_free(s["sig"])
            self.eng.host_free(s["lens"])
            self.eng.dev_free(s["ds"])
            self.eng.dev_free(s["dl"])
            if "cal" in s:
                self.eng.host_free(s["cal"])
                self.eng.dev_free(s["dcal"])
            if "offs" in s:
                self.eng.host_free(s["offs"])
                self.eng.dev_free(s["do"])
        if self.dsig16:
            self.eng.dev_free(self.dsig16)
            self.dsig16 = None
        if getattr(self, "_fp_dev", None):
            for ptr in self._fp_dev:
                self.eng.dev_free(ptr)
            self._fp_dev = None
        self.slots = []
        self.eng.close()

    # -- stages -------------------------------------------------------------------------------
    def _start_h2d(self, j: int, n: int):
        s = self.slots[j]
        if self.ragged:  # only the samples that exist
            self.eng.h2d_async(s["ds"], s["sig"], int(s["offs"][n]) * (2 if self.i16 else 4))
            self.eng.h2d_async(s["do"], s["offs"], (n + 1) * 8)
        else:
            self.eng.h2d_async(s["ds"], s["sig"], n * self.m * (2 if self.i16 else 4))
        self.eng.h2d_async(s["dl"], s["lens"], n * 4)
        if self.i16:
            self.eng.h2d_async(s["dcal"], s["cal"])
        self.eng.copy_mark(j)

    def _detect(self, j: int, n: int):
        """-> (rows, per-minibatch status or None)"""
        s = self.slots[j]
        self.eng.copy_wait(j)  # this slot's copies only: the next slot's may still be in flight
        dsig, dlen = s["ds"], s["dl"]
        # the CNN primary's options (the reference runs find_peaks and its row compaction per minibatch: adapted/detect/cnn.py:136-160)
        options = dict(minibatch=self.mb, second_opinion=self.second_opinion or False, with_start_peak=bool(self.with_start_peak))
        if self.native_i16:
            if self.ragged:
                self.eng.expand_ragged_i16(dsig, s["do"], dlen, n, self.dsig16)
                dsig = self.dsig16
            self._resident_i16 = (dsig, dlen, s["dcal"], s["dcal"] + self.N * 4)  # the raw matrix this call reads, and its calibration
            if self.primary == "cnn":
                from .detect import cnn as _cnn

                return _cnn.detect_rows_device_i16(self.eng, dsig, dlen, s["dcal"], s["dcal"] + self.N * 4, n, s["lens"][:n], self.model,
                                                   self.spc, **options), None
            return self.eng.detect_llr_rows_i16(dsig, dlen, s["dcal"], s["dcal"] + self.N * 4, n, self.mb, with_start_peak=self.with_start_peak)
        if self.ragged:  # packed reads (-> calibrated) -> float32 [n, m], NaN beyond each read
            if self.i16:
                self.eng.expand_ragged(dsig, True, s["do"], dlen, n, self.dsig16, s["dcal"], s["dcal"] + self.N * 4)
            else:
                self.eng.expand_ragged(dsig, False, s["do"], dlen, n, self.dsig16)
            dsig = self.dsig16
        elif self.i16:  # raw ADC -> float32 pA, NaN beyond the read, on the engine's stream ahead of the detect kernels
            self.eng.calibrate_i16(dsig, dlen, s["dcal"], s["dcal"] + self.N * 4, n, self.dsig16)
            dsig = self.dsig16
        self._resident = dsig  # the float32 [n, m] matrix this call reads (it stays until the next slot's call)
        if self.primary == "llr":
            # (the staging slots are NaN padded by the reader / the on-device calibration: the passes may stop at each read's end)
            rows, mbs = self.eng.detect_llr_rows(dsig, dlen, n, self.mb, with_start_peak=self.with_start_peak, device_ptrs=True,
                                                 tails_nan=True, flag_truncated=self.flag_truncated, resegment=getattr(self, "resegment", False))
            return rows, mbs
        if self.primary == "start_peak":
            return self.eng.detect_start_peak_rows(dsig, dlen, n, self.mb, device_ptrs=True), None
        from .detect import cnn as _cnn

        return _cnn.detect_rows_device_second_opinion(self.eng, dsig, dlen, n, s["lens"][:n], self.model, self.spc,
                                                      flag_truncated=self.flag_truncated, **options), None

    # -- driver -------------------------------------------------------------------------------
    def run(self, fill: Callable[[Callable[[], Tuple[np.ndarray, np.ndarray]]], Iterable[Tuple[int, object]]],
            on_rows: Callable[[object, np.ndarray], None], on_dropped: Optional[Callable[[object, int], None]] = None) -> int:
        """fill(get_buffers) -> iterator of (n, ids): every item announces that the buffers handed out by the LAST
        get_buffers() call now hold n reads (up to group * minibatch; ids: a sequence of n ids, sliced per minibatch when
        one is dropped -- or any tag when group == 1).  Returns the number of reads processed."""
        filled: "queue.Queue" = queue.Queue(maxsize=len(self.slots))
        done: "queue.Queue" = queue.Queue(maxsize=4 * len(self.slots))
        err = []
        cur = {"j": None}

        def get_buffers():
            j = self.free.get()
            cur["j"] = j
            sl = self._slot(j)
            head = (sl["sig"], sl["lens"], sl["offs"]) if self.ragged else (sl["sig"], sl["lens"])
            if self.i16:
                return head + (sl["cal"][0], sl["cal"][1])
            return head

        stop = threading.Event()

        def put_filled(item):
            while not stop.is_set():
                try:
                    filled.put(item, timeout=0.2)
                    return
                except queue.Full:
                    continue

        def producer():
            gen = fill(get_buffers)
            try:
                for n, ids in gen:
                    if stop.is_set():
                        break
                    put_filled((cur["j"], int(n), ids))
            except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread
                err.append(e)
            finally:
                if hasattr(gen, "close"):
                    try:
                        gen.close()  # (lets the reader shut its copy pool down)
                    except BaseException as e:  # noqa: BLE001
                        err.append(e)
                put_filled(None)

        def consumer():
            while True:
                item = done.get()
                if item is None:
                    return
                try:
                    on_rows(*item)
                except BaseException as e:  # noqa: BLE001
                    err.append(e)

        tp = threading.Thread(target=producer, daemon=True)
        tc = threading.Thread(target=consumer, daemon=True)
        tp.start()
        tc.start()
        total = 0
        pending = None  # slot whose H2D is in flight
        try:
            while True:
                item = filled.get()
                if item is not None:
                    self._start_h2d(item[0], item[1])
                if pending is not None:
                    j, n, ids = pending
                    rows, mbs = self._detect(j, n)
                    if getattr(self, "front_args", None) is not None:  # (with enable_adapter_front: ahead of the event segmentation)
                        rows = self._adapter_front(j, n, rows)
                    # (with enable_polya_length: a third item travels with the rows, sliced as they are)
                    # (with enable_fingerprints: the events, or None, and the fingerprints)
                    if getattr(self, "fp_params", None) is not None:
                        more = self._adapter_fingerprints(j, n, rows, mbs)
                    else:
                        more = (self._adapter_events(j, n, rows, mbs),) if getattr(self, "event_args", None) is not None else ()
                    if mbs is None or (mbs == lib.MB_OK).all():
                        done.put((ids, rows) + more)
                        total += n
                    else:  # some minibatch of the group was dropped (the reference logs it and goes on)
                        for q, st in enumerate(mbs):
                            a, b = q * self.mb, min(n, (q + 1) * self.mb)
                            sub = ids[a:b] if hasattr(ids, "__getitem__") and not isinstance(ids, tuple) else ids
                            if st == lib.MB_OK:
                                done.put((sub, rows[a:b]) + tuple(None if e is None else e[a:b] for e in more))
                                total += b - a
                            elif on_dropped:
                                on_dropped(sub, int(st))
                    self.free.put(j)
                pending = item
                if item is None:
                    break
                if err:
                    break
        finally:
            # an error (or an exception out of _detect) may leave the producer mid-slot: it has to be gone before the caller
            # frees the pinned slots it writes into (close()), so stop it, unblock it and wait for it
            stop.set()
            while True:
                try:
                    filled.get_nowait()
                except queue.Empty:
                    break
            for j in range(len(self.slots)):
                self.free.put(j)
            tp.join(timeout=120)
            producer_gone = not tp.is_alive()
            done.put(None)
            tc.join()
            try:
                self.eng.copy_wait(-1)  # no H2D copy may still be reading a pinned slot when the caller frees them
            except Exception as e:  # noqa: BLE001
                err.append(e)
            if not producer_gone:
                # still inside a read / decode that does not return: its slots must outlive it -- close() will not free them
                self.slots = [None] * len(self.slots)
                err.insert(0, RuntimeError("the reader thread did not stop within 120 s; its pinned staging slots are left allocated"))
            # the free list back to one token per slot for the next run()
            while True:
                try:
                    self.free.get_nowait()
                except queue.Empty:
                    break
            for j in range(len(self.slots)):
                self.free.put(j)
        if err:
            raise err[0]
        return total
