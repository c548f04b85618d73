"""CNN boundary head (the reference's adapted/detect/cnn.py) on MI355X.

Everything numeric is the HIP library: ``prepare_data`` (pool + per-read median / MAD normalisation, C1), the conv net
itself (C2: hand-written, the two 64 -> 64 layers on the float32 matrix cores -- adapted_amd/csrc/cnn_conv.h), ``cnn_predict``
(C3: both arg-maxes, scipy's find_peaks(distance=5) on the flattened scores, the per-read top-k and the reference's
row-compaction quirk -- adapted_amd/csrc/cnn_topk.h), the candidate validation loop (V1 with k candidates) and the short-read
fallback (C4: selection, the LLR chain and the re-validation on the rows where they lie -- adapted_amd/csrc/cnn_fallback.h).  The
product path (``detect_rows`` / ``detect_rows_device``) is ONE library call, ``adp_detect_cnn`` with ``ADP_CNN_FALLBACK``: no
host work behind it.  ``fallback="host"`` is the same fallback applied by the caller (three more library calls and the affected
reads over PCIe): what ``conv="torch"`` uses, and the yardstick of tests/test_gpu_cnn_fallback.py -- the rows are the same.
PyTorch is optional: ``load_cnn_model`` returns the reference's ``nn.Sequential`` (state-dict compatible), and
``conv="torch"`` runs the conv stack through PyTorch-ROCm / MIOpen instead (kept as the float32 cross-check of C2; the
hand-written stack is 3.4x faster at the 200 k window).

reference: BoundariesCNN :16-52, load_cnn_model :55-67, prepare_data :70-82, cnn_score :85-98,
cnn_predict :101-160, cnn_detect :165-182, cnn_detect_boundaries :185-201 (adapted/detect/cnn.py);
driver combined_detect_cnn adapted/detect/combined.py:230-309.
"""
from __future__ import annotations

import os
import warnings
from typing import List, Optional, Union

import numpy as np

from .. import lib
from ..container_types import Boundaries, DetectResults

SCORE_EXCL = -5.0
MODEL_DOWNSCALE = {"rna004_130bps@v0.2.4.pth": 10, "rna004_130bps@v0.2.4.npz": 10}
_MODEL_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models")


def _torch():
    import torch

    return torch


def BoundariesCNN(channels: int = 64, kernel_size: int = 7):
    """conv(1->C, k, stride k//2) - ReLU - conv(C->C) - ReLU - conv(C->C) - ReLU - convT(C->2, stride k//2);
    an ``nn.Sequential`` so that state-dict keys ("0.weight", "2.weight", ...) match the reference's."""
    nn = _torch().nn
    s, p = kernel_size // 2, kernel_size // 2
    return nn.Sequential(
        nn.Conv1d(1, channels, kernel_size, stride=s, padding=p), nn.ReLU(),
        nn.Conv1d(channels, channels, kernel_size, padding=p), nn.ReLU(),
        nn.Conv1d(channels, channels, kernel_size, padding=p), nn.ReLU(),
        nn.ConvTranspose1d(channels, 2, kernel_size, stride=s, padding=p),
    )


def _resolve(path: str) -> str:
    cands = [path]
    base = os.path.basename(path)
    stem = os.path.splitext(base)[0]
    for d in filter(None, [os.environ.get("ADAPTED_MODEL_DIR"), _MODEL_DIR]):
        cands += [os.path.join(d, base), os.path.join(d, stem + ".npz"), os.path.join(d, stem + ".pth")]
    for c in cands:
        if os.path.isfile(c):
            return c
    raise FileNotFoundError("Model weights not found at %s (searched %s)" % (path, ", ".join(cands)))


def load_cnn_model(path: str, device: Optional[Union[int, str]] = None):
    """Load weights from a ``.pth`` state dict (as shipped by the reference) or a ``.npz`` with the
    same keys.  The model is moved to the GPU and put in eval mode."""
    torch = _torch()
    f = _resolve(path)
    model = BoundariesCNN()
    if f.endswith(".npz"):
        z = np.load(f)
        sd = {k: torch.from_numpy(np.ascontiguousarray(z[k])) for k in z.files if k[0].isdigit()}
    else:
        sd = torch.load(f, weights_only=True, map_location="cpu")
    model.load_state_dict(sd)
    model.eval()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else "cpu"
    return model.to(torch.device("cuda", device) if isinstance(device, int) else torch.device(device))


def load_cnn_weights(path: str) -> dict:
    """The state dict as float32 numpy arrays, without PyTorch for ``.npz`` files (keys "0.weight" ... "6.bias")."""
    f = _resolve(path)
    if f.endswith(".npz"):
        z = np.load(f)
        return {k: np.ascontiguousarray(z[k], dtype=np.float32) for k in z.files if k[0].isdigit()}
    sd = _torch().load(f, weights_only=True, map_location="cpu")
    return {k: v.numpy() for k, v in sd.items()}


def _state_of(model, spc=None) -> dict:
    """model: the nn.Sequential of load_cnn_model, a state dict / dict of arrays, or None (the config's model_name)"""
    if model is None:
        return load_cnn_weights(spc.cnn_boundaries.model_name)
    if isinstance(model, dict):
        return model
    return model.state_dict()


def ensure_weights(eng, model, spc=None):
    """hand the model's weights to the engine once (adp_cnn_set_weights)"""
    key = id(model) if model is not None else ("cfg", spc.cnn_boundaries.model_name)
    if getattr(eng, "_cnn_key", None) != key:
        eng.cnn_set_weights(_state_of(model, spc))
        eng._cnn_key = key
        eng._cnn_model_ref = model  # (keeps id(model) from being reused while the engine remembers it)


def _model_device(model):
    return next(model.parameters()).device


def prepare_data(batch_of_signals: np.ndarray, core_params, spc=None, engine=None):
    """float32 [N, 1, Lc] on the GPU (C1, computed by the HIP library)."""
    torch = _torch()
    sig = np.ascontiguousarray(batch_of_signals, dtype=np.float32)
    n, m = sig.shape
    if engine is None:
        from .combined import get_engine

        engine = get_engine(spc, n, m, torch.cuda.current_device())
    off, ds = int(core_params.min_obs_adapter), int(core_params.downscale_factor)
    Lc = (m - off + ds - 1) // ds
    out = torch.empty((n, 1, Lc), dtype=torch.float32, device=torch.device("cuda", engine.device))
    engine.cnn_prepare(sig, n, out.data_ptr())
    return out


def cnn_score(batch_of_prepared_signals, model, engine=None):
    """float32 [N, 2, Lo].  engine: the hand-written conv stack of the HIP library (adp_cnn_forward); without one the
    PyTorch-ROCm modules of ``model`` (the float32 cross-check)."""
    torch = _torch()
    if engine is None:
        if len(model.state_dict()) == 0:
            raise ValueError("Model weights were not loaded")
        x = batch_of_prepared_signals
        # in slices of <= 2 GiB of 64-channel activations: MIOpen returns wrong scores for a batch beyond 4 GiB
        per_read = 64 * 4 * ((int(x.shape[-1]) - 1) // 3 + 1)
        step = max(1, (2 << 30) // per_read)
        with torch.no_grad():
            if x.shape[0] <= step:
                return model(x)
            return torch.cat([model(x[s0:s0 + step]) for s0 in range(0, x.shape[0], step)], dim=0)
    x = batch_of_prepared_signals.contiguous()
    n, _, Lc = x.shape
    Lo = 3 * ((Lc - 1) // 3 + 1) - 2
    ensure_weights(engine, model)
    out = torch.empty((n, 2, Lo), dtype=torch.float32, device=x.device)
    torch.cuda.current_stream(x.device).synchronize()  # the engine works on its own stream
    engine.cnn_forward(x.data_ptr(), n, Lc, out.data_ptr())
    return out


def cnn_predict(batch_of_prepared_signals, model, params, core_params, engine=None, conv: str = "hip") -> np.ndarray:
    """int [N, 1 + max(k, 1)] pooled indices: adapter position and the k poly(A) candidates (C3 on the device)."""
    torch = _torch()
    if engine is None:
        raise lib.HipLibraryError("cnn_predict runs on the HIP engine (no CPU path)")
    if int(params.polya_cand_k) != int(engine.cfg.polya_cand_k):
        raise ValueError("params.polya_cand_k differs from the engine's configuration")
    scores = cnn_score(batch_of_prepared_signals, model, engine=engine if conv == "hip" else None).contiguous()
    n, _, Lo = scores.shape
    torch.cuda.current_stream(scores.device).synchronize()
    b = engine.cnn_predict(scores.data_ptr(), n, n, Lo)
    off, ds = int(core_params.min_obs_adapter), int(core_params.downscale_factor)
    return np.where(b == 0, 0, (b - off) // ds)  # (a sample position of 0 stands for index 0, cnn.py:173-179)


def cnn_detect(batch_of_signals: np.ndarray, model, params, core_params, spc=None, engine=None, conv: str = "hip") -> np.ndarray:
    prepared = prepare_data(batch_of_signals, core_params, spc=spc, engine=engine)
    if engine is None:
        from .combined import get_engine

        engine = get_engine(spc, prepared.shape[0], np.asarray(batch_of_signals).shape[1], prepared.device.index)
    preds = (cnn_predict(prepared, model, params, core_params, engine=engine, conv=conv) * core_params.downscale_factor
             + core_params.min_obs_adapter).astype(int)
    preds[preds == core_params.min_obs_adapter] = 0  # where the prediction was zero, set back to zero
    return preds


def cnn_detect_boundaries(batch_of_signals: np.ndarray, model, params, core_params, spc=None) -> List[Boundaries]:
    preds = cnn_detect(batch_of_signals, model, params, core_params, spc=spc)
    return [Boundaries(adapter_start=0, adapter_end=p[0], polya_end=p[1], polya_end_topk=p[1:]) for p in preds]


def _need_fallback(rows, bounds, lens, spc):
    """C4 "hail mary" for short reads (combined.py:251-301): which reads take it"""
    ae, pe = bounds[:, 0], bounds[:, 1]
    return np.flatnonzero((rows["success"] == 0) & ~((rows["fail_code"] >= 9) & (rows["fail_code"] <= 14)) & (ae > 0) & (pe > 0)
                          & (pe - ae > 1000) & (np.asarray(lens).astype(np.int64) < 2 * spc.core.max_obs_adapter))


def _fallback_mode(fallback: str) -> str:
    if fallback not in ("device", "host"):
        raise ValueError('fallback must be "device" or "host"')
    return fallback


def _apply_fallback(eng, rows, idx, sig_sub, lens_sub, bounds, spc):
    new_pe, status = eng.llr_refine_polya(sig_sub, lens_sub, idx.size, bounds[idx, :2])
    for j, i in enumerate(idx):
        if status[j] != 0:  # the reference raised inside its per-read try block
            rows[i] = lib.empty_rows(1)[0]
            rows[i]["fail_code"] = status[j]
    redo = [j for j in range(idx.size) if status[j] == 0 and new_pe[j] > 0]
    if redo:
        ii = idx[redo]
        b2 = np.stack([bounds[ii, 0], new_pe[redo]], axis=1).astype(np.int64)
        rows[ii] = eng.validate_rows(sig_sub[redo], lens_sub[redo], len(ii), b2)


def _refuse_host_forms(conv: str, fallback: str, with_start_peak: bool, host_forms: bool, int16: bool = False, flag_truncated: bool = False):
    """What runs inside the library call has no host-side form: the start-peak overlay (applied to the row the call finally
    delivers), the LLR second opinion and the truncation look (behind the library's own conv stack and fallback) and int16 rows
    (read by the kernels themselves).  Rows made (conv = "torch") or replaced (fallback = "host") behind the call would come
    without them.  host_forms: the entry has those two forms.  Looks at nothing but its arguments, so it comes before an engine,
    a model or the configuration is touched."""
    if int16:
        if conv != "hip" or _fallback_mode(fallback) != "device":
            raise ValueError('int16 rows are read inside the library call: conv must be "hip" and fallback "device"')
        if flag_truncated:
            raise ValueError("the truncation look reads float32 rows: there is none over int16 rows")
        return
    for applies, what in ((with_start_peak, "with_start_peak"), (not host_forms, "the LLR second opinion / the truncation look")):
        if applies and conv != "hip":
            raise ValueError('%s runs inside the library call: conv must be "hip"' % what)
        if applies and _fallback_mode(fallback) != "device":
            raise ValueError('%s runs inside the library call: fallback must be "device"' % what)


# The one path behind every detect_rows* entry; their parameter lists are what callers and tests pin.  Kept as it was found:
#   - only the host-batch entries refuse polya_cand_k < 1 here, the resident ones leave it to the library;
#   - conv = "torch" never looks at ``fallback``: its fallback is the host's whatever that says;
#   - inside the library the fallback is always asked for (ADP_CNN_FALLBACK): the library applies it where the configuration has it;
#   - host_forms is the entry's, not the options': the _start_peak / _truncated / _second_opinion entries refuse conv = "torch"
#     and fallback = "host" with every option off as well;
#   - the resident forms run lib's check of the HIP runtime (Engine._in, detect_cnn_rows_i16); Engine.detect_llr_rows_i16 does not;
#   - combined_detect_cnn hands n == 0 to the engine and a single read's result back bare; combined_detect_cnn_llr returns [] and a list.
def _detect_rows(eng, sig, lens, model, spc, dlen: Optional[int] = None, n: Optional[int] = None, calibration=None, conv: str = "hip",
                 fallback: str = "device", second_opinion: bool = False, flag_truncated: bool = False, with_start_peak: bool = False,
                 minibatch: Optional[int] = None, host_forms: bool = False) -> np.ndarray:
    """combined_detect_cnn over one batch -> adp_row[]: ONE library call -- or, with conv = "torch" / fallback = "host", the
    predictions made / the short-read fallback applied here, behind it.  The batch: sig float32 [n, m] and lens int32 [n] on the
    host; or resident rows, sig and dlen (int32 [n]) pointers, n given and lens the host's copy of the lengths -- float32 rows,
    or with calibration = (dscale, doffset) pointers raw int16 rows (adp_detect_cnn_i16)."""
    resident, int16 = dlen is not None, calibration is not None
    lib.second_opinion_flags(second_opinion)  # (a ValueError for a value it does not know, before anything else)
    _refuse_host_forms(conv, fallback, with_start_peak, host_forms, int16, flag_truncated)
    if not resident:
        n = sig.shape[0]
        if int(spc.cnn_boundaries.polya_cand_k) < 1:
            raise ValueError("polya_cand_k must be >= 1")
    on_host = conv != "hip" or _fallback_mode(fallback) == "host"  # the fallback, and with it the predictions it selects by
    if conv == "hip":
        ensure_weights(eng, model, spc)
        options = dict(want_bounds=on_host, fallback=not on_host, second_opinion=second_opinion, with_start_peak=with_start_peak)
        if int16:
            rows, bounds = eng.detect_cnn_rows_i16(sig, dlen, *calibration, n, minibatch or n, **options)
        else:
            rows, bounds = eng.detect_cnn_rows(sig, dlen if resident else lens, n, minibatch or n, device_ptrs=resident,
                                               flag_truncated=flag_truncated, **options)
    else:
        preds = cnn_detect(sig, model, spc.cnn_boundaries, spc.core, spc=spc, engine=eng, conv=conv)
        bounds = np.ascontiguousarray(preds, dtype=np.int64)
        rows = eng.validate_rows(sig, lens, n, bounds)
    if on_host and spc.cnn_boundaries.fallback_to_llr_short_reads:
        idx = _need_fallback(rows, bounds, lens, spc)
        if idx.size:
            if resident:  # the selected reads over PCIe, one row each
                sub = np.zeros((idx.size, eng.m), dtype=np.float32)
                for j, i in enumerate(idx):
                    eng.d2h(sub[j], sig + int(i) * eng.m * 4)
            else:
                sub = sig[idx]
            _apply_fallback(eng, rows, idx, sub, np.asarray(lens)[idx], bounds, spc)
    return rows


def detect_rows(eng, sig: np.ndarray, lens: np.ndarray, model, spc, conv: str = "hip", fallback: str = "device") -> np.ndarray:
    """combined_detect_cnn over one batch -> adp_row[] (reference adapted/detect/combined.py:230-309).
    conv = "torch": the conv stack through PyTorch-ROCm instead of the library's own (cross-check; its fallback is the host's).
    fallback = "host": the short-read fallback applied here, behind the library call, instead of inside it (same rows)."""
    return _detect_rows(eng, sig, lens, model, spc, conv=conv, fallback=fallback, host_forms=True)


def detect_rows_device(eng, dsig: int, dlen: int, n: int, lens_host: np.ndarray, model, spc, minibatch: Optional[int] = None,
                       fallback: str = "device") -> np.ndarray:
    """combined_detect_cnn over a DEVICE-resident batch (pointers) -> adp_row[]; ONE library call (adp_detect_cnn), the
    short-read fallback included.  minibatch: reads per call of the reference (its find_peaks and row compaction work on one
    minibatch); default: the whole batch.  fallback = "host": the fallback applied here instead, on host copies of the
    affected reads (same rows)."""
    return _detect_rows(eng, dsig, lens_host, model, spc, dlen, n, fallback=fallback, minibatch=minibatch, host_forms=True)


def detect_rows_start_peak(eng, sig: np.ndarray, lens: np.ndarray, model, spc, conv: str = "hip", fallback: str = "device") -> np.ndarray:
    """detect_rows with the start-peak overlay (ADP_WITH_START_PEAK, include/adapted_hip.h): every row is detect_rows' row with the
    start-peak columns of detect_rna_start_peak and start_peak_type filled as combined_detect_llr2's option of that name fills
    them.  An extension: the reference keeps one primary per run.  ONE library call, so neither conv = "torch" nor
    fallback = "host".  (detect_rows itself keeps the parameters it was introduced with; the truncated / second-opinion forms
    take ``with_start_peak``.)"""
    return _detect_rows(eng, sig, lens, model, spc, conv=conv, fallback=fallback, with_start_peak=True)


def detect_rows_device_start_peak(eng, dsig: int, dlen: int, n: int, lens_host: np.ndarray, model, spc, minibatch: Optional[int] = None,
                                  fallback: str = "device") -> np.ndarray:
    """detect_rows_device with the start-peak overlay.  ONE library call over the resident batch."""
    return _detect_rows(eng, dsig, lens_host, model, spc, dlen, n, fallback=fallback, minibatch=minibatch, with_start_peak=True)


def detect_rows_truncated(eng, sig: np.ndarray, lens: np.ndarray, model, spc, conv: str = "hip", fallback: str = "device",
                          with_start_peak: bool = False) -> np.ndarray:
    """detect_rows with the truncation look behind it (ADP_FLAG_TRUNCATED, include/adapted_hip.h): a read whose poly(A) runs into
    the end of the preloaded window gets the row of the validation with (adapter end, window end) and polya_truncated
    (``reserved_`` bit 1); every row carries bit 2.  An extension: the reference never sets ``polya_truncated``.  ONE library call."""
    return _detect_rows(eng, sig, lens, model, spc, conv=conv, fallback=fallback, flag_truncated=True, with_start_peak=with_start_peak)


def detect_rows_device_truncated(eng, dsig: int, dlen: int, n: int, lens_host: np.ndarray, model, spc, minibatch: Optional[int] = None,
                                 fallback: str = "device", with_start_peak: bool = False) -> np.ndarray:
    """detect_rows_device with the truncation look behind it.  ONE library call over the resident batch."""
    return _detect_rows(eng, dsig, lens_host, model, spc, dlen, n, fallback=fallback, minibatch=minibatch, flag_truncated=True,
                        with_start_peak=with_start_peak)


def detect_rows_second_opinion(eng, sig: np.ndarray, lens: np.ndarray, model, spc, conv: str = "hip", fallback: str = "device",
                               flag_truncated: bool = False, second_opinion: bool = True, with_start_peak: bool = False) -> np.ndarray:
    """detect_rows with the LLR second opinion (ADP_CNN_SECOND_LLR): a read whose row fails gets the row combined_detect_llr2
    returns for it on this batch, where that row passes (``reserved_`` bit 0 marks it; lib.rows_to_results names its primary
    columns ``llr_*``).  An extension: the reference runs one primary per configuration.  ONE library call.
    with_start_peak: the overlay of detect_rows_start_peak on the rows this call delivers, the rescued ones included.
    second_opinion: True / "llr"; or "llr_resegment" -- a read whose second opinion fails behind a first change point is segmented
    once more from that opinion's poly(A) end and validated from its adapter end (ADP_CNN_SECOND_RESEGMENT, an extension, untuned;
    ``reserved_`` bits 0 and 5-9, ``llr_detect_log`` says so); the resident and int16 entries below take the same values.
    Anything else is a ValueError (lib.second_opinion_flags)."""
    return _detect_rows(eng, sig, lens, model, spc, conv=conv, fallback=fallback, second_opinion=second_opinion, flag_truncated=flag_truncated,
                        with_start_peak=with_start_peak)


def detect_rows_device_second_opinion(eng, dsig: int, dlen: int, n: int, lens_host: np.ndarray, model, spc, minibatch: Optional[int] = None,
                                      fallback: str = "device", flag_truncated: bool = False, second_opinion: bool = True,
                                      with_start_peak: bool = False) -> np.ndarray:
    """detect_rows_device with the LLR second opinion, per minibatch as combined_detect_llr2 would see it (its normalisation is
    the minibatch's).  ONE library call over the resident batch.  with_start_peak: as detect_rows_second_opinion's."""
    return _detect_rows(eng, dsig, lens_host, model, spc, dlen, n, fallback=fallback, minibatch=minibatch, second_opinion=second_opinion,
                        flag_truncated=flag_truncated, with_start_peak=with_start_peak)


def detect_rows_device_i16(eng, draw: int, dlen: int, dscale: int, doffset: int, n: int, lens_host: np.ndarray, model, spc,
                           minibatch: Optional[int] = None, with_start_peak: bool = False, second_opinion: bool = False,
                           fallback: str = "device", conv: str = "hip") -> np.ndarray:
    """detect_rows_device over RAW int16 samples resident on the device (draw int16 [n, m], dscale / doffset float32 [n], dlen
    int32 [n]: pointers): the CNN primary reads the ADC samples itself (adp_detect_cnn_i16) -- no float32 matrix is made -- with
    the short-read fallback on the device where the configuration has it, and the two options as
    detect_rows_device_second_opinion has them.  The rows are those of calibrate_i16 + that function, byte for byte.  ONE library
    call: there is no host-fallback and no torch-conv form (and no truncation look: that phase reads float32 rows)."""
    return _detect_rows(eng, draw, lens_host, model, spc, dlen, n, (dscale, doffset), conv=conv, fallback=fallback, minibatch=minibatch,
                        second_opinion=second_opinion, with_start_peak=with_start_peak)


def combined_detect_cnn_llr(batch_of_signals: np.ndarray, full_signal_lens: np.ndarray, model, spc, device: int = 0,
                            flag_truncated: bool = False, with_start_peak: bool = False, second_opinion="llr") -> List[DetectResults]:
    """combined_detect_cnn, and for the reads it fails combined_detect_llr2 on the same batch where that passes (an extension;
    such results carry ``llr_adapter_end`` / ``llr_polya_end`` instead of the ``cnn_*`` pair).  Always a list.
    with_start_peak: as combined_detect_cnn's.  second_opinion: "llr", or "llr_resegment" as detect_rows_second_opinion takes it."""
    from .combined import _as_batch, get_engine

    sig, lens = _as_batch(batch_of_signals, full_signal_lens)
    n, m = sig.shape
    if n == 0:
        return []
    eng = get_engine(spc, n, m, device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        rows = _detect_rows(eng, sig, lens, model, spc, second_opinion=second_opinion, flag_truncated=flag_truncated, with_start_peak=with_start_peak)
    return lib.rows_to_results(rows, "cnn", consume=True)


def combined_detect_cnn(batch_of_signals: np.ndarray, full_signal_lens: np.ndarray, model, spc,
                        device: int = 0, conv: str = "hip", flag_truncated: bool = False,
                        with_start_peak: bool = False) -> Union[List[DetectResults], DetectResults]:
    """model: the nn.Sequential of load_cnn_model, a dict of weight arrays (load_cnn_weights), or None (the config's model).
    flag_truncated: as combined_detect_llr2's (an extension, off by default).
    with_start_peak: the ``start_peak_*`` fields of detect_rna_start_peak on every result, as combined_detect_llr2's option of
    that name fills them (an extension, off by default: the reference keeps one primary per run); conv must be "hip"."""
    from .combined import _as_batch, get_engine

    host_forms = not (flag_truncated or with_start_peak)
    _refuse_host_forms(conv, "device", with_start_peak, host_forms)  # (here as well: before an engine is made)
    sig, lens = _as_batch(batch_of_signals, full_signal_lens)
    n, m = sig.shape
    eng = get_engine(spc, n, m, device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        rows = _detect_rows(eng, sig, lens, model, spc, conv=conv, flag_truncated=flag_truncated, with_start_peak=with_start_peak,
                            host_forms=host_forms)
    res = lib.rows_to_results(rows, "cnn", consume=True)
    return res if len(res) > 1 else res[0]
