"""The host side of the validation from a given adapter start and of the re-validating adapter-front pass
(include/adapted_hip_revalidate.h, adapted_amd/adapter_front.py, `adapted detect --adapter_front --adapter_front_revalidate`),
without a GPU: the header against its prototype table, the parameters, the command line's refusals, the pinned signatures, the
pipeline's and the public validator's wiring with recording engines, the Engine's handling of open-pore lists, and what the golden
case list reaches."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import revalidate_cases as R
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["adp_adapter_front_revalidate", "adp_adapter_front_revalidate_i16", "adp_validate_candidates_from"]


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(os.path.join(ROOT, "include", "adapted_hip_revalidate.h"))
    assert sorted(declared) == sorted(lib.REVALIDATE_PROTOTYPES) == NAMES
    others = (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES) | set(lib.EVENT_PROTOTYPES)
              | set(lib.FINGERPRINT_PROTOTYPES) | set(lib.ADAPTER_FRONT_PROTOTYPES) | set(lib.EXPORTS))
    assert not set(lib.REVALIDATE_PROTOTYPES) & others
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_revalidate.h"') == 1
    assert text.index('#include "adapted_hip_adapter_front.h"') < text.index('#include "adapted_hip_revalidate.h"') < text.index("adp_set_profiling")
    with open(os.path.join(ROOT, "include", "adapted_hip_revalidate.h")) as fh:
        own = fh.read()
    assert re.search(r"^#define\s+ADP_ROW_REVALIDATED\s+16\s*$", own, re.M) and lib.ROW_REVALIDATED == 16
    assert lib.ROW_REVALIDATED & (lib.ROW_FROM_SECOND_LLR | lib.ROW_POLYA_TRUNCATED | lib.ROW_TRUNC_LOOKED | lib.ROW_ADAPTER_FRONT) == 0
    L = lib.load()
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.REVALIDATE_PROTOTYPES[name].split(":")
        assert got_ret == ret and got_params.split() == params, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
    # the new forms are the plain ones with reval_out behind them; the validation takes the starts behind the bounds
    for plain, new in (("adp_adapter_front", NAMES[0]), ("adp_adapter_front_i16", NAMES[1])):
        assert lib.REVALIDATE_PROTOTYPES[new].split() == lib.ADAPTER_FRONT_PROTOTYPES[plain].split() + ["int32*"]
    v, f = lib.PROTOTYPES["adp_validate_candidates"].split(), lib.REVALIDATE_PROTOTYPES[NAMES[2]].split()
    assert f == v[:7] + ["int64*"] + v[7:]
    # a null handle is refused by all three
    a = lib.AdpAdapterFrontArgs(20.0, 90.0, 100, 2500, 1000, 0)
    rows = lib.empty_rows(1)
    info, i64, f64, rv = np.zeros((1, 4), dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(1), np.zeros((1, 2), dtype=np.int32)
    sig, lens = np.zeros((1, 8), dtype=np.float32), np.zeros(1, dtype=np.int32)
    assert L.adp_adapter_front_revalidate(None, sig, lens, 1, 8, rows, ctypes.byref(a), 0, info, i64, i64, f64, rv) == -1
    assert L.adp_adapter_front_revalidate_i16(None, None, None, None, None, 1, 8, rows, ctypes.byref(a), 1, info, i64, i64, f64, rv) == -1
    assert L.adp_validate_candidates_from(None, sig, lens, 1, 8, np.zeros((1, 2), dtype=np.int64), i64, 1, 0, rows) == -1
    assert L.adp_validate_candidates_from(None, sig, lens, 1, 8, np.zeros((1, 2), dtype=np.int64), None, 1, 0, rows) == -1
    with pytest.raises(ctypes.ArgumentError):  # int32 for int64 *starts
        L.adp_validate_candidates_from(None, sig, lens, 1, 8, np.zeros((1, 2), dtype=np.int64), lens, 1, 0, rows)


def test_params_defaults_parse_and_pad():
    from adapted_amd import adapter_front as af

    p = af.AdapterFrontParams()
    assert p.revalidate is False and [f for f in p.__dataclass_fields__][-1] == "revalidate"
    assert af.AdapterFrontParams(16, 64, 5.0, 91.5, 32) == af.AdapterFrontParams(16, 64, 5.0, 91.5, 32, False)
    a = af.AdapterFrontParams(16, 64, 5.0, 91.5, 32, True).args()
    assert (a.window, a.min_obs_adapter, a.min_shift, a.min_pA_current, a.min_adapter_len, a.pad) == (16, 64, 5.0, 91.5, 32, 0)
    assert af.AdapterFrontParams.parse("50,1200,12.5,100", min_adapter_len=7) == af.AdapterFrontParams(50, 1200, 12.5, 100.0, 7)
    assert af.AdapterFrontParams.parse("50,1200,12.5,100", min_adapter_len=7, revalidate=True) == af.AdapterFrontParams(50, 1200, 12.5, 100.0, 7, True)
    doc = af.__doc__.lower()
    assert "untuned" in doc and "not repeated" in doc and "revalidate" in doc and "rejected" in doc
    # what the re-validating form needs, said before the library is entered
    rows = np.zeros(2, dtype=af.lib.ROW_DTYPE)
    sig = np.zeros((2, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="engine"):
        af.adapter_front_rows(sig, np.zeros(2, dtype=np.int32), rows, af.AdapterFrontParams(min_adapter_len=5, revalidate=True))
    with pytest.raises(ValueError, match="min_adapter_len"):
        af.adapter_front_rows(sig, np.zeros(2, dtype=np.int32), rows, af.AdapterFrontParams(revalidate=True), engine=object())
    with pytest.raises(ValueError, match="host rows"):
        af.adapter_front_rows(4096, 4096, 8192, af.AdapterFrontParams(min_adapter_len=5, revalidate=True), n=2, m=8, engine=object())
    out = af.adapter_front_rows(np.zeros((0, 8), dtype=np.float32), None, np.zeros(0, dtype=af.lib.ROW_DTYPE),
                                af.AdapterFrontParams(min_adapter_len=5, revalidate=True), engine=object())
    assert len(out) == 6 and out[5].shape == (0, 2) and out[5].dtype == np.int32

    calls = []

    class Eng:
        def adapter_front_revalidate(self, sig, lens, rows, args, n=None, m=None):
            calls.append(("f32", lens is not None, n, m, args.min_adapter_len))
            return "info", "shift", "cand", "diff", "reval"

        def adapter_front_revalidate_i16(self, raw, dlen, scale, offset, rows, args, n, m=None):
            calls.append(("i16", raw, dlen, scale, offset, n, m))
            return "info", "shift", "cand", "diff", "reval"

    p = af.AdapterFrontParams(min_adapter_len=5, revalidate=True)
    out = af.adapter_front_rows(sig, np.zeros(2, dtype=np.int32), rows, p, engine=Eng())
    assert out[1:] == ("info", "shift", "cand", "diff", "reval") and out[0] is not rows
    af.adapter_front_rows(4096, 8, rows, p, n=2, m=8, calibration=(16, 24), engine=Eng())
    assert calls == [("f32", True, 2, None, 5), ("i16", 4096, 8, 16, 24, 2, 8)]


def test_cli_options_and_refusals(tmp_path):
    from adapted_amd import main
    from adapted_amd.config import get_chemistry_specific_config

    base = ["detect", "-i", str(tmp_path / "none.npz"), "-o", str(tmp_path)]
    args = main.build_parser().parse_args(base + ["-c", "RNA004"])
    assert args.adapter_front_revalidate is False
    args = main.build_parser().parse_args(base + ["-c", "RNA004", "--adapter_front"])
    assert main._check_adapter_front(args).revalidate is False
    args = main.build_parser().parse_args(base + ["-c", "RNA004", "--adapter_front", "--adapter_front_revalidate", "--adapter_front_params", "16,64,20,90"])
    p = main._check_adapter_front(args)
    assert p.revalidate is True and (p.window, p.min_obs_adapter) == (16, 64)
    overwrite = str(tmp_path / "overwrite.toml")
    spc = get_chemistry_specific_config("RNA004")
    spc.mvs_polya.mvs_detect_overwrite = True
    spc.to_toml(overwrite)
    for extra, say in ((["-c", "RNA004", "--adapter_front_revalidate"], "--adapter_front_revalidate goes with --adapter_front"),
                       (["--config", overwrite, "--adapter_front", "--adapter_front_revalidate"], "mvs_detect_overwrite")):
        with pytest.raises(SystemExit) as e:
            main.main(base + extra)
        assert say in str(e.value), (extra, e.value)
    assert not [d for d in os.listdir(tmp_path) if d.startswith("adapted_")]


def test_signatures_keep_their_pinned_tails():
    from adapted_amd import lib, main
    from adapted_amd.adapter_front import AdapterFrontParams

    params = list(inspect.signature(main.run_detect).parameters)
    assert params[-4:] == ["fingerprints", "polya_length", "adapter_nt", "event_params"] and params[-5] == "adapter_front"
    assert "adapter_front_revalidate" not in params
    assert list(inspect.signature(lib.Engine.adapter_front).parameters) == ["self", "sig", "full_lens", "rows", "args", "n", "m"]
    assert list(inspect.signature(lib.Engine.validate_rows).parameters) == ["self", "signals", "full_lens", "n", "bounds", "device_ptrs", "topk_none",
                                                                            "polya_truncated"]
    assert list(inspect.signature(lib.Engine.validate_rows_from).parameters)[:6] == ["self", "signals", "full_lens", "n", "bounds", "starts"]
    assert list(inspect.signature(lib.Engine.adapter_front_revalidate).parameters) == list(inspect.signature(lib.Engine.adapter_front).parameters)
    assert list(inspect.signature(lib.Engine.adapter_front_revalidate_i16).parameters) == list(inspect.signature(lib.Engine.adapter_front_i16).parameters)
    assert list(inspect.signature(AdapterFrontParams.parse).parameters) == ["text", "min_adapter_len", "revalidate"]


def test_pipeline_takes_the_revalidating_forms_only_when_asked():
    from adapted_amd import lib, pipeline
    from adapted_amd.adapter_front import AdapterFrontParams
    from adapted_amd.config import get_chemistry_specific_config

    calls = []

    class Eng:
        def adapter_front(self, sig, full_lens, rows, args, n=None, m=None):
            calls.append(("f32", sig, full_lens, n, m))
            return np.zeros((n, 4), dtype=np.int32), None, None, None

        def adapter_front_i16(self, raw, dlen, scale, offset, rows, args, n, m=None):
            calls.append(("i16", raw, dlen, scale, offset, n, m))
            return np.zeros((n, 4), dtype=np.int32), None, None, None

        def adapter_front_revalidate(self, sig, full_lens, rows, args, n=None, m=None):
            calls.append(("f32r", sig, full_lens, n, m, args.min_adapter_len))
            info = np.asarray([[0, 0, 0, 1], [0, 0, 0, 0]] + [[-1, 0, 0, 0]] * (n - 2), dtype=np.int32)
            return info, None, None, None, np.asarray([[1, 0], [0, 2]] + [[-1, 0]] * (n - 2), dtype=np.int32)

        def adapter_front_revalidate_i16(self, raw, dlen, scale, offset, rows, args, n, m=None):
            calls.append(("i16r", raw, dlen, scale, offset, n, m))
            return np.zeros((n, 4), dtype=np.int32), None, None, None, np.asarray([[0, 4]] + [[-1, 0]] * (n - 1), dtype=np.int32)

    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.primary, p.spc = "llr", get_chemistry_specific_config("RNA004")
    with pytest.raises(ValueError, match="min_adapter_len"):
        p.enable_adapter_front(AdapterFrontParams(revalidate=True))
    p.spc.mvs_polya.mvs_detect_overwrite = True
    with pytest.raises(ValueError, match="mvs_detect_overwrite"):
        p.enable_adapter_front(AdapterFrontParams(min_adapter_len=1000, revalidate=True))
    p.spc.mvs_polya.mvs_detect_overwrite = False
    p.m, p.eng, p.native_i16, p._resident, p._resident_i16 = 100, Eng(), False, 4096, (8192, 1, 2, 3)
    p.slots = [None, {"dl": 555}]
    rows = lib.empty_rows(3)
    p.enable_adapter_front(AdapterFrontParams(min_adapter_len=1000))
    assert p.front_revalidate is False
    p._adapter_front(1, 3, rows)
    p.native_i16 = True
    p._adapter_front(1, 2, rows[:2])
    assert calls == [("f32", 4096, None, 3, 100), ("i16", 8192, 1, 2, 3, 2, 100)]  # (today's calls)
    del calls[:]
    p.enable_adapter_front(AdapterFrontParams(min_adapter_len=1000, revalidate=True))
    assert p.front_revalidate is True and (p.front_patched, p.front_rejected) == (0, 0)
    p.native_i16 = False
    assert p._adapter_front(1, 3, rows) is rows and (p.front_patched, p.front_rejected) == (1, 1)
    p.native_i16 = True
    p._adapter_front(1, 2, rows[:2])
    assert calls == [("f32r", 4096, 555, 3, 100, 1000), ("i16r", 8192, 1, 2, 3, 2, 100)] and (p.front_patched, p.front_rejected) == (1, 2)
    src = inspect.getsource(pipeline.HostPipeline.run)
    assert src.index("self._adapter_front(j, n, rows)") < src.index("self._adapter_fingerprints(j, n, rows, mbs)") < src.index("self._adapter_events(j, n, rows, mbs)")


def test_public_validator_passes_the_start_on(monkeypatch):
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.container_types import Boundaries
    from adapted_amd.detect import combined

    calls = []

    class Eng:
        def validate_rows(self, sig, lens, n, b, topk_none=False, polya_truncated=False):
            calls.append(("plain", b.tolist(), topk_none, polya_truncated))
            return lib.empty_rows(1)

        def validate_rows_from(self, sig, lens, n, b, starts, topk_none=False, polya_truncated=False):
            calls.append(("from", b.tolist(), starts.tolist(), str(starts.dtype), topk_none, polya_truncated))
            return lib.empty_rows(1)

    monkeypatch.setattr(combined, "get_engine", lambda spc, n, m, device: Eng())
    spc = get_chemistry_specific_config("RNA004")
    spc.update_primary_method()
    spc.update_sig_preload_size()
    x = np.zeros(5000, dtype=np.float32)
    for start in (None, 0, 789):
        combined.validate_boundaries(x, Boundaries(adapter_start=start, adapter_end=3000, polya_end=4000, polya_end_topk=[4000, 3900]), spc, 5000)
    combined.validate_boundaries(x, Boundaries(adapter_start=5, adapter_end=3000, polya_end=4000, polya_end_topk=None, polya_truncated=True), spc, 5000)
    assert calls == [("plain", [[3000, 4000, 3900]], False, False)] * 2 + [("from", [[3000, 4000, 3900]], [789], "int64", False, False),
                                                                           ("from", [[3000, 4000]], [5], "int64", True, True)]


def test_engine_attaches_the_lists_of_replaced_rows_only():
    from adapted_amd import lib

    n = 4
    rows = lib.empty_rows(n)
    rows["n_open_pores"] = (20, 18, 3, 17)
    old = [lib.register_open_pores(np.arange(k)) for k in (20, 18)] + [-1, lib.register_open_pores(np.arange(17))]
    rows["open_pores_more"] = old
    arena = np.arange(100, 160, dtype=np.int32)
    seen = []

    def revalidate(h, sig, lens, nn, m, rr, args, flags, info, shift, cand, diff, reval):
        seen.append((nn, m, flags, lens.dtype.name))
        reval[:] = [[1, 0], [0, 2], [1, 0], [-1, 0]]
        rr["n_open_pores"][0], rr["open_pores_more"][0] = 19, 7  # replaced: an offset into this call's arena
        rr["n_open_pores"][2], rr["open_pores_more"][2] = 21, 30  # replaced, and its first row had a short list
        return 0

    def arena_fn(h, out, cap, used):
        used[0] = arena.size
        if out is not None:
            out[:] = arena
        return 0

    class L:
        adp_adapter_front_revalidate = staticmethod(revalidate)
        adp_open_pores_arena = staticmethod(arena_fn)

    eng = lib.Engine.__new__(lib.Engine)
    eng._h, eng.m, eng.lib = lib._VoidP(), 8, L
    sig = np.zeros((n, 8), dtype=np.float32)
    out = eng.adapter_front_revalidate(sig, [8, 8, 8, 8], rows, lib.AdpAdapterFrontArgs(20.0, 90.0, 16, 64, 5, 0))
    assert len(out) == 5 and out[4][:, 0].tolist() == [1, 0, 1, -1] and seen == [(n, 8, 0, "int32")]
    # rows 1 and 3 keep their tokens and their lists; rows 0 and 2 have new tokens for lists out of the arena; row 0's old list left
    assert rows["open_pores_more"][[1, 3]].tolist() == [old[1], old[3]]
    assert lib._OPEN_PORES_MORE[old[1]].size == 18 and lib._OPEN_PORES_MORE[old[3]].size == 17 and old[0] not in lib._OPEN_PORES_MORE
    t0, t2 = int(rows["open_pores_more"][0]), int(rows["open_pores_more"][2])
    assert t0 not in old and t2 not in old and t0 != t2
    assert lib._OPEN_PORES_MORE[t0].tolist() == arena[7:26].tolist() and lib._OPEN_PORES_MORE[t2].tolist() == arena[30:51].tolist()
    for t in (old[1], old[3], t0, t2):
        lib._OPEN_PORES_MORE.pop(t)
    with pytest.raises(ValueError, match="host rows"):
        eng.adapter_front_revalidate(sig, [8] * n, 4096, lib.AdpAdapterFrontArgs())
    with pytest.raises(ValueError, match="full_lens"):  # (the library copies n lengths: a shorter array never reaches it)
        eng.adapter_front_revalidate(sig, [8] * (n - 1), rows, lib.AdpAdapterFrontArgs())


@pytest.mark.parametrize("chem", R.CHEMS)
def test_golden_case_list_reaches_what_it_must(chem):
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config(chem)
    sigs, bounds, starts, lens, rows, ref0 = R.load(chem)
    assert len(sigs) == len(R.CASES) == len(rows) and (starts > 0).all()
    # the stored inputs are the cases'
    for c, x, b, s, fl in zip(R.CASES, sigs, bounds, starts, lens):
        bx, bb, bs, bfl = R.build(c)
        assert (bs, bfl) == (s, fl) and bb.tolist() == b.tolist() and bx.view(np.uint32).tobytes() == x.view(np.uint32).tobytes(), c["name"]
    cov = R.coverage(sigs, bounds, starts, lens, rows, ref0, mean_window=spc.real_range.mean_window,
                     max_obs_local_range=spc.real_range.max_obs_local_range, var_hi=spc.mvs_polya.pA_var_range[1],
                     mean_scale_lo=spc.mvs_polya.pA_mean_adapter_med_scale_range[0])
    missing = [k for k in R.REQUIRED if k not in cov]
    assert not missing, missing
    for fn in ("revalidate_signals.npz", "revalidate_%s.npz" % chem):
        assert os.path.getsize(os.path.join(R.GOLD, fn)) < 1 << 20
