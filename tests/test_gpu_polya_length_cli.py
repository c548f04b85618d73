"""`adapted detect --polya_length {events,adapter}` end to end on the GPU: the boundaries and failed-reads files stay byte for byte
what a run without the option writes, and polya_length/polya_length_<k>.csv holds, per passing read, what the segmentation's oracle
(tests/events_oracle.py) and estimate_polya_length give on that read's bounds."""
import os

import numpy as np
import pandas as pd
import pytest

import events_oracle as eo

pytestmark = pytest.mark.gpu
N = 64


def _spc():
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect = True
    spc.cnn_boundaries.cnn_detect = False
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


def _reads(m):
    """64 synthetic reads whose adapters are staircases (levels N(80, 7^2), dwell uniform in [20, 40]) under the read's own
    noise scaled to sd 1.5; the start-peak and open-pore decorations keep their levels"""
    from adapted_amd import synth

    sig, lens = synth.synth_batch(11, 0, N, m)
    rng = np.random.default_rng(5)
    for k in range(N):
        a_len, _, flags, sp_start, op_start = synth.read_params(11, k)
        mean = np.full(a_len, 80.0, dtype=np.float32)
        level = np.repeat(rng.normal(80.0, 7.0, size=a_len // 20 + 2), rng.integers(20, 41, size=a_len // 20 + 2))[:a_len]
        if flags & synth.FLAG_START_PEAK:
            mean[sp_start:sp_start + synth.SP_LEN] = 150.0
            level[sp_start:sp_start + synth.SP_LEN] = 150.0
        if flags & synth.FLAG_OPEN_PORE:
            mean[op_start:op_start + synth.OP_LEN] = 230.0
            level[op_start:op_start + synth.OP_LEN] = 230.0
        noise = (sig[k, :a_len] - mean).astype(np.float64) * (1.5 / 7.0)
        sig[k, :a_len] = (level + noise).astype(np.float32)
    return sig, lens


def _files(run_root):
    runs = [d for d in os.listdir(run_root) if d.startswith("adapted_")]
    assert len(runs) == 1, runs
    out = {}
    for sub in ("boundaries", "failed_reads", "polya_length"):
        d = os.path.join(run_root, runs[0], sub)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            with open(os.path.join(d, f), "rb") as fh:
                out[sub + "/" + f] = fh.read()
    return out, os.path.join(run_root, runs[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory, oracle_mod):
    from adapted_amd import main as cli

    tmp = tmp_path_factory.mktemp("polya_length_cli")
    spc = _spc()
    m = spc.sig_preload_size
    sig, lens = _reads(m)
    # the precondition, on the CPU oracle: at least half of the reads pass detect
    n_pass = sum(bool(r["success"]) for r in oracle_mod.detect_llr(sig, lens, spc))
    assert n_pass >= 32, n_pass
    ids = np.array(["read_%04d" % i for i in range(N)], dtype=object)
    np.savez(tmp / "reads_0.npz", signals=sig, full_lengths=lens, read_ids=ids)
    cfg = str(tmp / "cfg.toml")
    spc.to_toml(cfg)
    out = {}
    for name, extra in (("plain", []), ("events", ["--polya_length", "events"]), ("adapter", ["--polya_length", "adapter", "--adapter_nt", "60"])):
        cli.main(["detect", "-i", str(tmp / "reads_0.npz"), "-o", str(tmp / name), "--config", cfg, "-s", str(N), "-b", "24"] + extra)
        out[name] = _files(str(tmp / name))
    return sig, ids, out


def _frames(files, run_dir):
    """[(k, the boundaries frame, the polya_length frame)] of a run"""
    ks = sorted(int(f.split("_")[-1].split(".")[0]) for f in files if f.startswith("boundaries/"))
    return [(k, pd.read_csv(os.path.join(run_dir, "boundaries", "detected_boundaries_%d.csv" % k)),
             pd.read_csv(os.path.join(run_dir, "polya_length", "polya_length_%d.csv" % k))) for k in ks]


def test_the_option_leaves_the_existing_files_as_they_are(runs):
    _, _, out = runs
    plain = out["plain"][0]
    assert not any(f.startswith("polya_length/") for f in plain) and any(f.startswith("boundaries/") for f in plain)
    for name in ("events", "adapter"):
        got = out[name][0]
        assert {f: v for f, v in got.items() if not f.startswith("polya_length/")} == plain, name
        assert sorted(f.split("_")[-1] for f in got if f.startswith("polya_length/")) == sorted(f.split("_")[-1] for f in got if f.startswith("boundaries/"))


def test_events_method_equals_the_oracle_on_the_rows_bounds(runs):
    from adapted_amd.main import POLYA_LENGTH_COLUMNS
    from adapted_amd.polya_length import estimate_polya_length

    sig, ids, out = runs
    files, run_dir = out["events"]
    row_of = {str(rid): i for i, rid in enumerate(ids)}
    total = 0
    for k, bd, pl in _frames(files, run_dir):
        assert list(pl.columns) == POLYA_LENGTH_COLUMNS
        assert pl["read_id"].tolist() == bd["read_id"].tolist()  # one line per passing read, in the file's order
        total += len(pl)
        for (_, b), (_, p) in zip(bd.iterrows(), pl.iterrows()):
            a_s, a_e, p_e = int(b["adapter_start"]), int(b["adapter_end"]), int(b["polya_end"])
            bounds, status, med, mad = eo.segment(sig[row_of[b["read_id"]], a_s:a_e])
            assert status == 0 and not eo.has_close_ties(sig[row_of[b["read_id"]], a_s:a_e], 8, 8, 16.0, 1e-3)
            nt, spn = estimate_polya_length([a_s], [a_e], [p_e], method="events", event_len_med=[med])
            assert (int(p["adapter_len"]), int(p["polya_len"]), int(p["n_events"])) == (a_e - a_s, p_e - a_e, bounds.size - 1)
            for col, want in (("event_len_med", med), ("event_len_mad", mad), ("samples_per_nt", spn[0]), ("polya_nt", nt[0])):
                assert float(p[col]) == float(np.round(want, 3)), (b["read_id"], col, p[col], want)
            assert bounds.size > 20 and 20 <= med <= 45, (bounds.size, med)  # (a staircase of dwells in [20, 40] was found)
            assert pd.isna(p["polya_truncated"])  # (no --flag_truncated: the rows carry no flag)
    assert total >= 32 and total == sum(len(bd) for _, bd, _ in _frames(files, run_dir))


def test_adapter_method_divides_by_the_adapters_bases(runs):
    _, _, out = runs
    files, run_dir = out["adapter"]
    ev = {k: pl for k, _, pl in _frames(*out["events"])}
    for k, bd, pl in _frames(files, run_dir):
        assert pl["read_id"].tolist() == bd["read_id"].tolist()
        alen = (bd["adapter_end"] - bd["adapter_start"]).to_numpy(dtype=np.float64)
        assert pl["adapter_len"].tolist() == alen.tolist()
        assert pl["samples_per_nt"].tolist() == np.round(alen / 60.0, 3).tolist()
        plen = (bd["polya_end"] - bd["adapter_end"]).to_numpy(dtype=np.float64)
        assert pl["polya_nt"].tolist() == np.round(plen / (alen / 60.0), 3).tolist()
        for col in ("n_events", "event_len_med", "event_len_mad"):  # the segmentation's columns do not depend on the method
            assert pl[col].tolist() == ev[k][col].tolist()
