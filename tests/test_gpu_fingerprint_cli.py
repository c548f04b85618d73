"""`adapted detect --fingerprints E [--barcode_templates FILE.npz] [--dtw_band R]` end to end on the GPU: every other file of a run
stays byte for byte what a run without the option writes; fingerprints/fingerprints_<k>.npz and fingerprints/barcodes_<k>.csv hold,
per passing read, what the oracle (tests/fingerprint_oracle.py) gives on that read's bounds; combined with --polya_length events the
polya_length files are those of a run with that option alone."""
import os

import numpy as np
import pandas as pd
import pytest

import events_oracle as eo
import fingerprint_oracle as fo
from test_gpu_polya_length_cli import N, _reads, _spc

pytestmark = pytest.mark.gpu
E, BAND = 24, 3


def _files(run_root):
    runs = [d for d in os.listdir(run_root) if d.startswith("adapted_")]
    assert len(runs) == 1, runs
    out = {}
    for sub in ("boundaries", "failed_reads", "polya_length", "fingerprints"):
        d = os.path.join(run_root, runs[0], sub)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            with open(os.path.join(d, f), "rb") as fh:
                out[sub + "/" + f] = fh.read()
    return out, os.path.join(run_root, runs[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from adapted_amd import fingerprint as fpm
    from adapted_amd import main as cli

    tmp = tmp_path_factory.mktemp("fingerprint_cli")
    spc = _spc()
    sig, lens = _reads(spc.sig_preload_size)
    ids = np.array(["read_%04d" % i for i in range(N)], dtype=object)
    np.savez(tmp / "reads_0.npz", signals=sig, full_lengths=lens, read_ids=ids)
    cfg = str(tmp / "cfg.toml")
    spc.to_toml(cfg)
    out = {}

    def run(name, extra):
        cli.main(["detect", "-i", str(tmp / "reads_0.npz"), "-o", str(tmp / name), "--config", cfg, "-s", str(N), "-b", "24"] + extra)
        out[name] = _files(str(tmp / name))

    run("plain", [])
    run("fp", ["--fingerprints", str(E)])
    # templates: three fingerprints of the first file of that run
    with np.load(os.path.join(out["fp"][1], "fingerprints", "fingerprints_0.npz")) as z:
        pick = [i for i in range(len(z["count"])) if z["status"][i] == 0][:3]
        tm = fpm.Templates(["bcA", "bcB", "bcC"], z["fingerprints"][pick], z["count"][pick])
    assert len(pick) == 3
    fpm.save_templates(str(tmp / "templates.npz"), tm)
    run("polya", ["--polya_length", "events"])
    run("both", ["--fingerprints", str(E), "--barcode_templates", str(tmp / "templates.npz"), "--dtw_band", str(BAND), "--polya_length", "events"])
    return sig, ids, out, tm


def test_the_option_leaves_the_other_files_as_they_are(runs):
    _, _, out, _ = runs
    plain, polya = out["plain"][0], out["polya"][0]
    assert not any(f.startswith("fingerprints/") for f in plain) and any(f.startswith("boundaries/") for f in plain)
    fp, both = out["fp"][0], out["both"][0]
    assert {f: v for f, v in fp.items() if not f.startswith("fingerprints/")} == plain
    assert {f: v for f, v in both.items() if not f.startswith("fingerprints/")} == polya  # the polya_length files too
    ks = sorted(f.split("_")[-1].split(".")[0] for f in plain if f.startswith("boundaries/"))
    assert sorted(f for f in fp if f.startswith("fingerprints/")) == sorted("fingerprints/fingerprints_%s.npz" % k for k in ks)
    assert sorted(f for f in both if f.startswith("fingerprints/")) == sorted(
        ["fingerprints/fingerprints_%s.npz" % k for k in ks] + ["fingerprints/barcodes_%s.csv" % k for k in ks])


def test_the_files_equal_the_oracle_on_the_rows_bounds(runs):
    from adapted_amd.main import BARCODE_COLUMNS

    sig, ids, out, tm = runs
    row_of = {str(rid): i for i, rid in enumerate(ids)}
    t, tc = np.where(np.isnan(tm.levels), 0.0, tm.levels), tm.counts
    total = selected = 0
    for name in ("fp", "both"):
        files, run_dir = out[name]
        for k in sorted(int(f.split("_")[-1].split(".")[0]) for f in files if f.startswith("boundaries/")):
            bd = pd.read_csv(os.path.join(run_dir, "boundaries", "detected_boundaries_%d.csv" % k))
            with np.load(os.path.join(run_dir, "fingerprints", "fingerprints_%d.npz" % k)) as z:
                got = {key: z[key] for key in z.files}
            assert sorted(got) == ["count", "fingerprints", "lengths", "levels", "read_id", "status"]
            assert got["read_id"].tolist() == bd["read_id"].tolist()  # one entry per passing read, in the CSV's order
            want = []
            for _, b in bd.iterrows():
                x = sig[row_of[b["read_id"]], int(b["adapter_start"]):int(b["adapter_end"])]
                assert not eo.has_close_ties(x, 8, 8, 16.0, 1e-3)
                want.append(fo.levels(x, E))
            assert fo.same(got["count"], np.asarray([o["count"] for o in want], dtype=np.int32))
            assert fo.same(got["status"], np.asarray([o["status"] for o in want], dtype=np.int32))
            assert fo.same(got["lengths"], np.stack([o["lengths"] for o in want]))
            assert fo.same(got["levels"], np.stack([o["levels"] for o in want]))
            assert fo.same(got["fingerprints"], np.stack([o["fp"] for o in want]))
            assert all(o["status"] == 0 and o["nk"] > 20 for o in want)  # (staircase adapters: tests/test_gpu_polya_length_cli.py)
            selected += sum(o["nk"] > E - 1 for o in want)
            total += len(want)
            if name == "both":
                bc = pd.read_csv(os.path.join(run_dir, "fingerprints", "barcodes_%d.csv" % k), float_precision="round_trip")
                assert list(bc.columns) == BARCODE_COLUMNS and bc["read_id"].tolist() == bd["read_id"].tolist()
                best, bdist = fo.assign(fo.dtw(np.stack([o["fp"] for o in want]), [o["count"] for o in want], t, tc, BAND))
                assert bc["n_events"].tolist() == [o["count"] for o in want]
                assert bc["barcode"].tolist() == [tm.names[i] for i in best[:, 0]]
                assert bc["barcode_second"].tolist() == [tm.names[i] for i in best[:, 1]]
                assert fo.same(bc["dtw_dist"].to_numpy(dtype=np.float64), bdist[:, 0].copy())
                assert fo.same(bc["dtw_dist_second"].to_numpy(dtype=np.float64), bdist[:, 1].copy())
                assert fo.same(bc["dtw_margin"].to_numpy(dtype=np.float64), bdist[:, 1] - bdist[:, 0])
                if k == 0:
                    assert (bc["dtw_dist"] == 0.0).sum() >= 3  # the templates' own reads
    assert total >= 64 and selected >= 8  # (some adapters have more than E - 1 boundaries: the selection ran)
