"""`adapted detect --fingerprints E`, then `adapted templates`, then `adapted detect --barcode_templates` end to end on the GPU: the
template file is what barcode_templates.dba_templates gives from Python, which is what the oracle (tests/dtw_align_oracle.py) gives;
the third run's barcodes are fingerprint.assign_barcodes' on those templates.  And DBA on warped noisy copies, where the oracle's
inertia falls."""
import os

import numpy as np
import pandas as pd
import pytest

import dtw_align_oracle as do
from test_gpu_polya_length_cli import N, _reads, _spc

pytestmark = pytest.mark.gpu
E, BAND, ITERS, SAMPLE = 16, 2, 3, 8
SEED = 4  # (of _copies: chosen on the CPU, where the oracle's inertia falls -- test_inertia_falls_where_the_oracle_says_so checks it first)


def _run_dir(root):
    runs = [d for d in os.listdir(root) if d.startswith("adapted_")]
    assert len(runs) == 1, runs
    return os.path.join(root, runs[0])


def _fingerprints(run_dir):
    ids, fps, counts, status = [], [], [], []
    d = os.path.join(run_dir, "fingerprints")
    for k in sorted(int(f.split("_")[-1].split(".")[0]) for f in os.listdir(d) if f.startswith("fingerprints_")):
        with np.load(os.path.join(d, "fingerprints_%d.npz" % k)) as z:
            ids += [str(s) for s in z["read_id"]]
            fps.append(z["fingerprints"])
            counts.append(z["count"])
            status.append(z["status"])
    return ids, np.concatenate(fps), np.concatenate(counts), np.concatenate(status)


@pytest.fixture(scope="module")
def three_commands(tmp_path_factory):
    from adapted_amd import main as cli

    tmp = tmp_path_factory.mktemp("templates_cli")
    spc = _spc()
    sig, lens = _reads(spc.sig_preload_size)
    np.savez(tmp / "reads_0.npz", signals=sig, full_lengths=lens, read_ids=np.array(["read_%04d" % i for i in range(N)], dtype=object))
    cfg = str(tmp / "cfg.toml")
    spc.to_toml(cfg)
    detect = ["detect", "-i", str(tmp / "reads_0.npz"), "--config", cfg, "-s", str(N), "-b", "24", "--fingerprints", str(E)]
    cli.main(detect + ["-o", str(tmp / "first")])
    first = _run_dir(str(tmp / "first"))
    ids, fp, counts, status = _fingerprints(first)
    assert len(ids) >= 48 and (status == 0).all()
    # labels: three barcodes over the passing reads, two reads left out, one line for a read that did not pass
    labels = {rid: "bc%d" % (i % 3) for i, rid in enumerate(ids) if i not in (4, 9)}
    with open(tmp / "labels.csv", "w") as fh:
        fh.write("read_id,barcode\n" + "".join("%s,%s\n" % kv for kv in labels.items()) + "read_none,bc0\n")
    out = str(tmp / "templates.npz")
    cli.main(["templates", "-f", first, "-l", str(tmp / "labels.csv"), "-o", out, "--iters", str(ITERS), "--init_sample", str(SAMPLE),
              "--dtw_band", str(BAND)])
    cli.main(detect + ["-o", str(tmp / "third"), "--barcode_templates", out, "--dtw_band", str(BAND)])
    keep = [i for i, rid in enumerate(ids) if rid in labels]
    return fp[keep], counts[keep], np.asarray([labels[ids[i]] for i in keep]), out, _run_dir(str(tmp / "third"))


def test_the_template_file_is_dba_templates_which_is_the_oracle(three_commands):
    from adapted_amd import barcode_templates as bt
    from adapted_amd.fingerprint import load_templates

    fp, counts, labels, out, _ = three_commands
    got = load_templates(out)
    mine, info = bt.dba_templates(fp, counts, labels, band=BAND, iters=ITERS, init_sample=SAMPLE)
    want, winfo = bt.dba_templates(fp, counts, labels, band=BAND, iters=ITERS, init_sample=SAMPLE, align=do.align)
    assert got.names == mine.names == want.names == ["bc0", "bc1", "bc2"]
    assert do.same(got.levels, mine.levels) and do.same(mine.levels, want.levels) and got.counts.tolist() == mine.counts.tolist() == want.counts.tolist()
    assert info["iterations"] == winfo["iterations"] >= 1 and do.same(info["inertia"], winfo["inertia"]) and info["members"].tolist() == winfo["members"].tolist()
    with np.load(out, allow_pickle=False) as z:
        assert str(z["method"]) == "dba" and int(z["band"]) == BAND and int(z["iterations"]) == info["iterations"]
        assert z["members"].tolist() == info["members"].tolist() and int(z["members"].sum()) == len(labels) and do.same(z["inertia"], info["inertia"])
    # --method medoid: the start of the same build
    start, sinfo = bt.dba_templates(fp, counts, labels, band=BAND, iters=0, init_sample=SAMPLE)
    wstart, _ = bt.dba_templates(fp, counts, labels, band=BAND, iters=0, init_sample=SAMPLE, align=do.align)
    assert do.same(start.levels, wstart.levels) and sinfo["iterations"] == 0 and not do.same(start.levels, mine.levels)


def test_the_third_run_assigns_with_those_templates(three_commands):
    from adapted_amd.fingerprint import assign_barcodes, load_templates
    from adapted_amd.main import BARCODE_COLUMNS

    _, _, _, out, third = three_commands
    tm = load_templates(out)
    d = os.path.join(third, "fingerprints")
    total = 0
    for k in sorted(int(f.split("_")[-1].split(".")[0]) for f in os.listdir(d) if f.startswith("barcodes_")):
        bc = pd.read_csv(os.path.join(d, "barcodes_%d.csv" % k), float_precision="round_trip")
        with np.load(os.path.join(d, "fingerprints_%d.npz" % k)) as z:
            a = assign_barcodes(z["fingerprints"], z["count"], tm, band=BAND)
            assert bc["read_id"].tolist() == [str(s) for s in z["read_id"]]
        assert list(bc.columns) == BARCODE_COLUMNS
        assert bc["barcode"].tolist() == [tm.names[i] for i in a.best] and bc["barcode_second"].tolist() == [tm.names[i] for i in a.second]
        assert do.same(bc["dtw_dist"].to_numpy(dtype=np.float64), a.dist) and do.same(bc["dtw_dist_second"].to_numpy(dtype=np.float64), a.dist_second)
        total += len(bc)
    assert total >= 48


def _copies(seed, n_base=3, per=25, E=24):
    """warped noisy copies of three base sequences"""
    rng = np.random.default_rng(seed)
    fps, counts, labels = [], [], []
    for k in range(n_base):
        base = 2.0 * rng.standard_normal(int(rng.integers(9, 13)))
        for _ in range(per):
            x = np.repeat(base, rng.integers(1, 3, base.size))[:E]
            x = x + 0.3 * rng.standard_normal(x.size)
            row = np.full(E, np.nan)
            row[:x.size] = x
            fps.append(row)
            counts.append(x.size)
            labels.append("base%d" % k)
    return np.asarray(fps), np.asarray(counts, dtype=np.int32), np.asarray(labels)


def test_inertia_falls_where_the_oracle_says_so():
    from adapted_amd import barcode_templates as bt

    fp, counts, labels = _copies(SEED)
    want, winfo = bt.dba_templates(fp, counts, labels, iters=6, init_sample=10, align=do.align)
    first, last = winfo["inertia"][0].sum(), winfo["inertia"][-1].sum()
    assert winfo["iterations"] >= 2 and last <= first, (first, last)  # the oracle, on the CPU, before the GPU is asked
    got, info = bt.dba_templates(fp, counts, labels, iters=6, init_sample=10)
    assert do.same(got.levels, want.levels) and do.same(info["inertia"], winfo["inertia"]) and info["iterations"] == winfo["iterations"]
    assert info["inertia"][-1].sum() <= info["inertia"][0].sum() and info["members"].tolist() == [25, 25, 25]
