"""`adapted clusters` on the GPU, on a small fake run directory of fingerprints_<k>.npz files: the file it writes is a template
file, assign_barcodes on it reproduces the written clusters, and the DBA refinement is dba_templates on the written labels."""
import numpy as np
import pytest

import clusters_cases as cc
import dtw_cluster_oracle as co

pytestmark = pytest.mark.gpu


def _read_csv(path):
    with open(path) as fh:
        lines = [ln.rstrip("\n").split(",") for ln in fh]
    assert lines[0] == ["read_id", "cluster", "dtw_dist", "cluster_second", "dtw_dist_second", "dtw_margin", "in_sample", "silhouette"]
    return lines[1:]


def test_the_command_on_a_fake_run_directory(tmp_path, capsys):
    from adapted_amd import barcode_templates as bt
    from adapted_amd import clusters
    from adapted_amd import main as cli
    from adapted_amd.fingerprint import assign_barcodes, load_templates

    fp, counts, truth = cc.planted(per=15)
    fp[4, 0] = np.inf  # not usable
    counts[30] = 0
    run, ids = cc.write_run(tmp_path, fp, counts)
    use = np.flatnonzero([p not in (4, 30) for p in range(len(counts))])
    q = np.where(np.isfinite(fp[use]), fp[use], 0.0)
    out, acsv = str(tmp_path / "none.npz"), str(tmp_path / "none.csv")
    cli.main(["clusters", "-f", run, "-o", out, "-k", "2:6", "--sample", "40", "--dtw_band", "5", "--refine", "none", "--assignments", acsv])
    text = capsys.readouterr().out
    assert "4 clusters of 58 usable fingerprints (of 60; 40 sampled)" in text and text.count("<-") == 1
    tm = load_templates(out)
    want_t, want = clusters.discover_clusters(fp, counts, (2, 6), sample=40, band=5, engine=co.OracleEngine())
    assert tm.names == want_t.names == ["cluster_%03d" % c for c in range(4)] and co.same(tm.levels, want_t.levels)
    rows = _read_csv(acsv)
    assert [r[0] for r in rows] == ids.tolist() and rows[4][1:] == ["", "", "", "", "", "0", ""] and rows[30][1] == ""
    near = assign_barcodes(q, counts[use], tm, band=5)
    assert [rows[p][1] for p in use] == [tm.names[b] for b in near.best] and cc.same_partition(near.best, truth[use])
    assert [float(rows[p][2]) for p in use] == near.dist.tolist() and [float(rows[p][5]) for p in use] == near.margin.tolist()
    assert sum(int(r[6]) for r in rows) == 40 and all((r[7] != "") == (r[6] == "1") for r in rows)
    sil = {ids[p]: s for p, s in zip(want["sample_index"], want["silhouette"])}
    assert all(float(r[7]) == sil[r[0]] for r in rows if r[6] == "1")
    with np.load(out, allow_pickle=False) as z:
        assert [str(s) for s in z["medoid_read_id"]] == ids[want["medoid_index"]].tolist() and co.same(z["sweep"], want["sweep"])
        assert z["sizes"].tolist() == want["sizes"].tolist() and co.same(z["silhouette"], want["silhouette_mean"])
        assert z["members"].tolist() == np.bincount(near.best, minlength=4).tolist() and str(z["method"]) == "clusters"
    # the default: refined by DBA over the written labels
    out2, acsv2 = str(tmp_path / "dba.npz"), str(tmp_path / "dba.csv")
    cli.main(["clusters", "-f", run, "-o", out2, "-k", "2:6", "--sample", "40", "--dtw_band", "5", "--dba_iters", "3", "--assignments", acsv2])
    assert "refined by DBA" in capsys.readouterr().out
    rows2 = _read_csv(acsv2)
    assert rows2 == rows
    labels = np.asarray([rows2[p][1] for p in use])
    want_dba, info = bt.dba_templates(fp[use], counts[use], labels, band=5, iters=3)
    got = load_templates(out2)
    assert got.names == want_dba.names and co.same(got.levels, want_dba.levels) and got.counts.tolist() == want_dba.counts.tolist()
    with np.load(out2, allow_pickle=False) as z:
        assert str(z["method"]) == "clusters+dba" and int(z["iterations"]) == info["iterations"] and co.same(z["inertia"], info["inertia"])
        assert z["members"].tolist() == info["members"].tolist()
