"""The host side of the template building (adp_dtw_align, adp_dba_step, adapted_amd/barcode_templates.py, `adapted templates`),
without a GPU: the new header against its prototype table, the oracle's own invariants on every small shape, dba_templates on the
oracle in place of the GPU, the fingerprint files joined with their labels, and the command line with every refusal."""
import ctypes
import os

import numpy as np
import pytest

import dtw_align_oracle as do
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adapted_hip_templates.h")


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(HEADER)
    assert sorted(declared) == sorted(lib.TEMPLATE_PROTOTYPES) == ["adp_dba_step", "adp_dtw_align"]
    others = (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES) | set(lib.EVENT_PROTOTYPES)
              | set(lib.FINGERPRINT_PROTOTYPES) | set(lib.ADAPTER_FRONT_PROTOTYPES) | set(lib.REVALIDATE_PROTOTYPES) | set(lib.EXPORTS))
    assert not set(lib.TEMPLATE_PROTOTYPES) & others
    assert sorted(lib.FINGERPRINT_PROTOTYPES) == ["adp_dtw_assign", "adp_event_levels"]
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_templates.h"') == 1
    assert text.index('#include "adapted_hip_fingerprint.h"') < text.index('#include "adapted_hip_templates.h"') < text.index("adp_set_profiling")
    assert len(_prototypes(os.path.join(ROOT, "include", "adapted_hip.h"))) == len(lib.PROTOTYPES) == 62
    with open(HEADER) as fh:
        assert [ln.split()[1] for ln in fh if ln.startswith("#define")] == ["ADAPTED_HIP_TEMPLATES_H"]
    L = lib.load()
    assert L.adp_abi_version() == 3
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.TEMPLATE_PROTOTYPES[name].split(":")
        assert got_ret == ret and got_params.split() == params, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for q, t in zip(params, fn.argtypes):
            if q in lib._SCALARS:
                assert t is lib._SCALARS[q], (name, q)
            elif q[:-1] in lib._ELEMENTS:
                assert isinstance(t, lib._Pointer) and t.element == q[:-1], (name, q)
            else:
                assert t is ctypes.c_void_p and q == "adp_handle*", (name, q)
    # both calls take adp_dtw_assign's inputs with `which` behind the counts
    assign = lib.FINGERPRINT_PROTOTYPES["adp_dtw_assign"].split()
    for name in declared:
        mine = lib.TEMPLATE_PROTOTYPES[name].split()
        assert mine[:4] + mine[5:13] == assign[:12] and mine[4] == "int32*", name


def test_null_handle_is_refused():
    from adapted_amd import lib

    L = lib.load()
    q, qc, wh, t, tc = np.zeros((1, 4)), np.ones(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros((1, 4)), np.ones(1, dtype=np.int32)
    d, st = np.zeros(1), np.zeros(1, dtype=np.int32)
    assert L.adp_dtw_align(None, q, qc, wh, 1, 4, t, tc, 1, 4, 0, 0, d, st, None, None, None) < 0
    assert L.adp_dba_step(None, q, qc, wh, 1, 4, t, tc, 1, 4, 0, 0, np.zeros((1, 4)), st, d, None) < 0
    with pytest.raises(ctypes.ArgumentError):
        L.adp_dtw_align(None, q, qc, wh.astype(np.int64), 1, 4, t, tc, 1, 4, 0, 0, d, st, None, None, None)


def _sequence(rng, kind, n):
    return rng.standard_normal(n) if kind == "gauss" else rng.integers(-1, 2, n).astype(np.float64)


@pytest.mark.parametrize("kind", ["gauss", "ternary"])
def test_oracle_invariants_on_every_small_shape(kind):
    rng = np.random.default_rng(11 if kind == "gauss" else 12)
    tied = 0
    for n in range(1, 10):
        for m in range(1, 10):
            a, c = _sequence(rng, kind, n), _sequence(rng, kind, m)
            for band in (0, 1, 3):
                D = do.matrix(a, c, band)
                assert do.same(D, do.matrix_cells(a, c, band)) and do.same(D[n, m], do.dtw_pair(a, c, band))
                dist, st, lo, hi, sm, cells = do.align_pair(a, c, 12, band)
                assert st == 0 and do.same(dist, D[n, m])
                assert cells[0] == (n, m) and cells[-1] == (1, 1)
                R = max(band, abs(n - m)) if band > 0 else n + m
                acc, rev = 0.0, cells[::-1]  # from (1, 1) to (n, m)
                for at, (i, j) in enumerate(rev):
                    d = a[i - 1] - c[j - 1]
                    acc = d * d + acc
                    assert abs(i - j) <= R
                    if at + 1 < len(rev):
                        assert (rev[at + 1][0] - i, rev[at + 1][1] - j) in ((1, 1), (1, 0), (0, 1))
                assert do.same(np.float64(acc), np.float64(dist))
                # the runs: contiguous, in order, covering the query
                assert lo[0] == 0 and hi[m - 1] == n - 1 and (lo[m:] == -1).all() and (hi[m:] == -1).all() and np.isnan(sm[m:]).all()
                for j in range(m):
                    assert lo[j] <= hi[j] and sorted(i - 1 for i, jj in cells if jj == j + 1) == list(range(lo[j], hi[j] + 1))
                    if j:
                        assert lo[j] in (hi[j - 1], hi[j - 1] + 1)
                tied += int(any(D[i - 1, j - 1] == D[i - 1, j] or D[i - 1, j - 1] == D[i, j - 1] for i, j in cells if i > 1 and j > 1))
    if kind == "ternary":
        assert tied > 50  # (ties decide the path there)


def test_oracle_statuses_and_dba_step_by_hand():
    q = np.asarray([[1.0, 2.0, 3.0, np.nan], [1.0, np.nan, 0.0, 0.0], [1e200, 0.0, 0.0, 0.0], [5.0, 5.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    qc = np.asarray([3, 2, 1, 2, 0], dtype=np.int32)
    t = np.asarray([[1.0, 3.0, 0.0], [-1e200, 0.0, 0.0]])
    tc = np.asarray([2, 1], dtype=np.int32)
    which = np.asarray([0, 0, 1, -1, 0], dtype=np.int32)
    r = do.align(q, qc, which, t, tc)
    assert r["status"].tolist() == [0, 1, 2, 3, 1]
    # [1, 2, 3] on [1, 3]: D = [[0, 4], [1, 1], [5, 1]]: at (3,2) the diagonal D[2][1] = 1 and up D[2][2] = 1 are equal and the
    # diagonal wins: the path is (3,2) (2,1) (1,1)
    assert r["dist"][0] == 1.0 and r["lo"][0].tolist() == [0, 2, -1] and r["hi"][0].tolist() == [1, 2, -1]
    assert do.same(r["sum"][0], np.asarray([3.0, 3.0, np.nan]))
    assert np.isnan(r["dist"][[1, 3, 4]]).all() and r["dist"][2] == np.inf
    assert (r["lo"][1:] == -1).all() and (r["hi"][1:] == -1).all() and np.isnan(r["sum"][1:]).all()
    t_new, members, inertia, dist = do.dba_step(q, qc, which, t, tc)
    assert do.same(t_new, np.asarray([[1.5, 3.0, np.nan], [-1e200, np.nan, np.nan]]))  # (template 1: no member, its old value)
    assert members.tolist() == [1, 0] and inertia.tolist() == [1.0, 0.0] and do.same(dist, r["dist"])


def _labelled(seed=5, per=9, E=12):
    """three labels of warped noisy copies, a few members that are not usable"""
    rng = np.random.default_rng(seed)
    fps, counts, labels = [], [], []
    for lab, n in (("bc2", 7), ("bc1", 9), ("bc3", 6)):
        base = rng.standard_normal(n)
        for _ in range(per):
            x = np.repeat(base, rng.integers(1, 3, n))[:E]
            x = x + 0.05 * rng.standard_normal(x.size)
            row = np.full(E, np.nan)
            row[:x.size] = x
            fps.append(row)
            counts.append(x.size)
            labels.append(lab)
    fps, counts, labels = np.asarray(fps), np.asarray(counts, dtype=np.int32), np.asarray(labels)
    fps[3, 1] = np.nan  # inside its count: not usable
    counts[12] = 0
    return fps, counts, labels


def test_dba_templates_on_the_oracle_with_a_recording_align():
    from adapted_amd import barcode_templates as bt
    from adapted_amd.fingerprint import medoid_templates

    fp, counts, labels = _labelled()
    calls = []

    def align(q, qc, which, t, tc, band):
        calls.append((np.array(q), np.array(qc), np.array(which), np.array(t), np.array(tc), band))
        return do.align(q, qc, which, t, tc, band)

    tm, info = bt.dba_templates(fp, counts, labels, band=2, iters=4, init_sample=4, align=align)
    init, steps = calls[:3], calls[3:]
    assert tm.names == ["bc1", "bc2", "bc3"] and 1 <= info["iterations"] == len(steps) <= 4 and info["inertia"].shape == (info["iterations"], 3)
    # the first calls: the medoids' distances, per label every sampled member against every sampled member
    usable = np.asarray([1 <= counts[p] <= 12 and bool(np.isfinite(fp[p, :counts[p]]).all()) for p in range(len(counts))])
    sample = []
    for lab in tm.names:
        idx = np.flatnonzero((labels == lab) & usable)
        sample += [int(idx[(s * idx.size) // 4]) for s in range(4)]
    assert all(c[0].shape[0] == 4 * 4 and c[5] == 2 for c in init)
    start = medoid_templates(fp[sample], counts[sample], labels[sample], 2, distances=lambda q, qc, t, tc, b: do_dist(q, qc, t, tc, b))
    assert do.same(np.where(np.isnan(start.levels), 0.0, start.levels), steps[0][3]) and start.counts.tolist() == steps[0][4].tolist() == tm.counts.tolist()
    # the steps: all fingerprints, -1 for the members that are not usable, the oracle's iteration
    which = steps[0][2]
    assert which[3] == which[12] == -1 and (which[usable] == [tm.names.index(s) for s in labels[usable]]).all()
    t = steps[0][3]
    for it in range(info["iterations"]):
        assert do.same(steps[it][3], t) and do.same(steps[it][2], which)
        t_new, members, inertia, _ = do.dba_step(fp, counts, which, t, tm.counts, 2)
        assert do.same(info["inertia"][it], inertia)
        t = np.where(np.isnan(t_new), 0.0, t_new)
    assert do.same(tm.levels, t_new) and info["members"].tolist() == members.tolist() == [8, 8, 9]
    assert np.isnan(tm.levels[0, tm.counts[0]:]).all()
    if info["iterations"] < 4:  # it stopped because the last step changed no bit
        assert do.same(steps[-1][3], np.where(np.isnan(t_new), 0.0, t_new))
    # no step: the sampled medoid and the usable members
    tm0, info0 = bt.dba_templates(fp, counts, labels, band=2, iters=0, init_sample=4, align=align)
    assert do.same(tm0.levels, start.levels) and info0["iterations"] == 0 and info0["members"].tolist() == [8, 8, 9] and info0["inertia"].shape == (0, 3)
    # a sample of everything is medoid_templates itself
    tm_all, _ = bt.dba_templates(fp, counts, labels, iters=0, init_sample=4096, align=align)
    whole = medoid_templates(fp, counts, labels, 0, distances=do_dist)
    assert do.same(tm_all.levels, whole.levels)


def do_dist(q, qc, t, tc, band):
    return np.asarray([[do.dtw_pair(q[i, :qc[i]], t[k, :tc[k]], band) for k in range(t.shape[0])] for i in range(q.shape[0])])


def test_dba_templates_refusals():
    from adapted_amd import barcode_templates as bt

    fp, counts, labels = _labelled()
    for kw in ({"init_sample": 0}, {"init_sample": 4097}, {"iters": -1}, {"band": -1}):
        with pytest.raises(ValueError):
            bt.dba_templates(fp, counts, labels, align=do.align, **kw)
    with pytest.raises(ValueError, match="one label per fingerprint"):
        bt.dba_templates(fp, counts, labels[:-1], align=do.align)
    bad = counts.copy()
    bad[labels == "bc3"] = 0
    with pytest.raises(ValueError, match="no usable fingerprint"):
        bt.dba_templates(fp, bad, labels, align=do.align)
    with pytest.raises(ValueError):
        bt.dtw_align(fp, counts, np.full(len(counts), 3), fp[:3], counts[:3] * 0 + 1)  # (which: no such template; before any engine)
    with pytest.raises(ValueError):
        bt.dba_step(fp, counts, np.zeros(len(counts) - 1), fp[:3], counts[:3] * 0 + 1)


def _run_files(tmp_path, fp, counts, labels):
    """a run directory with two fingerprint files, and a labels CSV that leaves two reads out and names one that has no file"""
    d = tmp_path / "run" / "fingerprints"
    d.mkdir(parents=True)
    ids = np.asarray(["read_%03d" % i for i in range(len(counts))])
    cut = 10
    for k, sl in ((0, slice(0, cut)), (1, slice(cut, None))):
        np.savez(d / ("fingerprints_%d.npz" % k), read_id=ids[sl], count=counts[sl], status=np.zeros(len(counts[sl]), dtype=np.int32),
                 lengths=np.zeros(fp[sl].shape, dtype=np.int32), levels=fp[sl], fingerprints=fp[sl])
    (d / "barcodes_0.csv").write_text("read_id\n")  # (other files of that folder are not looked at)
    csv_path = tmp_path / "labels.csv"
    lines = ["name,rid,bc"] + ["x,%s,%s" % (ids[i], labels[i]) for i in range(len(ids)) if i not in (0, 20)] + ["x,read_999,bc1", "x,read_000,"]
    csv_path.write_text("\n".join(lines) + "\n")
    return str(tmp_path / "run"), str(csv_path), ids


def test_labelled_fingerprints_on_hand_made_files(tmp_path):
    from adapted_amd import barcode_templates as bt

    fp, counts, labels = _labelled()
    run, csv_path, ids = _run_files(tmp_path, fp, counts, labels)
    keep = [i for i in range(len(ids)) if i not in (0, 20)]  # (read_000: a line with an empty label is no label)
    for paths in (run, [run], [os.path.join(run, "fingerprints", "fingerprints_%d.npz" % k) for k in (0, 1)]):
        got, c, lab, report = bt.labelled_fingerprints(paths, csv_path, "rid", "bc")
        assert do.same(got, fp[keep]) and c.tolist() == counts[keep].tolist() and lab.tolist() == labels[keep].tolist()
        assert report == {"fingerprints": len(ids), "unlabelled": 2, "labels_without_fingerprint": 1}
    with pytest.raises(ValueError, match="no column 'barcode'"):
        bt.labelled_fingerprints(run, csv_path, "rid")
    with pytest.raises(ValueError, match="cannot be read"):
        bt.labelled_fingerprints(run, str(tmp_path / "none.csv"), "rid", "bc")
    with pytest.raises(ValueError, match="not a fingerprint file"):
        bt.labelled_fingerprints([csv_path], csv_path, "rid", "bc")
    with pytest.raises(ValueError, match="no fingerprints_<k>.npz"):
        bt.labelled_fingerprints(str(tmp_path), csv_path, "rid", "bc")
    np.savez(tmp_path / "narrow.npz", read_id=ids[:2], count=counts[:2], fingerprints=fp[:2, :5])
    with pytest.raises(ValueError, match="different widths"):
        bt.labelled_fingerprints([os.path.join(run, "fingerprints", "fingerprints_0.npz"), str(tmp_path / "narrow.npz")], csv_path, "rid", "bc")


def test_the_command_parses_refuses_and_writes_a_template_file(tmp_path, capsys):
    from adapted_amd import barcode_templates as bt
    from adapted_amd import main as cli
    from adapted_amd.fingerprint import load_templates

    fp, counts, labels = _labelled()
    run, csv_path, _ = _run_files(tmp_path, fp, counts, labels)
    out = str(tmp_path / "t.npz")
    base = ["templates", "-f", run, "-l", csv_path, "-o", out, "--read_id_colname", "rid", "--label_colname", "bc"]
    args = cli.build_parser().parse_args(base)
    assert (args.mode, args.method, args.iters, args.init_sample, args.dtw_band, args.device) == ("templates", "dba", 10, 256, 0, 0)
    assert args.fingerprints == [run] and args.labels == csv_path and args.output == out
    for extra in (["--method", "kmeans"], ["--iters", "x"]):  # (argparse's own refusals)
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + extra)
    for argv in (["templates", "-l", csv_path, "-o", out], ["templates", "-f", run, "-o", out], ["templates", "-f", run, "-l", csv_path]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(argv)
    empty = tmp_path / "empty.csv"
    empty.write_text("rid,bc\nread_999,bc1\n")
    binary = tmp_path / "binary.csv"
    binary.write_bytes(b"\xff\xfe\x00\x00rid,bc\n")
    refusals = [(base + ["--iters", "-1"], "--iters"), (base + ["--init_sample", "0"], "--init_sample"),
                (base + ["--init_sample", "4097"], "--init_sample"), (base + ["--dtw_band", "-1"], "--dtw_band"),
                (base + ["--device", "-1"], "--device"),
                (base[:2] + [str(tmp_path / "nowhere")] + base[3:], "does not exist"),
                (base[:4] + [str(tmp_path / "none.csv")] + base[5:], "cannot be read"),
                (base[:4] + [str(binary)] + base[5:], "labels file"),
                (base[:6] + [str(tmp_path / "nodir" / "t.npz")] + base[7:], "no directory"),
                (base[:7], "no column 'read_id'"), (base[:9], "no column 'barcode'"),
                (base[:4] + [str(empty)] + base[5:], "none of the 27 fingerprints has a label"),
                (base[:2] + [csv_path] + base[3:], "not a fingerprint file")]
    for argv, why in refusals:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)  # (refused before an engine is made: this test has no GPU)
        assert why in str(e.value), (argv, e.value)
    assert not os.path.exists(out)
    # the whole command on the oracle in place of the GPU
    for method in ("dba", "medoid"):
        report = bt.templates_command(cli.build_parser().parse_args(base + ["--method", method, "--iters", "3", "--init_sample", "5", "--dtw_band", "2"]),
                                      align=do.align)
        assert report["labels"] == ["bc1", "bc2", "bc3"] and report["unlabelled"] == 2 and "Templates of 3 labels" in capsys.readouterr().out
        got = load_templates(out)
        keep = [i for i in range(len(counts)) if i not in (0, 20)]
        want, info = bt.dba_templates(fp[keep], counts[keep], labels[keep], band=2, iters=3 if method == "dba" else 0, init_sample=5, align=do.align)
        assert got.names == want.names and do.same(got.levels, want.levels) and got.counts.tolist() == want.counts.tolist()
        with np.load(out, allow_pickle=False) as z:
            assert sorted(z.files) == ["band", "counts", "inertia", "iterations", "levels", "members", "method", "names"]
            assert str(z["method"]) == method and int(z["band"]) == 2 and int(z["iterations"]) == info["iterations"]
            assert z["members"].tolist() == info["members"].tolist() and do.same(z["inertia"], info["inertia"])
        assert info["iterations"] == 0 if method == "medoid" else 1 <= info["iterations"] <= 3
