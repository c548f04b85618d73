"""The host side of the k-nearest-neighbour barcode assignment (adp_dtw_knn, adapted_amd/knn.py, `adapted knn`), without a GPU: the
new header against its prototype table, the oracle against a brute-force loop, the vote on hand-made lists, the per-label spread,
every refusal of the command line, the command on the oracle in place of the GPU, and the numeric argument for the two lower bounds
the kernel abandons pairs behind -- kept here, where the next editor of adapted_amd/csrc/dtw_knn_api.h finds it."""
import ctypes
import json
import os

import numpy as np
import pytest

import clusters_cases as cc
import dtw_knn_oracle as ko
import fingerprint_oracle as fo
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adapted_hip_knn.h")


def test_prototype_table_and_constants_match_their_header():
    from adapted_amd import lib

    declared = _prototypes(HEADER)
    assert sorted(declared) == sorted(lib.KNN_PROTOTYPES) == ["adp_dtw_knn"]
    others = (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES) | set(lib.EVENT_PROTOTYPES)
              | set(lib.FINGERPRINT_PROTOTYPES) | set(lib.ADAPTER_FRONT_PROTOTYPES) | set(lib.REVALIDATE_PROTOTYPES)
              | set(lib.TEMPLATE_PROTOTYPES) | set(lib.CLUSTER_PROTOTYPES) | set(lib.RESEGMENT_PROTOTYPES) | set(lib.CSV_PROTOTYPES)
              | set(lib.EXPORTS))
    assert not set(lib.KNN_PROTOTYPES) & others
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_knn.h"') == 1
    assert text.index('#include "adapted_hip_clusters.h"') < text.index('#include "adapted_hip_knn.h"') < text.index("adp_set_profiling")
    assert len(_prototypes(os.path.join(ROOT, "include", "adapted_hip.h"))) == len(lib.PROTOTYPES) == 62
    with open(HEADER) as fh:
        head = fh.read()
    defines = {ln.split()[1]: ln.split()[2:] for ln in head.splitlines() if ln.startswith("#define")}
    assert sorted(defines) == ["ADAPTED_HIP_KNN_H", "ADP_KNN_NO_PRUNE", "KNN_KMAX", "KNN_NR_MAX"]
    assert defines["ADP_KNN_NO_PRUNE"][:3] == ["(1", "<<", "22)"] and lib.ADP_KNN_NO_PRUNE == 1 << 22
    assert int(defines["KNN_KMAX"][0]) == lib.KNN_KMAX == 32 and int(defines["KNN_NR_MAX"][0]) == lib.KNN_NR_MAX == 262144
    assert "STRICTLY" in head and "Untuned, nothing validated on real data" in head
    # the flag is no other flag of the ABI
    import re

    flags = [int(a) << int(b) if b else int(a) for a, b in re.findall(r"^#define ADP_[A-Z0-9_]+ \(?(\d+)(?: << (\d+)\))?\s", text, re.M)]
    assert lib.ADP_KNN_NO_PRUNE not in flags
    with open(os.path.join(ROOT, "adapted_amd", "csrc", "dtw_knn_api.h")) as fh:
        kernels = fh.read()
    assert "atomic" not in kernels.lower().replace("no float atomics", "")
    assert "THE FRONTIER BOUND" in kernels and "THE ENDPOINT BOUND" in kernels
    L = lib.load()
    assert L.adp_abi_version() == 3
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.KNN_PROTOTYPES[name].split(":")
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


def test_null_handle_is_refused_and_wrong_types_never_enter_the_library():
    from adapted_amd import lib

    L = lib.load()
    q, qc, r, rc = np.zeros((2, 4)), np.ones(2, dtype=np.int32), np.zeros((3, 4)), np.ones(3, dtype=np.int32)
    idx, dist, work, ex = np.zeros((2, 1), dtype=np.int32), np.zeros((2, 1)), np.zeros((2, 3), dtype=np.int64), np.full(2, -1, dtype=np.int32)
    assert L.adp_dtw_knn(None, q, qc, 2, 4, r, rc, 3, 4, 1, 0, 0, ex, idx, dist, work) == -1 and b"bad argument" in L.adp_last_error()
    assert L.adp_dtw_knn(None, q, qc, 2, 4, r, rc, 3, 4, 1, 0, 0, None, idx, dist, None) == -1 and b"bad argument" in L.adp_last_error()
    bad = [dict(q=q.astype(np.float32)), dict(qc=qc.astype(np.int64)), dict(r=r.astype(np.float32)), dict(rc=rc.astype(np.int64)),
           dict(ex=ex.astype(np.int64)), dict(idx=idx.astype(np.int64)), dict(dist=dist.astype(np.float32)), dict(work=work.astype(np.int32)),
           dict(r=np.zeros((3, 8))[:, ::2])]
    for change in bad:
        a = dict(q=q, qc=qc, r=r, rc=rc, ex=ex, idx=idx, dist=dist, work=work)
        a.update(change)
        with pytest.raises(ctypes.ArgumentError):
            L.adp_dtw_knn(None, a["q"], a["qc"], 2, 4, a["r"], a["rc"], 3, 4, 1, 0, 0, a["ex"], a["idx"], a["dist"], a["work"])


def test_oracle_against_a_brute_force_loop():
    for nq, nr, E, k, band, seed in ((4, 1, 3, 2, 0, 1), (5, 7, 6, 3, 0, 2), (6, 9, 5, 32, 2, 3), (3, 4, 1, 1, 0, 4)):
        q, qc, ok = cc.ragged(nq, E, seed)
        r, rc, _ = cc.ragged(nr, E + 1, seed + 50, unusable=False)
        r[nr - 1] = r[0]
        rc[nr - 1] = rc[0]  # a tie: the lower index first
        ex = np.asarray([(p * 3) % nr if p % 2 else -1 for p in range(nq)])
        idx, dist = ko.knn(q, qc, r, rc, k, band, ex)
        assert idx.shape == dist.shape == (nq, k) and idx.dtype == np.int32
        for p in range(nq):
            if not ok[p]:
                assert (idx[p] == -1).all() and np.isnan(dist[p]).all()
                continue
            pairs = sorted((fo.dtw_pair(q[p, :qc[p]], r[j, :rc[j]], band), j) for j in range(nr) if j != ex[p])[:k]
            assert idx[p, :len(pairs)].tolist() == [j for _, j in pairs] and (idx[p, len(pairs):] == -1).all()
            assert ko.same(dist[p, :len(pairs)], np.asarray([d for d, _ in pairs], dtype=np.float64)) and np.isnan(dist[p, len(pairs):]).all()
        assert ko.candidates(q, qc, nr, ex).tolist() == [(nr - (ex[p] >= 0)) if ok[p] else 0 for p in range(nq)]
    # +inf is an ordinary distance: it sorts last, by index
    idx, dist = ko.topk(np.asarray([[np.inf, 1.0, np.inf, 0.0]]), 4)
    assert idx.tolist() == [[3, 1, 0, 2]] and dist.tolist() == [[0.0, 1.0, np.inf, np.inf]]


def test_vote_on_hand_made_lists():
    from adapted_amd.knn import vote

    labels = np.asarray(["a", "a", "b", "b", "c", "a"])
    idx = np.asarray([[2, 0, 3, 1, -1],     # b, a, b, a: a tie of 2 : 2 -- b's first member is nearer
                      [0, 1, 5, -1, -1],    # all one label: no second
                      [4, 2, 3, -1, -1],    # c first, but b has two votes
                      [-1, -1, -1, -1, -1],  # nothing
                      [4, 0, 2, -1, -1]], dtype=np.int32)  # 1 : 1 : 1 -- the order of the neighbours
    dist = np.asarray([[1.0, 2.0, 3.0, 4.0, np.nan], [0.5, 0.5, 0.75, np.nan, np.nan], [0.0, 1.0, 2.0, np.nan, np.nan], [np.nan] * 5,
                       [1.0, 1.0, 1.0, np.nan, np.nan]])
    a = vote(idx, dist, labels)
    assert a.label.tolist() == ["b", "a", "b", None, "c"] and a.votes.tolist() == [2, 3, 2, 0, 1]
    assert a.label_second.tolist() == ["a", None, "c", None, "a"] and a.votes_second.tolist() == [2, 0, 1, 0, 1]
    assert ko.same(a.dtw_dist, np.asarray([1.0, 0.5, 1.0, np.nan, 1.0])) and ko.same(a.dtw_dist_second, np.asarray([2.0, np.nan, 0.0, np.nan, 1.0]))
    assert a.nearest.tolist() == [2, 0, 4, -1, 4]
    want = ko.vote(idx, dist, labels)
    for p in range(5):
        got = (a.label[p], int(a.votes[p]), float(a.dtw_dist[p]), a.label_second[p], int(a.votes_second[p]), float(a.dtw_dist_second[p]), int(a.nearest[p]))
        assert all(g == w or (isinstance(g, float) and np.isnan(g) and np.isnan(w)) for g, w in zip(got, want[p])), (p, got, want[p])


def test_the_per_label_spread_is_dba_templates():
    from adapted_amd.knn import per_label_spread

    labels = np.asarray(list("abababbbbbcb"))
    assert per_label_spread(labels, 0).tolist() == list(range(12))
    b = np.flatnonzero(labels == "b")
    for N in (1, 2, 3, 5, 100):
        want = []
        for lab in "abc":
            idx = np.flatnonzero(labels == lab)
            S = min(N, idx.size)
            want += [int(idx[(s * idx.size) // S]) for s in range(S)]
        assert per_label_spread(labels, N).tolist() == sorted(want)
    assert per_label_spread(labels, 3).tolist() == sorted([0, 2, 4, 10] + [int(b[0]), int(b[(1 * 8) // 3]), int(b[(2 * 8) // 3])])


def _planted_run(tmp_path, labelled=30):
    fp, counts, truth = cc.planted(per=10)
    fp[7, 1] = np.nan  # inside its count: not usable
    counts[11] = 0
    run, ids = cc.write_run(tmp_path, fp, counts)
    lab = tmp_path / "labels.csv"
    with open(lab, "w") as fh:
        fh.write("read_id,barcode,other\n")
        for p in range(labelled):
            fh.write("%s,bc%d,x\n" % (ids[p], truth[p]))
        fh.write("read_9999,bc0,x\n")  # a label without a fingerprint
    return fp, counts, truth, run, ids, str(lab)


def test_every_refusal_of_the_command_line_leaves_nothing_behind(tmp_path):
    from adapted_amd import main as cli

    fp, counts, truth, run, ids, lab = _planted_run(tmp_path)
    outdir = tmp_path / "out"
    outdir.mkdir()
    out, rep = str(outdir / "o.csv"), str(outdir / "r.json")
    base = ["knn", "-r", run, "-l", lab]
    cls = ["-f", run, "-o", out]
    args = cli.build_parser().parse_args(base + cls)
    assert (args.mode, args.neighbours, args.per_label, args.dtw_band, args.no_prune, args.evaluate, args.report, args.read_id_colname,
            args.label_colname, args.device) == ("knn", 5, 0, 0, False, False, None, "read_id", "barcode", 0)
    for argv in (["knn", "-l", lab] + cls, ["knn", "-r", run] + cls, base + cls + ["-k", "x"]):  # (argparse's own refusals)
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(argv)
    (tmp_path / "empty.csv").write_text("")
    (tmp_path / "nolabel.csv").write_text("read_id,barcode\nread_9999,bc0\n")
    only7 = tmp_path / "only7.csv"
    only7.write_text("read_id,barcode\n%s,bc0\n%s,bc1\n" % (ids[7], ids[11]))  # labels for the two unusable reads only
    few = tmp_path / "few.csv"
    few.write_text("read_id,barcode\n" + "".join("%s,bc%d\n" % (ids[p], truth[p]) for p in range(5)))
    np.savez(tmp_path / "narrow.npz", read_id=ids[:2], count=counts[:2], fingerprints=fp[:2, :5])
    one = os.path.join(run, "fingerprints", "fingerprints_0.npz")
    refusals = [(base + cls + ["-k", "0"], "K must lie in [1, 32]"), (base + cls + ["-k", "33"], "K must lie in [1, 32]"),
                (base + cls + ["--per_label", "-1"], "--per_label"), (base + cls + ["--dtw_band", "-1"], "--dtw_band"),
                (base + cls + ["--device", "-1"], "--device"), (base, "-f with -o, --evaluate"),
                (base + ["-f", run], "-f and -o go together"), (base + ["-o", out, "--evaluate"], "-f and -o go together"),
                (base + cls + ["--report", rep], "--report goes with --evaluate"),
                (base + ["-f", run, "-o", str(tmp_path / "nodir" / "o.csv")], "no directory"),
                (base + ["--evaluate", "--report", str(tmp_path / "nodir" / "r.json")], "no directory"),
                (["knn", "-r", str(tmp_path / "nowhere"), "-l", lab] + cls, "does not exist"),
                (base + ["-f", str(tmp_path / "nowhere"), "-o", out], "does not exist"),
                (["knn", "-r", run, "-l", str(tmp_path / "nolabels.csv")] + cls, "cannot be read"),
                (["knn", "-r", run, "-l", str(tmp_path / "empty.csv")] + cls, "is empty"),
                (base + cls + ["--label_colname", "nope"], "no column 'nope'"), (base + cls + ["--read_id_colname", "nope"], "no column 'nope'"),
                (["knn", "-r", __file__, "-l", lab] + cls, "not a fingerprint file"),
                (["knn", "-r", one, str(tmp_path / "narrow.npz"), "-l", lab] + cls, "different widths"),
                (["knn", "-r", run, "-l", str(tmp_path / "nolabel.csv")] + cls, "none of the 40 fingerprints"),
                (["knn", "-r", run, "-l", str(only7)] + cls, "none of the 40 fingerprints"),
                (["knn", "-r", run, "-l", str(few)] + cls + ["-k", "6"], "5 usable references, K = 6"),
                (["knn", "-r", run, "-l", str(few), "--evaluate"], "5 usable references, K + 1 = 6"),
                (base + cls + ["--per_label", "1"], "4 usable references, K = 5")]
    for argv, why in refusals:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)  # (refused before an engine is made: this test has no GPU)
        assert why in str(e.value), (argv, e.value)
        assert os.listdir(outdir) == [], argv


def test_more_references_than_the_call_takes_are_refused_by_name(tmp_path, monkeypatch):
    from adapted_amd import knn, lib
    from adapted_amd import main as cli

    fp, counts, truth, run, ids, lab = _planted_run(tmp_path)
    monkeypatch.setattr(lib, "KNN_NR_MAX", 20)
    with pytest.raises(SystemExit) as e:
        cli.main(["knn", "-r", run, "-l", lab, "--evaluate"])
    assert "28 references, at most 20" in str(e.value) and "--per_label" in str(e.value)
    with pytest.raises(ValueError):
        knn.dtw_knn(np.zeros((1, 3)), [1], np.zeros((21, 3)), [1] * 21, 1, engine=ko.OracleEngine())


def test_the_module_functions_refuse_before_an_engine_is_made():
    from adapted_amd import knn

    q, qc, r, rc = np.zeros((2, 3)), [1, 1], np.zeros((4, 3)), [1, 2, 3, 1]
    bad = np.zeros((4, 3))
    bad[1, 1] = np.nan
    for call in (lambda: knn.dtw_knn(q, qc, r, rc, 0), lambda: knn.dtw_knn(q, qc, r, rc, 33), lambda: knn.dtw_knn(q, qc, r, rc, 1, band=-1),
                 lambda: knn.dtw_knn(q, qc, r, [1, 2, 4, 1], 1), lambda: knn.dtw_knn(q, qc, r, [0, 1, 1, 1], 1), lambda: knn.dtw_knn(q, qc, bad, rc, 1),
                 lambda: knn.dtw_knn(q, qc, r, rc, 1, exclude=[0, 4]), lambda: knn.dtw_knn(q, qc, r, rc, 1, exclude=[0]),
                 lambda: knn.dtw_knn(q, qc, np.zeros((0, 3)), [], 1), lambda: knn.dtw_knn(q, qc, np.zeros((4, 513)), rc, 1),
                 lambda: knn.knn_barcodes(q, qc, r, rc, ["a"] * 3), lambda: knn.leave_one_out(r, rc, ["a"] * 4, k=4),
                 lambda: knn.leave_one_out(r, rc, ["a"] * 3)):
        with pytest.raises(ValueError):
            call()
    # (a NaN beyond a reference's count is padding, as in a fingerprint file)
    pad = np.arange(12.0).reshape(4, 3)
    pad[0, 1:] = np.nan
    idx, dist = knn.dtw_knn(q, qc, pad, rc, 2, engine=ko.OracleEngine())
    assert idx.tolist() == [[0, 1], [0, 1]] and dist.tolist() == [[0.0, 25.0], [0.0, 25.0]]


def test_the_command_end_to_end_on_the_oracle(tmp_path, capsys):
    from adapted_amd import knn
    from adapted_amd import main as cli

    fp, counts, truth, run, ids, lab = _planted_run(tmp_path)
    # the reads to classify: all 40, two columns wider than the reference; 30 of them are references themselves
    wide = np.concatenate([fp, np.full((fp.shape[0], 2), np.nan)], axis=1)
    qrun, qids = cc.write_run(tmp_path, wide, counts, cut=25, name="qrun")
    assert qids.tolist() == ids.tolist()
    out, rep = str(tmp_path / "o.csv"), str(tmp_path / "r.json")
    for per_label, K, band in ((0, 3, 0), (4, 5, 4)):
        eng = ko.OracleEngine()
        argv = ["knn", "-r", run, "-l", lab, "-f", qrun, "-o", out, "--evaluate", "--report", rep, "-k", str(K), "--dtw_band", str(band),
                "--per_label", str(per_label)]
        report = knn.knn_command(cli.build_parser().parse_args(argv), engine=eng)
        text = capsys.readouterr().out
        # the reference by hand: labelled (the first 30), usable (not 7, not 11), sampled
        ref = np.asarray([p for p in range(30) if p not in (7, 11)])
        if per_label:
            keep = []
            for lab_ in sorted(set(truth[ref].tolist())):
                idx = ref[truth[ref] == lab_]
                S = min(per_label, idx.size)
                keep += [int(idx[(s * idx.size) // S]) for s in range(S)]
            ref = np.asarray(sorted(keep))
        rlab = np.asarray(["bc%d" % truth[p] for p in ref])
        rfp = np.where(np.isfinite(fp[ref]), fp[ref], 0.0)
        ex = np.asarray([ref.tolist().index(p) if p in ref else -1 for p in range(40)])
        idx, dist = ko.knn(wide, counts, rfp, counts[ref], K, band, ex)
        want = ko.vote(idx, dist, rlab)
        assert report["references"] == ref.size and report["k"] == K and report["fingerprints"] == 40 and report["classified"] == 38
        assert report["abandoned_share"] == 0.0 and report["labels"] == ["bc0", "bc1", "bc2", "bc3"]
        assert len(eng.calls) == 2 and eng.calls[0]["exclude"].tolist() == ex.tolist() and eng.calls[0]["band"] == band
        assert eng.calls[1]["exclude"].tolist() == list(range(ref.size)) and eng.calls[1]["nq"] == eng.calls[1]["nr"] == ref.size
        with open(out) as fh:
            lines = [ln.rstrip("\n").split(",") for ln in fh]
        assert lines[0] == ["read_id", "n_events", "barcode", "votes", "dtw_dist", "barcode_second", "votes_second", "dtw_dist_second",
                            "nearest_read_id"]
        assert len(lines) == 41 and [ln[0] for ln in lines[1:]] == ids.tolist() and [int(ln[1]) for ln in lines[1:]] == counts.tolist()
        for p in range(40):
            ln, w = lines[1 + p], want[p]
            if p in (7, 11):
                assert ln[2:] == [""] * 7
                continue
            assert ln[2] == w[0] and int(ln[3]) == w[1] and float(ln[4]) == w[2] and ln[8] == ids[ref[w[6]]]
            assert ln[8] != ln[0]  # a read never votes for itself
            if w[3] is None:
                assert ln[5:8] == ["", "", ""]
            else:
                assert ln[5] == w[3] and int(ln[6]) == w[4] and float(ln[7]) == w[5]
        assert sum(ln[2] == "bc%d" % truth[p] for p, ln in enumerate(lines[1:]) if p not in (7, 11)) >= 36  # (the planted set is plain)
        # the evaluation
        names, conf, acc = ko.leave_one_out(fp[ref], counts[ref], rlab, K, band)
        ev = report["evaluation"]
        assert ev["names"] == names and np.array_equal(ev["confusion"], conf) and ev["confusion"].dtype == np.int64 and ev["accuracy"] == acc
        assert ev["n"] == ref.size and ev["k"] == K and acc > 0.9
        for i, s in enumerate(names):
            assert ev["labels"][s]["n"] == conf[i].sum() and ev["labels"][s]["recall"] == conf[i, i] / conf[i].sum()
            assert ev["labels"][s]["precision"] == conf[i, i] / conf[:, i].sum()
        with open(rep) as fh:
            js = json.load(fh)
        assert js["k"] == K and js["n"] == ref.size and js["accuracy"] == acc and js["names"] == names and js["confusion"] == conf.tolist()
        assert js["labels"] == ev["labels"] and js["band"] == band and js["references"] == ref.size
        assert "K = %d, n = %d, accuracy = %.6f" % (K, ref.size, acc) in text and "confusion" in text and "38 of 40 fingerprints classified" in text
    # classification alone, evaluation alone
    eng = ko.OracleEngine()
    knn.knn_command(cli.build_parser().parse_args(["knn", "-r", run, "-l", lab, "-f", qrun, "-o", out, "--no_prune"]), engine=eng)
    assert len(eng.calls) == 1 and eng.calls[0]["prune"] is False and eng.calls[0]["k"] == 5
    eng = ko.OracleEngine()
    r = knn.knn_command(cli.build_parser().parse_args(["knn", "-r", run, "-l", lab, "--evaluate"]), engine=eng)
    assert len(eng.calls) == 1 and eng.calls[0]["prune"] is True and "fingerprints" not in r


def _matrix(a, c, band):
    n, m = a.size, c.size
    R = max(band, abs(n - m)) if band > 0 else n + m
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if abs(i - j) <= R:
                d = a[i - 1] - c[j - 1]
                D[i, j] = d * d + min(min(D[i - 1, j], D[i, j - 1]), D[i - 1, j - 1])
    return D


def test_the_two_lower_bounds_hold_and_one_frontier_alone_does_not():
    """k_dtw_knn abandons a pair behind these.  The time of cell (i, j) is i + (j - 1) // C, the step at which lane (j - 1) // C
    computes it; the bound of step s is the least D over the cells of the times s - 1 and s.  The cells of time s alone are no
    bound: a diagonal step jumps over a time."""
    rng = np.random.default_rng(20241021)
    checks = both = single = endpoint = 0
    for trial in range(120):
        n, m = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        a = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
        c = a[np.minimum(np.arange(m), n - 1)] + 0.01 * rng.standard_normal(m) if trial % 3 == 0 else rng.standard_normal(m)
        if trial % 10 == 0:
            c = np.resize(a, m).copy()  # equal prefixes: a path of zeros along the diagonal
        for band in (0, 1, 3, 10):
            D = _matrix(a, c, band)
            assert D[n, m] == fo.dtw_pair(a, c, band)
            if n > 1 or m > 1:
                d1, dn = a[0] - c[0], a[n - 1] - c[m - 1]
                assert dn * dn + d1 * d1 <= D[n, m]
                endpoint += 1
            ii, jj = np.meshgrid(np.arange(1, n + 1), np.arange(1, m + 1), indexing="ij")
            for C in (1, 2, 4, 8):
                time = ii + (jj - 1) // C
                steps = n + (m - 1) // C
                assert time[n - 1, m - 1] == steps and time[0, 0] == 1
                for s in range(1, steps + 1):
                    now, before = D[1:, 1:][time == s], D[1:, 1:][time == s - 1]
                    checks += 1
                    assert min(now.min() if now.size else np.inf, before.min() if before.size else np.inf) <= D[n, m], (trial, band, C, s)
                    both += 1
                    if now.size and now.min() > D[n, m]:
                        single += 1
    assert checks == both > 10000 and endpoint > 200
    assert single > 0  # one frontier alone would have abandoned pairs it must not
