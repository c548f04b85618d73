"""The host side of the clustering of fingerprints without labels (adp_dtw_pairwise, adp_kmedoids_build, adp_kmedoids,
adp_silhouette, adapted_amd/clusters.py, `adapted clusters`), without a GPU: the new header against its prototype table, the
oracle's own known answers worked by hand, its silhouette against scikit-learn's, discover_clusters and the command on the oracle
in place of the GPU, every refusal of the command line, and the condition on the planted data the GPU test relies on."""
import ctypes
import os

import numpy as np
import pytest

import clusters_cases as cc
import dtw_align_oracle as do
import dtw_cluster_oracle as co
import fingerprint_oracle as fo
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adapted_hip_clusters.h")
NAMES = ["adp_dtw_pairwise", "adp_kmedoids", "adp_kmedoids_build", "adp_silhouette"]


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(HEADER)
    assert sorted(declared) == sorted(lib.CLUSTER_PROTOTYPES) == NAMES
    others = (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES) | set(lib.EVENT_PROTOTYPES)
              | set(lib.FINGERPRINT_PROTOTYPES) | set(lib.ADAPTER_FRONT_PROTOTYPES) | set(lib.REVALIDATE_PROTOTYPES)
              | set(lib.TEMPLATE_PROTOTYPES) | set(lib.CSV_PROTOTYPES) | set(lib.EXPORTS))
    assert not set(lib.CLUSTER_PROTOTYPES) & others
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_clusters.h"') == 1
    assert text.index('#include "adapted_hip_templates.h"') < text.index('#include "adapted_hip_clusters.h"') < text.index("adp_set_profiling")
    assert len(_prototypes(os.path.join(ROOT, "include", "adapted_hip.h"))) == len(lib.PROTOTYPES) == 62
    with open(HEADER) as fh:
        head = fh.read()
    assert [ln.split()[1] for ln in head.splitlines() if ln.startswith("#define")] == ["ADAPTED_HIP_CLUSTERS_H"]
    assert "p[l] += p[l + s]" in head and "Untuned, nothing validated on real data" in head
    with open(os.path.join(ROOT, "adapted_amd", "csrc", "dtw_cluster_api.h")) as fh:
        kernels = fh.read()
    assert "#define CL_NMAX %d " % lib.CLUSTER_MAX_ROWS in kernels and "#define CL_KMAX %d " % lib.CLUSTER_MAX_K in kernels
    assert "atomic" not in kernels.lower().replace("no float atomics", "")
    L = lib.load()
    assert L.adp_abi_version() == 3
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.CLUSTER_PROTOTYPES[name].split(":")
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
    q, qc, D = np.zeros((2, 4)), np.ones(2, dtype=np.int32), np.zeros((2, 2))
    med, a, cost, it, sil, gain = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(1, dtype=np.int32), np.zeros(2), np.zeros(1)
    assert L.adp_dtw_pairwise(None, q, qc, 2, 4, 0, 0, D) == -1 and b"bad argument" in L.adp_last_error()
    assert L.adp_kmedoids_build(None, D, 2, 1, 0, med, gain) == -1 and b"bad argument" in L.adp_last_error()
    assert L.adp_kmedoids(None, D, 2, 1, 1, 0, med, a, None, cost, it) == -1 and b"bad argument" in L.adp_last_error()
    assert L.adp_silhouette(None, D, 2, a, 1, 0, sil) == -1 and b"bad argument" in L.adp_last_error()
    with pytest.raises(ctypes.ArgumentError):  # float32 fingerprints
        L.adp_dtw_pairwise(None, q.astype(np.float32), qc, 2, 4, 0, 0, D)
    with pytest.raises(ctypes.ArgumentError):  # int64 counts
        L.adp_dtw_pairwise(None, q, qc.astype(np.int64), 2, 4, 0, 0, D)
    with pytest.raises(ctypes.ArgumentError):  # int64 for int32 *medoids_out
        L.adp_kmedoids_build(None, D, 2, 1, 0, med.astype(np.int64), gain)
    with pytest.raises(ctypes.ArgumentError):  # float32 matrix
        L.adp_kmedoids(None, D.astype(np.float32), 2, 1, 1, 0, med, a, None, cost, it)
    with pytest.raises(ctypes.ArgumentError):  # int64 for int32 *iters_out
        L.adp_kmedoids(None, D, 2, 1, 1, 0, med, a, None, cost, it.astype(np.int64))
    with pytest.raises(ctypes.ArgumentError):  # float64 for int32 *assign
        L.adp_silhouette(None, D, 2, a.astype(np.float64), 1, 0, sil)
    with pytest.raises(ctypes.ArgumentError):  # a matrix with strides
        L.adp_silhouette(None, np.zeros((2, 4))[:, ::2], 2, a, 1, 0, sil)


def test_the_order_of_a_sum_is_the_headers():
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 130, 200):
        t = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        p = [0.0] * 64
        for j in range(n):  # (ascending j: partial j % 64)
            p[j % 64] = p[j % 64] + float(t[j])
        s = 32
        while s >= 1:
            for lane in range(s):
                p[lane] = p[lane] + p[lane + s]
            s //= 2
        assert co.same(np.float64(p[0]), np.float64(co.osum(t)))
    t = rng.standard_normal((3, 5, 130))
    assert co.same(co.osum(t)[2, 4], co.osum(t[2, 4]))
    assert not co.same(co.osum(t), np.cumsum(t, axis=-1)[..., -1])  # (it is an order of its own)


def _line(*xs):
    x = np.asarray(xs, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


def test_three_points_on_a_line_by_hand():
    D = _line(0.0, 1.0, 5.0)
    # row sums 6, 5, 9: medoid 1.  dmin = [1, 0, 4]: the gains of rows 0 and 2 are 1 and 4: medoid 2; then row 0 with gain 1
    med, gain = co.build(D, 3)
    assert med.tolist() == [1, 2, 0] and gain.tolist() == [5.0, 4.0, 1.0]
    # from the medoids (0, 2): 1 goes to slot 0 (1 < 4); in slot 0 both members have the sum 1: the lowest index stays
    r = co.kmedoids(D, [0, 2], 5)
    assert r["medoids"].tolist() == [0, 2] and r["assign"].tolist() == [0, 0, 1] and r["iters"] == 0 and r["cost"].tolist() == [1.0]
    assert r["sums"].tolist() == [[1.0, 5.0], [1.0, 4.0], [9.0, 0.0]]
    # from (2, 1) -- slots in that order --: 0 goes to slot 1, whose members 0 and 1 both have the sum 1: the lowest index, 0,
    # takes the medoid from 1 -- one counted update at the same cost --, and the next update changes nothing
    r = co.kmedoids(D, [2, 1], 5)
    assert r["assign"].tolist() == [1, 1, 0] and r["medoids"].tolist() == [2, 0] and r["iters"] == 1 and r["cost"].tolist() == [1.0, 1.0]
    # the silhouette: a = 1, b = 5 -> 0.8; a = 1, b = 4 -> 0.75; a cluster of one -> 0
    assert co.silhouette(D, [0, 0, 1], 2).tolist() == [0.8, 0.75, 0.0]
    # four points, a bad start: medoids (0, 1) of 0, 1, 10, 11: slot 1 holds 1, 10, 11 with the sums 19, 10, 11: medoid 10; then
    # 1 moves to slot 0 and slot 1's sums are 1 and 1: 10 stays.  The cost: 0 + 0 + 9 + 10 = 19, then 0 + 1 + 0 + 1 = 2, twice
    D = _line(0.0, 1.0, 10.0, 11.0)
    r = co.kmedoids(D, [0, 1], 5)
    assert r["medoids"].tolist() == [0, 2] and r["assign"].tolist() == [0, 0, 1, 1] and r["iters"] == 1 and r["cost"].tolist() == [19.0, 2.0]
    r0 = co.kmedoids(D, [0, 1], 0)
    assert r0["medoids"].tolist() == [0, 1] and r0["assign"].tolist() == [0, 1, 1, 1] and r0["iters"] == 0 and r0["cost"].tolist() == [19.0]
    r1 = co.kmedoids(D, [0, 1], 1)
    assert r1["medoids"].tolist() == [0, 2] and r1["assign"].tolist() == [0, 0, 1, 1] and r1["iters"] == 1 and r1["cost"].tolist() == [19.0, 2.0]


def test_duplicates_never_empty_a_cluster_and_ties_go_to_the_lowest_index():
    D = _line(3.0, 3.0, 3.0, 7.0)  # rows 0, 1, 2 are one point
    med, gain = co.build(D, 4)
    # row sums 4, 4, 4, 12: the lowest index; then 3 (gain 4); then rows 1 and 2 with gain 0 each: the lowest that is no medoid
    assert med.tolist() == [0, 3, 1, 2] and gain.tolist() == [4.0, 4.0, 0.0, 0.0]
    r = co.kmedoids(D, [1, 0, 3], 5)
    # medoid 1 keeps slot 0 although medoid 0 is as near; row 2 goes to the lowest slot
    assert r["assign"].tolist() == [1, 0, 0, 2] and np.bincount(r["assign"]).min() >= 1 and r["iters"] == 0
    assert co.silhouette(D, r["assign"], 3).tolist() == [0.0, 0.0, 0.0, 0.0]  # (max(a, b) == 0, and clusters of one)
    Z = np.zeros((5, 5))  # all equal
    assert co.build(Z, 5)[0].tolist() == [0, 1, 2, 3, 4]
    r = co.kmedoids(Z, [4, 2], 3)
    assert r["assign"].tolist() == [0, 0, 1, 0, 0] and r["medoids"].tolist() == [0, 2] and r["iters"] == 1 and r["cost"].tolist() == [0.0, 0.0]


def test_k_one_k_n_and_the_build_prefix():
    D = cc.points_matrix(37, 5)
    n = D.shape[0]
    full, gain = co.build(D, n)
    assert sorted(full.tolist()) == list(range(n)) and (gain[1:] >= 0).all()
    for K in (1, 2, 3, 17, 36):
        med, g = co.build(D, K)
        assert med.tolist() == full[:K].tolist() and co.same(g, gain[:K])  # the prefix property, to the bit
    r = co.kmedoids(D, full[:1], 10)
    assert (r["assign"] == 0).all() and r["medoids"][0] == full[0] and r["iters"] == 0  # (BUILD's first medoid IS the 1-medoid)
    assert co.same(r["cost"][0], gain[0])
    assert co.silhouette(D, r["assign"], 1).tolist() == [0.0] * n
    r = co.kmedoids(D, full, 10)
    assert r["assign"][full].tolist() == list(range(n)) and r["iters"] == 0 and r["cost"].tolist() == [0.0]
    assert co.silhouette(D, r["assign"], n).tolist() == [0.0] * n
    with pytest.raises(ValueError):
        co.build(D, n + 1)
    for bad in (np.nan, -1.0, np.inf):
        B = D.copy()
        B[3, 4] = bad
        with pytest.raises(ValueError):
            co.build(B, 2)
        with pytest.raises(ValueError):
            co.kmedoids(B, [0, 1])
        with pytest.raises(ValueError):
            co.silhouette(B, [0] * n, 1)
    with pytest.raises(ValueError):
        co.silhouette(D, [0] * n, 2)  # an empty cluster
    with pytest.raises(ValueError):
        co.kmedoids(D, [1, 1])


def test_the_cost_does_not_increase_on_exact_sums():
    # (integer coordinates: every sum is exact, so PAM's argument holds to the bit)
    for seed in range(6):
        D = cc.points_matrix(90, seed, integer=True)
        r = co.kmedoids(D, [0, 1, 2, 3, 4], 50)
        assert r["iters"] >= 1 and (np.diff(r["cost"]) <= 0).all() and r["cost"].size == r["iters"] + 1


def test_silhouette_against_scikit_learn():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(9)
    for n in (3, 8, 70):
        D = cc.points_matrix(n, n, duplicates=n > 8)
        for K in range(2, n):
            a = rng.integers(0, K, n)
            a[:K] = np.arange(K)  # (no empty cluster)
            want = sk.silhouette_samples(D, a, metric="precomputed")
            got = co.silhouette(D, a, K)
            assert np.abs(got - want).max() <= 1e-12, (n, K)


def test_pairwise_oracle_is_the_assign_oracle_mirrored():
    q, qc, ok = cc.ragged(9, 7, 1)
    for band in (0, 2):
        d = co.pairwise(q, qc, band)
        assert co.same(d, d.T) and np.isnan(d[~ok]).all() and np.isnan(d[:, ~ok]).all()
        good = np.flatnonzero(ok)
        for i in good:
            for j in good:
                want = 0.0 if i == j else fo.dtw_pair(q[i, :qc[i]], q[j, :qc[j]], band)
                assert co.same(np.float64(d[i, j]), np.float64(want)) and not np.signbit(d[i, j])
                assert co.same(np.float64(want), np.float64(fo.dtw_pair(q[j, :qc[j]], q[i, :qc[i]], band)) if i != j else np.float64(0.0))


@pytest.fixture(scope="module")
def planted_result():
    from adapted_amd import clusters

    fp, counts, truth = cc.planted()
    eng = co.OracleEngine()
    tm, info = clusters.discover_clusters(fp, counts, (2, 8), engine=eng)
    return fp, counts, truth, eng, tm, info


def test_planted_clusters_are_recovered_by_the_oracle(planted_result):
    """the condition on the planted inputs that tests/test_gpu_clusters.py relies on"""
    fp, counts, truth, eng, tm, info = planted_result
    n = len(counts)
    assert n == 120 and 36 <= counts.min() and counts.max() <= 44 and len(set(counts.tolist())) > 3
    assert info["k"] == 4 and info["sweep"][:, 0].tolist() == [2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    # (0.5: the silhouette from which Kaufman and Rousseeuw call a structure reasonable -- the planted one is meant to be plain)
    assert int(np.argmax(info["sweep"][:, 2])) == 2 and info["sweep"][2, 2] > 0.5
    assert info["sample_index"].tolist() == list(range(n)) and cc.same_partition(info["assign"], truth)
    assert info["sizes"].tolist() == [30] * 4 and (info["silhouette_mean"] > 0.5).all()
    assert tm.names == ["cluster_000", "cluster_001", "cluster_002", "cluster_003"]
    for c, p in enumerate(info["medoid_index"]):
        assert info["assign"][p] == c and tm.counts[c] == counts[p] and co.same(tm.levels[c], fp[p])
    # one matrix, built once, given back
    assert eng.pairwise_calls == 1 and len(eng.freed) == 1 and not eng.mem


def test_discover_clusters_follows_its_rules_on_the_oracle():
    from adapted_amd import clusters

    fp, counts, truth = cc.planted(per=12)
    fp[5, 2] = np.nan  # inside its count: not usable
    counts[9] = 0
    eng = co.OracleEngine()
    tm, info = clusters.discover_clusters(fp, counts, (2, 5), sample=20, band=3, iters=7, engine=eng)
    idx = np.flatnonzero([p not in (5, 9) for p in range(len(counts))])
    sample = np.asarray([idx[(s * idx.size) // 20] for s in range(20)])
    assert info["sample_index"].tolist() == sample.tolist()
    q = np.where(np.isfinite(fp[sample]), fp[sample], 0.0)
    D = co.pairwise(q, counts[sample], 3)
    start, _ = co.build(D, 5)
    rows, best = [], None
    for K in range(2, 6):
        r = co.kmedoids(D, start[:K], 7)
        sil = co.silhouette(D, r["assign"], K)
        rows.append([K, r["cost"][-1], float(np.mean(sil)), r["iters"]])
        if best is None or rows[-1][2] > best[0]:
            best = (rows[-1][2], K, r, sil)
    assert co.same(info["sweep"], np.asarray(rows, dtype=np.float64)) and info["k"] == best[1]
    assert info["assign"].tolist() == best[2]["assign"].tolist() and co.same(info["silhouette"], best[3])
    assert info["medoid_index"].tolist() == sample[best[2]["medoids"]].tolist()
    # one K; a K above the usable count; bad options
    tm1, info1 = clusters.discover_clusters(fp, counts, 3, sample=20, engine=eng)
    assert info1["k"] == 3 and info1["sweep"].shape == (1, 4) and len(tm1.names) == 3
    for kw in ({"k": 0}, {"k": (3, 2)}, {"k": 4097}, {"k": len(counts) - 1}, {"k": 2, "sample": 1}, {"k": 2, "sample": 16385},
               {"k": 2, "band": -1}, {"k": 2, "iters": -1}):
        with pytest.raises(ValueError):
            clusters.discover_clusters(fp, counts, engine=eng, **kw)
    assert not eng.mem
    # the module functions refuse before an engine is made
    for call in (lambda: clusters.kmedoids_build(np.zeros((3, 3)), 4), lambda: clusters.kmedoids(np.zeros((3, 3)), [0, 0]),
                 lambda: clusters.kmedoids(np.zeros((3, 3)), [0], max_iter=-1), lambda: clusters.silhouette(np.zeros((3, 3)), [0, 0, 2], 2),
                 lambda: clusters.silhouette(np.zeros((3, 3)), [0, 0, 0], 2), lambda: clusters.dtw_pairwise(np.zeros((2, 3)), [1, 1], band=-1),
                 lambda: clusters.kmedoids_build(np.zeros((3, 2)), 1), lambda: clusters.kmedoids_build(1234, 1)):
        with pytest.raises(ValueError):
            call()


def test_the_command_parses_refuses_and_writes_its_files(tmp_path, capsys):
    from adapted_amd import barcode_templates as bt
    from adapted_amd import clusters
    from adapted_amd import main as cli
    from adapted_amd.fingerprint import Templates, load_templates

    fp, counts, truth = cc.planted(per=10)
    fp[7, 1] = np.nan
    counts[11] = 0
    run, ids = cc.write_run(tmp_path, fp, counts)
    out, acsv = str(tmp_path / "c.npz"), str(tmp_path / "a.csv")
    base = ["clusters", "-f", run, "-o", out, "-k", "2:6"]
    args = cli.build_parser().parse_args(base)
    assert (args.mode, args.clusters, args.sample, args.iters, args.dtw_band, args.refine, args.dba_iters, args.assignments, args.device) == (
        "clusters", "2:6", 4096, 50, 0, "dba", 10, None, 0)
    for extra in (["--refine", "kmeans"], ["--iters", "x"]):  # (argparse's own refusals)
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + extra)
    for argv in (["clusters", "-o", out, "-k", "2"], ["clusters", "-f", run, "-k", "2"], ["clusters", "-f", run, "-o", out]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(argv)
    np.savez(tmp_path / "narrow.npz", read_id=ids[:2], count=counts[:2], fingerprints=fp[:2, :5])
    one = os.path.join(run, "fingerprints", "fingerprints_0.npz")
    refusals = [(base[:6] + ["0"], "K must be >= 1"), (base[:6] + ["0:3"], "K must be >= 1"), (base[:6] + ["5:4"], "KMAX must be >= KMIN"),
                (base[:6] + ["4097"], "at most 4096"), (base[:6] + ["39"], "39 clusters of 38 usable"), (base[:6] + ["2:x"], "KMIN:KMAX"),
                (base[:6] + ["1:2:3"], "KMIN:KMAX"), (base + ["--sample", "1"], "--sample"), (base + ["--sample", "16385"], "--sample"),
                (base + ["--dtw_band", "-1"], "--dtw_band"), (base + ["--iters", "-1"], "--iters"), (base + ["--dba_iters", "-1"], "--dba_iters"),
                (base + ["--device", "-1"], "--device"), (base[:4] + [str(tmp_path / "nodir" / "c.npz")] + base[5:], "no directory"),
                (base + ["--assignments", str(tmp_path / "nodir" / "a.csv")], "no directory"),
                (base[:2] + [str(tmp_path / "nowhere")] + base[3:], "does not exist"),
                (base[:2] + [str(tmp_path / "narrow.npz").replace("narrow.npz", "a_missing.npz")] + base[3:], "does not exist"),
                (base[:2] + [one, str(tmp_path / "narrow.npz")] + base[3:], "different widths"),
                (base[:2] + [__file__] + base[3:], "not a fingerprint file")]
    for argv, why in refusals:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)  # (refused before an engine is made: this test has no GPU)
        assert why in str(e.value), (argv, e.value)
    assert not os.path.exists(out) and not os.path.exists(acsv)
    # the whole command on the oracle in place of the GPU
    use = np.flatnonzero([p not in (7, 11) for p in range(len(counts))])
    for refine in ("none", "dba"):
        eng = co.OracleEngine()
        a = cli.build_parser().parse_args(base + ["--refine", refine, "--dba_iters", "2", "--dtw_band", "4", "--sample", "30", "--assignments", acsv])
        report = clusters.clusters_command(a, engine=eng, align=do.align)
        text = capsys.readouterr().out
        assert report["k"] == 4 and report["usable"] == 38 and report["fingerprints"] == 40 and "4 clusters of 38 usable" in text and "<-" in text
        tm, info = clusters.discover_clusters(fp, counts, (2, 6), sample=30, band=4, engine=co.OracleEngine())
        q = np.where(np.isfinite(fp[use]), fp[use], 0.0)
        best, bd = fo.assign(fo.dtw(q, counts[use], np.where(np.isnan(tm.levels), 0.0, tm.levels), tm.counts, 4))
        assert cc.same_partition(best[:, 0], truth[use])
        got = load_templates(out)
        with np.load(out, allow_pickle=False) as z:
            assert sorted(z.files) == sorted(["band", "counts", "inertia", "iterations", "levels", "members", "method", "names",
                                              "medoid_read_id", "sizes", "silhouette", "sweep"])
            assert [str(s) for s in z["medoid_read_id"]] == ids[info["medoid_index"]].tolist() and z["sizes"].tolist() == info["sizes"].tolist()
            assert co.same(z["silhouette"], info["silhouette_mean"]) and co.same(z["sweep"], info["sweep"]) and int(z["band"]) == 4
            assert str(z["method"]) == ("clusters" if refine == "none" else "clusters+dba")
            if refine == "none":
                assert z["members"].tolist() == np.bincount(best[:, 0], minlength=4).tolist() and int(z["iterations"]) == 0 and z["inertia"].shape == (0, 4)
        if refine == "none":
            assert got.names == tm.names and co.same(got.levels, tm.levels) and got.counts.tolist() == tm.counts.tolist()
        else:
            labels = np.asarray([tm.names[b] for b in best[:, 0]])
            want, winfo = bt.dba_templates(fp[use], counts[use], labels, band=4, iters=2, align=do.align)
            assert got.names == want.names and co.same(got.levels, want.levels) and got.counts.tolist() == want.counts.tolist()
        # the assignments: a line per fingerprint, the last column empty outside the sample
        with open(acsv) as fh:
            lines = [ln.rstrip("\n").split(",") for ln in fh]
        assert lines[0] == ["read_id", "cluster", "dtw_dist", "cluster_second", "dtw_dist_second", "dtw_margin", "in_sample", "silhouette"]
        assert len(lines) == 41 and [ln[0] for ln in lines[1:]] == ids.tolist()
        assert lines[1 + 7][1:] == ["", "", "", "", "", "0", ""] and lines[1 + 11][1:] == ["", "", "", "", "", "0", ""]
        in_sample = set(info["sample_index"].tolist())
        for u, p in enumerate(use):
            ln = lines[1 + p]
            assert ln[1] == tm.names[best[u, 0]] and float(ln[2]) == bd[u, 0] and ln[3] == tm.names[best[u, 1]] and float(ln[4]) == bd[u, 1]
            assert float(ln[5]) == bd[u, 1] - bd[u, 0] and ln[6] == str(int(p in in_sample)) and (ln[7] != "") == (p in in_sample)
            if p in in_sample:
                assert float(ln[7]) == info["silhouette"][info["sample_index"].tolist().index(p)]
        assert not eng.mem
    assert isinstance(got, Templates)
