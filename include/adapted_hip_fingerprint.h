/* adapted_hip_fingerprint.h -- adapter event fingerprints and their comparison by dynamic time warping (an EXTENSION: the
 * reference has no such step; its README sends its users to a sister tool that tells barcoded adapters apart by the levels of
 * the adapter's events).  Part of the C ABI of include/adapted_hip.h, which includes this file (inside its extern "C" block,
 * behind its types, its flags and adapted_hip_events.h): include that one.  adapted_amd/lib.py restates these prototypes in
 * FINGERPRINT_PROTOTYPES; tests/test_fingerprint_cpu.py holds that table against this header.  The parameters are untuned and
 * no real data has been through either call: whether such fingerprints separate real barcodes is not claimed.
 *
 * adp_event_levels: the event table and a normalised fixed-width fingerprint of n_seg segments.  sig, len, n_reads, L, segs,
 * n_seg, args, ADP_IN_DEVICE and ADP_MVS_F64 are adp_segment_events' (adapted_hip_events.h), with its clipping and its checks;
 * 2 <= max_events = E <= 512, else ADP_ERR_INVALID before anything is launched.  Per clipped segment x of n samples:
 *   the status, the boundaries b and the gap statistics are adp_segment_events' (info_out and stats_out hold its bytes);
 *   with more than E - 1 boundaries the E - 1 greatest in the total order (score[b], b) stay -- the higher score first, the later
 *   index on equal scores --, in index order;
 *   edges = 0, the boundaries that stay, n; count = their number + 1 (a segment without a boundary is one event);
 *   lengths[e] = edge[e + 1] - edge[e]; levels[e] = np.mean(x[edge[e]:edge[e + 1]].astype(np.float64)) (numpy's add.reduce order);
 *   med = np.median(levels[:count]), mad = np.median(np.abs(levels[:count] - med)), fp[e] = (levels[e] - med) / mad, float64;
 *   fpstatus: 0 fine; 1 and 2 as the segmentation's (then count = 0); 4 mad == 0, or med or mad not finite (count, lengths and
 *   levels stay, fp is all NaN).  Entries at and beyond count: NaN in levels and fp, 0 in lengths.
 * Outputs, host memory: info_out int64 [n_seg, 2], stats_out double [n_seg, 2], count_out int32 [n_seg], fpstatus_out int32
 * [n_seg], lengths_out int32 [n_seg, E], levels_out double [n_seg, E], fp_out double [n_seg, E], norm_out double [n_seg, 2] (med,
 * mad); lengths_out, levels_out and norm_out may be NULL.  With ADP_OUT_DEVICE fp_out and count_out are device pointers (they
 * stay there for adp_dtw_assign); everything else is host memory.  The call completes before it returns.
 *
 * adp_dtw_assign: the DTW distance of nq queries q [nq, Eq] with q_count [nq] (host, or both device pointers with
 * ADP_IN_DEVICE) to nt templates t [nt, Et] with t_count [nt] (host), and the nearest two templates of every query.
 * 1 <= Eq, Et <= 512, 1 <= nt <= 4096, every t_count in [1, Et], every template value inside its count finite, band >= 0 (else
 * ADP_ERR_INVALID before anything is launched; the handle stays usable).  For a = q[p, :n] and c = t[k, :m], float64 as written:
 *   D[0][0] = 0, every other D[0][j] and D[i][0] = +inf; R = max(band, |n - m|) with band > 0, no limit with band == 0;
 *   D[i][j] = d * d + min(min(D[i-1][j], D[i][j-1]), D[i-1][j-1]) with d = a[i-1] - c[j-1] for |i - j| <= R, +inf elsewhere;
 *   dist[p][k] = D[n][m].
 * A query whose count lies outside [1, Eq], or that holds a value that is not finite inside its count, has NaN distances.
 * Outputs, host memory: dist_out double [nq, nt] (may be NULL); best_out int32 [nq, 2] -- the template of the least distance, the
 * lowest index on ties, and of the second least, -1 where there is none --; bestdist_out double [nq, 2], NaN where -1.  The distance
 * matrix is made in batches of queries within a byte budget (512 MiB; ADP_DTW_SCRATCH_MIB in the environment replaces it, read
 * per call).  The call completes before it returns. */
#ifndef ADAPTED_HIP_FINGERPRINT_H
#define ADAPTED_HIP_FINGERPRINT_H

int adp_event_levels(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                     const adp_event_args *args, int flags, int max_events, int64_t *info_out, double *stats_out, int32_t *count_out,
                     int32_t *fpstatus_out, int32_t *lengths_out, double *levels_out, double *fp_out, double *norm_out);
int adp_dtw_assign(adp_handle *h, const double *q, const int32_t *q_count, int nq, int Eq, const double *t, const int32_t *t_count,
                   int nt, int Et, int band, int flags, double *dist_out, int32_t *best_out, double *bestdist_out);

#endif /* ADAPTED_HIP_FINGERPRINT_H */
