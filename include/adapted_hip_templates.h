/* adapted_hip_templates.h -- building barcode templates: the warping path of a DTW alignment and one iteration of DTW barycentre
 * averaging, DBA (an EXTENSION, as adapted_hip_fingerprint.h is, whose adp_dtw_assign uses such templates).  Part of the C ABI of
 * include/adapted_hip.h, which includes this file (inside its extern "C" block, behind its types, its flags and
 * adapted_hip_fingerprint.h): include that one.  adapted_amd/lib.py restates these prototypes in TEMPLATE_PROTOTYPES;
 * tests/test_dtw_align_cpu.py holds that table against this header.  Nothing here is tuned and no real data has been through
 * either call: whether such templates separate real barcodes is not claimed.
 *
 * adp_dtw_align: every query q[p] of q [nq, Eq] with q_count [nq] (host, or both device pointers with ADP_IN_DEVICE) against ONE
 * template, t[which[p]] of t [nt, Et] with t_count [nt]; which [nq], t and t_count are host arrays.  which[p] == -1: the query is
 * skipped.  adp_dtw_assign's conditions hold (1 <= Eq, Et <= 512, 1 <= nt <= 4096, every t_count in [1, Et], every template value
 * inside its count finite, band >= 0), and every which[p] lies in [-1, nt): else ADP_ERR_INVALID before anything is launched; the
 * handle stays usable.  For a = q[p, :n], n = q_count[p], and c = t[k, :m], m = t_count[k], k = which[p], float64 as written:
 *   D is adp_dtw_assign's matrix: D[0][0] = 0, every other D[0][j] and D[i][0] = +inf; R = max(band, |n - m|) with band > 0, no
 *   limit with band == 0; D[i][j] = d * d + min(min(D[i-1][j], D[i][j-1]), D[i-1][j-1]) with d = a[i-1] - c[j-1] for |i - j| <= R,
 *   +inf elsewhere; dist[p] = D[n][m], the bits of adp_dtw_assign's dist[p][k].
 *   status[p]: 0 fine; 1 n outside [1, Eq] or a value that is not finite inside the count (dist NaN); 2 D[n][m] is not finite
 *   (dist is that value); 3 skipped (dist NaN; a skipped query is not looked at).
 *   The path, status 0 only, from (n, m) back to (1, 1): at i == 1 to (i, j - 1), at j == 1 to (i - 1, j), elsewhere to the
 *   predecessor of the least D -- on equal values (i - 1, j - 1) first, then (i - 1, j), then (i, j - 1).  Every template
 *   position j (0-based) holds a run of query indices: lo[p][j] the first and hi[p][j] the last (0-based), and
 *   sum[p][j] = a[lo] + a[lo + 1] + ... + a[hi], added from the left.  At and beyond m, and in every position of a query whose
 *   status is not 0: lo = hi = -1, sum NaN.
 * Outputs, host memory: dist_out double [nq], status_out int32 [nq]; lo_out, hi_out int32 [nq, Et] and sum_out double [nq, Et] may
 * be NULL.  The queries go in batches within adp_dtw_assign's byte budget (512 MiB; ADP_DTW_SCRATCH_MIB in the environment
 * replaces it, read per call), which covers the paths' outputs and the direction codes of the batch.  The call completes before it
 * returns.
 *
 * adp_dba_step: one DBA iteration over the same inputs, wholly on the device.  For every template k, with p0 < p1 < ... the
 * queries of status 0 whose which is k, and m = t_count[k]:
 *   T[j] = 0.0 + sum[p0][j] + sum[p1][j] + ..., one add per member in that order; N[j] = the sum of hi[p][j] - lo[p][j] + 1;
 *   t_new[k][j] = T[j] / N[j] for j < m; members[k] = their number; inertia[k] = 0.0 + dist[p0] + dist[p1] + ....
 *   A template without a member: t_new[k][j] = t[k][j] for j < m, members 0, inertia 0.0.  At and beyond m t_new is NaN.
 * The batches of the byte budget change no bit of any of this.  Outputs, host memory: t_new_out double [nt, Et], members_out int32
 * [nt], inertia_out double [nt]; dist_out double [nq] may be NULL.  The call completes before it returns. */
#ifndef ADAPTED_HIP_TEMPLATES_H
#define ADAPTED_HIP_TEMPLATES_H

int adp_dtw_align(adp_handle *h, const double *q, const int32_t *q_count, const int32_t *which, int nq, int Eq, const double *t,
                  const int32_t *t_count, int nt, int Et, int band, int flags, double *dist_out, int32_t *status_out, int32_t *lo_out,
                  int32_t *hi_out, double *sum_out);
int adp_dba_step(adp_handle *h, const double *q, const int32_t *q_count, const int32_t *which, int nq, int Eq, const double *t,
                 const int32_t *t_count, int nt, int Et, int band, int flags, double *t_new_out, int32_t *members_out,
                 double *inertia_out, double *dist_out);

#endif /* ADAPTED_HIP_TEMPLATES_H */
