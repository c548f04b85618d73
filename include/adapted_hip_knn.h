/* adapted_hip_knn.h -- the k nearest labelled fingerprints of every query under DTW: a classifier that keeps the labelled reads
 * themselves, where adp_dtw_assign keeps one template per label (an EXTENSION, as adapted_hip_fingerprint.h is, whose adp_dtw_assign
 * defines the distance).  Part of the C ABI of include/adapted_hip.h, which includes this file (inside its extern "C" block, behind
 * its types, its flags and adapted_hip_clusters.h): include that one.  adapted_amd/lib.py restates the prototype in KNN_PROTOTYPES;
 * tests/test_knn_cpu.py holds that table against this header; tests/dtw_knn_oracle.py restates every rule below in numpy.
 * Untuned, nothing validated on real data: how often a read gets its own label back is what this call lets a user find out, not
 * something it claims.
 *
 * adp_dtw_knn: q double [nq, Eq] with q_count int32 [nq] (host, or both device pointers with ADP_IN_DEVICE); r double [nr, Er] with
 * r_count int32 [nr] (host); exclude NULL, or host int32 [nq]: exclude[p] is the reference that does not count for query p, -1 for
 * none.  Refused with ADP_ERR_INVALID before anything is launched (the handle stays usable) unless nq >= 1, 1 <= Eq, Er <= 512,
 * 1 <= k <= 32 (KNN_KMAX), 1 <= nr <= 262144 (KNN_NR_MAX), band >= 0, every r_count lies in [1, Er], every reference value
 * inside its count is finite and every exclude[p] lies in [-1, nr).
 *   D(p, j) is adp_dtw_assign's distance of q[p] and r[j] to the bit (adapted_hip_fingerprint.h: the same recurrence, the same
 *   R = max(band, |n - m|) with band > 0, float64 as written there).
 *   idx_out int32 [nq, k] and dist_out double [nq, k], host memory: the k least of {(D(p, j), j): 0 <= j < nr, j != exclude[p]}
 *   in ascending lexicographic order -- the distance first, then the lower index.  +inf is an ordinary distance (it arises from
 *   overflow); NaN does not arise from finite inputs.  Entries beyond the candidates there are: -1 and NaN.  A query that
 *   adp_dtw_assign would give NaN distances (a count outside [1, Eq], a value that is not finite inside its count): all -1 and NaN.
 *   work_out, NULL or host int64 [nq, 3]: the pairs computed to the end, the pairs abandoned, the DP steps made (a pair of n and m
 *   events has n + (m - 1) / C of them, C = 1, 2, 4 or 8: the least of these that is >= ceil(Er / 64)).  It is a diagnostic and may
 *   differ from run to run; only this holds: finished + abandoned = the candidates of the query; with ADP_KNN_NO_PRUNE abandoned
 *   is 0 and the steps are all of them; an unusable query has zeros.
 *
 * A pair is abandoned only when a lower bound of D(p, j) that is valid in the recurrence's own floating-point arithmetic is STRICTLY
 * greater than a distance that is already known to be >= the query's final k-th least; idx_out and dist_out are therefore the same
 * bits with and without ADP_KNN_NO_PRUNE (every pair runs to the end), and from run to run.  The two bounds (their proofs stand
 * where they are computed, adapted_amd/csrc/dtw_knn_api.h): the endpoint bound (a[0] - c[0])^2 + (a[n-1] - c[m-1])^2 for n > 1 or
 * m > 1, and the least D over the cells the wavefront computed in its current and its previous step.
 *
 * The reference is uploaded once per call; the queries go in batches within adp_dtw_assign's byte budget (ADP_DTW_SCRATCH_MIB, read
 * per call).  A query's references are split into segments, one workgroup each, whose lists a second kernel merges: the default
 * segment makes about 8192 workgroups per batch and holds at least 256 references; ADP_KNN_SEGMENT_REFS in the environment (1 ..
 * 262144, read per call) replaces it, and ADP_KNN_CHECK_PERIOD (a power of two, 1 .. 64) the period of the abandon test.  Neither
 * changes a bit of the result.  The call completes before it returns. */
#ifndef ADAPTED_HIP_KNN_H
#define ADAPTED_HIP_KNN_H

#define ADP_KNN_NO_PRUNE (1 << 22) /* adp_dtw_knn: every pair runs to the end */
#define KNN_KMAX 32
#define KNN_NR_MAX 262144

int adp_dtw_knn(adp_handle *h, const double *q, const int32_t *q_count, int nq, int Eq, const double *r, const int32_t *r_count, int nr,
                int Er, int k, int band, int flags, const int32_t *exclude, int32_t *idx_out, double *dist_out, int64_t *work_out);

#endif /* ADAPTED_HIP_KNN_H */
