/* adapted_hip_clusters.h -- clustering fingerprints without labels: the all-pairs DTW matrix of a set of fingerprints, PAM's BUILD,
 * alternating k-medoids and the silhouette, on a matrix that may stay on the device from the first call to the last (an EXTENSION,
 * as adapted_hip_fingerprint.h is, whose adp_dtw_assign defines the distance).  Part of the C ABI of include/adapted_hip.h, which
 * includes this file (inside its extern "C" block, behind its types, its flags and adapted_hip_templates.h): include that one.
 * adapted_amd/lib.py restates these prototypes in CLUSTER_PROTOTYPES; tests/test_clusters_cpu.py holds that table against this
 * header; tests/dtw_cluster_oracle.py restates every rule below in numpy.  Untuned, nothing validated on real data: whether
 * fingerprints of real barcodes separate is what these calls let a user find out, not something they claim.
 *
 * Every call refuses what it does not take with ADP_ERR_INVALID before anything is launched (the matrix check of the last three
 * runs on the device, before anything else); the handle stays usable.  Every call completes before it returns.  No result depends on
 * scheduling: there are no float atomics.
 *
 * THE ORDER of every float64 sum over columns (or, for the cost, over rows) below: 64 partial sums; partial l adds, from +0.0, the
 * terms of the indices j = l (mod 64) in ascending j -- an index outside the set that is summed contributes nothing, which for these
 * non-negative terms is the same as adding +0.0 --; then the partials are folded, p[l] += p[l + s] for every l < s, for s = 32, 16,
 * 8, 4, 2, 1; the sum is p[0].
 *
 * adp_dtw_pairwise: q double [n, E] with q_count int32 [n] (host, or both device pointers with ADP_IN_DEVICE); 1 <= E <= 512,
 * 1 <= n <= 16384, band >= 0.  dist_out double [n, n], host memory, or device memory with ADP_OUT_DEVICE.
 *   dist[i][j], i != j, is bit for bit adp_dtw_assign's distance of query i to template j (adapted_hip_fingerprint.h: the same
 *   D[i][j] = d * d + min(min(D[i-1][j], D[i][j-1]), D[i-1][j-1]), the same R = max(band, |n_i - n_j|) with band > 0).  That
 *   recurrence is symmetric in its operands to the bit -- (a - c) * (a - c) and (c - a) * (c - a) are one value, and the least of
 *   the same three values is taken --, so every unordered pair is computed once and dist[j][i] is a copy of dist[i][j].
 *   dist[i][i] = +0.0.  A row adp_dtw_assign would give NaN distances (a count outside [1, E], a value that is not finite inside
 *   its count) has a NaN row and column, the diagonal included.
 *   Scratch is needed for a host matrix only (ADP_DTW_SCRATCH_MIB, adp_dtw_assign's byte budget, read per call): the whole matrix
 *   where it fits, else bands of its rows, in which a pair is computed once per band that holds one of its rows -- the same bits.
 *
 * The three calls below take dist double [n, n], host memory, or device memory with ADP_IN_DEVICE, 1 <= n <= 16384, and refuse a
 * matrix that holds a NaN, a negative value or an infinity.  They read rows only (row i for the distances of i): the matrix is
 * taken to be symmetric.  Every other array is host memory.
 *
 * adp_kmedoids_build: PAM's BUILD, deterministic; 1 <= kmax <= min(n, 4096).  medoids_out int32 [kmax], gain_out double [kmax].
 *   medoids[0] = the row i of the least sum over j of D[i][j] (THE ORDER), the lowest index on ties; gain[0] = that sum.
 *   With dmin[j] = the least D[m][j] over the medoids m so far: medoids[c] = the row i that is no medoid yet with the greatest
 *   gain_i = the sum over j of max(dmin[j] - D[i][j], 0.0) (THE ORDER), the lowest index on ties; gain[c] = that gain.
 *   A choice depends on the medoids before it only: the first K entries are BUILD's answer for every K <= kmax, to the bit.
 *
 * adp_kmedoids: alternating k-medoids from given medoids; 1 <= k <= min(n, 4096), 0 <= max_iter <= 2^20; medoids_io int32 [k]: k
 *   different rows, replaced by the final ones.
 *   Assignment: a medoid belongs to its own slot; every other row i to the slot c of the least D[i][medoids[c]], the lowest slot on
 *   ties (duplicate rows therefore never empty a cluster).  cost = the sum over i of D[i][medoids[assign[i]]] (THE ORDER, over i).
 *   sums[i][c] = the sum of D[i][j] over the members j of c (THE ORDER).  Update: slot c's medoid becomes its member i of the least
 *   sums[i][c], the lowest index on ties.  An update that changes no medoid ends the call and is not counted; so does the
 *   max_iter-th update that changes one.  iters_out[0] = the updates counted; cost_out double [max_iter + 1], of which
 *   [0, iters] are written: the cost before each counted update and of the final state.  assign_out int32 [n] and sums_out double
 *   [n, k] (may be NULL) are the final medoids' assignment and its sums.
 *
 * adp_silhouette: assign int32 [n] with every value in [0, k) and no cluster empty, 1 <= k <= min(n, 4096); sil_out double [n].
 *   With sums as above and size[c] the members of c: a = sums[i][own] / (size[own] - 1); b = the least sums[i][c] / size[c] over
 *   the other clusters c; sil[i] = (b - a) / max(a, b).  sil[i] = 0.0 for a cluster of one, where max(a, b) == 0, and for every
 *   row with k == 1 (scikit-learn's conventions). */
#ifndef ADAPTED_HIP_CLUSTERS_H
#define ADAPTED_HIP_CLUSTERS_H

int adp_dtw_pairwise(adp_handle *h, const double *q, const int32_t *q_count, int n, int E, int band, int flags, double *dist_out);
int adp_kmedoids_build(adp_handle *h, const double *dist, int n, int kmax, int flags, int32_t *medoids_out, double *gain_out);
int adp_kmedoids(adp_handle *h, const double *dist, int n, int k, int max_iter, int flags, int32_t *medoids_io, int32_t *assign_out,
                 double *sums_out, double *cost_out, int32_t *iters_out);
int adp_silhouette(adp_handle *h, const double *dist, int n, const int32_t *assign, int k, int flags, double *sil_out);

#endif /* ADAPTED_HIP_CLUSTERS_H */
