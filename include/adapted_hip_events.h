/* adapted_hip_events.h -- event segmentation of signal segments (an EXTENSION: the reference has no such step; its README,
 * "Poly(A) tail length estimation", leaves the event lengths of the adapter to another tool).  Part of the C ABI of
 * include/adapted_hip.h, which includes this file (inside its extern "C" block, behind its types and flags): include that one.
 * adapted_amd/lib.py restates these prototypes in EVENT_PROTOTYPES; tests/test_events_cpu.py holds that table against this header,
 * as tests/test_host_cpu.py holds PROTOTYPES against adapted_hip.h. */
#ifndef ADAPTED_HIP_EVENTS_H
#define ADAPTED_HIP_EVENTS_H

/* adp_segment_events: the boundaries between the events of n_seg segments x = signal[row, start:end] of signals [n_reads, L]
 * float32, or float64 with ADP_MVS_F64, and the median / median absolute deviation of the event lengths
 * (adapted_amd/csrc/events_api.h).  A segment is clipped to its read as adp_seg_stats clips it (end or start beyond len[row];
 * start < 0 or end <= start gives an empty one); n = the clipped size.  Everything below is float64 in the order written:
 *   mean[j]  = (x[j] + ... + x[j + w - 1]) / w, summed left to right; var[j] = (sum over the window of (x - mean[j])^2) / w
 *   score[i] = ((mean[i - w] - mean[i])^2 * w) / max(var[i - w] + var[i], var_floor) for w <= i <= n - w, 0.0 elsewhere
 *   boundaries = scipy.signal.find_peaks(score, height=threshold, distance=min_distance)[0] (on equal heights within
 *                min_distance the later index counts as the higher)
 *   median and median(|gap - median|) of np.diff(boundaries) -- NaN with fewer than two boundaries.
 * len and segs: HOST arrays, checked as adp_seg_stats checks them; rows of fewer than 2^30 samples.  flags: ADP_IN_DEVICE -- `sig`
 * is a device pointer.  2 <= window <= 64, min_distance >= 1, threshold and var_floor finite and > 0, cap >= 0 (else
 * ADP_ERR_INVALID before anything is launched; the handle stays usable).  Outputs, host memory:
 *   pos_out   int64 [n_seg, cap]  positions from the clipped segment's start, ascending, then -1 (may be NULL with cap == 0)
 *   info_out  int64 [n_seg, 2]    the number of boundaries (also counted past cap); status: 0 fine, 1 a NaN in the clipped
 *                                 slice (no boundaries, NaN statistics; a NaN elsewhere in the row is not read), 2 n < 2 window
 *   stats_out double [n_seg, 2]   median and MAD of the gaps (every boundary counts, also those past cap)
 * The call completes before it returns. */
typedef struct adp_event_args {
    double threshold, var_floor;
    int32_t window, min_distance;
} adp_event_args;
int adp_sizeof_event_args(void);
int adp_segment_events(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                       const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out, double *stats_out);

#endif /* ADAPTED_HIP_EVENTS_H */
