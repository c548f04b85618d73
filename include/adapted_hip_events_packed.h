/* adapted_hip_events_packed.h -- the packed forms of the two event calls (an EXTENSION, as adapted_hip_events.h and
 * adapted_hip_fingerprint.h are): the segments lie back to back in one array instead of inside the rows of a signal matrix, as
 * float32 pA or as the raw int16 ADC samples with a calibration per segment.  A finished run's adapters, a few thousand samples
 * of every read, reach the device that way without the reads around them (`adapted events`).  Part of the C ABI of
 * include/adapted_hip.h, which includes this file (inside its extern "C" block, behind adapted_hip_fingerprint.h): include that
 * one.  adapted_amd/lib.py restates these prototypes in EVENT_PACKED_PROTOTYPES; tests/test_events_packed_cpu.py holds that table
 * against this header.  The parameters are untuned and no real data has been through either call.
 *
 * Segment g is packed[offsets[g] : offsets[g + 1]); n = its size.  offsets: a HOST array of n_seg + 1 element offsets, int64,
 * offsets[0] >= 0, never decreasing, every segment of fewer than 2^30 samples.  Without ADP_PACKED_I16 the samples are float32 pA
 * and scale / offset are not read (they may be NULL).  With ADP_PACKED_I16 they are raw int16 ADC samples and scale / offset are
 * float32 [n_seg], one calibration per segment: x[k] = scale[g] * (float32(adc[k]) + offset[g]), both operations rounded to
 * float32 and never fused -- the bits adp_calibrate_i16 writes --, then widened to float64 as every float32 sample is.  A segment
 * starts at any element: nothing is assumed of its alignment beyond its element's.  With ADP_IN_DEVICE packed, scale and offset
 * are device pointers, else host memory.  ADP_MVS_F64 is refused: there is no float64 packed form.
 *
 * adp_segment_events_packed: args, cap and the three outputs are adp_segment_events' (adapted_hip_events.h), for x as above:
 * the same scores, boundaries, tie rules, statuses and gap statistics, to the byte.  An int16 sample is never NaN, so status 1
 * there means a calibration that is not finite.
 *
 * adp_event_levels_packed: args, max_events, the eight outputs and ADP_OUT_DEVICE (fp_out and count_out are device pointers, for
 * adp_dtw_assign) are adp_event_levels' (adapted_hip_fingerprint.h), for x as above, to the byte.
 *
 * Refused with ADP_ERR_INVALID before anything is launched (the handle stays usable): a null handle, args or required output;
 * n_seg < 1; offsets as they must not be; ADP_PACKED_I16 without scale or offset; ADP_MVS_F64; the argument ranges the two
 * matrix calls refuse.  The slots, the batches and ADP_EVENTS_SCRATCH_MIB are the matrix calls'.  Each call completes before it
 * returns. */
#ifndef ADAPTED_HIP_EVENTS_PACKED_H
#define ADAPTED_HIP_EVENTS_PACKED_H

#define ADP_PACKED_I16 (1u << 24) /* the two packed event calls: raw int16 samples with a calibration per segment */

int adp_segment_events_packed(adp_handle *h, const void *packed, const int64_t *offsets, const float *scale, const float *offset,
                              int n_seg, const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out,
                              double *stats_out);
int adp_event_levels_packed(adp_handle *h, const void *packed, const int64_t *offsets, const float *scale, const float *offset,
                            int n_seg, const adp_event_args *args, int flags, int max_events, int64_t *info_out, double *stats_out,
                            int32_t *count_out, int32_t *fpstatus_out, int32_t *lengths_out, double *levels_out, double *fp_out,
                            double *norm_out);

#endif /* ADAPTED_HIP_EVENTS_PACKED_H */
