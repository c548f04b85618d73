// mvs_kernels.hip -- the MVS poly(A) module's kernels and their launchers (mvs_api.h), a translation unit of their own.
#include "mvs_api.h"

// ---------------------------------------------------------------- launchers (called by adapted_hip.hip's adp_mvs_*; C linkage, as
// they are declared there inside its extern "C" block)
extern "C" {
__attribute__((visibility("hidden"))) int mvs_launch_check(bool f64, int grid, hipStream_t st, const void *sig, const int32_t *len, int n, int L, const int64_t *ae,
                     const int64_t *pe, const adp_mvs_args &a, void *scr, int32_t *info, double *vals)
{
    if (f64) hipLaunchKernelGGL(k_mvs_check<double>, dim3(grid), dim3(64), 0, st, (const double *)sig, len, n, L, ae, pe, a, (double *)scr, info, vals);
    else hipLaunchKernelGGL(k_mvs_check<float>, dim3(grid), dim3(64), 0, st, (const float *)sig, len, n, L, ae, pe, a, (float *)scr, info, vals);
    return (int)hipGetLastError();
}

__attribute__((visibility("hidden"))) int mvs_launch_at_loc(bool f64, int grid, hipStream_t st, const void *sig, const int32_t *len, int n, int L, const int64_t *loc,
                      const adp_mvs_args &a, void *scr, int32_t *info, int64_t *idx, double *vals)
{
    if (f64) hipLaunchKernelGGL(k_mvs_at_loc<double>, dim3(grid), dim3(64), 0, st, (const double *)sig, len, n, L, loc, a, (double *)scr, info, idx, vals);
    else hipLaunchKernelGGL(k_mvs_at_loc<float>, dim3(grid), dim3(64), 0, st, (const float *)sig, len, n, L, loc, a, (float *)scr, info, idx, vals);
    return (int)hipGetLastError();
}

__attribute__((visibility("hidden"))) int mvs_launch_stream(bool f64, int grid, hipStream_t st, const void *sig, const int32_t *len, int n, int L, const adp_mvs_args &a,
                      int64_t *out)
{
    if (f64) hipLaunchKernelGGL(k_mvs_stream<double>, dim3(grid), dim3(64), 0, st, (const double *)sig, len, n, L, a, out);
    else hipLaunchKernelGGL(k_mvs_stream<float>, dim3(grid), dim3(64), 0, st, (const float *)sig, len, n, L, a, out);
    return (int)hipGetLastError();
}

} // extern "C"
