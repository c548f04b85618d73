// np_sum.h -- np.add.reduce of a float64 (or, with float accumulators, float32) array in numpy's order, by one workgroup (a wave, or several)
// (trace_peaks_api.h: np.nanstd; mvs_api.h: np.mean / np.var of float64 input; sigstats_api.h: both types).
#pragma once
#include "common.h"

#define LP_MAXLEAF 136 // leaves of numpy's pairwise tree over one 8192-element buffer (each leaf > 56 elements: at most 147; 128 for 8192)

// ---------------------------------------------------------------- numpy's add.reduce order, one wave
// np.add.reduce over a contiguous array of A (double, float): buffers of <= 8192 elements added in sequence to 0.0, each summed by the
// pairwise recursion (numpy/_core/src/umath/loops_utils.h.src pairwise_sum: a node longer than 128 splits at
// n2 = n / 2 - (n / 2) % 8; a leaf of >= 8 elements uses 8 interleaved accumulators).  The leaves are summed by the threads of
// the workgroup in parallel, the tree is combined by thread 0 with a stack in LDS (no private arrays: no scratch).
template <class A> struct NpSumLdsT {
    int loff[LP_MAXLEAF];
    A lsum[LP_MAXLEAF];
    int so[16], sn[16], sph[16];
    A val[16];
    A out;
};
typedef NpSumLdsT<double> NpSumLds;

// the leaf of numpy's tree over [0, nb) that holds position p: (offset, length)
static __device__ __forceinline__ int2 np_leaf_of(int nb, int p)
{
    int o = 0, n = nb;
    while (n > 128) {
        int n2 = n / 2;
        n2 -= n2 % 8;
        if (p < o + n2) n = n2;
        else { o += n2; n -= n2; }
    }
    return make_int2(o, n);
}

template <class A = double, class F>
static __device__ __forceinline__ A np_pw_leaf(int o, int n, F get)
{
    if (n < 8) {
        A res = (A)0;
        for (int i = 0; i < n; i++) res += get(o + i);
        return res;
    }
    A r0 = get(o), r1 = get(o + 1), r2 = get(o + 2), r3 = get(o + 3), r4 = get(o + 4), r5 = get(o + 5), r6 = get(o + 6), r7 = get(o + 7);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += get(o + i); r1 += get(o + i + 1); r2 += get(o + i + 2); r3 += get(o + i + 3);
        r4 += get(o + i + 4); r5 += get(o + i + 5); r6 += get(o + i + 6); r7 += get(o + i + 7);
    }
    A res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; i++) res += get(o + i);
    return res;
}

// sum of get(k), k in [0, n), in numpy's order, accumulated in A (what get returns).  Uniform call of the whole workgroup; every thread gets the result.
template <class F, class A>
static __device__ A np_sum_wave(long n, F get, LDS NpSumLdsT<A> *s)
{
    const int ln = threadIdx.x, nt = blockDim.x;
    A t = (A)0;
    for (long b0 = 0; b0 < n; b0 += 8192) {
        const int nb = (int)(n - b0 < 8192 ? n - b0 : 8192);
        auto gb = [&](int k) { return get(b0 + k); };
        // the leaves, in order (every thread walks them alike: <= 7 levels per leaf)
        int nl = 0;
        for (int p = 0; p < nb; nl++) {
            const int2 lf = np_leaf_of(nb, p);
            if (ln == 0) s->loff[nl] = lf.x;
            p = lf.x + lf.y;
        }
        __syncthreads();
        for (int k = ln; k < nl; k += nt) {
            const int o = s->loff[k], e = (k + 1 < nl) ? s->loff[k + 1] : nb;
            s->lsum[k] = np_pw_leaf<A>(o, e - o, gb);
        }
        __syncthreads();
        if (ln == 0) {
            // post-order over the tree: (offset, length, phase) frames, finished subtrees on a value stack
            int sp = 1, rs = 0, leaf = 0;
            s->so[0] = 0; s->sn[0] = nb; s->sph[0] = 0;
            while (sp > 0) {
                sp--;
                const int o = s->so[sp], nn = s->sn[sp];
                if (s->sph[sp]) { const A rr = s->val[--rs], ll = s->val[--rs]; s->val[rs++] = ll + rr; continue; }
                if (nn <= 128) { s->val[rs++] = s->lsum[leaf++]; continue; }
                int n2 = nn / 2;
                n2 -= n2 % 8;
                s->so[sp] = o; s->sn[sp] = nn; s->sph[sp] = 1; sp++;
                s->so[sp] = o + n2; s->sn[sp] = nn - n2; s->sph[sp] = 0; sp++;
                s->so[sp] = o; s->sn[sp] = n2; s->sph[sp] = 0; sp++;
            }
            s->out = s->val[0];
        }
        __syncthreads();
        t += s->out;
        __syncthreads();
    }
    return t;
}
