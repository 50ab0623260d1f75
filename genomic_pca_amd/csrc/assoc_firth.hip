// The approximate Firth correction of the logistic score scan (gpca_assoc_logistic_firth; gpca_assoc_score.cpp; include/gpca.h section a15).
//
// The walk is the saddle-point correction's (assoc_spa.hip): after k_assoc_score_finish the band's (row, trait) items are taken in ranges
// of kAspListItems.  k_assoc_firth_flag (a thread per item) writes the item's normal value with status 0 and, where z is finite and
// |z| >= firth_z, takes a slot of the range's list from an atomic counter: the slot decides only which workgroup computes the item, every
// result goes to the item's own address.
// k_assoc_firth: asp_slots(N) persistent workgroups of kAspThreads threads (fewer where GPCA_ASP_SLOTS forces it: asp_clamp_slots; no
// result depends on the count) take the listed items in turn.  For an item the workgroup
//  1. stages g~ into its slice of the workspace as k_assoc_spa does (asp_stage_gt, assoc_stage.h), taking max |g~| on the way (a max
//     is exact and does not depend on the order);
//  2. runs the root rule of spa_math.h (firth_item): every pass is one sweep over g~ and mu with five running sums K .. K''''.
// Every sum over the samples: a thread adds its samples in ascending order, a wave adds its lanes by a butterfly (every lane ends with
// the same bits), the four waves' sums are added in the order (0 + 1) + (2 + 3).  The tree depends on N alone, there is no atomic on a
// sum, every thread holds the same value and takes the same branch of the root rule.  A band therefore gives the bits of the full
// call, and int8 and 2-bit residency (the same bytes in LDS) the same bits.
// Registers, LDS and scratch as hipcc reports them are in DESIGN section 7.
#include "assoc_stage.h"
#include "spa_math.h"

#pragma clang fp contract(off)

namespace gpca {

__global__ __launch_bounds__(256) void k_assoc_firth_flag(const double* __restrict__ stats, int T, int64_t item0, int64_t nitems, double firth_z,
                                                          double* __restrict__ out, int* __restrict__ list, unsigned* __restrict__ count) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nitems) return;
    const int64_t item = item0 + k;
    const double z = stats[item * 5 + 2];
    double* o = out + item * kAfiWidth;
    const double nan = __builtin_nan("");
    o[0] = spa_normal_log10p(z); o[1] = 0.0; o[2] = nan; o[3] = nan; o[4] = nan;
    if (z == z && fabs(z) != INFINITY && fabs(z) >= firth_z) list[atomicAdd(count, 1u)] = (int)k;
}

// the sums of five values over the workgroup: the same bits in every thread (red: 20 doubles)
__device__ __forceinline__ void afi_reduce5(double& a, double& b, double& c, double& d, double& e, double* red) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        a = a + __shfl_xor(a, s); b = b + __shfl_xor(b, s); c = c + __shfl_xor(c, s); d = d + __shfl_xor(d, s); e = e + __shfl_xor(e, s);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[wv] = a; red[4 + wv] = b; red[8 + wv] = c; red[12 + wv] = d; red[16 + wv] = e; }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[4] + red[5]) + (red[6] + red[7]);
    c = (red[8] + red[9]) + (red[10] + red[11]);
    d = (red[12] + red[13]) + (red[14] + red[15]);
    e = (red[16] + red[17]) + (red[18] + red[19]);
    __syncthreads();
}
// the largest of a non-negative value over the workgroup
__device__ __forceinline__ double afi_max(double a, double* red) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) a = fmax(a, __shfl_xor(a, s));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) red[wv] = a;
    __syncthreads();
    a = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return a;
}

struct AfiEval {
    const double* g;
    const double* mu;
    int64_t npad;
    double* red;
    __device__ void operator()(double beta, double& k0, double& k1, double& k2, double& k3, double& k4) const {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
        for (int64_t n = threadIdx.x; n < npad; n += kAspThreads) {
            const double gg = g[n], m = mu[n];
            double t1, t2, t3, t4;
            firth_terms1234(gg, m, beta, t1, t2, t3, t4);
            s0 = s0 + spa_term0(gg, m, beta);
            s1 = s1 + t1; s2 = s2 + t2; s3 = s3 + t3; s4 = s4 + t4;
        }
        afi_reduce5(s0, s1, s2, s3, s4, red);
        k0 = s0; k1 = s1; k2 = s2; k3 = s3; k4 = s4;
    }
};

// out [rows][T][kAfiWidth] of the band that starts at kept row row0; list [*count]: the flagged items of the range that starts at item0
template <bool PACKED>
__global__ __launch_bounds__(kAspThreads) void k_assoc_firth(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows,
                                                             int64_t N, int64_t npad, const unsigned* __restrict__ incw,
                                                             const unsigned* __restrict__ sums, const double* __restrict__ dv,
                                                             const double* __restrict__ Z, const double* __restrict__ mu, int T, int Pc,
                                                             int64_t row0, int64_t item0, const int* __restrict__ list,
                                                             const unsigned* __restrict__ count, double* gws, double* out) {
    __shared__ __attribute__((aligned(16))) uint8_t sx[kAspChunk];
    __shared__ double sa[kAsrMaxCols], red[20];
    const uint8_t* G = (const uint8_t*)Gv;
    const int tid = threadIdx.x, P = Pc + 1, L = asr_cols(T, Pc);
    const unsigned cnt = *count;
    double* gw = gws + (int64_t)blockIdx.x * npad;
    for (unsigned it = blockIdx.x; it < cnt; it += gridDim.x) {                 // (block-uniform)
        const int64_t item = item0 + list[it], i = item / T;
        const int t = (int)(item - i * T);
        const int64_t orow = krows[row0 + i];
        const unsigned nobs = sums[3 * i], s1 = sums[3 * i + 1];
        const bool flip = s1 > nobs;
        const double xbar = (double)(flip ? 2u * nobs - s1 : s1) / (double)nobs;
        if (tid < P) sa[tid] = dv[i * L + asr_col_a(T, Pc, t, tid)];
        const double* Zt = Z + (int64_t)t * P * npad;
        const double* mut = mu + (int64_t)t * npad;
        double gm = 0.0;
        asp_stage_gt<PACKED>(G, ldr, orow, N, npad, incw, flip, xbar, sa, P, Zt, sx, gw, [&](int64_t, double gg) { gm = fmax(gm, fabs(gg)); });
        const double U = dv[i * L + asr_col_r(T, t)], normal = out[item * kAfiWidth];   // (the flag kernel's value; thread 0 overwrites it below)
        const double gmax = afi_max(gm, red);                                   // (its barriers make g~ visible to the workgroup)
        AfiEval ev{gw, mut, npad, red};
        FirthResult r;
        firth_item(ev, U, gmax, normal, r);
        if (tid == 0) {
            double* o = out + item * kAfiWidth;
            o[0] = r.log10p; o[1] = (double)r.status; o[2] = flip ? -r.beta : r.beta; o[3] = r.se; o[4] = r.lrt;
        }
        __syncthreads();                                                        // (sa is rewritten for the next item)
    }
}

void launch_assoc_firth_flag(hipStream_t st, const double* stats, int T, int64_t item0, int64_t nitems, double firth_z, double* out, int* list,
                             unsigned* count) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(k_assoc_firth_flag, dim3((unsigned)((nitems + 255) / 256)), dim3(256), 0, st, stats, T, item0, nitems, firth_z, out, list,
                       count);
}

int launch_assoc_firth(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const unsigned* incw,
                       const unsigned* sums, const double* dv, const double* Z, const double* mu, int T, int Pc, int64_t row0,
                       int64_t item0, const int* list, const unsigned* count, double* gws, double* out, int64_t slots) {
    if (T < 1 || Pc < 0 || asr_cols(T, Pc) > kAsrMaxCols || N < 1 || slots < 1 || slots > asp_slots(N)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)slots), blk(kAspThreads);                         // (gws keeps asp_slots(N) slices: workgroup b writes slice b)
    const int64_t npad = asp_gpad(N);
    if (packed)
        hipLaunchKernelGGL((k_assoc_firth<true>), grid, blk, 0, st, G, ldr, krows, N, npad, incw, sums, dv, Z, mu, T, Pc, row0, item0, list,
                           count, gws, out);
    else
        hipLaunchKernelGGL((k_assoc_firth<false>), grid, blk, 0, st, G, ldr, krows, N, npad, incw, sums, dv, Z, mu, T, Pc, row0, item0, list,
                           count, gws, out);
    return 0;
}

}  // namespace gpca
