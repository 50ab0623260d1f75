// Admixture proportions (gpca_admix_init, gpca_admix_step, gpca_admix; gpca_admix.cpp; include/gpca.h section a21): one EM step of the
// ADMIXTURE model reads the kept rows' genotypes once and reduces the same per-genotype quantities a = g / p1 and b = (2 - g) / p0 over
// both axes: over the rows for Q, over the samples for F, with the log-likelihood beside them.
//
// k_admix_step: workgroup w owns the chunk w % chunks of kAdmChunk samples and the block w / chunks of kAdmRowBlock kept rows
// (adm_plan in plan_math.h) and walks the block in tiles of kAdmTile rows.  Per tile:
//   1. the tile's f and 1 - f go to LDS; thread t, which owns sample chunk * kAdmChunk + t and keeps its q in registers, fetches its
//      kAdmTile calls, forms p1 and p0 (k ascending, fmaf), a and b, adds a f_k and then b (1 - f_k) to its register sums S_k (the Q side,
//      rows ascending), adds its log-likelihood terms to an f64 register, and leaves a and b in LDS [row][sample];
//   2. the same threads as kAdmTile rows x kAdmGroups groups: thread (row, group) adds a q_k and b q_k over its group's
//      kAdmGroupSamples samples, ascending, with q from LDS (zero for a mode-2 sample and past N);
//   3. the groups' sums go to LDS over the a and b tiles, are added groups ascending, and the chunk's sums are written to the slab fpart.
// At the end a thread writes S_k to the slab qpart, and thread 0 adds the 256 f64 sums, ascending, into llpart.
// k_admix_f_update and k_admix_q_update add the slabs, chunks (blocks) ascending, and apply a21's updates; k_admix_sum64 adds f64 partials
// in a fixed strided order.  No atomic touches a floating-point sum (the two integer counts of a22's hold-out step alone go through integer
// atomics), and no order depends on anything but (rows, N, K): int8 and 2-bit rows run the same
// arithmetic on the same decoded calls.  Every product that enters a sum is an explicit fmaf; everything else is compiled without
// contraction.  Registers and LDS: the figures hipcc reports are in DESIGN section 7.
#include "syrk_tile.h"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace gpca {

constexpr float kAdmEps = 1e-5f;
constexpr float kAdmHi = 1.0f - 1e-5f;

// HOLD (a22's hold-out step): an observed call whose fold is `fold` counts nothing in any of the sums above; its log terms at the same
// p1 and p0 go to a second f64 register (same order), and two integer counters take the held calls and the heterozygous ones among them.
// llpart is then [partial][2], and the workgroup's counts are added to cvcnt [2] with one integer atomicAdd each.
template <bool PACKED, int KP, bool HOLD>
__global__ __launch_bounds__(kAdmThreads) void k_admix_step(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows,
                                                            int64_t rows, int64_t N, int K, int64_t chunks, const float* __restrict__ Q,
                                                            const float* __restrict__ F, const uint8_t* __restrict__ mode,
                                                            float* __restrict__ fpart, float* __restrict__ qpart, double* __restrict__ llpart,
                                                            unsigned long long* __restrict__ bad, uint32_t folds, uint32_t fold,
                                                            uint64_t cv_seed, unsigned long long* __restrict__ cvcnt) {
    __shared__ float s_ab[2 * kAdmTile * kAdmPitch];
    __shared__ float s_q[kAdmChunk * KP];
    __shared__ float s_f[2][kAdmTile * KP];
    __shared__ double s_ll[kAdmThreads];
    const int t = threadIdx.x;
    const int64_t chunk = (int64_t)blockIdx.x % chunks, block = (int64_t)blockIdx.x / chunks;
    const int64_t n = chunk * kAdmChunk + t;
    const bool live = n < N;
    const uint8_t* G = (const uint8_t*)Gv;

    float q[KP], S[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) { q[k] = (live && k < K) ? Q[n * K + k] : 0.0f; S[k] = 0.0f; }
    const bool contrib = live && (!mode || mode[n] != 2);
#pragma unroll
    for (int k = 0; k < KP; ++k) s_q[t * KP + k] = contrib ? q[k] : 0.0f;
    double ll = 0.0;
    [[maybe_unused]] double hl = 0.0;
    [[maybe_unused]] unsigned n_held = 0u, n_het = 0u;

    const int64_t ka = block * kAdmRowBlock, kb = ka + kAdmRowBlock < rows ? ka + kAdmRowBlock : rows;
    for (int64_t i0 = ka; i0 < kb; i0 += kAdmTile) {
        for (int e = t; e < kAdmTile * KP; e += kAdmThreads) {
            const int r = e / KP, k = e % KP;
            const bool in = i0 + r < kb && k < K;
            const float v = in ? F[(i0 + r) * K + k] : 0.0f;
            s_f[0][e] = v;
            s_f[1][e] = in ? 1.0f - v : 0.0f;
        }
        // the calls of the tile: 0, 1, 2; anything else (missing, past the block, past N) counts nothing
        unsigned c[kAdmTile];
#pragma unroll
        for (int r = 0; r < kAdmTile; ++r) {
            c[r] = kMissingByte;
            if (live && i0 + r < kb) {
                const int64_t orow = krows[i0 + r];
                c[r] = call_at<PACKED>(G, ldr, orow, n);
                if (!PACKED && c[r] > 2u && c[r] != kMissingByte) atomicMin(bad, (unsigned long long)orow);
            }
        }
        [[maybe_unused]] unsigned held = 0u;                                         // bit r: the call of row i0 + r is observed and held out
        if constexpr (HOLD) {
            if (live)
#pragma unroll
                for (int qd = 0; qd < kAdmTile / kAdmCvQuad; ++qd) {
                    const philox_out o = philox4x32_10((uint32_t)n, (uint32_t)((i0 >> 2) + qd), 0u, GPCA_STREAM_ADMIX_CV, (uint32_t)cv_seed, (uint32_t)(cv_seed >> 32));
#pragma unroll
                    for (int x = 0; x < kAdmCvQuad; ++x)
                        if (c[qd * kAdmCvQuad + x] <= 2u && adm_cv_fold_of(o.v[x], folds) == fold) held |= 1u << (qd * kAdmCvQuad + x);
                }
        }
        __syncthreads();                                                             // (and the sums of the tile before have left s_ab)
#pragma unroll 2
        for (int r = 0; r < kAdmTile; ++r) {
            const float* f = &s_f[0][r * KP];
            const float* omf = &s_f[1][r * KP];
            float p1 = 0.0f, p0 = 0.0f;
#pragma unroll
            for (int k = 0; k < KP; ++k) { p1 = fmaf(q[k], f[k], p1); p0 = fmaf(q[k], omf[k], p0); }
            bool obs = c[r] <= 2u;
            if constexpr (HOLD) {
                if ((held >> r) & 1u) {
                    const float h1 = (float)c[r], h0 = 2.0f - (float)c[r];
                    if (h1 > 0.0f) hl += (double)h1 * (double)logf(p1);
                    if (h0 > 0.0f) hl += (double)h0 * (double)logf(p0);
                    ++n_held;
                    n_het += c[r] == 1u ? 1u : 0u;
                    obs = false;
                }
            }
            const float w1 = obs ? (float)c[r] : 0.0f, w0 = obs ? 2.0f - (float)c[r] : 0.0f;
            const float a = w1 > 0.0f ? w1 / p1 : 0.0f, b = w0 > 0.0f ? w0 / p0 : 0.0f;
            if (w1 > 0.0f) ll += (double)w1 * (double)logf(p1);
            if (w0 > 0.0f) ll += (double)w0 * (double)logf(p0);
#pragma unroll
            for (int k = 0; k < KP; ++k) { S[k] = fmaf(a, f[k], S[k]); S[k] = fmaf(b, omf[k], S[k]); }
            s_ab[r * kAdmPitch + t] = a;
            s_ab[(kAdmTile + r) * kAdmPitch + t] = b;
        }
        __syncthreads();
        {
            const int r = t % kAdmTile, g = t / kAdmTile;
            float AQ[KP], BQ[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) { AQ[k] = 0.0f; BQ[k] = 0.0f; }
            for (int jj = 0; jj < kAdmGroupSamples; ++jj) {
                const int j = g * kAdmGroupSamples + jj;
                const float a = s_ab[r * kAdmPitch + j], b = s_ab[(kAdmTile + r) * kAdmPitch + j];
#pragma unroll
                for (int k = 0; k < KP; ++k) { AQ[k] = fmaf(a, s_q[j * KP + k], AQ[k]); BQ[k] = fmaf(b, s_q[j * KP + k], BQ[k]); }
            }
            __syncthreads();                                                         // every a and b was read: the tiles take the partials
#pragma unroll
            for (int k = 0; k < KP; ++k) {                                           // [k][a or b][group][row] = [k][a or b][t]
                s_ab[(k * 2 + 0) * kAdmThreads + t] = AQ[k];
                s_ab[(k * 2 + 1) * kAdmThreads + t] = BQ[k];
            }
        }
        __syncthreads();
        for (int e = t; e < kAdmTile * 2 * K; e += kAdmThreads) {
            const int r = e / (2 * K), cc = e % (2 * K), ab = cc / K, k = cc % K;
            float s = 0.0f;
            for (int g = 0; g < kAdmGroups; ++g) s += s_ab[((k * 2 + ab) * kAdmGroups + g) * kAdmTile + r];
            if (i0 + r < kb) fpart[adm_fpart_index(chunk, rows, i0 + r, ab, K, k)] = s;
        }
    }
    if (live)
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) qpart[adm_qpart_index(block, N, n, K, k)] = S[k];
    s_ll[t] = ll;
    __syncthreads();
    if constexpr (!HOLD) {
        if (t == 0) {
            double s = 0.0;
            for (int i = 0; i < kAdmThreads; ++i) s += s_ll[i];
            llpart[adm_llpart_index(block, chunks, chunk)] = s;
        }
    } else {
        __shared__ unsigned s_cnt[2];
        if (t == 0) {
            double s = 0.0;
            for (int i = 0; i < kAdmThreads; ++i) s += s_ll[i];
            llpart[adm_cv_llpart_index(block, chunks, chunk, 0)] = s;
            s_cnt[0] = 0u; s_cnt[1] = 0u;
        }
        __syncthreads();
        s_ll[t] = hl;
        if (n_held) atomicAdd(&s_cnt[0], n_held);                                    // at most kAdmRowBlock per thread: the sums fit 32 bits
        if (n_het) atomicAdd(&s_cnt[1], n_het);
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int i = 0; i < kAdmThreads; ++i) s += s_ll[i];
            llpart[adm_cv_llpart_index(block, chunks, chunk, 1)] = s;
            if (s_cnt[0]) atomicAdd(&cvcnt[0], (unsigned long long)s_cnt[0]);
            if (s_cnt[1]) atomicAdd(&cvcnt[1], (unsigned long long)s_cnt[1]);
        }
    }
}

// Fn [rows][K]: a thread per entry adds the chunks' sums, ascending; num = f AQ, den = num + (1 - f) BQ, f' = clamp(num / den), or f
// where den = 0
__global__ __launch_bounds__(kAdmSumThreads) void k_admix_f_update(const float* __restrict__ fpart, const float* __restrict__ F, int64_t rows,
                                                                   int K, int64_t chunks, float* __restrict__ Fn) {
    const int64_t e = (int64_t)blockIdx.x * kAdmSumThreads + threadIdx.x;
    if (e >= rows * K) return;
    const int64_t i = e / K;
    const int k = (int)(e % K);
    float AQ = 0.0f, BQ = 0.0f;
    for (int64_t c = 0; c < chunks; ++c) { AQ += fpart[adm_fpart_index(c, rows, i, 0, K, k)]; BQ += fpart[adm_fpart_index(c, rows, i, 1, K, k)]; }
    const float f = F[e];
    const float num = f * AQ, den = num + (1.0f - f) * BQ;
    float o = f;
    if (den > 0.0f) { o = num / den; o = o < kAdmEps ? kAdmEps : o > kAdmHi ? kAdmHi : o; }
    Fn[e] = o;
}

// Qn [N][K]: a thread per sample adds the blocks' sums, ascending; t_k = q_k S_k, q'_k = max(t_k / sum t, eps) / (their sum); the row is
// kept for a mode-1 sample and where sum t = 0 (no observed call)
__global__ __launch_bounds__(kAdmSumThreads) void k_admix_q_update(const float* __restrict__ qpart, const float* __restrict__ Q,
                                                                   const uint8_t* __restrict__ mode, int64_t N, int K, int64_t blocks,
                                                                   float* __restrict__ Qn) {
    const int64_t n = (int64_t)blockIdx.x * kAdmSumThreads + threadIdx.x;
    if (n >= N) return;
    float tk[kAdmMaxK], qk[kAdmMaxK];
    float tot = 0.0f;
#pragma unroll
    for (int k = 0; k < kAdmMaxK; ++k) {
        tk[k] = 0.0f; qk[k] = 0.0f;
        if (k < K) {
            float s = 0.0f;
            for (int64_t b = 0; b < blocks; ++b) s += qpart[adm_qpart_index(b, N, n, K, k)];
            qk[k] = Q[n * K + k];
            tk[k] = qk[k] * s;
            tot += tk[k];
        }
    }
    const bool keep = (mode && mode[n] == 1) || !(tot > 0.0f);
    float s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < kAdmMaxK; ++k)
        if (k < K) { float x = tk[k] / tot; x = x > kAdmEps ? x : kAdmEps; tk[k] = x; s2 += x; }
#pragma unroll
    for (int k = 0; k < kAdmMaxK; ++k)
        if (k < K) Qn[n * K + k] = keep ? qk[k] : tk[k] / s2;
}

// out [ncomp] = the sums of part [n][ncomp] (f64), one workgroup: thread t adds the entries t, t + 256, ... ascending, thread c < ncomp the
// 256 sums of component c, ascending
__global__ __launch_bounds__(kAdmSumThreads) void k_admix_sum64(const double* __restrict__ part, int64_t n, int ncomp, double* __restrict__ out) {
    __shared__ double s_s[2][kAdmSumThreads];
    const int t = threadIdx.x;
    for (int c = 0; c < ncomp; ++c) {
        double s = 0.0;
        for (int64_t i = t; i < n; i += kAdmSumThreads) s += part[i * ncomp + c];
        s_s[c][t] = s;
    }
    __syncthreads();
    if (t < ncomp) {
        double s = 0.0;
        for (int i = 0; i < kAdmSumThreads; ++i) s += s_s[t][i];
        out[t] = s;
    }
}

// a21's init: u = ((w >> 9) + 0.5) 2^-23 of the philox word w of (index, column); Q: x_k = 0.1 + 0.9 u, q_k = x_k / sum x; F:
// f_k = clamp(freq (0.5 + u)), freq = (n_het + 2 n_hom2) / (2 n_valid) of the row's QC counts (0.5 where n_valid = 0)
__device__ __forceinline__ float adm_uniform(uint32_t stream, uint64_t index, int k, uint64_t seed) {
    const philox_out o = philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), (uint32_t)(k >> 2), stream, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((float)(o.v[k & 3] >> 9) + 0.5f) * 1.1920928955078125e-07f;
}
__global__ __launch_bounds__(kAdmSumThreads) void k_admix_init(const int64_t* __restrict__ krows, const unsigned* __restrict__ counts, int64_t rows,
                                                               int64_t N, int K, uint64_t seed, float* __restrict__ Q, float* __restrict__ F) {
    const int64_t e = (int64_t)blockIdx.x * kAdmSumThreads + threadIdx.x;
    if (e < N) {
        float x[kAdmMaxK];
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < kAdmMaxK; ++k)
            if (k < K) { x[k] = 0.1f + 0.9f * adm_uniform(GPCA_STREAM_ADMIX_Q, (uint64_t)e, k, seed); s += x[k]; }
#pragma unroll
        for (int k = 0; k < kAdmMaxK; ++k)
            if (k < K) Q[e * K + k] = x[k] / s;
    } else if (e - N < rows) {
        const int64_t i = e - N;
        const unsigned* cn = counts + 4 * krows[i];
        const float freq = cn[0] == 0u ? 0.5f : (float)(((double)cn[2] + 2.0 * (double)cn[3]) / (2.0 * (double)cn[0]));
        for (int k = 0; k < K; ++k) {
            float f = freq * (0.5f + adm_uniform(GPCA_STREAM_ADMIX_F, (uint64_t)i, k, seed));
            F[i * K + k] = f < kAdmEps ? kAdmEps : f > kAdmHi ? kAdmHi : f;
        }
    }
}

// the SQUAREM quantities of element e of (Q, then F): r = t1 - t0, v = t2 - t1 - r, in f64
struct AdmRv { double t0, r, v; };
__device__ __forceinline__ AdmRv adm_rv(const float* a0, const float* a1, const float* a2, int64_t e) {
    const double x0 = (double)a0[e], x1 = (double)a1[e], x2 = (double)a2[e];
    AdmRv o; o.t0 = x0; o.r = x1 - x0; o.v = (x2 - x1) - o.r;
    return o;
}
// npart [blocks][2] = sum r^2, sum v^2 of the block's kAdmNormBlock elements: thread t adds its elements t, t + 256, ... ascending,
// thread 0 the 256 sums
__global__ __launch_bounds__(kAdmSumThreads) void k_admix_norms(int64_t nq, int64_t nf, AdmSet t0, AdmSet t1, AdmSet t2, double* __restrict__ npart) {
    __shared__ double s_s[2][kAdmSumThreads];
    const int t = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kAdmNormBlock;
    double rr = 0.0, vv = 0.0;
    for (int64_t e = e0 + t; e < e0 + kAdmNormBlock && e < nq + nf; e += kAdmSumThreads) {
        const AdmRv x = e < nq ? adm_rv(t0.Q, t1.Q, t2.Q, e) : adm_rv(t0.F, t1.F, t2.F, e - nq);
        rr += x.r * x.r; vv += x.v * x.v;
    }
    s_s[0][t] = rr; s_s[1][t] = vv;
    __syncthreads();
    if (t < 2) {
        double s = 0.0;
        for (int i = 0; i < kAdmSumThreads; ++i) s += s_s[t][i];
        npart[2 * (int64_t)blockIdx.x + t] = s;
    }
}

// (Qx, Fx) = t0 - 2 alpha r + alpha^2 v, formed in f64 and rounded once; F clamped to [eps, 1 - eps]; a Q row clamped to >= eps and divided
// by its sum, a mode-1 row copied from t0.  Threads 0 .. N - 1 take a row of Q each, the threads after them an entry of F each.
__global__ __launch_bounds__(kAdmSumThreads) void k_admix_extrap(int64_t N, int64_t nf, int K, AdmSet t0, AdmSet t1, AdmSet t2,
                                                                 const uint8_t* __restrict__ mode, double alpha, AdmSet tx) {
    const int64_t e = (int64_t)blockIdx.x * kAdmSumThreads + threadIdx.x;
    const double c1 = 2.0 * alpha, c2 = alpha * alpha;
    if (e < N) {
        const bool fixed = mode && mode[e] == 1;
        float x[kAdmMaxK];
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < kAdmMaxK; ++k)
            if (k < K) {
                const AdmRv y = adm_rv(t0.Q, t1.Q, t2.Q, e * K + k);
                const float z = (float)((y.t0 - c1 * y.r) + c2 * y.v);
                x[k] = z > kAdmEps ? z : kAdmEps;
                s += x[k];
            }
#pragma unroll
        for (int k = 0; k < kAdmMaxK; ++k)
            if (k < K) tx.Q[e * K + k] = fixed ? t0.Q[e * K + k] : x[k] / s;
    } else if (e - N < nf) {
        const AdmRv y = adm_rv(t0.F, t1.F, t2.F, e - N);
        const float z = (float)((y.t0 - c1 * y.r) + c2 * y.v);
        tx.F[e - N] = z > kAdmEps ? (z > kAdmHi ? kAdmHi : z) : kAdmEps;
    }
}

static inline unsigned adm_blocks(int64_t n) { return (unsigned)((n + kAdmSumThreads - 1) / kAdmSumThreads); }
static inline bool adm_shape_ok(int64_t rows, int64_t N, int K) {
    return rows >= 1 && N >= 1 && K >= 1 && K <= kAdmMaxK && rows < ((int64_t)1 << 31) && N < ((int64_t)1 << 31) &&
           adm_grid(adm_plan(rows, N)) < ((int64_t)1 << 31) && (rows + N) * (int64_t)K / kAdmSumThreads < ((int64_t)1 << 31);
}

int launch_admix_step(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t rows, int64_t N, int K,
                      const float* Q, const float* F, const uint8_t* mode, float* fpart, float* qpart, double* llpart, float* Qn, float* Fn,
                      double* ll, unsigned long long* bad, const AdmHold& hold) {
    if (!adm_shape_ok(rows, N, K)) return (int)hipErrorInvalidValue;
    if (hold.folds != 0 && (hold.folds < kAdmCvMinFolds || hold.folds > kAdmCvMaxFolds || hold.fold < 0 || hold.fold >= hold.folds || !hold.counts))
        return (int)hipErrorInvalidValue;
    const AdmPlan p = adm_plan(rows, N);
    const dim3 grid((unsigned)adm_grid(p)), blk(kAdmThreads);
    const uint32_t folds = (uint32_t)hold.folds, fold = (uint32_t)hold.fold;
#define GPCA_ADM(PK, KP, HD) hipLaunchKernelGGL((k_admix_step<PK, KP, HD>), grid, blk, 0, st, G, ldr, krows, rows, N, K, p.chunks, Q, F, mode, fpart, qpart, llpart, bad, folds, fold, hold.seed, hold.counts)
    const int kp = adm_kpad(K);
    if (hold.folds == 0) {
        if (packed) { if (kp == 4) GPCA_ADM(true, 4, false); else if (kp == 8) GPCA_ADM(true, 8, false); else GPCA_ADM(true, 16, false); }
        else { if (kp == 4) GPCA_ADM(false, 4, false); else if (kp == 8) GPCA_ADM(false, 8, false); else GPCA_ADM(false, 16, false); }
    } else {
        if (packed) { if (kp == 4) GPCA_ADM(true, 4, true); else if (kp == 8) GPCA_ADM(true, 8, true); else GPCA_ADM(true, 16, true); }
        else { if (kp == 4) GPCA_ADM(false, 4, true); else if (kp == 8) GPCA_ADM(false, 8, true); else GPCA_ADM(false, 16, true); }
    }
#undef GPCA_ADM
    hipLaunchKernelGGL(k_admix_f_update, dim3(adm_blocks(rows * K)), dim3(kAdmSumThreads), 0, st, fpart, F, rows, K, p.chunks, Fn);
    hipLaunchKernelGGL(k_admix_q_update, dim3(adm_blocks(N)), dim3(kAdmSumThreads), 0, st, qpart, Q, mode, N, K, p.blocks, Qn);
    hipLaunchKernelGGL(k_admix_sum64, dim3(1), dim3(kAdmSumThreads), 0, st, llpart, adm_llpart_capacity(p), hold.folds == 0 ? 1 : 2, ll);
    return 0;
}

int launch_admix_init(hipStream_t st, const int64_t* krows, const unsigned* counts, int64_t rows, int64_t N, int K, uint64_t seed, float* Q,
                      float* F) {
    if (!adm_shape_ok(rows, N, K)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_admix_init, dim3(adm_blocks(N + rows)), dim3(kAdmSumThreads), 0, st, krows, counts, rows, N, K, seed, Q, F);
    return 0;
}

int launch_admix_norms(hipStream_t st, int64_t rows, int64_t N, int K, const AdmSet& t0, const AdmSet& t1, const AdmSet& t2, double* npart,
                       double* nrm) {
    if (!adm_shape_ok(rows, N, K)) return (int)hipErrorInvalidValue;
    const int64_t nb = adm_norm_blocks(N, rows, K);
    hipLaunchKernelGGL(k_admix_norms, dim3((unsigned)nb), dim3(kAdmSumThreads), 0, st, adm_q_capacity(N, K), adm_f_capacity(rows, K), t0, t1, t2, npart);
    hipLaunchKernelGGL(k_admix_sum64, dim3(1), dim3(kAdmSumThreads), 0, st, npart, nb, 2, nrm);
    return 0;
}

int launch_admix_extrap(hipStream_t st, int64_t rows, int64_t N, int K, const AdmSet& t0, const AdmSet& t1, const AdmSet& t2,
                        const uint8_t* mode, double alpha, const AdmSet& tx) {
    if (!adm_shape_ok(rows, N, K)) return (int)hipErrorInvalidValue;
    const int64_t nf = adm_f_capacity(rows, K);
    hipLaunchKernelGGL(k_admix_extrap, dim3(adm_blocks(N + nf)), dim3(kAdmSumThreads), 0, st, N, nf, K, t0, t1, t2, mode, alpha, tx);
    return 0;
}

}  // namespace gpca
