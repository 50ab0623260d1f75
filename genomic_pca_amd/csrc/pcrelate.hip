// PC-Relate (gpca_pcrelate, gpca_pcrelate_isaf; gpca_pcrelate.cpp): ancestry-adjusted kinship from caller-supplied sample coordinates.
//
// k_pcrelate_beta regresses every kept row on the design rows of the training samples (one read of the genotypes, f64 sums, one
// rounding to f32).  With beta the individual-specific allele frequency of (row i, sample n) is, in f32,
//     mu = 0.5f * (fmaf chain over j = 0 .. P of beta[i][j] * x[n][j], from 0)                              (pcr_isaf8, the ONE function
// every kernel below goes through), the entry is valid when the call is observed and tau < mu < 1 - tau, and
//     r = valid (g - 2 mu),   s = valid sqrt(mu (1 - mu)),   num_ab = sum_i r_ia r_ib,   den_ab = sum_i s_ia s_ib,   nsnp_ab = sum_i valid_ia valid_ib.
//
// k_pcrelate is a lower-triangular symmetric rank-K update over the kept rows whose operands are stored nowhere: a workgroup owns one
// 128 x 128 tile (tile row >= tile column) of ONE of the two products (blockIdx.y: 0 = num from r, 1 = den from s, with the pair count),
// 8 waves of 32 x 64.  A stage is kPcrStageRows kept rows of the 256 samples of the tile's two sides: thread t builds the operand of
// sample t % 256 for 8 consecutive rows (its design row sits in registers, the 8 beta rows are wave-uniform) and writes it to LDS as
// [sample][row] f32, rows of an 8-group permuted so that the lane's ds_read_b128 holds the rows (2 t + lane / 32), t = 0 .. 3: the four
// v_mfma_f32_32x32x2_f32 of a group then take the rows in their order, and an accumulator is bit for bit the fmaf chain over the kept
// rows of its flush group.  Two LDS buffers: the waves multiply stage s from one while stage s + 1 (its genotype bytes loaded during
// stage s - 1) is built into the other and the bytes of stage s + 2 are requested, with one barrier per stage.  Every kPcrFlushRows
// kept rows, counted from the first kept row, the f32 accumulators are added to f64 running sums held in registers; the sums depend
// on nothing but the tile, so a band gives the bits of the full call, and int8 and 2-bit residency give the same bits.
// The two products run in workgroups of their own because one wave cannot hold both: 32 x 64 outputs x (f32 accumulator + f64 running
// sum) x 2 products, with the pair counts, is 224 of the 256 registers a wave of a 512-thread workgroup has.  Each product rebuilds mu.
// The pair count is exact: nsnp_ab = K - inv_a - inv_b + sum_i inv_ia inv_ib (inv = the entry is invalid, k_pcrelate_inv counts it per
// sample), the last sum on v_mfma_i32_32x32x16_i8 and only in stages where a wave ballot finds an invalid entry on both sides.
#include "syrk_tile.h"

namespace gpca {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPcrP1Max = kPcrMaxPcs + 1;
constexpr int kPcrPitch = kPcrStageRows + 4;        // floats per sample of a staged side (ds_read_b128 stays 16-byte aligned)
constexpr int kPcrInvPitch = kPcrStageRows + 8;     // bytes per sample of the staged invalid indicator (ds_read_b64 stays 8-byte aligned)
constexpr int kPcrMissing = (int)kMissingByte;
static_assert(kPcrStageRows == 16 && kPcrThreads == 4 * kPcrTile && kPcrFlushRows / kPcrStageRows >= 1, "staging map: 2 sides x 128 samples x 2 row halves");

// The individual-specific allele frequencies of one sample at 8 consecutive kept rows: bg = the rows' coefficients [P1][8] (the same
// for every lane), x = the sample's design row.  mu[r] = 0.5f * (fmaf chain over j = 0 .. P1 - 1, from 0).
__device__ __forceinline__ void pcr_isaf8(const float* __restrict__ bg, const float (&x)[kPcrP1Max], int P1, float (&mu)[8]) {
#pragma unroll
    for (int r = 0; r < 8; ++r) mu[r] = 0.0f;
#pragma unroll
    for (int j = 0; j < kPcrP1Max; ++j) {
        if (j < P1) {
#pragma unroll
            for (int r = 0; r < 8; ++r) mu[r] = fmaf(bg[8 * j + r], x[j], mu[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) mu[r] *= 0.5f;
}
__device__ __forceinline__ bool pcr_valid(unsigned call, float mu, float tau, float one_m_tau) {
    return call != (unsigned)kPcrMissing && mu > tau && mu < one_m_tau;
}
__device__ __forceinline__ void pcr_load_x(float (&x)[kPcrP1Max], const float* __restrict__ X, int64_t n, int P1) {
#pragma unroll
    for (int j = 0; j < kPcrP1Max; ++j) x[j] = j < P1 ? X[n * P1 + j] : 0.0f;
}

// the 8 calls of one sample at kept rows kr0 .. kr0 + 7 (rows past K and samples past N: missing; a byte that is no call:
// k_pcrelate_beta reports the row)
struct PcrFetch { unsigned lo, hi; };
template <bool PACKED>
__device__ __forceinline__ void pcr_fetch(PcrFetch& F, const uint8_t* __restrict__ G, int64_t ldr, const int64_t* __restrict__ krows,
                                          int64_t K, int64_t kr0, int64_t n, bool n_ok) {
    unsigned b[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        b[r] = (unsigned)kPcrMissing;
        if (kr0 + r < K && n_ok) b[r] = call_at<PACKED>(G, ldr, krows[kr0 + r], n);
    }
    F.lo = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    F.hi = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
}

// builds the thread's 8 operands of a stage and writes them to the stage's buffers (q: sample slot 0 .. 255, hf: row half of the stage)
template <int WHICH>
__device__ __forceinline__ void pcr_put(const PcrFetch& F, const float* __restrict__ bg, const float (&x)[kPcrP1Max], int P1, float tau,
                                        float one_m_tau, int nreal, float* op, uint8_t* inv, int q, int hf) {
    float mu[8], v[8];
    pcr_isaf8(bg, x, P1, mu);
    unsigned il = 0u, ih = 0u;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const unsigned call = ((r < 4 ? F.lo : F.hi) >> (8 * (r & 3))) & 0xffu;
        const bool ok = pcr_valid(call, mu[r], tau, one_m_tau);
        if (WHICH == 0) v[r] = ok ? (float)(int)call - 2.0f * mu[r] : 0.0f;
        else {
            v[r] = ok ? sqrtf(mu[r] * (1.0f - mu[r])) : 0.0f;
            const unsigned bit = (!ok && r < nreal) ? 1u : 0u;      // (rows past K and samples past N count nowhere)
            if (r < 4) il |= bit << (8 * r); else ih |= bit << (8 * (r - 4));
        }
    }
    float* dst = op + q * kPcrPitch + 8 * hf;
    f32x4 e, o;
    e[0] = v[0]; e[1] = v[2]; e[2] = v[4]; e[3] = v[6];
    o[0] = v[1]; o[1] = v[3]; o[2] = v[5]; o[3] = v[7];
    *reinterpret_cast<f32x4*>(dst) = e;
    *reinterpret_cast<f32x4*>(dst + 4) = o;
    if (WHICH == 1) *reinterpret_cast<uint2*>(inv + q * kPcrInvPitch + 8 * hf) = make_uint2(il, ih);
}

struct PcrSmem {
    float op[2][2 * kPcrTile * kPcrPitch];
    uint8_t inv[2][2 * kPcrTile * kPcrInvPitch];
};

// R [2][E]: num (WHICH 0) and den (WHICH 1) of the band; Q [E]: sum of inv_a inv_b.  Band element (a, b <= a), row0 <= a < row1,
// a < N, at band_index(row0, a, b, true).
template <bool PACKED, int WHICH>
__device__ __forceinline__ void pcr_tile(PcrSmem& sm, const uint8_t* __restrict__ G, int64_t ldr, const int64_t* __restrict__ krows,
                                         int64_t K, int64_t N, const float* __restrict__ betaG, const float* __restrict__ X, int P1,
                                         float tau, const int2 tl, int64_t row0, int64_t row1, double* __restrict__ R, int* __restrict__ Q,
                                         int64_t E) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5, wa = wv >> 1, wb = 2 * (wv & 1);
    const int64_t ca0 = (int64_t)tl.x * kPcrTile, cb0 = (int64_t)tl.y * kPcrTile;
    const bool act0 = !(tl.x == tl.y && wb > wa), act1 = !(tl.x == tl.y && wb + 1 > wa);
    const float one_m_tau = 1.0f - tau;

    // staging: sample slot q (side a: 0 .. 127, side b: 128 .. 255), row half hf of the stage (the same for the whole wave)
    const int q = threadIdx.x & (2 * kPcrTile - 1), hf = wv >> 2;
    const int64_t n = (q < kPcrTile ? ca0 : cb0) + (q & (kPcrTile - 1));
    const bool n_ok = n < N;
    float x[kPcrP1Max];
    pcr_load_x(x, X, n, P1);       // (X has pcr_npad(N) rows, zero past N)

    f32x16 acc[2];
    i32x16 qq[2];
    double run[2][16];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc[j][e] = 0.0f; qq[j][e] = 0; run[j][e] = 0.0; }

    const int64_t nst = pcr_stages(K);
    const int a_off = (32 * wa + c) * kPcrPitch + 4 * h, b_off = (kPcrTile + 32 * wb + c) * kPcrPitch + 4 * h;
    const int ia_off = (32 * wa + c) * kPcrInvPitch + 8 * h, ib_off = (kPcrTile + 32 * wb + c) * kPcrInvPitch + 8 * h;
    auto rows_of = [&](int64_t s) { return s * kPcrStageRows + 8 * hf; };
    auto bg_of = [&](int64_t s) { return betaG + (rows_of(s) >> 3) * (int64_t)(8 * P1); };
    // (samples past N are no samples: like the rows past K they set no invalid bit, so a clean tile with padding keeps the ballot quiet)
    auto nreal_of = [&](int64_t s) { const int64_t left = K - rows_of(s); return !n_ok ? 0 : (int)(left >= 8 ? 8 : (left <= 0 ? 0 : left)); };

    PcrFetch F;
    pcr_fetch<PACKED>(F, G, ldr, krows, K, rows_of(0), n, n_ok);
    pcr_put<WHICH>(F, bg_of(0), x, P1, tau, one_m_tau, nreal_of(0), sm.op[0], sm.inv[0], q, hf);
    if (nst > 1) pcr_fetch<PACKED>(F, G, ldr, krows, K, rows_of(1), n, n_ok);
    __syncthreads();
    for (int64_t s = 0; s < nst; ++s) {
        const float* op = sm.op[s & 1];
        if (act0) {
#pragma unroll
            for (int gq = 0; gq < kPcrStageRows / 8; ++gq) {
                const f32x4 va = *reinterpret_cast<const f32x4*>(op + a_off + 8 * gq);
                const f32x4 vb0 = *reinterpret_cast<const f32x4*>(op + b_off + 8 * gq);
                const f32x4 vb1 = *reinterpret_cast<const f32x4*>(op + b_off + 32 * kPcrPitch + 8 * gq);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[t], vb0[t], acc[0], 0, 0, 0);
                    if (act1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[t], vb1[t], acc[1], 0, 0, 0);
                }
            }
            if (WHICH == 1) {
                const uint8_t* iv = sm.inv[s & 1];
                const long ia = *reinterpret_cast<const long*>(iv + ia_off);
                const long ib0 = *reinterpret_cast<const long*>(iv + ib_off);
                const long ib1 = *reinterpret_cast<const long*>(iv + ib_off + 32 * kPcrInvPitch);
                const bool anya = __builtin_amdgcn_ballot_w64(ia != 0) != 0ull;                  // wave-uniform
                const bool anyb = __builtin_amdgcn_ballot_w64((ib0 | ib1) != 0) != 0ull;
                if (anya && anyb) {
                    qq[0] = __builtin_amdgcn_mfma_i32_32x32x16_i8(ia, ib0, qq[0], 0, 0, 0);
                    if (act1) qq[1] = __builtin_amdgcn_mfma_i32_32x32x16_i8(ia, ib1, qq[1], 0, 0, 0);
                }
            }
        }
        const bool flush = (s + 1) % (kPcrFlushRows / kPcrStageRows) == 0 || s + 1 == nst;
        if (flush && act0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) { run[j][e] += (double)acc[j][e]; acc[j][e] = 0.0f; }
        }
        if (s + 1 < nst) pcr_put<WHICH>(F, bg_of(s + 1), x, P1, tau, one_m_tau, nreal_of(s + 1), sm.op[(s + 1) & 1], sm.inv[(s + 1) & 1], q, hf);
        if (s + 2 < nst) pcr_fetch<PACKED>(F, G, ldr, krows, K, rows_of(s + 2), n, n_ok);
        __syncthreads();
    }

    const int64_t a_base = ca0 + 32 * wa;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t b_col = cb0 + 32 * (wb + j) + c;
        if (!(j ? act1 : act0) || b_col >= N) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t a = acc_row(a_base, e, h);
            if (band_holds<true>(row0, row1, N, a, b_col)) {
                const int64_t ix = band_index(row0, a, b_col, true);
                R[(int64_t)WHICH * E + ix] = run[j][e];
                if (WHICH == 1) Q[ix] = qq[j][e];
            }
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(kPcrThreads, 1) void k_pcrelate(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows,
                                                             int64_t K, int64_t N, const float* __restrict__ betaG,
                                                             const float* __restrict__ X, int P1, float tau, const int2* __restrict__ tiles,
                                                             int64_t row0, int64_t row1, double* __restrict__ R, int* __restrict__ Q, int64_t E) {
    __shared__ __attribute__((aligned(16))) PcrSmem sm;
    const int2 tl = tiles[blockIdx.x];
    if (blockIdx.y == 0) pcr_tile<PACKED, 0>(sm, (const uint8_t*)Gv, ldr, krows, K, N, betaG, X, P1, tau, tl, row0, row1, R, Q, E);
    else pcr_tile<PACKED, 1>(sm, (const uint8_t*)Gv, ldr, krows, K, N, betaG, X, P1, tau, tl, row0, row1, R, Q, E);
}

int launch_pcrelate(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N, const float* betaG,
                    const float* X, int P, float tau, const int2* tiles, int64_t ntiles, int64_t row0, int64_t row1, double* R, int* Q, int64_t E) {
    if (ntiles <= 0) return 0;
    if (P < 0 || P > kPcrMaxPcs || ntiles >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)ntiles, 2u);
    if (packed) hipLaunchKernelGGL(k_pcrelate<true>, grid, dim3(kPcrThreads), 0, st, G, ldr, krows, K, N, betaG, X, P + 1, tau, tiles, row0, row1, R, Q, E);
    else hipLaunchKernelGGL(k_pcrelate<false>, grid, dim3(kPcrThreads), 0, st, G, ldr, krows, K, N, betaG, X, P + 1, tau, tiles, row0, row1, R, Q, E);
    return 0;
}

// ---- regression of the kept rows on the design ----------------------------------------------------------------------------------
// Workgroup = kPcrBetaRows kept rows (lane = row), 4 waves; wave w carries the JW coefficients j = w JW + q.  The samples go through
// LDS in stages of kPcrBetaStage ([row][sample] bytes, a row's tail past N zeroed), so that the hat matrix is read once per 64 rows
// (its JW doubles of one sample are the same for the whole wave).  Per row: sum of H g' and of H [missing] in f64 over the samples in
// their order, the mean of the observed training calls from exact integers, beta = (float)(sum H g' + mean * sum H [missing]).
constexpr int kPcrBetaStage = 256;
constexpr int kPcrBetaPitch = kPcrBetaStage + 4;
template <bool PACKED, int JW>
__global__ __launch_bounds__(64 * kPcrBetaWaves) void k_pcrelate_beta(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows,
                                                                      int64_t K, int64_t N, const uint8_t* __restrict__ train,
                                                                      const double* __restrict__ Hw, int P1, float* __restrict__ betaG,
                                                                      float* __restrict__ beta_rm, unsigned long long* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) uint8_t lg[kPcrBetaRows * kPcrBetaPitch];
    __shared__ __attribute__((aligned(16))) uint8_t lt[kPcrBetaStage];
    const uint8_t* G = (const uint8_t*)Gv;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t k0 = (int64_t)blockIdx.x * kPcrBetaRows;
    // staging map: thread t loads 64 samples (16 dwords) of row t / 4
    const int srow = threadIdx.x >> 2, sseg = threadIdx.x & 3;
    const int64_t skr = k0 + srow;
    const int64_t sorow = skr < K ? krows[skr] : -1;
    double ag[JW], am[JW];
#pragma unroll
    for (int t = 0; t < JW; ++t) { ag[t] = 0.0; am[t] = 0.0; }
    unsigned sum = 0u, cnt = 0u, bd = 0u;
    for (int64_t n0 = 0; n0 < N; n0 += kPcrBetaStage) {
        __syncthreads();                                   // the previous stage's readers are done with the LDS
#pragma unroll 4
        for (int d = 0; d < 16; ++d) {
            const int64_t ns = n0 + 64 * sseg + 4 * d;
            unsigned a = 0u;
            if (sorow >= 0 && ns < N) {
                if (PACKED) {
                    a = unpack4(G[sorow * ldr + (ns >> 2)]);
                } else a = *reinterpret_cast<const unsigned*>(G + sorow * ldr + ns);
                const int64_t left = N - ns;
                if (left < 4) a &= (1u << (8 * (int)left)) - 1u;
                // valid bytes: 0, 1, 2 and 0x81
                const unsigned m = (a >> 7) & 0x01010101u, g = a & ~(m * 0xffu);
                if ((a & (m * 0xffu)) != m * 0x81u || (g & 0xfcfcfcfcu) != 0u || (g & (g >> 1) & 0x01010101u) != 0u) bd = 1u;
            }
            *reinterpret_cast<unsigned*>(lg + srow * kPcrBetaPitch + 64 * sseg + 4 * d) = a;
        }
        { const int64_t nt = n0 + threadIdx.x; lt[threadIdx.x] = nt < N ? train[nt] : (uint8_t)0; }
        __syncthreads();
        const int nn1 = (int)(N - n0 < kPcrBetaStage ? N - n0 : kPcrBetaStage);
        for (int nn = 0; nn < nn1; nn += 4) {
            const unsigned a = *reinterpret_cast<const unsigned*>(lg + lane * kPcrBetaPitch + nn);
            const unsigned tr4 = *reinterpret_cast<const unsigned*>(lt + nn);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (nn + b >= nn1) break;
                const unsigned call = (a >> (8 * b)) & 0xffu;
                const bool miss = call == (unsigned)kPcrMissing;
                const double gd = miss ? 0.0 : (double)(int)call;
                const double* hp = Hw + ((int64_t)wv * N + (n0 + nn + b)) * JW;
#pragma unroll
                for (int t = 0; t < JW; ++t) ag[t] = fma(hp[t], gd, ag[t]);
                if (__builtin_amdgcn_ballot_w64(miss) != 0ull) {
                    const double md = miss ? 1.0 : 0.0;
#pragma unroll
                    for (int t = 0; t < JW; ++t) am[t] = fma(hp[t], md, am[t]);
                }
                if (((tr4 >> (8 * b)) & 0xffu) != 0u && !miss) { sum += call; ++cnt; }
            }
        }
    }
    if (bd && sorow >= 0) atomicMin(bad, (unsigned long long)sorow);
    const int64_t kr = k0 + lane;                          // (kr < pcr_kpad(K): the grouped layout has the row)
    const double mean = cnt ? (double)sum / (double)cnt : 0.0;
#pragma unroll
    for (int t = 0; t < JW; ++t) {
        const int j = wv * JW + t;
        if (j >= P1) continue;
        const float bv = (kr < K && cnt) ? (float)fma(mean, am[t], ag[t]) : 0.0f;
        betaG[((kr >> 3) * P1 + j) * 8 + (kr & 7)] = bv;
        if (beta_rm && kr < K) beta_rm[kr * P1 + j] = bv;
    }
}

template <bool PACKED>
static void launch_beta_jw(int jw, dim3 grid, hipStream_t st, const void* G, int64_t ldr, const int64_t* krows, int64_t K, int64_t N,
                           const uint8_t* train, const double* Hw, int P1, float* betaG, float* beta_rm, unsigned long long* bad) {
    const dim3 blk(64 * kPcrBetaWaves);
#define GPCA_PCR_BETA(JW) case JW: hipLaunchKernelGGL((k_pcrelate_beta<PACKED, JW>), grid, blk, 0, st, G, ldr, krows, K, N, train, Hw, P1, betaG, beta_rm, bad); break;
    switch (jw) { GPCA_PCR_BETA(1) GPCA_PCR_BETA(2) GPCA_PCR_BETA(3) GPCA_PCR_BETA(4) GPCA_PCR_BETA(6) GPCA_PCR_BETA(9) default: break; }
#undef GPCA_PCR_BETA
}
void launch_pcrelate_beta(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N,
                          const uint8_t* train, const double* Hw, int P, float* betaG, float* beta_rm, unsigned long long* bad) {
    if (K <= 0) return;
    const dim3 grid((unsigned)(pcr_kpad(K) / kPcrBetaRows));
    if (packed) launch_beta_jw<true>(pcr_beta_width(P), grid, st, G, ldr, krows, K, N, train, Hw, P + 1, betaG, beta_rm, bad);
    else launch_beta_jw<false>(pcr_beta_width(P), grid, st, G, ldr, krows, K, N, train, Hw, P + 1, betaG, beta_rm, bad);
}

// mu [(row1 - row0)][N]: one thread per sample, blockIdx.y = the group of 8 kept rows (from row0 rounded down to a group)
__global__ __launch_bounds__(256) void k_pcrelate_isaf(const float* __restrict__ betaG, const float* __restrict__ X, int P1, int64_t N,
                                                       int64_t row0, int64_t row1, float* __restrict__ mu_out) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int64_t g8 = (row0 >> 3) + blockIdx.y;
    float x[kPcrP1Max], mu[8];
    pcr_load_x(x, X, n, P1);
    pcr_isaf8(betaG + g8 * (int64_t)(8 * P1), x, P1, mu);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int64_t kr = 8 * g8 + r;
        if (kr >= row0 && kr < row1) mu_out[(kr - row0) * N + n] = mu[r];
    }
}
void launch_pcrelate_isaf(hipStream_t st, const float* betaG, const float* X, int P, int64_t N, int64_t row0, int64_t row1, float* mu) {
    if (row1 <= row0) return;
    const int64_t ng = ((row1 + 7) >> 3) - (row0 >> 3);
    for (int64_t g0 = 0; g0 < ng; g0 += 32768) {           // (grid.y holds 65 535)
        const int64_t gn = ng - g0 < 32768 ? ng - g0 : 32768;
        const int64_t r0 = g0 == 0 ? row0 : ((row0 >> 3) + g0) * 8, r1 = std::min(row1, ((row0 >> 3) + g0 + gn) * 8);
        hipLaunchKernelGGL(k_pcrelate_isaf, dim3((unsigned)((N + 255) / 256), (unsigned)gn), dim3(256), 0, st, betaG, X, P + 1, N, r0, r1,
                           mu + (r0 - row0) * N);
    }
}

// inv[n] += invalid entries of sample n over the kept rows of the workgroup's chunk (u32 atomics: exact in any order)
constexpr int kPcrInvRows = 1024;
template <bool PACKED>
__global__ __launch_bounds__(256) void k_pcrelate_inv(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t K,
                                                      int64_t N, const float* __restrict__ betaG, const float* __restrict__ X, int P1, float tau,
                                                      unsigned* __restrict__ inv) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const uint8_t* G = (const uint8_t*)Gv;
    const float one_m_tau = 1.0f - tau;
    const int64_t i0 = (int64_t)blockIdx.y * kPcrInvRows, i1 = i0 + kPcrInvRows < K ? i0 + kPcrInvRows : K;
    float x[kPcrP1Max], mu[8];
    pcr_load_x(x, X, n, P1);
    unsigned ni = 0u;
    for (int64_t kr0 = i0; kr0 < i1; kr0 += 8) {
        PcrFetch F;
        pcr_fetch<PACKED>(F, G, ldr, krows, i1, kr0, n, true);
        pcr_isaf8(betaG + (kr0 >> 3) * (int64_t)(8 * P1), x, P1, mu);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned call = ((r < 4 ? F.lo : F.hi) >> (8 * (r & 3))) & 0xffu;
            if (kr0 + r < i1 && !pcr_valid(call, mu[r], tau, one_m_tau)) ++ni;
        }
    }
    if (ni) atomicAdd(inv + n, ni);
}
void launch_pcrelate_inv(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N,
                         const float* betaG, const float* X, int P, float tau, unsigned* inv) {
    if (K <= 0) return;
    const int64_t nch = (K + kPcrInvRows - 1) / kPcrInvRows;
    for (int64_t c0 = 0; c0 < nch; c0 += 32768) {           // (grid.y holds 65 535)
        const int64_t cn = nch - c0 < 32768 ? nch - c0 : 32768;
        const int64_t kr0 = c0 * kPcrInvRows, K1 = std::min(K, (c0 + cn) * kPcrInvRows);
        const dim3 grid((unsigned)((N + 255) / 256), (unsigned)cn);
        // (the chunk's rows are addressed from its first row: krows and betaG advance with it; kr0 is a multiple of 8)
        if (packed) hipLaunchKernelGGL(k_pcrelate_inv<true>, grid, dim3(256), 0, st, G, ldr, krows + kr0, K1 - kr0, N, betaG + kr0 * (int64_t)(P + 1), X, P + 1, tau, inv);
        else hipLaunchKernelGGL(k_pcrelate_inv<false>, grid, dim3(256), 0, st, G, ldr, krows + kr0, K1 - kr0, N, betaG + kr0 * (int64_t)(P + 1), X, P + 1, tau, inv);
    }
}

// kinship and pair counts of the band's rows (one workgroup per band row), in f64: kin = num / (4 den), NaN when nsnp = 0
__global__ __launch_bounds__(256) void k_pcrelate_finish(const double* __restrict__ R, const int* __restrict__ Q, const unsigned* __restrict__ inv,
                                                         int64_t K, int64_t E, int64_t row0, double* __restrict__ kin, int* __restrict__ nsnp) {
    const int64_t a = row0 + blockIdx.x;
    const int64_t o = band_index(row0, a, 0, true);
    for (int64_t b = threadIdx.x; b <= a; b += 256) {
        const int64_t ix = o + b;
        const int64_t ns = ((K - (int64_t)inv[a]) - (int64_t)inv[b]) + (int64_t)Q[ix];      // (a = b: Q = inv_a, so K - inv_a)
        kin[ix] = ns == 0 ? __builtin_nan("") : R[ix] / (4.0 * R[E + ix]);
        if (nsnp) nsnp[ix] = (int)ns;
    }
}
void launch_pcrelate_finish(hipStream_t st, const double* R, const int* Q, const unsigned* inv, int64_t K, int64_t E, int64_t row0,
                            int64_t row1, double* kin, int* nsnp) {
    if (row1 <= row0) return;
    hipLaunchKernelGGL(k_pcrelate_finish, dim3((unsigned)(row1 - row0)), dim3(256), 0, st, R, Q, inv, K, E, row0, kin, nsnp);
}

}  // namespace gpca
