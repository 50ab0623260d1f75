// Runs of homozygosity (gpca_roh; gpca_roh.cpp; include/gpca.h section a20): per sample, the maximal stretches of kept rows that a
// sliding window of W rows calls homozygous, as records (sample, first, last, n_het, n_missing).
//
// The access pattern is the sample counts' (sample_counts.hip): a thread owns kScLane = 16 consecutive samples (one uint4 of an int8
// row, one dword of a 2-bit row), a workgroup of one wave owns a chunk of 1 024 samples and one row split of the launch plan
// (roh_plan in plan_math.h), and walks kept rows through krows.  Everything is integer arithmetic; no float and no atomic touches an
// output (the one atomicMin is the invalid-genotype word, as everywhere).  Rows below are band-relative.
//
// k_roh_mark decides the rows of its split.  Per window domain [d0, d1) that the split meets, and with [pa, pb) the split's rows in
// it: it walks rows t = roh_win_lo .. roh_win_hi + W - 1 (its rows and a halo of at most W - 1 rows on either side, clipped at the
// domain) with running het and missing counts of the last W rows per sample, byte-wise, four samples to a dword: the entering row is
// added, the row W behind is fetched a second time and subtracted.  A count is at most W <= 64, so the byte compare "count <= H" is
// bit 7 of (0x80 + H) - count, with no borrow between bytes.  Once W rows are in, window s = t - W + 1 is complete: its 16 hit bits go
// to the thread's column of a ring of 64 windows in LDS (8 KiB; a thread reads only what it wrote, so there is no barrier) and are
// added to a third set of byte counters, the hits among the last W windows; the bits of window s - W come back from the ring and are
// taken off.  Windows before roh_win_lo are never counted: they cover no row of the piece.  Row j's covering windows end at
// min(j, d1 - W), so row s is decided when window s completes: in-ROH iff hits >= ceil(num cov / den), which is hits den >= num cov,
// again a byte compare.  Behind the domain's last window the rows j = d1 - W + 1 .. lose window j - W each and gain none.  The 16
// decisions are two bytes of the bit plane inroh [rows][npad / 8].  A domain shorter than W has no window: its rows are written 0
// (int8 rows are still read once, for the check of their values).
//
// k_roh_runs (compiled as count and as fill) walks the plane over the rows of its split only, four rows' plane bytes and genotypes in
// flight; the genotypes are fetched only where a wave ballot finds an open run or an in-ROH bit among the wave's samples.  A run
// starts at a row that is in-ROH where the previous row is not, or that has bit 1 of brk set (band row 0 always).  Het and missing
// calls on open runs are added byte-wise and flushed to u32 registers every 255 fetched rows.  A run that starts and ends inside the
// split is the split's own: counted (count pass) or written (fill pass).  What crosses a split boundary is left in the split's entry
// of rec [splits][npad][8] (count pass): the head = the continuation of a run from the split before (its rows, het and missing calls
// in this split, and whether it goes on into the next split), and the tail = a run that starts here and goes on into the next split
// (first row, het, missing).  Whether a run goes on is read from the plane's next row, so both sides of a boundary agree.
// k_roh_stitch (a thread per sample, splits ascending) joins tail, heads and the closing head into one run and credits it to the split
// it starts in, where it is the last record (count pass: cnt [split][sample] = the split's own runs + that one; then the exclusive
// scan over the splits and seg_count; fill pass: the joined run is written at base[n] + cnt[split][n] + the split's own runs).  The
// host scans seg_count into base [N].  Order and values depend on nothing but the band.
// Registers: the figures hipcc reports are in DESIGN section 7.
#include "syrk_tile.h"

namespace gpca {

template <bool PACKED> struct RohFetch;
template <> struct RohFetch<false> { uint4 v; };
template <> struct RohFetch<true> { unsigned v; };

// (base = the row-0 address of the thread's fetch, sc_row_offset: 16-byte (4-byte) aligned and inside the row's pitch)
__device__ __forceinline__ void roh_fetch(RohFetch<false>& F, const uint8_t* __restrict__ base, int64_t ldr, int64_t orow) {
    F.v = *reinterpret_cast<const uint4*>(base + orow * ldr);
}
__device__ __forceinline__ void roh_fetch(RohFetch<true>& F, const uint8_t* __restrict__ base, int64_t ldr, int64_t orow) {
    F.v = *reinterpret_cast<const unsigned*>(base + orow * ldr);
}
__device__ __forceinline__ unsigned roh_dword(const RohFetch<false>& F, int d) { return d == 0 ? F.v.x : d == 1 ? F.v.y : d == 2 ? F.v.z : F.v.w; }
__device__ __forceinline__ unsigned roh_dword(const RohFetch<true>& F, int d) { return unpack4((F.v >> (8 * d)) & 0xffu); }

// the missing (m) and het (h) indicator bytes of the thread's 16 samples on one row; vb = the byte masks of the samples below N;
// returns nonzero iff a sample below N holds a value outside {0, 1, 2, missing} (int8 rows only: 2-bit storage decodes to nothing else)
template <bool PACKED>
__device__ __forceinline__ unsigned roh_decode(const RohFetch<PACKED>& F, const unsigned (&vb)[4], unsigned (&m)[4], unsigned (&h)[4]) {
    unsigned bd = 0u;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned a = roh_dword(F, d) & vb[d];
        const unsigned mm = (a >> 7) & 0x01010101u;
        if (!PACKED) bd |= (a & 0x7c7c7c7cu) | ((((a >> 1) & a) | (mm & ((a >> 1) | ~a))) & 0x01010101u);
        m[d] = mm;
        h[d] = a & ~mm & 0x01010101u;                                              // (the missing code has bit 0 set)
    }
    return bd;
}
// bit 0 of each of a dword's four bytes as bits 0 .. 3 (the inverse of kept_bytes)
__device__ __forceinline__ unsigned roh_pack4(unsigned x) { return ((x * 0x01020408u) >> 24) & 0xfu; }
// the byte i of a dword quartet
__device__ __forceinline__ unsigned roh_byte(const unsigned (&w)[4], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// the decision of one row from the hit counters hw (bytes): in-ROH iff hits >= need, need = ceil(num cov / den) <= cov <= 64
__device__ __forceinline__ void roh_decide(uint8_t* __restrict__ pl, int64_t j, int64_t pitch, const unsigned (&hw)[4], unsigned cov, unsigned num,
                                           unsigned den, unsigned inb) {
    const unsigned need = (num * cov + den - 1u) / den;                              // (num cov <= 2^20 x 64)
    const unsigned add = (0x80u - need) * 0x01010101u;
    unsigned bits = 0u;
#pragma unroll
    for (int d = 0; d < 4; ++d) bits |= roh_pack4(((hw[d] + add) >> 7) & 0x01010101u) << (4 * d);   // byte: hits + 0x80 - need in 0x40 .. 0xc0, no carry
    *reinterpret_cast<unsigned short*>(pl + j * pitch) = (unsigned short)(bits & inb);
}

// plane [rows][pitch] of band rows [0, rows) in splits of `per` rows; dom [nd + 1] = the domains' first rows, then rows
template <bool PACKED>
__global__ __launch_bounds__(kScThreads) void k_roh_mark(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                         int64_t npad, int64_t chunks, int64_t row0, int64_t rows, int64_t per,
                                                         const int* __restrict__ dom, int nd, int W, unsigned H, unsigned M, unsigned num,
                                                         unsigned den, uint8_t* __restrict__ plane, int64_t pitch,
                                                         unsigned long long* __restrict__ bad) {
    __shared__ unsigned short ring[kRohMaxWindow][kScThreads];                       // the hit bits of the last 64 windows, per thread
    const int64_t chunk = (int64_t)blockIdx.x % chunks, split = (int64_t)blockIdx.x / chunks;
    const int64_t n0 = sc_thread_sample(chunk, threadIdx.x);
    if (n0 >= npad) return;
    const int64_t ka = split * per, kb = ka + per < rows ? ka + per : rows;
    const int64_t left = N - n0;
    const unsigned inb = left >= kScLane ? 0xffffu : (1u << (int)left) - 1u;       // (n0 < npad: left >= 1)
    unsigned vb[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) vb[d] = kept_bytes(inb, d) * 0xffu;
    const uint8_t* base = (const uint8_t*)Gv + sc_row_offset(PACKED, n0);
    uint8_t* pl = plane + roh_plane_index(0, pitch, n0);
    const unsigned hc = (0x80u | H) * 0x01010101u, mc = (0x80u | M) * 0x01010101u;
    const int tid = (int)threadIdx.x;

    // the domain that holds row ka: the last one that starts at or before it (dom[0] = 0)
    int lo = 0, hi = nd;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)dom[mid] <= ka) lo = mid; else hi = mid;
    }
    int di = lo;
    for (int64_t pa = ka; pa < kb; ++di) {
        const int64_t d0 = dom[di], d1 = dom[di + 1];
        const int64_t pb = kb < d1 ? kb : d1;
        if (d1 - d0 < W) {                                                          // no window: no row is in
            for (int64_t j = pa; j < pb; ++j) {
                if (!PACKED) {
                    RohFetch<PACKED> F;
                    unsigned m[4], h[4];
                    const int64_t orow = krows[row0 + j];
                    roh_fetch(F, base, ldr, orow);
                    if (roh_decode<PACKED>(F, vb, m, h)) atomicMin(bad, (unsigned long long)orow);
                }
                *reinterpret_cast<unsigned short*>(pl + j * pitch) = (unsigned short)0;
            }
            pa = pb;
            continue;
        }
        const int64_t s_lo = roh_win_lo(d0, pa, W), s_hi = roh_win_hi(d1, pb, W), t_hi = s_hi + W - 1, s_end = d1 - W;
        unsigned cm[4], ch[4], hw[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) { cm[d] = 0u; ch[d] = 0u; hw[d] = 0u; }
        for (int64_t t = s_lo; t <= t_hi; t += kRohUnroll) {
            RohFetch<PACKED> E[kRohUnroll], L[kRohUnroll];
            int64_t orow[kRohUnroll];
#pragma unroll
            for (int u = 0; u < kRohUnroll; ++u) {                                   // (wave-uniform conditions)
                const int64_t tt = t + u;
                E[u] = RohFetch<PACKED>{}; L[u] = RohFetch<PACKED>{}; orow[u] = 0;
                if (tt <= t_hi) {
                    orow[u] = krows[row0 + tt];
                    roh_fetch(E[u], base, ldr, orow[u]);
                    if (tt - s_lo >= W) roh_fetch(L[u], base, ldr, krows[row0 + tt - W]);
                }
            }
#pragma unroll
            for (int u = 0; u < kRohUnroll; ++u) {
                const int64_t tt = t + u;
                if (tt > t_hi) break;
                unsigned m[4], h[4];
                if (roh_decode<PACKED>(E[u], vb, m, h)) atomicMin(bad, (unsigned long long)orow[u]);
#pragma unroll
                for (int d = 0; d < 4; ++d) { cm[d] += m[d]; ch[d] += h[d]; }
                if (tt - s_lo >= W) {                                               // the row that leaves the window
                    roh_decode<PACKED>(L[u], vb, m, h);
#pragma unroll
                    for (int d = 0; d < 4; ++d) { cm[d] -= m[d]; ch[d] -= h[d]; }
                }
                if (tt - s_lo < W - 1) continue;
                const int64_t s = tt - W + 1;                                       // window s is complete
                if (s - W >= s_lo) {                                                // window s - W leaves (read before its slot is reused)
                    const unsigned lv = ring[(s - W) & (kRohMaxWindow - 1)][tid];
#pragma unroll
                    for (int d = 0; d < 4; ++d) hw[d] -= kept_bytes(lv, d);
                }
                unsigned hit16 = 0u;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned hb = (((hc - ch[d]) & (mc - cm[d])) >> 7) & 0x01010101u;   // bit 7 of a byte: het <= H and missing <= M
                    hw[d] += hb;
                    hit16 |= roh_pack4(hb) << (4 * d);
                }
                ring[s & (kRohMaxWindow - 1)][tid] = (unsigned short)hit16;
                // row s: its covering windows are roh_cov_lo .. s, all at or after s_lo and inside the last W
                if (s >= pa) roh_decide(pl, s, pitch, hw, (unsigned)(s - roh_cov_lo(d0, s, W) + 1), num, den, inb);
            }
        }
        if (s_hi == s_end)                                                          // behind the domain's last window: no window enters
            for (int64_t j = s_end + 1; j < pb; ++j) {
                if (j - W >= s_lo) {
                    const unsigned lv = ring[(j - W) & (kRohMaxWindow - 1)][tid];
#pragma unroll
                    for (int d = 0; d < 4; ++d) hw[d] -= kept_bytes(lv, d);
                }
                if (j >= pa) roh_decide(pl, j, pitch, hw, (unsigned)(s_end - roh_cov_lo(d0, j, W) + 1), num, den, inb);
            }
        pa = pb;
    }
}

// COUNT: rec [splits][npad][8] = what the split knows of every sample (kRohRec*).  FILL: the split's own runs, the i-th of sample n at
// record base[n] + cnt[split][n] + i of segs [cap][5] (records at or beyond cap are dropped).  brk [rows]: bit 1 = no run continues into
// the row (band row 0 always)
template <bool PACKED, bool FILL>
__global__ __launch_bounds__(kScThreads) void k_roh_runs(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                         int64_t npad, int64_t chunks, int64_t row0, int64_t rows, int64_t per,
                                                         const uint8_t* __restrict__ brk, const uint8_t* __restrict__ plane, int64_t pitch,
                                                         int64_t min_snp, int64_t max_het, unsigned* __restrict__ rec,
                                                         const unsigned* __restrict__ cnt, const unsigned long long* __restrict__ segbase,
                                                         unsigned* __restrict__ segs, int64_t cap) {
    const int64_t chunk = (int64_t)blockIdx.x % chunks, split = (int64_t)blockIdx.x / chunks;
    const int64_t n0 = sc_thread_sample(chunk, threadIdx.x);
    if (n0 >= npad) return;
    const int64_t ka = split * per, kb = ka + per < rows ? ka + per : rows;
    const int64_t left = N - n0;
    const unsigned inb = left >= kScLane ? 0xffffu : (1u << (int)left) - 1u;
    unsigned vb[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) vb[d] = kept_bytes(inb, d) * 0xffu;
    const uint8_t* base = (const uint8_t*)Gv + sc_row_offset(PACKED, n0);
    const uint8_t* pl = plane + roh_plane_index(0, pitch, n0);

    unsigned first[kScLane], ah[kScLane], am[kScLane], found[kScLane], hl[kScLane], hh[kScLane], hm[kScLane];
    unsigned long long off[kScLane];
#pragma unroll
    for (int i = 0; i < kScLane; ++i) {
        first[i] = 0u; ah[i] = 0u; am[i] = 0u; found[i] = 0u; hl[i] = 0u; hh[i] = 0u; hm[i] = 0u;
        off[i] = FILL && ((inb >> i) & 1u) ? segbase[n0 + i] + (unsigned long long)cnt[roh_cnt_index(split, npad, n0 + i)] : 0ull;
    }
    unsigned swh[4], swm[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) { swh[d] = 0u; swm[d] = 0u; }
    int fetched = 0;
    unsigned open = 0u, ishead = 0u;
    unsigned prev = ka > 0 ? (unsigned)*reinterpret_cast<const unsigned short*>(pl + (ka - 1) * pitch) & inb : 0u;

    // the runs of the samples in `ends` stop before row jj: a head is kept for the stitch, the split's own run is counted or written
    auto close = [&](unsigned ends, int64_t jj) {
#pragma unroll
        for (int i = 0; i < kScLane; ++i)
            if ((ends >> i) & 1u) {
                const unsigned nh = ah[i] + roh_byte(swh, i), nm = am[i] + roh_byte(swm, i);
                if ((ishead >> i) & 1u) {                                         // (the fill pass leaves the heads to the stitch)
                    if (!FILL) { hl[i] = (unsigned)(jj - ka); hh[i] = nh; hm[i] = nm; }
                } else if (jj - (int64_t)first[i] >= min_snp && (max_het < 0 || (int64_t)nh <= max_het)) {
                    if (FILL) {
                        const unsigned long long ix = off[i]++;
                        if (ix < (unsigned long long)cap) {
                            unsigned* r = segs + 5ull * ix;
                            r[0] = (unsigned)(n0 + i); r[1] = (unsigned)(row0 + first[i]); r[2] = (unsigned)(row0 + jj - 1); r[3] = nh; r[4] = nm;
                        }
                    } else {
                        found[i]++;
                    }
                }
                ah[i] = 0u; am[i] = 0u;
            }
#pragma unroll
        for (int d = 0; d < 4; ++d) { const unsigned keepb = ~(kept_bytes(ends, d) * 0xffu); swh[d] &= keepb; swm[d] &= keepb; }
        open &= ~ends;
        ishead &= ~ends;
    };

    for (int64_t j = ka; j < kb; j += kRohUnroll) {
        unsigned cur[kRohUnroll], anyc = 0u;
        bool cut[kRohUnroll];
#pragma unroll
        for (int u = 0; u < kRohUnroll; ++u) {                                       // (wave-uniform conditions)
            const int64_t jj = j + u;
            cur[u] = 0u; cut[u] = true;
            if (jj < kb) {
                cur[u] = (unsigned)*reinterpret_cast<const unsigned short*>(pl + jj * pitch) & inb;
                cut[u] = jj == 0 || (brk[jj] & 2u) != 0u;
            }
            anyc |= cur[u];
        }
        // the genotypes of the group: wanted iff a sample of the wave is in a run on one of its rows
        const bool want = __builtin_amdgcn_ballot_w64((open | anyc) != 0u) != 0ull;
        RohFetch<PACKED> F[kRohUnroll];
#pragma unroll
        for (int u = 0; u < kRohUnroll; ++u) {
            F[u] = RohFetch<PACKED>{};
            if (want && j + u < kb) roh_fetch(F[u], base, ldr, krows[row0 + j + u]);
        }
#pragma unroll
        for (int u = 0; u < kRohUnroll; ++u) {
            const int64_t jj = j + u;
            if (jj >= kb) break;
            const unsigned ends = open & (cut[u] ? 0xffffu : ~cur[u]);
            if (ends) close(ends, jj);
            const unsigned news = cur[u] & ~open;                                   // (what stays open holds cur set)
            if (news) {
#pragma unroll
                for (int i = 0; i < kScLane; ++i)
                    if ((news >> i) & 1u) first[i] = (unsigned)jj;
                if (jj == ka && !cut[u]) ishead |= news & prev;                      // the continuation of a run of the split before
                open |= news;
            }
            if (want) {
                unsigned m[4], h[4];
                roh_decode<PACKED>(F[u], vb, m, h);
#pragma unroll
                for (int d = 0; d < 4; ++d) { const unsigned ob = kept_bytes(open, d) * 0xffu; swh[d] += h[d] & ob; swm[d] += m[d] & ob; }
                if (++fetched == kRohFlushRows) {                                   // before a byte can wrap
#pragma unroll
                    for (int i = 0; i < kScLane; ++i) { ah[i] += roh_byte(swh, i); am[i] += roh_byte(swm, i); }
#pragma unroll
                    for (int d = 0; d < 4; ++d) { swh[d] = 0u; swm[d] = 0u; }
                    fetched = 0;
                }
            }
            prev = cur[u];
        }
    }
    // the split's end: a run goes on iff the next row is in-ROH and not cut (the next split reads the same two facts as its head)
    unsigned cont = 0u;
    if (kb < rows && (brk[kb] & 2u) == 0u) cont = (unsigned)*reinterpret_cast<const unsigned short*>(pl + kb * pitch) & inb;
    if (open & ~cont) close(open & ~cont, kb);
    if (!FILL) {
        // what is still open goes on: a head that spans the split (through), or a tail; rec = 8 u32 per sample, two uint4
        uint4* ro = reinterpret_cast<uint4*>(rec + roh_rec_index(split, npad, n0));
#pragma unroll
        for (int i = 0; i < kScLane; ++i) {
            const bool on = (open >> i) & 1u, head = (ishead >> i) & 1u;
            const unsigned nh = ah[i] + roh_byte(swh, i), nm = am[i] + roh_byte(swm, i);
            const bool through = on && head, tail = on && !head;
            ro[2 * i] = make_uint4(through ? (unsigned)(kb - ka) : hl[i], through ? nh : hh[i], through ? nm : hm[i],
                                   (through ? kRohFlagThrough : 0u) | (tail ? kRohFlagTail : 0u));
            ro[2 * i + 1] = make_uint4(tail ? first[i] : 0u, tail ? nh : 0u, tail ? nm : 0u, found[i]);
        }
    }
}

// a thread per sample, splits ascending: joins what crosses the split boundaries.  COUNT: cnt [s][n] = the split's own runs + the run
// that starts in it and ends in a later split, then its exclusive sum over the splits; seg_count [n] = the total.  FILL: writes the
// joined runs, each behind its first split's own runs
template <bool FILL>
__global__ __launch_bounds__(kRohStitchThreads) void k_roh_stitch(const unsigned* __restrict__ rec, unsigned* __restrict__ cnt, int64_t N, int64_t npad,
                                                                int64_t splits, int64_t per, int64_t row0, int64_t min_snp, int64_t max_het,
                                                                unsigned* __restrict__ seg_count, const unsigned long long* __restrict__ segbase,
                                                                unsigned* __restrict__ segs, int64_t cap) {
    const int64_t n = (int64_t)blockIdx.x * kRohStitchThreads + threadIdx.x;
    if (n >= N) return;
    bool open = false;
    unsigned cfirst = 0u, chet = 0u, cmis = 0u, cown = 0u;
    int64_t cs = 0;
    // (kRohStitchBatch entries' loads in flight: their addresses do not depend on what is joined)
    for (int64_t s0 = 0; s0 < splits; s0 += kRohStitchBatch) {
        uint4 av[kRohStitchBatch], bv[kRohStitchBatch];
#pragma unroll
        for (int u = 0; u < kRohStitchBatch; ++u) {
            av[u] = make_uint4(0u, 0u, 0u, 0u); bv[u] = make_uint4(0u, 0u, 0u, 0u);
            if (s0 + u < splits) {
                const uint4* r = reinterpret_cast<const uint4*>(rec + roh_rec_index(s0 + u, npad, n));
                av[u] = r[0]; bv[u] = r[1];
            }
        }
#pragma unroll
        for (int u = 0; u < kRohStitchBatch; ++u) {
            const int64_t s = s0 + u;
            if (s >= splits) break;
            const uint4 a = av[u], b = bv[u];
            if (!FILL) cnt[roh_cnt_index(s, npad, n)] = b.w;
            if (open) {                                                             // (a.x >= 1: the head the tail before it saw in the plane)
                chet += a.y; cmis += a.z;
                if (!(a.w & kRohFlagThrough)) {
                    const int64_t last = s * per + (int64_t)a.x - 1;
                    if (last - (int64_t)cfirst + 1 >= min_snp && (max_het < 0 || (int64_t)chet <= max_het)) {
                        if (FILL) {
                            const unsigned long long ix = segbase[n] + (unsigned long long)cnt[roh_cnt_index(cs, npad, n)] + cown;
                            if (ix < (unsigned long long)cap) {
                                unsigned* o = segs + 5ull * ix;
                                o[0] = (unsigned)n; o[1] = (unsigned)(row0 + cfirst); o[2] = (unsigned)(row0 + last); o[3] = chet; o[4] = cmis;
                            }
                        } else {
                            cnt[roh_cnt_index(cs, npad, n)] += 1u;                  // (cs < s: written above, by this thread)
                        }
                    }
                    open = false;
                }
            }
            if (a.w & kRohFlagTail) { open = true; cfirst = b.x; chet = b.y; cmis = b.z; cown = b.w; cs = s; }
        }
    }
    if (!FILL) {
        unsigned run = 0u;
        for (int64_t s0 = 0; s0 < splits; s0 += kRohStitchBatch) {
            unsigned c[kRohStitchBatch];
#pragma unroll
            for (int u = 0; u < kRohStitchBatch; ++u) c[u] = s0 + u < splits ? cnt[roh_cnt_index(s0 + u, npad, n)] : 0u;
#pragma unroll
            for (int u = 0; u < kRohStitchBatch; ++u) {
                if (s0 + u >= splits) break;
                cnt[roh_cnt_index(s0 + u, npad, n)] = run;
                run += c[u];
            }
        }
        seg_count[n] = run;
    }
}

static bool roh_plan_ok(int64_t N, int64_t rows, const RohPlan& plan) {
    return N >= 1 && rows >= 1 && rows < ((int64_t)1 << 31) && plan.chunks == sc_chunks(N) && plan.per >= 1 && plan.splits >= 1 &&
           (plan.splits - 1) * plan.per < rows && plan.splits * plan.per >= rows && sc_grid(plan) < ((int64_t)1 << 31);
}

int launch_roh_mark(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, int64_t row0, int64_t row1,
                    const RohPlan& plan, const int* dom, int64_t domains, int W, int H, int M, int num, int den, uint8_t* plane,
                    unsigned long long* bad) {
    const int64_t rows = row1 - row0;
    if (!roh_plan_ok(N, rows, plan) || domains < 1 || domains > rows || W < 1 || W > kRohMaxWindow || H < 0 || H > W || M < 0 || M > W ||
        num < 0 || num > den || den < 1 || den > kRohMaxDen)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)sc_grid(plan)), blk(kScThreads);
    const int64_t npad = roh_npad(N), pitch = roh_plane_pitch(N);
#define GPCA_ROH(PK) hipLaunchKernelGGL((k_roh_mark<PK>), grid, blk, 0, st, G, ldr, krows, N, npad, plan.chunks, row0, rows, plan.per, dom, (int)domains, W, (unsigned)H, (unsigned)M, (unsigned)num, (unsigned)den, plane, pitch, bad)
    if (packed) GPCA_ROH(true); else GPCA_ROH(false);
#undef GPCA_ROH
    return 0;
}

int launch_roh_runs(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, int64_t row0, int64_t row1,
                    const RohPlan& plan, const uint8_t* brk, const uint8_t* plane, int64_t min_snp, int64_t max_het, unsigned* rec,
                    unsigned* cnt, unsigned* seg_count, const unsigned long long* base, unsigned* segs, int64_t cap) {
    const int64_t rows = row1 - row0;
    const bool fill = segs != nullptr;
    if (!roh_plan_ok(N, rows, plan) || min_snp < 1 || (fill && (!base || cap < 1)) || (!fill && !seg_count)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)sc_grid(plan)), blk(kScThreads), sgrid((unsigned)((N + kRohStitchThreads - 1) / kRohStitchThreads)), sblk(kRohStitchThreads);
    const int64_t npad = roh_npad(N), pitch = roh_plane_pitch(N);
#define GPCA_ROH(PK, FL) hipLaunchKernelGGL((k_roh_runs<PK, FL>), grid, blk, 0, st, G, ldr, krows, N, npad, plan.chunks, row0, rows, plan.per, brk, plane, pitch, min_snp, max_het, rec, cnt, base, segs, cap)
    if (fill) { if (packed) GPCA_ROH(true, true); else GPCA_ROH(false, true); }
    else { if (packed) GPCA_ROH(true, false); else GPCA_ROH(false, false); }
#undef GPCA_ROH
#define GPCA_ROH(FL) hipLaunchKernelGGL((k_roh_stitch<FL>), sgrid, sblk, 0, st, rec, cnt, N, npad, plan.splits, plan.per, row0, min_snp, max_het, seg_count, base, segs, cap)
    if (fill) GPCA_ROH(true); else GPCA_ROH(false);
#undef GPCA_ROH
    return 0;
}

}  // namespace gpca
