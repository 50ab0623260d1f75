// gpca_f2_blocks / gpca_fstat_blocks / gpca_fstat (include/gpca.h section a23): the summed unbiased f2 of every jackknife block of rows
// and every pair of groups, and the two host rules that lay out the blocks and turn the sums into f2, f3 and f4 with their weighted
// block-jackknife standard errors.  The device call is gpca_group_counts' genotype pass as it is (k_gc_onehot, k_group_counts) and one
// reduction over the counts it leaves in the workspace (k_f2_blocks, f2_blocks.hip); the workspace lives for the call.
#include "gpca_internal.h"

#pragma clang fp contract(off)

using namespace gpca;

namespace {
struct FbWs {
    uint8_t* onehot = nullptr;
    int32_t *label = nullptr, *block = nullptr, *cnt = nullptr;
    unsigned *size = nullptr, *counts = nullptr;
    unsigned long long* bad = nullptr;
    long long* acc = nullptr;
    ~FbWs() { dfree(onehot); dfree(label); dfree(block); dfree(cnt); dfree(size); dfree(counts); dfree(bad); dfree(acc); }
};
}  // namespace

extern "C" int gpca_f2_blocks(gpca_handle* h, const int32_t* group, int32_t P, int64_t row0, int64_t row1, const int32_t* block, int32_t B,
                              int64_t* acc, int64_t* cnt, uint32_t* counts) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_f2_blocks");
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on) return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels, which is not implemented");
    if (multi_rank(h)) return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    const int64_t K = h->n_pca, N = h->N;
    if (!group) return fail(h, GPCA_ERR_BAD_ARG, f + ": group is required");
    if (!block) return fail(h, GPCA_ERR_BAD_ARG, f + ": block is required");
    if (!acc) return fail(h, GPCA_ERR_BAD_ARG, f + ": acc is required");
    if (!cnt) return fail(h, GPCA_ERR_BAD_ARG, f + ": cnt is required");
    if (P < 2 || P > kGcMaxGroups) return fail(h, GPCA_ERR_BAD_ARG, f + ": P must satisfy 2 <= P <= " + std::to_string(kGcMaxGroups));
    if (B < 1) return fail(h, GPCA_ERR_BAD_ARG, f + ": B must be at least 1");
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    const int64_t rows = row1 - row0;
    if (rows > kFbMaxRows) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band holds more than 2^21 rows (the sums are 64-bit): ask for fewer rows");
    if (N >= ((int64_t)1 << 30)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 2^30 or more samples (the counts are 32-bit)");
    std::vector<int32_t> label((size_t)gc_label_capacity(N));
    std::vector<unsigned> size((size_t)gc_size_capacity(), 0u);
    for (int64_t n = 0; n < N; ++n) {
        const int32_t g = group[n];
        if (g >= P) return fail(h, GPCA_ERR_BAD_ARG, f + ": group[" + std::to_string(n) + "] = " + std::to_string(g) + " is not below P = " + std::to_string(P));
        label[(size_t)n] = g < 0 ? -1 : g;
        if (g >= 0) size[(size_t)g]++;
    }
    for (int64_t r = 0; r < rows; ++r)
        if (block[r] < -1 || block[r] >= B)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": block[" + std::to_string(r) + "] = " + std::to_string(block[r]) + " (kept row " + std::to_string(row0 + r) +
                                                 ") is outside -1 .. B - 1 = " + std::to_string(B - 1));
    const int64_t nout = fb_out_capacity(B, P);
    std::fill(acc, acc + nout, (int64_t)0);
    std::fill(cnt, cnt + nout, (int64_t)0);
    if (rows == 0) return GPCA_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the band needs", fb_call_bytes(N, rows, P, B) + (double)(64 << 20)));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    FbWs ws;
    HIPCHK(dalloc(ws.onehot, (size_t)gc_onehot_capacity(N, P))); HIPCHK(dalloc(ws.label, (size_t)gc_label_capacity(N)));
    HIPCHK(dalloc(ws.size, (size_t)gc_size_capacity())); HIPCHK(dalloc(ws.counts, (size_t)gc_counts_capacity(rows, P))); HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(dalloc(ws.block, (size_t)fb_block_capacity(rows))); HIPCHK(dalloc(ws.acc, (size_t)nout)); HIPCHK(dalloc(ws.cnt, (size_t)nout));
    HIPCHK(hipMemcpyAsync(ws.label, label.data(), label.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.size, size.data(), size.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.block, block, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    HIPCHK(hipMemsetAsync(ws.acc, 0, (size_t)nout * 8, st));
    HIPCHK(hipMemsetAsync(ws.cnt, 0, (size_t)nout * 4, st));
    launch_gc_onehot(st, ws.label, N, P, ws.onehot);
    HIPCHK(hipGetLastError());
    {
        ScopedTimer t(h, "group_counts", 2.0 * 2.0 * (double)rows * (double)N * (double)gc_ppad(P), (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_group_counts(st, G, packed, ldr, h->d_pca_rows, N, ws.onehot, ws.size, P, row0, row1, ws.counts, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    {
        // ops: two divisions and three more per (row, group), six per (row, pair); bytes: the counts, read once
        ScopedTimer t(h, "f2_blocks", (double)rows * (5.0 * (double)P + 6.0 * (double)fb_pairs(P)), 4.0 * (double)gc_counts_capacity(rows, P));
        if (launch_f2_blocks(st, ws.counts, ws.block, rows, P, ws.acc, ws.cnt) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    std::vector<int32_t> c32((size_t)nout);
    HIPCHK(hipMemcpyAsync(acc, ws.acc, (size_t)nout * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c32.data(), ws.cnt, (size_t)nout * 4, hipMemcpyDeviceToHost, st));
    if (counts) HIPCHK(hipMemcpyAsync(counts, ws.counts, (size_t)gc_counts_capacity(rows, P) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < nout; ++i) cnt[i] = (int64_t)c32[(size_t)i];
    return GPCA_OK;
}

extern "C" int gpca_fstat_blocks(const uint8_t* chrom_change, const int64_t* pos, int64_t rows, int64_t size, int32_t unit, int32_t* block,
                                 int32_t* n_blocks) {
    if (rows < 0 || size < 1 || (unit != GPCA_FSTAT_BLOCK_VARIANTS && unit != GPCA_FSTAT_BLOCK_BP) || !n_blocks) return GPCA_ERR_BAD_ARG;
    if (rows > 0 && (!chrom_change || !block || (unit == GPCA_FSTAT_BLOCK_BP && !pos))) return GPCA_ERR_BAD_ARG;
    int64_t b = -1, held = 0, first = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const bool start = r == 0 || chrom_change[r] != 0 || (unit == GPCA_FSTAT_BLOCK_VARIANTS ? held >= size : pos[r] - first >= size);
        if (start) {
            if (b + 1 > (int64_t)INT32_MAX - 1) return GPCA_ERR_BAD_ARG;
            ++b; held = 0;
            if (unit == GPCA_FSTAT_BLOCK_BP) first = pos[r];
        }
        block[r] = (int32_t)b;
        ++held;
    }
    *n_blocks = (int32_t)(b + 1);
    return GPCA_OK;
}

extern "C" int gpca_fstat(const int64_t* acc, const int64_t* cnt, int32_t B, int32_t P, const int32_t* quads, int64_t M, double* out) {
    if (!acc || !cnt || !out || M < 0 || (M > 0 && !quads) || B < 1 || P < 2 || P > kGcMaxGroups) return GPCA_ERR_BAD_ARG;
    for (int64_t i = 0; i < 4 * M; ++i)
        if (quads[i] < 0 || quads[i] >= P) return GPCA_ERR_BAD_ARG;
    const int64_t pairs = fb_pairs(P);
    const double nan = std::nan(""), grid = 1.0 / kFbScale;
    std::vector<int32_t> used;
    std::vector<double> tminus, mb;
    for (int64_t s = 0; s < M; ++s) {
        double* o = out + 6 * s;
        const int32_t* qd = quads + 4 * s;
        // step 1: the four terms +f2(a,d) +f2(b,c) -f2(a,c) -f2(b,d), each times 1/2, combined over distinct pairs, pair index ascending
        const int32_t tx[4] = {qd[0], qd[1], qd[0], qd[1]}, ty[4] = {qd[3], qd[2], qd[2], qd[3]};
        const double ts[4] = {0.5, 0.5, -0.5, -0.5};
        int64_t pq[4];
        double pc[4];
        int np = 0;
        for (int k = 0; k < 4; ++k) {
            if (tx[k] == ty[k]) continue;
            const int i = std::max(tx[k], ty[k]), j = std::min(tx[k], ty[k]);
            const int64_t q = fb_pair_index(i, j);
            int at = 0;
            while (at < np && pq[at] != q) ++at;
            if (at == np) { pq[np] = q; pc[np] = 0.0; ++np; }
            pc[at] += ts[k];
        }
        int nq = 0;
        for (int k = 0; k < np; ++k)
            if (pc[k] != 0.0) { pq[nq] = pq[k]; pc[nq] = pc[k]; ++nq; }
        for (int a = 1; a < nq; ++a)                       // (at most four: an insertion sort by pair index)
            for (int c = a; c > 0 && pq[c - 1] > pq[c]; --c) { std::swap(pq[c - 1], pq[c]); std::swap(pc[c - 1], pc[c]); }
        if (nq == 0) { for (int k = 0; k < 6; ++k) o[k] = nan; continue; }
        // step 2: the used blocks
        used.clear();
        for (int32_t b = 0; b < B; ++b) {
            bool ok = true;
            for (int k = 0; k < nq; ++k) ok = ok && cnt[b * pairs + pq[k]] >= 1;
            if (ok) used.push_back(b);
        }
        const int64_t G = (int64_t)used.size();
        // step 3: the totals, as integers
        __int128 S[4] = {0, 0, 0, 0};
        int64_t C[4] = {0, 0, 0, 0};
        for (int32_t b : used)
            for (int k = 0; k < nq; ++k) { S[k] += acc[b * pairs + pq[k]]; C[k] += cnt[b * pairs + pq[k]]; }
        int64_t minc = C[0];
        for (int k = 1; k < nq; ++k) minc = std::min(minc, C[k]);
        o[4] = (double)G; o[5] = (double)minc;
        if (G < 2) { o[0] = o[1] = o[2] = o[3] = nan; continue; }
        double theta = 0.0;
        for (int k = 0; k < nq; ++k) theta += pc[k] * (((double)S[k] * grid) / (double)C[k]);
        // step 4: the weighted jackknife
        tminus.assign((size_t)G, 0.0); mb.assign((size_t)G, 0.0);
        int64_t n = 0;
        for (int64_t u = 0; u < G; ++u) {
            const int32_t b = used[(size_t)u];
            double tm = 0.0;
            int64_t m = 0;
            for (int k = 0; k < nq; ++k) {
                const int64_t cb = cnt[b * pairs + pq[k]];
                tm += pc[k] * (((double)(S[k] - acc[b * pairs + pq[k]]) * grid) / (double)(C[k] - cb));
                m += cb;
            }
            tminus[(size_t)u] = tm; mb[(size_t)u] = (double)m; n += m;
        }
        const double nn = (double)n, Gd = (double)G;
        double sub = 0.0;
        for (int64_t u = 0; u < G; ++u) sub += ((nn - mb[(size_t)u]) / nn) * tminus[(size_t)u];
        const double tj = Gd * theta - sub;
        double var = 0.0;
        for (int64_t u = 0; u < G; ++u) {
            const double hb = nn / mb[(size_t)u];
            const double tau = hb * theta - (hb - 1.0) * tminus[(size_t)u];
            const double e = tau - tj;
            var += (e * e) / (hb - 1.0);
        }
        var = (1.0 / Gd) * var;
        const double se = std::sqrt(var);
        o[0] = theta; o[1] = tj; o[2] = se; o[3] = theta / se;
    }
    return GPCA_OK;
}
