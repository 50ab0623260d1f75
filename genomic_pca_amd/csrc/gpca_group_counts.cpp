// gpca_group_counts / gpca_fst_hudson / gpca_fst_wc (include/gpca.h section a17): the genotype counts of every kept row inside every
// one of P sample groups, and the two host rules that turn them into Fst.  The call has its own workspace, allocated and freed per call,
// and reads nothing of the handle's state but the genotypes and the list of kept rows: one kernel builds the one-hot matrix of the
// labels, one pass over the band's kept rows multiplies it on the matrix cores (k_group_counts).
#include "gpca_internal.h"

#pragma clang fp contract(off)

using namespace gpca;

static_assert(GPCA_GROUPS_MAX == kGcMaxGroups, "include/gpca.h and plan_math.h");

namespace {
struct GcWs {
    uint8_t* onehot = nullptr;
    int32_t* label = nullptr;
    unsigned *size = nullptr, *counts = nullptr;
    unsigned long long* bad = nullptr;
    ~GcWs() { dfree(onehot); dfree(label); dfree(size); dfree(counts); dfree(bad); }
};
}  // namespace

extern "C" int gpca_group_counts(gpca_handle* h, const int32_t* group, int32_t P, int64_t row0, int64_t row1, uint32_t* counts) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_group_counts");
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on) return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels, which is not implemented");
    if (multi_rank(h)) return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    const int64_t K = h->n_pca, N = h->N;
    if (!group) return fail(h, GPCA_ERR_BAD_ARG, f + ": group is required");
    if (!counts) return fail(h, GPCA_ERR_BAD_ARG, f + ": counts is required");
    if (P < 1 || P > kGcMaxGroups) return fail(h, GPCA_ERR_BAD_ARG, f + ": P must satisfy 1 <= P <= " + std::to_string(kGcMaxGroups));
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    if (N >= ((int64_t)1 << 30)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 2^30 or more samples (the counts are 32-bit)");
    // the labels: a negative one is -1; the group sizes
    std::vector<int32_t> label((size_t)gc_label_capacity(N));
    std::vector<unsigned> size((size_t)gc_size_capacity(), 0u);
    for (int64_t n = 0; n < N; ++n) {
        const int32_t g = group[n];
        if (g >= P) return fail(h, GPCA_ERR_BAD_ARG, f + ": group[" + std::to_string(n) + "] = " + std::to_string(g) + " is not below P = " + std::to_string(P));
        label[(size_t)n] = g < 0 ? -1 : g;
        if (g >= 0) size[(size_t)g]++;
    }
    const int64_t rows = row1 - row0;
    if (rows == 0) return GPCA_OK;
    if (gc_row_blocks(rows) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band makes 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the band needs", gc_call_bytes(N, rows, P) + (double)(64 << 20)));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    GcWs ws;
    HIPCHK(dalloc(ws.onehot, (size_t)gc_onehot_capacity(N, P))); HIPCHK(dalloc(ws.label, (size_t)gc_label_capacity(N)));
    HIPCHK(dalloc(ws.size, (size_t)gc_size_capacity())); HIPCHK(dalloc(ws.counts, (size_t)gc_counts_capacity(rows, P))); HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(hipMemcpyAsync(ws.label, label.data(), label.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.size, size.data(), size.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    launch_gc_onehot(st, ws.label, N, P, ws.onehot);
    HIPCHK(hipGetLastError());
    {
        // ops as DESIGN counts them: two planes (het, hom) over the padded columns, the missing plane only where calls are missing
        ScopedTimer t(h, "group_counts", 2.0 * 2.0 * (double)rows * (double)N * (double)gc_ppad(P), (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_group_counts(st, G, packed, ldr, h->d_pca_rows, N, ws.onehot, ws.size, P, row0, row1, ws.counts, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    HIPCHK(hipMemcpyAsync(counts, ws.counts, (size_t)gc_counts_capacity(rows, P) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}

namespace {
// a group's allele count n = 2 n_obs and A1 frequency p = (n_het + 2 n_hom2) / n
inline void gc_freq(const uint32_t* c, double& n, double& p) {
    n = 2.0 * (double)c[0];
    p = ((double)c[1] + 2.0 * (double)c[2]) / n;
}
}  // namespace

extern "C" int gpca_fst_hudson(const uint32_t* counts, int64_t rows, int32_t P, double* num, double* den, double* sums) {
    if (!counts || !sums || rows < 0 || P < 2 || P > kGcMaxGroups) return GPCA_ERR_BAD_ARG;
    const int64_t pairs = (int64_t)P * (P - 1) / 2;
    const double nan = std::nan("");
    for (int64_t r = 0; r < rows; ++r) {
        const uint32_t* cr = counts + r * (int64_t)P * 3;
        for (int i = 1; i < P; ++i)
            for (int j = 0; j < i; ++j) {
                const int64_t q = (int64_t)i * (i - 1) / 2 + j;
                const uint32_t *ci = cr + 3 * i, *cj = cr + 3 * j;
                double nu = nan, de = nan;
                if (ci[0] >= 1u && cj[0] >= 1u) {
                    double ni, pi, nj, pj;
                    gc_freq(ci, ni, pi); gc_freq(cj, nj, pj);
                    const double d = pi - pj;
                    nu = (d * d - (pi * (1.0 - pi)) / (ni - 1.0)) - (pj * (1.0 - pj)) / (nj - 1.0);
                    de = pi * (1.0 - pj) + pj * (1.0 - pi);
                    sums[3 * q] += nu; sums[3 * q + 1] += de; sums[3 * q + 2] += 1.0;
                }
                if (num) num[r * pairs + q] = nu;
                if (den) den[r * pairs + q] = de;
            }
    }
    return GPCA_OK;
}

extern "C" int gpca_fst_wc(const uint32_t* counts, int64_t rows, int32_t P, const uint8_t* use, double* abc, double* sums) {
    if (!counts || !sums || rows < 0 || P < 1 || P > kGcMaxGroups) return GPCA_ERR_BAD_ARG;
    int used[kGcMaxGroups], r = 0;
    for (int p = 0; p < P; ++p) if (!use || use[p]) used[r++] = p;
    if (r < 2) return GPCA_ERR_BAD_ARG;
    const double rr = (double)r, nan = std::nan("");
    for (int64_t i = 0; i < rows; ++i) {
        const uint32_t* cr = counts + i * (int64_t)P * 3;
        bool ok = true;
        double nt = 0.0, sq = 0.0;
        for (int u = 0; u < r; ++u) {
            const double n = (double)cr[3 * used[u]];
            if (cr[3 * used[u]] < 1u) ok = false;
            nt += n; sq += n * n;
        }
        if (!ok || !(nt > rr)) {
            if (abc) abc[3 * i] = abc[3 * i + 1] = abc[3 * i + 2] = nan;
            continue;
        }
        double sp = 0.0, sh = 0.0;
        for (int u = 0; u < r; ++u) {
            const uint32_t* c = cr + 3 * used[u];
            double n2, p;
            gc_freq(c, n2, p);
            const double n = (double)c[0], hi = (double)c[1] / n;
            sp += n * p; sh += n * hi;
        }
        const double nbar = nt / rr, nc = (nt - sq / nt) / (rr - 1.0), pbar = sp / nt, hbar = sh / nt;
        double ss = 0.0;
        for (int u = 0; u < r; ++u) {
            const uint32_t* c = cr + 3 * used[u];
            double n2, p;
            gc_freq(c, n2, p);
            const double d = p - pbar;
            ss += (double)c[0] * (d * d);
        }
        const double s2 = ss / ((rr - 1.0) * nbar);
        const double core = pbar * (1.0 - pbar) - ((rr - 1.0) / rr) * s2;
        const double a = (nbar / nc) * (s2 - (core - hbar / 4.0) / (nbar - 1.0));
        const double b = (nbar / (nbar - 1.0)) * (core - ((2.0 * nbar - 1.0) / (4.0 * nbar)) * hbar);
        const double c = hbar / 2.0;
        if (abc) { abc[3 * i] = a; abc[3 * i + 1] = b; abc[3 * i + 2] = c; }
        sums[0] += a; sums[1] += (a + b) + c; sums[2] += 1.0;
    }
    return GPCA_OK;
}
