// gpca_sample_counts / gpca_het_weights / gpca_sample_het (include/gpca.h section a18): what a sample looks like over the kept rows of a
// band -- its observed, heterozygous and homozygous-A1 calls and a weighted count of its observed rows -- and the two host rules that
// turn a row's QC counts into its weight and a sample's sums into its inbreeding coefficient F.  The call has its own workspace,
// allocated and freed per call, and reads nothing of the handle's state but the genotypes and the list of kept rows: one pass over the
// band's kept rows (k_sample_counts) leaves a slab per row split, a second kernel adds the slabs (k_sc_sum).
#include "gpca_internal.h"

#pragma clang fp contract(off)

using namespace gpca;

namespace {
struct ScWs {
    unsigned *part = nullptr, *counts = nullptr, *q = nullptr;
    unsigned long long *qpart = nullptr, *qsum = nullptr, *bad = nullptr;
    ~ScWs() { dfree(part); dfree(counts); dfree(q); dfree(qpart); dfree(qsum); dfree(bad); }
};
constexpr uint32_t kScQMax = 1u << 30;
}  // namespace

extern "C" int gpca_sample_counts(gpca_handle* h, int64_t row0, int64_t row1, const uint32_t* q, uint32_t* counts, uint64_t* qsum) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_sample_counts");
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on) return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels, which is not implemented");
    if (multi_rank(h)) return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    const int64_t K = h->n_pca, N = h->N;
    if (!counts) return fail(h, GPCA_ERR_BAD_ARG, f + ": counts is required");
    if ((q != nullptr) != (qsum != nullptr)) return fail(h, GPCA_ERR_BAD_ARG, f + ": q and qsum go together (both or neither)");
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    const int64_t rows = row1 - row0;
    if (rows >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": a band of 2^31 or more rows (the counts are 32-bit): ask for fewer rows");
    unsigned long long qtot = 0;
    if (q)
        for (int64_t j = 0; j < rows; ++j) {
            if (q[j] > kScQMax) return fail(h, GPCA_ERR_BAD_ARG, f + ": q[" + std::to_string(j) + "] = " + std::to_string(q[j]) + " is above 2^30");
            qtot += q[j];
        }
    if (rows == 0) {                                                                 // written, not added to: an empty band is all zero
        std::fill(counts, counts + 3 * N, 0u);
        if (qsum) std::fill(qsum, qsum + N, (uint64_t)0);
        return GPCA_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    int64_t forced = 0;
    if (const char* e = std::getenv("GPCA_SAMPLE_COUNTS_SPLITS")) {                  // read per call: the tests' way to every split edge
        forced = std::strtoll(e, nullptr, 10);
        if (forced < 1) forced = 1;
    }
    const ScPlan plan = sc_plan(rows, N, cus, forced);
    if (sc_grid(plan) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band makes 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the band needs", sc_call_bytes(N, rows, plan.splits, q != nullptr) + (double)(64 << 20)));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    ScWs ws;
    HIPCHK(dalloc(ws.part, (size_t)sc_part_capacity(plan.splits, N))); HIPCHK(dalloc(ws.counts, (size_t)sc_counts_capacity(N))); HIPCHK(dalloc(ws.bad, 1));
    if (q) {
        HIPCHK(dalloc(ws.qpart, (size_t)sc_qpart_capacity(plan.splits, N))); HIPCHK(dalloc(ws.qsum, (size_t)sc_qsum_capacity(N)));
        HIPCHK(dalloc(ws.q, (size_t)sc_q_capacity(rows)));
        HIPCHK(hipMemcpyAsync(ws.q, q, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    {
        // ops as DESIGN counts them: three indicator adds per call; bytes: the band's calls once
        ScopedTimer t(h, "sample_counts", 3.0 * (double)rows * (double)N, (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_sample_counts(st, G, packed, ldr, h->d_pca_rows, N, ws.q, row0, row1, plan, ws.part, ws.qpart, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
        launch_sc_sum(st, ws.part, ws.qpart, N, plan.splits, rows, qtot, ws.counts, ws.qsum);
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    HIPCHK(hipMemcpyAsync(counts, ws.counts, (size_t)sc_counts_capacity(N) * 4, hipMemcpyDeviceToHost, st));
    if (q) HIPCHK(hipMemcpyAsync(qsum, ws.qsum, (size_t)sc_qsum_capacity(N) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}

extern "C" int gpca_het_weights(const uint32_t* qc, int64_t rows, uint32_t* q) {
    if (!qc || !q || rows < 0) return GPCA_ERR_BAD_ARG;
    for (int64_t i = 0; i < rows; ++i) {
        const uint32_t* c = qc + 4 * i;
        if (c[0] == 0u) { q[i] = 0u; continue; }
        const double tn = 2.0 * (double)c[0];
        const double p = ((double)c[2] + 2.0 * (double)c[3]) / tn;
        const double e = ((2.0 * p) * (1.0 - p)) * (tn / (tn - 1.0));
        q[i] = (uint32_t)std::floor(e * 1073741824.0 + 0.5);
    }
    return GPCA_OK;
}

extern "C" int gpca_sample_het(const uint32_t* counts, const uint64_t* qsum, int64_t N, double* out) {
    if (!counts || !qsum || !out || N < 0) return GPCA_ERR_BAD_ARG;
    for (int64_t n = 0; n < N; ++n) {
        const double nobs = (double)counts[3 * n];
        const double ohom = nobs - (double)counts[3 * n + 1];
        const double ehom = nobs - (double)qsum[n] / 1073741824.0;
        const double den = nobs - ehom;
        out[3 * n] = ohom; out[3 * n + 1] = ehom;
        out[3 * n + 2] = (counts[3 * n] == 0u || !(den > 0.0)) ? std::nan("") : (ohom - ehom) / den;
    }
    return GPCA_OK;
}
