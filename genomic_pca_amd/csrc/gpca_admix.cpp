// gpca_admix_init / gpca_admix_step / gpca_admix (include/gpca.h section a21): admixture proportions Q and ancestral frequencies F of the
// ADMIXTURE model over the kept rows of a resident handle, fitted by EM with an optional SQUAREM acceleration.  Each call has its own
// workspace, allocated and freed per call, and reads nothing of the handle's state but the genotypes, the list of kept rows and (the
// init) the rows' QC counts.  One step is k_admix_step and the slab sums behind it (admix.hip); Q, F and every intermediate stay on the
// device, and per step only the log-likelihood -- per SQUAREM cycle also the two norms -- comes back to the host.
// gpca_admix_cv_fold / gpca_admix_step_holdout / gpca_admix_cv (section a22): the same step with the observed calls of one fold masked in
// the kernel, the same loop (adm_fit, which gpca_admix runs too) once per fold, and the held-out calls' deviance as the score.
#include "gpca_internal.h"
#include "philox.hpp"

#pragma clang fp contract(off)

using namespace gpca;

namespace {
constexpr float kEps = 1e-5f;
constexpr float kHi = 1.0f - 1e-5f;
struct AdmWs {
    float* theta[10] = {};                               // up to 5 parameter sets: Q at 2 s, F at 2 s + 1
    uint8_t* mode = nullptr;
    float *fpart = nullptr, *qpart = nullptr;
    double *llpart = nullptr, *npart = nullptr, *sums = nullptr;   // sums [3] = ll, sum r^2, sum v^2
    unsigned long long* bad = nullptr;
    double* cvsums = nullptr;                            // a hold-out call: [2] = ll, held ll
    unsigned long long* cvcnt = nullptr;                 //                  [2] = n_held, n_het_held
    ~AdmWs() {
        for (float*& p : theta) dfree(p);
        dfree(mode); dfree(fpart); dfree(qpart); dfree(llpart); dfree(npart); dfree(sums); dfree(bad); dfree(cvsums); dfree(cvcnt);
    }
    AdmSet set(int s) const { return AdmSet{theta[2 * s], theta[2 * s + 1]}; }
};

// the state a call needs, in a18's order, then K
int adm_check(gpca_handle* h, const std::string& f, int K) {
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on) return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels, which is not implemented");
    if (multi_rank(h)) return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    if (K < 1 || K > kAdmMaxK) return fail(h, GPCA_ERR_BAD_ARG, f + ": K must be 1 .. " + std::to_string(kAdmMaxK) + " (K = " + std::to_string(K) + ")");
    if (h->n_pca >= ((int64_t)1 << 31) || h->N >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 2^31 or more kept rows or samples");
    return GPCA_OK;
}
int adm_check_mode(gpca_handle* h, const std::string& f, const uint8_t* mode, int64_t N) {
    if (mode)
        for (int64_t n = 0; n < N; ++n)
            if (mode[n] > 2) return fail(h, GPCA_ERR_BAD_ARG, f + ": mode[" + std::to_string(n) + "] = " + std::to_string((int)mode[n]) + " is not 0, 1 or 2");
    return GPCA_OK;
}
// a Q row is non-negative with a positive sum, an F value lies in [0, 1]
int adm_check_theta(gpca_handle* h, const std::string& f, const float* Q, const float* F, int64_t N, int64_t rows, int K) {
    for (int64_t n = 0; n < N; ++n) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) {
            const float q = Q[n * K + k];
            if (!(q >= 0.0f) || !std::isfinite(q)) return fail(h, GPCA_ERR_BAD_ARG, f + ": Q[" + std::to_string(n) + "][" + std::to_string(k) + "] is negative or not finite");
            s += (double)q;
        }
        if (!(s > 0.0)) return fail(h, GPCA_ERR_BAD_ARG, f + ": row " + std::to_string(n) + " of Q sums to zero");
    }
    for (int64_t e = 0; e < rows * K; ++e)
        if (!(F[e] >= 0.0f && F[e] <= 1.0f))
            return fail(h, GPCA_ERR_BAD_ARG, f + ": F[" + std::to_string(e / K) + "][" + std::to_string(e % K) + "] is outside [0, 1]");
    return GPCA_OK;
}
// the workspace of a call with `sets` parameter sets; hold: the call takes hold-out steps (llpart [partial][2], the sums and the counts)
int adm_alloc(gpca_handle* h, const std::string& f, AdmWs& ws, int64_t N, int64_t rows, int K, int sets, bool fit, bool hold = false) {
    const AdmPlan p = adm_plan(rows, N);
    CHK(preflight_device_memory(h, f.c_str(), "the kept rows need",
                                (hold ? adm_cv_call_bytes(N, rows, K, sets, fit) : adm_call_bytes(N, rows, K, sets, fit)) + (double)(64 << 20)));
    for (int s = 0; s < sets; ++s) {
        HIPCHK(dalloc(ws.theta[2 * s], (size_t)adm_q_capacity(N, K))); HIPCHK(dalloc(ws.theta[2 * s + 1], (size_t)adm_f_capacity(rows, K)));
    }
    HIPCHK(dalloc(ws.mode, (size_t)N));
    HIPCHK(dalloc(ws.fpart, (size_t)adm_fpart_capacity(p, rows, K))); HIPCHK(dalloc(ws.qpart, (size_t)adm_qpart_capacity(p, N, K)));
    HIPCHK(dalloc(ws.llpart, (size_t)(hold ? adm_cv_llpart_capacity(p) : adm_llpart_capacity(p))));
    if (hold) { HIPCHK(dalloc(ws.cvsums, (size_t)adm_cv_sums_capacity())); HIPCHK(dalloc(ws.cvcnt, (size_t)adm_cv_count_capacity())); }
    if (fit) HIPCHK(dalloc(ws.npart, (size_t)adm_npart_capacity(N, rows, K)));
    HIPCHK(dalloc(ws.sums, 3)); HIPCHK(dalloc(ws.bad, 1));
    return GPCA_OK;
}
// one step from set a to set b on the stream; *ll (host) is valid once the stream is synchronised.  hold.folds != 0: the hold-out step,
// whose two sums stay in ws.cvsums and whose counts are added to ws.cvcnt
int adm_step(gpca_handle* h, const std::string& f, const AdmWs& ws, bool has_mode, int K, int a, int b, double* ll, AdmHold hold = AdmHold{}) {
    const int64_t rows = h->n_pca, N = h->N;
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    {
        // ops as DESIGN counts them: 6 K multiply-adds per call; bytes: the kept rows' calls once
        const bool held = hold.folds != 0;
        hold.counts = ws.cvcnt;
        ScopedTimer t(h, held ? "admix_step_holdout" : "admix_step", 12.0 * (double)K * (double)rows * (double)N, (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_admix_step(h->st, G, packed, ldr, h->d_pca_rows, rows, N, K, ws.theta[2 * a], ws.theta[2 * a + 1], has_mode ? ws.mode : nullptr,
                              ws.fpart, ws.qpart, ws.llpart, ws.theta[2 * b], ws.theta[2 * b + 1], held ? ws.cvsums : ws.sums, ws.bad, hold) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(ll, hold.folds != 0 ? ws.cvsums : ws.sums, 8, hipMemcpyDeviceToHost, h->st));
    return GPCA_OK;
}
int adm_check_params(gpca_handle* h, const std::string& f, const gpca_admix_params* params) {
    if (!(params->tol >= 0.0)) return fail(h, GPCA_ERR_BAD_ARG, f + ": tol must be at least 0");
    if (params->max_iter < 0) return fail(h, GPCA_ERR_BAD_ARG, f + ": max_iter must be at least 0");
    if ((params->accel != 0 && params->accel != 1) || (params->init != 0 && params->init != 1))
        return fail(h, GPCA_ERR_BAD_ARG, f + ": accel and init are 0 or 1");
    return GPCA_OK;
}
int adm_check_folds(gpca_handle* h, const std::string& f, int folds) {
    if (folds < kAdmCvMinFolds || folds > kAdmCvMaxFolds)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": folds must be " + std::to_string(kAdmCvMinFolds) + " .. " + std::to_string(kAdmCvMaxFolds) + " (folds = " + std::to_string(folds) + ")");
    return GPCA_OK;
}
// init = 1: the caller's Q and F are checked and clamped into q0 and f0: F to [eps, 1 - eps]; a free row of Q that holds a value below
// eps to max(q, eps) / (their sum)
int adm_start(gpca_handle* h, const std::string& f, const uint8_t* mode, const float* Q, const float* F, int64_t N, int64_t rows, int K,
              std::vector<float>& q0, std::vector<float>& f0) {
    CHK(adm_check_theta(h, f, Q, F, N, rows, K));
    q0.assign(Q, Q + (size_t)adm_q_capacity(N, K)); f0.assign(F, F + (size_t)adm_f_capacity(rows, K));
    for (float& v : f0) v = v < kEps ? kEps : v > kHi ? kHi : v;
    for (int64_t n = 0; n < N; ++n) {
        if (mode && mode[n] == 1) continue;
        float* r = q0.data() + n * K;
        bool low = false;
        for (int k = 0; k < K; ++k) low = low || r[k] < kEps;
        if (!low) continue;
        float s = 0.0f;
        for (int k = 0; k < K; ++k) { r[k] = r[k] > kEps ? r[k] : kEps; s += r[k]; }
        for (int k = 0; k < K; ++k) r[k] = r[k] / s;
    }
    return GPCA_OK;
}
// The fit's loop (a21), which gpca_admix and every fold of gpca_admix_cv run: from the start (q0 / f0 when init = 1, else the philox init
// of the seed) in set 0, with `hold` on every step (folds = 0: the plain step).  ws holds 5 sets and the mode bytes; *cur = the set of the
// returned parameters, a free set is (*cur + 1) % 5.
struct AdmFitOut { int64_t steps = 0, cycles = 0, fallbacks = 0; int converged = 0; double loglik = 0.0; };
int adm_fit(gpca_handle* h, const std::string& f, const AdmWs& ws, const gpca_admix_params* params, bool has_mode, const std::vector<float>& q0,
            const std::vector<float>& f0, const AdmHold& hold, double* trace, int64_t trace_cap, AdmFitOut* out, int* cur_out) {
    const int64_t rows = h->n_pca, N = h->N;
    const int K = params->K;
    const size_t nq = (size_t)adm_q_capacity(N, K), nf = (size_t)adm_f_capacity(rows, K);
    hipStream_t st = h->st;
    if (params->init == 1) {
        HIPCHK(hipMemcpyAsync(ws.theta[0], q0.data(), nq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.theta[1], f0.data(), nf * 4, hipMemcpyHostToDevice, st));
    } else {
        if (launch_admix_init(st, h->d_pca_rows, h->d_counts, rows, N, K, params->seed, ws.theta[0], ws.theta[1]) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));

    // the sets: cur = theta0 of the cycle; the other four are handed round
    int cur = 0, s1 = 1, s2 = 2, sx = 3, s3 = 4;
    int64_t steps = 0, cycles = 0, fallbacks = 0;
    int converged = 0;
    double prev = 0.0, last = std::nan("");
    while (steps < params->max_iter) {
        double l0 = 0.0;
        CHK(adm_step(h, f, ws, has_mode, K, cur, s1, &l0, hold));
        if (steps == 0) CHK(asc_check_genotypes(h, f, ws.bad, st));
        else HIPCHK(hipStreamSynchronize(st));
        ++steps;
        if (cycles < trace_cap) trace[cycles] = l0;
        const bool had_prev = cycles > 0;
        ++cycles;
        last = l0;
        if (had_prev && l0 - prev < params->tol * std::fabs(l0)) { converged = 1; std::swap(cur, s1); break; }
        prev = l0;
        if (!params->accel || steps >= params->max_iter) { std::swap(cur, s1); continue; }
        double l1 = 0.0;
        CHK(adm_step(h, f, ws, has_mode, K, s1, s2, &l1, hold));
        ++steps;
        CHK(launch_admix_norms(st, rows, N, K, ws.set(cur), ws.set(s1), ws.set(s2), ws.npart, ws.sums + 1) != 0 ? fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused") : GPCA_OK);
        HIPCHK(hipGetLastError());
        double nrm[2] = {0.0, 0.0};
        HIPCHK(hipMemcpyAsync(nrm, ws.sums + 1, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!(nrm[1] > 0.0)) { ++fallbacks; std::swap(cur, s2); continue; }          // ||v|| = 0: from theta2
        if (steps >= params->max_iter) { std::swap(cur, s2); continue; }
        const double alpha = std::min(-std::sqrt(nrm[0]) / std::sqrt(nrm[1]), -1.0);
        CHK(launch_admix_extrap(st, rows, N, K, ws.set(cur), ws.set(s1), ws.set(s2), has_mode ? ws.mode : nullptr, alpha, ws.set(sx)) != 0 ? fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused") : GPCA_OK);
        HIPCHK(hipGetLastError());
        double lx = 0.0;
        CHK(adm_step(h, f, ws, has_mode, K, sx, s3, &lx, hold));
        HIPCHK(hipStreamSynchronize(st));
        ++steps;
        if (lx >= l1) std::swap(cur, s3);
        else { ++fallbacks; std::swap(cur, s2); }
    }
    out->steps = steps; out->cycles = cycles; out->fallbacks = fallbacks; out->converged = converged; out->loglik = last;
    *cur_out = cur;
    return GPCA_OK;
}
// one hold-out step from set a to set b, with the counts zeroed first; the sums and the counts come back once the stream is synchronised
int adm_score(gpca_handle* h, const std::string& f, const AdmWs& ws, bool has_mode, int K, int a, int b, const AdmHold& hold, double* sums2,
              unsigned long long* cnt2) {
    HIPCHK(hipMemsetAsync(ws.cvcnt, 0, 8 * (size_t)adm_cv_count_capacity(), h->st));
    CHK(adm_step(h, f, ws, has_mode, K, a, b, &sums2[0], hold));
    HIPCHK(hipMemcpyAsync(sums2, ws.cvsums, 8 * (size_t)adm_cv_sums_capacity(), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(cnt2, ws.cvcnt, 8 * (size_t)adm_cv_count_capacity(), hipMemcpyDeviceToHost, h->st));
    return GPCA_OK;
}
}  // namespace

extern "C" int gpca_admix_init(gpca_handle* h, int32_t K, uint64_t seed, float* Q, float* F) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_admix_init");
    if (!Q || !F) return fail(h, GPCA_ERR_BAD_ARG, f + ": Q and F are required");
    CHK(adm_check(h, f, K));
    const int64_t rows = h->n_pca, N = h->N;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the kept rows need", 4.0 * (double)(adm_q_capacity(N, K) + adm_f_capacity(rows, K)) + (double)(64 << 20)));
    AdmWs ws;
    HIPCHK(dalloc(ws.theta[0], (size_t)adm_q_capacity(N, K))); HIPCHK(dalloc(ws.theta[1], (size_t)adm_f_capacity(rows, K)));
    if (launch_admix_init(h->st, h->d_pca_rows, h->d_counts, rows, N, K, seed, ws.theta[0], ws.theta[1]) != 0)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(Q, ws.theta[0], (size_t)adm_q_capacity(N, K) * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(F, ws.theta[1], (size_t)adm_f_capacity(rows, K) * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return GPCA_OK;
}

extern "C" int gpca_admix_step(gpca_handle* h, int32_t K, const float* Q, const float* F, const uint8_t* mode, float* Qn, float* Fn, double* loglik) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_admix_step");
    if (!Q || !F || !Qn || !Fn || !loglik) return fail(h, GPCA_ERR_BAD_ARG, f + ": Q, F, Qn, Fn and loglik are required");
    CHK(adm_check(h, f, K));
    const int64_t rows = h->n_pca, N = h->N;
    CHK(adm_check_mode(h, f, mode, N));
    CHK(adm_check_theta(h, f, Q, F, N, rows, K));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    AdmWs ws;
    CHK(adm_alloc(h, f, ws, N, rows, K, 2, false));
    hipStream_t st = h->st;
    HIPCHK(hipMemcpyAsync(ws.theta[0], Q, (size_t)adm_q_capacity(N, K) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.theta[1], F, (size_t)adm_f_capacity(rows, K) * 4, hipMemcpyHostToDevice, st));
    if (mode) HIPCHK(hipMemcpyAsync(ws.mode, mode, (size_t)N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    double ll = 0.0;
    CHK(adm_step(h, f, ws, mode != nullptr, K, 0, 1, &ll));
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    HIPCHK(hipMemcpyAsync(Qn, ws.theta[2], (size_t)adm_q_capacity(N, K) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(Fn, ws.theta[3], (size_t)adm_f_capacity(rows, K) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *loglik = ll;
    return GPCA_OK;
}

extern "C" int gpca_admix(gpca_handle* h, const gpca_admix_params* params, const uint8_t* mode, float* Q, float* F, gpca_admix_info* info) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_admix");
    if (!params || !Q || !F || !info) return fail(h, GPCA_ERR_BAD_ARG, f + ": params, Q, F and info are required");
    const int K = params->K;
    CHK(adm_check(h, f, K));
    CHK(adm_check_params(h, f, params));
    if (info->trace_cap < 0 || (info->trace_cap > 0 && !info->trace)) return fail(h, GPCA_ERR_BAD_ARG, f + ": trace is required with trace_cap > 0");
    const int64_t rows = h->n_pca, N = h->N;
    CHK(adm_check_mode(h, f, mode, N));
    const size_t nq = (size_t)adm_q_capacity(N, K), nf = (size_t)adm_f_capacity(rows, K);
    std::vector<float> q0, f0;
    if (params->init == 1) CHK(adm_start(h, f, mode, Q, F, N, rows, K, q0, f0));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    AdmWs ws;
    CHK(adm_alloc(h, f, ws, N, rows, K, 5, true));
    hipStream_t st = h->st;
    if (mode) HIPCHK(hipMemcpyAsync(ws.mode, mode, (size_t)N, hipMemcpyHostToDevice, st));
    AdmFitOut o;
    int cur = 0;
    CHK(adm_fit(h, f, ws, params, mode != nullptr, q0, f0, AdmHold{}, info->trace, info->trace_cap, &o, &cur));
    HIPCHK(hipMemcpyAsync(Q, ws.theta[2 * cur], nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(F, ws.theta[2 * cur + 1], nf * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    info->steps = o.steps; info->cycles = o.cycles; info->converged = o.converged; info->fallbacks = (int32_t)o.fallbacks; info->loglik = o.loglik;
    return GPCA_OK;
}

// ---- a22: the cross-validation error ------------------------------------------------------------------------------------------------
extern "C" int gpca_admix_cv_fold(uint64_t seed, int32_t folds, int64_t row0, int64_t rows, int64_t N, uint8_t* out) {
    if (!out || folds < kAdmCvMinFolds || folds > kAdmCvMaxFolds || row0 < 0 || rows < 0 || N < 0 || row0 + rows > ((int64_t)1 << 31) ||
        N > ((int64_t)1 << 31))
        return GPCA_ERR_BAD_ARG;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t i = row0 + r;
        for (int64_t j = 0; j < N; ++j) {
            const philox_out o = philox4x32_10((uint32_t)j, (uint32_t)(i >> 2), 0u, GPCA_STREAM_ADMIX_CV, (uint32_t)seed, (uint32_t)(seed >> 32));
            out[r * N + j] = (uint8_t)adm_cv_fold_of(o.v[i & 3], (uint32_t)folds);
        }
    }
    return GPCA_OK;
}

extern "C" int gpca_admix_step_holdout(gpca_handle* h, int32_t K, const float* Q, const float* F, const uint8_t* mode, int32_t folds, int32_t fold,
                                       uint64_t cv_seed, float* Qn, float* Fn, double* loglik, double* held_loglik, int64_t* n_held,
                                       int64_t* n_het_held) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_admix_step_holdout");
    if (!Q || !F || !Qn || !Fn || !loglik || !held_loglik || !n_held || !n_het_held)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": Q, F, Qn, Fn, loglik, held_loglik, n_held and n_het_held are required");
    CHK(adm_check(h, f, K));
    CHK(adm_check_folds(h, f, folds));
    if (fold < 0 || fold >= folds) return fail(h, GPCA_ERR_BAD_ARG, f + ": fold must be 0 .. folds - 1 (fold = " + std::to_string(fold) + ")");
    const int64_t rows = h->n_pca, N = h->N;
    CHK(adm_check_mode(h, f, mode, N));
    CHK(adm_check_theta(h, f, Q, F, N, rows, K));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    AdmWs ws;
    CHK(adm_alloc(h, f, ws, N, rows, K, 2, false, true));
    hipStream_t st = h->st;
    HIPCHK(hipMemcpyAsync(ws.theta[0], Q, (size_t)adm_q_capacity(N, K) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.theta[1], F, (size_t)adm_f_capacity(rows, K) * 4, hipMemcpyHostToDevice, st));
    if (mode) HIPCHK(hipMemcpyAsync(ws.mode, mode, (size_t)N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    AdmHold hold; hold.folds = folds; hold.fold = fold; hold.seed = cv_seed;
    double sums[2] = {0.0, 0.0};
    unsigned long long cnt[2] = {0, 0};
    CHK(adm_score(h, f, ws, mode != nullptr, K, 0, 1, hold, sums, cnt));
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    HIPCHK(hipMemcpyAsync(Qn, ws.theta[2], (size_t)adm_q_capacity(N, K) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(Fn, ws.theta[3], (size_t)adm_f_capacity(rows, K) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *loglik = sums[0]; *held_loglik = sums[1]; *n_held = (int64_t)cnt[0]; *n_het_held = (int64_t)cnt[1];
    return GPCA_OK;
}

extern "C" int gpca_admix_cv(gpca_handle* h, const gpca_admix_params* params, const uint8_t* mode, int32_t folds, uint64_t cv_seed, const float* Q0,
                             const float* F0, gpca_admix_cv_fold_info* out, double* cv_error) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_admix_cv");
    if (!params || !out || !cv_error) return fail(h, GPCA_ERR_BAD_ARG, f + ": params, out and cv_error are required");
    const int K = params->K;
    CHK(adm_check(h, f, K));
    CHK(adm_check_folds(h, f, folds));
    CHK(adm_check_params(h, f, params));
    if (params->init == 1 && (!Q0 || !F0)) return fail(h, GPCA_ERR_BAD_ARG, f + ": Q0 and F0 are required with init = 1");
    const int64_t rows = h->n_pca, N = h->N;
    CHK(adm_check_mode(h, f, mode, N));
    std::vector<float> q0, f0;
    if (params->init == 1) CHK(adm_start(h, f, mode, Q0, F0, N, rows, K, q0, f0));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    AdmWs ws;
    CHK(adm_alloc(h, f, ws, N, rows, K, 5, true, true));
    hipStream_t st = h->st;
    if (mode) HIPCHK(hipMemcpyAsync(ws.mode, mode, (size_t)N, hipMemcpyHostToDevice, st));
    double dev_sum = 0.0;
    int64_t held_sum = 0;
    for (int c = 0; c < folds; ++c) {
        AdmHold hold; hold.folds = folds; hold.fold = c; hold.seed = cv_seed;
        AdmFitOut o;
        int cur = 0;
        CHK(adm_fit(h, f, ws, params, mode != nullptr, q0, f0, hold, nullptr, 0, &o, &cur));
        // the score: one more hold-out step at the returned parameters, whose Q' and F' go to a free set and are dropped
        double sums[2] = {0.0, 0.0};
        unsigned long long cnt[2] = {0, 0};
        CHK(adm_score(h, f, ws, mode != nullptr, K, cur, (cur + 1) % 5, hold, sums, cnt));
        CHK(asc_check_genotypes(h, f, ws.bad, st));
        gpca_admix_cv_fold_info& r = out[c];
        r.steps = o.steps; r.cycles = o.cycles; r.converged = o.converged; r.fallbacks = (int32_t)o.fallbacks; r.loglik = o.loglik;
        r.held_loglik = sums[1]; r.n_held = (int64_t)cnt[0]; r.n_het_held = (int64_t)cnt[1];
        r.deviance = -2.0 * sums[1] - 4.0 * 0.69314718055994530942 * (double)r.n_het_held;
        dev_sum += r.deviance; held_sum += r.n_held;
    }
    *cv_error = held_sum > 0 ? dev_sum / (double)held_sum : std::nan("");
    return GPCA_OK;
}
