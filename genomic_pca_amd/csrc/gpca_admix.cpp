// gpca_admix_init / gpca_admix_step / gpca_admix (include/gpca.h section a21): admixture proportions Q and ancestral frequencies F of the
// ADMIXTURE model over the kept rows of a resident handle, fitted by EM with an optional SQUAREM acceleration.  Each call has its own
// workspace, allocated and freed per call, and reads nothing of the handle's state but the genotypes, the list of kept rows and (the
// init) the rows' QC counts.  One step is k_admix_step and the slab sums behind it (admix.hip); Q, F and every intermediate stay on the
// device, and per step only the log-likelihood -- per SQUAREM cycle also the two norms -- comes back to the host.
#include "gpca_internal.h"

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
    ~AdmWs() { for (float*& p : theta) dfree(p); dfree(mode); dfree(fpart); dfree(qpart); dfree(llpart); dfree(npart); dfree(sums); dfree(bad); }
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
// the workspace of a call with `sets` parameter sets
int adm_alloc(gpca_handle* h, const std::string& f, AdmWs& ws, int64_t N, int64_t rows, int K, int sets, bool fit) {
    const AdmPlan p = adm_plan(rows, N);
    CHK(preflight_device_memory(h, f.c_str(), "the kept rows need", adm_call_bytes(N, rows, K, sets, fit) + (double)(64 << 20)));
    for (int s = 0; s < sets; ++s) {
        HIPCHK(dalloc(ws.theta[2 * s], (size_t)adm_q_capacity(N, K))); HIPCHK(dalloc(ws.theta[2 * s + 1], (size_t)adm_f_capacity(rows, K)));
    }
    HIPCHK(dalloc(ws.mode, (size_t)N));
    HIPCHK(dalloc(ws.fpart, (size_t)adm_fpart_capacity(p, rows, K))); HIPCHK(dalloc(ws.qpart, (size_t)adm_qpart_capacity(p, N, K)));
    HIPCHK(dalloc(ws.llpart, (size_t)adm_llpart_capacity(p)));
    if (fit) HIPCHK(dalloc(ws.npart, (size_t)adm_npart_capacity(N, rows, K)));
    HIPCHK(dalloc(ws.sums, 3)); HIPCHK(dalloc(ws.bad, 1));
    return GPCA_OK;
}
// one step from set a to set b on the stream; *ll (host) is valid once the stream is synchronised
int adm_step(gpca_handle* h, const std::string& f, const AdmWs& ws, bool has_mode, int K, int a, int b, double* ll) {
    const int64_t rows = h->n_pca, N = h->N;
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    {
        // ops as DESIGN counts them: 6 K multiply-adds per call; bytes: the kept rows' calls once
        ScopedTimer t(h, "admix_step", 12.0 * (double)K * (double)rows * (double)N, (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_admix_step(h->st, G, packed, ldr, h->d_pca_rows, rows, N, K, ws.theta[2 * a], ws.theta[2 * a + 1], has_mode ? ws.mode : nullptr,
                              ws.fpart, ws.qpart, ws.llpart, ws.theta[2 * b], ws.theta[2 * b + 1], ws.sums, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(ll, ws.sums, 8, hipMemcpyDeviceToHost, h->st));
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
    if (!(params->tol >= 0.0)) return fail(h, GPCA_ERR_BAD_ARG, f + ": tol must be at least 0");
    if (params->max_iter < 0) return fail(h, GPCA_ERR_BAD_ARG, f + ": max_iter must be at least 0");
    if ((params->accel != 0 && params->accel != 1) || (params->init != 0 && params->init != 1))
        return fail(h, GPCA_ERR_BAD_ARG, f + ": accel and init are 0 or 1");
    if (info->trace_cap < 0 || (info->trace_cap > 0 && !info->trace)) return fail(h, GPCA_ERR_BAD_ARG, f + ": trace is required with trace_cap > 0");
    const int64_t rows = h->n_pca, N = h->N;
    CHK(adm_check_mode(h, f, mode, N));
    const size_t nq = (size_t)adm_q_capacity(N, K), nf = (size_t)adm_f_capacity(rows, K);
    std::vector<float> q0, f0;
    if (params->init == 1) {
        CHK(adm_check_theta(h, f, Q, F, N, rows, K));
        // the inputs are clamped: F to [eps, 1 - eps]; a free row of Q that holds a value below eps to max(q, eps) / (their sum)
        q0.assign(Q, Q + nq); f0.assign(F, F + nf);
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
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    AdmWs ws;
    CHK(adm_alloc(h, f, ws, N, rows, K, 5, true));
    hipStream_t st = h->st;
    if (params->init == 1) {
        HIPCHK(hipMemcpyAsync(ws.theta[0], q0.data(), nq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.theta[1], f0.data(), nf * 4, hipMemcpyHostToDevice, st));
    } else {
        if (launch_admix_init(st, h->d_pca_rows, h->d_counts, rows, N, K, params->seed, ws.theta[0], ws.theta[1]) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    if (mode) HIPCHK(hipMemcpyAsync(ws.mode, mode, (size_t)N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));

    // the sets: cur = theta0 of the cycle; the other four are handed round
    int cur = 0, s1 = 1, s2 = 2, sx = 3, s3 = 4;
    int64_t steps = 0, cycles = 0, fallbacks = 0;
    int converged = 0;
    double prev = 0.0, last = std::nan("");
    const bool has_mode = mode != nullptr;
    while (steps < params->max_iter) {
        double l0 = 0.0;
        CHK(adm_step(h, f, ws, has_mode, K, cur, s1, &l0));
        if (steps == 0) CHK(asc_check_genotypes(h, f, ws.bad, st));
        else HIPCHK(hipStreamSynchronize(st));
        ++steps;
        if (cycles < info->trace_cap) info->trace[cycles] = l0;
        const bool had_prev = cycles > 0;
        ++cycles;
        last = l0;
        if (had_prev && l0 - prev < params->tol * std::fabs(l0)) { converged = 1; std::swap(cur, s1); break; }
        prev = l0;
        if (!params->accel || steps >= params->max_iter) { std::swap(cur, s1); continue; }
        double l1 = 0.0;
        CHK(adm_step(h, f, ws, has_mode, K, s1, s2, &l1));
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
        CHK(adm_step(h, f, ws, has_mode, K, sx, s3, &lx));
        HIPCHK(hipStreamSynchronize(st));
        ++steps;
        if (lx >= l1) std::swap(cur, s3);
        else { ++fallbacks; std::swap(cur, s2); }
    }
    HIPCHK(hipMemcpyAsync(Q, ws.theta[2 * cur], nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(F, ws.theta[2 * cur + 1], nf * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    info->steps = steps; info->cycles = cycles; info->converged = converged; info->fallbacks = (int32_t)fallbacks; info->loglik = last;
    return GPCA_OK;
}
