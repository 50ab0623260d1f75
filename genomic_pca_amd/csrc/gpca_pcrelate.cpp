// gpca_pcrelate_isaf / gpca_pcrelate (include/gpca.h section a11): PC-Relate from caller-supplied sample coordinates.  The design and
// the hat matrix are made on the host in f64 (P <= 32: a Cholesky of at most 33 x 33); one pass regresses every kept row on them
// (k_pcrelate_beta), then the band's tiles of the two pair sums run on the matrix cores (k_pcrelate).  The calls have their own
// workspace, allocated and freed per call, and read nothing of the handle's state but the genotypes and the list of kept rows.
#include "gpca_internal.h"

using namespace gpca;

namespace {
struct PcrWs {
    float *betaG = nullptr, *beta_rm = nullptr, *X = nullptr, *mu = nullptr;
    double *Hw = nullptr, *R = nullptr, *kin = nullptr;
    uint8_t* train = nullptr;
    unsigned long long* bad = nullptr;
    unsigned* inv = nullptr;
    int *Q = nullptr, *nsnp = nullptr;
    int2* tiles = nullptr;
    ~PcrWs() {
        dfree(betaG); dfree(beta_rm); dfree(X); dfree(mu); dfree(Hw); dfree(R); dfree(kin); dfree(train); dfree(bad); dfree(inv); dfree(Q);
        dfree(nsnp); dfree(tiles);
    }
};

// what both entry points check before they touch the device
int pcr_check(gpca_handle* h, const char* fn, const double* V, int32_t P) {
    const std::string f(fn);
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on)
        return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels; the f32 and f64 sums are not associative across panels, which is not implemented");
    if (multi_rank(h))
        return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows; the f32 and f64 sums are not associative across ranks, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    if (h->n_pca >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 2^31 or more kept rows (the counts are 32-bit)");
    if (P < 0 || P > kPcrMaxPcs) return fail(h, GPCA_ERR_BAD_ARG, f + ": P must lie in [0, " + std::to_string(kPcrMaxPcs) + "]");
    if (P > 0 && !V) return fail(h, GPCA_ERR_BAD_ARG, f + ": V is required when P > 0");
    return GPCA_OK;
}

// Step 1 (host, f64): x_n = (1, V_n1 / c_1, ..., V_nP / c_P), c_j = the root mean square of column j over the training samples;
// H = (X^T X)^-1 X^T over the training samples by Cholesky.  Xf [pcr_npad(N)][P + 1] = (float)x (zero past N); Hw in the layout of
// k_pcrelate_beta: [wave][n][width], coefficient j = wave * width + q, zero for samples outside the training set and for j > P.
int pcr_design(gpca_handle* h, const char* fn, const double* V, int P, const uint8_t* train, std::vector<float>& Xf, std::vector<double>& Hw,
               std::vector<uint8_t>& tr) {
    const std::string f(fn);
    const int64_t N = h->N;
    const int P1 = P + 1, JW = pcr_beta_width(P);
    tr.assign((size_t)N, 1);
    int64_t T = N;
    if (train) { T = 0; for (int64_t n = 0; n < N; ++n) { tr[(size_t)n] = train[n] ? 1 : 0; T += tr[(size_t)n]; } }
    if (T < (int64_t)P + 2)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": " + std::to_string(T) + " training samples, at least P + 2 = " + std::to_string(P + 2) + " are needed");
    for (int64_t n = 0; n < N; ++n)
        for (int j = 0; j < P; ++j)
            if (!std::isfinite(V[n * P + j]))
                return fail(h, GPCA_ERR_BAD_ARG, f + ": V[" + std::to_string(n) + "][" + std::to_string(j) + "] is not finite");
    std::vector<double> c((size_t)P1, 1.0);
    for (int j = 0; j < P; ++j) {
        double ss = 0.0;
        for (int64_t n = 0; n < N; ++n) if (tr[(size_t)n]) ss += V[n * P + j] * V[n * P + j];
        c[(size_t)j + 1] = std::sqrt(ss / (double)T);
        if (!(c[(size_t)j + 1] > 0.0) || !std::isfinite(c[(size_t)j + 1]))
            return fail(h, GPCA_ERR_BAD_ARG, f + ": column " + std::to_string(j) + " of V is zero on the training samples (or overflows)");
    }
    std::vector<double> X((size_t)N * P1);
    Xf.assign((size_t)pcr_x_capacity(N, P), 0.0f);
    for (int64_t n = 0; n < N; ++n) {
        X[(size_t)n * P1] = 1.0;
        for (int j = 1; j < P1; ++j) X[(size_t)n * P1 + j] = V[n * P + (j - 1)] / c[(size_t)j];
        for (int j = 0; j < P1; ++j) Xf[(size_t)n * P1 + j] = (float)X[(size_t)n * P1 + j];
    }
    // A = X^T X over the training samples; A = L L^T.  The columns have mean square 1, so A's diagonal is T: a pivot that falls to
    // 1e-10 of it means the columns are collinear to working precision.
    std::vector<double> A((size_t)P1 * P1, 0.0);
    for (int64_t n = 0; n < N; ++n) {
        if (!tr[(size_t)n]) continue;
        const double* x = &X[(size_t)n * P1];
        for (int i = 0; i < P1; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * P1 + j] += x[i] * x[j];
    }
    for (int j = 0; j < P1; ++j) {
        double d = A[(size_t)j * P1 + j];
        for (int k = 0; k < j; ++k) d -= A[(size_t)j * P1 + k] * A[(size_t)j * P1 + k];
        if (!(d > 1e-10 * (double)T))
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the design (1, V) is collinear on the training samples (Cholesky pivot " + std::to_string(j) + " failed)");
        const double l = std::sqrt(d);
        A[(size_t)j * P1 + j] = l;
        for (int i = j + 1; i < P1; ++i) {
            double s = A[(size_t)i * P1 + j];
            for (int k = 0; k < j; ++k) s -= A[(size_t)i * P1 + k] * A[(size_t)j * P1 + k];
            A[(size_t)i * P1 + j] = s / l;
        }
    }
    Hw.assign((size_t)pcr_hat_capacity(N, P), 0.0);
    std::vector<double> y((size_t)P1);
    for (int64_t n = 0; n < N; ++n) {
        if (!tr[(size_t)n]) continue;
        const double* x = &X[(size_t)n * P1];
        for (int i = 0; i < P1; ++i) {                       // L y = x
            double s = x[i];
            for (int k = 0; k < i; ++k) s -= A[(size_t)i * P1 + k] * y[(size_t)k];
            y[(size_t)i] = s / A[(size_t)i * P1 + i];
        }
        for (int i = P1 - 1; i >= 0; --i) {                  // L^T h = y
            double s = y[(size_t)i];
            for (int k = i + 1; k < P1; ++k) s -= A[(size_t)k * P1 + i] * y[(size_t)k];
            y[(size_t)i] = s / A[(size_t)i * P1 + i];
        }
        for (int j = 0; j < P1; ++j) Hw[((size_t)(j / JW) * (size_t)N + (size_t)n) * JW + (size_t)(j % JW)] = y[(size_t)j];
    }
    return GPCA_OK;
}

double pcr_common_bytes(int64_t K, int64_t N, int P, bool rm) {
    return 4.0 * (double)pcr_beta_capacity(K, P) * (rm ? 2.0 : 1.0) + 4.0 * (double)pcr_x_capacity(N, P) + 8.0 * (double)pcr_hat_capacity(N, P) + (double)N;
}

// Step 2: uploads the design and runs the regression; a kept row with a value outside {0, 1, 2, missing} is reported here
int pcr_regress(gpca_handle* h, const char* fn, PcrWs& ws, int P, bool rm, const std::vector<float>& Xf, const std::vector<double>& Hw,
                const std::vector<uint8_t>& tr) {
    const int64_t K = h->n_pca, N = h->N;
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    HIPCHK(dalloc(ws.betaG, (size_t)pcr_beta_capacity(K, P)));
    if (rm) HIPCHK(dalloc(ws.beta_rm, (size_t)pcr_beta_capacity(K, P)));
    HIPCHK(dalloc(ws.X, Xf.size())); HIPCHK(dalloc(ws.Hw, Hw.size())); HIPCHK(dalloc(ws.train, (size_t)N)); HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(hipMemcpyAsync(ws.X, Xf.data(), Xf.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.Hw, Hw.data(), Hw.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.train, tr.data(), (size_t)N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    {
        ScopedTimer t(h, "pcrelate_beta", 2.0 * 2.0 * (double)K * (double)N * (double)(P + 1), (double)K * (double)N * (packed ? 0.25 : 1.0));
        launch_pcrelate_beta(st, G, packed, ldr, h->d_pca_rows, K, N, ws.train, ws.Hw, P, ws.betaG, ws.beta_rm, ws.bad);
        HIPCHK(hipGetLastError());
    }
    return asc_check_genotypes(h, fn, ws.bad, st);
}
}  // namespace

extern "C" int gpca_pcrelate_isaf(gpca_handle* h, const double* V, int32_t P, const uint8_t* train, int64_t row0, int64_t row1, float* mu,
                                  float* beta) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const char fn[] = "gpca_pcrelate_isaf";
    CHK(pcr_check(h, fn, V, P));
    const int64_t K = h->n_pca, N = h->N;
    if (!mu && !beta) return fail(h, GPCA_ERR_BAD_ARG, "gpca_pcrelate_isaf: mu and beta are both NULL");
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_pcrelate_isaf: rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    std::vector<float> Xf; std::vector<double> Hw; std::vector<uint8_t> tr;
    CHK(pcr_design(h, fn, V, P, train, Xf, Hw, tr));
    const int64_t rows = row1 - row0;
    if (rows == 0) return GPCA_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, fn, "the band and the regression need", pcr_common_bytes(K, N, P, beta != nullptr) + (mu ? 4.0 * (double)rows * (double)N : 0.0) + (double)(64 << 20)));
    PcrWs ws;
    CHK(pcr_regress(h, fn, ws, P, beta != nullptr, Xf, Hw, tr));
    hipStream_t st = h->st;
    if (mu) {
        HIPCHK(dalloc(ws.mu, (size_t)rows * (size_t)N));
        launch_pcrelate_isaf(st, ws.betaG, ws.X, P, N, row0, row1, ws.mu);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(mu, ws.mu, (size_t)rows * (size_t)N * 4, hipMemcpyDeviceToHost, st));
    }
    if (beta) HIPCHK(hipMemcpyAsync(beta, ws.beta_rm + row0 * (P + 1), (size_t)rows * (size_t)(P + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}

extern "C" int gpca_pcrelate(gpca_handle* h, const double* V, int32_t P, const uint8_t* train, double tau, int64_t row0, int64_t row1,
                             double* kinship, int32_t* nsnp) {
    if (!h) return GPCA_ERR_BAD_ARG;
    if (!kinship) return fail(h, GPCA_ERR_BAD_ARG, "gpca_pcrelate: kinship is required");
    LOCK(h);
    static const char fn[] = "gpca_pcrelate";
    CHK(pcr_check(h, fn, V, P));
    const int64_t K = h->n_pca, N = h->N;
    if (row0 < 0 || row1 <= row0 || row1 > N)
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_pcrelate: rows must satisfy 0 <= row0 < row1 <= N (N = " + std::to_string(N) + ")");
    if (!(tau >= 0.0 && tau < 0.5)) return fail(h, GPCA_ERR_BAD_ARG, "gpca_pcrelate: tau must lie in [0, 0.5)");
    std::vector<float> Xf; std::vector<double> Hw; std::vector<uint8_t> tr;
    CHK(pcr_design(h, fn, V, P, train, Xf, Hw, tr));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    const int64_t E = band_entries(row0, row1, true), ntiles = band_tile_count(row0, row1, kPcrTile);
    if (ntiles >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, "gpca_pcrelate: the band makes 2^31 or more workgroups: ask for fewer rows");
    CHK(preflight_device_memory(h, fn, "the band and the regression need", pcr_common_bytes(K, N, P, false) + (28.0 + (nsnp ? 4.0 : 0.0)) * (double)E + 4.0 * (double)pcr_inv_capacity(N) +
                                 8.0 * (double)ntiles + (double)(64 << 20)));
    PcrWs ws;
    CHK(pcr_regress(h, fn, ws, P, false, Xf, Hw, tr));
    hipStream_t st = h->st;
    std::vector<int2> tiles;
    band_tile_list(row0, row1, kPcrTile, tiles);
    HIPCHK(dalloc(ws.tiles, tiles.size())); HIPCHK(dalloc(ws.inv, (size_t)pcr_inv_capacity(N)));
    HIPCHK(dalloc(ws.R, 2 * (size_t)E)); HIPCHK(dalloc(ws.Q, (size_t)E)); HIPCHK(dalloc(ws.kin, (size_t)E));
    if (nsnp) HIPCHK(dalloc(ws.nsnp, (size_t)E));
    HIPCHK(hipMemcpyAsync(ws.tiles, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.inv, 0, (size_t)pcr_inv_capacity(N) * 4, st));
    HIPCHK(hipMemsetAsync(ws.Q, 0, (size_t)E * 4, st));
    {
        const double pairs = 16384.0 * (double)ntiles;
        ScopedTimer t(h, "pcrelate", 2.0 * 2.0 * (double)(pcr_stages(K) * kPcrStageRows) * pairs, (double)K * (double)N * (packed ? 0.25 : 1.0));
        launch_pcrelate_inv(st, G, packed, ldr, h->d_pca_rows, K, N, ws.betaG, ws.X, P, (float)tau, ws.inv);
        if (launch_pcrelate(st, G, packed, ldr, h->d_pca_rows, K, N, ws.betaG, ws.X, P, (float)tau, ws.tiles, ntiles, row0, row1, ws.R, ws.Q, E) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, "gpca_pcrelate: the launch was refused");
        launch_pcrelate_finish(st, ws.R, ws.Q, ws.inv, K, E, row0, row1, ws.kin, ws.nsnp);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(kinship, ws.kin, (size_t)E * 8, hipMemcpyDeviceToHost, st));
    if (nsnp) HIPCHK(hipMemcpyAsync(nsnp, ws.nsnp, (size_t)E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}
