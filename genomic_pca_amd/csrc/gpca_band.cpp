// The host front end that gpca_grm, gpca_king, gpca_pcrelate and their neighbours gpca_project and gpca_ld_window share (declared in
// gpca_internal.h): the exchange with the status word behind the block, the kept-row bit mask, the readback of the kernels'
// invalid-genotype flag.  (The band geometry -- entries, indices, tiles -- is plan_math.h's.)
#include "gpca_internal.h"

using namespace gpca;

int exchange_with_status(gpca_handle* h, const char* fn, double* buf, size_t n, int& lrc, double* tail, size_t ntail) {
    h->status_own = h->err;
    status_histogram(h->h_status, lrc);
    if (hipMemcpyAsync(buf + n - 16, h->h_status, 16 * sizeof(double), hipMemcpyHostToDevice, h->st) != hipSuccess && lrc == GPCA_OK)
        lrc = fail(h, GPCA_ERR_HIP, std::string(fn) + ": status copy failed");
    CHK(allreduce_f64(h, buf, (int64_t)n));
    HIPCHK(hipMemcpyAsync(tail, buf + n - ntail, ntail * sizeof(double), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    const int own_rc = lrc;
    lrc = status_verdict(h, tail + ntail - 16, own_rc, h->status_own, fn);
    if (lrc == GPCA_OK) lrc = own_rc;
    return GPCA_OK;
}

int64_t kept_row_mask(const std::vector<uint8_t>& keep, int64_t Mpad, std::vector<uint32_t>& mask) {
    mask.assign((size_t)(Mpad / 32), 0u);
    int64_t kept = 0;
    for (size_t i = 0; i < keep.size(); ++i)
        if (keep[i]) { set_row_bit(mask, (int64_t)i); ++kept; }
    return kept;
}

int check_genotype_flag(gpca_handle* h, const char* fn, const char* whose, const unsigned* d_bad) {
    unsigned bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    if (bad) return fail(h, GPCA_ERR_INVALID_GENOTYPE, std::string(fn) + ": a " + whose + " row holds a genotype outside {0, 1, 2, missing}");
    return GPCA_OK;
}
