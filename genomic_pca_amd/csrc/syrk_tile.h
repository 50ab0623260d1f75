// The tile helpers of the sample-by-sample products (grm.hip, king.hip, pcrelate.hip) and of the other kernels that decode calls or walk
// a 32 x 32 accumulator (ld.hip, project.hip, assoc_stage.h): the decode of a call from either storage, the 4 rows x 4 samples unit that
// goes to LDS transposed, the kept-row byte mask, and the test and index of the elements of a 32 x 32 sub-tile that lie in a band of the
// lower triangle.  Everything is __device__ __forceinline__: a kernel that uses a helper compiles to what it compiled to with the helper's
// body written out.  (The main loops stay in their kernels: they differ in operand type, stage size and flush rule.)
#pragma once
#include "gemm_i8_common.h"

namespace gpca {

constexpr unsigned kMissingByte = 0x81u;            // the int8 missing code (-127) as a byte

// 4 x 4 byte transpose: x[r] holds bytes (r, 0..3) -> y[k] holds bytes (0..3, k)
__device__ __forceinline__ void tr4x4(const unsigned (&x)[4], unsigned (&y)[4]) {
    const unsigned a = (unsigned)permb((int)x[1], (int)x[0], 0x05010400u), b = (unsigned)permb((int)x[1], (int)x[0], 0x07030602u);
    const unsigned c = (unsigned)permb((int)x[3], (int)x[2], 0x05010400u), d = (unsigned)permb((int)x[3], (int)x[2], 0x07030602u);
    y[0] = (unsigned)permb((int)c, (int)a, 0x05040100u); y[1] = (unsigned)permb((int)c, (int)a, 0x07060302u);
    y[2] = (unsigned)permb((int)d, (int)b, 0x05040100u); y[3] = (unsigned)permb((int)d, (int)b, 0x07060302u);
}
// four 2-bit codes (sample k at bits 2k) -> four int8 calls (code 3 = missing -> -127)
__device__ __forceinline__ unsigned unpack4(unsigned v) {
    unsigned d = (v & 3u) | ((v & 0xcu) << 6) | ((v & 0x30u) << 12) | ((v & 0xc0u) << 18);
    const unsigned m = d & (d >> 1) & 0x01010101u;
    return (d & ~(m * 3u)) | (m * kMissingByte);
}
// the call of (row, sample n) as a byte: 0, 1, 2 or kMissingByte from 2-bit storage, the stored byte from int8 storage
template <bool PACKED>
__device__ __forceinline__ unsigned call_at(const uint8_t* __restrict__ G, int64_t ldr, int64_t row, int64_t n) {
    if (PACKED) {
        const unsigned code = (G[row * ldr + (n >> 2)] >> (2 * (int)(n & 3))) & 3u;
        return code == 3u ? kMissingByte : code;
    }
    return G[row * ldr + n];
}
// nibble k of a kept-row mask as four bytes: byte q = 1 iff bit 4 k + q is set
__device__ __forceinline__ unsigned kept_bytes(unsigned km, int k) { return (((km >> (4 * k)) & 0xfu) * 0x00204081u) & 0x01010101u; }

// A unit = 4 rows x 4 samples of the matrix.  unit_fetch: the four rows' bytes from src (the first row's byte of the unit's first
// sample; 2-bit storage: one byte per row); unit_put: decoded, transposed and stored as four dwords at dst [sample][row], pitch bytes
// per sample.
template <bool PACKED>
__device__ __forceinline__ void unit_fetch(unsigned (&x)[4], const uint8_t* __restrict__ src, int64_t ldr) {
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = PACKED ? (unsigned)src[r * ldr] : *reinterpret_cast<const unsigned*>(src + r * ldr);
}
template <bool PACKED>
__device__ __forceinline__ void unit_put(const unsigned (&f)[4], uint8_t* dst, int pitch) {
    unsigned x[4], y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = PACKED ? unpack4(f[r]) : f[r];
    tr4x4(x, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<unsigned*>(dst + k * pitch) = y[k];
}

// The elements of a 32 x 32 sub-tile that lie in a band: a lane of half h holds (a, b) = (acc_row(a_base, e, h), its column) in
// accumulator element e.  band_holds: (a, b) lies in the rows [row0, row1) of the lower triangle of N samples (DIAG: with its diagonal).
// Its band index is band_index(row0, a, b, DIAG) = band_entries(0, a, DIAG) - band_entries(0, row0, DIAG) + b.
template <bool DIAG>
__device__ __forceinline__ bool band_holds(int64_t row0, int64_t row1, int64_t N, int64_t a, int64_t b) {
    return a >= row0 && a < row1 && a < N && (DIAG ? b <= a : b < a);
}

}  // namespace gpca
