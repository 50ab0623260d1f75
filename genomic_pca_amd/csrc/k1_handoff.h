// What a K1 sweep (T = A Q, gpca_rsvd.cpp: stage_AQ) leaves behind for the quantisation of T' in front of K2 (stage_AtT_local): ONE
// record with one reset.  Plain C++ (no HIP type), like eig_result.h: gpca_internal.h includes it for the engine,
// tests/cpp/k1_handoff_audit.cpp includes it under a host compiler and walks every sweep.
//   after a K1 sweep with ...                  state     c = b^T T                                        quantiser of stage_AtT_local
//   scale_out == 0                             None      not formed                                       launch_quantize_f32
//   scale_out, K1 without abs-max (k_gq_i8)    None      launch_sum_partials_f32 per half                 launch_quantize_f32
//   scale_out, abs-max, resident               CFold     launch_post_k1, second stage in the quantiser    launch_quantize_f32_cfold
//   scale_out, abs-max, streamed (unfused)     AbsMax    launch_sum_partials_f32 per half                 launch_quantize_f32_premax
// None also after stage_AtT_local, after stage_power_fused, after anything that rewrites dT or r, and at the entry of rsvd_preflight.
#pragma once
#include <stdint.h>

namespace gpca {

enum class K1State { None, CFold, AbsMax };   // CFold: the digit scale is made (d_tscale / d_tinv), c's second stage waits in the scratch
enum class K1Quantiser { Plain, CFold, PreMax };
enum class K1CSum { NotFormed, SumPartials, PostK1 };

struct K1Handoff {
    K1State state = K1State::None;
    const double* amax[4] = {nullptr, nullptr, nullptr, nullptr};   // AbsMax: the column abs-max partials of each 32-column half, [parts][32]
    int64_t parts = 0;
    void reset() { *this = K1Handoff(); }
    K1Handoff take() { const K1Handoff was = *this; reset(); return was; }      // the consumer reads it and leaves None
};

inline K1State k1_state_after(int scale_out, bool streamed, bool leaves_absmax) {
    return !scale_out || !leaves_absmax ? K1State::None : (streamed ? K1State::AbsMax : K1State::CFold);
}
// The record after a sweep.  AbsMax is a streamed sweep's state only (a resident one folds its partials in launch_post_k1): the panels'
// partials were folded into amax_run ([4][32]) as the sweep went, one part per half.
inline K1Handoff k1_handoff_after(int scale_out, bool streamed, bool leaves_absmax, const double* amax_run) {
    K1Handoff r;
    r.state = k1_state_after(scale_out, streamed, leaves_absmax);
    for (int hf = 0; hf < 4 && r.state == K1State::AbsMax; ++hf) { r.amax[hf] = amax_run + 32 * hf; r.parts = 1; }
    return r;
}
inline K1CSum k1_csum(K1State s, int scale_out) {
    return !scale_out ? K1CSum::NotFormed : (s == K1State::CFold ? K1CSum::PostK1 : K1CSum::SumPartials);
}
inline K1Quantiser k1_quantiser(K1State s) {
    return s == K1State::CFold ? K1Quantiser::CFold : (s == K1State::AbsMax ? K1Quantiser::PreMax : K1Quantiser::Plain);
}

}  // namespace gpca
