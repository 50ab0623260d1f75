// The hand-off from a K1 sweep to the quantisation in front of K2 (genomic_pca_amd/csrc/k1_handoff.h): every combination of
// scale_out {0, 1} x streamed {0, 1} x K1 kernel {2-bit, narrow, DMA, simple int8} against the table of DESIGN.md section 3, written
// out row by row below; what consuming and resetting the record leave; where the streamed sweep's abs-max partials sit.
// Includes the header the engine itself uses in stage_AQ and stage_AtT_local.
#include "k1_handoff.h"

#include <cstdio>

using namespace gpca;

static long long g_checks = 0, g_fail = 0;
#define EXPECT(cond, ...)                                                        \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) { if (++g_fail <= 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } \
    } while (0)

enum Kind { k2bit, kNarrow, kDma, kSimpleI8 };
static const char* const kKindName[] = {"2-bit", "narrow", "DMA", "simple int8"};
struct Row { int scale_out, streamed; Kind kind; K1State state; K1CSum csum; K1Quantiser quantiser; };
static const Row kTable[] = {
    // scale_out == 0: nothing is handed on, c is not formed, a later quantisation is the plain one
    {0, 0, k2bit, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},     {0, 0, kNarrow, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},
    {0, 0, kDma, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},      {0, 0, kSimpleI8, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},
    {0, 1, k2bit, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},     {0, 1, kNarrow, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},
    {0, 1, kDma, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},      {0, 1, kSimpleI8, K1State::None, K1CSum::NotFormed, K1Quantiser::Plain},
    // scale_out, resident: the kernels with the abs-max epilogue hand on the made scale and the pending second stage of c
    {1, 0, k2bit, K1State::CFold, K1CSum::PostK1, K1Quantiser::CFold},       {1, 0, kNarrow, K1State::CFold, K1CSum::PostK1, K1Quantiser::CFold},
    {1, 0, kDma, K1State::CFold, K1CSum::PostK1, K1Quantiser::CFold},        {1, 0, kSimpleI8, K1State::None, K1CSum::SumPartials, K1Quantiser::Plain},
    // scale_out, streamed (unfused): the running abs-max, one part per half
    {1, 1, k2bit, K1State::AbsMax, K1CSum::SumPartials, K1Quantiser::PreMax}, {1, 1, kNarrow, K1State::AbsMax, K1CSum::SumPartials, K1Quantiser::PreMax},
    {1, 1, kDma, K1State::AbsMax, K1CSum::SumPartials, K1Quantiser::PreMax},  {1, 1, kSimpleI8, K1State::None, K1CSum::SumPartials, K1Quantiser::Plain},
};

static bool is_none(const K1Handoff& r) {
    return r.state == K1State::None && r.parts == 0 && !r.amax[0] && !r.amax[1] && !r.amax[2] && !r.amax[3];
}

int main() {
    static double amax_run[128];      // (only its addresses are used)
    int rows = 0;
    unsigned combos = 0;
    for (const Row& w : kTable) {
        ++rows;
        combos |= 1u << (w.scale_out * 8 + w.streamed * 4 + (int)w.kind);
        const bool leaves_absmax = w.kind != kSimpleI8;      // (k_gq_i8 is the one K1 without the abs-max epilogue)
        const char* kind = kKindName[w.kind];
        K1Handoff r = k1_handoff_after(w.scale_out, w.streamed != 0, leaves_absmax, amax_run);
        EXPECT(r.state == w.state && r.state == k1_state_after(w.scale_out, w.streamed != 0, leaves_absmax),
               "scale_out %d streamed %d %s: state %d, the table says %d", w.scale_out, w.streamed, kind, (int)r.state, (int)w.state);
        EXPECT(k1_csum(r.state, w.scale_out) == w.csum, "scale_out %d streamed %d %s: c summed as %d, the table says %d", w.scale_out, w.streamed, kind,
               (int)k1_csum(r.state, w.scale_out), (int)w.csum);
        EXPECT(k1_quantiser(r.state) == w.quantiser, "scale_out %d streamed %d %s: quantiser %d, the table says %d", w.scale_out, w.streamed, kind,
               (int)k1_quantiser(r.state), (int)w.quantiser);
        // where the partials sit: the running abs-max of the streamed sweep (one part, 32 columns per half), nothing in every other state
        if (w.state == K1State::AbsMax) {
            EXPECT(r.parts == 1, "scale_out %d streamed %d %s: %lld parts", w.scale_out, w.streamed, kind, (long long)r.parts);
            for (int hf = 0; hf < 4; ++hf) EXPECT(r.amax[hf] == amax_run + 32 * hf, "scale_out %d streamed %d %s: source of half %d", w.scale_out, w.streamed, kind, hf);
        } else {
            EXPECT(r.parts == 0, "scale_out %d streamed %d %s: %lld parts without an abs-max state", w.scale_out, w.streamed, kind, (long long)r.parts);
            for (int hf = 0; hf < 4; ++hf) EXPECT(r.amax[hf] == nullptr, "scale_out %d streamed %d %s: half %d has a source", w.scale_out, w.streamed, kind, hf);
        }
        // consuming: the consumer gets what was there and leaves none; a second quantisation is the plain one
        const K1Handoff before = r;
        const K1Handoff got = r.take();
        EXPECT(got.state == before.state && got.parts == before.parts && got.amax[0] == before.amax[0] && got.amax[3] == before.amax[3],
               "scale_out %d streamed %d %s: take() returned another record", w.scale_out, w.streamed, kind);
        EXPECT(is_none(r), "scale_out %d streamed %d %s: state %d after take()", w.scale_out, w.streamed, kind, (int)r.state);
        EXPECT(k1_quantiser(r.state) == K1Quantiser::Plain, "scale_out %d streamed %d %s: quantiser %d after take()", w.scale_out, w.streamed, kind, (int)k1_quantiser(r.state));
        // resetting (anything that rewrites dT or r; rsvd_preflight)
        K1Handoff again = before;
        again.reset();
        EXPECT(is_none(again), "scale_out %d streamed %d %s: state %d after reset()", w.scale_out, w.streamed, kind, (int)again.state);
    }
    EXPECT(rows == 2 * 2 * 4 && combos == 0xFFFFu, "%d rows walked, combinations %#x", rows, combos);
    EXPECT(is_none(K1Handoff()), "a fresh record is not none");
    // exactly three states, and every one was reached above
    int seen[3] = {0, 0, 0};
    for (const Row& w : kTable) seen[(int)w.state]++;
    EXPECT(seen[0] == 10 && seen[1] == 3 && seen[2] == 3, "states reached: %d %d %d", seen[0], seen[1], seen[2]);
    printf("k1_handoff_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
