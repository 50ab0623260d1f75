"""CPU-only: what a K1 sweep hands to the quantisation in front of K2 (genomic_pca_amd/csrc/k1_handoff.h).

stage_AQ leaves one of three states behind -- nothing; the digit scale made and the second stage of c = b^T T pending (a resident
sweep whose K1 has the abs-max epilogue: launch_post_k1); the running column abs-max of a streamed sweep -- and stage_AtT_local picks
its quantiser from it (launch_quantize_f32, _cfold, _premax) and leaves nothing.  Up to this test's pull request the state was four
loose fields of the handle, set in one function, read in another and cleared by hand in five more, none of which cleared the
pending fold: a call that ended between its K1 and its K2 left it for the next gpca_transform or gpca_refine.  That path cannot be
reached without provoking a failure, so the pin is here: tests/cpp/k1_handoff_audit.cpp includes the header the engine uses and walks
scale_out {0, 1} x streamed {0, 1} x K1 kernel {2-bit, narrow, DMA, simple int8} against the table of DESIGN.md section 3 (state, how
c is summed, quantiser), what take() and reset() leave from every state, and the source and part count of the streamed row.

A mutant: the three states kept and the resident abs-max row sent to the quantiser of the streamed one (in a copy of k1_handoff.h,
k1_quantiser returns K1Quantiser::PreMax for K1State::CFold; build the audit with -I pointing at the copy).  The audit reports
    FAIL scale_out 1 streamed 0 2-bit: quantiser 2, the table says 1
and the same line for the narrow and the DMA kernel: 3 failures."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genomic_pca_amd", "csrc")


def _build(tmp_path):
    exe = str(tmp_path / "k1_handoff_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "k1_handoff_audit.cpp"), "-o", exe])
    return exe


def test_every_sweep_against_the_table(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("k1_handoff_audit:") and " 0 failures" in last, last
    # per combination: state, c, quantiser; part count and four sources; take() (3) and reset(); then the walk, a fresh record, the states
    assert int(last.split()[1]) == 2 * 2 * 4 * (3 + 5 + 3 + 1) + 3, last


def test_the_engine_keeps_one_record_and_one_k1_launcher():
    """The four loose fields are gone from the engine, and every K1 kernel is launched from one place (k1_panel)."""
    for name in sorted(n for n in os.listdir(CSRC) if not n.endswith((".o", ".so"))):      # (sources, not what a build left beside them)
        text = open(os.path.join(CSRC, name), errors="replace").read()
        for word in ("apart_valid", "c_fold_pending", "apart_src", "apart_parts"):
            assert word not in text, (name, word)
    src = open(os.path.join(CSRC, "gpca_rsvd.cpp")).read()
    for call in ("launch_gq_2bit(", "launch_gq_n(", "launch_gq_d(", "launch_gq_i8("):
        assert src.count(call) == 1, (call, src.count(call))
    # ... inside k1_panel, which stage_AQ and stage_power_fused both call; the record is consumed by stage_AtT_local and reset by rsvd_preflight
    body = src[src.index("static int k1_panel("):]
    body = body[:body.index("\n}\n")]
    assert all(call in body for call in ("launch_gq_2bit(", "launch_gq_n(", "launch_gq_d(", "launch_gq_i8("))
    for fn in ("stage_AQ", "stage_power_fused"):
        body = src[src.index("static int %s(" % fn):]
        assert "k1_panel(h, pv, hf," in body[:body.index("\n}\n")], fn
    body = src[src.index("static int stage_AtT_local("):]
    assert "h->k1.take()" in body[:body.index("\n}\n")]
    body = src[src.index("static int rsvd_preflight("):]
    assert re.match(r"[^\n]*\n\s*h->k1\.reset\(\);", body), "rsvd_preflight resets the record before anything can return"
    assert "k1.reset()" in open(os.path.join(CSRC, "gpca_residency.cpp")).read()
