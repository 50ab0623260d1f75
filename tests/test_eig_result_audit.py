"""CPU-only: the host's verdict on the result block of the small dense step (genomic_pca_amd/csrc/eig_result.h).

Both device eigen kernels (small_eig.hip) leave two flags behind the singular values, eigenvalues and w of their result block: the
CholeskyQR pivot flag they copy through, and their own cap flag (the Jacobi sweep cap, the QL iteration cap, the QL ring giving up).
finish_small_eigh -- the one host wait of gpca_rsvd, gpca_rsvd_condensed, gpca_refine and the test hook gpca_device_tail -- turns
them into a status with eig_result_verdict; up to this test's pull request it read the first flag only, and a capped eigen step
returned GPCA_OK with half-rotated scores and loadings.

A non-converging eigenproblem cannot be forced on the device honestly (a NaN input ends the Jacobi after one sweep with the cap
clear, small_eig.hip), so the pin is here: tests/cpp/eig_result_audit.cpp includes the header the engine uses and walks hand-made
blocks over every combination of the two flags (pivot flag 0 / j + 1 at the width edges, cap flag 0 / set), every sketch width class
and payloads of zeros, finite values, NaN and Inf around them: pivot set -> GPCA_ERR_NOT_CONVERGED with the pivot's message (also
when the cap is set as well), cap alone -> GPCA_ERR_NOT_CONVERGED "the eigen step hit its sweep cap", neither -> GPCA_OK.

With the verdict finish_small_eigh had before (no look at res[kEigResFlag + 1]) the audit reports
    FAIL pivot 0 cap 1 l 1: status 0 ""
To see it again: in a copy of eig_result.h drop the `else if` branch and build the audit with -I pointing at the copy."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "eig_result_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "eig_result_audit.cpp"), "-o", exe])
    return exe


def test_every_combination_of_the_two_flags(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("eig_result_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) == 2 * 6 * 9 * 3 * 6, last      # every block was judged


def test_the_engine_uses_the_audited_verdict():
    """finish_small_eigh calls the audited function, and nothing else in the engine reads the flags of a product call's result block."""
    src = open(os.path.join(ROOT, "genomic_pca_amd", "csrc", "gpca_rsvd.cpp")).read()
    body = src[src.index("static int finish_small_eigh("):]
    body = body[:body.index("\n}\n")]
    assert "eig_result_verdict(res, h->l)" in body and "fail(h, verdict.status, verdict.msg)" in body
    assert "kEigResFlag" not in body
