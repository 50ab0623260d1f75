"""The native host program on the LD-pruning path: the flag rules of --gpca-indep-pairwise and formats.hpp's twins of io.ld_windows,
io.ld_bands and io.ld_prune without a GPU; on the GPU, byte-identical P.prune.in / P.prune.out / PCA / loadings files from the two
command lines."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from test_ld_host import BAD_FLAGS, BASE, pack_above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")


@pytest.fixture(scope="module")
def host_bin(gpca):
    gpca.load()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return BIN


@pytest.mark.parametrize("flags,msg", BAD_FLAGS)
def test_flag_errors_cpp(host_bin, flags, msg):
    r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, r.stderr
    assert "--gpca-indep-pairwise" in subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout


def test_cpp_windows_bands_and_prune_match_python(tmp_path):
    """formats.hpp against io.py on random chromosome runs, windows of both kinds, random threshold bits and MAFs with ties"""
    src = tmp_path / "drv.cpp"
    src.write_text(r'''
#include "formats.hpp"
#include <iostream>
int main() {
    std::string window; int64_t K, cap;
    while (std::cin >> window >> K >> cap) {
        std::vector<std::string> chrom((size_t)K); std::vector<int64_t> pos((size_t)K); std::vector<double> maf((size_t)K);
        for (int64_t i = 0; i < K; ++i) std::cin >> chrom[(size_t)i] >> pos[(size_t)i] >> maf[(size_t)i];
        std::vector<int64_t> we;
        try { we = gpca_host::ld_windows(chrom, pos, window); }
        catch (const std::runtime_error& e) { std::cout << "E " << e.what() << "\n"; continue; }
        std::cout << "W"; for (int64_t v : we) std::cout << " " << v; std::cout << "\n";
        std::vector<uint8_t> inset((size_t)K, 1);
        std::cout << "B";
        for (int64_t r0 = 0; r0 < K;) {
            int64_t r1, wm; gpca_host::ld_next_band(we, r0, cap, r1, wm);
            const int64_t words = (wm + 63) / 64;
            std::vector<uint64_t> above((size_t)((r1 - r0) * words));
            for (auto& v : above) std::cin >> v;
            gpca_host::ld_prune_band(we, r0, r1, above, words, maf, inset);
            std::cout << " " << r0 << ":" << r1 << ":" << wm;
            r0 = r1;
        }
        std::cout << "\nI "; for (uint8_t v : inset) std::cout << int(v); std::cout << "\n";
    }
    gpca_host::write_prune_ids(std::string(std::getenv("PRUNE_PREFIX")), {"rs1", "rs2", "rs3"}, {1, 0, 1});
    return 0;
}
''')
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"), str(src), "-lz", "-o", exe])
    rng = np.random.default_rng(5)
    cases, want = [], []
    for trial in range(120):
        sizes = rng.integers(1, 60, int(rng.integers(1, 4)))
        names = ["1", "chr2", "X"][:len(sizes)]
        chrom = np.concatenate([[n] * s for n, s in zip(names, sizes)])
        pos = np.concatenate([np.sort(rng.integers(1, 200_000, s)) for s in sizes])
        K = len(chrom)
        window = str(rng.choice(["2", "5", "50", "3kb", "40kb", "0.5kb", "1000kb"]))
        cap = int(rng.choice([1, 30, 500, 1 << 26]))
        if trial % 20 == 7 and K > 3:
            pos[1], pos[2] = max(pos[1], pos[2]) + 1, min(pos[1], pos[2])          # (only an error when 1 and 2 share a run)
        maf = rng.integers(0, 6, K) / 10.0
        head = f"{window} {K} {cap} " + " ".join(f"{c} {p} {float(m)!r}" for c, p, m in zip(chrom, pos, maf))
        try:
            we = gio.ld_windows(chrom, pos, window)
        except ValueError as e:
            cases.append(head); want += [f"E {e}"]
            continue
        dense = np.triu(rng.random((K, K)) < rng.choice([0.05, 0.4]), 1)
        words, bands = [], []
        for r0, r1, wm in gio.ld_bands(we, cap):
            bits = np.zeros((r1 - r0, (wm + 63) // 64 * 64), np.uint8)
            for i in range(r0, r1):
                n = int(we[i]) - i - 1
                bits[i - r0, :n] = dense[i, i + 1:i + 1 + n]
            ab = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
            words += [str(int(v)) for v in ab.ravel()]
            bands.append(((r0, r1, wm), ab))
        cases.append(head + " " + " ".join(words))
        inset = gio.ld_prune(we, (((r0, r1), ab) for (r0, r1, _), ab in bands), maf)
        assert np.array_equal(inset, gio.ld_prune(we, pack_above(dense, we)[0], maf))
        want += ["W " + " ".join(str(int(v)) for v in we), "B " + " ".join(f"{r0}:{r1}:{wm}" for (r0, r1, wm), _ in bands),
                 "I " + "".join(str(int(v)) for v in inset)]
    env = dict(os.environ, PRUNE_PREFIX=str(tmp_path / "c"))
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, env=env, check=True).stdout.split("\n")
    assert out[:-1] == want and any(w.startswith("E ") for w in want)
    gio.write_prune_ids(str(tmp_path / "p"), ["rs1", "rs2", "rs3"], np.array([True, False, True]))
    for ext in (".prune.in", ".prune.out"):
        assert open(str(tmp_path / "c") + ext, "rb").read() == open(str(tmp_path / "p") + ext, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("window", ["50", "3kb"])
def test_both_clis_indep_pairwise(tmp_path, host_bin, window):
    rng = np.random.default_rng(81)
    M, N = 2400, 300
    p = rng.uniform(0.1, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    for i in range(1, M):
        if i % 12:
            cp = rng.random(N) < 0.85
            G[i, cp] = G[i - 1, cp]
    # missing calls only where the call-rate filter drops the row: the PCA refuses a kept SNP with a missing call (as the reference does)
    G[200:230][rng.random((30, N)) < 0.1] = -127
    chrom = ["1"] * 1300 + ["2"] * 1100
    pos = list(range(1000, 1000 + 1300 * 100, 100)) + list(range(500, 500 + 1100 * 100, 100))
    pre = str(tmp_path / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], chrom, pos)
    ld = tmp_path / "ld.txt"
    ld.write_text("1 1 100000\n1 100501 200000\n2 1 60000\n2 60001 200000\n")
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", str(ld), "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0",
            "--gpca-indep-pairwise", window, "0.2", "--gpca-make-king", "--gpca-save-model"]
    out_py, out_c = str(tmp_path / "py" / "P"), str(tmp_path / "c" / "P")
    assert main(args + ["--out", out_py]) == 0
    r = subprocess.run([host_bin, *args, "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in (".prune.in", ".prune.out", ".eigensnp.pca.tsv", ".eigenvalues.tsv", ".eigensnp.loadings.tsv", ".eigensnp.model.tsv", ".kin0"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    n_in = open(out_py + ".prune.in").read().count("\n")
    n_out = open(out_py + ".prune.out").read().count("\n")
    assert n_in > 100 and n_out > 100
    assert open(out_py + ".eigensnp.loadings.tsv").read().count("\n") == 1 + n_in          # downstream sees the pruned set
    assert "LD pruning" in r.stderr
