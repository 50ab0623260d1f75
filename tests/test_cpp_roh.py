"""Both command lines with --gpca-homozyg, on a synthetic .bed of 160 samples and 700 SNPs on two chromosomes (random calls at common
frequencies, which hold no run at a window of 20), with a gap of 3 Mb inside chromosome 1, 0.5 % missing calls on the SNPs that no LD block holds, 20 SNPs that the
call-rate filter drops, and planted homozygous tracts: sample 3 on SNPs 40 .. 169, sample 7 on SNPs 230 .. 330 (across the gap at SNP
280, so two runs), sample 12 on SNPs 380 .. 470 (across the chromosome boundary at SNP 420, so two runs) and sample 20 on 18 SNPs,
which is too short in kb.
The two programs write byte-identical P.hom and P.hom.indiv; the files equal what the io writers produce from the numpy model of
tests/test_gpu_roh.py over the SNPs that pass the SNP QC; the planted tracts are found with the SNP1 / SNP2 the model gives; every
other output file is byte-identical to a run without the flags.  CPU-only: the refusals, alike in both programs."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from test_cpp_assoc_score import BIN, ROOT, gio_qc, host_bin  # noqa: F401  (fixtures)
from test_gpu_roh import model

M, N = 700, 160
CHR2, GAP = 420, 280
NEW = (".hom", ".hom.indiv")
FLAGS = ["--gpca-homozyg-window-snp", "20", "--gpca-homozyg-window-het", "1", "--gpca-homozyg-window-missing", "2", "--gpca-homozyg-snp", "15",
         "--gpca-homozyg-kb", "60", "--gpca-homozyg-density", "50", "--gpca-homozyg-gap", "1000", "--gpca-homozyg-het", "3"]
PARAMS = dict(W=20, H=1, M=2, num=1, den=20, min_snp=15, max_het=3)
TRACTS = {3: (40, 170), 7: (230, 331), 12: (380, 471), 20: (600, 618)}


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("roh")
    rng = np.random.default_rng(9)
    p = rng.uniform(0.25, 0.75, M)[:, None]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    for n, (a, b) in TRACTS.items():
        G[a:b, n] = np.where(rng.random(b - a) < 0.5, 0, 2)
    G[100, 3] = 1                                                     # one het call inside a tract stays inside the run
    out_of_blocks = np.r_[GAP:CHR2, 570:M]                             # (these rows pass the QC, no LD block holds them: the PCA
    G[out_of_blocks] = np.where(rng.random((len(out_of_blocks), N)) < 0.005, -127, G[out_of_blocks])   # takes no missing call on its own SNPs)
    G[400, 12] = -127                                                 # a missing call inside a tract is counted, not a break
    G[500:520][rng.random((20, N)) < 0.1] = -127                      # dropped by the call-rate filter
    chroms = ["1"] * CHR2 + ["2"] * (M - CHR2)
    pos = np.concatenate([1000 + 2000 * np.arange(GAP), 1000 + 2000 * GAP + 3_000_000 + 2000 * np.arange(CHR2 - GAP), 500 + 2000 * np.arange(M - CHR2)])
    pre = str(d / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], chroms, [int(x) for x in pos])
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = d / "ld.txt"
    ld.write_text("1 1 900000\n2 1 300000\n")
    return pre, str(ld), str(d), G


def expected_files(tmp, fs, st, G):
    """the files from the numpy model's records over the SNPs that pass the SNP QC, through the io rules and writers"""
    rows = np.flatnonzero(st["keep"])
    chroms = [fs.chromosomes[r] for r in rows]
    ids = [fs.variant_ids[r] for r in rows]
    pos = np.asarray([int(fs.positions[r]) for r in rows], np.int64)
    brk = gio.roh_breaks(chroms, pos, 1_000_000)
    segs, _ = model(G[rows], brk, PARAMS)
    keep = gio.roh_select(segs, pos, 60_000, 50_000)
    pre = os.path.join(tmp, "want", "P")
    os.makedirs(os.path.dirname(pre))
    gio.write_hom(pre, fs.family_ids, fs.sample_ids, chroms, ids, pos, segs, keep, brk)
    return pre, segs, keep, ids, brk


@pytest.mark.gpu
def test_both_clis_homozyg(tmp_path, host_bin, fileset):
    from genomic_pca_amd import _lib
    from genomic_pca_amd.engine import GpcaEngine
    pre, ld, d, G = fileset
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(gio_qc())
    n_keep = int(st["keep"].sum())
    assert 600 < n_keep < M and not st["keep"][500:520].any()
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0"]
    out = {n: str(tmp_path / n / "P") for n in ("py", "c", "plain")}
    assert main(args + FLAGS + ["--out", out["py"]]) == 0
    for extra, name in ((FLAGS, "c"), ([], "plain")):
        r = subprocess.run([host_bin, *args, *extra, "--out", out[name]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    files = lambda o: sorted(os.listdir(os.path.dirname(o)))
    read = lambda o, s: open(o + s, "rb").read()
    old = files(out["plain"])
    assert len(old) >= 2 and not any(f.endswith(NEW) for f in old)
    want, segs, keep, ids, brk = expected_files(str(tmp_path), fs, st, G)
    # the model finds what was planted: the tract of sample 3 whole (its het call inside), those of 7 and 12 cut at the gap and at the
    # chromosome, that of sample 20 found and dropped by the kb rule
    rows = np.flatnonzero(st["keep"])
    runs = lambda n: [(ids[f], ids[l], int(k)) for (s, f, l, _, _), k in zip(segs, keep) if s == n]
    assert int((brk == 2).sum()) == 1 and int((brk == 3).sum()) == 2 and rows[np.flatnonzero(brk == 2)[0]] == GAP
    for n, cutat in ((3, None), (7, GAP), (12, CHR2)):
        a, b = TRACTS[n]
        got = [r for r in runs(n) if r[2]]
        covered = lambda lo, hi: any(int(r[0][2:]) <= lo + 2 and int(r[1][2:]) >= hi - 3 for r in got)
        if cutat is None:
            assert covered(a, b), (n, got)
        else:
            assert covered(a, cutat) and covered(cutat, b) and not any(int(r[0][2:]) < cutat <= int(r[1][2:]) for r in got), (n, got)
    assert any(k == 0 for _, _, k in runs(20)) and not any(k for _, _, k in runs(20))
    for o in (out["py"], out["c"]):
        assert files(o) == sorted(old + ["P" + s for s in NEW])
        for s in NEW:
            assert read(o, s) == read(want, s) and len(read(o, s)) > 100, (o, s)
        for f in old:
            assert open(os.path.join(os.path.dirname(o), f), "rb").read() == open(os.path.join(os.path.dirname(out["plain"]), f), "rb").read(), (f, o)
    lines = read(out["c"], ".hom").decode().split("\n")
    assert lines[0].split("\t") == ["#FID", "IID", "CHROM", "SNP1", "SNP2", "POS1", "POS2", "KB", "NSNP", "DENSITY", "PHOM", "PHET"]
    assert [ln.split("\t")[1] for ln in lines[1:-1]] == sorted((ln.split("\t")[1] for ln in lines[1:-1]), key=lambda s: int(s[1:]))
    indiv = read(out["c"], ".hom.indiv").decode().split("\n")
    assert len(indiv) == N + 2 and indiv[1 + 3].split("\t")[2] == "1" and indiv[1 + 7].split("\t")[2] == "2" and indiv[1 + 0].split("\t")[2:] == ["0", "0", "NA", "0"]


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
NEEDS_RESIDENT = ("--gpca-homozyg needs the genotype matrix resident on the device: the runs of homozygosity of a matrix walked out of core "
                  "are not implemented")
THRESHOLD = "--gpca-homozyg-window-threshold must be a decimal number in [0, 1] whose exact fraction has a denominator of at most 2^20"
LENGTHS = "--gpca-homozyg-kb, --gpca-homozyg-density and --gpca-homozyg-gap must lie in [0, 1e12]"
WINDOW = "--gpca-homozyg-window-het and --gpca-homozyg-window-missing must lie in [0, --gpca-homozyg-window-snp]"


def test_homozyg_flag_refusals_are_the_same(tmp_path, host_bin):
    E = ["--eigensnp"]
    for flags, msg in ((["--gpca-homozyg"], "--gpca-homozyg needs the --eigensnp workflow"),
                       (["--gpca-homozyg-kb", "500"], "--gpca-homozyg needs the --eigensnp workflow"),
                       (E + ["--gpca-homozyg-window-snp", "0"], "--gpca-homozyg-window-snp must lie in [1, 64]"),
                       (E + ["--gpca-homozyg-window-snp", "65"], "--gpca-homozyg-window-snp must lie in [1, 64]"),
                       (E + ["--gpca-homozyg-window-het", "51"], WINDOW),
                       (E + ["--gpca-homozyg-window-snp", "4", "--gpca-homozyg-window-missing", "5"], WINDOW),
                       (E + ["--gpca-homozyg-window-het", "-1"], WINDOW),
                       (E + ["--gpca-homozyg-window-threshold", "1.01"], THRESHOLD),
                       (E + ["--gpca-homozyg-window-threshold", "0.0000001"], THRESHOLD),
                       (E + ["--gpca-homozyg-window-threshold", "1e-2"], THRESHOLD),
                       (E + ["--gpca-homozyg-window-threshold", "-0.1"], THRESHOLD),
                       (E + ["--gpca-homozyg-window-threshold", "."], THRESHOLD),
                       (E + ["--gpca-homozyg-window-threshold", "9" * 60 + ".5"], THRESHOLD),
                       (E + ["--gpca-homozyg-window-threshold", "0." + "3" * 60], THRESHOLD),
                       (E + ["--gpca-homozyg-snp", "0"], "--gpca-homozyg-snp must lie in [1, 2^31)"),
                       (E + ["--gpca-homozyg-kb", "-1"], LENGTHS),
                       (E + ["--gpca-homozyg-density", "nan"], LENGTHS),
                       (E + ["--gpca-homozyg-gap", "inf"], LENGTHS),
                       (E + ["--gpca-homozyg-het", "-1"], "--gpca-homozyg-het must lie in [0, 2^31)"),
                       (E + ["--gpca-homozyg", "--gpca-stream", "on"], NEEDS_RESIDENT),
                       (E + ["--gpca-homozyg-gap", "500", "--gpca-stream", "on"], NEEDS_RESIDENT)):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert str(ei.value) == "error: " + msg, (flags, str(ei.value))
        assert r.returncode == 2 and r.stderr == "error: " + msg + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset
    for ok in (["--gpca-homozyg"], ["--gpca-homozyg-window-snp", "64", "--gpca-homozyg-window-het", "64"], ["--gpca-homozyg-window-threshold", "1"],
               ["--gpca-homozyg-window-threshold", ".25", "--gpca-homozyg-het", "0", "--gpca-homozyg-kb", "0"],
               ["--gpca-homozyg-window-threshold", "0.00000095367431640625"], ["--gpca-homozyg", "--gpca-het"]):
        with pytest.raises(FileNotFoundError):
            main(BASE + E + ok)
        r = subprocess.run([host_bin, *BASE, *E, *ok], capture_output=True, text=True, timeout=60)
        assert r.returncode != 2 and "t.fam" in r.stderr, (ok, r.stderr)
    helptext = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in helptext for w in ("--gpca-homozyg ", "--gpca-homozyg-window-snp", "--gpca-homozyg-window-het", "--gpca-homozyg-window-missing",
                                       "--gpca-homozyg-window-threshold", "--gpca-homozyg-snp", "--gpca-homozyg-kb", "--gpca-homozyg-density",
                                       "--gpca-homozyg-gap", "--gpca-homozyg-het"))
