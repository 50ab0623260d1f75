"""Both command lines with --gpca-f2, --gpca-fstats and --gpca-fstat-block, on a synthetic .bed of the simulation of tests/_fstat_sim.py
(the tree ((A, B), (C, D)) with X = A / 2 + C / 2; 20 000 SNPs on two chromosomes, 30 samples per population, 2 % of the calls missing
except on the 400 SNPs the one LD block holds: the PCA itself takes no missing call).  The within file has shuffled rows, a sample with
NA, a sample it does not name and a sample the .fam does not have; its groups appear in another order than the simulation's.
The two programs write byte-identical P.f2.summary and P.fstats; the files equal what the io writers produce from the numpy models
(``test_gpu_group_counts.model``, ``test_gpu_f2_blocks.model_f2``) over the SNPs that pass the SNP QC, in blocks of 500 SNPs that end
at the chromosome change.  With --gpca-fst and --gpca-freq-strat beside them one genotype pass serves all: those files equal a run
without the f-statistic flags, and every other file is what a run without any of the flags writes.
CPU-only: the refusals, alike in both programs."""
import os
import subprocess

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from _fstat_sim import POPS, simulate
from test_cpp_assoc_score import BIN, ROOT, host_bin  # noqa: F401  (fixtures)
from test_gpu_f2_blocks import model_f2
from test_gpu_group_counts import model

M, CHR2, CLEAN = 20000, 12000, 400
NAMES = ["C", "X", "A", "D", "B"]              # in order of first appearance in the within file
FSTAT = (".f2.summary", ".fstats")
STRAT = (".frq.strat", ".fst.summary")
LIST = "# the admixture test, the tree and the wrong tree\nf3 X A C\nf4 A B C D\n\nf4 A C B D\nf2 B A\n"


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("fstats")
    G, pop = simulate(77, M=M)
    N = G.shape[1]
    G[:CLEAN][G[:CLEAN] == -127] = 0                                                 # the LD block's SNPs: no missing call
    rng = np.random.default_rng(78)
    pre = str(d / "in")
    chrom = ["1"] * CHR2 + ["2"] * (M - CHR2)
    pos = list(range(1, CHR2 + 1)) + list(range(1, M - CHR2 + 1))
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], chrom, pos)
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = d / "ld.txt"
    ld.write_text(f"1 1 {CLEAN}\n")
    label = np.array([NAMES.index(POPS[int(p)]) for p in pop], np.int32)             # index into NAMES
    label[[5, 9]] = -1                                                               # s5 has NA, s9 is absent
    order = [int(i) for i in rng.permutation(N)]
    for at, i in enumerate((61, 121, 1, 91, 31)):                                    # one sample of C, X, A, D, B first
        order.remove(i); order.insert(at, i)
    assert [POPS[int(pop[i])] for i in order[:5]] == NAMES
    with open(d / "within.txt", "w") as f:
        f.write("#FID IID GROUP\n")
        for i in order:
            if i != 9:
                f.write(f"fam{i // 4} s{i} {'NA' if i == 5 else NAMES[label[i]]}\n")
            if i == order[7]:
                f.write("fam999 s999 A\n\n")
    (d / "list.txt").write_text(LIST)
    return pre, str(ld), str(d), G, label, chrom, pos


def gio_qc():
    from genomic_pca_amd.engine import QcConfig
    return QcConfig(0.9, 0.01, 1.0)


@pytest.mark.gpu
def test_both_clis_fstats(tmp_path, host_bin, fileset):
    from genomic_pca_amd import _lib
    from genomic_pca_amd.engine import GpcaEngine
    pre, ld, d, G, label, chrom, pos = fileset
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(gio_qc())
    rows = np.flatnonzero(st["keep"])
    assert 0.9 * M < len(rows) < M
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0",
            "--eigensnp-min-call-rate", "0.9"]
    within = ["--gpca-within", os.path.join(d, "within.txt")]
    new = ["--gpca-f2", "--gpca-fstats", os.path.join(d, "list.txt"), "--gpca-fstat-block", "500"]
    strat = ["--gpca-freq-strat", "--gpca-fst", "hudson"]
    out = {n: str(tmp_path / n / "P") for n in ("py_f", "c_f", "py_all", "c_all", "c_strat", "plain")}
    assert main(args + within + new + ["--out", out["py_f"]]) == 0
    assert main(args + within + new + strat + ["--out", out["py_all"]]) == 0
    for extra, name in ((within + new, "c_f"), (within + new + strat, "c_all"), (within + strat, "c_strat"), ([], "plain")):
        r = subprocess.run([host_bin, *args, *extra, "--out", out[name]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    files = lambda o: sorted(os.listdir(os.path.dirname(o)))
    old = files(out["plain"])
    assert len(old) >= 3 and not any(f.endswith(FSTAT + STRAT) for f in old)
    assert files(out["py_f"]) == files(out["c_f"]) == sorted(old + ["P" + s for s in FSTAT])
    assert files(out["py_all"]) == files(out["c_all"]) == sorted(old + ["P" + s for s in FSTAT + STRAT])
    # what the numpy models give, through the io writers
    counts = model(G[rows], label, len(NAMES))
    block, B = gio.fstat_blocks([chrom[i] for i in rows], [pos[i] for i in rows], "500")
    n1 = int((rows < CHR2).sum())
    assert B == -(-n1 // 500) + -(-(len(rows) - n1) // 500) and block[n1 - 1] + 1 == block[n1]
    acc, cnt = model_f2(counts, block, B)
    want = str(tmp_path / "want" / "P")
    items = gio.read_fstats_list(os.path.join(d, "list.txt"), NAMES)
    stats = gpca.GpcaEngine.fstat(acc, cnt, [gio.fstat_quad(k, g) for k, g in items])
    gio.write_f2_summary(want, NAMES, gpca.GpcaEngine.fstat(acc, cnt, [(j, i, j, i) for j, i in gio.fst_pairs(len(NAMES))]))
    gio.write_fstats(want, NAMES, items, stats)
    for s in FSTAT:
        w = open(want + s, "rb").read()
        for o in ("py_f", "c_f", "py_all", "c_all"):
            assert open(out[o] + s, "rb").read() == w and len(w) > 100, (o, s)
    for s in STRAT:                                               # one pass serves all: the files of a run without the f-statistic flags
        w = open(out["c_strat"] + s, "rb").read()
        for o in ("py_all", "c_all"):
            assert open(out[o] + s, "rb").read() == w and len(w) > 100, (o, s)
    for f in old:                                                 # every other file: what the run without the new flags writes
        w = open(os.path.join(os.path.dirname(out["plain"]), f), "rb").read()
        for o in ("py_f", "c_f", "py_all", "c_all"):
            assert open(os.path.join(os.path.dirname(out[o]), f), "rb").read() == w, (f, o)
    # the shape of the files, and what they are for
    lines = [ln.split("\t") for ln in open(out["c_f"] + ".fstats").read().split("\n")[:-1]]
    assert lines[0] == "#STAT POP1 POP2 POP3 POP4 EST SE Z N_BLOCKS N_SNPS".split()
    assert [ln[:5] for ln in lines[1:]] == [["f3", "X", "A", "C", "."], ["f4", "A", "B", "C", "D"], ["f4", "A", "C", "B", "D"], ["f2", "B", "A", ".", "."]]
    z = [float(ln[7]) for ln in lines[1:]]
    print("Z of f3(X; A, C), f4(A, B; C, D), f4(A, C; B, D), f2(B, A):", z)
    assert z[0] < -10 and abs(z[1]) < 4 and z[2] > 10 and z[3] > 10 and all(int(ln[8]) == B for ln in lines[1:])
    f2 = [ln.split("\t") for ln in open(out["c_f"] + ".f2.summary").read().split("\n")[:-1]]
    assert f2[0] == "#POP1 POP2 F2 SE Z N_BLOCKS N_SNPS".split() and [ln[:2] for ln in f2[1:]] == [[NAMES[j], NAMES[i]] for j, i in gio.fst_pairs(5)]
    assert all(float(ln[2]) > 0 and int(ln[6]) <= len(rows) for ln in f2[1:])


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def test_fstat_flag_refusals_are_the_same(tmp_path, host_bin):
    good, one, lst, bad_name, bad_arity, missing = (str(tmp_path / n) for n in ("w.txt", "one.txt", "l.txt", "name.txt", "arity.txt", "nowhere.txt"))
    with open(good, "w") as f:
        f.write("FID IID GROUP\n" + "".join(f"f{i} s{i} G{i % 3}\n" for i in range(9)))
    with open(one, "w") as f:
        f.write("FID IID GROUP\n" + "".join(f"f{i} s{i} G\n" for i in range(9)))
    with open(lst, "w") as f:
        f.write("f2 G0 G1\nf3 G2 G0 G1\n")
    with open(bad_name, "w") as f:
        f.write("f2 G0 G1\n# a comment\nf4 G0 G1 G2 G7\n")
    with open(bad_arity, "w") as f:
        f.write("f3 G0 G1\n")
    E, W = ["--eigensnp"], ["--eigensnp", "--gpca-within", good]
    need = "--gpca-f2, --gpca-fstats and --gpca-fstat-block need --gpca-within"
    resident = "--gpca-within needs the genotype matrix resident on the device: the counts of a matrix walked out of core are not implemented"
    for flags, msg in ((E + ["--gpca-f2"], need), (E + ["--gpca-fstats", lst], need), (E + ["--gpca-fstat-block", "500"], need),
                       (W + ["--gpca-fstat-block", "500"], "--gpca-fstat-block needs --gpca-f2 or --gpca-fstats"),
                       (W + ["--gpca-fstat-block", "500", "--gpca-fst", "wc"], "--gpca-fstat-block needs --gpca-f2 or --gpca-fstats"),
                       (W + ["--gpca-f2", "--gpca-fstat-block", "1"], "--gpca-fstat-block: '1' is neither a variant count such as 500 nor a span such as 5000kb"),
                       (W + ["--gpca-f2", "--gpca-fstat-block", "5mb"], "--gpca-fstat-block: '5mb' is neither a variant count such as 500 nor a span such as 5000kb"),
                       (["--gpca-within", good, "--gpca-f2"], "--gpca-within needs the --eigensnp workflow"),
                       (E + ["--gpca-within", one, "--gpca-f2"], "--gpca-f2 and --gpca-fstats need at least two groups, --gpca-within names 1"),
                       (E + ["--gpca-within", one, "--gpca-fstats", lst], "--gpca-f2 and --gpca-fstats need at least two groups, --gpca-within names 1"),
                       (W + ["--gpca-fstats", bad_name], f"--gpca-fstats: {bad_name}:3: no group 'G7' in the within file"),
                       (W + ["--gpca-fstats", bad_arity, "--gpca-f2"], f"--gpca-fstats: {bad_arity}:1: f3 takes 3 groups, 2 are given"),
                       (W + ["--gpca-fstats", missing], f"--gpca-fstats: cannot open {missing}"),
                       (W + ["--gpca-f2", "--gpca-stream", "on"], resident), (W + ["--gpca-fstats", lst, "--gpca-stream", "on"], resident)):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert str(ei.value) == "error: " + msg, (flags, str(ei.value))
        assert r.returncode == 2 and r.stderr == "error: " + msg + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset: the new flags alone satisfy --gpca-within
    for ok in (["--gpca-f2"], ["--gpca-fstats", lst], ["--gpca-f2", "--gpca-fstats", lst, "--gpca-fstat-block", "250kb"],
               ["--gpca-f2", "--gpca-fst", "hudson", "--gpca-freq-strat", "--gpca-fstat-block", "2"]):
        with pytest.raises(FileNotFoundError):
            main(BASE + W + ok)
        r = subprocess.run([host_bin, *BASE, *W, *ok], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--gpca-" not in r.stderr, r.stderr
    helptext = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in helptext for w in ("--gpca-f2 ", "--gpca-fstats", "--gpca-fstat-block"))
