"""Both command lines with --gpca-within, --gpca-freq-strat, --gpca-fst, --gpca-fst-variants and --gpca-assoc-cc-freq, on a synthetic
.bed of three Balding-Nichols populations (F = 0.1; 60 / 100 / 37 samples, 1 000 SNPs, 20 SNPs that the call-rate filter drops and 200
that no LD block holds, with 0.5 % of their calls missing: the PCA itself takes no missing call) with one case / control trait.  The
within file has shuffled rows, a sample with NA, a sample it does not name and a sample the .fam does not have.
The two programs write byte-identical P.frq.strat, P.fst.summary, P.fst.var and P.cad.frq.cc, for Hudson's estimator and for
Weir-Cockerham's; the files equal what the io writers produce from a numpy model's counts over the SNPs that pass the SNP QC (the
LD blocks do not matter), with every labelled sample for the first three and the scan's include set for the last; every other output
file is byte-identical to a run without the new flags.
CPU-only: the refusals, alike in both programs."""
import os
import subprocess

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from test_cpp_assoc_score import BIN, ROOT, gio_qc, host_bin  # noqa: F401  (fixtures)
from test_gpu_group_counts import model

SIZES, F, M = [60, 100, 37], 0.1, 1000
NAMES = ["POP_B", "POP_A", "POP_C"]            # in order of first appearance in the within file
NEW = (".frq.strat", ".fst.summary", ".fst.var", ".cad.frq.cc")


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("strat")
    rng = np.random.default_rng(91)
    N = sum(SIZES)
    pop = np.repeat(np.arange(3), SIZES)
    anc = rng.uniform(0.1, 0.9, M)
    G = np.zeros((M, N), np.int8)
    for p in range(3):
        f = rng.beta(anc * (1 - F) / F, (1 - anc) * (1 - F) / F)[:, None]
        cols = np.flatnonzero(pop == p)
        G[:, cols] = (rng.random((M, len(cols))) < f).astype(np.int8) + (rng.random((M, len(cols))) < f).astype(np.int8)
    out_of_blocks = np.r_[400:500, 900:1000]                          # (the PCA takes no missing call: these rows pass the QC, no LD block holds them)
    G[out_of_blocks] = np.where(rng.random((200, N)) < 0.005, -127, G[out_of_blocks])
    G[300:320][rng.random((20, N)) < 0.1] = -127                      # dropped by the call-rate filter
    pre = str(d / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = d / "ld.txt"
    ld.write_text("1 1 400\n1 501 900\n")
    # the groups: sample 5 has NA, sample 9 is absent, s999 is not in the .fam; POP_B is named first
    label = np.array([{0: 1, 1: 0, 2: 2}[int(p)] for p in pop], np.int32)          # index into NAMES
    label[[5, 9]] = -1
    order = [int(i) for i in rng.permutation(N)]
    for at, i in enumerate((70, 20)):                                                # a POP_B sample first, a POP_A sample next
        order.remove(i); order.insert(at, i)
    with open(d / "within.txt", "w") as f:
        f.write("#FID IID GROUP\n")
        for i in order:
            if i != 9:
                f.write(f"fam{i // 4} s{i} {'NA' if i == 5 else NAMES[label[i]]}\n")
            if i == order[3]:
                f.write("fam999 s999 POP_A\n\n")
    # the trait: the populations differ in prevalence; s3 absent, s11 NA
    cc = (rng.random(N) < np.array([0.3, 0.5, 0.6])[pop]).astype(int)
    with open(d / "cc.pheno", "w") as f:
        f.write("FID IID cad\n")
        f.writelines(f"fam{i // 4} s{i} {'NA' if i == 11 else cc[i] + 1}\n" for i in order if i != 3)
    present = np.ones(N, bool); present[[3, 11]] = False
    return pre, str(ld), str(d), G, label, cc, present


def expected_files(tmp, fs, st, G, label, cc, present, method):
    """the four files from the numpy model's counts, through the io writers"""
    rows = np.flatnonzero(st["keep"])
    meta = ([fs.chromosomes[i] for i in rows], [int(fs.positions[i]) for i in rows], [fs.variant_ids[i] for i in rows])
    a1 = [fs.allele1[i] for i in rows]
    c = model(G[rows], label, 3)
    pre = os.path.join(tmp, "want", "P")
    gio.write_frq_strat(pre + ".frq.strat", *meta, a1, NAMES, c)
    pairs = gio.fst_pairs(3)
    if method == "hudson":
        fst, sums, num, den = gpca.fst_hudson(c, per_variant=True)
        gio.write_fst_var(pre, "hudson", *meta, NAMES, np.stack([num, den], -1))
    else:
        sums, abc = np.zeros((4, 3)), np.zeros((len(rows), 3, 3))
        for q, (j, i) in enumerate(pairs):
            use = np.zeros(3, np.uint8); use[[j, i]] = 1
            abc[:, q] = gpca.fst_wc(c, use, sums=sums[q], per_variant=True)[2]
        gpca.fst_wc(c, None, sums=sums[3])
        gio.write_fst_var(pre, "wc", *meta, NAMES, abc)
    gio.write_fst_summary(pre, method, NAMES, sums)
    lab_cc = np.where(present, cc, -1).astype(np.int32)
    gio.write_frq_strat(pre + ".cad.frq.cc", *meta, a1, ["CTRL", "CASE"], model(G[rows], lab_cc, 2))
    return pre


@pytest.mark.gpu
def test_both_clis_strat(tmp_path, host_bin, fileset):
    from genomic_pca_amd import _lib
    from genomic_pca_amd.engine import GpcaEngine
    pre, ld, d, G, label, cc, present = fileset
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(gio_qc())
    n_keep = int(st["keep"].sum())
    assert 800 < n_keep < M and not st["keep"][300:320].any() and st["keep"][900:].any()
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-pcs", "2", "--gpca-assoc-pheno", os.path.join(d, "cc.pheno"), "--gpca-assoc-logistic"]
    new = ["--gpca-within", os.path.join(d, "within.txt"), "--gpca-freq-strat", "--gpca-fst-variants", "--gpca-assoc-cc-freq", "--gpca-fst"]
    out = {n: str(tmp_path / n / "P") for n in ("py_h", "c_h", "py_w", "c_w", "plain")}
    assert main(args + new + ["hudson", "--out", out["py_h"]]) == 0
    assert main(args + new + ["wc", "--out", out["py_w"]]) == 0
    for extra, name in ((new + ["hudson"], "c_h"), (new + ["wc"], "c_w"), ([], "plain")):
        r = subprocess.run([host_bin, *args, *extra, "--out", out[name]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    files = lambda o: sorted(os.listdir(os.path.dirname(o)))
    old = files(out["plain"])
    assert len(old) >= 4 and not any(f.endswith(NEW) for f in old)
    for method, py, c in (("hudson", out["py_h"], out["c_h"]), ("wc", out["py_w"], out["c_w"])):
        assert files(py) == files(c) == sorted(old + ["P" + s for s in NEW])
        want = expected_files(str(tmp_path / method), fs, st, G, label, cc, present, method)
        for s in NEW:
            a, b, w = (open(p + s, "rb").read() for p in (py, c, want))
            assert a == b, (method, s)
            assert a == w and len(a) > 100, (method, s)
        for f in old:                                         # every other file: what the run without the new flags writes
            w = open(os.path.join(os.path.dirname(out["plain"]), f), "rb").read()
            for o in (py, c):
                assert open(os.path.join(os.path.dirname(o), f), "rb").read() == w, (f, o)
    # the shape of the files, and that the populations are as far apart as they were made
    strat = open(out["c_h"] + ".frq.strat").read().split("\n")
    assert strat[0] == "#CHROM\tPOS\tID\tA1\tGROUP\tOBS_CT\tA1_CT\tA1_FREQ\tHET_CT\tHOM_A1_CT\tHWE_P" and len(strat) == 2 + 3 * n_keep
    assert [ln.split("\t")[4] for ln in strat[1:4]] == NAMES
    summ = [ln.split("\t") for ln in open(out["c_h"] + ".fst.summary").read().split("\n")[1:-1]]
    assert [r[:2] for r in summ] == [["POP_B", "POP_A"], ["POP_B", "POP_C"], ["POP_A", "POP_C"]] and all(int(r[2]) == n_keep for r in summ)
    assert all(0.05 < float(r[3]) < 0.15 for r in summ), summ
    summ = [ln.split("\t") for ln in open(out["c_w"] + ".fst.summary").read().split("\n")[1:-1]]
    assert len(summ) == 4 and summ[3][:2] == ["*", "*"] and all(0.05 < float(r[3]) < 0.15 for r in summ), summ
    assert len(open(out["c_h"] + ".fst.var").read().split("\n")) == 2 + 3 * n_keep
    cc_lines = open(out["c_h"] + ".cad.frq.cc").read().split("\n")
    assert len(cc_lines) == 2 + 2 * n_keep and [ln.split("\t")[4] for ln in cc_lines[1:3]] == ["CTRL", "CASE"]


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def test_strat_flag_refusals_are_the_same(tmp_path, host_bin):
    ph = str(tmp_path / "cc.pheno")
    with open(ph, "w") as f:
        f.write("FID IID cc\n" + "".join(f"f{i} s{i} {1 + i % 2}\n" for i in range(6)))
    good, one, many, bad, twice, missing = (str(tmp_path / n) for n in ("w.txt", "one.txt", "many.txt", "bad.txt", "twice.txt", "nowhere.txt"))
    with open(good, "w") as f:
        f.write("FID IID GROUP\n" + "".join(f"f{i} s{i} G{i % 3}\n" for i in range(9)))
    with open(one, "w") as f:
        f.write("FID IID GROUP\n" + "".join(f"f{i} s{i} G\n" for i in range(9)) + "f9 s9 NA\n")
    with open(many, "w") as f:
        f.write("FID IID GROUP\n" + "".join(f"f{i} s{i} G{i}\n" for i in range(65)))
    with open(bad, "w") as f:
        f.write("FID IID POP\nf0 s0 A\n")
    with open(twice, "w") as f:
        f.write("FID IID GROUP\nf0 s0 A\nf1 s1 B\nf0 s0 B\n")
    E, W = ["--eigensnp"], ["--eigensnp", "--gpca-within", good]
    for flags, msg in ((E + ["--gpca-freq-strat"], "--gpca-freq-strat and --gpca-fst need --gpca-within"),
                       (E + ["--gpca-fst", "hudson"], "--gpca-freq-strat and --gpca-fst need --gpca-within"),
                       (W + ["--gpca-fst-variants", "--gpca-freq-strat"], "--gpca-fst-variants needs --gpca-fst"),
                       (W + ["--gpca-fst", "nei"], "--gpca-fst must be hudson or wc"),
                       (W, "--gpca-within needs --gpca-freq-strat or --gpca-fst"),
                       (["--gpca-within", good, "--gpca-freq-strat"], "--gpca-within needs the --eigensnp workflow"),
                       (E + ["--gpca-assoc-cc-freq"], "--gpca-assoc-cc-freq needs --gpca-assoc-logistic"),
                       (E + ["--gpca-assoc-pheno", ph, "--gpca-assoc-cc-freq"], "--gpca-assoc-cc-freq needs --gpca-assoc-logistic"),
                       (E + ["--gpca-within", many, "--gpca-freq-strat"], "--gpca-within: 65 groups are more than 64"),
                       (E + ["--gpca-within", one, "--gpca-fst", "wc"], "--gpca-fst needs at least two groups, --gpca-within names 1"),
                       (E + ["--gpca-within", bad, "--gpca-freq-strat"], f"--gpca-within: {bad}: the header `FID IID GROUP` is required"),
                       (E + ["--gpca-within", twice, "--gpca-freq-strat"], f"--gpca-within: {twice}:4: sample f0 s0 appears twice"),
                       (E + ["--gpca-within", missing, "--gpca-freq-strat"], f"--gpca-within: cannot open {missing}"),
                       (W + ["--gpca-freq-strat", "--gpca-stream", "on"],
                        "--gpca-within needs the genotype matrix resident on the device: the counts of a matrix walked out of core are not implemented"),
                       (W + ["--gpca-fst", "hudson", "--gpca-stream", "on"],
                        "--gpca-within needs the genotype matrix resident on the device: the counts of a matrix walked out of core are not implemented")):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert str(ei.value) == "error: " + msg, (flags, str(ei.value))
        assert r.returncode == 2 and r.stderr == "error: " + msg + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset
    for ok in (["--gpca-freq-strat"], ["--gpca-fst", "hudson"], ["--gpca-fst", "wc", "--gpca-fst-variants", "--gpca-freq-strat"],
               ["--gpca-within", one, "--gpca-freq-strat"]):
        with pytest.raises(FileNotFoundError):
            main(BASE + W + ok)
    helptext = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in helptext for w in ("--gpca-within", "--gpca-freq-strat", "--gpca-fst ", "--gpca-fst-variants", "--gpca-assoc-cc-freq"))
