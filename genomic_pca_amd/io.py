"""Host-side file formats either side of the hot path: PLINK BED/BIM/FAM, LD-block
files, a minimal VCF genotype reader, and the TSV writers.  Text parsing stays on the host (tiny); genotype
bytes go to the GPU untouched (2-bit BED payload or int8 dosages) and are decoded / QC'd there.

Reference behaviour restated (file:line):
  * BED: 3-byte magic 6c 1b 01 (SNP-major), ceil(N/4) bytes per SNP, 2 bits per sample LSB-first
    (tests/disk.py:89-135); .bim chrom/sid/bp columns, .fam iid column (prepare.rs:940-970 via bed_reader).
  * LD blocks: prepare.rs:1565-1616 (skip '#', 'chr\\t', 'chromosome\\t' headers; tag 'chr:start-end'; chromosome
    names lower-cased with a leading 'chr' stripped); SNP -> first matching block (prepare.rs:1447-1463).
  * VCF: biallelic single-base REF/ALT only (vcf.rs:109-121); GT 'a/b' or 'a|b' with alleles 0/1, anything else
    drops the variant (vcf.rs:52-63, 153-240); MAF filter default 0.01 (vcf.rs:244-266); id chr:pos:ref:alt.
  * writers: main.rs:696-839 ('{:.6}' fixed formatting, the exact headers and file suffixes).
"""
from __future__ import annotations

import gzip
import math
import os
import re
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

BED_MAGIC = b"\x6c\x1b\x01"


# ------------------------------------------------------------------------------------------------ PLINK
@dataclass
class PlinkFileset:
    bed_rows: np.ndarray          # uint8 [M, ceil(N/4)] (a memory map of the .bed payload)
    n_samples: int
    sample_ids: List[str]         # .fam IID
    variant_ids: List[str]        # .bim sid
    chromosomes: List[str]        # .bim chrom
    positions: np.ndarray         # .bim bp (int64)
    allele1: List[str] = None     # .bim column 5: A1, the allele the dosages count
    allele2: List[str] = None     # .bim column 6: A2
    family_ids: List[str] = None  # .fam FID


def _strip_ext(path: str) -> str:
    for ext in (".bed", ".bim", ".fam"):
        if path.endswith(ext):
            return path[: -len(ext)]
    return path


def read_plink(bed_path: str) -> PlinkFileset:
    prefix = _strip_ext(bed_path)
    iids, fids = [], []
    with open(prefix + ".fam") as f:
        for line in f:
            p = line.split()
            if p:
                iids.append(p[1] if len(p) > 1 else p[0])
                fids.append(p[0])
    sids, chroms, pos, a1, a2 = [], [], [], [], []
    with open(prefix + ".bim") as f:
        for line in f:
            p = line.split()
            if len(p) >= 4:
                chroms.append(p[0]); sids.append(p[1]); pos.append(int(p[3]))
                a1.append(p[4] if len(p) > 4 else "."); a2.append(p[5] if len(p) > 5 else ".")
    n, m = len(iids), len(sids)
    bpr = (n + 3) // 4
    with open(prefix + ".bed", "rb") as f:
        magic = f.read(3)
    if magic != BED_MAGIC:
        raise ValueError(f"{prefix}.bed: not a SNP-major PLINK .bed (magic {magic.hex()})")
    size = os.path.getsize(prefix + ".bed")
    if size != 3 + m * bpr:
        raise ValueError(f"{prefix}.bed: size {size} does not match {m} SNPs x {n} samples")
    rows = np.memmap(prefix + ".bed", dtype=np.uint8, mode="r", offset=3, shape=(m, bpr))
    return PlinkFileset(rows, n, iids, sids, chroms, np.asarray(pos, np.int64), a1, a2, fids)


def write_plink(prefix: str, dosage_count_a1: np.ndarray, sample_ids: Sequence[str], variant_ids: Sequence[str],
                chromosomes: Sequence[str], positions: Sequence[int], alleles: Optional[Sequence[Tuple[str, str]]] = None) -> None:
    """Test/fixture helper: int8 [M, N] count-A1 dosages (-127 missing) -> .bed/.bim/.fam."""
    g = np.asarray(dosage_count_a1, np.int8)
    m, n = g.shape
    code = np.full(g.shape, 1, np.uint8)          # 01 = missing
    code[g == 2] = 0; code[g == 1] = 2; code[g == 0] = 3
    pad = (-n) % 4
    if pad:
        code = np.concatenate([code, np.zeros((m, pad), np.uint8)], axis=1)
    c4 = code.reshape(m, -1, 4)
    rows = (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)
    with open(prefix + ".bed", "wb") as f:
        f.write(BED_MAGIC); f.write(rows.tobytes())
    with open(prefix + ".bim", "w") as f:
        for i, (c, s, p) in enumerate(zip(chromosomes, variant_ids, positions)):
            x1, x2 = alleles[i] if alleles is not None else ("A", "G")
            f.write(f"{c}\t{s}\t0\t{p}\t{x1}\t{x2}\n")
    with open(prefix + ".fam", "w") as f:
        for s in sample_ids:
            f.write(f"{s}\t{s}\t0\t0\t0\t-9\n")


# ------------------------------------------------------------------------------------------------ LD blocks
def normalize_chromosome_name(name: str) -> str:
    """prepare.rs:1610-1616."""
    name = name.lower()
    while name.startswith("chr"):
        name = name[3:]
    return name


def parse_ld_block_file(path: str) -> List[Tuple[str, int, int, str]]:
    """prepare.rs:1565-1607 -> [(chrom, start, end, tag)]."""
    blocks = []
    with open(path) as f:
        for line in f:
            t = line.strip()
            if not t or t.startswith("#") or t.startswith("chr\t") or t.startswith("chromosome\t"):
                continue
            p = t.split()
            if len(p) < 3:
                continue
            c = normalize_chromosome_name(p[0])
            start, end = int(p[1]), int(p[2])
            blocks.append((c, start, end, f"{c}:{start}-{end}"))
    return blocks


def map_snps_to_ld_blocks(blocks, chromosomes: Sequence[str], positions: Sequence[int], qc_keep: np.ndarray):
    """prepare.rs:1424-1563.  Returns (keep mask restricted to SNPs inside some block, [(tag, original_rows)] sorted
    by tag).  Each kept SNP goes to the FIRST block (file order) that contains it."""
    qc_keep = np.asarray(qc_keep).astype(bool)
    pos = np.asarray(positions, np.int64)
    norm = np.array([normalize_chromosome_name(c) for c in chromosomes])
    assigned = np.full(len(pos), -1, np.int64)
    for bi, (c, start, end, _) in enumerate(blocks):
        hit = qc_keep & (assigned < 0) & (norm == c) & (pos >= start) & (pos <= end)
        assigned[hit] = bi
    keep = assigned >= 0
    by_tag = {}
    for bi, (_, _, _, tag) in enumerate(blocks):
        rows = np.nonzero(assigned == bi)[0]
        if len(rows):
            by_tag.setdefault(tag, []).extend(rows.tolist())
    return keep.astype(np.uint8), sorted(((t, sorted(r)) for t, r in by_tag.items()), key=lambda x: x[0])


def read_sample_keep_file(path: str) -> List[str]:
    with open(path) as f:
        return [ln.split()[0] for ln in f if ln.strip()]


# ------------------------------------------------------------------------------------------------ VCF
def _gt_to_dosage(gt: str) -> Optional[int]:
    """vcf.rs:52-63: exactly 3 bytes, separator / or |, alleles 0/1."""
    if len(gt) != 3 or gt[1] not in "/|":
        return None
    a, b = gt[0], gt[2]
    if a not in "01" or b not in "01":
        return None
    return (a == "1") + (b == "1")


def _dosages_gt_first(rest: bytes, ns: int) -> Optional[np.ndarray]:
    """All sample columns of one record at once when GT is the first FORMAT key (the layout of 1000 Genomes-style files):
    every sample field must start with a 3-byte genotype `a/b` or `a|b`, a, b in {0, 1}, followed by ':' or the column end
    (vcf.rs:52-63).  Returns int8 dosages, or None if any sample breaks the rule (the variant is dropped, as in the reference)."""
    a = np.frombuffer(rest, np.uint8)
    if len(rest) == 4 * ns - 1:                                   # FORMAT = GT only: fixed 4-byte stride
        b = np.frombuffer(rest + b"\t", np.uint8).reshape(ns, 4)
        c0, sep, c1, end = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        if not (end == 9).all():
            return None
    else:
        tabs = np.flatnonzero(a == 9)
        if len(tabs) != ns - 1:
            return None
        starts = np.concatenate(([0], tabs + 1))
        ends = np.concatenate((tabs, [len(a)]))
        if ((ends - starts) < 3).any():
            return None
        c0, sep, c1 = a[starts], a[starts + 1], a[starts + 2]
        long_ = (ends - starts) > 3
        if long_.any() and not (a[starts[long_] + 3] == 58).all():   # a 3-byte GT must be followed by ':'
            return None
    if not (((c0 == 48) | (c0 == 49)).all() and ((c1 == 48) | (c1 == 49)).all() and ((sep == 47) | (sep == 124)).all()):
        return None
    return ((c0 - 48) + (c1 - 48)).astype(np.int8)


def read_vcf(path: str, maf_threshold: float = 0.01):
    """Returns (sample_names, variant_ids, int8 [variants, samples]) following vcf.rs:65-286.  Records are parsed as bytes;
    when GT leads the FORMAT column the whole sample row is converted with a handful of numpy operations (a chr22-scale file of
    2 504 samples parses at text-I/O speed instead of one Python call per genotype); any other FORMAT order takes the
    per-sample path."""
    opener = gzip.open if path.endswith(".gz") else open
    samples: List[str] = []
    ids: List[str] = []
    rows: List[np.ndarray] = []
    with opener(path, "rb") as f:
        for line in f:
            if line.startswith(b"##"):
                continue
            line = line.rstrip(b"\r\n")
            if line.startswith(b"#CHROM"):
                samples = [x.decode() for x in line.split(b"\t")[9:]]
                if not samples:
                    raise ValueError(f"VCF header from {path} contains no samples.")      # vcf.rs:31-36
                continue
            p = line.split(b"\t", 9)
            if len(p) < 10:
                continue
            chrom, pos, ref, alt, fmt_col, rest = p[0], p[1], p[3], p[4], p[8], p[9]
            if len(ref) != 1 or len(alt) != 1 or b"," in alt:                              # vcf.rs:109-121
                continue
            fmt = fmt_col.split(b":")
            if b"GT" not in fmt:
                continue
            gi = fmt.index(b"GT")
            ns = len(samples)
            if gi == 0:
                d = _dosages_gt_first(rest, ns)
            else:                                                                          # GT not first: per-sample path
                d = np.empty(ns, np.int8)
                fields = rest.split(b"\t")
                ok = len(fields) == ns
                if ok:
                    for si, field in enumerate(fields):
                        parts = field.split(b":")
                        v = _gt_to_dosage(parts[gi].decode()) if gi < len(parts) else None
                        if v is None:                                                      # any bad GT drops the variant
                            ok = False
                            break
                        d[si] = v
                if not ok:
                    d = None
            if d is None:
                continue
            af = float(d.sum(dtype=np.int64)) / (2 * ns)
            if min(af, 1.0 - af) < maf_threshold:                                          # vcf.rs:244-266
                continue
            ids.append(f"{chrom.decode()}:{pos.decode()}:{ref.decode()}:{alt.decode()}")
            rows.append(d)
    G = np.stack(rows) if rows else np.zeros((0, len(samples)), np.int8)
    return samples, ids, G


# ------------------------------------------------------------------------------------------------ writers
def _fmt6(x) -> str:
    return f"{float(x):.6f}"


def write_principal_components(prefix: str, suffix: str, sample_names: Sequence[str], pcs: np.ndarray) -> str:
    """main.rs:696-762: header SampleID\\tPC1..; '{:.6}'.  suffix = 'vcf.pca.tsv' or 'eigensnp.pca.tsv'."""
    path = f"{prefix}.{suffix}"
    if pcs.shape[1] == 0:
        return path
    with open(path, "w") as f:
        f.write("SampleID" + "".join(f"\tPC{i}" for i in range(1, pcs.shape[1] + 1)) + "\n")
        for i, name in enumerate(sample_names):
            if i < pcs.shape[0]:
                f.write(name + "".join("\t" + _fmt6(v) for v in pcs[i]) + "\n")
            else:
                f.write(name + "\tNA" * pcs.shape[1] + "\n")
    return path


def write_eigenvalues(prefix: str, eigenvalues: Sequence[float]) -> str:
    """main.rs:765-784: header written even when empty."""
    path = f"{prefix}.eigenvalues.tsv"
    with open(path, "w") as f:
        f.write("PC\tEigenvalue\n")
        for i, v in enumerate(eigenvalues):
            f.write(f"{i + 1}\t{_fmt6(v)}\n")
    return path


def write_loadings(prefix: str, variant_ids: Sequence[str], chromosomes: Sequence[str], positions: Sequence[int],
                   loadings: np.ndarray) -> str:
    """main.rs:787-839."""
    path = f"{prefix}.eigensnp.loadings.tsv"
    if loadings.shape[1] == 0:
        return path
    if not (len(variant_ids) == len(chromosomes) == len(positions) == loadings.shape[0]) and len(variant_ids):
        raise ValueError("Mismatch in lengths of variant metadata and loadings matrix rows.")     # main.rs:817-824
    with open(path, "w") as f:
        f.write("VariantID\tChrom\tPos" + "".join(f"\tPC{i}_loading" for i in range(1, loadings.shape[1] + 1)) + "\n")
        for i in range(len(variant_ids)):
            f.write(f"{variant_ids[i]}\t{chromosomes[i]}\t{positions[i]}" + "".join("\t" + _fmt6(v) for v in loadings[i]) + "\n")
    return path


# ------------------------------------------------------------------------------------------------ projection model
# P.eigensnp.model.tsv: what a projection of other samples onto fitted PCs needs (gpca_project): per PCA SNP its id, position,
# alleles (A1 = the counted allele), the f32 mean / s.d. of the standardisation and the f32 loadings, each written with %.9g so that
# it reads back to the same f32; the eigenvalues (%.17g) and the fitting sample count ride in the header lines.
MODEL_MAGIC = "#gpca-model v1"


@dataclass
class ProjectionModel:
    variant_ids: List[str]
    chromosomes: List[str]
    positions: List[int]
    allele1: List[str]
    allele2: List[str]
    mean: np.ndarray              # f32 [S]
    sd: np.ndarray                # f32 [S]
    loadings: np.ndarray          # f32 [S][k]
    eigenvalues: np.ndarray       # f64 [k]
    n_samples: int                # samples the model was fitted on

    @property
    def k(self) -> int:
        return self.loadings.shape[1]


def _g9(x) -> str:
    return "%.9g" % float(np.float32(x))


def write_model(prefix: str, model: ProjectionModel) -> str:
    path = f"{prefix}.eigensnp.model.tsv"
    k = model.k
    with open(path, "w") as f:
        f.write(f"{MODEL_MAGIC}\tk={k}\tfit_samples={int(model.n_samples)}\n")
        f.write("#eigenvalues" + "".join("\t%.17g" % float(v) for v in model.eigenvalues) + "\n")
        f.write("VariantID\tChrom\tPos\tA1\tA2\tMean\tSD" + "".join(f"\tPC{i}_loading" for i in range(1, k + 1)) + "\n")
        for i in range(len(model.variant_ids)):
            f.write(f"{model.variant_ids[i]}\t{model.chromosomes[i]}\t{int(model.positions[i])}\t{model.allele1[i]}\t{model.allele2[i]}\t"
                    f"{_g9(model.mean[i])}\t{_g9(model.sd[i])}" + "".join("\t" + _g9(v) for v in model.loadings[i]) + "\n")
    return path


def read_model(path: str) -> ProjectionModel:
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        if not head or head[0] != MODEL_MAGIC:
            raise ValueError(f"{path}: not a projection model (first line must start with '{MODEL_MAGIC}')")
        kv = dict(t.split("=", 1) for t in head[1:] if "=" in t)
        try:
            k, n_fit = int(kv["k"]), int(kv["fit_samples"])
        except (KeyError, ValueError):
            raise ValueError(f"{path}: the first line must carry k=<int> and fit_samples=<int>")
        ev_line = f.readline().rstrip("\n").split("\t")
        if not ev_line or ev_line[0] != "#eigenvalues":
            raise ValueError(f"{path}: second line must be '#eigenvalues ...'")
        ev = np.array([float(v) for v in ev_line[1:]], np.float64)
        cols = f.readline().rstrip("\n").split("\t")
        if cols[:7] != ["VariantID", "Chrom", "Pos", "A1", "A2", "Mean", "SD"] or len(cols) != 7 + k:
            raise ValueError(f"{path}: bad header line (VariantID Chrom Pos A1 A2 Mean SD and {k} loading columns expected)")
        ids, chroms, pos, a1, a2, rows = [], [], [], [], [], []
        for ln, line in enumerate(f, start=4):
            p = line.rstrip("\n").split("\t")
            if p == [""]:
                continue
            if len(p) != 7 + k:
                raise ValueError(f"{path}:{ln}: {len(p)} columns, {7 + k} expected")
            ids.append(p[0]); chroms.append(p[1]); pos.append(int(p[2])); a1.append(p[3]); a2.append(p[4])
            rows.append([float(v) for v in p[5:]])
    vals = np.array(rows, np.float64).reshape(len(rows), 2 + k).astype(np.float32)
    return ProjectionModel(ids, chroms, pos, a1, a2, vals[:, 0].copy(), vals[:, 1].copy(), np.ascontiguousarray(vals[:, 2:]), ev, n_fit)


@dataclass
class Alignment:
    mean: np.ndarray              # f32 [M_target]: the model's mean on the target's counted allele (2 - mean where flipped)
    sd: np.ndarray                # f32 [M_target]
    loadings: np.ndarray          # f32 [M_target][k]: zero rows = target variants outside the model
    matched: int                  # model SNPs used (same or swapped alleles)
    flipped: int                  # ... of them with A1 / A2 swapped
    allele_mismatch: int          # model SNPs whose ID matched but whose allele pair differs: dropped
    absent: int                   # model SNPs with no target variant of that ID


def align_model(model: ProjectionModel, variant_ids: Sequence[str], allele1: Sequence[str], allele2: Sequence[str]) -> Alignment:
    """The model's rows per target row, matched by variant ID ('.' never matches; the first target row of a duplicated ID is the
    one used).  Same (A1, A2): as is; swapped: mean -> 2 - mean, loadings -> -loadings; any other pair: dropped."""
    M = len(variant_ids)
    first = {}
    for i, v in enumerate(variant_ids):
        if v != "." and v not in first:
            first[v] = i
    mean = np.zeros(M, np.float32); sd = np.ones(M, np.float32)
    W = np.zeros((M, model.k), np.float32)
    matched = flipped = mismatch = absent = 0
    seen = set()
    for s, v in enumerate(model.variant_ids):
        i = first.get(v) if v != "." else None
        if i is None or i in seen:
            absent += 1
            continue
        if (allele1[i], allele2[i]) == (model.allele1[s], model.allele2[s]):
            mean[i], sd[i], W[i] = model.mean[s], model.sd[s], model.loadings[s]
        elif (allele1[i], allele2[i]) == (model.allele2[s], model.allele1[s]):
            mean[i], sd[i], W[i] = np.float32(2.0) - model.mean[s], model.sd[s], -model.loadings[s]
            flipped += 1
        else:
            mismatch += 1
            continue
        seen.add(i)
        matched += 1
    return Alignment(mean, sd, W, matched, flipped, mismatch, absent)


def write_projected(prefix: str, sample_names: Sequence[str], scores: np.ndarray, used: Sequence[int]) -> str:
    """Q.projected.pca.tsv: SampleID, PC1..PCk ('{:.6}' as the other PC files), SNPsUsed (model SNPs with an observed call)."""
    path = f"{prefix}.projected.pca.tsv"
    with open(path, "w") as f:
        f.write("SampleID" + "".join(f"\tPC{i}" for i in range(1, scores.shape[1] + 1)) + "\tSNPsUsed\n")
        for i, name in enumerate(sample_names):
            f.write(name + "".join("\t" + _fmt6(v) for v in scores[i]) + f"\t{int(used[i])}\n")
    return path


def write_grm(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], bands) -> Tuple[str, str, str]:
    """GCTA's binary GRM layout: P.grm.bin (f32 little-endian, lower triangle with the diagonal, packed row-major), P.grm.N.bin (f32,
    the number of SNPs behind each entry) and P.grm.id (FID<TAB>IID per sample).  bands: (grm, npairs) pairs of consecutive row bands
    in row order, each packed the same way (gpca_grm's output), written as they come: the whole matrix is never held."""
    n = len(sample_ids)
    if len(family_ids) != n:
        raise ValueError("write_grm: one family ID per sample")
    paths = (f"{prefix}.grm.bin", f"{prefix}.grm.N.bin", f"{prefix}.grm.id")
    total = 0
    with open(paths[0], "wb") as fg, open(paths[1], "wb") as fn:
        for g, npairs in bands:
            g = np.asarray(g).ravel()
            npairs = np.asarray(npairs).ravel()
            if g.shape != npairs.shape:
                raise ValueError("write_grm: a band's grm and npairs differ in length")
            fg.write(g.astype("<f4").tobytes())
            fn.write(npairs.astype("<f4").tobytes())
            total += g.size
    if total != n * (n + 1) // 2:
        raise ValueError(f"write_grm: the bands hold {total} entries, {n} samples need {n * (n + 1) // 2}")
    with open(paths[2], "w") as f:
        for fid, iid in zip(family_ids, sample_ids):
            f.write(f"{fid}\t{iid}\n")
    return paths


# ------------------------------------------------------------------------------------------------ KING-robust kinship
KIN0_HEADER = "#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP\n"


def king_bands(n: int, max_pairs: int = 1 << 26):
    """Consecutive row bands [row0, row1) of an n-sample STRICTLY lower triangle (row j holds j pairs), each of at most max_pairs
    pairs (at least one row): the bands gpca_king is asked for, one at a time."""
    r0 = 0
    while r0 < n:
        r1 = r0 + 1
        while r1 < n and (r1 + 1) * r1 // 2 - r0 * (r0 - 1) // 2 <= max_pairs:
            r1 += 1
        yield r0, r1
        r0 = r1


def band_pairs(row0: int, row1: int) -> Tuple[np.ndarray, np.ndarray]:
    """(j, k) sample indices of the pairs of a band, in gpca_king's order: j = row0 .. row1 - 1, k = 0 .. j - 1 (k < j)."""
    js = np.arange(row0, row1, dtype=np.int64)
    j = np.repeat(js, js)
    starts = np.repeat(np.cumsum(js) - js, js)
    k = np.arange(j.size, dtype=np.int64) - starts
    return j, k


def _fmt_kin(v: float) -> str:
    return "nan" if v != v else f"{v:.6f}"


def write_kin0(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], bands, min_kinship: Optional[float] = None) -> str:
    """P.kin0: one tab-separated line per pair, `FID1 IID1 FID2 IID2 NSNP HETHET IBS0 KINSHIP`, ID1 the earlier sample in .fam order,
    the kinship as %.6f (or nan).  bands: ((row0, row1), kinship, counts) in row order (gpca_king's output, counts [pairs][3]), written
    as they come: the whole matrix is never held.  min_kinship: only pairs with kinship >= it (NaN never passes)."""
    n = len(sample_ids)
    if len(family_ids) != n:
        raise ValueError("write_kin0: one family ID per sample")
    path = f"{prefix}.kin0"
    nxt = 0
    with open(path, "w") as f:
        f.write(KIN0_HEADER)
        for (r0, r1), kin, cnt in bands:
            if r0 != nxt:
                raise ValueError(f"write_kin0: band [{r0}, {r1}) does not follow row {nxt}")
            nxt = r1
            kin = np.asarray(kin, np.float64).ravel()
            cnt = np.asarray(cnt).reshape(-1, 3)
            j, k = band_pairs(r0, r1)
            if kin.size != j.size or cnt.shape[0] != j.size:
                raise ValueError(f"write_kin0: band [{r0}, {r1}) needs {j.size} pairs")
            sel = np.flatnonzero(kin >= min_kinship) if min_kinship is not None else range(j.size)
            f.writelines(f"{family_ids[k[i]]}\t{sample_ids[k[i]]}\t{family_ids[j[i]]}\t{sample_ids[j[i]]}\t{cnt[i, 0]}\t{cnt[i, 1]}\t"
                         f"{cnt[i, 2]}\t{_fmt_kin(kin[i])}\n" for i in sel)
    if nxt != n and n > 0:
        raise ValueError(f"write_kin0: the bands end at row {nxt}, {n} samples need {n}")
    return path


def king_unrelated(n: int, pairs) -> np.ndarray:
    """The greedy pruning rule of --gpca-king-cutoff: pairs = (i, j) sample indices of the related pairs (kinship above the cutoff; NaN
    never counts).  While any pair remains, the sample with the most remaining partners leaves, ties going to the later sample in .fam
    order.  Returns the in-set as a bool mask [n] (True = kept for the fit)."""
    adj = [set() for _ in range(n)]
    for i, j in pairs:
        i, j = int(i), int(j)
        if i == j or not (0 <= i < n and 0 <= j < n):
            raise ValueError(f"king_unrelated: bad pair ({i}, {j}) for {n} samples")
        adj[i].add(j); adj[j].add(i)
    deg = np.array([len(a) for a in adj], np.int64)
    keep = np.ones(n, bool)
    while n and deg.max() > 0:
        top = int(deg.max())
        s = int(np.flatnonzero(deg == top)[-1])                  # the later sample of the tie
        keep[s] = False
        for t in adj[s]:
            adj[t].discard(s); deg[t] -= 1
        adj[s].clear(); deg[s] = 0
    return keep


def write_king_cutoff_ids(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], keep: np.ndarray) -> Tuple[str, str]:
    """P.king.cutoff.in.id and P.king.cutoff.out.id: `#FID<TAB>IID`, then one line per sample in .fam order."""
    paths = (f"{prefix}.king.cutoff.in.id", f"{prefix}.king.cutoff.out.id")
    for path, want in zip(paths, (True, False)):
        with open(path, "w") as f:
            f.write("#FID\tIID\n")
            f.writelines(f"{family_ids[i]}\t{sample_ids[i]}\n" for i in range(len(sample_ids)) if bool(keep[i]) == want)
    return paths


# ------------------------------------------------------------------------------------------------ PC-Relate kinship
PCRELATE_KIN_HEADER = "#FID1\tIID1\tFID2\tIID2\tNSNP\tKINSHIP\n"
PCRELATE_INBREED_HEADER = "#FID\tIID\tNSNP\tF\n"


def pcrelate_bands(n: int, max_pairs: int = 1 << 26):
    """Consecutive row bands [row0, row1) of an n-sample lower triangle WITH its diagonal (row a holds a + 1 entries), each of at most
    max_pairs entries (at least one row): the bands gpca_pcrelate is asked for, one at a time."""
    r0 = 0
    while r0 < n:
        r1 = r0 + 1
        while r1 < n and (r1 + 1) * (r1 + 2) // 2 - r0 * (r0 + 1) // 2 <= max_pairs:
            r1 += 1
        yield r0, r1
        r0 = r1


def write_pcrelate(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], bands, min_kinship: Optional[float] = None) -> Tuple[str, str]:
    """P.pcrelate.kin: one tab-separated line per strictly lower pair, `FID1 IID1 FID2 IID2 NSNP KINSHIP`, ID1 the earlier sample in .fam
    order, the kinship as %.6f (or nan); P.pcrelate.inbreed: `FID IID NSNP F` per sample, F = 2 self-kinship - 1 from the diagonal.
    bands: ((row0, row1), kinship, nsnp) in row order (gpca_pcrelate's output: the lower triangle with its diagonal), written as they
    come.  min_kinship (the table filter): only pairs with kinship >= it (NaN never passes); the inbreeding file is not filtered."""
    n = len(sample_ids)
    if len(family_ids) != n:
        raise ValueError("write_pcrelate: one family ID per sample")
    paths = (f"{prefix}.pcrelate.kin", f"{prefix}.pcrelate.inbreed")
    nxt = 0
    with open(paths[0], "w") as f, open(paths[1], "w") as fi:
        f.write(PCRELATE_KIN_HEADER)
        fi.write(PCRELATE_INBREED_HEADER)
        for (r0, r1), kin, cnt in bands:
            if r0 != nxt:
                raise ValueError(f"write_pcrelate: band [{r0}, {r1}) does not follow row {nxt}")
            nxt = r1
            kin = np.asarray(kin, np.float64).ravel()
            cnt = np.asarray(cnt).ravel()
            need = r1 * (r1 + 1) // 2 - r0 * (r0 + 1) // 2
            if kin.size != need or cnt.size != need:
                raise ValueError(f"write_pcrelate: band [{r0}, {r1}) needs {need} entries")
            o = 0
            for a in range(r0, r1):
                row_k, row_c = kin[o:o + a], cnt[o:o + a]
                sel = np.flatnonzero(row_k >= min_kinship) if min_kinship is not None else range(a)
                f.writelines(f"{family_ids[b]}\t{sample_ids[b]}\t{family_ids[a]}\t{sample_ids[a]}\t{row_c[b]}\t{_fmt_kin(row_k[b])}\n" for b in sel)
                fi.write(f"{family_ids[a]}\t{sample_ids[a]}\t{cnt[o + a]}\t{_fmt_kin(2.0 * kin[o + a] - 1.0)}\n")
                o += a + 1
    if nxt != n and n > 0:
        raise ValueError(f"write_pcrelate: the bands end at row {nxt}, {n} samples need {n}")
    return paths


# ------------------------------------------------------------------------------------------------ windowed LD and LD pruning
def parse_ld_window(text: str) -> Tuple[str, int]:
    """The WINDOW of --gpca-indep-pairwise: "50" -> ("variants", 50): each SNP against the next 49 kept SNPs of its chromosome run
    (plink's window of 50 variants, step 1); "250kb" -> ("bp", 250000): later kept SNPs of the run at most 250 000 bp further on."""
    t = str(text).strip().lower()
    kb = t.endswith("kb")
    num = t[:-2].strip() if kb else t
    try:
        v = float(num) if kb else int(num)
    except ValueError:
        raise ValueError(f"bad LD window '{text}': expected a variant count such as 50 or a span such as 250kb") from None
    if kb:
        if not (v > 0 and np.isfinite(v)):
            raise ValueError(f"bad LD window '{text}': the span must be positive")
        return "bp", int(round(v * 1000))
    if v < 2:
        raise ValueError(f"bad LD window '{text}': a window in variants holds at least 2")
    return "variants", v


def ld_windows(chromosomes: Sequence[str], positions: Sequence[int], window: str) -> np.ndarray:
    """win_end [K] (int64) over the kept SNPs, in their order, for gpca_ld_window: SNP i is paired with the later SNPs j < win_end[i]
    of its chromosome run.  A chromosome that reappears after another, or positions that decrease inside a run, is an error that
    names the variant (by its index among the SNPs given)."""
    kind, w = parse_ld_window(window)
    K = len(chromosomes)
    pos = np.asarray(positions, np.int64)
    if pos.shape != (K,):
        raise ValueError("ld_windows: one position per chromosome entry")
    win_end = np.empty(K, np.int64)
    seen = set()
    s = 0
    while s < K:
        c = normalize_chromosome_name(chromosomes[s])
        if c in seen:
            raise ValueError(f"ld_windows: chromosome '{chromosomes[s]}' reappears at variant {s} after another chromosome: sort the variants")
        seen.add(c)
        e = s + 1
        while e < K and normalize_chromosome_name(chromosomes[e]) == c:
            if pos[e] < pos[e - 1]:
                raise ValueError(f"ld_windows: the position of variant {e} ({int(pos[e])}) is below that of the variant before it on chromosome "
                                 f"'{chromosomes[e]}': sort the variants")
            e += 1
        idx = np.arange(s, e, dtype=np.int64)
        if kind == "variants":
            win_end[s:e] = np.minimum(idx + w, e)
        else:
            win_end[s:e] = np.maximum(s + np.searchsorted(pos[s:e], pos[s:e] + w, side="right"), idx + 1)
        s = e
    return win_end


def ld_bands(win_end: np.ndarray, max_slots: int = 1 << 26):
    """Consecutive row bands (row0, row1, wmax) over the rows of win_end with (row1 - row0) * wmax <= max_slots (at least one row),
    wmax = the widest window of the band (at least 1): the bands gpca_ld_window is asked for, so that a kb window over a dense region
    stays bounded."""
    we = np.asarray(win_end, np.int64)
    K = we.size
    width = we - np.arange(K, dtype=np.int64) - 1
    r0 = 0
    while r0 < K:
        r1, wm = r0 + 1, max(int(width[r0]), 1)
        while r1 < K:
            w2 = max(wm, int(width[r1]))
            if (r1 + 1 - r0) * w2 > max_slots:
                break
            wm, r1 = w2, r1 + 1
        yield r0, r1, wm
        r0 = r1


def ld_prune(win_end: np.ndarray, above_bands, maf: np.ndarray) -> np.ndarray:
    """The pruning rule of --gpca-indep-pairwise.  above_bands: ((row0, row1), above) in row order, above [rows][words] uint64 as
    gpca_ld_window writes it (or one such array for all rows).  Walk i ascending; skip i if it is out; J = the in-window j still in with
    above(i, j), ascending; j* = the first of them with maf[j] > maf[i]; every member of J before j* (all of J if there is none) goes
    out; if j* exists, i goes out.  So of a pair above the threshold the SNP with the smaller MAF leaves, ties the later one, and once i
    has left its window is not looked at further.  Returns the in-set as a bool mask [K]."""
    we = np.asarray(win_end, np.int64)
    maf = np.asarray(maf, np.float64)
    K = we.size
    if maf.shape != (K,):
        raise ValueError("ld_prune: one MAF per row of win_end")
    if isinstance(above_bands, np.ndarray):
        above_bands = [((0, K), above_bands)]
    inset = np.ones(K, bool)
    nxt = 0
    for (r0, r1), above in above_bands:
        if r0 != nxt:
            raise ValueError(f"ld_prune: band [{r0}, {r1}) does not follow row {nxt}")
        nxt = r1
        above = np.ascontiguousarray(above, np.uint64).reshape(r1 - r0, -1) if r1 > r0 else np.zeros((0, 1), np.uint64)
        hot = np.flatnonzero(above.any(axis=1))
        for t in hot:
            i = r0 + int(t)
            if not inset[i]:
                continue
            bits = np.unpackbits(above[t].view(np.uint8), bitorder="little")[: max(int(we[i]) - i - 1, 0)]
            for d in np.flatnonzero(bits):
                j = i + 1 + int(d)
                if not inset[j]:
                    continue
                if maf[j] > maf[i]:
                    inset[i] = False
                    break
                inset[j] = False
    if nxt != K:
        raise ValueError(f"ld_prune: the bands end at row {nxt}, {K} rows need {K}")
    return inset


def maf_from_qc_detail(n_valid, n_het, n_hom2) -> np.ndarray:
    """maf = min(p, 1 - p), p = (n_het + 2 n_hom2) / (2 n_valid) in f64 (0 where nothing is observed)"""
    nv = np.asarray(n_valid, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = (np.asarray(n_het, np.float64) + 2.0 * np.asarray(n_hom2, np.float64)) / (2.0 * nv)
    p = np.where(nv > 0, p, 0.0)
    return np.minimum(p, 1.0 - p)


def write_prune_ids(prefix: str, variant_ids: Sequence[str], inset: np.ndarray) -> Tuple[str, str]:
    """P.prune.in and P.prune.out: one variant ID per line, in the order given (.bim order)."""
    if len(variant_ids) != len(inset):
        raise ValueError("write_prune_ids: one in-set flag per variant ID")
    paths = (f"{prefix}.prune.in", f"{prefix}.prune.out")
    for path, want in zip(paths, (True, False)):
        with open(path, "w") as f:
            f.writelines(f"{variant_ids[i]}\n" for i in range(len(variant_ids)) if bool(inset[i]) == want)
    return paths


# ------------------------------------------------------------------------------------------------ association scan
@dataclass
class PhenoTable:
    family_ids: List[str]
    sample_ids: List[str]
    names: List[str]              # the trait (or covariate) columns, in file order
    values: np.ndarray            # f64 [rows][len(names)], NaN = missing


def read_pheno(path: str) -> PhenoTable:
    """A whitespace-separated phenotype or covariate table.  The header `FID IID name...` (a leading '#' allowed) is required; `NA` and
    `nan` in any letter case mean missing; a repeated (FID, IID) is refused."""
    fids, iids, rows, names, seen = [], [], [], None, set()
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if names is None:
                if len(p) < 3 or p[0].lstrip("#").upper() != "FID" or p[1].upper() != "IID":
                    raise ValueError(f"{path}: the header `FID IID name...` with at least one column is required")
                names = p[2:]
                if len(set(names)) != len(names):
                    raise ValueError(f"{path}: a column name is repeated")
                continue
            if len(p) != 2 + len(names):
                raise ValueError(f"{path}:{ln}: {len(p)} fields, the header has {2 + len(names)}")
            if (p[0], p[1]) in seen:
                raise ValueError(f"{path}:{ln}: sample {p[0]} {p[1]} appears twice")
            seen.add((p[0], p[1]))
            vals = []
            for v in p[2:]:
                if v.lower() in ("na", "nan"):
                    vals.append(np.nan)
                else:
                    try:
                        if "_" in v:
                            raise ValueError
                        vals.append(float(v))
                    except ValueError:
                        raise ValueError(f"{path}:{ln}: `{v}` is not a number") from None
            fids.append(p[0]); iids.append(p[1]); rows.append(vals)
    if names is None:
        raise ValueError(f"{path}: the header `FID IID name...` with at least one column is required")
    return PhenoTable(fids, iids, names, np.asarray(rows, np.float64).reshape(len(rows), len(names)))


def align_pheno(table: PhenoTable, family_ids: Sequence[str], sample_ids: Sequence[str]) -> np.ndarray:
    """The table's rows in .fam order, matched by (FID, IID): f64 [len(sample_ids)][columns]; a sample absent from the table is missing
    (NaN) in every column; rows of the table that name no sample of the .fam are ignored."""
    at = {(f, i): r for r, (f, i) in enumerate(zip(table.family_ids, table.sample_ids))}
    out = np.full((len(sample_ids), len(table.names)), np.nan)
    for n, key in enumerate(zip(family_ids, sample_ids)):
        r = at.get(key)
        if r is not None:
            out[n] = table.values[r]
    return out


def assoc_bands(K: int, L: int, max_values: int = 1 << 26):
    """[row0, row1) bands of the K kept rows whose xb workspace (rows x L doubles) holds at most max_values entries (at least one row):
    the bands gpca_assoc_linear is asked for, one at a time."""
    step = max(max_values // max(L, 1), 1)
    return [(r0, min(r0 + step, K)) for r0 in range(0, K, step)]


def _g6(x) -> str:
    x = float(x)
    return "NA" if x != x else "%.6g" % x


def write_assoc(prefix: str, trait: str, chromosomes: Sequence[str], positions: Sequence[int], variant_ids: Sequence[str],
                allele1: Sequence[str], n_obs, a1_freq, beta, se, t, log10p, append: bool = False) -> str:
    """P.<trait>.assoc.linear: one tab-separated line per SNP, `#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE T_STAT LOG10P`; numbers as %.6g,
    NaN as NA, OBS_CT as an integer.  append=True adds the rows of a further band to the file (no header)."""
    path = f"{prefix}.{trait}.assoc.linear"
    n = len(variant_ids)
    for a in (chromosomes, positions, allele1, n_obs, a1_freq, beta, se, t, log10p):
        if len(a) != n:
            raise ValueError("write_assoc: one entry per SNP in every column")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "a" if append else "w") as f:
        if not append:
            f.write("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P\n")
        f.writelines(f"{chromosomes[i]}\t{int(positions[i])}\t{variant_ids[i]}\t{allele1[i]}\t{int(n_obs[i])}\t{_g6(a1_freq[i])}\t{_g6(beta[i])}\t"
                     f"{_g6(se[i])}\t{_g6(t[i])}\t{_g6(log10p[i])}\n" for i in range(n))
    return path


# ---- many-trait QTL scan (gpca_assoc_qtl, gpca_qtl_stats, gpca_qtl_t_min; include/gpca.h section a24): twins in host/formats.hpp ------------
QTL_HITS_PER_PAIRS = 4096         # assoc_qtl_bands: the record buffer holds one pair in this many of a band
QTL_BAND_WORK_MAX = 1 << 47       # assoc_qtl_bands: rows x N x T of one call (a few seconds of the matrix cores)


def assoc_qtl_bands(K: int, T: int, N: int, cap: int):
    """[row0, row1) bands of the K kept rows for gpca_assoc_qtl with a record buffer of cap hits: whole blocks of 128 rows (at least
    one block) such that cap holds one pair in QTL_HITS_PER_PAIRS of the band's rows x T pairs (a threshold scan keeps far fewer; a band
    that finds more is asked for again with a buffer of n_found; every band repeats the call's host step on all T traits, so bands are
    made long) and rows x N x T stays within QTL_BAND_WORK_MAX."""
    K, T, N, cap = int(K), max(int(T), 1), max(int(N), 1), max(int(cap), 1)
    step = min(cap * QTL_HITS_PER_PAIRS // T, QTL_BAND_WORK_MAX // (N * T))
    step = max(step // 128 * 128, 128)
    return [(r0, min(r0 + step, K)) for r0 in range(0, K, step)]


def write_qtl_hits(prefix: str, chromosomes: Sequence[str], positions: Sequence[int], variant_ids: Sequence[str], allele1: Sequence[str],
                   traits: Sequence[str], n_obs, a1_freq, beta, se, t, log10p, append: bool = False) -> str:
    """P.qtl.hits: one tab-separated line per hit in the order given (the scan's: ascending (row, trait)), `#CHROM POS ID A1 TRAIT OBS_CT
    A1_FREQ BETA SE T_STAT LOG10P`; every column holds one entry per hit (the SNP's columns repeated per hit); numbers as %.6g, NaN as
    NA, OBS_CT as an integer.  append=True adds the hits of a further band (no header)."""
    path = f"{prefix}.qtl.hits"
    n = len(traits)
    for a in (chromosomes, positions, variant_ids, allele1, n_obs, a1_freq, beta, se, t, log10p):
        if len(a) != n:
            raise ValueError("write_qtl_hits: one entry per hit in every column")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "a" if append else "w") as f:
        if not append:
            f.write("#CHROM\tPOS\tID\tA1\tTRAIT\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P\n")
        f.writelines(f"{chromosomes[i]}\t{int(positions[i])}\t{variant_ids[i]}\t{allele1[i]}\t{traits[i]}\t{int(n_obs[i])}\t{_g6(a1_freq[i])}\t"
                     f"{_g6(beta[i])}\t{_g6(se[i])}\t{_g6(t[i])}\t{_g6(log10p[i])}\n" for i in range(n))
    return path


def qtl_best_merge(best_r2, best_row, band_r2, band_row):
    """The running best over bands in ascending row order, in place: a band's (r2, row) replaces a trait's entry when the trait has
    none yet (row < 0) or the band's r2 is strictly larger, so a tie stays with the lower row.  Returns (best_r2, best_row)."""
    b2, bw = np.asarray(band_r2, np.float64), np.asarray(band_row, np.int64)
    with np.errstate(invalid="ignore"):
        take = (bw >= 0) & ((best_row < 0) | (b2 > best_r2))
    best_r2[take] = b2[take]
    best_row[take] = bw[take]
    return best_r2, best_row


def write_qtl_best(prefix: str, traits: Sequence[str], chromosomes: Sequence[str], positions: Sequence[int], variant_ids: Sequence[str],
                   allele1: Sequence[str], beta, se, t, log10p, n_tests) -> str:
    """P.qtl.best: one tab-separated line per trait, `#TRAIT CHROM POS ID A1 BETA SE T_STAT LOG10P N_TESTS`: the SNP with the largest r2
    for the trait over all bands (the lower row on a tie) and the number of live SNPs it was chosen from; a trait without a live SNP
    has NA in the SNP's columns (an entry of variant_ids that is None); numbers as %.6g, NaN as NA."""
    path = f"{prefix}.qtl.best"
    n = len(traits)
    for a in (chromosomes, positions, variant_ids, allele1, beta, se, t, log10p, n_tests):
        if len(a) != n:
            raise ValueError("write_qtl_best: one entry per trait in every column")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write("#TRAIT\tCHROM\tPOS\tID\tA1\tBETA\tSE\tT_STAT\tLOG10P\tN_TESTS\n")
        for i in range(n):
            if variant_ids[i] is None:
                f.write(f"{traits[i]}\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\t{int(n_tests[i])}\n")
            else:
                f.write(f"{traits[i]}\t{chromosomes[i]}\t{int(positions[i])}\t{variant_ids[i]}\t{allele1[i]}\t{_g6(beta[i])}\t{_g6(se[i])}\t"
                        f"{_g6(t[i])}\t{_g6(log10p[i])}\t{int(n_tests[i])}\n")
    return path


# ---- cis-QTL mapping (gpca_assoc_qtl_cis, gpca_qtl_beta_approx; include/gpca.h section a25) ------------------------------------------------
QTL_CIS_RESULT_BYTES_MAX = 256 << 20      # assoc_qtl_cis_bands: perm_r2 [G][P] f64 of one call


def qtl_cis_windows(chromosomes: Sequence[str], positions: Sequence[int], trait_chrom: Sequence[str], trait_pos: Sequence[int],
                    window_bp: int) -> np.ndarray:
    """win [G][2] (int64) for gpca_assoc_qtl_cis: [lo, hi) over the kept SNPs given (in their order) with |pos - trait_pos| <= window_bp
    on the trait's chromosome; lo = hi where none qualifies, [0, 0) for a chromosome the SNPs do not have.  The SNPs are ordered as
    ld_windows requires, and refused in its words."""
    K = len(chromosomes)
    pos = np.asarray(positions, np.int64)
    if pos.shape != (K,):
        raise ValueError("qtl_cis_windows: one position per chromosome entry")
    if len(trait_chrom) != len(trait_pos):
        raise ValueError("qtl_cis_windows: one position per trait chromosome")
    runs = {}
    s = 0
    while s < K:
        c = normalize_chromosome_name(chromosomes[s])
        if c in runs:
            raise ValueError(f"qtl_cis_windows: chromosome '{chromosomes[s]}' reappears at variant {s} after another chromosome: sort the variants")
        e = s + 1
        while e < K and normalize_chromosome_name(chromosomes[e]) == c:
            if pos[e] < pos[e - 1]:
                raise ValueError(f"qtl_cis_windows: the position of variant {e} ({int(pos[e])}) is below that of the variant before it on chromosome "
                                 f"'{chromosomes[e]}': sort the variants")
            e += 1
        runs[c] = (s, e)
        s = e
    w = int(window_bp)
    win = np.zeros((len(trait_chrom), 2), np.int64)
    for g, (tc, tp) in enumerate(zip(trait_chrom, trait_pos)):
        run = runs.get(normalize_chromosome_name(tc))
        if run is None:
            continue
        s, e = run
        win[g, 0] = s + int(np.searchsorted(pos[s:e], int(tp) - w, side="left"))
        win[g, 1] = s + int(np.searchsorted(pos[s:e], int(tp) + w, side="right"))
    return win


def read_trait_pos(path: str) -> dict:
    """A `TRAIT CHROM POS` table (that header; whitespace-separated): {trait: (chrom, pos)}.  A later line of a trait replaces an
    earlier one."""
    out = {}
    with open(path) as f:
        head = f.readline().split()
        if head != ["TRAIT", "CHROM", "POS"]:
            raise ValueError(f"{path}: the header must be 'TRAIT CHROM POS'")
        for ln, line in enumerate(f, 2):
            t = line.split()
            if not t:
                continue
            if len(t) != 3:
                raise ValueError(f"{path}: line {ln} does not hold TRAIT CHROM POS")
            digits = t[2][1:] if t[2][:1] in ("+", "-") else t[2]
            if not (digits.isascii() and digits.isdigit() and len(t[2]) <= 18):
                raise ValueError(f"{path}: line {ln}: the position '{t[2]}' is not an integer")
            out[t[0]] = (t[1], int(t[2]))
    return out


def assoc_qtl_cis_bands(G: int, P: int):
    """[g0, g1) bands of the G traits for gpca_assoc_qtl_cis such that perm_r2 [g1 - g0][P] (f64) stays within QTL_CIS_RESULT_BYTES_MAX
    (at least one trait per band; one band when P = 0)."""
    G, P = int(G), int(P)
    step = max(QTL_CIS_RESULT_BYTES_MAX // (8 * P), 1) if P > 0 else max(G, 1)
    return [(g0, min(g0 + step, G)) for g0 in range(0, G, step)]


def write_qtl_cis(prefix: str, traits: Sequence[str], trait_pos, res: dict, ids: Sequence[str], var_pos: Sequence[int],
                  a1: Sequence[str]) -> str:
    """P.qtl.cis: one tab-separated line per trait in the order given, `#TRAIT CHROM POS N_VAR ID VAR_POS A1 BETA SE T_STAT LOG10P_NOMINAL
    TRUE_DF SHAPE1 SHAPE2 PVAL_PERM LOG10P_BETA`.  trait_pos [G]: (chrom, pos) or None; res: assoc_qtl_cis's dict over the same traits
    (bands concatenated); ids, var_pos, a1: per kept row.  The SNP is the window's best row; BETA, SE, T_STAT by qtl_stats, LOG10P_NOMINAL
    at df = n - Pc - 2, the last five by qtl_beta_approx (NA without permutations).  A trait without a position is a row of NA; a
    trait with N_VAR = 0 has NA from ID on.  Numbers as %.6g, NaN as NA."""
    from .engine import GpcaEngine
    path = f"{prefix}.qtl.cis"
    G = len(traits)
    if len(trait_pos) != G or any(len(res[k]) != G for k in ("n_var", "best_row", "best_r2", "best_stat", "perm_r2")):
        raise ValueError("write_qtl_cis: one entry per trait in every column")
    df = float(res["df"])
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write("#TRAIT\tCHROM\tPOS\tN_VAR\tID\tVAR_POS\tA1\tBETA\tSE\tT_STAT\tLOG10P_NOMINAL\tTRUE_DF\tSHAPE1\tSHAPE2\tPVAL_PERM\tLOG10P_BETA\n")
        for g in range(G):
            if trait_pos[g] is None:
                f.write(traits[g] + "\tNA" * 15 + "\n")
                continue
            chrom, tp = trait_pos[g]
            nv = int(res["n_var"][g])
            if nv == 0:
                f.write(f"{traits[g]}\t{chrom}\t{int(tp)}\t0" + "\tNA" * 12 + "\n")
                continue
            row = int(res["best_row"][g])
            xb, sxx, yy = (float(v) for v in res["best_stat"][g])
            beta, se, t = GpcaEngine.qtl_stats(xb, sxx, yy, df)[0]
            l10 = GpcaEngine.student_t_log10p(t, df) if not np.isnan(t) else float("nan")
            pr = np.asarray(res["perm_r2"][g], np.float64)
            if pr.size:
                ba = GpcaEngine.qtl_beta_approx(pr, float(res["best_r2"][g]), df)
                tail = [ba["true_df"], ba["shape1"], ba["shape2"], ba["pval_perm"], ba["log10p_beta"]]
            else:
                tail = [float("nan")] * 5
            f.write(f"{traits[g]}\t{chrom}\t{int(tp)}\t{nv}\t{ids[row]}\t{int(var_pos[row])}\t{a1[row]}\t{_g6(beta)}\t{_g6(se)}\t{_g6(t)}\t"
                    f"{_g6(l10)}\t" + "\t".join(_g6(v) for v in tail) + "\n")
    return path


# ---- LD scores and LD-score regression (gpca_ld_score, gpca_ld_score_total, gpca_ldsc_fit; include/gpca.h section a19) -----------
def ld_score_sum(K: int, bands):
    """(acc int64 [K], partners int64 [K]) = the bands of GpcaEngine.ld_score added up.  bands: ((row0, row1), score[, partners]) over
    the bands of ld_bands, in any order; score (and partners) hold the band's span from row0, which reaches past row1 into the rows of
    the next bands.  partners stays 0 where no band gives one."""
    K = int(K)
    acc = np.zeros(K, np.int64)
    part = np.zeros(K, np.int64)
    for band in bands:
        (r0, r1), score = band[0], np.asarray(band[1])
        r0 = int(r0)
        if score.ndim != 1 or score.dtype.kind not in "iu" or r0 < 0 or r0 + score.size > K:
            raise ValueError(f"ld_score_sum: the band ({r0}, {int(r1)}) holds {score.size} sums from row {r0}, {K} rows are there")
        acc[r0:r0 + score.size] += score.astype(np.int64)
        if len(band) > 2 and band[2] is not None:
            pv = np.asarray(band[2])
            if pv.shape != score.shape:
                raise ValueError("ld_score_sum: partners and score of a band have one length")
            part[r0:r0 + pv.size] += pv.astype(np.int64)
    return acc, part


def write_ldscore(prefix: str, chromosomes: Sequence[str], ids: Sequence[str], positions: Sequence[int], l2, maf) -> List[str]:
    """P.l2.ldscore: tab-separated, header `CHR SNP BP L2`, one line per SNP, L2 as %.6g (ldsc's column layout); P.l2.M: the number of
    SNPs summed over; P.l2.M_5_50: those with MAF > 0.05."""
    n = len(ids)
    for a in (chromosomes, positions, l2, maf):
        if len(a) != n:
            raise ValueError("write_ldscore: one entry per SNP in every column")
    d = os.path.dirname(prefix)
    if d:
        os.makedirs(d, exist_ok=True)
    paths = [f"{prefix}.l2.ldscore", f"{prefix}.l2.M", f"{prefix}.l2.M_5_50"]
    with open(paths[0], "w") as f:
        f.write("CHR\tSNP\tBP\tL2\n")
        f.writelines(f"{chromosomes[i]}\t{ids[i]}\t{int(positions[i])}\t{_g6(l2[i])}\n" for i in range(n))
    with open(paths[1], "w") as f:
        f.write(f"{n}\n")
    with open(paths[2], "w") as f:
        f.write(f"{int(np.count_nonzero(np.asarray(maf, np.float64) > 0.05))}\n")
    return paths


LDSC_SUMMARY_HEADER = "#TRAIT\tTEST\tN\tM_USED\tMEAN_CHI2\tLAMBDA_GC\tINTERCEPT\tINTERCEPT_SE\tH2\tH2_SE\tRATIO\tRATIO_SE\n"


def write_ldsc_summary(prefix: str, rows) -> str:
    """P.ldsc.summary: one tab-separated line per trait, `#TRAIT TEST N M_USED MEAN_CHI2 LAMBDA_GC INTERCEPT INTERCEPT_SE H2 H2_SE RATIO
    RATIO_SE`.  rows: (trait, test, n, fit) with test = LINEAR or LOGISTIC, n = the samples of the scan and fit = the dict of
    GpcaEngine.ldsc_fit, or None where the regression was refused (its numbers are NA then).  N and M_USED are integers, the others
    %.6g, NaN as NA."""
    path = f"{prefix}.ldsc.summary"
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    keys = ("mean_chi2", "lambda_gc", "intercept", "intercept_se", "h2", "h2_se", "ratio", "ratio_se")
    with open(path, "w") as f:
        f.write(LDSC_SUMMARY_HEADER)
        for trait, test, n, fit in rows:
            if test not in ("LINEAR", "LOGISTIC"):
                raise ValueError(f"write_ldsc_summary: TEST is LINEAR or LOGISTIC, not '{test}'")
            if fit is None:
                f.write(f"{trait}\t{test}\t{int(n)}\tNA" + "\tNA" * len(keys) + "\n")
            else:
                f.write(f"{trait}\t{test}\t{int(n)}\t{int(fit['m_used'])}\t" + "\t".join(_g6(fit[k]) for k in keys) + "\n")
    return path


def binary_trait(values):
    """None, or the 0 / 1 recoding (1 = case, NaN stays NaN) of a trait column that is binary: its present (non-NaN) values are exactly
    {0, 1} (1 = case) or exactly {1, 2} (plink's coding, 2 = case).  A column with one class only is not binary."""
    v = np.asarray(values, np.float64).reshape(-1)
    present = set(np.unique(v[~np.isnan(v)]).tolist())
    if present == {0.0, 1.0}:
        return v.copy()
    if present == {1.0, 2.0}:
        return v - 1.0
    return None


ASSOC_SCORE_MAX_COLUMNS = 64


def assoc_score_groups(T: int, Pc: int):
    """[t0, t1) groups of T case / control traits, floor(64 / (Pc + 3)) to a group: what one gpca_assoc_logistic_score call takes."""
    g = ASSOC_SCORE_MAX_COLUMNS // (Pc + 3)
    if g < 1:
        raise ValueError(f"{Pc} covariates + 3 are more than {ASSOC_SCORE_MAX_COLUMNS} columns")
    return [(t0, min(t0 + g, T)) for t0 in range(0, T, g)]


def assoc_score_bands(K: int, T: int, Pc: int, max_values: int = 1 << 26):
    """[row0, row1) bands of the K kept rows for a group of T traits, sized as assoc_bands sizes them on the T (Pc + 3) panel columns."""
    return assoc_bands(K, T * (Pc + 3), max_values)


def spa_z_ok(x) -> bool:
    """The rule of gpca_assoc_logistic_spa's cutoff: at least 0.5, or inf (no correction); NaN is refused."""
    return bool(float(x) >= 0.5)


def firth_z_ok(x) -> bool:
    """The rule of gpca_assoc_logistic_firth's cutoff: at least 0, or inf (no correction); NaN is refused."""
    return bool(float(x) >= 0.0)


def write_assoc_logistic(prefix: str, trait: str, chromosomes: Sequence[str], positions: Sequence[int], variant_ids: Sequence[str],
                         allele1: Sequence[str], n_obs, a1_freq, beta, se, z, log10p, append: bool = False, spa=None, firth=None) -> str:
    """P.<trait>.assoc.logistic: one tab-separated line per SNP, `#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE Z_STAT LOG10P`; numbers as
    %.6g, NaN as NA, OBS_CT as an integer.  append=True adds the rows of a further band to the file (no header).  spa: the status of
    the saddle-point correction per SNP (gpca_assoc_logistic_spa: 0, 1, 2) adds the column `SPA` = N, Y, F (NA where LOG10P is NA).  firth: the status
    of the Firth correction per SNP (gpca_assoc_logistic_firth) adds the column `FIRTH` in the same way; the caller passes Firth's BETA
    and SE on the rows with status 1 (Z_STAT stays the score statistic).  Not both."""
    path = f"{prefix}.{trait}.assoc.logistic"
    n = len(variant_ids)
    if spa is not None and firth is not None:
        raise ValueError("write_assoc_logistic: spa or firth, not both")
    name, spa = ("FIRTH", firth) if firth is not None else ("SPA", spa)
    for a in (chromosomes, positions, allele1, n_obs, a1_freq, beta, se, z, log10p) + (() if spa is None else (spa,)):
        if len(a) != n:
            raise ValueError("write_assoc_logistic: one entry per SNP in every column")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tail = (lambda i: "") if spa is None else (lambda i: "\tNA" if log10p[i] != log10p[i] else "\t" + "NYF"[int(spa[i])])
    with open(path, "a" if append else "w") as f:
        if not append:
            f.write("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P" + ("" if spa is None else "\t" + name) + "\n")
        f.writelines(f"{chromosomes[i]}\t{int(positions[i])}\t{variant_ids[i]}\t{allele1[i]}\t{int(n_obs[i])}\t{_g6(a1_freq[i])}\t{_g6(beta[i])}\t"
                     f"{_g6(se[i])}\t{_g6(z[i])}\t{_g6(log10p[i])}{tail(i)}\n" for i in range(n))
    return path


# ---- gene-level set tests of the logistic score scan (gpca_assoc_logistic_set, gpca_set_test): twins in host/formats.hpp -----------------
ASSOC_SET_MAX_ROWS = 128


class VariantSet(NamedTuple):
    name: str
    chrom: str
    pos: int
    rows: np.ndarray        # kept rows (PCA-SNP order) of the listed IDs that are among the QC-kept SNPs: ascending, each once


def read_set_list(path: str, kept_ids: Sequence[str]) -> List[VariantSet]:
    """regenie's set list: one set per line, `NAME CHROM POS ID1,ID2,...` separated by blanks or tabs (empty lines and lines that start
    with # are skipped).  kept_ids: the IDs of the QC-kept SNPs in PCA-SNP order; an ID that is not among them is dropped, an ID that
    occurs twice among them means its first row, and an ID listed twice in a set counts once.  ValueError names the file and the line."""
    at = {}
    for i, v in enumerate(kept_ids):
        at.setdefault(v, i)
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p or p[0].startswith("#"):
                continue
            if len(p) != 4:
                raise ValueError(f"{path}:{ln}: `NAME CHROM POS ID1,ID2,...` is required")
            if not re.fullmatch(r"[+-]?[0-9]{1,18}", p[2], re.ASCII):                  # (what the twin in host/formats.hpp takes)
                raise ValueError(f"{path}:{ln}: `{p[2]}` is not a position")
            pos = int(p[2])
            rows = sorted({at[v] for v in p[3].split(",") if v in at})
            out.append(VariantSet(p[0], p[1], pos, np.asarray(rows, np.int64)))
    return out


def set_weights(a1_freq, kind: str) -> np.ndarray:
    """The weights of a set's variants from their A1 frequencies: `beta` = the Beta(maf; 1, 25) density 25 (1 - maf)^24 with
    maf = min(f, 1 - f) (the power by three squarings and one product, so that both programs round alike), `flat` = 1."""
    f = np.asarray(a1_freq, np.float64)
    if kind == "flat":
        return np.ones_like(f)
    if kind != "beta":
        raise ValueError("set_weights: beta or flat")
    q = 1.0 - np.minimum(f, 1.0 - f)
    q2 = q * q
    q4 = q2 * q2
    q8 = q4 * q4
    return 25.0 * ((q8 * q8) * q8)


def set_maf_ok(a1_freq, max_maf: float) -> np.ndarray:
    """Which variants enter a set: min(f, 1 - f) <= max_maf (a variant without an observed call, f = NaN, does not)."""
    f = np.asarray(a1_freq, np.float64)
    with np.errstate(invalid="ignore"):
        return np.minimum(f, 1.0 - f) <= max_maf


def assoc_set_groups(sizes: Sequence[int], T: int, Pc: int, max_values: int = 1 << 26):
    """[s0, s1) groups of consecutive sets (sizes = their row counts, each 1 .. 128) for one gpca_assoc_logistic_set call each: the listed
    rows' workspace (rows x T (Pc + 3) doubles, as assoc_score_bands counts it) and Phi (T m (m + 1) / 2 doubles per set) hold at most
    max_values entries each (at least one set)."""
    out, s0, rows, tri = [], 0, 0, 0
    for s, m in enumerate(sizes):
        r, t = rows + m, tri + m * (m + 1) // 2
        if s > s0 and (r * T * (Pc + 3) > max_values or t * T > max_values):
            out.append((s0, s))
            s0, r, t = s, m, m * (m + 1) // 2
        rows, tri = r, t
    if len(sizes) > s0:
        out.append((s0, len(sizes)))
    return out


def write_assoc_set(prefix: str, trait: str, names: Sequence[str], chromosomes: Sequence[str], positions: Sequence[int], n_var, results) -> str:
    """P.<trait>.assoc.set: one tab-separated line per set, in the order given, `#SET CHROM POS N_VAR N_USED BURDEN_BETA BURDEN_SE
    BURDEN_Z BURDEN_LOG10P SKAT_Q SKAT_LOG10P SKAT`; numbers as %.6g, NaN as NA; SKAT = Y, N, F for the status 1, 0, 2 of gpca_set_test
    (NA where SKAT_LOG10P is NA).  results: per set None (no test was made: everything after N_VAR is NA) or set_test's dict."""
    path = f"{prefix}.{trait}.assoc.set"
    n = len(names)
    for a in (chromosomes, positions, n_var, results):
        if len(a) != n:
            raise ValueError("write_assoc_set: one entry per set in every column")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write("#SET\tCHROM\tPOS\tN_VAR\tN_USED\tBURDEN_BETA\tBURDEN_SE\tBURDEN_Z\tBURDEN_LOG10P\tSKAT_Q\tSKAT_LOG10P\tSKAT\n")
        for i in range(n):
            r = results[i]
            head = f"{names[i]}\t{chromosomes[i]}\t{int(positions[i])}\t{int(n_var[i])}"
            if r is None:
                f.write(head + "\tNA" * 8 + "\n")
                continue
            lp = float(r["skat_log10p"])
            f.write(f"{head}\t{int(r['m_used'])}\t{_g6(r['burden_beta'])}\t{_g6(r['burden_se'])}\t{_g6(r['burden_z'])}\t{_g6(r['burden_log10p'])}\t"
                    f"{_g6(r['skat_q'])}\t{_g6(lp)}\t{'NA' if lp != lp else 'NYF'[int(r['skat_status'])]}\n")
    return path


# ---- genotype counts inside sample groups and Fst (gpca_group_counts, gpca_fst_hudson, gpca_fst_wc): twins in host/formats.hpp ------------
GROUPS_MAX = 64


class WithinTable(NamedTuple):
    family_ids: List[str]
    sample_ids: List[str]
    groups: List[Optional[str]]   # None = in no group (NA)
    names: List[str]              # the group names in order of first appearance in the file


def read_within(path: str) -> WithinTable:
    """A whitespace-separated table `FID IID GROUP`.  The header `FID IID GROUP` (a leading '#' allowed) is required; `NA` means no
    group; a repeated (FID, IID) is refused."""
    fids, iids, groups, names, seen, header = [], [], [], [], set(), False
    need = f"{path}: the header `FID IID GROUP` is required"
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if not header:
                if len(p) != 3 or p[0].lstrip("#").upper() != "FID" or p[1].upper() != "IID" or p[2].upper() != "GROUP":
                    raise ValueError(need)
                header = True
                continue
            if len(p) != 3:
                raise ValueError(f"{path}:{ln}: {len(p)} fields, the header has 3")
            if (p[0], p[1]) in seen:
                raise ValueError(f"{path}:{ln}: sample {p[0]} {p[1]} appears twice")
            seen.add((p[0], p[1]))
            g = None if p[2] == "NA" else p[2]
            if g is not None and g not in names:
                names.append(g)
            fids.append(p[0]); iids.append(p[1]); groups.append(g)
    if not header:
        raise ValueError(need)
    return WithinTable(fids, iids, groups, names)


def align_within(table: WithinTable, family_ids: Sequence[str], sample_ids: Sequence[str]) -> Tuple[np.ndarray, List[str]]:
    """(labels int32 [len(sample_ids)] in .fam order, the group names): label p = the sample is in group names[p], -1 = it is absent from
    the table or has no group.  The names are the table's, in order of first appearance in the file (a group none of whose samples is
    in the .fam stays, empty)."""
    index = {g: p for p, g in enumerate(table.names)}
    at = {(f, i): g for f, i, g in zip(table.family_ids, table.sample_ids, table.groups)}
    out = np.full(len(sample_ids), -1, np.int32)
    for n, key in enumerate(zip(family_ids, sample_ids)):
        g = at.get(key)
        if g is not None:
            out[n] = index[g]
    return out, list(table.names)


F2_BAND_ROWS_MAX = 1 << 21          # the rows gpca_f2_blocks takes in one call


def group_count_bands(K: int, P: int, max_values: int = 1 << 26, max_rows: Optional[int] = None):
    """[row0, row1) bands of the K kept rows whose counts (rows x P x 3) hold at most max_values entries (at least one row): the bands
    gpca_group_counts is asked for, one at a time.  max_rows: no band holds more rows than that (F2_BAND_ROWS_MAX for gpca_f2_blocks)."""
    step = max(max_values // (3 * max(P, 1)), 1)
    if max_rows is not None:
        step = max(min(step, int(max_rows)), 1)
    return [(r0, min(r0 + step, K)) for r0 in range(0, K, step)]


def _open_out(path: str, append: bool):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    return open(path, "a" if append else "w")


def write_frq_strat(path: str, chromosomes: Sequence[str], positions: Sequence[int], variant_ids: Sequence[str], allele1: Sequence[str],
                    names: Sequence[str], counts, append: bool = False) -> str:
    """The stratified frequency file `path` (P.frq.strat, P.<trait>.frq.cc): one tab-separated line per SNP and group, SNP-major,
    `#CHROM POS ID A1 GROUP OBS_CT A1_CT A1_FREQ HET_CT HOM_A1_CT HWE_P` from counts [SNPs][groups][3] = n_obs, n_het, n_hom2
    (gpca_group_counts).  Counts as integers, A1_CT = n_het + 2 n_hom2, A1_FREQ = A1_CT / (2 OBS_CT) and HWE_P =
    gpca_hwe_chi_squared_p_value(n_obs - n_het - n_hom2, n_het, n_hom2) as %.6g; both NA where OBS_CT = 0.  append=True adds the rows
    of a further band to the file (no header)."""
    from . import _lib
    cv = np.asarray(counts)
    n, P = len(variant_ids), len(names)
    if cv.shape != (n, P, 3):
        raise ValueError("write_frq_strat: counts must be [SNPs][groups][3]")
    for a in (chromosomes, positions, allele1):
        if len(a) != n:
            raise ValueError("write_frq_strat: one entry per SNP in every column")
    hwe = _lib.load().gpca_hwe_chi_squared_p_value
    with _open_out(path, append) as f:
        if not append:
            f.write("#CHROM\tPOS\tID\tA1\tGROUP\tOBS_CT\tA1_CT\tA1_FREQ\tHET_CT\tHOM_A1_CT\tHWE_P\n")
        for i in range(n):
            head = f"{chromosomes[i]}\t{int(positions[i])}\t{variant_ids[i]}\t{allele1[i]}\t"
            for p in range(P):
                obs, het, hom = int(cv[i, p, 0]), int(cv[i, p, 1]), int(cv[i, p, 2])
                a1 = het + 2 * hom
                if obs == 0:
                    fr, hw = "NA", "NA"
                else:
                    fr, hw = _g6(a1 / (2.0 * obs)), _g6(hwe(obs - het - hom, het, hom))
                f.write(f"{head}{names[p]}\t{obs}\t{a1}\t{fr}\t{het}\t{hom}\t{hw}\n")
    return path


def _ratio6(num: float, den: float) -> str:
    num, den = float(num), float(den)
    return "NA" if num != num or den != den or den == 0.0 else _g6(num / den)


def fst_pairs(P: int):
    """the pairs (j, i), j < i, of P groups in the order of gpca_fst_hudson's pair index i (i - 1) / 2 + j"""
    return [(j, i) for i in range(1, P) for j in range(i)]


def write_fst_summary(prefix: str, method: str, names: Sequence[str], sums) -> str:
    """P.fst.summary: `#GROUP1 GROUP2 N_VAR HUDSON_FST` (method "hudson") or `... WC_FST` ("wc"), tab-separated, one line per pair of
    groups with GROUP1 the earlier one, in the order of fst_pairs.  sums [pairs][3] = the running sum of the numerators (a), of the
    denominators (a + b + c) and the rows used; for "wc" with more than two groups a further last row of sums covers all groups jointly
    and is written as `* * N_VAR FST`.  FST = %.6g of the ratio of sums, NA where no row was used or the denominator is 0."""
    if method not in ("hudson", "wc"):
        raise ValueError("write_fst_summary: method is hudson or wc")
    P = len(names)
    pairs = fst_pairs(P)
    sv = np.asarray(sums, np.float64)
    joint = method == "wc" and P > 2
    if sv.shape != (len(pairs) + int(joint), 3):
        raise ValueError("write_fst_summary: sums must be [pairs][3] (one more row for the joint wc value of more than two groups)")
    path = f"{prefix}.fst.summary"
    with _open_out(path, False) as f:
        f.write("#GROUP1\tGROUP2\tN_VAR\t" + ("HUDSON_FST" if method == "hudson" else "WC_FST") + "\n")
        for q, (j, i) in enumerate(pairs):
            f.write(f"{names[j]}\t{names[i]}\t{int(sv[q, 2])}\t{'NA' if sv[q, 2] == 0 else _ratio6(sv[q, 0], sv[q, 1])}\n")
        if joint:
            f.write(f"*\t*\t{int(sv[-1, 2])}\t{'NA' if sv[-1, 2] == 0 else _ratio6(sv[-1, 0], sv[-1, 1])}\n")
    return path


def write_fst_var(prefix: str, method: str, chromosomes: Sequence[str], positions: Sequence[int], variant_ids: Sequence[str],
                  names: Sequence[str], values, append: bool = False) -> str:
    """P.fst.var: one tab-separated line per SNP and pair of groups (SNP-major, the pairs in the order of fst_pairs, GROUP1 the earlier
    group): `#CHROM POS ID GROUP1 GROUP2 NUM DEN FST` from values [SNPs][pairs][2] = num, den ("hudson"), or `#CHROM POS ID GROUP1 GROUP2
    A B C FST` from values [SNPs][pairs][3] = a, b, c ("wc", r = 2 on each pair).  Numbers as %.6g, NaN as NA; FST = NUM / DEN or
    A / ((A + B) + C), NA where that is NaN or the denominator is 0.  append=True adds the rows of a further band (no header)."""
    if method not in ("hudson", "wc"):
        raise ValueError("write_fst_var: method is hudson or wc")
    w = 2 if method == "hudson" else 3
    pairs = fst_pairs(len(names))
    n = len(variant_ids)
    vv = np.asarray(values, np.float64)
    if vv.shape != (n, len(pairs), w) or len(chromosomes) != n or len(positions) != n:
        raise ValueError("write_fst_var: values must be [SNPs][pairs][%d] with one entry per SNP in every column" % w)
    path = f"{prefix}.fst.var"
    with _open_out(path, append) as f:
        if not append:
            f.write("#CHROM\tPOS\tID\tGROUP1\tGROUP2\t" + ("NUM\tDEN" if method == "hudson" else "A\tB\tC") + "\tFST\n")
        for i in range(n):
            head = f"{chromosomes[i]}\t{int(positions[i])}\t{variant_ids[i]}\t"
            for q, (j, k) in enumerate(pairs):
                v = vv[i, q]
                den = v[1] if method == "hudson" else (v[0] + v[1]) + v[2]
                f.write(head + f"{names[j]}\t{names[k]}\t" + "\t".join(_g6(x) for x in v) + f"\t{_ratio6(v[0], den)}\n")
    return path


# ---- f-statistics (gpca_f2_blocks, gpca_fstat_blocks, gpca_fstat; include/gpca.h section a23): twins in host/formats.hpp -------------------
FSTAT_BLOCK_DEFAULT = "5000kb"


def fstat_blocks(chromosomes: Sequence[str], positions: Sequence[int], spec: str = FSTAT_BLOCK_DEFAULT) -> Tuple[np.ndarray, int]:
    """(block int32 [K], B): the jackknife block of every SNP of a list in genome order (gpca_fstat_blocks).  spec has parse_ld_window's
    grammar: "500" = blocks of 500 variants, "5000kb" = a block ends before the first SNP 5 000 000 bp or more beyond its first one; a
    new block starts at every change of chromosome."""
    import ctypes
    from . import _lib
    kind, w = parse_ld_window(spec)
    K = len(chromosomes)
    pos = np.ascontiguousarray(positions, np.int64)
    if pos.shape != (K,):
        raise ValueError("fstat_blocks: one position per chromosome entry")
    chrom = [normalize_chromosome_name(c) for c in chromosomes]
    change = np.zeros(max(K, 1), np.uint8)
    for r in range(1, K):
        change[r] = chrom[r] != chrom[r - 1]
    block = np.zeros(max(K, 1), np.int32)
    nb = ctypes.c_int32(0)
    rc = _lib.load().gpca_fstat_blocks(change.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p) if K else None, K, int(w),
                                       _lib.FSTAT_BLOCK_VARIANTS if kind == "variants" else _lib.FSTAT_BLOCK_BP,
                                       block.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nb))
    if rc != _lib.GPCA_OK:
        raise ValueError(f"fstat_blocks: gpca_fstat_blocks refused the block size '{spec}'")
    return block[:K], int(nb.value)


def read_fstats_list(path: str, names: Sequence[str]) -> List[Tuple[str, Tuple[int, ...]]]:
    """The statistics of --gpca-fstats: one per line, `f2 A B`, `f3 C A B` (C is the target) or `f4 A B C D` with group names; '#' lines
    and blank lines are skipped.  Returns [(kind, the groups' indices in names)].  An unknown name, another keyword or a wrong number
    of names is an error that names the line."""
    arity = {"f2": 2, "f3": 3, "f4": 4}
    index = {g: p for p, g in enumerate(names)}
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p or p[0].startswith("#"):
                continue
            if p[0] not in arity:
                raise ValueError(f"{path}:{ln}: '{p[0]}' is not f2, f3 or f4")
            if len(p) - 1 != arity[p[0]]:
                raise ValueError(f"{path}:{ln}: {p[0]} takes {arity[p[0]]} groups, {len(p) - 1} are given")
            for g in p[1:]:
                if g not in index:
                    raise ValueError(f"{path}:{ln}: no group '{g}' in the within file")
            out.append((p[0], tuple(index[g] for g in p[1:])))
    return out


def fstat_quad(kind: str, groups: Sequence[int]) -> Tuple[int, int, int, int]:
    """gpca_fstat's quad (a, b, c, d), read as f4(a, b; c, d): f2(A, B) = (A, B, A, B), f3(C; A, B) = (C, A, C, B), f4 as it is"""
    g = [int(x) for x in groups]
    if kind == "f2" and len(g) == 2:
        return g[0], g[1], g[0], g[1]
    if kind == "f3" and len(g) == 3:
        return g[0], g[1], g[0], g[2]
    if kind == "f4" and len(g) == 4:
        return g[0], g[1], g[2], g[3]
    raise ValueError("fstat_quad: f2 takes 2 groups, f3 3 and f4 4")


def write_f2_summary(prefix: str, names: Sequence[str], stats) -> str:
    """P.f2.summary: `#POP1 POP2 F2 SE Z N_BLOCKS N_SNPS`, tab-separated, one line per pair of groups with POP1 the earlier one, in the
    order of fst_pairs; stats [pairs][6] = gpca_fstat's rows of the quads (j, i, j, i).  F2 = theta, SE and Z as %.6g, NaN as NA; the
    blocks used and the SNPs of the pair as integers."""
    pairs = fst_pairs(len(names))
    sv = np.asarray(stats, np.float64)
    if sv.shape != (len(pairs), 6):
        raise ValueError("write_f2_summary: stats must be [pairs][6]")
    path = f"{prefix}.f2.summary"
    with _open_out(path, False) as f:
        f.write("#POP1\tPOP2\tF2\tSE\tZ\tN_BLOCKS\tN_SNPS\n")
        for q, (j, i) in enumerate(pairs):
            s = sv[q]
            f.write(f"{names[j]}\t{names[i]}\t{_g6(s[0])}\t{_g6(s[2])}\t{_g6(s[3])}\t{_count_or_na(s[4])}\t{_count_or_na(s[5])}\n")
    return path


def _count_or_na(x: float) -> str:
    x = float(x)
    return "NA" if x != x else str(int(x))


def write_fstats(prefix: str, names: Sequence[str], stats_list, stats) -> str:
    """P.fstats: `#STAT POP1 POP2 POP3 POP4 EST SE Z N_BLOCKS N_SNPS`, tab-separated, one line per statistic of stats_list
    (read_fstats_list) in its order, the groups as the list gave them and `.` for the columns a statistic does not have; stats [M][6] =
    gpca_fstat's rows of fstat_quad of each.  EST = theta; numbers as in write_f2_summary."""
    sv = np.asarray(stats, np.float64).reshape(-1, 6)
    if sv.shape[0] != len(stats_list):
        raise ValueError("write_fstats: one row of stats per statistic")
    path = f"{prefix}.fstats"
    with _open_out(path, False) as f:
        f.write("#STAT\tPOP1\tPOP2\tPOP3\tPOP4\tEST\tSE\tZ\tN_BLOCKS\tN_SNPS\n")
        for (kind, groups), s in zip(stats_list, sv):
            cols = [names[g] for g in groups] + ["."] * (4 - len(groups))
            f.write(kind + "\t" + "\t".join(cols) + f"\t{_g6(s[0])}\t{_g6(s[2])}\t{_g6(s[3])}\t{_count_or_na(s[4])}\t{_count_or_na(s[5])}\n")
    return path


# ---- genotype counts per sample, heterozygosity F and sample QC (gpca_sample_counts, gpca_het_weights, gpca_sample_het): twins in
# host/formats.hpp ------------------------------------------------------------------------------------------------------------------------
def sample_count_bands(K: int, max_rows: int = 1 << 24):
    """[row0, row1) bands of the K kept rows of at most max_rows rows: the bands gpca_sample_counts is asked for, one at a time (a band's
    weights travel with it; its counts are per sample and are summed over the bands by the caller)."""
    step = max(int(max_rows), 1)
    return [(r0, min(r0 + step, K)) for r0 in range(0, K, step)]


def write_smiss(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], counts, K: int) -> str:
    """P.smiss (plink --missing's sample table): one tab-separated line per sample, `#FID IID MISSING_CT OBS_CT F_MISS` from counts [N][3]
    = n_obs, n_het, n_hom2 over K SNPs: MISSING_CT = K - n_obs, OBS_CT = K (the SNPs looked at, as plink 2 prints it), F_MISS =
    MISSING_CT / K as %.6g (NA for K = 0)."""
    cv = np.asarray(counts)
    n = len(sample_ids)
    if cv.shape != (n, 3) or len(family_ids) != n:
        raise ValueError("write_smiss: counts must be [samples][3] with one FID and IID per sample")
    path = f"{prefix}.smiss"
    with _open_out(path, False) as f:
        f.write("#FID\tIID\tMISSING_CT\tOBS_CT\tF_MISS\n")
        for i in range(n):
            mis = int(K) - int(cv[i, 0])
            f.write(f"{family_ids[i]}\t{sample_ids[i]}\t{mis}\t{int(K)}\t{'NA' if K == 0 else _g6(float(mis) / float(K))}\n")
    return path


def write_het(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], counts, het) -> str:
    """P.het (plink --het): one tab-separated line per sample, `#FID IID O_HOM E_HOM OBS_CT F` from counts [N][3] (OBS_CT = n_obs, the
    sample's observed calls) and het [N][3] = O_HOM, E_HOM, F (gpca_sample_het); the three numbers as %.6g, NaN as NA."""
    cv, hv = np.asarray(counts), np.asarray(het, np.float64)
    n = len(sample_ids)
    if cv.shape != (n, 3) or hv.shape != (n, 3) or len(family_ids) != n:
        raise ValueError("write_het: counts and het must be [samples][3] with one FID and IID per sample")
    path = f"{prefix}.het"
    with _open_out(path, False) as f:
        f.write("#FID\tIID\tO_HOM\tE_HOM\tOBS_CT\tF\n")
        for i in range(n):
            f.write(f"{family_ids[i]}\t{sample_ids[i]}\t{_g6(hv[i, 0])}\t{_g6(hv[i, 1])}\t{int(cv[i, 0])}\t{_g6(hv[i, 2])}\n")
    return path


def sample_qc_pass(counts, K: int, F=None, mind: Optional[float] = None, het_sd: Optional[float] = None):
    """The sample filters (plink --mind; the usual heterozygosity rule of GWAS protocols) from counts [N][3] over K SNPs and F [N]
    (needed with het_sd).  Returns (pass uint8 [N], reason: a list of None, "MIND" or "HET").  Sequential f64 loops in sample order:
      mind:   F_MISS = (K - n_obs) / K; a sample fails MIND if n_obs = 0 or F_MISS > mind.
      het_sd: over the c samples that pass MIND and have a finite F, m = (sum F) / c and s = sqrt(sum (F - m)^2 / (c - 1)); a sample
              that passes MIND fails HET if F is NaN or |F - m| > het_sd s.  One round; with c < 2 or s = 0 only NaN fails."""
    cv = np.asarray(counts)
    n = cv.shape[0]
    if cv.ndim != 2 or cv.shape[1] != 3:
        raise ValueError("sample_qc_pass: counts must be [samples][3]")
    ok = np.ones(n, np.uint8)
    reason: List[Optional[str]] = [None] * n
    if mind is not None:
        for i in range(n):
            nobs = int(cv[i, 0])
            if nobs == 0 or float(int(K) - nobs) / float(K) > float(mind):
                ok[i], reason[i] = 0, "MIND"
    if het_sd is not None:
        fv = np.asarray(F, np.float64)
        if fv.shape != (n,):
            raise ValueError("sample_qc_pass: het_sd needs F with one entry per sample")
        c, tot = 0, 0.0
        for i in range(n):
            if ok[i] and math.isfinite(fv[i]):
                c += 1
                tot = tot + float(fv[i])
        m = tot / c if c else 0.0
        ss = 0.0
        for i in range(n):
            if ok[i] and math.isfinite(fv[i]):
                d = float(fv[i]) - m
                ss = ss + d * d
        s = math.sqrt(ss / (c - 1)) if c >= 2 else 0.0
        for i in range(n):
            if not ok[i]:
                continue
            x = float(fv[i])
            if x != x or (c >= 2 and s > 0.0 and abs(x - m) > float(het_sd) * s):
                ok[i], reason[i] = 0, "HET"
    return ok, reason


def write_sample_qc_ids(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], passed, reason) -> Tuple[str, str]:
    """P.sampleqc.in.id (`#FID IID`: the samples that pass) and P.sampleqc.out.id (`#FID IID REASON`, REASON = MIND or HET), both
    tab-separated, in sample order."""
    n = len(sample_ids)
    if len(family_ids) != n or len(passed) != n or len(reason) != n:
        raise ValueError("write_sample_qc_ids: one entry per sample in every column")
    pin, pout = f"{prefix}.sampleqc.in.id", f"{prefix}.sampleqc.out.id"
    with _open_out(pin, False) as fi, _open_out(pout, False) as fo:
        fi.write("#FID\tIID\n")
        fo.write("#FID\tIID\tREASON\n")
        for i in range(n):
            if passed[i]:
                fi.write(f"{family_ids[i]}\t{sample_ids[i]}\n")
            else:
                fo.write(f"{family_ids[i]}\t{sample_ids[i]}\t{reason[i]}\n")
    return pin, pout


# ---- runs of homozygosity (gpca_roh, gpca_roh_select): twins in host/formats.hpp -----------------------------------------------------------
def roh_breaks(chromosomes: Sequence[str], positions: Sequence[int], max_gap_bp: int) -> np.ndarray:
    """brk [K] (uint8) over the kept SNPs, in their order, for gpca_roh: 3 at the first SNP of every chromosome run (a window domain
    starts, and no run continues into it), 2 at a SNP that lies more than max_gap_bp behind the SNP before it, else 0.  A chromosome
    that reappears after another, or positions that decrease inside a run, is an error that names the variant (by its index among the
    SNPs given), as in ld_windows."""
    K = len(chromosomes)
    pos = np.asarray(positions, np.int64)
    if pos.shape != (K,):
        raise ValueError("roh_breaks: one position per chromosome entry")
    if int(max_gap_bp) < 0:
        raise ValueError("roh_breaks: the gap must be at least 0")
    brk = np.zeros(K, np.uint8)
    seen = set()
    s = 0
    while s < K:
        c = normalize_chromosome_name(chromosomes[s])
        if c in seen:
            raise ValueError(f"roh_breaks: chromosome '{chromosomes[s]}' reappears at variant {s} after another chromosome: sort the variants")
        seen.add(c)
        brk[s] = 3
        e = s + 1
        while e < K and normalize_chromosome_name(chromosomes[e]) == c:
            if pos[e] < pos[e - 1]:
                raise ValueError(f"roh_breaks: the position of variant {e} ({int(pos[e])}) is below that of the variant before it on chromosome "
                                 f"'{chromosomes[e]}': sort the variants")
            if int(pos[e]) - int(pos[e - 1]) > int(max_gap_bp):
                brk[e] = 2
            e += 1
        s = e
    return brk


def roh_bands(brk, max_rows: int = 1 << 24):
    """[row0, row1) bands over the rows of brk that are cut only where a window domain starts (bit 0): whole domains are added to a band
    while it stays within max_rows rows; a domain longer than that is a band of its own.  The bands gpca_roh is asked for, one at a
    time: their records and counts add up to the full call's."""
    bv = np.asarray(brk, np.uint8)
    K = bv.size
    starts = [0] + [int(j) for j in np.nonzero(bv & 1)[0] if j > 0] + [K]
    out = []
    r0 = 0
    for d in range(1, len(starts)):
        if d + 1 < len(starts) and starts[d + 1] - r0 <= max(int(max_rows), 1):
            continue
        if starts[d] > r0:
            out.append((r0, starts[d]))
        r0 = starts[d]
    return out


def roh_select(segs, positions, min_bp: int, max_bp_per_snp: int) -> np.ndarray:
    """keep [n] (uint8) of the records segs [n][5] = sample, first, last, n_het, n_missing (first and last index positions [K]), in
    integers: span = pos[last] - pos[first]; 1 iff span >= min_bp and span <= max_bp_per_snp x (last - first + 1).  The twin of
    gpca_roh_select."""
    sv = np.asarray(segs, np.int64).reshape(-1, 5)
    pos = np.asarray(positions, np.int64)
    keep = np.zeros(sv.shape[0], np.uint8)
    for i in range(sv.shape[0]):
        first, last = int(sv[i, 1]), int(sv[i, 2])
        if last < first:
            raise ValueError(f"roh_select: record {i} ends before it starts")
        span = int(pos[last]) - int(pos[first])
        keep[i] = 1 if span >= int(min_bp) and span <= int(max_bp_per_snp) * (last - first + 1) else 0
    return keep


def roh_summary(segs, keep, positions, brk, n_samples: int):
    """Per sample, from the kept records: (NSEG int64 [N], total bp int64 [N], FROH float64 [N]).  total bp = the sum of
    pos[last] - pos[first] over the sample's kept records; FROH = total bp / genome, genome = the sum over the window domains (bit 0 of
    brk; row 0 starts one) of pos[last row] - pos[first row]; NaN when that sum is 0."""
    sv = np.asarray(segs, np.int64).reshape(-1, 5)
    kv = np.asarray(keep).reshape(-1)
    pos = np.asarray(positions, np.int64)
    bv = np.asarray(brk, np.uint8)
    K = bv.size
    if kv.shape[0] != sv.shape[0] or pos.shape != (K,):
        raise ValueError("roh_summary: one keep flag per record and one position per row of brk")
    starts = [0] + [int(j) for j in np.nonzero(bv & 1)[0] if j > 0] + [K]
    genome = 0
    for d in range(len(starts) - 1):
        if starts[d + 1] > starts[d]:
            genome += int(pos[starts[d + 1] - 1]) - int(pos[starts[d]])
    nseg = np.zeros(int(n_samples), np.int64)
    total = np.zeros(int(n_samples), np.int64)
    for i in range(sv.shape[0]):
        if kv[i]:
            nseg[sv[i, 0]] += 1
            total[sv[i, 0]] += int(pos[sv[i, 2]]) - int(pos[sv[i, 1]])
    froh = np.full(int(n_samples), np.nan)
    if genome > 0:
        for n in range(int(n_samples)):
            froh[n] = float(int(total[n])) / float(genome)
    return nseg, total, froh


def write_hom(prefix: str, family_ids: Sequence[str], sample_ids: Sequence[str], chromosomes: Sequence[str], variant_ids: Sequence[str],
              positions: Sequence[int], segs, keep, brk) -> Tuple[str, str]:
    """P.hom (plink --homozyg's segment table): one tab-separated line per kept record, in sample order then by position,
    `#FID IID CHROM SNP1 SNP2 POS1 POS2 KB NSNP DENSITY PHOM PHET`: KB = span / 1000, DENSITY = KB / NSNP, PHOM = (NSNP - het -
    missing) / NSNP, PHET = het / NSNP, each as %.6g.  P.hom.indiv: one line per sample, `#FID IID NSEG KB KBAVG FROH` (roh_summary):
    KB = total bp / 1000, KBAVG = KB / NSEG (NA without a segment), FROH (NA where undefined).  chromosomes, variant_ids and positions
    are those of the kept SNPs."""
    sv = np.asarray(segs, np.int64).reshape(-1, 5)
    kv = np.asarray(keep).reshape(-1)
    pos = np.asarray(positions, np.int64)
    n = len(sample_ids)
    if len(family_ids) != n or kv.shape[0] != sv.shape[0] or len(chromosomes) != pos.size or len(variant_ids) != pos.size:
        raise ValueError("write_hom: one FID per IID, one keep flag per record, one chromosome and id per position")
    nseg, total, froh = roh_summary(sv, kv, pos, brk, n)
    phom, pind = f"{prefix}.hom", f"{prefix}.hom.indiv"
    with _open_out(phom, False) as f:
        f.write("#FID\tIID\tCHROM\tSNP1\tSNP2\tPOS1\tPOS2\tKB\tNSNP\tDENSITY\tPHOM\tPHET\n")
        for i in range(sv.shape[0]):
            if not kv[i]:
                continue
            s, first, last, nh, nm = (int(v) for v in sv[i])
            nsnp = last - first + 1
            kb = float(int(pos[last]) - int(pos[first])) / 1000.0
            f.write(f"{family_ids[s]}\t{sample_ids[s]}\t{chromosomes[first]}\t{variant_ids[first]}\t{variant_ids[last]}\t{int(pos[first])}\t"
                    f"{int(pos[last])}\t{_g6(kb)}\t{nsnp}\t{_g6(kb / float(nsnp))}\t{_g6(float(nsnp - nh - nm) / float(nsnp))}\t"
                    f"{_g6(float(nh) / float(nsnp))}\n")
    with _open_out(pind, False) as f:
        f.write("#FID\tIID\tNSEG\tKB\tKBAVG\tFROH\n")
        for i in range(n):
            kb = float(int(total[i])) / 1000.0
            f.write(f"{family_ids[i]}\t{sample_ids[i]}\t{int(nseg[i])}\t{_g6(kb)}\t{'NA' if nseg[i] == 0 else _g6(kb / float(int(nseg[i])))}\t"
                    f"{_g6(froh[i])}\n")
    return phom, pind


# ---- admixture proportions (gpca_admix; gpca.h section a21): the host rules around the fit ------------------------------------------
ADMIX_EPS = np.float32(1e-5)


def admix_order(Q, mode=None) -> np.ndarray:
    """The column order of an admixture result: the permutation (int64 [K]) by descending column sum of Q [N][K] over the samples with
    mode != 1, sums in f64 in sample order, ties to the lower index.  With a mode-1 sample (a supervised fit, whose columns are the
    groups) it is the identity."""
    qv = np.asarray(Q, np.float64)
    if qv.ndim != 2:
        raise ValueError("admix_order: Q must be [samples][K]")
    K = qv.shape[1]
    mv = np.zeros(qv.shape[0], np.uint8) if mode is None else np.asarray(mode)
    if mv.shape != (qv.shape[0],):
        raise ValueError("admix_order: one mode byte per sample")
    if (mv == 1).any():
        return np.arange(K, dtype=np.int64)
    sums = [0.0] * K
    for n in range(qv.shape[0]):
        for k in range(K):
            sums[k] += float(qv[n, k])
    return np.array(sorted(range(K), key=lambda k: (-sums[k], k)), np.int64)


def admix_supervised(labels, K: int, Q=None) -> Tuple[np.ndarray, np.ndarray]:
    """The start of a supervised fit from group labels [N] (0 .. K - 1; negative = no label): (Q float32 [N][K], mode uint8 [N]).  A
    labelled sample's row is the one-hot row of its group, clamped to >= 1e-5 and divided by its sum (f32, columns ascending), and its
    mode is 1; an unlabelled sample keeps its row of the given Q (1 / K without one) and mode 0."""
    lv = np.asarray(labels, np.int64).reshape(-1)
    K = int(K)
    if K < 1 or (lv >= K).any():
        raise ValueError("admix_supervised: a label must be below K")
    out = np.full((lv.size, K), np.float32(1.0) / np.float32(K), np.float32) if Q is None else np.array(Q, np.float32, order="C")
    if out.shape != (lv.size, K):
        raise ValueError("admix_supervised: Q must be [samples][K]")
    mode = (lv >= 0).astype(np.uint8)
    for n in np.nonzero(lv >= 0)[0]:
        row = np.full(K, ADMIX_EPS, np.float32)
        row[lv[n]] = np.float32(1.0)
        s = np.float32(0.0)
        for k in range(K):
            s = np.float32(s + row[k])
        out[n] = row / s
    return out, mode


def write_admix(prefix: str, K: int, family_ids: Sequence[str], sample_ids: Sequence[str], variant_ids: Sequence[str], Q, F, info) -> Tuple[str, ...]:
    """The files of an admixture fit, columns as given (the caller applies admix_order): P.<K>.Q, one line per sample of K `%.6f`
    separated by spaces (ADMIXTURE's layout); P.<K>.Q.id, `#FID IID` and one tab-separated line per sample; P.<K>.P, one line per SNP
    of K `%.6f` (the A1 frequency in each ancestry); P.<K>.P.id, one variant id per line; P.<K>.admix.log, `#K SEED STEPS CYCLES
    CONVERGED LOGLIK` and one tab-separated line from info (seed, steps, cycles, converged, loglik; the log-likelihood as %.4f)."""
    qv, fv = np.asarray(Q, np.float64), np.asarray(F, np.float64)
    K = int(K)
    if qv.shape != (len(sample_ids), K) or fv.shape != (len(variant_ids), K) or len(family_ids) != len(sample_ids):
        raise ValueError("write_admix: Q must be [samples][K] and F [SNPs][K], with one FID per IID")
    base = f"{prefix}.{K}"
    paths = (base + ".Q", base + ".Q.id", base + ".P", base + ".P.id", base + ".admix.log")
    for path, m in ((paths[0], qv), (paths[2], fv)):
        with _open_out(path, False) as f:
            for i in range(m.shape[0]):
                f.write(" ".join("%.6f" % float(v) for v in m[i]) + "\n")
    with _open_out(paths[1], False) as f:
        f.write("#FID\tIID\n")
        for a, b in zip(family_ids, sample_ids):
            f.write(f"{a}\t{b}\n")
    with _open_out(paths[3], False) as f:
        for v in variant_ids:
            f.write(f"{v}\n")
    with _open_out(paths[4], False) as f:
        f.write("#K\tSEED\tSTEPS\tCYCLES\tCONVERGED\tLOGLIK\n")
        f.write(f"{K}\t{int(info['seed'])}\t{int(info['steps'])}\t{int(info['cycles'])}\t{1 if info['converged'] else 0}\t{'%.4f' % float(info['loglik'])}\n")
    return paths


def write_admix_cv(prefix: str, rows) -> str:
    """P.admix.cv, the cross-validation of the admixture fit (gpca_admix_cv; gpca.h section a22): `#K FOLDS CV_SEED FOLD STEPS CONVERGED
    N_HELD DEVIANCE CV_ERROR`, tab-separated.  rows: one dict per fold (K, folds, cv_seed, fold, steps, converged, n_held, deviance), the
    folds of one K together and ascending; CV_ERROR of a fold is its deviance / n_held.  After the folds of a K comes one line with
    FOLD `*` and the totals: the summed steps, 1 if every fold converged, the summed n_held and deviance (folds ascending), and the K's
    cross-validation error, their quotient.  The two floats as `%.6f`, NaN (nothing held) as NA."""
    def num(x):
        return "NA" if x != x else "%.6f" % x

    def line(K, folds, seed, fold, steps, conv, held, dev):
        return f"{K}\t{folds}\t{seed}\t{fold}\t{steps}\t{1 if conv else 0}\t{held}\t{num(dev)}\t{num(dev / held if held > 0 else float('nan'))}\n"

    path = prefix + ".admix.cv"
    rows = list(rows)
    with _open_out(path, False) as f:
        f.write("#K\tFOLDS\tCV_SEED\tFOLD\tSTEPS\tCONVERGED\tN_HELD\tDEVIANCE\tCV_ERROR\n")
        i = 0
        while i < len(rows):
            j = i
            while j < len(rows) and int(rows[j]["K"]) == int(rows[i]["K"]):
                j += 1
            steps, conv, held, dev = 0, True, 0, 0.0
            for r in rows[i:j]:
                f.write(line(int(r["K"]), int(r["folds"]), int(r["cv_seed"]), int(r["fold"]), int(r["steps"]), bool(r["converged"]), int(r["n_held"]),
                             float(r["deviance"])))
                steps += int(r["steps"]); conv = conv and bool(r["converged"]); held += int(r["n_held"]); dev += float(r["deviance"])
            f.write(line(int(rows[i]["K"]), int(rows[i]["folds"]), int(rows[i]["cv_seed"]), "*", steps, conv, held, dev))
            i = j
    return path
