"""The GRM's host side without a GPU: GCTA's file layout (io.write_grm), the C ABI's constants and prototype, the command line's rules."""
import ctypes
import os
import re

import numpy as np
import pytest

from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import grm_bands, main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_grm_layout(tmp_path):
    n = 7
    il = np.tril_indices(n)
    full = np.arange(n * n, dtype=np.float64).reshape(n, n) / 3.0
    packed = full[il]
    npairs = (np.arange(packed.size) % 5 + 90).astype(np.float32)
    bands, r0 = [], 0
    for r1 in (2, 5, 7):
        a, b = r0 * (r0 + 1) // 2, r1 * (r1 + 1) // 2
        bands.append((packed[a:b], npairs[a:b]))
        r0 = r1
    pre = str(tmp_path / "out")
    paths = gio.write_grm(pre, [f"F{i}" for i in range(n)], [f"I{i}" for i in range(n)], iter(bands))
    assert paths == (pre + ".grm.bin", pre + ".grm.N.bin", pre + ".grm.id")
    assert os.path.getsize(paths[0]) == 4 * n * (n + 1) // 2 == os.path.getsize(paths[1])
    g = np.fromfile(paths[0], dtype="<f4")
    assert np.array_equal(g, packed.astype(np.float32))
    assert np.array_equal(np.fromfile(paths[1], dtype="<f4"), npairs)
    # element (i, j <= i) at i (i + 1) / 2 + j
    assert g[5 * 6 // 2 + 3] == np.float32(full[5, 3])
    assert open(paths[2]).read() == "".join(f"F{i}\tI{i}\n" for i in range(n))
    with pytest.raises(ValueError):
        gio.write_grm(pre, ["F"] * n, ["I"] * n, iter(bands[:2]))
    with pytest.raises(ValueError):
        gio.write_grm(pre, ["F"] * (n - 1), ["I"] * n, iter(bands))


def test_read_plink_family_ids(tmp_path):
    pre = str(tmp_path / "x")
    G = np.array([[0, 1, 2], [2, -127, 0]], np.int8)
    gio.write_plink(pre, G, ["a", "b", "c"], ["r1", "r2"], ["1", "1"], [10, 20])
    with open(pre + ".fam", "w") as f:
        f.write("fa a 0 0 0 -9\nfb b 0 0 0 -9\nfc c 0 0 0 -9\n")
    fs = gio.read_plink(pre + ".bed")
    assert fs.family_ids == ["fa", "fb", "fc"] and fs.sample_ids == ["a", "b", "c"]
    # existing positional construction keeps working without FIDs
    assert gio.PlinkFileset(fs.bed_rows, 3, fs.sample_ids, fs.variant_ids, fs.chromosomes, fs.positions).family_ids is None


def test_grm_constants_and_prototype():
    hdr = open(os.path.join(ROOT, "include", "gpca.h")).read()
    m = re.search(r"enum\s*\{\s*GPCA_GRM_STANDARDIZED\s*=\s*(\d+)\s*,\s*GPCA_GRM_CENTRED\s*=\s*(\d+)\s*\}", hdr)
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 1)
    assert (_lib.GRM_STANDARDIZED, _lib.GRM_CENTRED) == (0, 1)
    assert "gpca_grm" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["gpca_grm"]
    assert res is ctypes.c_int and args[1:] == [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert re.search(r"GPCA_API int gpca_grm\(gpca_handle\* h, int32_t scaling, int64_t row0, int64_t row1, double\* grm, float\* npairs", hdr)


def test_grm_bands_cover_the_triangle():
    for n, cap in ((1, 4), (10, 4), (100, 1000), (37, 1)):
        bands = list(grm_bands(n, cap))
        assert bands[0][0] == 0 and bands[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        assert all(r1 - r0 == 1 or r1 * (r1 + 1) // 2 - r0 * (r0 + 1) // 2 <= cap for r0, r1 in bands)


@pytest.mark.parametrize("extra", [[], ["--gpca-grm-scaling", "centred"]])
def test_make_grm_needs_eigensnp(extra):
    with pytest.raises(SystemExit) as ei:
        main(["--vcf-dir", "nowhere", "--components", "2", "--out", "x", "--gpca-make-grm", *extra])
    assert "--gpca-make-grm needs the --eigensnp workflow" in str(ei.value)
    with pytest.raises(SystemExit):
        main(["--bed-file", "t.bed", "--gpca-project-model", "m.tsv", "--out", "x", "--gpca-make-grm"])
    with pytest.raises(SystemExit):
        main(["--eigensnp", "--gpca-grm-scaling", "other"])
