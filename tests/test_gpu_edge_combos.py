"""The band kernels at the crossings of their edge axes: every case of the two pairwise tables of tests/_combos.py, per feature, on
the device, held to the feature's own model by the feature module's own checker.

The feature modules walk one axis at a time.  Here a band that does not start at 0 meets a keep mask with holes, the last partial
sample block, a live missing plane and a second workgroup in one call: group_counts (R = kGcRows = 128; x: P in {2, 33, 64}),
f2_blocks (R = kFbRun = 256; x: (P, blocks) in {(2, one block), (24, runs of 7 with rows in no block), (64, every row its own)}),
sample_counts (R = 64; x: forced splits and weights), roh (R = 64; x: (window, forced splits) in {(5, default), (50, 3), (64, 7)}, a
domain start at K // 3 and a cut at K // 2) and ld_score (R = 64; x: a uniform window of 1, 63 or 200 rows) over the row-band table;
king and grm (both scalings) over the sample-band table.  Every comparison is array_equal: the outputs are exact integers, or f64 of
exact integers.  One engine per (feature, storage) serves the whole table and is re-loaded per case, so a handle that changes its
shape, its keep mask and its band between calls is exercised as well.  tests/test_edge_combos_table.py shows, without a device, that
the tables cover every pair and that each case can bite.

RECORDS (not thresholds).  On one MI355X the 256 cases of this module take 3.4 s of wall time in all (pytest --durations, in one
process with the seven feature modules); the slowest case is grm at 4097 kept rows x 1025 samples with the tail band, 0.61 s, most
of it the numpy model.  Per feature, the slowest combo case against the slowest case of the feature's own module in the same run:
group_counts 0.02 s / 0.03 s (but 0.24 s for whichever case is the first GPU call of the process and brings the runtime up),
f2_blocks 0.03 s / 0.07 s, sample_counts 0.03 s / 0.14 s, roh 0.01 s / 0.06 s, ld_score 0.01 s / 0.16 s, king 0.15 s / 0.50 s,
grm 0.61 s / 0.32 s -- none above twice its module's, so the K = 4097 class stands at every sample count."""
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib

import _combos as C

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}


@pytest.fixture(scope="module")
def engine_of():
    """one engine per (feature, storage), opened at its first case and closed with the module"""
    pool = {}

    def get(feature, store):
        if (feature, store) not in pool:
            pool[feature, store] = gpca.GpcaEngine(storage=STORES[store])
        return pool[feature, store]
    yield get
    for e in pool.values():
        e.close()


def _cases(feature):
    return [pytest.param(i, id=f"{i}-{C.case_id(c)}") for i, c in enumerate(C.table_of(feature))]


def _run(feature, i, engine_of, monkeypatch):
    inp = C.build(feature, i)
    C.FEATURES[feature].run(engine_of(feature, inp["store"]), inp, monkeypatch)


@pytest.mark.parametrize("i", _cases("group_counts"))
def test_group_counts(i, engine_of, monkeypatch):
    _run("group_counts", i, engine_of, monkeypatch)


@pytest.mark.parametrize("i", _cases("f2_blocks"))
def test_f2_blocks(i, engine_of, monkeypatch):
    _run("f2_blocks", i, engine_of, monkeypatch)


@pytest.mark.parametrize("i", _cases("sample_counts"))
def test_sample_counts(i, engine_of, monkeypatch):
    _run("sample_counts", i, engine_of, monkeypatch)


@pytest.mark.parametrize("i", _cases("roh"))
def test_roh(i, engine_of, monkeypatch):
    _run("roh", i, engine_of, monkeypatch)


@pytest.mark.parametrize("i", _cases("ld_score"))
def test_ld_score(i, engine_of, monkeypatch):
    _run("ld_score", i, engine_of, monkeypatch)


@pytest.mark.parametrize("i", _cases("king"))
def test_king(i, engine_of, monkeypatch):
    _run("king", i, engine_of, monkeypatch)


@pytest.mark.parametrize("i", _cases("grm"))
def test_grm(i, engine_of, monkeypatch):
    _run("grm", i, engine_of, monkeypatch)
