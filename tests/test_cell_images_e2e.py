"""Barcode mode with the cells' index tables built on the device (t4_cellset stages compact images): the lock-step walk of
tests/test_cellset_emu.py against ONE unmodified reference SeqSet on a few dozen cells, with t4_cellset_image_stats held against
what the cells hold; and, on the GPU, `trust4-hip --barcode` against the reference binary, byte for byte."""
import ctypes as C
import filecmp
import os
import random

import pytest

import t4check
from t4libs import Ref
from test_cellset_emu import annotate, make_cells, run_cellset, run_reference
from test_stage1_e2e import REF_BIN, _barcode_case, _driver


@pytest.fixture(scope="module")
def emu_engine():
    os.environ["T4_LIB"] = t4check.build_emulator_lib()
    import trust4_amd
    eng = trust4_amd.Engine(0)
    yield eng
    eng.close()
    os.environ.pop("T4_LIB", None)


def table_slots(nkeys):
    sz = 64
    while 2 * sz < 3 * nkeys + 2:   # load factor <= 2/3
        sz <<= 1
    return sz


def live_keys_staged(eng, cs):
    fn = eng.lib.t4_cellset_live_keys_staged
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
    return fn(cs.h)


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libt4ref.so not built")
def test_cells_with_device_built_tables_match_reference(emu_engine, tmp_path):
    k, n_cells = 9, 30
    cells = make_cells(11, n_cells, 6)
    names, thr = annotate(cells, 11)
    release = {2, 17}
    ref, log_ref = run_reference(cells, names, thr, k, release)
    cs, log_mine = run_cellset(emu_engine, cells, names, thr, k, release, 8, 2)
    for bc in range(n_cells):
        assert log_ref[bc] == log_mine[bc], bc
    assert ref.size() == cs.size()
    bnames = ["BC%03d" % i for i in range(n_cells)]
    pa, pb = str(tmp_path / "ref.out"), str(tmp_path / "mine.out")
    ref.output_barcodes(pa, bnames)
    cs.output(pb, bnames)
    assert filecmp.cmp(pa, pb, shallow=False)
    assert sum(1 for l in log_ref for x in l if x[0] == "add" and x[1] >= 0) > 30
    # every image the cells staged had its table built on the device, from one record per key that owns postings
    c, st = cs.counters(), cs.image_stats()
    assert c["images_staged"] >= n_cells
    assert st["images_built_on_device"] == c["images_staged"]
    assert st["key_records_shipped"] == live_keys_staged(emu_engine, cs) > 0
    assert st["table_bytes_built_on_device"] >= 16 * 64 * st["images_built_on_device"]
    assert st["bytes_staged"] == c["bytes_staged"] > 16 * st["key_records_shipped"]


def test_key_records_equal_the_distinct_kmers_of_the_cells(emu_engine):
    """one contig per cell, one query batch over all cells: every cell is staged exactly once, and the key records shipped are the
    distinct k-mers of the contigs (a cell's index holds one list per k-mer of its contigs)"""
    import trust4_amd
    k, n_cells = 9, 24
    rnd = random.Random(4)
    cs = trust4_amd.CellSet(emu_engine, k, 13)
    contigs = []
    for bc in range(n_cells):
        unit = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(30, 90)))
        s = unit + unit[: rnd.randrange(0, 25)]   # some k-mers twice: one key, two postings
        contigs.append(s)
        assert cs.cell(bc).input_novel_read("Novel", s, 1, bc) == 0
    cs.prefetch(list(range(n_cells)), [s[5:] + "ACGTAC" for s in contigs], [0] * n_cells)
    st = cs.image_stats()
    distinct = [len({s[i:i + k] for i in range(len(s) - k + 1)}) for s in contigs]
    assert st["images_built_on_device"] == n_cells == cs.counters()["images_staged"]
    assert st["key_records_shipped"] == sum(distinct) == live_keys_staged(emu_engine, cs)
    assert st["table_bytes_built_on_device"] == sum(16 * table_slots(n) for n in distinct)
    for bc, s in enumerate(contigs):   # and the tables answer: the read that continues the contig extends it
        ret, _ = cs.cell(bc).add_read(s[5:] + "ACGTAC", "", 0, bc, 1, 0, 0.9)
        assert ret == 0, (bc, ret)
    cs.close()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/trust4 not shipped")
def test_barcode_driver_with_device_built_tables_matches_reference_binary(tmp_path):
    """`trust4-hip --barcode` on 4 000 synthetic pairs over 50 cells: _raw.out, _assembled_reads.fa and _final.out equal the
    reference binary's, and the run's statistics say the tables were built on the device"""
    import json
    stats = str(tmp_path / "stats.json")
    _barcode_case(tmp_path, _driver(), 4000, 50, 9, {"T4_THREADS": "8", "T4_STATS_JSON": stats})
    c = json.load(open(stats))["cells"]
    assert c["images_built_on_device"] == c["images_staged"] >= 50
    assert c["key_records_shipped"] > 0 and c["table_bytes_built_on_device"] >= 1024 * c["images_built_on_device"]
    assert c["bytes_staged"] > 16 * c["key_records_shipped"]
