"""Barcode mode with the cells' k-mer index built on the device from the contigs (t4_cellset in the indexed image form): the
lock-step walk of tests/test_cell_images_e2e.py against ONE unmodified reference SeqSet, with every staged image's counts held
against the host's own index (T4_TEST_IMAGE_CROSSCHECK, test builds only) and against the same walk in the compact form; one cell
driven by hand through InputNovelRead, extensions, ChangeKmerLength and further adds beside a twin in the compact form; and, on
the GPU, `trust4-hip --barcode` with T4_CELL_IMAGES=indexed against the reference binary, byte for byte."""
import filecmp
import json
import os
import random

import pytest

import t4check
from t4libs import Ref
from test_cellset_emu import CellWalk, annotate, make_cells, run_cellset, run_reference
from test_stage1_e2e import REF_BIN, _barcode_case, _driver


@pytest.fixture(scope="module")
def emu_engine():
    os.environ["T4_LIB"] = t4check.build_emulator_lib()
    import trust4_amd
    eng = trust4_amd.Engine(0)
    yield eng
    eng.close()
    os.environ.pop("T4_LIB", None)


def run_cellset_indexed(eng, cells, names, thr, k, release, lanes, window):
    """test_cellset_emu.run_cellset with the cell set in the indexed form"""
    import trust4_amd
    cs = trust4_amd.CellSet(eng, k, 13)
    cs.set_image_form("indexed")
    walks = [CellWalk(bc, reads, names[bc], thr[bc]) for bc, reads in enumerate(cells)]
    todo = list(range(len(cells)))
    active = []
    while todo or active:
        while todo and len(active) < lanes:
            active.append(todo.pop(0))
        bcs, rds = [], []
        for bc in active:
            for rd in walks[bc].upcoming(window):
                bcs.append(bc)
                rds.append(rd)
        cs.prefetch(bcs, rds, [0] * len(rds))
        for bc in list(active):
            w = walks[bc]
            for _ in range(window):
                if not w.done():
                    w.step(cs.cell(bc), 0)
            if w.done():
                if bc in release:
                    cs.cell(bc).release_finished_barcode(bc)
                cs.close_cell(bc)
                active.remove(bc)
    cs.update_all_consensus()
    return cs, [w.log for w in walks]


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libt4ref.so not built")
def test_cells_indexed_on_the_device_match_reference(emu_engine, tmp_path, monkeypatch):
    monkeypatch.setenv("T4_TEST_IMAGE_CROSSCHECK", "1")
    k, n_cells = 9, 30
    cells = make_cells(11, n_cells, 6)
    names, thr = annotate(cells, 11)
    release = {2, 17}
    ref, log_ref = run_reference(cells, names, thr, k, release)
    cs, log_mine = run_cellset_indexed(emu_engine, cells, names, thr, k, release, 8, 2)
    for bc in range(n_cells):
        assert log_ref[bc] == log_mine[bc], bc
    assert ref.size() == cs.size()
    bnames = ["BC%03d" % i for i in range(n_cells)]
    pa, pb = str(tmp_path / "ref.out"), str(tmp_path / "mine.out")
    ref.output_barcodes(pa, bnames)
    cs.output(pb, bnames)
    assert filecmp.cmp(pa, pb, shallow=False)
    assert sum(1 for l in log_ref for x in l if x[0] == "add" and x[1] >= 0) > 30
    c, st, ix = cs.counters(), cs.image_stats(), cs.indexed_stats()
    assert c["images_staged"] >= n_cells
    assert ix["images_indexed_on_device"] == c["images_staged"] == ix["images_crosschecked"]
    assert ix["cells_fallen_back_to_compact"] == 0 and ix["postings_built_on_device"] > 0
    assert st["key_records_shipped"] == 0 and st["images_built_on_device"] == 0
    assert st["bytes_staged"] == c["bytes_staged"]
    # the same walk in the compact form ships more
    monkeypatch.delenv("T4_TEST_IMAGE_CROSSCHECK")
    cs2, log_compact = run_cellset(emu_engine, cells, names, thr, k, release, 8, 2)
    assert log_compact == log_mine
    c2 = cs2.counters()
    assert c2["images_staged"] == c["images_staged"] and cs2.indexed_stats()["images_indexed_on_device"] == 0
    assert c["bytes_staged"] < c2["bytes_staged"]
    cs.close()
    cs2.close()


def test_image_form_is_set_before_the_first_prefetch(emu_engine, monkeypatch):
    """... and may be set after a cell got its first contig: the counts, kept only in the indexed form, are then taken from the index"""
    import trust4_amd
    monkeypatch.setenv("T4_TEST_IMAGE_CROSSCHECK", "1")
    cs = trust4_amd.CellSet(emu_engine, 9, 13)
    with pytest.raises(trust4_amd.api.T4Error):
        cs.set_image_form(7)
    s = "ACGTTGCAAGGCTTAACCGGATTACAGGCATCGATCGGATCAAGT"
    assert cs.cell(0).input_novel_read("Novel", s, 1, 0) == 0
    cs.set_image_form("indexed")
    cs.set_image_form("compact")
    cs.set_image_form("indexed")
    assert cs.cell(1).input_novel_read("Novel", s[::-1], 1, 1) == 0
    cs.prefetch([0, 1], [s[5:] + "ACGTAC", s[::-1][4:] + "TTGACA"], [0, 0])
    with pytest.raises(trust4_amd.api.T4Error):
        cs.set_image_form("compact")
    ix = cs.indexed_stats()
    assert ix["images_indexed_on_device"] == ix["images_crosschecked"] == 2
    assert cs.cell(0).add_read(s[5:] + "ACGTAC", "", 0, 0, 1, 0, 0.9)[0] == 0
    cs.close()


def test_one_cell_by_hand_beside_a_compact_twin(emu_engine, tmp_path, monkeypatch):
    """InputNovelRead, adds that extend to the right and to the left (every posting of the contig moves) and one that joins two
    contigs, ChangeKmerLength (the index and the counts are rebuilt; the cell store keeps its k, so the same k), then further
    adds: after every add the indexed cell answers as its twin in the compact form does, and every image's counts equal the index"""
    import trust4_amd
    monkeypatch.setenv("T4_TEST_IMAGE_CROSSCHECK", "1")
    rnd = random.Random(77)
    t = "".join(rnd.choice("ACGT") for _ in range(420))
    twins = [trust4_amd.CellSet(emu_engine, 9, 13) for _ in range(2)]
    twins[0].set_image_form("indexed")
    for cs in twins:
        assert cs.cell(0).input_novel_read("Novel", t[100:200], 1, 0) == 0
        assert cs.cell(0).input_novel_read("Novel", t[260:360], 1, 0) == 1

    def add(read):
        got = []
        for cs in twins:
            cs.prefetch([0], [read], [0])
            got.append(cs.cell(0).add_read(read, "", 0, 0, 1, 0, 0.9))
        assert got[0] == got[1], read
        return got[0][0]

    def outputs_equal():
        paths = [str(tmp_path / ("twin%d.out" % i)) for i in range(2)]
        for cs, p in zip(twins, paths):
            cs.output(p, ["BC0"])
        return filecmp.cmp(paths[0], paths[1], shallow=False)

    rets = [add(t[150:250])]           # extends contig 0 to the right
    rets.append(add(t[60:160]))        # ... and to the left: its postings shift
    rets.append(add(t[300:400]))       # extends contig 1
    rets.append(add(t[190:320]))       # reaches from contig 0 into contig 1
    rets.append(add(t[100:200]))       # inside
    assert rets[0] == 0 and rets[1] == 0 and rets[2] == 1 and all(r >= 0 for r in rets), rets
    assert outputs_equal()
    for cs in twins:
        cs.cell(0).change_kmer_length(9)
    rets2 = [add(t[20:110]), add(t[330:420]), add(t[150:260])]
    assert all(r >= 0 for r in rets2), rets2
    assert outputs_equal()
    ix = twins[0].indexed_stats()
    n_adds = len(rets) + len(rets2)
    assert ix["images_indexed_on_device"] == ix["images_crosschecked"] == twins[0].counters()["images_staged"] >= 2
    assert ix["images_indexed_on_device"] <= n_adds and ix["cells_fallen_back_to_compact"] == 0
    assert twins[0].image_stats()["key_records_shipped"] == 0 < twins[1].image_stats()["key_records_shipped"]
    for cs in twins:
        cs.close()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/trust4 not shipped")
def test_barcode_driver_with_indexed_images_matches_reference_binary(tmp_path):
    """`trust4-hip --barcode` on 4 000 synthetic pairs over 50 cells with T4_CELL_IMAGES=indexed: _raw.out, _assembled_reads.fa and
    _final.out equal the reference binary's, and the run's statistics say every image's index was built on the device"""
    stats = str(tmp_path / "stats.json")
    _barcode_case(tmp_path, _driver(), 4000, 50, 9, {"T4_THREADS": "8", "T4_STATS_JSON": stats, "T4_CELL_IMAGES": "indexed"})
    c = json.load(open(stats))["cells"]
    assert c["image_form"] == "indexed"
    assert c["images_indexed_on_device"] == c["images_staged"] >= 50
    assert c["key_records_shipped"] == 0 and c["images_built_on_device"] == 0
    assert c["postings_built_on_device"] > 0 and 0 < c["count_bytes_shipped"] < c["bytes_staged"]
