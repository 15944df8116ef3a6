"""Barcode mode with the cells' images resident on the device (t4_cellset in the resident image form): the lock-step walk of
tests/test_cellset_emu.py against ONE unmodified reference SeqSet -- return codes and strands per read, Output byte for byte -- with
windows of 1 and 4 reads, so that a cell's image is brought up to date by deltas many times while the cell is open; the same walk
with every staged image's counts held against the host's index (T4_TEST_IMAGE_CROSSCHECK, test builds only); and one cell set whose
form is chosen after its cells got contigs, beside a twin in the compact form. On the emulator build and, marked gpu, on the device."""
import filecmp
import os
import random

import pytest

import t4check
from t4libs import Ref
from test_cellset_emu import CellWalk, annotate, make_cells, run_cellset, run_reference


@pytest.fixture(scope="module", params=[True, pytest.param(False, marks=pytest.mark.gpu)], ids=["emu", "gpu"])
def eng(request):
    if request.param:
        os.environ["T4_LIB"] = t4check.build_emulator_lib()
    else:
        os.environ.pop("T4_LIB", None)
    import trust4_amd
    e = trust4_amd.Engine(0)
    e.emulated = request.param
    yield e
    e.close()
    os.environ.pop("T4_LIB", None)


def run_cellset_in_form(eng, form, cells, names, thr, k, release, lanes, window):
    """test_cellset_emu.run_cellset with the cell set in the given image form"""
    import trust4_amd
    cs = trust4_amd.CellSet(eng, k, 13)
    cs.set_image_form(form)
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


@pytest.fixture(scope="module")
def case():
    """12 cells of about 40 reads (50 to 150 bases; both ends extended, merges, consensus flips, adjacent duplicates, reads with an N);
    cell 5 releases its shallow contigs when it is done. The reference's walk is computed once."""
    k = 9
    cells = make_cells(23, 12, 22)
    names, thr = annotate(cells, 23)
    release = {5, 9}
    ref, log_ref = run_reference(cells, names, thr, k, release)
    assert 35 <= min(len(c) for c in cells) and sum(1 for l in log_ref for x in l if x[0] == "add" and x[1] >= 0) > 60
    return k, cells, names, thr, release, ref, log_ref


def walk_and_check(eng, case, tmp_path, window, crosscheck):
    k, cells, names, thr, release, ref, log_ref = case
    cs, log_mine = run_cellset_in_form(eng, "resident", cells, names, thr, k, release, 4, window)
    for bc in range(len(cells)):
        first = next((i for i, (a, b) in enumerate(zip(log_ref[bc], log_mine[bc])) if a != b), None)
        assert first is None and len(log_ref[bc]) == len(log_mine[bc]), (bc, first, log_ref[bc][first or 0], log_mine[bc][first or 0])
    assert ref.size() == cs.size()
    bnames = ["BC%03d" % i for i in range(len(cells))]
    pa, pb = str(tmp_path / "ref.out"), str(tmp_path / "mine.out")
    ref.output_barcodes(pa, bnames)
    cs.output(pb, bnames)
    assert filecmp.cmp(pa, pb, shallow=False)
    c, rs, ix, st = cs.counters(), cs.resident_stats(), cs.indexed_stats(), cs.image_stats()
    assert rs["images_resident_whole"] >= len(cells) and rs["deltas"] > len(cells)
    assert rs["images_resident_whole"] + rs["deltas"] == c["images_staged"]
    assert rs["deltas_sent_back"] == 0 and rs["cells_fallen_back_to_compact"] == 0
    assert rs["delta_contigs_shipped"] >= rs["deltas"] and rs["postings_rebuilt_on_device"] > 0
    assert ix["images_indexed_on_device"] == 0 and st["images_built_on_device"] == 0 and st["key_records_shipped"] == 0
    assert ix["images_crosschecked"] == (c["images_staged"] if crosscheck else 0)
    cs.close()


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libt4ref.so not built")
@pytest.mark.parametrize("window", [1, 4])
def test_resident_cells_match_reference(eng, case, tmp_path, window):
    walk_and_check(eng, case, tmp_path, window, False)


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libt4ref.so not built")
@pytest.mark.parametrize("window", [1, 4])
def test_resident_cells_match_reference_and_their_counts_match_the_index(case, tmp_path, monkeypatch, window):
    """emulator build only (the shadow check is compiled into test builds): every staged image's counts and total against the index"""
    monkeypatch.setenv("T4_LIB", t4check.build_emulator_lib())
    monkeypatch.setenv("T4_TEST_IMAGE_CROSSCHECK", "1")
    import trust4_amd
    e = trust4_amd.Engine(0)
    try:
        walk_and_check(e, case, tmp_path, window, True)
    finally:
        e.close()


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libt4ref.so not built")
def test_resident_deltas_ship_less_than_the_other_forms(eng, case):
    k, cells, names, thr, release, _, log_ref = case
    staged = {}
    for form in ("compact", "indexed", "resident"):
        cs, log = run_cellset_in_form(eng, form, cells, names, thr, k, release, 4, 1)
        assert log == log_ref
        staged[form] = cs.counters()["bytes_staged"]
        cs.close()
    assert staged["resident"] < staged["indexed"] < staged["compact"], staged


def test_form_chosen_late_and_set_back(eng, tmp_path, monkeypatch):
    """the form is chosen after the cells got their first contigs (the counts are then taken from the index, once), set back to
    compact and chosen again before the first prefetch; then extensions to both sides, a join of two contigs, ChangeKmerLength (the
    contigs are renumbered: a whole image) and more adds, each answered as a twin in the compact form answers, Output equal"""
    import trust4_amd
    if eng.emulated:
        monkeypatch.setenv("T4_TEST_IMAGE_CROSSCHECK", "1")
    rnd = random.Random(78)
    t = "".join(rnd.choice("ACGT") for _ in range(420))
    twins = [trust4_amd.CellSet(eng, 9, 13) for _ in range(2)]
    for cs in twins:
        assert cs.cell(0).input_novel_read("Novel", t[100:200], 1, 0) == 0
        assert cs.cell(0).input_novel_read("Novel", t[260:360], 1, 0) == 1
    with pytest.raises(trust4_amd.api.T4Error):
        twins[0].set_image_form(3)
    twins[0].set_image_form("resident")
    twins[0].set_image_form("compact")
    twins[0].set_image_form("resident")

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

    rets = [add(t[150:250]), add(t[60:160]), add(t[300:400]), add(t[190:320]), add(t[100:200])]
    assert rets[0] == 0 and rets[1] == 0 and rets[2] == 1 and all(r >= 0 for r in rets), rets
    with pytest.raises(trust4_amd.api.T4Error):
        twins[0].set_image_form("compact")   # not after the first prefetch
    assert outputs_equal()
    before = twins[0].resident_stats()
    assert before["images_resident_whole"] >= 1 and before["deltas"] >= 3   # (the join outgrows a stretch: whole again)
    for cs in twins:
        cs.cell(0).change_kmer_length(9)
    rets2 = [add(t[20:110]), add(t[330:420]), add(t[150:260])]
    assert all(r >= 0 for r in rets2), rets2
    assert outputs_equal()
    rs = twins[0].resident_stats()
    assert rs["images_resident_whole"] > before["images_resident_whole"] and rs["whole_restages"] == rs["images_resident_whole"] - 1 and rs["deltas"] > before["deltas"]
    assert rs["images_resident_whole"] + rs["deltas"] == twins[0].counters()["images_staged"]
    if eng.emulated:
        assert twins[0].indexed_stats()["images_crosschecked"] == twins[0].counters()["images_staged"]
    assert twins[0].counters()["bytes_staged"] < twins[1].counters()["bytes_staged"]
    for cs in twins:
        cs.close()


def test_count_of_256_sends_the_cell_to_the_compact_form_for_good(tmp_path, monkeypatch):
    """emulator build only (t4_assembler_test_index_again is compiled into test builds: nothing else reaches 256 equal postings in a
    few calls). Contig 0 of a resident cell is indexed 254 more times: every count is 255, the cell stays resident (whole once: the
    table is outgrown; then a delta). Once more: 256. From then on every image of the cell is compact, no delta and no resident image follows, the cell is
    counted once, and every add is answered as a twin in the compact form answers, Output equal."""
    import ctypes as C
    monkeypatch.setenv("T4_LIB", t4check.build_emulator_lib())
    monkeypatch.setenv("T4_TEST_IMAGE_CROSSCHECK", "1")
    import trust4_amd
    e = trust4_amd.Engine(0)
    again = e.lib.t4_assembler_test_index_again
    again.restype, again.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int]
    rnd = random.Random(79)
    t = "".join(rnd.choice("ACGT") for _ in range(600))
    twins = [trust4_amd.CellSet(e, 9, 13) for _ in range(2)]
    twins[0].set_image_form("resident")
    try:
        for cs in twins:
            assert cs.cell(0).input_novel_read("Novel", t[0:40], 1, 0) == 0        # the contig that is indexed again: 32 offsets
            assert cs.cell(0).input_novel_read("Novel", t[200:300], 1, 0) == 1     # the contig the reads extend

        def add(read):
            got = []
            for cs in twins:
                cs.prefetch([0], [read], [0])
                got.append(cs.cell(0).add_read(read, "", 0, 0, 1, 0, 0.9))
            assert got[0] == got[1], read
            return got[0][0]

        def index_again(times):
            for cs in twins:
                e.check(again(cs.cell(0).h, 0, times))

        assert add(t[250:350]) == 1                        # the first image: whole
        index_again(254)                                   # 255 at every offset of contig 0
        assert add(t[180:280]) == 1                        # whole again (8 128 more postings outgrow the table), still resident
        assert add(t[320:400]) == 1                        # ... and the next change is a delta
        rs = twins[0].resident_stats()
        assert rs["cells_fallen_back_to_compact"] == 0 and rs["deltas"] == 1 and rs["images_resident_whole"] == 2
        assert twins[0].image_stats()["images_built_on_device"] == 0 and twins[0].counters()["images_staged"] == 3
        index_again(1)                                     # 256
        rets = [add(t[380:470]), add(t[140:240]), add(t[5:40] + "ACGTTGCA"), add(t[440:540])]
        assert all(r >= 0 for r in rets), rets
        after = twins[0].resident_stats()
        assert after["cells_fallen_back_to_compact"] == 1
        assert (after["deltas"], after["images_resident_whole"], after["whole_restages"]) == (rs["deltas"], rs["images_resident_whole"], rs["whole_restages"])
        c = twins[0].counters()
        assert twins[0].image_stats()["images_built_on_device"] == c["images_staged"] - 3 >= 3   # every later image is compact
        assert twins[0].indexed_stats()["images_crosschecked"] == 3                               # (only the resident images are held against the index)
        paths = [str(tmp_path / ("twin%d.out" % i)) for i in range(2)]
        for cs, p in zip(twins, paths):
            cs.output(p, ["BC0"])
        assert filecmp.cmp(paths[0], paths[1], shallow=False)
    finally:
        for cs in twins:
            cs.close()
        e.close()
