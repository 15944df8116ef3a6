"""The two forms of a hit's sort key (seedChainPass: 32 bits when strand, contig id, diagonal and read offset fit, t4Key32Bits;
64 bits otherwise) at the set sizes and contig lengths where the form, or the width of one of its fields, changes -- with hits ON the
extremes of every field: the last contig id, contig 0 on the minus strand, the most negative and the most positive diagonal, the last
read offset (generators: keyform_gen.py, which asserts those extremes on the oracle's hits).

The form is chosen in three places that nothing ties together, and a wrong choice reports no error:
  - t4_index_commit walks the host sequences                      -> parts 1 and 2 (committed sets on every step; every sorter);
  - t4_index_apply_delta trusts the caller's max_seq_len          -> part 3 (a live image that crosses the steps both ways), part 4
    (the assembler's running maximum over its deltas, against the compiled reference's SeqSet), part 6 (negative control: an
    understated maximum does change an answer, on the emulator);
  - the per-cell images walk the staged records                   -> part 5 (a cell whose contig crosses a step between two rounds).
Every comparison is with the oracle and, when it was built, with the compiled reference; equality is exact. The emulator always
runs; `-m gpu` runs the same cases on the device."""
import filecmp
import functools
import os
import time

import numpy as np
import pytest

import keyform_gen as K
import t4check
import test_engine_emu as E
from t4libs import Ref, RefSeqSet
from test_query_edges import AIDS, TIER_CAP, check_add_query, check_overlap_path, checkers, landed, tiers, wide_reads


# The layout, stated once. It is used ONLY to assert that the cases below lie on both sides of every step; no result is checked against it.
def key_form(nseq, max_len):
    ib, cb = max(1, nseq.bit_length()), max(10, (max_len + 511).bit_length())     # 2^ib > nseq; 2^cb - 512 >= max_len
    return (ib, cb) if 1 + ib + cb + 9 <= 32 else None                            # None: the 64-bit form


def make_engine(emulated):
    if emulated:
        os.environ["T4_LIB"] = t4check.build_emulator_lib()
    else:
        os.environ.pop("T4_LIB", None)
    import trust4_amd
    return trust4_amd.Engine(0)


@pytest.fixture(params=[True, pytest.param(False, marks=pytest.mark.gpu)], ids=["emu", "gpu"])
def eng(request, monkeypatch):
    for a in AIDS:      # the real capacities and thresholds: no testing aid that moves one
        monkeypatch.delenv(a, raising=False)
    e = make_engine(request.param)
    e.emulated = request.param
    yield e
    e.close()
    os.environ.pop("T4_LIB", None)


def check_queries(eng, ix, es, reads, add_query=True, hits=False):
    """t4_overlaps (skip_repeats 0 and 1), t4_assign, t4_assign_strands, and t4_add_query with its ExtendOverlap results (and t4_hits
    when asked) against every checker -> the overlap counts"""
    chk = checkers(es)
    b = eng.upload(reads)
    if hits:
        off, h = ix.hits(b, 0, 0)
        assert t4check.check_hits(off, h, reads, es.o) == []
    for sk in (0, 1):
        cnt, ov = ix.overlaps(b, 0, sk, 128)
        for o in chk:
            assert t4check.check_overlaps(cnt, ov, reads, o, skip_repeats=sk) == [], sk
        if sk == 0:
            cnt0 = cnt
    strands = np.array([(0, 1, -1)[i % 3] for i in range(len(reads))], dtype=np.int32)
    aret, aout = ix.assign(b, 0)
    sret, sout = ix.assign_strands(b, strands)
    for o in chk:
        for i, rd in enumerate(reads):
            eret, eout = o.assign_read(rd, 0, -1)
            assert int(aret[i]) == eret and (eret == -1 or tuple(aout[i].tolist()) == tuple(eout)), (i, eret, int(aret[i]))
            eret, eout = o.assign_read(rd, int(strands[i]), -1)
            assert int(sret[i]) == eret and (eret == -1 or tuple(sout[i].tolist()) == tuple(eout)), (i, int(strands[i]), eret, int(sret[i]))
    if add_query:
        w0 = wide_reads(eng)
        check_add_query(eng, ix, es, reads, strands.tolist())
        assert wide_reads(eng) == w0      # every probe is the query kernel's own
    return cnt0


# ---- 1. committed sets on every step ------------------------------------------------------------------------------------------
# (nseq, maxSeqLen) -> the form: (idxBits, cBits), None for 64 bits
GRID = [
    ((4095, 512), (12, 10)), ((4096, 512), None),
    ((2047, 1536), (11, 11)), ((2047, 1537), None), ((2048, 1536), None),
    ((1023, 3584), (10, 12)), ((1023, 3585), None),
    ((511, 7680), (9, 13)), ((511, 7681), None),
    ((1, 600), (1, 11)),
    ((3, 65024), (2, 16)), ((3, 65025), (2, 17)),
    ((1023, 512), (10, 10)), ((1024, 512), (11, 10)),
]
K17 = [(4095, 512), (2047, 1537), (3, 65025)]       # the same at k = 17: a hashed table (htab) in place of the direct one


def test_grid_lies_on_both_sides_of_every_step():
    forms = dict(GRID)
    for point, form in GRID:
        assert key_form(*point) == form, point
    # the 22 / 23 edge of idxBits + cBits: every 32-bit point of sum 22 has a 64-bit neighbour one contig or one base away
    for (n, l), form in GRID:
        if form and sum(form) == 22:
            assert [forms.get(p, 0) for p in ((n + 1, l), (n, l + 1))].count(None) >= 1, (n, l)
    # a step of either field inside the 32-bit form; the narrowest idx field; the widest diagonal field in use
    assert forms[(1023, 512)][0] + 1 == forms[(1024, 512)][0] and forms[(3, 65024)][1] + 1 == forms[(3, 65025)][1]
    assert forms[(1, 600)][0] == 1 and max(f[1] for f in forms.values() if f) == 17
    assert all(p in forms for p in K17) and {forms[p] is None for p in K17} == {True, False}
    for n, l in forms:      # every point sits exactly on a step: one contig less or one base less is another layout, or one more is
        assert len({key_form(n, l), key_form(n + 1, l), key_form(n, l + 1), key_form(max(n - 1, 1), l), key_form(n, l - 1)}) > 1 or n == 1, (n, l)


@pytest.mark.parametrize("k,point", [(9, p) for p, _ in GRID] + [(17, p) for p in K17], ids=lambda v: str(v).replace(" ", ""))
def test_committed_set_on_a_step(eng, k, point):
    t0 = time.time()
    nseq, max_len = point
    es, reads = K.key_form_set(k, nseq, max_len, 1000 * k + nseq + max_len)
    ix = es.commit(eng)
    assert ix.size() == nseq
    cnt = check_queries(eng, ix, es, reads)
    # (what the oracle said of the far-end copies, r150 and r384 and their reverse complements: they are answered)
    half = len(reads) // 2
    assert all(es.o.overlaps_from_read(reads[i])[0] >= 1 for i in (0, 1, half, half + 1)) and (cnt[[0, 1, half, half + 1]] >= 1).all()
    print("key form %s of (%d, %d) at k = %d: %d reads, %.2f s" % (key_form(nseq, max_len), nseq, max_len, k, len(reads), time.time() - t0))


def test_longest_reads_in_the_smallest_tier(eng):
    """what the (1, 600) point found: a read of more than 328 bases has more than 640 k-mer positions on its two strands, the seed
    stage keeps one word per position in the tier's overlap array, and the smallest tier's 64 records hold 640 -- the words beyond
    them fell on the neighbouring array, and the read's first hits were lost unless the read happened to leave the tier for another
    reason. Such a read is handed on to the next tier now: reads of 328 bases stay in the 1 024-hit tier, reads of 329 and 384 bases
    with as few hits are answered by the second."""
    es = K.KeySet(9, 12)
    r384 = es.random_seq(K.READ_MAX)
    es.add(es.random_seq(300) + r384)
    es.add(es.random_seq(20) + r384[40:200] + es.random_seq(20))
    es.mirror()
    reads = [r384[-328:], r384[-329:], r384[:329], r384]
    reads += [K.rc(r) for r in reads]
    assert all(es.hits(r) <= TIER_CAP[0] for r in reads)
    cnt = check_overlap_path(eng, es.commit(eng), reads, checkers(es), tiers((0, len(reads)), (1, sum(1 for r in reads if len(r) > 328))))
    assert cnt.tolist() == [2] * len(reads)
    assert [es.o.overlaps_from_read(r)[1][0][1:3] for r in reads[:4]] == [(0, 327), (0, 328), (0, 328), (0, 383)]


# ---- 2. both sorters of each form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseq", [2047, 4096])
def test_every_sorter_of_the_form(eng, nseq):
    """reads of 4 097 - 8 192 hits (LDS tier 4: bitonicSort32 / bitonicSortReg) and of more than 8 192 (global scratch) through
    t4_overlaps and t4_assign, a read of at most 3 072 hits through the AddRead query's LDS tier (bitonicSortRegLds), in a set of
    the 32-bit form and in one of the 64-bit form"""
    t0 = time.time()
    es, reads, counts = K.sorter_set(nseq, 500 + nseq)
    assert (key_form(nseq, es.max_len()) is None) == (nseq == 4096)
    ix = es.commit(eng)
    tier_of = lambda h: next((i for i, c in enumerate(TIER_CAP) if h <= c), 5)
    assert [tier_of(h) for h in counts] == [4, 5, 2], counts
    for rd, h in zip(reads, counts):
        cnt = check_overlap_path(eng, ix, [rd], checkers(es), tiers((tier_of(h), 1)))
        assert cnt[0] == es.o.overlaps_from_read(rd)[0] > 1
    b = eng.upload(reads)
    cnt, ov = ix.overlaps(b, 0, 1, 128)
    for o in checkers(es):
        assert t4check.check_overlaps(cnt, ov, reads, o, skip_repeats=1) == []
    w0 = wide_reads(eng)
    check_add_query(eng, ix, es, [reads[2], K.rc(reads[2])], [0, 0])
    assert wide_reads(eng) == w0
    print("sorters at nseq %d: hits %s, %.2f s" % (nseq, counts, time.time() - t0))


# ---- 3. a live image that crosses the steps (t4_index_apply_delta) -------------------------------------------------------------
def test_live_image_across_the_steps(eng):
    """one image: a first delta of about a megabyte (copy-engine path), then small ones (read out of the pinned staging buffer) that
    grow the last contig over 512 bases (cBits 10 -> 11), contig 0 to 1 700 (the 64-bit form), add contigs in two deltas with no
    query in between (the wait for the staging buffer) up to 2 048 (idxBits 11 -> 12), and take the long contigs back (the 32-bit
    form again, at 12 + 10 bits). After every step the probes of the changed contigs and of an untouched one are queried."""
    t0 = time.time()
    es = K.KeySet(9, 33)
    img = E.LiveImage(9)
    ix = eng.index(9).set_params(31, 10, 0.9)

    def put(seq):
        i = es.add(seq)
        assert img.add(es.contigs[i][0], seq, es.contigs[i][2]) == i
        return i

    def swap(i, seq):
        es.contigs[i] = (es.contigs[i][0], seq, es.weights(seq))
        img.replace(i, seq, es.contigs[i][2])

    def check(ids, form):
        assert key_form(len(es.contigs), es.max_len()) == form, (len(es.contigs), es.max_len())
        es.mirror()
        reads = [r for i in ids for r in K.end_probes(es, es.contigs[i][1])]
        cnt = check_queries(eng, ix, es, reads, add_query=False, hits=True)
        assert (cnt >= 1).sum() >= 2 * len(ids)      # (far-end copies at the least)

    for i in range(2040):
        put(es.random_seq(500 if i == 0 else 480 if i == 2039 else 450 if i == 1000 else es.rnd.randint(40, 100)))
    img.flush(ix)
    check([0, 1000, 2039], (11, 10))
    swap(2039, es.random_seq(700))
    img.flush(ix)
    check([2039, 1000], (11, 11))
    swap(0, es.random_seq(1700))
    img.flush(ix)
    check([0, 2039, 1000], None)
    for _ in range(6):
        put(es.random_seq(es.rnd.randint(40, 100)))
    put(es.random_seq(300))
    img.flush(ix)                    # 2 047 contigs ...
    put(es.random_seq(420))
    img.flush(ix)                    # ... and one more, with no query in between
    check([2046, 2047, 0, 1000], None)
    swap(0, es.random_seq(400))
    swap(2039, es.random_seq(512))
    img.flush(ix)
    check([0, 2039, 2047, 1000], (12, 10))
    print("live image across the steps: %.2f s" % (time.time() - t0))


# ---- 4. the assembler's running maximum over its deltas, against the compiled reference ----------------------------------------
needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libt4ref.so not built")


def play(asm, script, window=0, barcode=-1, base=0, log=None, span=None, pre=None):
    """the script's calls on a SeqSet-like object -> one log entry per step (contig ids less `base`)"""
    log = [] if log is None else log
    lo, hi = span or (0, len(script))
    for i in range(lo, hi):
        step = script[i]
        if step[0] == "new":
            log.append(("new", asm.input_novel_read(step[1], step[2], step[3], barcode) - base))
        elif step[0] == "add":
            if pre:
                pre(step[1])
            elif window and not asm.window_valid():
                nxt = [s[1] for s in script[i:] if s[0] == "add"][:window]
                asm.prefetch(nxt, [0] * len(nxt))
            ret, strand = asm.add_read(step[1], "", 0, barcode, 1, 0, 0.9)
            log.append(("add", ret - base if ret >= 0 else ret, strand))
        elif step[0] == "k":
            asm.change_kmer_length(step[1])
            log.append(step)
        elif step[0] == "shallow":
            asm.release_shallow_contigs(step[1])
            log.append(step)
        else:
            asm.update_all_consensus()
            log.append(step)
    return log


@functools.lru_cache(maxsize=None)
def grow_reference():
    """the reference's answers to the script of part 4, computed once: (script, log, Output bytes)"""
    import tempfile
    script, ends, lens = K.grow_case(4)
    ref = RefSeqSet(9)
    log = play(ref, script)
    with tempfile.TemporaryDirectory() as tmp:
        ref.output(os.path.join(tmp, "ref.out"))
        out = open(os.path.join(tmp, "ref.out"), "rb").read()
    # the case is what it sets out to be: contigs A and B are built and grow past 512 and 1 536 bases before contig C is touched, and
    # the exact copies of their far ends are added to them every time
    at_c = next(i for i, s in enumerate(script) if s[0] == "new" and s[1] == "C")
    assert [x for x in log[:at_c] if x[0] == "new"] == [("new", 0), ("new", 1)] and log[at_c] == ("new", 2)
    a_adds = sum(1 for s, x in zip(script[:at_c], log[:at_c]) if s[0] == "add" and x[1] == 0)
    b_adds = sum(1 for s, x in zip(script[:at_c], log[:at_c]) if s[0] == "add" and x[1] == 1)
    assert 150 + 60 * (a_adds - 1) == lens[0] > 512 and 150 + 60 * (b_adds - 1) == lens[1] > 1536, (a_adds, b_adds)
    assert all(log[pos][1] in (0, 1) for pos, kind in ends if kind in (0, 1)), [log[pos] for pos, kind in ends]
    assert script[at_c + 1][0] == "add" and log[at_c + 1][1] == 2 and (at_c + 2, 0) in ends
    # ... contig C is touched alone once more after ChangeKmerLength, and it is the one contig ReleaseShallowContigs drops
    at_k = script.index(("k", 11))
    assert script[at_k + 1][0] == "add" and log[at_k + 1][1] == 2 and (at_k + 2, 0) in ends
    assert ("shallow", 2) in script[at_k:] and out.count(b">") == 2
    return script, log, out


@pytest.mark.skipif(not RefSeqSet.shallow_available(), reason="oracle/_ref/libt4ref.so or libt4refshallow.so not built")
@pytest.mark.parametrize("mode", ["plain", "window8", "verify"])
def test_assembler_keeps_the_longest_contig_in_mind(eng, tmp_path, monkeypatch, mode):
    """the builder tells its image the longest contig as a running maximum over its deltas: contigs grow past 512 and past 1 536
    bases, then a round touches a third, short contig only, and the reads after it lie at the far ends of the long ones (and overhang
    them); the same after ChangeKmerLength (which starts the maximum afresh) and after ReleaseShallowContigs. Every return value and
    strand equals the reference SeqSet's, Output is byte-identical: without a window, with a window of 8, with every served entry
    queried again (T4_VERIFY_WINDOW)."""
    import trust4_amd
    t0 = time.time()
    script, log_ref, out_ref = grow_reference()
    if mode == "verify":
        monkeypatch.setenv("T4_VERIFY_WINDOW", "1")
    mine = trust4_amd.Assembler(eng, 9)
    log = play(mine, script, window=0 if mode == "plain" else 8)
    first = next((i for i, (a, b) in enumerate(zip(log_ref, log)) if a != b), None)
    assert first is None and len(log) == len(log_ref), (first, script[first][0], log_ref[first], log[first])
    if mode != "plain":
        assert mine.counters()["window_hits"] > 0
    mine.output(str(tmp_path / "mine.out"))
    assert open(str(tmp_path / "mine.out"), "rb").read() == out_ref
    mine.close()
    print("assembler (%s): %d calls, %.2f s" % (mode, len(script), time.time() - t0))


# ---- 5. a cell's image across a step (t4_cellset_*) ---------------------------------------------------------------------------
@needs_ref
def test_cell_image_across_a_step(eng, tmp_path):
    """barcode mode: a cell whose second contig grows from 450 to 750 bases between two rounds (its image is staged anew: cBits 10 ->
    11) beside a cell that stays small, then a cell of 513 contigs whose last one has 7 681 bases (the 64-bit form); reads at the
    far ends and overhanging them. One reference SeqSet keyed by barcode, walked cell after cell."""
    import trust4_amd
    t0 = time.time()
    cells, ends = K.cell_case(5)
    ref = RefSeqSet(9, 13, consider_barcode=True)
    log_ref = {}
    for bc in sorted(cells):
        log_ref[bc] = play(ref, cells[bc], barcode=bc, base=ref.size())
    ref.update_all_consensus()
    for bc, lst in ends.items():       # the reference puts the copies of the far end on the long contig (the cell's last but for cell 0's)
        assert all(log_ref[bc][pos][1] == (1 if bc == 0 else 512) for pos, kind in lst if kind in (0, 1)), (bc, [log_ref[bc][pos] for pos, _ in lst])
    assert key_form(2, 450) == (2, 10) and key_form(2, 750) == (2, 11) and key_form(513, 7681) is None
    cs = trust4_amd.CellSet(eng, 9, 13)
    log = {bc: [] for bc in cells}
    at = {bc: 0 for bc in cells}
    for active in ([0, 1], [2]):
        while any(at[bc] < len(cells[bc]) for bc in active):
            todo = [bc for bc in active if at[bc] < len(cells[bc])]
            adds = [bc for bc in todo if cells[bc][at[bc]][0] == "add"]
            if adds:       # one round: the cells' next reads are queried together, each against its own image
                cs.prefetch(adds, [cells[bc][at[bc]][1] for bc in adds], [0] * len(adds))
            for bc in todo:
                play(cs.cell(bc), cells[bc], barcode=bc, log=log[bc], span=(at[bc], at[bc] + 1), pre=lambda rd: None)
                at[bc] += 1
        for bc in active:
            cs.close_cell(bc)
    cs.update_all_consensus()
    for bc in cells:
        first = next((i for i, (a, b) in enumerate(zip(log_ref[bc], log[bc])) if a != b), None)
        assert first is None and len(log[bc]) == len(log_ref[bc]), (bc, first, log_ref[bc][first], log[bc][first])
    assert ref.size() == cs.size()
    names = ["BC%03d" % i for i in range(len(cells))]
    pa, pb = str(tmp_path / "ref.out"), str(tmp_path / "mine.out")
    ref.output_barcodes(pa, names)
    cs.output(pb, names)
    assert filecmp.cmp(pa, pb, shallow=False)
    cs.close()
    print("cell images across a step: %.2f s" % (time.time() - t0))


# ---- 6. negative control, emulator only: an understated maximum does change an answer ------------------------------------------
def test_understated_maximum_is_visible(monkeypatch):
    """the evidence that parts 3 to 5 can see a stale maximum: 40 contigs at k = 9, contig 39 of 700 bases ending in a 150-base read;
    told max_seq_len = 512 the image mis-sorts that read's hits and t4_overlaps differs from the oracle; told 700 it agrees.
    Emulator only, this shape only (a mis-decoded key may name an offset outside its contig)."""
    for a in AIDS:
        monkeypatch.delenv(a, raising=False)
    eng = make_engine(True)
    try:
        es = K.KeySet(9, 6)
        img = E.LiveImage(9)
        ix = eng.index(9).set_params(31, 10, 0.9)
        rd = es.random_seq(150)
        for i in range(40):
            es.add(es.random_seq(60) if i < 39 else es.random_seq(550) + rd)
            img.add(*es.contigs[i])
        es.mirror()
        assert es.o.overlaps_from_read(rd)[0] == 1 and es.o.assign_read(rd, 0, -1)[0] == 39
        b = eng.upload([rd])
        img.flush(ix, max_seq_len=512)
        cnt, ov = ix.overlaps(b, 0, 0, 128)
        assert t4check.check_overlaps(cnt, ov, [rd], es.o) != []
        img.flush(ix, max_seq_len=700)
        cnt, ov = ix.overlaps(b, 0, 0, 128)
        assert t4check.check_overlaps(cnt, ov, [rd], es.o) == [] and cnt[0] == 1
        assert int(ix.assign(b, 0)[0][0]) == 39
    finally:
        eng.close()
        os.environ.pop("T4_LIB", None)
