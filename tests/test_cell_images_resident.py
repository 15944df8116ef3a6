"""Per-barcode set images that stay in their arena slot (the resident form: t4_cellstore_stage_delta, cellDeltaApplyKernel, then
cellIndexBuildKernel reading the slot) against the images the host writes in full (t4_cellstore_stage, the yardstick). A synthetic
cell is a set of contigs plus one count byte per offset; it goes into slot R whole, then every change of the host state travels
to R as a delta -- the touched contigs only -- while a second slot Y takes the whole new state through t4_cellstore_stage. Both are
read back (t4_cellstore_read_image) and compared:
  per contig   name, gene type, barcode, length, consensus with its terminator, predicate bytes with the terminator's;
  the view     every scalar but the table's mask (R's table is sized from npost, Y's from the distinct keys);
  the index    as a map: (c) every key's sorted postings are the same in R, in Y and in the host state, (d) R's lists tile
               [0, npost) exactly once, (e) every key of R is reachable from its home slot, every other slot is (~0, 0, 0);
  queries      counts, ov, ext, ext_ret of six reads against R and against Y, byte for byte.
On the emulator build of the kernels and, marked gpu, through libt4hip.so."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import t4check
from test_cell_images import M64, View, mix64, table_slots
from test_cell_images_indexed import FullView, ICell, IStore, check_pair, code_of, lists_of, mutate, rand_seq

T4_ERR_ARG = -1
T4_CELL_DELTA_WHOLE = 1
SEQ = np.dtype([("consOff", "<i4"), ("len", "<i4"), ("pwOff", "<i4"), ("barcode", "<i4"), ("isRef", "u1"), ("geneType", "u1"),
                ("name", "u1", 4), ("pad", "<u2")])   # T4SeqInfo
assert SEQ.itemsize == 24


def al16(x):
    return (x + 15) & ~15


def marks(s, k):
    """the counts BuildIndexFromRead leaves: one posting per offset with a whole ACGT k-mer that differs from the k-mer before it"""
    out = []
    for o in range(max(0, len(s) - k + 1)):
        km = s[o:o + k]
        out.append(0 if set(km) - set("ACGT") or (o > 0 and km == s[o - 1:o - 1 + k]) else 1)
    return out


class RCell:
    """the host state of one cell: names, consensus, posWeight counts, posting counts"""

    def __init__(self, rnd, barcode, cons, k):
        self.rnd, self.barcode, self.k = rnd, barcode, k
        self.cons, self.names, self.pw, self.counts = [], [], [], []
        for s in cons:
            self.add(s)

    nseq = property(lambda self: len(self.cons))
    npost = property(lambda self: int(sum(int(np.sum(c)) for c in self.counts)))

    def _pw(self, s):
        return np.array([self.rnd.randrange(0, 6) for _ in range(4 * len(s))], dtype=np.int32)

    def set(self, i, s, name=None):
        self.cons[i], self.pw[i], self.counts[i] = s, self._pw(s), np.array(marks(s, self.k), dtype=np.uint8)
        if name is not None:
            self.names[i] = name
        return [i]

    def add(self, s, name=None):
        self.cons.append(""), self.names.append(""), self.pw.append(None), self.counts.append(None)
        return self.set(self.nseq - 1, s, (["IGHV", "TRBC", "IGKJ", "Novel"][(self.nseq - 1) % 4]) if name is None else name)

    def release(self, i):
        return self.set(i, "", "")

    def icell(self):
        """the same state as the yardstick's helpers want it: the index derived from the counts"""
        c = ICell(self.rnd, self.barcode, self.cons, [x.tolist() for x in self.counts], k=self.k)
        c.names, c.pw = list(self.names), list(self.pw)
        return c

    def lens(self, ids=None):
        return [len(self.cons[i]) for i in (range(self.nseq) if ids is None else ids)]


class RStore(IStore):
    def __init__(self, eng, k=9):
        super().__init__(eng, k)
        P, I, L, Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
        for name, res, args in (("t4_cellstore_stage_delta", I, [P, I, I, I, I, P, P, P, P, P, P, L, P]),
                                ("t4_cellstore_resident_image_bytes", Z, [I, P]), ("t4_cellstore_delta_fits", I, [P, I, I, I, P, P, L]),
                                ("t4_cellstore_resident_stats", I, [P, P]), ("t4_cellstore_bytes_staged", L, [P]),
                                ("t4_cellstore_patch", I, [P, I, I, P, P])):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args

    def resident_bytes(self, lens):
        a = np.array(lens, dtype=np.int32)
        return self.lib.t4_cellstore_resident_image_bytes(len(lens), a.ctypes.data if len(lens) else None)

    def reserve_for(self, max_slot, cell, full=True):
        need = self.resident_bytes(cell.lens())
        if full:
            need += self.lib.t4_cellstore_full_image_bytes(*cell.icell().sizes())
        self.eng.check(self.lib.t4_cellstore_prepare(self.h, max_slot, need))

    def stage_delta_rc(self, slot, cell, touched=None, npost=None, ids=None):
        """touched None: the whole image. ids: what is passed as touched_ids (default: touched)"""
        given = list(range(cell.nseq)) if touched is None else list(touched)
        n = len(given)
        names = (C.c_char_p * n)(*[cell.names[i].encode() for i in given])
        cons = (C.c_char_p * n)(*[cell.cons[i].encode() for i in given])
        pw = (C.c_void_p * n)(*[cell.pw[i].ctypes.data if len(cell.pw[i]) else None for i in given])
        cnt = (C.c_void_p * n)(*[cell.counts[i].ctypes.data if len(cell.counts[i]) else None for i in given])
        lens = np.array([len(cell.counts[i]) for i in given], dtype=np.int32)
        tid = np.array(given if ids is None else ids, dtype=np.int32)
        o_pw = np.full(max(cell.nseq, 1), -1, dtype=np.int64)
        rc = self.lib.t4_cellstore_stage_delta(self.h, slot, cell.barcode, cell.nseq, -1 if touched is None else n, tid.ctypes.data,
                                               C.cast(names, C.c_void_p), C.cast(cons, C.c_void_p), C.cast(pw, C.c_void_p), C.cast(cnt, C.c_void_p),
                                               lens.ctypes.data, cell.npost if npost is None else npost, o_pw.ctypes.data)
        return rc, o_pw

    def stage_whole(self, slot, cell):
        rc, o = self.stage_delta_rc(slot, cell)
        self.eng.check(rc)
        return o

    def stage_delta(self, slot, cell, touched):
        rc, o = self.stage_delta_rc(slot, cell, touched)
        self.eng.check(rc)
        return o

    def rstats(self):
        v = (C.c_int64 * 7)()
        self.eng.check(self.lib.t4_cellstore_resident_stats(self.h, C.cast(v, C.c_void_p)))
        return dict(zip(("whole", "deltas", "delta_contigs", "sent_back", "restages", "postings", "table_bytes"), v))

    def bytes_staged(self):
        return self.lib.t4_cellstore_bytes_staged(self.h)

    def err(self):
        return self.lib.t4_last_error(self.eng.h).decode()


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


@pytest.fixture
def store(eng):
    s = RStore(eng)
    yield s
    s.close()


def records(img, view):
    o = view.seqs - view.ctab
    return np.frombuffer(img[o:o + 24 * view.nseq].tobytes(), dtype=SEQ)


def contigs_of(img, view):
    """per contig what a query can see of it: (name, gene type, barcode, isRef, length, consensus + terminator, predicate bytes + terminator's)"""
    o_cons, o_pw = view.cons - view.ctab, view.pw - view.ctab
    out = []
    for r in records(img, view):
        n = int(r["len"]) + 1
        out.append((bytes(r["name"]), int(r["geneType"]), int(r["barcode"]), int(r["isRef"]), int(r["len"]),
                    bytes(img[o_cons + r["consOff"]:o_cons + r["consOff"] + n]), bytes(img[o_pw + r["pwOff"]:o_pw + r["pwOff"] + n])))
    return out


def check_equal(cell, resident, full):
    (img_r, vr), (img_y, vy) = resident, full
    ic = cell.icell()
    for f in View.SCALARS:
        if f != "hashMask":
            assert getattr(vr, f) == getattr(vy, f), f
    assert vr.nseq == cell.nseq and vr.ctab % 16 == 0
    cr, cy = contigs_of(img_r, vr), contigs_of(img_y, vy)
    assert cr == cy
    assert [c[4] for c in cr] == cell.lens() and [c[5] for c in cr] == [s.encode() + b"\0" for s in cell.cons]
    lr, mr, tr = lists_of(img_r, vr)
    ly, _, _ = lists_of(img_y, vy)
    want = {c: sorted(v) for c, v in ic.lists.items()}
    assert lr == ly == want                                                # (c), and (b)'s {code: cnt}
    at = 0
    for st, n in sorted(mr.values()):                                      # (d)
        assert st == at and n > 0
        at += n
    assert at == cell.npost and vr.seqs - vr.post >= 8 * cell.npost
    assert len(tr) >= table_slots(cell.npost) >= table_slots(len(want))    # the table serves npost keys at a load of 2/3
    mask, codes = len(tr) - 1, tr["code"]
    for c in want:                                                         # (e)
        s = mix64(c) & mask
        for _ in range(len(tr)):
            assert codes[s] != M64, "key %d behind an empty slot" % c
            if codes[s] == c:
                break
            s = (s + 1) & mask
        else:
            raise AssertionError("key %d not found" % c)
    empty = tr[codes == M64]
    assert len(empty) == len(tr) - len(want) and not empty["start"].any() and not empty["cnt"].any()
    return len(tr)


def reads_of(rnd, cell, n=6):
    out = []
    src = [s for s in cell.cons if len(s) >= 40 and "N" not in s] or ["ACGT" * 12]
    for j in range(n):
        s = src[j % len(src)]
        m = min(len(s), rnd.randrange(36, 56))
        at = rnd.randrange(0, len(s) - m + 1)
        out.append(mutate(rnd, s[at:at + m], rnd.randrange(0, 3)))
    return out


def compare(store, cell, r, y, rnd):
    """slot y takes the cell's state whole through t4_cellstore_stage; r (staged by the caller, same flush) must equal it"""
    store.stage_form(y, cell.icell(), "full")
    slots = check_equal(cell, store.read(r), store.read(y))
    reads = reads_of(rnd, cell)
    res_r = store.query([r] * len(reads), reads, [cell.barcode] * len(reads))
    res_y = store.query([y] * len(reads), reads, [cell.barcode] * len(reads))
    for a, b in zip(res_r, res_y):
        assert a.tobytes() == b.tobytes()
    return slots, int(res_r[0].sum())


def step(store, cell, r, y, touched, rnd):
    """one delta: must be taken as a delta"""
    store.reserve_for(max(r, y), cell)
    before = store.rstats()
    store.stage_delta(r, cell, touched)
    out = compare(store, cell, r, y, rnd)
    after = store.rstats()
    assert (after["deltas"] - before["deltas"], after["delta_contigs"] - before["delta_contigs"], after["whole"] - before["whole"]) == (1, len(touched), 0)
    return out


def change(store, cell, r, y, touched, rnd):
    """a delta where the slot's layout takes it (1), the whole image where the store says it does not (0)"""
    ids, lens = np.array(touched, dtype=np.int32), np.array(cell.lens(touched), dtype=np.int32)
    if store.lib.t4_cellstore_delta_fits(store.h, r, cell.nseq, len(touched), ids.ctypes.data, lens.ctypes.data, cell.npost) == 1:
        step(store, cell, r, y, touched, rnd)
        return 1
    whole_after_misfit(store, cell, r, y, touched, rnd)
    return 0


def start_cell(rnd, k, ncontig):
    hom = rand_seq(rnd, 30) + "G" * (k + 21) + rand_seq(rnd, 30)
    with_n = rand_seq(rnd, 60) + "N" + rand_seq(rnd, 80)
    # a lone contig starts at 370 bases: 354 or 362 postings give a table of 1024 slots, which serves 682 -- the changes reach 613;
    # beside the 700-base contig 100 bases do (2048 slots serve 1364, the changes stay below 1250)
    cons = [rand_seq(rnd, 370 if ncontig == 1 else 100), rand_seq(rnd, k - 1), hom, rand_seq(rnd, k), with_n, rand_seq(rnd, 700)][:ncontig]
    return RCell(rnd, 40 + ncontig, cons, k)


def every_kind_of_delta(eng, k, ncontig, seed):
    """every kind is taken as a DELTA (step asserts the counters): the first contig's stretch has room for its 122 more bases and the
    table, sized from the first image's postings, serves every total the changes reach (start_cell)"""
    rnd = random.Random(seed)
    store = RStore(eng, k)
    try:
        cell = start_cell(rnd, k, ncontig)
        r, y = store.open(), store.open()
        store.reserve_for(max(r, y), cell)
        store.stage_whole(r, cell)
        slots, hits = compare(store, cell, r, y, rnd)
        assert slots == table_slots(cell.npost) and hits > 0
        last = cell.nseq - 1
        s = lambda i: cell.cons[i]
        # append 1 and 60 bases, prepend 1 and 60 bases (every offset of the contig shifts)
        for grow in (lambda x: x + rand_seq(rnd, 1), lambda x: x + rand_seq(rnd, 60), lambda x: rand_seq(rnd, 1) + x, lambda x: rand_seq(rnd, 60) + x):
            step(store, cell, r, y, cell.set(0, grow(s(0))), rnd)
        # substitute one base in the middle and one in the last k-mer
        for pos in (len(s(0)) // 2, len(s(0)) - 2):
            step(store, cell, r, y, cell.set(0, s(0)[:pos] + {"A": "C", "C": "G", "G": "T", "T": "A"}[s(0)[pos]] + s(0)[pos + 1:]), rnd)
        step(store, cell, r, y, cell.add(rand_seq(rnd, 90)), rnd)                       # a new contig
        step(store, cell, r, y, cell.add(rand_seq(rnd, 55)), rnd)
        step(store, cell, r, y, cell.release(cell.nseq - 2), rnd)                       # a released one
        # a merge: one contig released, the other rewritten
        gone, kept = cell.nseq - 1, 0
        merged = s(kept)[:100] + s(gone)
        step(store, cell, r, y, sorted(cell.release(gone) + cell.set(kept, merged, "TRBV")), rnd)
        # two contigs in one delta (the last one again when there is only one more)
        other = min(2, last)
        step(store, cell, r, y, sorted(set(cell.set(0, s(0)[3:]) + cell.set(other, s(other) + rand_seq(rnd, 7)))), rnd)
        # nothing but counts: a second posting at one offset, none at another
        cell.counts[0][5] += 1
        cell.counts[0][9] = 0
        step(store, cell, r, y, [0], rnd)
    finally:
        store.close()


@pytest.mark.parametrize("k", [9, 17])
@pytest.mark.parametrize("ncontig", [1, 6])
def test_every_kind_of_delta_equals_the_whole_image(eng, k, ncontig):
    every_kind_of_delta(eng, k, ncontig, 100 * k + ncontig)


def test_negative_control_a_dropped_contig_is_seen(monkeypatch):
    """emulator only: with the test knob that keeps the first touched contig of every delta back, the comparison above fails"""
    monkeypatch.setenv("T4_LIB", t4check.build_emulator_lib())
    import trust4_amd
    e = trust4_amd.Engine(0)
    try:
        every_kind_of_delta(e, 9, 6, 906)
        monkeypatch.setenv("T4_TEST_DELTA_DROP", "1")
        with pytest.raises((AssertionError, trust4_amd.api.T4Error)):   # (a comparison, or the device's own check of the counts' total)
            every_kind_of_delta(e, 9, 6, 906)
    finally:
        e.close()


def stretch_of(store, slot, i):
    img, v = store.read(slot)
    rec = records(img, v)
    return int(rec[i + 1]["consOff"] - rec[i]["consOff"])


def whole_after_misfit(store, cell, r, y, touched, rnd):
    """the delta is sent back, nothing queued; the cell goes whole and equals its yardstick"""
    store.reserve_for(max(r, y), cell)
    before, staged = store.rstats(), store.bytes_staged()
    rc, _ = store.stage_delta_rc(r, cell, touched)
    assert rc == T4_CELL_DELTA_WHOLE
    store.read(r)
    assert store.bytes_staged() == staged
    store.stage_whole(r, cell)
    out = compare(store, cell, r, y, rnd)
    after = store.rstats()
    assert [after[f] - before[f] for f in ("sent_back", "restages", "whole", "deltas")] == [1, 1, 1, 0]
    return out


def test_contig_fills_its_stretch_then_outgrows_it(store):
    rnd = random.Random(11)
    cell = RCell(rnd, 3, [rand_seq(rnd, 100), rand_seq(rnd, 700)], 9)   # (postings enough that the table has room for the growth)
    r, y = store.open(), store.open()
    store.reserve_for(y, cell)
    store.stage_whole(r, cell)
    compare(store, cell, r, y, rnd)
    cap = stretch_of(store, r, 0)
    assert cap % 128 == 0 and cap >= 101
    step(store, cell, r, y, cell.set(0, cell.cons[0] + rand_seq(rnd, cap - 1 - 100)), rnd)   # length + terminator == the stretch
    assert stretch_of(store, r, 0) == cap
    whole_after_misfit(store, cell, r, y, cell.set(0, cell.cons[0] + "A"), rnd)
    assert stretch_of(store, r, 0) > cap


def test_more_contigs_than_records(store):
    rnd = random.Random(12)
    cell = RCell(rnd, 4, [rand_seq(rnd, 50)], 9)
    r, y = store.open(), store.open()
    store.reserve_for(y, cell)
    store.stage_whole(r, cell)
    compare(store, cell, r, y, rnd)
    img, v = store.read(r)
    room = (v.pw - v.seqs) // 24   # records between the postings and the predicate bytes
    assert room >= 2
    for _ in range(room + 1):
        touched = cell.add(rand_seq(rnd, 8))   # (shorter than k: no posting, the table stays as it is)
        if not change(store, cell, r, y, touched, rnd):   # sent back, staged whole, compared
            break
    else:
        raise AssertionError("%d contigs in %d records" % (cell.nseq, room))
    assert 2 < cell.nseq <= room + 1
    step(store, cell, r, y, cell.add(rand_seq(rnd, 8)), rnd)   # the fresh layout has spare records again


def test_table_step_from_64_to_128_slots_and_back(store):
    rnd = random.Random(13)
    s = rand_seq(rnd, 50)
    cell = RCell(rnd, 5, [s, rand_seq(rnd, 30)], 9)
    assert cell.npost == 42 + 22
    cell.counts[1][:] = 0                      # 42 postings: the last number a table of 64 slots serves
    r, y = store.open(), store.open()
    store.reserve_for(y, cell)
    store.stage_whole(r, cell)
    assert compare(store, cell, r, y, rnd)[0] == 64 == table_slots(42)
    cell.counts[1][3] = 1                      # 43
    assert whole_after_misfit(store, cell, r, y, [1], rnd)[0] == 128 == table_slots(43)
    cell.counts[1][3] = 0                      # back to 42: fits the table it has, stays resident
    assert step(store, cell, r, y, [1], rnd)[0] == 128
    store.reserve_for(y, cell)
    store.stage_whole(r, cell)                 # a whole image sizes the table anew
    assert compare(store, cell, r, y, rnd)[0] == 64


def test_count_of_255_stays_resident(store):
    rnd = random.Random(14)
    cell = RCell(rnd, 6, [rand_seq(rnd, 120), rand_seq(rnd, 60)], 9)
    cell.counts[0][17] = 200
    r, y = store.open(), store.open()
    store.reserve_for(y, cell)
    store.stage_whole(r, cell)
    compare(store, cell, r, y, rnd)
    cell.counts[0][17] = 255
    step(store, cell, r, y, [0], rnd)


def test_recycled_slot_starts_whole(store):
    rnd = random.Random(15)
    cell = RCell(rnd, 7, [rand_seq(rnd, 300), rand_seq(rnd, 80)], 9)
    r, y = store.open(), store.open()
    store.reserve_for(y, cell)
    store.stage_whole(r, cell)
    compare(store, cell, r, y, rnd)
    store.eng.check(store.lib.t4_cellstore_close(store.h, r))
    again = store.open()
    assert again == r
    other = RCell(rnd, 8, [rand_seq(rnd, 70)], 9)
    store.reserve_for(y, other)
    rc, _ = store.stage_delta_rc(again, other, [0])
    assert rc == T4_ERR_ARG and "no resident image" in store.err()
    store.stage_whole(again, other)
    compare(store, other, again, y, rnd)
    step(store, other, again, y, other.set(0, other.cons[0] + "ACGTTG"), rnd)
    # an image of another form ends residency as well
    store.reserve(again, [(other.icell(), "indexed")])
    store.stage_form(again, other.icell(), "indexed")
    store.read(again)
    store.reserve_for(y, other)
    rc, _ = store.stage_delta_rc(again, other, [0])
    assert rc == T4_ERR_ARG and "no resident image" in store.err()


def test_one_flush_of_all_forms_with_patches(store):
    """a full, a compact, an indexed, a resident-whole and a resident-delta image and byte patches on a resident slot in ONE flush"""
    rnd = random.Random(16)
    cells = [RCell(rnd, 20 + i, [rand_seq(rnd, rnd.randrange(45, 200)) for _ in range(1 + i % 3)], 9) for i in range(6)]
    slots = [store.open() for _ in cells]
    yard = [store.open() for _ in cells]
    top = max(slots + yard)
    # before the flush under test: cells 4 and 5 are resident
    for i in (4, 5):
        store.reserve_for(top, cells[i], full=False)
        store.stage_whole(slots[i], cells[i])
    img5, v5 = store.read(slots[5])
    rec5 = records(img5, v5)
    touched = cells[4].set(0, "ACGTAC" + cells[4].cons[0]) + cells[4].add(rand_seq(rnd, 64))
    need = sum(store.staged_bytes(c.icell(), f) for c, f in zip(cells, ("full", "compact", "indexed")))
    need += store.resident_bytes(cells[3].lens()) + store.resident_bytes(cells[4].lens(touched))
    store.eng.check(store.lib.t4_cellstore_prepare(store.h, top, need))
    flushed = store.bytes_staged()
    o_pw = [store.stage_form(slots[i], cells[i].icell(), f) for i, f in enumerate(("full", "compact", "indexed"))]
    store.stage_whole(slots[3], cells[3])
    store.stage_delta(slots[4], cells[4], touched)
    # patches on resident slot 5: two predicate bytes of its first contig get the values other counts would give
    offs = np.array([v5.pw - v5.ctab + rec5[0]["pwOff"] + p for p in (2, 11)], dtype=np.int64)
    vals = np.array([1, 8], dtype=np.uint8)
    cells[5].pw[0][4 * 2:4 * 2 + 4] = [5, 0, 0, 0]      # sum 5 < 3 * 5: bit 0
    cells[5].pw[0][4 * 11:4 * 11 + 4] = [0, 0, 0, 3]    # bit 3
    store.eng.check(store.lib.t4_cellstore_patch(store.h, slots[5], 2, offs.ctypes.data, vals.ctypes.data))
    images = [store.read(s) for s in slots]              # the first read is the flush
    assert store.bytes_staged() - flushed == need + 2
    for c, sy in zip(cells, yard):
        store.reserve(top, [(c.icell(), "full")])
        store.stage_form(sy, c.icell(), "full")
    for i, f in enumerate(("full", "compact", "indexed")):
        check_pair(cells[i].icell(), store.read(yard[i]), images[i], (o_pw[i], o_pw[i]))
    for i in (3, 4, 5):
        check_equal(cells[i], images[i], store.read(yard[i]))


def test_refusals_queue_nothing(store):
    rnd = random.Random(17)
    cell = RCell(rnd, 9, [rand_seq(rnd, 90), rand_seq(rnd, 60)], 9)
    r, y, fresh = store.open(), store.open(), store.open()
    store.reserve_for(y, cell)
    store.stage_whole(r, cell)
    compare(store, cell, r, y, rnd)
    store.eng.check(store.lib.t4_cellstore_prepare(store.h, fresh, 8 * store.resident_bytes(cell.lens())))
    staged = store.bytes_staged()
    rc, _ = store.stage_delta_rc(r, cell, [1], ids=[2])                     # a touched id out of range
    assert rc == T4_ERR_ARG and "outside the cell" in store.err()
    rc, _ = store.stage_delta_rc(r, cell, [0, 1], ids=[1, 0])               # ... out of order
    assert rc == T4_ERR_ARG
    beyond = np.append(cell.counts[1], np.uint8(1))                         # a count at o + k beyond the contig
    good, cell.counts[1] = cell.counts[1], beyond
    rc, _ = store.stage_delta_rc(r, cell, [1])
    assert rc == T4_ERR_ARG and "offset %d" % (60 - 9 + 1) in store.err()
    cell.counts[1] = good
    rc, _ = store.stage_delta_rc(r, cell, [1], npost=cell.npost + 1)        # counts that do not add up to npost
    assert rc == T4_ERR_ARG and "add up" in store.err()
    rc, _ = store.stage_delta_rc(r, cell, npost=cell.npost - 1)             # ... of a whole image
    assert rc == T4_ERR_ARG and "add up" in store.err()
    rc, _ = store.stage_delta_rc(fresh, cell, [0])                          # a slot with no resident image
    assert rc == T4_ERR_ARG and "no resident image" in store.err()
    store.read(r)
    assert store.bytes_staged() == staged
    step(store, cell, r, y, cell.set(1, cell.cons[1] + "TTGACC"), rnd)      # the slot is as it was: the next delta applies


def test_flush_refuses_a_counted_kmer_with_an_n(store):
    rnd = random.Random(18)
    good = RCell(rnd, 10, [rand_seq(rnd, 100)], 9)
    bad = RCell(rnd, 11, [rand_seq(rnd, 70), rand_seq(rnd, 50)], 9)
    s_good, s_bad, y = store.open(), store.open(), store.open()
    for s, c in ((s_good, good), (s_bad, bad)):
        store.reserve_for(y, c)
        store.stage_whole(s, c)
    compare(store, bad, s_bad, y, rnd)
    t = bad.cons[1]
    bad.cons[1] = t[:20] + "N" + t[21:]          # the counts still count the k-mers across position 20
    store.eng.check(store.lib.t4_cellstore_prepare(store.h, y, store.resident_bytes(bad.lens()) + store.resident_bytes(good.lens()) + 64))
    store.stage_delta(s_good, good, good.set(0, good.cons[0] + "ACCGT"))
    rc, _ = store.stage_delta_rc(s_bad, bad, [1])
    assert rc == 0                               # the host cannot see it
    rc, _, _ = store.read_rc(s_good)             # the flush
    assert rc == T4_ERR_ARG
    msg = store.err()
    assert "slot %d" % s_bad in msg and "ACGT" in msg, msg
    compare(store, good, s_good, y, rnd)         # the other image of that flush is whole
    rc, _ = store.stage_delta_rc(s_bad, bad, [1])
    assert rc == T4_ERR_ARG and "no resident image" in store.err()   # the refused slot wants a whole image
    bad.set(1, bad.cons[1])
    store.reserve_for(y, bad)
    store.stage_whole(s_bad, bad)
    compare(store, bad, s_bad, y, rnd)


def test_bytes_of_a_one_contig_delta(store):
    rnd = random.Random(19)
    cell = RCell(rnd, 12, [rand_seq(rnd, n) for n in (150, 220, 90, 400, 130, 310)], 9)
    r = store.open()
    store.reserve_for(r, cell, full=False)
    store.stage_whole(r, cell)
    store.read(r)
    touched = cell.set(2, cell.cons[2] + rand_seq(rnd, 25))
    store.reserve_for(r, cell, full=False)
    before = store.bytes_staged()
    store.stage_delta(r, cell, touched)
    store.read(r)
    shipped = store.bytes_staged() - before
    ic = cell.icell()
    assert shipped == store.resident_bytes([115]) == al16(40) + 3 * al16(116) + 128
    assert shipped < store.lib.t4_cellstore_indexed_image_bytes(ic.nseq, ic.cons_bytes)
