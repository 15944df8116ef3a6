"""Per-barcode set images whose k-mer index -- hash table AND postings -- is built on the device from the image's own contigs
(t4_cellstore_stage_indexed + cellIndexBuildKernel) against the images the host writes in full (t4_cellstore_stage, the yardstick).
A synthetic cell is a set of contigs plus one count byte per offset (the postings the index holds there); Python derives the key
list and the postings from them. The cell goes into slot A whole and into slot B as contigs + counts, both in ONE flush, both are
read back (t4_cellstore_read_image) and compared:
  (a) everything from the sequence records to the end of the image is byte-equal, the views are equal apart from the base
      pointers, the images have the same size;
  (b) both tables have table_slots(nkeys) slots and the same {code: cnt};
  (c) for every code the sorted list of (contig, offset) postings is the same in A and B (the order inside a list is free);
  (d) in B the lists tile [0, npost) without overlap or gap;
  (e) in B every key is reachable from mix64(code) & mask without crossing an empty slot, every other slot is exactly (~0, 0, 0).
On the emulator build of the kernels and, marked gpu, through libt4hip.so."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import t4check
from test_cell_images import M64, Store, View, codes_with_home, mix64, table_map, table_of, table_slots

T4_ERR_ARG = -1
K = 9
OV = np.dtype([("seqIdx", "<i4"), ("readStart", "<i4"), ("readEnd", "<i4"), ("seqStart", "<i4"), ("seqEnd", "<i4"), ("strand", "<i4"),
               ("matchCnt", "<i4"), ("indelCnt", "<i4"), ("similarity", "<f8")])   # t4_overlap


def al16(x):
    return (x + 15) & ~15


def code_of(kmer):
    c = 0
    for ch in kmer:
        c = (c << 2) | "ACGT".index(ch)
    return c


def kmer_of(code, k=K):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def rand_seq(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def all_marked(s, k=K):
    return [1] * max(0, len(s) - k + 1)


class ICell:
    """contigs + counts: counts[i][o] postings (i, o); the index they stand for is derived here"""

    def __init__(self, rnd, barcode, cons, counts, nkeys=None, k=K, derive=True):
        self.barcode, self.nseq, self.cons, self.k = barcode, len(cons), list(cons), k
        self.counts = [None if c is None else np.array(c, dtype=np.uint8) for c in counts]
        self.names = (["IGHV", "TRBC", "", "IGKJ"] + ["Novel"] * self.nseq)[:self.nseq]
        self.pw = [np.array([rnd.randrange(0, 6) for _ in range(4 * len(s))], dtype=np.int32) for s in cons]
        self.lists = {}   # code -> [(contig, offset)] with repeats
        if derive:
            for i, (s, c) in enumerate(zip(cons, self.counts)):
                for o, m in enumerate([] if c is None else c.tolist()):
                    if m:
                        self.lists.setdefault(code_of(s[o:o + k]), []).extend([(i, o)] * m)
        self.npost = sum(len(v) for v in self.lists.values())
        self.nkeys = len(self.lists) if nkeys is None else nkeys
        self.cons_bytes = sum(len(s) + 1 for s in cons)

    # the key list of the yardstick: the keys with postings, then keys without any up to the announced number (they only size the table)
    def key_list(self):
        codes = list(self.lists)
        cnts = [len(self.lists[c]) for c in codes]
        spare = (1 << (2 * self.k)) + 5
        while len(codes) < self.nkeys:
            codes.append(spare)
            cnts.append(0)
            spare += 1
        post = np.array([v for c in self.lists for p in self.lists[c] for v in p], dtype=np.int32)
        return codes, cnts, post

    def sizes(self):   # (nseq, nkeys, npost, cons_bytes) of t4_cellstore_*image_bytes
        return self.nseq, self.nkeys, self.npost, self.cons_bytes


class FullView:
    """an ICell as tests/test_cell_images.Store.stage wants a cell"""

    def __init__(self, cell):
        self.barcode, self.nseq, self.names, self.cons, self.pw = cell.barcode, cell.nseq, cell.names, cell.cons, cell.pw
        self.codes, self.cnts, self.post = cell.key_list()
        if not len(self.post):
            self.post = np.zeros(2, dtype=np.int32)


class IStore(Store):
    def __init__(self, eng, k=K):
        super().__init__(eng, k)
        P, I, L, Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
        for name, res, args in (("t4_cellstore_stage_indexed", I, [P, I, I, I, P, P, P, L, L, P, P, P]),
                                ("t4_cellstore_indexed_image_bytes", Z, [I, L]), ("t4_cellstore_indexed_stats", I, [P, P]),
                                ("t4_cellstore_query", I, [P, I, P, P, P, P, P, I, P, I, P, P, P, P])):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args

    def staged_bytes(self, cell, form):
        if form == "indexed":
            return self.lib.t4_cellstore_indexed_image_bytes(cell.nseq, cell.cons_bytes)
        if form == "compact":
            return self.lib.t4_cellstore_image_bytes(cell.nseq, len(cell.lists), cell.npost, cell.cons_bytes)
        return self.lib.t4_cellstore_full_image_bytes(*cell.sizes())

    def reserve(self, max_slot, cells_forms):
        self.eng.check(self.lib.t4_cellstore_prepare(self.h, max_slot, sum(self.staged_bytes(c, f) for c, f in cells_forms)))

    def stage_indexed_rc(self, slot, cell, npost=None, short=False):
        n = cell.nseq
        names = (C.c_char_p * n)(*[x.encode() for x in cell.names])
        cons = (C.c_char_p * n)(*[x.encode() for x in cell.cons])
        pw = (C.c_void_p * n)(*[a.ctypes.data for a in cell.pw])
        cnt = (C.c_void_p * n)(*[None if a is None or not len(a) else a.ctypes.data for a in cell.counts])
        lens = np.array([0 if a is None else len(a) for a in cell.counts], dtype=np.int32)
        o_pw = C.c_int64(-1)
        rc = self.lib.t4_cellstore_stage_indexed(self.h, slot, cell.barcode, n, C.cast(names, C.c_void_p), C.cast(cons, C.c_void_p),
                                                 C.cast(pw, C.c_void_p), cell.nkeys, cell.npost if npost is None else npost,
                                                 C.cast(cnt, C.c_void_p), lens.ctypes.data if n else None, C.addressof(o_pw))
        return rc, o_pw.value

    def stage_form(self, slot, cell, form):
        if form == "indexed":
            rc, o = self.stage_indexed_rc(slot, cell)
            self.eng.check(rc)
            return o
        return self.stage(slot, FullView(cell), form == "compact")

    def istats(self):
        v = (C.c_int64 * 4)()
        self.eng.check(self.lib.t4_cellstore_indexed_stats(self.h, C.cast(v, C.c_void_p)))
        return list(v)

    def query(self, slots, reads, barcodes, max_per_read=32):
        n = len(reads)
        bases = "".join(reads).encode()
        offs = np.cumsum([0] + [len(r) for r in reads]).astype(np.int64)
        sl, bc = np.array(slots, dtype=np.int32), np.array(barcodes, dtype=np.int32)
        st, fac = np.zeros(n, dtype=np.int32), np.full(n, 2.0)
        counts, ret = np.zeros(n, dtype=np.int32), np.zeros(n * max_per_read, dtype=np.int32)
        ov, ext = np.zeros(n * max_per_read, dtype=OV), np.zeros(n * max_per_read, dtype=OV)
        self.eng.check(self.lib.t4_cellstore_query(self.h, n, sl.ctypes.data, bases, offs.ctypes.data, bc.ctypes.data, st.ctypes.data, 0,
                                                   fac.ctypes.data, max_per_read, counts.ctypes.data, ov.ctypes.data, ext.ctypes.data, ret.ctypes.data))
        return counts, ov, ext, ret


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
    s = IStore(eng)
    yield s
    s.close()


def lists_of(img, view):
    """{code: sorted postings} and {code: (start, cnt)} of an image read back"""
    tab = table_of(img, view)
    m = table_map(tab)
    o_post = view.post - view.ctab
    npost = sum(n for _, n in m.values())
    post = np.frombuffer(img[o_post:o_post + 8 * npost].tobytes(), dtype="<i4").reshape(-1, 2)
    assert all(st + n <= npost for st, n in m.values())
    return {c: sorted(map(tuple, post[st:st + n].tolist())) for c, (st, n) in m.items()}, m, tab


def check_pair(cell, full, indexed, o_pw):
    (img_a, va), (img_b, vb) = full, indexed
    o_seq = va.seqs - va.ctab
    # (a)
    assert len(img_a) == len(img_b) and o_seq % 16 == 0
    assert bytes(img_a[o_seq:]) == bytes(img_b[o_seq:])
    for f in View.SCALARS:
        assert getattr(va, f) == getattr(vb, f), f
    for f in View.POINTERS:
        assert getattr(va, f) - va.ctab == getattr(vb, f) - vb.ctab, f
    assert va.ctab != vb.ctab and vb.ctab % 16 == 0
    assert va.pw - va.ctab == o_pw[0] == o_pw[1]
    la, ma, ta = lists_of(img_a, va)
    lb, mb, tb = lists_of(img_b, vb)
    # (b)
    assert len(ta) == len(tb) == table_slots(cell.nkeys)
    assert {c: n for c, (_, n) in ma.items()} == {c: n for c, (_, n) in mb.items()} == {c: len(v) for c, v in cell.lists.items()}
    # (c)
    assert la == lb == {c: sorted(v) for c, v in cell.lists.items()}
    # (d)
    at = 0
    for st, n in sorted(mb.values()):
        assert st == at and n > 0
        at += n
    assert at == cell.npost and vb.seqs - vb.post >= 8 * cell.npost
    # (e)
    mask = len(tb) - 1
    codes = tb["code"]
    for c in cell.lists:
        s = mix64(c) & mask
        for _ in range(len(tb)):
            assert codes[s] != M64, "key %d behind an empty slot" % c
            if codes[s] == c:
                break
            s = (s + 1) & mask
        else:
            raise AssertionError("key %d not found" % c)
    empty = tb[codes == M64]
    assert len(empty) == len(tb) - len(cell.lists) and not empty["start"].any() and not empty["cnt"].any()


def run_pairs(store, cells):
    """every cell in full into a slot of its own and indexed into another, ONE flush, all read back and compared; the counters
    against their closed forms"""
    a = [store.open() for _ in cells]
    b = [store.open() for _ in cells]
    store.reserve(max(a + b), [(c, "full") for c in cells] + [(c, "indexed") for c in cells])
    before, ibefore = store.stats(), store.istats()
    o_pw = [(store.stage_form(sa, c, "full"), store.stage_form(sb, c, "indexed")) for c, sa, sb in zip(cells, a, b)]
    for c, sa, sb, o in zip(cells, a, b, o_pw):
        check_pair(c, store.read(sa), store.read(sb), o)
    after, iafter = store.stats(), store.istats()
    assert after[:3] == before[:3]   # the compact form's counters do not move
    assert after[3] - before[3] == sum(store.staged_bytes(c, "full") + store.staged_bytes(c, "indexed") for c in cells)
    assert [x - y for x, y in zip(iafter, ibefore)] == [len(cells), sum(al16(c.cons_bytes) for c in cells), sum(c.npost for c in cells),
                                                         sum(16 * table_slots(c.nkeys) for c in cells)]
    for c in cells:   # the closed form of the staged size: count bytes + the image from its sequence records on + the view
        tail = al16(al16(al16(24 * c.nseq) + c.cons_bytes) + c.cons_bytes + 16)
        assert store.staged_bytes(c, "indexed") == al16(c.cons_bytes) + tail + 128
    return a, b


def test_no_contig_and_no_counts(store):
    rnd = random.Random(1)
    none = ICell(rnd, 3, [], [])
    zeros = ICell(rnd, 4, [rand_seq(rnd, 40), rand_seq(rnd, 25)], [[0] * 32, None])
    for c in (none, zeros):
        assert c.npost == 0 and table_slots(c.nkeys) == 64
    run_pairs(store, [none, zeros])


def test_contig_lengths_around_k(store):
    rnd = random.Random(2)
    short = ICell(rnd, 5, [rand_seq(rnd, K - 1), rand_seq(rnd, 30)], [None, all_marked("x" * 30)])
    exact = ICell(rnd, 6, [rand_seq(rnd, K)], [[1]])
    assert exact.npost == 1
    run_pairs(store, [short, exact])


def test_one_key_two_offsets_and_two_contigs(store):
    rnd = random.Random(3)
    unit = rand_seq(rnd, 50)
    twice = unit + unit[:20]
    inside = ICell(rnd, 7, [twice], [all_marked(twice)])
    assert any(len({o for _, o in v}) == 2 for v in inside.lists.values())
    other = rand_seq(rnd, 10) + unit + rand_seq(rnd, 7)
    across = ICell(rnd, 8, [unit, other], [all_marked(unit), all_marked(other)])
    assert any(len({s for s, _ in v}) == 2 for v in across.lists.values())
    run_pairs(store, [inside, across])


def test_homopolymer_puts_every_posting_on_one_key(store):
    rnd = random.Random(4)
    cell = ICell(rnd, 9, ["A" * 70, rand_seq(rnd, 33)], [[1] * 62, all_marked("x" * 33)])
    assert len(cell.lists[0]) == 62
    run_pairs(store, [cell])


@pytest.mark.parametrize("m", [2, 3, 255])
def test_repeated_postings(store, m):
    rnd = random.Random(m)
    s = rand_seq(rnd, 45)
    cnt = all_marked(s)
    cnt[11] = m
    cell = ICell(rnd, 10, [s], [cnt])
    assert cell.npost == len(cnt) - 1 + m
    run_pairs(store, [cell])


def test_sparse_marks_and_homopolymer_skip(store):
    rnd = random.Random(5)
    s = rand_seq(rnd, 80)
    third = ICell(rnd, 11, [s], [[1 if o % 3 == 0 else 0 for o in range(len(s) - K + 1)]])
    # BuildIndexFromRead skips a k-mer equal to the one before it: of a homopolymer stretch only the first offset is indexed
    h = rand_seq(rnd, 12) + "C" + "G" * 20 + "T" + rand_seq(rnd, 12)
    cnt = [1] * (len(h) - K + 1)
    for o in range(1, len(cnt)):
        if h[o:o + K] == h[o - 1:o - 1 + K]:
            cnt[o] = 0
    assert cnt.count(0) == 20 - K
    run_pairs(store, [third, ICell(rnd, 12, [h], [cnt])])


def cell_of_codes(rnd, barcode, codes, nkeys=None):
    """one contig of exactly k bases per key"""
    return ICell(rnd, barcode, [kmer_of(c) for c in codes], [[1]] * len(codes), nkeys=nkeys)


@pytest.mark.parametrize("nkeys", [42, 43])
def test_table_size_step(store, nkeys):
    rnd = random.Random(nkeys)
    cell = cell_of_codes(rnd, 13, rnd.sample(range(1 << 18), nkeys))
    assert len(cell.lists) == nkeys and table_slots(nkeys) == (128 if nkeys == 43 else 64)
    run_pairs(store, [cell])


def test_more_keys_announced_than_own_postings(store):
    rnd = random.Random(6)
    s = rand_seq(rnd, 60)
    cell = ICell(rnd, 14, [s], [all_marked(s)], nkeys=200)
    assert len(cell.lists) < 60 and table_slots(200) == 512
    run_pairs(store, [cell])


def test_shared_home_slot_and_wrap_around(store):
    rnd = random.Random(7)
    shared = cell_of_codes(rnd, 15, codes_with_home(17, 8, 63))
    wrap = cell_of_codes(rnd, 16, codes_with_home(63, 6, 63) + codes_with_home(0, 2, 63))
    assert all(c < (1 << (2 * K)) for c in list(shared.lists) + list(wrap.lists))
    run_pairs(store, [shared, wrap])


def test_several_keys_per_thread(store):
    rnd = random.Random(50)
    cons = [rand_seq(rnd, 1100) for _ in range(5)]
    cell = ICell(rnd, 77, cons, [all_marked(s) for s in cons])
    assert 4500 < len(cell.lists) <= 5 * 1092
    run_pairs(store, [cell])


def small_cell(rnd, i):
    n = [0, 1, 2, 3][i % 4]
    cons = [rand_seq(rnd, rnd.randrange(8, 60)) for _ in range(n)]
    return ICell(rnd, i, cons, [[rnd.choice([0, 1, 1, 2]) for _ in all_marked(s)] for s in cons])


def test_one_flush_of_more_images_than_workgroups_in_all_three_forms(store, eng):
    n = 300 if eng.emulated else 8 * eng.cus() + 50
    n = 3 * ((n + 2) // 3)   # a third full, a third compact, a third indexed -- each against a full yardstick
    rnd = random.Random(300)
    cells = [small_cell(rnd, i) for i in range(n)]
    forms = ["full", "compact", "indexed"]
    a = [store.open() for _ in cells]
    b = [store.open() for _ in cells]
    store.reserve(max(a + b), [(c, "full") for c in cells] + [(c, forms[i % 3]) for i, c in enumerate(cells)])
    o_pw = [(store.stage_form(sa, c, "full"), store.stage_form(sb, c, forms[i % 3])) for i, (c, sa, sb) in enumerate(zip(cells, a, b))]
    assert n > 8 * eng.cus()
    before = store.istats()
    for c, sa, sb, o in zip(cells, a, b, o_pw):
        check_pair(c, store.read(sa), store.read(sb), o)
    assert store.istats()[0] - before[0] == n // 3


def test_more_indexed_images_than_workgroups(store, eng):
    n = 300 if eng.emulated else 8 * eng.cus() + 50
    rnd = random.Random(301)
    run_pairs(store, [small_cell(rnd, i) for i in range(n)])


def test_restaged_slot_and_recycled_slot(store):
    rnd = random.Random(21)
    a, b = store.open(), store.open()

    def pair(sa, sb, n_bases):
        cons = [rand_seq(rnd, n_bases // 2), rand_seq(rnd, n_bases - n_bases // 2)]
        cell = ICell(rnd, 9, cons, [all_marked(s) for s in cons])
        store.reserve(max(sa, sb), [(cell, "full"), (cell, "indexed")])
        o = (store.stage_form(sa, cell, "full"), store.stage_form(sb, cell, "indexed"))
        check_pair(cell, store.read(sa), store.read(sb), o)

    for n_bases in (300, 30, 1600):
        pair(a, b, n_bases)
    store.eng.check(store.lib.t4_cellstore_close(store.h, b))
    pair(a, store.open(), 1200)


def test_host_refuses_bad_counts_before_anything_is_queued(store):
    rnd = random.Random(31)
    s = rand_seq(rnd, 40)
    slot = store.open()
    beyond = ICell(rnd, 1, [s], [[1] * (len(s) - K + 1) + [1]], derive=False)
    beyond.npost = len(s) - K + 2
    beyond.nkeys = 64
    good = ICell(rnd, 1, [s], [all_marked(s)])
    store.reserve(slot, [(good, "indexed")] * 3)
    before = store.stats()
    rc, _ = store.stage_indexed_rc(slot, beyond)
    assert rc == T4_ERR_ARG and "offset %d" % (len(s) - K + 1) in store.lib.t4_last_error(store.eng.h).decode()
    rc, _ = store.stage_indexed_rc(slot, good, npost=good.npost + 1)
    assert rc == T4_ERR_ARG and "add up" in store.lib.t4_last_error(store.eng.h).decode()
    empty_table = ICell(rnd, 1, [s], [all_marked(s)], nkeys=0)
    rc, _ = store.stage_indexed_rc(slot, empty_table)
    assert rc == T4_ERR_ARG
    # nothing was queued: the slot is free for an image in the same flush, and only that image is staged
    full = store.open()
    store.reserve(max(slot, full), [(good, "full")])
    o = (store.stage_form(full, good, "full"), store.stage_form(slot, good, "indexed"))
    check_pair(good, store.read(full), store.read(slot), o)
    assert store.stats()[3] - before[3] == store.staged_bytes(good, "full") + store.staged_bytes(good, "indexed")


@pytest.mark.parametrize("what", ["N", "small_table"])
def test_device_refuses_and_the_store_goes_on(store, what):
    """what the host cannot see: a counted k-mer with an N, a table too small for the distinct k-mers. T4_ERR_ARG from the flush
    naming the slot; the good image of the same flush is whole; the refused slot takes a good image afterwards"""
    rnd = random.Random(41)
    s = rand_seq(rnd, 90)
    good = ICell(rnd, 5, [s], [all_marked(s)])
    if what == "N":
        t = s[:30] + "N" + s[31:]
        bad = ICell(rnd, 4, [t], [all_marked(t)], derive=False)
        bad.npost, bad.nkeys = len(t) - K + 1, 90
    else:
        bad = ICell(rnd, 4, [s], [all_marked(s)], nkeys=20)   # 64 slots for 82 distinct 9-mers
        assert len(bad.lists) > 64
    s_good, s_bad = store.open(), store.open()
    store.reserve(s_bad, [(good, "indexed"), (bad, "indexed")])
    store.stage_form(s_good, good, "indexed")
    rc, _ = store.stage_indexed_rc(s_bad, bad)
    assert rc == 0   # the host accepts it
    rc, _, _ = store.read_rc(s_good)   # the flush
    assert rc == T4_ERR_ARG
    msg = store.lib.t4_last_error(store.eng.h).decode()
    assert "slot %d" % s_bad in msg and ("ACGT" in msg if what == "N" else "too small" in msg), msg
    s_full = store.open()
    store.reserve(max(s_full, s_bad), [(good, "full"), (good, "indexed")])
    o_full = store.stage_form(s_full, good, "full")
    img_full = store.read(s_full)
    check_pair(good, img_full, store.read(s_good), (o_full, o_full))   # the good image of the refused flush
    o = store.stage_form(s_bad, good, "indexed")
    check_pair(good, img_full, store.read(s_bad), (o_full, o))


def mutate(rnd, s, n):
    x = list(s)
    for p in rnd.sample(range(len(x)), n):
        x[p] = rnd.choice([c for c in "ACGT" if c != x[p]])
    return "".join(x)


def test_queries_answer_the_same(store):
    """six cells in A/B pairs; 40 reads each, cut from the contigs with one to three substitutions, some across a contig's end:
    counts, ov, ext and ext_ret of t4_cellstore_query are equal byte for byte"""
    rnd = random.Random(61)
    cells, reads_of = [], []
    for i in range(6):
        unit = rand_seq(rnd, 40)
        rep = rand_seq(rnd, 25)
        cons = [rand_seq(rnd, 30) + unit + rand_seq(rnd, 20), rand_seq(rnd, 15) + unit + rand_seq(rnd, 40),
                rand_seq(rnd, 20) + rep + rand_seq(rnd, 18) + rep + rand_seq(rnd, 12)]
        assert all(60 <= len(s) <= 120 for s in cons)
        cell = ICell(rnd, 20 + i, cons, [all_marked(s) for s in cons])
        cells.append(cell)
        reads = []
        for j in range(40):
            s = cons[j % 3]
            n = rnd.randrange(36, 56)
            if j % 5 == 4:   # across the contig's end: the tail of the read is not the contig's
                piece = s[len(s) - n + 12:] + rand_seq(rnd, 12)
            else:
                at = rnd.randrange(0, len(s) - n + 1)
                piece = s[at:at + n]
            reads.append(mutate(rnd, piece, rnd.randrange(1, 4)))
        reads_of.append(reads)
        # at least one read meets a key with more than one posting
        assert any(len(cell.lists.get(code_of(r[p:p + K]), ())) > 1 for r in reads for p in range(len(r) - K + 1))
    a = [store.open() for _ in cells]
    b = [store.open() for _ in cells]
    store.reserve(max(a + b), [(c, "full") for c in cells] + [(c, "indexed") for c in cells])
    for c, sa, sb in zip(cells, a, b):
        store.stage_form(sa, c, "full")
        store.stage_form(sb, c, "indexed")
    reads = [r for rs in reads_of for r in rs]
    bcs = [c.barcode for c, rs in zip(cells, reads_of) for _ in rs]
    res_a = store.query([sa for sa, rs in zip(a, reads_of) for _ in rs], reads, bcs)
    res_b = store.query([sb for sb, rs in zip(b, reads_of) for _ in rs], reads, bcs)
    assert res_a[0].sum() > len(reads) // 2   # the reads do overlap their contigs
    for x, y in zip(res_a, res_b):
        assert x.tobytes() == y.tobytes()
