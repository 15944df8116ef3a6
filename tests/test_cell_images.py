"""Per-barcode set images whose hash table is built on the device (t4_cellstore_stage_compact + cellTableBuildKernel) against the
images the host writes in full (t4_cellstore_stage, the yardstick): the same synthetic cell goes into slot A whole and into slot B
as compact key records, both slots are read back (t4_cellstore_read_image) and compared:
  (a) everything from the postings to the end of the image is byte-equal, the views are equal apart from the base pointers;
  (b) the two tables have the same number of slots and hold the same map {code: (start, cnt)};
  (c) in B every key is reachable from mix64(code) & mask without crossing an empty slot, every other slot is exactly (~0, 0, 0).
On the emulator build of the kernels and, marked gpu, through libt4hip.so."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import t4check

T4_ERR_ARG = -1
M64 = (1 << 64) - 1
ENT = np.dtype([("code", "<u8"), ("start", "<u4"), ("cnt", "<u4")])   # T4HashEntC


def mix64(z):
    """t4k::mix64 (trust4_amd/csrc/t4_kernels.h)"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def table_slots(nkeys):
    sz = 64
    while 2 * sz < 3 * nkeys + 2:
        sz <<= 1
    return sz


class View(C.Structure):   # T4IndexView (trust4_amd/csrc/t4_device.h), 128 bytes
    _fields_ = ([(n, C.c_int) for n in ("k", "nseq", "direct", "considerBarcode")] + [("hashMask", C.c_uint64)] +
                [(n, C.c_uint64) for n in ("table", "htab", "post", "seqs", "cons", "pw", "ctab")] +
                [(n, C.c_int) for n in ("radius", "hitLenRequired", "nomatchGapLimit", "firstIsRef", "hasNovel", "key32")] +
                [(n, C.c_double) for n in ("novelSim", "refSim", "repeatSim")])

    SCALARS = ("k", "nseq", "direct", "considerBarcode", "hashMask", "table", "htab", "radius", "hitLenRequired", "nomatchGapLimit",
               "firstIsRef", "hasNovel", "key32", "novelSim", "refSim", "repeatSim")
    POINTERS = ("post", "seqs", "cons", "pw")   # relative to ctab, the base of the image


assert C.sizeof(View) == 128


class Cell:
    """one synthetic cell: contigs with posWeight counts, keys (code, cnt) with `cnt` postings each"""

    def __init__(self, rnd, barcode, key_cnts, nseq=2):
        self.barcode, self.nseq = barcode, nseq
        self.cons = ["".join(rnd.choice("ACGT") for _ in range(rnd.randrange(20, 70))) for _ in range(nseq)]
        self.names = ["IGHV", "TRBC", "", "IGKJ"][:nseq] + ["Novel"] * max(0, nseq - 4)
        self.pw = [np.array([rnd.randrange(0, 6) for _ in range(4 * len(s))], dtype=np.int32) for s in self.cons]
        self.codes = [c for c, _ in key_cnts]
        self.cnts = [n for _, n in key_cnts]
        self.post = np.array([v for _, n in key_cnts for _ in range(n) for v in (rnd.randrange(nseq), rnd.randrange(0, 60))], dtype=np.int32)
        self.expect, at = {}, 0
        for c, n in key_cnts:
            if n > 0:
                self.expect[c] = (at, n)
                at += n
        self.npost = at

    def sizes(self):
        return self.nseq, len(self.codes), self.npost, sum(len(s) + 1 for s in self.cons)


class Store:
    """the internal t4_cellstore entry points (trust4_amd/csrc/t4_internal.h) of the library the engine loaded"""

    def __init__(self, eng, k=9):
        self.eng, lib = eng, eng.lib
        P, I, L, Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
        stage = [P, I, I, I, P, P, P, L, P, P, P, P, P, P]
        for name, res, args in (("t4_cellstore_create", I, [P, I, C.POINTER(P)]), ("t4_cellstore_destroy", None, [P]),
                                ("t4_cellstore_open", I, [P, C.POINTER(I)]), ("t4_cellstore_close", I, [P, I]),
                                ("t4_cellstore_stage", I, stage), ("t4_cellstore_stage_compact", I, stage),
                                ("t4_cellstore_image_bytes", Z, [I, L, L, L]), ("t4_cellstore_full_image_bytes", Z, [I, L, L, L]),
                                ("t4_cellstore_prepare", I, [P, I, Z]), ("t4_cellstore_image_stats", I, [P, P]),
                                ("t4_cellstore_read_image", I, [P, I, P, Z, C.POINTER(Z), P])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        self.lib = lib
        self.h = P()
        eng.check(lib.t4_cellstore_create(eng.h, k, C.byref(self.h)))

    def close(self):
        if self.h:
            self.lib.t4_cellstore_destroy(self.h)
            self.h = None

    def open(self):
        s = C.c_int(-1)
        self.eng.check(self.lib.t4_cellstore_open(self.h, C.byref(s)))
        return s.value

    def prepare(self, max_slot, cells):
        """room for every cell of `cells` once in full and once compact"""
        need = sum(self.lib.t4_cellstore_full_image_bytes(*c.sizes()) + self.lib.t4_cellstore_image_bytes(*c.sizes()) for c in cells)
        self.eng.check(self.lib.t4_cellstore_prepare(self.h, max_slot, need))

    def stage(self, slot, cell, compact):
        n = cell.nseq
        names = (C.c_char_p * n)(*[x.encode() for x in cell.names])
        cons = (C.c_char_p * n)(*[x.encode() for x in cell.cons])
        pw = (C.c_void_p * n)(*[a.ctypes.data for a in cell.pw])
        code = np.array(cell.codes, dtype=np.uint64)
        bucket = np.array([(c + cell.barcode + 1) % 1000003 for c in cell.codes], dtype=np.int32)
        cnt = np.array(cell.cnts, dtype=np.int32)
        o_pw = C.c_int64(-1)
        fn = self.lib.t4_cellstore_stage_compact if compact else self.lib.t4_cellstore_stage
        rc = fn(self.h, slot, cell.barcode, n, C.cast(names, C.c_void_p), C.cast(cons, C.c_void_p), C.cast(pw, C.c_void_p), len(cell.codes),
                code.ctypes.data, bucket.ctypes.data, cnt.ctypes.data, cell.post.ctypes.data, C.addressof(o_pw), None)
        self.eng.check(rc)
        return o_pw.value

    def read_rc(self, slot):
        n = C.c_size_t(0)
        view = View()
        rc = self.lib.t4_cellstore_read_image(self.h, slot, None, 0, C.byref(n), C.addressof(view))
        if rc:
            return rc, None, None
        buf = np.zeros(n.value, dtype=np.uint8)
        rc = self.lib.t4_cellstore_read_image(self.h, slot, buf.ctypes.data, buf.nbytes, C.byref(n), C.addressof(view))
        return rc, buf, view

    def read(self, slot):
        rc, buf, view = self.read_rc(slot)
        self.eng.check(rc)
        return buf, view

    def stats(self):
        v = (C.c_int64 * 4)()
        self.eng.check(self.lib.t4_cellstore_image_stats(self.h, C.cast(v, C.c_void_p)))
        return list(v)


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
    s = Store(eng)
    yield s
    s.close()


def table_of(img, view):
    sz = view.hashMask + 1
    assert sz & (sz - 1) == 0 and view.post - view.ctab == 16 * sz   # the postings follow the table
    return np.frombuffer(img[:16 * sz].tobytes(), dtype=ENT)


def table_map(tab):
    live = tab[tab["code"] != M64]
    m = {int(e["code"]): (int(e["start"]), int(e["cnt"])) for e in live}
    assert len(m) == len(live)   # no code twice
    return m


def check_pair(cell, full, compact, o_pw):
    (img_a, va), (img_b, vb) = full, compact
    o_post = va.post - va.ctab
    assert len(img_a) == len(img_b) and o_post % 16 == 0
    # (a) the image behind the table, and the views apart from the base pointers
    assert bytes(img_a[o_post:]) == bytes(img_b[o_post:])
    for f in View.SCALARS:
        assert getattr(va, f) == getattr(vb, f), f
    for f in View.POINTERS:
        assert getattr(va, f) - va.ctab == getattr(vb, f) - vb.ctab, f
    assert va.ctab != vb.ctab and va.ctab % 16 == 0 and vb.ctab % 16 == 0
    assert va.pw - va.ctab == o_pw[0] == o_pw[1]
    assert va.seqs - va.post >= 8 * cell.npost
    # (b) the same table size, the same map -- the one the key list describes
    ta, tb = table_of(img_a, va), table_of(img_b, vb)
    assert len(ta) == len(tb) == table_slots(len(cell.codes))
    assert table_map(ta) == table_map(tb) == cell.expect
    # (c) every key of B reachable from its home slot before an empty one; every slot without a key is exactly (~0, 0, 0)
    mask = len(tb) - 1
    codes = tb["code"]
    for c in cell.expect:
        s = mix64(c) & mask
        for _ in range(len(tb)):
            assert codes[s] != M64, "key %d behind an empty slot" % c
            if codes[s] == c:
                break
            s = (s + 1) & mask
        else:
            raise AssertionError("key %d not found" % c)
    empty = tb[codes == M64]
    assert len(empty) == len(tb) - len(cell.expect) and not empty["start"].any() and not empty["cnt"].any()


def run_pairs(store, cells):
    """every cell staged in full into a slot of its own and compact into another, ONE flush, all read back and compared"""
    a = [store.open() for _ in cells]
    b = [store.open() for _ in cells]
    store.prepare(max(a + b), cells)
    before = store.stats()
    o_pw = [(store.stage(sa, c, False), store.stage(sb, c, True)) for c, sa, sb in zip(cells, a, b)]
    for c, sa, sb, o in zip(cells, a, b, o_pw):
        check_pair(c, store.read(sa), store.read(sb), o)
    after = store.stats()
    assert after[0] - before[0] == len(cells)
    assert after[1] - before[1] == sum(len(c.expect) for c in cells)
    assert after[2] - before[2] == sum(16 * table_slots(len(c.codes)) for c in cells)
    full = sum(store.lib.t4_cellstore_full_image_bytes(*c.sizes()) for c in cells)
    assert after[3] - before[3] == full + sum(store.lib.t4_cellstore_image_bytes(c.nseq, len(c.expect), c.npost, c.sizes()[3]) for c in cells)
    assert 2 * full > after[3] - before[3]   # the compact form is the smaller one
    return a, b


def distinct_codes(rnd, n, bits=18):
    return rnd.sample(range(1 << bits), n)


def codes_with_home(home, n, mask, start=0):
    out, c = [], start
    while len(out) < n:
        if mix64(c) & mask == home:
            out.append(c)
        c += 1
    return out


@pytest.mark.parametrize("nkeys", [0, 1, 42, 43])
def test_table_sizes(store, nkeys):
    """0 keys: 64 slots, all empty; 1 key; 42 and 43 keys: the step from 64 to 128 slots (2 * sz < 3 * n + 2)"""
    rnd = random.Random(nkeys)
    cell = Cell(rnd, 3, [(c, rnd.randrange(1, 4)) for c in distinct_codes(rnd, nkeys)])
    assert table_slots(nkeys) == (128 if nkeys == 43 else 64)
    run_pairs(store, [cell])


def test_keys_sharing_one_home_slot(store):
    rnd = random.Random(8)
    cell = Cell(rnd, 0, [(c, rnd.randrange(1, 5)) for c in codes_with_home(17, 8, 63)])
    run_pairs(store, [cell])


def test_probe_wraps_around_the_table_end(store):
    rnd = random.Random(6)
    cell = Cell(rnd, 11, [(c, 2) for c in codes_with_home(63, 6, 63)] + [(c, 1) for c in codes_with_home(0, 2, 63)])
    run_pairs(store, [cell])


def test_key_without_postings_is_left_out(store):
    rnd = random.Random(5)
    codes = distinct_codes(rnd, 9)
    cell = Cell(rnd, 2, [(c, 0 if i in (0, 4, 8) else 3) for i, c in enumerate(codes)])
    assert len(cell.expect) == 6 and cell.npost == 18
    a, b = run_pairs(store, [cell])
    for slot in a + b:
        img, view = store.read(slot)
        m = table_map(table_of(img, view))
        assert codes[0] not in m and codes[4] not in m and codes[8] not in m


def test_several_keys_per_thread(store):
    rnd = random.Random(50)
    cell = Cell(rnd, 77, [(c, 1 + (i % 3 == 0)) for i, c in enumerate(distinct_codes(rnd, 5000))], nseq=5)
    run_pairs(store, [cell])


def test_one_flush_of_more_images_than_workgroups(store, eng):
    """the grid of the build kernel is capped at 8 workgroups per CU: more images than that in ONE flush run its grid-stride loop"""
    n = 300 if eng.emulated else 8 * eng.cus() + 50
    assert n > 8 * eng.cus()
    rnd = random.Random(300)
    sizes = [0, 1, 2, 5, 17, 42, 43, 64, 90]
    cells = [Cell(rnd, i, [(c, rnd.randrange(1, 3)) for c in distinct_codes(rnd, sizes[i % len(sizes)])], nseq=1 + i % 2) for i in range(n)]
    run_pairs(store, cells)


def test_restaged_slot_and_recycled_slot(store):
    """a slot staged again with a smaller, then a larger image (the slot grows), and a closed slot's arena block reused"""
    rnd = random.Random(21)
    a, b = store.open(), store.open()
    for nkeys in (100, 3, 4000):
        cell = Cell(rnd, 9, [(c, 1) for c in distinct_codes(rnd, nkeys)])
        store.prepare(max(a, b), [cell])
        o = (store.stage(a, cell, False), store.stage(b, cell, True))
        check_pair(cell, store.read(a), store.read(b), o)
    store.eng.check(store.lib.t4_cellstore_close(store.h, b))
    b2 = store.open()
    cell = Cell(rnd, 9, [(c, 2) for c in distinct_codes(rnd, 3000)])
    store.prepare(max(a, b2), [cell])
    o = (store.stage(a, cell, False), store.stage(b2, cell, True))
    check_pair(cell, store.read(a), store.read(b2), o)


def test_duplicate_code_is_refused(store):
    """the same code twice: the device build meets its own code in the table, sets the flag and stops probing; the flush reports
    T4_ERR_ARG naming the slot, and the store goes on"""
    rnd = random.Random(13)
    codes = distinct_codes(rnd, 20)
    bad = Cell(rnd, 4, [(c, 1) for c in codes + [codes[7]]])
    good = Cell(rnd, 5, [(c, 2) for c in codes])
    s_good, s_bad = store.open(), store.open()
    store.prepare(s_bad, [bad, good])
    store.stage(s_good, good, True)
    store.stage(s_bad, bad, True)
    rc, _, _ = store.read_rc(s_good)   # the flush
    assert rc == T4_ERR_ARG
    msg = store.lib.t4_last_error(store.eng.h).decode()
    assert "slot %d" % s_bad in msg and "twice" in msg, msg
    # the good image of the same flush is whole, and the slot of the refused one takes a new image
    img, view = store.read(s_good)
    assert table_map(table_of(img, view)) == good.expect
    s_full = store.open()
    store.prepare(max(s_full, s_bad), [good])
    o = (store.stage(s_full, good, False), store.stage(s_bad, good, True))
    check_pair(good, store.read(s_full), store.read(s_bad), o)
