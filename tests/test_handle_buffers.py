"""Device memory, pinned memory and events of the long-lived handles (t4_ctx, t4_index, t4_batch, t4_kmer_counter, t4_cellstore)
on their error paths (emulator build: the emulator counts hipMalloc / hipHostMalloc blocks and events and can make one chosen
hipMalloc or hipHostMalloc fail). A case is a list of steps on fresh handles. For every step under test and every allocation k of
it -- device allocations first, then pinned ones -- the step with allocation k failing returns T4_ERR_HIP with a message, the same
step repeated at once on the same handles and every step after it give the bytes of the undisturbed run, and after everything is
destroyed as many device blocks, pinned blocks and events are live as before t4_init."""
import ctypes as C
import gc
import os
import random

import numpy as np
import pytest

import t4check
from test_cell_images import Cell, Store
from test_engine_emu import LiveImage
from test_oneshot_buffers import COMP, CONTIG, K, READS

T4_ERR_HIP = -2
V = C.c_void_p
AIDS = ("T4_AQ_CAP_LIMIT", "T4_AQ_POOL_CAP", "T4_AQ_CAND_CAP", "T4_AQ_FORCE_GLOBAL", "T4_AQ_EXTEND_DEFER", "T4_WIDE_MIN_HITS", "T4_WIDE_PCAP",
        "T4_WIDE_PARTS", "T4_WIDE_GROUPS", "T4_WIDE_OFF", "T4_KC_SLOTS", "T4_LIVE_LANES")


def rand_seq(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


RND = random.Random(7)
CONTIG1 = rand_seq(RND, 60)                       # shares no 9-mer with CONTIG: its posting lists never move
QUERY = READS + [CONTIG1[8:40]]
VARIANTS = [CONTIG[:p] + COMP[CONTIG[p]] + CONTIG[p + 1:] for p in (7, 14, 21, 28, 35, 42, 49)]
FRESH = [rand_seq(RND, 60) for _ in range(2)]
LONG_READS = [rand_seq(RND, 100) for _ in range(8)]


@pytest.fixture(scope="module")
def emu():
    """the emulated library with its bookkeeping hooks; and trust4_amd bound to it"""
    path = t4check.build_emulator_lib()
    os.environ["T4_LIB"] = path
    lib = C.CDLL(path)
    for name in ("hipemu_live_blocks", "hipemu_live_host_blocks", "hipemu_live_events"):
        getattr(lib, name).restype = C.c_longlong
    lib.hipemu_fail_malloc.argtypes = [C.c_longlong]
    lib.hipemu_fail_host_malloc.argtypes = [C.c_longlong]
    saved = {a: os.environ.pop(a) for a in AIDS if a in os.environ}
    gc.collect()   # contexts that earlier modules left to the collector go now, not between two counts
    yield lib
    lib.hipemu_fail_malloc(0)
    lib.hipemu_fail_host_malloc(0)
    os.environ.update(saved)
    os.environ.pop("T4_LIB", None)


def live(emu):
    return emu.hipemu_live_blocks(), emu.hipemu_live_host_blocks(), emu.hipemu_live_events()


def arm(emu, kind, k):
    (emu.hipemu_fail_malloc if kind == "device" else emu.hipemu_fail_host_malloc)(k)


def run(emu, env, case, fail=None):
    """t4_init, the steps of `case` (fail = (step, kind, k): that step with its k-th allocation of that kind failing, then once
    more), destroy everything -> (outputs of the steps, whether the step failed, what stayed live)"""
    import trust4_amd
    gc.collect()
    start = live(emu)
    os.environ.update(env)
    failed = False
    try:
        eng, keep = trust4_amd.Engine(0), []
        try:
            outs = []
            for i, (step, _) in enumerate(case(eng, keep)):
                if fail and fail[0] == i:
                    arm(emu, fail[1], fail[2])
                    try:
                        out, err = step(), None
                    except trust4_amd.api.T4Error as e:
                        out, err = None, e
                    finally:
                        arm(emu, fail[1], 0)
                    if err is not None:
                        failed = True
                        assert err.code == T4_ERR_HIP, (fail, err)
                        assert eng.lib.t4_last_error(eng.h), fail
                        out = step()
                else:
                    out = step()
                outs.append(out)
        finally:
            for o in reversed(keep):
                o.close()
            eng.close()
    finally:
        for a in env:
            os.environ.pop(a, None)
    return outs, failed, tuple(b - a for a, b in zip(start, live(emu)))


# (case, allocation) pairs whose repeated call does not give the undisturbed result for a reason that is not ownership: none
NOT_REPEATABLE = []


def check_case(emu, env, case):
    """-> allocations per kind that were made to fail, over all steps under test"""
    import trust4_amd
    expect, _, left = run(emu, env, case)
    assert left == (0, 0, 0)
    probe = trust4_amd.Engine(0)
    under_test = [inject for _, inject in case(probe, [])]   # (the set-up half of a case makes no handle)
    probe.close()
    bad, made = [], {"device": 0, "pinned": 0}
    for s, inject in enumerate(under_test):
        for kind in ("device", "pinned") if inject else ():
            for k in range(1, 200):
                outs, failed, left = run(emu, env, case, (s, kind, k))
                if not failed:   # the step makes fewer than k allocations of this kind
                    assert outs == expect and left == (0, 0, 0)
                    break
                made[kind] += 1
                if outs != expect and (case.__name__, s, kind, k) not in NOT_REPEATABLE:
                    bad.append("step %d, %s allocation %d: the repeated step or a later one gives another result" % (s, kind, k))
                if left != (0, 0, 0):
                    bad.append("step %d, %s allocation %d: %r device blocks / pinned blocks / events left behind" % (s, kind, k, left))
    assert not bad, bad
    return made


def test_t4_init(emu):
    """every allocation of t4_init failing in turn: no ctx comes out and nothing stays live (the ctx's own destructor frees what was
    made; there is no ctx to ask for a message)"""
    import trust4_amd
    lib = trust4_amd.api._load()
    gc.collect()
    start, made = live(emu), {}
    for kind in ("device", "pinned"):
        for k in range(1, 50):
            h = V(1)
            arm(emu, kind, k)
            rc = lib.t4_init(0, C.byref(h))
            arm(emu, kind, 0)
            if rc == 0:
                lib.t4_destroy(h)
                assert live(emu) == start
                break
            assert rc == T4_ERR_HIP and not h.value, (kind, k, rc, h.value)
            assert live(emu) == start, (kind, k)
            assert lib.t4_init(0, C.byref(h)) == 0 and h.value   # ... and the next one stands
            lib.t4_destroy(h)
            assert live(emu) == start, (kind, k)
        made[kind] = k - 1
    assert made == {"device": 3, "pinned": 1}


def contig_index(eng, keep, consider_barcode=False, barcodes=(-1, -1)):
    ix = eng.index(K, consider_barcode)
    keep.append(ix)
    ix.add_contig("c0", CONTIG, barcodes[0])
    ix.add_contig("c1", CONTIG1, barcodes[1])
    return ix.set_params(K, 10, 0.9)


def query_bytes(res):
    return tuple(res[f].tobytes() for f in ("counts", "status", "stats")) + tuple(None if o is None else o.tobytes() for o in res["ov"])


def served_wide(eng, i):
    g, n, huge, n4 = V(), C.c_int(0), C.c_int(0), C.c_int(0)
    eng.lib.t4_add_query_groups.restype = C.c_int
    return eng.lib.t4_add_query_groups(eng.h, i, C.byref(g), C.byref(n), C.byref(huge), C.byref(n4)) == 1


def case_add_query(eng, keep):
    """a whole AddRead query call with candidates on a fresh ctx: blobs, pools, scratch, the wide pools when the route is on"""
    def setup():
        contig_index(eng, keep).commit()

    def call():
        res = eng.add_query_whole(keep[0], READS)
        assert (res["counts"] > 0).all()
        return query_bytes(res) + tuple(served_wide(eng, i) for i in range(len(READS)))
    return [(setup, False), (call, True)]


def test_add_query_single_workgroup(emu):
    made = check_case(emu, {}, case_add_query)
    # device: the two blobs, the record copies of the extension launch (2), DP scratch (2), the global-scratch tier (5), and the 16
    # pools of the wide query, which are made whenever the route is open; pinned: the blobs' twins, the result pool, the candidate
    # pool, the wide query's head bitmaps and dependency records
    assert made == {"device": 11 + 16, "pinned": 4 + 2}
    assert run(emu, {}, case_add_query)[0][1][-2:] == (False, False)


def test_add_query_both_reads_wide(emu):
    env = {"T4_WIDE_MIN_HITS": "1", "T4_WIDE_PCAP": "64"}
    made = check_case(emu, env, case_add_query)
    assert made == {"device": 11 + 16, "pinned": 4 + 2}
    assert run(emu, env, case_add_query)[0][1][-2:] == (True, True)


def test_add_query_pools_grow_and_repeat(emu):
    env = {"T4_AQ_POOL_CAP": "1", "T4_AQ_CAND_CAP": "1"}
    made = check_case(emu, env, case_add_query)
    assert made["pinned"] >= 6   # both pools at least twice
    assert run(emu, env, case_add_query)[0][1] == run(emu, {}, case_add_query)[0][1]


def flush(img, ix, junk=0):
    """LiveImage.flush, with `junk` more bases behind the last contig (nobody reads them: they make the delta large)"""
    if not junk:
        return img.flush(ix)
    at = img.bases_used
    img.bases_used += junk
    keys = img.keys if img.rebuilt else {c: img.keys[c] for c in img.dirty_keys}
    slots = [(e[0], c, e[1], e[2]) for c, e in keys.items()]
    runs = [(at_, [img.post[at_]]) for at_ in sorted(img.dirty_post)]
    seqs = [(i, img.seqs[i][0], len(img.seqs[i][1]), -1, img.seqs[i][3]) for i in sorted(img.dirty_seq)]
    bases = [(img.seqs[i][0], img.seqs[i][1].encode() + b"\0", img.seqs[i][2]) for i in sorted(img.dirty_seq)] + [(at, b"A" * junk, b"\x01" * junk)]
    ix.apply_delta(img.slots, 1 if img.rebuilt else 0, len(img.post) + 8, img.bases_used + 8, len(img.seqs) + 4, len(img.seqs),
                   max(len(x[1]) for x in img.seqs), slots, runs, seqs, bases)
    img.dirty_keys, img.dirty_post, img.dirty_seq, img.rebuilt = set(), set(), set(), False


def sorted_hits(ix, b):
    off, hits = ix.hits(b, 0, 0)
    rows = [t4check.hits_as_sorted_rows(off, hits, i) for i in range(b.n)]   # (the order among a read's hits is the posting order: any)
    return off.tobytes(), tuple(m[np.lexsort(m.T[::-1])].tobytes() for m in rows)


def case_apply_delta(eng, keep):
    """three deltas of a live set, each followed by queries of reads whose contigs the delta did not ship again (what growKeep
    copied); the answers are held against an index of the same contigs made by t4_index_commit"""
    img, names = LiveImage(K, 512), []
    state = {}

    def setup():
        ix = eng.index(K).set_params(K, 10, 0.9)
        keep.append(ix)
        keep.append(eng.upload(QUERY))

    def delta(contigs, junk, slots):
        def step():
            if state.get("added") is not contigs:   # (once, also when the step is repeated)
                for s in contigs:
                    names.append("c%d" % len(names))
                    img.add(names[-1], s)
                state["added"] = contigs
            flush(img, keep[0], junk)
            assert img.slots == slots
        return step

    def observe():
        ix, b = keep[0], keep[1]
        ref = eng.index(K).set_params(K, 10, 0.9)
        for nm, (_, cons, _, _) in zip(names, img.seqs):
            ref.add_contig(nm, cons)
        ref.commit()
        try:
            got = sorted_hits(ix, b)
            cnt, ov = ix.overlaps(b, 0, 0, 16)
            assert got == sorted_hits(ref, b) and (cnt > 0).all()
            rcnt, rov = ref.overlaps(b, 0, 0, 16)
            assert cnt.tobytes() == rcnt.tobytes() and ov.tobytes() == rov.tobytes()
        finally:
            ref.close()
        return got, cnt.tobytes(), ov.tobytes()
    # first delta: every array and the staging pair; second: more postings, bases, sequences than there is room for and a delta
    # beyond the staging buffer's first megabyte; third: a table of another size
    return [(setup, False), (delta([CONTIG, CONTIG1], 0, 512), True), (observe, False), (delta(VARIANTS, 600000, 512), True), (observe, False),
            (delta(FRESH, 0, 1024), True), (observe, False)]


def test_index_apply_delta(emu):
    made = check_case(emu, {}, case_apply_delta)
    # first: table, postings, sequences, bases x 2, staging; second: postings, sequences, bases x 2, staging; third: table
    assert made == {"device": 6 + 5 + 1, "pinned": 1 + 1}


def case_upload_and_commit(eng, keep):
    """t4_reads_upload_flags with barcodes; t4_index_commit with a direct table and with a hashed one"""
    bases, offs, bcs = np.frombuffer("".join(QUERY).encode(), np.uint8), np.cumsum([0] + [len(r) for r in QUERY]).astype(np.int64), np.array([3, 3, 4], np.int32)
    made = []

    class Made:
        n = len(QUERY)

        def close(self):
            for h in made:
                eng.lib.t4_batch_destroy(h)

    def setup():
        contig_index(eng, keep, False, (3, 4))
        contig_index(eng, keep, True, (3, 4))

    def upload():
        h = V(1)
        rc = eng.lib.t4_reads_upload_flags(eng.h, bases.ctypes.data_as(V), offs.ctypes.data_as(V), bcs.ctypes.data_as(V), len(QUERY), 0, C.byref(h))
        assert (rc == 0) == bool(h.value)   # no batch comes out of a failed call
        eng.check(rc)
        made.append(h)
        if len(keep) < 3:
            keep.append(Made())
        keep[2].h = h

    def commit(which):
        return lambda: keep[which].commit() and None

    def observe():
        out = []
        for ix in keep[:2]:
            off, hits = ix.hits(keep[2], 0, 0)
            assert (np.diff(off) > 0).all()
            out.append((off.tobytes(), hits.tobytes()))
        return out
    return [(setup, False), (upload, True), (commit(0), True), (commit(1), True), (observe, False)]


def test_upload_flags_and_index_commit(emu):
    made = check_case(emu, {}, case_upload_and_commit)
    assert made == {"device": 4 + 5 + 5, "pinned": 0}


def case_cellstore(eng, keep):
    """prepare, two cells staged (one in full, one as compact key records), flush, patch, flush, read_image"""
    rnd = random.Random(11)
    cells = [Cell(rnd, bc, [(c, 1 + c % 3) for c in rnd.sample(range(1 << 18), 40)], nseq=1) for bc in (3, 4)]
    eng.lib.t4_cellstore_patch.restype, eng.lib.t4_cellstore_patch.argtypes = C.c_int, [V, C.c_int, C.c_int, V, V]
    slots, o_pw = [], {}

    def setup():
        keep.append(Store(eng))
        slots.extend(keep[0].open() for _ in cells)

    def prepare():
        keep[0].prepare(max(slots), cells)

    def stage(i):
        def step():
            o_pw[i] = keep[0].stage(slots[i], cells[i], compact=bool(i))
        return step

    def read(i):
        def step():   # (t4_cellstore_read_image flushes first)
            buf, view = keep[0].read(slots[i])
            return buf.tobytes(), tuple(getattr(view, f) for f in view.SCALARS if f not in ("table", "htab")), tuple(getattr(view, f) - view.ctab for f in view.POINTERS)
        return step

    def patch():
        offs, vals = np.array([o_pw[0], o_pw[0] + 3], np.int64), np.array([0xA5, 0x5A], np.uint8)
        eng.check(eng.lib.t4_cellstore_patch(keep[0].h, slots[0], 2, offs.ctypes.data_as(V), vals.ctypes.data_as(V)))
    return [(setup, False), (prepare, True), (stage(0), True), (stage(1), True), (read(0), True), (patch, True), (read(0), True), (read(1), False)]


def test_cellstore(emu):
    made = check_case(emu, {}, case_cellstore)
    # prepare: the views and the staging pair; stage: the arena's first chunk; flush: descriptors, the build error word and its
    # pinned copy; the flush after the patch: the patch records
    assert made == {"device": 2 + 1 + 2 + 1, "pinned": 1 + 1}
    outs = run(emu, {}, case_cellstore)[0]
    before, after = np.frombuffer(outs[4][0], np.uint8), np.frombuffer(outs[6][0], np.uint8)
    assert (before != after).sum() == 2 and outs[4][1:] == outs[6][1:]   # the patch landed, and nothing else moved


def case_kmer_counter(eng, keep):
    """create, add past the first table's load, merge another read set's k-mers past the second table's"""
    codes, vals = np.arange(1, 3001, dtype=np.uint64) * np.uint64(77), np.arange(3000, dtype=np.int32) % 5 + 1

    def setup():
        keep.append(eng.upload(LONG_READS))

    def create():
        kc = eng.kmer_counter(K, max_kmers=1 << 16)
        keep.append(kc)

    def add():
        keep[1].add(keep[0])

    def merge():
        keep[1].merge(codes, vals, only_present=False)

    def observe():
        c, v = keep[1].export()
        o = np.argsort(c)
        assert len(c)
        return c[o].tobytes(), v[o].tobytes()
    return [(setup, False), (create, True), (add, True), (observe, False), (merge, True), (observe, False)]


def test_kmer_counter(emu):
    made = check_case(emu, {"T4_KC_SLOTS": "1024"}, case_kmer_counter)
    assert made["device"] >= 4 + 2 + 2 and made["pinned"] == 0   # the four blocks; one rehash of add at least; one of merge at least


def whole_run(emu, env, play):
    import trust4_amd
    gc.collect()
    start = live(emu)
    os.environ.update(env)
    try:
        eng = trust4_amd.Engine(0)
        try:
            play(eng)
        finally:
            eng.close()
    finally:
        for a in env:
            os.environ.pop(a, None)
    assert live(emu) == start


def test_assembler_with_two_lanes_leaves_nothing(emu):
    """an undisturbed builder over a few reads, with a second query lane (a lane owns a ctx and a device image of the set)"""
    def play(eng):
        import trust4_amd
        asm = trust4_amd.Assembler(eng, K)
        for i, s in enumerate([CONTIG, CONTIG1] + FRESH):
            assert asm.input_novel_read("C%d" % i, s, 1, -1) >= 0
        reads = QUERY + [FRESH[0][5:45], FRESH[1][10:50]] + QUERY
        rets, events = [], emu.hipemu_live_events()
        for i, rd in enumerate(reads):
            if not asm.window_valid():
                asm.prefetch(reads[i:i + 3], [0] * len(reads[i:i + 3]))
            rets.append(asm.add_read(rd, "", 0, -1, 1, 0, 0.9)[0])
        asm.update_all_consensus()
        assert sum(1 for r in rets if r >= 0) >= len(QUERY), rets
        assert emu.hipemu_live_events() >= events + 4 + 1   # the second lane's ctx; the image of a lane that has queried
        asm.close()
    whole_run(emu, {"T4_LIVE_LANES": "2"}, play)


def test_cellset_over_two_barcodes_leaves_nothing(emu):
    def play(eng):
        import trust4_amd
        cs = trust4_amd.CellSet(eng, K, 13)
        for bc, s in enumerate([CONTIG, CONTIG1]):
            assert cs.cell(bc).input_novel_read("Novel", s, 1, bc) == 0
        cs.prefetch([0, 1], [CONTIG[5:] + "ACGTAC", CONTIG1[5:] + "ACGTAC"], [0, 0])
        for bc, s in enumerate([CONTIG, CONTIG1]):
            assert cs.cell(bc).add_read(s[5:] + "ACGTAC", "", 0, bc, 1, 0, 0.9)[0] == 0
        cs.update_all_consensus()
        cs.close()
    whole_run(emu, {}, play)
