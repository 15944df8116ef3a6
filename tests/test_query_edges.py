"""Reads placed exactly on the capacity and threshold edges of the query kernels, and one step past them, with the REAL capacities
(no testing aid that moves an edge is set). Every case compares the engine through the C ABI with the oracle, and with the
compiled reference when it was built, and asserts which tier or path the read took:
  - rough-annotation / overlap / assign path (runQuery): hit capacity of every LDS tier (1024 / 2048 / 3072 / 4096 / 8192, a read
    of N hits stays in its tier, N + 1 goes to the next), overlap capacity of the tiers (64 / 128 / 128 / 256 / 512: one overlap
    more and the read is pushed on to the next tier);
  - t4_hits: 65 536 hits per read, refused at 65 537;
  - the repeat-skip rule of GetHitsFromRead: lists of 99 and 100 postings, the first and the last k-mer, skipLimit running out;
  - lists of exactly 10 000 and 10 001 postings: answered, or refused loudly where only the wide query could answer;
  - possibleOverlapCnt: 100 / 101 groups of four or more hits (single-workgroup tiers and the wide query), 1000 / 1001 (GPU);
  - AddRead query path: the wide query's threshold T4_WIDE_MIN_HITS (3072 / 3073 hits), ExtendOverlap deferral (16 / 17 overlaps,
    t4_add_query_defer_stats), the LDS tier's 512 overlaps (513: global scratch inside the launch, t4_add_query_stats[3]).
The CPU suite runs every case but t4_hits' 65 536 and the 1000-group classes on the emulator build; `-m gpu` runs all of them on
the GPU."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import edge_gen as G
import t4check
from t4libs import Ref

AIDS = ("T4_AQ_CAP_LIMIT", "T4_WIDE_PCAP", "T4_WIDE_PARTS", "T4_WIDE_GROUPS", "T4_WIDE_MIN_HITS", "T4_AQ_EXTEND_DEFER", "T4_WIDE_OFF",
        "T4_AQ_FORCE_GLOBAL", "T4_STATIC_STRIDE")
TIER_CAP = (1024, 2048, 3072, 4096, 8192)


@pytest.fixture
def real_caps(monkeypatch):
    for a in AIDS:
        monkeypatch.delenv(a, raising=False)
    return monkeypatch


def make_engine(emulated):
    if emulated:
        os.environ["T4_LIB"] = t4check.build_emulator_lib()
    else:
        os.environ.pop("T4_LIB", None)
    import trust4_amd
    return trust4_amd.Engine(0)


@pytest.fixture(params=[True, pytest.param(False, marks=pytest.mark.gpu)], ids=["emu", "gpu"])
def eng(request, real_caps):
    e = make_engine(request.param)
    e.emulated = request.param
    yield e
    e.close()
    os.environ.pop("T4_LIB", None)


def checkers(es):
    return [es.o] + ([es.ref()] if Ref.available() else [])


def landed(eng):
    """reads of the last runQuery call per tier list: five LDS tiers, then the global-scratch tier"""
    return eng.stats()["tier_reads"]


def tiers(*pairs):
    out = [0] * 6
    for t, n in pairs:
        out[t] += n
    return out


def check_overlap_path(eng, ix, reads, chk, expect_tiers, room=128):
    """t4_overlaps, ExtendOverlap of every returned overlap (factors 1 and 2), t4_assign and t4_assign_strands against every checker;
    the tier lists of the overlaps call and of the assign call are `expect_tiers`"""
    b = eng.upload(reads)
    cnt, ov = ix.overlaps(b, 0, 0, room)
    assert landed(eng) == expect_tiers
    for o in chk:
        assert t4check.check_overlaps(cnt, ov, reads, o) == []
    m = min(room, 128)   # (t4_extend takes up to 128 overlaps of a read)
    for factor in (1.0, 2.0):
        ret, ext = ix.extend(b, np.minimum(cnt, m), np.ascontiguousarray(ov[:, :m]), factor)
        for i, rd in enumerate(reads):
            for t in range(min(max(int(cnt[i]), 0), m)):
                o_in = tuple(ov[i, t].tolist())
                for o in chk:
                    eret, eout = o.extend_overlap(rd if o_in[5] == 1 else G.rc(rd), factor, o_in)
                    assert int(ret[i, t]) == eret and tuple(ext[i, t].tolist()) == tuple(eout), (i, t, o_in)
    aret, aout = ix.assign(b, 0)
    assert landed(eng) == expect_tiers
    strands = np.array([(0, 1, -1)[i % 3] for i in range(len(reads))], dtype=np.int32)
    sret, sout = ix.assign_strands(b, strands)
    for o in chk:
        for i, rd in enumerate(reads):
            eret, eout = o.assign_read(rd, 0, -1)
            assert int(aret[i]) == eret and (eret == -1 or tuple(aout[i].tolist()) == tuple(eout)), (i, eret, int(aret[i]))
            eret, eout = o.assign_read(rd, int(strands[i]), -1)
            assert int(sret[i]) == eret and (eret == -1 or tuple(sout[i].tolist()) == tuple(eout)), (i, int(strands[i]))
    return cnt


# ---- hit capacity of every LDS tier (binKernel: H > cap[t] goes up) ---------------------------------------------------------------
@pytest.mark.parametrize("k", [9, 11])
def test_tier_hit_capacity_edges(eng, k):
    t0 = time.time()
    es = G.EdgeSet(k, 31, 100 + k)
    reads = G.reads_with_hits(es, [n + d for n in TIER_CAP for d in (-1, 0, 1)])
    ix = es.commit(eng)
    chk = checkers(es)
    for t, n in enumerate(TIER_CAP):
        # N - 1 and N hits stay in tier t, N + 1 goes to tier t + 1 (the global-scratch tier after 8192)
        cnt = check_overlap_path(eng, ix, reads[3 * t: 3 * t + 3], chk, tiers((t, 2), (t + 1, 1)))
        assert (cnt > 0).all()
    print("tier hit edges k=%d: %.1f s" % (k, time.time() - t0))


def test_annotate_tier_hit_capacity_edges(eng, tmp_path):
    """the same edges on a reference gene set (annotation: no repeat-skip rule)"""
    es = G.RefEdgeSet(9, 17, 7)
    reads = G.ref_reads_with_hits(es, [n + d for n in TIER_CAP for d in (0, 1)])
    ix = es.commit(eng)
    chk = [es.o] + ([es.ref(tmp_path)] if Ref.available() else [])
    for t in range(len(TIER_CAP)):
        rs = reads[2 * t: 2 * t + 2]
        ann = ix.annotate_rough(eng.upload(rs))
        assert landed(eng) == tiers((t, 1), (t + 1, 1))
        for o in chk:
            assert t4check.check_annotate(ann, rs, o) == []
        assert (ann["seqIdx"][:, 0] != -1).all()


# ---- overlap capacity of the tiers (an overflowing read is pushed on to the next tier's list) -----------------------------------
# (overlaps of GetOverlapsFromHits, tier the read's hits bin it to, hits to pad to) -> the tiers it passes through
OV_EDGES = [
    (64, 0, None, [0]), (65, 0, None, [0, 1]),                       # tier 0 holds 64
    (128, 1, None, [1]), (129, 1, None, [1, 2, 3]),                  # tier 1 holds 128, and so does tier 2: on to tier 3
    (256, 3, 3500, [3]), (257, 3, 3500, [3, 4]),                     # tier 3 holds 256
    (512, 4, None, [4]), (513, 4, None, [4, 5]),                     # tier 4 holds 512: on to the global-scratch tier
]


@pytest.mark.parametrize("k", [9, 11])
@pytest.mark.parametrize("edge", range(0, len(OV_EDGES), 2), ids=["tier0", "tier1-2", "tier3", "tier4"])
def test_tier_overlap_capacity_edges(eng, edge, k):
    t0 = time.time()
    es = G.EdgeSet(k, 17, 300 + edge + k)
    cases = OV_EDGES[edge: edge + 2]
    reads = [G.read_with_overlaps(es, n, hits=pad) for n, _, pad, _ in cases]
    ix = es.commit(eng)
    chk = checkers(es)
    for (n, t, _, path), rd in zip(cases, reads):
        h = es.hits(rd)
        assert (t == 0 or h > TIER_CAP[t - 1]) and h <= TIER_CAP[t], (n, h)   # binned to tier t by its hits
        check_overlap_path(eng, ix, [rd], chk, tiers(*[(x, 1) for x in path]), room=1024)
    print("overlap edges %s: %.1f s" % (cases, time.time() - t0))


# ---- the repeat-skip rule of GetHitsFromRead (SeqSet.hpp:1381-1391): lists of 100+ postings ------------------------------------
def test_repeat_skip_rule_edges(eng):
    k = 9
    es = G.EdgeSet(k, 31, 55)
    reads = [es.new_read() for _ in range(5)]
    # one list grown to `size` at each of the given positions of the read
    plan = [([70], 99), ([70], 100), ([0, 141], 100), ([60, 61, 62, 63, 64, 65], 100), ([60, 61, 62, 63, 64, 65], 99)]
    for rd, (pos, _) in zip(reads, plan):
        for c in range(3):
            es.copy_of(rd, reverse=c == 1)
    for rd, (pos, size) in zip(reads, plan):
        for p in pos:
            km = rd[p: p + k]
            while es.list_size(km) < size:
                es.add(km)
            assert es.list_size(km) == size
    ix = es.commit(eng)
    chk = checkers(es)
    skipped = []
    for rd, (pos, size) in zip(reads, plan):
        h = es.o.hits(rd, strand=1, cap=1 << 20)
        skipped.append(sorted(set(pos) - set(h[:, 2].tolist())))
    # skipLimit = k / 2 = 4 on a contig set: 99 postings are never skipped, 100 are -- but not at the first or the last k-mer, and
    # not a fifth one in a row
    assert skipped == [[], [70], [], [60, 61, 62, 63, 65], []], skipped
    b = eng.upload(reads)
    for sk in (0, 1):
        off, hits = ix.hits(b, 0, sk)
        for o in chk:
            assert t4check.check_hits(off, hits, reads, o, allow_total_skip=sk) == []
        cnt, ov = ix.overlaps(b, 0, sk, 128)
        for o in chk:
            assert t4check.check_overlaps(cnt, ov, reads, o, skip_repeats=sk) == []
    for strand in (1, -1):
        off, hits = ix.hits(b, strand, 0)
        for o in chk:
            assert t4check.check_hits(off, hits, reads, o, strand=strand) == []
    check_overlap_path(eng, ix, reads, chk, tiers((0, 5)))


# ---- lists of 10 000 and 10 001 postings (SeqSet.hpp:802, 876, 936) -------------------------------------------------------------
def long_list_set(size):
    """read = P (19 bases) + Q: contig A is P alone, and k-mers 0, 5 and 10 of the read (the ones the repeat-skip rule lets through
    when every k-mer between them has 100+ postings) hold `size` postings; contig B is a copy of Q (hits of short lists). Beyond
    10000 postings the reference removes A's group, which has no hit of a shorter list (removeOnlyRepeats, SeqSet.hpp:802-811)."""
    k = 9
    es = G.EdgeSet(k, 17, 77)
    rd = es.new_read(80)
    es.add(rd[:19])
    es.add(rd[19:])
    for p in range(11):
        km = rd[p: p + k]
        want = size if p in (0, 5, 10) else 100
        for _ in range(want - es.list_size(km)):
            es.add(km)
        assert es.list_size(km) == want
    h = es.o.hits(rd, strand=1, cap=1 << 20)
    assert sorted(set(h[:, 2].tolist()) & set(range(11))) == [0, 5, 10]
    return es, rd


def test_lists_of_10000_postings_on_a_contig_set(eng):
    """runQuery has no wide query: a read with a list of 10 000 postings is answered like the reference, one with a list of 10 001
    (where the reference's removeOnlyRepeats begins) is refused loudly by every runQuery call"""
    import trust4_amd
    for size in (10000, 10001):
        es, rd = long_list_set(size)
        ix = es.commit(eng)
        if size == 10000:
            cnt = check_overlap_path(eng, ix, [rd], checkers(es), tiers((5, 1)))
            assert cnt[0] == 2
        else:
            assert es.o.overlaps_from_read(rd)[0] == 1   # A's group removed
            b = eng.upload([rd])
            for call in (lambda: ix.overlaps(b, 0, 0, 128), lambda: ix.assign(b, 0), lambda: ix.assign_strands(b, [0])):
                with pytest.raises(trust4_amd.T4Error) as e:
                    call()
                assert "posting list beyond 10000" in str(e.value)


def test_lists_of_10000_postings_on_a_reference_set(eng, tmp_path):
    """the rough annotation (no repeat-skip rule on a reference set): a list of 10 000 postings answered, 10 001 refused"""
    import trust4_amd
    for size in (10000, 10001):
        es = G.RefEdgeSet(9, 17, size)
        rd = es.new_read()
        for c in range(3):
            es.add(G.rc(rd) if c == 1 else rd)
        for _ in range(size - es.list_size(rd[:9])):
            es.add(rd[:9])
        assert es.list_size(rd[:9]) == size
        ix = es.commit(eng)
        b = eng.upload([rd])
        if size == 10000:
            ann = ix.annotate_rough(b)
            assert landed(eng) == tiers((5, 1))
            chk = [es.o] + ([es.ref(tmp_path)] if Ref.available() else [])
            for o in chk:
                assert t4check.check_annotate(ann, [rd], o) == []
            assert ann["seqIdx"][0, 0] != -1
        else:
            with pytest.raises(trust4_amd.T4Error) as e:
                ix.annotate_rough(b)
            assert "posting list beyond 10000" in str(e.value)


# ---- AddRead query path -------------------------------------------------------------------------------------------------------
def aq_stats(eng):
    out = (C.c_int64 * 7)()
    eng.lib.t4_add_query_stats(eng.h, out)
    return list(out)


def wide_reads(eng):
    out = (C.c_int64 * 4)()
    eng.lib.t4_add_query_wide_stats(eng.h, out)
    return out[0]


def check_add_query(eng, ix, es, reads, strands, room=256):
    import test_wide_query as W
    factors = [1.0 + (i % 2) for i in range(len(reads))]
    cnt, ov, ex, ret = W.add_query(eng, ix, reads, strands, factors, room)
    for o in checkers(es):
        for i, rd in enumerate(reads):
            eret, lst = o.overlaps_from_read(rd, strand=strands[i], skip_repeats=0, cap=room + 8)
            assert eret == cnt[i] and [tuple(x) for x in ov[i, :max(eret, 0)].tolist()] == [tuple(x) for x in lst], i
            for t in range(max(eret, 0)):
                o_in = tuple(ov[i, t].tolist())
                xret, xout = o.extend_overlap(rd if o_in[5] == 1 else G.rc(rd), factors[i], o_in)
                assert int(ret[i, t]) == xret and tuple(ex[i, t].tolist()) == tuple(xout), (i, t)
    return cnt


def test_add_query_wide_threshold(eng):
    """T4_WIDE_MIN_HITS = 3072: a read of 3072 hits stays in the query kernel, one of 3073 goes to the wide query"""
    es = G.EdgeSet(9, 31, 9)
    reads = G.reads_with_hits(es, [3071, 3072, 3073])
    ix = es.commit(eng)
    for rd, wide in zip(reads, (0, 0, 1)):
        w0, g0 = wide_reads(eng), aq_stats(eng)[3]
        check_add_query(eng, ix, es, [rd], [0])
        assert (wide_reads(eng) - w0, aq_stats(eng)[3] - g0) == (wide, 0)


def reads_with_final_overlaps(es, targets, length=80):
    """reads that GetOverlapsFromRead returns exactly targets[i] overlaps for: copies of the read, a few substitutions each"""
    out = []
    for n in targets:
        rd = es.new_read(length)
        while es.o.overlaps_from_read(rd)[0] < n:
            es.copy_of(rd, subs=es.rnd.randint(0, 1), reverse=es.rnd.random() < 0.5)
        assert es.o.overlaps_from_read(rd)[0] == n
        out.append(rd)
    return out


def deferred_reads(eng):
    out = (C.c_int64 * 1)()
    eng.check(eng.lib.t4_add_query_defer_stats(eng.h, out))
    return out[0]


def test_add_query_extend_deferral_edge(eng):
    """T4_AQ_EXTEND_DEFER = 16: reads of 15 and 16 overlaps extend inside the query kernel, a read of 17 leaves it to extendKernel"""
    es = G.EdgeSet(9, 31, 16)
    reads = reads_with_final_overlaps(es, [15, 16, 17])
    ix = es.commit(eng)
    for rd, strand, n, deferred in zip(reads, (0, 1, 0), (15, 16, 17), (0, 0, 1)):
        assert es.hits(rd) <= 3072   # the query kernel serves it (the wide query leaves every extension to extendKernel)
        d0, w0 = deferred_reads(eng), wide_reads(eng)
        cnt = check_add_query(eng, ix, es, [rd], [strand])
        assert cnt.tolist() == [n] and (deferred_reads(eng) - d0, wide_reads(eng) - w0) == (deferred, 0), (n, deferred_reads(eng) - d0)


def test_add_query_lds_overlap_capacity(eng):
    """the AddRead query's LDS tier holds 8192 hits and 512 overlaps: a read of 513 overlaps (and fewer hits than the wide query's
    threshold) moves to global scratch inside the same launch (t4_add_query_stats[3]); one of 512 stays"""
    es = G.EdgeSet(9, 11, 512)
    reads = [G.read_with_overlaps(es, n, win=11) for n in (512, 513)]
    ix = es.commit(eng)
    for rd, glob in zip(reads, (0, 1)):
        assert es.hits(rd) <= 3072
        w0, g0 = wide_reads(eng), aq_stats(eng)[3]
        check_add_query(eng, ix, es, [rd], [0], room=1024)
        assert (wide_reads(eng) - w0, aq_stats(eng)[3] - g0) == (0, glob)


# ---- possibleOverlapCnt (SeqSet.hpp:815-822): more than 100 / 1000 groups of 4+ hits raise novelMinHitRequired -------------------
def possible_class_set(groups, windows_in_longest, pad=None, seed=3):
    """`groups` contigs that hold 4+ hits of the read on one strand: one made of `windows_in_longest` 18-base windows of the read in
    reverse order (the longest group; its windows chain one by one), the others one window each (10 hits at k = 9)"""
    es = G.EdgeSet(9, 17, seed + groups)
    rd = es.new_read()
    es.add("".join(rd[s: s + 18] for s in range(18 * (windows_in_longest - 1), -1, -18)))
    for i in range(groups - 1):
        st = i % (len(rd) - 18 + 1)
        es.add(rd[st: st + 18])
    if pad:
        es.pad_hits(rd, pad)
    return es, rd


# (groups, windows of the longest group) at N and N + 1: at N every window is an overlap, at N + 1 the raised threshold drops them all
POSSIBLE_EDGES = [((100, 8), (101, 8)), ((1000, 4), (1001, 4))]


def check_possible_classes(eng, edge):
    """single-workgroup tiers: the class edge decides between all the windows' overlaps and none (asserted on the oracle first)"""
    for (groups, w), survive in zip(POSSIBLE_EDGES[edge], (True, False)):
        es, rd = possible_class_set(groups, w)
        n = es.o.overlaps_from_read(rd, cap=4096)[0]
        assert (n >= groups) if survive else n == 0, (groups, n)
        ix = es.commit(eng)
        h = es.hits(rd)
        t = next((i for i, c in enumerate(TIER_CAP) if h <= c), 5)
        if edge == 0:
            check_overlap_path(eng, ix, [rd], checkers(es), tiers((t, 1)))
        else:   # 1000 overlaps: beyond t4_overlaps' 128 records of a read -- counts and records through the AddRead query
            b = eng.upload([rd])
            cnt, _ = ix.overlaps(b, 0, 0, 8)
            assert landed(eng) == tiers((5, 1)) and cnt[0] == n
            check_add_query(eng, ix, es, [rd], [0], room=2048)


def test_possible_overlap_class_100(eng):
    check_possible_classes(eng, 0)


@pytest.mark.gpu
def test_possible_overlap_class_1000(real_caps):
    eng = make_engine(False)
    eng.emulated = False
    try:
        check_possible_classes(eng, 1)
    finally:
        eng.close()


def test_possible_overlap_class_on_the_wide_query(eng):
    """the same 100 / 101 edge on a read the wide query serves (the count is summed over its partitions)"""
    for groups, survive in ((100, True), (101, False)):
        es, rd = possible_class_set(groups, 8, pad=3500)
        n = es.o.overlaps_from_read(rd, cap=4096)[0]
        assert (n >= groups) if survive else n == 0, (groups, n)
        ix = es.commit(eng)
        w0 = wide_reads(eng)
        check_add_query(eng, ix, es, [rd], [0], room=1024)
        assert wide_reads(eng) - w0 == 1


# ---- GPU only: the edges beyond 8192 hits ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_t4_hits_capacity_and_refusal(real_caps):
    """t4_hits holds 65 536 hits of one read; at 65 537 it refuses loudly"""
    import trust4_amd
    eng = make_engine(False)
    try:
        es = G.RefEdgeSet(9, 17, 65)
        reads = G.ref_reads_with_hits(es, [65536, 65537])
        ix = es.commit(eng)
        b = eng.upload(reads[:1])
        off, hits = ix.hits(b, 0, 0)
        assert int(off[-1]) == 65536
        assert t4check.check_hits(off, hits, reads[:1], es.o) == []
        with pytest.raises(trust4_amd.T4Error) as e:
            ix.hits(eng.upload(reads), 0, 0)
        assert "read 1 has more than 65536 hits" in str(e.value)
    finally:
        eng.close()
