"""The wide AddRead query for `--trimLevel 2`: skipRepeats queries (GetOverlapsFromRead with repetitiveData, SeqSet.hpp:1508-1556: a
first pass that drops every list of 100 or more postings and runs GetOverlapsFromHits with filter 0, then -- only when that pass
finds no overlap -- the plain pass) and reads that carry a barcode on an index that is not keyed by barcode (postings of contigs with
another barcode are no hits, every hit counts repeats = 1: SeqSet.hpp:1406-1418). Both used to keep the single-workgroup limits, so a
read that met a list of more than 10 000 postings was refused. Every case compares t4_add_query / t4_assign_wide with the oracle, and
with the compiled reference when it was built, records and doubles with ==, after asserting on the oracle that its input is what it is
meant to be:
  1  second pass on lists of 10 000 / 10 001 postings after an empty first pass (skip_repeats = 1, no barcode)
  2  removeOnlyRepeats after an empty first pass: one overlap at 10 000, none at 10 001
  3  a first pass that is not empty: the second never runs, nothing goes wide with the real capacities
  4  barcoded reads on a set that is not keyed by barcode, through t4_add_query and t4_assign_wide
  5  route against route on a random set: real capacities, a small tier capacity, small wide pools -- byte-identical
The CPU suite runs every case on the emulator build; `-m gpu` runs them on the GPU."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import edge_gen as G
import test_assign_wide as A
import test_query_edges as Q
import test_wide_query as W
from t4libs import Oracle, Ref

AIDS = A.AIDS


@pytest.fixture(params=[True, pytest.param(False, marks=pytest.mark.gpu)], ids=["emu", "gpu"])
def engines(request, monkeypatch):
    """make(**aids) -> an engine created with exactly these testing aids in the environment (most are read once per ctx); the engine
    made last is the one to use"""
    made = []

    def make(**aids):
        for a in AIDS:
            monkeypatch.delenv(a, raising=False)
        for a, v in aids.items():
            monkeypatch.setenv(a, str(v))
        e = A.make_engine(request.param)   # (the aids stay set: the wide pools read theirs when they are first needed)
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()
    os.environ.pop("T4_LIB", None)


class BcSet:
    """a contig set whose contigs carry barcodes, in an Oracle (index not keyed by barcode) -- built from an EdgeSet's contigs"""

    def __init__(self, es, barcode_of):
        self.k, self.hit_len = es.k, es.hit_len
        self.o = Oracle(es.k)
        self.o.set_hit_len_required(es.hit_len)
        self.contigs = []
        self.rnd = random.Random(len(es.contigs))
        for i, (name, s, w) in enumerate(es.contigs):
            self.add(s, barcode_of(i), w, name)

    def add(self, seq, barcode=-1, w=None, name=None):
        if w is None:
            w = np.zeros((len(seq), 4), dtype=np.int32)
            for j, ch in enumerate(seq):
                w[j, "ACGT".index(ch)] = self.rnd.randint(1, 9)
        name = name or "x%d" % len(self.contigs)
        assert self.o.add_novel(name, seq, 1, barcode, w) == len(self.contigs)
        self.contigs.append((name, seq, w, barcode))
        return len(self.contigs) - 1

    def random_seq(self, n):
        return "".join(self.rnd.choice("ACGT") for _ in range(n))

    def commit(self, eng):
        ix = eng.index(self.k)
        for name, s, w, bc in self.contigs:
            ix.add_contig(name, s, bc, w)
        ix.set_params(self.hit_len, 10, 0.9).commit()
        return ix

    def checkers(self):
        out = [self.o]
        if Ref.available():
            r = Ref(self.k)
            for name, s, w, bc in self.contigs:
                r.add_novel(name, s, 1, bc, w)
            r.set_hit_len_required(self.hit_len)
            out.append(r)
        return out


def add_query(eng, ix, reads, strands, barcodes, skip, factors, room):
    from trust4_amd.api import OV_DTYPE
    n = len(reads)
    P = C.c_void_p
    bases = ("".join(reads) or "A").encode()
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    st = np.asarray(strands, dtype=np.int32)
    bc = np.asarray(barcodes, dtype=np.int32)
    fac = np.asarray(factors, dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    ov, ex, ret = np.zeros((n, room), dtype=OV_DTYPE), np.zeros((n, room), dtype=OV_DTYPE), np.zeros((n, room), dtype=np.int32)
    eng.check(eng.lib.t4_add_query(ix.h, n, bases, offs.ctypes.data_as(P), bc.ctypes.data_as(P), st.ctypes.data_as(P), int(skip), fac.ctypes.data_as(P), room,
                                   cnt.ctypes.data_as(P), ov.ctypes.data_as(P), ex.ctypes.data_as(P), ret.ctypes.data_as(P)))
    return cnt, ov, ex, ret


def factors_of(barcodes, skip):
    """ExtendOverlap's mismatch factor as AddRead passes it (SeqSet.hpp:3597-3598)"""
    return [2.0 if (b != -1 or skip) else 1.0 for b in barcodes]


def first_pass(o, rd, strand, barcode, hit_len):
    """the raw overlaps of the first pass of a skipRepeats query: GetHitsFromRead(allowTotalSkip) + GetOverlapsFromHits(filter 0)"""
    return o.overlaps_from_hits(rd, strand=strand, barcode=barcode, allow_total_skip=1, hit_len_required=hit_len, filt=0, cap=1 << 14)


def deciding_hits(o, rd, strand, barcode, skip, hit_len):
    """the hit array of the pass whose overlaps GetOverlapsFromRead goes on with"""
    first = bool(skip) and len(first_pass(o, rd, strand, barcode, hit_len)) > 0
    return o.hits(rd, strand=strand, barcode=barcode, allow_total_skip=1 if first else 0, cap=1 << 22)


def expected_groups(h, length):
    """the dependency records the wide query returns (test_wide_query.expected_groups) of a hit array"""
    tab = {}
    for idx, off, roff, st, _rep in h.tolist():
        d = tab.setdefault(idx * 2 + (1 if st == 1 else 0), {})
        d[off - roff] = d.get(off - roff, 0) + 1
    out = []
    for key in sorted(tab, key=lambda x: (x & 1, x >> 1)):
        ats = [at for at, c in tab[key].items() if c >= 3]
        lo, hi = (min(ats), max(ats) + length - 1) if ats else (0x7FFFFFFF, -0x7FFFFFFF)
        out.append((key, sum(tab[key].values()), lo, hi))
    return out


def check_query(eng, chk, ix, hit_len, reads, strands, barcodes, skip, room=64):
    """one t4_add_query call against every checker: counts, overlap records, the ExtendOverlap of every record; the dependency records
    of every read the wide query served -> (result arrays, rows the wide query served)"""
    factors = factors_of(barcodes, skip)
    res = add_query(eng, ix, reads, strands, barcodes, skip, factors, room)
    cnt, ov, ex, ret = res
    for o in chk:
        for i, rd in enumerate(reads):
            eret, lst = o.overlaps_from_read(rd, strand=int(strands[i]), barcode=int(barcodes[i]), skip_repeats=int(skip), cap=room + 8)
            assert eret == cnt[i], (i, eret, int(cnt[i]))
            assert [tuple(x) for x in ov[i, :max(eret, 0)].tolist()] == [tuple(x) for x in lst], (i, "overlap list")
            for t in range(max(eret, 0)):
                o_in = tuple(ov[i, t].tolist())
                xret, xout = o.extend_overlap(rd if o_in[5] == 1 else G.rc(rd), factors[i], o_in)
                assert int(ret[i, t]) == xret and tuple(ex[i, t].tolist()) == tuple(xout), (i, t, o_in)
    wide = []
    for i, rd in enumerate(reads):
        g = W.groups_of(eng, i)
        if g is not None:
            wide.append(i)
            h = deciding_hits(chk[0], rd, int(strands[i]), int(barcodes[i]), skip, hit_len)
            assert g[0] == expected_groups(h, len(rd)), (i, "dependency records")
            if int(barcodes[i]) != -1:
                assert g[1] == 0 and not any(g[3]), (i, "a barcoded read's hits all count repeats = 1")
    return res, wide


def same_results(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- lists of 10 000 / 10 001 postings under skip_repeats and barcodes ---------------------------------------------------------------
def contig_barcode(i):
    """contig A (0) carries barcode 3, and so does a third of the one-k-mer contigs; the others carry 5 or none"""
    return 3 if i == 0 else -1 if i == 1 else (3, 5, -1)[i % 3]


@functools.lru_cache(maxsize=None)
def long_list_case(size):
    """test_query_edges.long_list_set(size) with contig barcodes, and two reads that begin with its P (19 bases; k-mers 0, 5 and 10 hold
    `size` postings, the k-mers between them 100):
      plain  P + a tail that meets no contig: the first pass is empty, the second meets the long lists and returns contig A
      ror    P + a tail of which one more contig X holds three k-mers on three diagonals: three hits of short lists and no run of two,
             so no overlap in either pass, but a group that switches on removeOnlyRepeats once a list holds more than 10 000 postings
             (the reference measures X's group in full: see the filler below)
    -> (set, plain, ror, index of X)"""
    es, rd = Q.long_list_set(size)
    bs = BcSet(es, contig_barcode)
    k, p = es.k, rd[:19]

    def hits_of(r):
        return bs.o.hits(r, strand=0, cap=1 << 20)

    def tail_without_hits():
        while True:
            r = p + bs.random_seq(61)
            h = hits_of(r)
            if (h[:, 3] == 1).all() and set(h[:, 2].tolist()) == {0, 5, 10}:
                return r

    plain = tail_without_hits()
    while True:
        ror = tail_without_hits()
        if not set(G.kmers(ror[19:], k)) & set(G.kmers(plain, k)):
            break
    # X: k-mers 29, 44 and 59 of `ror` at 5, 30 and 50 -- diagonals -24, -14, -9
    while True:
        x = bs.random_seq(5) + ror[29: 29 + k] + bs.random_seq(16) + ror[44: 44 + k] + bs.random_seq(11) + ror[59: 59 + k] + bs.random_seq(6)
        probe = Oracle(k)
        w = np.ones((len(x), 4), dtype=np.int32)
        probe.add_novel("x", x, 1, -1, w)
        h = probe.hits(ror, strand=0, cap=1 << 10)
        if sorted((a, b) for _, a, b, _, _ in h.tolist()) == [(5, 29), (30, 44), (50, 59)] and len(probe.hits(plain, strand=0, cap=1 << 10)) == 0:
            break
    # The statistics loop steps `i = j; ++i` (SeqSet.hpp:810 and the loop's own increment): behind a measured group it passes over the
    # first hit of the next one. Between A and X lie 3 (size - 1) groups of one hit, which vanish and reappear in turn, so with an odd
    # `size` X would be measured one hit short and removeOnlyRepeats would stay off: one more group of one hit (k-mer 35 of the tail)
    # puts X back in step.
    if size % 2 == 1:
        bs.add(ror[35: 35 + k], -1)
    ix_x = bs.add(x, -1)
    h = hits_of(ror)
    on_x = h[h[:, 0] == ix_x]
    assert len(on_x) == 3 and len(set((on_x[:, 1] - on_x[:, 2]).tolist())) == 3 and (on_x[:, 4] <= 100).all()
    assert set(hits_of(plain)[:, 2].tolist()) == {0, 5, 10}
    return bs, plain, ror, ix_x


@pytest.mark.parametrize("size", [10000, 10001])
def test_second_pass_on_the_long_lists(engines, size):
    """case 1: the first pass is empty, the plain pass that follows meets lists of `size` postings and returns contig A"""
    import trust4_amd
    bs, plain, _, _ = long_list_case(size)
    o = bs.o
    assert first_pass(o, plain, 0, -1, bs.hit_len) == []
    eret, lst = o.overlaps_from_read(plain, skip_repeats=1)
    assert eret == 1 and lst[0][0] == 0 and (o.hits(plain, strand=0, cap=1 << 20)[:, 4] > 10000).any() == (size == 10001)
    chk = bs.checkers()
    eng = engines()
    ix = bs.commit(eng)
    before = W.wide_stats(eng)[0]
    _, wide = check_query(eng, chk, ix, bs.hit_len, [plain], [0], [-1], 1)
    # (30 000 hits: with the real threshold the plain pass is the wide query's at either size, as it is for skip_repeats = 0)
    assert wide == [0] and W.wide_stats(eng)[0] - before == 1
    check_query(eng, chk, ix, bs.hit_len, [plain], [0], [-1], 0)
    # the 10 000 edge by itself: with the hit threshold out of the way the tiers answer 10 000, and only the long list sends 10 001 wide
    eng2 = engines(T4_WIDE_MIN_HITS=1 << 20)
    ix2 = bs.commit(eng2)
    _, wide = check_query(eng2, chk, ix2, bs.hit_len, [plain], [0], [-1], 1)
    assert wide == ([0] if size == 10001 else []) and W.wide_stats(eng2)[0] == len(wide)
    # t4_overlaps has no wide query: what it says of the same read is pinned by test_query_edges
    if size == 10001:
        with pytest.raises(trust4_amd.T4Error) as e:
            ix.overlaps(eng.upload([plain]), 0, 1, 64)
        assert "posting list beyond 10000" in str(e.value)


@pytest.mark.parametrize("size", [10000, 10001])
def test_remove_only_repeats_after_an_empty_first_pass(engines, size):
    """case 2: X's three hits of short lists make no overlap but switch on removeOnlyRepeats at 10 001, which removes A's group"""
    bs, _, ror, _ = long_list_case(size)
    o = bs.o
    assert first_pass(o, ror, 0, -1, bs.hit_len) == []
    for skip in (0, 1):
        eret, lst = o.overlaps_from_read(ror, skip_repeats=skip)
        assert (eret, [x[0] for x in lst]) == ((1, [0]) if size == 10000 else (0, []))
    chk = bs.checkers()
    eng = engines()
    ix = bs.commit(eng)
    for skip in (1, 0):
        res, wide = check_query(eng, chk, ix, bs.hit_len, [ror], [0], [-1], skip)
        assert wide == [0] and int(res[0][0]) == (1 if size == 10000 else 0)
    eng2 = engines(T4_WIDE_MIN_HITS=1 << 20)
    res, wide = check_query(eng2, chk, bs.commit(eng2), bs.hit_len, [ror], [0], [-1], 1)
    assert wide == ([0] if size == 10001 else [])


def test_first_pass_not_empty(engines):
    """case 3: readA and readB of test_assign_wide.heavy_set meet the long lists, but their first pass (every list of 100 or more
    postings dropped) finds their tails' contigs: the second never runs, and nothing is beyond one workgroup"""
    es, ra, rb, _ = A.heavy_set(10001)
    reads = [ra, rb, G.rc(rb)]
    for rd in reads:
        assert len(first_pass(es.o, rd, 0, -1, es.hit_len)) > 0
        assert (es.o.hits(rd, strand=0, cap=1 << 20)[:, 4] > 10000).any() and (es.o.hits(rd, strand=0, allow_total_skip=1, cap=1 << 20)[:, 4] < 100).all()
    eng = engines()
    ix = es.commit(eng)
    res, wide = check_query(eng, A.checkers(es), ix, es.hit_len, reads, [0, 0, 0], [-1, -1, -1], 1)
    assert wide == [] and W.wide_stats(eng)[0] == 0 and (res[0] > 0).all()


@pytest.mark.parametrize("size", [10000, 10001])
def test_barcoded_reads_on_a_set_not_keyed_by_barcode(engines, size):
    """case 4: the read with barcode 3 (contig A's), 5 and none, with and without skip_repeats; then AssignRead over the same batch"""
    bs, plain, _, _ = long_list_case(size)
    o = bs.o
    bcs = [3, 5, -1]
    reads = [plain] * 3
    for skip in (0, 1):
        got = [[x[0] for x in o.overlaps_from_read(plain, barcode=b, skip_repeats=skip)[1]] for b in bcs]
        assert got == [[0], [], [0]], got
    h3 = o.hits(plain, strand=0, barcode=3, cap=1 << 20)
    assert 3000 < len(h3) < len(o.hits(plain, strand=0, cap=1 << 20)) // 2 and (h3[:, 4] == 1).all()   # filtered, and every hit repeats = 1
    assert all(bs.contigs[i][3] == 3 for i in set(h3[:, 0].tolist()))
    chk = bs.checkers()
    eng = engines()
    ix = bs.commit(eng)
    for skip in (0, 1):
        res, wide = check_query(eng, chk, ix, bs.hit_len, reads, [0, 0, 0], bcs, skip)
        assert wide == [0, 1, 2] and res[0].tolist() == [1, 0, 1]
    b = eng.upload(reads, np.array(bcs, dtype=np.int32))
    ret, out = ix.assign_wide(b, strand=0)
    # (with a list of 10 001 postings the tiers of t4_assign report all three rows; with 10 000 they answer them)
    assert eng.assign_wide_stats() == ((0, 3) if size == 10001 else (3, 0))
    A.check_rows(ret, out, reads, [0, 0, 0], chk, barcodes=bcs)
    eng2 = engines(T4_ASSIGN_WIDE_ALL=1)
    ret2, out2 = bs.commit(eng2).assign_wide(eng2.upload(reads, np.array(bcs, dtype=np.int32)), strand=0)
    assert eng2.assign_wide_stats() == (0, 3) and A.same_bytes((ret, out), (ret2, out2))


# ---- route against route ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def route_case(seed=23):
    """test_assign_wide.random_case with contig barcodes from {-1, 0, 1, 2} and about 120 one-k-mer contigs: 105 of the k-mer that opens
    a 17-base window of a contig (the window and its reverse complement are reads whose first pass is one base short of
    hitLenRequired, hence empty, and whose plain pass -- which never passes over the first or the last k-mer -- finds the contig),
    the rest on k-mers of other contigs. Reads carry mixed barcodes; one is shorter than k, one holds N."""
    rnd = random.Random(seed)
    es, reads = A.random_case(seed)
    bs = BcSet(es, lambda i: (-1, 0, 1, 2)[(i * 7 + 3) % 4])
    k = bs.k
    for src in range(len(es.contigs)):
        c = es.contigs[src][1]
        st = 30
        win = c[st: st + 17]
        if len(set(G.kmers(win, k))) == 9 and all(len(bs.o.hits(km, strand=0, cap=1 << 12)) == 1 for km in G.kmers(win, k)):
            break
    for _ in range(105):
        bs.add(win[:k], rnd.choice((-1, 0, 1, 2)))
    for t in range(15):
        c = es.contigs[(src + 1 + t) % len(es.contigs)][1]
        bs.add(c[40: 40 + k], rnd.choice((-1, 0, 1, 2)))
    reads = reads + [win, G.rc(win), "ACGTAC", reads[0][:40] + "N" + reads[0][41:], ""]
    src_bc = bs.contigs[src][3]
    barcodes = [rnd.choice((-1, -1, 0, 1, 2)) for _ in reads]
    barcodes[-5], barcodes[-4] = -1, src_bc
    return bs, reads, barcodes, src


def test_route_against_route(engines):
    """case 5: one workgroup per read (real capacities: nothing here is heavy), the wide query for every read of more than 40 hits, and
    the same with partitions of 256 keys (one contig's hits must fit one) and pools that grow on demand -- byte-identical, and equal to the oracle"""
    bs, reads, barcodes, src = route_case()
    o = bs.o
    n = len(reads)
    strands = [(0, 0, 1, -1)[i % 4] for i in range(n)]
    strands[-5] = strands[-4] = 0
    for i in (n - 5, n - 4):   # the two windows: first pass empty, the plain pass finds the contig
        assert first_pass(o, reads[i], 0, barcodes[i], bs.hit_len) == []
        assert [x[0] for x in o.overlaps_from_read(reads[i], barcode=barcodes[i], skip_repeats=1)[1]] == [src]
    sizes = [len(o.hits(km, strand=1, cap=1 << 12)) for km in set(G.kmers(bs.contigs[src][1], bs.k))]
    assert max(sizes) >= 100
    assert o.overlaps_from_read(reads[-3])[0] == -1 and "N" in reads[-2] and reads[-1] == ""
    first = [len(reads[i]) >= bs.k and len(first_pass(o, reads[i], strands[i], barcodes[i], bs.hit_len)) > 0 for i in range(n)]
    assert sum(first) > n // 2
    groups = {}   # the expected dependency records of a read, by (read, skip): computed once for the routes that serve it wide

    def groups_expected(i, skip):
        if (i, skip) not in groups:
            h = o.hits(reads[i], strand=strands[i], barcode=barcodes[i], allow_total_skip=1 if (skip and first[i]) else 0, cap=1 << 22)
            groups[i, skip] = expected_groups(h, len(reads[i]))
        return groups[i, skip]
    chk = bs.checkers()
    results = {}
    for name, aids in (("real", {}), ("cap", dict(T4_AQ_CAP_LIMIT=40)), ("pools", dict(T4_AQ_CAP_LIMIT=40, T4_WIDE_PCAP=256, T4_WIDE_PARTS=8, T4_WIDE_GROUPS=64))):
        eng = engines(**aids)
        ix = bs.commit(eng)
        for skip in (0, 1):
            before = W.wide_stats(eng)
            if name == "real":
                res, wide = check_query(eng, chk, ix, bs.hit_len, reads, strands, barcodes, skip, room=96)
                assert wide == [] and W.wide_stats(eng)[0] == 0
            else:
                fac = factors_of(barcodes, skip)
                res = add_query(eng, ix, reads, strands, barcodes, skip, fac, 96)
                wide = [i for i in range(n) if W.groups_of(eng, i) is not None]
                st = W.wide_stats(eng)
                assert st[0] - before[0] == len(wide) > 0
                assert any(barcodes[i] != -1 for i in wide), "no barcoded read on the wide route"
                if skip:
                    assert n - 5 in wide and n - 4 in wide   # (second sweep: their first pass found nothing)
                for i in wide:
                    assert W.groups_of(eng, i)[0] == groups_expected(i, skip), (name, skip, i)
                if name == "pools":
                    assert st[2] > before[2] or skip   # calls repeated with larger pools (the pools have grown by the second call)
            results[name, skip] = res
            # an empty batch is answered, with nothing
            assert add_query(eng, ix, [], [], [], skip, [], 8)[0].tolist() == []
    for skip in (0, 1):
        assert same_results(results["real", skip], results["cap", skip]) and same_results(results["real", skip], results["pools", skip])


# ---- the ordered contig builder under --trimLevel 2 --------------------------------------------------------------------------------
def drive_trim2(asm, reads, names, barcodes, thresholds, update_every=150, window=0):
    """test_assembler_emu.drive with repetitiveData set and a barcode per read (main.cpp:1224-1235, 1700-1701 under --trimLevel 2)"""
    log = []
    prev_ret, n_ok = -1, 0
    for i, rd in enumerate(reads):
        if window and not (i > 0 and rd == reads[i - 1]) and not asm.window_valid():
            nxt = [j for j in range(i, len(reads)) if j == 0 or reads[j] != reads[j - 1]][:window]
            asm.prefetch([reads[j] for j in nxt], [0] * len(nxt), [barcodes[j] for j in nxt], 1)
        if i > 0 and rd == reads[i - 1]:
            ret = asm.repeat_add_read(rd) if prev_ret not in (-1, -3) else prev_ret
            log.append(("rep", ret))
        else:
            ret, strand = asm.add_read(rd, names[i], 0, barcodes[i], 1 + (i % 7), 1, thresholds[i])
            log.append(("add", ret, strand))
            if ret < 0 and i % 3 != 2:
                ret = asm.input_novel_read(names[i] if names[i] else "Novel", rd, 1 if i % 5 else -1, barcodes[i])
                log.append(("new", ret))
        prev_ret = ret
        if ret >= 0:
            n_ok += 1
            if n_ok % update_every == 0:
                asm.update_all_consensus()
    asm.update_all_consensus()
    return log


@pytest.mark.parametrize("cap_limit", [40, 0], ids=["cap40", "realcaps"])
def test_assembler_in_lock_step_with_the_reference(engines, tmp_path, monkeypatch, cap_limit):
    """case 6: AddRead / RepeatAddRead / InputNovelRead with repetitiveData and barcodes (a gene id for about 70 % of the reads), a
    window of 32 and a tier capacity of 40 hits, so that window entries with skip and with barcodes are served by the wide query:
    return codes, strands and Output equal the compiled reference's SeqSet; every served entry is queried again (T4_VERIFY_WINDOW).
    With the real capacities the tiers serve every entry: the same checks on that route."""
    import filecmp
    import zlib
    import test_assembler_emu as E
    import trust4_amd
    from t4libs import REF_FA, RefSeqSet
    if not Ref.available():
        pytest.skip("oracle/_ref/libt4ref.so not built")
    seed, k = 5, 9
    reads = E.make_reads(seed, 160, 10)
    o = Oracle(9, REF_FA, 17)
    rnd = random.Random(seed)
    names, thr, barcodes, ids = [], [], [], {}
    for rd in reads:
        _, g = o.annotate_read0(rd)
        nm = ""
        for t in range(4):
            if g[t][0] != -1:
                nm = o.name(g[t][0])[:4]
        names.append(nm)
        thr.append(rnd.choice([0.9, 0.95, 0.97]))
        key = rd.replace("N", "A")[:40]   # (a read and its copy with an N share the fake V assignment)
        barcodes.append(ids.setdefault(nm, len(ids)) if nm and zlib.crc32(key.encode()) % 10 < 8 else -1)
    share = sum(1 for b in barcodes if b != -1) / len(barcodes)
    assert 0.5 < share < 0.9 and len(set(barcodes)) >= 3, (share, set(barcodes))
    ref = RefSeqSet(k)
    log_ref = drive_trim2(ref, reads, names, barcodes, thr)
    monkeypatch.setenv("T4_VERIFY_WINDOW", "1")
    eng = engines(**({"T4_AQ_CAP_LIMIT": cap_limit} if cap_limit else {}))
    mine = trust4_amd.Assembler(eng, k)
    log_mine = drive_trim2(mine, reads, names, barcodes, thr, window=32)
    first_diff = next((i for i, (a, b) in enumerate(zip(log_ref, log_mine)) if a != b), None)
    assert first_diff is None and len(log_ref) == len(log_mine), (first_diff, log_ref[first_diff], log_mine[first_diff])
    pa, pb = str(tmp_path / "ref_raw.out"), str(tmp_path / "mine_raw.out")
    ref.output(pa)
    mine.output(pb)
    assert filecmp.cmp(pa, pb, shallow=False)
    assert sum(1 for x in log_ref if x[0] == "add" and x[1] >= 0) > len(reads) // 10
    c = mine.counters()
    assert c["window_hits"] > 0
    lc = (C.c_int64 * 28)()
    eng.check(eng.lib.t4_assembler_live_counters(mine.h, lc, 28))
    assert lc[27] > 0 or not cap_limit, "no window entry was served by the wide query"
    mine.close()


# ---- the whole program -----------------------------------------------------------------------------------------------------------------
def _trim2_program_case(tmp_path, driver, pairs, clones, seed, cap_limit):
    """test_stage1_e2e._bulk_case under --trimLevel 2 (every AddRead with repetitiveData, V gene ids as barcodes), with a small tier
    capacity and T4_VERIFY_WINDOW: outputs against the reference binary's, the log's count of wide-served window entries"""
    import filecmp
    import re
    import subprocess
    import test_stage1_e2e as S
    fa = str(tmp_path / "ref.fa")
    S._gunzip(S.REF_FA, fa)
    pre = str(tmp_path / "b")
    subprocess.run([os.path.join(S.ROOT, "tools", "t4synth"), fa, str(pairs), str(clones), str(seed), pre], check=True, stdout=subprocess.DEVNULL)
    args = ["--skipMateExtension", "--trimLevel", "2", "-f", fa, "-1", pre + "_1.fq", "-2", pre + "_2.fq"]
    ref_out, my_out = str(tmp_path / "ref"), str(tmp_path / "mine")
    subprocess.run([S.REF_BIN, "-t", "1"] + args + ["-o", ref_out], check=True, stderr=subprocess.DEVNULL)
    e = dict(os.environ)
    for a in AIDS:
        e.pop(a, None)
    e.update({"T4_VERIFY_WINDOW": "1", "T4_TIMING": "1"})
    if cap_limit:
        e["T4_AQ_CAP_LIMIT"] = str(cap_limit)
    p = subprocess.run([driver, "-t", "4"] + args + ["-o", my_out], check=True, env=e, stderr=subprocess.PIPE, text=True)
    for suffix in ("_raw.out", "_assembled_reads.fa", "_final.out"):
        assert filecmp.cmp(ref_out + suffix, my_out + suffix, shallow=False), suffix
    log = p.stderr
    m = re.search(r"wide query served (\d+) window entries", log)
    assert m and (int(m.group(1)) > 0 or not cap_limit), log[-800:]
    v = re.search(r"T4_VERIFY_WINDOW: (\d+) served window entries queried again at serve time, all equal to their cached results", log)
    assert v and int(v.group(1)) > 0, log[-800:]
    return int(m.group(1)), int(v.group(1))


def _ref_bin():
    import test_stage1_e2e as S
    return S.REF_BIN


@pytest.mark.parametrize("cap_limit", [120, 0], ids=["cap120", "realcaps"])
def test_whole_program_emulated(tmp_path, cap_limit):
    """case 7 on the emulator build: 240 pairs of 5 clones; with the real capacities too, where the single-workgroup tiers serve every
    window entry (entries with skip stand under the conservative rule on either route: T4_VERIFY_WINDOW holds them to a fresh query)"""
    import test_stage1_e2e as S
    if not os.path.exists(_ref_bin()):
        pytest.skip("oracle/_ref/trust4 not built")
    _trim2_program_case(tmp_path, S._emulated_driver(), 240, 5, 11, cap_limit)


@pytest.mark.gpu
def test_whole_program_gpu(tmp_path):
    """case 7 on the GPU: 6 000 pairs of 120 clones"""
    import test_stage1_e2e as S
    if not os.path.exists(_ref_bin()):
        pytest.skip("oracle/_ref/trust4 not shipped")
    _trim2_program_case(tmp_path, S._driver(), 6000, 120, 11, 2000)
