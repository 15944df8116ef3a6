"""t4_assign_wide: SeqSet::AssignRead (SeqSet.hpp:4632-4701) without the limits of the single-workgroup tiers. Reads that t4_assign and
t4_assign_strands refuse (a posting list beyond 10 000 entries, more than 262 144 hits, more than 16 384 overlaps) are answered
through the AddRead query path and AssignRead's pick on the device (assignPickKernel); every other read gets the old entries' bytes.
Every case compares with the oracle, and with the compiled reference when it was built, as test_query_edges.check_overlap_path does:
the return value always, the whole record when the reference's return value is not -1.
  1  lists of 10 001 postings answered (strand arguments 0 / 1 / -1, through strand= and strands=); 10 000: no read on the wide route
  2  ordinary and heavy reads in one batch: ordinary rows are t4_assign's / t4_assign_strands' bytes, the split is exact
  3  every read on the wide route (T4_ASSIGN_WIDE_ALL): assign_wide == assign == oracle on a random set
  4  the pick's edges: 0 / 1 / 300 overlaps, the spanning extension first and last in the sorted order, a read shorter than k,
     an empty batch -- and the pick kernel on records made by hand (ties, the field a similarity-failed extension leaves behind)
  5  mismatch factor 2.0: barcoded reads on a set whose index is keyed by barcode
  6  contract: reference sets refused, NULL outputs, no state left behind
The CPU suite runs every case on the emulator build; `-m gpu` runs them on the GPU."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import edge_gen as G
import t4check
from t4libs import Oracle, Ref, Synth, rows_to_strs

AIDS = ("T4_AQ_CAP_LIMIT", "T4_WIDE_PCAP", "T4_WIDE_PARTS", "T4_WIDE_GROUPS", "T4_WIDE_MIN_HITS", "T4_AQ_EXTEND_DEFER", "T4_WIDE_OFF",
        "T4_AQ_FORCE_GLOBAL", "T4_STATIC_STRIDE", "T4_ASSIGN_WIDE_ALL")
NONE = (-1, -1, -1, -1, -1, 1, 0, 0, 0.0)   # the record of a read that is not assigned


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
    e.env = real_caps
    yield e
    e.close()
    os.environ.pop("T4_LIB", None)


def checkers(es):
    return [es.o] + ([es.ref()] if Ref.available() else [])


def check_rows(ret, out, reads, strands, chk, rows=None, barcodes=None):
    """rows of an assign call against every checker: the return value always, the whole record when the checker's is not -1"""
    assigned = 0
    for o in chk:
        for i in (range(len(reads)) if rows is None else rows):
            eret, eout = o.assign_read(reads[i], int(strands[i]), -1 if barcodes is None else int(barcodes[i]))
            assert int(ret[i]) == eret and (eret == -1 or tuple(out[i].tolist()) == tuple(eout)), (i, int(strands[i]), eret, eout, int(ret[i]), out[i])
            assigned += eret != -1
    return assigned


def same_bytes(a, b, rows_a=None, rows_b=None):
    """(ret, out) of two assign calls, byte for byte (-1 rows included)"""
    ra, oa = (a[0], a[1]) if rows_a is None else (a[0][rows_a], a[1][rows_a])
    rb, ob = (b[0], b[1]) if rows_b is None else (b[0][rows_b], b[1][rows_b])
    return ra.tobytes() == rb.tobytes() and oa.tobytes() == ob.tobytes()


def sub(rd, positions):
    """the read with a substitution at every one of the positions"""
    s = list(rd)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


# ---- lists beyond 10 000 postings -------------------------------------------------------------------------------------------------
ORDINARY_HITS = [300, 600, 800, 700]


@functools.lru_cache(maxsize=None)
def heavy_set(size):
    """test_query_edges.long_list_set with a second heavy read: readA = P (19 bases) + Q, readB = P + another tail. Contig A is P
    alone, contig B a copy of Q, contig C a copy of the whole of readB with two substitutions in its tail; k-mers 0, 5 and 10 of P
    (the ones the repeat-skip rule lets through when every k-mer between them has 100+ postings) hold `size` postings. Both reads
    meet the long lists; AssignRead answers C for readB and -1 for readA (B does not reach the start of the read). Four ordinary
    reads of a few hundred hits each stand beside them. -> (set, readA, readB, ordinary reads)"""
    k = 9
    es = G.EdgeSet(k, 17, 77)
    ra = es.new_read(80)
    while True:
        rb = ra[:19] + es.random_seq(61)
        mine = G.kmers(rb, k)[11:] + G.kmers(G.rc(rb), k)[:-11]
        if len(set(mine)) == len(mine) and not (set(mine) & es._taken()):
            break
    es.reads.append(rb)
    es.add(ra[:19])
    es.add(ra[19:])
    c = list(rb)
    for p in (45, 66):
        c[p] = "ACGT"[("ACGT".index(c[p]) + 1) % 4]
    es.add("".join(c))
    ordinary = G.reads_with_hits(es, ORDINARY_HITS)
    for p in range(11):
        km = ra[p: p + k]
        want = size if p in (0, 5, 10) else 100
        for _ in range(want - es.list_size(km)):
            es.add(km)
        assert es.list_size(km) == want
    for rd in (ra, rb):
        h = es.o.hits(rd, strand=1, cap=1 << 20)
        assert sorted(set(h[:, 2].tolist()) & set(range(11))) == [0, 5, 10]
    return es, ra, rb, ordinary


def on_long_lists(es, rd, strand):
    """does the read meet the long lists under this strand argument? (their hits are on the strand of readA / readB alone)"""
    return len(es.o.hits(rd, strand=strand, cap=1 << 20)) > 10000


def test_lists_of_10001_postings_are_answered(eng):
    import trust4_amd
    es, ra, rb, _ = heavy_set(10001)
    heavy = [ra, rb, G.rc(rb)]
    # the inputs are what they are meant to be: a heavy read that is assigned, one that is not, and the old entries refuse them
    assert es.o.assign_read(rb, 0, -1)[0] == 2 and es.o.assign_read(G.rc(rb), 0, -1)[0] == 2 and es.o.assign_read(ra, 0, -1)[0] == -1
    ix = es.commit(eng)
    chk = checkers(es)
    b = eng.upload(heavy)
    with pytest.raises(trust4_amd.T4Error) as e:
        ix.assign(b, 0)
    assert "posting list beyond 10000" in str(e.value)
    for strand, wide in ((0, 3), (1, 2), (-1, 1)):
        # every read that meets the long lists under this strand argument takes the wide route (the reverse complement of readB has
        # no hit at all with strand 1, readA and readB none to speak of with strand -1: the tiers answer those, with -1)
        assert sum(on_long_lists(es, rd, strand) for rd in heavy) == wide
        ret, out = ix.assign_wide(b, strand=strand)
        assert eng.assign_wide_stats() == (len(heavy) - wide, wide)
        st = [strand] * len(heavy)
        assigned = check_rows(ret, out, heavy, st, chk)
        assert assigned == len(chk) * (2 if strand == 0 else 1)   # readB on its own strand only
        assert same_bytes((ret, out), ix.assign_wide(b, strands=st))
        assert eng.assign_wide_stats() == (len(heavy) - wide, wide)
    st = [1, 1, -1]
    ret, out = ix.assign_wide(b, strands=st)
    assert eng.assign_wide_stats() == (0, 3)
    assert check_rows(ret, out, heavy, st, chk) == 2 * len(chk) and ret.tolist() == [-1, 2, 2]


def test_lists_of_10000_postings_stay_on_the_tiers(eng):
    es, ra, rb, _ = heavy_set(10000)
    ix = es.commit(eng)
    heavy = [ra, rb, G.rc(rb)]
    b = eng.upload(heavy)
    ret, out = ix.assign_wide(b, strand=0)
    assert eng.assign_wide_stats() == (len(heavy), 0)
    assert check_rows(ret, out, heavy, [0] * 3, checkers(es)) > 0
    assert same_bytes((ret, out), ix.assign(b, 0))


# ---- ordinary and heavy reads in one batch ---------------------------------------------------------------------------------------
def test_mixed_batch(eng):
    es, ra, rb, ordinary = heavy_set(10001)
    ix = es.commit(eng)
    chk = checkers(es)
    reads = [rb, ordinary[0], ordinary[1], ra, ordinary[2], ordinary[3], G.rc(rb)]
    heavy_rows, ord_rows = [0, 3, 6], [1, 2, 4, 5]
    b, b_ord = eng.upload(reads), eng.upload(ordinary)
    ret, out = ix.assign_wide(b, strand=0)
    assert eng.assign_wide_stats() == (len(ord_rows), len(heavy_rows))
    assert same_bytes((ret, out), ix.assign(b_ord, 0), rows_a=ord_rows)
    assert check_rows(ret, out, reads, [0] * len(reads), chk, rows=heavy_rows) == 2 * len(chk)
    assert check_rows(ret, out, reads, [0] * len(reads), chk, rows=ord_rows) > 0
    strands = np.array([1, 0, -1, 0, 1, -1, -1], dtype=np.int32)
    ret, out = ix.assign_wide(b, strands=strands)
    assert eng.assign_wide_stats() == (len(ord_rows), len(heavy_rows))
    assert same_bytes((ret, out), ix.assign_strands(b_ord, strands[ord_rows]), rows_a=ord_rows)
    assert check_rows(ret, out, reads, strands, chk, rows=heavy_rows) == 2 * len(chk)
    assert (ret[ord_rows] == -1).any() and (ret[ord_rows] != -1).any()   # -1 rows are among the bytes compared


# ---- route against route ----------------------------------------------------------------------------------------------------------
def random_case(seed, k=9, n_contigs=30, per_contig=7):
    """contigs cut from synthetic transcripts with random per-base weights; reads drawn from them with 0-4 substitutions and up to
    two single-base indels, half of them reverse complemented"""
    rnd = random.Random(seed)
    es = G.EdgeSet(k, 17, seed)
    for f in rows_to_strs(Synth(60, seed).next_reads(n_contigs))[:n_contigs]:
        w = np.zeros((len(f), 4), dtype=np.int32)
        for j, ch in enumerate(f):
            bi = "ACGT".index(ch)
            w[j, bi] = rnd.randint(1, 20)
            if rnd.random() < 0.1:
                w[j, (bi + 1) % 4] = rnd.randint(0, 12)
        assert es.o.add_novel("c%d" % len(es.contigs), f, 1, -1, w) == len(es.contigs)
        es.contigs.append(("c%d" % len(es.contigs), f, w))
    reads = []
    for _, c, _ in es.contigs:
        for _ in range(per_contig):
            st = rnd.randint(0, 60)
            rd = list(c[st: st + rnd.randint(60, 110)])
            for _ in range(rnd.randint(0, 4)):
                rd[rnd.randrange(len(rd))] = rnd.choice("ACGT")
            for _ in range(rnd.randint(0, 2)):
                p = rnd.randrange(5, len(rd) - 5)
                if rnd.random() < 0.5:
                    del rd[p]
                else:
                    rd.insert(p, rnd.choice("ACGT"))
            rd = "".join(rd)
            reads.append(G.rc(rd) if rnd.random() < 0.5 else rd)
    return es, reads


def extension_fell_back_before_the_hit(o, rd, hit_seq):
    """does an overlap that AssignRead extends before the one it settles on come back from ExtendOverlap as it went in (return value 0,
    `extendedOverlap = overlap`, SeqSet.hpp:1243-1246: the similarity cut)? Overlaps of more matches sort first."""
    n, ovs = o.overlaps_from_read(rd)
    ovs = [tuple(x) for x in ovs]
    hit = [x for x in ovs if x[0] == hit_seq]
    for x in ovs:
        if x[6] > max(h[6] for h in hit):
            eret, eout = o.extend_overlap(rd if x[5] == 1 else G.rc(rd), 1.0, x)
            if eret == 0 and tuple(eout) == x:
                return True
    return False


def test_every_read_on_the_wide_route(eng):
    """T4_ASSIGN_WIDE_ALL: the pick of assignPickKernel against mode 2 of the query kernel and against the oracle, about 200 reads.

    The issue asks for a read whose answer has indelCnt != 0 (a similarity-failed extension with indels before the hit). A contig
    set has none: GetOverlapsFromRead zeroes the similarity of an overlap of a contig as soon as it counts an indel
    (SeqSet.hpp:1969-2006) and then drops it at the similarity cut (2100-2108), so every overlap AssignRead sees has indelCnt 0 and
    the field it leaves behind is 0 whatever fails. What a set can hold, and this one is asserted to, is a similarity-failed
    extension before the hit; the field itself is moved by hand in test_pick_kernel_on_records_made_by_hand."""
    es, reads = random_case(5)
    es.o.set_novel_similarity(0.95)
    # two copies of one more read: X holds more matches in its overlap (three substitutions within six bases of either end) and falls
    # to the similarity cut once extended over them, Y (one substitution nine bases from either end) is the answer
    rx = es.new_read(100)
    es.add(sub(rx, (1, 3, 5, 94, 96, 98)))
    es.add(sub(rx, (8, 91)))
    reads.append(rx)
    ix = es.commit(eng)
    ix.set_params(17, 10, 0.95)
    b = eng.upload(reads)
    strands = np.array([(0, 1, -1)[i % 3] for i in range(len(reads))], dtype=np.int32)
    old = ix.assign(b, 0), ix.assign_strands(b, strands)
    eng.env.setenv("T4_ASSIGN_WIDE_ALL", "1")
    new = ix.assign_wide(b, strand=0)
    assert eng.assign_wide_stats() == (0, len(reads))
    new_st = ix.assign_wide(b, strands=strands)
    assert eng.assign_wide_stats() == (0, len(reads))
    assert same_bytes(new, old[0]) and same_bytes(new_st, old[1])
    assert check_rows(new[0], new[1], reads, [0] * len(reads), [es.o]) > len(reads) // 4
    assert check_rows(new_st[0], new_st[1], reads, strands, [es.o]) > len(reads) // 8
    assert int(new[0][-1]) == len(es.contigs) - 1 and extension_fell_back_before_the_hit(es.o, rx, int(new[0][-1]))
    assert not any(tuple(x.tolist())[7] for x in new[1])   # (see the docstring)


# ---- the pick's edges -------------------------------------------------------------------------------------------------------------
def test_pick_edges(eng):
    es = G.EdgeSet(9, 17, 41)
    # more overlaps than the workgroup has lanes, a ragged tail, no hit: 600 windows on both strands, of which GetOverlapsFromRead
    # keeps the 300 of the better strand (G.read_with_overlaps(es, 300) would leave the pick 150: fewer than its 256 lanes)
    r300 = G.read_with_overlaps(es, 600)
    r1 = es.new_read(100)
    es.copy_of(r1, reverse=True)                         # one overlap
    id1 = len(es.contigs) - 1
    r0 = es.new_read(100)                                # no overlap
    # the only spanning extension first in the sorted order: an exact copy among windows of the read
    rf = es.new_read(100)
    es.add(rf)
    idf = len(es.contigs) - 1
    for st in (0, 20, 45, 60):
        es.add(es.random_seq(25) + rf[st: st + 40] + es.random_seq(25))
    # ... and last: its overlap stops short of substitutions near both ends of the read, the others (longer windows of the read
    # between random flanks) hold more matches and do not reach the ends
    rl = es.new_read(100)
    es.add(sub(rl, (8, 91)))
    idl = len(es.contigs) - 1
    for a, z in ((0, 92), (3, 95), (6, 99)):
        es.add(es.random_seq(25) + rl[a: z] + es.random_seq(25))
    reads = [r300, r1, r0, rf, rl, "ACGTAC", ""]
    exp = [es.o.assign_read(rd, 0, -1)[0] for rd in reads]
    assert exp == [-1, id1, -1, idf, idl, -1, -1], exp
    counts = [es.o.overlaps_from_read(rd, cap=4096)[0] for rd in reads]
    assert counts[:3] == [300, 1, 0] and counts[5] == -1, counts
    for rd, idx, first in ((rf, idf, True), (rl, idl, False)):
        ovs = [tuple(x) for x in es.o.overlaps_from_read(rd)[1]]
        assert len(ovs) >= 4
        mine = [x[6] for x in ovs if x[0] == idx]
        others = [x[6] for x in ovs if x[0] != idx]
        assert len(mine) == 1 and (mine[0] > max(others) if first else mine[0] < min(others)), (first, ovs)
    ix = es.commit(eng)
    chk = checkers(es)
    b = eng.upload(reads)
    old = ix.assign(b, 0)
    eng.env.setenv("T4_ASSIGN_WIDE_ALL", "1")
    new = ix.assign_wide(b, strand=0)
    assert eng.assign_wide_stats() == (0, len(reads))
    assert same_bytes(new, old)
    assert check_rows(new[0], new[1], reads, [0] * len(reads), chk) == 3 * len(chk)
    assert [tuple(x.tolist()) for x in new[1][[0, 2, 5, 6]]] == [NONE] * 4
    ret, out = ix.assign_wide(eng.upload([]), strand=0)
    assert len(ret) == 0 and len(out) == 0 and eng.assign_wide_stats() == (0, 0)


def pick_reference(ov, ext, ret, aux, length):
    """AssignRead's loop over one read's records (SeqSet.hpp:4649-4699) as mode 2 of the query kernel restates it"""
    def key(i):
        o = ov[i]
        den = (1 << 40) if (o["similarity"] == 0 or o["matchCnt"] == 0) else int(o["seqEnd"] - o["seqStart"] + 1 + o["readEnd"] - o["readStart"] + 1)
        return (-int(o["matchCnt"]), den, -int(o["readEnd"] - o["readStart"]), int(o["seqIdx"]), int(o["strand"]), int(o["readStart"]),
                int(o["readEnd"]), int(o["seqStart"]), int(o["seqEnd"]), i)
    stale = 0
    for i in sorted(range(len(ov)), key=key):
        e = ext[i]
        if ret[i] == 1 and e["readStart"] == 0 and e["readEnd"] == length - 1:
            return int(ov[i]["seqIdx"]), (int(ov[i]["seqIdx"]), 0, length - 1, int(e["seqStart"]), int(e["seqEnd"]), int(ov[i]["strand"]), int(e["matchCnt"]),
                                          stale, float(e["matchCnt"]) / float(aux[i]))
        if aux[i] == 0:
            stale = int(ov[i]["indelCnt"])
    return -1, NONE


def test_pick_kernel_on_records_made_by_hand(eng):
    """assignPickKernel on records no contig set produces: overlaps with indels whose extension failed the similarity cut before the
    hit (the indelCnt AssignRead leaves behind), ties in every field but the pool index, a zero similarity, reads of 0 / 1 / 63 /
    64 / 65 / 256 / 257 / 1000 / 5000 records, the hit first, last, absent"""
    import trust4_amd
    rnd = np.random.RandomState(7)
    sizes = [0, 1, 1, 63, 64, 65, 256, 257, 1000, 1000, 5000, 5000, 700]
    length = 120
    ovs, exts, rets, auxs, counts, base = [], [], [], [], [], []
    for r, n in enumerate(sizes):
        ov = np.zeros(n, dtype=trust4_amd.api.OV_DTYPE)
        # few distinct values per field: many ties down to the last fields of the comparison, and whole duplicates
        ov["matchCnt"] = rnd.choice([0, 60, 60, 80, 100], size=n)
        ov["readStart"] = rnd.randint(0, 3, size=n)
        ov["readEnd"] = length - 1 - rnd.randint(0, 3, size=n)
        ov["seqStart"] = rnd.randint(0, 3, size=n)
        ov["seqEnd"] = ov["seqStart"] + length - 1 - rnd.randint(0, 3, size=n)
        ov["seqIdx"] = rnd.randint(0, 4, size=n)
        ov["strand"] = rnd.choice([-1, 1], size=n)
        ov["indelCnt"] = rnd.randint(0, 5, size=n)
        den = ov["seqEnd"] - ov["seqStart"] + 1 + ov["readEnd"] - ov["readStart"] + 1
        ov["similarity"] = np.where(rnd.rand(n) < 0.2, 0.0, ov["matchCnt"] / den)
        ext = ov.copy()
        mode = r % 3   # spanning extensions: a few anywhere / none / only among the records of fewest matches (the hit sorts last)
        spans = (rnd.rand(n) < 0.02) if mode == 0 else np.zeros(n, dtype=bool) if mode == 1 else (ov["matchCnt"] == 0) & (rnd.rand(n) < 0.3)
        if n == 1:
            spans[:] = r == 1
        ext["readStart"] = np.where(spans, 0, 1)
        ext["readEnd"] = length - 1
        ext["matchCnt"] = ov["matchCnt"] + rnd.randint(0, 9, size=n)
        ret = np.where(spans, 1, rnd.randint(0, 2, size=n)).astype(np.int32)
        aux = np.where((ret == 0) & (rnd.rand(n) < 0.5), 0, 200 + rnd.randint(0, 40, size=n)).astype(np.int32)
        counts.append(n); base.append(sum(len(x) for x in ovs))
        ovs.append(ov); exts.append(ext); rets.append(ret); auxs.append(aux)
    exp = [pick_reference(ovs[r], exts[r], rets[r], auxs[r], length) for r in range(len(sizes))]
    assert sum(1 for e in exp if e[0] != -1 and e[1][7] != 0) >= 3 and sum(1 for e in exp if e[0] == -1) >= 4
    ov, ext, ret, aux = (np.ascontiguousarray(np.concatenate(x)) for x in (ovs, exts, rets, auxs))
    counts, base = np.array(counts, dtype=np.int32), np.array(base, dtype=np.int32)
    counts[0] = -1   # (GetOverlapsFromRead's value for a read shorter than k)
    lens = np.full(len(sizes), length, dtype=np.int32)
    out_ret, out = np.zeros(len(sizes), dtype=np.int32), np.zeros(len(sizes), dtype=trust4_amd.api.OV_DTYPE)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    fn = eng.lib.t4_assign_pick
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 6
    eng.check(fn(eng.h, len(sizes), P(counts), P(base), P(lens), len(ov), P(ov), P(ext), P(ret), P(aux), P(out_ret), P(out)))
    for r, (eret, eout) in enumerate(exp):
        assert int(out_ret[r]) == eret and tuple(out[r].tolist()) == tuple(eout), (r, sizes[r], eret, eout, out[r])


# ---- mismatch factor 2.0 ----------------------------------------------------------------------------------------------------------
def test_barcoded_reads(eng):
    """a set whose index is keyed by barcode: AssignRead extends with mismatch factor 2.0 for a read that has a barcode"""
    rnd = random.Random(19)
    k = 9
    o = Oracle(k)
    o.lib.t4o_set_consider_barcode(o.h, 1)
    ix = eng.index(k, consider_barcode=True)
    contigs = []
    for i, f in enumerate(rows_to_strs(Synth(60, 19).next_reads(18))[:18]):
        w = np.zeros((len(f), 4), dtype=np.int32)
        for j, ch in enumerate(f):
            w[j, "ACGT".index(ch)] = rnd.randint(1, 20)
        assert o.add_novel("c%d" % i, f, 1, i % 3, w) == ix.add_contig("c%d" % i, f, i % 3, w)
        contigs.append((f, i % 3))
    o.set_hit_len_required(13)
    ix.set_params(13, 10, 0.9).commit()
    reads, bcs = [], []
    for f, bc in contigs:
        for _ in range(4):
            st = rnd.randint(0, 60)
            rd = list(f[st: st + rnd.randint(60, 110)])
            for p in rnd.sample(range(len(rd)), rnd.randint(0, 6)):   # up to six substitutions: some pass at factor 2.0 only
                rd[p] = rnd.choice("ACGT")
            rd = "".join(rd)
            reads.append(G.rc(rd) if rnd.random() < 0.5 else rd)
            bcs.append(bc if rnd.random() < 0.8 else (bc + 1) % 3)
    bcs = np.array(bcs, dtype=np.int32)
    b = eng.upload(reads, bcs)
    old = ix.assign(b, 0)
    eng.env.setenv("T4_ASSIGN_WIDE_ALL", "1")
    new = ix.assign_wide(b, strand=0)
    assert eng.assign_wide_stats() == (0, len(reads))
    assert same_bytes(new, old)
    assert check_rows(new[0], new[1], reads, [0] * len(reads), [o], barcodes=bcs) > len(reads) // 3
    assert (new[0] != -1).any() and (new[0] == -1).any()


# ---- contract ---------------------------------------------------------------------------------------------------------------------
def test_contract(eng):
    import trust4_amd
    rs = G.RefEdgeSet(9, 17, 3)
    rd = rs.new_read()
    rs.add(rd)
    rix = rs.commit(eng)
    with pytest.raises(trust4_amd.T4Error) as e:
        rix.assign_wide(eng.upload([rd]), strand=0)
    assert e.value.code == -4 and "contig set" in str(e.value)
    es, reads = random_case(11, n_contigs=8, per_contig=4)
    ix = es.commit(eng)
    b = eng.upload(reads)
    for aid in (None, "1"):
        if aid:
            eng.env.setenv("T4_ASSIGN_WIDE_ALL", aid)
        first = ix.assign_wide(b, strand=0)
        again = ix.assign_wide(b, strand=0)
        assert same_bytes(first, again)                      # nothing of the first call is left in the AddRead query's pools
        assert eng.assign_wide_stats() == ((0, len(reads)) if aid else (len(reads), 0))
        assert check_rows(first[0], first[1], reads, [0] * len(reads), [es.o]) > 0
        # NULL ret / out are tolerated as in t4_assign
        ret = np.zeros(len(reads), dtype=np.int32)
        eng.check(eng.lib.t4_assign_wide(ix.h, b.h, 0, None, ret.ctypes.data_as(C.c_void_p), None))
        assert ret.tobytes() == first[0].tobytes()
        out = np.zeros(len(reads), dtype=trust4_amd.api.OV_DTYPE)
        eng.check(eng.lib.t4_assign_wide(ix.h, b.h, 0, None, None, out.ctypes.data_as(C.c_void_p)))
        assert out.tobytes() == first[1].tobytes()
        eng.check(eng.lib.t4_assign_wide(ix.h, b.h, 0, None, None, None))
    # the AddRead query path still works on this ctx, and an AddRead query in flight refuses the call
    st = np.zeros(len(reads), dtype=np.int32)
    fa = np.ones(len(reads), dtype=np.float64)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    buf = np.frombuffer(("".join(reads) + "\0").encode(), dtype=np.uint8)
    V = C.c_void_p
    begin = eng.lib.t4_add_query_pool_begin2
    begin.restype, begin.argtypes = C.c_int, [V, C.c_int, V, V, V, V, C.c_int, V, V, V, V, C.c_int]
    eng.check(begin(ix.h, len(reads), buf.ctypes.data_as(V), off.ctypes.data_as(V), None, st.ctypes.data_as(V), 0, fa.ctypes.data_as(V), None, None, None, 0))
    with pytest.raises(trust4_amd.T4Error) as e:
        ix.assign_wide(b, strand=0)
    assert e.value.code == -5
    outs = [V() for _ in range(5)]
    end = eng.lib.t4_add_query_pool_end
    end.restype, end.argtypes = C.c_int, [V] + [C.POINTER(V)] * 5
    eng.check(end(eng.h, *[C.byref(x) for x in outs]))
    assert same_bytes(ix.assign_wide(b, strand=0), first)
