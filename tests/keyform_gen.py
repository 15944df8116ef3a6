"""Generators of contig sets whose hits sit on the extremes of the sort key of a hit (t4_device.h: strand | contig id | diagonal |
read offset, in 32 or in 64 bits): the last contig id, contig 0 on the minus strand, the most negative diagonal a set of its
longest contig's length can produce (a read that begins with the contig's last bases), the most positive one (a 384-base read
that ends with a contig's first bases), the last read offset.

A set is built in an Oracle as it goes; what a generator aims at (the extremes, a hit count) is measured on the ORACLE's hits,
and a generator that misses its target raises, as in edge_gen.py. Everything is seeded; nothing is written to disk."""
import random

import numpy as np

from t4libs import Oracle

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
READ_MAX = 384      # T4_MAXL
EDGE = 40           # bases a read shares with the end of a contig it overhangs
FILLER = 40         # length of a filler contig


def rc(s):
    return "".join(COMP[x] for x in reversed(s))


def kmers(s, k):
    return {s[i:i + k] for i in range(len(s) - k + 1)}


class KeySet:
    """a contig set under construction, mirrored in an Oracle; the surface test_query_edges.checkers / check_add_query expect"""

    def __init__(self, k, seed, hit_len=31):
        self.k, self.hit_len = k, hit_len
        self.rnd = random.Random(seed)
        self.np_rnd = np.random.RandomState(seed)
        self.contigs = []           # (name, seq, weights)
        self.o, self._ref = None, None

    def random_seq(self, n):
        return "".join(self.rnd.choice("ACGT") for _ in range(n))

    def weights(self, seq):
        w = np.zeros((len(seq), 4), dtype=np.int32)
        code = np.frombuffer(seq.encode(), dtype=np.uint8)
        col = np.select([code == ord(c) for c in "ACGT"], [0, 1, 2, 3], default=0)
        w[np.arange(len(seq)), col] = self.np_rnd.randint(1, 10, size=len(seq))
        return w

    def add(self, seq):
        self.contigs.append(("e%d" % len(self.contigs), seq, self.weights(seq)))
        return len(self.contigs) - 1

    def mirror(self):
        """a fresh Oracle holding the contigs as they are now (the oracle has no edit call)"""
        self.o, self._ref = Oracle(self.k), None
        for i, (name, s, w) in enumerate(self.contigs):
            assert self.o.add_novel(name, s, 1, -1, w) == i
        self.o.set_hit_len_required(self.hit_len)
        return self.o

    def commit(self, eng):
        ix = eng.index(self.k)
        for name, s, w in self.contigs:
            ix.add_contig(name, s, -1, w)
        ix.set_params(self.hit_len, 10, 0.9).commit()
        return ix

    def ref(self):
        """the same set in the compiled reference (callers check Ref.available())"""
        from t4libs import Ref
        if self._ref is None:     # built once per state of the set (mirror() forgets it)
            self._ref = Ref(self.k)
            for name, s, w in self.contigs:
                self._ref.add_novel(name, s, 1, -1, w)
            self._ref.set_hit_len_required(self.hit_len)
        return self._ref

    def hits(self, rd):
        return len(self.o.hits(rd, strand=0, cap=1 << 20))

    def max_len(self):
        return max(len(c[1]) for c in self.contigs)


def end_probes(es, seq, with_rc=True):
    """reads that put hits on the extreme diagonals of contig `seq`: copies of its far end (150 bases, and 384 when it is that
    long), a read that begins with its last EDGE bases, a 384-base read that ends with its first EDGE bases, the reverse complement
    of its first 150 bases (the same bases when it is shorter) -- and the reverse complements of all of them"""
    out = [seq[-150:]]
    if len(seq) >= READ_MAX:
        out.append(seq[-READ_MAX:])
    out.append(seq[-EDGE:] + es.random_seq(150 - EDGE))
    out.append(es.random_seq(READ_MAX - EDGE) + seq[:EDGE])
    out.append(rc(seq[:150]))
    return out + ([rc(r) for r in out] if with_rc else [])


def key_form_set(k, nseq, max_len, seed, hit_len=31):
    """`nseq` contigs, the longest of `max_len` bases: filler of FILLER random bases, and probe contigs at ids 0, 1, nseq - 2 and
    nseq - 1. Contigs 0 and nseq - 1 are of the greatest length; contig nseq - 1 ends with a 384-base read, contig 0 with a 150-base
    read and begins with the reverse complement of another; contigs 1 and nseq - 2 carry a window of the read their neighbour
    ends with. -> (set, reads); the extremes are asserted on the oracle's hits before anything is returned."""
    assert nseq >= 1 and nseq != 2 and max_len >= (READ_MAX + 150 if nseq == 1 else READ_MAX + EDGE)
    es = KeySet(k, seed, hit_len)
    r384, r150, s150 = es.random_seq(READ_MAX), es.random_seq(150), es.random_seq(150)
    last = es.random_seq(max_len - READ_MAX) + r384
    first = (rc(s150) + es.random_seq(max_len - 300) + r150) if nseq > 1 else None
    if nseq == 1:
        last = rc(s150) + last[150:]
        r150 = last[-150:]
    win150 = es.random_seq(10) + r150[30:120] + es.random_seq(10)
    win384 = es.random_seq(10) + r384[100:300] + es.random_seq(10)
    special = {nseq - 1: last}
    if nseq > 1:
        special[0] = first
    if nseq == 3:
        special[1] = win150 + win384
    elif nseq > 3:
        special[1], special[nseq - 2] = win150, win384
    for i in range(nseq):
        es.add(special.get(i) or es.random_seq(FILLER))
    assert len(es.contigs) == nseq and es.max_len() == max_len == len(es.contigs[-1][1]) == len(es.contigs[0][1])
    es.mirror()
    # the probes: both ends of the last contig (far-end copies, the two overhanging reads), the far end and the start of contig 0,
    # a chimera of two of them (last contig's far end on the plus strand, contig 0's start on the minus strand)
    begin, finish = last[-EDGE:] + es.random_seq(150 - EDGE), es.random_seq(READ_MAX - EDGE) + last[:EDGE]
    reads = [r150, r384, s150, begin, finish, r384[-100:] + s150[:100]]
    if nseq > 1:
        reads.append(first[-EDGE:] + es.random_seq(150 - EDGE))
    reads += [rc(r) for r in reads]
    assert_extremes(es, reads, nseq, max_len)
    return es, reads


def all_hits(es, reads):
    """the oracle's hits of every read: rows (idx, offset, readOffset, strand, repeats)"""
    return np.concatenate([es.o.hits(rd, strand=0, cap=1 << 16) for rd in reads])


def assert_extremes(es, reads, nseq, max_len):
    h = all_hits(es, reads)
    idx, diag, roff, strand = h[:, 0], h[:, 2] - h[:, 1], h[:, 2], h[:, 3]
    missed = []
    if not (idx == nseq - 1).any():
        missed.append("no hit on the last contig id")
    if not ((idx == 0) & (strand == -1)).any():
        missed.append("no hit on contig 0 on the minus strand")
    if not (diag <= -(max_len - EDGE)).any():
        missed.append("no hit on the diagonal -(maxSeqLen - %d)" % EDGE)
    if not (diag >= READ_MAX - EDGE - es.k).any():
        missed.append("no hit on a diagonal of %d or more" % (READ_MAX - EDGE - es.k))
    if not (roff == READ_MAX - es.k).any():
        missed.append("no hit at the last read offset")
    if not ((idx == nseq - 1) & (diag <= -(max_len - EDGE))).any() or not ((idx == nseq - 1) & (diag >= READ_MAX - EDGE - es.k)).any():
        missed.append("the last contig id does not meet both extreme diagonals")
    if nseq > 3:   # two adjacent ids answer one read, at either end of the id range
        for a, b in ((0, 1), (nseq - 2, nseq - 1)):
            if not any({a, b} <= set(es.o.hits(rd, strand=0, cap=1 << 16)[:, 0].tolist()) for rd in reads):
                missed.append("no read with hits on contigs %d and %d" % (a, b))
    if missed:
        raise AssertionError("(%d, %d) k=%d: %s" % (nseq, max_len, es.k, "; ".join(missed)))


def sorter_set(nseq, seed, k=9):
    """three 150-base reads with substituted copies in the set -- 4 097 to 8 192 hits (LDS tier 4), more than 8 192 (the
    global-scratch tier), and at most 3 072 (the AddRead query kernel's own range) -- and filler up to `nseq` contigs.
    -> (set, [read of tier 4, read of the global tier, small read], their hit counts); a read that misses its range raises"""
    es = KeySet(k, seed)
    reads = [es.random_seq(150) for _ in range(3)]
    for rd, copies in zip(reads, (50, 70, 18)):
        for c in range(copies):
            s = list(rd)
            for _ in range(es.rnd.randint(0, 2)):
                p = es.rnd.randrange(len(s))
                s[p] = es.rnd.choice([x for x in "ACGT" if x != s[p]])
            s = "".join(s)
            es.add(rc(s) if c % 2 else s)
    while len(es.contigs) < nseq:
        es.add(es.random_seq(FILLER))
    assert len(es.contigs) == nseq and es.max_len() == 150
    es.mirror()
    counts = [es.hits(rd) for rd in reads]
    if not (4097 <= counts[0] <= 8192 and counts[1] > 8192 and 2049 <= counts[2] <= 3072):
        raise AssertionError("hits %s outside (4097-8192, > 8192, 2049-3072)" % counts)
    return es, reads, counts


def grow_case(seed, k=9):
    """part 4: two random transcripts (about 900 and about 2 000 bases), a short third one, as a script of SeqSet calls:
    ("new", name, read, strand) InputNovelRead, ("add", read) AddRead, ("k", n) ChangeKmerLength, ("shallow", n)
    ReleaseShallowContigs, ("update",) UpdateAllConsensus. -> (script, (position, kind) of the end-of-contig AddReads -- kinds 0 and
    1 are exact copies of a contig's last 150 bases, forward and reverse complement --, the transcripts' lengths)"""
    rnd = random.Random(seed)
    seq = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    t1, t2, t3 = seq(930), seq(2010), seq(270)     # (150 + a multiple of the step of 60)
    script, ends = [], []

    def walk(name, t):
        script.append(("new", name, t[:150], 1))
        for st in [0] + list(range(60, len(t) - 150 + 1, 60)):      # (the seed read twice: every base of A and B is covered twice or more)
            script.append(("add", t[st:st + 150]))
        script.append(("update",))

    ts = [t1, t2]

    def end_reads(thin):
        for i in (0, 1):
            t, x = ts[i], seq(110)
            grown = t + x      # the transcript once the overhanging read has extended the contig
            tail = [t[-150:], rc(t[-150:]), t[-EDGE:] + x, grown[-150:], rc(grown[-190:-40]), rc(seq(110) + t[:EDGE])]
            for kind, rd in enumerate(tail[:thin]):
                ends.append((len(script), kind))
                script.append(("add", rd))
            if thin >= 3:
                ts[i] = grown

    walk("A", t1)
    walk("B", t2)
    script.append(("new", "C", t3[:150], 1))
    script.append(("add", t3[100:250]))     # the delta of this round holds contig C alone
    end_reads(6)
    script.append(("update",))
    script.append(("k", 11))
    script.append(("add", t3[:60]))         # C: bases 60 to 99 stay covered once between stretches covered twice -- the one shallow contig
    end_reads(4)
    script.append(("shallow", 2))
    shallow_at = len(script)
    end_reads(3)
    # after ReleaseShallowContigs the reference's index still names the released contig: no later read may touch it
    taken = kmers(t3, 11) | kmers(rc(t3), 11)
    for step in script[shallow_at:]:
        if step[0] == "add" and kmers(step[1], 11) & taken:
            raise AssertionError("a read after ReleaseShallowContigs shares a k-mer with the released contig")
    return script, ends, (len(t1), len(t2), len(t3))


def cell_case(seed):
    """part 5: one script of SeqSet calls per cell (barcode). Cell 0: a short contig first, then a contig that grows from 450 to 750
    bases and is then met at its far end; cell 1 stays small; cell 2 holds 512 contigs of 40 bases and, last, one of 7 681, met at
    both ends. In cells 0 and 2 the longest contig is not the first one. -> {barcode: script}, (position, kind) of cell 0's and of
    cell 2's end-of-contig AddReads (kinds 0 and 1: exact copies of the contig's last 150 bases)"""
    rnd = random.Random(seed)
    seq = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))

    def tail(t):
        x = seq(110)
        grown = t + x
        return [t[-150:], rc(t[-150:]), t[-EDGE:] + x, grown[-150:], rc(seq(110) + t[:EDGE])]

    t0, u, long_ = seq(750), seq(300), seq(7681)
    c0 = [("new", "S", seq(100), 1), ("new", "A", t0[:150], 1)] + [("add", t0[st:st + 150]) for st in range(60, 601, 60)]
    ends0 = [(len(c0) + i, i) for i in range(5)]
    c0 += [("add", rd) for rd in tail(t0)]
    c1 = [("new", "B", u[:150], 1), ("add", u[60:210]), ("add", u[100:250]), ("add", rc(u[-150:])), ("add", u[30:180])]
    c2 = [("new", "F", seq(FILLER), 1) for _ in range(512)] + [("new", "L", long_, 1)]
    ends2 = [(len(c2) + i, i) for i in range(5)]
    c2 += [("add", rd) for rd in tail(long_)]
    return {0: c0, 1: c1, 2: c2}, {0: ends0, 2: ends2}
