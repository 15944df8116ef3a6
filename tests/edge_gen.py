"""Generators of contig sets and reads that sit exactly on a capacity or threshold edge of the query kernels.

Every generator builds its contig set in an Oracle as it goes and measures the property it aims at there (hits of the read,
overlaps of GetOverlapsFromHits, postings of one list); a generator that misses its target raises. The building blocks:
  - copies of the read (forward or reverse complement, a few substitutions): about one hit per k-mer and one overlap each;
  - windows of the read just long enough to chain: one overlap each for few hits;
  - contigs of exactly one k-mer of the read: one more hit each, nothing else.
Everything is seeded; nothing is written to disk."""
import random

import numpy as np

from t4libs import Oracle

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s):
    return "".join(COMP[x] for x in reversed(s))


def kmers(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


class EdgeSet:
    """A contig set under construction, mirrored in an Oracle (which measures every target)."""

    def __init__(self, k, hit_len, seed):
        self.k, self.hit_len = k, hit_len
        self.rnd = random.Random(seed)
        self.contigs = []           # (name, seq, weights)
        self.o = Oracle(k)
        self.o.set_hit_len_required(hit_len)
        self.reads = []

    def random_seq(self, n):
        return "".join(self.rnd.choice("ACGT") for _ in range(n))

    def new_read(self, length=150):
        """a random read whose k-mers occur once among both strands of every read of this set"""
        while True:
            rd = self.random_seq(length)
            mine = kmers(rd, self.k) + kmers(rc(rd), self.k)
            if len(set(mine)) == len(mine) and not (set(mine) & self._taken()):
                self.reads.append(rd)
                return rd

    def _taken(self):
        out = set()
        for r in self.reads:
            out.update(kmers(r, self.k))
            out.update(kmers(rc(r), self.k))
        return out

    def add(self, seq):
        w = np.zeros((len(seq), 4), dtype=np.int32)
        for j, ch in enumerate(seq):
            w[j, "ACGT".index(ch)] = self.rnd.randint(1, 9)
        name = "e%d" % len(self.contigs)
        assert self.o.add_novel(name, seq, 1, -1, w) == len(self.contigs)
        self.contigs.append((name, seq, w))

    def copy_of(self, rd, subs=0, reverse=False):
        s = list(rd)
        for _ in range(subs):
            p = self.rnd.randrange(len(s))
            s[p] = self.rnd.choice([c for c in "ACGT" if c != s[p]])
        s = "".join(s)
        self.add(rc(s) if reverse else s)

    def hits(self, rd):
        return len(self.o.hits(rd, strand=0, cap=1 << 20))

    def overlaps(self, rd):
        return len(self.o.overlaps_from_hits(rd, strand=0, hit_len_required=self.hit_len, filt=1, cap=1 << 14))

    def list_size(self, kmer):
        """postings of one k-mer, measured: hits of the k-mer itself as a read (one strand; it occurs once in it)"""
        return len(self.o.hits(kmer, strand=1, cap=1 << 20))

    def pad_hits(self, rd, target):
        """one-k-mer contigs of the read's k-mers (both strands, round robin) until the read has exactly `target` hits"""
        ks = kmers(rd, self.k)
        ks = [x for pair in zip(ks, kmers(rc(rd), self.k)) for x in pair]
        at = self.rnd.randrange(len(ks))
        h = self.hits(rd)
        while h < target:
            for _ in range(target - h):
                self.add(ks[at % len(ks)])
                at += 1
            h = self.hits(rd)
        if h != target:
            raise AssertionError("hits %d, target %d" % (h, target))
        return h

    def commit(self, eng):
        ix = eng.index(self.k)
        for name, s, w in self.contigs:
            ix.add_contig(name, s, -1, w)
        ix.set_params(self.hit_len, 10, 0.9).commit()
        return ix

    def ref(self):
        """the same set in the compiled reference (callers check Ref.available())"""
        from t4libs import Ref
        r = Ref(self.k)
        for name, s, w in self.contigs:
            r.add_novel(name, s, 1, -1, w)
        r.set_hit_len_required(self.hit_len)
        return r


def reads_with_hits(es, targets, subs=2):
    """reads of exactly targets[i] hits each (both strands): copies of every read first (half of them reverse complements, a few
    substitutions), then one-k-mer contigs of a read's own k-mers, which no other read of the set holds"""
    reads = []
    for target in targets:
        rd = es.new_read()
        nk = len(rd) - es.k + 1
        for c in range(max(0, (target - 2 * nk) // nk)):
            es.copy_of(rd, subs=es.rnd.randint(0, subs), reverse=c % 2 == 1)
        reads.append(rd)
    for rd, target in zip(reads, targets):
        es.pad_hits(rd, target)
    got = [es.hits(rd) for rd in reads]
    if got != list(targets):
        raise AssertionError("hits %s, targets %s" % (got, list(targets)))
    return reads


def read_with_overlaps(es, n_ov, hits=None, win=None):
    """a read with exactly `n_ov` overlaps of GetOverlapsFromHits (windows of the read, both strands), then padded to `hits` hits"""
    rd = es.new_read()
    win = win or max(es.hit_len, 2 * es.k)
    starts = list(range(0, len(rd) - win + 1))
    es.rnd.shuffle(starts)
    i = 0
    while es.overlaps(rd) < n_ov:
        if i > 4 * n_ov:
            raise AssertionError("windows of %d bases do not reach %d overlaps" % (win, n_ov))
        for _ in range(n_ov - es.overlaps(rd)):
            st = starts[i % len(starts)]
            w = rd[st: st + win]
            es.add(rc(w) if i % 2 else w)
            i += 1
    got = es.overlaps(rd)
    if got != n_ov:
        raise AssertionError("overlaps %d, target %d" % (got, n_ov))
    if hits is not None:
        es.pad_hits(rd, hits)
        if es.overlaps(rd) != n_ov:
            raise AssertionError("padding moved the overlap count")
    return rd


class RefEdgeSet(EdgeSet):
    """A reference gene set (annotation path: no repeat-skip rule) under construction, mirrored in an Oracle. Reference records of
    identical sequence are merged on input (SeqSet::InputRefFa), so every record carries its own number of N before and after it:
    N windows hold no k-mer, so they add no hit."""

    def __init__(self, k, hit_len, seed):
        import ctypes as C
        self.k, self.hit_len = k, hit_len
        self.rnd = random.Random(seed)
        self.records = []
        self.o = Oracle(k)
        self.o.set_hit_len_required(hit_len)
        self._add = self.o.lib.t4o_add_ref_record
        self._add.restype = C.c_int
        self._add.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        self.reads = []

    def add(self, seq, gene="IGHV"):
        n = len(self.records)
        s = "N" * (n // 64) + seq + "N" * (n % 64)
        name = "%s1-%d*01" % (gene, n)
        assert self._add(self.o.h, name.encode(), s.encode()) == n
        self.records.append((name, s))

    def commit(self, eng):
        ix = eng.index(self.k)
        for name, s in self.records:
            ix.add_ref_record(name, s)
        return ix.set_params(self.hit_len, 10, 0.9).commit()

    def ref(self, tmp_path):
        from t4libs import Ref
        fa = tmp_path / "edge_ref.fa"
        fa.write_text("".join(">%s\n%s\n" % r for r in self.records))
        r = Ref(self.k, str(fa))
        r.set_hit_len_required(self.hit_len)
        return r


def ref_reads_with_hits(es, targets):
    """reads of exactly targets[i] hits on a reference set: exact copies (forward and reverse complement), then one-k-mer records"""
    reads = []
    for target in targets:
        rd = es.new_read()
        ks = kmers(rd, es.k)
        ks = [x for pair in zip(ks, kmers(rc(rd), es.k)) for x in pair]
        nk = len(ks) // 2
        for c in range(max(0, (target - 2 * nk) // nk)):
            es.add(rc(rd) if c % 2 else rd)
        for t in range(target - es.hits(rd)):
            es.add(ks[t % len(ks)])
        reads.append(rd)
    got = [es.hits(rd) for rd in reads]
    if got != list(targets):
        raise AssertionError("hits %s, targets %s" % (got, list(targets)))
    return reads
