"""Cases that sit on the edges of the k-mer counter (t4_kmer_count_*: kmerAddKernel, kmerSetKernel, kmerRehashKernel, kmerExportKernel,
kmerMergeKernel, kmerStatsKernel in csrc/t4_kernels.h), a restatement of its table hash, and the predicates that prove an edge is
really hit. Pure Python, seeded, nothing is written to disk.

Statistics (`stats_cases(k)`): reads are built as head + tail. A head is added to the counter at least twice, so its k-mers have a
count above 1; a tail is never added (k <= 2: heads over A/T, tails over C/G, so that no tail or junction k-mer is ever a counted
one). The last k-mer with a count above 1 is then the head's last, and the quality scan of GetCountStatsAndTrim (KmerCount.hpp:
177-288) reaches down to position len(head) and no further. `py_stats` restates that function on a dict of counts; the generator
asserts on it that every case lands where it was aimed, and the tests compare it with the C oracle too.

Table (`wrap_codes`, `distinct_codes`, `kc_mix`, `home`): codes chosen by their home slot in a table of 1 024 slots."""
import functools
import math
import random
import struct

MAXL = 384                      # T4_MAXL
SLOTS0 = 1024                   # the smallest table: t4_kmer_count_create with max_kmers <= 512 starts at its ceiling of 1 024 slots
MAX_BARCODE = (1 << 22) - 2     # T4_KMER_COUNT_MAX_BARCODE
BARCODE_SHIFT = 42
M64 = (1 << 64) - 1
KS = (1, 2, 20, 21, 31)
EQ_TAILS = (10, 20, 50, 100, 200, 380)   # len - j at which badCnt == 0.1 * (len - j) can hold exactly
CEIL_TAILS = (7, 15, 33, 101, 255)       # ... and where it cannot: ceil(0.1 * (len - j)) bad bytes meet the rule, one fewer do not
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


# ---- codes and the table hash -------------------------------------------------------------------------------------------------
def kc_mix(z):
    """kcMix of t4_kernels.h: the 64-bit mixer whose low bits are a key's home slot"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def home(key, slots=SLOTS0):
    return kc_mix(key) & (slots - 1)


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def code(s):
    """KmerCode of a k-mer without N: two bits a base, the first base in the highest bits"""
    v = 0
    for c in s:
        v = v << 2 | "ACGT".index(c)
    return v


def canon(s):
    return min(code(s), code(rc(s)))


def spell(c, k):
    return "".join("ACGT"[c >> 2 * (k - 1 - i) & 3] for i in range(k))


def valid_kmers(read, k):
    """canonical codes of the read's windows without N, in read order"""
    return [canon(read[p:p + k]) for p in range(len(read) - k + 1) if "N" not in read[p:p + k]]


def barcode_key(c, barcode):
    """the key of k-mer code c in a per-barcode counter (kmerAddKernel: `salt`)"""
    return c | (barcode + 1) << BARCODE_SHIFT


def count_reads(reads, k, barcodes=None):
    """the table a counter holds after add() of the reads: {key: count}"""
    t = {}
    for i, r in enumerate(reads):
        for c in valid_kmers(r, k):
            key = c if barcodes is None else barcode_key(c, barcodes[i])
            t[key] = t.get(key, 0) + 1
    return t


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


# ---- GetCountStatsAndTrim restated ---------------------------------------------------------------------------------------------
def py_stats(k, table, read, qual):
    """-> dict: mn, md, avg (as float32), new_len as t4_kmer_count_stats gives them, and how they came about: n (valid k-mers), kk
    (entries the median is taken over), i (one past the last count above 1), lo (the lowest position the quality scan reaches),
    trim (trimStart), evals [(j, len - j, badCnt, rule met)] for every bad byte the scan met, in scan order"""
    L = len(read)
    if L < k:
        return dict(mn=-1, md=-1, avg=-1.0, new_len=L, n=0, kk=-1, i=0, lo=L, trim=-1, evals=[])
    v = [c if c > 0 else 1 for c in (table.get(c, 0) for c in valid_kmers(read, k))]
    n = len(v)
    if n == 0:
        return dict(mn=-L, md=-L, avg=float(-L), new_len=0 if qual is not None else L, n=0, kk=-1, i=0, lo=L, trim=-1, evals=[])
    kk, trim, i, evals, new_len, nul = n, -1, 0, [], L, set()
    if qual is not None:
        i = n
        while i > 0 and v[i - 1] <= 1:
            i -= 1
        bad = 0
        for j in range(L - 1, i + k - 2, -1):
            if ord(qual[j]) - 32 <= 15:
                bad += 1
                hit = bad >= 0.1 * (L - j)
                evals.append((j, L - j, bad, hit))
                if hit:
                    trim = j
        if trim > 0:
            kk, new_len = trim - k + 1, trim
            nul.add(trim)
        if 0 < trim < k:
            kk, new_len = 0, 0
            nul.add(0)
    buf = v + [0] * (L + 1 - n)
    if kk > 0:
        buf[:kk] = sorted(buf[:kk])
    mn, md = buf[0], buf[kk // 2 if kk > 0 else 0]
    avg = f32(sum(v) / kk) if kk else math.inf
    for p, ch in enumerate(read):
        if ch == "N" and p not in nul:
            mn = 0 if mn >= 0 else mn - 1
    return dict(mn=mn, md=md, avg=avg, new_len=new_len, n=n, kk=kk, i=i, lo=i + k - 1 if qual is not None else L, trim=trim, evals=evals)


# ---- statistics cases ---------------------------------------------------------------------------------------------------------
def quals(L, bad_at, bad="/", good="0"):
    """L quality bytes: `bad` at the positions bad_at, `good` elsewhere; a string of several bytes is used in turn"""
    return "".join(bad[p % len(bad)] if p in bad_at else good[p % len(good)] for p in range(L))


class _Builder:
    def __init__(self, k):
        self.k, self.rnd = k, random.Random(7000 + k)
        self.ha, self.ta = ("AT", "CG") if k <= 2 else ("ACGT", "ACGT")
        self.adds, self.cases = [], []

    def head(self, h, times=2):
        s = "".join(self.rnd.choice(self.ha) for _ in range(h))
        self.adds += [s] * times
        return s

    def tail(self, t):
        return "".join(self.rnd.choice(self.ta) for _ in range(t))

    def case(self, tag, read, qual=None, **expect):
        assert qual is None or len(qual) == len(read)
        self.cases.append(dict(tag=tag, read=read, qual=qual, expect=expect))


def _build(k):
    b = _Builder(k)
    hk = max(k, 4)   # a head of this many bases: the scan stops at position hk, which is above 0
    b.adds.append("N" * MAXL)   # counts nothing; the compiled reference sizes its buffers by the longest read it was given (SetBuffer)
    # lengths: the 64-lane stride of the position loops and T4_MAXL; without qualities, all good, and a tail cut at the head's end
    for L in (k - 1, k, k + 1, k + 63, k + 64, k + 65, MAXL - 1, MAXL):
        h = L if L <= k else max(k, L // 2)
        read = b.head(h, times=2 + L % 3) + b.tail(L - h)
        m = L - h
        b.case(("len", L), read)
        b.case(("len", L, "good"), read, quals(L, ()))
        b.case(("len", L, "cut"), read, quals(L, range(h, h + math.ceil(0.1 * m))), trim=h if m and L >= k else -1)
    # the 10 % rule: len - j = m scanned bytes, a block of bad bytes that begins at j = the head's end
    for m in EQ_TAILS + CEIL_TAILS:
        h = hk
        if h + m > MAXL:
            continue   # (j >= k - 1 and len <= 384: a tail of 380 is in reach for k <= 5 only)
        nb = math.ceil(0.1 * m)
        for bad, good in (("/", "0"), ("!", "~")) + ((("/!", "0~I"),) if m == 20 else ()):
            read = b.head(h) + b.tail(m)
            b.case(("rule", m, "meets", bad), read, quals(h + m, range(h, h + nb), bad, good), trim=h)
            b.case(("rule", m, "misses", bad), read, quals(h + m, range(h, h + nb - 1), bad, good), trim=-1)
    # meets the rule, fails it further left, meets it again still further left: the lowest j wins
    L = hk + 60
    b.case(("rule", "meets-fails-meets"), b.head(hk) + b.tail(60), quals(L, [L - 5, L - 30, L - 38, L - 39, L - 40]), trim=L - 40)
    # where the trim lands: a read of uncounted k-mers (i = 0), everything from t on is bad
    for t in (k + 1, k, k - 1):
        for bad, good in (("/", "0"), ("!", "~")):
            L = k + 12
            b.case(("lands", t - k, bad), b.tail(L), quals(L, range(t, L), bad, good), trim=t)
    if k > 2:   # the same with every k-mer counted exactly once (a count of 1 is not above 1)
        once = b.tail(k + 12)
        b.adds.append(once)
        b.case(("lands", 0, "once"), once, quals(k + 12, range(k, k + 12)), trim=k)
    # the protected region: the scan stops at the head's end
    h = k + 5
    for m in (10, 11):
        read = b.head(h) + b.tail(m)
        b.case(("protected", m, "below"), read, quals(h + m, range(0, h)), trim=-1)
        b.case(("protected", m, "at"), read, quals(h + m, [h]), trim=h if m <= 10 else -1)
    b.case(("protected", 5, "just below"), b.head(h) + b.tail(5), quals(h + 5, [h - 1]), trim=-1)
    # median: kk odd and even, all counts equal, one k-mer, two counts split in half, and over what a trim leaves
    for h in (k + 6, k + 7, k):
        b.case(("median", "equal", h - k + 1), b.head(h, times=3))
        b.case(("median", "equal", h - k + 1, "q"), b.head(h, times=3), quals(h, ()))
    read = b.head(k + 4) + b.tail(5)
    b.case(("median", "halves"), read)
    b.case(("median", "halves", "q"), read, quals(k + 9, ()))
    L = k + 12
    b.case(("median", "after trim"), b.head(k + 4) + b.tail(8), quals(L, range(L - 6, L)), trim=L - 6)
    L = k + 40   # eight N kill more k-mers than the trim takes away: kk > n, entries never written count as 0
    read = b.tail(L)
    b.case(("median", "kk>n"), read[:3] + "N" * 8 + read[11:], quals(L, range(L - 5, L)), trim=L - 5)
    # ... and so many more that the zeros reach the middle: 16 counts, 36 entries, the median is one of the 20 never written
    b.case(("median", "kk>2n"), "N" * 25 + b.tail(L - 25), quals(L, range(L - 5, L)), trim=L - 5)
    # N rule
    read = b.head(2 * k + 10)
    one, several = read[:k + 5] + "N" + read[k + 6:], "N" + read[1:k + 5] + "N" + read[k + 6:-1] + "N"
    for tag, r in (("one", one), ("several", several)):
        b.case(("N", tag), r)
        b.case(("N", tag, "q"), r, quals(len(r), ()))
    L, t = k + 20, k + 8
    read = b.tail(L)
    b.case(("N", "at trimStart"), read[:t] + "N" + read[t + 1:], quals(L, range(t, L)), trim=t)
    b.case(("N", "after trimStart"), read[:t + 1] + "N" + read[t + 2:], quals(L, range(t, L)), trim=t)
    L = 2 * k + 5
    b.case(("N", "first, emptied"), "N" + b.tail(L - 1), quals(L, range(k - 1, L)), trim=k - 1)
    L = min(3 * k + 2, MAXL)
    read = "".join("N" if p % k == k - 1 else c for p, c in enumerate(b.tail(L)))
    b.case(("N", "every k-mer"), read)
    b.case(("N", "every k-mer", "q"), read, quals(L, ()))
    table = count_reads(b.adds, k)
    for c in b.cases:
        c["model"] = m = py_stats(k, table, c["read"], c["qual"])
        if "trim" in c["expect"]:
            assert m["trim"] == c["expect"]["trim"], (k, c["tag"], m["trim"], c["expect"])
    return tuple(b.adds), tuple(b.cases), table


@functools.lru_cache(maxsize=None)
def stats_cases(k):
    """-> (reads to add, cases, the table they make); a case: dict(tag, read, qual or None, expect, model = py_stats of it)"""
    return _build(k)


# ---- predicates on a case's model ---------------------------------------------------------------------------------------------
def trims_at(case, t):
    return case["qual"] is not None and case["model"]["trim"] == t and t > 0


def emptied(case):
    m = case["model"]
    return case["qual"] is not None and m["kk"] == 0 and m["new_len"] == 0 and m["n"] > 0


def byte_scanned(case, byte):
    """the quality byte lies where the scan looks at it"""
    q, m = case["qual"], case["model"]
    return q is not None and m["n"] > 0 and chr(byte) in q[m["lo"]:]


def rule_at_equality(case, m):
    """the bad bytes among the last m are exactly 0.1 * m, the lowest of them at len - m, where the scan ends and the read is cut"""
    mo = case["model"]
    return any(j == mo["lo"] == mo["trim"] and d == m and hit and bad * 10 == m and bad == 0.1 * d for j, d, bad, hit in mo["evals"])


def rule_one_below_equality(case, m):
    """exactly m bytes are scanned, 0.1 * m - 1 of them are bad, and nothing is cut"""
    q, mo = case["qual"], case["model"]
    return (q is not None and mo["n"] > 0 and len(q) - mo["lo"] == m and m % 10 == 0 and mo["trim"] == -1
            and sum(ord(x) <= 47 for x in q[mo["lo"]:]) == m // 10 - 1)


def rule_meets_fails_meets(case):
    hits = [hit for _, _, _, hit in case["model"]["evals"]]
    s = "".join("T" if h else "F" for h in hits)
    return "TF" in s and s.rfind("T") > s.find("TF") + 1 and case["model"]["trim"] == case["model"]["evals"][-1][0]


def reference_may_differ(read, qual, read_after):
    """The compiled reference sorts stale entries of its reused buffer for a read that has an N, got qualities, and was trimmed
    (test_kmer_count_emu.test_oracle_kmer_count_vs_reference); read_after: what the ORACLE left of the read"""
    return "N" in read and qual is not None and read_after != read


# ---- table cases ----------------------------------------------------------------------------------------------------------------
def distinct_codes(n, seed, k=21, exclude=(), accept=lambda c: True, canonical=True):
    """n distinct codes: canonical k-mer codes, or (canonical=False) codes of k-mers that are NOT canonical, as a -c file may hold"""
    rnd, out, seen = random.Random(seed), [], set(exclude)
    while len(out) < n:
        s = "".join(rnd.choice("ACGT") for _ in range(k))
        c = canon(s) if canonical else max(code(s), code(rc(s)))
        if c in seen or not accept(c) or (not canonical and c == canon(s)):
            continue
        seen.add(c)
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def wrap_codes():
    """-> (last, first, absent): 48 codes whose home is one of the last 8 of 1 024 slots (40 canonical 21-mers, 8 that are not), 12
    canonical 21-mers whose home is slot 0..7, and canonical 21-mers not among them whose home is slot 1020, 0, 3 and 30 -- inside the
    chain that the first two groups make, whatever the order of insertion: it covers slots 1016 + 8 .. at least 1016 + 59"""
    last = distinct_codes(40, 1, accept=lambda c: home(c) >= SLOTS0 - 8) + distinct_codes(8, 2, accept=lambda c: home(c) >= SLOTS0 - 8, canonical=False)
    first = distinct_codes(12, 3, accept=lambda c: home(c) < 8)
    absent = [distinct_codes(1, 4 + h, exclude=last + first, accept=lambda c: home(c) == h)[0] for h in (1020, 0, 3, 30)]
    return tuple(last), tuple(first), tuple(absent)


def top_bit_kmer(k, seed):
    """a k-mer whose canonical code has its highest bit (2k - 1) set: it begins with G and ends with C, and so does its reverse"""
    rnd = random.Random(seed)
    s = "G" + "".join(rnd.choice("ACGT") for _ in range(k - 2)) + "C"
    assert canon(s) >> (2 * k - 1) == 1
    return s


def short_read_batch(n=10000, seed=11, k=21):
    """n reads of 21..30 bases cut from a few templates (counts above 1), every 97th shorter than k -> (reads, indices of the short)"""
    rnd = random.Random(seed)
    tpl = ["".join(rnd.choice("ACGT") for _ in range(60)) for _ in range(200)]
    reads, short = [], []
    for i in range(n):
        t = tpl[rnd.randrange(len(tpl))]
        L = rnd.randint(k, 30)
        if i % 97 == 5:
            L = rnd.choice((0, 1, k - 1))
            short.append(i)
        p = rnd.randrange(0, 60 - L + 1)
        r = t[p:p + L]
        if L >= k and rnd.random() < 0.05:
            q = rnd.randrange(L)
            r = r[:q] + "N" + r[q + 1:]
        reads.append(r)
    return reads, short
