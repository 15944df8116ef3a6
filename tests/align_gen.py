"""Generators of alignment problems that sit on the band, length and tie-break edges of the gap-DP formulations, and of overlaps
with crafted overhangs for ExtendOverlap. Everything is seeded; nothing is written to disk.

Gap DP (t4_gap_dp): `dp_cases(kind)` returns (targets, patterns, tags): a grid of (lent, lenp) pairs crossed with content families
in which alignment paths of equal score are the rule (homopolymers, tandem repeats with an indel of any length at the first base,
the last base or the middle, leading and trailing gaps), equal-length pairs around the two ungapped early returns, N, and for the
posWeight aligner columns with zero sum, with two bases that pass IsBaseEqual, with none, and counts up to 10^6.
`expected_status` is the engine's contract for the status word, a function of the lengths alone.

ExtendOverlap (t4_extend): `ExtendSet` holds a few contigs (random, tandem repeat, one with zero-sum and ambiguous columns) in an
Oracle, and `extend_cases` cuts reads from them and hands back overlaps whose anchor leaves overhangs of a chosen size and content."""
import random

import numpy as np

from t4libs import Oracle

MAXGAP = 320          # T4_MAXGAP: longest side of one gap DP
DIR_BYTES = 49152     # T4_DIR_BYTES: traceback bytes of one scratch-row alignment
BAND_FWD, BAND_WAVE, BAND_OCT = 32, 64, 16   # T4_DPW, one wavefront, one 16-lane DPP row

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s):
    return "".join(COMP[x] for x in reversed(s))


def band(lent, lenp):
    return 11 + abs(lent - lenp)


def expected_status(kind, impl, lent, lenp):
    """The status word t4_gap_dp promises (include/trust4_hip.h), from the lengths alone.
    Every formulation answers an empty side (and 1 x 1, and equal lengths, whose band is 11 columns) before it looks at its band.
    The pattern is staged in LDS by the kernel, so a pattern beyond 320 bases is refused by every formulation first."""
    assert kind in (0, 1) and impl in (0, 1, 2, 3, 4)
    W = band(lent, lenp)
    if impl == 3:      # eight per wavefront: both sides are checked before anything else
        if lent > MAXGAP or lenp > MAXGAP:
            return 2
        if lent == 0 or lenp == 0:
            return 0
        return 2 if W > BAND_OCT else 0
    if impl == 2:      # one per wavefront
        if lenp > MAXGAP:
            return 2
        if lent == 0 or lenp == 0:
            return 0
        return 2 if (W > BAND_WAVE or lent > MAXGAP) else 0
    if lenp > MAXGAP:
        return 1
    if lent == 0 or lenp == 0:
        return 0
    if lent > MAXGAP:
        return 1
    if impl == 0 and W <= BAND_FWD:     # forward counts in LDS; wider bands fall back to the scratch rows
        return 0
    return 1 if (lenp + 1) * min(W, lent) > DIR_BYTES else 0


# ---- lengths ------------------------------------------------------------------------------------------------------------------
def length_grid():
    """(lent, lenp) pairs, both signs of lent - lenp"""
    g = [(a, b) for a in range(4) for b in range(4)]
    for d in (4, 5, 6, 7, 20, 21, 22, 23, 52, 53, 54, 55):     # bands of 15..18, 31..34, 63..66 columns
        for short in (12, 150 - d // 2, MAXGAP - d):             # short (band wider than the target: DW = lent), middle, long
            g += [(short + d, short), (short, short + d)]
    for a, b in ((319, 319), (320, 320), (321, 321), (320, 321), (321, 320), (319, 320), (320, 315), (315, 320), (321, 316), (316, 321),
                 (321, 0), (0, 321), (321, 1), (1, 321), (320, 0), (0, 320), (320, 1), (1, 320), (321, 300), (300, 321), (330, 330), (400, 100), (100, 400)):
        g.append((a, b))
    # both sides of (lenp + 1) * min(W, lent) = 49 152 with both sides inside 320
    g += [(153, 320), (154, 320), (160, 320), (177, 320), (178, 320), (153, 319), (154, 319), (154, 318), (155, 318), (320, 160), (320, 165)]
    # band wider than the target
    g += [(2, 9), (3, 30), (5, 40), (8, 70), (9, 2), (30, 3), (10, 64), (10, 63), (11, 75)]
    return g


def quirk_grid():
    """kind 0: lent > 4 * (lenp + 1), the border quirk of the traceback's row 0; lenp <= 12 keeps the band inside 64 columns"""
    return [(9, 1), (10, 1), (20, 1), (54, 1), (13, 2), (14, 2), (40, 2), (17, 3), (30, 3), (25, 5), (26, 5), (40, 5), (58, 5), (37, 8),
            (53, 12), (54, 12), (60, 12), (65, 12), (66, 12), (8, 1), (12, 2), (24, 5), (52, 12)]


# ---- content ------------------------------------------------------------------------------------------------------------------
FAMILIES = ("random", "homopolymer", "tandem2", "tandem3", "tandem5", "two_letter")
WHERE = ("first", "last", "middle", "scattered")


def base_sequence(rnd, n, family):
    if family == "random":
        return [rnd.choice("ACGT") for _ in range(n)]
    if family == "homopolymer":
        return [rnd.choice("ACGT")] * n
    if family == "two_letter":
        return [rnd.choice("AC") for _ in range(n)]
    u = int(family[6:])
    while True:
        unit = [rnd.choice("ACGT") for _ in range(u)]
        if len(set(unit)) > 1:
            break
    ph = rnd.randrange(u)
    return [unit[(i + ph) % u] for i in range(n)]


def make_pair(rnd, lent, lenp, family, where, subs=0, n_rate=0.0):
    """target and pattern of exactly (lent, lenp) bases: the longer one is a `family` sequence, the shorter one is it without
    |lent - lenp| bases -- one block at its first base, its last base or its middle, or single bases scattered over it"""
    big, small = max(lent, lenp), min(lent, lenp)
    s = base_sequence(rnd, big, family)
    d = big - small
    if where == "first":
        x = s[d:]
    elif where == "last":
        x = s[:small]
    elif where == "middle":
        at = (big - d) // 2
        x = s[:at] + s[at + d:]
    else:
        drop = set(rnd.sample(range(big), d))
        x = [c for i, c in enumerate(s) if i not in drop]
    t, p = (s, x) if lent >= lenp else (x, s)
    t, p = list(t), list(p)
    for _ in range(subs):
        if p:
            q = rnd.randrange(len(p))
            p[q] = rnd.choice([c for c in "ACGT" if c != p[q]])
    if n_rate:
        t = ["N" if rnd.random() < n_rate else c for c in t]
        p = ["N" if rnd.random() < n_rate else c for c in p]
    assert len(t) == lent and len(p) == lenp
    return "".join(t), "".join(p)


COLUMN_STYLES = ("plain", "mixed", "big")


def weights_of(rnd, t, style):
    """_posWeight columns of a target whose consensus is t (N: a column without counts).
    mixed: zero-sum columns (IsBaseEqual is true for every base), columns where two bases pass sum < 3 * count, columns where
    none does; big: counts up to 10^6."""
    w = np.zeros((len(t), 4), dtype=np.int32)
    for i, c in enumerate(t):
        if c == "N":
            continue
        b = "ACGT".index(c)
        if style == "plain":
            w[i, b] = rnd.randint(1, 30)
        elif style == "big":
            w[i, b] = rnd.choice([1, 999999, 1000000, 333334])
            if rnd.random() < 0.3:
                w[i, (b + 1) % 4] = rnd.choice([1, 499999, 500000, 1000000])    # 2 * other < count decides
        else:
            m = rnd.random()
            if m < 0.55:
                w[i, b] = rnd.randint(1, 30)
            elif m < 0.65:
                pass                                            # zero sum
            elif m < 0.8:
                w[i, b] = 4
                w[i, (b + 1 + rnd.randrange(3)) % 4] = 4        # two bases pass: 8 < 12
            elif m < 0.9:
                w[i] = (1, 1, 1, 1)                             # none passes: 4 < 3 is false
                w[i, b] = rnd.choice([1, 2])                    # (2: 5 < 6, this base passes alone)
            else:
                w[i, b] = 2
                w[i, (b + 1) % 4] = 1                           # 3 < 6 passes, 3 < 3 does not
    return w


def equal_length_pairs(rnd, kind):
    """equal lengths around the ungapped early returns: 3 / 4 / 5 substitutions (affine shortcut: mm <= 3), 2 / 3 mismatching
    columns (posWeight: score >= 2 * len - 8, i.e. mm <= 2), first / last / random placement, up to 320 bases"""
    out = []
    for L in (2, 3, 5, 12, 40, 150, 319, 320):
        for mm in ((2, 3, 4) if kind == 1 else (3, 4, 5)):
            if mm > L:
                continue
            for family in ("random", "two_letter", "tandem2", "tandem3"):
                for place in ("first", "last", "random", "spread"):
                    s = base_sequence(rnd, L, family)
                    if place == "first":
                        pos = list(range(mm))
                    elif place == "last":
                        pos = list(range(L - mm, L))
                    elif place == "random":
                        pos = rnd.sample(range(L), mm)
                    else:
                        pos = [(i * L) // mm for i in range(mm)]
                    p = list(s)
                    for q in pos:
                        p[q] = rnd.choice([c for c in "ACGT" if c != s[q]])
                    out.append(("".join(s), "".join(p), "equal/%d/%d/%s/%s" % (L, mm, family, place)))
    return out


def dp_cases(kind, seed=1, thin=1):
    """-> (targets, patterns, tags); kind 1 targets are [lent, 4] int32 arrays. thin > 1 keeps, of the cases with a side beyond
    70 bases, every thin-th (the emulator's share; every length pair keeps at least one case)"""
    rnd = random.Random(seed * 2 + kind)
    raw = []
    for lent, lenp in length_grid() + (quirk_grid() if kind == 0 else []):
        for fi, family in enumerate(FAMILIES):
            for wi, where in enumerate(WHERE):
                if lent == lenp and wi > 0 and max(lent, lenp) > 3:
                    continue
                subs = (fi + wi) % 3
                n_rate = 0.04 if (fi + 2 * wi) % 5 == 0 else 0.0
                t, p = make_pair(rnd, lent, lenp, family, where, subs, n_rate)
                raw.append((t, p, "grid/%d/%d/%s/%s" % (lent, lenp, family, where)))
    # tandem repeats: an indel of one unit and of a non-multiple of the unit, at the first base, the last base and the middle
    for u in (2, 3, 5):
        for d in (u, u + 1, 2 * u, 2 * u - 1, 1):
            for L in (16, 31, 90):
                for where in WHERE[:3]:
                    for lent, lenp in ((L, L - d), (L - d, L)):
                        t, p = make_pair(rnd, lent, lenp, "tandem%d" % u, where)
                        raw.append((t, p, "tandem/%d/%d/%d/%s" % (u, lent, lenp, where)))
    raw += equal_length_pairs(rnd, kind)
    # a repeat against itself out of phase (equal and nearly equal lengths): a gap at either end, and cells where the insertion and
    # the deletion tie with different counts behind them
    for family in ("tandem2", "tandem3", "tandem5", "two_letter"):
        for L in (8, 20, 61, 150, 320):
            for shift in (1, 2, 3, 4):
                for extra in (0, 1, -2):
                    for subs in (0, 2):
                        s = base_sequence(rnd, L + shift + 2, family)
                        t, p = s[:L], s[shift: shift + L + extra]
                        for _ in range(subs):
                            q = rnd.randrange(len(p))
                            p[q] = rnd.choice([c for c in "ACGT" if c != p[q]])
                        raw.append(("".join(t), "".join(p), "phase/%s/%d/%d/%d/%d" % (family, L, shift, extra, subs)))
    # related random sequences, as the suite had them
    for it in range(150):
        lt = rnd.randint(0, 60)
        t = [rnd.choice("ACGT") for _ in range(lt)]
        p = list(t)
        for _ in range(rnd.randint(0, 6)):
            c = rnd.random()
            if p and c < 0.35:
                del p[rnd.randrange(len(p))]
            elif c < 0.7:
                p.insert(rnd.randint(0, len(p)), rnd.choice("ACGT"))
            elif p:
                p[rnd.randrange(len(p))] = rnd.choice("ACGTN")
        raw.append(("".join(t), "".join(p), "related/%d" % it))
    T, P, tags = [], [], []
    seen_long = {}
    for i, (t, p, tag) in enumerate(raw):
        if thin > 1 and max(len(t), len(p)) > 70:
            key = (len(t), len(p))
            seen_long[key] = seen_long.get(key, 0) + 1
            if seen_long[key] > 1 and i % thin:
                continue
        if kind == 1:
            t = weights_of(rnd, t, COLUMN_STYLES[i % 3])
        T.append(t)
        P.append(p)
        tags.append(tag)
    return T, P, tags


# ---- ExtendOverlap --------------------------------------------------------------------------------------------------------------
def base_equal(w, c):
    """AlignAlgo::IsBaseEqual"""
    s = int(w.sum())
    return s == 0 or c == "N" or s < 3 * int(w["ACGT".index(c)])


class ExtendSet:
    """Contigs with their posWeight columns, mirrored in an Oracle: 0 and 1 random, 2 a tandem repeat of period 3 with a random
    stretch in its middle (the k-mers a read needs to be a read of it), 3 random with zero-sum and ambiguous columns."""

    def __init__(self, k=9, seed=5, length=900):
        self.k = k
        self.rnd = rnd = random.Random(seed)
        self.o = Oracle(k)
        self.o.set_hit_len_required(31)
        self.contigs = []
        for i in range(4):
            if i == 2:
                s = base_sequence(rnd, length, "tandem3")
                s[400:440] = [rnd.choice("ACGT") for _ in range(40)]
            else:
                s = [rnd.choice("ACGT") for _ in range(length)]
            s = "".join(s)
            w = weights_of(rnd, s, "mixed" if i == 3 else "plain")
            assert self.o.add_novel("x%d" % i, s, 1, -1, w) == i
            self.contigs.append(("x%d" % i, s, w))

    def commit(self, eng):
        ix = eng.index(self.k)
        for name, s, w in self.contigs:
            ix.add_contig(name, s, -1, w)
        return ix.set_params(31, 10, 0.9).commit()

    def ref(self):
        from t4libs import Ref
        r = Ref(self.k)
        for name, s, w in self.contigs:
            r.add_novel(name, s, 1, -1, w)
        r.set_hit_len_required(31)
        return r


SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 169, 170, 171, 255, 256)
READ_MAX = 384


def size_class(n):
    return "0" if n == 0 else "1-2" if n <= 2 else "3-64" if n <= 64 else "65-128" if n <= 128 else "129-170" if n <= 170 else "171-256" if n <= 256 else "257+"


def mismatch_plans():
    """name -> function(size) -> scan steps (1 = the base next to the anchor) that mismatch, or None when the size does not fit"""
    plans = {}
    for m in range(5):
        plans["first%d" % m] = lambda size, m=m: list(range(1, m + 1)) if size >= m else None
        plans["far%d" % m] = lambda size, m=m: list(range(size - m + 1, size + 1)) if size >= m else None
        plans["spread%d" % m] = lambda size, m=m: sorted({1 + (i * (size - 1)) // max(m - 1, 1) for i in range(m)}) if size >= 2 * m and m else None
    # the good-prefix rule's tie: of the first n steps exactly n / 4 mismatch (share 3/4: not "more than"), one fewer, one more; the
    # n-th step itself matches; every step beyond n mismatches, so that n is the last candidate
    for n in (4, 8, 64, 128):
        for delta, nm in ((0, "tie"), (-1, "above"), (1, "below")):
            for early in (True, False):
                def plan(size, n=n, delta=delta, early=early):
                    if size < n:
                        return None
                    q = n // 4 + delta
                    inside = list(range(1, q + 1)) if early else list(range(n - q, n))
                    return inside + list(range(n + 1, size + 1))
                plans["share%d%s%s" % (n, nm, "early" if early else "late")] = plan
    return plans


def extend_cases(es, seed=9, thin=1):
    """-> list of dicts: read (as uploaded), ov (the overlap as t4_extend takes it), aligned (the read on the overlap's strand),
    sizes (left, right overhang), planted (what was placed on each side)"""
    rnd = random.Random(seed)
    plans = mismatch_plans()
    cases = []

    def craft(ci, left, right, anchor, lplan, rplan, strand, low_match, edit=None, n_in_read=0, cut=None):
        """a read over contig ci: `left` + anchor + `right` bases; cut = ("contig_start" | "contig_end" | "read", extra): the
        overhang is cut short by the contig's end (the read goes on beyond it) or the read's (the contig goes on: always)"""
        name, cs, w = es.contigs[ci]
        extraL = extraR = 0
        if cut == "contig_start":
            a, extraL = 0, rnd.randint(1, 20)                # the read has extraL bases before the contig's first base
        elif cut == "contig_end":
            a, extraR = len(cs) - (left + anchor + right), rnd.randint(1, 20)
        else:
            a = rnd.randint(30, len(cs) - (left + anchor + right) - 30)
        if ci == 2:    # the anchor over the random stretch, or deep inside the repeat
            a = min(max(400 - left + rnd.randint(0, 8), 0), len(cs) - (left + anchor + right)) if cut is None else a
        body = list(cs[a: a + left + anchor + right])
        for side, size, plan in ((0, left, lplan), (1, right, rplan)):
            steps = plans[plan](size) if plan else []
            if steps is None:
                return
            for st in steps:
                pos = left - st if side == 0 else left + anchor + st - 1
                wcol = w[a + pos]
                bad = [c for c in "ACGT" if not base_equal(wcol, c)]
                if not bad:
                    return          # a column every base matches: the plan cannot be placed here
                body[pos] = rnd.choice(bad)
        if edit:
            side, kind_, frac = edit
            size = left if side == 0 else right
            if size < 12:
                return
            pos = int(size * frac)
            pos = (left - 1 - pos) if side == 0 else (left + anchor + pos)
            if kind_ == "del":     # the read lacks a contig base; its overhang is refilled from the contig beyond it
                if side == 0:
                    if a == 0:
                        return
                    body = [cs[a - 1]] + body[:pos] + body[pos + 1:]
                else:
                    if a + len(body) >= len(cs):
                        return
                    body = body[:pos] + body[pos + 1:] + [cs[a + len(body)]]
            else:                  # the read has a base the contig lacks
                ins = rnd.choice("ACGT")
                body = (body[1:pos + 1] + [ins] + body[pos + 1:]) if side == 0 else (body[:pos] + [ins] + body[pos:-1])
        for _ in range(n_in_read):
            side = rnd.randrange(2)
            size = left if side == 0 else right
            if size:
                body[(rnd.randrange(size)) if side == 0 else (left + anchor + rnd.randrange(size))] = "N"
        junkL = [rnd.choice("ACGT") for _ in range(extraL)]
        junkR = [rnd.choice("ACGT") for _ in range(extraR)]
        aligned = "".join(junkL + body + junkR)
        if len(aligned) > READ_MAX:
            return
        rs, re_ = extraL + left, extraL + left + anchor - 1
        ss, se = a + left, a + left + anchor - 1
        match = 2 * anchor
        if low_match:
            match = max(2, (match * 3) // 5)
        ov = (ci, rs, re_, ss, se, strand, match, 0, match / (2.0 * anchor))
        cases.append({"read": aligned if strand == 1 else rc(aligned), "aligned": aligned, "ov": ov, "sizes": (left, right),
                      "planted": (lplan, rplan, edit, n_in_read, cut)})

    biggest = READ_MAX - 1
    one_sided = list(SIZES) + [biggest]
    it = 0
    # sizes x (left only, right only, both) x 0..4 mismatches
    for size in one_sided:
        for sides in ("L", "R", "LR"):
            for pl in ("first0", "first2", "first3", "far3", "spread2", "spread3", "spread4", "far4", "first1"):
                it += 1
                if thin > 1 and size > 70 and it % thin:
                    continue
                other = rnd.choice([0, 1, 2, 20, 63, 64, 65]) if sides == "LR" else 0
                if size + other + 1 > READ_MAX:
                    other = 0
                left, right = (size, other) if sides != "R" else (other, size)
                if sides == "LR" and it % 2:
                    left, right = right, left
                anchor = min(rnd.choice([1, 9, 31, 60]), READ_MAX - left - right)
                lp = pl if left == size else rnd.choice(["first0", "spread3"])
                rp = pl if right == size else rnd.choice(["first0", "spread3"])
                craft(it % 2, left, right, anchor, lp, rp, 1 if it % 3 else -1, it % 4 == 0)
    # both sides long: four sides of up to 170 bases fit the deferred kernel's direction buffer together, longer ones do not
    for left, right in ((170, 170), (171, 171), (169, 171), (129, 254), (255, 128), (128, 128), (64, 65), (191, 192)):
        for pl in ("spread3", "spread4", "first0"):
            it += 1
            craft(it % 2, left, right, 1, pl, "spread3", 1 if it % 2 else -1, False)
    # the 3/4 rule
    for name in plans:
        if not name.startswith("share"):
            continue
        n = int("".join(ch for ch in name[5:8] if ch.isdigit()))
        for size in (n, n + 1, n + 40):
            for side in (0, 1):
                for low in (False, True):
                    it += 1
                    if thin > 1 and size > 70 and it % thin:
                        continue
                    left, right = (size, 0) if side == 0 else (0, size)
                    craft(it % 2, left, right, 31, name if side == 0 else None, name if side == 1 else None, 1 if it % 3 else -1, low)
    # an insertion or a deletion inside the overhang, in random sequence (contigs 0, 1), inside a tandem repeat (2), with ambiguous columns (3)
    for ci in (0, 1, 2, 3):
        for size in (12, 40, 64, 65, 128, 170, 171, 256, 300):
            for side in (0, 1):
                for kind_ in ("del", "ins"):
                    for frac in (0.1, 0.5, 0.9):
                        it += 1
                        if thin > 1 and size > 70 and it % thin:
                            continue
                        left, right = (size, 20) if side == 0 else (20, size)
                        craft(ci, left, right, 31, "first0", "first0", 1 if it % 2 else -1, it % 5 == 0, edit=(side, kind_, frac))
    # N in the read's overhang; zero-sum and ambiguous columns in the contig's (contig 3)
    for ci in (0, 3, 2):
        for size in (2, 30, 64, 65, 129, 200):
            for pl in ("first0", "first3", "spread3", "spread4", "share8tieearly", "share64tielate"):
                it += 1
                if thin > 1 and size > 70 and it % thin:
                    continue
                craft(ci, size, size // 2, 31, pl, pl if plans[pl](size // 2) is not None else "first0", 1 if it % 2 else -1, it % 3 == 0, n_in_read=it % 4)
    # cut short by the contig's end
    for cut in ("contig_start", "contig_end"):
        for size in (0, 1, 2, 63, 64, 65, 170, 171, 256):
            for pl in ("first0", "spread3", "far4"):
                it += 1
                if thin > 1 and size > 70 and it % thin:
                    continue
                left, right = (size, 40) if cut == "contig_start" else (40, size)
                craft(it % 2, left, right, 31, pl if left == size else "first0", pl if right == size else "first0", 1 if it % 2 else -1, False, cut=cut)
    return cases


def sliding_anchor_overlaps(es, ci, n, seed):
    """one 384-base read of contig ci with substitutions every few bases near both ends and a deletion, and n overlaps whose anchors
    slide over its clean middle: every overlap has two long overhangs that need the DP -> (read, list of overlaps)"""
    rnd = random.Random(seed)
    name, cs, w = es.contigs[ci]
    a = 100
    body = list(cs[a: a + READ_MAX + 1])
    for pos in list(range(3, 120, 13)) + list(range(270, 380, 11)):
        body[pos] = rnd.choice([c for c in "ACGT" if c != body[pos]])
    del body[250]             # from here on the read is one base ahead of the contig
    read = "".join(body)
    ovs = []
    for i in range(n):
        rs = 125 + (i % 100)
        re_ = rs + 9 + (i // 100) * 3
        ovs.append((ci, rs, re_, a + rs, a + re_, 1, 2 * (re_ - rs + 1), 0, 1.0))
    return read, ovs
