"""FASTQ text on the device (csrc/t4_text.h: line table, record validation, packing, low-complexity rule, candidate combine) against a
Python restatement of the split, of the packing -- bit for bit what t4_reads_upload_flags(T4_READS_KMERS_ONLY) makes from the same
strings, compared through t4_batch_read -- and of isLowComplexity (FastqExtractor.cpp:105-127). On the emulator build of the same
kernel source, and with -m gpu on the product library."""
import os
import random

import numpy as np
import pytest

import t4check
from t4libs import REF_FA, Oracle, RefMain
from test_stage0_e2e import stage0_input

T4_ERR_ARG = -1
MAXL = 384


@pytest.fixture(scope="module", params=[True, pytest.param(False, marks=pytest.mark.gpu)], ids=["emu", "gpu"])
def eng(request):
    if request.param:
        os.environ["T4_LIB"] = t4check.build_emulator_lib()
    else:
        os.environ.pop("T4_LIB", None)
    import trust4_amd
    e = trust4_amd.Engine(0)
    e.emulated = request.param
    e.tile = e.lib.t4_text_tile_bytes()
    yield e
    e.close()
    os.environ.pop("T4_LIB", None)


@pytest.fixture(scope="module")
def tx(eng):
    t = eng.text(1 << 16)
    yield t
    t.close()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def py_line_table(data, final):
    starts = [0] + [i + 1 for i, b in enumerate(data) if b == 10]
    if final and data and data[-1] != 10:
        starts.append(len(data) + 1)
    return starts


def py_low(s):
    n = len(s)
    cnt = [s.count(x) for x in "ACGTN"]
    if any(c >= n // 2 for c in cnt[:4]) or cnt[4] >= n // 10:
        return 1
    return 1 if sum(1 for c in cnt[:4] if c <= 2) >= 2 else 0


def py_scan(data, final):
    """-> (info as t4_text_scan gives it, [(start, id line, seq, qual)] of the whole records)"""
    st = py_line_table(data, final)
    lines = [data[st[j]:st[j + 1] - 1] for j in range(len(st) - 1)]
    nrec = len(lines) // 4
    status, bad, longest, recs = 0, -1, 0, []
    for r in range(nrec):
        a, s, p, q = lines[4 * r:4 * r + 4]
        recs.append((st[4 * r], a, s, q))
        ok = lambda x: all(33 <= b <= 126 for b in x)
        if a[:1] != b"@": rs = 1
        elif p[:1] != b"+": rs = 2
        elif len(q) != len(s): rs = 3
        elif s[:1] in (b"@", b">", b"+"): rs = 4
        elif not ok(s) or not ok(q) or b"\r" in a + p: rs = 5
        elif len(s) > MAXL: rs = 6
        elif not all(65 <= b <= 90 for b in s): rs = 7
        else: rs = 0
        if rs and not status:
            status, bad = rs, r
        if not rs:
            longest = max(longest, len(s))
    if final and len(lines) % 4 and not status:
        status, bad = 8, nrec
    return (nrec, min(st[4 * nrec], len(data)) if nrec else 0, status, bad, longest), recs


def py_pack(seqs):
    longest = max([len(s) for s in seqs] + [0])
    wpk, wnm = max(1, (longest + 15) // 16), max(1, (longest + 31) // 32)
    pk, nm = np.zeros((len(seqs), wpk), np.uint32), np.zeros((len(seqs), wnm), np.uint32)
    for i, s in enumerate(seqs):
        for j, ch in enumerate(s):
            v = "ACGT".find(ch)
            if ch == "N":
                nm[i, j >> 5] |= np.uint32(1 << (j & 31)); v = 0
            elif v < 0:
                v = 3
            pk[i, j >> 4] |= np.uint32(v << ((j & 15) * 2))
    return pk, nm, np.array([len(s) for s in seqs], np.int32), longest


def fastq(seqs, ids=None, quals=None, plus=None):
    out = []
    for i, s in enumerate(seqs):
        out.append("@%s\n%s\n%s\n%s\n" % (ids[i] if ids else "r%d" % i, s, plus[i] if plus else "+", quals[i] if quals else "F" * len(s)))
    return "".join(out).encode()


def check_piece(eng, tx, data, final=True, want_status=0):
    """scan `data`, compare the line table, the scan's info and the records with the restatement -> the piece's sequences"""
    info = tx.scan(data, final)
    want, recs = py_scan(data, final)
    assert tx.lines().tolist() == py_line_table(data, final)
    assert info[:4] == want[:4] and info[2] == want_status
    start, low = tx.records()
    assert start.tolist() == [r[0] for r in recs] + [want[1]]
    if info[2]:
        with pytest.raises(Exception) as e:
            tx.batch()
        assert e.value.code == T4_ERR_ARG and b"status" in eng.lib.t4_last_error(eng.h)
        return None
    assert info[4] == want[4]
    seqs = [r[2].decode() for r in recs]
    assert low.tolist() == [py_low(s) for s in seqs]
    for first, n in ((0, len(seqs)), (1, len(seqs) - 2)):   # the whole piece; a part of it (rows sized by its own longest read)
        if n < 0 or (first and n == 0):
            continue
        part = seqs[first:first + n]
        b, u = tx.batch(first, n), eng.upload(part, flags=1)
        try:
            got, host, mine = b.read(), u.read(), py_pack(part)
            for k in range(3):
                assert got[k].shape == mine[k].shape and (got[k] == mine[k]).all() and (host[k] == mine[k]).all(), (first, n, k)
            assert got[4] == mine[3] == host[4]
            assert got[3].tolist() == [py_low(s) for s in part] and not host[3].any()
        finally:
            b.close(); u.close()
    return seqs


def rand_seq(rnd, n, alphabet="ACGT"):
    return "".join(rnd.choice(alphabet) for _ in range(n))


# ---- word edges --------------------------------------------------------------------------------------------------------------------
def test_word_edges(eng, tx):
    rnd = random.Random(1)
    seqs = [rand_seq(rnd, n) for n in (0, 1, 15, 16, 17, 31, 32, 33, 383, 384)]
    for n in (33, 40, 384):
        s = list(rand_seq(rnd, n))
        for p in (0, 15, 16, 31, 32, n - 1):
            s[p] = "N"
        seqs.append("".join(s))
    seqs.append("ACGTRYKMSWBDHVACGTNACGTUX" * 3)   # IUPAC and other letters: coded as T
    assert check_piece(eng, tx, fastq(seqs)) == seqs
    short = [rand_seq(rnd, n) for n in (16, 3, 0, 16)]   # longest read 16: one pk word, one nm word per row
    check_piece(eng, tx, fastq(short))
    b = tx.batch()
    assert b.read()[0].shape == (4, 1) and b.read()[1].shape == (4, 1)
    b.close()


# ---- the classic traps -------------------------------------------------------------------------------------------------------------
def test_classic_traps(eng, tx):
    rnd = random.Random(2)
    seqs = [rand_seq(rnd, 40) for _ in range(5)]
    ids = ["a b", "c\td e", "plain", "x/1", "@@"]
    quals = ["@" + "F" * 39, "+" + "F" * 39, "F" * 40, "+@" * 20, "@" * 40]
    plus = ["+", "+c\td e", "+plain", "+", "+"]
    data = fastq(seqs, ids, quals, plus)
    assert check_piece(eng, tx, data) == seqs
    whole = (tx.scan(data), tx.records()[0].tolist(), tx.records()[1].tolist())
    cut = (tx.scan(data[:-1]), tx.records()[0].tolist(), tx.records()[1].tolist())   # the same without the last '\n'
    assert check_piece(eng, tx, data[:-1]) == seqs
    assert whole[0][0] == cut[0][0] and whole[0][2:] == cut[0][2:] and whole[0][1] == cut[0][1] + 1
    assert whole[1][:-1] == cut[1][:-1] and whole[2] == cut[2]


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
def test_pieces_cut_at_every_byte(eng, tx):
    rnd = random.Random(3)
    seqs = [rand_seq(rnd, n) for n in (20, 7, 33)]
    data = fastq(seqs, ids=["one", "two 2", "three"])
    whole = [r[1:] for r in py_scan(data, True)[1]]
    for cut in range(len(data) + 1):
        i1 = tx.scan(data[:cut], final=False)
        w1, r1 = py_scan(data[:cut], False)
        assert i1 == w1 and i1[2] == 0, cut
        s1 = tx.records()[0].tolist()
        rest = data[i1[1]:cut] + data[cut:]   # carry + rest
        i2 = tx.scan(rest, final=True)
        w2, r2 = py_scan(rest, True)
        assert i2 == w2 and i2[2] == 0, cut
        assert s1 == [r[0] for r in r1] + [w1[1]] and tx.records()[0].tolist() == [r[0] for r in r2] + [w2[1]]
        assert [r[1:] for r in r1] + [r[1:] for r in r2] == whole, cut
    assert tx.scan(b"@id with no newline ACGT", final=False)[:3] == (0, 0, 0)
    for final in (False, True):
        assert tx.scan(b"", final) == (0, 0, 0, -1, 0) and tx.lines().tolist() == [0]
        b = tx.batch()
        assert b.n == 0
        b.close()


# ---- tiles -------------------------------------------------------------------------------------------------------------------------
def test_line_table_across_tiles(eng, tx):
    rnd = random.Random(4)
    tile = eng.tile
    seqs, size = [], 0
    while size < 3 * tile + 200:
        seqs.append(rand_seq(rnd, rnd.choice((0, 1, 30, 75, 100, 150)), "ACGTN"))
        size += 2 * len(seqs[-1]) + 12
    for grow in range(34):   # every newline walks across the tile edges and the 16-byte load edges
        data = fastq(seqs, ids=["i" * (1 + grow)] + ["r%d" % i for i in range(1, len(seqs))])
        assert tx.scan(data)[2] == 0
        assert tx.lines().tolist() == py_line_table(data, True), grow
    check_piece(eng, tx, data)
    long_id = fastq(seqs[:3], ids=["L" * (tile + 37), "m", "n" * 50])   # a line longer than a tile
    check_piece(eng, tx, long_id)
    two = fastq(seqs)[:2 * tile - 1] + b"\n"   # exactly two tiles, a newline in the last byte
    assert len(two) == 2 * tile
    tx.scan(two, final=False)
    assert tx.lines().tolist() == py_line_table(two, False)
    tx.scan(two[:-1] + b"A", final=True)   # ... and a last line that ends with the tile
    assert tx.lines().tolist() == py_line_table(two[:-1] + b"A", True)


# ---- status ------------------------------------------------------------------------------------------------------------------------
GOOD = "@g\nACGTACGTAC\n+\nFFFFFFFFFF\n"
STATUS_CASES = [
    ("fasta", 1, ">g\nACGT\n>h\nACGT\n"), ("no_plus", 2, "@g\nACGT\nFFFF\n@h\n"), ("wrapped", 2, "@g\nACGT\nACGT\n+\nFFFF\nFFFF\n@h\nAC\n"),
    ("qual_short", 3, "@g\nACGT\n+\nFFF\n"), ("seq_at", 4, "@g\n@CGT\n+\nFFFF\n"), ("seq_gt", 4, "@g\n>CGT\n+\nFFFF\n"), ("seq_plus", 4, "@g\n+CGT\n+\nFFFF\n"),
    ("crlf", 5, "@g\r\nACGT\r\n+\r\nFFFF\r\n"), ("cr_in_id", 5, "@g\rx\nACGT\n+\nFFFF\n"), ("space_in_seq", 5, "@g\nAC T\n+\nFFFF\n"),
    ("high_qual", 5, "@g\nACGT\n+\nFF\x7fF\n"), ("long", 6, "@g\n%s\n+\n%s\n" % ("ACGT" * 96 + "A", "F" * 385)), ("lowercase", 7, "@g\nACgT\n+\nFFFF\n"),
    ("digit", 7, "@g\nAC1T\n+\nFFFF\n"), ("left_over_1", 8, "\n"), ("left_over_3", 8, "@g\nACGT\n+\n"),
]


@pytest.mark.parametrize("name,status,bad", STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_status(eng, tx, name, status, bad):
    for lead in (0, 3):   # the bad record first; behind three good ones
        data = (GOOD * lead + bad).encode()
        check_piece(eng, tx, data, want_status=status)
        assert tx.scan(data)[3] == lead
    if status != 8:
        other = STATUS_CASES[(STATUS_CASES.index((name, status, bad)) + 3) % 14][2]   # two bad records: the lower number is reported
        info = tx.scan((GOOD + bad + GOOD * 8 + other).encode())
        assert info[2:4] == (status, 1) and info == py_scan((GOOD + bad + GOOD * 8 + other).encode(), True)[0]


# ---- low complexity ----------------------------------------------------------------------------------------------------------------
def low_cases():
    out = []
    for n in (40, 41):   # cnt == n / 2 and one below, even and odd n
        for c in (n // 2, n // 2 - 1):
            rest = n - c
            out.append("A" * c + ("CGT" * n)[:rest])
            out.append(("CGA" * n)[:rest] + "T" * c)
    for n in (40, 49, 50):   # N count at n / 10 and one below
        for c in (n // 10, n // 10 - 1):
            out.append("N" * c + ("ACGT" * n)[:n - c])
    for k in (2, 3):   # two letters with at most 2 -- at 2 and at 3
        out.append("A" * k + "C" * k + "GT" * 10)
        out.append("GT" * 10 + "A" * 2 + "C" * k)
    out += ["", "A", "ACGT", "ACGTACGTACGT", "R" * 30, "ACGTRY" * 8, "ACGGTCATTGCAGGATCCGTTAACGGCTAAGTCCGATTGC", "N" * 5 + "ACGTTGCA" * 6]
    return out


def test_low_complexity(eng, tx):
    seqs = low_cases()
    assert check_piece(eng, tx, fastq(seqs)) == seqs
    low = tx.records()[1].tolist()
    assert 0 in low and 1 in low
    if RefMain.available():
        rm = RefMain()
        assert low == [1 if rm.is_low_complexity(s) else 0 for s in seqs]


# ---- candidate test ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def candidate_case(eng):
    pairs = stage0_input(11, 40, 80)
    pairs += [(pairs[0][0], "A" * 150), ("", "ACGT")]
    for a, b in list(pairs):   # a pair whose read passes and whose mate is a low-complexity homopolymer
        if not py_low(a):
            pairs.append((a, "T" * 120))
            break
    o = Oracle(9, REF_FA, 27)
    hit = lambda s: 0 if py_low(s) else int(o.has_hit_in_set(s, 0) != 0)
    return pairs, [hit(a) for a, _ in pairs], [hit(b) for _, b in pairs]


def test_candidate_test(eng, candidate_case):
    pairs, h1, h2 = candidate_case
    ref = eng.index(9).set_params(27, 10, 0.9).load_ref_fasta(REF_FA).commit()
    t1, t2 = eng.text(1 << 16), eng.text(1 << 16)
    made = [ref, t1, t2]
    try:
        r1, r2 = [a for a, _ in pairs], [b for _, b in pairs]
        assert t1.scan(fastq(r1))[2] == 0 and t2.scan(fastq(r2))[2] == 0
        b1, b2 = t1.batch(), t2.batch()
        u1, u2 = eng.upload(r1, flags=1), eng.upload(r2, flags=1)
        made += [b1, b2, u1, u2]
        # the same decision from t4_has_hit on host-filtered batches
        f1, f2 = [s for s in r1 if not py_low(s)], [s for s in r2 if not py_low(s)]
        g1, g2 = eng.upload(f1, flags=1), eng.upload(f2, flags=1)
        made += [g1, g2]
        hh1, hh2 = iter(ref.has_hit(g1).tolist()), iter(ref.has_hit(g2).tolist())
        k1 = [0 if py_low(s) else int(next(hh1) != 0) for s in r1]
        k2 = [0 if py_low(s) else int(next(hh2) != 0) for s in r2]
        assert k1 == h1 and k2 == h2
        want = [a | b for a, b in zip(h1, h2)]
        assert 20 < sum(want) < len(want) - 20 and sum(h1) < sum(want)
        assert ref.candidate_test(b1, b2).tolist() == want
        assert ref.candidate_test(b1).tolist() == h1 and ref.candidate_test(b2).tolist() == h2   # single-end form
        # batches of t4_reads_upload_flags carry no low-complexity bytes: every read counts as not low
        n1 = [int(o != 0) for o in ref.has_hit(u1).tolist()]
        n2 = [int(o != 0) for o in ref.has_hit(u2).tolist()]
        assert ref.candidate_test(u1, u2).tolist() == [a | b for a, b in zip(n1, n2)]
        assert ref.candidate_test(b1, u2).tolist() == [a | b for a, b in zip(h1, n2)]
        assert b1.read()[2].tolist() == [len(s) for s in r1]   # the batch's lengths are as they were
        made.append(t2.batch(0, 3))
        with pytest.raises(Exception) as e:
            ref.candidate_test(b1, made[-1])
        assert e.value.code == T4_ERR_ARG
    finally:
        for o in reversed(made):
            o.close()
