"""The pairs of a scanned piece after ProcessRead as a device batch with qualities (csrc/t4_text.h textPairRowsKernel /
textPairScanKernel / textPairPackKernel, t4_text_pairs_batch), the count statistics on the qualities such a batch carries
(t4_kmer_count_stats_resident) and a counter that grows beyond its max_kmers (t4_kmer_count_reserve). Expected rows are built in
Python from Text.process_pairs by the rule of the stage-1 driver's loop -- pairs in input order; read 1 if flag 1, once more if
flag 4, read 2 (letters other than ACGT as N) if flag 2 -- and uploaded (T4_READS_KMERS_ONLY): the new batch must hold the same
words, bit for bit. On the emulator build of the same kernel source, and with -m gpu on the product library."""
import random

import numpy as np
import pytest

from t4libs import KmerCountChecker
from test_engine_emu import pair_cases
from test_fastq_text import eng, fastq, py_low  # noqa: F401 (the fixture)
from test_kmer_count_emu import same
from test_text_pairs import edge_pairs, rc, scan_pair

T4_ERR_ARG, T4_ERR_UNSUPPORTED = -1, -4
KMERS_ONLY = 1
N_CASES = 400
EDGE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 383, 384)   # the word edges of pk (16 bases a word) and nm (32)


@pytest.fixture(scope="module")
def pieces(eng):  # noqa: F811
    a, b = eng.text(1 << 18), eng.text(1 << 18)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def cases():
    """pair_cases(5, N_CASES): all four kinds, dropped reads among them; made once, shared, never changed"""
    return tuple(tuple(x) for x in pair_cases(5, N_CASES))


def expected_rows(res, R2, Q2):
    """what the driver's loop appends for the pairs (res: Text.process_pairs of them) -> (reads, their qualities, whether a read 1
    among them holds a letter other than A, C, G, T, N)"""
    rows, quals, other = [], [], 0
    for i, r in enumerate(res):
        if r is None:
            continue
        _, rd, ql, fl = r
        if fl & 1:
            rows.append(rd); quals.append(ql.decode("latin-1"))
            other |= 1 if set(rd) - set("ACGTN") else 0
            if fl & 4:
                rows.append(rd); quals.append(ql.decode("latin-1"))
        if fl & 2:
            rows.append("".join(c if c in "ACGT" else "N" for c in R2[i])); quals.append(Q2[i])
    return rows, quals, other


def check_batch(eng, got, info, rows, quals, flag=0, with_quals=True):  # noqa: F811
    assert got.n == len(rows) and info == (len(rows), sum(len(r) for r in rows), max([len(r) for r in rows] + [0]), flag), (info, len(rows))
    if rows:
        up = eng.upload(rows, flags=KMERS_ONLY)
        try:
            g, u = got.read(), up.read()
            for k in range(3):   # pk, nm, len
                assert g[k].shape == u[k].shape and (g[k] == u[k]).all(), (k, np.argwhere(g[k] != u[k])[:4])
            assert g[4] == u[4] and not g[3].any()   # the longest read; no low-complexity byte is set
        finally:
            up.close()
    q = got.quals()
    if not with_quals:
        assert q is None
        return
    qb, off = q
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in quals], dtype=np.int64)]).tolist()
    assert qb.tobytes() == "".join(quals).encode("latin-1")


def run_pairs(eng, pieces, R1, Q1, R2, Q2, skip=None, with_quals=True, **how):  # noqa: F811
    """scan, process_pairs, pairs_batch of the whole piece, compared -> (batch, rows, qualities, process_pairs' result)"""
    a, b = scan_pair(pieces, R1, Q1, R2, Q2, **how)
    ahead = how.get("ahead", 0)
    res = a.process_pairs(b, first_mate=ahead, skip=skip)
    rows, quals, flag = expected_rows(res, R2, Q2)
    got, info = a.pairs_batch(b, first_mate=ahead, with_quals=with_quals)
    check_batch(eng, got, info, rows, quals, flag, with_quals)
    got.flag = flag
    return got, rows, quals, res


def test_pair_cases(eng, pieces, cases):  # noqa: F811
    R1, Q1, R2, Q2 = cases
    got, rows, quals, res = run_pairs(eng, pieces, R1, Q1, R2, Q2)
    got.close()
    kinds = {r[0] for r in res}
    assert kinds == {0, 1, 2, 3}
    assert any(r[3] & 4 for r in res)                                     # a merged read, listed twice
    assert any(r[0] == 1 and r[3] & 1 for r in res)                       # a changed read (cut to the overlap), taken from where it was written
    assert any(not r[3] & 1 for r in res)                                 # a read 1 dropped as of low complexity
    assert len(rows) > N_CASES and len(R1) > 256                          # more than one workgroup of the row scan


def test_edge_pairs(eng, pieces):  # noqa: F811
    R1, Q1, R2, Q2 = (list(x) for x in edge_pairs())
    keep = [i for i in range(len(R1)) if i != 5]   # (pair 5 merges into 728 bases: test_refusals)
    sel = lambda X: [X[i] for i in keep]
    got, rows, quals, res = run_pairs(eng, pieces, sel(R1), sel(Q1), sel(R2), sel(Q2))
    got.close()
    assert {r[0] for r in res} == {0, 1, 2, 3} and any("N" in r for r in rows)
    assert got.flag == 1 and any("R" in r for r in rows)   # (one read 1 holds R / Y)


def edge_length_pairs(L, rnd):
    """pairs of two unrelated reads of L bases (not of low complexity where a read of L bases can be anything else), one with N"""
    def seq():
        for _ in range(200):
            s = "".join(rnd.choice("ACGT") for _ in range(L))
            if not py_low(s):
                return s
        return s
    R1, R2 = [seq() for _ in range(5)], [seq() for _ in range(5)]
    if L >= 31:
        R1[1] = R1[1][:L - 1] + "N"; R2[2] = "N" + R2[2][1:L - 2] + "NN"   # (the last bits of the last nm word; its first)
    qual = lambda: "".join(rnd.choice("#5FI~!") for _ in range(L))
    return R1, [qual() for _ in R1], R2, [qual() for _ in R2]


@pytest.mark.parametrize("L", EDGE_LENGTHS)
def test_edge_lengths(eng, pieces, L):  # noqa: F811
    for seed in range(100 + L, 140 + L):   # (short random mates may overlap by chance: pairs that all stay as they are)
        R1, Q1, R2, Q2 = edge_length_pairs(L, random.Random(seed))
        if all(r[0] == 0 for r in scan_pair(pieces, R1, Q1, R2, Q2)[0].process_pairs(pieces[1])):
            break
    assert all(len(x) == L for x in R1 + R2 + Q1 + Q2)
    got, rows, quals, res = run_pairs(eng, pieces, R1, Q1, R2, Q2)
    got.close()
    if L >= 15:
        assert rows and max(len(r) for r in rows) == L
    else:
        assert not rows   # (reads of 0 or 1 bases are of low complexity: an empty batch)


def test_low_complexity_drops_and_skips(eng, pieces, cases):  # noqa: F811
    rnd = random.Random(3)
    rn = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    # read 2 dropped; read 1 dropped; both dropped; both kept
    R1, R2 = [rn(60), "A" * 60, "C" * 50, rn(70)], ["A" * 60, rn(60), "G" * 40 + "T" * 5, rn(70)]
    Q1, Q2 = ["F" * len(x) for x in R1], ["5" * len(x) for x in R2]
    got, rows, quals, res = run_pairs(eng, pieces, R1, Q1, R2, Q2)
    got.close()
    assert [r[3] & 3 for r in res] == [1, 2, 0, 3] and rows == [R1[0], R2[1], R1[3], R2[3]]
    # skip bytes 1 (a dropped pair) and 2 (another rank's): neither gives a row
    R1, Q1, R2, Q2 = (x[:90] for x in cases)
    skip = np.array([1 + (i % 2) if i % 3 == 0 else 0 for i in range(90)], dtype=np.uint8)
    got, rows, quals, res = run_pairs(eng, pieces, R1, Q1, R2, Q2, skip=skip)
    got.close()
    assert sum(r is None for r in res) == 30 and rows
    # every pair skipped: an empty batch
    got, rows, quals, res = run_pairs(eng, pieces, R1, Q1, R2, Q2, skip=np.ones(90, dtype=np.uint8))
    got.close()
    assert rows == []


def test_part_of_a_piece(eng, pieces, cases):  # noqa: F811
    R1, Q1, R2, Q2 = (x[:60] for x in cases)
    a, b = scan_pair(pieces, R1, Q1, R2, Q2, ahead=3, open_end=True)
    # first_read != first_mate, n smaller than the piece
    res = a.process_pairs(b, first=7, first_mate=10, n=21)
    rows, quals, _ = expected_rows(res, R2[7:28], Q2[7:28])
    got, info = a.pairs_batch(b, first=7, first_mate=10, n=21)
    check_batch(eng, got, info, rows, quals)
    got.close()
    # without qualities
    got, info = a.pairs_batch(b, first=7, first_mate=10, n=21, with_quals=False)
    check_batch(eng, got, info, rows, quals, with_quals=False)
    got.close()
    # n = 0
    assert a.process_pairs(b, first=40, first_mate=43, n=0) == []
    got, info = a.pairs_batch(b, first=40, first_mate=43, n=0)
    check_batch(eng, got, info, [], [])
    got.close()


def other_letter_pairs():
    rnd = random.Random(15)
    t = "".join(rnd.choice("ACGT") for _ in range(260))
    r1, r2 = t[:150], list(rc(t[110:]))
    r2[3] = "R"; r2[140] = "Y"
    far = "".join(rnd.choice("ACGT") for _ in range(150))
    r3 = list(far); r3[7] = "K"
    # a merged pair with Y inside the overlap of read 2; a plain pair with R / Y in read 2; the same with K in read 1
    return [r1, far, "".join(r3)], ["F" * 150] * 3, ["".join(r2)] * 3, ["F" * 150] * 3


def test_other_letters(eng, pieces):  # noqa: F811
    R1, Q1, R2, Q2 = other_letter_pairs()
    # in read 2 only: the rows hold N, the flag is clear
    got, rows, quals, res = run_pairs(eng, pieces, R1[:2], Q1[:2], R2[:2], Q2[:2])
    got.close()
    assert got.flag == 0 and res[1][3] & 2 and rows[-1].count("N") == 2 and "R" not in rows[-1]
    # in a read 1: code 3 as an upload packs it, the flag is set
    got, rows, quals, res = run_pairs(eng, pieces, R1, Q1, R2, Q2)
    got.close()
    assert got.flag == 1 and "K" in rows[-2]


def test_batch_outlives_the_piece(eng, pieces, cases):  # noqa: F811
    R1, Q1, R2, Q2 = (x[:40] for x in cases)
    got, rows, quals, _ = run_pairs(eng, pieces, R1, Q1, R2, Q2)
    a, b = pieces
    a.scan(fastq(["ACGT"])); b.scan(fastq(["ACGT"]))   # the pieces are gone; the batch owns its rows and qualities
    check_batch(eng, got, (len(rows), sum(len(r) for r in rows), max(len(r) for r in rows), 0), rows, quals)
    got.close()


@pytest.fixture(scope="module")
def counted(eng, pieces, cases):  # noqa: F811
    """120 pairs: the batch from the device's text, the same reads uploaded, and counters fed the one and the other"""
    R1, Q1, R2, Q2 = (x[:120] for x in cases)
    got, rows, quals, _ = run_pairs(eng, pieces, R1, Q1, R2, Q2)
    up = eng.upload(rows, flags=KMERS_ONLY)
    kc = eng.kmer_counter(21, max_kmers=1)
    kc.reserve(sum(len(r) for r in rows)).add(got)
    ref = eng.kmer_counter(21, max_kmers=sum(max(0, len(r) - 20) for r in rows) + 8).add(up)
    yield got, up, kc, ref, rows, quals
    for o in (got, up, kc, ref):
        o.close()


def test_counts(eng, counted):  # noqa: F811
    got, up, kc, ref, rows, quals = counted
    as_dict = lambda c: dict(zip(*[x.tolist() for x in c.export()]))
    mine = as_dict(kc)
    assert len(mine) > 1024 * 6 // 10 and mine == as_dict(ref)   # (beyond what max_kmers = 1 stood for: 1024 slots)
    oracle = KmerCountChecker(21)
    for r in rows:
        oracle.add(r)
    for use_q in (False, True):
        mn, md, av, ln = kc.stats_resident(got, use_q)
        for i, r in enumerate(rows):
            _, omn, omd, oav, after, _ = oracle.stats(r, quals[i] if use_q else None)
            assert (int(mn[i]), int(md[i]), int(ln[i])) == (omn, omd, len(after)) and same(float(av[i]), float(oav)), (i, use_q, r)


def test_stats_resident(eng, counted):  # noqa: F811
    got, up, kc, ref, rows, quals = counted
    for use_q in (False, True):
        a, b = kc.stats_resident(got, use_q), ref.stats(up, quals if use_q else None)
        for k in range(4):
            assert a[k].dtype == b[k].dtype and (a[k] == b[k]).all(), (use_q, k)
    assert (kc.stats_resident(got, True)[3] < np.array([len(r) for r in rows])).any()   # some read is trimmed


def test_refusals(eng, pieces, cases):  # noqa: F811
    import trust4_amd
    R1, Q1, R2, Q2 = (x[:30] for x in cases)

    def refused(call, code, word):
        with pytest.raises(trust4_amd.api.T4Error) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    a, b = scan_pair(pieces, R1, Q1, R2, Q2)
    refused(lambda: a.pairs_batch(b), T4_ERR_ARG, "did not succeed")                 # no process_pairs since the scan
    a.process_pairs(b, first=2, first_mate=2, n=20)
    refused(lambda: a.pairs_batch(b), T4_ERR_ARG, "covered")                         # another range
    refused(lambda: a.pairs_batch(b, first=2, first_mate=3, n=20), T4_ERR_ARG, "covered")
    refused(lambda: b.pairs_batch(a, first=2, first_mate=2, n=20), T4_ERR_ARG, "did not succeed")   # the handles the other way round
    a.pairs_batch(b, first=2, first_mate=2, n=20)[0].close()
    b.scan(b.data)                                                                   # a rescan in between, of either piece
    refused(lambda: a.pairs_batch(b, first=2, first_mate=2, n=20), T4_ERR_ARG, "scanned again")
    a.process_pairs(b)
    a.scan(a.data)
    refused(lambda: a.pairs_batch(b), T4_ERR_ARG, "did not succeed")
    with pytest.raises(trust4_amd.api.T4Error):                                      # a prior call that ran out of room
        a.process_pairs_raw(b, out_cap=0)
    refused(lambda: a.pairs_batch(b), T4_ERR_ARG, "did not succeed")
    # a merged row beyond 384: two 250-base mates that overlap by 30
    rnd = random.Random(8)
    t = "".join(rnd.choice("ACGT") for _ in range(470))
    L1, LQ1, L2, LQ2 = list(R1[:5]) + [t[:250]], list(Q1[:5]) + ["F" * 250], list(R2[:5]) + [rc(t[220:])], list(Q2[:5]) + ["F" * 250]
    a, b = scan_pair(pieces, L1, LQ1, L2, LQ2)
    res = a.process_pairs(b)
    assert res[5][0] == 2 and len(res[5][1]) == 470
    refused(lambda: a.pairs_batch(b), T4_ERR_UNSUPPORTED, "470")
    run_pairs(eng, pieces, R1, Q1, R2, Q2)[0].close()                                # ... and the handles serve a normal piece
    # use_quals on a batch without qualities
    got, _ = pieces[0].pairs_batch(pieces[1], with_quals=False)
    kc = eng.kmer_counter(21, max_kmers=1 << 16).add(got)
    try:
        refused(lambda: kc.stats_resident(got, True), T4_ERR_ARG, "no qualities")
        assert len(kc.stats_resident(got, False)[0]) == got.n
    finally:
        kc.close()
        got.close()
