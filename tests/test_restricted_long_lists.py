"""Restricted re-queries of reads that meet posting lists beyond 10000 entries (t4_kernels.h restrictedRepeatTests).

Such a read switches on removeOnlyRepeats in GetOverlapsFromHits (SeqSet.hpp:796-806): a (strand, contig) group without a hit of
a list of at most 10000 postings is dropped (871-887), and so is a concordant run [s, e) of a group unless one of the first e
entries of the WHOLE hit array from s on is such a hit (931-947, the quirk: k indexes the whole array). A restricted re-query --
the overlaps of the read with ONE contig -- applies both tests once it is armed with what the read's last whole query left: the
two flags, M and the head of the hit array as a bitmap (t4_add_query_head).

Case 1 holds the kernel against the oracle: GetOverlapsFromHits(filter = 1) over the whole read, cut down to the probed contig.
"""
import random

import numpy as np
import pytest

import t4check
from test_wide_query import build_set, groups_of, rc

K, HIT_LEN = 9, 17
N_CONTIGS = 10400       # the smallest count that puts the shared segment's lists beyond 10000 postings


def long_list_set(eng, seed=8):
    """The set of test_wide_query.run_huge_lists -- every contig carries one 48-bp segment, a few carry a `private` stretch left of
    it -- with reads that take only the last 12 bases of a private stretch. The repeat-skip rule of GetHitsFromRead emits every
    fifth k-mer of the shared segment, so a contig without the stretch holds 9 hits with the read and one with it 18: they leave
    novelMinHitRequired at 18 / 2 = 9, which the 9 long-list hits of the others still reach -- nothing but the removeOnlyRepeats
    tests keeps those out of the result. Reads given as their reverse complement put long-list entries at the head of the hit
    array (the minus strand's groups come first), which is where the run test alone drops runs."""
    rnd = random.Random(seed)
    shared = "".join(rnd.choice("ACGT") for _ in range(48))
    private = ["".join(rnd.choice("ACGT") for _ in range(70)) for _ in range(6)]
    contigs = []
    for i in range(N_CONTIGS):
        left = private[i % 6] if i % 1733 < 3 else "".join(rnd.choice("ACGT") for _ in range(rnd.randint(20, 40)))
        s = left + shared + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(10, 30)))
        w = np.zeros((len(s), 4), dtype=np.int32)
        for j, ch in enumerate(s):
            w[j, "ACGT".index(ch)] = rnd.randint(1, 9)
        contigs.append(("c%d" % i, s, w))
    o, ix = build_set(eng, contigs, K, HIT_LEN)
    reads = []
    for t in range(6):
        rd = private[t][58:] + shared
        reads.append(rd if t % 2 == 0 else rc(rd))
    reads.append(private[0][:64])      # not `huge`: every list it meets is short
    carriers = {t: [i for i in range(N_CONTIGS) if i % 1733 < 3 and i % 6 == t] for t in range(6)}
    return o, ix, reads, carriers


def oracle_view(o, read):
    """what the oracle alone says of a read: the overlaps of GetOverlapsFromHits(filter 1) by contig; per (contig, strand) the hits
    as (read offset, contig offset, repeats); the head of the hit array in the reference's order (strand, contig, read offset) as
    0 / 1 values, 1 = a list of at most 10000 postings; novelMinHitRequired per strand (minus, plus)"""
    by_contig = {}
    for tup, _chain in o.overlaps_from_hits(read, strand=0, hit_len_required=HIT_LEN, filt=1, cap=2 * N_CONTIGS + 64, ccap=1 << 21):
        by_contig.setdefault(tup[0], set()).add(tup[1:6])
    hits = o.hits(read, strand=0, cap=1 << 22).tolist()
    hits.sort(key=lambda h: (h[3], h[0], h[2]))
    groups = {}
    for idx, off, roff, st, rep in hits:
        groups.setdefault((idx, 1 if st == 1 else 0), []).append((roff, off, rep))
    # the statistics loop of SeqSet.hpp:784-823, with its `i = j` before the loop's own `++i`
    possible, longest, i = [0, 0], [0, 0], 0
    while i < len(hits):
        j = i + 1
        while j < len(hits) and hits[j][3] == hits[i][3] and hits[j][0] == hits[i][0]:
            j += 1
        plus = 1 if hits[i][3] == 1 else 0
        possible[plus] += 1 if j - i > 3 else 0
        longest[plus] = max(longest[plus], j - i)
        i = j + 1
    thr = []
    for t in range(2):
        p, big = possible[t], longest[t]
        thr.append(int(big * 0.75) if p > 100000 else big // 2 if p > 10000 else big // 3 if p > 1000 else big // 4 if p > 100 else 3)
    return by_contig, groups, [1 if h[4] <= 10000 else 0 for h in hits], thr


def classify(by_contig, groups, thr):
    """contigs with a run that passes the size tests of SeqSet.hpp:923-925, by what the oracle makes of them: a -- long-list hits
    only (the group test drops the group); b -- a hit of a shorter list, and the oracle forms an overlap; c -- a hit of a shorter
    list, so the group test passes, and still no overlap: the run test alone dropped every run"""
    kinds = {"a": [], "b": [], "c": []}
    for (c, plus), hits in groups.items():
        diag = {}
        for roff, off, _rep in hits:
            diag[roff - off] = diag.get(roff - off, 0) + 1
        if not any(n >= thr[plus] and n * K >= HIT_LEN for n in diag.values()):
            continue
        uniq = any(rep <= 10000 for _, _, rep in hits)
        kinds["a" if not uniq else "b" if by_contig.get(c) else "c"].append(c)
    return kinds


def group_info(groups, c):
    """the group-info bits of contig c as the wide records carry them: minus group | plus group << 4"""
    out = 0
    for plus in (0, 1):
        hits = groups.get((c, plus), [])
        if hits:
            small = sum(1 for _, _, rep in hits if rep <= 10000)
            out |= (min(small, 4) | (8 if min(hits)[2] <= 10000 else 0)) << (4 * plus)
    return out


def restricted(eng, ix, read, contigs, force, armed=None):
    """restricted re-queries of one read against `contigs` -> per contig (status, set of overlap geometry, info word)"""
    n = len(contigs)
    if armed is not None:
        m, words, ror = armed
        eng.arm_long_lists([ror | 4 | (m << 3)] * n, [0] * n, words)
    res = eng.add_query_whole(ix, [read] * n, only_seq=contigs, force_min=[force] * n)
    info = eng.last_long_lists()
    assert (info is None) == (armed is None)
    out = []
    for t in range(n):
        geo = set() if res["ov"][t] is None else {tuple(int(x) for x in r.tolist()[1:6]) for r in res["ov"][t]}
        out.append((int(res["status"][t]), geo, 0 if info is None else int(info[t])))
    return out


def run_kernel_against_oracle(make_engine):
    eng = make_engine()
    o, ix, reads, carriers = long_list_set(eng)
    whole = eng.add_query_whole(ix, reads)
    heads = [eng.query_head(i) for i in range(len(reads))]
    wide = [groups_of(eng, i) for i in range(len(reads))]
    seen = {"a": set(), "b": set(), "c": set()}
    for i, read in enumerate(reads[:-1]):
        assert wide[i] is not None and wide[i][1] == 1 and heads[i] is not None, (i, "a read with lists beyond 10000 postings, served by the wide query")
        m, words, ror = heads[i]
        by_contig, groups, flat, thr = oracle_view(o, read)
        assert [int(whole["stats"][i][6]), int(whole["stats"][i][7])] == thr, (i, "novelMinHitRequired")
        force = thr[0] | (thr[1] << 16)
        assert [(int(words[k >> 5]) >> (k & 31)) & 1 for k in range(m)] == flat[:m], (i, "head bitmap")
        # the probed contigs, classified by the oracle's hits alone: the carriers of the read's private stretch and a few of each kind
        kinds = classify(by_contig, groups, thr)
        kind_of = {c: kd for kd, lst in kinds.items() for c in lst}
        probe = list(carriers[i])
        for kd in "abc":
            probe += [c for c in kinds[kd] if c not in probe][:4]
        for c in probe:
            if c in kind_of:
                seen[kind_of[c]].add((i, c))
        got = restricted(eng, ix, read, probe, force, armed=(m, words, ror))
        plain = restricted(eng, ix, read, probe, force)
        for c, (status, geo, info), (status0, geo0, _) in zip(probe, got, plain):
            want = by_contig.get(c, set())
            print("read %d contig %d kind %s: oracle %d overlaps, armed %d (status %d), not armed %d" % (i, c, kind_of.get(c, "-"), len(want), len(geo), status, len(geo0)))
            assert status == 0 and geo == want, (i, c, kind_of.get(c), sorted(geo), sorted(want))
            assert info == (0x100 | group_info(groups, c)), (i, c, hex(info), hex(group_info(groups, c)))
            if kind_of.get(c) in ("a", "c"):   # the negative control: without the tests the kernel forms overlaps the reference never does
                assert status0 == 0 and geo0 != want, (i, c, kind_of[c])
        # a run that ends beyond the head is not guessed
        beyond = (kinds["b"] + kinds["c"])[:1]
        assert beyond and m > 4
        short = restricted(eng, ix, read, beyond, force, armed=(4, words[:1], ror))
        assert short[0][0] == 5 and not short[0][1], (i, short)
    assert len(seen["a"]) >= 3 and len(seen["b"]) >= 3 and len(seen["c"]) >= 1, {k: len(v) for k, v in seen.items()}
    # a read that is not `huge`: nothing to arm, today's records
    i = len(reads) - 1
    assert heads[i] is None
    by_contig, groups, _flat, thr = oracle_view(o, reads[i])
    assert [int(whole["stats"][i][6]), int(whole["stats"][i][7])] == thr
    force = thr[0] | (thr[1] << 16)
    probe = carriers[0] + [7]
    for c, (status, geo, info) in zip(probe, restricted(eng, ix, reads[i], probe, force)):
        assert status == 0 and geo == by_contig.get(c, set()) and info == 0, (c, sorted(geo))
    assert by_contig.get(carriers[0][0])


def test_restricted_requery_applies_the_repeat_tests_emulated(monkeypatch):
    monkeypatch.setenv("T4_LIB", t4check.build_emulator_lib())
    monkeypatch.delenv("T4_WIDE_PCAP", raising=False)
    monkeypatch.delenv("T4_AQ_CAP_LIMIT", raising=False)
    import trust4_amd
    run_kernel_against_oracle(lambda: trust4_amd.Engine(0))


@pytest.mark.gpu
def test_restricted_requery_applies_the_repeat_tests_gpu(monkeypatch):
    monkeypatch.delenv("T4_LIB", raising=False)
    monkeypatch.delenv("T4_WIDE_PCAP", raising=False)
    monkeypatch.delenv("T4_AQ_CAP_LIMIT", raising=False)
    import trust4_amd
    run_kernel_against_oracle(lambda: trust4_amd.Engine(0))


# ---- case 2: the ordered contig builder in lock-step with the compiled reference ----------------------------------------------------
def long_list_stream(seed=8):
    """The same set offered as novel reads, and two dozen reads of two private stretches behind it: every one overlaps the few
    contigs that carry its stretch (and meets the shared segment's lists of more than 10000 postings), the first of a stretch extends
    one of those contigs to the right, the others sit inside them. All on the strand of the contigs: no overlap on the other one."""
    rnd = random.Random(seed)
    shared = "".join(rnd.choice("ACGT") for _ in range(48))
    private = ["".join(rnd.choice("ACGT") for _ in range(70)) for _ in range(6)]
    contigs = []
    for i in range(N_CONTIGS):
        left = private[i % 6] if i % 1733 < 3 else "".join(rnd.choice("ACGT") for _ in range(rnd.randint(20, 40)))
        contigs.append(left + shared + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(10, 30))))
    reads = []
    for n in range(12):
        for t in (4, 5):
            c = [i for i in range(N_CONTIGS) if i % 1733 < 3 and i % 6 == t][-1]
            tail = contigs[c][70 + 48:]
            if n == 0:
                reads.append(private[t][40:] + shared + tail + "".join(rnd.choice("ACGT") for _ in range(25)))
            else:
                reads.append(private[t][58 - 3 * n:] + shared + tail[:rnd.randint(0, len(tail))])
    return contigs, reads


def drive_long_lists(asm, contigs, reads, window=0):
    log = []
    for i, s in enumerate(contigs):
        log.append(("new", asm.input_novel_read("c%d" % i, s, 1, -1)))
    for i, rd in enumerate(reads):
        if window and not asm.window_valid():
            asm.prefetch(reads[i: i + window], [0] * len(reads[i: i + window]))
        ret, strand = asm.add_read(rd, "", 0, -1, 1, 0, 0.9)
        log.append(("add", ret, strand))
    asm.update_all_consensus()
    return log


def run_lock_step(eng, tmp_path, monkeypatch, capfd):
    import ctypes as C
    import filecmp
    import re
    import trust4_amd
    from t4libs import Ref, RefSeqSet
    if not Ref.available():
        pytest.skip("oracle/_ref/libt4ref.so not built")
    contigs, reads = long_list_stream()
    ref = RefSeqSet(K)
    log_ref = drive_long_lists(ref, contigs, reads)
    pa = str(tmp_path / "ref_raw.out")
    ref.output(pa)
    assert sum(1 for x in log_ref if x[0] == "add" and x[1] >= 0) >= len(reads) // 2
    counters = {}
    monkeypatch.setenv("T4_VERIFY_WINDOW", "1")
    for switch in (True, False):
        if switch:
            monkeypatch.setenv("T4_FRAGILE_CHECKS", "1")
        else:
            monkeypatch.delenv("T4_FRAGILE_CHECKS")
        mine = trust4_amd.Assembler(eng, K)
        log_mine = drive_long_lists(mine, contigs, reads, window=len(reads))
        first_diff = next((i for i, (a, b) in enumerate(zip(log_ref, log_mine)) if a != b), None)
        assert first_diff is None and len(log_ref) == len(log_mine), (switch, first_diff, log_ref[first_diff], log_mine[first_diff])
        pb = str(tmp_path / ("mine_raw_%d.out" % switch))
        mine.output(pb)
        assert filecmp.cmp(pa, pb, shallow=False), switch
        assert mine.counters()["window_hits"] > 0
        capfd.readouterr()
        lc = (C.c_int64 * 30)()
        eng.check(eng.lib.t4_assembler_live_counters(mine.h, lc, 30))
        v = re.search(r"T4_VERIFY_WINDOW: (\d+) served window entries queried again at serve time, all equal to their cached results", capfd.readouterr().err)
        assert v and int(v.group(1)) > 0
        counters[switch] = (int(lc[28]), int(lc[29]), int(lc[27]), int(v.group(1)))
        mine.close()
    for switch in (True, False):
        print("T4_FRAGILE_CHECKS %s: [28] %d, [29] %d, wide-served entries %d, entries verified %d" % (("set" if switch else "unset",) + counters[switch]))
    assert counters[True][0] > 0, counters
    assert counters[False][0] == 0 and counters[False][1] > 0, counters


def test_assembler_serves_long_list_entries_by_restricted_requeries_emulated(tmp_path, monkeypatch, capfd):
    import test_assign_wide as A
    for a in A.AIDS:
        monkeypatch.delenv(a, raising=False)
    eng = A.make_engine(True)
    try:
        run_lock_step(eng, tmp_path, monkeypatch, capfd)
    finally:
        eng.close()
        monkeypatch.delenv("T4_LIB", raising=False)


@pytest.mark.gpu
def test_assembler_serves_long_list_entries_by_restricted_requeries_gpu(tmp_path, monkeypatch, capfd):
    import test_assign_wide as A
    for a in A.AIDS:
        monkeypatch.delenv(a, raising=False)
    eng = A.make_engine(False)
    try:
        run_lock_step(eng, tmp_path, monkeypatch, capfd)
    finally:
        eng.close()
