"""The k-mer counter (t4_kmer_count_*) at its table, key and trimming edges; the cases and the predicates that prove an edge is hit
come from kmer_edge_gen. Every comparison is exact. Statistics are compared with the C oracle (t4o_kc_*), table contents with a
Python dict of the keys. Each engine test runs on the emulator build of the kernel source and, with -m gpu, on the product library,
from the same cases; no case is left out by looking at what the engine returned.

What the table does, as far as these tests rely on it (t4_kmer_count_create, kmerEnsureRoom in csrc/t4_api.hip):
  * max_kmers <= 512 gives a table of 1 024 slots that is also its ceiling; only reserve() and merge() move the ceiling.
  * reserve(n) on such a counter doubles the ceiling until (used + n) * 10 <= ceiling * 6, then rehashes into tables four times as
    large, capped by the ceiling, until the table is the ceiling. slots * 6 = 3 * 2^j is never a multiple of 10, so the condition
    cannot hold with equality: the tests sit one below and one above it (used + n = 614 / 615 for 1 024 slots, 2 457 / 2 458 for
    4 096, 4 915 / 4 916 for 8 192).
  * The size is read off by filling the table: set() takes exactly slots - used new codes, one more is refused (and the message
    names the slots). set() itself grows a table that is below its ceiling, so what is pinned is the ceiling reserve() chose, to
    which it also brings the table; the load at which a table below its ceiling is rehashed shows in no result.
  * merge() without only_present raises the ceiling like reserve() (include/trust4_hip.h: "the table grows beyond what max_kmers
    ... stood for"), so a further k-mer merged into a full table is taken and the table grows; set() and add() refuse it.
  * t4_kmer_count_add slices a batch and grows between slices only while the table is below its ceiling. Without the T4_KC_SLOTS
    test knob that needs a first table of 2^22 slots and over a million distinct k-mers, beyond what a test here may take;
    test_kmer_count_emu.test_kmer_count_table_grows_emulated covers it with the knob. Here a batch of more than 4 096 reads goes into
    a counter that reserve() grew first.
An MI355X has 256 compute units, so the add and statistics launches have 8 192 workgroups; the 10 000-read batch exceeds that
(test_more_reads_than_workgroups asserts it against t4_device_cus). The run on an MI355X, tables of 1 024 to 16 384 slots filled to
load 1.0 among it, is profiles/r16_gpu_kmer_count_edges.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmer_edge_gen as g
from t4libs import KmerCountChecker, Ref
from test_fastq_text import eng, py_low  # noqa: F401 (the fixture)
from test_text_pairs import scan_pair
from test_text_pairs_batch import expected_rows

T4_ERR_ARG, T4_ERR_UNSUPPORTED = -1, -4
V = C.c_void_p


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def refused(call, code, *words):
    import trust4_amd
    with pytest.raises(trust4_amd.api.T4Error) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def as_dict(kc):
    codes, vals = kc.export()
    assert len(set(codes.tolist())) == len(codes) == kc.distinct()   # `used` (what export reports) == occupied slots
    return dict(zip(codes.tolist(), vals.tolist()))


def kc_set(eng, kc, table):  # noqa: F811
    codes, vals = np.array(list(table.keys()), dtype=np.uint64), np.array(list(table.values()), dtype=np.int32)
    eng.check(eng.lib.t4_kmer_count_set(kc.h, codes.ctypes.data_as(V), vals.ctypes.data_as(V), C.c_int64(len(codes))))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def same_avg(a, b):
    """float32 values with the same bits (so +-inf must match), or both NaN"""
    return bits(a) == bits(b) or (np.isnan(np.float32(a)) and np.isnan(np.float32(b)))


def oracle_for(reads, k):
    o = KmerCountChecker(k)
    for r in reads:
        o.add(r)
    return o


@functools.lru_cache(maxsize=None)
def oracle_results(k):
    """t4o_kc_stats of every case of stats_cases(k), computed once: [(min, median, avg, length afterwards, read afterwards)]"""
    adds, cases, _ = g.stats_cases(k)
    o = oracle_for(adds, k)
    out = []
    for c in cases:
        _, mn, md, av, after, _ = o.stats(c["read"], c["qual"])
        out.append((mn, md, av, len(after), after))
    return tuple(out)


def check_stats(got, want, what):
    """got: (min, median, avg, new_len) arrays of the engine; want: [(min, median, avg, new_len, ...)] of the oracle"""
    mn, md, av, ln = got
    for i, w in enumerate(want):
        e = (int(mn[i]), int(md[i]), float(av[i]), int(ln[i]))
        assert e[:2] == w[:2] and same_avg(e[2], w[2]) and e[3] == w[3], (what(i), e, w[:4])


def stats_by_quals(kc, eng, cases):  # noqa: F811
    """engine statistics of the cases, those without qualities in one call and those with in another -> [(mn, md, av, ln)] per case"""
    out = [None] * len(cases)
    for with_q in (False, True):
        idx = [i for i, c in enumerate(cases) if (c["qual"] is not None) == with_q]
        b = eng.upload([cases[i]["read"] for i in idx])
        mn, md, av, ln = kc.stats(b, [cases[i]["qual"] for i in idx] if with_q else None)
        b.close()
        for j, i in enumerate(idx):
            out[i] = (int(mn[j]), int(md[j]), float(av[j]), int(ln[j]))
    return out


# ---- the generator itself (no engine) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", g.KS)
def test_cases_sit_on_their_edges(k):
    adds, cases, table = g.stats_cases(k)
    any_case = lambda p: any(p(c) for c in cases)
    lens = {len(c["read"]) for c in cases}
    assert {k - 1, k, k + 1, k + 63, k + 64, k + 65, 383, 384} <= lens
    assert any_case(lambda c: len(c["read"]) == k - 1 and c["qual"] is not None and c["model"]["mn"] == -1 and c["model"]["new_len"] == k - 1)
    assert max(table.values()) > 2 and min(table.values()) >= 1          # reads added several times
    # where the trim lands
    assert any_case(lambda c: g.trims_at(c, k + 1)) and any_case(lambda c: g.trims_at(c, k) and c["model"]["kk"] == 1 and c["model"]["new_len"] == k)
    if k > 1:
        assert any_case(lambda c: g.trims_at(c, k - 1) and g.emptied(c) and c["model"]["avg"] == float("inf"))
    else:   # trimStart 0 does not trim although every byte is bad
        assert any_case(lambda c: c["qual"] is not None and c["model"]["trim"] == 0 and c["model"]["new_len"] == len(c["read"]) and set(c["qual"]) == {"/"})
    # quality bytes on both sides of the edge, where the scan looks at them
    for byte in (47, 48, 33, 126):
        assert any_case(lambda c: g.byte_scanned(c, byte)), byte
    # the 10 % rule
    for m in g.EQ_TAILS:
        if max(k, 4) + m <= g.MAXL:
            assert any_case(lambda c: g.rule_at_equality(c, m)) and any_case(lambda c: g.rule_one_below_equality(c, m)), m
    assert (k <= 2) == any_case(lambda c: g.rule_at_equality(c, 380))    # j >= k - 1 and len <= 384: only a small k reaches 380
    for m in g.CEIL_TAILS:
        for side, trimmed in (("meets", True), ("misses", False)):
            c = [c for c in cases if c["tag"][:3] == ("rule", m, side)]
            assert c and all((x["model"]["trim"] > 0) == trimmed and len(x["read"]) - x["model"]["lo"] == m for x in c), (m, side)
    assert any_case(g.rule_meets_fails_meets)
    # the protected region
    prot = {c["tag"][1:]: c for c in cases if c["tag"][0] == "protected"}
    for m in (10, 11):
        c = prot[(m, "below")]
        assert c["model"]["trim"] == -1 and "/" in c["qual"][:c["model"]["lo"]] and "/" not in c["qual"][c["model"]["lo"]:]
        c = prot[(m, "at")]
        assert c["qual"][c["model"]["lo"]] == "/" and (c["model"]["trim"] == c["model"]["lo"]) == (m <= 10)
    # median
    med = {c["tag"][1:]: c["model"] for c in cases if c["tag"][0] == "median"}
    assert {med[("equal", n)]["kk"] for n in (7, 8, 1)} == {7, 8, 1}
    assert med[("halves",)]["kk"] == 10 and med[("halves",)]["md"] > 1
    m = med[("after trim",)]
    assert m["kk"] == 7 < m["n"] == 13 and m["md"] > 1      # over the 13 counts of the whole read the median would be 1
    assert med[("kk>n",)]["kk"] > med[("kk>n",)]["n"] and med[("kk>n",)]["mn"] == 0
    m = med[("kk>2n",)]
    assert (m["n"], m["kk"], m["md"]) == (16, 36, 0)        # the median is an entry the read never wrote
    # N rule
    nn = {c["tag"][1:]: c for c in cases if c["tag"][0] == "N"}
    assert nn[("one", "q")]["model"]["mn"] == 0 and nn[("several",)]["model"]["mn"] == 0
    assert nn[("at trimStart",)]["model"]["mn"] >= 1 and nn[("after trimStart",)]["model"]["mn"] == 0
    c = nn[("first, emptied",)]
    assert c["read"][0] == "N" and (g.emptied(c) and c["model"]["mn"] >= 1 if k > 1 else c["model"]["mn"] == 0)
    c, L = nn[("every k-mer", "q")], len(nn[("every k-mer",)]["read"])
    assert (c["model"]["mn"], c["model"]["md"], c["model"]["avg"], c["model"]["new_len"]) == (-L, -L, float(-L), 0)
    assert nn[("every k-mer",)]["model"]["new_len"] == L


@pytest.mark.parametrize("k", g.KS)
def test_restatement_equals_oracle(k):
    """py_stats, on which the predicates rest, says what t4o_kc_stats says"""
    _, cases, _ = g.stats_cases(k)
    for c, w in zip(cases, oracle_results(k)):
        m = c["model"]
        assert (m["mn"], m["md"], m["new_len"]) == (w[0], w[1], w[3]) and same_avg(m["avg"], w[2]), (c["tag"], m, w)


def test_reference_comparison_leaves_out_little():
    """the cases the oracle-against-reference comparison must pass over: reads with N only, and less than a quarter of all"""
    skipped = total = 0
    for k in g.KS:
        _, cases, _ = g.stats_cases(k)
        for c, w in zip(cases, oracle_results(k)):
            total += 1
            if g.reference_may_differ(c["read"], c["qual"], w[4]):
                assert "N" in c["read"]
                skipped += 1
    assert 0 < skipped and skipped * 4 < total, (skipped, total)


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("k", g.KS)
def test_oracle_equals_reference(k):
    adds, cases, _ = g.stats_cases(k)
    o, r = KmerCountChecker(k, False), KmerCountChecker(k, True)
    for x in adds:
        assert o.add(x) == r.add(x)
    for c in cases:
        a, b = o.stats(c["read"], c["qual"]), r.stats(c["read"], c["qual"])
        if g.reference_may_differ(c["read"], c["qual"], a[4]):
            continue
        assert a[:3] == b[:3] and same_avg(a[3], b[3]) and a[4:] == b[4:], (c["tag"], a, b)


def test_hash_restatement_places_the_wrap_codes():
    last, first, absent = g.wrap_codes()
    assert len(last) >= 40 and all(g.home(c) >= g.SLOTS0 - 8 for c in last) and all(g.home(c) < 8 for c in first)
    assert min(g.home(c) for c in last) <= 1020 and [g.home(c) for c in absent] == [1020, 0, 3, 30]
    assert len(set(last + first + absent)) == len(last) + len(first) + len(absent)
    assert g.kc_mix(0) == 0 and g.kc_mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF   # splitmix64's finalizer and its first output for seed 0


# ---- 1. statistics and trimming ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", g.KS)
def test_stats_edges(eng, k):  # noqa: F811
    adds, cases, table = g.stats_cases(k)
    kc = eng.kmer_counter(k, max_kmers=sum(max(0, len(r) - k + 1) for r in adds) + 8)
    b = eng.upload(list(adds))
    kc.add(b)
    b.close()
    assert as_dict(kc) == table
    got, want = stats_by_quals(kc, eng, cases), oracle_results(k)
    for c, e, w in zip(cases, got, want):
        assert e[:2] == w[:2] and same_avg(e[2], w[2]) and e[3] == w[3], (k, c["tag"], e, w[:4])
    kc.close()


def test_zero_and_negative_counts_read_as_one(eng):  # noqa: F811
    kmers = ["ACGGTCATTGACCATGCAAGT", "GGATCCATTGACAATGCATGA", "TTGACCGATAGGCATCAGGAC", "CATTAGGACCATAGACCAGAT"]
    table = dict(zip((g.canon(s) for s in kmers), (0, -5, 3, -(1 << 31))))
    kc = eng.kmer_counter(21, max_kmers=64)
    kc_set(eng, kc, table)
    assert as_dict(kc) == table
    read = kmers[2] + kmers[0]   # one k-mer with count 3, one with 0, the 20 between them absent
    b = eng.upload(kmers + [g.rc(kmers[1]), read])
    mn, md, av, ln = kc.stats(b)
    assert mn.tolist() == [1, 1, 3, 1, 1, 1] and md.tolist() == [1, 1, 3, 1, 1, 1]
    assert av.tolist() == [1.0, 1.0, 3.0, 1.0, 1.0, g.f32(24 / 22)] and ln.tolist() == [21] * 5 + [42]
    b.close()
    kc.close()


def test_stats_resident_edges(eng):  # noqa: F811
    """the same kernel on the qualities a t4_text_pairs_batch batch carries: the length family and the 10 % rule cases of k = 21"""
    k = 21
    adds, cases, _ = g.stats_cases(k)
    mine = [c for c in cases if c["qual"] is not None and len(c["read"]) >= 15 and c["tag"][0] in ("len", "rule", "lands", "protected")]
    rnd = np.random.RandomState(5)
    R1, Q1 = [c["read"] for c in mine], [c["qual"] for c in mine]
    R2 = ["".join("ACGT"[x] for x in rnd.randint(0, 4, 60)) for _ in mine]
    Q2 = ["0" * 30 + "/" * 30 for _ in mine]
    pieces = eng.text(1 << 18), eng.text(1 << 18)
    a, b = scan_pair(pieces, R1, Q1, R2, Q2)
    rows, quals, _ = expected_rows(a.process_pairs(b), R2, Q2)
    kept = set(zip(rows, quals))
    assert all((r, q) in kept for r, q in zip(R1, Q1) if not py_low(r)) and sum(not py_low(r) for r in R1) >= 40
    assert {len(r) for r in rows} >= {k - 1, k, k + 1, k + 63, k + 64, k + 65, 383, 384}
    got, _ = a.pairs_batch(b)
    o = oracle_for(adds, k)
    kc = eng.kmer_counter(k, max_kmers=sum(max(0, len(r) - k + 1) for r in adds) + 8)
    up = eng.upload(list(adds))
    kc.add(up)
    for use_q in (False, True):
        want = []
        for r, q in zip(rows, quals):
            _, mn, md, av, after, _ = o.stats(r, q if use_q else None)
            want.append((mn, md, av, len(after)))
        check_stats(kc.stats_resident(got, use_q), want, lambda i: (use_q, rows[i], quals[i]))
    assert any(w[3] < len(r) for w, r in zip(want, rows))
    for x in (got, up, kc) + pieces:
        x.close()


# ---- 2. the table ---------------------------------------------------------------------------------------------------------------
def lookups(eng, kc, codes, k=21):  # noqa: F811
    """the count each canonical k-mer code reads as: statistics of a read that spells it, and of one that spells its reverse"""
    b = eng.upload([g.spell(c, k) for c in codes] + [g.rc(g.spell(c, k)) for c in codes])
    mn, md, av, ln = kc.stats(b)
    b.close()
    n = len(codes)
    assert mn.tolist() == md.tolist() == av.tolist() and mn[:n].tolist() == mn[n:].tolist() and ln.tolist() == [k] * (2 * n)
    return mn[:n].tolist()


def test_probe_chain_wraps(eng):  # noqa: F811
    last, first, absent = g.wrap_codes()
    table = {c: 2 + i for i, c in enumerate(last)}
    kc = eng.kmer_counter(21, max_kmers=512)
    kc_set(eng, kc, table)
    assert as_dict(kc) == table
    table.update({c: 100 + i for i, c in enumerate(first)})   # displaced behind the chain that came over the end of the table
    kc_set(eng, kc, {c: table[c] for c in first})
    assert as_dict(kc) == table
    canonical = [c for c in table if c < (1 << 42) and g.canon(g.spell(c, 21)) == c]
    assert len(canonical) == 52 and len(table) == 60
    assert lookups(eng, kc, canonical) == [table[c] for c in canonical]
    assert lookups(eng, kc, list(absent)) == [1] * len(absent)
    noncanon = [c for c in table if c not in canonical]      # a read that spells one of them looks up its canonical form: absent
    assert len(noncanon) == 8 and lookups(eng, kc, [g.canon(g.spell(c, 21)) for c in noncanon]) == [1] * 8
    both = list(absent) + canonical[:3]                      # merge(only_present): the absent end at the chain's empty slot and stay out
    kc.merge(np.array(both, dtype=np.uint64), np.arange(50, 50 + len(both), dtype=np.int32), only_present=True)
    for i, c in enumerate(canonical[:3]):
        table[c] += 50 + len(absent) + i
    assert as_dict(kc) == table
    b = eng.upload([g.spell(c, 21) for c in canonical[:5]])  # add() finds them through the same chain
    kc.add(b)
    b.close()
    for c in canonical[:5]:
        table[c] += 1
    assert as_dict(kc) == table
    kc.close()


def full_table(eng):  # noqa: F811
    codes = g.distinct_codes(600, 21) + g.distinct_codes(424, 22, canonical=False)
    table = {c: 1 + i % 7 for i, c in enumerate(codes)}
    kc = eng.kmer_counter(21, max_kmers=512)
    kc_set(eng, kc, table)
    return kc, table, codes[:600]


def test_full_table(eng):  # noqa: F811
    kc, table, canonical = full_table(eng)
    assert kc.distinct() == g.SLOTS0 and as_dict(kc) == table
    extra = g.distinct_codes(40, 23, exclude=table)
    assert lookups(eng, kc, canonical[::6]) == [table[c] for c in canonical[::6]]
    assert lookups(eng, kc, extra) == [1] * 40                 # every slot is looked at once, then the loop ends
    one = np.array(extra[:1], dtype=np.uint64), np.array([9], dtype=np.int32)
    kc.merge(*one, only_present=True)                          # absent: passed over
    kc.merge(np.array(canonical[:2], dtype=np.uint64), np.array([10, 20], dtype=np.int32), only_present=True)
    table[canonical[0]] += 10
    table[canonical[1]] += 20
    assert as_dict(kc) == table
    refused(lambda: kc_set(eng, kc, {extra[0]: 9}), T4_ERR_UNSUPPORTED, "more distinct k-mers")
    assert as_dict(kc) == table
    kc.close()
    kc, table, _ = full_table(eng)
    b = eng.upload([g.spell(extra[1], 21)])
    refused(lambda: kc.add(b), T4_ERR_UNSUPPORTED, "more distinct k-mers")
    assert as_dict(kc) == table
    b.close()
    kc.close()
    kc, table, _ = full_table(eng)                             # merge moves the ceiling (see the module's docstring): taken, and all stay
    kc.merge(*one)
    table[extra[0]] = 9
    assert as_dict(kc) == table and len(table) == g.SLOTS0 + 1
    kc.close()


def check_slots(eng, kc, table, slots, seed):  # noqa: F811
    """the table has `slots` slots: set() takes slots - used new codes and no more"""
    fresh = g.distinct_codes(slots - len(table) + 1, seed, exclude=table)
    more = {c: 3 + i % 5 for i, c in enumerate(fresh[:-1])}
    if more:
        kc_set(eng, kc, more)
    table = {**table, **more}
    assert kc.distinct() == slots and as_dict(kc) == table
    refused(lambda: kc_set(eng, kc, {fresh[-1]: 1}), T4_ERR_UNSUPPORTED, "more distinct k-mers", "(%d slots)" % slots)


# (used + incoming, the slots the table must have afterwards): one below and one above (used + incoming) * 10 == slots * 6 for tables
# of 1 024, 4 096 and 8 192 slots -- reached in steps of four: 1 024 -> 4 096, 1 024 -> 4 096 -> 8 192, 1 024 -> 4 096 -> 16 384
@pytest.mark.parametrize("total,slots", [(614, 1024), (615, 2048), (2457, 4096), (2458, 8192), (4915, 8192), (4916, 16384)])
def test_reserve_thresholds(eng, total, slots):  # noqa: F811
    assert total * 10 <= slots * 6 and total * 10 > (slots // 2) * 6
    codes = g.distinct_codes(200, 31) + g.distinct_codes(100, 32, canonical=False)
    table = {c: 1 + i % 9 for i, c in enumerate(codes)}
    kc = eng.kmer_counter(21, max_kmers=1)
    kc_set(eng, kc, table)
    kc.reserve(total - len(table))
    assert as_dict(kc) == table
    check_slots(eng, kc, table, slots, 33)
    kc.close()


def test_growth_keeps_every_pair(eng):  # noqa: F811
    """set, reserve, add, set, reserve ...: after every step the table is the dict, through 1 024 -> 2 048 -> 8 192 slots, with counts
    above 1 and codes that are not canonical in it"""
    kc = eng.kmer_counter(21, max_kmers=1)
    table = {c: 1 + i % 9 for i, c in enumerate(g.distinct_codes(300, 41) + g.distinct_codes(200, 42, canonical=False))}
    kc_set(eng, kc, table)
    reads, _ = g.short_read_batch(300, seed=43)
    for step, total in enumerate((1200, 4000)):
        kc.reserve(total - len(table))
        assert as_dict(kc) == table
        part = reads[step * 100:step * 100 + 100] * 2
        b = eng.upload(part)
        kc.add(b)
        b.close()
        for key, n in g.count_reads(part, 21).items():
            table[key] = table.get(key, 0) + n
        assert as_dict(kc) == table and len(table) < total
        fresh = g.distinct_codes(total - len(table), 44 + step, exclude=table)
        kc_set(eng, kc, {c: 5 for c in fresh})
        table.update({c: 5 for c in fresh})
        assert as_dict(kc) == table and len(table) == total
    check_slots(eng, kc, table, 8192, 46)
    kc.close()


def test_export_with_too_little_room(eng):  # noqa: F811
    table = {c: 1 + i for i, c in enumerate(g.distinct_codes(300, 51))}
    kc = eng.kmer_counter(21, max_kmers=512)
    kc_set(eng, kc, table)
    for cap in (1, len(table) - 1):
        codes, vals = np.full(len(table) + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(len(table) + 8, -77, dtype=np.int32)
        n = C.c_int64(-1)
        eng.check(eng.lib.t4_kmer_count_export(kc.h, codes.ctypes.data_as(V), vals.ctypes.data_as(V), C.c_int64(cap), C.byref(n)))
        assert n.value == len(table)
        got = list(zip(codes[:cap].tolist(), vals[:cap].tolist()))
        assert len({c for c, _ in got}) == cap and all(table.get(c) == v for c, v in got)
        assert (codes[cap:] == 0xA5A5A5A5A5A5A5A5).all() and (vals[cap:] == -77).all()
    kc.close()


def test_keys(eng):  # noqa: F811
    # k = 31: a canonical code with bit 61 set; all-A (code 0, stored as key 1) and all-T, the same k-mer
    top = g.top_bit_kmer(31, 61)
    reads = [top, g.rc(top), "A" * 31, "T" * 31, "A" * 40, top[:30] + "N"]
    kc = eng.kmer_counter(31, max_kmers=256)
    b = eng.upload(reads)
    kc.add(b)
    table = g.count_reads(reads, 31)
    assert table == {g.canon(top): 2, 0: 12} and g.canon(top) >> 61 == 1
    assert as_dict(kc) == table
    check_stats(kc.stats(b), [oracle_for(reads, 31).stats(r)[1:4] + (len(r),) for r in reads], lambda i: reads[i])
    b.close()
    kc.close()
    # even k: reverse palindromes are counted once per occurrence
    reads = ["AACGCGTT" * 3, "AACGCGTTAACGCGTT", "ACGT" * 5, g.rc("AACGCGTT" * 3)]
    kc = eng.kmer_counter(8, max_kmers=256)
    b = eng.upload(reads)
    kc.add(b)
    table = g.count_reads(reads, 8)
    assert table[g.code("AACGCGTT")] == 8 and g.canon("AACGCGTT") == g.code("AACGCGTT") == g.code(g.rc("AACGCGTT"))
    assert as_dict(kc) == table
    check_stats(kc.stats(b), [oracle_for(reads, 8).stats(r)[1:4] + (len(r),) for r in reads], lambda i: reads[i])
    b.close()
    kc.close()
    # a read and its reverse complement: the counts double, no k-mer is new
    read = g.top_bit_kmer(21, 62) + g.spell(g.distinct_codes(1, 63)[0], 21) * 2
    kc = eng.kmer_counter(21, max_kmers=256)
    b1, b2 = eng.upload([read]), eng.upload([g.rc(read)])
    kc.add(b1)
    once = as_dict(kc)
    kc.add(b2)
    assert once == g.count_reads([read], 21) and as_dict(kc) == {c: 2 * n for c, n in once.items()}
    b1.close()
    b2.close()
    kc.close()
    # a homopolymer of 384 bases: 364 positions, every lane of the wavefront on the one slot at once
    kc = eng.kmer_counter(21, max_kmers=256)
    b = eng.upload(["A" * 384, "T" * 384, "C" * 383])
    kc.add(b)
    assert as_dict(kc) == {0: 728, g.code("C" * 21): 363}
    mn, md, av, ln = kc.stats(b)
    assert mn.tolist() == md.tolist() == av.tolist() == [728, 728, 363]
    b.close()
    kc.close()


@pytest.mark.parametrize("k", (9, 21, 31))
def test_n_placement_in_add(eng, k):  # noqa: F811
    rnd = np.random.RandomState(k)
    seq = lambda n: "".join("ACGT"[x] for x in rnd.randint(0, 4, n))
    start, end = seq(k) + "N" + seq(k - 1), seq(k - 1) + "N" + seq(k)
    none = "".join("N" if p % k == k - 1 else c for p, c in enumerate(seq(4 * k)))
    reads = [start, end, none, "N" + seq(k - 1), seq(k - 1) + "N"]
    table = g.count_reads(reads, k)
    assert table == {g.canon(start[:k]): 1, g.canon(end[k:]): 1} and len(table) == 2
    kc = eng.kmer_counter(k, max_kmers=256)
    b = eng.upload(reads)
    kc.add(b)
    assert as_dict(kc) == table
    o = oracle_for(reads, k)
    check_stats(kc.stats(b), [o.stats(r)[1:4] + (len(r),) for r in reads], lambda i: reads[i])
    b.close()
    kc.close()


def test_more_reads_than_workgroups(eng):  # noqa: F811
    """10 000 reads of 21..30 bases, reads shorter than k among them, for a launch of 32 workgroups a compute unit (8 192 on the 256
    compute units of an MI355X): a workgroup meets a short read and then a normal one in its stride loop. Into a counter of 1 024
    slots that reserve() grew: t4_kmer_count_add takes the batch in one slice of more than 4 096 reads."""
    k = 21
    reads, short = g.short_read_batch(10000)
    assert len(reads) > eng.cus() * 32 and len(reads) > 8192 and len(short) > 100
    table = g.count_reads(reads, k)
    kc = eng.kmer_counter(k, max_kmers=1)
    kc.reserve(sum(max(0, len(r) - k + 1) for r in reads))
    b = eng.upload(reads)
    kc.add(b)
    assert as_dict(kc) == table and max(table.values()) > 10
    got = kc.stats(b)
    sample = sorted({0, len(reads) - 1} | {j for i in short for j in (i - 1, i, i + 1)} | set(range(7, len(reads), 41)))
    assert len(sample) >= 500
    o = oracle_for(reads, k)
    want = [o.stats(reads[i])[1:4] + (len(reads[i]),) for i in sample]
    check_stats(tuple(x[sample] for x in got), want, lambda j: (sample[j], reads[sample[j]]))
    b.close()
    kc.close()


# ---- 3. per-barcode keys ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (21, 9))
def test_barcodes_keep_apart(eng, k):  # noqa: F811
    top = g.top_bit_kmer(k, 70 + k)
    assert g.canon(top) >> (2 * k - 1) == 1 and (k != 21 or g.canon(top) >> 41 == 1)   # k = 21: next to the barcode's lowest bit
    read = top + g.spell(g.distinct_codes(1, 71, k=k)[0], k) + top[::-1]
    n = len(set(g.valid_kmers(read, k)))
    bcs = [-1, 0, 1, g.MAX_BARCODE, 0, g.MAX_BARCODE, g.MAX_BARCODE, 1, 1, 1, 1]
    reads = [read] * len(bcs)
    table = g.count_reads(reads, k, bcs)
    assert len(table) == 4 * n and {key >> g.BARCODE_SHIFT for key in table} == {0, 1, 2, g.MAX_BARCODE + 1} and max(table) >> 63 == 1
    kc = eng.kmer_counter(k, max_kmers=512, per_barcode=True)
    b = eng.upload(reads, bcs)
    kc.add(b)
    assert kc.distinct() == 4 * n and as_dict(kc) == table
    per = {bc: oracle_for([read] * bcs.count(bc), k) for bc in set(bcs)}
    want = [per[bc].stats(read)[1:4] + (len(read),) for bc in bcs]
    assert {w[0] for w in want} == {1, 2, 3, 5}
    check_stats(kc.stats(b), want, lambda i: bcs[i])
    check_stats(kc.stats_resident(b, False), want, lambda i: bcs[i])
    b.close()
    kc.close()


def test_barcodes_beyond_the_key_are_refused(eng):  # noqa: F811
    """barcode + 1 has 22 bits of the key: 4 194 303 would read as `no barcode`, b + 2^22 as b. Such a batch is refused, not counted."""
    read = "".join("ACGT"[x] for x in np.random.RandomState(9).randint(0, 4, 40))
    kc = eng.kmer_counter(21, max_kmers=512, per_barcode=True)
    for bcs, bad in (([0, 4194304], "4194304"), ([-1, 4194303], "4194303"), ([-2, 0], "-2")):
        b = eng.upload([read, read], bcs)
        for call in (lambda: kc.add(b), lambda: kc.stats(b), lambda: kc.stats_resident(b, False)):
            refused(call, T4_ERR_UNSUPPORTED, "barcode " + bad, str(g.MAX_BARCODE))
        b.close()
    assert kc.distinct() == 0
    for bcs in ([0, 1], [0, g.MAX_BARCODE], [-1, g.MAX_BARCODE]):
        kc = eng.kmer_counter(21, max_kmers=512, per_barcode=True)
        b = eng.upload([read, read], bcs)
        kc.add(b)
        for got in (kc.stats(b), kc.stats_resident(b, False)):
            assert got[0].tolist() == [1, 1] and got[1].tolist() == [1, 1] and got[2].tolist() == [1.0, 1.0]
        assert kc.distinct() == 40 and as_dict(kc) == g.count_reads([read, read], 21, bcs)
        b.close()
        kc.close()
