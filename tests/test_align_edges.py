"""The alignment kernels at their band, length and tie-break edges (generators: align_gen.py).

Gap DP (t4_gap_dp, both aligners, every formulation): a grid of lengths that puts cases on both sides of every band edge
(16 / 17, 32 / 33, 64 / 65 columns), of the 320-base limit and of the direction-byte limit, crossed with content in which
alignment paths of equal score are the rule. The status word of every case is asserted against `align_gen.expected_status`, a
function of the lengths alone, and every case whose expected status is 0 is compared: no case is left out by looking at what the
engine returned.

ExtendOverlap (t4_extend, t4_add_query): caller-supplied overlaps whose anchors leave overhangs of chosen size and content on a
read of up to 384 bases: sizes on the 64-position steps of the ballot scan and on the chunking of the direction buffer, mismatches
on the exact tie of the 3/4 good-prefix rule and on the 2 / 3 edge of the rule that calls for the DP, insertions and deletions,
N, zero-sum and ambiguous columns, both strands, both mismatch factors.

Every comparison is with the oracle and, when it was built, with the compiled reference; equality is exact. The emulator runs a
thinned set (every length pair, every family; fewer repeats of the long cases), `-m gpu` the full one."""
import os
import time

import numpy as np
import pytest

import align_gen as A
import t4check
from t4libs import Oracle, Ref


def make_engine(emulated):
    if emulated:
        os.environ["T4_LIB"] = t4check.build_emulator_lib()
    else:
        os.environ.pop("T4_LIB", None)
    import trust4_amd
    return trust4_amd.Engine(0)


@pytest.fixture(params=[True, pytest.param(False, marks=pytest.mark.gpu)], ids=["emu", "gpu"])
def eng(request, monkeypatch):
    from test_query_edges import AIDS
    for a in AIDS:      # the real capacities and thresholds: no testing aid that moves one
        monkeypatch.delenv(a, raising=False)
    e = make_engine(request.param)
    e.emulated = request.param
    yield e
    e.close()
    os.environ.pop("T4_LIB", None)


def aligners():
    return [Oracle(9)] + ([Ref(9)] if Ref.available() else [])


def stats_of(al):
    return (al.count(0), al.count(1), al.count(2) + al.count(3))


def lens_of(T, P):
    return [(len(t), len(p)) for t, p in zip(T, P)]


def assert_edges_covered(kind, impl, lens, status):
    """at least one case on each side of the edge this formulation stops at, and of the 320 / 321 edge (cases that run a band: both
    sides of two bases or more, unequal lengths)"""
    real = [(lt, lp, s) for (lt, lp), s in zip(lens, status) if lt >= 2 and lp >= 2 and lt != lp]
    inside = [(lt, lp, s) for lt, lp, s in real if lt <= A.MAXGAP and lp <= A.MAXGAP]
    W = lambda lt, lp: A.band(lt, lp)
    for lo in (16, 32, 64):
        assert any(W(lt, lp) == lo for lt, lp, _ in inside) and any(W(lt, lp) == lo + 1 for lt, lp, _ in inside), (kind, impl, lo)
    edge = {3: 16, 2: 64}.get(impl)
    if edge:
        assert all(s == 0 for lt, lp, s in inside if W(lt, lp) == edge) and all(s == 2 for lt, lp, s in inside if W(lt, lp) == edge + 1)
    for side in (0, 1):
        assert any((lt, lp)[side] == 320 and s == 0 for lt, lp, s in real if max(lt, lp) == 320), (kind, impl, side)
        assert any((lt, lp)[side] == 321 and s != 0 for lt, lp, s in real), (kind, impl, side)
    if impl in (0, 1, 4):
        cells = lambda lt, lp: (lp + 1) * min(W(lt, lp), lt)
        assert any(s == 0 and 48000 < cells(lt, lp) <= A.DIR_BYTES for lt, lp, s in inside), (kind, impl)
        assert any(s == 1 and cells(lt, lp) > A.DIR_BYTES for lt, lp, s in inside), (kind, impl)
    assert any(W(lt, lp) > lt for lt, lp, _ in inside)      # band wider than the target: DW = lent


@pytest.mark.parametrize("kind", [0, 1])
def test_gap_dp_edges(eng, kind):
    t0 = time.time()
    T, P, tags = A.dp_cases(kind, thin=8 if eng.emulated else 1)
    n = len(P)
    lens = lens_of(T, P)
    truth = []
    for o in aligners():
        res = [o.global_alignment(t, p)[1] if kind == 0 else o.global_alignment_posweight(t, p)[1] for t, p in zip(T, P)]
        if truth:
            bad = [i for i in range(n) if res[i] != truth[i]]
            assert not bad, ("oracle and reference disagree", [tags[i] for i in bad[:5]])
        truth = res          # the reference's answer when it is there
    exp = [stats_of(al) for al in truth]
    for impl in (0, 1, 2, 3) + ((4,) if kind == 1 else ()):
        status = [A.expected_status(kind, impl, lt, lp) for lt, lp in lens]
        if impl == 4:
            got, strings = eng.gap_dp(kind, T, P, 4)
        else:
            got, strings = eng.gap_dp(kind, T, P, impl), None
        bad = [i for i in range(n) if int(got[i, 3]) != status[i]]
        assert not bad, ("status", kind, impl, [(tags[i], lens[i], status[i], got[i].tolist()) for i in bad[:5]])
        cmp_ = [i for i in range(n) if status[i] == 0]
        bad = [i for i in cmp_ if tuple(got[i, :3].tolist()) != exp[i]]
        assert not bad, ("counts", kind, impl, len(bad), [(tags[i], exp[i], got[i].tolist()) for i in bad[:5]])
        if strings is not None:
            bad = [i for i in cmp_ if strings[i] != truth[i]]
            assert not bad, ("edit strings", len(bad), [(tags[i], truth[i], strings[i]) for i in bad[:3]])
        refused = n - len(cmp_)
        print("gap DP kind %d impl %d: %d compared, %d refused (status %s)" % (kind, impl, len(cmp_), refused, sorted(set(status) - {0})))
        assert len(cmp_) > 0 and refused > 0
        assert_edges_covered(kind, impl, lens, status)
    if kind == 0:    # the border quirk needs a traceback that reaches row 0 beyond column 4 * (lenp + 1)
        assert sum(1 for (lt, lp), al in zip(lens, truth) if lp >= 1 and lt > 4 * (lp + 1) and A.band(lt, lp) <= 64) > 50
    # ties are the rule in these families: many alignments with indels next to matches
    assert sum(1 for e in exp if e[2] > 0 and e[0] > 0) > n // 4
    print("gap DP kind %d: %d cases, %.1f s" % (kind, n, time.time() - t0))


# ---- ExtendOverlap on placed overhangs -------------------------------------------------------------------------------------------
def side_facts(es, case):
    """per side of a case: (size, mismatches of the ungapped alignment, needs the DP)"""
    ci, rs, re_, ss, se = case["ov"][:5]
    w = es.contigs[ci][2]
    rd = case["aligned"]
    out = []
    for side, size in enumerate(case["sizes"]):
        t0, p0 = (ss - size, rs - size) if side == 0 else (se + 1, re_ + 1)
        mm = sum(0 if A.base_equal(w[t0 + i], rd[p0 + i]) else 1 for i in range(size))
        out.append((size, mm, size > 1 and not ((size - mm) * 2 - mm * 2 >= size * 2 - 8)))
    return out


def run_extend(eng, ix, cases, chk, per_read=1):
    """t4_extend of every case (one overlap per read), both mismatch factors, against every checker -> expected (ret, out) at factor 1"""
    from trust4_amd.api import OV_DTYPE
    b = eng.upload([c["read"] for c in cases])
    ov = np.zeros((len(cases), per_read), dtype=OV_DTYPE)
    for i, c in enumerate(cases):
        ov[i, 0] = c["ov"]
    cnt = np.ones(len(cases), dtype=np.int32)
    first = None
    for factor in (1.0, 2.0):
        ret, ext = ix.extend(b, cnt, ov, factor)
        exp = None
        for o in chk:
            res = [o.extend_overlap(c["aligned"], factor, c["ov"]) for c in cases]
            assert exp is None or res == exp, "oracle and reference disagree"
            exp = res
        bad = [i for i in range(len(cases)) if (int(ret[i, 0]), tuple(ext[i, 0].tolist())) != (exp[i][0], tuple(exp[i][1]))]
        assert not bad, (factor, len(bad), [(cases[i]["planted"], cases[i]["ov"], exp[i], int(ret[i, 0]), ext[i, 0].tolist()) for i in bad[:4]])
        first = first or exp
    return first


def test_extend_placed_overhangs(eng):
    t0 = time.time()
    es = A.ExtendSet()
    ix = es.commit(eng)
    chk = [es.o] + ([es.ref()] if Ref.available() else [])
    cases = A.extend_cases(es, thin=6 if eng.emulated else 1)
    for c in cases:    # self-consistent coordinates inside read and contig
        ci, rs, re_, ss, se = c["ov"][:5]
        assert 0 <= rs <= re_ < len(c["read"]) <= A.READ_MAX and 0 <= ss <= se < len(es.contigs[ci][1]) and re_ - rs == se - ss
    exp = run_extend(eng, ix, cases, chk)
    # what the cases reached, per overhang-size class
    tally = {}
    for c, (ret, out) in zip(cases, exp):
        facts = side_facts(es, c)
        for side, (size, mm, dp) in enumerate(facts):
            t = tally.setdefault(A.size_class(size), {"sides": 0, "dp": 0, "indel": 0, "ret0": 0, "ret1": 0})
            t["sides"] += 1
            t["dp"] += dp
            # an alignment with an indel: the side's overhang is given up (ret 0 and the coordinates stop short of it)
            gave_up = ret == 0 and ((c["ov"][1] - out[1]) if side == 0 else (out[2] - c["ov"][2])) < size
            t["indel"] += bool(c["planted"][2] and c["planted"][2][0] == side and dp and gave_up)
            t["ret%d" % ret] += 1
    for k in ("0", "1-2", "3-64", "65-128", "129-170", "171-256", "257+"):
        print("t4_extend overhangs of %-8s %s" % (k, tally.get(k)))
    for k in ("3-64", "65-128", "129-170", "171-256", "257+"):
        assert all(tally[k][f] > 0 for f in ("dp", "indel", "ret0", "ret1")), (k, tally[k])
    for k in ("0", "1-2"):
        assert tally[k]["ret0"] > 0 and tally[k]["ret1"] > 0, (k, tally[k])
    # both sides of the DP rule (2 / 3 mismatches) and of both strands
    mms = {mm for c in cases for _, mm, _ in side_facts(es, c)}
    assert {0, 1, 2, 3, 4} <= mms and {c["ov"][5] for c in cases} == {1, -1}
    print("t4_extend: %d placed overlaps, %.1f s" % (len(cases), time.time() - t0))


def test_extend_many_long_sides_of_one_read(eng):
    """up to 128 overlaps of one read (t4_extend's limit), each with two long overhangs that need the DP: the direction buffer is
    carved into chunks, four sides at a time, and the read climbs the tiers for the room its overlaps need"""
    from trust4_amd.api import OV_DTYPE
    es = A.ExtendSet()
    ix = es.commit(eng)
    chk = [es.o] + ([es.ref()] if Ref.available() else [])
    counts = (128, 65, 64, 17) if not eng.emulated else (128, 17)
    reads, lists = [], []
    for i, n in enumerate(counts):
        rd, ovs = A.sliding_anchor_overlaps(es, i % 2, n, 40 + i)
        reads.append(rd)
        lists.append(ovs)
    b = eng.upload(reads)
    ov = np.zeros((len(reads), 128), dtype=OV_DTYPE)
    for i, ovs in enumerate(lists):
        for t, o in enumerate(ovs):
            ov[i, t] = o
    cnt = np.array(counts, dtype=np.int32)
    for factor in (1.0, 2.0):
        ret, ext = ix.extend(b, cnt, ov, factor)
        n0 = 0
        for i, ovs in enumerate(lists):
            for t, o_in in enumerate(ovs):
                for o in chk:
                    eret, eout = o.extend_overlap(reads[i], factor, o_in)
                    assert int(ret[i, t]) == eret and tuple(ext[i, t].tolist()) == tuple(eout), (i, t, o_in, eout, ext[i, t].tolist())
                n0 += eret == 0
        assert n0 > sum(counts) // 2     # the right overhang holds a deletion


def add_query_long_overhang_set(n_contigs, seed):
    """a 384-base read and n_contigs contigs that share one stretch of it, with flanks that follow the read's but for a substitution
    every eighth base (no shared 9-mer: the overlap stays the shared stretch) and, in every third contig, a missing base: every
    overlap GetOverlapsFromRead returns has long overhangs on both sides that need the DP"""
    import edge_gen as G
    es = G.EdgeSet(9, 31, seed)
    rd = es.new_read(A.READ_MAX)
    for i in range(n_contigs):
        lo = 150 + 4 * (i % 11)
        hi = lo + 60
        flank = list(rd)
        for pos in list(range(lo - 1 - (i % 5), -1, -8)) + list(range(hi + (i % 7), len(rd), 8)):
            flank[pos] = es.rnd.choice([c for c in "ACGT" if c != rd[pos]])
        if i % 3 == 0:
            del flank[30 + i]
        if i % 3 == 1:
            del flank[300 + i]
        es.add("".join(flank))
    return es, rd


def test_add_query_deferred_extension_of_long_overhangs(eng):
    """the same through t4_add_query: more than 16 overlaps on a 384-base read leave their extension to extendKernel, whose 8 KiB
    direction buffer takes sides of more than 170 bases one at a time"""
    from test_query_edges import check_add_query, deferred_reads, wide_reads
    es, rd = add_query_long_overhang_set(24, 61)
    ix = es.commit(eng)
    ret, lst = es.o.overlaps_from_read(rd)
    assert ret > 16
    long_sides = sum((o[1] > 170) + (len(rd) - 1 - o[2] > 170) for o in lst)
    assert long_sides >= 8 and all(o[1] > 100 and len(rd) - 1 - o[2] > 100 for o in lst)
    for strand, read in ((0, rd), (0, A.rc(rd)), (1, rd)):
        d0, w0 = deferred_reads(eng), wide_reads(eng)
        cnt = check_add_query(eng, ix, es, [read], [strand])
        assert cnt.tolist() == [ret] and (deferred_reads(eng) - d0, wide_reads(eng) - w0) == (1, 0)
