"""Device memory of the one-shot entry points on their error paths (emulator build: the emulator counts hipMalloc / hipFree and can
make one chosen hipMalloc fail). For every entry point and every allocation k of the call -- the pool growths of a fresh context
included -- the call with allocation k failing returns T4_ERR_HIP with a message, the same call repeated at once on the same context
gives what the undisturbed run gave, and after the teardown as many blocks are live as after the undisturbed run's."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import t4check

T4_ERR_HIP = -2
K = 9
CONTIG = "ACGGTCATTGCAGGATCCGTTAACGGCTAAGTCCGATTGCAAGCTTGGACCATGCATTGCC"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
READS = [CONTIG[5:25], "".join(COMP[x] for x in reversed(CONTIG[30:52]))]
QUALS = ["I" * 12 + "#" * 8, "I" * 22]
V = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(V)


@pytest.fixture(scope="module")
def emu():
    """the emulated library with its allocation hooks; and trust4_amd bound to it"""
    path = t4check.build_emulator_lib()
    os.environ["T4_LIB"] = path
    lib = C.CDLL(path)
    lib.hipemu_live_blocks.restype = C.c_longlong
    lib.hipemu_malloc_calls.restype = C.c_longlong
    lib.hipemu_fail_malloc.argtypes = [C.c_longlong]
    gc.collect()   # contexts that earlier modules left to the collector go now, not between two counts
    yield lib
    lib.hipemu_fail_malloc(0)
    os.environ.pop("T4_LIB", None)


def contig_set(eng, keep):
    ix = eng.index(K)
    keep.append(ix)
    ix.add_contig("c0", CONTIG)
    ix.set_params(K, 10, 0.9).commit()
    b = eng.upload(READS)
    keep.append(b)
    return ix, b


@pytest.fixture(scope="module")
def tail_inputs(emu):
    """inputs of t4_extend and t4_consensus_recompute, from a context of their own: the contexts under test stay fresh"""
    import trust4_amd
    eng, keep = trust4_amd.Engine(0), []
    ix, b = contig_set(eng, keep)
    cnt, ov = ix.overlaps(b, 0, 0, 4)
    ret, asg = ix.assign_strands(b, [0, 0])
    assert (cnt > 0).all() and (ret == 0).all()
    for o in reversed(keep):
        o.close()
    eng.close()
    return cnt, ov, asg


# Every case: set-up on the fresh context `eng` (what it creates goes into `keep`), then -> (call, observe). call() is the entry
# point under test, once; it returns the call's outputs or None. observe(), when there is one, reads the state the call left.
def case_hits(eng, keep, tail):
    ix, b = contig_set(eng, keep)

    def call():
        off, hits = np.zeros(len(READS) + 1, np.int64), np.zeros(256, np.dtype("<i4, <i4, <i4, <i4, <i4"))
        eng.check(eng.lib.t4_hits(ix.h, b.h, 0, 0, ptr(off), ptr(hits), len(hits)))
        assert off[-1] > 0
        return off.tobytes(), hits[:off[-1]].tobytes()
    return call, None


def case_gap_dp_chars(eng, keep, tail):
    return (lambda: eng.gap_dp(0, [CONTIG[:20], CONTIG[20:41]], [CONTIG[:9] + CONTIG[10:20], CONTIG[20:41]], 0).tobytes()), None


def case_gap_dp_posweight_align(eng, keep, tail):
    onehot = lambda s: np.eye(4, dtype=np.int32)[["ACGT".index(x) for x in s]]

    def call():
        out, strings = eng.gap_dp(1, [onehot(CONTIG[:20]), onehot(CONTIG[20:41])], [CONTIG[:9] + CONTIG[10:20], CONTIG[20:41]], 4)
        assert all(s is not None for s in strings)
        return out.tobytes(), strings
    return call, None


def case_mate_overlap(eng, keep, tail):
    return (lambda: eng.mate_overlap([CONTIG[:24], CONTIG[30:50]], [CONTIG[10:34], CONTIG[5:25]], [10, 10], True).tobytes()), None


def case_process_pairs(eng, keep, tail):
    r2 = ["".join(COMP[x] for x in reversed(CONTIG[12:34])), READS[1]]
    return (lambda: eng.process_pairs([CONTIG[:24], READS[0]], ["I" * 24, QUALS[0]], r2, ["I" * 22, QUALS[1]])), None


def kmer_counter(eng, keep):
    kc = eng.kmer_counter(K, max_kmers=64)
    keep.append(kc)
    b = eng.upload(READS)
    keep.append(b)
    kc.add(b)
    return kc, b


def sorted_pairs(kc):
    codes, vals = kc.export()
    o = np.argsort(codes)
    return codes[o].tobytes(), vals[o].tobytes()


def case_kmer_count_set(eng, keep, tail):
    kc, _ = kmer_counter(eng, keep)
    codes, counts = np.array([5, 77, 5], np.uint64), np.array([3, 4, 9], np.int32)
    return (lambda: eng.check(eng.lib.t4_kmer_count_set(kc.h, ptr(codes), ptr(counts), C.c_int64(3)))), (lambda: sorted_pairs(kc))


def case_kmer_count_export(eng, keep, tail):
    kc, _ = kmer_counter(eng, keep)
    return (lambda: sorted_pairs(kc)), None


def case_kmer_count_merge(eng, keep, tail):
    kc, _ = kmer_counter(eng, keep)
    held = np.sort(kc.export()[0])[:3]   # (the table hands its pairs out in any order)
    codes, vals = np.concatenate([held, np.array([1, 2], np.uint64)]), np.array([5, 6, 7, 8, 9], np.int32)
    return (lambda: kc.merge(codes, vals, only_present=False) and None), (lambda: sorted_pairs(kc))


def case_kmer_count_stats(eng, keep, tail):
    kc, b = kmer_counter(eng, keep)
    return (lambda: tuple(a.tobytes() for a in kc.stats(b, QUALS))), None


def case_assign_strands(eng, keep, tail):
    ix, b = contig_set(eng, keep)
    return (lambda: tuple(a.tobytes() for a in ix.assign_strands(b, [1, -1]))), None


def case_consensus_recompute(eng, keep, tail):
    ix, b = contig_set(eng, keep)

    def call():
        pw, cons, changed = ix.consensus_recompute(b, tail[2], len(CONTIG), mult=[2, 3])
        return pw.tobytes(), cons, changed
    return call, None


def case_extend(eng, keep, tail):
    ix, b = contig_set(eng, keep)
    return (lambda: tuple(a.tobytes() for a in ix.extend(b, tail[0], tail[1], 1.0))), None


def case_reads_upload_flags(eng, keep, tail):
    bases, offs, bcs = np.frombuffer("".join(READS).encode(), np.uint8), np.array([0, 20, 42], np.int64), np.array([3, 4], np.int32)
    made = []

    def call():
        h = V(1)
        rc = eng.lib.t4_reads_upload_flags(eng.h, ptr(bases), ptr(offs), ptr(bcs), 2, 0, C.byref(h))
        assert (rc == 0) == bool(h.value)   # no batch comes out of a failed call
        eng.check(rc)
        made.append(h)

    class Made:
        def close(self):
            for h in made:
                eng.lib.t4_batch_destroy(h)
    keep.append(Made())
    return call, (lambda: int(eng.lib.t4_batch_size(made[-1])))


# the hipMalloc calls of the call on a fresh context: its own buffers, and the pools it makes grow
CASES = [(case_hits, 6), (case_gap_dp_chars, 7), (case_gap_dp_posweight_align, 8), (case_mate_overlap, 6), (case_process_pairs, 11),
         (case_kmer_count_set, 2), (case_kmer_count_export, 3), (case_kmer_count_merge, 2), (case_kmer_count_stats, 6),
         (case_assign_strands, 7), (case_consensus_recompute, 5), (case_extend, 9), (case_reads_upload_flags, 4)]


def run(emu, case, tail, fail_at):
    """t4_init, set-up, the call (its fail_at-th hipMalloc failing, then once more undisturbed), destroy everything
    -> (outputs, hipMalloc calls of the first call, live blocks at the end)"""
    import trust4_amd
    eng, keep = trust4_amd.Engine(0), []
    try:
        call, observe = case(eng, keep, tail)
        before = emu.hipemu_malloc_calls()
        emu.hipemu_fail_malloc(fail_at)
        try:
            out, err = call(), None
        except trust4_amd.api.T4Error as e:
            out, err = None, e
        finally:
            emu.hipemu_fail_malloc(0)
        mallocs = emu.hipemu_malloc_calls() - before
        if fail_at:
            assert err is not None and err.code == T4_ERR_HIP, (fail_at, err)
            assert eng.lib.t4_last_error(eng.h), fail_at
            out = call()
        elif err is not None:
            raise err
        if observe:
            out = observe()
    finally:
        for o in reversed(keep):
            o.close()
        eng.close()
    return out, mallocs, emu.hipemu_live_blocks()


@pytest.mark.parametrize("case,allocs", CASES, ids=[c.__name__[5:] for c, _ in CASES])
def test_failed_allocation_frees_and_recovers(emu, tail_inputs, case, allocs):
    expect, m, live0 = run(emu, case, tail_inputs, 0)
    assert m == allocs
    bad, held = [], live0
    for k in range(1, m + 1):
        out, _, live = run(emu, case, tail_inputs, k)
        if out != expect:
            bad.append("allocation %d of %d: the repeated call gives another result" % (k, m))
        if live != held:
            bad.append("allocation %d of %d: %d device blocks left behind" % (k, m, live - held))
        held = live
    assert not bad and held == live0, bad
