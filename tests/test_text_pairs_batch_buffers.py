"""Device and pinned memory of t4_text_pairs_batch, t4_kmer_count_reserve and t4_kmer_count_stats_resident on their error paths, in
the manner of test_text_pairs_buffers.py (emulator build): every device and every pinned allocation of create -> scan x 2 ->
process_pairs -> pairs_batch -> reserve -> add -> stats_resident -> destroy fails in turn, the step returns T4_ERR_HIP with a
message, the repeated step and the steps after it give the bytes of the undisturbed run, and nothing is left live once everything
is destroyed."""
from test_engine_emu import pair_cases
from test_fastq_text import fastq
from test_handle_buffers import check_case, emu  # noqa: F401 (the fixture)

R1, Q1, R2, Q2 = pair_cases(5, 24)


def case_pairs_batch(eng, keep):
    def setup():
        pass

    def create():
        made = []
        try:
            for _ in range(2):
                made.append(eng.text(1 << 14))
            made.append(eng.kmer_counter(21, max_kmers=1))
        except Exception:
            for o in made:
                o.close()
            raise
        keep.extend(made)

    def scan():
        return keep[0].scan(fastq(R1, quals=Q1)), keep[1].scan(fastq(["ACGT"] + R2, quals=["FFFF"] + Q2)[:-1])

    def pairs():
        return keep[0].process_pairs(keep[1], first_mate=1)

    def as_bytes(b):
        return tuple(x.tobytes() for x in b.read()[:4]) + tuple(x.tobytes() for x in b.quals())

    def batch():
        b, info = keep[0].pairs_batch(keep[1], first_mate=1)
        keep.append(b)
        assert info[0] > 24 and info[3] == 0
        return info, as_bytes(b)

    def batch_again():
        # the scratch is there now: only the batch's own arrays are made (here without qualities, and for no pair at all)
        b, info = keep[0].pairs_batch(keep[1], first_mate=1, with_quals=False)
        try:
            out = info, tuple(x.tobytes() for x in b.read()[:4]), b.quals()
        finally:
            b.close()
        return out

    def reserve():
        keep[2].reserve(24 * 2 * 150)
        return keep[2].distinct()

    def add():
        keep[2].add(keep[3])
        return sorted(zip(*[x.tolist() for x in keep[2].export()]))

    def stats():
        return tuple(x.tobytes() for x in keep[2].stats_resident(keep[3], True)) + tuple(x.tobytes() for x in keep[2].stats_resident(keep[3], False))
    return [(setup, False), (create, True), (scan, True), (pairs, True), (batch, True), (batch_again, True), (reserve, True), (add, False), (stats, True)]


def test_text_pairs_batch(emu):  # noqa: F811
    made = check_case(emu, {}, case_pairs_batch)
    # create: seven device arrays and two pinned blocks per text handle, four device arrays of the counter; the first process_pairs
    # call: five device arrays and a pinned word (test_text_pairs_buffers.py). The first pairs_batch call: the rows ahead of every pair,
    # the workgroups' sums, the info words and their pinned twin; the batch's pk, nm, len, low, qualities and offsets. The second one:
    # pk, nm, len, low. reserve: from 1 024 slots to 4 096 and to 16 384 (7 200 k-mers at a load of 0.6 need 12 000 slots), keys and counts
    # each time. stats_resident: four result arrays, twice. (export, in a step that is not under test, makes its own.)
    assert made["device"] == (2 * 7 + 4) + 5 + (3 + 6) + 4 + 2 * 2 + 2 * 4 and made["pinned"] == 2 * 2 + 1 + 1
