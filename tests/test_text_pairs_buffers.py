"""Device and pinned memory of t4_text_process_pairs on its error paths, in the manner of test_text_buffers.py (emulator build):
every device and every pinned allocation of create -> scan x 2 -> process_pairs -> destroy fails in turn, the step returns
T4_ERR_HIP with a message, the repeated step and the steps after it give the bytes of the undisturbed run, and nothing is left live
once everything is destroyed."""
from test_engine_emu import pair_cases
from test_fastq_text import fastq
from test_handle_buffers import check_case, emu  # noqa: F401 (the fixture)

R1, Q1, R2, Q2 = pair_cases(5, 24)


def case_text_pairs(eng, keep):
    def setup():
        pass

    def create():
        made = []
        try:
            for _ in range(2):
                made.append(eng.text(1 << 14))
        except Exception:
            for o in made:
                o.close()
            raise
        keep.extend(made)

    def scan():
        return keep[0].scan(fastq(R1, quals=Q1)), keep[1].scan(fastq(["ACGT"] + R2, quals=["FFFF"] + Q2)[:-1])

    def pairs():
        out = keep[0].process_pairs(keep[1], first_mate=1)
        assert {0, 1, 2} <= {o[0] for o in out}
        return out

    def pairs_again():
        # the buffers are there now: a part of the piece, with skip bytes, and once more with room for nothing
        part = keep[0].process_pairs(keep[1], first=2, first_mate=3, n=20, skip=[i % 3 == 0 for i in range(20)])
        try:
            keep[0].process_pairs_raw(keep[1], first_mate=1, out_cap=0)
            need = None
        except Exception as e:
            need = e.out_bytes
        return part, need
    return [(setup, False), (create, True), (scan, True), (pairs, True), (pairs_again, True)]


def test_text_process_pairs(emu):  # noqa: F811
    made = check_case(emu, {}, case_text_pairs)
    # create: seven device arrays and two pinned blocks per handle (test_text_buffers.py). The first process_pairs call: meta words,
    # skip bytes, the need word, the two output buffers; the need word's pinned twin. Later calls make nothing.
    assert made["device"] == 2 * 7 + 5 and made["pinned"] == 2 * 2 + 1
