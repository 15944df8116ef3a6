"""Device and pinned memory of the text front end (t4_text_create / scan / batch / records / destroy, t4_candidate_test) on its error
paths, in the manner of test_handle_buffers.py (emulator build): every device and every pinned allocation of every step fails in
turn, the step returns T4_ERR_HIP with a message, the repeated step and the steps after it give the bytes of the undisturbed run,
and nothing is left live once everything is destroyed."""
from test_fastq_text import fastq
from test_handle_buffers import check_case, emu  # noqa: F401 (the fixture)
from test_oneshot_buffers import CONTIG, K, READS

SEQS = [READS[0], "A" * 30, CONTIG[3:40], "", READS[1], "ACGTN" * 9]
MATES = [CONTIG[10:33], READS[1], "T" * 25, "ACGT", "N" * 12, CONTIG[20:58]]


def case_text(eng, keep):
    def setup():
        ix = eng.index(K)
        keep.append(ix)
        ix.add_contig("c0", CONTIG)
        ix.set_params(K, 10, 0.9).commit()

    def all_or_none(makers):   # a step that failed half way leaves none of its handles behind: the step is repeated whole
        made = []
        try:
            for m in makers:
                made.append(m())
        except Exception:
            for o in made:
                o.close()
            raise
        keep.extend(made)

    def create():
        all_or_none([lambda: eng.text(4096), lambda: eng.text(4096)])

    def scan():
        return keep[1].scan(fastq(SEQS) + b"@partial\nAC", final=False), keep[2].scan(fastq(MATES)[:-1], final=True)

    def batch():
        # the whole piece; of the mates' also a part, with rows of its own width
        all_or_none([keep[1].batch, keep[2].batch, lambda: keep[2].batch(1, 3)])
        return [tuple(a.tobytes() if hasattr(a, "tobytes") else a for a in b.read()) for b in keep[3:6]]

    def records():
        return [tuple(a.tobytes() for a in t.records()) for t in keep[1:3]] + [keep[1].records(2, 3)[0].tobytes()]

    def candidate():
        ix = keep[0]
        out = (ix.candidate_test(keep[3], keep[4]).tobytes(), ix.candidate_test(keep[3]).tobytes())
        assert 0 < sum(out[0]) < len(SEQS)
        return out
    return [(setup, False), (create, True), (scan, True), (batch, True), (records, True), (candidate, True)]


def test_text_front_end(emu):  # noqa: F811
    made = check_case(emu, {}, case_text)
    # create: per handle the text, tile counts, line table, three per-record arrays, the info words; staging and the info words' twin.
    # batch: four arrays per batch. candidate test: query lengths and the two keep arrays, the per-call pools of the first query
    assert made["device"] >= 2 * 7 + 3 * 4 + 3 and made["pinned"] == 2 * 2
