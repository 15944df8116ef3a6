"""`trust4-hip` under T4_GPU_PARSE=1 T4_TEXT_COUNTS=1: the 21-mers are counted piece by piece from the text the device holds
(t4_text_pairs_batch -> t4_kmer_count_reserve -> t4_kmer_count_add), and the count statistics and the quality trimming run on the
batches kept from that (t4_kmer_count_stats_resident): no base and no quality is uploaded a second time. Byte-identical to the
reference `trust4` (oracle/_ref/trust4) and to the run without the switch in bulk mode, barcode mode, under --cellShard, with
--trimLevel 0, gzip input and qualities with low tails; command lines and inputs the switch does not take run as without it, and
say so. Emulated (the test build of the driver) and, with -m gpu, the knob build of the product driver on the GPU."""
import gzip
import os
import random
import re
import shutil

import pytest

from test_stage1_e2e import REF_BIN, _kmer_count_file
from test_stage1_text_e2e import (ON, barcode_missing_case, bulk, exe, knob_driver, rewrite, run, same_files, synth_bulk,  # noqa: F401 (fixtures)
                                  tiny, took_device_path, took_host_path)

COUNTS = dict(ON, T4_TEXT_COUNTS="1")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/trust4 not built")
NEW = r"21-mers counted from the device's reads \(T4_TEXT_COUNTS=1\): (\d+) batches in [0-9.]+ s of the input loop, (\d+) kept for the statistics"
OLD = "T4_TEXT_COUNTS: the 21-mers are counted from the reads of the host's list as without the switch (%s)"


def took_new_path(log, kept=None, more_than_one_batch=True):
    """-> (batches, kept); kept None: every batch was kept for the statistics pass"""
    m = re.search(NEW, log)
    assert m and "T4_TEXT_COUNTS: the 21-mers are counted from the reads of the host's list" not in log, log[-1200:]
    batches, k = int(m.group(1)), int(m.group(2))
    assert batches > (1 if more_than_one_batch else 0) and k == (batches if kept is None else kept), m.group(0)
    assert "timing: 21-mers counted (on the device)" in log
    return batches, k


def took_todays_path(log, why):
    assert (OLD % why) in log and not re.search(NEW, log), log[-1200:]


def bulk_args(bulk, extra=()):  # noqa: F811
    return ["--skipMateExtension", "-f", bulk["fa"], "-1", bulk[1], "-2", bulk[2]] + list(extra)


# ---- the new path -------------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("piece", ["4096", None], ids=["pieces_4096", "default_piece"])
def test_bulk(tmp_path, exe, bulk, piece):  # noqa: F811
    import json
    sj = str(tmp_path / "stats.json")
    p = run(exe, bulk_args(bulk), str(tmp_path / "on"), dict(COUNTS, T4_STATS_JSON=sj, **({"T4_TEST_TEXT_PIECE": piece} if piece else {})), threads="4")
    took_device_path(p.stderr)
    batches, kept = took_new_path(p.stderr, more_than_one_batch=piece is not None)
    assert json.load(open(sj))["text_counts"] == {"on": 1, "batches": batches, "kept": kept}
    same_files(bulk["ref"], str(tmp_path / "on"))
    same_files(bulk["off"], str(tmp_path / "on"))


@needs_ref
def test_bulk_trim_level_0(tmp_path, exe, bulk):  # noqa: F811
    import subprocess
    args = bulk_args(bulk, ["--trimLevel", "0"])
    subprocess.run([REF_BIN, "-t", "1"] + args + ["-o", str(tmp_path / "ref")], check=True, stderr=subprocess.DEVNULL)
    run(exe, args, str(tmp_path / "off"), dict(ON, T4_TEST_TEXT_PIECE="4096"))
    p = run(exe, args, str(tmp_path / "on"), dict(COUNTS, T4_TEST_TEXT_PIECE="4096"))
    took_new_path(p.stderr)
    same_files(str(tmp_path / "ref"), str(tmp_path / "on"))
    same_files(str(tmp_path / "off"), str(tmp_path / "on"))


@needs_ref
def test_bulk_gzip(tmp_path, exe, bulk):  # noqa: F811
    for mate in (1, 2):
        with open(bulk[mate], "rb") as f, gzip.open(str(tmp_path / ("in_%d.fq.gz" % mate)), "wb") as g:
            shutil.copyfileobj(f, g)
    args = ["--skipMateExtension", "-f", bulk["fa"], "-1", str(tmp_path / "in_1.fq.gz"), "-2", str(tmp_path / "in_2.fq.gz")]
    p = run(exe, args, str(tmp_path / "on"), dict(COUNTS, T4_TEST_TEXT_PIECE="4096"))
    took_device_path(p.stderr)
    took_new_path(p.stderr)
    same_files(bulk["ref"], str(tmp_path / "on"))
    same_files(bulk["off"], str(tmp_path / "on"))


def low_tails(src, dst, seed):
    """the records of `src` with qualities whose tails are low, so that the trimming of the statistics pass cuts reads"""
    rnd = random.Random(seed)
    lines = open(src).read().split("\n")[:-1]
    with open(dst, "w") as f:
        for i in range(0, len(lines), 4):
            n = len(lines[i + 1])
            tail = min(n, rnd.choice([0, 0, 10, 25, 60]))
            q = "".join(rnd.choice("FI:") for _ in range(n - tail)) + "".join(rnd.choice("#+5") for _ in range(tail))
            f.write("%s\n%s\n+\n%s\n" % (lines[i], lines[i + 1], q))


def low_tails_case(tmp_path, driver, bulk, env, threads="2"):  # noqa: F811
    import subprocess
    f1, f2 = str(tmp_path / "q_1.fq"), str(tmp_path / "q_2.fq")
    low_tails(bulk[1], f1, 5)
    low_tails(bulk[2], f2, 6)
    args = ["--skipMateExtension", "-f", bulk["fa"], "-1", f1, "-2", f2]
    subprocess.run([REF_BIN, "-t", "1"] + args + ["-o", str(tmp_path / "ref")], check=True, stderr=subprocess.DEVNULL)
    run(driver, args, str(tmp_path / "off"), threads=threads)
    p = run(driver, args, str(tmp_path / "on"), env, threads=threads)
    took_new_path(p.stderr)
    same_files(str(tmp_path / "ref"), str(tmp_path / "on"))
    same_files(str(tmp_path / "off"), str(tmp_path / "on"))
    if "off" in bulk:   # (the run on the qualities as they were: the tails were cut)
        assert open(str(tmp_path / "on_assembled_reads.fa")).read() != open(bulk["off"] + "_assembled_reads.fa").read()
    return p.stderr


@needs_ref
def test_bulk_low_quality_tails(tmp_path, exe, bulk):  # noqa: F811
    low_tails_case(tmp_path, exe, bulk, dict(COUNTS, T4_TEST_TEXT_PIECE="4096"))


@needs_ref
def test_barcode_mode(tmp_path, exe):  # noqa: F811
    log = barcode_missing_case(tmp_path, exe, 160, 8, 6, dict(COUNTS, T4_TEST_TEXT_PIECE="8192"))   # (skip byte 1: pairs without a barcode)
    took_device_path(log)
    took_new_path(log)


@pytest.fixture(scope="module")
def cells(tmp_path_factory, exe):  # noqa: F811
    """160 pairs in 8 cells: the files of the reference binary and of the single-process run with T4_GPU_PARSE=1 alone"""
    import subprocess
    from t4libs import REF_FA, ROOT
    from test_stage1_e2e import _gunzip
    d = tmp_path_factory.mktemp("stage1_text_counts_cells")
    fa, pre = str(d / "ref.fa"), str(d / "c5")
    _gunzip(REF_FA, fa)
    subprocess.run([os.path.join(ROOT, "tools", "t4synth"), fa, "160", "0", "6", pre, "--cells", "8"], check=True)
    args = ["-f", fa, "-1", pre + "_1.fq", "-2", pre + "_2.fq", "--barcode", pre + "_bc.fa", "--UMI", pre + "_umi.fa"]
    subprocess.run([REF_BIN, "-t", "1"] + args + ["-o", str(d / "ref")], check=True, stderr=subprocess.DEVNULL)
    p = run(exe, args, str(d / "off"), dict(ON, T4_TEST_TEXT_PIECE="8192"))
    took_device_path(p.stderr)
    assert "T4_TEXT_COUNTS" not in p.stderr
    same_files(str(d / "ref"), str(d / "off"))
    assert open(str(d / "ref_raw.out")).read().count(">") >= 8
    return {"args": args, "ref": str(d / "ref"), "off": str(d / "off")}


@needs_ref
@pytest.mark.parametrize("dealt", ["dealt_out", "dealt_later"])
def test_two_ranks_cell_shard(tmp_path, exe, cells, dealt):  # noqa: F811
    """Two emulated ranks under --cellShard over --gatherDir with the switch set on both; their merged files against the reference
    binary's and against the single-process run without the switch. With the input dealt out by cells (skip byte 2) a rank's batches
    hold its own reads only and every one is kept; with T4_SHARD_INPUT=0 every rank counts the whole sample from the device's reads
    and lets go of the other ranks' reads afterwards, so no batch is kept and the statistics pass uploads."""
    import subprocess
    env = dict(os.environ, **COUNTS, T4_TEST_TEXT_PIECE="8192", HIPEMU_THREADS="2", T4_THREADS="2")
    if dealt == "dealt_later":
        env["T4_SHARD_INPUT"] = "0"
    gdir = tmp_path / "gather"
    gdir.mkdir()
    merged = str(tmp_path / "merged")
    procs = [subprocess.Popen([exe] + cells["args"] + ["-o", merged, "--cellShard", "%d/2" % r, "--gatherDir", str(gdir)], env=env, stderr=subprocess.PIPE, text=True)
             for r in range(2)]
    logs = [p.communicate(timeout=900)[1] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], logs
    assert "Gathered 2 shards over files" in logs[0]
    for log in logs:
        took_device_path(log)
        assert ("their pairs alone are processed and counted here" in log) == (dealt == "dealt_out"), log[-1200:]
        took_new_path(log, kept=None if dealt == "dealt_out" else 0)
    same_files(cells["ref"], merged)
    same_files(cells["off"], merged)


# ---- today's path, with the switch set ------------------------------------------------------------------------------------------------
def on_and_off(tmp_path, driver, args, env_extra=None, threads="2"):
    """the run with T4_GPU_PARSE=1 alone and the one with T4_TEXT_COUNTS=1 beside it -> the log of the latter; the files must be the same"""
    e = dict(env_extra or {})
    run(driver, args, str(tmp_path / "off"), dict(ON, T4_TEST_TEXT_PIECE="4096", **e), threads=threads)
    p = run(driver, args, str(tmp_path / "on"), dict(COUNTS, T4_TEST_TEXT_PIECE="4096", **e), threads=threads)
    same_files(str(tmp_path / "off"), str(tmp_path / "on"))
    assert open(str(tmp_path / "on_raw.out")).read().count(">") > 0
    return p.stderr


def reads_of(path):
    return open(path).read().split("\n")[1::4]


def test_count_file_keeps_todays_path(tmp_path, exe, tiny):  # noqa: F811
    fa, f1, f2 = tiny
    cfile = str(tmp_path / "counts.fa")
    _kmer_count_file(cfile, reads_of(f1) + reads_of(f2))
    log = on_and_off(tmp_path, exe, ["--skipMateExtension", "-f", fa, "-1", f1, "-2", f2, "-c", cfile])
    took_device_path(log, 0)
    took_todays_path(log, "a -c file")


def test_host_counts_keep_todays_path(tmp_path, exe, tiny):  # noqa: F811
    fa, f1, f2 = tiny
    log = on_and_off(tmp_path, exe, ["--skipMateExtension", "-f", fa, "-1", f1, "-2", f2], {"T4_GPU_KMERCOUNT": "0"})
    took_device_path(log, 0)
    took_todays_path(log, "T4_GPU_KMERCOUNT=0")
    assert "timing: 21-mers counted (on the device)" not in log


def test_other_letter_in_a_read_1(tmp_path, exe, tiny):  # noqa: F811
    fa, f1, f2 = tiny
    lines = open(f1).read().split("\n")
    # Record 20 (a later piece: counts had accumulated and were dropped) becomes a read of 30 bases with an R, and an N in every one of
    # its 21-mers: it stays through ProcessRead, has no valid k-mer, and the trimming empties it -- the stages behind the statistics,
    # which take ACGTN only, never see it, so the run ends well with and without the switch.
    rnd = random.Random(4)
    seq = "".join(rnd.choice("ACGT") for _ in range(30))
    lines[4 * 20 + 1] = seq[:3] + "R" + seq[4:14] + "N" + seq[15:]
    lines[4 * 20 + 3] = "F" * 30
    g1 = str(tmp_path / "r_1.fq")
    with open(g1, "w") as f:
        f.write("\n".join(lines))
    log = on_and_off(tmp_path, exe, ["--skipMateExtension", "-f", fa, "-1", g1, "-2", f2])
    took_device_path(log, 0)
    took_todays_path(log, "a letter other than ACGTN in a read 1")


def test_give_back(tmp_path, exe, bulk):  # noqa: F811
    g1, g2 = str(tmp_path / "blank_1.fq"), str(tmp_path / "blank_2.fq")
    rewrite(bulk[1], g1, "blank")   # (a blank line after record 100: pieces before it were counted)
    rewrite(bulk[2], g2, "blank")
    log = on_and_off(tmp_path, exe, ["--skipMateExtension", "-f", bulk["fa"], "-1", g1, "-2", g2])
    took_host_path(log, "the device path gave the input back")
    took_todays_path(log, "the input went through the host loop")


@needs_ref
def test_contig_min_cov_counts_on_the_device_statistics_uploaded(tmp_path, exe):  # noqa: F811
    """--contigMinCov 2: reads leave the list between the counts and the statistics, so no batch is kept"""
    log = barcode_missing_case(tmp_path, exe, 160, 8, 6, dict(COUNTS, T4_TEST_TEXT_PIECE="8192"), extra=["--contigMinCov", "2"])
    took_device_path(log)
    took_new_path(log, kept=0)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_exe():
    return knob_driver(False)


@pytest.mark.gpu
@needs_ref
def test_bulk_gpu(tmp_path, gpu_exe):
    fa, f1, f2 = synth_bulk(tmp_path, 3000, 100, 2)
    log = low_tails_case(tmp_path, gpu_exe, {"fa": fa, 1: f1, 2: f2}, dict(COUNTS, T4_TEST_TEXT_PIECE="262144"), threads="8")
    took_device_path(log, 300)


@pytest.mark.gpu
@needs_ref
def test_barcode_mode_gpu(tmp_path, gpu_exe):
    log = barcode_missing_case(tmp_path, gpu_exe, 3000, 60, 4, dict(COUNTS, T4_TEST_TEXT_PIECE="262144"))
    took_device_path(log, 300)
    took_new_path(log)
