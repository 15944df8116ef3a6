"""`trust4-hip` under T4_GPU_PARSE=1: the two mate files go to the device piece by piece as bytes, the device finds the records and
runs ProcessRead on them where they lie (t4_text_scan, t4_text_process_pairs), and the host builds the read records of the pairs
that are left out of the pieces (host/text_records.h). Byte-identical to the reference `trust4` (oracle/_ref/trust4) and to the run
without the switch, in bulk mode, barcode mode and under --cellShard; inputs the device path gives back and command lines it does
not take run through the host loop, identical to the run without the switch. Emulated (a test build of the driver with
-DT4_TEST_KNOBS, for T4_TEST_TEXT_PIECE) and, with -m gpu, a knob build of the product driver on the GPU."""
import filecmp
import gzip
import os
import re
import shutil
import subprocess
import threading

import pytest

from t4libs import REF_FA, ROOT
from test_dist_gloo import run_engine_merge
from test_stage1_e2e import REF_BIN, _barcode_case, _bulk_case, _emulated_driver, _gunzip

SYNTH = os.path.join(ROOT, "tools", "t4synth")
SUFFIXES = ("_raw.out", "_assembled_reads.fa", "_final.out")
ON = {"T4_GPU_PARSE": "1", "T4_TIMING": "1"}
needs_ref = pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/trust4 not built")
MERGED = r"ProcessRead on the device: (\d+) pairs stay as they are, (\d+) read-through, (\d+) merged, (\d+) with one mate for both"


def knob_driver(emulated):
    """the driver source with -DT4_TEST_KNOBS, linked against the emulator build of the kernels or against the product library"""
    if emulated:
        return _emulated_driver()
    import trust4_amd.build as b
    lib, exe = b.build(), os.path.join(ROOT, "trust4_amd", "bin", "trust4-hip-knobs")
    host = os.path.join(ROOT, "trust4_amd", "host")
    srcs = [os.path.join(host, f) for f in ("trust4_main.cpp", "seq_reader.h", "process_read.h", "byte_stream.h", "text_records.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max([os.path.getmtime(x) for x in srcs] + [os.path.getmtime(lib)]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DT4_TEST_KNOBS", "-o", exe, srcs[0], "-L" + os.path.dirname(lib), "-lt4hip",
                        "-Wl,-rpath," + os.path.dirname(lib), "-lz", "-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module")
def exe():
    return _emulated_driver()


def run(driver, args, out, env=None, check=True, threads="2"):
    e = dict(os.environ)
    for k in ("T4_GPU_PARSE", "T4_TEST_TEXT_PIECE"):
        e.pop(k, None)
    e["T4_TIMING"] = "1"
    e.update(env or {})
    return subprocess.run([driver, "-t", threads] + args + ["-o", out], env=e, stderr=subprocess.PIPE, text=True, check=check)


def same_files(a, b):
    for s in SUFFIXES:
        assert filecmp.cmp(a + s, b + s, shallow=False), (a, b, s)


def took_device_path(log, merged_more_than=20):
    assert "path: device text" in log and "path: host" not in log, log[-800:]
    m = re.search(MERGED, log)
    assert m and int(m.group(3)) > merged_more_than, log[-800:]


def took_host_path(log, reason):
    assert ("path: host (%s" % reason) in log and "path: device text" not in log, log[-800:]


def synth_bulk(d, pairs, clones, seed):
    fa = str(d / "ref.fa")
    _gunzip(REF_FA, fa)
    pre = str(d / "b")
    subprocess.run([SYNTH, fa, str(pairs), str(clones), str(seed), pre], check=True, stdout=subprocess.DEVNULL)
    return fa, pre + "_1.fq", pre + "_2.fq"


@pytest.fixture(scope="module")
def bulk(tmp_path_factory, exe):
    """the input of _bulk_case(.., 240, 5, 11, ..) once more, with the files of the reference binary and of the run without the switch"""
    d = tmp_path_factory.mktemp("stage1_text_bulk")
    fa, f1, f2 = synth_bulk(d, 240, 5, 11)
    args = ["--skipMateExtension", "-f", fa, "-1", f1, "-2", f2]
    subprocess.run([REF_BIN, "-t", "1"] + args + ["-o", str(d / "ref")], check=True, stderr=subprocess.DEVNULL)
    p = run(exe, args, str(d / "off"), threads="4")
    took_host_path(p.stderr, "T4_GPU_PARSE is not 1")
    same_files(str(d / "ref"), str(d / "off"))
    return {"fa": fa, 1: f1, 2: f2, "ref": str(d / "ref"), "off": str(d / "off"), "dir": d}


# ---- the device path ---------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("piece", ["4096", None], ids=["pieces_4096", "default_piece"])
def test_bulk(tmp_path, exe, bulk, piece):
    env = dict(ON, **({"T4_TEST_TEXT_PIECE": piece} if piece else {}))
    log = _bulk_case(tmp_path, exe, 240, 5, 11, env)   # (compares with the reference binary)
    took_device_path(log)
    assert ("pieces of %s bytes" % (piece or str(16 << 20))) in log
    assert filecmp.cmp(str(tmp_path / "b_1.fq"), bulk[1], shallow=False)   # (the same input as the fixture's)
    same_files(bulk["off"], str(tmp_path / "mine"))


@needs_ref
def test_bulk_gzip(tmp_path, exe, bulk):
    for mate in (1, 2):
        with open(bulk[mate], "rb") as f, gzip.open(str(tmp_path / ("in_%d.fq.gz" % mate)), "wb") as g:
            shutil.copyfileobj(f, g)
    args = ["--skipMateExtension", "-f", bulk["fa"], "-1", str(tmp_path / "in_1.fq.gz"), "-2", str(tmp_path / "in_2.fq.gz")]
    p = run(exe, args, str(tmp_path / "on"), dict(ON, T4_TEST_TEXT_PIECE="4096"))
    took_device_path(p.stderr)
    same_files(bulk["ref"], str(tmp_path / "on"))
    same_files(bulk["off"], str(tmp_path / "on"))


def barcode_missing_case(tmp_path, driver, pairs, cells, seed, env, extra=()):
    """_barcode_case's input with every 17th barcode `missing_barcode`: the reference binary, the run without the switch, the run with it"""
    fa = str(tmp_path / "ref.fa")
    _gunzip(REF_FA, fa)
    pre = str(tmp_path / "m5")
    subprocess.run([SYNTH, fa, str(pairs), "0", str(seed), pre, "--cells", str(cells)], check=True)
    lines = open(pre + "_bc.fa").read().split("\n")
    assert len(lines) >= 2 * pairs and lines[0].startswith(">")
    for i in range(0, pairs, 17):
        lines[2 * i + 1] = "missing_barcode"
    with open(pre + "_bc.fa", "w") as f:
        f.write("\n".join(lines))
    args = ["-f", fa, "-1", pre + "_1.fq", "-2", pre + "_2.fq", "--barcode", pre + "_bc.fa", "--UMI", pre + "_umi.fa"] + list(extra)
    ref_o, off_o, on_o = (str(tmp_path / x) for x in ("m_ref", "m_off", "m_on"))
    subprocess.run([REF_BIN, "-t", "1"] + args + ["-o", ref_o], check=True, stderr=subprocess.DEVNULL)
    run(driver, args, off_o)
    p = run(driver, args, on_o, env)
    same_files(ref_o, on_o)
    same_files(off_o, on_o)
    assert open(on_o + "_raw.out").read().count(">") >= cells
    return p.stderr


@needs_ref
def test_barcode_mode(tmp_path, exe):
    _barcode_case(tmp_path, exe, 160, 8, 6, dict(ON, T4_TEST_TEXT_PIECE="8192", T4_THREADS="2"))   # (compares with the reference binary)
    log = barcode_missing_case(tmp_path, exe, 160, 8, 6, dict(ON, T4_TEST_TEXT_PIECE="8192"))
    took_device_path(log)
    assert sum(int(x) for x in re.search(MERGED, log).groups()) == 160 - 10   # (the pairs without a barcode were not looked at)


@needs_ref
def test_two_ranks_cell_shard(tmp_path, exe):
    """two emulated ranks with --cellShard over --gatherDir: every rank uploads the bytes and builds the records of its own cells only"""
    n = run_engine_merge(tmp_path, exe, 160, 8, 6, 2, env=dict(ON, T4_TEST_TEXT_PIECE="8192", HIPEMU_THREADS="2", T4_THREADS="2"), expect_log="path: device text")
    assert n >= 8


# ---- give-backs ----------------------------------------------------------------------------------------------------------------------
def rewrite(src, dst, how):
    recs = open(src).read().split("\n")[:-1]
    recs = [recs[4 * i:4 * i + 4] for i in range(len(recs) // 4)]
    if how == "wrapped":
        text = "".join("%s\n%s\n%s\n+\n%s\n%s\n" % (a, s[:len(s) // 2], s[len(s) // 2:], q[:len(q) // 2], q[len(q) // 2:]) for a, s, _, q in recs)
    elif how == "fasta":
        text = "".join(">%s\n%s\n" % (a[1:], s) for a, s, _, q in recs)
    elif how == "crlf":
        text = "".join("%s\r\n%s\r\n+\r\n%s\r\n" % (a, s, q) for a, s, _, q in recs)
    else:   # a blank line after record 100
        text = "".join("%s\n%s\n+\n%s\n%s" % (a, s, q, "\n" if i == 99 else "") for i, (a, s, _, q) in enumerate(recs))
    with open(dst, "w", newline="") as f:
        f.write(text)


def give_back_case(tmp_path, driver, fa, f1, f2, how, env):
    g1, g2 = str(tmp_path / ("%s_1.fq" % how)), str(tmp_path / ("%s_2.fq" % how))
    rewrite(f1, g1, how)
    rewrite(f2, g2, how)
    args = ["--skipMateExtension", "-f", fa, "-1", g1, "-2", g2]
    off_o, on_o = str(tmp_path / "off"), str(tmp_path / "on")
    run(driver, args, off_o)
    p = run(driver, args, on_o, env)
    line = [x for x in p.stderr.split("\n") if "T4_GPU_PARSE: status" in x]
    assert len(line) == 1 and g1 in line[0] and "record" in line[0], p.stderr[-800:]
    took_host_path(p.stderr, "the device path gave the input back")
    same_files(off_o, on_o)
    assert open(on_o + "_raw.out").read().count(">") > 0
    return line[0]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage1_text_tiny")
    return synth_bulk(d, 30, 2, 3)


@pytest.mark.parametrize("how", ["fasta", "wrapped", "crlf", "blank"])
def test_give_back(tmp_path, exe, bulk, tiny, how):
    # (a form of the whole file is met in the first piece: a small input does; the blank line lies in a later piece of the larger one)
    fa, f1, f2 = (bulk["fa"], bulk[1], bulk[2]) if how == "blank" else tiny
    line = give_back_case(tmp_path, exe, fa, f1, f2, how, dict(ON, T4_TEST_TEXT_PIECE="4096"))
    assert ("status %d " % {"fasta": 1, "wrapped": 2, "crlf": 5, "blank": 1}[how]) in line
    if how == "blank":   # (reads, numberings and counts had accumulated and were dropped)
        assert "record 100 " in line


# ---- refusals, and command lines that keep the host path ----------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["mate_2", "mate_2_empty"])
def test_short_mate_file_as_on_the_host_path(tmp_path, exe, tiny, short):
    fa, f1, f2 = tiny
    cut = str(tmp_path / "cut.fq")
    with open(cut, "w") as f:
        f.write("" if "empty" in short else "\n".join(open(f2).read().split("\n")[:4 * 20]) + "\n")
    args = ["--skipMateExtension", "-f", fa, "-1", f1, "-2", cut]
    off = run(exe, args, str(tmp_path / "off"), check=False)
    msg = lambda p: [x for x in p.stderr.split("\n") if "fewer reads" in x]
    assert off.returncode != 0 and len(msg(off)) == 1
    for piece in ("2048", "1048576"):
        on = run(exe, args, str(tmp_path / "on"), dict(ON, T4_TEST_TEXT_PIECE=piece), check=False)
        assert on.returncode == off.returncode and msg(on) == msg(off), on.stderr[-800:]


@pytest.mark.parametrize("length", [250, 400])
def test_long_first_read_refused_as_on_the_host_path(tmp_path, exe, tiny, length):
    """a first read of more than 200 bases: the host loop's refusal (beyond 384 the piece has status 6 and is given back to it)"""
    fa, f1, f2 = tiny
    g1 = str(tmp_path / "long_1.fq")
    with open(g1, "w") as f:
        f.write("@long\n%s\n+\n%s\n" % ("ACGT" * (length // 4), "I" * (length // 4 * 4)) + "".join(open(f1).read().split("\n", 4)[4:]))
    args = ["--skipMateExtension", "-f", fa, "-1", g1, "-2", f2]
    off = run(exe, args, str(tmp_path / "off"), check=False)
    on = run(exe, args, str(tmp_path / "on"), ON, check=False)
    msg = lambda p: [x for x in p.stderr.split("\n") if "long-read mode" in x]
    assert off.returncode != 0 and on.returncode == off.returncode and len(msg(off)) == 1 and msg(on) == msg(off), on.stderr[-800:]
    assert ("T4_GPU_PARSE: status 6 " in on.stderr) == (length > 384)


def test_short_barcode_file_as_on_the_host_path(tmp_path, exe):
    fa = str(tmp_path / "ref.fa")
    _gunzip(REF_FA, fa)
    pre = str(tmp_path / "c")
    subprocess.run([SYNTH, fa, "30", "0", "3", pre, "--cells", "3"], check=True)
    for name, what in (("_bc.fa", "barcode"), ("_umi.fa", "UMI")):
        cut = str(tmp_path / ("cut" + name))
        with open(cut, "w") as f:
            f.write("\n".join(open(pre + name).read().split("\n")[:2 * 20]) + "\n")
        files = {"_bc.fa": pre + "_bc.fa", "_umi.fa": pre + "_umi.fa"}
        files[name] = cut
        args = ["-f", fa, "-1", pre + "_1.fq", "-2", pre + "_2.fq", "--barcode", files["_bc.fa"], "--UMI", files["_umi.fa"]]
        off = run(exe, args, str(tmp_path / "off"), check=False)
        on = run(exe, args, str(tmp_path / "on"), dict(ON, T4_TEST_TEXT_PIECE="2048"), check=False)
        msg = lambda p: [x for x in p.stderr.split("\n") if "fewer records" in x]
        assert off.returncode != 0 and on.returncode == off.returncode and msg(off) == ["The %s file has fewer records than the read file." % what] and msg(on) == msg(off), on.stderr[-800:]


def test_command_lines_that_keep_the_host_path(tmp_path, exe, tiny):
    fa, f1, f2 = tiny
    p = run(exe, ["-f", fa, "-u", f1], str(tmp_path / "u"), ON)
    took_host_path(p.stderr, "single-end input")
    p = run(exe, ["--skipMateExtension", "-f", fa, "-1", f1, "-1", f1, "-2", f2, "-2", f2], str(tmp_path / "two"), ON)
    took_host_path(p.stderr, "more than one file per mate")
    fifo = str(tmp_path / "in_1.fifo")
    os.mkfifo(fifo)

    def feed():
        with open(f1, "rb") as src, open(fifo, "wb") as dst:
            shutil.copyfileobj(src, dst)
    th = threading.Thread(target=feed)
    th.start()
    try:
        p = run(exe, ["--skipMateExtension", "-f", fa, "-1", fifo, "-2", f2], str(tmp_path / "fifo"), ON)
    finally:   # (a driver that ended without opening the FIFO must not leave the writer waiting for a reader)
        fd = os.open(fifo, os.O_RDONLY | os.O_NONBLOCK)
        th.join()
        os.close(fd)
    took_host_path(p.stderr, "a read file that is not a regular file")
    run(exe, ["--skipMateExtension", "-f", fa, "-1", f1, "-2", f2], str(tmp_path / "plain"))
    same_files(str(tmp_path / "plain"), str(tmp_path / "fifo"))


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_exe():
    return knob_driver(False)


@pytest.mark.gpu
@needs_ref
def test_bulk_gpu(tmp_path, gpu_exe):
    log = _bulk_case(tmp_path, gpu_exe, 3000, 100, 2, dict(ON, T4_TEST_TEXT_PIECE="262144"), threads="8")
    took_device_path(log, 300)
    run(gpu_exe, ["--skipMateExtension", "-f", str(tmp_path / "ref.fa"), "-1", str(tmp_path / "b_1.fq"), "-2", str(tmp_path / "b_2.fq")], str(tmp_path / "off"), threads="8")
    same_files(str(tmp_path / "off"), str(tmp_path / "mine"))


@pytest.mark.gpu
@needs_ref
def test_barcode_mode_gpu(tmp_path, gpu_exe):
    log = barcode_missing_case(tmp_path, gpu_exe, 3000, 60, 4, ON)
    took_device_path(log, 300)


@pytest.mark.gpu
def test_give_back_gpu(tmp_path, gpu_exe):
    fa, f1, f2 = synth_bulk(tmp_path, 600, 20, 5)
    line = give_back_case(tmp_path, gpu_exe, fa, f1, f2, "blank", dict(ON, T4_TEST_TEXT_PIECE="16384"))
    assert "status 1 " in line and "record 100 " in line
