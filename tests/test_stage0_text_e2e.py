"""`fastq-extractor-hip` under T4_GPU_PARSE=1: the FASTQ text goes to the device piece by piece (t4_text_*, t4_candidate_test) and the
host cuts the kept records out of the pieces. Byte-identical to the reference `fastq-extractor` (oracle/_ref/fastq-extractor) where
it is built; inputs the device path gives back (status != 0) and options it does not take run on the host path, identical to the run
without the switch. Emulated (a test build of the driver with -DT4_TEST_KNOBS, for T4_TEST_TEXT_PIECE) and, with -m gpu, on the GPU."""
import filecmp
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import t4check
from t4libs import REF_FA, ROOT, Synth
from test_stage0_e2e import REF_EXT, barcode_inputs, BARCODE_CASES, stage0_input

HOST = os.path.join(ROOT, "trust4_amd", "host")
SRCS = [os.path.join(HOST, f) for f in ("fastq_extractor_main.cpp", "read_format.h", "seq_reader.h")]
needs_ref = pytest.mark.skipif(not os.path.exists(REF_EXT), reason="oracle/_ref/fastq-extractor not built")


def knob_driver(emulated):
    """the driver source with -DT4_TEST_KNOBS, linked against the emulator build of the kernels or against the product library"""
    if emulated:
        lib, exe, link = t4check.build_emulator_lib(), os.path.join(ROOT, "tests", "hipemu", "fastq-extractor-hip-text-emu"), "-lt4hip_emu"
    else:
        import trust4_amd.build as b
        lib, exe, link = b.build(), os.path.join(ROOT, "trust4_amd", "bin", "fastq-extractor-hip-knobs"), "-lt4hip"
    if not os.path.exists(exe) or os.path.getmtime(exe) < max([os.path.getmtime(x) for x in SRCS] + [os.path.getmtime(lib)]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DT4_TEST_KNOBS", "-o", exe, SRCS[0], "-L" + os.path.dirname(lib), link,
                        "-Wl,-rpath," + os.path.dirname(lib), "-lz", "-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module", params=[True, pytest.param(False, marks=pytest.mark.gpu)], ids=["emu", "gpu"])
def driver(request):
    return knob_driver(request.param)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """stage0_input(11, 60, 150) as two FASTQ files (ids with /1 and /2, a comment on some), their gzip copies, the reference set"""
    d = tmp_path_factory.mktemp("stage0_text")
    fa = str(d / "ref.fa")
    with gzip.open(REF_FA, "rb") as f, open(fa, "wb") as g:
        shutil.copyfileobj(f, g)
    pairs = stage0_input(11, 60, 150)
    files = {"fa": fa, "pairs": pairs}
    for mate in (1, 2):
        text = "".join("@q%d/%d%s\n%s\n+\n%s\n" % (i, mate, " len=%d" % len(p[mate - 1]) if i % 3 == 0 else "", p[mate - 1], "F" * len(p[mate - 1]))
                       for i, p in enumerate(pairs)).encode()
        files[mate] = str(d / ("in_%d.fq" % mate))
        with open(files[mate], "wb") as f:
            f.write(text)
        with gzip.open(files[mate] + ".gz", "wb") as f:
            f.write(text)
    return files


def run(exe, args, out, env=None, check=True):
    e = dict(os.environ)
    e.pop("T4_GPU_PARSE", None)
    e.update(env or {})
    return subprocess.run([exe] + args + ["-o", out], env=e, stderr=subprocess.PIPE, text=True, check=check)


def same_files(a, b, names):
    for s in names:
        assert filecmp.cmp(a + s, b + s, shallow=False), s


CASES = {   # mode, extra arguments, environment beside the switch, gzip input
    "paired": ("paired", [], {}, False), "single": ("single", [], {}, False),
    "pieces_4096": ("paired", [], {"T4_TEST_TEXT_PIECE": "4096"}, False), "single_pieces_1500": ("single", [], {"T4_TEST_TEXT_PIECE": "1500"}, False),
    "t2_ids": ("paired", ["-t", "2"], {"T4_TEST_TEXT_PIECE": "8192"}, False), "gzip": ("paired", [], {"T4_TEST_TEXT_PIECE": "4096"}, True),
}


@needs_ref
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_path_matches_reference_binary(tmp_path, driver, inputs, case):
    mode, extra, env, gz = CASES[case]
    f1, f2 = (inputs[1] + ".gz", inputs[2] + ".gz") if gz else (inputs[1], inputs[2])
    args = ["-f", inputs["fa"]] + (["-u", f1] if mode == "single" else ["-1", f1, "-2", f2])
    ref_o, my_o = str(tmp_path / "ref"), str(tmp_path / "mine")
    subprocess.run([REF_EXT] + (extra or ["-t", "1"]) + args + ["-o", ref_o], check=True, stderr=subprocess.DEVNULL)
    p = run(driver, extra + args, my_o, dict(env, T4_GPU_PARSE="1", T4_TIMING="1"))
    assert "path: device text" in p.stderr and "host path" not in p.stderr, p.stderr
    names = [".fq"] if mode == "single" else ["_1.fq", "_2.fq"]
    same_files(ref_o, my_o, names)
    kept = open(my_o + names[0]).read().count("\n") // 4
    assert 40 <= kept < len(inputs["pairs"]) // 2
    assert ("%d of %d" % (kept, len(inputs["pairs"]))) in p.stderr


def rewrite(inputs, d, how):
    """the same reads in a form the device path gives back -> (file 1, file 2, status it names)"""
    out = []
    for mate in (1, 2):
        recs = open(inputs[mate]).read().split("\n")[:-1]
        recs = [recs[4 * i:4 * i + 4] for i in range(len(recs) // 4)]
        if how == "wrapped":
            text = "".join("%s\n%s\n%s\n+\n%s\n%s\n" % (a, s[:len(s) // 2], s[len(s) // 2:], q[:len(q) // 2], q[len(q) // 2:]) for a, s, _, q in recs)
        elif how == "fasta":
            text = "".join(">%s\n%s\n" % (a[1:], s) for a, s, _, q in recs)
        elif how == "crlf":
            text = "".join("%s\r\n%s\r\n+\r\n%s\r\n" % (a, s, q) for a, s, _, q in recs)
        else:   # a trailing blank line
            text = "".join("%s\n%s\n+\n%s\n" % (a, s, q) for a, s, _, q in recs) + "\n"
        out.append(str(d / ("%s_%d.fq" % (how, mate))))
        with open(out[-1], "w", newline="") as f:
            f.write(text)
    return out[0], out[1], {"wrapped": 2, "fasta": 1, "crlf": 5, "blank": 8}[how]


@pytest.mark.parametrize("how", ["wrapped", "fasta", "crlf", "blank"])
def test_fallback_to_the_host_path(tmp_path, driver, inputs, how):
    f1, f2, status = rewrite(inputs, tmp_path, how)
    args = ["-f", inputs["fa"], "-1", f1, "-2", f2]
    off_o, on_o = str(tmp_path / "off"), str(tmp_path / "on")
    run(driver, args, off_o)
    p = run(driver, args, on_o, {"T4_GPU_PARSE": "1", "T4_TIMING": "1", "T4_TEST_TEXT_PIECE": "16384"})   # (the blank line is met in the fourth piece)
    same_files(off_o, on_o, ["_1.fq", "_2.fq"])
    assert os.path.getsize(on_o + "_1.fq") > 4000
    line = [x for x in p.stderr.split("\n") if "T4_GPU_PARSE" in x and "status" in x]
    assert len(line) == 1 and ("status %d " % status) in line[0] and "path: host" in p.stderr, p.stderr


def test_barcode_run_keeps_the_host_path(tmp_path, driver, inputs):
    f1, f2, fb, wl, tr = barcode_inputs(tmp_path, 13, 30, 60)
    args = ["-f", inputs["fa"], "-1", f1, "-2", f2] + BARCODE_CASES["plain_barcode"](fb, f1, wl, tr)
    off_o, on_o = str(tmp_path / "off"), str(tmp_path / "on")
    run(driver, args, off_o)
    p = run(driver, args, on_o, {"T4_GPU_PARSE": "1", "T4_TIMING": "1"})
    same_files(off_o, on_o, ["_1.fq", "_2.fq", "_bc.fa", "_umi.fa"])
    assert "path: host (--barcode)" in p.stderr
    q = run(driver, ["-f", inputs["fa"], "-1", inputs[1], "-2", inputs[2], "--readFormat", "r1:0:99"], str(tmp_path / "fmt"), {"T4_GPU_PARSE": "1", "T4_TIMING": "1"})
    assert "path: host (--readFormat" in q.stderr


@pytest.mark.parametrize("short", ["mate_2", "mate_2_empty", "mate_1", "mate_1_empty"])
def test_mismatched_files_as_today(tmp_path, driver, inputs, short):
    """different record counts: today's message and exit status (a longer mate file is not an error, today and here)"""
    cut = str(tmp_path / "cut.fq")
    src = open(inputs[2 if "mate_2" in short else 1]).read().split("\n")
    with open(cut, "w") as f:
        f.write("" if "empty" in short else "\n".join(src[:4 * 100]) + "\n")
    f1, f2 = (inputs[1], cut) if "mate_2" in short else (cut, inputs[2])
    args = ["-f", inputs["fa"], "-1", f1, "-2", f2]
    for piece in ("4096", "1048576"):
        off = run(driver, args, str(tmp_path / "off"), check=False)
        on = run(driver, args, str(tmp_path / "on"), {"T4_GPU_PARSE": "1", "T4_TEST_TEXT_PIECE": piece}, check=False)
        assert on.returncode == off.returncode
        msg = lambda p: [x for x in p.stderr.split("\n") if "different number" in x or "empty" in x]
        assert msg(on) == msg(off)
        assert (on.returncode != 0) == (short != "mate_1") and (len(msg(on)) == 1) == (short != "mate_1")
        if short == "mate_1":
            same_files(str(tmp_path / "off"), str(tmp_path / "on"), ["_1.fq", "_2.fq"])


@pytest.mark.gpu
def test_two_pieces_per_file_product_binary(tmp_path):
    """60 000 pairs, 2 % receptor pairs (the benchmark's generator), plain files, the product binary at its default piece size: each
    file spans two pieces. Compared with the same binary without the switch, which the existing tests hold to the reference."""
    import trust4_amd.build as b
    b.build()
    exe = os.path.join(ROOT, "trust4_amd", "bin", "fastq-extractor-hip")
    fa = str(tmp_path / "ref.fa")
    with gzip.open(REF_FA, "rb") as f, open(fa, "wb") as g:
        shutil.copyfileobj(f, g)
    n, nrec = 60000, 1200
    r1, r2 = Synth(2000, 1).next_pairs(nrec)
    rnd = np.random.RandomState(5)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    order = rnd.permutation(n)
    for name, rec in (("in_1.fq", r1), ("in_2.fq", r2)):
        rows = [bytes(x[:150]) for x in rec] + [x.tobytes() for x in acgt[rnd.randint(0, 4, size=(n - nrec, 150))]]
        with open(str(tmp_path / name), "wb") as f:
            f.write(b"".join(b"@q%d\n%s\n+\n%s\n" % (i, rows[i], b"F" * 150) for i in order))
        assert 16 << 20 < os.path.getsize(str(tmp_path / name)) < 32 << 20
    args = ["-f", fa, "-1", str(tmp_path / "in_1.fq"), "-2", str(tmp_path / "in_2.fq")]
    run(exe, args, str(tmp_path / "off"))
    p = run(exe, args, str(tmp_path / "on"), {"T4_GPU_PARSE": "1", "T4_TIMING": "1"})
    assert "path: device text" in p.stderr and "host path" not in p.stderr, p.stderr
    same_files(str(tmp_path / "off"), str(tmp_path / "on"), ["_1.fq", "_2.fq"])
    assert nrec * 9 // 10 <= open(str(tmp_path / "on_1.fq")).read().count("\n") // 4 < 2 * nrec
