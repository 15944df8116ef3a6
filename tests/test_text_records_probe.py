"""The record cutting of trust4-hip's device path (trust4_amd/host/text_records.h: offset table plus piece -> id, sequence, qualities)
as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/text_records_probe.cpp): hand-made records,
pieces cut at every byte, open and closed ends, and offset tables that do not fit their text. No GPU, nothing loaded into Python."""
import os
import subprocess

from t4libs import ROOT


def test_record_cutting_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "text_records_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "text_records_probe.cpp"), "-lz"], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok text records: 6 records"), (p.stdout[-400:], p.stderr[-1500:])
