"""`trust4-hip --barcode` with T4_CELL_IMAGES=resident -- the cells' images stay in their arena slots and change by deltas -- against
the reference binary: _raw.out, _assembled_reads.fa and _final.out byte for byte, with one and with four cell groups, and the run's
statistics say the images travelled whole once and as deltas afterwards. A small case through the driver linked against the
emulator build of the kernels, and the synthetic barcoded pairs of tests/test_cell_images_indexed_e2e.py on the GPU."""
import json
import os

import pytest

from test_stage1_e2e import REF_BIN, _barcode_case, _driver, _emulated_driver


def check_stats(path, cells, groups):
    c = json.load(open(path))["cells"]
    assert c["image_form"] == "resident" and c["groups"] == groups
    assert c["images_resident_whole"] >= cells and c["deltas"] > 0 and c["whole_restages"] > 0
    assert c["images_resident_whole"] + c["deltas"] == c["images_staged"]
    assert c["delta_contigs_shipped"] >= c["deltas"]
    assert c["images_indexed_on_device"] == 0 and c["images_built_on_device"] == 0 and c["key_records_shipped"] == 0


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/trust4 not built")
@pytest.mark.parametrize("groups", [1, 4])
def test_barcode_driver_with_resident_images_emulated(tmp_path, groups):
    stats = str(tmp_path / "stats.json")
    _barcode_case(tmp_path, _emulated_driver(), 160, 8, 6, {"T4_LANES": "8", "T4_WINDOW": "2", "T4_THREADS": "4", "T4_CELL_GROUPS": str(groups),
                                                            "HIPEMU_THREADS": "2", "T4_STATS_JSON": stats, "T4_CELL_IMAGES": "resident"})
    check_stats(stats, 8, groups)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/trust4 not shipped")
@pytest.mark.parametrize("groups", [1, 4])
def test_barcode_driver_with_resident_images_matches_reference_binary(tmp_path, groups):
    """4 000 synthetic pairs over 50 cells"""
    stats = str(tmp_path / "stats.json")
    _barcode_case(tmp_path, _driver(), 4000, 50, 9, {"T4_THREADS": "8", "T4_CELL_GROUPS": str(groups), "T4_STATS_JSON": stats, "T4_CELL_IMAGES": "resident"})
    check_stats(stats, 50, groups)
