"""The stage table (quade_amd/stages.py) that drives a run's read stages: its order, the bytes a table has in the ranks' exchange,
what a conf switches on through it and the reports it writes; and that no test module imports another one."""
import glob
import os
import re

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from tests.stage_support import _one_sample_conf

NAMES = ["quality", "cycle", "clip", "trim", "pairtrim", "filter"]
# a table of the stage for a sheet of 4 samples (9 destinations), and the uint64 its packed form starts with (None: nothing)
SHAPES = {"quality": ((9, 2, 6), 9), "cycle": ((56472,), 56472), "clip": ((2, 12), None), "trim": ((2, 8), None),
          "pairtrim": ((1040,), None), "filter": ((9, 8), 9)}
REPORTS = ["Quade_quality_report.csv", "Quade_cycle_report.csv", "Quade_clip_report.csv", "Quade_trim_report.csv",
           "Quade_pair_trim_report.csv", "Quade_filter_report.csv"]
ALL_ON = ("quality_report : True\ncycle_report : True\n[trim]\nfront_clip_R1 : 2\nquality_cutoff : 20\npair_overlap : True\n"
          "[filter]\nmin_length : 40\n")


def test_the_table_lists_the_six_stages_in_pipeline_order():
    assert [s.name for s in hb.STAGES] == NAMES and list(hb.STAGE) == NAMES
    assert all(hb.STAGE[s.name] is s for s in hb.STAGES)


@pytest.mark.parametrize("name", NAMES)
def test_pack_format(name):
    """the rendezvous format, built here by hand: the destination count in front of qstats and filter tables, the value count in
    front of the cycle table, nothing in front of the others; then the values, little-endian uint64 in C order"""
    shape, head = SHAPES[name]
    table = np.random.default_rng(len(name)).integers(0, 1 << 63, shape, dtype=np.uint64)
    want = (b"" if head is None else np.array([head], dtype="<u8").tobytes()) + table.astype("<u8").tobytes()
    assert hb.pack_table(name, table) == want == hb.pack_table(hb.STAGE[name], table.reshape(-1))
    back = hb.unpack_table(name, want)
    back = hb.cstats_flat(back) if name == "cycle" else back
    assert back.shape == shape and back.dtype == np.uint64 and (back == table).all() and back.flags.writeable
    for bad in (want[:-8], want + bytes(8)):
        with pytest.raises(AssertionError, match="of the wrong size"):
            hb.unpack_table(name, bad)


def _stub(stage):
    table = np.zeros([3 if d < 0 else d for d in stage.shape], dtype=np.uint64)  # one sample: 3 destinations
    return stage.view(table) if stage.view else table


@pytest.mark.parametrize("extra,on", [(ALL_ON, True), ("", False)], ids=["all_on", "all_off"])
def test_conf_switches_and_reports_through_the_table(tmp_path, extra, on):
    cf = qconf.QuadeConf(_one_sample_conf(tmp_path, extra))
    assert cf.can_pipe and [s.on(cf) for s in hb.STAGES] == [on] * 6
    assert [s.conf_params(cf) is not None for s in hb.STAGES] == [False, False, True, True, True, True]
    out = tmp_path / "out"
    out.mkdir()
    written = [os.path.basename(s.write_report(str(out), _stub(s), ["S1"], s.conf_params(cf))) for s in hb.STAGES if s.on(cf)]
    assert written == (REPORTS if on else []) and sorted(os.listdir(out)) == sorted(written)
    for name in written:
        assert (out / name).read_text().startswith("Program Quade-")


def test_no_test_module_imports_another():
    here = os.path.dirname(os.path.abspath(__file__))
    paths = sorted(glob.glob(os.path.join(here, "test_*.py")))
    assert len(paths) > 30
    pattern = re.compile(r"^\s*(from\s+tests\.test_\w+\s+import|from\s+tests\s+import\s+[^\n]*\btest_\w+|import\s+tests\.test_\w+|"
                         r"from\s+\.\s*test_\w+\s+import|from\s+\.\s+import\s+[^\n]*\btest_\w+)", re.M)
    found = [(os.path.basename(p), m.group(0).strip()) for p in paths for m in pattern.finditer(open(p).read())]
    assert not found, found
