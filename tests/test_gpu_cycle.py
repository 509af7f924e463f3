"""The per-cycle counters on the MI355X (qd_cstats_*, quade_amd/csrc/quade_cstats.hip): the table read back from the device equals
tests/cycle_model.py's plain Python sums, exactly -- for the stage on its own (qd_dev_cstats: record shapes, alignments, quality
bytes, letters, groups, drop bytes, both sides of the LDS range, accumulation, state and errors) and through the command line (the
report against the model over the oracle's per-destination output files).  The texts are tests/test_gpu_quality.py's: every
alignment of both lines, CRLF, every quality byte including < 33 and >= 0x80, the bases ACGTNnacgtRYKM.* (its own first test
pins that ground)."""
import os
import shutil

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import cycle_report as cr
from quade_amd import hip_backend as hb
from quade_amd import quality_report as qr
from tests import cycle_model as CM
from tests import qstats_model as QM
from tests import stage_support as SS
from tests.run_support import _compare_dirs
from tests.stage_support import LENS, Stage, _barcodes, _cli, _engine, torch_cuda  # noqa: F401
from tests.stage_support import _plain_dataset as _dataset

pytestmark = pytest.mark.gpu
UND = CM.UNDETERMINED
WG_PAIRS = 4096  # pairs per workgroup of the kernel (quade_cstats.hip)


class CStage(Stage):
    def model(self, codes, drop=None):
        drop = [0] * self.n if drop is None else drop
        return CM.table([(int(c), int(d), a, b) for c, d, a, b in zip(codes, drop, self.p1, self.p2)])

    def run(self, eng, codes, drop=None):
        eng.dev_cstats(self.t1, self.r1, self.t2, self.r2, np.asarray(codes, dtype=np.uint16), drop)


def _cengine(S=1):
    eng = _engine(S, enable=False)
    eng.cstats_enable(True)
    return eng


def _check(eng, want):
    got = eng.cstats_read()
    assert set(got) == set(want) == {"cycle", "len", "meanq", "gc"}
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == np.uint64
        assert (got[k] == want[k]).all(), (k, np.argwhere(got[k] != want[k])[:8])
    assert (got["len"].sum(axis=2)[:, 0] == got["len"].sum(axis=2)[:, 1]).all()  # a pair adds one read to R1 and to R2 of its group


def _mix(seed, n):
    return np.array([0, 1, UND], dtype=np.uint16)[np.random.default_rng(seed).integers(0, 3, n)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025, 2 * WG_PAIRS + 1])
def test_stage_pair_counts_all_three_groups(torch_cuda, n):
    """lengths 0 .. 300 of tests/test_gpu_quality.py's LENS; the last count makes three workgroups"""
    assert LENS == (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 151, 300)
    st = CStage(10 + n, n)
    codes = _mix(n, n)
    with _cengine(1) as eng:
        st.run(eng, codes)
        want = st.model(codes)
        _check(eng, want)
        if n >= 63:
            assert (want["len"].sum(axis=2) > 0).all() and want["cycle"][:, :, 299].any()
            assert (want["cycle"].sum(axis=(0, 1, 2)) > 0).all()  # every counter is fed


@pytest.mark.parametrize("routing", ["pass", "undetermined", "mix", "sheet96", "sheet4000"])
def test_stage_routing(torch_cuda, routing):
    n = 400
    rng = np.random.default_rng(len(routing))
    S = {"sheet96": 96, "sheet4000": 4000}.get(routing, 1)
    if routing == "pass":
        codes = np.zeros(n, dtype=np.uint16)
    elif routing == "undetermined":
        codes = np.full(n, UND, dtype=np.uint16)
    elif routing == "mix":
        codes = _mix(7, n)
    else:  # odd and even codes of the whole sheet, the last ones included
        codes = rng.integers(0, 2 * S + 1, n)
        codes[:5] = (2 * S - 1, 2 * S - 2, 0, 1, 2 * S)
        codes[codes == 2 * S] = UND
    st = CStage(40 + S, n)
    with _cengine(S) as eng:
        st.run(eng, codes)
        want = st.model(codes)
        present = [bool(want["len"][g].any()) for g in range(3)]
        assert present == {"pass": [True, False, False], "undetermined": [False, False, True]}.get(routing, [True, True, True])
        _check(eng, want)


def test_stage_both_sides_of_the_lds_range_and_of_the_cycle_limit(torch_cuda):
    lds = hb.load_library().qd_cstats_lds_cycles()
    assert 16 <= lds < 1023
    lens = (lds - 1, lds, lds + 1, 1023, 1024, 1025, 2500, 0, 1, 17, 151)
    st = CStage(50, 130, lens=lens)
    assert {len(s) for s, _ in st.p1} == set(lens) == {len(s) for s, _ in st.p2}
    codes = _mix(50, 130)
    with _cengine(1) as eng:
        st.run(eng, codes)
        want = st.model(codes)
        assert want["cycle"][:, :, lds - 1].any() and want["cycle"][:, :, lds].any() and want["cycle"][:, :, 1023].any()
        assert want["len"][:, :, 1024].sum() > want["len"][:, :, 1023].sum() > 0  # 1024, 1025 and 2500 share the last bin
        _check(eng, want)


@pytest.mark.parametrize("dropped", ["none", "some", "all"])
def test_stage_drop_bytes(torch_cuda, dropped):
    n = 300
    st = CStage(60, n)
    codes = _mix(60, n)
    drop = np.zeros(n, dtype=np.uint8)
    if dropped == "some":
        drop[np.random.default_rng(61).random(n) < 0.4] = 3
        drop[::17] = 255  # any non-zero byte drops
    elif dropped == "all":
        drop[:] = 1
    with _cengine(1) as eng:
        st.run(eng, codes, drop)
        want = st.model(codes, drop)
        assert int(want["len"].sum()) == 2 * int((drop == 0).sum())  # a dropped pair adds nothing anywhere
        _check(eng, want)
        if dropped == "all":
            assert not any(v.any() for v in eng.cstats_read().values())
        elif dropped == "some":
            assert 0.2 * n < int((drop != 0).sum()) < 0.8 * n


def test_stage_one_length_for_every_read(torch_cuda):
    """every read of a run has one length: the hot len bin comes out exact (two workgroups)"""
    n = WG_PAIRS + 300
    st = CStage(70, n, lens=(151,))
    codes = np.zeros(n, dtype=np.uint16)
    with _cengine(1) as eng:
        st.run(eng, codes)
        got = eng.cstats_read()
        assert got["len"][0, :, 151].tolist() == [n, n] and int(got["len"].sum()) == 2 * n
        _check(eng, st.model(codes))


def test_accumulation_reset_and_add(torch_cuda):
    S = 3
    a, b = CStage(20, 300), CStage(21, 65)
    ca = np.random.default_rng(1).integers(0, 2 * S, 300)
    cb = np.random.default_rng(2).integers(0, 2 * S, 65)
    cb[::7] = UND
    with _cengine(S) as eng, _cengine(S) as other:
        a.run(eng, ca)
        b.run(eng, cb)
        both = CM.add(a.model(ca), b.model(cb))
        _check(eng, both)
        eng.reset_counts()
        assert not any(v.any() for v in eng.cstats_read().values())
        b.run(eng, cb)
        _check(eng, b.model(cb))
        a.run(other, ca)
        eng.cstats_add(other.cstats_read())  # a second context's table folds in
        _check(eng, both)
        _check(other, a.model(ca))
        eng.set_barcodes(_barcodes(S + 1))  # the table does not depend on the sheet: new barcodes leave it on and as it is
        _check(eng, both)
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.cstats_add(np.zeros(5, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        out = np.zeros(7, dtype=np.uint64)
        assert eng.lib.qd_cstats_read(eng._h, hb._ptr(out), 7) == hb.QD_ERR_INVALID
        eng.cstats_enable(False)
        for call in (eng.cstats_read, lambda: eng.cstats_add(np.zeros(hb.CSTATS_VALUES, np.uint64)), lambda: b.run(eng, cb)):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        eng.cstats_enable(True)
        assert not any(v.any() for v in eng.cstats_read().values())
    with hb.Engine(0) as bare:  # no plan, no barcodes: the table is independent of both
        bare.cstats_enable(True)
        assert not any(v.any() for v in bare.cstats_read().values())


def test_bad_tables_and_codes_are_refused_before_the_launch(torch_cuda):
    S = 2
    st = CStage(30, 64)
    codes = np.random.default_rng(3).integers(0, 2 * S, 64).astype(np.uint16)
    with _cengine(S) as eng:
        st.run(eng, codes)
        want = st.model(codes)
        _check(eng, want)
        # a bad table never becomes an address: refused on the host, nothing launched, the table as it was
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_cstats(st.t1, bad, st.t2, st.r2, codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        bad = st.r2.copy()
        bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_cstats(st.t1, st.r1, st.t2, bad, codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        for code in (2 * S, 0xFFFE):
            c2 = codes.copy()
            c2[9] = code
            with pytest.raises(hb.QuadeHipError) as ei:
                st.run(eng, c2)
            assert ei.value.code == hb.QD_ERR_INVALID
        _check(eng, want)


def test_cross_checks_against_the_quality_counters_of_the_same_call(torch_cuda):
    """reads of at most 1024 bases: summed over cycles and groups N, qual_sum, q20 and q30 are the qstats table's columns, and the
    sum of L * len[L] its bases"""
    S, n = 5, 700
    st = CStage(80, n, lens=LENS + (1023, 1024))
    codes = np.random.default_rng(80).integers(0, 2 * S + 1, n)
    codes[codes == 2 * S] = UND
    with _engine(S) as eng:  # the quality counters on
        eng.cstats_enable(True)
        Stage.run(st, eng, codes)
        st.run(eng, codes)
        qs, cs = eng.qstats_read(), eng.cstats_read()
        assert (qs == Stage.model(st, S, codes)).all()
        want = [[int(qs[:, r, k].sum()) for k in range(6)] for r in range(2)]
        assert CM.qstats_columns(cs) == want and want[0][0] == n and min(want[0] + want[1]) > 0
        # per group too: pass = the even codes
        even = [int(qs[0:2 * S:2, r, 1].sum()) for r in range(2)]
        assert [int(sum(L * int(v) for L, v in enumerate(cs["len"][0, r]))) for r in range(2)] == even


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
def _write_conf(path, files, samples, cycle=True, **kw):
    SS._write_conf(path, files, samples, **kw)
    if cycle:
        text = open(path).read().replace("[output]\n", "[output]\ncycle_report : True\n", 1)
        open(path, "w").write(text)


def _names(samples):
    return [s[0] for s in samples]


def _text(table):
    return "\n".join(cr.report_lines(table)) + "\n"


def _oracle_report(conf, ref_dir, samples):
    """-> (the report's text by the model over the oracle's output files, the table)"""
    os.makedirs(ref_dir, exist_ok=True)
    qo.run_quade(str(conf), outdir=str(ref_dir))
    table = CM.table_from_outputs(str(ref_dir), _names(samples))
    return _text(table), table


def _report(work):
    with open(os.path.join(str(work), cr.REPORT_NAME)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 3 000 pairs in BGZF, batch_pairs 1000, run once with the option on; the model's report from the oracle's outputs"""
    top = tmp_path_factory.mktemp("cycle_bgzf")
    files, samples = _dataset(str(top / "data"), 41, 2, 3000, bgzf=True)
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    want, table = _oracle_report(conf, top / "ref", samples)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, want=want, table=table, mine=top / "mine", ref=top / "ref")


def test_cli_report_equals_the_model_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    assert (t["len"].sum(axis=2) > 0).all() and t["cycle"][:, :, :, 4].sum() > 0 and 5000 < t["len"][:, 0].sum() < 6000
    assert _report(run["mine"]) == run["want"]
    _compare_dirs(str(run["mine"]), str(run["ref"]))  # every other output as without the option
    lines = run["want"].split("\n")
    assert lines[2].startswith("group\tread\tcycle") and "Read lengths" in lines and "Reads of 1024" not in run["want"]
    assert sum(1 for ln in lines if ln.startswith("Total\tR1\t") and len(ln.split("\t")) == 16) == 151  # the longest read


def test_cli_report_equals_the_model_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 42, 2, 3000, bgzf=False)
    conf = tmp_path / "conf.txt"
    _write_conf(conf, files, samples)
    want, _ = _oracle_report(conf, tmp_path / "ref", samples)
    _cli(conf, tmp_path / "mine")
    assert _report(tmp_path / "mine") == want
    _compare_dirs(str(tmp_path / "mine"), str(tmp_path / "ref"))


def test_cli_report_does_not_depend_on_write_flags_or_chunk_workers(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "flags.txt"
    _write_conf(conf, run["files"], run["samples"], flags=(True, False, False))
    _cli(conf, tmp_path / "flags")
    assert _report(tmp_path / "flags") == run["want"]
    assert not [f for f in os.listdir(tmp_path / "flags") if "_fail_" in f or f.startswith("Undetermined")]
    conf = tmp_path / "workers.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="chunk_workers : 2\n")
    _cli(conf, tmp_path / "workers")
    assert _report(tmp_path / "workers") == run["want"]


def test_cli_two_ranks_sharded_and_whole_chunks(bgzf_run, tmp_path):
    """2 ranks on GPU 0 (tables through the rendezvous files): each a pair range of ONE shared BGZF chunk, then a chunk each"""
    run = bgzf_run
    conf = tmp_path / "shared.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : True\n", chunks=[0])
    want, _ = _oracle_report(conf, tmp_path / "ref", run["samples"])
    _cli(conf, tmp_path / "shared", ranks=2)
    assert _report(tmp_path / "shared") == want != run["want"]
    conf = tmp_path / "two.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : False\n")
    _cli(conf, tmp_path / "two", ranks=2)
    assert _report(tmp_path / "two") == run["want"]  # = the single process's report
    assert not [f for f in os.listdir(tmp_path / "two") if f.startswith(".quade_rdv")]


def test_cli_behind_trim_pair_overlap_and_filter(torch_cuda, tmp_path):
    """[trim], pair_overlap and [filter] on, all write flags on: the report is the model over the files this run wrote (which
    tests/test_gpu_filter.py pins), and its totals are those of the Quade_quality_report.csv of the same run"""
    files, samples = SS._filter_dataset(str(tmp_path / "data"), 71, 2, 1500, bgzf=True)
    conf = tmp_path / "conf.txt"
    SS._write_conf(conf, files, samples, extra=SS.TRIMS + SS.FILTER, quality=True)
    text = open(conf).read().replace("[output]\n", "[output]\ncycle_report : True\n", 1)
    open(conf, "w").write(text)
    _cli(conf, tmp_path / "mine")
    table = CM.table_from_outputs(str(tmp_path / "mine"), _names(samples))
    assert _report(tmp_path / "mine") == _text(table)
    assert (table["len"].sum(axis=2) > 0).all() and not table["len"][:, :, :40].any()  # the filter's min_length 40 held
    with open(tmp_path / "mine" / qr.REPORT_NAME) as fh:
        rows = [ln.split("\t") for ln in fh.read().split("\n") if ln.startswith("Total\t")]
    cols = CM.qstats_columns(table)
    for r, row in enumerate(rows):  # reads, bases, q20, q30, mean quality, N
        records, bases, qual_sum, q20, q30, n_bases = cols[r]
        assert [row[2], row[3], row[5], row[6], row[9], row[10]] == [str(records), str(bases), str(q20), str(q30),
                                                                      qr.ratio(qual_sum, bases), str(n_bases)]
    assert len(rows) == 2


def test_cli_option_off_writes_nothing_new(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "off.txt"
    _write_conf(conf, run["files"], run["samples"], cycle=False)
    _cli(conf, tmp_path / "off")
    assert not os.path.exists(tmp_path / "off" / cr.REPORT_NAME)
    assert sorted(os.listdir(tmp_path / "off")) == sorted(f for f in os.listdir(run["mine"]) if f != cr.REPORT_NAME)
    _compare_dirs(str(tmp_path / "off"), str(run["ref"]))


def test_bundled_golden_run_with_the_option_on(torch_cuda, tmp_path, bundled_dir):
    """the reference's own 299 pairs: other outputs byte-identical, the report = the model over the reference's result files"""
    from quade_amd.quade import Quade
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt")) as fh:
        base = fh.read()
    work = tmp_path / "result"
    work.mkdir()
    conf = work / "conf.txt"
    conf.write_text(base.replace("[output]\n", "[output]\ncycle_report : True\n", 1))
    old = os.getcwd()
    os.chdir(str(work))
    try:
        q = Quade(conf_file=str(conf))
        assert q() == 0
    finally:
        os.chdir(old)
    os.remove(conf)
    st = q.pipe_stats
    assert st is not None and st["gzip_fallbacks"] == 0 and st["host_inflated_runs"] == 0, st
    _compare_dirs(str(work), os.path.join(bundled_dir, "result"))  # all other outputs byte-identical to the goldens
    table = CM.table_from_outputs(os.path.join(bundled_dir, "result"), ["S1", "S2"])
    assert [int(table["len"][g, 0].sum()) for g in range(3)] == [52, 0, 247]
    assert _report(work) == _text(table)
