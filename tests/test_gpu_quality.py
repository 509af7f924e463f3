"""The yield and quality counters on the MI355X (qd_qstats_*, quade_amd/csrc/quade_qstats.hip): the table read back from the device
equals tests/qstats_model.py's plain Python sums, exactly -- for the stage on its own (qd_dev_qstats: record shapes, alignments,
quality bytes, destination shapes on both accumulation paths, accumulation, state and errors) and through the command line
(the report against the model over the oracle's per-destination output files)."""
import os
import shutil

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from quade_amd import quality_report as qr
from tests import mismatch_model as MM
from tests import qstats_model as QM
from tests import stage_support as SS
from tests.run_support import _compare_dirs, _scan
from tests.stage_support import LENS, N_SAMPLES, QUALS, Stage, _barcodes, _cli, _engine, torch_cuda  # noqa: F401
from tests.stage_support import _plain_dataset as _dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UND = QM.UNDETERMINED


def _check(eng, want):
    got = eng.qstats_read()
    assert got.shape == want.shape and got.dtype == np.uint64
    assert (got == want).all(), np.argwhere(got != want)[:8]
    assert (got[:, 0, 0] == got[:, 1, 0]).all()  # a pair adds one record to R1 and to R2 of its destination


def test_the_tests_record_table_is_the_device_scans(torch_cuda):
    st = Stage(1, 1025)
    for text, recs, pairs in ((st.t1, st.r1, st.p1), (st.t2, st.r2, st.p2)):
        n, got, res = _scan(text)
        assert n == 1025 and res[5] == 0 and (got == recs).all()
        assert all(text[int(r[3]):int(r[3]) + int(r[4])] == s and text[int(r[5]):int(r[5]) + int(r[4])] == q for r, (s, q) in zip(recs, pairs))
        # the ground the stage tests stand on: every alignment of both lines, CRLF, every quality byte, the Q20 / Q30 edges, N and n
        assert {int(r[3]) % 16 for r in recs if r[4]} == set(range(16)) == {int(r[5]) % 16 for r in recs if r[4]}
        assert b"\r\n" in text and set(b"".join(q for _, q in pairs)) == set(QUALS) >= {52, 53, 62, 63, 0, 32, 128, 255}
        assert {len(s) for s, _ in pairs} == set(LENS)
        allseq = b"".join(s for s, _ in pairs)
        assert allseq.count(b"N") and allseq.count(b"n") and allseq.count(b"a")
    assert any(len(a[0]) != len(b[0]) for a, b in zip(st.p1, st.p2))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_stage_pair_counts_all_three_destinations(torch_cuda, n):
    st = Stage(10 + n, n)
    codes = np.array([0, 1, UND], dtype=np.uint16)[np.random.default_rng(n).integers(0, 3, n)]
    with _engine(1) as eng:
        assert eng.qstats_kind() == "lds"
        st.run(eng, codes)
        want = st.model(1, codes)
        _check(eng, want)
        if n >= 63:
            assert (want[:, 0, 0] > 0).all()


def test_stage_every_pair_undetermined(torch_cuda):
    st = Stage(3, 65)
    codes = np.full(65, UND, dtype=np.uint16)
    with _engine(1) as eng:
        st.run(eng, codes)
        want = st.model(1, codes)
        assert int(want[2, 0, 0]) == 65 and not want[:2].any()
        _check(eng, want)


def test_stage_skewed_routing_on_the_lds_path(torch_cuda):
    """S = 96, three workgroups, 90 % of the pairs to one destination"""
    S, n = 96, 5000
    rng = np.random.default_rng(4)
    st = Stage(4, n)
    codes = rng.integers(0, 2 * S + 1, n)
    codes[codes == 2 * S] = UND
    codes[rng.random(n) < 0.9] = 21
    with _engine(S) as eng:
        assert eng.qstats_kind() == "lds"
        st.run(eng, codes)
        want = st.model(S, codes)
        assert int(want[21, 0, 0]) > 0.88 * n and int((want[:, 0, 0] > 0).sum()) > 150
        _check(eng, want)


def test_stage_large_sheet_on_the_global_path(torch_cuda):
    """S = 4 000: the partials do not fit LDS; equal destinations inside a wave are merged (runs of equal codes make them)"""
    S, n = 4000, 20000
    rng = np.random.default_rng(5)
    st = Stage(5, n, lens=(0, 1, 5, 16, 17, 64, 151))
    codes = rng.integers(0, 2 * S + 1, n)
    codes[codes == 2 * S] = UND
    runs = rng.integers(0, n - 8, 400)
    for a in runs:
        codes[a:a + int(rng.integers(2, 7))] = codes[a]  # neighbours with one destination: 2 .. 4 pairs of a wave
    with _engine(S) as eng:
        assert eng.qstats_kind() == "global"
        st.run(eng, codes)
        _check(eng, st.model(S, codes))


@pytest.mark.parametrize("S,kind", [(682, "lds"), (683, "global")])
def test_stage_both_sides_of_the_lds_limit(torch_cuda, S, kind):
    n = 3000
    rng = np.random.default_rng(S)
    st = Stage(6, n, lens=(0, 3, 16, 65))
    codes = rng.integers(2 * S - 40, 2 * S + 1, n)  # the last destinations of the table
    codes[codes == 2 * S] = UND
    with _engine(S) as eng:
        assert eng.qstats_kind() == kind
        st.run(eng, codes)
        _check(eng, st.model(S, codes))


def test_stage_reads_longer_than_the_lds_partials_take(torch_cuda):
    """reads of more than 2 047 bases go to the 64-bit table directly (a workgroup's 32-bit partials are sized for shorter ones)"""
    st = Stage(7, 70, lens=(2047, 2048, 2049, 5000, 16, 0, 300))
    codes = np.array([0, 1, UND], dtype=np.uint16)[np.random.default_rng(7).integers(0, 3, 70)]
    with _engine(1) as eng:
        st.run(eng, codes)
        _check(eng, st.model(1, codes))


def test_accumulation_reset_and_add(torch_cuda):
    S = 3
    a, b = Stage(20, 300), Stage(21, 65)
    ca = np.random.default_rng(1).integers(0, 2 * S, 300)
    cb = np.random.default_rng(2).integers(0, 2 * S, 65)
    cb[::7] = UND
    with _engine(S) as eng, _engine(S) as other:
        a.run(eng, ca)
        b.run(eng, cb)
        both = a.model(S, ca) + b.model(S, cb)
        _check(eng, both)
        before = eng.counts().copy()
        eng.reset_counts()
        assert not eng.qstats_read().any() and eng.qstats_kind() == "lds"
        b.run(eng, cb)
        _check(eng, b.model(S, cb))
        a.run(other, ca)
        eng.qstats_add(other.qstats_read())  # a second context's table folds in
        _check(eng, both)
        _check(other, a.model(S, ca))
        assert (eng.counts() == 0).all() and (before == 0).all()  # the pair counters are the match kernels' alone
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.qstats_add(np.zeros(5, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        eng.qstats_enable(False)
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.qstats_read()
        assert ei.value.code == hb.QD_ERR_STATE
        eng.qstats_enable(True)
        assert not eng.qstats_read().any()


def test_state_and_errors(torch_cuda):
    S = 2
    st = Stage(30, 64)
    codes = np.random.default_rng(3).integers(0, 2 * S, 64).astype(np.uint16)
    with hb.Engine(0) as eng:
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.qstats_enable(True)  # no plan, no barcodes
        assert ei.value.code == hb.QD_ERR_STATE
        eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        eng.set_barcodes(_barcodes(S))
        for call in (eng.qstats_read, eng.qstats_kind, lambda: st.run(eng, codes), lambda: eng.qstats_add(np.zeros((5, 2, 6), np.uint64))):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        eng.qstats_enable(True)
        out = np.zeros(7, dtype=np.uint64)
        assert eng.lib.qd_qstats_read(eng._h, hb._ptr(out), 7) == hb.QD_ERR_INVALID
        st.run(eng, codes)
        want = st.model(S, codes)
        _check(eng, want)
        # a bad table never becomes an address: refused on the host, nothing launched, the table as it was
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_qstats(st.t1, bad, st.t2, st.r2, codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        bad = st.r2.copy()
        bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_qstats(st.t1, st.r1, st.t2, bad, codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        for code in (2 * S, 0xFFFE):
            c2 = codes.copy()
            c2[9] = code
            with pytest.raises(hb.QuadeHipError) as ei:
                st.run(eng, c2)
            assert ei.value.code == hb.QD_ERR_INVALID
        _check(eng, want)
        eng.set_barcodes(_barcodes(S + 1))  # new barcodes turn the counters off
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.qstats_read()
        assert ei.value.code == hb.QD_ERR_STATE
        eng.qstats_enable(True)
        assert eng.qstats_read().shape == (2 * S + 3, 2, 6)
        eng.set_plan(hb.make_plan(True, 20, (0, 8), (0, 8)))  # and so does a new plan
        eng.set_barcodes(_barcodes(S))
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.qstats_kind()
        assert ei.value.code == hb.QD_ERR_STATE


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------


def _write_conf(path, files, samples, quality=True, **kw):
    SS._write_conf(path, files, samples, quality=quality, **kw)


def _oracle_report(conf, ref_dir, samples):
    """-> (the report's text by the model over the oracle's output files, the oracle's counts)"""
    os.makedirs(ref_dir, exist_ok=True)
    sset, _ = qo.run_quade(str(conf), outdir=str(ref_dir))
    table = QM.table_from_outputs(str(ref_dir), [s[0] for s in samples])
    return "\n".join(qr.report_lines(table, [s[0] for s in samples])) + "\n", sset.counts(), table


def _report(work):
    with open(os.path.join(str(work), qr.REPORT_NAME)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 3 000 pairs in BGZF, run once with the option on; the model's report from the oracle's outputs"""
    top = tmp_path_factory.mktemp("quality_bgzf")
    files, samples = _dataset(str(top / "data"), 41, 2, 3000, bgzf=True)
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    want, counts, table = _oracle_report(conf, top / "ref", samples)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, want=want, counts=counts, table=table, mine=top / "mine", ref=top / "ref")


def test_cli_report_equals_the_model_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    assert int(t[:, 0, 0].sum()) == run["counts"][0] < 6000  # malformed records were dropped
    assert (t[0::2, 0, 0] > 0).all() and t[1:-1:2, 0, 0].sum() > 0 and t[-1, 0, 0] > 0 and t[:, :, 5].sum() > 0
    assert _report(run["mine"]) == run["want"]
    _compare_dirs(str(run["mine"]), str(run["ref"]))  # every other output as without the option
    # reads per destination = the pair counters of Quade_report.csv
    rows = [ln.split("\t") for ln in run["want"].split("\n")[3:] if ln]
    reads = {(r[0], r[1]): int(r[2]) for r in rows}
    with open(run["mine"] / "Quade_report.csv") as fh:
        rep = fh.read().split("\n")
    head = dict(ln.split("\t") for ln in rep[2:9])
    assert reads[("Total", "R1")] == reads[("Total", "R2")] == int(head["Total pair"])
    assert reads[("Undetermined", "R1")] == int(head["Pair Undetermined"])
    blocks = "\n".join(rep).split("Sample Name\t")[1:]
    assert len(blocks) == N_SAMPLES
    for b in blocks:
        f = dict(ln.split("\t") for ln in b.split("\n")[1:4])
        name = b.split("\n")[0]
        for r in ("R1", "R2"):
            assert reads[(name + "_pass", r)] == int(f["Pair pass quality"]) and reads[(name + "_fail", r)] == int(f["Pair fail quality"])


def test_cli_report_equals_the_model_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 42, 2, 3000, bgzf=False)
    conf = tmp_path / "conf.txt"
    _write_conf(conf, files, samples)
    want, counts, _ = _oracle_report(conf, tmp_path / "ref", samples)
    _cli(conf, tmp_path / "mine")
    assert _report(tmp_path / "mine") == want


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
    want, _, _ = _oracle_report(conf, tmp_path / "ref", run["samples"])
    _cli(conf, tmp_path / "shared", ranks=2)
    assert _report(tmp_path / "shared") == want != run["want"]
    conf = tmp_path / "two.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : False\n")
    _cli(conf, tmp_path / "two", ranks=2)
    assert _report(tmp_path / "two") == run["want"]  # = the single process's report
    assert not [f for f in os.listdir(tmp_path / "two") if f.startswith(".quade_rdv")]


def test_cli_rescued_pairs_count_under_their_sample(torch_cuda, tmp_path, monkeypatch):
    files, samples = _dataset(str(tmp_path / "data"), 43, 1, 3000, bgzf=True, one_off=True)
    conf = tmp_path / "conf.txt"
    _write_conf(conf, files, samples, index_extra="index1_mismatches : 1\nindex2_mismatches : 1\n")
    exact, counts0, _ = _oracle_report(conf, tmp_path / "ref0", samples)
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, 16, 8, 1, 1))
    want, counts1, _ = _oracle_report(conf, tmp_path / "ref1", samples)
    assert counts1[3] < counts0[3] and want != exact  # pairs were rescued
    _cli(conf, tmp_path / "mine")
    assert _report(tmp_path / "mine") == want


def test_cli_option_off_writes_nothing_new(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "off.txt"
    _write_conf(conf, run["files"], run["samples"], quality=False)
    _cli(conf, tmp_path / "off")
    assert not os.path.exists(tmp_path / "off" / qr.REPORT_NAME)
    assert sorted(os.listdir(tmp_path / "off")) == sorted(f for f in os.listdir(run["mine"]) if f != qr.REPORT_NAME)
    _compare_dirs(str(tmp_path / "off"), str(run["ref"]))


def test_bundled_golden_run_with_the_option_on(torch_cuda, tmp_path, bundled_dir):
    """the reference's own 299 pairs: S1_pass, S2_pass and Undetermined rows = the model over the reference's result files"""
    from quade_amd.quade import Quade
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt")) as fh:
        base = fh.read()
    work = tmp_path / "result"
    work.mkdir()
    conf = work / "conf.txt"
    conf.write_text(base.replace("[output]\n", "[output]\nquality_report : True\n", 1))
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
    table = QM.table_from_outputs(os.path.join(bundled_dir, "result"), ["S1", "S2"])
    assert [int(table[d, 0, 0]) for d in range(5)] == [25, 0, 27, 0, 247]
    want = qr.report_lines(table, ["S1", "S2"])
    got = _report(work).split("\n")
    assert got[:3] == want[:3]
    rows = {tuple(ln.split("\t")[:2]): ln for ln in got[3:] if ln}
    for ln in want[3:]:
        key = tuple(ln.split("\t")[:2])
        if key[0] in ("S1_pass", "S2_pass", "Undetermined"):
            assert rows[key] == ln
    assert got[:-1] == want  # (the fail destinations are empty in the goldens and in the run: the whole file agrees)
