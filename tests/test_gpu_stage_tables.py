"""The six read stages of one context side by side on the MI355X (qd_qstats_*, qd_cstats_*, qd_clip_*, qd_trim_*, qd_pairtrim_*,
qd_filter_*): they share one table helper and one upload harness in quade_api.cpp and one marshalling helper in hip_backend.py, so
what can go wrong is the wiring -- one stage's call reaching another stage's table, or a size taken from the wrong stage.  One
Engine with two samples and every stage on takes one small batch: every table equals its Python model, an add reaches its own table
and no other, and every refusal (wrong size, stage off, a record beyond its text) names the right error and changes nothing.  Every
refusal here is a host-side check that returns before any launch."""
import numpy as np
import pytest

from quade_amd import hip_backend as hb
from tests import clip_model as CM
from tests import cycle_model as CYM
from tests import filter_model as FM
from tests import pairtrim_model as PM
from tests import qstats_model as QM
from tests import trim_model as TM
from tests.stage_support import _barcodes, _text_from

pytestmark = pytest.mark.gpu

S, N, L = 2, 17, 20  # 17 pairs: one full step of a workgroup's 16 rows and one row of a ragged second step
BY_ENGINE = {s.engine: s for s in hb.STAGES}  # the product's stage table, by the prefix of the Engine methods
STAGES = tuple(BY_ENGINE)  # qstats, cstats, clip, trim, pairtrim, filter: stage k of the add test is STAGES[k - 1]
CODES = (0, 3, CYM.UNDETERMINED)  # sample 0 pass, sample 1 fail, Undetermined
CLIP = CM.Params(front_clip=(1, 0), tail_clip=(0, 2), window_size=4, window_quality=20, poly_g_min_length=6, min_length=5)
TRIM = TM.Params("AGATCGGAAG", "AGATCGGAAG", quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=4)
PAIR = PM.Params(min_overlap=8, max_mismatches=2, max_mismatch_pct=20, min_length=6)
FILTER = FM.Params(min_length=18, max_n=1, min_mean_quality=20, min_complexity_pct=30)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


class Batch(object):
    """17 pairs of 2 x 20 bp; _text_from gives the names 2 .. 22 bytes, so the lines start at several offsets mod 16.  Among the
    pairs: inserts shorter than the reads (R2 the reverse complement of R1's start), adapters, poly-G tails, N and low qualities, so
    that every stage's counters move."""

    def __init__(self):
        rng = np.random.default_rng(1417)
        self.cases = ([], [])
        for j in range(N):
            s1 = bytearray(b"ACGT"[int(v)] for v in rng.integers(0, 4, L))
            s2 = bytearray(b"ACGT"[int(v)] for v in rng.integers(0, 4, L))
            if j % 4 == 1:  # an insert of 12 .. 19 bases
                I = 12 + j % 8
                s2[:I] = bytes(s1[:I]).translate(COMP)[::-1]
            if j % 4 == 2:
                s1[L - 7:] = TRIM.adapters[0][:7]
            if j % 5 == 3:
                s2[L - 8:] = b"G" * 8
            if j % 6 == 4:
                s1[3:6] = b"NnN"
            if j % 7 == 5:
                s2[:] = b"A" * L
            q = [bytearray(33 + int(v) for v in rng.integers(2 if j % 3 == 0 else 22, 41, L)) for _ in range(2)]
            self.cases[0].append(("pair %d" % j, bytes(s1), bytes(q[0])))
            self.cases[1].append(("pair %d" % j, bytes(s2), bytes(q[1])))
        (self.t1, self.r1), (self.t2, self.r2) = (_text_from(rng, c) for c in self.cases)
        self.codes = np.array([CODES[j % 3] for j in range(N)], dtype=np.uint16)

    def pairs(self):
        return [(int(self.codes[j]), self.cases[0][j][1:], self.cases[1][j][1:]) for j in range(N)]

    def run(self, eng, stage, r1=None):
        """the stage's dev_* over the batch (r1: another record table for R1)"""
        a = (self.t1, self.r1 if r1 is None else r1, self.t2, self.r2)
        if stage in ("qstats", "cstats", "filter"):
            return getattr(eng, "dev_" + stage)(*a, self.codes)
        return getattr(eng, "dev_" + stage)(*a)

    def model(self):
        """-> {stage: its table after one run over the batch, flat uint64}"""
        clip, trim, pair, flt = CM.new_table(), TM.new_table(), PM.new_table(), FM.new_table(S)
        for code, r1, r2 in self.pairs():
            for r, (seq, qual) in enumerate((r1, r2)):
                CM.count(clip, seq, qual, r, CLIP)
                TM.count(trim, seq, qual, r, TRIM)
            PM.count(pair, r1[0], r2[0], PAIR)
            FM.count(flt, code, r1, r2, FILTER)
        out = {"qstats": QM.table(S, self.pairs()), "cstats": hb.cstats_flat(CYM.table([(c, 0, r1, r2) for c, r1, r2 in self.pairs()])),
               "clip": clip, "trim": trim, "pairtrim": pair, "filter": flt}
        return {k: np.array(v, dtype=np.uint64).reshape(-1) for k, v in out.items()}


def _configured():
    eng = hb.Engine(0)
    eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
    eng.set_barcodes(_barcodes(S))
    return eng


def _read(eng, stage):
    return np.asarray(BY_ENGINE[stage].read(eng)).reshape(-1).copy()


def _read_all(eng):
    return {stage: _read(eng, stage) for stage in STAGES}


def _raw_read(eng, stage, out):
    """qd_<stage>_read into a caller's array, whatever its size"""
    eng._chk(getattr(eng.lib, "qd_%s_read" % stage)(eng._h, hb._ptr(out), out.size))


@pytest.fixture(scope="module")
def ctx():
    """(the engine with all six stages on, the batch, T0: every table after every stage has run over the batch once, and what
    every table holds now: the test that adds keeps it current)"""
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    batch = Batch()
    with _configured() as eng:
        eng.qstats_enable(True)
        eng.cstats_enable(True)
        eng.clip_set(**CLIP.keywords())
        eng.trim_set(TRIM.adapters[0], TRIM.adapters[1], TRIM.quality_cutoff, TRIM.min_overlap, TRIM.max_mismatch_pct, TRIM.min_length)
        eng.pairtrim_set(**PAIR.keywords())
        eng.filter_set(**FILTER.keywords())
        for stage in STAGES:
            batch.run(eng, stage)
        t0 = _read_all(eng)
        yield eng, batch, t0, {k: v.copy() for k, v in t0.items()}


def _check_all(eng, now):
    got = _read_all(eng)
    for stage in STAGES:
        assert got[stage].shape == now[stage].shape and (got[stage] == now[stage]).all(), stage


def test_baseline_equals_the_models(ctx):
    eng, batch, t0, _ = ctx
    want = batch.model()
    assert [t0[s].size for s in STAGES] == [(2 * S + 1) * 12, hb.CSTATS_VALUES, 24, 16, hb.PAIRTRIM_VALUES, (2 * S + 1) * 8]
    for stage in STAGES:
        assert (t0[stage] == want[stage]).all(), stage
        assert t0[stage].any(), stage  # (the batch moves every stage's counters)
    # the batch is what the stages are meant to see: a short insert, an adapter, a poly-G tail and a dropped pair among its pairs
    assert want["pairtrim"][PM.PAIRS + 2] > 0 and want["trim"][5] > 0 and want["clip"][9] + want["clip"][12 + 9] > 0
    assert 0 < want["filter"].reshape(-1, 8)[:, 1:6].sum() < N


def test_an_add_reaches_its_own_table_only(ctx):
    eng, batch, t0, now = ctx
    for k, stage in enumerate(STAGES, 1):
        getattr(eng, stage + "_add")(np.full(now[stage].size, k, dtype=np.uint64))
        now[stage] += np.uint64(k)
        assert (now[stage] == t0[stage] + np.uint64(k)).all()
        _check_all(eng, now)  # this stage's table is T0 + k in every cell, the others are as they were


@pytest.mark.parametrize("stage", STAGES)
def test_a_table_one_value_short_is_refused(ctx, stage):
    eng, batch, _, now = ctx
    short = np.zeros(now[stage].size - 1, dtype=np.uint64)
    with pytest.raises(hb.QuadeHipError) as ei:
        _raw_read(eng, stage, short)
    assert ei.value.code == hb.QD_ERR_INVALID
    with pytest.raises(hb.QuadeHipError) as ei:
        getattr(eng, stage + "_add")(short + np.uint64(1))
    assert ei.value.code == hb.QD_ERR_INVALID
    _check_all(eng, now)


@pytest.mark.parametrize("stage", STAGES)
def test_a_stage_that_is_off_is_refused(ctx, stage):
    _, batch, _, now = ctx
    with _configured() as off:
        table = np.zeros(now[stage].size, dtype=np.uint64)
        for call in (lambda: _raw_read(off, stage, table), lambda: getattr(off, stage + "_add")(table)):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        if stage in ("clip", "trim", "pairtrim", "filter"):
            with pytest.raises(hb.QuadeHipError) as ei:
                batch.run(off, stage)
            assert ei.value.code == hb.QD_ERR_STATE


@pytest.mark.parametrize("stage", STAGES)
def test_a_record_beyond_its_text_is_refused(ctx, stage):
    eng, batch, _, now = ctx
    bad = batch.r1.copy()
    bad[N - 1, 5] = len(batch.t1) + 1 - int(bad[N - 1, 4])  # qual + seq_len: one byte beyond the text
    with pytest.raises(hb.QuadeHipError) as ei:
        batch.run(eng, stage, r1=bad)
    assert ei.value.code == hb.QD_ERR_INVALID
    _check_all(eng, now)
