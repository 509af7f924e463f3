"""The six read stages of one context side by side on the MI355X (qd_qstats_*, qd_cstats_*, qd_clip_*, qd_trim_*, qd_pairtrim_*,
qd_filter_*): they share one table helper and one upload harness in quade_api.cpp and one marshalling helper in hip_backend.py, so
what can go wrong is the wiring -- one stage's call reaching another stage's table, or a size taken from the wrong stage.  One
Engine with two samples and every stage on takes one small batch: every table equals its Python model, an add reaches its own table
and no other, and every refusal (wrong size, stage off, a record beyond its text) names the right error and changes nothing.  Every
refusal here is a host-side check that returns before any launch.

The last three tests switch all nine stages on (posttrim, screen and dup besides the six), each in an Engine of its own: what the
stages share on the host beyond a table -- switching off, resetting, installing -- is walked once over every stage there."""
import numpy as np
import pytest

from quade_amd import hip_backend as hb
from quade_amd.screen import canonical_words
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

    def run(self, eng, stage, r1=None, codes=None):
        """the stage's dev_* over the batch (r1: another record table for R1, codes: other routing codes)"""
        a = (self.t1, self.r1 if r1 is None else r1, self.t2, self.r2)
        if stage in ("qstats", "cstats", "filter", "screen", "dup"):
            return getattr(eng, "dev_" + stage)(*a, self.codes if codes is None else codes)
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


# ---- all nine stages on: what they share beyond a table ----
ALL = STAGES + ("posttrim", "screen", "dup")
POST = dict(tail_n=1, poly_x_min_length=6, max_length_r1=0, max_length_r2=0, min_length=0)
DUP = dict(bases=8, sample=1, slots=1 << 10)
SCREEN_K = 15
FILTER_OFF = dict(FM.Params().keywords())  # every rule None, qualified_quality 15
PER_DESTINATION = ("qstats", "filter", "screen", "dup")  # what new barcodes and a new plan switch off
TRIM_GET = dict(adapter_r1=TRIM.adapters[0].decode(), adapter_r2=TRIM.adapters[1].decode(), quality_cutoff=TRIM.quality_cutoff,
                min_overlap=TRIM.min_overlap, max_mismatch_pct=TRIM.max_mismatch_pct, min_length=TRIM.min_length)


def _kmers(batch):
    """a handful of canonical 15-mers of the batch's own reads, ascending"""
    words = [w[ok] for w, ok in (canonical_words(batch.cases[r][j][1], SCREEN_K) for r, j in ((0, 0), (1, 3), (0, 7)))]
    return np.unique(np.concatenate(words))


def _all_on(eng, batch):
    """the six stages as the module's fixture sets them, then posttrim, screen and dup -> what every *_get gives now"""
    kmers = _kmers(batch)
    eng.qstats_enable(True)
    eng.cstats_enable(True)
    eng.clip_set(**CLIP.keywords())
    eng.trim_set(**TRIM_GET)
    eng.pairtrim_set(**PAIR.keywords())
    eng.posttrim_set(**POST)
    eng.filter_set(**FILTER.keywords())
    eng.screen_set(kmer=SCREEN_K, min_hits=1, action="report", kmers=kmers)
    eng.dup_set(**DUP)
    return dict(clip=CLIP.keywords(), trim=TRIM_GET, pairtrim=PAIR.keywords(), posttrim=POST, filter=FILTER.keywords(),
                screen=dict(kmer=SCREEN_K, min_hits=1, action="report", n_kmers=len(kmers)), dup=DUP), kmers


def _gets(eng):
    return {stage: getattr(eng, stage + "_get")() for stage in OFF_GET}


def _read9(eng, stages=ALL):
    """every stage's table, flat; dup's key table as sorted (w1, w2, d, count) rows beside its counters"""
    out = {}
    for stage in stages:
        if stage == "dup":
            keys, counts = eng.dup_read()
            out["dup keys"] = np.array(sorted(tuple(int(x) for x in k) + (int(n),) for k, n in zip(keys, counts)), dtype=np.uint64).reshape(-1, 4)
            out["dup"] = eng.dup_stats().reshape(-1).copy()
        elif stage in BY_ENGINE:
            out[stage] = _read(eng, stage)
        else:
            out[stage] = getattr(eng, stage + "_read")().reshape(-1).copy()
    return out


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), k


def _run9(eng, batch, stages=ALL):
    for stage in stages:
        batch.run(eng, stage)


OFF_GET = dict(clip=dict.fromkeys(CLIP.keywords(), 0), trim=dict(dict.fromkeys(TRIM_GET, 0), adapter_r1="", adapter_r2=""),
               pairtrim=dict.fromkeys(PAIR.keywords(), 0), posttrim=dict.fromkeys(POST, 0), filter=FILTER_OFF, screen=None, dup=None)


def _active(eng, stage):
    return bool(getattr(eng.lib, "qd_%s_active" % stage)(eng._h))


def _off(eng, stage):
    """the stage's table is gone (QD_ERR_STATE) and its parameters are the off values"""
    for call in (eng.dup_stats, eng.dup_read) if stage == "dup" else (getattr(eng, stage + "_read"),):
        with pytest.raises(hb.QuadeHipError) as ei:
            call()
        assert ei.value.code == hb.QD_ERR_STATE, stage
    if stage in OFF_GET:  # (the two reports have neither parameters nor a qd_*_active)
        assert not _active(eng, stage) and getattr(eng, stage + "_get")() == OFF_GET[stage], stage


def test_reset_set_barcodes_and_close_with_every_stage_on():
    batch = Batch()
    with _configured() as eng:
        gets, _ = _all_on(eng, batch)
        _run9(eng, batch)
        first = _read9(eng)
        for k, v in first.items():
            assert v.any(), k  # (the batch moves every table)
        eng.reset_counts()
        zero = _read9(eng)
        assert all(not v.any() for v in zero.values()) and zero["dup keys"].shape == (0, 4)
        assert _gets(eng) == gets and eng.screen_active()
        assert all(_active(eng, stage) for stage in OFF_GET)
        _run9(eng, batch)
        _same(_read9(eng), first)  # the reset left nothing behind and lost no parameter
        kept = tuple(s for s in ALL if s not in PER_DESTINATION)
        want = {k: v for k, v in first.items() if k in kept}
        for change in (lambda: eng.set_barcodes(_barcodes(S)), lambda: eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))):
            change()
            for stage in PER_DESTINATION:
                _off(eng, stage)
            assert eng.filter_get() == FILTER_OFF and not eng.screen_active()
            _same(_read9(eng, kept), want)
            assert {k: v for k, v in _gets(eng).items() if k in kept} == {k: v for k, v in gets.items() if k in kept}
            # every stage on again and run once, so that the second change has the four to switch off
            _all_on(eng, batch)
            _run9(eng, batch)
            _same(_read9(eng), first)
        eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))  # the five on, the four off: closed like this
        assert not eng.screen_active() and eng.clip_active() and eng.posttrim_active()
    with _configured() as fresh:  # the context above went with its tables allocated; a new one works and has every stage off
        for stage in ALL:
            _off(fresh, stage)
        fresh.cstats_enable(True)
        batch.run(fresh, "cstats")
        assert (_read(fresh, "cstats") == first["cstats"]).all()


def test_reset_without_barcodes_zeroes_the_cycle_table_too():
    """reset_counts of a context without barcodes walks the same tables as with them: before the stages' tables stood in one array
    it zeroed the four trimming stages' counters only, and the cycle table (on without plan or barcodes as well) kept its counts."""
    batch = Batch()
    undetermined = np.full(N, CYM.UNDETERMINED, dtype=np.uint16)  # without barcodes the only code there is
    with hb.Engine(0) as eng:
        eng.cstats_enable(True)
        eng.clip_set(tail_clip_r1=1)
        clip = eng.clip_get()
        batch.run(eng, "cstats", codes=undetermined)
        batch.run(eng, "clip")
        assert _read(eng, "cstats").any() and _read(eng, "clip").any()
        eng.reset_counts()
        assert not _read(eng, "cstats").any() and not _read(eng, "clip").any()
        assert eng.clip_get() == clip and clip["tail_clip_r1"] == 1 and eng.clip_active()


def test_a_rejected_set_leaves_every_other_stage_alone():
    batch = Batch()
    with _configured() as eng:
        gets, kmers = _all_on(eng, batch)
        _run9(eng, batch)
        first = _read9(eng)
        bad_sets = (lambda: eng.clip_set(**dict(CLIP.keywords(), front_clip_r1=1001)),
                    lambda: eng.trim_set(**dict(TRIM_GET, quality_cutoff=94)),
                    lambda: eng.pairtrim_set(**dict(PAIR.keywords(), min_overlap=7)),
                    lambda: eng.posttrim_set(**dict(POST, poly_x_min_length=5)),
                    lambda: eng.filter_set(**dict(FILTER.keywords(), max_n=100001)),
                    lambda: eng.screen_set(kmer=14, min_hits=1, action="report", kmers=kmers),
                    lambda: eng.dup_set(**dict(DUP, bases=7)))
        for k, bad in enumerate(bad_sets):
            with pytest.raises(hb.QuadeHipError) as ei:
                bad()
            assert ei.value.code == hb.QD_ERR_INVALID, k
            _same(_read9(eng), first)
            assert _gets(eng) == gets, k
