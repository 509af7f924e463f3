"""The duplication tally on the MI355X (qd_dup_*, quade_amd/csrc/quade_dup.hip): the key table and the per-destination counters
equal tests/dup_model.py's plain Python definition, exactly -- for the stage on its own (qd_dev_dup: every window size and sample
rate, reads at every alignment, both sides of the window's edges, a hot key, distinct keys, both accumulation paths of the
counters, accumulation, state and errors, a table that overflows, tags that collide), through the command line (the report against
the model over the run's own output files, chunk workers, ranks, write flags, the option absent) and beside the six read stages in
one context."""
import os
from collections import Counter

import numpy as np
import pytest

from quade_amd import duplication_report as dr
from quade_amd import filter_report as fr
from quade_amd import hip_backend as hb
from quade_amd import pair_trim_report as pr
from quade_amd import trim_report as tr
from tests import dup_model as DM
from tests import filter_model as FM
from tests import qstats_model as QM
from tests import stage_support as SS
from tests.stage_support import FILTER, P_F, P_PAIR, P_TRIM, TRIMS, _barcodes, _cli, _text_from, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
UND = DM.UNDETERMINED
S_STAGE = 3
SLOTS = 1 << 16
HOT = 3000  # pairs of one key: whole waves of one slot


def _engine(S=S_STAGE, **kw):
    eng = hb.Engine(0)
    eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
    eng.set_barcodes(_barcodes(S))
    if kw:
        eng.dup_set(**kw)
    return eng


def _rs(rng, L, alphabet=b"ACGT"):
    return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))


def _put(s, i, b):
    return s[:i] + b + s[i + 1:]


def _cases(rng, B, n, S):
    """n pairs (code, seq1, seq2, reason).  The first pairs walk through the window's edges; then, room permitting, one key HOT
    times, one sequence pair under two codes, and distinct random pairs; a fifth of all pairs carries a reason byte."""
    codes = list(range(2 * S)) + [UND]
    edge = [(_rs(rng, 151), _rs(rng, 151))]  # (a batch of one pair is a keyed pair)
    for _ in range(3):
        for L in (0, B - 1, B, B + 1, 151):  # every length class in R1 and in R2
            edge.append((_rs(rng, L), _rs(rng, 151)))
            edge.append((_rs(rng, 151), _rs(rng, L)))
            edge.append((_rs(rng, L), _rs(rng, L)))
        for bad in (b"N", b"n", b".", b"\xc1"):  # an invalid byte at the window's first and last base, and just behind it
            for at in (0, B - 1, B):
                a, b = _rs(rng, 60), _rs(rng, 60)
                edge.append((_put(a, at, bad), b))
                edge.append((a, _put(b, at, bad)))
    for _ in range(6):  # lower case is folded: the same key as the upper-case pair beside it
        a, b = _rs(rng, 40), _rs(rng, 40)
        edge.append((a, b))
        edge.append((a.lower(), _rs(rng, 40, b"acgt")))
        edge.append((a.lower(), b.lower()))
    out = [(codes[int(rng.integers(0, len(codes)))], a, b) for a, b in edge]
    if n >= len(out) + HOT + 200:
        a, b = _rs(rng, 151), _rs(rng, 100)
        out += [(2, a, b + _rs(rng, 5))] * 1 + [(2, a, b)] * (HOT - 1)  # (behind the window the reads may differ)
        a, b = _rs(rng, 151), _rs(rng, 151)
        out += [(0, a, b), (1, a, b), (0, a, b), (UND, a, b)]  # one sequence pair under three codes: three keys
    while len(out) < n:  # distinct keys (at B = 8 a few may meet: the model counts them all the same)
        out.append((codes[int(rng.integers(0, len(codes)))], _rs(rng, 151), _rs(rng, 151)))
    out = [out[int(i)] for i in rng.permutation(len(out))][:n] if n >= len(edge) else out[:n]
    return [(c, a, b, int(rng.integers(1, 6)) if rng.integers(0, 5) == 0 else 0) for c, a, b in out]


class Stage(object):
    def __init__(self, seed, B, n, S=S_STAGE, cases=None):
        rng = np.random.default_rng(seed)
        self.S, self.n = S, n
        self.cases = _cases(rng, B, n, S) if cases is None else cases
        self.t1, self.r1 = _text_from(rng, [("", a, b"I" * len(a)) for _, a, _, _ in self.cases])
        self.t2, self.r2 = _text_from(rng, [("", b, b"5" * len(b)) for _, _, b, _ in self.cases])
        self.codes = np.array([c for c, _, _, _ in self.cases], dtype=np.uint16)
        self.drop = np.array([w for _, _, _, w in self.cases], dtype=np.uint8)

    def model(self, P):
        return DM.tally(self.S, self.cases, P)

    def run(self, eng, drop=True):
        eng.dev_dup(self.t1, self.r1, self.t2, self.r2, self.codes, self.drop if drop else None)


def _device(eng):
    keys, counts = eng.dup_read()
    assert keys.dtype == np.uint64 and keys.shape == (len(counts), 3)
    return DM.table_counter(keys, counts), eng.dup_stats()


def _check_exact(eng, model, model_stats):
    assert DM.no_shared_tags(model.keys())  # so that not_tallied == 0 is a fact about the input
    table, stats = _device(eng)
    DM.check_exact(table, stats, model, model_stats)


# ---- the stage against the model ---------------------------------------------------------------------------------------------------
def test_the_generated_input_holds_the_cases():
    st = Stage(1, 32, 5000)
    starts = {int(q[3] + 3) % 16 for q in st.r1 if q[4] >= 32} & {int(q[3] + 3) % 16 for q in st.r2 if q[4] >= 32}
    assert starts == set(range(16)) and b"\r\n" in st.t1 and b"\r\n" in st.t2  # every alignment of the window, CRLF line ends
    table, stats = st.model(DM.Params(32, 1, SLOTS))
    tot = [sum(col) for col in zip(*stats)]
    assert 0.15 * st.n < st.n - tot[DM.PAIRS] < 0.25 * st.n  # a fifth carries a reason byte
    assert tot[DM.SHORT] > 5 and tot[DM.WITH_N] > 5 and max(table.values()) > 0.7 * HOT and len(table) > 1000
    assert all(r[DM.PAIRS] > 0 for r in stats)
    lens = {(len(a), len(b)) for _, a, b, _ in st.cases}
    assert {(0, 151), (31, 151), (32, 151), (33, 151), (151, 0), (151, 31), (0, 0), (32, 32), (33, 33)} <= lens
    by_seq = {}  # one sequence pair under several codes: as many keys
    for c, a, b, w in st.cases:
        if not w and len(a) == 151 and len(b) == 151:
            by_seq.setdefault((a, b), set()).add(c)
    assert any(len(cs) >= 2 and all(table[(DM.word(a, 32), DM.word(b, 32), DM.dest(c, st.S))] >= 1 for c in cs) for (a, b), cs in by_seq.items())


@pytest.mark.parametrize("sample", [1, 4])
@pytest.mark.parametrize("B", [8, 31, 32])
@pytest.mark.parametrize("n", [1, 255, 5000])
def test_stage_equals_the_model(torch_cuda, n, B, sample):
    st = Stage(100 + n + B, B, n)
    P = DM.Params(B, sample, SLOTS)
    model, model_stats = st.model(P)
    with _engine(**P.keywords()) as eng:
        assert eng.dup_get() == P.keywords()
        st.run(eng)
        _check_exact(eng, model, model_stats)
    if n == 5000:  # a wave full of one slot, distinct keys, and the sample a strict part of the keys
        full = st.model(DM.Params(B, 1, SLOTS))[0]
        assert max(full.values()) > 0.7 * HOT and len(full) > 1000
        assert (model == full) if sample == 1 else (0.1 * len(full) < len(model) < 0.5 * len(full))


@pytest.mark.parametrize("drop", [True, False])
def test_the_reason_bytes_are_optional(torch_cuda, drop):
    st = Stage(7, 16, 600)
    cases = st.cases if drop else [(c, a, b, 0) for c, a, b, _ in st.cases]
    model, model_stats = DM.tally(st.S, cases, DM.Params(16, 1, SLOTS))
    with _engine(bases=16, sample=1, slots=SLOTS) as eng:
        st.run(eng, drop=drop)
        _check_exact(eng, model, model_stats)
    assert sum(r[0] for r in model_stats) == (600 if not drop else 600 - int((st.drop != 0).sum()))


@pytest.mark.parametrize("S", [1, 1023, 1024])
def test_stage_sample_counts_and_both_sides_of_the_lds_limit(torch_cuda, S):
    """S = 1023: the counters' 32-bit partials in LDS (2047 destinations); S = 1024: merged global atomics.  The pairs go to the
    last 41 destinations, in runs of equal codes so that the wave's rows meet"""
    st = Stage(40 + S, 32, 1500, S=S)
    rng = np.random.default_rng(S)
    codes = rng.integers(max(0, 2 * S - 40), 2 * S + 1, st.n)
    for a in rng.integers(0, st.n - 8, 100):
        codes[a:a + 5] = codes[a]
    codes[codes == 2 * S] = UND
    st.codes = codes.astype(np.uint16)
    st.cases = [(int(c), a, b, w) for c, (_, a, b, w) in zip(st.codes, st.cases)]
    P = DM.Params(32, 1, SLOTS)
    model, model_stats = st.model(P)
    with _engine(S, **P.keywords()) as eng:
        st.run(eng)
        _check_exact(eng, model, model_stats)
    used = [d for d, r in enumerate(model_stats) if r[0]]
    assert len(used) == min(41, 2 * S + 1) and min(used) == max(0, 2 * S - 40)


# ---- accumulation and state --------------------------------------------------------------------------------------------------------
def test_two_calls_equal_the_model_of_their_union_and_reset(torch_cuda):
    a, b = Stage(20, 24, 900), Stage(21, 24, 333)
    b.cases[:50] = a.cases[:50]  # keys of the first call come again in the second
    b = Stage(21, 24, 333, cases=b.cases)
    P = DM.Params(24, 2, SLOTS)
    with _engine(**P.keywords()) as eng:
        a.run(eng)
        _check_exact(eng, *a.model(P))
        b.run(eng)
        model, model_stats = DM.tally(S_STAGE, a.cases + b.cases, P)
        _check_exact(eng, model, model_stats)
        assert any(model[k] > a.model(P)[0][k] > 0 for k in model)
        eng.reset_counts()  # both tables empty, the stage still on
        table, stats = _device(eng)
        assert table == Counter() and not stats.any() and eng.dup_get() == P.keywords()
        b.run(eng)
        _check_exact(eng, *b.model(P))


def test_a_growing_second_call_equals_the_model_of_the_union(torch_cuda):
    """333 pairs, then 5 000: the second call's batch list is more than twice the first's, so the stream's list is freed and allocated
    again behind the first call's kernels; the key table and the counters carry over."""
    a, b = Stage(22, 24, 333), Stage(23, 24, 5000)
    b.cases[:50] = a.cases[:50]  # keys of the first call come again in the second
    b = Stage(23, 24, 5000, cases=b.cases)
    P = DM.Params(24, 2, SLOTS)
    with _engine(**P.keywords()) as eng:
        a.run(eng)
        b.run(eng)
        model, model_stats = DM.tally(S_STAGE, a.cases + b.cases, P)
        _check_exact(eng, model, model_stats)  # (sampled == tallied + not_tallied per destination is part of it)
        assert any(model[k] > a.model(P)[0][k] > 0 for k in model)


def test_state_and_errors(torch_cuda):
    st = Stage(30, 32, 64)
    P = DM.Params(32, 1, 1 << 12)
    with hb.Engine(0) as eng:
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dup_set(**P.keywords())  # no plan, no barcodes: the counters have a row per destination
        assert ei.value.code == hb.QD_ERR_STATE
        eng.dup_set(on=False)  # nothing to turn off: accepted
        eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        eng.set_barcodes(_barcodes(S_STAGE))
        assert eng.dup_get() is None
        for call in (eng.dup_stats, eng.dup_read, lambda: st.run(eng)):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        eng.dup_set(**P.keywords())
        st.run(eng)
        model, model_stats = st.model(P)
        _check_exact(eng, model, model_stats)
        for bad in (dict(bases=7), dict(bases=33), dict(bases=0), dict(sample=0), dict(sample=3), dict(sample=2048), dict(sample=-4),
                    dict(slots=512), dict(slots=3000), dict(slots=1 << 29), dict(slots=0)):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.dup_set(**dict(P.keywords(), **bad))
            assert ei.value.code == hb.QD_ERR_INVALID, bad
            assert eng.dup_get() == P.keywords()  # a rejected call changes nothing: not the parameters, not the tables
        _check_exact(eng, model, model_stats)
        for size in (34, 36, 5):
            out = np.zeros(size, dtype=np.uint64)
            assert eng.lib.qd_dup_stats(eng._h, hb._ptr(out), size) == hb.QD_ERR_INVALID
        assert eng.lib.qd_dup_read(eng._h, None, None, 0) == -len(model)  # the sizing call
        # a bad table never becomes an address: refused on the host, nothing launched, the tables as they were
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_dup(st.t1, bad, st.t2, st.r2, st.codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        c2 = st.codes.copy()
        c2[9] = 2 * S_STAGE
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_dup(st.t1, st.r1, st.t2, st.r2, c2)
        assert ei.value.code == hb.QD_ERR_INVALID
        _check_exact(eng, model, model_stats)
        eng.dup_set(on=False)  # off: both tables are freed and later calls count nothing
        assert eng.dup_get() is None and eng.lib.qd_dup_set(eng._h, None) == 0
        for call in (eng.dup_stats, eng.dup_read, lambda: st.run(eng)):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        eng.dup_set(**P.keywords())
        table, stats = _device(eng)
        assert table == Counter() and not stats.any()
        st.run(eng)
        eng.set_barcodes(_barcodes(S_STAGE + 1))  # new barcodes turn the stage off, as they do the read filter
        assert eng.dup_get() is None
        eng.dup_set(**P.keywords())
        assert eng.dup_stats().shape == (2 * S_STAGE + 3, 5) and not eng.dup_stats().any()
        eng.set_plan(hb.make_plan(True, 20, (0, 8), (0, 8)))  # and so does a new plan
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dup_read()
        assert ei.value.code == hb.QD_ERR_STATE


# ---- a table that cannot hold every key --------------------------------------------------------------------------------------------
def _distinct(seed, n, S=S_STAGE):
    rng = np.random.default_rng(seed)
    codes = list(range(2 * S)) + [UND]
    cases = [(codes[int(rng.integers(0, len(codes)))], _rs(rng, 40), _rs(rng, 40), 0) for _ in range(n)]
    cases += cases[:n // 3]  # a third of the keys twice
    return Stage(seed, 32, len(cases), S=S, cases=cases)


def test_overflow(torch_cuda):
    """3 000 distinct keys into 1 024 slots: the table fills, every entry present is exact, the others' pairs are not_tallied"""
    st = _distinct(50, 3000)
    P = DM.Params(32, 1, 1024)
    model, model_stats = st.model(P)
    assert len(model) == 3000 and DM.no_shared_tags(model.keys())
    with _engine(**P.keywords()) as eng:
        st.run(eng)
        table, stats = _device(eng)
    assert len(table) == 1024
    DM.check_lossy(table, stats, model, model_stats)
    assert sum(int(r[DM.NOT_TALLIED]) for r in stats) == sum(c for k, c in model.items() if k not in table) >= 1976


def test_tag_collisions(torch_cuda):
    """dup_tag_bits 6: 400 distinct keys share 63 tags.  One key per tag owns the entry, the others are not_tallied"""
    st = _distinct(51, 400)
    P = DM.Params(32, 1, SLOTS)
    model, model_stats = st.model(P)
    tags = {DM.trim(DM.key_hash(k), 6) for k in model}
    assert len(model) == 400 and len(tags) <= 63
    with _engine(**P.keywords()) as eng:
        eng.set_option("dup_tag_bits", 6)
        st.run(eng)
        table, stats = _device(eng)
        assert len(table) == len(tags) and {DM.trim(DM.key_hash(k), 6) for k in table} == tags
        DM.check_lossy(table, stats, model, model_stats)
        eng.set_option("dup_tag_bits", 64)
        eng.reset_counts()
        st.run(eng)
        _check_exact(eng, model, model_stats)
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.set_option("dup_tag_bits", 0)
        assert ei.value.code == hb.QD_ERR_INVALID


# ---- the pipeline through the command line -----------------------------------------------------------------------------------------
N_CHUNK = 600
_SEEN = {}


def _dup_inserts(g, i, sample, kind):
    """the filter tests' insert reads; about a third of the pairs repeats the reads of an earlier pair of its destination (the
    same sample; an unknown index, a low index quality or a good one), also one of the chunk before"""
    where = (sample, 0 if kind == 0 else 1 if kind in (2, 3) else 2)
    seen = _SEEN.setdefault(where, [])
    if seen and g.rng.integers(0, 3) == 0:
        return seen[int(g.rng.integers(0, len(seen)))]
    seen.append(SS._filter_inserts(g, i, sample, kind))
    return seen[-1]


def _write_conf(path, files, samples, sample=1, report=True, extra=TRIMS + FILTER, gpu="", **kw):
    SS._write_conf(path, files, samples, extra=extra, gpu="duplicate_slots : %d\n" % SLOTS + gpu, **kw)
    if report:
        text = SS._read(path).replace("[output]\n", "[output]\nduplication_report : True\nduplication_sample : %d\n" % sample, 1)
        open(path, "w").write(text)


def _model_from_outputs(outdir, samples, P):
    """the model over the records of a run's own output files -> (Counter, stats)"""
    names = [s[0] for s in samples]
    stems = [n + q for n in names for q in ("_pass", "_fail")] + ["Undetermined"]
    pairs = []
    for d, stem in enumerate(stems):
        p1, p2 = (os.path.join(str(outdir), stem + r + ".fastq.gz") for r in ("_R1", "_R2"))
        if os.path.exists(p1):
            r1, r2 = QM.fastq_records(p1), QM.fastq_records(p2)
            assert len(r1) == len(r2)
            pairs += [(UND if d == 2 * len(names) else d, a[0], b[0], 0) for a, b in zip(r1, r2)]
    return DM.tally(len(names), pairs, P)


def _report(outdir):
    return SS._read(os.path.join(str(outdir), dr.REPORT_NAME))


def _want(run, sample):
    table, stats = _model_from_outputs(run["mine"], run["samples"], DM.Params(32, sample, SLOTS))
    keys, counts = DM.arrays(table)
    return "\n".join(dr.report_lines(stats, keys, counts, [s[0] for s in run["samples"]], dict(bases=32, sample=sample, slots=SLOTS))) + "\n", table, stats


@pytest.fixture(scope="module")
def cli_run(torch_cuda, tmp_path_factory):
    """2 chunks x 600 pairs in BGZF behind [trim] and [filter], run once with the report on (sample 1); the files against the
    oracle's outputs trimmed and filtered by the models"""
    top = tmp_path_factory.mktemp("dup_cli")
    _SEEN.clear()
    files, samples = SS._dataset(str(top / "data"), 81, 2, N_CHUNK, True, _dup_inserts, SS._same_places, sample_first=True)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples, report=False, extra="")
    SS._oracle_run(plain, top / "ref")
    texts, ftable, first, second = FM.filtered_outputs(str(top / "ref"), [s[0] for s in samples], P_F, P_TRIM, P_PAIR)
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    _cli(conf, top / "mine")
    SS._check_files(top / "mine", texts)
    return dict(top=top, files=files, samples=samples, texts=texts, mine=top / "mine", ftable=ftable, first=first, second=second)


def test_cli_report_equals_the_model_over_the_outputs(cli_run):
    run = cli_run
    want, table, stats = _want(run, 1)
    assert _report(run["mine"]) == want
    tot = [sum(col) for col in zip(*stats)]
    pairs, tallied = tot[DM.PAIRS], sum(table.values())
    assert 300 < pairs < 2 * N_CHUNK and 0.2 * tallied < tallied - len(table) < 0.5 * tallied  # about a third repeats an earlier pair
    assert max(table.values()) >= 3 and tot[DM.NOT_TALLIED] == 0 and tot[DM.SAMPLED] == tallied
    SS._check_report(run["mine"], fr, run["ftable"], [s[0] for s in run["samples"]], P_F.keywords())


def test_cli_sample_4(cli_run, tmp_path):
    run = cli_run
    conf = tmp_path / "s4.txt"
    _write_conf(conf, run["files"], run["samples"], sample=4)
    _cli(conf, tmp_path / "s4")
    SS._check_files(tmp_path / "s4", run["texts"])
    want, table, stats = _want(run, 4)
    assert _report(tmp_path / "s4") == want != _report(run["mine"])
    full = _want(run, 1)[1]
    assert 0 < len(table) < 0.6 * len(full) and all(full[k] == c for k, c in table.items())


def test_cli_chunk_workers_ranks_and_write_flags(cli_run, tmp_path):
    """the report does not depend on who counted: two chunk workers (two contexts merged by key), two ranks (merged through the
    rendezvous files), and Undetermined not written (it is counted all the same)"""
    run = cli_run
    want = _report(run["mine"])
    conf = tmp_path / "workers.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="chunk_workers : 2\n")
    _cli(conf, tmp_path / "workers")
    assert _report(tmp_path / "workers") == want
    SS._check_files(tmp_path / "workers", run["texts"])
    conf = tmp_path / "ranks.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : False\n")
    _cli(conf, tmp_path / "ranks", ranks=2)
    assert _report(tmp_path / "ranks") == want
    assert not [f for f in os.listdir(tmp_path / "ranks") if f.startswith(".quade_rdv")]
    conf = tmp_path / "flags.txt"
    _write_conf(conf, run["files"], run["samples"], flags=(True, True, False))
    _cli(conf, tmp_path / "flags")
    assert _report(tmp_path / "flags") == want and "Undetermined_R1.fastq.gz" in run["texts"]
    SS._check_files(tmp_path / "flags", run["texts"], only=lambda f: not f.startswith("Undetermined"))


def test_cli_without_the_option_nothing_changes(cli_run, tmp_path):
    run = cli_run
    for name, lines in (("absent", ""), ("false", "duplication_report : False\nduplication_sample : 4\n"), ("empty", "duplication_report :\n")):
        conf = tmp_path / (name + ".txt")
        _write_conf(conf, run["files"], run["samples"], report=False)
        text = SS._read(conf).replace("[output]\n", "[output]\n" + lines, 1)
        open(conf, "w").write(text)
        _cli(conf, tmp_path / name)
        assert not os.path.exists(tmp_path / name / dr.REPORT_NAME)
        mine, other = sorted(os.listdir(run["mine"])), sorted(os.listdir(tmp_path / name))
        assert [f for f in mine if f != dr.REPORT_NAME] == other and len(other) > 12
        for f in other:  # the fastq files byte for byte, the compressed bytes included, and the other stages' reports
            a, b = (open(os.path.join(str(d), f), "rb").read() for d in (run["mine"], tmp_path / name))
            if f == "Quade_report.csv":
                a, b = a.split(b"\n", 1)[1], b.split(b"\n", 1)[1]  # (behind the dated first line)
            assert a == b, f
        assert {fr.REPORT_NAME, tr.REPORT_NAME, pr.REPORT_NAME} <= set(other)


# ---- beside the six read stages in one context -------------------------------------------------------------------------------------
def test_all_stages_in_one_context(torch_cuda):
    """one context with the six read stages and the tally on, one without the tally: the same calls leave the same six tables,
    and the tally's own tables are the model's -- no call reaches another stage's table"""
    st = Stage(60, 16, 300, S=2)
    P = DM.Params(16, 1, 1 << 10)
    model, model_stats = st.model(P)

    def six(eng):
        eng.qstats_enable(True)
        eng.cstats_enable(True)
        eng.clip_set(front_clip_r1=1, tail_clip_r2=2, window_size=4, window_quality=20, poly_g_min_length=6, min_length=5)
        eng.trim_set("AGATCGGAAG", "AGATCGGAAG", 20, 3, 10, 4)
        eng.pairtrim_set(min_overlap=8, max_mismatches=2, max_mismatch_pct=20, min_length=6)
        eng.filter_set(min_length=18, max_n=1)

    def run_six(eng):
        a = (st.t1, st.r1, st.t2, st.r2)
        eng.dev_qstats(*a, st.codes)
        eng.dev_cstats(*a, st.codes, st.drop)
        eng.dev_clip(*a)
        eng.dev_trim(*a)
        eng.dev_pairtrim(*a)
        eng.dev_filter(*a, st.codes)

    def tables(eng):
        return {s.engine: np.asarray(s.read(eng)).reshape(-1).copy() for s in hb.STAGES}

    with _engine(2) as plain, _engine(2) as eng:
        six(plain)
        run_six(plain)
        want = tables(plain)
        assert len(want) == 6 and all(t.any() for t in want.values())
        six(eng)
        eng.dup_set(**P.keywords())
        run_six(eng)
        st.run(eng)
        got = tables(eng)
        for name in want:
            assert got[name].shape == want[name].shape and (got[name] == want[name]).all(), name
        _check_exact(eng, model, model_stats)
        eng.filter_add(np.ones(want["filter"].size, dtype=np.uint64))  # another stage's add leaves the tally alone, and the reverse
        _check_exact(eng, model, model_stats)
        st.run(eng)
        got = tables(eng)
        assert (got["filter"] == want["filter"] + np.uint64(1)).all() and all((got[k] == want[k]).all() for k in want if k != "filter")
        with pytest.raises(hb.QuadeHipError) as ei:
            plain.dev_dup(st.t1, st.r1, st.t2, st.r2, st.codes)
        assert ei.value.code == hb.QD_ERR_STATE
