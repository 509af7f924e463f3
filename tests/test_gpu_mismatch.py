"""Mismatch-tolerant matching on the MI355X: routing codes, molecular bytes and counters equal to the oracle with the tolerant
lookup of tests/mismatch_model.py installed (qo.SampleSet monkeypatched; the oracle itself is unmodified), on every path that
launches the match kernels: fast and generic kernels, ragged batches, pinned slots, and the command line's device pipeline; and, on
tight and combinatorial sheets, equal to the brute-force model of tests/mismatch_model.py on every key within budget of a barcode
and on the keys one substitution too far (tests/mismatch_support.py; tests/test_host_mismatch.py pins that model to the oracle)."""
import gzip
import os

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from quade_amd import synth
from tests import helpers as H
from tests import mismatch_model as MM
from tests import mismatch_support as MS
from tests.mismatch_support import SHAPES, make_reads, rows_on_device, sheet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch


@pytest.fixture(scope="module")
def engine(torch_cuda):
    with hb.Engine(0) as e:
        yield e


def tolerant_oracle(monkeypatch, shape, bcs, streams, m1, m2):
    plan, (w1, w2), _ = SHAPES[shape]
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, w1 + w2, w1, m1, m2))
    reads = []
    for s, q in streams:
        reads += [[x.decode() for x in s], [x.decode() for x in q]]
    if len(streams) == 1:
        reads += [None, None]
    return H.oracle_on_reads(bcs, plan, *reads)


def setup(engine, shape, bcs, m1, m2, kernel=0):
    engine.set_plan(SHAPES[shape][0])
    engine.set_barcodes(bcs)
    engine.set_option("kernel", kernel)
    engine.set_mismatches(m1, m2)


def check(engine, torch, streams, want, n, lens=None):
    codes_o, _, mol_o, counts_o = want
    seq, qual, lrows, _ = rows_on_device(torch, engine.layout, streams)
    engine.reset_counts()
    codes, mol = H.hip_on_device(engine, seq, qual, n, lens=lrows if lens else None)
    assert (codes == codes_o[:n]).all(), np.flatnonzero(codes != codes_o[:n])[:10]
    if engine.layout.mol_width:
        assert H.mol_rows_to_str(mol) == mol_o[:n]
    return engine.counts()


CASES = [("single8", 1, 0), ("single8", 2, 0), ("dual8", 1, 0), ("dual8", 0, 1), ("dual8", 1, 1), ("dual8", 2, 2),
         ("wide10", 1, 1), ("kit6", 1, 1), ("kit8u9", 1, 1)]


@pytest.mark.parametrize("shape,m1,m2", CASES)
def test_shapes_fast_and_generic(torch_cuda, engine, monkeypatch, shape, m1, m2):
    S = 12 if shape == "single8" and m1 == 2 else (24 if 2 in (m1, m2) else 64)  # a single 8-base read holds few codes at distance 5
    bcs = sheet(shape, S, m1, m2)
    n = 4097
    streams = make_reads(shape, bcs, n, m1, m2, seed=100 + CASES.index((shape, m1, m2)))
    want = tolerant_oracle(monkeypatch, shape, bcs, streams, m1, m2)
    codes_o, counts_o = want[0], want[3]
    for kernel in (1, 2):
        setup(engine, shape, bcs, m1, m2, kernel)
        counts = check(engine, torch_cuda, streams, want, n)
        assert (counts == counts_o).all(), (kernel, counts, counts_o)
    # the budgets rescue pairs on both sides of the quality gate
    engine.set_mismatches(0, 0)
    engine.reset_counts()
    seq, qual, _, _ = rows_on_device(torch_cuda, engine.layout, streams)
    codes0, _ = H.hip_on_device(engine, seq, qual, n)
    moved = (codes0 == 0xFFFF) & (codes_o != 0xFFFF)
    rescued_pass, rescued_fail = int((moved & (codes_o % 2 == 0)).sum()), int((moved & (codes_o % 2 == 1)).sum())
    assert rescued_pass > 0 and rescued_fail > 0
    assert ((codes0 == codes_o) | moved).all()  # exact hits keep their codes


def test_batch_sizes(torch_cuda, engine, monkeypatch):
    bcs = sheet("dual8", 96, 1, 1)
    N = 70003
    streams = make_reads("dual8", bcs, N, 1, 1, seed=5)
    want = tolerant_oracle(monkeypatch, "dual8", bcs, streams, 1, 1)
    prefix_counts = {n: tolerant_oracle(monkeypatch, "dual8", bcs, [(s[:n], q[:n]) for s, q in streams], 1, 1)[3]
                     for n in (1, 511, 4097)}
    prefix_counts[N] = want[3]
    for kernel in (1, 2):
        setup(engine, "dual8", bcs, 1, 1, kernel)
        for n in (0, 1, 511, 4097, N):
            if n == 0:
                engine.reset_counts()
                H.hip_on_device(engine, *rows_on_device(torch_cuda, engine.layout, [(s[:1], q[:1]) for s, q in streams])[:2], 0)
                assert not engine.counts().any()
                continue
            counts = check(engine, torch_cuda, [(s[:n], q[:n]) for s, q in streams], want, n)
            assert (counts == prefix_counts[n]).all(), (kernel, n)


def test_ragged_batches(torch_cuda, engine, monkeypatch):
    """short reads (cut inside the barcode slice) match exactly only; the rest of the batch is rescued"""
    bcs = sheet("dual8", 96, 1, 1)
    n = 20011
    streams = make_reads("dual8", bcs, n, 1, 1, seed=9, short_frac=0.1)
    want = tolerant_oracle(monkeypatch, "dual8", bcs, streams, 1, 1)
    setup(engine, "dual8", bcs, 1, 1)
    seq, qual, lens, full = rows_on_device(torch_cuda, engine.layout, streams)
    assert not full
    short = np.flatnonzero(np.array([len(streams[0][0][r]) < 8 or len(streams[1][0][r]) < 8 for r in range(n)])).astype(np.uint32)
    sidx = torch_cuda.from_numpy(short).cuda()
    for ragged in (True, False):
        engine.reset_counts()
        codes = torch_cuda.full((n,), 0x7777, dtype=torch_cuda.int16, device="cuda")
        st = torch_cuda.cuda.current_stream().cuda_stream
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        if ragged:
            engine.demux_device_ragged(n, ptr(seq), ptr(qual), codes.data_ptr(), None, ptr(lens), short.size, sidx.data_ptr(), stream=st)
        else:  # len rows for every pair: the generic kernel
            engine.demux_device(n, ptr(seq), ptr(qual), codes.data_ptr(), None, lens=ptr(lens), stream=st)
        torch_cuda.cuda.synchronize()
        c = codes.cpu().numpy().view(np.uint16)
        assert (c == want[0]).all(), (ragged, np.flatnonzero(c != want[0])[:10])
        assert (engine.counts() == want[3]).all()


def test_pinned_slots(torch_cuda, monkeypatch):
    bcs = sheet("kit8u9", 96, 1, 1)
    n = 9001
    streams = make_reads("kit8u9", bcs, n, 1, 1, seed=13)
    codes_o, _, mol_o, counts_o = tolerant_oracle(monkeypatch, "kit8u9", bcs, streams, 1, 1)
    with hb.Engine(0) as eng:
        setup(eng, "kit8u9", bcs, 1, 1)
        eng.slots_create(2, 4096)
        L = eng.layout
        got_codes, got_mol = [], []
        for i, a in enumerate(range(0, n, 4096)):
            b = min(n, a + 4096)
            v = eng.slot(i % 2)
            if i >= 2:
                eng.wait(i % 2)
            for k, (s, q) in enumerate(streams):
                sr, qr, _, _ = hb.pack_index_reads(L, k, s[a:b], q[a:b])
                v["seq"][k][:b - a] = sr
                v["qual"][k][:b - a] = qr
            eng.submit(i % 2, b - a)
            eng.wait(i % 2)
            got_codes.append(v["codes"][:b - a].copy())
            got_mol.append(v["mol"][:b - a].copy())
        codes = np.concatenate(got_codes)
        assert (codes == codes_o).all()
        assert H.mol_rows_to_str(np.concatenate(got_mol)) == mol_o
        assert (eng.counts() == counts_o).all()
        eng.slots_destroy()


@pytest.mark.parametrize("S", [1536, 8192])
def test_large_sheets(torch_cuda, engine, monkeypatch, S):
    bcs = sheet("dual8", S, 1, 1, seed=S)
    n = 12007
    streams = make_reads("dual8", bcs, n, 1, 1, seed=S + 1)
    want = tolerant_oracle(monkeypatch, "dual8", bcs, streams, 1, 1)
    for kernel in (0, 2):
        setup(engine, "dual8", bcs, 1, 1, kernel)
        assert (check(engine, torch_cuda, streams, want, n) == want[3]).all()


def test_api_state_and_resets(torch_cuda, monkeypatch):
    bcs = sheet("dual8", 32, 1, 1)
    with hb.Engine(0) as eng:
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.set_mismatches(1, 1)
        assert ei.value.code == hb.QD_ERR_STATE
        eng.set_plan(SHAPES["dual8"][0])
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.set_mismatches(1, 1)
        assert ei.value.code == hb.QD_ERR_STATE
        eng.set_barcodes(bcs)
        for bad in ((3, 0), (0, -1)):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.set_mismatches(*bad)
            assert ei.value.code == hb.QD_ERR_INVALID
        # a colliding sheet: the first pair named
        coll = list(bcs)
        coll[5] = coll[2][:3] + ("A" if coll[2][3] != "A" else "C") + coll[2][4:]
        eng.set_barcodes(coll)
        first = MM.first_collision(coll, 16, 8, 1, 1)
        assert first is not None and first[1] == 5
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.set_mismatches(1, 1)
        assert ei.value.code == hb.QD_ERR_BARCODE and "barcodes %d and %d collide" % first in str(ei.value)
        # single index: m2 must be 0
        eng.set_plan(SHAPES["single8"][0])
        eng.set_barcodes([b[:8] for b in bcs[:8]])
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.set_mismatches(1, 1)
        assert ei.value.code == hb.QD_ERR_INVALID
        # budgets reset by set_plan / set_barcodes: today's exact codes again
        n = 3001
        streams = make_reads("dual8", bcs, n, 1, 1, seed=21)
        exact = tolerant_oracle(monkeypatch, "dual8", bcs, streams, 0, 0)
        tol = tolerant_oracle(monkeypatch, "dual8", bcs, streams, 1, 1)
        assert (exact[0] != tol[0]).any()
        for reset in ("plan", "barcodes", "zero"):
            setup(eng, "dual8", bcs, 1, 1)
            assert (check(eng, torch_cuda, streams, tol, n) == tol[3]).all()
            if reset == "plan":
                eng.set_plan(SHAPES["dual8"][0])
                eng.set_barcodes(bcs)
            elif reset == "barcodes":
                eng.set_barcodes(bcs)
            else:
                eng.set_mismatches(0, 0)  # (0, 0) set explicitly: today's codes
            assert (check(eng, torch_cuda, streams, exact, n) == exact[3]).all()


# ---- tight and combinatorial sheets: every key within budget, and the keys one substitution too far, against the model ---------
def _launch(engine, torch, dev, n, mode, short=None):
    """one launch over the first n pairs of the rows on the device (plain: whole rows; lens: a length per read, the generic
    kernel; ragged: the short pairs listed) behind a counter reset -> (codes, molecular rows, counters)"""
    seq, qual, lens = dev
    engine.reset_counts()
    if mode != "ragged":
        codes, mol = H.hip_on_device(engine, seq, qual, n, lens=lens if mode == "lens" else None)
        return codes, mol, engine.counts()
    M = engine.layout.mol_width
    codes = torch.full((max(n, 1),), 0x7777, dtype=torch.int16, device="cuda")
    mol = torch.full((max(n, 1), max(M, 1)), 0x55, dtype=torch.uint8, device="cuda")
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    engine.demux_device_ragged(n, ptr(seq), ptr(qual), codes.data_ptr(), mol.data_ptr() if M else None, ptr(lens), short.numel(),
                               short.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return codes.cpu().numpy().view(np.uint16)[:n], (mol.cpu().numpy()[:n] if M else None), engine.counts()


def _same(got, want, c, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (c.name, what, bad.size, [(int(r), c.keys[r].tobytes(), c.sheet[c.origin[r]], hex(int(got[r])), hex(int(want[r])))
                                                   for r in bad[:5]])


def _corpus_against_the_model(torch, engine, c):
    """the corpus's reads under every kernel the plan has: codes and counters equal the model's on every pair; and without
    budgets exactly the pairs that the model rescues are Undetermined"""
    engine.set_plan(c.shape.plan)
    engine.set_barcodes(c.sheet)
    seq, qual, lens, full = rows_on_device(torch, engine.layout, c.streams)
    assert full == (not c.short.any())
    short = None if full else torch.from_numpy(np.flatnonzero(c.short).astype(np.uint32)).cuda()
    modes = ("plain",) if full else ("ragged", "lens")
    want_mol = None
    if engine.layout.mol_width:
        want_mol = np.frombuffer(b"".join(c.molecular()), np.uint8).reshape(c.n, engine.layout.mol_width)
    engine.set_option("kernel", 0)
    has_fast = engine.kernel_kind() == "fast"
    try:
        for kernel in (0, 2) + ((1,) if has_fast else ()):
            engine.set_option("kernel", kernel)
            engine.set_mismatches(c.m1, c.m2)
            assert engine.kernel_kind() == ("generic" if kernel == 2 or not has_fast else "fast")
            for mode in modes:
                assert mode != "lens" or engine.kernel_kind(has_len=True) == "generic"
                codes, mol, counts = _launch(engine, torch, (seq, qual, lens), c.n, mode, short)
                _same(codes, c.codes, c, (kernel, mode))
                assert (counts == c.counts()).all(), (c.name, kernel, mode)
                if want_mol is not None:  # the molecular bytes are the reads' slice, and rescued pairs keep them
                    assert (mol == want_mol).all() and (mol[c.rescued] == want_mol[c.rescued]).all() and c.rescued.any()
            engine.set_mismatches(0, 0)
            for mode in modes:
                codes, _, counts = _launch(engine, torch, (seq, qual, lens), c.n, mode, short)
                _same(codes, c.exact, c, (kernel, mode, "no budgets"))
                assert (codes[c.rescued] == 0xFFFF).all() and (counts == c.counts(c.exact)).all()
    finally:
        engine.set_option("kernel", 0)


@pytest.mark.parametrize("name", sorted(MS.CORPORA))
def test_neighbourhoods_equal_the_model(torch_cuda, engine, name):
    """Sheets as tight as the collision rule allows, whose samples share whole parts (candidate lists longer than one), with
    every key within budget of every barcode and a sample of the keys one substitution too far (tests/test_host_mismatch.py
    holds the corpora to their conditions and the model to the oracle).  Slices at an offset, parts of unequal width, unequal
    budgets, barcodes with N, barcodes of several lengths, and a sheet past the per-workgroup histogram are among them."""
    _corpus_against_the_model(torch_cuda, engine, MS.corpus(name))


@pytest.mark.parametrize("shape", sorted(MS.NO_SEGMENTS))
def test_the_branch_without_segments(torch_cuda, engine, shape):
    """parts narrower than budget + 1: no pigeonhole, the rescue compares with every barcode.  One sample and all 5^K keys: every
    full-length key is its sample's, pass or fail by the gate; the same keys in reads cut inside the slice stay Undetermined"""
    c = MS.no_segments_corpus(shape)
    gate_fails = (c.quals.astype(np.int64) - 33 < c.shape.plan.min_qual).any(axis=1)
    assert (c.codes[~c.short] == gate_fails[~c.short]).all() and (c.codes[c.short] == 0xFFFF).all()
    assert c.short.sum() == (~c.short).sum() == 4 * 5 ** c.K and gate_fails[~c.short].any() and not gate_fails[~c.short].all()
    _corpus_against_the_model(torch_cuda, engine, c)


def test_compact_boundaries(torch_cuda, engine):
    """mm_compact lists 8 codes per lane step and 32 768 per workgroup: batches that end just before, at and just behind both,
    all to be rescued, none (every pair exact), and all listed but none rescued (every pair unrelated)"""
    c = MS.corpus("comb_8x12")
    rng = np.random.default_rng(3)
    N, plan = 32769, c.shape.plan
    engine.set_plan(plan)
    engine.set_barcodes(c.sheet)
    batches = {}
    for what, rows in (("one off", np.flatnonzero(c.d1 + c.d2 == 1)), ("exact", np.flatnonzero(c.d1 + c.d2 == 0))):
        pick = rng.choice(rows, N, replace=True)
        batches[what] = ([([s[r] for r in pick], [q[r] for r in pick]) for s, q in c.streams], c.codes[pick])
    keys = MS.ACGT[rng.integers(0, 4, (N + 2000, c.K))]
    streams, quals = MS.reads_from_keys(c.shape, keys, np.zeros(keys.shape, bool), rng)
    codes = MM.codes_for_keys(keys, quals, c.sheet, c.K, c.w1, c.m1, c.m2, plan.min_qual)
    far = np.flatnonzero(codes == 0xFFFF)[:N]
    batches["unrelated"] = ([([s[r] for r in far], [q[r] for r in far]) for s, q in streams], codes[far])
    assert far.size == N and (batches["one off"][1] != 0xFFFF).all() and (batches["exact"][1] != 0xFFFF).all()
    try:
        for kernel in (1, 2):
            engine.set_option("kernel", kernel)
            engine.set_mismatches(c.m1, c.m2)
            assert engine.kernel_kind() == {1: "fast", 2: "generic"}[kernel]
            for what, (reads, want) in batches.items():
                seq, qual, lens, full = rows_on_device(torch_cuda, engine.layout, reads)
                assert full
                for n in (7, 8, 9, 32767, 32768, 32769):
                    got, _, counts = _launch(engine, torch_cuda, ([t[:n] for t in seq], [t[:n] for t in qual], None), n, "plain")
                    assert (got == want[:n]).all(), (kernel, what, n, np.flatnonzero(got != want[:n])[:10])
                    assert (counts == MM.counts_for_codes(want[:n], len(c.sheet))).all(), (kernel, what, n)
    finally:
        engine.set_option("kernel", 0)


def test_counters_accumulate_across_launches_and_folds(torch_cuda, engine):
    """the rescue's signed move out of UNDETERMINED into the 64-bit totals, over launches without a reset and across folds of the
    32-bit rows (a fold in front of every launch: fold_pairs below the batch size)"""
    c = MS.corpus("comb_8x12")
    engine.set_plan(c.shape.plan)
    engine.set_barcodes(c.sheet)
    seq, qual, _, _ = rows_on_device(torch_cuda, engine.layout, c.streams)
    want = c.counts()
    assert want[3] > 0 and c.rescued.sum() > 40000 and c.n > 40000
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    codes = torch_cuda.full((c.n,), 0x7777, dtype=torch_cuda.int16, device="cuda")
    try:
        for kernel in (0, 2):
            engine.set_option("kernel", kernel)
            engine.set_mismatches(c.m1, c.m2)
            engine.set_option("fold_pairs", 40000)
            engine.reset_counts()
            for launches in (1, 2, 3, 1):
                if launches == 1:
                    engine.reset_counts()
                    assert not engine.counts().any()
                engine.demux_device(c.n, ptr(seq), ptr(qual), codes.data_ptr(), None, stream=torch_cuda.cuda.current_stream().cuda_stream)
                counts = engine.counts()
                assert (counts.view(np.int64) >= 0).all() and (counts == launches * want).all(), (kernel, launches, counts[:4], want[:4])
            assert (codes.cpu().numpy().view(np.uint16) == c.codes).all()
    finally:
        engine.set_option("fold_pairs", 0xFFFFFFFF)
        engine.set_option("kernel", 0)


def test_cli_rescued_pairs_in_every_per_destination_report(torch_cuda, tmp_path, monkeypatch):
    """One command-line run at (1, 1) over 2 BGZF chunks x 1 500 pairs, a tenth of the index reads one substitution from a
    barcode, with [filter] and every per-destination report on: the fastq outputs are the tolerant oracle's with the filter's
    model applied, and the quality, cycle, filter, duplication and unknown-barcode reports equal their models fed from those
    outputs -- a rescued pair counts under its sample everywhere.  Then the same with two chunk workers."""
    from collections import Counter
    from quade_amd import cycle_report as cyr
    from quade_amd import duplication_report as dr
    from quade_amd import filter_report as fr
    from quade_amd import quality_report as qr
    from tests import cycle_model as CYM
    from tests import dup_model as DM
    from tests import filter_model as FM
    from tests import qstats_model as QM
    from tests import stage_support as SS
    from tests import unknown_model as UM
    # (malformed records at the same places of all four streams: the pairs stay together, so the index reads keep their meaning)
    files, samples = SS._dataset(str(tmp_path / "data"), 47, 2, 1500, True, SS._plain_inserts, SS._same_places, one_off=True)
    names, slots = [s[0] for s in samples], 1 << 16
    budgets = "index1_mismatches : 1\nindex2_mismatches : 1\n"
    plain = tmp_path / "plain.txt"
    SS._write_conf(plain, files, samples, index_extra=budgets)
    counts0 = np.array(SS._oracle_run(plain, tmp_path / "ref0").counts(), dtype=np.int64)
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, 16, 8, 1, 1))
    counts1 = np.array(SS._oracle_run(plain, tmp_path / "ref1").counts(), dtype=np.int64)
    # pairs were rescued into every sample; nothing else moved
    moved = counts1[4:] - counts0[4:]
    assert counts0[0] == counts1[0] < 3000 and (moved >= 0).all() and (moved.reshape(-1, 2).sum(axis=1) > 0).all()
    assert 100 < moved.sum() == counts0[3] - counts1[3] and counts1[3] > 100
    texts, ftable, _, _ = FM.filtered_outputs(str(tmp_path / "ref1"), names, SS.P_F)
    exact_texts = FM.filtered_outputs(str(tmp_path / "ref0"), names, SS.P_F)[0]
    size = lambda t, part: sum(len(v) for f, v in t.items() if part in f)  # noqa: E731
    assert size(texts, "_pass_R1") > size(exact_texts, "_pass_R1") and size(texts, "Undetermined_R1") < size(exact_texts, "Undetermined_R1")  # some get past the filter
    want = tmp_path / "want"
    want.mkdir()
    for f, text in texts.items():
        with gzip.open(want / f, "wb") as fh:
            fh.write(text)
    pairs = []
    for d, stem in enumerate([n + q for n in names for q in ("_pass", "_fail")] + ["Undetermined"]):
        r1, r2 = (QM.fastq_records(str(want / (stem + r + ".fastq.gz"))) if stem + r + ".fastq.gz" in texts else [] for r in ("_R1", "_R2"))
        pairs += [(0xFFFF if d == 2 * len(names) else d, a[0], b[0], 0) for a, b in zip(r1, r2)]
    table, stats = DM.tally(len(names), pairs, DM.Params(32, 1, slots))
    unknown = Counter()
    with gzip.open(tmp_path / "ref1" / "Undetermined_R1.fastq.gz", "rt") as fh:  # (the tally sees every Undetermined pair, filtered or not)
        unknown.update(ln.strip().rsplit(":", 1)[1].upper() for i, ln in enumerate(fh) if i % 4 == 0)
    assert sum(unknown.values()) == counts1[3] and all(len(k) == 16 for k in unknown)
    for work, gpu in (("mine", ""), ("workers", "chunk_workers : 2\n")):
        conf = tmp_path / (work + ".txt")
        SS._write_conf(conf, files, samples, quality=True, index_extra=budgets, extra=SS.FILTER, gpu="duplicate_slots : %d\n" % slots + gpu)
        conf.write_text(conf.read_text().replace("[output]\n", "[output]\ncycle_report : True\nduplication_report : True\n"
                                                 "duplication_sample : 1\ntop_unknown_barcodes : 1000\n", 1))
        mine = tmp_path / work
        SS._cli(conf, mine)
        SS._check_files(mine, texts)
        SS._check_main_report(mine, tmp_path / "ref1")
        SS._check_report(mine, fr, ftable, names, SS.P_F.keywords())
        SS._check_report(mine, qr, QM.table_from_outputs(str(want), names), names)
        SS._check_report(mine, cyr, CYM.table_from_outputs(str(want), names))
        SS._check_report(mine, dr, stats, *DM.arrays(table), names, dict(bases=32, sample=1, slots=slots))
        head, _, rows = UM.parse_report(str(mine / "Quade_unknown_barcodes.csv"))
        assert head == {"Pair Undetermined": str(counts1[3]), "Short index slice": "0", "Not tallied": "0",
                        "Distinct barcodes tallied": str(len(unknown))}
        fused = [(s[0], s[1] + s[2]) for s in samples]
        assert len(rows) == len(unknown) <= 1000
        for r, (key, c) in zip(rows, UM.report_order(unknown)):
            name, d1, d2 = UM.nearest_brute(key, fused, 8)
            assert r == [key[:8], key[8:], str(c), str(c * 100 // counts1[3]), name, str(d1), str(d2)] and (d1 > 1 or d2 > 1)


def _decompressed(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".fastq.gz"):
            with gzip.open(os.path.join(d, f), "rb") as fh:
                out[f] = fh.read()
    return out


def test_cli_device_pipeline_end_to_end(torch_cuda, tmp_path, monkeypatch):
    """synthetic BGZF dataset (10 % of the index reads carry an N) through the command line's device pipeline at (1, 1)"""
    data = tmp_path / "data"
    data.mkdir()
    paths, bcs = synth.write_fastq_dataset(str(data), 6000, n_samples=12, insert_len=50, seed=8)
    fused = [a + b for a, b in bcs]
    assert hb.check_mismatch_collisions(fused, 16, 8, 1, 1) is None
    conf = str(tmp_path / "conf.txt")
    synth.write_conf(conf, paths, bcs)
    text = open(conf).read().replace("index2_end : 8\n", "index2_end : 8\nindex1_mismatches : 1\nindex2_mismatches : 1\n", 1)
    open(conf, "w").write(text)
    out_hip, out_ref = tmp_path / "hip", tmp_path / "ref"
    out_hip.mkdir()
    out_ref.mkdir()
    from quade_amd.quade import Quade
    old = os.getcwd()
    os.chdir(str(out_hip))
    try:
        q = Quade.class_init(["-c", conf])
        assert q.cf.idx1_mismatches == q.cf.idx2_mismatches == 1 and q.cf.device_pipeline
        assert q() == 0
    finally:
        os.chdir(old)
    st = getattr(q, "pipe_stats", None)
    assert st is not None and st["gzip_fallbacks"] == 0, st
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, 16, 8, 1, 1))
    qo.run_quade(conf, outdir=str(out_ref))
    got, ref = _decompressed(str(out_hip)), _decompressed(str(out_ref))
    assert sorted(got) == sorted(ref) and all(got[f] == ref[f] for f in ref)
    rep = lambda d: open(os.path.join(d, "Quade_report.csv")).read().split("\n")  # noqa: E731
    a, b = rep(str(out_hip)), rep(str(out_ref))
    assert a[0].startswith("Program Quade 0.3.2\tDate ") and a[1:] == b[1:]
