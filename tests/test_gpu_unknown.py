"""The unknown-barcode tally on the MI355X: the table read back from the device equals a collections.Counter over the upper-cased
barcode slices of the pairs the unmodified oracle routes to 0xFFFF (tests/unknown_model.py), on every path that launches the
match kernels, across launches and streams, with the mismatch rescue, under overflow and tag collisions, and through the
command line (the bundled golden run: the truth is the name suffixes of the reference's own Undetermined file)."""
import gzip
import os
import shutil
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from quade_amd import synth
from tests import helpers as H
from tests import mismatch_model as MM
from tests import unknown_model as UM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch


@pytest.fixture()
def engine(torch_cuda):
    with hb.Engine(0) as e:
        yield e


class Planted(object):
    """synth's workload `name` (matches, one-substitution reads, random reads, lower case) with a planted unknown set written over
    22 % of the pairs: one hot key (>= 30 % of the Undetermined pairs) and lower-case spellings of it, poly-G, keys with N,
    keys one substitution from a sample.  short_frac: reads cut inside (or behind) their index window, rows zero padded."""

    def __init__(self, name, n, seed, short_frac=0.0):
        w = synth.generate(name, n, seed=seed)
        lay = w.layout
        rng = np.random.default_rng(seed)
        ns, iw = lay.n_streams, synth.CONFIGS[name].get("iw", 8)
        K = iw * ns
        self.w, self.n, self.K, self.w1 = w, n, K, iw
        seq = [t.numpy().copy() for t in w.seq]
        qual = [t.numpy().copy() for t in w.qual]
        bcs = w.barcodes.numpy()
        taken = set(w.barcode_strings())
        hot = None
        while hot is None or hot in taken:
            hot = "".join(rng.choice(list("ACGT"), K))
        self.hot = hot
        key = np.concatenate([s[:, :iw] for s in seq], axis=1)
        kind = rng.integers(0, 100, n)
        hot_b = np.frombuffer(hot.encode(), np.uint8)
        key[kind < 14] = hot_b
        lower = np.flatnonzero((kind >= 14) & (kind < 16))
        key[lower] = hot_b
        key[lower, rng.integers(0, K, lower.size)] |= 0x20  # folds into the hot key's entry
        key[(kind >= 16) & (kind < 18)] = ord("G")
        withn = np.flatnonzero((kind >= 18) & (kind < 20))
        key[withn] = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, (withn.size, K))]
        key[withn, rng.integers(0, K, withn.size)] = ord("N")
        key[withn[:3]] = ord("N")
        near = np.flatnonzero((kind >= 20) & (kind < 22))
        key[near] = bcs[rng.integers(0, bcs.shape[0], near.size)]
        pos = rng.integers(0, K, near.size)
        key[near, pos] = np.where(key[near, pos] == ord("A"), ord("C"), ord("A"))
        for k in range(ns):
            seq[k][:, :iw] = key[:, k * iw:(k + 1) * iw]
        self.lens = [np.full(n, lay.seq_off[k] + lay.seq_width[k], dtype=np.uint8) for k in range(ns)]
        cut = np.flatnonzero(rng.integers(0, 1000, n) < int(1000 * short_frac))
        for r in cut:
            k = int(rng.integers(0, ns))
            c = int(rng.integers(0, self.lens[k][r]))
            self.lens[k][r] = c
            seq[k][r, c:] = 0
            qc = max(0, min(lay.qual_width[k], c - (lay.qual_off[k] - lay.seq_off[k])))
            qual[k][r, qc:] = 0xFF
        self.short_idx = cut.astype(np.uint32)
        self.seq, self.qual = seq, qual
        self.bcs = w.barcode_strings()

    def oracle(self):
        lay = self.w.layout
        reads = []
        for k in range(lay.n_streams):
            reads += list(H.rows_to_reads(self.seq[k], self.qual[k], lay.seq_width[k], lay.qual_off[k] - lay.seq_off[k],
                                          lay.qual_width[k], self.lens[k]))
        if lay.n_streams == 1:
            reads += [None, None]
        return H.oracle_on_reads(self.bcs, self.w.plan, *reads)

    def device(self, torch, lo=0, hi=None):
        hi = self.n if hi is None else hi
        f = lambda arrs: [torch.from_numpy(a[lo:hi]).cuda() for a in arrs]  # noqa: E731
        return f(self.seq), f(self.qual), f(self.lens)


def launch(torch, eng, seq, qual, n, lens=None, short=None, stream=0):
    """one qd_demux_device / _ragged call; returns (codes tensor, mol tensor or None) -- not synchronised"""
    M = eng.layout.mol_width
    codes = torch.full((max(n, 1),), 0x7777, dtype=torch.int16, device="cuda")
    mol = torch.full((max(n, 1), max(M, 1)), 0x55, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    if short is not None:
        eng.demux_device_ragged(n, ptr(seq), ptr(qual), codes.data_ptr(), mol.data_ptr() if M else None, ptr(lens),
                                int(short.numel()), short.data_ptr(), stream=stream)
    else:
        eng.demux_device(n, ptr(seq), ptr(qual), codes.data_ptr(), mol.data_ptr() if M else None,
                         lens=ptr(lens) if lens else (None, None), stream=stream)
    return codes, (mol if M else None)


def read_table(eng):
    keys, counts = eng.unknown_read()
    return UM.table_counter(keys, counts), eng.unknown_stats()


def np_codes(codes, n):
    return codes.cpu().numpy().view(np.uint16)[:n]


# ---- 1. parity of the tally ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("cfg2", 4097), ("cfg3", 30001), ("cfg4", 4097), ("cfg5", 70003), ("cfg3", 1)])
def test_tally_equals_the_oracle_counter(torch_cuda, engine, name, n):
    torch = torch_cuda
    p = Planted(name, n, seed=300 + n, short_frac=0.05)
    whole = Planted(name, n, seed=300 + n)
    for case, kernel in ((whole, "fast"), (whole, "generic"), (p, "ragged")):
        codes_o, idx_o, mol_o, counts_o = case.oracle()
        model, short = UM.model_from_oracle(codes_o, idx_o, case.K)
        if n > 1000:
            U = int(counts_o[3])
            assert model[case.hot] >= 0.30 * U, (model[case.hot], U)
            assert model["G" * case.K] > 0 and model["N" * case.K] >= 3 and any("N" in k for k in model)
            assert short > 0 or kernel != "ragged"
        engine.set_plan(case.w.plan)
        engine.set_barcodes(case.bcs)
        engine.set_option("force_generic", int(kernel == "generic"))
        engine.unknown_enable(1 << 16)
        seq, qual, lens = case.device(torch)
        if kernel == "ragged":
            assert engine.kernel_kind(False) == "fast"
            sidx = torch.from_numpy(case.short_idx.astype(np.int64)).to(torch.int32).cuda() if case.short_idx.size else \
                torch.zeros(1, dtype=torch.int32, device="cuda")
            codes, mol = launch(torch, engine, seq, qual, n, lens, sidx[:case.short_idx.size])
        else:
            assert engine.kernel_kind(False) == kernel
            codes, mol = launch(torch, engine, seq, qual, n)
        engine.synchronize()
        assert (np_codes(codes, n) == codes_o).all()
        counts = engine.counts()
        assert (counts == counts_o).all()
        table, stats = read_table(engine)
        UM.check_exact(table, stats, model, short, counts[3])
        engine.set_option("force_generic", 0)


# ---- 2. accumulation and streams ----------------------------------------------------------------------------------------------
def test_accumulation_over_slots_and_caller_streams(torch_cuda):
    torch = torch_cuda
    n, B = 40009, 4096  # 10 batches
    p = Planted("cfg3", n, seed=77)
    codes_o, idx_o, _, counts_o = p.oracle()
    model, short = UM.model_from_oracle(codes_o, idx_o, p.K)
    with hb.Engine(0) as eng:
        eng.set_plan(p.w.plan)
        eng.set_barcodes(p.bcs)
        eng.unknown_enable(1 << 16)
        seq, qual, _ = p.device(torch)
        launch(torch, eng, seq, qual, n)
        one, stats1 = read_table(eng)
        UM.check_exact(one, stats1, model, short, eng.counts()[3])
        # pinned slots: 3 slots, 10 batches, every slot's launch on its own stream
        eng.reset_counts()
        assert int(eng.unknown_stats().sum()) == 0 and len(eng.unknown_read()[1]) == 0
        eng.slots_create(3, B)
        for i, a in enumerate(range(0, n, B)):
            b = min(n, a + B)
            s = i % 3
            if i >= 3:
                eng.wait(s)
            v = eng.slot(s)
            for k in range(2):
                v["seq"][k][:b - a] = p.seq[k][a:b]
                v["qual"][k][:b - a] = p.qual[k][a:b]
            eng.submit(s, b - a)
        for s in range(3):
            eng.wait(s)
        table, stats = read_table(eng)
        assert (eng.counts() == counts_o).all()
        UM.check_exact(table, stats, model, short, counts_o[3])
        assert table == one
        eng.slots_destroy()
        # several qd_demux_device calls alternating over two caller streams
        eng.reset_counts()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        keep = []
        for i, a in enumerate(range(0, n, B)):
            b = min(n, a + B)
            keep.append(launch(torch, eng, [t[a:b] for t in seq], [t[a:b] for t in qual], b - a, stream=streams[i % 2].cuda_stream))
        eng.synchronize()
        table, stats = read_table(eng)
        assert (eng.counts() == counts_o).all()
        UM.check_exact(table, stats, model, short, counts_o[3])
        assert table == one
        assert (np.concatenate([np_codes(c, min(n, a + B) - a) for (c, _), a in zip(keep, range(0, n, B))]) == codes_o).all()


# ---- 3. with budgets (1, 1) ---------------------------------------------------------------------------------------------------
def test_rescued_pairs_are_not_tallied(torch_cuda, engine, monkeypatch):
    torch = torch_cuda
    from tests.mismatch_support import SHAPES, make_reads, rows_on_device, sheet
    bcs = sheet("dual8", 64, 1, 1)
    n = 20011
    streams = make_reads("dual8", bcs, n, 1, 1, seed=31, short_frac=0.05)
    plan = SHAPES["dual8"][0]
    reads = []
    for s, q in streams:
        reads += [[x.decode() for x in s], [x.decode() for x in q]]
    exact = H.oracle_on_reads(bcs, plan, *reads)
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, 16, 8, 1, 1))
    tol = H.oracle_on_reads(bcs, plan, *reads)
    monkeypatch.undo()
    model, short = UM.model_from_oracle(tol[0], tol[1], 16)
    model0, short0 = UM.model_from_oracle(exact[0], exact[1], 16)
    assert sum(model0.values()) > sum(model.values()) > 0 and short == short0 > 0
    engine.set_plan(plan)
    engine.set_barcodes(bcs)
    engine.set_mismatches(1, 1)
    engine.unknown_enable(1 << 16)
    seq, qual, lens, full = rows_on_device(torch, engine.layout, streams)
    assert not full
    short_idx = np.flatnonzero(np.array([len(streams[0][0][r]) < 8 or len(streams[1][0][r]) < 8 for r in range(n)]))
    sidx = torch.from_numpy(short_idx.astype(np.int64)).to(torch.int32).cuda()
    for generic in (False, True):
        engine.reset_counts()
        codes, _ = launch(torch, engine, seq, qual, n, lens=lens, short=None if generic else sidx)
        engine.synchronize()
        assert (np_codes(codes, n) == tol[0]).all()
        table, stats = read_table(engine)
        UM.check_exact(table, stats, model, short, engine.counts()[3])
    engine.set_mismatches(0, 0)  # the tally stays on: now the exact model
    engine.reset_counts()
    launch(torch, engine, seq, qual, n, lens=lens, short=sidx)
    table, stats = read_table(engine)
    UM.check_exact(table, stats, model0, short0, engine.counts()[3])


def test_growing_batches_on_two_streams_with_the_rescue(torch_cuda, engine, monkeypatch):
    """Batches of 300, 5 000, 700 and 9 000 pairs alternate over two caller streams with budgets (1, 1): on either stream the second
    batch is more than the first one's rescue list and tally scratch hold (700 > 300, 9 000 > 5 000), so both are freed and
    allocated again behind that stream's work, and the tally reads the rescue's new list."""
    torch = torch_cuda
    from tests.mismatch_support import SHAPES, make_reads, rows_on_device, sheet
    sizes = (300, 5000, 700, 9000)
    n = sum(sizes)
    bcs = sheet("dual8", 64, 1, 1)
    streams = make_reads("dual8", bcs, n, 1, 1, seed=47, short_frac=0.05)
    plan = SHAPES["dual8"][0]
    reads = []
    for s, q in streams:
        reads += [[x.decode() for x in s], [x.decode() for x in q]]
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, 16, 8, 1, 1))
    codes_o, idx_o, _, counts_o = H.oracle_on_reads(bcs, plan, *reads)
    monkeypatch.undo()
    model, short = UM.model_from_oracle(codes_o, idx_o, 16)
    assert sum(model.values()) > 0 and short > 0
    engine.set_plan(plan)
    engine.set_barcodes(bcs)
    engine.set_mismatches(1, 1)
    engine.unknown_enable(1 << 16)
    seq, qual, lens, full = rows_on_device(torch, engine.layout, streams)
    assert not full
    cuda_streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep, a = [], 0
    for i, m in enumerate(sizes):
        cut = lambda ts: [t[a:a + m] for t in ts]  # noqa: E731
        keep.append(launch(torch, engine, cut(seq), cut(qual), m, lens=cut(lens), stream=cuda_streams[i % 2].cuda_stream))
        a += m
    engine.synchronize()
    assert (np.concatenate([np_codes(c, m) for (c, _), m in zip(keep, sizes)]) == codes_o).all()
    counts = engine.counts()
    assert (counts == counts_o).all()
    table, stats = read_table(engine)
    UM.check_exact(table, stats, model, short, counts[3])


# ---- 4. no side effects, state ------------------------------------------------------------------------------------------------
def test_no_side_effects_and_state(torch_cuda):
    torch = torch_cuda
    p = Planted("cfg4", 30001, seed=5)
    with hb.Engine(0) as eng:
        for call in (eng.unknown_stats, eng.unknown_read, lambda: eng.unknown_enable(1 << 12)):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        eng.set_plan(p.w.plan)
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.unknown_enable(1 << 12)
        assert ei.value.code == hb.QD_ERR_STATE
        eng.set_barcodes(p.bcs)
        for bad in (1000, 1 << 9, 1 << 29, 3 << 10, -1024):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.unknown_enable(bad)
            assert ei.value.code == hb.QD_ERR_INVALID
        for bad in (0, 65):
            with pytest.raises(hb.QuadeHipError):
                eng.set_option("unknown_tag_bits", bad)
        seq, qual, _ = p.device(torch)
        out = {}
        for on in (False, True, False):
            eng.unknown_enable(1 << 14 if on else 0)
            eng.reset_counts()
            codes, mol = launch(torch, eng, seq, qual, p.n)
            eng.synchronize()
            got = (np_codes(codes, p.n).copy(), mol.cpu().numpy().copy(), eng.counts())
            if on:
                assert int(eng.unknown_stats()[0]) > 0
            else:
                with pytest.raises(hb.QuadeHipError) as ei:
                    eng.unknown_stats()
                assert ei.value.code == hb.QD_ERR_STATE
            for a, b in zip(got, out.setdefault("first", got)):
                assert (a == b).all()
        # qd_reset_counts empties the table, qd_set_barcodes and qd_set_plan turn the tally off
        eng.unknown_enable(1 << 14)
        launch(torch, eng, seq, qual, p.n)
        assert int(eng.unknown_stats()[3]) > 0
        eng.reset_counts()
        assert not eng.unknown_stats().any() and len(eng.unknown_read()[1]) == 0
        launch(torch, eng, seq, qual, p.n)
        table, stats = read_table(eng)
        UM.check_invariant(table, stats, eng.counts()[3])
        for turn_off in (lambda: eng.set_barcodes(p.bcs), lambda: (eng.set_plan(p.w.plan), eng.set_barcodes(p.bcs))):
            eng.unknown_enable(1 << 14)
            eng.unknown_stats()
            turn_off()
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.unknown_stats()
            assert ei.value.code == hb.QD_ERR_STATE


# ---- 5. overflow, 6. tag collisions -------------------------------------------------------------------------------------------
def _distinct_keys_workload(torch, n_keys, n, seed):
    """cfg3 rows whose keys are n_keys distinct random 16-mers outside the sheet, each pair drawing one (skewed)"""
    w = synth.generate("cfg3", n, seed=seed)
    rng = np.random.default_rng(seed)
    pool = np.unique(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2 * n_keys, 16))], axis=0)
    sheet = set(w.barcode_strings())
    pool = np.array([k for k in pool if bytes(k).decode() not in sheet][:n_keys])
    assert pool.shape[0] == n_keys
    pick = np.minimum((rng.random(n) ** 2 * n_keys).astype(np.int64), n_keys - 1)
    pick[:n_keys] = np.arange(n_keys)  # every key at least once
    key = pool[pick]
    seq = [w.seq[0].numpy().copy(), w.seq[1].numpy().copy()]
    seq[0][:, :8], seq[1][:, :8] = key[:, :8], key[:, 8:]
    model = Counter(bytes(k).decode() for k in key)
    return w, [torch.from_numpy(s).cuda() for s in seq], [t.cuda() for t in w.qual], model


@pytest.mark.parametrize("n_keys,lossy", [(3000, True), (1000, False), (500, False)])
def test_overflow_accounting(torch_cuda, engine, n_keys, lossy):
    """slots = 1024.  A few thousand distinct keys cannot all be admitted: dropped > 0 and the accounting conditions hold.  Fewer
    than 1024 distinct keys are all admitted (the probe limit of a 1024-slot table is the whole table): dropped == 0."""
    torch = torch_cuda
    n = 20000
    w, seq, qual, model = _distinct_keys_workload(torch, n_keys, n, seed=n_keys)
    engine.set_plan(w.plan)
    engine.set_barcodes(w.barcode_strings())
    engine.unknown_enable(1024)
    launch(torch, engine, seq, qual, n)
    launch(torch, engine, seq, qual, n)  # accumulation under overflow: every count doubles
    model = Counter({k: 2 * c for k, c in model.items()})
    table, stats = read_table(engine)
    U = engine.counts()[3]
    assert int(U) == 2 * n
    if lossy:
        UM.check_lossy(table, stats, model, 0, U)
        assert len(table) == 1024
    else:
        UM.check_exact(table, stats, model, 0, U)


def test_tag_collisions(torch_cuda, engine):
    """unknown_tag_bits = 6: 64 tags for 400 distinct keys in 2^16 slots.  One key per tag owns the entry, the others are dropped."""
    torch = torch_cuda
    n = 20000
    w, seq, qual, model = _distinct_keys_workload(torch, 400, n, seed=6)
    engine.set_plan(w.plan)
    engine.set_barcodes(w.barcode_strings())
    engine.set_option("unknown_tag_bits", 6)
    engine.unknown_enable(1 << 16)
    launch(torch, engine, seq, qual, n)
    table, stats = read_table(engine)
    UM.check_lossy(table, stats, model, 0, engine.counts()[3])
    assert 0 < len(table) <= 64
    engine.set_option("unknown_tag_bits", 64)
    engine.reset_counts()
    launch(torch, engine, seq, qual, n)
    table, stats = read_table(engine)
    UM.check_exact(table, stats, model, 0, engine.counts()[3])


# ---- 7. full size, once -------------------------------------------------------------------------------------------------------
def test_full_size_cfg3(torch_cuda):
    """100 M pairs of cfg3 in one launch at the default 2^24 slots; the truth is torch.unique over the packed, case-folded keys of
    the pairs the generator marks 0xFFFF (about 5 M distinct keys: a load of 0.3)."""
    torch = torch_cuda
    n = 100_000_000
    w = synth.generate("cfg3", n, device="cuda")
    und = w.expected == 0xFFFF
    key = torch.cat([w.seq[0][und][:, :8], w.seq[1][und][:, :8]], dim=1)
    key = torch.where((key >= 97) & (key <= 122), key - 32, key).contiguous()
    uniq, cnt = torch.unique(key.view(torch.int64), dim=0, return_counts=True)
    del key
    with hb.Engine(0) as eng:
        eng.set_plan(w.plan)
        eng.set_barcodes(w.barcode_strings())
        eng.unknown_enable(1 << 24)
        assert eng.kernel_kind() == "fast"
        codes = torch.empty(n, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.demux_device(n, [t.data_ptr() for t in w.seq], [t.data_ptr() for t in w.qual], codes.data_ptr(), None)
        eng.synchronize()
        stats = eng.unknown_stats()
        counts = eng.counts()
        keys, kc = eng.unknown_read()
    assert int(counts[3]) == int(und.sum())
    assert int(stats[2]) == 0 and int(stats[1]) == 0 and int(stats[0]) == int(counts[3]) and int(stats[3]) == uniq.shape[0]
    got = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64).reshape(-1, 2)).cuda()
    gu, inv = torch.unique(got, dim=0, return_inverse=True)
    assert gu.shape[0] == got.shape[0] and torch.equal(gu, uniq)
    gc = torch.zeros(gu.shape[0], dtype=torch.int64, device="cuda")
    gc[inv] = torch.from_numpy(kc.astype(np.int64)).cuda()
    assert torch.equal(gc, cnt)


# ---- 8. command line, the bundled golden run; 9. merging ----------------------------------------------------------------------
def _run_cli(conf, workdir):
    from quade_amd.quade import Quade
    old = os.getcwd()
    os.chdir(workdir)
    try:
        q = Quade(conf_file=conf)
        assert q() == 0
    finally:
        os.chdir(old)
    return q


def _golden_truth(bundled_dir):
    names = Counter()
    with gzip.open(os.path.join(bundled_dir, "result", "Undetermined_R1.fastq.gz"), "rt") as fh:
        for i, ln in enumerate(fh):
            if i % 4 == 0:
                names[ln.strip().split(":")[-2].upper()] += 1  # "...:IDX:MOL"
    return names


@pytest.mark.parametrize("path", ["device_pipeline", "pinned_slots"])
def test_cli_bundled_golden_run(torch_cuda, tmp_path, bundled_dir, path):
    from tests.run_support import _compare_dirs
    truth = _golden_truth(bundled_dir)
    assert sum(truth.values()) == 247 and len(truth) == 19
    assert UM.report_order(truth)[:6] == [("GCCAGCCA", 53), ("CGATCGAT", 48), ("TGACTGAC", 40), ("CAGACAGA", 38), ("GTGAGTGA", 29),
                                          ("AGTCAGTC", 26)]
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt")) as fh:
        base = fh.read()
    assert "[output]\n" in base
    extra = "" if path == "device_pipeline" else "\n[gpu]\ndevice_pipeline : False\n"
    for opt in (True, False):
        work = tmp_path / ("with" if opt else "without")
        work.mkdir()
        conf = work / "conf.txt"
        conf.write_text((base.replace("[output]\n", "[output]\ntop_unknown_barcodes : 10\n", 1) if opt else base) + extra)
        _run_cli(str(conf), str(work))
        os.remove(conf)
        _compare_dirs(str(work), os.path.join(bundled_dir, "result"))
        report = work / "Quade_unknown_barcodes.csv"
        if not opt:
            assert not report.exists()
            continue
        head, cols, rows = UM.parse_report(str(report))
        assert head == {"Pair Undetermined": "247", "Short index slice": "0", "Not tallied": "0", "Distinct barcodes tallied": "19"}
        assert cols == ["index1_seq", "index2_seq", "count", "percent_of_undetermined", "nearest_sample", "index1_distance",
                        "index2_distance"]
        assert [r[0] + r[1] for r in rows] == ["GCCAGCCA", "CGATCGAT", "TGACTGAC", "CAGACAGA", "GTGAGTGA", "AGTCAGTC",
                                        "AGTGAGTG", "CAGTCAGT", "CCAGCCAG", "CCGACCGA"]
        samples = [("S1", "ACAGACAG"), ("S2", "CTTGCTTG")]
        for r, (key, c) in zip(rows, UM.report_order(truth)):
            name, d1, d2 = UM.nearest_brute(key, samples, 4)
            assert r == [key[:4], key[4:], str(c), str(c * 100 // 247), name, str(d1), str(d2)]


def test_merging_chunk_workers_and_ranks(torch_cuda, tmp_path):
    """3 chunks: one worker and one rank, chunk_workers : 2 (two contexts), and 2 ranks on GPU 0 over the files transport all
    write the same Quade_unknown_barcodes.csv; its rows are the oracle's Undetermined index slices."""
    from tests.run_support import _conf, _make_dataset
    rng = np.random.default_rng(99)
    bcs = sorted({("".join(rng.choice(list("ACGT"), 8)), "".join(rng.choice(list("ACGT"), 8))) for _ in range(7)})
    data = tmp_path / "data"
    data.mkdir()
    files = _make_dataset(str(data), rng, 3, 150, True, 8, list(bcs), trunc=True)
    samples = [("S%d" % i, b1, b2) for i, (b1, b2) in enumerate(bcs)]
    outs = {}
    for mode, gpu in (("one", ""), ("workers", "chunk_workers : 2\n"), ("ranks", "")):
        conf = tmp_path / (mode + ".txt")
        _conf(str(conf), files, True, ((1, 8), (1, 8), None, None), 25, samples, gpu="[gpu]\nbatch_pairs : 64\n" + gpu)
        conf.write_text(conf.read_text().replace("[output]\n", "[output]\ntop_unknown_barcodes : 1000\n", 1))
        work = tmp_path / mode
        work.mkdir()
        if mode == "ranks":
            env = dict(os.environ, PYTHONPATH=ROOT, QUADE_DIST_TRANSPORT="files", QUADE_DEVICE="0")
            for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
                env.pop(k, None)
            r = subprocess.run([sys.executable, "-m", "quade_amd.launch", "-n", "2", "-c", str(conf)], cwd=str(work), env=env,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        else:
            _run_cli(str(conf), str(work))
        outs[mode] = (work / "Quade_unknown_barcodes.csv").read_text()
    assert outs["one"] == outs["workers"] == outs["ranks"]
    ref = tmp_path / "ref"
    ref.mkdir()
    sset, _ = qo.run_quade(str(tmp_path / "one.txt"), outdir=str(ref))
    truth, short = Counter(), 0
    with gzip.open(ref / "Undetermined_R1.fastq.gz", "rt") as fh:
        for i, ln in enumerate(fh):
            if i % 4 == 0:
                key = ln.strip().rsplit(":", 1)[1].upper()
                if len(key) < 16:
                    short += 1
                else:
                    truth[key] += 1
    head, cols, rows = UM.parse_report(str(tmp_path / "one" / "Quade_unknown_barcodes.csv"))
    assert head == {"Pair Undetermined": str(sset.counts()[3]), "Short index slice": str(short), "Not tallied": "0",
                    "Distinct barcodes tallied": str(len(truth))} and short > 0
    assert [(r[0] + r[1], int(r[2])) for r in rows] == UM.report_order(truth)
