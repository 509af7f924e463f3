"""The index-hopping matrix on the MI355X: the table read back from the device equals, cell by cell, a collections.Counter over
(index-1 part, index-2 part) of the pairs the unmodified oracle routes to 0xFFFF (tests/hop_model.py) -- on every path that
launches the match kernels, across launches and streams, with the mismatch rescue and the unknown tally beside it -- and the
report the command line writes equals the report module fed with the model's table."""
import functools
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from quade_amd import hopping_report as hr
from quade_amd import synth
from tests import helpers as H
from tests import hop_model as HM
from tests import mismatch_model as MM
from tests import unknown_model as UM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70001  # several workgroups, a partial wave at the end, enough pairs for a hot cell to fill the LDS hash's probe sequence
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch


@pytest.fixture()
def engine(torch_cuda):
    with hb.Engine(0) as e:
        yield e


def _word(i, L):
    return "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(L))


def _rows(strings):
    return np.array([np.frombuffer(s.encode(), np.uint8) for s in strings], dtype=np.uint8)


class Planted(object):
    """n pairs of index reads over a sheet: three quarters carry a sample's barcode (a few of them lower case or with one
    low-quality base), one quarter is the planted Undetermined set written over the index windows --
      swapped partners (a's index 1 with b's index 2, a != b and off the sheet), one such cell made hot (>= 30 % of the planted
      pairs), lower-case spellings of swapped partners, a known index 1 with a random index 2 and the reverse, random in both
      parts, a part with one N, a part one substitution from a sample.
    keys: the pairs' fused slices when given (synth's workload), drawn from the sheet otherwise.  short_frac: reads cut inside
    (or behind) their index window; reads(True) has them cut, reads(False) whole."""

    def __init__(self, plan, bcs, n, seed, keys=None, quals=None, short_frac=0.03):
        rng = np.random.default_rng(seed)
        self.plan, self.bcs, self.n = plan, list(bcs), n
        w1, w2 = plan.idx1_end - plan.idx1_start, plan.idx2_end - plan.idx2_start
        K = w1 + w2
        self.w1, self.K = w1, K
        self.P1, self.P2, self.part1, self.part2 = HM.part_lists(self.bcs, K, w1)
        self.n1, self.n2 = len(self.P1), len(self.P2)
        on = [b for b in self.bcs if len(b) == K]
        p1, p2 = _rows(list(self.P1)), _rows(list(self.P2))
        sheet_cells = set(zip(self.part1, self.part2))
        off = [(a, b) for a in range(self.n1) for b in range(self.n2) if (a, b) not in sheet_cells]
        assert off, "a sheet without an unexpected cell"
        off = np.array(off)
        if keys is None:
            keys = _rows(on)[rng.integers(0, len(on), n)].copy()
            lc = np.flatnonzero(rng.integers(0, 100, n) < 3)
            keys[lc, rng.integers(0, K, lc.size)] |= 0x20
        if quals is None:
            quals = (rng.integers(30, 41, (n, K)) + 33).astype(np.uint8)
            bad = np.flatnonzero(rng.integers(0, 100, n) < 15)
            quals[bad, rng.integers(0, K, bad.size)] = (rng.integers(2, 25, bad.size) + 33).astype(np.uint8)
        keys = keys.copy()
        kind = rng.integers(0, 100, n) if n > 1 else np.array([9])
        self.hot = tuple(int(x) for x in off[rng.integers(0, len(off))])
        sel = kind < 9  # 36 % of the planted quarter
        keys[sel, :w1], keys[sel, w1:] = p1[self.hot[0]], p2[self.hot[1]]
        sel = np.flatnonzero((kind >= 9) & (kind < 13) | (kind >= 21) & (kind < 25))  # swapped partners, and what is made of them
        cell = off[rng.integers(0, len(off), sel.size)]
        keys[sel, :w1], keys[sel, w1:] = p1[cell[:, 0]], p2[cell[:, 1]]
        # a known index 1 (of any sample whose barcode has w1 bases at least, on the matrix or off it) with a random index 2, the reverse
        first = _rows([b[:w1] for b in self.bcs if len(b) >= w1])
        sel = np.flatnonzero((kind >= 13) & (kind < 16))
        keys[sel, :w1], keys[sel, w1:] = first[rng.integers(0, len(first), sel.size)], ACGT[rng.integers(0, 4, (sel.size, w2))]
        sel = np.flatnonzero((kind >= 16) & (kind < 19))
        keys[sel, :w1], keys[sel, w1:] = ACGT[rng.integers(0, 4, (sel.size, w1))], p2[rng.integers(0, self.n2, sel.size)]
        sel = np.flatnonzero((kind >= 19) & (kind < 21))
        keys[sel] = ACGT[rng.integers(0, 4, (sel.size, K))]
        sel = np.flatnonzero((kind >= 21) & (kind < 23))  # lower case: one letter, or the whole slice
        keys[sel, rng.integers(0, K, sel.size)] |= 0x20
        keys[sel[::3]] |= 0x20
        sel = np.flatnonzero(kind == 23)
        keys[sel, rng.integers(0, K, sel.size)] = ord("N")
        sel = np.flatnonzero(kind == 24)
        pos = rng.integers(0, K, sel.size)
        keys[sel, pos] = np.where(keys[sel, pos] == ord("A"), ord("C"), ord("A"))
        self.keys, self.quals = keys, quals
        # the reads: the slice at the plan's offset, random bases in front of it, nothing behind
        starts, widths = (plan.idx1_start, plan.idx2_start), (w1, w2)
        self.full, self.cut = [], []
        is_cut = rng.integers(0, 1000, n) < int(1000 * short_frac)
        side = rng.integers(0, 2, n)
        for k in range(2):
            L, at = starts[k] + widths[k], k * w1
            seq = ACGT[rng.integers(0, 4, (n, L))]
            qual = np.full((n, L), ord("I"), np.uint8)
            seq[:, starts[k]:] = keys[:, at:at + widths[k]]
            qual[:, starts[k]:] = quals[:, at:at + widths[k]]
            sb, qb = seq.tobytes(), qual.tobytes()
            s = [sb[r * L:(r + 1) * L] for r in range(n)]
            q = [qb[r * L:(r + 1) * L] for r in range(n)]
            self.full.append((s, q))
            lens = np.where(is_cut & (side == k), rng.integers(0, L, n), L)
            self.cut.append(([x[:c] for x, c in zip(s, lens)], [x[:c] for x, c in zip(q, lens)]))
        self.short_idx = np.flatnonzero(is_cut).astype(np.uint32)

    def reads(self, cut):
        return self.cut if cut else self.full

    @functools.lru_cache(maxsize=None)
    def oracle(self, cut=False, lo=0, hi=None):
        """(codes, counts, model Counter, short, the fused slices) of the unmodified oracle over pairs [lo, hi)"""
        args = []
        for s, q in self.reads(cut):
            args += [[x.decode("latin-1") for x in s[lo:hi]], [x.decode("latin-1") for x in q[lo:hi]]]
        codes, idx, _, counts = H.oracle_on_reads(self.bcs, self.plan, *args)
        model, short = HM.model_from_oracle(codes, idx, self.K, self.w1, self.P1, self.P2)
        return codes, counts, model, short, idx

    def rows(self, torch, layout, cut=False, lo=0, hi=None):
        """device rows of pairs [lo, hi): (seq, qual, lens) lists of cuda tensors"""
        seq, qual, lens = [], [], []
        for k, (s, q) in enumerate(self.reads(cut)):
            sr, qr, lr, _ = hb.pack_index_reads(layout, k, s[lo:hi], q[lo:hi])
            seq.append(torch.from_numpy(sr).cuda())
            qual.append(torch.from_numpy(qr).cuda())
            lens.append(torch.from_numpy(lr).cuda())
        return seq, qual, lens

    def check(self, table, model, short, undetermined):
        HM.check_table(table, self.n1, self.n2, model, short, undetermined, self.part1, self.part2)


def _from_synth(name, n, seed):
    w = synth.generate(name, n, seed=seed)
    iw = synth.CONFIGS[name].get("iw", 8)
    keys = np.concatenate([t.numpy()[:, :iw] for t in w.seq], axis=1)
    quals = np.concatenate([t.numpy()[:, :iw] for t in w.qual], axis=1)
    return Planted(w.plan, w.barcode_strings(), n, seed, keys=keys, quals=quals)


def comb_sheet():
    """8 x 12 with six combinations left off"""
    left_off = {(0, 0), (1, 5), (3, 3), (4, 11), (7, 0), (7, 11)}
    return [_word(7 * a + 3, 8) + _word(11 * b + 600, 8) for a in range(8) for b in range(12) if (a, b) not in left_off]


@functools.lru_cache(maxsize=None)
def case(name, n=N):
    """the workloads, built once: (Planted, force_generic)"""
    dual8 = synth.config_plan("cfg3")
    if name in ("cfg3", "wide10"):  # 8 + 8 with S = 96; 10 + 10: part 1 crosses a word boundary and part 2 starts at byte 10
        return _from_synth(name, n, seed=4100 + n), 0
    if name == "w6_8":
        return Planted(hb.make_plan(True, 25, (0, 6), (0, 8)), [_word(5 * i + 1, 6) + _word(9 * i + 2, 8) for i in range(40)], n, 42), 0
    if name == "generic17":  # a part of three words: the generic kernel's envelope, index 1 at offset 2 of its read
        return Planted(hb.make_plan(True, 25, (2, 19), (0, 8)), [_word(1000003 * i + 5, 17) + _word(13 * i + 7, 8) for i in range(24)], n, 43), 1
    if name == "comb":
        return Planted(dual8, comb_sheet(), n, 44), 0
    if name == "off_matrix":  # barcodes of 15, 13 and 8 bases between the K-long ones: they take no part
        bcs = [_word(3 * i + 1, 8) + _word(5 * i + 2, 8) for i in range(12)]
        bcs[3:3] = ["GGTTGGTTCCAACCA", "TTGGTTGGAACCA"]
        bcs.append("CCGGCCGG")
        return Planted(dual8, bcs, n, 45), 0
    if name == "far64":  # a sheet without collisions under budgets (1, 1)
        return Planted(dual8, synth.make_far_barcodes(64, 8, 8, 1, 1, seed=1), n, 46), 0
    raise KeyError(name)


def launch(torch, eng, seq, qual, n, lens=None, short=None, stream=0):
    """one qd_demux_device / _ragged call; returns the codes tensor -- not synchronised"""
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
    return codes, mol


def np_codes(codes, n):
    return codes[0].cpu().numpy().view(np.uint16)[:n]


def setup(eng, p, generic=0, budgets=None, hop=True, unknown=0):
    eng.set_plan(p.plan)
    eng.set_barcodes(p.bcs)
    eng.set_option("force_generic", int(generic))
    if budgets:
        eng.set_mismatches(*budgets)
    if unknown:
        eng.unknown_enable(unknown)
    if hop:
        eng.hop_enable(True)
        assert eng.hop_shape() == (p.n1, p.n2)


def short_list(torch, p):
    return torch.from_numpy(p.short_idx.astype(np.int64)).to(torch.int32).cuda()


# ---- 1. the table equals the model, sheet by sheet and plan by plan -------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg3", "wide10", "w6_8", "generic17", "comb", "off_matrix"])
def test_table_equals_the_model(torch_cuda, engine, name):
    """qd_demux_device over whole reads, then qd_demux_device_ragged with 3 % of the reads cut: the zero-padded rows go to `short`"""
    torch = torch_cuda
    p, generic = case(name)
    setup(engine, p, generic)
    assert engine.kernel_kind(False) == ("generic" if generic else "fast")
    for cut in (False, True):
        codes_o, counts_o, model, short, _ = p.oracle(cut)
        planted = sum(model.values()) + short
        assert model[p.hot] >= 0.30 * 0.9 * 0.25 * p.n and planted >= 0.2 * p.n, (model[p.hot], planted)
        assert (short > 0) == cut
        both = sum(c for (a, b), c in model.items() if a < p.n1 and b < p.n2)
        assert both > model[p.hot] and model[(p.n1, p.n2)] > 0 and len(model) > 8
        assert any(a < p.n1 and b == p.n2 for a, b in model) and any(a == p.n1 and b < p.n2 for a, b in model)
        engine.reset_counts()
        seq, qual, lens = p.rows(torch, engine.layout, cut)
        codes = launch(torch, engine, seq, qual, p.n, lens if cut else None, short_list(torch, p) if cut else None)
        engine.synchronize()
        assert (np_codes(codes, p.n) == codes_o).all()
        counts = engine.counts()
        assert (counts == counts_o).all()
        p.check(engine.hop_read(), model, short, counts[3])


def test_one_pair_and_no_pair(torch_cuda, engine):
    torch = torch_cuda
    p, _ = case("cfg3", 1)
    setup(engine, p)
    codes_o, counts_o, model, short, _ = p.oracle(False)
    assert sum(model.values()) == 1  # the one pair is a planted one
    seq, qual, lens = p.rows(torch, engine.layout)
    launch(torch, engine, seq, qual, 0)
    engine.synchronize()
    assert not engine.hop_read().any()
    launch(torch, engine, seq, qual, 1)
    engine.synchronize()
    p.check(engine.hop_read(), model, short, engine.counts()[3])


# ---- 2. paths: pinned slots, streams, accumulation and reset --------------------------------------------------------------------
def test_pinned_slots_streams_and_reset(torch_cuda, engine):
    torch = torch_cuda
    p, _ = case("cfg3")
    setup(engine, p)
    codes_o, counts_o, model, short, _ = p.oracle(False)
    seq, qual, _ = p.rows(torch, engine.layout)
    B = 8192
    # qd_submit through 3 pinned slots, every slot's launch on its own stream
    engine.slots_create(3, B)
    host = [(s.cpu().numpy(), q.cpu().numpy()) for s, q in zip(seq, qual)]
    for i, a in enumerate(range(0, p.n, B)):
        b, s = min(p.n, a + B), i % 3
        if i >= 3:
            engine.wait(s)
        v = engine.slot(s)
        for k in range(2):
            v["seq"][k][:b - a] = host[k][0][a:b]
            v["qual"][k][:b - a] = host[k][1][a:b]
        engine.submit(s, b - a)
    for s in range(3):
        engine.wait(s)
    assert (engine.counts() == counts_o).all()
    p.check(engine.hop_read(), model, short, counts_o[3])
    engine.slots_destroy()
    # two launches on two caller streams into one table
    engine.reset_counts()
    assert not engine.hop_read().any()
    half = 35008  # (rows of 8 bytes: the second launch's rows start 16-byte aligned)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep = [launch(torch, engine, [t[a:b] for t in seq], [t[a:b] for t in qual], b - a, stream=streams[i].cuda_stream)
            for i, (a, b) in enumerate(((0, half), (half, p.n)))]
    engine.synchronize()
    assert (np.concatenate([np_codes(keep[0], half), np_codes(keep[1], p.n - half)]) == codes_o).all()
    p.check(engine.hop_read(), model, short, engine.counts()[3])
    # three launches, then qd_reset_counts, then one launch
    for _ in range(2):
        launch(torch, engine, seq, qual, p.n)
    engine.synchronize()
    p.check(engine.hop_read(), HM.Counter({k: 3 * c for k, c in model.items()}), 3 * short, engine.counts()[3])
    engine.reset_counts()
    launch(torch, engine, seq, qual, p.n)
    engine.synchronize()
    p.check(engine.hop_read(), model, short, engine.counts()[3])


# ---- 3. with budgets (1, 1); with the unknown tally; with the option off --------------------------------------------------------
def test_rescued_pairs_are_not_in_the_table(torch_cuda, engine, monkeypatch):
    """With budgets (1, 1) the rescued pairs leave the table, and a pair within 1 of a part that stays Undetermined counts as
    no match for that part: the model is the exact one over the tolerant oracle's Undetermined pairs."""
    torch = torch_cuda
    p, _ = case("far64", 30011)
    exact = p.oracle(True)
    args = []
    for s, q in p.reads(True):
        args += [[x.decode() for x in s], [x.decode() for x in q]]
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, p.K, p.w1, 1, 1))
    codes_t, idx_t, _, counts_t = H.oracle_on_reads(p.bcs, p.plan, *args)
    monkeypatch.undo()
    model, short = HM.model_from_oracle(codes_t, idx_t, p.K, p.w1, p.P1, p.P2)
    assert sum(exact[2].values()) > sum(model.values()) > 0 and short == exact[3] > 0
    # planted: part 1 one substitution from a sample's, part 2 another sample's -- Undetermined, and row n1
    assert sum(c for (a, b), c in model.items() if a == p.n1 and b < p.n2) > 0
    setup(engine, p, budgets=(1, 1))
    seq, qual, lens = p.rows(torch, engine.layout, True)
    for generic in (False, True):
        engine.reset_counts()
        codes = launch(torch, engine, seq, qual, p.n, lens, None if generic else short_list(torch, p))
        engine.synchronize()
        assert (np_codes(codes, p.n) == codes_t).all()
        p.check(engine.hop_read(), model, short, engine.counts()[3])
    engine.set_mismatches(0, 0)  # the matrix stays on: now the exact model
    engine.reset_counts()
    launch(torch, engine, seq, qual, p.n, lens, short_list(torch, p))
    engine.synchronize()
    p.check(engine.hop_read(), exact[2], exact[3], engine.counts()[3])


def test_beside_the_unknown_tally_and_switched_off(torch_cuda, engine):
    """Matrix and tally together: both tables are right and the tally's is what it is with the matrix off.  With the matrix off,
    codes, counters and the tally's table are those of a run that never enabled it, and qd_hop_read gives QD_ERR_STATE."""
    torch = torch_cuda
    p, _ = case("cfg3")
    codes_o, counts_o, model, short, idx_o = p.oracle(True)
    umodel, ushort = UM.model_from_oracle(codes_o, idx_o, p.K)
    seen = {}
    for step in ("never", "on", "off"):
        if step == "never":
            setup(engine, p, hop=False, unknown=1 << 16)
        else:
            engine.hop_enable(step == "on")
            engine.reset_counts()
        seq, qual, lens = p.rows(torch, engine.layout, True)
        codes = launch(torch, engine, seq, qual, p.n, lens, short_list(torch, p))
        engine.synchronize()
        keys, kc = engine.unknown_read()
        got = (np_codes(codes, p.n).copy(), codes[1].cpu().numpy().copy(), engine.counts(), UM.table_counter(keys, kc), engine.unknown_stats())
        UM.check_exact(got[3], got[4], umodel, ushort, got[2][3])
        if step == "on":
            p.check(engine.hop_read(), model, short, got[2][3])
        else:
            for call in (engine.hop_read, engine.hop_shape, lambda: engine.hop_add(np.zeros(hb.hop_values(p.n1, p.n2), np.uint64))):
                with pytest.raises(hb.QuadeHipError) as ei:
                    call()
                assert ei.value.code == hb.QD_ERR_STATE
        first = seen.setdefault("first", got)
        assert (got[0] == first[0]).all() and (got[1] == first[1]).all() and (got[2] == first[2]).all()
        assert got[3] == first[3] and (got[4] == first[4]).all()
    assert (seen["first"][0] == codes_o).all()


# ---- 4. state -----------------------------------------------------------------------------------------------------------------------
def test_state_and_add(torch_cuda):
    torch = torch_cuda
    p, _ = case("comb")
    with hb.Engine(0) as eng, hb.Engine(0) as other:
        for call in (eng.hop_read, eng.hop_shape, eng.hop_enable):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        eng.set_plan(p.plan)
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.hop_enable()
        assert ei.value.code == hb.QD_ERR_STATE
        # a single-index plan
        eng.set_plan(hb.make_plan(False, 25, (0, 8)))
        eng.set_barcodes(["ACGTACGT", "TTTTCCCC"])
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.hop_enable()
        assert ei.value.code == hb.QD_ERR_INVALID
        eng.hop_enable(False)
        # qd_set_barcodes and qd_set_plan after enable turn it off
        for turn_off in (lambda: eng.set_barcodes(p.bcs), lambda: (eng.set_plan(p.plan), eng.set_barcodes(p.bcs))):
            setup(eng, p)
            turn_off()
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.hop_read()
            assert ei.value.code == hb.QD_ERR_STATE
        # a second context's table joins: the model over both inputs
        half = p.n // 2
        setup(eng, p)
        setup(other, p)
        parts = []
        for e, (lo, hi) in ((eng, (0, half)), (other, (half, p.n))):
            seq, qual, _ = p.rows(torch, e.layout, False, lo, hi)
            launch(torch, e, seq, qual, hi - lo)
            e.synchronize()
            parts.append(e.hop_read())
        codes_o, counts_o, model, short, _ = p.oracle(False)
        for bad in (parts[1][:-1], np.zeros(3, np.uint64)):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.hop_add(bad)
            assert ei.value.code == hb.QD_ERR_INVALID
        eng.hop_add(parts[1])
        assert (eng.hop_read() == parts[0] + parts[1]).all()
        p.check(eng.hop_read(), model, short, counts_o[3])
        assert (other.hop_read() == parts[1]).all()


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------
def _fastq_reads(path):
    """(sequences, qualities) of the records a reader keeps: those whose sequence and quality lines have one length"""
    with gzip.open(path, "rt") as fh:
        lines = fh.read().split("\n")
    kept = [(s, q) for s, q in zip(lines[1::4], lines[3::4]) if len(s) == len(q)]
    return [s for s, _ in kept], [q for _, q in kept]


def _expected_report(bcs, names, plan, reads, budgets=(0, 0)):
    """the report module fed with the model's table: the model run over the index reads"""
    codes, idx, _, counts = H.oracle_on_reads(bcs, plan, *reads)
    w1 = plan.idx1_end - plan.idx1_start
    K = w1 + plan.idx2_end - plan.idx2_start
    P1, P2, part1, part2 = HM.part_lists(bcs, K, w1)
    model, short = HM.model_from_oracle(codes, idx, K, w1, P1, P2)
    assert sum(model.values()) + short == int(counts[3])
    table = HM.model_table(model, short, len(P1), len(P2))
    lines = hr.report_lines(table, len(P1), len(P2), part1, part2, list(zip(names, bcs)), w1, budgets, int(counts[0]),
                            [int(counts[4 + 2 * i]) + int(counts[5 + 2 * i]) for i in range(len(bcs))])
    return "\n".join(lines) + "\n", model


@pytest.mark.parametrize("path", ["device_pipeline", "pinned_slots"])
def test_cli_bundled_golden_run(torch_cuda, tmp_path, bundled_dir, path):
    from tests.run_support import _compare_dirs, _run_cli
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt")) as fh:
        base = fh.read()
    assert "[output]\n" in base
    extra = "" if path == "device_pipeline" else "\n[gpu]\ndevice_pipeline : False\n"
    reads = [[], [], [], []]
    for c in (1, 2, 3):  # index read 1 is R2, index read 2 is R3; pair j of a chunk is kept record j of each of its four files
        kept = {r: _fastq_reads(os.path.join(bundled_dir, "dataset", "C%d_%s.fastq.gz" % (c, r))) for r in ("R1", "R2", "R3", "R4")}
        pairs = min(len(s) for s, _ in kept.values())
        for k, r in enumerate(("R2", "R3")):
            reads[2 * k] += kept[r][0][:pairs]
            reads[2 * k + 1] += kept[r][1][:pairs]
    plan = hb.make_plan(True, 25, (0, 4), (0, 4), (3, 6), (3, 6))
    want, model = _expected_report(["ACAGACAG", "CTTGCTTG"], ["S1", "S2"], plan, reads)
    assert sum(model.values()) == 247  # (all of them in (n1, n2): neither index of the dataset's other pairs is on the sheet)
    for opt in (True, False):
        work = tmp_path / ("with" if opt else "without")
        work.mkdir()
        conf = work / "conf.txt"
        conf.write_text((base.replace("[output]\n", "[output]\nindex_hopping_report : True\n", 1) if opt else base) + extra)
        _run_cli(str(conf), str(work))
        os.remove(conf)
        _compare_dirs(str(work), os.path.join(bundled_dir, "result"))  # every fastq.gz byte for byte, Quade_report.csv as before
        report = work / hr.REPORT_NAME
        if opt:
            assert report.read_text() == want
        else:
            assert not report.exists()


def _synthetic_dataset(d, seed, n_chunks, n):
    """n_chunks x n pairs with dual 8 bp indexes over a 6 x 5 combinatorial sheet with four combinations left off: matches, swapped
    partners, unknown partners, lower case, N and cut index reads"""
    from tests.run_support import _write_fastq
    rng = np.random.default_rng(seed)
    c1, c2 = [_word(17 * i + 4, 8) for i in range(6)], [_word(29 * i + 300, 8) for i in range(5)]
    samples = [("S%d" % (5 * a + b), c1[a], c2[b]) for a in range(6) for b in range(5) if (a, b) not in {(0, 0), (2, 3), (5, 4), (5, 1)}]
    r1, r2 = _rows(c1), _rows(c2)
    files = {"seq_R1": [], "seq_R2": [], "index_R1": [], "index_R2": []}
    reads = [[], [], [], []]
    for c in range(n_chunks):
        names = ["SIM:1:FC:%d:%d:%d" % (c, i, i * 7) for i in range(n)]
        i1, i2 = r1[rng.integers(0, 6, n)].copy(), r2[rng.integers(0, 5, n)].copy()
        kind = rng.integers(0, 100, n)
        sel = np.flatnonzero(kind < 5)
        i2[sel] = ACGT[rng.integers(0, 4, (sel.size, 8))]
        sel = np.flatnonzero((kind >= 5) & (kind < 10))
        i1[sel] = ACGT[rng.integers(0, 4, (sel.size, 8))]
        sel = np.flatnonzero((kind >= 10) & (kind < 14))
        i1[sel, rng.integers(0, 8, sel.size)] |= 0x20
        sel = np.flatnonzero((kind >= 14) & (kind < 17))
        i2[sel, rng.integers(0, 8, sel.size)] = ord("N")
        cut = np.where(kind >= 97, rng.integers(0, 8, n), 8)
        q = (rng.integers(20, 41, (4, n, 8)) + 33).astype(np.uint8)
        ins = ACGT[rng.integers(0, 4, (2, n, 8))]
        rows = {"seq_R1": (ins[0], q[0], None), "seq_R2": (ins[1], q[1], None), "index_R1": (i1, q[2], cut), "index_R2": (i2, q[3], None)}
        for k, (s, qq, ln) in rows.items():
            ss = [bytes(x).decode() for x in s]
            qs = [bytes(x).decode() for x in qq]
            if ln is not None:
                ss, qs = [x[:m] for x, m in zip(ss, ln)], [x[:m] for x, m in zip(qs, ln)]
            path = os.path.join(d, "C%d_%s.fastq.gz" % (c, k))
            _write_fastq(path, names, ss, qs)
            files[k].append(path)
            if k.startswith("index"):
                j = 0 if k == "index_R1" else 2
                reads[j] += ss
                reads[j + 1] += qs
    return files, samples, reads


def _launch_ranks(conf, work, n, env_extra):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "quade_amd.launch", "-n", str(n), "-c", str(conf)], cwd=str(work), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])


def _n_devices():
    try:
        return hb.device_count()
    except Exception:  # no library / no GPU: the module is only collected then (every test is marked gpu)
        return 0


@pytest.fixture(scope="module")
def synthetic_run(tmp_path_factory):
    """about 20 000 pairs in 3 chunks, the conf files of every mode, and the expected report"""
    from tests.run_support import _conf
    d = tmp_path_factory.mktemp("hop_cli")
    files, samples, reads = _synthetic_dataset(str(d), 1234, 3, 6700)
    want, model = _expected_report([a + b for _, a, b in samples], [nm for nm, _, _ in samples], synth.config_plan("cfg3"), reads)
    assert sum(c for (a, b), c in model.items() if a < 6 and b < 5) > 1000

    def conf(mode, gpu):
        path = d / (mode + ".txt")
        _conf(str(path), files, True, ((1, 8), (1, 8), None, None), 25, samples, gpu="[gpu]\n" + gpu)
        path.write_text(path.read_text().replace("[output]\n", "[output]\nindex_hopping_report : True\n", 1))
        work = d / mode
        work.mkdir()
        return str(path), str(work)

    return conf, want


@pytest.mark.parametrize("mode,gpu", [("one", "batch_pairs : 3000\n"), ("workers", "chunk_workers : 2\nbatch_pairs : 3000\n"),
                                      ("slots", "device_pipeline : False\nbatch_pairs : 3000\n"),
                                      ("ranks_one_gpu", "batch_pairs : 3000\n")])
def test_cli_synthetic_run(torch_cuda, synthetic_run, mode, gpu):
    """one context, chunk_workers : 2, the pinned slots, and two ranks on GPU 0 over the files transport: the same file each time"""
    from tests.run_support import _run_cli
    conf, want = synthetic_run
    path, work = conf(mode, gpu)
    if mode == "ranks_one_gpu":
        _launch_ranks(path, work, 2, {"QUADE_DIST_TRANSPORT": "files", "QUADE_DEVICE": "0"})
    else:
        _run_cli(path, work)
    with open(os.path.join(work, hr.REPORT_NAME)) as fh:
        assert fh.read() == want


@pytest.mark.skipif(_n_devices() < 2, reason="needs at least two visible GPUs (RCCL wants one rank per device)")
def test_cli_two_ranks_two_gpus(torch_cuda, synthetic_run):
    conf, want = synthetic_run
    path, work = conf("ranks", "batch_pairs : 3000\n")
    _launch_ranks(path, work, 2, {})
    with open(os.path.join(work, hr.REPORT_NAME)) as fh:
        assert fh.read() == want
