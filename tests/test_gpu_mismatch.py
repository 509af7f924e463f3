"""Mismatch-tolerant matching on the MI355X: routing codes, molecular bytes and counters equal to the oracle with the tolerant
lookup of tests/mismatch_model.py installed (qo.SampleSet monkeypatched; the oracle itself is unmodified), on every path that
launches the match kernels: fast and generic kernels, ragged batches, pinned slots, and the command line's device pipeline."""
import gzip
import os

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from quade_amd import synth
from tests import helpers as H
from tests import mismatch_model as MM
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
