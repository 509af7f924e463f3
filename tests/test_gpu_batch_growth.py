"""A batch whose output needs more than the reservation gave (quade_amd/csrc/quade_pipe.cpp: reserve_buffers, then need_pair_buffers /
need_scan_tables / need_out_buffers once more per batch, all sized by batch_sizes.h).  The run's buffers are reserved once, from what a
record of every stream weighs at the head of the first chunk's files; here that chunk holds 200 pairs of 36-base reads and the second
2 500 pairs of 151-base reads, three batches at batch_pairs 1024.  What outgrows the reservation, by batch_sizes.h: the output set's
text (reserved for 1024 pairs of ~105-byte records, ~0.23 MB; a batch of the long records formats to ~0.7 MB) and with it the coder's
sub-block tables and scratch (subs, ranges, crc, sub_out, sub_bytes: reserved for T / 64 KiB + 16 sub-blocks).  What does not: the
pair-sized tables (most_pairs adds 1024 pairs to what the largest seq_R1 file holds, so it is batch_pairs here), the windows and scan
tables (reserved with 96 MiB to spare) and the member slots (16 pieces reserved, 14 regions at most).  The statistics do not show a
growth; the test holds the bytes.  Once with the stages off against the oracle's directory, as tests/test_gpu_geometry.py compares it,
and once with clip, post-trim and filter on -- their tables are part of the reservation then -- against those stages' models chained
in the pipeline's order."""
import os

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import clip_report as cr
from quade_amd import filter_report as fr
from quade_amd import hip_backend as hb
from quade_amd import posttrim_report as xr
from tests import clip_model as CM
from tests import filter_model as FM
from tests import posttrim_model as XM
from tests import stage_support as SS
from tests.run_support import _compare_dirs, _conf, _gz, _write_fastq
from tests.stage_support import _cli, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

B = 1024
CHUNKS = ((200, 36), (2500, 151))  # (pairs, bases per insert read)
GPU = "[gpu]\nbatch_pairs : %d\ngzip_level : 1\n" % B
CLIP = "front_clip_R2 : 5\ntail_clip_R1 : 1\nwindow_size : 4\nwindow_quality : 18\npoly_g : True\n"
P_CLIP = CM.Params(front_clip=(0, 5), tail_clip=(1, 0), window_size=4, window_quality=18, poly_g_min_length=10, min_length=25)
POST = "tail_n : True\npoly_x : True\nmax_length_R1 : 100\nmax_length_R2 : 90\nmin_length : 25\n"
P_POST = XM.Params(tail_n=1, poly_x_min_length=10, max_length=(100, 90), min_length=25)
FILTER = "[filter]\nmin_length : 30\nmax_n : 2\nmin_mean_quality : 20\n"
P_F = FM.Params(min_length=30, max_n=2, min_mean_quality=20)


def _insert(g, i, L):
    """a read of L bases with food for the three stages: N inside, trailing N, a poly-G tail, a low-quality 3' tail, low qualities
    throughout"""
    s, qual = g.rnd(L), g.q(L, 22, 42)
    if i % 7 == 0:
        for p in g.rng.integers(0, L * 2 // 3, 4):
            s = s[:int(p)] + "N" + s[int(p) + 1:]
    if i % 4 == 1:
        k = int(g.rng.integers(1, 9))
        s = s[:L - k] + "N" * k
    elif i % 8 == 2:
        k = int(g.rng.integers(10, 16))
        s = s[:L - k] + "G" * k
    elif i % 5 == 3:
        k = int(g.rng.integers(4, L // 3))
        qual = g.q(L - k, 22, 42) + g.q(k, 2, 16)
    elif i % 13 == 6:
        qual = g.q(L, 17, 22)
    return s, qual


def _dataset(d, seed):
    """CHUNKS as four BGZF files per chunk, dual 8 + 8 index over 3 far barcodes -> (files, samples)"""
    rng = np.random.default_rng(seed)
    g = SS.Draw(rng)
    bcs = sorted(set(SS.MM_far_barcodes()))[:3]
    os.makedirs(d, exist_ok=True)
    files = {"seq_R1": [], "seq_R2": [], "index_R1": [], "index_R2": []}
    for c, (n, L) in enumerate(CHUNKS):
        names = ["SIM:1:FC:%d:%d:%d" % (c, i, i * 7) + "x" * (i % 5) for i in range(n)]
        streams = {k: ([], []) for k in files}
        for i in range(n):
            sample, kind = int(rng.integers(0, len(bcs))), int(rng.integers(0, 10))
            for key in ("seq_R1", "seq_R2"):
                s, qual = _insert(g, i, L)
                streams[key][0].append(s)
                streams[key][1].append(qual)
            for k, key in enumerate(("index_R1", "index_R2")):
                streams[key][0].append(g.rnd(8) if kind == 0 else bcs[sample][k])  # (0: a random index)
                streams[key][1].append(g.q(8, 15 if kind in (2, 3) else 30, 41))   # (2, 3: low index qualities)
        for key, (ss, qs) in streams.items():
            p = os.path.join(d, "C%d_%s.fastq.gz" % (c, key))
            _write_fastq(p, names, ss, qs)
            text = _gz(p)
            assert hb.load_library().qd_write_gzip_file(p.encode(), hb._ptr(np.frombuffer(text, dtype=np.uint8)), len(text), 1, -1) == 0
            files[key].append(p)
    return files, [("S%d" % i, b1, b2) for i, (b1, b2) in enumerate(bcs)]


def _write_conf(path, files, samples, extra=""):
    _conf(str(path), files, True, ((1, 8), (1, 8), None, None), 25, samples, gpu=GPU)
    if extra:
        with open(str(path), "a") as fh:
            fh.write(extra)


@pytest.fixture(scope="module")
def data(torch_cuda, tmp_path_factory):
    """the dataset, the conf without the stages and the oracle's run of it: both tests' reference"""
    top = tmp_path_factory.mktemp("batch_growth")
    files, samples = _dataset(str(top / "data"), 27)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples)
    ref = top / "ref"
    ref.mkdir()
    sset, _ = qo.run_quade(str(plain), outdir=str(ref))
    counts = sset.counts()
    assert counts[0] == sum(n for n, _ in CHUNKS) and all(v > 0 for v in counts[1:4])  # pass, fail and Undetermined
    return dict(top=top, files=files, samples=samples, plain=plain, ref=ref, counts=counts)


def test_stages_off_equals_the_oracle(data, tmp_path):
    from quade_amd.quade import Quade
    from quade_amd.sample import Sample
    mine = tmp_path / "mine"
    mine.mkdir()
    old = os.getcwd()
    os.chdir(str(mine))
    try:
        q = Quade(conf_file=str(data["plain"]))
        assert q() == 0
    finally:
        os.chdir(old)
    assert Sample.COUNTS() == data["counts"]
    _compare_dirs(str(mine), str(data["ref"]))
    assert q.use_pipe
    st = q.pipe_stats
    print("\nbatch growth, stages off: %s" % " ".join("%s=%d" % (k, st[k]) for k in ("pairs", "batches", "rescans", "bgzf_blocks", "pieces", "host_coded_pieces")))
    assert st["pairs"] == sum(n for n, _ in CHUNKS)
    assert st["batches"] == sum((n + B - 1) // B for n, _ in CHUNKS) == 4, st  # one of short records, then three of long ones
    assert st["bgzf_blocks"] > 0 and st["host_inflated_runs"] == 0 and st["text_segments"] == 0 and st["host_coded_pieces"] == 0, st


def test_clip_posttrim_and_filter_on_equal_the_chained_models(data, tmp_path):
    names = [s[0] for s in data["samples"]]
    clipped, ctable = CM.clipped_outputs(str(data["ref"]), P_CLIP)
    post, xtable = XM.posttrimmed_outputs(CM.write_outputs(clipped, str(tmp_path / "clipped")), P_POST)
    texts, table, _, _ = FM.filtered_outputs(XM.write_outputs(post, str(tmp_path / "post")), names, P_F)
    # every stage acts, in both chunks' read lengths, and the filter keeps and drops pairs
    raw = {f: _gz(os.path.join(str(data["ref"]), f)) for f in clipped}
    assert all(clipped[f] != raw[f] for f in raw) and any(post[f] != clipped[f] for f in post)
    t = np.array(table, dtype=np.int64)
    assert 0 < int(t[:, 1:6].sum()) < int(t[:, 0].sum()) == data["counts"][0]
    conf = tmp_path / "conf.txt"
    _write_conf(conf, data["files"], data["samples"], extra="[trim]\n" + CLIP + POST + FILTER)
    mine = tmp_path / "mine"
    _cli(conf, mine)
    SS._check_files(mine, texts)
    SS._check_main_report(mine, data["ref"])
    SS._check_report(mine, cr, ctable, P_CLIP.keywords())
    SS._check_report(mine, xr, xtable, P_POST.keywords())
    SS._check_report(mine, fr, table, names, P_F.keywords())
