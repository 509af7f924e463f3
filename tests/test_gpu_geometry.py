"""The chunk loop of the device pipeline (run_chunk in quade_amd/csrc/quade_pipe.cpp) on records that are not all one size: the
profiles of tests/record_geometry.py, each through one CLI run per file format, against oracle.run_quade's directory byte for byte --
and, from the run's statistics, that the run went where the profile aims (without that a pass proves nothing).

What the statistics can show at these sizes.  A window takes its text in whole uploads: 16 MiB of compressed bytes (BGZF blocks, or a
gzip member's bytes, which one step inflates as far as they reach) or a read of 8 MiB of plain text, and every turn of the loop asks
for more than the window holds, so it brings at least one upload while the stream has any.  Every stream of the six profiles of the
issue is smaller than an upload: its first upload is the whole stream, the next turn finds its end, and from then on no window is
short of records while its stream has more (step 3 of the loop).  No batch but a chunk's last is short of batch_pairs then:
batches == sum of ceil(pairs / B) over the chunks, in every format.  That is asserted, in place of "batches > ceil(pairs / B)" for
`regimes` and `dropped_runs`: a batch accepted short of B with input left needs B kept records that outweigh an upload (with B = 97,
86 KB of plain text or 170 KB of compressed bytes per kept record), which streams of 3 000 ordinary records cannot hold.  What these
profiles do reach follows from windows that hold far more, or far fewer, records than the learned bytes per record promise:
windows of dozens of batches beside windows of one, chunks that end with one stream while another holds thirty times more, a line
table outgrown (rescans), a chunk of no pairs, streams shifted by six batches.

The seventh profile, `sparse`, is there for the short batches: seq_R2 keeps one record in 26 and then one in 51, so as plain text an
upload brings 83 and then 42 kept records to a batch of 97 (test_host_geometry counts them).  The loop takes 83 as most of a batch,
three times, and tops the window up once more where 42 arrive: batches > ceil(pairs / B) there.  Compressed, its filler shrinks to
one upload and the rule of the other profiles holds again."""
import os

import pytest

from oracle import quade_oracle as qo
from tests import record_geometry as G
from tests.run_support import _compare_dirs, _conf

pytestmark = pytest.mark.gpu

SEED = 20
RUNS = [(name, fmt) for name in G.NAMES for fmt in (G.FORMATS if name in ("ragged", "ends", "dropped_runs", "sparse") else ("bgzf", "gz"))]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """expected(name) -> (the oracle's output directory, its counters) for a profile: run once per profile on the plain texts, which
    are the same in every format"""
    done = {}

    def expected(name):
        if name not in done:
            p = G.profile(name, SEED)
            d = tmp_path_factory.mktemp("oracle_" + name)
            files = G.write(p, d, "plain")
            conf = os.path.join(str(d), "conf.txt")
            _conf(conf, files, True, G.POSITIONS, G.MIN_QUAL, p.samples)
            ref = os.path.join(str(d), "ref")
            os.mkdir(ref)
            sset, _ = qo.run_quade(conf, outdir=ref)
            assert sset.counts()[0] == p.facts["pairs"]
            assert all(v > 0 for v in sset.counts()[1:4])  # pass, fail and Undetermined
            done[name] = (ref, sset.counts())
        return done[name]
    return expected


def _run(tmp_path, name, fmt, gpu, oracle):
    """one CLI run of the profile's files in that format; the outputs and counters are the oracle's"""
    from quade_amd.quade import Quade
    from quade_amd.sample import Sample
    p = G.profile(name, SEED)
    ref, counts = oracle(name)
    data, mine = tmp_path / "data", tmp_path / "mine"
    data.mkdir()
    mine.mkdir()
    files = G.write(p, data, fmt)
    conf = str(tmp_path / "conf.txt")
    _conf(conf, files, True, G.POSITIONS, G.MIN_QUAL, p.samples, gpu="[gpu]\nbatch_pairs : %d\n%s" % (p.batch_pairs, gpu))
    old = os.getcwd()
    os.chdir(str(mine))
    try:
        q = Quade(conf_file=conf)
        assert q() == 0
    finally:
        os.chdir(old)
    assert Sample.COUNTS() == counts
    _compare_dirs(str(mine), ref)
    return p, q


@pytest.mark.parametrize("name,fmt", RUNS)
def test_device_pipeline_equals_the_oracle(tmp_path, name, fmt, oracle):
    p, q = _run(tmp_path, name, fmt, "", oracle)
    assert q.use_pipe
    st = q.pipe_stats
    print("\ngeometry %s %s: %s" % (name, fmt, " ".join("%s=%d" % (k, st[k]) for k in (
        "pairs", "batches", "rescans", "text_segments", "gzip_steps", "gzip_members", "gzip_fallbacks", "bgzf_blocks", "host_inflated_runs",
        "pieces", "host_coded_pieces"))))
    B, per_chunk = p.batch_pairs, p.facts["pairs_per_chunk"]
    assert st["pairs"] == p.facts["pairs"] == sum(per_chunk)
    if (name, fmt) == ("sparse", "plain"):  # uploads of fewer kept records than B: batches short of B with input left
        assert st["batches"] > (p.facts["pairs"] + B - 1) // B, st
        assert st["text_segments"] >= 3 + len(p.facts["kept_per_upload"]) + 1, st
    else:  # every stream of every chunk is one upload (the module's docstring): no batch but a chunk's last is short of B
        assert st["batches"] == sum((n + B - 1) // B for n in per_chunk), st
    if fmt == "bgzf":
        assert st["bgzf_blocks"] > 0 and st["host_inflated_runs"] == 0 and st["text_segments"] == 0, st
    elif fmt == "gz":
        assert st["gzip_fallbacks"] == 0 and st["gzip_members"] == 4 * p.n_chunks and st["text_segments"] == 0, st  # every file is opened
    else:
        assert st["text_segments"] >= 4 * p.n_chunks and st["bgzf_blocks"] == 0 and st["gzip_steps"] == 0, st  # an upload per file at least
    if name == "chunk_regimes":  # chunk 1's seq_R1 has more lines than the table that chunk 0 left can hold
        assert st["rescans"] >= 1, st
    if name != "giant":  # (giant: whatever the coder makes of a record of 400 KB; the figure is in the pull request's table)
        assert st["host_coded_pieces"] == 0, st


@pytest.mark.parametrize("name", G.NAMES)
def test_pinned_slots_path_equals_the_oracle(tmp_path, name, oracle):
    """the batch pipeline over pinned slots reads the same files with the host's readers: same outputs"""
    p, q = _run(tmp_path, name, "gz", "device_pipeline : False\n", oracle)
    assert not q.use_pipe
