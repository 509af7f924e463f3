"""The device pipeline on compressed inputs that span several uploads: the framings of tests/upload_seams.py (proven on the host by
tests/test_host_upload_seams.py), each through one CLI run with batch_pairs 97, against oracle.run_quade's directory byte for byte
and its counters -- and, from the run's statistics, that the run went where the framing aims.  One oracle run per text set.

What each framing reaches in quade_amd/csrc/quade_pipe.cpp (Feeder::feed_bgzf / feed_gzip with feed_cut.h's cutter, gz_append / gz_steps / top_up, drain_chunk):

  gz               SEG_GZIP uploads two to four of a file; gz_append joins them at comp_off + comp_len; steps that resume at walk.bit
                   behind bytes that keep_from has moved; the 32 KiB carried window; stepped_end / stuck (an upload ends inside a
                   block); the member's CRC combined over its steps; the fourth upload reuses a page-locked buffer (take_pin)
  bgzf             the partial block behind a buffer's last whole one carried in `tail`; file_pos / seg.file_off above 0
  gz_members       headers and trailers read with pread at file offsets while the payload is on the device: a trailer that ends at a
                   seam, one across a seam, a header across a seam; walk.bit >= 8 * (comp_off + comp_len) (the next member has nothing
                   on the device yet); an empty member; the zero-padding rule
  bgzf_seams       an empty `tail` (a block ends at a buffer's end); fewer than 18 bytes of a header at a buffer's end; 18 or more
                   bytes but not the whole extra field (the feeder took that for "no longer BGZF" and sent the rest of the file down
                   the host's text path: text_segments == 0 is the assertion that caught it)
  bgzf_then_gz     switch_at > 0: text_from(c, path, switch_at) behind blocks that the device inflated
  gz_refused_late  gz_fallback with host_skip = walk.text > 0: the host inflates the member again from its start and the text that
                   was delivered is dropped -- text_in_bytes says that no byte came twice or not at all
  *_damaged_late   a decoder status or a CRC of the second upload fails the run with the file's name; the next run is clean
  ends_early_*     a chunk that ends with index_R2 while the insert streams' uploads are in flight: skip_below, drain_chunk,
                   segments "left over from a chunk that ended early", gz_close with file_done still false
  dense            one buffer whose blocks hold more than SEG_TEXT_MAX of text goes out in several segments

These texts hardly compress, so the coder may hand members to the host: host_coded_pieces is printed, not asserted."""
import gzip
import os
import time

import pytest

from oracle import quade_oracle as qo
from tests import record_geometry as G
from tests import upload_seams as U
from tests.run_support import _compare_dirs, _conf

pytestmark = pytest.mark.gpu

SHOWN = ("pairs", "batches", "gzip_steps", "gzip_units", "gzip_members", "bgzf_blocks", "text_segments", "gzip_fallbacks", "host_inflated_runs",
         "host_coded_pieces", "text_in_bytes")


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    """files(framing): the framing's files, written once per module"""
    made = {}

    def files(framing):
        if framing not in made:
            made[framing] = U.frame(framing, tmp_path_factory.mktemp(framing))
        return made[framing]
    yield files
    U.forget()


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """expected(text set) -> (the oracle's output directory, its counters): one run per text set on the plain texts"""
    done = {}

    def expected(name):
        if name not in done:
            p = U.texts(name)
            d = tmp_path_factory.mktemp("oracle_" + name)
            files = G.write(p, d, "plain")
            conf = os.path.join(str(d), "conf.txt")
            _conf(conf, files, True, G.POSITIONS, G.MIN_QUAL, p.samples)
            ref = os.path.join(str(d), "ref")
            os.mkdir(ref)
            t0 = time.time()
            sset, _ = qo.run_quade(conf, outdir=ref)
            print("\nupload seams: oracle run of %s: %.1f s" % (name, time.time() - t0))
            assert sset.counts()[0] == p.facts["pairs"]
            assert all(v > 0 for v in sset.counts()[1:4])  # pass, fail and Undetermined
            for path in sum(files.values(), []):
                os.remove(path)
            done[name] = (ref, sset.counts())
        return done[name]
    return expected


def _cli(base, files, p, gpu=""):
    """one CLI run in base/mine: (the Quade object, its return value, seconds)"""
    from quade_amd.quade import Quade
    mine = base / "mine"
    base.mkdir(exist_ok=True)
    mine.mkdir()
    conf = str(base / "conf.txt")
    _conf(conf, files, True, G.POSITIONS, G.MIN_QUAL, p.samples, gpu="[gpu]\nbatch_pairs : %d\n%s" % (p.batch_pairs, gpu))
    old = os.getcwd()
    os.chdir(str(mine))
    try:
        q = Quade(conf_file=conf)
        t0 = time.time()
        try:
            rc = q()
        except BaseException:
            for eng in q.engines:  # (a run that fails leaves its contexts open)
                eng.close()
            raise
        return q, rc, time.time() - t0
    finally:
        os.chdir(old)


def _run(base, framing, on_disk, oracle, gpu=""):
    """one CLI run of the framing's files; the outputs and counters are the oracle's.  (text set, Quade object)"""
    from quade_amd.sample import Sample
    p = U.texts(U.FRAMINGS[framing])
    ref, counts = oracle(p.name)
    q, rc, seconds = _cli(base, on_disk(framing), p, gpu)
    assert rc == 0
    assert Sample.COUNTS() == counts
    _compare_dirs(str(base / "mine"), ref)
    st = q.pipe_stats if q.use_pipe else None
    print("\nupload seams %s%s: %.1f s%s" % (framing, " (pinned slots)" if st is None else "", seconds,
                                           "" if st is None else " " + " ".join("%s=%d" % (k, st[k]) for k in SHOWN)))
    return p, q


def _text_bytes(p):
    return sum(len(c[k]) for c in p.chunks for k in G.STREAMS)


def _all_blocks(files):
    return sum(len(G.bgzf_blocks(path)) for k in G.STREAMS for path in files[k])


@pytest.fixture(scope="module")
def gz_run(tmp_path_factory, on_disk, oracle):
    """the statistics of framing gz's run: the test of gz itself, the control of gz_refused_late and what the run without
    inflate_overlap is compared with"""
    p, q = _run(tmp_path_factory.mktemp("gz_run"), "gz", on_disk, oracle)
    assert q.use_pipe
    return q.pipe_stats


def test_gz_one_member_per_stream(gz_run, on_disk):
    p, st, files = U.texts("long"), gz_run, on_disk("gz")
    assert st["pairs"] == p.facts["pairs"]
    assert st["gzip_members"] == 4 and st["gzip_fallbacks"] == 0 and st["text_segments"] == 0 and st["bgzf_blocks"] == 0, st
    # a top-up stops after one upload (test_host_upload_seams: its precondition), so every upload gets a step of its own at least
    assert st["gzip_steps"] >= sum(U.uploads(files[k][0]) for k in G.STREAMS) == 8, st
    assert st["text_in_bytes"] == _text_bytes(p), st


def test_bgzf_by_the_librarys_writer(tmp_path, on_disk, oracle):
    p, q = _run(tmp_path, "bgzf", on_disk, oracle)
    st = q.pipe_stats
    assert q.use_pipe and st["pairs"] == p.facts["pairs"]
    assert st["bgzf_blocks"] == _all_blocks(on_disk("bgzf")) and st["host_inflated_runs"] == 0 and st["text_segments"] == 0, st
    assert st["text_in_bytes"] == _text_bytes(p) and st["gzip_steps"] == 0, st


def test_gz_members_with_seams_at_the_uploads_ends(tmp_path, on_disk, oracle):
    p, q = _run(tmp_path, "gz_members", on_disk, oracle)
    st, files = q.pipe_stats, on_disk("gz_members")
    written = sum(len(U.members(files[k][0])[0]) for k in G.STREAMS)
    assert written == 6 + 2 + 1 + 1
    assert q.use_pipe and st["gzip_members"] == written and st["gzip_fallbacks"] == 0 and st["text_segments"] == 0, st  # (the empty one counts)
    assert st["pairs"] == p.facts["pairs"] and st["text_in_bytes"] == _text_bytes(p), st


def test_bgzf_seams_stay_on_the_device(tmp_path, on_disk, oracle):
    """text_segments == 0: no buffer's end -- on a block boundary, inside the first 18 bytes of a header, inside a long extra field --
    makes the feeder hand the rest of the file to the host's text path"""
    p, q = _run(tmp_path, "bgzf_seams", on_disk, oracle)
    st = q.pipe_stats
    assert q.use_pipe and st["pairs"] == p.facts["pairs"]
    assert st["text_segments"] == 0, st
    assert st["bgzf_blocks"] == _all_blocks(on_disk("bgzf_seams")) and st["host_inflated_runs"] == 0, st
    assert st["text_in_bytes"] == _text_bytes(p) and st["gzip_steps"] == 0, st


def test_bgzf_then_gz_goes_on_as_text(tmp_path, on_disk, oracle):
    p, q = _run(tmp_path, "bgzf_then_gz", on_disk, oracle)
    st, files = q.pipe_stats, on_disk("bgzf_then_gz")
    blocks = len(U.bgzf_layout(files["seq_R1"][0])) + sum(len(G.bgzf_blocks(files[k][0])) for k in ("seq_R2", "index_R1", "index_R2"))
    assert q.use_pipe and st["pairs"] == p.facts["pairs"]
    assert st["bgzf_blocks"] == blocks and st["text_segments"] >= 1 and st["host_inflated_runs"] == 0, st
    assert st["text_in_bytes"] == _text_bytes(p), st


def test_gz_refused_late_falls_back_behind_delivered_text(tmp_path, on_disk, oracle, gz_run):
    """The device refuses a block of seq_R2's second upload: the host reads the member again from its start and drops the text that
    the first upload's steps delivered (host_skip).  The control, framing gz, never falls back."""
    assert gz_run["gzip_fallbacks"] == 0
    p, q = _run(tmp_path, "gz_refused_late", on_disk, oracle)
    st = q.pipe_stats
    assert q.use_pipe and st["pairs"] == p.facts["pairs"]
    assert st["gzip_fallbacks"] == 1 and st["text_segments"] >= 1 and st["gzip_members"] == 3, st
    assert st["text_in_bytes"] == _text_bytes(p), st  # no byte delivered twice or left out


@pytest.mark.parametrize("fmt", ["gz", "bgzf"])
def test_damage_behind_the_first_upload_fails_the_run_and_the_next_run_is_clean(tmp_path, fmt, on_disk, oracle, capfd):
    from quade_amd import hip_backend as hb
    from quade_amd.sample import Sample
    p, files = U.texts("long"), on_disk(fmt + "_damaged_late")
    oracle("long")
    said = ""
    try:
        q, rc, _ = _cli(tmp_path / "damaged", files, p)
        assert rc != 0
    except (IOError, hb.QuadeHipError) as e:
        said = str(e)
    finally:
        Sample.RESET()
    out = capfd.readouterr()
    print("\nupload seams %s_damaged_late: %s" % (fmt, said))
    assert os.path.basename(files["seq_R1"][0]) in said + out.out + out.err, said
    p, q = _run(tmp_path / "healthy", fmt, on_disk, oracle)
    assert q.use_pipe and q.pipe_stats["pairs"] == p.facts["pairs"] and q.pipe_stats["text_segments"] == 0


@pytest.mark.parametrize("fmt", ["gz", "bgzf"])
def test_chunk_ends_early_while_uploads_are_in_flight(tmp_path, fmt, on_disk, oracle):
    p, q = _run(tmp_path, "ends_early_" + fmt, on_disk, oracle)
    st = q.pipe_stats
    assert q.use_pipe and st["pairs"] == 150 + 300 == p.facts["pairs"], st
    assert st["batches"] == 2 + 4, st
    if fmt == "gz":
        assert st["gzip_fallbacks"] == 0, st
    else:
        assert st["host_inflated_runs"] == 0, st
    assert st["text_segments"] == 0, st


def test_dense_buffer_goes_out_in_several_segments(tmp_path, on_disk, oracle):
    p, q = _run(tmp_path, "dense", on_disk, oracle)
    st = q.pipe_stats
    assert q.use_pipe and st["pairs"] == p.facts["pairs"]
    assert st["bgzf_blocks"] == _all_blocks(on_disk("dense")) and st["host_inflated_runs"] == 0 and st["text_segments"] == 0, st
    assert st["text_in_bytes"] == _text_bytes(p), st


@pytest.mark.parametrize("framing", ["gz", "gz_members"])
def test_pinned_slots_path_reads_the_same_files(tmp_path, framing, on_disk, oracle):
    """the batch pipeline over pinned slots reads the same files with the host's readers: same outputs"""
    p, q = _run(tmp_path, framing, on_disk, oracle, "device_pipeline : False\n")
    assert not q.use_pipe


def test_gz_with_the_steps_on_the_compute_stream(tmp_path, on_disk, oracle, gz_run):
    """inflate_overlap 0 (QUADE_PIPE_INFLATE_OVERLAP=0) puts the gzip steps on the compute stream: the same outputs from the same steps"""
    from quade_amd import hip_backend as hb
    from quade_amd.conf import QuadeConf
    from quade_amd.sample import Sample, WriterSet
    p, files = U.texts("long"), on_disk("gz")
    ref, counts = oracle("long")
    conf = str(tmp_path / "conf.txt")
    _conf(conf, files, True, G.POSITIONS, G.MIN_QUAL, p.samples)
    cf = QuadeConf(conf)
    Sample.RESET()
    Sample.CLASS_INIT(True, True, True, cf.minimal_qual, outdir=str(tmp_path), gzip_level=1)
    for name, index in cf.samples:
        Sample(name=name, index=index)
    out = tmp_path / "mine"
    out.mkdir()
    try:
        with hb.Engine(0) as eng:
            eng.set_plan(cf.plan())
            eng.set_barcodes(Sample.BARCODES())
            ws = WriterSet(str(out), 1, deflate_device=-1)
            with hb.Pipe(eng, p.batch_pairs) as pipe:
                pipe.set_option("inflate_overlap", 0)
                t0 = time.time()
                st = pipe.run([(cf.seq_R1[0], cf.seq_R2[0], cf.index_R1[0], cf.index_R2[0], ws.handle(), None, None)])
                seconds = time.time() - t0
            ws.close()
            assert [int(x) for x in eng.counts()] == counts
    finally:
        Sample.RESET()
    print("\nupload seams gz (inflate_overlap 0): %.1f s %s" % (seconds, " ".join("%s=%d" % (k, st[k]) for k in SHOWN)))
    names = sorted(f for f in os.listdir(ref) if f.endswith(".fastq.gz"))
    assert names == sorted(f for f in os.listdir(str(out)) if f.endswith(".fastq.gz"))
    for f in names:
        assert gzip.open(str(out / f)).read() == gzip.open(os.path.join(ref, f)).read(), f
    for k in ("pairs", "batches", "gzip_steps", "gzip_members", "gzip_fallbacks", "text_segments", "text_in_bytes"):
        assert st[k] == gz_run[k], (k, st[k], gz_run[k])
