"""The adapter content report off the GPU: the model against str.find, the conf options with the probe list they make and the
configurations they reject, the report writer against hand-written text, the exchange format of the ranks, the exported symbols,
and the three pinned stage tuples."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import adapter_report as ar
from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from tests import adapter_model as AM
from tests.stage_support import _one_sample_conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = "adapter_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
BUILTIN = [("illumina_universal", "AGATCGGAAGAG"), ("illumina_small_rna_3p", "TGGAATTCTCGG"), ("illumina_small_rna_5p", "GATCGTCGGACT"),
           ("nextera_transposase", "CTGTCTCTTATA"), ("poly_a", "AAAAAAAAAAAA"), ("poly_g", "GGGGGGGGGGGG")]


def _conf(tmp_path, output="", trim="", gpu=""):
    return _one_sample_conf(tmp_path, extra=output, gpu=("[trim]\n" + trim if trim else "") + gpu)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def test_model_against_str_find_on_random_reads_with_planted_probes():
    rng = np.random.default_rng(11)
    probes = [p for _, p in AM.BUILTIN] + [b"ACGTTGCAAGCT"]
    hits = 0
    for i in range(400):
        L = int(rng.integers(0, 90))
        s = bytearray(b"ACGTNacgtn"[int(v)] for v in rng.integers(0, 10 if i % 3 else 4, L))
        for _ in range(int(rng.integers(0, 3))):  # planted, sometimes in lower case, sometimes over the end
            p = probes[int(rng.integers(0, len(probes)))]
            at = int(rng.integers(0, L + 1))
            s[at:at + 12] = p.lower() if rng.integers(0, 2) else p
        s = bytes(s)
        f = AM.firsts(s, probes)
        want = [s.upper().find(p) for p in probes]
        assert f[:-1] == [None if w < 0 else w for w in want], (s, f)
        assert f[-1] == (min(w for w in want if w >= 0) if max(want) >= 0 else None)
        hits += sum(w >= 0 for w in want)
    assert hits > 200
    # a byte that folds to a letter of ACGT without being one matches as that letter; one that does not never matches
    assert AM.first(b"agatcggaagag", b"AGATCGGAAGAG") == 0 and AM.first(b"AGATCGGAAGAN", b"AGATCGGAAGAG") is None
    assert AM.first(b"AGATCGGAAGA", b"AGATCGGAAGAG") is None and AM.first(b"", b"AGATCGGAAGAG") is None
    assert AM.first(b"A" * 40, b"A" * 12) == 0 and AM.first(b"CAGATCGGAAGAGAGATCGGAAGAG", b"AGATCGGAAGAG") == 1


def test_model_table_and_its_cross_checks():
    probes = [p for _, p in AM.BUILTIN]
    pairs = [(0, b"TTAGATCGGAAGAGCC", b"G" * 30), (3, b"ACGT" * 5, b"ctgtctcttatacacatct"), (AM.UNDETERMINED, b"", b"AAAAAAAAAAAN"),
             (0, b"C" * 1040 + b"AGATCGGAAGAG", b"C" * 1023 + b"AGATCGGAAGAG")]
    t = AM.table(2, probes, pairs)
    assert t["hist"].shape == (2, 17, 1025) and t["dest"].shape == (5, 2, 18) and t["hist"].size + t["dest"].size == AM.values(2) == 35030
    assert t["hist"][0, 0, 2] == 1 and t["hist"][0, 16, 2] == 1 and t["hist"][1, 5, 0] == 1 and t["hist"][1, 3, 0] == 1
    assert t["hist"][0, 0, 1024] == 1 and t["hist"][1, 0, 1023] == 1 and t["hist"][1, 0, 1024] == 0 and not t["hist"][:, 6:16].any()
    assert t["dest"][:, :, 0].tolist() == [[2, 2], [0, 0], [0, 0], [1, 1], [1, 1]] and not t["dest"][4, :, 1:].any()
    assert (t["hist"].sum(axis=2) == t["dest"].sum(axis=0)[:, 1:]).all()
    assert AM.add(t, t)["dest"][0, 0, 0] == 4


# ---- the conf --------------------------------------------------------------------------------------------------------------------
def test_conf_defaults_aliases_and_sequences_left_off(tmp_path):
    cf = qconf.QuadeConf(_conf(tmp_path))
    assert cf.adapter_report is False and cf.adapter_report_extra == "" and cf.adapter_params() is None and not hb.ADAPTERS.on(cf)
    for off in ("adapter_report :\n", "adapter_report : False\n"):
        assert qconf.QuadeConf(_conf(tmp_path, off)).adapter_report is False
    cf = qconf.QuadeConf(_conf(tmp_path, "adapter_report : True\n"))
    assert cf.adapter_report is True and hb.ADAPTERS.on(cf)
    assert cf.adapter_params() == dict(probes=BUILTIN, aliases=[], left_off=[]) and list(hb.ADAPTER_BUILTIN) == BUILTIN
    assert [(n, p.decode()) for n, p in AM.BUILTIN] == BUILTIN
    # [trim] adapters under their names: R1 is an alias of the universal probe, R2 a probe of its own; then the extras
    extra = "mine=acgtacgtacgtAAAA;again=ACGTACGTACGTCC;short=ACGTACGTACG;iupac=ACGTACGTACGNACGT;late_n=GGGGAAAACCCCN;g=GGGGGGGGGGGGGG"
    cf = qconf.QuadeConf(_conf(tmp_path, "adapter_report : True\nadapter_report_extra : %s\n" % extra,
                               trim="adapter_R1 : AGATCGGAAGAGCACACGTC\nadapter_R2 : CTGTCTCTTATC\n"))
    P = cf.adapter_params()
    assert P["probes"] == BUILTIN + [("adapter_R2", "CTGTCTCTTATC"), ("mine", "ACGTACGTACGT"), ("late_n", "GGGGAAAACCCC")]
    assert P["aliases"] == [("adapter_R1", "illumina_universal"), ("again", "mine"), ("g", "poly_g")]
    assert P["left_off"] == [("short", "shorter than 12 bases"), ("iupac", "the first 12 bases are not all A, C, G or T")]
    assert cf.trim  # the report's probes leave the trimming stage as configured


def test_conf_rejects_the_17th_probe_and_malformed_extras(tmp_path):
    def seq(i):
        return "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(6)) + "ACCATG"
    ten = ";".join("u%d=%s" % (i, seq(i)) for i in range(10))
    cf = qconf.QuadeConf(_conf(tmp_path, "adapter_report : True\nadapter_report_extra : %s\n" % ten))
    assert len(cf.adapter_params()["probes"]) == 16
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "adapter_report : True\nadapter_report_extra : %s;u10=%s\n" % (ten, seq(10))))
    assert str(ei.value) == qconf.ADAPTER_TOO_MANY and "16" in qconf.ADAPTER_TOO_MANY
    # an alias and a sequence left off take no slot
    cf = qconf.QuadeConf(_conf(tmp_path, "adapter_report : True\nadapter_report_extra : %s;again=%s;n=NNNNNNNNNNNNN\n" % (ten, seq(3))))
    assert len(cf.adapter_params()["probes"]) == 16 and cf.adapter_params()["aliases"] == [("again", "u3")]
    for bad in ("noequals", "a=ACGTACGTACGT;", "a=ACGTACGTACGT;;b=CCCCAAAATTTT", "a b=ACGTACGTACGT", "a-b=ACGTACGTACGT", "=ACGTACGTACGT",
                "a=", "a=ACGT ACGTACGT", "a=ACGTACGTACG7", "a=ACGTACGTACGT;a=CCCCAAAATTTT", "poly_a=ACGTACGTACGT", "adapter_R1=ACGTACGTACGT"):
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, "adapter_report : True\nadapter_report_extra : %s\n" % bad,
                                  trim="adapter_R1 : AGATCGGAAGAGC\n"))
        assert str(ei.value) == qconf.ADAPTER_EXTRA, bad


def test_conf_extra_alone_switches_nothing_on(tmp_path):
    cf = qconf.QuadeConf(_conf(tmp_path, "adapter_report_extra : a=ACGTACGTACGT\n"))
    assert cf.adapter_report is False and cf.adapter_params() is None and not [s.name for s in hb.READ_STAGES if s.on(cf)]
    cf = qconf.QuadeConf(_conf(tmp_path, "adapter_report_extra : not even well formed\n"))  # ... and is not looked at
    assert cf.adapter_report is False
    cf = qconf.QuadeConf(_conf(tmp_path, "adapter_report_extra : a=ACGTACGTACGT\n", gpu="[gpu]\ndevice_pipeline : False\n"))
    assert cf.adapter_report is False and not cf.can_pipe


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n", "gzip_level : 6\n"])
def test_conf_needs_the_device_pipeline(tmp_path, gpu):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "adapter_report : True\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == NEEDS == qconf.ADAPTER_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "adapter_report : False\n", gpu="[gpu]\n" + gpu)).adapter_report is False


def test_rejected_configurations_end_the_command_line_with_status_1(tmp_path):
    for k, (output, gpu, text) in enumerate((("adapter_report : True\n", "[gpu]\ndevice_pipeline : False\n", NEEDS),
                                             ("adapter_report : True\nadapter_report_extra : a:b\n", "", qconf.ADAPTER_EXTRA))):
        work = tmp_path / str(k)
        work.mkdir()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", _conf(work, output, gpu=gpu)], cwd=str(work),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1, (r.stdout, r.stderr)
        assert text in r.stdout + r.stderr
        assert not (work / ar.REPORT_NAME).exists() and not (work / "Quade_report.csv").exists()


def test_help_text_says_what_the_stage_counts():
    text = " ".join(qconf.ADAPTER_HELP.split())
    for words in ("adapter_report", "adapter_report_extra", "only stage that counts the RAW insert reads", "device_pipeline", "AGATCGGAAGAG",
                  "At most 16 distinct probes"):
        assert words in text, words


# ---- the report ------------------------------------------------------------------------------------------------------------------
def test_report_lines_against_hand_written_text():
    S = 1
    t = AM._arrays(AM._lists(S))
    params = dict(probes=[("uni", "AGATCGGAAGAG"), ("nx", "CTGTCTCTTATA"), ("mine", "ACGTACGTACGT")], aliases=[("adapter_R1", "uni"), ("x", "uni")],
                  left_off=[("short", "shorter than 12 bases")])
    # R1: 10 reads in S_pass, 4 in S_fail, 6 Undetermined; uni in 5 (positions 3, 3, 40, 40, >=1024), nx in 5 (0, 3, 7, 7, 7), one read has both (nx at 0, uni at 3): any in 9
    t["dest"][:, 0, 0] = (10, 4, 6)
    t["hist"][0, 0, 3], t["hist"][0, 0, 40], t["hist"][0, 0, 1024] = 2, 2, 1
    t["hist"][0, 1, 0], t["hist"][0, 1, 3], t["hist"][0, 1, 7] = 1, 1, 3
    t["hist"][0, 16, 0], t["hist"][0, 16, 3], t["hist"][0, 16, 7], t["hist"][0, 16, 40], t["hist"][0, 16, 1024] = 1, 2, 3, 2, 1
    t["dest"][0, 0, 1], t["dest"][2, 0, 1] = 3, 2
    t["dest"][0, 0, 2], t["dest"][1, 0, 2] = 1, 4
    t["dest"][0, 0, 17], t["dest"][1, 0, 17], t["dest"][2, 0, 17] = 3, 4, 2
    # R2: 20 reads, nothing found
    t["dest"][:, 1, 0] = (10, 4, 6)
    lines = ar.report_lines(t, ["S"], params)
    assert lines == [
        "Program Quade-adapters 0.3.2", "",
        "Probes", "slot\tname\tprobe\taliases", "0\tuni\tAGATCGGAAGAG\tadapter_R1,x", "1\tnx\tCTGTCTCTTATA\t", "2\tmine\tACGTACGTACGT\t", "",
        "Left off", "name\treason", "short\tshorter than 12 bases", "",
        "Reads with a probe", "read\tprobe\treads\treads_with_probe\tper_100000",
        "R1\tuni\t20\t5\t25000", "R1\tnx\t20\t5\t25000", "R1\tmine\t20\t0\t0", "R1\tany\t20\t9\t45000",
        "R2\tuni\t20\t0\t0", "R2\tnx\t20\t0\t0", "R2\tmine\t20\t0\t0", "R2\tany\t20\t0\t0", "",
        "top_adapter_R1\tuni", "top_adapter_R2\tnone", "",  # a tie goes to the lower slot
        "Content by position (cumulative)", "read\tposition\tuni\tnx\tmine\tany",
        "R1\t0\t0\t1\t0\t1", "R1\t3\t2\t2\t0\t3", "R1\t7\t2\t5\t0\t6", "R1\t40\t4\t5\t0\t8", "R1\t>=1024\t5\t5\t0\t9", "",
        "Per destination",
        "destination\tR1_reads\tR1_uni\tR1_nx\tR1_mine\tR1_any\tR1_any_pct\tR2_reads\tR2_uni\tR2_nx\tR2_mine\tR2_any\tR2_any_pct",
        "S_pass\t10\t3\t1\t0\t3\t30.00\t10\t0\t0\t0\t0\t0.00", "S_fail\t4\t0\t4\t0\t4\t100.00\t4\t0\t0\t0\t0\t0.00",
        "Undetermined\t6\t2\t0\t0\t2\t33.33\t6\t0\t0\t0\t0\t0.00", "Total\t20\t5\t5\t0\t9\t45.00\t20\t0\t0\t0\t0\t0.00"]
    t["hist"][0, 1, 9] += 1
    t["dest"][1, 0, 2] += 1
    assert "top_adapter_R1\tnx" in ar.report_lines(t, ["S"], params)
    with pytest.raises(AssertionError):
        ar.report_lines(t, ["S", "T"], params)


def test_write_report_writes_the_lines_without_a_date(tmp_path):
    t = AM.table(1, [p for _, p in AM.BUILTIN], [(0, b"TTAGATCGGAAGAGCC", b"G" * 30), (1, b"ACGT", b"ACGT")])
    params = dict(probes=[(n, p.decode()) for n, p in AM.BUILTIN], aliases=[], left_off=[])
    for name in ("a.csv", "b.csv"):
        ar.write_report(str(tmp_path / name), t, ["S1"], params)
    text = (tmp_path / "a.csv").read_text()
    assert text == (tmp_path / "b.csv").read_text() == "\n".join(ar.report_lines(t, ["S1"], params)) + "\n"
    assert "Date" not in text and ar.REPORT_NAME == "Quade_adapter_report.csv"
    assert "R1\t2\t1\t0\t0\t0\t0\t0\t1" in text and "R2\t0\t0\t0\t0\t0\t0\t1\t1" in text and "top_adapter_R2\tpoly_g" in text
    # through the stage table, as the run writes it
    path = hb.ADAPTERS.write_report(str(tmp_path), hb.adapters_views(hb.adapters_flat(t)), ["S1"], params)
    assert os.path.basename(path) == ar.REPORT_NAME and open(path).read() == text


# ---- the exchange of the ranks and the stage tuples ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1, 3])
def test_pack_unpack_round_trip(S):
    n = hb.adapters_values(S)
    assert n == 34850 + (2 * S + 1) * 36 == AM.values(S)
    a = np.random.default_rng(S).integers(0, 1 << 62, n, dtype=np.uint64)
    v = hb.adapters_views(a)
    assert v["hist"].shape == (2, 17, 1025) and v["dest"].shape == (2 * S + 1, 2, 18)
    assert v["hist"][1, 16, 1024] == a[34849] and v["dest"][0, 0, 0] == a[34850] and v["dest"][2 * S, 1, 17] == a[-1] and v["hist"][0, 1, 0] == a[1025]
    assert (hb.adapters_flat(v) == a).all() and (hb.adapters_flat(a) == a).all()
    blob = hb.pack_table("adapters", v)
    assert isinstance(blob, bytes) and len(blob) == 8 + 8 * n and blob == hb.pack_table(hb.ADAPTERS, a)
    assert int(np.frombuffer(blob, dtype=np.uint64, count=1)[0]) == n and blob[8:] == a.tobytes()
    back = hb.unpack_table("adapters", blob)
    assert set(back) == {"hist", "dest"} and all(back[k].dtype == np.uint64 and (back[k] == v[k]).all() for k in v)
    back["hist"][0, 0, 0] += 1  # a writable copy
    for bad in (blob[:-8], blob + bytes(8), blob[:8] + blob[16:], np.array([n - 36], dtype=np.uint64).tobytes() + blob[8:],
                np.array([n + 36], dtype=np.uint64).tobytes() + blob[8:] + bytes(36 * 8), blob[:8]):
        with pytest.raises(AssertionError):
            hb.unpack_table("adapters", bad)
    with pytest.raises(AssertionError):
        hb.adapters_views(a[:-1])
    m = AM.table(S, [b"ACGTACGTACGT"], [(AM.UNDETERMINED, b"ACGTACGTACGTA", b"")])
    assert all((hb.adapters_views(hb.adapters_flat(m))[k] == m[k]).all() for k in m)


def test_the_pinned_stage_tuples_are_unchanged_and_the_run_walks_a_further_one():
    assert [s.name for s in hb.STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "filter"]
    assert [s.name for s in hb.RUN_STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter"]
    assert [s.name for s in hb.PIPE_STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter", "screen"]
    assert hb.READ_STAGES[0] is hb.ADAPTERS and hb.READ_STAGES[1:] == hb.PIPE_STAGES and hb.ADAPTERS.name == "adapters"
    assert "adapters" not in hb.PIPE_STAGE and all(hb.READ_STAGE[s.name] is s for s in hb.READ_STAGES)
    # what the other stages pack is what it was: a count of rows, of values, or nothing in front
    q = np.arange(3 * 12, dtype=np.uint64)
    assert hb.pack_table("quality", q) == np.array([3], dtype=np.uint64).tobytes() + q.tobytes()
    assert (hb.unpack_table("quality", hb.pack_table("quality", q)) == q.reshape(3, 2, 6)).all()
    c = np.arange(24, dtype=np.uint64)
    assert hb.pack_table("clip", c) == c.tobytes() and (hb.unpack_table("clip", c.tobytes()) == c.reshape(2, 12)).all()
    with open(os.path.join(ROOT, "quade_amd", "quade.py")) as fh:
        assert fh.read().count("hb.READ_STAGES") == 2


def test_exported_symbols_and_layout_constants():
    new = {"qd_adapters_set", "qd_adapters_get", "qd_adapters_read", "qd_adapters_add", "qd_dev_adapters"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_adapters_device", "qd_adapters_active"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6
    rule = text.split("int qd_adapters_set")[0][-6000:]
    assert "no reference counterpart" in rule and "only stage that counts raw reads" in rule
    consts = {k: int(v) for k, v in re.findall(r"#define (QD_ADAPTERS_[A-Z_]+) (\d+)", header)}
    assert consts == dict(QD_ADAPTERS_K=hb.ADAPTER_K, QD_ADAPTERS_PROBES=hb.ADAPTER_PROBES, QD_ADAPTERS_BINS=hb.ADAPTER_BINS,
                          QD_ADAPTERS_HIST_VALUES=hb.ADAPTER_HIST_VALUES, QD_ADAPTERS_DEST_VALUES=hb.ADAPTER_DEST_VALUES)
    assert (AM.K, AM.PROBES, AM.BINS, AM.HIST_VALUES, AM.DEST_VALUES) == (12, 16, 1025, 34850, 36) == \
        (hb.ADAPTER_K, hb.ADAPTER_PROBES, hb.ADAPTER_BINS, hb.ADAPTER_HIST_VALUES, hb.ADAPTER_DEST_VALUES)
