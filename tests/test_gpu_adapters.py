"""The adapter content on the MI355X (qd_adapters_*, quade_amd/csrc/quade_adapters.hip): the table read back from the device equals
tests/adapter_model.py's plain Python search, exactly -- for the stage on its own (qd_dev_adapters: lengths, every start of a read,
the seams of the packed words and of the lanes' shares, case, N, several probes, both sides of the staged-line limit and of the
last bin, routing, more than one workgroup, accumulation, state and errors) and through the command line (the report against the
writer fed with the model over the oracle's per-destination output files, which hold the raw reads by the routing)."""
import os

import numpy as np
import pytest

from quade_amd import adapter_report as ar
from quade_amd import hip_backend as hb
from tests import adapter_model as AM
from tests import stage_support as SS
from tests.stage_support import _barcodes, _cli, _engine, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
UND = AM.UNDETERMINED
BUILTIN = [p for _, p in AM.BUILTIN]
UNI, NEXTERA, POLY_A, POLY_G = BUILTIN[0], BUILTIN[3], BUILTIN[4], BUILTIN[5]
WG_READS = 2048  # reads per workgroup of the kernel (quade_adapters.hip)


def _bg(rng, L, alphabet=b"CCT"):
    """L random bases without A and G, never 12 equal ones in a row"""
    s = bytearray(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))
    for i in range(5, L, 6):
        s[i] = ord("T") if s[i - 1] == ord("C") else ord("C")
    return bytes(s)


def _plant(s, at, probe):
    """probe over s from `at` on, cut at the end of s"""
    out = bytearray(s)
    out[at:at + len(probe)] = probe[:max(0, len(s) - at)]
    return bytes(out[:len(s)])


class AStage(object):
    """pairs of reads (bytes) as two fastq texts with their record tables; R1 and R2 of a pair need not be alike"""

    def __init__(self, seed, reads1, reads2):
        rng = np.random.default_rng(seed)
        assert len(reads1) == len(reads2)
        self.n, self.p1, self.p2 = len(reads1), list(reads1), list(reads2)
        self.t1, self.r1 = SS._text_from(rng, [("", s, b"I" * len(s)) for s in reads1])
        self.t2, self.r2 = SS._text_from(rng, [("", s, b"5" * len(s)) for s in reads2])

    def model(self, S, probes, codes):
        return AM.table(S, probes, [(int(c), a, b) for c, a, b in zip(codes, self.p1, self.p2)])

    def run(self, eng, codes):
        eng.dev_adapters(self.t1, self.r1, self.t2, self.r2, np.asarray(codes, dtype=np.uint16))


def _aengine(S=1, probes=BUILTIN):
    eng = _engine(S, enable=False)
    eng.adapters_set(probes)
    return eng


def _check(eng, want):
    got = eng.adapters_read()
    assert set(got) == set(want) == {"hist", "dest"}
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == np.uint64
        assert (got[k] == want[k]).all(), (k, np.argwhere(got[k] != want[k])[:8], got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])
    assert (got["hist"].sum(axis=2) == got["dest"].sum(axis=0)[:, 1:]).all()  # a read with first(a) has one bin
    assert (got["dest"][:, 0, 0] == got["dest"][:, 1, 0]).all()  # a pair adds one read to R1 and to R2 of its destination
    return got


def _run(st, S=1, probes=BUILTIN, codes=None):
    """-> the table, which equals the model's"""
    codes = np.zeros(st.n, dtype=np.uint16) if codes is None else codes
    with _aengine(S, probes) as eng:
        st.run(eng, codes)
        got = _check(eng, st.model(S, probes, codes))
        assert int(got["dest"][:, 0, 0].sum()) == st.n
        return {k: v.copy() for k, v in got.items()}


# ---- the stage ---------------------------------------------------------------------------------------------------------------------
def test_stage_read_lengths(torch_cuda):
    """0, 11, 12, 13 and 16 k - 1, 16 k + 1 up to the staged-line limit: the probe at the last start, at a random one, and none"""
    rng = np.random.default_rng(1)
    lens = [0, 11, 12, 13] + [16 * k + d for k in range(1, 22) for d in (-1, 0, 1)]
    r1, r2 = [], []
    for L in lens:
        for where in ("last", "random", "none"):
            s = _bg(rng, L)
            if L >= 12 and where != "none":
                s = _plant(s, L - 12 if where == "last" else int(rng.integers(0, L - 11)), UNI)
            r1.append(s)
            r2.append(_plant(_bg(rng, lens[int(rng.integers(0, len(lens)))]), 0, NEXTERA))
    got = _run(AStage(1, r1, r2))
    assert got["hist"][0, 0].sum() == 2 * sum(L >= 12 for L in lens) and got["hist"][0, 0, 337 - 12] >= 1 and got["hist"][0, 0, 0] >= 1
    assert got["hist"][1, 3, 0] > 40 and not got["hist"][1, 3, 1:].any()


def test_stage_every_start_of_a_100_base_read(torch_cuda):
    """one probe at every p from 0 to 88: every seam of the packed words and of the lanes' shares; at 89 it does not fit"""
    rng = np.random.default_rng(2)
    r1 = [_plant(_bg(rng, 100), p, UNI) for p in range(0, 90)]
    r2 = [_plant(_bg(rng, 100), p, POLY_G) for p in range(89, -1, -1)]
    got = _run(AStage(2, r1, r2))
    assert got["hist"][0, 0, :89].tolist() == [1] * 89 and got["hist"][0, 0].sum() == 89 and got["hist"][0, 16, :89].tolist() == [1] * 89
    assert got["hist"][1, 5, :89].tolist() == [1] * 89 and got["hist"][1, 5].sum() == 89
    assert got["dest"][0].tolist() == [[90, 89] + [0] * 15 + [89], [90] + [0] * 5 + [89] + [0] * 10 + [89]]


def test_stage_case_and_n(torch_cuda):
    """lower and mixed case match; an N (or n, or any other byte) at each of the 12 positions of a planted probe does not"""
    rng = np.random.default_rng(3)
    r1 = [_plant(_bg(rng, 60), 20, UNI.lower()), _plant(_bg(rng, 60), 21, b"AgAtCgGaAgAg"), _plant(_bg(rng, 60).lower(), 22, UNI)]
    for i in range(12):
        for other in b"Nn.R":
            r1.append(_plant(_bg(rng, 60), 20, UNI[:i] + bytes([other]) + UNI[i + 1:]))
    r2 = [_bg(rng, 30) for _ in r1]
    got = _run(AStage(3, r1, r2))
    assert got["hist"][0, 0, 20:23].tolist() == [1, 1, 1] and got["hist"][0].sum() == 6 and not got["hist"][1].any()


def test_stage_several_occurrences_and_several_probes(torch_cuda):
    rng = np.random.default_rng(4)
    twice = _plant(_plant(_bg(rng, 120), 70, UNI), 31, UNI)             # the first occurrence counts
    both = _plant(_plant(_bg(rng, 120), 17, NEXTERA), 64, UNI)          # both are counted, any is the lower
    both2 = _plant(_plant(_bg(rng, 120), 90, NEXTERA), 5, UNI)
    run = _plant(_bg(rng, 100), 33, b"A" * 40)                          # poly_a inside a run of 40 A: its first start only
    overlap = _plant(_bg(rng, 50), 10, UNI[:6] + UNI)                   # AGATCGAGATCGGAAGAG: the probe starts at 16
    r1 = [twice, both, both2, run, overlap]
    got = _run(AStage(4, r1, [_bg(rng, 20)] * len(r1)))
    assert sorted(np.flatnonzero(got["hist"][0, 0]).tolist()) == [5, 16, 31, 64] and got["hist"][0, 3, 17] == 1 and got["hist"][0, 3, 90] == 1
    assert got["hist"][0, 4].sum() == 1 and got["hist"][0, 4, 33] == 1
    assert sorted(np.flatnonzero(got["hist"][0, 16]).tolist()) == [5, 16, 17, 31, 33] and got["hist"][0, 16].sum() == 5


def test_stage_all_sixteen_slots_and_one_slot(torch_cuda):
    rng = np.random.default_rng(5)
    probes = BUILTIN + [bytes(b"ACGT"[(i >> (2 * k)) & 3] for k in range(12)) for i in range(1000, 1010)]
    assert len(probes) == 16 == len(set(probes))
    r1 = [_plant(_bg(rng, 80), int(rng.integers(0, 69)), probes[i % 16]) for i in range(64)]
    r2 = [_plant(_plant(_bg(rng, 150), 100, probes[(i + 1) % 16]), 3 * (i % 16), probes[15 - i % 16]) for i in range(64)]
    st = AStage(5, r1, r2)
    got = _run(st, probes=probes)
    assert (got["hist"][0, :16].sum(axis=1) >= 4).all() and (got["hist"][1, :16].sum(axis=1) >= 4).all()
    one = _run(st, probes=[probes[9]])
    assert one["hist"][0, 0].sum() == 4 and not one["hist"][:, 1:16].any() and (one["hist"][:, 16] == one["hist"][:, 0]).all()
    assert (one["hist"][:, 0] == got["hist"][:, 9]).all()


def test_stage_both_sides_of_the_staged_line_and_of_the_last_bin(torch_cuda):
    """reads of 330 bases fit the slab at some alignments only, reads of 340 never; a read of 1 100 bases has starts on both sides
    of bin 1024"""
    rng = np.random.default_rng(6)
    r1, r2 = [], []
    for L in (330, 340, 321, 322, 336, 337):
        for _ in range(12):  # (names of 1 .. 24 bytes move the line over the alignments)
            r1.append(_plant(_bg(rng, L), int(rng.integers(0, L - 11)), UNI))
            r2.append(_plant(_bg(rng, L), L - 12, POLY_G.lower()))
    for p in (1011, 1012, 1023, 1024, 1080):
        r1.append(_plant(_bg(rng, 1100), p, UNI))
        r2.append(_plant(_plant(_bg(rng, 1100), p, NEXTERA), 1040, UNI))
    got = _run(AStage(6, r1, r2))
    assert got["hist"][0, 0, [1011, 1012, 1023]].tolist() == [1, 1, 1] and got["hist"][0, 0, 1024] == 2  # 1024 and 1080 share the last bin
    assert got["hist"][1, 3, [1011, 1012, 1023, 1024]].tolist() == [1, 1, 1, 2] and got["hist"][1, 0, 1024] == 5
    assert got["hist"][1, 5, [318, 328, 309, 310, 324, 325]].tolist() == [12] * 6


def test_stage_r1_and_r2_of_different_lengths(torch_cuda):
    rng = np.random.default_rng(7)
    r1 = [_plant(_bg(rng, L), 0, UNI) for L in (12, 400, 0, 151, 20)]
    r2 = [_plant(_bg(rng, L), L - 12, UNI) for L in (400, 12, 151, 12, 337)]
    got = _run(AStage(7, r1, r2))
    assert got["hist"][0, 0, 0] == 4 and sorted(np.flatnonzero(got["hist"][1, 0]).tolist()) == [0, 139, 325, 388]


@pytest.mark.parametrize("S", [2, 120])
def test_stage_routing(torch_cuda, S):
    """pass, fail and 0xFFFF over a sheet of 2; a sheet of 120 has more destinations than the workgroup keeps partials for"""
    n = 300
    rng = np.random.default_rng(8)
    codes = rng.integers(0, 2 * S + 1, n)
    codes[:5] = (2 * S - 1, 2 * S - 2, 0, 1, 2 * S)
    codes[codes == 2 * S] = UND
    r1 = [_plant(_bg(rng, 70), int(rng.integers(0, 59)), BUILTIN[i % 6]) if i % 3 else _bg(rng, 70) for i in range(n)]
    r2 = [_plant(_bg(rng, 40), int(rng.integers(0, 29)), BUILTIN[i % 5]) if i % 2 else _bg(rng, 40) for i in range(n)]
    got = _run(AStage(8, r1, r2), S=S, codes=codes.astype(np.uint16))
    assert got["dest"].shape == (2 * S + 1, 2, 18) and got["dest"][2 * S, 0, 0] == int((codes == UND).sum()) > 0
    assert (got["dest"][:, 0, 0] > 0).sum() > min(2 * S, 100) and got["dest"][:, :, 17].sum() == 200 + 150


@pytest.mark.parametrize("n", [1, 1024, 1025, WG_READS + 1])
def test_stage_pair_counts(torch_cuda, n):
    """one pair; 1 024 and 1 025; one more than a workgroup takes"""
    rng = np.random.default_rng(n)
    r1 = [_plant(_bg(rng, 40), int(rng.integers(0, 29)), UNI) if i % 4 == 0 else _bg(rng, 40) for i in range(n)]
    r2 = [_plant(_bg(rng, 30), 7, POLY_A) if i % 7 == 0 else _bg(rng, 30) for i in range(n)]
    codes = np.array([0, 1, UND], dtype=np.uint16)[rng.integers(0, 3, n)]
    got = _run(AStage(n, r1, r2), codes=codes)
    assert got["hist"][0, 0].sum() == (n + 3) // 4 and got["hist"][1, 4, 7] == (n + 6) // 7


def test_accumulation_reset_add_and_state(torch_cuda):
    S = 3
    rng = np.random.default_rng(9)
    a = AStage(20, [_plant(_bg(rng, 80), i % 60, UNI) for i in range(200)], [_bg(rng, 50) for _ in range(200)])
    b = AStage(21, [_bg(rng, 30) for _ in range(65)], [_plant(_bg(rng, 90), i, NEXTERA) for i in range(65)])
    ca = rng.integers(0, 2 * S, 200).astype(np.uint16)
    cb = rng.integers(0, 2 * S, 65).astype(np.uint16)
    cb[::7] = UND
    n_values = hb.adapters_values(S)
    with _aengine(S) as eng, _aengine(S) as other:
        assert eng.adapters_active() and eng.adapters_get() == [p.decode() for p in BUILTIN]
        a.run(eng, ca)
        b.run(eng, cb)
        both = AM.add(a.model(S, BUILTIN, ca), b.model(S, BUILTIN, cb))
        _check(eng, both)
        eng.reset_counts()
        assert not any(v.any() for v in eng.adapters_read().values())
        b.run(eng, cb)
        _check(eng, b.model(S, BUILTIN, cb))
        a.run(other, ca)
        eng.adapters_add(other.adapters_read())  # a second context's table folds in
        _check(eng, both)
        _check(other, a.model(S, BUILTIN, ca))
        # a table of another size, bad probes: refused, and nothing changes
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.adapters_add(np.zeros(n_values - 36, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        out = np.zeros(n_values + 36, dtype=np.uint64)
        assert eng.lib.qd_adapters_read(eng._h, hb._ptr(out), out.size) == hb.QD_ERR_INVALID
        seventeen = BUILTIN + [bytes(b"ACGT"[(i >> (2 * k)) & 3] for k in range(12)) for i in range(2000, 2011)]
        assert len(set(seventeen)) == 17
        for bad in ([UNI, b"AGATCGGAAGAN"], [UNI, UNI.lower()], [UNI, NEXTERA, UNI], seventeen):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.adapters_set(bad)
            assert ei.value.code == hb.QD_ERR_INVALID
        assert eng.adapters_get() == [p.decode() for p in BUILTIN]
        _check(eng, both)
        # set while on: a new table for the new probes
        eng.adapters_set([NEXTERA, UNI])
        assert eng.adapters_get() == [NEXTERA.decode(), UNI.decode()] and not any(v.any() for v in eng.adapters_read().values())
        a.run(eng, ca)
        _check(eng, a.model(S, [NEXTERA, UNI], ca))
        # off: by no probes; every entry then says so
        eng.adapters_set([])
        assert not eng.adapters_active() and eng.adapters_get() == []
        for call in (eng.adapters_read, lambda: eng.adapters_add(np.zeros(n_values, np.uint64)), lambda: b.run(eng, cb)):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        eng.adapters_set(BUILTIN, on=False)  # off while off
        assert not eng.adapters_active()
        eng.adapters_set(BUILTIN)  # set while off
        assert eng.adapters_active() and not any(v.any() for v in eng.adapters_read().values())
        eng.set_barcodes(_barcodes(S + 1))  # the table has a row per destination: new barcodes turn the stage off
        assert not eng.adapters_active() and eng.adapters_get() == []
        eng.adapters_set(BUILTIN)
        assert eng.adapters_read()["dest"].shape == (2 * (S + 1) + 1, 2, 18)
    with hb.Engine(0) as bare:  # no plan, no barcodes
        with pytest.raises(hb.QuadeHipError) as ei:
            bare.adapters_set(BUILTIN)
        assert ei.value.code == hb.QD_ERR_STATE


def test_bad_tables_and_codes_are_refused_before_the_launch(torch_cuda):
    S = 2
    rng = np.random.default_rng(10)
    st = AStage(30, [_plant(_bg(rng, 50), 5, UNI) for _ in range(64)], [_bg(rng, 50) for _ in range(64)])
    codes = rng.integers(0, 2 * S, 64).astype(np.uint16)
    with _aengine(S) as eng:
        st.run(eng, codes)
        want = st.model(S, BUILTIN, codes)
        _check(eng, want)
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_adapters(st.t1, bad, st.t2, st.r2, codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        for code in (2 * S, 0xFFFE):
            c2 = codes.copy()
            c2[9] = code
            with pytest.raises(hb.QuadeHipError) as ei:
                st.run(eng, c2)
            assert ei.value.code == hb.QD_ERR_INVALID
        _check(eng, want)


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
EXTRA = "adapter_report_extra : r2_tail=AGATCGGAAGAGCGTCGTGT;mine=ACGTACGTACGTAAA;short=ACGT\n"
PROBES = AM.BUILTIN + (("mine", b"ACGTACGTACGT"),)  # r2_tail is an alias of illumina_universal, short is left off
PARAMS = dict(probes=[(n, p.decode()) for n, p in PROBES], aliases=[("r2_tail", "illumina_universal")], left_off=[("short", "shorter than 12 bases")])


def _write_conf(path, files, samples, adapters=True, **kw):
    SS._write_conf(path, files, samples, **kw)
    if adapters:
        text = open(path).read().replace("[output]\n", "[output]\nadapter_report : True\n" + EXTRA, 1)
        open(path, "w").write(text)


def _names(samples):
    return [s[0] for s in samples]


def _model_report(conf, ref_dir, samples):
    """the oracle's run of the conf (it knows nothing of the option) -> (the report's text by the writer over the model's table of the
    reads in its output files, the table)"""
    SS._oracle_run(conf, ref_dir)
    table = AM.table_from_outputs(str(ref_dir), _names(samples), [p for _, p in PROBES])
    return "\n".join(ar.report_lines(table, _names(samples), PARAMS)) + "\n", table


def _report(work):
    return SS._read(os.path.join(str(work), ar.REPORT_NAME))


def _same_files(mine, other, but=(ar.REPORT_NAME,)):
    """every file of `mine` but the adapter report is in `other`, byte for byte (Quade_report.csv: behind its dated first line)"""
    a, b = (sorted(f for f in os.listdir(str(d)) if f not in but) for d in (mine, other))
    assert a == b and len(a) > 10
    for f in a:
        x, y = (open(os.path.join(str(d), f), "rb").read() for d in (mine, other))
        if f == "Quade_report.csv":
            x, y = x.split(b"\n", 1)[1], y.split(b"\n", 1)[1]
        assert x == y, f


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 1 500 pairs in BGZF whose fragments read through into the adapters (a sample of poly-G reads, lower case, N),
    batch_pairs 1000: run once with the option on and once with it off; the model's report from the oracle's outputs"""
    top = tmp_path_factory.mktemp("adapters_bgzf")
    files, samples = SS._filter_dataset(str(top / "data"), 51, 2, 1500, bgzf=True)
    conf, plain = top / "conf.txt", top / "plain.txt"
    _write_conf(conf, files, samples)
    _write_conf(plain, files, samples, adapters=False)
    want, table = _model_report(plain, top / "ref", samples)
    _cli(conf, top / "mine")
    _cli(plain, top / "off")
    return dict(top=top, files=files, samples=samples, want=want, table=table, mine=top / "mine", off=top / "off", ref=top / "ref")


def test_cli_report_equals_the_model_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    pairs = int(t["dest"][:, 0, 0].sum())
    assert 2900 < pairs <= 3000 and (t["dest"][:, 0, 0] > 0).all()
    assert t["dest"][:, 0, 1].sum() > 300 and t["dest"][:, 1, 1].sum() > 300 and t["dest"][:, :, 6].sum() > 100  # universal in both reads, poly_g
    assert len(np.flatnonzero(t["hist"][0, 0])) > 50  # the adapter starts where the fragment ends
    assert _report(run["mine"]) == run["want"]
    lines = run["want"].split("\n")
    assert "top_adapter_R1\tillumina_universal" in lines and "6\tmine\tACGTACGTACGT\t" in lines
    assert "0\tillumina_universal\tAGATCGGAAGAG\tr2_tail" in lines and "short\tshorter than 12 bases" in lines


def test_cli_every_other_file_is_as_with_the_option_off(bgzf_run):
    run = bgzf_run
    assert not os.path.exists(run["off"] / ar.REPORT_NAME) and os.path.exists(run["mine"] / ar.REPORT_NAME)
    _same_files(run["mine"], run["off"])
    from tests.run_support import _compare_dirs
    _compare_dirs(str(run["off"]), str(run["ref"]))  # ... which is the oracle's


def test_cli_report_equals_the_model_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = SS._filter_dataset(str(tmp_path / "data"), 52, 2, 1000, bgzf=False)
    conf = tmp_path / "conf.txt"
    _write_conf(conf, files, samples)
    want, table = _model_report(conf, tmp_path / "ref", samples)
    _cli(conf, tmp_path / "mine")
    assert _report(tmp_path / "mine") == want and table["dest"][:, :, 1].sum() > 400


def test_cli_the_stage_sees_raw_reads_whatever_runs_behind_it(bgzf_run, tmp_path):
    """[trim] with adapters, a cutoff and pair_overlap, [filter] and a screen that drops: the same counts as without them.  (The
    [trim] adapters join the probes as aliases of the universal one, so the table is the same and the report names them.)"""
    run = bgzf_run
    with open(tmp_path / "spike.fa", "wb") as fh:
        fh.write(b">spike\n" + _bg(np.random.default_rng(1), 300, b"ACGT") + b"\n>dark\n" + b"G" * 60 + b"\n")
    screen = "[screen]\nreference : %s\nkmer : 21\naction : drop\n" % (tmp_path / "spike.fa")
    conf = tmp_path / "all.txt"
    _write_conf(conf, run["files"], run["samples"], extra=SS.TRIMS + SS.FILTER + screen, quality=True)
    _cli(conf, tmp_path / "all")
    params = dict(PARAMS, aliases=[("adapter_R1", "illumina_universal"), ("adapter_R2", "illumina_universal")] + PARAMS["aliases"])
    assert _report(tmp_path / "all") == "\n".join(ar.report_lines(run["table"], _names(run["samples"]), params)) + "\n"
    # the stages behind it did run: the quality report counts fewer reads and bases than the adapter report's reads
    with open(tmp_path / "all" / "Quade_quality_report.csv") as fh:
        total = [ln.split("\t") for ln in fh.read().split("\n") if ln.startswith("Total\t")]
    assert 0 < int(total[0][2]) < int(run["table"]["dest"][:, 0, 0].sum())
    screened = SS._read(tmp_path / "all" / "Quade_screen_report.csv").split("\n")[-2].split("\t")
    assert screened[0] == "Total" and 0 < int(screened[1]) < int(run["table"]["dest"][:, 0, 0].sum())  # the pairs the filter kept
    assert os.path.exists(tmp_path / "all" / "Quade_trim_report.csv") and os.path.exists(tmp_path / "all" / "Quade_pair_trim_report.csv")


def test_cli_chunk_workers_and_a_chunk_cut_across_parts(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "workers.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="chunk_workers : 2\n")
    _cli(conf, tmp_path / "workers")
    assert _report(tmp_path / "workers") == run["want"]
    conf = tmp_path / "shared.txt"  # 2 ranks on GPU 0, each a pair range of every chunk; the tables meet through the rendezvous files
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : True\n")
    _cli(conf, tmp_path / "shared", ranks=2)
    assert _report(tmp_path / "shared") == run["want"]
    assert not [f for f in os.listdir(tmp_path / "shared") if f.startswith(".quade_rdv")]


def test_cli_write_flags_do_not_matter(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "flags.txt"
    _write_conf(conf, run["files"], run["samples"], flags=(True, False, False))
    _cli(conf, tmp_path / "flags")
    assert _report(tmp_path / "flags") == run["want"]
    assert not [f for f in os.listdir(tmp_path / "flags") if "_fail_" in f or f.startswith("Undetermined")]


def test_cli_option_rejected_without_the_device_pipeline(bgzf_run, tmp_path):
    import subprocess
    import sys
    run = bgzf_run
    conf = tmp_path / "slots.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="device_pipeline : False\n")
    r = subprocess.run([sys.executable, os.path.join(SS.ROOT, "bin", "Quade.py"), "-c", str(conf)], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, PYTHONPATH=SS.ROOT))
    assert r.returncode == 1 and "adapter_report needs the device pipeline" in r.stdout + r.stderr
    assert not os.path.exists(tmp_path / ar.REPORT_NAME) and not os.path.exists(tmp_path / "Quade_report.csv")
