"""The index-hopping report off the GPU: qd_hop_index against the model's part lists, the limit, the conf option and both
rejections, the ranks' exchange format, the writer on hand-made tables, and the exported symbols."""
import os
import subprocess

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import hopping_report as hr
from tests import hop_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _word(i, L):
    """the i-th word of length L over ACGT (distinct for distinct i < 4^L)"""
    return "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(L))


def combinatorial_sheet():
    """8 index-1 values x 12 index-2 values, row-major, six combinations left off"""
    off = {(0, 0), (1, 5), (3, 3), (4, 11), (7, 0), (7, 11)}
    return [_word(100 + a, 8) + _word(900 + b, 8) for a in range(8) for b in range(12) if (a, b) not in off]


SHEETS = {
    "unique_dual": ([_word(3 * i + 1, 8) + _word(5 * i + 2, 8) for i in range(96)], 16, 8),
    "combinatorial": (combinatorial_sheet(), 16, 8),
    "three_lengths": (["ACGTACGTTTTTAAAA", "ACGTACG", "ACGTACGTCCCCAAAA", "GGGGGGGGTTTTAAAACC", "GGGGGGGGTTTTAAAA", "TTTT",
                       "CCCCCCCCGGGGAAAA"], 16, 8),
    "lower_case": (["ACGTACGTTTTTAAAA", "acgtacgtTTTTAAAA", "ACGTACGTttttaaaa", "AcGTACGTCCCCAAAA"], 16, 8),
    "single_sample": (["ACGTACGTTTTTAAAA"], 16, 8),
    "w1_6_w2_8": ([_word(i % 5, 6) + _word(i, 8) for i in range(20)], 14, 6),
}


@pytest.mark.parametrize("name", sorted(SHEETS))
def test_hop_index_equals_the_model(name):
    bcs, K, w1 = SHEETS[name]
    P1, P2, part1, part2 = HM.part_lists(bcs, K, w1)
    g1, g2, n1, n2 = hb.hop_index(bcs, K, w1)
    assert (n1, n2) == (len(P1), len(P2))
    assert list(g1) == part1 and list(g2) == part2
    if name == "combinatorial":
        assert (n1, n2, len(bcs)) == (8, 12, 90)
    if name == "three_lengths":
        assert part1 == [0, -1, 0, -1, 1, -1, 2] and part2 == [0, -1, 1, -1, 0, -1, 2]
    if name == "lower_case":
        assert (n1, n2) == (3, 3)  # as registered: the spellings are different values


def test_hop_index_bad_arguments():
    for K, w1 in ((16, 0), (16, 16), (8, 9), (33, 8), (1, 1)):
        with pytest.raises(hb.QuadeHipError) as ei:
            hb.hop_index(["ACGTACGTACGTACGT"], K, w1)
        assert ei.value.code == hb.QD_ERR_INVALID
    assert hb.hop_index([], 16, 8)[2:] == (0, 0)


def test_limit():
    """(n1 + 1) * (n2 + 1) <= 2^24: 4 095 x 4 095 is accepted, 4 096 x 4 095 is rejected"""
    bcs = [_word(i, 8) + _word(i, 8) for i in range(4095)]
    assert hb.hop_index(bcs, 16, 8)[2:] == (4095, 4095)
    with pytest.raises(hb.QuadeHipError) as ei:
        hb.hop_index(bcs + [_word(4095, 8) + _word(0, 8)], 16, 8)
    assert ei.value.code == hb.QD_ERR_UNSUPPORTED and "4096 x 4095" in str(ei.value)


def _conf(tmp_path, output_extra="", dual=True, samples=(("S1", "ACAGACAG", "CTTGCTTG"),)):
    f = tmp_path / "reads.fastq"
    f.write_text("")
    txt = "[quality]\nminimal_qual : 25\n[fastq]\nseq_R1 : {0}\nseq_R2 : {0}\nindex_R1 : {0}\n".format(f)
    if dual:
        txt += "index_R2 : {0}\n".format(f)
    txt += "[index]\nindex2 : %s\nmolecular1 : False\nmolecular2 : False\nindex1_start : 1\nindex1_end : 8\n" % dual
    if dual:
        txt += "index2_start : 1\nindex2_end : 8\n"
    txt += "[output]\nwrite_pass : True\nwrite_fail : True\nwrite_undetermined : True\n" + output_extra
    for i, (name, b1, b2) in enumerate(samples):
        txt += "[sample%d]\nname : %s\nindex1_seq : %s\n" % (i + 1, name, b1) + ("index2_seq : %s\n" % b2 if dual else "")
    p = tmp_path / "conf.txt"
    p.write_text(txt)
    return str(p)


@pytest.mark.parametrize("extra,want", [("", False), ("index_hopping_report :\n", False), ("index_hopping_report : False\n", False),
                                        ("index_hopping_report : True\n", True), ("index_hopping_report : yes\n", True)])
def test_conf_option(tmp_path, extra, want):
    assert qconf.QuadeConf(_conf(tmp_path, extra)).index_hopping_report is want
    assert "index_hopping_report" in qconf.HOPPING_HELP and "share" in qconf.HOPPING_HELP and "lower bounds" in qconf.HOPPING_HELP


def _rejected(conf, capsys):
    from quade_amd.quade import Quade
    with pytest.raises(SystemExit) as ei:
        Quade(conf_file=conf)
    assert ei.value.code == 1
    return capsys.readouterr().out.rstrip("\n").split("\n")


def test_conf_without_index2_is_rejected(tmp_path, capsys):
    out = _rejected(_conf(tmp_path, "index_hopping_report : True\n", dual=False), capsys)
    assert out[-2:] == ["One of the value in the configuration file is not correct", qconf.HOPPING_NEEDS]
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "index_hopping_report : True\n", dual=False))
    assert str(ei.value) == "index_hopping_report needs a dual index (index2 : True)"
    assert not qconf.QuadeConf(_conf(tmp_path, "", dual=False)).index_hopping_report


def test_sheet_over_the_limit_is_rejected(tmp_path, capsys):
    samples = [("S%d" % i, _word(i, 8), _word(i, 8)) for i in range(4095)]
    from quade_amd.quade import Quade
    q = Quade(conf_file=_conf(tmp_path, "index_hopping_report : True\n", samples=samples))  # accepted: no GPU is touched yet
    assert q.hop_index[2:] == (4095, 4095)
    assert Quade(conf_file=_conf(tmp_path, "", samples=samples[:3])).hop_index is None
    capsys.readouterr()
    out = _rejected(_conf(tmp_path, "index_hopping_report : True\n", samples=samples + [("X", _word(4095, 8), _word(0, 8))]), capsys)
    assert out[-2:] == ["One of the value in the configuration file is not correct", qconf.HOPPING_TOO_MANY]
    assert "16777216" in qconf.HOPPING_TOO_MANY


def test_template_unchanged(bundled_dir):
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt"), "rb") as fh:
        assert qconf.template_bytes() == fh.read()
    assert b"index_hopping_report" not in qconf.template_bytes()


def test_pack_unpack():
    rng = np.random.default_rng(5)
    for n1, n2 in ((0, 0), (1, 1), (8, 12), (3, 200)):
        t = rng.integers(0, 1 << 62, hb.hop_values(n1, n2)).astype(np.uint64)
        blob = hb.pack_hop(n1, n2, t)
        assert len(blob) == 16 + 8 * t.size
        g1, g2, got = hb.unpack_hop(blob)
        assert (g1, g2) == (n1, n2) and got.dtype == np.uint64 and (got == t).all()
    blob = hb.pack_hop(8, 12, np.zeros(hb.hop_values(8, 12), np.uint64))
    for bad in (blob[:-8], blob + b"\0" * 8, blob[:8], hb.pack_hop(12, 8, np.zeros(hb.hop_values(8, 12), np.uint64))[:16] + blob[16:-8]):
        with pytest.raises(AssertionError):
            hb.unpack_hop(bad)
    with pytest.raises(AssertionError):
        hb.pack_hop(8, 12, np.zeros(5, np.uint64))


# ---- the writer --------------------------------------------------------------------------------------------------------------
def parse_report(lines):
    """-> (head lines, combination column names, combination rows, sample column names, sample rows)"""
    assert lines.count("") == 2
    i, j = lines.index(""), len(lines) - 1 - lines[::-1].index("")
    split = lambda ls: [ln.split("\t") for ln in ls]  # noqa: E731
    return lines[:i], lines[i + 1].split("\t"), split(lines[i + 2:j]), lines[j + 1].split("\t"), split(lines[j + 2:])


def _lines(table, bcs, K, w1, budgets=(0, 0), pairs=None, assigned=None):
    part1, part2, n1, n2 = hb.hop_index(bcs, K, w1)
    samples = [("S%d" % i, b) for i, b in enumerate(bcs)]
    assigned = [10 * (i + 1) for i in range(len(bcs))] if assigned is None else assigned
    pairs = sum(assigned) + int(np.asarray(table, dtype=np.uint64).sum()) if pairs is None else pairs
    return hr.report_lines(table, n1, n2, part1, part2, samples, w1, budgets, pairs, assigned), (part1, part2, n1, n2)


def test_writer_order_ties_and_head(tmp_path):
    bcs, K, w1 = SHEETS["three_lengths"]
    n1 = n2 = 3
    cells = np.zeros((n1 + 1, n2 + 1), dtype=np.uint64)
    cells[2, 0], cells[0, 2], cells[1, 1], cells[1, 2], cells[2, 1] = 7, 7, 9, 7, 1  # three ties at 7: (0, 2), (1, 2), (2, 0)
    cells[0, n2], cells[2, n2], cells[n1, 1], cells[n1, n2] = 4, 6, 5, 100
    table = np.concatenate([cells.reshape(-1), np.array([3], np.uint64)])
    lines, _ = _lines(table, bcs, K, w1)
    head, ccols, crows, scols, srows = parse_report(lines)
    assigned = sum(10 * (i + 1) for i in range(7))
    both, U = 31, 31 + 10 + 5 + 100 + 3
    assert head == ["index1 width\t8", "index2 width\t8", "distinct index1\t3", "distinct index2\t3", "samples off the matrix\t3",
                    "mismatch budgets\t0,0", "pairs\t%d" % (assigned + U), "assigned\t%d" % assigned, "undetermined\t%d" % U,
                    "short index slice\t3", "both indexes known\t31", "index1 known only\t10", "index2 known only\t5",
                    "neither known\t100", "unexpected_per_100000\t%d" % (both * 100000 // (assigned + both))]
    assert tuple(ccols) == hr.COMBINATION_COLUMNS == ("index1_seq", "index2_seq", "count", "per_100000_of_undetermined",
                                                      "index1_samples", "index2_samples")
    P1, P2, part1, part2 = HM.part_lists(bcs, K, w1)
    seq1 = {v: k for k, v in P1.items()}
    seq2 = {v: k for k, v in P2.items()}
    names1 = {a: ",".join("S%d" % s for s in range(7) if part1[s] == a) for a in range(3)}
    names2 = {b: ",".join("S%d" % s for s in range(7) if part2[s] == b) for b in range(3)}
    want = [(1, 1, 9), (0, 2, 7), (1, 2, 7), (2, 0, 7), (2, 1, 1)]  # count descending, then a, then b
    assert crows == [[seq1[a], seq2[b], str(c), str(c * 100000 // U), names1[a], names2[b]] for a, b, c in want]
    assert names1[0] == "S0,S2" and names2[0] == "S0,S4"
    assert tuple(scols) == hr.SAMPLE_COLUMNS
    assert [r[0] for r in srows] == ["S0", "S2", "S4", "S6"]  # the on-matrix samples in sheet order
    row, col = cells[:3, :3].sum(1), cells[:3, :3].sum(0)
    for r in srows:
        s = int(r[0][1:])
        a, b = part1[s], part2[s]
        assert r == [r[0], bcs[s][:8], bcs[s][8:], str(10 * (s + 1)), str(int(row[a])), str(int(col[b])), str(int(cells[a, 3])),
                     str(int(cells[3, b]))]
    path = tmp_path / hr.REPORT_NAME
    hr.write_report(str(path), table, 3, 3, part1, part2, [("S%d" % i, b) for i, b in enumerate(bcs)], w1, (0, 0), assigned + U,
                    [10 * (i + 1) for i in range(7)])
    text = path.read_text()
    assert text == "\n".join(lines) + "\n" and "Date" not in text and hr.REPORT_NAME == "Quade_index_hopping_report.csv"


def test_writer_cut_at_10000_rows():
    """a synthetic 128 x 128 sheet with every cell off the diagonal taken: 16 256 unexpected cells, 10 000 listed"""
    bcs = [_word(i, 8) + _word(i, 8) for i in range(128)]
    rng = np.random.default_rng(8)
    cells = np.zeros((129, 129), dtype=np.uint64)
    cells[:128, :128] = rng.integers(1, 40, (128, 128))  # many ties
    cells[np.arange(128), np.arange(128)] = 0
    table = np.concatenate([cells.reshape(-1), np.zeros(1, np.uint64)])
    lines, _ = _lines(table, bcs, 16, 8)
    head, ccols, crows, scols, srows = parse_report(lines)
    want = sorted(((int(cells[a, b]), a, b) for a in range(128) for b in range(128) if cells[a, b]), key=lambda t: (-t[0], t[1], t[2]))
    assert len(want) == 128 * 127 and len(crows) == 10001
    assert [(r[0], r[1], int(r[2])) for r in crows[:10000]] == [(_word(a, 8), _word(b, 8), c) for c, a, b in want[:10000]]
    assert crows[10000] == ["other_cells", str(len(want) - 10000), str(sum(c for c, _, _ in want[10000:]))]
    assert len(srows) == 128
    # exactly 10 000 cells: no `other_cells` line
    flat = cells[:128, :128].reshape(-1).copy()
    flat[np.flatnonzero(flat)[10000:]] = 0
    cells[:128, :128] = flat.reshape(128, 128)
    lines, _ = _lines(np.concatenate([cells.reshape(-1), np.zeros(1, np.uint64)]), bcs, 16, 8)
    crows = parse_report(lines)[2]
    assert len(crows) == 10000 and crows[-1][0] != "other_cells"


def test_writer_shared_sums_on_the_combinatorial_sheet():
    bcs, K, w1 = SHEETS["combinatorial"]
    rng = np.random.default_rng(9)
    cells = rng.integers(1, 50, (9, 13)).astype(np.uint64)
    P1, P2, part1, part2 = HM.part_lists(bcs, K, w1)
    for a, b in zip(part1, part2):
        cells[a, b] = 0  # the on-sheet cells
    table = np.concatenate([cells.reshape(-1), np.array([2], np.uint64)])
    lines, _ = _lines(table, bcs, K, w1)
    head, ccols, crows, scols, srows = parse_report(lines)
    left_off = [(_word(100 + a, 8), _word(900 + b, 8)) for a, b in [(0, 0), (1, 5), (3, 3), (4, 11), (7, 0), (7, 11)]]
    assert all(cells[P1[s1], P2[s2]] > 0 for s1, s2 in left_off)
    assert sorted((r[0], r[1]) for r in crows) == sorted(left_off)  # the only cells with both parts known that are off the sheet
    assert len(srows) == 90
    by_a, by_b = {}, {}
    for r, a, b in zip(srows, part1, part2):
        by_a.setdefault(a, set()).add((r[4], r[6]))
        by_b.setdefault(b, set()).add((r[5], r[7]))
        assert int(r[4]) == int(cells[a, :12].sum()) and int(r[5]) == int(cells[:8, b].sum())
        assert int(r[6]) == int(cells[a, 12]) and int(r[7]) == int(cells[8, b])
    assert all(len(v) == 1 for v in by_a.values()) and all(len(v) == 1 for v in by_b.values())  # samples sharing a part share its sums
    assert all(r[4].count(",") >= 9 and r[5].count(",") >= 5 for r in crows)  # the samples that carry each part, comma-joined


def test_writer_divisor_zero_and_lower_bound_line():
    bcs, K, w1 = SHEETS["single_sample"]
    table = np.zeros(5, np.uint64)
    lines, _ = _lines(table, bcs, K, w1, assigned=[0])
    head, ccols, crows, scols, srows = parse_report(lines)
    assert head[-1] == "unexpected_per_100000\t0" and "undetermined\t0" in head and crows == []
    assert srows == [["S0", "ACGTACGT", "TTTTAAAA", "0", "0", "0", "0", "0"]]
    assert hr.LOWER_BOUND_LINE not in lines
    for budgets in ((1, 0), (0, 2), (1, 1)):
        lines, _ = _lines(table, bcs, K, w1, budgets=budgets, assigned=[0])
        at = lines.index("mismatch budgets\t%d,%d" % budgets)
        assert lines[at + 1] == "Exact per-part matching: rates are lower bounds" == hr.LOWER_BOUND_LINE
        assert lines[at + 2].startswith("pairs\t")
    with pytest.raises(AssertionError):
        hr.report_lines(np.zeros(4, np.uint64), 1, 1, [0], [0], [("S0", bcs[0])], 8, (0, 0), 0, [0])


def test_exported_symbols_and_abi():
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    new = {"qd_hop_index", "qd_hop_enable", "qd_hop_shape", "qd_hop_read", "qd_hop_add"}
    assert new <= names
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    assert all(("int %s(" % n) in text for n in new) and new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text  # additive: the version stays
