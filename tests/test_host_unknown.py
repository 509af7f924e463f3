"""The unknown-barcode report off the GPU: the conf option, the host merge of the tables, the writer (order, ties, percent,
escaping, columns, nearest sample against brute force) and the exported symbols."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import unknown_report as ur
from tests import unknown_model as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(tmp_path, output_extra="", dual=True, gpu=""):
    f = tmp_path / "reads.fastq"
    f.write_text("")
    txt = "[quality]\nminimal_qual : 25\n[fastq]\nseq_R1 : {0}\nseq_R2 : {0}\nindex_R1 : {0}\n".format(f)
    if dual:
        txt += "index_R2 : {0}\n".format(f)
    txt += "[index]\nindex2 : %s\nmolecular1 : False\nmolecular2 : False\nindex1_start : 1\nindex1_end : 8\n" % dual
    if dual:
        txt += "index2_start : 1\nindex2_end : 8\n"
    txt += "[output]\nwrite_pass : True\nwrite_fail : True\nwrite_undetermined : True\n" + output_extra + gpu
    txt += "[sample1]\nname : S1\nindex1_seq : ACAGACAG\n" + ("index2_seq : CTTGCTTG\n" if dual else "")
    p = tmp_path / "conf.txt"
    p.write_text(txt)
    return str(p)


@pytest.mark.parametrize("extra,want", [("", 0), ("top_unknown_barcodes :\n", 0), ("top_unknown_barcodes : 0\n", 0),
                                        ("top_unknown_barcodes : 10\n", 10), ("top_unknown_barcodes : 1000\n", 1000)])
def test_conf_option(tmp_path, extra, want):
    cf = qconf.QuadeConf(_conf(tmp_path, extra))
    assert cf.top_unknown_barcodes == want
    assert cf.unknown_slots == 1 << 24


def test_conf_option_rejected(tmp_path):
    for bad in (1001, -1):
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, "top_unknown_barcodes : %d\n" % bad))
        assert str(ei.value) == "Authorized values for top_unknown_barcodes : 0 to 1000"
    with pytest.raises(AssertionError):
        qconf.QuadeConf(_conf(tmp_path, "top_unknown_barcodes : 5\n", gpu="[gpu]\nunknown_slots : 3000\n"))
    assert qconf.QuadeConf(_conf(tmp_path, "", gpu="[gpu]\nunknown_slots : 1024\n")).unknown_slots == 1024


def test_conf_option_single_index(tmp_path):
    cf = qconf.QuadeConf(_conf(tmp_path, "top_unknown_barcodes : 7\n", dual=False))
    assert cf.top_unknown_barcodes == 7 and not cf.idx2
    assert "top_unknown_barcodes" in qconf.UNKNOWN_HELP and "unknown_slots" in qconf.UNKNOWN_HELP


def test_template_unchanged(bundled_dir):
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt"), "rb") as fh:
        assert qconf.template_bytes() == fh.read()
    assert b"top_unknown_barcodes" not in qconf.template_bytes()


def _random_table(rng, n, K, alphabet=b"ACGTN"):
    keys = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), (n, K))]
    keys = np.unique(keys, axis=0)
    rng.shuffle(keys)
    return keys, rng.integers(1, 50, keys.shape[0]).astype(np.uint64)


def test_merge_unknown_against_counter():
    rng = np.random.default_rng(3)
    tables = [_random_table(rng, n, 3) for n in (40, 90, 0, 1, 60)]  # 125 possible keys: many shared
    want = Counter()
    for k, c in tables:
        want.update(UM.table_counter(k, c))
    keys, counts = hb.merge_unknown(tables)
    assert UM.table_counter(keys, counts) == want
    assert [(bytes(k).decode(), int(c)) for k, c in zip(keys, counts)] == UM.report_order(want)
    k0, c0 = hb.merge_unknown([])
    assert len(c0) == 0 and len(k0) == 0
    # the exchange format of the ranks
    k2, c2, s2, d2 = hb.unpack_unknown(hb.pack_unknown(keys, counts, 5, 7))
    assert (k2 == keys).all() and (c2 == counts).all() and (s2, d2) == (5, 7)
    k2, c2, s2, d2 = hb.unpack_unknown(hb.pack_unknown(k0, c0, 0, 1))
    assert len(c2) == 0 and d2 == 1
    big = (np.uint64(1) << np.uint64(62))
    _, c3 = hb.merge_unknown([(keys[:1], np.array([big], np.uint64)), (keys[:1], np.array([big + np.uint64(1)], np.uint64))])
    assert int(c3[0]) == (1 << 63) + 1  # sums stay integers


def test_writer_dual(tmp_path):
    rng = np.random.default_rng(11)
    samples = [("S%d" % i, "".join(rng.choice(list("ACGT"), 16))) for i in range(40)] + [("ODD", "ACGTACGTACG")]
    samples.insert(3, ("DUP_NEAR", samples[0][1][:15] + ("A" if samples[0][1][15] != "A" else "C")))
    keys, counts = _random_table(rng, 300, 16)
    counts[:20] = 9  # ties: ordered by key bytes
    keys[5, 3], keys[6, 9], keys[7, 0] = 0x20, 0xC3, 0x7F
    keys[8] = np.frombuffer(samples[0][1].encode(), np.uint8)
    counts[5:9] = [100, 101, 102, 103]  # the rows with escapes and the planted neighbour lead the table
    keys[8, 2] = ord("N")  # one substitution from S0 (and at most two from DUP_NEAR: S0 has the lower ordinal at a tie)
    U = int(counts.sum()) + 12 + 5
    path = str(tmp_path / ur.REPORT_NAME)
    ur.write_report(path, keys, counts, 12, 5, U, 50, 8, True, samples)
    head, cols, rows = UM.parse_report(path)
    assert head == {"Pair Undetermined": str(U), "Short index slice": "12", "Not tallied": "5",
                    "Distinct barcodes tallied": str(len(counts))}
    assert cols == ["index1_seq", "index2_seq", "count", "percent_of_undetermined", "nearest_sample", "index1_distance",
                    "index2_distance"]
    want = UM.report_order(UM.table_counter(keys, counts))[:50]
    assert len(rows) == 50
    for row, (key, c) in zip(rows, want):
        assert row[0] == ur.escape(key[:8].encode("latin-1")) and row[1] == ur.escape(key[8:].encode("latin-1"))
        assert int(row[2]) == c and int(row[3]) == c * 100 // U
        assert (row[4], int(row[5]), int(row[6])) == UM.nearest_brute(key, samples, 8)
    assert ur.escape(b"A \xc3\x7fz~!") == "A\\x20\\xC3\\x7Fz~!"
    text = open(path).read()
    assert "\\x20" in text and "\\xC3" in text and "\\x7F" in text and "Date" not in text
    key8 = bytes(keys[8]).decode()
    assert UM.nearest_brute(key8, samples, 8) == ("S0", 1, 0)


def test_writer_single_index_and_no_k_long_barcode(tmp_path):
    rng = np.random.default_rng(12)
    keys, counts = _random_table(rng, 30, 6)
    samples = [("A", "ACGTAC"), ("B", "TTTTTT"), ("C", "ACG")]
    path = str(tmp_path / "u.csv")
    ur.write_report(path, keys, counts, 0, 0, int(counts.sum()), 1000, 6, False, samples)
    head, cols, rows = UM.parse_report(path)
    assert cols == ["index1_seq", "count", "percent_of_undetermined", "nearest_sample", "index1_distance"]
    assert len(rows) == len(counts)
    for row, (key, c) in zip(rows, UM.report_order(UM.table_counter(keys, counts))):
        name, d1, d2 = UM.nearest_brute(key, samples, 6)
        assert row == [key, str(c), str(c * 100 // int(counts.sum())), name, str(d1)] and d2 == 0
    # a sheet without a barcode of the key's length: the three fields stay empty
    ur.write_report(path, keys, counts, 0, 0, int(counts.sum()), 5, 3, True, [("C", "ACG")])
    _, cols, rows = UM.parse_report(path)
    assert len(cols) == 7 and all(r[4:] == ["", "", ""] for r in rows) and len(rows) == 5
    # nothing undetermined: an empty table
    ur.write_report(path, np.zeros((0, 0), np.uint8), np.zeros(0, np.uint64), 0, 0, 0, 10, 8, True, samples)
    head, cols, rows = UM.parse_report(path)
    assert head["Pair Undetermined"] == "0" and head["Distinct barcodes tallied"] == "0" and rows == []


def test_exported_symbols():
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"qd_unknown_enable", "qd_unknown_stats", "qd_unknown_read"} <= names
    assert hb.load_library().qd_version() == 6
