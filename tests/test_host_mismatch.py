"""Mismatch-tolerant matching, host side (no GPU): the [index] options, the host-only collision check against a brute force
written from the rule (tests/mismatch_model.py), and the command line on a colliding sample sheet."""
import os
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import hip_backend as hb
from quade_amd import synth
from quade_amd.conf import MISMATCH_HELP, QuadeConf, template_bytes
from tests import mismatch_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(tmp_path, index_extra="", dual=True, samples=(("S1", "ACGTACGT", "TTGGCCAA"), ("S2", "GGGGAAAA", "CCCCTTTT"))):
    names = ["r1.fq", "r2.fq", "i1.fq", "i2.fq"]
    for n in names:
        (tmp_path / n).write_bytes(b"")
    text = ("[quality]\nminimal_qual : 25\n[fastq]\nseq_R1 : {0}/r1.fq\nseq_R2 : {0}/r2.fq\nindex_R1 : {0}/i1.fq\n"
            "index_R2 : {0}/i2.fq\n[index]\nindex2 : {1}\nmolecular1 : False\nmolecular2 : False\nindex1_start : 1\n"
            "index1_end : 8\nindex2_start : 1\nindex2_end : 8\n{2}[output]\nwrite_pass : True\nwrite_fail : True\n"
            "write_undetermined : True\n").format(tmp_path, dual, index_extra)
    for i, (name, a, b) in enumerate(samples):
        text += "[sample%d]\nname : %s\nindex1_seq : %s\nindex2_seq : %s\n" % (i + 1, name, a, b)
    p = tmp_path / "conf.txt"
    p.write_text(text)
    return str(p)


def test_conf_budgets_default_to_zero(tmp_path):
    cf = QuadeConf(_conf(tmp_path))
    assert (cf.idx1_mismatches, cf.idx2_mismatches) == (0, 0)
    cf = QuadeConf(_conf(tmp_path, "index1_mismatches : 1\nindex2_mismatches : 2\n"))
    assert (cf.idx1_mismatches, cf.idx2_mismatches) == (1, 2)
    # single index: index2_mismatches is ignored, as index2_start / index2_end are
    cf = QuadeConf(_conf(tmp_path, "index1_mismatches : 2\nindex2_mismatches : 2\n", dual=False))
    assert (cf.idx1_mismatches, cf.idx2_mismatches) == (2, 0)
    assert "index1_mismatches" in MISMATCH_HELP and "index2_mismatches" in MISMATCH_HELP


@pytest.mark.parametrize("extra,msg", [("index1_mismatches : 3\n", "index1_mismatches : 0 to 2"),
                                       ("index2_mismatches : -1\n", "index2_mismatches : 0 to 2")])
def test_conf_budget_range(tmp_path, extra, msg):
    with pytest.raises(AssertionError) as ei:
        QuadeConf(_conf(tmp_path, extra))
    assert msg in str(ei.value)
    with pytest.raises(ValueError):
        QuadeConf(_conf(tmp_path, "index1_mismatches : one\n"))


def test_template_is_unchanged(tmp_path):
    golden = os.path.join(ROOT, "tests", "golden", "bundled", "result", "Quade_conf_file.txt")
    with open(golden, "rb") as fh:
        assert template_bytes() == fh.read()
    assert b"mismatches" not in template_bytes()


def test_new_entry_points_are_typed():
    names = {s[0] for s in hb.SYMBOLS}
    assert {"qd_check_mismatch_collisions", "qd_set_mismatches"} <= names
    assert hasattr(hb.Engine, "set_mismatches")


def _random_sheet(rng, S, K, alphabet, other_len=0.0):
    out = set()
    while len(out) < S:
        L = K if rng.random() >= other_len else int(rng.integers(max(1, K - 2), K + 3))
        out.add("".join(rng.choice(list(alphabet), L)))
    out = list(out)
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("seed", range(6))
def test_collision_check_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    seen = {True: 0, False: 0}
    for trial in range(60):
        dual = trial % 3 != 0
        K = int(rng.integers(2, 11))
        w1 = int(rng.integers(1, K)) if dual else K  # the split at w1 anywhere inside the key
        m1 = int(rng.integers(0, 3))
        m2 = int(rng.integers(0, 3)) if dual else 0
        alphabet = "ACGTN" if trial % 2 else "ACGT"
        S = int(rng.integers(2, min(40, len(alphabet) ** K // 2)))
        bcs = _random_sheet(rng, S, K, alphabet, other_len=0.3 if trial % 4 == 1 else 0.0)
        want = MM.first_collision(bcs, K, w1, m1, m2)
        got = hb.check_mismatch_collisions(bcs, K, w1, m1, m2)
        assert got == want, (bcs, K, w1, m1, m2)
        seen[want is None] += 1
    assert seen[True] and seen[False]  # both outcomes were exercised


def test_collision_check_details():
    K, w1 = 4, 2
    # N is an ordinary symbol: "ACNN" vs "ACGT" differ in two bytes of part 2
    assert hb.check_mismatch_collisions(["ACNN", "ACGT"], K, w1, 0, 1) == (0, 1)
    assert hb.check_mismatch_collisions(["ACNN", "ACGT"], K, w1, 1, 0) is None
    # a barcode whose length is not K never collides (it matches exactly only)
    assert hb.check_mismatch_collisions(["ACG", "ACGT", "ACGA"], K, w1, 0, 1) == (1, 2)
    assert hb.check_mismatch_collisions(["ACG", "ACGT", "ACGAA"], K, w1, 2, 2) is None
    # the first colliding pair in ordinal order (i, then j)
    sheet = ["AAAA", "CCCC", "CCCA", "AAAC", "CCAA"]
    assert hb.check_mismatch_collisions(sheet, K, w1, 0, 1) == MM.first_collision(sheet, K, w1, 0, 1) == (0, 3)
    # m = 0 on both parts: only equal barcodes collide
    assert hb.check_mismatch_collisions(sheet, K, w1, 0, 0) is None
    with pytest.raises(hb.QuadeHipError):
        hb.check_mismatch_collisions(sheet, K, w1, 3, 0)
    with pytest.raises(hb.QuadeHipError):
        hb.check_mismatch_collisions(sheet, K, K + 1, 1, 0)


def test_far_sheet_generator_does_not_collide():
    for (w1, w2, m1, m2, S) in [(8, 8, 1, 1, 1536), (8, 8, 2, 2, 24), (8, 0, 1, 0, 40)]:
        bcs = synth.make_far_barcodes(S, w1, w2, m1, m2, seed=4)
        assert len(set(bcs)) == S and all(len(b) == w1 + w2 for b in bcs)
        assert hb.check_mismatch_collisions(bcs, w1 + w2, w1, m1, m2) is None
    # the existing generator is untouched: cfg5's uniform sheet collides under (1, 1)
    w = synth.generate("cfg5", 16, seed=3)
    assert hb.check_mismatch_collisions(w.barcode_strings(), 16, 8, 1, 1) is not None


def _run_cli(conf, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "quade_amd.quade", "-c", conf], cwd=str(cwd), env=env,
                          capture_output=True, text=True, timeout=300)


def test_cli_rejects_a_colliding_sheet(tmp_path):
    samples = (("A1", "ACGTACGT", "TTGGCCAA"), ("B2", "GGGGAAAA", "CCCCTTTT"), ("C3", "ACGTACGA", "TTGGCCAT"))
    conf = _conf(tmp_path, "index1_mismatches : 1\nindex2_mismatches : 1\n", samples=samples)
    r = _run_cli(conf, tmp_path)
    assert r.returncode == 1, r.stdout + r.stderr
    assert ("One of the value in the configuration file is not correct\n"
            "A1 and C3 : Index collision with index1_mismatches=1 index2_mismatches=1") in r.stdout
    # under (1, 0) the same sheet does not collide (d2 = 1 > 0), and (0, 0) is the reference's exact matching
    for extra in ("index1_mismatches : 1\n", ""):
        r = _run_cli(_conf(tmp_path, extra, samples=samples), tmp_path)
        assert "Index collision" not in r.stdout
