"""Mismatch-tolerant matching, host side (no GPU): the [index] options, the host-only collision check against a brute force
written from the rule (tests/mismatch_model.py), and the command line on a colliding sample sheet; and the ground the GPU tests of the
tight and combinatorial sheets stand on: the brute-force model of the routing codes pinned to the unmodified oracle with the tolerant
lookup installed, and the conditions that keep every corpus of tests/mismatch_support.py from going hollow."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from quade_amd import synth
from quade_amd.conf import MISMATCH_HELP, QuadeConf, template_bytes
from tests import helpers as H
from tests import mismatch_model as MM
from tests import mismatch_support as MS

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


# ---- the tight and combinatorial corpora of the GPU tests: the model pinned to the oracle, and the corpora kept from going hollow ----
def test_model_by_hand():
    K, w1, q40 = 4, 2, np.full((1, 4), 73, np.uint8)
    one = lambda key, sheet, m1, m2, quals=q40: int(MM.codes_for_keys(np.frombuffer(key, np.uint8)[None, :], quals, sheet, K, w1, m1, m2, 25)[0])  # noqa: E731
    sheet = ["ACGT", "TTTTT", "GGCC"]
    assert one(b"GGCC", sheet, 0, 0) == 4 and one(b"GGCA", sheet, 0, 0) == 0xFFFF
    assert one(b"GGCA", sheet, 0, 1) == 4 and one(b"GGCA", sheet, 1, 0) == 0xFFFF  # the budgets are per part
    assert one(b"GGAA", sheet, 1, 1) == 0xFFFF and one(b"GGAA", sheet, 0, 2) == 4 and one(b"ANGN", sheet, 1, 1) == 0  # N is a symbol
    assert one(b"TTTT", ["TTTTT", "TTT"], 2, 2) == 0xFFFF == one(b"TTTT", sheet, 1, 1)  # a barcode of another length matches exactly only
    low = q40.copy()
    low[0, 3] = 24 + 33
    at = q40.copy()
    at[0, 0] = 25 + 33
    assert one(b"ACGA", sheet, 0, 1, low) == 1 and one(b"ACGA", sheet, 0, 1, at) == 0
    # an exact hit is taken first, whatever else is within budget; without one, two barcodes within budget are a colliding sheet
    assert one(b"ACGT", ["ACGA", "ACGT"], 0, 1) == 2
    with pytest.raises(AssertionError):
        one(b"ACGC", ["ACGA", "ACGT"], 0, 1)
    codes = np.array([0, 3, 0xFFFF, 3, 4], dtype=np.uint16)
    assert MM.counts_for_codes(codes, 3).tolist() == [5, 2, 2, 1, 1, 0, 0, 2, 1, 0]


def _spheres(w, m):
    """how many strings over five symbols lie at exactly m substitutions from one of w bases"""
    return math.comb(w, m) * 4 ** m if m <= w else 0


@pytest.mark.parametrize("name", sorted(MS.CORPORA))
def test_corpus_conditions(name):
    c = MS.corpus(name)
    shape, (m1, m2), sizes, cap, alphabet = MS.CORPORA[name]
    w = (c.w1, c.K - c.w1)
    assert hb.check_mismatch_collisions(c.sheet, c.K, c.w1, m1, m2) is None
    assert len(set(c.sheet)) == len(c.sheet) == int(np.prod(sizes)) + (3 if name == "mixed_len" else 0)
    for codes, width, m in zip(c.lists, w, (m1, m2)):  # tight: no pair closer than 2m + 1 (1 at m = 0), the first pair exactly there
        d = [[MM.part_distances(a, b, width)[0] for b in codes] for a in codes]
        assert min(d[i][j] for i in range(len(codes)) for j in range(i)) == d[0][1] == max(1, 2 * m + 1)
    # every key within budget of every barcode with a neighbourhood: the whole product of the two balls, each key once
    made = np.unique(c.origin[~c.short])
    inside = (c.d1 <= m1) & (c.d2 <= m2) & ~c.short
    ball = [sum(_spheres(w[p], d) for d in range(m + 1)) for p, m in enumerate((m1, m2))]
    assert made.size == (68 if name == "comb_96x96" else int(np.prod(sizes)))
    for s in made[:: max(1, made.size // 8)]:
        mine = c.keys[inside & (c.origin == s)]
        assert mine.shape[0] == ball[0] * ball[1] == np.unique(mine, axis=0).shape[0]
    assert int(inside.sum()) == made.size * ball[0] * ball[1]
    corner = int(((c.d1 == m1) & (c.d2 == m2) & ~c.short).sum())
    assert corner == made.size * _spheres(w[0], m1) * _spheres(w[1], m2) and (corner >= 1000 or name == "single8_m1")
    # the two shells: exactly one substitution over budget on one part, within budget on the other, `cap` of each per barcode at most
    for over1, over2 in ((1, 0), (0, 1)):
        shell = (c.d1 == m1 + over1 if over1 else c.d1 <= m1) & (c.d2 == m2 + over2 if over2 else c.d2 <= m2) & ~c.short
        full = (_spheres(w[0], m1 + 1) * ball[1]) if over1 else (ball[0] * _spheres(w[1], m2 + 1))
        assert int(shell.sum()) == made.size * min(cap, full)
    outside = ((c.d1 > m1) | (c.d2 > m2)) & ~c.short
    assert int((inside | outside).sum()) == int((~c.short).sum())
    # within budget of its own barcode: that sample; some keys just outside belong to ANOTHER sample, the tight neighbour
    assert (c.codes[inside] // 2 == c.origin[inside]).all()
    assert int((outside & (c.codes != 0xFFFF) & (c.codes // 2 != c.origin)).sum()) >= 40
    assert not (outside & (c.codes // 2 == c.origin)).any()
    determined = c.codes != 0xFFFF
    for what in (c.rescued, ~determined, determined & (c.codes % 2 == 0), determined & (c.codes % 2 == 1)):
        assert int(what.sum()) >= 100
    assert (c.exact[~c.rescued] == c.codes[~c.rescued]).all()
    if name == "with_N":
        assert sum("N" in b for b in c.sheet) >= 2
    if name == "mixed_len":
        assert sorted(len(b) for b in c.sheet[-3:]) == [8, 13, 15] and c.sheet[:-3] == MS.corpus("comb_8x12").sheet
        cut = np.flatnonzero(c.short)
        assert cut.size == -(-(c.n - cut.size) // 10) and(c.keys[:c.n - cut.size] == MS.corpus("comb_8x12").keys).all()
        assert 0.4 < float((c.codes[cut] == 0xFFFF).mean()) < 0.6 and set(c.codes[cut].tolist()) == {0xFFFF} | set(range(192, 198))
    if name == "comb_96x96":
        assert 2 * len(c.sheet) > 16000  # past the rescue's per-workgroup histogram: counted in global memory
        assert min(MS.longest_candidate_lists(c.sheet, c.K, c.w1, m1, m2)) >= 96  # whichever part: lists of 96 and more


def test_which_part_the_candidate_lists_come_from():
    """the part whose longest candidate list is shorter.  Lists longer than one -- what uniform sheets never have"""
    a = MS.corpus("comb_8x12")
    # index read 1's part: its 8 codes share no half, so 12 samples per list; three of the other part's 12 codes share a half (3 x 8)
    assert MS.longest_candidate_lists(a.sheet, 16, 8, 1, 1) == [12, 24]
    b = MS.corpus("comb_12x8_m10")
    # index read 2's part, whole (budget 0: one segment), 8 codes in 12 samples each; two of the 12 codes of part 1 share a half (2 x 8)
    assert MS.longest_candidate_lists(b.sheet, 16, 8, 1, 0) == [16, 12]
    c = MS.corpus("comb_12x8_m01")
    assert MS.longest_candidate_lists(c.sheet, 16, 8, 0, 1) == [12, 16]   # the mirror image: index read 1's part, whole
    assert MS.longest_candidate_lists(MS.corpus("comb_96x96").sheet, 16, 8, 1, 1) == [384, 288]  # index read 2's part
    far = synth.make_far_barcodes(96, 8, 8, 1, 1, seed=1)
    assert MS.longest_candidate_lists(far, 16, 8, 1, 1) == [4, 3]  # uniform draws: the few that share a 4-base half by chance
    for shape, (m1, m2) in MS.NO_SEGMENTS.items():
        s = MS.TIGHT[shape]
        assert MS.longest_candidate_lists(["AC"], s.w1 + s.w2, s.w1, m1, m2) == [None, None]


def _oracle_on(monkeypatch, c, rows):
    monkeypatch.setattr(qo, "SampleSet", MM.tolerant_sampleset(qo, c.K, c.w1, c.m1, c.m2))
    reads = []
    for s, q in c.streams:
        reads += [[s[r].decode() for r in rows], [q[r].decode() for r in rows]]
    if len(c.streams) == 1:
        reads += [None, None]
    return H.oracle_on_reads(c.sheet, c.shape.plan, *reads)


@pytest.mark.parametrize("name", sorted(MS.CORPORA) + ["no_segments_" + s for s in sorted(MS.NO_SEGMENTS)])
def test_model_agrees_with_the_tolerant_oracle(monkeypatch, name):
    """the unmodified oracle with TolerantIndex installed, on a seeded sub-sample of every corpus's reads: every code, the
    fused slice, the molecular bytes and the counter vector"""
    c = MS.no_segments_corpus(name[len("no_segments_"):]) if name.startswith("no_segments_") else MS.corpus(name)
    rows = c.sample(4000, seed=11)
    assert rows.size == min(4000, c.n) and (not c.short.any() or c.short[rows].sum() >= min(100, c.short.sum()))
    codes, idx, mol, counts = _oracle_on(monkeypatch, c, rows)
    assert (codes == c.codes[rows]).all(), rows[np.flatnonzero(codes != c.codes[rows])[:10]]
    assert (counts == c.counts(c.codes[rows])).all()
    full = rows[~c.short[rows]]
    assert [i.upper().encode() for i, r in zip(idx, rows) if not c.short[r]] == [c.keys[r].tobytes() for r in full]
    if c.shape.plan.mol1_end:
        want = c.molecular()
        assert mol == [want[r].decode() for r in rows] and len(want[0]) == 3
    # and without budgets: what the model calls rescued is Undetermined, everything else keeps its code
    monkeypatch.setattr(c, "m1", 0)
    monkeypatch.setattr(c, "m2", 0)
    codes0 = _oracle_on(monkeypatch, c, rows)[0]
    assert (codes0 == c.exact[rows]).all() and (codes0[c.rescued[rows]] == 0xFFFF).all()


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
