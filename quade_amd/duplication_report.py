# -*- coding: utf-8 -*-
"""
Quade_duplication_report.csv: the library duplication rate ([output] duplication_report, conf.DUPLICATION_HELP) -- the parameters,
then for every destination (<sample>_pass, <sample>_fail, Undetermined) and Total the five counters of the device table
(include/quade_hip.h, qd_dup_*) with what the key table adds to them (tallied pairs, distinct keys, duplicate pairs and their
percentage), then the duplication levels of the whole run: how many keys, and how many pairs, occur once, twice, ... (1 to 31 and
>=32; only the levels that occur).  Every figure is over the sampled keys: a sampled key keeps its exact multiplicity, so the rates
are unbiased estimates of the library's.  The reference has no counterpart.  Integer arithmetic only and no date, so that files
can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, write_lines

REPORT_NAME = "Quade_duplication_report.csv"
PROGRAM = "Quade-duplication " + QUADE_VERSION.split()[-1]
PARAMS = ("bases", "sample", "slots")
COUNTERS = ("pairs", "short", "with_n", "sampled", "not_tallied")  # a destination's row of the table (hip_backend.DUP_COUNTERS)
COLUMNS = ("destination", "pairs", "short", "with_n", "keyed", "sampled", "not_tallied", "tallied", "distinct", "duplicate_pairs",
           "duplication_pct")
LEVEL_COLUMNS = ("duplication_level", "keys", "pairs")
TOP_LEVEL = 32  # the last bin: this many occurrences and more
PAIRS, SHORT, WITH_N, SAMPLED, NOT_TALLIED = range(5)


def _row(name, c, tallied, distinct):
    keyed = c[PAIRS] - c[SHORT] - c[WITH_N]
    return "\t".join([name] + [str(x) for x in (c[PAIRS], c[SHORT], c[WITH_N], keyed, c[SAMPLED], c[NOT_TALLIED], tallied, distinct,
                                                tallied - distinct)] + [ratio(tallied - distinct, tallied, 100)])


def report_lines(stats, keys, counts, samples, params):
    """The file's lines.  stats: [2 * S + 1][5] (qd_dup_stats, summed over contexts and ranks); keys [n][3] = (w1, w2, d) with
    counts [n]: the merged key table, every key once, in any order; samples: the names in sheet order; params: a mapping with
    PARAMS."""
    rows = [[int(x) for x in row] for row in stats]
    samples = list(samples)
    assert len(rows) == 2 * len(samples) + 1 and all(len(r) == len(COUNTERS) for r in rows), "one row of 5 per destination"
    assert len(keys) == len(counts), "one count per key"
    tallied, distinct = [0] * len(rows), [0] * len(rows)
    levels = {}  # level -> [keys, pairs]
    for k, c in zip(keys, counts):
        d, c = int(k[2]), int(c)
        assert 0 <= d < len(rows) and c > 0, "a key of no destination, or an entry without pairs"
        tallied[d] += c
        distinct[d] += 1
        lv = levels.setdefault(min(c, TOP_LEVEL), [0, 0])
        lv[0] += 1
        lv[1] += c
    lines = ["Program " + PROGRAM, ""]
    lines += ["%s\t%s" % (name, params[name]) for name in PARAMS]
    lines += ["", "\t".join(COLUMNS)]
    names = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined"]
    for name, c, t, u in zip(names, rows, tallied, distinct):
        lines.append(_row(name, c, t, u))
    lines.append(_row("Total", [sum(col) for col in zip(*rows)], sum(tallied), sum(distinct)))
    lines += ["", "\t".join(LEVEL_COLUMNS)]
    for level in sorted(levels):
        lines.append("\t".join([str(level) if level < TOP_LEVEL else ">=%d" % TOP_LEVEL] + [str(x) for x in levels[level]]))
    return lines


def write_report(path, stats, keys, counts, samples, params):
    write_lines(path, report_lines(stats, keys, counts, samples, params))
