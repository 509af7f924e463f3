# -*- coding: utf-8 -*-
"""
Quade_filter_report.csv: what the read filter ([filter] section, conf.FILTER_HELP) dropped -- the parameters, then for every
destination (<sample>_pass, <sample>_fail, Undetermined) and Total the eight counters of the device table (include/quade_hip.h,
qd_filter_*): pairs in, pairs kept, pairs dropped per reason, bases in and bases kept, with the percentages of pairs and of bases
kept.  The reference has no counterpart.  Integer arithmetic only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, write_lines
from .stages import FILTER_COUNTERS as COUNTERS  # a destination's row of the table
from .stages import FILTER_KEYS as PARAMS
from .stages import FILTER_REASONS as REASONS

REPORT_NAME = "Quade_filter_report.csv"
PROGRAM = "Quade-filter " + QUADE_VERSION.split()[-1]
COLUMNS = ("destination", "pairs_in", "pairs_kept") + REASONS + ("bases_in", "bases_kept", "percent_pairs_kept", "percent_bases_kept")
PAIRS, BASES_IN, BASES_DROPPED = 0, 6, 7


def _row(name, c):
    c = [int(x) for x in c]
    kept, bases = c[PAIRS] - sum(c[1:6]), c[BASES_IN] - c[BASES_DROPPED]
    return "\t".join([name, str(c[PAIRS]), str(kept)] + [str(x) for x in c[1:6]] + [str(c[BASES_IN]), str(bases), ratio(kept, c[PAIRS], 100),
                                                                                  ratio(bases, c[BASES_IN], 100)])


def report_lines(table, samples, params):
    """The file's lines.  table: [2 * S + 1][8] (qd_filter_read); samples: the names in sheet order; params: a mapping with PARAMS
    (None or absent = the rule is off, written as an empty value)."""
    rows = [[int(x) for x in row] for row in table]
    assert len(rows) == 2 * len(samples) + 1 and all(len(r) == len(COUNTERS) for r in rows), "one row of 8 per destination"
    lines = ["Program " + PROGRAM, ""]
    lines += ["%s\t%s" % (name, "" if params.get(name) is None else params[name]) for name in PARAMS]
    lines += ["", "\t".join(COLUMNS)]
    names = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined"]
    for name, c in zip(names, rows):
        lines.append(_row(name, c))
    lines.append(_row("Total", [sum(col) for col in zip(*rows)]))
    return lines


def write_report(path, table, samples, params):
    write_lines(path, report_lines(table, samples, params))
