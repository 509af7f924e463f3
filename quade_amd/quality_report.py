# -*- coding: utf-8 -*-
"""
Quade_quality_report.csv: what every destination received ([output] quality_report, conf.QUALITY_HELP) -- reads, bases, bases
at or above Q20 and Q30, mean quality, mean length and N content, for R1 and R2.  The reference has no counterpart (Quade 0.3.2
reports pair counts only).  The counters come from the device (include/quade_hip.h, qd_qstats_*); everything here is integer
arithmetic on 2 * (2 * S + 2) rows, so that the text is reproducible and files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION

REPORT_NAME = "Quade_quality_report.csv"
PROGRAM = "Quade-quality " + QUADE_VERSION.split()[-1]  # (no date: the file can be compared whole)
COLUMNS = ("destination", "read", "reads", "bases", "mean_length", "q20_bases", "q30_bases", "percent_q20", "percent_q30",
           "mean_quality", "n_bases", "percent_n")
RECORDS, BASES, QUAL_SUM, Q20, Q30, N_BASES = range(6)  # a table row (stages.QSTATS_COUNTERS)


def ratio(x, y, scale=1):
    """x * scale / y with two decimals, rounded down; 0.00 when y is 0"""
    if not y:
        return "0.00"
    v = int(x) * scale * 100 // int(y)
    return "%d.%02d" % (v // 100, v % 100)


def write_lines(path, lines):
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_report_lines(program, params, columns, table, shares):
    """The body the read-scoped reports share: the program line, the parameters block (params: its lines), the column names, then
    one row for R1, R2 and Total: the row's counters, then shares(counters), the ratio columns."""
    lines = ["Program " + program, ""] + list(params) + ["", "\t".join(columns)]
    rows = [[int(x) for x in t] for t in table]
    for name, c in (("R1", rows[0]), ("R2", rows[1]), ("Total", [a + b for a, b in zip(*rows)])):
        lines.append("\t".join([name] + [str(x) for x in c] + shares(c)))
    return lines


def _row(name, read, c):
    c = [int(x) for x in c]
    return "\t".join([name, read, str(c[RECORDS]), str(c[BASES]), ratio(c[BASES], c[RECORDS]), str(c[Q20]), str(c[Q30]),
                      ratio(c[Q20], c[BASES], 100), ratio(c[Q30], c[BASES], 100), ratio(c[QUAL_SUM], c[BASES]), str(c[N_BASES]),
                      ratio(c[N_BASES], c[BASES], 100)])


def report_lines(table, samples):
    """The file's lines.  table[d][r][k]: destination d = routing code (2 * i = sample i's pass, 2 * i + 1 = its fail, 2 * S =
    Undetermined), r = 0 / 1 for R1 / R2, k as hip_backend.QSTATS_COUNTERS; samples: the names in ordinal order.  Every
    destination is listed, also one without reads or whose files are not written."""
    samples = list(samples)
    assert len(table) == 2 * len(samples) + 1, "the table holds 2 * S + 1 destinations"
    names = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined"]
    lines = ["Program " + PROGRAM, "", "\t".join(COLUMNS)]
    total = [[0] * 6, [0] * 6]
    for d, name in enumerate(names):
        for r, read in enumerate(("R1", "R2")):
            c = [int(x) for x in table[d][r]]
            total[r] = [a + b for a, b in zip(total[r], c)]
            lines.append(_row(name, read, c))
    for r, read in enumerate(("R1", "R2")):
        lines.append(_row("Total", read, total[r]))
    return lines


def write_report(path, table, samples):
    write_lines(path, report_lines(table, samples))
