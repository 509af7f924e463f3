# -*- coding: utf-8 -*-
"""
Quade_trim_report.csv: what the 3' trimming of the insert reads ([trim] section, conf.TRIM_HELP) removed -- the parameters, then
for R1, R2 and both the eight counters of the device table (include/quade_hip.h, qd_trim_*) and the shares of reads and bases
trimmed.  The reference has no counterpart.  Integer arithmetic only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio

REPORT_NAME = "Quade_trim_report.csv"
PROGRAM = "Quade-trim " + QUADE_VERSION.split()[-1]
COUNTERS = ("reads", "bases_in", "bases_out", "quality_trimmed_reads", "quality_trimmed_bases", "adapter_reads", "adapter_bases",
            "floored_reads")  # a table row (hip_backend.TRIM_COUNTERS)
COLUMNS = ("read",) + COUNTERS + ("percent_quality_trimmed_reads", "percent_adapter_reads", "percent_bases_trimmed")
PARAMS = ("adapter_r1", "adapter_r2", "quality_cutoff", "min_overlap", "max_mismatch_pct", "min_length")
READS, BASES_IN, BASES_OUT, Q_READS, Q_BASES, A_READS, A_BASES, FLOORED = range(8)


def _row(name, c):
    c = [int(x) for x in c]
    return "\t".join([name] + [str(x) for x in c] + [ratio(c[Q_READS], c[READS], 100), ratio(c[A_READS], c[READS], 100),
                                                     ratio(c[BASES_IN] - c[BASES_OUT], c[BASES_IN], 100)])


def report_lines(table, params):
    """The file's lines.  table[r][k]: r = 0 / 1 for R1 / R2, k as COUNTERS; params: a mapping with PARAMS' keys (an unset adapter
    is the empty string)."""
    assert len(table) == 2 and all(len(t) == len(COUNTERS) for t in table), "the table holds 2 x 8 counters"
    lines = ["Program " + PROGRAM, ""]
    lines += ["%s\t%s" % (k, params[k]) for k in PARAMS]
    lines += ["", "\t".join(COLUMNS)]
    rows = [[int(x) for x in t] for t in table]
    for name, c in (("R1", rows[0]), ("R2", rows[1]), ("Total", [a + b for a, b in zip(*rows)])):
        lines.append(_row(name, c))
    return lines


def write_report(path, table, params):
    with open(path, "w") as fh:
        fh.write("\n".join(report_lines(table, params)) + "\n")
