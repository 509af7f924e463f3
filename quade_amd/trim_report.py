# -*- coding: utf-8 -*-
"""
Quade_trim_report.csv: what the 3' trimming of the insert reads ([trim] section, conf.TRIM_HELP) removed -- the parameters, then
for R1, R2 and both the eight counters of the device table (include/quade_hip.h, qd_trim_*) and the shares of reads and bases
trimmed.  The reference has no counterpart.  Integer arithmetic only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, read_report_lines, write_lines
from .stages import TRIM_COUNTERS as COUNTERS  # a table row

REPORT_NAME = "Quade_trim_report.csv"
PROGRAM = "Quade-trim " + QUADE_VERSION.split()[-1]
COLUMNS = ("read",) + COUNTERS + ("percent_quality_trimmed_reads", "percent_adapter_reads", "percent_bases_trimmed")
PARAMS = ("adapter_r1", "adapter_r2", "quality_cutoff", "min_overlap", "max_mismatch_pct", "min_length")
READS, BASES_IN, BASES_OUT, Q_READS, Q_BASES, A_READS, A_BASES, FLOORED = range(8)


def _shares(c):
    return [ratio(c[Q_READS], c[READS], 100), ratio(c[A_READS], c[READS], 100), ratio(c[BASES_IN] - c[BASES_OUT], c[BASES_IN], 100)]


def report_lines(table, params):
    """The file's lines.  table[r][k]: r = 0 / 1 for R1 / R2, k as COUNTERS; params: a mapping with PARAMS' keys (an unset adapter
    is the empty string)."""
    assert len(table) == 2 and all(len(t) == len(COUNTERS) for t in table), "the table holds 2 x 8 counters"
    return read_report_lines(PROGRAM, ["%s\t%s" % (k, params[k]) for k in PARAMS], COLUMNS, table, _shares)


def write_report(path, table, params):
    write_lines(path, report_lines(table, params))
