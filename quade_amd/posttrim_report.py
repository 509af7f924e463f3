# -*- coding: utf-8 -*-
"""
Quade_post_trim_report.csv: what the post-trimming of the insert reads ([trim] section, conf.POSTTRIM_HELP) removed behind the
adapter and overlap trimming -- the parameters, then for R1, R2 and both the sixteen counters of the device table
(include/quade_hip.h, qd_posttrim_*) and the shares of reads and bases cut.  The reference has no counterpart.  Integer
arithmetic only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, read_report_lines, write_lines
from .stages import POSTTRIM_COUNTERS as COUNTERS  # a table row

REPORT_NAME = "Quade_post_trim_report.csv"
PROGRAM = "Quade-post-trim " + QUADE_VERSION.split()[-1]
COLUMNS = ("read",) + COUNTERS + ("percent_n_tail_reads", "percent_polyx_reads", "percent_cropped_reads", "percent_bases_trimmed")
PARAMS = ("tail_n", "poly_x_min_length", "max_length_r1", "max_length_r2", "min_length")  # 0 = the rule is off
(READS, BASES_IN, BASES_OUT, N_READS, N_BASES, A_READS, A_BASES, C_READS, C_BASES, G_READS, G_BASES, T_READS, T_BASES, CROP_READS,
 CROP_BASES, FLOORED) = range(16)


def _shares(c):
    return [ratio(c[N_READS], c[READS], 100), ratio(c[A_READS] + c[C_READS] + c[G_READS] + c[T_READS], c[READS], 100),
            ratio(c[CROP_READS], c[READS], 100), ratio(c[BASES_IN] - c[BASES_OUT], c[BASES_IN], 100)]


def report_lines(table, params):
    """The file's lines.  table[r][k]: r = 0 / 1 for R1 / R2, k as COUNTERS; params: a mapping with PARAMS' keys."""
    assert len(table) == 2 and all(len(t) == len(COUNTERS) for t in table), "the table holds 2 x 16 counters"
    return read_report_lines(PROGRAM, ["%s\t%s" % (k, params[k]) for k in PARAMS], COLUMNS, table, _shares)


def write_report(path, table, params):
    write_lines(path, report_lines(table, params))
