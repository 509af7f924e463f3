# -*- coding: utf-8 -*-
"""
Quade_clip_report.csv: what the end clipping, sliding-window and poly-G trimming of the insert reads ([trim] section,
conf.CLIP_HELP) removed -- the parameters, then for R1, R2 and both the twelve counters of the device table
(include/quade_hip.h, qd_clip_*) and the shares of reads and bases cut.  The reference has no counterpart.  Integer arithmetic
only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, read_report_lines, write_lines
from .stages import CLIP_COUNTERS as COUNTERS  # a table row

REPORT_NAME = "Quade_clip_report.csv"
PROGRAM = "Quade-clip " + QUADE_VERSION.split()[-1]
COLUMNS = ("read",) + COUNTERS + ("percent_window_reads", "percent_polyg_reads", "percent_bases_clipped")
PARAMS = ("front_clip_r1", "front_clip_r2", "tail_clip_r1", "tail_clip_r2", "window_size", "window_quality", "poly_g_min_length",
          "min_length")  # 0 = the rule is off
READS, BASES_IN, BASES_OUT, F_READS, F_BASES, T_READS, T_BASES, W_READS, W_BASES, G_READS, G_BASES, FLOORED = range(12)


def _shares(c):
    return [ratio(c[W_READS], c[READS], 100), ratio(c[G_READS], c[READS], 100), ratio(c[BASES_IN] - c[BASES_OUT], c[BASES_IN], 100)]


def report_lines(table, params):
    """The file's lines.  table[r][k]: r = 0 / 1 for R1 / R2, k as COUNTERS; params: a mapping with PARAMS' keys."""
    assert len(table) == 2 and all(len(t) == len(COUNTERS) for t in table), "the table holds 2 x 12 counters"
    return read_report_lines(PROGRAM, ["%s\t%s" % (k, params[k]) for k in PARAMS], COLUMNS, table, _shares)


def write_report(path, table, params):
    write_lines(path, report_lines(table, params))
