# -*- coding: utf-8 -*-
"""
Quade_clip_report.csv: what the end clipping, sliding-window and poly-G trimming of the insert reads ([trim] section,
conf.CLIP_HELP) removed -- the parameters, then for R1, R2 and both the twelve counters of the device table
(include/quade_hip.h, qd_clip_*) and the shares of reads and bases cut.  The reference has no counterpart.  Integer arithmetic
only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio

REPORT_NAME = "Quade_clip_report.csv"
PROGRAM = "Quade-clip " + QUADE_VERSION.split()[-1]
COUNTERS = ("reads", "bases_in", "bases_out", "front_clipped_reads", "front_clipped_bases", "tail_clipped_reads", "tail_clipped_bases",
            "window_reads", "window_bases", "polyg_reads", "polyg_bases", "floored_reads")  # a table row (hip_backend.CLIP_COUNTERS)
COLUMNS = ("read",) + COUNTERS + ("percent_window_reads", "percent_polyg_reads", "percent_bases_clipped")
PARAMS = ("front_clip_r1", "front_clip_r2", "tail_clip_r1", "tail_clip_r2", "window_size", "window_quality", "poly_g_min_length",
          "min_length")  # 0 = the rule is off
READS, BASES_IN, BASES_OUT, F_READS, F_BASES, T_READS, T_BASES, W_READS, W_BASES, G_READS, G_BASES, FLOORED = range(12)


def _row(name, c):
    c = [int(x) for x in c]
    return "\t".join([name] + [str(x) for x in c] + [ratio(c[W_READS], c[READS], 100), ratio(c[G_READS], c[READS], 100),
                                                     ratio(c[BASES_IN] - c[BASES_OUT], c[BASES_IN], 100)])


def report_lines(table, params):
    """The file's lines.  table[r][k]: r = 0 / 1 for R1 / R2, k as COUNTERS; params: a mapping with PARAMS' keys."""
    assert len(table) == 2 and all(len(t) == len(COUNTERS) for t in table), "the table holds 2 x 12 counters"
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
