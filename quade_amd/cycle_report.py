# -*- coding: utf-8 -*-
"""
Quade_cycle_report.csv: quality and base content by cycle, and the distributions of read length, per-read mean quality and
per-read GC percent ([output] cycle_report, conf.CYCLE_HELP) -- for the groups pass, fail, Undetermined and their Total, and for
R1 and R2.  The reference has no counterpart.  The counters come from the device (include/quade_hip.h, qd_cstats_*, which
defines every one of them); everything here is integer arithmetic, so that the text is reproducible and files can be compared
whole.

Derived values: reads(c), the reads that have a cycle c, is not stored: it is the sum of the length bins minus the sum of
len[0..c].  other(c) = reads(c) - A - C - G - T - N.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, write_lines
from .stages import CSTATS_GROUPS as GROUPS  # the table's order; Total follows

REPORT_NAME = "Quade_cycle_report.csv"
PROGRAM = "Quade-cycle " + QUADE_VERSION.split()[-1]  # (no date: the file can be compared whole)
READS = ("R1", "R2")
A, C, G, T, N, QUAL_SUM, Q20, Q30 = range(8)  # a cycle's counters (stages.CSTATS_COUNTERS)
CYCLE_COLUMNS = ("group", "read", "cycle", "reads", "A", "C", "G", "T", "N", "other", "percent_gc", "mean_quality", "q20", "q30",
                 "percent_q20", "percent_q30")
LAST_LENGTH = ">=1024"  # the label of the last length bin


def _ints(a):
    """nested lists of Python integers (sums beyond 2^63 stay exact)"""
    if hasattr(a, "tolist"):
        a = a.tolist()
    return [_ints(x) for x in a] if isinstance(a, (list, tuple)) else int(a)


def _with_total(per_group):
    """[group][read][...] -> the same with Total = the sum of the groups appended"""
    def add(x, y):
        return [add(p, q) for p, q in zip(x, y)] if isinstance(x, list) else x + y
    total = per_group[0]
    for g in per_group[1:]:
        total = add(total, g)
    return per_group + [total]


def cycle_rows(cycle, length):
    """One (group, read): cycle[1024][8], length[1025] -> the rows' values behind (group, read), for the cycles up to the last one
    that a read has"""
    rows, reads = [], sum(length)
    for c in range(len(cycle)):
        reads -= length[c]  # reads with L > c
        if reads <= 0:
            break
        k = cycle[c]
        other = reads - k[A] - k[C] - k[G] - k[T] - k[N]
        rows.append([str(c + 1), str(reads), str(k[A]), str(k[C]), str(k[G]), str(k[T]), str(k[N]), str(other),
                     ratio(k[G] + k[C], reads, 100), ratio(k[QUAL_SUM], reads), str(k[Q20]), str(k[Q30]),
                     ratio(k[Q20], reads, 100), ratio(k[Q30], reads, 100)])
    return rows


def report_lines(table):
    """The file's lines.  table: hip_backend.cstats_views' dict -- cycle[3][2][1024][8], len[3][2][1025], meanq[3][2][94],
    gc[3][2][101], groups in GROUPS' order."""
    cycle, length, meanq, gc = (_with_total(_ints(table[k])) for k in ("cycle", "len", "meanq", "gc"))
    assert len(cycle) == len(GROUPS) + 1 and all(len(x) == 2 for x in cycle), "the table holds 3 groups of 2 reads"
    names = GROUPS + ("Total",)
    lines = ["Program " + PROGRAM, ""]
    long_reads = sum(length[-1][r][-1] for r in range(2))
    if long_reads:
        lines += ["Reads of 1024 bases or more\t%d\t(cycles from 1025 on are not counted per cycle)" % long_reads, ""]
    lines.append("\t".join(CYCLE_COLUMNS))
    for g, name in enumerate(names):
        for r, read in enumerate(READS):
            lines += ["\t".join([name, read] + row) for row in cycle_rows(cycle[g][r], length[g][r])]
    for title, column, bins, label in (("Read lengths", "length", length, lambda i, n: LAST_LENGTH if i == n - 1 else str(i)),
                                       ("Per-read mean quality", "mean_quality", meanq, lambda i, n: str(i)),
                                       ("Per-read GC percent", "percent_gc", gc, lambda i, n: str(i))):
        lines += ["", title, "\t".join(("group", "read", column, "reads"))]
        for g, name in enumerate(names):
            for r, read in enumerate(READS):
                h = bins[g][r]
                lines += ["\t".join((name, read, label(i, len(h)), str(v))) for i, v in enumerate(h) if v]
    return lines


def write_report(path, table):
    write_lines(path, report_lines(table))
