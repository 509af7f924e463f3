# -*- coding: utf-8 -*-
"""
Quade_pair_trim_report.csv: what the paired-end overlap trimming of the insert reads ([trim] pair_overlap, conf.PAIR_HELP) cut and
the insert sizes it found -- the parameters, then for R1, R2 and both the six counters of the device table (include/quade_hip.h,
qd_pairtrim_*) with the shares of reads and bases cut, the three pair counters, and one line per insert size seen.  The reference
has no counterpart.  Integer arithmetic only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, read_report_lines, write_lines
from .stages import PAIRTRIM_BINS as BINS  # insert sizes 0 .. 1023 and ">=1024"
from .stages import PAIRTRIM_COUNTERS as COUNTERS  # a row per read
from .stages import PAIRTRIM_PAIR_COUNTERS as PAIR_COUNTERS
from .stages import PAIRTRIM_VALUES as VALUES  # the table

REPORT_NAME = "Quade_pair_trim_report.csv"
PROGRAM = "Quade-pair-trim " + QUADE_VERSION.split()[-1]
COLUMNS = ("read",) + COUNTERS + ("percent_overlap_trimmed_reads", "percent_bases_trimmed")
PARAMS = ("pair_min_overlap", "pair_max_mismatches", "pair_max_mismatch_pct", "min_length")
KEYS = ("min_overlap", "max_mismatches", "max_mismatch_pct", "min_length")  # PARAMS as Engine.pairtrim_set's keywords
READS, BASES_IN, BASES_OUT, CUT_READS, CUT_BASES, FLOORED = range(6)
PAIRS, OVERLAPPED, SHORT = range(3)


def _shares(c):
    return [ratio(c[CUT_READS], c[READS], 100), ratio(c[BASES_IN] - c[BASES_OUT], c[BASES_IN], 100)]


def report_lines(table, params):
    """The file's lines.  table: the 1040 values of qd_pairtrim_read; params: a mapping with KEYS."""
    t = [int(x) for x in table]
    assert len(t) == VALUES, "the table holds 1040 values"
    k = len(COUNTERS)
    rows, pairs, hist = [t[:k], t[k:2 * k]], t[2 * k:2 * k + 3], t[2 * k + 3:]
    lines = read_report_lines(PROGRAM, ["pair_overlap\tTrue"] + ["%s\t%s" % (name, params[key]) for name, key in zip(PARAMS, KEYS)],
                              COLUMNS, rows, _shares)
    lines.append("")
    lines += ["%s\t%d\t%s" % (name, v, ratio(v, pairs[PAIRS], 100)) for name, v in zip(PAIR_COUNTERS, pairs)]
    lines += ["", "insert_size\tpairs"]
    lines += ["%d\t%d" % (i, v) for i, v in enumerate(hist[:-1]) if v]
    lines += [">=1024\t%d" % hist[-1], "not_overlapped\t%d" % (pairs[PAIRS] - pairs[OVERLAPPED])]
    return lines


def write_report(path, table, params):
    write_lines(path, report_lines(table, params))
