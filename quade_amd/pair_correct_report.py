# -*- coding: utf-8 -*-
"""
Quade_pair_correct_report.csv: what the overlap base correction of the read pairs ([trim] pair_correct, conf.CORRECT_HELP) wrote --
the parameters, then for R1, R2 and both the reads, the reads and bases corrected and their shares (corrected bases per overlap base
of the read), then the pair counters of the device table (include/quade_hip.h, qd_paircorrect_*) with the mismatch rate per 100 000
overlap bases before and after the correction.  The reference has no counterpart.  Integer arithmetic only and no date, so that
files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, read_report_lines, write_lines
from .stages import PAIRCORRECT_COUNTERS as COUNTERS  # the table
from .stages import PAIRCORRECT_VALUES as VALUES

REPORT_NAME = "Quade_pair_correct_report.csv"
PROGRAM = "Quade-pair-correct " + QUADE_VERSION.split()[-1]
COLUMNS = ("read", "reads", "corrected_reads", "corrected_bases", "overlap_bases", "percent_corrected_reads", "percent_corrected_bases")
PARAMS = ("pair_correct_good_quality", "pair_correct_bad_quality")
KEYS = ("good_quality", "bad_quality")  # PARAMS as Engine.paircorrect_set's keywords
R1_READS, R1_BASES, R2_READS, R2_BASES, PAIRS, OVERLAPPED, OVERLAP_BASES, MISMATCHES, UNRESOLVED, CORRECTED_PAIRS = range(10)


def _shares(c):
    reads, corrected_reads, corrected_bases, overlap_bases = c
    return [ratio(corrected_reads, reads, 100), ratio(corrected_bases, overlap_bases, 100)]


def report_lines(table, params):
    """The file's lines.  table: the 10 values of qd_paircorrect_read; params: a mapping with KEYS."""
    t = [int(x) for x in table]
    assert len(t) == VALUES == len(COUNTERS), "the table holds 10 values"
    rows = [[t[PAIRS], t[R1_READS], t[R1_BASES], t[OVERLAP_BASES]], [t[PAIRS], t[R2_READS], t[R2_BASES], t[OVERLAP_BASES]]]
    lines = read_report_lines(PROGRAM, ["pair_correct\tTrue"] + ["%s\t%s" % (name, params[key]) for name, key in zip(PARAMS, KEYS)],
                              COLUMNS, rows, _shares)
    corrected = t[R1_BASES] + t[R2_BASES]
    lines.append("")
    lines += ["pairs\t%d" % t[PAIRS],
              "overlapped_pairs\t%d\t%s" % (t[OVERLAPPED], ratio(t[OVERLAPPED], t[PAIRS], 100)),
              "overlap_bases\t%d" % t[OVERLAP_BASES],
              "mismatches\t%d" % t[MISMATCHES],
              "corrected\t%d\t%s" % (corrected, ratio(corrected, t[MISMATCHES], 100)),
              "unresolved\t%d\t%s" % (t[UNRESOLVED], ratio(t[UNRESOLVED], t[MISMATCHES], 100)),
              "corrected_pairs\t%d\t%s" % (t[CORRECTED_PAIRS], ratio(t[CORRECTED_PAIRS], t[OVERLAPPED], 100)),
              "mismatches_per_100000_overlap_bases_before\t%s" % ratio(t[MISMATCHES], t[OVERLAP_BASES], 100000),
              "mismatches_per_100000_overlap_bases_after\t%s" % ratio(t[UNRESOLVED], t[OVERLAP_BASES], 100000)]
    return lines


def write_report(path, table, params):
    write_lines(path, report_lines(table, params))
