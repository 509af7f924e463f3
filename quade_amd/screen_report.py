# -*- coding: utf-8 -*-
"""
Quade_screen_report.csv: what the k-mer screen ([screen] section, conf.SCREEN_HELP) found of the reference -- the parameters with
the reference's file name, records, bases and distinct k-mers, then for every destination (<sample>_pass, <sample>_fail,
Undetermined) and Total the eight counters of the device table (include/quade_hip.h, qd_screen_*), the percentages of pairs
matched and of k-mers hit, and the pairs the stage dropped.  The reference has no counterpart.  Tab-separated, integer arithmetic
only and no date, so that files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, write_lines
from .stages import SCREEN_COUNTERS as COUNTERS  # a destination's row of the table

REPORT_NAME = "Quade_screen_report.csv"
PROGRAM = "Quade-screen " + QUADE_VERSION.split()[-1]
COLUMNS = ("destination",) + COUNTERS + ("matched_pct", "hit_kmer_pct", "dropped_pairs")
REFERENCE = ("name", "records", "bases", "kmers")  # the keys of params["reference"]
PARAMS = ("kmer", "min_hits", "action")
PAIRS, MATCHED, R1_HIT, R2_HIT, KMERS, HIT_KMERS, BASES_IN, BASES_MATCHED = range(8)


def _row(name, c, drop):
    c = [int(x) for x in c]
    return "\t".join([name] + [str(x) for x in c] + [ratio(c[MATCHED], c[PAIRS], 100), ratio(c[HIT_KMERS], c[KMERS], 100),
                                                     str(c[MATCHED] if drop else 0)])


def report_lines(table, samples, params):
    """The file's lines.  table: [2 * S + 1][8] (qd_screen_read); samples: the names in sheet order; params: a mapping with PARAMS
    and "reference", a mapping with REFERENCE (what conf.screen_params gives)."""
    rows = [[int(x) for x in row] for row in table]
    assert len(rows) == 2 * len(samples) + 1 and all(len(r) == len(COUNTERS) for r in rows), "one row of 8 per destination"
    ref = params.get("reference") or {}
    lines = ["Program " + PROGRAM, ""]
    lines += ["reference\t%s" % ref.get("name", "")]
    lines += ["reference_%s\t%s" % (k, ref.get(k, "")) for k in REFERENCE[1:]]
    lines += ["%s\t%s" % (k, params[k]) for k in PARAMS]
    lines += ["", "\t".join(COLUMNS)]
    drop = params["action"] in ("drop", 1)
    names = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined"]
    for name, c in zip(names, rows):
        lines.append(_row(name, c, drop))
    lines.append(_row("Total", [sum(col) for col in zip(*rows)], drop))
    return lines


def write_report(path, table, samples, params):
    write_lines(path, report_lines(table, samples, params))
