# -*- coding: utf-8 -*-
"""
Quade_adapter_report.csv: which known adapters start where in the RAW insert reads ([output] adapter_report, conf.ADAPTER_HELP) --
the probes in force with their aliases, the user sequences left off, for R1 and R2 the reads that hold each probe and any of them
with their share per 100000, the most frequent probe, the cumulative content by position (the curve FastQC draws) and the counts
per destination (<sample>_pass, <sample>_fail, Undetermined) and Total.  The reference has no counterpart.  The counters come
from the device (include/quade_hip.h, qd_adapters_*, which defines every one of them).  Tab-separated, integer arithmetic only and
no date, so that two runs of one input give the same file and files can be compared whole.
"""
from __future__ import annotations

from . import QUADE_VERSION
from .quality_report import ratio, write_lines
from .stages import ADAPTER_BINS, ADAPTER_COLUMNS, ADAPTER_PROBES

REPORT_NAME = "Quade_adapter_report.csv"
PROGRAM = "Quade-adapters " + QUADE_VERSION.split()[-1]
READS = ("R1", "R2")
ANY = ADAPTER_PROBES  # the histogram's last column; a destination's columns are reads, the slots, any
LAST_POSITION = ">=1024"  # the label of the last bin
PER = 100000


def _ints(a):
    """nested lists of Python integers (sums beyond 2^63 stay exact)"""
    if hasattr(a, "tolist"):
        a = a.tolist()
    return [_ints(x) for x in a] if isinstance(a, (list, tuple)) else int(a)


def top_adapter(names, counts):
    """the probe with the highest count, ties by slot order; "none" when every count is 0"""
    best = max(range(len(names)), key=lambda a: (counts[a], -a)) if names else None
    return names[best] if best is not None and counts[best] else "none"


def report_lines(table, samples, params):
    """The file's lines.  table: hip_backend.adapters_views' dict -- hist[2][17][1025], dest[2S+1][2][18]; samples: the names in
    sheet order; params: what conf.adapter_params gives -- probes [(name, probe)] in slot order, aliases [(name, of)], left_off
    [(name, reason)]."""
    hist, dest = _ints(table["hist"]), _ints(table["dest"])
    probes = list(params["probes"])
    names = [name for name, _ in probes]
    cols = list(range(len(probes))) + [ANY]  # the columns in force
    assert len(hist) == 2 and all(len(h) == ADAPTER_COLUMNS and all(len(b) == ADAPTER_BINS for b in h) for h in hist), "hist[2][17][1025]"
    assert len(dest) == 2 * len(samples) + 1 and all(len(d) == 2 and all(len(c) == ADAPTER_COLUMNS + 1 for c in d) for d in dest), \
        "one row of 2 x 18 per destination"
    assert len(probes) <= ADAPTER_PROBES
    lines = ["Program " + PROGRAM, "", "Probes", "slot\tname\tprobe\taliases"]
    for a, (name, probe) in enumerate(probes):
        lines.append("\t".join((str(a), name, probe, ",".join(n for n, of in params.get("aliases", ()) if of == name))))
    lines += ["", "Left off", "name\treason"]
    lines += ["%s\t%s" % (name, reason) for name, reason in params.get("left_off", ())]
    # reads, and reads with each probe: the destinations' sums
    total = [[sum(d[r][c] for d in dest) for c in range(ADAPTER_COLUMNS + 1)] for r in range(2)]
    lines += ["", "Reads with a probe", "read\tprobe\treads\treads_with_probe\tper_%d" % PER]
    for r, read in enumerate(READS):
        for a in cols:
            with_probe = total[r][1 + a]
            lines.append("\t".join((read, "any" if a == ANY else names[a], str(total[r][0]), str(with_probe),
                                    str(with_probe * PER // total[r][0] if total[r][0] else 0))))
    lines += [""] + ["top_adapter_%s\t%s" % (read, top_adapter(names, total[r][1:1 + len(names)])) for r, read in enumerate(READS)]
    lines += ["", "Content by position (cumulative)", "\t".join(["read", "position"] + names + ["any"])]
    for r, read in enumerate(READS):
        seen = [0] * len(cols)
        for b in range(ADAPTER_BINS):
            here = [hist[r][a][b] for a in cols]
            seen = [s + h for s, h in zip(seen, here)]
            if any(here):
                lines.append("\t".join([read, LAST_POSITION if b == ADAPTER_BINS - 1 else str(b)] + [str(s) for s in seen]))
    per_read = ["reads"] + names + ["any", "any_pct"]
    lines += ["", "Per destination", "\t".join(["destination"] + [read + "_" + c for read in READS for c in per_read])]
    rows = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined", "Total"]
    for name, d in zip(rows, dest + [total]):
        cells = [name]
        for r in range(2):
            cells += [str(d[r][0])] + [str(d[r][1 + a]) for a in cols] + [ratio(d[r][1 + ANY], d[r][0], 100)]
        lines.append("\t".join(cells))
    return lines


def write_report(path, table, samples, params):
    write_lines(path, report_lines(table, samples, params))
