# -*- coding: utf-8 -*-
"""
Quade_index_hopping_report.csv: the index pairs of the Undetermined reads against the sheet ([output] index_hopping_report,
conf.HOPPING_HELP has the definition).  The reference has no counterpart; bcl2fastq and BCL Convert call the same figures "Index
Hopping Counts".  The table comes from the device (include/quade_hip.h, qd_hop_*) and the part lists from qd_hop_index; everything
here is host work on that table: sums, the order of the unexpected combinations and the text.  Tab-separated, integer arithmetic,
no date: two runs of one input give the same file.
"""
from __future__ import annotations

import numpy as np

REPORT_NAME = "Quade_index_hopping_report.csv"
MAX_ROWS = 10000  # unexpected combinations listed; the rest is summed in the `other_cells` line
LOWER_BOUND_LINE = "Exact per-part matching: rates are lower bounds"
COMBINATION_COLUMNS = ("index1_seq", "index2_seq", "count", "per_100000_of_undetermined", "index1_samples", "index2_samples")
SAMPLE_COLUMNS = ("sample", "index1_seq", "index2_seq", "assigned", "index1_with_other_index2", "index2_with_other_index1",
                  "index1_only", "index2_only")


def report_lines(table, n1, n2, part1, part2, samples, w1, budgets, pairs, sample_assigned):
    """The file's lines.  table: uint64[(n1+1)*(n2+1)+1] (qd_hop_read's layout, summed over contexts and ranks); part1 / part2 /
    n1 / n2: what hip_backend.hop_index gave for the sheet; samples: (name, barcode) in ordinal order; w1: bases of index 1's part;
    budgets: (index1_mismatches, index2_mismatches); pairs: the run's total; sample_assigned: pass + fail per sample."""
    table = np.asarray(table, dtype=np.uint64).reshape(-1)
    assert table.size == (n1 + 1) * (n2 + 1) + 1, "an index-hopping table of %d values for %d x %d parts" % (table.size, n1, n2)
    cells = table[:-1].reshape(n1 + 1, n2 + 1)
    short = int(table[-1])
    on = [s for s in range(len(samples)) if part1[s] >= 0]
    seq1, seq2 = [None] * n1, [None] * n2  # a part's bases and the samples that carry it, from the part lists alone
    names1, names2 = [[] for _ in range(n1)], [[] for _ in range(n2)]
    for s in on:
        name, bc = samples[s]
        seq1[part1[s]], seq2[part2[s]] = bc[:w1], bc[w1:]
        names1[part1[s]].append(name)
        names2[part2[s]].append(name)
    inner = cells[:n1, :n2]
    both = int(inner.sum(dtype=np.uint64))
    only1 = int(cells[:n1, n2].sum(dtype=np.uint64))
    only2 = int(cells[n1, :n2].sum(dtype=np.uint64))
    neither = int(cells[n1, n2])
    undetermined = both + only1 + only2 + neither + short
    assigned = sum(int(x) for x in sample_assigned)
    K = max([len(bc) for s, (_, bc) in enumerate(samples) if part1[s] >= 0] or [0])
    lines = ["index1 width\t{}".format(w1), "index2 width\t{}".format(K - w1 if K else 0),
             "distinct index1\t{}".format(n1), "distinct index2\t{}".format(n2),
             "samples off the matrix\t{}".format(len(samples) - len(on)),
             "mismatch budgets\t{},{}".format(int(budgets[0]), int(budgets[1]))]
    if budgets[0] > 0 or budgets[1] > 0:
        lines.append(LOWER_BOUND_LINE)
    lines += ["pairs\t{}".format(int(pairs)), "assigned\t{}".format(assigned), "undetermined\t{}".format(undetermined),
              "short index slice\t{}".format(short), "both indexes known\t{}".format(both), "index1 known only\t{}".format(only1),
              "index2 known only\t{}".format(only2), "neither known\t{}".format(neither),
              "unexpected_per_100000\t{}".format(both * 100000 // (assigned + both) if assigned + both else 0), ""]
    # the unexpected combinations: count descending, then a, then b (flat order is (a, b) ascending; the sort is stable)
    lines.append("\t".join(COMBINATION_COLUMNS))
    flat = np.flatnonzero(inner.reshape(-1))
    counts = inner.reshape(-1)[flat]
    order = np.argsort(-counts.astype(np.int64), kind="stable")
    for i in order[:MAX_ROWS]:
        a, b = divmod(int(flat[i]), n2)
        c = int(counts[i])
        lines.append("\t".join([seq1[a], seq2[b], str(c), str(c * 100000 // undetermined), ",".join(names1[a]), ",".join(names2[b])]))
    if order.size > MAX_ROWS:
        rest = counts[order[MAX_ROWS:]]
        lines.append("other_cells\t{}\t{}".format(rest.size, int(rest.sum(dtype=np.uint64))))
    lines.append("")
    # the on-matrix samples in sheet order; samples that share a part share its sums
    lines.append("\t".join(SAMPLE_COLUMNS))
    row_sum = inner.sum(axis=1, dtype=np.uint64) if n2 else np.zeros(n1, dtype=np.uint64)
    col_sum = inner.sum(axis=0, dtype=np.uint64) if n1 else np.zeros(n2, dtype=np.uint64)
    for s in on:
        a, b = int(part1[s]), int(part2[s])
        name, bc = samples[s]
        lines.append("\t".join([name, bc[:w1], bc[w1:], str(int(sample_assigned[s])), str(int(row_sum[a])), str(int(col_sum[b])),
                                str(int(cells[a, n2])), str(int(cells[n1, b]))]))
    return lines


def write_report(path, *args, **kw):
    with open(path, "w") as fh:
        fh.write("\n".join(report_lines(*args, **kw)) + "\n")
