"""The semantics of the unknown-barcode tally, written once for the tests and independent of the product code.

The truth is a collections.Counter over idx[i].upper() of the pairs that the unmodified oracle routes to 0xFFFF (idx = the fused
barcode slice the oracle itself cut); slices shorter than K count as `short` instead.  The helpers below turn a device table
into the same form, state the accounting conditions of the feature, and find a row's nearest sample by brute force.
"""
from collections import Counter

import numpy as np


def model_from_oracle(codes, idx, K):
    """(Counter of upper-cased K-long keys, short) over the pairs with code 0xFFFF"""
    model, short = Counter(), 0
    for c, s in zip(codes, idx):
        if int(c) != 0xFFFF:
            continue
        if len(s) < K:
            short += 1
        else:
            model[s.upper()] += 1
    return model, short


def table_counter(keys, counts):
    out = Counter()
    if len(counts) == 0:
        return out
    keys = np.asarray(keys, dtype=np.uint8).reshape(len(counts), -1)
    for k, c in zip(keys, counts):
        key = bytes(k).decode("latin-1")
        assert key not in out, "a key twice in one table: %r" % key
        out[key] = int(c)
    return out


def check_invariant(table, stats, undetermined):
    """sum(counts) + short + dropped == UNDETERMINED, and the totals agree with the table"""
    tallied, short, dropped, distinct = (int(x) for x in stats)
    assert tallied == sum(table.values())
    assert distinct == len(table)
    assert tallied + short + dropped == int(undetermined), (tallied, short, dropped, int(undetermined))


def check_exact(table, stats, model, short, undetermined):
    """dropped == 0: the table is the exact multiset"""
    check_invariant(table, stats, undetermined)
    assert int(stats[2]) == 0, "dropped = %d" % int(stats[2])
    assert int(stats[1]) == short, (int(stats[1]), short)
    assert table == model, (sorted((model - table).items())[:5], sorted((table - model).items())[:5])


def check_lossy(table, stats, model, short, undetermined):
    """dropped > 0: every entry is exact, no absent key has more than `dropped` occurrences"""
    check_invariant(table, stats, undetermined)
    dropped = int(stats[2])
    assert dropped > 0
    assert int(stats[1]) == short
    for key, c in table.items():
        assert model[key] == c, (key, c, model[key])
    worst = max([c for key, c in model.items() if key not in table] or [0])
    assert worst <= dropped, (worst, dropped)
    assert sum(c for key, c in model.items() if key not in table) == dropped


def nearest_brute(key, samples, w1):
    """samples: (name, barcode) in ordinal order.  (name, d1, d2) of the sample of len(key) with the smallest d1 + d2, lowest
    ordinal on a tie; None when no barcode has that length."""
    best = None
    for name, bc in samples:
        bc = bc.upper()
        if len(bc) != len(key):
            continue
        d1 = sum(1 for a, b in zip(key[:w1], bc[:w1]) if a != b)
        d2 = sum(1 for a, b in zip(key[w1:], bc[w1:]) if a != b)
        if best is None or d1 + d2 < best[1] + best[2]:
            best = (name, d1, d2)
    return best


def report_order(model):
    """[(key, count)]: count descending, then key bytes ascending"""
    return sorted(model.items(), key=lambda kv: (-kv[1], kv[0].encode("latin-1")))


def parse_report(path):
    """-> (head dict, column names, rows as lists)"""
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[-1] == "" and lines[4] == ""
    head = dict(ln.split("\t") for ln in lines[:4])
    return head, lines[5].split("\t"), [ln.split("\t") for ln in lines[6:-1]]
