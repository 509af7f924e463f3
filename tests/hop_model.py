"""The semantics of the index-hopping matrix, written once for the tests and independent of the product code.

The part lists are two dicts built by first appearance over the K-long barcodes of the sheet, as registered.  The truth is a
collections.Counter over (a, b) of the pairs that the unmodified oracle routes to 0xFFFF: idx = the fused barcode slice the oracle
itself cut, a = the ordinal of idx[:w1].upper() in the first dict or n1, b = that of idx[w1:].upper() in the second or n2; slices
shorter than K count as `short` instead.  The helpers below turn a device table into the same form and state the invariants.
"""
from collections import Counter


def part_lists(barcodes, K, w1):
    """-> (P1, P2, part1, part2): the dicts value -> ordinal, and per sample its two ordinals (-1, -1 off the matrix)"""
    P1, P2, part1, part2 = {}, {}, [], []
    for bc in barcodes:
        if len(bc) != K:
            part1.append(-1)
            part2.append(-1)
            continue
        if bc[:w1] not in P1:
            P1[bc[:w1]] = len(P1)
        if bc[w1:] not in P2:
            P2[bc[w1:]] = len(P2)
        part1.append(P1[bc[:w1]])
        part2.append(P2[bc[w1:]])
    return P1, P2, part1, part2


def model_from_slices(slices, K, w1, P1, P2):
    """(Counter of (a, b), short) over fused index slices (every one of them an Undetermined pair's)"""
    model, short = Counter(), 0
    for s in slices:
        if len(s) < K:
            short += 1
            continue
        a = P1.get(s[:w1].upper(), len(P1))
        b = P2.get(s[w1:].upper(), len(P2))
        model[(a, b)] += 1
    return model, short


def model_from_oracle(codes, idx, K, w1, P1, P2):
    """the same over the pairs of an oracle run whose code is 0xFFFF"""
    return model_from_slices([s for c, s in zip(codes, idx) if int(c) == 0xFFFF], K, w1, P1, P2)


def table_counter(table, n1, n2):
    """a table in qd_hop_read's layout -> (Counter of (a, b) over its non-zero cells, short)"""
    assert len(table) == (n1 + 1) * (n2 + 1) + 1
    out = Counter()
    for a in range(n1 + 1):
        for b in range(n2 + 1):
            c = int(table[a * (n2 + 1) + b])
            if c:
                out[(a, b)] = c
    return out, int(table[-1])


def model_table(model, short, n1, n2):
    """the model in qd_hop_read's layout, a list of ints"""
    t = [0] * ((n1 + 1) * (n2 + 1) + 1)
    for (a, b), c in model.items():
        t[a * (n2 + 1) + b] = c
    t[-1] = short
    return t


def check_table(table, n1, n2, model, short, undetermined, part1, part2):
    """the table equals the model cell by cell, `short` too; sum(table) == UNDETERMINED; every on-sheet cell is 0"""
    got, got_short = table_counter(table, n1, n2)
    assert got == model, (sorted((model - got).items())[:5], sorted((got - model).items())[:5])
    assert got_short == short, (got_short, short)
    assert sum(int(x) for x in table) == int(undetermined), (sum(int(x) for x in table), int(undetermined))
    for a, b in zip(part1, part2):
        assert a < 0 or got[(a, b)] == 0, (a, b, got[(a, b)])
