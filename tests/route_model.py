"""A plain Python model of the stages that turn a batch's record tables into output bytes (quade_amd/csrc/quade_text.hip:
pack_rows, dest_lens, the sort by destination, scan_gathered, dest_bounds, the host's layout of the output text, format_records,
member_offsets / member_copy), written to be read against the reference: the tag and the record are src/FastqWriter.py:61-69, the
slices are src/Quade.py:217-218, 246-247 (Python slices of the index reads, raw case), the routing is src/Sample.py:74-91.

Everything is loops over bytes objects and lists of ints: no numpy, nothing clever.  A read is (name, seq, qual), an index read is
its sequence (rows: (seq, qual)); a plan is anything with the fields of qd_plan, a layout anything with the fields of qd_layout."""

GUARD = 0xEE  # QD_DEV_GUARD_BYTE: what the stage entries leave in bytes that no kernel owns
UNDETERMINED = 0xFFFF
NONE = 0xFFFFFFFF


# ---- tables -> reads ---------------------------------------------------------------------------------------------------------
def read_of(text, rec):
    """(name, seq, qual) of a record table row (head, name_off, name_len, seq, seq_len, qual: qd_dev_fastq_scan's layout)"""
    _head, name_off, name_len, seq, seq_len, qual = [int(v) for v in rec]
    return text[name_off:name_off + name_len], text[seq:seq + seq_len], text[qual:qual + seq_len]


def parse_record(record):
    """(name, seq, qual) of the four lines of a kept record, as the reference's reader hands them on: a '\\r' before the newline is
    not part of a line, the name is the header without its first byte, cut at the first blank"""
    head, seq, _plus, qual = [ln[:-1] if ln.endswith(b"\r") else ln for ln in record.split(b"\n")[:4]]
    fields = head[1:].split()
    return (fields[0] if fields else b""), seq, qual


# ---- index rows (pack_rows; the operands of src/Quade.py:217-218) ------------------------------------------------------------------
def rows(layout, k, reads):
    """reads: [(seq, qual)] of index stream k -> (seq rows, qual rows, len row): lists of bytes / ints"""
    so, sw, ss = layout.seq_off[k], layout.seq_width[k], layout.seq_stride[k]
    qo, qw, qs = layout.qual_off[k], layout.qual_width[k], layout.qual_stride[k]
    seq_rows, qual_rows, lens = [], [], []
    for seq, qual in reads:
        s = seq[so:so + sw]
        q = qual[qo:qo + qw]
        seq_rows.append(s + b"\x00" * (ss - len(s)))
        qual_rows.append(q + b"\xff" * (qs - len(q)))
        lens.append(min(255, len(seq)))
    return seq_rows, qual_rows, lens


def short_set(layout, streams):
    """streams: the reads of every index stream -> the pairs with a read shorter than its window (quade_text.h: qd_pack_args)"""
    out = set()
    for k in range(layout.n_streams):
        for j, (seq, _qual) in enumerate(streams[k]):
            if len(seq) < layout.seq_off[k] + layout.seq_width[k]:
                out.add(j)
    return out


# ---- one record ----------------------------------------------------------------------------------------------------------------
def windows(plan):
    """[(idx_start, idx_end, mol_start, mol_end)] of the plan's index streams"""
    w = [(plan.idx1_start, plan.idx1_end, plan.mol1_start, plan.mol1_end)]
    if plan.dual:
        w.append((plan.idx2_start, plan.idx2_end, plan.mol2_start, plan.mol2_end))
    return w


def tag(plan, index_seqs):
    """':IDX' or ':IDX:MOL' (src/FastqWriter.py:61-66): the slices of the index reads as read, ':MOL' only when it is not empty"""
    idx, mol = b"", b""
    for (i0, i1, m0, m1), seq in zip(windows(plan), index_seqs):
        idx += seq[i0:i1]
        mol += seq[m0:m1]
    return b":" + idx + (b":" + mol if mol else b"")


def record(read, the_tag):
    name, seq, qual = read
    return b"@" + name + the_tag + b"\n" + seq + b"\n+\n" + qual + b"\n"


def destination(code, n_samples):
    return 2 * n_samples if code == UNDETERMINED or code >= 2 * n_samples else code


def enabled(d, n_samples, flags):
    write_pass, write_fail, write_undetermined = flags
    if d == 2 * n_samples:
        return bool(write_undetermined)
    return bool(write_fail) if d & 1 else bool(write_pass)


# ---- a batch -------------------------------------------------------------------------------------------------------------------
def route(plan, n_samples, flags, reads1, reads2, index_seqs, codes, drop=None, out_cap=None):
    """reads1 / reads2: [(name, seq, qual)] of the pairs, index_seqs: [[I1 sequence of every pair], [I2 ...]], codes: routing codes.
    -> dict: every table qd_dev_route_format returns (lists of ints), "text": {(d, k): the destination's R1 (k = 0) / R2 text},
    "used", and "out": the whole buffer of out_cap bytes (default: used) with GUARD wherever no record lies."""
    n, nd = len(codes), 2 * n_samples + 1
    dest, recs1, recs2 = [], [], []
    for j in range(n):
        d = destination(int(codes[j]), n_samples)
        dest.append(d)
        if enabled(d, n_samples, flags) and not (drop is not None and drop[j]):
            t = tag(plan, [s[j] for s in index_seqs])
            recs1.append(record(reads1[j], t))
            recs2.append(record(reads2[j], t))
        else:  # no room in any output
            recs1.append(b"")
            recs2.append(b"")
    perm = sorted(range(n), key=lambda j: dest[j])  # (sorted is stable)
    sdest = [dest[j] for j in perm]
    g1, g2 = [0], [0]
    for j in perm:
        g1.append(g1[-1] + len(recs1[j]))
        g2.append(g2[-1] + len(recs2[j]))
    first, g1_first, g2_first = [NONE] * nd, [NONE] * nd, [NONE] * nd
    for k in range(n - 1, -1, -1):
        first[sdest[k]], g1_first[sdest[k]], g2_first[sdest[k]] = k, g1[k], g2[k]
    # a destination's pairs are consecutive in sorted order: its text is their records one behind the other
    parts = {(d, k): [] for d in range(nd) for k in (0, 1)}
    for j in perm:
        parts[(dest[j], 0)].append(recs1[j])
        parts[(dest[j], 1)].append(recs2[j])
    text = {key: b"".join(v) for key, v in parts.items()}
    # the buffer: every destination's R1 region in ascending d, then every R2 region, each non-empty one on a multiple of 16
    at, where, base = 0, {}, ([0] * nd, [0] * nd)
    for k in (0, 1):
        g, g_first = (g1, g1_first) if k == 0 else (g2, g2_first)
        start = [g[n]] * (nd + 1)  # G where d's text starts: at its first pair, else where the next destination with pairs starts
        for d in range(nd - 1, -1, -1):
            start[d] = g_first[d] if first[d] != NONE else start[d + 1]
        for d in range(nd):
            base[k][d] = at - start[d]
            if text[(d, k)]:
                where[(d, k)] = at
                at = (at + len(text[(d, k)]) + 15) // 16 * 16
    used = at
    out = bytearray([GUARD]) * (used if out_cap is None else out_cap)
    for (d, k), a in where.items():
        out[a:a + len(text[(d, k)])] = text[(d, k)]
    return {"dest": dest, "len1": [len(r) for r in recs1], "len2": [len(r) for r in recs2], "perm": perm, "sdest": sdest, "g1": g1, "g2": g2,
            "first": first, "g1_first": g1_first, "g2_first": g2_first, "base1": base[0], "base2": base[1], "text": text, "where": where,
            "used": used, "out": bytes(out)}


# ---- members -------------------------------------------------------------------------------------------------------------------
def pack_members(slots, stride, lens, packed_cap):
    """slots: bytes, member i = slots[i * stride : i * stride + lens[i]] -> (offsets[n + 1], packed bytes of packed_cap, GUARD behind)"""
    offsets, members = [0], []
    for i, L in enumerate(lens):
        members.append(slots[i * stride:i * stride + L])
        offsets.append(offsets[-1] + L)
    return offsets, b"".join(members) + bytes([GUARD]) * (packed_cap - offsets[-1])
