"""The semantics of mismatch-tolerant matching, written once for the tests and independent of the product code.

Budgets m1 (index read 1's part of the fused barcode, [0, w1)) and m2 (index read 2's part, [w1, K)).  A key (the pair's
fused slice, upper-cased) that matches no barcode exactly goes to the barcode of length K within m1 substitutions on the
first part and m2 on the second; bytes are compared as they are (N is an ordinary symbol).  A key shorter than K, and a
barcode whose length is not K, match exactly only.  Two K-long barcodes collide when their distances are <= 2*m1 and <= 2*m2.

tolerant_sampleset(qo, ...) returns a subclass of the oracle's SampleSet whose INDEX_TO_SAMPLE resolves exactly first and
then by this rule, so that the unmodified oracle (qo.demux_reads, qo.run_quade) produces tolerant codes, outputs and reports
when the tests monkeypatch qo.SampleSet with it.  codes_for_keys states the same rule once more for whole corpora of keys at
once (numpy, no oracle, no product code); tests/test_host_mismatch.py holds the two to each other.
"""
import numpy as np


def part_distances(a, b, w1):
    """(Hamming distance on [0, w1), on [w1, len)) of two equally long byte strings / str"""
    d1 = sum(1 for x, y in zip(a[:w1], b[:w1]) if x != y)
    d2 = sum(1 for x, y in zip(a[w1:], b[w1:]) if x != y)
    return d1, d2


def collide(a, b, K, w1, m1, m2):
    if len(a) != K or len(b) != K:
        return False
    d1, d2 = part_distances(a, b, w1)
    return d1 <= 2 * m1 and d2 <= 2 * m2


def first_collision(barcodes, K, w1, m1, m2):
    """first colliding ordinal pair (i < j, lexicographic) or None"""
    for i in range(len(barcodes)):
        for j in range(i + 1, len(barcodes)):
            if collide(barcodes[i], barcodes[j], K, w1, m1, m2):
                return i, j
    return None


class TolerantIndex(dict):
    """INDEX_TO_SAMPLE that, once active, also resolves keys within budget (the per-part rule)."""

    def __init__(self, K, w1, m1, m2):
        super().__init__()
        self.K, self.w1, self.m1, self.m2 = K, w1, m1, m2
        self.active = False
        self._mat = None

    def _near(self, key):
        if not self.active or len(key) != self.K or self.m1 + self.m2 == 0:
            return None
        if self._mat is None:  # the K-long barcodes as a matrix (large sheets: one numpy pass per lookup)
            items = [(k, v) for k, v in dict.items(self) if len(k) == self.K]
            self._vals = [v for _, v in items]
            self._mat = np.array([np.frombuffer(k.encode("latin-1"), np.uint8) for k, _ in items],
                                 dtype=np.uint8).reshape(len(items), self.K)
        if not self._vals:
            return None
        diff = self._mat != np.frombuffer(key.encode("latin-1"), np.uint8)[None, :]
        ok = (diff[:, :self.w1].sum(1) <= self.m1) & (diff[:, self.w1:].sum(1) <= self.m2)
        hits = np.flatnonzero(ok)
        assert hits.size <= 1, "colliding sample sheet"
        return self._vals[int(hits[0])] if hits.size else None

    def __contains__(self, key):
        return dict.__contains__(self, key) or self._near(key) is not None

    def __getitem__(self, key):
        if dict.__contains__(self, key):
            return dict.__getitem__(self, key)
        v = self._near(key)
        if v is None:
            raise KeyError(key)
        return v


UNDETERMINED = 0xFFFF


def _part_values(rows):
    """the distinct rows of a byte matrix and every row's place among them (a part of no width: one empty value)"""
    if rows.shape[1] == 0:
        return rows[:1], np.zeros(rows.shape[0], dtype=np.int64)
    values, where = np.unique(rows, axis=0, return_inverse=True)
    return values, where.reshape(-1)


def codes_for_keys(keys, quals, sheet, K, w1, m1, m2, min_qual, chunk_bytes=1 << 25):
    """Routing codes (uint16) of fused keys by the rule above, brute force.  keys: uint8 [n, K], upper-cased; quals: uint8 [n, K],
    the slice's quality bytes (Phred + 33); sheet: the barcodes in ordinal order (those not K long match exactly only, so no K-long
    key reaches them).  2 * sample (+ 1 when a slice quality is below min_qual), 0xFFFF when no K-long barcode is within (m1, m2)
    per part.  An exact hit is taken first; otherwise at most one barcode may qualify (asserted: the collision rule).

    Every key is compared with every K-long barcode: its first part with the distinct first parts of the sheet and its second
    part with the distinct second parts ([n, U, w] byte compares, chunked), and the barcodes -- a grid over those two lists of
    values -- are then counted per key wherever both parts are within budget."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, K)
    quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1, K)
    n = keys.shape[0]
    ids = [i for i, b in enumerate(sheet) if len(b) == K]
    fail = (quals.astype(np.int32) - 33 < min_qual).any(axis=1)
    out = np.full(n, UNDETERMINED, dtype=np.uint16)
    if not ids or n == 0:
        return out
    bc = np.array([np.frombuffer(sheet[i].encode("latin-1"), np.uint8) for i in ids], dtype=np.uint8).reshape(len(ids), K)
    v1, at1 = _part_values(bc[:, :w1])
    v2, at2 = _part_values(bc[:, w1:])
    grid = np.zeros((v1.shape[0], v2.shape[0]), dtype=np.float64)  # ordinal + 1 of the barcode made of (first part, second part)
    assert len({(int(a), int(b)) for a, b in zip(at1, at2)}) == len(ids), "equal barcodes"
    grid[at1, at2] = np.asarray(ids, dtype=np.float64) + 1
    there = (grid > 0).astype(np.float64)
    step = max(1, chunk_bytes // (max(v1.shape[0], v2.shape[0]) * K))
    for a in range(0, n, step):
        k = keys[a:a + step]
        d1 = (k[:, None, :w1] != v1[None, :, :]).sum(axis=2)
        d2 = (k[:, None, w1:] != v2[None, :, :]).sum(axis=2)
        exact = (((d1 == 0).astype(np.float64) @ grid) * (d2 == 0)).sum(axis=1)
        in1, in2 = (d1 <= m1).astype(np.float64), (d2 <= m2)
        hits = ((in1 @ there) * in2).sum(axis=1)
        near = ((in1 @ grid) * in2).sum(axis=1)
        assert (hits[exact == 0] <= 1).all(), "colliding sample sheet"
        found = np.where(exact > 0, exact, np.where(hits == 1, near, 0)).astype(np.int64)
        code = (found - 1) * 2 + fail[a:a + step]
        out[a:a + step] = np.where(found > 0, code, UNDETERMINED).astype(np.uint16)
    return out


def counts_for_codes(codes, S):
    """the ABI's counter vector uint64[2S + 4] of a batch's codes: [total, pass, fail, undetermined, pass_0, fail_0, pass_1, ...]"""
    codes = np.asarray(codes, dtype=np.uint16)
    per = np.bincount(codes[codes != UNDETERMINED].astype(np.int64), minlength=2 * S)
    assert per.size == 2 * S
    out = np.zeros(2 * S + 4, dtype=np.uint64)
    out[0] = codes.size
    out[1] = per[0::2].sum()
    out[2] = per[1::2].sum()
    out[3] = int((codes == UNDETERMINED).sum())
    out[4:] = per
    return out


def tolerant_sampleset(qo, K, w1, m1, m2):
    """SampleSet of the oracle module qo with the tolerant lookup (active from the first FINDER call on)."""

    class TolerantSampleSet(qo.SampleSet):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.INDEX_TO_SAMPLE = TolerantIndex(K, w1, m1, m2)

        def FINDER(self, *a, **kw):
            self.INDEX_TO_SAMPLE.active = True
            return super().FINDER(*a, **kw)

    return TolerantSampleSet

