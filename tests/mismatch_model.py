"""The semantics of mismatch-tolerant matching, written once for the tests and independent of the product code.

Budgets m1 (index read 1's part of the fused barcode, [0, w1)) and m2 (index read 2's part, [w1, K)).  A key (the pair's
fused slice, upper-cased) that matches no barcode exactly goes to the barcode of length K within m1 substitutions on the
first part and m2 on the second; bytes are compared as they are (N is an ordinary symbol).  A key shorter than K, and a
barcode whose length is not K, match exactly only.  Two K-long barcodes collide when their distances are <= 2*m1 and <= 2*m2.

tolerant_sampleset(qo, ...) returns a subclass of the oracle's SampleSet whose INDEX_TO_SAMPLE resolves exactly first and
then by this rule, so that the unmodified oracle (qo.demux_reads, qo.run_quade) produces tolerant codes, outputs and reports
when the tests monkeypatch qo.SampleSet with it.
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

