"""What the mismatch and unknown-barcode GPU tests share: the plan shapes, sample sheets and index reads with planted mismatches."""
import numpy as np

from quade_amd import hip_backend as hb
from quade_amd import synth


# shapes: (plan, barcode bases per index read (w1, w2), read length per index read)
SHAPES = {
    "single8": (hb.make_plan(False, 25, (0, 8)), (8, 0), 8),
    "dual8": (synth.config_plan("cfg3"), (8, 8), 8),
    "wide10": (synth.config_plan("wide10"), (10, 10), 10),
    "kit6": (synth.config_plan("kit6"), (6, 6), 6),
    "kit8u9": (synth.config_plan("kit8u9"), (8, 8), 17),
}


def make_reads(shape, bcs, n, m1, m2, seed, short_frac=0.0):
    """Index reads (lists of bytes per stream: sequences, qualities) of n pairs over the sample sheet bcs: exact barcodes, one
    or two substitutions (by another symbol of ACGTN) in either part, uniform reads, lower case, low-quality barcode
    positions, and (short_frac) reads cut inside their barcode slice."""
    plan, (w1, w2), L = SHAPES[shape]
    rng = np.random.default_rng(seed)
    K = w1 + w2
    bc = np.array([np.frombuffer(b.encode(), np.uint8) for b in bcs], dtype=np.uint8).reshape(len(bcs), K)
    key = bc[rng.integers(0, len(bcs), n)].copy()
    kind = rng.integers(0, 100, n)
    acgtn = np.frombuffer(b"ACGTN", np.uint8)

    def substitute(rows, lo, hi):
        pos = rng.integers(lo, hi, rows.size)
        new = acgtn[rng.integers(0, 5, rows.size)]
        same = new == key[rows, pos]
        new[same] = np.where(key[rows, pos][same] == ord("N"), ord("A"), ord("N"))
        key[rows, pos] = new

    parts = [(0, w1)] + ([(w1, K)] if w2 else [])
    one = np.flatnonzero((kind >= 40) & (kind < 70))
    side = rng.integers(0, len(parts), one.size)
    for i, p in enumerate(parts):
        substitute(one[side == i], *p)
    two = np.flatnonzero((kind >= 70) & (kind < 85))
    substitute(two, 0, K)
    substitute(two, 0, K)
    rnd = np.flatnonzero(kind >= 92)
    key[rnd] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (rnd.size, K))]
    lc = np.flatnonzero(rng.integers(0, 100, n) < 5)
    key[lc, rng.integers(0, K, lc.size)] |= 0x20
    q = (rng.integers(30, 41, (n, K)) + 33).astype(np.uint8)
    bad = np.flatnonzero(rng.integers(0, 100, n) < 20)
    q[bad, rng.integers(0, K, bad.size)] = (rng.integers(2, 25, bad.size) + 33).astype(np.uint8)
    streams = []
    ns = 2 if plan.dual else 1
    cut = rng.integers(0, 100, n) < int(100 * short_frac)
    for k in range(ns):
        iw = w1 if k == 0 else w2
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L))]
        seq[:, :iw] = key[:, k * w1:k * w1 + iw]
        qual = np.full((n, L), ord("I"), np.uint8)
        qual[:, :iw] = q[:, k * w1:k * w1 + iw]
        lens = np.where(cut & (rng.integers(0, 2, n) == k), rng.integers(1, iw, n), L)
        streams.append(([bytes(seq[r, :lens[r]]) for r in range(n)], [bytes(qual[r, :lens[r]]) for r in range(n)]))
    return streams


def rows_on_device(torch, layout, streams):
    seq, qual, lens, full = [], [], [], True
    for k, (s, q) in enumerate(streams):
        sr, qr, lr, f = hb.pack_index_reads(layout, k, s, q)
        full = full and f
        seq.append(torch.from_numpy(sr).cuda())
        qual.append(torch.from_numpy(qr).cuda())
        lens.append(torch.from_numpy(lr).cuda())
    return seq, qual, lens, full


def sheet(shape, S, m1, m2, seed=1):
    _, (w1, w2), _ = SHAPES[shape]
    return synth.make_far_barcodes(S, w1, w2, m1, m2, seed=seed)
