# -*- coding: utf-8 -*-
"""
The reference of the k-mer screen ([screen] section, conf.SCREEN_HELP): a FASTA file, plain or gzip, read on the host and turned
into the sorted distinct canonical words of its k-mers with numpy -- what Engine.screen_set takes.  Every rank and chunk worker
builds the same array from the same file, so nothing about the reference is exchanged.  The user supplies the FASTA: no genome
is shipped with the package.  Nothing here touches libquade_hip.so.
"""
from __future__ import annotations

import gzip
from collections import namedtuple

import numpy as np

MIN_KMER, MAX_KMER = 15, 32
MAX_KMERS = 1 << 22       # QD_SCREEN_MAX_KMERS
LDS_MAX_KMERS = 6144      # QD_SCREEN_LDS_MAX_KMERS: up to here the kernel keeps the hash table in LDS

# kmers: uint64, ascending, distinct; records: the FASTA's records; bases: their sequence bytes, valid or not
Reference = namedtuple("Reference", "kmers records bases")


def read_fasta(path):
    """the file's bytes, a gzip file (by its magic number, whatever its name) decompressed"""
    with open(path, "rb") as fh:
        data = fh.read()
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data


def records_of(data):
    """FASTA bytes -> the records' sequences, line ends and blanks removed.  A line starting with '>' begins a record; sequence in
    front of the first such line is a record of its own."""
    out, cur = [], None
    for line in data.split(b"\n"):
        line = line.strip()
        if line[:1] == b">":
            if cur is not None:
                out.append(b"".join(cur))
            cur = []
        elif line:
            if cur is None:
                cur = []
            cur.append(line.replace(b" ", b"").replace(b"\t", b""))
    if cur is not None:
        out.append(b"".join(cur))
    return out


def canonical_words(seq, k):
    """One sequence (bytes or a uint8 array) -> the canonical word of every position [0, len - k] and whether its k-mer exists:
    (uint64[n], bool[n])."""
    s = np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)
    n = s.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    u = s & 0xDF
    bad = np.concatenate([[0], np.cumsum(~np.isin(u, np.frombuffer(b"ACGT", dtype=np.uint8)))])
    exists = bad[k:] == bad[:-k]
    code = ((u >> 1) & 3).astype(np.uint64)
    w, rc = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    two = np.uint64(2)
    for i in range(k):
        w = (w << two) | code[i:i + n]
        rc = (rc << two) | (code[k - 1 - i:k - 1 - i + n] ^ two)
    return np.minimum(w, rc), exists


def reference_kmers(data, k):
    """FASTA bytes -> Reference: the sorted distinct canonical words of every k-mer of every record.  Records are linear and k-mers
    never span two of them; lower case counts; any byte but A, C, G, T breaks k-mers."""
    assert MIN_KMER <= k <= MAX_KMER, "kmer: 15 to 32"
    recs = records_of(data)
    # one pass over all records: a '>' between two of them breaks every k-mer that would span them
    words, exists = canonical_words(b">".join(recs), k)
    return Reference(np.unique(words[exists]), len(recs), sum(len(r) for r in recs))
