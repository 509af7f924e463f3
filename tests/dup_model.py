"""The semantics of the duplication tally, written once for the tests and independent of the product code (plain Python integers).

Definition (include/quade_hip.h and quade_amd/csrc/quade_dup.h state the same; the kernels implement exactly this).  Parameters:
B = bases (8 .. 32), sample (a power of two, 1 .. 1024), slots (a power of two, 2^10 .. 2^28).  Per pair that carries no filter
reason, with reads s1, s2 of current lengths L1, L2:
  fold     u(b) = b & 0xDF; a base is valid when u(b) is one of A, C, G, T
  code     c(b) = (u(b) >> 1) & 3, which gives A 0, C 1, T 2, G 3
  class    the first that applies: short (L1 < B or L2 < B); with_n (an invalid base among the first B of either read); keyed
  key      (w1, w2, d): w_r = sum over i < B of c(s_r[i]) << (2 i); d = the routing code, 0xFFFF mapped to 2 S
  hash     h = tag({w1, w2, d, 0}): the unknown tally's tag function, restated below mod 2^64
  sampled  sample == 1, or h >> (64 - log2 sample) == 0
  tally    sampled pairs are counted per key in a table of `slots` entries: slot tag = trim(h, tag_mask), home slot = home(tag),
           probe limit min(slots, 1024); a pair that finds no entry, or whose tag belongs to another key, is not_tallied

The model is the ideal table (every sampled key admitted); check_exact / check_lossy state what a device table must satisfy against
it, in the manner of tests/unknown_model.py.
"""
from collections import Counter

UNDETERMINED = 0xFFFF
M64 = (1 << 64) - 1
COUNTERS = ("pairs", "short", "with_n", "sampled", "not_tallied")
PAIRS, SHORT, WITH_N, SAMPLED, NOT_TALLIED = range(5)
TOP_LEVEL = 32


class Params(object):
    def __init__(self, bases=32, sample=16, slots=1 << 24):
        assert 8 <= bases <= 32 and 1 <= sample <= 1024 and sample & (sample - 1) == 0
        assert 1 << 10 <= slots <= 1 << 28 and slots & (slots - 1) == 0
        self.bases, self.sample, self.slots = bases, sample, slots

    def keywords(self):
        return dict(bases=self.bases, sample=self.sample, slots=self.slots)


def fold(b):
    return b & 0xDF


def valid(b):
    return fold(b) in b"ACGT"


def code(b):
    return (fold(b) >> 1) & 3


def word(seq, B):
    """the first B bases of seq (len(seq) >= B, all valid) as one integer below 2^(2 B)"""
    w = 0
    for i in range(B):
        w |= code(seq[i]) << (2 * i)
    return w


def tag(words):
    """the 64-bit tag of four key words (qd_uk_tag)"""
    assert len(words) == 4
    h = 0x9E3779B97F4A7C15
    for w in words:
        h = ((h ^ w) * 0xFF51AFD7ED558CCD) & M64
        h ^= h >> 32
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    return h ^ (h >> 29)


def trim(h, tag_bits=64):
    """the slot tag: the low tag_bits of h, 0 replaced by 1 (qd_uk_trim)"""
    t = h & ((1 << tag_bits) - 1)
    return t if t else 1


def home(t, lg):
    """first slot of a tag's probe sequence (qd_uk_home)"""
    return ((t * 0x9E3779B97F4A7C15) & M64) >> (64 - lg)


def key_hash(key):
    return tag((key[0], key[1], key[2], 0))


def sampled(h, sample):
    lg = sample.bit_length() - 1
    return sample == 1 or (h >> (64 - lg)) == 0


def classify(seq1, seq2, B):
    """'short', 'with_n' or the pair's (w1, w2)"""
    if len(seq1) < B or len(seq2) < B:
        return "short"
    if not all(valid(b) for b in seq1[:B] + seq2[:B]):
        return "with_n"
    return word(seq1, B), word(seq2, B)


def dest(c, S):
    d = 2 * S if c == UNDETERMINED else c
    assert 0 <= d <= 2 * S
    return d


def tally(S, pairs, P):
    """pairs: (code, seq1, seq2, dropped) -> (Counter of the sampled keys (w1, w2, d), stats [2 S + 1][5] with not_tallied 0)"""
    stats = [[0] * len(COUNTERS) for _ in range(2 * S + 1)]
    table = Counter()
    for c, s1, s2, dropped in pairs:
        if dropped:
            continue
        d = dest(int(c), S)
        stats[d][PAIRS] += 1
        k = classify(bytes(s1), bytes(s2), P.bases)
        if k == "short":
            stats[d][SHORT] += 1
        elif k == "with_n":
            stats[d][WITH_N] += 1
        else:
            key = (k[0], k[1], d)
            if sampled(key_hash(key), P.sample):
                stats[d][SAMPLED] += 1
                table[key] += 1
    return table, stats


def no_shared_tags(keys, tag_bits=64):
    """no two of the keys share a slot tag: not_tallied == 0 is then a fact about the input (given room in the table)"""
    tags = [trim(key_hash(k), tag_bits) for k in keys]
    return len(set(tags)) == len(tags)


def table_counter(keys, counts):
    """a device table (keys [n][3], counts [n]) as a Counter; a key twice is an error"""
    out = Counter()
    for k, c in zip(keys, counts):
        key = (int(k[0]), int(k[1]), int(k[2]))
        assert key not in out, "a key twice in one table: %r" % (key,)
        assert int(c) > 0, "an entry without pairs"
        out[key] = int(c)
    return out


def by_dest(table, n_dest):
    out = [0] * n_dest
    for (_, _, d), c in table.items():
        out[d] += c
    return out


def check_invariant(table, stats):
    """per destination: sampled == tallied + not_tallied"""
    tallied = by_dest(table, len(stats))
    for d, row in enumerate(stats):
        assert int(row[SAMPLED]) == tallied[d] + int(row[NOT_TALLIED]), (d, [int(x) for x in row], tallied[d])


def check_exact(table, stats, model, model_stats):
    """not_tallied == 0 everywhere: the table is the exact multiset and the counters are the model's"""
    check_invariant(table, stats)
    assert [[int(x) for x in r] for r in stats] == [list(r) for r in model_stats]
    assert all(int(r[NOT_TALLIED]) == 0 for r in stats)
    assert table == model, (sorted((model - table).items())[:5], sorted((table - model).items())[:5])


def check_lossy(table, stats, model, model_stats):
    """some pairs were not tallied: every entry present is exact, and per destination not_tallied is the pairs of the absent keys"""
    check_invariant(table, stats)
    assert sum(int(r[NOT_TALLIED]) for r in stats) > 0
    for d, (row, want) in enumerate(zip(stats, model_stats)):
        assert [int(x) for x in row[:NOT_TALLIED]] == list(want[:NOT_TALLIED]), d
    for key, c in table.items():
        assert model[key] == c, (key, c, model[key])
    absent = by_dest(Counter({k: c for k, c in model.items() if k not in table}), len(stats))
    assert absent == [int(r[NOT_TALLIED]) for r in stats]


def report_rows(table, stats):
    """the report's figures: ([per destination and then Total: pairs, short, with_n, keyed, sampled, not_tallied, tallied, distinct,
    duplicate_pairs], {level 1 .. 32 (32: and more): (keys, pairs)} of the levels that occur)"""
    n = len(stats)
    tallied, distinct = by_dest(table, n), by_dest(Counter({k: 1 for k in table}), n)
    rows = []
    for d in range(n):
        p, s, w, smp, nt = (int(x) for x in stats[d])
        rows.append([p, s, w, p - s - w, smp, nt, tallied[d], distinct[d], tallied[d] - distinct[d]])
    rows.append([sum(col) for col in zip(*rows)])
    levels = {}
    for c in table.values():
        k, p = levels.get(min(c, TOP_LEVEL), (0, 0))
        levels[min(c, TOP_LEVEL)] = (k + 1, p + c)
    return rows, levels


def arrays(table):
    """the Counter as (keys [n][3], counts [n]) lists, the form quade_amd.duplication_report takes"""
    items = sorted(table.items())
    return [list(k) for k, _ in items], [c for _, c in items]
