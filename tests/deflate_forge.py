"""A DEFLATE writer for tests: streams that are legal (or illegal in exactly one way) but that zlib and libdeflate never write.

The inflaters (quade_amd/csrc/inflate3_lane.h, quade_inflate.hip, quade_inflate3.hip, quade_pgz.cpp) are otherwise only ever fed what
those two encoders emit.  Here every token, every code length and every header field is chosen by hand: distances 32 507 .. 32 768,
258 as symbol 284 + 31, 15-bit codes followed by 13 extra bits, degenerate and run-length coded code tables, dozens of tiny blocks of
mixed types, gzip / BGZF framing with every optional field -- and one stream per refusal RFC 1951 asks of a decoder.

Standard library only.  `corpus()` is built once per process; tests/test_host_forge.py proves it against zlib.

Tokens of a block: an int is a literal byte; `(length, distance)` a match; `(258, distance, True)` a match whose length is written
as symbol 284 with 31 extra bits; `("S", symbol)` a bare literal/length symbol; `("D", symbol, extra)` a bare distance symbol.
"""
import struct
import zlib

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 0, 0)
CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class BitWriter(object):
    """LSB-first bits into bytes; the accumulator is an int that is emptied every kilobit."""
    __slots__ = ("out", "acc", "n")

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 1024:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n &= 7

    def align(self):
        self.n = (self.n + 7) & ~7

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def raw(self, data):
        assert self.n % 8 == 0
        self.out += self.acc.to_bytes(self.n >> 3, "little")
        self.acc = self.n = 0
        self.out += data

    def getvalue(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def _reverse(code, nbits):
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lengths):
    """code lengths -> per symbol (code as it goes into an LSB-first stream, bits), None for a symbol without a code.  The lengths
    need not make a complete code (the illegal cases use that): an over-subscribed set just gives colliding codes."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if not l:
            out.append(None)
            continue
        out.append((_reverse(nxt[l] & ((1 << l) - 1), l), l))
        nxt[l] += 1
    return out


def balanced(symbols, n):
    """a complete code over `symbols` (of n): the shortest that is nearly flat.  One symbol: a single 1-bit code (incomplete, legal)."""
    syms = sorted(set(symbols))
    lens = [0] * n
    k = len(syms)
    if k == 1:
        lens[syms[0]] = 1
        return lens
    m = (k - 1).bit_length()
    short = (1 << m) - k
    for i, s in enumerate(syms):
        lens[s] = m - 1 if i < short else m
    return lens


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _len_symbol(length):
    for s in range(28, -1, -1):
        if LBASE[s] <= length:
            return s
    raise ValueError(length)


def _dist_symbol(dist):
    for s in range(29, -1, -1):
        if DBASE[s] <= dist:
            return s
    raise ValueError(dist)


def symbols_used(tokens):
    """(literal/length symbols, distance symbols) a token list needs, end-of-block included"""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        elif t[0] == "S":
            ls.add(t[1])
        elif t[0] == "D":
            ds.add(t[1])
        else:
            ls.add(284 if len(t) > 2 and t[2] else 257 + _len_symbol(t[0]))
            ds.add(_dist_symbol(t[1]))
    return ls, ds


def emit_tokens(w, tokens, lit, dist, eob=True):
    put = w.put
    for t in tokens:
        if isinstance(t, int):
            put(*lit[t])
        elif t[0] == "S":
            put(*lit[t[1]])
        elif t[0] == "D":
            put(*dist[t[1]])
            put(t[2], DEXT[t[1]])
        else:
            length, d = t[0], t[1]
            if len(t) > 2 and t[2]:
                assert length == 258
                put(*lit[284])
                put(31, 5)
            else:
                s = _len_symbol(length)
                put(*lit[257 + s])
                put(length - LBASE[s], LEXT[s])
            s = _dist_symbol(d)
            put(*dist[s])
            put(d - DBASE[s], DEXT[s])
    if eob:
        put(*lit[256])


def fixed_block(w, tokens, final=False):
    w.put((1 if final else 0) | (1 << 1), 3)
    emit_tokens(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def stored_block(w, data, final=False, nlen=None):
    assert len(data) <= 65535
    w.put(1 if final else 0, 3)
    w.align()
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + bytes(data))


def rle_plain(lengths):
    """every code length as itself"""
    return [(l, 0) for l in lengths]


def rle_greedy(lengths):
    """runs as zlib would code them: 18 / 17 for zeros, 16 for repeats"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
        out.extend([(v, 0)] * run)
        i = j
    return out


def rle_expand(plan):
    """the code lengths a plan of (symbol, extra) stands for"""
    out = []
    for s, x in plan:
        if s < 16:
            out.append(s)
        elif s == 16:
            out.extend([out[-1]] * (3 + x))
        else:
            out.extend([0] * ((3 if s == 17 else 11) + x))
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_header(w, litlens, distlens, final=False, plan=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
    """BFINAL, BTYPE 2, HLIT / HDIST / HCLEN, the code-length code and the run-length coded lengths.
    plan: (symbol, extra) items for the lit + dist lengths together (default: every length as itself); cl_lens: the code-length
    code's 19 lengths by symbol (default: a nearly flat complete code over the symbols the plan uses); hclen / hlit / hdist: the
    header's counts when they are not to follow from the lists."""
    if plan is None:
        plan = rle_plain(list(litlens) + list(distlens))
    if cl_lens is None:
        used = sorted({s for s, _ in plan})
        if len(used) == 1:  # (the code-length code must be complete: a second, unused 1-bit code)
            used.append(0 if used[0] else 1)
        cl_lens = balanced(used, 19)
    if hclen is None:
        hclen = max(4, 1 + max(k for k in range(19) if cl_lens[CLORDER[k]]))
    w.put((1 if final else 0) | (2 << 1), 3)
    w.put((len(litlens) if hlit is None else hlit) - 257, 5)
    w.put((len(distlens) if hdist is None else hdist) - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CLORDER[k]], 3)
    cl = canonical(cl_lens)
    for s, x in plan:
        w.put(*cl[s])
        if s >= 16:
            w.put(x, CL_EXTRA[s])


def dynamic_block(w, tokens, litlens=None, distlens=None, final=False, eob=True, **kw):
    """litlens / distlens default to nearly flat codes over what the tokens use (no distances: HDIST 1 with length 0)"""
    ls, ds = symbols_used(tokens)
    if litlens is None:
        litlens = balanced(ls, max(ls) + 1 if max(ls) > 256 else 257)
    if distlens is None:
        distlens = balanced(ds, max(ds) + 1) if ds else [0]
    dynamic_header(w, litlens, distlens, final, **kw)
    emit_tokens(w, tokens, canonical(litlens), canonical(distlens), eob)


def expand(tokens, text):
    """tokens appended to text (a bytearray)"""
    for t in tokens:
        if isinstance(t, int):
            text.append(t)
        else:
            length, d = t[0], t[1]
            assert 1 <= d <= len(text), (d, len(text))
            if d >= length:
                text += text[len(text) - d:len(text) - d + length]
            else:
                for _ in range(length):
                    text.append(text[-d])
    return text


# ---- framing -------------------------------------------------------------------------------------------------------------------------
def gzip_member(raw, text, extra=None, name=None, comment=None, hcrc=False, crc=None, isize=None):
    """RFC 1952: any of FEXTRA (extra: the field's bytes), FNAME, FCOMMENT (bytes without the NUL), FHCRC"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x00\x03"
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    text = b"" if text is None else text
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc, (len(text) if isize is None else isize) & 0xFFFFFFFF)


def subfield(si, data):
    return si + struct.pack("<H", len(data)) + data


def bgzf_block(raw, text, before=b"", after=b"", crc=None, isize=None):
    """a BGZF block (SAM specification 4.1): the 'BC' subfield holds the block's size - 1; before / after: other extra subfields"""
    xlen = len(before) + 6 + len(after)
    bsize = 12 + xlen + len(raw) + 8
    assert bsize <= 65536, bsize
    text = b"" if text is None else text
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + before + b"BC" + struct.pack("<HH", 2, bsize - 1) + after + raw +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc, len(text) if isize is None else isize))


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------
class _Rng(object):
    """a fixed sequence (64-bit LCG): the corpus is the same bytes in every process"""

    def __init__(self, seed):
        self.s = seed

    def next(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.s >> 33) % n


def _acgt(rng, n):
    return [b"ACGT"[rng.next(4)] for _ in range(n)]


def _done(w, toks):
    return w.getvalue(), bytes(expand(toks, bytearray()))


def _l1(rng, alt284, first_at_32768):
    """32 768 literals of ACGT, then matches of 258 and 3 at distances 32 768, 32 767 and 32 507; the first match either directly
    behind the literals (position 32 768: it reaches byte 0) or some literals later"""
    toks = _acgt(rng, 32768)
    if not first_at_32768:
        toks += _acgt(rng, 5)
    for d in (32768, 32767, 32507):
        toks += [(258, d, True) if alt284 else (258, d), (3, d)] + _acgt(rng, 2)
    w = BitWriter()
    dynamic_block(w, toks, final=True)
    return _done(w, toks)


# L2: one literal at each length 2,2,2,3 .. 14 and two at 15: nine symbols behind 7 bits; the distance code holds all 30 symbols,
# 28 and 29 (13 extra bits) at 15 bits: ten behind 6 bits -- every lane configuration's long-symbol table holds both
def _l2_codes():
    lit = [0] * 286
    order = [ord("A"), ord("C"), ord("G"), ord("T"), 10, 256, 257, 285, ord("N"), ord("@"), ord("+"), ord("I"), 284, ord(":"), 258, ord("#"), ord("F")]
    for s, l in zip(order, [2, 2, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]):
        lit[s] = l
    dist = [4] * 13 + [5, 5, 5, 6, 6] + [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]
    assert len(dist) == 30
    return lit, dist


def _l2(rng, full_hclen):
    if not full_hclen:
        # the smallest HCLEN a legal block allows is 5 (16, 17, 18, 0, 8: with 4 every length would be zero, and no end-of-block code):
        # every code is 8 bits -- literals 0 .. 254 and end-of-block, HDIST 1 of length 0
        toks = list(range(255))
        litl = [8] * 255 + [0, 8]
        plan = [(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0), (0, 0), (8, 0), (0, 0)]
        assert rle_expand(plan) == litl + [0]
        cl = [0] * 19
        cl[16], cl[0], cl[8] = 1, 2, 2
        w = BitWriter()
        dynamic_header(w, litl, [0], final=True, plan=plan, cl_lens=cl)
        emit_tokens(w, toks, canonical(litl), canonical([0]))
        return _done(w, toks)
    lit, dist = _l2_codes()
    toks = _acgt(rng, 32768) + [ord(c) for c in "@N+I:#F\n"]
    for d in (32768, 24577, 24576, 16385, 32767, 12289, 8193, 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049,
              3073, 4097, 6145):
        toks += [(258, d), (3, d), (258, d, True), (4, d), ord("#")]
    w = BitWriter()
    dynamic_block(w, toks, lit, dist, final=True)  # (HCLEN 19: symbol 15, the last in the header's order, is in use)
    return _done(w, toks)


def _l2x(rng, n_text=3000):
    """256 literal/length symbols at 15 bits (end of block among them), seven at 1 .. 7 bits: no lane configuration's table holds it"""
    lit = [0] * 286
    short = [ord("A"), ord("C"), ord("G"), ord("T"), 10, 257, ord("N")]
    for s, l in zip(short, range(1, 8)):
        lit[s] = l
    longs = [s for s in range(286) if s not in short and s not in (256, 285)][:254] + [256, 285]
    for s in longs:
        lit[s] = 15
    assert sum(1 for l in lit if l == 15) == 256
    long_bytes = [s for s in longs if s < 256]
    toks, n = [], 0
    for i in range(n_text):
        toks.append(long_bytes[rng.next(len(long_bytes))] if rng.next(16) == 0 else (65, 67, 71, 84, 10, 78)[rng.next(6)])
        n += 1
        if i % 97 == 96:
            toks.append((3, 1 + rng.next(min(n, 60))))
            n += 3
        if i % 501 == 500:
            toks.append((258, 1 + rng.next(60)))
            n += 258
    w = BitWriter()
    dynamic_block(w, toks, lit, balanced(range(12), 12), final=True)
    return _done(w, toks)


def _mix_blocks(rng, with_big_stored):
    """about 60 blocks in one stream, of every type and of the emptiest kinds"""
    w, toks = BitWriter(), []

    def some(n):
        t = _acgt(rng, n) + [10]
        if len(toks) > 40:
            t += [(3 + rng.next(30), 1 + rng.next(40))]
        return t

    for r in range(8):
        stored_block(w, b"")                                   # empty stored, non-final (what a sync flush writes)
        fixed_block(w, [])                                     # empty fixed: 10 bits
        b = [b"ACGTN@+\n"[r]]
        stored_block(w, bytes(b))                              # 1-byte stored
        toks += b
        t = some(20 + 7 * r)
        dynamic_block(w, t)
        toks += t
        t = some(5 + r)
        fixed_block(w, t)
        toks += t
        dynamic_block(w, [], litlens=[0] * 256 + [1], distlens=[0])  # empty dynamic: the only code is end-of-block
        if r % 3 == 0:
            w.put(0, 3)                                        # an empty stored block whose header starts at any bit offset
            w.align()
            w.raw(b"\0\0\xff\xff")
    if with_big_stored:
        big = bytes(_acgt(rng, 65535))
        stored_block(w, big)
        toks += list(big)
    return w, toks


def _l5(rng, ending, with_big_stored=False):
    w, toks = _mix_blocks(rng, with_big_stored)
    if ending == "aligned":  # a final fixed block that ends exactly on a byte boundary (a 9-bit literal moves its end by one bit)
        for nine in range(8):
            t = [65, 10] + [200] * nine
            probe = BitWriter()
            probe.put(0, w.bitpos() % 8)
            fixed_block(probe, t, final=True)
            if probe.bitpos() % 8 == 0:
                break
        assert probe.bitpos() % 8 == 0
        fixed_block(w, t, final=True)
        toks += t
    else:  # a final empty stored block
        stored_block(w, b"", final=True)
    return _done(w, toks)


def _l6_chain():
    """64 KiB of back-to-back matches of 258 at distances 1 .. 8: every byte's chain of parents leads to the first eight"""
    toks, n, k = list(b"ACGTTGCA"), 8, 0
    while n + 258 <= 65536 - 3:
        toks.append((258, 1 + k % 8))
        n += 258
        k += 1
    toks.append((65536 - n, 3))
    w = BitWriter()
    dynamic_block(w, toks, final=True)
    return _done(w, toks)


TEXT_BYTES = [9, 10, 13] + list(range(32, 127))


def _l6_gzip(rng, n_text=1_300_000, block_text=9_000):
    """Literals of 98 text bytes (6 .. 7 bits each: more than 1 MiB of stream) in dynamic blocks of ~8 KiB; behind EVERY block start -- so
    behind every stretch, unit and step boundary a decoder cuts at -- matches whose source starts in front of the block and runs into
    their own output (distance > position in the block, length > distance - position), the far distances among them."""
    w = BitWriter()
    text = bytearray()
    litl = balanced(TEXT_BYTES + [256, 257 + 17, 285], 286)  # (lengths 43 .. 50 and 258)
    lits = canonical(litl)
    far = (32768, 32767, 32507, 24577, 9000, 300, 40, 9)
    bi = 0
    while len(text) < n_text:
        final = len(text) + block_text >= n_text
        toks = []
        if text:
            lead = bi % 3  # the match's position in the block
            toks += [TEXT_BYTES[rng.next(98)] for _ in range(lead)]
            k = min((1, 2, 7, 100, 257)[bi % 5], len(text))  # its source starts k bytes in front of the block and is longer than that
            toks.append((258, lead + k))
            if far[bi % 8] <= len(text):
                toks.append((43 + bi % 8, far[bi % 8]))
        toks += [TEXT_BYTES[rng.next(98)] for _ in range(block_text)]
        ds = symbols_used(toks)[1]
        dl = balanced(ds, 30) if ds else [0]
        dynamic_header(w, litl, dl, final, plan=rle_greedy(litl + dl))
        emit_tokens(w, toks, lits, canonical(dl))
        expand(toks, text)
        bi += 1
    return w.getvalue(), bytes(text)


def _zlib_flushes(rng):
    text = bytes(b"ACGTN\n@+I#"[rng.next(10)] for _ in range(20_000))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b""
    for a in range(0, len(text), 1000):
        raw += c.compress(text[a:a + 1000]) + c.flush(zlib.Z_FULL_FLUSH if a % 7000 == 6000 else zlib.Z_SYNC_FLUSH)
    return raw + c.flush(), text


def _legal(rng):
    out = []

    def add(name, pair, **tags):
        out.append((name, pair[0], pair[1], tags))

    add("L1 far matches", _l1(rng, False, False), needs_history=True)
    add("L1 258 as 284+31", _l1(rng, True, False), needs_history=True)
    add("L1 first match at 32768 reaches byte 0", _l1(rng, True, True), needs_history=True)
    add("L2 widest codes, HCLEN 19", _l2(rng, True), needs_history=True, long_codes=19)
    add("L2 smallest HCLEN", _l2(rng, False))
    add("L2x 256 codes of 15 bits", _l2x(rng), long_codes=256)

    def one(toks, **kw):
        w = BitWriter()
        dynamic_block(w, toks, final=True, **kw)
        return _done(w, toks)

    t = _acgt(rng, 300)
    add("L3 literals only, HDIST 1 of length 0", one(t, distlens=[0]))
    add("L3 one distance code of 1 bit", one(t + [(258, 1), (3, 1), 10], distlens=[1]))
    add("L3 empty block: only end-of-block, 1 bit", one([], litlens=[0] * 256 + [1], distlens=[0]))
    add("L3 two-symbol distance code", one(t + [(9, 1), (258, 2), (3, 1), 10], distlens=[1, 1]))
    # L4: code-length runs.  lit: A C G T at 3 bits, newline + end-of-block + length 3 at 3 bits, one more at 3: 8 codes of 3 bits;
    # the distance code's first 8 lengths are 3 as well, so that a 16 can repeat across the boundary
    litl = [0] * 258
    for s in (65, 67, 71, 84, 10, 78, 256, 257):
        litl[s] = 3
    distl = [3] * 8
    t4 = _acgt(rng, 100) + [(3, 1), (3, 8), (3, 12), (3, 16), 10, 78]
    plan = ([(0, 0)] * 10 + [(3, 0), (18, 43), (3, 0), (0, 0), (3, 0), (17, 0), (3, 0), (17, 3), (3, 0), (17, 2), (3, 0)] +   # .. symbol 84
            [(18, 127), (16, 3), (17, 0), (16, 0), (18, 0), (16, 3), (17, 1)] +   # 171 zeros: 18 with 138, 16 behind 18 and behind 17 (repeats zero)
            [(3, 0), (16, 3), (16, 0)])                                          # 256, then 16s that run through 257 into the distance lengths
    lens = rle_expand(plan)
    assert lens == litl + distl, [i for i in range(min(len(lens), 266)) if lens[i] != (litl + distl)[i]][:5]

    def planned(plan, litl, distl, toks):
        w = BitWriter()
        dynamic_header(w, litl, distl, final=True, plan=plan)
        emit_tokens(w, toks, canonical(litl), canonical(distl))
        return _done(w, toks)

    add("L4 runs: 16 across the boundary, 18 x 138, 16 after 17 and 18", planned(plan, litl, distl, t4))
    for ending in ("aligned", "empty stored"):
        add("L5 block mix, final " + ending, _l5(rng, ending), multi_block=True)
    add("L5 block mix with a stored block of 65535", _l5(rng, "empty stored", True), multi_block=True, gzip_only=True)
    add("L5 zlib sync and full flushes", _zlib_flushes(rng), multi_block=True)
    add("L6 chains of 258 at distances 1..8", _l6_chain(), isize_64k=True)
    add("L6 matches across every block start", _l6_gzip(rng), multi_block=True, needs_history=True, gzip_only=True)
    return out


def _illegal(rng):
    out = []

    def add(name, w, isize, **tags):
        tags["isize"] = isize
        out.append((name, w.getvalue() if isinstance(w, BitWriter) else w, None, tags))

    base = _acgt(rng, 200)
    tail = _acgt(rng, 50)

    # I1: a distance that reaches in front of the stream's start
    w = BitWriter()
    fixed_block(w, [65, (3, 2)] + tail, final=True)
    add("I1 distance 2 at position 1", w, 4 + len(tail), too_far=True)
    w = BitWriter()
    first = _acgt(rng, 32000)
    dynamic_block(w, first)
    second = _acgt(rng, 767)
    dynamic_block(w, second + [(258, 32768)] + tail, final=True)
    add("I1 distance 32768 at position 32767, second block", w, 32767 + 258 + len(tail), too_far=True, multi_block=True)
    # I2 / I3: symbols the fixed code has and DEFLATE does not
    w = BitWriter()
    fixed_block(w, base + [("S", 257), ("D", 30, 0)] + tail, final=True)
    add("I2 fixed block, distance symbol 30", w, len(base) + 3 + len(tail))
    w = BitWriter()
    fixed_block(w, base + [("S", 286)] + tail, final=True)
    add("I3 fixed block, literal/length symbol 286", w, len(base) + len(tail))

    lit8 = balanced([65, 67, 71, 84, 10, 78, 256, 257], 258)  # eight codes of 3 bits
    toks = base + [(3, 1)] + tail
    n = len(base) + 3 + len(tail)

    def header_case(name, litl, distl, **kw):
        w = BitWriter()
        dynamic_header(w, litl, distl, final=True, **kw)
        emit_tokens(w, toks, [c or (0, 1) for c in canonical(litl)[:258]], [c or (0, 1) for c in canonical(distl)])
        add(name, w, n)

    over = list(lit8)
    over[66] = 3
    header_case("I4 over-subscribed literal code", over, [1, 1])
    inc = list(lit8)
    inc[78] = 0
    header_case("I5 incomplete literal code", inc, [1, 1])
    header_case("I6 incomplete distance code of two lengths", lit8, [1, 2])
    noeob = list(lit8)
    noeob[256], noeob[66] = 0, 3
    header_case("I7 no end-of-block code", noeob, [1, 1])
    header_case("I8 HLIT 287", lit8 + [0] * 29, [1, 1])
    header_case("I9 HDIST 31", lit8, [1, 1] + [0] * 29)
    full = rle_plain(lit8 + [1, 1])
    header_case("I10 repeat-previous as the first code length", lit8, [1, 1], plan=[(16, 0)] + full[3:], cl_lens=balanced([0, 1, 3, 16], 19))
    header_case("I11 a repeat that runs past HLIT + HDIST", lit8, [1, 1], plan=full[:-1] + [(16, 0)], cl_lens=balanced([0, 1, 3, 16], 19))
    cl = balanced([0, 1, 3], 19)
    cl[3] += 1
    header_case("I12 incomplete code-length code", lit8, [1, 1], cl_lens=cl)
    w = BitWriter()
    stored_block(w, bytes(base), nlen=(len(base) ^ 0xFFFF) ^ 0x0100)
    fixed_block(w, tail, final=True)
    add("I13 stored block, LEN / NLEN mismatch", w, len(base) + len(tail))
    w = BitWriter()
    fixed_block(w, base)
    w.put(1 | (3 << 1), 3)
    emit_tokens(w, tail, canonical(FIXED_LIT), canonical(FIXED_DIST))
    add("I14 BTYPE 3", w, len(base) + len(tail))
    w = BitWriter()
    dynamic_header(w, lit8, [1], final=True)
    emit_tokens(w, base + [("S", 257)], canonical(lit8), [(0, 1)], eob=False)
    w.put(1, 1)  # the distance code's one code is '0'
    emit_tokens(w, tail, canonical(lit8), [(0, 1)])
    add("I15 the unused bit pattern of a single 1-bit distance code", w, n)
    w = BitWriter()
    fixed_block(w, base)
    dynamic_block(w, tail)
    add("I16 no final block", w, len(base) + len(tail))
    return out


# ---- a GIVEN text in the corpus's kinds of blocks (the pipeline tests re-frame an input file with these) -------------------------------
def l2x_litlens():
    """the L2x literal/length code over every byte value: A C G T newline N and length 3 at 1 .. 7 bits, 256 symbols at 15 bits"""
    lit = [0] * 286
    short = [ord("A"), ord("C"), ord("G"), ord("T"), 10, 257, ord("N")]
    for s, l in zip(short, range(1, 8)):
        lit[s] = l
    for s in [s for s in range(286) if s not in short and s not in (256, 285)][:254] + [256, 285]:
        lit[s] = 15
    return lit


def far_tokens(text, start, end):
    """text[start:end] as literals and, wherever the text allows one, a match at a distance of 32 504 .. 32 768 (zlib stops at 32 506)"""
    toks, p = [], start
    while p < end:
        if p >= 32768 and p % 5 == 0 and p + 3 <= end:
            lo = p - 32768
            j = text.find(text[p:p + 3], lo, lo + 265)
            if j >= 0:
                ln = 3
                while ln < 258 and p + ln < end and text[j + ln] == text[p + ln]:
                    ln += 1
                toks.append((ln, p - j))
                p += ln
                continue
        toks.append(text[p])
        p += 1
    return toks


def forge_stream(text, block=20_000, l2x=True):
    """one DEFLATE stream for `text`: (with l2x) a block of the L2x code first -- long_codes=256: no lane configuration decodes it --,
    then dynamic blocks with far matches, an empty stored block (a sync flush) and an empty fixed block between them"""
    w = BitWriter()
    at = 0
    if l2x:
        at = min(1500, len(text))
        lit = l2x_litlens()
        dynamic_header(w, lit, [0], final=at == len(text), plan=rle_greedy(lit + [0]))
        emit_tokens(w, list(text[:at]), canonical(lit), [None])
    while at < len(text) or not w.bitpos():
        end = min(at + block, len(text))
        stored_block(w, b"")
        fixed_block(w, [])
        dynamic_block(w, far_tokens(text, at, end), final=end == len(text))
        if end == at:
            break
        at = end
    return w.getvalue()


def forge_bgzf_file(text, block_text=40_000):
    """`text` as a BGZF file whose every block is such a stream (matches reach 32 768 back inside the block), EOF block at the end"""
    out = []
    for a in range(0, len(text), block_text):
        part = text[a:a + block_text]
        out.append(bgzf_block(forge_stream(part, block=21_000, l2x=False), part))
    return b"".join(out) + bgzf_block(b"\x03\x00", b"")


_CORPUS = None


def corpus():
    """[(name, raw deflate stream, expected text or None for an illegal stream, tags)], built once per process.
    tags: long_codes=N (literal/length + distance symbols with codes longer than 7 bits -- beyond 112 no lane configuration decodes
    the block), needs_history (matches reach 32 KiB back), multi_block, gzip_only (does not fit BGZF blocks as it is), isize_64k (a
    text of exactly 65 536 bytes); illegal cases: isize (the text length a decoder that overlooked the defect would arrive at)."""
    global _CORPUS
    if _CORPUS is None:
        rng = _Rng(20240229)
        _CORPUS = _legal(rng) + _illegal(rng)
    return _CORPUS


def case(name_prefix):
    hits = [c for c in corpus() if c[0].startswith(name_prefix)]
    assert len(hits) == 1, (name_prefix, [c[0] for c in hits])
    return hits[0]
