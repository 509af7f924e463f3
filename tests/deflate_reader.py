"""A DEFLATE reader for tests: what a gzip member SAYS, block by block and token by token (RFC 1951 / 1952).

zlib tells whether a member inflates to its text; it does not tell how.  The tests of the device's coders
(tests/test_gpu_coder_corpus.py) must know that a text reached the seam it was built for -- a distance of exactly 32 768, a
token of more than 32 bits, a zero run of 138 in the header -- and read that from the member itself, whatever bytes the coder
chose.  The counterpart of tests/deflate_forge.py (which writes such streams); tests/test_host_coder_corpus.py proves the two
and zlib agree.

Standard library only.  Symbols are decoded by one table lookup on a peek of the block's longest code (at most 15 bits); the
bits come from an accumulator that is refilled eight bytes at a time.  A defect raises ValueError.
"""
import struct
from collections import namedtuple

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# kind: "stored" | "fixed" | "dynamic"; bit_start / bit_end: of the block (its BFINAL bit .. behind its last bit) in the member;
# hlit / hdist: how many literal/length and distance code lengths a dynamic block sends (None otherwise); cl_ops: the code-length
# code's operations as sent, (symbol 0 .. 18, how many lengths it stands for); tokens: (bit position in the member, bits, text
# position, length, distance), a literal with length 1 and distance 0, the end-of-block code not among them
Block = namedtuple("Block", "kind final bit_start bit_end text_start text_len hlit hdist litlens distlens cl_ops tokens")
Member = namedtuple("Member", "text crc32 isize blocks header_bytes length")


def _table(lengths):
    """code lengths -> (table, peek bits): table[peek] = symbol << 4 | length, 0 where no code reaches.  An over-subscribed set
    is a defect; an incomplete one is accepted (RFC 1951 allows the one-code distance tree, and a hole only matters when hit)."""
    top = max(lengths) if lengths else 0
    if top == 0:
        return [0], 0
    count = [0] * (top + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code, space = [0] * (top + 2), 0, 1 << top
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
        space -= count[l] << (top - l)
    if space < 0:
        raise ValueError("over-subscribed code")
    tab = [0] * (1 << top)
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l]
            nxt[l] += 1
            r = int(format(c, "0%db" % l)[::-1], 2)  # Huffman codes go most significant bit first
            tab[r::1 << l] = [s << 4 | l] * (1 << (top - l))
    return tab, top


_FIXED = None


def read_deflate(data, bit=0, text=None, max_blocks=None):
    """the blocks of the DEFLATE stream that starts at bit `bit` of data, up to and with its final block: (text, blocks, bit
    behind the final block).  text: a bytearray that is continued (history of a preset dictionary), a new one by default.
    max_blocks: stop behind that many blocks, final or not (what stands at a position where no stream begins)."""
    global _FIXED
    out = bytearray() if text is None else text
    blocks = []
    n_data = len(data)
    pos = bit >> 3  # next byte to load
    acc, n = 0, 0
    if bit & 7:
        acc, n, pos = data[pos] >> (bit & 7), 8 - (bit & 7), pos + 1
    from_bytes = int.from_bytes

    def need(k):  # at least k <= 56 bits in acc (zeros behind the end: a read there is caught by `at() > 8 * n_data`)
        nonlocal acc, n, pos
        if n < k:
            acc |= from_bytes(data[pos:pos + 8], "little") << n
            pos += 8
            n += 64

    def at():
        return 8 * pos - n

    def take(k):
        nonlocal acc, n
        need(k)
        v = acc & ((1 << k) - 1)
        acc >>= k
        n -= k
        return v

    final = 0
    while not final and (max_blocks is None or len(blocks) < max_blocks):
        bit_start = at()
        final = take(1)
        btype = take(2)
        text_start = len(out)
        hlit = hdist = None
        litlens = distlens = None
        cl_ops, tokens = [], []
        if btype == 3:
            raise ValueError("block type 3")
        if btype == 0:
            drop = n & 7  # to the byte boundary
            acc >>= drop
            n -= drop
            ln, nln = take(16), take(16)
            if ln ^ nln != 0xFFFF:
                raise ValueError("stored block: LEN / NLEN")
            a = at() >> 3
            if a + ln > n_data:
                raise ValueError("stored block: truncated")
            out += data[a:a + ln]
            pos, acc, n = a + ln, 0, 0
            blocks.append(Block("stored", final, bit_start, at(), text_start, ln, None, None, None, None, cl_ops, tokens))
            continue
        if btype == 1:
            if _FIXED is None:
                _FIXED = (_table(FIXED_LIT), _table(FIXED_DIST))
            (ltab, lpeek), (dtab, dpeek) = _FIXED
            litlens, distlens = list(FIXED_LIT), list(FIXED_DIST)
        else:
            hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
            if hlit > 286:
                raise ValueError("HLIT > 286")
            cl = [0] * 19
            for k in range(hclen):
                cl[CLORDER[k]] = take(3)
            ctab, cpeek = _table(cl)
            lens = []
            while len(lens) < hlit + hdist:
                need(24)
                e = ctab[acc & ((1 << cpeek) - 1)]
                if not e:
                    raise ValueError("no such code-length code")
                s, l = e >> 4, e & 15
                acc >>= l
                n -= l
                if s < 16:
                    lens.append(s)
                    cl_ops.append((s, 1))
                    continue
                if s == 16:
                    if not lens:
                        raise ValueError("repeat without a length")
                    r = 3 + take(2)
                    lens.extend([lens[-1]] * r)
                else:
                    r = 3 + take(3) if s == 17 else 11 + take(7)
                    lens.extend([0] * r)
                cl_ops.append((s, r))
            if len(lens) > hlit + hdist:
                raise ValueError("code lengths run past HLIT + HDIST")
            litlens, distlens = lens[:hlit], lens[hlit:]
            if not litlens[256]:
                raise ValueError("no end-of-block code")
            (ltab, lpeek), (dtab, dpeek) = _table(litlens), _table(distlens)
        lmask, dmask = (1 << lpeek) - 1, (1 << dpeek) - 1
        add = tokens.append
        while True:
            if n < 48:  # a token is at most 15 + 5 + 15 + 13 bits
                acc |= from_bytes(data[pos:pos + 8], "little") << n
                pos += 8
                n += 64
            e = ltab[acc & lmask]
            if not e:
                raise ValueError("no such literal/length code")
            s, l = e >> 4, e & 15
            if s < 256:
                add((8 * pos - n, l, len(out), 1, 0))
                out.append(s)
                acc >>= l
                n -= l
                continue
            if s == 256:
                acc >>= l
                n -= l
                break
            s -= 257
            if s > 28:
                raise ValueError("length symbol 286 / 287")
            x = LEXT[s]
            length = LBASE[s] + ((acc >> l) & ((1 << x) - 1))
            bits = l + x
            e = dtab[(acc >> bits) & dmask]
            if not e:
                raise ValueError("no such distance code")
            d, l = e >> 4, e & 15
            if d > 29:
                raise ValueError("distance symbol 30 / 31")
            bits += l
            x = DEXT[d]
            dist = DBASE[d] + ((acc >> bits) & ((1 << x) - 1))
            bits += x
            at_text = len(out)
            if dist > at_text:
                raise ValueError("distance %d at text position %d" % (dist, at_text))
            add((8 * pos - n, bits, at_text, length, dist))
            acc >>= bits
            n -= bits
            if dist >= length:
                out += out[at_text - dist:at_text - dist + length]
            else:
                unit = out[at_text - dist:]
                out += (unit * (length // dist + 1))[:length]
        if at() > 8 * n_data:
            raise ValueError("the stream ends inside a block")
        blocks.append(Block("fixed" if btype == 1 else "dynamic", final, bit_start, at(), text_start, len(out) - text_start, hlit, hdist,
                            litlens, distlens, cl_ops, tokens))
    if at() > 8 * n_data:
        raise ValueError("the stream ends inside a block")
    return out, blocks, at()


def gzip_header_bytes(gz, off=0):
    """length of the gzip header at gz[off:] (RFC 1952: FEXTRA, FNAME, FCOMMENT, FHCRC)"""
    if len(gz) < off + 10 or gz[off] != 0x1F or gz[off + 1] != 0x8B or gz[off + 2] != 8 or gz[off + 3] & 0xE0:
        raise ValueError("no gzip header")
    flg, a = gz[off + 3], off + 10
    if flg & 4:
        a += 2 + struct.unpack_from("<H", gz, a)[0]
    for f in (8, 16):
        if flg & f:
            a = gz.index(b"\0", a) + 1
    if flg & 2:
        a += 2
    return a - off


def read_member(gz, off=0):
    """the gzip member at gz[off:]: its text, the CRC-32 and ISIZE its trailer states (not verified here: the caller compares
    them with the text's), its blocks with bit positions counted from the member's first byte, and its length in bytes"""
    gz = bytes(gz[off:]) if off else bytes(gz)
    hb = gzip_header_bytes(gz)
    text, blocks, bit = read_deflate(gz, 8 * hb)
    tr = (bit + 7) >> 3
    if tr + 8 > len(gz):
        raise ValueError("no trailer")
    crc, isize = struct.unpack_from("<II", gz, tr)
    return Member(bytes(text), crc, isize, blocks, hb, tr + 8)


def read_members(gz):
    """every member of a gzip file"""
    out, off = [], 0
    while off < len(gz):
        out.append(read_member(gz, off))
        off += out[-1].length
    return out


def huffman_depth(counts):
    """depth of the deepest leaf of a Huffman tree for the non-zero ones of these counts, without any limit on the code length
    (two queues: the sorted leaves and the inner nodes, which come out in order).  Above 15: the block needed the limit."""
    leaves = sorted((c, 0) for c in counts if c)
    if len(leaves) < 2:
        return len(leaves)
    inner, i, j = [], 0, 0
    while len(leaves) - i + len(inner) - j > 1:
        pick = []
        for _ in range(2):
            if i < len(leaves) and (j >= len(inner) or leaves[i][0] <= inner[j][0]):
                pick.append(leaves[i])
                i += 1
            else:
                pick.append(inner[j])
                j += 1
        inner.append((pick[0][0] + pick[1][0], 1 + max(pick[0][1], pick[1][1])))
    return inner[-1][1]
