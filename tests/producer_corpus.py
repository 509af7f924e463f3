"""DEFLATE streams as the writers of real .fastq.gz files make them, for the tests of the device inflaters: libdeflate (fastp, htslib /
bgzip, samtools) at levels 1, 6, 9 and 12, pigz's shape (chunks with the previous 32 KiB as dictionary, a sync flush behind each), GNU
gzip's own deflate -- and three decoys: a dynamic block's header planted where no block starts.

zlib, which the other tests' inputs come from, never writes a block of more than 32 767 symbols nor a distance above 32 506; libdeflate
writes blocks of 300 KB of text (160 000 tokens, 150 KB of compressed bytes: nine stretches of the gzip probe without a block start) and
distances up to 32 768.  tests/test_host_producers.py proves with tests/deflate_reader.py that the streams have these shapes.

`corpus()` yields (name, raw DEFLATE stream, text, tags) like deflate_forge.corpus(); built once per process.
tags: producer ("libdeflate" | "pigz" | "gzip" | "decoy"), level, text (the text's name), needs ("libdeflate" | "gzip" | None: what must
be on the machine), decoy_byte (where the planted header stands in the stream; decoy (c): decoy_bit, header_bits), chunks (pigz: how many).
"""
import ctypes
import shutil
import subprocess
import zlib

import numpy as np

from tests import deflate_forge as F
from tests import deflate_reader as R

PIGZ_CHUNK = 128 << 10
BGZF_TEXT = 65280
STRETCH = 16 << 10  # the gzip probe's default stretch (quade_inflate3.hip); the tests' small geometry halves it


# ---- texts ---------------------------------------------------------------------------------------------------------------------------
def fastq(rng, n_bytes, n_qual=11, read_len=None):
    """records as tests/test_gpu_gunzip.py makes them"""
    out, size, i = [], 0, 0
    A = np.frombuffer(b"ACGTN", np.uint8)
    while size < n_bytes:
        L = read_len or int(rng.integers(30, 151))
        rec = b"@SIM:1:FC:%d:%d 1:N:0:\n%s\n+\n%s\n" % (i % 97, i * 7, bytes(A[rng.integers(0, 4, L)]), bytes(rng.integers(35, 35 + n_qual, L).astype(np.uint8)))
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n_bytes]


_TEXTS = None


def texts():
    """name -> text: the smallest sizes that still reach the seams (eight libdeflate blocks; twice the text per stretch; length 258 at
    distance 1; stored blocks; a fixed block; nothing)"""
    global _TEXTS
    if _TEXTS is None:
        rng = np.random.default_rng(20250611)
        _TEXTS = {"fastq": fastq(rng, 2_400_000), "fastq, 4 qualities, one read length": fastq(rng, 2_400_000, n_qual=4, read_len=150),
                  "runs": b"A" * 700_000, "random bytes": bytes(rng.integers(0, 256, 400_000).astype(np.uint8))}
        _TEXTS["short"] = _TEXTS["fastq"][:300]
        _TEXTS["tiny"] = _TEXTS["fastq"][:30]  # (300 bytes still get a dynamic block from libdeflate 1.x; 30 a fixed or a stored one)
        _TEXTS["empty"] = b""
    return _TEXTS


# ---- producers -----------------------------------------------------------------------------------------------------------------------
_LIBDEFLATE = False


def libdeflate():
    """libdeflate.so.0 (the name quade_io.cpp loads), or None"""
    global _LIBDEFLATE
    if _LIBDEFLATE is False:
        try:
            lib = ctypes.CDLL("libdeflate.so.0")
            lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
            lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
            lib.libdeflate_deflate_compress_bound.restype = ctypes.c_size_t
            lib.libdeflate_deflate_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
            lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
            lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
            lib.libdeflate_free_compressor.restype = None
            lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
            _LIBDEFLATE = lib
        except OSError:
            _LIBDEFLATE = None
    return _LIBDEFLATE


def libdeflate_raw(text, level):
    lib = libdeflate()
    c = lib.libdeflate_alloc_compressor(level)
    assert c, level
    try:
        cap = lib.libdeflate_deflate_compress_bound(c, len(text))
        out = ctypes.create_string_buffer(max(cap, 1))
        n = lib.libdeflate_deflate_compress(c, text, len(text), out, cap)
        assert n, (level, len(text))
        return out.raw[:n]
    finally:
        lib.libdeflate_free_compressor(c)


def zlib_raw(text, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(text) + c.flush()


def pigz_raw(text, chunk=PIGZ_CHUNK):
    """pigz's stream, made with zlib: every chunk coded on its own with the 32 KiB before it as dictionary and ended with a sync flush
    (an empty stored block), the last one with the final block"""
    out = []
    for a in range(0, max(len(text), 1), chunk):
        kw = {"zdict": text[max(0, a - 32768):a]} if a else {}
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, **kw)
        out.append(c.compress(text[a:a + chunk]) + c.flush(zlib.Z_FINISH if a + chunk >= len(text) else zlib.Z_SYNC_FLUSH))
    return b"".join(out)


def gnu_gzip():
    return shutil.which("gzip")


def gnu_gzip_raw(text, level):
    """the DEFLATE stream of the member GNU gzip writes (its own deflate, not zlib's), header and trailer taken off"""
    member = subprocess.run([gnu_gzip(), "-%d" % level, "-c", "-n"], input=text, stdout=subprocess.PIPE, check=True).stdout
    return member[R.gzip_header_bytes(member):-8]


# ---- blocks written again at another bit position --------------------------------------------------------------------------------------
def recode(w, raw, final=True):
    """the blocks of the stream `raw` appended to the BitWriter w: the same block types, code lengths and tokens (the header's run-length
    coding is deflate_forge's), its final block final or not.  Returns the stream's text."""
    text, blocks, _ = R.read_deflate(raw)
    for b in blocks:
        last = bool(b.final and final)
        if b.kind == "stored":
            F.stored_block(w, bytes(text[b.text_start:b.text_start + b.text_len]), final=last)
            continue
        toks = [text[t[2]] if t[4] == 0 else (t[3], t[4]) for t in b.tokens]
        if b.kind == "fixed":
            F.fixed_block(w, toks, final=last)
        else:
            F.dynamic_header(w, b.litlens, b.distlens, last, plan=F.rle_greedy(list(b.litlens) + list(b.distlens)))
            F.emit_tokens(w, toks, F.canonical(b.litlens), F.canonical(b.distlens))
    return bytes(text)


def one_block_tokens(raw):
    """all tokens of a stream (whose matches stay inside it), for one block"""
    text, blocks, _ = R.read_deflate(raw)
    return [text[t[2]] if t[4] == 0 else (t[3], t[4]) for b in blocks for t in b.tokens if b.kind != "stored"], bytes(text)


# ---- decoys --------------------------------------------------------------------------------------------------------------------------
def decoy_block(at=1_000_000):
    """A non-final dynamic block of a zlib level-6 stream of fastq, whole: (its bits as an int, how many, how many of them are the header)"""
    text = texts()["fastq"][at:at + 3000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(text) + c.flush(zlib.Z_SYNC_FLUSH)
    _, blocks, _ = R.read_deflate(raw + b"\x03\x00")  # (an empty final block, for the reader)
    b = blocks[0]
    assert b.kind == "dynamic" and not b.final and b.text_len == len(text)
    nbits = b.bit_end - b.bit_start
    return (int.from_bytes(raw, "little") >> b.bit_start) & ((1 << nbits) - 1), nbits, b.tokens[0][0] - b.bit_start


def decoy_bytes():
    """that block, its bits shifted to a byte boundary.  As the data of a stored block these bytes stand verbatim in a stream: a dynamic
    block's header holds there, and no block begins."""
    v, nbits, _ = decoy_block()
    return v.to_bytes((nbits + 7) >> 3, "little")


def _stored_data_at(w):
    """the byte at which the data of a stored block would begin that is written to w next"""
    return ((w.bitpos() + 3 + 7) >> 3) + 4


def decoy_a(big_raw, lead_bytes=40_000, stretch=STRETCH):
    """zlib blocks, then a stored block whose data ends with the decoy, directly in front of the blocks of big_raw (a libdeflate block of
    300 KB of text).  With `stretch` the decoy stands 16 bytes behind a stretch boundary of the probe, the true start of the long block
    1.5 KB further in the same stretch: the probe finds the decoy and never the true start.  (raw, text, decoy_byte)"""
    fq = texts()["fastq"]
    decoy = decoy_bytes()
    w = F.BitWriter()
    text = bytearray(recode(w, zlib_raw(fq[1_100_000:1_100_000 + lead_bytes]), final=False))
    at = _stored_data_at(w)
    fill = 16 if not stretch else (at + stretch - 1) // stretch * stretch + 16 - at
    data = fq[1_200_000:1_200_000 + fill] + decoy
    F.stored_block(w, data)
    text += data
    text += recode(w, big_raw, final=True)
    return w.getvalue(), bytes(text), at + fill


def decoy_b(stretch=STRETCH):
    """zlib blocks; a stored block of text up to 700 bytes in front of a stretch boundary; there a small dynamic block as zlib writes it
    (the first block start of its stretch: the true start of what follows); behind the boundary a stored block with the decoy, an empty
    fixed block's worth of text, and ONE dynamic block of 300 KB of text (all tokens of a zlib stream under a nearly flat code), whose
    start the decoy hides; zlib blocks to the end.  The unit from the true start has its stop -- the decoy -- some hundred bytes on and
    300 KB of text to run through.  (raw, text, decoy_byte)"""
    fq = texts()["fastq"]
    decoy = decoy_bytes()
    w = F.BitWriter()
    text = bytearray(recode(w, zlib_raw(fq[1_300_000:1_400_000]), final=False))
    small = zlib_raw(fq[1_400_000:1_401_500])
    at = _stored_data_at(w)
    boundary = (at + stretch + 1024 + stretch - 1) // stretch * stretch
    pad = fq[1_410_000:1_410_000 + boundary - (len(small) - 40) - at]  # the small block straddles the boundary, 40 bytes behind it
    F.stored_block(w, pad)
    text += pad
    assert boundary - len(small) < w.bitpos() // 8 < boundary
    text += recode(w, small, final=False)
    assert w.bitpos() // 8 >= boundary
    decoy_byte = _stored_data_at(w)
    F.stored_block(w, decoy)
    text += decoy
    some = list(fq[1_420_000:1_420_050])
    F.fixed_block(w, some)
    text += bytes(some)
    toks, t = one_block_tokens(zlib_raw(fq[1_500_000:1_800_000]))
    F.dynamic_block(w, toks)
    text += t
    text += recode(w, zlib_raw(fq[1_800_000:1_900_000]), final=True)
    return w.getvalue(), bytes(text), decoy_byte


# literals 0 .. 126 at 7 bits, literal 127 and end-of-block at 8: every string of bits without 1111111 1 is a run of literals
FLAT_LITLENS = [7] * 127 + [8] + [0] * 128 + [8]


def spell(v, nbits):
    """the first nbits (or a few more) of the bit string v as literals of the FLAT_LITLENS code, None if end-of-block stands in it"""
    by_code = {c: sym for sym, c in enumerate(F.canonical(FLAT_LITLENS)) if c}
    out, i = [], 0
    while i < nbits:
        sym = by_code.get(((v >> i) & 127, 7))
        if sym is None:
            sym = by_code[((v >> i) & 255, 8)]
            if sym == 256:
                return None
        out.append(sym)
        i += 7 if sym < 127 else 8
    return out


def decoy_c(stretch=STRETCH, n_tokens=300_000):
    """The member BEGINS with one dynamic block of 300 000 literals (fastq under the FLAT_LITLENS code: 260 KB of stream), and a few bytes
    behind the first stretch boundary its literals spell a dynamic block's header: the only candidate the probe finds in the block
    stands INSIDE it, no block boundary lies between the true start and the decoy, and the first unit of the first step has token
    room for one stretch and 300 000 tokens to decode.  zlib blocks to the end.  (raw, text, the decoy's BIT, its header's bits, decoy_block's argument)"""
    fq = texts()["fastq"]
    for at in range(1_000_000, 1_100_000, 3000):
        v, nbits, hdr = decoy_block(at)
        planted = spell(v, hdr + 64)
        if planted is not None:
            break
    assert planted is not None
    w = F.BitWriter()
    F.dynamic_header(w, FLAT_LITLENS, [0], plan=F.rle_greedy(FLAT_LITLENS + [0]))
    n1 = (8 * (stretch + 8) - w.bitpos() + 6) // 7
    toks = list(fq[2_000_000:2_000_000 + n1])
    assert max(toks) < 127
    lits = F.canonical(FLAT_LITLENS)
    F.emit_tokens(w, toks, lits, [None], eob=False)
    decoy_bit = w.bitpos()
    assert 8 * stretch < decoy_bit < 8 * (stretch + 16)
    rest = list(fq[2_000_000 + n1:2_000_000 + n_tokens - len(planted)])
    F.emit_tokens(w, planted + rest, lits, [None])
    text = bytearray(toks + planted + rest)
    text += recode(w, zlib_raw(fq[1_900_000:1_960_000]), final=True)
    return w.getvalue(), bytes(text), decoy_bit, hdr, at


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------
LIBDEFLATE_LEVELS = (1, 6, 9, 12)
GZIP_LEVELS = (1, 6, 9)
_CORPUS = None


def corpus():
    """[(name, raw, text, tags)].  The libdeflate cases (decoy (a) among them) are there when the library loads, GNU gzip's when the
    program is found; the zlib-built ones always."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    out = []
    for tname, text in texts().items():
        if libdeflate():
            for lv in LIBDEFLATE_LEVELS:
                out.append(("libdeflate %d, %s" % (lv, tname), libdeflate_raw(text, lv), text, dict(producer="libdeflate", level=lv, text=tname, needs="libdeflate")))
        raw = pigz_raw(text)
        out.append(("pigz shape, " + tname, raw, text, dict(producer="pigz", level=6, text=tname, needs=None, chunks=max(1, -(-len(text) // PIGZ_CHUNK)))))
        if gnu_gzip():
            for lv in GZIP_LEVELS:
                out.append(("GNU gzip -%d, %s" % (lv, tname), gnu_gzip_raw(text, lv), text, dict(producer="gzip", level=lv, text=tname, needs="gzip")))
    if libdeflate():
        raw, text, at = decoy_a(libdeflate_raw(texts()["fastq"][:300_000], 6))
        out.append(("decoy (a) in front of a libdeflate 6 block of 300 KB", raw, text, dict(producer="decoy", level=6, text="decoy", needs="libdeflate", decoy_byte=at)))
    raw, text, at = decoy_b()
    out.append(("decoy (b) behind the true start of a long run", raw, text, dict(producer="decoy", level=6, text="decoy", needs=None, decoy_byte=at)))
    raw, text, bit, hdr, src = decoy_c()
    out.append(("decoy (c) inside the block the member begins with", raw, text, dict(producer="decoy", level=6, text="decoy", needs=None, decoy_bit=bit, header_bits=hdr, decoy_source=src)))
    _CORPUS = out
    return out


def case(name_prefix):
    hits = [c for c in corpus() if c[0].startswith(name_prefix)]
    assert len(hits) == 1, (name_prefix, [c[0] for c in hits])
    return hits[0]


_BGZF = None


def bgzf_cases():
    """[(name, [(raw, text) per piece], tags)]: the first 300 000 bytes of the fastq in pieces of 65 280 and 4 000 bytes and the short text
    in pieces of 1 byte (the piece sizes of tests/test_gpu_inflate.py), every piece a stream of its own by libdeflate 1 / 6 / 9 / 12 and
    GNU gzip -1 / -6 / -9; two pieces of 65 280 bytes of fastq with 41 qualities by libdeflate; decoy (a) cut to one block's text."""
    global _BGZF
    if _BGZF is not None:
        return _BGZF
    out = []
    makers = []
    if libdeflate():
        makers += [("libdeflate %d" % lv, "libdeflate", lv, lambda t, lv=lv: libdeflate_raw(t, lv)) for lv in LIBDEFLATE_LEVELS]
    if gnu_gzip():
        makers += [("GNU gzip -%d" % lv, "gzip", lv, lambda t, lv=lv: gnu_gzip_raw(t, lv)) for lv in GZIP_LEVELS]
    wide = fastq(np.random.default_rng(20250612), 2 * BGZF_TEXT, n_qual=41)  # 41 qualities: more than 32 767 tokens in a block's text
    for tname, text, piece in (("fastq", texts()["fastq"][:300_000], BGZF_TEXT), ("fastq", texts()["fastq"][:300_000], 4000), ("short", texts()["short"], 1),
                               ("fastq, 41 qualities", wide, BGZF_TEXT)):
        parts = [text[a:a + piece] for a in range(0, len(text), piece)]
        for mname, needs, lv, make in makers:
            if tname == "fastq, 41 qualities" and needs != "libdeflate":
                continue
            out.append(("%s, %s in pieces of %d" % (mname, tname, piece), [(make(p), p) for p in parts], dict(producer=needs, level=lv, needs=needs, piece=piece, text=tname)))
    if libdeflate():
        lead = 2000
        room = BGZF_TEXT - lead - 16 - len(decoy_bytes())
        raw, text, at = decoy_a(libdeflate_raw(texts()["fastq"][:room], 6), lead_bytes=lead, stretch=0)
        assert len(text) == BGZF_TEXT
        out.append(("decoy (a) in one block", [(raw, text)], dict(producer="decoy", level=6, needs="libdeflate", piece=BGZF_TEXT, decoy_byte=at)))
    _BGZF = out
    return out


# ---- what a stream says (tests/test_host_producers.py) -----------------------------------------------------------------------------------
def long_codes(block):
    """literal/length + distance symbols with codes longer than 7 bits (deflate_forge's tag of the same name)"""
    return sum(1 for l in list(block.litlens) + list(block.distlens) if l > 7)


_SHAPES = {}


def shape(name, raw):
    """per stream, read once (the tokens themselves are not kept): its text and per block kind, final, bit_start, bit_end, text_start,
    text_len, tokens, max_dist (longest distance), long_codes, cross (matches that begin in one pigz chunk and reach into the one before)"""
    if name not in _SHAPES:
        text, blocks, _ = R.read_deflate(raw)
        _SHAPES[name] = (bytes(text), [dict(kind=b.kind, final=b.final, bit_start=b.bit_start, bit_end=b.bit_end, text_start=b.text_start, text_len=b.text_len,
                                           tokens=len(b.tokens), max_dist=max((t[4] for t in b.tokens), default=0),
                                           long_codes=long_codes(b) if b.kind == "dynamic" else 0,
                                           cross=sum(1 for t in b.tokens if t[4] > t[2] % PIGZ_CHUNK and t[2] >= PIGZ_CHUNK)) for b in blocks])
    return _SHAPES[name]
