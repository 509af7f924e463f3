"""Compressed inputs that span several uploads, for the tests of the pipeline's feeder and of its gzip bookkeeping (Feeder::one_file,
gz_append / gz_steps / top_up, drain_chunk in quade_amd/csrc/quade_pipe.cpp): texts(name, seed) -> a record_geometry.Profile, and
frame(framing, dir, seed) -> the conf's file lists.  An ordinary module: no test module imports another one.

A stream reaches the device in uploads of S = 16 MiB of the file's bytes (SEG_BYTES).  The oracle costs per pair and an upload costs
per byte, so the insert reads are long (20 000 and 10 000 bases) and drawn uniformly from bytes 33 .. 126: DEFLATE keeps 83 % of such
a text, and 1 600 pairs make 53 MB of seq_R1 (four uploads) and 27 MB of seq_R2 (two).  The index streams are record_geometry._chunk's:
pass, fail and Undetermined occur.  Three text sets:

  long        one chunk of N_LONG pairs, batch_pairs 97; the framings below
  ends_early  chunk 0: insert streams of three uploads each, index_R2 of 150 records (the chunk ends while uploads are in flight);
              chunk 1: 300 ordinary pairs.  Framings ends_early_gz, ends_early_bgzf
  dense       one chunk; seq_R1's reads are 60 000 x 'A' with quality 'I', so one upload of BGZF blocks holds more than SEG_TEXT_MAX =
              128 MiB of text and goes out in several segments.  Framing dense (BGZF)

Framings of `long` (the index streams are always small one-member or BGZF files):

  gz                one zlib level-6 member per stream
  bgzf              the library's own writer (record_geometry.write_text)
  gz_members        seq_R1 as six members whose FNAME lengths place the seams to the byte: a trailer that ends at S, an empty member at
                    S, deflate data that ends at 2S - 4 (CRC in front of the seam, ISIZE behind it), a header with FEXTRA, FNAME,
                    FCOMMENT and FHCRC that starts at 3S - 5, a member of 10 bytes of text, 4 096 zero bytes behind the last member;
                    seq_R2 as two members that meet inside the second upload
  bgzf_seams        seq_R1 block by block (zlib raw deflate of at most 60 000 bytes, deflate_forge.bgzf_block, a 'ZZ' subfield behind
                    'BC' sets a block's size): under the feeder's cuts (bgzf_cuts) a block ends at a buffer's end, one starts 7 bytes
                    before a buffer's end, one with an extra field of 200 bytes starts 100 bytes before a buffer's end; an empty block
                    in the middle and bgzip's EOF marker at the end
  bgzf_then_gz      seq_R1 as BGZF up to a block boundary behind S + 1 MiB, the rest of the text as one level-6 member
  gz_refused_late   seq_R2 as one member: zlib up to a full flush, then deflate_forge.forge_stream over the last FORGED_TEXT bytes,
                    which begins with a block no lane configuration decodes -- at a file offset behind S
  gz_damaged_late, bgzf_damaged_late   gz and bgzf with one byte of seq_R1's payload flipped between S + 1 MiB and 2S

Facts are counted from the files (members, bgzf_layout, bgzf_cuts, uploads), never from the builders' bookkeeping."""
import functools
import os
import zlib

import numpy as np

from tests import deflate_forge as F
from tests import record_geometry as G

S = 16 << 20              # SEG_BYTES: bytes per upload
SEG_TEXT_MAX = 128 << 20  # text of one BGZF segment at most
BATCH = 97
SETS = ("long", "ends_early", "dense")
N_LONG, N_EARLY, N_EARLY_INDEX_R2, N_EARLY_NEXT, N_DENSE = 1600, 1050, 150, 300, 1150
LEN_R1, LEN_R2, LEN_DENSE = 20000, 10000, 60000
BLOCK_TEXT = 60000        # text per hand-made BGZF block at most
FORGED_TEXT = 200_000     # gz_refused_late: the text behind the full flush
INSERTS = ("seq_R1", "seq_R2")
EOF_BLOCK = F.bgzf_block(b"\x03\x00", b"")  # bgzip's end-of-file marker: an empty block of 28 bytes
FRAMINGS = {"gz": "long", "bgzf": "long", "gz_members": "long", "bgzf_seams": "long", "bgzf_then_gz": "long", "gz_refused_late": "long",
            "gz_damaged_late": "long", "bgzf_damaged_late": "long", "ends_early_gz": "ends_early", "ends_early_bgzf": "ends_early", "dense": "dense"}


# ---- the texts ------------------------------------------------------------------------------------------------------------------
def _uniform(rng, n):
    return rng.integers(33, 127, n, dtype=np.uint8).tobytes()


def _inserts(rng, c, n, mean, read_no):
    """n records whose reads and qualities are mean +- 10 % bytes drawn uniformly from 33 .. 126"""
    out = []
    for i in range(n):
        L = int(rng.integers(mean - mean // 10, mean + mean // 10 + 1))
        out.append(G._record(G._plain_name(c, i), read_no, _uniform(rng, L), _uniform(rng, L)))
    return b"".join(out)


def _long(rng, samples):
    chunk = G._join(G._chunk(rng, samples, 0, N_LONG, len1=0, len2=0))
    chunk["seq_R1"] = _inserts(rng, 0, N_LONG, LEN_R1, b"1")
    chunk["seq_R2"] = _inserts(rng, 0, N_LONG, LEN_R2, b"2")
    return [chunk]


def _ends_early(rng, samples):
    c0 = G._join(G._chunk(rng, samples, 0, N_EARLY, len1=0, len2=0, counts={"index_R2": N_EARLY_INDEX_R2}))
    c0["seq_R1"] = _inserts(rng, 0, N_EARLY, LEN_R1, b"1")
    c0["seq_R2"] = _inserts(rng, 0, N_EARLY, LEN_R1, b"2")
    return [c0, G._join(G._chunk(rng, samples, 1, N_EARLY_NEXT))]


def _dense(rng, samples):
    chunk = G._join(G._chunk(rng, samples, 0, N_DENSE, len1=0))
    chunk["seq_R1"] = b"".join(G._record(G._plain_name(0, i), b"1", b"A" * LEN_DENSE, b"I" * LEN_DENSE) for i in range(N_DENSE))
    return [chunk]


_BUILDERS = {"long": _long, "ends_early": _ends_early, "dense": _dense}


@functools.lru_cache(maxsize=None)
def texts(name, seed=0):
    """the text set of that name as a record_geometry.Profile; the same texts for the same seed (cached: treat them as read-only, and
    call forget() when a module is done with them: they are large)"""
    rng = np.random.default_rng([100 + SETS.index(name), seed])
    samples = G._sheet(rng)
    p = G.Profile(name, seed, BATCH, _BUILDERS[name](rng, samples), samples)
    p.facts = G._facts(p)
    return p


def deflate6(text):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(text) + c.flush()


@functools.lru_cache(maxsize=None)
def _raw6(name, seed, c, k):
    return deflate6(texts(name, seed).chunks[c][k])


def forget():
    texts.cache_clear()
    _raw6.cache_clear()


# ---- the files ------------------------------------------------------------------------------------------------------------------
def _put(path, data):
    with open(path, "wb") as fh:
        fh.write(data)


def _get(path):
    with open(path, "rb") as fh:
        return fh.read()


def _paths(p, d):
    return {k: [os.path.join(str(d), "C%d_%s.fastq.gz" % (c, k)) for c in range(p.n_chunks)] for k in G.STREAMS}


def _write(p, d, fmt, streams=G.STREAMS):
    """the streams' files in record_geometry's formats, but a gz insert stream as a level-6 member (deflated once per process)"""
    files = _paths(p, d)
    for k in streams:
        for c, chunk in enumerate(p.chunks):
            if fmt == "gz" and k in INSERTS:
                _put(files[k][c], F.gzip_member(_raw6(p.name, p.seed, c, k), chunk[k]))
            else:
                G.write_text(files[k][c], chunk[k], fmt)
    return files


def _deflate_to(text, start, room):
    """level-6 raw DEFLATE of text[start:start + n], n chosen so that the stream is 1 .. 1 500 bytes shorter than `room`:
    (stream, n, bytes short).  The end is found by asking a copy of the compressor, 512 bytes of text at a time, what it would end in."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    out, size, at = [], 0, start
    while True:
        step = 65536 if size + 200_000 < room else 0
        if not step:
            end = c.copy().flush()
            short = room - size - len(end)
            assert short >= 1, (room, size, len(end))
            if short <= 1500:
                break
            step = 4096 if short > 20000 else 512
        assert at + step < len(text), "the text is too short for this member"
        out.append(c.compress(text[at:at + step]))
        size += len(out[-1])
        at += step
    return b"".join(out) + end, at - start, short


def _gz_members(p, d):
    files = _write(p, d, "gz", ("index_R1", "index_R2"))
    text = p.chunks[0]["seq_R1"]
    parts, pos, t = [], 0, 0

    def add(member):
        nonlocal pos
        parts.append(member)
        pos += len(member)

    def data_ends_at(end):  # a member whose header's FNAME is as long as it takes for its deflate data to end at that file offset
        nonlocal t
        raw, n, short = _deflate_to(text, t, end - pos - 10)
        add(F.gzip_member(raw, text[t:t + n], name=b"n" * (short - 1)))
        t += n
        assert pos == end + 8
    data_ends_at(S - 8)                       # the trailer ends at S
    add(F.gzip_member(deflate6(b""), b""))    # an empty member directly behind the seam
    data_ends_at(2 * S - 4)                   # CRC before 2S, ISIZE behind it
    data_ends_at(3 * S - 13)                  # ... so that the next header starts at 3S - 5 and straddles 3S
    add(F.gzip_member(deflate6(text[t:-10]), text[t:-10], extra=F.subfield(b"XY", b"abc"), name=b"reads.fastq", comment=b"this header straddles an upload",
                      hcrc=True))
    add(F.gzip_member(deflate6(text[-10:]), text[-10:]))
    _put(files["seq_R1"][0], b"".join(parts) + bytes(4096))
    text = p.chunks[0]["seq_R2"]
    cut = len(text) * 13 // 16
    _put(files["seq_R2"][0], F.gzip_member(deflate6(text[:cut]), text[:cut]) + F.gzip_member(deflate6(text[cut:]), text[cut:]))
    return files


def _block(part, after=b""):
    return F.bgzf_block(deflate6(part), part, after=after)


def _bgzf_seams(p, d):
    files = _write(p, d, "bgzf", ("seq_R2", "index_R1", "index_R2"))
    text = p.chunks[0]["seq_R1"]
    out, at, t = [], 0, 0  # file offset, text offset

    def put(block):
        nonlocal at
        out.append(block)
        at += len(block)

    def plain(n, after=b""):
        nonlocal t
        assert 0 < n <= BLOCK_TEXT and t + n < len(text)
        put(_block(text[t:t + n], after))
        t += n

    def land(T):  # blocks up to file offset T exactly: whole ones, one of half the rest, one padded with 'ZZ' to the byte
        while T - at > 100_000:
            plain(BLOCK_TEXT)
        plain(int((T - at) / 2 / 0.84))
        n = int((T - at - 2000) / 0.84)
        pad = T - at - len(_block(text[t:t + n])) - 4
        assert 0 <= pad < 8000, pad
        plain(n, F.subfield(b"ZZ", bytes(pad)))
        assert at == T
    land(S)                                          # a block ends exactly at the first buffer's end: the second covers [S, 2S)
    put(EOF_BLOCK)                                   # an empty block in the middle of the file
    land(2 * S - 7)
    plain(BLOCK_TEXT)                                # starts 7 bytes before the second buffer's end: the third covers [2S - 7, 3S - 7)
    land(3 * S - 7 - 100)
    plain(BLOCK_TEXT, F.subfield(b"ZZ", bytes(190)))  # XLEN 200, 100 of its bytes in the third buffer
    while t < len(text):
        n = min(BLOCK_TEXT, len(text) - t)
        put(_block(text[t:t + n]))
        t += n
    put(EOF_BLOCK)
    _put(files["seq_R1"][0], b"".join(out))
    return files


def _bgzf_then_gz(p, d):
    files = _write(p, d, "bgzf")
    path, text = files["seq_R1"][0], p.chunks[0]["seq_R1"]
    raw = _get(path)
    at, t = next((at, t) for at, _, _, t, _ in bgzf_layout(path) if at >= S + (1 << 20))
    _put(path, raw[:at] + F.gzip_member(deflate6(text[t:]), text[t:]))
    return files


def _gz_refused_late(p, d):
    files = _write(p, d, "gz", ("seq_R1", "index_R1", "index_R2"))
    text = p.chunks[0]["seq_R2"]
    n = len(text) - FORGED_TEXT
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(text[:n]) + c.flush(zlib.Z_FULL_FLUSH)  # byte-aligned, no final block, no history behind it
    _put(files["seq_R2"][0], F.gzip_member(raw + F.forge_stream(text[n:]), text))
    return files


def _flip(path, at):
    raw = bytearray(_get(path))
    raw[at] ^= 0x5A
    _put(path, bytes(raw))


def _gz_damaged_late(p, d):
    files = _write(p, d, "gz")
    _flip(files["seq_R1"][0], S + S // 2)
    return files


def _bgzf_damaged_late(p, d):
    files = _write(p, d, "bgzf")
    path = files["seq_R1"][0]
    at, size, xlen, _, _ = next(b for b in bgzf_layout(path) if b[0] + b[1] > S + S // 2)
    _flip(path, at + 12 + xlen + (size - 12 - xlen - 8) // 2)
    return files


def _dense_bgzf(p, d):
    files = _write(p, d, "bgzf", ("seq_R2", "index_R1", "index_R2"))
    text = p.chunks[0]["seq_R1"]
    _put(files["seq_R1"][0], b"".join(_block(text[a:a + BLOCK_TEXT]) for a in range(0, len(text), BLOCK_TEXT)) + EOF_BLOCK)
    return files


_FRAMERS = {"gz": lambda p, d: _write(p, d, "gz"), "bgzf": lambda p, d: _write(p, d, "bgzf"), "gz_members": _gz_members, "bgzf_seams": _bgzf_seams,
            "bgzf_then_gz": _bgzf_then_gz, "gz_refused_late": _gz_refused_late, "gz_damaged_late": _gz_damaged_late,
            "bgzf_damaged_late": _bgzf_damaged_late, "ends_early_gz": lambda p, d: _write(p, d, "gz"),
            "ends_early_bgzf": lambda p, d: _write(p, d, "bgzf"), "dense": _dense_bgzf}


def frame(framing, d, seed=0):
    """the framing's files under d: {stream: [path of chunk 0, ...]}, what run_support._conf takes"""
    return _FRAMERS[framing](texts(FRAMINGS[framing], seed), d)


# ---- what a file holds, from its bytes ------------------------------------------------------------------------------------------
def uploads(path):
    """uploads of an ordinary gzip file: the feeder sends it as it is, S bytes at a time"""
    return -(-os.path.getsize(path) // S)


def members(path):
    """([(header at, FLG, deflate data at, trailer at, text bytes)] of every gzip member of a file, the bytes behind the last one),
    by RFC 1952 and zlib's inflater"""
    raw = _get(path)
    out, at = [], 0
    while raw[at:at + 3] == b"\x1f\x8b\x08":
        flg, p = raw[at + 3], at + 10
        if flg & 4:
            p += 2 + int.from_bytes(raw[p:p + 2], "little")
        for bit in (8, 16):
            if flg & bit:
                p = raw.index(b"\0", p) + 1
        if flg & 2:
            p += 2
        d = zlib.decompressobj(-15)
        text = d.decompress(raw[p:])
        assert d.eof
        trailer = len(raw) - len(d.unused_data)
        assert int.from_bytes(raw[trailer:trailer + 4], "little") == zlib.crc32(text) and int.from_bytes(raw[trailer + 4:trailer + 8], "little") == len(text)
        out.append((at, flg, p, trailer, len(text)))
        at = trailer + 8
    return out, raw[at:]


def bgzf_layout(path, upto=None):
    """[(block at, bytes, XLEN, first text byte, text bytes)] of the BGZF blocks at the head of a file (all of it, or it ends where
    no block starts), from their BSIZE and ISIZE fields; other subfields may stand behind 'BC'"""
    raw = _get(path)
    out, at, t = [], 0, 0
    while at < len(raw) and raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00":
        size = int.from_bytes(raw[at + 16:at + 18], "little") + 1
        isize = int.from_bytes(raw[at + size - 4:at + size], "little")
        out.append((at, size, int.from_bytes(raw[at + 10:at + 12], "little"), t, isize))
        t += isize
        at += size
    return out


def bgzf_cuts(path):
    """A model of the feeder's cuts (feed::Cutter, quade_amd/csrc/feed_cut.h): buffer k covers the file's bytes [pos_k, pos_k + S), and pos_k+1 is the start
    of the first block that is not wholly inside it.  [(pos_k, [blocks wholly inside buffer k])] up to the end of the file's blocks"""
    blocks = bgzf_layout(path)
    out, i = [], 0
    while i < len(blocks):
        pos, j = blocks[i][0], i
        while j < len(blocks) and blocks[j][0] + blocks[j][1] <= pos + S:
            j += 1
        assert j > i
        out.append((pos, blocks[i:j]))
        i = j
    return out
