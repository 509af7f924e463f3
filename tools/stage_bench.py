#!/usr/bin/env python3
"""Cost of one read stage's kernel over resident text: one batch of the device pipeline -- 2 M pairs of 2 x 150 bp insert reads
as fastq text in HBM with their record tables (and routing codes) -- worked on by the kernel qd_pipe_run launches, through the
pipeline's internal entry qd_<stage>_device.  Several contexts on one device take the same batch: one with the stage off, one
with it on, and for some stages one that runs a comparison kernel; their calls alternate on one stream (off, on, off, on, ...) and
each is timed by HIP events.  "off" does what process_batch does with the stage off, launches nothing and shows what the timing
itself costs.  After the timed steps the stage's table is read back and checked against what the batch must have counted.  Prints
one JSON line ("tool": "<stage>_bench"): per case the medians, the spread and the byte floor (the lines' bytes at 6.3 TB/s).

usage: python tools/stage_bench.py --stage qstats|cycle|clip|trim|pairtrim|paircorrect|posttrim|filter|screen|dup|adapters [--pairs N] [--bases L] [--steps K] [--warmup W]
                                   [--once CASE] [--out FILE]
  --once CASE  set up, run ONE launch and exit (for `rocprofv3 --kernel-trace --stats -- python ...`); CASE by stage:
    qstats    hot | spread | off      routing: 96 samples with 90 % of the pairs to 8 destinations (per-workgroup partials in LDS) |
                                      4 000 samples, uniform (64-bit global atomics); off: the context with the table off
    cycle     pass | mix | long | off every pair to a pass file | a third each to pass, fail, Undetermined | reads of 2 x --bases;
                                      interleaved with the quality counters' kernel over the same batch
    clip      CASE:PCT                yardstick | window | poly_g | all, over a batch with PCT % of the reads ending in 30 G; the
                                      yardstick is the 3' trimming kernel with a cutoff only
    trim      PCT                     PCT % of the reads carry their adapter from a random position on
    pairtrim  PCT | poly              PCT % of the pairs read from an insert of 30 .. --bases - 1 bases | poly-A against poly-T
    paircorrect PCT | unresolved      PCT % of the pairs read from a short insert, about 1 % of the overlap positions a Q2 call in R2
                                      against Q37 in R1 | every pair from a short insert and both calls at Q37 (nothing to write);
                                      interleaved with the pairtrim kernel, with and without the hand-over of I*, over the same batch
    posttrim  CASE:PCT                clip_poly_g | polyx | crop | all, over a batch with PCT % of the reads ending in 30 A;
                                      clip_poly_g is the clip kernel with its poly-G rule alone over the same share of G tails
    filter    drop0 | drop10 | drop100 | spread | off   the share of pairs dropped (poly-G in R1), hot or spread routing;
                                      interleaved with the quality counters' kernel over the same batch
    screen    lds_PCT | ldscap_PCT | globaledge_PCT | global_PCT | off   the k-mer screen against a PhiX-sized random reference
                                      (5 386 bases, the hash table in LDS), one of 6 144 k-mers (the fullest LDS table), of 6 145 (the
                                      smallest table in global memory) or of 200 000, PCT (0 | 10 | 100) % of the pairs drawn from
                                      the reference; interleaved with the quality counters' and the pairtrim kernel
    dup       sSAMPLE_dPCT | off      the duplication tally with duplication_sample SAMPLE (16 | 1) over a batch in which PCT (0 |
                                      30 | 100) % of the pairs repeat another pair's reads and destination, 8 hot destinations;
                                      interleaved with the quality counters' kernel over the same batch
    adapters  pN_PCT | off            the adapter content with N (6 | 16) probes in force over a batch in which PCT (0 | 10 | 100) % of the
                                      reads carry the Illumina universal adapter from a random position on; interleaved with the
                                      quality counters' kernel over the same batch
The end-to-end rates come from tools/e2e_bench.py with the stage's E2E_* switch against none."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from quade_amd import hip_backend as hb  # noqa: E402

COPY_RATE = 6.3e12  # bytes/s an MI355X copies at (measured float4 copy)
ADAPTERS = ("AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")
G_TAIL = 30
PLAN = hb.make_plan(True, 25, (0, 8), (0, 8))


# ---- the batch: resident text, record tables, routing codes -----------------------------------------------------------------------
def generator(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def plain_seq(g, n, L):
    """bases with an N in 16"""
    return torch.tensor(list(b"ACGTACGTACGTACGN"), dtype=torch.uint8, device="cuda")[torch.randint(0, 16, (n, L), generator=g, device="cuda")]


def plain_qual(g, n, L):
    """Phred 2 .. 40"""
    return torch.randint(35, 74, (n, L), generator=g, device="cuda", dtype=torch.uint8)


def make_text(n, L, seed, plant=None):
    """n records "@<20-byte name>\\n<L bases>\\n+\\n<L qualities>\\n" on the device, their record table (6 uint32 each) and a record's
    bytes.  plant(g, n, L) -> (bases, qualities) uint8[n, L] is what a stage puts into the reads (adapters, G tails, short inserts),
    drawn from the text's generator behind the names; None: plain_seq and plain_qual."""
    g = generator(seed)
    rec = 1 + 20 + 1 + L + 1 + 2 + L + 1
    t = torch.empty((n, rec), dtype=torch.uint8, device="cuda")
    t[:, 0] = ord("@")
    t[:, 1:21] = torch.randint(48, 58, (n, 20), generator=g, device="cuda", dtype=torch.uint8)
    t[:, 22:22 + L], t[:, 25 + L:25 + 2 * L] = plant(g, n, L) if plant else (plain_seq(g, n, L), plain_qual(g, n, L))
    t[:, 21] = t[:, 22 + L] = t[:, 24 + L] = t[:, 25 + 2 * L] = 10
    t[:, 23 + L] = ord("+")
    head = torch.arange(n, device="cuda", dtype=torch.int64) * rec
    recs = torch.stack([head, head + 1, torch.full_like(head, 20), head + 22, torch.full_like(head, L), head + 25 + L], dim=1)
    assert n * rec < 1 << 31
    return t.reshape(-1), recs.to(torch.int32).contiguous(), rec


class Batch(object):
    """R1 and R2 texts (seeds s1, s2; plant per read: plants[r]) with their tables, and tables for a stage's output"""

    def __init__(self, n, L, s1=1, s2=2, plants=(None, None)):
        self.n, self.L = n, L
        self.t1, self.r1, self.rec = make_text(n, L, s1, plants[0])
        self.t2, self.r2, _ = make_text(n, L, s2, plants[1])

    def outputs(self):
        self.o1, self.o2 = torch.empty_like(self.r1), torch.empty_like(self.r2)
        return self.o1.data_ptr(), self.o2.data_ptr()

    def kept_whole(self):
        """a stage that writes new tables changed nothing but the lengths, and lengthened no read"""
        return bool((self.o1[:, [0, 1, 2, 3, 5]] == self.r1[:, [0, 1, 2, 3, 5]]).all()) and int(self.o1[:, 4].max()) <= self.L


def routed_codes(g, n, name):
    """-> (samples, routing codes): hot = 96 samples, 90 % of the pairs to 8 destinations; spread = 4 000 samples, uniform over the
    8 001 destinations"""
    S = 96 if name == "hot" else 4000
    codes = torch.randint(0, 2 * S + 1, (n,), generator=g, device="cuda")
    if name == "hot":
        hot = torch.rand(n, generator=g, device="cuda") < 0.9
        codes[hot] = torch.randint(0, 8, (int(hot.sum()),), generator=g, device="cuda") * 2
    codes[codes == 2 * S] = 0xFFFF
    return S, codes.to(torch.int16).contiguous()


def contexts(kinds, S=None):
    """{name: a context set up by kinds[name](engine) (None: left as it is)}, in kinds' order; S: with the plan and S barcodes"""
    engines = {}
    for k, setup in kinds.items():
        eng = hb.Engine(0)
        if S is not None:
            eng.set_plan(PLAN)
            eng.set_barcodes(["".join("ACGT"[(i >> (2 * j)) & 3] for j in range(16)) for i in range(S)])
        if setup:
            setup(eng)
        engines[k] = eng
    return engines


def close(engines):
    for eng in engines.values():
        eng.close()


# ---- launching and timing -----------------------------------------------------------------------------------------------------------
class Bench(object):
    def __init__(self, a):
        self.a, self.lib, self.st = a, hb.load_library(), torch.cuda.current_stream()

    def entry(self, name):
        """the pipeline's internal entry qd_<name>_device: a context, device pointers of the batch, two more and a stream"""
        f = getattr(self.lib, "qd_%s_device" % name)
        f.restype, f.argtypes = C.c_int, [C.c_void_p] * 5 + [C.c_uint32] + [C.c_void_p] * 3
        return f

    def asker(self, name):
        """qd_<name>_active: what process_batch asks before it launches"""
        f = getattr(self.lib, "qd_%s_active" % name)
        f.restype, f.argtypes = C.c_int, [C.c_void_p]
        return f

    def launch(self, f, eng, b, x, y):
        rc = f(eng._h, b.t1.data_ptr(), b.r1.data_ptr(), b.t2.data_ptr(), b.r2.data_ptr(), b.n, x, y, self.st.cuda_stream)
        assert rc == 0, rc

    def timed(self, run):
        """run: {name: launcher}, called in this order in every step, each between two events -> {name: sorted milliseconds}"""
        for _ in range(self.a.warmup):
            for f in run.values():
                f()
        ev = {k: [] for k in run}
        for _ in range(self.a.steps):
            for k, f in run.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.st)
                f()
                e1.record(self.st)
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        return {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}

    def once_in(self, values):
        if self.a.once not in values:
            sys.exit("--once for --stage %s: %s" % (self.a.stage, " | ".join(v for v in values if v)))

    def once(self, f, result):
        f()
        torch.cuda.synchronize()
        return result

    def floor_ms(self, lines, L=None):
        """reading `lines` lines of every pair once at COPY_RATE"""
        return float(lines) * self.a.pairs * (L or self.a.bases) / COPY_RATE * 1e3

    def head(self, tool, **more):
        out = {"tool": tool, "device": torch.cuda.get_device_name(0), "pairs_per_launch": self.a.pairs, "bases_per_read": self.a.bases}
        out.update(more)
        return out


def median(v):
    return v[len(v) // 2]


def off_on(ms):
    return {"off_median_ms": median(ms["off"]), "on_median_ms": median(ms["on"]), "off_min_ms": ms["off"][0], "off_max_ms": ms["off"][-1],
            "on_min_ms": ms["on"][0], "on_max_ms": ms["on"][-1]}


def by_name(ms):
    out = {}
    for k, v in ms.items():
        out.update({k + "_median_ms": median(v), k + "_min_ms": v[0], k + "_max_ms": v[-1]})
    return out


# ---- the stages: their cases, launchers and the checks on the table ---------------------------------------------------------------
def qstats(B):
    a, n, L = B.a, B.a.pairs, B.a.bases
    B.once_in((None, "hot", "spread", "off"))
    launch, b, g = B.entry("qstats"), Batch(n, L), generator(7)

    def measure(name):
        S, codes = routed_codes(g, n, name)
        engines = contexts({"off": None, "on": lambda e: e.qstats_enable(True)}, S)
        run = {k: (lambda k=k: B.launch(launch, engines[k], b, codes.data_ptr(), None)) for k in engines}  # (no drop bytes)
        if a.once:
            return B.once(run["off" if a.once == "off" else "on"], {"once": a.once, "pairs": n, "bases": L, "path": engines["on"].qstats_kind()})
        ms = B.timed(run)
        table, launches = engines["on"].qstats_read(), a.steps + a.warmup
        assert int(table[:, 0, 0].sum()) == launches * n and int(table[:, :, 1].sum()) == 2 * launches * n * L
        out = {"routing": name, "samples": S, "path": engines["on"].qstats_kind(), **off_on(ms), "byte_floor_ms": B.floor_ms(4),
               "busiest_destination_share": float(table[:, 0, 0].max()) / (launches * n)}
        close(engines)
        return out

    if a.once:
        return measure("hot" if a.once == "off" else a.once)
    return B.head("qstats_bench", text_bytes=2 * n * b.rec, line_bytes=4 * n * L, steps=a.steps, hot=measure("hot"), spread=measure("spread"))


def cycle(B):
    a, n, S = B.a, B.a.pairs, 96
    cases = {"pass": ("pass", 1), "mix": ("mix", 1), "long": ("pass", 2)}  # routing, read length in units of --bases
    B.once_in([None, "off"] + sorted(cases))
    launch, g = {"off": B.entry("cstats"), "cycle": B.entry("cstats"), "qstats": B.entry("qstats")}, generator(7)
    kinds = {"off": None, "cycle": lambda e: e.cstats_enable(True), "qstats": lambda e: e.qstats_enable(True)}

    def measure(case):
        route, mult = cases[case]
        L = a.bases * mult
        b = Batch(n, L)
        codes = torch.randint(0, S, (n,), generator=g, device="cuda") * 2  # pass
        if route == "mix":
            third = torch.randint(0, 3, (n,), generator=g, device="cuda")
            codes[third == 1] += 1
            codes[third == 2] = 0xFFFF
        codes = codes.to(torch.int16).contiguous()
        engines = contexts({k: kinds[k] for k in (("off",) if a.once == "off" else ("cycle",) if a.once else kinds)}, S)
        # "off": what process_batch does with the table off -- the same call, which launches nothing
        run = {k: (lambda k=k: B.launch(launch[k], engines[k], b, codes.data_ptr(), None)) for k in engines}
        if a.once:
            out = B.once(run["off" if a.once == "off" else "cycle"], {"once": a.once, "pairs": n, "bases": L})
            close(engines)
            return out
        ms = B.timed(run)
        launches = a.steps + a.warmup
        t, q = engines["cycle"].cstats_read(), engines["qstats"].qstats_read()
        assert int(t["len"].sum()) == 2 * launches * n and int(t["len"][:, :, L].sum()) == 2 * launches * n  # the one hot length bin
        groups = [int(t["len"][k].sum()) for k in range(3)]
        assert (groups[1] == groups[2] == 0) if route == "pass" else min(groups) > 0.3 * 2 * launches * n
        for k, col in ((4, 5), (5, 2), (6, 3), (7, 4)):  # N, qual_sum, q20, q30 against the quality counters of the same batch
            assert int(t["cycle"][:, :, :, k].sum()) == int(q[:, :, col].sum()), (k, col)
        floor = B.floor_ms(4, L)
        out = {"case": case, "samples": S, "bases_per_read": L, "byte_floor_ms": floor,
               "cycle_over_qstats": median(ms["cycle"]) / median(ms["qstats"]), "cycle_over_floor": median(ms["cycle"]) / floor, **by_name(ms)}
        close(engines)
        return out

    if a.once:
        return measure("pass" if a.once == "off" else a.once)
    out = B.head("cycle_bench", steps=a.steps, lds_cycles=B.lib.qd_cstats_lds_cycles())
    for case in cases:
        out[case] = measure(case)
    return out


def g_tails(share):
    """a `share` of the reads ends in G_TAIL bases G; qualities 30 .. 40, on half the reads a 3' tail of 0 .. 40 bases at 2 .. 19 (not
    under a G tail: a dark cluster reads as high-quality G)"""
    def plant(g, n, L):
        seq = plain_seq(g, n, L)
        col = torch.arange(L, device="cuda").reshape(1, L)
        has = (torch.rand(n, generator=g, device="cuda") < share).reshape(n, 1)
        seq = torch.where(has & (col >= L - G_TAIL), torch.full_like(seq, ord("G")), seq)
        qual = torch.randint(33 + 30, 33 + 41, (n, L), generator=g, device="cuda", dtype=torch.uint8)
        low = torch.randint(33 + 2, 33 + 20, (n, L), generator=g, device="cuda", dtype=torch.uint8)
        tail = torch.randint(0, 41, (n, 1), generator=g, device="cuda") * (torch.rand(n, 1, generator=g, device="cuda") < 0.5)
        return seq, torch.where(~has & (col >= L - tail), low, qual)
    return plant


def clip(B):
    a, n, L = B.a, B.a.pairs, B.a.bases
    launch = {"yardstick": B.entry("trim"), "window": B.entry("clip"), "poly_g": B.entry("clip"), "all": B.entry("clip")}
    engines = contexts({"yardstick": lambda e: e.trim_set(quality_cutoff=20), "window": lambda e: e.clip_set(window_size=4, window_quality=20),
                        "poly_g": lambda e: e.clip_set(poly_g_min_length=10),
                        "all": lambda e: e.clip_set(tail_clip_r1=1, tail_clip_r2=1, window_size=4, window_quality=20, poly_g_min_length=10)})
    floor = B.floor_ms(4)

    def measure(pct, only=None):
        b = Batch(n, L, plants=(g_tails(pct / 100.0),) * 2)
        o1, o2 = b.outputs()
        run = {k: (lambda k=k: B.launch(launch[k], engines[k], b, o1, o2)) for k in engines}
        if only is not None:
            return B.once(run[only], {"once": only, "g_tail_percent": pct, "pairs": n, "bases": L})
        for eng in engines.values():
            eng.reset_counts()
        ms = B.timed(run)
        runs = a.steps + a.warmup
        out = {"g_tail_percent": pct, "byte_floor_ms": floor, "cases": {}}
        for k in engines:
            table = engines[k].trim_read() if k == "yardstick" else engines[k].clip_read()
            assert int(table[0, 0]) == int(table[1, 0]) == runs * n and int(table[:, 1].sum()) == 2 * runs * n * L
            per = lambda c: float(table[:, c].sum()) / (2 * runs * n)  # noqa: E731
            row = {"median_ms": median(ms[k]), "min_ms": ms[k][0], "max_ms": ms[k][-1], "over_yardstick": median(ms[k]) / median(ms["yardstick"]),
                   "over_floor": median(ms[k]) / floor, "mean_bases_out": per(2)}
            if k != "yardstick":
                row.update(window_read_share=per(7), polyg_read_share=per(9))
            out["cases"][k] = row
        return out

    if a.once is not None:
        case, pct = a.once.split(":")
        assert case in engines, "--once yardstick|window|poly_g|all:PCT"
        return measure(int(pct), only=case)
    out = B.head("clip_bench", line_bytes=4 * n * L, steps=a.steps, yardstick="trim_reads, quality_cutoff 20, no adapter",
                 params={k: engines[k].clip_get() for k in list(engines)[1:]}, batches=[measure(pct) for pct in (0, 10, 100)])
    close(engines)
    return out


def adapters(adapter, share, whole=None):
    """a `share` of the reads holds the adapter (cut at the read's end) from a random position on; whole: a list that receives, per
    text made, the reads that hold the adapter's first 12 bases whole"""
    def plant(g, n, L):
        seq, held = plain_seq(g, n, L), 0
        if share > 0:
            ad = torch.tensor(list(adapter.encode()), dtype=torch.uint8, device="cuda")
            has = torch.rand(n, generator=g, device="cuda") < share
            p = torch.randint(0, L, (n, 1), generator=g, device="cuda")
            col = torch.arange(L, device="cuda").reshape(1, L)
            inside = has.reshape(n, 1) & (col >= p) & (col < p + len(ad))
            seq = torch.where(inside, ad[(col - p).clamp(0, len(ad) - 1)], seq)
            held = int((has & (p[:, 0] <= L - 12)).sum())
        if whole is not None:
            whole.append(held)
        return seq, plain_qual(g, n, L)
    return plant


def rewriting(B, name, engines, b):
    """{off, on} launchers of a stage that writes new record tables (trim, pairtrim) as process_batch runs it: it asks whether the
    stage is on and launches only then"""
    launch, active, (o1, o2) = B.entry(name), B.asker(name), b.outputs()
    return {k: (lambda k=k: B.launch(launch, engines[k], b, o1, o2) if active(engines[k]._h) else None) for k in engines}


def trim(B):
    a, n, L = B.a, B.a.pairs, B.a.bases
    engines = contexts({"off": None, "on": lambda e: e.trim_set(ADAPTERS[0], ADAPTERS[1], quality_cutoff=20)})
    floor = B.floor_ms(4)

    def measure(pct):
        b = Batch(n, L, plants=(adapters(ADAPTERS[0], pct / 100.0), adapters(ADAPTERS[1], pct / 100.0)))
        run = rewriting(B, "trim", engines, b)
        if a.once is not None:
            return B.once(run["on"], {"once": pct, "pairs": n, "bases": L})
        engines["on"].reset_counts()
        ms = B.timed(run)
        table, launches = engines["on"].trim_read(), a.steps + a.warmup
        assert int(table[0, 0]) == int(table[1, 0]) == launches * n and int(table[:, 1].sum()) == 2 * launches * n * L
        assert b.kept_whole()
        per = lambda k: float(table[:, k].sum()) / (2 * launches * n)  # noqa: E731
        return {"adapter_percent": pct, **off_on(ms), "byte_floor_ms": floor, "on_over_floor": median(ms["on"]) / floor,
                "quality_trimmed_read_share": per(3), "adapter_read_share": per(5), "mean_bases_out": per(2)}

    if a.once is not None:
        return measure(int(a.once))
    out = B.head("trim_bench", line_bytes=4 * n * L, steps=a.steps, params=engines["on"].trim_get(),
                 batches=[measure(pct) for pct in (0, 10, 100)])
    close(engines)
    return out


def insert_pairs(n, L, seed, case):
    """-> (R1, R2) base codes [n, L] on the device (0 .. 3 = A C G T); case: the percentage of pairs read from an insert of
    30 .. L - 1 bases, or "poly" """
    g = generator(seed)
    if case == "poly":
        return torch.zeros((n, L), dtype=torch.int64, device="cuda"), torch.full((n, L), 3, dtype=torch.int64, device="cuda")
    frag = torch.randint(0, 4, (n, L), generator=g, device="cuda")
    r1 = frag.clone()
    r2 = torch.randint(0, 4, (n, L), generator=g, device="cuda")
    if case > 0:
        short = torch.rand(n, generator=g, device="cuda") < case / 100.0
        insert = torch.randint(30, L, (n, 1), generator=g, device="cuda")
        col = torch.arange(L, device="cuda").reshape(1, L)
        inside = short.reshape(n, 1) & (col < insert)
        rc = 3 - torch.gather(frag, 1, (insert - 1 - col).clamp(0, L - 1))
        r2 = torch.where(inside, rc, r2)
        r1 = torch.where(short.reshape(n, 1) & (col >= insert), torch.randint(0, 4, (n, L), generator=g, device="cuda"), r1)
    return r1, r2


def pairtrim(B):
    a, n, L = B.a, B.a.pairs, B.a.bases
    engines = contexts({"off": None, "on": lambda e: e.pairtrim_set()})
    floor = B.floor_ms(2)
    acgt = lambda codes: lambda g, n_, L_: (torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[codes], plain_qual(g, n_, L_))  # noqa: E731

    def measure(case):
        c1, c2 = insert_pairs(n, L, 1, case)
        b = Batch(n, L, 2, 3, plants=(acgt(c1), acgt(c2)))
        del c1, c2
        run = rewriting(B, "pairtrim", engines, b)
        if a.once is not None:
            return B.once(run["on"], {"once": case, "pairs": n, "bases": L})
        engines["on"].reset_counts()
        ms = B.timed(run)
        reads, pairs, hist = hb.split_pairtrim(engines["on"].pairtrim_read())
        launches = a.steps + a.warmup
        assert pairs[0] == reads[0][0] == reads[1][0] == launches * n and reads[0][1] == reads[1][1] == launches * n * L
        assert sum(hist) == pairs[1] and b.kept_whole()
        if case != "poly":  # an unrelated pair is next to never accepted, an insert always found
            assert abs(pairs[2] / pairs[0] - case / 100.0) < 0.01, pairs
        return {"case": case, **off_on(ms), "byte_floor_ms": floor, "on_over_floor": median(ms["on"]) / floor,
                "overlapped_pair_share": pairs[1] / pairs[0], "short_insert_pair_share": pairs[2] / pairs[0],
                "mean_bases_out": (reads[0][2] + reads[1][2]) / (2.0 * pairs[0])}

    if a.once is not None:
        out = measure(a.once if a.once == "poly" else int(a.once))
    else:
        out = B.head("pairtrim_bench", line_bytes=2 * n * L, steps=a.steps, params=engines["on"].pairtrim_get(),
                     batches=[measure(case) for case in (0, 10, 100, "poly")])
    close(engines)
    return out


def paircorrect(B):
    """The overlap base correction beside the overlap kernel that feeds it, over the same batch in the same step: pairtrim as every
    run launches it, pairtrim storing every pair's I* (the hand-over), then the correction.  The texts are put back before every step
    (untimed): a corrected batch holds nothing to write."""
    a, n, L = B.a, B.a.pairs, B.a.bases
    engines = contexts({"pairtrim": lambda e: e.pairtrim_set(), "on": lambda e: (e.pairtrim_set(), e.paircorrect_set())})
    floor = B.floor_ms(2)
    lib, st = B.lib, B.st.cuda_stream
    pt = B.entry("pairtrim")
    pti = lib.qd_pairtrim_device_inserts
    pti.restype, pti.argtypes = C.c_int, [C.c_void_p] * 5 + [C.c_uint32] + [C.c_void_p] * 4
    pc = lib.qd_paircorrect_device
    pc.restype, pc.argtypes = C.c_int, [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p]
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")

    def measure(case):
        pct, good2 = (100, True) if case == "unresolved" else (case, False)
        c1, c2 = insert_pairs(n, L, 1, pct)
        g = generator(11)
        # a wrong call in one position of R2 in a hundred (over the whole read: those outside an overlap change nothing here)
        wrong = torch.rand((n, L), generator=g, device="cuda") < 0.01
        c2e = torch.where(wrong, (c2 + torch.randint(1, 4, (n, L), generator=g, device="cuda")) % 4, c2)
        q1 = torch.full((n, L), 33 + 37, dtype=torch.uint8, device="cuda")
        q2 = q1 if good2 else torch.where(wrong, torch.full_like(q1, 33 + 2), q1)
        b = Batch(n, L, 2, 3, plants=(lambda g_, n_, L_: (letters[c1], q1), lambda g_, n_, L_: (letters[c2e], q2)))
        del c1, c2, c2e, wrong, q1, q2
        keep1, keep2 = b.t1.clone(), b.t2.clone()
        o1, o2 = b.outputs()
        inserts = torch.zeros(n, dtype=torch.int64, device="cuda")
        args = (b.t1.data_ptr(), b.r1.data_ptr(), b.t2.data_ptr(), b.r2.data_ptr())

        def check(rc):
            assert rc == 0, rc

        run = {"pairtrim": lambda: check(pt(engines["pairtrim"]._h, *args, n, o1, o2, st)),
               "pairtrim_inserts": lambda: check(pti(engines["on"]._h, *args, n, o1, o2, inserts.data_ptr(), st)),
               "paircorrect": lambda: check(pc(engines["on"]._h, *args, inserts.data_ptr(), n, st))}
        if a.once is not None:
            run["pairtrim_inserts"]()
            return B.once(run["paircorrect"], {"once": case, "pairs": n, "bases": L})
        for eng in engines.values():
            eng.reset_counts()
        ev = {k: [] for k in run}
        for step in range(a.warmup + a.steps):
            b.t1.copy_(keep1)
            b.t2.copy_(keep2)
            for k, f in run.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(B.st)
                f()
                e1.record(B.st)
                if step >= a.warmup:
                    ev[k].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}
        t = [int(x) for x in engines["on"].paircorrect_read()]
        launches = a.steps + a.warmup
        reads, pairs, _ = hb.split_pairtrim(engines["on"].pairtrim_read())
        assert t[4] == launches * n == pairs[0] and t[5] == pairs[1] and t[7] == t[1] + t[3] + t[8] and b.kept_whole()
        # R1 is never the doubtful read; Q37 against Q37 stays; a Q2 call is corrected (but for the rare pair accepted at another insert)
        assert t[1] == 0 and (t[3] == 0 and t[8] > 0 if good2 else t[8] * 1000 <= t[7])
        assert bool((b.t1 == keep1).all()) and (good2 or pct == 0 or not bool((b.t2 == keep2).all()))
        return {"case": case, "byte_floor_ms": floor, **by_name(ms), "paircorrect_over_pairtrim": median(ms["paircorrect"]) / median(ms["pairtrim"]),
                "paircorrect_over_floor": median(ms["paircorrect"]) / floor,
                "hand_over_store_ms": median(ms["pairtrim_inserts"]) - median(ms["pairtrim"]),
                "overlapped_pair_share": t[5] / t[4], "overlap_bases_per_pair": t[6] / t[4], "mismatches_per_launch": t[7] / launches,
                "corrected_bases_per_launch": t[3] / launches, "unresolved_per_launch": t[8] / launches, "corrected_pairs_per_launch": t[9] / launches}

    if a.once is not None:
        out = measure(a.once if a.once == "unresolved" else int(a.once))
    else:
        out = B.head("paircorrect_bench", line_bytes=2 * n * L, steps=a.steps, params=engines["on"].paircorrect_get(),
                     pair_params=engines["on"].pairtrim_get(), batches=[measure(case) for case in (0, 10, 100, "unresolved")])
    close(engines)
    return out


def x_tails(share, base):
    """a `share` of the reads ends in G_TAIL times `base`; plain qualities"""
    def plant(g, n, L):
        seq = plain_seq(g, n, L)
        col = torch.arange(L, device="cuda").reshape(1, L)
        has = (torch.rand(n, generator=g, device="cuda") < share).reshape(n, 1)
        return torch.where(has & (col >= L - G_TAIL), torch.full_like(seq, ord(base)), seq), plain_qual(g, n, L)
    return plant


def posttrim(B):
    """The post-trim kernel's cases over a batch with PCT % of the reads ending in 30 A, beside the clip stage's poly-G-only case
    over the same batch with G in place of A (the two kernels stage the same line and walk the same rounds).  The byte floor: the
    records in and out and the sequence line of every read."""
    a, n, L = B.a, B.a.pairs, B.a.bases
    kinds = {"clip_poly_g": lambda e: e.clip_set(poly_g_min_length=10), "polyx": lambda e: e.posttrim_set(poly_x_min_length=10),
             "crop": lambda e: e.posttrim_set(max_length_r1=100, max_length_r2=100),
             "all": lambda e: e.posttrim_set(tail_n=1, poly_x_min_length=10, max_length_r1=140, max_length_r2=140)}
    launch = {k: B.entry("clip" if k == "clip_poly_g" else "posttrim") for k in kinds}
    engines = contexts(kinds)
    floor = 2.0 * n * (2 * 24 + L) / COPY_RATE * 1e3

    def measure(pct, only=None):
        b = Batch(n, L, plants=(x_tails(pct / 100.0, "A"),) * 2)
        bg = Batch(n, L, plants=(x_tails(pct / 100.0, "G"),) * 2)
        o1, o2 = b.outputs()
        run = {k: (lambda k=k: B.launch(launch[k], engines[k], bg if k == "clip_poly_g" else b, o1, o2)) for k in engines}
        if only is not None:
            return B.once(run[only], {"once": only, "a_tail_percent": pct, "pairs": n, "bases": L})
        for eng in engines.values():
            eng.reset_counts()
        ms = B.timed(run)
        runs = a.steps + a.warmup
        out = {"a_tail_percent": pct, "byte_floor_ms": floor, "cases": {}}
        for k in engines:
            table = engines[k].clip_read() if k == "clip_poly_g" else engines[k].posttrim_read()
            assert int(table[0, 0]) == int(table[1, 0]) == runs * n and int(table[:, 1].sum()) == 2 * runs * n * L
            per = lambda c: float(table[:, c].sum()) / (2 * runs * n)  # noqa: E731
            row = {"median_ms": median(ms[k]), "min_ms": ms[k][0], "max_ms": ms[k][-1], "over_clip_poly_g": median(ms[k]) / median(ms["clip_poly_g"]),
                   "over_floor": median(ms[k]) / floor, "mean_bases_out": per(2)}
            if k == "clip_poly_g":
                row.update(polyg_read_share=per(9))
                assert abs(per(9) - pct / 100.0) < 0.01
            else:
                row.update(n_tail_read_share=per(3), polya_read_share=per(5), cropped_read_share=per(13))
                assert k == "crop" or abs(per(5) - pct / 100.0) < 0.01  # a planted tail is always found, a random one next to never
            out["cases"][k] = row
        return out

    if a.once is not None:
        case, pct = a.once.split(":")
        assert case in engines, "--once clip_poly_g|polyx|crop|all:PCT"
        return measure(int(pct), only=case)
    out = B.head("posttrim_bench", line_bytes=2 * n * L, steps=a.steps, yardstick="clip_reads, poly_g_min_length 10, the same share of G tails",
                 params={k: engines[k].posttrim_get() for k in list(engines)[1:]}, batches=[measure(pct) for pct in (0, 10, 100)])
    close(engines)
    return out


def filter_(B):
    a, n, L = B.a, B.a.pairs, B.a.bases
    cases = {"drop0": (0.0, "hot"), "drop10": (0.1, "hot"), "drop100": (1.0, "hot"), "spread": (0.1, "spread")}
    rules = dict(min_length=30, max_n=5, max_unqualified_pct=40, min_mean_quality=20, min_complexity_pct=30)
    B.once_in([None, "off"] + sorted(cases))
    f_launch, q_launch, active, g = B.entry("filter"), B.entry("qstats"), B.asker("filter"), generator(7)
    kinds = {"off": None, "filter": lambda e: e.filter_set(**rules), "qstats": lambda e: e.qstats_enable(True)}
    reason = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    floor = B.floor_ms(4)

    def texts(share):
        """the batch with `share` of its pairs poly-G in R1; the other reads are drawn so that every rule passes them (bases from ACGT
        where make_text has an N in 16, Phred 20 .. 40 where it has 2 .. 40): the dropped share is exactly the poly-G share"""
        b = Batch(n, L)
        bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
        for t in (b.t1, b.t2):
            v = t.view(n, b.rec)
            v[:, 22:22 + L] = bases[torch.randint(0, 4, (n, L), generator=g, device="cuda")]
            v[:, 25 + L:25 + 2 * L] = torch.randint(53, 74, (n, L), generator=g, device="cuda", dtype=torch.uint8)
        poly = torch.rand(n, generator=g, device="cuda") < share if 0 < share < 1 else torch.full((n,), share >= 1, device="cuda")
        b.t1.view(n, b.rec)[poly, 22:22 + L] = ord("G")
        return b, int(poly.sum())

    def measure(case):
        share, route = cases[case]
        b, n_poly = texts(share)
        S, codes = routed_codes(g, n, route)
        engines = contexts({k: kinds[k] for k in (("off",) if a.once == "off" else ("filter",) if a.once else kinds)}, S)

        def off():  # what process_batch does with the stage off: it asks, and launches nothing
            assert active(engines["off"]._h) == 0
        run = {"off": off, "filter": lambda: B.launch(f_launch, engines["filter"], b, codes.data_ptr(), reason.data_ptr()),
               "qstats": lambda: B.launch(q_launch, engines["qstats"], b, codes.data_ptr(), None)}
        run = {k: run[k] for k in engines}
        if a.once:
            out = B.once(run["off" if a.once == "off" else "filter"],
                         {"once": a.once, "pairs": n, "bases": L, "path": engines["filter"].filter_kind() if "filter" in engines else None})
            close(engines)
            return out
        ms = B.timed(run)
        table, launches = engines["filter"].filter_read(), a.steps + a.warmup
        assert int(table[:, 0].sum()) == launches * n and int(table[:, 6].sum()) == 2 * launches * n * L
        assert int(table[:, 5].sum()) == launches * n_poly and int(table[:, 1:5].sum()) == 0 and int(reason[:n].count_nonzero()) == n_poly
        out = {"case": case, "samples": S, "path": engines["filter"].filter_kind(), "dropped_share": n_poly / n, "byte_floor_ms": floor,
               "filter_over_qstats": median(ms["filter"]) / median(ms["qstats"]), "filter_over_floor": median(ms["filter"]) / floor, **by_name(ms)}
        close(engines)
        return out

    if a.once:
        return measure("drop10" if a.once == "off" else a.once)
    out = B.head("filter_bench", line_bytes=4 * n * L, steps=a.steps, rules=rules)
    for case in cases:
        out[case] = measure(case)
    return out


def screen(B):
    """The k-mer screen's kernel with the reference's hash table in LDS (a PhiX-sized random reference) and in global memory (a
    reference of 200 000 k-mers), 0, 10 and 100 % of the pairs drawn from the reference, beside the quality counters' kernel and the
    pairtrim kernel over the same batch.  The byte floor: the two records, the code and the hit words of every pair and the sequence
    line of every read."""
    from quade_amd import screen as qscreen
    a, n, L, k = B.a, B.a.pairs, B.a.bases, 31
    # bases of the random reference: PhiX's size; the fullest LDS table (6 144 k-mers) and the smallest global one (6 145), the two
    # sides of the threshold; 200 000 k-mers
    refs = {"lds": 5386, "ldscap": qscreen.LDS_MAX_KMERS + k - 1, "globaledge": qscreen.LDS_MAX_KMERS + k, "global": 200000 + k - 1}
    cases = {"%s_%d" % (place, pct): (place, pct) for place in refs for pct in (0, 10, 100)}
    B.once_in([None, "off"] + sorted(cases))
    g = generator(7)
    f = B.lib.qd_screen_device
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 5 + [C.c_uint32] + [C.c_void_p] * 5
    q_launch, p_launch, active = B.entry("qstats"), B.entry("pairtrim"), B.asker("screen")
    hits = torch.zeros((n + 64, 2), dtype=torch.int32, device="cuda")
    flag = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    floor = n * (2 * 24 + 2 + 8 + 1 + 2 * L) / COPY_RATE * 1e3
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")

    def reference(place):
        seq = bases[torch.randint(0, 4, (refs[place],), generator=g, device="cuda")]
        ref = qscreen.reference_kmers(b">random\n" + bytes(seq.cpu().numpy()) + b"\n", k)
        return seq, ref.kmers

    def texts(seq, pct):
        """the batch (bases from ACGT) with pct % of its pairs off the reference: R1 and R2 two stretches of it"""
        b = Batch(n, L)
        take = torch.rand(n, generator=g, device="cuda") < pct / 100.0 if 0 < pct < 100 else torch.full((n,), pct >= 100, device="cuda")
        col = torch.arange(L, device="cuda").reshape(1, L)
        for t in (b.t1, b.t2):
            v = t.view(n, b.rec)
            v[:, 22:22 + L] = bases[torch.randint(0, 4, (n, L), generator=g, device="cuda")]
            at = torch.randint(0, seq.numel() - L, (n, 1), generator=g, device="cuda")
            v[:, 22:22 + L] = torch.where(take.reshape(n, 1), seq[at + col], v[:, 22:22 + L])
        return b, int(take.sum())

    def measure(case):
        place, pct = cases[case]
        seq, kmers = reference(place)
        b, n_ref = texts(seq, pct)
        S, codes = routed_codes(g, n, "hot")
        kinds = {"off": None, "screen": lambda e: e.screen_set(kmer=k, min_hits=1, action="drop", kmers=kmers),
                 "qstats": lambda e: e.qstats_enable(True), "pairtrim": lambda e: e.pairtrim_set()}
        engines = contexts({name: kinds[name] for name in (("off",) if a.once == "off" else ("screen",) if a.once else kinds)}, S)
        o1, o2 = b.outputs()

        def off():  # what process_batch does with the stage off: it asks, and launches nothing
            assert active(engines["off"]._h) == 0

        def on():
            rc = f(engines["screen"]._h, b.t1.data_ptr(), b.r1.data_ptr(), b.t2.data_ptr(), b.r2.data_ptr(), n, codes.data_ptr(), None,
                   hits.data_ptr(), flag.data_ptr(), B.st.cuda_stream)
            assert rc == 0, rc
        run = {"off": off, "screen": on, "qstats": lambda: B.launch(q_launch, engines["qstats"], b, codes.data_ptr(), None),
               "pairtrim": lambda: B.launch(p_launch, engines["pairtrim"], b, o1, o2)}
        run = {name: run[name] for name in engines}
        if a.once:
            out = B.once(run["off" if a.once == "off" else "screen"],
                         {"once": a.once, "pairs": n, "bases": L, "path": engines["screen"].screen_kind() if "screen" in engines else None})
            close(engines)
            return out
        ms = B.timed(run)
        table, launches = engines["screen"].screen_read(), a.steps + a.warmup
        tot = [int(x) for x in table.sum(axis=0)]
        # every read is bases alone: all its k-mers exist; a pair off the reference hits with all of them, another pair with none
        assert tot[0] == launches * n and tot[6] == 2 * launches * n * L and tot[4] == 2 * launches * n * (L - k + 1)
        assert tot[1] == tot[2] == tot[3] == launches * n_ref and tot[5] == 2 * launches * n_ref * (L - k + 1)
        assert int(flag[:n].count_nonzero()) == n_ref and int(hits[:n].sum()) == 2 * n_ref * (L - k + 1)
        out = {"case": case, "table": engines["screen"].screen_kind(), "reference_kmers": int(kmers.size), "kmer": k, "samples": S,
               "matched_share": n_ref / n, "byte_floor_ms": floor, "screen_over_qstats": median(ms["screen"]) / median(ms["qstats"]),
               "screen_over_pairtrim": median(ms["screen"]) / median(ms["pairtrim"]), "screen_over_floor": median(ms["screen"]) / floor,
               **by_name(ms)}
        close(engines)
        return out

    if a.once:
        return measure("lds_10" if a.once == "off" else a.once)
    out = B.head("screen_bench", line_bytes=2 * n * L, steps=a.steps, lds_max_kmers=qscreen.LDS_MAX_KMERS,
                 lds_bytes_per_workgroup=(8 << 14) + 24576, workgroup_lanes=1024)
    for case in cases:
        out[case] = measure(case)
    return out


def dup(B):
    """The duplication tally's three launches (dup_keys, dup_claim, dup_count) against the quality counters' kernel.  The byte floor:
    the two records, the code and the reason byte of every pair, the aligned 16-byte words that hold the first 32 bases of both
    reads, and 24 bytes per listed pair."""
    a, n, L = B.a, B.a.pairs, B.a.bases
    cases = {"s%d_d%d" % (s, d): (s, d) for s in (16, 1) for d in (0, 30, 100)}
    B.once_in([None, "off"] + sorted(cases))
    d_launch, q_launch, active, g = B.entry("dup"), B.entry("qstats"), B.asker("dup"), generator(7)
    reason = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    TEMPLATES = 1024  # at 100 % every pair repeats one of these

    def texts(pct, codes):
        """the batch (bases from ACGT: every pair is keyed) with pct % of its pairs a copy of another pair -- reads and code"""
        b = Batch(n, L)
        bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
        for t in (b.t1, b.t2):
            t.view(n, b.rec)[:, 22:22 + L] = bases[torch.randint(0, 4, (n, L), generator=g, device="cuda")]
        if pct >= 100:
            copy = torch.arange(n, device="cuda") >= TEMPLATES
            src = torch.randint(0, TEMPLATES, (n,), generator=g, device="cuda")
        else:
            copy = torch.rand(n, generator=g, device="cuda") < pct / 100.0
            src = torch.randint(0, n, (n,), generator=g, device="cuda")
        if pct:
            for t in (b.t1, b.t2):
                v = t.view(n, b.rec)
                v[copy] = v[src[copy]]
            codes[copy] = codes[src[copy]]
        words = sum(int((((r[:, 3].to(torch.int64) + t.data_ptr()) % 16 + 32 + 15) // 16).sum()) for t, r in ((b.t1, b.r1), (b.t2, b.r2)))
        return b, 16 * words

    def measure(case):
        sample, pct = cases[case]
        S, codes = routed_codes(g, n, "hot")
        b, word_bytes = texts(pct, codes)
        kinds = {"off": None, "dup": lambda e: e.dup_set(bases=32, sample=sample), "qstats": lambda e: e.qstats_enable(True)}
        engines = contexts({k: kinds[k] for k in (("off",) if a.once == "off" else ("dup",) if a.once else kinds)}, S)

        def off():  # what process_batch does with the stage off: it asks, and launches nothing
            assert active(engines["off"]._h) == 0
        run = {"off": off, "dup": lambda: B.launch(d_launch, engines["dup"], b, codes.data_ptr(), reason.data_ptr()),
               "qstats": lambda: B.launch(q_launch, engines["qstats"], b, codes.data_ptr(), None)}
        run = {k: run[k] for k in engines}
        if a.once:
            out = B.once(run["off" if a.once == "off" else "dup"], {"once": a.once, "pairs": n, "bases": L})
            close(engines)
            return out
        ms = B.timed(run)
        stats, launches = engines["dup"].dup_stats(), a.steps + a.warmup
        keys, counts = engines["dup"].dup_read()
        tot = [int(x) for x in stats.sum(axis=0)]
        assert tot[0] == launches * n and tot[1] == tot[2] == 0 and tot[3] == int(counts.sum()) + tot[4] and tot[3] % launches == 0
        listed = tot[3] // launches  # the same batch every launch: its sampled pairs
        assert int(counts.min()) % launches == 0 and (sample > 1 or listed == n)
        floor = (n * (2 * 24 + 2 + 1) + word_bytes + 24 * listed) / COPY_RATE * 1e3
        out = {"case": case, "sample": sample, "duplicate_pct_planted": pct, "samples": S, "listed_pairs": listed, "distinct_keys": len(counts),
               "duplicate_pairs_share": 1.0 - len(counts) / max(listed, 1), "not_tallied": tot[4], "byte_floor_ms": floor,
               "qstats_byte_floor_ms": B.floor_ms(4), "dup_over_qstats": median(ms["dup"]) / median(ms["qstats"]),
               "dup_over_floor": median(ms["dup"]) / floor, **by_name(ms)}
        close(engines)
        return out

    if a.once:
        return measure("s16_d30" if a.once == "off" else a.once)
    out = B.head("dup_bench", steps=a.steps, slots=1 << 24)
    for case in cases:
        out[case] = measure(case)
    return out


def adapter_content(B):
    a, n, L, S = B.a, B.a.pairs, B.a.bases, 96
    cases = {"p%d_%d" % (k, pct): (k, pct) for pct in (0, 10, 100) for k in (6, 16)}
    B.once_in([None, "off"] + sorted(cases))
    builtin = [probe for _, probe in hb.ADAPTER_BUILTIN]
    more = ["".join("ACGT"[(i >> (2 * j)) & 3] for j in range(12)) for i in range(3000, 3010)]  # ten probes no read is planted with
    search = B.lib.qd_adapters_device  # (context, the batch's four pointers, pairs, codes, stream)
    search.restype, search.argtypes = C.c_int, [C.c_void_p] * 5 + [C.c_uint32] + [C.c_void_p] * 2
    count, g = B.entry("qstats"), generator(7)
    codes = torch.randint(0, S, (n,), generator=g, device="cuda") * 2 + (torch.rand(n, generator=g, device="cuda") < 0.1)  # a tenth fail
    codes = codes.to(torch.int16).contiguous()

    def measure(case):
        k, pct = cases[case]
        tally = []
        b = Batch(n, L, plants=(adapters(ADAPTERS[0], pct / 100.0, tally),) * 2)  # both reads the universal adapter: the probe's 12 bases
        kinds = {"off": None, "adapters": lambda e: e.adapters_set(builtin + more[:k - 6]), "qstats": lambda e: e.qstats_enable(True)}
        engines = contexts({x: kinds[x] for x in (("off",) if a.once == "off" else ("adapters",) if a.once else kinds)}, S)

        def run_search(eng):  # "off": what process_batch does with the stage off -- the same call, which launches nothing
            rc = search(eng._h, b.t1.data_ptr(), b.r1.data_ptr(), b.t2.data_ptr(), b.r2.data_ptr(), n, codes.data_ptr(), B.st.cuda_stream)
            assert rc == 0, rc
        run = {x: ((lambda x=x: B.launch(count, engines[x], b, codes.data_ptr(), None)) if x == "qstats" else (lambda x=x: run_search(engines[x])))
               for x in engines}
        if a.once:
            out = B.once(run["off" if a.once == "off" else "adapters"], {"once": a.once, "pairs": n, "bases": L})
            close(engines)
            return out
        ms = B.timed(run)
        launches = a.steps + a.warmup
        t = engines["adapters"].adapters_read()
        # the table against what the generator planted: every read once, the planted probes at least (a random read holds a given
        # 12-mer about once in 120 000 reads), the unused slots empty, and the two parts of the table agree
        assert t["dest"][:, :, 0].sum(axis=0).tolist() == [launches * n] * 2
        found = [int(t["hist"][r, 0].sum()) for r in range(2)]
        assert all(launches * tally[r] <= found[r] <= launches * (tally[r] + n // 20000) for r in range(2)), (found, tally)
        assert (t["hist"].sum(axis=2) == t["dest"].sum(axis=0)[:, 1:]).all() and not t["hist"][:, k:16].any()
        assert (t["hist"][:, 16].sum(axis=1) >= t["hist"][:, 0].sum(axis=1)).all()
        floor = B.floor_ms(2)  # the two sequence lines
        out = {"case": case, "probes": k, "adapter_percent": pct, "samples": S, "reads_with_universal": [f // launches for f in found],
               "planted": tally, "byte_floor_ms": floor, "qstats_byte_floor_ms": B.floor_ms(4),
               "adapters_over_qstats": median(ms["adapters"]) / median(ms["qstats"]), "adapters_over_floor": median(ms["adapters"]) / floor,
               **by_name(ms)}
        close(engines)
        return out

    if a.once:
        return measure("p6_10" if a.once == "off" else a.once)
    out = B.head("adapters_bench", steps=a.steps)
    for case in cases:
        out[case] = measure(case)
    return out


STAGES = {"adapters": adapter_content, "dup": dup, "qstats": qstats, "cycle": cycle, "clip": clip, "trim": trim, "pairtrim": pairtrim, "paircorrect": paircorrect, "posttrim": posttrim, "filter": filter_, "screen": screen}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", required=True, choices=sorted(STAGES))
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--bases", type=int, default=150)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(STAGES[a.stage](Bench(a)))
    print(line)
    if a.out and a.once is None:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
