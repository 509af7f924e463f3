#!/usr/bin/env python3
"""Cost of the clip kernel (qd_clip_set, quade_clip.hip) over resident text: one batch of the device pipeline -- 2 M pairs of
2 x 150 bp insert reads as fastq text in HBM with their record tables -- run through the kernel qd_pipe_run launches, beside the
nearest existing kernel on the same batch in the same session: trim_reads with a quality cutoff only (quade_trim.hip), which stages
the same lines.  One context per case on one device; their calls alternate on one stream (yardstick, window, poly-G, all, ...) and
each is timed by HIP events.  Cases: the window rule alone (4 bases, mean quality 20), the poly-G rule alone (10 bases), and all
rules together (1 base off each 3' end, window, poly-G).  Three batches: 0 %, 10 % and 100 % of the reads end in 30 G of high
quality; half the reads of every batch have a low-quality 3' tail of up to 40 bases.  Prints one JSON line: per batch and case the
median, the spread, the ratio to the yardstick and to the byte floor (reading the four lines once at 6.3 TB/s).

usage: python tools/clip_bench.py [--pairs N] [--bases L] [--steps K] [--warmup W] [--once CASE:PCT] [--out FILE]
  --once CASE:PCT  set up the batch with PCT % G tails, run ONE launch of CASE and exit (for `rocprofv3 --kernel-trace --stats -- python ...`)
The end-to-end rates come from tools/e2e_bench.py with E2E_CLIP=1 against none."""
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
G_TAIL = 30
CASES = ("yardstick", "window", "poly_g", "all")


def make_text(n, L, seed, share):
    """n records "@<20-byte name>\\n<L bases>\\n+\\n<L qualities>\\n" on the device and their record table (6 uint32 each); a
    `share` of the reads ends in G_TAIL bases G; qualities 30 .. 40, on half the reads a 3' tail of 0 .. 40 bases at 2 .. 19 (not
    under a G tail: a dark cluster reads as high-quality G)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rec = 1 + 20 + 1 + L + 1 + 2 + L + 1
    t = torch.empty((n, rec), dtype=torch.uint8, device="cuda")
    t[:, 0] = ord("@")
    t[:, 1:21] = torch.randint(48, 58, (n, 20), generator=g, device="cuda", dtype=torch.uint8)
    t[:, 21] = 10
    bases = torch.tensor(list(b"ACGTACGTACGTACGN"), dtype=torch.uint8, device="cuda")
    seq = bases[torch.randint(0, 16, (n, L), generator=g, device="cuda")]
    col = torch.arange(L, device="cuda").reshape(1, L)
    has = (torch.rand(n, generator=g, device="cuda") < share).reshape(n, 1)
    seq = torch.where(has & (col >= L - G_TAIL), torch.full_like(seq, ord("G")), seq)
    t[:, 22:22 + L] = seq
    t[:, 22 + L] = 10
    t[:, 23 + L] = ord("+")
    t[:, 24 + L] = 10
    qual = torch.randint(33 + 30, 33 + 41, (n, L), generator=g, device="cuda", dtype=torch.uint8)
    low = torch.randint(33 + 2, 33 + 20, (n, L), generator=g, device="cuda", dtype=torch.uint8)
    tail = torch.randint(0, 41, (n, 1), generator=g, device="cuda") * (torch.rand(n, 1, generator=g, device="cuda") < 0.5)
    t[:, 25 + L:25 + 2 * L] = torch.where(~has & (col >= L - tail), low, qual)
    t[:, 25 + 2 * L] = 10
    head = torch.arange(n, device="cuda", dtype=torch.int64) * rec
    recs = torch.stack([head, head + 1, torch.full_like(head, 20), head + 22, torch.full_like(head, L), head + 25 + L], dim=1)
    assert n * rec < 1 << 31
    return t.reshape(-1), recs.to(torch.int32).contiguous(), rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--bases", type=int, default=150)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.pairs, a.bases
    lib = hb.load_library()
    # the pipeline's internal entries: device pointers and a stream
    launches = {}
    for name in ("qd_trim_device", "qd_clip_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        launches[name] = f
    st = torch.cuda.current_stream()
    engines = {k: hb.Engine(0) for k in CASES}
    engines["yardstick"].trim_set(quality_cutoff=20)
    engines["window"].clip_set(window_size=4, window_quality=20)
    engines["poly_g"].clip_set(poly_g_min_length=10)
    engines["all"].clip_set(tail_clip_r1=1, tail_clip_r2=1, window_size=4, window_quality=20, poly_g_min_length=10)
    floor_ms = 4.0 * n * L / COPY_RATE * 1e3

    def measure(pct, only=None):
        t1, r1, rec = make_text(n, L, 1, pct / 100.0)
        t2, r2, _ = make_text(n, L, 2, pct / 100.0)
        o1, o2 = torch.empty_like(r1), torch.empty_like(r2)

        def once(k):
            f = launches["qd_trim_device" if k == "yardstick" else "qd_clip_device"]
            rc = f(engines[k]._h, t1.data_ptr(), r1.data_ptr(), t2.data_ptr(), r2.data_ptr(), n, o1.data_ptr(), o2.data_ptr(), st.cuda_stream)
            assert rc == 0, rc

        if only is not None:
            once(only)
            torch.cuda.synchronize()
            return {"once": only, "g_tail_percent": pct, "pairs": n, "bases": L}
        for eng in engines.values():
            eng.reset_counts()
        for _ in range(a.warmup):
            for k in CASES:
                once(k)
        ev = {k: [] for k in CASES}
        for _ in range(a.steps):
            for k in CASES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                once(k)
                e1.record(st)
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        runs = a.steps + a.warmup
        out = {"g_tail_percent": pct, "byte_floor_ms": floor_ms, "cases": {}}
        for k in CASES:
            table = engines[k].trim_read() if k == "yardstick" else engines[k].clip_read()
            assert int(table[0, 0]) == int(table[1, 0]) == runs * n and int(table[:, 1].sum()) == 2 * runs * n * L
            per = lambda c: float(table[:, c].sum()) / (2 * runs * n)  # noqa: E731
            row = {"median_ms": med[k], "min_ms": ms[k][0], "max_ms": ms[k][-1], "over_yardstick": med[k] / med["yardstick"],
                   "over_floor": med[k] / floor_ms, "mean_bases_out": per(2)}
            if k != "yardstick":
                row.update(window_read_share=per(7), polyg_read_share=per(9))
            out["cases"][k] = row
        return out

    if a.once is not None:
        case, pct = a.once.split(":")
        assert case in CASES
        print(json.dumps(measure(int(pct), only=case)))
        return
    out = {"tool": "clip_bench", "device": torch.cuda.get_device_name(0), "pairs_per_launch": n, "bases_per_read": L,
           "line_bytes": 4 * n * L, "steps": a.steps, "yardstick": "trim_reads, quality_cutoff 20, no adapter",
           "params": {k: engines[k].clip_get() for k in CASES[1:]}, "batches": [measure(pct) for pct in (0, 10, 100)]}
    for eng in engines.values():
        eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
