#!/usr/bin/env python3
"""Cost of the trimming kernel (qd_trim_set, quade_trim.hip) over resident text: one batch of the device pipeline -- 2 M pairs of
2 x 150 bp insert reads as fastq text in HBM with their record tables -- trimmed by the kernel qd_pipe_run launches (quality
cutoff 20, a 33-base adapter per read, the defaults otherwise).  Two contexts on one device, one with trimming off and one with it
on, take the same batch; their calls alternate on one stream (off, on, off, on, ...) and each is timed by HIP events: "off" asks
qd_trim_active as the pipeline does, launches nothing and shows what the timing itself costs.  Three batches: 0 %, 10 % and 100 %
of the reads carry their adapter from a random position on.  Prints one JSON line: per batch the medians off and on, the spread
of both, and the byte floor (reading the four lines once at 6.3 TB/s).

usage: python tools/trim_bench.py [--pairs N] [--bases L] [--steps K] [--warmup W] [--once PCT] [--out FILE]
  --once PCT  set up the batch with PCT % adapters, run ONE launch and exit (for `rocprofv3 --kernel-trace --stats -- python ...`)
The end-to-end rates come from tools/e2e_bench.py with E2E_TRIM=1 against none."""
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


def make_text(n, L, seed, adapter, share):
    """n records "@<20-byte name>\\n<L bases>\\n+\\n<L qualities>\\n" on the device and their record table (6 uint32 each); a
    `share` of the reads holds the adapter (cut at the read's end) from a random position on"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rec = 1 + 20 + 1 + L + 1 + 2 + L + 1
    t = torch.empty((n, rec), dtype=torch.uint8, device="cuda")
    t[:, 0] = ord("@")
    t[:, 1:21] = torch.randint(48, 58, (n, 20), generator=g, device="cuda", dtype=torch.uint8)
    t[:, 21] = 10
    bases = torch.tensor(list(b"ACGTACGTACGTACGN"), dtype=torch.uint8, device="cuda")
    seq = bases[torch.randint(0, 16, (n, L), generator=g, device="cuda")]
    if share > 0:
        ad = torch.tensor(list(adapter.encode()), dtype=torch.uint8, device="cuda")
        has = torch.rand(n, generator=g, device="cuda") < share
        p = torch.randint(0, L, (n, 1), generator=g, device="cuda")
        col = torch.arange(L, device="cuda").reshape(1, L)
        inside = has.reshape(n, 1) & (col >= p) & (col < p + len(ad))
        seq = torch.where(inside, ad[(col - p).clamp(0, len(ad) - 1)], seq)
    t[:, 22:22 + L] = seq
    t[:, 22 + L] = 10
    t[:, 23 + L] = ord("+")
    t[:, 24 + L] = 10
    t[:, 25 + L:25 + 2 * L] = torch.randint(35, 74, (n, L), generator=g, device="cuda", dtype=torch.uint8)
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
    ap.add_argument("--once", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.pairs, a.bases
    lib = hb.load_library()
    launch, active = lib.qd_trim_device, lib.qd_trim_active  # the pipeline's internal entries: device pointers and a stream
    launch.restype = active.restype = C.c_int
    launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    active.argtypes = [C.c_void_p]
    st = torch.cuda.current_stream()
    engines = {"off": hb.Engine(0), "on": hb.Engine(0)}
    engines["on"].trim_set(ADAPTERS[0], ADAPTERS[1], quality_cutoff=20)
    floor_ms = 4.0 * n * L / COPY_RATE * 1e3

    def measure(pct):
        t1, r1, rec = make_text(n, L, 1, ADAPTERS[0], pct / 100.0)
        t2, r2, _ = make_text(n, L, 2, ADAPTERS[1], pct / 100.0)
        o1, o2 = torch.empty_like(r1), torch.empty_like(r2)

        def once(eng):
            if active(eng._h):  # (what process_batch does)
                rc = launch(eng._h, t1.data_ptr(), r1.data_ptr(), t2.data_ptr(), r2.data_ptr(), n, o1.data_ptr(), o2.data_ptr(), st.cuda_stream)
                assert rc == 0, rc

        if a.once is not None:
            once(engines["on"])
            torch.cuda.synchronize()
            return {"once": pct, "pairs": n, "bases": L}
        engines["on"].reset_counts()
        for _ in range(a.warmup):
            for k in ("off", "on"):
                once(engines[k])
        ev = {"off": [], "on": []}
        for _ in range(a.steps):
            for k in ("off", "on"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                once(engines[k])
                e1.record(st)
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}
        table = engines["on"].trim_read()
        launches = a.steps + a.warmup
        assert int(table[0, 0]) == int(table[1, 0]) == launches * n and int(table[:, 1].sum()) == 2 * launches * n * L
        assert (o1[:, [0, 1, 2, 3, 5]] == r1[:, [0, 1, 2, 3, 5]]).all() and int(o1[:, 4].max()) <= L
        per = lambda k: float(table[:, k].sum()) / (2 * launches * n)  # noqa: E731
        return {"adapter_percent": pct, "off_median_ms": ms["off"][len(ms["off"]) // 2], "on_median_ms": ms["on"][len(ms["on"]) // 2],
                "off_min_ms": ms["off"][0], "off_max_ms": ms["off"][-1], "on_min_ms": ms["on"][0], "on_max_ms": ms["on"][-1],
                "byte_floor_ms": floor_ms, "on_over_floor": ms["on"][len(ms["on"]) // 2] / floor_ms,
                "quality_trimmed_read_share": per(3), "adapter_read_share": per(5), "mean_bases_out": per(2)}

    if a.once is not None:
        print(json.dumps(measure(a.once)))
        return
    out = {"tool": "trim_bench", "device": torch.cuda.get_device_name(0), "pairs_per_launch": n, "bases_per_read": L,
           "line_bytes": 4 * n * L, "steps": a.steps, "params": engines["on"].trim_get(),
           "batches": [measure(pct) for pct in (0, 10, 100)]}
    for eng in engines.values():
        eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
