#!/usr/bin/env python3
"""Cost of the quality counters' kernel (qd_qstats_enable, quade_qstats.hip) over resident text: one batch of the device
pipeline -- 2 M pairs of 2 x 150 bp insert reads as fastq text in HBM with their record tables and routing codes -- counted by
the kernel qd_pipe_run launches.  Two contexts on one device, one with the table off and one with it on, take the same batch;
their calls alternate on one stream (off, on, off, on, ...) and each is timed by HIP events: "off" launches nothing and shows
what the timing itself costs.  Two routings:
  hot    : 96 samples, 90 % of the pairs to 8 destinations (per-workgroup partials in LDS)
  spread : 4 000 samples, uniform over the 8 001 destinations (64-bit global atomics)
Prints one JSON line: per routing the medians off and on, the spread of both, and the byte floor (the four lines' bytes at
6.3 TB/s).

usage: python tools/qstats_bench.py [--pairs N] [--bases L] [--steps K] [--warmup W] [--once hot|spread|off] [--out FILE]
  --once hot|spread  set up, run ONE launch with the table on and exit (for `rocprofv3 --kernel-trace --stats -- python ...`)
  --once off         the same call on the context with the table off (hot routing): the trace shows no kernel of this file
The end-to-end rates come from tools/e2e_bench.py with E2E_QUALITY=1 against none."""
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


def make_text(n, L, seed):
    """n records "@<20-byte name>\\n<L bases>\\n+\\n<L qualities>\\n" on the device and their record table (6 uint32 each)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rec = 1 + 20 + 1 + L + 1 + 2 + L + 1
    t = torch.empty((n, rec), dtype=torch.uint8, device="cuda")
    t[:, 0] = ord("@")
    t[:, 1:21] = torch.randint(48, 58, (n, 20), generator=g, device="cuda", dtype=torch.uint8)
    t[:, 21] = 10
    bases = torch.tensor(list(b"ACGTACGTACGTACGN"), dtype=torch.uint8, device="cuda")
    t[:, 22:22 + L] = bases[torch.randint(0, 16, (n, L), generator=g, device="cuda")]
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
    ap.add_argument("--once", default=None, choices=[None, "hot", "spread", "off"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.pairs, a.bases
    lib = hb.load_library()
    launch = lib.qd_qstats_device  # the pipeline's internal entry: device pointers and a stream
    launch.restype = C.c_int
    launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    t1, r1, rec = make_text(n, L, 1)
    t2, r2, _ = make_text(n, L, 2)
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(7)
    plan = hb.make_plan(True, 25, (0, 8), (0, 8))
    barcodes = lambda S: ["".join("ACGT"[(i >> (2 * k)) & 3] for k in range(16)) for i in range(S)]  # noqa: E731

    def routing(name):
        S = 96 if name == "hot" else 4000
        codes = torch.randint(0, 2 * S + 1, (n,), generator=g, device="cuda")
        if name == "hot":
            hot = torch.rand(n, generator=g, device="cuda") < 0.9
            codes[hot] = torch.randint(0, 8, (int(hot.sum()),), generator=g, device="cuda") * 2
        codes[codes == 2 * S] = 0xFFFF
        engines = {}
        for k in ("off", "on"):
            eng = hb.Engine(0)
            eng.set_plan(plan)
            eng.set_barcodes(barcodes(S))
            if k == "on":
                eng.qstats_enable(True)
            engines[k] = eng
        return S, codes.to(torch.int16).contiguous(), engines

    def once(eng, codes):
        rc = launch(eng._h, t1.data_ptr(), r1.data_ptr(), t2.data_ptr(), r2.data_ptr(), n, codes.data_ptr(), None, st.cuda_stream)  # (no drop bytes)
        assert rc == 0, rc

    floor_ms = 4.0 * n * L / COPY_RATE * 1e3

    def measure(name):
        S, codes, engines = routing(name)
        if a.once:
            once(engines["off" if a.once == "off" else "on"], codes)
            torch.cuda.synchronize()
            return {"once": a.once, "pairs": n, "bases": L, "path": engines["on"].qstats_kind()}
        for _ in range(a.warmup):
            for k in ("off", "on"):
                once(engines[k], codes)
        ev = {"off": [], "on": []}
        for _ in range(a.steps):
            for k in ("off", "on"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                once(engines[k], codes)
                e1.record(st)
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}
        table = engines["on"].qstats_read()
        launches = a.steps + a.warmup
        assert int(table[:, 0, 0].sum()) == launches * n and int(table[:, :, 1].sum()) == 2 * launches * n * L
        out = {"routing": name, "samples": S, "path": engines["on"].qstats_kind(), "off_median_ms": ms["off"][len(ms["off"]) // 2],
               "on_median_ms": ms["on"][len(ms["on"]) // 2], "off_min_ms": ms["off"][0], "off_max_ms": ms["off"][-1],
               "on_min_ms": ms["on"][0], "on_max_ms": ms["on"][-1], "byte_floor_ms": floor_ms,
               "busiest_destination_share": float(table[:, 0, 0].max()) / (launches * n)}
        for eng in engines.values():
            eng.close()
        return out

    if a.once:
        print(json.dumps(measure("hot" if a.once == "off" else a.once)))
        return
    out = {"tool": "qstats_bench", "device": torch.cuda.get_device_name(0), "pairs_per_launch": n, "bases_per_read": L,
           "text_bytes": 2 * n * rec, "line_bytes": 4 * n * L, "steps": a.steps, "hot": measure("hot"), "spread": measure("spread")}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
