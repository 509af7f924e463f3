#!/usr/bin/env python3
"""Cost of the per-cycle counters' kernel (qd_cstats_enable, quade_cstats.hip) over resident text: one batch of the device
pipeline -- 2 M pairs of 2 x 150 bp insert reads as fastq text in HBM with their record tables and routing codes -- counted by
the kernel qd_pipe_run launches.  Per case three contexts on one device take the same batch and their calls alternate on one
stream (off, cycle, qstats, off, ...), each timed by HIP events: "off" launches nothing and shows what the timing itself costs,
"qstats" is the quality counters' kernel (quade_qstats.hip), which reads the same four lines with the same lane shape and is the
yardstick.  Cases (96 samples):
  pass  : every pair to an even code (one group: the hottest LDS words)
  mix   : an even mix of pass, fail and Undetermined
  long  : reads of 2 x 300 bp, every pair pass (two 16-byte words per lane and line, still inside the LDS range)
Prints one JSON line: per case the medians and spreads, the kernel's time over qstats', and the byte floor (the four lines'
bytes at 6.3 TB/s).

usage: python tools/cycle_bench.py [--pairs N] [--bases L] [--steps K] [--warmup W] [--once CASE|off] [--out FILE]
  --once CASE   set up, run ONE launch of the kernel and exit (for `rocprofv3 --kernel-trace --stats -- python ...`)
  --once off    the same call path on a context with the table off (no other context is made): the trace shows no kernel of
                this file
The end-to-end rates come from tools/e2e_bench.py with E2E_CYCLE=1 against none."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from quade_amd import hip_backend as hb  # noqa: E402
from tools.qstats_bench import COPY_RATE, make_text  # noqa: E402

CASES = {"pass": ("pass", 1), "mix": ("mix", 1), "long": ("pass", 2)}  # routing, read length in units of --bases
S = 96


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--bases", type=int, default=150)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", default=None, choices=[None, "off"] + sorted(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.pairs
    lib = hb.load_library()
    c_launch, q_launch = lib.qd_cstats_device, lib.qd_qstats_device  # the pipeline's internal entries: device pointers and a stream
    c_launch.restype = q_launch.restype = C.c_int
    c_launch.argtypes = q_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(7)
    plan = hb.make_plan(True, 25, (0, 8), (0, 8))
    barcodes = ["".join("ACGT"[(i >> (2 * k)) & 3] for k in range(16)) for i in range(S)]

    def routing(name):
        codes = torch.randint(0, S, (n,), generator=g, device="cuda") * 2  # pass
        if name == "mix":
            third = torch.randint(0, 3, (n,), generator=g, device="cuda")
            codes[third == 1] += 1
            codes[third == 2] = 0xFFFF
        return codes.to(torch.int16).contiguous()

    def measure(case):
        route, mult = CASES[case]
        L = a.bases * mult
        floor_ms = 4.0 * n * L / COPY_RATE * 1e3
        t1, r1, _ = make_text(n, L, 1)
        t2, r2, _ = make_text(n, L, 2)
        codes = routing(route)
        engines = {}
        for k in ("off",) if a.once == "off" else ("cycle",) if a.once else ("off", "cycle", "qstats"):
            eng = hb.Engine(0)
            eng.set_plan(plan)
            eng.set_barcodes(barcodes)
            if k == "cycle":
                eng.cstats_enable(True)
            if k == "qstats":
                eng.qstats_enable(True)
            engines[k] = eng

        def once(k):
            # "off": what process_batch does with the table off -- the same call, which launches nothing
            launch = q_launch if k == "qstats" else c_launch
            rc = launch(engines[k]._h, t1.data_ptr(), r1.data_ptr(), t2.data_ptr(), r2.data_ptr(), n, codes.data_ptr(), None, st.cuda_stream)
            assert rc == 0, rc

        if a.once:
            once("off" if a.once == "off" else "cycle")
            torch.cuda.synchronize()
            for eng in engines.values():
                eng.close()
            return {"once": a.once, "pairs": n, "bases": L}
        for _ in range(a.warmup):
            for k in engines:
                once(k)
        ev = {k: [] for k in engines}
        for _ in range(a.steps):
            for k in engines:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                once(k)
                e1.record(st)
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}
        launches = a.steps + a.warmup
        t, q = engines["cycle"].cstats_read(), engines["qstats"].qstats_read()
        assert int(t["len"].sum()) == 2 * launches * n and int(t["len"][:, :, L].sum()) == 2 * launches * n  # the one hot length bin
        groups = [int(t["len"][k].sum()) for k in range(3)]
        assert (groups[1] == groups[2] == 0) if route == "pass" else min(groups) > 0.3 * 2 * launches * n
        for k, col in ((4, 5), (5, 2), (6, 3), (7, 4)):  # N, qual_sum, q20, q30 against the quality counters of the same batch
            assert int(t["cycle"][:, :, :, k].sum()) == int(q[:, :, col].sum()), (k, col)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        out = {"case": case, "samples": S, "bases_per_read": L, "byte_floor_ms": floor_ms, "cycle_over_qstats": med["cycle"] / med["qstats"],
               "cycle_over_floor": med["cycle"] / floor_ms}
        for k, v in ms.items():
            out.update({k + "_median_ms": med[k], k + "_min_ms": v[0], k + "_max_ms": v[-1]})
        for eng in engines.values():
            eng.close()
        return out

    if a.once:
        print(json.dumps(measure("pass" if a.once == "off" else a.once)))
        return
    out = {"tool": "cycle_bench", "device": torch.cuda.get_device_name(0), "pairs_per_launch": n, "bases_per_read": a.bases,
           "steps": a.steps, "lds_cycles": lib.qd_cstats_lds_cycles()}
    for case in CASES:
        out[case] = measure(case)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
