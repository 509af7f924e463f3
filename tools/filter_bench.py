#!/usr/bin/env python3
"""Cost of the read filter's kernel (qd_filter_set, quade_filter.hip) over resident text: one batch of the device pipeline -- 2 M
pairs of 2 x 150 bp insert reads as fastq text in HBM with their record tables and routing codes -- filtered by the kernel
qd_pipe_run launches.  Per case three contexts on one device take the same batch and their calls alternate on one stream (off,
filter, qstats, off, ...), each timed by HIP events: "off" launches nothing and shows what the timing itself costs, "qstats" is
the quality counters' kernel (quade_qstats.hip), which reads the same four lines with the same lane shape and is the yardstick:
the filter should cost no more than twice as much.  Cases: a share of the pairs is made poly-G, which the filter
(min_length 30, max_n 5, max_unqualified_pct 40, min_mean_quality 20, min_complexity_pct 30) drops:
  drop0 / drop10 / drop100 : 0 %, 10 %, 100 % of the pairs dropped; 96 samples, 90 % of the pairs to 8 destinations (LDS partials)
  spread                   : 10 % dropped; 4 000 samples, uniform over the 8 001 destinations (64-bit global atomics)
Prints one JSON line: per case the medians and spreads, the filter's time over qstats', and the byte floor (the four lines'
bytes at 6.3 TB/s).

usage: python tools/filter_bench.py [--pairs N] [--bases L] [--steps K] [--warmup W] [--once CASE|off] [--out FILE]
  --once CASE   set up, run ONE launch of the filter and exit (for `rocprofv3 --kernel-trace --stats -- python ...`)
  --once off    the same call path on a context with the stage off (drop10; no other context is made): the trace shows no kernel
                of this file
The end-to-end rates come from tools/e2e_bench.py with E2E_FILTER=1 against none."""
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

CASES = {"drop0": (0.0, "hot"), "drop10": (0.1, "hot"), "drop100": (1.0, "hot"), "spread": (0.1, "spread")}
RULES = dict(min_length=30, max_n=5, max_unqualified_pct=40, min_mean_quality=20, min_complexity_pct=30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--bases", type=int, default=150)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", default=None, choices=[None, "off"] + sorted(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.pairs, a.bases
    lib = hb.load_library()
    f_launch, q_launch = lib.qd_filter_device, lib.qd_qstats_device  # the pipeline's internal entries: device pointers and a stream
    active = lib.qd_filter_active
    f_launch.restype = q_launch.restype = active.restype = C.c_int
    active.argtypes = [C.c_void_p]
    f_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    q_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(7)
    plan = hb.make_plan(True, 25, (0, 8), (0, 8))
    barcodes = lambda S: ["".join("ACGT"[(i >> (2 * k)) & 3] for k in range(16)) for i in range(S)]  # noqa: E731
    reason = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    floor_ms = 4.0 * n * L / COPY_RATE * 1e3

    def texts(share):
        """the batch with `share` of its pairs poly-G in R1; the other reads are drawn so that every rule passes them (bases from ACGT
        where make_text has an N in 16, Phred 20 .. 40 where it has 2 .. 40): the dropped share is exactly the poly-G share"""
        t1, r1, rec = make_text(n, L, 1)
        t2, r2, _ = make_text(n, L, 2)
        bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
        for t in (t1, t2):
            v = t.view(n, rec)
            v[:, 22:22 + L] = bases[torch.randint(0, 4, (n, L), generator=g, device="cuda")]
            v[:, 25 + L:25 + 2 * L] = torch.randint(53, 74, (n, L), generator=g, device="cuda", dtype=torch.uint8)
        poly = torch.rand(n, generator=g, device="cuda") < share if 0 < share < 1 else torch.full((n,), share >= 1, device="cuda")
        t1.view(n, rec)[poly, 22:22 + L] = ord("G")
        return t1, r1, t2, r2, int(poly.sum())

    def routing(name):
        S = 96 if name == "hot" else 4000
        codes = torch.randint(0, 2 * S + 1, (n,), generator=g, device="cuda")
        if name == "hot":
            hot = torch.rand(n, generator=g, device="cuda") < 0.9
            codes[hot] = torch.randint(0, 8, (int(hot.sum()),), generator=g, device="cuda") * 2
        codes[codes == 2 * S] = 0xFFFF
        engines = {}
        for k in ("off",) if a.once == "off" else ("filter",) if a.once else ("off", "filter", "qstats"):
            eng = hb.Engine(0)
            eng.set_plan(plan)
            eng.set_barcodes(barcodes(S))
            if k == "filter":
                eng.filter_set(**RULES)
            if k == "qstats":
                eng.qstats_enable(True)
            engines[k] = eng
        return S, codes.to(torch.int16).contiguous(), engines

    def measure(case):
        share, route = CASES[case]
        t1, r1, t2, r2, n_poly = texts(share)
        S, codes, engines = routing(route)

        def once(k):
            if k == "filter":
                rc = f_launch(engines[k]._h, t1.data_ptr(), r1.data_ptr(), t2.data_ptr(), r2.data_ptr(), n, codes.data_ptr(), reason.data_ptr(), st.cuda_stream)
            elif k == "qstats":
                rc = q_launch(engines[k]._h, t1.data_ptr(), r1.data_ptr(), t2.data_ptr(), r2.data_ptr(), n, codes.data_ptr(), None, st.cuda_stream)
            else:  # what process_batch does with the stage off: it asks, and launches nothing
                rc = 0 if active(engines[k]._h) == 0 else -1
            assert rc == 0, rc

        if a.once:
            once("off" if a.once == "off" else "filter")
            torch.cuda.synchronize()
            out = {"once": a.once, "pairs": n, "bases": L, "path": engines["filter"].filter_kind() if "filter" in engines else None}
            for eng in engines.values():
                eng.close()
            return out
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
        table = engines["filter"].filter_read()
        launches = a.steps + a.warmup
        assert int(table[:, 0].sum()) == launches * n and int(table[:, 6].sum()) == 2 * launches * n * L
        assert int(table[:, 5].sum()) == launches * n_poly and int(table[:, 1:5].sum()) == 0 and int(reason[:n].count_nonzero()) == n_poly
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        out = {"case": case, "samples": S, "path": engines["filter"].filter_kind(), "dropped_share": n_poly / n, "byte_floor_ms": floor_ms,
               "filter_over_qstats": med["filter"] / med["qstats"], "filter_over_floor": med["filter"] / floor_ms}
        for k, v in ms.items():
            out.update({k + "_median_ms": med[k], k + "_min_ms": v[0], k + "_max_ms": v[-1]})
        for eng in engines.values():
            eng.close()
        return out

    if a.once:
        print(json.dumps(measure("drop10" if a.once == "off" else a.once)))
        return
    out = {"tool": "filter_bench", "device": torch.cuda.get_device_name(0), "pairs_per_launch": n, "bases_per_read": L,
           "line_bytes": 4 * n * L, "steps": a.steps, "rules": RULES}
    for case in CASES:
        out[case] = measure(case)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
