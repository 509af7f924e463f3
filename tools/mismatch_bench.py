#!/usr/bin/env python3
"""Cost of mismatch-tolerant matching (qd_set_mismatches) on the resident hot path: dual 8+8 bp index, 96 samples drawn at
per-part distance >= 3 (no collision under budgets (1, 1)), 10 % of the pairs one substitution away from their barcode (the
pairs the rescue moves), 100 M pairs resident in HBM.  Demux time by HIP events on the launch stream at budgets (0, 0)
against (1, 1); the difference is the rescue post-pass (compaction + match).  Prints one JSON line.

usage: python tools/mismatch_bench.py [--pairs N] [--steps K] [--warmup W] [--once M1,M2] [--out FILE]
  --once M1,M2   set up, run ONE demux at those budgets and exit (for `rocprofv3 --kernel-trace --stats -- python ...`)
The end-to-end rates come from tools/e2e_bench.py with E2E_MISMATCHES=1,1 against no budgets."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from quade_amd import hip_backend as hb  # noqa: E402
from quade_amd import synth  # noqa: E402


def workload(n, seed=7):
    """rows of n pairs on cuda:0 for the cfg3 plan, the sheet (list of str) and the layout"""
    plan = synth.config_plan("cfg3")
    lay = hb.plan_layout(plan)
    bcs = synth.make_far_barcodes(96, 8, 8, 1, 1, seed=seed)
    bc = torch.tensor(np.array([np.frombuffer(b.encode(), np.uint8) for b in bcs]), device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    acgtn = torch.tensor(list(b"ACGTN"), dtype=torch.uint8, device="cuda")
    seq = [torch.empty((n, lay.seq_stride[k]), dtype=torch.uint8, device="cuda") for k in range(2)]
    qual = [torch.empty((n, lay.qual_stride[k]), dtype=torch.uint8, device="cuda") for k in range(2)]
    chunk = 16_000_000
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        key = bc[torch.randint(0, 96, (m,), generator=g, device="cuda")]
        miss = torch.randint(0, 10, (m,), generator=g, device="cuda") == 0
        rows = torch.nonzero(miss).squeeze(1)
        pos = torch.randint(0, 16, (rows.numel(),), generator=g, device="cuda")
        old = key[rows, pos]
        idx = (old == 67).long() + 2 * (old == 71).long() + 3 * (old == 84).long() + 4 * (old == 78).long()
        key[rows, pos] = acgtn[(idx + torch.randint(1, 5, (rows.numel(),), generator=g, device="cuda")) % 5]
        q = (torch.randint(30, 41, (m, 16), generator=g, device="cuda") + 33).to(torch.uint8)
        bad = torch.randint(0, 100, (m,), generator=g, device="cuda") < 15
        q[bad, 0] = 40
        for k in range(2):
            seq[k][a:a + m].zero_()
            seq[k][a:a + m, :8] = key[:, 8 * k:8 * k + 8]
            qual[k][a:a + m].fill_(0xFF)
            qual[k][a:a + m, :8] = q[:, 8 * k:8 * k + 8]
    torch.cuda.synchronize()
    return plan, lay, bcs, seq, qual


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.pairs
    plan, lay, bcs, seq, qual = workload(n)
    codes = torch.empty(n + 8, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream()
    eng = hb.Engine(0)
    eng.set_plan(plan)
    eng.set_barcodes(bcs)
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731

    def run(m1, m2, steps, warmup):
        eng.set_mismatches(m1, m2)
        eng.reset_counts()
        for _ in range(warmup):
            eng.demux_device(n, ptr(seq), ptr(qual), codes.data_ptr(), stream=st.cuda_stream)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for e0, e1 in ev:
            e0.record(st)
            eng.demux_device(n, ptr(seq), ptr(qual), codes.data_ptr(), stream=st.cuda_stream)
            e1.record(st)
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        c = eng.counts()
        return {"budgets": [m1, m2], "median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1],
                "undetermined_per_launch": int(c[3]) // (steps + warmup), "pairs_per_launch": n}

    if a.once:
        m1, m2 = (int(x) for x in a.once.split(","))
        print(json.dumps(run(m1, m2, 1, 0)))
        return
    r0 = run(0, 0, a.steps, a.warmup)
    r1 = run(1, 1, a.steps, a.warmup)
    r0b = run(0, 0, a.steps, a.warmup)  # (0, 0) again: the drift of the device between the two runs
    out = {"tool": "mismatch_bench", "device": eng.device_info()["name"], "config": "cfg3 plan, 96 samples at per-part distance >= 3, "
           "10 % one substitution away", "exact": r0, "exact_again": r0b, "tolerant_1_1": r1,
           "rescue_ms": r1["median_ms"] - (r0["median_ms"] + r0b["median_ms"]) / 2,
           "rescued_per_launch": r0["undetermined_per_launch"] - r1["undetermined_per_launch"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
