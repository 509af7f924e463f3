#!/usr/bin/env python3
"""Cost of the unknown-barcode tally (qd_unknown_enable) on the resident hot path: synth's cfg3 (dual 8+8 bp index, 96 samples,
10 % of the pairs Undetermined), 100 M pairs resident in HBM.  Two contexts on one device, one with the tally off and one with
it on, take the same rows; their launches alternate on one stream (off, on, off, on, ...) so that both see the same device
state, and each launch is timed by HIP events.  Two key distributions:
  distinct : synth's own Undetermined pairs (half of them uniform random reads: millions of distinct keys)
  hot      : 80 % of the Undetermined pairs rewritten to 8 keys
Prints one JSON line: per distribution the medians with the tally off and on, their difference, and the spread of the "off"
launches (the floor under which a difference means nothing).

usage: python tools/unknown_bench.py [--pairs N] [--steps K] [--warmup W] [--slots S] [--once off|on] [--hot] [--out FILE]
  --once off|on  set up, run ONE demux with the tally off / on and exit (for `rocprofv3 --kernel-trace --stats -- python ...`;
                 with --hot on the hot distribution)
The end-to-end rates come from tools/e2e_bench.py with E2E_UNKNOWN=10 against none."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from quade_amd import hip_backend as hb  # noqa: E402
from quade_amd import synth  # noqa: E402


def make_hot(w, seed=3):
    """80 % of the Undetermined pairs of w get one of 8 keys that are not on the sheet (in place)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sheet = set(w.barcode_strings())
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    hot = []
    while len(hot) < 8:
        k = acgt[torch.randint(0, 4, (16,), generator=g, device="cuda")]
        if bytes(k.cpu().tolist()).decode() not in sheet:
            hot.append(k)
    hot = torch.stack(hot)
    rows = torch.nonzero(w.expected == 0xFFFF).squeeze(1)
    rows = rows[torch.rand(rows.numel(), generator=g, device="cuda") < 0.8]
    key = hot[torch.randint(0, 8, (rows.numel(),), generator=g, device="cuda")]
    w.seq[0][rows, :8] = key[:, :8]
    w.seq[1][rows, :8] = key[:, 8:]
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 24)
    ap.add_argument("--once", default=None)
    ap.add_argument("--hot", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.pairs
    w = synth.generate("cfg3", n, device="cuda")
    codes = torch.empty(n + 8, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream()
    engines = {}
    for name in ("off", "on"):
        eng = hb.Engine(0)
        eng.set_plan(w.plan)
        eng.set_barcodes(w.barcode_strings())
        if name == "on":
            eng.unknown_enable(a.slots)
        engines[name] = eng
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731

    def once(eng):
        eng.demux_device(n, ptr(w.seq), ptr(w.qual), codes.data_ptr(), stream=st.cuda_stream)

    if a.once:
        if a.hot:
            make_hot(w)
        once(engines[a.once])
        torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "hot": a.hot, "pairs": n}))
        return

    def measure(label):
        for eng in engines.values():
            eng.reset_counts()
        for _ in range(a.warmup):
            for name in ("off", "on"):
                once(engines[name])
        ev = {"off": [], "on": []}
        for _ in range(a.steps):
            for name in ("off", "on"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                once(engines[name])
                e1.record(st)
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}
        stats = [int(x) for x in engines["on"].unknown_stats()]
        launches = a.steps + a.warmup
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        return {"distribution": label, "off_median_ms": med["off"], "on_median_ms": med["on"], "tally_ms": med["on"] - med["off"],
                "off_min_ms": ms["off"][0], "off_max_ms": ms["off"][-1], "on_min_ms": ms["on"][0], "on_max_ms": ms["on"][-1],
                "undetermined_per_launch": int(engines["on"].counts()[3]) // launches, "tallied_per_launch": stats[0] // launches,
                "dropped": stats[2], "distinct_entries": stats[3], "table_load": stats[3] / a.slots}

    distinct = measure("distinct")
    make_hot(w)
    hot = measure("hot")
    out = {"tool": "unknown_bench", "device": engines["on"].device_info()["name"], "config": "cfg3, 96 samples, 10 % Undetermined",
           "pairs_per_launch": n, "slots": a.slots, "steps": a.steps, "distinct": distinct, "hot": hot}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
