#!/usr/bin/env python3
"""Cost of the index-hopping matrix (qd_hop_enable) on the resident hot path, against the unknown-barcode tally's over the same
batch: synth's cfg3 (dual 8+8 bp index, 96 samples, 10 % of the pairs Undetermined), 100 M pairs resident in HBM.  Three
contexts on one device -- nothing enabled, the matrix, the tally -- take the same rows; their launches alternate on one stream
(off, hop, tally, off, ...) so that all see the same device state, and each launch is timed by HIP events.  Three fills of the
Undetermined share, written over the index windows of the pairs the generator marks 0xFFFF:
  neither : uniform random reads, neither index among the sheet's values: every pair in cell (n1, n2)
  one     : one unexpected combination: every pair in one cell
  spread  : unexpected combinations drawn evenly over all (a, b) with a < n1, b < n2 that are off the sheet
Prints one JSON line: per fill the medians of the three contexts, what the matrix and the tally add, and the spread of the "off"
launches (the floor under which a difference means nothing).  The yardstick is the tally's added time in the same session; the
matrix's table is checked against its invariant (sum == Undetermined, and where the fill puts the pairs) afterwards.

usage: python tools/hop_bench.py [--pairs N] [--steps K] [--warmup W] [--slots S] [--once off|hop|tally] [--fill F] [--out FILE]
  --once CASE  set up, run ONE demux with that context and exit (for `rocprofv3 --kernel-trace --stats -- python ...`; --fill
               chooses the fill, default neither)
The end-to-end rates come from tools/e2e_bench.py with E2E_HOPPING=1 against none."""
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

FILLS = ("neither", "one", "spread")


def _words(rows):
    """uint8 [n, 8] -> int64 [n]"""
    return rows.contiguous().view(torch.int64).squeeze(1)


def fill(w, kind, parts, seed=3):
    """rewrites the index windows of the Undetermined pairs of w in place; parts = (part1, part2, n1, n2) of the sheet.
    Returns the cells the pairs go to: a list of (a, b), None = every off-sheet cell with both parts known."""
    part1, part2, n1, n2 = parts
    g = torch.Generator(device="cuda").manual_seed(seed)
    bcs = w.barcodes.cuda()
    first = {int(a): s for s, a in reversed(list(enumerate(part1)))}  # a sample that carries part a
    second = {int(b): s for s, b in reversed(list(enumerate(part2)))}
    p1 = torch.stack([bcs[first[a], :8] for a in range(n1)])
    p2 = torch.stack([bcs[second[b], 8:] for b in range(n2)])
    rows = torch.nonzero(w.expected == 0xFFFF).squeeze(1)
    m = rows.numel()
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    if kind == "neither":
        cells = [(n1, n2)]
        for k, known in ((0, _words(p1)), (1, _words(p2))):
            r = acgt[torch.randint(0, 4, (m, 8), generator=g, device="cuda")]
            for _ in range(32):
                hit = torch.isin(_words(r), known)
                if not bool(hit.any()):
                    break
                r[hit] = acgt[torch.randint(0, 4, (int(hit.sum()), 8), generator=g, device="cuda")]
            w.seq[k][rows, :8] = r
    else:
        on = torch.zeros((n1, n2), dtype=torch.bool, device="cuda")
        on[torch.tensor(part1, device="cuda").long(), torch.tensor(part2, device="cuda").long()] = True
        off = torch.nonzero(~on)
        assert off.shape[0] > 0, "the sheet has no unexpected cell"
        if kind == "one":
            pick = off[:1].expand(m, 2)
            cells = [tuple(int(x) for x in off[0])]
        else:
            pick = off[torch.randint(0, off.shape[0], (m,), generator=g, device="cuda")]
            cells = None
        w.seq[0][rows, :8] = p1[pick[:, 0]]
        w.seq[1][rows, :8] = p2[pick[:, 1]]
    torch.cuda.synchronize()
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 24)
    ap.add_argument("--once", default=None, choices=("off", "hop", "tally"))
    ap.add_argument("--fill", default=None, choices=FILLS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.pairs
    w = synth.generate("cfg3", n, device="cuda")
    bcs = w.barcode_strings()
    parts = hb.hop_index(bcs, 16, 8)
    part1, part2, n1, n2 = parts
    codes = torch.empty(n + 8, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream()
    engines = {}
    for name in ("off", "hop", "tally"):
        eng = hb.Engine(0)
        eng.set_plan(w.plan)
        eng.set_barcodes(bcs)
        if name == "hop":
            eng.hop_enable(True)
        if name == "tally":
            eng.unknown_enable(a.slots)
        engines[name] = eng
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731

    def once(eng):
        eng.demux_device(n, ptr(w.seq), ptr(w.qual), codes.data_ptr(), stream=st.cuda_stream)

    if a.once:
        fill(w, a.fill or "neither", parts)
        once(engines[a.once])
        torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "fill": a.fill or "neither", "pairs": n}))
        return

    def measure(kind):
        cells = fill(w, kind, parts)
        for eng in engines.values():
            eng.reset_counts()
        for _ in range(a.warmup):
            for name in engines:
                once(engines[name])
        ev = {name: [] for name in engines}
        for _ in range(a.steps):
            for name in engines:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                once(engines[name])
                e1.record(st)
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ev.items()}
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        launches = a.steps + a.warmup
        # the invariant: sum(table) == Undetermined; and the pairs are where the fill put them
        table = engines["hop"].hop_read()
        und = int(engines["hop"].counts()[3])
        assert int(table.sum()) == und, (int(table.sum()), und)
        inner = table[:-1].reshape(n1 + 1, n2 + 1)
        assert not inner[part1, part2].any(), "an on-sheet cell is not 0"
        if cells is not None:
            assert sum(int(inner[c]) for c in cells) == und, (kind, und)
        else:
            assert int(inner[:n1, :n2].sum()) == und, (kind, und)
        stats = [int(x) for x in engines["tally"].unknown_stats()]
        assert stats[0] + stats[1] + stats[2] == int(engines["tally"].counts()[3])
        return {"fill": kind, "off_median_ms": med["off"], "hop_median_ms": med["hop"], "tally_median_ms": med["tally"],
                "hop_ms": med["hop"] - med["off"], "tally_ms": med["tally"] - med["off"],
                "target_met": bool(med["hop"] - med["off"] <= med["tally"] - med["off"]),
                "off_min_ms": ms["off"][0], "off_max_ms": ms["off"][-1], "hop_min_ms": ms["hop"][0], "hop_max_ms": ms["hop"][-1],
                "tally_min_ms": ms["tally"][0], "tally_max_ms": ms["tally"][-1], "undetermined_per_launch": und // launches,
                "cells_used": int(np.count_nonzero(inner)), "tally_distinct": stats[3], "tally_dropped": stats[2]}

    out = {"tool": "hop_bench", "device": engines["hop"].device_info()["name"], "config": "cfg3, 96 samples, 10 % Undetermined",
           "pairs_per_launch": n, "n1": n1, "n2": n2, "tally_slots": a.slots, "steps": a.steps,
           "fills": [measure(kind) for kind in ((a.fill,) if a.fill else FILLS)]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
