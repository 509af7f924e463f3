#!/usr/bin/env python3
"""Cost of the overlap trimming kernel (qd_pairtrim_set, quade_pairtrim.hip) over resident text: one batch of the device pipeline
-- 2 M pairs of 2 x 150 bp insert reads as fastq text in HBM with their record tables -- run through the kernel qd_pipe_run
launches (the defaults: pair_min_overlap 30, pair_max_mismatches 5, pair_max_mismatch_pct 20).  Two contexts on one device, one
with the stage off and one with it on, take the same batch; their calls alternate on one stream (off, on, off, on, ...) and each
is timed by HIP events: "off" asks qd_pairtrim_active as the pipeline does, launches nothing and shows what the timing itself
costs.  Four batches: 0 %, 10 % and 100 % of the pairs come from an insert of 30 .. 149 bases (the others are unrelated reads: every
candidate is tried and fails), and a low-complexity batch (poly-A against poly-T: every candidate matches, the first is compared
in full).  Prints one JSON line: per batch the medians off and on, the spread of both, and the byte floor (reading the two
sequence lines once at 6.3 TB/s).

Reads of more than 321 bases do not fit the kernel's LDS slab and take its byte loop over global memory: `--bases 400` (with fewer
pairs) times that path; the inserts then lie in 30 .. 399.

usage: python tools/pairtrim_bench.py [--pairs N] [--bases L] [--steps K] [--warmup W] [--once CASE] [--out FILE]
  --once CASE  set up the batch CASE (0, 10, 100 or poly), run ONE launch and exit (for `rocprofv3 --kernel-trace --stats -- python ...`)
The end-to-end rates come from tools/e2e_bench.py with E2E_PAIRTRIM=1 against none."""
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


def make_pairs(n, L, seed, case):
    """-> (R1, R2) base codes uint8[n, L] on the device (0 .. 3 = A C G T); case: the percentage of pairs read from an insert of
    30 .. L - 1 bases, or "poly" """
    g = torch.Generator(device="cuda").manual_seed(seed)
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


def make_text(codes, seed):
    """n records "@<20-byte name>\\n<L bases>\\n+\\n<L qualities>\\n" on the device and their record table (6 uint32 each)"""
    n, L = codes.shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    rec = 1 + 20 + 1 + L + 1 + 2 + L + 1
    t = torch.empty((n, rec), dtype=torch.uint8, device="cuda")
    t[:, 0] = ord("@")
    t[:, 1:21] = torch.randint(48, 58, (n, 20), generator=g, device="cuda", dtype=torch.uint8)
    t[:, 21] = 10
    t[:, 22:22 + L] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[codes]
    t[:, 22 + L] = 10
    t[:, 23 + L] = ord("+")
    t[:, 24 + L] = 10
    t[:, 25 + L:25 + 2 * L] = torch.randint(35, 74, (n, L), generator=g, device="cuda", dtype=torch.uint8)
    t[:, 25 + 2 * L] = 10
    head = torch.arange(n, device="cuda", dtype=torch.int64) * rec
    recs = torch.stack([head, head + 1, torch.full_like(head, 20), head + 22, torch.full_like(head, L), head + 25 + L], dim=1)
    assert n * rec < 1 << 31
    return t.reshape(-1), recs.to(torch.int32).contiguous()


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
    launch, active = lib.qd_pairtrim_device, lib.qd_pairtrim_active  # the pipeline's internal entries: device pointers and a stream
    launch.restype = active.restype = C.c_int
    launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    active.argtypes = [C.c_void_p]
    st = torch.cuda.current_stream()
    engines = {"off": hb.Engine(0), "on": hb.Engine(0)}
    engines["on"].pairtrim_set()
    floor_ms = 2.0 * n * L / COPY_RATE * 1e3

    def measure(case):
        c1, c2 = make_pairs(n, L, 1, case)
        t1, r1 = make_text(c1, 2)
        t2, r2 = make_text(c2, 3)
        del c1, c2
        o1, o2 = torch.empty_like(r1), torch.empty_like(r2)

        def once(eng):
            if active(eng._h):  # (what process_batch does)
                rc = launch(eng._h, t1.data_ptr(), r1.data_ptr(), t2.data_ptr(), r2.data_ptr(), n, o1.data_ptr(), o2.data_ptr(), st.cuda_stream)
                assert rc == 0, rc

        if a.once is not None:
            once(engines["on"])
            torch.cuda.synchronize()
            return {"once": case, "pairs": n, "bases": L}
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
        reads, pairs, hist = hb.split_pairtrim(engines["on"].pairtrim_read())
        launches = a.steps + a.warmup
        assert pairs[0] == reads[0][0] == reads[1][0] == launches * n and reads[0][1] == reads[1][1] == launches * n * L
        assert sum(hist) == pairs[1] and (o1[:, [0, 1, 2, 3, 5]] == r1[:, [0, 1, 2, 3, 5]]).all() and int(o1[:, 4].max()) <= L
        if case != "poly":  # an unrelated pair is next to never accepted, an insert always found
            assert abs(pairs[2] / pairs[0] - case / 100.0) < 0.01, pairs
        return {"case": case, "off_median_ms": ms["off"][len(ms["off"]) // 2], "on_median_ms": ms["on"][len(ms["on"]) // 2],
                "off_min_ms": ms["off"][0], "off_max_ms": ms["off"][-1], "on_min_ms": ms["on"][0], "on_max_ms": ms["on"][-1],
                "byte_floor_ms": floor_ms, "on_over_floor": ms["on"][len(ms["on"]) // 2] / floor_ms,
                "overlapped_pair_share": pairs[1] / pairs[0], "short_insert_pair_share": pairs[2] / pairs[0],
                "mean_bases_out": (reads[0][2] + reads[1][2]) / (2.0 * pairs[0])}

    if a.once is not None:
        print(json.dumps(measure(a.once if a.once == "poly" else int(a.once))))
        for eng in engines.values():
            eng.close()
        return
    out = {"tool": "pairtrim_bench", "device": torch.cuda.get_device_name(0), "pairs_per_launch": n, "bases_per_read": L,
           "line_bytes": 2 * n * L, "steps": a.steps, "params": engines["on"].pairtrim_get(),
           "batches": [measure(case) for case in (0, 10, 100, "poly")]}
    for eng in engines.values():
        eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
