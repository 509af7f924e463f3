#!/usr/bin/env python3
"""End-to-end rate: synthetic 2x150 bp fastq.gz chunks in -> per-sample fastq.gz + report out through
the CLI driver.  Host bound (gunzip, scan, format, gzip); printed as one JSON line.
usage: python tools/e2e_bench.py [pairs] [gzip level] [chunks] [--single-member | --members] [--binned] [--ranks N]
input files: BGZF (bgzip layout) by default, --members = 8 MB gzip members, --single-member = one gzip member
env: E2E_PARALLEL_GUNZIP (1; 0 = ordinary gzip files on one thread each), E2E_GUNZIP_CHUNK, E2E_GUNZIP_IN_FLIGHT, E2E_DEVICE_INFLATE (0; 1 = BGZF inflate on the GPU), E2E_DEVICE_DEFLATE (0; 1 = Huffman-only members made on the GPU, level -1), E2E_WORKERS (chunk_workers), E2E_IO_THREADS, E2E_SAMPLES (96), E2E_BATCH (the driver's default), E2E_DEVICE_PIPELINE (1; 0 = batch pipeline over pinned slots), E2E_MISMATCHES ("m1,m2": [index] index1_mismatches / index2_mismatches; unset = exact matching), E2E_UNKNOWN (N: [output] top_unknown_barcodes; unset = no tally), E2E_HOPPING (1: [output] index_hopping_report : True; unset = no matrix), E2E_QUALITY (1: [output] quality_report : True; unset = no counters), E2E_CYCLE (1: [output] cycle_report : True; unset = no per-cycle counters), E2E_ADAPTERS (1: [output] adapter_report : True with the built-in probes; unset = no adapter content), E2E_TRIM (1: a [trim] section with quality_cutoff 20 and the two TruSeq adapters; unset = no trimming), E2E_PAIRTRIM (1: [trim] pair_overlap : True with its defaults; unset = no overlap trimming), E2E_PAIRCORRECT (1, with E2E_PAIRTRIM: [trim] pair_correct : True with its defaults; unset = no overlap base correction), E2E_CLIP (1: [trim] tail_clip_R1 / tail_clip_R2 : 1, window_size 4 with window_quality 20 and poly_g : True; unset = no clipping), E2E_POSTTRIM (1: [trim] tail_n and poly_x : True and max_length_R1 / max_length_R2 : 140; unset = no post-trimming), E2E_FILTER (1: a [filter] section with min_length 30, max_n 5, max_unqualified_pct 40, min_mean_quality 20 and min_complexity_pct 30; unset = no filter), E2E_SCREEN (1: a [screen] section with a seeded random 5 386-base reference written next to the conf, kmer 31 and action report; "drop": action drop; unset = no screen), E2E_DUP (1: [output] duplication_report : True at duplication_sample E2E_DUP_SAMPLE (16); the JSON line then has the wall time of the end-of-run gather and merge; unset = no tally), QUADE_PROFILE=1 (stage timers)"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quade_amd import synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
level = int(args[1]) if len(args) > 1 else 1
n_chunks = int(args[2]) if len(args) > 2 else 1  # the same files listed n_chunks times
single = "--single-member" in sys.argv
fmt = 0 if single else ((8 << 20) if "--members" in sys.argv else "bgzf")
ranks = int(sys.argv[sys.argv.index("--ranks") + 1]) if "--ranks" in sys.argv else 1
workers = int(os.environ.get("E2E_WORKERS", "1"))
io_thr = int(os.environ.get("E2E_IO_THREADS", "0"))
n_samples = int(os.environ.get("E2E_SAMPLES", "96"))
batch = int(os.environ.get("E2E_BATCH", "0"))  # 0: the driver's default (2 M pairs through the device pipeline, 500 k over pinned slots)
dev_pipe = os.environ.get("E2E_DEVICE_PIPELINE", "1") not in ("0", "false", "False")
work = tempfile.mkdtemp(prefix="quade_e2e_")
from quade_amd import hip_backend as _hb  # noqa: E402
for _name, _env in (("parallel_gunzip", "E2E_PARALLEL_GUNZIP"), ("gunzip_chunk_bytes", "E2E_GUNZIP_CHUNK"), ("gunzip_in_flight", "E2E_GUNZIP_IN_FLIGHT"),
                    ("bgzf_in_flight", "E2E_BGZF_IN_FLIGHT"), ("bgzf_device_lanes", "E2E_BGZF_DEVICE_LANES"),
                    ("bgzf_device_run_bytes", "E2E_BGZF_DEVICE_RUN_BYTES")):
    if os.environ.get(_env):  # ordinary gzip inputs: the parallel inflater on / off, its chunk size, chunks in flight per file
        assert _hb.load_library().qd_io_set_option(_name.encode(), int(os.environ[_env])) == 0
try:
    t0 = time.perf_counter()
    quals = "binned" if "--binned" in sys.argv else "uniform"  # --binned: insert-read qualities as current instruments write them
    paths, bcs = synth.write_fastq_dataset(work, n, n_samples=n_samples, member_bytes=fmt, qualities=quals)
    t_gen = time.perf_counter() - t0
    conf = os.path.join(work, "conf.txt")
    dev_inflate = os.environ.get("E2E_DEVICE_INFLATE", "0") not in ("0", "false", "False")
    dev_deflate = os.environ.get("E2E_DEVICE_DEFLATE", "0") not in ("0", "false", "False")  # gzip level -1 only
    synth.write_conf(conf, paths, bcs, n_chunks, gpu="[gpu]\n%sgzip_level : %d\nchunk_workers : %d\nio_threads : %d\ndevice_inflate : %s\ndevice_deflate : %s\ndevice_pipeline : %s\n"
                     % ("batch_pairs : %d\n" % batch if batch else "", level, workers, io_thr, dev_inflate, dev_deflate, dev_pipe))
    mm = os.environ.get("E2E_MISMATCHES")
    if mm:  # mismatch budgets in the [index] section
        m1, m2 = (int(x) for x in mm.split(","))
        with open(conf) as fh:
            text = fh.read().replace("index2_end : 8\n", "index2_end : 8\nindex1_mismatches : %d\nindex2_mismatches : %d\n" % (m1, m2), 1)
        with open(conf, "w") as fh:
            fh.write(text)
    unk = os.environ.get("E2E_UNKNOWN")
    if unk:  # the report of the top unknown barcodes in the [output] section
        with open(conf) as fh:
            text = fh.read().replace("[output]\n", "[output]\ntop_unknown_barcodes : %d\n" % int(unk), 1)
        with open(conf, "w") as fh:
            fh.write(text)
    hopping = os.environ.get("E2E_HOPPING", "0") not in ("", "0")
    if hopping:  # the index-hopping report in the [output] section
        with open(conf) as fh:
            text = fh.read().replace("[output]\n", "[output]\nindex_hopping_report : True\n", 1)
        with open(conf, "w") as fh:
            fh.write(text)
    cycle = os.environ.get("E2E_CYCLE", "0") not in ("", "0")
    if cycle:  # the per-cycle report in the [output] section
        with open(conf) as fh:
            text = fh.read().replace("[output]\n", "[output]\ncycle_report : True\n", 1)
        with open(conf, "w") as fh:
            fh.write(text)
    adapters = os.environ.get("E2E_ADAPTERS", "0") not in ("", "0")
    if adapters:  # the adapter content report in the [output] section
        with open(conf) as fh:
            text = fh.read().replace("[output]\n", "[output]\nadapter_report : True\n", 1)
        with open(conf, "w") as fh:
            fh.write(text)
    quality = os.environ.get("E2E_QUALITY", "0") not in ("", "0")
    if quality:  # the yield and quality report in the [output] section
        with open(conf) as fh:
            text = fh.read().replace("[output]\n", "[output]\nquality_report : True\n", 1)
        with open(conf, "w") as fh:
            fh.write(text)
    dup = int(os.environ.get("E2E_DUP_SAMPLE", "16")) if os.environ.get("E2E_DUP", "0") not in ("", "0") else 0
    if dup:  # the duplication report in the [output] section, at duplication_sample E2E_DUP_SAMPLE
        with open(conf) as fh:
            text = fh.read().replace("[output]\n", "[output]\nduplication_report : True\nduplication_sample : %d\n" % dup, 1)
        with open(conf, "w") as fh:
            fh.write(text)
    trim = os.environ.get("E2E_TRIM", "0") not in ("", "0")
    if trim:  # 3' trimming of the insert reads: a [trim] section behind everything else
        with open(conf, "a") as fh:
            fh.write("\n[trim]\nquality_cutoff : 20\nadapter_R1 : AGATCGGAAGAGCACACGTCTGAACTCCAGTCA\nadapter_R2 : AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT\n")
    pairtrim = os.environ.get("E2E_PAIRTRIM", "0") not in ("", "0")
    if pairtrim:  # paired-end overlap trimming: into the [trim] section, which is the file's last when E2E_TRIM made one
        with open(conf, "a") as fh:
            fh.write(("" if trim else "\n[trim]\n") + "pair_overlap : True\n")
    paircorrect = os.environ.get("E2E_PAIRCORRECT", "0") not in ("", "0")
    if paircorrect:  # overlap base correction behind it: into the same [trim] section (the conf is rejected without pair_overlap)
        with open(conf, "a") as fh:
            fh.write(("" if trim or pairtrim else "\n[trim]\n") + "pair_correct : True\n")
    clip = os.environ.get("E2E_CLIP", "0") not in ("", "0")
    if clip:  # end clipping, window and poly-G trimming: into the [trim] section, the file's last when one of the two above made it
        with open(conf, "a") as fh:
            fh.write(("" if trim or pairtrim or paircorrect else "\n[trim]\n") + "tail_clip_R1 : 1\ntail_clip_R2 : 1\nwindow_size : 4\nwindow_quality : 20\npoly_g : True\n")
    posttrim = os.environ.get("E2E_POSTTRIM", "0") not in ("", "0")
    if posttrim:  # trailing-N, poly-X and max_length trimming: into the [trim] section, the file's last when one of the three above made it
        with open(conf, "a") as fh:
            fh.write(("" if trim or pairtrim or paircorrect or clip else "\n[trim]\n") + "tail_n : True\npoly_x : True\nmax_length_R1 : 140\nmax_length_R2 : 140\n")
    filt = os.environ.get("E2E_FILTER", "0") not in ("", "0")
    if filt:  # read filtering: a [filter] section behind everything else
        with open(conf, "a") as fh:
            fh.write("\n[filter]\nmin_length : 30\nmax_n : 5\nmax_unqualified_pct : 40\nmin_mean_quality : 20\nmin_complexity_pct : 30\n")
    screen = os.environ.get("E2E_SCREEN", "0")
    screen = "" if screen in ("", "0") else "drop" if screen == "drop" else "report"
    if screen:  # the k-mer screen: a [screen] section behind everything else, over a seeded random reference of PhiX's size
        import random
        rnd = random.Random(5386)
        with open(os.path.join(work, "reference.fa"), "w") as fh:
            fh.write(">random\n" + "".join(rnd.choice("ACGT") for _ in range(5386)) + "\n")
        with open(conf, "a") as fh:
            fh.write("\n[screen]\nreference : %s\nkmer : 31\nmin_hits : 1\naction : %s\n" % (os.path.join(work, "reference.fa"), screen))
    out = os.path.join(work, "out")
    os.mkdir(out)
    os.chdir(out)
    pipe_stats = None
    if ranks > 1:  # one process per GPU; on a 1-GPU box all ranks share GPU 0 and the counts go through files
        env = dict(os.environ, PYTHONPATH=ROOT)
        if os.environ.get("E2E_SHARE_GPU0"):
            env.update(QUADE_DIST_TRANSPORT="files", QUADE_DEVICE="0")
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-m", "quade_amd.launch", "-n", str(ranks), "-c", conf], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        dt = time.perf_counter() - t0
        cpu_s = None
        assert r.returncode == 0, r.stdout[-2000:]
        with open("Quade_report.csv") as fh:
            counts = [int(ln.split("\t")[1]) for ln in fh.read().split("\n")[2:6]]
    else:
        from quade_amd.quade import Quade
        from quade_amd.sample import Sample
        import ctypes as _C
        _lib = _hb.load_library()
        _names, _secs = (_C.c_char_p * 32)(), (_C.c_double * 32)()
        _lib.qd_io_stage_seconds(None, None, 0, 1)  # reset: the dataset was written through the same pool
        c0 = os.times()
        t0 = time.perf_counter()
        _q = Quade(conf_file=conf)
        _q()
        dt = time.perf_counter() - t0
        c1 = os.times()
        if os.environ.get("QUADE_PROFILE"):  # thread-CPU seconds of the library's stages (all threads)
            k = _lib.qd_io_stage_seconds(_names, _secs, 32, 0)
            tot = (c1.user - c0.user) + (c1.system - c0.system)
            cpu_sum = 0.0
            for i in range(k):
                nm = _names[i].decode()
                if "count / 1e9" in nm:
                    print("\t[n]   %-60s %d" % (nm.replace(" (count / 1e9)", ""), round(_secs[i] * 1e9)))
                elif "WALL" in nm:
                    print("\t[wall] %-59s %7.2f s" % (nm, _secs[i]))
                else:
                    cpu_sum += _secs[i]
                    print("\t[cpu] %-44s %7.2f s  %5.2f core-s per M pairs" % (nm, _secs[i], _secs[i] / (n * n_chunks / 1e6)))
            print("\t[cpu] %-44s %7.2f s  %5.2f core-s per M pairs (python main thread, index packing, tags, unaccounted)"
                  % ("everything else", tot - cpu_sum, (tot - cpu_sum) / (n * n_chunks / 1e6)))
        cpu_s = (c1.user - c0.user) + (c1.system - c0.system)  # every thread of this process (readers, pool, main)
        cpu_user, cpu_sys = c1.user - c0.user, c1.system - c0.system
        counts = Sample.COUNTS()[:4]
        pipe_stats = getattr(_q, "pipe_stats", None)
    from quade_amd.fastq_writer import host_cores, io_backend, io_threads
    print(json.dumps({"mode": "end-to-end fastq.gz -> fastq.gz", "chunks": n_chunks, "pairs": n * n_chunks, "seconds": dt,
                      "pairs_per_s": n * n_chunks / dt, "gzip_level": level, "counts": counts, "chunk_workers": workers,
                      "ranks": ranks, "qualities": quals, "device_inflate": dev_inflate, "device_deflate": dev_deflate, "device_pipeline": dev_pipe and ranks == 1 and pipe_stats is not None, "pipeline": pipe_stats if ranks == 1 else None, "parallel_gunzip": os.environ.get("E2E_PARALLEL_GUNZIP", "1") != "0", "samples": n_samples, "batch_pairs": batch, "mismatches": mm, "top_unknown_barcodes": unk, "index_hopping_report": hopping, "quality_report": quality, "cycle_report": cycle, "adapter_report": adapters, "duplication_sample": dup or None, "duplication_merge_seconds": getattr(_q, "dup_merge_seconds", None) if ranks == 1 else None, "trim": trim, "pair_trim": pairtrim, "pair_correct": paircorrect, "clip": clip, "posttrim": posttrim, "filter": filt, "screen": screen or None, "input": {0: "single gzip member", "bgzf": "BGZF"}.get(fmt, "8 MB gzip members"), "gzip_backend": io_backend(),
                      "io_threads": io_threads(), "host_cores": host_cores(), "host_logical_cpus": os.cpu_count(), "dataset_seconds": round(t_gen, 1),
                      "cpu_seconds": cpu_s, "cpu_user_sys": [round(cpu_user, 2), round(cpu_sys, 2)] if cpu_s else None, "cpu_seconds_per_M_pairs": cpu_s / (n * n_chunks / 1e6) if cpu_s else None,
                      "core_utilisation": cpu_s / (dt * host_cores()) if cpu_s else None}))
finally:
    os.chdir("/")
    shutil.rmtree(work, ignore_errors=True)
