# -*- coding: utf-8 -*-
"""
Configuration file handling: the schema of Quade 0.3.2's Quade_conf_file.txt, re-expressed for
Python 3.  Parsing and validation follow src/Quade.py:92-142 and 258-284 of the reference (same
sections, option names, 1-based -> 0-based start conversion, assertion messages); the example
file written by `-i` is the reference's template byte for byte (src/Conf_file.py:18-104; shipped as
package data, quade_amd/data/Quade_conf_file.txt).  An optional [gpu] section that reference conf
files simply do not have is read when present (defaults apply otherwise; see GPU_SECTION_HELP), and so are the optional
mismatch budgets of the [index] section (MISMATCH_HELP), the unknown-barcode report (UNKNOWN_HELP), the index-hopping report (HOPPING_HELP) and the quality report
(QUALITY_HELP), the per-cycle report (CYCLE_HELP), the adapter content report (ADAPTER_HELP) and the duplication report (DUPLICATION_HELP) of the [output] section, an optional [trim] section (CLIP_HELP, TRIM_HELP, PAIR_HELP, CORRECT_HELP, POSTTRIM_HELP), an optional [filter] section
(FILTER_HELP) and an optional [screen] section (SCREEN_HELP).
"""
from __future__ import annotations

import configparser
import os
import zlib

CONF_NAME = "Quade_conf_file.txt"

TEMPLATE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", CONF_NAME)

GPU_SECTION_HELP = """\
Optional [gpu] section (not in Quade 0.3.2; a conf file without it runs with the defaults):
  [gpu]
  devices : 0            GPUs to use: "all" or a blank separated list of device ids
  device_pipeline : True the whole chunk loop on the GPU (libquade_hip qd_pipe_run): BGZF blocks inflated, records found, index rows
                         packed and matched, records scattered by routing code, formatted, CRC-32'd and coded into gzip members with
                         the fastq text staying in device memory; only compressed bytes cross PCIe (17-21 M pairs/s at 0.06-0.12
                         core-s per M pairs on one MI355X).  Needs device_inflate, device_deflate and gzip_level 1 or -1 (one pipeline per device
                         and chunk worker, chunks dealt out); anything else runs the batch pipeline over pinned slots (7 M pairs/s at 1.5).
                         Inputs that are not BGZF are inflated by the host's threads and join the device path as text
  shard_chunks : auto    under a launcher (one process per GPU): a chunk is cut into pair ranges over ALL ranks -- auto: when there are
                         fewer chunks than ranks, True: always, False: never (chunk c belongs to rank c mod N).  Needs the device
                         pipeline and BGZF inputs (an index pass counts lines and kept records per block range, so that pair j is
                         still record j of every stream); other chunks stay with one rank
  batch_pairs : 2000000  read pairs per device batch (device pipeline; its buffers are sized from it: ~25 GB of the GPU's 288 at
                         2x150 bp); 500000 over pinned slots (host memory in flight grows with it: ~3 GB at 2x150 bp)
  slots : 3              pinned staging slots per device (pinned-slots path: H2D / kernel / D2H overlap)
  gzip_level : 1         deflate level of the output fastq.gz files (0-9; -1 = Huffman coding only).  1, the default, is
                         the level the GPU codes itself: files about the size of libdeflate's level 6 on records with binned
                         qualities (21.0 % of the text; level 6: 19.2 %, level 1: 20.9 %), between its levels 6 and 1 on uniformly
                         random ones (41.9 %; 40.3 / 43.2 %); levels 2-9 are libdeflate on the host's pool (level 6: 1.6 M pairs/s).
                         The device's level-1 files are not byte-reproducible from run to run (their decompressed content is).
                         The reference writes with Python's gzip default (9); only the decompressed bytes are its format
  chunk_workers : 1      chunks processed concurrently (a pipeline / a slot set each; outputs identical)
  io_threads : 0         threads of the native I/O pool (0 = one per core)
  device_deflate : True  with gzip_level -1 or 1: the output members are made on the GPU (-1: Huffman coding only; 1: LZ77 + Huffman,
                         one workgroup per 64 KiB of formatted text); no effect at the other levels
  device_inflate : True  BGZF (bgzip) input files are inflated on the GPU, one workgroup of 512-1024 lanes per block (every block's
                         CRC-32 is checked against its trailer; a block the device refuses is inflated by the host); ordinary gzip
                         files are inflated by the host's threads whatever this says
"""

MISMATCH_HELP = """\
Optional [index] options (not in Quade 0.3.2, whose parser ignores them; absent = 0 = exact matching as the reference):
  index1_mismatches : 0  substitutions tolerated in index read 1's part of the barcode: 0, 1 or 2
  index2_mismatches : 0  the same for index read 2's part: 0, 1 or 2 (ignored when index2 is False)
A read whose barcode slice has no exact match goes to the one sample whose barcode is within both budgets (N counts as an
ordinary base).  Two samples whose barcodes are within 2 x index1_mismatches and 2 x index2_mismatches of each other collide:
the configuration is rejected before any read is processed.
"""

UNKNOWN_HELP = """\
Optional [output] option (not in Quade 0.3.2, whose parser ignores it; absent or empty = 0 = no report):
  top_unknown_barcodes : 0  0 to 1000: write Quade_unknown_barcodes.csv with the N most frequent barcodes of the Undetermined
                            pairs (index1_seq, index2_seq, count, percent of Undetermined, the nearest sample and its distance
                            per index read).  The barcodes are counted on the GPU, in a table of [gpu] unknown_slots entries
Optional [gpu] option:
  unknown_slots : 16777216  entries of that table per context: a power of two, 1024 to 268435456 (48 bytes each).  Barcodes that
                            find no room are counted as "Not tallied" in the report's head
"""

HOPPING_HELP = """\
Optional [output] option (not in Quade 0.3.2, whose parser ignores it; absent, empty or False = no report):
  index_hopping_report : False  True: write Quade_index_hopping_report.csv next to the report.  Needs index2 : True.  With K the
                            width of the fused barcode, w1 the width of index 1's window and w2 = K - w1: take the samples whose
                            barcode is K long, in sheet order (the others are "off the matrix"); the distinct values of their
                            first w1 bases, in order of first appearance, are the n1 index-1 values, the distinct values of
                            their last w2 bases the n2 index-2 values.  Every pair that ends Undetermined (after the exact match
                            and the mismatch rescue) is counted on the GPU in the cell (a, b) of a table of (n1+1) x (n2+1)
                            cells: a = the index-1 value its index 1 slice equals after upper-casing, or "none", b the same for
                            index 2 (N and any other byte are ordinary symbols); a pair with a read that ends inside its index
                            window counts as "short index slice" instead.  A cell with both parts known is an unexpected
                            combination -- index hopping, or a combination missing from the sheet -- and
                            unexpected_per_100000 = both known * 100000 // (assigned + both known).  Matching per part is
                            exact whatever the mismatch budgets are (a tolerant match per part is not unique): with a budget
                            above 0 the rates are lower bounds, and the report says so.  The per-sample rows give the pairs that
                            carry the sample's index 1 with another known index 2, its index 2 with another known index 1, and
                            either with an unknown partner; in a combinatorial sheet the samples that share an index value
                            share that sum.  At most 10000 combinations are listed.  (n1+1) x (n2+1) may not exceed 16777216
                            (4095 distinct values per index read); the report works on every path and [gpu] configuration
"""

HOPPING_NEEDS = "index_hopping_report needs a dual index (index2 : True)"
HOPPING_TOO_MANY = "index_hopping_report : (distinct index1 + 1) x (distinct index2 + 1) may not exceed 16777216"

QUALITY_HELP = """\
Optional [output] option (not in Quade 0.3.2, whose parser ignores it; absent, empty or False = no report):
  quality_report : False    True: write Quade_quality_report.csv next to the report -- for every destination (<sample>_pass,
                            <sample>_fail, Undetermined, Total) and for R1 and R2: reads, bases, mean length, bases at or above
                            Q20 and Q30 (Phred+33) with their percentages, mean quality, N bases and their percentage.  A
                            destination whose write flag is off is counted all the same.  The reads are counted on the GPU while
                            the device pipeline holds their text, so the option needs the device pipeline: [gpu] device_pipeline,
                            device_inflate and device_deflate True (the defaults) and gzip_level 1 or -1
"""

QUALITY_NEEDS = "quality_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"

CYCLE_HELP = """\
Optional [output] option (not in Quade 0.3.2, whose parser ignores it; absent, empty or False = no report):
  cycle_report : False      True: write Quade_cycle_report.csv next to the report -- for the groups pass, fail, Undetermined and
                            Total and for R1 and R2: per cycle (up to 1024) the reads, A, C, G, T, N and other bases, GC percent,
                            mean quality and the bases at or above Q20 and Q30 (Phred+33) with their percentages; then the
                            distributions of read length, per-read mean quality and per-read GC percent.  The reads are those
                            the output stages see (behind [trim], pair_overlap and [filter]), whatever the write flags say:
                            the reads quality_report counts.  They are counted on the GPU while the device pipeline holds their
                            text, so the option needs the device pipeline: [gpu] device_pipeline, device_inflate and
                            device_deflate True (the defaults) and gzip_level 1 or -1
"""

CYCLE_NEEDS = "cycle_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"

ADAPTER_HELP = """\
Optional [output] options (not in Quade 0.3.2, whose parser ignores them; absent, empty or False = no report):
  adapter_report : False    True: write Quade_adapter_report.csv next to the report -- which known adapters start where in R1 and
                            R2: for every probe and for any of them the reads that hold it and their share per 100000, the most
                            frequent one (top_adapter_R1, top_adapter_R2), the cumulative content by position (the curve FastQC
                            draws) and the counts per destination (<sample>_pass, <sample>_fail, Undetermined, Total).  A probe is
                            the first 12 bases of an adapter; a read holds it where 12 consecutive bases equal it, either case,
                            and an N matches nothing.  The built-in probes are illumina_universal AGATCGGAAGAG,
                            illumina_small_rna_3p TGGAATTCTCGG, illumina_small_rna_5p GATCGTCGGACT, nextera_transposase
                            CTGTCTCTTATA, poly_a and poly_g; [trim] adapter_R1 and adapter_R2 join them under those names when
                            set.  The report describes the library, not what the trimmers left: it is the only stage that counts
                            the RAW insert reads, as they are in the input files -- in front of the clipping, [trim],
                            pair_overlap, the post-trimming, [filter] and [screen] -- and every pair the run routes, whatever the
                            write flags say and whatever the filter or the screen drop later.  Read it before choosing
                            adapter_R1, poly_g or poly_x.  The reads are searched on the GPU while the device pipeline holds
                            their text, so the option needs the device pipeline: [gpu] device_pipeline, device_inflate and
                            device_deflate True (the defaults) and gzip_level 1 or -1
  adapter_report_extra :    NAME=SEQ;NAME=SEQ... further probes: a name is letters, digits and _ and differs from every other
                            name, the probe is the first 12 bases of SEQ.  A sequence shorter than 12 bases or whose first 12
                            are not all A, C, G or T is left off, one whose probe equals an earlier probe is an alias of it: the
                            report lists both.  At most 16 distinct probes in all.  Without adapter_report the option does nothing
"""

ADAPTER_NEEDS = "adapter_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
ADAPTER_EXTRA = "adapter_report_extra : NAME=SEQ;NAME=SEQ... with names of letters, digits and _ that differ from every other probe's name"
ADAPTER_TOO_MANY = "adapter_report : more than 16 distinct probes (6 built in, adapter_R1, adapter_R2 and adapter_report_extra)"
ADAPTER_SHORT = "shorter than 12 bases"
ADAPTER_NOT_ACGT = "the first 12 bases are not all A, C, G or T"

DUPLICATION_HELP = """\
Optional [output] options (not in Quade 0.3.2, whose parser ignores them; absent, empty or False = no report):
  duplication_report : False  True: write Quade_duplication_report.csv next to the report -- for every destination (<sample>_pass,
                            <sample>_fail, Undetermined) and Total: the pairs, those too short or with an N to be keyed, the keyed,
                            sampled and tallied pairs, the distinct keys, duplicate_pairs = tallied - distinct and their percentage;
                            then how many keys and pairs of the run occur once, twice, ... (levels 1 to 31 and >=32).  A pair's
                            key is the first duplication_bases bases of R1 and of R2 (case folded; A, C, G, T only) and its
                            destination: equal sequences in two destinations are two keys, duplicates are a per-library matter.
                            The pairs are those the output stages see (behind [trim], pair_overlap and [filter]), whatever the
                            write flags say: the pairs quality_report counts.  They are counted on the GPU, in a hash table that
                            every batch feeds, so the option needs the device pipeline: [gpu] device_pipeline, device_inflate and
                            device_deflate True (the defaults) and gzip_level 1 or -1
  duplication_bases : 32    8 to 32: a pair whose R1 or R2 is shorter is counted as short, one with another letter among these
                            bases as with_n; neither is keyed
  duplication_sample : 16   a power of two, 1 to 1024: one key in this many is counted (chosen by a hash of the key, so a counted
                            key keeps its exact multiplicity and every GPU and rank counts the same keys).  Rates over the sample
                            are unbiased estimates of the library's; 1 counts every key
Optional [gpu] option:
  duplicate_slots : 16777216  entries of the hash table per context: a power of two, 1024 to 268435456 (48 bytes each).  Pairs
                            whose key finds no room are counted as not_tallied
"""

DUPLICATION_NEEDS = "duplication_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
DUPLICATION_BASES = "Authorized values for duplication_bases : 8 to 32"
DUPLICATION_SAMPLE = "Authorized values for duplication_sample : a power of two, 1 to 1024"
DUPLICATION_SLOTS = "[gpu] duplicate_slots : a power of two, 1024 to 268435456"

TRIM_HELP = """\
Optional [trim] section (not in Quade 0.3.2, whose parser ignores it; absent = the insert reads leave as they came): 3' trimming of
the insert reads on the GPU.  Index reads, names and the :IDX[:MOL] tag are never touched.  In this order:
  quality_cutoff : 0        1 to 93: cut the low-quality 3' tail (cutadapt's / BWA's rule: walking from the 3' end, the position
                            where the running sum of cutoff - Phred is largest, stopping once it turns negative); 0 = off
  adapter_R1 :              1 to 64 letters of ACGT: cut the read at the leftmost position from which it matches the start of the
  adapter_R2 :              adapter up to the read's end (substitutions only; N and any other byte is a mismatch); empty = none
  min_overlap : 3           1 to 64 and not above a set adapter's length: shorter overlaps at the 3' end are left alone
  max_mismatch_pct : 10     0 to 50: an overlap of ov bases may hold ov * max_mismatch_pct // 100 mismatches
  min_length : 0            0 to 65535: a read is never cut below min(min_length, its length)
Trimming is on when an adapter is set or quality_cutoff > 0; Quade_trim_report.csv is then written next to the report.  The
reads are trimmed while the device pipeline holds their text, so the section needs the device pipeline: [gpu] device_pipeline,
device_inflate and device_deflate True (the defaults) and gzip_level 1 or -1
"""

TRIM_NEEDS = "[trim] needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
TRIM_ADAPTER = "Authorized values for adapter_R1 and adapter_R2 : 1 to 64 letters of ACGT"
TRIM_CUTOFF = "Authorized values for quality_cutoff : 0 to 93"
TRIM_OVERLAP = "Authorized values for min_overlap : 1 to 64, and not above the length of a set adapter"
TRIM_MISMATCH = "Authorized values for max_mismatch_pct : 0 to 50"
TRIM_LENGTH = "Authorized values for min_length : 0 to 65535"

CLIP_HELP = """\
Optional [trim] options (not in Quade 0.3.2, whose parser ignores them; absent = as before): end clipping, sliding-window quality
trimming and poly-G tail trimming of the insert reads on the GPU, in front of the 3' trimming above (fastp's order: fixed
trimming, cut_right, poly-G, then adapters).  Index reads, names and the :IDX[:MOL] tag are never touched.  In this order:
  front_clip_R1 : 0         0 to 1000: bases cut from the 5' end of every R1 / R2 read (a spacer, a random primer); the read's
  front_clip_R2 : 0         sequence and quality lines then start that many bytes later
  tail_clip_R1 : 0          0 to 1000: bases cut from the 3' end of every R1 / R2 read (the last cycle of a 151-cycle run)
  tail_clip_R2 : 0
  window_size :             1 to 100, with window_quality 1 to 93 (both or neither): cut the read at the start of the first window
  window_quality :          of window_size bases whose mean Phred is below window_quality (Trimmomatic SLIDINGWINDOW, fastp
                            cut_right); a read shorter than the window is left alone
  poly_g : False            True: cut a poly-G tail (two-colour instruments read a dark cluster as high-quality G) of at least
  poly_g_min_length : 10    poly_g_min_length bases, 6 to 100: walking from the 3' end, one base other than G per 8 is forgiven,
                            at most 5; the cut is at the leftmost G reached (fastp's rule; g counts as G, N does not)
min_length (above) holds for these cuts too, except that a front clip is never given back.  The stage is on when a clip is > 0, a
window is set or poly_g is True; Quade_clip_report.csv is then written next to the report.  These options do not turn the 3'
trimming on.  Quade_trim_report.csv's bases_in, pair_overlap, [filter], quality_report and cycle_report see the reads as this
stage left them: with pair_overlap a front clip of F1 + F2 bases shortens the reported insert sizes by that much, and the
reverse complement of R2's clipped 5' bases is cut from R1's 3' end when the insert is short (as fastp's trim_front in front of
its overlap analysis).  The reads are clipped while the device pipeline holds their text, so the options need the device pipeline:
[gpu] device_pipeline, device_inflate and device_deflate True (the defaults) and gzip_level 1 or -1
"""

CLIP_NEEDS = ("[trim] clipping (front_clip, tail_clip, window_size, poly_g) needs the device pipeline (device_pipeline, device_inflate, "
              "device_deflate : True and gzip_level 1 or -1)")
CLIP_FIXED = "Authorized values for front_clip_R1, front_clip_R2, tail_clip_R1 and tail_clip_R2 : 0 to 1000"
CLIP_WINDOW_SIZE = "Authorized values for window_size : 1 to 100"
CLIP_WINDOW_QUALITY = "Authorized values for window_quality : 1 to 93"
CLIP_WINDOW_BOTH = "window_size and window_quality are set together or not at all"
CLIP_POLY_G = "Authorized values for poly_g_min_length : 6 to 100"

PAIR_HELP = """\
Optional [trim] options (not in Quade 0.3.2, whose parser ignores them; absent = as before): paired-end overlap trimming of the
insert reads on the GPU, which needs no adapter sequence.  When the insert is shorter than the reads, R1 and the reverse complement
of R2 overlap over the whole insert and everything behind it is adapter.  Runs behind the 3' trimming above when both are on.
  pair_overlap : False         True: look for the insert length I at which R1 and the reverse complement of R2 agree; an insert
                               shorter than the longer read cuts both reads to it (an insert at least that long cuts nothing, and
                               wins over a shorter one); min_length (above) holds for these cuts too
  pair_min_overlap : 30        8 to 1000: the reads must overlap by at least this many bases at I
  pair_max_mismatches : 5      0 to 64: an overlap of ov bases may hold min(pair_max_mismatches, ov * pair_max_mismatch_pct // 100)
  pair_max_mismatch_pct : 20   0 to 50  mismatches (N and any other byte is a mismatch; lower case matches)
Quade_pair_trim_report.csv is then written next to the report: what was cut and the insert sizes of the library.  The reads are
trimmed while the device pipeline holds their text, so pair_overlap needs the device pipeline: [gpu] device_pipeline,
device_inflate and device_deflate True (the defaults) and gzip_level 1 or -1
"""

PAIR_NEEDS = "pair_overlap needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
PAIR_OVERLAP = "Authorized values for pair_min_overlap : 8 to 1000"
PAIR_MISMATCHES = "Authorized values for pair_max_mismatches : 0 to 64"
PAIR_MISMATCH_PCT = "Authorized values for pair_max_mismatch_pct : 0 to 50"

CORRECT_HELP = """\
Optional [trim] options (not in Quade 0.3.2, whose parser ignores them; absent = as before): overlap base correction of the read
pairs on the GPU, what fastp does under --correction.  pair_overlap (above) accepts an overlap with a few disagreeing positions; at
each of them the instrument read the same base twice, and where one call is confident and the other doubtful the confident base,
with its quality, is written over the doubtful one.  Runs directly behind pair_overlap, on the reads as that stage received them,
for every pair with an insert length I (shorter than the reads or not), and in front of the post-trimming.
  pair_correct : False               True: at a position i of R1 with partner j = I - 1 - i of R2 that is no pair of complementary
                                     letters of ACGT (either case): if R1's byte is a letter with quality >= pair_correct_good_quality
                                     and R2's quality is <= pair_correct_bad_quality, R2 gets the complement (upper case) and R1's
                                     quality; else the same with the reads exchanged; else the position stays unresolved
  pair_correct_good_quality : 30     1 to 93
  pair_correct_bad_quality : 14      0 to pair_correct_good_quality - 1
No length changes and no pair is dropped; the post-trimming, [filter], [screen], quality_report, cycle_report, duplication_report
and the output files see the corrected reads, adapter_report the raw ones, and Quade_pair_trim_report.csv is as without the option.
Quade_pair_correct_report.csv is then written next to the report: reads and bases corrected per read, overlap bases, mismatches,
corrected, unresolved, and the mismatch rate per 100 000 overlap bases before and after.  pair_correct needs pair_overlap : True
and, as that does, the device pipeline
"""

CORRECT_NEEDS = "pair_correct needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
CORRECT_NEEDS_OVERLAP = "pair_correct needs pair_overlap : True"
CORRECT_GOOD = "Authorized values for pair_correct_good_quality : 1 to 93"
CORRECT_BAD = "Authorized values for pair_correct_bad_quality : 0 to pair_correct_good_quality - 1"

POSTTRIM_HELP = """\
Optional [trim] options (not in Quade 0.3.2, whose parser ignores them; absent = as before): trailing-N, poly-X tail and
max_length trimming of the insert reads on the GPU, behind the clipping, the 3' trimming and pair_overlap above and in front of
[filter] (fastp's order: adapters, then trim_poly_x, then max_len1 / max_len2; cutadapt's --trim-n).  A poly-A tail sits between
the insert and the adapter, so it shows only once the adapter is gone.  Index reads, names and the :IDX[:MOL] tag are never
touched, no read is moved and no pair is dropped.  For an insert read r (0 = R1, 1 = R2), take the record the stage receives,
that is, what clip, trim and pairtrim left: sequence bytes s, length L; u(b) = b & 0xDF; P = poly_x_min_length;
M_r = max_length[r].  Each of steps 1 to 3 is skipped when not configured; its output length is then its input length.
  tail_n : False            1 trailing N (tail_n : True): Ln = L - k, where k is the number of consecutive bytes at the 3' end
                            with u(b) == 'N'
  poly_x : False            2 poly-X (poly_x : True, P 6..100, default 10): for each X in A, C, G, T, Lx(X) is the clip stage's
  poly_x_min_length : 10    step 3 exactly as include/quade_hip.h states it for poly-G, with X in place of 'G', over s[0 .. Ln)
                            (walking from the 3' end, one base other than X per 8 is forgiven, at most 5, a run of at least P,
                            cut at the leftmost X reached).  Lp = min over X of Lx(X).  The read's tail base is the X with
                            Lx(X) < Ln; at most one such X exists.  N and every other byte count as a mismatch.  One pass only:
                            a T run behind an A run loses the T run
  max_length_R1 :           3 crop (M_r > 0, 1 to 65535; absent, empty or 0 = off): Lm = min(Lp, M_r)
  max_length_R2 :
                            4 floor: Lout = max(Lm, min(min_length, L)), min_length (above) being the [trim] section's
The record becomes seq_len = Lout; its other fields stay.  The stage is on when tail_n or poly_x is True or a max_length is above
0; poly_x_min_length alone switches nothing on.  Quade_post_trim_report.csv is then written next to the report.  These options
turn neither the clipping nor the 3' trimming on.  [filter], quality_report, cycle_report, duplication_report and the output
files see the reads as this stage left them.  min_length may not be above a max_length that is set.  The reads are trimmed while
the device pipeline holds their text, so the options need the device pipeline: [gpu] device_pipeline, device_inflate and
device_deflate True (the defaults) and gzip_level 1 or -1
"""

POSTTRIM_NEEDS = ("[trim] post-trimming (tail_n, poly_x, max_length) needs the device pipeline (device_pipeline, device_inflate, "
                  "device_deflate : True and gzip_level 1 or -1)")
POSTTRIM_POLY_X = "Authorized values for poly_x_min_length : 6 to 100"
POSTTRIM_MAX_LENGTH = "Authorized values for max_length_R1 and max_length_R2 : 0 to 65535"
POSTTRIM_FLOOR = "min_length may not be above a max_length_R1 or max_length_R2 that is set"

FILTER_HELP = """\
Optional [filter] section (not in Quade 0.3.2, whose parser ignores it; absent = every pair is written): discard pairs on the GPU,
behind the [trim] stages and on what they left.  A pair is dropped, its R1 and its R2 record, for the first of these rules that
either of its reads fails; an absent or empty option turns its rule off.  For a read of L bases:
  min_length :              1 to 100000: too_short, L < min_length (fastp -l, cutadapt -m)
  max_n :                   0 to 100000: too_many_n, more than max_n bases N or n (fastp -n)
  max_unqualified_pct :     0 to 100: low_quality, more than this percentage of the bases below Phred qualified_quality (fastp -u)
  qualified_quality : 15    1 to 93: the Phred value (Phred+33) a base needs to be qualified (fastp -q)
  min_mean_quality :        1 to 93: low_mean_quality, mean Phred below it (fastp -e)
  min_complexity_pct :      1 to 100: low_complexity, less than this percentage of the bases differ from the base behind them
                            (fastp -y with -Y); a poly-G read has 0
The filter applies to every pair, Undetermined included.  Quade_report.csv still counts assignments, the trim reports what
their stages saw, and quality_report the pairs that were written; a destination that loses all its pairs has no files, as one
that received none.  Quade_filter_report.csv is written next to the report: per destination, pairs in, kept and dropped by
reason, bases in and kept.  The pairs are filtered while the device pipeline holds their text, so the section needs the device
pipeline: [gpu] device_pipeline, device_inflate and device_deflate True (the defaults) and gzip_level 1 or -1
"""

FILTER_NEEDS = "[filter] needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
FILTER_RANGES = {"min_length": (1, 100000), "max_n": (0, 100000), "max_unqualified_pct": (0, 100), "qualified_quality": (1, 93),
                 "min_mean_quality": (1, 93), "min_complexity_pct": (1, 100)}
FILTER_RULES = ("min_length", "max_n", "max_unqualified_pct", "min_mean_quality", "min_complexity_pct")  # in the rule's order


SCREEN_HELP = """\
Optional [screen] section (not in Quade 0.3.2, whose parser ignores it; absent = as before): a k-mer screen of the insert reads
against a reference on the GPU -- PhiX, a spike-in, an rRNA set, a vector, a contaminant -- what bbduk does with ref=phix.fa k=31
in a pass of its own over every output file.  The user supplies the FASTA; no genome is shipped.
  reference :               a FASTA path, plain or .gz; an empty value turns the stage off
  kmer : 31                 15 to 32
  min_hits : 1              1 to 65535
  action : report           report or drop
u(b) = b & 0xDF.  A base is valid when u(b) is one of A, C, G, T.  Its code is c(b) = (u(b) >> 1) & 3, which gives A 0, C 1, T 2,
G 3 (the duplication key's code); the complement is c ^ 2.  The k-mer at position p of a sequence s exists when s[p .. p + k) are
all valid.  Its forward word is w = sum c(s[p + i]) << 2 (k - 1 - i), its reverse-complement word
rc = sum (c(s[p + k - 1 - i]) ^ 2) << 2 (k - 1 - i), its canonical word min(w, rc).  The reference set R holds the distinct
canonical words of every k-mer of every record of the reference FASTA.  Records are linear; a line starting with '>' separates
records, so k-mers never span two records; lower case counts; any other letter breaks k-mers.  hits(read) is the number of
positions p in [0, L - k] whose k-mer exists and whose canonical word is in R.  A read shorter than k has 0 hits and 0 k-mers.  A
pair is matched when hits(R1) + hits(R2) >= min_hits.
The stage sees the pairs the output stages see: behind clip, [trim], pair_overlap, post-trim and [filter], only pairs the filter
kept, the reads as those stages left them, every destination whatever its write flag.  With action : report nothing else
changes.  With action : drop a matched pair leaves the run the way a filtered pair does: it is in no file, and quality_report,
cycle_report and duplication_report do not count it; Quade_report.csv and Quade_filter_report.csv are exactly as without the
stage.  Quade_screen_report.csv is written next to the report: per destination pairs, matched pairs, reads with a hit, k-mers,
hit k-mers, bases in and bases of the matched pairs.  A reference of up to 6144 distinct k-mers (PhiX has about 5400) is looked up
in the compute unit's LDS, a larger one, up to 4194304, in global memory.  The reads are screened while the device pipeline
holds their text, so the section needs the device pipeline: [gpu] device_pipeline, device_inflate and device_deflate True (the
defaults) and gzip_level 1 or -1
"""

SCREEN_NEEDS = "[screen] needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
SCREEN_REFERENCE = "[screen] reference is missing or cannot be read as a FASTA file, plain or gzip"
SCREEN_NO_KMER = "[screen] reference holds no k-mer: no record has kmer valid bases in a row"
SCREEN_TOO_MANY = "[screen] reference holds more than 4194304 distinct k-mers"
SCREEN_KMER = "Authorized values for [screen] kmer : 15 to 32"
SCREEN_MIN_HITS = "Authorized values for [screen] min_hits : 1 to 65535"
SCREEN_ACTION = "Authorized values for [screen] action : report or drop"


def filter_range_message(name):
    return "Authorized values for [filter] %s : %d to %d" % ((name,) + FILTER_RANGES[name])


def template_bytes():
    """The example configuration file, byte for byte the reference's template: the package ships the
    reference-held golden copy (test/result/Quade_conf_file.txt = the text src/Conf_file.py:18-104
    writes) as data and reads it at run time."""
    with open(TEMPLATE_PATH, "rb") as fp:
        return fp.read()


def write_example_conf(path=CONF_NAME):
    """`-i`: write an example configuration file in the current folder (src/Conf_file.py:15-18)."""
    with open(path, "wb") as fp:
        fp.write(template_bytes())


class QuadeConf(object):
    """Parsed configuration.  Field names follow the attributes of the reference's Quade object
    (src/Quade.py:96-122): positions are dicts {"start": 0-based, "end": 1-based inclusive}."""

    def __init__(self, conf_file):
        # Verify if conf file was given and is valid (src/Quade.py:87-88)
        assert conf_file, "A path to the configuration file is mandatory"
        is_readable_file(conf_file)
        self.conf = conf_file
        cp = configparser.RawConfigParser(allow_no_value=True)
        cp.read(self.conf)

        self.minimal_qual = cp.getint("quality", "minimal_qual")

        self.idx1 = True
        self.idx2 = cp.getboolean("index", "index2")
        self.mol1 = self.idx1 and cp.getboolean("index", "molecular1")
        self.mol2 = self.idx2 and cp.getboolean("index", "molecular2")

        def pos(enabled, name):
            if not enabled:
                return {"start": 0, "end": 0}
            return {"start": cp.getint("index", name + "_start") - 1, "end": cp.getint("index", name + "_end")}

        self.idx1_pos = pos(True, "index1")
        self.idx2_pos = pos(self.idx2, "index2")
        self.mol1_pos = pos(self.mol1, "molecular1")
        self.mol2_pos = pos(self.mol2, "molecular2")
        # optional mismatch budgets (extension, MISMATCH_HELP): 0 = exact matching
        def budget(name, enabled):
            if not enabled or not cp.has_option("index", name) or cp.get("index", name) in (None, ""):
                return 0
            return cp.getint("index", name)

        self.idx1_mismatches = budget("index1_mismatches", True)
        self.idx2_mismatches = budget("index2_mismatches", self.idx2)

        self.seq_R1 = cp.get("fastq", "seq_R1").split()
        self.seq_R2 = cp.get("fastq", "seq_R2").split()
        self.index_R1 = cp.get("fastq", "index_R1").split()
        self.index_R2 = [] if not self.idx2 else cp.get("fastq", "index_R2").split()

        self.write_undetermined = cp.getboolean("output", "write_undetermined")
        self.write_pass = cp.getboolean("output", "write_pass")
        self.write_fail = cp.getboolean("output", "write_fail")
        # optional report of the most frequent unknown barcodes (extension, UNKNOWN_HELP): 0 = none
        self.top_unknown_barcodes = 0
        if cp.has_option("output", "top_unknown_barcodes") and cp.get("output", "top_unknown_barcodes") not in (None, ""):
            self.top_unknown_barcodes = cp.getint("output", "top_unknown_barcodes")
        # optional index-hopping report (extension, HOPPING_HELP)
        self.index_hopping_report = False
        if cp.has_option("output", "index_hopping_report") and cp.get("output", "index_hopping_report") not in (None, ""):
            self.index_hopping_report = cp.get("output", "index_hopping_report").strip().lower() in ("true", "1", "yes", "on")
        # optional yield and quality report per destination (extension, QUALITY_HELP)
        self.quality_report = False
        if cp.has_option("output", "quality_report") and cp.get("output", "quality_report") not in (None, ""):
            self.quality_report = cp.get("output", "quality_report").strip().lower() in ("true", "1", "yes", "on")

        # optional duplication report (extension, DUPLICATION_HELP)
        def out(name, default):
            if cp.has_option("output", name) and cp.get("output", name) not in (None, ""):
                return cp.getint("output", name)
            return default

        self.duplication_report = False
        if cp.has_option("output", "duplication_report") and cp.get("output", "duplication_report") not in (None, ""):
            self.duplication_report = cp.get("output", "duplication_report").strip().lower() in ("true", "1", "yes", "on")
        self.duplication_bases = out("duplication_bases", 32)
        self.duplication_sample = out("duplication_sample", 16)

        # optional [trim] section (extension, TRIM_HELP): 3' quality and adapter trimming of the insert reads
        def trim(name, default, conv=int):
            if cp.has_section("trim") and cp.has_option("trim", name) and cp.get("trim", name) not in (None, ""):
                return conv(cp.get("trim", name))
            return default

        self.adapter_R1 = trim("adapter_R1", "", str).strip().upper()
        self.adapter_R2 = trim("adapter_R2", "", str).strip().upper()
        self.quality_cutoff = trim("quality_cutoff", 0)
        self.min_overlap = trim("min_overlap", 3)
        self.max_mismatch_pct = trim("max_mismatch_pct", 10)
        self.min_length = trim("min_length", 0)
        # ... its end clipping, window and poly-G trimming in front of that (CLIP_HELP): None = no window
        self.front_clip = (trim("front_clip_R1", 0), trim("front_clip_R2", 0))
        self.tail_clip = (trim("tail_clip_R1", 0), trim("tail_clip_R2", 0))
        self.window_size = trim("window_size", None)
        self.window_quality = trim("window_quality", None)
        self.poly_g = trim("poly_g", False, lambda v: v.strip().lower() in ("true", "1", "yes", "on"))
        self.poly_g_min_length = trim("poly_g_min_length", 10)
        # ... and its paired-end overlap trimming (PAIR_HELP)
        self.pair_overlap = trim("pair_overlap", False, lambda v: v.strip().lower() in ("true", "1", "yes", "on"))
        self.pair_min_overlap = trim("pair_min_overlap", 30)
        self.pair_max_mismatches = trim("pair_max_mismatches", 5)
        self.pair_max_mismatch_pct = trim("pair_max_mismatch_pct", 20)
        # ... and the overlap base correction behind it (CORRECT_HELP)
        self.pair_correct = trim("pair_correct", False, lambda v: v.strip().lower() in ("true", "1", "yes", "on"))
        self.pair_correct_good_quality = trim("pair_correct_good_quality", 30)
        self.pair_correct_bad_quality = trim("pair_correct_bad_quality", 14)
        # ... and what is trimmed behind all of that (POSTTRIM_HELP): a max_length of 0 = no crop
        self.tail_n = trim("tail_n", False, lambda v: v.strip().lower() in ("true", "1", "yes", "on"))
        self.poly_x = trim("poly_x", False, lambda v: v.strip().lower() in ("true", "1", "yes", "on"))
        self.poly_x_min_length = trim("poly_x_min_length", 10)
        self.max_length = (trim("max_length_R1", 0), trim("max_length_R2", 0))

        # optional per-cycle quality and base-content report (extension, CYCLE_HELP)
        self.cycle_report = False
        if cp.has_option("output", "cycle_report") and cp.get("output", "cycle_report") not in (None, ""):
            self.cycle_report = cp.get("output", "cycle_report").strip().lower() in ("true", "1", "yes", "on")
        # optional adapter content report of the raw insert reads (extension, ADAPTER_HELP); the extra probes count only with it
        self.adapter_report = False
        if cp.has_option("output", "adapter_report") and cp.get("output", "adapter_report") not in (None, ""):
            self.adapter_report = cp.get("output", "adapter_report").strip().lower() in ("true", "1", "yes", "on")
        self.adapter_report_extra = ""
        if cp.has_option("output", "adapter_report_extra") and cp.get("output", "adapter_report_extra") not in (None, ""):
            self.adapter_report_extra = cp.get("output", "adapter_report_extra").strip()
        self._adapters = None  # adapter_params' dict, made by _test_values when the report is on
        # optional [filter] section (extension, FILTER_HELP): None = the rule is off
        def flt(name, default=None):
            if cp.has_section("filter") and cp.has_option("filter", name) and cp.get("filter", name) not in (None, ""):
                return int(cp.get("filter", name))
            return default

        self.filter_min_length = flt("min_length")
        self.filter_max_n = flt("max_n")
        self.filter_max_unqualified_pct = flt("max_unqualified_pct")
        self.filter_qualified_quality = flt("qualified_quality", 15)
        self.filter_min_mean_quality = flt("min_mean_quality")
        self.filter_min_complexity_pct = flt("min_complexity_pct")

        # optional [screen] section (extension, SCREEN_HELP): an empty reference = off
        def scr(name, default, conv=int):
            if cp.has_section("screen") and cp.has_option("screen", name) and cp.get("screen", name) not in (None, ""):
                return conv(cp.get("screen", name))
            return default

        self.screen_reference = scr("reference", "", str).strip()
        self.screen_kmer = scr("kmer", 31)
        self.screen_min_hits = scr("min_hits", 1)
        self.screen_action = scr("action", "report", str).strip().lower()
        self._screen_ref = None  # screen.Reference, read by _test_values when the stage is on

        # (name, fused barcode) per [sample*] section, in file order (src/Quade.py:133-139)
        self.samples = []
        for section in [i for i in cp.sections() if i.startswith("sample")]:
            if self.idx2:
                self.samples.append((cp.get(section, "name"),
                                     cp.get(section, "index1_seq") + cp.get(section, "index2_seq")))
            else:
                self.samples.append((cp.get(section, "name"), cp.get(section, "index1_seq")))

        # optional [gpu] section (extension; defaults keep reference conf files working)
        def opt(name, default, conv=int):
            if cp.has_section("gpu") and cp.has_option("gpu", name) and cp.get("gpu", name) not in (None, ""):
                return conv(cp.get("gpu", name))
            return default

        self.devices = opt("devices", "0", str).split()
        self.batch_pairs = opt("batch_pairs", 500000)
        self.slots = opt("slots", 3)
        self.gzip_level = opt("gzip_level", 1)
        self.chunk_workers = opt("chunk_workers", 1)
        self.io_threads = opt("io_threads", 0)
        self.unknown_slots = opt("unknown_slots", 1 << 24)
        self.duplicate_slots = opt("duplicate_slots", 1 << 24)
        self.device_inflate = opt("device_inflate", "True", str).strip().lower() in ("true", "1", "yes", "on")
        self.device_deflate = opt("device_deflate", "True", str).strip().lower() in ("true", "1", "yes", "on")
        # the whole chunk loop on the device (qd_pipe_*): text stays in HBM from the inflater to the coder.  Needs the device's
        # inflate and deflate stages and a gzip level the device codes (1, -1); batch_pairs then defaults to 2 000 000
        self.device_pipeline = opt("device_pipeline", "True", str).strip().lower() in ("true", "1", "yes", "on")
        self.batch_pairs_given = cp.has_section("gpu") and cp.has_option("gpu", "batch_pairs")
        # one chunk across several ranks: auto (fewer chunks than ranks), True, False
        self.shard_chunks = opt("shard_chunks", "auto", str).strip().lower()
        if self.shard_chunks in ("1", "yes", "on"):
            self.shard_chunks = "true"
        if self.shard_chunks in ("0", "no", "off"):
            self.shard_chunks = "false"

        self._test_values()

    def _test_values(self):
        """src/Quade.py:258-279"""
        assert 0 <= self.minimal_qual <= 40, "Authorized values for minimal_qual : 0 to 40"
        if self.idx2:
            assert len(self.seq_R1) == len(self.seq_R2) == len(self.index_R1) == len(self.index_R2) > 0, \
                "seq_R1, seq_R2, index_R1 and index_R2 are mandatory and have to contain the same number of files"
            for fp in (self.seq_R1 + self.seq_R2 + self.index_R1 + self.index_R2):
                is_readable_file(fp)
        else:
            assert len(self.seq_R1) == len(self.seq_R2) == len(self.index_R1) > 0, \
                "seq_R1, seq_R2 and index_R1 are mandatory and have to contain the same number of files"
            for fp in (self.seq_R1 + self.seq_R2 + self.index_R1):
                is_readable_file(fp)
        assert 0 <= self.idx1_mismatches <= 2, "Authorized values for index1_mismatches : 0 to 2"
        assert 0 <= self.idx2_mismatches <= 2, "Authorized values for index2_mismatches : 0 to 2"
        assert 0 <= self.top_unknown_barcodes <= 1000, "Authorized values for top_unknown_barcodes : 0 to 1000"
        assert 1 << 10 <= self.unknown_slots <= 1 << 28 and self.unknown_slots & (self.unknown_slots - 1) == 0, \
            "[gpu] unknown_slots : a power of two, 1024 to 268435456"
        assert not self.index_hopping_report or self.idx2, HOPPING_NEEDS
        assert not self.quality_report or self.can_pipe, QUALITY_NEEDS
        assert not self.cycle_report or self.can_pipe, CYCLE_NEEDS
        if self.adapter_report:  # the probes are settled here, before any read is processed
            assert self.can_pipe, ADAPTER_NEEDS
            self._adapters = self._adapter_probes()
        assert 8 <= self.duplication_bases <= 32, DUPLICATION_BASES
        assert 1 <= self.duplication_sample <= 1024 and self.duplication_sample & (self.duplication_sample - 1) == 0, DUPLICATION_SAMPLE
        assert 1 << 10 <= self.duplicate_slots <= 1 << 28 and self.duplicate_slots & (self.duplicate_slots - 1) == 0, DUPLICATION_SLOTS
        assert not self.duplication_report or self.can_pipe, DUPLICATION_NEEDS
        for a in (self.adapter_R1, self.adapter_R2):
            assert len(a) <= 64 and not a.strip("ACGT"), TRIM_ADAPTER
        assert 0 <= self.quality_cutoff <= 93, TRIM_CUTOFF
        assert 1 <= self.min_overlap <= 64 and all(self.min_overlap <= len(a) for a in (self.adapter_R1, self.adapter_R2) if a), \
            TRIM_OVERLAP
        assert 0 <= self.max_mismatch_pct <= 50, TRIM_MISMATCH
        assert 0 <= self.min_length <= 65535, TRIM_LENGTH
        assert not self.trim or self.can_pipe, TRIM_NEEDS
        assert all(0 <= v <= 1000 for v in self.front_clip + self.tail_clip), CLIP_FIXED
        assert (self.window_size is None) == (self.window_quality is None), CLIP_WINDOW_BOTH
        assert self.window_size is None or 1 <= self.window_size <= 100, CLIP_WINDOW_SIZE
        assert self.window_quality is None or 1 <= self.window_quality <= 93, CLIP_WINDOW_QUALITY
        assert 6 <= self.poly_g_min_length <= 100, CLIP_POLY_G
        assert not self.clip or self.can_pipe, CLIP_NEEDS
        assert 8 <= self.pair_min_overlap <= 1000, PAIR_OVERLAP
        assert 0 <= self.pair_max_mismatches <= 64, PAIR_MISMATCHES
        assert 0 <= self.pair_max_mismatch_pct <= 50, PAIR_MISMATCH_PCT
        assert not self.pair_trim or self.can_pipe, PAIR_NEEDS
        assert 1 <= self.pair_correct_good_quality <= 93, CORRECT_GOOD
        assert 0 <= self.pair_correct_bad_quality < self.pair_correct_good_quality, CORRECT_BAD
        assert not self.pair_correction or self.can_pipe, CORRECT_NEEDS
        assert not self.pair_correction or self.pair_trim, CORRECT_NEEDS_OVERLAP
        assert 6 <= self.poly_x_min_length <= 100, POSTTRIM_POLY_X
        assert all(0 <= m <= 65535 for m in self.max_length), POSTTRIM_MAX_LENGTH
        assert all(self.min_length <= m for m in self.max_length if m), POSTTRIM_FLOOR
        assert not self.posttrim or self.can_pipe, POSTTRIM_NEEDS
        for name, value in self.filter_params().items():
            assert value is None or FILTER_RANGES[name][0] <= value <= FILTER_RANGES[name][1], filter_range_message(name)
        assert not self.filter or self.can_pipe, FILTER_NEEDS
        if self.screen:  # the reference is read here, before any read is processed
            from . import screen
            assert screen.MIN_KMER <= self.screen_kmer <= screen.MAX_KMER, SCREEN_KMER
            assert 1 <= self.screen_min_hits <= 65535, SCREEN_MIN_HITS
            assert self.screen_action in ("report", "drop"), SCREEN_ACTION
            assert self.can_pipe, SCREEN_NEEDS
            try:
                data = screen.read_fasta(self.screen_reference)
            except (OSError, EOFError, zlib.error):
                raise AssertionError(SCREEN_REFERENCE)
            self._screen_ref = screen.reference_kmers(data, self.screen_kmer)
            assert self._screen_ref.kmers.size > 0, SCREEN_NO_KMER
            assert self._screen_ref.kmers.size <= screen.MAX_KMERS, SCREEN_TOO_MANY
        for pos in [self.idx1_pos, self.idx2_pos, self.mol1_pos, self.mol2_pos]:
            assert pos["start"] >= 0
            assert pos["end"] >= pos["start"]
        assert self.batch_pairs >= 1 and 1 <= self.slots <= 64 and -1 <= self.gzip_level <= 9 and \
            1 <= self.chunk_workers <= 64 and 0 <= self.io_threads <= 1024, \
            "[gpu] batch_pairs >= 1, 1 <= slots <= 64, -1 <= gzip_level <= 9, 1 <= chunk_workers <= 64, 0 <= io_threads <= 1024"

    @property
    def can_pipe(self):
        """the device pipeline can run: every device stage is on and the gzip level is one the device codes; what the read
        stages need (the *_NEEDS messages) and what Quade takes the pipeline for"""
        return bool(self.device_pipeline and self.device_inflate and self.device_deflate and self.gzip_level in (1, -1))

    def _adapter_probes(self):
        """The probes of the adapter content report (ADAPTER_HELP): the built-in list, adapter_R1 and adapter_R2 when set, then
        adapter_report_extra -> dict(probes=[(name, probe)] in slot order, aliases=[(name, the name of the earlier equal probe)],
        left_off=[(name, reason)])"""
        import re
        from .stages import ADAPTER_BUILTIN, ADAPTER_K, ADAPTER_PROBES
        given = list(ADAPTER_BUILTIN) + [(name, seq) for name, seq in (("adapter_R1", self.adapter_R1), ("adapter_R2", self.adapter_R2)) if seq]
        for item in (self.adapter_report_extra.split(";") if self.adapter_report_extra else []):
            m = re.match(r"^\s*([A-Za-z0-9_]+)\s*=\s*([A-Za-z]+)\s*$", item)
            assert m, ADAPTER_EXTRA
            given.append((m.group(1), m.group(2)))
        assert len(set(name for name, _ in given)) == len(given), ADAPTER_EXTRA
        probes, aliases, left_off = [], [], []
        for name, seq in given:
            probe = seq[:ADAPTER_K].upper()
            if len(probe) < ADAPTER_K:
                left_off.append((name, ADAPTER_SHORT))
            elif probe.strip("ACGT"):
                left_off.append((name, ADAPTER_NOT_ACGT))
            elif probe in [p for _, p in probes]:
                aliases.append((name, [n for n, p in probes if p == probe][0]))
            else:
                probes.append((name, probe))
        assert len(probes) <= ADAPTER_PROBES, ADAPTER_TOO_MANY
        return dict(probes=probes, aliases=aliases, left_off=left_off)

    def adapter_params(self):
        """what Engine.adapters_set takes, and the report: the probes in force, the aliases and the sequences left off"""
        return self._adapters

    def duplication_params(self):
        """what Engine.dup_set takes"""
        return dict(bases=self.duplication_bases, sample=self.duplication_sample, slots=self.duplicate_slots)

    @property
    def trim(self):
        """3' trimming of the insert reads is on (TRIM_HELP)"""
        return bool(self.adapter_R1 or self.adapter_R2 or self.quality_cutoff > 0)

    def trim_params(self):
        """what Engine.trim_set takes"""
        return dict(adapter_r1=self.adapter_R1, adapter_r2=self.adapter_R2, quality_cutoff=self.quality_cutoff,
                    min_overlap=self.min_overlap, max_mismatch_pct=self.max_mismatch_pct, min_length=self.min_length)

    @property
    def clip(self):
        """end clipping, window or poly-G trimming of the insert reads is on (CLIP_HELP)"""
        return bool(any(self.front_clip) or any(self.tail_clip) or self.window_size is not None or self.poly_g)

    def clip_params(self):
        """what Engine.clip_set takes"""
        return dict(front_clip_r1=self.front_clip[0], front_clip_r2=self.front_clip[1], tail_clip_r1=self.tail_clip[0],
                    tail_clip_r2=self.tail_clip[1], window_size=self.window_size or 0, window_quality=self.window_quality or 0,
                    poly_g_min_length=self.poly_g_min_length if self.poly_g else 0, min_length=self.min_length)

    @property
    def pair_trim(self):
        """paired-end overlap trimming of the insert reads is on (PAIR_HELP)"""
        return bool(self.pair_overlap)

    def pair_trim_params(self):
        """what Engine.pairtrim_set takes"""
        return dict(min_overlap=self.pair_min_overlap, max_mismatches=self.pair_max_mismatches,
                    max_mismatch_pct=self.pair_max_mismatch_pct, min_length=self.min_length)

    @property
    def pair_correction(self):
        """overlap base correction of the read pairs is on (CORRECT_HELP)"""
        return bool(self.pair_correct)

    def pair_correct_params(self):
        """what Engine.paircorrect_set takes"""
        return dict(good_quality=self.pair_correct_good_quality, bad_quality=self.pair_correct_bad_quality)

    @property
    def posttrim(self):
        """trailing-N, poly-X or max_length trimming of the insert reads is on (POSTTRIM_HELP)"""
        return bool(self.tail_n or self.poly_x or any(self.max_length))

    def posttrim_params(self):
        """what Engine.posttrim_set takes"""
        return dict(tail_n=int(self.tail_n), poly_x_min_length=self.poly_x_min_length if self.poly_x else 0,
                    max_length_r1=self.max_length[0], max_length_r2=self.max_length[1], min_length=self.min_length)

    @property
    def filter(self):
        """read filtering is on: any rule of the [filter] section is set (FILTER_HELP)"""
        p = self.filter_params()
        return any(p[name] is not None for name in FILTER_RULES)

    def filter_params(self):
        """what Engine.filter_set takes: None = the rule is off"""
        return dict(min_length=self.filter_min_length, max_n=self.filter_max_n, max_unqualified_pct=self.filter_max_unqualified_pct,
                    qualified_quality=self.filter_qualified_quality, min_mean_quality=self.filter_min_mean_quality,
                    min_complexity_pct=self.filter_min_complexity_pct)

    @property
    def screen(self):
        """the k-mer screen is on: the [screen] section names a reference (SCREEN_HELP)"""
        return bool(self.screen_reference)

    def screen_params(self):
        """what Engine.screen_set takes: the parameters, the reference set's words and, for the report, what the FASTA held"""
        ref = self._screen_ref
        return dict(kmer=self.screen_kmer, min_hits=self.screen_min_hits, action=self.screen_action, kmers=ref.kmers,
                    reference=dict(name=os.path.basename(self.screen_reference), records=ref.records, bases=ref.bases,
                                   kmers=int(ref.kmers.size)))

    def plan(self):
        """The qd_plan the HIP library takes (include/quade_hip.h)."""
        from .hip_backend import make_plan
        p = lambda d: (d["start"], d["end"])  # noqa: E731
        return make_plan(self.idx2, self.minimal_qual, p(self.idx1_pos), p(self.idx2_pos),
                         p(self.mol1_pos), p(self.mol2_pos))


def is_readable_file(fp):
    """src/Quade.py:281-284"""
    if not os.access(fp, os.R_OK):
        raise IOError("{} is not a valid file".format(fp))
