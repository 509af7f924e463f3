# -*- coding: utf-8 -*-
"""
The read stages of the device pipeline, described once: the columns of their counter tables (include/quade_hip.h, qd_qstats_*,
qd_cstats_*, qd_clip_*, qd_trim_*, qd_pairtrim_*, qd_paircorrect_*, qd_posttrim_*, qd_filter_*, qd_screen_*, qd_adapters_*), the bytes a table has when the ranks
exchange it, and READ_STAGES, the table Quade.__call__ walks to switch the stages on, to collect their tables and to write their reports.  hip_backend and the
report modules take the columns from here; nothing here touches libquade_hip.so.
"""
from __future__ import annotations

import importlib
import os
from collections import namedtuple

import numpy as np

QSTATS_COUNTERS = ("records", "bases", "qual_sum", "q20_bases", "q30_bases", "n_bases")  # per destination and read (qd_qstats_*)

CLIP_COUNTERS = ("reads", "bases_in", "bases_out", "front_clipped_reads", "front_clipped_bases", "tail_clipped_reads", "tail_clipped_bases",
                 "window_reads", "window_bases", "polyg_reads", "polyg_bases", "floored_reads")  # per read R1 / R2 (qd_clip_*)

TRIM_COUNTERS = ("reads", "bases_in", "bases_out", "quality_trimmed_reads", "quality_trimmed_bases", "adapter_reads", "adapter_bases",
                 "floored_reads")  # per read R1 / R2 (qd_trim_*)

POSTTRIM_COUNTERS = ("reads", "bases_in", "bases_out", "n_tail_reads", "n_tail_bases", "polya_reads", "polya_bases", "polyc_reads",
                     "polyc_bases", "polyg_reads", "polyg_bases", "polyt_reads", "polyt_bases", "cropped_reads", "cropped_bases",
                     "floored_reads")  # per read R1 / R2 (qd_posttrim_*)

PAIRTRIM_COUNTERS = ("reads", "bases_in", "bases_out", "overlap_trimmed_reads", "overlap_trimmed_bases", "floored_reads")  # per read
PAIRTRIM_PAIR_COUNTERS = ("pairs", "overlapped_pairs", "short_insert_pairs")
PAIRTRIM_BINS = 1025  # insert sizes: bin I for I < 1024, the last bin for I >= 1024
PAIRTRIM_VALUES = 2 * len(PAIRTRIM_COUNTERS) + len(PAIRTRIM_PAIR_COUNTERS) + PAIRTRIM_BINS  # qd_pairtrim_*'s table: 1040


def split_pairtrim(table):
    """a table -> (per read [2][6], the three pair counters, the 1025 insert size bins), Python integers"""
    t = [int(x) for x in np.asarray(table).reshape(PAIRTRIM_VALUES)]
    k = len(PAIRTRIM_COUNTERS)
    return [t[:k], t[k:2 * k]], t[2 * k:2 * k + 3], t[2 * k + 3:]


# qd_paircorrect_*'s table: the overlap base correction behind the overlap trimming
PAIRCORRECT_COUNTERS = ("r1_corrected_reads", "r1_corrected_bases", "r2_corrected_reads", "r2_corrected_bases", "pairs", "overlapped_pairs",
                        "overlap_bases", "mismatches", "unresolved", "corrected_pairs")
PAIRCORRECT_VALUES = len(PAIRCORRECT_COUNTERS)  # 10


# qd_filter_*: the reasons (the reason byte of a dropped pair is the index + 1), the table's columns and the parameters
FILTER_REASONS = ("too_short", "too_many_n", "low_quality", "low_mean_quality", "low_complexity")
FILTER_COUNTERS = ("pairs",) + FILTER_REASONS + ("bases_in", "bases_dropped")  # per destination
FILTER_KEYS = ("min_length", "max_n", "max_unqualified_pct", "qualified_quality", "min_mean_quality", "min_complexity_pct")

# qd_screen_*: the table's columns per destination, and the actions in the order of their numbers
SCREEN_COUNTERS = ("pairs", "matched_pairs", "r1_hit_reads", "r2_hit_reads", "kmers", "hit_kmers", "bases_in", "bases_matched")
SCREEN_ACTIONS = ("report", "drop")

# the per-cycle table (qd_cstats_*): uint64, group-major (pass, fail, Undetermined), then read; per (group, read) the sections
CSTATS_GROUPS = ("pass", "fail", "Undetermined")
CSTATS_COUNTERS = ("A", "C", "G", "T", "N", "qual_sum", "q20", "q30")  # per cycle
CSTATS_CYCLES, CSTATS_LEN_BINS, CSTATS_MEANQ_BINS, CSTATS_GC_BINS = 1024, 1025, 94, 101
CSTATS_SECTIONS = (("cycle", (CSTATS_CYCLES, len(CSTATS_COUNTERS))), ("len", (CSTATS_LEN_BINS,)), ("meanq", (CSTATS_MEANQ_BINS,)),
                   ("gc", (CSTATS_GC_BINS,)))
CSTATS_GR_VALUES = CSTATS_CYCLES * len(CSTATS_COUNTERS) + CSTATS_LEN_BINS + CSTATS_MEANQ_BINS + CSTATS_GC_BINS  # 9412
CSTATS_VALUES = len(CSTATS_GROUPS) * 2 * CSTATS_GR_VALUES  # 56472


def cstats_views(flat):
    """The flat table (uint64[CSTATS_VALUES]) as a dict of views into it: cycle[3, 2, 1024, 8], len[3, 2, 1025],
    meanq[3, 2, 94], gc[3, 2, 101] -- [group][R1, R2][...]"""
    flat = np.asarray(flat)
    assert flat.shape == (CSTATS_VALUES,) and flat.dtype == np.uint64, "cycle table of the wrong size"
    per = flat.reshape(len(CSTATS_GROUPS), 2, CSTATS_GR_VALUES)
    out, at = {}, 0
    for name, shape in CSTATS_SECTIONS:
        size = int(np.prod(shape))
        out[name] = per[:, :, at:at + size].reshape((len(CSTATS_GROUPS), 2) + shape)
        at += size
    return out


def cstats_flat(table):
    """cstats_views' dict (or a flat table) -> the flat uint64[CSTATS_VALUES] layout of qd_cstats_read"""
    if not isinstance(table, dict):
        flat = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1)
        assert flat.size == CSTATS_VALUES, "cycle table of the wrong size"
        return flat
    per = np.concatenate([np.asarray(table[name], dtype=np.uint64).reshape(len(CSTATS_GROUPS), 2, -1) for name, _ in CSTATS_SECTIONS],
                         axis=2)
    assert per.shape == (len(CSTATS_GROUPS), 2, CSTATS_GR_VALUES), "cycle table of the wrong size"
    return np.ascontiguousarray(per).reshape(-1)


class Stage(namedtuple("Stage", "name engine conf params shape count what flat view report report_args")):
    """One read stage.
    name         its name in the rendezvous directory (the ranks' exchange) and in STAGE
    engine       the prefix of its Engine methods: <engine>_read, and <engine>_set(**params) or <engine>_enable(True)
    conf         the QuadeConf attribute that says the stage is on
    params       the QuadeConf method that gives its keyword parameters, or None: the stage has none
    shape        its table, uint64; a leading -1 = one row per destination (2 * samples + 1); (-1,) = a flat table whose size depends
                 on the samples (count "values")
    count        the uint64 in front of the packed table: "rows" (the destinations), "values" (all of them) or None
    what         the table's name in the message of a blob of the wrong size
    flat, view   None, or table -> flat array and flat array -> table for a stage whose table is not one array (cycle: a dict)
    report       the module that writes its report: REPORT_NAME and write_report(path, table, *report_args)
    report_args  what write_report takes behind the table: "samples" (the names in sheet order), "params"
    """
    __slots__ = ()

    def on(self, cf):
        return bool(getattr(cf, self.conf))

    def conf_params(self, cf):
        return getattr(cf, self.params)() if self.params else None

    def enable(self, eng, cf):
        """switches the stage on in a context, as the conf says"""
        if self.params:
            getattr(eng, self.engine + "_set")(**self.conf_params(cf))
        else:
            getattr(eng, self.engine + "_enable")(True)

    def read(self, eng):
        """a context's table, as one array that can be summed"""
        table = getattr(eng, self.engine + "_read")()
        return self.flat(table) if self.flat else table

    def report_module(self):
        return importlib.import_module("." + self.report, __package__)

    def write_report(self, outdir, table, samples=(), params=None):
        """the stage's report file in outdir -> its path"""
        mod = self.report_module()
        path = os.path.join(outdir, mod.REPORT_NAME)
        mod.write_report(path, table, *[{"samples": list(samples), "params": params}[a] for a in self.report_args])
        return path


# In pipeline order.  (The tally of the unknown barcodes is not a stage of this table: its tables merge by key, not by adding, and
# its report takes the run's counters and the sample sheet -- Quade._collect_unknown.)
STAGES = (
    Stage("quality", "qstats", "quality_report", None, (-1, 2, len(QSTATS_COUNTERS)), "rows", "quality table",
          None, None, "quality_report", ("samples",)),
    Stage("cycle", "cstats", "cycle_report", None, (CSTATS_VALUES,), "values", "cycle table",
          cstats_flat, cstats_views, "cycle_report", ()),
    Stage("clip", "clip", "clip", "clip_params", (2, len(CLIP_COUNTERS)), None, "clip counters",
          None, None, "clip_report", ("params",)),
    Stage("trim", "trim", "trim", "trim_params", (2, len(TRIM_COUNTERS)), None, "trim counters",
          None, None, "trim_report", ("params",)),
    Stage("pairtrim", "pairtrim", "pair_trim", "pair_trim_params", (PAIRTRIM_VALUES,), None, "an overlap trimming table",
          None, None, "pair_trim_report", ("params",)),
    Stage("filter", "filter", "filter", "filter_params", (-1, len(FILTER_COUNTERS)), "rows", "filter table",
          None, None, "filter_report", ("samples", "params")),
)
STAGE = {s.name: s for s in STAGES}

# STAGES and STAGE stay the six stages above: tests pin them, names and sizes.  The post-trimming stage (qd_posttrim_*) stands
# in RUN_STAGES, the seven stages up to the filter in pipeline order.
POSTTRIM = Stage("posttrim", "posttrim", "posttrim", "posttrim_params", (2, len(POSTTRIM_COUNTERS)), None, "post-trim counters",
                 None, None, "posttrim_report", ("params",))
RUN_STAGES = STAGES[:5] + (POSTTRIM,) + STAGES[5:]  # quality, cycle, clip, trim, pairtrim, posttrim, filter
RUN_STAGE = {s.name: s for s in RUN_STAGES}


# RUN_STAGES is pinned at those seven in turn.  The k-mer screen (qd_screen_*) runs behind the filter: PIPE_STAGES is every stage
# in pipeline order, and what Quade.__call__, pack_table and unpack_table walk.
SCREEN = Stage("screen", "screen", "screen", "screen_params", (-1, len(SCREEN_COUNTERS)), "rows", "screen table",
               None, None, "screen_report", ("samples", "params"))
PIPE_STAGES = RUN_STAGES + (SCREEN,)  # quality, cycle, clip, trim, pairtrim, posttrim, filter, screen
PIPE_STAGE = {s.name: s for s in PIPE_STAGES}


# the adapter content table (qd_adapters_*): uint64, hist[R1, R2][16 probe slots, any][1025 bins] and then, per destination,
# dest[R1, R2][reads, 16 probe slots, any].  The probes are the first 12 bases of an adapter; the built-in ones are FastQC's
# adapter_list, in its order
ADAPTER_K, ADAPTER_PROBES, ADAPTER_BINS = 12, 16, 1025
ADAPTER_COLUMNS = ADAPTER_PROBES + 1  # the slots, then any
ADAPTER_HIST_VALUES = 2 * ADAPTER_COLUMNS * ADAPTER_BINS  # 34850
ADAPTER_DEST_VALUES = 2 * (ADAPTER_COLUMNS + 1)  # per destination: 36
ADAPTER_BUILTIN = (("illumina_universal", "AGATCGGAAGAG"), ("illumina_small_rna_3p", "TGGAATTCTCGG"),
                   ("illumina_small_rna_5p", "GATCGTCGGACT"), ("nextera_transposase", "CTGTCTCTTATA"),
                   ("poly_a", "AAAAAAAAAAAA"), ("poly_g", "GGGGGGGGGGGG"))


def adapters_values(n_samples):
    return ADAPTER_HIST_VALUES + (2 * n_samples + 1) * ADAPTER_DEST_VALUES


def adapters_views(flat):
    """The flat table (uint64[34850 + (2S+1) * 36]) as a dict of views into it: hist[2, 17, 1025] and dest[2S+1, 2, 18]"""
    flat = np.asarray(flat)
    rest = flat.size - ADAPTER_HIST_VALUES
    assert flat.ndim == 1 and flat.dtype == np.uint64 and rest >= ADAPTER_DEST_VALUES and rest % (2 * ADAPTER_DEST_VALUES) == ADAPTER_DEST_VALUES, \
        "adapter table of the wrong size"
    return {"hist": flat[:ADAPTER_HIST_VALUES].reshape(2, ADAPTER_COLUMNS, ADAPTER_BINS),
            "dest": flat[ADAPTER_HIST_VALUES:].reshape(-1, 2, ADAPTER_COLUMNS + 1)}


def adapters_flat(table):
    """adapters_views' dict (or a flat table) -> the flat layout of qd_adapters_read"""
    if isinstance(table, dict):
        table = np.concatenate([np.asarray(table[k], dtype=np.uint64).reshape(-1) for k in ("hist", "dest")])
    flat = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1)
    adapters_views(flat)  # (the size)
    return flat


# PIPE_STAGES is pinned at those eight in turn.  The adapter content (qd_adapters_*) is counted in front of all of them, on the
# reads as the scan left them: READ_STAGES is every stage in pipeline order, and what Quade.__call__, pack_table and unpack_table
# walk.  Its table's size depends on the sheet in one part only: shape (-1,), its value count in front of the packed table.
ADAPTERS = Stage("adapters", "adapters", "adapter_report", "adapter_params", (-1,), "values", "adapter table",
                 adapters_flat, adapters_views, "adapter_report", ("samples", "params"))
READ_STAGES = (ADAPTERS,) + PIPE_STAGES  # adapters, quality, cycle, clip, trim, pairtrim, posttrim, filter, screen
READ_STAGE = {s.name: s for s in READ_STAGES}


# READ_STAGES is pinned at those nine in turn, and so is where Quade.__call__ walks it.  The overlap base correction
# (qd_paircorrect_*) runs directly behind pairtrim: a Stage outside the tuples, which Quade.__call__ switches on and collects
# explicitly beside its two walks, the way it handles the duplication tally and the hopping matrix.  pack_table and unpack_table
# take it as they take any Stage.
PAIRCORRECT = Stage("paircorrect", "paircorrect", "pair_correction", "pair_correct_params", (PAIRCORRECT_VALUES,), None,
                    "an overlap correction table", None, None, "pair_correct_report", ("params",))


def _stage(stage):
    return stage if isinstance(stage, Stage) else READ_STAGE[stage]


def pack_table(stage, table):
    """One context's or rank's table of a stage (a Stage or its name) as bytes, for the ranks' exchange through the rendezvous
    directory: the count the stage writes in front, then the values.  Any array of the right size packs alike."""
    stage = _stage(stage)
    table = np.ascontiguousarray(stage.flat(table) if stage.flat else table, dtype=np.uint64).reshape(stage.shape)
    head = {"rows": table.shape[0], "values": table.size}.get(stage.count)
    return (b"" if head is None else np.array([head], dtype=np.uint64).tobytes()) + table.tobytes()


def unpack_table(stage, blob):
    """pack_table's bytes -> the table in the stage's shape, a writable copy (tables are summed in place)"""
    stage = _stage(stage)
    at = 8 if stage.count else 0
    n = int(np.frombuffer(blob, dtype=np.uint64, count=1)[0]) if stage.count else 0
    counted = stage.count == "rows" or stage.shape[0] == -1  # the count in front says how long the table is (adapters: its view checks it)
    values = n * int(np.prod(stage.shape[1:])) if counted else int(np.prod(stage.shape))
    assert len(blob) == at + values * 8 and (stage.count != "values" or n == values), stage.what + " of the wrong size"
    table = np.frombuffer(blob, dtype=np.uint64, offset=at).reshape((n,) + stage.shape[1:] if counted else stage.shape).copy()
    return stage.view(table) if stage.view else table
