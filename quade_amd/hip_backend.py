# -*- coding: utf-8 -*-
"""
ctypes binding of libquade_hip.so (include/quade_hip.h) -- the only compute path of this package.

There is deliberately no fallback: if the shared library is missing, or no gfx950 device is
usable, construction fails with an exception that says so.  numpy is used for host buffers only.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

# the read stages' table layouts, their bytes in the ranks' exchange and the stage table live in stages.py; hb.X reaches them all
from .stages import (ADAPTER_BINS, ADAPTER_BUILTIN, ADAPTER_COLUMNS, ADAPTER_DEST_VALUES, ADAPTER_HIST_VALUES, ADAPTER_K,  # noqa: F401
                     ADAPTER_PROBES, ADAPTERS, READ_STAGE, READ_STAGES, adapters_flat, adapters_values, adapters_views,
                     CLIP_COUNTERS, CSTATS_COUNTERS, CSTATS_CYCLES, CSTATS_GC_BINS, CSTATS_GR_VALUES, CSTATS_GROUPS,  # noqa: F401
                     CSTATS_LEN_BINS, CSTATS_MEANQ_BINS, CSTATS_SECTIONS, CSTATS_VALUES, FILTER_COUNTERS, FILTER_KEYS, FILTER_REASONS,
                     PAIRCORRECT, PAIRCORRECT_COUNTERS, PAIRCORRECT_VALUES, PAIRTRIM_BINS, PAIRTRIM_COUNTERS, PAIRTRIM_PAIR_COUNTERS, PAIRTRIM_VALUES, POSTTRIM, POSTTRIM_COUNTERS,
                     PIPE_STAGE, PIPE_STAGES, QSTATS_COUNTERS, RUN_STAGE, RUN_STAGES, SCREEN, SCREEN_ACTIONS, SCREEN_COUNTERS, STAGE,
                     STAGES, TRIM_COUNTERS, cstats_flat, cstats_views, pack_table, split_pairtrim, unpack_table)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libquade_hip.so")

QD_OK = 0
QD_ERR_INVALID, QD_ERR_NO_DEVICE, QD_ERR_HIP, QD_ERR_STATE = -1, -2, -3, -4
QD_ERR_UNSUPPORTED, QD_ERR_BARCODE, QD_ERR_FORMAT = -5, -6, -7
QD_UNKNOWN_READ_ERROR = -(1 << 40)  # qd_unknown_read: a value <= this is this + QD_ERR_*
QD_DUP_READ_ERROR = QD_UNKNOWN_READ_ERROR  # qd_dup_read follows the same protocol
DUP_COUNTERS = ("pairs", "short", "with_n", "sampled", "not_tallied")  # a destination's row of qd_dup_stats
CODE_UNDETERMINED = 0xFFFF


class QuadeHipError(RuntimeError):
    def __init__(self, code, text):
        RuntimeError.__init__(self, "libquade_hip error %d: %s" % (code, text))
        self.code = code


class qd_plan(C.Structure):
    _fields_ = [("dual", C.c_int32), ("min_qual", C.c_int32),
                ("idx1_start", C.c_int32), ("idx1_end", C.c_int32),
                ("idx2_start", C.c_int32), ("idx2_end", C.c_int32),
                ("mol1_start", C.c_int32), ("mol1_end", C.c_int32),
                ("mol2_start", C.c_int32), ("mol2_end", C.c_int32)]


class qd_layout(C.Structure):
    _fields_ = [("n_streams", C.c_int32),
                ("seq_off", C.c_int32 * 2), ("seq_width", C.c_int32 * 2), ("seq_stride", C.c_int32 * 2),
                ("qual_off", C.c_int32 * 2), ("qual_width", C.c_int32 * 2), ("qual_stride", C.c_int32 * 2),
                ("key_width", C.c_int32), ("mol_width", C.c_int32)]


class qd_rows(C.Structure):
    _fields_ = [("seq", C.c_void_p * 2), ("qual", C.c_void_p * 2), ("len", C.c_void_p * 2)]


class qd_clip_params(C.Structure):
    _fields_ = [("front_clip", C.c_int32 * 2), ("tail_clip", C.c_int32 * 2), ("window_size", C.c_int32), ("window_quality", C.c_int32),
                ("poly_g_min_length", C.c_int32), ("min_length", C.c_int32)]


class qd_trim_params(C.Structure):
    _fields_ = [("adapter_r1", C.c_uint8 * 64), ("adapter_r2", C.c_uint8 * 64), ("adapter_r1_len", C.c_int32), ("adapter_r2_len", C.c_int32),
                ("quality_cutoff", C.c_int32), ("min_overlap", C.c_int32), ("max_mismatch_pct", C.c_int32), ("min_length", C.c_int32)]


class qd_pairtrim_params(C.Structure):
    _fields_ = [("min_overlap", C.c_int32), ("max_mismatches", C.c_int32), ("max_mismatch_pct", C.c_int32), ("min_length", C.c_int32)]


class qd_paircorrect_params(C.Structure):
    _fields_ = [("good_quality", C.c_int32), ("bad_quality", C.c_int32)]


class qd_posttrim_params(C.Structure):
    _fields_ = [("tail_n", C.c_int32), ("poly_x_min_length", C.c_int32), ("max_length", C.c_int32 * 2), ("min_length", C.c_int32)]


class qd_screen_params(C.Structure):
    _fields_ = [("kmer", C.c_int32), ("min_hits", C.c_int32), ("action", C.c_int32)]


class qd_filter_params(C.Structure):
    _fields_ = [("min_length", C.c_int32), ("max_n", C.c_int32), ("max_unqualified_pct", C.c_int32), ("qualified_quality", C.c_int32),
                ("min_mean_quality", C.c_int32), ("min_complexity_pct", C.c_int32)]


class qd_dup_params(C.Structure):
    _fields_ = [("bases", C.c_int32), ("sample", C.c_int32), ("slots", C.c_int64)]


class qd_text_batch(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_int64), ("rec_off", C.c_void_p), ("n_records", C.c_int64),
                ("handle", C.c_void_p)]


class qd_slot_buffers(C.Structure):
    _fields_ = [("seq", C.c_void_p * 2), ("qual", C.c_void_p * 2), ("len", C.c_void_p * 2),
                ("codes", C.c_void_p), ("mol", C.c_void_p), ("max_pairs", C.c_int64),
                ("short_idx", C.c_void_p * 2), ("short_cap", C.c_int64)]


class qd_pipe_chunk(C.Structure):
    _fields_ = [("r1", C.c_char_p), ("r2", C.c_char_p), ("i1", C.c_char_p), ("i2", C.c_char_p), ("sink", C.c_void_p),
                ("begin_message", C.c_char_p), ("end_message", C.c_char_p),
                ("start_offset", C.c_int64 * 4), ("skip_bytes", C.c_int64 * 4), ("skip_kept", C.c_int64 * 4), ("max_pairs", C.c_int64)]


class qd_grain_info(C.Structure):
    _fields_ = [("file_offset", C.c_int64), ("n_lines", C.c_uint32), ("kept", C.c_uint32 * 4), ("skip_bytes", C.c_uint32 * 4),
                ("incomplete", C.c_uint32 * 4)]


class qd_pipe_stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("pairs", "batches", "bgzf_blocks", "host_inflated_runs", "text_segments", "pieces",
                                         "host_coded_pieces", "text_in_bytes", "text_out_bytes", "gzip_bytes", "rescans")] + \
               [(n, C.c_double) for n in ("run_s", "wait_input_s", "wait_sync_s", "wait_out_set_s", "alloc_s", "collector_wait_s", "download_s", "append_s")] + \
               [(n, C.c_int64) for n in ("gzip_steps", "gzip_units", "gzip_members", "gzip_fallbacks")]


STREAM_CONTEXT = C.c_void_p(-1)  # QD_STREAM_CONTEXT: the context's own stream (None/0 = HIP's null stream)


# every symbol include/quade_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("qd_plan_layout", C.c_int, [C.POINTER(qd_plan), C.POINTER(qd_layout)]),
    ("qd_version", C.c_int, []),
    ("qd_strerror", C.c_char_p, [C.c_int]),
    ("qd_last_error", C.c_char_p, [_P]),
    ("qd_device_count", C.c_int, [C.POINTER(C.c_int32)]),
    ("qd_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("qd_destroy", C.c_int, [_P]),
    ("qd_device_info", C.c_int, [_P, C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("qd_set_plan", C.c_int, [_P, C.POINTER(qd_plan)]),
    ("qd_get_layout", C.c_int, [_P, C.POINTER(qd_layout)]),
    ("qd_set_barcodes", C.c_int, [_P, C.c_int32, _P, _P]),
    ("qd_demux_device", C.c_int, [_P, C.c_int64, C.POINTER(qd_rows), _P, _P, _P]),
    ("qd_demux_device_ragged", C.c_int, [_P, C.c_int64, C.POINTER(qd_rows), _P, _P, C.c_int64, _P, _P]),
    ("qd_kernel_kind", C.c_int, [_P, C.c_int]),
    ("qd_set_option", C.c_int, [_P, C.c_char_p, C.c_int64]),
    ("qd_check_mismatch_collisions", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("qd_set_mismatches", C.c_int, [_P, C.c_int32, C.c_int32]),
    ("qd_unknown_enable", C.c_int, [_P, C.c_int64]),
    ("qd_unknown_stats", C.c_int, [_P, _P]),
    ("qd_unknown_read", C.c_int64, [_P, _P, _P, C.c_int64]),
    ("qd_hop_index", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("qd_hop_enable", C.c_int, [_P, C.c_int32]),
    ("qd_hop_shape", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("qd_hop_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_hop_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_qstats_enable", C.c_int, [_P, C.c_int32]),
    ("qd_qstats_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_qstats_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_qstats_kind", C.c_int, [_P]),
    ("qd_clip_set", C.c_int, [_P, C.POINTER(qd_clip_params)]),
    ("qd_clip_get", C.c_int, [_P, C.POINTER(qd_clip_params)]),
    ("qd_clip_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_clip_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_trim_set", C.c_int, [_P, C.POINTER(qd_trim_params)]),
    ("qd_trim_get", C.c_int, [_P, C.POINTER(qd_trim_params)]),
    ("qd_trim_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_trim_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_pairtrim_set", C.c_int, [_P, C.POINTER(qd_pairtrim_params)]),
    ("qd_pairtrim_get", C.c_int, [_P, C.POINTER(qd_pairtrim_params)]),
    ("qd_pairtrim_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_pairtrim_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_paircorrect_set", C.c_int, [_P, C.POINTER(qd_paircorrect_params)]),
    ("qd_paircorrect_get", C.c_int, [_P, C.POINTER(qd_paircorrect_params)]),
    ("qd_paircorrect_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_paircorrect_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_posttrim_set", C.c_int, [_P, C.POINTER(qd_posttrim_params)]),
    ("qd_posttrim_get", C.c_int, [_P, C.POINTER(qd_posttrim_params)]),
    ("qd_posttrim_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_posttrim_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_screen_set", C.c_int, [_P, C.POINTER(qd_screen_params), _P, C.c_int64]),
    ("qd_screen_get", C.c_int, [_P, C.POINTER(qd_screen_params), C.POINTER(C.c_int64)]),
    ("qd_screen_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_screen_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_screen_kind", C.c_int, [_P]),
    ("qd_screen_first_slot", C.c_int64, [C.c_uint64, C.c_int64]),
    ("qd_filter_set", C.c_int, [_P, C.POINTER(qd_filter_params)]),
    ("qd_filter_get", C.c_int, [_P, C.POINTER(qd_filter_params)]),
    ("qd_filter_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_filter_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_filter_kind", C.c_int, [_P]),
    ("qd_cstats_enable", C.c_int, [_P, C.c_int32]),
    ("qd_cstats_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_cstats_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_cstats_lds_cycles", C.c_int, []),
    ("qd_adapters_set", C.c_int, [_P, _P, C.c_int32]),
    ("qd_adapters_get", C.c_int, [_P, _P, C.POINTER(C.c_int32)]),
    ("qd_adapters_read", C.c_int, [_P, _P, C.c_int64]),
    ("qd_adapters_add", C.c_int, [_P, _P, C.c_int64]),
    ("qd_dup_set", C.c_int, [_P, C.POINTER(qd_dup_params)]),
    ("qd_dup_get", C.c_int, [_P, C.POINTER(qd_dup_params)]),
    ("qd_dup_stats", C.c_int, [_P, _P, C.c_int64]),
    ("qd_dup_read", C.c_int64, [_P, _P, _P, C.c_int64]),
    ("qd_get_counts", C.c_int, [_P, _P, C.c_int32]),
    ("qd_reset_counts", C.c_int, [_P]),
    ("qd_add_counts", C.c_int, [_P, _P, C.c_int32]),
    ("qd_synchronize", C.c_int, [_P]),
    ("qd_slots_create", C.c_int, [_P, C.c_int32, C.c_int64]),
    ("qd_slots_destroy", C.c_int, [_P]),
    ("qd_slot_get", C.c_int, [_P, C.c_int32, C.POINTER(qd_slot_buffers)]),
    ("qd_submit", C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32]),
    ("qd_submit_ragged", C.c_int, [_P, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    ("qd_wait", C.c_int, [_P, C.c_int32]),
    ("qd_fastq_index", C.c_int64, [_P, C.c_int64, C.c_int64, _P, C.POINTER(C.c_int64)]),
    ("qd_pack_index_fastq", C.c_int64, [C.POINTER(qd_layout), C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, _P,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int64), _P, C.c_int64,
                                        C.POINTER(C.c_int64)]),
    ("qd_pack_index_reads", C.c_int, [C.POINTER(qd_layout), C.c_int32, C.c_int64, _P, _P, _P, _P, _P, _P,
                                      C.POINTER(C.c_int32)]),
    ("qd_build_tags", C.c_int, [C.POINTER(qd_layout), C.POINTER(qd_plan), C.c_int64, C.POINTER(_P), C.POINTER(_P), _P,
                                _P, C.c_int32, _P]),
    ("qd_format_records", C.c_int64, [_P, _P, _P, C.c_int64, _P, C.c_int32, _P, _P, C.c_int64]),
    ("qd_comm_unique_id", C.c_int, [_P]),
    ("qd_comm_create_local", C.c_int, [C.POINTER(_P), C.c_int32, C.POINTER(_P)]),
    ("qd_comm_create_rank", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    ("qd_comm_world", C.c_int, [_P]),
    ("qd_reduce_counts", C.c_int, [_P, _P, C.c_int32]),
    ("qd_comm_destroy", C.c_int, [_P]),
    ("qd_comm_last_error", C.c_char_p, []),
    ("qd_io_stage_seconds", C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    ("qd_write_gzip_file", C.c_int, [C.c_char_p, _P, C.c_int64, C.c_int32, C.c_int64]),
    ("qd_reader_open", C.c_int, [C.c_char_p, C.c_int64, C.c_int32, C.POINTER(_P)]),
    ("qd_reader_open_on", C.c_int, [C.c_char_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("qd_reader_inflate_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("qd_inflater_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("qd_inflater_run", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int32)]),
    ("qd_inflater_run_pinned", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int32)]),
    ("qd_pinned_alloc", _P, [C.c_int64]),
    ("qd_pinned_free", None, [_P]),
    ("qd_inflater_destroy", C.c_int, [_P]),
    ("qd_inflater_last_error", C.c_char_p, [_P]),
    ("qd_io_set_option", C.c_int, [C.c_char_p, C.c_int64]),
    ("qd_reader_gunzip_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("qd_gunzip_buffer", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64), _P]),
    ("qd_gunzip_last_error", C.c_char_p, []),
    ("qd_deflater_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("qd_deflater_run", C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    ("qd_huffman_member_bound", C.c_int64, [C.c_int64]),
    ("qd_deflater_set_level", C.c_int, [_P, C.c_int32]),
    ("qd_inflater_set_form", C.c_int, [_P, C.c_int32]),
    ("qd_deflater_destroy", C.c_int, [_P]),
    ("qd_deflater_last_error", C.c_char_p, [_P]),
    ("qd_sink_set_device_deflate", C.c_int, [_P, C.c_int32]),
    ("qd_sink_device_members", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("qd_reader_next", C.c_int, [_P, C.POINTER(qd_text_batch)]),
    ("qd_text_batch_free", C.c_int, [_P]),
    ("qd_reader_close", C.c_int, [_P]),
    ("qd_reader_last_error", C.c_char_p, [_P]),
    ("qd_io_threads", C.c_int, [C.c_int32]),
    ("qd_io_backend", C.c_int, []),
    ("qd_host_cores", C.c_int, []),
    ("qd_sink_create", C.c_int, [C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 C.POINTER(_P)]),
    ("qd_sink_set_quiet", C.c_int, [_P, C.c_int32]),
    ("qd_sink_route", C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int32, _P]),
    ("qd_sink_route_batches", C.c_int, [_P, C.c_int64, _P, C.POINTER(qd_text_batch), C.POINTER(qd_text_batch), _P, C.c_int32, _P]),
    ("qd_sink_flush", C.c_int, [_P]),
    ("qd_sink_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("qd_sink_last_error", C.c_char_p, [_P]),
    ("qd_sink_close", C.c_int, [_P]),
    ("qd_pipe_create", C.c_int, [_P, C.POINTER(_P)]),
    ("qd_pipe_set_option", C.c_int, [_P, C.c_char_p, C.c_int64]),
    ("qd_pipe_run", C.c_int, [_P, C.POINTER(qd_pipe_chunk), C.c_int32, C.POINTER(qd_pipe_stats)]),
    ("qd_pipe_index", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(qd_grain_info), C.c_int32, C.POINTER(C.c_int32)]),
    ("qd_pipe_last_error", C.c_char_p, [_P]),
    ("qd_pipe_destroy", C.c_int, [_P]),
    ("qd_dev_fastq_scan", C.c_int64, [C.c_int, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _P, C.c_int64, _P]),
    ("qd_dev_crc32", C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, C.POINTER(C.c_uint32)]),
    ("qd_pool_trim", C.c_int, []),
    ("qd_dev_gunzip", C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64), C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    ("qd_dev_sort_by_dest", C.c_int, [C.c_int, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    ("qd_dev_qstats", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P]),
    ("qd_dev_clip", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("qd_dev_trim", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("qd_dev_pairtrim", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("qd_dev_paircorrect", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P, _P]),
    ("qd_dev_posttrim", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("qd_dev_filter", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("qd_dev_screen", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P]),
    ("qd_dev_cstats", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("qd_dev_dup", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("qd_dev_adapters", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P]),
    ("qd_dev_pack_rows", C.c_int, [C.c_int, C.POINTER(qd_layout), _P * 2, C.c_int64 * 2, _P * 2, C.c_int64, C.c_int64, _P * 2, _P * 2, _P * 2,
                                   _P, C.c_int64, C.POINTER(C.c_uint32)]),
    ("qd_dev_route_format", C.c_int, [C.c_int, C.POINTER(qd_plan), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P * 4, C.c_int64 * 4, _P * 4, _P, _P,
                                      C.c_int64, C.c_int32] + [_P] * 13 + [C.c_int64, C.POINTER(C.c_int64)]),
    ("qd_dev_pack_members", C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64]),
    ("qd_get_plan", C.c_int, [_P, C.POINTER(qd_plan)]),
    ("qd_context_device", C.c_int, [_P, C.POINTER(C.c_int32)]),
]

_lib = None


def load_library(path=None):
    """Loads libquade_hip.so and types every entry point.  Raises (never falls back)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    default = path is None
    path = path or os.environ.get("QUADE_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            "%s not found: build it first (python -c 'import __graft_entry__ as g; g.build()' or "
            "make -C quade_amd/csrc).  quade_amd has no CPU fallback." % path)
    _preload_shared_hip_runtime()
    lib = C.CDLL(path)
    for name, restype, argtypes in SYMBOLS:
        if not default and not hasattr(lib, name):
            continue  # an explicitly given build (A/B variants of older sources in tools/tune.py) may predate an entry point
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    if default:
        _lib = lib
    return lib


def _preload_shared_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64 (soname
    libamdhip64.so.7, same as the system one this library links).  If ours is loaded first the
    system copy gets mapped, a later `import torch` maps its bundled copy as well, and the second
    HSA initialisation finds no GPU.  Mapping torch's copy first (when torch is installed; torch
    itself is not imported) makes both sides resolve to the same runtime whatever the import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _ptr(a):
    """address of a numpy array (host) / int address / None"""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    return a.ctypes.data


def plan_layout(plan: qd_plan) -> qd_layout:
    lib = load_library()
    lay = qd_layout()
    r = lib.qd_plan_layout(C.byref(plan), C.byref(lay))
    if r != QD_OK:
        raise QuadeHipError(r, lib.qd_strerror(r).decode())
    return lay


def make_plan(dual, min_qual, idx1, idx2=(0, 0), mol1=(0, 0), mol2=(0, 0)) -> qd_plan:
    """Positions are (start0, end) pairs exactly as src/Quade.py:105-116 stores them."""
    return qd_plan(int(bool(dual)), int(min_qual), idx1[0], idx1[1], idx2[0], idx2[1],
                   mol1[0], mol1[1], mol2[0], mol2[1])


# ---- host helpers (no GPU) ---------------------------------------------------------------------------
def fastq_index(text: bytes | np.ndarray, max_records=None):
    """Offsets of the kept records of decompressed fastq text (see qd_fastq_index).
    Returns (rec_off int64[n+1], consumed)."""
    lib = load_library()
    buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    if max_records is None:
        max_records = int(np.count_nonzero(buf == 10)) // 4 + 1
    off = np.empty(max_records + 1, dtype=np.int64)
    consumed = C.c_int64(0)
    n = lib.qd_fastq_index(_ptr(buf), buf.size, max_records, _ptr(off), C.byref(consumed))
    if n < 0:
        raise QuadeHipError(int(n), lib.qd_strerror(int(n)).decode())
    return off[:n + 1], consumed.value


def pack_index_fastq(layout: qd_layout, k: int, text, seq_rows, qual_rows, len_rows, max_records, short_idx=None):
    """Packs stream k from fastq text into the given row arrays (numpy uint8, C-contiguous, or raw
    addresses).  short_idx: uint32 array that receives the indices of the reads shorter than their
    window.  Returns (n_records, all_full, consumed, n_short)."""
    lib = load_library()
    buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    full = C.c_int32(1)
    consumed = C.c_int64(0)
    n_short = C.c_int64(0)
    n = lib.qd_pack_index_fastq(C.byref(layout), k, _ptr(buf), buf.size, max_records, _ptr(seq_rows),
                                _ptr(qual_rows), _ptr(len_rows), C.byref(full), C.byref(consumed),
                                _ptr(short_idx), 0 if short_idx is None else short_idx.size, C.byref(n_short))
    if n < 0:
        raise QuadeHipError(int(n), lib.qd_strerror(int(n)).decode())
    return int(n), bool(full.value), consumed.value, n_short.value


def pack_index_reads(layout: qd_layout, k: int, seqs, quals):
    """Packs lists of bytes (sequences, quality strings) -> (seq_rows, qual_rows, len_rows, all_full)."""
    lib = load_library()
    n = len(seqs)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=n)
    assert all(len(q) == len(s) for s, q in zip(seqs, quals)), "seq/qual length mismatch"
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    seq = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)
    qual = np.frombuffer(b"".join(quals) + b"\0", dtype=np.uint8)
    seq_rows = np.empty((n, layout.seq_stride[k]), dtype=np.uint8)
    qual_rows = np.empty((n, layout.qual_stride[k]), dtype=np.uint8)
    len_rows = np.empty(n, dtype=np.uint8)
    full = C.c_int32(1)
    r = lib.qd_pack_index_reads(C.byref(layout), k, n, _ptr(seq), _ptr(qual), _ptr(offsets), _ptr(seq_rows),
                                _ptr(qual_rows), _ptr(len_rows), C.byref(full))
    if r != QD_OK:
        raise QuadeHipError(r, lib.qd_strerror(r).decode())
    return seq_rows, qual_rows, len_rows, bool(full.value)


def build_tags(layout: qd_layout, plan: qd_plan, n, seq_rows, len_rows=None, mol_rows=None):
    """Name suffixes ':IDX[:MOL]' of n pairs -> (tag_rows uint8 [n, stride], tag_len uint8 [n]).
    mol_rows: the device's molecular output (n x mol_width), used for the MOL part when given."""
    lib = load_library()
    stride = 2 + layout.key_width + layout.mol_width
    tags = np.empty((max(n, 1), stride), dtype=np.uint8)
    tlen = np.empty(max(n, 1), dtype=np.uint8)
    sp = (_P * 2)(*[_ptr(seq_rows[k]) if k < len(seq_rows) else None for k in range(2)])
    lp = (_P * 2)(*[(_ptr(len_rows[k]) if len_rows and k < len(len_rows) else None) for k in range(2)])
    r = lib.qd_build_tags(C.byref(layout), C.byref(plan), int(n), sp, lp,
                          _ptr(mol_rows) if layout.mol_width else None, _ptr(tags), stride, _ptr(tlen))
    if r != QD_OK:
        raise QuadeHipError(r, lib.qd_strerror(r).decode())
    return tags[:n], tlen[:n]


def format_records(text, rec_off, sel, tags, tag_len):
    """Output text of the records `sel` (int64 indices) of `text` with their name tags, as a numpy
    uint8 array (buffer protocol: zlib and file.write take it without another copy)."""
    lib = load_library()
    buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    sel = np.ascontiguousarray(sel, dtype=np.int64)
    if sel.size == 0:
        return np.empty(0, dtype=np.uint8)
    cap = int((rec_off[sel + 1] - rec_off[sel]).sum() + tag_len[sel].astype(np.int64).sum() + 8 * sel.size)
    out = np.empty(cap, dtype=np.uint8)
    n = lib.qd_format_records(_ptr(buf), _ptr(rec_off), _ptr(sel), sel.size, _ptr(tags), tags.shape[1],
                              _ptr(tag_len), _ptr(out), cap)
    if n < 0:
        raise QuadeHipError(int(n), "qd_format_records failed")
    return out[:n]


def device_count():
    """Number of HIP devices the library sees; raises when there is none (no CPU fallback)."""
    lib = load_library()
    n = C.c_int32(0)
    r = lib.qd_device_count(C.byref(n))
    if r != QD_OK:
        raise QuadeHipError(r, lib.qd_last_error(None).decode())
    return n.value


def _barcode_blob(barcodes):
    """list of str/bytes -> (blob uint8, offsets int32[S+1]) as qd_set_barcodes takes them"""
    bs = [b.encode("latin-1") if isinstance(b, str) else bytes(b) for b in barcodes]
    offs = np.zeros(len(bs) + 1, dtype=np.int32)
    if bs:
        np.cumsum([len(b) for b in bs], out=offs[1:])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), offs, len(bs)


def check_mismatch_collisions(barcodes, key_width, w1, m1, m2):
    """Host only (no GPU): the first colliding ordinal pair (i, j) of the sample sheet under budgets (m1, m2) -- barcodes of
    length key_width whose per-part Hamming distances are <= 2*m1 on [0, w1) and <= 2*m2 on [w1, key_width) -- or None."""
    lib = load_library()
    blob, offs, n = _barcode_blob(barcodes)
    a, b = C.c_int32(-1), C.c_int32(-1)
    r = lib.qd_check_mismatch_collisions(n, _ptr(blob), _ptr(offs), int(key_width), int(w1), int(m1), int(m2),
                                         C.byref(a), C.byref(b))
    if r == QD_ERR_BARCODE:
        return a.value, b.value
    if r != QD_OK:
        raise QuadeHipError(r, lib.qd_strerror(r).decode())
    return None


HOP_MAX_CELLS = 1 << 24  # (n1 + 1) * (n2 + 1) at most (include/quade_hip.h)


def hop_index(barcodes, key_width, w1):
    """Host only (no GPU): the part lists of the index-hopping matrix, as qd_hop_index defines them -- (part1 int32[S], part2
    int32[S], n1, n2): per sample the ordinal of its index-1 / index-2 value among the sheet's distinct values in order of first
    appearance, -1 for a barcode that is not key_width long.  A sheet over the limit raises QuadeHipError(QD_ERR_UNSUPPORTED)."""
    lib = load_library()
    blob, offs, n = _barcode_blob(barcodes)
    part1, part2 = np.full(max(n, 1), -1, dtype=np.int32), np.full(max(n, 1), -1, dtype=np.int32)
    n1, n2 = C.c_int32(0), C.c_int32(0)
    r = lib.qd_hop_index(n, _ptr(blob), _ptr(offs), int(key_width), int(w1), _ptr(part1), _ptr(part2), C.byref(n1), C.byref(n2))
    if r == QD_ERR_UNSUPPORTED:
        raise QuadeHipError(r, "%d x %d distinct index values: (n1+1)*(n2+1) may not exceed %d" % (n1.value, n2.value, HOP_MAX_CELLS))
    if r != QD_OK:
        raise QuadeHipError(r, lib.qd_strerror(r).decode())
    return part1[:n], part2[:n], n1.value, n2.value


def hop_values(n1, n2):
    """values of an index-hopping table: the (n1 + 1) x (n2 + 1) cells and `short`"""
    return (n1 + 1) * (n2 + 1) + 1


def pack_hop(n1, n2, table):
    """One context's or rank's index-hopping table as bytes (the ranks' exchange through the rendezvous directory): n1 and n2 in
    front of the values; unpack_hop reverses it."""
    table = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1)
    assert table.size == hop_values(n1, n2), "an index-hopping table of %d values for %d x %d parts" % (table.size, n1, n2)
    return np.array([n1, n2], dtype=np.uint64).tobytes() + table.tobytes()


def unpack_hop(blob):
    """-> (n1, n2, table uint64[(n1+1)*(n2+1)+1]); asserts that the blob holds exactly what its head names"""
    assert len(blob) >= 16, "an index-hopping table of %d bytes has no head" % len(blob)
    n1, n2 = (int(x) for x in np.frombuffer(blob, dtype=np.uint64, count=2))
    assert len(blob) == 16 + 8 * hop_values(n1, n2), \
        "an index-hopping table of %d bytes does not hold the %d x %d parts its head names" % (len(blob), n1, n2)
    return n1, n2, np.frombuffer(blob, dtype=np.uint64, count=hop_values(n1, n2), offset=16)


def _merge_keyed(keys, counts):
    """Key rows [n, w] with one count each -> (the distinct rows ascending, per row the sum of its counts as uint64)."""
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    total = np.zeros(uniq.shape[0], dtype=np.uint64)
    np.add.at(total, inv.reshape(-1), counts)
    return uniq, total


def merge_unknown(tables):
    """Host: unknown-barcode tables (keys uint8[n, K], counts uint64[n]) of several contexts or ranks -> one table with the counts
    of equal keys summed, in report order: count descending, then key bytes ascending.  Returns (keys, counts)."""
    tables = [(np.asarray(k, dtype=np.uint8), np.asarray(c, dtype=np.uint64)) for k, c in tables]
    tables = [(k.reshape(c.size, -1), c) for k, c in tables if c.size]
    if not tables:
        return np.zeros((0, 0), dtype=np.uint8), np.zeros(0, dtype=np.uint64)
    K = tables[0][0].shape[1]
    assert all(k.shape[1] == K for k, _ in tables), "tables of different key widths"
    uniq, total = _merge_keyed(np.concatenate([k for k, _ in tables]), np.concatenate([c for _, c in tables]))
    order = np.argsort(-total.astype(np.int64), kind="stable")
    return np.ascontiguousarray(uniq[order]), total[order]


def pack_unknown(keys, counts, short, dropped):
    """One context's or rank's tally as bytes (the ranks' exchange through the rendezvous directory); unpack_unknown reverses it."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(len(counts), -1) if len(counts) else np.zeros((0, 0), dtype=np.uint8)
    head = np.array([len(counts), keys.shape[1] if len(counts) else 0, short, dropped], dtype=np.uint64)
    return head.tobytes() + keys.tobytes() + np.ascontiguousarray(counts, dtype=np.uint64).tobytes()


def unpack_unknown(blob):
    """-> (keys uint8[n, K], counts uint64[n], short, dropped)"""
    n, K, short, dropped = (int(x) for x in np.frombuffer(blob, dtype=np.uint64, count=4))
    keys = np.frombuffer(blob, dtype=np.uint8, count=n * K, offset=32).reshape(n, K)
    counts = np.frombuffer(blob, dtype=np.uint64, count=n, offset=32 + n * K)
    return keys, counts, short, dropped


def merge_dup(tables):
    """Host: duplication tables (keys uint64[n, 3] = (w1, w2, d), counts uint64[n]) of several contexts or ranks -> one table with
    the counts of equal keys summed, rows ascending by (d, w1, w2); a single table holds every key once already and is returned as
    it is.  Returns (keys, counts)."""
    tables = [(np.asarray(k, dtype=np.uint64).reshape(-1, 3), np.asarray(c, dtype=np.uint64).reshape(-1)) for k, c in tables]
    assert all(k.shape[0] == c.size for k, c in tables), "one count per key"
    tables = [(k, c) for k, c in tables if c.size]
    if not tables:
        return np.zeros((0, 3), dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    if len(tables) == 1:
        return tables[0]
    uniq, total = _merge_keyed(np.concatenate([k for k, _ in tables])[:, [2, 0, 1]], np.concatenate([c for _, c in tables]))
    return np.ascontiguousarray(uniq[:, [1, 2, 0]]), total


_DUP_MAGIC = 0x3150554445445551  # "QUDEDUP1"


def pack_dup(keys, counts, stats):
    """One context's or rank's tally as bytes (the ranks' exchange through the rendezvous directory): keys uint64[n, 3], counts
    uint64[n], stats uint64[2S+1, 5] (dup_stats); unpack_dup reverses it."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(counts.size, 3)
    stats = np.ascontiguousarray(stats, dtype=np.uint64).reshape(-1, len(DUP_COUNTERS))
    head = np.array([_DUP_MAGIC, counts.size, stats.shape[0]], dtype=np.uint64)
    return head.tobytes() + stats.tobytes() + keys.tobytes() + counts.tobytes()


def unpack_dup(blob):
    """-> (keys uint64[n, 3], counts uint64[n], stats uint64[rows, 5]); ValueError when the blob is not whole"""
    if len(blob) < 24:
        raise ValueError("a duplication table of %d bytes has no head" % len(blob))
    magic, n, rows = (int(x) for x in np.frombuffer(blob, dtype=np.uint64, count=3))
    V = len(DUP_COUNTERS)
    if magic != _DUP_MAGIC or len(blob) != 24 + 8 * (rows * V + 4 * n):
        raise ValueError("a duplication table of %d bytes does not hold the %d entries and %d rows its head names" % (len(blob), n, rows))
    stats = np.frombuffer(blob, dtype=np.uint64, count=rows * V, offset=24).reshape(rows, V)
    keys = np.frombuffer(blob, dtype=np.uint64, count=3 * n, offset=24 + 8 * rows * V).reshape(n, 3)
    counts = np.frombuffer(blob, dtype=np.uint64, count=n, offset=24 + 8 * (rows * V + 3 * n))
    return keys, counts, stats


FILTER_KIND_LDS, FILTER_KIND_GLOBAL = 1, 2


# ---- device context -------------------------------------------------------------------------------------
class Engine(object):
    """One libquade_hip context = one MI355X.  Mirrors what Sample.CLASS_INIT + Sample(name, index)
    configure in the reference (src/Sample.py:48-54,132-153) and runs FINDER for whole batches."""

    def __init__(self, device_id=0, lib_path=None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        r = self.lib.qd_create(int(device_id), C.byref(h))
        if r != QD_OK:
            raise QuadeHipError(r, self.lib.qd_last_error(None).decode())
        self._h = h
        self.device_id = int(device_id)
        self.n_samples = 0
        self.layout = None
        self._slot_views = {}

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self.lib.qd_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r != QD_OK:
            raise QuadeHipError(r, self.lib.qd_last_error(self._h).decode() or self.lib.qd_strerror(r).decode())

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_int32(0), C.c_int64(0)
        self._chk(self.lib.qd_device_info(self._h, name, 256, C.byref(cus), C.byref(mem)))
        return {"name": name.value.decode(), "compute_units": cus.value, "total_mem": mem.value}

    # -- configuration
    def set_plan(self, plan: qd_plan):
        self._chk(self.lib.qd_set_plan(self._h, C.byref(plan)))
        lay = qd_layout()
        self._chk(self.lib.qd_get_layout(self._h, C.byref(lay)))
        self.layout = lay
        self.plan = plan
        return lay

    def set_barcodes(self, barcodes):
        """barcodes: list of upper-case str/bytes in sample-ordinal order (SAMPLE_LIST order)."""
        bs = [b.encode("latin-1") if isinstance(b, str) else bytes(b) for b in barcodes]
        offs = np.zeros(len(bs) + 1, dtype=np.int32)
        if bs:
            np.cumsum([len(b) for b in bs], out=offs[1:])
        blob = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8)
        self._chk(self.lib.qd_set_barcodes(self._h, len(bs), _ptr(blob), _ptr(offs)))
        self.n_samples = len(bs)

    def set_mismatches(self, m1, m2=0):
        """Mismatch budgets of index read 1's and index read 2's part (0..2 each; qd_set_mismatches).  After set_barcodes:
        set_plan and set_barcodes reset them to 0."""
        self._chk(self.lib.qd_set_mismatches(self._h, int(m1), int(m2)))

    def unknown_enable(self, slots):
        """Tally of the unknown barcodes (qd_unknown_enable): a device table of `slots` entries (a power of two, 2^10 .. 2^28)
        counts the fused barcode keys of the pairs that stay Undetermined; 0 turns it off.  After set_barcodes (and
        set_mismatches): set_plan and set_barcodes turn it off, reset_counts empties it."""
        self._chk(self.lib.qd_unknown_enable(self._h, int(slots)))

    def unknown_stats(self):
        """numpy uint64[4]: tallied pairs, short slices, dropped (not admitted to the table), distinct entries"""
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.qd_unknown_stats(self._h, _ptr(out)))
        return out

    def _tally_read(self, fn, width, dtype):
        """A key tally's entries through its qd_*_read entry `fn` (one sizing protocol: asked for the size, then read with that
        room until the table has not grown meanwhile): (keys dtype[n, width], counts uint64[n])."""
        n = fn(self._h, None, None, 0)
        while True:
            if n <= QD_UNKNOWN_READ_ERROR:
                self._chk(int(n - QD_UNKNOWN_READ_ERROR))
            if n == 0:
                return np.zeros((0, width), dtype=dtype), np.zeros(0, dtype=np.uint64)
            cap = int(-n)
            keys = np.zeros((cap, width), dtype=dtype)
            counts = np.zeros(cap, dtype=np.uint64)
            n = fn(self._h, _ptr(keys), _ptr(counts), cap)
            if n > 0:
                return keys[:n], counts[:n]

    def unknown_read(self):
        """The table's entries in no particular order: (keys uint8[n, key_width], counts uint64[n])."""
        return self._tally_read(self.lib.qd_unknown_read, self.layout.key_width if self.layout is not None else 0, np.uint8)

    def hop_enable(self, on=True):
        """Index-hopping matrix (qd_hop_enable; conf.HOPPING_HELP has the definition): every pair that stays Undetermined is
        counted in the cell (its index 1 among the sheet's distinct index-1 values, its index 2 among the distinct index-2
        values), on every launch path.  A dual plan only.  After set_barcodes (and set_mismatches): set_plan and set_barcodes turn
        it off, reset_counts zeroes it."""
        self._chk(self.lib.qd_hop_enable(self._h, int(bool(on))))

    def hop_shape(self):
        """(n1, n2): the sheet's distinct index-1 and index-2 values"""
        n1, n2 = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.qd_hop_shape(self._h, C.byref(n1), C.byref(n2)))
        return n1.value, n2.value

    def hop_read(self):
        """numpy uint64[(n1+1)*(n2+1)+1]: the cells row-major (row n1 / column n2 = no part), then `short`"""
        n1, n2 = self.hop_shape()
        return self._table_read(self.lib.qd_hop_read, hop_values(n1, n2))

    def hop_add(self, table):
        """Another context's table (hop_read's layout) joins this context's (qd_hop_add)."""
        self._table_add(self.lib.qd_hop_add, table)

    # -- the read stages: what their dev_* and *_add methods share
    @staticmethod
    def _pair_inputs(text1, recs1, text2, recs2, codes=None, drop=None):
        """A batch as the qd_dev_* entries take it: texts as bytes or uint8 arrays, recs uint32[n, 6] in dev_fastq_scan's layout,
        codes None or uint16[n], drop None or uint8[n] -> (the two texts, the two record tables, codes, drop, n), contiguous."""
        t = [np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)
             for x in (text1, text2)]
        r = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, 6) for x in (recs1, recs2)]
        n = r[0].shape[0]
        if codes is None:
            if r[1].shape[0] != n:
                raise ValueError("recs1 and recs2 must have one entry per pair")
        else:
            codes = np.ascontiguousarray(codes, dtype=np.uint16).reshape(-1)
            if not (r[1].shape[0] == n == codes.size):
                raise ValueError("recs1, recs2 and codes must have one entry per pair")
        if drop is not None:
            drop = np.ascontiguousarray(drop, dtype=np.uint8)
            if drop.shape != (n,):
                raise ValueError("drop must have one byte per pair")
        return t, r, codes, drop, n

    def _dev_recs(self, fn, text1, recs1, text2, recs2):
        """a stage that writes new record tables (qd_dev_clip, qd_dev_trim, qd_dev_pairtrim, qd_dev_posttrim) -> the two tables"""
        t, r, _, _, n = self._pair_inputs(text1, recs1, text2, recs2)
        out = [np.zeros_like(x) for x in r]
        self._chk(fn(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n, _ptr(out[0]), _ptr(out[1])))
        return out[0], out[1]

    def _table_read(self, fn, shape):
        """a table through its qd_*_read entry `fn` -> uint64 of `shape`"""
        out = np.zeros(shape, dtype=np.uint64)
        self._chk(fn(self._h, _ptr(out), out.size))
        return out

    def _table_add(self, fn, table):
        table = np.ascontiguousarray(table, dtype=np.uint64)
        self._chk(fn(self._h, _ptr(table), table.size))

    def qstats_enable(self, on=True):
        """Yield and quality counters per destination (qd_qstats_enable): every pair the device pipeline routes adds its two
        insert reads to a device table.  After set_barcodes: set_plan and set_barcodes turn it off, reset_counts zeroes it."""
        self._chk(self.lib.qd_qstats_enable(self._h, int(bool(on))))

    def qstats_read(self):
        """numpy uint64[2S+1, 2, 6]: [destination (code; Undetermined last)][R1, R2][QSTATS_COUNTERS]"""
        return self._table_read(self.lib.qd_qstats_read, (2 * self.n_samples + 1, 2, len(QSTATS_COUNTERS)))

    def qstats_add(self, table):
        """Another context's table (qstats_read's layout) joins this context's (qd_qstats_add)."""
        self._table_add(self.lib.qd_qstats_add, table)

    def qstats_kind(self):
        """How a launch accumulates: "lds" (per-workgroup partials) or "global" (64-bit global atomics)."""
        kind = self.lib.qd_qstats_kind(self._h)
        if kind < 0:
            self._chk(kind)
        return {1: "lds", 2: "global"}[kind]

    def dev_qstats(self, text1, recs1, text2, recs2, codes):
        """The counters' stage over host buffers (qd_dev_qstats): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout, codes uint16[n]; adds to the context's table."""
        t, r, codes, _, n = self._pair_inputs(text1, recs1, text2, recs2, codes)
        self._chk(self.lib.qd_dev_qstats(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n, _ptr(codes)))

    def clip_set(self, front_clip_r1=0, front_clip_r2=0, tail_clip_r1=0, tail_clip_r2=0, window_size=0, window_quality=0,
                 poly_g_min_length=0, min_length=0):
        """End clipping, window and poly-G trimming of the insert reads in the device pipeline, in front of trim_set's stage
        (qd_clip_set; conf.CLIP_HELP has the rules).  Every rule off (the defaults) turns the stage off and frees the counters; a
        value out of range is QD_ERR_INVALID and changes nothing."""
        P = qd_clip_params()
        P.front_clip[0], P.front_clip[1], P.tail_clip[0], P.tail_clip[1] = int(front_clip_r1), int(front_clip_r2), int(tail_clip_r1), int(tail_clip_r2)
        P.window_size, P.window_quality, P.poly_g_min_length, P.min_length = int(window_size), int(window_quality), int(poly_g_min_length), int(min_length)
        self._chk(self.lib.qd_clip_set(self._h, C.byref(P)))

    def clip_get(self):
        """The parameters in force, as clip_set's keywords (the stage off: all zero)."""
        P = qd_clip_params()
        self._chk(self.lib.qd_clip_get(self._h, C.byref(P)))
        return dict(front_clip_r1=P.front_clip[0], front_clip_r2=P.front_clip[1], tail_clip_r1=P.tail_clip[0], tail_clip_r2=P.tail_clip[1],
                    window_size=P.window_size, window_quality=P.window_quality, poly_g_min_length=P.poly_g_min_length, min_length=P.min_length)

    def clip_active(self):
        """whether the stage is on: what the pipeline asks before every batch (qd_clip_active, an internal entry of the library)"""
        f = self.lib.qd_clip_active
        f.restype, f.argtypes = C.c_int, [_P]
        return bool(f(self._h))

    def clip_read(self):
        """numpy uint64[2, 12]: [R1, R2][CLIP_COUNTERS]"""
        return self._table_read(self.lib.qd_clip_read, (2, len(CLIP_COUNTERS)))

    def clip_add(self, table):
        """Another context's counters (clip_read's layout) join this context's (qd_clip_add)."""
        self._table_add(self.lib.qd_clip_add, table)

    def dev_clip(self, text1, recs1, text2, recs2):
        """The clip stage over host buffers (qd_dev_clip): texts as bytes or uint8 arrays, recs uint32[n, 6] in dev_fastq_scan's
        layout; -> the two tables as the stage leaves them (seq, qual and seq_len change); adds to the context's counters."""
        return self._dev_recs(self.lib.qd_dev_clip, text1, recs1, text2, recs2)

    def trim_set(self, adapter_r1="", adapter_r2="", quality_cutoff=0, min_overlap=3, max_mismatch_pct=10, min_length=0):
        """3' trimming of the insert reads in the device pipeline (qd_trim_set; conf.TRIM_HELP has the rules).  Neither an adapter
        nor a cutoff turns it off and frees the counters; a value out of range is QD_ERR_INVALID and changes nothing."""
        P = qd_trim_params()
        for name, a in (("adapter_r1", adapter_r1), ("adapter_r2", adapter_r2)):
            a = a.encode() if isinstance(a, str) else bytes(a)
            if len(a) > 64:
                raise QuadeHipError(QD_ERR_INVALID, "qd_trim_set: an adapter has 1 to 64 letters")
            getattr(P, name)[:len(a)] = list(a)
            setattr(P, name + "_len", len(a))
        P.quality_cutoff, P.min_overlap, P.max_mismatch_pct, P.min_length = int(quality_cutoff), int(min_overlap), int(max_mismatch_pct), int(min_length)
        self._chk(self.lib.qd_trim_set(self._h, C.byref(P)))

    def trim_get(self):
        """The parameters in force, as trim_set's keywords (adapters upper case; trimming off: no adapters, all zero)."""
        P = qd_trim_params()
        self._chk(self.lib.qd_trim_get(self._h, C.byref(P)))
        return dict(adapter_r1=bytes(P.adapter_r1[:P.adapter_r1_len]).decode(), adapter_r2=bytes(P.adapter_r2[:P.adapter_r2_len]).decode(),
                    quality_cutoff=P.quality_cutoff, min_overlap=P.min_overlap, max_mismatch_pct=P.max_mismatch_pct, min_length=P.min_length)

    def trim_read(self):
        """numpy uint64[2, 8]: [R1, R2][TRIM_COUNTERS]"""
        return self._table_read(self.lib.qd_trim_read, (2, len(TRIM_COUNTERS)))

    def trim_add(self, table):
        """Another context's counters (trim_read's layout) join this context's (qd_trim_add)."""
        self._table_add(self.lib.qd_trim_add, table)

    def dev_trim(self, text1, recs1, text2, recs2):
        """The trimming stage over host buffers (qd_dev_trim): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout; -> the two tables with the lengths the reads keep; adds to the context's counters."""
        return self._dev_recs(self.lib.qd_dev_trim, text1, recs1, text2, recs2)

    def pairtrim_set(self, min_overlap=30, max_mismatches=5, max_mismatch_pct=20, min_length=0, on=True):
        """Paired-end overlap trimming of the insert reads in the device pipeline (qd_pairtrim_set; conf.PAIR_HELP has the
        rules).  on=False turns it off and frees the table; a value out of range is QD_ERR_INVALID and changes nothing."""
        if not on:
            self._chk(self.lib.qd_pairtrim_set(self._h, None))
            return
        P = qd_pairtrim_params(int(min_overlap), int(max_mismatches), int(max_mismatch_pct), int(min_length))
        self._chk(self.lib.qd_pairtrim_set(self._h, C.byref(P)))

    def pairtrim_get(self):
        """The parameters in force, as pairtrim_set's keywords (the stage off: all zero)."""
        P = qd_pairtrim_params()
        self._chk(self.lib.qd_pairtrim_get(self._h, C.byref(P)))
        return dict(min_overlap=P.min_overlap, max_mismatches=P.max_mismatches, max_mismatch_pct=P.max_mismatch_pct, min_length=P.min_length)

    def pairtrim_read(self):
        """numpy uint64[1040]: [R1, R2][PAIRTRIM_COUNTERS], PAIRTRIM_PAIR_COUNTERS, the insert size bins (split_pairtrim)"""
        return self._table_read(self.lib.qd_pairtrim_read, PAIRTRIM_VALUES)

    def pairtrim_add(self, table):
        """Another context's table (pairtrim_read's layout) joins this context's (qd_pairtrim_add)."""
        self._table_add(self.lib.qd_pairtrim_add, table)

    def dev_pairtrim(self, text1, recs1, text2, recs2):
        """The overlap trimming stage over host buffers (qd_dev_pairtrim): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout; -> the two tables with the lengths the reads keep; adds to the context's table."""
        return self._dev_recs(self.lib.qd_dev_pairtrim, text1, recs1, text2, recs2)

    def paircorrect_set(self, good_quality=30, bad_quality=14, on=True):
        """Overlap base correction of the read pairs in the device pipeline, directly behind pairtrim_set's stage
        (qd_paircorrect_set; conf.CORRECT_HELP has the rule).  on=False turns it off and frees the table; a value out of range is
        QD_ERR_INVALID and changes nothing."""
        if not on:
            self._chk(self.lib.qd_paircorrect_set(self._h, None))
            return
        P = qd_paircorrect_params(int(good_quality), int(bad_quality))
        self._chk(self.lib.qd_paircorrect_set(self._h, C.byref(P)))

    def paircorrect_get(self):
        """The parameters in force, as paircorrect_set's keywords (the stage off: all zero)."""
        P = qd_paircorrect_params()
        self._chk(self.lib.qd_paircorrect_get(self._h, C.byref(P)))
        return dict(good_quality=P.good_quality, bad_quality=P.bad_quality)

    def paircorrect_read(self):
        """numpy uint64[10]: PAIRCORRECT_COUNTERS"""
        return self._table_read(self.lib.qd_paircorrect_read, PAIRCORRECT_VALUES)

    def paircorrect_add(self, table):
        """Another context's table (paircorrect_read's layout) joins this context's (qd_paircorrect_add)."""
        self._table_add(self.lib.qd_paircorrect_add, table)

    def dev_paircorrect(self, text1, recs1, text2, recs2, inserts=None):
        """The overlap base correction over host buffers (qd_dev_paircorrect): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout; inserts: a pair's insert length I each (0 = none), used as given, or None: the overlap trimming
        kernel runs first with the context's parameters and supplies them; -> the two texts as the stage leaves them (uint8
        arrays); adds to the context's table."""
        t, r, _, _, n = self._pair_inputs(text1, recs1, text2, recs2)
        if inserts is not None:
            inserts = np.ascontiguousarray(inserts, dtype=np.uint64)
            if inserts.shape != (n,):
                raise ValueError("inserts must have one value per pair")
        out = [np.zeros_like(x) for x in t]
        self._chk(self.lib.qd_dev_paircorrect(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n,
                                              None if inserts is None else _ptr(inserts), _ptr(out[0]), _ptr(out[1])))
        return out[0], out[1]

    def posttrim_set(self, tail_n=0, poly_x_min_length=0, max_length_r1=0, max_length_r2=0, min_length=0):
        """Trailing-N, poly-X and max_length trimming of the insert reads in the device pipeline, behind pairtrim_set's stage and in
        front of filter_set's (qd_posttrim_set; conf.POSTTRIM_HELP has the rules).  Every rule off (the defaults) turns the stage
        off and frees the counters; a value out of range is QD_ERR_INVALID and changes nothing."""
        P = qd_posttrim_params()
        P.tail_n, P.poly_x_min_length, P.min_length = int(tail_n), int(poly_x_min_length), int(min_length)
        P.max_length[0], P.max_length[1] = int(max_length_r1), int(max_length_r2)
        self._chk(self.lib.qd_posttrim_set(self._h, C.byref(P)))

    def posttrim_get(self):
        """The parameters in force, as posttrim_set's keywords (the stage off: all zero)."""
        P = qd_posttrim_params()
        self._chk(self.lib.qd_posttrim_get(self._h, C.byref(P)))
        return dict(tail_n=P.tail_n, poly_x_min_length=P.poly_x_min_length, max_length_r1=P.max_length[0], max_length_r2=P.max_length[1],
                    min_length=P.min_length)

    def posttrim_active(self):
        """whether the stage is on: what the pipeline asks before every batch (qd_posttrim_active, an internal entry of the library)"""
        f = self.lib.qd_posttrim_active
        f.restype, f.argtypes = C.c_int, [_P]
        return bool(f(self._h))

    def posttrim_read(self):
        """numpy uint64[2, 16]: [R1, R2][POSTTRIM_COUNTERS]"""
        return self._table_read(self.lib.qd_posttrim_read, (2, len(POSTTRIM_COUNTERS)))

    def posttrim_add(self, table):
        """Another context's counters (posttrim_read's layout) join this context's (qd_posttrim_add)."""
        self._table_add(self.lib.qd_posttrim_add, table)

    def dev_posttrim(self, text1, recs1, text2, recs2):
        """The post-trimming stage over host buffers (qd_dev_posttrim): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout; -> the two tables with the lengths the reads keep; adds to the context's counters."""
        return self._dev_recs(self.lib.qd_dev_posttrim, text1, recs1, text2, recs2)

    def filter_set(self, min_length=None, max_n=None, max_unqualified_pct=None, qualified_quality=15, min_mean_quality=None,
                   min_complexity_pct=None, on=True):
        """Read filtering in the device pipeline (qd_filter_set; conf.FILTER_HELP has the rules).  None = the rule is off;
        on=False, or every rule None, turns the stage off and frees the table; a value out of range is QD_ERR_INVALID and
        changes nothing.  Needs the plan and the barcodes."""
        if not on:
            self._chk(self.lib.qd_filter_set(self._h, None))
            return
        given = (min_length, max_n, max_unqualified_pct, qualified_quality, min_mean_quality, min_complexity_pct)
        # (a negative number is no way to say "off" here: -2 so that the library refuses it, as it refuses every bad value)
        P = qd_filter_params(*[-1 if x is None else (int(x) if int(x) >= 0 else -2) for x in given])
        self._chk(self.lib.qd_filter_set(self._h, C.byref(P)))

    def filter_get(self):
        """The parameters in force, as filter_set's keywords (a rule that is off: None)."""
        P = qd_filter_params()
        self._chk(self.lib.qd_filter_get(self._h, C.byref(P)))
        return {k: (None if getattr(P, k) < 0 else int(getattr(P, k))) for k in FILTER_KEYS}

    def filter_read(self):
        """numpy uint64[2S+1, 8]: [destination (code; Undetermined last)][FILTER_COUNTERS]"""
        return self._table_read(self.lib.qd_filter_read, (2 * self.n_samples + 1, len(FILTER_COUNTERS)))

    def filter_add(self, table):
        """Another context's table (filter_read's layout) joins this context's (qd_filter_add)."""
        self._table_add(self.lib.qd_filter_add, table)

    def filter_kind(self):
        """FILTER_KIND_LDS or FILTER_KIND_GLOBAL: the accumulation the kernel takes for this context's sample count"""
        kind = self.lib.qd_filter_kind(self._h)
        if kind < 0:
            self._chk(kind)
        return kind

    def dev_filter(self, text1, recs1, text2, recs2, codes):
        """The filter stage over host buffers (qd_dev_filter): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout, codes uint16[n]; -> uint8[n], 0 = kept or the rule that dropped the pair; adds to the
        context's table."""
        t, r, codes, _, n = self._pair_inputs(text1, recs1, text2, recs2, codes)
        out = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.qd_dev_filter(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n, _ptr(codes), _ptr(out)))
        return out

    def screen_set(self, kmer=31, min_hits=1, action="report", kmers=None, reference=None, on=True):
        """The k-mer screen against a reference in the device pipeline, behind filter_set's stage (qd_screen_set; conf.SCREEN_HELP
        has the definition).  kmers: the reference set's distinct canonical words, uint64, ascending (screen.reference_kmers makes
        them); action "report" or "drop" (or 0, 1); reference: what the report says about the FASTA, not looked at here.
        on=False, or no k-mers, turns the stage off and frees the hash table and the counters; a bad value is QD_ERR_INVALID and
        changes nothing.  Needs the plan and the barcodes."""
        if not on or kmers is None or len(kmers) == 0:
            self._chk(self.lib.qd_screen_set(self._h, None, None, 0))
            return
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1)
        P = qd_screen_params(int(kmer), int(min_hits), SCREEN_ACTIONS.index(action) if action in SCREEN_ACTIONS else int(action))
        self._chk(self.lib.qd_screen_set(self._h, C.byref(P), _ptr(kmers), kmers.size))

    def screen_get(self):
        """The parameters in force, as screen_set's keywords with n_kmers in place of the words; None when the stage is off."""
        P, n = qd_screen_params(), C.c_int64(0)
        self._chk(self.lib.qd_screen_get(self._h, C.byref(P), C.byref(n)))
        return dict(kmer=int(P.kmer), min_hits=int(P.min_hits), action=SCREEN_ACTIONS[P.action], n_kmers=int(n.value)) if n.value else None

    def screen_active(self):
        """whether the stage is on: what the pipeline asks before every batch (qd_screen_active, an internal entry of the library)"""
        f = self.lib.qd_screen_active
        f.restype, f.argtypes = C.c_int, [_P]
        return bool(f(self._h))

    def screen_kind(self):
        """Where the kernel keeps the reference's hash table: "lds" or "global"."""
        kind = self.lib.qd_screen_kind(self._h)
        if kind < 0:
            self._chk(kind)
        return {1: "lds", 2: "global"}[kind]

    def screen_first_slot(self, word, n_kmers):
        """the slot at which the probe for a canonical word starts in the table built for n_kmers words (qd_screen_first_slot)"""
        slot = self.lib.qd_screen_first_slot(int(word), int(n_kmers))
        if slot < 0:
            self._chk(int(slot))
        return int(slot)

    def screen_read(self):
        """numpy uint64[2S+1, 8]: [destination (code; Undetermined last)][SCREEN_COUNTERS]"""
        return self._table_read(self.lib.qd_screen_read, (2 * self.n_samples + 1, len(SCREEN_COUNTERS)))

    def screen_add(self, table):
        """Another context's table (screen_read's layout) joins this context's (qd_screen_add)."""
        self._table_add(self.lib.qd_screen_add, table)

    def dev_screen(self, text1, recs1, text2, recs2, codes, drop=None):
        """The screen stage over host buffers (qd_dev_screen): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout, codes uint16[n], drop None or uint8[n] (non-zero = the pair is skipped); -> (hits uint32[n, 2],
        flags uint8[n]: the drop byte of a skipped pair, 0x80 for a matched pair under action drop, else 0); adds to the context's
        table."""
        t, r, codes, drop, n = self._pair_inputs(text1, recs1, text2, recs2, codes, drop)
        hits, flags = np.zeros((n, 2), dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.qd_dev_screen(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n, _ptr(codes),
                                         _ptr(drop) if drop is not None else None, _ptr(hits), _ptr(flags)))
        return hits, flags

    def cstats_enable(self, on=True):
        """Per-cycle quality and base content and the per-read distributions (qd_cstats_enable): every pair the device pipeline
        routes adds its two insert reads to a device table.  Independent of plan and barcodes; reset_counts zeroes it."""
        self._chk(self.lib.qd_cstats_enable(self._h, int(bool(on))))

    def cstats_read(self):
        """dict of uint64 views into one flat table: cycle[3, 2, 1024, 8], len[3, 2, 1025], meanq[3, 2, 94], gc[3, 2, 101] --
        [CSTATS_GROUPS][R1, R2][...] (cstats_flat gives the flat table back)"""
        return cstats_views(self._table_read(self.lib.qd_cstats_read, CSTATS_VALUES))

    def cstats_add(self, table):
        """Another context's table (cstats_read's dict or flat) joins this context's (qd_cstats_add)."""
        self._table_add(self.lib.qd_cstats_add, cstats_flat(table) if isinstance(table, dict) else np.reshape(table, -1))

    def dev_cstats(self, text1, recs1, text2, recs2, codes, drop=None):
        """The per-cycle stage over host buffers (qd_dev_cstats): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout, codes uint16[n], drop None or uint8[n] (non-zero = the pair is skipped); adds to the context's
        table."""
        t, r, codes, drop, n = self._pair_inputs(text1, recs1, text2, recs2, codes, drop)
        self._chk(self.lib.qd_dev_cstats(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n, _ptr(codes),
                                         _ptr(drop) if drop is not None else None))

    def adapters_set(self, probes=(), aliases=None, left_off=None, on=True):
        """The adapter content of the raw insert reads in the device pipeline, in front of every trimming stage (qd_adapters_set;
        conf.ADAPTER_HELP has the definition).  probes: up to 16 (name, probe) or plain probes of 12 bases of ACGT, no two equal;
        their order is the table's slot order.  aliases and left_off are the report's (conf.adapter_params).  No probe or
        on=False turns the stage off and frees the table; a bad probe is QD_ERR_INVALID and changes nothing.  Needs the plan
        and the barcodes, which turn it off; reset_counts zeroes the table."""
        seqs = [p if isinstance(p, (str, bytes)) else p[1] for p in probes] if on else []
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        if not seqs:
            self._chk(self.lib.qd_adapters_set(self._h, None, 0))
            return
        if any(len(s) != ADAPTER_K for s in seqs):
            raise ValueError("a probe is %d bases" % ADAPTER_K)
        flat = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        self._chk(self.lib.qd_adapters_set(self._h, _ptr(flat), len(seqs)))

    def adapters_get(self):
        """the probes in force, in slot order, as strings; [] when the stage is off (qd_adapters_get)"""
        buf, n = np.zeros(ADAPTER_PROBES * ADAPTER_K, dtype=np.uint8), C.c_int32(0)
        self._chk(self.lib.qd_adapters_get(self._h, _ptr(buf), C.byref(n)))
        return [buf[a * ADAPTER_K:(a + 1) * ADAPTER_K].tobytes().decode() for a in range(n.value)]

    def adapters_active(self):
        """whether the stage is on (qd_adapters_active, an internal entry of the library)"""
        f = self.lib.qd_adapters_active
        f.restype, f.argtypes = C.c_int, [_P]
        return bool(f(self._h))

    def adapters_read(self):
        """dict of uint64 views into one flat table: hist[2, 17, 1025] -- [R1, R2][16 probe slots, any][min(first, 1024)] -- and
        dest[2S+1, 2, 18] -- [destination (code; Undetermined last)][R1, R2][reads, 16 probe slots, any] (adapters_flat gives the
        flat table back)"""
        return adapters_views(self._table_read(self.lib.qd_adapters_read, adapters_values(self.n_samples)))

    def adapters_add(self, table):
        """Another context's table (adapters_read's dict or flat) joins this context's (qd_adapters_add)."""
        self._table_add(self.lib.qd_adapters_add, adapters_flat(table) if isinstance(table, dict) else np.reshape(table, -1))

    def dev_adapters(self, text1, recs1, text2, recs2, codes):
        """The adapter content stage over host buffers (qd_dev_adapters): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout, codes uint16[n]; adds to the context's table."""
        t, r, codes, _, n = self._pair_inputs(text1, recs1, text2, recs2, codes)
        self._chk(self.lib.qd_dev_adapters(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n, _ptr(codes)))

    def dup_set(self, bases=32, sample=16, slots=1 << 24, on=True):
        """The duplication tally in the device pipeline (qd_dup_set; conf.DUPLICATION_HELP has the definition): `bases` 8 .. 32
        of either read make a pair's key, keys are sampled one in `sample` (a power of two, 1 .. 1024) and counted in a table of
        `slots` entries (a power of two, 2^10 .. 2^28).  on=False turns the stage off and frees both tables; a value out of range
        is QD_ERR_INVALID and changes nothing.  Needs the plan and the barcodes."""
        if not on:
            self._chk(self.lib.qd_dup_set(self._h, None))
            return
        P = qd_dup_params(int(bases), int(sample), int(slots))
        self._chk(self.lib.qd_dup_set(self._h, C.byref(P)))

    def dup_get(self):
        """The parameters in force, as dup_set's keywords; None when the stage is off."""
        P = qd_dup_params()
        self._chk(self.lib.qd_dup_get(self._h, C.byref(P)))
        return dict(bases=int(P.bases), sample=int(P.sample), slots=int(P.slots)) if P.slots else None

    def dup_stats(self):
        """numpy uint64[2S+1, 5]: [destination (code; Undetermined last)][DUP_COUNTERS]"""
        return self._table_read(self.lib.qd_dup_stats, (2 * self.n_samples + 1, len(DUP_COUNTERS)))

    def dup_read(self):
        """The key table's entries in no particular order: (keys uint64[n, 3] = (w1, w2, d), counts uint64[n])."""
        return self._tally_read(self.lib.qd_dup_read, 3, np.uint64)

    def dev_dup(self, text1, recs1, text2, recs2, codes, drop=None):
        """The duplication tally over host buffers (qd_dev_dup): texts as bytes or uint8 arrays, recs uint32[n, 6] in
        dev_fastq_scan's layout, codes uint16[n], drop None or uint8[n] (non-zero = the pair is skipped); adds to the context's
        two tables."""
        t, r, codes, drop, n = self._pair_inputs(text1, recs1, text2, recs2, codes, drop)
        self._chk(self.lib.qd_dev_dup(self._h, _ptr(t[0]), t[0].size, _ptr(r[0]), _ptr(t[1]), t[1].size, _ptr(r[1]), n, _ptr(codes),
                                      _ptr(drop) if drop is not None else None))

    def set_option(self, name, value):
        self._chk(self.lib.qd_set_option(self._h, name.encode(), int(value)))

    def kernel_kind(self, has_len=False):
        return {1: "fast", 2: "generic"}[self.lib.qd_kernel_kind(self._h, int(has_len))]

    # -- device-resident batches (pointers are device addresses, e.g. torch tensor .data_ptr())
    @staticmethod
    def _rows(seq, qual, lens):
        rows = qd_rows()
        for k in range(2):
            rows.seq[k] = seq[k] if k < len(seq) else None
            rows.qual[k] = qual[k] if k < len(qual) else None
            rows.len[k] = lens[k] if k < len(lens) else None
        return rows

    def demux_device(self, n_pairs, seq, qual, codes, mol=None, lens=(None, None), stream=None):
        """stream: a hipStream_t handle (0 = HIP's null stream); None = the context's own stream."""
        rows = self._rows(seq, qual, lens)
        st = STREAM_CONTEXT if stream is None else stream
        self._chk(self.lib.qd_demux_device(self._h, int(n_pairs), C.byref(rows), codes, mol, st))

    def demux_device_ragged(self, n_pairs, seq, qual, codes, mol, lens, n_short, short_idx, stream=None):
        """short_idx: device address of n_short unique uint32 pair indices (the short reads)."""
        rows = self._rows(seq, qual, lens)
        st = STREAM_CONTEXT if stream is None else stream
        self._chk(self.lib.qd_demux_device_ragged(self._h, int(n_pairs), C.byref(rows), codes, mol, int(n_short),
                                                  short_idx, st))

    def synchronize(self):
        self._chk(self.lib.qd_synchronize(self._h))

    def counts(self):
        out = np.zeros(2 * self.n_samples + 4, dtype=np.uint64)
        self._chk(self.lib.qd_get_counts(self._h, _ptr(out), out.size))
        return out

    def add_counts(self, counts):
        """Another context's counter vector (numpy uint64[2S+4]) joins this context's totals (qd_add_counts)."""
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        self._chk(self.lib.qd_add_counts(self._h, _ptr(counts), counts.size))

    def reset_counts(self):
        self._chk(self.lib.qd_reset_counts(self._h))

    # -- pinned slots
    def slots_create(self, n_slots, max_pairs):
        self._chk(self.lib.qd_slots_create(self._h, int(n_slots), int(max_pairs)))
        self._slot_views = {}
        self.n_slots, self.slot_pairs = int(n_slots), int(max_pairs)

    def slots_destroy(self):
        self._slot_views = {}
        self._chk(self.lib.qd_slots_destroy(self._h))

    def slot(self, i):
        """numpy views over the pinned host buffers of slot i."""
        if i in self._slot_views:
            return self._slot_views[i]
        sb = qd_slot_buffers()
        self._chk(self.lib.qd_slot_get(self._h, i, C.byref(sb)))
        L, n = self.layout, sb.max_pairs

        def view(addr, shape, dtype=np.uint8):
            if not addr:
                return None
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            buf = (C.c_uint8 * nbytes).from_address(addr)
            return np.frombuffer(buf, dtype=dtype).reshape(shape)

        v = {"seq": [], "qual": [], "len": [], "max_pairs": n}
        for k in range(L.n_streams):
            v["seq"].append(view(sb.seq[k], (n, L.seq_stride[k])))
            v["qual"].append(view(sb.qual[k], (n, L.qual_stride[k])))
            v["len"].append(view(sb.len[k], (n,)))
        v["codes"] = view(sb.codes, (n,), np.uint16)
        v["mol"] = view(sb.mol, (n, L.mol_width)) if L.mol_width else None
        v["short"] = [view(sb.short_idx[k], (sb.short_cap,), np.uint32) for k in range(L.n_streams)]
        self._slot_views[i] = v
        return v

    def submit(self, slot, n_pairs, has_len=False):
        self._chk(self.lib.qd_submit(self._h, int(slot), int(n_pairs), int(bool(has_len))))

    def submit_ragged(self, slot, n_pairs, n_short):
        """n_short: per stream, how many short reads the packer listed in the slot's `short` arrays."""
        ns = (C.c_int64 * 2)(*(list(n_short) + [0, 0])[:2])
        self._chk(self.lib.qd_submit_ragged(self._h, int(slot), int(n_pairs), ns))

    def wait(self, slot):
        self._chk(self.lib.qd_wait(self._h, int(slot)))


# ---- multi-GPU count reduce (RCCL through the C ABI) --------------------------------------------------------
UNIQUE_ID_BYTES = 128


def comm_unique_id():
    """128 opaque bytes made by rank 0 (ncclGetUniqueId) that every rank of a communicator needs."""
    lib = load_library()
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    r = lib.qd_comm_unique_id(buf)
    if r != QD_OK:
        raise QuadeHipError(r, lib.qd_comm_last_error().decode())
    return bytes(buf)


class Comm(object):
    """The contexts whose counters are summed by one RCCL all-reduce (include/quade_hip.h, qd_comm)."""

    def __init__(self, handle, engines):
        self.lib = load_library()
        self._h = handle
        self.engines = engines

    @classmethod
    def local(cls, engines):
        """One process, one context per local device (ncclCommInitAll)."""
        lib = load_library()
        arr = (_P * len(engines))(*[e._h for e in engines])
        h = C.c_void_p()
        r = lib.qd_comm_create_local(arr, len(engines), C.byref(h))
        if r != QD_OK:
            raise QuadeHipError(r, lib.qd_comm_last_error().decode())
        return cls(h, list(engines))

    @classmethod
    def rank(cls, engine, world, rank, unique_id):
        """One process per device: this process's rank of a `world`-rank communicator (ncclCommInitRank)."""
        lib = load_library()
        assert len(unique_id) == UNIQUE_ID_BYTES
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        r = lib.qd_comm_create_rank(engine._h, int(world), int(rank), buf, C.byref(h))
        if r != QD_OK:
            raise QuadeHipError(r, lib.qd_comm_last_error().decode())
        return cls(h, [engine])

    @property
    def world(self):
        return self.lib.qd_comm_world(self._h)

    def reduce_counts(self):
        """Sum of every member context's counters (all ranks): numpy uint64[2S+4]."""
        out = np.zeros(2 * self.engines[0].n_samples + 4, dtype=np.uint64)
        r = self.lib.qd_reduce_counts(self._h, _ptr(out), out.size)
        if r != QD_OK:
            raise QuadeHipError(r, self.lib.qd_comm_last_error().decode())
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.lib.qd_comm_destroy(self._h)
            self._h = None


class Inflater(object):
    """BGZF blocks -> text on the device (qd_inflater_*): one lane per block, CRC32 of every block checked."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        h = _P()
        r = self.lib.qd_inflater_create(int(device_id), C.byref(h))
        if r != QD_OK:
            raise QuadeHipError(r, self.lib.qd_inflater_last_error(None).decode())
        self._h = h

    def set_form(self, form):
        """1: one wave per block; 2: speculative spans; 3: one lane decodes a block's symbols once, a workgroup resolves the tokens."""
        r = self.lib.qd_inflater_set_form(self._h, int(form))
        if r != QD_OK:
            raise QuadeHipError(r, "no such inflater form: %r" % (form,))

    def run(self, comp, out_len):
        """comp: bytes of whole BGZF blocks; out_len: the sum of their ISIZE fields.  Returns the text (bytes)."""
        src = np.frombuffer(comp, dtype=np.uint8)
        out = np.empty(max(int(out_len), 1), dtype=np.uint8)
        bad = C.c_int32(-1)
        r = self.lib.qd_inflater_run(self._h, _ptr(src), len(src), _ptr(out), int(out_len), C.byref(bad))
        if r != QD_OK:
            e = QuadeHipError(r, self.lib.qd_inflater_last_error(self._h).decode())
            e.bad_block = bad.value
            raise e
        return out[:out_len].tobytes()

    def close(self):
        if getattr(self, "_h", None):
            self.lib.qd_inflater_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def dev_gunzip(gz, out_cap, device_id=0, step_bytes=64 << 20, stretch_bytes=0, unit_text=0):
    """A whole gzip file image (bytes: one or more members) -> its text, inflated by the device's gzip kernels (qd_dev_gunzip).
    Returns (text bytes, stats dict).  QuadeHipError(QD_ERR_FORMAT) for input the device does not decode (not gzip, damaged, ...)."""
    lib = load_library()
    src = np.frombuffer(gz, dtype=np.uint8) if len(gz) else np.zeros(1, np.uint8)
    out = np.empty(max(int(out_cap), 1), dtype=np.uint8)
    n = C.c_int64(0)
    st = (C.c_int64 * 8)()
    r = lib.qd_dev_gunzip(int(device_id), _ptr(src), len(gz), _ptr(out), int(out_cap), C.byref(n), int(step_bytes), int(stretch_bytes), int(unit_text), st)
    stats = dict(zip(("members", "steps", "stretches", "units", "chain_retries", "partial_last", "plain_probes"), [int(x) for x in st]))
    if r != QD_OK:
        e = QuadeHipError(r, "qd_dev_gunzip: the device did not inflate the stream")
        e.stats = stats
        raise e
    return out[:n.value].tobytes(), stats


DEV_GUARD_BYTE = 0xEE  # QD_DEV_GUARD_BYTE


def _text_array(t):
    return (np.frombuffer(t, dtype=np.uint8) if len(t) else np.zeros(1, np.uint8)) if not isinstance(t, np.ndarray) else t


def dev_pack_rows(layout: qd_layout, texts, recs, short_cap, short_room=None, device_id=0):
    """The index-row stage over host buffers (qd_dev_pack_rows): texts = one or two index texts (bytes or uint8 arrays), recs their
    uint32[n, 6] tables.  Returns (seq_rows, qual_rows, len_rows: a list per stream; short_idx uint32[short_room], n_short)."""
    lib = load_library()
    ns = layout.n_streams
    t = [_text_array(x) for x in texts[:ns]]
    r = [np.ascontiguousarray(x, dtype=np.uint32) for x in recs[:ns]]
    n = r[0].shape[0]
    assert all(x.shape == (n, 6) for x in r)
    seq = [np.empty((n, layout.seq_stride[k]), dtype=np.uint8) for k in range(ns)]
    qual = [np.empty((n, layout.qual_stride[k]), dtype=np.uint8) for k in range(ns)]
    lens = [np.empty(n, dtype=np.uint8) for k in range(ns)]
    room = int(short_cap) if short_room is None else int(short_room)
    short_idx = np.zeros(max(room, 1), dtype=np.uint32)
    n_short = C.c_uint32(0)
    two = lambda a: (_P * 2)(*[_ptr(a[k]) if k < ns else None for k in range(2)])  # noqa: E731
    rc = lib.qd_dev_pack_rows(int(device_id), C.byref(layout), two(t), (C.c_int64 * 2)(*[len(texts[k]) if k < ns else 0 for k in range(2)]), two(r), n,
                              int(short_cap), two(seq), two(qual), two(lens), _ptr(short_idx), room, C.byref(n_short))
    if rc != QD_OK:
        raise QuadeHipError(rc, "qd_dev_pack_rows: " + lib.qd_strerror(rc).decode())
    return seq, qual, lens, short_idx[:room], int(n_short.value)


ROUTE_TABLES = ("dest", "len1", "len2", "perm", "sdest", "g1", "g2", "first", "g1_first", "g2_first", "base1", "base2")


def dev_route_format(plan: qd_plan, n_samples, flags, texts, recs, codes, drop=None, shift=0, out_cap=0, device_id=0):
    """The routing and format chain of a batch over host buffers (qd_dev_route_format): flags = (write_pass, write_fail,
    write_undetermined); texts / recs = R1, R2, I1[, I2] (bytes or uint8 arrays; uint32[n, 6] tables).  Returns a dict of
    ROUTE_TABLES plus "out" (uint8[out_cap], DEV_GUARD_BYTE where no record lies) and "used".  QuadeHipError(QD_ERR_INVALID) with
    .used set when out_cap is too small."""
    lib = load_library()
    ns = 4 if plan.dual else 3
    t = [_text_array(x) for x in texts[:ns]]
    r = [np.ascontiguousarray(x, dtype=np.uint32) for x in recs[:ns]]
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    n, nd = codes.size, 2 * int(n_samples) + 1
    assert all(x.shape == (n, 6) for x in r)
    if drop is not None:
        drop = np.ascontiguousarray(drop, dtype=np.uint8)
        assert drop.shape == (n,)
    four = lambda a: (_P * 4)(*[_ptr(a[k]) if k < ns else None for k in range(4)])  # noqa: E731
    res = {"dest": np.zeros(n, np.uint16), "len1": np.zeros(n, np.uint32), "len2": np.zeros(n, np.uint32), "perm": np.zeros(n, np.uint32),
           "sdest": np.zeros(n, np.uint16), "g1": np.zeros(n + 1, np.uint32), "g2": np.zeros(n + 1, np.uint32), "first": np.zeros(nd, np.uint32),
           "g1_first": np.zeros(nd, np.uint32), "g2_first": np.zeros(nd, np.uint32), "base1": np.zeros(nd, np.int64), "base2": np.zeros(nd, np.int64)}
    out = np.zeros(max(int(out_cap), 1), dtype=np.uint8)
    used = C.c_int64(-1)
    rc = lib.qd_dev_route_format(int(device_id), C.byref(plan), int(n_samples), int(flags[0]), int(flags[1]), int(flags[2]), four(t),
                                 (C.c_int64 * 4)(*[len(texts[k]) if k < ns else 0 for k in range(4)]), four(r), _ptr(codes), _ptr(drop), n, int(shift),
                                 *([_ptr(res[k]) for k in ROUTE_TABLES] + [_ptr(out), int(out_cap), C.byref(used)]))
    if rc != QD_OK:
        e = QuadeHipError(rc, "qd_dev_route_format: " + lib.qd_strerror(rc).decode())
        e.used = used.value
        raise e
    res["out"] = out[:int(out_cap)]
    res["used"] = used.value
    return res


def dev_pack_members(slots, stride, lens, packed_cap, device_id=0):
    """Members in slots of `stride` bytes -> (offsets uint64[n + 1], packed uint8[packed_cap]) by qd_dev_pack_members; the bytes
    behind offsets[n] are DEV_GUARD_BYTE."""
    lib = load_library()
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    slots = np.ascontiguousarray(slots, dtype=np.uint8)
    n = lens.size
    assert slots.size >= n * int(stride)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    packed = np.zeros(max(int(packed_cap), 1), dtype=np.uint8)
    rc = lib.qd_dev_pack_members(int(device_id), _ptr(slots) if n else None, int(stride), _ptr(lens) if n else None, n, _ptr(offsets), _ptr(packed),
                                 int(packed_cap))
    if rc != QD_OK:
        raise QuadeHipError(rc, "qd_dev_pack_members: " + lib.qd_strerror(rc).decode())
    return offsets, packed[:int(packed_cap)]


class Pipe(object):
    """The device-resident chunk pipeline of one context (include/quade_hip.h, qd_pipe_*): whole chunks of fastq(.gz)
    files in, routed fastq.gz members out, the text staying in HBM in between."""

    def __init__(self, engine, batch_pairs=None):
        self.lib = load_library()
        self.engine = engine
        h = _P()
        r = self.lib.qd_pipe_create(engine._h, C.byref(h))
        if r != QD_OK:
            raise QuadeHipError(r, self.lib.qd_pipe_last_error(None).decode())
        self._h = h
        if batch_pairs:
            self.set_option("batch_pairs", batch_pairs)

    def set_option(self, name, value):
        r = self.lib.qd_pipe_set_option(self._h, name.encode(), int(value))
        if r != QD_OK:
            raise QuadeHipError(r, self.lib.qd_pipe_last_error(self._h).decode())

    def index(self, path, world, rank, grains_per_rank=8):
        """This rank's grains of the BGZF file `path` for a chunk that `world` ranks share (qd_pipe_index): a list of dicts
        {file_offset, n_lines, kept[4], skip_bytes[4], incomplete[4]}, or None when the file cannot be shared this way."""
        arr = (qd_grain_info * grains_per_rank)()
        n = C.c_int32(0)
        r = self.lib.qd_pipe_index(self._h, str(path).encode(), int(world), int(rank), int(grains_per_rank), arr, grains_per_rank, C.byref(n))
        if r == QD_ERR_UNSUPPORTED:
            return None
        if r != QD_OK:
            msg = self.lib.qd_pipe_last_error(self._h).decode()
            if r == QD_ERR_FORMAT:
                raise IOError(msg)
            raise QuadeHipError(r, msg)
        return [{"file_offset": int(g.file_offset), "n_lines": int(g.n_lines), "kept": [int(x) for x in g.kept],
                 "skip_bytes": [int(x) for x in g.skip_bytes], "incomplete": [int(x) for x in g.incomplete]} for g in arr[:n.value]]

    def run(self, chunks):
        """chunks: list of (r1, r2, i1, i2 or None, sink handle, begin message or None, end message or None[, part]) where part
        (a chunk that several ranks share: dist.plan_parts) = {"start_offset": [4], "skip_bytes": [4], "skip_kept": [4], "max_pairs": n}.
        Returns the statistics as a dict."""
        def enc(x):
            return None if x is None else (x if isinstance(x, bytes) else str(x).encode())
        arr = (qd_pipe_chunk * max(len(chunks), 1))()
        for i, ch in enumerate(chunks):
            r1, r2, i1, i2, sink, m0, m1 = ch[:7]
            part = ch[7] if len(ch) > 7 and ch[7] else None
            z = (C.c_int64 * 4)(0, 0, 0, 0)
            arr[i] = qd_pipe_chunk(enc(r1), enc(r2), enc(i1), enc(i2), sink, enc(m0), enc(m1), z, z, z, 0)
            if part:
                for k in range(4):
                    arr[i].start_offset[k] = int(part["start_offset"][k])
                    arr[i].skip_bytes[k] = int(part["skip_bytes"][k])
                    arr[i].skip_kept[k] = int(part["skip_kept"][k])
                arr[i].max_pairs = int(part["max_pairs"])
        st = qd_pipe_stats()
        r = self.lib.qd_pipe_run(self._h, arr, len(chunks), C.byref(st))
        if r != QD_OK:
            msg = self.lib.qd_pipe_last_error(self._h).decode()
            if r == QD_ERR_FORMAT:
                raise IOError(msg)
            raise QuadeHipError(r, msg)
        return {n: getattr(st, n) for n, _ in qd_pipe_stats._fields_}

    def close(self):
        if getattr(self, "_h", None):
            self.lib.qd_pipe_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
