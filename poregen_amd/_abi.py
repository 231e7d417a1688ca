"""ctypes mirror of include/pgmove.h. Fails loudly if libpgmove.so has not been built."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpgmove.so")

PG_OK = 0
PG_ERR_NO_DEVICE = -1
PG_ERR_INVALID_ARG = -2
PG_ERR_INPUT = -3
PG_ERR_RNA_FLAG = -4
PG_ERR_HIP = -5
PG_ERR_STATE = -6
PG_ERR_UNSUPPORTED = -7
PG_LOC_HOST = 0
PG_LOC_DEVICE = 1
PG_FLAG_LAZY_STATS = 1
PG_FLAG_PROFILE = 2
PG_FLAG_OVERLAP = 4
PG_FLAG_DEBUG_NARROW = 8
PG_FLAG_SHORT_READS_OK = 16
PG_FLAG_SKIP_OUT_OF_RANGE = 32
PG_FLAG_STOP_WHEN_FULL = 64
PG_FLAG_DEFER_STATS = 128
PG_FLAG_DEBUG_SPLIT_WALK = 256
PG_FLAG_OVERLAP_TAIL = 512
PG_FLAG_ONE_STREAM = 1024
PG_MODEL_KEEP_FIRST = 1
PG_KFREQ_N_TO_T = 1
PG_DMODEL_PROFILE = 256
PG_DMODEL_EVENTS, PG_DMODEL_EVENTS_KEEP = 512, 1024
PG_EVENTS_OK, PG_EVENTS_HOST_FILE, PG_EVENTS_ONE_SAMPLE, PG_EVENTS_TOO_LONG, PG_EVENTS_TOO_WIDE, PG_EVENTS_BAD_VALUE, PG_EVENTS_DECLINED = 0, 1, 2, 4, 8, 16, 32
PG_EVENTS_COL_MEAN_MEDIAN, PG_EVENTS_COL_MEAN_SSTDEV, PG_EVENTS_COL_SD_MEDIAN, PG_EVENTS_COL_SD_SSTDEV = 0, 1, 2, 3
PG_MVOPS_RNA, PG_MVOPS_N_TO_T = 1, 2
PG_MVOPS_ST_ACCEPTED, PG_MVOPS_ST_NO_MOVE_IN_TABLE, PG_MVOPS_ST_NEGATIVE_TAIL, PG_MVOPS_ST_BASES_LEFT_OVER, PG_MVOPS_ST_BAD_STRIDE = 0, 1, 2, 3, 4
PG_MVOPS_ST_NO_CIGAR, PG_MVOPS_ST_CIGAR_LENGTH, PG_MVOPS_ST_CIGAR_OP = 5, 6, 7
PG_MODEL_TEXT_MEDIAN, PG_MODEL_TEXT_SSTDEV, PG_MODEL_TEXT_DWELL = 0, 1, 2
PG_FIT_ST_OK, PG_FIT_ST_OUT_OF_SIGNAL, PG_FIT_ST_TOO_LONG, PG_FIT_ST_FEW_EVENTS, PG_FIT_ST_FLAT, PG_FIT_ST_NEGATIVE_SCALE, PG_FIT_ST_SKIPPED = 0, 1, 2, 3, 4, 5, 16
PG_SIM_ST_OK, PG_SIM_ST_TOO_SHORT, PG_SIM_ST_BAD_BASE, PG_SIM_ST_NO_LEVEL = 0, 1, 2, 3
PG_POOL_NO_GROUP = 0xffffffff
PG_POOL_MAX_LABELINGS = 16
PG_POOL_GROUP_OK, PG_POOL_GROUP_EMPTY, PG_POOL_GROUP_REFUSED = 0, 1, 2

# every symbol include/pgmove.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "pg_default_params", "pg_last_error", "pg_version", "pg_build_slot_tables", "pg_create", "pg_destroy",
    "pg_reset", "pg_submit", "pg_count", "pg_collect", "pg_stats", "pg_collect_gathered", "pg_job_totals_device", "pg_sync", "pg_finish", "pg_finish_deferred", "pg_fetch_samples", "pg_text", "pg_fetch_text", "pg_text_device", "pg_all_slots_full",
    "pg_last_batch_device", "pg_kernel_stats", "pg_kernel_stats_reset", "pg_set_stream", "pg_model", "pg_model_device", "pg_model_format",
    "pg_job_create", "pg_job_destroy", "pg_job_last_error", "pg_job_submit", "pg_job_submit_shards", "pg_job_reset", "pg_job_sync", "pg_job_all_slots_full", "pg_job_finish",
    "pg_job_finish_deferred", "pg_job_fetch_samples", "pg_job_text", "pg_job_fetch_text",
    "pg_job_uses_rccl", "pg_job_model", "pg_job_kernel_stats", "pg_runtime_init", "pg_all_slots_full_settled", "pg_job_all_slots_full_settled", "pg_poll", "pg_job_poll",
    "pg_kfreq_create", "pg_kfreq_destroy", "pg_kfreq_last_error", "pg_kfreq_submit", "pg_kfreq_submit_reads", "pg_kfreq_submit_fasta", "pg_kfreq_reads_piece", "pg_kfreq_sync", "pg_kfreq_finish",
    "pg_fscore_create", "pg_fscore_destroy", "pg_fscore_last_error", "pg_fscore_submit", "pg_fscore_sync", "pg_fscore_finish",
    "pg_pamean_create", "pg_pamean_destroy", "pg_pamean_last_error", "pg_pamean_submit", "pg_pamean_sync", "pg_pamean_finish",
    "pg_pamean_submit_svb", "pg_pamean_svb_samples",
    "pg_sigdec_create", "pg_sigdec_destroy", "pg_sigdec_last_error", "pg_sigdec_counts", "pg_sigdec_decode",
    "pg_dmodel_create", "pg_dmodel_destroy", "pg_dmodel_last_error", "pg_dmodel_submit", "pg_dmodel_sync", "pg_dmodel_finish", "pg_dmodel_format",
    "pg_dmodel_finish_events", "pg_dmodel_format_events", "pg_dmodel_events_refusal", "pg_dmodel_events_values", "pg_dmodel_events_ms", "pg_model_events", "pg_events_status_text",
    "pg_pool_create", "pg_pool_destroy", "pg_pool_last_error", "pg_pool_submit", "pg_pool_sync", "pg_pool_finish", "pg_pool_format", "pg_pool_refusal",
    "pg_transform_model", "pg_transform_free",
    "pg_mvops_create", "pg_mvops_destroy", "pg_mvops_last_error", "pg_mvops_piece", "pg_mvops_set_stream", "pg_mvops_stream", "pg_mvops_expand", "pg_mvops_project",
    "pg_mvops_project_stranded", "pg_refseq_create", "pg_refseq_destroy", "pg_refseq_last_error", "pg_refseq_set_stream", "pg_refseq_add", "pg_refseq_slice",
    "pg_fit_create", "pg_fit_destroy", "pg_fit_last_error", "pg_fit_set_model", "pg_fit_submit", "pg_fit_finish", "pg_fit_set_stream", "pg_fit_pass_ms",
    "pg_fit_parse_model", "pg_fit_residuals", "pg_fit_calibrate", "pg_set_read_scaling",
    "pg_realign_create", "pg_realign_destroy", "pg_realign_last_error", "pg_realign_set_model", "pg_realign_set_stream", "pg_realign_submit", "pg_realign_kernel_ms",
    "pg_realign_walk", "pg_realign_walk_gapped", "pg_realign_set_phase",
    "pg_evalign_create", "pg_evalign_destroy", "pg_evalign_last_error", "pg_evalign_set_model", "pg_evalign_set_stream", "pg_evalign_submit", "pg_evalign_copy_text",
    "pg_evalign_kernel_ms", "pg_evalign_walk", "pg_evalign_walk_gapped", "pg_evalign_row_text",
    "pg_sim_create", "pg_sim_destroy", "pg_sim_last_error", "pg_sim_set_stream", "pg_sim_stream", "pg_sim_set_model", "pg_sim_generate", "pg_sim_kernel_ms", "pg_sim_walk",
    "pg_sim_parse_model", "pg_sim_parse_dwell",
    "pg_sigenc_create", "pg_sigenc_destroy", "pg_sigenc_last_error", "pg_sigenc_set_stream", "pg_sigenc_stream", "pg_sigenc_bound", "pg_sigenc_encode", "pg_sigenc_kernel_ms",
]
PG_JOB_EXCHANGE_AUTO, PG_JOB_EXCHANGE_HOST, PG_JOB_EXCHANGE_RCCL = 0, 1, 2


class PgParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("kmer_size", C.c_uint32), ("sig_move_offset", C.c_uint32),
        ("signal_print_margin", C.c_uint32), ("sample_limit", C.c_uint32), ("max_dur", C.c_uint32),
        ("min_dur", C.c_uint32), ("kmer_pick_margin", C.c_int32), ("scaling", C.c_int32),
        ("allow_rna", C.c_int32), ("pa_min", C.c_double), ("pa_max", C.c_double), ("n_slots", C.c_uint32),
        ("flags", C.c_uint32), ("device", C.c_int32), ("reserved", C.c_int32),
        ("table_t", C.c_void_p), ("table_u", C.c_void_p),
    ]


class PgBatch(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("location", C.c_int32), ("n_reads", C.c_uint32), ("n_ops", C.c_uint32),
        ("sig", C.c_void_p), ("sig_off", C.c_void_p), ("digitisation", C.c_void_p), ("offset", C.c_void_p),
        ("range", C.c_void_p), ("query_start", C.c_void_p), ("target_start", C.c_void_p), ("target_end", C.c_void_p),
        ("seq", C.c_void_p), ("seq_off", C.c_void_p), ("op_n", C.c_void_p), ("op_t", C.c_void_p), ("op_off", C.c_void_p),
        ("flags", C.c_uint32), ("reserved", C.c_uint32),
    ]


PG_BATCH_ALL_MATCHES = 1
PG_BATCH_RESIDENT = 2
PG_BATCH_GAPPED = 4


class PgResult(C.Structure):
    _fields_ = [
        ("n_slots", C.c_uint32), ("reserved", C.c_uint32), ("n_events", C.c_uint64), ("n_samples", C.c_uint64),
        ("n_reads", C.c_uint64), ("counts", C.c_void_p), ("ev_off", C.c_void_p), ("ev_len", C.c_void_p),
        ("ev_read", C.c_void_p), ("samp_off", C.c_void_p), ("samples", C.c_void_p), ("read_skipped", C.c_void_p),
    ]


class PgTextResult(C.Structure):
    _fields_ = [("n_slots", C.c_uint32), ("reserved", C.c_uint32), ("n_bytes", C.c_uint64), ("slot_off", C.POINTER(C.c_uint64))]


class PgDeviceView(C.Structure):
    _fields_ = [
        ("n_events", C.c_uint64), ("n_samples", C.c_uint64), ("d_keep", C.c_void_p), ("d_ev_off", C.c_void_p),
        ("d_ev_len", C.c_void_p), ("d_ev_read", C.c_void_p), ("d_samp_off", C.c_void_p), ("d_samples", C.c_void_p),
        ("d_med", C.c_void_p), ("d_mad", C.c_void_p),
    ]


class PgModelResult(C.Structure):
    _fields_ = [
        ("n_slots", C.c_uint32), ("flags", C.c_uint32), ("n_values", C.c_void_p), ("median", C.c_void_p), ("sstdev", C.c_void_p),
        ("mid_lo", C.c_void_p), ("mid_hi", C.c_void_p), ("origin", C.c_void_p), ("sum1", C.c_void_p), ("sum2_lo", C.c_void_p),
        ("sum2_hi", C.c_void_p), ("dwell_n", C.c_void_p), ("dwell_median", C.c_void_p),
    ]


class PgEventsResult(C.Structure):
    _fields_ = [("means", PgModelResult), ("sds", PgModelResult), ("status", C.c_void_p), ("n_events", C.c_void_p)]


class PgKfreqResult(C.Structure):
    _fields_ = [("kmer_size", C.c_uint32), ("reserved", C.c_uint32), ("n_odd", C.c_uint64),
                ("odd_keys", C.c_void_p), ("odd_counts", C.c_void_p)]


class PgF1Params(C.Structure):
    _fields_ = [("rna", C.c_int32), ("use_region", C.c_int32), ("threshold", C.c_int64), ("region_start", C.c_int64),
                ("region_end", C.c_int64)]


class PgF1Batch(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("location", C.c_int32), ("reserved", C.c_int32), ("ss", C.c_void_p),
                ("ss_off", C.c_void_p), ("sig_start", C.c_void_p), ("first_ref", C.c_void_p)]


class PgF1Result(C.Structure):
    _fields_ = [("totals", C.c_uint64 * 4), ("n_pairs", C.c_uint64), ("err_pair", C.c_int64), ("err_code", C.c_uint32),
                ("err_side", C.c_uint32)]


class PgPameanBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("location", C.c_int32), ("reserved", C.c_int32), ("sig", C.c_void_p), ("sig_off", C.c_void_p),
                ("digitisation", C.c_void_p), ("offset", C.c_void_p), ("range", C.c_void_p)]


class PgPameanResult(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_fallback", C.c_uint64), ("n_samples", C.c_uint64), ("mean", C.c_double), ("sstdev", C.c_double)]


class PgSigencResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_block_bytes", C.c_uint64), ("blocks", C.c_void_p), ("block_off", C.c_void_p)]


class PgSvbBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("location", C.c_int32), ("reserved", C.c_int32), ("blocks", C.c_void_p),
                ("n_block_bytes", C.c_uint64), ("block_off", C.c_void_p)]


class PgDmodelInfo(C.Structure):
    _fields_ = [("n_files", C.c_uint64), ("n_bytes", C.c_uint64), ("n_values", C.c_uint64), ("n_host_files", C.c_uint64),
                ("host_files", C.POINTER(C.c_uint32)), ("n_batches", C.c_uint32), ("reserved", C.c_uint32),
                ("parse_ms", C.c_double), ("model_ms", C.c_double)]


class PgPoolResult(C.Structure):
    _fields_ = [("model", PgModelResult), ("n_groups", C.c_uint32), ("n_batches", C.c_uint32), ("status", C.c_void_p), ("refused_file", C.c_void_p),
                ("n_files", C.c_void_p), ("n_files_total", C.c_uint64), ("n_bytes", C.c_uint64), ("n_values", C.c_uint64), ("select_ms", C.c_double)]


class PgKernelStat(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class PgMvopsBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("location", C.c_int32), ("flags", C.c_uint32), ("mv", C.c_void_p), ("n_mv_bytes", C.c_uint64),
                ("mv_off", C.c_void_p), ("stride", C.c_void_p), ("ns", C.c_void_p), ("ts", C.c_void_p), ("l_seq", C.c_void_p), ("flag", C.c_void_p),
                ("seq_bytes", C.c_void_p), ("n_seq_bytes", C.c_uint64), ("byte_off", C.c_void_p)]


class PgMvopsResult(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_ops", C.c_uint64), ("n_seq", C.c_uint64), ("n_refused", C.c_uint64), ("first_refused", C.c_int64),
                ("op_n", C.c_void_p), ("op_t", C.c_void_p), ("op_off", C.c_void_p), ("query_start", C.c_void_p), ("target_start", C.c_void_p),
                ("target_end", C.c_void_p), ("seq", C.c_void_p), ("seq_off", C.c_void_p), ("status", C.c_void_p), ("status_host", C.c_void_p)]


class PgMvopsCigars(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("location", C.c_int32), ("flags", C.c_uint32), ("op_n", C.c_void_p), ("n_ops", C.c_uint64), ("op_off", C.c_void_p),
                ("query_start", C.c_void_p), ("status", C.c_void_p), ("cigar", C.c_void_p), ("n_cigar", C.c_uint64), ("cigar_off", C.c_void_p), ("pos", C.c_void_p)]


class PgMvopsProjection(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_ops", C.c_uint64), ("n_refused", C.c_uint64), ("first_refused", C.c_int64),
                ("op_n", C.c_void_p), ("op_t", C.c_void_p), ("op_off", C.c_void_p), ("query_start", C.c_void_p), ("target_start", C.c_void_p),
                ("target_end", C.c_void_p), ("query_end", C.c_void_p), ("ref_len", C.c_void_p), ("n_match", C.c_void_p), ("status", C.c_void_p),
                ("status_host", C.c_void_p), ("ref_len_host", C.c_void_p), ("n_match_host", C.c_void_p), ("query_end_host", C.c_void_p)]


class PgMvopsStrands(C.Structure):
    _fields_ = [("reverse", C.c_void_p), ("contig_len", C.c_void_p)]


class PgRefseqReads(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("location", C.c_int32), ("contig", C.c_void_p), ("pos", C.c_void_p), ("ref_len", C.c_void_p), ("reverse", C.c_void_p)]


class PgRefseqSlices(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("seq_off", C.c_void_p), ("n_seq", C.c_uint64)]


class PgFitParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sig_move_offset", C.c_uint32), ("min_dur", C.c_uint32), ("max_dur", C.c_uint32), ("min_events", C.c_uint32),
                ("rna", C.c_int32)]


class PgFitReads(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("sums", C.c_void_p), ("status", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p)]


class PgFitScaling(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_ok", C.c_uint64), ("d_sums", C.c_void_p), ("d_status", C.c_void_p), ("d_a", C.c_void_p), ("d_b", C.c_void_p),
                ("d_center", C.c_void_p), ("d_spread", C.c_void_p), ("d_use", C.c_void_p), ("n_status", C.c_uint64 * 8), ("solve_ms", C.c_double)]


PG_SCALING_PER_READ = 2


class PgFitResult(C.Structure):
    _fields_ = [("kmer_size", C.c_uint32), ("reserved", C.c_uint32), ("n_slots", C.c_uint64), ("n_samples", C.c_void_p), ("n_events", C.c_void_p),
                ("sum_d", C.c_void_p), ("sum_dd_lo", C.c_void_p), ("sum_dd_hi", C.c_void_p), ("reads", C.c_uint64), ("fitted", C.c_uint64),
                ("events", C.c_uint64), ("samples", C.c_uint64), ("clamped", C.c_uint64)]


class PgRealignParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sig_move_offset", C.c_uint32), ("min_dur", C.c_uint32), ("max_dur", C.c_uint32), ("rna", C.c_int32),
                ("band", C.c_uint32), ("min_len", C.c_uint32), ("phase", C.c_uint32)]


class PgRealignRead(C.Structure):
    _fields_ = [("n_free", C.c_uint32), ("n_moved", C.c_uint32), ("sum_abs_shift", C.c_uint64), ("cost_before_lo", C.c_uint64), ("cost_before_hi", C.c_uint64),
                ("cost_after_lo", C.c_uint64), ("cost_after_hi", C.c_uint64)]


class PgRealignReads(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_reads", C.c_uint64), ("n_ops", C.c_uint64), ("op_n", C.c_void_p), ("reads", C.c_void_p)]


class PgEvalignParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sig_move_offset", C.c_uint32), ("min_dur", C.c_uint32), ("max_dur", C.c_uint32), ("rna", C.c_int32),
                ("sample_rate", C.c_uint32), ("flags", C.c_uint32)]


class PgEvalignMeta(C.Structure):
    _fields_ = [("ref_start", C.c_void_p), ("reverse", C.c_void_p), ("contig", C.c_void_p), ("contig_off", C.c_void_p), ("label", C.c_void_p), ("label_off", C.c_void_p)]


class PgEvalignOut(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_reads", C.c_uint64), ("n_rows", C.c_uint64), ("row_off", C.c_void_p), ("rows", C.c_void_p),
                ("rows_host", C.c_void_p), ("text", C.c_void_p), ("text_bytes", C.c_uint64)]


PG_EVALIGN_TEXT, PG_EVALIGN_HOST_ROWS = 1, 2
# pg_evalign_row as a numpy structured type (40 bytes)
EVALIGN_ROW_DTYPE = [("read", "<u4"), ("event", "<u4"), ("start", "<u8"), ("n", "<u4"), ("slot", "<u4"), ("first", "<u4"), ("mean_u", "<i4"), ("stdv_u", "<i4"), ("z_c", "<i4")]


class PgSimParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kmer_size", C.c_uint32), ("sig_move_offset", C.c_uint32), ("rna", C.c_int32), ("seed", C.c_uint64), ("range_e4", C.c_uint64),
                ("digitisation", C.c_uint32), ("offset", C.c_int32), ("off_spread", C.c_uint32), ("spread_pct", C.c_uint32), ("lead", C.c_uint32), ("lead_level", C.c_uint32),
                ("lead_stdv", C.c_uint32), ("reserved", C.c_uint32)]


class PgSimBatch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("location", C.c_int32), ("n_reads", C.c_uint32), ("reserved", C.c_uint32), ("first_read", C.c_uint64), ("seq", C.c_void_p),
                ("seq_off", C.c_void_p)]


class PgSimResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_reads", C.c_uint64), ("n_ops", C.c_uint64), ("n_samples", C.c_uint64), ("n_seq", C.c_uint64),
                ("n_refused", C.c_uint64), ("sig", C.c_void_p), ("sig_off", C.c_void_p), ("digitisation", C.c_void_p), ("offset", C.c_void_p), ("range", C.c_void_p),
                ("query_start", C.c_void_p), ("target_start", C.c_void_p), ("target_end", C.c_void_p), ("seq", C.c_void_p), ("seq_off", C.c_void_p), ("op_n", C.c_void_p),
                ("op_t", C.c_void_p), ("op_off", C.c_void_p), ("status", C.c_void_p), ("status_host", C.c_void_p)]


_lib = None


def _preload_hip_runtime():
    """libpgmove.so has no DT_NEEDED on the HIP runtime (see Makefile): bring exactly one copy into the
    global symbol scope first. With PyTorch present that must be the libamdhip64 it bundles, otherwise the
    process would hold two HIP/HSA runtimes and the second one finds no GPU."""
    cands = []
    try:
        import torch  # noqa: F401  (loads its bundled ROCm libraries)
        cands.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except Exception:
        pass
    cands += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    last = None
    for path in cands:
        if os.path.isabs(path) and not os.path.exists(path):
            continue
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
            return path
        except OSError as e:  # try the next candidate
            last = e
    raise RuntimeError(f"no HIP runtime (libamdhip64) could be loaded: {last}")


def load():
    """Load libpgmove.so (once). Raises if the HIP library is missing: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `make` (or __graft_entry__.build()). "
            "poregen_amd has no CPU fallback for the gmove path.")
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    vp, u32, i32, u64p = C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p
    lib.pg_default_params.argtypes = [C.POINTER(PgParams)]; lib.pg_default_params.restype = None
    lib.pg_last_error.argtypes = [vp]; lib.pg_last_error.restype = C.c_char_p
    lib.pg_version.argtypes = []; lib.pg_version.restype = C.c_char_p
    lib.pg_build_slot_tables.argtypes = [u32, C.POINTER(C.c_char_p), u32, vp, vp]; lib.pg_build_slot_tables.restype = i32
    lib.pg_create.argtypes = [C.POINTER(PgParams), C.POINTER(vp)]; lib.pg_create.restype = i32
    lib.pg_destroy.argtypes = [vp]; lib.pg_destroy.restype = None
    lib.pg_reset.argtypes = [vp]; lib.pg_reset.restype = i32
    lib.pg_submit.argtypes = [vp, C.POINTER(PgBatch)]; lib.pg_submit.restype = i32
    lib.pg_count.argtypes = [vp, C.POINTER(PgBatch), u64p, i32]; lib.pg_count.restype = i32
    lib.pg_collect.argtypes = [vp, u64p, i32]; lib.pg_collect.restype = i32
    lib.pg_stats.argtypes = [vp]; lib.pg_stats.restype = i32
    lib.pg_collect_gathered.argtypes = [vp, u64p, C.c_uint32, C.c_uint32]; lib.pg_collect_gathered.restype = i32
    lib.pg_finish_deferred.argtypes = [vp, C.POINTER(PgResult)]; lib.pg_finish_deferred.restype = i32
    lib.pg_fetch_samples.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_void_p]; lib.pg_fetch_samples.restype = i32
    lib.pg_text.argtypes = [vp, C.POINTER(PgTextResult)]; lib.pg_text.restype = i32
    lib.pg_fetch_text.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_void_p]; lib.pg_fetch_text.restype = i32
    lib.pg_job_totals_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]; lib.pg_job_totals_device.restype = i32
    lib.pg_sync.argtypes = [vp]; lib.pg_sync.restype = i32
    lib.pg_set_stream.argtypes = [vp, vp]; lib.pg_set_stream.restype = i32
    lib.pg_finish.argtypes = [vp, C.POINTER(PgResult)]; lib.pg_finish.restype = i32
    lib.pg_all_slots_full.argtypes = [vp]; lib.pg_all_slots_full.restype = i32
    lib.pg_last_batch_device.argtypes = [vp, C.POINTER(PgDeviceView)]; lib.pg_last_batch_device.restype = i32
    lib.pg_kernel_stats.argtypes = [vp, C.POINTER(PgKernelStat), u32, C.POINTER(u32)]; lib.pg_kernel_stats.restype = i32
    lib.pg_kernel_stats_reset.argtypes = [vp]; lib.pg_kernel_stats_reset.restype = i32
    lib.pg_model.argtypes = [vp, u32, C.POINTER(PgModelResult)]; lib.pg_model.restype = i32
    lib.pg_model_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, C.POINTER(PgModelResult)]; lib.pg_model_device.restype = i32
    lib.pg_model_format.argtypes = [C.POINTER(PgModelResult), u32, i32, C.c_char_p, C.c_size_t]; lib.pg_model_format.restype = C.c_size_t
    lib.pg_runtime_init.argtypes = [i32]; lib.pg_runtime_init.restype = i32
    lib.pg_all_slots_full_settled.argtypes = [vp]; lib.pg_all_slots_full_settled.restype = i32
    lib.pg_job_all_slots_full_settled.argtypes = [vp]; lib.pg_job_all_slots_full_settled.restype = i32
    lib.pg_poll.argtypes = [vp]; lib.pg_poll.restype = i32
    lib.pg_job_poll.argtypes = [vp]; lib.pg_job_poll.restype = i32
    lib.pg_job_create.argtypes = [C.POINTER(PgParams), C.POINTER(C.c_int32), u32, u32, C.POINTER(vp)]; lib.pg_job_create.restype = i32
    lib.pg_job_destroy.argtypes = [vp]; lib.pg_job_destroy.restype = None
    lib.pg_job_last_error.argtypes = [vp]; lib.pg_job_last_error.restype = C.c_char_p
    lib.pg_job_submit.argtypes = [vp, C.POINTER(PgBatch)]; lib.pg_job_submit.restype = i32
    if hasattr(lib, "pg_job_submit_shards"):  # (a measurement build of an earlier round loaded through bench.py --lib lacks the newer entry points)
        lib.pg_job_submit_shards.argtypes = [vp, C.POINTER(PgBatch), C.c_uint32]; lib.pg_job_submit_shards.restype = i32
        lib.pg_job_reset.argtypes = [vp]; lib.pg_job_reset.restype = i32
    lib.pg_job_sync.argtypes = [vp]; lib.pg_job_sync.restype = i32
    lib.pg_job_all_slots_full.argtypes = [vp]; lib.pg_job_all_slots_full.restype = i32
    lib.pg_job_finish.argtypes = [vp, C.POINTER(PgResult)]; lib.pg_job_finish.restype = i32
    lib.pg_job_finish_deferred.argtypes = [vp, C.POINTER(PgResult)]; lib.pg_job_finish_deferred.restype = i32
    lib.pg_job_fetch_samples.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_void_p]; lib.pg_job_fetch_samples.restype = i32
    lib.pg_job_text.argtypes = [vp, C.POINTER(PgTextResult)]; lib.pg_job_text.restype = i32
    lib.pg_job_fetch_text.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_void_p]; lib.pg_job_fetch_text.restype = i32
    lib.pg_text_device.argtypes = [vp, u32, C.c_uint64, vp, vp, vp, C.POINTER(PgTextResult)]; lib.pg_text_device.restype = i32
    lib.pg_job_uses_rccl.argtypes = [vp]; lib.pg_job_uses_rccl.restype = i32
    lib.pg_job_model.argtypes = [vp, u32, C.POINTER(PgModelResult)]; lib.pg_job_model.restype = i32
    lib.pg_job_kernel_stats.argtypes = [vp, u32, C.POINTER(PgKernelStat), u32, C.POINTER(u32)]; lib.pg_job_kernel_stats.restype = i32
    lib.pg_kfreq_create.argtypes = [u32, i32, C.POINTER(vp)]; lib.pg_kfreq_create.restype = i32
    lib.pg_kfreq_destroy.argtypes = [vp]; lib.pg_kfreq_destroy.restype = None
    lib.pg_kfreq_last_error.argtypes = [vp]; lib.pg_kfreq_last_error.restype = C.c_char_p
    lib.pg_kfreq_submit.argtypes = [vp, vp, C.c_uint64, i32]; lib.pg_kfreq_submit.restype = i32
    lib.pg_kfreq_submit_reads.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, u32, i32]; lib.pg_kfreq_submit_reads.restype = i32
    lib.pg_kfreq_submit_fasta.argtypes = [vp, vp, C.c_uint64, i32]; lib.pg_kfreq_submit_fasta.restype = i32
    lib.pg_kfreq_reads_piece.argtypes = [vp]; lib.pg_kfreq_reads_piece.restype = u32
    lib.pg_kfreq_sync.argtypes = [vp]; lib.pg_kfreq_sync.restype = i32
    lib.pg_kfreq_finish.argtypes = [vp, vp, C.POINTER(PgKfreqResult)]; lib.pg_kfreq_finish.restype = i32
    lib.pg_fscore_create.argtypes = [C.POINTER(PgF1Params), i32, C.POINTER(vp)]; lib.pg_fscore_create.restype = i32
    lib.pg_fscore_destroy.argtypes = [vp]; lib.pg_fscore_destroy.restype = None
    lib.pg_fscore_last_error.argtypes = [vp]; lib.pg_fscore_last_error.restype = C.c_char_p
    lib.pg_fscore_submit.argtypes = [vp, C.POINTER(PgF1Batch)]; lib.pg_fscore_submit.restype = i32
    lib.pg_fscore_sync.argtypes = [vp]; lib.pg_fscore_sync.restype = i32
    lib.pg_fscore_finish.argtypes = [vp, C.POINTER(PgF1Result), vp, C.c_uint64]; lib.pg_fscore_finish.restype = i32
    lib.pg_pamean_create.argtypes = [i32, C.POINTER(vp)]; lib.pg_pamean_create.restype = i32
    lib.pg_pamean_destroy.argtypes = [vp]; lib.pg_pamean_destroy.restype = None
    lib.pg_pamean_last_error.argtypes = [vp]; lib.pg_pamean_last_error.restype = C.c_char_p
    lib.pg_pamean_submit.argtypes = [vp, C.POINTER(PgPameanBatch), vp]; lib.pg_pamean_submit.restype = i32
    lib.pg_pamean_sync.argtypes = [vp]; lib.pg_pamean_sync.restype = i32
    lib.pg_pamean_finish.argtypes = [vp, C.POINTER(PgPameanResult)]; lib.pg_pamean_finish.restype = i32
    lib.pg_pamean_submit_svb.argtypes = [vp, C.POINTER(PgSvbBatch), vp, vp, vp, vp]; lib.pg_pamean_submit_svb.restype = i32
    lib.pg_pamean_svb_samples.argtypes = [vp]; lib.pg_pamean_svb_samples.restype = C.c_uint64
    lib.pg_sigdec_create.argtypes = [i32, C.POINTER(vp)]; lib.pg_sigdec_create.restype = i32
    lib.pg_sigdec_destroy.argtypes = [vp]; lib.pg_sigdec_destroy.restype = None
    lib.pg_sigdec_last_error.argtypes = [vp]; lib.pg_sigdec_last_error.restype = C.c_char_p
    lib.pg_sigdec_counts.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, i32, vp]; lib.pg_sigdec_counts.restype = i32
    lib.pg_sigdec_decode.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, i32, vp, vp, vp]; lib.pg_sigdec_decode.restype = i32
    lib.pg_dmodel_create.argtypes = [i32, u32, C.POINTER(vp)]; lib.pg_dmodel_create.restype = i32
    lib.pg_dmodel_destroy.argtypes = [vp]; lib.pg_dmodel_destroy.restype = None
    lib.pg_dmodel_last_error.argtypes = [vp]; lib.pg_dmodel_last_error.restype = C.c_char_p
    lib.pg_dmodel_submit.argtypes = [vp, vp, vp, u32, i32]; lib.pg_dmodel_submit.restype = i32
    lib.pg_dmodel_sync.argtypes = [vp]; lib.pg_dmodel_sync.restype = i32
    lib.pg_dmodel_finish.argtypes = [vp, C.POINTER(PgModelResult), C.POINTER(PgDmodelInfo)]; lib.pg_dmodel_finish.restype = i32
    lib.pg_dmodel_format.argtypes = [vp, u32, i32, C.c_char_p, C.c_size_t]; lib.pg_dmodel_format.restype = C.c_size_t
    if hasattr(lib, "pg_dmodel_finish_events"):  # (bench.py --lib may load a library built from an older tree, without the event table)
        lib.pg_dmodel_finish_events.argtypes = [vp, C.POINTER(PgModelResult), C.POINTER(PgModelResult), C.POINTER(vp), C.POINTER(vp)]; lib.pg_dmodel_finish_events.restype = i32
        lib.pg_dmodel_format_events.argtypes = [vp, u32, i32, C.c_char_p, C.c_size_t]; lib.pg_dmodel_format_events.restype = C.c_size_t
        lib.pg_dmodel_events_refusal.argtypes = [vp, u32]; lib.pg_dmodel_events_refusal.restype = C.c_char_p
        lib.pg_dmodel_events_values.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]; lib.pg_dmodel_events_values.restype = i32
        lib.pg_dmodel_events_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]; lib.pg_dmodel_events_ms.restype = i32
        lib.pg_model_events.argtypes = [vp, u32, C.POINTER(PgEventsResult)]; lib.pg_model_events.restype = i32
        lib.pg_events_status_text.argtypes = [u32]; lib.pg_events_status_text.restype = C.c_char_p
    if hasattr(lib, "pg_pool_create"):  # (as above: an earlier round's measurement build lacks the newer entry points)
        lib.pg_pool_create.argtypes = [i32, u32, vp, C.c_uint64, u32, C.POINTER(vp)]; lib.pg_pool_create.restype = i32
        lib.pg_pool_destroy.argtypes = [vp]; lib.pg_pool_destroy.restype = None
        lib.pg_pool_last_error.argtypes = [vp]; lib.pg_pool_last_error.restype = C.c_char_p
        lib.pg_pool_submit.argtypes = [vp, vp, vp, u32, vp, i32]; lib.pg_pool_submit.restype = i32
        lib.pg_pool_sync.argtypes = [vp]; lib.pg_pool_sync.restype = i32
        lib.pg_pool_finish.argtypes = [vp, C.POINTER(PgPoolResult)]; lib.pg_pool_finish.restype = i32
        lib.pg_pool_format.argtypes = [vp, u32, i32, C.c_char_p, C.c_size_t]; lib.pg_pool_format.restype = C.c_size_t
        lib.pg_pool_refusal.argtypes = [vp, u32]; lib.pg_pool_refusal.restype = C.c_char_p
    lib.pg_transform_model.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t,
                                       C.POINTER(vp), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]; lib.pg_transform_model.restype = i32
    lib.pg_transform_free.argtypes = [vp]; lib.pg_transform_free.restype = None
    lib.pg_mvops_create.argtypes = [i32, C.POINTER(vp)]; lib.pg_mvops_create.restype = i32
    lib.pg_mvops_destroy.argtypes = [vp]; lib.pg_mvops_destroy.restype = None
    lib.pg_mvops_last_error.argtypes = [vp]; lib.pg_mvops_last_error.restype = C.c_char_p
    lib.pg_mvops_piece.argtypes = [vp]; lib.pg_mvops_piece.restype = u32
    lib.pg_mvops_set_stream.argtypes = [vp, vp]; lib.pg_mvops_set_stream.restype = i32
    lib.pg_mvops_stream.argtypes = [vp]; lib.pg_mvops_stream.restype = vp
    lib.pg_mvops_expand.argtypes = [vp, C.POINTER(PgMvopsBatch), C.POINTER(PgMvopsResult)]; lib.pg_mvops_expand.restype = i32
    lib.pg_mvops_project.argtypes = [vp, C.POINTER(PgMvopsCigars), C.POINTER(PgMvopsProjection)]; lib.pg_mvops_project.restype = i32
    lib.pg_mvops_project_stranded.argtypes = [vp, C.POINTER(PgMvopsCigars), C.POINTER(PgMvopsStrands), C.POINTER(PgMvopsProjection)]; lib.pg_mvops_project_stranded.restype = i32
    lib.pg_refseq_create.argtypes = [i32, C.POINTER(vp)]; lib.pg_refseq_create.restype = i32
    lib.pg_refseq_destroy.argtypes = [vp]; lib.pg_refseq_destroy.restype = None
    lib.pg_refseq_last_error.argtypes = [vp]; lib.pg_refseq_last_error.restype = C.c_char_p
    lib.pg_refseq_set_stream.argtypes = [vp, vp]; lib.pg_refseq_set_stream.restype = i32
    lib.pg_refseq_add.argtypes = [vp, vp, C.c_uint64, C.POINTER(i32)]; lib.pg_refseq_add.restype = i32
    lib.pg_refseq_slice.argtypes = [vp, C.POINTER(PgRefseqReads), C.POINTER(PgRefseqSlices)]; lib.pg_refseq_slice.restype = i32
    if hasattr(lib, "pg_fit_create"):  # (as above: a library built from an older tree has no fit handle)
        lib.pg_fit_create.argtypes = [C.POINTER(PgFitParams), i32, C.POINTER(vp)]; lib.pg_fit_create.restype = i32
        lib.pg_fit_destroy.argtypes = [vp]; lib.pg_fit_destroy.restype = None
        lib.pg_fit_last_error.argtypes = [vp]; lib.pg_fit_last_error.restype = C.c_char_p
        lib.pg_fit_set_model.argtypes = [vp, vp, u32]; lib.pg_fit_set_model.restype = i32
        lib.pg_fit_submit.argtypes = [vp, C.POINTER(PgBatch), vp, C.POINTER(PgFitReads)]; lib.pg_fit_submit.restype = i32
        lib.pg_fit_finish.argtypes = [vp, C.POINTER(PgFitResult)]; lib.pg_fit_finish.restype = i32
        lib.pg_fit_calibrate.argtypes = [vp, C.POINTER(PgBatch), vp, C.POINTER(PgFitScaling)]; lib.pg_fit_calibrate.restype = i32
        lib.pg_set_read_scaling.argtypes = [vp, vp, vp, vp, i32]; lib.pg_set_read_scaling.restype = i32
        lib.pg_fit_set_stream.argtypes = [vp, vp]; lib.pg_fit_set_stream.restype = i32
        lib.pg_fit_pass_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]; lib.pg_fit_pass_ms.restype = i32
        lib.pg_fit_parse_model.argtypes = [C.c_char_p, C.c_size_t, u32, C.POINTER(u32), vp, C.c_size_t, C.POINTER(i32), C.c_char_p, C.c_size_t]; lib.pg_fit_parse_model.restype = i32
        lib.pg_fit_residuals.argtypes = [C.c_uint64, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.pg_fit_residuals.restype = i32
    if hasattr(lib, "pg_realign_create"):  # (as above: a library built from an older tree has no realign handle)
        lib.pg_realign_create.argtypes = [C.POINTER(PgRealignParams), i32, C.POINTER(vp)]; lib.pg_realign_create.restype = i32
        lib.pg_realign_destroy.argtypes = [vp]; lib.pg_realign_destroy.restype = None
        lib.pg_realign_last_error.argtypes = [vp]; lib.pg_realign_last_error.restype = C.c_char_p
        lib.pg_realign_set_model.argtypes = [vp, vp, u32]; lib.pg_realign_set_model.restype = i32
        lib.pg_realign_set_stream.argtypes = [vp, vp]; lib.pg_realign_set_stream.restype = i32
        lib.pg_realign_submit.argtypes = [vp, C.POINTER(PgBatch), vp, vp, vp, C.POINTER(PgRealignReads)]; lib.pg_realign_submit.restype = i32
        lib.pg_realign_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]; lib.pg_realign_kernel_ms.restype = i32
        lib.pg_realign_walk.argtypes = [C.POINTER(PgRealignParams), vp, u32, vp, u32, vp, C.c_int64, vp, C.c_uint64, C.c_double, C.c_double, vp, C.POINTER(PgRealignRead)]
        lib.pg_realign_walk.restype = i32
        if hasattr(lib, "pg_realign_walk_gapped"):  # (a library built from the tree before gapped batches: --lib A/B runs of the all-matches submits)
            lib.pg_realign_walk_gapped.argtypes = [C.POINTER(PgRealignParams), vp, u32, vp, C.c_uint64, vp, vp, u32, C.c_int64, vp, C.c_uint64, C.c_double, C.c_double, vp,
                                                   C.POINTER(PgRealignRead)]
            lib.pg_realign_walk_gapped.restype = i32
        if hasattr(lib, "pg_realign_set_phase"):  # (a library built from the tree before the phase: --lib A/B runs at phase 0)
            lib.pg_realign_set_phase.argtypes = [vp, u32]; lib.pg_realign_set_phase.restype = i32
    if hasattr(lib, "pg_evalign_create"):  # (as above: a library built from an older tree has no eventalign handle)
        dbl = C.c_double
        lib.pg_evalign_create.argtypes = [C.POINTER(PgEvalignParams), i32, C.POINTER(vp)]; lib.pg_evalign_create.restype = i32
        lib.pg_evalign_destroy.argtypes = [vp]; lib.pg_evalign_destroy.restype = None
        lib.pg_evalign_last_error.argtypes = [vp]; lib.pg_evalign_last_error.restype = C.c_char_p
        lib.pg_evalign_set_model.argtypes = [vp, vp, vp, u32]; lib.pg_evalign_set_model.restype = i32
        lib.pg_evalign_set_stream.argtypes = [vp, vp]; lib.pg_evalign_set_stream.restype = i32
        lib.pg_evalign_submit.argtypes = [vp, C.POINTER(PgBatch), vp, vp, vp, C.POINTER(PgEvalignMeta), C.POINTER(PgEvalignOut)]; lib.pg_evalign_submit.restype = i32
        lib.pg_evalign_copy_text.argtypes = [vp, vp, C.c_uint64]; lib.pg_evalign_copy_text.restype = i32
        lib.pg_evalign_kernel_ms.argtypes = [vp, vp]; lib.pg_evalign_kernel_ms.restype = i32
        lib.pg_evalign_walk.argtypes = [C.POINTER(PgEvalignParams), vp, vp, u32, vp, u32, vp, C.c_int64, vp, C.c_uint64, dbl, dbl, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.pg_evalign_walk.restype = i32
        lib.pg_evalign_walk_gapped.argtypes = [C.POINTER(PgEvalignParams), vp, vp, u32, vp, C.c_uint64, vp, vp, u32, C.c_int64, vp, C.c_uint64, dbl, dbl, vp, C.c_uint64,
                                               C.POINTER(C.c_uint64)]
        lib.pg_evalign_walk_gapped.restype = i32
        lib.pg_evalign_row_text.argtypes = [vp, vp, u32, vp, u32, vp, u32, C.c_uint64, C.c_int64, i32, u32, u32, u32, vp, C.c_uint64]; lib.pg_evalign_row_text.restype = C.c_uint64
    if hasattr(lib, "pg_sim_create"):  # (as above: a library built from an older tree has no simulator)
        lib.pg_sim_create.argtypes = [C.POINTER(PgSimParams), i32, C.POINTER(vp)]; lib.pg_sim_create.restype = i32
        lib.pg_sim_destroy.argtypes = [vp]; lib.pg_sim_destroy.restype = None
        lib.pg_sim_last_error.argtypes = [vp]; lib.pg_sim_last_error.restype = C.c_char_p
        lib.pg_sim_set_stream.argtypes = [vp, vp]; lib.pg_sim_set_stream.restype = i32
        lib.pg_sim_stream.argtypes = [vp]; lib.pg_sim_stream.restype = vp
        lib.pg_sim_set_model.argtypes = [vp, vp, vp, vp, u32]; lib.pg_sim_set_model.restype = i32
        lib.pg_sim_generate.argtypes = [vp, C.POINTER(PgSimBatch), C.POINTER(PgSimResult)]; lib.pg_sim_generate.restype = i32
        lib.pg_sim_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]; lib.pg_sim_kernel_ms.restype = i32
        lib.pg_sim_walk.argtypes = [C.POINTER(PgSimParams), vp, vp, vp, vp, u32, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(u32), C.POINTER(i32)]
        lib.pg_sim_walk.restype = i32
        lib.pg_sim_parse_model.argtypes = [C.c_char_p, C.c_size_t, u32, C.POINTER(u32), vp, vp, C.c_size_t, C.POINTER(i32), C.c_char_p, C.c_size_t]; lib.pg_sim_parse_model.restype = i32
        lib.pg_sim_parse_dwell.argtypes = [C.c_char_p, C.c_size_t, u32, C.POINTER(u32), vp, C.c_size_t, C.c_char_p, C.c_size_t]; lib.pg_sim_parse_dwell.restype = i32
    if hasattr(lib, "pg_sigenc_create"):  # (as above: a library built from an older tree has no encoder)
        lib.pg_sigenc_create.argtypes = [i32, C.POINTER(vp)]; lib.pg_sigenc_create.restype = i32
        lib.pg_sigenc_destroy.argtypes = [vp]; lib.pg_sigenc_destroy.restype = None
        lib.pg_sigenc_last_error.argtypes = [vp]; lib.pg_sigenc_last_error.restype = C.c_char_p
        lib.pg_sigenc_set_stream.argtypes = [vp, vp]; lib.pg_sigenc_set_stream.restype = i32
        lib.pg_sigenc_stream.argtypes = [vp]; lib.pg_sigenc_stream.restype = vp
        lib.pg_sigenc_bound.argtypes = [vp, C.c_uint64]; lib.pg_sigenc_bound.restype = C.c_uint64
        lib.pg_sigenc_encode.argtypes = [vp, vp, vp, C.c_uint64, i32, C.POINTER(PgSigencResult)]; lib.pg_sigenc_encode.restype = i32
        lib.pg_sigenc_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]; lib.pg_sigenc_kernel_ms.restype = i32
    _lib = lib
    return lib
