/* pgmove.h -- C ABI of libpgmove: the MI355X (gfx950) implementation of poregen's `gmove` collector.
 *
 * The reference (hiruna72/poregen) has no plugin/FFI interface; its only seam for this path is the
 * internal C++ function
 *     void process_move_table_paf(char *move_table, std::map<std::string,FILE*>&, slow5_file_t **sp,
 *                                 opt_t*, std::map<std::string,uint64_t>&, std::vector<std::string>& kmers,
 *                                 char *fastq)                                   (src/gmove.cpp:76, 707-975)
 * called once from gmove() (src/gmove.cpp:515). This header is the boundary a maintainer would bind
 * at that seam: the host keeps all I/O (slow5lib / PAF / FASTQ parsing, the k-mer
 * list, output files) and hands batches of parsed reads to the device; the device does the per-read
 * ss walk, event filtering, deterministic first-`sample_limit` selection per k-mer, pA conversion,
 * med-MAD normalisation and the gather of kept windows.
 *
 * Conventions: plain C types only; no exceptions cross the ABI; every call returns a pg_status
 * (0 = ok, <0 = error, text via pg_last_error); the library never calls exit(). One pg_ctx per host
 * thread (like the reference, a context is not thread-safe). There is NO CPU fallback: pg_create
 * fails with PG_ERR_NO_DEVICE when no HIP device is usable.
 *
 * Entry point                      replaces (reference file:line)
 * -------------------------------  ---------------------------------------------------------------
 * pg_default_params                init_opt defaults                      src/poregen.cpp:209-237
 * pg_build_slot_tables             kmer_file_pointer_array/kmer_frequency_map keyed by k-mer string
 *                                                                         src/gmove.cpp:460-477
 * pg_create / pg_destroy           per-run state set up in gmove()        src/gmove.cpp:460-503
 * pg_submit                        one batch of while(getline) iterations src/gmove.cpp:732-969
 * pg_count + pg_collect            the same, split at the "count == sample_limit" test
 *                                  (src/gmove.cpp:925-927) so that several GPUs can exchange
 *                                  per-k-mer counts between the two halves
 * pg_finish                        the bytes the fprintf calls would have produced, as binary
 *                                                                         src/gmove.cpp:938-950
 * pg_finish_deferred /             the same with the samples left on the device, fetched range by range
 * pg_fetch_samples
 * pg_text / pg_fetch_text /        those bytes themselves: fprintf(f, "%.8f,") ... "%.8f;" on the device   src/gmove.cpp:938-944
 * pg_text_device
 * pg_all_slots_full                the early loop exit                    src/gmove.cpp:733-735
 * pg_model / pg_model_device /     the step behind gmove in the reference's pipeline: dump files -> tr | tail | datamash
 * pg_model_format                  median / sstdev per k-mer, awk | datamash median of the dwell times
 *                                                                         scripts/poregen.sh:54-85, 33-52
 * pg_job_create / _submit / _sync  a batch split over the node's GPUs from one process: the shape of the reference's only
 * / _finish / _all_slots_full /    parallel driver, work_db (a batch split over worker threads)   src/thread.c:119-132,
 * _model / _destroy                plugged in at the same seam as pg_submit                       src/gmove.cpp:515
 * pg_job_finish_deferred /         the job's output side, as the pg_ctx calls of the same names: the shards' kept samples
 * _fetch_samples / _text /         concatenated on the first device (peer copies over xGMI), text produced there
 * _fetch_text                                                                                     src/gmove.cpp:938-950
 * pg_set_stream / pg_sync /        (no counterpart: the reference is synchronous and single-threaded)
 * pg_runtime_init / pg_poll / pg_all_slots_full_settled / pg_last_batch_device / pg_kernel_stats*
 *
 * The `kmer_freq` subtool (src/kmer_freq.cpp) has a handle of its own:
 * pg_kfreq_create / pg_kfreq_destroy  the generated 4^k keys at zero and the map   src/kmer_freq.cpp:148-157
 * pg_kfreq_submit                  the getline loop over the FASTQ: lines, the     src/kmer_freq.cpp:160-181
 *                                  sequence-line test, one map increment per window
 * pg_kfreq_submit_reads            the same loop over the FASTQ that `samtools fastq` README.md STEP 2
 *                                  (and `sed '2~4s/N/T/g'`) would print from a batch
 *                                  of BAM records, without the text: the records'
 *                                  packed sequence fields are the input
 * pg_kfreq_submit_fasta            the same count over a FASTA (README.md STEP 3:   README.md STEP 2-3
 *                                  count_kmer_freq.py 5 ${FASTA}), records wrapped
 *                                  over any number of lines
 * pg_kfreq_reads_piece             (no counterpart)
 * pg_kfreq_finish                  the map's contents (dense ACGT counts + the     src/kmer_freq.cpp:189-192
 *                                  other keys in byte order); sorting and printing,
 *                                  :194-220, stay with the caller
 * pg_kfreq_sync / pg_kfreq_last_error  (no counterpart)
 *
 * The move tables of BAM records to ss ops (scripts/poregen.sh STEP 4, `reform -c -k 1`) have one:
 * pg_mvops_create / _destroy       (no counterpart)
 * pg_mvops_expand                  the PAF branch of reform() for a batch of      src/reform.cpp:284-358
 *                                  records, and `samtools fastq` of their bases
 * pg_mvops_project                 those ops carried through the records' CIGARs   README.md, first paragraph ("signal-to-read
 *                                  onto the reference: the PAF that gmove's PAF    or signal-to-reference"); src/gmove.cpp:792-860
 *                                  walk reads against a reference FASTA (the       reads such a PAF, src/realign.cpp, which was
 *                                  reference leaves making it to squigualiser)     to write it, is an empty copy of reform
 * pg_mvops_project_stranded        the same for records of either strand: a        (no counterpart: the reference has no
 *                                  reverse record is a forward record on the       projection; src/gmove.cpp:792-805 fetches
 *                                  reverse complement of its contig                whatever contig a PAF names)
 * pg_mvops_piece / _set_stream /   (no counterpart)
 * _stream / _last_error
 * pg_refseq_create / _destroy /    (no counterpart)
 * _add / _set_stream / _last_error
 * pg_refseq_slice                  faidx_fetch_seq(m_fai, tid, st_k, end_k - 1)    src/gmove.cpp:792-805
 *                                  for a batch of reads, reverse-complemented for
 *                                  reverse-strand ones
 *
 * The F1-score metric (src/f1_score/f1score.py) has one too:
 * pg_fscore_create / _destroy     args.rna / args.threshold / args.region         src/f1_score/f1score.py:59-66, 234-246
 * pg_fscore_submit                 parse_ss_string + compare_mappings of every     src/f1_score/f1score.py:7-119, 135-153
 *                                  compared pair (the dict rules, si parsing and
 *                                  printing, :157-231, stay with the caller)
 * pg_fscore_finish                 the TOT_* sums (per pair on request)            src/f1_score/f1score.py:224-229
 * pg_fscore_sync / _last_error     (no counterpart)
 *
 * The k-mer model from dump directories (STEP 6 of scripts/poregen.sh as a tool of its own) has one as well:
 * pg_dmodel_create / _destroy      (no counterpart)
 * pg_dmodel_submit                 tr ';,' '\n' < file | tail -n +2 and awk -F';' of a batch of dump files: the text parsed on the
 *                                  device                                          scripts/poregen.sh:66-67, 43
 * pg_dmodel_finish / _format       datamash median / sstdev per file               scripts/poregen.sh:66-67, 43
 * pg_dmodel_sync / _last_error     (no counterpart)
 * pg_dmodel_finish_events /        (no counterpart: per file the median / sstdev of its events' means and of its events' standard
 * _format_events / _events_*,      deviations, which the pipeline's one sstdev over all samples cannot tell apart; PG_DMODEL_EVENTS)
 * pg_model_events
 *
 * Pools of dump files -- several files read as one, `cat F1 F2 ... | tr | tail | datamash` -- have one too:
 * pg_pool_create / _destroy        (no counterpart)
 * pg_pool_submit                   the same parse; every file carries one group per labeling
 * pg_pool_finish / _format         datamash median / sstdev of every group's files concatenated        scripts/poregen.sh:73-74
 * pg_pool_sync / _last_error /     (no counterpart)
 * _refusal
 *
 * STEP 7 of the same script, the raw model to the final model file, is one host-only call:
 * pg_transform_model               apply_transformation and set_stddev: echo | bc -l per row, datamash min max, cut | paste
 *                                                                                  scripts/poregen.sh:87-148
 * pg_transform_free                (no counterpart)
 *
 * Whether a model is any good (the reference asks other tools: scripts/eventaling.sh runs f5c eventalign, scripts/sim.sh squigulator and a
 * basecaller) is answered by a handle of its own:
 * pg_fit_create / _destroy /        (no counterpart)
 * _last_error / _set_stream
 * pg_fit_parse_model               a model file as `poregen transform` writes it -> levels in 1e-3 pA
 * pg_fit_set_model / _submit /     per read sample = shift + scale * level over the basecaller's segmentation, then per k-mer how far
 * _finish / _residuals / _pass_ms  its samples lie from the level the model claims
 * pg_fit_calibrate                 the per-read line alone, left on the device as the collector's per-read center and spread
 *                                  (nanopolish, f5c and uncalled4 calibrate each read to the current model before they collect)
 * pg_set_read_scaling              hands a batch's center / spread / use to a pg_params.scaling == PG_SCALING_PER_READ collector
 *
 * The reference's `realign` command (src/main.c; src/realign.cpp is a copy of reform that aligns nothing) is a handle that does align:
 * pg_realign_create / _destroy /   (no counterpart)
 * _last_error / _set_stream
 * pg_realign_set_model / _submit / the move table's boundaries moved within a band to where the samples fit the model's levels best
 * _kernel_ms / _walk
 *
 * The reference's own evaluation of a finished model, scripts/eventaling.sh (f5c eventalign --kmer-model), as the project's own rule:
 * pg_evalign_create / _destroy /   (no counterpart)
 * _last_error / _set_stream
 * pg_evalign_set_model / _submit / one row per event that fit counts: its place, level and spread in the model's units, the model's
 * _copy_text / _kernel_ms / _walk  level and level_stdv for its k-mer, the standardized level; nanopolish / f5c eventalign columns
 * / _walk_gapped / _row_text
 *
 * The generative direction (scripts/sim.sh asks squigulator; the rule here is the project's own, fit's inverted):
 * pg_sim_create / _destroy /        (no counterpart)
 * _last_error / _set_stream / _stream
 * pg_sim_parse_model / _parse_dwell a model file with its level_stdv column, the file `poregen model --dwell_model` writes
 * pg_sim_set_model / _generate /    k-mer model + sequences -> raw signal + the ops that are true by construction, laid out as a pg_batch
 * _kernel_ms / _walk
 *
 * The writing side of the svb-zd signal blocks pg_sigdec_* reads (slow5lib's svb-zd press on the host):
 * pg_sigenc_create / _destroy /     (no counterpart)
 * _last_error / _set_stream / _stream
 * pg_sigenc_bound / _encode /       int16 samples on the device -> the shortest svb-zd block of every read, back to back
 * _kernel_ms
 */
#ifndef PGMOVE_H
#define PGMOVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t pg_status;
enum {
    PG_OK = 0,
    PG_ERR_NO_DEVICE = -1,    /* no usable HIP device / HIP runtime error at create */
    PG_ERR_INVALID_ARG = -2,  /* bad parameter or malformed batch layout */
    PG_ERR_INPUT = -3,        /* a read is outside the reference's defined behaviour (see pg_last_error) */
    PG_ERR_RNA_FLAG = -4,     /* RNA-oriented record without allow_rna (src/gmove.cpp:795-797) */
    PG_ERR_HIP = -5,          /* HIP runtime failure */
    PG_ERR_STATE = -6,        /* calls made in the wrong order */
    PG_ERR_UNSUPPORTED = -7   /* valid input this build cannot process (reported, never silently wrong) */
};

enum { PG_LOC_HOST = 0, PG_LOC_DEVICE = 1 };

/* pg_params.flags */
enum {
    PG_FLAG_LAZY_STATS = 1u << 0, /* compute median/MAD only for reads that contribute a kept event
                                     (legal: event acceptance is signal-independent in the PAF path);
                                     default (eager) is to compute them for every read of the batch, with one exception: a
                                     pg_submit batch that is counted front first (pg_kernel_stats: front_complete) and whose front
                                     completes every k-mer starts its statistics behind the front's scan and leaves out the reads
                                     behind the last one that can own a kept event -- the reference does not touch the reads behind
                                     the completing one either (gmove.cpp:733-735). Their d_med / d_mad are NaN, no result changes.
                                     A read with an unusable calibration fails the batch wherever it lies; reads long enough to be
                                     cut into slices are always computed. Not with PG_FLAG_SKIP_OUT_OF_RANGE or PG_FLAG_PROFILE. */
    PG_FLAG_PROFILE = 1u << 1,    /* record HIP events around every kernel (pg_kernel_stats). Each kernel is timed over the WHOLE
                                     batch: a profiling context never leaves reads out of the statistics (see PG_FLAG_LAZY_STATS),
                                     so bytes of the batch / time of k_read_stats (bench.py's roofline object) means what it says */
    PG_FLAG_ONE_STREAM = 1u << 10, /* every kernel of a batch on ONE stream. Since round 3 the DEFAULT is the two-stream mode below
                                     (PG_FLAG_OVERLAP) whenever the context computes eager statistics and none of PG_FLAG_PROFILE /
                                     _LAZY_STATS / _SKIP_OUT_OF_RANGE / _DEFER_STATS / _OVERLAP_TAIL is set: batches that follow each other
                                     run 14-17 % faster (0.161 -> 0.139 ms per 50 000-read batch). This flag keeps the one-stream form:
                                     short jobs (a hardware queue takes 15-20 ms to create: the CLI sets it), clean per-kernel timings.
                                     Both flags are defaults PER BATCH since round 10: see PG_FLAG_OVERLAP. */
    PG_FLAG_OVERLAP = 1u << 2,    /* two-stream mode, THE DEFAULT since round 3 (see PG_FLAG_ONE_STREAM for when it applies): the statistics
                                     kernels of batch i+1 run on a second stream next to the event / rank / emit chain of batches i and
                                     i+1; that stream is created with a quarter of the compute units (of every XCD) withheld, so that the
                                     chain's workgroups find room. Pays when batches follow each other (configs[1]: 0.162 -> 0.141 ms per
                                     batch). Every kernel then shares the chip: per-kernel timings (PG_FLAG_PROFILE, bench.py's roofline
                                     object) are taken on one stream. Setting the flag explicitly asks for the mode where it is not the
                                     default. The gather stays on the chain's stream (beside the chain of batch i+1 it was worth 0-5 %,
                                     profiles/r04_side_gather.txt).
                                     Since round 10 the mode is a default PER BATCH: the flag gives the context its second stream, and a
                                     pg_submit batch whose statistics are ordered behind the front's scan (see PG_FLAG_LAZY_STATS) is
                                     queued on the chain's stream alone, exactly as a PG_FLAG_ONE_STREAM context queues it -- behind a
                                     complete front there is too little left to overlap (pg_kernel_stats: front_one_stream;
                                     PGMOVE_FRONT_TWO_STREAMS=1 keeps such batches on two streams: tests, A/B). Every other batch of the
                                     context uses both streams as before. No result depends on the mode.
                                     A batch whose statistics stand on the chain's stream behind the front's scan (this one, and the
                                     same batch of a PG_FLAG_ONE_STREAM context) queues them in the launch of the rank emit kernel:
                                     one launch, workgroups of two kinds that share nothing (pg_kernel_stats: emit_stats_fused;
                                     PGMOVE_NO_EMIT_STATS=1, read per batch, keeps the two launches: tests, A/B). */
    PG_FLAG_SHORT_READS_OK = 1u << 4, /* a read with fewer than k matched bases simply has no events (move-table front-end,
                                        where that is well defined); default: PG_ERR_INPUT, because the PAF path of the
                                        reference has undefined behaviour there (src/gmove.cpp:891) */
    PG_FLAG_SKIP_OUT_OF_RANGE = 1u << 5, /* a read with ANY sample outside [pa_min, pa_max] is skipped as a whole instead of
                                           zero-filling the sample: the SAM/BAM front-end (src/gmove.cpp:1149-1160). Event
                                           acceptance then depends on the signal, so the statistics pass runs first. */
    PG_FLAG_DEBUG_NARROW = 1u << 3, /* tests: shrink the exact MAD candidate window to one code so that the fallback search runs */
    PG_FLAG_OVERLAP_TAIL = 1u << 9, /* the statistics of a batch on a second stream, forked BEHIND the walk and the counting kernels:
                                     * the small launches of pg_collect (sample_limit cut, emit, offset scan) run next to the
                                     * streaming kernel; the streams join in front of the gather. Ignored with PG_FLAG_LAZY_STATS,
                                     * PG_FLAG_SKIP_OUT_OF_RANGE, PG_FLAG_OVERLAP and PG_FLAG_DEFER_STATS. */
    PG_FLAG_DEBUG_SPLIT_WALK = 1u << 8, /* tests / measurement: every read takes the generic wave-per-read walk (k_walk), also the reads of
                                        * matches only that the op-parallel event kernel (k_events) would handle */
    PG_FLAG_DEFER_STATS = 1u << 7, /* multi-GPU step: pg_count does not queue the per-read statistics (median/MAD of every read, which
                                     * do not depend on the exchange); pg_stats queues them -- between the ISSUE of the caller's
                                     * collective and the wait for it, so that the all_gather's latency hides behind the streaming
                                     * kernel -- or, if pg_stats is not called, pg_collect does. Ignored with PG_FLAG_LAZY_STATS,
                                     * PG_FLAG_SKIP_OUT_OF_RANGE and PG_FLAG_OVERLAP (their statistics are placed already). */
    PG_FLAG_STOP_WHEN_FULL = 1u << 6 /* the slots are the WHOLE k-mer list: the reference stops reading PAF lines once every k-mer is
                                     * complete (src/gmove.cpp:733-735), so a read behind the one that completes the last k-mer
                                     * is never looked at and cannot fail the job. With this flag a per-read input error is
                                     * reported only if the reference would have reached that read. Without it (a slice of the
                                     * list: the reference reads every line) every read of every batch counts. */
};

typedef struct pg_ctx pg_ctx;

/* Mirrors the gmove-relevant members of opt_t (src/poregen.h:48-79). */
typedef struct {
    uint32_t struct_size;         /* sizeof(pg_params), for ABI evolution */
    uint32_t kmer_size;           /* -k                       default 9 */
    uint32_t sig_move_offset;     /* -m                       default 0; must be <= kmer_size */
    uint32_t signal_print_margin; /* --margin                 default 0 */
    uint32_t sample_limit;        /* --sample_limit           default 100 */
    uint32_t max_dur;             /* --max_dur                default 70 */
    uint32_t min_dur;             /* --min_dur                default 5 */
    int32_t  kmer_pick_margin;    /* --kmer_pick_margin       default 2; must be >= 0 */
    int32_t  scaling;             /* --scaling: 0 none, 1 med-MAD (effective default 0), PG_SCALING_PER_READ: pg_set_read_scaling */
    int32_t  allow_rna;           /* --rna */
    double   pa_min;              /* --pa_min                 default 40.0 */
    double   pa_max;              /* --pa_max                 default 180.0 */
    uint32_t n_slots;             /* number of k-mers in the slice [index_start, index_end] */
    uint32_t flags;               /* PG_FLAG_* */
    int32_t  device;              /* HIP device ordinal */
    int32_t  reserved;
    /* code -> slot tables, int32[4^k], host memory, copied at pg_create; -1 = k-mer not in the slice.
     * The code of a k-mer is its base-4 value, first base most significant, A=0 C=1 G=2 T/U=3.
     * table_t is used for DNA-oriented records (sequence spelled with T), table_u for RNA-oriented
     * records (T->U applied, src/gmove.cpp:815-817). pg_build_slot_tables fills both. */
    const int32_t *table_t;
    const int32_t *table_u;
} pg_params;

/* One batch of reads in PAF line order, structure-of-arrays. All arrays are caller-owned. LIFETIME: pg_count / pg_submit
 * return with work still queued -- a device batch is read by kernels queued behind the call, a host batch is staged with
 * asynchronous copies out of the caller's memory -- so the arrays must stay valid and unmodified until pg_sync (or pg_finish /
 * pg_all_slots_full / the next pg_count / pg_submit on the context, which synchronise) has returned. `location` says whether
 * every pointer is a host or a device pointer (device pointers must belong to pg_params.device). sig must be 16-byte aligned.
 * A device batch must be complete on the context's stream (pg_set_stream) before the call, or be produced on that stream.
 *
 * Read r:  signal   sig[sig_off[r] .. sig_off[r+1])               slow5_rec_t.raw_signal
 *          digitisation/offset/range[r]                            slow5_rec_t fields
 *          query_start[r], target_start[r], target_end[r]          PAF columns 3, 8, 9
 *          seq[seq_off[r] .. seq_off[r+1])  = faidx_fetch_seq(tid, min(ts,te), max(ts,te)-1) as
 *                                             fetched (ASCII, no T->U); empty if the name is absent
 *          ss ops  op_n/op_t[op_off[r] .. op_off[r+1]): op_t 0=',' (match) 1='I' 2='D'
 */
typedef struct {
    uint32_t struct_size;
    int32_t  location;
    uint32_t n_reads;
    uint32_t n_ops;               /* device batches: op_off[n_reads] if the caller knows it (it sizes the work buffers without a
                                   * round trip to the device); 0 = the library reads it back (one synchronisation of the
                                   * context's stream per call). A wrong value is detected on the device and fails the batch
                                   * with PG_ERR_INVALID_ARG; no kernel touches memory behind n_ops. Host batches: ignored. */
    const int16_t  *sig;
    const uint64_t *sig_off;      /* [n_reads+1] */
    const double   *digitisation; /* [n_reads] */
    const double   *offset;
    const double   *range;
    const int32_t  *query_start;
    const int32_t  *target_start;
    const int32_t  *target_end;
    const uint8_t  *seq;
    const uint64_t *seq_off;      /* [n_reads+1] */
    const uint32_t *op_n;
    const uint8_t  *op_t;
    const uint64_t *op_off;       /* [n_reads+1] */
    uint32_t flags;               /* PG_BATCH_* */
    uint32_t reserved;
} pg_batch;
/* pg_batch.flags */
enum {
    PG_BATCH_ALL_MATCHES = 1u << 0 /* the caller vouches that every ss op of the batch is a match (what `reform` writes): the generic
                                    * wave-per-read walk is not launched at all. Verified on the device: a batch that holds an I, a D or
                                    * an unknown op after all fails with PG_ERR_INVALID_ARG (never a wrong result). */
    ,
    PG_BATCH_RESIDENT = 1u << 1    /* device batches of a context that runs on the CALLER's stream (pg_set_stream): the batch's arrays are complete
                                    * -- nothing queued on that stream produces them (a shard uploaded once and synchronised, as in a multi-GPU
                                    * job's steady state). Without it the statistics stream waits for everything the caller's stream holds in
                                    * front of pg_count, which includes the previous batch's gather: the statistics of a batch then start a whole
                                    * chain later than on the context's own stream (156 -> 13x us per step of the one-rank RCCL step). */
    ,
    PG_BATCH_GAPPED = 1u << 2      /* pg_fit_submit and pg_realign_submit: the ops are the signal-to-reference alignment -- op_t 0 (match), 1 (I) or
                                    * 2 (D) -- and seq / seq_off hold every read's reference slice, as pg_mvops_project and pg_refseq leave them.
                                    * Not together with PG_BATCH_ALL_MATCHES (PG_ERR_INVALID_ARG). The collector (pg_submit) ignores it. */
};

/* Host-side view of everything collected so far, in reference order: for slot s, its kept events are
 * e in [ev_off[s], ev_off[s+1]); event e has ev_len[e] samples at samples[samp_off[e] ..], and came
 * from read ev_read[e] (0-based index over all reads submitted to this context, in order).
 * Memory is owned by the context and valid until the next pg_submit/pg_collect/pg_reset/pg_destroy. */
typedef struct {
    uint32_t n_slots;
    uint32_t reserved;
    uint64_t n_events;
    uint64_t n_samples;
    uint64_t n_reads;             /* reads submitted so far */
    const uint64_t *counts;       /* [n_slots]   freq.txt values (<= sample_limit) */
    const uint64_t *ev_off;       /* [n_slots+1] */
    const uint32_t *ev_len;       /* [n_events]  */
    const uint32_t *ev_read;      /* [n_events]  */
    const uint64_t *samp_off;     /* [n_events+1] */
    const double   *samples;      /* [n_samples] */
    const uint8_t  *read_skipped; /* [n_reads] 1 = silently skipped (fetched length < k, gmove.cpp:806-808) */
} pg_result;

typedef struct {
    const char *name;     /* kernel name */
    uint64_t launches;
    double   total_ms;    /* HIP-event time on the launching stream */
} pg_kernel_stat;

void        pg_default_params(pg_params *p);
const char *pg_last_error(const pg_ctx *ctx); /* ctx may be NULL: error of the last failed pg_create */
const char *pg_version(void);

/* Fill int32[4^k] tables from the slice's k-mer strings (slot i = kmers[i]). K-mers containing
 * characters outside ACGTU, or both T and U, can never equal a fetched window and get no entry.
 * Returns PG_ERR_INVALID_ARG on duplicate k-mers or k > 13. */
pg_status pg_build_slot_tables(uint32_t kmer_size, const char *const *kmers, uint32_t n_slots,
                               int32_t *table_t, int32_t *table_u);

/* Brings the HIP runtime up on `device` (the first call in a process takes 0.1-0.2 s): a host that has other start-up work -- file
 * indices, parsing -- calls this on a thread of its own first; pg_create afterwards finds the runtime ready. Optional. */
pg_status pg_runtime_init(int32_t device);
pg_status pg_create(const pg_params *params, pg_ctx **out);
void      pg_destroy(pg_ctx *ctx);
pg_status pg_reset(pg_ctx *ctx); /* forget all reads/events, keep parameters and buffers */

/* count + collect with base = events accepted by earlier batches of this context */
pg_status pg_submit(pg_ctx *ctx, const pg_batch *batch);

/* pg_params.scaling == PG_SCALING_PER_READ: every batch brings a center, a spread and a use flag per read (pg_fit_calibrate computes
 * them), and the collector stores (pA - center[r]) / spread[r] per sample: one subtraction, one division, as med-MAD's (x - median) / MAD.
 * A sample whose pA lies outside [pa_min, pa_max] is zeroed first, as for med-MAD (gmove.cpp:756-759, 774): it is stored as
 * (0 - center) / spread. A read with use == 0 contributes no event; it is reported as a read with an out-of-range sample is under
 * PG_FLAG_SKIP_OUT_OF_RANGE: pg_result.read_skipped is 1, and it fails nothing. A read with use != 0 whose spread is not a finite non-zero
 * number or whose center is not finite fails the batch with PG_ERR_INVALID_ARG; the error names the lowest such read.
 * The arrays ([n_reads] of the NEXT pg_count / pg_submit only, host or device memory by `location`, with the lifetime of that batch's
 * arrays; NULL only for a batch of no reads) are consumed by that call; it waits for the one word that says whether a read was refused. PG_ERR_STATE: a batch of such a
 * context without this call in front, and this call on a context of any other scaling. pg_create refuses the scaling together with
 * PG_FLAG_SKIP_OUT_OF_RANGE (both own the per-read skip array); pg_job_create refuses it with PG_ERR_UNSUPPORTED. No per-read statistics
 * are computed; pg_device_view.d_med / d_mad show center and spread. */
enum { PG_SCALING_PER_READ = 2 };
pg_status pg_set_read_scaling(pg_ctx *ctx, const double *center, const double *spread, const uint8_t *use, int32_t location);

/* Phase 1: walk/filter/rank one batch; writes the batch's accepted-event count per slot (uncapped)
 * to counts_out (uint64[n_slots]) in host or device memory. */
pg_status pg_count(pg_ctx *ctx, const pg_batch *batch, uint64_t *counts_out, int32_t counts_location);
/* Phase 2: keep the events whose rank (base[slot] + rank inside the batch) is < sample_limit and
 * gather their windows. base = uint64[n_slots], number of accepted events that precede this batch in
 * reference order (earlier batches, lower ranks of a multi-GPU job); NULL = the context's own running
 * count. The batch pointers given to pg_count must still be valid. */
pg_status pg_collect(pg_ctx *ctx, const uint64_t *base, int32_t base_location);
/* Between pg_count and pg_collect of a context created with PG_FLAG_DEFER_STATS: queue the statistics of the counted batch
 * (src/gmove.cpp:754-771 for every read) on the context's stream now. A no-op when nothing was deferred. */
pg_status pg_stats(pg_ctx *ctx);
/* Phase 2 of a multi-GPU job, straight from the all-gather: all_counts = uint64[world][n_slots] in DEVICE memory, row g =
 * pg_count's output of rank g (the receive buffer of the all_gather). base = sum of the rows below `rank`, computed on
 * the device on the context's stream: the step needs no host arithmetic and no extra kernels of the caller.
 * Replaces nothing in the reference (which is single-process); the order semantics are those of pg_collect. */
pg_status pg_collect_gathered(pg_ctx *ctx, const uint64_t *all_counts, uint32_t world, uint32_t rank);

/* After pg_collect_gathered: device pointers (uint64[n_slots], stable for the life of the context, contents rewritten by
 * every pg_collect_gathered on the context's stream) to the accepted events of ALL ranks per slot and to the job's freq.txt
 * values min(total, sample_limit) (src/gmove.cpp:945-953, 523-534) -- produced by the kernel that sums the lower ranks' rows,
 * so a multi-GPU step needs no reduction of its own. Either output pointer may be NULL. */
pg_status pg_job_totals_device(pg_ctx *ctx, const uint64_t **d_total, const uint64_t **d_freq);

pg_status pg_sync(pg_ctx *ctx);                      /* wait for all device work of the context */
/* Run the context's main chain on a caller-owned HIP stream (hipStream_t passed as void*), e.g. PyTorch's current
 * stream, so that collectives issued by the caller between pg_count and pg_collect are ordered without host
 * synchronisation. NULL restores the context's own stream. */
pg_status pg_set_stream(pg_ctx *ctx, void *hip_stream);
pg_status pg_finish(pg_ctx *ctx, pg_result *out);     /* sync, copy results to host, merge batches */
/* pg_finish without the samples' trip to the host: every array of pg_result is filled except `samples` (NULL whenever the kept samples
 * are still on the device: one batch, or several merged there). pg_fetch_samples then copies any range [first, first + n) of the
 * job's k-mer-major sample stream (the indices samp_off counts in) into a host buffer of the caller's; after pg_finish_deferred it
 * may be called from SEVERAL host threads at once, so that a writer formats and writes one k-mer range while the next one is on its
 * way -- the reference prints as it goes (src/gmove.cpp:938-944); the CLI's dump writers do this. Valid until the next
 * pg_submit / pg_count / pg_reset. A later pg_finish still hands the samples out as a whole. */
pg_status pg_finish_deferred(pg_ctx *ctx, pg_result *out);
pg_status pg_fetch_samples(pg_ctx *ctx, uint64_t first, uint64_t n, double *dst);

/* The dump files' TEXT, produced on the device: for every slot the bytes the reference's fprintf calls write into dump/<KMER> --
 * "%.8f," per sample, "%.8f;" for an event's last one (src/gmove.cpp:938-944) -- as one buffer in HBM, slot after slot; slot s is
 * bytes [slot_off[s], slot_off[s+1]). Without -d only (the ':' of src/gmove.cpp:960-962 depend on the reads: a host job). The digits
 * are printf's (correctly rounded, ties to even on the binary value). PG_ERR_UNSUPPORTED -- never a wrong digit -- if a kept sample is
 * not finite or |sample| >= 4e7, or if the samples of several batches had to be merged on the host: format there (pg_finish).
 * Calls pg_finish_deferred first; pg_fetch_text copies a byte range to the host and may be called from several threads at once.
 * Valid until the next pg_submit / pg_count / pg_reset / pg_text. */
typedef struct {
    uint32_t n_slots, reserved;
    uint64_t n_bytes;
    const uint64_t *slot_off; /* [n_slots + 1], host memory owned by the context */
} pg_text_result;
pg_status pg_text(pg_ctx *ctx, pg_text_result *out);
pg_status pg_fetch_text(pg_ctx *ctx, uint64_t first, uint64_t n, char *dst);
/* The same from DEVICE arrays in pg_result layout (what pg_last_batch_device or poregen_amd.dist.gather_kept hand out; pg_job_text's
 * merged view): n_events kept events, d_ev_off[n_slots + 1], d_samp_off[n_events + 1], d_samples on pg_params.device. The text is the
 * context's (pg_fetch_text), the arrays stay the caller's. */
pg_status pg_text_device(pg_ctx *ctx, uint32_t n_slots, uint64_t n_events, const uint64_t *d_ev_off, const uint64_t *d_samp_off,
                         const double *d_samples, pg_text_result *out);
int32_t   pg_all_slots_full(pg_ctx *ctx);            /* 1 when every slot holds sample_limit events (waits for the device) */
/* The same as of the last batch the context has already waited for (pg_submit / pg_count wait for the PREVIOUS batch): no wait.
 * A host that parses batch i+1 while batch i is on the device asks this after submitting i+1 and learns about batch i. */
int32_t   pg_all_slots_full_settled(const pg_ctx *ctx);
/* Has the device finished the last submitted batch? 1 = yes (the batch is then settled: its per-read errors are returned as a
 * negative pg_status, pg_all_slots_full_settled speaks about it), 0 = still running. Never waits. */
int32_t   pg_poll(pg_ctx *ctx);

/* device-resident view of the LAST collected batch (for callers that keep results on the GPU) */
typedef struct {
    uint64_t n_events, n_samples;
    const uint64_t *d_keep;     /* [n_slots] kept events of this batch per slot */
    const uint64_t *d_ev_off;   /* [n_slots+1] */
    const uint32_t *d_ev_len;
    const uint32_t *d_ev_read;  /* read index inside the batch */
    const uint64_t *d_samp_off;
    const double   *d_samples;
    const double   *d_med;      /* [n_reads] (scaling==1; scaling 2: the read's center and spread; NaN where not computed: reads without a kept event under PG_FLAG_LAZY_STATS, */
    const double   *d_mad;      /* and the reads from the cut read on behind a complete front: PG_FLAG_LAZY_STATS, stats_cut_batches) */
} pg_device_view;
pg_status pg_last_batch_device(pg_ctx *ctx, pg_device_view *out);

/* Per-k-mer model over everything collected so far, computed on the device from the kept samples: what the
 * reference's pipeline gets by reading the dump files back as text (scripts/poregen.sh:54-85: `tr ';,' '\n' < file |
 * tail -n +2 | datamash median 1` and `... | datamash sstdev 1`; :33-52: awk comma counts | datamash median).
 * The values are those of the "%.8f" TEXT gmove writes (src/gmove.cpp:941-944), i.e. integers of 1e-8 units:
 *   - the first value of every file is dropped (`tail -n +2`) unless PG_MODEL_KEEP_FIRST is given;
 *   - median = datamash's: middle value, or the mean of the two middle values;  sstdev = sqrt(sum (x-mean)^2/(n-1));
 *   - dwell  = median over the file's ';'-separated fields of the number of commas: samples-1 per event, plus one 0
 *     for the empty field behind the last ';' (files without events have no fields at all).
 * Calls pg_finish first. Arrays are owned by the context, valid until the next pg_model/pg_reset/pg_destroy.
 * PG_ERR_UNSUPPORTED (never a wrong number) if a slot holds a non-finite sample or |sample| >= 4e7, more than 2^23
 * values, or values further than 2^40 units (10995.1 pA) from its first one. */
enum { PG_MODEL_KEEP_FIRST = 1u << 0 };
typedef struct {
    uint32_t n_slots;
    uint32_t flags;
    const uint64_t *n_values;     /* [n_slots] values that count (0: the fields below are NaN / 0) */
    const double   *median;       /* [n_slots] */
    const double   *sstdev;       /* [n_slots] NaN when n_values < 2 */
    const int64_t  *mid_lo;       /* [n_slots] the two middle order statistics, exact, in 1e-8 units */
    const int64_t  *mid_hi;
    const int64_t  *origin;       /* [n_slots] exact moments of d = value - origin (1e-8 units): */
    const int64_t  *sum1;         /*           sum d                                              */
    const uint64_t *sum2_lo;      /*           sum d*d, low and high 64 bits                      */
    const uint64_t *sum2_hi;
    const uint64_t *dwell_n;      /* [n_slots] fields awk sees (kept events + 1), 0 for an empty file */
    const double   *dwell_median; /* [n_slots] */
} pg_model_result;
enum { PG_MODEL_TEXT_MEDIAN = 0, PG_MODEL_TEXT_SSTDEV = 1, PG_MODEL_TEXT_DWELL = 2 };
pg_status pg_model(pg_ctx *ctx, uint32_t flags, pg_model_result *out);
/* The same reduction over caller-owned DEVICE arrays in pg_result layout: ev_off uint64[n_slots+1], samp_off
 * uint64[ev_off[n_slots]+1], ev_len uint32[], samples double[] -- e.g. the kept events of all ranks of a multi-GPU job
 * brought together on the writing rank (poregen_amd/dist.py gather_kept). Uses the context's stream and result buffers;
 * the arrays must be complete before the call (no ordering with other streams is implied). */
pg_status pg_model_device(pg_ctx *ctx, uint32_t n_slots, const uint64_t *d_ev_off, const uint64_t *d_samp_off,
                          const uint32_t *d_ev_len, const double *d_samples, uint32_t flags, pg_model_result *out);
/* The number as datamash prints it ("%.14Lg" of its long double; "nan" for sstdev of one value; empty string when the
 * slot has no value at all, like datamash on empty input). Returns the length written (excluding the NUL), 0 on error.
 * Caveat (parity of this call is UNPINNED: datamash is not in the image): the 14 digits of the sample standard deviation are
 * decided here in exact integer arithmetic on the "%.8f" values. datamash rounds a long double that it computed with rounded
 * intermediate sums; on a file whose exact sstdev lies within a few 1e-19 (relative) of a 14th-digit rounding boundary -- the
 * fuzzer found one 5e-9 of a 14th-digit unit below it -- the real pipeline (scripts/poregen.sh:54-85) may print the neighbouring
 * digit. Undecidable without datamash; the exact value is what this returns. */
size_t pg_model_format(const pg_model_result *m, uint32_t slot, int32_t which, char *buf, size_t cap);

/* ---- one job over several GPUs of one node, driven from ONE host process ---------------------------------------------
 * The reference is a single process (src/main.c:64-103 -> gmove(), src/gmove.cpp:213) whose only parallel driver is
 * work_db (src/thread.c:119-132: a batch split over worker threads, each working a contiguous range); pg_job is that
 * shape with GPUs as the workers, at the same seam as pg_submit (src/gmove.cpp:515, 732-969): a batch's reads are cut into
 * n contiguous PAF-ordered shards, device i works shard i on its own host thread, and the "count == sample_limit" test
 * (src/gmove.cpp:925-927) is resolved by ONE exchange per batch -- an ncclAllGather (RCCL over xGMI) of every shard's
 * uint64[n_slots] accepted-event counts, in place in each device's receive buffer, whose rows below a shard (plus the
 * running total of the earlier batches, kept as row 0 of the same buffer) are its base (pg_collect_gathered). The per-read
 * statistics are queued behind the issue of the collective and hide it. pg_job_finish returns the job's per-k-mer streams
 * in reference order (slot, then batch, then shard): byte for byte what one context fed the same batches returns.
 * pg_job_submit takes a host batch and cuts it; pg_job_submit_shards takes one batch per device, host or device-resident. A device may be listed more than once (several shards on one GPU); the exchange then goes through
 * host memory (RCCL needs distinct devices), as it does when librccl cannot be loaded and PG_JOB_EXCHANGE_RCCL is not set. */
typedef struct pg_job pg_job;
enum {
    PG_JOB_EXCHANGE_AUTO = 0, /* RCCL when the listed devices are distinct and librccl loads, else through the host */
    PG_JOB_EXCHANGE_HOST = 1, /* always through host memory */
    PG_JOB_EXCHANGE_RCCL = 2  /* always RCCL: pg_job_create fails when it is unavailable or a device is listed twice */
};
/* params->device is ignored (devices[] decides); params->flags as for pg_create (PG_FLAG_DEFER_STATS is added). */
pg_status   pg_job_create(const pg_params *params, const int32_t *devices, uint32_t n_devices, uint32_t exchange, pg_job **out);
void        pg_job_destroy(pg_job *job);
const char *pg_job_last_error(const pg_job *job);       /* job may be NULL: error of the last failed pg_job_create */
/* Queues the whole batch on all devices and returns; the batch arrays must stay valid until pg_job_sync / the next
 * pg_job_submit / pg_job_finish has returned (see pg_batch). */
pg_status   pg_job_submit(pg_job *job, const pg_batch *host_batch);
/* The same step for shards that already are where they will be worked: shards[g] (g < n_devices, in PAF order) is rank g's part of the
 * batch as a pg_batch of its own -- PG_LOC_DEVICE arrays resident on devices[g] and complete before the call, or PG_LOC_HOST. Nothing is
 * cut or copied on the host and, with device shards, nothing crosses PCIe inside the step: a device-resident N-GPU step driven from the
 * C++ host (src/gmove.cpp:732-969 over N devices; lifetime of the arrays as pg_job_submit). Results: those of pg_job_submit on the
 * concatenation of the shards. A PG_LOC_DEVICE shard whose sig / sig_off / op_n / seq are not device memory on devices[g] is refused with
 * PG_ERR_INVALID_ARG (hipPointerGetAttributes, once per array and call) before anything is launched on it.
 * Where a rank's statistics are queued relative to the count exchange is a PROVISIONAL rule (csrc/pg_job_rule.h; no run on more than one
 * GPU exists yet): PGMOVE_JOB_STATS_RULE=front|behind|auto in the environment overrides it; results never depend on it. */
pg_status   pg_job_submit_shards(pg_job *job, const pg_batch *shards, uint32_t n_shards);
pg_status   pg_job_reset(pg_job *job);                  /* as pg_reset: the next submit starts a new job on the same devices and communicators */
pg_status   pg_job_sync(pg_job *job);                   /* wait for every device; surfaces per-read errors (lowest shard first) */
int32_t     pg_job_all_slots_full(pg_job *job);         /* src/gmove.cpp:733-735 for the job */
int32_t     pg_job_all_slots_full_settled(const pg_job *job); /* as pg_all_slots_full_settled */
int32_t     pg_job_poll(pg_job *job);                    /* as pg_poll, for every device of the job */
pg_status   pg_job_finish(pg_job *job, pg_result *out); /* merged view, owned by the job until the next submit / destroy */
/* As pg_finish_deferred / pg_fetch_samples / pg_text / pg_fetch_text for the job. The shards' kept samples are concatenated ON THE
 * JOB'S FIRST DEVICE -- one peer copy per shard that sits on another device (xGMI), one launch of (k-mer, batch, shard) segment copies:
 * north_star's "concatenate the buffers over xGMI" -- and stay there: pg_job_finish_deferred returns everything but `samples` (NULL),
 * pg_job_fetch_samples copies any range of the merged stream to the host (callable from several threads at once), pg_job_text
 * produces the dump files' bytes from it on that device (PG_ERR_UNSUPPORTED as pg_text), pg_job_model reduces it there.
 * pg_job_finish = the same merge + ONE download. (A shard whose own batches had to be merged on the host sends the job through the
 * host merge instead; the results are the same.) */
pg_status   pg_job_finish_deferred(pg_job *job, pg_result *out);
pg_status   pg_job_fetch_samples(pg_job *job, uint64_t first, uint64_t n, double *dst);
pg_status   pg_job_text(pg_job *job, pg_text_result *out);
pg_status   pg_job_fetch_text(pg_job *job, uint64_t first, uint64_t n, char *dst);
/* 1 when the last pg_job_create chose RCCL for this job's exchange, 0 = host memory */
int32_t     pg_job_uses_rccl(const pg_job *job);
/* The k-mer model of the whole job (see pg_model): the merged kept samples are reduced on the job's first device. */
pg_status   pg_job_model(pg_job *job, uint32_t flags, pg_model_result *out);
/* pg_kernel_stats of one shard's context (PG_FLAG_PROFILE in the job's params): what a rank-level early-out skipped shows up here */
pg_status   pg_job_kernel_stats(pg_job *job, uint32_t shard, pg_kernel_stat *out, uint32_t cap, uint32_t *n_out);

/* profiling (PG_FLAG_PROFILE): per-kernel launch counts and HIP-event times since the last reset. With or without the flag, counters
 * follow as entries of 0 ms when they are not 0: stats_cancelled_on_device, long_reads_split, long_helpers_short_batches,
 * front_complete / front_missed (settled pg_submit batches whose events were counted front first: the first tiles completed every k-mer and
 * the tiles behind them were not walked / did not, and were; PGMOVE_FRONT_TILES=n sets the front in tiles of 4096 ops, 0 = never),
 * stats_cut_batches / stats_cut_reads (those of the front_complete batches whose eager statistics were ordered behind the front's scan, and
 * the reads from their cut reads on, whose samples the statistics did not touch: PG_FLAG_LAZY_STATS), front_one_stream (settled batches
 * of a two-stream context that were queued on the chain's stream alone: PG_FLAG_OVERLAP), emit_stats_fused (settled batches whose
 * statistics and rank emit were queued as one launch; 0 with PGMOVE_NO_EMIT_STATS=1 and for every batch that is not front first), and the
 * gathers for many kept events by the kernel queued: gather_form_wave, gather_form_evpair, gather_form_lanes4 / 8 / 16; k_sort_scatter:
 * passes of the LSD radix sort queued (more than 2^20 slots; the entry "sort_events" counts the whole sort once per batch) */
pg_status pg_kernel_stats(pg_ctx *ctx, pg_kernel_stat *out, uint32_t cap, uint32_t *n_out);
pg_status pg_kernel_stats_reset(pg_ctx *ctx);

/* ---- kmer_freq: every k-byte window of every FASTQ sequence line, counted on the device ----------------------------------------
 * The input is the raw FASTQ bytes in pieces cut at ANY byte offset; the line structure is found on the device and the state that
 * crosses a piece boundary stays there. Rules (src/kmer_freq.cpp:160-181): lines as getline returns them, line i is a sequence line
 * iff i % 4 == 1, the last byte of every line (its '\n', or the last byte of an unterminated final line) is dropped, every window of
 * kmer_size bytes of the rest is a key. ACGT windows are counted densely (index = 2-bit codes, A=0 C=1 G=2 T=3, first base most
 * significant: the lexicographic order of the generated keys); any other window is a key of its own bytes ("odd key").
 * A NUL byte in a sequence line is refused: pg_kfreq_finish returns PG_ERR_INPUT. No CPU fallback: PG_ERR_NO_DEVICE without a GPU.
 * A stream (up to the next finish) takes one of three input forms: FASTQ text (pg_kfreq_submit), packed reads (pg_kfreq_submit_reads) or
 * FASTA text (pg_kfreq_submit_fasta). Any mix of them returns PG_ERR_INVALID_ARG and counts nothing. */
typedef struct pg_kfreq pg_kfreq;
typedef struct {
    uint32_t kmer_size;
    uint32_t reserved;
    uint64_t n_odd;              /* keys that are not all ACGT */
    const uint8_t *odd_keys;     /* n_odd * kmer_size bytes, ascending in unsigned byte order (memcmp) */
    const uint64_t *odd_counts;  /* n_odd counts; both arrays owned by the handle until the next finish / destroy */
} pg_kfreq_result;
/* kmer_size in [1,12] (4^12 u64 counters = 128 MiB). The odd-key list takes PGKFREQ_ODD_CAP (default 48 M) 16-byte entries. */
pg_status pg_kfreq_create(uint32_t kmer_size, int32_t device, pg_kfreq **out);
void      pg_kfreq_destroy(pg_kfreq *h);
const char *pg_kfreq_last_error(const pg_kfreq *h); /* h may be NULL: error of the last failed pg_kfreq_create */
/* The next n_bytes of the stream. PG_LOC_HOST: any host memory, free for reuse when the call returns (page-locked memory is copied
 * from directly, other memory through two pinned staging buffers). PG_LOC_DEVICE: memory of the handle's device, complete before the
 * call; it is read in place and must stay unchanged until pg_kfreq_sync or pg_kfreq_finish. */
pg_status pg_kfreq_submit(pg_kfreq *h, const void *data, uint64_t n_bytes, int32_t location);
/* The stream's other input form: n_reads reads as a BAM record stores its sequence, two 4-bit codes per byte ("=ACMGRSVTWYHKDBN",
 * high nibble first). Read r is l_seq[r] bases from byte byte_off[r] of seq_bytes (any offset; reads may lie anywhere in the
 * n_seq_bytes bytes, so a run of whole BAM records can be passed as it is); the low nibble of the last byte of an odd-length read is
 * padding and never read as a base. Each read counts as one FASTQ sequence line: l_seq - kmer_size + 1 windows, none if it is shorter;
 * ACGT windows densely, any other window as an odd key of its letters. reverse[r] != 0: the read is counted as `samtools fastq` prints
 * a record with flag 0x10, bases in reverse order and every code complemented (its four bits reversed: A<->T, C<->G, M<->K, R<->Y,
 * V<->B, H<->D; '=', S, W, N stay). flags: PG_KFREQ_N_TO_T counts code 15 (N) of the printed read as T (sed '2~4s/N/T/g'); other
 * ambiguity codes stay. The result equals pg_kfreq_submit on the FASTQ text of the reads with every line '\n'-terminated.
 * location as for pg_kfreq_submit, for all four arrays; host arrays are free for reuse when the
 * call returns. Long reads are cut into pieces of pg_kfreq_reads_piece(h) windows, one wave of the device each. */
enum { PG_KFREQ_N_TO_T = 1 };
pg_status pg_kfreq_submit_reads(pg_kfreq *h, const uint8_t *seq_bytes, uint64_t n_seq_bytes, const uint64_t *byte_off, const uint32_t *l_seq,
                                const uint8_t *reverse, uint64_t n_reads, uint32_t flags, int32_t location);
uint32_t  pg_kfreq_reads_piece(const pg_kfreq *h);
/* The stream's third input form: the next n_bytes of a FASTA, in pieces cut at ANY byte offset; location and lifetime as for
 * pg_kfreq_submit. Lines end at '\n' and nowhere else (a '\r' is a byte of its line; the last line may be unterminated). A line whose
 * first byte is '>' is a header line, every other line -- an empty one, one with '>' further in -- a sequence line. A record is a
 * maximal run of sequence lines with no header line between them (also in front of the first header; a header followed by a header is
 * an empty record), its sequence those lines' bytes in order without the '\n's, and every window of kmer_size bytes of a record's
 * sequence is a key: windows run across line ends, never across a header. ACGT windows densely, any other window ('N', lower case,
 * '\r', ...) as an odd key of its bytes, as in the FASTQ form. No byte is dropped: the window that ends on the stream's last byte
 * counts (the one difference to the FASTQ form over the same bytes). The result equals pg_kfreq_submit on the FASTQ text
 * "@\n" + sequence + "\n+\n\n" of every record. A NUL byte in a sequence line: PG_ERR_INPUT at finish; header lines are not looked at. */
pg_status pg_kfreq_submit_fasta(pg_kfreq *h, const void *data, uint64_t n_bytes, int32_t location);
pg_status pg_kfreq_sync(pg_kfreq *h);
/* End of stream (FASTQ form: the window ending on its last byte is dropped, the unterminated-final-line rule). counts_out: host u64[4^kmer_size].
 * The handle is reset afterwards, also after an error: the next submit starts a new stream. */
pg_status pg_kfreq_finish(pg_kfreq *h, uint64_t *counts_out, pg_kfreq_result *out);

/* ---- f1_score: per-signal-point agreement of two ss signal alignments, counted on the device ------------------------------------
 * A batch holds n_pairs pairs of ss strings, concatenated: string 2p is side 1 (file 1) of pair p, string 2p+1 side 2; string s is
 * bytes [ss_off[s], ss_off[s + 1]) of ss. Per string: the first signal index (si[0]) and the first reference position (si[2]; side 2
 * with --base_shift added). Per pair (TP, FP, TN, FN) as f1score.py's evaluate_alignments counts them: op "<n>," maps n points to the
 * current ref and steps it by dir (+1, or -1 with rna), "<n>I" maps n points to -1, "<n>D" steps the ref by dir * n, other letters do
 * nothing; over the overlap of the two signal ranges a point counts TN / FP / FN by which ref is -1, then TP if |r1 - r2| <= threshold
 * and FP otherwise; with use_region a point is skipped when region_start > r1 + 1 or region_end < r1 + 1.
 * Refused, PG_ERR_INPUT from pg_fscore_finish with the first failing pair in pg_fscore_result: an empty ss, an ss ending in a digit, a byte
 * >= 0x80, an op count >= 2^32, a side that maps no point. No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_fscore pg_fscore;
typedef struct {
    int32_t rna;              /* dir = -1 */
    int32_t use_region;
    int64_t threshold;
    int64_t region_start, region_end;
} pg_fscore_params;
typedef struct {
    uint64_t n_pairs;
    int32_t location;         /* PG_LOC_HOST or PG_LOC_DEVICE: where ss lies (ss_off / sig_start / first_ref are host arrays) */
    int32_t reserved;
    const uint8_t *ss;
    const uint64_t *ss_off;   /* 2 * n_pairs + 1 non-decreasing offsets */
    const int64_t *sig_start; /* 2 * n_pairs */
    const int64_t *first_ref; /* 2 * n_pairs */
} pg_fscore_batch;
typedef struct {
    uint64_t totals[4];       /* TP, FP, TN, FN over every pair submitted since the last finish */
    uint64_t n_pairs;
    int64_t err_pair;         /* PG_ERR_INPUT: the first failing pair (in submission order), else -1 */
    uint32_t err_code;        /* 1 empty ss, 2 ss ends in a digit, 3 byte >= 0x80, 4 op count >= 2^32, 5 no signal point */
    uint32_t err_side;        /* 0: side 1 (file 1), 1: side 2 */
} pg_fscore_result;
pg_status pg_fscore_create(const pg_fscore_params *params, int32_t device, pg_fscore **out);
void      pg_fscore_destroy(pg_fscore *h);
const char *pg_fscore_last_error(const pg_fscore *h); /* h may be NULL: error of the last failed pg_fscore_create */
/* PG_LOC_HOST ss: any host memory, free for reuse when the call returns. PG_LOC_DEVICE ss: memory of the handle's device, complete
 * before the call, read in place and unchanged until pg_fscore_sync or pg_fscore_finish. Pairs are cut into pieces of at most 32 MiB of ss
 * (a larger pair makes a piece of its own), so device memory stays bounded. */
pg_status pg_fscore_submit(pg_fscore *h, const pg_fscore_batch *batch);
pg_status pg_fscore_sync(pg_fscore *h);
/* totals (and, when pair_counts is set, host u64[4 * min(cap_pairs, n_pairs)] per pair) of every pair since the last finish. The
 * handle is reset afterwards, also after an error. */
pg_status pg_fscore_finish(pg_fscore *h, pg_fscore_result *out, uint64_t *pair_counts, uint64_t cap_pairs);

/* ---- subtool0 / pa_stats: the mean pA of every read, and of every sample of the dataset ------------------------------------------
 * Per read (src/poregen.cpp:133-151, printed by output_db, src/poregen.cpp:166-175, as printf("%s\t%f\n", read_id, mean)): the mean of
 * x_i = ((double)raw_i + offset) * (range / digitisation), which the reference sums SEQUENTIALLY in one double from 0.0. The library
 * returns, for every read with n > 0, a double whose printf("%f") text is the reference's text: the device counts exact integer moments
 * of the samples and settles the text from them where a proven bound allows (csrc/pg_pamean.h); every other read (a mean too near a
 * rounding boundary of %f, a non-finite digitisation / offset / range, a read longer than 2^30 samples) is finished on the host by
 * the reference's own loop. Zero-length reads get NaN (the reference prints nothing for them).
 * Per dataset (scripts/poregen.sh STEP 7, `sigtk pa | datamash mean 1 sstdev 1`): N = sum n, the mean and the sample standard
 * deviation sqrt(sum (x - mean)^2 / (N - 1)) of all pA values, folded in file order from exact per-read integer moments; the result does
 * not depend on how the reads are cut into batches or where they lie. The moments are those of a_i = (raw_i + offset) * scale taken
 * exactly, not of the rounded x_i: |x_i - a_i| <= 2.0001 u |a_i| (u = 2^-53), so the relative gap to the exact statistics of the x_i is
 * at most about 2u mean|x| / |mean| for the mean and 2u sqrt(1 + mean^2 / var) for the sstdev -- below 1e-13 while |mean| / sstdev < 400
 * (nanopore pA data: about 5), larger for a dataset with almost no spread far from zero. Not byte-pinned to
 * sigtk | datamash (section 11.3). No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_pamean pg_pamean;
typedef struct {
    uint64_t n_reads;
    int32_t location;              /* PG_LOC_HOST or PG_LOC_DEVICE: all five arrays */
    int32_t reserved;
    const int16_t *sig;
    const uint64_t *sig_off;       /* n_reads + 1 non-decreasing offsets into sig, which holds at least sig_off[n_reads] samples (the
                                      library cannot see the size of sig: offsets past it are read); a read has fewer than 2^33 samples */
    const double *digitisation, *offset, *range; /* n_reads each */
} pg_pamean_batch;
typedef struct {
    uint64_t n_reads;              /* reads submitted since the last finish (zero-length ones included) */
    uint64_t n_fallback;           /* reads whose mean the host finished with the sequential loop */
    uint64_t n_samples;            /* N */
    double mean;                   /* NaN when N == 0 */
    double sstdev;                 /* NaN when N < 2 */
} pg_pamean_result;
pg_status pg_pamean_create(int32_t device, pg_pamean **out);
void      pg_pamean_destroy(pg_pamean *h);
const char *pg_pamean_last_error(const pg_pamean *h); /* h may be NULL: error of the last failed pg_pamean_create */
/* Queues one batch and returns; means_out (host double[n_reads], may be NULL) is filled by the next pg_pamean_sync / submit / finish.
 * PG_LOC_HOST arrays: any host memory (page-locked signal is copied from directly, other memory through a pinned buffer); they must stay
 * valid until that call returns (the host reads the samples of the reads it finishes). PG_LOC_DEVICE arrays: memory of the handle's
 * device, complete before the call, read in place and unchanged until that call returns. */
pg_status pg_pamean_submit(pg_pamean *h, const pg_pamean_batch *batch, double *means_out);
pg_status pg_pamean_sync(pg_pamean *h);
/* The dataset summary of every read since the last finish; the handle is reset afterwards, also after an error. */
pg_status pg_pamean_finish(pg_pamean *h, pg_pamean_result *out);

/* ---- svb-zd signal blocks decoded on the device ----------------------------------------------------------------------------------
 * A BLOW5 record with signal compression svb-zd holds its samples as a block: u32 count, ceil(count / 4) control bytes (2 bits per
 * value: byte length - 1, value i in bits 2 (i & 3) of byte i >> 2), then the values' 1-4 little-endian data bytes; the samples are the
 * running sum, modulo 2^32 from 0, of the zig-zag decoded values, cut to 16 bits. Every code of every length is valid input (a small
 * value in a long code, a non-zero top byte, a wrapping sum), unused bytes behind the data are accepted, and a 4-byte block with count 0
 * is an empty read. The blocks of n_reads reads lie in one byte array, read r in [block_off[r], block_off[r + 1]), at any byte offset.
 * A block is corrupt when it is shorter than 4 bytes, when the control bytes of its count or one data byte per value do not fit (found
 * on the host, before anything is sized by the count), or when its byte lengths sum to more than its data bytes (found on the device).
 * A corrupt block is flagged, never an error of the call: no load for it leaves the block, nothing is stored outside its read's span.
 * No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_sigdec pg_sigdec;
pg_status pg_sigdec_create(int32_t device, pg_sigdec **out);
void      pg_sigdec_destroy(pg_sigdec *h);
const char *pg_sigdec_last_error(const pg_sigdec *h); /* h may be NULL: error of the last failed pg_sigdec_create */
/* counts_out (host u32[n_reads]): the samples each read decodes to -- the block's count, 0 for a block the host's checks refuse. */
pg_status pg_sigdec_counts(pg_sigdec *h, const void *blocks, uint64_t n_block_bytes, const uint64_t *block_off, uint64_t n_reads, int32_t location,
                           uint32_t *counts_out);
/* Decodes read r to sig_out_device[sig_off[r] ... sig_off[r] + count(r)) and returns when the samples are there. location says where
 * blocks lies: PG_LOC_HOST, any host memory (page-locked memory is copied from directly, other memory through a pinned buffer), or
 * PG_LOC_DEVICE, memory of the handle's device, complete before the call. block_off, sig_off (n_reads + 1 non-decreasing offsets each;
 * a span shorter than its read's count is PG_ERR_INVALID_ARG) and bad_out (n_reads bytes: 1 for a corrupt block, whose span then holds
 * unspecified samples) are host memory. Samples outside [sig_off[r], sig_off[r] + count(r)) are not written. */
pg_status pg_sigdec_decode(pg_sigdec *h, const void *blocks, uint64_t n_block_bytes, const uint64_t *block_off, uint64_t n_reads, int32_t location,
                           int16_t *sig_out_device, const uint64_t *sig_off, uint8_t *bad_out);

typedef struct {
    uint64_t n_reads;
    int32_t location;              /* PG_LOC_HOST or PG_LOC_DEVICE: where blocks lies */
    int32_t reserved;
    const void *blocks;
    uint64_t n_block_bytes;
    const uint64_t *block_off;     /* host, n_reads + 1 */
} pg_svb_batch;
/* pg_pamean_submit for a batch whose samples are still svb-zd blocks: they are decoded on the device into a buffer of the handle, the
 * reads back to back, and that buffer takes the PG_LOC_DEVICE path of pg_pamean_submit. digitisation, offset and range are host arrays
 * of n_reads values; nothing of the batch is needed after the call returns. A corrupt block fails the call with PG_ERR_INPUT -- the
 * text names the first such read's index in the batch and says "corrupt streamvbyte block" --, nothing of the batch is counted and the
 * handle stays usable. */
pg_status pg_pamean_submit_svb(pg_pamean *h, const pg_svb_batch *svb, const double *digitisation, const double *offset, const double *range,
                               double *means_out);
/* the samples pg_pamean_submit_svb has decoded on the device since create */
uint64_t  pg_pamean_svb_samples(const pg_pamean *h);

/* ---- move tables to ss ops: what `reform -c -k 1 -m 0` prints for a batch of BAM records, produced on the device -------------------------
 * Read r of a batch: its table is the int8 elements of the record's mv:B:c array behind the stride element, bytes [mv_off[r], mv_off[r + 1])
 * of mv as they lie in the record (any byte offset; an element is a move iff it is 1), with stride[r] = the array's first element, ns[r] and
 * ts[r] the tags of those names, l_seq[r] bases packed two 4-bit codes per byte from byte byte_off[r] of seq_bytes (the layout of
 * pg_kfreq_submit_reads) and flag[r] the record's FLAG. Records with flag 0x100 or 0x800 are the caller's to drop. With pos[] the 1-based
 * positions of the moves and n the table's length, the read's ops are (host/reform_cli.cpp, reform_record; src/reform.cpp:284-358):
 *   query_start = ts + (pos[0] - 1) * stride;  one op (pos[j + 1] - pos[j]) * stride per later move while bases remain;  then, if an element
 *   lies behind pos[0] and a base remains, the tail op (n - pos[last]) * stride + (ns - ((n - 1) * stride + ts))
 * in reform's arithmetic (uint32 gaps that wrap, int64 ns and ts). target_start / target_end are 0 / l_seq, or l_seq / 0 with PG_MVOPS_RNA
 * (`reform --rna`); seq is the read as `samtools fastq` prints it (flag 0x10: reversed and complemented; PG_MVOPS_N_TO_T: N printed as T).
 * A read reform refuses gets no ops and a status: the caller decides what that means. An accepted read has exactly l_seq ops, all matches.
 * The result lies in device memory of the handle, laid out as the arrays of the same names of a pg_batch, op_t all 0 (the batch may be
 * submitted with PG_BATCH_ALL_MATCHES), complete when the call returns, valid until the next pg_mvops_expand or pg_mvops_destroy on the
 * handle. location: where all nine input arrays lie; host arrays are free for reuse when the call returns, device arrays are read in place.
 * Long tables are cut into pieces of pg_mvops_piece elements, one wave of the device each. No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_mvops pg_mvops;
enum { PG_MVOPS_RNA = 1, PG_MVOPS_N_TO_T = 2 };
enum { PG_MVOPS_ST_ACCEPTED = 0, PG_MVOPS_ST_NO_MOVE_IN_TABLE = 1, PG_MVOPS_ST_NEGATIVE_TAIL = 2, PG_MVOPS_ST_BASES_LEFT_OVER = 3, PG_MVOPS_ST_BAD_STRIDE = 4 };
typedef struct {
    uint64_t n_reads;
    int32_t  location;           /* PG_LOC_HOST or PG_LOC_DEVICE */
    uint32_t flags;              /* PG_MVOPS_* */
    const int8_t   *mv;
    uint64_t n_mv_bytes;         /* bytes of mv; mv_off[n_reads] may not exceed it */
    const uint64_t *mv_off;      /* [n_reads + 1] */
    const int32_t  *stride;      /* [n_reads] */
    const uint64_t *ns, *ts;
    const uint32_t *l_seq, *flag;
    const uint8_t  *seq_bytes;
    uint64_t n_seq_bytes;
    const uint64_t *byte_off;    /* [n_reads] */
} pg_mvops_batch;
typedef struct {
    uint64_t n_reads, n_ops, n_seq;  /* n_ops = op_off[n_reads], n_seq = seq_off[n_reads] */
    uint64_t n_refused;
    int64_t  first_refused;          /* the first read with a status other than 0, or -1 */
    const uint32_t *op_n;            /* device, dense */
    const uint8_t  *op_t;            /* device, all 0 */
    const uint64_t *op_off;          /* device [n_reads + 1] */
    const int32_t  *query_start, *target_start, *target_end; /* device [n_reads] */
    const uint8_t  *seq;             /* device, ASCII */
    const uint64_t *seq_off;         /* device [n_reads + 1] */
    const uint32_t *status;          /* device [n_reads], PG_MVOPS_ST_* */
    const uint32_t *status_host;     /* the same in host memory of the handle */
} pg_mvops_result;
pg_status pg_mvops_create(int32_t device, pg_mvops **out);
void      pg_mvops_destroy(pg_mvops *h);
const char *pg_mvops_last_error(const pg_mvops *h); /* h may be NULL: error of the last failed pg_mvops_create */
uint32_t  pg_mvops_piece(const pg_mvops *h);        /* h may be NULL */
/* The kernels and copies of the following calls go to a caller-owned HIP stream (hipStream_t as void*, e.g. the one handed to
 * pg_set_stream); NULL restores the handle's own. pg_mvops_stream returns the stream in use. */
pg_status pg_mvops_set_stream(pg_mvops *h, void *hip_stream);
void     *pg_mvops_stream(const pg_mvops *h);
pg_status pg_mvops_expand(pg_mvops *h, const pg_mvops_batch *batch, pg_mvops_result *out);

/* The ops of a batch carried through the records' CIGARs onto the reference (`poregen reform -c --to_ref`; the rule: csrc/pg_refops.h).
 * Input: the ops to project as DEVICE arrays of device `h` was created on, whatever `location` says -- op_n, op_off[n_reads + 1], query_start
 * and status as pg_mvops_expand leaves them (every op a match, op j of a read belongs to base j of SEQ, or to base L - 1 - j with
 * PG_MVOPS_RNA; n_ops = the elements of op_n) -- and the CIGARs: read r's words are cigar[cigar_off[r] .. cigar_off[r + 1]) as a BAM record
 * stores them (len << 4 | op, op 0..8 = MIDNSHP=X), pos[r] its 0-based position. location: where cigar, cigar_off and pos lie; host arrays
 * are free for reuse when the call returns. Along a read's words (in reverse order with PG_MVOPS_RNA), q counting the bases used: an S in
 * front of the first M/=/X/I/D/N adds ops q .. q + len to query_start; an S behind it drops them; M, = and X copy them; an I writes one
 * op I of their sum (uint32); D and N write one op D of len; H, P and every word of length 0 do nothing. ref_len = the M/=/X/D/N lengths,
 * target_start / target_end = pos, pos + ref_len (PG_MVOPS_RNA: the other way round), n_match = the match ops, query_end = the new
 * query_start + every value written as a match or an I. Statuses: a read the expansion refused keeps its code; no word:
 * PG_MVOPS_ST_NO_CIGAR; the M/I/S/=/X lengths do not come to the read's ops: PG_MVOPS_ST_CIGAR_LENGTH; an op code above 8:
 * PG_MVOPS_ST_CIGAR_OP -- the first of these decides. A refused read has no ops, ref_len, n_match and the target columns 0 and keeps
 * its query_start (= query_end). cigar_off that decreases or runs past n_cigar (op_off likewise) is PG_ERR_INVALID_ARG, decided before
 * any kernel reads a word. The result lies in device memory of the handle, laid out as the arrays of the same names of a pg_batch --
 * seq / seq_off of that batch are the caller's: the reference slices [min, max) of the target columns -- which is submitted WITHOUT
 * PG_BATCH_ALL_MATCHES; complete when the call returns, valid until the next pg_mvops_project or pg_mvops_destroy on the handle. It
 * shares nothing with the result of pg_mvops_expand, which it may read in place and leaves as it is. Reads are cut into pieces of
 * pg_mvops_piece bases, one wave of the device each. No CPU fallback: PG_ERR_NO_DEVICE without a GPU (at pg_mvops_create). */
enum { PG_MVOPS_ST_NO_CIGAR = 5, PG_MVOPS_ST_CIGAR_LENGTH = 6, PG_MVOPS_ST_CIGAR_OP = 7 };
typedef struct {
    uint64_t n_reads;
    int32_t  location;           /* of cigar, cigar_off and pos: PG_LOC_HOST or PG_LOC_DEVICE */
    uint32_t flags;              /* PG_MVOPS_RNA */
    const uint32_t *op_n;        /* device */
    uint64_t n_ops;              /* elements of op_n; op_off[n_reads] may not exceed it */
    const uint64_t *op_off;      /* device [n_reads + 1] */
    const int32_t  *query_start; /* device [n_reads] */
    const uint32_t *status;      /* device [n_reads], PG_MVOPS_ST_* */
    const uint32_t *cigar;
    uint64_t n_cigar;            /* words of cigar; cigar_off[n_reads] may not exceed it */
    const uint64_t *cigar_off;   /* [n_reads + 1] */
    const int32_t  *pos;         /* [n_reads], 0-based */
} pg_mvops_cigars;
typedef struct {
    uint64_t n_reads, n_ops;         /* n_ops = op_off[n_reads] */
    uint64_t n_refused;
    int64_t  first_refused;          /* the first read with a status other than 0, or -1 */
    const uint32_t *op_n;            /* device, dense */
    const uint8_t  *op_t;            /* device: 0 match, 1 I, 2 D */
    const uint64_t *op_off;          /* device [n_reads + 1] */
    const int32_t  *query_start, *target_start, *target_end, *query_end; /* device [n_reads] */
    const uint32_t *ref_len, *n_match, *status;                          /* device [n_reads] */
    const uint32_t *status_host, *ref_len_host, *n_match_host;           /* the same in host memory of the handle */
    const int32_t  *query_end_host;
} pg_mvops_projection;
pg_status pg_mvops_project(pg_mvops *h, const pg_mvops_cigars *cigars, pg_mvops_projection *out);

/* The same with the records' strands. A reverse-strand record (flag 0x10) is a forward record on the reverse complement of its contig:
 * with reverse[r] != 0 op j of read r belongs to base L - 1 - j of the stored SEQ (with PG_MVOPS_RNA: to base j), so the words are walked
 * in reverse order iff PG_MVOPS_RNA is set for a forward read and iff it is not for a reverse one, and pos' = contig_len[r] - pos[r] -
 * ref_len (uint32 arithmetic, cast to int32) stands where pos[r] stood in target_start / target_end. A reverse read whose contig_len is
 * <= 0 (no @SQ line; a length above 2^31 - 1 is to be passed as 0) gets PG_MVOPS_ST_NO_CONTIG_LEN, decided behind the seven other
 * codes. Everything else is pg_mvops_project's, which is this call with strands == NULL; a pg_mvops_strands whose two pointers are NULL
 * is the same. reverse and contig_len lie where cigars->location says; one of the two alone is PG_ERR_INVALID_ARG. */
enum { PG_MVOPS_ST_NO_CONTIG_LEN = 8 };
typedef struct {
    const uint8_t *reverse;      /* [n_reads]: 0 forward, anything else reverse */
    const int32_t *contig_len;   /* [n_reads]: the length of the read's reference sequence */
} pg_mvops_strands;
pg_status pg_mvops_project_stranded(pg_mvops *h, const pg_mvops_cigars *cigars, const pg_mvops_strands *strands, pg_mvops_projection *out);

/* ---- refseq: the reference slices of mapped reads, gathered on the device ---------------------------------------------------------------
 * What `gmove --reform --ref` hands the collector as seq / seq_off of a pg_batch: for every read the bases [st_k, end_k) of its contig
 * (st_k / end_k = the smaller / larger of pos and pos + ref_len under an unsigned compare), fetched as htslib 1.17's faidx_fetch_seq(st_k,
 * end_k - 1) fetches them -- clamped into the contig; ref_len == 0 gives the ONE base at pos - 1, faidx_adjust_position's quirk (the rule:
 * csrc/pg_refseq.h). With reverse[r] != 0 the slice is those bases in reverse order, each complemented (A<->T, C<->G in either case,
 * U -> A, u -> a, every other byte as it is): the slice of the contig's reverse complement.
 * Contigs are added one by one, whenever a caller first needs them: `bases` are the contig's bytes with the line ends removed, copied to a
 * device buffer of their own when pg_refseq_add returns; *index is the number pg_refseq_reads::contig names it by. A contig index of -1
 * is "no such contig" and gives an empty slice. location: where contig, pos, ref_len and reverse lie. An index outside [-1, n_contigs)
 * is PG_ERR_INVALID_ARG for host arrays and is taken as -1 for device arrays. The result lies in device memory of the handle, as
 * pg_batch::seq / seq_off take it; complete when the call returns, valid until the next pg_refseq_slice or pg_refseq_destroy. No load
 * leaves a contig, no store a read's span. No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_refseq pg_refseq;
typedef struct {
    uint64_t n_reads;
    int32_t  location;           /* PG_LOC_HOST or PG_LOC_DEVICE */
    const int32_t  *contig;      /* [n_reads]: the index pg_refseq_add gave, or -1 */
    const int32_t  *pos;         /* [n_reads], 0-based */
    const uint32_t *ref_len;     /* [n_reads] */
    const uint8_t  *reverse;     /* [n_reads], or NULL: every read forward */
} pg_refseq_reads;
typedef struct {
    const uint8_t  *seq;         /* device, read r's slice at seq_off[r] .. seq_off[r + 1] */
    const uint64_t *seq_off;     /* device [n_reads + 1] */
    uint64_t n_seq;              /* = seq_off[n_reads] */
} pg_refseq_slices;
pg_status pg_refseq_create(int32_t device, pg_refseq **out);
void      pg_refseq_destroy(pg_refseq *h);
const char *pg_refseq_last_error(const pg_refseq *h); /* h may be NULL: error of the last failed pg_refseq_create */
pg_status pg_refseq_set_stream(pg_refseq *h, void *hip_stream); /* as pg_mvops_set_stream */
pg_status pg_refseq_add(pg_refseq *h, const uint8_t *bases, uint64_t n, int32_t *index);
pg_status pg_refseq_slice(pg_refseq *h, const pg_refseq_reads *reads, pg_refseq_slices *out);

/* ---- model: the k-mer model from the TEXT of dump files, parsed and reduced on the device ---------------------------------------------
 * What scripts/poregen.sh:54-85 (tr ';,' '\n' | tail -n +2 | datamash median 1 / sstdev 1) and :33-52 (awk comma counts | datamash
 * median) compute per dump file, for files that already exist: written by the reference, by an earlier run, with -d, or several
 * directories' files of one name back to back. A submission holds n_files files: file i is bytes [file_off[i], file_off[i + 1]).
 * The device parses the files of the strict grammar  (-?D+.DDDDDDDD[,;])*  -- exactly eight decimals, |value| < 4e7, the last byte
 * a ';': every file gmove writes without -d -- into integers of 1e-8 units and reduces them with pg_model's kernels: the same exact
 * median and moments, without a double in between. Every other file (':' of -d, a newline, "1e2", "+1.5", blanks, "inf", another
 * number of decimals, an unclosed last event, ...) and every file the reduction declines (more than 2^23 values, values further than
 * 2^40 units from the first, a negative zero that may be the median) is finished on the host by the pipeline's rules restated
 * (strtold into long double, datamash's median and sstdev); pg_dmodel_info counts them. No valid input is refused.
 * Results: pg_model_result over all files since the last finish, in submission order. For a file the host finished, the exact fields
 * (mid_lo, mid_hi, origin, sum1, sum2_*) are 0 and median / sstdev are the long doubles rounded; its texts come from pg_dmodel_format,
 * which is pg_model_format for every other file. The --stdv_limit cap stays with the caller. No CPU fallback for the whole:
 * PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_dmodel pg_dmodel;
enum { PG_DMODEL_PROFILE = 1u << 8 }; /* pg_dmodel_create flags (beside PG_MODEL_KEEP_FIRST): time the kernels with HIP events */
typedef struct {
    uint64_t n_files;
    uint64_t n_bytes;
    uint64_t n_values;            /* values the device parsed (before tail -n +2) */
    uint64_t n_host_files;        /* files finished on the host */
    const uint32_t *host_files;   /* [n_host_files] their indices, ascending; owned by the handle until the next finish / destroy */
    uint32_t n_batches, reserved;
    double parse_ms, model_ms;    /* PG_DMODEL_PROFILE: device time of the parse kernels and of the reduction, else 0 */
} pg_dmodel_info;
pg_status pg_dmodel_create(int32_t device, uint32_t flags, pg_dmodel **out);
void      pg_dmodel_destroy(pg_dmodel *h);
const char *pg_dmodel_last_error(const pg_dmodel *h); /* h may be NULL: error of the last failed pg_dmodel_create */
/* file_off: host uint64[n_files + 1], non-decreasing, file_off[0] = 0; bytes: file_off[n_files] bytes, at most 2^31, n_files at most 2^24
 * per call. PG_LOC_HOST: any host memory, free for reuse when the call returns. PG_LOC_DEVICE: memory of the handle's device, complete
 * before the call, read in place and unchanged until pg_dmodel_sync or pg_dmodel_finish. The call queues the batch and settles the one
 * before it (download, host-finished files), so that a caller reads its next files while this batch is on the device. */
pg_status pg_dmodel_submit(pg_dmodel *h, const void *bytes, const uint64_t *file_off, uint32_t n_files, int32_t location);
pg_status pg_dmodel_sync(pg_dmodel *h);
/* Every file since the last finish. out and info (may be NULL) are owned by the handle until the next submit / finish / destroy. */
pg_status pg_dmodel_finish(pg_dmodel *h, pg_model_result *out, pg_dmodel_info *info);
/* pg_model_format for the handle's last finish (which = PG_MODEL_TEXT_*), with the host-finished files' texts as datamash prints them */
size_t    pg_dmodel_format(const pg_dmodel *h, uint32_t file, int32_t which, char *buf, size_t cap);

/* ---- the event table: per file the median and sstdev of its events' LEVELS and of its events' SPREADS -----------------------------------
 * pg_dmodel_finish reduces all samples of a file at once, which mixes the noise inside an event with the spread between events. A handle
 * created with PG_DMODEL_EVENTS also computes, for every event (the values up to a ';'), in 1e-8 units and in exact integer arithmetic,
 *   mean    m = floor((2 S + n) / (2 n)), S the sum of its n samples: the mean rounded to the nearest unit, halves up
 *   spread  s = (isqrt(floor(4 N / D)) + 1) div 2, N = n sum d^2 - (sum d)^2, d = sample - first sample, D = n (n - 1): the sample
 *           standard deviation rounded to the nearest unit, halves up
 * on the device (a segmented reduction over the parsed values), and reduces a file's m and its s, in file order and
 * with the first value KEPT whatever PG_MODEL_KEEP_FIRST says, exactly as pg_dmodel_finish reduces samples: `means` and `sds` are
 * pg_model_result over the same files (dwell_n 0), their texts pg_model_format's. There is NO host path: a file's table is REFUSED --
 * status[file] != 0, empty columns, a message; the other files are still right -- when pg_dmodel_finish finishes the file on the host,
 * when one of its events has one sample, more than 4096 samples or a sample 2^41 units or further from its first, or when the reduction
 * declines its means or spreads. Never a wrong number. Without the flag a handle does none of this and allocates nothing for it. */
enum { PG_DMODEL_EVENTS = 1u << 9,        /* pg_dmodel_create: also the event table */
       PG_DMODEL_EVENTS_KEEP = 1u << 10 }; /* ... and keep every event's m and s on the host for pg_dmodel_events_values (implies PG_DMODEL_EVENTS) */
enum { PG_EVENTS_OK = 0, PG_EVENTS_HOST_FILE = 1, PG_EVENTS_ONE_SAMPLE = 2, PG_EVENTS_TOO_LONG = 4, PG_EVENTS_TOO_WIDE = 8, PG_EVENTS_BAD_VALUE = 16,
       PG_EVENTS_DECLINED = 32 };          /* status bits of a refused file */
enum { PG_EVENTS_COL_MEAN_MEDIAN = 0, PG_EVENTS_COL_MEAN_SSTDEV = 1, PG_EVENTS_COL_SD_MEDIAN = 2, PG_EVENTS_COL_SD_SSTDEV = 3 };
/* The event table of the files of the last pg_dmodel_finish (which it calls when there was none since the last submit). status and n_events
 * (may be NULL): [n_files], owned by the handle like the results. PG_ERR_INVALID_ARG for a handle without PG_DMODEL_EVENTS. */
pg_status pg_dmodel_finish_events(pg_dmodel *h, pg_model_result *means, pg_model_result *sds, const uint32_t **status, const uint64_t **n_events);
/* one field of the table as datamash would print it (column = PG_EVENTS_COL_*): "" for a file without events or a refused one */
size_t    pg_dmodel_format_events(const pg_dmodel *h, uint32_t file, int32_t column, char *buf, size_t cap);
/* why the file's table was refused at the last pg_dmodel_finish_events ("" for one that was not); owned by the handle */
const char *pg_dmodel_events_refusal(const pg_dmodel *h, uint32_t file);
/* PG_DMODEL_EVENTS_KEEP: m and s of all *n events, file after file: n_events[file] each, the parser's count, so a refused file's events
 * lie between its neighbours' (s = 0 where there is none; a file outside the strict grammar has no events); owned by the handle */
pg_status pg_dmodel_events_values(const pg_dmodel *h, const int64_t **mean, const int64_t **sd, uint64_t *n);
/* PG_DMODEL_PROFILE: device time of the per-event kernels and of the two reductions behind them since the last finish (either may be NULL) */
pg_status pg_dmodel_events_ms(const pg_dmodel *h, double *event_ms, double *reduce_ms);

/* The event table of a context's kept events (see pg_model: the same events, slot by slot), computed on the device from the kept samples
 * as the "%.8f" text stands for them. Calls pg_finish first. Arrays are owned by the context until the next pg_model_events / pg_reset /
 * pg_destroy. Unlike pg_model a refused slot fails nothing here: the caller decides (status as above; PG_EVENTS_HOST_FILE never). */
typedef struct {
    pg_model_result means, sds;   /* one slot per k-mer: the reduction of its events' m and of their s */
    const uint32_t *status;       /* [n_slots] PG_EVENTS_* bits */
    const uint64_t *n_events;     /* [n_slots] */
} pg_events_result;
pg_status pg_model_events(pg_ctx *ctx, uint32_t flags, pg_events_result *out);
/* the message that goes with a status ("" for PG_EVENTS_OK and for bits this library does not know), in a buffer of the calling thread
 * that its next call overwrites */
const char *pg_events_status_text(uint32_t status);

/* ---- pools: median and sstdev of dump files read back to back, parsed, kept and selected on the device --------------------------------
 * A pool is a list of dump files in a fixed order; its numbers are the pipeline's for the files concatenated: `cat F1 F2 ... | tr ';,' '\n'
 * | tail -n +2 | datamash median 1` and `... sstdev 1` (scripts/poregen.sh:73-74). So the first value of the CONCATENATION is dropped --
 * the first value of the first member that has one -- unless PG_MODEL_KEEP_FIRST is given. A caller declares n_labelings labelings,
 * labeling l with n_groups[l] groups; every submitted file carries one group id per labeling (PG_POOL_NO_GROUP: in none), and the files
 * of a group count in submission order, across submits. Per batch the device parses the text (the kernels of pg_dmodel_*), reduces every
 * file with its first value kept, and appends the parsed values to an arena of 8 bytes per value that lives until finish. finish adds the
 * files' exact moments up on the host and selects every group's two middle values on the device: a radix selection over the arena, seven
 * streaming reads of it for all labelings and groups at once.
 * A group is REFUSED -- status, the first file that caused it, a message; every other group is still right -- when one of its members
 * is a file pg_dmodel_* would finish on the host (outside the strict grammar, more than 2^23 values, values further than 2^40 units from
 * its first), when it holds a negative zero and both middle values are 0, when it has more than 2^32 - 1 values, or when its moments do
 * not fit the result's fields. There is NO host path for pools: the text of earlier batches is gone at finish. Never a wrong number.
 * max_values caps the arena (0: half of the device's free memory at create, in values); a submit that would pass it fails with
 * PG_ERR_UNSUPPORTED, counts nothing of its batch and leaves the handle usable. No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_pool pg_pool;
#define PG_POOL_NO_GROUP 0xffffffffu
#define PG_POOL_MAX_LABELINGS 16u
enum { PG_POOL_GROUP_OK = 0, PG_POOL_GROUP_EMPTY = 1, PG_POOL_GROUP_REFUSED = 2 };
typedef struct {
    pg_model_result model;        /* one slot per group, labeling after labeling; dwell_n 0 and dwell_median NaN; a refused group reads as empty */
    uint32_t n_groups, n_batches; /* sum of n_groups[] */
    const uint32_t *status;       /* [n_groups] PG_POOL_GROUP_* */
    const int64_t  *refused_file; /* [n_groups] the first file (index in submission order since the last finish) that caused the refusal, else -1 */
    const uint64_t *n_files;      /* [n_groups] members */
    uint64_t n_files_total, n_bytes;
    uint64_t n_values;            /* values in the arena */
    double select_ms;             /* device time of the seven histogram passes and their picks (HIP events) */
} pg_pool_result;
pg_status pg_pool_create(int32_t device, uint32_t n_labelings, const uint32_t *n_groups, uint64_t max_values, uint32_t flags, pg_pool **out);
void      pg_pool_destroy(pg_pool *h);
const char *pg_pool_last_error(const pg_pool *h); /* h may be NULL: error of the last failed pg_pool_create */
/* bytes, file_off, n_files, location: as pg_dmodel_submit, with the same limits. group: host uint32[n_labelings][n_files]. The call
 * returns when the batch is in the arena; PG_LOC_DEVICE bytes are free again then. */
pg_status pg_pool_submit(pg_pool *h, const void *bytes, const uint64_t *file_off, uint32_t n_files, const uint32_t *group, int32_t location);
pg_status pg_pool_sync(pg_pool *h);
/* Every file since the last finish; the arena is emptied by the next submit. out is owned by the handle until the next submit / finish / destroy. */
pg_status pg_pool_finish(pg_pool *h, pg_pool_result *out);
/* pg_model_format of a group (which = PG_MODEL_TEXT_MEDIAN or PG_MODEL_TEXT_SSTDEV); an empty or refused group gives the empty string */
size_t    pg_pool_format(const pg_pool *h, uint32_t group, int32_t which, char *buf, size_t cap);
/* why the group was refused at the last finish ("" for a group that was not); owned by the handle */
const char *pg_pool_refusal(const pg_pool *h, uint32_t group);

/* ---- transform: the raw k-mer model to the final model file (STEP 7), on the host -------------------------------------------------------
 * scripts/poregen.sh:87-129 (apply_transformation) and, with stdv_from, :131-148 (set_stddev), without bc, datamash, cut and paste. No
 * handle, no device, no global state: 4^k rows of exact decimal arithmetic by bc's rules (scale 20; csrc/pg_bcdec.h).
 *   raw        n bytes of KMER<TAB>level_mean<TAB>level_stdv rows (further columns ignored; a last line without '\n' counts)
 *   A, B       NUL-terminated decimal texts: level_mean' = (level_mean * A) + B  (sstdev and mean of the whole pA dataset)
 *   C, D       level_stdv' = (level_stdv - min) * (D - C) / (max - min) + C, min and max as `datamash min 1 max 1` prints them
 *   stdv_from  NULL, or n_from bytes of a model file: column 3 of its lines 8 onward replaces level_stdv', by position, verbatim
 * PG_OK: *out holds *n_out bytes (and a NUL behind them) -- the seven header lines, "#k" with the first k-mer's length, and one row per
 * input row -- to be released with pg_transform_free. PG_ERR_INPUT: the model is refused as a whole (a field that is no number to bc
 * -- "1e-05", "nan", "+1", an empty field --, a row with fewer than 3 fields, k-mers of two lengths, max == min, an empty model, unequal
 * row counts with stdv_from, a text bc would wrap); *out is NULL and err (err_cap bytes, may be NULL) names the line and the reason.
 * PG_ERR_INVALID_ARG: a missing pointer, or out of memory. Never a wrong digit. */
pg_status pg_transform_model(const char *raw, size_t n, const char *A, const char *B, const char *C, const char *D, const char *stdv_from, size_t n_from,
                             char **out, size_t *n_out, char *err, size_t err_cap);
void      pg_transform_free(char *text);

/* ---- fit: a k-mer model scored against signal and move tables -------------------------------------------------------------------------------
 * Input: batches laid out as pg_mvops_expand leaves them (every op a match, as many ops as bases), the signal as the collector takes it.
 * For a read of Lb bases seq, ops n_0 .. n_{Lb-1} and query_start q, event e is the samples [q + n_0 + .. + n_{e-1}, .. + n_e). For
 * i = 0 .. Lb - k the event e = i + sig_move_offset (if e < Lb) carries the k-mer seq[i, i + k) -- seq[Lb - i - k, Lb - i) with rna -- and
 * counts when min_dur <= n_e <= max_dur, all its letters are ACGT and the model has a level for it. All device arithmetic is integer.
 * Pass 1, per read, over the samples r (raw int16) of its counted events, l the event's level in 1e-3 pA: N = sum 1, SL = sum l,
 * SLL = sum l^2, SR = sum r, SRL = sum r l, SRR = sum r^2 and E, the counted events (pg_fit_sums, exact). The host solves
 * r = a + b l by least squares: den = N SLL - SL^2, numb = N SRL - SL SR, numa = SR SLL - SL SRL in 128-bit integers,
 * b = (double)numb / (double)den, a = (double)numa / (double)den. Statuses, tested in this order: out_of_signal (q < 0 or the ops run
 * past the read's samples), too_long (N > 2^24; only N and E are kept), few_events (E < min_events), flat (den = 0), negative_scale
 * (numb <= 0). Pass 2, per k-mer, over the samples of the fitted reads: c = llrint(((double)r - a) * (1.0 / b)), d = c - l clamped to
 * |d| <= 2^18 - 1; per slot (the k-mer's rank in ACGT order) the samples, the events, sum d and sum d^2, exact and independent of order.
 * No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_fit pg_fit;
enum { PG_FIT_ST_OK = 0, PG_FIT_ST_OUT_OF_SIGNAL = 1, PG_FIT_ST_TOO_LONG = 2, PG_FIT_ST_FEW_EVENTS = 3, PG_FIT_ST_FLAT = 4, PG_FIT_ST_NEGATIVE_SCALE = 5,
       PG_FIT_ST_REF_LENGTH = 6,   /* gapped batches: the reference slice has not as many bases as the ops have columns */
       PG_FIT_ST_SKIPPED = 16 };   /* PG_FIT_ST_SKIPPED + c: the caller's skip code c for the read (1 <= c < 2^16) */
typedef struct {
    uint32_t struct_size;          /* sizeof(pg_fit_params) */
    uint32_t sig_move_offset;      /* -m            at most 64 */
    uint32_t min_dur, max_dur;     /* --min_dur, --max_dur: min_dur <= max_dur <= 2^20 */
    uint32_t min_events;           /* --min_events */
    int32_t  rna;                  /* --rna */
} pg_fit_params;
typedef struct { int64_t n, sl, sll, sr, srl, srr, e; } pg_fit_sums; /* 56 bytes per read */
typedef struct {                   /* the reads of one submit; arrays owned by the handle until its next submit / finish / destroy */
    uint64_t n_reads;
    const pg_fit_sums *sums;
    const uint32_t *status;        /* PG_FIT_ST_* */
    const double *a, *b;           /* 0 unless the status is PG_FIT_ST_OK */
} pg_fit_reads;
typedef struct {                   /* every submit since the last finish; arrays owned by the handle until its next submit / finish / destroy */
    uint32_t kmer_size, reserved;
    uint64_t n_slots;              /* 4^kmer_size */
    const uint64_t *n_samples, *n_events; /* [n_slots] */
    const int64_t  *sum_d;
    const uint64_t *sum_dd_lo, *sum_dd_hi; /* sum d^2, low and high 64 bits */
    uint64_t reads, fitted, events, samples, clamped; /* reads submitted and fitted; counted events and samples of the fitted reads; clamped samples */
} pg_fit_result;
pg_status pg_fit_create(const pg_fit_params *params, int32_t device, pg_fit **out);
void      pg_fit_destroy(pg_fit *h);
const char *pg_fit_last_error(const pg_fit *h); /* h may be NULL: error of the last failed pg_fit_create */
/* levels: host uint32[4^kmer_size], the level of every slot in 1e-3 pA, 0 < level < 2^18, or 0 for a k-mer without one (its events are
 * skipped); kmer_size 1 to 9. Not between a submit and the finish behind it (PG_ERR_STATE). */
pg_status pg_fit_set_model(pg_fit *h, const uint32_t *levels, uint32_t kmer_size);
/* One batch: both passes, and the solve between them; returns when the batch is done. The batch (PG_LOC_HOST or PG_LOC_DEVICE; digitisation,
 * offset, range, target_start and target_end are not read) must carry PG_BATCH_ALL_MATCHES; one that holds an I, a D or an unknown op is
 * refused with PG_ERR_INVALID_ARG (looked for on the device) and counts nothing, the handle stays usable. At most 2^28 samples of signal
 * (PG_ERR_UNSUPPORTED beyond). skip: NULL, or host uint32[n_reads]: a read with skip != 0 takes no part and is reported with the status
 * PG_FIT_ST_SKIPPED + skip (pg_mvops_result.status_host fits: the reads reform refuses).
 * Or the batch carries PG_BATCH_GAPPED (both flags: PG_ERR_INVALID_ARG): ops on the signal-to-reference alignment, op_t 0 (match), 1 (I)
 * or 2 (D; a code above 2: PG_ERR_INVALID_ARG), seq / seq_off the reads' reference slices (at most 2^32 - 1 bases each). A match of n and
 * an I of n take n samples, a D none; a match takes one reference column, a D of n takes n, an I none. With c_j the column in front of op
 * j, C a read's total and S its slice's length, event j counts iff it is a match, ops j - m .. j - m + k - 1 all exist and are matches,
 * min_dur <= n_j <= max_dur, and its k-mer -- seq[c_j - m, c_j - m + k), with rna seq[S - (c_j - m) - k, S - (c_j - m)) -- lies in the slice,
 * has ACGT letters and a level. A read with S != C (an empty slice, a contig the FASTA lacks) is PG_FIT_ST_REF_LENGTH, ranked behind
 * out_of_signal; no kernel reads its seq. Everything behind the pairing is as above. */
pg_status pg_fit_submit(pg_fit *h, const pg_batch *batch, const uint32_t *skip, pg_fit_reads *out);
/* A batch's reads put on the model's pA scale, for the collector (pg_set_read_scaling): pass 1 as pg_fit_submit runs it -- the same
 * batches, flags, refusals and limits, and digitisation, offset and range ARE read -- then the solve on the device (k_fit_solve: the host's
 * numbers bit for bit) and, per read, by this rule, each line one rounded IEEE double operation:
 *     g      = range / digitisation
 *     center = (a + offset) * g
 *     spread = (b * 1000.0) * g                  (levels are in 1e-3 pA)
 *     use    = status == PG_FIT_ST_OK  &&  center is finite  &&  spread is finite and > 0
 * (center = spread = 0 where use is 0). A sample's pA is center + spread * (the model's level in pA) up to the fit's residual, so
 * (pA - center) / spread is the sample on the model's pA scale. No pass 2: nothing is added to what pg_fit_finish returns. Synchronous;
 * nothing per read comes back to the host: the arrays are DEVICE memory, owned by the handle until its next submit / calibrate / destroy.
 * d_sums of a too_long read hold N and E only, as pg_fit_reads.sums do. */
typedef struct {
    uint64_t n_reads, n_ok;        /* n_ok: reads with use set */
    const pg_fit_sums *d_sums; const uint32_t *d_status; const double *d_a, *d_b;
    const double *d_center, *d_spread; const uint8_t *d_use;
    uint64_t n_status[8];          /* reads per PG_FIT_ST_* 0 .. 6; [7]: reads with a skip code. n_status[0] - n_ok reads are ok and not usable */
    double solve_ms;               /* HIP-event time of k_fit_solve and the tally behind it */
} pg_fit_scaling;
pg_status pg_fit_calibrate(pg_fit *h, const pg_batch *batch, const uint32_t *skip, pg_fit_scaling *out);
/* The per-slot sums and the totals of every submit since the last finish; the handle is reset afterwards (the model stays). */
pg_status pg_fit_finish(pg_fit *h, pg_fit_result *out);
/* The kernels and copies of the following calls go to a caller-owned HIP stream (hipStream_t as void*); NULL restores the handle's own. */
pg_status pg_fit_set_stream(pg_fit *h, void *hip_stream);
/* HIP-event time of the two passes' kernels since create or the last call of this (either pointer may be NULL) */
pg_status pg_fit_pass_ms(pg_fit *h, double *pass_one_ms, double *pass_two_ms);
/* Host only, no device needed. A model file in the format `poregen transform` writes: '#' lines and the "kmer<TAB>..." header line are
 * skipped, rows are KMER<TAB>level_mean<TAB>level_stdv (further fields ignored, level_stdv not used), all k-mers of one length 1 to 9
 * (want_k != 0: that length), U read as T. levels_out (cap_slots >= 4^k entries) gets level_mean rounded to the nearest 1e-3 pA, halves up,
 * exactly, on the decimal text; 0 for a k-mer the file does not hold. *uses_u (may be NULL): the file spells U. PG_ERR_INPUT: the model is
 * refused as a whole -- a field that is no number, a level outside (0, 262.144) pA, a k-mer twice, a letter outside ACGTU, two lengths, no
 * k-mer at all -- and err (err_cap bytes, may be NULL) names the line and the reason. */
pg_status pg_fit_parse_model(const char *text, size_t n, uint32_t want_k, uint32_t *kmer_size_out, uint32_t *levels_out, size_t cap_slots, int32_t *uses_u,
                             char *err, size_t err_cap);
/* Host only. A slot's residuals from its sums, n_samples > 0, in 1e-3 pA: mean = floor((2 sum d + n) / (2 n)) and
 * rms = (isqrt(floor(4 sum d^2 / n)) + 1) div 2, each the nearest unit with halves up. */
pg_status pg_fit_residuals(uint64_t n_samples, int64_t sum_d, uint64_t sum_dd_lo, uint64_t sum_dd_hi, int64_t *mean, int64_t *rms);

/* ---- realign: the boundaries of the move table refined against a k-mer model ----------------------------------------------------------------
 * The move table puts every event boundary on a multiple of the stride; this moves each by up to `band` samples to where the samples fit
 * the model's levels best. Input: a batch as pg_fit_submit takes it, and per read the status, a and b that pg_fit_submit returned for this
 * same batch under the same model, sig_move_offset, rna, min_dur and max_dur. Only reads with PG_FIT_ST_OK are refined; every other read
 * keeps its ops and reports zeros. With B_0 = query_start and B_e = B_{e-1} + n_{e-1}, event e is refinable iff it counts by fit's rule
 * (level l_e); boundary e, 0 < e < Lb, is free iff events e - 1 and e are both refinable and e % 256 != phase (0 unless asked for); every other boundary is pinned,
 * B_0 and B_Lb included. A sample r under level l costs d^2, d fit's pass-2 residual (c = llrint(((double)r - a) * (1.0 / b)), d = c - l
 * clamped to |d| <= 2^18 - 1). Per maximal run of free boundaries e0 < e < e1 between the pinned P0 = B_e0 and P1 = B_e1 a dynamic program
 * runs over the candidates p = B_e + j, |j| <= band, that are admissible (P0 + (e - e0) min_len <= p <= P1 - (e1 - e) min_len):
 * D[e0][P0] = 0, D[e][p] = min over reachable admissible p' with p' + min_len <= p of D[e-1][p'] + cost of event e - 1 on [p', p), a tie
 * taking the smallest p'; the new boundaries are traced back from P1. The original boundaries are always a solution, so
 * cost_after <= cost_before. All of it is integer arithmetic behind the residual: results do not depend on the device's scheduling.
 * No CPU fallback: PG_ERR_NO_DEVICE without a GPU (pg_realign_walk is the rule on the host, for tests). */
typedef struct pg_realign pg_realign;
typedef struct {
    uint32_t struct_size;          /* sizeof(pg_realign_params) */
    uint32_t sig_move_offset;      /* -m            at most 64 */
    uint32_t min_dur, max_dur;     /* --min_dur, --max_dur: min_dur <= max_dur <= 4096 */
    int32_t  rna;                  /* --rna */
    uint32_t band;                 /* --band        0 .. 31 */
    uint32_t min_len;              /* --min_len     1 .. min_dur: the fewest samples a refined event keeps */
    uint32_t phase;                /* 0 .. 255: the boundaries e with e % 256 == phase are the pinned ones; 0 (a zeroed struct) is the rule above */
} pg_realign_params;
typedef struct {                   /* one read; the costs are sums of d^2 over its refinable events under the old and the new boundaries */
    uint32_t n_free, n_moved;      /* free boundaries; those that moved */
    uint64_t sum_abs_shift;        /* sum of |new - old| over the free boundaries, in samples */
    uint64_t cost_before_lo, cost_before_hi, cost_after_lo, cost_after_hi; /* low and high 64 bits */
} pg_realign_read;
typedef struct {                   /* one submit; reads is owned by the handle until its next submit / destroy, op_n until the submit after the next */
    uint32_t struct_size;          /* sizeof(pg_realign_reads), set by the caller */
    uint32_t reserved;
    uint64_t n_reads, n_ops;
    const uint32_t *op_n;          /* DEVICE memory, laid out exactly as the batch's op_n: a pg_batch may point at it */
    const pg_realign_read *reads;  /* host [n_reads] */
} pg_realign_reads;
pg_status pg_realign_create(const pg_realign_params *params, int32_t device, pg_realign **out);
void      pg_realign_destroy(pg_realign *h);
const char *pg_realign_last_error(const pg_realign *h); /* h may be NULL: error of the last failed pg_realign_create */
/* levels and kmer_size as pg_fit_set_model takes them */
pg_status pg_realign_set_model(pg_realign *h, const uint32_t *levels, uint32_t kmer_size);
/* The kernels and copies of the following calls go to a caller-owned HIP stream (hipStream_t as void*); NULL restores the handle's own. */
pg_status pg_realign_set_stream(pg_realign *h, void *hip_stream);
/* The pinned period's phase for the following submits (pg_realign_params.phase), so that one handle serves rounds that alternate it: the
 * boundaries a round with phase 0 pins, at multiples of 256, are free in a round with phase 128. PG_ERR_INVALID_ARG above 255. Not while
 * a submit runs. */
pg_status pg_realign_set_phase(pg_realign *h, uint32_t phase);
/* One batch, synchronous. The batch as pg_fit_submit takes it (PG_BATCH_ALL_MATCHES; an I, a D or an unknown op: PG_ERR_INVALID_ARG, the
 * handle stays usable; at most 2^28 samples). status, a, b: host arrays [n_reads] of pg_fit_reads. A read with PG_FIT_ST_OK whose ops leave
 * its samples, or whose a or b is no fit's (b not a finite positive number), fails the batch with PG_ERR_INVALID_ARG before any kernel
 * indexes the signal. A handle has two output arrays and alternates them: the batch's op_n may be the op_n the handle's previous submit
 * returned (rounds: fit the refined ops, realign them again), and that array stays valid until the submit after this one.
 * With PG_BATCH_GAPPED (as pg_fit_submit takes it): an I or a D is never refinable, so both boundaries beside it are pinned, and a D has no
 * samples between them; the refined ops keep op_t and the op_n of every I and D; the pinned period counts ops. A read with
 * PG_FIT_ST_OK whose slice has not as many bases as its ops have columns fails the batch like one whose ops leave its samples. */
pg_status pg_realign_submit(pg_realign *h, const pg_batch *batch, const uint32_t *status, const double *a, const double *b, pg_realign_reads *out);
/* HIP-event time of the alignment kernel since create or the last call of this */
pg_status pg_realign_kernel_ms(pg_realign *h, double *ms);
/* Host only, no device needed: the rule for one fitted read, the recurrence over all pairs of candidates as stated above. seq: lb bases,
 * op_n: lb ops, sig: the read's n_sig samples. op_out[lb] gets the refined ops. PG_ERR_INPUT: the ops leave the samples. */
pg_status pg_realign_walk(const pg_realign_params *params, const uint32_t *levels, uint32_t kmer_size, const uint8_t *seq, uint32_t lb, const uint32_t *op_n, int64_t query_start,
                          const int16_t *sig, uint64_t n_sig, double a, double b, uint32_t *op_out, pg_realign_read *out);
/* The same for one read of a PG_BATCH_GAPPED batch: seq is its reference slice of n_seq bases, op_t its op codes. op_out keeps the op_n of
 * every I and D. PG_ERR_INPUT: the ops leave the samples, or the slice has not as many bases as the ops have columns (such a read has no
 * fit); PG_ERR_INVALID_ARG: an op code above 2. */
pg_status pg_realign_walk_gapped(const pg_realign_params *params, const uint32_t *levels, uint32_t kmer_size, const uint8_t *seq, uint64_t n_seq, const uint32_t *op_n,
                                 const uint8_t *op_t, uint32_t lb, int64_t query_start, const int16_t *sig, uint64_t n_sig, double a, double b, uint32_t *op_out,
                                 pg_realign_read *out);

/* ---- eventalign: one row per counted event against the k-mer model ---------------------------------------------------------------------------
 * The per-event view of what fit sums up: for every event that fit counts, of every read whose fit is PG_FIT_ST_OK, where it lies, its
 * level and spread in the model's units, the model's level and level_stdv for its k-mer and the standardized level. Input: a batch as
 * pg_fit_submit takes it (PG_BATCH_ALL_MATCHES or PG_BATCH_GAPPED), and per read the status, a and b that pg_fit_submit returned for this
 * same batch under the same model, sig_move_offset, rna, min_dur and max_dur -- as pg_realign_submit takes them. The events are the
 * basecaller's segmentation (refined by realign where the caller ran it), not f5c's; the columns are nanopolish / f5c
 * `eventalign --scale-events --signal-index`.
 * Per event of n raw samples r_i, with L and SD its k-mer's level and level_stdv in 1e-3 pA: u_i = 1000 r_i; m_raw the mean and s_raw the
 * sample standard deviation (0 for n = 1) of the u_i, each rounded to the nearest unit with halves up, in integers; per read
 * A = 1000.0 * a, G = (1.0 / b) / 1000.0; mean_u = llrint(((double)m_raw - A) * G), stdv_u = llrint((double)s_raw * G), the products cut
 * to +-2^21 first; z_c = floor((200 (mean_u - L) + SD) / (2 SD)), hundredths of a standard deviation. Rows are ordered by (read, event)
 * and dense; nothing depends on the device's scheduling. No CPU fallback: PG_ERR_NO_DEVICE without a GPU (pg_evalign_walk is the rule on
 * the host, for tests). */
typedef struct pg_evalign pg_evalign;
enum { PG_EVALIGN_TEXT = 1u << 0,       /* the text is produced (a header line, then one line per row) */
       PG_EVALIGN_HOST_ROWS = 1u << 1 };/* pg_evalign_out.rows_host is filled */
typedef struct {
    uint32_t struct_size;          /* sizeof(pg_evalign_params) */
    uint32_t sig_move_offset;      /* -m            at most 64 */
    uint32_t min_dur, max_dur;     /* --min_dur, --max_dur: 1 <= min_dur <= max_dur <= 4096 */
    int32_t  rna;                  /* --rna */
    uint32_t sample_rate;          /* --sample_rate: 0 = event_length in samples; 1 .. 10^6 = in seconds, five decimals */
    uint32_t flags;                /* PG_EVALIGN_* */
} pg_evalign_params;
typedef struct {                   /* one row, 40 bytes */
    uint32_t read, event;          /* the read's index in the batch; the op's index in its read */
    uint64_t start;                /* the event's first sample, counted in the read's signal */
    uint32_t n, slot, first;       /* samples; the k-mer's rank in ACGT order; its first base in the read's seq */
    int32_t  mean_u, stdv_u, z_c;  /* 1e-3 pA, 1e-3 pA, hundredths */
} pg_evalign_row;
typedef struct {                   /* per read, host arrays [n_reads]; any pointer may be NULL for its default */
    const int64_t  *ref_start;     /* forward-strand 0-based coordinate of the leftmost contig base the read's seq covers; NULL: 0 */
    const uint8_t  *reverse;       /* non-zero: a reverse-strand read; NULL: forward */
    const uint8_t  *contig;        /* the reads' contig strings back to back, contig_off[n_reads + 1]; NULL: empty */
    const uint64_t *contig_off;
    const uint8_t  *label;         /* the read_index column, label_off[n_reads + 1]; NULL: the decimal index of the read in the batch */
    const uint64_t *label_off;
} pg_evalign_meta;
typedef struct {                   /* one submit; everything is owned by the handle and valid until its next submit / destroy */
    uint32_t struct_size;          /* sizeof(pg_evalign_out), set by the caller */
    uint32_t reserved;
    uint64_t n_reads, n_rows;
    const uint64_t *row_off;       /* host [n_reads + 1]: read r has the rows [row_off[r], row_off[r + 1]) */
    const pg_evalign_row *rows;    /* DEVICE memory [n_rows] */
    const pg_evalign_row *rows_host; /* host [n_rows] with PG_EVALIGN_HOST_ROWS, else NULL */
    const char *text;              /* DEVICE memory [text_bytes] with PG_EVALIGN_TEXT, else NULL */
    uint64_t text_bytes;
} pg_evalign_out;
pg_status pg_evalign_create(const pg_evalign_params *params, int32_t device, pg_evalign **out);
void      pg_evalign_destroy(pg_evalign *h);
const char *pg_evalign_last_error(const pg_evalign *h); /* h may be NULL: error of the last failed pg_evalign_create */
/* levels as pg_fit_set_model takes them; stdvs: host uint32[4^kmer_size], level_stdv in 1e-3 pA, below 2^18. A k-mer with a level and a
 * level_stdv of 0 refuses the model (PG_ERR_INPUT): the handle then has no model, and a submit fails with PG_ERR_INPUT until one is set. */
pg_status pg_evalign_set_model(pg_evalign *h, const uint32_t *levels, const uint32_t *stdvs, uint32_t kmer_size);
/* The kernels and copies of the following calls go to a caller-owned HIP stream (hipStream_t as void*); NULL restores the handle's own. */
pg_status pg_evalign_set_stream(pg_evalign *h, void *hip_stream);
/* One batch, synchronous. status, a, b: host arrays [n_reads] of pg_fit_reads; meta may be NULL. Refused, the handle staying usable: both
 * batch flags or neither, an op code above 2 (an op that is no match in a PG_BATCH_ALL_MATCHES batch), a read with PG_FIT_ST_OK whose ops
 * leave its samples or whose a, b are no fit's (PG_ERR_INVALID_ARG); more than 2^28 samples of signal (PG_ERR_UNSUPPORTED). */
pg_status pg_evalign_submit(pg_evalign *h, const pg_batch *batch, const uint32_t *status, const double *a, const double *b, const pg_evalign_meta *meta, pg_evalign_out *out);
/* The last submit's text into a host buffer of the caller's (cap >= text_bytes) */
pg_status pg_evalign_copy_text(pg_evalign *h, char *dst, uint64_t cap);
/* HIP-event time of the three stages (count, rows, text: lengths + scan + write) since create or the last call of this; ms: double[3] */
pg_status pg_evalign_kernel_ms(pg_evalign *h, double *ms);
/* Host only, no device needed: the rule for one fitted read. seq: its lb bases, op_n: lb ops, sig: its n_sig samples. rows_out (cap
 * entries) gets the rows, `read` 0; *n_rows their number (also when cap is too small: PG_ERR_INVALID_ARG then). PG_ERR_INPUT: the ops
 * leave the samples, or a k-mer with a level has a level_stdv of 0. */
pg_status pg_evalign_walk(const pg_evalign_params *params, const uint32_t *levels, const uint32_t *stdvs, uint32_t kmer_size, const uint8_t *seq, uint32_t lb, const uint32_t *op_n,
                          int64_t query_start, const int16_t *sig, uint64_t n_sig, double a, double b, pg_evalign_row *rows_out, uint64_t cap, uint64_t *n_rows);
/* The same for one read of a PG_BATCH_GAPPED batch: seq is its reference slice of n_seq bases, op_t its op codes. PG_ERR_INPUT also when
 * the slice has not as many bases as the ops have columns; PG_ERR_INVALID_ARG: an op code above 2. */
pg_status pg_evalign_walk_gapped(const pg_evalign_params *params, const uint32_t *levels, const uint32_t *stdvs, uint32_t kmer_size, const uint8_t *seq, uint64_t n_seq,
                                 const uint32_t *op_n, const uint8_t *op_t, uint32_t lb, int64_t query_start, const int16_t *sig, uint64_t n_sig, double a, double b,
                                 pg_evalign_row *rows_out, uint64_t cap, uint64_t *n_rows);
/* Host only: the line of one row as the device writes it. contig / label: the read's strings; kmer: the kmer_size letters of the read's seq
 * at row->first; n_seq: the bases of the read's seq. Returns the bytes the line has; they are written when cap holds them. */
uint64_t  pg_evalign_row_text(const pg_evalign_row *row, const uint8_t *contig, uint32_t contig_len, const uint8_t *label, uint32_t label_len, const uint8_t *kmer,
                              uint32_t kmer_size, uint64_t n_seq, int64_t ref_start, int32_t reverse, uint32_t sample_rate, uint32_t level, uint32_t stdv, char *dst, uint64_t cap);

/* ---- simulate: raw signal and its true alignment drawn from a k-mer model --------------------------------------------------------------------
 * The generative direction of fit's rule, the project's own (not squigulator's algorithm). Random numbers are Philox4x32-10 with the key
 * (seed low, seed high) and the counter (i, stream, read low, read high), read = first_read + r: stream 0 per read, stream 1 the dwell of
 * op i, stream 2 sample i of the read -- every draw is addressed, so the result does not depend on how reads are cut into batches.
 * Per slot (a k-mer's rank in ACGT order) a level and a stdv in 1e-3 pA (0 < level < 2^18, 0 = no level; 0 <= stdv < 2^18) and a dwell of
 * 1 to 4096 samples. A read of Lb bases has Lb events; event e takes the slot of the k-mer at i = clamp(e - sig_move_offset, 0, Lb - k):
 * seq[i, i + k), or seq[Lb - i - k, Lb - i) with rna; U reads as T. Refused, in this order: Lb < k (too_short), a letter outside ACGTU
 * (bad_base), an event whose k-mer has no level (no_level); a refused read has no ops and no samples.
 * Dwell of event e, D the slot's: w = D spread_pct div 100, lo = max(1, D - w), hi = D + w, n_e = lo + ((x0 (hi - lo + 1)) >> 32), x0 of
 * stream 1, i = e. The signal is `lead` samples under (lead_level, lead_stdv), then the events back to back (query_start = lead). Sample j
 * of the read under level l and spread s: G = the sum of the 12 bytes of x0, x1, x2 of stream 2, i = j, minus 1530;
 * v = l + floor((s G + 128) / 256); t = (v Q + 2^31) >> 32; raw = clamp(t - off_r, -32768, 32767), with
 * Q = floor((digitisation 10 2^32 + range_e4 div 2) / range_e4) per run and off_r = offset - off_spread + ((x0 (2 off_spread + 1)) >> 32),
 * x0 of stream 0, i = 0, per read. All of it is integer arithmetic. No CPU fallback for pg_sim_generate: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_sim pg_sim;
enum { PG_SIM_ST_OK = 0, PG_SIM_ST_TOO_SHORT = 1, PG_SIM_ST_BAD_BASE = 2, PG_SIM_ST_NO_LEVEL = 3 };
typedef struct {
    uint32_t struct_size;          /* sizeof(pg_sim_params) */
    uint32_t kmer_size;            /* -k            1 to 9 */
    uint32_t sig_move_offset;      /* -m            at most 64 */
    int32_t  rna;                  /* --rna */
    uint64_t seed;                 /* --seed */
    uint64_t range_e4;             /* --range in 1e-4 pA, above 0; Q (above) must stay below 2^40 */
    uint32_t digitisation;         /* --digitisation  1 to 65536 */
    int32_t  offset;               /* --offset        within +-2^20 */
    uint32_t off_spread;           /* --offset_spread at most 65536 */
    uint32_t spread_pct;           /* --dwell_spread  0 to 100 */
    uint32_t lead;                 /* --lead          samples in front of the first event, at most 2^20 */
    uint32_t lead_level, lead_stdv;/* in 1e-3 pA, below 2^18 */
    uint32_t reserved;
} pg_sim_params;
typedef struct {
    uint32_t struct_size;          /* sizeof(pg_sim_batch) */
    int32_t  location;             /* PG_LOC_HOST or PG_LOC_DEVICE: seq and seq_off */
    uint32_t n_reads, reserved;
    uint64_t first_read;           /* the global number of read 0 */
    const uint8_t  *seq;           /* ASCII, the reads 5'->3' as they pass the pore (3'->5' text with rna is the caller's business: see rna above) */
    const uint64_t *seq_off;       /* [n_reads + 1] */
} pg_sim_batch;
typedef struct {                   /* one generate: DEVICE arrays laid out as the arrays of the same names of a pg_batch, op_t all 0 (the batch may be
                                    * submitted with PG_BATCH_ALL_MATCHES), complete when the call returns, valid until the next pg_sim_generate or
                                    * pg_sim_destroy on the handle. seq and seq_off are the caller's own arrays for a PG_LOC_DEVICE batch. */
    uint32_t struct_size, reserved;/* sizeof(pg_sim_result), set by the caller */
    uint64_t n_reads, n_ops, n_samples, n_seq, n_refused;
    const int16_t  *sig;           /* 16-byte aligned, 16 bytes of zeros behind the last sample */
    const uint64_t *sig_off;
    const double   *digitisation, *offset, *range; /* offset = off_r of the read */
    const int32_t  *query_start, *target_start, *target_end; /* lead (0 for a refused read); 0 and Lb, or Lb and 0 with rna, as pg_mvops_expand */
    const uint8_t  *seq;
    const uint64_t *seq_off;
    const uint32_t *op_n;
    const uint8_t  *op_t;
    const uint64_t *op_off;
    const uint32_t *status;        /* PG_SIM_ST_* */
    const uint32_t *status_host;   /* the same on the host */
} pg_sim_result;
/* A parameter outside its bounds is refused here (PG_ERR_INVALID_ARG), before a device is asked for. */
pg_status pg_sim_create(const pg_sim_params *params, int32_t device, pg_sim **out);
void      pg_sim_destroy(pg_sim *h);
const char *pg_sim_last_error(const pg_sim *h); /* h may be NULL: error of the last failed pg_sim_create */
/* The kernels and copies of the following calls go to a caller-owned HIP stream (hipStream_t as void*); NULL restores the handle's own. */
pg_status pg_sim_set_stream(pg_sim *h, void *hip_stream);
void     *pg_sim_stream(const pg_sim *h);
/* levels, stdvs, dwells: host uint32[4^kmer_size], kmer_size the handle's. The stdvs are used as they are: a caller that scales the noise
 * does it beforehand, stdv <- (stdv noise_q8 + 128) >> 8; all 0 is an ideal signal. */
pg_status pg_sim_set_model(pg_sim *h, const uint32_t *levels, const uint32_t *stdvs, const uint32_t *dwells, uint32_t kmer_size);
/* One batch, synchronous. More than 2^28 samples in all: PG_ERR_UNSUPPORTED, nothing of that size is allocated, the handle stays usable. */
pg_status pg_sim_generate(pg_sim *h, const pg_sim_batch *batch, pg_sim_result *out);
/* HIP-event time of the two kernels since create or the last call of this (either pointer may be NULL) */
pg_status pg_sim_kernel_ms(pg_sim *h, double *ops_ms, double *emit_ms);
/* Host only, no device needed: the rule for one read (its global number `read`), for tests. op_out[lb] gets the ops, *n_samples the
 * samples, sig_out gets them if sig_cap holds them all, *off_r (may be NULL) the read's offset; a refused read has neither. */
pg_status pg_sim_walk(const pg_sim_params *params, const uint32_t *levels, const uint32_t *stdvs, const uint32_t *dwells, const uint8_t *seq, uint32_t lb, uint64_t read,
                      uint32_t *op_out, int16_t *sig_out, uint64_t sig_cap, uint64_t *n_samples, uint32_t *status, int32_t *off_r);
/* Host only. pg_fit_parse_model with level_stdv kept: rounded to 1e-3 pA with halves up, exactly, on the decimal text; a row without a
 * level_stdv, or with one that is no number or outside [0, 262.144) pA, refuses the model. */
pg_status pg_sim_parse_model(const char *text, size_t n, uint32_t want_k, uint32_t *kmer_size_out, uint32_t *levels_out, uint32_t *stdvs_out, size_t cap_slots, int32_t *uses_u,
                             char *err, size_t err_cap);
/* Host only. The file `poregen model --dwell_model` writes: rows KMER<TAB>median, a median that ends in .5 is rounded up; a row with an
 * empty or "nan" median is skipped. dwells_out (cap_slots >= 4^k): 0 for a k-mer the file does not give. PG_ERR_INPUT: refused as a whole
 * (a median that is no number or outside 1 to 4096, a k-mer twice, a letter outside ACGTU, two lengths, no k-mer), err names the line. */
pg_status pg_sim_parse_dwell(const char *text, size_t n, uint32_t want_k, uint32_t *kmer_size_out, uint32_t *dwells_out, size_t cap_slots, char *err, size_t err_cap);

/* ---- svb-zd signal blocks encoded on the device -----------------------------------------------------------------------------------
 * The block of a read of n int16 samples (the layout pg_sigdec_* reads) is the shortest one, which is what slow5lib writes:
 * d_i = s_i - s_{i-1} in int32 from s_{-1} = 0, v_i = (d_i << 1) ^ (d_i >> 31), each v_i in the fewest of 1, 2 or 3 little-endian bytes
 * (int16 samples cannot give a 4-byte value), the unused bits of the last control byte 0 and nothing behind the data bytes; n = 0 is the
 * 4-byte block. The blocks of a batch lie back to back in read order, at whatever byte offsets that gives.
 * No CPU fallback: PG_ERR_NO_DEVICE without a GPU. */
typedef struct pg_sigenc pg_sigenc;
typedef struct {
    uint32_t struct_size, reserved;/* sizeof(pg_sigenc_result), set by the caller */
    uint64_t n_block_bytes;        /* = block_off[n_reads] */
    const uint8_t *blocks;         /* DEVICE memory of the handle: complete when the call returns, valid until the next pg_sigenc_encode or
                                    * pg_sigenc_destroy on the handle */
    const uint64_t *block_off;     /* HOST memory of the handle, n_reads + 1 offsets into blocks, valid as long. blocks, n_block_bytes and
                                    * block_off are directly usable as a pg_svb_batch with PG_LOC_DEVICE. */
} pg_sigenc_result;
pg_status pg_sigenc_create(int32_t device, pg_sigenc **out);
void      pg_sigenc_destroy(pg_sigenc *h);
const char *pg_sigenc_last_error(const pg_sigenc *h); /* h may be NULL: error of the last failed pg_sigenc_create */
/* Run on a caller-owned hipStream_t (waits for the work the handle has on the stream in use first); NULL restores the handle's own. */
pg_status pg_sigenc_set_stream(pg_sigenc *h, void *hip_stream);
void     *pg_sigenc_stream(const pg_sigenc *h);
/* Host only. No batch with these offsets encodes to more bytes: the sum of 4 + ceil(n / 4) + 3 n over its reads. UINT64_MAX for
 * offsets that decrease (or null offsets with n_reads > 0). */
uint64_t  pg_sigenc_bound(const uint64_t *sig_off, uint64_t n_reads);
/* Read r is sig[sig_off[r] ... sig_off[r + 1]); sig_off is host memory, n_reads + 1 non-decreasing offsets. location says where sig
 * lies: PG_LOC_HOST, any host memory (copied to a buffer of the handle), or PG_LOC_DEVICE, memory of the handle's device, complete
 * before the call; it is read in place. Returns when the blocks are there. Refused before anything is allocated: offsets that decrease
 * (PG_ERR_INPUT), a read of more than 2^32 - 1 samples, more than 2^28 samples in one call (both PG_ERR_UNSUPPORTED: encode fewer
 * reads at a time); the handle stays usable. */
pg_status pg_sigenc_encode(pg_sigenc *h, const int16_t *sig, const uint64_t *sig_off, uint64_t n_reads, int32_t location, pg_sigenc_result *out);
/* HIP-event time of the sizes kernel and of the emit kernel since the last call of this function, in ms. */
pg_status pg_sigenc_kernel_ms(pg_sigenc *h, double *lens_ms, double *emit_ms);


#ifdef __cplusplus
}
#endif
#endif
