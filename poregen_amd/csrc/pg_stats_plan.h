// pg_stats_plan.h -- where the per-read statistics of one batch run, and who writes their records (pg_api.hip: pg_count decides once per
// batch and keeps the answer in the context; launch_stats, pg_stats, pg_collect and settle_batch read it). Host-only arithmetic, kept apart
// so that the whole truth table can be tested without a device (poregen_amd/_pg_hosttest.so: pgt_stats_plan; tests/test_host_logic.py).
// DESIGN.md 3.2 has the table of the places; the reasons for each ordering stand next to the code that queues it.
//
// The seven places:
//   NONE           scaling 0 and no PG_FLAG_SKIP_OUT_OF_RANGE: nobody reads a median or a MAD
//   OOR_FIRST      PG_FLAG_SKIP_OUT_OF_RANGE: on the chain's stream behind k_batch_init, in front of the walk, which needs their verdict
//   SECOND_STREAM  PG_FLAG_OVERLAP: on the statistics stream from the start of the batch, beside the whole counting chain; that stream
//                  writes its own records (k_read_plan) and resets its own flags
//   CHAIN          on the chain's stream behind the counting kernels: a one-stream context, and a two-stream context's batch whose
//                  statistics wait for the front's scan anyway (one_stream_batch)
//   TAIL_FORK      PG_FLAG_OVERLAP_TAIL: forked onto the second stream behind the counting kernels, beside pg_collect's small launches
//   DEFERRED       PG_FLAG_DEFER_STATS: left to pg_stats / pgi_stats_gathered / pg_collect, on the chain's stream
//   LAZY           PG_FLAG_LAZY_STATS: in pg_collect behind the emit kernel, for the reads that own a kept event only
// Beside the place: a CHAIN batch behind the cut (with_emit) leaves its statistics to pg_collect, which queues them in the launch of the rank
// emit kernel (k_emit_stats); PGMOVE_NO_EMIT_STATS keeps the two launches.
#pragma once
#include "../../include/pgmove.h"
#include <cstdint>

enum PgStatsPlace { PG_STATS_NONE = 0, PG_STATS_OOR_FIRST, PG_STATS_SECOND_STREAM, PG_STATS_CHAIN, PG_STATS_TAIL_FORK, PG_STATS_DEFERRED, PG_STATS_LAZY };

struct PgStatsPlan {
    PgStatsPlace place;
    bool behind_cut;        // eager statistics of a batch counted front first: k_read_stats reads the cut-read word the front's scan leaves
    bool one_stream_batch;  // a two-stream context's batch that is queued on the chain's stream alone (always behind_cut, always CHAIN)
    bool records_in_init;   // k_batch_init writes the statistics records: no k_read_plan
    bool flags_in_init;     // k_batch_init resets the slot's statistics flags, in front of the statistics in stream (or fork) order
    bool rare_with_scan;    // the rare workers ride in the launch of pg_collect's sample-offset scan, the next one on the chain's stream
    bool with_emit;         // CHAIN and behind_cut: pg_count leaves the statistics pending, and pg_collect queues them in the emit kernel's launch (k_emit_stats)
};

static inline bool pg_stats_on_second_stream(PgStatsPlace p) { return p == PG_STATS_SECOND_STREAM || p == PG_STATS_TAIL_FORK; }

// ctx_flags: the context's effective flags (pg_create has defaulted PG_FLAG_OVERLAP); front_tiles: the batch's front (0: counted in one
// pass); front_two_streams: PGMOVE_FRONT_TWO_STREAMS is set (tests, A/B: a front-first batch keeps the second stream); no_emit_stats:
// PGMOVE_NO_EMIT_STATS is set (tests, A/B: k_read_stats and k_rank_emit stay two launches)
static inline PgStatsPlan pg_stats_plan(uint32_t ctx_flags, int32_t scaling, uint32_t front_tiles, uint32_t n_reads, bool front_two_streams, bool no_emit_stats = false) {
    const bool skip_oor = (ctx_flags & PG_FLAG_SKIP_OUT_OF_RANGE) != 0;
    const bool lazy = !skip_oor && scaling == 1 && (ctx_flags & PG_FLAG_LAZY_STATS) != 0;
    const bool eager = skip_oor || (scaling == 1 && !lazy);
    // PG_FLAG_OVERLAP_TAIL and PG_FLAG_DEFER_STATS are ignored with PG_FLAG_OVERLAP: by the CONTEXT's flag, also on a one-stream batch
    const bool ctx_overlap = !skip_oor && (ctx_flags & PG_FLAG_OVERLAP) != 0;
    PgStatsPlan p{};
    // not with PG_FLAG_SKIP_OUT_OF_RANGE (the walk waits for the statistics' verdict), and not in a PG_FLAG_PROFILE context: its passes
    // time each kernel over the whole batch (include/pgmove.h)
    p.behind_cut = front_tiles != 0 && eager && !skip_oor && !(ctx_flags & PG_FLAG_PROFILE);
    p.one_stream_batch = ctx_overlap && p.behind_cut && !front_two_streams;
    if (skip_oor) p.place = PG_STATS_OOR_FIRST;
    else if (lazy) p.place = PG_STATS_LAZY;
    else if (!eager) p.place = PG_STATS_NONE;
    else if (ctx_overlap) p.place = p.one_stream_batch ? PG_STATS_CHAIN : PG_STATS_SECOND_STREAM;
    else if (ctx_flags & PG_FLAG_DEFER_STATS) p.place = PG_STATS_DEFERRED;
    else if (ctx_flags & PG_FLAG_OVERLAP_TAIL) p.place = PG_STATS_TAIL_FORK;
    else p.place = PG_STATS_CHAIN;
    const bool second_from_start = ctx_overlap && !p.one_stream_batch; // the batch leaves records and flags to the statistics stream
    p.records_in_init = eager && !second_from_start && n_reads > 0;
    p.flags_in_init = !second_from_start;
    p.rare_with_scan = p.place == PG_STATS_CHAIN || p.place == PG_STATS_DEFERRED || p.place == PG_STATS_LAZY;
    // a front (front_tiles != 0) means pg_submit, direct ranking, not dense, sample_limit > 0 (pg_api.hip: front_tiles_for): the emit kernel
    // that follows is k_rank_emit, on the same stream, and nothing but the counting tail stands between the two
    p.with_emit = p.place == PG_STATS_CHAIN && p.behind_cut && !no_emit_stats;
    return p;
}

// Must the statistics stream wait for the chain's stream before it takes a SECOND_STREAM batch? For a host batch (its staging copies), for
// a device batch on the caller's stream that the caller does not declare PG_BATCH_RESIDENT (its producer), and behind a one-stream batch
// (whose statistics ran on the chain's stream). pg_count has the reasons, where it queues the wait.
static inline bool pg_stats_fork_waits(bool batch_is_host, bool user_stream, bool batch_resident, bool prev_one_stream) {
    return batch_is_host || (user_stream && !batch_resident) || prev_one_stream;
}
