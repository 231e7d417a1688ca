// pg_cli.h -- what the subcommands that run on the device share besides the file readers (pg_host.h): the error exit, option values,
// file suffixes, the HIP check, and for `fit` and `realign` the model, the batch handed to pg_fit_* and the per-k-mer table; the rounds of
// fit and realign that `realign --rounds` and `gmove --reform --realign` share.
// (`transform` words its errors its own way and is built without HIP: it does not include this.)
#pragma once
#include "../../../include/pgmove.h"
#include "../pg_fit.h"
#include "../pg_hip_host.h"
#include "pg_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

inline int die(const char *fmt, const std::string &a = "") { fprintf(stderr, fmt, a.c_str()); fputc('\n', stderr); return EXIT_FAILURE; }

// a whole number in [min, max] and nothing else; a sign only where a negative number is taken
inline bool whole_int(const char *s, long long min, long long max, long long &v) {
    char *end = nullptr;
    if (!s || !*s || *s == '+' || (*s == '-' && min >= 0)) return false;
    v = strtoll(s, &end, 10);
    return *end == 0 && v >= min && v <= max;
}

inline bool ends_with(const char *s, const char *suffix) { const size_t a = strlen(s), b = strlen(suffix); return a >= b && !strcmp(s + a - b, suffix); }
inline bool is_sam_or_bam(const char *path) { return ends_with(path, ".bam") || ends_with(path, ".sam"); }

// hip_ok(e, what): true, or "[tool] what: <HIP's text>" on stderr, *status = EXIT_FAILURE and false
struct HipOk {
    const char *tool; int *status;
    bool operator()(hipError_t e, const char *what) const {
        if (e == hipSuccess) return true;
        fprintf(stderr, "[%s] %s: %s\n", tool, what, hipGetErrorString(e)); *status = EXIT_FAILURE; return false;
    }
};

// A batch's signal to the device on `stream`, behind whatever the stream still holds of the batch before (the buffers may be freed to grow).
inline bool upload_signal(const HipOk &hip_ok, PgDev<int16_t> &d_sig, PgDev<uint64_t> &d_sigoff, const std::vector<int16_t> &sig, const std::vector<uint64_t> &sig_off, hipStream_t stream) {
    const size_t sb = sig.size() * sizeof(int16_t), ob = sig_off.size() * 8;
    return hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize") && hip_ok(d_sig.ensure(sb ? sb : 1, sb + sb / 4 + 256), "hipMalloc") &&
           hip_ok(d_sigoff.ensure(ob, ob + ob / 4), "hipMalloc") && (!sb || hip_ok(hipMemcpyAsync(d_sig.p, sig.data(), sb, hipMemcpyHostToDevice, stream), "hipMemcpyAsync")) &&
           hip_ok(hipMemcpyAsync(d_sigoff.p, sig_off.data(), ob, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
}

// the first n reads of an expansion with their uploaded signal: every op is a match and a read has as many ops as bases, what `reform` writes
inline pg_batch device_batch(const pg_mvops_result &mr, size_t n, uint64_t n_ops, const int16_t *sig, const uint64_t *sig_off) {
    pg_batch b; memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.location = PG_LOC_DEVICE; b.n_reads = (uint32_t)n; b.n_ops = (uint32_t)n_ops;
    b.sig = sig; b.sig_off = sig_off; b.query_start = mr.query_start; b.target_start = mr.target_start; b.target_end = mr.target_end;
    b.seq = mr.seq; b.seq_off = mr.seq_off; b.op_n = mr.op_n; b.op_t = mr.op_t; b.op_off = mr.op_off;
    b.flags = PG_BATCH_ALL_MATCHES;
    return b;
}

// ---- fit and realign ---------------------------------------------------------------------------------------------------------------
// the model: parsed and refused on the host, before any device is touched. levels gets 4^PG_FIT_MAX_K entries.
inline bool load_level_model(const char *tool, const char *path, long long k_opt, std::vector<uint32_t> &levels, uint32_t &k, int32_t &uses_u) {
    pgh::MappedFile mf;
    if (!mf.open(path)) { fprintf(stderr, "[%s] cannot open the model %s\n", tool, path); return false; }
    levels.assign((size_t)1 << (2 * PG_FIT_MAX_K), 0);
    char perr[400];
    if (pg_fit_parse_model(mf.data, mf.size, (uint32_t)k_opt, &k, levels.data(), levels.size(), &uses_u, perr, sizeof perr) == PG_OK) return true;
    fprintf(stderr, "[%s] the model %s is refused: %s\n", tool, path, perr);
    return false;
}

// a read's status as the tables print it: fit's own, or the code of the expansion for a read reform refuses (PG_FIT_ST_SKIPPED + code)
inline const char *fit_status_name(uint32_t st) {
    static const char *const kFit[] = {"ok", "out_of_signal", "too_long", "few_events", "flat", "negative_scale"};
    static const char *const kReform[] = {"", "no_move_in_table", "negative_tail", "bases_left_over", "bad_stride"};
    if (st < 6) return kFit[st];
    if (st > PG_FIT_ST_SKIPPED && st < PG_FIT_ST_SKIPPED + 5) return kReform[st - PG_FIT_ST_SKIPPED];
    return "refused";
}

// the rms residual of n samples with sum d^2 = hi 2^64 + lo, in pA with three decimals; empty without a sample
inline std::string rms_text(uint64_t n, uint64_t lo, uint64_t hi) {
    if (!n) return "";
    int64_t mean, rms;
    pg_fit_slot_resid(n, 0, lo, hi, mean, rms);
    return pg_fit_units_text(rms);
}
inline std::string pooled_rms(const pg_fit_result &r, uint64_t n_slots) { // over every k-mer
    unsigned __int128 dd = 0;
    for (uint64_t s = 0; s < n_slots; s++) dd += ((unsigned __int128)r.sum_dd_hi[s] << 64) | r.sum_dd_lo[s];
    return rms_text(r.samples, (uint64_t)dd, (uint64_t)(dd >> 64));
}

// The rounds of `realign --rounds` and `gmove --reform --realign` over one device batch: round t fits the ops of round t - 1 (ops_0: the
// batch's) and refines them with that fit, at phase 0 when t is odd and 128 when it is even, so that what one round pins the next one
// refines. Nothing but the ops goes from round to round. fit1 fits round 1, fit_more the rounds behind it (the same handle where nobody
// pools round 1's sums). op_n: the last round's ops, the realign handle's array, valid until the handle's submit after the next.
struct RealignRounds {
    std::vector<pg_realign_read> acc;  // per read: the counts summed over the rounds, cost_before of round 1, cost_after of the last round
    std::vector<uint32_t> status;      // per read: round 1's fit
    std::vector<uint64_t> ns_before, ns_after; // per read: the counted samples of round 1's and of the last round's fit, 0 unless that fit is ok
    const uint32_t *op_n = nullptr;
    uint64_t refined = 0, n_free = 0, n_moved = 0; // over every batch: reads round 1 fits; free and moved boundaries, summed over the rounds
    std::string err;

    bool run(pg_fit *fit1, pg_fit *fit_more, pg_realign *ra, const pg_batch &b, long long rounds) {
        const size_t n = b.n_reads;
        pg_batch cur = b;
        acc.assign(n, pg_realign_read{0, 0, 0, 0, 0, 0, 0}); status.assign(n, 0); ns_before.assign(n, 0); ns_after.assign(n, 0);
        for (long long t = 1; t <= rounds; t++) {
            pg_fit *fit = t == 1 ? fit1 : fit_more;
            pg_fit_reads f;
            pg_realign_reads rr; memset(&rr, 0, sizeof rr); rr.struct_size = sizeof rr;
            if (pg_fit_submit(fit, &cur, nullptr, &f) != PG_OK) { err = pg_fit_last_error(fit); return false; }
            if (pg_realign_set_phase(ra, t % 2 ? 0u : 128u) != PG_OK || pg_realign_submit(ra, &cur, f.status, f.a, f.b, &rr) != PG_OK) { err = pg_realign_last_error(ra); return false; }
            for (size_t i = 0; i < n; i++) {
                const pg_realign_read &q = rr.reads[i];
                pg_realign_read &o = acc[i];
                const uint64_t ns = f.status[i] == PG_FIT_ST_OK ? (uint64_t)f.sums[i].n : 0;
                o.n_free += q.n_free; o.n_moved += q.n_moved; o.sum_abs_shift += q.sum_abs_shift;
                if (t == 1) { o.cost_before_lo = q.cost_before_lo; o.cost_before_hi = q.cost_before_hi; status[i] = f.status[i]; ns_before[i] = ns; refined += f.status[i] == PG_FIT_ST_OK; }
                o.cost_after_lo = q.cost_after_lo; o.cost_after_hi = q.cost_after_hi; ns_after[i] = ns;
                n_free += q.n_free; n_moved += q.n_moved;
            }
            cur.op_n = op_n = rr.op_n;
        }
        return true;
    }
    // read_id  status  n_free  n_moved  sum_abs_shift  rms_before  rms_after
    void row(FILE *fp, const char *id, size_t i) const {
        const pg_realign_read &q = acc[i];
        fprintf(fp, "%s\t%s\t%u\t%u\t%llu\t%s\t%s\n", id, fit_status_name(status[i]), q.n_free, q.n_moved, (unsigned long long)q.sum_abs_shift,
                rms_text(ns_before[i], q.cost_before_lo, q.cost_before_hi).c_str(), rms_text(ns_after[i], q.cost_after_lo, q.cost_after_hi).c_str());
    }
};

// KMER  n_samples  n_events  level  mean_resid  rms_resid for every k-mer in ACGT order; EXIT_SUCCESS, or EXIT_FAILURE with the reason on stderr
inline int write_kmer_table(const char *path, uint32_t k, bool uses_u, const std::vector<uint32_t> &levels, const pg_fit_result &res) {
    FILE *kf = fopen(path, "w");
    if (!kf) return die("Could not open %s for writing.", path);
    std::string name(k, 'A');
    const char *alpha = uses_u ? "ACGU" : "ACGT";
    for (uint64_t s = 0; s < (1ull << (2 * k)); s++) {
        for (uint32_t j = 0; j < k; j++) name[j] = alpha[(s >> (2 * (k - 1 - j))) & 3];
        fprintf(kf, "%s\t%llu\t%llu\t%s\t", name.c_str(), (unsigned long long)res.n_samples[s], (unsigned long long)res.n_events[s], levels[s] ? pg_fit_units_text(levels[s]).c_str() : "");
        if (res.n_samples[s]) {
            int64_t mean, rms;
            pg_fit_slot_resid(res.n_samples[s], res.sum_d[s], res.sum_dd_lo[s], res.sum_dd_hi[s], mean, rms);
            fprintf(kf, "%s\t%s\n", pg_fit_units_text(mean).c_str(), pg_fit_units_text(rms).c_str());
        } else fprintf(kf, "\t\n");
    }
    return fclose(kf) == 0 ? EXIT_SUCCESS : die("Error in writing %s.", path);
}
