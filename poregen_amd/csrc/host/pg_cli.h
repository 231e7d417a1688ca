// pg_cli.h -- what the subcommands that run on the device share besides the file readers (pg_host.h): the error exit, option values,
// file suffixes, the HIP check, and for `fit` and `realign` the model, the batch handed to pg_fit_* and the per-k-mer table; the rounds of
// fit and realign that `realign --rounds` and `gmove --reform --realign` share; the --ref route (RefRoute) that `gmove --reform --ref`,
// `fit --ref` and `realign --ref` share.
// (`transform` words its errors its own way and is built without HIP: it does not include this.)
#pragma once
#include "../../../include/pgmove.h"
#include "../pg_fit.h"
#include "../pg_hip_host.h"
#include "pg_host.h"
#include "pg_moverecs.h"

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
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
// the model: parsed and refused on the host, before any device is touched. levels gets 4^PG_FIT_MAX_K entries. stdvs (may be null): the
// level_stdv column is kept too, in 1e-3 pA; a row without one, or a k-mer whose level_stdv rounds to 0, then refuses the model.
inline bool load_level_model(const char *tool, const char *path, long long k_opt, std::vector<uint32_t> &levels, uint32_t &k, int32_t &uses_u, std::vector<uint32_t> *stdvs = nullptr) {
    pgh::MappedFile mf;
    if (!mf.open(path)) { fprintf(stderr, "[%s] cannot open the model %s\n", tool, path); return false; }
    levels.assign((size_t)1 << (2 * PG_FIT_MAX_K), 0);
    char perr[400];
    if (!stdvs) {
        if (pg_fit_parse_model(mf.data, mf.size, (uint32_t)k_opt, &k, levels.data(), levels.size(), &uses_u, perr, sizeof perr) == PG_OK) return true;
    } else {
        stdvs->assign(levels.size(), 0);
        if (pg_sim_parse_model(mf.data, mf.size, (uint32_t)k_opt, &k, levels.data(), stdvs->data(), levels.size(), &uses_u, perr, sizeof perr) == PG_OK) {
            for (uint64_t s = 0; s < (1ull << (2 * k)); s++)
                if (levels[s] && !(*stdvs)[s]) {
                    std::string name(k, 'A');
                    for (uint32_t j = 0; j < k; j++) name[j] = "ACGT"[(s >> (2 * (k - 1 - j))) & 3];
                    fprintf(stderr, "[%s] the model %s is refused: the level_stdv of %s is 0 after rounding to 0.001 pA\n", tool, path, name.c_str());
                    return false;
                }
            return true;
        }
    }
    fprintf(stderr, "[%s] the model %s is refused: %s\n", tool, path, perr);
    return false;
}

// a read's status as the tables print it: fit's own, or the code of the expansion for a read reform refuses (PG_FIT_ST_SKIPPED + code)
inline const char *fit_status_name(uint32_t st) {
    static const char *const kFit[] = {"ok", "out_of_signal", "too_long", "few_events", "flat", "negative_scale", "ref_length"};
    static const char *const kReform[] = {"", "no_move_in_table", "negative_tail", "bases_left_over", "bad_stride"};
    if (st < 7) return kFit[st];
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

// ---- the --ref route that `gmove --reform --ref`, `fit --ref` and `realign --ref` share ----------------------------------------------------
// Per batch, behind pg_mvops_expand: the ops are carried through the records' CIGARs onto the reference on the expander
// (pg_mvops_project[_stranded]), and every read's slice of the FASTA is fetched -- on the host (faidx_fetch_seq over the target columns,
// as the PAF front-end does it), or with --both_strands cut on the device (pg_refseq_slice), reversed and complemented for a
// reverse-strand record. The records that are not taken are skipped and counted by pgh::next_move_record.
struct RefRoute {
    pgh::FastxIndex fai;
    bool both_strands = false, rna = false;
    uint64_t skipped = 0, reverse_taken = 0;   // the counters next_move_record fills
    pg_mvops_projection pr;                    // the last batch's projection: the expander's arrays, until its next project
    uint64_t n_ops = 0, n_seq = 0;             // the last batch's ops and bases
    std::vector<uint8_t> h_seq; std::vector<uint64_t> h_seqoff; // the slices on the host (without --both_strands)
    const uint8_t *d_seq = nullptr; const uint64_t *d_seqoff = nullptr; // --both_strands: the slices on the device, the refseq handle's until its next batch
    pg_refseq *refseq = nullptr;
    std::unordered_map<std::string, int32_t> contig_index;
    std::vector<int32_t> contig, clen; std::vector<uint8_t> reverse;
    std::string slice;
    RefRoute() { memset(&pr, 0, sizeof pr); }
    ~RefRoute() { release(); }
    RefRoute(const RefRoute &) = delete; RefRoute &operator=(const RefRoute &) = delete;
    void release() { if (refseq) { pg_refseq_destroy(refseq); refseq = nullptr; } }
    uint64_t *skipped_counter() { return &skipped; }
    uint64_t *reverse_counter() { return both_strands ? &reverse_taken : nullptr; }
    void print_skipped(const char *tool) const {
        if (both_strands) pgh::print_both_strands_skipped(tool, skipped, reverse_taken); else pgh::print_to_ref_skipped(tool, skipped);
    }
    // The projection of the first n records of rb, expanded into mr on ex. A record reform --to_ref ends on cuts the batch in front of
    // it: n shrinks and `bad` gets reform's line. false: the library's error is on stderr.
    bool project(const char *tool, pg_mvops *ex, const pgh::MoveRecs &rb, const pg_mvops_result &mr, size_t &n, std::string &bad, bool &cut) {
        pg_mvops_cigars cg; memset(&cg, 0, sizeof cg);
        cg.n_reads = n; cg.location = PG_LOC_HOST; cg.flags = rna ? PG_MVOPS_RNA : 0;
        cg.op_n = mr.op_n; cg.n_ops = mr.n_ops; cg.op_off = mr.op_off; cg.query_start = mr.query_start; cg.status = mr.status;
        cg.cigar = rb.cigar.data(); cg.n_cigar = rb.cigar_off[n]; cg.cigar_off = rb.cigar_off.data(); cg.pos = rb.pos.data();
        pg_mvops_strands strands; memset(&strands, 0, sizeof strands);
        if (both_strands) { // the strand from the flag, the contig's length from the header, as reform --to_ref --both_strands has them
            reverse.resize(n); clen.resize(n);
            for (size_t i = 0; i < n; i++) { reverse[i] = (rb.flag[i] & 0x10u) ? 1 : 0; clen[i] = pgh::contig_len_of(rb.ref_len[i]); }
            strands.reverse = reverse.data(); strands.contig_len = clen.data();
        }
        cut = false;
        if (pg_mvops_project_stranded(ex, &cg, both_strands ? &strands : nullptr, &pr) != PG_OK) { fprintf(stderr, "[%s] %s\n", tool, pg_mvops_last_error(ex)); return false; }
        if (pr.first_refused >= 0) { // reform --to_ref ends on this record: the reads in front of it are the batch
            n = (size_t)pr.first_refused; cut = true;
            const uint32_t code = pr.status_host[n];
            bad = pgh::reform_error((std::string(pgh::to_ref_refusal(code)) + " (status " + std::to_string(code) + ")").c_str(), rb.names[n]);
        }
        return true;
    }
    // The slices of the first n records (behind project), and n_ops / n_seq. false: the error is on stderr (HIP's through hip_ok).
    bool slices(const char *tool, const HipOk &hip_ok, int device, hipStream_t xs, const pgh::MoveRecs &rb, size_t n) {
        n_ops = n_seq = 0; d_seq = nullptr; d_seqoff = nullptr;
        if (!n) return true;
        if (both_strands) {
            if (!refseq && pg_refseq_create(device, &refseq) != PG_OK) { fprintf(stderr, "[%s] %s\n", tool, pg_refseq_last_error(nullptr)); *hip_ok.status = EXIT_FAILURE; return false; }
            contig.resize(n);
            bool ok = pg_refseq_set_stream(refseq, xs) == PG_OK;
            for (size_t i = 0; ok && i < n; i++) {
                auto it = contig_index.find(rb.rname[i]);
                if (it == contig_index.end()) {
                    int32_t idx = -1; // the whole contig, its line ends stripped; a name the FASTA does not hold stays -1
                    if (fai.fetch(rb.rname[i], 0, INT64_MAX / 4, slice)) ok = pg_refseq_add(refseq, (const uint8_t *)slice.data(), slice.size(), &idx) == PG_OK;
                    it = contig_index.emplace(rb.rname[i], idx).first;
                }
                contig[i] = it->second;
            }
            pg_refseq_reads rr; memset(&rr, 0, sizeof rr);
            rr.n_reads = n; rr.location = PG_LOC_HOST; rr.contig = contig.data(); rr.pos = rb.pos.data(); rr.ref_len = pr.ref_len_host; rr.reverse = reverse.data();
            pg_refseq_slices rsl; memset(&rsl, 0, sizeof rsl);
            if (!ok || pg_refseq_slice(refseq, &rr, &rsl) != PG_OK) { fprintf(stderr, "[%s] %s\n", tool, pg_refseq_last_error(refseq)); *hip_ok.status = EXIT_FAILURE; return false; }
            n_seq = rsl.n_seq; d_seq = rsl.seq; d_seqoff = rsl.seq_off;
        } else {
            // faidx_fetch_seq(m_fai, tid, st_k, end_k - 1) with st_k / end_k = min / max of the target columns, as the PAF front-end
            // does it; a name the FASTA does not hold gives an empty slice, and the device skips the read
            h_seq.clear(); h_seqoff.assign(1, 0);
            for (size_t i = 0; i < n; i++) {
                const int32_t lo = rb.pos[i], hi = (int32_t)((uint32_t)rb.pos[i] + pr.ref_len_host[i]);
                const int64_t a = rna ? hi : lo, b2 = rna ? lo : hi;
                const int64_t st_k = (uint64_t)a > (uint64_t)b2 ? b2 : a, end_k = (uint64_t)a > (uint64_t)b2 ? a : b2;
                fai.fetch(rb.rname[i], (int)st_k, (int)(end_k - 1), slice);
                h_seq.insert(h_seq.end(), slice.begin(), slice.end()); h_seqoff.push_back(h_seq.size());
            }
            n_seq = h_seq.size();
        }
        return hip_ok(hipMemcpy(&n_ops, pr.op_off + n, sizeof n_ops, hipMemcpyDeviceToHost), "hipMemcpy");
    }
    // The slices in the caller's own device buffers, on stream xs, complete when this returns (two batches may be in flight).
    bool to_device(const HipOk &hip_ok, hipStream_t xs, size_t n, PgDev<uint8_t> &seq, PgDev<uint64_t> &seq_off) {
        const void *src = both_strands ? (const void *)d_seq : (const void *)h_seq.data(), *src_off = both_strands ? (const void *)d_seqoff : (const void *)h_seqoff.data();
        const hipMemcpyKind kind = both_strands ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        return hip_ok(seq.ensure(n_seq ? n_seq : 1, n_seq + n_seq / 4 + 256), "hipMalloc") && hip_ok(seq_off.ensure((n + 1) * 8, (n + 1) * 10), "hipMalloc") &&
               (!n_seq || hip_ok(hipMemcpyAsync(seq.p, src, n_seq, kind, xs), "hipMemcpyAsync")) && hip_ok(hipMemcpyAsync(seq_off.p, src_off, (n + 1) * 8, kind, xs), "hipMemcpyAsync") &&
               hip_ok(hipStreamSynchronize(xs), "hipStreamSynchronize");
    }
    // the batch fit and realign take: the projection's ops over the slices in `seq` / `seq_off` (to_device), flagged PG_BATCH_GAPPED
    pg_batch gapped_batch(size_t n, const int16_t *sig, const uint64_t *sig_off, const uint8_t *seq, const uint64_t *seq_off) const {
        pg_batch b; memset(&b, 0, sizeof b);
        b.struct_size = sizeof b; b.location = PG_LOC_DEVICE; b.n_reads = (uint32_t)n; b.n_ops = (uint32_t)n_ops;
        b.sig = sig; b.sig_off = sig_off; b.query_start = pr.query_start; b.target_start = pr.target_start; b.target_end = pr.target_end;
        b.seq = seq; b.seq_off = seq_off; b.op_n = pr.op_n; b.op_t = pr.op_t; b.op_off = pr.op_off;
        b.flags = PG_BATCH_GAPPED;
        return b;
    }
};
