// fit_cli.cpp -- `poregen fit`: how well does a k-mer model explain a dataset? The reference asks other tools (scripts/eventaling.sh runs f5c
// eventalign --kmer-model, scripts/sim.sh squigulator, a basecaller and an identity script); here the question goes to the basecaller's own
// segmentation. The records are read as `gmove --reform` reads them (move arrays and packed bases to the device, pg_mvops_expand, untrimmed
// signal), every read is calibrated against the model -- sample = shift + scale * level, least squares over its counted events -- and every
// k-mer's samples are then compared with the level the model claims (pg_fit_*, include/pgmove.h; the rule: csrc/pg_fit.h).
//   per read   read_id  status  n_events  n_samples  shift  scale  rms          (the three numbers "%.6f", empty unless the status is ok)
//   per k-mer  KMER  n_samples  n_events  level  mean_resid  rms_resid           (pA with three decimals; the last two empty when n_samples is 0)
#include "../../../include/pgmove.h"
#include "../pg_fit.h"
#include "../pg_hip_host.h"
#include "pg_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <getopt.h>
#include <string>
#include <vector>

namespace {

const struct option kLongOptions[] = {
    {"rna", no_argument, nullptr, 0},              // 0
    {"n_to_t", no_argument, nullptr, 0},           // 1
    {"min_dur", required_argument, nullptr, 0},    // 2
    {"max_dur", required_argument, nullptr, 0},    // 3
    {"min_events", required_argument, nullptr, 0}, // 4
    {"kmer_table", required_argument, nullptr, 0}, // 5
    {"batch_reads", required_argument, nullptr, 0},// 6
    {"device", required_argument, nullptr, 0},     // 7
    {"help", no_argument, nullptr, 'h'},           // 8
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen fit [options] MODEL reads.slow5/blow5 reads.bam/sam\n");
    fprintf(fp, "\nscore a k-mer model against the signal and the move tables: per read sample = shift + scale * level, per k-mer the residuals\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   -k INT                     k-mer length; must be the model's [the model's]\n");
    fprintf(fp, "   -m INT                     move start offset [0]\n");
    fprintf(fp, "   --rna                      the dataset is direct RNA\n");
    fprintf(fp, "   --n_to_t                   an N of a read counts as T\n");
    fprintf(fp, "   --min_dur INT              minimum number of samples of an event [5]\n");
    fprintf(fp, "   --max_dur INT              maximum number of samples of an event [70]\n");
    fprintf(fp, "   --min_events INT           counted events a read needs to be fitted [20]\n");
    fprintf(fp, "   -o FILE                    the per-read table [stdout]\n");
    fprintf(fp, "   --kmer_table FILE          the per-k-mer table\n");
    fprintf(fp, "   --batch_reads INT          reads per device batch [4000]\n");
    fprintf(fp, "   --device INT               HIP device [0]\n");
    fprintf(fp, "   -h                         help\n");
}

int die(const char *fmt, const std::string &a = "") { fprintf(stderr, fmt, a.c_str()); fputc('\n', stderr); return EXIT_FAILURE; }

bool whole_uint(const char *s, long long max, long long &v) {
    char *end = nullptr;
    if (!s || !*s || *s == '-' || *s == '+') return false;
    v = strtoll(s, &end, 10);
    return *end == 0 && v >= 0 && v <= max;
}

const char *status_name(uint32_t st) {
    static const char *const kFit[] = {"ok", "out_of_signal", "too_long", "few_events", "flat", "negative_scale"};
    static const char *const kReform[] = {"", "no_move_in_table", "negative_tail", "bases_left_over", "bad_stride"};
    if (st < 6) return kFit[st];
    if (st > PG_FIT_ST_SKIPPED && st < PG_FIT_ST_SKIPPED + 5) return kReform[st - PG_FIT_ST_SKIPPED];
    return "refused";
}

} // namespace

int fit_main(int argc, char **argv) {
    long long k_opt = 0, m = 0, min_dur = 5, max_dur = 70, min_events = 20, batch_reads = 4000, device = 0;
    bool rna = false, n_to_t = false, help = false;
    const char *out_path = nullptr, *kmer_path = nullptr;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "k:m:o:h", kLongOptions, &longindex)) >= 0) {
        bool ok = true;
        if (c == 'k') ok = whole_uint(optarg, PG_FIT_MAX_K, k_opt) && k_opt >= 1;
        else if (c == 'm') ok = whole_uint(optarg, 64, m);
        else if (c == 'o') out_path = optarg;
        else if (c == 'h') help = true;
        else if (c == 0 && longindex == 0) rna = true;
        else if (c == 0 && longindex == 1) n_to_t = true;
        else if (c == 0 && longindex == 2) ok = whole_uint(optarg, PG_FIT_MAX_DUR, min_dur);
        else if (c == 0 && longindex == 3) ok = whole_uint(optarg, PG_FIT_MAX_DUR, max_dur);
        else if (c == 0 && longindex == 4) ok = whole_uint(optarg, 0xffffffffll, min_events);
        else if (c == 0 && longindex == 5) kmer_path = optarg;
        else if (c == 0 && longindex == 6) ok = whole_uint(optarg, 1 << 24, batch_reads) && batch_reads >= 1;
        else if (c == 0 && longindex == 7) ok = whole_uint(optarg, 1024, device);
        else { print_help(stderr); return EXIT_FAILURE; }
        if (!ok) {
            fprintf(stderr, "[fit] %s%s: '%s' is not a value it takes (-k 1..9, -m 0..64, durations 0..%u)\n", c ? "-" : "--", c ? std::string(1, (char)c).c_str() : kLongOptions[longindex].name,
                    optarg, PG_FIT_MAX_DUR);
            return EXIT_FAILURE;
        }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    if (argc - optind != 3) { print_help(stderr); return EXIT_FAILURE; }
    if (min_dur > max_dur) return die("[fit] --min_dur may not exceed --max_dur");
    const char *model_path = argv[optind], *slow5_path = argv[optind + 1], *sam_path = argv[optind + 2];
    {
        const size_t ml = strlen(sam_path);
        if (!(ml >= 4 && (!strcmp(sam_path + ml - 4, ".bam") || !strcmp(sam_path + ml - 4, ".sam")))) return die("[fit] the records come from a .bam or .sam file, not %s", sam_path);
    }
    // ---- the model: parsed and refused on the host, before any device is touched
    pgh::MappedFile mf;
    if (!mf.open(model_path)) return die("[fit] cannot open the model %s", model_path);
    std::vector<uint32_t> levels((size_t)1 << (2 * PG_FIT_MAX_K));
    uint32_t k = 0; int32_t uses_u = 0; char perr[400];
    if (pg_fit_parse_model(mf.data, mf.size, (uint32_t)k_opt, &k, levels.data(), levels.size(), &uses_u, perr, sizeof perr) != PG_OK) {
        fprintf(stderr, "[fit] the model %s is refused: %s\n", model_path, perr);
        return EXIT_FAILURE;
    }
    mf.close();
    const uint64_t n_slots = 1ull << (2 * k);
    std::string err;
    pgh::Slow5File s5;
    if (!s5.open(slow5_path, err)) { fprintf(stderr, "Error in opening file %s\n[fit] %s\n", slow5_path, err.c_str()); return EXIT_FAILURE; }
    pgh::SamBamReader sam;
    if (!sam.open(sam_path, err)) return die("[fit] %s", err);
    FILE *fp = stdout;
    if (out_path && !(fp = fopen(out_path, "w"))) return die("Could not open %s for writing.", out_path);
    if (kmer_path && !pgh::can_write_file(kmer_path)) { if (out_path) fclose(fp); return die("Could not open %s for writing.", kmer_path); }

    pg_fit_params prm; memset(&prm, 0, sizeof prm);
    prm.struct_size = sizeof prm; prm.sig_move_offset = (uint32_t)m; prm.min_dur = (uint32_t)min_dur; prm.max_dur = (uint32_t)max_dur; prm.min_events = (uint32_t)min_events; prm.rna = rna;
    pg_fit *fit = nullptr; pg_mvops *ex = nullptr;
    int status = EXIT_SUCCESS;
    auto finish_files = [&]() { if (out_path) fclose(fp); else fflush(fp); };
    if (pg_fit_create(&prm, (int32_t)device, &fit) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_fit_last_error(nullptr)); finish_files(); return EXIT_FAILURE; }
    if (pg_fit_set_model(fit, levels.data(), k) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_fit_last_error(fit)); pg_fit_destroy(fit); finish_files(); return EXIT_FAILURE; }
    if (pg_mvops_create((int32_t)device, &ex) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_mvops_last_error(nullptr)); pg_fit_destroy(fit); finish_files(); return EXIT_FAILURE; }
    // the expander's stream carries the signal's upload, the expansion and the fit: one queue, in order
    const hipStream_t xs = (hipStream_t)pg_mvops_stream(ex);
    if (pg_fit_set_stream(fit, xs) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; }

    struct Recs {
        std::vector<std::string> names; std::vector<int8_t> mv; std::vector<uint64_t> mv_off{0}, ns, ts, boff; std::vector<int32_t> stride;
        std::vector<uint32_t> l_seq, flag; std::vector<uint8_t> seqb;
        void clear() { names.clear(); mv.clear(); mv_off.assign(1, 0); ns.clear(); ts.clear(); boff.clear(); stride.clear(); l_seq.clear(); flag.clear(); seqb.clear(); }
    } rb;
    auto reform_msg = [](const char *msg, const std::string &id) { char b[600]; snprintf(b, sizeof b, "[reform::ERROR]\033[1;31m %s Read_id: %s\033[0m", msg, id.c_str()); return std::string(b); };
    PgDev<int16_t> d_sig; PgDev<uint64_t> d_sigoff;
    std::vector<int16_t> sig; std::vector<uint64_t> sig_off; std::vector<double> dig, off, range;
    pgh::RawMoveRec raw; pgh::Slow5Rec rec;
    bool eof = false, pending = false;
    auto take = [&]() { // the record in raw / rec joins the batch
        rb.names.push_back(raw.qname);
        rb.mv.insert(rb.mv.end(), raw.mv, raw.mv + (raw.mv_len - 1)); rb.mv_off.push_back(rb.mv.size());
        rb.stride.push_back(raw.stride); rb.ns.push_back(raw.ns); rb.ts.push_back(raw.ts); rb.l_seq.push_back(raw.l_seq); rb.flag.push_back(raw.flag);
        rb.boff.push_back(rb.seqb.size()); rb.seqb.insert(rb.seqb.end(), raw.packed, raw.packed + ((size_t)raw.l_seq + 1) / 2);
        sig.insert(sig.end(), rec.raw.begin(), rec.raw.end()); sig_off.push_back(sig.size());
        dig.push_back(rec.digitisation); off.push_back(rec.offset); range.push_back(rec.range);
    };
    while ((!eof || pending) && status == EXIT_SUCCESS) {
        // ---- the records: the first one that cannot be taken ends the run behind the reads in front of it, with gmove --reform's message
        rb.clear(); sig.clear(); sig_off.assign(1, 0); dig.clear(); off.clear(); range.clear();
        std::string bad;
        while (rb.names.size() < (size_t)batch_reads && sig.size() < (size_t)(PG_FIT_BATCH_SAMPLES / 2)) {
            if (pending) { // the record that did not fit the batch in front: read, checked and fetched already
                pending = false;
                if (rec.raw.size() > (size_t)PG_FIT_BATCH_SAMPLES) { bad = "[fit] read " + raw.qname + " has more than 2^28 samples"; break; }
                take();
                continue;
            }
            const int nr = sam.next_raw(raw, err);
            if (nr == 0) { eof = true; break; }
            if (nr < 0) { bad = "[fit] " + err; break; }
            if (raw.flag & 0x900u) continue; // secondary / supplementary: `samtools fastq` does not print them
            if (!raw.has_ns) { bad = reform_msg("tag 'ns' is not found. Please check your SAM/BAM file:", raw.qname); break; }
            if (!raw.has_ts) { bad = reform_msg("tag 'ts' is not found. Please check your SAM/BAM file:", raw.qname); break; }
            if (!raw.has_mv) { bad = reform_msg("NULL returned for tag mv:", raw.qname); break; }
            if (!raw.mv_is_Bc) { bad = reform_msg("tag 'mv' specification is incorrect.", raw.qname); break; }
            if (raw.mv_len == 0) { bad = reform_msg("mv array length is 0:", raw.qname); break; }
            std::string e2;
            if (!s5.get(raw.qname, rec, e2)) { bad = "Error in when fetching the read (" + e2 + ")"; break; }
            if (sig.size() + rec.raw.size() > (size_t)PG_FIT_BATCH_SAMPLES) { pending = true; break; } // it opens the next batch (the reader is not called before it is taken)
            take();
        }
        const size_t n = rb.names.size();
        if (n) {
            auto hip_ok = [&](hipError_t e, const char *what) { if (e == hipSuccess) return true; fprintf(stderr, "[fit] %s: %s\n", what, hipGetErrorString(e)); status = EXIT_FAILURE; return false; };
            const size_t sb = sig.size() * sizeof(int16_t);
            if (!hip_ok(hipSetDevice((int)device), "hipSetDevice") || !hip_ok(hipStreamSynchronize(xs), "hipStreamSynchronize") || !hip_ok(d_sig.ensure(sb ? sb : 1, sb + sb / 4 + 256), "hipMalloc") ||
                !hip_ok(d_sigoff.ensure((n + 1) * 8, (n + 1) * 10), "hipMalloc") || (sb && !hip_ok(hipMemcpyAsync(d_sig.p, sig.data(), sb, hipMemcpyHostToDevice, xs), "hipMemcpyAsync")) ||
                !hip_ok(hipMemcpyAsync(d_sigoff.p, sig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, xs), "hipMemcpyAsync")) break;
            pg_mvops_batch mb; memset(&mb, 0, sizeof mb);
            mb.n_reads = n; mb.location = PG_LOC_HOST; mb.flags = (rna ? PG_MVOPS_RNA : 0) | (n_to_t ? PG_MVOPS_N_TO_T : 0);
            mb.mv = rb.mv.data(); mb.n_mv_bytes = rb.mv_off[n]; mb.mv_off = rb.mv_off.data(); mb.stride = rb.stride.data(); mb.ns = rb.ns.data(); mb.ts = rb.ts.data();
            mb.l_seq = rb.l_seq.data(); mb.flag = rb.flag.data(); mb.seq_bytes = rb.seqb.data(); mb.n_seq_bytes = rb.seqb.size(); mb.byte_off = rb.boff.data();
            pg_mvops_result mr;
            if (pg_mvops_expand(ex, &mb, &mr) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_mvops_last_error(ex)); status = EXIT_FAILURE; break; }
            pg_batch b; memset(&b, 0, sizeof b);
            b.struct_size = sizeof b; b.location = PG_LOC_DEVICE; b.n_reads = (uint32_t)n; b.n_ops = 0;
            b.sig = d_sig.p; b.sig_off = d_sigoff.p; b.query_start = mr.query_start; b.target_start = mr.target_start; b.target_end = mr.target_end;
            b.seq = mr.seq; b.seq_off = mr.seq_off; b.op_n = mr.op_n; b.op_t = mr.op_t; b.op_off = mr.op_off;
            b.flags = PG_BATCH_ALL_MATCHES;
            pg_fit_reads fr;
            if (pg_fit_submit(fit, &b, mr.status_host, &fr) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; break; }
            for (size_t i = 0; i < n; i++) {
                const pg_fit_sums &q = fr.sums[i];
                fprintf(fp, "%s\t%s\t%lld\t%lld\t", rb.names[i].c_str(), status_name(fr.status[i]), (long long)q.e, (long long)q.n);
                if (fr.status[i] == PG_FIT_ST_OK) {
                    long double rep[3];
                    pg_fit_report(PgFitSums{q.n, q.sl, q.sll, q.sr, q.srl, q.srr, q.e}, dig[i], off[i], range[i], rep);
                    fprintf(fp, "%.6Lf\t%.6Lf\t%.6Lf\n", rep[0], rep[1], rep[2]);
                } else fprintf(fp, "\t\t\n");
            }
        }
        if (status == EXIT_SUCCESS && !bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); status = EXIT_FAILURE; }
    }
    pg_fit_result res; memset(&res, 0, sizeof res);
    if (status == EXIT_SUCCESS && pg_fit_finish(fit, &res) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; }
    if (status == EXIT_SUCCESS) {
        unsigned __int128 dd = 0;
        for (uint64_t s = 0; s < n_slots; s++) dd += ((unsigned __int128)res.sum_dd_hi[s] << 64) | res.sum_dd_lo[s];
        if (kmer_path) {
            FILE *kf = fopen(kmer_path, "w");
            if (!kf) { status = die("Could not open %s for writing.", kmer_path); }
            else {
                std::string name(k, 'A');
                const char *alpha = uses_u ? "ACGU" : "ACGT";
                for (uint64_t s = 0; s < n_slots; s++) {
                    for (uint32_t j = 0; j < k; j++) name[j] = alpha[(s >> (2 * (k - 1 - j))) & 3];
                    fprintf(kf, "%s\t%llu\t%llu\t%s\t", name.c_str(), (unsigned long long)res.n_samples[s], (unsigned long long)res.n_events[s],
                            levels[s] ? pg_fit_units_text(levels[s]).c_str() : "");
                    if (res.n_samples[s]) {
                        int64_t mean, rms;
                        pg_fit_slot_resid(res.n_samples[s], res.sum_d[s], res.sum_dd_lo[s], res.sum_dd_hi[s], mean, rms);
                        fprintf(kf, "%s\t%s\n", pg_fit_units_text(mean).c_str(), pg_fit_units_text(rms).c_str());
                    } else fprintf(kf, "\t\n");
                }
                if (fclose(kf) != 0) status = die("Error in writing %s.", kmer_path);
            }
        }
        std::string pooled;
        if (res.samples) {
            int64_t mean, rms;
            pg_fit_slot_resid(res.samples, 0, (uint64_t)dd, (uint64_t)(dd >> 64), mean, rms);
            pooled = pg_fit_units_text(rms);
        }
        fprintf(stderr, "[fit] k=%u reads=%llu fitted=%llu events=%llu samples=%llu clamped=%llu rms_resid=%s\n", k, (unsigned long long)res.reads, (unsigned long long)res.fitted,
                (unsigned long long)res.events, (unsigned long long)res.samples, (unsigned long long)res.clamped, pooled.c_str());
    }
    finish_files();
    pg_fit_destroy(fit);
    pg_mvops_destroy(ex);
    return status;
}
