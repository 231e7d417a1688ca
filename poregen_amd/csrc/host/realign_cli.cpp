// realign_cli.cpp -- `poregen realign`: the move table's event boundaries, which the basecaller puts on multiples of its stride, moved to
// where the samples fit a k-mer model best. The reference's dispatcher has the command (src/main.c); what stands behind it there
// (src/realign.cpp) is a copy of reform that aligns nothing. The records are read as `poregen fit` reads them; per batch the move tables
// are expanded (pg_mvops_expand), every read is calibrated against the model (pg_fit_submit), its free boundaries are refined within
// --band samples (pg_realign_submit; the rule: csrc/pg_realign.h) and the refined segmentation is scored again by a second fit handle.
//   -o            per read the PAF line `poregen reform -c -k 1 -m 0 --stride 0 [--rna]` prints, with the refined durations in ss:Z:
//   --read_table  read_id  status  n_free  n_moved  sum_abs_shift  rms_before  rms_after      (pA with three decimals, empty unless ok)
//   --kmer_table  fit's per-k-mer table on the refined segmentation
#include "../../../include/pgmove.h"
#include "../pg_realign.h"
#include "../pg_hip_host.h"
#include "pg_host.h"

#include <cinttypes>
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
    {"min_len", required_argument, nullptr, 0},    // 8
    {"band", required_argument, nullptr, 0},       // 9
    {"read_table", required_argument, nullptr, 0}, // 10
    {"help", no_argument, nullptr, 'h'},           // 11
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen realign [options] MODEL reads.slow5/blow5 reads.bam/sam\n");
    fprintf(fp, "\nrefine the event boundaries of the move table against a k-mer model; writes PAF with ss:Z: as `reform -c -k 1` does\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   -k INT                     k-mer length; must be the model's [the model's]\n");
    fprintf(fp, "   -m INT                     move start offset [0]\n");
    fprintf(fp, "   --rna                      the dataset is direct RNA\n");
    fprintf(fp, "   --n_to_t                   an N of a read counts as T\n");
    fprintf(fp, "   --min_dur INT              minimum number of samples of an event that is refined [5]\n");
    fprintf(fp, "   --max_dur INT              maximum number of samples of an event that is refined, at most %u [70]\n", PG_RL_MAX_DUR);
    fprintf(fp, "   --min_events INT           counted events a read needs to be fitted [20]\n");
    fprintf(fp, "   --min_len INT              fewest samples a refined event keeps, 1 to --min_dur [3]\n");
    fprintf(fp, "   --band INT                 how far a boundary may move, in samples, 0 to %u [10]\n", PG_RL_MAX_BAND);
    fprintf(fp, "   -o FILE                    the refined PAF [stdout]\n");
    fprintf(fp, "   --read_table FILE          the per-read table\n");
    fprintf(fp, "   --kmer_table FILE          the per-k-mer table of the refined segmentation\n");
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
    return st < 6 ? kFit[st] : "refused";
}

std::string rms_text(uint64_t n, uint64_t lo, uint64_t hi) {
    if (!n) return "";
    int64_t mean, rms;
    pg_fit_slot_resid(n, 0, lo, hi, mean, rms);
    return pg_fit_units_text(rms);
}

} // namespace

int realign_main(int argc, char **argv) {
    long long k_opt = 0, m = 0, min_dur = 5, max_dur = 70, min_events = 20, batch_reads = 4000, device = 0, min_len = 3, band = 10;
    bool rna = false, n_to_t = false, help = false;
    const char *out_path = nullptr, *kmer_path = nullptr, *read_path = nullptr;
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
        else if (c == 0 && longindex == 2) ok = whole_uint(optarg, PG_RL_MAX_DUR, min_dur);
        else if (c == 0 && longindex == 3) ok = whole_uint(optarg, PG_RL_MAX_DUR, max_dur);
        else if (c == 0 && longindex == 4) ok = whole_uint(optarg, 0xffffffffll, min_events);
        else if (c == 0 && longindex == 5) kmer_path = optarg;
        else if (c == 0 && longindex == 6) ok = whole_uint(optarg, 1 << 24, batch_reads) && batch_reads >= 1;
        else if (c == 0 && longindex == 7) ok = whole_uint(optarg, 1024, device);
        else if (c == 0 && longindex == 8) ok = whole_uint(optarg, PG_RL_MAX_DUR, min_len) && min_len >= 1;
        else if (c == 0 && longindex == 9) ok = whole_uint(optarg, PG_RL_MAX_BAND, band);
        else if (c == 0 && longindex == 10) read_path = optarg;
        else { print_help(stderr); return EXIT_FAILURE; }
        if (!ok) {
            fprintf(stderr, "[realign] %s%s: '%s' is not a value it takes (-k 1..9, -m 0..64, durations 0..%u, --min_len from 1, --band 0..%u)\n", c ? "-" : "--",
                    c ? std::string(1, (char)c).c_str() : kLongOptions[longindex].name, optarg, PG_RL_MAX_DUR, PG_RL_MAX_BAND);
            return EXIT_FAILURE;
        }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    if (argc - optind != 3) { print_help(stderr); return EXIT_FAILURE; }
    if (min_dur > max_dur) return die("[realign] --min_dur may not exceed --max_dur");
    if (min_len > min_dur) return die("[realign] --min_len may not exceed --min_dur");
    const char *model_path = argv[optind], *slow5_path = argv[optind + 1], *sam_path = argv[optind + 2];
    {
        const size_t ml = strlen(sam_path);
        if (!(ml >= 4 && (!strcmp(sam_path + ml - 4, ".bam") || !strcmp(sam_path + ml - 4, ".sam")))) return die("[realign] the records come from a .bam or .sam file, not %s", sam_path);
    }
    // ---- the model: parsed and refused on the host, before any device is touched
    pgh::MappedFile mf;
    if (!mf.open(model_path)) return die("[realign] cannot open the model %s", model_path);
    std::vector<uint32_t> levels((size_t)1 << (2 * PG_FIT_MAX_K));
    uint32_t k = 0; int32_t uses_u = 0; char perr[400];
    if (pg_fit_parse_model(mf.data, mf.size, (uint32_t)k_opt, &k, levels.data(), levels.size(), &uses_u, perr, sizeof perr) != PG_OK) {
        fprintf(stderr, "[realign] the model %s is refused: %s\n", model_path, perr);
        return EXIT_FAILURE;
    }
    mf.close();
    const uint64_t n_slots = 1ull << (2 * k);
    std::string err;
    pgh::Slow5File s5;
    if (!s5.open(slow5_path, err)) { fprintf(stderr, "Error in opening file %s\n[realign] %s\n", slow5_path, err.c_str()); return EXIT_FAILURE; }
    pgh::SamBamReader sam;
    if (!sam.open(sam_path, err)) return die("[realign] %s", err);
    FILE *fp = stdout, *rf = nullptr;
    if (out_path && !(fp = fopen(out_path, "w"))) return die("Could not open %s for writing.", out_path);
    auto finish_files = [&]() { if (out_path) fclose(fp); else fflush(fp); if (rf) fclose(rf); rf = nullptr; };
    if (read_path && !(rf = fopen(read_path, "w"))) { finish_files(); return die("Could not open %s for writing.", read_path); }
    if (kmer_path && !pgh::can_write_file(kmer_path)) { finish_files(); return die("Could not open %s for writing.", kmer_path); }

    pg_fit_params prm; memset(&prm, 0, sizeof prm);
    prm.struct_size = sizeof prm; prm.sig_move_offset = (uint32_t)m; prm.min_dur = (uint32_t)min_dur; prm.max_dur = (uint32_t)max_dur; prm.min_events = (uint32_t)min_events; prm.rna = rna;
    pg_realign_params rp; memset(&rp, 0, sizeof rp);
    rp.struct_size = sizeof rp; rp.sig_move_offset = (uint32_t)m; rp.min_dur = (uint32_t)min_dur; rp.max_dur = (uint32_t)max_dur; rp.rna = rna; rp.band = (uint32_t)band; rp.min_len = (uint32_t)min_len;
    pg_fit *fit = nullptr, *fit2 = nullptr; pg_realign *ra = nullptr; pg_mvops *ex = nullptr;
    int status = EXIT_SUCCESS;
    auto release = [&]() { if (fit) pg_fit_destroy(fit); if (fit2) pg_fit_destroy(fit2); if (ra) pg_realign_destroy(ra); if (ex) pg_mvops_destroy(ex); };
    if (pg_fit_create(&prm, (int32_t)device, &fit) != PG_OK || pg_fit_create(&prm, (int32_t)device, &fit2) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_realign_create(&rp, (int32_t)device, &ra) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_realign_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_mvops_create((int32_t)device, &ex) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_mvops_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_fit_set_model(fit, levels.data(), k) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; }
    else if (pg_fit_set_model(fit2, levels.data(), k) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fit2)); status = EXIT_FAILURE; }
    else if (pg_realign_set_model(ra, levels.data(), k) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_realign_last_error(ra)); status = EXIT_FAILURE; }
    if (status != EXIT_SUCCESS) { release(); finish_files(); return status; }
    // the expander's stream carries the signal's upload, the expansion, both fits and the alignment: one queue, in order
    const hipStream_t xs = (hipStream_t)pg_mvops_stream(ex);
    if (pg_fit_set_stream(fit, xs) != PG_OK || pg_fit_set_stream(fit2, xs) != PG_OK || pg_realign_set_stream(ra, xs) != PG_OK) { fprintf(stderr, "[realign] cannot share the expander's stream\n"); status = EXIT_FAILURE; }

    struct Recs {
        std::vector<std::string> names; std::vector<int8_t> mv; std::vector<uint64_t> mv_off{0}, ns, ts, boff; std::vector<int32_t> stride;
        std::vector<uint32_t> l_seq, flag; std::vector<uint8_t> seqb;
        void clear() { names.clear(); mv.clear(); mv_off.assign(1, 0); ns.clear(); ts.clear(); boff.clear(); stride.clear(); l_seq.clear(); flag.clear(); seqb.clear(); }
    } rb;
    auto reform_msg = [](const char *msg, const std::string &id) { char b[600]; snprintf(b, sizeof b, "[reform::ERROR]\033[1;31m %s Read_id: %s\033[0m", msg, id.c_str()); return std::string(b); };
    static const char *const kRefusal[] = {"", "the move table holds fewer moves than sig_move_offset + 1.", "Error in calcuation. (ns - ((i-1)*EXPECTED_STRIDE + ts)) > 0 is not valid.",
                                           "Error in the implementation. Please report the command with minimal reproducible data.", "the stride of the move table (mv[0]) is less than 1."};
    PgDev<int16_t> d_sig; PgDev<uint64_t> d_sigoff;
    std::vector<int16_t> sig; std::vector<uint64_t> sig_off;
    std::vector<uint32_t> h_ops; std::vector<int32_t> h_qs;
    pgh::RawMoveRec raw; pgh::Slow5Rec rec;
    bool eof = false, pending = false;
    uint64_t total_free = 0, total_moved = 0;
    auto take = [&]() { // the record in raw / rec joins the batch
        rb.names.push_back(raw.qname);
        rb.mv.insert(rb.mv.end(), raw.mv, raw.mv + (raw.mv_len - 1)); rb.mv_off.push_back(rb.mv.size());
        rb.stride.push_back(raw.stride); rb.ns.push_back(raw.ns); rb.ts.push_back(raw.ts); rb.l_seq.push_back(raw.l_seq); rb.flag.push_back(raw.flag);
        rb.boff.push_back(rb.seqb.size()); rb.seqb.insert(rb.seqb.end(), raw.packed, raw.packed + ((size_t)raw.l_seq + 1) / 2);
        sig.insert(sig.end(), rec.raw.begin(), rec.raw.end()); sig_off.push_back(sig.size());
    };
    while ((!eof || pending) && status == EXIT_SUCCESS) {
        // ---- the records: the first one that cannot be taken ends the run behind the reads in front of it, with gmove --reform's message
        rb.clear(); sig.clear(); sig_off.assign(1, 0);
        std::string bad;
        while (rb.names.size() < (size_t)batch_reads && sig.size() < (size_t)(PG_FIT_BATCH_SAMPLES / 2)) {
            if (pending) { // the record that did not fit the batch in front: read, checked and fetched already
                pending = false;
                if (rec.raw.size() > (size_t)PG_FIT_BATCH_SAMPLES) { bad = "[realign] read " + raw.qname + " has more than 2^28 samples"; break; }
                take();
                continue;
            }
            const int nr = sam.next_raw(raw, err);
            if (nr == 0) { eof = true; break; }
            if (nr < 0) { bad = "[realign] " + err; break; }
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
        size_t n = rb.names.size();
        if (n) {
            auto hip_ok = [&](hipError_t e, const char *what) { if (e == hipSuccess) return true; fprintf(stderr, "[realign] %s: %s\n", what, hipGetErrorString(e)); status = EXIT_FAILURE; return false; };
            const size_t sb = sig.size() * sizeof(int16_t);
            if (!hip_ok(hipSetDevice((int)device), "hipSetDevice") || !hip_ok(hipStreamSynchronize(xs), "hipStreamSynchronize") || !hip_ok(d_sig.ensure(sb ? sb : 1, sb + sb / 4 + 256), "hipMalloc") ||
                !hip_ok(d_sigoff.ensure((n + 1) * 8, (n + 1) * 10), "hipMalloc") || (sb && !hip_ok(hipMemcpyAsync(d_sig.p, sig.data(), sb, hipMemcpyHostToDevice, xs), "hipMemcpyAsync")) ||
                !hip_ok(hipMemcpyAsync(d_sigoff.p, sig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, xs), "hipMemcpyAsync")) break;
            pg_mvops_batch mb; memset(&mb, 0, sizeof mb);
            mb.n_reads = n; mb.location = PG_LOC_HOST; mb.flags = (rna ? PG_MVOPS_RNA : 0) | (n_to_t ? PG_MVOPS_N_TO_T : 0);
            mb.mv = rb.mv.data(); mb.n_mv_bytes = rb.mv_off[n]; mb.mv_off = rb.mv_off.data(); mb.stride = rb.stride.data(); mb.ns = rb.ns.data(); mb.ts = rb.ts.data();
            mb.l_seq = rb.l_seq.data(); mb.flag = rb.flag.data(); mb.seq_bytes = rb.seqb.data(); mb.n_seq_bytes = rb.seqb.size(); mb.byte_off = rb.boff.data();
            pg_mvops_result mr;
            if (pg_mvops_expand(ex, &mb, &mr) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_mvops_last_error(ex)); status = EXIT_FAILURE; break; }
            if (mr.first_refused >= 0) { // reform returns -1 on this record: the reads in front of it are the batch, and the last one
                const size_t f = (size_t)mr.first_refused;
                const uint32_t code = mr.status_host[f];
                bad = reform_msg(kRefusal[code < 5 ? code : 3], rb.names[f]);
                n = f;
            }
            uint64_t n_ops = 0; // an accepted read has as many ops as bases
            for (size_t i = 0; i < n; i++) n_ops += rb.l_seq[i];
            if (n_ops > 0xffffffffull) { fprintf(stderr, "[realign] a batch of more than 2^32 - 1 bases: use a smaller --batch_reads\n"); status = EXIT_FAILURE; break; }
            if (n) {
                pg_batch b; memset(&b, 0, sizeof b);
                b.struct_size = sizeof b; b.location = PG_LOC_DEVICE; b.n_reads = (uint32_t)n; b.n_ops = (uint32_t)n_ops;
                b.sig = d_sig.p; b.sig_off = d_sigoff.p; b.query_start = mr.query_start; b.target_start = mr.target_start; b.target_end = mr.target_end;
                b.seq = mr.seq; b.seq_off = mr.seq_off; b.op_n = mr.op_n; b.op_t = mr.op_t; b.op_off = mr.op_off;
                b.flags = PG_BATCH_ALL_MATCHES;
                pg_fit_reads fr, fr2;
                pg_realign_reads rr; memset(&rr, 0, sizeof rr); rr.struct_size = sizeof rr;
                if (pg_fit_submit(fit, &b, nullptr, &fr) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; break; }
                if (pg_realign_submit(ra, &b, fr.status, fr.a, fr.b, &rr) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_realign_last_error(ra)); status = EXIT_FAILURE; break; }
                pg_batch b2 = b; b2.op_n = rr.op_n;
                if (pg_fit_submit(fit2, &b2, nullptr, &fr2) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fit2)); status = EXIT_FAILURE; break; }
                h_ops.resize(n_ops); h_qs.resize(n);
                if ((n_ops && !hip_ok(hipMemcpy(h_ops.data(), rr.op_n, n_ops * 4, hipMemcpyDeviceToHost), "hipMemcpy")) ||
                    !hip_ok(hipMemcpy(h_qs.data(), mr.query_start, n * 4, hipMemcpyDeviceToHost), "hipMemcpy")) break;
                uint64_t at = 0;
                for (size_t i = 0; i < n; i++) {
                    const uint32_t lb = rb.l_seq[i];
                    uint64_t end = (uint64_t)(int64_t)h_qs[i];
                    for (uint32_t e = 0; e < lb; e++) end += h_ops[at + e];
                    const char *id = rb.names[i].c_str();
                    fprintf(fp, "%s\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t+\t%s\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t255\tss:Z:", id, rb.ns[i],
                            (uint64_t)(int64_t)h_qs[i], end, id, lb, rna ? lb : 0u, rna ? 0u : lb, lb, lb);
                    for (uint32_t e = 0; e < lb; e++) fprintf(fp, "%" PRIu32 ",", h_ops[at + e]);
                    fputc('\n', fp);
                    at += lb;
                    const pg_realign_read &q = rr.reads[i];
                    total_free += q.n_free; total_moved += q.n_moved;
                    if (rf) {
                        const bool ok = fr.status[i] == PG_FIT_ST_OK;
                        const uint64_t ns = ok ? (uint64_t)fr.sums[i].n : 0;
                        fprintf(rf, "%s\t%s\t%u\t%u\t%llu\t%s\t%s\n", id, status_name(fr.status[i]), q.n_free, q.n_moved, (unsigned long long)q.sum_abs_shift,
                                rms_text(ns, q.cost_before_lo, q.cost_before_hi).c_str(), rms_text(ns, q.cost_after_lo, q.cost_after_hi).c_str());
                    }
                }
            }
        }
        if (status == EXIT_SUCCESS && !bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); status = EXIT_FAILURE; }
    }
    pg_fit_result res, res2; memset(&res, 0, sizeof res); memset(&res2, 0, sizeof res2);
    if (status == EXIT_SUCCESS && (pg_fit_finish(fit, &res) != PG_OK || pg_fit_finish(fit2, &res2) != PG_OK)) { fprintf(stderr, "[realign] %s%s\n", pg_fit_last_error(fit), pg_fit_last_error(fit2)); status = EXIT_FAILURE; }
    if (status == EXIT_SUCCESS) {
        auto pooled = [&](const pg_fit_result &r) {
            unsigned __int128 dd = 0;
            for (uint64_t s = 0; s < n_slots; s++) dd += ((unsigned __int128)r.sum_dd_hi[s] << 64) | r.sum_dd_lo[s];
            return rms_text(r.samples, (uint64_t)dd, (uint64_t)(dd >> 64));
        };
        if (kmer_path) {
            FILE *kf = fopen(kmer_path, "w");
            if (!kf) { status = die("Could not open %s for writing.", kmer_path); }
            else {
                std::string name(k, 'A');
                const char *alpha = uses_u ? "ACGU" : "ACGT";
                for (uint64_t s = 0; s < n_slots; s++) {
                    for (uint32_t j = 0; j < k; j++) name[j] = alpha[(s >> (2 * (k - 1 - j))) & 3];
                    fprintf(kf, "%s\t%llu\t%llu\t%s\t", name.c_str(), (unsigned long long)res2.n_samples[s], (unsigned long long)res2.n_events[s],
                            levels[s] ? pg_fit_units_text(levels[s]).c_str() : "");
                    if (res2.n_samples[s]) {
                        int64_t mean, rms;
                        pg_fit_slot_resid(res2.n_samples[s], res2.sum_d[s], res2.sum_dd_lo[s], res2.sum_dd_hi[s], mean, rms);
                        fprintf(kf, "%s\t%s\n", pg_fit_units_text(mean).c_str(), pg_fit_units_text(rms).c_str());
                    } else fprintf(kf, "\t\n");
                }
                if (fclose(kf) != 0) status = die("Error in writing %s.", kmer_path);
            }
        }
        fprintf(stderr, "[realign] k=%u band=%lld min_len=%lld reads=%llu refined=%llu free=%llu moved=%llu rms_resid_before=%s rms_resid_after=%s\n", k, band, min_len,
                (unsigned long long)res.reads, (unsigned long long)res.fitted, (unsigned long long)total_free, (unsigned long long)total_moved, pooled(res).c_str(), pooled(res2).c_str());
    }
    finish_files();
    release();
    return status;
}
