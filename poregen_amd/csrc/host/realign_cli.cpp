// realign_cli.cpp -- `poregen realign`: the move table's event boundaries, which the basecaller puts on multiples of its stride, moved to
// where the samples fit a k-mer model best. The reference's dispatcher has the command (src/main.c); what stands behind it there
// (src/realign.cpp) is a copy of reform that aligns nothing. The records are read as `poregen fit` reads them; per batch the move tables
// are expanded (pg_mvops_expand), every read is calibrated against the model (pg_fit_submit), its free boundaries are refined within
// --band samples (pg_realign_submit; the rule: csrc/pg_realign.h) and the refined segmentation is scored again by a second fit handle.
// With --rounds R the last two steps repeat: round t fits the ops of round t - 1 and refines them at phase 0 (t odd) or 128 (t even), so
// that the boundaries one round pins at multiples of 256 are free in the next; a read that is not fitted in a round keeps its ops in it.
//   -o            per read the PAF line `poregen reform -c -k 1 -m 0 --stride 0 [--rna]` prints, with the refined durations in ss:Z:
//   --read_table  read_id  status  n_free  n_moved  sum_abs_shift  rms_before  rms_after      (pA with three decimals, empty unless ok)
//   --kmer_table  fit's per-k-mer table on the refined segmentation
#include "../pg_realign.h"
#include "pg_cli.h"
#include "pg_moverecs.h"

#include <cinttypes>
#include <getopt.h>

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
    {"rounds", required_argument, nullptr, 0},     // 11
    {"help", no_argument, nullptr, 'h'},           // 12
    {"ref", required_argument, nullptr, 0},        // 13
    {"both_strands", no_argument, nullptr, 0},     // 14
    {"rc_suffix", required_argument, nullptr, 0},  // 15
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen realign [options] MODEL reads.slow5/blow5 reads.bam/sam\n");
    fprintf(fp, "       poregen realign --ref REF.fa [--both_strands] [--rc_suffix STR] [options] MODEL reads.slow5/blow5 mapped.bam/sam\n");
    fprintf(fp, "\nrefine the event boundaries of the move table against a k-mer model; writes PAF with ss:Z: as `reform -c -k 1` does\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   -k INT                     k-mer length; must be the model's [the model's]\n");
    fprintf(fp, "   -m INT                     move start offset [0]\n");
    fprintf(fp, "   --rna                      the dataset is direct RNA\n");
    fprintf(fp, "   --n_to_t                   an N of a read counts as T\n");
    fprintf(fp, "   --ref REF.fa               a MAPPED .bam / .sam: refine the signal-to-reference alignment -- the ops carried through each record's CIGAR on the\n");
    fprintf(fp, "                              GPU, the k-mers the record's slice of REF.fa spells; an I or a D pins the boundaries beside it and keeps its length.\n");
    fprintf(fp, "                              -o is the PAF `reform -c -k 1 -m 0 --stride 0 --to_ref` prints, with the refined durations (--band 0: that PAF).\n");
    fprintf(fp, "                              Unmapped and reverse-strand records are skipped and counted. Not with --n_to_t\n");
    fprintf(fp, "   --both_strands             with --ref: reverse-strand records are taken too, as `reform --to_ref --both_strands` writes them\n");
    fprintf(fp, "   --rc_suffix STR            with --both_strands: the suffix of a reverse-strand record's target name [_rc]\n");
    fprintf(fp, "   --min_dur INT              minimum number of samples of an event that is refined [5]\n");
    fprintf(fp, "   --max_dur INT              maximum number of samples of an event that is refined, at most %u [70]\n", PG_RL_MAX_DUR);
    fprintf(fp, "   --min_events INT           counted events a read needs to be fitted [20]\n");
    fprintf(fp, "   --min_len INT              fewest samples a refined event keeps, 1 to --min_dur [3]\n");
    fprintf(fp, "   --band INT                 how far a boundary may move, in samples, 0 to %u [10]\n", PG_RL_MAX_BAND);
    fprintf(fp, "   --rounds INT               rounds of fit and refinement, 1 to 8; even rounds pin the boundaries at 128 + 256 i instead of 256 i [1]\n");
    fprintf(fp, "   -o FILE                    the refined PAF of the last round [stdout]\n");
    fprintf(fp, "   --read_table FILE          the per-read table: status and rms_before of round 1, rms_after of the last round; n_free, n_moved and\n");
    fprintf(fp, "                              sum_abs_shift are sums over the rounds (a boundary free in two rounds counts twice)\n");
    fprintf(fp, "   --kmer_table FILE          the per-k-mer table of the refined segmentation\n");
    fprintf(fp, "   --batch_reads INT          reads per device batch [4000]\n");
    fprintf(fp, "   --device INT               HIP device [0]\n");
    fprintf(fp, "   -h                         help\n");
}

} // namespace

int realign_main(int argc, char **argv) {
    long long k_opt = 0, m = 0, min_dur = 5, max_dur = 70, min_events = 20, batch_reads = 4000, device = 0, min_len = 3, band = 10, rounds = 1;
    bool rna = false, n_to_t = false, help = false;
    const char *out_path = nullptr, *kmer_path = nullptr, *read_path = nullptr, *ref_path = nullptr, *rc_suffix = nullptr;
    bool both_strands = false;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "k:m:o:h", kLongOptions, &longindex)) >= 0) {
        bool ok = true;
        if (c == 'k') ok = whole_int(optarg, 1, PG_FIT_MAX_K, k_opt);
        else if (c == 'm') ok = whole_int(optarg, 0, 64, m);
        else if (c == 'o') out_path = optarg;
        else if (c == 'h') help = true;
        else if (c == 0 && longindex == 0) rna = true;
        else if (c == 0 && longindex == 1) n_to_t = true;
        else if (c == 0 && longindex == 2) ok = whole_int(optarg, 0, PG_RL_MAX_DUR, min_dur);
        else if (c == 0 && longindex == 3) ok = whole_int(optarg, 0, PG_RL_MAX_DUR, max_dur);
        else if (c == 0 && longindex == 4) ok = whole_int(optarg, 0, 0xffffffffll, min_events);
        else if (c == 0 && longindex == 5) kmer_path = optarg;
        else if (c == 0 && longindex == 6) ok = whole_int(optarg, 1, 1 << 24, batch_reads);
        else if (c == 0 && longindex == 7) ok = whole_int(optarg, 0, 1024, device);
        else if (c == 0 && longindex == 8) ok = whole_int(optarg, 1, PG_RL_MAX_DUR, min_len);
        else if (c == 0 && longindex == 9) ok = whole_int(optarg, 0, PG_RL_MAX_BAND, band);
        else if (c == 0 && longindex == 10) read_path = optarg;
        else if (c == 0 && longindex == 11) ok = whole_int(optarg, 1, 8, rounds);
        else if (c == 0 && longindex == 13) ref_path = optarg;
        else if (c == 0 && longindex == 14) both_strands = true;
        else if (c == 0 && longindex == 15) rc_suffix = optarg;
        else { print_help(stderr); return EXIT_FAILURE; }
        if (!ok) {
            fprintf(stderr, "[realign] %s%s: '%s' is not a value it takes (-k 1..9, -m 0..64, durations 0..%u, --min_len from 1, --band 0..%u, --rounds 1..8)\n", c ? "-" : "--",
                    c ? std::string(1, (char)c).c_str() : kLongOptions[longindex].name, optarg, PG_RL_MAX_DUR, PG_RL_MAX_BAND);
            return EXIT_FAILURE;
        }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    if (argc - optind != 3) { print_help(stderr); return EXIT_FAILURE; }
    if (min_dur > max_dur) return die("[realign] --min_dur may not exceed --max_dur");
    if (min_len > min_dur) return die("[realign] --min_len may not exceed --min_dur");
    if (both_strands && !ref_path) return die("[realign] --both_strands applies with --ref only");
    if (rc_suffix && !both_strands) return die("[realign] --rc_suffix applies with --both_strands only");
    if (ref_path && n_to_t) return die("[realign] --ref cannot be combined with --n_to_t: the sequence is the reference's, there is nothing to rewrite");
    if (!rc_suffix) rc_suffix = "_rc";
    const char *model_path = argv[optind], *slow5_path = argv[optind + 1], *sam_path = argv[optind + 2];
    if (!is_sam_or_bam(sam_path)) return die("[realign] the records come from a .bam or .sam file, not %s", sam_path);
    std::vector<uint32_t> levels;
    uint32_t k = 0; int32_t uses_u = 0;
    if (!load_level_model("realign", model_path, k_opt, levels, k, uses_u)) return EXIT_FAILURE;
    RefRoute route; // --ref: the FASTA, the projection and the slices of every batch
    route.both_strands = both_strands; route.rna = rna;
    if (ref_path) {
        std::string ferr;
        if (!route.fai.load(ref_path, ferr)) { fprintf(stderr, "Error in loading the reference %s%s%s\n", ref_path, ferr.empty() ? "" : ": ", ferr.c_str()); return EXIT_FAILURE; }
    }
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
    pg_fit *fit = nullptr, *fit2 = nullptr, *fitm = nullptr; pg_realign *ra = nullptr; pg_mvops *ex = nullptr; // fitm: the fits of rounds 2 .. R, which no table pools
    int status = EXIT_SUCCESS;
    auto release = [&]() { if (fit) pg_fit_destroy(fit); if (fit2) pg_fit_destroy(fit2); if (fitm) pg_fit_destroy(fitm); if (ra) pg_realign_destroy(ra); if (ex) pg_mvops_destroy(ex); };
    if (pg_fit_create(&prm, (int32_t)device, &fit) != PG_OK || pg_fit_create(&prm, (int32_t)device, &fit2) != PG_OK || (rounds > 1 && pg_fit_create(&prm, (int32_t)device, &fitm) != PG_OK)) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_realign_create(&rp, (int32_t)device, &ra) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_realign_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_mvops_create((int32_t)device, &ex) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_mvops_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_fit_set_model(fit, levels.data(), k) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; }
    else if (pg_fit_set_model(fit2, levels.data(), k) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fit2)); status = EXIT_FAILURE; }
    else if (fitm && pg_fit_set_model(fitm, levels.data(), k) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fitm)); status = EXIT_FAILURE; }
    else if (pg_realign_set_model(ra, levels.data(), k) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_realign_last_error(ra)); status = EXIT_FAILURE; }
    if (status != EXIT_SUCCESS) { release(); finish_files(); return status; }
    // the expander's stream carries the signal's upload, the expansion, both fits and the alignment: one queue, in order
    const hipStream_t xs = (hipStream_t)pg_mvops_stream(ex);
    if (pg_fit_set_stream(fit, xs) != PG_OK || pg_fit_set_stream(fit2, xs) != PG_OK || (fitm && pg_fit_set_stream(fitm, xs) != PG_OK) || pg_realign_set_stream(ra, xs) != PG_OK) { fprintf(stderr, "[realign] cannot share the expander's stream\n"); status = EXIT_FAILURE; }

    PgDev<int16_t> d_sig; PgDev<uint64_t> d_sigoff; PgDev<uint8_t> d_seq; PgDev<uint64_t> d_seqoff;
    std::vector<uint32_t> h_ops; std::vector<int32_t> h_qs, h_ts, h_te; std::vector<uint8_t> h_opt; std::vector<uint64_t> h_opoff;
    RealignRounds rr;
    pgh::MoveSignalBatches in(sam, s5, "realign", (size_t)batch_reads, (size_t)(PG_FIT_BATCH_SAMPLES / 2), (size_t)PG_FIT_BATCH_SAMPLES);
    const pgh::MoveRecs &rb = in.recs;
    const HipOk hip_ok{"realign", &status};
    if (ref_path) { in.to_ref_skipped = route.skipped_counter(); in.reverse_taken = route.reverse_counter(); }
    while (!in.done() && status == EXIT_SUCCESS) {
        // ---- the records: the first one that cannot be taken ends the run behind the reads in front of it, with gmove --reform's message
        std::string bad;
        in.next(bad);
        size_t n = rb.size();
        if (n) {
            if (!hip_ok(hipSetDevice((int)device), "hipSetDevice") || !upload_signal(hip_ok, d_sig, d_sigoff, in.sig, in.sig_off, xs)) break;
            pg_mvops_batch mb;
            rb.fill(mb, n, (rna ? PG_MVOPS_RNA : 0) | (n_to_t ? PG_MVOPS_N_TO_T : 0));
            pg_mvops_result mr;
            if (pg_mvops_expand(ex, &mb, &mr) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_mvops_last_error(ex)); status = EXIT_FAILURE; break; }
            if (ref_path) { // the ops onto the reference and the slices of REF.fa; a record reform --to_ref ends on ends the run behind the reads in front
                bool cut = false;
                if (!route.project("realign", ex, rb, mr, n, bad, cut)) { status = EXIT_FAILURE; break; }
                if (!route.slices("realign", hip_ok, (int)device, xs, rb, n) || (n && !route.to_device(hip_ok, xs, n, d_seq, d_seqoff))) { status = EXIT_FAILURE; break; }
            } else if (mr.first_refused >= 0) { // reform returns -1 on this record: the reads in front of it are the batch, and the last one
                n = (size_t)mr.first_refused;
                bad = pgh::reform_error(pgh::reform_refusal(mr.status_host[n]), rb.names[n]);
            }
            uint64_t n_ops = 0; // an accepted read has as many ops as bases
            for (size_t i = 0; i < n; i++) n_ops += rb.l_seq[i];
            if (ref_path) n_ops = route.n_ops;
            if (n_ops > 0xffffffffull) { fprintf(stderr, "[realign] a batch of more than 2^32 - 1 bases: use a smaller --batch_reads\n"); status = EXIT_FAILURE; break; }
            if (n) {
                const pg_batch b = ref_path ? route.gapped_batch(n, d_sig.p, d_sigoff.p, d_seq.p, d_seqoff.p) : device_batch(mr, n, n_ops, d_sig.p, d_sigoff.p);
                pg_fit_reads fr2;
                if (!rr.run(fit, fitm, ra, b, rounds)) { fprintf(stderr, "[realign] %s\n", rr.err.c_str()); status = EXIT_FAILURE; break; }
                pg_batch b2 = b; b2.op_n = rr.op_n;
                if (pg_fit_submit(fit2, &b2, nullptr, &fr2) != PG_OK) { fprintf(stderr, "[realign] %s\n", pg_fit_last_error(fit2)); status = EXIT_FAILURE; break; }
                h_ops.resize(n_ops); h_qs.resize(n);
                if ((n_ops && !hip_ok(hipMemcpy(h_ops.data(), rr.op_n, n_ops * 4, hipMemcpyDeviceToHost), "hipMemcpy")) ||
                    !hip_ok(hipMemcpy(h_qs.data(), b.query_start, n * 4, hipMemcpyDeviceToHost), "hipMemcpy")) break;
                if (ref_path) { // the line reform --to_ref prints, the refined durations in its ss:Z:
                    const pg_mvops_projection &pr = route.pr;
                    h_ts.resize(n); h_te.resize(n); h_opt.resize(n_ops); h_opoff.resize(n + 1);
                    if (!hip_ok(hipMemcpy(h_ts.data(), pr.target_start, n * 4, hipMemcpyDeviceToHost), "hipMemcpy") || !hip_ok(hipMemcpy(h_te.data(), pr.target_end, n * 4, hipMemcpyDeviceToHost), "hipMemcpy") ||
                        (n_ops && !hip_ok(hipMemcpy(h_opt.data(), pr.op_t, n_ops, hipMemcpyDeviceToHost), "hipMemcpy")) ||
                        !hip_ok(hipMemcpy(h_opoff.data(), pr.op_off, (n + 1) * 8, hipMemcpyDeviceToHost), "hipMemcpy")) break;
                    for (size_t i = 0; i < n; i++) {
                        const bool reverse = both_strands && (rb.flag[i] & 0x10u);
                        const char *id = rb.names[i].c_str();
                        fprintf(fp, "%s\t%" PRIu64 "\t%d\t%d\t%c\t%s%s\t%" PRId64 "\t%d\t%d\t%" PRIu32 "\t%" PRIu32 "\t255\tss:Z:", id, rb.ns[i], h_qs[i], pr.query_end_host[i], reverse ? '-' : '+',
                                rb.rname[i].c_str(), reverse ? rc_suffix : "", rb.ref_len[i], h_ts[i], h_te[i], pr.n_match_host[i], pr.ref_len_host[i]);
                        for (uint64_t e = h_opoff[i]; e < h_opoff[i + 1]; e++) fprintf(fp, "%" PRIu32 "%c", h_ops[e], ",ID"[h_opt[e] < 3 ? h_opt[e] : 0]);
                        fputc('\n', fp);
                        if (rf) rr.row(rf, id, i);
                    }
                }
                uint64_t at = 0;
                for (size_t i = 0; !ref_path && i < n; i++) {
                    const uint32_t lb = rb.l_seq[i];
                    uint64_t end = (uint64_t)(int64_t)h_qs[i];
                    for (uint32_t e = 0; e < lb; e++) end += h_ops[at + e];
                    const char *id = rb.names[i].c_str();
                    fprintf(fp, "%s\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t+\t%s\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t255\tss:Z:", id, rb.ns[i],
                            (uint64_t)(int64_t)h_qs[i], end, id, lb, rna ? lb : 0u, rna ? 0u : lb, lb, lb);
                    for (uint32_t e = 0; e < lb; e++) fprintf(fp, "%" PRIu32 ",", h_ops[at + e]);
                    fputc('\n', fp);
                    at += lb;
                    if (rf) rr.row(rf, id, i);
                }
            }
        }
        if (status == EXIT_SUCCESS && !bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); status = EXIT_FAILURE; }
    }
    pg_fit_result res, res2; memset(&res, 0, sizeof res); memset(&res2, 0, sizeof res2);
    if (status == EXIT_SUCCESS && (pg_fit_finish(fit, &res) != PG_OK || pg_fit_finish(fit2, &res2) != PG_OK)) { fprintf(stderr, "[realign] %s%s\n", pg_fit_last_error(fit), pg_fit_last_error(fit2)); status = EXIT_FAILURE; }
    if (status == EXIT_SUCCESS) {
        if (kmer_path) status = write_kmer_table(kmer_path, k, uses_u != 0, levels, res2);
        const std::string rounds_text = rounds > 1 ? " rounds=" + std::to_string(rounds) : std::string();
        fprintf(stderr, "[realign] k=%u band=%lld min_len=%lld%s reads=%llu refined=%llu free=%llu moved=%llu rms_resid_before=%s rms_resid_after=%s\n", k, band, min_len,
                rounds_text.c_str(), (unsigned long long)res.reads, (unsigned long long)res.fitted, (unsigned long long)rr.n_free, (unsigned long long)rr.n_moved, pooled_rms(res, n_slots).c_str(),
                pooled_rms(res2, n_slots).c_str());
    }
    if (ref_path) route.print_skipped("realign");
    finish_files();
    route.release();
    release();
    return status;
}
