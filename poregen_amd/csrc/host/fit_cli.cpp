// fit_cli.cpp -- `poregen fit`: how well does a k-mer model explain a dataset? The reference asks other tools (scripts/eventaling.sh runs f5c
// eventalign --kmer-model, scripts/sim.sh squigulator, a basecaller and an identity script); here the question goes to the basecaller's own
// segmentation. The records are read as `gmove --reform` reads them (move arrays and packed bases to the device, pg_mvops_expand, untrimmed
// signal), every read is calibrated against the model -- sample = shift + scale * level, least squares over its counted events -- and every
// k-mer's samples are then compared with the level the model claims (pg_fit_*, include/pgmove.h; the rule: csrc/pg_fit.h).
//   per read   read_id  status  n_events  n_samples  shift  scale  rms          (the three numbers "%.6f", empty unless the status is ok)
//   per k-mer  KMER  n_samples  n_events  level  mean_resid  rms_resid           (pA with three decimals; the last two empty when n_samples is 0)
#include "pg_cli.h"
#include "pg_moverecs.h"

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
    {"help", no_argument, nullptr, 'h'},           // 8
    {"ref", required_argument, nullptr, 0},        // 9
    {"both_strands", no_argument, nullptr, 0},     // 10
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen fit [options] MODEL reads.slow5/blow5 reads.bam/sam\n");
    fprintf(fp, "       poregen fit --ref REF.fa [--both_strands] [options] MODEL reads.slow5/blow5 mapped.bam/sam\n");
    fprintf(fp, "\nscore a k-mer model against the signal and the move tables: per read sample = shift + scale * level, per k-mer the residuals\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   -k INT                     k-mer length; must be the model's [the model's]\n");
    fprintf(fp, "   -m INT                     move start offset [0]\n");
    fprintf(fp, "   --rna                      the dataset is direct RNA\n");
    fprintf(fp, "   --n_to_t                   an N of a read counts as T\n");
    fprintf(fp, "   --ref REF.fa               a MAPPED .bam / .sam: score the model against the k-mers the REFERENCE spells -- the ops are carried through each\n");
    fprintf(fp, "                              record's CIGAR on the GPU and the sequence is the record's slice of REF.fa, as `gmove --reform --ref` takes them;\n");
    fprintf(fp, "                              an event counts when the k ops of its window are matches. Unmapped and reverse-strand records are skipped and\n");
    fprintf(fp, "                              counted; a read whose slice REF.fa lacks has the status ref_length. Not with --n_to_t\n");
    fprintf(fp, "   --both_strands             with --ref: reverse-strand records are taken too, as `gmove --reform --ref --both_strands` takes them\n");
    fprintf(fp, "   --min_dur INT              minimum number of samples of an event [5]\n");
    fprintf(fp, "   --max_dur INT              maximum number of samples of an event [70]\n");
    fprintf(fp, "   --min_events INT           counted events a read needs to be fitted [20]\n");
    fprintf(fp, "   -o FILE                    the per-read table [stdout]\n");
    fprintf(fp, "   --kmer_table FILE          the per-k-mer table\n");
    fprintf(fp, "   --batch_reads INT          reads per device batch [4000]\n");
    fprintf(fp, "   --device INT               HIP device [0]\n");
    fprintf(fp, "   -h                         help\n");
}

} // namespace

int fit_main(int argc, char **argv) {
    long long k_opt = 0, m = 0, min_dur = 5, max_dur = 70, min_events = 20, batch_reads = 4000, device = 0;
    bool rna = false, n_to_t = false, help = false;
    const char *out_path = nullptr, *kmer_path = nullptr, *ref_path = nullptr;
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
        else if (c == 0 && longindex == 2) ok = whole_int(optarg, 0, PG_FIT_MAX_DUR, min_dur);
        else if (c == 0 && longindex == 3) ok = whole_int(optarg, 0, PG_FIT_MAX_DUR, max_dur);
        else if (c == 0 && longindex == 4) ok = whole_int(optarg, 0, 0xffffffffll, min_events);
        else if (c == 0 && longindex == 5) kmer_path = optarg;
        else if (c == 0 && longindex == 6) ok = whole_int(optarg, 1, 1 << 24, batch_reads);
        else if (c == 0 && longindex == 7) ok = whole_int(optarg, 0, 1024, device);
        else if (c == 0 && longindex == 9) ref_path = optarg;
        else if (c == 0 && longindex == 10) both_strands = true;
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
    if (both_strands && !ref_path) return die("[fit] --both_strands applies with --ref only");
    if (ref_path && n_to_t) return die("[fit] --ref cannot be combined with --n_to_t: the sequence is the reference's, there is nothing to rewrite");
    const char *model_path = argv[optind], *slow5_path = argv[optind + 1], *sam_path = argv[optind + 2];
    if (!is_sam_or_bam(sam_path)) return die("[fit] the records come from a .bam or .sam file, not %s", sam_path);
    std::vector<uint32_t> levels;
    uint32_t k = 0; int32_t uses_u = 0;
    if (!load_level_model("fit", model_path, k_opt, levels, k, uses_u)) return EXIT_FAILURE;
    RefRoute route; // --ref: the FASTA, the projection and the slices of every batch
    route.both_strands = both_strands; route.rna = rna;
    if (ref_path) {
        std::string ferr;
        if (!route.fai.load(ref_path, ferr)) { fprintf(stderr, "Error in loading the reference %s%s%s\n", ref_path, ferr.empty() ? "" : ": ", ferr.c_str()); return EXIT_FAILURE; }
    }
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

    PgDev<int16_t> d_sig; PgDev<uint64_t> d_sigoff; PgDev<uint8_t> d_seq; PgDev<uint64_t> d_seqoff;
    pgh::MoveSignalBatches in(sam, s5, "fit", (size_t)batch_reads, (size_t)(PG_FIT_BATCH_SAMPLES / 2), (size_t)PG_FIT_BATCH_SAMPLES);
    const HipOk hip_ok{"fit", &status};
    if (ref_path) { in.to_ref_skipped = route.skipped_counter(); in.reverse_taken = route.reverse_counter(); }
    while (!in.done() && status == EXIT_SUCCESS) {
        // ---- the records: the first one that cannot be taken ends the run behind the reads in front of it, with gmove --reform's message
        std::string bad;
        in.next(bad);
        size_t n = in.recs.size();
        if (n) {
            if (!hip_ok(hipSetDevice((int)device), "hipSetDevice") || !upload_signal(hip_ok, d_sig, d_sigoff, in.sig, in.sig_off, xs)) break;
            pg_mvops_batch mb;
            in.recs.fill(mb, n, (rna ? PG_MVOPS_RNA : 0) | (n_to_t ? PG_MVOPS_N_TO_T : 0));
            pg_mvops_result mr;
            if (pg_mvops_expand(ex, &mb, &mr) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_mvops_last_error(ex)); status = EXIT_FAILURE; break; }
            pg_batch b = device_batch(mr, n, 0, d_sig.p, d_sigoff.p);
            const uint32_t *skip = mr.status_host;
            if (ref_path) { // the ops onto the reference, the slices of REF.fa: a gapped batch; a record reform --to_ref ends on ends the run
                bool cut = false;
                if (!route.project("fit", ex, in.recs, mr, n, bad, cut)) { status = EXIT_FAILURE; break; }
                if (!route.slices("fit", hip_ok, (int)device, xs, in.recs, n) || (n && !route.to_device(hip_ok, xs, n, d_seq, d_seqoff))) { status = EXIT_FAILURE; break; }
                b = route.gapped_batch(n, d_sig.p, d_sigoff.p, d_seq.p, d_seqoff.p);
                skip = nullptr; // (every read in front of a refused one is accepted)
            }
            pg_fit_reads fr; memset(&fr, 0, sizeof fr);
            if (n && pg_fit_submit(fit, &b, skip, &fr) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; break; }
            for (size_t i = 0; i < n; i++) {
                const pg_fit_sums &q = fr.sums[i];
                fprintf(fp, "%s\t%s\t%lld\t%lld\t", in.recs.names[i].c_str(), fit_status_name(fr.status[i]), (long long)q.e, (long long)q.n);
                if (fr.status[i] == PG_FIT_ST_OK) {
                    long double rep[3];
                    pg_fit_report(PgFitSums{q.n, q.sl, q.sll, q.sr, q.srl, q.srr, q.e}, in.dig[i], in.off[i], in.range[i], rep);
                    fprintf(fp, "%.6Lf\t%.6Lf\t%.6Lf\n", rep[0], rep[1], rep[2]);
                } else fprintf(fp, "\t\t\n");
            }
        }
        if (status == EXIT_SUCCESS && !bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); status = EXIT_FAILURE; }
    }
    pg_fit_result res; memset(&res, 0, sizeof res);
    if (status == EXIT_SUCCESS && pg_fit_finish(fit, &res) != PG_OK) { fprintf(stderr, "[fit] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; }
    if (status == EXIT_SUCCESS) {
        if (kmer_path) status = write_kmer_table(kmer_path, k, uses_u != 0, levels, res);
        fprintf(stderr, "[fit] k=%u reads=%llu fitted=%llu events=%llu samples=%llu clamped=%llu rms_resid=%s\n", k, (unsigned long long)res.reads, (unsigned long long)res.fitted,
                (unsigned long long)res.events, (unsigned long long)res.samples, (unsigned long long)res.clamped, pooled_rms(res, n_slots).c_str());
    }
    if (ref_path) route.print_skipped("fit");
    finish_files();
    pg_fit_destroy(fit);
    route.release();
    pg_mvops_destroy(ex);
    return status;
}
