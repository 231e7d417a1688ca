// eventalign_cli.cpp -- `poregen eventalign`: the per-event table of a dataset against a k-mer model, the view scripts/eventaling.sh asks
// f5c eventalign --kmer-model for. The events are the basecaller's segmentation (refined by --realign where asked), not f5c's; the columns
// and their meaning are nanopolish / f5c `eventalign --scale-events --signal-index`. The records are read as `fit` reads them, every batch is
// expanded (and, with --ref, projected onto the reference), fitted (pg_fit_submit: sample = shift + scale * level per read) and its counted
// events are written one line each on the device (pg_evalign_*, include/pgmove.h; the rule: csrc/pg_evalign.h).
#include "pg_cli.h"
#include "pg_moverecs.h"
#include "../pg_evalign.h"
#include "../pg_realign.h"

#include <getopt.h>

namespace {

const struct option kLongOptions[] = {
    {"rna", no_argument, nullptr, 0},              // 0
    {"n_to_t", no_argument, nullptr, 0},           // 1
    {"min_dur", required_argument, nullptr, 0},    // 2
    {"max_dur", required_argument, nullptr, 0},    // 3
    {"min_events", required_argument, nullptr, 0}, // 4
    {"summary", required_argument, nullptr, 0},    // 5
    {"batch_reads", required_argument, nullptr, 0},// 6
    {"device", required_argument, nullptr, 0},     // 7
    {"help", no_argument, nullptr, 'h'},           // 8
    {"ref", required_argument, nullptr, 0},        // 9
    {"both_strands", no_argument, nullptr, 0},     // 10
    {"realign", no_argument, nullptr, 0},          // 11
    {"band", required_argument, nullptr, 0},       // 12
    {"rounds", required_argument, nullptr, 0},     // 13
    {"min_len", required_argument, nullptr, 0},    // 14
    {"print_read_names", no_argument, nullptr, 0}, // 15
    {"sample_rate", required_argument, nullptr, 0},// 16
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen eventalign [options] -o FILE MODEL reads.slow5/blow5 reads.bam/sam\n");
    fprintf(fp, "       poregen eventalign --ref REF.fa [--both_strands] [options] -o FILE MODEL reads.slow5/blow5 mapped.bam/sam\n");
    fprintf(fp, "\none line per event that `poregen fit` counts: where it lies, its level and spread in the model's units, the model's level and level_stdv\n");
    fprintf(fp, "for its k-mer and the standardized level; the columns of nanopolish / f5c eventalign --scale-events --signal-index\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   -o FILE                    the table (required)\n");
    fprintf(fp, "   -k INT                     k-mer length; must be the model's [the model's]\n");
    fprintf(fp, "   -m INT                     move start offset [0]\n");
    fprintf(fp, "   --rna                      the dataset is direct RNA\n");
    fprintf(fp, "   --n_to_t                   an N of a read counts as T\n");
    fprintf(fp, "   --ref REF.fa               a MAPPED .bam / .sam: the k-mers and positions are the reference's, as `fit --ref` takes them; contig is RNAME\n");
    fprintf(fp, "   --both_strands             with --ref: reverse-strand records are taken too; their position and reference_kmer are the forward strand's\n");
    fprintf(fp, "   --min_dur INT              minimum number of samples of an event, from 1 [5]\n");
    fprintf(fp, "   --max_dur INT              maximum number of samples of an event, up to %u [70]\n", PG_EA_MAX_DUR);
    fprintf(fp, "   --min_events INT           counted events a read needs to be fitted [20]\n");
    fprintf(fp, "   --realign                  refine the boundaries against the model first (as `poregen realign`); the rows are those of the refined ops\n");
    fprintf(fp, "   --band INT                 with --realign: how far a boundary may move [10]\n");
    fprintf(fp, "   --rounds INT               with --realign: rounds of fit and realign, 1 to 8 [1]\n");
    fprintf(fp, "   --min_len INT              with --realign: the fewest samples a refined event keeps [3]\n");
    fprintf(fp, "   --print_read_names         read_index is the read's name [its 0-based index among the records taken]\n");
    fprintf(fp, "   --sample_rate INT          event_length in seconds at this many samples per second, 1 to %u [in samples]\n", PG_EA_MAX_RATE);
    fprintf(fp, "   --summary FILE             the per-read table `poregen fit -o` writes, for this run\n");
    fprintf(fp, "   --batch_reads INT          reads per device batch [4000]\n");
    fprintf(fp, "   --device INT               HIP device [0]\n");
    fprintf(fp, "   -v INT                     verbosity; from 4 the kernel times [0]\n");
    fprintf(fp, "   -h                         help\n");
}

} // namespace

int eventalign_main(int argc, char **argv) {
    long long k_opt = 0, m = 0, min_dur = 5, max_dur = 70, min_events = 20, batch_reads = 4000, device = 0, min_len = 3, band = 10, rounds = 1, sample_rate = 0, verbose = 0;
    bool rna = false, n_to_t = false, help = false, both_strands = false, realign = false, read_names = false, realign_opt = false;
    const char *out_path = nullptr, *summary_path = nullptr, *ref_path = nullptr;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "k:m:o:v:h", kLongOptions, &longindex)) >= 0) {
        bool ok = true;
        if (c == 'k') ok = whole_int(optarg, 1, PG_FIT_MAX_K, k_opt);
        else if (c == 'm') ok = whole_int(optarg, 0, 64, m);
        else if (c == 'o') out_path = optarg;
        else if (c == 'v') ok = whole_int(optarg, 0, 10, verbose);
        else if (c == 'h') help = true;
        else if (c == 0 && longindex == 0) rna = true;
        else if (c == 0 && longindex == 1) n_to_t = true;
        else if (c == 0 && longindex == 2) ok = whole_int(optarg, 1, PG_EA_MAX_DUR, min_dur);
        else if (c == 0 && longindex == 3) ok = whole_int(optarg, 1, PG_EA_MAX_DUR, max_dur);
        else if (c == 0 && longindex == 4) ok = whole_int(optarg, 0, 0xffffffffll, min_events);
        else if (c == 0 && longindex == 5) summary_path = optarg;
        else if (c == 0 && longindex == 6) ok = whole_int(optarg, 1, 1 << 24, batch_reads);
        else if (c == 0 && longindex == 7) ok = whole_int(optarg, 0, 1024, device);
        else if (c == 0 && longindex == 9) ref_path = optarg;
        else if (c == 0 && longindex == 10) both_strands = true;
        else if (c == 0 && longindex == 11) realign = true;
        else if (c == 0 && longindex == 12) { ok = whole_int(optarg, 0, PG_RL_MAX_BAND, band); realign_opt = true; }
        else if (c == 0 && longindex == 13) { ok = whole_int(optarg, 1, 8, rounds); realign_opt = true; }
        else if (c == 0 && longindex == 14) { ok = whole_int(optarg, 1, PG_EA_MAX_DUR, min_len); realign_opt = true; }
        else if (c == 0 && longindex == 15) read_names = true;
        else if (c == 0 && longindex == 16) ok = whole_int(optarg, 1, PG_EA_MAX_RATE, sample_rate);
        else { print_help(stderr); return EXIT_FAILURE; }
        if (!ok) {
            fprintf(stderr, "[eventalign] %s%s: '%s' is not a value it takes (-k 1..9, -m 0..64, durations 1..%u, --sample_rate 1..%u, --min_len from 1, --band 0..%u, --rounds 1..8)\n",
                    c ? "-" : "--", c ? std::string(1, (char)c).c_str() : kLongOptions[longindex].name, optarg, PG_EA_MAX_DUR, PG_EA_MAX_RATE, PG_RL_MAX_BAND);
            return EXIT_FAILURE;
        }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    if (argc - optind != 3) { print_help(stderr); return EXIT_FAILURE; }
    if (!out_path) { fprintf(stderr, "[eventalign] -o FILE is required\n"); print_help(stderr); return EXIT_FAILURE; }
    if (min_dur > max_dur) return die("[eventalign] --min_dur may not exceed --max_dur");
    if (realign_opt && !realign) return die("[eventalign] --band, --rounds and --min_len apply with --realign only");
    if (realign && min_len > min_dur) return die("[eventalign] --min_len may not exceed --min_dur");
    if (both_strands && !ref_path) return die("[eventalign] --both_strands applies with --ref only");
    if (ref_path && n_to_t) return die("[eventalign] --ref cannot be combined with --n_to_t: the sequence is the reference's, there is nothing to rewrite");
    const char *model_path = argv[optind], *slow5_path = argv[optind + 1], *sam_path = argv[optind + 2];
    if (!is_sam_or_bam(sam_path)) return die("[eventalign] the records come from a .bam or .sam file, not %s", sam_path);
    std::vector<uint32_t> levels, stdvs;
    uint32_t k = 0; int32_t uses_u = 0;
    if (!load_level_model("eventalign", model_path, k_opt, levels, k, uses_u, &stdvs)) return EXIT_FAILURE;
    RefRoute route; // --ref: the FASTA, the projection and the slices of every batch
    route.both_strands = both_strands; route.rna = rna;
    if (ref_path) {
        std::string ferr;
        if (!route.fai.load(ref_path, ferr)) { fprintf(stderr, "Error in loading the reference %s%s%s\n", ref_path, ferr.empty() ? "" : ": ", ferr.c_str()); return EXIT_FAILURE; }
    }
    std::string err;
    pgh::Slow5File s5;
    if (!s5.open(slow5_path, err)) { fprintf(stderr, "Error in opening file %s\n[eventalign] %s\n", slow5_path, err.c_str()); return EXIT_FAILURE; }
    pgh::SamBamReader sam;
    if (!sam.open(sam_path, err)) return die("[eventalign] %s", err);
    FILE *fp = fopen(out_path, "w"), *sf = nullptr;
    if (!fp) return die("Could not open %s for writing.", out_path);
    auto finish_files = [&]() { if (fp) fclose(fp); fp = nullptr; if (sf) fclose(sf); sf = nullptr; };
    if (summary_path && !(sf = fopen(summary_path, "w"))) { finish_files(); return die("Could not open %s for writing.", summary_path); }

    pg_fit_params prm; memset(&prm, 0, sizeof prm);
    prm.struct_size = sizeof prm; prm.sig_move_offset = (uint32_t)m; prm.min_dur = (uint32_t)min_dur; prm.max_dur = (uint32_t)max_dur; prm.min_events = (uint32_t)min_events; prm.rna = rna;
    pg_realign_params rp; memset(&rp, 0, sizeof rp);
    rp.struct_size = sizeof rp; rp.sig_move_offset = (uint32_t)m; rp.min_dur = (uint32_t)min_dur; rp.max_dur = (uint32_t)max_dur; rp.rna = rna; rp.band = (uint32_t)band; rp.min_len = (uint32_t)min_len;
    pg_evalign_params ep; memset(&ep, 0, sizeof ep);
    ep.struct_size = sizeof ep; ep.sig_move_offset = (uint32_t)m; ep.min_dur = (uint32_t)min_dur; ep.max_dur = (uint32_t)max_dur; ep.rna = rna; ep.sample_rate = (uint32_t)sample_rate;
    ep.flags = PG_EVALIGN_TEXT;
    pg_fit *fit = nullptr, *fitr = nullptr; pg_realign *ra = nullptr; pg_evalign *ea = nullptr; pg_mvops *ex = nullptr; // fitr: the fits of the rounds, whose sums nobody reads
    int status = EXIT_SUCCESS;
    auto release = [&]() { if (fit) pg_fit_destroy(fit); if (fitr) pg_fit_destroy(fitr); if (ra) pg_realign_destroy(ra); if (ea) pg_evalign_destroy(ea); if (ex) pg_mvops_destroy(ex); };
    if (pg_fit_create(&prm, (int32_t)device, &fit) != PG_OK || (realign && pg_fit_create(&prm, (int32_t)device, &fitr) != PG_OK)) { fprintf(stderr, "[eventalign] %s\n", pg_fit_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (realign && pg_realign_create(&rp, (int32_t)device, &ra) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_realign_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_evalign_create(&ep, (int32_t)device, &ea) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_evalign_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_mvops_create((int32_t)device, &ex) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_mvops_last_error(nullptr)); status = EXIT_FAILURE; }
    else if (pg_fit_set_model(fit, levels.data(), k) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; }
    else if (fitr && pg_fit_set_model(fitr, levels.data(), k) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_fit_last_error(fitr)); status = EXIT_FAILURE; }
    else if (ra && pg_realign_set_model(ra, levels.data(), k) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_realign_last_error(ra)); status = EXIT_FAILURE; }
    else if (pg_evalign_set_model(ea, levels.data(), stdvs.data(), k) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_evalign_last_error(ea)); status = EXIT_FAILURE; }
    if (status != EXIT_SUCCESS) { release(); finish_files(); return status; }
    // the expander's stream carries the signal's upload, the expansion, the fits, the alignment and the table: one queue, in order
    const hipStream_t xs = (hipStream_t)pg_mvops_stream(ex);
    if (pg_fit_set_stream(fit, xs) != PG_OK || (fitr && pg_fit_set_stream(fitr, xs) != PG_OK) || (ra && pg_realign_set_stream(ra, xs) != PG_OK) || pg_evalign_set_stream(ea, xs) != PG_OK) {
        fprintf(stderr, "[eventalign] cannot share the expander's stream\n"); status = EXIT_FAILURE;
    }

    PgDev<int16_t> d_sig; PgDev<uint64_t> d_sigoff; PgDev<uint8_t> d_seq; PgDev<uint64_t> d_seqoff;
    RealignRounds rr;
    std::vector<int64_t> ref_start; std::vector<uint8_t> reverse, contig, label; std::vector<uint64_t> contig_off, label_off;
    std::vector<char> text;
    uint64_t taken = 0, reads = 0, fitted = 0, rows = 0, text_bytes = 0;
    double ms[3] = {0, 0, 0};
    bool header_written = false;
    pgh::MoveSignalBatches in(sam, s5, "eventalign", (size_t)batch_reads, (size_t)(PG_FIT_BATCH_SAMPLES / 2), (size_t)PG_FIT_BATCH_SAMPLES);
    const pgh::MoveRecs &rb = in.recs;
    const HipOk hip_ok{"eventalign", &status};
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
            if (pg_mvops_expand(ex, &mb, &mr) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_mvops_last_error(ex)); status = EXIT_FAILURE; break; }
            pg_batch b = device_batch(mr, n, 0, d_sig.p, d_sigoff.p);
            const uint32_t *skip = mr.status_host;
            if (ref_path) { // the ops onto the reference, the slices of REF.fa: a gapped batch; a record reform --to_ref ends on ends the run
                bool cut = false;
                if (!route.project("eventalign", ex, rb, mr, n, bad, cut)) { status = EXIT_FAILURE; break; }
                if (!route.slices("eventalign", hip_ok, (int)device, xs, rb, n) || (n && !route.to_device(hip_ok, xs, n, d_seq, d_seqoff))) { status = EXIT_FAILURE; break; }
                b = route.gapped_batch(n, d_sig.p, d_sigoff.p, d_seq.p, d_seqoff.p);
                skip = nullptr; // (every read in front of a refused one is accepted)
            }
            if (n && realign) { // the rows are those of the last round's ops and of a fit on them (a read reform refuses has no ops: nothing of it moves)
                if (!rr.run(fitr, fitr, ra, b, rounds)) { fprintf(stderr, "[eventalign] %s\n", rr.err.c_str()); status = EXIT_FAILURE; break; }
                b.op_n = rr.op_n;
            }
            pg_fit_reads fr; memset(&fr, 0, sizeof fr);
            if (n && pg_fit_submit(fit, &b, skip, &fr) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_fit_last_error(fit)); status = EXIT_FAILURE; break; }
            for (size_t i = 0; sf && i < n; i++) {
                const pg_fit_sums &q = fr.sums[i];
                fprintf(sf, "%s\t%s\t%lld\t%lld\t", rb.names[i].c_str(), fit_status_name(fr.status[i]), (long long)q.e, (long long)q.n);
                if (fr.status[i] == PG_FIT_ST_OK) {
                    long double rep[3];
                    pg_fit_report(PgFitSums{q.n, q.sl, q.sll, q.sr, q.srl, q.srr, q.e}, in.dig[i], in.off[i], in.range[i], rep);
                    fprintf(sf, "%.6Lf\t%.6Lf\t%.6Lf\n", rep[0], rep[1], rep[2]);
                } else fprintf(sf, "\t\t\n");
            }
            if (n) {
                // what the text says of every read beyond its rows
                ref_start.assign(n, 0); reverse.assign(n, 0); contig.clear(); label.clear(); contig_off.assign(1, 0); label_off.assign(1, 0);
                for (size_t i = 0; i < n; i++) {
                    const std::string &cn = ref_path ? rb.rname[i] : rb.names[i];
                    const std::string ln = read_names ? rb.names[i] : std::to_string(taken + i);
                    contig.insert(contig.end(), cn.begin(), cn.end()); contig_off.push_back(contig.size());
                    label.insert(label.end(), ln.begin(), ln.end()); label_off.push_back(label.size());
                    if (ref_path) { ref_start[i] = rb.pos[i]; reverse[i] = both_strands && (rb.flag[i] & 0x10u) ? 1 : 0; }
                    fitted += fr.status[i] == PG_FIT_ST_OK;
                }
                pg_evalign_meta meta; memset(&meta, 0, sizeof meta);
                meta.ref_start = ref_start.data(); meta.reverse = reverse.data(); meta.contig = contig.data(); meta.contig_off = contig_off.data(); meta.label = label.data(); meta.label_off = label_off.data();
                pg_evalign_out eo; memset(&eo, 0, sizeof eo); eo.struct_size = sizeof eo;
                if (pg_evalign_submit(ea, &b, fr.status, fr.a, fr.b, &meta, &eo) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_evalign_last_error(ea)); status = EXIT_FAILURE; break; }
                text.resize(eo.text_bytes);
                if (pg_evalign_copy_text(ea, text.data(), text.size()) != PG_OK) { fprintf(stderr, "[eventalign] %s\n", pg_evalign_last_error(ea)); status = EXIT_FAILURE; break; }
                const size_t hdr = strlen(PG_EA_HEADER), from = header_written ? hdr : 0; // every batch's text starts with the header line: the file keeps the first
                if (fwrite(text.data() + from, 1, text.size() - from, fp) != text.size() - from) { fprintf(stderr, "Error in writing %s.\n", out_path); status = EXIT_FAILURE; break; }
                header_written = true;
                double t[3] = {0, 0, 0};
                pg_evalign_kernel_ms(ea, t);
                for (int j = 0; j < 3; j++) ms[j] += t[j];
                taken += n; reads += n; rows += eo.n_rows; text_bytes += text.size() - from;
            }
        }
        if (status == EXIT_SUCCESS && !bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); status = EXIT_FAILURE; }
    }
    if (!header_written && fp) { fputs(PG_EA_HEADER, fp); text_bytes += strlen(PG_EA_HEADER); } // no record at all: the header alone
    if (status == EXIT_SUCCESS) {
        fprintf(stderr, "[eventalign] k=%u reads=%llu fitted=%llu rows=%llu text_bytes=%llu\n", k, (unsigned long long)reads, (unsigned long long)fitted, (unsigned long long)rows,
                (unsigned long long)text_bytes);
        if (verbose >= 4) fprintf(stderr, "[eventalign] kernels: count %.3f ms, rows %.3f ms, text %.3f ms\n", ms[0], ms[1], ms[2]);
    }
    if (ref_path) route.print_skipped("eventalign");
    if (fp && fclose(fp) != 0 && status == EXIT_SUCCESS) { fprintf(stderr, "Error in writing %s.\n", out_path); status = EXIT_FAILURE; }
    fp = nullptr;
    finish_files();
    route.release();
    release();
    return status;
}
