// simulate_cli.cpp -- `poregen simulate`: raw signal and the alignment that is true by construction, drawn from a k-mer model. The reference
// asks squigulator (scripts/sim.sh); the rule here is this project's own, fit's inverted (csrc/pg_sim.h, pg_sim_* of include/pgmove.h), and
// no squigulator output is reproduced. Reads are drawn from the reference sequences on the host (stream 0 of the generator), the signal and
// the ops come from the device, batch after batch; the files that belong together are written from them:
//   -o reads.slow5 / .blow5   the signal (ASCII SLOW5, or BLOW5: as it is, or with --compress zlib|zstd records and / or --sig_compress svb-zd
//                             signals, whose blocks are encoded on the device (pg_sigenc_*) and copied back in place of the samples)
//   -c FILE                   the TRUE alignment, as the PAF `poregen reform -c -k 1 -m 0 --stride 0 [--rna]` prints
//   -q FILE                   the reads as FASTQ
//   --moves FILE              a headerless SAM as a basecaller writes it: mv:B:c with every true boundary rounded to the stride from ts
#include "../pg_sim.h"
#include "pg_cli.h"

#include <algorithm>
#include <cerrno>
#include <getopt.h>
#include <thread>

namespace {

const struct option kLongOptions[] = {
    {"rna", no_argument, nullptr, 0},                 // 0
    {"seed", required_argument, nullptr, 0},          // 1
    {"read_len", required_argument, nullptr, 0},      // 2
    {"full_contigs", no_argument, nullptr, 0},        // 3
    {"dwell_mean", required_argument, nullptr, 0},    // 4
    {"dwell_model", required_argument, nullptr, 0},   // 5
    {"dwell_spread", required_argument, nullptr, 0},  // 6
    {"noise_scale", required_argument, nullptr, 0},   // 7
    {"ideal", no_argument, nullptr, 0},               // 8
    {"digitisation", required_argument, nullptr, 0},  // 9
    {"range", required_argument, nullptr, 0},         // 10
    {"offset", required_argument, nullptr, 0},        // 11
    {"offset_spread", required_argument, nullptr, 0}, // 12
    {"lead", required_argument, nullptr, 0},          // 13
    {"moves", required_argument, nullptr, 0},         // 14
    {"stride", required_argument, nullptr, 0},        // 15
    {"batch_reads", required_argument, nullptr, 0},   // 16
    {"device", required_argument, nullptr, 0},        // 17
    {"compress", required_argument, nullptr, 0},      // 18
    {"sig_compress", required_argument, nullptr, 0},  // 19
    {"help", no_argument, nullptr, 'h'},
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen simulate [options] -o reads.slow5/blow5 MODEL ref.fa/fasta\n");
    fprintf(fp, "\nraw signal and its true alignment drawn from a k-mer model (the project's own rule, not squigulator's)\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   -k INT                     k-mer length; must be the model's [the model's]\n");
    fprintf(fp, "   -m INT                     move start offset [0]\n");
    fprintf(fp, "   --rna                      direct RNA: forward strand only, the 3' end passes the pore first\n");
    fprintf(fp, "   --seed INT                 seed of the generator [0]\n");
    fprintf(fp, "   -n INT                     reads to draw [1000]\n");
    fprintf(fp, "   --read_len INT             mean read length; lengths are uniform in [read_len / 2, 3 read_len / 2], cut at the contig's end [4000]\n");
    fprintf(fp, "   --full_contigs             one read per contig instead\n");
    fprintf(fp, "   --dwell_mean INT           samples per base of a k-mer --dwell_model does not give [10]\n");
    fprintf(fp, "   --dwell_model FILE         KMER<TAB>median dwell, as `poregen model --dwell_model` writes it\n");
    fprintf(fp, "   --dwell_spread PCT         a dwell is uniform within +-PCT percent of its k-mer's [50]\n");
    fprintf(fp, "   --noise_scale NUM          the model's level_stdv times NUM (in steps of 1/256) [1]\n");
    fprintf(fp, "   --ideal                    no noise\n");
    fprintf(fp, "   --digitisation INT         [8192]\n");
    fprintf(fp, "   --range NUM                in pA [1467.61]\n");
    fprintf(fp, "   --offset INT               [10]\n");
    fprintf(fp, "   --offset_spread INT        a read's offset is uniform within +-INT of --offset [10]\n");
    fprintf(fp, "   --lead INT                 samples in front of the first event [0]\n");
    fprintf(fp, "   -o FILE                    the signal: .slow5 (ASCII) or .blow5\n");
    fprintf(fp, "   --compress STR             .blow5: record compression, none, zlib or zstd [none]\n");
    fprintf(fp, "   --sig_compress STR         .blow5: signal compression, none or svb-zd (encoded on the device) [none]\n");
    fprintf(fp, "   -t INT                     threads that compress records, at most 16 [the smaller of 16 and the machine's]\n");
    fprintf(fp, "   -c FILE                    the true alignment: PAF with ss:Z:\n");
    fprintf(fp, "   -q FILE                    the reads: FASTQ\n");
    fprintf(fp, "   --moves FILE               SAM with mv:B:c, ts:i: and ns:i:, the boundaries rounded to --stride\n");
    fprintf(fp, "   --stride INT               stride of the move table [5, with --rna 10]\n");
    fprintf(fp, "   --batch_reads INT          reads per device batch [2000]\n");
    fprintf(fp, "   --device INT               HIP device [0]\n");
    fprintf(fp, "   -h                         help\n");
}

bool whole_u64(const char *s, unsigned long long &v) {
    char *end = nullptr;
    if (!s || !*s || *s == '+' || *s == '-') return false;
    errno = 0;
    v = strtoull(s, &end, 10);
    return *end == 0 && errno == 0;
}
// a non-negative decimal times mult, to the nearest integer with halves up, exactly
bool decimal_times(const char *s, uint32_t mult, uint32_t &out) {
    pgbc::Dec d;
    return s && *s && pgbc::parse(s, strlen(s), d) && !d.neg && pg_fit_round_dec(d, mult, out) == 0;
}

struct Contig { std::string name, seq; };
// a FASTA: names up to the first blank, sequence lines joined and upper-cased
bool read_fasta(const char *path, std::vector<Contig> &out, std::string &err) {
    pgh::MappedFile f;
    if (!f.open(path)) { err = std::string("cannot open ") + path; return false; }
    const char *p = f.data, *e = f.data + f.size;
    while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        const char *le = nl ? nl : e;
        const char *q = le;
        if (q > p && q[-1] == '\r') q--;
        if (q > p && *p == '>') {
            const char *t = p + 1;
            while (t < q && *t != ' ' && *t != '\t') t++;
            out.push_back(Contig{std::string(p + 1, t), ""});
        } else if (q > p) {
            if (out.empty()) { err = std::string(path) + " does not begin with a '>' line"; return false; }
            std::string &s = out.back().seq;
            for (const char *c = p; c < q; c++) s.push_back((*c >= 'a' && *c <= 'z') ? (char)(*c - 32) : *c);
        }
        p = nl ? nl + 1 : e;
    }
    if (out.empty()) { err = std::string(path) + " holds no sequence"; return false; }
    return true;
}
char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : (c == 'T' || c == 'U') ? 'A' : 'N'; }

} // namespace

int simulate_main(int argc, char **argv) {
    long long k_opt = 0, m = 0, n_reads = 1000, read_len = 4000, dwell_mean = 10, spread = 50, digitisation = 8192, offset = 10, off_spread = 10, lead = 0, stride = 0, batch_reads = 2000,
              device = 0, threads = 0;
    pgh::Slow5Writer::RecPress rec_press = pgh::Slow5Writer::REC_NONE;
    pgh::Slow5Writer::SigPress sig_press = pgh::Slow5Writer::SIG_NONE;
    unsigned long long seed = 0;
    uint32_t noise_q8 = 256, range_e4 = 14676100;
    bool rna = false, full = false, ideal = false, help = false;
    const char *out_path = nullptr, *paf_path = nullptr, *fq_path = nullptr, *sam_path = nullptr, *dwell_path = nullptr;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "k:m:n:o:c:q:t:h", kLongOptions, &longindex)) >= 0) {
        bool ok = true;
        if (c == 'k') ok = whole_int(optarg, 1, PG_FIT_MAX_K, k_opt);
        else if (c == 'm') ok = whole_int(optarg, 0, 64, m);
        else if (c == 'n') ok = whole_int(optarg, 1, 1ll << 40, n_reads);
        else if (c == 'o') out_path = optarg;
        else if (c == 'c') paf_path = optarg;
        else if (c == 'q') fq_path = optarg;
        else if (c == 't') ok = whole_int(optarg, 1, 1 << 20, threads);
        else if (c == 'h') help = true;
        else if (c == 0 && longindex == 0) rna = true;
        else if (c == 0 && longindex == 1) ok = whole_u64(optarg, seed);
        else if (c == 0 && longindex == 2) ok = whole_int(optarg, 1, 1 << 28, read_len);
        else if (c == 0 && longindex == 3) full = true;
        else if (c == 0 && longindex == 4) ok = whole_int(optarg, 1, PG_SIM_MAX_DWELL, dwell_mean);
        else if (c == 0 && longindex == 5) dwell_path = optarg;
        else if (c == 0 && longindex == 6) ok = whole_int(optarg, 0, 100, spread);
        else if (c == 0 && longindex == 7) ok = decimal_times(optarg, 256, noise_q8) && noise_q8 <= (1u << 16);
        else if (c == 0 && longindex == 8) ideal = true;
        else if (c == 0 && longindex == 9) ok = whole_int(optarg, 1, PG_SIM_MAX_DIGITISATION, digitisation);
        else if (c == 0 && longindex == 10) ok = decimal_times(optarg, 10000, range_e4) && range_e4 >= 1;
        else if (c == 0 && longindex == 11) ok = whole_int(optarg, -PG_SIM_MAX_OFFSET, PG_SIM_MAX_OFFSET, offset);
        else if (c == 0 && longindex == 12) ok = whole_int(optarg, 0, PG_SIM_MAX_OFF_SPREAD, off_spread);
        else if (c == 0 && longindex == 13) ok = whole_int(optarg, 0, PG_SIM_MAX_LEAD, lead);
        else if (c == 0 && longindex == 14) sam_path = optarg;
        else if (c == 0 && longindex == 15) ok = whole_int(optarg, 1, 127, stride);
        else if (c == 0 && longindex == 16) ok = whole_int(optarg, 1, 1 << 20, batch_reads);
        else if (c == 0 && longindex == 17) ok = whole_int(optarg, 0, 1024, device);
        else if (c == 0 && longindex == 18) ok = pgh::Slow5Writer::parse_rec_press(optarg, rec_press);
        else if (c == 0 && longindex == 19) ok = pgh::Slow5Writer::parse_sig_press(optarg, sig_press);
        else { print_help(stderr); return EXIT_FAILURE; }
        if (!ok) {
            fprintf(stderr, "[simulate] %s%s: '%s' is not a value it takes\n", c ? "-" : "--", c ? std::string(1, (char)c).c_str() : kLongOptions[longindex].name, optarg);
            return EXIT_FAILURE;
        }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    if (argc - optind != 2) { print_help(stderr); return EXIT_FAILURE; }
    if (!out_path) return die("[simulate] -o reads.slow5 or reads.blow5 is required");
    const bool blow5 = ends_with(out_path, ".blow5");
    if (!blow5 && !ends_with(out_path, ".slow5")) return die("[simulate] the signal goes to a .slow5 or .blow5 file, not %s", out_path);
    const bool svb = sig_press == pgh::Slow5Writer::SIG_SVB_ZD;
    if (!blow5 && (svb || rec_press != pgh::Slow5Writer::REC_NONE)) return die("[simulate] --compress and --sig_compress are for a .blow5 file; %s is ASCII", out_path);
    if (rec_press == pgh::Slow5Writer::REC_ZSTD && !pgh::Slow5Writer::zstd_available())
        return die("[simulate] --compress zstd needs libzstd.so.1, which was not found on this machine");
    // (a command may use 16 CPUs where the machine shows many times as many)
    if (!threads) threads = std::max(1u, std::thread::hardware_concurrency());
    threads = std::min(threads, 16ll);
    if (!stride) stride = rna ? 10 : 5;
    const char *model_path = argv[optind], *ref_path = argv[optind + 1];
    if (!pg_sim_q((uint32_t)digitisation, range_e4)) return die("[simulate] --digitisation / --range is too large (digitisation 10 2^32 / range in 1e-4 pA must stay below 2^40)");

    // ---- the model and the dwells: parsed and refused on the host, before any device is touched
    pgh::MappedFile mf;
    if (!mf.open(model_path)) return die("[simulate] cannot open the model %s", model_path);
    const size_t cap = (size_t)1 << (2 * PG_FIT_MAX_K);
    std::vector<uint32_t> levels(cap), stdvs(cap), dwells(cap, 0);
    uint32_t k = 0; int32_t uses_u = 0; char perr[400];
    if (pg_sim_parse_model(mf.data, mf.size, (uint32_t)k_opt, &k, levels.data(), stdvs.data(), cap, &uses_u, perr, sizeof perr) != PG_OK) {
        fprintf(stderr, "[simulate] the model %s is refused: %s\n", model_path, perr);
        return EXIT_FAILURE;
    }
    mf.close();
    const uint64_t n_slots = 1ull << (2 * k);
    if (dwell_path) {
        if (!mf.open(dwell_path)) return die("[simulate] cannot open the dwell model %s", dwell_path);
        uint32_t dk = 0;
        if (pg_sim_parse_dwell(mf.data, mf.size, k, &dk, dwells.data(), cap, perr, sizeof perr) != PG_OK) {
            fprintf(stderr, "[simulate] the dwell model %s is refused: %s\n", dwell_path, perr);
            return EXIT_FAILURE;
        }
        mf.close();
    }
    uint64_t n_level = 0, sum_level = 0, sum_stdv = 0; uint32_t min_dwell = 0xffffffffu;
    for (uint64_t s = 0; s < n_slots; s++) {
        if (!dwells[s]) dwells[s] = (uint32_t)dwell_mean;
        stdvs[s] = ideal ? 0u : (uint32_t)(((uint64_t)stdvs[s] * noise_q8 + 128) >> 8);
        if (stdvs[s] >= PG_SIM_MAX_LEVEL) return die("[simulate] --noise_scale takes a level_stdv to 262.144 pA or beyond");
        if (!levels[s]) continue;
        n_level++; sum_level += levels[s]; sum_stdv += stdvs[s];
        const uint32_t w = dwells[s] * (uint32_t)spread / 100u, lo = dwells[s] > w + 1 ? dwells[s] - w : 1u;
        if (lo < min_dwell) min_dwell = lo;
    }
    if (sam_path && min_dwell < (uint32_t)stride) {
        fprintf(stderr, "[simulate] --moves: the smallest possible dwell is %u samples, below the stride of %lld: the rounded boundaries would not stay apart (raise --dwell_mean, lower --dwell_spread or --stride)\n",
                min_dwell, stride);
        return EXIT_FAILURE;
    }
    std::vector<Contig> contigs; std::string err;
    if (!read_fasta(ref_path, contigs, err)) return die("[simulate] %s", err);
    std::vector<uint64_t> c_off(contigs.size() + 1, 0);
    for (size_t i = 0; i < contigs.size(); i++) c_off[i + 1] = c_off[i] + contigs[i].seq.size();
    const uint64_t total = c_off.back();
    if (!total) return die("[simulate] %s holds no base", ref_path);

    pg_sim_params prm; memset(&prm, 0, sizeof prm);
    prm.struct_size = sizeof prm; prm.kmer_size = k; prm.sig_move_offset = (uint32_t)m; prm.rna = rna; prm.seed = seed; prm.range_e4 = range_e4; prm.digitisation = (uint32_t)digitisation;
    prm.offset = (int32_t)offset; prm.off_spread = (uint32_t)off_spread; prm.spread_pct = (uint32_t)spread; prm.lead = (uint32_t)lead;
    prm.lead_level = n_level ? (uint32_t)((2 * sum_level + n_level) / (2 * n_level)) : 0u;   // the rounded means of the model's columns
    prm.lead_stdv = n_level ? (uint32_t)((2 * sum_stdv + n_level) / (2 * n_level)) : 0u;

    pgh::Slow5Writer s5;
    if (!s5.open(out_path, blow5, 4000.0, rec_press, sig_press, (unsigned)threads, err)) return die("%s", err);
    FILE *paf = nullptr, *fq = nullptr, *sam = nullptr;
    auto close_all = [&]() { bool ok = true; for (FILE **f : {&paf, &fq, &sam}) if (*f) { ok = (fclose(*f) == 0) && ok; *f = nullptr; } return ok; };
    for (auto pf : {std::make_pair(paf_path, &paf), std::make_pair(fq_path, &fq), std::make_pair(sam_path, &sam)})
        if (pf.first && !(*pf.second = fopen(pf.first, "w"))) { close_all(); return die("Could not open %s for writing.", pf.first); }

    pg_sim *sim = nullptr;
    if (pg_sim_create(&prm, (int32_t)device, &sim) != PG_OK) { fprintf(stderr, "[simulate] %s\n", pg_sim_last_error(nullptr)); close_all(); return EXIT_FAILURE; }
    int status = EXIT_SUCCESS;
    if (pg_sim_set_model(sim, levels.data(), stdvs.data(), dwells.data(), k) != PG_OK) { fprintf(stderr, "[simulate] %s\n", pg_sim_last_error(sim)); status = EXIT_FAILURE; }
    pg_sigenc *enc = nullptr;
    if (svb && status == EXIT_SUCCESS && pg_sigenc_create((int32_t)device, &enc) != PG_OK) { fprintf(stderr, "[simulate] %s\n", pg_sigenc_last_error(nullptr)); status = EXIT_FAILURE; }

    const uint64_t want = full ? contigs.size() : (uint64_t)n_reads;
    uint64_t written = 0, refused[4] = {0, 0, 0, 0}, samples = 0, bases = 0, sig_copied = 0;
    std::vector<uint8_t> blocks; const uint64_t *block_off = nullptr;
    std::vector<uint8_t> seq; std::vector<uint64_t> seq_off; std::vector<int16_t> sig; std::vector<uint32_t> ops; std::vector<uint64_t> sig_off, op_off; std::vector<double> offs;
    std::string line;
    for (uint64_t first = 0; first < want && status == EXIT_SUCCESS;) {
        // ---- the reads of the batch: at most batch_reads of them and 2^26 bases
        seq.clear(); seq_off.assign(1, 0);
        uint64_t r = first;
        for (; r < want && r - first < (uint64_t)batch_reads && seq.size() < (1u << 26); r++) {
            if (full) { const std::string &s = contigs[r].seq; seq.insert(seq.end(), s.begin(), s.end()); }
            else {
                const PgSimPick p = pg_sim_pick(seed, r, total, (uint32_t)read_len, rna);
                size_t ci = 0;
                while (c_off[ci + 1] <= p.pos) ci++;                       // (few contigs; p.pos < total)
                const std::string &s = contigs[ci].seq;
                const uint64_t at = p.pos - c_off[ci], len = std::min<uint64_t>(p.len, s.size() - at);
                if (!p.reverse) seq.insert(seq.end(), s.begin() + at, s.begin() + at + len);
                else for (uint64_t i = 0; i < len; i++) seq.push_back((uint8_t)complement(s[at + len - 1 - i]));
            }
            seq_off.push_back(seq.size());
        }
        const uint64_t n = r - first;
        pg_sim_batch b; memset(&b, 0, sizeof b);
        b.struct_size = sizeof b; b.location = PG_LOC_HOST; b.n_reads = (uint32_t)n; b.first_read = first; b.seq = seq.data(); b.seq_off = seq_off.data();
        pg_sim_result res; memset(&res, 0, sizeof res); res.struct_size = sizeof res;
        pg_status st = pg_sim_generate(sim, &b, &res);
        if (st == PG_ERR_UNSUPPORTED && batch_reads > 1) { batch_reads = (batch_reads + 1) / 2; continue; } // too many samples at once: the same reads in smaller batches
        if (st != PG_OK) { fprintf(stderr, "[simulate] %s\n", pg_sim_last_error(sim)); status = EXIT_FAILURE; break; }
        ops.resize(res.n_ops); sig_off.resize(n + 1); op_off.resize(n + 1); offs.resize(n);
        auto hip_ok = [&](hipError_t e) { return HipOk{"simulate", &status}(e, "hipMemcpy"); };
        if ((res.n_ops && !hip_ok(hipMemcpy(ops.data(), res.op_n, res.n_ops * 4, hipMemcpyDeviceToHost))) ||
            !hip_ok(hipMemcpy(sig_off.data(), res.sig_off, (n + 1) * 8, hipMemcpyDeviceToHost)) || !hip_ok(hipMemcpy(op_off.data(), res.op_off, (n + 1) * 8, hipMemcpyDeviceToHost)) ||
            (n && !hip_ok(hipMemcpy(offs.data(), res.offset, n * 8, hipMemcpyDeviceToHost))))
            break;
        if (svb) {
            // the samples stay where the simulator left them: their blocks are encoded there, and the blocks are what crosses to the host
            pg_sigenc_result er; memset(&er, 0, sizeof er); er.struct_size = sizeof er;
            if (pg_sigenc_encode(enc, res.sig, sig_off.data(), n, PG_LOC_DEVICE, &er) != PG_OK) { fprintf(stderr, "[simulate] %s\n", pg_sigenc_last_error(enc)); status = EXIT_FAILURE; break; }
            blocks.resize(er.n_block_bytes); block_off = er.block_off;
            if (er.n_block_bytes && !hip_ok(hipMemcpy(blocks.data(), er.blocks, er.n_block_bytes, hipMemcpyDeviceToHost))) break;
            sig_copied += er.n_block_bytes;
        } else {
            sig.resize(res.n_samples);
            if (res.n_samples && !hip_ok(hipMemcpy(sig.data(), res.sig, res.n_samples * 2, hipMemcpyDeviceToHost))) break;
            sig_copied += res.n_samples * 2;
        }
        for (uint64_t i = 0; i < n && status == EXIT_SUCCESS; i++) {
            const uint32_t rs = res.status_host[i];
            if (rs != PG_SIM_ST_OK) { refused[rs < 4 ? rs : 0]++; continue; }
            const std::string id = full ? contigs[first + i].name : "sim_" + std::to_string(first + i);
            const uint64_t ns = sig_off[i + 1] - sig_off[i], lb = op_off[i + 1] - op_off[i];
            const uint32_t *o = ops.data() + op_off[i];
            const char *bases_p = (const char *)seq.data() + seq_off[i];
            const double range = (double)range_e4 / 10000.0;
            if (!(svb ? s5.add_block(id, (double)digitisation, offs[i], range, blocks.data() + block_off[i], block_off[i + 1] - block_off[i], err)
                      : s5.add(id, (double)digitisation, offs[i], range, sig.data() + sig_off[i], ns, err))) { status = die("%s", err); break; }
            if (paf) {
                line = id + "\t" + std::to_string(ns) + "\t" + std::to_string(lead) + "\t" + std::to_string(ns) + "\t+\t" + id + "\t" + std::to_string(lb) + "\t" +
                       std::to_string(rna ? lb : 0) + "\t" + std::to_string(rna ? 0 : lb) + "\t" + std::to_string(lb) + "\t" + std::to_string(lb) + "\t255\tss:Z:";
                for (uint64_t e = 0; e < lb; e++) { line += std::to_string(o[e]); line += ','; }
                line += '\n';
                fwrite(line.data(), 1, line.size(), paf);
            }
            if (fq) { fprintf(fq, "@%s\n", id.c_str()); fwrite(bases_p, 1, lb, fq); fputs("\n+\n", fq); line.assign(lb, '?'); fwrite(line.data(), 1, lb, fq); fputc('\n', fq); }
            if (sam) {
                // the boundaries B_e, rounded: element c_e / stride of the table is a move; the table ends where the signal does
                const uint64_t n_mv = (ns - (uint64_t)lead) / (uint64_t)stride + 1;
                line.assign(n_mv * 2, ',');                               // ",0" per element
                for (uint64_t j = 0; j < n_mv; j++) line[2 * j + 1] = '0';
                uint64_t B = (uint64_t)lead;
                for (uint64_t e = 0; e < lb; B += o[e], e++) line[2 * (pg_sim_round_stride(B, (uint32_t)lead, (uint32_t)stride) / (uint64_t)stride) + 1] = '1';
                fprintf(sam, "%s\t4\t*\t0\t0\t*\t*\t0\t0\t", id.c_str());
                fwrite(bases_p, 1, lb, sam);
                fputc('\t', sam);
                { std::string qual(lb, '?'); fwrite(qual.data(), 1, lb, sam); }
                fprintf(sam, "\tmv:B:c,%lld%s\tts:i:%lld\tns:i:%llu\n", stride, line.c_str(), lead, (unsigned long long)ns);
            }
            written++; samples += ns; bases += lb;
        }
        first = r;
    }
    if (status == EXIT_SUCCESS && !s5.close(err)) status = die("%s", err);
    if (!close_all() && status == EXIT_SUCCESS) status = die("[simulate] error in writing the output files");
    if (status == EXIT_SUCCESS)
        fprintf(stderr, "[simulate] k=%u reads=%llu written=%llu refused=%llu (too_short=%llu bad_base=%llu no_level=%llu) bases=%llu samples=%llu\n", k, (unsigned long long)want,
                (unsigned long long)written, (unsigned long long)(want - written), (unsigned long long)refused[1], (unsigned long long)refused[2], (unsigned long long)refused[3],
                (unsigned long long)bases, (unsigned long long)samples);
    if (status == EXIT_SUCCESS && (svb || rec_press != pgh::Slow5Writer::REC_NONE))
        fprintf(stderr, "[simulate] signal: sig_compress=%s compress=%s threads=%lld signal bytes copied from the device=%llu\n", svb ? "svb-zd" : "none",
                rec_press == pgh::Slow5Writer::REC_ZLIB ? "zlib" : rec_press == pgh::Slow5Writer::REC_ZSTD ? "zstd" : "none", threads, (unsigned long long)sig_copied);
    pg_sigenc_destroy(enc);
    pg_sim_destroy(sim);
    return status;
}
