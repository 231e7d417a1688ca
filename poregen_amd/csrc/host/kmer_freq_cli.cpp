// kmer_freq_cli.cpp -- `poregen kmer_freq`: the reference's command line and output (src/kmer_freq.cpp:70-223) over
// libpgmove's pg_kfreq_* (include/pgmove.h). Host work here: options, reading the FASTQ in pieces (cut at any byte; the
// device finds the lines), merging the dense counts with the other keys in byte order, sorting and printing.
//
// Rules kept from the reference, with its lines:
//   * optstring "v:o:hV" and the long options sort, print_absent_kmers, help, version, output, debug-break (:19-27, :74).
//     --sort takes 0, 1 or 2 and --print_absent_kmers 0 or 1 by atoi (:104-115), else an ERROR and exit 1. --debug-break is
//     accepted and ignored: the reference tests longindex == 4 for it (:116), which is `output`. Unknown options: getopt's
//     message, then ignored. -v sets the log level (:93-95); only the level that silences ERROR (0) changes what is printed.
//   * -V prints "subtool0 0.1.0" at once (:96-98). -h sends the help to stdout and exits 0 after parsing; a positional count
//     other than 2 sends it to stderr and exits 1 (:121-127).
//   * -o is opened (truncated) after those checks, before kmer_size is parsed and the FASTQ is opened (:129-137).
//   * stderr gets "kmer_size: %d" (:139) and "num_kmers: %d" (:153); an unreadable FASTQ "Error in opening file %s" (:159-162).
//   * the keys are the 4^k generated ACGT k-mers at 0 plus every other window met, in std::map order = unsigned byte order
//     (:148-157, :185-192); --sort 1: count ascending then key ascending, --sort 2: count descending then key descending
//     (:194-212); --print_absent_kmers 0 drops zero counts (:215-219); one line "%s\t%" PRIu64 "\n" per key (:220).
// Beyond the reference: a file named *.bam or *.sam (the suffix test of gmove_cli.cpp) is read as the basecaller's BAM / SAM, and its
// reads are counted as the FASTQ that `samtools fastq FILE` would print (flags 0x100 / 0x800 skipped, flag 0x10 reverse-complemented;
// host/kfreq_reads.cpp, pg_kfreq_submit_reads); --n_to_t adds the workflow's `sed '2~4s/N/T/g'` (README.md STEP 2 of the reference) and
// is refused for FASTQ input. A file named *.fa, *.fasta or *.fna, or any file with --fasta, is read as a FASTA (README.md STEP 3 of the
// reference runs the count on one): header lines start with '>', a record's sequence may be wrapped over any number of lines and its
// windows run across the line ends (pg_kfreq_submit_fasta). --fasta on a .bam / .sam is refused. Any other name is FASTQ, as before.
// Refused (exit 1, DESIGN.md "kmer_freq"): kmer_size outside 1..12 (the reference recurses without end for negative values,
// prints one empty key for 0, and needs gigabytes of strings above 12), and a NUL byte in a sequence line (PG_ERR_INPUT).
#include "../../../include/pgmove.h"
#include "pg_kfreq_host.h"

#include <algorithm>
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <getopt.h>
#include <string>
#include <vector>

namespace {

int g_log_level = 3; // LOG_INFO (src/error.h): ERROR prints from level 1

#define KF_ERROR(fmt, ...)                                                                                            \
    do {                                                                                                              \
        if (g_log_level >= 1) fprintf(stderr, "[%s::ERROR]\033[1;31m " fmt "\033[0m At %s:%d\n", "kmer_freq", __VA_ARGS__, __FILE__, __LINE__); \
    } while (0)

const struct option kLongOptions[] = {
    {"sort", required_argument, nullptr, 0},               // 0
    {"print_absent_kmers", required_argument, nullptr, 0}, // 1
    {"help", no_argument, nullptr, 'h'},                   // 2
    {"version", no_argument, nullptr, 'V'},                // 3
    {"output", required_argument, nullptr, 'o'},           // 4
    {"debug-break", required_argument, nullptr, 0},        // 5
    {"n_to_t", no_argument, nullptr, 0},                   // 6 (not in the reference: appended, the indices above keep their meaning)
    {"fasta", no_argument, nullptr, 0},                    // 7 (likewise)
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) { // src/kmer_freq.cpp:30-42
    fprintf(fp, "Usage: poregen kmer_freq kmer_size reads.fastq|reads.bam|reads.sam|seqs.fa|seqs.fasta|seqs.fna\n");
    fprintf(fp, "\nbasic options:\n");
    fprintf(fp, "   --sort INT                 sort based on frequency (0-no sorting, 1-ascend, 2-descend) [0] \n");
    fprintf(fp, "   --print_absent_kmers INT   print kmers with 0 frequency (0-do not print, 1-print) [1] \n");
    fprintf(fp, "   --n_to_t                   count N as T, as sed '2~4s/N/T/g' on the FASTQ would (.bam / .sam input only)\n");
    fprintf(fp, "   --fasta                    read the file as a FASTA, records wrapped or not (implied by .fa / .fasta / .fna)\n");
    fprintf(fp, "   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   --verbose INT              verbosity level [%d]\n", g_log_level);
    fprintf(fp, "   --version                  print version\n");
    fprintf(fp, "\nadvanced options:\n");
    fprintf(fp, "   --debug-break INT          break after processing the specified no. of batches\n");
}

// a key as a number whose order is the byte order of its k bytes (k <= 12: 96 bits)
struct Key {
    uint64_t hi; uint32_t lo;
    bool operator<(const Key &o) const { return hi != o.hi ? hi < o.hi : lo < o.lo; }
    bool operator==(const Key &o) const { return hi == o.hi && lo == o.lo; }
};
Key key_of_bytes(const uint8_t *b, uint32_t k) {
    uint8_t x[12] = {0};
    memcpy(x, b, k);
    Key r{0, 0};
    for (int i = 0; i < 8; i++) r.hi = r.hi << 8 | x[i];
    for (int i = 8; i < 12; i++) r.lo = r.lo << 8 | x[i];
    return r;
}
const char kBase[4] = {'A', 'C', 'G', 'T'};
void bytes_of_code(uint32_t code, uint32_t k, uint8_t *out) {
    for (uint32_t i = 0; i < k; i++) out[i] = (uint8_t)kBase[(code >> (2 * (k - 1 - i))) & 3];
}

struct Entry { uint64_t count; Key key; }; // key bytes recovered from `key`

class Writer {
  public:
    explicit Writer(FILE *f) : f_(f) { buf_.reserve(kCap + 64); }
    ~Writer() { flush(); }
    void line(const Key &key, uint32_t k, uint64_t count) {
        uint8_t b[12];
        for (uint32_t i = 0; i < k; i++) b[i] = i < 8 ? (uint8_t)(key.hi >> (8 * (7 - i))) : (uint8_t)(key.lo >> (8 * (11 - i)));
        buf_.append(reinterpret_cast<const char *>(b), k);
        buf_.push_back('\t');
        char d[24]; int n = 0;
        do { d[n++] = (char)('0' + count % 10); count /= 10; } while (count);
        while (n) buf_.push_back(d[--n]);
        buf_.push_back('\n');
        if (buf_.size() >= kCap) flush();
    }
    void flush() { if (!buf_.empty()) { fwrite(buf_.data(), 1, buf_.size(), f_); buf_.clear(); } }

  private:
    static constexpr size_t kCap = 1 << 20;
    FILE *f_;
    std::string buf_;
};

uint64_t piece_bytes() {
    if (const char *s = getenv("POREGEN_KFREQ_PIECE")) { const long long v = atoll(s); if (v >= 1) return (uint64_t)v; }
    return 64ull << 20;
}

} // namespace

int kmer_freq_main(int argc, char **argv) {
    int c, longindex = 0;
    int flag_sort = 0, flag_print_absent = 1;
    bool n_to_t = false, fasta = false;
    bool help_to_stdout = false;
    const char *out_path = nullptr;
    optind = 1;
    while ((c = getopt_long(argc, argv, "v:o:hV", kLongOptions, &longindex)) >= 0) {
        if (c == 'v') g_log_level = atoi(optarg);
        else if (c == 'V') { fprintf(stdout, "subtool0 %s\n", "0.1.0"); exit(EXIT_SUCCESS); }
        else if (c == 'h') help_to_stdout = true;
        else if (c == 'o') out_path = optarg;
        else if (c == 0 && longindex == 0) {
            const int v = atoi(optarg);
            if (v != 0 && v != 1 && v != 2) { KF_ERROR("sort argument must be 0,1 or 2 You entered %d", v); exit(EXIT_FAILURE); }
            flag_sort = v;
        } else if (c == 0 && longindex == 1) {
            const int v = atoi(optarg);
            if (v != 0 && v != 1) { KF_ERROR("print_absent_kmers flag must be 0 or 1 You entered %d", v); exit(EXIT_FAILURE); }
            flag_print_absent = v;
        } else if (c == 0 && longindex == 6) n_to_t = true;
        else if (c == 0 && longindex == 7) fasta = true;
        // longindex 5 (debug-break): accepted, no effect (the reference reads it at longindex 4)
    }
    if (argc - optind != 2 || help_to_stdout) {
        print_help(help_to_stdout ? stdout : stderr);
        exit(help_to_stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    const std::string in_name(argv[optind + 1]);
    const std::string ext = in_name.size() >= 4 ? in_name.substr(in_name.size() - 4) : "";
    const bool is_bam = ext == ".bam", is_reads = is_bam || ext == ".sam";
    auto ends_with = [&](const char *suffix) { const size_t m = strlen(suffix); return in_name.size() >= m && in_name.compare(in_name.size() - m, m, suffix) == 0; };
    if (fasta && is_reads) {
        KF_ERROR("--fasta does not apply to .bam and .sam input You entered %s", in_name.c_str());
        exit(EXIT_FAILURE);
    }
    if (ends_with(".fa") || ends_with(".fasta") || ends_with(".fna")) fasta = true;
    if (n_to_t && !is_reads) {
        KF_ERROR("--n_to_t applies to .bam and .sam input only (for a FASTQ: sed '2~4s/N/T/g') You entered %s", in_name.c_str());
        exit(EXIT_FAILURE);
    }
    FILE *out = stdout;
    if (out_path) {
        out = fopen(out_path, "w");
        if (!out) { KF_ERROR("Could not to open file %s: %s", out_path, strerror(errno)); exit(EXIT_FAILURE); }
    }
    const int k_arg = atoi(argv[optind++]);
    const char *fastq = argv[optind];
    fprintf(stderr, "kmer_size: %d\n", k_arg);
    if (k_arg < 1 || k_arg > 12) {
        KF_ERROR("kmer_size must be between 1 and 12 You entered %d", k_arg);
        exit(EXIT_FAILURE);
    }
    const uint32_t k = (uint32_t)k_arg;
    const uint32_t n_codes = 1u << (2 * k);
    fprintf(stderr, "num_kmers: %d\n", (int)n_codes);

    FILE *in = fopen(fastq, "r");
    if (!in) { fprintf(stderr, "Error in opening file %s\n", fastq); exit(EXIT_FAILURE); }
    pgh::PackedReads reads;
    if (is_reads) {
        fclose(in);
        std::string err;
        if (!reads.open(fastq, is_bam, err)) { KF_ERROR("%s: %s", fastq, err.c_str()); exit(EXIT_FAILURE); }
    }

    pg_kfreq *h = nullptr;
    if (pg_kfreq_create(k, 0, &h) != PG_OK) {
        KF_ERROR("%s", pg_kfreq_last_error(nullptr));
        exit(EXIT_FAILURE);
    }
    const uint64_t piece = piece_bytes();
    if (is_reads) {
        // a batch is on the device's side when submit_reads returns: the next one is inflated and parsed while it is counted
        pgh::PackedBatch b;
        std::string err;
        int rc;
        while ((rc = reads.next(b, piece, err)) == 1) {
            if (pg_kfreq_submit_reads(h, b.seq.data(), b.seq.size(), b.off.data(), b.len.data(), b.rev.data(), b.len.size(),
                                      n_to_t ? PG_KFREQ_N_TO_T : 0, PG_LOC_HOST) != PG_OK) { KF_ERROR("%s", pg_kfreq_last_error(h)); exit(EXIT_FAILURE); }
        }
        if (rc < 0) { KF_ERROR("%s: %s", fastq, err.c_str()); exit(EXIT_FAILURE); }
    } else {
        std::vector<uint8_t> buf(piece);
        for (;;) {
            const size_t got = fread(buf.data(), 1, piece, in);
            if (got && (fasta ? pg_kfreq_submit_fasta : pg_kfreq_submit)(h, buf.data(), got, PG_LOC_HOST) != PG_OK) { KF_ERROR("%s", pg_kfreq_last_error(h)); exit(EXIT_FAILURE); }
            if (got < piece) break;
        }
        if (ferror(in)) { KF_ERROR("reading %s: %s", fastq, strerror(errno)); exit(EXIT_FAILURE); }
        fclose(in);
    }
    std::vector<uint64_t> counts(n_codes);
    pg_kfreq_result r;
    if (pg_kfreq_finish(h, counts.data(), &r) != PG_OK) { KF_ERROR("%s: %s", fastq, pg_kfreq_last_error(h)); exit(EXIT_FAILURE); }

    // dense keys (code order = byte order over A<C<G<T) merged with the other keys (already in byte order)
    std::vector<Entry> all;
    all.reserve(n_codes + r.n_odd);
    {
        uint64_t j = 0;
        uint8_t kb[12];
        for (uint32_t code = 0; code < n_codes; code++) {
            bytes_of_code(code, k, kb);
            const Key dk = key_of_bytes(kb, k);
            for (; j < r.n_odd; j++) {
                const Key ok = key_of_bytes(r.odd_keys + j * k, k);
                if (!(ok < dk)) break;
                all.push_back({r.odd_counts[j], ok});
            }
            all.push_back({counts[code], dk});
        }
        for (; j < r.n_odd; j++) all.push_back({r.odd_counts[j], key_of_bytes(r.odd_keys + j * k, k)});
    }
    if (flag_sort == 1)
        std::sort(all.begin(), all.end(), [](const Entry &a, const Entry &b) { return a.count != b.count ? a.count < b.count : a.key < b.key; });
    else if (flag_sort == 2)
        std::sort(all.begin(), all.end(), [](const Entry &a, const Entry &b) { return a.count != b.count ? a.count > b.count : b.key < a.key; });
    {
        Writer w(out);
        for (const Entry &e : all)
            if (flag_print_absent || e.count) w.line(e.key, k, e.count);
    }
    pg_kfreq_destroy(h);
    if (out_path) fclose(out);
    else fflush(out);
    return 0;
}
