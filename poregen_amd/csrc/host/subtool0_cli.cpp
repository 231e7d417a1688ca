// subtool0_cli.cpp -- `poregen subtool0` (src/subtool0.c, src/poregen.cpp:24-180 of the reference) and `poregen pa_stats`, over
// libpgmove's pg_pamean_* (include/pgmove.h). Host work here: options, the file-order record walk, decoding records on a thread pool
// while the device works on the batch before, and printing. Records with svb-zd signals are only inflated here: their signal blocks go
// to the device as they lie in the record and are decoded there (pg_pamean_submit_svb).
//
// Rules kept from the reference, with its lines (src/subtool0.c):
//   * optstring "t:B:K:v:o:hV" and the long options threads, batchsize, max-bytes, verbose, help, version, output, debug-break (:16-25,
//     :72). -B is mm_parse_num (src/misc.h:67-79: K/M/G suffixes), -K and -t atoi; a value of 0 or below is an ERROR and exit 1
//     (:91-108). They size the reference's batches and threads; here they are checked and never change the output (the device batches
//     by bytes, the pool is min(-t, 16) threads). -o is accepted and ignored (the loop has no 'o' branch), and so is --debug-break
//     (checked against longindex 15, :120). Unknown options: getopt's message, then ignored.
//   * -V prints "subtool0 0.1.0" at once (:116-118). -h sends the help to stdout and exits 0 after parsing; a positional count other
//     than 1 sends it to stderr and exits 1 (:126-133). A file that cannot be opened exits 1 (src/poregen.cpp:29-33).
//   * records in FILE order, without the read-id index (slow5_get_next_bytes, src/poregen.cpp:99): every record of a file with
//     duplicate ids is printed. One line "%s\t%f\n" (read id, mean) per record with at least one sample (src/poregen.cpp:166-175).
// pa_stats: the same walk, then one line "MEAN\tSSTDEV" of all pA values, "%.14g" as datamash prints by default (the numbers STEP 7 of
// scripts/poregen.sh takes from `sigtk pa | datamash mean 1 sstdev 1`); fewer than 2 samples in the file is an error (exit 1).
#include "../../../include/pgmove.h"
#include "pg_host.h"

#include <hip/hip_runtime_api.h>
#include "../pg_hip_host.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <getopt.h>
#include <string>
#include <sys/time.h>
#include <thread>
#include <vector>

namespace {

int g_log_level = 3; // LOG_INFO (src/error.h): ERROR prints from level 1

#define S0_ERROR(tool, fmt, ...)                                                                                        \
    do {                                                                                                                \
        if (g_log_level >= 1) fprintf(stderr, "[%s::ERROR]\033[1;31m " fmt "\033[0m At %s:%d\n", tool, __VA_ARGS__, __FILE__, __LINE__); \
    } while (0)

const struct option kLongOptions[] = {
    {"threads", required_argument, nullptr, 't'},   // 0
    {"batchsize", required_argument, nullptr, 'K'}, // 1
    {"max-bytes", required_argument, nullptr, 'B'}, // 2
    {"verbose", required_argument, nullptr, 'v'},   // 3
    {"help", no_argument, nullptr, 'h'},            // 4
    {"version", no_argument, nullptr, 'V'},         // 5
    {"output", required_argument, nullptr, 'o'},    // 6
    {"debug-break", required_argument, nullptr, 0}, // 7
    {nullptr, 0, nullptr, 0}};

struct Opts { int32_t batch_size = 512; int64_t batch_bytes = 20 * 1000 * 1000; int32_t threads = 8; };

void print_help(FILE *fp, const char *cmd, const Opts &o) { // src/subtool0.c:28-44
    fprintf(fp, "Usage: poregen %s reads.blow5\n", cmd);
    fprintf(fp, "\nbasic options:\n");
    fprintf(fp, "   -t INT                     number of processing threads [%d]\n", o.threads);
    fprintf(fp, "   -K INT                     batch size (max number of reads loaded at once) [%d]\n", o.batch_size);
    fprintf(fp, "   -B FLOAT[K/M/G]            max number of bytes loaded at once [%.1fM]\n", o.batch_bytes / (float)(1000 * 1000));
    fprintf(fp, "   -h                         help\n");
    fprintf(fp, "   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   --verbose INT              verbosity level [%d]\n", g_log_level);
    fprintf(fp, "   --version                  print version\n");
    fprintf(fp, "\nadvanced options:\n");
    fprintf(fp, "   --debug-break INT          break after processing the specified no. of batches\n");
}

int64_t mm_parse_num(const char *str) { // src/misc.h:67-79
    char *p;
    double x = strtod(str, &p);
    if (*p == 'G' || *p == 'g') x *= 1e9;
    else if (*p == 'M' || *p == 'm') x *= 1e6;
    else if (*p == 'K' || *p == 'k') x *= 1e3;
    return (int64_t)(x + .499);
}

double now() { struct timeval tp; gettimeofday(&tp, nullptr); return tp.tv_sec + tp.tv_usec * 1e-6; }

uint64_t batch_bytes_from_env() { // record bytes per device batch
    if (const char *s = getenv("POREGEN_PAMEAN_BATCH_BYTES")) { const long long v = atoll(s); if (v >= 1) return (uint64_t)v; }
    return 64ull << 20;
}

// one batch of records, decoded: the layout pg_pamean_batch takes
struct HostBatch {
    size_t n = 0;
    std::vector<std::string> ids;
    std::vector<uint64_t> off;            // n + 1
    std::vector<double> dig, offs, rng, means;
    PgPinned<int16_t> sig; // the decoded samples are written here once and go to the device by DMA from here
    // svb-zd files: the signal blocks back to back instead, and where each lies (off: the samples they will decode to)
    bool svb = false;
    PgPinned<unsigned char> blocks;
    std::vector<uint64_t> block_off;      // n + 1
};

class Walker {
  public:
    Walker(const pgh::Slow5File &f, unsigned n_threads) : f_(f), nt_(n_threads) {}
    // decodes records [first, first + n) into b; false (err) when one of them cannot be decoded
    bool fill(HostBatch &b, size_t first, size_t n, std::string &err) {
        if (f_.has_svb_views()) return fill_svb(b, first, n, err);
        b.n = n;
        b.ids.assign(n, std::string()); b.off.assign(n + 1, 0);
        b.dig.resize(n); b.offs.resize(n); b.rng.resize(n); b.means.assign(n, 0.0);
        const bool view = f_.has_raw_views();
        std::vector<pgh::Slow5File::RawView> views(view ? n : 0);
        std::vector<pgh::Slow5Rec> recs(view ? 0 : n);
        std::vector<std::string> errs(n);
        std::atomic<bool> bad{false};
        on_threads(n, [&](size_t i) {
            bool ok;
            if (view) {
                ok = f_.record_view(first + i, b.ids[i], views[i], errs[i]);
                if (ok) { b.off[i + 1] = views[i].n; b.dig[i] = views[i].digitisation; b.offs[i] = views[i].offset; b.rng[i] = views[i].range; }
            } else {
                ok = f_.record(first + i, b.ids[i], recs[i], errs[i]);
                if (ok) { b.off[i + 1] = recs[i].raw.size(); b.dig[i] = recs[i].digitisation; b.offs[i] = recs[i].offset; b.rng[i] = recs[i].range; }
            }
            if (!ok) bad = true;
        });
        if (bad) {
            for (size_t i = 0; i < n; i++) if (!errs[i].empty()) { err = "record " + std::to_string(first + i) + ": " + errs[i]; return false; }
        }
        for (size_t i = 0; i < n; i++) b.off[i + 1] += b.off[i];
        const size_t want = std::max<uint64_t>(b.off[n], 1) * sizeof(int16_t);
        if (b.sig.ensure(want, want + want / 4) != hipSuccess) { // (batches differ in size: a little room saves re-pinning)
            err = "cannot allocate page-locked memory for the samples";
            return false;
        }
        int16_t *dst = b.sig.p;
        on_threads(n, [&](size_t i) { // the samples copied once, from the mapping (or the decoder) to page-locked memory
            const uint64_t len = b.off[i + 1] - b.off[i];
            if (!len) return;
            if (view) memcpy(dst + b.off[i], views[i].samples, len * sizeof(int16_t));
            else { memcpy(dst + b.off[i], recs[i].raw.data(), len * sizeof(int16_t)); std::vector<int16_t>().swap(recs[i].raw); }
        });
        return true;
    }

    // svb-zd: the headers of records [first, first + n) parsed, their blocks copied to b.blocks. Uncompressed records: the blocks are
    // located first and copied once, from the mapping. zlib / zstd records: every thread inflates its run of records through one
    // buffer and keeps the blocks, back to back, in a buffer of its own that lasts from batch to batch; the runs are then copied to
    // their places. (Keeping every inflated record until the offsets are known cost more in fresh pages than the host decoder took.)
    bool fill_svb(HostBatch &b, size_t first, size_t n, std::string &err) {
        b.n = n; b.svb = true;
        b.ids.assign(n, std::string()); b.off.assign(n + 1, 0); b.block_off.assign(n + 1, 0);
        b.dig.resize(n); b.offs.resize(n); b.rng.resize(n); b.means.assign(n, 0.0);
        const bool packed = f_.records_compressed();
        std::vector<pgh::Slow5File::SvbView> views(packed ? 0 : n);
        std::vector<std::string> errs(n);
        std::atomic<bool> bad{false};
        if (runs_.size() < nt_) runs_.resize(nt_);
        on_runs(n, [&](unsigned t, size_t lo, size_t hi) {
            std::vector<unsigned char> body;
            if (packed) runs_[t].clear();
            for (size_t i = lo; i < hi; i++) {
                pgh::Slow5File::SvbView one;
                pgh::Slow5File::SvbView &v = packed ? one : views[i];
                if (!f_.record_svb(first + i, b.ids[i], v, body, errs[i])) { bad = true; continue; }
                b.off[i + 1] = v.count; b.block_off[i + 1] = v.len;
                b.dig[i] = v.digitisation; b.offs[i] = v.offset; b.rng[i] = v.range;
                if (packed) runs_[t].insert(runs_[t].end(), v.block, v.block + v.len);
            }
        });
        if (bad) {
            for (size_t i = 0; i < n; i++) {
                if (errs[i].empty()) { // a block in front of the first refused record may be one the device would refuse: the first error of the batch is reported
                    pgh::Slow5Rec rec;
                    std::string id;
                    if (f_.record(first + i, id, rec, errs[i])) continue;
                }
                err = "record " + std::to_string(first + i) + ": " + errs[i];
                return false;
            }
        }
        for (size_t i = 0; i < n; i++) { b.off[i + 1] += b.off[i]; b.block_off[i + 1] += b.block_off[i]; }
        const size_t want = std::max<uint64_t>(b.block_off[n], 1);
        if (b.blocks.ensure(want, want + want / 4) != hipSuccess) {
            err = "cannot allocate page-locked memory for the samples";
            return false;
        }
        unsigned char *dst = b.blocks.p;
        on_runs(n, [&](unsigned t, size_t lo, size_t hi) {
            if (packed) { if (!runs_[t].empty()) memcpy(dst + b.block_off[lo], runs_[t].data(), runs_[t].size()); return; }
            for (size_t i = lo; i < hi; i++) memcpy(dst + b.block_off[i], views[i].block, views[i].len);
        });
        return true;
    }

  private:
    // every thread takes a contiguous run of the n items
    void on_runs(size_t n, const std::function<void(unsigned, size_t, size_t)> &fn) {
        const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt_, n / 64 + 1));
        if (nt == 1) { fn(0, 0, n); return; }
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; t++) pool.emplace_back([&, t] { fn(t, n * t / nt, n * (t + 1) / nt); });
        for (auto &th : pool) th.join();
    }
    void on_threads(size_t n, const std::function<void(size_t)> &fn) {
        on_runs(n, [&](unsigned, size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) fn(i); });
    }
    std::vector<std::vector<unsigned char>> runs_; // fill_svb: the blocks of each thread's run
    const pgh::Slow5File &f_;
    unsigned nt_;
};

// pa_stats' two numbers as it prints them ("%.14g"): `poregen transform --signal` takes the texts from the same walk
struct StatsTexts { bool print; std::string mean, sstdev; };

// The walk of one file: every record in file order, batch by batch through pg_pamean_*. stats == nullptr: subtool0's line per record;
// otherwise the dataset's mean and sstdev. Every error is the tool's ERROR line and exit 1.
void walk(const char *tool, const char *path, const Opts &opt, StatsTexts *stats) {
    const double t0 = now();
    pgh::Slow5File f;
    std::string err;
    if (!f.open_walk(path, err)) { S0_ERROR(tool, "Error opening SLOW5 file %s: %s", path, err.c_str()); exit(EXIT_FAILURE); }
    pg_pamean *h = nullptr;
    if (pg_pamean_create(0, &h) != PG_OK) { S0_ERROR(tool, "%s", pg_pamean_last_error(nullptr)); exit(EXIT_FAILURE); }
    unsigned nt = std::thread::hardware_concurrency();
    nt = std::max(1u, std::min({nt ? nt : 1u, 16u, (unsigned)opt.threads}));
    Walker w(f, nt);

    // device batches by record bytes (a record's bytes bound its samples' bytes within the compression ratio)
    const uint64_t want = batch_bytes_from_env();
    std::vector<size_t> cuts{0};
    {
        uint64_t acc = 0;
        for (size_t i = 0; i < f.n_records(); i++) {
            acc += f.record_bytes(i);
            if (acc >= want || i + 1 - cuts.back() >= (1u << 20)) { cuts.push_back(i + 1); acc = 0; }
        }
        if (cuts.back() != f.n_records()) cuts.push_back(f.n_records());
    }
    const size_t n_batches = cuts.size() - 1;
    HostBatch hb[2];
    double t_decode = 0, t_wait = 0;
    auto parse_error = [&]() { S0_ERROR(tool, "Error parsing the record: %s", err.c_str()); exit(EXIT_FAILURE); };
    auto fill = [&](size_t k) {
        const double a = now();
        if (!w.fill(hb[k & 1], cuts[k], cuts[k + 1] - cuts[k], err)) parse_error();
        t_decode += now() - a;
    };
    auto submit = [&](size_t k) {
        HostBatch &b = hb[k & 1];
        pg_status st;
        if (b.svb) {
            pg_svb_batch sb{};
            sb.n_reads = b.n; sb.location = PG_LOC_HOST;
            sb.blocks = b.blocks.p; sb.n_block_bytes = b.block_off[b.n]; sb.block_off = b.block_off.data();
            st = pg_pamean_submit_svb(h, &sb, b.dig.data(), b.offs.data(), b.rng.data(), b.means.data());
            unsigned long long r = 0;
            if (st == PG_ERR_INPUT && sscanf(pg_pamean_last_error(h), "pg_pamean_submit_svb: read %llu: corrupt streamvbyte block", &r) == 1) {
                err = "record " + std::to_string(cuts[k] + r) + ": corrupt streamvbyte block"; // a block only the device can refuse: the host decoder's words
                parse_error();
            }
        } else {
            pg_pamean_batch pb{};
            pb.n_reads = b.n; pb.location = PG_LOC_HOST;
            pb.sig = b.sig.p; pb.sig_off = b.off.data();
            pb.digitisation = b.dig.data(); pb.offset = b.offs.data(); pb.range = b.rng.data();
            st = pg_pamean_submit(h, &pb, b.means.data());
        }
        if (st != PG_OK) { S0_ERROR(tool, "%s", pg_pamean_last_error(h)); exit(EXIT_FAILURE); }
    };
    // Batch k + 1 is decoded while the device works on batch k. A batch of svb-zd blocks is submitted before batch k is printed: a record
    // that cannot be decoded ends the run with the batch before its own unprinted, whether the host refuses it (fill) or the device (submit).
    std::string out;
    if (n_batches) { fill(0); submit(0); }
    for (size_t k = 0; k < n_batches; k++) {
        HostBatch &b = hb[k & 1];
        const bool more = k + 1 < n_batches;
        if (more) fill(k + 1);
        const double a = now();
        if (pg_pamean_sync(h) != PG_OK) { S0_ERROR(tool, "%s", pg_pamean_last_error(h)); exit(EXIT_FAILURE); }
        t_wait += now() - a;
        const bool early = more && hb[(k + 1) & 1].svb;
        if (early) submit(k + 1);
        if (!stats) {
            out.clear();
            char num[512];
            for (size_t i = 0; i < b.n; i++) {
                if (b.off[i + 1] == b.off[i]) continue;
                const int len = snprintf(num, sizeof num, "%f", b.means[i]);
                out += b.ids[i]; out += '\t'; out.append(num, (size_t)len); out += '\n';
            }
            fwrite(out.data(), 1, out.size(), stdout);
        }
        if (more && !early) submit(k + 1);
    }
    pg_pamean_result r;
    if (pg_pamean_finish(h, &r) != PG_OK) { S0_ERROR(tool, "%s", pg_pamean_last_error(h)); exit(EXIT_FAILURE); }
    const unsigned long long on_device = pg_pamean_svb_samples(h);
    pg_pamean_destroy(h);
    if (stats) {
        if (r.n_samples < 2) { S0_ERROR(tool, "%s holds %llu pA values: the sample standard deviation needs at least 2", path, (unsigned long long)r.n_samples); exit(EXIT_FAILURE); }
        char t[64];
        snprintf(t, sizeof t, "%.14g", r.mean); stats->mean = t;
        snprintf(t, sizeof t, "%.14g", r.sstdev); stats->sstdev = t;
        if (stats->print) fprintf(stdout, "%s\t%s\n", stats->mean.c_str(), stats->sstdev.c_str());
    }
    fflush(stdout);
    fprintf(stderr, "[%s] %llu records, %llu samples, %llu finished on the host; host decode %.3f s, waiting for the device %.3f s, total %.3f s\n", tool,
            (unsigned long long)r.n_reads, (unsigned long long)r.n_samples, (unsigned long long)r.n_fallback, t_decode, t_wait, now() - t0);
    if (g_log_level >= 4) fprintf(stderr, "[%s] %llu samples decoded from svb-zd blocks on the device\n", tool, on_device); // (-v 4 and above)
}

int run(const char *tool, int argc, char **argv, bool stats) {
    int c, longindex = 0;
    Opts opt;
    bool help_to_stdout = false;
    optind = 1;
    while ((c = getopt_long(argc, argv, "t:B:K:v:o:hV", kLongOptions, &longindex)) >= 0) {
        if (c == 'B') {
            opt.batch_bytes = mm_parse_num(optarg);
            if (opt.batch_bytes <= 0) { S0_ERROR(tool, "%s", "Maximum number of bytes should be larger than 0."); exit(EXIT_FAILURE); }
        } else if (c == 'K') {
            opt.batch_size = atoi(optarg);
            if (opt.batch_size < 1) { S0_ERROR(tool, "Batch size should larger than 0. You entered %d", opt.batch_size); exit(EXIT_FAILURE); }
        } else if (c == 't') {
            opt.threads = atoi(optarg);
            if (opt.threads < 1) { S0_ERROR(tool, "Number of threads should larger than 0. You entered %d", opt.threads); exit(EXIT_FAILURE); }
        } else if (c == 'v') g_log_level = atoi(optarg);
        else if (c == 'V') { fprintf(stdout, "%s %s\n", tool, "0.1.0"); exit(EXIT_SUCCESS); }
        else if (c == 'h') help_to_stdout = true;
        // 'o' and --debug-break (c == 0, longindex 7): accepted, no effect
    }
    if (argc - optind != 1 || help_to_stdout) {
        print_help(help_to_stdout ? stdout : stderr, tool, opt);
        exit(help_to_stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    StatsTexts st{true, "", ""};
    walk(tool, argv[optind], opt, stats ? &st : nullptr);
    return 0;
}

} // namespace

int subtool0_main(int argc, char **argv) { return run("subtool0", argc, argv, false); }
int pa_stats_main(int argc, char **argv) { return run("pa_stats", argc, argv, true); }
// `poregen transform --signal FILE` (transform_cli.cpp): the two texts `poregen pa_stats FILE` prints, nothing on stdout; exits like pa_stats
void pa_stats_texts(const char *tool, const char *path, std::string &mean, std::string &sstdev) {
    StatsTexts st{false, "", ""};
    walk(tool, path, Opts(), &st);
    mean = st.mean; sstdev = st.sstdev;
}
