// model_cli.cpp -- `poregen model`: STEP 6 of the reference's pipeline (scripts/poregen.sh:54-85 calculate_mean_stddev_all and :33-52
// calculate_dwell_times_medians) as a tool of its own, over libpgmove's pg_dmodel_* (include/pgmove.h). The reference has no such
// command: its script runs `tr | tail | datamash` twice per dump file. Host work here: options, listing and merging the directories
// (pg_dumpdir.h), reading the files of batch i + 1 on -t threads while batch i is on the device, the --stdv_limit cap, printing.
//   * one line per name, NAME<TAB>median<TAB>stddev, to -o (truncated) or stdout          scripts/poregen.sh:66-72
//   * stddev > limit (bc -l on the two texts) prints the limit's text                     scripts/poregen.sh:69-71
//   * --dwell_model FILE: NAME<TAB>median dwell, appended                                 scripts/poregen.sh:43-45
//   * --pool START:LEN: one line per sub-k-mer name[START:START+LEN], SUB<TAB>median<TAB>stddev of that group's files read back to back
//     (pg_pool_*): `cat` of the files | tr | tail | datamash                              scripts/poregen.sh:73-74
//   * --event_model FILE: NAME<TAB>events<TAB>median and sstdev of the events' means<TAB>median and sstdev of the events' standard
//     deviations (pg_dmodel_finish_events; no counterpart in the script, which cannot tell the two apart). A file whose table the library
//     refuses ends the command with status 1 before anything is written
#include "../pg_dumphost.h"
#include "pg_cli.h"
#include "pg_dumpdir.h"
#include "pg_poolnames.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <future>
#include <getopt.h>
#include <string>
#include <vector>

namespace {

const struct option kLongOptions[] = {
    {"stdv_limit", required_argument, nullptr, 0},  // 0
    {"dwell_model", required_argument, nullptr, 0}, // 1
    {"keep_first", no_argument, nullptr, 0},        // 2
    {"output", required_argument, nullptr, 'o'},    // 3
    {"threads", required_argument, nullptr, 't'},   // 4
    {"help", no_argument, nullptr, 'h'},            // 5
    {"pool", required_argument, nullptr, 0},        // 6
    {"event_model", required_argument, nullptr, 0}, // 7
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen model [options] DUMP_DIR [DUMP_DIR ...]\n");
    fprintf(fp, "\nKMER<TAB>median<TAB>stddev of every dump file, computed on the GPU; files of one name in several directories count as one file\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   --stdv_limit NUM           cap of the stddev column [3.1]\n");
    fprintf(fp, "   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   --dwell_model FILE         also append KMER<TAB>median dwell to FILE (scripts/poregen.sh calculate_dwell_times_medians)\n");
    fprintf(fp, "   --event_model FILE         also write KMER<TAB>n_events<TAB>mean_median<TAB>mean_sstdev<TAB>sd_median<TAB>sd_sstdev: per file the median and\n");
    fprintf(fp, "                              sstdev of its events' means and of its events' standard deviations (an event: the values up to a ';')\n");
    fprintf(fp, "   --keep_first               keep the first value of every file (the pipeline's `tail -n +2` drops it)\n");
    fprintf(fp, "   --pool START:LEN           pool the files by the LEN bases of their names from 0-based START: SUB<TAB>median<TAB>stddev of each group's files read as one\n");
    fprintf(fp, "   -t INT                     threads that read files [8], at most 16\n");
    fprintf(fp, "   -h                         help\n");
}

uint64_t batch_bytes() {
    if (const char *s = getenv("POREGEN_MODEL_BATCH")) { const long long v = atoll(s); if (v >= 1) return (uint64_t)v; }
    return 64ull << 20;
}

struct Batch { size_t first = 0, n = 0; std::vector<uint8_t> bytes; std::vector<uint64_t> file_off; std::string err; bool ok = true; double secs = 0; };

// --pool START:LEN: the files grouped by name[START:START+LEN], every group's files in name order read as one file
int pool_main(const std::vector<std::string> &dirs, const char *spec, const char *stdv_limit, const char *out_path, bool keep_first, int n_threads) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    char *end = nullptr;
    const long long start = strtoll(spec, &end, 10);
    if (end == spec || *end != ':' || start < 0) return die("--pool takes START:LEN with START >= 0. You entered %s", spec);
    const char *lp = end + 1;
    const long long len = strtoll(lp, &end, 10);
    if (end == lp || *end || len < 1) return die("--pool takes START:LEN with LEN >= 1. You entered %s", spec);
    const clk::time_point t_start = clk::now();
    pgh::DumpSet ds;
    std::string err;
    if (!pgh::list_dump_dirs(dirs, n_threads, ds, err)) return die("%s", err);
    pgh::PoolNames pn;
    if (!pgh::check_pool_names(ds.names, pn, err)) return die("[model] --pool: %s", err);
    if ((unsigned long long)start + (unsigned long long)len > pn.k) return die(("[model] --pool %s does not lie inside names of length " + std::to_string(pn.k)).c_str(), spec);
    const double t_list = secs(t_start, clk::now());
    // the names are sorted, so are the sub-k-mers of one START when taken in a sorted set
    std::vector<std::string> subs;
    for (const std::string &n : ds.names) subs.push_back(n.substr((size_t)start, (size_t)len));
    std::vector<std::string> uniq(subs);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<uint32_t> group_of(subs.size());
    for (size_t i = 0; i < subs.size(); i++) group_of[i] = (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), subs[i]) - uniq.begin());
    pg_pool *h = nullptr; pg_pool_result res; pgh::PoolTimes tm;
    if (!pgh::run_pool(ds, n_threads, keep_first, {(uint32_t)uniq.size()}, [&](size_t f, uint32_t *g) { g[0] = group_of[f]; }, &h, res, tm, err)) return die("[model] %s", err);
    uint32_t bad; std::string what;
    if (pgh::pool_refused(ds, h, res, bad, what)) { fprintf(stderr, "[model] group %s is refused: %s\n", uniq[bad].c_str(), what.c_str()); pg_pool_destroy(h); return EXIT_FAILURE; }
    const clk::time_point p0 = clk::now();
    FILE *fp = stdout;
    if (out_path && !(fp = fopen(out_path, "w"))) { pg_pool_destroy(h); return die("Could not open %s for writing.", out_path); }
    char a[64], b[64];
    for (uint32_t g = 0; g < res.n_groups; g++) {
        pg_pool_format(h, g, PG_MODEL_TEXT_MEDIAN, a, sizeof a); pg_pool_format(h, g, PG_MODEL_TEXT_SSTDEV, b, sizeof b);
        fprintf(fp, "%s\t%s\t%s\n", uniq[g].c_str(), a, pg_dump_sd_capped(b, stdv_limit) ? stdv_limit : b);
    }
    if (out_path) fclose(fp); else fflush(fp);
    pgh::pool_summary("model", res, tm, t_list, secs(p0, clk::now()), n_threads);
    pg_pool_destroy(h);
    return EXIT_SUCCESS;
}

} // namespace

int model_main(int argc, char **argv) {
    using clk = std::chrono::steady_clock;
    const char *stdv_limit = "3.1", *out_path = nullptr, *dwell_path = nullptr, *pool = nullptr, *event_path = nullptr;
    bool keep_first = false, help = false;
    int n_threads = 8;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:t:h", kLongOptions, &longindex)) >= 0) {
        if (c == 'o') out_path = optarg;
        else if (c == 't') n_threads = atoi(optarg);
        else if (c == 'h') help = true;
        else if (c == 0 && longindex == 0) stdv_limit = optarg;
        else if (c == 0 && longindex == 1) dwell_path = optarg;
        else if (c == 0 && longindex == 2) keep_first = true;
        else if (c == 0 && longindex == 6) pool = optarg;
        else if (c == 0 && longindex == 7) event_path = optarg;
        else { print_help(stderr); return EXIT_FAILURE; }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    if (argc - optind < 1) { print_help(stderr); return EXIT_FAILURE; }
    { char *end = nullptr; (void)strtold(stdv_limit, &end); if (end == stdv_limit || *end) return die("--stdv_limit must be a number. You entered %s", stdv_limit); }
    if (n_threads < 1) return die("-t must be at least 1. You entered %s", std::to_string(n_threads));
    if (n_threads > 16) n_threads = 16;
    std::vector<std::string> dirs(argv + optind, argv + argc);
    if (pool && dwell_path) return die("--dwell_model cannot be combined with --pool%s");
    if (pool && event_path) return die("--event_model cannot be combined with --pool%s");
    if (event_path && !pgh::can_write_file(event_path)) return die("Could not open %s for writing.", event_path);
    if (pool) return pool_main(dirs, pool, stdv_limit, out_path, keep_first, n_threads);

    const clk::time_point t_start = clk::now();
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    pgh::DumpSet ds;
    std::string err;
    if (!pgh::list_dump_dirs(dirs, n_threads, ds, err)) return die("%s", err);
    const double t_list = secs(t_start, clk::now());

    // batches of whole logical files, bounded by bytes (a larger file is a batch of its own) and by the library's limits
    const uint64_t cap = std::min<uint64_t>(batch_bytes(), 1ull << 31);
    std::vector<std::pair<size_t, size_t>> batches;
    for (size_t i = 0; i < ds.names.size();) {
        if (ds.size[i] > (1ull << 31)) return die("%s is larger than 2^31 bytes", ds.names[i]);
        size_t j = i; uint64_t b = 0;
        while (j < ds.names.size() && j - i < (1u << 22) && (j == i || b + ds.size[j] <= cap)) b += ds.size[j++];
        batches.emplace_back(i, j - i);
        i = j;
    }
    auto read_batch = [&](size_t k) {
        Batch b; b.first = batches[k].first; b.n = batches[k].second;
        const clk::time_point t0 = clk::now();
        b.ok = pgh::read_dump_files(ds, b.first, b.n, n_threads, b.bytes, b.file_off, b.err);
        b.secs = secs(t0, clk::now());
        return b;
    };
    // the first batch is read while the HIP runtime comes up
    std::future<Batch> next;
    if (!batches.empty()) next = std::async(std::launch::async, read_batch, (size_t)0);
    const clk::time_point t_dev0 = clk::now();
    pg_dmodel *h = nullptr;
    if (pg_dmodel_create(0, (keep_first ? PG_MODEL_KEEP_FIRST : 0u) | (event_path ? (uint32_t)PG_DMODEL_EVENTS : 0u), &h) != PG_OK) { if (next.valid()) next.wait(); return die("[model] %s", pg_dmodel_last_error(nullptr)); }
    const double t_create = secs(t_dev0, clk::now());
    double t_read = 0, t_wait = 0, t_submit = 0;
    for (size_t k = 0; k < batches.size(); k++) {
        const clk::time_point w0 = clk::now();
        Batch b = next.get();
        t_wait += secs(w0, clk::now()); t_read += b.secs;
        if (k + 1 < batches.size()) next = std::async(std::launch::async, read_batch, k + 1);
        if (!b.ok) { if (next.valid()) next.wait(); pg_dmodel_destroy(h); return die("%s", b.err); }
        const clk::time_point s0 = clk::now();
        if (pg_dmodel_submit(h, b.bytes.data(), b.file_off.data(), (uint32_t)b.n, PG_LOC_HOST) != PG_OK) { if (next.valid()) next.wait(); const int rc = die("[model] %s", pg_dmodel_last_error(h)); pg_dmodel_destroy(h); return rc; }
        t_submit += secs(s0, clk::now());
    }
    const clk::time_point f0 = clk::now();
    pg_model_result mr; pg_dmodel_info info;
    if (pg_dmodel_finish(h, &mr, &info) != PG_OK) { const int rc = die("[model] %s", pg_dmodel_last_error(h)); pg_dmodel_destroy(h); return rc; }
    const double t_finish = secs(f0, clk::now());
    if (info.n_files != ds.names.size()) { pg_dmodel_destroy(h); return die("[model] internal: %s files came back", std::to_string(info.n_files)); }

    // the event table has no host path: one refused file ends the command before anything is written
    pg_model_result em, es; const uint32_t *ev_status = nullptr; const uint64_t *ev_n = nullptr;
    if (event_path) {
        if (pg_dmodel_finish_events(h, &em, &es, &ev_status, &ev_n) != PG_OK) { const int rc = die("[model] %s", pg_dmodel_last_error(h)); pg_dmodel_destroy(h); return rc; }
        for (uint32_t i = 0; i < mr.n_slots; i++)
            if (ev_status[i]) {
                fprintf(stderr, "[model] the event table of %s is refused: %s\n", ds.names[i].c_str(), pg_dmodel_events_refusal(h, i));
                pg_dmodel_destroy(h);
                return EXIT_FAILURE;
            }
    }
    const clk::time_point p0 = clk::now();
    int status = EXIT_SUCCESS;
    FILE *fp = stdout;
    if (out_path && !(fp = fopen(out_path, "w"))) { pg_dmodel_destroy(h); return die("Could not open %s for writing.", out_path); }
    char a[64], b[64];
    for (uint32_t i = 0; i < mr.n_slots; i++) {
        pg_dmodel_format(h, i, PG_MODEL_TEXT_MEDIAN, a, sizeof a); pg_dmodel_format(h, i, PG_MODEL_TEXT_SSTDEV, b, sizeof b);
        fprintf(fp, "%s\t%s\t%s\n", ds.names[i].c_str(), a, pg_dump_sd_capped(b, stdv_limit) ? stdv_limit : b);
    }
    if (out_path) fclose(fp); else fflush(fp);
    if (dwell_path) {
        FILE *fd = fopen(dwell_path, "a"); // the script appends to this file
        if (!fd) { fprintf(stderr, "Could not open %s for writing.\n", dwell_path); status = EXIT_FAILURE; }
        else {
            for (uint32_t i = 0; i < mr.n_slots; i++) { pg_dmodel_format(h, i, PG_MODEL_TEXT_DWELL, a, sizeof a); fprintf(fd, "%s\t%s\n", ds.names[i].c_str(), a); }
            fclose(fd);
        }
    }
    if (event_path) {
        FILE *fe = fopen(event_path, "w");
        if (!fe) { fprintf(stderr, "Could not open %s for writing.\n", event_path); status = EXIT_FAILURE; }
        else {
            char c4[4][64];
            for (uint32_t i = 0; i < mr.n_slots; i++) {
                for (int32_t col = 0; col < 4; col++) pg_dmodel_format_events(h, i, col, c4[col], sizeof c4[col]);
                fprintf(fe, "%s\t%llu\t%s\t%s\t%s\t%s\n", ds.names[i].c_str(), (unsigned long long)ev_n[i], c4[0], c4[1], c4[2], c4[3]);
            }
            fclose(fe);
        }
    }
    const double t_print = secs(p0, clk::now());
    fprintf(stderr, "[model] n_files: %llu n_bytes: %llu n_values: %llu n_batches: %u n_host_files: %llu\n", (unsigned long long)info.n_files,
            (unsigned long long)info.n_bytes, (unsigned long long)info.n_values, info.n_batches, (unsigned long long)info.n_host_files);
    fprintf(stderr, "[model] time: listing %.3f s, device context %.3f s, reading files %.3f s on %d threads (waited for: %.3f s), submit %.3f s, finish %.3f s, printing %.3f s\n",
            t_list, t_create, t_read, n_threads, t_wait, t_submit, t_finish, t_print);
    pg_dmodel_destroy(h);
    return status;
}
