// offsets_cli.cpp -- `poregen offsets`: which base position of the k-mer under the pore decides the current level. The reference takes the
// answer (SIG_MOVE_OFFSET=4 in scripts/poregen.sh, --base_shift afterwards) from a separate tool, squigualiser calculate_offsets; here it
// is a question to the dump files themselves: pool every file with A at position j, every one with C there, and so on -- K labelings of 4
// groups over one parse and one arena (pg_pool_*, include/pgmove.h) -- and look where the four pooled medians lie furthest apart. A pool's
// numbers are `cat` of its files | tr ';,' '\n' | tail -n +2 | datamash median 1 / sstdev 1 (scripts/poregen.sh:73-74).
//   base    POS  B  n_files  n_values  median  stddev      4K rows, POS 0..K-1, B in the order A C G T (or U)
//   spread  POS  S                                         K rows: largest - smallest median of the position's groups that have a value
//   best    POS                                            the position with the largest S (ties: the lowest); omitted when no POS has one
#include "pg_cli.h"
#include "pg_dumpdir.h"
#include "pg_poolnames.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <getopt.h>
#include <string>
#include <vector>

namespace {

const struct option kLongOptions[] = {
    {"keep_first", no_argument, nullptr, 0},     // 0
    {"output", required_argument, nullptr, 'o'}, // 1
    {"threads", required_argument, nullptr, 't'},// 2
    {"help", no_argument, nullptr, 'h'},         // 3
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen offsets [options] DUMP_DIR [DUMP_DIR ...]\n");
    fprintf(fp, "\nper base position of the dump files' k-mer names: median and stddev of the files pooled by the base there, and the spread of the four medians\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   --keep_first               keep the first value of every pool (the pipeline's `tail -n +2` drops it)\n");
    fprintf(fp, "   -t INT                     threads that read files [8], at most 16\n");
    fprintf(fp, "   -h                         help\n");
}

} // namespace

int offsets_main(int argc, char **argv) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const char *out_path = nullptr;
    bool keep_first = false, help = false;
    int n_threads = 8;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:t:h", kLongOptions, &longindex)) >= 0) {
        if (c == 'o') out_path = optarg;
        else if (c == 't') n_threads = atoi(optarg);
        else if (c == 'h') help = true;
        else if (c == 0 && longindex == 0) keep_first = true;
        else { print_help(stderr); return EXIT_FAILURE; }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    if (argc - optind < 1) { print_help(stderr); return EXIT_FAILURE; }
    if (n_threads < 1) return die("-t must be at least 1. You entered %s", std::to_string(n_threads));
    if (n_threads > 16) n_threads = 16;
    std::vector<std::string> dirs(argv + optind, argv + argc);

    const clk::time_point t_start = clk::now();
    pgh::DumpSet ds;
    std::string err;
    if (!pgh::list_dump_dirs(dirs, n_threads, ds, err)) return die("%s", err);
    pgh::PoolNames pn;
    if (!pgh::check_pool_names(ds.names, pn, err)) return die("[offsets] %s", err);
    if (pn.k > PG_POOL_MAX_LABELINGS) return die("[offsets] names of length %s: at most 16 bases are taken", std::to_string(pn.k));
    const double t_list = secs(t_start, clk::now());
    const uint32_t K = (uint32_t)pn.k;
    pg_pool *h = nullptr; pg_pool_result res; pgh::PoolTimes tm;
    auto groups_of = [&](size_t f, uint32_t *g) { for (uint32_t j = 0; j < K; j++) g[j] = pgh::pool_base_code(ds.names[f][j]); };
    if (!pgh::run_pool(ds, n_threads, keep_first, std::vector<uint32_t>(K, 4u), groups_of, &h, res, tm, err)) return die("[offsets] %s", err);
    uint32_t bad; std::string what;
    if (pgh::pool_refused(ds, h, res, bad, what)) {
        fprintf(stderr, "[offsets] group %c at position %u is refused: %s\n", pn.alphabet[bad % 4], bad / 4, what.c_str());
        pg_pool_destroy(h);
        return EXIT_FAILURE;
    }
    const clk::time_point p0 = clk::now();
    FILE *fp = stdout;
    if (out_path && !(fp = fopen(out_path, "w"))) { pg_pool_destroy(h); return die("Could not open %s for writing.", out_path); }
    char a[64], b[64];
    std::vector<__int128> spread(K, -1); // in half units (mid_lo + mid_hi); -1: fewer than two groups have a value
    for (uint32_t j = 0; j < K; j++) {
        __int128 lo = 0, hi = 0; int have = 0;
        for (uint32_t x = 0; x < 4; x++) {
            const uint32_t g = 4 * j + x;
            pg_pool_format(h, g, PG_MODEL_TEXT_MEDIAN, a, sizeof a); pg_pool_format(h, g, PG_MODEL_TEXT_SSTDEV, b, sizeof b);
            fprintf(fp, "base\t%u\t%c\t%llu\t%llu\t%s\t%s\n", j, pn.alphabet[x], (unsigned long long)res.n_files[g], (unsigned long long)res.model.n_values[g], a, b);
            if (!res.model.n_values[g]) continue;
            const __int128 m2 = (__int128)res.model.mid_lo[g] + res.model.mid_hi[g];
            if (!have || m2 < lo) lo = m2;
            if (!have || m2 > hi) hi = m2;
            have++;
        }
        if (have >= 2) spread[j] = hi - lo;
    }
    int best = -1;
    for (uint32_t j = 0; j < K; j++) {
        if (spread[j] < 0) { fprintf(fp, "spread\t%u\t\n", j); continue; }
        fprintf(fp, "spread\t%u\t%.14Lg\n", j, (long double)spread[j] / 2e8L);
        if (best < 0 || spread[j] > spread[(size_t)best]) best = (int)j;
    }
    if (best >= 0) fprintf(fp, "best\t%d\n", best);
    if (out_path) fclose(fp); else fflush(fp);
    pgh::pool_summary("offsets", res, tm, t_list, secs(p0, clk::now()), n_threads);
    pg_pool_destroy(h);
    return EXIT_SUCCESS;
}
