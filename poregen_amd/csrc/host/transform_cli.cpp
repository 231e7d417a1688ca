// transform_cli.cpp -- `poregen transform`: STEP 7 of the reference's pipeline (scripts/poregen.sh:87-129 apply_transformation, :131-148
// set_stddev) as a tool of its own. The reference has no such command: its script pipes two expressions per row into `bc -l` and takes
// min / max from datamash. The arithmetic is pg_transform.h over pg_bcdec.h, on the host; nothing here touches the GPU unless --signal
// asks for the dataset's mean and sstdev, which is pa_stats' walk (subtool0_cli.cpp) in this process.
//   * the output is assembled in memory and -o is opened only when every row is done: a refused model writes nothing, exit 1
//   * --signal FILE: A and B are the two "%.14g" texts `poregen pa_stats FILE` prints, echoed on stderr; a text with an exponent is
//     refused like any other text that is no number to bc
#include "../pg_transform.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <getopt.h>
#include <string>

#ifdef PG_REFORM_ONLY // the sanitizer build of the host-only subtools (Makefile: asan): no device code linked
static void pa_stats_texts(const char *, const char *, std::string &, std::string &) { fprintf(stderr, "[transform] this build has no --signal\n"); exit(EXIT_FAILURE); }
#else
void pa_stats_texts(const char *tool, const char *path, std::string &mean, std::string &sstdev);
#endif

namespace {

const struct option kLongOptions[] = {
    {"stdv", required_argument, nullptr, 0},      // 0
    {"mean", required_argument, nullptr, 0},      // 1
    {"signal", required_argument, nullptr, 0},    // 2
    {"stdv_min", required_argument, nullptr, 0},  // 3
    {"stdv_max", required_argument, nullptr, 0},  // 4
    {"stdv_from", required_argument, nullptr, 0}, // 5
    {"output", required_argument, nullptr, 'o'},  // 6
    {"help", no_argument, nullptr, 'h'},          // 7
    {nullptr, 0, nullptr, 0}};

void print_help(FILE *fp) {
    fprintf(fp, "Usage: poregen transform [options] RAW_MODEL\n");
    fprintf(fp, "\nthe model file f5c, squigulator or uncalled4 load, from KMER<TAB>median<TAB>stddev rows: level_mean = (median * A) + B,\n");
    fprintf(fp, "level_stdv = (stddev - min) * (D - C) / (max - min) + C, digit for digit as `bc -l` prints them\n");
    fprintf(fp, "\noptions:\n");
    fprintf(fp, "   --stdv NUM                 A: sstdev of the whole pA dataset (the reference's example: 17.569300789355)\n");
    fprintf(fp, "   --mean NUM                 B: mean of the whole pA dataset (84.112089074928)\n");
    fprintf(fp, "   --signal FILE              instead of --stdv and --mean: compute both from reads.{slow5,blow5} on the GPU (what `poregen pa_stats FILE` prints)\n");
    fprintf(fp, "   --stdv_min NUM             C: lower end of the level_stdv range [2.5]\n");
    fprintf(fp, "   --stdv_max NUM             D: upper end of the level_stdv range [4]\n");
    fprintf(fp, "   --stdv_from MODEL          take the level_stdv column from MODEL, row by row (scripts/poregen.sh set_stddev)\n");
    fprintf(fp, "   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   -h                         help\n");
}

bool read_file(const char *path, std::string &data) {
    FILE *fp = fopen(path, "rb");
    if (!fp) return false;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) data.append(buf, got);
    const bool ok = !ferror(fp);
    fclose(fp);
    return ok;
}

int die(const char *fmt, const std::string &a) { fprintf(stderr, "[transform::ERROR]\033[1;31m "); fprintf(stderr, fmt, a.c_str()); fprintf(stderr, "\033[0m\n"); return EXIT_FAILURE; }

} // namespace

int transform_main(int argc, char **argv) {
    const char *A = nullptr, *B = nullptr, *signal = nullptr, *C = "2.5", *D = "4", *from_path = nullptr, *out_path = nullptr;
    bool help = false;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:h", kLongOptions, &longindex)) >= 0) {
        if (c == 'o') out_path = optarg;
        else if (c == 'h') help = true;
        else if (c == 0 && longindex == 0) A = optarg;
        else if (c == 0 && longindex == 1) B = optarg;
        else if (c == 0 && longindex == 2) signal = optarg;
        else if (c == 0 && longindex == 3) C = optarg;
        else if (c == 0 && longindex == 4) D = optarg;
        else if (c == 0 && longindex == 5) from_path = optarg;
        else { print_help(stderr); return EXIT_FAILURE; }
    }
    if (help) { print_help(stdout); return EXIT_SUCCESS; }
    // exactly one of --signal and the pair --stdv + --mean
    if (argc - optind != 1 || (signal ? (A || B) : !(A && B))) { print_help(stderr); return EXIT_FAILURE; }

    std::string raw, from, mean_text, stdv_text;
    if (!read_file(argv[optind], raw)) return die("Could not read %s", argv[optind]);
    if (from_path && !read_file(from_path, from)) return die("Could not read %s", from_path);
    if (signal) {
        pa_stats_texts("transform", signal, mean_text, stdv_text);
        fprintf(stderr, "[transform] --mean %s --stdv %s (pa_stats of %s)\n", mean_text.c_str(), stdv_text.c_str(), signal);
        A = stdv_text.c_str(); B = mean_text.c_str();
    }
    std::string out, err;
    if (!pgtr::transform(raw.data(), raw.size(), A, B, C, D, from_path ? from.data() : nullptr, from.size(), out, err)) return die("%s: nothing written", err);

    FILE *fp = stdout;
    if (out_path && !(fp = fopen(out_path, "w"))) return die("Could not open %s for writing.", out_path);
    const bool ok = fwrite(out.data(), 1, out.size(), fp) == out.size();
    if ((out_path ? fclose(fp) : fflush(fp)) != 0 || !ok) return die("Could not write %s", out_path ? out_path : "the output");
    return EXIT_SUCCESS;
}
