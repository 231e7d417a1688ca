// main.cpp -- `poregen` dispatcher (src/main.c:64-103): the gmove, kmer_freq, f1_score, subtool0, pa_stats, model, offsets, fit, realign, simulate and eventalign subtools (device path),
// reform and transform (host-only; transform --signal runs pa_stats' device path).
#include <cstdio>
#include <cstring>
#include <string>
#include <sys/resource.h>
#include <sys/time.h>
#include <cstdlib>
#include <unistd.h>

#ifdef PG_REFORM_ONLY // the sanitizer build of the host-only subtools, reform and transform (Makefile: asan): no device code linked
static int gmove_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int kmer_freq_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int f1_score_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int subtool0_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int pa_stats_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int model_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int offsets_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int fit_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int realign_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int simulate_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
static int eventalign_main(int, char **) { fprintf(stderr, "[poregen] this build holds reform only\n"); return 1; }
#else
int gmove_main(int argc, char **argv);
int kmer_freq_main(int argc, char **argv);
int f1_score_main(int argc, char **argv);
int subtool0_main(int argc, char **argv);
int pa_stats_main(int argc, char **argv);
int model_main(int argc, char **argv);
int offsets_main(int argc, char **argv);
int fit_main(int argc, char **argv);
int realign_main(int argc, char **argv);
int simulate_main(int argc, char **argv);
int eventalign_main(int argc, char **argv);
#endif
int reform_main(int argc, char **argv);
int transform_main(int argc, char **argv);

static double realtime() { struct timeval tp; gettimeofday(&tp, nullptr); return tp.tv_sec + tp.tv_usec * 1e-6; }
static double cputime() { struct rusage r; getrusage(RUSAGE_SELF, &r); return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec); }
static long peakrss() { struct rusage r; getrusage(RUSAGE_SELF, &r); return r.ru_maxrss * 1024; }

static int usage(FILE *fp, int code) {
    fprintf(fp, "Usage: poregen <command> [options]\n\ncommand:\n         gmove      move k-mer signal samples into k-mer buckets (MI355X implementation)\n         reform     rewrite a SAM/BAM move table as TSV or as PAF with ss:Z:\n         kmer_freq  count the k-mers of the reads in a FASTQ, BAM or SAM file\n         f1_score   compare two ss signal alignments (SAM/BAM) point by point: TP/FP/TN/FN, F1 score\n         subtool0   mean pA of every read of a SLOW5/BLOW5 file\n         pa_stats   mean and sample standard deviation of every pA value of a SLOW5/BLOW5 file\n         model      k-mer model (median, stddev, dwell) from the files of dump directories\n         offsets    which base of the k-mer decides the level: medians of the dump files pooled by the base at every position\n         transform  the final model file from a raw k-mer model: (median * stdv) + mean, stddev projected onto [2.5, 4]\n         fit        score a k-mer model against signal and move tables: per read shift and scale, per k-mer the residuals\n         realign    refine the event boundaries of the move table against a k-mer model: PAF with ss:Z:, per read and per k-mer the residuals before and after\n         simulate   draw raw signal and its true alignment from a k-mer model: SLOW5/BLOW5, PAF with ss:Z:, FASTQ, SAM with a move table\n         eventalign one line per event against a k-mer model: position, level, spread, model level and standardized level (nanopolish / f5c eventalign columns)\n");
    return code;
}

int main(int argc, char **argv) {
    const double t0 = realtime();
    if (argc < 2) return usage(stderr, 1);
    int ret;
    if (strcmp(argv[1], "gmove") == 0) ret = gmove_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "reform") == 0) ret = reform_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "kmer_freq") == 0) ret = kmer_freq_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "f1_score") == 0) ret = f1_score_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "subtool0") == 0) ret = subtool0_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "pa_stats") == 0) ret = pa_stats_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "model") == 0) ret = model_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "offsets") == 0) ret = offsets_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "transform") == 0) ret = transform_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "fit") == 0) ret = fit_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "realign") == 0) ret = realign_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "simulate") == 0) ret = simulate_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "eventalign") == 0) ret = eventalign_main(argc - 1, argv + 1);
    else if (strcmp(argv[1], "--version") == 0 || strcmp(argv[1], "-V") == 0) { fprintf(stdout, "poregen 0.1.0 (pgmove, gfx950)\n"); return 0; }
    else if (strcmp(argv[1], "--help") == 0 || strcmp(argv[1], "-h") == 0) return usage(stdout, 0);
    else { fprintf(stderr, "[poregen] Unrecognised command %s\n", argv[1]); return usage(stderr, 1); }
    fprintf(stderr, "[%s] Version: %s\n", __func__, "0.1.0");
    fprintf(stderr, "[%s] CMD:", __func__);
    for (int i = 0; i < argc; ++i) fprintf(stderr, " %s", argv[i]);
    fprintf(stderr, "\n[%s] Real time: %.3f sec; CPU time: %.3f sec; Peak RAM: %.3f GB\n\n", __func__, realtime() - t0, cputime(), peakrss() / 1024.0 / 1024.0 / 1024.0);
    // Everything this process owns is closed and flushed by now. Tearing the HIP runtime down call by call (static destructors,
    // hsa_shut_down, one hipFree per buffer) takes 0.1-0.2 s of a run that lasts 0.3-0.7 s; the operating system reclaims the
    // same resources at exit. POREGEN_CLEAN_EXIT=1 keeps the orderly teardown (sanitizer and leak-check runs).
    if (!getenv("POREGEN_CLEAN_EXIT")) { fflush(stdout); fflush(stderr); _exit(ret); }
    return ret;
}
