// reform_cli.cpp -- `poregen reform`: rewrite a basecaller move table (SAM/BAM tags mv:B:c, ns, ts) as a
// per-k-mer TSV or as the PAF + ss:Z: records `poregen gmove --paf` consumes.
//
// Replaces reform() of the reference (src/reform.cpp:79-371). Host-only: the work is one pass over a byte
// array per read, far below anything worth a kernel launch. The output is derived from the list of move
// positions of each read instead of the reference's three interleaved scans; the bytes written are the same
// (pinned by the reference's own expected files, tests/golden/reform/).
#include "../pg_refops.h"
#include "pg_moverecs.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <getopt.h>
#include <string>
#include <vector>

namespace {

constexpr uint32_t kDefaultStride = 5; // EXPECTED_STRIDE, src/reform.cpp:22

// --rna, --stride: what `squigualiser reform --rna` adds to the reference's reform (scripts/poregen.sh STEP 4) and the stride of an
// RNA004 basecaller's move table (10)
struct Extra {
    bool rna = false;
    uint32_t stride = kDefaultStride; // the stride mv[0] has to hold; 0: whatever it holds, from 1 up (the gmove BAM path takes any)
    bool both_strands = false;        // --to_ref --both_strands: reverse-strand records are written against RNAME + rc_suffix
    std::string rc_suffix = "_rc";
};

const struct option kLongOptions[] = {
    {"kmer_length", required_argument, nullptr, 'k'},
    {"sig_move_offset", required_argument, nullptr, 'm'},
    {"", no_argument, nullptr, 'c'},
    {"threads", required_argument, nullptr, 't'},
    {"batchsize", required_argument, nullptr, 'K'},
    {"max-bytes", required_argument, nullptr, 'B'},
    {"verbose", required_argument, nullptr, 'v'},
    {"help", no_argument, nullptr, 'h'},
    {"version", no_argument, nullptr, 'V'},
    {"output", required_argument, nullptr, 'o'},
    {"debug-break", required_argument, nullptr, 0},
    {"rna", no_argument, nullptr, 0},
    {"stride", required_argument, nullptr, 0},
    {"to_ref", no_argument, nullptr, 0},
    {"both_strands", no_argument, nullptr, 0},
    {"rc_suffix", required_argument, nullptr, 0},
    {nullptr, 0, nullptr, 0}};

void usage(FILE *fp, uint32_t k, uint32_t m) {
    fprintf(fp, "Usage: poregen reform basecalled.SAM/BAM\n\nbasic options:\n");
    fprintf(fp, "   -k, --kmer_length          kmer length [%u]\n", k);
    fprintf(fp, "   -m, --sig_move_offset      signal move offset [%u]\n", m);
    fprintf(fp, "   -c                         write move table in paf format\n");
    fprintf(fp, "   -h                         help\n");
    fprintf(fp, "   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   --verbose INT              verbosity level\n");
    fprintf(fp, "   --version                  print version\n");
    fprintf(fp, "   --rna                      dataset is rna: PAF target columns n_kmers, 0 and a k-mer index that counts down\n");
    fprintf(fp, "   --stride INT               expected stride of the move table, 0 = any [%u]\n", kDefaultStride);
    fprintf(fp, "   --to_ref                   mapped SAM/BAM (dorado --reference, dorado aligner), with -c -k 1 -m 0: carry the ops through every record's\n");
    fprintf(fp, "                              CIGAR onto the reference -- the PAF of the signal-to-reference alignment that `gmove FILE.paf --fastq REF.fa`\n");
    fprintf(fp, "                              reads: qname, ns, query_start, query_end, +, RNAME, its length, target_start, target_end, n_match, ref_len,\n");
    fprintf(fp, "                              255, ss:Z: with N, / NI / ND (with --rna: the CIGAR in reverse order, target_start > target_end). Unmapped\n");
    fprintf(fp, "                              and reverse-strand records (flag 0x4, no RNAME, flag 0x10) are skipped and counted, secondary and\n");
    fprintf(fp, "                              supplementary ones (0x900) dropped; a read whose table or CIGAR is refused ends the run\n");
    fprintf(fp, "   --both_strands             with --to_ref: reverse-strand records (flag 0x10) are written too, as forward records on the reverse\n");
    fprintf(fp, "                              complement of their reference: strand -, target name RNAME + the suffix, target columns counted from the\n");
    fprintf(fp, "                              other end (length - pos - ref_len). `gmove FILE.paf --fastq BOTH.fa` reads the file when BOTH.fa holds every\n");
    fprintf(fp, "                              sequence and, under the suffixed name, its reverse complement. Needs the @SQ lengths\n");
    fprintf(fp, "   --rc_suffix STR            with --both_strands: the suffix [_rc]\n");
}

// --to_ref: every record through the two rules the kernels compile (pg_mvops.h, pg_refops.h), on the host. 0, or 1 behind the message.
int to_ref(FILE *out, pgh::SamBamReader &rd, const Extra &x) {
    pgh::RawMoveRec raw;
    std::string bad;
    std::vector<uint32_t> ops, op_n; std::vector<uint8_t> seq, op_t;
    uint64_t skipped = 0, reverse_taken = 0;
    int got;
    while ((got = pgh::next_move_record(rd, raw, "reform", bad, &skipped, x.both_strands ? &reverse_taken : nullptr)) > 0) {
        if (x.stride && raw.stride != (int)x.stride) { fprintf(stderr, "[reform::ERROR]\033[1;31m expected stride of %u is missing. Read_id: %s\033[0m\n", x.stride, raw.qname.c_str()); return 1; }
        const uint32_t L = raw.l_seq, nw = (uint32_t)raw.cigar.size();
        ops.assign((size_t)L + 1, 0); seq.resize((size_t)L + 1); op_n.resize((size_t)L + nw + 1); op_t.resize((size_t)L + nw + 1);
        uint32_t n_ops = 0; int32_t qs = 0;
        const uint32_t st = pg_mv_expand_host((const uint8_t *)raw.mv, raw.mv_len - 1, raw.stride, raw.ns, raw.ts, L, raw.packed, false, false, ops.data(), &n_ops, &qs, seq.data());
        const bool reverse = (raw.flag & 0x10u) != 0; // (taken with --both_strands only)
        const PgRfHost h = pg_refops_host(ops.data(), n_ops, qs, st, raw.cigar.data(), nw, raw.pos, x.rna, op_n.data(), op_t.data(), reverse, pgh::contig_len_of(raw.ref_len));
        if (h.status) {
            fprintf(stderr, "%s\n", pgh::reform_error((std::string(pgh::to_ref_refusal(h.status)) + " (status " + std::to_string(h.status) + ")").c_str(), raw.qname).c_str());
            return 1;
        }
        fprintf(out, "%s\t%" PRIu64 "\t%d\t%d\t%c\t%s%s\t%" PRId64 "\t%d\t%d\t%" PRIu32 "\t%" PRIu32 "\t255\tss:Z:", raw.qname.c_str(), raw.ns, h.query_start, h.query_end,
                reverse ? '-' : '+', raw.rname.c_str(), reverse ? x.rc_suffix.c_str() : "", raw.ref_len, h.target_start, h.target_end, h.n_match, h.ref_len);
        for (uint32_t i = 0; i < h.n_ops; i++) fprintf(out, "%" PRIu32 "%c", op_n[i], ",ID"[op_t[i]]);
        fputc('\n', out);
    }
    if (got < 0) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    if (x.both_strands) pgh::print_both_strands_skipped("reform", skipped, reverse_taken); else pgh::print_to_ref_skipped("reform", skipped);
    return 0;
}

int fail(const char *msg) {
    fprintf(stderr, "[reform::ERROR]\033[1;31m %s\033[0m\n", msg);
    return -1;
}

// One record. Returns 0, or -1 where the reference returns -1 (src/reform.cpp:212-240,344-357) or would read
// past the end of the mv array (src/reform.cpp:248-254,287-294: fewer than sig_move_offset+1 moves).
int reform_record(FILE *out, const pgh::MoveRec &r, uint32_t k, uint32_t m, bool paf, const Extra &x) {
    if (!r.has_ns) return fail("tag 'ns' is not found. Please check your SAM/BAM file: ");
    if (!r.has_ts) return fail("tag 'ts' is not found. Please check your SAM/BAM file: ");
    if (!r.has_mv) return fail("NULL returned for tag mv: ");
    if (!r.mv_is_Bc) return fail("tag 'mv' specification is incorrect");
    if (r.mv_len == 0) return fail("mv array length is 0: ");
    if (x.stride ? r.stride != (int)x.stride : r.stride < 1) {
        if (x.stride == kDefaultStride) return fail("expected stride of 5 is missing.");
        if (!x.stride) return fail("the stride of the move table (mv[0]) is less than 1.");
        fprintf(stderr, "[reform::ERROR]\033[1;31m expected stride of %u is missing.\033[0m\n", x.stride);
        return -1;
    }
    const uint32_t stride = (uint32_t)r.stride;

    const uint32_t len_mv = r.mv_len;
    const int64_t ns = (int64_t)r.ns, ts = (int64_t)r.ts;
    // 1-based positions in mv[] of the moves
    std::vector<uint32_t> pos;
    for (uint32_t i = 1; i < len_mv; i++)
        if (r.is_one[i - 1]) pos.push_back(i);
    if (pos.size() < (size_t)m + 1) return fail("the move table holds fewer moves than sig_move_offset + 1");

    // number of k-mers, with the reference's unsigned wrap-around when the read is shorter than k-1
    uint32_t n_kmers = (uint32_t)r.seq.size() - k + 1;
    const uint32_t first = pos[m];            // the move that opens k-mer 0
    const size_t n_after = pos.size() - (m + 1); // moves that close a k-mer
    const bool body = first + 1 <= len_mv - 1;  // at least one mv element lies after `first`
    const char *id = r.qname.c_str();

    if (!paf) { // src/reform.cpp:245-282
        uint64_t start = (uint64_t)(ts + ((int64_t)first - 1) * stride);
        // --rna: the rows keep their signal order, the index counts down from n_kmers - 1 (the 3' end is sequenced first)
        uint32_t kmer_idx = x.rna ? n_kmers - 1 : 0;
        const uint32_t step = x.rna ? (uint32_t)-1 : 1u;
        for (size_t j = 0; j < n_after && n_kmers > 0; j++, n_kmers--) {
            const uint64_t end = (uint64_t)(ts + ((int64_t)pos[m + 1 + j] - 1) * stride);
            fprintf(out, "%s\t%" PRIu32 "\t%" PRIu64 "\t%" PRIu64 "\n", id, kmer_idx, start, end);
            kmer_idx += step;
            start = end;
        }
        if (body && n_kmers > 0) // the last k-mer runs to the end of the signal
            fprintf(out, "%s\t%" PRIu32 "\t%" PRIu64 "\t%" PRIu64 "\n", id, kmer_idx, start, (uint64_t)ns);
        return 0;
    }

    // PAF, src/reform.cpp:284-358. Column 4: the raw-signal end = the move that closes the last k-mer
    // (counted over ALL moves, the skipped ones included), or ns when the table runs out first.
    const uint32_t want = n_kmers + m + 1;
    uint64_t raw_end;
    if (want > pos.size()) raw_end = (uint64_t)ns;
    else raw_end = (uint64_t)(ts + ((int64_t)(want ? pos[want - 1] : 2u) - 1) * stride);
    fprintf(out, "%s\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t+\t%s\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t255\tss:Z:", id, (uint64_t)ns,
            (uint64_t)(ts + ((int64_t)first - 1) * stride), raw_end, id, n_kmers, x.rna ? n_kmers : 0u, x.rna ? 0u : n_kmers, n_kmers, n_kmers);
    uint32_t prev = first;
    for (size_t j = 0; j < n_after && n_kmers > 0; j++, n_kmers--) {
        fprintf(out, "%" PRIu32 ",", (pos[m + 1 + j] - prev) * stride);
        prev = pos[m + 1 + j];
    }
    if (body && n_kmers > 0) {
        const uint32_t last = len_mv - 1;
        const int64_t tail = ns - ((int64_t)((last - 1) * stride) + ts);
        if (tail < 0) return fail("Error in calcuation. (ns - ((i-1)*EXPECTED_STRIDE + ts)) > 0 is not valid");
        n_kmers--;
        fprintf(out, "%" PRIu32 ",", (uint32_t)((last - prev) * stride + tail));
    }
    if (n_kmers != 0) {
        fprintf(stderr, "[reform::ERROR]\033[1;31m Error in the implementation. Please report the command with minimal reproducible data. Read_id: %s\033[0m\n", id);
        return -1;
    }
    fputc('\n', out);
    return 0;
}

} // namespace

int reform_main(int argc, char **argv) {
    uint32_t k = 9, m = 0; // init_opt, src/poregen.cpp:209-237
    bool paf = false, help_to_stdout = false, to_ref_mode = false, have_rc_suffix = false;
    Extra extra;
    const char *out_path = nullptr;
    int c, longindex = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "k:m:ct:B:K:v:o:hV", kLongOptions, &longindex)) >= 0) {
        if (c == 'k') k = (uint32_t)atoi(optarg);
        else if (c == 'm') m = (uint32_t)atoi(optarg);
        else if (c == 'c') paf = true;
        else if (c == 'K') { if (atoi(optarg) < 1) { fail("Batch size should larger than 0."); exit(EXIT_FAILURE); } }
        else if (c == 't') { if (atoi(optarg) < 1) { fail("Number of threads should larger than 0."); exit(EXIT_FAILURE); } }
        else if (c == 'o') out_path = optarg;
        else if (c == 'V') { fprintf(stdout, "subtool0 0.1.0\n"); exit(EXIT_SUCCESS); }
        else if (c == 'h') help_to_stdout = true;
        else if (c == 0 && !strcmp(kLongOptions[longindex].name, "rna")) extra.rna = true;
        else if (c == 0 && !strcmp(kLongOptions[longindex].name, "to_ref")) to_ref_mode = true;
        else if (c == 0 && !strcmp(kLongOptions[longindex].name, "both_strands")) extra.both_strands = true;
        else if (c == 0 && !strcmp(kLongOptions[longindex].name, "rc_suffix")) { extra.rc_suffix = optarg; have_rc_suffix = true; }
        else if (c == 0 && !strcmp(kLongOptions[longindex].name, "stride")) {
            if (atoi(optarg) < 0) { fail("Stride should not be negative."); exit(EXIT_FAILURE); }
            extra.stride = (uint32_t)atoi(optarg);
        }
    }
    if (k < 1) return fail("kmer length must be a positive integer");
    if (k <= m) return fail("signal move offset value must less than the kmer length");
    if (to_ref_mode && !help_to_stdout && (!paf || k != 1 || m != 0)) { fail("--to_ref requires -c -k 1 -m 0"); usage(stderr, k, m); return EXIT_FAILURE; }
    if (extra.both_strands && !to_ref_mode && !help_to_stdout) { fail("--both_strands applies with --to_ref only"); usage(stderr, k, m); return EXIT_FAILURE; }
    if (have_rc_suffix && !extra.both_strands && !help_to_stdout) { fail("--rc_suffix applies with --both_strands only"); usage(stderr, k, m); return EXIT_FAILURE; }
    if (argc - optind != 1 || help_to_stdout) {
        fail("not enough arguments");
        usage(help_to_stdout ? stdout : stderr, k, m);
        if (help_to_stdout) exit(EXIT_SUCCESS);
        return EXIT_FAILURE;
    }
    const char *in_path = argv[optind];
    fprintf(stderr, "bam_file : %s\nkmer length : %" PRIu32 "\nsignal move offset : %" PRIu32 "\noutput format : %s\n", in_path, k, m, paf ? "paf" : "tsv");

    FILE *out = stdout;
    if (out_path) {
        out = fopen(out_path, "w");
        if (!out) { fprintf(stderr, "[reform::ERROR]\033[1;31m Failed to open %s\033[0m\n", out_path); exit(EXIT_FAILURE); }
    }
    pgh::SamBamReader rd;
    std::string err;
    if (!rd.open(in_path, err)) { fprintf(stderr, "[reform::ERROR]\033[1;31m %s: %s\033[0m\n", in_path, err.c_str()); exit(EXIT_FAILURE); }
    if (to_ref_mode) {
        const int rc = to_ref(out, rd, extra);
        if (out_path) fclose(out); else fflush(out);
        return rc;
    }
    pgh::MoveRec rec;
    int got, ret = 0;
    while ((got = rd.next(rec, err)) > 0)
        if ((ret = reform_record(out, rec, k, m, paf, extra)) != 0) break;
    if (got < 0) { fail(err.c_str()); ret = -1; }
    if (out_path) fclose(out);
    else fflush(out);
    return ret;
}
