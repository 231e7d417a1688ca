// f1_cli.cpp -- `poregen f1_score`: the reference's F1-score metric (src/f1_score/f1score.py) over libpgmove's pg_fscore_* (include/pgmove.h).
// Host work here: options, reading both files (f1_reader.cpp), the dict rules, parsing si, packing the ss bytes of the compared pairs,
// the metrics and printing. The per-signal-point comparison runs on the device.
//
// Rules kept from the reference, with its lines:
//   * argparse (:234-246): bam1 bam2, --read_limit (100), --base_shift (0), --read_id, --region, --rna, --threshold (0), as
//     "--opt value" or "--opt=value"; the int options as Python int(). Usage errors print argparse's usage and exit 2; -h / --help
//     prints the help and exits 0. Prefix abbreviations are not accepted.
//   * a record is kept when flag 0x100 and 0x10 are clear; every kept record of both files must carry ss and si (Z tags), checked
//     while file 1 and then file 2 are loaded in full (:157-190). read name -> record: a repeated name keeps its first position and
//     its last record (:186-188).
//   * --region (:59-66, :166): commas removed, "CHR:START-END" with two ints, else an error; records as fetch(CHR, START, END) gives
//     them: contig CHR (a contig the header does not list is an error), pos < END and bam_endpos > START (START < 0 or START > END
//     are pysam's errors). The file is scanned in order (no index), so SAM text works too, where pysam refuses.
//   * pairs in file 1's order (:199-231): --read_id skips every other name without counting it; names missing from file 2 are
//     not compared but count; the loop stops when the count equals --read_limit (0 or negative: never).
//   * si split on ',' and every field parsed as int() with at least 4 fields; first signal si[0], first ref si[2] (both DNA and RNA:
//     :212-224 and :21 swap si[2] / si[3] twice), --base_shift added to side 2 (:217-221), direction -1 with --rna.
//   * metrics (:121-133) in double, zero denominators 0.0, printed as :230-231 print them.
// Errors (exit 1, a message naming the read on stderr, nothing on stdout) where the reference raises. Refused although Python would
// go on: si values or --base_shift of magnitude 2^62 or more, non-ASCII si, op counts >= 2^32, non-ASCII ss bytes.
#include "../../../include/pgmove.h"
#include "pg_f1_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

const char *kUsage = "usage: f1_score [-h] [--read_limit READ_LIMIT] [--base_shift BASE_SHIFT] [--read_id READ_ID] [--region REGION] [--rna]\n"
                     "                [--threshold THRESHOLD]\n"
                     "                bam1 bam2\n";

void print_help() {
    fputs(kUsage, stdout);
    fputs("\nCompare BAM/SAM files.\n\npositional arguments:\n"
          "  bam1                  Path to the first BAM/SAM file.\n"
          "  bam2                  Path to the second BAM/SAM file.\n\noptions:\n"
          "  -h, --help            show this help message and exit\n"
          "  --read_limit READ_LIMIT\n                        Limit the number of records to process.\n"
          "  --base_shift BASE_SHIFT\n                        Base shift to apply to the second alignment file.\n"
          "  --read_id READ_ID     Specific read ID to compare.\n"
          "  --region REGION       Genomic region to filter reads, format: 'chr:start-end'.\n"
          "  --rna                 specify for RNA reads\n"
          "  --threshold THRESHOLD\n                        margin of error between reference positions allowed\n", stdout);
}

int usage_error(const std::string &msg) {
    fputs(kUsage, stderr);
    fprintf(stderr, "f1_score: error: %s\n", msg.c_str());
    return 2;
}

int fail(const std::string &msg) {
    fprintf(stderr, "[f1_score::ERROR] %s\n", msg.c_str());
    return 1;
}

struct Region { std::string chrom; int64_t start = 0, end = 0; };

// parse_region (:59-66): commas removed, exactly one ':', START-END as exactly two ints
bool parse_region(const std::string &in, Region &r, std::string &err) {
    std::string s;
    for (char c : in) if (c != ',') s += c;
    const size_t c1 = s.find(':');
    if (c1 == std::string::npos || s.find(':', c1 + 1) != std::string::npos) { err = "Region must be in the format 'chr:start-end'."; return false; }
    const std::string pos = s.substr(c1 + 1);
    const size_t d1 = pos.find('-');
    if (d1 == std::string::npos || pos.find('-', d1 + 1) != std::string::npos) { err = "Region must be in the format 'chr:start-end'."; return false; }
    int rs = pgh::parse_py_int(std::string_view(pos).substr(0, d1), r.start), re = pgh::parse_py_int(std::string_view(pos).substr(d1 + 1), r.end);
    if (rs == 1 || re == 1) { err = "Region must be in the format 'chr:start-end'."; return false; }
    if (rs == 2 || re == 2) { err = "region coordinates of magnitude 2^62 or more are not supported"; return false; }
    r.chrom = s.substr(0, c1);
    return true;
}

struct Loaded {
    pgh::AlnFile file;
    std::vector<uint32_t> order;                       // dict insertion order: index of the record that currently wins
    std::unordered_map<std::string_view, uint32_t> at; // name -> position in order
};

// load_file_to_dict (:157-190)
bool load_dict(const std::string &path, const Region *region, Loaded &L, std::string &err) {
    unsigned hw = std::thread::hardware_concurrency();
    if (!L.file.load(path, hw ? hw : 1, err)) { err = path + ": " + err; return false; }
    int32_t tid = -1;
    if (region) {
        for (size_t i = 0; i < L.file.refs.size(); i++) if (L.file.refs[i] == region->chrom) { tid = (int32_t)i; break; }
        if (tid < 0) { err = "invalid contig `" + region->chrom + "`"; return false; }
        if (region->start < 0) { err = "start out of range (" + std::to_string(region->start) + ")"; return false; }
        if (region->start > region->end) { err = "invalid coordinates: start (" + std::to_string(region->start) + ") > stop (" + std::to_string(region->end) + ")"; return false; }
    }
    L.at.reserve(L.file.recs.size());
    for (uint32_t i = 0; i < L.file.recs.size(); i++) {
        const pgh::AlnRec &r = L.file.recs[i];
        if (region && (r.tid != tid || r.pos >= region->end || r.endpos <= region->start)) continue;
        if (r.flag & 0x110) continue; // secondary or reverse
        if (!r.has_ss || !r.ss_is_z) { err = "'ss' tag not found (as a Z string) in record with read ID " + std::string(r.name); return false; }
        if (!r.has_si || !r.si_is_z) { err = "'si' tag not found (as a Z string) in record with read ID " + std::string(r.name); return false; }
        auto it = L.at.find(r.name);
        if (it == L.at.end()) { L.at.emplace(r.name, (uint32_t)L.order.size()); L.order.push_back(i); }
        else L.order[it->second] = i;
    }
    return true;
}

// si -> (si[0], si[2]); 0 ok, else an error message
bool parse_si(std::string_view si, int64_t &sig0, int64_t &ref0, std::string &err) {
    int64_t f[3] = {0, 0, 0};
    size_t n = 0, a = 0;
    while (true) {
        const size_t c = si.find(',', a);
        const std::string_view field = si.substr(a, c == std::string_view::npos ? std::string_view::npos : c - a);
        for (unsigned char ch : field) if (ch >= 0x80) { err = "si holds a byte outside ASCII (not supported)"; return false; }
        int64_t v = 0;
        const int rc = pgh::parse_py_int(field, v);
        if (rc == 1) { err = "invalid literal for int() with base 10: '" + std::string(field) + "' in si"; return false; }
        if (rc == 2) { err = "si value " + std::string(field) + " has a magnitude of 2^62 or more (not supported)"; return false; }
        if (n < 3) f[n] = v;
        n++;
        if (c == std::string_view::npos) break;
        a = c + 1;
    }
    if (n < 4) { err = "si has fewer than 4 fields (tuple index out of range)"; return false; }
    sig0 = f[0]; ref0 = f[2];
    return true;
}

bool parse_int_opt(const char *name, const std::string &v, int64_t &out, std::string &err) {
    const int rc = pgh::parse_py_int(v, out);
    if (rc == 1) { err = std::string("argument --") + name + ": invalid int value: '" + v + "'"; return false; }
    if (rc == 2) { err = std::string("argument --") + name + ": magnitudes of 2^62 or more are not supported"; return false; }
    return true;
}

} // namespace

int f1_score_main(int argc, char **argv) {
    int64_t read_limit = 100, base_shift = 0, threshold = 0;
    std::string read_id, region_s;
    bool rna = false;
    std::vector<std::string> pos;
    bool only_pos = false;
    auto is_negative_number = [](const std::string &a) { // argparse's _negative_number_matcher: ^-\d+$|^-\d*\.\d+$
        if (a.size() < 2 || a[0] != '-') return false;
        size_t i = 1; while (i < a.size() && isdigit((unsigned char)a[i])) i++;
        if (i == a.size()) return true;
        if (a[i] != '.') return false;
        size_t j = i + 1; while (j < a.size() && isdigit((unsigned char)a[j])) j++;
        return j == a.size() && j > i + 1;
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (only_pos || a == "-" || a.empty() || a[0] != '-' || is_negative_number(a)) { pos.push_back(a); continue; }
        if (a == "--") { only_pos = true; continue; }
        if (a == "-h" || a == "--help") { print_help(); return 0; }
        std::string name = a, val;
        bool has_val = false;
        const size_t eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) { name = a.substr(0, eq); val = a.substr(eq + 1); has_val = true; }
        std::string err;
        if (name == "--rna") {
            if (has_val) return usage_error("argument --rna: ignored explicit argument '" + val + "'");
            rna = true; continue;
        }
        static const char *kValued[] = {"--read_limit", "--base_shift", "--read_id", "--region", "--threshold"};
        bool known = false;
        for (const char *k : kValued) known |= name == k;
        if (!known) return usage_error("unrecognized arguments: " + a);
        if (!has_val) {
            // argparse takes the next word unless it looks like an option (a negative number does not)
            if (i + 1 >= argc || (argv[i + 1][0] == '-' && argv[i + 1][1] != 0 && !is_negative_number(argv[i + 1])))
                return usage_error("argument " + name + ": expected one argument");
            val = argv[++i];
        }
        if (name == "--read_id") read_id = val;
        else if (name == "--region") region_s = val;
        else if (!parse_int_opt(name.c_str() + 2, val, name == "--read_limit" ? read_limit : name == "--base_shift" ? base_shift : threshold, err))
            return usage_error(err);
    }
    if (pos.size() < 2) return usage_error("the following arguments are required: " + std::string(pos.empty() ? "bam1, bam2" : "bam2"));
    if (pos.size() > 2) {
        std::string extra;
        for (size_t i = 2; i < pos.size(); i++) extra += (i > 2 ? " " : "") + pos[i];
        return usage_error("unrecognized arguments: " + extra);
    }
    // --region and --read_id count only when non-empty (`if region:`, `if args.read_id and ...`)
    Region region;
    const bool use_region = !region_s.empty();
    std::string err;
    Loaded d1, d2;
    // load_file_to_dict(bam1) opens the file, then parses the region
    {
        FILE *fp = fopen(pos[0].c_str(), "rb");
        if (!fp) return fail("cannot open " + pos[0]);
        fclose(fp);
    }
    if (use_region && !parse_region(region_s, region, err)) return fail(err);
    if (!load_dict(pos[0], use_region ? &region : nullptr, d1, err)) return fail(err);
    if (!load_dict(pos[1], use_region ? &region : nullptr, d2, err)) return fail(err);

    // the compared pairs, in file 1's order, up to the first si that does not parse
    struct Pair { uint32_t r1, r2; int64_t sig[2], ref[2]; };
    std::vector<Pair> pairs;
    std::string host_err;
    uint64_t read_count = 0;
    for (uint32_t k = 0; k < d1.order.size(); k++) {
        const pgh::AlnRec &a = d1.file.recs[d1.order[k]];
        if (!read_id.empty() && a.name != read_id) continue;
        auto it = d2.at.find(a.name);
        if (it != d2.at.end()) {
            const uint32_t i2 = d2.order[it->second];
            const pgh::AlnRec &b = d2.file.recs[i2];
            Pair p{d1.order[k], i2, {0, 0}, {0, 0}};
            if (!parse_si(a.si, p.sig[0], p.ref[0], err) || !parse_si(b.si, p.sig[1], p.ref[1], err)) {
                host_err = "read " + std::string(a.name) + ": " + err;
                break;
            }
            p.ref[1] += base_shift;
            pairs.push_back(p);
        }
        read_count++;
        if (read_count == (uint64_t)read_limit && read_limit > 0) break;
    }

    // the device: every compared pair's two ss strings, packed in batches
    pg_fscore_params prm{};
    prm.rna = rna; prm.use_region = use_region; prm.threshold = threshold; prm.region_start = region.start; prm.region_end = region.end;
    pg_fscore *h = nullptr;
    pg_fscore_result res{};
    res.err_pair = -1;
    if (pairs.empty()) { // nothing to compare: the totals are zero (a failing si, if any, is reported below)
        if (!host_err.empty()) return fail(host_err);
    } else if (pg_fscore_create(&prm, 0, &h) != PG_OK) return fail(pg_fscore_last_error(nullptr));
    constexpr uint64_t kBatchBytes = 256ull << 20;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<int64_t> sig, ref;
    auto flush = [&]() -> pg_status {
        if (sig.empty()) return PG_OK;
        pg_fscore_batch b{};
        b.n_pairs = sig.size() / 2; b.location = PG_LOC_HOST; b.ss = bytes.data(); b.ss_off = off.data(); b.sig_start = sig.data(); b.first_ref = ref.data();
        const pg_status s = pg_fscore_submit(h, &b);
        bytes.clear(); off.assign(1, 0); sig.clear(); ref.clear();
        return s;
    };
    off.assign(1, 0);
    pg_status st = PG_OK;
    for (const Pair &p : pairs) {
        const pgh::AlnRec *r[2] = {&d1.file.recs[p.r1], &d2.file.recs[p.r2]};
        for (int side = 0; side < 2; side++) {
            bytes.insert(bytes.end(), r[side]->ss.begin(), r[side]->ss.end());
            off.push_back(bytes.size());
            sig.push_back(p.sig[side]); ref.push_back(p.ref[side]);
        }
        if (bytes.size() >= kBatchBytes && (st = flush()) != PG_OK) break;
    }
    if (h && st == PG_OK) st = flush();
    if (h && st == PG_OK) st = pg_fscore_finish(h, &res, nullptr, 0);
    const std::string dev_err = st != PG_OK ? pg_fscore_last_error(h) : "";
    if (h) pg_fscore_destroy(h);
    if (st == PG_ERR_INPUT && res.err_pair >= 0 && (uint64_t)res.err_pair < pairs.size()) {
        static const char *what[] = {"", "ss is empty (string index out of range)", "Invalid ss string. It should end with a non-numeric character.",
                                     "ss holds a byte outside ASCII (not supported)", "an ss op count of 2^32 or more (not supported)",
                                     "no signal point is mapped (list index out of range)"};
        const Pair &p = pairs[(size_t)res.err_pair];
        return fail("read " + std::string(d1.file.recs[p.r1].name) + ", file " + std::to_string(res.err_side + 1) + ": " +
                    (res.err_code < 6 ? what[res.err_code] : dev_err.c_str()));
    }
    if (st != PG_OK) return fail(dev_err);
    if (!host_err.empty()) return fail(host_err);

    const uint64_t TP = res.totals[0], FP = res.totals[1], TN = res.totals[2], FN = res.totals[3];
    auto ratio = [](uint64_t a, uint64_t b) { return b > 0 ? (double)a / (double)b : 0.0; };
    const double precision = ratio(TP, TP + FP), recall = ratio(TP, TP + FN);
    const double f1 = precision + recall > 0 ? 2 * (precision * recall) / (precision + recall) : 0.0;
    const double specificity = ratio(TN, TN + FP), accuracy = ratio(TP + TN, TP + FP + TN + FN);
    printf("TP\tFP\tTN\tFN\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\n", TP, FP, TN, FN);
    printf("precision\trecall\tF1_score\tspecificity\taccuracy\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\n", precision, recall, f1, specificity, accuracy);
    return 0;
}
