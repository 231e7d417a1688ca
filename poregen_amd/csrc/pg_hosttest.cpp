// pg_hosttest.cpp -- host-only build of the shared (host+device) arithmetic of libpgmove, so that the
// CPU test-suite can exercise exactly the code the kernels run (pg_select.h) without a GPU.
// Not part of the product path: nothing here is reachable from libpgmove's C ABI.
#include "pg_select.h"
#include <vector>
#include <cstdint>
#include <cstring>

extern "C" int pgt_plan(double dig, double off, double range, double pa_min, double pa_max, int32_t *out4) {
    PgReadPlan p = pg_make_plan(dig, off, range, pa_min, pa_max);
    out4[0] = p.c_lo; out4[1] = p.span; out4[2] = p.z0; out4[3] = p.status;
    return p.status;
}

// histogram + inclusive prefix on the host, then the shared selection
extern "C" int pgt_medmad(const int16_t *raw, uint64_t n, double dig, double off, double range,
                          double pa_min, double pa_max, double *med, double *mad, double *mad_raw) {
    PgReadPlan p = pg_make_plan(dig, off, range, pa_min, pa_max);
    if (p.status != 0) return p.status;
    std::vector<uint32_t> pre((size_t)(p.span > 0 ? p.span : 1), 0u);
    for (uint64_t i = 0; i < n; i++) {
        int idx = (int)raw[i] - p.c_lo;
        if (idx >= 0 && idx < p.span) pre[(size_t)idx]++;
    }
    for (int b = 1; b < p.span; b++) pre[(size_t)b] += pre[(size_t)b - 1];
    PgMedMad mm = pg_medmad_from_prefix(pre.data(), p, n, off, range / dig);
    *med = mm.med; *mad = mm.mad; *mad_raw = mm.mad_raw;
    return 0;
}

// the symmetric fast path of the selection alone: 1 = applicable (outputs set), 0 = the kernel would take the general path
extern "C" int pgt_medmad_sym(const int16_t *raw, uint64_t n, double dig, double off, double range,
                              double pa_min, double pa_max, double *med, double *mad, double *mad_raw) {
    PgReadPlan p = pg_make_plan(dig, off, range, pa_min, pa_max);
    if (p.status != 0) return p.status;
    std::vector<uint32_t> pre((size_t)(p.span > 0 ? p.span : 1), 0u);
    for (uint64_t i = 0; i < n; i++) {
        int idx = (int)raw[i] - p.c_lo;
        if (idx >= 0 && idx < p.span) pre[(size_t)idx]++;
    }
    for (int b = 1; b < p.span; b++) pre[(size_t)b] += pre[(size_t)b - 1];
    PgMedMad mm;
    if (!pg_medmad_sym(pre.data(), p, n, off, range / dig, mm)) return 0;
    *med = mm.med; *mad = mm.mad; *mad_raw = mm.mad_raw;
    return 1;
}

// the dense gathers' division (pg_select.h: pg_div_by_recip) next to the plain one: 1 = the two agree bit for bit
extern "C" int pgt_div_by_recip(double a, double b, double *q_recip, double *q_div) {
    const double y = 1.0 / b;
    *q_recip = pg_div_by_recip(a, b, y); *q_div = a / b;
    uint64_t x, z; memcpy(&x, q_recip, 8); memcpy(&z, q_div, 8);
    return x == z;
}
extern "C" int pgt_div_domain_ok(double offset, double scale) { return pg_div_domain_ok(offset, scale) ? 1 : 0; }

// ---- host parsers / writer of the CLI (poregen_amd/csrc/host) ------------------------------------------
#include "host/pg_host.h"
#include <cstring>
#include <string>

extern "C" size_t pgt_format_f8(double v, char *buf) { return pgh::format_f8(v, buf); }

// returns number of ops, or -1 on a "Bad ss" condition; fills up to cap entries
extern "C" long pgt_tokenize_ss(const char *ss, uint32_t *op_n, uint8_t *op_t, size_t cap) {
    std::vector<uint32_t> n; std::vector<uint8_t> t; std::string err;
    if (!pgh::tokenize_ss(ss, strlen(ss), n, t, err)) return -1;
    for (size_t i = 0; i < n.size() && i < cap; i++) { op_n[i] = n[i]; op_t[i] = t[i]; }
    return (long)n.size();
}

// fetch [beg,end] of `name`; returns length or -2 if the name is absent (htslib contract), -3 on I/O error
extern "C" long pgt_fastx_fetch(const char *path, const char *name, long beg, long end, char *out, size_t cap) {
    pgh::FastxIndex fx; std::string err, s;
    if (!fx.load(path, err)) return -3;
    if (!fx.fetch(name, beg, end, s)) return -2;
    if (s.size() < cap) { memcpy(out, s.data(), s.size()); out[s.size()] = 0; }
    return (long)s.size();
}

// decode one read of a SLOW5/BLOW5 file; returns len_raw_signal or -1; copies up to cap samples
extern "C" long pgt_slow5_get(const char *path, const char *read_id, double *dig_off_range, int16_t *raw, size_t cap) {
    pgh::Slow5File f; std::string err;
    if (!f.open(path, err)) return -1;
    pgh::Slow5Rec r;
    if (!f.get(read_id, r, err)) return -1;
    dig_off_range[0] = r.digitisation; dig_off_range[1] = r.offset; dig_off_range[2] = r.range;
    for (size_t i = 0; i < r.raw.size() && i < cap; i++) raw[i] = r.raw[i];
    return (long)r.raw.size();
}

extern "C" long pgt_slow5_count(const char *path) {
    pgh::Slow5File f; std::string err;
    if (!f.open(path, err)) return -1;
    return (long)f.n_reads();
}

extern "C" int pgt_parse_paf(char *line, int32_t *cols6, char *rid, char *tid, char *ss, size_t cap) {
    pgh::PafRec p;
    int rc = pgh::parse_paf_line(line, strlen(line), p);
    if (rc != 0) return rc;
    cols6[0] = p.qlen; cols6[1] = p.query_start; cols6[2] = p.query_end; cols6[3] = p.tlen; cols6[4] = p.target_start; cols6[5] = p.target_end;
    snprintf(rid, cap, "%s", p.rid.c_str()); snprintf(tid, cap, "%s", p.tid.c_str());
    if (p.ss_len < cap) { memcpy(ss, p.ss, p.ss_len); ss[p.ss_len] = 0; }
    return 0;
}

// first record of a SAM/BAM file: returns number of moves (mv entries after the stride) or -1; seq/qname copied
extern "C" long pgt_sam_first(const char *path, char *qname, char *seq, size_t cap, long long *stride_ns_ts, uint8_t *is_one, size_t mcap) {
    pgh::SamBamReader r; std::string err;
    if (!r.open(path, err)) return -1;
    pgh::MoveRec m;
    if (r.next(m, err) != 1) return -1;
    snprintf(qname, cap, "%s", m.qname.c_str()); snprintf(seq, cap, "%s", m.seq.c_str());
    stride_ns_ts[0] = m.stride; stride_ns_ts[1] = m.has_ns ? (long long)m.ns : -1; stride_ns_ts[2] = m.has_ts ? (long long)m.ts : -1;
    const long n_moves = (long)m.is_one.size();
    for (size_t i = 0; i < m.is_one.size() && i < mcap; i++) is_one[i] = m.is_one[i];
    pgh::MoveRec m2;
    if (r.next(m2, err) != 0) return -2; // the fixtures hold exactly one record
    return n_moves;
}

// pg_model.h: the fixed-point view of a "%.8f" print-out, and the host-side finishing arithmetic on hand-made moments
#include "pg_model.h"
#include <algorithm>
#include <cstdio>
extern "C" long long pgt_fixed8(double x, int *bad) { bool b = false; const long long v = pg_fixed8(x, b); *bad = b; return v; }
// values given as 1e-8 units: median text and sstdev text the library would print (same arithmetic as pg_model_format)
extern "C" void pgt_model_texts(const long long *units, size_t n, char *med, char *sd, size_t cap) {
    std::vector<long long> v(units, units + n);
    PgSlotModel m{};
    m.n = n; m.origin = n ? v[0] : 0;
    for (size_t i = 0; i < n; i++) {
        const long long d = v[i] - m.origin; const unsigned long long ad = (unsigned long long)(d < 0 ? -d : d);
        const unsigned long long h = ad >> PG_MODEL_LIMB_BITS, l = ad & ((1u << PG_MODEL_LIMB_BITS) - 1);
        m.s1 += d; m.s2_hh += h * h; m.s2_hl += h * l; m.s2_ll += l * l;
    }
    std::sort(v.begin(), v.end());
    if (n) { m.mid_lo = v[(n - 1) / 2]; m.mid_hi = v[n / 2]; }
    med[0] = sd[0] = 0;
    if (!n) return;
    snprintf(med, cap, "%.14Lg", pg_model_median(m));
    if (n < 2) snprintf(sd, cap, "nan");
    else {
        const unsigned __int128 s2 = ((unsigned __int128)m.s2_hh << 40) + ((unsigned __int128)m.s2_hl << 21) + m.s2_ll;
        const __int128 s1 = m.s1;
        pg_model_sstdev_text(n, (unsigned __int128)n * s2 - (unsigned __int128)(s1 * s1), sd, cap);
    }
}
// the sstdev text of n values whose n * sum d^2 - (sum d)^2 is num (given as two 64-bit halves), and -- for comparison -- the plain
// "%.14Lg" of the long double square root
extern "C" void pgt_sstdev_text(unsigned long long n, unsigned long long num_hi, unsigned long long num_lo, char *exact, char *plain, size_t cap) {
    const unsigned __int128 num = ((unsigned __int128)num_hi << 64) | num_lo;
    pg_model_sstdev_text(n, num, exact, cap);
    snprintf(plain, cap, "%.14Lg", sqrtl((long double)num / ((long double)n * (long double)(n - 1))) / 1e8L);
}

// ---- pg_hostmem.h: does a big SampleVec really ask for transparent huge pages? -------------------------------------------------
#include "pg_hostmem.h"
#include <fstream>
#include <sstream>
// 1 = the mapping that holds a SampleVec of n doubles carries the "hg" VmFlag (madvise(MADV_HUGEPAGE) took effect), 0 = it does not,
// -1 = /proc/self/smaps could not be read. anon_huge_kb (may be null): the mapping's AnonHugePages after a first touch.
extern "C" int pgt_samplevec_hugepage(size_t n, long *anon_huge_kb) {
    SampleVec v;
    v.resize(n);
    for (size_t i = 0; i < n; i += 512) v[i] = 1.0; // first touch
    const uintptr_t p = reinterpret_cast<uintptr_t>(v.data());
    std::ifstream f("/proc/self/smaps");
    if (!f) return -1;
    std::string line; bool inside = false; int hg = 0; long ahp = 0;
    while (std::getline(f, line)) {
        unsigned long a = 0, b = 0;
        if (sscanf(line.c_str(), "%lx-%lx ", &a, &b) == 2) { inside = p >= a && p < b; continue; } /* a mapping's header line */
        if (!inside) continue;
        if (line.rfind("AnonHugePages:", 0) == 0) ahp = atol(line.c_str() + 14);
        if (line.rfind("VmFlags:", 0) == 0) { std::istringstream is(line.substr(8)); std::string t; while (is >> t) if (t == "hg") hg = 1; }
    }
    if (anon_huge_kb) *anon_huge_kb = ahp;
    return hg;
}

// ---- corrupt-input probes (tests/test_host_corrupt.py): every read of a SLOW5/BLOW5 file / every record of a SAM/BAM file is decoded;
// returns the number decoded, or -1 with the reader's message in errbuf -- never a crash
static void put_err(const std::string &e, char *errbuf, size_t cap) { if (errbuf && cap) { const size_t n = e.size() < cap - 1 ? e.size() : cap - 1; memcpy(errbuf, e.data(), n); errbuf[n] = 0; } }
extern "C" long pgt_slow5_scan(const char *path, char *errbuf, size_t cap) {
    pgh::Slow5File f; std::string err;
    if (!f.open(path, err)) { put_err(err, errbuf, cap); return -1; }
    long n = 0;
    for (const std::string &id : f.ids_in_file_order()) {
        pgh::Slow5Rec r;
        if (!f.get(id, r, err)) { put_err(err, errbuf, cap); return -1; }
        ++n;
    }
    return n;
}
extern "C" long pgt_sambam_scan(const char *path, char *errbuf, size_t cap) {
    pgh::SamBamReader rd; std::string err;
    if (!rd.open(path, err)) { put_err(err, errbuf, cap); return -1; }
    long n = 0;
    for (;;) {
        pgh::MoveRec m;
        const int rc = rd.next(m, err);
        if (rc < 0) { put_err(err, errbuf, cap); return -1; }
        if (rc == 0) break;
        ++n;
    }
    return n;
}

// the placement of a rank's statistics relative to the count exchange (pg_job_rule.h): 1 = behind the wait, 0 = in front of it
#include "pg_job_rule.h"
extern "C" int pgt_job_stats_rule(uint32_t rank, const uint64_t *shard_ops, const uint64_t *shard_reads, uint32_t n_slots, uint64_t sample_limit,
                                  int have_batch, uint64_t full_slots_prev, const char *mode) {
    return (int)pg_job_stats_place(rank, shard_ops, shard_reads, n_slots, sample_limit, have_batch != 0, full_slots_prev, mode && *mode ? mode : nullptr);
}

// where a batch's per-read statistics run (pg_stats_plan.h): out6 = place, behind_cut, one_stream_batch, records_in_init, flags_in_init, rare_with_scan
#include "pg_stats_plan.h"
extern "C" void pgt_stats_plan(uint32_t ctx_flags, int32_t scaling, uint32_t front_tiles, uint32_t n_reads, int front_two_streams, int32_t *out6) {
    const PgStatsPlan p = pg_stats_plan(ctx_flags, scaling, front_tiles, n_reads, front_two_streams != 0);
    out6[0] = p.place; out6[1] = p.behind_cut; out6[2] = p.one_stream_batch; out6[3] = p.records_in_init; out6[4] = p.flags_in_init; out6[5] = p.rare_with_scan;
}
// PgStatsPlan::with_emit alone, with the switch (PGMOVE_NO_EMIT_STATS) that pgt_stats_plan's signature has no room for
extern "C" int pgt_stats_plan_with_emit(uint32_t ctx_flags, int32_t scaling, uint32_t front_tiles, uint32_t n_reads, int front_two_streams, int no_emit_stats) {
    return pg_stats_plan(ctx_flags, scaling, front_tiles, n_reads, front_two_streams != 0, no_emit_stats != 0).with_emit ? 1 : 0;
}
extern "C" int pgt_stats_fork_waits(int batch_is_host, int user_stream, int batch_resident, int prev_one_stream) {
    return pg_stats_fork_waits(batch_is_host != 0, user_stream != 0, batch_resident != 0, prev_one_stream != 0) ? 1 : 0;
}

// ---- subtool0 / pa_stats (pg_pamean.h, host/io.cpp) ----------------------------------------------------------------------------
#include "pg_pamean.h"
extern "C" int pgt_pa_shift(double offset) { return pg_pa_shift(offset); }
// the device's decision for one read, from the integer moments it counts: 1 = settled (*mean set)
extern "C" int pgt_pa_certify(uint64_t n, int64_t s1, uint64_t sa, double offset, double scale, double *mean) {
    return pg_pa_certify(n, s1, sa, pg_pa_shift(offset), offset, scale, mean);
}
extern "C" double pgt_pa_sequential_mean(const int16_t *raw, uint64_t n, double dig, double off, double range) {
    return pg_pa_sequential_mean(raw, n, dig, off, range);
}
// the file-order walk: record count, or -1 (errbuf); ids joined by '\n' into ids (cap bytes), sample counts into lens (up to max)
extern "C" long pgt_slow5_walk(const char *path, char *ids, size_t cap, uint64_t *lens, size_t max, char *errbuf, size_t ecap) {
    pgh::Slow5File f; std::string err, all;
    if (!f.open_walk(path, err)) { put_err(err, errbuf, ecap); return -1; }
    for (size_t i = 0; i < f.n_records(); i++) {
        std::string id; pgh::Slow5Rec r;
        if (!f.record(i, id, r, err)) { put_err(err, errbuf, ecap); return -1; }
        all += id; all += '\n';
        if (i < max) lens[i] = r.raw.size();
    }
    if (all.size() < cap) { memcpy(ids, all.data(), all.size()); ids[all.size()] = 0; }
    return (long)f.n_records();
}

// ---- svb-zd blocks (pg_svb.h): the checks the host makes before a block reaches the device, and the walk that hands the blocks over --
#include "pg_svb.h"
extern "C" int pgt_svb_check(uint64_t len, uint32_t count) { return pg_svb_check(len, count); }
extern "C" uint64_t pgt_svb_nctrl(uint32_t count) { return pg_svb_nctrl(count); }
extern "C" void pgt_svb_levels(uint32_t *out3) { out3[0] = PG_SVB_LANE_VALUES; out3[1] = PG_SVB_WAVE_VALUES; out3[2] = PG_SVB_PIECE_VALUES; }
// record count, or -1 (errbuf: "record <i>: <message>"); counts and block lengths of up to max records, the blocks back to back in blocks
extern "C" long pgt_slow5_svb_walk(const char *path, uint32_t *counts, uint64_t *lens, size_t max, uint8_t *blocks, size_t cap, char *errbuf, size_t ecap) {
    pgh::Slow5File f; std::string err;
    if (!f.open_walk(path, err)) { put_err(err, errbuf, ecap); return -1; }
    if (!f.has_svb_views()) { put_err("no svb-zd signals", errbuf, ecap); return -1; }
    size_t at = 0;
    for (size_t i = 0; i < f.n_records(); i++) {
        std::string id; pgh::Slow5File::SvbView v; std::vector<unsigned char> inflated;
        if (!f.record_svb(i, id, v, inflated, err)) { put_err("record " + std::to_string(i) + ": " + err, errbuf, ecap); return -1; }
        if (i < max) { counts[i] = v.count; lens[i] = v.len; }
        if (at + v.len <= cap) memcpy(blocks + at, v.block, v.len);
        at += v.len;
    }
    return (long)f.n_records();
}

// ---- poregen model (pg_dumphost.h, host/pg_dumpdir.h): the host path of a dump file and the directory listing / merging ------------
#include "pg_dumphost.h"
#include "host/pg_dumpdir.h"
// the raw model lines (which = 0, stddev capped at `limit`) or the dwell lines (which = 1) of the directories' logical files, all of them
// finished by the host path; returns the length (the text is cut at cap - 1), or -1 with the message in errbuf
extern "C" long pgt_dump_model_host(const char *const *dirs, size_t n_dirs, int which, const char *limit, int keep_first, int n_threads,
                                    char *out, size_t cap, char *errbuf, size_t ecap) {
    pgh::DumpSet ds; std::string err, text;
    if (!pgh::list_dump_dirs(std::vector<std::string>(dirs, dirs + n_dirs), n_threads, ds, err)) { put_err(err, errbuf, ecap); return -1; }
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    if (!pgh::read_dump_files(ds, 0, ds.names.size(), n_threads, bytes, off, err)) { put_err(err, errbuf, ecap); return -1; }
    for (size_t i = 0; i < ds.names.size(); i++) {
        const char *b = reinterpret_cast<const char *>(bytes.data()) + off[i];
        const size_t len = off[i + 1] - off[i];
        text += ds.names[i]; text += '\t';
        if (which == 0) {
            PgDumpHostStats hs;
            pg_dump_host_stats(b, len, keep_first != 0, hs);
            text += hs.median; text += '\t'; text += pg_dump_sd_capped(hs.sstdev.c_str(), limit) ? std::string(limit) : hs.sstdev;
        } else {
            PgDumpHostDwell hd;
            pg_dump_host_dwell(b, len, hd);
            char t[64]; t[0] = 0;
            if (hd.n) snprintf(t, sizeof t, "%.14Lg", ((long double)hd.mid_lo + (long double)hd.mid_hi) / 2.0L);
            text += t;
        }
        text += '\n';
    }
    if (out && cap) { const size_t n = text.size() < cap - 1 ? text.size() : cap - 1; memcpy(out, text.data(), n); out[n] = 0; }
    return (long)text.size();
}

// ---- kmer_freq on SAM/BAM input (pg_kfreq_codes.h): the 4-bit code htslib packs for a byte of SEQ, a code's letter and its complement --
#include "pg_kfreq_codes.h"
extern "C" int pgt_kf_code_of_byte(int byte) { return (int)pg_kf_code_of_byte((uint32_t)byte & 0xff); }
extern "C" int pgt_kf_letter(int code) { return (int)pg_kf_letter((uint32_t)code & 15); }
extern "C" int pgt_kf_complement(int code) { return (int)pg_kf_complement((uint32_t)code & 15); }

// ---- kmer_freq on FASTA input (pg_kfreq_fasta.h): the kernels' decomposition on the host -- a unit's tiles summarised span by span as
// k_kf_fa_lines does, then every span walked from the state k_kf_fa_count derives for it (tile summaries across tiles, span summaries
// inside one), the carried state handed from unit to unit. Only the order differs: one thread after the other instead of a scan.
#include "pg_kfreq_fasta.h"
#include <map>
namespace {
constexpr uint64_t kFaTile = (uint64_t)kFaSpan * kFaTileSpans;
struct FaHostSink {
    uint32_t k; std::map<uint32_t, uint64_t> *hist; std::map<std::string, uint64_t> *odd_map;
    void dense(uint32_t code) { (*hist)[code]++; }
    void odd(uint64_t lo, uint32_t hi) {
        std::string key(k, '\0');
        for (uint32_t i = 0; i < k; i++) { const uint32_t sh = k - 1 - i; key[i] = (char)(sh < 8 ? lo >> (8 * sh) : hi >> (8 * (sh - 8))); }
        (*odd_map)[key]++;
    }
};
struct FaHostLoad {
    const uint8_t *p; uint64_t base, n;
    void operator()(uint32_t ch, uint32_t (&ws)[4]) const {
        for (int i = 0; i < 4; i++) ws[i] = 0;
        for (uint32_t b = 0; b < 16; b++) { const uint64_t o = base + 16 * ch + b; if (o < n) ws[b >> 2] |= (uint32_t)p[o] << (8 * (b & 3)); }
    }
};
struct FaHostState { uint32_t kind; PgFaSum rec; };
uint32_t fa_host_span(const uint8_t *p, uint64_t base, uint64_t n, PgFaSpan &sp) { // returns the span's first byte
    uint32_t w[kFaSpan / 4];
    FaHostLoad load{p, base, n};
    for (uint32_t ch = 0; ch < kFaSpan / 16; ch++) { uint32_t ws[4]; load(ch, ws); for (int i = 0; i < 4; i++) w[4 * ch + i] = ws[i]; }
    pg_fa_span_summary(w, (uint32_t)std::min<uint64_t>(kFaSpan, n - base), sp);
    return w[0] & 0xff;
}
bool fa_host_unit(const uint8_t *p, uint64_t n, uint32_t k, FaHostState &st, FaHostSink &sink) {
    const uint64_t n_tiles = (n + kFaTile - 1) / kFaTile;
    std::vector<uint64_t> tile_ls(n_tiles, 0);
    std::vector<PgFaSum> tile_fa(n_tiles), tile_pb(n_tiles);
    for (uint64_t t = 0; t < n_tiles; t++) { // k_kf_fa_lines
        const uint64_t tile0 = t * kFaTile, tile_end = std::min<uint64_t>(n, tile0 + kFaTile);
        uint64_t ls = 0, fa_end = tile_end;
        PgFaSum rest = pg_fa_empty();
        for (uint64_t base = tile0; base < tile_end; base += kFaSpan) {
            PgFaSpan sp;
            const uint32_t first_byte = fa_host_span(p, base, n, sp);
            rest = pg_fa_compose(rest, ls ? pg_fa_resolve(pg_fa_kind_at(p, ls, base, PG_FA_SEQ), first_byte, sp.fa, sp.pb) : sp.pb);
            if (sp.has_nl) {
                if (!ls) { fa_end = base; while (p[fa_end] != '\n') fa_end++; }
                ls = base + sp.last_nl + 1;
            }
        }
        PgFaSum f = pg_fa_empty();
        for (uint64_t q = fa_end - tile0 > kFaTail ? fa_end - kFaTail : tile0; q < fa_end; q++) pg_fa_append(f, p[q]);
        tile_ls[t] = ls; tile_fa[t] = f; tile_pb[t] = rest;
    }
    bool bad = false;
    uint64_t line_in = 0;
    PgFaSum rec_in = st.rec;
    for (uint64_t t = 0; t < n_tiles; t++) { // k_kf_fa_count, block t
        const uint64_t tile0 = t * kFaTile, tile_end = std::min<uint64_t>(n, tile0 + kFaTile);
        uint64_t ls = line_in;
        PgFaSum rec = rec_in;
        for (uint64_t base = tile0; base < tile_end; base += kFaSpan) {
            PgFaSpan sp;
            const uint32_t first_byte = fa_host_span(p, base, n, sp);
            const uint32_t kind = pg_fa_kind_at(p, ls, base, st.kind);
            FaHostLoad load{p, base, n};
            bad |= pg_fa_walk(load, (uint32_t)std::min<uint64_t>(kFaSpan, n - base), k, kind, rec, sink);
            rec = pg_fa_compose(rec, pg_fa_resolve(kind, first_byte, sp.fa, sp.pb));
            if (sp.has_nl) ls = base + sp.last_nl + 1;
        }
        // what the next block folds from the tile summaries
        rec_in = pg_fa_compose(rec_in, pg_fa_resolve(pg_fa_kind_at(p, line_in, tile0, st.kind), p[tile0], tile_fa[t], tile_pb[t]));
        line_in = std::max(line_in, tile_ls[t]);
    }
    st.kind = pg_fa_kind_at(p, line_in, n, st.kind);
    st.rec = rec_in;
    return bad;
}
} // namespace
// The FASTA form on data[0, n) delivered in pieces that end at cuts[0] <= cuts[1] <= ... (the last one at n), each piece cut into units of
// at most `unit` bytes. The ACGT keys met, ascending: codes into dense_codes, counts into dense_counts, up to dense_cap, their number into
// *n_dense. The odd keys in byte order: k bytes each into odd_keys, counts into odd_counts, up to odd_cap. Returns the number of odd keys;
// *nul = a sequence line holds a NUL byte.
extern "C" long pgt_kf_fasta(const uint8_t *data, uint64_t n, const uint64_t *cuts, size_t n_cuts, uint32_t k, uint64_t unit,
                             uint32_t *dense_codes, uint64_t *dense_counts, size_t dense_cap, uint8_t *odd_keys, uint64_t *odd_counts,
                             size_t *n_dense, size_t odd_cap, int *nul) {
    std::map<uint32_t, uint64_t> hist;
    std::map<std::string, uint64_t> odd;
    FaHostSink sink{k, &hist, &odd};
    FaHostState st{PG_FA_FRESH, pg_fa_empty()};
    bool bad = false;
    uint64_t at = 0;
    for (size_t c = 0; c < n_cuts; c++) {
        const uint64_t end = std::min<uint64_t>(cuts[c], n);
        while (at < end) {
            const uint64_t m = std::min<uint64_t>(unit, end - at);
            const std::vector<uint8_t> u(data + at, data + at + m); // a buffer of its own: nothing outside the unit can be read unnoticed
            bad |= fa_host_unit(u.data(), m, k, st, sink);
            at += m;
        }
    }
    size_t i = 0;
    for (const auto &kv : hist) {
        if (i < dense_cap) { dense_codes[i] = kv.first; dense_counts[i] = kv.second; }
        i++;
    }
    *n_dense = i;
    i = 0;
    for (const auto &kv : odd) {
        if (i < odd_cap) { memcpy(odd_keys + i * k, kv.first.data(), k); odd_counts[i] = kv.second; }
        i++;
    }
    *nul = bad;
    return (long)i;
}

// ---- kmer_freq on FASTQ input (pg_kfreq_text.h): the kernels' decomposition on the host -- a unit's newlines counted per tile as k_kf_lines
// does, then every span of every tile walked from the line index k_kf_count derives for it (the carried state, the tiles in front, the
// spans in front inside the tile), then the seam and the next unit's state, which workgroup 0 forms. One thread after the other.
#include "pg_kfreq_text.h"
namespace {
struct KfHostSink {
    uint32_t k; std::map<uint32_t, uint64_t> *hist; std::map<std::string, uint64_t> *odd_map;
    void dense(uint32_t code) { (*hist)[code]++; }
    void odd(uint64_t lo, uint32_t hi) {
        uint32_t key[4];
        pg_kf_odd_key(lo, hi, k, key);
        std::string s(k, '\0');
        for (uint32_t i = 0; i < k; i++) s[i] = (char)(key[i >> 2] >> (8 * (i & 3)));
        (*odd_map)[s]++;
    }
};
uint32_t kf_host_newlines(const uint8_t *p, uint64_t from, uint64_t to) {
    uint32_t c = 0;
    for (uint64_t q = from; q < to; q++) c += p[q] == '\n';
    return c;
}
bool kf_host_unit(const uint8_t *p, uint64_t n, uint32_t k, KfState &st, KfHostSink &sink) {
    const uint32_t n_tiles = (uint32_t)((n + PG_KF_TILE - 1) / PG_KF_TILE);
    std::vector<uint32_t> tile_nl(n_tiles);
    for (uint32_t t = 0; t < n_tiles; t++) tile_nl[t] = kf_host_newlines(p, t * PG_KF_TILE, std::min<uint64_t>(n, (t + 1) * PG_KF_TILE)); // k_kf_lines
    bool bad = false;
    uint32_t total_nl = 0;
    for (uint32_t blk = 0; blk < n_tiles; blk++) { // k_kf_count, block blk
        const uint32_t upto = blk == 0 ? n_tiles : blk;
        uint32_t tile_pre = 0;
        for (uint32_t tid = 0; tid < PG_KF_THREADS; tid++)
            for (uint32_t i = tid; i < upto; i += PG_KF_THREADS) tile_pre += tile_nl[i];
        if (blk == 0) { total_nl = tile_pre; tile_pre = 0; }
        uint32_t excl = 0; // newlines of the spans in front, inside the tile
        for (uint32_t tid = 0; tid < PG_KF_THREADS; tid++) {
            const uint64_t base = blk * PG_KF_TILE + tid * (uint64_t)PG_KF_SPAN;
            if (base >= n) break;
            FaHostLoad load{p, base, n};
            bad |= pg_kf_walk(p, base, n, k, (st.mod4 + tile_pre + excl) & 3, load, sink);
            excl += kf_host_newlines(p, base, std::min<uint64_t>(n, base + PG_KF_SPAN));
        }
    }
    st = pg_kf_seam(st, p, n, k, total_nl, sink); // block 0, thread 0
    return bad;
}
} // namespace
extern "C" void pgt_kfreq_levels(uint64_t *out6) {
    out6[0] = PG_KF_SPAN; out6[1] = PG_KF_TILE; out6[2] = PG_KF_UNIT; out6[3] = PG_KF_MAX_K; out6[4] = PG_KF_LDS_MAX_K; out6[5] = PG_KF_ODD_LDS;
}
// The FASTQ form on data[0, n), pieces, units and outputs as for pgt_kf_fasta. The window that ends on the stream's last byte is never
// settled, as in pg_kfreq_finish. *nul = a sequence line holds a NUL byte.
extern "C" long pgt_kf_text(const uint8_t *data, uint64_t n, const uint64_t *cuts, size_t n_cuts, uint32_t k, uint64_t unit,
                            uint32_t *dense_codes, uint64_t *dense_counts, size_t dense_cap, uint8_t *odd_keys, uint64_t *odd_counts,
                            size_t *n_dense, size_t odd_cap, int *nul) {
    std::map<uint32_t, uint64_t> hist;
    std::map<std::string, uint64_t> odd;
    KfHostSink sink{k, &hist, &odd};
    KfState st{};
    bool bad = false;
    uint64_t at = 0;
    for (size_t c = 0; c < n_cuts; c++) {
        const uint64_t end = std::min<uint64_t>(cuts[c], n);
        while (at < end) {
            const uint64_t m = std::min<uint64_t>(unit, end - at);
            const std::vector<uint8_t> u(data + at, data + at + m); // a buffer of its own: nothing outside the unit can be read unnoticed
            bad |= kf_host_unit(u.data(), m, k, st, sink);
            at += m;
        }
    }
    size_t i = 0;
    for (const auto &kv : hist) {
        if (i < dense_cap) { dense_codes[i] = kv.first; dense_counts[i] = kv.second; }
        i++;
    }
    *n_dense = i;
    i = 0;
    for (const auto &kv : odd) {
        if (i < odd_cap) { memcpy(odd_keys + i * k, kv.first.data(), k); odd_counts[i] = kv.second; }
        i++;
    }
    *nul = bad;
    return (long)i;
}

// ---- move-table expansion: the per-read rule the kernels of pg_mvops.hip compile (pg_mvops.h), run on the host ----------------------
#include "pg_mvops.h"
extern "C" void pgt_mvops_levels(uint32_t *out3) { out3[0] = PG_MVOPS_LANE; out3[1] = PG_MVOPS_STEP; out3[2] = PG_MVOPS_PIECE; }
extern "C" int pgt_mvops_mask4(uint32_t w) { return (int)pg_mv_mask4(w); }
extern "C" int pgt_mvops_expand(const uint8_t *mv, uint32_t n, int32_t stride, uint64_t ns, uint64_t ts, uint32_t l_seq, const uint8_t *packed, int reverse,
                                int n_to_t, uint32_t *ops, uint32_t *n_ops, int32_t *query_start, uint8_t *seq) {
    return (int)pg_mv_expand_host(mv, n, stride, ns, ts, l_seq, packed, reverse != 0, n_to_t != 0, ops, n_ops, query_start, seq);
}

// ---- ops through a CIGAR onto the reference: the per-read rule the kernels of pg_refops.hip compile (pg_refops.h), run on the host ------
#include "pg_refops.h"
// out8: status, n_ops, ref_len, n_match, query_start, query_end, target_start, target_end; op_n / op_t have room for L + n_words values
extern "C" void pgt_refops(const uint32_t *o, uint32_t L, int32_t query_start, uint32_t status_in, const uint32_t *cigar, uint32_t n_words, int32_t pos, int rna,
                           uint32_t *op_n, uint8_t *op_t, int64_t *out8) {
    const PgRfHost h = pg_refops_host(o, L, query_start, status_in, cigar, n_words, pos, rna != 0, op_n, op_t);
    out8[0] = h.status; out8[1] = h.n_ops; out8[2] = h.ref_len; out8[3] = h.n_match; out8[4] = h.query_start; out8[5] = h.query_end; out8[6] = h.target_start; out8[7] = h.target_end;
}
// the same with the record's strand: reverse (flag 0x10) and the length of its contig
extern "C" void pgt_refops_strand(const uint32_t *o, uint32_t L, int32_t query_start, uint32_t status_in, const uint32_t *cigar, uint32_t n_words, int32_t pos, int rna,
                                  int reverse, int32_t contig_len, uint32_t *op_n, uint8_t *op_t, int64_t *out8) {
    const PgRfHost h = pg_refops_host(o, L, query_start, status_in, cigar, n_words, pos, rna != 0, op_n, op_t, reverse != 0, contig_len);
    out8[0] = h.status; out8[1] = h.n_ops; out8[2] = h.ref_len; out8[3] = h.n_match; out8[4] = h.query_start; out8[5] = h.query_end; out8[6] = h.target_start; out8[7] = h.target_end;
}

// ---- reference slices (pg_refseq.h): the clamp and the complement the kernels of pg_refseq.hip compile, run on the host -----------------
#include "pg_refseq.h"
// out2: the first base and the number of bases of the slice; contig_len < 0: no such contig
extern "C" void pgt_refseq_clamp(int32_t pos, uint32_t ref_len, int64_t contig_len, int64_t *out2) {
    const PgRsSpan sp = pg_rs_clamp(pos, ref_len, contig_len);
    out2[0] = sp.beg; out2[1] = sp.n;
}
extern "C" void pgt_refseq_complement(const uint8_t *in, uint8_t *out, uint64_t n) { for (uint64_t i = 0; i < n; i++) out[i] = pg_rs_complement(in[i]); }
// one read's slice of `contig`, as the copy kernel writes it; returns its length, or -1 where it would leave the contig or `cap`
extern "C" long pgt_refseq_slice(const uint8_t *contig, int64_t contig_len, int32_t pos, uint32_t ref_len, int reverse, uint8_t *out, uint64_t cap) {
    const PgRsSpan sp = pg_rs_clamp(pos, ref_len, contig_len);
    if (sp.n && (sp.beg < 0 || sp.beg + sp.n > contig_len || (uint64_t)sp.n > cap)) return -1;
    for (int64_t k = 0; k < sp.n; k++) out[k] = reverse ? pg_rs_complement(contig[sp.beg + sp.n - 1 - k]) : contig[sp.beg + k];
    return (long)sp.n;
}

// ---- the dump-text parser (pg_dumptext.h): the geometry of its kernels and the field rule they compile, run on the host ----------------
#include "pg_dumptext.h"
extern "C" void pgt_dumptext_levels(uint32_t *out4) { out4[0] = PG_DT_LANE; out4[1] = PG_DT_TILE; out4[2] = PG_DT_BLOCK; out4[3] = PG_DT_MIN_FIELD; }
// 1 = the field in front of the separator at p[sep] is one of the strict grammar (*units, *negzero set); lo = the first byte of its file
extern "C" int pgt_dumptext_field(const uint8_t *p, uint64_t sep, uint64_t lo, int64_t *units, int *negzero) {
    int64_t u = 0; bool nz = false;
    const bool ok = pg_dt_parse_field(p, sep, lo, u, nz);
    *units = u; *negzero = nz;
    return ok;
}

// ---- pools of dump files (pg_pool.h): the tile geometry of the selection and the exact combination of per-file moments ---------------
#include "pg_pool.h"
extern "C" void pgt_pool_levels(uint32_t *out4) { out4[0] = PG_POOL_TILE; out4[1] = PG_POOL_DIRECT; out4[2] = PG_POOL_THREADS; out4[3] = PG_POOL_MAX_LABELINGS; }
// members as (n, origin, s1, s2 lo / hi). out8: status, why, n, origin, s1, s2 lo, s2 hi, 0; num2: n * s2 - s1^2 lo, hi; sd: its sstdev text
extern "C" int pgt_pool_combine(size_t count, const uint64_t *n, const int64_t *origin, const int64_t *s1, const uint64_t *s2_lo, const uint64_t *s2_hi,
                                int drop_first, int64_t second, int64_t *out8, uint64_t *num2, char *sd, size_t cap) {
    std::vector<PgPoolMember> m(count);
    for (size_t i = 0; i < count; i++) m[i] = PgPoolMember{n[i], origin[i], s1[i], ((unsigned __int128)s2_hi[i] << 64) | s2_lo[i]};
    PgPoolMoments pm;
    pg_pool_combine(m.data(), count, drop_first != 0, second, pm);
    out8[0] = pm.status; out8[1] = pm.why; out8[2] = (int64_t)pm.n; out8[3] = pm.origin; out8[4] = pm.s1;
    out8[5] = (int64_t)(uint64_t)pm.s2; out8[6] = (int64_t)(uint64_t)(pm.s2 >> 64); out8[7] = 0;
    num2[0] = (uint64_t)pm.num; num2[1] = (uint64_t)(pm.num >> 64);
    sd[0] = 0;
    if (pm.status == PG_POOL_ST_OK) { if (pm.n < 2) snprintf(sd, cap, "nan"); else pg_model_sstdev_text(pm.n, pm.num, sd, cap); }
    return pm.status;
}

// ---- the event table (pg_evstat.h): the geometry of k_ev_stats and the rule for one event, run on the host ------------------------------
#include "pg_evstat.h"
extern "C" void pgt_evstat_levels(uint64_t *out5) { out5[0] = PG_EV_MAX_LEN; out5[1] = (uint64_t)PG_EV_MAX_DEV; out5[2] = PG_EV_LANE; out5[3] = PG_EV_TILE; out5[4] = PG_EV_BLOCK; }
// the refusal code (PG_EV_*) of the event units[0 .. n), n >= 1; *m and *s where they exist, else 0
extern "C" int pgt_evstat(const int64_t *units, uint64_t n, int64_t *m, int64_t *s) {
    *m = 0; *s = 0;
    PgEvSums sums{0, 0, 0};
    uint32_t code = n > PG_EV_MAX_LEN ? (uint32_t)PG_EV_TOO_LONG : 0u; // (the codes are bits: a long event may be a wide one too)
    for (uint64_t i = 0; i < n; i++) { const int64_t d = pg_ev_dev(units[i], units[0], code); if (n <= PG_EV_MAX_LEN) pg_ev_add(sums, d); }
    if (code) return (int)code;
    return (int)pg_ev_finish(units[0], n, sums, *m, *s);
}
// the same over events back to back: event e is units[off[e] .. off[e + 1])
extern "C" void pgt_evstat_many(const int64_t *units, const uint64_t *off, uint64_t n_events, int64_t *m, int64_t *s, int32_t *code) {
    for (uint64_t e = 0; e < n_events; e++) code[e] = pgt_evstat(units + off[e], off[e + 1] - off[e], m + e, s + e);
}

// ---- fit (pg_fit.h): the model parser, the walk of one read, the solve and the text rules, run on the host ------------------------------
#include "pg_fit.h"
extern "C" void pgt_fit_levels(uint64_t *out8) {
    out8[0] = PG_FIT_STEP; out8[1] = PG_FIT_PIECE; out8[2] = PG_FIT_THREADS; out8[3] = PG_FIT_LDS_K; out8[4] = PG_FIT_GRID; out8[5] = (uint64_t)PG_FIT_MAX_N;
    out8[6] = PG_FIT_MAX_LEVEL; out8[7] = (uint64_t)PG_FIT_CLAMP;
}
// 0 and k, levels (cap_slots entries), uses_u; or -1 with the reason in err
extern "C" int pgt_fit_parse_model(const char *text, size_t n, uint32_t want_k, uint32_t *k, uint32_t *levels, size_t cap_slots, int *uses_u, char *err, size_t ecap) {
    PgFitModel md; std::string why;
    if (!pg_fit_parse_model_text(text, n, want_k, md, why) || md.levels.size() > cap_slots) { snprintf(err, ecap, "%s", why.c_str()); return -1; }
    memcpy(levels, md.levels.data(), md.levels.size() * sizeof(uint32_t));
    *k = md.k; *uses_u = md.uses_u ? 1 : 0;
    return 0;
}
// the counted events of one read (first sample, samples, slot: up to cap of them) and its seven sums; -1: out_of_signal
extern "C" long pgt_fit_walk(const uint8_t *seq, uint32_t lb, const uint32_t *op_n, int64_t q, const int16_t *sig, uint64_t n_sig, const uint32_t *levels, uint32_t k, uint32_t m,
                             int rna, uint32_t min_dur, uint32_t max_dur, uint64_t *ev_start, uint32_t *ev_n, int32_t *ev_slot, size_t cap, int64_t *sums7) {
    std::vector<PgFitEvent> ev; PgFitSums s;
    if (!pg_fit_walk_host(seq, lb, op_n, q, sig, n_sig, levels, k, m, rna != 0, min_dur, max_dur, ev, s)) return -1;
    for (size_t i = 0; i < ev.size() && i < cap; i++) { ev_start[i] = ev[i].start; ev_n[i] = ev[i].n; ev_slot[i] = ev[i].slot; }
    memcpy(sums7, &s, sizeof s);
    return (long)ev.size();
}
// the same for a gapped read (seq: its slice of n_seq bases; op_t 0 match, 1 I, 2 D); -1: out_of_signal, -6: ref_length, -100: an op code
// above 2 or a slice above 2^32 - 1 bases
extern "C" long pgt_fit_walk_gapped(const uint8_t *seq, uint64_t n_seq, const uint32_t *op_n, const uint8_t *op_t, uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig,
                                    const uint32_t *levels, uint32_t k, uint32_t m, int rna, uint32_t min_dur, uint32_t max_dur, uint64_t *ev_start, uint32_t *ev_n, int32_t *ev_slot,
                                    size_t cap, int64_t *sums7) {
    std::vector<PgFitEvent> ev; PgFitSums s;
    const int st = pg_fit_gap_walk_host(seq, n_seq, op_n, op_t, lb, q, sig, n_sig, levels, k, m, rna != 0, min_dur, max_dur, ev, s);
    if (st < 0) return -100;
    if (st != PG_FIT_OK) return -(long)st;
    for (size_t i = 0; i < ev.size() && i < cap; i++) { ev_start[i] = ev[i].start; ev_n[i] = ev[i].n; ev_slot[i] = ev[i].slot; }
    memcpy(sums7, &s, sizeof s);
    return (long)ev.size();
}
// the status; a, b and 1 / b as they go to the device; shift, scale and rms as the per-read table prints them ("%.6f"), 64 bytes each
extern "C" int pgt_fit_solve(const int64_t *sums7, uint32_t min_events, double dig, double off, double range, double *ab3, char *text3) {
    PgFitSums s; memcpy(&s, sums7, sizeof s);
    const PgFitSolve v = pg_fit_solve(s, min_events);
    ab3[0] = v.a; ab3[1] = v.b; ab3[2] = v.inv_b;
    text3[0] = text3[64] = text3[128] = 0;
    if (v.status == PG_FIT_OK) {
        long double rep[3]; pg_fit_report(s, dig, off, range, rep);
        for (int i = 0; i < 3; i++) snprintf(text3 + 64 * i, 64, "%.6Lf", rep[i]);
    }
    return (int)v.status;
}
// the hand-written conversion of lo + 2^64 hi (two's complement) and, in native, the compiler's own
extern "C" double pgt_fit_i128_to_double(uint64_t lo, uint64_t hi, double *native) {
    const __int128 v = (__int128)(((unsigned __int128)hi << 64) | lo);
    if (native) *native = (double)v;
    return pg_fit_i128_to_double(v);
}
// pg_fit_solve_hd: the status; a, b and 1 / b; and the collector's center, spread (out5[3], out5[4]) and use by the rule of pg_fit.h
extern "C" int pgt_fit_solve_hd(const int64_t *sums7, uint32_t min_events, double dig, double off, double range, double *out5, int *use) {
    PgFitSums s; memcpy(&s, sums7, sizeof s);
    const PgFitSolve v = pg_fit_solve_hd(s, min_events);
    const PgFitScale sc = pg_fit_scale_rule(v.status, v.a, v.b, dig, off, range);
    out5[0] = v.a; out5[1] = v.b; out5[2] = v.inv_b; out5[3] = sc.center; out5[4] = sc.spread;
    if (use) *use = sc.use;
    return (int)v.status;
}
// the rule alone, for any status, a and b
extern "C" int pgt_fit_scale_rule(uint32_t status, double a, double b, double dig, double off, double range, double *out2) {
    const PgFitScale sc = pg_fit_scale_rule(status, a, b, dig, off, range);
    out2[0] = sc.center; out2[1] = sc.spread;
    return sc.use;
}
extern "C" int pgt_fit_resid(int r, double a, double inv_b, int l, int *clamped) { bool c; const int32_t d = pg_fit_resid(r, a, inv_b, l, c); *clamped = c; return d; }
// the two residual columns of a slot as the k-mer table prints them
extern "C" void pgt_fit_resid_text(uint64_t n, int64_t sum_d, uint64_t dd_lo, uint64_t dd_hi, char *mean, char *rms, size_t cap) {
    int64_t m, q; pg_fit_slot_resid(n, sum_d, dd_lo, dd_hi, m, q);
    snprintf(mean, cap, "%s", pg_fit_units_text(m).c_str()); snprintf(rms, cap, "%s", pg_fit_units_text(q).c_str());
}

// ---- realign (pg_realign.h): the rule for one fitted read, run on the host ------------------------------------------------------------------
#include "pg_realign.h"
extern "C" void pgt_realign_levels(uint64_t *out3) { out3[0] = PG_RL_MAX_BAND; out3[1] = PG_RL_MAX_DUR; out3[2] = PG_FIT_PIECE; }
extern "C" int pgt_realign_params_ok(uint32_t band, uint32_t min_len, uint32_t min_dur, uint32_t max_dur) { return pg_rl_params_ok(band, min_len, min_dur, max_dur) ? 1 : 0; }
// 0 and the refined ops (lb of them), out7 = n_free, n_moved, sum_abs_shift, cost_before lo / hi, cost_after lo / hi; -1: out_of_signal
extern "C" int pgt_realign_walk(const uint8_t *seq, uint32_t lb, const uint32_t *op_n, int64_t q, const int16_t *sig, uint64_t n_sig, const uint32_t *levels, uint32_t k, uint32_t m,
                                int rna, uint32_t min_dur, uint32_t max_dur, uint32_t band, uint32_t min_len, double a, double b, uint32_t *op_out, uint64_t *out7) {
    PgRlRead r;
    if (!pg_rl_walk_host(seq, lb, op_n, q, sig, n_sig, levels, k, m, rna != 0, min_dur, max_dur, band, min_len, 0, a, b, op_out, r)) return -1;
    out7[0] = r.n_free; out7[1] = r.n_moved; out7[2] = r.sum_abs_shift; out7[3] = (uint64_t)r.cost_before; out7[4] = (uint64_t)(r.cost_before >> 64);
    out7[5] = (uint64_t)r.cost_after; out7[6] = (uint64_t)(r.cost_after >> 64);
    return 0;
}
// the same for a gapped read, under a phase; -1: the read has no fit (out_of_signal, ref_length, an op code above 2)
extern "C" int pgt_realign_walk_gapped(const uint8_t *seq, uint64_t n_seq, const uint32_t *op_n, const uint8_t *op_t, uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig,
                                       const uint32_t *levels, uint32_t k, uint32_t m, int rna, uint32_t min_dur, uint32_t max_dur, uint32_t band, uint32_t min_len, uint32_t phase,
                                       double a, double b, uint32_t *op_out, uint64_t *out7) {
    static const uint8_t none = 0;
    PgRlRead r;
    if (!pg_rl_walk_any(seq, n_seq, lb ? op_t : &none, lb, op_n, q, sig, n_sig, levels, k, m, rna != 0, min_dur, max_dur, band, min_len, phase, a, b, op_out, r)) return -1;
    out7[0] = r.n_free; out7[1] = r.n_moved; out7[2] = r.sum_abs_shift; out7[3] = (uint64_t)r.cost_before; out7[4] = (uint64_t)(r.cost_before >> 64);
    out7[5] = (uint64_t)r.cost_after; out7[6] = (uint64_t)(r.cost_after >> 64);
    return 0;
}
// the pieces a read of lb ops is cut into under a phase: out[2 j] = first op, out[2 j + 1] = ops of piece j; returns their number (or -1: cap)
extern "C" long pgt_realign_pieces(uint32_t lb, uint32_t phase, uint32_t *out, size_t cap) {
    const uint64_t np = pg_rl_pieces(lb, phase);
    if (np > cap) return -1;
    for (uint32_t j = 0; j < np; j++) pg_rl_piece(lb, phase, j, out[2 * j], out[2 * j + 1]);
    return (long)np;
}

// ---- eventalign (pg_evalign.h): one event from its samples, the walk of one read, the text of a row ------------------------------------------
#include "pg_evalign.h"
extern "C" void pgt_evalign_levels(uint64_t *out3) { out3[0] = PG_EA_MAX_DUR; out3[1] = PG_EA_MAX_RATE; out3[2] = sizeof(PgEaRow); }
extern "C" int pgt_evalign_params_ok(uint32_t min_dur, uint32_t max_dur, uint32_t rate) { return pg_ea_params_ok(min_dur, max_dur, rate) ? 1 : 0; }
// one event of n samples under the fit (a, b) and the k-mer's (L, SD): out3 = mean_u, stdv_u, z_c
extern "C" void pgt_evalign_event(const int16_t *sig, uint32_t n, double a, double b, uint32_t L, uint32_t SD, int32_t *out3) {
    double A, G; pg_ea_read_scale(a, b, A, G);
    int64_t s1 = 0; uint64_t s2 = 0;
    for (uint32_t i = 0; i < n; i++) { const int64_t d = 1000ll * ((int64_t)sig[i] - (int64_t)sig[0]); s1 += d; s2 += (uint64_t)(d * d); }
    pg_ea_event(sig[0], n, s1, s2, A, G, L, SD, out3[0], out3[1], out3[2]);
}
extern "C" int pgt_evalign_z(int64_t mean_u, uint32_t L, uint32_t SD) { return pg_ea_z(mean_u, L, SD); }
// the rows of one read (op_t null: all matches), 40 bytes each, up to cap of them; returns their number, or -1 - (the walk's code)
extern "C" long pgt_evalign_walk(const uint8_t *seq, uint64_t n_seq, const uint32_t *op_n, const uint8_t *op_t, uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig,
                                 const uint32_t *levels, const uint32_t *stdvs, uint32_t k, uint32_t m, int rna, uint32_t min_dur, uint32_t max_dur, double a, double b, void *rows,
                                 size_t cap) {
    std::vector<PgEaRow> r;
    const int st = pg_ea_walk_host(seq, n_seq, op_n, op_t, lb, q, sig, n_sig, levels, stdvs, k, m, rna != 0, min_dur, max_dur, a, b, r);
    if (st != PG_FIT_OK) return st < 0 ? -100 + st : -1 - st;
    memcpy(rows, r.data(), (r.size() < cap ? r.size() : cap) * sizeof(PgEaRow));
    return (long)r.size();
}
// the line of one row: returns pg_ea_row_len, *written = what pg_ea_row_write stored (dst holds at least 4096 bytes more than the strings)
extern "C" uint32_t pgt_evalign_row_text(const void *row40, const uint8_t *contig, uint32_t contig_len, const uint8_t *label, uint32_t label_len, const uint8_t *kmer, uint32_t k,
                                         uint32_t S, int64_t ref_start, int reverse, uint32_t rate, uint32_t L, uint32_t SD, char *dst, uint32_t *written) {
    PgEaRow o; memcpy(&o, row40, sizeof o);
    PgEaText t;
    t.contig = contig; t.contig_len = contig_len; t.label = label; t.label_len = label_len; t.kmer = kmer; t.k = k; t.S = S; t.first = o.first; t.reverse = reverse ? 1 : 0;
    t.event = o.event; t.n = o.n; t.sample_rate = rate; t.L = L; t.SD = SD; t.mean_u = o.mean_u; t.stdv_u = o.stdv_u; t.z_c = o.z_c; t.ref_start = ref_start; t.start = o.start;
    *written = pg_ea_row_write(dst, t);
    return pg_ea_row_len(t);
}
extern "C" const char *pgt_evalign_header() { return PG_EA_HEADER; }

// ---- simulate (pg_sim.h): the generator, the rule for one read, the parsers, the command's read drawing and stride rounding -----------------
#include "pg_sim.h"
extern "C" void pgt_sim_levels(uint64_t *out6) {
    out6[0] = PG_SIM_PIECE; out6[1] = PG_SIM_LANE; out6[2] = PG_SIM_MAX_LEVEL; out6[3] = PG_SIM_MAX_DWELL; out6[4] = PG_SIM_BATCH_SAMPLES; out6[5] = PG_SIM_MAX_Q;
}
extern "C" void pgt_sim_philox(const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4) {
    const PgSimX x = pg_sim_philox(ctr4[0], ctr4[1], ctr4[2], ctr4[3], key2[0], key2[1]);
    out4[0] = x.x0; out4[1] = x.x1; out4[2] = x.x2; out4[3] = x.x3;
}
extern "C" uint64_t pgt_sim_q(uint32_t digitisation, uint64_t range_e4) { return pg_sim_q(digitisation, range_e4); }
// the status; ops (lb of them) and samples (up to cap) of an accepted read; rule11 = k, m, rna, seed, Q, offset, off_spread, spread_pct, lead, lead_level, lead_stdv
extern "C" int pgt_sim_walk(const int64_t *rule11, const uint32_t *levels, const uint32_t *stdvs, const uint32_t *dwells, const uint8_t *seq, uint32_t lb, uint64_t read, uint32_t *ops,
                            int16_t *sig, uint64_t cap, uint64_t *n_sig, int32_t *off_r) {
    const PgSimRule R{(uint32_t)rule11[0], (uint32_t)rule11[1], rule11[2] != 0, (uint64_t)rule11[3], (uint64_t)rule11[4], (int32_t)rule11[5], (uint32_t)rule11[6], (uint32_t)rule11[7],
                      (uint32_t)rule11[8], (uint32_t)rule11[9], (uint32_t)rule11[10]};
    std::vector<uint32_t> o; std::vector<int16_t> s;
    const uint32_t st = pg_sim_walk_host(R, levels, stdvs, dwells, seq, lb, read, o, s, off_r);
    if (!o.empty()) memcpy(ops, o.data(), o.size() * 4);
    *n_sig = s.size();
    if (!s.empty() && s.size() <= cap) memcpy(sig, s.data(), s.size() * 2);
    return (int)st;
}
extern "C" int pgt_sim_parse_dwell(const char *text, size_t n, uint32_t want_k, uint32_t *k, uint32_t *dwells, size_t cap_slots, char *err, size_t ecap) {
    std::vector<uint32_t> dw; std::string why;
    if (!pg_sim_parse_dwell_text(text, n, want_k, *k, dw, why) || dw.size() > cap_slots) { snprintf(err, ecap, "%s", why.c_str()); return -1; }
    memcpy(dwells, dw.data(), dw.size() * 4);
    return 0;
}
extern "C" int pgt_sim_parse_model(const char *text, size_t n, uint32_t want_k, uint32_t *k, uint32_t *levels, uint32_t *stdvs, size_t cap_slots, char *err, size_t ecap) {
    PgFitModel md; std::vector<uint32_t> sd; std::string why;
    if (!pg_fit_parse_model_text(text, n, want_k, md, why, &sd) || md.levels.size() > cap_slots) { snprintf(err, ecap, "%s", why.c_str()); return -1; }
    memcpy(levels, md.levels.data(), md.levels.size() * 4); memcpy(stdvs, sd.data(), sd.size() * 4);
    *k = md.k;
    return 0;
}
extern "C" void pgt_sim_pick(uint64_t seed, uint64_t read, uint64_t total, uint32_t read_len, int rna, uint64_t *out3) {
    const PgSimPick p = pg_sim_pick(seed, read, total, read_len, rna != 0);
    out3[0] = p.pos; out3[1] = p.len; out3[2] = p.reverse ? 1 : 0;
}
extern "C" uint64_t pgt_sim_round_stride(uint64_t B, uint32_t lead, uint32_t stride) { return pg_sim_round_stride(B, lead, stride); }
// the writer behind `simulate -o`: n records (ids NUL-separated) into an ASCII SLOW5 or an uncompressed BLOW5; 0, or -1
extern "C" int pgt_sim_write_slow5(const char *path, int binary, uint64_t n, const char *ids, const double *dig, const double *off, const double *range, const int16_t *raw,
                                   const uint64_t *raw_off) {
    pgh::Slow5Writer w; std::string err;
    if (!w.open(path, binary != 0, 4000.0, err)) return -1;
    for (uint64_t i = 0; i < n; i++, ids += strlen(ids) + 1)
        if (!w.add(ids, dig[i], off[i], range[i], raw + raw_off[i], raw_off[i + 1] - raw_off[i], err)) return -1;
    return w.close(err) ? 0 : -1;
}

// ---- svb-zd written (pg_svb.h: the encoder's rule; host/io.cpp: the writer that takes the blocks) -------------------------------------
extern "C" uint64_t pgt_svb_bound(uint64_t n) { return pg_svb_bound(n); }
extern "C" uint32_t pgt_svb_max_v(void) { return PG_SVB_MAX_V; }
// the block of one read into out (cap >= pg_svb_bound(n), else nothing is written); returns its bytes
extern "C" uint64_t pgt_svb_encode(const int16_t *s, uint32_t n, uint8_t *out, uint64_t cap) {
    return cap >= pg_svb_bound(n) ? pg_svb_encode_host(s, n, out) : 0;
}
extern "C" int pgt_zstd_can_compress(void) { return pgh::Slow5Writer::zstd_available() ? 1 : 0; }
// the writer with its two methods by name: n records from raw samples (sig "none") or from finished blocks (sig "svb-zd", sig_off then
// counts bytes); 0, -1 (errbuf), or -2 for a name the writer does not know
extern "C" int pgt_sim_write_blow5(const char *path, int binary, const char *rec, const char *sig, unsigned threads, uint64_t n, const char *ids, const double *dig,
                                   const double *off, const double *range, const void *signal, const uint64_t *sig_off, char *errbuf, size_t ecap) {
    pgh::Slow5Writer::RecPress rp; pgh::Slow5Writer::SigPress sp;
    if (!pgh::Slow5Writer::parse_rec_press(rec, rp) || !pgh::Slow5Writer::parse_sig_press(sig, sp)) return -2;
    pgh::Slow5Writer w; std::string err;
    if (!w.open(path, binary != 0, 4000.0, rp, sp, threads, err)) { put_err(err, errbuf, ecap); return -1; }
    for (uint64_t i = 0; i < n; i++, ids += strlen(ids) + 1) {
        const uint64_t len = sig_off[i + 1] - sig_off[i];
        const bool ok = sp == pgh::Slow5Writer::SIG_SVB_ZD ? w.add_block(ids, dig[i], off[i], range[i], (const unsigned char *)signal + sig_off[i], len, err)
                                                           : w.add(ids, dig[i], off[i], range[i], (const int16_t *)signal + sig_off[i], len, err);
        if (!ok) { put_err(err, errbuf, ecap); return -1; }
    }
    if (!w.close(err)) { put_err(err, errbuf, ecap); return -1; }
    return 0;
}

// ---- the record and signal batches of fit and realign (host/pg_moverecs.h), run to the end of the files ---------------------------------
#include "host/pg_moverecs.h"
// Per batch that holds a read its reads and samples; per read, in the order taken, the id (0-terminated, back to back), seven numbers --
// stride, ns, ts, l_seq, elements of the table behind the stride, samples, sum of the samples --, the offset of the calibration, the
// table's elements and the packed bases (both back to back); `bad`: why the run ended, empty at the end of the files. Returns the number
// of batches, -1 (bad: why a file cannot be opened) or -2 when an array is too small.
extern "C" long pgt_move_batches(const char *sam_path, const char *slow5_path, size_t max_reads, size_t soft, size_t hard, uint64_t *batch_reads, uint64_t *batch_samples,
                                 size_t batch_cap, char *ids, size_t ids_cap, int64_t *nums7, double *offset, size_t reads_cap, int8_t *mv, size_t mv_cap, uint8_t *packed,
                                 size_t packed_cap, char *bad, size_t bad_cap) {
    pgh::SamBamReader sam; pgh::Slow5File s5; std::string why;
    if (!sam.open(sam_path, why) || !s5.open(slow5_path, why)) { put_err(why, bad, bad_cap); return -1; }
    pgh::MoveSignalBatches in(sam, s5, "hosttest", max_reads, soft, hard);
    size_t nb = 0, nr = 0, ni = 0, nm = 0, np = 0;
    for (bool more = true; more && !in.done();) {
        more = in.next(why);
        const pgh::MoveRecs &rb = in.recs;
        if (!rb.size()) continue;
        if (nb == batch_cap || nr + rb.size() > reads_cap || nm + rb.mv.size() > mv_cap || np + rb.seqb.size() > packed_cap) return -2;
        batch_reads[nb] = rb.size(); batch_samples[nb++] = in.sig.size();
        for (size_t i = 0; i < rb.size(); i++, nr++) {
            if (ni + rb.names[i].size() + 1 > ids_cap) return -2;
            memcpy(ids + ni, rb.names[i].c_str(), rb.names[i].size() + 1); ni += rb.names[i].size() + 1;
            int64_t sum = 0;
            for (uint64_t s = in.sig_off[i]; s < in.sig_off[i + 1]; s++) sum += in.sig[s];
            const int64_t v[7] = {rb.stride[i], (int64_t)rb.ns[i], (int64_t)rb.ts[i], rb.l_seq[i], (int64_t)(rb.mv_off[i + 1] - rb.mv_off[i]), (int64_t)(in.sig_off[i + 1] - in.sig_off[i]), sum};
            memcpy(nums7 + 7 * nr, v, sizeof v);
            offset[nr] = in.off[i];
        }
        if (rb.mv.size()) memcpy(mv + nm, rb.mv.data(), rb.mv.size());
        if (rb.seqb.size()) memcpy(packed + np, rb.seqb.data(), rb.seqb.size());
        nm += rb.mv.size(); np += rb.seqb.size();
    }
    put_err(why, bad, bad_cap);
    return (long)nb;
}
