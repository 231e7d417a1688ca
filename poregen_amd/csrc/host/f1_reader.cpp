// f1_reader.cpp -- the records `poregen f1_score` reads: name, flag, contig, position, CIGAR end and the ss / si Z tags of every SAM or
// BAM record, plus the reference names. The BGZF blocks of a BAM file are found in one pass over the block headers and inflated in
// parallel, each straight to its place in one buffer (with the default --read_limit the whole-file parse is the entire run).
// gmove / reform keep their own streaming reader (SamBamReader in io.cpp), unchanged.
#include "pg_f1_host.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <zlib.h>

namespace pgh {

int parse_py_int(std::string_view s, int64_t &out) {
    auto space = [](unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); };
    size_t a = 0, b = s.size();
    while (a < b && space((unsigned char)s[a])) a++;
    while (b > a && space((unsigned char)s[b - 1])) b--;
    bool neg = false;
    if (a < b && (s[a] == '+' || s[a] == '-')) { neg = s[a] == '-'; a++; }
    if (a == b) return 1;
    constexpr uint64_t kMax = 1ull << 62;
    uint64_t v = 0;
    bool big = false, prev_digit = false;
    for (size_t i = a; i < b; i++) {
        const char c = s[i];
        if (c == '_') {
            if (!prev_digit || i + 1 == b) return 1; // a '_' only between two digits
            prev_digit = false;
            continue;
        }
        if (c < '0' || c > '9') return 1;
        if (!big) { v = v * 10 + (uint64_t)(c - '0'); if (v >= kMax) big = true; }
        prev_digit = true;
    }
    if (!prev_digit) return 1;
    if (big) return 2;
    out = neg ? -(int64_t)v : (int64_t)v;
    return 0;
}

namespace {

// htslib's bam_endpos: pos + the reference length of the CIGAR (M, D, N, =, X), pos + 1 when unmapped or that length is 0
int64_t end_of(int64_t pos, uint32_t flag, int64_t rlen) { return pos + ((flag & 4) || rlen == 0 ? 1 : rlen); }
bool ref_op(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

} // namespace

bool AlnFile::load(const std::string &path, unsigned threads, std::string &err) {
    if (!f_.open(path)) { err = "cannot open " + path; return false; }
    bam_ = f_.size >= 4 && (unsigned char)f_.data[0] == 0x1f && (unsigned char)f_.data[1] == 0x8b;
    refs.clear(); recs.clear();
    return bam_ ? parse_bam(threads, err) : parse_sam(err);
}

bool AlnFile::parse_sam(std::string &err) {
    const char *p = f_.data, *e = f_.data + f_.size;
    std::vector<std::pair<std::string_view, int32_t>> names; // sorted after the header
    bool sorted = false;
    auto tid_of = [&](std::string_view rn) -> int32_t {
        if (!sorted) { std::sort(names.begin(), names.end()); sorted = true; }
        auto it = std::lower_bound(names.begin(), names.end(), std::make_pair(rn, (int32_t)-1));
        return it != names.end() && it->first == rn ? it->second : -1;
    };
    while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        const char *le = nl ? nl : e;
        const char *next = nl ? nl + 1 : e;
        if (le > p && le[-1] == '\r') le--; // htslib drops a CR before the newline
        if (le == p) { p = next; continue; }
        if (*p == '@') {
            if (le - p > 4 && memcmp(p, "@SQ\t", 4) == 0) {
                for (const char *q = p + 4; q < le;) {
                    const char *t = (const char *)memchr(q, '\t', (size_t)(le - q)); if (!t) t = le;
                    if (t - q >= 3 && memcmp(q, "SN:", 3) == 0) {
                        names.emplace_back(std::string_view(q + 3, (size_t)(t - q - 3)), (int32_t)refs.size());
                        refs.emplace_back(q + 3, t);
                        sorted = false;
                    }
                    q = t + 1;
                }
            }
            p = next; continue;
        }
        AlnRec r;
        int col = 0;
        std::string_view rname, cigar;
        int64_t pos1 = 0;
        for (const char *q = p; q <= le;) {
            const char *t = (const char *)memchr(q, '\t', (size_t)(le - q)); if (!t) t = le;
            const std::string_view f(q, (size_t)(t - q));
            if (col == 0) r.name = f;
            else if (col == 1) r.flag = (uint32_t)strtoul(std::string(f).c_str(), nullptr, 0);
            else if (col == 2) rname = f;
            else if (col == 3) pos1 = strtoll(std::string(f).c_str(), nullptr, 10);
            else if (col == 5) cigar = f;
            else if (col >= 11 && f.size() >= 5 && f[2] == ':' && f[4] == ':') {
                if (f[0] == 's' && f[1] == 's' && !r.has_ss) { r.has_ss = true; r.ss_is_z = f[3] == 'Z'; r.ss = f.substr(5); }
                if (f[0] == 's' && f[1] == 'i' && !r.has_si) { r.has_si = true; r.si_is_z = f[3] == 'Z'; r.si = f.substr(5); }
            }
            col++;
            if (t >= le) break;
            q = t + 1;
        }
        if (col < 11) { err = "malformed SAM record"; return false; }
        r.tid = rname == "*" ? -1 : tid_of(rname);
        r.pos = pos1 - 1;
        int64_t rlen = 0;
        if (cigar != "*") {
            uint64_t n = 0;
            for (char c : cigar) {
                if (c >= '0' && c <= '9') { n = n * 10 + (uint64_t)(c - '0'); continue; }
                const char *ops = "MIDNSHP=X";
                const char *o = strchr(ops, c);
                if (!o || !c) { err = "malformed CIGAR in SAM record"; return false; }
                if (ref_op((int)(o - ops))) rlen += (int64_t)n;
                n = 0;
            }
        }
        r.endpos = end_of(r.pos, r.flag, rlen);
        recs.push_back(r);
        p = next;
    }
    return true;
}

bool bgzf_scan(const char *data, size_t size, size_t &pos, size_t want, std::vector<BgzfBlock> &blocks, size_t &total, std::string &err) {
    blocks.clear();
    total = 0;
    while (pos < size && total < want) {
        if (size - pos < 18) { err = "corrupt BGZF block"; return false; }
        const unsigned char *b = (const unsigned char *)data + pos;
        if (b[0] != 0x1f || b[1] != 0x8b || !(b[3] & 4)) { err = "corrupt BGZF block"; return false; }
        uint16_t xlen; memcpy(&xlen, b + 10, 2);
        if (12u + (size_t)xlen > size - pos) { err = "corrupt BGZF block"; return false; }
        uint32_t bsize = 0; bool found = false;
        for (size_t o = 12; o + 4 <= 12u + xlen;) {
            uint16_t slen; memcpy(&slen, b + o + 2, 2);
            if (b[o] == 'B' && b[o + 1] == 'C' && slen == 2 && o + 6 <= 12u + xlen) { uint16_t v; memcpy(&v, b + o + 4, 2); bsize = (uint32_t)v + 1; found = true; }
            o += 4u + slen;
        }
        const size_t hdr = 12u + xlen;
        if (!found || bsize > size - pos || bsize < hdr + 8) { err = "corrupt BGZF block"; return false; }
        uint32_t isize; memcpy(&isize, b + bsize - 4, 4);
        if (isize > 65536u) { err = "corrupt BGZF block"; return false; }
        blocks.push_back(BgzfBlock{pos, hdr, bsize - hdr - 8, total, isize});
        total += isize;
        pos += bsize;
    }
    return true;
}

bool bgzf_inflate(const char *data, const std::vector<BgzfBlock> &blocks, char *out, unsigned threads, std::string &err) {
    std::atomic<size_t> next{0};
    std::atomic<bool> bad{false};
    auto work = [&]() {
        z_stream zs; memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) { bad = true; return; }
        for (size_t i; !bad && (i = next.fetch_add(64)) < blocks.size();) {
            for (size_t k = i; k < std::min(blocks.size(), i + 64); k++) {
                const BgzfBlock &bl = blocks[k];
                if (!bl.isize) continue;
                if (inflateReset(&zs) != Z_OK) { bad = true; break; }
                zs.next_in = (Bytef *)(data + bl.off + bl.hdr); zs.avail_in = (uInt)bl.clen;
                zs.next_out = (Bytef *)out + bl.out; zs.avail_out = bl.isize;
                if (inflate(&zs, Z_FINISH) != Z_STREAM_END || zs.avail_out != 0) { bad = true; break; }
            }
        }
        inflateEnd(&zs);
    };
    const unsigned nt = std::max(1u, std::min({threads, 16u, (unsigned)(blocks.size() / 64 + 1)}));
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    if (bad) { err = "zlib error in BGZF block"; return false; }
    return true;
}

bool AlnFile::parse_bam(unsigned threads, std::string &err) {
    // 1. the blocks: compressed extent and inflated size, from the headers and footers alone
    std::vector<BgzfBlock> blocks;
    size_t total = 0, pos = 0;
    if (!bgzf_scan(f_.data, f_.size, pos, SIZE_MAX, blocks, total, err)) return false;
    // 2. inflate them in parallel, each to its offset
    text_.resize(total);
    if (!bgzf_inflate(f_.data, blocks, text_.data(), threads, err)) return false;
    // 3. header and records
    const char *d = text_.data();
    size_t p = 0;
    auto need = [&](size_t k) { return total - p >= k; };
    if (!need(12) || memcmp(d, "BAM\1", 4) != 0) { err = "not a BAM file"; return false; }
    int32_t l_text; memcpy(&l_text, d + 4, 4);
    p = 8;
    if (l_text < 0 || !need((size_t)l_text + 4)) { err = "truncated BAM header"; return false; }
    p += (size_t)l_text;
    int32_t n_ref; memcpy(&n_ref, d + p, 4); p += 4;
    if (n_ref < 0) { err = "corrupt BAM header"; return false; }
    for (int32_t i = 0; i < n_ref; i++) {
        if (!need(4)) { err = "truncated BAM header"; return false; }
        int32_t l_name; memcpy(&l_name, d + p, 4); p += 4;
        if (l_name < 1 || !need((size_t)l_name + 4)) { err = "truncated BAM header"; return false; }
        refs.emplace_back(d + p, strnlen(d + p, (size_t)l_name));
        p += (size_t)l_name + 4;
    }
    while (p < total) {
        if (!need(4)) { err = "truncated BAM record"; return false; }
        int32_t block_size; memcpy(&block_size, d + p, 4);
        if (block_size < 32 || !need(4 + (size_t)block_size)) { err = "truncated BAM record"; return false; }
        const unsigned char *r = (const unsigned char *)d + p + 4, *rend = r + block_size;
        p += 4 + (size_t)block_size;
        AlnRec a;
        int32_t ref_id, pos; memcpy(&ref_id, r, 4); memcpy(&pos, r + 4, 4);
        const uint8_t l_read_name = r[8];
        uint16_t n_cigar, flag; memcpy(&n_cigar, r + 12, 2); memcpy(&flag, r + 14, 2);
        int32_t l_seq; memcpy(&l_seq, r + 16, 4);
        a.flag = flag;
        a.tid = ref_id >= 0 && ref_id < n_ref ? ref_id : -1;
        a.pos = pos;
        const unsigned char *q = r + 32;
        auto left = [&]() { return (size_t)(rend - q); };
        if ((size_t)l_read_name > left()) { err = "corrupt BAM record"; return false; }
        a.name = std::string_view((const char *)q, l_read_name ? strnlen((const char *)q, l_read_name) : 0); q += l_read_name;
        if (4u * (size_t)n_cigar > left()) { err = "corrupt BAM record"; return false; }
        int64_t rlen = 0;
        for (uint32_t i = 0; i < n_cigar; i++) { uint32_t c; memcpy(&c, q + 4 * i, 4); if (ref_op((int)(c & 15))) rlen += c >> 4; }
        q += 4u * (size_t)n_cigar;
        a.endpos = end_of(a.pos, a.flag, rlen);
        if (l_seq < 0 || ((size_t)l_seq + 1) / 2 + (size_t)l_seq > left()) { err = "corrupt BAM record"; return false; }
        q += ((size_t)l_seq + 1) / 2 + (size_t)l_seq;
        while (left() >= 3) {
            const char t0 = (char)q[0], t1 = (char)q[1], ty = (char)q[2];
            q += 3;
            size_t adv = 0;
            switch (ty) {
                case 'A': case 'c': case 'C': adv = 1; break;
                case 's': case 'S': adv = 2; break;
                case 'i': case 'I': case 'f': adv = 4; break;
                case 'Z': case 'H': { const unsigned char *z = (const unsigned char *)memchr(q, 0, left()); if (!z) { err = "corrupt BAM tag"; return false; } adv = (size_t)(z - q) + 1; break; }
                case 'B': {
                    if (left() < 5) { err = "corrupt BAM tag"; return false; }
                    const char sub = (char)q[0]; int32_t cnt; memcpy(&cnt, q + 1, 4);
                    const size_t esz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                    if (cnt < 0 || (size_t)cnt > (left() - 5) / esz) { err = "corrupt BAM tag"; return false; }
                    adv = 5 + esz * (size_t)cnt; break;
                }
                default: err = "unknown BAM tag type"; return false;
            }
            if (adv > left()) { err = "corrupt BAM tag"; return false; }
            const std::string_view z = ty == 'Z' ? std::string_view((const char *)q, adv - 1) : std::string_view();
            if (t0 == 's' && t1 == 's' && !a.has_ss) { a.has_ss = true; a.ss_is_z = ty == 'Z'; a.ss = z; }
            if (t0 == 's' && t1 == 'i' && !a.has_si) { a.has_si = true; a.si_is_z = ty == 'Z'; a.si = z; }
            q += adv;
        }
        recs.push_back(a);
    }
    return true;
}

} // namespace pgh
