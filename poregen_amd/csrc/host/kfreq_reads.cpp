// kfreq_reads.cpp -- the reads of a SAM or BAM file in the packed form `poregen kmer_freq` hands to the device (pg_kfreq_host.h).
// Which records count is `samtools fastq`'s default: flags 0x100 (secondary) and 0x800 (supplementary) are skipped, flag 0x10 marks the
// read as stored reverse-complemented. What the device makes of a read is in include/pgmove.h (pg_kfreq_submit_reads).
#include "pg_kfreq_host.h"
#include "../pg_kfreq_codes.h"

#include <cstdlib>
#include <cstring>

namespace pgh {

namespace {
constexpr uint32_t kSkipFlags = 0x900;
constexpr unsigned kInflateThreads = 16; // f1_reader's cap; a batch of 64 MiB holds about 1000 blocks
}

bool PackedReads::more(size_t want, std::string &err) {
    text_.erase(text_.begin(), text_.begin() + (long)tpos_);
    tpos_ = 0;
    if (pos_ >= f_.size) return false;
    size_t total = 0;
    if (!bgzf_scan(f_.data, f_.size, pos_, want ? want : 1, blocks_, total, err)) return false;
    const size_t old = text_.size();
    text_.resize(old + total);
    return bgzf_inflate(f_.data, blocks_, text_.data() + old, kInflateThreads, err);
}

bool PackedReads::open(const std::string &path, bool as_bam, std::string &err) {
    if (!f_.open(path)) { err = "cannot open " + path; return false; }
    bam_ = as_bam;
    pos_ = 0; text_.clear(); tpos_ = 0;
    if (!bam_) return true;
    // the header: magic, l_text, text, n_ref, the references (name length, name, length)
    auto have = [&](size_t n) {
        while (text_.size() < n) {
            if (!more(1 << 20, err)) { if (err.empty()) err = text_.size() < 4 ? "not a BAM file" : "truncated BAM header"; return false; }
        }
        return true;
    };
    if (f_.size < 18 || (unsigned char)f_.data[0] != 0x1f || (unsigned char)f_.data[1] != 0x8b) { err = "not a BAM file"; return false; }
    if (!have(4)) return false;
    if (memcmp(text_.data(), "BAM\1", 4) != 0) { err = "not a BAM file"; return false; }
    if (!have(12)) return false;
    int32_t l_text; memcpy(&l_text, text_.data() + 4, 4);
    if (l_text < 0) { err = "corrupt BAM header"; return false; }
    size_t p = 8 + (size_t)l_text;
    if (!have(p + 4)) return false;
    int32_t n_ref; memcpy(&n_ref, text_.data() + p, 4); p += 4;
    if (n_ref < 0) { err = "corrupt BAM header"; return false; }
    for (int32_t i = 0; i < n_ref; i++) {
        if (!have(p + 4)) return false;
        int32_t l_name; memcpy(&l_name, text_.data() + p, 4);
        if (l_name < 0) { err = "corrupt BAM header"; return false; }
        p += 4 + (size_t)l_name + 4;
        if (!have(p)) return false;
    }
    tpos_ = p;
    return true;
}

int PackedReads::next(PackedBatch &out, size_t want, std::string &err) {
    out.clear();
    if (!bam_) {
        if (pos_ >= f_.size) return 0;
        const char *e = f_.data + f_.size;
        const size_t stop = f_.size - pos_ > want ? pos_ + want : f_.size; // lines that start in front of `stop`
        while (pos_ < stop) {
            const char *p = f_.data + pos_;
            const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
            const char *le = nl ? nl : e;
            pos_ = (size_t)((nl ? nl + 1 : e) - f_.data);
            if (le > p && le[-1] == '\r') le--;
            if (le == p || *p == '@') continue; // blank or header line
            int col = 0;
            uint32_t flag = 0;
            const char *seq = nullptr; size_t n = 0;
            for (const char *q = p; q <= le;) {
                const char *t = (const char *)memchr(q, '\t', (size_t)(le - q)); if (!t) t = le;
                if (col == 1) flag = (uint32_t)strtoul(std::string(q, t).c_str(), nullptr, 0);
                else if (col == 9) { seq = q; n = (size_t)(t - q); }
                col++;
                if (t >= le) break;
                q = t + 1;
            }
            if (col < 11) { err = "malformed SAM record"; return -1; }
            if (flag & kSkipFlags) continue;
            if (n == 1 && *seq == '*') n = 0;
            if (n > 0x7fffffffu) { err = "SAM record with more than 2^31 - 1 bases"; return -1; }
            const size_t at = out.seq.size();
            out.seq.resize(at + (n + 1) / 2);
            uint8_t *dst = out.seq.data() + at;
            for (size_t i = 0; i + 1 < n; i += 2)
                dst[i >> 1] = (uint8_t)(pg_kf_code_of_byte((unsigned char)seq[i]) << 4 | pg_kf_code_of_byte((unsigned char)seq[i + 1]));
            if (n & 1) dst[n >> 1] = (uint8_t)(pg_kf_code_of_byte((unsigned char)seq[n - 1]) << 4);
            out.off.push_back(at); out.len.push_back((uint32_t)n); out.rev.push_back(flag & 0x10 ? 1 : 0);
        }
        return 1;
    }
    bool any = false;
    for (;;) {
        // every whole record of what is inflated
        while (text_.size() - tpos_ >= 4) {
            int32_t block_size; memcpy(&block_size, text_.data() + tpos_, 4);
            if (block_size < 32) { err = "corrupt BAM record"; return -1; }
            if (text_.size() - tpos_ - 4 < (size_t)block_size) break;
            const unsigned char *r = (const unsigned char *)text_.data() + tpos_ + 4;
            tpos_ += 4 + (size_t)block_size;
            any = true;
            const uint8_t l_read_name = r[8];
            uint16_t n_cigar, flag; memcpy(&n_cigar, r + 12, 2); memcpy(&flag, r + 14, 2);
            int32_t l_seq; memcpy(&l_seq, r + 16, 4);
            const size_t head = 32 + (size_t)l_read_name + 4u * (size_t)n_cigar;
            if (l_seq < 0 || head > (size_t)block_size || ((size_t)l_seq + 1) / 2 + (size_t)l_seq > (size_t)block_size - head) { err = "corrupt BAM record"; return -1; }
            if (flag & kSkipFlags) continue;
            const size_t at = out.seq.size(), nb = ((size_t)l_seq + 1) / 2;
            out.seq.resize(at + nb);
            if (nb) memcpy(out.seq.data() + at, r + head, nb);
            out.off.push_back(at); out.len.push_back((uint32_t)l_seq); out.rev.push_back(flag & 0x10 ? 1 : 0);
        }
        if (any) return 1;
        if (!more(want, err)) {
            if (!err.empty()) return -1;
            if (text_.size() != tpos_) { err = "truncated BAM record"; return -1; }
            return 0;
        }
    }
}

} // namespace pgh
