// pg_f1_host.h -- host side of `poregen f1_score`: the alignment records the F1-score metric reads (src/f1_score/f1score.py:157-190)
// and the Python int() parser its si / option values go through.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "pg_host.h"

namespace pgh {

// one SAM/BAM record as f1score.py sees it; the views point into the AlnFile that returned it
struct AlnRec {
    std::string_view name, ss, si; // ss / si: the value of the FIRST tag of that name (pysam's get_tag)
    uint32_t flag = 0;
    int32_t tid = -1;              // index into AlnFile::refs, -1 for '*' or a name the header does not list
    int64_t pos = -1, endpos = 0;  // 0-based leftmost position; htslib's bam_endpos (CIGAR reference length, at least 1)
    bool has_ss = false, has_si = false, ss_is_z = false, si_is_z = false;
};

// A whole SAM text or BGZF BAM file, detected by content as SamBamReader::open does. BAM blocks are inflated on up to
// `threads` threads (at most 16) into one buffer, then the records are parsed in file order.
class AlnFile {
public:
    bool load(const std::string &path, unsigned threads, std::string &err);
    std::vector<std::string> refs; // @SQ SN (SAM) / the binary reference list (BAM)
    std::vector<AlnRec> recs;
    bool is_bam() const { return bam_; }
private:
    MappedFile f_;
    std::vector<char> text_; // BAM: the inflated stream
    bool bam_ = false;
    bool parse_sam(std::string &err);
    bool parse_bam(unsigned threads, std::string &err);
};

// The BGZF layer of that reader, for callers that take a BAM file piece by piece (kmer_freq). bgzf_scan walks the block headers and
// footers from file offset `pos` until the blocks found inflate to `want` bytes or more, or the file ends (`pos` moves behind the last
// block taken; `out` of a block is its place among the bytes of this scan); bgzf_inflate inflates them to out + block.out on up to
// `threads` threads, 16 at most.
struct BgzfBlock { size_t off, hdr, clen, out; uint32_t isize; };
bool bgzf_scan(const char *data, size_t size, size_t &pos, size_t want, std::vector<BgzfBlock> &blocks, size_t &total, std::string &err);
bool bgzf_inflate(const char *data, const std::vector<BgzfBlock> &blocks, char *out, unsigned threads, std::string &err);

// Python's int(str) for base 10 on ASCII text: surrounding whitespace, one sign, digits with single '_' between them.
// Returns 0 ok, 1 not an integer (Python's ValueError), 2 a magnitude of 2^62 or more (valid, but refused here).
int parse_py_int(std::string_view s, int64_t &out);

} // namespace pgh
