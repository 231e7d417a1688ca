// pg_kfreq_host.h -- host side of `poregen kmer_freq` on SAM/BAM input: the reads of the file, batch by batch, in the packed form
// pg_kfreq_submit_reads takes (include/pgmove.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "pg_f1_host.h"

namespace pgh {

// what one pg_kfreq_submit_reads call takes: read r is len[r] bases from byte off[r] of seq, two 4-bit codes per byte
struct PackedBatch {
    std::vector<uint8_t> seq;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint8_t> rev; // flag 0x10
    void clear() { seq.clear(); off.clear(); len.clear(); rev.clear(); }
};

// The records `samtools fastq` prints by default (-F 0x900: flags 0x100 and 0x800 are skipped), in file order. BAM: BGZF blocks are
// inflated `want` bytes at a time on up to 16 threads and each kept record's sequence field is copied as it lies (no per-base work).
// SAM: column 10 is packed by htslib's rule (pg_kfreq_codes.h), "*" is an empty read, header lines are optional.
class PackedReads {
public:
    // as_bam: the caller's choice (by file name); a BAM file whose first block is not BGZF holding "BAM\1" is refused
    bool open(const std::string &path, bool as_bam, std::string &err);
    // the next batch: about `want` bytes of the file's (inflated) text. 1 = a batch (it may hold no read), 0 = end of file, -1 = error
    int next(PackedBatch &out, size_t want, std::string &err);
private:
    MappedFile f_;
    bool bam_ = false;
    size_t pos_ = 0;          // SAM: offset of the next line; BAM: offset of the next BGZF block
    std::vector<char> text_;  // BAM: inflated bytes, consumed up to tpos_
    size_t tpos_ = 0;
    std::vector<BgzfBlock> blocks_;
    bool more(size_t want, std::string &err); // inflate the next blocks behind what is left of text_; false: error, or (err empty) no block left
};

} // namespace pgh
