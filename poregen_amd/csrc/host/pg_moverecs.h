// pg_moverecs.h -- the records of a SAM / BAM file as a move-table batch (pg_mvops_batch), read once for `gmove --reform`, `fit` and
// `realign`: which records are taken, why one is not (reform's texts), and -- for the two commands that fetch a read's signal with its
// record -- where a batch ends. Host only: nothing of HIP.
#pragma once
#include "../../../include/pgmove.h"
#include "pg_host.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace pgh {

// reform's error line, in its red: the message, then the read
inline std::string reform_error(const char *msg, const std::string &read_id) {
    char b[600]; snprintf(b, sizeof b, "[reform::ERROR]\033[1;31m %s Read_id: %s\033[0m", msg, read_id.c_str()); return std::string(b);
}
// what reform says of a read the expansion refuses (pg_mvops_result::status_host); a code it does not know is an error of the implementation
inline const char *reform_refusal(uint32_t code) {
    static const char *const kRefusal[] = {"", "the move table holds fewer moves than sig_move_offset + 1.", "Error in calcuation. (ns - ((i-1)*EXPECTED_STRIDE + ts)) > 0 is not valid.",
                                           "Error in the implementation. Please report the command with minimal reproducible data.", "the stride of the move table (mv[0]) is less than 1."};
    return kRefusal[code < 5 ? code : 3];
}
// ... and of a read whose CIGAR the projection onto the reference refuses (codes 5 to 7); the expansion's codes keep their texts
inline const char *to_ref_refusal(uint32_t code) {
    return code == 5 ? "the record has no CIGAR." : code == 6 ? "the M/I/S/=/X lengths of the CIGAR do not come to the bases of the read." :
           code == 7 ? "the CIGAR holds an operation that is none of MIDNSHP=X." :
           code == 8 ? "the length of the reference sequence is not known (no @SQ line), a reverse-strand record cannot be placed." : reform_refusal(code);
}
// the contig length the projection takes for a record (pg_refops.h): 0 stands for "not known", a length above 2^31 - 1 among them
inline int32_t contig_len_of(int64_t ref_len) { return ref_len > 0 && ref_len <= 0x7fffffffll ? (int32_t)ref_len : 0; }
// the line both commands print at the end of a run that projected onto a reference
inline void print_to_ref_skipped(const char *tool, uint64_t n) {
    fprintf(stderr, "[%s] %llu records skipped: unmapped (flag 0x4 or no reference name) or on the reverse strand (flag 0x10)\n", tool, (unsigned long long)n);
}
// ... with --both_strands
inline void print_both_strands_skipped(const char *tool, uint64_t n, uint64_t reverse_taken) {
    fprintf(stderr, "[%s] %llu records skipped: unmapped (flag 0x4 or no reference name); %llu reverse-strand records taken\n", tool, (unsigned long long)n,
            (unsigned long long)reverse_taken);
}

// the records of a batch, back to back, in the layout pg_mvops_batch takes
struct MoveRecs {
    std::vector<std::string> names; std::vector<int8_t> mv; std::vector<uint64_t> mv_off{0}, ns, ts, boff; std::vector<int32_t> stride;
    std::vector<uint32_t> l_seq, flag; std::vector<uint8_t> seqb;
    // where the records are mapped (pg_mvops_cigars): the CIGAR words back to back, the 0-based positions, the references' names and lengths
    std::vector<uint32_t> cigar; std::vector<uint64_t> cigar_off{0}; std::vector<int32_t> pos; std::vector<std::string> rname; std::vector<int64_t> ref_len;
    size_t size() const { return names.size(); }
    void clear() {
        names.clear(); mv.clear(); mv_off.assign(1, 0); ns.clear(); ts.clear(); boff.clear(); stride.clear(); l_seq.clear(); flag.clear(); seqb.clear();
        cigar.clear(); cigar_off.assign(1, 0); pos.clear(); rname.clear(); ref_len.clear();
    }
    void push(const RawMoveRec &raw) {
        cigar.insert(cigar.end(), raw.cigar.begin(), raw.cigar.end()); cigar_off.push_back(cigar.size());
        pos.push_back(raw.pos); rname.push_back(raw.rname); ref_len.push_back(raw.ref_len);
        names.push_back(raw.qname);
        mv.insert(mv.end(), raw.mv, raw.mv + (raw.mv_len - 1)); mv_off.push_back(mv.size());
        stride.push_back(raw.stride); ns.push_back(raw.ns); ts.push_back(raw.ts); l_seq.push_back(raw.l_seq); flag.push_back(raw.flag);
        boff.push_back(seqb.size()); seqb.insert(seqb.end(), raw.packed, raw.packed + ((size_t)raw.l_seq + 1) / 2);
    }
    void fill(pg_mvops_batch &mb, size_t n, uint32_t flags) const { // the first n records, on the host
        memset(&mb, 0, sizeof mb);
        mb.n_reads = n; mb.location = PG_LOC_HOST; mb.flags = flags;
        mb.mv = mv.data(); mb.n_mv_bytes = mv_off[n]; mb.mv_off = mv_off.data(); mb.stride = stride.data(); mb.ns = ns.data(); mb.ts = ts.data();
        mb.l_seq = l_seq.data(); mb.flag = flag.data(); mb.seq_bytes = seqb.data(); mb.n_seq_bytes = seqb.size(); mb.byte_off = boff.data();
    }
};

// The next record a batch takes: 1 with the record in `raw`, 0 at the end of the file, -1 with `bad` saying why the record (or the file
// behind it) cannot be taken -- the first such record ends the run behind the reads in front of it, with gmove --reform's message.
// to_ref_skipped (gmove --reform --ref, reform --to_ref): records that are not mapped to the forward strand of a reference -- flag 0x4, no
// RNAME, flag 0x10 -- are stepped over and counted there. reverse_taken (--both_strands, with to_ref_skipped): mapped records with flag 0x10
// are taken instead and counted there.
inline int next_move_record(SamBamReader &sam, RawMoveRec &raw, const char *tool, std::string &bad, uint64_t *to_ref_skipped = nullptr, uint64_t *reverse_taken = nullptr) {
    for (std::string err;;) {
        const int nr = sam.next_raw(raw, err);
        if (nr == 0) return 0;
        if (nr < 0) { bad = "[" + std::string(tool) + "] " + err; return -1; }
        if (raw.flag & 0x900u) continue; // secondary / supplementary: `samtools fastq` does not print them
        if (to_ref_skipped && ((raw.flag & (reverse_taken ? 0x4u : 0x14u)) || raw.rname.empty())) { ++*to_ref_skipped; continue; }
        if (to_ref_skipped && reverse_taken && (raw.flag & 0x10u)) ++*reverse_taken;
        const char *why = !raw.has_ns ? "tag 'ns' is not found. Please check your SAM/BAM file:" : !raw.has_ts ? "tag 'ts' is not found. Please check your SAM/BAM file:" :
                          !raw.has_mv ? "NULL returned for tag mv:" : !raw.mv_is_Bc ? "tag 'mv' specification is incorrect." : raw.mv_len == 0 ? "mv array length is 0:" : nullptr;
        if (!why) return 1;
        bad = reform_error(why, raw.qname);
        return -1;
    }
}

// Records and their signals, batch by batch (fit, realign). A batch closes once it holds max_reads reads or at least `soft` samples. A
// fetched record that would take it past `hard` samples is kept, opens the next batch and is not read again; one longer than `hard` on
// its own ends the run, as does a read the SLOW5 file does not hold.
class MoveSignalBatches {
public:
    MoveSignalBatches(SamBamReader &sam, Slow5File &s5, const char *tool, size_t max_reads, size_t soft, size_t hard)
        : sam_(sam), s5_(s5), tool_(tool), max_reads_(max_reads), soft_(soft), hard_(hard) {}
    // the batch: record i's samples are sig[sig_off[i] .. sig_off[i + 1])
    MoveRecs recs; std::vector<int16_t> sig; std::vector<uint64_t> sig_off{0}; std::vector<double> dig, off, range;
    // --ref: the records next_move_record steps over are counted here (null: every record is taken, as without --ref)
    uint64_t *to_ref_skipped = nullptr, *reverse_taken = nullptr;
    // Fills the next batch. false: `bad` says why the run ends behind this batch, which still holds the reads in front of the record.
    bool next(std::string &bad);
    bool done() const { return eof_ && !pending_; }
private:
    void take(); // the record in raw_ / rec_ joins the batch
    SamBamReader &sam_; Slow5File &s5_; const char *tool_; size_t max_reads_, soft_, hard_;
    RawMoveRec raw_; Slow5Rec rec_;
    bool eof_ = false, pending_ = false; // pending_: raw_ / rec_ hold the record that did not fit the batch in front
};

} // namespace pgh
