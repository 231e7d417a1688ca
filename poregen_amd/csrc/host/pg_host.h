// pg_host.h -- host side of the `poregen gmove` drop-in: file parsers, k-mer list, dump writer.
// Everything here is I/O and bookkeeping; the computation is behind include/pgmove.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

namespace pgh {

// May `path` be written? For an output that is written at the end of a run and is asked about at its start, without creating it: an
// existing file must be writable, a new one needs a writable directory.
bool can_write_file(const char *path);

// ---- memory-mapped read-only file ---------------------------------------------------------------------
struct MappedFile {
    const char *data = nullptr;
    size_t size = 0;
    int fd = -1;
    bool open(const std::string &path);
    void close();
    ~MappedFile() { close(); }
};

// ---- SLOW5 / BLOW5 (replaces slow5_open / slow5_idx_load / slow5_get, src/gmove.cpp:493-503,745) --------
struct Slow5Rec {
    double digitisation = 0, offset = 0, range = 0;
    std::vector<int16_t> raw;
};
class Slow5File {
public:
    bool open(const std::string &path, std::string &err); // opens and indexes (read id -> record location)
    bool get(const std::string &read_id, Slow5Rec &out, std::string &err) const; // false if absent / malformed
    // uncompressed BLOW5 (records and signals stored as they are): the samples of a read where they lie in the mapped file, so that a
    // caller can copy them ONCE, straight to where they are needed. false if absent / malformed (err) -- only when has_raw_views()
    struct RawView { const void *samples = nullptr; uint64_t n = 0; double digitisation = 0, offset = 0, range = 0; };
    bool has_raw_views() const { return binary_ && rec_press_ == 0 && sig_press_ == 0; }
    bool raw_view(const std::string &read_id, RawView &v, std::string &err) const;
    size_t n_reads() const { return index_.size(); }
    // File-order walk (subtool0: slow5_get_next_bytes, src/poregen.cpp:84-116): every record in the order of the file, records with the
    // same read id included; no read-id index is built (get / raw_view / n_reads are not for a walk). record / record_view may be called
    // from several threads at once.
    bool open_walk(const std::string &path, std::string &err);
    size_t n_records() const { return recs_.size(); }
    uint64_t record_bytes(size_t i) const { return recs_[i].len; }
    bool record(size_t i, std::string &read_id, Slow5Rec &out, std::string &err) const;
    bool record_view(size_t i, std::string &read_id, RawView &v, std::string &err) const; // has_raw_views() only
    // svb-zd BLOW5 (record compression none, zlib or zstd): a record's calibration and its signal block (pg_svb.h) as a byte range, for a
    // decoder elsewhere. The block has passed pg_svb_check and lies in the mapped file or, for compressed records, in `inflated`, which
    // the caller keeps for as long as it needs the block.
    struct SvbView { const unsigned char *block = nullptr; uint64_t len = 0; uint32_t count = 0; double digitisation = 0, offset = 0, range = 0; };
    bool has_svb_views() const { return binary_ && sig_press_ == 1; }
    bool records_compressed() const { return rec_press_ != 0; } // the blocks then lie in `inflated`, else in the mapped file
    bool record_svb(size_t i, std::string &read_id, SvbView &v, std::vector<unsigned char> &inflated, std::string &err) const; // has_svb_views() only
    bool is_binary() const { return binary_; }
    const std::vector<std::string> &ids_in_file_order() const { return order_; }
private:
    struct Loc { uint64_t off, len; };
    MappedFile f_;
    bool binary_ = false;
    uint8_t rec_press_ = 0, sig_press_ = 0;
    int col_dig_ = 2, col_off_ = 3, col_range_ = 4, col_len_ = 6, col_sig_ = 7;
    std::unordered_map<std::string, Loc> index_;
    std::vector<std::string> order_;
    bool walk_ = false;
    std::vector<Loc> recs_; // open_walk: every record, in file order
    bool index_ascii(std::string &err);
    bool index_blow5(std::string &err);
    bool body_of(const Loc &l, std::vector<unsigned char> &inflated, const unsigned char *&body, size_t &blen, std::string &err) const;
    bool head_of(const unsigned char *body, size_t blen, std::string *read_id, double &dig, double &off, double &range, uint64_t &len, size_t &p,
                 std::string &err) const;
    bool decode_blow5(const Loc &l, Slow5Rec &out, std::string &err, std::string *read_id = nullptr) const;
    bool parse_ascii(const Loc &l, Slow5Rec &out, const std::string &label, std::string &err) const;
    bool view_blow5(const Loc &l, RawView &v, std::string &err, std::string *read_id = nullptr) const;
};

// ---- SLOW5 / BLOW5 writer (`poregen simulate -o`): ASCII SLOW5, or BLOW5 -- as it is, or with the records compressed (zlib, zstd) and / or
// the signals as svb-zd blocks (pg_svb.h) that the caller has encoded; one read group; the header lines Slow5File needs to read the file
// back. Code of its own: nothing of the reading paths is shared or changed.
class Slow5Writer {
public:
    enum RecPress { REC_NONE = 0, REC_ZLIB = 1, REC_ZSTD = 2 }; // header byte 9
    enum SigPress { SIG_NONE = 0, SIG_SVB_ZD = 1 };            // header byte 14
    static bool parse_rec_press(const char *name, RecPress &out); // "none", "zlib", "zstd"
    static bool parse_sig_press(const char *name, SigPress &out); // "none", "svb-zd"
    static bool zstd_available();                                 // libzstd.so.1 with what REC_ZSTD needs is on this machine
    ~Slow5Writer();
    bool open(const std::string &path, bool binary, double sampling_rate, std::string &err); // nothing compressed
    // BLOW5 with the two methods; threads: records are compressed on that many threads (each record on its own, written in the order they
    // were added: the file does not depend on the number). An ASCII file takes REC_NONE and SIG_NONE alone.
    bool open(const std::string &path, bool binary, double sampling_rate, RecPress rec, SigPress sig, unsigned threads, std::string &err);
    bool add(const std::string &read_id, double digitisation, double offset, double range, const int16_t *raw, uint64_t n, std::string &err); // SIG_NONE
    // SIG_SVB_ZD: a finished block of `len` bytes; the record's len_raw_signal holds len
    bool add_block(const std::string &read_id, double digitisation, double offset, double range, const unsigned char *block, uint64_t len, std::string &err);
    bool close(std::string &err); // writes the end-of-file marker of a BLOW5 file
private:
    bool put_body(const std::string &read_id, double digitisation, double offset, double range, uint64_t len_field, const void *signal, uint64_t bytes, std::string &err);
    bool flush(std::string &err); // compresses and writes the waiting records
    void *fp_ = nullptr; // FILE *
    bool binary_ = false;
    double rate_ = 4000.0;
    RecPress rec_ = REC_NONE;
    SigPress sig_ = SIG_NONE;
    unsigned threads_ = 1;
    std::string line_;
    std::vector<std::string> waiting_; // record bodies not yet compressed
    size_t waiting_bytes_ = 0;
};

// ---- FASTA/FASTQ with faidx semantics (replaces fai_load / faidx_fetch_seq, src/gmove.cpp:724,805) -----
class FastxIndex {
public:
    bool load(const std::string &path, std::string &err);
    // htslib 1.17 faidx_fetch_seq(fai, name, beg, end, &len): [beg,end] 0-based inclusive, clamped into the
    // sequence; returns false (len = -2 in htslib) when the name is absent
    bool fetch(const std::string &name, int64_t beg, int64_t end, std::string &out) const;
private:
    struct Ent { uint64_t seq_off; int64_t len; uint32_t line_bases, line_width; };
    MappedFile f_;
    std::unordered_map<std::string, Ent> idx_;
};

// ---- PAF with ss:Z: (replaces parse_paf_rec, src/gmove.cpp:977-1052) -----------------------------------
struct PafRec {
    std::string rid, tid;
    int32_t qlen = 0, query_start = 0, query_end = 0, tlen = 0, target_start = 0, target_end = 0;
    const char *ss = nullptr; // points into the line buffer
    size_t ss_len = 0;
};
// returns 0 ok, 1 = fewer than 12 columns (the reference asserts), 2 = no ss:Z: tag (the reference exits 1)
int parse_paf_line(char *line, size_t len, PafRec &out);
// tokenises "<n>," "<n>I" "<n>D" (src/gmove.cpp:831-871); returns false on the reference's "Bad ss" exits
bool tokenize_ss(const char *ss, size_t len, std::vector<uint32_t> &op_n, std::vector<uint8_t> &op_t, std::string &err);

// ---- SAM / BAM records with the move table tags (replaces sam_open/sam_read1/bam_aux_get, src/gmove.cpp:1067-1134) --
struct MoveRec {
    std::string qname, seq;        // SEQ with every letter outside ACGT mapped to 'N' (gmove.cpp:1128-1134)
    int stride = 0;                // mv[0]
    uint32_t mv_len = 0;           // bam_auxB_len of mv (stride element included)
    std::vector<uint8_t> is_one;   // mv[1..]: 1 where the value is 1
    uint64_t ns = 0, ts = 0;       // signal length / trim offset tags
    bool has_ns = false, has_ts = false, has_mv = false, mv_is_Bc = false;
};
// The same record with nothing expanded (gmove --reform): the move array and the bases as a BAM record stores them -- the int8
// elements of mv:B:c behind the stride element, two 4-bit base codes per byte (csrc/pg_kfreq_codes.h). A BAM record's two arrays are
// pointed at where they lie in the reader's buffer, a SAM line's are packed into the record's own storage; either way the pointers hold
// until the next call on the reader.
struct RawMoveRec {
    std::string qname;
    uint32_t flag = 0, l_seq = 0;
    int stride = 0;                // mv[0]
    uint32_t mv_len = 0;           // elements of mv, the stride element included
    const int8_t *mv = nullptr;    // mv[1..]: mv_len - 1 elements
    const uint8_t *packed = nullptr; // (l_seq + 1) / 2 bytes
    uint64_t ns = 0, ts = 0;
    bool has_ns = false, has_ts = false, has_mv = false, mv_is_Bc = false;
    std::vector<int8_t> mv_store; std::vector<uint8_t> packed_store; // SAM
    // where the record is mapped: the CIGAR as a BAM record stores it (words len << 4 | op, op 0..8 = MIDNSHP=X; a SAM line's text is
    // parsed into the same words, a letter that is none of the nine into op 15), the 0-based position (-1: none), the reference's name
    // (empty: none, SAM's `*`) and its length from @SQ / the BAM header's reference list (0: not listed)
    std::vector<uint32_t> cigar;
    int32_t pos = -1;
    std::string rname;
    int64_t ref_len = 0;
};
class SamBamReader {
public:
    bool open(const std::string &path, std::string &err); // SAM text or BGZF-compressed BAM, detected by content
    int next(MoveRec &out, std::string &err);              // 1 = record, 0 = end of file, -1 = error
    int next_raw(RawMoveRec &out, std::string &err);       // the same
private:
    int next_impl(MoveRec &out, RawMoveRec *raw, std::string &err);
    MappedFile f_;
    bool bam_ = false;
    size_t pos_ = 0;                 // SAM: offset into the file; BAM: offset of the next BGZF block
    std::vector<unsigned char> buf_; // BAM: inflated bytes not yet consumed
    size_t bpos_ = 0;
    std::vector<std::pair<std::string, int64_t>> refs_; // BAM: the header's reference list, by refID
    std::unordered_map<std::string, int64_t> sq_;        // SAM: LN of every @SQ line, by SN
    bool fill(size_t need, std::string &err);
};

// ---- k-mer list (src/poregen.cpp:248-267, src/gmove.cpp:394-426) ----------------------------------------
void generate_kmers(int k, bool rna, std::vector<std::string> &out);
// returns 0 ok, 1 cannot open, 2 a line does not have exactly k characters + '\n'
int read_kmer_file(const std::string &path, int k, std::vector<std::string> &out, std::string &err);

// ---- dump directory (src/gmove.cpp:107-140, 460-473, 525-534, 938-950, 196-203) -------------------------
int create_dir(const char *dir_name); // 0 ok / created, -1 exists and not empty, -2 cannot create
// "%.8f" exactly as glibc printf prints it; returns the number of characters written (buf >= 400 bytes)
size_t format_f8(double v, char *buf);
struct DumpInput {
    uint32_t n_slots;
    const uint64_t *counts, *ev_off, *samp_off;
    const uint32_t *ev_len, *ev_read;
    const double *samples;   // the job's k-mer-major sample stream on the host, or null: then `fetch` brings ranges of it (pg_fetch_samples)
    const uint8_t *read_skipped;
    uint64_t n_reads;
    std::function<bool(uint64_t first, uint64_t n, double *dst)> fetch; // callable from several threads at once
};
// Plain storage for the big host buffers (a batch's signal, the pieces the dump writers fetch): a mapping of its own with transparent huge
// pages asked for (the boxes run THP in "madvise" mode). 200 page faults instead of 100 000 per 400 MB at the first touch, the runtime pins
// 200 pages instead of 100 000 when it copies from / into it (staging a 176 MB batch: 35 -> 14 ms; tools/probe/e2e_staging.sh), and as many
// pages less to hand back when the process ends. Not initialised, not copyable.
struct HugeBuf {
    void *p = nullptr; size_t bytes = 0;
    HugeBuf() = default;
    HugeBuf(const HugeBuf &) = delete; HugeBuf &operator=(const HugeBuf &) = delete;
    ~HugeBuf() { release(); }
    void release();
    bool grow(size_t want_bytes, size_t keep_bytes); // false: out of memory; the first keep_bytes survive
};

// writes dump/<kmer> for every slot and freq.txt; delimit = -d; returns false on I/O error
bool write_dump_dir(const std::string &out_dir, const std::vector<std::string> &slot_kmers, const DumpInput &in, bool delimit,
                    uint32_t sample_limit, unsigned n_threads, std::string &err);
// the same from text the device has produced (pg_text): slot s is bytes [slot_off[s], slot_off[s + 1]) of one stream, fetched in pieces
struct TextInput {
    uint32_t n_slots;
    const uint64_t *slot_off, *counts;
    std::function<bool(uint64_t first, uint64_t n, char *dst)> fetch; // callable from several threads at once
};
bool write_dump_dir_text(const std::string &out_dir, const std::vector<std::string> &slot_kmers, const TextInput &in, unsigned n_threads, std::string &err);
bool touch_dump_files(const std::string &out_dir, const std::vector<std::string> &slot_kmers, std::string &err);

} // namespace pgh
