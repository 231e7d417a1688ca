// moverecs.cpp -- where a batch of records and signals ends (pg_moverecs.h).
#include "pg_moverecs.h"

namespace pgh {

void MoveSignalBatches::take() {
    recs.push(raw_);
    sig.insert(sig.end(), rec_.raw.begin(), rec_.raw.end()); sig_off.push_back(sig.size());
    dig.push_back(rec_.digitisation); off.push_back(rec_.offset); range.push_back(rec_.range);
}

bool MoveSignalBatches::next(std::string &bad) {
    recs.clear(); sig.clear(); sig_off.assign(1, 0); dig.clear(); off.clear(); range.clear();
    while (recs.size() < max_reads_ && sig.size() < soft_) {
        if (pending_) { // the record that did not fit the batch in front: read, checked and fetched already
            pending_ = false;
            if (rec_.raw.size() > hard_) { bad = "[" + std::string(tool_) + "] read " + raw_.qname + " has more than 2^28 samples"; return false; } // (the commands' cap)
            take();
            continue;
        }
        const int nr = next_move_record(sam_, raw_, tool_, bad, to_ref_skipped, reverse_taken);
        if (nr == 0) eof_ = true;
        if (nr <= 0) return nr == 0;
        std::string e2;
        if (!s5_.get(raw_.qname, rec_, e2)) { bad = "Error in when fetching the read (" + e2 + ")"; return false; }
        if (sig.size() + rec_.raw.size() > hard_) { pending_ = true; break; } // it opens the next batch (the reader is not called before it is taken)
        take();
    }
    return true;
}

} // namespace pgh
