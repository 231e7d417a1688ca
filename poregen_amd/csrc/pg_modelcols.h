// pg_modelcols.h -- the columns of a pg_model_result as a handle keeps them on the host, one entry per file or slot, filled from the
// reduction's records (PgSlotModel, PgSlotDwell). Used by pg_model / pg_model_device / pg_model_events (pg_api.hip) and by pg_dmodel_*
// (pg_dumptext.hip). pg_pool.hip keeps its own arrays: its groups are filled by index from combined moments, not from such records.
// Host code; not installed.
#pragma once
#include "../../include/pgmove.h"
#include "pg_model.h"
#include <vector>

struct PgModelCols {
    std::vector<uint64_t> n, s2lo, s2hi, dn;
    std::vector<int64_t> lo, hi, origin, s1;
    std::vector<double> med, sd, dmed;
    size_t size() const { return n.size(); }
    void clear() { for (auto *v : {&n, &s2lo, &s2hi, &dn}) v->clear(); for (auto *v : {&lo, &hi, &origin, &s1}) v->clear(); for (auto *v : {&med, &sd, &dmed}) v->clear(); }
    // one entry as the reduction left it; d == nullptr: no dwell (dwell_n 0, dwell_median NaN)
    void push(const PgSlotModel &m, const PgSlotDwell *d = nullptr) {
        const unsigned __int128 s2 = ((unsigned __int128)m.s2_hh << 40) + ((unsigned __int128)m.s2_hl << 21) + m.s2_ll;
        n.push_back(m.n); lo.push_back(m.mid_lo); hi.push_back(m.mid_hi); origin.push_back(m.origin); s1.push_back(m.s1);
        s2lo.push_back((uint64_t)s2); s2hi.push_back((uint64_t)(s2 >> 64));
        med.push_back(m.n ? (double)pg_model_median(m) : NAN); sd.push_back(m.n >= 2 ? (double)(pg_model_sstdev_units(m) / 1e8L) : NAN);
        dn.push_back(d ? d->n : 0); dmed.push_back(d && d->n ? ((double)d->mid_lo + (double)d->mid_hi) / 2.0 : NAN);
    }
    // one entry without exact fields (a file finished on the host): the rounded numbers only
    void push_rounded(uint64_t count, double median, double sstdev, uint64_t dwell_n, double dwell_median) {
        n.push_back(count); lo.push_back(0); hi.push_back(0); origin.push_back(0); s1.push_back(0); s2lo.push_back(0); s2hi.push_back(0);
        med.push_back(median); sd.push_back(sstdev); dn.push_back(dwell_n); dmed.push_back(dwell_median);
    }
    void fill(pg_model_result &r, uint32_t flags) const {
        r.n_slots = (uint32_t)n.size(); r.flags = flags;
        r.n_values = n.data(); r.median = med.data(); r.sstdev = sd.data(); r.mid_lo = lo.data(); r.mid_hi = hi.data(); r.origin = origin.data();
        r.sum1 = s1.data(); r.sum2_lo = s2lo.data(); r.sum2_hi = s2hi.data(); r.dwell_n = dn.data(); r.dwell_median = dmed.data();
    }
};
