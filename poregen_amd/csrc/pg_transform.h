// pg_transform.h -- STEP 7 of the reference's pipeline on the host (no device code; shared by `poregen transform` and libpgmove's
// pg_transform_model): scripts/poregen.sh:87-129 apply_transformation and :131-148 set_stddev, with bc's arithmetic from pg_bcdec.h.
//   rows    KMER<TAB>level_mean<TAB>level_stdv, further columns ignored; a last line without '\n' counts (the script's `read` drops it)
//   header  the script's seven lines; "#k" carries the length of the first k-mer (the script prints 5), every k-mer has that length
//   min/max `cut -f3 | datamash min 1 max 1`: the smallest and the largest level_stdv as long doubles, printed "%.14Lg"
//   row     level_mean' = (level_mean * A) + B;  level_stdv' = (level_stdv - min) * (D - C) / (max - min) + C, operation by operation
//   from    set_stddev: column 3 of lines 8.. of another model replaces level_stdv', by position, verbatim
// Anything bc would not compute -- a field that is no number, a row without samples (fewer than 3 fields), max == min, an empty model,
// a k-mer of another length, a result bc would wrap -- refuses the whole model: `out` is left empty and `err` names the line.
#pragma once
#include "pg_bcdec.h"

#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

namespace pgtr {

struct Row { const char *kmer; size_t kmer_len; const char *f[2]; size_t f_len[2]; size_t line; };

// the lines of a text: a last line without '\n' counts, a '\n' at the very end opens no further line
inline void split_lines(const char *t, size_t n, std::vector<std::pair<const char *, size_t>> &lines) {
    for (size_t i = 0; i < n;) {
        size_t j = i;
        while (j < n && t[j] != '\n') j++;
        lines.emplace_back(t + i, j - i);
        i = j + 1;
    }
}

// the first `want` tab-separated fields of a line; returns how many there are (at most want)
inline int split_fields(const char *l, size_t n, int want, const char **f, size_t *f_len) {
    int k = 0;
    for (size_t i = 0; k < want;) {
        size_t j = i;
        while (j < n && l[j] != '\t') j++;
        f[k] = l + i; f_len[k] = j - i; k++;
        if (j >= n) break;
        i = j + 1;
    }
    return k;
}

inline std::string quoted(const char *s, size_t n) { return "'" + std::string(s, n > 80 ? 80 : n) + (n > 80 ? "...'" : "'"); }

// datamash's print of a min / max: strtold, "%.14Lg" (trailing zeros go; 15 digits or more are rounded; an exponent can appear)
inline std::string datamash_g(long double v) {
    char t[64];
    snprintf(t, sizeof t, "%.14Lg", v);
    return t;
}

inline bool transform(const char *raw, size_t n, const char *A, const char *B, const char *C, const char *D, const char *from, size_t n_from,
                      std::string &out, std::string &err) {
    out.clear();
    auto fail = [&](const std::string &why) { err = why; out.clear(); return false; };
    pgbc::Dec a, b, c, d;
    const struct { const char *name, *text; pgbc::Dec *v; } consts[4] = {{"A (--stdv)", A, &a}, {"B (--mean)", B, &b}, {"C (--stdv_min)", C, &c}, {"D (--stdv_max)", D, &d}};
    for (const auto &k : consts)
        if (!k.text || !pgbc::parse(k.text, strlen(k.text), *k.v)) return fail(std::string(k.name) + " is not a number: " + quoted(k.text ? k.text : "", k.text ? strlen(k.text) : 0));

    std::vector<std::pair<const char *, size_t>> lines;
    split_lines(raw, n, lines);
    if (lines.empty()) return fail("the raw model is empty");
    std::vector<Row> rows(lines.size());
    std::vector<pgbc::Dec> mean(lines.size()), stdv(lines.size());
    long double lo = 0, hi = 0;
    for (size_t i = 0; i < lines.size(); i++) {
        Row &r = rows[i];
        r.line = i + 1;
        const std::string at = "line " + std::to_string(r.line) + ": ";
        const char *f[3]; size_t fl[3];
        const int nf = split_fields(lines[i].first, lines[i].second, 3, f, fl);
        if (nf < 3) return fail(at + "k-mer " + quoted(f[0], fl[0]) + " has no samples (" + std::to_string(nf) + " of 3 fields)");
        r.kmer = f[0]; r.kmer_len = fl[0]; r.f[0] = f[1]; r.f_len[0] = fl[1]; r.f[1] = f[2]; r.f_len[1] = fl[2];
        if (r.kmer_len == 0) return fail(at + "the k-mer is empty");
        if (r.kmer_len != rows[0].kmer_len) return fail(at + "k-mer " + quoted(f[0], fl[0]) + " has " + std::to_string(r.kmer_len) + " letters, the first one has " + std::to_string(rows[0].kmer_len));
        if (!pgbc::parse(f[1], fl[1], mean[i])) return fail(at + "level_mean " + quoted(f[1], fl[1]) + " is not a number");
        if (!pgbc::parse(f[2], fl[2], stdv[i])) return fail(at + "level_stdv " + quoted(f[2], fl[2]) + " is not a number");
        const long double v = strtold(std::string(f[2], fl[2]).c_str(), nullptr);
        if (i == 0 || v < lo) lo = v;
        if (i == 0 || v > hi) hi = v;
    }
    const std::string lo_text = datamash_g(lo), hi_text = datamash_g(hi);
    pgbc::Dec mn, mx, span, dc;
    if (!pgbc::parse(lo_text, mn)) return fail("the smallest level_stdv prints as " + lo_text + " (%.14Lg), which is not a number to bc");
    if (!pgbc::parse(hi_text, mx)) return fail("the largest level_stdv prints as " + hi_text + " (%.14Lg), which is not a number to bc");
    if (!pgbc::sub(mx, mn, span) || !pgbc::sub(d, c, dc)) return fail("a constant has too many digits");
    if (span.m.zero()) return fail("every level_stdv is " + lo_text + ": max == min, nothing to project onto [C, D]");

    std::vector<std::pair<const char *, size_t>> from_col;
    if (from) {
        std::vector<std::pair<const char *, size_t>> fl_;
        split_lines(from, n_from, fl_);
        for (size_t i = 7; i < fl_.size(); i++) { // its data rows: `tail -n +8`
            const char *f[3]; size_t fl[3];
            if (split_fields(fl_[i].first, fl_[i].second, 3, f, fl) < 3) return fail("--stdv_from line " + std::to_string(i + 1) + ": no level_stdv column (fewer than 3 fields)");
            from_col.emplace_back(f[2], fl[2]);
        }
        if (from_col.size() != rows.size())
            return fail("--stdv_from holds " + std::to_string(from_col.size()) + " data rows (lines 8 onward), the raw model " + std::to_string(rows.size()));
    }

    std::string o = "#ont_model_name\tnone\n#kit\tnone\n#strand\ttemplate\n#k\t" + std::to_string(rows[0].kmer_len) +
                    "\n#alphabet\tnucleotide\n#original_file\tnone\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\tweight\n";
    std::string text;
    for (size_t i = 0; i < rows.size(); i++) {
        const std::string at = "line " + std::to_string(rows[i].line) + ": ";
        pgbc::Dec t, u;
        if (!pgbc::mul(mean[i], a, t) || !pgbc::add(t, b, t)) return fail(at + "level_mean has too many digits");
        if (!pgbc::print(t, text)) return fail(at + "the transformed level_mean has more than 68 characters (bc would break the line)");
        o.append(rows[i].kmer, rows[i].kmer_len); o += '\t'; o += text; o += '\t';
        if (!pgbc::sub(stdv[i], mn, u) || !pgbc::mul(u, dc, u) || !pgbc::div(u, span, u) || !pgbc::add(u, c, u)) return fail(at + "level_stdv has too many digits");
        if (!pgbc::print(u, text)) return fail(at + "the transformed level_stdv has more than 68 characters (bc would break the line)");
        if (from) o.append(from_col[i].first, from_col[i].second); else o += text;
        o += '\n';
    }
    out.swap(o);
    err.clear();
    return true;
}

} // namespace pgtr
