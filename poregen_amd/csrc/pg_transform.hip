// pg_transform.hip -- pg_transform_model / pg_transform_free (include/pgmove.h): STEP 7 of the reference's pipeline behind the C ABI.
// Host code only -- 4^k rows of exact decimal arithmetic (pg_transform.h, pg_bcdec.h) have no hot path and launch nothing; the file sits
// in libpgmove so that Python and other callers reach the same arithmetic the `poregen transform` command runs.
#include "../../include/pgmove.h"
#include "pg_transform.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <exception>
#include <string>

extern "C" {

pg_status pg_transform_model(const char *raw, size_t n, const char *A, const char *B, const char *C, const char *D, const char *stdv_from, size_t n_from,
                             char **out, size_t *n_out, char *err, size_t err_cap) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (err && err_cap) err[0] = 0;
    auto say = [&](const std::string &s) { if (err && err_cap) snprintf(err, err_cap, "%s", s.c_str()); };
    if (!out || !n_out || (!raw && n) || (!stdv_from && n_from)) { say("pg_transform_model: out, n_out and every text with a length must be given"); return PG_ERR_INVALID_ARG; }
    std::string text, why;
    try {
        if (!pgtr::transform(raw, n, A, B, C, D, stdv_from, n_from, text, why)) { say(why); return PG_ERR_INPUT; }
    } catch (const std::exception &) { say("out of memory"); return PG_ERR_INVALID_ARG; }
    char *p = (char *)malloc(text.size() + 1);
    if (!p) { say("out of memory"); return PG_ERR_INVALID_ARG; }
    memcpy(p, text.data(), text.size());
    p[text.size()] = 0;
    *out = p; *n_out = text.size();
    return PG_OK;
}

void pg_transform_free(char *text) { free(text); }

} // extern "C"
