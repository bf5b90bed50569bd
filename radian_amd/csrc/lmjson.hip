// lmjson.hip -- host code: the RNA model file, radian/basecall.py:48-57 (json.load + re-keying), read straight into the dense table
// rd_load_lm takes.  The reference's default model has 4^11 = 4 194 304 contexts in ~420 MB of JSON; the standard library's parser
// builds 4.2 M Python strings and 21 M floats for it (21 s, 2 GB) before the table can be filled.  This is a one-pass scanner for the
// one shape such a file has -- an object of "ACGT..." keys, each with an array of four numbers --
//
//     { "AAAAAAAAAAA": [0.25, 0.25, 0.25, 0.25], "AAAAAAAAAAC": [ ... ], ... }
//
// and ANYTHING else (escapes in a key, another alphabet, nested values, NaN / Infinity literals, a fifth number, trailing text) makes
// it return RD_ERR_FORMAT without a verdict: the caller then runs the standard parser, whose errors are the reference's.  Numbers are
// converted by std::from_chars (locale-independent, correctly rounded: the double Python's float() gives for the same text); a repeated
// key keeps its last value (json.load's dict does the same); contexts the file does not hold stay NaN (sparse model: rd_load_lm).
//
// No GPU is touched; the file is part of libradian_hip.so so that the host side stays one ctypes binding.
#include "common.h"
#include "../../include/radian_hip.h"

#include <charconv>
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

inline const char* skip_ws(const char* p, const char* e)
{
    while (p < e && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) p++;
    return p;
}

inline int base_code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// JSON number grammar (RFC 8259): -? (0 | [1-9][0-9]*) (. [0-9]+)? ([eE] [+-]? [0-9]+)?   -> end of the token, or nullptr
inline const char* number_end(const char* p, const char* e)
{
    if (p < e && *p == '-') p++;
    if (p >= e) return nullptr;
    if (*p == '0') p++;
    else if (*p >= '1' && *p <= '9') {
        while (p < e && *p >= '0' && *p <= '9') p++;
    } else return nullptr;
    if (p < e && *p == '.') {
        p++;
        if (p >= e || *p < '0' || *p > '9') return nullptr;
        while (p < e && *p >= '0' && *p <= '9') p++;
    }
    if (p < e && (*p == 'e' || *p == 'E')) {
        p++;
        if (p < e && (*p == '+' || *p == '-')) p++;
        if (p >= e || *p < '0' || *p > '9') return nullptr;
        while (p < e && *p >= '0' && *p <= '9') p++;
    }
    return p;
}

}  // namespace

// Context length of the first key of the object in buf (1..13), or RD_ERR_FORMAT.
extern "C" int rd_lm_json_probe(const char* buf, size_t n, int* k_out)
{
    RD_REQUIRE(buf && k_out, "rd_lm_json_probe: null argument");
    const char* e = buf + n;
    const char* p = skip_ws(buf, e);
    if (p >= e || *p != '{') return RD_ERR_FORMAT;
    p = skip_ws(p + 1, e);
    if (p >= e || *p != '"') return RD_ERR_FORMAT;
    p++;
    int k = 0;
    while (p < e && base_code(*p) >= 0) {
        p++;
        k++;
    }
    if (p >= e || *p != '"' || k < 1 || k > 13) return RD_ERR_FORMAT;
    *k_out = k;
    return RD_OK;
}

// Fill table[4^k][4] (the caller has set every value to NaN) from the object in buf.  *n_entries = key/value pairs read,
// *n_contexts = distinct contexts among them.  RD_ERR_FORMAT: not the expected shape (the table is then in an undefined state).
extern "C" int rd_lm_json_fill(const char* buf, size_t n, int k, double* table, int64_t* n_entries, int64_t* n_contexts)
{
    RD_REQUIRE(buf && table && n_entries && n_contexts && k >= 1 && k <= 13, "rd_lm_json_fill: bad argument");
    const char* e = buf + n;
    const char* p = skip_ws(buf, e);
    if (p >= e || *p != '{') return RD_ERR_FORMAT;
    p = skip_ws(p + 1, e);
    int64_t entries = 0, distinct = 0;
    if (p < e && *p == '}') {
        p = skip_ws(p + 1, e);
        if (p != e) return RD_ERR_FORMAT;
        *n_entries = 0;
        *n_contexts = 0;
        return RD_OK;
    }
    for (;;) {
        if (p >= e || *p != '"' || e - p < k + 2) return RD_ERR_FORMAT;
        p++;
        size_t row = 0;
        for (int i = 0; i < k; i++) {
            const int c = base_code(p[i]);
            if (c < 0) return RD_ERR_FORMAT;
            row = (row << 2) | (size_t)c;
        }
        p += k;
        if (*p != '"') return RD_ERR_FORMAT;          // a longer or shorter key: mixed lengths are the standard parser's to report
        p = skip_ws(p + 1, e);
        if (p >= e || *p != ':') return RD_ERR_FORMAT;
        p = skip_ws(p + 1, e);
        if (p >= e || *p != '[') return RD_ERR_FORMAT;
        p = skip_ws(p + 1, e);
        double v[4];
        for (int i = 0; i < 4; i++) {
            const char* q = number_end(p, e);
            if (!q) return RD_ERR_FORMAT;
            const auto r = std::from_chars(p, q, v[i]);
            if (r.ec != std::errc() || r.ptr != q || std::isnan(v[i])) return RD_ERR_FORMAT;   // (out of range -> inf in Python: leave it to it)
            p = skip_ws(q, e);
            if (p >= e || *p != (i < 3 ? ',' : ']')) return RD_ERR_FORMAT;
            p = skip_ws(p + 1, e);
        }
        double* t = table + row * 4;
        if (std::isnan(t[0])) distinct++;
        t[0] = v[0];
        t[1] = v[1];
        t[2] = v[2];
        t[3] = v[3];
        entries++;
        if (p >= e) return RD_ERR_FORMAT;
        if (*p == ',') {
            p = skip_ws(p + 1, e);
            continue;
        }
        if (*p != '}') return RD_ERR_FORMAT;
        p = skip_ws(p + 1, e);
        if (p != e) return RD_ERR_FORMAT;
        break;
    }
    *n_entries = entries;
    *n_contexts = distinct;
    return RD_OK;
}

// The writer: table [4^k][4] -> the text the reader above (and json.load) takes, one pass, keys in row order.  Every number is written with the
// shortest digits that convert back to the same double (std::to_chars), so both readers return the table bit for bit.  Rows of NaN -- contexts
// a sparse model does not hold -- are left out; a NaN beside numbers, an infinity or a negative value is no probability and is refused.
// *n_rows = keys written, *n_bytes = size of the text.
extern "C" int rd_lm_json_write(const char* path, const double* table, int k, int64_t* n_rows, int64_t* n_bytes)
{
    RD_REQUIRE(path && table && n_rows && n_bytes, "rd_lm_json_write: null argument");
    RD_REQUIRE(k >= 1 && k <= 13, "rd_lm_json_write: context length %d out of range [1,13]", k);
    const size_t n = (size_t)1 << (2 * k);
    for (size_t c = 0; c < n; c++) {
        const double* d = table + c * 4;
        const int nan = (int)std::isnan(d[0]) + (int)std::isnan(d[1]) + (int)std::isnan(d[2]) + (int)std::isnan(d[3]);
        RD_REQUIRE(nan == 0 || nan == 4, "rd_lm_json_write: context %zu mixes NaN with numbers", c);
        for (int i = 0; i < 4 && !nan; i++)
            RD_REQUIRE(std::isfinite(d[i]) && !std::signbit(d[i]), "rd_lm_json_write: context %zu holds %g, which is no probability", c, d[i]);
    }
    FILE* f = fopen(path, "wb");
    if (!f) {
        rd_set_error("rd_lm_json_write: cannot open %s for writing", path);
        return RD_ERR_IO;
    }
    constexpr size_t kEntryMax = 13 + 8 + 4 * 26 + 8;     // key, punctuation, four numbers of at most 24 characters
    std::vector<char> buf((size_t)1 << 20);
    size_t fill = 0;
    int64_t rows = 0, bytes = 0;
    bool ok = true;
    buf[fill++] = '{';
    for (size_t c = 0; c < n && ok; c++) {
        const double* d = table + c * 4;
        if (std::isnan(d[0])) continue;
        if (fill + kEntryMax > buf.size()) {
            ok = fwrite(buf.data(), 1, fill, f) == fill;
            bytes += (int64_t)fill;
            fill = 0;
        }
        char* p = buf.data() + fill;
        if (rows) {
            *p++ = ',';
            *p++ = ' ';
        }
        *p++ = '"';
        for (int i = k - 1; i >= 0; i--) *p++ = "ACGT"[(c >> (2 * i)) & 3];
        *p++ = '"';
        *p++ = ':';
        *p++ = ' ';
        *p++ = '[';
        for (int i = 0; i < 4; i++) {
            if (i) {
                *p++ = ',';
                *p++ = ' ';
            }
            p = std::to_chars(p, p + 26, d[i]).ptr;
        }
        *p++ = ']';
        fill = (size_t)(p - buf.data());
        rows++;
    }
    buf[fill++] = '}';
    ok = ok && fwrite(buf.data(), 1, fill, f) == fill;
    bytes += (int64_t)fill;
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        rd_set_error("rd_lm_json_write: writing %s failed", path);
        return RD_ERR_IO;
    }
    *n_rows = rows;
    *n_bytes = bytes;
    return RD_OK;
}
