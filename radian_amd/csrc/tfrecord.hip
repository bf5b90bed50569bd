// tfrecord.hip -- host code: labelled signal windows out of TFRecord shards of tf.train.Example records, the format the
// reference trains and validates on (radian/data.py:9-31, `read_tfrecord`), without TensorFlow.
//
// Framing of one record (TFRecordWriter, uncompressed -- data.py reads shards with a plain TFRecordDataset):
//   u64 length, u32 masked_crc32c(length bytes), length bytes of data, u32 masked_crc32c(data)     (little-endian)
//   masked(c) = ((c >> 15) | (c << 17)) + 0xa282ead8
// Both checksums are verified.  The data is a serialised tf.train.Example:
//   Example  { Features features = 1; }             Features { map<string, Feature> feature = 1; }
//   Feature  { oneof { BytesList bytes_list = 1; FloatList float_list = 2; Int64List int64_list = 3; } }
//   FloatList { repeated float value = 1; }         Int64List { repeated int64 value = 1; }
// Repeated values are accepted packed (one length-delimited field) and unpacked (one field per value), mixed as protobuf
// allows; a repeated message field or a map key that occurs twice merges / overrides as protobuf parsers do (the last
// Feature of a key wins).  Unknown fields are skipped.
//
// The four features of read_tfrecord: `signal` FixedLenFeature([1024], float32), `label` VarLenFeature(float32) cast to int,
// `signal_length` and `label_length` FixedLenFeature([], int64).  Refused with RD_ERR_FORMAT, naming the record:
// a bad checksum, a truncated frame or message, a missing feature or one of another kind / size, signal_length outside
// 1..1024, label_length outside 0..len(label), and a counted label (the first label_length values) that is not exactly
// 0, 1, 2 or 3.  Values past label_length are padding and are not read (ctc_batch_cost takes the first label_length).
//
// The writer (rd_tfrecord_write, radian_amd/label_build.py) emits the same four features -- `signal` and `label` as packed float lists,
// the two lengths as one int64 each, map entries in key order -- framed with both masked checksums; a shard it wrote reads back exactly.
//
// Every access is bounds-checked (tests/asan_tfrecord.cpp feeds truncated and corrupted shards in exact-size buffers).
// No GPU is touched; the file is part of libradian_hip.so so that the host side stays one ctypes binding.
#include "common.h"
#include "../../include/radian_hip.h"

#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

struct rd_tfrecord {
    std::vector<float> signal;        // [n][1024]
    std::vector<int32_t> input_len;   // signal_length
    std::vector<int64_t> label_off;   // [n + 1] into labels
    std::vector<uint8_t> labels;      // the counted labels, 0..3
};

namespace {

constexpr int TF_WIN = 1024;

struct Refused {   // thrown inside, RD_ERR_FORMAT at the C boundary
    std::string why;
};

[[noreturn]] void refuse(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Refused{buf};
}

// crc32c (Castagnoli, reflected polynomial 0x82f63b78), slicing-by-8: ~1.5 GB/s per core
struct Crc32cTables {
    uint32_t t[8][256];
    Crc32cTables()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82f63b78u & (0u - (c & 1)));
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < 8; s++) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xff];
    }
};
const Crc32cTables kCrc;

uint32_t crc32c(const uint8_t* p, size_t n)
{
    uint32_t c = 0xffffffffu;
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = kCrc.t[7][lo & 0xff] ^ kCrc.t[6][(lo >> 8) & 0xff] ^ kCrc.t[5][(lo >> 16) & 0xff] ^ kCrc.t[4][lo >> 24] ^
            kCrc.t[3][hi & 0xff] ^ kCrc.t[2][(hi >> 8) & 0xff] ^ kCrc.t[1][(hi >> 16) & 0xff] ^ kCrc.t[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = (c >> 8) ^ kCrc.t[0][(c ^ *p++) & 0xff];
    return c ^ 0xffffffffu;
}

uint32_t masked(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// a bounded protobuf reader over [p, end)
struct Pb {
    const uint8_t* p;
    const uint8_t* end;
    int64_t rec;

    bool more() const { return p < end; }
    uint64_t varint()
    {
        uint64_t v = 0;
        for (int s = 0; s < 64; s += 7) {
            if (p >= end) refuse("record %lld: truncated varint", (long long)rec);
            const uint8_t b = *p++;
            v |= (uint64_t)(b & 0x7f) << s;
            if (!(b & 0x80)) return v;
        }
        refuse("record %lld: varint longer than 10 bytes", (long long)rec);
    }
    Pb sub()   // a length-delimited field's body
    {
        const uint64_t n = varint();
        if (n > (uint64_t)(end - p)) refuse("record %lld: a length-delimited field runs past its message", (long long)rec);
        Pb s{p, p + n, rec};
        p += n;
        return s;
    }
    void fixed(size_t n, void* out)
    {
        if ((size_t)(end - p) < n) refuse("record %lld: truncated fixed-width field", (long long)rec);
        memcpy(out, p, n);
        p += n;
    }
    void skip(int wt)
    {
        uint8_t tmp[8];
        switch (wt) {
        case 0: varint(); break;
        case 1: fixed(8, tmp); break;
        case 2: sub(); break;
        case 5: fixed(4, tmp); break;
        default: refuse("record %lld: protobuf wire type %d is not supported", (long long)rec, wt);
        }
    }
};

struct Feat {
    int kind = 0;   // 0 absent, 1 bytes, 2 float, 3 int64
    std::vector<float> f;
    std::vector<int64_t> i;
};

void parse_list(Pb body, Feat& ft, int kind)
{
    ft.kind = kind;
    ft.f.clear();
    ft.i.clear();
    while (body.more()) {
        const uint64_t tag = body.varint();
        const int field = (int)(tag >> 3), wt = (int)(tag & 7);
        if (field != 1 || kind == 1) {
            body.skip(wt);
            continue;
        }
        if (kind == 2) {
            if (wt == 5) {
                float v;
                body.fixed(4, &v);
                ft.f.push_back(v);
            } else if (wt == 2) {
                Pb pk = body.sub();
                if ((pk.end - pk.p) % 4) refuse("record %lld: packed float list of %lld bytes", (long long)body.rec, (long long)(pk.end - pk.p));
                const size_t n = (size_t)(pk.end - pk.p) / 4, at = ft.f.size();
                ft.f.resize(at + n);
                if (n) memcpy(ft.f.data() + at, pk.p, n * 4);
            } else {
                body.skip(wt);
            }
        } else {
            if (wt == 0) {
                ft.i.push_back((int64_t)body.varint());
            } else if (wt == 2) {
                Pb pk = body.sub();
                while (pk.more()) ft.i.push_back((int64_t)pk.varint());
            } else {
                body.skip(wt);
            }
        }
    }
}

// Feature message -> the last kind set wins (oneof)
void parse_feature(Pb body, Feat& ft)
{
    while (body.more()) {
        const uint64_t tag = body.varint();
        const int field = (int)(tag >> 3), wt = (int)(tag & 7);
        if (field >= 1 && field <= 3 && wt == 2)
            parse_list(body.sub(), ft, field);
        else
            body.skip(wt);
    }
}

enum { F_SIGNAL, F_LABEL, F_SIGLEN, F_LABLEN, F_N };
const char* const kNames[F_N] = {"signal", "label", "signal_length", "label_length"};

void parse_example(Pb ex, Feat (&fs)[F_N])
{
    while (ex.more()) {
        const uint64_t tag = ex.varint();
        const int wt = (int)(tag & 7);
        if ((tag >> 3) != 1 || wt != 2) {
            ex.skip(wt);
            continue;
        }
        Pb feats = ex.sub();   // Features
        while (feats.more()) {
            const uint64_t t2 = feats.varint();
            const int w2 = (int)(t2 & 7);
            if ((t2 >> 3) != 1 || w2 != 2) {
                feats.skip(w2);
                continue;
            }
            Pb entry = feats.sub();   // map entry {string key = 1; Feature value = 2;}
            std::string key;
            Feat val;
            bool have_val = false;
            while (entry.more()) {
                const uint64_t t3 = entry.varint();
                const int f3 = (int)(t3 >> 3), w3 = (int)(t3 & 7);
                if (f3 == 1 && w3 == 2) {
                    Pb k = entry.sub();
                    key.assign((const char*)k.p, (size_t)(k.end - k.p));
                } else if (f3 == 2 && w3 == 2) {
                    val = Feat();
                    parse_feature(entry.sub(), val);
                    have_val = true;
                } else {
                    entry.skip(w3);
                }
            }
            for (int k = 0; k < F_N; k++)
                if (key == kNames[k]) fs[k] = have_val ? val : Feat();
        }
    }
}

void decode_record(const uint8_t* data, size_t n, int64_t rec, rd_tfrecord* out)
{
    Feat fs[F_N];
    parse_example(Pb{data, data + n, rec}, fs);
    const int want[F_N] = {2, 2, 3, 3};
    for (int k = 0; k < F_N; k++) {
        if (fs[k].kind == 0) refuse("record %lld: feature '%s' is missing", (long long)rec, kNames[k]);
        if (fs[k].kind != want[k]) refuse("record %lld: feature '%s' is not a %s list", (long long)rec, kNames[k], want[k] == 2 ? "float" : "int64");
    }
    if (fs[F_SIGNAL].f.size() != TF_WIN)
        refuse("record %lld: 'signal' has %zu values, not %d", (long long)rec, fs[F_SIGNAL].f.size(), TF_WIN);
    for (int k = F_SIGLEN; k <= F_LABLEN; k++)
        if (fs[k].i.size() != 1) refuse("record %lld: '%s' has %zu values, not 1", (long long)rec, kNames[k], fs[k].i.size());
    const int64_t sl = fs[F_SIGLEN].i[0], ll = fs[F_LABLEN].i[0];
    if (sl < 1 || sl > TF_WIN) refuse("record %lld: signal_length %lld is outside 1..%d", (long long)rec, (long long)sl, TF_WIN);
    const std::vector<float>& lab = fs[F_LABEL].f;
    if (ll < 0 || ll > (int64_t)lab.size())
        refuse("record %lld: label_length %lld is outside 0..len(label) = %zu", (long long)rec, (long long)ll, lab.size());
    for (int64_t k = 0; k < ll; k++) {
        const float v = lab[(size_t)k];
        if (!(v == 0.f || v == 1.f || v == 2.f || v == 3.f))
            refuse("record %lld: label %lld is %g, not one of 0, 1, 2, 3", (long long)rec, (long long)k, (double)v);
        out->labels.push_back((uint8_t)v);
    }
    out->signal.insert(out->signal.end(), fs[F_SIGNAL].f.begin(), fs[F_SIGNAL].f.end());
    out->input_len.push_back((int32_t)sl);
    out->label_off.push_back((int64_t)out->labels.size());
}

void index_shard(const uint8_t* p, size_t n, rd_tfrecord* out)
{
    out->label_off.assign(1, 0);
    size_t at = 0;
    for (int64_t rec = 0; at < n; rec++) {
        if (n - at < 12) refuse("record %lld: truncated frame header (%zu bytes left)", (long long)rec, n - at);
        uint64_t len;
        uint32_t lcrc;
        memcpy(&len, p + at, 8);
        memcpy(&lcrc, p + at + 8, 4);
        if (masked(crc32c(p + at, 8)) != lcrc) refuse("record %lld: length checksum mismatch", (long long)rec);
        at += 12;
        if (len > n - at || n - at - len < 4)
            refuse("record %lld: truncated frame (%llu data bytes + 4 announced, %zu left)", (long long)rec, (unsigned long long)len, n - at);
        uint32_t dcrc;
        memcpy(&dcrc, p + at + len, 4);
        if (masked(crc32c(p + at, (size_t)len)) != dcrc) refuse("record %lld: data checksum mismatch", (long long)rec);
        decode_record(p + at, (size_t)len, rec, out);
        at += (size_t)len + 4;
    }
}

// ---- writer: one serialised tf.train.Example, built inside out ----
void put_varint(std::string& o, uint64_t v)
{
    while (v >= 0x80) {
        o.push_back((char)(v | 0x80));
        v >>= 7;
    }
    o.push_back((char)v);
}

void put_delimited(std::string& o, int field, const std::string& body)
{
    put_varint(o, (uint64_t)field << 3 | 2);
    put_varint(o, body.size());
    o += body;
}

// map entry {key = 1, value = 2: Feature {kind_field: list {value = 1, packed}}}; an empty list is an empty list message
void put_feature(std::string& feats, const char* key, int kind_field, const std::string& packed)
{
    std::string list, feature, entry;
    if (!packed.empty()) put_delimited(list, 1, packed);
    put_delimited(feature, kind_field, list);
    put_delimited(entry, 1, key);
    put_delimited(entry, 2, feature);
    put_delimited(feats, 1, entry);
}

void put_example(std::string& out, const float* signal, int64_t signal_length, const uint8_t* label, int64_t label_length)
{
    std::string feats, pk;
    pk.resize((size_t)label_length * 4);
    for (int64_t k = 0; k < label_length; k++) {
        const float v = (float)label[k];
        memcpy(&pk[(size_t)k * 4], &v, 4);
    }
    put_feature(feats, kNames[F_LABEL], 2, pk);
    pk.clear();
    put_varint(pk, (uint64_t)label_length);
    put_feature(feats, kNames[F_LABLEN], 3, pk);
    pk.assign((const char*)signal, (size_t)TF_WIN * 4);
    put_feature(feats, kNames[F_SIGNAL], 2, pk);
    pk.clear();
    put_varint(pk, (uint64_t)signal_length);
    put_feature(feats, kNames[F_SIGLEN], 3, pk);
    std::string ex;
    put_delimited(ex, 1, feats);
    const uint64_t len = ex.size();
    char head[12];
    memcpy(head, &len, 8);
    const uint32_t lcrc = masked(crc32c((const uint8_t*)head, 8)), dcrc = masked(crc32c((const uint8_t*)ex.data(), ex.size()));
    memcpy(head + 8, &lcrc, 4);
    out.append(head, 12);
    out += ex;
    out.append((const char*)&dcrc, 4);
}

template <typename F>
int guarded(const char* fn, F&& body)
{
    try {
        return body();
    } catch (const Refused& r) {
        rd_set_error("%s: %s", fn, r.why.c_str());
        return RD_ERR_FORMAT;
    } catch (const std::bad_alloc&) {
        rd_set_error("%s: out of host memory", fn);
        return RD_ERR_NOMEM;
    }
}

}  // namespace

extern "C" uint32_t rd_crc32c(const void* buf, size_t n) { return crc32c((const uint8_t*)buf, n); }

extern "C" int rd_tfrecord_open_mem(const void* buf, size_t n, rd_tfrecord** out)
{
    RD_REQUIRE(out && (buf || n == 0), "rd_tfrecord_open_mem: null argument");
    *out = nullptr;
    return guarded("rd_tfrecord_open_mem", [&]() {
        rd_tfrecord* f = new rd_tfrecord();
        try {
            index_shard((const uint8_t*)buf, n, f);
        } catch (...) {
            delete f;
            throw;
        }
        *out = f;
        return RD_OK;
    });
}

extern "C" int rd_tfrecord_open(const char* path, rd_tfrecord** out)
{
    RD_REQUIRE(path && out, "rd_tfrecord_open: null argument");
    *out = nullptr;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
        rd_set_error("rd_tfrecord_open: cannot open %s: %s", path, strerror(errno));
        return RD_ERR_IO;
    }
    struct stat st;
    if (fstat(fd, &st) != 0) {
        rd_set_error("rd_tfrecord_open: cannot stat %s: %s", path, strerror(errno));
        close(fd);
        return RD_ERR_IO;
    }
    const size_t n = (size_t)st.st_size;
    void* map = nullptr;
    if (n) {
        map = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (map == MAP_FAILED) {
            rd_set_error("rd_tfrecord_open: cannot map %s: %s", path, strerror(errno));
            close(fd);
            return RD_ERR_IO;
        }
    }
    close(fd);
    const int rc = rd_tfrecord_open_mem(map, n, out);
    if (map) munmap(map, n);
    if (rc == RD_ERR_FORMAT) {
        const std::string why = rd_last_error();
        rd_set_error("%s (%s)", why.c_str(), path);
    }
    return rc;
}

extern "C" void rd_tfrecord_close(rd_tfrecord* f) { delete f; }

extern "C" int rd_tfrecord_count(const rd_tfrecord* f, int64_t* n_records, int64_t* n_labels)
{
    RD_REQUIRE(f && n_records, "rd_tfrecord_count: null argument");
    *n_records = (int64_t)f->input_len.size();
    if (n_labels) *n_labels = (int64_t)f->labels.size();
    return RD_OK;
}

extern "C" int rd_tfrecord_read(const rd_tfrecord* f, int64_t lo, int64_t hi, float* signals, int32_t* input_len, int64_t* label_off,
                                int32_t* label_len, uint8_t* labels, int64_t labels_cap)
{
    RD_REQUIRE(f, "rd_tfrecord_read: null handle");
    const int64_t n = (int64_t)f->input_len.size();
    RD_REQUIRE(0 <= lo && lo <= hi && hi <= n, "rd_tfrecord_read: records [%lld, %lld) of %lld", (long long)lo, (long long)hi, (long long)n);
    RD_REQUIRE(lo == hi || (signals && input_len && label_off && label_len), "rd_tfrecord_read: null argument");
    const int64_t l0 = f->label_off[(size_t)lo], nl = f->label_off[(size_t)hi] - l0;
    RD_REQUIRE(nl <= labels_cap && (nl == 0 || labels), "rd_tfrecord_read: %lld labels, capacity %lld", (long long)nl, (long long)labels_cap);
    if (lo == hi) {
        if (label_off) label_off[0] = 0;
        return RD_OK;
    }
    memcpy(signals, f->signal.data() + (size_t)lo * TF_WIN, (size_t)(hi - lo) * TF_WIN * sizeof(float));
    memcpy(input_len, f->input_len.data() + lo, (size_t)(hi - lo) * sizeof(int32_t));
    for (int64_t r = lo; r <= hi; r++) label_off[r - lo] = f->label_off[(size_t)r] - l0;
    for (int64_t r = lo; r < hi; r++) label_len[r - lo] = (int32_t)(f->label_off[(size_t)r + 1] - f->label_off[(size_t)r]);
    if (nl) memcpy(labels, f->labels.data() + l0, (size_t)nl);
    return RD_OK;
}

extern "C" int rd_tfrecord_write(const char* path, const float* signals, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
                                 const int32_t* label_len, int64_t n, int append)
{
    RD_REQUIRE(path && n >= 0 && (n == 0 || (signals && input_len && label_off && label_len)), "rd_tfrecord_write: bad argument");
    for (int64_t r = 0; r < n; r++) {
        RD_REQUIRE(input_len[r] >= 1 && input_len[r] <= TF_WIN, "rd_tfrecord_write: record %lld: signal_length %d is outside 1..%d", (long long)r,
                   input_len[r], TF_WIN);
        RD_REQUIRE(label_len[r] >= 0 && label_off[r] >= 0 && (label_len[r] == 0 || labels), "rd_tfrecord_write: record %lld: label_length %d at offset %lld",
                   (long long)r, label_len[r], (long long)label_off[r]);
        for (int k = 0; k < label_len[r]; k++)
            RD_REQUIRE(labels[label_off[r] + k] <= 3, "rd_tfrecord_write: record %lld: label %d is %d, not one of 0, 1, 2, 3", (long long)r, k,
                       labels[label_off[r] + k]);
    }
    return guarded("rd_tfrecord_write", [&]() {
        FILE* f = fopen(path, append ? "ab" : "wb");
        if (!f) {
            rd_set_error("rd_tfrecord_write: cannot open %s: %s", path, strerror(errno));
            return RD_ERR_IO;
        }
        std::string buf;
        bool ok = true;
        for (int64_t r = 0; r < n && ok; r++) {
            put_example(buf, signals + (size_t)r * TF_WIN, input_len[r], labels ? labels + label_off[r] : nullptr, label_len[r]);
            if (buf.size() >= (4u << 20) || r + 1 == n) {
                ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
                buf.clear();
            }
        }
        if (fclose(f) != 0) ok = false;
        if (!ok) {
            rd_set_error("rd_tfrecord_write: writing %s failed: %s", path, strerror(errno));
            return RD_ERR_IO;
        }
        return RD_OK;
    });
}
