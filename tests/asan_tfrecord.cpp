// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for radian_amd/csrc/tfrecord.hip (host code; sanitizers run on the CPU build only).
// usage: asan_tfrecord <iterations> <shard.tfrecords>...   Every shard is parsed from an exact-size heap copy (a read past either end is an
// ASan report) and every record copied out; then `iterations` truncated / corrupted copies per shard go through the same calls -- half of
// them with the checksums recomputed after the mutation, so that the protobuf decoder sees the damage.  Whatever the reader answers
// (RD_OK, RD_ERR_FORMAT) is fine -- it must not touch memory outside the image or its output arrays.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
struct rd_tfrecord;
extern "C" int rd_tfrecord_open_mem(const void* buf, size_t n, rd_tfrecord** out);
extern "C" void rd_tfrecord_close(rd_tfrecord* f);
extern "C" int rd_tfrecord_count(const rd_tfrecord* f, int64_t* n_records, int64_t* n_labels);
extern "C" int rd_tfrecord_read(const rd_tfrecord* f, int64_t lo, int64_t hi, float* signals, int32_t* input_len, int64_t* label_off,
                                int32_t* label_len, uint8_t* labels, int64_t labels_cap);
extern "C" uint32_t rd_crc32c(const void* buf, size_t n);
void rd_set_error(const char* fmt, ...) { (void)fmt; }
extern "C" const char* rd_last_error() { return ""; }

static long g_opened = 0, g_refused = 0, g_records = 0;

static uint32_t masked(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

static void drive(const std::vector<uint8_t>& img)
{
    const size_t n = img.size();
    uint8_t* buf = (uint8_t*)malloc(n ? n : 1);   // exact size
    if (n) memcpy(buf, img.data(), n);
    rd_tfrecord* f = nullptr;
    if (rd_tfrecord_open_mem(buf, n, &f) == 0) {
        g_opened++;
        int64_t cnt = 0, nl = 0;
        rd_tfrecord_count(f, &cnt, &nl);
        float* sig = (float*)malloc((size_t)(cnt ? cnt : 1) * 1024 * 4);   // exact sizes again
        int32_t* il = (int32_t*)malloc((size_t)(cnt ? cnt : 1) * 4);
        int64_t* off = (int64_t*)malloc((size_t)(cnt + 1) * 8);
        int32_t* ll = (int32_t*)malloc((size_t)(cnt ? cnt : 1) * 4);
        uint8_t* lab = (uint8_t*)malloc((size_t)(nl ? nl : 1));
        if (rd_tfrecord_read(f, 0, cnt, sig, il, off, ll, lab, nl) == 0) g_records += cnt;
        free(sig), free(il), free(off), free(ll), free(lab);
        rd_tfrecord_close(f);
    } else {
        g_refused++;
    }
    free(buf);
}

// recompute every frame's checksums (as far as the frames parse)
static void reframe(std::vector<uint8_t>& b)
{
    size_t at = 0;
    while (b.size() - at >= 12) {
        uint64_t len;
        memcpy(&len, b.data() + at, 8);
        const uint32_t lc = masked(rd_crc32c(b.data() + at, 8));
        memcpy(b.data() + at + 8, &lc, 4);
        at += 12;
        if (len > b.size() - at || b.size() - at - len < 4) return;
        const uint32_t dc = masked(rd_crc32c(b.data() + at, (size_t)len));
        memcpy(b.data() + at + len, &dc, 4);
        at += (size_t)len + 4;
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int iters = atoi(argv[1]);
    std::mt19937_64 rng(12345);
    for (int a = 2; a < argc; a++) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) return 3;
        std::vector<uint8_t> img;
        uint8_t tmp[65536];
        size_t k;
        while ((k = fread(tmp, 1, sizeof tmp, fp)) > 0) img.insert(img.end(), tmp, tmp + k);
        fclose(fp);
        const long before = g_records;
        drive(img);
        printf("%s: %ld records\n", argv[a], g_records - before);
        for (int it = 0; it < iters; it++) {
            std::vector<uint8_t> m = img;
            const int kind = (int)(rng() % 4);
            if (kind == 0 && !m.empty()) {
                m.resize(rng() % m.size());   // truncated
            } else {
                const int flips = 1 + (int)(rng() % 8);
                for (int f = 0; f < flips && !m.empty(); f++) {
                    const size_t at = rng() % m.size();
                    if (rng() % 3 == 0)
                        m[at] = 0xff;
                    else
                        m[at] ^= (uint8_t)(1u << (rng() % 8));
                }
                if (kind >= 2) reframe(m);
            }
            drive(m);
        }
    }
    printf("no sanitizer report\n%ld opened %ld refused\n", g_opened, g_refused);
    return 0;
}
