// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host halves of the RNA-model builder: rd_fasta_scan (radian_amd/csrc/lmbuild.hip)
// and rd_lm_json_write (radian_amd/csrc/lmjson.hip).  Sanitizers run on the CPU build only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
extern "C" int rd_fasta_scan(const char* buf, size_t n, int field, const char* value, uint8_t* codes, int64_t* offsets, int64_t* counts);
extern "C" int rd_lm_json_write(const char* path, const double* table, int k, int64_t* n_rows, int64_t* n_bytes);
extern "C" int rd_lm_json_probe(const char* buf, size_t n, int* k_out);
extern "C" int rd_lm_json_fill(const char* buf, size_t n, int k, double* table, int64_t* n_entries, int64_t* n_contexts);
void rd_set_error(const char* fmt, ...) { (void)fmt; }

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            return 1;                                                \
        }                                                            \
    } while (0)

int main(int argc, char** argv)
{
    std::mt19937_64 rng(11);
    static const char alphabet[] = ">|ACGTUNacgtun*- \r\n\t\n\n19;\x00\xff_pc";
    const size_t n_alpha = sizeof(alphabet) - 1;
    const int iters = argc > 1 ? atoi(argv[1]) : 100000;
    const char* path = argc > 2 ? argv[2] : "/tmp/asan_fasta.json";
    long ok = 0, total = 0;
    for (int it = 0; it < iters; it++) {
        std::string s;
        if (it % 3) {   // a valid FASTA, then mutated
            const int n = rng() % 6;
            for (int i = 0; i < n; i++) {
                s += ">id" + std::to_string(i) + (rng() % 2 ? "|x|pc|" : "|y") + (rng() % 4 ? "\n" : "\r\n");
                const int lines = rng() % 4;
                for (int l = 0; l < lines; l++) {
                    const int len = rng() % 30;
                    for (int j = 0; j < len; j++) s += "ACGTUNacgtn*-"[rng() % 13];
                    if (l + 1 < lines || i + 1 < n || rng() % 2) s += (rng() % 4 ? "\n" : "\r\n");
                }
            }
            const int muts = rng() % 3;
            for (int m = 0; m < muts && !s.empty(); m++) {
                const size_t pos = rng() % s.size();
                switch (rng() % 3) {
                    case 0: s[pos] = alphabet[rng() % n_alpha]; break;
                    case 1: s.erase(pos, 1 + rng() % 3); break;
                    default: s.insert(pos, 1, alphabet[rng() % n_alpha]); break;
                }
            }
            if (rng() % 8 == 0) s.resize(rng() % (s.size() + 1));
        } else {
            const int n = rng() % 50;
            for (int i = 0; i < n; i++) s += alphabet[rng() % n_alpha];
        }
        char* buf = (char*)malloc(s.size() ? s.size() : 1);            // exact size: a read past the end is an ASan error
        memcpy(buf, s.data(), s.size());
        const int field = (int)(rng() % 5) - 1;
        const char* value = rng() % 2 ? "pc" : "";
        int64_t c1[3] = {0, 0, 0}, c2[3] = {0, 0, 0};
        total++;
        if (rd_fasta_scan(buf, s.size(), field, value, nullptr, nullptr, c1) == 0) {
            uint8_t* codes = (uint8_t*)malloc(c1[2] ? (size_t)c1[2] : 1);      // exact sizes again
            int64_t* offsets = (int64_t*)malloc((size_t)(c1[1] + 1) * sizeof(int64_t));
            CHECK(rd_fasta_scan(buf, s.size(), field, value, codes, offsets, c2) == 0);
            CHECK(c1[0] == c2[0] && c1[1] == c2[1] && c1[2] == c2[2] && c1[1] <= c1[0]);
            CHECK(offsets[0] == 0 && offsets[c1[1]] == c1[2]);
            for (int64_t r = 0; r < c1[1]; r++) CHECK(offsets[r] <= offsets[r + 1]);
            for (int64_t i = 0; i < c1[2]; i++) CHECK(codes[i] < 4 || codes[i] == 255);
            free(codes);
            free(offsets);
            ok++;
        }
        free(buf);
        if (it % 400 == 0) {   // the writer: a table with NaN rows and extreme values, written and read back by the library's reader
            const int k = 1 + (int)(rng() % 4);
            const size_t n = (size_t)1 << (2 * k);
            double* t = (double*)malloc(n * 4 * sizeof(double));
            const double special[] = {0.0, 1.0, 5e-324, 1e-310, 0.1, 1.0 / 3.0, 1.7976931348623157e308, 2.2250738585072014e-308, 1e22};
            for (size_t c = 0; c < n; c++)
                for (int i = 0; i < 4; i++) t[c * 4 + i] = rng() % 3 ? (double)(rng() % 100000) / 100000.0 * (rng() % 5 ? 1 : 1e-300) : special[rng() % 9];
            for (size_t c = 1; c < n; c++)
                if (rng() % 4 == 0)
                    for (int i = 0; i < 4; i++) t[c * 4 + i] = NAN;
            int64_t rows = 0, bytes = 0;
            CHECK(rd_lm_json_write(path, t, k, &rows, &bytes) == 0);
            FILE* f = fopen(path, "rb");
            CHECK(f);
            char* text = (char*)malloc((size_t)bytes);
            CHECK(fread(text, 1, (size_t)bytes, f) == (size_t)bytes && fgetc(f) == EOF);
            fclose(f);
            int kk = 0;
            CHECK(rd_lm_json_probe(text, (size_t)bytes, &kk) == 0 && kk == k);
            std::vector<double> back(n * 4, NAN);
            int64_t ne = 0, nc = 0;
            CHECK(rd_lm_json_fill(text, (size_t)bytes, k, back.data(), &ne, &nc) == 0 && ne == rows && nc == rows);
            for (size_t i = 0; i < n * 4; i++) CHECK((std::isnan(t[i]) && std::isnan(back[i])) || memcmp(&t[i], &back[i], 8) == 0);
            t[5] = -1.0;
            CHECK(rd_lm_json_write(path, t, k, &rows, &bytes) != 0);
            t[5] = INFINITY;
            CHECK(rd_lm_json_write(path, t, k, &rows, &bytes) != 0);
            free(text);
            free(t);
        }
    }
    printf("%ld of %ld texts accepted, no sanitizer report\n", ok, total);
    return 0;
}
