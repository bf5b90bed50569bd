// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/pileup.hip (the argument checks, the op
// validator, the rules of pileup_rules.h, the plain loops of rd_pileup_host; sanitizers run on the CPU build only -- the kernels are not
// compiled here).  usage: asan_pileup <iterations>   The rules at their limits first.  Every iteration draws pairs whose column strings
// are random mixtures of M / X / D / I runs (runs of 64 and more, leading and trailing gaps, pairs without an M / X column, empty pairs
// among them) into EXACT-SIZE heap buffers (a read or a write past either end is an ASan report), calls the host twin and checks every
// table entry and per-pair field against a loop of its own written from the contract's text; then the same buffers go through the
// refusals, which must answer RD_ERR_ARG and write nothing.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../radian_amd/csrc/pileup.hip"   // the host half (this is no HIP build): the device blocks' layout functions live in its unnamed namespace

extern "C" int rd_pileup_host(const uint8_t* ops, const int64_t* ops_off, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads,
                              const int64_t* read_off, int n_pairs, const int64_t* site0, int64_t n_sites, uint32_t* sites, uint64_t* profile,
                              int32_t* out);
void rd_set_error(const char* fmt, ...) { (void)fmt; }

static long g_accepted = 0, g_refused = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            exit(1);                                                     \
        }                                                                \
    } while (0)

template <typename T> static T* exact(const std::vector<T>& v)
{
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// the contract over one pair, column by column with explicit run bookkeeping from the left AND the position arrays (not the library's loop)
static void own_pair(const std::string& o, const std::string& A, const std::string& B, int64_t s0, std::vector<uint32_t>& site,
                     std::vector<uint64_t>& prof, int32_t* res)
{
    const int64_t L = (int64_t)o.size();
    std::vector<int64_t> ri(L), qj(L);
    int64_t i = 0, j = 0, lo = -1, hi = -1;
    for (int64_t k = 0; k < L; k++) {
        ri[k] = i, qj[k] = j;
        if (o[k] == 'M' || o[k] == 'X') {
            if (lo < 0) lo = k;
            hi = k;
        }
        i += o[k] != 'I';
        j += o[k] != 'D';
    }
    for (int c = 0; c < PILEUP_RES; c++) res[c] = 0;
    if (lo < 0) {
        res[0] = PILEUP_NO_BASE;
        res[4] = (int32_t)B.size();
        return;
    }
    const auto ctx = [&](int64_t at, int e) {
        const int km = pileup_kmer((const uint8_t*)A.data(), (int64_t)A.size(), at);
        if (km >= 0) prof[PILEUP_KMER + km * 4 + e]++;
    };
    site[(s0 + ri[lo]) * 8 + 7]++;
    for (int64_t k = lo; k <= hi;) {
        int64_t e = k;
        while (e + 1 <= hi && o[e + 1] == o[k]) e++;
        const int64_t len = e - k + 1;
        for (int64_t c = k; c <= e; c++) {
            if (o[k] == 'M' || o[k] == 'X') {
                const int ca = pileup_code((uint8_t)A[ri[c]]), cb = pileup_code((uint8_t)B[qj[c]]);
                site[(s0 + ri[c]) * 8 + cb]++;
                prof[PILEUP_CONF + ca * 6 + cb]++;
                ctx(ri[c], o[k] == 'M' ? 0 : 1);
                res[o[k] == 'M' ? 6 : 7]++;
            } else if (o[k] == 'D') {
                site[(s0 + ri[c]) * 8 + 5]++;
                prof[PILEUP_CONF + pileup_code((uint8_t)A[ri[c]]) * 6 + 5]++;
                ctx(ri[c], 2);
                res[9]++;
            } else {
                prof[PILEUP_INS_BASE + pileup_code((uint8_t)B[qj[c]])]++;
                res[8]++;
            }
        }
        if (o[k] == 'D') prof[PILEUP_DEL_LEN + (len >= 64 ? 63 : len - 1)]++;
        if (o[k] == 'I') {
            prof[PILEUP_INS_LEN + (len >= 64 ? 63 : len - 1)]++;
            site[(s0 + ri[k] - 1) * 8 + 6]++;   // the run lies between span offsets ri - 1 and ri
            ctx(ri[k] - 1, 3);
        }
        k = e + 1;
    }
    res[2] = (int32_t)ri[lo];
    res[3] = (int32_t)ri[hi] + 1;
    res[4] = (int32_t)qj[lo];
    res[5] = (int32_t)((int64_t)B.size() - qj[hi] - 1);
}

// The yardsticks of pu_ops_layout / pu_ops_pair and pu_read_layout: the offset expressions that rd_pileup_add_ops and the two phases of
// rd_pileup_read held before the layout functions replaced them, written out literally; on seeded random dimensions (0 and 1 of each among
// them) the totals and every offset must be equal.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    char* const base = (char*)((uintptr_t)1 << 32);
    for (int it = 0; it < 4000; it++) {
        const int nb = (int)dim(300);
        std::vector<int64_t> n(nb), m(nb), L(nb);
        for (int k = 0; k < nb; k++) n[k] = (int64_t)dim(3000), m[k] = (int64_t)dim(3000), L[k] = (int64_t)dim(6000);
        const size_t res_at = align_up((size_t)nb * sizeof(AlnPair), 256), site_at = res_at + align_up((size_t)nb * ALN_RES * 4, 256);
        const size_t out_at = site_at + align_up((size_t)nb * 8, 256);
        size_t at = out_at + align_up((size_t)nb * PILEUP_RES * 4, 256);
        Carve c;
        PuOpsAt o;
        pu_ops_layout(c, nb, &o);
        CHECK(o.res == res_at && o.site == site_at && o.out == out_at && c.at == at);
        for (int k = 0; k < nb; k++) {
            AlnPair d, e;
            d.n = (int32_t)n[k];
            d.m = (int32_t)m[k];
            d.ref = (int64_t)at;
            d.read = d.ref + d.n;
            d.ops = d.read + d.m;
            d.bnd = d.dir = 0;
            at += (size_t)d.n + d.m + (size_t)L[k];
            pu_ops_pair(c, n[k], m[k], L[k], &e);
            CHECK(e.n == d.n && e.m == d.m && e.ref == d.ref && e.read == d.read && e.ops == d.ops && e.bnd == 0 && e.dir == 0 && c.at == at);
        }
        // rd_pileup_read: the first phase reserves up to the rows, the second the rows as well
        const int64_t S = (int64_t)dim(3000000), need = (int64_t)dim(1000000);
        const size_t scan_bytes = dim(100000);
        const size_t pos_at = align_up((size_t)S * 4, 256), tmp_at = pos_at + align_up((size_t)S * 4, 256), rows_at = tmp_at + align_up(scan_bytes, 256);
        const size_t counts_at = rows_at + align_up((size_t)need * 4, 256), total = counts_at + (size_t)need * PILEUP_CH * 4;
        PuReadWs w;
        Carve dry0, dry1, wet(base);
        pu_read_layout(dry0, S, scan_bytes, 0, &w);
        CHECK(dry0.at == rows_at && !w.flag && !w.site);
        pu_read_layout(dry1, S, scan_bytes, need, &w);
        CHECK(dry1.at == total);
        pu_read_layout(wet, S, scan_bytes, need, &w);
        CHECK(wet.at == total && (char*)w.flag == base && (char*)w.pos == base + pos_at && (char*)w.tmp == base + tmp_at && (char*)w.site == base + rows_at &&
              (char*)w.counts == base + counts_at);
    }
}

int main(int argc, char** argv)
{
    const long iters = argc > 1 ? atol(argv[1]) : 20;
    check_layout();
    // the rules at their limits
    CHECK(pileup_code('A') == 0 && pileup_code('C') == 1 && pileup_code('G') == 2 && pileup_code('T') == 3 && pileup_code('N') == 4 && pileup_code('a') == 4 &&
          pileup_code('U') == 4 && pileup_code(0) == 4 && pileup_code(255) == 4);
    CHECK(pileup_len_bucket(1) == 0 && pileup_len_bucket(63) == 62 && pileup_len_bucket(64) == 63 && pileup_len_bucket(65) == 63 &&
          pileup_len_bucket(((int64_t)1 << 28)) == 63);
    {
        const uint8_t s[] = "ACGTACGTNA";
        CHECK(pileup_kmer(s, 10, 0) == -1 && pileup_kmer(s, 10, 1) == -1 && pileup_kmer(s, 10, 7) == -1 && pileup_kmer(s, 10, 8) == -1 && pileup_kmer(s, 10, 9) == -1);
        CHECK(pileup_kmer(s, 10, 2) == ((0 * 4 + 1) * 4 + 2) * 16 + 3 * 4 + 0 && pileup_kmer(s, 10, 5) == ((3 * 4 + 0) * 4 + 1) * 16 + 2 * 4 + 3);
        CHECK(pileup_kmer(s, 10, 6) == -1 && pileup_kmer(s, 4, 2) == -1 && pileup_kmer(s, 5, 2) >= 0 && pileup_kmer(s, 0, 0) == -1);
        const uint8_t t[] = "TTTTT";
        CHECK(pileup_kmer(t, 5, 2) == 1023);
    }
    CHECK(PILEUP_PROFILE_LEN == 4259 && PILEUP_KMER + 4 * 1023 + 3 == PILEUP_INS_LEN - 1 && PILEUP_INS_LEN + 64 == PILEUP_DEL_LEN);
    std::mt19937_64 rng(2323);
    auto uni = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
    const char letters[] = "ACGTACGTACGTNau";
    for (long it = 0; it < iters; it++) {
        const int P = (int)uni(0, 8);
        std::vector<std::string> O(P), A(P), B(P);
        std::vector<int64_t> s0(P);
        int64_t n_sites = 1;
        for (int p = 0; p < P; p++) {
            const int n_runs = (int)uni(0, 9);
            const int flavour = (int)uni(0, 9);   // 0: gaps only
            for (int r = 0; r < n_runs; r++) {
                const char kind = flavour == 0 ? "DI"[uni(0, 1)] : "MMMXDI"[uni(0, 5)];
                const int64_t len_choices[6] = {1, 2, uni(1, 9), uni(1, 9), 64, uni(60, 140)};
                O[p].append((size_t)len_choices[uni(0, 5)], kind);
            }
            for (char c : O[p]) {
                if (c != 'I') A[p].push_back(letters[uni(0, 14)]);
                if (c != 'D') B[p].push_back(letters[uni(0, 14)]);
            }
            s0[p] = uni(0, 40);
            n_sites = std::max(n_sites, s0[p] + (int64_t)A[p].size());
        }
        n_sites += uni(0, 3);
        std::vector<uint8_t> ops, refs, reads;
        std::vector<int64_t> ooff(1, 0), roff(1, 0), qoff(1, 0);
        for (int p = 0; p < P; p++) {
            ops.insert(ops.end(), O[p].begin(), O[p].end());
            refs.insert(refs.end(), A[p].begin(), A[p].end());
            reads.insert(reads.end(), B[p].begin(), B[p].end());
            ooff.push_back((int64_t)ops.size()), roff.push_back((int64_t)refs.size()), qoff.push_back((int64_t)reads.size());
        }
        uint8_t *p_ops = exact(ops), *p_refs = exact(refs), *p_reads = exact(reads);
        int64_t *p_ooff = exact(ooff), *p_roff = exact(roff), *p_qoff = exact(qoff), *p_s0 = exact(s0);
        const size_t sb = (size_t)n_sites * 8 * 4, pb = (size_t)PILEUP_PROFILE_LEN * 8, ob = (size_t)P * PILEUP_RES * 4;
        uint32_t* sites = (uint32_t*)calloc(1, sb);
        uint64_t* prof = (uint64_t*)calloc(1, pb);
        int32_t* out = (int32_t*)malloc(ob ? ob : 1);
        CHECK(rd_pileup_host(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out) == 0);
        g_accepted++;
        {
            std::vector<uint32_t> es((size_t)n_sites * 8, 0);
            std::vector<uint64_t> ep((size_t)PILEUP_PROFILE_LEN, 0);
            std::vector<int32_t> eo((size_t)P * PILEUP_RES + 1);
            for (int p = 0; p < P; p++) own_pair(O[p], A[p], B[p], s0[p], es, ep, &eo[(size_t)p * PILEUP_RES]);
            CHECK(memcmp(es.data(), sites, sb) == 0);
            CHECK(memcmp(ep.data(), prof, pb) == 0);
            CHECK(ob == 0 || memcmp(eo.data(), out, ob) == 0);
            // a second call ADDS: every counter doubles
            CHECK(rd_pileup_host(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out) == 0);
            for (size_t k = 0; k < es.size(); k++) CHECK(sites[k] == 2 * es[k]);
            for (size_t k = 0; k < ep.size(); k++) CHECK(prof[k] == 2 * ep[k]);
        }
        // the refusals: RD_ERR_ARG, nothing written
        auto refused = [&](const uint8_t* o, const int64_t* oo, const uint8_t* rf, const int64_t* ro, const uint8_t* rd, const int64_t* qo, int n,
                           const int64_t* s, int64_t ns, uint32_t* st, uint64_t* pr, int32_t* ou) {
            memset(sites, 0x4d, sb);
            memset(prof, 0x4d, pb);
            memset(out, 0x4d, ob);
            CHECK(rd_pileup_host(o, oo, rf, ro, rd, qo, n, s, ns, st, pr, ou) == -1);
            for (size_t k = 0; k < sb; k++) CHECK(((unsigned char*)sites)[k] == 0x4d);
            for (size_t k = 0; k < pb; k++) CHECK(((unsigned char*)prof)[k] == 0x4d);
            for (size_t k = 0; k < ob; k++) CHECK(((unsigned char*)out)[k] == 0x4d);
            g_refused++;
        };
        refused(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, -1, p_s0, n_sites, sites, prof, out);
        refused(p_ops, nullptr, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out);
        refused(p_ops, p_ooff, p_refs, nullptr, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out);
        refused(p_ops, p_ooff, p_refs, p_roff, p_reads, nullptr, P, p_s0, n_sites, sites, prof, out);
        refused(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, nullptr, out);
        refused(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, -1, sites, prof, out);
        refused(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, ((int64_t)1 << 30) + 1, sites, prof, out);
        if (P) {
            refused(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, nullptr, n_sites, sites, prof, out);
            refused(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, nullptr);
            const auto with_s0 = [&](int p, int64_t v) {
                auto copy = s0;
                copy[(size_t)p] = v;
                int64_t* q = exact(copy);
                refused(p_ops, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, q, n_sites, sites, prof, out);
                free(q);
            };
            with_s0((int)uni(0, P - 1), -1);
            with_s0((int)uni(0, P - 1), n_sites + 1);
            for (int p = 0; p < P; p++)
                if (!A[p].empty()) {
                    with_s0(p, n_sites - (int64_t)A[p].size() + 1);   // one site past the table
                    break;
                }
            {
                auto copy = ooff;
                copy[0] = 1;
                int64_t* q = exact(copy);
                refused(p_ops, q, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out);
                free(q);
            }
        }
        if (!ops.empty()) {
            const auto with_op = [&](size_t k, uint8_t v) {
                auto copy = ops;
                copy[k] = v;
                uint8_t* q = exact(copy);
                refused(q, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out);
                free(q);
            };
            const size_t k = (size_t)uni(0, (int64_t)ops.size() - 1);
            with_op(k, 'S');
            with_op(k, 'm');
            with_op(k, 0);
            with_op(k, ops[k] == 'I' ? 'D' : 'I');   // a valid op that consumes other characters than the pair has
            refused(nullptr, p_ooff, p_refs, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out);
        }
        if (!refs.empty()) refused(p_ops, p_ooff, nullptr, p_roff, p_reads, p_qoff, P, p_s0, n_sites, sites, prof, out);
        if (!reads.empty()) refused(p_ops, p_ooff, p_refs, p_roff, nullptr, p_qoff, P, p_s0, n_sites, sites, prof, out);
        free(sites), free(prof), free(out), free(p_ops), free(p_refs), free(p_reads), free(p_ooff), free(p_roff), free(p_qoff), free(p_s0);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
