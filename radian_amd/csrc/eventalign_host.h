// eventalign_host.h -- host only: the window's own scale in plain loops, for the host twins (rd_eventalign_host, rd_sigmap_host).  The rule
// is eventalign_rules.h's text: m2 = the sum of the two middle order statistics, d4 = the same of |2x - m2|.
#pragma once
#include <stdint.h>
#include <vector>

// the two middle order statistics of n keys counted in cnt[0 .. n_keys)
inline int32_t ea_middle2(const std::vector<int64_t>& cnt, int n_keys, int64_t n)
{
    const int64_t k1 = (n - 1) / 2, k2 = n / 2;
    int64_t c = 0;
    int v1 = -1, v2 = -1;
    for (int k = 0; k < n_keys; k++) {
        c += cnt[k];
        if (v1 < 0 && k1 < c) v1 = k;
        if (v2 < 0 && k2 < c) { v2 = k; break; }
    }
    return v1 + v2;
}

// the scale of T >= 1 samples, as rd_polya_segment's
inline void ea_host_scale(const int16_t* x, int64_t T, std::vector<int64_t>& cnt, int32_t* m2, int32_t* d4)
{
    cnt.assign(65536, 0);
    for (int64_t i = 0; i < T; i++) cnt[(int)x[i] + 32768]++;
    *m2 = ea_middle2(cnt, 65536, T) - 65536;
    cnt.assign(131072, 0);
    for (int64_t i = 0; i < T; i++) {
        const int v = 2 * (int)x[i] - *m2;
        cnt[v < 0 ? -v : v]++;
    }
    *d4 = ea_middle2(cnt, 131072, T);
}
