// Stand-alone driver of the Reduce batch's slab layout (gsc_reduce_layout.h:
// gsc::reduce_layout), meant for a host sanitizer build with no HIP in it:
//   make -C soundchunks_amd/csrc reduce_layout_check
// For 1, 2 and 3 frames, every K per frame out of 2, 255, 256, 257, 2048 and
// 4096 (equal and mixed), every N per frame out of K + 1, 513 and 6615, the row
// widths 8, 16 and 32, packed features and features at the caller's offsets:
// every frame's regions (clusters, counts by id and counts by position in dI,
// the four floats per point in dF, the centroids in dC, the tail slot) lie
// inside the returned totals; no two regions of a slab overlap; with equal K
// the offsets are those run_reduce_batch_dev wrote out by hand before the
// layout had one owner, with mixed K those of gsc_scan_reduce_frames, both
// restated here.  One line per frame count; exit status 0 when nothing failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

// gsc_device.h marks a few functions for the device compiler; a host compiler reads them as plain C++
#define __host__
#define __device__
#include "../../soundchunks_amd/csrc/gsc_reduce_layout.h"

namespace {

int g_bad = 0;
long g_cases = 0;

#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                  \
            std::printf("\n");                                         \
            ++g_bad;                                                   \
            return;                                                    \
        }                                                              \
    } while (0)

using Region = std::pair<int64_t, int64_t>;  // [first, second)

// inside [0, total) and pairwise disjoint
bool tiles(std::vector<Region> r, int64_t total) {
    std::sort(r.begin(), r.end());
    int64_t at = 0;
    for (const Region& x : r) {
        if (x.first < at || x.second < x.first || x.second > total) return false;
        at = x.second;
    }
    return true;
}

int padded(int K) {  // restated: the power of two at or above K, at least 256
    int k = 256;
    while (k < K) k *= 2;
    return k;
}

void check_case(int nf, const int* N, const int* K, int D, bool packed) {
    ++g_cases;
    std::vector<int64_t> xoff(static_cast<size_t>(nf));
    for (int i = 0; i < nf; ++i) xoff[size_t(i)] = 1000 + int64_t(i) * 7000 * D;  // a caller's slab with gaps
    const int dcol = D - 2;
    const gsc::ReduceLayout L = gsc::reduce_layout(nf, N, K, packed ? nullptr : xoff.data(), D, dcol);
    CHECK(int(L.frames.size()) == nf, "nf %d: %zu frames", nf, L.frames.size());
    int64_t nsum = 0, ksum = 0;
    int kmax = 0, nmax = 0;
    bool equal = true;
    for (int i = 0; i < nf; ++i) {
        nsum += N[i];
        ksum += K[i];
        kmax = std::max(kmax, K[i]);
        nmax = std::max(nmax, N[i]);
        equal = equal && K[i] == K[0];
    }
    const int Kp = padded(kmax);
    CHECK(L.points == nsum && L.max_n == nmax && L.max_k == kmax, "nf %d: sums", nf);
    std::vector<Region> rI, rF, rC, rT;
    int64_t no = 0, ko = 0;
    for (int i = 0; i < nf; ++i) {
        const gsc::ReduceFrame& f = L.frames[size_t(i)];
        CHECK(f.N == N[i] && f.K == K[i] && f.dcol == dcol, "frame %d: shape", i);
        CHECK(f.iters == 0 && f.done == 0 && f.generic == 0 && f.plain == 0 && !f.cl_host && !f.notify,
              "frame %d: outputs not zero", i);
        rI.push_back({f.n_off, f.n_off + N[i]});
        rI.push_back({f.k_off, f.k_off + K[i]});
        rI.push_back({f.ka_off, f.ka_off + padded(K[i])});  // the frame's own padded layout
        rF.push_back({f.n_off * 4, f.n_off * 4 + int64_t(N[i]) * 4});
        rC.push_back({f.c_off, f.c_off + int64_t(K[i]) * D});
        rT.push_back({f.t_off, f.t_off + int64_t(4096) * 16});
        // gsc_scan_reduce_frames, as it stood
        CHECK(f.x_off == (packed ? no * D : xoff[size_t(i)]), "frame %d: x_off %lld", i, (long long)f.x_off);
        CHECK(f.c_off == ko * D && f.n_off == no && f.k_off == nsum + ko && f.ka_off == nsum + ksum + int64_t(i) * Kp &&
                  f.t_off == int64_t(i) * 4096 * 16,
              "frame %d of %d: mixed-K offsets", i, nf);
        if (equal) {  // run_reduce_batch_dev, as it stood
            const int64_t k = K[0];
            CHECK(f.c_off == int64_t(i) * k * D && f.k_off == nsum + int64_t(i) * k &&
                      f.ka_off == nsum + int64_t(nf) * k + int64_t(i) * Kp,
                  "frame %d of %d: equal-K offsets", i, nf);
        }
        no += N[i];
        ko += K[i];
    }
    CHECK(L.nI == size_t(nsum + ksum + int64_t(nf) * Kp) && L.nF == size_t(nsum) * 4 && L.nC == size_t(ksum) * size_t(D) &&
              L.nT == size_t(nf) * 4096 * 16,
          "nf %d: totals", nf);
    if (equal) CHECK(L.nI == size_t(nsum + int64_t(nf) * (K[0] + Kp)) && L.nC == size_t(nf) * size_t(K[0]) * size_t(D), "nf %d: equal-K totals", nf);
    CHECK(tiles(rI, int64_t(L.nI)), "nf %d: dI regions leave the slab or overlap", nf);
    CHECK(tiles(rF, int64_t(L.nF)), "nf %d: dF regions leave the slab or overlap", nf);
    CHECK(tiles(rC, int64_t(L.nC)), "nf %d: dC regions leave the slab or overlap", nf);
    CHECK(tiles(rT, int64_t(L.nT)), "nf %d: tail slots leave the slab or overlap", nf);
}

}  // namespace

int main() {
    const int Ks[] = {2, 255, 256, 257, 2048, 4096};
    for (int nf = 1; nf <= 3; ++nf) {
        const long before = g_cases;
        int kc = 1, nc = 1;
        for (int i = 0; i < nf; ++i) kc *= 6, nc *= 3;
        for (int kc_i = 0; kc_i < kc; ++kc_i)
            for (int nc_i = 0; nc_i < nc; ++nc_i) {
                int K[3], N[3];
                for (int i = 0, a = kc_i, b = nc_i; i < nf; ++i, a /= 6, b /= 3) {
                    K[i] = Ks[a % 6];
                    const int Ns[] = {K[i] + 1, 513, 6615};
                    N[i] = Ns[b % 3];
                }
                for (int D : {8, 16, 32})
                    for (bool packed : {true, false}) check_case(nf, N, K, D, packed);
            }
        std::printf("frames %d: %ld layouts\n", nf, g_cases - before);
    }
    if (g_bad) std::printf("%d check(s) failed\n", g_bad);
    return g_bad ? 1 : 0;
}
