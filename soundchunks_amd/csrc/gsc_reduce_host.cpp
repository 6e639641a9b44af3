// Host side of TFrame.Reduce on the device: the KNNScanReduce round loop over
// the batched and the generic kernel, the batch driver of yakmo seeding + scan
// (run_reduce_batch_dev) with its diagnostics, and the drop-in test entry
// points that run the same kernels on caller arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/soundchunks.h"
#include "gsc_encode_host.h"
#include "gsc_launch.h"
#include "gsc_reduce_layout.h"

namespace gsc {

std::atomic<int> g_scan_rounds{0};

void compact_rows(std::vector<float>* v, int n, int dp, int d) {
    if (dp == d) return;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < d; ++k) (*v)[size_t(i) * d + k] = (*v)[size_t(i) * dp + k];
    v->resize(size_t(n) * d);
}

namespace {

// IntPower(10.0, -Precision) (encoder.lpr:761)
double scan_tolerance(int precision) {
    if (precision <= 0) return 1.0;
    double p = 1.0, base = 10.0;
    int i = precision;
    while (i > 0) {
        while ((i & 1) == 0) {
            i >>= 1;
            base = base * base;
        }
        --i;
        p = p * base;
    }
    return 1.0 / p;
}

// D in {8, 16, 32} and 2 <= K <= 4096: the batched speculative kernel
// (gsc_scan.hip) covers the pass (D = 32 with 2048 < K <= 4096 on one CU per
// frame in the split layout: the cepstrum half of each centroid in HBM).
bool batched_scan_shape(int D, int K) {
    if (std::getenv("GSC_SCAN_GENERIC")) return false;  // diagnostic switch
    return (D == 8 || D == 16 || D == 32) && K >= 2 && K <= 4096;
}

// The scan's experiment switches of the environment as the kernels' `opts`:
// bit 0 (diagnostic GSC_SCAN_FULL_A1): full-dimension A1 bounds in every pass
// bit 1 (GSC_SCAN_NO_PRUNE): no per-wave A1 pruning
// bits 8..15 (GSC_SCAN_KB): queries per speculative batch (below the kernel's 32)
// They exist only in a scan object built with -DGSC_SCAN_EXPERIMENTS
// (tools/build_variant.sh); the product build says so once and ignores them.
int scan_experiment_opts() {
    const char* full = std::getenv("GSC_SCAN_FULL_A1");
    const char* nopr = std::getenv("GSC_SCAN_NO_PRUNE");
    const char* kb = std::getenv("GSC_SCAN_KB");
    if (!full && !nopr && !kb) return 0;
    if (!gsc_scan_has_experiments()) {
        static std::atomic<bool> said{false};
        if (!said.exchange(true))
            std::fprintf(stderr,
                         "soundchunks:%s%s%s set, but the scan experiments are not compiled into this build "
                         "(tools/build_variant.sh NAME -DGSC_SCAN_EXPERIMENTS): ignored\n",
                         full ? " GSC_SCAN_FULL_A1" : "", nopr ? " GSC_SCAN_NO_PRUNE" : "", kb ? " GSC_SCAN_KB" : "");
        return 0;
    }
    return (full ? 1 : 0) | (nopr ? 2 : 0) | ((kb ? (std::atoi(kb) & 255) : 0) << 8);
}

// side stream and events of the batched scan, one set per device for the life
// of the process: the general instantiation runs beside the PLAIN one
// (gsc_scan.hip launch_scan).  `mu` serialises the enqueue of one round, so the
// fork / join events of two host threads do not interleave.
struct ScanFork {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    std::mutex mu;
    hipError_t err = hipSuccess;
    bool made = false;
};

ScanFork* scan_fork() {
    constexpr int kMaxDev = 64;
    static ScanFork forks[kMaxDev];
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    ScanFork& f = forks[dev];
    if (!f.made) {
        f.made = true;
        f.err = hipStreamCreateWithFlags(&f.side, hipStreamNonBlocking);
        if (f.err == hipSuccess) f.err = hipEventCreateWithFlags(&f.fork, hipEventDisableTiming);
        if (f.err == hipSuccess) f.err = hipEventCreateWithFlags(&f.join, hipEventDisableTiming);
    }
    return f.err == hipSuccess ? &f : nullptr;
}

// all KNNScanReduce passes of a batch laid out as L (its descriptors at dfr);
// converged frames exit early, the generic launch after a batched one only
// runs the frames the batched kernel handed over (NaN centroids)
hipError_t launch_scan_passes(int D, ReduceFrame* dfr, const ReduceLayout& L, const float* X, float* C, int* is,
                              float* fs, const float* rate, int precision) {
    const int nf = int(L.frames.size()), K = L.max_k;  // K: the largest of the call's frames
    const double tol = scan_tolerance(precision);
    const bool batched = batched_scan_shape(D, K);
    int logk = 0;
    while ((1 << logk) < padded_k(K)) ++logk;
    DevBuf<float> tails;  // split layout: every frame's tail features (ReduceFrame::t_off)
    if (batched && gsc_scan_tail_floats_per_frame(D, logk) > 0) {
        const hipError_t e = tails.alloc(L.nT);
        if (e != hipSuccess) return e;
    }
    // frame kinds to enqueue: no frame of this call is plain when K is not the
    // layout's power of two (a host fact); whether a row is NaN is not one, so
    // the general instantiation is always enqueued, on a stream of its own
    // (the split layout has no PLAIN object)
    const int kinds = batched && K == (1 << logk) && gsc_scan_has_plain(D, logk) ? 3 : 2;
    ScanFork* sf = kinds == 3 ? scan_fork() : nullptr;
    if (kinds == 3) {
        if (!sf) return hipErrorUnknown;
        // the frames' kind, once: it cannot change during the frame (descriptors start as general)
        const hipError_t e = gsc_launch_scan_classify(D, logk, dfr, nf, C, nullptr);
        if (e != hipSuccess) return e;
    }
    const int opts = batched ? scan_experiment_opts() : 0;
    int max_passes = kMaxScanIters;
    if (const char* e = std::getenv("GSC_SCAN_MAX_PASSES")) max_passes = std::max(1, std::min(kMaxScanIters, std::atoi(e)));
    // every launch advances each live frame by at least one pass (the batched
    // kernel runs a frame until it converges or meets a NaN pass, which the
    // generic launch then takes), so max_passes rounds always suffice
    std::vector<int32_t> flags(2 * static_cast<size_t>(nf));  // (done, generic) per frame
    static_assert(offsetof(ReduceFrame, generic) == offsetof(ReduceFrame, done) + sizeof(int32_t), "adjacent flags");
    for (int round = 0; round < max_passes; ++round) {
        if (batched) {
            hipError_t e;
            if (sf) {
                std::lock_guard<std::mutex> lk(sf->mu);
                e = gsc_launch_scan_batch(D, logk, dfr, nf, X, C, is, rate, tol, max_passes, opts, tails.p, kinds, nullptr,
                                          sf->side, sf->fork, sf->join);
            } else {
                e = gsc_launch_scan_batch(D, logk, dfr, nf, X, C, is, rate, tol, max_passes, opts, tails.p, kinds, nullptr,
                                          nullptr, nullptr, nullptr);
            }
            if (e != hipSuccess) return e;
            // the generic kernel runs only when the batched one handed a frame
            // over (an empty launch of it still costs ~30 ms: 256 large-LDS
            // workgroups); stop once every frame is done
            e = hipMemcpy2D(flags.data(), 2 * sizeof(int32_t), &dfr[0].done, sizeof(ReduceFrame), 2 * sizeof(int32_t),
                            size_t(nf), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return e;
            g_scan_rounds.fetch_add(1);
            bool any_generic = false, all_done = true;
            for (int i = 0; i < nf; ++i) {
                all_done = all_done && flags[2 * size_t(i)] != 0;
                any_generic = any_generic || flags[2 * size_t(i) + 1] != 0;
            }
            if (all_done) break;
            if (!any_generic) continue;
        }
        const hipError_t e = gsc_launch_scan_pass(D, dfr, nf, K, X, C, is, fs, rate, tol, max_passes, batched ? 1 : 0, nullptr);
        if (e != hipSuccess) return e;
        if (!batched) g_scan_rounds.fetch_add(1);  // the generic kernel runs one pass per round
    }
    return hipSuccess;
}

// rate = Single(1/sqrt(cnt)) for cnt in [0, n] (encoder.lpr:735)
std::vector<float> rate_table(int n) {
    std::vector<float> t(size_t(n) + 2);
    t[0] = 0.0f;
    for (int c = 1; c < int(t.size()); ++c) t[c] = float(1.0 / std::sqrt(double(c)));
    return t;
}

// GSC_HOST_TIMING / GSC_FRAME_STATS: what the descriptors of a finished batch say
void report_reduce_batch(const std::vector<ReduceFrame>& fr, int K) {
    const int nf = int(fr.size());
    if (std::getenv("GSC_HOST_TIMING")) {  // spread of the frames' finishing times (the scan tail)
        std::vector<uint64_t> t;
        for (int i = 0; i < nf; ++i)
            if (fr[i].t_done) t.push_back(fr[i].t_done);
        if (!t.empty()) {
            std::sort(t.begin(), t.end());
            const double last = double(t.back());
            auto at = [&](double q) { return (last - double(t[size_t(q * double(t.size() - 1))])) / 1e5; };
            std::fprintf(stderr, "scan tail: frames finished [ms before the last] min %.1f p10 %.1f p50 %.1f p90 %.1f\n",
                         at(0.0), at(0.1), at(0.5), at(0.9));
        }
    }
    if (std::getenv("GSC_FRAME_STATS")) {  // diagnostic: per-frame chain length and finishing time
        uint64_t t0 = ~0ull;
        for (int i = 0; i < nf; ++i)
            if (fr[i].t_done) t0 = std::min<uint64_t>(t0, fr[i].t_done);
        for (int i = 0; i < nf; ++i)
            std::fprintf(stderr, "frame %d: N %d passes %d slow %d restarts %d done +%.1f ms kind %s plain_passes %d\n", i,
                         fr[i].N, fr[i].iters, fr[i].slow, fr[i].restarts,
                         fr[i].t_done ? double(fr[i].t_done - t0) / 1e5 : -1.0, fr[i].plain ? "plain" : "general",
                         fr[i].plain_passes);
    }
    if (std::getenv("GSC_HOST_TIMING") && nf > 0 && fr[0].ystamps[6] + fr[0].ystamps[1] + fr[0].ystamps[2] != 0) {
        // stamps builds: yakmo phase clocks, mean over frames (cycles per pick)
        double m[16] = {};
        for (int i = 0; i < nf; ++i)
            for (int k = 0; k < 16; ++k) m[k] += double(fr[i].ystamps[k]) / double(nf) / double(K);
        std::fprintf(stderr,
                     "yakmo stamps [clk/pick]: chain pick %.0f fast %.0f slow %.0f wait %.0f (fast calls %.1f"
                     " slow blocks %.1f) | dist pick+sdlo %.0f compute %.0f wait %.0f | negative deltas dropped"
                     " per pick: chain %.3g dist %.3g\n",
                     m[0], m[1], m[2], m[3], m[4], m[5], m[8], m[9], m[10], m[6], m[14]);
    }
}

// GSC_SCAN_DEBUG: the counters of a stamps build for one frame
void report_scan_debug(const ReduceFrame& f) {
    std::fprintf(stderr, "scan: passes %d slow %d restarts %d loop_iters(last pass) %d err %.9g tree_exact %d"
                         " kind %s plain_passes %d\n",
                 f.iters, f.slow, f.restarts, f.loop_iters, f.err, f.tree_exact, f.plain ? "plain" : "general",
                 f.plain_passes);
    std::fprintf(stderr, "stamps [prep A1 A2 B2 part3 part4 B1 vcheck won setup soloA soloDFS a2win a2far a2box a2out]");
    for (int w = 0; w < 8; ++w) {
        std::fprintf(stderr, "\n  w%d:", w);
        for (int k = 0; k < 16; ++k) std::fprintf(stderr, " %.3g", double(f.stamps[w * 16 + k]));
    }
    std::fprintf(stderr, "\nA1 queries [home pruned evaluated | iterations fixups pending | clk: box+home midbarrier]"
                         "\n  (one-CU frames: stamps slot 'vcheck' = A1 after the mid barrier + vp_end, slot 'A1' = the V check)");
    for (int w = 0; w < 8; ++w) {
        std::fprintf(stderr, "\n  w%d:", w);
        for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %.4g", double(f.acounts[w * 8 + k]));
    }
    const uint64_t* x = f.xcounts;
    std::fprintf(stderr,
                 "\niterations [kind: count, cycles]: bubble %llu %.4g | with new queries %llu %.4g (new queries %llu)"
                 " | with fixups %llu %.4g | with a solo %llu %.4g | A2 queries on per-wave bounds %llu",
                 (unsigned long long)x[0], double(x[1]), (unsigned long long)x[2], double(x[3]),
                 (unsigned long long)x[8], (unsigned long long)x[4], double(x[5]), (unsigned long long)x[6],
                 double(x[7]), (unsigned long long)x[9]);
    std::fprintf(stderr, "\napproximate certificates failed: no unique minimum %llu, a far step not provable %llu",
                 (unsigned long long)x[10], (unsigned long long)x[11]);
    std::fprintf(stderr, "\nfailed queries by cause: snapshot uncertified %llu, c* moved past m2 %llu, V check %llu"
                 " (V check only %llu)", (unsigned long long)x[12], (unsigned long long)x[13],
                 (unsigned long long)x[14], (unsigned long long)x[15]);
    const uint64_t* x2 = f.xcounts2;
    std::fprintf(stderr, "\nsolo answer = speculative c*: by cause uncertified %llu, m2 %llu, V %llu | solos with a remainder"
                         " %llu, of them same answer %llu (remainder queries valid to the next failure %llu, whole"
                         " remainder valid %llu)", (unsigned long long)x2[0], (unsigned long long)x2[1],
                 (unsigned long long)x2[2], (unsigned long long)x2[3], (unsigned long long)x2[4],
                 (unsigned long long)x2[5], (unsigned long long)x2[6]);
    std::fprintf(stderr, "\nin-batch DFS answers %llu, of them failing at commit %llu", (unsigned long long)x2[8],
                 (unsigned long long)x2[9]);
    std::fprintf(stderr, "\n");
}

// rows of d floats -> rows of dp (trailing zeros)
std::vector<float> pad_rows(const float* x, int n, int d, int dp) {
    std::vector<float> v(size_t(n) * dp, 0.0f);
    for (int i = 0; i < n; ++i) std::memcpy(&v[size_t(i) * dp], x + size_t(i) * d, sizeof(float) * size_t(d));
    return v;
}

// KNNScanReduce of several frames in ONE launch, from the caller's centroids,
// with a K per frame: the same kernels as the encoder, the yakmo seeding
// skipped.  x / centroids / clusters are the frames' arrays one after another
// (ns[i] x d0, ks[i] x d0, ns[i]).
int scan_reduce_host(int nf, int d0, const int* ns, const float* x, const int* ks, float* centroids, int* clusters,
                     int precision, int* iters, int* plain, int* plain_passes, double* err, bool debug) {
    if (d0 <= 0 || d0 > 32) return set_last_error("KNNScanReduce kernels support 1 <= d <= 32 features");
    const int d = feature_stride((d0 + 1) / 2);  // padded with zero features (residual divides by d0)
    ReduceLayout L = reduce_layout(nf, ns, ks, nullptr, d, d0);
    std::vector<ReduceFrame>& fr = L.frames;
    const int nsum = int(L.points), ksum = int(L.nC / size_t(d));
    const std::vector<float> xp = pad_rows(x, nsum, d0, d);
    std::vector<float> cp = pad_rows(centroids, ksum, d0, d);
    DevBuf<float> dX, dC, dRate, dF;
    DevBuf<int> dI;
    DevBuf<ReduceFrame> dFr;
    HIP_TRY(dF.alloc(L.nF));
    HIP_TRY(dX.alloc(xp.size()));
    HIP_TRY(dC.alloc(cp.size()));
    HIP_TRY(dI.alloc(L.nI));
    HIP_TRY(dFr.alloc(size_t(nf)));
    const std::vector<float> rt = rate_table(L.max_n);
    HIP_TRY(dRate.alloc(rt.size()));
    HIP_TRY(hipMemcpy(dX.p, xp.data(), sizeof(float) * xp.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dC.p, cp.data(), sizeof(float) * cp.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dRate.p, rt.data(), sizeof(float) * rt.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dFr.p, fr.data(), sizeof(ReduceFrame) * size_t(nf), hipMemcpyHostToDevice));
    HIP_TRY(launch_scan_passes(d, dFr.p, L, dX.p, dC.p, dI.p, dF.p, dRate.p, precision));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(cp.data(), dC.p, sizeof(float) * cp.size(), hipMemcpyDeviceToHost));
    compact_rows(&cp, ksum, d, d0);
    std::memcpy(centroids, cp.data(), sizeof(float) * size_t(ksum) * d0);
    HIP_TRY(hipMemcpy(clusters, dI.p, sizeof(int) * size_t(nsum), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fr.data(), dFr.p, sizeof(ReduceFrame) * size_t(nf), hipMemcpyDeviceToHost));
    for (int i = 0; i < nf; ++i) {
        if (fr[i].loop_iters < 0)
            return set_last_error("KNNScanReduce: batched pipeline made no progress (guard tripped)");
        if (iters) iters[i] = fr[i].iters;
        if (plain) plain[i] = fr[i].plain;
        if (plain_passes) plain_passes[i] = fr[i].plain_passes;
        if (err) err[i] = fr[i].err;
    }
    if (debug && std::getenv("GSC_SCAN_DEBUG")) report_scan_debug(fr[0]);
    return 0;
}

}  // namespace

// ---- batched device stage (declared in gsc_encode_host.h) -------------------
int run_reduce_batch_dev(int D, int K, int precision, const std::vector<int>& Ns, const std::vector<int64_t>& xoff,
                         const float* dX, std::vector<float>* C, std::vector<int>* clusters, std::vector<int>* iters,
                         std::vector<int>* slow, long long* restarts, double* yakmo_ms, double* scan_ms, int* cl_host,
                         int* notify, int dcol) {
    // launches: one yakmo launch + kMaxScanIters scan launches per batch
    const int nf = int(Ns.size());
    if (nf == 0) return 0;
    if (D != 8 && D != 16 && D != 32)
        return set_last_error("KNNScanReduce kernels support D = 8, 16 or 32 (ChunkSize 4, 8, 16)");
    const std::vector<int> Ks(size_t(nf), K);
    ReduceLayout L = reduce_layout(nf, Ns.data(), Ks.data(), xoff.data(), D, dcol);
    std::vector<ReduceFrame>& fr = L.frames;
    if (cl_host && notify)
        for (int i = 0; i < nf; ++i) {
            fr[i].cl_host = cl_host + fr[i].n_off;
            fr[i].notify = notify + i;
        }
    DevBuf<float> dC, dF, dRate, dYSum;
    DevBuf<int> dI;
    DevBuf<uint32_t> dBits;
    DevBuf<ReduceFrame> dFr;
    HIP_TRY(dC.alloc(L.nC));
    HIP_TRY(dF.alloc(L.nF));
    HIP_TRY(dI.alloc(L.nI));
    if (L.max_n > gsc_yakmo_max_lds_points()) {  // long frames: yakmo's bitmap and prefix summaries in HBM
        HIP_TRY(dBits.alloc(gsc_yakmo_big_words(L.points, nf)));
        HIP_TRY(dYSum.alloc(gsc_yakmo_big_floats(L.points, nf)));
    }
    HIP_TRY(dFr.alloc(size_t(nf)));
    const std::vector<float> rt = rate_table(L.max_n);
    HIP_TRY(dRate.alloc(rt.size()));
    HIP_TRY(hipMemcpy(dRate.p, rt.data(), sizeof(float) * rt.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dFr.p, fr.data(), sizeof(ReduceFrame) * size_t(nf), hipMemcpyHostToDevice));
    Event e0, e1, e2;
    HIP_TRY(e0.create());
    HIP_TRY(e1.create());
    HIP_TRY(e2.create());
    HIP_TRY(hipEventRecord(e0.e, nullptr));
    HIP_TRY(gsc_launch_yakmo(D, dFr.p, nf, dX, dC.p, dF.p, dI.p, dYSum.p, dBits.p, L.max_n, nullptr));
    HIP_TRY(hipEventRecord(e1.e, nullptr));
    HIP_TRY(launch_scan_passes(D, dFr.p, L, dX, dC.p, dI.p, dF.p, dRate.p, precision));
    HIP_TRY(hipEventRecord(e2.e, nullptr));
    HIP_TRY(hipEventSynchronize(e2.e));
    float t1 = 0, t2 = 0;
    (void)hipEventElapsedTime(&t1, e0.e, e1.e);
    (void)hipEventElapsedTime(&t2, e1.e, e2.e);
    if (yakmo_ms) *yakmo_ms += t1;
    if (scan_ms) *scan_ms += t2;
    C->resize(L.nC);
    clusters->resize(size_t(L.points));
    HIP_TRY(hipMemcpy(C->data(), dC.p, sizeof(float) * C->size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(clusters->data(), dI.p, sizeof(int) * size_t(L.points), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fr.data(), dFr.p, sizeof(ReduceFrame) * size_t(nf), hipMemcpyDeviceToHost));
    report_reduce_batch(fr, K);
    iters->resize(size_t(nf));
    slow->resize(size_t(nf));
    for (int i = 0; i < nf; ++i) {
        (*iters)[i] = fr[i].iters;
        (*slow)[i] = fr[i].slow;
        if (restarts) *restarts += fr[i].restarts;
        if (fr[i].loop_iters < 0)
            return set_last_error("KNNScanReduce: batched pipeline made no progress (guard tripped)");
    }
    return 0;
}

}  // namespace gsc

// ============================================================================
// C ABI: the drop-in test entry points of the Reduce kernels
// ============================================================================
using namespace gsc;

extern "C" {

int gsc_yakmo_chain_test(int ppl, const float* pts, int nbk, float run, int* accepted, float* run_out, float* ck,
                         float* bmn, float* bmx) {
    if (require_device() != 0) return -1;
    if ((ppl != 8 && ppl != 16) || nbk < 1 || nbk > ppl)
        return set_last_error("gsc_yakmo_chain_test: ppl 8 / 16, 1 <= nbk <= ppl");
    DevBuf<float> dP, dO;
    DevBuf<int> dK;
    HIP_TRY(dP.alloc(size_t(64) * nbk));
    HIP_TRY(dO.alloc(1 + 3 * 64));
    HIP_TRY(dK.alloc(1));
    HIP_TRY(hipMemcpy(dP.p, pts, sizeof(float) * 64 * size_t(nbk), hipMemcpyHostToDevice));
    HIP_TRY(gsc_launch_yakmo_chain_test(ppl, dP.p, nbk, run, dK.p, dO.p));
    HIP_TRY(hipDeviceSynchronize());
    float o[1 + 3 * 64];
    HIP_TRY(hipMemcpy(o, dO.p, sizeof(o), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(accepted, dK.p, sizeof(int), hipMemcpyDeviceToHost));
    *run_out = o[0];
    for (int b = 0; b < nbk; ++b) {
        ck[b] = o[1 + b];
        bmn[b] = o[1 + 64 + b];
        bmx[b] = o[1 + 128 + b];
    }
    return 0;
}

// yakmo's seeding alone (no KNNScanReduce pass) of several frames in ONE launch,
// with an N and a K per frame: x / centroids / labels are the frames' arrays
// one after another (ns[i] x d0, ks[i] x d0, ns[i]); labels (may be null) is the
// seeding assignment.  A frame over gsc_yakmo_max_lds_points() puts every frame
// of the launch on the kernel's HBM instantiation.
int gsc_yakmo_seed_means_frames(int nf, int d0, const int* ns, const float* x, const int* ks, float* centroids,
                                int* labels) {
    if (require_device() != 0) return -1;
    if (nf <= 0 || !ns || !ks || !x || !centroids) return set_last_error("gsc_yakmo_seed_means_frames: invalid argument");
    for (int i = 0; i < nf; ++i)
        if (ks[i] >= ns[i] || ks[i] <= 0 || ks[i] > kMaxK) return set_last_error("yakmo needs 0 < k < n, k <= 4096");
    if (d0 <= 0 || d0 > 32) return set_last_error("yakmo: 1 <= d <= 32 features");
    const int d = feature_stride((d0 + 1) / 2);  // the kernel width; trailing zero features change nothing
    const ReduceLayout L = reduce_layout(nf, ns, ks, nullptr, d, 0);
    const int nsum = int(L.points), ksum = int(L.nC / size_t(d));
    const std::vector<float> X = pad_rows(x, nsum, d0, d);
    std::vector<float> C(L.nC);
    DevBuf<float> dX, dC, dF, dYSum;
    DevBuf<int> dI;
    DevBuf<uint32_t> dBits;
    DevBuf<ReduceFrame> dFr;
    HIP_TRY(dX.alloc(X.size()));
    HIP_TRY(dC.alloc(L.nC));
    // (the pick's replay loads whole 64-point rows of d0: a last frame of fewer
    // than 22 points would read past its 4 N floats)
    HIP_TRY(dF.alloc(L.nF + 64));
    HIP_TRY(dI.alloc(L.nI));
    HIP_TRY(dBits.alloc(gsc_yakmo_big_words(L.points, nf)));
    HIP_TRY(dYSum.alloc(gsc_yakmo_big_floats(L.points, nf)));
    HIP_TRY(dFr.alloc(size_t(nf)));
    HIP_TRY(hipMemcpy(dX.p, X.data(), sizeof(float) * X.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dFr.p, L.frames.data(), sizeof(ReduceFrame) * size_t(nf), hipMemcpyHostToDevice));
    HIP_TRY(gsc_launch_yakmo(d, dFr.p, nf, dX.p, dC.p, dF.p, dI.p, dYSum.p, dBits.p, L.max_n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(C.data(), dC.p, sizeof(float) * C.size(), hipMemcpyDeviceToHost));
    compact_rows(&C, ksum, d, d0);
    std::memcpy(centroids, C.data(), sizeof(float) * size_t(ksum) * d0);
    if (labels) HIP_TRY(hipMemcpy(labels, dI.p, sizeof(int) * size_t(nsum), hipMemcpyDeviceToHost));
    return 0;
}

// the seeds of one frame
int gsc_yakmo_seed_means(int n, int d0, const float* x, int k, float* centroids) {
    return gsc_yakmo_seed_means_frames(1, d0, &n, x, &k, centroids, nullptr);
}

int gsc_scan_reduce(int n, int d0, const float* x, int k, float* centroids, int* clusters, int precision, int* iters) {
    if (require_device() != 0) return -1;
    return scan_reduce_host(1, d0, &n, x, &k, centroids, clusters, precision, iters, nullptr, nullptr, nullptr, true);
}

// Internal (tests and tools; not part of include/soundchunks.h): scan_reduce_host
// with a K per frame.  Out per frame: passes, the frame's kind (1 = plain), the
// passes its PLAIN kernel ran, the last pass's residual.
int gsc_scan_reduce_frames(int nf, int d0, const int* ns, const float* x, const int* ks, float* centroids,
                           int* clusters, int precision, int* iters, int* plain, int* plain_passes, double* err) {
    if (require_device() != 0) return -1;
    if (nf <= 0 || !ns || !ks || !x || !centroids || !clusters)
        return set_last_error("gsc_scan_reduce_frames: invalid argument");
    if (d0 <= 0 || d0 > 32) return set_last_error("KNNScanReduce kernels support 1 <= d <= 32 features");
    for (int i = 0; i < nf; ++i)
        if (ns[i] <= 0 || ks[i] < 2 || ks[i] > kMaxK)
            return set_last_error("gsc_scan_reduce_frames: invalid frame shape");
    return scan_reduce_host(nf, d0, ns, x, ks, centroids, clusters, precision, iters, plain, plain_passes, err, false);
}

}  // extern "C"
