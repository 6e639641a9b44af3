// The encode of a frame range on the device (Encoder::encode_range): device
// DSP, the batched Reduce with the KNNFit / prune / packing pipeline running
// beside it on frame groups as the scan finishes them (PostLoop, post_group),
// reconstruction, and the range's timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/soundchunks.h"
#include "gsc_decode.h"
#include "gsc_encode_host.h"
#include "gsc_encoder.h"
#include "gsc_launch.h"

namespace gsc {
namespace {

// Pinned host staging, kept across encode calls (pinning ~100 MB per call
// would cost more than the transfers).  Leaked on purpose: it lives until the
// process exits, after the HIP runtime may already be gone.
struct PinnedBuf {
    unsigned flags = hipHostMallocDefault;
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
        const hipError_t e = hipHostMalloc(&p, want, flags);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

struct PinnedArena {
    std::mutex m;
    // host-side DMA staging: candidates up, use counts down, remap up, words down, codes down
    PinnedBuf cand, cnt, remap, words, codes;
    // written by the scan kernel (fine-grained, mapped): final clusters and done flags
    PinnedBuf cl{hipHostMallocMapped | hipHostMallocCoherent}, notify{hipHostMallocMapped | hipHostMallocCoherent};
};

PinnedArena& pinned_arena() {
    static PinnedArena* a = new PinnedArena;
    return *a;
}

// The one way an Encoder:: method reports a HIP failure: "<stage>: <what>: <HIP's text>" into *err
struct StageErr {
    const char* stage;
    std::string* err;
    bool operator()(hipError_t r, const char* what) const {
        if (r == hipSuccess) return true;
        *err = std::string(stage) + ": " + what + ": " + hipGetErrorString(r);
        return false;
    }
};

// test hook (tests/test_gpu_parity.py): GSC_TEST_FAIL_POST set makes ONE
// post_group call of the process fail, while the scan may still be running
bool inject_post_failure() {
    static std::atomic<int> used{0};
    return std::getenv("GSC_TEST_FAIL_POST") != nullptr && used.exchange(1) == 0;
}

}  // namespace

// KNNFit + prune/sort + index packing of one encode, run on frame groups as
// they become ready (frames that skip the Reduce at once, reduced frames when
// the scan kernel signals them), on its own non-blocking stream so that the
// groups run on the CUs that finished frames leave idle.
struct PostCtx {
    hipStream_t st = nullptr;
    bool recon = false;
    std::vector<int64_t> coff, roff, woff, noff;  // per frame: candidates (floats), R slots, words, chunks
    DevBuf<float> dCand;
    DevBuf<int> dBest, dCnt, dRemap;
    DevBuf<uint32_t> dWords, dCodes;
    DevBuf<FitFrame> dFit;
    DevBuf<PackFrame> dPack;
    // with a seek table: the packer's checkpoints, frame i's ceil(n / kDecodeS) at cpoff[i]
    bool table = false;
    std::vector<int64_t> cpoff;
    DevBuf<uint64_t> dCps;
    std::vector<uint64_t> hCps;
    DevArena ov_arena;  // KNNFit overflow replay scratch (kept until the encode is done)
    const float* dQry = nullptr;
    float* hCand = nullptr;
    int *hCnt = nullptr, *hRemap = nullptr;
    uint32_t *hWords = nullptr, *hCodes = nullptr;
    int slot = 0;  // next descriptor slot in dFit / dPack
    double knn_ms = 0;
    int groups = 0;
    long long ov_queries = 0;  // KNNFit queries replayed through ANN's priority search
    ~PostCtx() {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
};

#pragma GCC visibility push(hidden)

// The post worker of one encode: post_group over the frames that are ready,
// until every frame is done or the Reduce has failed.  With a batched scan it
// runs on a thread of its own beside run_reduce_batch_dev.
struct PostLoop {
    Encoder& enc;
    std::vector<FrameState>& frames;
    const std::vector<char>& is_red;
    PostCtx& pc;
    bool batched_scan = false;
    // host-mapped, written by the scan kernel: reduced frame j's done flag, and
    // its final clusters at cl_host + red_noff[j]
    const int* notify = nullptr;
    const int* cl_host = nullptr;
    std::vector<int64_t> red_noff;
    std::vector<int> red_pos;  // frame -> its place among the reduced frames, or -1
    // 0: scanning; 1: every frame's clusters are final (notified ones in
    // cl_host, the others in cl_final); -1: the Reduce failed
    std::atomic<int> scan_state{0};
    std::vector<int> cl_final;
    std::string err;
    double overlap_ms = 0;  // post_group time spent while the scan still ran

    int run() {
        const int nfr = int(frames.size());
        std::vector<char> done(size_t(nfr), 0);
        int remaining = nfr;
        while (remaining > 0) {
            const int st = scan_state.load(std::memory_order_acquire);
            if (st < 0) return 0;
            std::vector<int> ids;
            for (int i = 0; i < nfr; ++i) {
                if (done[size_t(i)]) continue;
                const int j = red_pos[size_t(i)];
                const bool notified = j >= 0 && batched_scan && __atomic_load_n(&notify[j], __ATOMIC_ACQUIRE) != 0;
                if (j < 0 || notified || st == 1) ids.push_back(i);
            }
            // during the scan, wait for a group worth a launch
            if (ids.empty() || (st == 0 && int(ids.size()) < std::min(remaining, 8))) {
                std::this_thread::sleep_for(std::chrono::microseconds(500));
                continue;
            }
            for (int i : ids) {
                const int j = red_pos[size_t(i)];
                if (j < 0 || !batched_scan) continue;
                FrameState& f = frames[size_t(i)];
                if (__atomic_load_n(&notify[j], __ATOMIC_ACQUIRE) != 0)
                    f.clusters.assign(cl_host + red_noff[size_t(j)], cl_host + red_noff[size_t(j) + 1]);
                else
                    f.clusters.assign(cl_final.begin() + long(red_noff[size_t(j)]),
                                      cl_final.begin() + long(red_noff[size_t(j) + 1]));
            }
            const double tg = now_ms();
            if (enc.post_group(frames, ids, is_red, pc, &err) != 0) return -1;
            if (st == 0) overlap_ms += now_ms() - tg;
            for (int i : ids) done[size_t(i)] = 1;
            remaining -= int(ids.size());
        }
        return 0;
    }
};

namespace {

// what encode_range measures and counts on its way, for gsc_timing and GSC_HOST_TIMING
struct RangeStats {
    double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;  // start, DSP done, scan done, post done, output done
    double dsp_ms = 0, yak_ms = 0, scan_ms = 0, recon_ms = 0;
    long long passes = 0, slow = 0, restarts = 0;
};

// element counts of the post slabs of a range
struct PostTotals {
    int64_t cand = 0, red = 0, words = 0, chunks = 0, cps = 0;
};

// The KNNFit / prune / packing pipeline's slabs for the whole range: every
// frame's offsets into them (pc), the device slabs, pc's stream and the pinned
// staging of `pa`, all before the scan starts -- nothing is allocated or freed
// while it runs.  nred frames with nred_pts points in all go through the Reduce.
int plan_post_slabs(const std::vector<FrameState>& frames, const std::vector<char>& is_red, int K, int cs, int nred,
                    int64_t nred_pts, PinnedArena& pa, PostCtx& pc, PostTotals* tot, std::string* err) {
    const int nfr = int(frames.size());
    for (auto* v : {&pc.coff, &pc.roff, &pc.woff, &pc.noff, &pc.cpoff}) v->resize(size_t(nfr));
    PostTotals& t = *tot;
    for (int i = 0; i < nfr; ++i) {
        const int rmax = is_red[size_t(i)] ? K : frames[i].n;  // reducedChunks.Count before pruning
        pc.coff[size_t(i)] = t.cand;
        pc.roff[size_t(i)] = t.red;
        pc.woff[size_t(i)] = t.words;
        pc.noff[size_t(i)] = t.chunks;
        pc.cpoff[size_t(i)] = t.cps;
        t.cand += int64_t(rmax) * cs;
        t.red += rmax;
        t.words += pack_word_capacity(frames[i].n);
        t.chunks += frames[i].n;
        t.cps += (int64_t(frames[i].n) + kDecodeS - 1) / kDecodeS;
    }
    if (pc.table && t.cps >= (int64_t(1) << 31)) {
        *err = "seek table: too many checkpoints for one call";
        return -1;
    }
    if (pc.table) pc.hCps.resize(size_t(t.cps));
    const StageErr chk{"KNNFit/pack pipeline setup", err};
    const size_t nc = size_t(t.cand), nr = size_t(t.red), nw = size_t(t.words), nn = size_t(t.chunks);
    if (!chk(hipStreamCreateWithFlags(&pc.st, hipStreamNonBlocking), "stream") || !chk(pc.dCand.alloc(nc), "alloc") ||
        !chk(pc.dBest.alloc(nn), "alloc") || !chk(pc.dCnt.alloc(nr), "alloc") || !chk(pc.dRemap.alloc(nr), "alloc") ||
        !chk(pc.dWords.alloc(nw), "alloc") || !chk(pc.dFit.alloc(size_t(std::max(nfr, 1))), "alloc") ||
        !chk(pc.dPack.alloc(size_t(std::max(nfr, 1))), "alloc") || (pc.recon && !chk(pc.dCodes.alloc(nn), "alloc")) ||
        (pc.table && !chk(pc.dCps.alloc(size_t(std::max<int64_t>(t.cps, 1))), "alloc")) ||
        !chk(pa.cand.reserve(sizeof(float) * nc), "pinned alloc") ||
        !chk(pa.cnt.reserve(sizeof(int) * nr), "pinned alloc") ||
        !chk(pa.remap.reserve(sizeof(int) * nr), "pinned alloc") ||
        !chk(pa.words.reserve(sizeof(uint32_t) * nw), "pinned alloc") ||
        (pc.recon && !chk(pa.codes.reserve(sizeof(uint32_t) * nn), "pinned alloc")) ||
        !chk(pa.cl.reserve(sizeof(int) * size_t(std::max<int64_t>(nred_pts, 1))), "pinned alloc") ||
        !chk(pa.notify.reserve(sizeof(int) * size_t(std::max(nred, 1))), "pinned alloc") ||
        !chk(hipMemsetAsync(pc.dWords.p, 0, sizeof(uint32_t) * nw, pc.st), "memset"))
        return -1;
    pc.hCand = pa.cand.as<float>();
    pc.hCnt = pa.cnt.as<int>();
    pc.hRemap = pa.remap.as<int>();
    pc.hWords = pa.words.as<uint32_t>();
    pc.hCodes = pa.codes.as<uint32_t>();
    return 0;
}

// -py: TFrame.Reduce with PythonReduce (encoder.lpr:837-841): Birch labels
// (gsc_birch_host.cpp) of the features at dFeat + xoff[j], no yakmo and no KNNScanReduce
int reduce_python(std::vector<FrameState>& frames, const std::vector<int>& red_idx, const std::vector<int64_t>& xoff,
                  const float* dFeat, int K, int D, int DP, std::string* err) {
    for (size_t j = 0; j < red_idx.size(); ++j) {
        FrameState& f = frames[red_idx[j]];
        std::vector<float> x(size_t(f.n) * DP);
        if (hipMemcpy(x.data(), dFeat + xoff[j], sizeof(float) * x.size(), hipMemcpyDeviceToHost) != hipSuccess) {
            *err = "-py: feature download failed";
            return -1;
        }
        compact_rows(&x, f.n, DP, D);  // cluster.py reads the real features (extern.pas:363-369)
        f.clusters.resize(size_t(f.n));
        if (birch_reduce_labels(f.n, D, x.data(), K, f.clusters.data(), err) != 0) return -1;
        f.scan_iters = 0;
        f.scan_slow = 0;
    }
    return 0;
}

// The batched Reduce of the frames red_idx on the calling thread, the post
// worker beside it on a thread of its own; returns when both are done.  The
// Reduce's failure is in *err, the worker's in post.err (rc in *post_rc).
int reduce_with_post_worker(PostLoop& post, const std::vector<int>& red_idx, const std::vector<int>& Ns,
                            const std::vector<int64_t>& xoff, const float* dFeat, int DP, int D, int K, int precision,
                            int* cl_host, int* notify, RangeStats* rs, int* post_rc, std::string* err) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::thread worker([&] {
        if (hipSetDevice(dev) != hipSuccess) {
            post.err = "KNNFit/pack pipeline: hipSetDevice failed";
            *post_rc = -1;
            return;
        }
        *post_rc = post.run();
    });
    std::vector<float> C;
    std::vector<int> it, sl;
    g_scan_rounds.store(0);
    int* cl_dev = nullptr;
    int* nt_dev = nullptr;
    int rr = 0;
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&cl_dev), cl_host, 0) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&nt_dev), notify, 0) != hipSuccess) {
        rr = set_last_error("KNNScanReduce: no device address for the host-mapped cluster buffers");
    } else {
        rr = run_reduce_batch_dev(DP, K, precision, Ns, xoff, dFeat, &C, &post.cl_final, &it, &sl, &rs->restarts,
                                  &rs->yak_ms, &rs->scan_ms, cl_dev, nt_dev, D);
    }
    rs->t2 = now_ms();
    if (rr != 0) *err = last_error();
    post.scan_state.store(rr != 0 ? -1 : 1, std::memory_order_release);
    worker.join();
    if (rr != 0) return -1;
    for (size_t j = 0; j < red_idx.size(); ++j) {
        FrameState& f = post.frames[size_t(red_idx[j])];
        f.scan_iters = it[j];
        f.scan_slow = sl[j];
        rs->passes += it[j];
        rs->slow += sl[j];
    }
    return 0;
}

// GSC_HOST_TIMING's lines and the range's gsc_timing
void report_range(const RangeStats& s, const PostCtx& pc, double overlap_ms, const std::vector<FrameState>& frames,
                  const std::vector<int>& red_idx, gsc_timing* tim) {
    if (std::getenv("GSC_HOST_TIMING"))
        std::fprintf(stderr,
                     "host timing [ms]: frames+dsp %.1f (dsp %.1f) | reduce (yakmo %.1f scan %.1f) %.1f |"
                     " post after the scan %.1f (in the scan tail %.1f, KNNFit kernels %.1f, %d groups) | concat %.1f"
                     " | hipMalloc/hipFree so far %.1f\n",
                     s.t1 - s.t0, s.dsp_ms, s.yak_ms, s.scan_ms, s.t2 - s.t1, s.t3 - s.t2, overlap_ms, pc.knn_ms, pc.groups,
                     s.t4 - s.t3, double(g_devbuf_ns.exchange(0)) / 1e6);
    if (std::getenv("GSC_HOST_TIMING") && !red_idx.empty()) {  // per-frame pass counts (scan tail)
        std::vector<int> h(kMaxScanIters + 1, 0);
        for (int i : red_idx) h[std::min(kMaxScanIters, std::max(0, frames[i].scan_iters))]++;
        std::fprintf(stderr, "scan passes histogram:");
        for (int v = 0; v <= kMaxScanIters; ++v)
            if (h[v]) std::fprintf(stderr, " %d:%d", v, h[v]);
        std::fprintf(stderr, "\n");
    }
    if (!tim) return;
    tim->host_frames_ms = s.t1 - s.t0 - s.dsp_ms;
    tim->gpu_dsp_ms = s.dsp_ms;
    tim->gpu_yakmo_ms = s.yak_ms;
    tim->gpu_scan_ms = s.scan_ms;
    tim->gpu_knnfit_ms = pc.knn_ms;
    tim->host_post_ms = s.t4 - s.t2 - s.recon_ms;  // what the post-processing adds after the scan
    tim->gpu_recon_ms = s.recon_ms;
    tim->post_overlap_ms = overlap_ms;
    tim->post_groups = pc.groups;
    tim->knnfit_overflow = pc.ov_queries;
    tim->frames = int(frames.size());
    tim->reduce_frames = int(red_idx.size());
    long long pts = 0, pp = 0, cand = 0;
    for (auto& f : frames) {
        pts += f.n;
        pp += (long long)f.scan_iters * f.n;
        cand += (long long)f.n * 4 * f.r_before_prune;
    }
    tim->points = pts;
    tim->scan_passes = s.passes;
    tim->scan_slow = s.slow;
    tim->scan_restarts = s.restarts;
    tim->scan_point_passes = pp;
    tim->scan_launches = g_scan_rounds.exchange(0);
    tim->knnfit_launches = pc.groups;
    tim->knnfit_pairs = cand;
}

// use counts of the group's frames, from the device slab to the pinned staging
bool download_use_counts(const std::vector<FrameState>& frames, const std::vector<int>& ids, PostCtx& c,
                         const StageErr& chk) {
    for (int id : ids) {
        const size_t i = size_t(id);
        if (!chk(hipMemcpyAsync(c.hCnt + c.roff[i], c.dCnt.p + c.roff[i], sizeof(int) * size_t(frames[i].r),
                                hipMemcpyDeviceToHost, c.st),
                 "use count download"))
            return false;
    }
    return true;
}

// Queries whose tie set exceeds ANN's 64-NN bucket, in the group's frames ovk
// (indices into ids / fit): their candidates, queries and flagged answers
// gathered as a batch of their own, ANN's priority search over each frame's
// candidate tree (run_knnfit_overflow), the answers scattered back into dBest.
int replay_overflow(int cs, const std::vector<FrameState>& frames, const std::vector<int>& ids,
                    const std::vector<FitFrame>& fit, const std::vector<int>& ovk, PostCtx& c, const StageErr& chk) {
    const hipStream_t st = c.st;
    std::vector<FitFrame> lf;
    std::vector<float> lcand, lq, leps;
    std::vector<int> lbest, lidx;
    for (int k : ovk) {
        const FrameState& f = frames[size_t(ids[k])];
        FitFrame x = fit[size_t(k)];
        x.cand_off = int64_t(lcand.size());
        x.q_off = int64_t(lq.size());
        x.out_off = int64_t(lbest.size());
        lcand.insert(lcand.end(), c.hCand + fit[size_t(k)].cand_off, c.hCand + fit[size_t(k)].cand_off + size_t(f.r) * cs);
        lq.resize(lq.size() + size_t(f.n) * cs);
        lbest.resize(lbest.size() + size_t(f.n));
        if (!chk(hipMemcpyAsync(lq.data() + x.q_off, c.dQry + fit[size_t(k)].q_off, sizeof(float) * size_t(f.n) * cs,
                                hipMemcpyDeviceToHost, st),
                 "query download") ||
            !chk(hipMemcpyAsync(lbest.data() + x.out_off, c.dBest.p + fit[size_t(k)].out_off, sizeof(int) * size_t(f.n),
                                hipMemcpyDeviceToHost, st),
                 "download"))
            return -1;
        lidx.push_back(int(lf.size()));
        leps.push_back(x.eps);
        lf.push_back(x);
    }
    if (!chk(hipStreamSynchronize(st), "download")) return -1;
    c.ov_queries += std::count(lbest.begin(), lbest.end(), -1);
    if (run_knnfit_overflow(cs, lf, lidx, leps, lcand, lq, &lbest, st, &c.ov_arena) != 0) {
        *chk.err = last_error();
        return -1;
    }
    for (size_t j = 0; j < ovk.size(); ++j)
        if (!chk(hipMemcpyAsync(c.dBest.p + fit[size_t(ovk[j])].out_off, lbest.data() + lf[j].out_off,
                                sizeof(int) * size_t(lf[j].N), hipMemcpyHostToDevice, st),
                 "upload"))
            return -1;
    return 0;
}

}  // namespace
#pragma GCC visibility pop

// ---- Encoder::device_dsp: FindAttenuationDivider + features on the device --
int Encoder::device_dsp(int b, std::vector<FrameState>& frames, DevBuf<float>* dX, std::vector<int64_t>* xoff,
                        double* ms, std::string* err, DevBuf<float>* dQ) {
    const int cs = opt_.chunk_size, ch = channels_, nfr = int(frames.size());
    const int obd = (1 << (opt_.chunk_bit_depth - 1)) - 1;
    const int e = b + nfr;
    const int64_t s_first = fr_start_[b], span = int64_t(fr_end_[e - 1]) - s_first + 1;
    std::vector<DspFrame> df(static_cast<size_t>(nfr));
    xoff->assign(size_t(nfr), 0);
    int64_t xo = 0, co = 0;
    int max_n = 0;
    for (int i = 0; i < nfr; ++i) {
        const FrameState& f = frames[i];
        df[i] = DspFrame{};
        df[i].s_off = int64_t(f.start) - s_first;
        df[i].x_off = xo;
        df[i].c_off = co;
        df[i].sc = f.sample_count;
        df[i].n = f.n;
        (*xoff)[i] = xo;
        xo += int64_t(f.n) * feature_stride(cs);
        co += f.n;
        max_n = std::max(max_n, f.n);
    }
    std::vector<double> trig;
    double s0 = 0, scale = 0;
    trig_pack(cs, &trig, &s0, &scale);
    DevBuf<double> dS, dT;
    DevBuf<DspFrame> dF;
    DevBuf<uint8_t> dNR;
    DevBuf<int16_t> dP;
    const double t0 = now_ms();
    if (dS.alloc(size_t(ch) * size_t(span)) != hipSuccess || dT.alloc(trig.size()) != hipSuccess ||
        dF.alloc(size_t(nfr)) != hipSuccess || dNR.alloc(size_t(co)) != hipSuccess || dX->alloc(size_t(xo)) != hipSuccess ||
        dP.alloc(size_t(ch) * size_t(span)) != hipSuccess ||
        (dQ && dQ->alloc(size_t(co) * size_t(cs)) != hipSuccess)) {
        *err = "device DSP: out of device memory";
        return -1;
    }
    const StageErr chk{"device DSP", err};
    // the SmallInt samples of the span (a quarter of the f64 bytes), converted on the device
    if (!chk(hipMemcpy(dP.p, pcm_.data() + size_t(s_first - pcm_off_) * ch, sizeof(int16_t) * size_t(ch) * size_t(span),
                       hipMemcpyHostToDevice),
             "sample upload") ||
        !chk(gsc_launch_pcm(dP.p, span, ch, dS.p, nullptr), "sample conversion") ||
        !chk(hipMemcpy(dT.p, trig.data(), sizeof(double) * trig.size(), hipMemcpyHostToDevice), "trig upload") ||
        !chk(hipMemcpy(dF.p, df.data(), sizeof(DspFrame) * size_t(nfr), hipMemcpyHostToDevice), "frame upload") ||
        !chk(gsc_launch_atten(cs, dF.p, nfr, dS.p, span, ch, obd, nullptr), "atten launch") ||
        !chk(gsc_launch_features(cs, dF.p, nfr, max_n, dS.p, span, ch, dT.p, s0, scale, dX->p, dNR.p,
                                 dQ ? dQ->p : nullptr, nullptr),
             "features launch"))
        return -1;
    std::vector<uint8_t> nr(static_cast<size_t>(co));
    if (!chk(hipMemcpy(df.data(), dF.p, sizeof(DspFrame) * size_t(nfr), hipMemcpyDeviceToHost), "frame download") ||
        !chk(hipMemcpy(nr.data(), dNR.p, size_t(co), hipMemcpyDeviceToHost), "flag download"))
        return -1;
    for (int i = 0; i < nfr; ++i) {
        FrameState& f = frames[i];
        f.atten_div = df[i].atten_div;
        const uint8_t* q = nr.data() + df[i].c_off;
        for (int c = 0; c < f.n; ++c) {
            f.neg[c] = q[c] & 1;
            f.rev[c] = (q[c] >> 1) & 1;
        }
    }
    if (ms) *ms += now_ms() - t0;
    return 0;
}

// ---- Encoder::device_recon: reconstruction + PsyADelta numerator (f4) -----
int Encoder::device_recon(int b, const std::vector<FrameState>& frames, ReconOut* ro, std::string* err) {
    const int cs = opt_.chunk_size, ch = channels_, nfr = int(frames.size());
    if (nfr == 0) return 0;
    const double t0 = now_ms();
    const int64_t s_first = fr_start_[b], span = int64_t(fr_end_[b + nfr - 1]) - s_first + 1;
    std::vector<ReconFrame> rf(static_cast<size_t>(nfr));
    int64_t nchunk = 0, nred = 0;
    int max_n = 0;
    for (int i = 0; i < nfr; ++i) {
        const FrameState& f = frames[i];
        rf[i] = ReconFrame{nchunk, nred, int64_t(f.start) - s_first, f.n, f.sample_count, 1.0 / double(f.atten_div)};
        nchunk += f.n;
        nred += f.r;
        max_n = std::max(max_n, f.n);
    }
    std::vector<uint32_t> words(static_cast<size_t>(nchunk));
    std::vector<int16_t> rdst(static_cast<size_t>(std::max<int64_t>(nred, 1) * cs));
    std::vector<uint8_t> ratten(static_cast<size_t>(std::max<int64_t>(nred, 1)));
    parallel_for(nfr, host_threads(), [&](int i) {
        const FrameState& f = frames[i];
        uint32_t* w = words.data() + rf[i].chunk_off;
        for (int c = 0; c < f.n; ++c) w[c] = uint32_t(f.red[c]) << 2 | uint32_t(f.neg[c] & 1) << 1 | uint32_t(f.rev[c] & 1);
        std::copy(f.rdst.begin(), f.rdst.begin() + long(size_t(f.r) * cs), rdst.begin() + long(rf[i].red_off * cs));
        std::copy(f.ratten.begin(), f.ratten.begin() + f.r, ratten.begin() + long(rf[i].red_off));
    });
    // srcData of the range (SmallInt, zero past the file's own samples: PrepareFrames pads, encoder.lpr:1317-1323)
    const int64_t psc = ro->wav_len >= 44 ? int64_t((ro->wav_len - 44) / (2 * size_t(ch))) : 0;
    std::vector<int16_t> src(static_cast<size_t>(span * ch), 0);
    const int64_t avail = std::max<int64_t>(0, std::min(span, psc - s_first));
    if (avail > 0) std::memcpy(src.data(), ro->wav + 44 + size_t(s_first) * ch * 2, size_t(avail) * ch * 2);
    DevBuf<ReconFrame> dF;
    DevBuf<uint32_t> dW;
    DevBuf<int16_t> dR, dOut, dSrc;
    DevBuf<uint8_t> dA;
    DevBuf<unsigned long long> dAcc;
    const StageErr chk{"reconstruction", err};
    const size_t nout = size_t(span) * ch;
    if (!chk(dF.alloc(size_t(nfr)), "alloc") || !chk(dW.alloc(words.size()), "alloc") ||
        !chk(dR.alloc(rdst.size()), "alloc") || !chk(dA.alloc(ratten.size()), "alloc") ||
        !chk(dOut.alloc(nout), "alloc") || !chk(dSrc.alloc(nout), "alloc") || !chk(dAcc.alloc(1), "alloc"))
        return -1;
    if (!chk(hipMemcpy(dF.p, rf.data(), sizeof(ReconFrame) * rf.size(), hipMemcpyHostToDevice), "upload") ||
        !chk(hipMemcpy(dW.p, words.data(), sizeof(uint32_t) * words.size(), hipMemcpyHostToDevice), "upload") ||
        !chk(hipMemcpy(dR.p, rdst.data(), sizeof(int16_t) * rdst.size(), hipMemcpyHostToDevice), "upload") ||
        !chk(hipMemcpy(dA.p, ratten.data(), ratten.size(), hipMemcpyHostToDevice), "upload") ||
        !chk(hipMemcpy(dSrc.p, src.data(), sizeof(int16_t) * nout, hipMemcpyHostToDevice), "upload") ||
        !chk(hipMemset(dOut.p, 0, sizeof(int16_t) * nout), "memset") ||  // dstData starts zeroed (encoder.lpr:497-501)
        !chk(hipMemset(dAcc.p, 0, sizeof(unsigned long long)), "memset") ||
        !chk(gsc_launch_recon(dF.p, nfr, max_n, cs, ch, opt_.chunk_bit_depth, dW.p, dR.p, dA.p, dOut.p, nullptr),
             "recon launch") ||
        !chk(gsc_launch_sqdiff(dSrc.p, dOut.p, int64_t(nout), dAcc.p, nullptr), "PsyADelta launch"))
        return -1;
    unsigned long long sq = 0;
    if (!chk(hipMemcpy(ro->pcm + size_t(s_first) * ch, dOut.p, sizeof(int16_t) * nout, hipMemcpyDeviceToHost),
             "download") ||
        !chk(hipMemcpy(&sq, dAcc.p, sizeof(sq), hipMemcpyDeviceToHost), "download"))
        return -1;
    ro->sq += sq;
    ro->ms += now_ms() - t0;
    return 0;
}

int Encoder::post_group(std::vector<FrameState>& frames, const std::vector<int>& ids,
                        const std::vector<char>& reduced, PostCtx& c, std::string* err) {
    const int cs = opt_.chunk_size, bd = opt_.chunk_bit_depth, obd = (1 << (bd - 1)) - 1;
    const int g = int(ids.size());
    if (g == 0) return 0;
    if (inject_post_failure()) {
        *err = "injected post_group failure (GSC_TEST_FAIL_POST)";
        return -1;
    }
    const StageErr chk{"KNNFit/pack pipeline", err};
    std::vector<float> eps(static_cast<size_t>(g));
    // TFrame.Reduce's tail (cluster means, sort, reduced chunks) and the
    // KNNFit candidates (encoder.lpr:843-889, 928-938), per frame on the host pool
    parallel_for(g, host_threads(), [&](int k) {
        FrameState& f = frames[size_t(ids[k])];
        frame_reduce_post(f, reduced[size_t(ids[k])] != 0);
        const double law = 1.0 / double(f.atten_div);
        // epsilon (encoder.lpr:940-943), accumulated in Single
        float acc = 1.0f;
        for (int j = 0; j <= 15; ++j) acc = float(double(acc) + double(j) * law);
        const float e1 = 1.0f / (float(1 << bd) * acc);
        const float e2 = float(1.0 / 32767.0);
        eps[size_t(k)] = e1 > e2 ? e1 : e2;
        float* cp = c.hCand + c.coff[size_t(ids[k])];
        for (int r = 0; r < f.r; ++r) {
            double coeff = 1.0;
            for (int a = 0; a <= f.ratten[r]; ++a) coeff += double(a) * law;
            for (int j = 0; j < cs; ++j) {
                double v = double(f.rdst[size_t(r) * cs + j]) / (double(obd) * coeff);
                v = std::min(1.0, std::max(-1.0, v));
                *cp++ = float(v);
            }
        }
    });
    const int gb = c.slot;
    c.slot += g;
    std::vector<FitFrame> fit(static_cast<size_t>(g));
    std::vector<PackFrame> pk(static_cast<size_t>(g));
    int maxN = 0, maxR = 0;
    for (int k = 0; k < g; ++k) {
        const size_t i = size_t(ids[k]);
        const FrameState& f = frames[i];
        fit[size_t(k)] = FitFrame{c.coff[i], c.noff[i] * cs, c.noff[i], f.r, f.n, eps[size_t(k)], 0};
        pk[size_t(k)] = PackFrame{c.noff[i], c.roff[i], c.woff[i], f.n, f.r, 0, c.table ? int32_t(c.cpoff[i]) : 0};
        maxN = std::max(maxN, f.n);
        maxR = std::max(maxR, f.r);
    }
    Event e0, e1;
    if (!chk(e0.create(), "event") || !chk(e1.create(), "event")) return -1;
    const hipStream_t st = c.st;
    bool ok = chk(hipMemcpyAsync(c.dFit.p + gb, fit.data(), sizeof(FitFrame) * size_t(g), hipMemcpyHostToDevice, st),
                  "upload") &&
              chk(hipMemcpyAsync(c.dPack.p + gb, pk.data(), sizeof(PackFrame) * size_t(g), hipMemcpyHostToDevice, st),
                  "upload");
    for (int k = 0; ok && k < g; ++k) {
        const size_t i = size_t(ids[k]);
        ok = chk(hipMemcpyAsync(c.dCand.p + c.coff[i], c.hCand + c.coff[i], sizeof(float) * size_t(frames[i].r) * cs,
                                hipMemcpyHostToDevice, st),
                 "candidate upload");
    }
    ok = ok && chk(hipEventRecord(e0.e, st), "event") &&
         chk(gsc_launch_knnfit(cs, c.dFit.p + gb, g, maxN, maxR, c.dCand.p, c.dQry, c.dBest.p, st), "KNNFit launch") &&
         chk(hipEventRecord(e1.e, st), "event") &&
         chk(gsc_launch_usecount(c.dPack.p + gb, g, c.dBest.p, c.dCnt.p, st), "use count launch") &&
         chk(hipMemcpyAsync(fit.data(), c.dFit.p + gb, sizeof(FitFrame) * size_t(g), hipMemcpyDeviceToHost, st),
             "download") &&
         download_use_counts(frames, ids, c, chk);
    if (!ok || !chk(hipStreamSynchronize(st), "KNNFit")) return -1;
    float t = 0;
    if (hipEventElapsedTime(&t, e0.e, e1.e) == hipSuccess) c.knn_ms += t;
    // queries whose tie set exceeds ANN's 64-NN bucket: ANN's priority search
    // over the frame's candidate tree (rare; it waits for the scan)
    std::vector<int> ovk;
    for (int k = 0; k < g; ++k)
        if (fit[size_t(k)].overflow > 0) ovk.push_back(k);
    if (!ovk.empty()) {
        const double t0 = now_ms();
        if (replay_overflow(cs, frames, ids, fit, ovk, c, chk) != 0) return -1;
        ok = chk(gsc_launch_usecount(c.dPack.p + gb, g, c.dBest.p, c.dCnt.p, st), "use count launch") &&
             download_use_counts(frames, ids, c, chk);
        if (!ok || !chk(hipStreamSynchronize(st), "use counts")) return -1;
        c.knn_ms += now_ms() - t0;
    }
    // prune + sort by use count on the host, then the index stream on the device
    parallel_for(g, host_threads(), [&](int k) {
        const size_t i = size_t(ids[k]);
        frame_prune(frames[i], c.hCnt + c.roff[i], c.hRemap + c.roff[i]);
    });
    // SaveStream's Assert(reducedChunks.Count <= CMaxChunksPerFrame) (encoder.lpr:986;
    // built with assertions on): only a -pr0 passthrough frame (KNNFit over
    // every chunk) can keep more than 4096 entries after pruning
    for (int k = 0; k < g; ++k) {
        const FrameState& f = frames[size_t(ids[k])];
        if (f.r > kMaxK) {
            *err = "SaveStream: Assert(reducedChunks.Count <= CMaxChunksPerFrame) failed: frame " +
                   std::to_string(f.index) + " keeps " + std::to_string(f.r) + " reduced chunks";
            return -1;
        }
    }
    ok = true;
    for (int k = 0; ok && k < g; ++k) {
        const size_t i = size_t(ids[k]);
        ok = chk(hipMemcpyAsync(c.dRemap.p + c.roff[i], c.hRemap + c.roff[i],
                                sizeof(int) * size_t(frames[i].r_before_prune), hipMemcpyHostToDevice, st),
                 "remap upload");
    }
    ok = ok && chk(gsc_launch_pack(c.dPack.p + gb, g, c.dBest.p, c.dRemap.p, c.dWords.p, c.recon ? c.dCodes.p : nullptr,
                                   c.table ? c.dCps.p : nullptr, st),
                   "pack launch") &&
         chk(hipMemcpyAsync(pk.data(), c.dPack.p + gb, sizeof(PackFrame) * size_t(g), hipMemcpyDeviceToHost, st),
             "download") &&
         chk(hipStreamSynchronize(st), "pack");
    for (int k = 0; ok && k < g; ++k) {
        const size_t i = size_t(ids[k]);
        const int64_t nw = (int64_t(pk[size_t(k)].nbits) + 31) / 32;  // whole u32 words (>= the 16-bit words used)
        if (pk[size_t(k)].nbits < 0 || nw > pack_word_capacity(frames[i].n)) {  // pack_kernel refused the overrun
            *err = "index packer overran its word slab";
            return -1;
        }
        ok = chk(hipMemcpyAsync(c.hWords + c.woff[i], c.dWords.p + c.woff[i], sizeof(uint32_t) * size_t(nw),
                                hipMemcpyDeviceToHost, st),
                 "stream download");
        if (ok && c.recon)
            ok = chk(hipMemcpyAsync(c.hCodes + c.noff[i], c.dCodes.p + c.noff[i], sizeof(uint32_t) * size_t(frames[i].n),
                                    hipMemcpyDeviceToHost, st),
                     "code download");
        const size_t ncp = c.table ? (size_t(frames[i].n) + kDecodeS - 1) / kDecodeS : 0;
        if (ok && ncp)  // the checkpoints come down with the words
            ok = chk(hipMemcpyAsync(c.hCps.data() + c.cpoff[i], c.dCps.p + c.cpoff[i], sizeof(uint64_t) * ncp,
                                    hipMemcpyDeviceToHost, st),
                     "checkpoint download");
        frames[i].nbits = pk[size_t(k)].nbits;
    }
    if (!ok || !chk(hipStreamSynchronize(st), "stream download")) return -1;
    parallel_for(g, host_threads(), [&](int k) {
        const size_t i = size_t(ids[k]);
        FrameState& f = frames[i];
        frame_save_head(f);
        const size_t nbytes = size_t((pk[size_t(k)].nbits + 15) / 16) * 2;  // 16-bit words, the last zero-padded
        const uint8_t* wb = reinterpret_cast<const uint8_t*>(c.hWords + c.woff[i]);
        f.stream.insert(f.stream.end(), wb, wb + nbytes);
        if (c.recon) {  // final index / dstNegative / dstReversed per chunk (reconstruction)
            f.red.resize(size_t(f.n));
            f.neg.resize(size_t(f.n));
            f.rev.resize(size_t(f.n));
            const uint32_t* cw = c.hCodes + c.noff[i];
            for (int j = 0; j < f.n; ++j) {
                f.red[size_t(j)] = int(cw[j] >> 2);
                f.neg[size_t(j)] = uint8_t((cw[j] >> 1) & 1);
                f.rev[size_t(j)] = uint8_t(cw[j] & 1);
            }
        }
    });
    c.groups += 1;
    return 0;
}

int Encoder::dsp_frame(int fi, int* atten_div, std::vector<float>* feat, std::string* err) {
    if (require_device() != 0) {
        *err = last_error();
        return -1;
    }
    if (fi < 0 || fi >= frame_count()) {
        *err = "frame index out of range";
        return -1;
    }
    warm_trig_tables(opt_.chunk_size);
    std::vector<FrameState> frames(1);
    frames[0].index = fi;
    frames[0].start = fr_start_[fi];
    frames[0].sample_count = fr_end_[fi] - fr_start_[fi] + 1;
    frame_host_src(frames[0]);
    DevBuf<float> dX;
    std::vector<int64_t> xoff;
    if (device_dsp(fi, frames, &dX, &xoff, nullptr, err) != 0) return -1;
    *atten_div = frames[0].atten_div;
    const int dp = feature_stride(opt_.chunk_size);
    feat->resize(size_t(frames[0].n) * dp);
    if (hipMemcpy(feat->data(), dX.p, sizeof(float) * feat->size(), hipMemcpyDeviceToHost) != hipSuccess) {
        *err = "feature download failed";
        return -1;
    }
    compact_rows(feat, frames[0].n, dp, 2 * opt_.chunk_size);
    return 0;
}

// ---- Encoder::encode_range: host srcData, device DSP + hot path ------------
int Encoder::encode_range(int b, int e, std::vector<uint8_t>* out, std::string* err, gsc_timing* tim,
                          ReconOut* recon, std::vector<size_t>* frame_bytes, std::vector<uint8_t>* table) {
    if (require_device() != 0) {
        *err = last_error();
        return -1;
    }
    const int cs = opt_.chunk_size, D = 2 * cs, K = opt_.chunks_per_frame;
    const int DP = feature_stride(cs);  // the feature slab's row width (D features, then zeros)
    const int nfr = e - b;
    RangeStats rs;
    // 1. the frames: host srcData
    std::vector<FrameState> frames(static_cast<size_t>(std::max(nfr, 0)));
    rs.t0 = now_ms();
    warm_trig_tables(cs);  // FPC trig tables, built before the workers start
    parallel_for(nfr, host_threads(), [&](int i) {
        FrameState& f = frames[i];
        f.index = b + i;
        f.start = fr_start_[b + i];
        f.sample_count = fr_end_[b + i] - fr_start_[b + i] + 1;
        frame_host_src(f);
    });
    // 2. the DSP
    DevBuf<float> dFeat, dQry;
    std::vector<int64_t> feat_off;
    if (nfr > 0 && device_dsp(b, frames, &dFeat, &feat_off, &rs.dsp_ms, err, &dQry) != 0) return -1;
    rs.t1 = now_ms();
    // 3. the frames to reduce: those with more chunks than ChunksPerFrame
    std::vector<int> red_idx, Ns;
    std::vector<int64_t> red_xoff;
    std::vector<char> is_red(size_t(nfr), 0);
    int64_t nred_pts = 0;
    for (int i = 0; i < nfr; ++i)
        if (opt_.precision > 0 && frames[i].n > K) {
            red_idx.push_back(i);
            Ns.push_back(frames[i].n);
            red_xoff.push_back(feat_off[i]);
            is_red[size_t(i)] = 1;
            nred_pts += frames[i].n;
        }
    const int nred = int(red_idx.size());
    // 4. the post slabs.  The shared pinned arena is held for the whole encode,
    // and released only after pc's stream and every device launch of this
    // encode have drained (destroyed in reverse order: post, pc, drain, then the lock)
    PinnedArena& pa = pinned_arena();
    std::lock_guard<std::mutex> arena_lock(pa.m);
    struct DeviceDrain {
        ~DeviceDrain() { (void)hipDeviceSynchronize(); }
    } drain_before_unlock;
    PostCtx pc;
    pc.recon = recon != nullptr;
    pc.table = table != nullptr;
    pc.dQry = dQry.p;
    PostTotals totals;
    if (plan_post_slabs(frames, is_red, K, cs, nred, nred_pts, pa, pc, &totals, err) != 0) return -1;
    int* notify = pa.notify.as<int>();
    int* cl_host = pa.cl.as<int>();
    std::memset(notify, 0, sizeof(int) * size_t(std::max(nred, 1)));
    PostLoop post{*this, frames, is_red, pc};
    post.batched_scan = nred > 0 && !opt_.python_reduce;
    post.notify = notify;
    post.cl_host = cl_host;
    post.red_noff.assign(size_t(nred) + 1, 0);
    post.red_pos.assign(size_t(nfr), -1);
    for (int j = 0; j < nred; ++j) {
        post.red_noff[size_t(j) + 1] = post.red_noff[size_t(j)] + Ns[size_t(j)];
        post.red_pos[size_t(red_idx[size_t(j)])] = j;
    }
    // 5. -py, or the batched Reduce with the post worker beside it
    if (nred > 0 && opt_.python_reduce) {
        const double tb = now_ms();
        if (reduce_python(frames, red_idx, red_xoff, dFeat.p, K, D, DP, err) != 0) return -1;
        rs.scan_ms += now_ms() - tb;
    }
    int post_rc = 0;
    if (post.batched_scan) {
        if (reduce_with_post_worker(post, red_idx, Ns, red_xoff, dFeat.p, DP, D, K, opt_.precision, cl_host, notify, &rs,
                                    &post_rc, err) != 0)
            return -1;
    } else {
        rs.t2 = now_ms();
        post.scan_state.store(1, std::memory_order_release);
        post_rc = post.run();
    }
    if (post_rc != 0) {
        *err = post.err;
        return -1;
    }
    rs.t3 = now_ms();
    // 6. recon
    if (recon && device_recon(b, frames, recon, err) != 0) return -1;
    rs.recon_ms = now_ms() - rs.t3;
    // 7. the bytes, and the table
    out->clear();
    size_t bytes = 0;
    for (auto& f : frames) bytes += f.stream.size();
    out->reserve(bytes);
    for (auto& f : frames) out->insert(out->end(), f.stream.begin(), f.stream.end());
    if (frame_bytes) {
        frame_bytes->clear();
        for (auto& f : frames) frame_bytes->push_back(f.stream.size());
    }
    if (table) {
        // the returned bytes as a stream of their own: offsets from their start.  Only the
        // fields index_table_write reads are filled.
        Index ix;
        ix.frames.resize(frames.size());
        size_t off = 0;
        for (size_t i = 0; i < frames.size(); ++i) {
            ix.frames[i].off = off;
            ix.frames[i].nbits = uint64_t(frames[i].nbits);
            off += frames[i].stream.size();
        }
        ix.len = off;
        ix.cps = std::move(pc.hCps);
        index_table_write(ix, table);
    }
    rs.t4 = now_ms();
    // 8. timing
    report_range(rs, pc, post.overlap_ms, frames, red_idx, tim);
    return 0;
}

}  // namespace gsc
