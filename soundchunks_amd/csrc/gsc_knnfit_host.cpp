// Host side of TFrame.KNNFit outside the encode pipeline: the overflow replay
// through ANN's priority search (run_knnfit_overflow, also called by the
// pipeline's post_group), the synchronous batch driver and its entry points
// gsc_knnfit_assign_frames (several frames, one launch) and gsc_knnfit_assign.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/soundchunks.h"
#include "gsc_encode_host.h"
#include "gsc_launch.h"

namespace gsc {

int run_knnfit_overflow(int CS, const std::vector<FitFrame>& fr, const std::vector<int>& ov_frames,
                        const std::vector<float>& eps, const std::vector<float>& cand, const std::vector<float>& q,
                        std::vector<int>* best, hipStream_t st, DevArena* arena) {
    const int nt = int(ov_frames.size());
    const double t_begin = now_ms();
    std::vector<float> pts;
    std::vector<int64_t> pt_off(static_cast<size_t>(nt)), nd_off(static_cast<size_t>(nt));
    std::vector<int> caps(static_cast<size_t>(nt));
    int64_t nodes = 0;
    int max_n = 0;
    for (int t = 0; t < nt; ++t) {
        const FitFrame& f = fr[size_t(ov_frames[t])];
        const int n = 4 * f.R;
        pt_off[t] = int64_t(pts.size());
        pts.resize(pts.size() + size_t(n) * CS);
        float* o = pts.data() + pt_off[t];
        const float* c = cand.data() + f.cand_off;
        for (int r = 0; r < f.R; ++r) {
            const float* v = c + size_t(r) * CS;
            for (int j = 0; j < CS; ++j) {
                const float fw = v[j], rv = v[CS - 1 - j];
                // makeFloatSample of the negated int16: exact negation, but 0 stays +0
                o[(size_t(4 * r) + 0) * CS + j] = fw;
                o[(size_t(4 * r) + 1) * CS + j] = rv;
                o[(size_t(4 * r) + 2) * CS + j] = fw == 0.0f ? 0.0f : -fw;
                o[(size_t(4 * r) + 3) * CS + j] = rv == 0.0f ? 0.0f : -rv;
            }
        }
        int p2 = 1;
        while (p2 < n) p2 <<= 1;
        caps[t] = 2 * p2;
        nd_off[t] = nodes;
        nodes += caps[t];
        max_n = std::max(max_n, n);
    }
    // jobs: every query the brute-force kernel flagged
    std::vector<KnnOvJob> jobs;
    for (int t = 0; t < nt; ++t) {
        const FitFrame& f = fr[size_t(ov_frames[t])];
        for (int i = 0; i < f.N; ++i)
            if ((*best)[size_t(f.out_off + i)] == -1) {
                jobs.push_back(KnnOvJob{t, int(f.q_off + int64_t(i) * CS), int(f.out_off + i), eps[size_t(ov_frames[t])]});
            }
    }
    if (jobs.empty()) return 0;
    if (q.size() > size_t(INT32_MAX)) return set_last_error("KNNFit overflow: query slab exceeds 2^31 floats");
    // the box queues (<= one push per split node each): bounded launches
    const int pq_cap = max_n + 2;
    const size_t per_job = size_t(pq_cap) * (sizeof(float) + sizeof(int4));
    const int chunk = int(std::max<size_t>(64, std::min<size_t>(jobs.size(), (size_t(2) << 30) / per_job)));
    // the caller's arena (no allocation on the replay's stream, nothing freed
    // before the owner is done); every sub-buffer poison-filled below
    const size_t npts = pts.size() / size_t(CS);
    const size_t R = DevArena::round_up(sizeof(float) * pts.size()) + 2 * DevArena::round_up(sizeof(float) * npts) +
                     2 * DevArena::round_up(sizeof(int) * size_t(nodes)) + 2 * DevArena::round_up(sizeof(float) * size_t(nodes)) +
                     DevArena::round_up(sizeof(int) * npts) + DevArena::round_up(sizeof(float) * size_t(2 * CS * nt)) +
                     DevArena::round_up(sizeof(AnnTree) * size_t(nt)) + DevArena::round_up(sizeof(float) * q.size()) +
                     DevArena::round_up(sizeof(int) * best->size()) + DevArena::round_up(sizeof(KnnOvJob) * jobs.size()) +
                     DevArena::round_up(sizeof(float) * size_t(chunk) * pq_cap) +
                     DevArena::round_up(sizeof(int4) * size_t(chunk) * pq_cap);
    HIP_TRY(arena->reset(R));
    float* dPts = arena->take<float>(pts.size());
    int* dPidx = arena->take<int>(npts);
    float* dVal = arena->take<float>(npts);
    int* dCd = arena->take<int>(size_t(nodes));
    float* dCv = arena->take<float>(size_t(nodes));
    float* dLo = arena->take<float>(size_t(nodes));
    float* dHi = arena->take<float>(size_t(nodes));
    float* dBnd = arena->take<float>(size_t(2 * CS * nt));
    AnnTree* dTrees = arena->take<AnnTree>(size_t(nt));
    float* dQ = arena->take<float>(q.size());
    int* dOut = arena->take<int>(best->size());
    KnnOvJob* dJobs = arena->take<KnnOvJob>(jobs.size());
    float* dPqk = arena->take<float>(size_t(chunk) * pq_cap);
    int4* dPqn = arena->take<int4>(size_t(chunk) * pq_cap);
    if (!dPqn) return set_last_error("KNNFit overflow: replay arena too small");
    HIP_TRY(hipMemsetAsync(arena->p, 0xff, arena->used, st));  // poison (dCd's -1 marks unbuilt nodes too)
    HIP_TRY(hipMemcpyAsync(dPts, pts.data(), sizeof(float) * pts.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dQ, q.data(), sizeof(float) * q.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dOut, best->data(), sizeof(int) * best->size(), hipMemcpyHostToDevice, st));
    std::vector<AnnTree> trees(static_cast<size_t>(nt));
    for (int t = 0; t < nt; ++t) {
        AnnTree& a = trees[size_t(t)];
        a.pts = dPts + pt_off[t];
        a.n = 4 * fr[size_t(ov_frames[t])].R;
        a.dd = CS;
        a.pidx = dPidx + pt_off[t] / CS;
        a.cd = dCd + nd_off[t];
        a.cv = dCv + nd_off[t];
        a.lo = dLo + nd_off[t];
        a.hi = dHi + nd_off[t];
        a.bnd = dBnd + size_t(2 * CS) * size_t(t);
        a.val = dVal + pt_off[t] / CS;
        a.ncap = caps[t];
    }
    HIP_TRY(hipMemcpyAsync(dTrees, trees.data(), sizeof(AnnTree) * size_t(nt), hipMemcpyHostToDevice, st));
    const bool timing = std::getenv("GSC_HOST_TIMING") != nullptr;
    Event eb0, eb1;  // diagnostic
    if (timing) {
        HIP_TRY(eb0.create());
        HIP_TRY(eb1.create());
        HIP_TRY(hipEventRecord(eb0.e, st));
    }
    HIP_TRY(gsc_launch_ann_build_many(dTrees, nt, st));
    if (timing) HIP_TRY(hipEventRecord(eb1.e, st));
    HIP_TRY(hipMemcpyAsync(dJobs, jobs.data(), sizeof(KnnOvJob) * jobs.size(), hipMemcpyHostToDevice, st));
    for (size_t j0 = 0; j0 < jobs.size(); j0 += size_t(chunk)) {
        const int nj = int(std::min<size_t>(size_t(chunk), jobs.size() - j0));
        HIP_TRY(gsc_launch_knnfit_ann(dTrees, dJobs + j0, nj, dQ, dOut, dPqk, dPqn, pq_cap, st));
    }
    HIP_TRY(hipMemcpyAsync(best->data(), dOut, sizeof(int) * best->size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (timing) {
        float bms = 0.0f;
        (void)hipEventElapsedTime(&bms, eb0.e, eb1.e);
        std::fprintf(stderr, "KNNFit overflow: %d trees (largest %d candidates), %zu queries, %.2f ms (tree builds %.2f ms)\n",
                     nt, max_n, jobs.size(), now_ms() - t_begin, double(bms));
    }
    for (const KnnOvJob& j : jobs) {
        const int b = (*best)[size_t(j.out)];
        if (b == -4)
            return set_last_error("KNNFit overflow: a tree index left its frame's arrays (device bounds check)");
        if (b < 0) return set_last_error("KNNFit: ANN priority search emulation failed");
    }
    return 0;
}

namespace {

// KNNFit of whole frames from host arrays, synchronously; knn_ms: the kernel's and the replay's time;
// overflow (may be null): per frame, the queries the brute-force kernel flagged for the replay
int run_knnfit_batch(int CS, const std::vector<int>& Rs, const std::vector<int>& Ns, const std::vector<float>& eps,
                     const std::vector<float>& cand, const std::vector<float>& q, std::vector<int>* best,
                     double* knn_ms, std::vector<int>* overflow) {
    const int nf = int(Ns.size());
    if (nf == 0) return 0;
    std::vector<FitFrame> fr(static_cast<size_t>(nf));
    int64_t co = 0, qo = 0;
    int maxN = 0, maxR = 0;
    for (int i = 0; i < nf; ++i) {
        fr[i] = FitFrame{};
        fr[i].cand_off = co;
        fr[i].q_off = qo;
        fr[i].out_off = qo / CS;
        fr[i].R = Rs[i];
        fr[i].N = Ns[i];
        fr[i].eps = eps[i];
        co += int64_t(Rs[i]) * CS;
        qo += int64_t(Ns[i]) * CS;
        maxN = std::max(maxN, Ns[i]);
        maxR = std::max(maxR, Rs[i]);
    }
    DevBuf<float> dCand, dQ;
    DevBuf<int> dOut;
    DevBuf<FitFrame> dFr;
    HIP_TRY(dCand.alloc(size_t(co)));
    HIP_TRY(dQ.alloc(size_t(qo)));
    HIP_TRY(hipMemcpy(dQ.p, q.data(), sizeof(float) * size_t(qo), hipMemcpyHostToDevice));
    HIP_TRY(dOut.alloc(size_t(qo / CS)));
    HIP_TRY(dFr.alloc(size_t(nf)));
    HIP_TRY(hipMemcpy(dCand.p, cand.data(), sizeof(float) * size_t(co), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dFr.p, fr.data(), sizeof(FitFrame) * size_t(nf), hipMemcpyHostToDevice));
    Event e0, e1;
    HIP_TRY(e0.create());
    HIP_TRY(e1.create());
    HIP_TRY(hipEventRecord(e0.e, nullptr));
    HIP_TRY(gsc_launch_knnfit(CS, dFr.p, nf, maxN, maxR, dCand.p, dQ.p, dOut.p, nullptr));
    HIP_TRY(hipEventRecord(e1.e, nullptr));
    HIP_TRY(hipEventSynchronize(e1.e));
    float t = 0;
    (void)hipEventElapsedTime(&t, e0.e, e1.e);
    if (knn_ms) *knn_ms += t;
    best->resize(size_t(qo / CS));
    HIP_TRY(hipMemcpy(best->data(), dOut.p, sizeof(int) * best->size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fr.data(), dFr.p, sizeof(FitFrame) * size_t(nf), hipMemcpyDeviceToHost));
    std::vector<int> ov_frames;
    if (overflow) overflow->assign(size_t(nf), 0);
    for (int i = 0; i < nf; ++i) {
        if (fr[i].overflow > 0) ov_frames.push_back(i);
        if (overflow) (*overflow)[size_t(i)] = fr[i].overflow;
    }
    if (!ov_frames.empty()) {
        const double t0 = now_ms();
        DevArena arena;  // synchronous call: freed on return, after the stream sync
        if (run_knnfit_overflow(CS, fr, ov_frames, eps, cand, q, best, nullptr, &arena) != 0) return -1;
        if (knn_ms) *knn_ms += now_ms() - t0;
    }
    return 0;
}

}  // namespace
}  // namespace gsc

// KNNFit of nf frames in ONE launch, an r, an n and an eps per frame: cand_fwd,
// q and best hold the frames' arrays one after another (rs[i] x cs, ns[i] x cs,
// ns[i]); overflow[i] (may be null) counts frame i's queries whose tie set
// exceeded the 64-NN bucket, which the ANN replay answered.
extern "C" int gsc_knnfit_assign_frames(int nf, int cs, const int* rs, const float* cand_fwd, const int* ns,
                                        const float* q, const float* eps, int* best, int* overflow) {
    using gsc::set_last_error;
    if (gsc::require_device() != 0) return -1;
    if (nf <= 0) return set_last_error("gsc_knnfit_assign_frames: nf must be positive");
    if (cs < 1 || cs > 16) return set_last_error("gsc_knnfit_assign_frames: cs outside 1..16");
    if (!rs) return set_last_error("gsc_knnfit_assign_frames: rs is null");
    if (!cand_fwd) return set_last_error("gsc_knnfit_assign_frames: cand_fwd is null");
    if (!ns) return set_last_error("gsc_knnfit_assign_frames: ns is null");
    if (!q) return set_last_error("gsc_knnfit_assign_frames: q is null");
    if (!eps) return set_last_error("gsc_knnfit_assign_frames: eps is null");
    if (!best) return set_last_error("gsc_knnfit_assign_frames: best is null");
    size_t rsum = 0, nsum = 0;
    for (int i = 0; i < nf; ++i) {
        if (rs[i] < 1) return set_last_error("gsc_knnfit_assign_frames: every r must be at least 1");
        if (ns[i] < 1) return set_last_error("gsc_knnfit_assign_frames: every n must be at least 1");
        rsum += size_t(rs[i]);
        nsum += size_t(ns[i]);
    }
    std::vector<int> Rs(rs, rs + nf), Ns(ns, ns + nf), out, ov;
    std::vector<float> E(eps, eps + nf), C(cand_fwd, cand_fwd + rsum * size_t(cs)), Q(q, q + nsum * size_t(cs));
    double ms = 0;
    if (gsc::run_knnfit_batch(cs, Rs, Ns, E, C, Q, &out, &ms, &ov) != 0) return -1;
    std::memcpy(best, out.data(), sizeof(int) * nsum);
    if (overflow) std::memcpy(overflow, ov.data(), sizeof(int) * size_t(nf));
    return 0;
}

// one frame
extern "C" int gsc_knnfit_assign(int r, int cs, const float* cand_fwd, int n, const float* q, float eps, int* best) {
    return gsc_knnfit_assign_frames(1, cs, &r, cand_fwd, &n, q, &eps, best, nullptr);
}
