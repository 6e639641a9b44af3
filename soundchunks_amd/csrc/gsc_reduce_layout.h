// Where every frame of a Reduce / KNNScanReduce batch lives in the batch's
// slabs, and how large those slabs are: the one place that knows.  Host code
// with no HIP call in it (tools/encode/reduce_layout_check.cpp runs it under
// the host sanitizers).
//
//   dI (ints)  : [ clusters, N per frame | counts by centroid id, K per frame |
//                  counts by kd-leaf position, Kp per frame ]
//   dF (floats): 4 per point
//   dC (floats): K x D centroids per frame, one after another
//   tails      : the split layout's slot per frame (tail_offset)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gsc_device.h"

namespace gsc {
#pragma GCC visibility push(hidden)

// leaves of the batched kernel's layout: K rounded up to a power of two, at
// least 256 (a K below it runs the padded layout, gsc_tree.h pad_tree)
inline int padded_k(int K) {
    int k = 256;
    while (k < K) k <<= 1;
    return k;
}

// split-layout tail array offset of frame i (frames' slots of the largest size)
inline int64_t tail_offset(int i) { return int64_t(i) * 4096 * 16; }

struct ReduceLayout {
    std::vector<ReduceFrame> frames;        // offsets, N, K and dcol set; everything else zero
    size_t nI = 0, nF = 0, nC = 0, nT = 0;  // elements of the dI, dF, dC and tails slabs
    int64_t points = 0;                     // sum of N
    int max_n = 0, max_k = 0;
};

// N[i] points and K[i] centroids per frame; frame i's N[i] x D features at
// x_off[i] of the caller's slab (null: packed, one frame after another); dcol:
// the real colCount (<= D, 0 = D).  The per-position scratch covers the padded
// layout of the largest K.
inline ReduceLayout reduce_layout(int nf, const int* N, const int* K, const int64_t* x_off, int D, int dcol) {
    ReduceLayout L;
    L.frames.assign(size_t(nf), ReduceFrame{});
    int64_t ksum = 0;
    for (int i = 0; i < nf; ++i) {
        L.points += N[i];
        ksum += K[i];
        L.max_n = std::max(L.max_n, N[i]);
        L.max_k = std::max(L.max_k, K[i]);
    }
    const int Kp = padded_k(L.max_k);
    int64_t no = 0, ko = 0;
    for (int i = 0; i < nf; ++i) {
        ReduceFrame& f = L.frames[size_t(i)];
        f.x_off = x_off ? x_off[i] : no * D;
        f.c_off = ko * D;
        f.n_off = no;
        f.k_off = L.points + ko;
        f.ka_off = L.points + ksum + int64_t(i) * Kp;
        f.t_off = tail_offset(i);
        f.N = N[i];
        f.K = K[i];
        f.dcol = dcol;
        no += N[i];
        ko += K[i];
    }
    L.nI = size_t(L.points) + size_t(ksum) + size_t(nf) * size_t(Kp);
    L.nF = size_t(L.points) * 4;
    L.nC = size_t(ksum) * size_t(D);
    L.nT = size_t(tail_offset(nf));
    return L;
}

#pragma GCC visibility pop
}  // namespace gsc
