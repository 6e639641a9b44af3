// What the decode kernels and their launchers share (gsc_decode.hip,
// gsc_decode_crops.hip, gsc_decode_resample.hip, gsc_decode_mix.hip), each in one place: the bit
// walk of one checkpoint segment and the sample arithmetic
// (decoder/decoder.lpr:163-203), the binary search, a frame's tables staged in
// LDS or read from global memory, a crop's segments, frames and output
// elements, the walk of a crop's frames and the passes of a resampled tile with
// the caller's sink, the job of a crop that is planned on the device, and the
// dynamic-LDS limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "gsc_crop_plan.h"
#include "gsc_decode.h"

namespace gsc {

// Where a segment's walk ended: the bit offset within the frame's bitstream
// and variableCodingHeader, in make_checkpoint's form.
struct WalkEnd {
    uint64_t bit;
    int hdr;
};

// The bit walk, in one place: n symbols (n <= kDecodeS) from checkpoint cp of
// a bitstream that starts at byte bs_off of the word slab; sink(i, idx, neg,
// rev) takes symbol i with its raw index (nothing clamped).  The bytes are
// read as aligned 32-bit words; a word past nwords reads as zero.  The caller
// checked bs_off >= 0.
template <typename Sink>
__device__ __forceinline__ WalkEnd walk_segment(const uint32_t* __restrict__ words, int64_t nwords, int64_t bs_off,
                                                uint64_t cp, int ver, int n, Sink sink) {
    int hdr = (int)(cp & 7) - 1;  // variableCodingHeader on entry
    hdr = hdr > 3 ? 3 : hdr;
    const uint64_t bit = (cp >> 3) + (uint64_t)bs_off * 8;
    int64_t w = (int64_t)(bit >> 5);
    const int sh = (int)(bit & 31);
    const int rev_bit = ver > 0 ? 1 : 0;
    uint64_t buf = (w >= 0 && w < nwords ? words[w] : 0u) >> sh;
    int have = 32 - sh;
    int walked = 0;  // bits consumed: at most 17 * kDecodeS
    ++w;
    for (int i = 0; i < n; ++i) {
        if (have <= 32) {  // refill: 33 bits or more, a symbol has at most 17
            buf |= (uint64_t)(w >= 0 && w < nwords ? words[w] : 0u) << have;
            have += 32;
            ++w;
        }
        const uint32_t v = (uint32_t)buf;
        const uint32_t neg = v & 1u;
        const uint32_t rev = rev_bit ? (v >> 1) & 1u : 0u;
        int used = 1 + rev_bit;
        const int has = (int)((v >> used) & 1u);
        const int nh = (int)((v >> (used + 1)) & 3u);
        hdr = has ? nh : hdr;
        used += 1 + 2 * has;
        // the next four 3-bit blocks, first block most significant; the hdr + 1
        // leading ones are the index (no per-lane trip count: lanes stay converged)
        const uint32_t g = v >> used;
        const uint32_t r4 = (g & 7u) << 9 | ((g >> 3) & 7u) << 6 | ((g >> 6) & 7u) << 3 | ((g >> 9) & 7u);
        int idx = (int)(r4 >> (3 * (3 - hdr)));
        used += 3 * (hdr + 1);
        buf >>= used;
        have -= used;
        walked += used;
        sink(i, idx, neg, rev);
    }
    return WalkEnd{(cp >> 3) + (uint64_t)walked, hdr};
}

// The walk with one word per symbol, idx << 2 | neg << 1 | rev, written to
// o[0 .. n); an index past count - 1 is clamped.  The caller checked that o
// holds n words.
__device__ __forceinline__ void unpack_segment(const uint32_t* __restrict__ words, int64_t nwords, int64_t bs_off,
                                               uint64_t cp, int ver, int count, int n, uint16_t* o) {
    const int idx_max = count > 0 ? count - 1 : 0;
    (void)walk_segment(words, nwords, bs_off, cp, ver, n, [&](int i, int idx, uint32_t neg, uint32_t rev) {
        idx = idx > idx_max ? idx_max : idx;
        o[i] = (uint16_t)((uint32_t)idx << 2 | neg << 1 | rev);
    });
}

// The fields of a symbol word for sample j of its chunk: the chunk index
// (clamped to count - 1), the negate flag, and j mirrored when the chunk is reversed.
__device__ __forceinline__ void symbol_fields(uint32_t w, int count, int cs, int j, int* idx, int* neg, int* jj) {
    const int i = (int)(w >> 2);
    *idx = i >= count ? count - 1 : i;
    *neg = (int)((w >> 1) & 1u);
    *jj = (w & 1u) ? cs - 1 - j : j;
}

// Cardinal(attr * chunkSmp) shr 15, low word (decoder.lpr:198-201): the
// product wraps in 32 bits, it is not clamped
__device__ __forceinline__ int16_t synth_sample(int lut, int v) {
    return (int16_t)(uint16_t)(((uint32_t)(lut * v)) >> 15);
}

// The last i of [lo, hi] with key(i) <= x; lo when there is none.
template <typename Key>
__device__ __forceinline__ int last_le(int lo, int hi, int64_t x, Key key) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key(mid) <= x) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

// The codebook and attenuation slabs a frame's cb_off and att_off index.
struct TableSlabs {
    const int16_t* cb;
    int64_t ncb;
    const uint8_t* att;
    int64_t natt;
};

// A frame's tables in a workgroup's dynamic LDS (stage_tables); StagedTables{}: not staged.
struct StagedTables {
    const int16_t* cb = nullptr;
    const uint8_t* att = nullptr;
    bool on = false;
};

// Whether a frame's tables fit lds_bytes and lie inside their slabs, so that
// they can be copied to LDS word by word.
__device__ __forceinline__ bool tables_staged(const FrameTables& f, const TableSlabs& g, int lds_bytes) {
    const int64_t cbn = (int64_t)f.count * f.cs;
    return staged_size(f.count, f.cs).bytes <= lds_bytes && f.cb_off >= 0 && (f.cb_off & 1) == 0 &&
           f.cb_off + cbn + 1 <= g.ncb && f.att_off >= 0 && f.att_off + f.count <= g.natt;
}

// Every lane of a workgroup: copies the frame's tables to smem when
// tables_staged says so.  The caller puts a barrier after it, and one before
// it when smem is still being read.
__device__ __forceinline__ StagedTables stage_tables(const FrameTables& f, const TableSlabs& g, int lds_bytes,
                                                     unsigned char* smem, int tid, int threads) {
    const int64_t att_at = staged_size(f.count, f.cs).att_at;
    const StagedTables lds{reinterpret_cast<const int16_t*>(smem), smem + att_at, tables_staged(f, g, lds_bytes)};
    if (lds.on) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(g.cb + f.cb_off);
        uint32_t* dst = reinterpret_cast<uint32_t*>(smem);
        const int nw = (int)(((int64_t)f.count * f.cs + 1) / 2);
        for (int i = tid; i < nw; i += threads) dst[i] = src[i];
        for (int i = tid; i < f.count; i += threads) smem[att_at + i] = g.att[f.att_off + i];
    }
    return lds;
}

// Sample j of the chunk of symbol word w: from the staged tables, or from the
// global slabs with every index clamped to its slab.
__device__ __forceinline__ int16_t table_sample(const FrameTables& f, const int* lut, uint32_t w, int j,
                                                const StagedTables& lds, const TableSlabs& g) {
    int idx, neg, jj;
    symbol_fields(w, f.count, f.cs, j, &idx, &neg, &jj);
    int a, v;
    if (lds.on) {
        a = lds.att[idx];
        v = lds.cb[idx * f.cs + jj];
    } else {
        int64_t ai = f.att_off + idx, ci = f.cb_off + (int64_t)idx * f.cs + jj;
        ai = ai < 0 ? 0 : (ai >= g.natt ? g.natt - 1 : ai);
        ci = ci < 0 ? 0 : (ci >= g.ncb ? g.ncb - 1 : ci);
        a = g.att[ai];
        v = g.cb[ci];
    }
    return synth_sample(lut[neg * 16 + (a & 15)], v);
}

// ---- what the crop kernels share (gsc_decode_crops.hip, gsc_decode_resample.hip) ----

// Segment seg of frame f of a crop's stream to o[0 .. kDecodeS); false (nothing
// written) when the segment or its checkpoint lies outside the stream's slabs.
__device__ __forceinline__ bool unpack_crop_segment(const CropJob& job, const ResFrame& f, int64_t seg,
                                                    uint16_t* o) {
    if (seg < 0 || seg > f.nsym / kDecodeS) return false;
    const int64_t s0 = seg * kDecodeS;
    if (s0 >= f.nsym) return false;
    const int n = (int)(f.nsym - s0 < kDecodeS ? f.nsym - s0 : kDecodeS);
    const int64_t c = f.cp_first + seg;
    if (c < 0 || c >= job.ncp || f.bs_off < 0) return false;
    unpack_segment(job.words, job.nwords, f.bs_off, job.cps[c], f.ver, f.count, n, o);
    return true;
}

template <typename T>
__device__ __forceinline__ T to_out(int16_t v);
template <>
__device__ __forceinline__ int16_t to_out<int16_t>(int16_t v) {
    return v;
}
template <>
__device__ __forceinline__ float to_out<float>(int16_t v) {
    return (float)v * (1.0f / 32768.0f);
}

// the frame of [f0, f1) that holds sample s: the last one whose first sample is <= s
__device__ __forceinline__ int crop_frame_of(const CropJob& job, int f0, int f1, int64_t s) {
    return last_le(f0, f1 - 1, s, [&](int i) { return job.frames[i].first_sample; });
}

// the tables of a crop's stream in global memory
__device__ __forceinline__ TableSlabs crop_tables(const CropJob& job) {
    return TableSlabs{job.cb, job.ncb, job.att, job.natt};
}

// Element l of a run of nt samples x channels that starts at sample ta of a
// crop's row: its sample, its channel, and its place in the output.
template <bool PLANAR>
__device__ __forceinline__ int64_t crop_elem(int l, int nt, int64_t ta, int channels, int64_t length, int64_t out_base,
                                             int64_t* t, int* k) {
    if (PLANAR) {
        *k = l / nt;
        *t = ta + (l - *k * nt);
        return out_base + (int64_t)*k * length + *t;
    }
    *t = ta + l / channels;
    *k = l % channels;
    return out_base + *t * channels + *k;
}

// value(t, k) for samples [ta, tb) of a crop's row, every channel, by a whole workgroup
template <typename T, bool PLANAR, typename Value>
__device__ __forceinline__ void crop_write_run(int64_t ta, int64_t tb, int channels, int64_t length, int64_t out_base,
                                               T* __restrict__ out, int64_t nout, int tid, int threads, Value value) {
    const int nt = (int)(tb - ta);
    for (int l = tid; l < nt * channels; l += threads) {
        int64_t t;
        int k;
        const int64_t oi = crop_elem<PLANAR>(l, nt, ta, channels, length, out_base, &t, &k);
        if (oi >= 0 && oi < nout) out[oi] = to_out<T>(value(t, k));
    }
}

// The walk of the native-rate crop kernels (crop_fused_kernel,
// crop_fused_bound_kernel, mix_fused_kernel).  A workgroup owns samples
// [t0, t1) of one crop's row, every channel: [t0, tc) are decoded, [tc, t1) lie
// past the crop's clipped length.  The frames that [t0, tc) crosses are taken
// one after another: frame(job, f, fr, ta, tb, write) hands the frame's share
// [ta, tb) to write(ua, ub, value) and puts its own barriers around what it
// keeps in LDS.  blank(ua, ub) gets what is past the clipped length and what no
// frame of a stale span covers.  write and blank are the caller's sink: the crop
// kernels store, the mix kernels accumulate.
template <typename Write, typename Blank, typename Frame>
__device__ __forceinline__ void crop_walk_run(const CropJob& job, int64_t t0, int64_t t1, Write write, Blank blank,
                                              Frame frame) {
    const bool span_ok = job.f0 >= 0 && job.f0 < job.f1 && job.f1 <= job.nframes;
    const int64_t tc = !span_ok ? t0 : (job.count < t1 ? (job.count > t0 ? job.count : t0) : t1);
    blank(tc, t1);
    if (tc <= t0) return;
    const int fa = crop_frame_of(job, job.f0, job.f1, job.begin + t0);
    const int fb = crop_frame_of(job, job.f0, job.f1, job.begin + tc - 1);
    int64_t done = t0;  // every sample of [t0, done) is written
    for (int fr = fa; fr <= fb; ++fr) {
        const ResFrame& f = job.frames[fr];
        if (f.cs <= 0 || f.ch <= 0 || f.ch > 255 || f.count <= 0 || f.nsym <= 0) continue;
        // this frame's share of the run
        int64_t ta = f.first_sample - job.begin, tb = ta + f.nsym / f.ch * f.cs;
        ta = ta < done ? done : ta;
        tb = tb > tc ? tc : tb;
        if (ta >= tb) continue;
        blank(done, ta);
        frame(job, f, fr, ta, tb, write);
        done = tb;
    }
    blank(done, tc);
}

// ---- the fused walk of a frame (crop_fused_kernel, crop_fused_bound_kernel, envelope_kernel) ----

// No symbol scratch and no unpack launch.  A workgroup takes a run of tile_len
// samples of one crop; per frame the run crosses, and per stretch of symbol
// rows whose symbols span at most kFusedSegs checkpoint segments, its first
// lanes unpack those segments into LDS (one lane per segment, as
// decode_unpack_kernel), then all lanes write the stretch's samples with the
// codebook read from global memory.
constexpr int kFusedThreads = 256;
constexpr int kFusedSegs = 64;

// crop_walk_job's `frame` of the fused kernels: ssym holds kFusedSegs segments, slut 32 words
__device__ __forceinline__ auto fused_frame(uint16_t* ssym, int* slut, int tid) {
    return [=](const CropJob& job, const ResFrame& f, int, int64_t ta, int64_t tb, auto write) {
        const int cs = f.cs, ch = f.ch;
        const TableSlabs g = crop_tables(job);
        const int64_t off = job.begin - f.first_sample;  // sample of the frame = off + t
        const int64_t qa = (off + ta) / cs, qb = (off + tb - 1) / cs;
        // rows per stretch: their symbols span at most kFusedSegs segments wherever the stretch starts
        const int64_t rows = (int64_t)(kFusedSegs - 1) * kDecodeS / ch;
        for (int64_t q0 = qa; q0 <= qb; q0 += rows) {
            const int64_t q1 = q0 + rows - 1 < qb ? q0 + rows - 1 : qb;
            const int64_t seg_lo = q0 * ch / kDecodeS;
            int64_t nseg = ((q1 + 1) * ch - 1) / kDecodeS - seg_lo + 1;
            nseg = nseg > kFusedSegs ? kFusedSegs : nseg;
            __syncthreads();  // the previous stretch's symbols are no longer read
            if (tid < 32) slut[tid] = f.lut[tid];
            for (int i = tid; i < (int)nseg; i += kFusedThreads) {
                uint16_t* o = ssym + i * kDecodeS;
                if (!unpack_crop_segment(job, f, seg_lo + i, o))
                    for (int z = 0; z < kDecodeS; ++z) o[z] = 0;
            }
            __syncthreads();
            int64_t ua = q0 * cs - off, ub = (q1 + 1) * cs - off;
            ua = ua < ta ? ta : ua;
            ub = ub > tb ? tb : ub;
            write(ua, ub, [&](int64_t t, int k) {
                const int64_t local = off + t;
                const int64_t rel = local / cs * ch + k - seg_lo * kDecodeS;  // the symbol's place in ssym
                if (k < ch && local >= 0 && rel >= 0 && rel < nseg * kDecodeS && local / cs * ch + k < f.nsym)
                    return table_sample(f, slut, ssym[rel], (int)(local % cs), StagedTables{}, g);
                return (int16_t)0;
            });
        }
    };
}

// ---- crops whose list lives on the device (gsc_crop_binding_decode) ----

// A value every lane of the wave holds alike, in scalar registers from here on.
__device__ __forceinline__ int32_t wave_uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)((uint64_t)hi << 32 | lo);
}
template <typename P>
__device__ __forceinline__ const P* wave_uniform(const P* p) {
    return reinterpret_cast<const P*>((uintptr_t)wave_uniform((int64_t)reinterpret_cast<uintptr_t>(p)));
}

// One lane: the CropJob of crop c = (stream, begin, count) of a bound call, as
// plan_crops and the host fill it for the other calls.
// Returns what the call reports as written: the clipped count, or -1 for a bad
// crop, whose job is empty (f0 == f1), so that the kernels zero its row and
// read nothing through it.  The stream index is checked before it is used, the
// frame searches stay inside [0, nframes).
__device__ __forceinline__ int64_t bound_plan(const BoundStream* __restrict__ streams, int nstreams,
                                              const int64_t* __restrict__ c, int64_t length, int out_ch,
                                              CropJob* job) {
    CropJob j{};
    int64_t written = -1;
    const int64_t s = c[0], begin = c[1], count = c[2];
    if (crop_stream_status(s, nstreams) == kCropGood) {
        const BoundStream& d = streams[s];
        const ResFrame* frames = d.frames;
        CropSpan sp;
        if (crop_plan_one(begin, count, length, d.samples, d.nframes, d.rate_up, d.rate_down, d.half_taps,
                          [&](int i) { return frames[i].first_sample; }, &sp) == kCropGood) {
            j = CropJob{frames,     d.cps,     d.words,  d.cb,      d.att, d.ncp, d.nwords,     d.ncb,
                        d.natt,     begin,     sp.count, d.nframes, sp.f0, sp.f1, sp.src_begin,
                        sp.src_end, d.table,   d.rate_up, d.rate_down, d.half_taps, d.channels, out_ch};
            written = sp.count;
        }
    }
    *job = j;
    return written;
}

// bound_job's LDS: a whole number of 16 bytes, so that a kernel's static LDS
// stays one and its dynamic LDS starts 16-byte aligned
struct alignas(16) SharedJob {
    CropJob job;
};

// A job that one lane left in LDS, to every wave's scalar registers (after the barrier that
// follows the store).
__device__ __forceinline__ CropJob shared_job_load(const CropJob* sjob) {
    CropJob j;
    j.frames = wave_uniform(sjob->frames);
    j.cps = wave_uniform(sjob->cps);
    j.words = wave_uniform(sjob->words);
    j.cb = wave_uniform(sjob->cb);
    j.att = wave_uniform(sjob->att);
    j.ncp = wave_uniform(sjob->ncp);
    j.nwords = wave_uniform(sjob->nwords);
    j.ncb = wave_uniform(sjob->ncb);
    j.natt = wave_uniform(sjob->natt);
    j.begin = wave_uniform(sjob->begin);
    j.count = wave_uniform(sjob->count);
    j.nframes = wave_uniform(sjob->nframes);
    j.f0 = wave_uniform(sjob->f0);
    j.f1 = wave_uniform(sjob->f1);
    j.src_begin = wave_uniform(sjob->src_begin);
    j.src_end = wave_uniform(sjob->src_end);
    j.table = wave_uniform(sjob->table);
    j.rate_up = wave_uniform(sjob->rate_up);
    j.rate_down = wave_uniform(sjob->rate_down);
    j.half_taps = wave_uniform(sjob->half_taps);
    j.src_ch = wave_uniform(sjob->src_ch);
    j.out_ch = wave_uniform(sjob->out_ch);
    return j;
}

// Every lane of a workgroup, once, before anything else: the job of the
// workgroup's crop.  Lane 0 alone reads the crop and runs the two frame
// searches (bound_plan), leaves the job in *sjob (LDS) and, in the crop's first
// tile, stores written[crop]; after the barrier every wave takes the job to
// scalar registers, so that the rest of the kernel sees what a job loaded from
// the host's array gives it.
__device__ __forceinline__ CropJob bound_job(const BoundStream* __restrict__ streams, int nstreams,
                                             const int64_t* __restrict__ crops, int64_t crop, bool first_tile,
                                             int64_t length, int out_ch, int64_t* __restrict__ written,
                                             SharedJob* shared) {
    CropJob* sjob = &shared->job;
    if (threadIdx.x == 0) {
        const int64_t w = bound_plan(streams, nstreams, crops + 3 * crop, length, out_ch, sjob);
        if (first_tile && written) written[crop] = w;
    }
    __syncthreads();
    return shared_job_load(sjob);
}

// ---- the resampling crop kernels (gsc_decode_resample.hip, gsc_decode_mix.hip) ----

constexpr int kResThreads = 256;
constexpr int kResSegs = 16;  // checkpoint segments of one stretch in LDS

// Samples [sa, sb) of a crop's stream, every channel, to
// ssrc[(s - ia) * ch + k], by a whole workgroup; what no frame covers stays as it is.
__device__ __forceinline__ void resample_fill(const CropJob& job, int64_t sa, int64_t sb, int64_t ia, int ch,
                                              int16_t* ssrc, int src_cap, uint16_t* ssym, int* slut, int tid) {
    const TableSlabs g = crop_tables(job);
    const int fa = crop_frame_of(job, job.f0, job.f1, sa);
    const int fb = crop_frame_of(job, job.f0, job.f1, sb - 1);
    for (int fr = fa; fr <= fb; ++fr) {
        const ResFrame& f = job.frames[fr];
        if (f.cs <= 0 || f.ch != ch || f.count <= 0 || f.nsym <= 0) continue;
        const int cs = f.cs;
        const int64_t fs = f.first_sample, fe = fs + f.nsym / ch * cs;
        const int64_t xa = sa > fs ? sa : fs, xb = sb < fe ? sb : fe;
        if (xa >= xb) continue;
        const int64_t qa = (xa - fs) / cs, qb = (xb - 1 - fs) / cs;
        // rows per stretch: their symbols span at most kResSegs segments wherever the stretch starts
        const int64_t rows = (int64_t)(kResSegs - 1) * kDecodeS / ch;
        for (int64_t q0 = qa; q0 <= qb; q0 += rows) {
            const int64_t q1 = q0 + rows - 1 < qb ? q0 + rows - 1 : qb;
            const int64_t seg_lo = q0 * ch / kDecodeS;
            int64_t nseg = ((q1 + 1) * ch - 1) / kDecodeS - seg_lo + 1;
            nseg = nseg > kResSegs ? kResSegs : nseg;
            __syncthreads();  // the previous stretch's symbols are no longer read
            if (tid < 32) slut[tid] = f.lut[tid];
            for (int i = tid; i < (int)nseg; i += kResThreads) {
                uint16_t* o = ssym + i * kDecodeS;
                if (!unpack_crop_segment(job, f, seg_lo + i, o))
                    for (int z = 0; z < kDecodeS; ++z) o[z] = 0;
            }
            __syncthreads();
            int64_t ua = fs + q0 * cs, ub = fs + (q1 + 1) * cs;
            ua = ua < xa ? xa : ua;
            ub = ub > xb ? xb : ub;
            const int64_t n = (ub - ua) * ch;
            for (int64_t l = tid; l < n; l += kResThreads) {
                const int64_t s = ua + l / ch;
                const int k = (int)(l % ch);
                const int64_t local = s - fs;
                const int64_t si = local / cs * ch + k, rel = si - seg_lo * kDecodeS;
                int16_t v = 0;
                if (rel >= 0 && rel < nseg * kDecodeS && si < f.nsym)
                    v = table_sample(f, slut, ssym[rel], (int)(local % cs), StagedTables{}, g);
                const int64_t di = (s - ia) * ch + k;
                if (di >= 0 && di < src_cap) ssrc[di] = v;
            }
        }
    }
}

// Outputs [t0, t1) of one crop's row, a tile of at most tile_len, by a whole
// workgroup (crop_resample_kernel, crop_resample_bound_kernel, mix_resample_kernel):
// write(ua, ub, value) gets the outputs of a pass, blank(ua, ub) what lies past
// the crop's clipped length or belongs to a job that fails a check.  ssrc holds
// src_cap int16, ssym kResSegs segments, slut 32 words.  write and blank are the
// caller's sink: the crop kernels store, the mix kernels accumulate.
template <typename Write, typename Blank>
__device__ __forceinline__ void resample_run(const CropJob& job, int64_t t0, int64_t t1, int tile_len, int channels,
                                             int src_cap, int16_t* ssrc, uint16_t* ssym, int* slut, Write write,
                                             Blank blank) {
    const int tid = threadIdx.x;
    const int L = job.rate_up, M = job.rate_down, H = job.half_taps, C = job.src_ch;
    const int taps = 2 * H, before = H > 0 ? H - 1 : 0;
    // what the 32-bit position arithmetic of a pass and the LDS indices rely on
    bool ok = job.f0 >= 0 && job.f0 < job.f1 && job.f1 <= job.nframes && L > 0 && L <= (1 << 17) && M > 0 &&
              M <= (1 << 21) && H >= 0 && taps <= kResampleMaxTaps && (H == 0 || job.table != nullptr) && C > 0 &&
              C <= 255 && job.out_ch == channels && (C == channels || C == 1 || channels == 1) && job.begin >= 0 &&
              job.begin <= ((int64_t)1 << 40) && job.src_begin >= 0 && job.src_begin <= job.src_end;
    const int64_t cap = ok ? src_cap / C : 0;  // source samples per channel of a pass
    ok = ok && cap - taps - 2 >= 0;
    // outputs per pass: n outputs read at most (n - 1) * M / L + taps + 2 source samples
    int64_t sub = ok ? (cap - taps - 2) * L / M + 1 : 1;
    sub = sub > tile_len ? tile_len : sub;
    const int64_t tc = !ok ? t0 : (job.count < t1 ? (job.count > t0 ? job.count : t0) : t1);
    blank(tc, t1);
    for (int64_t na = t0; na < tc; na += sub) {
        const int64_t nb = na + sub < tc ? na + sub : tc;
        // output n sits at source position (begin * L + n * M) / L; within a pass the offset fits 32 bits
        const int64_t p = job.begin * L + na * M;
        const int64_t bi = p / L;
        const uint32_t br = (uint32_t)(p - bi * L);
        const uint32_t ul = br + (uint32_t)(nb - 1 - na) * (uint32_t)M;
        const int64_t ia = bi - before, ib = bi + ul / (uint32_t)L + H;  // the span, both ends included
        const int64_t span = ib - ia + 1;
        if (span > cap) {  // never, by the choice of sub
            blank(na, nb);
            continue;
        }
        __syncthreads();  // the previous pass's span is no longer read
        for (int i = tid; i < (int)span * C; i += kResThreads) ssrc[i] = 0;
        __syncthreads();
        const int64_t sa = ia > job.src_begin ? ia : job.src_begin, sb = ib + 1 < job.src_end ? ib + 1 : job.src_end;
        if (sa < sb) resample_fill(job, sa, sb, ia, C, ssrc, (int)span * C, ssym, slut, tid);
        __syncthreads();
        // channel k of the output at offset u = br + (n - na) * M of the pass
        auto one = [&](uint32_t qi, const int32_t* __restrict__ row, int k) {
            const int16_t* x = ssrc + (int)qi * C + k;  // (qi + taps - 1) * C + k < span * C
            if (H == 0) return (int)x[0];
            int64_t acc = 0;
            for (int j = 0; j < taps; ++j) acc += (int64_t)row[j] * (int64_t)x[j * C];
            const int64_t y = (acc + ((int64_t)1 << (kResampleShift - 1))) >> kResampleShift;
            return (int)(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
        };
        write(na, nb, [&](int64_t n, int c) {
            const uint32_t u = br + (uint32_t)(n - na) * (uint32_t)M;
            const uint32_t qi = u / (uint32_t)L, phase = u - qi * (uint32_t)L;
            const int32_t* row = job.table + (int64_t)phase * taps;
            if (C == channels) return (int16_t)one(qi, row, c);
            if (C == 1) return (int16_t)one(qi, row, 0);
            int sum = 0;  // channels == 1: the mean, rounded half up
            for (int k = 0; k < C; ++k) sum += one(qi, row, k);
            const int num = 2 * sum + C, den = 2 * C;
            int q = num / den;
            q -= (num % den < 0) ? 1 : 0;
            return (int16_t)q;
        });
    }
}


// f(T{}, std::bool_constant<PLANAR>{}) for the output's element type and layout
template <typename F>
hipError_t dispatch_out(int is_float, int planar, F f) {
    if (is_float) return planar ? f(float{}, std::true_type{}) : f(float{}, std::false_type{});
    return planar ? f(int16_t{}, std::true_type{}) : f(int16_t{}, std::false_type{});
}

// Raises the dynamic LDS a kernel may use once per device and size, not per
// launch: the limit belongs to the kernel as loaded on one device, so what was
// granted is remembered per device ordinal (past kDevices, asked every time).
struct LdsLimit {
    static constexpr int kDevices = 16;
    std::atomic<int> granted[kDevices] = {};
};
template <typename K>
hipError_t allow_lds(K kernel, int lds_bytes, LdsLimit* lim) {
    if (lds_bytes <= 32 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<int>* slot = dev >= 0 && dev < LdsLimit::kDevices ? &lim->granted[dev] : nullptr;
    if (slot && lds_bytes <= slot->load(std::memory_order_relaxed)) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            lds_bytes);
    if (e == hipSuccess && slot) slot->store(lds_bytes, std::memory_order_relaxed);
    return e;
}

}  // namespace gsc
