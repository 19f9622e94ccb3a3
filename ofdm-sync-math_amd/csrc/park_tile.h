// park_tile.h — the LDS-tiled direct-sum engine shared by corr.hip (ofs_park_metric, the ZC matched
// filter) and park_chunk.hip (ofs_park_metric_chunk): the sample loaders, the tile geometry and the
// body of one Park tile.  park_kernel and park_chunk_kernel both run park_tile(), so an output of the
// chunked call is computed by the very expressions of the one-shot call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ofdmsync.h"

namespace ofs_tile {

template <class R> struct C2;
template <> struct C2<float> { using T = float2; };
template <> struct C2<double> { using T = double2; };

template <int FMT, class R>
__device__ __forceinline__ typename C2<R>::T ld_c(const void* p, int64_t i) {
    typename C2<R>::T o;
    if constexpr (FMT == OFS_C64) {
        const float2 v = reinterpret_cast<const float2*>(p)[i];
        o.x = (R)v.x; o.y = (R)v.y;
    } else if constexpr (FMT == OFS_C128) {
        const double2 v = reinterpret_cast<const double2*>(p)[i];
        o.x = (R)v.x; o.y = (R)v.y;
    } else {
        const short2 v = reinterpret_cast<const short2*>(p)[i];
        o.x = (R)v.x; o.y = (R)v.y;
    }
    return o;
}

constexpr int CW = 256;          // threads per workgroup (Park, matched filter)
constexpr int OPT = 8;           // consecutive outputs per thread
constexpr int CD = CW * OPT;     // outputs per workgroup tile
constexpr int PADF = OPT;        // front pad of the staged tile (Park's backward window)

__host__ __device__ constexpr int64_t split_stride(int64_t len) { return (len + OPT - 1) / OPT | 1; }

// samples of one staged Park tile and the dynamic LDS it takes
__host__ __device__ constexpr int64_t park_tile_len(int half) { return CD + 2 * (int64_t)half - 2 + 2 * PADF; }
template <class R>
constexpr size_t park_tile_lds(int half) {
    return (size_t)split_stride(park_tile_len(half)) * OPT * sizeof(typename C2<R>::T);
}

// ------------------------------------------------------------------------------------------
// Park: P(d) = Σ_br Σ_{k<half} x[d-k]·x[d+k]; E(d) = Σ_br Σ_{k<half} |x[d+k]|²;
//       M = |P|²/max(E,1e-12)²;  d = half + i   (park.py:76-113)
// Tile: outputs i in [i0, i0 + CD), global samples g in [g0, g0 + len), g0 = i0 + 1 - PADF, fetched
// through load(br, g) (zero outside the stream).
// Thread t, output q: backward b_q = x[d-k], forward f_q = x[d+k]; per step k one new
// backward value (q = 0) and one new forward value (q = OPT-1) come from LDS; the others
// rotate through a ring whose slot is (q ∓ k) mod OPT, resolved at compile time by
// unrolling k by OPT.
// ------------------------------------------------------------------------------------------
// Energy: the OPT outputs of a thread share all but the first / last few samples of their
// windows, so (SPLIT, half >= OPT) E_q = C + H_q + T_q with C = Σ_{k=OPT-1}^{half-1} |x[d0+k]|²
// (accumulated once, from output 0's forward values), H_q = Σ_{k=q}^{OPT-2} |x[d0+k]|² and
// T_q = Σ_{k=half}^{half+q-1} |x[d0+k]|² — sums of non-negative terms only, 2 instead of 2·OPT FMAs
// per step.
// (packed forms of the complex MAC measured no faster for fp32 - vector-type swizzles 3.95 ms, two
// inline-asm v_pk_fma_f32 with op_sel 2.67 ms, against 2.51 ms for the scalar FMAs: r02ab)
//
// Nothing an output computes depends on i0 or on the stream around its window: P is one FMA chain
// over branches and k, the SPLIT energy rounds by the output's position q = i mod OPT in its thread
// (i0 is a multiple of OPT in both callers), and a sample outside [i+1, i+2·half-1] reaches output i
// nowhere.  Outputs i in [lo, hi) are stored, at index i - ioff of the row pointers.
template <class R, class V>
__device__ __forceinline__ void park_mac(const V& b, const V& f, R& pr, R& pi) {
    pr = fma(b.x, f.x, fma(-b.y, f.y, pr));
    pi = fma(b.x, f.y, fma(b.y, f.x, pi));
}

template <class R, bool SPLIT, class Load>
__device__ __forceinline__ void park_tile(typename C2<R>::T* seg, int64_t i0, int nb, int half, Load load,
                                          int64_t lo, int64_t hi, int64_t ioff, R* __restrict__ Mo,
                                          R* __restrict__ Po, R* __restrict__ Eo) {
    using V = typename C2<R>::T;
    const int t = threadIdx.x;
    const int64_t g0 = i0 + 1 - PADF;
    const int64_t len = park_tile_len(half);
    const int64_t S = split_stride(len);
    const int ksteps = (half + OPT - 1) / OPT * OPT;
    // a thread none of whose outputs is stored only helps staging (the last tile of a stream; a chunk
    // call's first and last tile, where whole waves are idle when the chunk is short)
    const int64_t it = i0 + (int64_t)OPT * t;
    const bool live = it < hi && it + OPT > lo;

    R pr[OPT], pi[OPT], en[OPT];
#pragma unroll
    for (int q = 0; q < OPT; ++q) { pr[q] = 0; pi[q] = 0; en[q] = 0; }

    for (int br = 0; br < nb; ++br) {
        __syncthreads();
        for (int64_t j = t; j < len; j += CW) seg[(j % OPT) * S + j / OPT] = load(br, g0 + j);
        __syncthreads();
        if (!live) continue;                              // (every thread still meets the barriers above)
        // seg index of x[d0 + OPT*t + q + m] is PADF + half - 1 + OPT*t + q + m
        auto at = [&](int64_t j) -> V { return seg[(j % OPT) * S + j / OPT]; };
        const int64_t c0 = PADF + half - 1 + (int64_t)OPT * t;
        V bw[OPT], fw[OPT];
#pragma unroll
        for (int q = 0; q < OPT; ++q) { bw[q] = at(c0 + q); fw[q] = at(c0 + q); }
        R ce = 0;                                         // SPLIT: C of this branch
        for (int kk = 0; kk < ksteps; kk += OPT) {
#pragma unroll
            for (int u = 0; u < OPT; ++u) {
                const int k = kk + u;
                if (k < half) {
#pragma unroll
                    for (int q = 0; q < OPT; ++q) {
                        const V bq = bw[(q - u + OPT) % OPT];
                        const V fq = fw[(q + u) % OPT];
                        park_mac<R, V>(bq, fq, pr[q], pi[q]);
                        if (!SPLIT) en[q] = fma(fq.x, fq.x, fma(fq.y, fq.y, en[q]));
                    }
                    if (SPLIT && (kk > 0 || u >= OPT - 1)) {
                        const V f0 = fw[u % OPT];         // x[d0 + k]
                        ce = fma(f0.x, f0.x, fma(f0.y, f0.y, ce));
                    }
                }
                // next step: new backward x[d0+OPT t-(k+1)] into slot of b_{OPT-1},
                //            new forward  x[d0+OPT t+OPT-1+k+1] into slot of f_0
                bw[(OPT - 1 - u + OPT) % OPT] = at(c0 - (k + 1));
                fw[u % OPT] = at(c0 + OPT + k);
            }
        }
        if constexpr (SPLIT) {
            R hd[OPT], tl[OPT];                           // |x[d0+k]|², |x[d0+half+k]|², k < OPT-1
#pragma unroll
            for (int k = 0; k < OPT - 1; ++k) {
                const V h = at(c0 + k), w = at(c0 + half + k);
                hd[k] = fma(h.x, h.x, h.y * h.y);
                tl[k] = fma(w.x, w.x, w.y * w.y);
            }
            R hs = 0, ts = 0;
#pragma unroll
            for (int q = OPT - 1; q >= 0; --q) {          // H_q: suffix of hd from q
                en[q] += ce + hs;
                if (q > 0) hs += hd[q - 1];
            }
#pragma unroll
            for (int q = 1; q < OPT; ++q) { ts += tl[q - 1]; en[q] += ts; }   // T_q
        }
    }
#pragma unroll
    for (int q = 0; q < OPT; ++q) {
        const int64_t i = i0 + (int64_t)OPT * t + q;
        if (i >= lo && i < hi) {
            const int64_t o = i - ioff;
            const R e = en[q] > (R)1e-12 ? en[q] : (R)1e-12;
            if (Mo) Mo[o] = (pr[q] * pr[q] + pi[q] * pi[q]) / (e * e);
            if (Po) { Po[2 * o] = pr[q]; Po[2 * o + 1] = pi[q]; }
            if (Eo) Eo[o] = en[q];
        }
    }
}

}  // namespace ofs_tile
