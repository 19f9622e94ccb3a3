// chunk_state.h — what the resumable chunk-fed calls (the *_chunk*.hip files) have in common.
//
// Every chunk entry point refuses the same arguments (chunk_args_bad).  The two metrics with a running
// peak (park_chunk.hip, zc_freq_chunk.hip) also share one state design: a 64-byte header with n_seen and
// the running first argmax, then a ring [n_br][Hr] of raw samples in the input's own format, keyed by the
// absolute sample index (sample g at slot g mod Hr).  Their metric kernels read the stream as
// [ring | chunk] (ring_slot); a second kernel, one workgroup per stream, writes the chunk's newest
// min(Tc, Hr) samples back (ring_write), scans the call's metric row (row_peak), folds the workgroup's
// candidates (peak_fold) into the carried peak and rewrites the header.  The headers themselves
// (ParkChunkHdr, ZfcHdr: ABI, include/ofdmsync.h) and the kernels stay with their detectors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ofdmsync.h"
#include "ofs_common.h"

namespace ofs_chunk {

// The refusal list of every chunk call: sizes, an empty chunk that is no flush, a missing or not
// 16-byte-aligned state, missing samples.  (A call adds its own conditions and returns OFS_OK for
// B = 0 only after all of them.)
inline bool chunk_args_bad(int64_t B, int64_t Tc, int64_t max_tc, int32_t final, const void* state, const void* x) {
    return B < 0 || Tc < 0 || Tc > max_tc || (Tc == 0 && !final) || OFS_MISSING(state, B) ||
           (reinterpret_cast<uintptr_t>(state) & 15) != 0 || OFS_MISSING(x, B * Tc);
}

// one raw sample of input format FMT, as the ring keeps it
template <int FMT> struct Sample { using T = short2; };                        // OFS_CI16
template <> struct Sample<OFS_C64> { using T = float2; };
template <> struct Sample<OFS_C128> { using T = double2; };
__host__ __device__ constexpr int sample_bytes(int fmt) { return fmt == OFS_C64 ? 8 : fmt == OFS_C128 ? 16 : 4; }

// [ring | chunk]: ring slot of the sample `back` places before sample n_seen (-Hr <= back < 0),
// r0 = n_seen mod Hr
__device__ __forceinline__ int ring_slot(int r0, int64_t back, int Hr) {
    int s = r0 + (int)back;                                                    // in (-Hr, Hr)
    if (s < 0) s += Hr;
    return s;
}

// the newest min(Tc, Hr) samples of stream b's chunk x[B][nb][Tc] into its ring [nb][Hr], by NT threads
template <int FMT, int NT>
__device__ __forceinline__ void ring_write(void* ringp, const void* x, int64_t b, int nb, int64_t Tc,
                                           int64_t n_seen, int Hr, int t) {
    using S = typename Sample<FMT>::T;
    S* ring = static_cast<S*>(ringp);
    const int64_t cnt = Tc < Hr ? Tc : Hr;
    const int r0 = (int)((n_seen + Tc - cnt) % Hr);
    for (int br = 0; br < nb; ++br) {
        const S* xs = static_cast<const S*>(x) + (b * nb + br) * Tc + (Tc - cnt);
        for (int64_t j = t; j < cnt; j += NT) {
            int s = r0 + (int)j;
            if (s >= Hr) s -= Hr;
            ring[(int64_t)br * Hr + s] = xs[j];
        }
    }
}

// running first argmax (np.argmax: the first maximal element; the first NaN wins once one appears)
struct ChunkPeak { double v; int64_t i; int kind; };                           // kind 0 none, 1 a number, 2 the first NaN
__device__ __forceinline__ bool peak_beats(const ChunkPeak& o, const ChunkPeak& m) {     // o replaces m
    if (o.kind == 0) return false;
    if (m.kind == 0) return true;
    if (o.kind != m.kind) return o.kind == 2;
    if (o.kind == 2) return o.i < m.i;
    return o.v > m.v || (o.v == m.v && o.i < m.i);
}

// this thread's peak over elements [j0, j1) of a metric row, element j at index i0 + j: NT threads, UL
// independent loads in flight per thread and round (one workgroup reads the whole row: with one load
// at a time the scan of a long row waits out one memory latency per element)
template <int NT, int UL, class R>
__device__ __forceinline__ ChunkPeak row_peak(const R* row, int64_t j0, int64_t j1, int64_t i0, int t) {
    ChunkPeak me{0.0, 0, 0};
    for (int64_t jb = j0 + t; jb < j1; jb += (int64_t)UL * NT) {
        double v[UL];
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int64_t j = jb + (int64_t)u * NT;
            v[u] = j < j1 ? (double)row[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int64_t j = jb + (int64_t)u * NT;
            const ChunkPeak c{v[u], i0 + j, j < j1 ? (v[u] != v[u] ? 2 : 1) : 0};
            if (peak_beats(c, me)) me = c;
        }
    }
    return me;
}

// The carried peak `pk` folded with the NT threads' candidates, returned to thread 0: a shuffle
// butterfly, then one LDS slot per wave.  Holds a __syncthreads(): what every thread read before the
// call (the state header) may be overwritten by thread 0 after it.
template <int NT>
__device__ __forceinline__ ChunkPeak peak_fold(ChunkPeak me, ChunkPeak pk, int t) {
    __shared__ ChunkPeak wp[NT / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const ChunkPeak o{__shfl_xor(me.v, m), __shfl_xor(me.i, m), __shfl_xor(me.kind, m)};
        if (peak_beats(o, me)) me = o;
    }
    if ((t & 63) == 0) wp[t >> 6] = me;
    __syncthreads();
    if (t == 0)
        for (int w = 0; w < NT / 64; ++w)
            if (peak_beats(wp[w], pk)) pk = wp[w];
    return pk;
}

}  // namespace ofs_chunk
