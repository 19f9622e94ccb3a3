// aa_words.h — sample access and row prefixes shared by the wave-per-stream integer / fp64 kernels
// (aa_exact.hip, aa_chunk.hip): int16 I/Q words, packed 12-bit AXIS words, complex128.
#pragma once
#include "ofs_common.h"
#include "ofdmsync.h"

namespace ofs {

// E consecutive int16 I/Q words (packed (I, Q) in one int32) of one lane, zero past T
template <int E>
__device__ __forceinline__ void load_words(const int32_t* xs, int64_t n0, int64_t T, int32_t (&w)[E]) {
    if (n0 + E <= T && (reinterpret_cast<uintptr_t>(xs + n0) & (4 * E - 1)) == 0) {
        if constexpr (E == 1) {
            w[0] = xs[n0];
        } else if constexpr (E == 2) {
            const int2 v = *reinterpret_cast<const int2*>(xs + n0);
            w[0] = v.x; w[1] = v.y;
        } else {
#pragma unroll
            for (int j = 0; j < E; j += 4) {
                const int4 v = *reinterpret_cast<const int4*>(xs + n0 + j);
                w[j] = v.x; w[j + 1] = v.y; w[j + 2] = v.z; w[j + 3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = (n0 + e < T) ? xs[n0 + e] : 0;
    }
}
// OFS_CP12: E consecutive time indices n0.. of the NA channels of one stream (base x8), decoded
// to the int16 I/Q words above.  Fast path: the lane's 3·NA·E bytes with dword loads from the
// dword below, realigned with v_alignbyte (groups then sit at compile-time byte offsets); used
// when the row is whole and the rounded-up dword window stays inside the buffer.  Otherwise per
// byte with zero fill past T.
__device__ __forceinline__ int32_t cp12_word(uint32_t g) {
    const int32_t i = ((int32_t)(g << 20)) >> 20;              // bits 0-11, sign-extended
    const int32_t q = ((int32_t)(g << 8)) >> 20;               // bits 12-23
    return (i & 0xffff) | (int32_t)((uint32_t)q << 16);
}
template <int E, int NA>
__device__ __forceinline__ void cp12_load(const uint8_t* x8, int64_t sbyte, int64_t n0, int64_t T, int64_t total,
                                          int32_t (&w)[NA][E]) {
    constexpr int NB = 3 * NA * E;                              // bytes wanted
    constexpr int ND = (NB + 3 + 3) / 4;                        // dwords covering them at any shift
    const int64_t p = sbyte + 3 * NA * n0;                      // absolute byte offset in the buffer
    const int64_t a = p & ~(int64_t)3;
    if (n0 + E <= T && a + 4 * ND <= total) {
        const uint32_t* d = reinterpret_cast<const uint32_t*>(x8 - sbyte + a);
        uint32_t v[ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) v[j] = d[j];
        const uint32_t sh = (uint32_t)(p & 3);
        uint32_t al[ND - 1];                                    // bytes p, p+1, ... in order
#pragma unroll
        for (int j = 0; j + 1 < ND; ++j) al[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], sh);
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
            for (int t = 0; t < NA; ++t) {
                const int bo = 3 * (e * NA + t);                // compile-time after unrolling
                const uint64_t win = ((uint64_t)al[bo / 4 + 1 < ND - 1 ? bo / 4 + 1 : ND - 2] << 32) | al[bo / 4];
                w[t][e] = cp12_word((uint32_t)(win >> (8 * (bo & 3))) & 0xffffffu);
            }
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
            for (int t = 0; t < NA; ++t) {
                if (n0 + e < T) {
                    const uint8_t* q = x8 + 3 * (NA * (n0 + e) + t);
                    w[t][e] = cp12_word((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16));
                } else {
                    w[t][e] = 0;
                }
            }
    }
}

__device__ __forceinline__ double w_re(int32_t w) { return (double)(int16_t)(w & 0xffff); }
__device__ __forceinline__ double w_im(int32_t w) { return (double)(w >> 16); }

// sample access of the wave-per-stream sync_aa kernel: int16 I/Q words (exact integer sums) or
// complex128 (fp64 prefix differences over the stream, the general engine's arithmetic)
template <int FMT> struct XSamp;
template <> struct XSamp<OFS_CI16> {
    using W = int32_t;
    static __device__ __forceinline__ W zero() { return 0; }
    static __device__ __forceinline__ double re(W w) { return w_re(w); }
    static __device__ __forceinline__ double im(W w) { return w_im(w); }
    template <int E>
    static __device__ __forceinline__ void load(const W* xs, int64_t n0, int64_t T, W (&w)[E]) {
        load_words<E>(xs, n0, T, w);
    }
};
template <> struct XSamp<OFS_C128> {
    using W = double2;
    static __device__ __forceinline__ W zero() { return make_double2(0.0, 0.0); }
    static __device__ __forceinline__ double re(W w) { return w.x; }
    static __device__ __forceinline__ double im(W w) { return w.y; }
    template <int E>
    static __device__ __forceinline__ void load(const W* xs, int64_t n0, int64_t T, W (&w)[E]) {
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = (n0 + e < T) ? xs[n0 + e] : zero();
    }
};

// in-lane inclusive prefix of v, then the lane's exclusive wave prefix and the row total
template <int E>
struct RowPrefix {
    double f[E], excl, tot;
    __device__ __forceinline__ void run(const double (&v)[E]) {
        f[0] = v[0];
#pragma unroll
        for (int e = 1; e < E; ++e) f[e] = f[e - 1] + v[e];
        const double incl = scan_add(f[E - 1]);
        excl = shr1z(incl);
        tot = readlane(incl, 63);
    }
};

}  // namespace ofs
