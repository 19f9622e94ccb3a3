// zs_body.h — the per-workgroup body of the block-initialised sliding DFT (zc_freq.compute_frequency_metric,
// zc_freq.py:62-99), shared by the one-shot kernels (zc_slide.hip) and the resumable chunk-fed kernels
// (zc_freq_chunk.hip), with the host-side plan both calls choose by.  The algorithm is described in
// zc_slide.hip.
//
// The two bodies are the statement lists zs_slide_body.h (per bin) and zs_pair_body.h (mirror pairs): a
// kernel includes one INSIDE its function body, with the argument block `a` (ZsArgs), the dynamic LDS
// `zsm`, a context `cx` and the template parameters NB, BPL or PPL, DEFER and OUT in scope.  They are
// text, not functions, so that the one-shot kernels stay the functions they were: the argument block is
// read as the kernel parameter it is, and the compiler emits for them the code it emitted before the
// body was shared (a body taking `a` by reference re-read it from memory behind every barrier and
// measured 0.5-1 % slower on the reference shape).  A context CX (every hook takes `a`):
//     CX::chunks(a, rows, W, c0, c1)  the workgroup's chunk range [c0, c1) (c1 - c0 <= rows·W)
//     CX::len(a)       samples T the stream has (samples i >= T are staged as zeros)
//     CX::row0(rb), CX::ld(a, row0 + r, i)   sample i (absolute, 0 <= i < T) of branch rb + r of the stream
//     CX::ld2(a, r, i0, N, p, v)      p = x[i0 + N], v = x[i0] of branch r
//     CX::end(a)       the stream's offset count T - (N + cp) + 1: the recursion's input d is zero from there on
//     CX::stored(a, s) offset s is stored by this call
//     CX::out(a)       out(a)[s] is where the metric of offset s goes
// Samples are read in the block phases (zs_blocks, zs_blocks_pair) and in the staging of d (zs_stage_d
// and its inline twin in the per-step DPP form of the per-bin body) only, all under an i < T guard.  Output s depends on x[cp + floor(s/C)·C .. cp + s + N - 1] and on s mod C, and
// on nothing else: not on c0, c1, W, the workgroup count or the stored range.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdint.h>
#include "chunk_state.h"

namespace {

struct ZsArgs {
    const void* x; int64_t B, T; int N, cp; int64_t noff;   // x, T, noff, metric: the one-shot context's (ZsWhole)
    int C, W;                      // chunk / block length (C | N), waves per workgroup
    int64_t nchunks, groups;       // chunks per stream, workgroups per stream
    int nbins; double t_energy; void* metric;
    int kb[64]; double tr[64], ti[64];
    int npairs; int pk[32], ps[32], pn[32];   // pair kernel: bins k (0 < k < N/2) and N-k at slots ps / pn
    int gblk;                                 // pair kernel: block DFTs by Goertzel pairs (else Horner per bin)
};

template <int FMT>
__device__ __forceinline__ double2 ldx(const void* p, int64_t i) {
    if constexpr (FMT == OFS_C64) {
        const float2 v = static_cast<const float2*>(p)[i];
        return make_double2(v.x, v.y);
    } else if constexpr (FMT == OFS_C128) {
        return static_cast<const double2*>(p)[i];
    } else {
        const short2 v = static_cast<const short2*>(p)[i];
        return make_double2(v.x, v.y);
    }
}

// The whole-stream context of the one-shot call: stream b = blockIdx.x / groups of x[B][NB][T], every
// offset stored.  It holds b only; every hook takes the kernel's argument block and is the expression
// the one-shot kernels had before the body was shared.
template <int FMT, int NB, class OUT>
struct ZsWhole {
    int64_t b;
    __device__ __forceinline__ void chunks(const ZsArgs& a, int rows, int W, int64_t& c0, int64_t& c1) {
        b = blockIdx.x / a.groups;
        const int64_t g = blockIdx.x - b * a.groups;
        c0 = g * rows * (int64_t)W;
        c1 = min(c0 + rows * (int64_t)W, a.nchunks);
    }
    __device__ __forceinline__ int64_t row0(int rb) const { return b * NB + rb; }
    __device__ __forceinline__ int64_t len(const ZsArgs& a) const { return a.T; }
    __device__ __forceinline__ int64_t end(const ZsArgs& a) const { return a.noff; }
    __device__ __forceinline__ double2 ld(const ZsArgs& a, int64_t row, int64_t i) const {
        return ldx<FMT>(a.x, row * a.T + i);
    }
    // p = x[i0 + N], v = x[i0] of branch r
    __device__ __forceinline__ void ld2(const ZsArgs& a, int r, int64_t i0, int N, double2& p, double2& v) const {
        const int64_t base = (b * NB + r) * a.T;
        p = ldx<FMT>(a.x, base + i0 + N);
        v = ldx<FMT>(a.x, base + i0);
    }
    __device__ __forceinline__ bool stored(const ZsArgs& a, int64_t s) const { return s < a.noff; }
    __device__ __forceinline__ OUT* out(const ZsArgs& a) const { return static_cast<OUT*>(a.metric) + b * a.noff; }
};

// The context of a chunk call: the stream is [ring | chunk].  Samples g < n_seen come from the ring
// [NB][Hr] of the state (slot g mod Hr; r0 = n_seen mod Hr), samples n_seen <= g < T = n_seen + Tc from
// the call's chunk x[B][NB][Tc]; offsets [lo, hi) are stored, offset s at element s - off0 of the row.
template <int FMT, int NB, class OUT>
struct ZsRing {
    const void* x; const void* ring; int64_t n_seen, T, lo, hi, Tc, xrow0, off0, c0, c1; int Hr, r0; OUT* row;
    __device__ __forceinline__ void chunks(const ZsArgs&, int, int, int64_t& c0_, int64_t& c1_) const { c0_ = c0; c1_ = c1; }
    __device__ __forceinline__ int64_t row0(int rb) const { return rb; }
    __device__ __forceinline__ int64_t len(const ZsArgs&) const { return T; }
    __device__ __forceinline__ int64_t end(const ZsArgs&) const { return hi; }
    __device__ __forceinline__ double2 ld(const ZsArgs&, int64_t r, int64_t i) const {
        if (i >= n_seen) return ldx<FMT>(x, (xrow0 + r) * Tc + (i - n_seen));
        if (i < n_seen - Hr) return make_double2(0.0, 0.0);            // (never read: Hr >= N + C - 2)
        return ldx<FMT>(ring, r * Hr + ofs_chunk::ring_slot(r0, i - n_seen, Hr));
    }
    __device__ __forceinline__ void ld2(const ZsArgs& a, int r, int64_t i0, int N, double2& p, double2& v) const {
        p = ld(a, r, i0 + N);
        v = ld(a, r, i0);
    }
    __device__ __forceinline__ bool stored(const ZsArgs&, int64_t s) const { return s >= lo && s < hi; }
    __device__ __forceinline__ OUT* out(const ZsArgs&) const { return row - off0; }   // out()[s], lo <= s < hi
};

// exp(-2 pi i m / N) for an exact integer m in [0, N)
__device__ __forceinline__ double2 twid(int64_t m, int N) {
    double s, c;
    sincospi(-2.0 * (double)m / (double)N, &s, &c);
    return make_double2(c, s);
}
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
// a * b + c
__device__ __forceinline__ double2 cfma(double2 a, double2 b, double2 c) {
    return make_double2(fma(a.x, b.x, fma(-a.y, b.y, c.x)), fma(a.x, b.y, fma(a.y, b.x, c.y)));
}
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
constexpr int ZS_MAXW = 16;

// sum over the LPC lanes of a row (8 or 16), result in every lane of the row
template <int LPC>
__device__ __forceinline__ double row_sum(double v) {
    v += ofs::dpp_d<0xB1>(v);          // quad_perm [1,0,3,2]
    v += ofs::dpp_d<0x4E>(v);          // quad_perm [2,3,0,1]
    if constexpr (LPC == 8) {
        v += ofs::dpp_d<0x141>(v);     // row_half_mirror: lane i <-> 7 - i within 8 lanes
    } else {
        v += ofs::dpp_d<0x124>(v);     // row_ror:4
        v += ofs::dpp_d<0x128>(v);     // row_ror:8
    }
    return v;
}

// DPP move into the lanes of the banks in BANK (4-lane groups of a 16-lane row), `old` elsewhere
template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_d_bank(double old, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xf, BANK, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xf, BANK, false);
    return __hiloint2double(hi, lo);
}

// Sums over the LPC lanes of a row of two steps' values at once (v0: step u, v1: step u + 1): the
// first stage pairs the row's lower half with its upper half and each side keeps one step (lower:
// u, upper: u + 1) and adds the partner's value of that step, so the remaining stages reduce ONE
// value: 1 + log2(LPC/2) stages for both steps instead of 2·log2(LPC).  Result: the lower half of
// the row holds Σ v0, the upper half Σ v1.
template <int LPC>
__device__ __forceinline__ double row_sum2(double v0, double v1) {
    constexpr int SWAP = LPC == 16 ? 0x128 : 0x141;   // row_ror:8 | row_half_mirror (lane i <-> 7 - i)
    constexpr int LO = LPC == 16 ? 0x3 : 0x5;         // banks of the lower half: 0,1 | 0,2
    constexpr int HI = 0xf ^ LO;
    const double keep = dpp_d_bank<0xE4, LO>(v1, v0);  // quad_perm identity: v0 in the lower half, else v1
    const double recv = dpp_d_bank<SWAP, HI>(dpp_d_bank<SWAP, LO>(v0, v0), v1);
    double v = keep + recv;
    v += ofs::dpp_d<0xB1>(v);                         // quad_perm [1,0,3,2]
    v += ofs::dpp_d<0x4E>(v);                         // quad_perm [2,3,0,1]
    if constexpr (LPC == 16) v += ofs::dpp_d<0x141>(v);   // row_half_mirror within the 8-lane half
    return v;
}

// Sums over a 16-lane row of four steps' values (v0..v3: steps u..u+3) by two reduce-scatter stages:
// row_ror:8 (lanes 0-7 keep steps u, u+1, lanes 8-15 steps u+2, u+3), then row_half_mirror (lane i
// <-> 7 - i: banks 0/2 keep the first of their two steps, banks 1/3 the second), then two quad
// stages on ONE value: 6 stages for four steps instead of 16.  Bank q of the row (lanes 4q..4q+3)
// ends with Σ v_q.
__device__ __forceinline__ double row_sum4(double v0, double v1, double v2, double v3) {
    const double k0 = dpp_d_bank<0xE4, 0x3>(v2, v0), k1 = dpp_d_bank<0xE4, 0x3>(v3, v1);
    const double a0 = k0 + dpp_d_bank<0x128, 0xC>(dpp_d_bank<0x128, 0x3>(v0, v0), v2);
    const double a1 = k1 + dpp_d_bank<0x128, 0xC>(dpp_d_bank<0x128, 0x3>(v1, v1), v3);
    double v = dpp_d_bank<0xE4, 0x5>(a1, a0) + dpp_d_bank<0x141, 0xA>(dpp_d_bank<0x141, 0x5>(a0, a0), a1);
    v += ofs::dpp_d<0xB1>(v);                         // quad_perm [1,0,3,2]
    v += ofs::dpp_d<0x4E>(v);                         // quad_perm [2,3,0,1]
    return v;
}

constexpr int ZS_G = 16;               // steps per group (one d staging, one store round)
// per-wave staging entries per branch: one block (phase 1), two half blocks (the pair kernel's
// phase 1) or ZS_G steps of d per row (phase 2)
__host__ __device__ constexpr int zs_stg(int C, int rows) {
    return C > ZS_G * rows ? (C > 128 ? C : 128) : (ZS_G * rows > 128 ? ZS_G * rows : 128);
}
// pair kernel: per-wave staging = one branch's block staging, or phase 2's d values of every branch
__host__ __device__ constexpr int zs_pair_stgw(int C, int rows, int nb) {
    return zs_stg(C, rows) > nb * rows * ZS_G ? zs_stg(C, rows) : nb * rows * ZS_G;
}
// pair kernel LDS: one branch's blocks (the workgroup's chunks + N/C - 1) + the waves' staging
__host__ __device__ constexpr size_t zs_pair_lds(int C, int N, int rows, int W, int nb) {
    return ((size_t)(rows * W + N / C - 1) * 64 + (size_t)W * zs_pair_stgw(C, rows, nb)) * 16;
}
constexpr int ZS_RG = 4;               // DEFER: steps per LDS partial round
constexpr int ZS_PS = 3 * 64 + 2;      // DEFER: doubles per step plane [cr, ci, e][64 lanes] + 16 B, so the
                                       // four summing lanes of a row read different bank groups
#ifndef OFS_ZS_UNROLL
#define OFS_ZS_UNROLL 2                // steps unrolled (tuning builds: -DOFS_ZS_UNROLL=1|4)
#endif
#ifndef OFS_ZS_DUNROLL
#define OFS_ZS_DUNROLL 1               // DEFER: steps unrolled per partial round (1 | 2 | 4)
#endif

// Phase 1 of both kernels: block DFTs β_k(m) = Σ_{j<C} x[cp + (c0+m)C + j] w^{kj} of the workgroup's
// nblk blocks into beta[m][NB][64 slots], one block per wave at a time (lane = bin slot, Horner in
// w^{4k} over four interleaved chains, samples broadcast from the wave's LDS staging).
template <int NB, class CX>
__device__ __forceinline__ void zs_blocks(const ZsArgs& a, const CX& cx, double2* beta, double2* stg, int STG, int64_t row0,
                                          int64_t c0, int nblk, int lane, int w) {
    const int C = a.C, N = a.N, W = a.W;
    const int kb = lane < a.nbins ? a.kb[lane] : 0;
    const double2 z = twid(kb, N), z2 = twid((2 * (int64_t)kb) % N, N), z3 = twid((3 * (int64_t)kb) % N, N);
    const double2 z4 = twid((4 * (int64_t)kb) % N, N);
    for (int m = w; m < nblk; m += W) {
        const int64_t s0 = a.cp + (c0 + m) * (int64_t)C;
#pragma unroll
        for (int r = 0; r < NB; ++r)
            for (int j = lane; j < C; j += 64) {
                const int64_t i = s0 + j;
                stg[r * STG + j] = i < cx.len(a) ? cx.ld(a, row0 + r, i) : make_double2(0.0, 0.0);
            }
        wave_sync();
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            double2 acc[4] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0),
                              make_double2(0.0, 0.0)};
            const double2* xs = stg + r * STG;
            for (int i = C / 4 - 1; i >= 0; --i) {
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p] = cfma(acc[p], z4, xs[4 * i + p]);
            }
            double2 v = acc[0];
            v = cfma(acc[1], z, v);
            v = cfma(acc[2], z2, v);
            v = cfma(acc[3], z3, v);
            beta[(m * NB + r) * 64 + lane] = v;
        }
        wave_sync();                                                   // staging reused
    }
}

// Phase 1 of the pair kernel: the same block DFTs, two bins per lane.  Lanes 0-31 take block m, lanes
// 32-63 block m+1, lane p the pair (k, N-k): four interleaved Goertzel resonators per branch run over
// the samples j = 4i + ch (frequency φ = 4θ, coefficient 2 cos φ, M = C/4 samples each; 4 VALU per
// sample for both bins against 4 per bin in the Horner form), and with u = w^{k(C-4)}, v = w^{kC}
//     Σ_i x[4i+ch] w^{±4ki} = u^{±1}·s_{M-1} - v^{±1}·s_{M-2},   β_{±k} = Σ_ch w^{±k ch}·(that)
// (the resonator's state grows at most ~M²·|x| at φ -> 0, so the error stays ~M²·2^-53 relative).
// Samples are staged 64 per block at a time, so the staging area is the per-bin kernel's.
template <int NB, class CX>
__device__ __forceinline__ void zs_blocks_pair(const ZsArgs& a, const CX& cx, double2* beta, double2* stg, int STG, int64_t row0,
                                               int64_t c0, int nblk, int lane, int w) {
    const int C = a.C, N = a.N, W = a.W, M = C / 4;
    const int half = lane >> 5, p = lane & 31;
    const bool valid = p < a.npairs;
    const int k = valid ? a.pk[p] : 1, sp = valid ? a.ps[p] : 0, sn = valid ? a.pn[p] : 0;
    const double c2 = 2.0 * twid((4 * (int64_t)k) % N, N).x;           // 2 cos 4θ
    const double2 u = twid(((int64_t)k * (C - 4)) % N, N), v = twid(((int64_t)k * C) % N, N);
    const double2 w1 = twid(k, N);
    for (int m0 = 2 * w; m0 < nblk; m0 += 2 * W) {
        const int m = m0 + half;
        double2 g[4][NB], h[4][NB];                                    // s_n, s_{n-1} of chain ch
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int r = 0; r < NB; ++r) { g[ch][r] = make_double2(0.0, 0.0); h[ch][r] = make_double2(0.0, 0.0); }
        for (int hb = 0; hb < C; hb += 64) {                           // 64 samples of each block
#pragma unroll
            for (int r = 0; r < NB; ++r)
                for (int j = lane; j < 128; j += 64) {
                    const int64_t i = a.cp + (c0 + m0 + (j >> 6)) * (int64_t)C + hb + (j & 63);
                    stg[r * STG + j] = i < cx.len(a) ? cx.ld(a, row0 + r, i) : make_double2(0.0, 0.0);
                }
            wave_sync();
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                const double2* xs = stg + r * STG + half * 64;
#pragma unroll 2
                for (int i = 0; i < 16; i += 2) {                      // two samples per chain: g, h swap roles
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) {
                        const double2 x0 = xs[4 * i + ch], x1 = xs[4 * i + 4 + ch];
                        h[ch][r] = make_double2(fma(c2, g[ch][r].x, x0.x - h[ch][r].x), fma(c2, g[ch][r].y, x0.y - h[ch][r].y));
                        g[ch][r] = make_double2(fma(c2, h[ch][r].x, x1.x - g[ch][r].x), fma(c2, h[ch][r].y, x1.y - g[ch][r].y));
                    }
                }
            }
            wave_sync();                                               // staging reused
        }
        if (valid && m < nblk) {
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                double2 bp = make_double2(0.0, 0.0), bn = make_double2(0.0, 0.0);
#pragma unroll
                for (int ch = 3; ch >= 0; --ch) {                      // Horner in w^{±k} over the chains
                    const double2 S = g[ch][r], S1 = h[ch][r];
                    const double2 zp = make_double2(u.x * S.x - u.y * S.y - (v.x * S1.x - v.y * S1.y),
                                                    u.x * S.y + u.y * S.x - (v.x * S1.y + v.y * S1.x));
                    const double2 zn = make_double2(u.x * S.x + u.y * S.y - (v.x * S1.x + v.y * S1.y),
                                                    u.x * S.y - u.y * S.x - (v.x * S1.y - v.y * S1.x));
                    bp = ch == 3 ? zp : cfma(bp, w1, zp);
                    bn = ch == 3 ? zn : cfma(bn, make_double2(w1.x, -w1.y), zn);
                }
                beta[(m * NB + r) * 64 + sp] = bp;
                beta[(m * NB + r) * 64 + sn] = bn;
            }
        }
    }
}

// d = x[s'+N] - x[s'] of the ZS_G steps og.. of this row's chunk into dbuf[NB][rows][ZS_G]
template <int NB, int LPC, int ROWS, class CX>
__device__ __forceinline__ void zs_stage_d(const ZsArgs& a, const CX& cx, double2* dbuf, int64_t o0, int og, bool live,
                                           int row, int sl) {
#pragma unroll
    for (int j = 0; j < ZS_G / LPC; ++j) {
        const int u = sl + LPC * j;
        const int64_t s = o0 + og + u;
        const int64_t i0 = a.cp + s;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            double2 d = make_double2(0.0, 0.0);
            if (live && s < cx.end(a) && i0 + a.N < cx.len(a)) {
                double2 p, v;
                cx.ld2(a, r, i0, a.N, p, v);
                d = make_double2(p.x - v.x, p.y - v.y);
            }
            dbuf[(r * ROWS + row) * ZS_G + u] = d;
        }
    }
}




}  // namespace

// ------------------------------------------------------------------------------------------------
// The plan of both calls.  Only C, the bins per lane, the body (pair / per bin) and the form of the
// row sums enter an output's arithmetic, and each is a function of (n_br, N, the template, the ZS_*
// variants) alone.  W and the workgroup count follow from the number of chunks a call covers; they
// decide which wave computes a block or a chunk, never what it computes.
// ------------------------------------------------------------------------------------------------
namespace {
// Row sums: deferred LDS partials for one branch, per-step DPP for two (measured, profiles/r03l_*:
// one branch 0.188 -> 0.183 ms, two branches 0.796 -> 0.840 ms); variant ZS_DEFER=0|1 forces either (A/B)
inline bool zs_defer(int n_br) {
    const int64_t v = ofs::variant(ofs::V_ZS_DEFER);
    return v != INT64_MIN ? v != 0 : n_br == 1;
}

// The pair body parks the waves' partials (ZS_RG·ZS_PS doubles = 6208 B per wave) in its block region,
// one branch's rows·W + N/C - 1 blocks of 1 KiB: where W·6208 B would reach past it into the waves'
// staging, the per-step DPP row sums serve instead.  The deferred and the DPP sums differ in the last
// bits, and a chunk call runs other W than the one-shot call, so the rule asks whether EVERY W up to
// the largest (16 waves for one branch, 8 for two) fits, and is a function of (rows, n_br, N/C) alone:
// the one-shot call and every chunk call of a stream take the same form.  8 rows (one branch): always
// (8 KiB of blocks per wave).  4 rows (two branches): from N/C >= 18 on (8·2112 B <= (N/C - 1) KiB).
constexpr bool zs_pair_defer_fits(int rows, int n_br, int nq) {
    const long wmax = n_br == 1 ? 16 : 8, per = (long)(ZS_RG * ZS_PS * sizeof(double));
    return wmax * per <= (rows * wmax + nq - 1) * (long)(64 * sizeof(double2));
}
static_assert(zs_pair_defer_fits(8, 1, 1) && !zs_pair_defer_fits(4, 2, 17) && zs_pair_defer_fits(4, 2, 18),
              "pair body: deferred row sums");

// variant ZS_PAIR=0: the per-bin kernel even for a paired template (A/B)
inline bool zs_pair_enabled() {
    return !ofs::variant_off(ofs::V_ZS_PAIR);
}

// The pair kernel's template condition: every bin pairs with its mirror N - k (neither 0 nor N/2)
// and sin(2πk/N) >= 1/2048 (the resonator's error grows as 1/sin θ).  Fills a.npairs / pk / ps / pn.
inline bool zs_pairs(ZsArgs& a) {
    const int N = a.N, n = a.nbins;
    if (n % 2 || n > 64) return false;
    bool used[64] = {};
    int np = 0;
    for (int i = 0; i < n; ++i) {
        const int k = a.kb[i];
        if (k <= 0 || 2 * k == N || k >= N) return false;
        if (2 * k > N) continue;                      // the mirror half is matched from its partner
        int j = -1;
        for (int m = 0; m < n; ++m)
            if (!used[m] && m != i && a.kb[m] == N - k) { j = m; break; }
        if (j < 0 || used[i]) return false;
        if (std::sin(2.0 * M_PI * k / N) < 1.0 / 2048) return false;
        used[i] = used[j] = true;
        a.pk[np] = k; a.ps[np] = i; a.pn[np] = j;
        ++np;
    }
    if (2 * np != n) return false;
    a.npairs = np;
    for (int p = np; p < 32; ++p) { a.pk[p] = 1; a.ps[p] = 0; a.pn[p] = 0; }
    return true;
}

// bins per lane of the slide: 8 for one branch (variant ZS_BPL=4 for the A/B), 4 for two (8 would
// exceed the 128 VGPRs of a 16-wave workgroup and spill)
inline int zs_bpl(int n_br) {
    return (n_br == 2 || ofs::variant_is(ofs::V_ZS_BPL, 4)) ? 4 : 8;
}

// chunk / block length C (C | N; 256 for N >= 8192 keeps the blocks per window at <= 32): a function
// of N and the ZS_C variant only
inline int zs_chunk_len(int N) {
    int C = (N >= 8192 && N % 256 == 0) ? 256 : (N % 128 == 0 ? 128 : 64);
    const int64_t c = ofs::variant(ofs::V_ZS_C);                       // A/B: chunk length override
    if (c >= 64 && c <= 256 && c % 64 == 0 && N % c == 0) C = (int)c;
    return C;
}

// waves per workgroup W (<= 16; 8 for two branches) for a call of nchunks chunks per stream, and the
// per-bin body's LDS; false if the blocks of a window do not fit (W = 1 is then too large as well, so
// the answer does not depend on nchunks)
inline bool zs_plan_chunks(int n_br, int N, int bpl, int C, int64_t nchunks, int& W, size_t& lds) {
    W = (int)std::min<int64_t>(n_br == 1 ? 16 : 8, (nchunks + bpl - 1) / bpl);
    const int stg = zs_stg(C, bpl);
    auto lds_of = [&](int w) { return ((size_t)(bpl * w + N / C - 1) * 64 + (size_t)w * stg) * n_br * sizeof(double2); };
    while (W > 1 && lds_of(W) > 160 * 1024) --W;
    lds = lds_of(W);
    return lds <= 160 * 1024;
}

// The rest of the plan from the template: body, block-DFT form, LDS.  a.N, a.C, a.W, a.nbins, a.kb set.
struct ZsForm { bool pair, defer; int bpl; size_t lds; };
inline ZsForm zs_form(ZsArgs& a, int n_br, size_t lds_bins) {
    ZsForm f;
    f.bpl = zs_bpl(n_br);
    a.npairs = 0;
    a.gblk = !ofs::variant_off(ofs::V_ZS_GBLK);                     // 0: Horner block DFTs in the pair kernel (A/B)
    f.pair = zs_pair_enabled() && f.bpl == (n_br == 2 ? 4 : 8) && zs_pairs(a);
    f.lds = f.pair ? zs_pair_lds(a.C, a.N, f.bpl, a.W, n_br) : lds_bins;   // pair: one branch's blocks at a time
    f.defer = zs_defer(n_br);
    if (f.pair && !zs_pair_defer_fits(f.bpl, n_br, a.N / a.C)) f.defer = false;
    if (!f.pair && n_br == 1 && f.bpl == 4) f.defer = false;           // 4 one-branch bins per lane: the block
    return f;                                                          // region may not hold the partials
}

inline void zs_template(ZsArgs& a, int nbins, const int* kb, const double* tr, const double* ti, double t_energy) {
    a.nbins = nbins; a.t_energy = t_energy;
    for (int i = 0; i < 64; ++i) {
        a.kb[i] = i < nbins ? kb[i] : 0;
        a.tr[i] = i < nbins ? tr[i] : 0.0;
        a.ti[i] = i < nbins ? ti[i] : 0.0;
    }
}

inline bool zs_shape_ok(int fmt, int n_br, int N, int nbins) {
    return (fmt == OFS_C64 || fmt == OFS_C128 || fmt == OFS_CI16) && (n_br == 1 || n_br == 2) && N >= 64 &&
           N % 64 == 0 && nbins >= 1 && nbins <= 64;
}
}  // namespace
