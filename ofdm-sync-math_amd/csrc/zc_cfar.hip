// zc_cfar.hip — zc_v2 CFAR + gate (zc_v2.py:300-346 + :374-446), fused, lane-per-stream recursion.
//
// The only sequential part of zc_streaming_detection is the reference's running sum
// (RunningSum.step, zc_v2.py:219-238): acc = (acc + c[i]) - c[i-W] in float64, left to right.
// Its rounding does not commute, so it is evaluated exactly in that order — but by ONE LANE PER
// STREAM: a workgroup owns ZS streams (16 on the LDS-DMA path), and ZS lanes of its wave 0 (the
// walker) advance the ZS recursions together, one sample per step (2 dependent v_add_f64).
// Everything else is parallel over samples and runs in the ZH helper waves of the workgroup (7 on
// the LDS-DMA path), one chunk behind the walker:
// the threshold flags (corr_scaled >= thresh_scaled, |c| >= min), the stores of every state
// array (coalesced 64-sample rows), and the gate machine in closed form.
//
// Chunks of ZC = 64·ZR samples, staged through LDS (global -> registers -> LDS, two chunks ahead):
//   c tiles (3 buffers: walker reads chunk q while the helpers read chunk q-1 and chunk q+1 lands),
//   c[i-W] tiles (2 buffers, walker only), running-sum tiles (2 buffers, walker -> helpers).
// One barrier per chunk.
//
// Gate (zc_v2.py:374-446) in closed form over the valid samples (valid = i >= W is a prefix):
// with Hp = max(H, 1) and prev(n) the last above sample < n, an open gate closes at the first
// non-above n with n - prev(n) = Hp (the low counter reaches H - 1 before it), and an above
// sample opens a gate iff it is the first one or its gap to prev exceeds Hp (the previous gate
// has closed).  For Hp >= 64 (one row) a row holds at most one close (the carried gate's, at
// prev + Hp, before any above sample of the row) and then at most one open (its first above
// sample).  The peak is the first maximum of c over [gate_start, gate_end] (strict >, the
// opening sample first); gate_mask marks (gate_start, gate_end], and [gate_start, n) for a gate
// still open at the end.  Shorter hysteresis runs the sequential kernel of corr.hip.
#include "ofs_common.h"
#include "ofdmsync.h"
#include "zc_tiles.h"

using namespace ofs;

namespace {

struct ZcArgs {
    const double* mag;
    int64_t B, n;
    int W; double tv, scale, minmag; int reflen, Hp;
    double* local_sum; double* corr_scaled; double* thresh_scaled;
    uint8_t* above; uint8_t* valid; uint8_t* gate_mask;
    int max_ev; int32_t* n_ev; int64_t* ev; double* ev_v;
};

// DMA: the walker stages the c / c[i-W] tiles with LDS-DMA (global_load_lds_dwordx4, no
// registers), two chunks ahead of use instead of one (the register path's loads land one chunk
// period after they are issued, so a chunk could not be shorter than a memory round trip);
// taken when every tile row is a whole, 16-byte-aligned 1 KiB span (host checks).
// HG: the helpers read c from global memory (L2: the walker's DMA brought the rows in) instead of the
// LDS tile: taken when state arrays are stored (paired, r06k: state mode 0.564 -> 0.540 ms;
// events + mask only 0.285 -> 0.342 ms, so not there)

#ifndef OFS_ZC_TIMING
#define OFS_ZC_TIMING 0            // diagnostic builds: per-role cycles (tools/zc_phase.py)
#endif
#if OFS_ZC_TIMING
__device__ unsigned long long zc_prof[8];
__device__ unsigned zc_hwid[4096 * 8];       // HW_ID of every wave (workgroup-major), first launch rows
#define ZC_T(i)                                                                                      \
    if (lane == 0) { const long long t_ = __builtin_amdgcn_s_memtime(); tacc[i] += t_ - tprev; tprev = t_; }
#else
#define ZC_T(i)
#endif

template <bool DMA, int ZS, int ZH, bool HG>
__global__ __launch_bounds__(64 * (1 + ZH))
void zc_cfar_kernel(ZcArgs a) {
#pragma clang fp contract(off)
#if OFS_ZC_TIMING
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tprev = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096 && threadIdx.x / 64 < 8)
        zc_hwid[blockIdx.x * 8 + threadIdx.x / 64] = __builtin_amdgcn_s_getreg(4 | (31 << 11));
#endif
    constexpr int NC = DMA ? 4 : 3, NO = DMA ? 3 : 2;
    constexpr int ZDMA_PER_CHUNK = 2 * ZS * (ZC / 128);   // DMA instructions per chunk (c and c[i-W])
    __shared__ double tc[NC][ZS][ZP];     // c
    __shared__ double to[NO][ZS][ZP];     // c[i - W] (0 before the window fills)
    __shared__ double ta[2][ZS][ZP];      // running sum after sample i
    static_assert(sizeof(tc) + sizeof(to) + sizeof(ta) <= 160 * 1024,
                  "zc_cfar_kernel: static LDS beyond gfx950's 160 KiB per workgroup (ZS / ZC / ZP)");
    const int lane = threadIdx.x & 63;
    // role of this wave: 0 = walker, 1..ZH = helpers.  (Measured and not kept: the walker chosen by
    // SIMD id so both workgroups' walkers share a SIMD, 0.38 -> 0.45 ms; an idle 8th wave as the
    // walker's SIMD partner, 0.362 -> 0.373 ms; the walker's SIMD-mates, waves 4, 8, ... of the
    // workgroup, idling at the barriers only, r05ao: bit-identical, 0.2925 vs 0.2864 ms with 9 working
    // helpers, 13 waves 0.444: SIMD sharing is not what slows the chain.)
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    constexpr int NJ = (ZS + ZH - 1) / ZH;                           // streams per helper wave
    const int hi = wv - 1;                                           // helper rank
    const int64_t b0 = (int64_t)blockIdx.x * ZS;
    const int ns = (int)min((int64_t)ZS, a.B - b0);          // streams of this workgroup
    const int64_t n = a.n;
    const int nch = (int)((n + ZC - 1) / ZC);

    // loader = the walker wave, which issues no global stores: its wait for the loads of the next
    // chunk (staged one iteration after they are issued) never drains the helpers' stores.
    // (Two register sets, loads two chunks ahead: measured slower, 0.64 vs 0.46 ms.)
    // zc_chunk_kernel has its own load / stage pair: its c[i-W] comes from the carried history ring.
    double pc[ZR][ZS], po[ZR][ZS];
    const double* cw = a.mag + b0 * n;                        // this workgroup's streams
    auto load = [&](int q) {
#pragma unroll
        for (int rr = 0; rr < ZR; ++rr) {
            const int64_t i = (int64_t)q * ZC + 64 * rr + lane;
#pragma unroll
            for (int s = 0; s < ZS; ++s) {
                const bool ok = s < ns && i < n;
                pc[rr][s] = ok ? cw[s * n + i] : 0.0;
                po[rr][s] = (ok && i >= a.W) ? cw[s * n + i - a.W] : 0.0;
            }
        }
    };
    auto stage = [&](int q) {
#pragma unroll
        for (int rr = 0; rr < ZR; ++rr)
#pragma unroll
            for (int s = 0; s < ZS; ++s) {
                tc[q % NC][s][64 * rr + lane] = pc[rr][s];
                to[q % NO][s][64 * rr + lane] = po[rr][s];
            }
    };
    // DMA path: 1 KiB per instruction (64 lanes x 16 B); rows of absent streams re-read the last
    // stream (unused); c[i-W] tiles of chunks before the window fills copy the c tile (the walker
    // uses zeros there: W is a whole number of chunks on this path)
    auto dma = [&](int q) {
#pragma unroll
        for (int s = 0; s < ZS; ++s) {
            const int ss = s < ns ? s : ns - 1;
            const double* src = cw + (int64_t)ss * n + (int64_t)q * ZC + 2 * lane;
            const double* srco = (int64_t)q * ZC >= a.W ? src - a.W : src;
#pragma unroll
            for (int j = 0; j < ZC / 128; ++j) {
                lds_dma16(src + 128 * j, &tc[q % NC][s][128 * j]);
                lds_dma16(srco + 128 * j, &to[q % NO][s][128 * j]);
            }
        }
    };

    ZcGate g[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { g[j].last_above = -1; g[j].gs = 0; g[j].pk = 0; g[j].pv = 0.0; g[j].open = 0; g[j].nev = 0; }
    double acc = 0.0;                                         // walker lane s < ns: stream b0 + s

    // LDS-only barrier (zc_tiles.h): the helpers' global stores are never waited for
    auto lds_barrier = [] {
        if constexpr (DMA) {
            // no memory-model fence here: with LDS-DMA in the kernel the compiler implements a
            // "local" release fence as vmcnt(0), which would drain the DMAs in flight (and the
            // helpers' stores) every chunk.  This wave's LDS accesses complete at lgkmcnt(0); the
            // DMA'd tiles a chunk reads were waited for by the walker before the barrier.
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        } else {
            zc_lds_barrier();
        }
    };
    if (wv == 0) {
        if constexpr (DMA) {
            dma(0);
            if (1 < nch) dma(1);
        } else {
            load(0);
            stage(0);
            if (1 < nch) load(1);
        }
    }
    lds_barrier();
    for (int q = 0; q <= nch; ++q) {
        if (wv == 0) {
            if constexpr (DMA) {
                if (q + 2 < nch) dma(q + 2);
                // chunk q has landed once at most the (up to two) later chunks' DMAs are in flight
                // (loads complete in order, so "at most min(63, later x per-chunk) outstanding"
                // implies chunk q has landed; 63 = the vmcnt field's maximum)
                constexpr int V2 = 2 * ZDMA_PER_CHUNK < 63 ? 2 * ZDMA_PER_CHUNK : 63;
                constexpr int V1 = ZDMA_PER_CHUNK < 63 ? ZDMA_PER_CHUNK : 63;
                const int later = min(2, nch - 1 - q);
                if (later >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(V2) : "memory");
                else if (later == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(V1) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                ZC_T(0)
            } else {
                if (q + 1 < nch) stage(q + 1);                // loaded during the previous chunk
                if (q + 2 < nch) load(q + 2);
            }
        }
        if (wv == 0) {
            // ---- walker: the exact left-to-right recursion of RunningSum.step ----
            if (q < nch && lane < ZS) {
                const int cnt = (int)min((int64_t)ZC, n - (int64_t)q * ZC);
                const double* x = tc[q % NC][lane];
                const double* o = to[q % NO][lane];
                const bool ozero = DMA && (int64_t)q * ZC < a.W;      // DMA path: before the window fills
                double* r = ta[q & 1][lane];
                if (cnt == ZC) {
                    // ozero is uniform per chunk: a chain without the c[i-W] reads and selects
                    // (x - 0.0 == x exactly, -0.0 included) instead of two v_cndmask per sample
                    if (ozero) zc_walk_chunk<ZC, true>(x, o, r, acc);
                    else zc_walk_chunk<ZC, false>(x, o, r, acc);
                } else {
                    for (int u = 0; u < cnt; ++u) { acc = (acc + x[u]) - (ozero ? 0.0 : o[u]); r[u] = acc; }
                }
            }
            ZC_T(1)
        } else if (q >= 1) {
            // ---- helpers: chunk q-1 (flags, stores, gate) ----
            const int qc = q - 1;
            // pass 1: the flags of every (row, stream) of this wave.  A chunk with no
            // above sample and no open gate (the common case: events are sparse) needs no gate
            // logic - its gate_mask rows are 0 - so the wave skips the scalar gate machine.
            bool quiet = true;
            double cv[ZR][NJ], lv[ZR][NJ];
            uint64_t am[ZR][NJ];
            // every LDS read of the chunk first (one latency for all of them, not one per row),
            // then the flags with non-short-circuit logic (no exec-mask branches per term).
            // zc_chunk_kernel has these loops too (rotated tile slots, valid from the stream's own
            // count); the decision itself, zc_above, is shared.  The ballots and the quiet decision
            // as one template function with the valid test as a lambda: 3999 -> 4001, 3886 -> 3891,
            // 4981 -> 4985 instructions here, 8572 -> 8573 there, so both stay written out.
#pragma unroll
            for (int rr = 0; rr < ZR; ++rr)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int s = hi + ZH * j;
                    const int sr = s < ns ? s : 0;
                    if constexpr (HG) {
                        const int64_t ig = (int64_t)qc * ZC + 64 * rr + lane;
                        cv[rr][j] = ig < n ? cw[(int64_t)sr * n + ig] : 0.0;
                    } else {
                        cv[rr][j] = tc[qc % NC][sr][64 * rr + lane];
                    }
                    lv[rr][j] = ta[qc & 1][sr][64 * rr + lane];
                }
#pragma unroll
            for (int rr = 0; rr < ZR; ++rr) {
                const int64_t i = (int64_t)qc * ZC + 64 * rr + lane;
                const bool vd = (i < n) & (i >= a.W);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int s = hi + ZH * j;
                    am[rr][j] = zc_above(a, (s < ns) & vd, cv[rr][j], lv[rr][j]);
                    if (am[rr][j]) quiet = false;
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (g[j].open) quiet = false;
#pragma unroll
            for (int rr = 0; rr < ZR; ++rr) {
            const int64_t base = (int64_t)qc * ZC + 64 * rr;
            const int64_t i = base + lane;
            const bool inb = i < n;
            const bool vd = inb && i >= a.W;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int s = hi + ZH * j;
                if (s >= ns) break;
                const double c = cv[rr][j];
                const double ls = lv[rr][j];
                const double cs = c * a.scale, th = ls * a.tv;
                const uint64_t abm = am[rr][j];
                const bool ab = (abm >> lane) & 1;
                const int64_t o = (b0 + s) * n + i;
                if (quiet) {
                    if (inb) zc_store(a, o, ls, cs, th, 0, vd, 0);
                    continue;
                }
                ZcGate& G = g[j];
                // gate in closed form (Hp >= 64): carried close first, then this row's first above
                int close_l = -1;                                     // row lane of the close
                if (G.open) {
                    const int64_t nc = G.last_above + a.Hp;
                    const int64_t fa = abm ? base + __builtin_ctzll(abm) : INT64_MAX;
                    if (nc >= base && nc < base + 64 && nc < n && fa > nc) close_l = (int)(nc - base);
                }
                const int open_l = abm ? __builtin_ctzll(abm) : -1;
                const bool carried = G.open != 0;
                const bool opens = open_l >= 0 && (!carried || close_l >= 0);   // Hp >= 64: open after close
                // gate_mask: carried gate over [0, close] (or the whole row), new gate over (open, 63]
                const int cend = carried ? (close_l >= 0 ? close_l : 63) : -1;
                const bool mk = inb && ((lane <= cend) || (opens && lane > open_l));
                if (carried) {                                       // peak over [0, cend]
                    zc_peak(G, inb && lane <= cend, c, base);
                    if (close_l >= 0) {
                        ZC_EVENT(a, G, b0 + s, base + close_l, lane);
                        G.open = 0; G.pv = 0.0;
                    }
                }
                if (opens) {                                         // opening sample, then (open, 63]
                    G.open = 1; G.gs = base + open_l; G.pk = G.gs;
                    G.pv = readlane(c, open_l);
                    zc_peak(G, inb && lane > open_l, c, base);
                }
                if (abm) G.last_above = base + 63 - __builtin_clzll(abm);
                if (inb) zc_store(a, o, ls, cs, th, ab, vd, mk);
            }
            }
            ZC_T(3)
        }
        lds_barrier();
        if (wv == 0) { ZC_T(2) } else { ZC_T(4) }
    }
    // ---- gates still open at the end: gate_end = n, gate_mask[gate_start:n] ----
    if (wv >= 1) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int s = hi + ZH * j;
            if (s >= ns) break;
            ZcGate& G = g[j];
            if (G.open) {
                ZC_EVENT(a, G, b0 + s, n, lane);
                if (lane == 0 && a.gate_mask) a.gate_mask[(b0 + s) * n + G.gs] = 1;
            }
            if (lane == 0 && a.n_ev) a.n_ev[b0 + s] = G.nev;
        }
    }
#if OFS_ZC_TIMING
    if (lane == 0)
        for (int i = 0; i < 5; ++i) atomicAdd(&zc_prof[i], (unsigned long long)tacc[i]);
#endif
}

}  // namespace

// the one dispatch decision of the zc_v2 CFAR + gate (W: the running-sum window, max(1, window_size)):
// 0 the sequential kernel of corr.hip, 1 the fused kernel with register-staged tiles, 2 with LDS-DMA
// tiles storing events and gate mask only, 3 with LDS-DMA tiles and the state arrays.  Both the
// launch below and the query ofs_zc_detect_plan go through it.
int ofs_zc_cfar_plan(int64_t n, int W, int hyst, bool state, bool aligned16) {
    const int Hp = hyst > 1 ? hyst : 1;
    if (Hp < 64 || n <= 0 || ofs::variant_on(ofs::V_ZC_SEQ)) return 0;
    const bool dma = ZC % 128 == 0 && n % ZC == 0 && W % ZC == 0 && W >= 0 && aligned16 &&
                     !ofs::variant_on(ofs::V_ZC_NODMA);
    return !dma ? 1 : state ? 3 : 2;
}

// fused CFAR + gate for hysteresis >= one chunk; returns 0 when the shape is not covered
int ofs_zc_cfar_try(const double* corr_mag, int64_t B, int64_t n, int W, double tv, double scale,
                    double minmag, int reflen, int hyst, double* local_sum, double* corr_scaled,
                    double* thresh_scaled, uint8_t* above, uint8_t* valid, uint8_t* gate_mask, int max_ev,
                    int32_t* n_ev, int64_t* ev, double* ev_v, hipStream_t st) {
    const int Hp = hyst > 1 ? hyst : 1;
    const bool state = local_sum || corr_scaled || thresh_scaled;
    const int plan = B > 0 ? ofs_zc_cfar_plan(n, W, hyst, state, (reinterpret_cast<uintptr_t>(corr_mag) & 15) == 0) : 0;
    if (plan == 0) return 0;
    ZcArgs a{corr_mag, B, n, W, tv, scale, minmag, reflen, Hp, local_sum, corr_scaled, thresh_scaled,
             above, valid, gate_mask, max_ev, n_ev, ev, ev_v};
    constexpr int SD = ZS_DMA, HD = ZH_DMA, SR = ZS_REG, HR = ZH_REG;
    const dim3 gd((unsigned)((B + SD - 1) / SD)), gr((unsigned)((B + SR - 1) / SR));
    if (plan == 3) hipLaunchKernelGGL((zc_cfar_kernel<true, SD, HD, true>), gd, dim3(64 * (1 + HD)), 0, st, a);
    else if (plan == 2) hipLaunchKernelGGL((zc_cfar_kernel<true, SD, HD, false>), gd, dim3(64 * (1 + HD)), 0, st, a);
    else hipLaunchKernelGGL((zc_cfar_kernel<false, SR, HR, false>), gr, dim3(64 * (1 + HR)), 0, st, a);
    return hipGetLastError() == hipSuccess ? 1 : OFS_EHIP;
}

#if OFS_ZC_TIMING
// per-role cycle totals of zc_cfar_kernel since the last call (diagnostic builds): walker DMA wait,
// walker chain, walker barrier, helper work, helper barrier
extern "C" int ofs_zc_prof(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(zc_prof), 5 * sizeof(unsigned long long)) != hipSuccess) return -1;
    const unsigned long long z[8] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(zc_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
extern "C" int ofs_zc_hwid(unsigned* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(zc_hwid), 4096 * 8 * sizeof(unsigned)) == hipSuccess ? 0 : -1;
}
#endif
