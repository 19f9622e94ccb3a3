// aa_fast.hip — register-resident fast path of the [A][A] S&C detector (sync_aa.py:421-571).
//
// One wave64 per receive stream, no LDS, no barriers.  Row k of a stream holds RL = 64·E
// samples; lane l owns the E consecutive samples n = RL·k + E·l + e.  With L = MR·RL the
// delayed sample x[n-L] sits in the SAME lane and element MR rows back, so the lagged
// product x[n]·conj(x[n-L]) needs no data movement.
//
// Window sums without cancellation: for n in row k (k >= MR)
//     P[n] = suf_{k-MR}(e') + sum_{j=k-MR+1}^{k-1} tot_j + pre_k(e')
// where pre_k is the in-row inclusive prefix (fp64: lane-serial + DPP wave scan), tot_j the
// row totals (fp64, wave-uniform) and suf_{k-MR} the part of row k-MR after position n —
// computed in fp64 when that row was processed and retained in fp32 registers.  Every piece
// sums only in-window terms, so fp32 storage error is relative to the window, not to the
// stream or a loud burst next to a quiet window.  Each row is processed in two passes:
// (1) lane totals -> wave scan; (2) products recomputed while outputs stream out, which keeps
// the register footprint at ~3L/64 retained floats per lane.
//
// Gate / peak / CFO events (sync_aa.py:495-568) use the closed form of aa_events
// (ofdmsync.hip), streamed row by row (aa_gate.h): prev-above by lane-serial + DPP max-scan,
// opens/closes by ballot, per-gate argmax by wave reductions, scalar carry between rows.
#include <cfloat>
#include <cmath>
#include "ofs_common.h"
#include "aa_gate.h"
#include "ofdmsync.h"

using namespace ofs;

namespace {

constexpr int FAST_WG = 64;       // one wave = one stream per workgroup (paired A/B: 2-6 % faster than 256)
constexpr int TMAX = 1024;        // stream length handled by the fast path
constexpr int FAST_CAP_LDS = 160 * 1024 / 10;   // occupancy cap of the storing kernel: 10 workgroups per CU (launch)
// its full-stream form: 7 per CU (the measured value; at most 160 KiB / 7 = 23405, less the allocation granule)
constexpr int FAST_CAP_LDS_FULL = 23000;

typedef float nf4 __attribute__((ext_vector_type(4)));
typedef float nf2 __attribute__((ext_vector_type(2)));
// complex values as packed fp32 pairs (re, im): products, in-lane partials and window sums issue
// as v_pk_fma / v_pk_add (half the VALU of the scalar form)
typedef float pf2 __attribute__((ext_vector_type(2)));
// acc + c·conj(d) = acc + (c.x d.x + c.y d.y, c.y d.x - c.x d.y)
__device__ __forceinline__ pf2 mulc_acc(pf2 c, pf2 d, pf2 acc) {
    acc = __builtin_elementwise_fma(c, d.xx, acc);
    return __builtin_elementwise_fma(c.yx, pf2{d.y, -d.y}, acc);
}
// Output stores of the storing kernel (P, R, M; event stores stay plain).  SP = cache policy of the
// store: 0 plain, 1 non-temporal (variant FAST_ST_POLICY; the default of the headline kernel, launch()).
template <int SP>
__device__ __forceinline__ void st_out(float4* p, float4 v) {
    const nf4 d = nf4{v.x, v.y, v.z, v.w};
    if constexpr (SP == 1) __builtin_nontemporal_store(d, reinterpret_cast<nf4*>(p));
    else *p = v;
}
template <int SP>
__device__ __forceinline__ void st_out(float2* p, float2 v) {
    const nf2 d = nf2{v.x, v.y};
    if constexpr (SP == 1) __builtin_nontemporal_store(d, reinterpret_cast<nf2*>(p));
    else *p = v;
}

// Input loads of the full-stream form: 16 bytes at p.  LP = cache policy (variant FAST_LD_POLICY): 0 plain,
// 1 non-temporal (the default, launch(): x is read exactly once).  Both are loads whose returns the compiler
// counts itself (the per-row vmcnt waits depend on it).
template <int LP>
__device__ __forceinline__ float4 ld_x(const char* p) {
    if constexpr (LP == 1) {
        const nf4 v = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return *reinterpret_cast<const float4*>(p);
    }
}

// Row-paired R / M store (E = 2): rows k, k+1 of one stream are 256 consecutive floats (1 KiB) of the
// buffer.  Lane l holds (a[0], a[1]) = floats 2l, 2l+1 of row k and (b[0], b[1]) of row k+1; it stores
// floats [4l, 4l+4) of the span - the values of lanes 2(l & 31), 2(l & 31) + 1 of row k + (l >= 32) -
// as one float4, so the wave instruction writes one contiguous 1 KiB span in lane order.  The move:
// a quad-perm DPP packs what the even (odd) source lanes hand over into one register - even lanes
// keep row k's value, odd lanes take row k+1's from the lane below (above) - then one ds_bpermute per
// output dword with the same index for all four.  No LDS allocation, no barrier; all 64 lanes active.
template <int SP>
__device__ __forceinline__ void st_rows2(float* span, const float (&a)[2], const float (&b)[2], int lane) {
    const bool odd = (lane & 1) != 0;
    const int idx = (lane < 32 ? 2 * lane : 2 * lane - 63) * 4;
    float o[4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int ai = __float_as_int(a[e]), bi = __float_as_int(b[e]);
        // the DPP moves run with every lane active (before the selects, not inside a ?: arm)
        const int bdn = dpp_i<0xA0>(bi);                        // quad_perm:[0,0,2,2]: lane 2i+1 <- b of lane 2i
        const int aup = dpp_i<0xF5>(ai);                        // quad_perm:[1,1,3,3]: lane 2i <- a of lane 2i+1
        const int we = odd ? bdn : ai;
        const int wo = odd ? bi : aup;
        o[e] = __int_as_float(__builtin_amdgcn_ds_bpermute(idx, we));
        o[2 + e] = __int_as_float(__builtin_amdgcn_ds_bpermute(idx, wo));
    }
    st_out<SP>(reinterpret_cast<float4*>(span) + lane, make_float4(o[0], o[1], o[2], o[3]));
}


// Stream staging: every row of the lane's samples is loaded into registers up front and each row's
// first use waits only for its own loads.  Staging through a wave-private LDS slice (LDS-DMA) measured
// 1-3 % slower (profiles/r01c_staging_ab.log, r02av_staging_ab.jsonl), and pinning the loads to reach
// more waves per SIMD is slower too: the kernel is not latency-starved at 3 waves/SIMD
// (profiles/r06b_headline_pinned_loads_waves_ab.jsonl).  The gate machine runs per row: run after the
// row loop it was neutral on the headline and 5 % slower detect-only
// (profiles/r05_headline_gate_breakdown.txt).
//
// DO: detect-only instantiation (P/R/M/valid not stored, events only: SURVEY §8d); S32: fp32
// row scans (ofs_common.h row_scan; the detect-only default, issue-bound there); SV: store path of
// the one-antenna E = 2 storing kernel = 2 * (row-paired R/M stores) + (non-temporal stores, st_out)
//
// FS: full-stream form of the SV = 3 kernel (launch(): T == TMAX, P, R, M and the event outputs all
// present, no valid, detect on; variant FAST_FULL = 0 keeps the generic form).  Same arithmetic and data
// movement, same bits; what goes is the generality around them: T is a constant (no row guards, no
// zero-fill selects, no clamped load index, every R/M row pair goes out paired), no pointer is tested,
// each buffer is one scalar base per stream plus one 32-bit lane offset (16 * lane bytes for x, P and
// the paired R/M spans alike; the row offset is a constant), the above flags are an fp32 compare against
// AaFastArgs::thr32, and the gate machine is chosen at launch: FS = 1 the scan-free rows (max(hyst, 1)
// >= RL), FS = 2 the scan rows - not both bodies inline behind a per-row test.
// LP: cache policy of the full-stream form's input loads (ld_x)
template <int E, int MR, int NA, bool DO, bool S32, int SV = 0, int FS = 0, int LP = 0>
__global__ __launch_bounds__(FAST_WG) void aa_fast_kernel(AaFastArgs a) {
    static_assert(SV == 0 || (E == 2 && NA == 1 && !DO), "store-path variants: one-antenna E = 2 storing kernel");
    static_assert(FS == 0 || (SV == 3 && !S32), "full-stream form: the headline's kernel");
    static_assert(LP == 0 || FS != 0, "load-policy arms: the full-stream form");
    constexpr bool FULL = FS != 0;
    constexpr int SP = SV & 1;                 // output store cache policy
    constexpr bool RP = (SV & 2) != 0;         // R/M of rows k, k+1 (k even) as one 16-byte store per lane
    constexpr int RL = 64 * E;                 // samples per row
    constexpr int RW = TMAX / RL;              // rows per stream
    constexpr int L = MR * RL;
    constexpr int V4 = E / 2;                  // float4 (2 samples) per lane per row
    static_assert(MR >= 1 && MR <= RW, "window must fit the stream tile");
    const int lane = threadIdx.x & 63;
    // the wave index is 0 (one wave per workgroup), but the compiler does not know it: the term keeps the
    // stream index of the generic form in a VGPR.  Without it the index is wave-uniform, all 142
    // instantiations compile differently and detect-only measured 1-2 % slower (0.0943-0.0949 against
    // 0.0930-0.0936 ms, profiles/aa_fast_rowsums_candidates.txt)
    const int w = FULL ? 0 : threadIdx.x >> 6;
    // block order: one antenna plain blockIdx, two the XCD remap (paired under the occupancy cap,
    // profiles/r06n_headline_remap_ff_ab.txt: without the remap cfg3 0.2994 -> 0.2940 ms, detect-only
    // 0.1036 -> 0.0949, T 4096 1.225 -> 1.211; two antennas 0.4004 -> 0.4055 and the 2 x 5315 shape
    // slower in 2 of 3 rounds - they keep it)
    const int64_t b = (int64_t)(NA == 1 ? blockIdx.x : xcd_block()) + w;
    if (b >= a.B) return;
    const int T = FULL ? TMAX : (int)a.T;
    // FULL: byte offset of this lane's 16 bytes in a row of x / P and in a row pair of R / M
    const uint32_t lo16 = 16u * (uint32_t)lane;
    // register staging: every row of the lane's samples is loaded up front (RW * V4 float4), each
    // row's first use waits only for its own loads (vmcnt counts in order)
    float4 xreg[NA][RW][V4];
    if constexpr (FULL) {
        const char* const xb = reinterpret_cast<const char*>(a.x) + b * (TMAX * 8);
#pragma unroll
        for (int k = 0; k < RW; ++k) xreg[0][k][0] = ld_x<LP>(xb + RL * 8 * k + lo16);
    } else {
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            const float2* xs = reinterpret_cast<const float2*>(a.x) + (b * NA + t) * a.T;
#pragma unroll
            for (int k = 0; k < RW; ++k)
#pragma unroll
                for (int j = 0; j < V4; ++j) {
                    int n = RL * k + E * lane + 2 * j;
                    n = n < T ? n : T - 2;                      // in-bounds; zeroed on read
                    xreg[t][k][j] = *reinterpret_cast<const float4*>(xs + n);
                }
        }
    }
    auto xrow = [&](int t, int k, pf2 (&c)[E]) {
#pragma unroll
        for (int j = 0; j < V4; ++j) {
            const bool ok = FULL || RL * k + E * lane + 2 * j < T;
            const float4 v = xreg[t][k][j];
            c[2 * j] = ok ? pf2{v.x, v.y} : pf2{0.f, 0.f};
            c[2 * j + 1] = ok ? pf2{v.z, v.w} : pf2{0.f, 0.f};
        }
    };

    pf2 sS[MR][E];                              // retained in-window suffixes (ring by k % MR)
    float sE[MR][E];
    double Cr[RW + 1], Ci[RW + 1], Ce[RW + 1];  // running row bases (wave-uniform)
    Cr[0] = Ci[0] = Ce[0] = 0.0;

    // scan-free gate flags: detect-only, and the one-antenna storing kernel (round 6, under the occupancy
    // cap: 0.2905 -> 0.2889 ms, 0.2979 -> 0.2966 with the remap; r06m / r06n)
    AaRowGate<E, float, false, (bool)(DO || NA == 1)> gate;   // event state (wave-uniform)
    const bool detect = FULL || a.detect;
    if (detect)
        gate.init(a.hyst, L, a.thr, a.fs, a.max_ev, a.ev_i + b * (int64_t)a.max_ev * 4,
                  a.ev_r + b * (int64_t)a.max_ev * 4);

    float* Pout = DO ? nullptr : reinterpret_cast<float*>(a.P);
    float* Rout = DO ? nullptr : reinterpret_cast<float*>(a.R);
    float* Mout = DO ? nullptr : reinterpret_cast<float*>(a.M);
    const float floor_ = 1e-6f * (float)L;
    float hR[2] = {0.f, 0.f}, hM[2] = {0.f, 0.f};   // RP: R, M of the even row, held for one row
    // resident head (OFS_AA_HEAD_RESIDENT): P[n], M[n] of n < L are +0.0 for any input (no lagged product,
    // m = 0) and the caller's buffers already hold them, so rows k < MR store R alone (wave-uniform)
    const bool head = !DO && a.head_resident != 0;
    // FULL: this stream's outputs, one scalar base each
    char* const Pb = FULL ? reinterpret_cast<char*>(a.P) + b * (TMAX * 8) : nullptr;
    float* const Rb = FULL ? reinterpret_cast<float*>(a.R) + b * TMAX : nullptr;
    float* const Mb = FULL ? reinterpret_cast<float*>(a.M) + b * TMAX : nullptr;

#pragma unroll
    for (int k = 0; k < RW; ++k) {
        if (FULL || RL * k < T) {                               // wave-uniform row guard
            const int nb = RL * k + E * lane;                   // first sample of this lane
            // ---- lagged products x[n]·conj(x[n-L]) and energies, fp32 ----
            // summed over the antennas, like the reference's per-antenna running sums added up
            // (sync_aa.py:463-480)
            pf2 av[E];
            float aE[E];
#pragma unroll
            for (int e = 0; e < E; ++e) { av[e] = pf2{0.f, 0.f}; aE[e] = 0.f; }
#pragma unroll
            for (int t = 0; t < NA; ++t) {
                pf2 c[E];
                xrow(t, k, c);
#pragma unroll
                for (int e = 0; e < E; ++e) aE[e] += fmaf(c[e].x, c[e].x, c[e].y * c[e].y);
                if (k >= MR) {
                    pf2 d[E];
                    xrow(t, k - MR, d);
#pragma unroll
                    for (int e = 0; e < E; ++e) av[e] = mulc_acc(c[e], d[e], av[e]);
                }
            }
            // ---- in-lane partials, each summing only the terms it stands for:
            //      forward f[e] = sum_{e'<=e} a[e'], backward g[e] = sum_{e'>e} a[e'] ----
            pf2 fS[E], gS[E];
            float fE[E], gE[E];
            fS[0] = av[0]; fE[0] = aE[0];
#pragma unroll
            for (int e = 1; e < E; ++e) { fS[e] = fS[e - 1] + av[e]; fE[e] = fE[e - 1] + aE[e]; }
            gS[E - 1] = pf2{0.f, 0.f}; gE[E - 1] = 0.f;
#pragma unroll
            for (int e = E - 2; e >= 0; --e) { gS[e] = gS[e + 1] + av[e + 1]; gE[e] = gE[e + 1] + aE[e + 1]; }
            // ---- lane totals: fp64 DPP wave scan, row totals, rows inside the window ----
            // rows k < MR have no lagged product: their lane totals, and so every part of the P scans,
            // are +0.0 - only the energy is scanned there (the same bits: a scan of zeros gives +0.0)
            const RowScan sEr = row_scan<S32>(fE[E - 1]);
            RowScan sRr{0.f, 0.f, 0.0}, sIr{0.f, 0.f, 0.0};
            if (k >= MR) { sRr = row_scan<S32>(fS[E - 1].x); sIr = row_scan<S32>(fS[E - 1].y); }
            const double totR = sRr.tot, totI = sIr.tot, totE = sEr.tot;
            const pf2 xS = pf2{sRr.x, sIr.x};                        // lanes < l
            const float xE = sEr.x;
            const pf2 uS = pf2{sRr.u, sIr.u};                        // lanes > l
            const float uE = sEr.u;
            Cr[k + 1] = Cr[k] + totR; Ci[k + 1] = Ci[k] + totI; Ce[k + 1] = Ce[k] + totE;
            const pf2 wS = pf2{(float)((k >= MR) ? (Cr[k] - Cr[k - MR + 1]) : Cr[k]),
                               (float)((k >= MR) ? (Ci[k] - Ci[k - MR + 1]) : Ci[k])};
            const float wE = (float)((k >= MR) ? (Ce[k] - Ce[k - MR + 1]) : Ce[k]);

            // ---- window sums  P = suffix(row k-MR) + rows between + prefix(row k) ----
            float pf[E][2], mf[E], pmf[E], rf[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                pf2 P = wS + (xS + fS[e]);
                float RR = wE + (xE + fE[e]);
                if (k >= MR) { P += sS[k % MR][e]; RR += sE[k % MR][e]; }
                sS[k % MR][e] = uS + gS[e]; sE[k % MR][e] = uE + gE[e];
                const float pm = fmaf(P.x, P.x, P.y * P.y);
                float m = 0.f;
                if (k >= MR && RR > floor_) m = fminf(pm * __builtin_amdgcn_rcpf(RR * RR), 1.f);
                pf[e][0] = P.x; pf[e][1] = P.y; rf[e] = RR; mf[e] = m; pmf[e] = pm;
            }

            if constexpr (FULL) {
                // every row whole, every pair paired; rows k < MR of a resident head store R alone
                const bool pm_row = !(k < MR && head);
                if (pm_row) st_out<SP>(reinterpret_cast<float4*>(Pb + RL * 8 * k + lo16), make_float4(pf[0][0], pf[0][1], pf[1][0], pf[1][1]));
                if ((k & 1) == 0) {
                    hR[0] = rf[0]; hR[1] = rf[1]; hM[0] = mf[0]; hM[1] = mf[1];
                } else {
                    st_rows2<SP>(Rb + RL * (k - 1), hR, rf, lane);
                    if (pm_row) st_rows2<SP>(Mb + RL * (k - 1), hM, mf, lane);
                }
            } else {
            const int64_t o = b * a.T + nb;
            float* const Pk = (k < MR && head) ? nullptr : Pout;   // this row's P / M stores (none: resident head)
            float* const Mk = (k < MR && head) ? nullptr : Mout;
            // row-paired R/M stores (st_rows2): rows k0 = k & ~1 and k0 + 1 go out together from the odd
            // row when both lie entirely inside the stream and T % 4 == 0 (the span b*T + RL*k0 is then
            // 16-byte aligned and ends inside the stream); every other row stores its own float2
            // (wave-uniform choice)
            const bool paired = RP && (T & 3) == 0 && RL * ((k & ~1) + 2) <= T;
#pragma unroll
            for (int j = 0; j < V4; ++j) {
                if (nb + 2 * j < T) {
                    if (Pk) st_out<SP>(reinterpret_cast<float4*>(Pk + 2 * (o + 2 * j)),
                                         make_float4(pf[2 * j][0], pf[2 * j][1], pf[2 * j + 1][0], pf[2 * j + 1][1]));
                    // float4 R/M stores need T % 4 == 0: otherwise the last pair of a stream
                    // would spill into the next stream's first samples (and b*T+nb is not
                    // 16-byte aligned for odd b)
                    if (paired) {                               // R/M of this row: st_rows2 below
                    } else if (E % 4 != 0 || (T & 3) != 0) {
                        if (Rout) st_out<SP>(reinterpret_cast<float2*>(Rout + o + 2 * j), make_float2(rf[2 * j], rf[2 * j + 1]));
                        if (Mk) st_out<SP>(reinterpret_cast<float2*>(Mk + o + 2 * j), make_float2(mf[2 * j], mf[2 * j + 1]));
                    } else if ((j & 1) == 0) {
                        if (Rout) st_out<SP>(reinterpret_cast<float4*>(Rout + o + 2 * j),
                                             make_float4(rf[2 * j], rf[2 * j + 1], rf[2 * j + 2], rf[2 * j + 3]));
                        if (Mk) st_out<SP>(reinterpret_cast<float4*>(Mk + o + 2 * j),
                                             make_float4(mf[2 * j], mf[2 * j + 1], mf[2 * j + 2], mf[2 * j + 3]));
                    }
                    if (!DO && a.valid) { a.valid[o + 2 * j] = (k >= MR); a.valid[o + 2 * j + 1] = (k >= MR); }
                }
            }
            if constexpr (RP) {
                if (paired) {
                    if ((k & 1) == 0) {
                        hR[0] = rf[0]; hR[1] = rf[1]; hM[0] = mf[0]; hM[1] = mf[1];
                    } else {
                        const int64_t o0 = b * a.T + RL * (k - 1);
                        if (Rout) st_rows2<SP>(Rout + o0, hR, rf, lane);
                        // a pair inside the head (k < MR) is not written; one that straddles L (odd MR)
                        // goes out whole, the head row's zeros included
                        if (Mk) st_rows2<SP>(Mk + o0, hM, mf, lane);
                    }
                }
            }
            }

            // ---- events: closed-form gate machine, streamed per row (aa_gate.h) ----
            if (detect && k >= MR) {
                float pr[E], pi[E];
#pragma unroll
                for (int e = 0; e < E; ++e) { pr[e] = pf[e][0]; pi[e] = pf[e][1]; }
                if constexpr (FULL) {
                    // m >= thr32 in fp32 is (double)m >= thr for every m and thr (launch())
                    bool ab[E];
#pragma unroll
                    for (int e = 0; e < E; ++e) ab[e] = mf[e] >= a.thr32;
                    gate.template row_flags<FS, true>(lane, k, nb, T, ab, pmf, pr, pi, mf);
                } else {
                    gate.row(lane, k, nb, T, mf, pmf, pr, pi);
                }
            }
        }
    }
    if (detect) gate.finish(lane, T, a.n_ev + b);
}

// ------------------------------------------------------------------------------------------
// Streaming variant for ANY stream length (T > 1024 or odd T: the reference's own detector
// input, sync_aa.run_single_test, is ~4.2-5.3k samples x 2 antennas, sync_aa.py:699-738).
// Same row layout, window split and gate machine as aa_fast_kernel; instead of holding the
// whole stream in registers, rows stream from HBM PD rows ahead of use and only what the
// window needs is retained: the raw samples of rows k-MR..k-1 (lag L = MR rows), the fp32
// in-window suffixes of those rows and the fp64 row bases C[k-MR+1..k] (register rings
// indexed by k mod MR, resolved at compile time by unrolling the row loop by the ring period).
// Odd T: the stream base is only 8-byte aligned, so pair loads/stores use 8-byte-aligned
// vector types (gfx950 global memory ops need dword alignment only) and the last, partial row
// falls back to per-sample accesses.
// ------------------------------------------------------------------------------------------
typedef float f4u __attribute__((ext_vector_type(4), aligned(8)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));

// workgroup size of the streaming kernel: the one-antenna storing kernel runs 2 streams per workgroup
// (round 6, paired, profiles/r06v_stream_kernel_variants_ab.txt: T 4096 1.222 -> 1.192 ms); two
// antennas (the 2 x 5315 reference shape: 0.578 vs 0.608 ms) and detect-only keep one
constexpr int stream_wg(int na, bool det_only) { return (na == 1 && !det_only) ? 128 : 64; }

// per-wave state of the streaming kernel; row<U, FIRST, GUARD>() processes row k whose ring
// position k mod PER == U is a compile-time constant: FIRST = rows k < MR (no lagged product,
// window clipped at 0), GUARD = a row that may reach past T (partial row / tail)
template <int E, int MR, int NA, bool DO>
struct AaStream {
    static constexpr int RL = 64 * E;
    static constexpr int L = MR * RL;
    static constexpr int V4 = E / 2;                         // sample pairs per lane per row
    // rows in flight ahead of use (paired A/B, tools/lib_ab.py, r02e: 1 antenna PD 2, 2 antennas
    // with the LDS lag ring PD 4; the peeled steady loop + scan-free gate flags + these took the
    // T = 4096 shape 1.32 -> 1.09 ms and the 2 x 5315 reference shape 0.75 -> 0.49 ms)
    static constexpr int PD = (E == 2 && NA == 2) ? 4 : 2;
    static constexpr int PER = MR > PD ? MR : PD;            // unroll period (MR, PD powers of 2)
    // lag ring (raw samples of rows k-MR..k-1) in a wave-private LDS slice instead of VGPRs: two
    // antennas (frees 32 VGPRs there)
    static constexpr bool LDSLAG = NA == 2;

    const float2* xb;
    float4 (*lag)[NA][V4][64];                               // LDSLAG: [MR][NA][V4][lane]
    int64_t T, o0;
    int Ti, nrows, full_rows, lane;
    pf2 lx[LDSLAG ? 1 : NA][MR][E];                          // x of rows k-MR..k-1 (lag L)
    pf2 sS[MR][E];                                           // retained in-window suffixes
    float sE[MR][E];
    double cbR[MR], cbI[MR], cbE[MR];                        // row bases C[j], j in (k-MR, k]
    double CR, CI, CE;                                       // C[k]: prefix at the start of row k
    float2 nx[PD][NA][E];                                    // rows k..k+PD-1 in flight
    AaRowGate<E, float, false, true> gate;
    float2* Pout; float* Rout; float* Mout; uint8_t* Vout;
    bool detect, head;                                       // head: P, M of n < L resident (not stored)
    float floor_;

    // a row's samples of every antenna: 8-byte-aligned pair loads for whole rows, per-sample
    // with zero fill past T otherwise (wave-uniform choice)
    __device__ __forceinline__ void load_row(int k, float2 (&dst)[NA][E]) {
        const int64_t n0 = (int64_t)RL * k + E * lane;
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            const float2* xs = xb + (int64_t)t * T;
            if (k < full_rows) {
#pragma unroll
                for (int j = 0; j < V4; ++j) {
                    const f4u v = *reinterpret_cast<const f4u*>(xs + n0 + 2 * j);
                    dst[t][2 * j] = make_float2(v.x, v.y);
                    dst[t][2 * j + 1] = make_float2(v.z, v.w);
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) dst[t][e] = (n0 + e < T) ? xs[n0 + e] : make_float2(0.f, 0.f);
            }
        }
    }

    template <int U, bool FIRST, bool GUARD>
    __device__ __forceinline__ void row(int k) {
        constexpr int sl = U % MR;                           // ring slot of row k-MR (and k)
        constexpr int so = (U + 1) % MR;                     // slot of C[k-MR+1]
        const int nb = RL * k + E * lane;
        float2 cur[NA][E];
#pragma unroll
        for (int t = 0; t < NA; ++t)
#pragma unroll
            for (int e = 0; e < E; ++e) cur[t][e] = nx[U % PD][t][e];
        if (!GUARD || k + PD < nrows) load_row(k + PD, nx[U % PD]);
        // lagged samples x[n-L] (row k-MR) of every antenna
        pf2 d[NA][E];
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            if constexpr (LDSLAG) {
#pragma unroll
                for (int j = 0; j < V4; ++j) {
                    const float4 v = FIRST ? make_float4(0.f, 0.f, 0.f, 0.f) : lag[sl][t][j][lane];
                    d[t][2 * j] = pf2{v.x, v.y}; d[t][2 * j + 1] = pf2{v.z, v.w};
                    lag[sl][t][j][lane] = make_float4(cur[t][2 * j].x, cur[t][2 * j].y, cur[t][2 * j + 1].x,
                                                      cur[t][2 * j + 1].y);
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    d[t][e] = lx[t][sl][e];
                    lx[t][sl][e] = pf2{cur[t][e].x, cur[t][e].y};
                }
            }
        }
        // From here to the row bases: aa_fast_kernel's row sums, expression for expression (the tests hold
        // the kernels bit-identical to each other, so the two copies move together).  One shared function
        // was built and measured: bit-identical, but the two-antenna kernel here ran 0.4-0.5 % slower in
        // every round and three aa_fast_kernel instantiations lost a wave per SIMD
        // (profiles/aa_fast_rowsums_candidates.txt).
        // ---- lagged products x[n]·conj(x[n-L]) and energies, summed over the antennas ----
        pf2 av[E];
        float aE[E];
#pragma unroll
        for (int e = 0; e < E; ++e) { av[e] = pf2{0.f, 0.f}; aE[e] = 0.f; }
#pragma unroll
        for (int t = 0; t < NA; ++t)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const pf2 c = pf2{cur[t][e].x, cur[t][e].y};
                aE[e] += fmaf(c.x, c.x, c.y * c.y);
                if (!FIRST) av[e] = mulc_acc(c, d[t][e], av[e]);
            }
        // ---- in-lane partials (forward f, backward g), fp64 wave scan ----
        pf2 fS[E], gS[E];
        float fE[E], gE[E];
        fS[0] = av[0]; fE[0] = aE[0];
#pragma unroll
        for (int e = 1; e < E; ++e) { fS[e] = fS[e - 1] + av[e]; fE[e] = fE[e - 1] + aE[e]; }
        gS[E - 1] = pf2{0.f, 0.f}; gE[E - 1] = 0.f;
#pragma unroll
        for (int e = E - 2; e >= 0; --e) { gS[e] = gS[e + 1] + av[e + 1]; gE[e] = gE[e + 1] + aE[e + 1]; }
        const RowScan se_ = row_scan<false>(fE[E - 1]);
        const double tE = se_.tot;
        const float xE = se_.x, uE = se_.u;
        double tR = 0.0, tI = 0.0;
        pf2 xS = pf2{0.f, 0.f}, uS = pf2{0.f, 0.f};
        if (!FIRST) {                                        // no lagged product before row MR
            const RowScan sr_ = row_scan<false>(fS[E - 1].x), si_ = row_scan<false>(fS[E - 1].y);
            tR = sr_.tot; tI = si_.tot;
            xS = pf2{sr_.x, si_.x};
            uS = pf2{sr_.u, si_.u};
        }
        const pf2 wS = FIRST ? pf2{(float)CR, (float)CI} : pf2{(float)(CR - cbR[so]), (float)(CI - cbI[so])};
        const float wE = (float)(FIRST ? CE : CE - cbE[so]);
        // ---- window sums P = suffix(row k-MR) + rows between + prefix(row k) ----
        float pr[E], pi[E], rf[E], mf[E], pmf[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            pf2 P = wS + (xS + fS[e]);
            float RR = wE + (xE + fE[e]);
            if (!FIRST) { P += sS[sl][e]; RR += sE[sl][e]; }
            sS[sl][e] = uS + gS[e]; sE[sl][e] = uE + gE[e];
            const float pm = fmaf(P.x, P.x, P.y * P.y);
            float m = 0.f;
            if (!FIRST && RR > floor_) m = fminf(pm * __builtin_amdgcn_rcpf(RR * RR), 1.f);
            pr[e] = P.x; pi[e] = P.y; rf[e] = RR; mf[e] = m; pmf[e] = pm;
        }
        cbR[so] = CR + tR; cbI[so] = CI + tI; cbE[so] = CE + tE;
        CR += tR; CI += tI; CE += tE;
        // ---- stores ----
        if (!DO) {
            const int64_t o = o0 + nb;
            // resident head (OFS_AA_HEAD_RESIDENT): the FIRST rows are n < L, where P = M = +0.0 is
            // already in the caller's buffers
            float2* const Pk = (FIRST && head) ? nullptr : Pout;
            float* const Mk = (FIRST && head) ? nullptr : Mout;
            if (!GUARD || k < full_rows) {
#pragma unroll
                for (int j = 0; j < V4; ++j) {
                    if (Pk) *reinterpret_cast<f4u*>(Pk + o + 2 * j) = f4u{pr[2 * j], pi[2 * j], pr[2 * j + 1], pi[2 * j + 1]};
                    if (Rout) *reinterpret_cast<f2u*>(Rout + o + 2 * j) = f2u{rf[2 * j], rf[2 * j + 1]};
                    if (Mk) *reinterpret_cast<f2u*>(Mk + o + 2 * j) = f2u{mf[2 * j], mf[2 * j + 1]};
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (nb + e < Ti) {
                        if (Pk) Pk[o + e] = make_float2(pr[e], pi[e]);
                        if (Rout) Rout[o + e] = rf[e];
                        if (Mk) Mk[o + e] = mf[e];
                    }
            }
            if (Vout) {
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (nb + e < Ti) Vout[o + e] = (uint8_t)(!FIRST);
            }
        }
        // ---- events: closed-form gate machine, streamed per row (aa_gate.h) ----
        if (!FIRST && detect) gate.row(lane, k, nb, Ti, mf, pmf, pr, pi);
    }

    // rows [k0, k0 + PER) with k0 % PER == 0; FIRST_BLOCK: k0 == 0 (rows < MR are FIRST)
    template <bool FIRST_BLOCK, bool GUARD, int U = 0>
    __device__ __forceinline__ void block(int k0) {
        if constexpr (U < PER) {
            const int k = k0 + U;
            if (!GUARD || k < nrows) {
                row<U, FIRST_BLOCK && (U < MR), GUARD>(k);
                block<FIRST_BLOCK, GUARD, U + 1>(k0);
            }
        }
    }
};

template <int E, int MR, int NA, bool DO>
__global__ __launch_bounds__(stream_wg(NA, DO)) void aa_stream_kernel(AaFastArgs a) {
    using S = AaStream<E, MR, NA, DO>;
    constexpr int SWG = stream_wg(NA, DO);
    __shared__ float4 lagbuf[SWG / 64][S::LDSLAG ? MR : 1][NA][S::V4][64];
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)(NA == 1 ? blockIdx.x : xcd_block()) * (SWG / 64) + (threadIdx.x >> 6);   // (as aa_fast_kernel)
    if (b >= a.B) return;
    S s;
    s.lane = lane;
    s.lag = lagbuf[threadIdx.x >> 6];
    s.T = a.T;
    s.Ti = (int)a.T;
    s.o0 = b * a.T;
    s.nrows = (int)((a.T + S::RL - 1) / S::RL);
    s.full_rows = (int)(a.T / S::RL);                        // rows entirely inside the stream
    s.xb = reinterpret_cast<const float2*>(a.x) + b * NA * a.T;
    s.CR = s.CI = s.CE = 0.0;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        s.cbR[m] = 0.0; s.cbI[m] = 0.0; s.cbE[m] = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            s.sS[m][e] = pf2{0.f, 0.f}; s.sE[m][e] = 0.f;
#pragma unroll
            for (int t = 0; t < (S::LDSLAG ? 1 : NA); ++t) s.lx[t][m][e] = pf2{0.f, 0.f};
        }
    }
#pragma unroll
    for (int p = 0; p < S::PD; ++p)
        if (p < s.nrows) s.load_row(p, s.nx[p]);
    s.detect = a.detect != 0;
    if (s.detect)
        s.gate.init(a.hyst, S::L, a.thr, a.fs, a.max_ev, a.ev_i + b * (int64_t)a.max_ev * 4,
                    a.ev_r + b * (int64_t)a.max_ev * 4);
    s.Pout = DO ? nullptr : reinterpret_cast<float2*>(a.P);
    s.Rout = DO ? nullptr : reinterpret_cast<float*>(a.R);
    s.Mout = DO ? nullptr : reinterpret_cast<float*>(a.M);
    s.Vout = DO ? nullptr : a.valid;
    s.head = !DO && a.head_resident != 0;
    s.floor_ = 1e-6f * (float)S::L;

    // warm-up block (rows 0..PER-1: the first MR have no lagged product), steady blocks of
    // whole rows with no per-row guards, then the guarded tail
    s.template block<true, true>(0);
    int k0 = S::PER;
    for (; k0 + S::PER + S::PD <= s.full_rows; k0 += S::PER) s.template block<false, false>(k0);
    for (; k0 < s.nrows; k0 += S::PER) s.template block<false, true>(k0);
    if (a.detect) s.gate.finish(lane, s.Ti, a.n_ev + b);
}

template <int E, int MR, int NA>
int launch_stream(const AaFastArgs& a, hipStream_t st) {
    const bool det_only = a.detect && !a.P && !a.R && !a.M && !a.valid;
    constexpr int WGD = stream_wg(NA, true), WGS = stream_wg(NA, false);
    const int64_t grid = det_only ? (a.B + WGD / 64 - 1) / (WGD / 64) : (a.B + WGS / 64 - 1) / (WGS / 64);
    // occupancy cap of the two-antenna storing kernel: 24 KiB of LDS per workgroup in all (unused
    // dynamic LDS on top of its 8 KiB lag ring at L 512) = 6 workgroups per CU.  Paired on the
    // reference's detector shape (16384 x 2 x 5315, L 512; 3 rounds, profiles/r06g_occupancy_sweeps.txt):
    // lag ring alone 0.6005 ms, + 8 KiB 0.5843, + 12 KiB 0.5783, + 16 KiB 0.5737, + 20 KiB 0.6044
    // (~27 KiB per workgroup rounds up past 160 KiB / 6: 5 per CU); one antenna at T = 4096 is faster
    // uncapped (1.186 vs 1.228 ms).  variant OCC_LDS (bytes added) overrides.
    using S = AaStream<E, MR, NA, false>;
    constexpr size_t lag_lds = (size_t)(WGS / 64) * (S::LDSLAG ? MR : 1) * NA * S::V4 * 64 * 16;
    constexpr size_t cap_total = 24 * 1024;
    const size_t dflt = (!det_only && NA == 2 && cap_total > lag_lds) ? cap_total - lag_lds : 0;
    const size_t shm = ofs::variant(ofs::V_OCC_LDS) == INT64_MIN ? dflt : ofs::occ_lds();
    if (det_only)
        hipLaunchKernelGGL((aa_stream_kernel<E, MR, NA, true>), dim3((unsigned)grid), dim3(WGD), shm, st, a);
    else
        hipLaunchKernelGGL((aa_stream_kernel<E, MR, NA, false>), dim3((unsigned)grid), dim3(WGS), shm, st, a);
    return hipGetLastError() == hipSuccess ? 1 : OFS_EHIP;
}

// ofs_aa_fast_plan tries E = 2 first, so E = 4 is reached only by L = 2048 (MR = 8): its other
// windows are not instantiated (0: the general engine)
template <int E, int NA>
int launch_stream_mr(int mr, const AaFastArgs& a, hipStream_t st) {
    if (mr == 8) return launch_stream<E, 8, NA>(a, st);
    if constexpr (E == 2) {
        switch (mr) {
            case 1: return launch_stream<E, 1, NA>(a, st);
            case 2: return launch_stream<E, 2, NA>(a, st);
            case 4: return launch_stream<E, 4, NA>(a, st);
        }
    }
    return 0;
}

// row-scan precision of the register-staged kernel: the detect-only launch scans in fp32, the
// storing launch in fp64; variants FAST_SCAN_DO / FAST_SCAN = 32 | 64 override (tests run the
// storing kernel with the detect-only arithmetic to classify its events, A/B)
bool scan32(bool det_only) {
    const int64_t v = ofs::variant(det_only ? ofs::V_FAST_SCAN_DO : ofs::V_FAST_SCAN);
    if (v == 32 || v == 64) return v == 32;
    return det_only;
}

// The smallest float >= thr.  For a float m, (double)m >= thr exactly when m >= that float: a float at
// or above thr is at or above the smallest such float, and that float is itself >= thr.  NaN stays NaN
// (both compares false), thr beyond FLT_MAX gives +inf (only m = +inf passes, as in fp64), thr below
// -FLT_MAX gives -FLT_MAX (m = -inf fails, as in fp64), a subnormal stays exact (the kernels keep fp32
// subnormals); the sign of a zero does not matter to >=.
float thr_as_f32(double thr) {
    if (thr != thr || thr == (double)INFINITY || thr == -(double)INFINITY) return (float)thr;
    if (thr > (double)FLT_MAX) return INFINITY;
    if (thr < -(double)FLT_MAX) return -FLT_MAX;
    float f = (float)thr;                                    // in range: round to nearest
    if ((double)f < thr) f = nextafterf(f, INFINITY);
    return f;
}

template <int E, int MR, int NA>
int launch(const AaFastArgs& a, hipStream_t st) {
    const bool det_only = a.detect && !a.P && !a.R && !a.M && !a.valid;
    const bool s32 = scan32(det_only);
    const dim3 grid((unsigned)a.B), blk(FAST_WG);            // one wave = one stream per workgroup
    // Occupancy cap: the P/R/M-storing one-antenna kernel runs 10 workgroups (waves) per CU instead
    // of the 12 its 139 VGPRs allow, through 16 KiB of unused dynamic LDS per workgroup (160 KiB per
    // CU / 10).  Paired, 11 rotated rounds on the headline (profiles/r06d_headline_occupancy_sweep.json):
    // 12 per CU 0.2980 ms, 11 0.2920, 10 0.2908, 9 0.2948, 8 0.2954 - fewer streams in flight per CU
    // beat more (so do 3 vs 4 vs 5 waves/SIMD, r06b).  variant FAST_LDS = bytes per workgroup
    // overrides (1: no cap, A/B).
    const int64_t pad = ofs::variant_or(ofs::V_FAST_LDS, (!det_only && NA == 1) ? FAST_CAP_LDS : 0);
    const size_t shm = pad > 0 && pad <= 65536 ? (size_t)pad : 0;
    // store path of the one-antenna E = 2 storing kernel with fp64 scans (the headline): row-paired
    // 16-byte R/M stores and non-temporal P/R/M stores.  Paired on the same buffers, 3 fresh allocations x
    // 11 rotated repetitions, against plain float2 stores (profiles/headline_store_path_arms.jsonl; A/A
    // spread 0.04 %): pairing alone -0.3..-1.0 %, non-temporal alone -6.7..-7.9 %, both -8.1..-9.3 %
    // (0.2805-0.2834 -> 0.2571-0.2584 ms); write-through forms (sc1, sc0 sc1) within +-0.1 % of plain,
    // removed.  Variants FAST_RMPAIR = 0 | 1, FAST_ST_POLICY = 0 | 1 override (tests: bit-identity).
    if constexpr (E == 2 && NA == 1) {
        if (!det_only && !s32) {
            const int sv = (ofs::variant_or(ofs::V_FAST_RMPAIR, 1) != 0 ? 2 : 0) | (ofs::variant_or(ofs::V_FAST_ST_POLICY, 1) == 1 ? 1 : 0);
            // full-stream form (aa_fast_kernel, FS) for the shape the batch detector launches: a whole
            // stream, every output and the events; windows of 1, 2, 4 rows.  Variant FAST_FULL = 0: the
            // generic form (A/B, the tests' reference arm).  The gate rows are chosen here, once.
            if constexpr (MR == 1 || MR == 2 || MR == 4) {
                if (sv == 3 && a.T == TMAX && a.P && a.R && a.M && !a.valid && a.detect && a.n_ev && a.ev_i && a.ev_r &&
                    !ofs::variant_off(ofs::V_FAST_FULL)) {
                    AaFastArgs f = a;
                    f.thr32 = thr_as_f32(a.thr);
                    // Its own occupancy cap: with a third fewer instructions per stream the waves reach their
                    // loads and stores sooner, and the steady-state optimum moves from 10 to 7 workgroups per CU
                    // (paired on the same buffers, 8 allocations in 3 sessions, profiles/headline_full_cap_*.jsonl:
                    // 7 per CU -4.1..-8.6 % against 10, 8 and 9 per CU -0.9..-3.0 %, 6 per CU +7.4..+9.9 %; the
                    // generic form at 7 per CU +17..+20 %).  At 10 per CU this form is 2.6 % faster to 8.2 %
                    // slower than the generic one in steady state; at 7 it is 0.4..6.8 % faster.  The first
                    // launches after other work (bench.py's 110) prefer 10 by ~4 % (0.198-0.209 against
                    // 0.205-0.213 ms) - both beat the generic form's 0.220-0.226 ms.  DESIGN.md §4.1.
                    const int64_t padf = ofs::variant_or(ofs::V_FAST_LDS, FAST_CAP_LDS_FULL);
                    const size_t shmf = padf > 0 && padf <= 65536 ? (size_t)padf : 0;
                    const bool ff = (a.hyst > 1 ? a.hyst : 1) >= 64 * E;
                    // Input loads non-temporal (ld_x; variant FAST_LD_POLICY = 0: plain, the tests' reference arm;
                    // any other value is the default).  Paired on the same buffers against plain loads, 3 fresh
                    // allocations x 11 rotated repetitions: -4.4..-6.3 %; the raw-buffer-load forms measured with
                    // it (plain, sc1, sc0 sc1 within +-0.5 % of the plain global load, nt = this arm) were removed.
                    // The cap was re-swept under it and stays at 7 per CU.  DESIGN.md §4.1.
                    const bool nt = ofs::variant(ofs::V_FAST_LD_POLICY) != 0;
                    if (ff && nt) hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 3, 1, 1>), grid, blk, shmf, st, f);
                    else if (ff) hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 3, 1, 0>), grid, blk, shmf, st, f);
                    else if (nt) hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 3, 2, 1>), grid, blk, shmf, st, f);
                    else hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 3, 2, 0>), grid, blk, shmf, st, f);
                    return hipGetLastError() == hipSuccess ? 1 : OFS_EHIP;
                }
            }
            switch (sv) {
                case 0: hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 0>), grid, blk, shm, st, a); break;
                case 1: hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 1>), grid, blk, shm, st, a); break;
                case 2: hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 2>), grid, blk, shm, st, a); break;
                default: hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false, 3>), grid, blk, shm, st, a);
            }
            return hipGetLastError() == hipSuccess ? 1 : OFS_EHIP;
        }
    }
    if (det_only && s32) hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, true, true>), grid, blk, shm, st, a);
    else if (det_only) hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, true, false>), grid, blk, shm, st, a);
    else if (s32) hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, true>), grid, blk, shm, st, a);
    else hipLaunchKernelGGL((aa_fast_kernel<E, MR, NA, false, false>), grid, blk, shm, st, a);
    return hipGetLastError() == hipSuccess ? 1 : OFS_EHIP;
}

template <int E, int NA, int MR = 1>
int launch_mr(int mr, const AaFastArgs& a, hipStream_t st) {
    if constexpr (MR > TMAX / (64 * E)) {
        return 0;
    } else {
        if (mr == MR) return launch<E, MR, NA>(a, st);
        return launch_mr<E, NA, MR + 1>(mr, a, st);
    }
}

template <int NA>
int launch_e(int E, int mr, const AaFastArgs& a, hipStream_t st) {
    switch (E) {
        case 2: return launch_mr<2, NA>(mr, a, st);
        case 4: return launch_mr<4, NA>(mr, a, st);
        case 8: return launch_mr<8, NA>(mr, a, st);
    }
    return 0;
}

int pick_e(int L) {
    // samples per lane per row; variant FAST_E = 2|4|8 overrides (A/B, parity classification)
    const int forced = (int)ofs::variant_or(ofs::V_FAST_E, 0);
    if (forced == 2 || forced == 4 || forced == 8) return (L % (64 * forced) == 0) ? forced : 0;
    for (int e : {2, 4, 8})                                  // E=2 measured 3 % faster than 4 (r01c)
        if (L % (64 * e) == 0) return e;
    return 0;
}

// detect-only (events without P/R/M stores: VALU/issue-bound, not HBM-bound, SQ counters r03a):
// samples per lane per row.  With fp32 row scans (3 x ~7 VALU per row instead of ~25) E = 4 is
// the fastest (r03f: 0.1071 ms vs 0.1134 at E = 8, 0.1191 / 0.1193 with fp64 scans at E = 4 / 8);
// variant FAST_E_DO = 2|4|8 overrides.
int pick_e_do(int L) {
    const int forced = (int)ofs::variant_or(ofs::V_FAST_E_DO, 0);
    for (int e : {forced, 4, 8, 2})
        if ((e == 2 || e == 4 || e == 8) && L % (64 * e) == 0) return e;
    return 0;
}

}  // namespace

// 10*E + MR of the register-staged kernel (even T <= 1024), 100 + 10*E + MR of the streaming
// kernel (any other T), 0 if the general engine handles the shape
int ofs_aa_fast_plan(int fmt, int precision, int n_ant, int64_t T, int L) {
    if (fmt != OFS_C64 || precision != OFS_FP32) return 0;
    if (n_ant != 1 && n_ant != 2) return 0;
    if (T < 1 || L < 128) return 0;
    if (T <= TMAX && !(T & 1) && L <= TMAX) {
        const int E = pick_e(L);
        if (E) return 10 * E + L / (64 * E);
    }
    if (T > 0x7fffffff - 1024) return 0;                     // row indices in int
    for (int e : {2, 4}) {                                   // streaming: window of 1, 2, 4 or 8 rows
        if (L % (64 * e)) continue;
        const int mr = L / (64 * e);
        if (mr == 1 || mr == 2 || mr == 4 || mr == 8) return 100 + 10 * e + mr;
    }
    return 0;
}

int ofs_aa_fast_try(int fmt, int precision, int n_ant, const AaFastArgs& a, hipStream_t st) {
    const int plan = ofs_aa_fast_plan(fmt, precision, n_ant, a.T, a.L);
    if (!plan) return 0;
    if (plan >= 100) {
        const int E = (plan - 100) / 10, mr = plan % 10;
        if (E == 2) return n_ant == 1 ? launch_stream_mr<2, 1>(mr, a, st) : launch_stream_mr<2, 2>(mr, a, st);
        return n_ant == 1 ? launch_stream_mr<4, 1>(mr, a, st) : launch_stream_mr<4, 2>(mr, a, st);
    }
    int E = plan / 10, mr = plan % 10;
    if (a.detect && !a.P && !a.R && !a.M && !a.valid) {
        // detect-only: its own row width (fewer fp64 row scans per sample); the events are those of
        // the same window sums in another fp32 summation order (parity: oracle/parity.py criterion)
        const int ed = pick_e_do(a.L);
        if (ed) { E = ed; mr = a.L / (64 * ed); }
    }
    return n_ant == 1 ? launch_e<1>(E, mr, a, st) : launch_e<2>(E, mr, a, st);
}
