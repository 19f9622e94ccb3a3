// rtl_chunk.hip — resumable form of rtl_exact_kernel for integer streams of any length
// (ofs_minn_rtl_chunk): one call takes the next Tc samples of B streams and returns the eight
// minn_rtl arrays of those samples and the gate events that closed among them; what the next call
// needs stays in a caller-owned state buffer on the device.
//
// HISTORY, NOT RUNNING SUMS.  Per stream the state keeps the last 3Q samples per branch as decoded
// int16 I/Q words.  A call runs the one-shot kernel's row loop over the virtual stream
// [history (3Q) | chunk (Tc)]: the 3·MW history rows only refill the lag words and the prefix rings
// (no stores, no smoothing, no gate).  corr_total[i] and energy_total[i] depend on x[i-3Q+1 .. i]
// only, so every chunk position sees the window sums of the unbroken stream.  The lag products of
// the first Q history samples are formed against a zero lag line; that adds one and the same
// integer to every prefix that enters c0-c1, c1-c2 (both windows start at or after history sample
// Q + 1), so it cancels.  All prefixes are exact integers ((Tc + 3Q)·n_br <= 2^21 keeps them below
// 2^53, for full-range int16 words too).  A fresh stream's history is zeros: the zero delay lines.
//
// ABSOLUTE INDEX.  The state carries n_seen.  The reference's registers hold 0 until their first
// valid sample (corr/energy_recent from Q-1, the previous taps from 2Q-1, the third energy tap and
// metric_valid from 3Q-1): each test is made on n_seen + i per sample, so a chunk edge may fall
// anywhere, inside the first 3Q samples of the stream too.
//
// IIR STATE.  sm (the float state, f64 bits) and si (the floor state) are carried exactly; the
// smoothing's 256-sample segments start at the chunk's first sample and lane 0 of the first segment
// enters with the carried state, so an accepted chain is the reference trajectory whatever the
// chunking (rtl_smooth.h).  A carried state below 2^-700 fails the fma path's guard like any other
// entering state and takes the general path.
//
// GATE.  AaRowGate, RTL + ABS form, in call-local gate coordinates g = chunk index + 256·KOFF,
// KOFF = ceil(max(H, 1) / 256) segments, so that the last above-threshold position of an earlier call
// is never negative while it can still matter.  Unlike sync_aa the RTL machine never closes a gate
// at the end of the stream: every call reports open_gate_start, final or not.
//
// State of one stream (ofs_rtl_chunk_state_bytes = 128 + 24·n_br·Q bytes, all-zero = fresh):
//   RtlChunkHdr (128 B), then two history slots [2][n_br][3Q] int32 words.  A call reads slot
//   `parity` and writes the other one, so no word is overwritten before it is read.
#include "chunk_state.h"
#include "aa_gate.h"
#include "aa_words.h"
#include "rtl_smooth.h"
#include "ofdmsync.h"

#include <type_traits>

using namespace ofs;

namespace {

struct RtlChunkHdr {
    int64_t n_seen;                 // samples of this stream consumed by earlier calls
    int64_t carry_p1;               // 1 + absolute index of the last above-threshold sample, 0 = none
    int64_t ev_start, bidx;         // open gate: its start, its peak so far (absolute)
    double bpm;                     // open gate: corr_positive at that peak
    double sm;                      // IIR state, float mode (and (double)si in floor mode)
    int64_t si;                     // IIR state, floor mode
    int32_t gate_open, parity;      // parity: history slot holding the last 3Q samples
    int32_t wide, pad0;             // wide: a word beyond 12 bits was seen (sticky; int32 row scans off)
    int64_t pad[7];
};
static_assert(sizeof(RtlChunkHdr) == 128, "state header");

struct RtlChunkArgs {
    const void* x; int64_t B, Tc;
    uint8_t* state; int64_t state_bytes;
    int32_t shift, smooth_mode, frac_bits; double thr_value;
    double* corr_total; double* corr_positive; double* smooth; double* energy_total;
    double* corr_scaled; double* energy_scaled; uint8_t* mvalid; uint8_t* above;
    int32_t detect, hyst, toff, max_ev; int32_t* n_ev; int64_t* ev; int64_t* open_start;
    int32_t fin;
};

constexpr int XR = 256;                 // up to 4 waves = 4 streams per workgroup

// The header is the same for every lane of the wave: its fields are moved to scalar registers
// (v_readfirstlane), where they live through the kernel.  Held in vector registers they took the kernel
// past 128 VGPRs, 3 waves per SIMD instead of the one-shot kernel's 4.
__device__ __forceinline__ int32_t uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni(int64_t v) {
    return (int64_t)(((uint64_t)(uint32_t)uni((int32_t)((uint64_t)v >> 32)) << 32) | (uint32_t)uni((int32_t)v));
}
__device__ __forceinline__ double uni(double v) { return __longlong_as_double(uni((int64_t)__double_as_longlong(v))); }
__device__ __forceinline__ RtlChunkHdr load_hdr(const RtlChunkHdr* p) {
    const RtlChunkHdr v = *p;
    RtlChunkHdr h{};
    h.n_seen = uni(v.n_seen); h.carry_p1 = uni(v.carry_p1); h.ev_start = uni(v.ev_start); h.bidx = uni(v.bidx);
    h.bpm = uni(v.bpm); h.sm = uni(v.sm); h.si = uni(v.si);
    h.gate_open = uni(v.gate_open); h.parity = uni(v.parity); h.wide = uni(v.wide);
    return h;
}

// per-wave LDS: rtl_exact_kernel's layout plus the floor-mode state handed to the walker lane
__host__ __device__ constexpr size_t rtl_chunk_wave_lds(int E, int MW, int nb) {
    return rtl_wave_lds(E, MW, nb) + 2 * sizeof(double);
}

template <int E, int MW, int NB, bool CP>
__global__ __launch_bounds__(XR) void rtl_chunk_kernel(RtlChunkArgs a) {
#pragma clang fp contract(off)
    constexpr int RL = 64 * E;
    constexpr int Q = MW * RL;
    constexpr int NR = rtl_ring_rows(MW);
    constexpr int H = 3 * Q;                                       // history samples = HR whole rows
    constexpr int HR = 3 * MW;
    constexpr int RPS = SEG / RL;
    static_assert(SEG % RL == 0, "segment = whole metric rows");
    extern __shared__ __attribute__((aligned(16))) double rcm[];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int wpb = blockDim.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * wpb + w;
    const int64_t Tc = a.Tc;
    const int nseg = (int)((Tc + SEG - 1) / SEG);
    constexpr size_t wave_dbl = rtl_chunk_wave_lds(E, MW, NB) / sizeof(double);
    constexpr size_t hst_off = rtl_wave_lds(E, MW, NB) / sizeof(double);
    const int smode = a.smooth_mode == 1 ? 2 : (a.shift == 0 ? 1 : 0);
    const bool walk = smode == 2;                                  // RTL floor IIR: walker lane (barriers)
    if (b >= a.B) {                 // no stream: still meet the workgroup's two barriers per segment
        if (walk)
            for (int g = 0; g < nseg; ++g) { lds_barrier(); lds_barrier(); }
        return;
    }
    double* hae_ = rcm + wave_dbl * w;
    double* hac_ = hae_ + NR * E * 64;
    double* hcp = hac_ + NR * E * 64;                                // segment corr_positive
    double* hes = hcp + SEG_PAD;                                     // segment energy_scaled
    int32_t* hx_ = reinterpret_cast<int32_t*>(hes + SEG_PAD);
    double* hst = rcm + wave_dbl * w + hst_off;                      // floor mode: sm, si for the walker
    auto hae = [&](int r, int e) -> double& { return hae_[(r * E + e) * 64 + lane]; };
    auto hac = [&](int r, int e) -> double& { return hac_[(r * E + e) * 64 + lane]; };
    auto hx = [&](int t, int m, int e) -> int32_t& { return hx_[((t * MW + m) * E + e) * 64 + lane]; };

    uint8_t* sp = a.state + b * a.state_bytes;
    RtlChunkHdr* hdr = reinterpret_cast<RtlChunkHdr*>(sp);
    const RtlChunkHdr h = load_hdr(hdr);
    const int par = h.parity & 1;
    int32_t* hist = reinterpret_cast<int32_t*>(sp + sizeof(RtlChunkHdr));
    const int32_t* hin = hist + (int64_t)par * NB * H;
    int32_t* hout = hist + (int64_t)(par ^ 1) * NB * H;

    const int nrows = (int)((Tc + RL - 1) / RL);                     // chunk rows
    const int32_t* xs = reinterpret_cast<const int32_t*>(a.x) + b * NB * Tc;
    const int64_t sbyte = b * NB * Tc * 3;                         // CP12: stream start in bytes
    const uint8_t* x8 = reinterpret_cast<const uint8_t*>(a.x) + sbyte;
    const int64_t total = a.B * NB * Tc * 3;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) { hae(r, e) = 0.0; hac(r, e) = 0.0; }
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int m = 0; m < MW; ++m)
#pragma unroll
            for (int e = 0; e < E; ++e) hx(t, m, e) = 0;

    // chunk index from which the sample with absolute index n is reached (0: already passed)
    auto rel = [&](int64_t n) -> int {
        const int64_t d = n - h.n_seen;
        return d <= 0 ? 0 : (d > 0x7fffffff ? 0x7fffffff : (int)d);
    };
    const int t1 = rel(Q - 1), t2 = rel(2 * Q - 1), t3 = rel(3 * Q - 1);   // t3: first metric_valid sample
    const int64_t row_off = b * Tc;
    const bool vec_st = (Tc % SC) == 0 && (reinterpret_cast<uintptr_t>(a.above) & 3) == 0 &&
                        ((reinterpret_cast<uintptr_t>(a.smooth) | reinterpret_cast<uintptr_t>(a.corr_scaled)) & 15) == 0;
    const double inv = ldexp(1.0, -(a.shift > 0 ? a.shift : 0));   // exact 1 / 2^shift
    const double keep = 1.0 - inv;
    const double scale = (double)(1ll << a.frac_bits);
    double CC = 0.0, CE = 0.0;
    bool wide = h.wide != 0;                                       // carried: the history words count
    double sm = h.sm;                                              // IIR state carried between segments and calls
    long long si = h.si;
    if (walk && lane == 0) { hst[0] = sm; hst[1] = __longlong_as_double(si); }

    // gate coordinates: chunk index + GO, absolute index = gate coordinate + abs0
    const int Hp = a.hyst > 1 ? a.hyst : 1;
    const int KOFF = (Hp + SEG - 1) / SEG;
    const int GO = SEG * KOFF;
    const int Tg = (int)Tc + GO;                                   // end of the chunk
    AaRowGate<SC, double, true, true, false, true> gate;           // detect_minn_rtl, closed form, resumable
    if (a.detect) {
        gate.init(a.hyst, Q, 0.0, 0.0, a.max_ev, a.ev ? a.ev + b * (int64_t)a.max_ev * 4 : nullptr, nullptr, a.toff);
        gate.load(h.n_seen - GO, h.carry_p1, h.gate_open, h.ev_start, h.bidx, h.bpm, 0.0, 0.0, 0.0);
    }

    // chunk rows arrive one segment ahead of use (rtl_exact_kernel: a segment takes all its rows before
    // it issues any store); the history rows are all taken at once before them
    int32_t nx[RPS][NB][E];
    auto load_row = [&](int64_t n0, int32_t (&dst)[NB][E]) {
        if constexpr (CP) {
            cp12_load<E, NB>(x8, sbyte, n0, Tc, total, dst);
        } else {
#pragma unroll
            for (int t = 0; t < NB; ++t) load_words<E>(xs + t * Tc, n0, Tc, dst[t]);
        }
    };
    auto load_seg = [&](int g) {
#pragma unroll
        for (int j = 0; j < RPS; ++j)
            if (g * RPS + j < nrows) load_row((int64_t)RL * (g * RPS + j) + E * lane, nx[j]);
    };
    // the last 3Q samples of [history | chunk] become the next call's history (other slot); hi = the
    // word's index there
    auto keep_words = [&](int64_t hi, const int32_t (&cur)[NB][E]) {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (hi + e >= 0 && hi + e < H) {
#pragma unroll
                for (int t = 0; t < NB; ++t) hout[t * H + hi + e] = cur[t][e];
            }
    };
    // lag products and energies of virtual row k, their row prefix, the prefix rings
    auto ring_row = [&](int k, const int32_t (&cur)[NB][E], double (&c0)[E], double (&e0)[E]) {
        const int xsl = k % MW;
        // int32 row scans while every word seen is 12-bit (rtl_exact_kernel): the same integers
        constexpr bool IROW = 64 * E * NB <= 128;
        if constexpr (IROW && !CP) {
            int bad = 0;
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int32_t wd = cur[t][e];
                    bad |= (int)((unsigned)((int16_t)(wd & 0xffff) + 2048) >= 4096u) |
                           (int)((unsigned)((wd >> 16) + 2048) >= 4096u);
                }
            wide = wide || __ballot(bad) != 0;
        }
        double qcf[E], qef[E], qcx, qex, qct, qet;
        if (IROW && !wide) {
            int pc[E], en[E];
#pragma unroll
            for (int e = 0; e < E; ++e) { pc[e] = 0; en[e] = 0; }
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int32_t d = hx(t, xsl, e);
                    const int xr = (int16_t)(cur[t][e] & 0xffff), xi = cur[t][e] >> 16;
                    pc[e] += (int16_t)(d & 0xffff) * xr + (d >> 16) * xi;   // minn_rtl.py:616, exact
                    en[e] += xr * xr + xi * xi;                               // :617
                    hx(t, xsl, e) = cur[t][e];
                }
            RowPrefixI<E> ic, ie;
            ic.run(pc); ie.run(en);
#pragma unroll
            for (int e = 0; e < E; ++e) { qcf[e] = (double)ic.f[e]; qef[e] = (double)ie.f[e]; }
            qcx = (double)ic.excl; qex = (double)ie.excl; qct = (double)ic.tot; qet = (double)ie.tot;
        } else {
            double pc[E], en[E];
#pragma unroll
            for (int e = 0; e < E; ++e) { pc[e] = 0.0; en[e] = 0.0; }
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int32_t d = hx(t, xsl, e);
                    const double xr = w_re(cur[t][e]), xi = w_im(cur[t][e]);
                    pc[e] += w_re(d) * xr + w_im(d) * xi;            // minn_rtl.py:616, exact
                    en[e] += xr * xr + xi * xi;                       // :617
                    hx(t, xsl, e) = cur[t][e];
                }
            RowPrefix<E> dc, de;
            dc.run(pc); de.run(en);
#pragma unroll
            for (int e = 0; e < E; ++e) { qcf[e] = dc.f[e]; qef[e] = de.f[e]; }
            qcx = dc.excl; qex = de.excl; qct = dc.tot; qet = de.tot;
        }
        const int s0r = k % NR;                                        // slot of row k
#pragma unroll
        for (int e = 0; e < E; ++e) {
            c0[e] = (CC + qcx) + qcf[e];
            e0[e] = (CE + qex) + qef[e];
            hac(s0r, e) = c0[e];
            hae(s0r, e) = e0[e];
        }
        CC += qct; CE += qet;
    };

    if (nrows > 0) {
        load_seg(0);
        // ---------------- history rows: lag words and prefix rings only ----------------------------
        int32_t hrow[HR][NB][E];
#pragma unroll
        for (int k = 0; k < HR; ++k)
#pragma unroll
            for (int t = 0; t < NB; ++t) load_words<E>(hin + t * H, (int64_t)RL * k + E * lane, H, hrow[k][t]);
#pragma unroll
        for (int k = 0; k < HR; ++k) {
            if (!a.fin && (int64_t)RL * (k + 1) > Tc) keep_words((int64_t)RL * k + E * lane - Tc, hrow[k]);
            double c0[E], e0[E];
            ring_row(k, hrow[k], c0, e0);
        }
    }

    // phase-C stores of a lane's chunk (issued one segment late)
    auto store_chunk = [&](int64_t c0, const double (&own)[SC], const bool (&abv)[SC]) {
        if (vec_st && c0 + SC <= Tc) {
            const int64_t gi = row_off + c0;
#pragma unroll
            for (int e = 0; e < SC; e += 2) {
                if (a.smooth) *reinterpret_cast<double2*>(a.smooth + gi + e) = make_double2(own[e], own[e + 1]);
                if (a.corr_scaled)
                    *reinterpret_cast<double2*>(a.corr_scaled + gi + e) = make_double2(own[e] * scale, own[e + 1] * scale);
            }
            if (a.above) {
                if constexpr (SC == 4) {
                    *reinterpret_cast<uint32_t*>(a.above + gi) =
                        (uint32_t)abv[0] | ((uint32_t)abv[1] << 8) | ((uint32_t)abv[2] << 16) | ((uint32_t)abv[3] << 24);
                } else {
#pragma unroll
                    for (int e = 0; e < SC; ++e) a.above[gi + e] = (uint8_t)abv[e];
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < SC; ++e) {
                const int64_t p = c0 + e;
                if (p < Tc) {
                    const int64_t gi = row_off + p;
                    if (a.smooth) a.smooth[gi] = own[e];
                    if (a.corr_scaled) a.corr_scaled[gi] = own[e] * scale;
                    if (a.above) a.above[gi] = (uint8_t)abv[e];
                }
            }
        }
    };
    bool pend = false;                                             // a chunk's stores deferred
    int64_t pend_c0 = 0;
    double pend_own[SC];
    bool pend_abv[SC];

    for (int g = 0; g < nseg; ++g) {
        const int s0 = SEG * g;                                    // chunk index of the segment's start
        const int k0 = g * RPS, k1 = min(nrows, (g + 1) * RPS);
        int32_t rows[RPS][NB][E];                                  // the segment's rows, taken at once
#pragma unroll
        for (int j = 0; j < RPS; ++j)
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) rows[j][t][e] = nx[j][t][e];
        if (g + 1 < nseg) load_seg(g + 1);
        if (pend) { store_chunk(pend_c0, pend_own, pend_abv); pend = false; }
        // ---------------- phase A: metric rows of the segment (stores of the metric arrays) ----
#pragma unroll
        for (int j = 0; j < RPS; ++j) {
            const int kc = k0 + j;                                 // chunk row; virtual row kc + HR
            if (kc >= k1) break;
            const int k = kc + HR;
            const int i0 = RL * kc + E * lane;                     // chunk index of element 0
            const int32_t (&cur)[NB][E] = rows[j];
            if (!a.fin && (int64_t)RL * (kc + 1) + H > Tc) keep_words((int64_t)i0 + H - Tc, cur);
            double c0[E], e0[E];
            ring_row(k, cur, c0, e0);
            const int s1 = (k + NR - MW) % NR, s2 = (k + NR - 2 * MW) % NR, s3 = (k + NR - 3 * MW) % NR;
            // every lag row exists (k >= 3 MW).  STEADY rows (every sample past the fill phase and inside
            // the chunk: wave-uniform): no tap selects, no store guards - the same values
            auto metric = [&](auto steady_c) {
                constexpr bool STEADY = decltype(steady_c)::value;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const double c1 = hac(s1, e), c2 = hac(s2, e);
                    const double e1 = hae(s1, e), e2 = hae(s2, e), e3 = hae(s3, e);
                    const int i = i0 + e;
                    double ct, et;
                    if constexpr (STEADY) {
                        ct = 0.0 + ((c0[e] - c1) + (c1 - c2));                          // minn_rtl.py:696
                        et = 0.0 + (((e0[e] - e1) + (e1 - e2)) + (e2 - e3));            // :697-701
                    } else {
                        // the reference's registers hold 0 before their first valid sample (absolute index)
                        const double cr_ = (i >= t1) ? c0[e] - c1 : 0.0;
                        const double cp_ = (i >= t2) ? c1 - c2 : 0.0;
                        const double er_ = (i >= t1) ? e0[e] - e1 : 0.0;
                        const double ep_ = (i >= t2) ? e1 - e2 : 0.0;
                        const double ep2 = (i >= t3) ? e2 - e3 : 0.0;
                        ct = 0.0 + (cr_ + cp_);
                        et = 0.0 + ((er_ + ep_) + ep2);
                    }
                    const double cpos = ct > 0.0 ? ct : 0.0;               // :704
                    const double es = (a.thr_value == 0.0) ? 0.0 : et * a.thr_value;   // :718-721
                    const int li = i - s0;
                    hcp[seg_at(li)] = cpos;
                    hes[seg_at(li)] = es;
                    if (STEADY || i < Tc) {
                        const int64_t gi = row_off + i;
                        if (a.corr_total) a.corr_total[gi] = ct;
                        if (a.corr_positive) a.corr_positive[gi] = cpos;
                        if (a.energy_total) a.energy_total[gi] = et;
                        if (a.energy_scaled) a.energy_scaled[gi] = es;
                        if (a.mvalid) a.mvalid[gi] = (uint8_t)(i >= t3);
                    }
                }
            };
            if (RL * kc >= t3 && (int64_t)RL * (kc + 1) <= Tc) metric(std::true_type{});
            else metric(std::false_type{});
        }
        const int c0 = s0 + SC * lane;                             // first sample of my chunk
        const int send = (int)min(Tc, (int64_t)s0 + SEG);
        bool abv[SC];
        double cp8[SC], own[SC];
        if (walk) {
            // ---------- phase B (RTL floor mode): one walker lane per stream of the workgroup -----
            lds_barrier();
            if (w == 0 && lane < wpb && (int64_t)blockIdx.x * wpb + lane < a.B) {
                const double* wcp = rcm + wave_dbl * lane + 2 * NR * E * 64;
                double* wes = const_cast<double*>(wcp) + SEG_PAD;
                double* wst = rcm + wave_dbl * lane + hst_off;
                const int n = send - s0;
                const int v0 = max(0, min(n, t3 - s0));
                double sv = wst[0];
                long long siv = __double_as_longlong(wst[1]);
                rtl_walk<2>(wcp, wes, n, v0, inv, scale, a.shift, sv, siv);
                wst[0] = sv; wst[1] = __longlong_as_double(siv);
            }
            lds_barrier();
            sm = hst[0]; si = __double_as_longlong(hst[1]);
#pragma unroll
            for (int e = 0; e < SC; ++e) {
                const int p = c0 + e;
                const int at = seg_at(SC * lane + e);
                cp8[e] = hcp[at];
                const long long v = __double_as_longlong(hes[at]);
                own[e] = __longlong_as_double(v & 0x7fffffffffffffffll);
                abv[e] = p < Tc && v < 0;
            }
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---------- phase B (float IIR): segment-parallel, lane j = chunk j -----------------
            double cv[SC];
            bool upd[SC];
#pragma unroll
            for (int e = 0; e < SC; ++e) {
                const int p = c0 + e;
                upd[e] = p >= t3 && p < Tc;
                cv[e] = hcp[seg_at(SC * lane + e)];
            }
            if (smode == 1) {                                          // shift 0: s = c (no chain)
                // the state is held where the metric is not valid yet: the carried state
#pragma unroll
                for (int e = 0; e < SC; ++e) own[e] = upd[e] ? cv[e] : sm;
                if (send - 1 >= t3) sm = hcp[seg_at(send - 1 - s0)];
            } else {
                const bool interior = s0 >= t3 && (int64_t)s0 + SEG <= Tc && a.shift <= 14;
                long long rounds = 0;
                rtl_float_seg(cv, upd, lane, interior, inv, keep, sm, own, rounds);
            }
            // ---------- phase C: threshold (chunk layout) -----------------------------------------
#pragma unroll
            for (int e = 0; e < SC; ++e) {
                const int at = seg_at(SC * lane + e);
                cp8[e] = cv[e];
                abv[e] = upd[e] && (own[e] * scale >= hes[at]);              // minn_rtl.py:717-722
            }
        }
        // ---------- phase C: gate; the chunk's stores wait for the next segment's row take -----------
        pend = true;
        pend_c0 = c0;
#pragma unroll
        for (int e = 0; e < SC; ++e) { pend_own[e] = own[e]; pend_abv[e] = abv[e]; }
        if (a.detect && send > t3) {
            double none[SC];
#pragma unroll
            for (int e = 0; e < SC; ++e) none[e] = 0.0;
            gate.row_flags(lane, g + KOFF, c0 + GO, Tg, abv, cp8, none, none, none);
        }
        __builtin_amdgcn_wave_barrier();                               // LDS reuse by the next segment
    }
    if (pend) store_chunk(pend_c0, pend_own, pend_abv);

    int64_t carry_p1 = h.carry_p1, ev_start = h.ev_start, bidx = h.bidx;
    int open = h.gate_open;
    double bpm = h.bpm;
    if (a.detect) {
        // the lanes' bests went into the carried peak row by row (last maximum, >=)
        gate.save(carry_p1, open, ev_start, bidx);
        bpm = gate.bpm;
        if (lane == 0) {
            a.n_ev[b] = gate.n_ev;
            a.open_start[b] = open ? ev_start : -1;                // never closed at the end of the stream
        }
    }
    if (a.fin) {                                                     // fresh again: zero history, zero header
        for (int j = 4 * lane; j < NB * H; j += 256) *reinterpret_cast<int4*>(hout + j) = make_int4(0, 0, 0, 0);
    }
    if (lane == 0) {
        RtlChunkHdr o{};
        o.parity = par ^ 1;
        if (!a.fin) {
            o.n_seen = h.n_seen + Tc;
            o.carry_p1 = carry_p1; o.ev_start = open ? ev_start : 0; o.bidx = open ? bidx : 0;
            o.bpm = open ? bpm : 0.0;
            o.gate_open = open;
            o.sm = sm; o.si = si; o.wide = wide ? 1 : 0;
        }
        *hdr = o;
    }
}

template <int E, int MW, int NB, bool CP>
int rtl_chunk_launch_k(const RtlChunkArgs& a, hipStream_t st) {
    constexpr size_t per_wave = rtl_chunk_wave_lds(E, MW, NB);
    int wpb = XR / 64;                                       // waves (streams) per workgroup
    while (wpb > 1 && per_wave * wpb > 64 * 1024) wpb >>= 1;
    static_assert(per_wave <= 64 * 1024, "one wave's rings fit the default LDS limit");
    const int64_t nblk = (a.B + wpb - 1) / wpb;
    if (nblk > 0x7fffffffll) return OFS_EINVAL;
    hipLaunchKernelGGL((rtl_chunk_kernel<E, MW, NB, CP>), dim3((unsigned)nblk), dim3(64 * wpb), per_wave * wpb, st, a);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}
template <int E, int MW>
int rtl_chunk_launch(int fmt, int nb, const RtlChunkArgs& a, hipStream_t st) {
    if (fmt == OFS_CP12)
        return nb == 1 ? rtl_chunk_launch_k<E, MW, 1, true>(a, st) : rtl_chunk_launch_k<E, MW, 2, true>(a, st);
    return nb == 1 ? rtl_chunk_launch_k<E, MW, 1, false>(a, st) : rtl_chunk_launch_k<E, MW, 2, false>(a, st);
}

// the table of ofs_rtl_exact_plan: Q = 64·E·MW
bool rtl_chunk_shape_ok(int n_br, int Q) {
    return (n_br == 1 || n_br == 2) && (Q == 64 || Q == 128 || Q == 256 || Q == 512);
}

}  // namespace

extern "C" {

int64_t ofs_rtl_chunk_state_bytes(int32_t n_br, int32_t Q) {
    if (!rtl_chunk_shape_ok(n_br, Q)) return OFS_EINVAL;
    return (int64_t)sizeof(RtlChunkHdr) + (int64_t)2 * n_br * 3 * Q * (int64_t)sizeof(int32_t);
}

int64_t ofs_rtl_chunk_max_samples(int32_t n_br, int32_t Q) {
    if (!rtl_chunk_shape_ok(n_br, Q)) return OFS_EINVAL;
    return ((int64_t)1 << 21) / n_br - 3 * (int64_t)Q;           // (Tc + 3Q)·n_br <= 2^21: prefixes < 2^53
}

int32_t ofs_minn_rtl_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc, int32_t Q,
                           int32_t smooth_shift, int32_t smooth_mode, int64_t threshold_value,
                           int32_t threshold_frac_bits, void* state,
                           double* corr_total, double* corr_positive, double* smooth_metric, double* energy_total,
                           double* corr_scaled, double* energy_scaled, uint8_t* metric_valid, uint8_t* above_threshold,
                           int32_t detect, int32_t hysteresis, int32_t timing_offset, int32_t max_events,
                           int32_t* n_events, int64_t* events, int64_t* open_gate_start, int32_t final, void* stream) {
    if ((in_fmt != OFS_CI16 && in_fmt != OFS_CP12) || !rtl_chunk_shape_ok(n_br, Q) ||
        ofs_chunk::chunk_args_bad(B, Tc, ofs_rtl_chunk_max_samples(n_br, Q), final, state, x))
        return OFS_EINVAL;
    if (smooth_shift < 0 || smooth_shift > 62 || threshold_frac_bits < 0 || threshold_frac_bits > 62 ||
        (smooth_mode != 0 && smooth_mode != 1) || hysteresis < 0 || hysteresis > OFS_RTL_CHUNK_MAX_HYSTERESIS)
        return OFS_EINVAL;
    if (detect && (OFS_MISSING(n_events, B) || OFS_MISSING(open_gate_start, B) || max_events < 0 ||
                   (max_events > 0 && OFS_MISSING(events, B))))
        return OFS_EINVAL;
    if (B == 0) return OFS_OK;
    RtlChunkArgs a{};
    a.x = x; a.B = B; a.Tc = Tc; a.state = reinterpret_cast<uint8_t*>(state);
    a.state_bytes = ofs_rtl_chunk_state_bytes(n_br, Q);
    a.shift = smooth_shift; a.smooth_mode = smooth_mode; a.frac_bits = threshold_frac_bits;
    a.thr_value = (double)threshold_value;
    a.corr_total = corr_total; a.corr_positive = corr_positive; a.smooth = smooth_metric;
    a.energy_total = energy_total; a.corr_scaled = corr_scaled; a.energy_scaled = energy_scaled;
    a.mvalid = metric_valid; a.above = above_threshold;
    a.detect = detect; a.hyst = hysteresis; a.toff = timing_offset; a.max_ev = max_events;
    a.n_ev = n_events; a.ev = events; a.open_start = open_gate_start; a.fin = final != 0;
    hipStream_t st = (hipStream_t)stream;
    switch (Q) {
        case 64: return rtl_chunk_launch<1, 1>(in_fmt, n_br, a, st);
        case 128: return rtl_chunk_launch<1, 2>(in_fmt, n_br, a, st);
        case 256: return rtl_chunk_launch<2, 2>(in_fmt, n_br, a, st);
        case 512: return rtl_chunk_launch<4, 2>(in_fmt, n_br, a, st);
    }
    return OFS_EINVAL;
}

}  // extern "C"
