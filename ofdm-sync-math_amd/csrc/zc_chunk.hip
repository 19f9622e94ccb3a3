// zc_chunk.hip — resumable form of the zc_v2 CFAR + gate (ofs_zc_detect_chunk): one call takes the
// next Tc magnitudes of B streams and returns the CFAR arrays of those samples, the gate mask and the
// gate events that closed among them; what the next call needs stays in a caller-owned state buffer.
//
// The kernel is the register-staged form of zc_cfar_kernel (zc_cfar.hip) - walker wave, helper waves
// one chunk behind, one LDS-only barrier per 128-sample chunk.  What the two kernels have in common
// is in zc_tiles.h and used by both: the geometry, the walker's recursion, the gate record, the CFAR
// decision, the event record, the row stores and the barrier (each checked to leave all four kernels'
// instruction text as it was).  Two parts have a sibling in zc_cfar_kernel that
// is written out there too, because they differ: the load / stage pair (here c[i - W] comes from the
// ring) and the loops of the flag pass (tile slots rotated, not divided; valid from vfrom[j], not W).
// A change to either is looked at on both sides.  What differs:
//
// HISTORY.  The state keeps the last W magnitudes as a ring indexed by the absolute sample: c[n] lives
// in slot n mod W, which is the slot that held c[n - W].  The walker's c[i - W] tile reads the ring
// while n0 + i - W lies before the call (i < W) and the chunk itself afterwards.  A fresh stream's ring
// is zeros and (acc + c) - 0.0 == acc + c bit for bit, so the recursion needs no "window not yet full"
// branch at all; only metric_valid = n >= W is decided per stream on n.  The ring is written back after
// the main loop (the last min(W, Tc) magnitudes of the call), behind a full barrier: every read of the
// old history has been consumed by then.  With Tc < W a call replaces Tc slots and keeps the rest.
//
// GATE.  One row machine for every hysteresis (the one-shot call has a closed form for Hp >= 64 and a
// sequential kernel below): with Hp = max(H, 1) an open gate closes at the first non-above sample n
// with n - (last above sample) = Hp.  Per 64-sample row the wave walks the ballot of the above flags
// with scalar bit operations - runs of above samples move last_above, the first gap that reaches Hp
// closes - and does one wave maximum per gate segment of the row (first maximum, strict >, the opening
// sample first), so a row with k closes costs k + 1 reductions and a quiet chunk none.  gate_mask marks
// (gate_start, gate_end].  The machine's state (open, gate_start, peak, last above sample) is absolute
// and is carried in the state header, so a gate stays open over any number of calls.
//
// State of one stream (ofs_zc_chunk_state_bytes = 64 + 8 W rounded up to 16, all-zero = fresh):
//   ZcChunkHdr (64 B), then the ring double[W] (the next sample's slot is n_seen mod W).  A state row is read and written only by the workgroup
//   that owns the stream.
#include "chunk_state.h"
#include "ofdmsync.h"
#include "zc_tiles.h"

using namespace ofs;

namespace {

constexpr int ZS = ZS_REG, ZH = ZH_REG;   // streams per workgroup (walker lanes), helper waves
constexpr int NJ = (ZS + ZH - 1) / ZH;   // streams per helper wave

struct ZcChunkHdr {
    double acc;                   // running sum after the last sample
    int64_t n_seen;               // samples of this stream consumed by earlier calls
    int64_t last_above;           // open gate: its last above-threshold sample (absolute)
    int64_t gs, pk;               // open gate: its start, its peak so far (absolute)
    double pv;                    // open gate: corr_mag at that peak
    int32_t open, pad0;
    int64_t pad;
};
static_assert(sizeof(ZcChunkHdr) == 64, "state header");

struct ZcChunkArgs {
    const double* mag; int64_t ld, B, Tc;
    uint8_t* state; int64_t state_bytes;
    int W, tcm;                   // tcm = Tc mod W
    double tv, scale, minmag; int reflen, Hp;
    double* local_sum; double* corr_scaled; double* thresh_scaled;
    uint8_t* above; uint8_t* valid; uint8_t* gate_mask;
    int max_ev; int32_t* n_ev; int64_t* ev; double* ev_v; int64_t* open_start;
    int fin;
};

// diagnostic builds (-DOFS_ZC_CHUNK_TIMING=1, tools/zc_chunk_phase.py): s_memtime ticks per role and
// phase, summed over the waves of the role: [0..6] walker wave, [8..14] helper waves;
// phase 0 entry (header reads, first tiles), 1 tile loads + staging, 2 chain / helper work, 3 chunk barrier,
// 4 the full barrier after the loop (drains the wave's memory operations), 5 ring write-back + second full
// barrier, 6 headers and counts
#ifndef OFS_ZC_CHUNK_TIMING
#define OFS_ZC_CHUNK_TIMING 0
#endif
#if OFS_ZC_CHUNK_TIMING
__device__ unsigned long long zcc_prof[16];
#define YC_T(i)                                                                                      \
    if (lane == 0) { const long long t_ = __builtin_amdgcn_s_memtime(); tacc[i] += t_ - tprev; tprev = t_; }
#else
#define YC_T(i)
#endif

__global__ __launch_bounds__(64 * (1 + ZH))
void zc_chunk_kernel(ZcChunkArgs a) {
#pragma clang fp contract(off)
#if OFS_ZC_CHUNK_TIMING
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tprev = __builtin_amdgcn_s_memtime();
#endif
    __shared__ double tc[3][ZS][ZP];      // c
    __shared__ double to[2][ZS][ZP];      // c[n - W]: ring, then the chunk itself
    __shared__ double ta[2][ZS][ZP];      // running sum after sample i
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // 0 = walker, 1..ZH = helpers
    const int hi = wv - 1;
    const int64_t b0 = (int64_t)blockIdx.x * ZS;
    const int ns = (int)min((int64_t)ZS, a.B - b0);          // streams of this workgroup
    const int64_t Tc = a.Tc;
    const int64_t nch = (Tc + ZC - 1) / ZC;
    const int W = a.W;
    auto hdr_of = [&](int s) { return reinterpret_cast<ZcChunkHdr*>(a.state + (b0 + s) * a.state_bytes); };
    auto ring_of = [&](int s) { return reinterpret_cast<double*>(a.state + (b0 + s) * a.state_bytes + sizeof(ZcChunkHdr)); };

    // loader = the walker wave (it issues no global stores in the main loop)
    // ring slot of a stream's next sample: n_seen mod W (unsigned, so always inside the ring)
    auto slot_of = [&](int s) {
        return __builtin_amdgcn_readfirstlane((int)((uint64_t)hdr_of(s)->n_seen % (uint64_t)W));
    };
    int r0[ZS];                                               // ring slot of the call's first sample
    const double* cw = a.mag + b0 * a.ld;
    if (wv == 0) {
#pragma unroll
        for (int s = 0; s < ZS; ++s) r0[s] = s < ns ? slot_of(s) : 0;
    }
    // load / stage: zc_cfar_kernel's register pair with the ring as the source of c[i - W] for i < W
    double pc[ZR][ZS], po[ZR][ZS];
    auto load = [&](int64_t q) {
#pragma unroll
        for (int rr = 0; rr < ZR; ++rr) {
            const int64_t i = q * ZC + 64 * rr + lane;
#pragma unroll
            for (int s = 0; s < ZS; ++s) {
                const bool ok = s < ns && i < Tc;
                pc[rr][s] = ok ? cw[s * a.ld + i] : 0.0;
                double o = 0.0;
                if (ok) {
                    if (i >= W) {
                        o = cw[s * a.ld + i - W];
                    } else {
                        int k = r0[s] + (int)i;
                        k = k >= W ? k - W : k;
                        o = ring_of(s)[k];
                    }
                }
                po[rr][s] = o;
            }
        }
    };
    auto stage = [&](int q3, int q2) {                        // tile slots of the chunk: q mod 3, q mod 2
#pragma unroll
        for (int rr = 0; rr < ZR; ++rr)
#pragma unroll
            for (int s = 0; s < ZS; ++s) {
                tc[q3][s][64 * rr + lane] = pc[rr][s];
                to[q2][s][64 * rr + lane] = po[rr][s];
            }
    };

    // helpers: the gate machines and sample counts of their streams hi, hi + ZH, ...
    ZcGate g[NJ];
    int64_t n0[NJ], vfrom[NJ];                                // first sample's absolute index; first valid i
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        g[j].last_above = 0; g[j].gs = 0; g[j].pk = 0; g[j].pv = 0.0; g[j].open = 0; g[j].nev = 0;
        n0[j] = 0; vfrom[j] = 0;
        const int s = hi + ZH * j;
        if (wv >= 1 && s < ns) {
            const ZcChunkHdr h = *hdr_of(s);
            g[j].last_above = h.last_above; g[j].gs = h.gs; g[j].pk = h.pk; g[j].pv = h.pv; g[j].open = h.open != 0;
            n0[j] = h.n_seen;
            vfrom[j] = h.n_seen >= W ? 0 : W - h.n_seen;
        }
    }
    double acc = 0.0;                                         // walker lane s < ns: stream b0 + s
    if (wv == 0 && lane < ns) acc = hdr_of(lane)->acc;

    if (wv == 0) {
        load(0);
        stage(0, 0);
        if (1 < nch) load(1);
    }
    zc_lds_barrier();
    YC_T(0)
    int c3 = 0;                                               // q mod 3, rotated (no 64-bit division per chunk)
    for (int64_t q = 0; q <= nch; ++q) {
        const int c2 = (int)(q & 1);
        const int n3 = c3 == 2 ? 0 : c3 + 1, p3 = c3 == 0 ? 2 : c3 - 1;   // (q + 1) mod 3, (q - 1) mod 3
        if (wv == 0) {
            if (q + 1 < nch) stage(n3, c2 ^ 1);               // loaded during the previous chunk
            if (q + 2 < nch) load(q + 2);
            YC_T(1)
            // ---- walker: the exact left-to-right recursion of RunningSum.step ----
            if (q < nch && lane < ZS) {
                const int cnt = (int)min((int64_t)ZC, Tc - q * ZC);
                const double* x = tc[c3][lane];
                const double* o = to[c2][lane];
                double* r = ta[c2][lane];
                if (cnt == ZC) {
                    zc_walk_chunk<ZC, false>(x, o, r, acc);
                } else {
                    for (int u = 0; u < cnt; ++u) { acc = (acc + x[u]) - o[u]; r[u] = acc; }
                }
            }
            YC_T(2)
        } else if (q >= 1) {
            // ---- helpers: chunk q-1 (flags, stores, gate) ----
            const int64_t qc = q - 1;
            const int q3 = p3, q2 = c2 ^ 1;
            // pass 1: the flags of every (row, stream) of this wave.  A chunk with no above sample and
            // no open gate needs no gate logic: its gate_mask rows are 0.  (The loops are zc_cfar_kernel's
            // with the tile slots rotated and valid = i >= vfrom[j]; as one function they changed all four
            // kernels by 1 - 5 instructions, see there.)
            bool quiet = true;
            double cv[ZR][NJ], lv[ZR][NJ];
            uint64_t am[ZR][NJ];
#pragma unroll
            for (int rr = 0; rr < ZR; ++rr)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int s = hi + ZH * j;
                    const int sr = s < ns ? s : 0;
                    cv[rr][j] = tc[q3][sr][64 * rr + lane];
                    lv[rr][j] = ta[q2][sr][64 * rr + lane];
                }
#pragma unroll
            for (int rr = 0; rr < ZR; ++rr) {
                const int64_t i = qc * ZC + 64 * rr + lane;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int s = hi + ZH * j;
                    const bool vd = (i < Tc) & (i >= vfrom[j]);
                    am[rr][j] = zc_above(a, (s < ns) & vd, cv[rr][j], lv[rr][j]);
                    if (am[rr][j]) quiet = false;
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (g[j].open) quiet = false;
#pragma unroll
            for (int rr = 0; rr < ZR; ++rr) {
                const int64_t i0 = qc * ZC + 64 * rr;             // call-local index of the row's lane 0
                const int64_t i = i0 + lane;
                const bool inb = i < Tc;
                const int cnt = (int)min((int64_t)64, Tc - i0);   // samples of the row (<= 0: none)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int s = hi + ZH * j;
                    if (s >= ns) break;
                    const double c = cv[rr][j];
                    const double ls = lv[rr][j];
                    const double cs = c * a.scale, th = ls * a.tv;
                    const uint64_t abm = am[rr][j];
                    const bool vd = inb && i >= vfrom[j];
                    const int64_t o = (b0 + s) * Tc + i;
                    uint64_t mk = 0;                              // gate_mask bits of the row
                    if (!quiet && cnt > 0) {
                        ZcGate& G = g[j];
                        const int64_t base = n0[j] + i0;          // absolute index of the row's lane 0
                        int pos = 0;
                        while (pos < cnt) {
                            if (G.open) {
                                // first non-above sample of [pos, cnt) whose gap to the last above sample is Hp
                                int p = pos, cl = -1;
                                for (;;) {
                                    const uint64_t rest = p < 64 ? (abm >> p) : 0;
                                    const int na = rest ? p + (int)__builtin_ctzll(rest) : 64;
                                    const int64_t nc = G.last_above + a.Hp;
                                    const int lim = na < cnt ? na : cnt;          // non-above samples [p, lim)
                                    if (nc < base + lim) { cl = (int)(nc - base); break; }
                                    if (na >= cnt) break;
                                    const uint64_t run = ~(abm >> na);           // the run of above samples from na
                                    const int r = run ? (int)__builtin_ctzll(run) : 64;
                                    G.last_above = base + na + r - 1;
                                    p = na + r;
                                }
                                const int e = cl >= 0 ? cl : cnt - 1;            // the gate's samples here: [pos, e]
                                mk |= (e >= 63 ? ~0ull : ((1ull << (e + 1)) - 1)) & ~((1ull << pos) - 1);
                                // zc_peak of zc_tiles.h written out: calling it here folds one scalar sign
                                // extension (8572 -> 8571 instructions) and a Tc = 1024 push then measured
                                // 0.0772 ms against the parent's 0.0765 - 0.0767 (profiles/zc_chunked_ab.jsonl)
                                const bool in = lane >= pos && lane <= e;
                                const double m = wave_max(in ? c : -__builtin_huge_val());
                                if (m > G.pv) {
                                    const uint64_t at = __ballot(in && c == m);
                                    G.pv = m; G.pk = base + __builtin_ctzll(at);
                                }
                                if (cl >= 0) {
                                    ZC_EVENT(a, G, b0 + s, base + cl, lane);
                                    G.open = 0; G.pv = 0.0;
                                    pos = cl + 1;
                                } else {
                                    pos = cnt;
                                }
                            } else {
                                const uint64_t rest = abm >> pos;                // pos < cnt <= 64
                                if (!rest) break;
                                const int op = pos + (int)__builtin_ctzll(rest);
                                G.open = 1; G.gs = base + op; G.pk = G.gs; G.last_above = G.gs;
                                G.pv = readlane(c, op);
                                pos = op + 1;
                            }
                        }
                    }
                    if (inb) zc_store(a, o, ls, cs, th, (abm >> lane) & 1, vd, (mk >> lane) & 1);
                }
            }
            YC_T(2)
        }
        zc_lds_barrier();
        YC_T(3)
        c3 = n3;
    }

    // ---- the ring: the last min(W, Tc) magnitudes of the call (zeros on a final call).  Every read of
    // the old history was consumed before the loop's last barrier; the full barrier also completes the
    // header reads of every wave before any header write below ----
    __syncthreads();
    YC_T(4)
    for (int s = 0; s < ns; ++s) {
        double* ring = ring_of(s);
        if (a.fin) {
            for (int k = (int)threadIdx.x; k < W; k += 64 * (1 + ZH)) ring[k] = 0.0;
        } else {
            const int rp = slot_of(s);
            const int m = (int)min((int64_t)W, Tc);
            int start = Tc > W ? rp + a.tcm : rp;                 // slot of sample Tc - m
            start = start >= W ? start - W : start;
            const double* src = cw + s * a.ld + (Tc - m);
            for (int k = (int)threadIdx.x; k < m; k += 64 * (1 + ZH)) {
                int slot = start + k;
                slot = slot >= W ? slot - W : slot;
                ring[slot] = src[k];
            }
        }
    }
    __syncthreads();
    YC_T(5)

    // ---- headers, counts, open gates ----
    if (wv == 0) {
        if (lane < ns) hdr_of(lane)->acc = a.fin ? 0.0 : acc;
    } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int s = hi + ZH * j;
            if (s >= ns) break;
            ZcGate& G = g[j];
            const int64_t b = b0 + s;
            if (lane == 0) a.open_start[b] = G.open ? G.gs : -1;
            if (a.fin && G.open) {                             // closes at the stream's sample count
                ZC_EVENT(a, G, b, n0[j] + Tc, lane);
                // gate_mask[gate_start:n] of the reference: the start sample, where it lies in this call
                if (lane == 0 && a.gate_mask && G.gs >= n0[j] && G.gs - n0[j] < Tc)
                    zc_st(&a.gate_mask[b * Tc + (G.gs - n0[j])], (uint8_t)1);
            }
            if (lane == 0) {
                a.n_ev[b] = G.nev;
                ZcChunkHdr* h = hdr_of(s);
                const bool keep = !a.fin;
                const bool op = keep && G.open;
                h->n_seen = keep ? n0[j] + Tc : 0;
                h->last_above = op ? G.last_above : 0;
                h->gs = op ? G.gs : 0;
                h->pk = op ? G.pk : 0;
                h->pv = op ? G.pv : 0.0;
                h->open = op ? 1 : 0;
                h->pad0 = 0;
                h->pad = 0;
            }
        }
    }
#if OFS_ZC_CHUNK_TIMING
    YC_T(6)
    if (lane == 0)
        for (int i = 0; i < 7; ++i) atomicAdd(&zcc_prof[(wv == 0 ? 0 : 8) + i], (unsigned long long)tacc[i]);
#endif
}

}  // namespace

extern "C" {

int64_t ofs_zc_chunk_state_bytes(int32_t window_size) {
    if (window_size < 0 || window_size > OFS_ZC_CHUNK_MAX_WINDOW) return OFS_EINVAL;
    const int64_t W = window_size > 1 ? window_size : 1;
    return ((int64_t)sizeof(ZcChunkHdr) + 8 * W + 15) / 16 * 16;
}

int32_t ofs_zc_detect_chunk(const double* corr_mag, int64_t ld_mag, int64_t B, int64_t Tc,
                            int32_t window_size, int64_t thresh_value, int32_t thresh_frac_bits,
                            double min_corr_mag, int32_t reference_length, int32_t hysteresis,
                            void* state,
                            double* local_sum, double* corr_scaled, double* thresh_scaled,
                            uint8_t* above_threshold, uint8_t* metric_valid, uint8_t* gate_mask,
                            int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_peak,
                            int64_t* open_gate_start, int32_t final, void* stream) {
    const int64_t sb = ofs_zc_chunk_state_bytes(window_size);
    if (ofs_chunk::chunk_args_bad(B, Tc, INT64_MAX, final, state, corr_mag) || (B > 1 && ld_mag < Tc) || sb < 0 ||
        thresh_frac_bits < 0 || thresh_frac_bits > 62 || hysteresis < 0 ||
        hysteresis > OFS_ZC_CHUNK_MAX_HYSTERESIS || max_events < 0)
        return OFS_EINVAL;
    if ((reinterpret_cast<uintptr_t>(corr_mag) & 7) != 0 ||
        OFS_MISSING(n_events, B) || OFS_MISSING(open_gate_start, B) ||
        (max_events > 0 && B > 0 && (!ev_int || !ev_peak)))
        return OFS_EINVAL;
    if (B == 0) return OFS_OK;
    const int64_t nblk = (B + ZS - 1) / ZS;
    if (nblk > 0x7fffffffll) return OFS_EINVAL;
    ZcChunkArgs a{};
    a.mag = corr_mag; a.ld = ld_mag; a.B = B; a.Tc = Tc;
    a.state = reinterpret_cast<uint8_t*>(state); a.state_bytes = sb;
    a.W = window_size > 1 ? window_size : 1;                   // RunningSum: max(1, W)
    a.tcm = (int)(Tc % a.W);
    a.tv = (double)thresh_value; a.scale = (double)(1ll << thresh_frac_bits); a.minmag = min_corr_mag;
    a.reflen = reference_length; a.Hp = hysteresis > 1 ? hysteresis : 1;
    a.local_sum = local_sum; a.corr_scaled = corr_scaled; a.thresh_scaled = thresh_scaled;
    a.above = above_threshold; a.valid = metric_valid; a.gate_mask = gate_mask;
    a.max_ev = max_events; a.n_ev = n_events; a.ev = max_events > 0 ? ev_int : nullptr;
    a.ev_v = max_events > 0 ? ev_peak : nullptr;
    a.open_start = open_gate_start; a.fin = final != 0;
    hipLaunchKernelGGL(zc_chunk_kernel, dim3((unsigned)nblk), dim3(64 * (1 + ZH)), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}

#if OFS_ZC_CHUNK_TIMING
// per-role, per-phase cycle totals of zc_chunk_kernel since the last call (diagnostic builds)
int ofs_zc_chunk_prof(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(zcc_prof), sizeof(zcc_prof)) != hipSuccess) return -1;
    const unsigned long long z[16] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(zcc_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
