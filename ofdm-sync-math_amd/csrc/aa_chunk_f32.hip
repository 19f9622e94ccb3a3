// aa_chunk_f32.hip — resumable form of the fp32 [A][A] fast path (aa_fast_kernel / aa_stream_kernel,
// complex64 in, fp32 out) for streams that arrive in chunks (ofs_aa_detect_chunk_f32): one call takes
// the next Tc samples of B streams and returns their P, R, M, valid and the gate events that closed
// among them; what the next call needs stays in a caller-owned state buffer on the device.
//
// THE SAME ARITHMETIC, CONTINUED.  The one-shot kernels compute, in rows of RL = 128 samples aligned to
// the start of the stream,
//     P[n] = suffix(row k-MR, after n) + (float)(C[k] - C[k-MR+1]) + prefix(row k, up to n)
// with fp32 in-row partials and C the fp64 running sum of the row totals since sample 0.  Neither the
// partials nor C are exact, so a call cannot restart them: it has to produce the very same fp32 and
// fp64 values.  State form (a) of DESIGN §4.3f: per stream the state keeps the raw samples from the
// start of absolute row k0 - 2·MR up to n_seen (k0 = n_seen / 128: 2L + n_seen % 128 samples per antenna)
// and the fp64 base C[k0 - MR].  A call runs the one-shot row loop over the virtual stream
// [history | chunk], whose rows are the absolute rows k0 - 2·MR, k0 - 2·MR + 1, ...:
//   rows k0 - 2·MR .. k0 - MR - 1   refill the lag ring (raw samples only);
//   rows k0 - MR .. k0 - 1          are replayed from C[k0 - MR]: the same products, the same scans, the
//                                   same sequence cb[so] = C + t; C += t - they refill the suffix ring
//                                   and the base ring, store nothing and are not shown to the gate;
//   rows k0 ..                      are computed, and the positions >= n_seen are stored and gated.
// Row k0 is recomputed whole (its first n_seen % 128 samples are in the history); a row that the chunk
// leaves incomplete is computed with zeros after its last sample, which no output at or before that
// sample depends on (prefix scans), and is computed again by the call that completes it.  Rows of
// absolute index < MR take the one-shot kernels' no-lag form (P = M = +0.0 whatever the samples are),
// rows of negative index (a young stream's history) do not exist and are skipped.
//
// GATE.  AaRowGate in its ABS form, as in aa_chunk.hip: call-local gate coordinates
// g = virtual position + RL·KOFF, KOFF = ceil(max(H, 1) / RL) rows.  Unlike there, the first row shown to
// the gate starts before n_seen: its positions < n_seen are dead - never above, |P|² = -1 so that they
// never become a peak - and the last above position of an earlier call is loaded only while its gate is
// still open (otherwise its close, which lies before n_seen, would be found a second time).
//
// State of one stream (ofs_aa_chunk_f32_state_bytes = 128 + 2·n_ant·(2L + 128)·8 bytes, all-zero = fresh):
//   AaChunkF32Hdr (128 B), then two history slots [2][n_ant][2L + 128] complex64.  A call reads slot
//   `parity` and writes the other one, so no word is overwritten before it is read.
#include "chunk_state.h"
#include "aa_gate.h"
#include "ofdmsync.h"

using namespace ofs;

namespace {

struct AaChunkF32Hdr {
    int64_t n_seen;                 // samples of this stream consumed by earlier calls
    int64_t carry_p1;               // 1 + absolute index of the last above-threshold sample, 0 = none
    int64_t ev_start, bidx;         // open gate: its start, its peak so far (absolute)
    double bpm, bpr, bpi, bm;       // open gate: |P|², P, M at that peak (fp32 values)
    int32_t gate_open, parity;      // parity: history slot holding the samples since row k0 - 2·MR
    double CR, CI, CE;              // C[k0 - MR]: fp64 sum of the row totals of rows < k0 - MR
    int64_t pad[4];
};
static_assert(sizeof(AaChunkF32Hdr) == 128, "state header");

struct AaChunkF32Args {
    const void* x; int64_t B, Tc;
    uint8_t* state; int64_t state_bytes;
    void* P; void* R; void* M; uint8_t* valid;
    int32_t detect; double thr; int32_t hyst; double fs;
    int32_t max_ev; int32_t* n_ev; int64_t* ev_i; double* ev_r;
    int32_t fin;
};

constexpr int XC = 256;                 // 4 waves = 4 streams per workgroup
constexpr int64_t MAX_TC = (int64_t)1 << 30;    // in-call positions (history + chunk + gate offset) stay below 2^31

// complex values as packed fp32 pairs, products and stores: as in aa_fast.hip, expression for expression
typedef float pf2 __attribute__((ext_vector_type(2)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(8)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
// acc + c·conj(d) = acc + (c.x d.x + c.y d.y, c.y d.x - c.x d.y)
__device__ __forceinline__ pf2 mulc_acc(pf2 c, pf2 d, pf2 acc) {
    acc = __builtin_elementwise_fma(c, d.xx, acc);
    return __builtin_elementwise_fma(c.yx, pf2{d.y, -d.y}, acc);
}

template <int MR, int NA>
__global__ __launch_bounds__(XC) void aa_chunk_f32_kernel(AaChunkF32Args a) {
    constexpr int E = 2;
    constexpr int RL = 64 * E;
    constexpr int L = MR * RL;
    constexpr int HS = 2 * L + RL;                           // samples of one history slot, per antenna
    constexpr int PD = 2;                                    // rows in flight ahead of use
    constexpr int PER = MR > PD ? MR : PD;                   // unroll period (MR, PD powers of 2)
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (XC / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int64_t Tc = a.Tc;
    uint8_t* sp = a.state + b * a.state_bytes;
    AaChunkF32Hdr* hdr = reinterpret_cast<AaChunkF32Hdr*>(sp);
    const AaChunkF32Hdr h = *hdr;
    const int par = h.parity & 1;
    float2* hist = reinterpret_cast<float2*>(sp + sizeof(AaChunkF32Hdr));
    const float2* hin = hist + (int64_t)par * NA * HS;
    float2* hout = hist + (int64_t)(par ^ 1) * NA * HS;
    const float2* xs = reinterpret_cast<const float2*>(a.x) + b * NA * Tc;

    // virtual stream [history | chunk]: virtual row j is the absolute row kb + j
    const int64_t k0 = h.n_seen / RL;
    const int64_t kb = k0 - 2 * MR;
    const int Hn = (int)(h.n_seen - RL * kb);                // history samples: 2L + n_seen % RL
    const int Vend = Hn + (int)Tc;                           // end of the chunk
    // a flush (Tc = 0) closes the open gate from the saved fields alone: no rows
    const int nrows = Tc > 0 ? (Vend + RL - 1) / RL : 0;
    const int jz = kb < 0 ? (int)-kb : 0;                    // rows j < jz lie before the stream: skipped
    const int jf = kb < MR ? (int)(MR - kb) : 0;             // rows j < jf have absolute index < MR: no lag
    const int dk = (int)((h.n_seen + Tc) / RL - k0);         // rows the next call's history starts later
    const int js = dk + MR;                                  // the row whose base C the next call starts from
    const int hshift = RL * dk;

    auto load_row = [&](int j, float2 (&dst)[NA][E]) {       // row j of [history | chunk]
        const int v0 = RL * j + E * lane;
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            if (j < jz) {
                dst[t][0] = make_float2(0.f, 0.f); dst[t][1] = make_float2(0.f, 0.f);
            } else if (RL * (j + 1) <= Hn) {                 // whole row in the history (16-byte aligned)
                const float4 v = *reinterpret_cast<const float4*>(hin + t * HS + v0);
                dst[t][0] = make_float2(v.x, v.y); dst[t][1] = make_float2(v.z, v.w);
            } else if (RL * j >= Hn && RL * (j + 1) <= Vend) {   // whole row in the chunk (8-byte aligned)
                const f4u v = *reinterpret_cast<const f4u*>(xs + t * Tc + (v0 - Hn));
                dst[t][0] = make_float2(v.x, v.y); dst[t][1] = make_float2(v.z, v.w);
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int v = v0 + e;
                    float2 s = make_float2(0.f, 0.f);
                    if (v < Hn) s = hin[t * HS + v];
                    else if (v < Vend) s = xs[t * Tc + (v - Hn)];
                    dst[t][e] = s;
                }
            }
        }
    };
    // the samples from absolute row k0' - 2·MR on become the next call's history (other slot)
    auto store_hist = [&](int j, const float2 (&cur)[NA][E]) {
        if (a.fin || j < jz || RL * (j + 1) <= hshift) return;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int v = RL * j + E * lane + e;
            const int hv = v - hshift;
            if (hv >= 0 && v < Vend) {
#pragma unroll
                for (int t = 0; t < NA; ++t) hout[t * HS + hv] = cur[t][e];
            }
        }
    };

    pf2 lx[NA][MR][E];                                       // x of rows k-MR..k-1 (lag L)
    pf2 sS[MR][E];                                           // retained in-window suffixes
    float sE[MR][E];
    double cbR[MR], cbI[MR], cbE[MR];                        // row bases C[j], j in (k-MR, k]
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        cbR[m] = 0.0; cbI[m] = 0.0; cbE[m] = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            sS[m][e] = pf2{0.f, 0.f}; sE[m][e] = 0.f;
#pragma unroll
            for (int t = 0; t < NA; ++t) lx[t][m][e] = pf2{0.f, 0.f};
        }
    }
    double CR = h.CR, CI = h.CI, CE = h.CE;                  // C[k]: prefix at the start of row k
    double nCR = h.CR, nCI = h.CI, nCE = h.CE;               // C at the start of row js

    // rows 0 .. MR-1: raw samples into the lag ring
    if (nrows > 0) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            float2 cur[NA][E];
            load_row(m, cur);
            store_hist(m, cur);
#pragma unroll
            for (int t = 0; t < NA; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) lx[t][m][e] = pf2{cur[t][e].x, cur[t][e].y};
        }
    }
    float2 nx[PD][NA][E];
#pragma unroll
    for (int p = 0; p < PD; ++p) {
        if (MR + p < nrows) load_row(MR + p, nx[p]);
        else
#pragma unroll
            for (int t = 0; t < NA; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) nx[p][t][e] = make_float2(0.f, 0.f);
    }

    // gate coordinates: virtual position + GO, absolute index = gate coordinate + abs0
    const int Hp = a.hyst > 1 ? a.hyst : 1;
    const int KOFF = (Hp + RL - 1) / RL;
    const int GO = RL * KOFF;
    const int Tg = Vend + GO;                                // end of the chunk
    AaRowGate<E, float, false, true, true, true> gate;
    if (a.detect) {
        gate.init(a.hyst, L, a.thr, a.fs, a.max_ev, a.ev_i + b * (int64_t)a.max_ev * 4,
                  a.ev_r + b * (int64_t)a.max_ev * 4);
        // a closed gate's last above position has had its close: not loaded (the close lies before n_seen)
        gate.load(RL * kb - GO, h.gate_open ? h.carry_p1 : 0, h.gate_open, h.ev_start, h.bidx, (float)h.bpm,
                  (float)h.bpr, (float)h.bpi, (float)h.bm);
    }
    float2* Pout = reinterpret_cast<float2*>(a.P) + b * Tc;
    float* Rout = reinterpret_cast<float*>(a.R) + b * Tc;
    float* Mout = reinterpret_cast<float*>(a.M) + b * Tc;
    uint8_t* Vout = a.valid ? a.valid + b * Tc : nullptr;
    const float floor_ = 1e-6f * (float)L;
    const int Tci = (int)Tc;

    for (int j0 = MR; j0 < nrows; j0 += PER) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int j = j0 + u;
            if (j < nrows) {
                const int sl = u % MR;                       // ring slot of row k-MR (and k)
                const int so = (u + 1) % MR;                 // slot of C[k-MR+1]
                const int nb = RL * j + E * lane;            // virtual position of element 0
                float2 cur[NA][E];
#pragma unroll
                for (int t = 0; t < NA; ++t)
#pragma unroll
                    for (int e = 0; e < E; ++e) cur[t][e] = nx[u % PD][t][e];
                if (j + PD < nrows) load_row(j + PD, nx[u % PD]);
                store_hist(j, cur);
                if (j == js) { nCR = CR; nCI = CI; nCE = CE; }
                if (j < jz) continue;                        // before the stream
                const bool first = j < jf;                   // absolute row < MR (wave-uniform)
                // lagged samples x[n-L] (row k-MR) of every antenna
                pf2 d[NA][E];
#pragma unroll
                for (int t = 0; t < NA; ++t)
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        d[t][e] = lx[t][sl][e];
                        lx[t][sl][e] = pf2{cur[t][e].x, cur[t][e].y};
                    }
                // From here to the row bases: the row sums of aa_fast_kernel / aa_stream_kernel, expression
                // for expression (tests/test_gpu_aa_chunked_f32.py holds this copy bit-identical to them).
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
                        if (!first) av[e] = mulc_acc(c, d[t][e], av[e]);
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
                if (!first) {                                // no lagged product before row MR
                    const RowScan sr_ = row_scan<false>(fS[E - 1].x), si_ = row_scan<false>(fS[E - 1].y);
                    tR = sr_.tot; tI = si_.tot;
                    xS = pf2{sr_.x, si_.x};
                    uS = pf2{sr_.u, si_.u};
                }
                const pf2 wS = first ? pf2{(float)CR, (float)CI} : pf2{(float)(CR - cbR[so]), (float)(CI - cbI[so])};
                const float wE = (float)(first ? CE : CE - cbE[so]);
                // ---- window sums P = suffix(row k-MR) + rows between + prefix(row k) ----
                float pr[E], pi[E], rf[E], mf[E], pmf[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    pf2 P = wS + (xS + fS[e]);
                    float RR = wE + (xE + fE[e]);
                    if (!first) { P += sS[sl][e]; RR += sE[sl][e]; }
                    sS[sl][e] = uS + gS[e]; sE[sl][e] = uE + gE[e];
                    const float pm = fmaf(P.x, P.x, P.y * P.y);
                    float m = 0.f;
                    if (!first && RR > floor_) m = fminf(pm * __builtin_amdgcn_rcpf(RR * RR), 1.f);
                    pr[e] = P.x; pi[e] = P.y; rf[e] = RR; mf[e] = m; pmf[e] = pm;
                }
                cbR[so] = CR + tR; cbI[so] = CI + tI; cbE[so] = CE + tE;
                CR += tR; CI += tI; CE += tE;
                if (RL * (j + 1) <= Hn) continue;            // a replayed row: rings and bases only
                // ---- stores: the positions of this call's chunk ----
                const int i0 = nb - Hn;                      // chunk index of element 0
                bool live[E];
#pragma unroll
                for (int e = 0; e < E; ++e) live[e] = i0 + e >= 0 && i0 + e < Tci;
                if (live[0] && live[1]) {
                    if (a.P) *reinterpret_cast<f4u*>(Pout + i0) = f4u{pr[0], pi[0], pr[1], pi[1]};
                    if (a.R) *reinterpret_cast<f2u*>(Rout + i0) = f2u{rf[0], rf[1]};
                    if (a.M) *reinterpret_cast<f2u*>(Mout + i0) = f2u{mf[0], mf[1]};
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (live[e]) {
                            if (a.P) Pout[i0 + e] = make_float2(pr[e], pi[e]);
                            if (a.R) Rout[i0 + e] = rf[e];
                            if (a.M) Mout[i0 + e] = mf[e];
                        }
                }
                if (Vout) {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (live[e]) Vout[i0 + e] = (uint8_t)(!first);
                }
                // ---- events: closed-form gate machine, streamed per row (aa_gate.h) ----
                if (a.detect && !first) {
                    bool ab[E];
                    float pmg[E];
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        ab[e] = live[e] && (double)mf[e] >= a.thr;
                        pmg[e] = live[e] ? pmf[e] : -1.f;    // a dead position is never a peak
                    }
                    gate.row_flags(lane, j + KOFF, nb + GO, Tg, ab, pmg, pr, pi, mf);
                }
            }
        }
    }
    int64_t carry_p1 = 0, ev_start = h.ev_start, bidx = h.bidx;
    int open = h.gate_open;
    double bpm = h.bpm, bpr = h.bpr, bpi = h.bpi, bm = h.bm;
    if (h.gate_open) carry_p1 = h.carry_p1;
    if (a.detect) {
        if (gate.gate_open) {
            gate.merge();                                            // the lanes' bests into the peak so far
            if (a.fin) { gate.emit(lane, Tg); gate.gate_open = 0; } // end of stream: the gate closes at n_seen
        }
        gate.save(carry_p1, open, ev_start, bidx);
        bpm = gate.bpm; bpr = gate.bpr; bpi = gate.bpi; bm = gate.bm;
        if (lane == 0) a.n_ev[b] = gate.n_ev;
    }
    if (lane == 0) {
        AaChunkF32Hdr o{};                                           // final: fresh again (the history is not read)
        o.parity = par ^ 1;
        if (!a.fin) {
            o.n_seen = h.n_seen + Tc;
            o.carry_p1 = carry_p1; o.ev_start = open ? ev_start : 0; o.bidx = open ? bidx : 0;
            o.bpm = open ? bpm : 0.0; o.bpr = open ? bpr : 0.0; o.bpi = open ? bpi : 0.0; o.bm = open ? bm : 0.0;
            o.gate_open = open;
            o.CR = nCR; o.CI = nCI; o.CE = nCE;
        }
        *hdr = o;
    }
}

template <int MR, int NA>
int chunk_launch(const AaChunkF32Args& a, hipStream_t st) {
    hipLaunchKernelGGL((aa_chunk_f32_kernel<MR, NA>), dim3((unsigned)((a.B + XC / 64 - 1) / (XC / 64))), dim3(XC), 0,
                       st, a);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}
template <int MR>
int chunk_launch_na(int na, const AaChunkF32Args& a, hipStream_t st) {
    return na == 1 ? chunk_launch<MR, 1>(a, st) : chunk_launch<MR, 2>(a, st);
}

bool chunk_shape_ok(int n_ant, int L) {
    return (n_ant == 1 || n_ant == 2) && (L == 128 || L == 256 || L == 512 || L == 1024);
}

}  // namespace

extern "C" {

int64_t ofs_aa_chunk_f32_state_bytes(int32_t n_ant, int32_t L) {
    if (!chunk_shape_ok(n_ant, L)) return OFS_EINVAL;
    return (int64_t)sizeof(AaChunkF32Hdr) + (int64_t)2 * n_ant * (2 * L + 128) * (int64_t)sizeof(float2);
}

int64_t ofs_aa_chunk_f32_max_samples(int32_t n_ant, int32_t L) {
    if (!chunk_shape_ok(n_ant, L)) return OFS_EINVAL;
    return MAX_TC;
}

int32_t ofs_aa_detect_chunk_f32(const void* x, int64_t B, int32_t n_ant, int64_t Tc, int32_t L,
                                void* state, void* P, void* R, void* M, uint8_t* valid,
                                int32_t detect, double threshold, int32_t hysteresis, double sample_rate,
                                int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_real,
                                int32_t final, void* stream) {
    if (!chunk_shape_ok(n_ant, L) || ofs_chunk::chunk_args_bad(B, Tc, MAX_TC, final, state, x) ||
        hysteresis > OFS_AA_CHUNK_MAX_HYSTERESIS)
        return OFS_EINVAL;
    if (detect && (OFS_MISSING(n_events, B) || max_events < 0 || (max_events > 0 && B > 0 && (!ev_int || !ev_real))))
        return OFS_EINVAL;
    if (B == 0) return OFS_OK;
    if ((B + XC / 64 - 1) / (XC / 64) > 0x7fffffffll) return OFS_EINVAL;
    AaChunkF32Args a{};
    a.x = x; a.B = B; a.Tc = Tc; a.state = reinterpret_cast<uint8_t*>(state);
    a.state_bytes = ofs_aa_chunk_f32_state_bytes(n_ant, L);
    a.P = P; a.R = R; a.M = M; a.valid = valid;
    a.detect = detect; a.thr = threshold; a.hyst = hysteresis; a.fs = sample_rate;
    a.max_ev = max_events; a.n_ev = n_events; a.ev_i = ev_int; a.ev_r = ev_real; a.fin = final != 0;
    hipStream_t st = (hipStream_t)stream;
    switch (L) {
        case 128: return chunk_launch_na<1>(n_ant, a, st);
        case 256: return chunk_launch_na<2>(n_ant, a, st);
        case 512: return chunk_launch_na<4>(n_ant, a, st);
        case 1024: return chunk_launch_na<8>(n_ant, a, st);
    }
    return OFS_EINVAL;
}

}  // extern "C"
