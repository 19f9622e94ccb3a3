// win_chunk.hip — resumable form of the fp32 window-metric fast path (win_fast_kernel, win_fast.hip:
// complex64 in, fp32 out) for streams that arrive in chunks (ofs_win_metric_chunk): one call takes the
// next Tc samples of B streams and returns M, P, R of the reference's streaming metrics
//   kind 1  sc.sc_streaming_metric                        (D = W = N/2, R = S_e(n))
//   kind 2  combined_sc_min.schmidl_cox_streaming_metric  (D = W = N/2, R = S_e(n) + S_e(n-W))
//   kind 3  minn.minn_streaming_metric(_parameterized)    (D = W = N/4, P over n and n-2W, R over three)
// at the stream's newest samples; what the next call needs stays in a caller-owned state buffer.
//
// THE SAME ARITHMETIC, CONTINUED (state form (a) of DESIGN §4.3f, as aa_chunk_f32.hip).  The one-shot
// kernel computes, in rows of RL = 64·E samples aligned to the start of the stream,
//     S[n] = suffix(row k-MW, after n) + (float)(C[k] - C[k-MW+1]) + prefix(row k, up to n)
// with fp32 in-row partials and C the fp64 running sum of the row totals since sample 0, and reads S
// again MW (combined) or MW and 2·MW (Minn) rows later from its history rings.  Neither the partials
// nor C are exact, so a call cannot restart them: it produces the very same fp32 and fp64 values.  Per
// stream the state keeps the raw samples from the start of absolute row k0 - HR - 2·MW up to n_seen
// (k0 = n_seen / RL; HR = 0 / MW / 2·MW history rows for kind 1 / 2 / 3) and the fp64 bases
// C[k0 - HR - MW].  A call runs the one-shot row loop over the virtual stream [history | chunk], whose
// rows are the absolute rows kb = k0 - HR - 2·MW, kb + 1, ...:
//   rows kb .. kb + MW - 1        refill the lag ring (raw samples only);
//   rows kb + MW .. k0 - 1        are replayed from the carried C: the same products, the same scans, the
//                                 same sequence cb[so] = C + t; C += t.  They refill the suffix ring, the
//                                 base ring and the history rings and store nothing.  The window sums of
//                                 the first MW of them lack their suffix and base; those land in history
//                                 slots that the following HR rows overwrite before any output reads them;
//   rows k0 ..                    are computed, and the positions >= n_seen are stored.
// Row k0 is recomputed whole (its first n_seen % RL samples are in the history); a row that the chunk
// leaves incomplete is computed with zeros after its last sample, which no output at or before that
// sample depends on (prefix scans), and is computed again by the call that completes it.  Rows of
// absolute index < MW take the one-shot kernel's no-lag form; rows of negative index (a young stream's
// history) do not exist and are skipped, so the rings they would have filled stay zero - and are added
// unconditionally, as the one-shot kernel adds its zero-initialised rings.
//
// Output element i of a call belongs to the stream's sample n = n_seen + i, the reference's index
// d = n - (N - 1); elements with d < 0 are written as +0.0.
//
// State of one stream (ofs_win_chunk_state_bytes = 64 + 2·n_br·(HR + 2·MW + 1)·RL·8 bytes, all-zero =
// fresh): WinChunkHdr (64 B), then two history slots [2][n_br][(HR + 2·MW + 1)·RL] complex64.  A call
// reads slot `parity` and writes the other one, so no word is overwritten before it is read.
#include "chunk_state.h"
#include "ofdmsync.h"

using namespace ofs;

namespace {

struct WinChunkHdr {
    int64_t n_seen;                 // samples of this stream consumed by earlier calls
    int32_t parity, pad0;           // parity: history slot holding the samples since row kb
    double CR, CI, CE;              // C[k0 - HR - MW]: fp64 sum of the row totals of the rows before it
    int64_t pad[3];
};
static_assert(sizeof(WinChunkHdr) == 64, "state header");

struct WinChunkArgs {
    const void* x; int64_t B, Tc;
    uint8_t* state; int64_t state_bytes;
    void* M; void* P; void* R; int64_t* d0;
    int32_t fin;
};

constexpr int WC_WG = 256;                      // 4 waves = 4 streams per workgroup
constexpr int64_t WC_MAX_TC = (int64_t)1 << 30; // in-call positions (history + chunk + one row) stay below 2^31
enum { WC_SC = 1, WC_COMB = 2, WC_MINN = 3 };

typedef float wf4u __attribute__((ext_vector_type(4), aligned(8)));
typedef float wf2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float wf4ua __attribute__((ext_vector_type(4), aligned(4)));
// packed fp32 pairs and the conjugated product of win_fast.hip, expression for expression
typedef float pf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pf2 cjmul_acc(pf2 c, pf2 d, pf2 acc) {
    acc = __builtin_elementwise_fma(c.xx, d, acc);
    return __builtin_elementwise_fma(c.yy, pf2{d.y, -d.x}, acc);
}

constexpr int wc_hist_rows(int mode, int mw) {  // HR + 2·MW
    return (mode == WC_SC ? 0 : mode == WC_COMB ? mw : 2 * mw) + 2 * mw;
}

template <int MODE, int E, int MW, int NB>
__global__ __launch_bounds__(WC_WG) void win_chunk_kernel(WinChunkArgs a) {
    constexpr int RL = 64 * E;
    constexpr int W = MW * RL;
    constexpr int N = (MODE == WC_MINN) ? 4 * W : 2 * W;
    constexpr int HR = (MODE == WC_MINN) ? 2 * MW : MW;     // history ring rows (COMB / MINN), as win_fast
    constexpr int HB = wc_hist_rows(MODE, MW);               // rows of history before row k0
    constexpr int HS = (HB + 1) * RL;                        // samples of one history slot, per branch
    constexpr int PD = 2;                                    // rows in flight ahead of use
    constexpr int PER = HR > PD ? HR : PD;                   // unroll period (ring sizes divide it)
    constexpr int V4 = E / 2;                                // float4 loads per lane per row
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (WC_WG / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int64_t Tc = a.Tc;
    uint8_t* sp = a.state + b * a.state_bytes;
    WinChunkHdr* hdr = reinterpret_cast<WinChunkHdr*>(sp);
    const WinChunkHdr h = *hdr;
    const int par = h.parity & 1;
    float2* hist = reinterpret_cast<float2*>(sp + sizeof(WinChunkHdr));
    const float2* hin = hist + (int64_t)par * NB * HS;
    float2* hout = hist + (int64_t)(par ^ 1) * NB * HS;
    const float2* xs = reinterpret_cast<const float2*>(a.x) + b * NB * Tc;

    // virtual stream [history | chunk]: virtual row j is the absolute row kb + j
    const int64_t k0 = h.n_seen / RL;
    const int64_t kb = k0 - HB;
    const int Hn = (int)(h.n_seen - RL * kb);                // history samples: HB·RL + n_seen % RL
    const int Vend = Hn + (int)Tc;                           // end of the chunk
    const int nrows = Tc > 0 ? (Vend + RL - 1) / RL : 0;
    const int jz = kb < 0 ? (int)-kb : 0;                    // rows j < jz lie before the stream: skipped
    const int jf = kb < MW ? (int)(MW - kb) : 0;             // rows j < jf have absolute index < MW: no lag
    const int dk = (int)((h.n_seen + Tc) / RL - k0);         // rows the next call's history starts later
    const int js = dk + MW;                                  // the row whose base C the next call starts from
    const int hshift = RL * dk;
    // virtual position of the sample n = N - 1 (d = 0): outputs before it are +0.0
    const int vN = RL * kb >= N - 1 ? 0 : (int)(N - 1 - RL * kb);

    auto load_row = [&](int j, float4 (&dst)[NB][V4]) {      // row j of [history | chunk]
        const int v0 = RL * j + E * lane;
#pragma unroll
        for (int t = 0; t < NB; ++t) {
#pragma unroll
            for (int q = 0; q < V4; ++q) {
                if (j < jz) {
                    dst[t][q] = make_float4(0.f, 0.f, 0.f, 0.f);
                } else if (RL * (j + 1) <= Hn) {             // whole row in the history (16-byte aligned)
                    dst[t][q] = *reinterpret_cast<const float4*>(hin + t * HS + v0 + 2 * q);
                } else if (RL * j >= Hn && RL * (j + 1) <= Vend) {   // whole row in the chunk (8-byte aligned)
                    const wf4u v = *reinterpret_cast<const wf4u*>(xs + t * Tc + (v0 + 2 * q - Hn));
                    dst[t][q] = make_float4(v.x, v.y, v.z, v.w);
                } else {
                    float2 s[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int v = v0 + 2 * q + i;
                        s[i] = make_float2(0.f, 0.f);
                        if (v < Hn) s[i] = hin[t * HS + v];
                        else if (v < Vend) s[i] = xs[t * Tc + (v - Hn)];
                    }
                    dst[t][q] = make_float4(s[0].x, s[0].y, s[1].x, s[1].y);
                }
            }
        }
    };
    // the samples from absolute row kb + dk on become the next call's history (other slot)
    auto store_hist = [&](int j, const float4 (&cur)[NB][V4]) {
        if (a.fin || j < jz || RL * (j + 1) <= hshift) return;
        const int v0 = RL * j + E * lane;
        if (RL * j >= hshift && RL * (j + 1) <= Vend) {      // whole row kept (16-byte aligned)
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int q = 0; q < V4; ++q)
                    *reinterpret_cast<float4*>(hout + t * HS + (v0 + 2 * q - hshift)) = cur[t][q];
        } else {
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int q = 0; q < V4; ++q) {
                    const int v = v0 + 2 * q, hv = v - hshift;
                    if (hv >= 0 && v < Vend) hout[t * HS + hv] = make_float2(cur[t][q].x, cur[t][q].y);
                    if (hv + 1 >= 0 && v + 1 < Vend) hout[t * HS + hv + 1] = make_float2(cur[t][q].z, cur[t][q].w);
                }
        }
    };

    pf2 lx[NB][MW][E];                           // x of rows k-MW..k-1 (lag D = W), per branch
    pf2 sS[MW][E];                               // retained in-window suffixes (conj products)
    float sE[MW][E];
    pf2 hS[HR][E];                               // window sums of past rows (MINN: products)
    float hE[HR][E];                             // (COMB / MINN: energies)
    double cbR[MW], cbI[MW], cbE[MW];            // row bases C[j] for j in (k-MW, k]
#pragma unroll
    for (int m = 0; m < MW; ++m) {
        cbR[m] = 0.0; cbI[m] = 0.0; cbE[m] = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            sS[m][e] = pf2{0.f, 0.f}; sE[m][e] = 0.f;
#pragma unroll
            for (int t = 0; t < NB; ++t) lx[t][m][e] = pf2{0.f, 0.f};
        }
    }
#pragma unroll
    for (int m = 0; m < HR; ++m)
#pragma unroll
        for (int e = 0; e < E; ++e) { hS[m][e] = pf2{0.f, 0.f}; hE[m][e] = 0.f; }
    double CR = h.CR, CI = h.CI, CE = h.CE;      // C[k]: prefix at the start of row k
    double nCR = h.CR, nCI = h.CI, nCE = h.CE;   // C at the start of row js

    // rows 0 .. MW-1: raw samples into the lag ring
    if (nrows > 0) {
#pragma unroll
        for (int m = 0; m < MW; ++m) {
            float4 cur[NB][V4];
            load_row(m, cur);
            store_hist(m, cur);
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float4 v = cur[t][e / 2];
                    lx[t][m][e] = (e & 1) ? pf2{v.z, v.w} : pf2{v.x, v.y};
                }
        }
    }
    float4 nx[PD][NB][V4];
#pragma unroll
    for (int p = 0; p < PD; ++p) {
        if (MW + p < nrows) load_row(MW + p, nx[p]);
        else
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int q = 0; q < V4; ++q) nx[p][t][q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    float* Mo = a.M ? reinterpret_cast<float*>(a.M) + b * Tc : nullptr;
    float2* Po = a.P ? reinterpret_cast<float2*>(a.P) + b * Tc : nullptr;
    float* Ro = a.R ? reinterpret_cast<float*>(a.R) + b * Tc : nullptr;
    const int Tci = (int)Tc;

    for (int j0 = MW; j0 < nrows; j0 += PER) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int j = j0 + u;
            if (j < nrows) {
                const int sl = u % MW;                              // ring slot of row k (and k-MW)
                float4 cur[NB][V4];
#pragma unroll
                for (int t = 0; t < NB; ++t)
#pragma unroll
                    for (int q = 0; q < V4; ++q) cur[t][q] = nx[u % PD][t][q];
                if (j + PD < nrows) load_row(j + PD, nx[u % PD]);   // PD rows ahead
                store_hist(j, cur);
                if (j == js) { nCR = CR; nCI = CI; nCE = CE; }
                if (j < jz) continue;                               // before the stream
                const bool lag = j >= jf;                           // absolute row >= MW (wave-uniform)
                // From here to the row bases: the row body of win_fast_kernel, expression for expression
                // (tests/test_gpu_win_chunked.py holds this copy bit-identical to it).
                // ---- lagged products conj(x[j])·x[j-D] and energies, summed over the branches ----
                pf2 av[E];
                float aE[E];
#pragma unroll
                for (int e = 0; e < E; ++e) { av[e] = pf2{0.f, 0.f}; aE[e] = 0.f; }
#pragma unroll
                for (int t = 0; t < NB; ++t) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {                   // zeros past the chunk from load_row
                        const float4 v = cur[t][e / 2];
                        const pf2 c = (e & 1) ? pf2{v.z, v.w} : pf2{v.x, v.y};
                        aE[e] += fmaf(c.x, c.x, c.y * c.y);
                        if (lag) av[e] = cjmul_acc(c, lx[t][sl][e], av[e]);
                        lx[t][sl][e] = c;
                    }
                }
                // ---- in-lane partials (forward f, backward g) ----
                pf2 fS[E], gS[E];
                float fE[E], gE[E];
                fS[0] = av[0]; fE[0] = aE[0];
#pragma unroll
                for (int e = 1; e < E; ++e) { fS[e] = fS[e - 1] + av[e]; fE[e] = fE[e - 1] + aE[e]; }
                gS[E - 1] = pf2{0.f, 0.f}; gE[E - 1] = 0.f;
#pragma unroll
                for (int e = E - 2; e >= 0; --e) { gS[e] = gS[e + 1] + av[e + 1]; gE[e] = gE[e + 1] + aE[e + 1]; }
                // ---- lane totals: fp64 wave scan; row totals; rows strictly inside the window ----
                const double iR = scan_add((double)fS[E - 1].x), iI = scan_add((double)fS[E - 1].y), iE = scan_add((double)fE[E - 1]);
                const double tR = readlane(iR, 63), tI = readlane(iI, 63), tE = readlane(iE, 63);
                const pf2 xS = pf2{(float)shr1z(iR), (float)shr1z(iI)}, uS = pf2{(float)(tR - iR), (float)(tI - iI)};
                const float xE = (float)shr1z(iE), uE = (float)(tE - iE);
                const int so = (u + 1) % MW;                        // slot of C[k-MW+1]
                const pf2 wS = lag ? pf2{(float)(CR - cbR[so]), (float)(CI - cbI[so])} : pf2{(float)CR, (float)CI};
                const float wE = (float)(lag ? CE - cbE[so] : CE);
                // ---- window sums, outputs ----
                float oM[E], oR[E];
                pf2 oP[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    pf2 S = wS + (xS + fS[e]);
                    float SE = wE + (xE + fE[e]);
                    if (lag) { S += sS[sl][e]; SE += sE[sl][e]; }
                    sS[sl][e] = uS + gS[e]; sE[sl][e] = uE + gE[e];
                    pf2 P = S;
                    float RR = SE;
                    if constexpr (MODE == WC_COMB) {
                        RR += hE[sl][e];                            // S_e(n - W): row k-MW
                        hE[sl][e] = SE;
                    } else if constexpr (MODE == WC_MINN) {
                        const int h2 = u % HR;                      // row k-2MW (and k)
                        const int h1 = (u + MW) % HR;               // row k-MW
                        P += hS[h2][e];
                        RR += hE[h1][e] + hE[h2][e];
                        hS[h2][e] = S; hE[h2][e] = SE;
                    }
                    const float den = fmaxf(RR, 1e-12f);
                    const float num = (MODE == WC_MINN) ? fmaxf(P.x, 0.f) * fmaxf(P.x, 0.f) : fmaf(P.x, P.x, P.y * P.y);
                    oM[e] = num * __builtin_amdgcn_rcpf(den * den);
                    oP[e] = P; oR[e] = RR;
                }
                // C[k+1] replaces C[k-MW+1] in the ring
                cbR[so] = CR + tR; cbI[so] = CI + tI; cbE[so] = CE + tE;
                CR += tR; CI += tI; CE += tE;
                if (RL * (j + 1) <= Hn) continue;                   // a replayed row: rings and bases only
                // ---- stores: the positions of this call's chunk; +0.0 while d < 0 ----
                const int nb = RL * j + E * lane;                   // virtual position of element 0
                const int i0 = nb - Hn;                             // chunk index of element 0
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (nb + e < vN) { oM[e] = 0.f; oR[e] = 0.f; oP[e] = pf2{0.f, 0.f}; }
                if (i0 >= 0 && i0 + E <= Tci) {
                    if constexpr (E >= 4) {
#pragma unroll
                        for (int q = 0; q < E; q += 4) {
                            if (Mo) *reinterpret_cast<wf4ua*>(Mo + i0 + q) = wf4ua{oM[q], oM[q + 1], oM[q + 2], oM[q + 3]};
                            if (Ro) *reinterpret_cast<wf4ua*>(Ro + i0 + q) = wf4ua{oR[q], oR[q + 1], oR[q + 2], oR[q + 3]};
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < E; q += 2) {
                            if (Mo) *reinterpret_cast<wf2u*>(Mo + i0 + q) = wf2u{oM[q], oM[q + 1]};
                            if (Ro) *reinterpret_cast<wf2u*>(Ro + i0 + q) = wf2u{oR[q], oR[q + 1]};
                        }
                    }
#pragma unroll
                    for (int q = 0; q < E; q += 2)
                        if (Po) *reinterpret_cast<wf4u*>(Po + i0 + q) = wf4u{oP[q].x, oP[q].y, oP[q + 1].x, oP[q + 1].y};
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const int i = i0 + e;
                        if (i >= 0 && i < Tci) {
                            if (Mo) Mo[i] = oM[e];
                            if (Po) Po[i] = make_float2(oP[e].x, oP[e].y);
                            if (Ro) Ro[i] = oR[e];
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) {
        if (a.d0) a.d0[b] = h.n_seen - (N - 1);
        WinChunkHdr o{};                                     // final: fresh again (the history is not read)
        if (!a.fin) {
            o.n_seen = h.n_seen + Tc;
            o.parity = par ^ 1;
            o.CR = nCR; o.CI = nCI; o.CE = nCE;
        }
        *hdr = o;
    }
}

template <int MODE, int E, int MW, int NB>
int launch(const WinChunkArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((win_chunk_kernel<MODE, E, MW, NB>), dim3((unsigned)((a.B + WC_WG / 64 - 1) / (WC_WG / 64))),
                       dim3(WC_WG), 0, st, a);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}

template <int MODE, int NB>
int launch_plan(int plan, const WinChunkArgs& a, hipStream_t st) {
    switch (plan) {                                          // 10·E + MW of ofs_win_plan
        case 21: return launch<MODE, 2, 1, NB>(a, st);
        case 41: return launch<MODE, 4, 1, NB>(a, st);
        case 42: return launch<MODE, 4, 2, NB>(a, st);
        case 44: return launch<MODE, 4, 4, NB>(a, st);
        case 48:
            if constexpr (NB == 1) return launch<MODE, 4, 8, 1>(a, st);
    }
    return OFS_EINVAL;
}

template <int NB>
int launch_mode(int kind, int plan, const WinChunkArgs& a, hipStream_t st) {
    switch (kind) {
        case WC_SC: return launch_plan<WC_SC, NB>(plan, a, st);
        case WC_COMB: return launch_plan<WC_COMB, NB>(plan, a, st);
        case WC_MINN: return launch_plan<WC_MINN, NB>(plan, a, st);
    }
    return OFS_EINVAL;
}

// 10·E + MW of the one-shot fast kernel for this shape (the chunked kernel runs the same rows), or 0
int chunk_plan(int kind, int n_br, int symbol_len) {
    if (kind < WC_SC || kind > WC_MINN || symbol_len < 1) return 0;
    const int plan = ofs_win_fast_plan(kind, OFS_C64, OFS_FP32, n_br, symbol_len, symbol_len);
    switch (plan) {                                          // the table compiled above, nothing else
        case 21: case 41: case 42: case 44: return plan;
        case 48: return n_br == 1 ? plan : 0;
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t ofs_win_chunk_state_bytes(int32_t kind, int32_t n_br, int32_t symbol_len) {
    const int plan = chunk_plan(kind, n_br, symbol_len);
    if (!plan) return OFS_EINVAL;
    const int64_t RL = 64 * (plan / 10);
    return (int64_t)sizeof(WinChunkHdr) + 2 * n_br * (wc_hist_rows(kind, plan % 10) + 1) * RL * (int64_t)sizeof(float2);
}

int64_t ofs_win_chunk_max_samples(int32_t kind, int32_t n_br, int32_t symbol_len) {
    if (!chunk_plan(kind, n_br, symbol_len)) return OFS_EINVAL;
    return WC_MAX_TC;
}

int32_t ofs_win_metric_chunk(int32_t kind, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                             int32_t symbol_len, void* state, void* M, void* P, void* R,
                             int64_t* d0, int32_t final, void* stream) {
    const int plan = chunk_plan(kind, n_br, symbol_len);
    if (!plan || ofs_chunk::chunk_args_bad(B, Tc, WC_MAX_TC, final, state, x))
        return OFS_EINVAL;
    if (B == 0) return OFS_OK;
    if ((B + WC_WG / 64 - 1) / (WC_WG / 64) > 0x7fffffffll) return OFS_EINVAL;
    WinChunkArgs a{};
    a.x = x; a.B = B; a.Tc = Tc; a.state = reinterpret_cast<uint8_t*>(state);
    a.state_bytes = ofs_win_chunk_state_bytes(kind, n_br, symbol_len);
    a.M = M; a.P = P; a.R = R; a.d0 = d0; a.fin = final != 0;
    hipStream_t st = (hipStream_t)stream;
    return n_br == 1 ? launch_mode<1>(kind, plan, a, st) : launch_mode<2>(kind, plan, a, st);
}

}  // extern "C"
