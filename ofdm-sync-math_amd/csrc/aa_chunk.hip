// aa_chunk.hip — resumable form of aa_exact_kernel for integer streams of any length
// (ofs_aa_detect_chunk): one call takes the next Tc samples of B streams and returns their P, R,
// M, valid and the gate events that closed among them; what the next call needs stays in a
// caller-owned state buffer on the device.
//
// HISTORY, NOT CARRIED SUMS.  Per stream the state keeps the last 2L samples per antenna as decoded
// int16 I/Q words.  A call runs the one-shot kernel's row loop over the virtual stream
// [history (2L) | chunk (Tc)]: the 2·MR history rows only refill the lag ring and the prefix ring
// (no stores, no gate), and every virtual position >= 2L then sees exactly the products and the
// window sums of the unbroken stream.  They are exact integers ((Tc + 2L)·n_ant <= 2^21 keeps
// every prefix below 2^53), so P and R equal the one-shot values bit for bit and M, computed from
// them by the same expressions, does too.  A fresh stream's history is zeros: the one-shot
// kernel's zero lag line.
//
// ABSOLUTE POSITIONS.  The state carries n_seen; valid[n] and whether the gate sees a sample depend
// on the absolute index n_seen + i >= L, per sample.  The gate machine (AaRowGate, ABS form) runs in
// call-local "gate coordinates" g = virtual position + RL·KOFF, KOFF = ceil(max(H, 1) / RL) rows, so
// that the last above-threshold position of an earlier call is never negative while it can still
// matter; its wave-uniform fields are loaded from and saved to the state as absolute indices.
//
// State of one stream (ofs_aa_chunk_state_bytes = 128 + 16·n_ant·L bytes, all-zero = fresh):
//   AaChunkHdr (128 B), then two history slots [2][n_ant][2L] int32 words.  A call reads slot
//   `parity` and writes the other one, so no word is overwritten before it is read.
#include "chunk_state.h"
#include "aa_gate.h"
#include "aa_words.h"
#include "ofdmsync.h"

using namespace ofs;

namespace {

struct AaChunkHdr {
    int64_t n_seen;                 // samples of this stream consumed by earlier calls
    int64_t carry_p1;               // 1 + absolute index of the last above-threshold sample, 0 = none
    int64_t ev_start, bidx;         // open gate: its start, its peak so far (absolute)
    double bpm, bpr, bpi, bm;       // open gate: |P|², P, M at that peak
    int32_t gate_open, parity;      // parity: history slot holding the last 2L samples
    int64_t pad[7];
};
static_assert(sizeof(AaChunkHdr) == 128, "state header");

struct AaChunkArgs {
    const void* x; int64_t B, Tc;
    uint8_t* state; int64_t state_bytes;
    void* P; void* R; void* M; uint8_t* valid;
    int32_t detect; double thr; int32_t hyst; double fs;
    int32_t max_ev; int32_t* n_ev; int64_t* ev_i; double* ev_r;
    int32_t fin;
};

constexpr int XC = 256;                 // 4 waves = 4 streams per workgroup

template <int FMT, int E, int MR, int NA>
__global__ __launch_bounds__(XC) void aa_chunk_kernel(AaChunkArgs a) {
    using X = XSamp<OFS_CI16>;                               // CP12 decodes to int16 I/Q words
    using W = int32_t;
    constexpr int RL = 64 * E;
    constexpr int L = MR * RL;
    constexpr int H = 2 * L;                                 // history samples = HR whole rows
    constexpr int HR = 2 * MR;
    constexpr int PD = 4;                                    // rows in flight ahead of use
    constexpr int PER = MR > PD ? MR : PD;                   // unroll period (MR, PD powers of 2)
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (XC / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int64_t Tc = a.Tc;
    uint8_t* sp = a.state + b * a.state_bytes;
    AaChunkHdr* hdr = reinterpret_cast<AaChunkHdr*>(sp);
    const AaChunkHdr h = *hdr;
    const int par = h.parity & 1;
    W* hist = reinterpret_cast<W*>(sp + sizeof(AaChunkHdr));
    const W* hin = hist + (int64_t)par * NA * H;
    W* hout = hist + (int64_t)(par ^ 1) * NA * H;
    // a flush (Tc = 0) closes the open gate from the saved fields alone: no rows
    const int nrows = Tc > 0 ? HR + (int)((Tc + RL - 1) / RL) : 0;
    const W* xs = reinterpret_cast<const W*>(a.x) + b * NA * Tc;
    const int64_t sbyte = b * NA * Tc * 3;                       // CP12: stream start in bytes
    const uint8_t* x8 = reinterpret_cast<const uint8_t*>(a.x) + sbyte;
    const int64_t total = a.B * NA * Tc * 3;
    auto load_all = [&](int k, W (&dst)[NA][E]) {            // row k of [history | chunk]
        const int64_t n0 = (int64_t)RL * k + E * lane;
        if (k < HR) {
#pragma unroll
            for (int t = 0; t < NA; ++t) load_words<E>(hin + t * H, n0, H, dst[t]);
        } else if constexpr (FMT == OFS_CP12) {
            cp12_load<E, NA>(x8, sbyte, n0 - H, Tc, total, dst);
        } else {
#pragma unroll
            for (int t = 0; t < NA; ++t) load_words<E>(xs + t * Tc, n0 - H, Tc, dst[t]);
        }
    };

    W lag[NA][MR][E];                                        // raw samples of rows k-MR..k-1
    double Ar[MR][E], Ai[MR][E], Ae[MR][E];                  // prefix values of rows k-MR..k-1
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            Ar[m][e] = 0.0; Ai[m][e] = 0.0; Ae[m][e] = 0.0;
#pragma unroll
            for (int t = 0; t < NA; ++t) lag[t][m][e] = X::zero();
        }
    double CR = 0.0, CI = 0.0, CE = 0.0;                     // prefix at the start of row k

    W nx[PD][NA][E];
#pragma unroll
    for (int p = 0; p < PD; ++p) {
        if (p < nrows) load_all(p, nx[p]);
        else
#pragma unroll
            for (int t = 0; t < NA; ++t)
#pragma unroll
                for (int e = 0; e < E; ++e) nx[p][t][e] = X::zero();
    }

    // gate coordinates: virtual position + GO, absolute index = gate coordinate + abs0
    const int Hp = a.hyst > 1 ? a.hyst : 1;
    const int KOFF = (Hp + RL - 1) / RL;
    const int GO = RL * KOFF;
    const int Tg = H + (int)Tc + GO;                         // end of the chunk
    AaRowGate<E, double, false, true, true, true> gate;
    if (a.detect) {
        gate.init(a.hyst, L, a.thr, a.fs, a.max_ev, a.ev_i + b * (int64_t)a.max_ev * 4,
                  a.ev_r + b * (int64_t)a.max_ev * 4);
        gate.load(h.n_seen - H - GO, h.carry_p1, h.gate_open, h.ev_start, h.bidx, h.bpm, h.bpr, h.bpi, h.bm);
    }
    double2* Pout = reinterpret_cast<double2*>(a.P) + b * Tc;
    double* Rout = reinterpret_cast<double*>(a.R) + b * Tc;
    double* Mout = reinterpret_cast<double*>(a.M) + b * Tc;
    uint8_t* Vout = a.valid ? a.valid + b * Tc : nullptr;
    const double floor_ = 1e-6 * (double)L;
    const int64_t first_valid = (int64_t)L - h.n_seen;       // chunk index of absolute position L

    for (int k0 = 0; k0 < nrows; k0 += PER) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int k = k0 + u;
            if (k < nrows) {
                const int nb = RL * k + E * lane;            // virtual position of element 0
                W cur[NA][E];
#pragma unroll
                for (int t = 0; t < NA; ++t)
#pragma unroll
                    for (int e = 0; e < E; ++e) cur[t][e] = nx[u % PD][t][e];
                if (k + PD < nrows) load_all(k + PD, nx[u % PD]);
                const int sl = u % MR;                       // ring slot of row k-MR (and k)
                double pr[E], pi[E], en[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    pr[e] = 0.0; pi[e] = 0.0; en[e] = 0.0;
#pragma unroll
                    for (int t = 0; t < NA; ++t) {
                        const double xr = X::re(cur[t][e]), xi = X::im(cur[t][e]);
                        const double dr = X::re(lag[t][sl][e]), di = X::im(lag[t][sl][e]);
                        pr[e] += xr * dr + xi * di;                  // x[n]·conj(x[n-L]), exact
                        pi[e] += xi * dr - xr * di;
                        en[e] += xr * xr + xi * xi;
                        lag[t][sl][e] = cur[t][e];
                    }
                }
                // the last 2L samples of [history | chunk] become the next call's history (other slot)
                if (!a.fin && (int64_t)RL * (k + 1) > Tc) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const int64_t hi = (int64_t)nb + e - Tc;
                        if (hi >= 0 && hi < H) {
#pragma unroll
                            for (int t = 0; t < NA; ++t) hout[t * H + hi] = cur[t][e];
                        }
                    }
                }
                RowPrefix<E> qr, qi, qe;
                qr.run(pr); qi.run(pi); qe.run(en);
                const int64_t i0 = (int64_t)nb - H;                  // chunk index of element 0
                double oP[E][2], oR[E], oM[E], opm[E];
                bool vld[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const double A_r = (CR + qr.excl) + qr.f[e];
                    const double A_i = (CI + qi.excl) + qi.f[e];
                    const double A_e = (CE + qe.excl) + qe.f[e];
                    const double Pr = A_r - Ar[sl][e], Pi = A_i - Ai[sl][e], Rr = A_e - Ae[sl][e];
                    Ar[sl][e] = A_r; Ai[sl][e] = A_i; Ae[sl][e] = A_e;
                    const double pm = Pr * Pr + Pi * Pi;
                    const bool valid = i0 + e >= first_valid;        // absolute n >= L, per sample
                    double m = 0.0;
                    if (valid && Rr > floor_) { m = pm / (Rr * Rr); m = m < 1.0 ? m : 1.0; }
                    oP[e][0] = Pr; oP[e][1] = Pi; oR[e] = Rr; oM[e] = m; opm[e] = pm; vld[e] = valid;
                }
                CR += qr.tot; CI += qi.tot; CE += qe.tot;
                if (k < HR) continue;                                // history rows: rings only
                // stores: a lane's E samples are contiguous; R/M pairs where 16-byte aligned
                const bool whole = i0 + E <= Tc;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (a.P && i0 + e < Tc) Pout[i0 + e] = make_double2(oP[e][0], oP[e][1]);
                if constexpr (E >= 2) {
                    const bool pr_ok = whole && (reinterpret_cast<uintptr_t>(Rout + i0) & 15) == 0;
                    const bool pm_ok = whole && (reinterpret_cast<uintptr_t>(Mout + i0) & 15) == 0;
                    if (a.R) {
                        if (pr_ok) {
#pragma unroll
                            for (int e = 0; e < E; e += 2)
                                *reinterpret_cast<double2*>(Rout + i0 + e) = make_double2(oR[e], oR[e + 1]);
                        } else {
#pragma unroll
                            for (int e = 0; e < E; ++e)
                                if (i0 + e < Tc) Rout[i0 + e] = oR[e];
                        }
                    }
                    if (a.M) {
                        if (pm_ok) {
#pragma unroll
                            for (int e = 0; e < E; e += 2)
                                *reinterpret_cast<double2*>(Mout + i0 + e) = make_double2(oM[e], oM[e + 1]);
                        } else {
#pragma unroll
                            for (int e = 0; e < E; ++e)
                                if (i0 + e < Tc) Mout[i0 + e] = oM[e];
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (i0 + e < Tc) {
                            if (a.R) Rout[i0 + e] = oR[e];
                            if (a.M) Mout[i0 + e] = oM[e];
                        }
                }
                if (Vout) {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (i0 + e < Tc) Vout[i0 + e] = (uint8_t)vld[e];
                }
                if (a.detect) {
                    double ppr[E], ppi[E];
                    bool ab[E];
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        ppr[e] = oP[e][0]; ppi[e] = oP[e][1];
                        ab[e] = i0 + e < Tc && vld[e] && oM[e] >= a.thr;
                    }
                    gate.row_flags(lane, k + KOFF, nb + GO, Tg, ab, opm, ppr, ppi, oM);
                }
            }
        }
    }
    int64_t carry_p1 = h.carry_p1, ev_start = h.ev_start, bidx = h.bidx;
    int open = h.gate_open;
    double bpm = h.bpm, bpr = h.bpr, bpi = h.bpi, bm = h.bm;
    if (a.detect) {
        if (gate.gate_open) {
            gate.merge();                                            // the lanes' bests into the peak so far
            if (a.fin) { gate.emit(lane, Tg); gate.gate_open = 0; } // end of stream: the gate closes at n_seen
        }
        gate.save(carry_p1, open, ev_start, bidx);
        bpm = gate.bpm; bpr = gate.bpr; bpi = gate.bpi; bm = gate.bm;
        if (lane == 0) a.n_ev[b] = gate.n_ev;
    }
    if (a.fin) {                                                     // fresh again: zero history, zero header
        for (int j = 4 * lane; j < NA * H; j += 256) *reinterpret_cast<int4*>(hout + j) = make_int4(0, 0, 0, 0);
    }
    if (lane == 0) {
        AaChunkHdr o{};
        o.parity = par ^ 1;
        if (!a.fin) {
            o.n_seen = h.n_seen + Tc;
            o.carry_p1 = carry_p1; o.ev_start = open ? ev_start : 0; o.bidx = open ? bidx : 0;
            o.bpm = open ? bpm : 0.0; o.bpr = open ? bpr : 0.0; o.bpi = open ? bpi : 0.0; o.bm = open ? bm : 0.0;
            o.gate_open = open;
        }
        *hdr = o;
    }
}

template <int FMT, int E, int MR, int NA>
int chunk_launch(const AaChunkArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((aa_chunk_kernel<FMT, E, MR, NA>), dim3((unsigned)((a.B + XC / 64 - 1) / (XC / 64))), dim3(XC),
                       0, st, a);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}
template <int E, int MR>
int chunk_launch_na(int fmt, int na, const AaChunkArgs& a, hipStream_t st) {
    if (fmt == OFS_CP12)
        return na == 1 ? chunk_launch<OFS_CP12, E, MR, 1>(a, st) : chunk_launch<OFS_CP12, E, MR, 2>(a, st);
    return na == 1 ? chunk_launch<OFS_CI16, E, MR, 1>(a, st) : chunk_launch<OFS_CI16, E, MR, 2>(a, st);
}

bool chunk_shape_ok(int n_ant, int L) {
    return (n_ant == 1 || n_ant == 2) && (L == 64 || L == 128 || L == 256 || L == 512 || L == 1024);
}

}  // namespace

extern "C" {

int64_t ofs_aa_chunk_state_bytes(int32_t n_ant, int32_t L) {
    if (!chunk_shape_ok(n_ant, L)) return OFS_EINVAL;
    return (int64_t)sizeof(AaChunkHdr) + (int64_t)2 * n_ant * 2 * L * (int64_t)sizeof(int32_t);
}

int64_t ofs_aa_chunk_max_samples(int32_t n_ant, int32_t L) {
    if (!chunk_shape_ok(n_ant, L)) return OFS_EINVAL;
    return ((int64_t)1 << 21) / n_ant - 2 * (int64_t)L;          // (Tc + 2L)·n_ant <= 2^21: sums < 2^53
}

int32_t ofs_aa_detect_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_ant, int64_t Tc, int32_t L,
                            void* state, void* P, void* R, void* M, uint8_t* valid,
                            int32_t detect, double threshold, int32_t hysteresis, double sample_rate,
                            int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_real,
                            int32_t final, void* stream) {
    if ((in_fmt != OFS_CI16 && in_fmt != OFS_CP12) || !chunk_shape_ok(n_ant, L) ||
        ofs_chunk::chunk_args_bad(B, Tc, ofs_aa_chunk_max_samples(n_ant, L), final, state, x) ||
        hysteresis > OFS_AA_CHUNK_MAX_HYSTERESIS)
        return OFS_EINVAL;
    if (detect && (OFS_MISSING(n_events, B) || max_events < 0 || (max_events > 0 && B > 0 && (!ev_int || !ev_real))))
        return OFS_EINVAL;
    if (B == 0) return OFS_OK;
    if ((B + XC / 64 - 1) / (XC / 64) > 0x7fffffffll) return OFS_EINVAL;
    AaChunkArgs a{};
    a.x = x; a.B = B; a.Tc = Tc; a.state = reinterpret_cast<uint8_t*>(state);
    a.state_bytes = ofs_aa_chunk_state_bytes(n_ant, L);
    a.P = P; a.R = R; a.M = M; a.valid = valid;
    a.detect = detect; a.thr = threshold; a.hyst = hysteresis; a.fs = sample_rate;
    a.max_ev = max_events; a.n_ev = n_events; a.ev_i = ev_int; a.ev_r = ev_real; a.fin = final != 0;
    hipStream_t st = (hipStream_t)stream;
    switch (L) {
        case 64: return chunk_launch_na<1, 1>(in_fmt, n_ant, a, st);
        case 128: return chunk_launch_na<2, 1>(in_fmt, n_ant, a, st);
        case 256: return chunk_launch_na<2, 2>(in_fmt, n_ant, a, st);
        case 512: return chunk_launch_na<2, 4>(in_fmt, n_ant, a, st);
        case 1024: return chunk_launch_na<2, 8>(in_fmt, n_ant, a, st);
    }
    return OFS_EINVAL;
}

}  // extern "C"
