// rtl_smooth.h — what the one-shot and the resumable minn_rtl kernels share (aa_exact.hip
// rtl_exact_kernel, rtl_chunk.hip rtl_chunk_kernel): the int32 row prefix, the per-wave LDS layout,
// and the IIR smoothing of a 256-sample segment in its three forms (segment-parallel bit-exact float
// recursion, shift 0, floor-mode walker lane).
#pragma once
#include "ofs_common.h"

namespace ofs {

// The same row prefix on int32 values (integer-valued products of 12-bit words: a row of 64·E
// samples of one or two branches stays below 2^31), exactly the doubles' values
template <int E>
struct RowPrefixI {
    int f[E], excl, tot;
    __device__ __forceinline__ void run(const int (&v)[E]) {
        f[0] = v[0];
#pragma unroll
        for (int e = 1; e < E; ++e) f[e] = f[e - 1] + v[e];
        const int incl = scan_add_i32(f[E - 1]);
        excl = dppz_i<0x138>(incl);                   // wave_shr:1, lane 0 <- 0
        tot = __builtin_amdgcn_readlane(incl, 63);
    }
};

// ---- segment-parallel smoothing -----------------------------------------------------------
// The stream is cut into segments of SEG = 64·SC samples; lane j owns the chunk of SC samples
// [s0 + SC·j, s0 + SC·(j+1)).  The float IIR s <- s + (c - s)·2^-k (minn_rtl.py:706-715) is
// evaluated EXACTLY - the reference's sequential operation sequence, contraction off - by
// every lane over its own chunk, from an entering state that is made self-consistent:
//   1. guess: each lane maps its chunk from s = 0 and records the affine map s_out = A·s_in + Z;
//      a wave scan of the maps applied to the exact carried state gives every chunk's
//      entering state to a few ulps;
//   2. round: every lane runs the exact recursion over its chunk from its entering state; the
//      chain is consistent when each lane's entering state equals lane j-1's leaving state
//      bit for bit (lane 0 enters with the exact carried state).  Otherwise every lane takes
//      lane j-1's leaving state as its new entering state and the round repeats.
// The recursion is deterministic, so a consistent chain IS the reference's trajectory (by
// induction from lane 0).  After round r lanes 0..r are exact, so it ends within 64 rounds
// (the sequential cost); in practice the guessed trajectories coincide with the exact one
// inside a chunk or two and a segment takes a few rounds.  The integer floor-shift RTL mode
// (not contractive to the bit) runs in a walker lane per stream instead (rtl_walk).
#ifndef OFS_RTL_SC
#define OFS_RTL_SC 4
#endif
constexpr int SC = OFS_RTL_SC;
static_assert(SC % 2 == 0, "chunk stores go out as 16-byte pairs");
constexpr int SEG = 64 * SC;
constexpr int SEG_PAD = SEG + SEG / SC;                // chunk stride SC + 1 doubles (banks)
__device__ __forceinline__ int seg_at(int i) { return i + i / SC; }

// per-wave LDS: prefix rows k-3MW..k of Ae and Ac, the raw words of rows k-MW..k-1 of every
// branch (lane-private columns), the segment's corr_positive and energy_scaled
__host__ __device__ constexpr int rtl_ring_rows(int MW) { return 3 * MW + 1; }
__host__ __device__ constexpr size_t rtl_wave_lds(int E, int MW, int nb) {
    return (size_t)2 * rtl_ring_rows(MW) * E * 64 * sizeof(double) + (size_t)2 * SEG_PAD * sizeof(double) +
           (size_t)nb * MW * E * 64 * sizeof(int32_t);
}

__device__ __forceinline__ bool same_bits(double a, double b) {
    return __double_as_longlong(a) == __double_as_longlong(b);
}

// One walker lane's pass over a segment (phase B below): the reference's IIR (minn_rtl.py:706-715)
// exactly as written, branch-free per sample, SM = 0 float s += (c - s)/2^k, 1 shift 0 (s = c),
// 2 RTL floor shift; the threshold decision (:717-722) goes into the stored value's sign bit.
template <int SM>
__device__ __forceinline__ void rtl_walk(const double* __restrict__ wcp, double* __restrict__ wes, int n, int v0,
                                         double inv, double scale, int shift, double& sv, long long& siv) {
    constexpr long long SIGN = (long long)(1ull << 63);
    auto step = [&](double c, double es) -> double {
        if constexpr (SM == 0) sv = sv + (c - sv) * inv;
        else if constexpr (SM == 1) sv = c;
        else {
            const long long ci = (long long)c;
            siv = shift == 0 ? ci : siv + ((ci - siv) >> shift);
            sv = (double)siv;
        }
        return __longlong_as_double(__double_as_longlong(sv) | (sv * scale >= es ? SIGN : 0ll));
    };
    int li = 0;
    for (; li < v0; ++li) wes[seg_at(li)] = sv;                  // before metric_valid: state held
    for (; li + 8 <= n; li += 8) {
        double cb[8], eb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { cb[u] = wcp[seg_at(li + u)]; eb[u] = wes[seg_at(li + u)]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) wes[seg_at(li + u)] = step(cb[u], eb[u]);
    }
    for (; li < n; ++li) wes[seg_at(li)] = step(wcp[seg_at(li)], wes[seg_at(li)]);
}

// workgroup barrier ordering LDS only: a __syncthreads() fence would also wait for every global
// store in flight (vmcnt(0)), a store round trip per segment
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

#ifndef OFS_RTL_MAXROUNDS                   // diagnostic builds only: < 64 cuts the rounds (inexact)
#define OFS_RTL_MAXROUNDS 64
#endif
// Fast segments test the chain every OFS_RTL_RPT-th round: an untested round's hand-over
// and the tested round's are the same operation, and a consistent tested round is the
// reference trajectory as before; the test (compare, ballot, scalar branch) is what the
// group saves, at most RPT - 1 extra rounds per segment (RPT 1 / 2 / 3 / 4: cfg2b 0.048
// / 0.043 / 0.0414 / 0.0413 ms, profiles/r04t_*).
#ifndef OFS_RTL_RPT
#define OFS_RTL_RPT 4                      // rounds per consistency test on fast segments (tuning builds)
#endif

// The float IIR (shift >= 1) over one segment, lane j = chunk j: cv = the lane's corr_positive,
// upd = which of its samples update the state (metric_valid and inside the stream; elsewhere the
// state is held), sm = the exact state entering the segment, replaced by the one leaving it; own =
// the state after each of the lane's samples.  `interior`: every sample of the segment updates and
// shift <= 14.  rounds counts the speculation rounds (diagnostic builds).
// rtl_exact_kernel keeps this block inline, word for word: calling it from there changed the
// instruction stream of all 24 instantiations of that kernel (regalloc / scheduling, up to 80
// instructions either way), and the one-shot kernel is the yardstick the resumable one is measured
// against.  A change to the recursion goes into both.
__device__ __forceinline__ void rtl_float_seg(const double (&cv)[SC], const bool (&upd)[SC], int lane, bool interior,
                                              double inv, double keep, double& sm, double (&own)[SC],
                                              long long& rounds) {
#pragma clang fp contract(off)
    // 1. chunk maps from s = 0: s_out = A·s_in + Z (approximate arithmetic is fine here)
    double A = 1.0, Z = 0.0;
#pragma unroll
    for (int e = 0; e < SC; ++e) {
        if (upd[e]) {
            Z = Z + (cv[e] - Z) * inv;
            A = A * keep;
        }
    }
    // inclusive wave scan of the affine maps (lane-1's map first, then mine): DPP
    // ladder row_shr 1/2/4/8, row_bcast 15/31
    double sa = A, sz = Z;
    const int rl = lane & 15;
    auto comb = [&](double pa, double pz, bool take) {
        if (take) { sz = sa * pz + sz; sa = sa * pa; }
    };
    { const double pa = ofs::dpp_d<0x111>(sa), pz = ofs::dpp_d<0x111>(sz); comb(pa, pz, rl >= 1); }
    { const double pa = ofs::dpp_d<0x112>(sa), pz = ofs::dpp_d<0x112>(sz); comb(pa, pz, rl >= 2); }
    { const double pa = ofs::dpp_d<0x114>(sa), pz = ofs::dpp_d<0x114>(sz); comb(pa, pz, rl >= 4); }
    { const double pa = ofs::dpp_d<0x118>(sa), pz = ofs::dpp_d<0x118>(sz); comb(pa, pz, rl >= 8); }
    { const double pa = ofs::dpp_d<0x142>(sa), pz = ofs::dpp_d<0x142>(sz); comb(pa, pz, (lane & 31) >= 16); }
    { const double pa = ofs::dpp_d<0x143>(sa), pz = ofs::dpp_d<0x143>(sz); comb(pa, pz, lane >= 32); }
    // entering state of my chunk: exclusive map applied to the carried exact state
    const double ea = ofs::wave_shr1(sa, lane, 1.0), ez = ofs::wave_shr1(sz, lane, 0.0);
    double enter = lane == 0 ? sm : ea * sm + ez;
    // Interior segments (every sample updates) whose entering states are all 0 or >= 2^-700
    // run the step as fma(c - s, 2^-k, s): (c - s)·2^-k is exact (a power-of-two scaling that
    // cannot reach the subnormal range: s >= 0 shrinks by at most 2 per step, 256 steps per
    // segment, and a non-zero c - s is a multiple of ulp(s) >= 2^-752), so the fused add
    // rounds exactly as the reference's separate multiply and add do - 2 VALU per step
    // instead of 3 plus the per-sample update selects.  (States stay >= 2^-956 over the
    // segment, so |c - s| >= 2^-1008 when non-zero and the scaled value is normal for k <= 14.)
    const bool fast = interior && __ballot(!(enter == 0.0 || enter >= 0x1p-700)) == 0;
    // 2./3. exact chunk runs until the chain is self-consistent: every lane runs the
    // reference recursion over its chunk from `enter`, then takes lane-1's leaving
    // state (DPP wave_shr:1) as its new `enter`; stop when no lane's entering state
    // changes.  Lane 0 starts exact, and after round r lanes 0..r are exact: <= 64 rounds.
    if (fast) {
        for (int round = 0; round <= OFS_RTL_MAXROUNDS; round += OFS_RTL_RPT) {
            double st = enter;
#pragma unroll
            for (int r = 1; r < OFS_RTL_RPT; ++r) {            // untested rounds
#pragma unroll
                for (int e = 0; e < SC; ++e) st = fma(cv[e] - st, inv, st);
                enter = ofs::wave_shr1(st, lane, sm);
                st = enter;
            }
#pragma unroll
            for (int e = 0; e < SC; ++e) {
                st = fma(cv[e] - st, inv, st);
                own[e] = st;
            }
            const double prev_leave = ofs::wave_shr1(st, lane, sm);
            rounds += OFS_RTL_RPT;
            if (__ballot(!same_bits(enter, prev_leave)) == 0) {
                sm = readlane(st, 63);
                break;
            }
            enter = prev_leave;
        }
    } else {
        for (int round = 0; round <= OFS_RTL_MAXROUNDS; ++round) {
            double st = enter;
#pragma unroll
            for (int e = 0; e < SC; ++e) {
                if (upd[e]) st = st + (cv[e] - st) * inv;
                own[e] = st;
            }
            const double prev_leave = ofs::wave_shr1(st, lane, sm);
            ++rounds;
            if (__ballot(!same_bits(enter, prev_leave)) == 0) {
                sm = readlane(st, 63);
                break;
            }
            enter = prev_leave;
        }
    }
}

}  // namespace ofs
