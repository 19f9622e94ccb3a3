// zc_tiles.h — what the one-shot and the resumable zc_v2 CFAR + gate kernels share (zc_cfar.hip
// zc_cfar_kernel, zc_chunk.hip zc_chunk_kernel): the tile geometry, the walker's recursion over one
// chunk, the gate record, the helpers' row stores and the LDS-only barrier of the register-staged form.
// Every piece here leaves the three zc_cfar_kernel builds and zc_chunk_kernel with the instruction text
// and .amdhsa_ directives of its inline form (tools/kernel_text.py, profiles/zc_refactor_isa.txt).
// What differs between the kernels stays in them, cross-referenced there.
#pragma once
#include "ofs_common.h"

namespace ofs {

// streams per workgroup (walker lanes) and helper waves: LDS-DMA path 16 streams, 11 helpers (one
// workgroup of 12 waves per CU, 154 VGPRs = 3 waves/SIMD; round 5, paired builds on zc_detect: 7 / 8 /
// 11 / 15 helpers 0.306 / 0.289 / 0.286 / 0.492 ms, profiles/r05p_zc_cfar_helpers_ab.txt; static LDS (4 + 3 + 2) x 16 x 130 doubles = 149,760 B = 146.25 KiB of
// gfx950's 160 KiB, asserted in the kernel); register path 8 streams, 3 helpers ((3 + 2 + 2) x 8 x
// 130 doubles = 57 KiB; its staging registers scale with the stream count).  zc_chunk_kernel is built
// on the register path's geometry.
constexpr int ZS_DMA = 16, ZH_DMA = 11;
constexpr int ZS_REG = 8, ZH_REG = 3;
constexpr int ZR = 2;             // 64-sample rows of the gate machine per chunk
constexpr int ZC = 64 * ZR;       // samples per chunk
constexpr int ZP = ZC + 2;        // LDS row pitch in doubles (16-byte rows; walker column reads spread over banks)

// per-stream gate state, wave-uniform in the helper wave that owns the stream
struct ZcGate {
    int64_t last_above;     // last above sample (one-shot: < current row, -1 if none; resumable: absolute)
    int64_t gs, pk;
    double pv;
    int open, nev;
};

// state / mask stores of the helpers: non-temporal (streamed past the caches; nothing here reads
// them back).  r05av, bit-identical: state arrays 0.63 -> 0.56 ms, events + mask unchanged (0.286)
template <class T>
__device__ __forceinline__ void zc_st(T* p, T v) { __builtin_nontemporal_store(v, p); }

// one sample's row of the state arrays and masks at offset o of the [B][n] outputs (A: ZcArgs /
// ZcChunkArgs; null arrays are not stored)
template <class A>
__device__ __forceinline__ void zc_store(const A& a, int64_t o, double ls, double cs, double th, uint8_t ab,
                                         uint8_t vd, uint8_t mk) {
    if (a.local_sum) zc_st(&a.local_sum[o], ls);
    if (a.corr_scaled) zc_st(&a.corr_scaled[o], cs);
    if (a.thresh_scaled) zc_st(&a.thresh_scaled[o], th);
    if (a.above) zc_st(&a.above[o], ab);
    if (a.valid) zc_st(&a.valid[o], vd);
    if (a.gate_mask) zc_st(&a.gate_mask[o], mk);
}

// the CFAR decision of one 64-sample row (zc_v2.py:300-346), non-short-circuit (no exec-mask branch per
// term): the lanes whose sample is `live` (inside the stream, metric_valid) and above both thresholds
template <class A>
__device__ __forceinline__ uint64_t zc_above(const A& a, bool live, double c, double ls) {
    return __ballot(live & (c * a.scale >= ls * a.tv) & (c >= a.minmag));
}

// open gate: the peak over the row's lanes `in` (first maximum, strict >: an earlier row's peak stays).
// zc_cfar_kernel's two updates; zc_chunk_kernel keeps its own copy (it compiled one instruction shorter
// with this one and a short push measured slower, see there)
__device__ __forceinline__ void zc_peak(ZcGate& G, bool in, double c, int64_t base) {
    const double m = wave_max(in ? c : -__builtin_huge_val());
    if (m > G.pv) {
        const uint64_t at = __ballot(in && c == m);
        G.pv = m; G.pk = base + __builtin_ctzll(at);
    }
}

// event record G.nev of stream b = (peak, gate_start, gate_end, detected_start) from lanes 0-3, and the
// peak's magnitude; a record past max_ev is counted and not stored.  A macro, the one form that keeps
// the four kernels' instruction text: as a template function taking (a, b, nev, pk, gs, end, pv, lane) by
// value the three zc_cfar_kernel builds went 3999 -> 4005, 3886 -> 3928, 4981 -> 5338 instructions and
// zc_chunk_kernel 8572 -> 8774; taking the gate by reference they moved as well.
#define ZC_EVENT(a, G, b, end, lane)                                                                     \
    do {                                                                                                 \
        if ((a).ev && (G).nev < (a).max_ev && (lane) < 4) {                                              \
            int64_t* r_ = (a).ev + ((b) * (int64_t)(a).max_ev + (G).nev) * 4;                            \
            const int64_t ds_ = (G).pk - (a).reflen + 1 > 0 ? (G).pk - (a).reflen + 1 : 0;               \
            r_[lane] = (lane) == 0 ? (G).pk : (lane) == 1 ? (G).gs : (lane) == 2 ? (end) : ds_;          \
            if ((lane) == 0 && (a).ev_v) (a).ev_v[(b) * (int64_t)(a).max_ev + (G).nev] = (G).pv;         \
        }                                                                                                \
        (G).nev += 1;                                                                                    \
    } while (0)

// walker: the exact left-to-right recursion of RunningSum.step over one full chunk of this lane's
// stream; LDS reads a batch of ZB samples ahead of the dependent adds (the chain is 2 v_add_f64 per
// sample; an LDS round trip per sample would set the pace instead).  OZ: c[i-W] is 0 (window not yet
// full; the resumable kernel's history ring makes that case zeros in o instead).
template <int ZCN, bool OZ>
__device__ __forceinline__ void zc_walk_chunk(const double* x, const double* o, double* r, double& acc) {
#pragma clang fp contract(off)
    constexpr int ZB = 8;
    double2 xv[ZB / 2], ov[ZB / 2];
#pragma unroll
    for (int j = 0; j < ZB / 2; ++j) {
        xv[j] = reinterpret_cast<const double2*>(x)[j];
        if (!OZ) ov[j] = reinterpret_cast<const double2*>(o)[j];
    }
#pragma unroll
    for (int bb = 0; bb < ZCN / ZB; ++bb) {
        double2 xn[ZB / 2], on[ZB / 2];
        if (bb + 1 < ZCN / ZB) {
#pragma unroll
            for (int j = 0; j < ZB / 2; ++j) {
                xn[j] = reinterpret_cast<const double2*>(x + (bb + 1) * ZB)[j];
                if (!OZ) on[j] = reinterpret_cast<const double2*>(o + (bb + 1) * ZB)[j];
            }
        }
#pragma unroll
        for (int j = 0; j < ZB / 2; ++j) {
            double2 rr;
            if (OZ) {
                acc = acc + xv[j].x; rr.x = acc;
                acc = acc + xv[j].y; rr.y = acc;
            } else {
                acc = (acc + xv[j].x) - ov[j].x; rr.x = acc;
                acc = (acc + xv[j].y) - ov[j].y; rr.y = acc;
            }
            reinterpret_cast<double2*>(r + bb * ZB)[j] = rr;
        }
        if (bb + 1 < ZCN / ZB) {
#pragma unroll
            for (int j = 0; j < ZB / 2; ++j) { xv[j] = xn[j]; if (!OZ) ov[j] = on[j]; }
        }
    }
}

// LDS-only barrier of the register-staged tiles: the helpers' global stores are never waited for (a
// __syncthreads() fence would drain them, a full store round trip per chunk); the loads are staged one
// iteration after they are issued, so their wait overlaps a whole chunk of work
__device__ __forceinline__ void zc_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

}  // namespace ofs
