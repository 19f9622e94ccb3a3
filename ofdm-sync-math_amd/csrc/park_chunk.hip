// park_chunk.hip — resumable form of the Park mirror-product metric (ofs_park_metric, corr.hip) for
// streams that arrive in chunks (ofs_park_metric_chunk): one call takes the next Tc samples of B
// streams and returns M, P, E of park.park_streaming_metric (park.py:64-114) at the stream's newest
// samples, with the running np.argmax of M (the reference's detection, park.py:161-164) carried along.
//
// THE SAME ARITHMETIC, TILE FOR TILE.  Output i (d = half + i) reads x[i+1 .. i+2·half-1] and nothing
// else, and park_tile() (park_tile.h) computes it by expressions that depend on i only through
// q = i mod OPT, the output's place among the OPT outputs of its thread.  The one-shot call starts its
// threads at i ≡ 0 (mod OPT).  A chunk call covers the outputs [lo, hi) = [max(i_first, 0), i_first + Tc),
// i_first = n_seen - 2·half + 1, and starts its tiles at OPT·floor(lo / OPT): every output keeps its q,
// runs the same FMA chains and the same energy sums, and is stored if it lies in [lo, hi).
//
// The samples before the chunk that those outputs read (at most 2·half + OPT - 2) come from a ring in
// the state, kept in the input's own format and keyed by the absolute sample index (slot g mod Hr,
// Hr = 2·half + 2·OPT rounded up to a multiple of 4: the whole staged tile of the first group, its
// unused front pad included, lies inside it).  Several workgroups of one stream read the ring and
// n_seen (tiles 0 .. (2·half + OPT - 2) / CD), so the metric kernel writes neither: a second kernel on
// the same HIP stream, one workgroup per stream, writes the chunk's newest min(Tc, Hr) samples into
// the ring, folds this call's M row into the carried peak, writes d0 and the peak outputs and advances
// (final: zeroes) the header.
//
// ONE OUTPUT MORE THAN THE REFERENCE.  The sums of output d read up to x[d+half-1], but the reference
// (and ofs_park_metric) stops at d = T - half - 1: it wants sample d + half to exist.  A chunk call
// stores output d as soon as its window is complete (n = d + half - 1), so after T samples the stream
// has the T - 2·half outputs of the one-shot call and one more, d = T - half, which a one-shot call on
// any longer stream returns.  The running peak is the reference's argmax over ITS outputs on the
// samples so far: a call's newest output waits in the header (pend_*) and joins the peak in the next
// call that brings a sample; final drops it.
//
// State of one stream (ofs_park_chunk_state_bytes = 64 + n_br·Hr·sample_bytes, all-zero = fresh):
// ParkChunkHdr (64 B), then the ring [n_br][Hr] in the input format.  There are no carried sums.
#include <type_traits>
#include "ofs_common.h"
#include "ofdmsync.h"
#include "park_tile.h"

using namespace ofs_tile;

namespace {

struct ParkChunkHdr {
    int64_t n_seen;                 // samples of this stream consumed by earlier calls
    int64_t peak_d;                 // d of the running first argmax of M (peak_kind != 0)
    double peak_v;                  // its M, widened
    int32_t peak_kind;              // 0 no output in the peak yet, 1 a number, 2 the first NaN
    int32_t pend_kind;              // the newest output (d = n_seen - half), not yet in the peak: 0 none, 1, 2
    double pend_v;                  // its M, widened
    int64_t pad[3];
};
static_assert(sizeof(ParkChunkHdr) == 64, "state header");

struct ParkChunkArgs {
    const void* x; int64_t B, Tc; int32_t nb, half, Hr;
    uint8_t* state; int64_t state_bytes;
    void* M; void* P; void* E;
    int64_t* d0; int64_t* peak_index; double* peak_value;
    int64_t ntile; int32_t fin;
};

constexpr int64_t PC_MAX_TC = (int64_t)1 << 30;
constexpr int PC_UW = 256;                                  // threads of the update kernel

__host__ __device__ constexpr int pc_sample_bytes(int fmt) { return fmt == OFS_C64 ? 8 : fmt == OFS_C128 ? 16 : 4; }
__host__ __device__ constexpr int pc_ring(int half) { return (2 * half + 2 * OPT + 3) & ~3; }

// ------------------------------------------------------------------------------------------
// metric kernel: tile blockIdx.x % ntile of stream blockIdx.x / ntile; reads the state, writes M / P / E
// ------------------------------------------------------------------------------------------
template <int FMT, class R, bool SPLIT>
__global__ __launch_bounds__(CW) void park_chunk_kernel(ParkChunkArgs a) {
    using V = typename C2<R>::T;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x / a.ntile;
    const int64_t tile = blockIdx.x - b * a.ntile;
    const int64_t Tc = a.Tc;
    const int nb = a.nb, half = a.half, Hr = a.Hr;
    const uint8_t* sp = a.state + b * a.state_bytes;
    const int64_t n_seen = reinterpret_cast<const ParkChunkHdr*>(sp)->n_seen;
    const void* ring = sp + sizeof(ParkChunkHdr);
    R* Mo = a.M ? reinterpret_cast<R*>(a.M) + b * Tc : nullptr;
    R* Po = a.P ? reinterpret_cast<R*>(a.P) + 2 * b * Tc : nullptr;
    R* Eo = a.E ? reinterpret_cast<R*>(a.E) + b * Tc : nullptr;

    // element j of the call is output i = i_first + j; the fill phase (i < 0) is +0.0
    const int64_t i_first = n_seen - 2 * (int64_t)half + 1;
    const int64_t nz = i_first >= 0 ? 0 : (-i_first < Tc ? -i_first : Tc);
    for (int64_t j = tile * CW + t; j < nz; j += a.ntile * CW) {
        if (Mo) Mo[j] = 0;
        if (Po) { Po[2 * j] = 0; Po[2 * j + 1] = 0; }
        if (Eo) Eo[j] = 0;
    }
    const int64_t lo = i_first > 0 ? i_first : 0, hi = i_first + Tc;
    const int64_t i0 = lo / OPT * OPT + tile * CD;
    if (i0 >= hi) return;                                    // whole workgroup: no output in this tile

    const int64_t n_end = n_seen + Tc;
    const int r0 = (int)(n_seen % Hr);                       // ring slot of sample n_seen
    auto load = [&](int br, int64_t g) -> V {                // sample g of [ring | chunk], zero elsewhere
        V v; v.x = 0; v.y = 0;
        if (g >= n_seen) {
            if (g < n_end) v = ld_c<FMT, R>(a.x, (b * nb + br) * Tc + (g - n_seen));
        } else if (g >= 0 && g >= n_seen - Hr) {
            int s = r0 + (int)(g - n_seen);                  // in (-Hr, Hr)
            if (s < 0) s += Hr;
            v = ld_c<FMT, R>(ring, (int64_t)br * Hr + s);
        }
        return v;
    };
    park_tile<R, SPLIT>(reinterpret_cast<V*>(smem_raw), i0, nb, half, load, lo, hi, i_first, Mo, Po, Eo);
}

// ------------------------------------------------------------------------------------------
// update kernel: one workgroup per stream, after the metric kernel
// ------------------------------------------------------------------------------------------
// running first argmax (np.argmax: the first maximal element; the first NaN wins once one appears)
struct Peak { double v; int64_t d; int kind; };
__device__ __forceinline__ bool peak_beats(const Peak& o, const Peak& m) {     // o replaces m
    if (o.kind == 0) return false;
    if (m.kind == 0) return true;
    if (o.kind != m.kind) return o.kind == 2;
    if (o.kind == 2) return o.d < m.d;
    return o.v > m.v || (o.v == m.v && o.d < m.d);
}

template <int FMT, class R>
__global__ __launch_bounds__(PC_UW) void park_chunk_update_kernel(ParkChunkArgs a) {
    using S = typename std::conditional<FMT == OFS_C64, float2, typename std::conditional<FMT == OFS_C128, double2, short2>::type>::type;
    __shared__ Peak wp[PC_UW / 64];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t Tc = a.Tc;
    const int half = a.half, Hr = a.Hr;
    uint8_t* sp = a.state + b * a.state_bytes;
    ParkChunkHdr* hdr = reinterpret_cast<ParkChunkHdr*>(sp);
    const ParkChunkHdr h = *hdr;
    const int64_t n_seen = h.n_seen;

    if (!a.fin) {                                            // the newest min(Tc, Hr) samples into the ring
        S* ring = reinterpret_cast<S*>(sp + sizeof(ParkChunkHdr));
        const int64_t cnt = Tc < Hr ? Tc : Hr;
        const int r0 = (int)((n_seen + Tc - cnt) % Hr);
        for (int br = 0; br < a.nb; ++br) {
            const S* xs = reinterpret_cast<const S*>(a.x) + (b * a.nb + br) * Tc + (Tc - cnt);
            for (int64_t j = t; j < cnt; j += PC_UW) {
                int s = r0 + (int)j;
                if (s >= Hr) s -= Hr;
                ring[(int64_t)br * Hr + s] = xs[j];
            }
        }
    }

    // The peak runs over the outputs the reference has on the samples so far, d <= n - half - 1: the
    // call's newest output (d = n - half) waits in the header until a later sample arrives.
    Peak me{0.0, 0, 0};
    const R* row = a.M ? reinterpret_cast<const R*>(a.M) + b * Tc : nullptr;
    const int64_t i_first = n_seen - 2 * (int64_t)half + 1;
    const int64_t nz = i_first >= 0 ? 0 : (-i_first < Tc ? -i_first : Tc);
    if (row) {                                               // this call's valid outputs but the newest
        for (int64_t j = nz + t; j < Tc - 1; j += PC_UW) {
            const double v = (double)row[j];
            const Peak c{v, half + i_first + j, v != v ? 2 : 1};
            if (peak_beats(c, me)) me = c;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const Peak o{__shfl_xor(me.v, m), __shfl_xor(me.d, m), __shfl_xor(me.kind, m)};
        if (peak_beats(o, me)) me = o;
    }
    if ((t & 63) == 0) wp[t >> 6] = me;
    __syncthreads();                                         // also: every thread has read the header
    if (t == 0) {
        Peak pk{h.peak_v, h.peak_d, h.peak_kind};
        const Peak pend{h.pend_v, n_seen - half, h.pend_kind};
        if (Tc > 0 && peak_beats(pend, pk)) pk = pend;
        for (int w = 0; w < PC_UW / 64; ++w)
            if (peak_beats(wp[w], pk)) pk = wp[w];
        if (a.d0) a.d0[b] = n_seen - half + 1;
        if (a.peak_index) a.peak_index[b] = pk.kind ? pk.d : -1;
        if (a.peak_value) a.peak_value[b] = pk.kind ? pk.v : 0.0;
        ParkChunkHdr o{};                                    // final: fresh again (the ring is not read)
        if (!a.fin) {
            o.n_seen = n_seen + Tc;
            o.peak_d = pk.d; o.peak_v = pk.v; o.peak_kind = pk.kind;
            if (row && Tc - 1 >= nz) {                       // (not final, so Tc >= 1)
                const double v = (double)row[Tc - 1];
                o.pend_v = v; o.pend_kind = v != v ? 2 : 1;
            }
        }
        *hdr = o;
    }
}

template <int FMT, class R>
int launch(const ParkChunkArgs& a, hipStream_t st) {
    if (a.Tc > 0) {
        // the one-shot call's choice (corr.hip park_launch): shared-window energy from half = OPT - 1 on,
        // unless variant PARK_DIRECT asks for the per-output sums
        const bool split = a.half >= OPT - 1 && !ofs::variant_on(ofs::V_PARK_DIRECT);
        auto k = split ? park_chunk_kernel<FMT, R, true> : park_chunk_kernel<FMT, R, false>;
        const size_t lds = park_tile_lds<R>(a.half);
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return OFS_EHIP;
        hipLaunchKernelGGL(k, dim3((unsigned)(a.B * a.ntile)), dim3(CW), lds, st, a);
        if (hipGetLastError() != hipSuccess) return OFS_EHIP;
    }
    hipLaunchKernelGGL((park_chunk_update_kernel<FMT, R>), dim3((unsigned)a.B), dim3(PC_UW), 0, st, a);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}

// the supported (format, precision) pairs and shapes
bool shape_ok(int in_fmt, int n_br, int N) {
    if (n_br < 1 || N / 2 < 1) return false;
    switch (in_fmt) {
        case OFS_C64: return N <= 8190;                      // fp32: the one-shot call's LDS limit
        case OFS_C128: case OFS_CI16: return N <= 4094;      // fp64
    }
    return false;
}
int pair_precision(int in_fmt) { return in_fmt == OFS_C64 ? OFS_FP32 : OFS_FP64; }

}  // namespace

extern "C" {

int64_t ofs_park_chunk_state_bytes(int32_t in_fmt, int32_t n_br, int32_t N) {
    if (!shape_ok(in_fmt, n_br, N)) return OFS_EINVAL;
    return (int64_t)sizeof(ParkChunkHdr) + (int64_t)n_br * pc_ring(N / 2) * pc_sample_bytes(in_fmt);
}

int64_t ofs_park_chunk_max_samples(int32_t in_fmt, int32_t n_br, int32_t N) {
    if (!shape_ok(in_fmt, n_br, N)) return OFS_EINVAL;
    return PC_MAX_TC;
}

int32_t ofs_park_metric_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                              int32_t N, int32_t precision, void* state,
                              void* M, void* P, void* E, int64_t* d0,
                              int64_t* peak_index, double* peak_value,
                              int32_t final, void* stream) {
    if (!shape_ok(in_fmt, n_br, N) || precision != pair_precision(in_fmt) || B < 0 || Tc < 0 || Tc > PC_MAX_TC ||
        (Tc == 0 && !final) || OFS_MISSING(state, B) || (reinterpret_cast<uintptr_t>(state) & 15) != 0 ||
        OFS_MISSING(x, B * Tc) || (!M && (peak_index || peak_value) && B * Tc > 0))
        return OFS_EINVAL;
    if (B == 0) return OFS_OK;
    ParkChunkArgs a{};
    a.x = x; a.B = B; a.Tc = Tc; a.nb = n_br; a.half = N / 2; a.Hr = pc_ring(N / 2);
    a.state = reinterpret_cast<uint8_t*>(state);
    a.state_bytes = ofs_park_chunk_state_bytes(in_fmt, n_br, N);
    a.M = M; a.P = P; a.E = E; a.d0 = d0; a.peak_index = peak_index; a.peak_value = peak_value;
    a.ntile = (Tc + OPT - 1 + CD - 1) / CD;                  // outputs [OPT·floor(lo / OPT), hi): at most Tc + OPT - 1
    a.fin = final != 0;
    if (B > 0x7fffffffll || B * a.ntile > 0x7fffffffll) return OFS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    switch (in_fmt) {
        case OFS_C64: return launch<OFS_C64, float>(a, st);
        case OFS_C128: return launch<OFS_C128, double>(a, st);
        default: return launch<OFS_CI16, double>(a, st);
    }
}

}  // extern "C"
