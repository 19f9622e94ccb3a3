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
#include "chunk_state.h"
#include "park_tile.h"

using namespace ofs_tile;
using namespace ofs_chunk;

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
            v = ld_c<FMT, R>(ring, (int64_t)br * Hr + ring_slot(r0, g - n_seen, Hr));
        }
        return v;
    };
    park_tile<R, SPLIT>(reinterpret_cast<V*>(smem_raw), i0, nb, half, load, lo, hi, i_first, Mo, Po, Eo);
}

// ------------------------------------------------------------------------------------------
// update kernel: one workgroup per stream, after the metric kernel
// ------------------------------------------------------------------------------------------
template <int FMT, class R>
__global__ __launch_bounds__(PC_UW) void park_chunk_update_kernel(ParkChunkArgs a) {
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t Tc = a.Tc;
    const int half = a.half;
    uint8_t* sp = a.state + b * a.state_bytes;
    ParkChunkHdr* hdr = reinterpret_cast<ParkChunkHdr*>(sp);
    const ParkChunkHdr h = *hdr;
    const int64_t n_seen = h.n_seen;

    if (!a.fin) ring_write<FMT, PC_UW>(sp + sizeof(ParkChunkHdr), a.x, b, a.nb, Tc, n_seen, a.Hr, t);

    // The peak runs over the outputs the reference has on the samples so far, d <= n - half - 1: the
    // call's newest output (d = n - half) waits in the header until a later sample arrives.
    const R* row = a.M ? reinterpret_cast<const R*>(a.M) + b * Tc : nullptr;
    const int64_t i_first = n_seen - 2 * (int64_t)half + 1;
    const int64_t nz = i_first >= 0 ? 0 : (-i_first < Tc ? -i_first : Tc);
    ChunkPeak me{0.0, 0, 0};
    if (row) me = row_peak<PC_UW, 1>(row, nz, Tc - 1, half + i_first, t);     // this call's valid outputs but the newest
    ChunkPeak pk{h.peak_v, h.peak_d, h.peak_kind};
    const ChunkPeak pend{h.pend_v, n_seen - half, h.pend_kind};
    if (Tc > 0 && peak_beats(pend, pk)) pk = pend;
    pk = peak_fold<PC_UW>(me, pk, t);
    if (t == 0) {
        if (a.d0) a.d0[b] = n_seen - half + 1;
        if (a.peak_index) a.peak_index[b] = pk.kind ? pk.i : -1;
        if (a.peak_value) a.peak_value[b] = pk.kind ? pk.v : 0.0;
        ParkChunkHdr o{};                                    // final: fresh again (the ring is not read)
        if (!a.fin) {
            o.n_seen = n_seen + Tc;
            o.peak_d = pk.i; o.peak_v = pk.v; o.peak_kind = pk.kind;
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
    return (int64_t)sizeof(ParkChunkHdr) + (int64_t)n_br * pc_ring(N / 2) * sample_bytes(in_fmt);
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
    if (!shape_ok(in_fmt, n_br, N) || precision != pair_precision(in_fmt) ||
        chunk_args_bad(B, Tc, PC_MAX_TC, final, state, x) || (!M && (peak_index || peak_value) && B * Tc > 0))
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
