// frame_capture.hip — resumable frame capture for streams that arrive in chunks (ofs_frame_capture_chunk):
// the link between the chunk-fed detectors, which report an event after its samples have left, and the
// receiver back-end, which wants the frame's samples resident.  One call takes the next Tc samples of B
// streams and a list of trigger indices per stream (read on the device, e.g. a detector's frame_start
// column of the same push) and emits every frame [s, s + F) whose last sample has arrived, in the
// input's own format, bit for bit.
//
// State of one stream (ofs_frame_capture_state_bytes = 192 + n_br·Hr·sample_bytes, all-zero = fresh):
// FcHdr (192 B: n_seen, the queue of pending starts), then the ring [n_br][Hr] of chunk_state.h, sample
// g at slot g mod Hr.  Hr is `history` rounded up to whole 16-byte words; the rounding is storage only:
// a trigger is late by `history`, never by Hr.
//
// RETRIEVABLE WHEN COMPLETE.  A start s is queued only if s >= n0 - H (n0: samples before that call).  If
// it completes in the same call, its samples lie in [ring | chunk] of that call.  If it completes in a
// later call with n0' samples before it, it was incomplete at the end of the call before, s + F > n0', so
// s > n0' - F >= n0' - H: still in the ring, which holds the last min(n0', Hr) >= min(n0', H) samples.
//
// Two launches per call, as in park_chunk.hip: the gather reads [ring | chunk] and writes the frames'
// sample words; then one workgroup per stream writes the chunk's newest samples into the ring, the
// bookkeeping outputs and the header.  Both recompute the call's small queue decision (fc_decide) from the
// old header and the triggers; only the second kernel writes the state.
//
// COMPACT FORM (ofs_frame_capture_compact): the same capture, the frames written densely.  The frame of
// stream b in slot j goes to row row0[b] + j of frames [cap][n_br][F], row0 the exclusive prefix sum of the
// streams' frame counts, so the rows are in (stream, slot) order and their number lies in device memory
// (n_rows) for ofs_rx_backend_counted.  Two small kernels run first: a thread per stream counts the frames
// the call will emit (fc_count: fc_decide's count alone) into n_frames, then ONE workgroup walks n_frames
// in blocks of FC_SCAN_BLK, four streams per thread, scans each block and carries the running total in 64
// bits; no workgroup waits on another and the result does not depend on timing.  The gather and update
// kernels are the slot form's with another destination row (template flag CMP, an argument struct of its
// own: the slot form's instantiations keep their text); rows at or beyond cap are not written, their
// frames are lost.
#include <algorithm>
#include "chunk_state.h"

using namespace ofs_chunk;

namespace {

constexpr int FC_QMAX = 16;                                   // max_pending
constexpr int FC_NT = 256;                                    // threads of both kernels
constexpr int FC_GMAX = 16;                                   // gather workgroups per stream, at most
constexpr int FC_UL = 4;                                      // 16-byte words per gather thread and round
constexpr int FC_CNT_NT = 64;                                 // threads of a count workgroup (a thread per stream)
constexpr int FC_SCAN_NT = 1024;                              // threads of the scanning workgroup
constexpr int FC_SCAN_PT = 4;                                 // streams per thread and block
constexpr int FC_SCAN_BLK = FC_SCAN_NT * FC_SCAN_PT;          // streams per block of the scan
constexpr int64_t FC_HMAX = ((int64_t)1 << 30) - 4;           // history (ring_write's int slot arithmetic)

struct FcHdr {
    int64_t n_seen;                 // samples of this stream consumed by earlier calls
    int32_t n_pend;                 // queued starts whose frame is not complete yet
    int32_t pad0;
    int64_t pend[FC_QMAX];          // the queue, oldest first
    int64_t pad[6];
};
static_assert(sizeof(FcHdr) == 192, "state header");

struct FcArgs {
    const void* x; int64_t B, Tc; int32_t nb, F, H, Hr, Q;
    int64_t offset;
    const int64_t* trig; int64_t trig_ld, trig_stride; const int32_t* n_trig; int32_t trig_max;
    uint8_t* state; int64_t state_bytes;
    void* frames; int64_t* frame_start; int32_t* n_frames; int32_t* dropped;
    int32_t G, fin;
};

// ofs_frame_capture_compact: dense rows.  A kernel argument type of its own: the slot form keeps its own.
struct FcArgsC : FcArgs { int64_t cap; int32_t* frame_stream; int32_t* row0; int32_t* n_rows; };
template <bool CMP> struct FcArgsOf { using T = FcArgs; };
template <> struct FcArgsOf<true> { using T = FcArgsC; };

__host__ __device__ constexpr int fc_ring(int fmt, int H) {
    const int vs = 16 / sample_bytes(fmt);
    return (H + vs - 1) / vs * vs;
}

// what one call does to one stream's queue
struct FcDecision {
    int64_t emit[FC_QMAX];          // starts of the frames this call writes, slot order
    int64_t keep[FC_QMAX];          // starts still pending after the call
    int32_t ne, nk, late, full;
};

__device__ __forceinline__ int fc_trig_count(const FcArgs& a, int64_t b) {
    if (!a.n_trig) return 0;
    const int k = a.n_trig[b];
    return k < 0 ? 0 : (k < a.trig_max ? k : a.trig_max);
}

// The decision of stream b, by thread 0 into LDS; ends with a barrier.  Triggers in index order: late
// (before max(0, n0 - H)), queue full, or appended; then the queue in order: complete frames leave it.
__device__ __forceinline__ void fc_decide(const FcArgs& a, int64_t b, const FcHdr* hdr, int k, FcDecision* d) {
    if (threadIdx.x == 0) {
        const int64_t n0 = hdr->n_seen, n1 = n0 + a.Tc;
        const int64_t oldest = n0 > a.H ? n0 - a.H : 0;
        int np = hdr->n_pend < 0 ? 0 : (hdr->n_pend < a.Q ? hdr->n_pend : a.Q);   // (a state of other arguments: in bounds)
        for (int i = 0; i < np; ++i) d->keep[i] = hdr->pend[i];
        int late = 0, full = 0;
        for (int j = 0; j < k; ++j) {
            const int64_t s = a.trig[b * a.trig_ld + j * a.trig_stride] + a.offset;
            if (s < oldest) ++late;
            else if (np >= a.Q) ++full;
            else d->keep[np++] = s;
        }
        int ne = 0, nk = 0;
        for (int i = 0; i < np; ++i) {                        // (nk <= i: the compaction never overtakes the read)
            const int64_t s = d->keep[i];
            if (s + a.F <= n1) d->emit[ne++] = s;
            else d->keep[nk++] = s;
        }
        d->ne = ne; d->nk = nk; d->late = late; d->full = full;
    }
    __syncthreads();
}

// fc_decide's ne alone, by one thread without LDS (the count kernel): the same three-way test
// per trigger, the same completion test per queued start
__device__ __forceinline__ int fc_count(const FcArgs& a, int64_t b, const FcHdr* hdr, int k) {
    const int64_t n0 = hdr->n_seen, n1 = n0 + a.Tc;
    const int64_t oldest = n0 > a.H ? n0 - a.H : 0;
    int np = hdr->n_pend < 0 ? 0 : (hdr->n_pend < a.Q ? hdr->n_pend : a.Q);
    int ne = 0;
    for (int i = 0; i < np; ++i) ne += hdr->pend[i] + a.F <= n1;
    for (int j = 0; j < k; ++j) {
        const int64_t s = a.trig[b * a.trig_ld + j * a.trig_stride] + a.offset;
        if (s >= oldest && np < a.Q) {
            ++np;
            ne += s + a.F <= n1;
        }
    }
    return ne;
}

__device__ __forceinline__ int32_t fc_clamp32(int64_t v) { return v > INT32_MAX ? INT32_MAX : (int32_t)v; }

// ------------------------------------------------------------------------------------------
// count and scan kernels (compact form), before the gather; they write n_frames, row0 and n_rows
// ------------------------------------------------------------------------------------------
// The count: a thread per stream, small workgroups spread over the CUs.  Most streams, most pushes: two
// loads (n_pend, the trigger count) and no frame.  The header reads are one cache line per stream, each in
// another page (the state's stride); done by the ONE scanning workgroup they took 10 - 12 us at 4096
// streams, bound by one CU's memory pipeline, so they are a launch of their own.
__global__ __launch_bounds__(FC_CNT_NT) void frame_count_kernel(FcArgsC a) {
    const int64_t b = (int64_t)blockIdx.x * FC_CNT_NT + threadIdx.x;
    if (b >= a.B) return;
    const FcHdr* hdr = reinterpret_cast<const FcHdr*>(a.state + b * a.state_bytes);
    const int k = fc_trig_count(a, b);
    a.n_frames[b] = (hdr->n_pend != 0 || k != 0) ? fc_count(a, b, hdr, k) : 0;
}

// The scan: ONE workgroup walks n_frames in blocks of FC_SCAN_BLK, thread t takes the FC_SCAN_PT consecutive
// streams b0 + PT·t + u.  The threads' sums are scanned (wave ladder, then the 16 wave totals through LDS)
// and the running total of the blocks before, kept in 64 bits and equal in every thread, is added.  Only
// what is stored is clamped.  B = 0 (no update kernel follows): the -1 fill of every row is done here.
__global__ __launch_bounds__(FC_SCAN_NT) void frame_scan_kernel(FcArgsC a) {
    __shared__ int32_t wtot[FC_SCAN_NT / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t total = 0;
    for (int64_t b0 = 0; b0 < a.B; b0 += FC_SCAN_BLK) {
        const int64_t bt = b0 + (int64_t)t * FC_SCAN_PT;          // this thread's first stream
        int c[FC_SCAN_PT];
        int sum = 0;
#pragma unroll
        for (int u = 0; u < FC_SCAN_PT; ++u) {
            c[u] = bt + u < a.B ? a.n_frames[bt + u] : 0;
            sum += c[u];
        }
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        int before = 0, block = 0;
#pragma unroll
        for (int i = 0; i < FC_SCAN_NT / 64; ++i) {
            const int v = wtot[i];
            before += i < w ? v : 0;
            block += v;
        }
        __syncthreads();                                          // (wtot is written again by the next block)
        int64_t run = total + before + incl - sum;
#pragma unroll
        for (int u = 0; u < FC_SCAN_PT; ++u) {
            if (bt + u < a.B) a.row0[bt + u] = fc_clamp32(run);
            run += c[u];
        }
        total += block;
    }
    if (t == 0 && a.n_rows) {
        a.n_rows[0] = (int32_t)(total < a.cap ? total : a.cap);
        a.n_rows[1] = fc_clamp32(total > a.cap ? total - a.cap : 0);
    }
    if (a.B == 0)
        for (int64_t r = t; r < a.cap; r += FC_SCAN_NT) {
            if (a.frame_start) a.frame_start[r] = -1;
            if (a.frame_stream) a.frame_stream[r] = -1;
        }
}

// ------------------------------------------------------------------------------------------
// gather kernel: workgroup blockIdx.x % G of stream blockIdx.x / G; reads the state, writes sample words
// ------------------------------------------------------------------------------------------
// A row (one branch of one frame) is written in 16-byte words of the DESTINATION: word v holds the row's
// samples [v·VS - lead, v·VS - lead + VS), lead = the row's first sample's place in its 16-byte word.  A
// word that lies inside the row is one 16-byte store; the row's first and last words may be partial and
// go sample by sample.  The source is read sample by sample: s is arbitrary, so it has no alignment.  A
// thread loads FC_UL words before it stores them: a frame that only a few workgroups copy (few streams
// emit in a push) is a chain of memory latencies, one per round.
template <int FMT, bool CMP = false>
__global__ __launch_bounds__(FC_NT) void frame_gather_kernel(typename FcArgsOf<CMP>::T a) {
    using S = typename Sample<FMT>::T;
    constexpr int VS = 16 / (int)sizeof(S);
    struct alignas(16) Word { S s[VS]; };
    __shared__ FcDecision dec;
    const int64_t b = blockIdx.x / a.G;
    const int g = (int)(blockIdx.x - b * a.G);
    const uint8_t* sp = a.state + b * a.state_bytes;
    const FcHdr* hdr = reinterpret_cast<const FcHdr*>(sp);
    const int k = fc_trig_count(a, b);
    if (hdr->n_pend == 0 && k == 0) return;                   // (uniform) most streams, most pushes
    fc_decide(a, b, hdr, k, &dec);
    const int ne = dec.ne;
    if (ne == 0) return;

    const int nb = a.nb, F = a.F, Hr = a.Hr;
    const int64_t Tc = a.Tc, n0 = hdr->n_seen;
    const S* ring = reinterpret_cast<const S*>(sp + sizeof(FcHdr));
    const S* xs = static_cast<const S*>(a.x);
    S* out = static_cast<S*>(a.frames);
    int64_t row0 = 0;                                             // (compact form) the stream's first row
    if constexpr (CMP) row0 = a.row0[b];
    for (int r = 0; r < ne * nb; ++r) {
        const int slot = r / nb, br = r - slot * nb;
        if constexpr (CMP)
            if (row0 + slot >= a.cap) break;                      // no row left: this frame and the later ones are lost
        const int64_t s = dec.emit[slot];
        const int rs = (int)(s % Hr);                         // ring slot of the row's first sample (s >= 0)
        const S* rrow = ring + (int64_t)br * Hr;
        const S* xrow = xs + (b * nb + br) * Tc - n0;         // sample g of the chunk at xrow[g], g >= n0
        S* orow = out + (((CMP ? row0 : b * a.Q) + slot) * nb + br) * (int64_t)F;
        const int lead = (int)((reinterpret_cast<uintptr_t>(orow) & 15) / sizeof(S));
        const int nw = (lead + F + VS - 1) / VS;
        auto src = [&](int i) -> const S* {                   // where sample s + i of [ring | chunk] lies, 0 <= i < F
            const int64_t gi = s + i;
            int q = rs + i;                                   // i < F <= Hr: one wrap at most
            if (q >= Hr) q -= Hr;
            return gi >= n0 ? xrow + gi : rrow + q;           // (an address select: the loads stay unconditional)
        };
        for (int v0 = g * FC_NT * FC_UL + threadIdx.x; v0 < nw; v0 += a.G * FC_NT * FC_UL) {
            S w[FC_UL][VS];
#pragma unroll
            for (int u = 0; u < FC_UL; ++u) {                 // a round's loads first: FC_UL words in flight per lane
                const int i0 = (v0 + u * FC_NT) * VS - lead;
#pragma unroll
                for (int e = 0; e < VS; ++e) {                // (a sample outside the row: read the nearest one inside,
                    const int i = i0 + e;                     // never stored)
                    w[u][e] = *src(i < 0 ? 0 : (i < F ? i : F - 1));
                }
            }
#pragma unroll
            for (int u = 0; u < FC_UL; ++u) {                 // (a word past the row: no sample of it passes the test)
                const int i0 = (v0 + u * FC_NT) * VS - lead;
                if (i0 >= 0 && i0 + VS <= F) {
                    Word t;
#pragma unroll
                    for (int e = 0; e < VS; ++e) t.s[e] = w[u][e];
                    *reinterpret_cast<Word*>(orow + i0) = t;
                } else {
#pragma unroll
                    for (int e = 0; e < VS; ++e)
                        if (i0 + e >= 0 && i0 + e < F) orow[i0 + e] = w[u][e];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// update kernel: one workgroup per stream, after the gather
// ------------------------------------------------------------------------------------------
template <int FMT, bool CMP = false>
__global__ __launch_bounds__(FC_NT) void frame_update_kernel(typename FcArgsOf<CMP>::T a) {
    __shared__ FcDecision dec;
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    uint8_t* sp = a.state + b * a.state_bytes;
    FcHdr* hdr = reinterpret_cast<FcHdr*>(sp);
    const int64_t n_seen = hdr->n_seen;
    fc_decide(a, b, hdr, fc_trig_count(a, b), &dec);          // (its barrier: every read of the header is done)
    if (!a.fin) ring_write<FMT, FC_NT>(sp + sizeof(FcHdr), a.x, b, a.nb, a.Tc, n_seen, a.Hr, t);
    if constexpr (CMP) {
        const int64_t row = (int64_t)a.row0[b] + t;               // (row0 clamped: then at or beyond cap)
        if (t < dec.ne && row < a.cap) {
            a.frame_start[row] = dec.emit[t];
            a.frame_stream[row] = (int32_t)b;
        }
        // the rows no frame of this call took, shared out over the workgroups
        for (int64_t r = a.n_rows[0] + b * FC_NT + t; r < a.cap; r += a.B * FC_NT) {
            a.frame_start[r] = -1;
            a.frame_stream[r] = -1;
        }
    } else {
        if (t < a.Q) a.frame_start[b * a.Q + t] = t < dec.ne ? dec.emit[t] : -1;
    }
    if (t < FC_QMAX) hdr->pend[t] = (!a.fin && t < dec.nk) ? dec.keep[t] : 0;
    if (t == 0) {
        a.n_frames[b] = dec.ne;
        a.dropped[3 * b + 0] = dec.late;
        a.dropped[3 * b + 1] = dec.full;
        a.dropped[3 * b + 2] = a.fin ? dec.nk : 0;           // cut by the stream's end
        hdr->n_seen = a.fin ? 0 : n_seen + a.Tc;              // final: fresh again (the ring is not read)
        hdr->n_pend = a.fin ? 0 : dec.nk;
        hdr->pad0 = 0;
    }
}

template <int FMT, bool CMP>
int launch(const typename FcArgsOf<CMP>::T& a, hipStream_t st) {
    if constexpr (CMP) {
        if (a.B > 0) {
            hipLaunchKernelGGL(frame_count_kernel, dim3((unsigned)((a.B + FC_CNT_NT - 1) / FC_CNT_NT)), dim3(FC_CNT_NT), 0,
                               st, a);
            if (hipGetLastError() != hipSuccess) return OFS_EHIP;
        }
        hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(FC_SCAN_NT), 0, st, a);
        if (hipGetLastError() != hipSuccess) return OFS_EHIP;
        if (a.B == 0) return OFS_OK;
    }
    hipLaunchKernelGGL((frame_gather_kernel<FMT, CMP>), dim3((unsigned)(a.B * a.G)), dim3(FC_NT), 0, st, a);
    if (hipGetLastError() != hipSuccess) return OFS_EHIP;
    hipLaunchKernelGGL((frame_update_kernel<FMT, CMP>), dim3((unsigned)a.B), dim3(FC_NT), 0, st, a);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}

bool shape_ok(int in_fmt, int n_br, int64_t F, int64_t H, int Q) {
    return (in_fmt == OFS_C64 || in_fmt == OFS_C128 || in_fmt == OFS_CI16) && n_br >= 1 && F >= 1 && H >= F &&
           H <= FC_HMAX && Q >= 1 && Q <= FC_QMAX;
}

// both entry points: the slot form (cmp == nullptr) or the compact form with its own outputs in *cmp
int32_t capture(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc, int32_t frame_len,
                int32_t history, int32_t max_pending, int64_t offset, const int64_t* trig, int64_t trig_ld,
                int64_t trig_stride, const int32_t* n_trig, int32_t trig_max, void* state, void* frames,
                int64_t* frame_start, int32_t* n_frames, int32_t* dropped, int32_t final, const FcArgsC* cmp,
                void* stream) {
    if (chunk_args_bad(B, Tc, INT64_MAX / (B > 0 ? B : 1), final, state, x) ||
        !shape_ok(in_fmt, n_br, frame_len, history, max_pending) || trig_max < 0 ||
        (n_trig && trig_max > 0 && !trig) || OFS_MISSING(frames, B) || OFS_MISSING(frame_start, B) ||
        OFS_MISSING(n_frames, B) || OFS_MISSING(dropped, B) ||
        (reinterpret_cast<uintptr_t>(frames) & (sample_bytes(in_fmt) - 1)) != 0)
        return OFS_EINVAL;
    if (cmp && (cmp->cap < 1 || cmp->cap > INT32_MAX || OFS_MISSING(cmp->frame_stream, B) ||
                OFS_MISSING(cmp->row0, B) || OFS_MISSING(cmp->n_rows, B)))
        return OFS_EINVAL;
    if (B == 0 && !(cmp && (cmp->n_rows || frame_start || cmp->frame_stream))) return OFS_OK;
    FcArgsC a{};
    if (cmp) a = *cmp;
    a.x = x; a.B = B; a.Tc = Tc; a.nb = n_br; a.F = frame_len; a.H = history; a.Hr = fc_ring(in_fmt, history);
    a.Q = max_pending; a.offset = offset;
    a.trig = trig; a.trig_ld = trig_ld; a.trig_stride = trig_stride; a.n_trig = n_trig; a.trig_max = trig_max;
    a.state = reinterpret_cast<uint8_t*>(state);
    a.state_bytes = ofs_frame_capture_state_bytes(in_fmt, n_br, frame_len, history, max_pending);
    a.frames = frames; a.frame_start = frame_start; a.n_frames = n_frames; a.dropped = dropped;
    // gather workgroups per stream: one per 64 KiB of the frames a call can emit (4 rounds of FC_UL words per
    // thread), FC_GMAX at most; few, because in most pushes all of them only read the header and leave
    const int64_t bytes = (int64_t)max_pending * n_br * frame_len * sample_bytes(in_fmt);
    a.G = (int)std::min<int64_t>(FC_GMAX, std::max<int64_t>(1, (bytes + 65535) / 65536));
    a.fin = final != 0;
    if (B * a.G > 0x7fffffffll) return OFS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (cmp) {
        switch (in_fmt) {
            case OFS_C64: return launch<OFS_C64, true>(a, st);
            case OFS_C128: return launch<OFS_C128, true>(a, st);
            default: return launch<OFS_CI16, true>(a, st);
        }
    }
    switch (in_fmt) {
        case OFS_C64: return launch<OFS_C64, false>(a, st);
        case OFS_C128: return launch<OFS_C128, false>(a, st);
        default: return launch<OFS_CI16, false>(a, st);
    }
}

}  // namespace

extern "C" {

int64_t ofs_frame_capture_state_bytes(int32_t in_fmt, int32_t n_br, int32_t frame_len, int32_t history,
                                      int32_t max_pending) {
    if (!shape_ok(in_fmt, n_br, frame_len, history, max_pending)) return OFS_EINVAL;
    return (int64_t)sizeof(FcHdr) + (int64_t)n_br * fc_ring(in_fmt, history) * sample_bytes(in_fmt);
}

int32_t ofs_frame_capture_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                                int32_t frame_len, int32_t history, int32_t max_pending, int64_t offset,
                                const int64_t* trig, int64_t trig_ld, int64_t trig_stride,
                                const int32_t* n_trig, int32_t trig_max, void* state,
                                void* frames, int64_t* frame_start, int32_t* n_frames, int32_t* dropped,
                                int32_t final, void* stream) {
    return capture(in_fmt, x, B, n_br, Tc, frame_len, history, max_pending, offset, trig, trig_ld, trig_stride,
                   n_trig, trig_max, state, frames, frame_start, n_frames, dropped, final, nullptr, stream);
}

int32_t ofs_frame_capture_compact(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                                  int32_t frame_len, int32_t history, int32_t max_pending, int64_t offset,
                                  const int64_t* trig, int64_t trig_ld, int64_t trig_stride,
                                  const int32_t* n_trig, int32_t trig_max, void* state, int64_t cap,
                                  void* frames, int64_t* frame_start, int32_t* frame_stream, int32_t* row0,
                                  int32_t* n_rows, int32_t* n_frames, int32_t* dropped, int32_t final,
                                  void* stream) {
    FcArgsC c{};
    c.cap = cap; c.frame_stream = frame_stream; c.row0 = row0; c.n_rows = n_rows;
    return capture(in_fmt, x, B, n_br, Tc, frame_len, history, max_pending, offset, trig, trig_ld, trig_stride,
                   n_trig, trig_max, state, frames, frame_start, n_frames, dropped, final, &c, stream);
}

}  // extern "C"
