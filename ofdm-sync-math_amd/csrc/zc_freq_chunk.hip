// zc_freq_chunk.hip — resumable form of the frequency-domain ZC metric (ofs_zc_freq_metric on its
// sliding kernels, zc_slide.hip) for streams that arrive in chunks (ofs_zc_freq_metric_chunk): one
// call takes the next Tc samples of B streams and returns zc_freq.compute_frequency_metric
// (zc_freq.py:62-99) at the stream's newest samples, with the running np.argmax of the metric (the
// reference's detection, zc_freq.py:144) carried along.
//
// THE SAME ARITHMETIC, CHUNK FOR CHUNK.  The sliding kernel cuts the offsets into chunks of C and
// starts chunk c from its own exact window, built from the block DFTs of the samples
// cp + cC .. cp + cC + N - 1 (blocks at the absolute positions cp + mC); the recursion then runs at most
// C steps.  So output s reads x[cp + floor(s/C)·C .. cp + s + N - 1] and depends on its place s mod C in
// its chunk, and on nothing else: not on where a launch begins or ends, and not on the waves per
// workgroup or the workgroup count (zs_body.h).  A chunk call with n_seen samples behind it covers the
// offsets [lo, hi) = [max(s_first, 0), s_first + Tc), s_first = n_seen - (N + cp) + 1: it runs the body
// on the chunks floor(lo/C) .. ceil(hi/C) - 1 of the stream of T = n_seen + Tc samples and stores what
// lies in [lo, hi).  A one-shot call on those T samples computes the same chunks from the same samples
// (every block a chunk with an output below hi reads ends at or before sample T - 1), and a one-shot
// call on a longer stream computes them again, with more samples behind them that none of them reads.
// Samples the stream does not have yet are staged as zeros, as the one-shot call stages i >= T: they
// reach the recursion only after its last stored output.
//
// The samples before the chunk that those outputs read come from a ring in the state, kept in the
// input's own format and keyed by the absolute sample index (slot g mod Hr).  The oldest sample a call
// reads is cp + floor(lo/C)·C >= cp + lo - (C - 1) = n_seen - (N + C - 2) (while lo = 0: sample cp, at
// most N - 1 back), so Hr = N + C holds them all.  Several workgroups of one stream read the ring and
// n_seen, so the metric kernel writes neither: a second kernel on the same HIP stream, one workgroup
// per stream, writes the chunk's newest min(Tc, Hr) samples into the ring, folds this call's metric
// row into the carried peak, writes off0 and the peak outputs and advances (final: zeroes) the header.
//
// State of one stream (ofs_zc_freq_chunk_state_bytes = 64 + n_br·Hr·sample_bytes, all-zero = fresh):
// ZfcHdr (64 B), then the ring [n_br][Hr] in the input format.  There are no carried sums.
#include "zs_body.h"

using namespace ofs_chunk;

namespace {

struct ZfcHdr {
    int64_t n_seen;                 // samples of this stream consumed by earlier calls
    int64_t peak_s;                 // offset of the running first argmax of the metric (peak_kind != 0)
    double peak_v;                  // its value, widened
    int32_t peak_kind;              // 0 no output in the peak yet, 1 a number, 2 the first NaN
    int32_t pad0;
    int64_t pad[4];
};
static_assert(sizeof(ZfcHdr) == 64, "state header");

struct ZfcArgs {
    ZsArgs z;                       // template, N, cp, C, W, groups; x = the chunk [B][n_br][Tc], metric [B][Tc]
    uint8_t* state; int64_t state_bytes, Tc;
    int32_t nb, Hr, fin;
    int64_t* off0; int64_t* peak_index; double* peak_value;
};

constexpr int64_t ZFC_MAX_TC = (int64_t)1 << 30;
constexpr int ZFC_UW = 1024;                                // threads of the update kernel
constexpr int ZFC_UL = 8;                                   // metric loads in flight per thread of its peak fold

// ring length: the N + C - 2 samples before a call that its outputs may read, rounded up to N + C
__host__ __device__ constexpr int zfc_ring(int N, int C) { return N + C; }

// ------------------------------------------------------------------------------------------
// metric kernel: workgroup blockIdx.x / B of stream blockIdx.x % B; reads the state.  A call's grid is
// sized for the most chunks any alignment can touch, (Tc - 1) / C + 2, so the last workgroup of a
// stream often has no chunk and exits at once.  Workgroups are numbered group-major so that those
// come last in the grid: numbered stream-major, with two groups per stream every odd workgroup would
// be empty, and the dispatcher, which deals consecutive workgroups round-robin over the 8 XCDs, would
// leave half the XCDs without work (measured so: ONE push of 16384 samples took 2.4 x the one-shot call,
// DESIGN §4.6c).
// ------------------------------------------------------------------------------------------
template <int FMT, int NB, int NR, class OUT, bool PAIR, bool DEFER>
__global__ __launch_bounds__(64 * ZS_MAXW) void zfc_kernel(ZfcArgs q) {
    extern __shared__ __attribute__((aligned(16))) double2 zsm[];
    const ZsArgs& a = q.z;
    const int64_t g = blockIdx.x / a.B, b = blockIdx.x - g * a.B;
    const uint8_t* sp = q.state + b * q.state_bytes;
    const int64_t n_seen = reinterpret_cast<const ZfcHdr*>(sp)->n_seen;
    const int64_t Tc = q.Tc;
    OUT* row = static_cast<OUT*>(a.metric) + b * Tc;

    // element j of the call is offset s = s_first + j; the fill phase (s < 0) is +0.0
    const int64_t s_first = n_seen - ((int64_t)a.N + a.cp) + 1;
    const int64_t nz = s_first >= 0 ? 0 : (-s_first < Tc ? -s_first : Tc);
    for (int64_t j = g * blockDim.x + threadIdx.x; j < nz; j += a.groups * blockDim.x) row[j] = 0;
    const int64_t lo = s_first > 0 ? s_first : 0, hi = s_first + Tc;
    if (hi <= lo) return;                                    // whole workgroup: the call is all fill phase
    const int64_t cend = (hi + a.C - 1) / a.C;
    const int64_t c0 = lo / a.C + g * NR * (int64_t)a.W;
    if (c0 >= cend) return;                                  // whole workgroup: no chunk of this stream
    const int64_t c1 = min(c0 + NR * (int64_t)a.W, cend);

    ZsRing<FMT, NB, OUT> cx;
    cx.x = a.x; cx.ring = sp + sizeof(ZfcHdr);
    cx.n_seen = n_seen; cx.T = n_seen + Tc; cx.lo = lo; cx.hi = hi; cx.Tc = Tc; cx.xrow0 = b * NB; cx.off0 = s_first;
    cx.c0 = c0; cx.c1 = c1;
    cx.Hr = q.Hr; cx.r0 = (int)(n_seen % q.Hr); cx.row = row;
    if constexpr (PAIR) {
        constexpr int PPL = NR / 2;
#include "zs_pair_body.h"
    } else {
        constexpr int BPL = NR;
#include "zs_slide_body.h"
    }
}

// ------------------------------------------------------------------------------------------
// update kernel: one workgroup per stream, after the metric kernel
// ------------------------------------------------------------------------------------------
template <int FMT, class OUT>
__global__ __launch_bounds__(ZFC_UW) void zfc_update_kernel(ZfcArgs q) {
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t Tc = q.Tc;
    uint8_t* sp = q.state + b * q.state_bytes;
    ZfcHdr* hdr = reinterpret_cast<ZfcHdr*>(sp);
    const ZfcHdr h = *hdr;
    const int64_t n_seen = h.n_seen;

    if (!q.fin) ring_write<FMT, ZFC_UW>(sp + sizeof(ZfcHdr), q.z.x, b, q.nb, Tc, n_seen, q.Hr, t);

    const OUT* row = q.z.metric ? static_cast<const OUT*>(q.z.metric) + b * Tc : nullptr;
    const int64_t s_first = n_seen - ((int64_t)q.z.N + q.z.cp) + 1;
    const int64_t nz = s_first >= 0 ? 0 : (-s_first < Tc ? -s_first : Tc);
    ChunkPeak me{0.0, 0, 0};
    if (row) me = row_peak<ZFC_UW, ZFC_UL>(row, nz, Tc, s_first, t);   // this call's outputs (every one is the reference's)
    const ChunkPeak pk = peak_fold<ZFC_UW>(me, ChunkPeak{h.peak_v, h.peak_s, h.peak_kind}, t);
    if (t == 0) {
        if (q.off0) q.off0[b] = s_first;
        if (q.peak_index) q.peak_index[b] = pk.kind ? pk.i : -1;
        if (q.peak_value) q.peak_value[b] = pk.kind ? pk.v : 0.0;
        ZfcHdr o{};                                          // final: fresh again (the ring is not read)
        if (!q.fin) {
            o.n_seen = n_seen + Tc;
            o.peak_s = pk.i; o.peak_v = pk.v; o.peak_kind = pk.kind;
        }
        *hdr = o;
    }
}

template <auto KERN>
int zfc_launch(const ZfcArgs& q, size_t lds, hipStream_t st) {
    // the dynamic-LDS limit, on every launch: no state of the library's, right on every device
    if (hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return OFS_EHIP;
    hipLaunchKernelGGL(KERN, dim3((unsigned)(q.z.B * q.z.groups)), dim3(64 * q.z.W), lds, st, q);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}

template <int FMT, int NB, class OUT>
int zfc_go(const ZfcArgs& q, const ZsForm& f, bool metric, hipStream_t st) {
    if (metric) {
        int r;
        if (f.pair) {
            constexpr int ROWS = NB == 2 ? 4 : 8;            // the one-shot call's PPL = ROWS / 2
            r = f.defer ? zfc_launch<zfc_kernel<FMT, NB, ROWS, OUT, true, true>>(q, f.lds, st)
                        : zfc_launch<zfc_kernel<FMT, NB, ROWS, OUT, true, false>>(q, f.lds, st);
        } else if constexpr (NB == 2) {
            r = f.defer ? zfc_launch<zfc_kernel<FMT, 2, 4, OUT, false, true>>(q, f.lds, st)
                        : zfc_launch<zfc_kernel<FMT, 2, 4, OUT, false, false>>(q, f.lds, st);
        } else if (f.bpl == 4) {
            r = zfc_launch<zfc_kernel<FMT, 1, 4, OUT, false, false>>(q, f.lds, st);
        } else {
            r = f.defer ? zfc_launch<zfc_kernel<FMT, 1, 8, OUT, false, true>>(q, f.lds, st)
                        : zfc_launch<zfc_kernel<FMT, 1, 8, OUT, false, false>>(q, f.lds, st);
        }
        if (r != OFS_OK) return r;
    }
    hipLaunchKernelGGL((zfc_update_kernel<FMT, OUT>), dim3((unsigned)q.z.B), dim3(ZFC_UW), 0, st, q);
    return hipGetLastError() == hipSuccess ? OFS_OK : OFS_EHIP;
}

// the supported (format, precision) pairs and shapes: those of the sliding kernel (ofs_zc_slide_ok)
bool zfc_shape_ok(int in_fmt, int n_br, int N, int cp) {
    if (!zs_shape_ok(in_fmt, n_br, N, 1) || cp < 0) return false;
    int W;
    size_t lds;
    return zs_plan_chunks(n_br, N, zs_bpl(n_br), zs_chunk_len(N), 1, W, lds);
}
int zfc_precision(int in_fmt) { return in_fmt == OFS_C64 ? OFS_FP32 : OFS_FP64; }

}  // namespace

extern "C" {

int64_t ofs_zc_freq_chunk_state_bytes(int32_t in_fmt, int32_t n_br, int32_t N, int32_t cp) {
    if (!zfc_shape_ok(in_fmt, n_br, N, cp)) return OFS_EINVAL;
    return (int64_t)sizeof(ZfcHdr) + (int64_t)n_br * zfc_ring(N, zs_chunk_len(N)) * sample_bytes(in_fmt);
}

int64_t ofs_zc_freq_chunk_max_samples(int32_t in_fmt, int32_t n_br, int32_t N, int32_t cp) {
    if (!zfc_shape_ok(in_fmt, n_br, N, cp)) return OFS_EINVAL;
    return ZFC_MAX_TC;
}

int32_t ofs_zc_freq_metric_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                                 int32_t N, int32_t cp, int32_t precision, int32_t n_bins,
                                 const int32_t* bin_indices, const double* template_bins,
                                 double template_energy, void* state, void* metric, int64_t* off0,
                                 int64_t* peak_index, double* peak_value, int32_t final, void* stream) {
    if (!zfc_shape_ok(in_fmt, n_br, N, cp) || precision != zfc_precision(in_fmt) || n_bins < 1 || n_bins > 64 ||
        !bin_indices || !template_bins || chunk_args_bad(B, Tc, ZFC_MAX_TC, final, state, x) ||
        (!metric && (peak_index || peak_value) && B * Tc > 0))
        return OFS_EINVAL;
    if (B == 0) return OFS_OK;
    ZfcArgs q{};
    ZsArgs& a = q.z;
    a.x = x; a.B = B; a.N = N; a.cp = cp; a.metric = Tc > 0 ? metric : nullptr;
    int kb[64];
    double tr[64], ti[64];
    for (int i = 0; i < n_bins; ++i) {                       // reduced mod N: fftshift(fft)[(N/2+k)%N] = fft[k mod N]
        kb[i] = (int)(((bin_indices[i] % N) + N) % N);
        tr[i] = template_bins[2 * i]; ti[i] = template_bins[2 * i + 1];
    }
    zs_template(a, n_bins, kb, tr, ti, template_energy);
    // the one-shot call's plan (zs_body.h): C, bins per lane, body and row sums do not depend on Tc;
    // W and the workgroup count follow from the chunks a call can touch, (Tc - 1) / C + 2 at the most
    const int bpl = zs_bpl(n_br);
    a.C = zs_chunk_len(N);
    const int64_t nch = Tc > 0 ? (Tc - 1) / a.C + 2 : 1;
    size_t lds;
    if (!zs_plan_chunks(n_br, N, bpl, a.C, nch, a.W, lds)) return OFS_EINVAL;
    a.nchunks = nch;
    a.groups = (nch + (int64_t)bpl * a.W - 1) / ((int64_t)bpl * a.W);
    if (B > 0x7fffffffll || B * a.groups > 0x7fffffffll) return OFS_EINVAL;
    const ZsForm form = zs_form(a, n_br, lds);
    q.state = reinterpret_cast<uint8_t*>(state);
    q.state_bytes = ofs_zc_freq_chunk_state_bytes(in_fmt, n_br, N, cp);
    q.Tc = Tc; q.nb = n_br; q.Hr = zfc_ring(N, a.C); q.fin = final != 0;
    q.off0 = off0; q.peak_index = peak_index; q.peak_value = peak_value;
    hipStream_t st = (hipStream_t)stream;
    const bool run = a.metric != nullptr;
#define ZFC_CASE(F, NBV, O) if (in_fmt == F && n_br == NBV) return zfc_go<F, NBV, O>(q, form, run, st);
    ZFC_CASE(OFS_C64, 1, float) ZFC_CASE(OFS_C64, 2, float) ZFC_CASE(OFS_C128, 1, double)
    ZFC_CASE(OFS_C128, 2, double) ZFC_CASE(OFS_CI16, 1, double) ZFC_CASE(OFS_CI16, 2, double)
#undef ZFC_CASE
    return OFS_EINVAL;
}

}  // extern "C"
