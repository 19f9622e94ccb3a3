// zc_slide.hip — zc_freq.compute_frequency_metric (zc_freq.py:62-99) at EVERY offset of long
// streams: the 62 template bins of each window's N-point DFT by a sliding DFT in fp64.
//
// For window start s' = cp + s (offset s) and template bin k (w = exp(-2 pi i / N)):
//     X_s[k] = Σ_{n<N} x[s' + n] w^{kn}           (= fft(window)[k mod N], zc_freq.py:92-94)
//     X_{s+1}[k] = w^{-k} (X_s[k] + x[s' + N] - x[s'])                    (the sliding recursion)
//     metric(s) = |Σ_br Σ_k conj(t_k) X_s,br[k]|² / max(E_t Σ_br Σ_k |X_s,br[k]|², 1e-12)
//
// Work split (one workgroup = W waves = BPL·W consecutive chunks of C offsets of one stream):
//   phase 1  block DFTs  β_k(m) = Σ_{j<C} x[cp + mC + j] w^{kj}  of the workgroup's BPL·W + N/C - 1
//            blocks, one block per wave at a time (lane = bin, Horner in w^{4k} over four
//            interleaved chains, samples broadcast from LDS), kept in LDS;
//   phase 2  each wave slides BPL chunks at once (BPL = bins per lane, 8 by default): a row of
//            LPC = 64/BPL lanes owns one chunk, lane (r, j) owns bins j, j+LPC, ... (64 slots; slots
//            >= n_bins have w^{-k} = 0 and stay 0).  A chunk's initial window is
//            Σ_{q<N/C} w^{kqC} β_k(c + q) (no per-chunk N-sample sum), then C steps of the
//            recursion; per step the numerator / energy terms are summed in-lane over the lane's
//            BPL bins and across the row's LPC lanes by DPP (quad_perm, then row_half_mirror for
//            8 lanes or row_ror 4/8 for 16: every lane gets the row total), and lane (r, u mod LPC)
//            keeps step u's result for coalesced stores once per 16 steps.  More bins per lane =
//            fewer cross-lane steps per offset (BPL 4 -> 8: 21 -> ~15 VALU per offset).
//            DEFER (default): no per-step DPP at all - each lane parks its in-lane partials of
//            ZS_RG = 4 steps in LDS (the block-DFT region, dead once the initial windows are
//            built), then lane (r, j < 4) sums the row's partials of step j.  fp64 has no DPP
//            arithmetic (each DPP stage is 2 v_mov_dpp + 1 add), so the row sums were 27 of the
//            136 VALU per step, plus the keep selects; deferred, they cost ~6.
// Every chunk starts from its own exact window (block sums), so the recursion runs at most C
// steps (error ~C·2^-53 relative).  fp64 state throughout; OUT = float rounds only the metric.
//
// What a workgroup does lives in zs_body.h and the statement lists zs_slide_body.h / zs_pair_body.h,
// shared with the resumable chunk-fed call (zc_freq_chunk.hip); the kernels here include them with the
// whole-stream context (ZsWhole) and store every offset.
#include "zs_body.h"

namespace {

template <int FMT, int NB, int BPL, class OUT, bool DEFER>
__global__ __launch_bounds__(64 * ZS_MAXW) void zc_slide_kernel(ZsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 zsm[];
    ZsWhole<FMT, NB, OUT> cx{0};
#include "zs_slide_body.h"
}

template <int FMT, int NB, int PPL, class OUT, bool DEFER>
__global__ __launch_bounds__(64 * ZS_MAXW) void zc_pair_kernel(ZsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 zsm[];
    ZsWhole<FMT, NB, OUT> cx{0};
#include "zs_pair_body.h"
}

template <class K>
int zs_launch(K kern, bool& attr, const ZsArgs& a, size_t lds, hipStream_t st) {
    if (!attr) {                                      // the dynamic-LDS limit, once per instantiation
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return OFS_EHIP;
        attr = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.B * a.groups)), dim3(64 * a.W), lds, st, a);
    return hipGetLastError() == hipSuccess ? 1 : OFS_EHIP;
}

template <int FMT, int NB, class OUT>
int zs_go(const ZsArgs& a, const ZsForm& f, hipStream_t st) {
    const bool df = f.defer;
    static bool at[6] = {false, false, false, false, false, false};
    if (f.pair) {
        constexpr int PPL = NB == 2 ? 2 : 4;          // rows of 32/PPL lanes: 4 chunks (two branches) / 8 per wave
        return df ? zs_launch(zc_pair_kernel<FMT, NB, PPL, OUT, true>, at[0], a, f.lds, st)
                  : zs_launch(zc_pair_kernel<FMT, NB, PPL, OUT, false>, at[1], a, f.lds, st);
    }
    if constexpr (NB == 2) {
        return df ? zs_launch(zc_slide_kernel<FMT, 2, 4, OUT, true>, at[2], a, f.lds, st)
                  : zs_launch(zc_slide_kernel<FMT, 2, 4, OUT, false>, at[3], a, f.lds, st);
    } else {
        if (f.bpl == 4)                               // 4 one-branch bins per lane: never deferred (zs_form)
            return zs_launch(zc_slide_kernel<FMT, 1, 4, OUT, false>, at[4], a, f.lds, st);
        return df ? zs_launch(zc_slide_kernel<FMT, 1, 8, OUT, true>, at[2], a, f.lds, st)
                  : zs_launch(zc_slide_kernel<FMT, 1, 8, OUT, false>, at[3], a, f.lds, st);
    }
}

// C, W and the per-bin body's LDS of a one-shot call of noff offsets; false if the blocks do not fit
bool zs_plan(int n_br, int N, int bpl, int& C, int& W, size_t& lds, int64_t noff) {
    C = zs_chunk_len(N);
    return zs_plan_chunks(n_br, N, bpl, C, (noff + C - 1) / C, W, lds);
}
}  // namespace

// Shapes the sliding kernel takes: N a multiple of 64, 1 or 2 branches, <= 64 template bins, the
// blocks of a window in LDS.
extern "C" int ofs_zc_slide_ok(int fmt, int n_br, int N, int nbins, int64_t noff) {
    if (!(zs_shape_ok(fmt, n_br, N, nbins) && noff > 0)) return 0;
    int C, W;
    size_t lds;
    return zs_plan(n_br, N, zs_bpl(n_br), C, W, lds, noff) ? 1 : 0;
}

// Launch (1), unsupported shape (0) or OFS_E*.  kb: template bins already reduced mod N (host).
extern "C" int ofs_zc_slide_launch(int fmt, int n_br, int out_f32, const void* x, int64_t B, int64_t T, int N, int cp,
                                   int nbins, const int* kb, const double* tr, const double* ti, double t_energy,
                                   void* metric, hipStream_t st) {
    const int64_t noff = T - ((int64_t)N + cp) + 1;
    if (noff <= 0) return OFS_ESHORT;
    if (!ofs_zc_slide_ok(fmt, n_br, N, nbins, noff)) return 0;
    ZsArgs a;
    a.x = x; a.B = B; a.T = T; a.N = N; a.cp = cp; a.noff = noff; a.metric = metric;
    zs_template(a, nbins, kb, tr, ti, t_energy);
    size_t lds;
    const int bpl = zs_bpl(n_br);
    if (!zs_plan(n_br, N, bpl, a.C, a.W, lds, noff)) return 0;
    a.nchunks = (noff + a.C - 1) / a.C;
    a.groups = (a.nchunks + (int64_t)bpl * a.W - 1) / ((int64_t)bpl * a.W);
    if (a.B * a.groups > 0x7fffffff) return 0;
    const bool f = out_f32 != 0;
    const ZsForm form = zs_form(a, n_br, lds);
#define ZS_CASE(F, NBV) \
    if (fmt == F && n_br == NBV) \
        return f ? zs_go<F, NBV, float>(a, form, st) : zs_go<F, NBV, double>(a, form, st);
    ZS_CASE(OFS_C64, 1) ZS_CASE(OFS_C64, 2) ZS_CASE(OFS_C128, 1) ZS_CASE(OFS_C128, 2)
    ZS_CASE(OFS_CI16, 1) ZS_CASE(OFS_CI16, 2)
#undef ZS_CASE
    return 0;
}
