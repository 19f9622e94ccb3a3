/*
 * ofdmsync.h — C ABI of the MI355X-native OFDM preamble-sync engine (libofdmsync.so).
 *
 * Drop-in boundary for the timing-metric + CFO hot path of amcolex/ofdm-sync-math.
 * The reference has no FFI: its "interface" is a set of plain Python functions
 * (SURVEY.md §8b).  Each entry point below replaces the arithmetic of one of them; the
 * Python mirror in ofdm-sync-math_amd/ (same module/function names) binds these
 * symbols with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch CUDA tensor storage),
 *     except where noted; buffers are caller-allocated, nothing is allocated inside;
 *   - a pointer may be NULL when the buffer it describes is empty (B = 0 or T = 0);
 *   - input samples are laid out [B][n_branch][T] (stream-major, branch, time), the
 *     branch axis is SUMMED exactly like axis 0 of the reference's 2-D inputs;
 *   - outputs are laid out [B][n_out];
 *   - work is enqueued on `stream` (a hipStream_t; NULL = default stream) and is
 *     stream-ordered: no host synchronisation happens inside any call;
 *   - return value: 0 on success, negative OFS_E* on error (no partial launch on
 *     argument errors); the library keeps no global mutable state (re-entrant).
 */
#ifndef OFDMSYNC_H
#define OFDMSYNC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* input sample formats */
#define OFS_C64   0   /* interleaved float32 (re, im)                                  */
#define OFS_C128  1   /* interleaved float64 (re, im)                                  */
#define OFS_CI16  2   /* interleaved int16 (I, Q), e.g. 12-bit ADC words sign-extended  */
/* packed 12-bit AXIS words, the RTL detector's wire format (ref/test_minn_preamble_detector.py:41-47,
 * ref/minn_preamble_detector.sv:152-155): per time index one word of n_ant 24-bit channel groups,
 * channel c at bit 24*c with I in its bits 0-11 and Q in 12-23 (two's complement), words packed
 * back to back little-endian (3 * n_ant bytes per time index); layout [B][T][3 * n_ant] bytes.
 * Accepted by ofs_aa_detect (OFS_FP64, 1-2 antennas) and ofs_minn_rtl (1-2 branches) on their
 * integer-exact plans; other entry points / shapes return OFS_EINVAL. */
#define OFS_CP12  3

/* arithmetic precision of a call */
#define OFS_FP32  0   /* fp32 products / in-row scans, fp64 row bases; f32/c64 outputs  */
#define OFS_FP64  1   /* fp64 throughout; f64/c128 outputs (bit-exact on integer input) */

/* status codes */
#define OFS_OK            0
#define OFS_EINVAL       -1   /* bad argument (null required pointer, bad size, bad enum)  */
#define OFS_ETOOLONG     -2   /* window/halo does not fit one workgroup's LDS tile          */
#define OFS_EHIP         -3   /* kernel launch failed (hipGetLastError)                     */
#define OFS_ESHORT       -4   /* stream shorter than one symbol (zc_freq.py:76-78 raises)   */
#define OFS_EFFT         -5   /* rocFFT plan creation / execution failed                    */

/* ofs_zc_correlate modes */
#define OFS_ZC_RAW        0   /* per-branch np.convolve(x, conj(ref[::-1]))                 */
#define OFS_ZC_V2         1   /* zc_v2 detect_zc_preamble: sum of per-branch normalised corr */
#define OFS_ZC_COMBINED   2   /* zc.py: sum_br corr / (|ref| sqrt(max(sum_br E, 0) + 1e-12)) */
#define OFS_ZC_NORMALIZE  3   /* zc_v2.normalize_correlation(corr_in, x, ref), one branch    */
#define OFS_ZC_SUM        4   /* sum_br raw corr (detect_zc_preamble, normalize=False)       */

int32_t ofs_version(void);
/* sha256 (16 hex digits) of the csrc sources (.hip, .h) and include/ofdmsync.h this library was
 * built from ("unknown" for a build without it). */
const char* ofs_source_hash(void);
const char* ofs_status_string(int32_t status);

/*
 * Debug / A-B variants (not part of the reference interface; no reference counterpart).
 * Every dispatch decision and every arithmetic choice of the library depends only on the call's
 * arguments, EXCEPT where a variant has been set through this one entry point.  Variants exist
 * so the tests can force an alternative kernel on the same input (e.g. the general LDS engine
 * against the integer-exact wave kernel, the rocFFT matched-filter pipeline against the fused LDS
 * FFT) and the measurement tools can time both.  Nothing reads the environment.  All variants
 * start unset (OFS_VARIANT_UNSET); a process that never calls ofs_debug_set_variant runs the
 * default dispatch.  Names (value meaning):
 *   EXACT        0: sync_aa / minn_rtl integer-exact and fp64 wave kernels off (general engine)
 *   FAST_E       2|4|8: samples per lane of the storing aa_fast kernel
 *   FAST_E_DO    2|4|8: samples per lane of the detect-only aa_fast kernel
 *   FAST_SCAN    32|64: row-scan precision of the storing aa_fast kernel (default 64)
 *   FAST_SCAN_DO 32|64: row-scan precision of the detect-only aa_fast kernel (default 32)
 *   RTL_WPB      1|2: streams per workgroup of rtl_exact_kernel (default 4)
 *   PARK_DIRECT  1: Park energies as direct window sums (no shared-window split)
 *   ZW64         0: zc_freq N = 4096 window FFT through zc_win_kernel instead of zc_win64_kernel
 *   ZW64_GRID    n > 0: cap of the persistent zc_win64 grid (default: CU count)
 *   ZS           0: zc_freq fp64 through the round-2 one-chunk-per-wave kernel
 *   ZF_ITEMS     n > 0: chunk-count target of that kernel (default 4096)
 *   ZS_PAIR      0: per-bin sliding DFT instead of the pair resonators
 *   ZS_DEFER     0|1: row sums per step (DPP) / deferred through LDS
 *   ZS_BPL       4: bins per lane of the one-branch sliding kernel (default 8)
 *   ZS_C         64|128|192|256: chunk length of the sliding kernels (must divide N)
 *   ZS_GBLK      0: Horner block DFTs in the pair kernel instead of Goertzel
 *   MC_FUSED     0: ZC matched filter through the rocFFT pipeline instead of the fused LDS FFT
 *   MC_FUSE_X    0: fused LDS FFT with the separate extract kernel
 *   MC_PERS      0: fused LDS FFT one block per 1024-thread workgroup instead of the persistent
 *                512-thread kernel that prefetches the next block
 *   ZC_SEQ       1: zc_v2 CFAR + gate through the sequential one-wave-per-stream kernel
 *   ZC_NODMA     1: zc_v2 CFAR tiles through registers instead of LDS-DMA
 *   BE_FAST      0: receiver back-end through the generic kernel
 *   FAST_LDS     n > 0: bytes of unused dynamic LDS per workgroup of the aa_fast kernel (occupancy
 *                cap; default 16384 for the one-antenna storing kernel = 10 per CU, 23000 = 7 per CU for
 *                its full-stream form, 1 = no cap)
 *   OCC_LDS      n >= 0: bytes of unused dynamic LDS added to the other wave-per-stream launches
 *                (aa_stream, win_fast, aa_exact, rtl_exact, the fast back-end; occupancy A/B)
 *   FAST_RMPAIR  0|1: R and M of two adjacent rows of the one-antenna E = 2 storing aa_fast kernel as
 *                one 16-byte store per lane (one contiguous 1 KiB span per wave instruction; default 1)
 *   FAST_ST_POLICY 0|1: that kernel's P/R/M stores plain / non-temporal (default 1)
 *   FAST_LD_POLICY 0: input loads of that kernel's full-stream form plain instead of non-temporal (same
 *                bits; default 1, any other value is the default; A/B and the tests' reference arm)
 *   FAST_HEAD    0: ofs_aa_detect_ex ignores OFS_AA_HEAD_RESIDENT (the P/M head is rewritten; A/B of
 *                both arms on the same buffers)
 *   FAST_FULL    0: the headline shape (one antenna, T = 1024, L = 128 | 256 | 512, P, R, M and events,
 *                no valid) through the generic aa_fast kernel instead of its full-stream form (same
 *                bits; A/B and the tests' reference arm)
 * ofs_debug_set_variant returns OFS_EINVAL for an unknown name; value OFS_VARIANT_UNSET clears
 * one variant, ofs_debug_reset_variants clears all.  The table is per calling thread
 * (thread_local): a variant set by one thread steers only the calls that same thread makes, and
 * every new thread starts with all variants unset.  A call reads each variant once, at dispatch.
 */
#define OFS_VARIANT_UNSET INT64_MIN
int32_t ofs_debug_set_variant(const char* name, int64_t value);
int64_t ofs_debug_get_variant(const char* name);
int32_t ofs_debug_reset_variants(void);

/*
 * [A][A] streaming Schmidl-Cox detector.
 * Replaces sync_aa.aa_detect_streaming (sync_aa.py:421-571): P[n], R[n], M[n], valid[n]
 * (sync_aa.py:458-493) and, if detect != 0, the gate/peak/CFO events (sync_aa.py:495-568).
 *   P: [B][T] c64|c128, R, M: [B][T] f32|f64 (per precision); valid: [B][T] uint8; each nullable
 *   (detect on a stream longer than one LDS tile needs P and M).
 *   n_events: [B] int32 (total events per stream, may exceed max_events);
 *   ev_int:  [B][max_events][4] int64 = peak_index, gate_start, gate_end, frame_start;
 *   ev_real: [B][max_events][4] f64   = P_re, P_im, M_at_peak, cfo_hz.
 */
int32_t ofs_aa_detect(int32_t in_fmt, const void* x, int64_t B, int32_t n_ant, int64_t T,
                      int32_t L, int32_t precision, void* P, void* R, void* M, uint8_t* valid,
                      int32_t detect, double threshold, int32_t hysteresis, double sample_rate,
                      int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_real,
                      void* stream);

/*
 * ofs_aa_detect with flags; ofs_aa_detect is the flags = 0 call.  Unknown flag bits: OFS_EINVAL.
 *
 * OFS_AA_HEAD_RESIDENT: the caller guarantees that P[b][n] and M[b][n] already hold +0.0 (all-zero
 * bits) for every b and every n < min(L, T).  Those elements are constant by the algorithm's
 * definition - the delay line is not yet valid there, so P[n] = M[n] = +0.0 for any input, NaN and
 * Inf included - and a caller that reuses its output buffers from call to call still holds them.
 * The library may then leave them unwritten (it may also still write zeros there); every n >= L is
 * written exactly as without the flag, and R, valid, the events and n_events are unaffected.  A
 * permission, not an obligation: the fp32 fast paths (ofs_aa_plan 1000-1199) use it, every other
 * plan (general engine, integer-exact / fp64 wave kernels) and detect-only calls ignore it.
 */
#define OFS_AA_HEAD_RESIDENT 1u
int32_t ofs_aa_detect_ex(int32_t in_fmt, const void* x, int64_t B, int32_t n_ant, int64_t T,
                         int32_t L, int32_t precision, void* P, void* R, void* M, uint8_t* valid,
                         int32_t detect, double threshold, int32_t hysteresis, double sample_rate,
                         int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_real,
                         void* stream, uint32_t flags);

/*
 * Which kernel ofs_aa_detect dispatches a shape to (pure query, no launch):
 *   1000 + 10*E + MR : register-resident wave-per-stream fast path (E samples per lane,
 *                      L = 64*E*MR), complex64 / OFS_FP32 / 1-2 antennas / even T <= 1024;
 *   1100 + 10*E + MR : streaming wave-per-stream fast path, same arithmetic, any other T
 *                      (rows streamed from HBM, lag / window rings in registers), MR <= 8;
 *   2000 + 10*E + MR : integer-exact wave-per-stream path, OFS_CI16 / OFS_FP64, 1-2 antennas,
 *                      T * n_ant <= 2^21 (all window sums exact integers), L = 64*E*MR, MR <= 8;
 *   3000 + 10*E + MR : the same wave-per-stream kernel on OFS_C128 / OFS_FP64 input (fp64 prefix
 *                      differences over the stream, any T: the reference's running-sum error regime);
 *   1                : general LDS engine, events fused (stream fits one tile);
 *   2                : general LDS engine, tiled, events in a second pass over P/M;
 *   <0               : invalid arguments or window too long (as ofs_aa_detect would return).
 */
int32_t ofs_aa_plan(int32_t in_fmt, int32_t precision, int32_t n_ant, int64_t T, int32_t L);

/*
 * Resumable chunked [A][A] detection for integer streams of any length (no reference counterpart:
 * the reference's sample-by-sample loop, sync_aa.py:421-571, is the specification).
 *
 * A stream is fed in consecutive chunks of Tc samples; ofs_aa_detect_chunk returns the chunk's
 * P/R/M/valid and the gate events that CLOSED among its samples, and keeps what the next call needs
 * in a caller-owned state buffer on the device.  The library allocates nothing and keeps no global
 * state.
 *   in_fmt  OFS_CI16: x = [B][n_ant][Tc] int16 (I, Q);  OFS_CP12: x = [B][Tc][3 * n_ant] bytes.
 *           Arithmetic is fp64 (as OFS_FP64 in ofs_aa_detect).  n_ant 1-2; L 64, 128, 256, 512 or 1024.
 *   state   [B][ofs_aa_chunk_state_bytes(n_ant, L)] bytes, 16-byte aligned, device memory.  The layout
 *           is opaque; ALL-ZERO BYTES ARE A FRESH STREAM, so any subset of streams is reset with a
 *           memset of its rows (stream-ordered with the calls).  One state row belongs to one stream:
 *           in_fmt, n_ant, L, threshold, hysteresis and detect must not change between the calls of
 *           a stream (sample_rate and max_events may), and the calls of a stream must be ordered
 *           (same HIP stream, or synchronised by the caller).
 *   P, R, M, valid  [B][Tc] c128 / f64 / f64 / uint8, each nullable; index i of a call is the stream's
 *           absolute sample n = (samples of earlier calls) + i; valid = n >= L.
 *   events  as ofs_aa_detect, written from slot 0 of every call, with ABSOLUTE int64 indices
 *           (peak_index, gate_start, gate_end, frame_start = peak_index - 2L + 1).  n_events[b] is the
 *           number of gates that closed during this call (exact even above max_events).  A gate still
 *           open at the end of the chunk is carried, not closed, unless final != 0: then it closes
 *           at gate_end = the stream's sample count, as ofs_aa_detect closes it at T, and the state
 *           is a fresh stream again after the call.
 *   Tc      1 .. ofs_aa_chunk_max_samples(n_ant, L) = 2^21 / n_ant - 2L ((Tc + 2L) * n_ant <= 2^21
 *           keeps every window sum an exact integer below 2^53); Tc = 0 with final != 0 is a flush:
 *           no samples, open gates close and emit (x, P, R, M, valid unused).
 * EQUIVALENCE GUARANTEE.  For any split of a stream into chunks within the per-call limit, the
 * concatenated P, R, M, valid and the sequence of events (the last call final) equal bit for bit
 * what ONE ofs_aa_detect call on the whole stream returns on its integer-exact plan
 * (ofs_aa_plan 2000-2999); for streams longer than that plan reaches they equal the reference's
 * float64 loop on P, R, valid and the events' integers, with M and the events' reals as close as
 * ofs_aa_detect's (the window sums are the same exact integers).
 * Calls are stream-ordered and never synchronise with the host: consecutive chunks may be enqueued
 * back to back.  OFS_EINVAL (before any launch): another in_fmt, n_ant outside 1-2, an L outside the
 * table, Tc < 0 or above the limit, Tc = 0 without final, B < 0, a null or misaligned state with
 * B > 0, a null x with B * Tc > 0, hysteresis > OFS_AA_CHUNK_MAX_HYSTERESIS, detect with a null
 * n_events or with null event arrays while max_events > 0.  There is no fall-back to the general
 * engine.  ofs_aa_chunk_state_bytes returns the bytes of ONE stream's state (a multiple of 16) and
 * ofs_aa_chunk_max_samples the largest Tc of one call; both return OFS_EINVAL (< 0) for an unsupported
 * n_ant or L.
 */
#define OFS_AA_CHUNK_MAX_HYSTERESIS (1 << 28)
int64_t ofs_aa_chunk_state_bytes(int32_t n_ant, int32_t L);
int64_t ofs_aa_chunk_max_samples(int32_t n_ant, int32_t L);
int32_t ofs_aa_detect_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_ant, int64_t Tc, int32_t L,
                            void* state, void* P, void* R, void* M, uint8_t* valid,
                            int32_t detect, double threshold, int32_t hysteresis, double sample_rate,
                            int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_real,
                            int32_t final, void* stream);

/*
 * Resumable chunked [A][A] detection for complex64 streams: the chunk-fed form of the fp32 fast path
 * (ofs_aa_detect(OFS_C64, ..., OFS_FP32), ofs_aa_plan 1000-1199).  Same contract as ofs_aa_detect_chunk:
 * caller-owned state [B][ofs_aa_chunk_f32_state_bytes(n_ant, L)], 16-byte aligned, ALL-ZERO BYTES ARE A
 * FRESH STREAM; events from slot 0 of every call with absolute int64 indices (frame_start =
 * peak_index - 2L + 1); n_events exact even above max_events; an open gate is carried until final != 0,
 * which closes it at the stream's sample count and leaves a fresh state; Tc = 0 with final is a flush;
 * calls are stream-ordered, never synchronise with the host, allocate nothing and keep no global state.
 *   x       [B][n_ant][Tc] complex64 (this call's chunk); n_ant 1-2; L 128, 256, 512 or 1024.
 *   P, R, M, valid  [B][Tc] c64 / f32 / f32 / uint8, each nullable.
 *   Tc      1 .. ofs_aa_chunk_f32_max_samples(n_ant, L) = 2^30 (in-call positions - 2L + 127 history
 *           samples, the chunk and a gate offset of at most OFS_AA_CHUNK_MAX_HYSTERESIS + 128 - stay
 *           below 2^31).
 *   n_ant, L, threshold, hysteresis and detect must not change between the calls of a stream.
 * EQUIVALENCE GUARANTEE.  For any split of a stream of T samples into chunks, the concatenated P, R, M,
 * valid and the sequence of events (the last call final) - integers and reals - equal BIT FOR BIT what
 * one ofs_aa_detect(OFS_C64, ..., OFS_FP32) call WITH P, R AND M PRESENT returns on the whole stream on
 * plans 1000-1199.  The arithmetic is that of this storing call (rows of 128 samples, 2 per lane, fp64
 * row scans), whether or not P/R/M are passed here.  The one-shot DETECT-ONLY call (no P/R/M/valid)
 * uses another row width and fp32 scans and is NOT the yardstick: its events may differ from these
 * where the decision is a near-tie, exactly as they may from the one-shot storing call's.
 * For n < L the outputs are P = M = +0.0 and valid = 0 for any input, NaN and Inf included: those rows
 * take the no-lag form by their absolute index, nothing is multiplied with a zero history.  Behind
 * non-finite samples an output word is a NaN exactly where the one-shot call's is, with the same
 * payload; its SIGN bit is outside the guarantee, because the one-shot kernels of plans 10xx and 11xx
 * do not agree on it among themselves (two NaNs of opposite sign in one add).
 * STREAM LENGTH.  The state carries the fp64 running sums C of the row totals since sample 0 (of the
 * lagged products and of the energy), and a window's "rows between" term is a difference of two of
 * them, so its absolute error grows as 2^-53 * |C|.  At unit amplitude |C| is about the sample count n,
 * and a window sum is about L with an fp32 ulp of 2^-23 * L: the carried error reaches one such ulp at
 * n = 2^30 * L samples (2^37 for L = 128, 2^40 for L = 1024: hours at 100 MS/s).  Up to there the
 * guarantee above is what bounds the error (it is the one-shot call's); beyond it the outputs still
 * equal what a one-shot call of that length would compute, but that value itself degrades.  final (or
 * zeroing the state) restarts C.  Energy far above unit amplitude shortens the span in proportion.
 * OFS_EINVAL (before any launch): n_ant outside 1-2, an L outside the table, Tc < 0 or above the limit,
 * Tc = 0 without final, B < 0, a null or misaligned state with B > 0, a null x with B * Tc > 0,
 * hysteresis > OFS_AA_CHUNK_MAX_HYSTERESIS, detect with a null n_events or with null event arrays while
 * max_events > 0.  There is no fall-back to the general engine.  The two helpers return OFS_EINVAL (< 0)
 * for an unsupported n_ant or L; the state size is a multiple of 16.
 */
int64_t ofs_aa_chunk_f32_state_bytes(int32_t n_ant, int32_t L);
int64_t ofs_aa_chunk_f32_max_samples(int32_t n_ant, int32_t L);
int32_t ofs_aa_detect_chunk_f32(const void* x, int64_t B, int32_t n_ant, int64_t Tc, int32_t L,
                                void* state, void* P, void* R, void* M, uint8_t* valid,
                                int32_t detect, double threshold, int32_t hysteresis, double sample_rate,
                                int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_real,
                                int32_t final, void* stream);

/*
 * Schmidl-Cox half-symbol metric, reference index convention d = 0 .. T-N.
 * r_mode 0 replaces sc.sc_streaming_metric (sc.py:42-78; R = second-half energy);
 * r_mode 1 replaces combined_sc_min.schmidl_cox_streaming_metric (combined_sc_min.py:116-164;
 * R = energy of both halves).  symbol_len = N (even).  M, P, R: [B][T-N+1], each nullable.
 */
int32_t ofs_sc_metric(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                      int32_t symbol_len, int32_t r_mode, int32_t precision,
                      void* M, void* P, void* R, void* stream);

/*
 * Minn [A A -A -A] metric: replaces minn.minn_streaming_metric (minn.py:59-112),
 * minn.minn_streaming_metric_parameterized (minn.py:697-751) and
 * combined_sc_min.minn_streaming_metric (combined_sc_min.py:60-113).  Q = symbol_len/4.
 * M, P, R: [B][T-N+1], each nullable.
 */
int32_t ofs_minn_metric(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                        int32_t symbol_len, int32_t precision, void* M, void* P, void* R,
                        void* stream);

/*
 * RTL-style adjacent-quarter Minn metric: replaces minn_rtl.minn_rtl_streaming_metric
 * (minn_rtl.py:667-733) and, if detect != 0, minn_rtl.detect_minn_rtl (minn_rtl.py:750-825).
 * Always fp64 (integer-valued inputs give the reference's exact integers).
 *   smooth_mode 0: float IIR of minn_rtl.py:706-715; 1: integer floor-shift IIR of
 *   ref/minn_preamble_detector.sv:288-296 (for integer inputs).
 *   corr_total, energy_total: [B][T] f64 (required); the other arrays nullable;
 *   n_events [B] int32; events [B][max_events][4] int64 = peak, detected, seg_start, seg_end;
 *   open_gate_start [B] int64 = start of a gate still open at the end of the stream, or -1.
 */
int32_t ofs_minn_rtl(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                     int32_t Q, int32_t smooth_shift, int32_t smooth_mode,
                     int64_t threshold_value, int32_t threshold_frac_bits,
                     double* corr_total, double* corr_positive, double* smooth_metric,
                     double* energy_total, double* corr_scaled, double* energy_scaled,
                     uint8_t* metric_valid, uint8_t* above_threshold,
                     int32_t detect, int32_t hysteresis, int32_t timing_offset,
                     int32_t max_events, int32_t* n_events, int64_t* events,
                     int64_t* open_gate_start, void* stream);

/*
 * Which kernel ofs_minn_rtl dispatches a shape to (pure query): 2000 + 10*E + MW for the
 * integer-exact wave-per-stream kernel (OFS_CI16, 1-4 branches, T * n_br <= 2^21, Q = 64*E*MW
 * <= 512: metric, smoothing, threshold and gate FSM in one pass), 0 for the general engine
 * (window kernel + lane-per-stream IIR/gate kernel).
 */
int32_t ofs_rtl_plan(int32_t in_fmt, int32_t n_br, int64_t T, int32_t Q);

/*
 * Resumable chunked minn_rtl detection for integer streams of any length (no reference counterpart:
 * the reference's sample-by-sample models, minn_rtl.py:583-825, are the specification).
 *
 * A stream is fed in consecutive chunks of Tc samples; ofs_minn_rtl_chunk returns the chunk's eight
 * metric arrays and the gate events that CLOSED among its samples, and keeps what the next call needs
 * (the last 3Q samples, the IIR state, the gate machine) in a caller-owned state buffer on the device.
 * The library allocates nothing and keeps no global state.
 *   in_fmt  OFS_CI16: x = [B][n_br][Tc] int16 (I, Q);  OFS_CP12: x = [B][Tc][3 * n_br] bytes.
 *           n_br 1-2; Q 64, 128, 256 or 512 (the table of the integer-exact one-shot kernel).
 *   state   [B][ofs_rtl_chunk_state_bytes(n_br, Q)] bytes, 16-byte aligned, device memory.  The layout
 *           is opaque; ALL-ZERO BYTES ARE A FRESH STREAM, so any subset of streams is reset with a
 *           memset of its rows (stream-ordered with the calls).  One state row belongs to one stream:
 *           in_fmt, n_br, Q, smooth_shift, smooth_mode, threshold_value, threshold_frac_bits,
 *           hysteresis, timing_offset and detect must not change between the calls of a stream
 *           (max_events and which arrays are requested may), and the calls of a stream must be ordered
 *           (same HIP stream, or synchronised by the caller).
 *   corr_total .. above_threshold  [B][Tc], f64 / uint8 as in ofs_minn_rtl, EACH nullable; index i of a
 *           call is the stream's absolute sample n = (samples of earlier calls) + i.  The fill phase
 *           (taps valid from n = Q-1, 2Q-1, 3Q-1; metric_valid = n >= 3Q-1) is decided on n, so a chunk
 *           edge may fall anywhere.  smooth_metric at a sample that is not valid yet is the held state.
 *   events  [B][max_events][4] int64 = peak, peak + timing_offset, seg_start, seg_end, ABSOLUTE indices,
 *           written from slot 0 of every call while n_events < max_events; n_events[b] is the number of
 *           gates that closed during this call (exact even above max_events).  The peak is the LAST
 *           maximum of corr_positive in the gate (>=), across calls too.  A gate still open at the end
 *           of the chunk is carried, over any number of calls.  As in ofs_minn_rtl it is never closed
 *           at the end of the stream: every call writes open_gate_start[b], the absolute start of the
 *           gate open after the chunk, or -1.
 *   final   != 0 changes nothing in the outputs; the state is a fresh stream again after the call.
 *   Tc      1 .. ofs_rtl_chunk_max_samples(n_br, Q) = 2^21 / n_br - 3Q ((Tc + 3Q) * n_br <= 2^21 keeps
 *           every prefix an exact integer below 2^53); Tc = 0 with final != 0 is a flush: no samples,
 *           n_events = 0, open_gate_start as carried, the streams fresh afterwards (x and the arrays
 *           unused).
 * EQUIVALENCE GUARANTEE.  For any split of a stream into chunks within the per-call limit, the
 * concatenated arrays and the concatenated events equal bit for bit what ONE ofs_minn_rtl call on the
 * whole stream returns, on every input that call handles exactly (its integer-exact plan,
 * ofs_rtl_plan 2000-2999), and the last call's open_gate_start equals the one-shot call's.  Streams
 * may be longer than that plan reaches; there the results equal the reference's float64 models.
 * Calls are stream-ordered and never synchronise with the host: consecutive chunks may be enqueued
 * back to back.  OFS_EINVAL (before any launch): another in_fmt, n_br outside 1-2, a Q outside the
 * table, Tc < 0 or above the limit, Tc = 0 without final, B < 0, a null or misaligned state with
 * B > 0, a null x with B * Tc > 0, smooth_shift or threshold_frac_bits outside 0-62, smooth_mode not 0
 * or 1, hysteresis < 0 or > OFS_RTL_CHUNK_MAX_HYSTERESIS, max_events < 0, detect with a null n_events
 * or open_gate_start or with null events while max_events > 0.  There is no fall-back to the general
 * engine.  ofs_rtl_chunk_state_bytes returns the bytes of ONE stream's state (a multiple of 16) and
 * ofs_rtl_chunk_max_samples the largest Tc of one call; both return OFS_EINVAL (< 0) for an unsupported
 * n_br or Q.
 */
#define OFS_RTL_CHUNK_MAX_HYSTERESIS (1 << 28)
int64_t ofs_rtl_chunk_state_bytes(int32_t n_br, int32_t Q);
int64_t ofs_rtl_chunk_max_samples(int32_t n_br, int32_t Q);
int32_t ofs_minn_rtl_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc, int32_t Q,
                           int32_t smooth_shift, int32_t smooth_mode, int64_t threshold_value,
                           int32_t threshold_frac_bits, void* state,
                           double* corr_total, double* corr_positive, double* smooth_metric, double* energy_total,
                           double* corr_scaled, double* energy_scaled, uint8_t* metric_valid, uint8_t* above_threshold,
                           int32_t detect, int32_t hysteresis, int32_t timing_offset, int32_t max_events,
                           int32_t* n_events, int64_t* events, int64_t* open_gate_start, int32_t final, void* stream);

/*
 * Gate / peak FSM alone on precomputed metric arrays: replaces minn_rtl.detect_minn_rtl
 * (minn_rtl.py:750-825) when called on an existing MinnRTLMetricState.
 *   corr_positive: [B][T] f64; above_threshold, metric_valid: [B][T] uint8 (0/1);
 *   outputs as for ofs_minn_rtl.
 */
int32_t ofs_minn_rtl_gate(const double* corr_positive, const uint8_t* above_threshold,
                          const uint8_t* metric_valid, int64_t B, int64_t T,
                          int32_t hysteresis, int32_t timing_offset, int32_t max_events,
                          int32_t* n_events, int64_t* events, int64_t* open_gate_start,
                          void* stream);

/*
 * combined_sc_min detector front end (combined_sc_min.py:333-334: minn_streaming_metric and
 * schmidl_cox_streaming_metric on the same rx): both metrics in one pass over the input
 * (fused fp32 kernel for complex64 / 1-2 branches / N/4 a multiple of 64; otherwise the two
 * kernels above back to back).  Outputs as ofs_sc_metric (r_mode 1) and ofs_minn_metric.
 */
int32_t ofs_sc_minn_metric(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                           int32_t symbol_len, int32_t precision, void* M_sc, void* P_sc, void* R_sc,
                           void* M_minn, void* P_minn, void* R_minn, void* stream);

/*
 * Which kernel a window-metric call runs on: kind 1 = ofs_sc_metric r_mode 0, 2 = r_mode 1,
 * 3 = ofs_minn_metric, 4 = ofs_sc_minn_metric.  Returns 10*E + MW of the streaming fp32 fast kernel (win_fast.hip:
 * complex64, 1-2 branches, any T >= N, window of MW rows of 64*E samples), or 0 for the general
 * LDS-tiled engine.
 */
int32_t ofs_win_plan(int32_t kind, int32_t in_fmt, int32_t precision, int32_t n_br, int64_t T,
                     int32_t symbol_len);

/*
 * Resumable chunked S&C / combined S&C / Minn window metrics for complex64 streams: the chunk-fed form
 * of the streaming fp32 fast kernel behind ofs_sc_metric / ofs_minn_metric (ofs_win_plan > 0).  The
 * reference's sc.sc_streaming_metric, combined_sc_min.schmidl_cox_streaming_metric and
 * minn.minn_streaming_metric(_parameterized) are the specification.
 *
 * A stream is fed in consecutive chunks of Tc samples; ofs_win_metric_chunk returns M, P, R at the
 * chunk's samples and keeps what the next call needs (the last 1.5 N samples at most, and the fp64 row
 * bases of the one-shot kernel) in a caller-owned state buffer on the device.  The library allocates
 * nothing and keeps no global state.
 *   kind    1 = ofs_sc_metric r_mode 0, 2 = ofs_sc_metric r_mode 1, 3 = ofs_minn_metric (as ofs_win_plan;
 *           kind 4, the fused kernel, has no chunked form).
 *   x       [B][n_br][Tc] complex64 (this call's chunk), branches summed.  Supported (kind, n_br,
 *           symbol_len) are exactly those with ofs_win_plan(kind, OFS_C64, OFS_FP32, n_br, T, symbol_len) > 0
 *           for some T >= symbol_len: n_br 1-2, the window W = symbol_len / 2 (kinds 1, 2) or
 *           symbol_len / 4 (kind 3) one of 128, 256, 512, 1024, 2048, and W = 2048 with one branch only.
 *   state   [B][ofs_win_chunk_state_bytes(kind, n_br, symbol_len)] bytes, 16-byte aligned, device memory.
 *           The layout is opaque; ALL-ZERO BYTES ARE A FRESH STREAM, so any subset of streams is reset
 *           with a memset of its rows (stream-ordered with the calls).  One state row belongs to one
 *           stream: kind, n_br and symbol_len must not change between the calls of a stream, and the
 *           calls of a stream must be ordered (same HIP stream, or synchronised by the caller).
 *   M, P, R [B][Tc] f32 / c64 / f32, EACH nullable.  Element i of a call belongs to the stream's newest
 *           sample n = (samples of earlier calls) + i, that is to the reference's output index
 *           d = n - (symbol_len - 1).  Elements with d < 0 are written as +0.0 (all-zero bits) for any
 *           input, NaN and Inf included.  The fill phase is decided per stream on n, so after a reset of
 *           some state rows the streams of one call may be at different n.
 *   d0      [B] int64, nullable; every call writes the d of its element 0 (negative while a stream fills).
 *   final   != 0 changes nothing in the outputs; the state is a fresh stream again after the call.
 *   Tc      1 .. ofs_win_chunk_max_samples(kind, n_br, symbol_len) = 2^30 (in-call positions - at most
 *           1.5 * symbol_len + 255 history samples, the chunk and one row of padding - stay below
 *           2^31); Tc = 0 with final != 0 is a flush: no samples, d0 written, the streams fresh afterwards
 *           (x and the arrays unused).
 * EQUIVALENCE GUARANTEE.  For any split of a stream of T >= symbol_len samples into chunks, each output
 * array concatenated over the calls, with its first symbol_len - 1 elements dropped, equals BIT FOR BIT
 * the [T - symbol_len + 1] array that ONE ofs_sc_metric (kinds 1, 2) or ofs_minn_metric (kind 3) call with
 * OFS_C64 and OFS_FP32 returns on the whole stream on its fast plan - whichever of M / P / R are
 * requested here.  Exception: behind non-finite samples an output word is a NaN exactly where the
 * one-shot call's is, with the same payload, but its SIGN bit is outside the guarantee (as for
 * ofs_aa_detect_chunk_f32).
 * STREAM LENGTH.  The state carries the fp64 running sums C of the row totals since sample 0 (of the
 * lagged products and of the energy), and a window's "rows between" term is a difference of two of
 * them, so its absolute error grows as 2^-53 * |C|.  At unit amplitude |C| is about the sample count n,
 * and a window sum is about W with an fp32 ulp of 2^-23 * W: the carried error reaches one such ulp at
 * n = 2^30 * W samples (2^37 for W = 128, 2^41 for W = 2048: hours at 100 MS/s).  Up to there the
 * guarantee above is what bounds the error (it is the one-shot call's); beyond it the outputs still
 * equal what a one-shot call of that length would compute, but that value itself degrades.  final (or
 * zeroing the state) restarts C.  Energy far above unit amplitude shortens the span in proportion.
 * Calls are stream-ordered and never synchronise with the host: consecutive chunks may be enqueued back
 * to back.  OFS_EINVAL (before any launch): an unsupported (kind, n_br, symbol_len), Tc < 0 or above the
 * limit, Tc = 0 without final, B < 0, a null or misaligned state with B > 0, a null x with B * Tc > 0.
 * B = 0 is a valid no-op.  There is no fall-back to the general engine.  ofs_win_chunk_state_bytes
 * returns the bytes of ONE stream's state (a multiple of 16) and ofs_win_chunk_max_samples the largest
 * Tc of one call; both return OFS_EINVAL (< 0) for an unsupported shape.
 */
int64_t ofs_win_chunk_state_bytes(int32_t kind, int32_t n_br, int32_t symbol_len);
int64_t ofs_win_chunk_max_samples(int32_t kind, int32_t n_br, int32_t symbol_len);
int32_t ofs_win_metric_chunk(int32_t kind, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                             int32_t symbol_len, void* state, void* M, void* P, void* R,
                             int64_t* d0, int32_t final, void* stream);

/*
 * CP-correlation CFO: replaces core.estimate_cfo_from_cp (core.py:179-196), batched with a
 * per-stream CP start.  starts: [B] int64 (device); P_out: [B][2] f64 (nullable);
 * cfo_out: [B] f64.  Windows must lie inside [0, T) (checked by the caller).
 */
int32_t ofs_cp_cfo(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                   const int64_t* starts, int32_t n_fft, int32_t cp_len, double fs_hz,
                   double* P_out, double* cfo_out, void* stream);

/*
 * CP-correlation searches around an estimated CP start est[b], with
 * P_w(d) = sum_br sum_{n<win_len} x[d+n]·conj(x[d+n+n_fft]) over d in
 * [max(0, est - span), min(T - (n_fft + win_len), est + span)):
 *   mode OFS_CPS_ROBUST (0): cfo from the angle of sum_d P_w(d) — replaces
 *        core.estimate_cfo_from_cp_robust (core.py:199-231) with win_len = its `win`;
 *   mode OFS_CPS_PEAK (1):   d* = first argmax |P_w(d)|, cfo from P_w(d*) — replaces
 *        core.estimate_cfo_from_cp_peak / _peak_with_index (core.py:234-303) and
 *        core.find_cp_start_via_corr (core.py:306-336; span = search_half) with win_len = cp_len.
 * est: [B] int64; P_out [B][2] f64 and d_out [B] int64 nullable; cfo_out [B] f64;
 * status [B] int32: 0 searched, 1 empty range (the reference then falls back to
 * estimate_cfo_from_cp at est: the caller runs ofs_cp_cfo; d_out = est, cfo_out = NaN).
 * Windows are summed directly in fp64 (no prefix differences).
 * Mode 1 skips a window whose |P_w(d)| is NaN (it never compares above, as in the reference's
 * `mag > best_mag`); a non-empty range without any comparable window gives the reference's
 * initial values (core.py:289-291): d_out = the range's first offset max(0, est - span),
 * P_out = (0, 0), cfo_out = -0.0, status 0.
 */
#define OFS_CPS_ROBUST 0
#define OFS_CPS_PEAK   1
int32_t ofs_cp_search(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                      const int64_t* est, int32_t n_fft, int32_t win_len, int32_t span,
                      int32_t mode, double fs_hz, double* P_out, int64_t* d_out,
                      double* cfo_out, int32_t* status, void* stream);

/*
 * Receiver back-end after sync, batched over frames: the chain of sc.run_simulation
 * (sc.py:274-311) over core.py helpers - estimate_cfo_from_cp (core.py:179-196, skipped when
 * cfo_in is given), apply_cfo(-cfo) (:123-138) + branch mean, ofdm_fft_used (:171-176),
 * ls_channel_estimate (:339-341), estimate_timing_offset_from_phase_slope (:443-469),
 * equalize (:344-345), align_complex_gain (:357-362), evm_rms_db (:365-370).  fp64.
 *   pilot_start / data_start [B] int64: CP start of the pilot / data symbol (device);
 *   cfo_in [B] f64 or NULL; bins [n_used] int32 (device): centred subcarrier indices k, used
 *   for the gather X[k mod N] (= fftshift + (N/2 + k) % N) and as the fit's abscissa;
 *   pilot_used / data_used: c128 [.. ][n_used] known symbols, row stride (elements) per frame
 *   (0 = one row shared by all frames);  n_fft a power of two <= 4096.
 * Outputs (device, nullable): cfo_out [B], h_out / xa_out c128 [B][n_used], gain_out c128 [B],
 * evm_out, evm_db_out, slope_out (rad/bin), sto_out (samples) [B] f64.
 * At the stream's edges (pilot_start / data_start may be negative or reach past T, T may be
 * shorter than n_fft; pinned by tests/backend_frames.py and tests/test_gpu_backend_exact.py):
 *   zero-fill: a window sample whose index i lies outside [0, T) is (+0, +0) - as is any zero
 *     sample, whatever the tone's signs (the branch sum starts from +0);
 *   pair-drop: the CP pair (pilot_start + n, pilot_start + n_fft + n), n < cp_len, counts only if
 *     both indices are in [0, T); with no pair left (cp_len = 0 included) cfo_out = -0.0;
 *   a frame decodes exactly like the same frame inside the stream padded with zeros at both ends
 *     (ofs_rx_backend_at with origin = -pad: bit for bit, apart from the sign of a zero cfo_out);
 *   windows wholly outside the stream: the spectrum is (+0, +0) on every bin, so h_out = ±0 with
 *     numpy's signs for 0 / (pilot + 1e-9) - its phases are 0, -0 or ±pi and slope_out / sto_out
 *     are np.unwrap's and the fit's on those - and a zero data window gives xa_out = gain_out = 0,
 *     evm_out = 1.  Every output stays finite.
 */
int32_t ofs_rx_backend(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                       int32_t n_fft, int32_t cp_len, double fs_hz, const int64_t* pilot_start,
                       const int64_t* data_start, const double* cfo_in, int32_t n_used,
                       const int32_t* bins, const void* pilot_used, int64_t pilot_stride,
                       const void* data_used, int64_t data_stride, double* cfo_out, void* h_out,
                       void* xa_out, void* gain_out, double* evm_out, double* evm_db_out,
                       double* slope_out, double* sto_out, void* stream);

/*
 * ofs_rx_backend with a stream origin, for frames cut out of a longer stream (ofs_frame_capture_chunk):
 * origin [B] int64 (device), origin[b] = the absolute stream index of x[b][.][0].  It enters the CFO
 * tone's phase index alone - exp(-i 2 pi cfo (origin + n) / fs) at local sample n - so a slice
 * x = stream[.., o : o + T] decoded with origin = o and starts shifted by -o gives, BIT FOR BIT, every
 * output of ofs_rx_backend on the whole stream.  The CP correlation and the bounds 0 <= n < T do not
 * depend on it.  origin == NULL is ofs_rx_backend (the same kernels).  Everything else as above.
 * origin is not checked: any int64 is taken, negative values included (a stream padded in front of
 * its first sample has origin = -pad), and the phase index origin + n is converted to double as it is.
 */
int32_t ofs_rx_backend_at(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                          int32_t n_fft, int32_t cp_len, double fs_hz, const int64_t* pilot_start,
                          const int64_t* data_start, const double* cfo_in, int32_t n_used,
                          const int32_t* bins, const void* pilot_used, int64_t pilot_stride,
                          const void* data_used, int64_t data_stride, double* cfo_out, void* h_out,
                          void* xa_out, void* gain_out, double* evm_out, double* evm_db_out,
                          double* slope_out, double* sto_out, const int64_t* origin, void* stream);

/*
 * ofs_rx_backend_at with the number of frames read on the device: n_active points to ONE int32 in device
 * memory (e.g. n_rows of ofs_frame_capture_compact, written by an earlier call on the same stream).  The
 * frames b < min(B, max(*n_active, 0)) are decoded exactly as ofs_rx_backend_at decodes them; no output
 * word of any other row is written.  B stays the capacity: it sizes the arrays, the argument checks and
 * the launch (the host does not know the count); a workgroup beyond the count leaves at once.
 * n_active == NULL is ofs_rx_backend_at (the same kernels).  n_active given with origin == NULL is
 * OFS_EINVAL.  Everything else as above.
 */
int32_t ofs_rx_backend_counted(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                               int32_t n_fft, int32_t cp_len, double fs_hz, const int64_t* pilot_start,
                               const int64_t* data_start, const double* cfo_in, int32_t n_used,
                               const int32_t* bins, const void* pilot_used, int64_t pilot_stride,
                               const void* data_used, int64_t data_stride, double* cfo_out, void* h_out,
                               void* xa_out, void* gain_out, double* evm_out, double* evm_db_out,
                               double* slope_out, double* sto_out, const int64_t* origin,
                               const int32_t* n_active, void* stream);

/*
 * Batched receive-stream synthesis (benchmark / test input): the channel +
 * impairment chain of channel.apply_channel (channel.py:80-98), core.apply_cfo
 * (core.py:123-138) and sync_aa.quantize_adc (sync_aa.py:263-291):
 *   out[b][br][n] = q(base[br][off_b + n] * exp(i 2 pi cfo_b n / fs) + CN(0, 10^(-snr_b/10)))
 * with off_b ~ U{0..max_offset-1}, snr_b ~ U[snr_lo, snr_hi] dB, cfo_b ~ U[cfo_lo, cfo_hi] Hz drawn
 * per stream from Philox-4x32-10(seed, b) (distribution-level, not numpy's stream).
 *   base: [n_br][base_len] c128 (device; unit-power faded preamble, zero past its end);
 *   out_fmt OFS_C64 | OFS_C128 | OFS_CI16 (q = round(x * adc_scale) clipped to [-2048, 2047]);
 *   out: [B][n_br][T]; params: [B][3] f64 = offset, snr_db, cfo_hz (nullable).
 */
int32_t ofs_synth_batch(const void* base, int64_t base_len, int32_t n_br, int64_t B, int64_t T,
                        int32_t max_offset, double snr_lo_db, double snr_hi_db, double cfo_lo_hz,
                        double cfo_hi_hz, double fs_hz, uint64_t seed, int32_t out_fmt,
                        double adc_scale, void* out, double* params, void* stream);

/*
 * Frame synthesis: the whole per-stream chain of sync_aa.run_single_test (sync_aa.py:699-738),
 * every stream its own frame and payload:
 *   frame_b = [pre_pad zeros][preamble][n_sym random-QPSK OFDM symbols + CP][post_pad zeros]
 *             (symbols as sync_aa.build_random_qpsk_symbol, sync_aa.py:238-260: QPSK on the n_bins
 *             FFT bins `bins` (centred index k -> k mod n_fft), inverse FFT, unit power, CP);
 *   y_br     = frame_b conv cir_br (sync_aa.py:611-621); rx_br = (y_br + CN(0, mean|y_br|^2 /
 *             10^(snr_b/10))) * exp(i 2 pi cfo_b n / fs) (:622-631, :637-645);
 *   if full_scale_ratio > 0: quantize_adc(rx, rms(rx over all branches) * full_scale_ratio)
 *             (:263-291, :726-735), 12 bits;
 *   out[b][br][t] = rx_br[win_start + off_b + t] (0 outside the frame), off_b ~ U{0..max_offset-1}.
 *   preconv: [n_br][pre_len + taps - 1] c128 = preamble conv cir_br (shared part, host-built);
 *   cir: [n_br][taps] c128; n_br <= 4; n_fft a power of two <= 4096.
 *   out_fmt OFS_C64 | OFS_C128 (dequantized values if quantized) | OFS_CI16 (ADC codes when
 *   quantized); params [B][4] f64 = window start, snr_db, cfo_hz, full scale (nullable);
 *   phases [B][n_sym][n_bins] u8 = the QPSK phase indices drawn (nullable).
 */
int32_t ofs_synth_frames(const void* preconv, int64_t preconv_len, const void* cir, int64_t taps,
                         int32_t n_br, int32_t pre_pad, int32_t pre_len, int32_t n_sym, int32_t n_fft,
                         int32_t cp_len, const int32_t* bins, int32_t n_bins, int32_t post_pad, int64_t B,
                         int64_t T, int64_t win_start, int32_t max_offset, double snr_lo_db,
                         double snr_hi_db, double cfo_lo_hz, double cfo_hi_hz, double fs_hz,
                         double full_scale_ratio, uint64_t seed, int32_t out_fmt, void* out,
                         double* params, uint8_t* phases, void* stream);

/*
 * Park mirror-symmetry metric: replaces park.park_streaming_metric (park.py:64-114).
 * half = N/2; outputs for d in [half, T-half-1], n_out = T - 2*half, laid out [B][n_out]:
 *   P (c64|c128) = sum_br sum_{k<half} x[d-k]*x[d+k]; E (f32|f64) = sum_br sum_{k<half}|x[d+k]|^2;
 *   M = |P|^2 / max(E, 1e-12)^2.  Each output nullable.  T < 2*half+1 or half == 0: nothing
 *   to compute, returns OFS_OK (the reference returns empty arrays).  Tile + halo must fit
 *   LDS: N <= 8190 (fp32) / 4094 (fp64), else OFS_ETOOLONG.
 */
int32_t ofs_park_metric(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                        int32_t N, int32_t precision, void* M, void* P, void* E, void* stream);

/*
 * Resumable chunked Park metric with a running peak, for streams of any length: the chunk-fed form of
 * ofs_park_metric.  The reference's park.park_streaming_metric (park.py:64-114) and its detection
 * argmax(M) (park.py:161-164) are the specification.
 *
 * A stream is fed in consecutive chunks of Tc samples; ofs_park_metric_chunk returns M, P, E at the
 * chunk's samples and keeps what the next call needs (the last 2*half + 16 samples at most, in the
 * input's own format, and the running peak of M) in a caller-owned state buffer on the device.  The
 * library allocates nothing, reads no environment and keeps no global state.
 *   in_fmt, precision   one of the pairs (OFS_C64, OFS_FP32), (OFS_C128, OFS_FP64), (OFS_CI16, OFS_FP64).
 *   x       [B][n_br][Tc] samples in in_fmt (this call's chunk), branches summed; n_br >= 1.
 *   N       symbol length, half = N / 2 >= 1, N <= 8190 (fp32) / 4094 (fp64) as for ofs_park_metric.
 *   state   [B][ofs_park_chunk_state_bytes(in_fmt, n_br, N)] bytes, 16-byte aligned, device memory.
 *           The layout is opaque; ALL-ZERO BYTES ARE A FRESH STREAM, so any subset of streams is reset
 *           with a memset of its rows (stream-ordered with the calls).  One state row belongs to one
 *           stream: in_fmt, n_br and N must not change between the calls of a stream, and the calls of
 *           a stream must be ordered (same HIP stream, or synchronised by the caller).
 *   M, P, E [B][Tc] f32 / c64 / f32 (fp32) or f64 / c128 / f64 (fp64), EACH nullable.  Element j of a
 *           call belongs to the stream's newest sample n = (samples of earlier calls) + j, that is to
 *           the reference's centre index d = n - half + 1, the first d whose window
 *           x[d-half+1 .. d+half-1] is complete.  Elements with d < half (the reference has no such
 *           output) are written as +0.0 (all-zero bits) for any input, NaN and Inf included.  The fill
 *           phase is decided per stream on n, so after a reset of some state rows the streams of one
 *           call may be at different n.
 *   d0      [B] int64, nullable; every call writes the d of its element 0.
 *   peak_index [B] int64, peak_value [B] f64, each nullable: after every call the running np.argmax of
 *           M over the outputs the reference has on the stream's n samples so far (half <= d <=
 *           n - half - 1, see below), as ofs_row_argmax defines it (the first maximal element; the
 *           first NaN once one has appeared): the peak's d and its M widened to f64; -1 and 0.0 while
 *           the stream has no such output (n < 2*half + 1).  The peak advances only in calls that pass
 *           M.
 *   final   != 0 changes nothing in the outputs of this call (the peak outputs include its M); the
 *           state is a fresh stream again after the call.
 *   Tc      1 .. ofs_park_chunk_max_samples(in_fmt, n_br, N) = 2^30; Tc = 0 with final != 0 is a flush:
 *           no samples, d0 and the peak outputs written, the streams fresh afterwards (x and the arrays
 *           unused).
 * EQUIVALENCE GUARANTEE.  For any split of a stream of T >= 2*half + 1 samples into chunks, each output
 * array concatenated over the calls, with its first 2*half - 1 elements dropped, begins with, BIT FOR
 * BIT, the [T - 2*half] array that ONE ofs_park_metric call with the same in_fmt and precision returns
 * on the whole stream - whichever of M / P / E are requested here.  One element follows it: the output
 * d = T - half, whose window ends at the stream's last sample.  The reference and ofs_park_metric stop
 * one output earlier (they ask for sample d + half, which no sum reads); that element is what
 * ofs_park_metric returns at d on any longer stream.  The peak follows the reference: an output joins
 * it in the call that brings sample d + half, so after the last call peak_index - half and peak_value
 * equal what ofs_row_argmax returns on the one-shot call's M, and after every call they are the
 * argmax of what the one-shot call returns on the samples so far.  Variant PARK_DIRECT
 * (ofs_debug_set_variant) selects the energy form of both calls alike, so the pair stays equal.
 * Exception: behind non-finite samples an output word is a NaN exactly where the one-shot call's is,
 * but its SIGN bit is outside the guarantee (as for ofs_win_metric_chunk).
 * STREAM LENGTH.  The state carries samples and the peak, no sums: every output is computed from its
 * own window alone, so nothing degrades with the stream's length.  Only the sample count n limits it,
 * and that is an int64.
 * Calls are stream-ordered and never synchronise with the host: consecutive chunks may be enqueued back
 * to back (two kernels per call: the metric, then one small workgroup per stream that writes the
 * history, folds the peak and advances the state).  OFS_EINVAL (before any launch): a (in_fmt,
 * precision) pair other than the three above, n_br < 1, half < 1 or N above the limit, Tc < 0 or above
 * the limit, Tc = 0 without final, B < 0, a null or misaligned state with B > 0, a null x with
 * B * Tc > 0, peak_index or peak_value with a null M and B * Tc > 0.  B = 0 is a valid no-op.
 * ofs_park_chunk_state_bytes returns the bytes of ONE stream's state (a multiple of 16) and
 * ofs_park_chunk_max_samples the largest Tc of one call; both return OFS_EINVAL (< 0) for an
 * unsupported shape.
 */
int64_t ofs_park_chunk_state_bytes(int32_t in_fmt, int32_t n_br, int32_t N);
int64_t ofs_park_chunk_max_samples(int32_t in_fmt, int32_t n_br, int32_t N);
int32_t ofs_park_metric_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                              int32_t N, int32_t precision, void* state,
                              void* M, void* P, void* E, int64_t* d0,
                              int64_t* peak_index, double* peak_value,
                              int32_t final, void* stream);

/*
 * ZC matched filter / normaliser (fp64): replaces zc_v2.matched_filter_correlation
 * (zc_v2.py:244-254), normalize_correlation (:257-271), the branch combine of
 * detect_zc_preamble (:489-503) and the inline combiner of zc.py:106-126.
 *   ref: [N] c128 (device); ref_energy = sum |ref|^2 (host scalar, as the reference computes it);
 *   corr: c128 [B][n_br][T+N-1] (mode OFS_ZC_RAW) or [B][T+N-1] (other modes), nullable;
 *   corr_mag: f64 |corr| with the same layout, nullable (one of corr / corr_mag required);
 *   corr_in: c128 [B][T+N-1] raw correlation (OFS_ZC_NORMALIZE only, n_br must be 1).
 *   N + 2048 samples of halo must fit LDS (N <= 6100).
 */
int32_t ofs_zc_correlate(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                         const void* ref, int32_t N, double ref_energy, int32_t mode,
                         const void* corr_in, void* corr, double* corr_mag, void* stream);

/*
 * The same correlation by FFT overlap-save (SURVEY §8(f)3 "via FFT correlation"): fp64 rocFFT
 * transforms of M-sample blocks (M a power of two >= 2N, 0 = chosen to minimise the work),
 * pointwise product with FFT_M(conj(ref reversed)), inverse, then the valid outputs combined
 * and normalised per `mode` (OFS_ZC_RAW, _V2, _COMBINED, _SUM; as ofs_zc_correlate, the window
 * energy from an fp64 prefix over each block; ref_energy as ofs_zc_correlate).  The plan is made
 * for one reference (host c128, N taps) and one batch shape; `scratch` must hold *scratch_bytes (the [rows * blocks][M] c128
 * spectra), `work` *work_bytes (rocFFT work area, may be 0).  A plan carries its rocFFT execution
 * state: use it from one host thread / stream at a time (one plan per concurrent caller).
 *
 * Non-finite samples.  ofs_zc_correlate gives a non-finite output exactly where the N-sample window
 * holds a NaN or infinite sample, as the reference does.  Here a non-finite sample spoils its whole
 * block: every output of each block whose M-sample input span [q*S - (N-1), q*S - (N-1) + M) holds
 * it (S = M - N + 1; up to two blocks) may be NaN, which it is not in the reference.  Every output of
 * every other block and of every other stream is what it is without that sample, bit for bit.
 * Finite samples of any size: |corr| stays finite wherever corr does (|c| up to the fp64 range), and a
 * window whose energy overflows to +inf gives 0 (corr / inf, zc_v2.py:269-271); once a block's energy
 * prefix has overflowed, its later windows are summed directly.
 */
int32_t ofs_zc_mf_plan_create(const void* ref, int32_t N, int64_t B, int32_t n_br, int64_t T, int32_t M,
                              void** plan_out, size_t* work_bytes, size_t* scratch_bytes);
int32_t ofs_zc_mf_plan_destroy(void* plan);
int32_t ofs_zc_correlate_fft(void* plan, int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                             double ref_energy, int32_t mode, void* corr, double* corr_mag, void* scratch,
                             void* work, void* stream);

/*
 * ZC frequency-domain metric: replaces zc_freq.compute_frequency_metric (zc_freq.py:62-99).
 * For off in [0, T-(N+cp)]: 62-bin DFT of x[off+cp : off+cp+N] at fftshift positions
 * (N/2 + bin_indices) % N, metric = |sum_br vdot(t, bins)|^2 / max(E_t * sum_br sum|bins|^2, 1e-12).
 * bin_indices [n_bins] int32 and template_bins [n_bins] c128 are HOST pointers (n_bins <= 64);
 * metric: [B][T-(N+cp)+1] (device), f64 for OFS_FP64, f32 for OFS_FP32.
 *   OFS_FP64: sliding DFT in fp64 (zc_slide.hip: block-DFT-initialised chunks, four chunks per
 *     wave; N a multiple of 64, n_br <= 2), else the one-chunk-per-wave sliding DFT (n_br <= 4).
 *   OFS_FP32: few offsets per stream (<= 64, OFS_C64, N = 64*2^j <= 4096, the cfg5 shape): a
 *     per-window 64 x N/64 pruned FFT in fp32; otherwise the fp64 sliding DFT of zc_slide.hip with
 *     the metric rounded to fp32 (n_br <= 2, N a multiple of 64, blocks within LDS), else the
 *     one-chunk-per-wave fp64 sliding DFT with the metric rounded to fp32 (n_br <= 4).
 *   n_br > 4: OFS_EINVAL (cover it, and templates of more than 64 bins, with ofs_zc_freq_partial
 *     over branch / bin groups + ofs_zc_freq_finish, as the Python mirror does).
 * Returns OFS_ESHORT when T < N + cp (the reference raises ValueError).
 */
int32_t ofs_zc_freq_metric(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T,
                           int32_t N, int32_t cp, int32_t precision, int32_t n_bins,
                           const int32_t* bin_indices, const double* template_bins,
                           double template_energy, void* metric, void* stream);
/* which zc_freq kernel a one-branch shape runs on: 1 one-chunk-per-wave sliding DFT (fp64), 2 window
 * FFT (fp32), 3 N = 4096 window FFT with the column sums reduced across lanes (fp32; taken when the
 * template bins' residues mod 64 are distinct, as the PSS template's are, otherwise 2), 4 block-
 * initialised sliding DFT (fp64), 5 the same with the metric rounded to fp32, 6 the one-chunk-per-
 * wave sliding DFT with the metric rounded to fp32, 0 none */
int32_t ofs_zc_freq_plan(int32_t in_fmt, int32_t precision, int64_t T, int32_t N, int32_t cp);

/*
 * Resumable chunked zc_freq metric with a running peak, for streams of any length: the chunk-fed form
 * of ofs_zc_freq_metric on its sliding kernels (plans 4 / 5).  The reference's
 * zc_freq.compute_frequency_metric (zc_freq.py:62-99) and its detection int(np.argmax(metric))
 * (zc_freq.py:144) are the specification.
 *
 * A stream is fed in consecutive chunks of Tc samples; ofs_zc_freq_metric_chunk returns the metric at
 * the chunk's samples and keeps what the next call needs (the last N + C samples, in the input's own
 * format, and the running peak of the metric; C = 64, 128 or 256 is the sliding kernel's chunk length,
 * a function of N) in a caller-owned state buffer on the device.  The library allocates nothing, reads
 * no environment and keeps no global state.
 *   in_fmt, precision   one of the pairs (OFS_C64, OFS_FP32: fp64 arithmetic, the metric rounded to f32),
 *           (OFS_C128, OFS_FP64), (OFS_CI16, OFS_FP64).
 *   x       [B][n_br][Tc] samples in in_fmt (this call's chunk); n_br is 1 or 2.
 *   N, cp   the shapes the sliding kernel takes: N >= 64 and a multiple of 64, the blocks of a window
 *           within LDS; cp >= 0.
 *   n_bins, bin_indices, template_bins, template_energy   the template as for ofs_zc_freq_metric (HOST
 *           pointers, 1 <= n_bins <= 64), passed to every call; it must not change within a stream.  A
 *           template of mirror pairs (k, N - k) runs the pair body and any other the per-bin body, by
 *           the one-shot call's own rule.
 *   state   [B][ofs_zc_freq_chunk_state_bytes(in_fmt, n_br, N, cp)] bytes, 16-byte aligned, device
 *           memory.  The layout is opaque; ALL-ZERO BYTES ARE A FRESH STREAM, so any subset of streams
 *           is reset with a memset of its rows (stream-ordered with the calls).  One state row belongs
 *           to one stream: in_fmt, n_br, N, cp and the template must not change between the calls of a
 *           stream, and the calls of a stream must be ordered (same HIP stream, or synchronised by the
 *           caller).
 *   metric  [B][Tc] f32 (OFS_FP32) or f64, nullable.  Element j of a call belongs to the stream's newest
 *           sample n = (samples of earlier calls) + j, that is to offset s = n - (N + cp) + 1, the first
 *           offset whose window x[cp+s .. cp+s+N-1] is complete.  Elements with s < 0 are written as
 *           +0.0 (all-zero bits) for any input, NaN and Inf included.  The fill phase is decided per
 *           stream on n, so after a reset of some state rows the streams of one call may be at
 *           different n.  Without metric the call only takes the samples in.
 *   off0    [B] int64, nullable; every call writes the s of its element 0.
 *   peak_index [B] int64, peak_value [B] f64, each nullable: after every call the running np.argmax of
 *           the metric over the offsets 0 .. s_newest, as ofs_row_argmax defines it (the first maximal
 *           element; the first NaN once one has appeared): the peak's offset and its metric widened to
 *           f64; -1 and 0.0 while the stream has no output (n < N + cp).  The peak advances only in
 *           calls that pass metric.  Every computed output is one the reference has on the samples so
 *           far, so no output waits for a later call.
 *   final   != 0 changes nothing in the outputs of this call; the state is a fresh stream again after
 *           the call.
 *   Tc      1 .. ofs_zc_freq_chunk_max_samples(in_fmt, n_br, N, cp) = 2^30; Tc = 0 with final != 0 is a
 *           flush: no samples, off0 and the peak outputs written, the streams fresh afterwards (x and
 *           metric unused).
 * EQUIVALENCE GUARANTEE.  For any split of a stream of T >= N + cp samples into chunks, the metric
 * concatenated over the calls, with its first N + cp - 1 elements dropped, equals BIT FOR BIT the
 * [T - (N+cp) + 1] array that ONE ofs_zc_freq_metric call with the same in_fmt and precision returns
 * on the whole stream from its sliding kernel (ofs_zc_freq_plan 4 / 5).  After the last call the peak
 * equals ofs_row_argmax of that array, and after every call it is the argmax of what the one-shot call
 * returns on the samples so far.  The ZS_* variants (ofs_debug_set_variant) select the form of both
 * calls alike.  Outside the guarantee: the SIGN bit of a NaN output (a NaN appears exactly where the
 * one-shot call has one), and the one-shot call's fp32 window-FFT plans (2 / 3: OFS_C64 with at most
 * 64 offsets), which are another arithmetic.
 * STREAM LENGTH.  The state carries samples and the peak, no sums: every output is computed from the
 * samples of its own chunk of C offsets alone, so nothing degrades with the stream's length.  Only
 * the sample count n limits it, and that is an int64.
 * Calls are stream-ordered and never synchronise with the host: consecutive chunks may be enqueued back
 * to back (two kernels per call: the metric, then one small workgroup per stream that writes the
 * history, folds the peak and advances the state).  OFS_EINVAL (before any launch): a (in_fmt,
 * precision) pair other than the three above, n_br other than 1 or 2, N below 64 or no multiple of 64
 * or beyond LDS, cp < 0, n_bins outside 1..64, a null bin_indices or template_bins, Tc < 0 or above
 * the limit, Tc = 0 without final, B < 0, a null or misaligned state with B > 0, a null x with
 * B * Tc > 0, peak_index or peak_value with a null metric and B * Tc > 0.  B = 0 is a valid no-op.
 * ofs_zc_freq_chunk_state_bytes returns the bytes of ONE stream's state (64 + n_br * (N + C) * sample
 * bytes, a multiple of 16) and ofs_zc_freq_chunk_max_samples the largest Tc of one call; both return
 * OFS_EINVAL (< 0) for an unsupported shape.
 */
int64_t ofs_zc_freq_chunk_state_bytes(int32_t in_fmt, int32_t n_br, int32_t N, int32_t cp);
int64_t ofs_zc_freq_chunk_max_samples(int32_t in_fmt, int32_t n_br, int32_t N, int32_t cp);
int32_t ofs_zc_freq_metric_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                                 int32_t N, int32_t cp, int32_t precision, int32_t n_bins,
                                 const int32_t* bin_indices, const double* template_bins,
                                 double template_energy, void* state, void* metric, int64_t* off0,
                                 int64_t* peak_index, double* peak_value, int32_t final, void* stream);

/* Partial sums of the zc_freq metric over one group of branches and one group of template bins, so
 * any branch count and any template length reduce to kernels of <= 4 branches x <= 64 bins (the
 * reference loops over every branch and bin, zc_freq.py:85-97).  For off in [0, noff), noff =
 * T-(N+cp)+1, with bins b_{br,j} as in ofs_zc_freq_metric over branches br0 .. br0+n_grp-1 of x
 * ([B][n_br][T]) and the n_bins (<= 64) given bins:
 *   part[b][off] = (Re C, Im C, D),  C = Σ_br Σ_j conj(t_j)·b_{br,j},  D = Σ_br Σ_j |b_{br,j}|²
 * stored, or added onto part when accumulate != 0 (part: [B][noff][3] f64, device).  The groups'
 * C and D add exactly as the reference's per-branch vdot / energy sums do, before the one
 * normalisation of ofs_zc_freq_finish.  fp64 sliding DFT (one chunk of offsets per wave). */
int32_t ofs_zc_freq_partial(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T, int32_t br0,
                            int32_t n_grp, int32_t N, int32_t cp, int32_t n_bins, const int32_t* bin_indices,
                            const double* template_bins, int32_t accumulate, double* part, void* stream);
/* metric[b][off] = |C|² / max(E_t·D, 1e-12) from accumulated partial sums; f32 (OFS_FP32) or f64 out. */
int32_t ofs_zc_freq_finish(const double* part, int64_t B, int64_t noff, double template_energy,
                           int32_t precision, void* metric, void* stream);

/*
 * rocFFT leg of the ZC frequency-domain metric (zc_freq.py:62-99 and the argmax of
 * zc_freq.py:144), the north-star "rocFFT + HIP conj-mul/|.|^2/argmax" formulation, kept beside
 * the fused window-FFT kernel of ofs_zc_freq_metric for comparison (it writes and re-reads the
 * full spectrum).  A plan is a batched forward C2C rocFFT plan over n_windows = B * n_br windows
 * of N samples, input distance in_dist (= T), out-of-place into a dense [n_windows][N] spectrum;
 * it is host state owned by the caller (create once per shape, destroy when done).
 *   precision OFS_FP32: complex64 input/spectrum, f32 metric; OFS_FP64: complex128, f64 metric.
 *   work_bytes: size of the rocFFT work buffer the caller passes to ofs_zc_freq_metric_fft.
 */
int32_t ofs_zc_fft_plan_create(int32_t precision, int32_t N, int64_t n_windows, int64_t in_dist,
                               void** plan, size_t* work_bytes);
/* As ofs_zc_fft_plan_create; prune_bins > 0 (N a power of two <= 4096) makes the plan PRUNED: a
 * rocFFT store callback keeps only the template bins, so ofs_zc_freq_metric_fft's `spectrum` is
 * a compact [n_windows][prune_bins] buffer (n_bins must equal prune_bins) and the dense N-point
 * spectrum never reaches HBM.  prune_bins == 0: the dense plan. */
int32_t ofs_zc_fft_plan_create2(int32_t precision, int32_t N, int64_t n_windows, int64_t in_dist,
                                int32_t prune_bins, void** plan_out, size_t* work_bytes);
/* As ofs_zc_fft_plan_create2, executed in chunks of chunk_windows windows (0 = all n_windows in
 * one execution; a multiple of n_br at execute time): each chunk is one rocFFT execution into the
 * same [chunk][N] (or [chunk][prune_bins]) `spectrum` buffer followed by its gather, so the
 * spectrum the FFT writes is re-read from the Infinity Cache instead of HBM when chunk * N * esz
 * is well inside its 256 MiB.  ofs_zc_fft_plan_chunk returns the windows per execution (the
 * spectrum buffer's row count). */
int32_t ofs_zc_fft_plan_create3(int32_t precision, int32_t N, int64_t n_windows, int64_t in_dist,
                                int32_t prune_bins, int64_t chunk_windows, void** plan_out,
                                size_t* work_bytes);
/* ROWS plan for the reference's sliding shape (many offsets per stream): one rocFFT execution covers
 * EVERY offset of rows_per_exec consecutive [T]-sample rows (rows = stream x branch; 0 = all
 * total_rows; at execute time a multiple of n_br) - its windows start at sample cp of the first row
 * at a distance of ONE sample, (rows-1)*T + n_off of them (N a power of two <= 4096).  prune_bins =
 * n_bins: the store callback keeps the template bins of the windows that lie inside one row, spectrum
 * buffer [ofs_zc_fft_plan_chunk(plan)][prune_bins]; prune_bins = 0: no callback (rocFFT's callback
 * path blocks the host per execution), every window's dense spectrum goes to a
 * [ofs_zc_fft_plan_chunk(plan)][N] buffer and the gather reads the template bins from it.
 * ofs_zc_freq_metric_fft then issues 2 launches per row group instead of 2 per offset.  The FFTs
 * cover T instead of n_off windows per row (T / n_off times the per-offset plan's transforms). */
int32_t ofs_zc_fft_plan_create_rows(int32_t precision, int32_t N, int32_t cp, int64_t T,
                                    int64_t total_rows, int64_t rows_per_exec, int32_t prune_bins,
                                    void** plan_out, size_t* work_bytes);
int64_t ofs_zc_fft_plan_chunk(const void* plan);
int32_t ofs_zc_fft_plan_destroy(void* plan);
/*
 * For each offset off in [0, T-(N+cp)]: one batched rocFFT of x[b][br][off+cp : off+cp+N] into
 * `spectrum` ([chunk][N] device scratch, chunk = ofs_zc_fft_plan_chunk = B*n_br unless the plan
 * is chunked), then one gather kernel: metric[b][off] =
 * |sum_br vdot(t, bins)|^2 / max(E_t * sum_br sum |bins|^2, 1e-12), bins at the reference's
 * fftshift positions (N/2 + bin_indices) % N.  bin_indices [n_bins] int32, template_bins [n_bins]
 * c128: HOST pointers (n_bins <= 64).  metric [B][n_off]; peak_index [B] int64 / peak_value [B]
 * f64 (nullable) = first argmax of each row (np.argmax).  Returns OFS_ESHORT when T < N + cp.
 */
int32_t ofs_zc_freq_metric_fft(void* plan, int32_t in_fmt, const void* x, int64_t B, int32_t n_br,
                               int64_t T, int32_t N, int32_t cp, int32_t n_bins,
                               const int32_t* bin_indices, const double* template_bins,
                               double template_energy, void* spectrum, void* work, void* metric,
                               int64_t* peak_index, double* peak_value, void* stream);
/* first argmax of each row of v [B][n] (f32 | f64 per precision), np.argmax semantics (the first
 * maximal element; the first NaN if any): index [B] int64, value [B] f64, each nullable. */
int32_t ofs_row_argmax(int32_t precision, const void* v, int64_t B, int64_t n, int64_t* index,
                       double* value, void* stream);

/*
 * ZC CFAR + gate: replaces zc_v2.zc_streaming_detection (zc_v2.py:300-346) fused with
 * detect_zc_peaks (:374-446).  corr_mag: [B][n] f64.  Outputs [B][n], each nullable:
 * local_sum, corr_scaled, thresh_scaled (f64), above_threshold, metric_valid, gate_mask (u8).
 * n_events [B] int32 (total, may exceed max_events); ev_int [B][max_events][4] int64 =
 * peak_index, gate_start, gate_end, detected_start; ev_peak [B][max_events] f64 peak_value.
 * The running sum is the reference's sequential float64 recursion (bit-identical).
 */
int32_t ofs_zc_detect(const double* corr_mag, int64_t B, int64_t n, int32_t window_size,
                      int64_t thresh_value, int32_t thresh_frac_bits, double min_corr_mag,
                      int32_t reference_length, int32_t hysteresis, double* local_sum,
                      double* corr_scaled, double* thresh_scaled, uint8_t* above_threshold,
                      uint8_t* metric_valid, uint8_t* gate_mask, int32_t max_events,
                      int32_t* n_events, int64_t* ev_int, double* ev_peak, void* stream);
/*
 * Which kernel ofs_zc_detect launches for streams of n samples (no GPU call): 0 the sequential
 * one-wave-per-stream kernel (max(hysteresis, 1) < 64, or variant ZC_SEQ), 1 the fused kernel with
 * register-staged tiles, 2 the fused kernel with LDS-DMA tiles storing events and gate_mask only,
 * 3 the fused kernel with LDS-DMA tiles and state arrays.  want_state: any of local_sum,
 * corr_scaled, thresh_scaled is requested; aligned16: corr_mag is 16-byte aligned.  LDS-DMA needs n
 * and max(window_size, 1) whole multiples of 128, an aligned corr_mag and variant ZC_NODMA unset.
 * ofs_zc_detect takes its decision from the same function.
 */
int32_t ofs_zc_detect_plan(int64_t n, int32_t window_size, int32_t hysteresis, int32_t want_state,
                           int32_t aligned16);

/* Gate alone on caller-provided flags: replaces zc_v2.detect_zc_peaks (zc_v2.py:374-446). */
int32_t ofs_zc_gate(const double* corr_mag, const uint8_t* above_threshold, const uint8_t* metric_valid,
                    int64_t B, int64_t n, int32_t reference_length, int32_t hysteresis,
                    uint8_t* gate_mask, int32_t max_events, int32_t* n_events, int64_t* ev_int,
                    double* ev_peak, void* stream);

/*
 * Resumable chunked zc_v2 CFAR + gate for magnitude streams of any length (the reference calls
 * zc_streaming_detection "FPGA-friendly streaming detection", zc_v2.py:300-346 + :374-446; its
 * sample-by-sample loops are the specification).
 *
 * A stream's |corr| is fed in consecutive chunks of Tc samples; ofs_zc_detect_chunk returns the chunk's
 * CFAR arrays, its gate mask and the gate events that CLOSED among its samples, and keeps what the next
 * call needs in a caller-owned state buffer on the device.  The library allocates nothing and keeps no
 * global state.
 *   corr_mag  f64; row b starts at corr_mag + b * ld_mag (elements), ld_mag >= Tc: a column slice of a
 *           wider buffer (the matched filter's output, say) is passed in place.  Rows need only 8-byte
 *           alignment.  Element i of a call is the stream's absolute sample
 *           n = (samples of earlier calls) + i.  W = max(1, window_size); metric_valid = n >= W.  The
 *           fill phase is decided PER STREAM on n, not per call: after a reset of some state rows the
 *           streams of one call are at different n.
 *   state   [B][ofs_zc_chunk_state_bytes(window_size)] bytes, 16-byte aligned, device memory.  The
 *           layout is opaque: it holds the running sum acc, the last W magnitudes, the int64 sample
 *           count and the gate machine (open, gate_start, peak_index, peak_value, last above sample).
 *           ALL-ZERO BYTES ARE A FRESH STREAM, so any subset of streams is reset with a memset of its
 *           rows (stream-ordered with the calls).  window_size, thresh_value, thresh_frac_bits,
 *           min_corr_mag, reference_length and hysteresis must not change between the calls of a
 *           stream (max_events and which arrays are requested may), and the calls of a stream must be
 *           ordered (same HIP stream, or synchronised by the caller).  W is 1 .. OFS_ZC_CHUNK_MAX_WINDOW.
 *   local_sum .. gate_mask  dense [B][Tc], f64 / uint8 as in ofs_zc_detect, EACH nullable (events +
 *           gate_mask only is the benchmarked mode); the values are those of ofs_zc_detect at the same
 *           absolute sample.
 *   events  only the gates that closed among this call's samples, written from slot 0 of every call,
 *           ABSOLUTE int64 indices: ev_int [B][max_events][4] = peak_index, gate_start, gate_end,
 *           detected_start = max(0, peak_index - reference_length + 1); ev_peak [B][max_events] the
 *           peak value.  n_events[b] is exact also above max_events; slots at or beyond
 *           min(n_events, max_events) are not written.  The peak is the FIRST maximum of corr_mag in
 *           the gate (strict >, the opening sample is the first candidate), across calls too.  A gate
 *           still open at the end of the chunk is carried, over any number of calls.
 *   open_gate_start [B], written by every call: the absolute start of the gate that is open after the
 *           call's last sample, or -1.  On a final call it names the gate that `final` then closes.
 *   final   != 0: an open gate closes with gate_end = the stream's sample count, as ofs_zc_detect does
 *           at n, and emits its event; the state is a fresh stream afterwards.  Tc = 0 with final != 0
 *           is a flush (no samples; corr_mag and the arrays unused); Tc = 0 without final is OFS_EINVAL.
 * EQUIVALENCE GUARANTEE.  For any split of a stream into chunks, on ANY float64 input (the running sum
 * is the reference's literal left-to-right recursion acc = (acc + c[n]) - c[n - W] with acc and the
 * last W magnitudes carried), the concatenated arrays and the concatenated events equal bit for bit
 * what ONE ofs_zc_detect call on the whole stream returns, with one exception in gate_mask: the
 * reference sets gate_mask[gate_start:n] for a gate still open at the end (zc_v2.py:444), which
 * includes the start sample that a closed gate never gets.  The final call sets it wherever those
 * samples lie in its own chunk; if gate_start lies in an earlier call, that single sample was already
 * returned as 0, and the last call's open_gate_start names it.
 * Calls are stream-ordered and never synchronise with the host: consecutive chunks may be enqueued
 * back to back.  OFS_EINVAL (before any launch): B < 0 or Tc < 0, Tc = 0 without final, ld_mag < Tc
 * with B > 1, a window_size above OFS_ZC_CHUNK_MAX_WINDOW, thresh_frac_bits outside 0-62,
 * hysteresis < 0 or > OFS_ZC_CHUNK_MAX_HYSTERESIS, max_events < 0, a null or misaligned state with
 * B > 0, a null corr_mag with B * Tc > 0 or one that is not 8-byte aligned, a null n_events or
 * open_gate_start with B > 0, null event arrays with max_events > 0.  B = 0 is a valid no-op with every
 * pointer null.  ofs_zc_chunk_state_bytes returns the bytes of ONE stream's state (a multiple of 16),
 * or OFS_EINVAL (< 0) for a window_size below 0 or above the limit (0 counts as 1).
 */
#define OFS_ZC_CHUNK_MAX_WINDOW     (1 << 16)
#define OFS_ZC_CHUNK_MAX_HYSTERESIS (1 << 28)
int64_t ofs_zc_chunk_state_bytes(int32_t window_size);
int32_t ofs_zc_detect_chunk(const double* corr_mag, int64_t ld_mag, int64_t B, int64_t Tc,
                            int32_t window_size, int64_t thresh_value, int32_t thresh_frac_bits,
                            double min_corr_mag, int32_t reference_length, int32_t hysteresis,
                            void* state,
                            double* local_sum, double* corr_scaled, double* thresh_scaled,
                            uint8_t* above_threshold, uint8_t* metric_valid, uint8_t* gate_mask,
                            int32_t max_events, int32_t* n_events, int64_t* ev_int, double* ev_peak,
                            int64_t* open_gate_start, int32_t final, void* stream);

/*
 * Resumable frame capture for chunk-fed streams: the link between the chunked detectors, whose events
 * arrive after the frame's samples have left, and ofs_rx_backend_at, which wants the frame resident.
 *
 * A stream is fed in consecutive chunks of Tc samples.  The state (caller-owned, on the device) keeps the
 * last `history` samples of every branch in the input's own format and a queue of at most `max_pending`
 * frame starts.  Each call takes trigger indices from device memory - typically the frame_start column
 * of a detector's event buffer written by the same push, so no host round trip - and emits every frame
 * [s, s + frame_len) whose last sample has arrived, across any chunking.  The library allocates nothing,
 * reads no environment and keeps no global state.
 *   in_fmt     OFS_C64, OFS_C128 or OFS_CI16.  Packed 12-bit words (OFS_CP12) are not supported: their
 *              samples straddle bytes, so a frame at an arbitrary start is no byte copy.
 *   x          [B][n_br][Tc] samples in in_fmt (this call's chunk); n_br >= 1, branches kept apart.
 *   frame_len  F >= 1 samples per frame and branch.
 *   history    H, F <= H <= 2^30 - 4: the samples before the current chunk that stay retrievable.
 *   max_pending  Q in 1 .. 16: queued starts per stream, and frames one call can emit per stream.
 *   offset     added to every trigger; negative values capture a lead-in.
 *   trig, trig_ld, trig_stride, n_trig, trig_max   stream b has k = min(max(n_trig[b], 0), trig_max)
 *              triggers, trigger j gives s = trig[b * trig_ld + j * trig_stride] + offset (int64 elements;
 *              n_trig [B] int32).  n_trig == NULL: no triggers in this call.  With ev_int [B][E][4] of
 *              ofs_aa_detect_chunk(_f32): trig = &ev_int[0][0][3], trig_ld = 4 * E, trig_stride = 4,
 *              n_trig = n_events, trig_max = E.
 *   state      [B][ofs_frame_capture_state_bytes(in_fmt, n_br, frame_len, history, max_pending)] bytes,
 *              16-byte aligned, device memory.  The layout is opaque; ALL-ZERO BYTES ARE A FRESH STREAM,
 *              so any subset of streams is reset with a memset of its rows (stream-ordered with the
 *              calls); in_fmt, n_br, frame_len, history and max_pending must not change between the calls
 *              of a stream, and the calls of a stream must be ordered.
 *   frames     [B][Q][n_br][F] samples in in_fmt, aligned to one sample.
 *   frame_start [B][Q] int64, n_frames [B] int32, dropped [B][3] int32.
 * Per stream, with n0 samples before the call and n1 = n0 + Tc, in this order:
 *   1. Triggers in index order: s < max(0, n0 - H) (the samples are gone, or the index is negative) counts
 *      in dropped[b][0] (late); else, with Q starts pending, in dropped[b][1] (queue full); else s joins
 *      the queue.  Lateness is decided by `history` alone, whatever the storage is rounded to.
 *   2. Pending starts in queue order: if s + F <= n1 the frame leaves the queue into the next output
 *      slot: frame_start[b][slot] = s and frames[b][slot][br][0:F] = the stream's samples [s, s + F) of
 *      every branch, bit for bit.  (H >= F: a queued start is still retrievable when it completes.)
 *   3. n_frames[b] = slots written; frame_start[b][slot] = -1 for the unused slots; the sample words of
 *      unused slots are left untouched; dropped[b][0..2] are this call's counts.  All written by every call.
 *   4. final != 0: starts still pending count in dropped[b][2] (cut by the stream's end) and the stream
 *      is fresh after the call.
 *   5. Otherwise the state takes the chunk's newest samples and n1.
 * Overlapping frames, unsorted triggers and several frames per call follow from these rules.  s + offset
 * must not overflow int64.
 *   Tc         any length >= 1 (there is no upper limit); Tc = 0 with final != 0 is a flush (x unused).
 * Calls are stream-ordered and never synchronise with the host (two kernels per call: the gather, then
 * one small workgroup per stream that writes the history, the bookkeeping outputs and the state).
 * OFS_EINVAL (before any launch): a format other than the three above, n_br < 1, frame_len < 1, history <
 * frame_len or above the limit, max_pending outside 1 .. 16, trig_max < 0, a null trig with n_trig given
 * and trig_max > 0, B < 0, Tc < 0, Tc = 0 without final, a null or misaligned state or a null output with
 * B > 0, a null x with B * Tc > 0.  B = 0 is a valid no-op.  ofs_frame_capture_state_bytes returns the
 * bytes of ONE stream's state (a multiple of 16), or OFS_EINVAL (< 0) for unsupported arguments.
 */
int64_t ofs_frame_capture_state_bytes(int32_t in_fmt, int32_t n_br, int32_t frame_len, int32_t history,
                                      int32_t max_pending);
int32_t ofs_frame_capture_chunk(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                                int32_t frame_len, int32_t history, int32_t max_pending, int64_t offset,
                                const int64_t* trig, int64_t trig_ld, int64_t trig_stride,
                                const int32_t* n_trig, int32_t trig_max, void* state,
                                void* frames, int64_t* frame_start, int32_t* n_frames, int32_t* dropped,
                                int32_t final, void* stream);

/*
 * ofs_frame_capture_chunk with the frames written densely and their number left in device memory, so that
 * ofs_rx_backend_counted can decode them without the host ever seeing a count.  Formats, trigger
 * arguments, rules 1, 2, 4 and 5, `final`, the OFS_EINVAL conditions, the state layout and
 * ofs_frame_capture_state_bytes are those of the slot form: after the same pushes the state bytes of the
 * two are equal, and one stream may alternate between them.  Only where frames are written differs:
 *   cap         capacity in rows, 1 .. 2^31 - 1 (anything else: OFS_EINVAL).
 *   frames      [cap][n_br][F] samples in in_fmt, aligned to one sample.
 *   frame_start [cap] int64, frame_stream [cap] int32, row0 [B] int32, n_rows [2] int32,
 *   n_frames    [B] int32, dropped [B][3] int32 (as above).
 * n_frames[b] = the frames of stream b that left the queue in this call (rule 2); row0[b] = the exclusive
 * prefix sum of n_frames over b (exact in 64 bits, stored clamped to 2^31 - 1).  The frame of stream b in
 * slot j belongs to row r = row0[b] + j: rows are in (stream, slot) order.  r < cap: the samples are
 * written to frames[r], frame_start[r] = s, frame_stream[r] = b.  r >= cap: the frame is LOST - it has
 * left the queue and is not retried.  n_rows[0] = min(total, cap), n_rows[1] = max(total - cap, 0) (lost;
 * clamped to 2^31 - 1).  Every call writes n_rows, row0, n_frames, dropped, and -1 into frame_start[r] and
 * frame_stream[r] for n_rows[0] <= r < cap; the sample words of those rows are left untouched.
 * A null output with B > 0 is OFS_EINVAL.  B = 0 is a valid no-op that still writes n_rows = {0, 0} and
 * the -1 fill where those pointers are given.
 * Four kernels per call, stream-ordered, no host synchronisation: a thread per stream counts its frames,
 * one workgroup scans the counts (deterministic; no workgroup waits on another), then the slot form's
 * gather and update with the row as destination.
 */
int32_t ofs_frame_capture_compact(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t Tc,
                                  int32_t frame_len, int32_t history, int32_t max_pending, int64_t offset,
                                  const int64_t* trig, int64_t trig_ld, int64_t trig_stride,
                                  const int32_t* n_trig, int32_t trig_max, void* state, int64_t cap,
                                  void* frames, int64_t* frame_start, int32_t* frame_stream, int32_t* row0,
                                  int32_t* n_rows, int32_t* n_frames, int32_t* dropped, int32_t final,
                                  void* stream);

/* ---- detection post-processing (metric streams -> timing decisions) -------------------------
 * Metrics are [B][n] device arrays; `precision` names their element type (OFS_FP32 = float,
 * OFS_FP64 = double).  Smoothed outputs are f64.  Per-stream `status` reports what the
 * reference would do: >= 0 ok (for ofs_plateau_end the branch taken), < 0 it raises ValueError.
 *
 * Non-finite samples are decided as numpy decides them.  Every argmax is np.argmax: NaN is the
 * maximum, the first index wins among equals (NaNs included), and -inf is a value like any other,
 * so an all-NaN or all -inf stream answers index 0 and no index is ever out of [0, n).  Where the
 * reference takes np.max, a NaN maximum makes `max > 0`, `max <= 0` and every comparison with a
 * level derived from it false, and the reference's branch for that is taken.  The sign bit and
 * payload of a NaN output are not specified.
 */

/* minn._trailing_average / combined_sc_min._trailing_average (minn.py:115-128,
 * combined_sc_min.py:167-180) of max(x, 0) when clip_negative != 0 (minn.py:149), else of x:
 * the reference's float64 running-sum recursion, sample by sample.  out: [B][n] f64.
 * np.maximum keeps NaN and turns -inf into 0; a NaN, or a +inf once it leaves the window
 * (inf - inf), makes every later output NaN, as in the reference.  No status: never raises. */
int32_t ofs_trailing_average(int32_t precision, const void* x, int64_t B, int64_t n, int32_t win,
                             int32_t clip_negative, double* out, void* stream);

/* sc.find_plateau_end_from_metric (sc.py:81-146).  lookahead < 0 means None.  Ms: [B][max(n, w)]
 * f64 (numpy "same" convolution length); plateau_end: [B] int64; status: [B] int32 = branch
 * (1 drop below 95 %, 2 earliest long run above 60 %, 3 slope fallback, 4 fallback on an empty
 * window, 0 empty metric), -3 where numpy's broadcast would raise (plateau_end is -1 then).
 * A NaN in Ms (a NaN sample, or +inf and -inf in one window): the centre is the first NaN, the
 * 95 % and 60 % tests fail, and the slope fallback's argmax takes the first NaN drop (branch 3 or
 * 4, or -3).  +inf without NaN is its own 95 % level (branch 1 at the centre when cp_len > 1 and
 * the centre is not last); all -inf likewise answers index 0, branch 1. */
int32_t ofs_plateau_end(int32_t precision, const void* M, int64_t B, int64_t n, int32_t cp_len,
                        int32_t lookahead, int32_t smooth_win, double* Ms, int64_t* plateau_end,
                        int32_t* status, void* stream);

/* minn.find_minn_peak (minn.py:131-205) on the trailing average Ms (ofs_trailing_average):
 * gate = longest run of Ms >= gate_threshold * max(Ms) (earliest on ties) cut to
 * [bound_lo, bound_hi) (0, n for no bounds); empty gate -> global argmax.  peak, gate_lo,
 * gate_hi: [B] int64 (gate_* nullable); status 0 ok, -1 empty metric (n == 0), -2 no positive
 * peak (max(Ms) <= 0; peak is -1 and the gate 0, 0 for both).  A NaN in Ms is the maximum: it is
 * neither <= 0 nor reached by any sample, so the gate is empty and peak = the first NaN, gate
 * [peak, peak + 1), status 0.  +inf is an ordinary maximum (level = threshold * inf). */
int32_t ofs_minn_peak(const double* Ms, int64_t B, int64_t n, double gate_threshold, int64_t bound_lo,
                      int64_t bound_hi, int64_t* peak, int64_t* gate_lo, int64_t* gate_hi, int32_t* status,
                      void* stream);

/* The S&C gate of combined_sc_min.run_simulation (combined_sc_min.py:337-358):
 * mask = M_sc / max >= threshold (max > 0) else M_sc >= threshold, seeded with the argmax when
 * empty.  mask: [B][n] uint8 (nullable); span: [B][2] int64 = first, last + 1 (nullable).
 * No status: n == 0 writes span 0, 0.  A NaN sample makes the maximum NaN, so the comparison is the
 * unnormalised one and NaN samples fail it; if nothing passes, the seed is the first NaN.  All
 * -inf (or all NaN) gives the seed at index 0, span 0, 1.  With max = +inf, M_sc / max is 0 for
 * finite samples and NaN (fails) for the +inf ones. */
int32_t ofs_sc_gate(int32_t precision, const void* M_sc, int64_t B, int64_t n, double threshold,
                    uint8_t* mask, int64_t* span, void* stream);

/* combined_sc_min._streaming_peak_detector (combined_sc_min.py:183-209) as used by
 * combined_sc_min.find_minn_peak (:212-259): first argmax (strict >) of Ms over the FIRST run of
 * mask within [bound_lo, bound_hi).  peak: [B] int64; status 0 ok (n == 0: peak 0), -1 empty
 * gate region (peak -1).  This is the reference's loop, not np.argmax: the run's first sample seeds
 * the best value and only a strictly larger sample replaces it.  A run that starts with NaN
 * answers its start; a NaN later in the run is skipped; a run of -inf answers its start. */
int32_t ofs_segment_peak(const double* Ms, const uint8_t* mask, int64_t B, int64_t n, int64_t bound_lo,
                         int64_t bound_hi, int64_t* peak, int32_t* status, void* stream);


/* ------------------------------------------------------------------------------------------
 * The receiver back-end helpers one by one (the reference drivers call them individually,
 * sc.py:274-311), batched over rows, device pointers, c128 = interleaved (re, im) doubles.
 * Row operands ("ref", "den") take a row stride in elements (0 = one row shared by all).
 * ------------------------------------------------------------------------------------------ */

/* core.ofdm_fft_used (core.py:171-176): out[b][u] = fftshift(fft(x[b], n=n_fft))[(n_fft/2 +
 * bins[u]) % n_fft] = DFT_n_fft of x[b][0 : min(T, n_fft)] zero-padded, at bin bins[u] mod n_fft
 * (numpy's fft(x, n) truncates or zero-pads).  x [B][T] c64/c128/int16 I/Q; bins [n_used] int32
 * (device); out c128 [B][n_used]; n_fft a power of two <= 4096.  fp64 radix-2 FFT in LDS. */
int32_t ofs_fft_used(int32_t in_fmt, const void* x, int64_t B, int64_t T, int32_t n_fft, int32_t n_used,
                     const int32_t* bins, void* out, void* stream);

/* core.ls_channel_estimate (core.py:339-341) and core.equalize (:344-345): out = num / (den + eps)
 * with numpy's complex128 division (Smith's algorithm with the reciprocal scale, no contraction:
 * bit-identical to numpy).  num, out [B][n] c128; den [.][n] c128 with row stride den_stride. */
int32_t ofs_cdiv_eps(const void* num, int64_t B, int64_t n, const void* den, int64_t den_stride, double eps,
                     void* out, void* stream);

/* core.remove_common_phase (core.py:348-354): cpe = angle(mean(x)) when ref is NULL, else
 * angle(vdot(ref, x) / (vdot(ref, ref) + 1e-12)); out = x * exp(-i cpe).  x [B][n] c128;
 * ref [.][n] c128 (ref_stride) or NULL; cpe [B] f64; out [B][n] c128 (nullable). */
int32_t ofs_common_phase(const void* x, int64_t B, int64_t n, const void* ref, int64_t ref_stride, void* out,
                         double* cpe, void* stream);

/* core.align_complex_gain (core.py:357-362): g = vdot(x, ref) / (vdot(x, x) + eps); out = x * g.
 * gain [B] c128; out [B][n] c128 (nullable). */
int32_t ofs_align_gain(const void* x, int64_t B, int64_t n, const void* ref, int64_t ref_stride, double eps,
                       void* out, void* gain, void* stream);

/* core.evm_rms_db (core.py:365-370): evm = sqrt(mean|x - ref|^2 / mean|ref|^2),
 * evm_db = 20 log10(evm + 1e-12).  evm, evm_db [B] f64 (each nullable). */
int32_t ofs_evm(const void* x, int64_t B, int64_t n, const void* ref, int64_t ref_stride, double* evm,
                double* evm_db, void* stream);

/* core.estimate_timing_offset_from_phase_slope (core.py:443-469): phi = unwrap(angle(h)) (numpy's
 * unwrap rule), slope = Σ (k - k̄)(phi - phī) / (Σ (k - k̄)² + 1e-12) over the abscissa bins[u]
 * (centred subcarrier indices), sto = -slope * n_fft / (2 pi).  h [B][n_used] c128; slope, sto
 * [B] f64 (each nullable). */
int32_t ofs_phase_slope(const void* h, int64_t B, int32_t n_used, const int32_t* bins, int32_t n_fft,
                        double* slope, double* sto, void* stream);

/* core.apply_cfo (core.py:123-138): out[b][br][n] = x[b][br][n] * exp(i phi_n), phi_n =
 * ((2 pi cfo_b) n) * (1 / fs) - the reference's operation order (its complex scalar arithmetic
 * reduces to these two products); one tone per stream, shared by its branches.  x [B][n_br][T]
 * c64/c128/int16 I/Q; cfo_hz [B] f64 (device); out c128 [B][n_br][T]. */
int32_t ofs_apply_cfo(int32_t in_fmt, const void* x, int64_t B, int32_t n_br, int64_t T, const double* cfo_hz,
                      double fs_hz, void* out, void* stream);

/* sync_aa.quantize_adc (sync_aa.py:263-291): per component v -> round(clip(v / fs, -1, 1 - 1/L) * L)
 * / L * fs, L = 2^(bits-1), round half to even (np.round).  precision OFS_FP32: complex64 in and
 * out, every operation in fp32 (numpy 2 keeps float32 when full_scale is a Python float);
 * OFS_FP64: c64 or c128 in, c128 out (a float64 full_scale promotes).  Bit-identical to numpy. */
int32_t ofs_quantize_adc(int32_t in_fmt, const void* x, int64_t n, double full_scale, int32_t bits,
                         int32_t precision, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OFDMSYNC_H */
