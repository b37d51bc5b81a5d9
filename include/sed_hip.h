/* libsed_hip.so -- C ABI of the MI355X-native MAT-SED hot path (gfx950).
 *
 * The reference (cai525/Transformer4SED) is pure PyTorch and has no FFI of its own; the seam is the set of
 * Python call contracts of SURVEY.md section 8(b).  This header is the native boundary behind those contracts:
 * every entry point takes raw DEVICE pointers, sizes and a hipStream_t, never allocates or frees caller-visible
 * memory, keeps no static state, is stream-ordered and re-entrant, and returns 0 or a negative error code
 * (-1 bad argument, -2 HIP launch failure, -(1000 + hipError_t) for a failed launch with the HIP error code) which the Python binding
 * (transformer4sed_amd/_lib.py) turns into RuntimeError.  Each entry cites the reference code it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions: f32 = float, 16-bit operands = raw uint16 bit patterns (void*): bf16, or IEEE half where an `f16` flag is
 * set (forward activations/weights; gradient-side operands are always bf16), row-major, "D" = 768 channels,
 * H = 12 heads x 64.  Sequence-padded buffers ("pad") must be zero-initialised once by the caller.
 */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

/* ABI version.  Bumped whenever an EXISTING entry point changes its argument list (new entry points alone do not bump it; a changed
 * one normally gets a new suffixed name instead, like sed_median_filter_k).  History: 3 = round 3 (sed_relpos_attn_fwd gained O_split,
 * sed_relpos_attn_bwd gained Pst, both in place); 4 = round 4.  A binding compares sed_abi_version() with the header it was written
 * against before the first call (transformer4sed_amd/_lib.py does). */
#define SED_HIP_ABI_VERSION 7

#ifdef __cplusplus
extern "C" {
#endif

int sed_abi_version(int reserved);

/* ------------------------------------------------------------------ frontend / augment / post-process */
/* PasstFeatureExtractor.forward + .normalize (src/models/passt/passt_feature_extraction.py:46-94).
 * wav [B,L] f32 -> out [B,128,T] f32; window [800] symmetric Hann, twiddle [1024] float2 exp(-2 pi i k/1024),
 * melw [128,513] dense Kaldi bank (host-built per (fmin,fmax)), mel_range [128,2] non-zero bin range.  maxbits_tmp: scratch of 32 B words
 * (32 partial |max| values per clip).  do_log bit 0: (log(mel + 1e-5) + 4.5) / 5; bit 1 (test aid): the round-5 kernel. */
int sed_logmel_fwd(const float* wav, float* out, uint32_t* maxbits_tmp, const float* window, const float* twiddle,
                   const float* melw, const int* mel_range, int B, int L, int T, int do_log, hipStream_t stream);
/* Polyphase FIR resampler, the device counterpart of the offline tool src/utils/resample.py:10-14 (16 kHz -> 32 kHz): x [B,L] ->
 * y [B,Lout], taps h [ntaps] and alignment (n_pre_pad, n_pre_remove) as scipy.signal.resample_poly defines them (host-built). */
int sed_resample_poly(const float* x, float* y, const float* h, int B, int L, int Lout, int up, int down, int ntaps,
                      int n_pre_pad, int n_pre_remove, hipStream_t stream);
/* The same resampler on 16-bit PCM file bodies (round 5, the batched input pipeline data.WavBatchStream -- replaces the per-file
 * librosa.load + resample of src/preprocess/feats_extraction.py:7-12 / src/utils/resample.py:10-14): x [B,L] int16 zero padded,
 * lens [B] real sample counts; int16 -> fp32 by 2^-15 inside; y [B,Lout] with zeros from ceil(lens[b] up / down) on (pad_wav). */
int sed_resample_poly_pcm16(const int16_t* x, const int* lens, float* y, const float* h, int B, int L, int Lout, int up, int down,
                            int ntaps, int n_pre_pad, int n_pre_remove, hipStream_t stream);
/* frame_shift + mixup (src/preprocess/data_aug.py:11-28, 75-90); shift [B], perm [B] / cmix [B,2]={c,1-c} nullable */
int sed_roll_mix(const float* in, float* out, const int* shift, const int* perm, const float* cmix, int B, int F, int T,
                 int clamp01, hipStream_t stream);
/* freq_nonlinear (gather-lerp table) + filt_aug additive term (data_aug.py:150-192, 207-222) */
int sed_warp_filt(const float* in, float* out, const int* kidx, const float* lam, const float* add, int B, int F, int T,
                  hipStream_t stream);
/* In-place box fill x[:, f0:f1, t0:t1] = value on x [B,F,T]: time_mask (src/preprocess/data_aug.py:93-108: features 0 / 1e-4 and labels 0
 * over a time range) and torchaudio's FrequencyMasking as called at data_aug.py:136-140 (a frequency range, all clips, value 0).  An empty
 * range is a no-op (python slice semantics are resolved by the caller). */
int sed_mask_box(float* x, int B, int F, int T, int f0, int f1, int t0, int t1, float value, hipStream_t stream);
/* add_noise (data_aug.py:195-204): out[b] = x[b] + noise[b] * std(x[b]) / snr_lin[b], std unbiased over the n = F*T elements of a clip
 * (torch.std over dims (1,2)), snr_lin = 10^(snr_dB/20); noise = the caller's standard-normal draws.  part: scratch fp32 [B, 64, 3]. */
int sed_add_noise(const float* x, const float* noise, const float* snr_lin, float* part, float* out, int B, int n,
                  hipStream_t stream);
/* median_filter_torch (src/postprocess/filter.py:4-36, mode 0); scipy median / max filter as called at
 * src/codec/decoder.py:91,94 (modes 1, 2); optional per-(clip,class) weak-mask multiplier (decoder.py:22-23,80) */
int sed_median_filter(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C, int mode,
                      hipStream_t stream);
/* the same filters with the caller's bound `max_size` on the window sizes (which live on the device): with it, windows of 24 frames and more
 * (the evaluation path filters with 32 / 128 frames, recipes/desed/finetune/train.py:221-227) take an order-statistics kernel -- global
 * ranks of the padded column once, windows as bitmaps over ranks -- instead of the O(k^2) rank search; same element selected, bit-exact.
 * In that kernel a window larger than max_size comes out as a NaN plane for its (clip, class).  csrc/median_filter.hip. */
int sed_median_filter_k(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C, int mode,
                        int max_size, hipStream_t stream);
/* Multilabel average precision, torchmetrics 0.11 MultilabelAveragePrecision with thresholds=None (the AudioSet-Strong validation metric,
 * recipes/audioset_strong/base/passt_cnn/train.py:239-314 and the two detect_any_sound loops; csrc/metrics.hip).  Storage: scores [C][cap]
 * f32 and labels [C][cap] uint8, class-major, caller-owned.
 * sed_ap_append: preds / target [B,C] f32 (target 0 / 1) -> clips n0 .. n0+B-1.  If any score of the batch lies outside [0, 1] (or is NaN)
 * the whole batch is stored as sigmoid(preds); that decision is taken on the device (flags: 64 ints of scratch).  status[0] |= 2 for a NaN
 * score, 4 for a target outside {0, 1} (the caller zeroes it once and reads it when it computes).
 * sed_ap_grow: copies clips 0 .. n-1 of every class into a larger storage (device to device).
 * sed_ap_compute: ap[C] (double; NaN for a class without a positive) and npos[C] over clips 0 .. N-1.  chunk (1 .. 20000): clips per
 * LDS sort; N <= chunk runs in one launch from LDS, otherwise all_sorted / pos_sorted (uint32 [C][ceil(N/chunk) chunk] each) hold the
 * sorted chunks.  pos_cnt (int) and partial (uint64) [C][ceil(N/chunk)] are scratch.  The result does not depend on clip order or chunk. */
int sed_ap_append(const float* preds, const float* target, int B, int C, int n0, int cap, int* flags, int* status, float* scores,
                  uint8_t* labels, hipStream_t stream);
int sed_ap_grow(const float* old_scores, const uint8_t* old_labels, int C, int n, int old_cap, float* new_scores, uint8_t* new_labels,
                int new_cap, hipStream_t stream);
int sed_ap_compute(const float* scores, const uint8_t* labels, int C, int N, int cap, int chunk, uint32_t* all_sorted, uint32_t* pos_sorted,
                   int* pos_cnt, unsigned long long* partial, double* ap, int* npos, hipStream_t stream);
/* ROC area and partial ROC area from the same storage (csrc/metrics.hip; DESIGN.md section 7g holds the definition): the AUC / d' that
 * AudioSet systems report beside the mAP, and the per-class integers of the segment-based mpAUC that src/utils/validate_submissions.py:111
 * asks for on MAESTRO.  out: int64 [C][SED_ROC_OUT] = P, Nn, auc2, area2, fp_a, tp_a, fp_b, tp_b over items 0 .. N-1, where point a is
 * the last ROC point with fp <= floor(max_fpr Nn) (max_fpr in (0, 1]) and b the next one; the caller finishes in float64.  chunk
 * (1 .. SED_ROC_MAX_CHUNK) and all_sorted / pos_sorted / pos_cnt as for sed_ap_compute; scratch: uint64 [C (2 ceil(N/chunk) + 1)].  With
 * N <= chunk only scores, labels and out are touched.  The result does not depend on item order or chunk. */
#define SED_ROC_OUT 8
#define SED_ROC_MAX_CHUNK 20000
int sed_roc_compute(const float* scores, const uint8_t* labels, int C, int N, int cap, int chunk, double max_fpr, uint32_t* all_sorted,
                    uint32_t* pos_sorted, int* pos_cnt, unsigned long long* scratch, long long* out, hipStream_t stream);
/* Segment scores from frame scores on the device (csrc/segment_pool.hip): get_segment_scores and
 * get_segment_scores_and_overlap_add of src/codec/decoder.py:138-230.
 * sed_segment_pool: scores [n,T,C] f32, ts_us [T+1] frame boundaries in microseconds (not decreasing), per clip its length clip_len_us
 * and the row row_off of its first segment in pooled [cap_rows][C] f32; clip i fills ceil(clip_len_us[i] / seg_us) <= max_seg rows with
 * the duration-weighted means of its frames.
 * sed_segment_gather: file segment s of S averages the pooled rows rows[ptr[s] .. ptr[s+1]) (CSR, at most max_rows each, nnz in all,
 * each below n_rows) in the order given; out [C][ld] f32 class-major (ld >= S), 0 for a segment without a row.
 * status: int [SED_SEG_STATUS_WORDS], sticky, zeroed once by the caller; a word is set to 1 for: a segment without weight, a NaN
 * score, a row outside the storage, a row list longer than max_rows. */
#define SED_SEG_STATUS_WORDS 4
#define SED_SEG_ZERO_WEIGHT 0
#define SED_SEG_NAN 1
#define SED_SEG_BAD_ROW 2
#define SED_SEG_LONG_LIST 3
int sed_segment_pool(const float* scores, const int64_t* ts_us, const int64_t* clip_len_us, const int* row_off, int64_t seg_us, int n,
                     int T, int C, int max_seg, int cap_rows, float* pooled, int* status, hipStream_t stream);
int sed_segment_gather(const float* pooled, const int* ptr, const int* rows, int S, int C, int n_rows, int nnz, int max_rows, int ld,
                       float* out, int* status, hipStream_t stream);
/* Intersection-based PSDS (Bilen et al. 2020, over all score values as in Ebbers et al. 2022): what src/evaluation_measures.py:299-341
 * `compute_psds_from_scores` gets from sed_scores_eval, and the objective metric of recipes/desed/finetune/train.py:229-253, 370-398
 * (csrc/psds.hip; DESIGN.md section 7b holds the definition).
 * sed_psds_sweep: scores [B,T,C] f32, post-processed frame scores.  For every (clip, class) the threshold events in descending score
 * order into slots [B][C][T]: ev_val (score value), ev_dtp / ev_dfp (int16 change of the clip's TP / FP count of that class once the
 * threshold passes below the value), ev_dct (int64 change of sum_k CT_k ct_q[k]); slots past the clip's distinct values are zero events.
 * clip_id [B]: row of each clip in the ground truth, gt_ptr [n_clips + 1] CSR into gt_cls / gt_on / gt_off (microseconds), a clip's
 * events sorted by class, at most 256 of them.  ts_us [T + 1]: frame boundaries in microseconds; frames t < min(t_pos, n_frames[b])
 * take part (t_pos: leading frames of positive duration; n_frames may be NULL).  dtc, gtc in (0, 1].  ct_q [C] with ev_dct, or both
 * NULL for no cross-trigger threshold (then cttc is ignored); with them C <= 32 and cttc in (0, 1].  T <= 1024.  status[0] |= 2 for a
 * NaN score, 8 for a clip with too many events (the caller zeroes it once). */
int sed_psds_sweep(const float* scores, const int* clip_id, const int* n_frames, const int64_t* ts_us, int t_pos, const int* gt_ptr,
                   const int* gt_cls, const int64_t* gt_on, const int64_t* gt_off, const int64_t* ct_q, double dtc, double gtc,
                   double cttc, int B, int T, int C, float* ev_val, int16_t* ev_dtp, int16_t* ev_dfp, int64_t* ev_dct, int* status,
                   hipStream_t stream);
/* Event-based (collar) and segment-based F1 counts: what src/evaluation_measures.py:52-152 (`event_based_evaluation_df`,
 * `segment_based_evaluation_df`) and 256-295 (`log_sedeval_metrics`) get from sed_eval on the event lists of src/codec/decoder.py:15-35,
 * logged by recipes/desed/finetune/train.py:370-398, 481-517 (csrc/event_f1.hip; DESIGN.md section 7c holds the definition).
 * sed_event_f1_counts: one wave per (clip, class) adds n_ref, n_sys, tp, seg_tp, seg_fp, seg_fn to counts [C][6] (int64, the caller
 * zeroes it once).  Estimated events, frame form: active [B,T,C] bytes, non-zero = on; the maximal runs a..b of every class span
 * ts_us[a] .. ts_us[b + 1] (ts_us [T + 1], microseconds; T <= 1024).  List form (active NULL, T and ts_us ignored): est_ptr [B + 1] CSR
 * into est_cls / est_on / est_off, a clip's events sorted by class and onset, disjoint within a class, at most 512 per clip and class.
 * clip_id [B]: row of each clip in the ground truth, gt_ptr [n_clips + 1] CSR into gt_cls / gt_on / gt_off (microseconds), a clip's
 * events sorted by class, at most 256 of them.  tp: maximum matching of the hits |ron - eon| <= collar_us and
 * (double)|roff - eoff| <= max((double)collar_us, p * (double)(roff - ron)).  Segments of res_us, at most 64 per clip.  status[0] |= 1
 * if the estimates a reference event hits are not one index interval, 4 / 8 / 16 for too many estimates / events / segments (the caller
 * zeroes it once). */
int sed_event_f1_counts(const uint8_t* active, const int* est_ptr, const int* est_cls, const int64_t* est_on, const int64_t* est_off,
                        const int* clip_id, const int64_t* ts_us, const int* gt_ptr, const int* gt_cls, const int64_t* gt_on,
                        const int64_t* gt_off, int64_t collar_us, double p, int64_t res_us, int B, int T, int C, int64_t* counts,
                        int* status, hipStream_t stream);

/* ------------------------------------------------------------------ GEMM family (nn.Linear / conv / autograd GEMMs) */
/* C[M,N] = A[M,K] . B[N,K]^T, bf16 operands, fp32 accumulate, fused epilogue `epi`:
 * 0 outF=acc*alpha+bias | 1 outF=resF+acc+bias (resF may alias outF) | 2 outH=bf16(acc+bias) | 3 outH=h, outH2=gelu(h) | 4 outH=acc*gelu'(auxH)
 * `f16`: 0 = bf16 operands / outputs, 1 = IEEE half, 3 = half, but tensors only the bf16 backward consumes are written as bf16
 *        (epi 3 / 8: the pre-activation outH;  sed_gemm_qkv: row-major v, qt, kt, q2t).
 * 5 atomicAdd(outF, acc*alpha) (split-K; `ksplit` is a hint, the library re-derives it for the tile shape it dispatches) | 7 outF and outH | 8 outH=h, outF=gelu(h) fp32.  Replaces F.linear at src/models/passt/passt.py:271,274,
 * 332,342; src/models/transformer/transformerXL.py:382,493,584; src/models/passt/passt_sed.py:196; conv2d passt.py:307 */
int sed_gemm_nt(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi, const float* bias,
                const float* resF, float* outF, void* outH, void* outH2, const void* auxH, int ldc, float alpha,
                int ksplit, int f16, hipStream_t stream);
/* sed_gemm_qkv (all its outputs) on two of the three split-precision terms: A plain f16 [M, K], Wsplit the split weight image [N, 3K] =
 * [hi | hi | lo]; result A . (hi + lo)^T.  The context network's in_proj (src/models/transformer/transformerXL.py:382-384), whose output is
 * insensitive to the activation's lo part (tools/err_sim.py).  256 x 256 kernel: M >= 1024. */
int sed_gemm_qkv_w2s(const void* A, const void* Wsplit, const float* bias, int M, int K, int heads, int seq, int seq_pad, void* q,
                     void* k, void* v, void* qt, void* kt, void* vt, void* q2, void* q2t, const float* pos_u, const float* pos_v,
                     int f16, hipStream_t stream);
/* Number of CUs the persistent GEMM kernels (256 x 256 tiles: every forward / dX GEMM; the TN weight-gradient kernel's split count)
 * size their grids for; 0 = all (default; the environment variable SED_GEMM_CUS is read when nothing was set).  The one process-wide
 * setting of the library: a data-parallel job whose RCCL kernels run beside the backward leaves their CUs out (ddp.py).  The persistent
 * kernels walk their tiles dynamically (per-XCD counters), so a workgroup that starts late only shortens the others' share. */
int sed_gemm_set_cu_budget(int n_cus);
/* Measurement aid: n_cus single-wave workgroups (one per CU) that idle for `usec` microseconds on `stream` -- the stand-in for
 * communication kernels in tools/cu_steal.py (profiles/r4_cu_steal.txt).  Not used by the product path. */
int sed_debug_hold_cus(int n_cus, int usec, hipStream_t stream);
/* Test aid: synchronises the device and returns the number of non-zero words in the dynamic-walk counter ring (0 when idle). */
int sed_debug_tile_counters_dirty(int reserved);
/* sed_gemm_nt / sed_gemm_qkv with a ROW-GROUP bias: row m additionally gets gbias[(m / gb_rows) * N + n] (fp32 [M / gb_rows, N]; gb_rows =
 * tokens per clip >= 128, M % gb_rows == 0; epilogues 0-3, 7, 8).  Carries the weight-rounding correction of the evaluation-mode encoder:
 * mean_t(x) . (W - f16(W))^T per clip, added to the F.linear results of src/models/passt/passt.py:332,342 and timm Mlp fc1 / fc2
 * (same reference lines as sed_gemm_nt) so that frame posteriors stay inside BASELINE.json's 1e-3 at the validation temperature. */
int sed_gemm_nt_gb(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi, const float* bias,
                   const float* resF, float* outF, void* outH, void* outH2, const void* auxH, int ldc, float alpha, int f16,
                   const float* gbias, int gb_rows, hipStream_t stream);
int sed_gemm_qkv_gb(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq, int seq_pad, void* q,
                    void* k, void* v, int f16, const float* gbias, int gb_rows, hipStream_t stream);
/* The same F.linear calls with TWO-TERM weights (evaluation-mode encoder, default): A [M, K] f16 against B [N, 2K] =
 * [f16(W) | f16(W - f16(W))] (sed_split3_f16 mode 2); the A panel is walked twice, so the result carries the fp32 weight to ~2^-19 at the
 * cost of twice the MFMA work.  256^2 kernel only: N % 256 == 0, M >= 1024, f16; epi 1 (fp32 + residual) or 3 (GELU, outH nullable). */
int sed_gemm_nt_w2(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi, const float* bias,
                   const float* resF, float* outF, void* outH, void* outH2, int ldc, int f16, hipStream_t stream);
int sed_gemm_qkv_w2(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq, int seq_pad, void* q,
                    void* k, void* v, int f16, hipStream_t stream);
/* ... with the lo product x . (W - f16(W))^T on the fp8 matrix path (v_mfma_scale_f32_16x16x128_f8f6f4): half of an f16 K pass for a
 * term that is 2^-12 of the result and needs ~4 significant bits of either factor.  Operand rows carry both images: A [M][K f16 | K e4m3]
 * (row pitch lda halfs >= 3K / 2; the e4m3 half = 2^-2 x the activation: sed_fp8_tail, or the producing kernels' fp8 flags), B [N][K f16 |
 * K e4m3] = sed_weight_two_term_f8(W, s) with f8_exp = s.  K % 128 == 0; otherwise like sed_gemm_nt_w2 / sed_gemm_qkv_w2. */
int sed_gemm_nt_w2f8(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi, const float* bias,
                     const float* resF, float* outF, void* outH, void* outH2, int ldc, int out_e4m3, int f8_exp, hipStream_t stream);
/* (out_e4m3 != 0, epi 3 with outH NULL: outH2 rows are [N f16 | N e4m3], ldc >= 3N / 2 -- the fc1 activation leaves as fc2's A operand) */
int sed_gemm_qkv_w2f8(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq, int seq_pad, void* q,
                      void* k, void* v, int f8_exp, hipStream_t stream);
/* sed_gemm_nt_gb with epi 3 (fused GELU, outH NULL) whose result leaves as rows [N f16 | N e4m3] (ldc >= 3N / 2): fc1 of the evaluation-mode
 * encoder on f16 weights + the per-clip mean correction, writing fc2's two-image A operand.  N % 256 == 0, M >= 1024, f16. */
int sed_gemm_nt_gb_e4m3(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias, void* outH2, int ldc,
                        const float* gbias, int gb_rows, hipStream_t stream);
/* x rows [K f16 | K e4m3] of pitch ld halfs: fills the e4m3 half (OCP e4m3, round to nearest even, clamped to +-448) with 2^-2 x the f16 half */
int sed_fp8_tail(void* x, int M, int K, int ld, hipStream_t stream);
/* fp32 weight [N, K] -> out rows [f16(W) | e4m3(2^s (W - f16(W)))], 3K bytes each */
int sed_weight_two_term_f8(const float* w, void* out, int64_t N, int K, int s, hipStream_t stream);
/* LayerNorm FOLDED into the two Linear layers around it -- timm Block.forward `x = x + attn(norm1(x))`, `x = x + mlp(norm2(x))`
 * (src/models/passt/passt.py:360-363 with the F.linear calls of :332,342 and Mlp fc1 / fc2) for no-grad f16 passes (teacher, inference), so
 * that the normalised tensor never exists in memory:
 *   sed_gemm_nt_lnp   the residual Linear (proj / fc2): outF = residual + A . B^T + bias (fp32, may alias resF) AND x16 = its f16 image AND
 *                     rowpart [M][N / 64][2] = per-row (sum, sum of squares) of every 64-column slice
 *   sed_ln_fold_stats rowpart -> rowstat [M][2] = (mean, 1 / sqrt(var + eps)) over D = 64 S columns
 *   sed_ln_fold_weight W16 [N, K] = f16(gamma[k] W[n, k]), colS[n] = sum_k W16[n, k], colC[n] = sum_k beta[k] W[n, k] + bias[n]
 *   sed_gemm_nt_lnc / sed_gemm_qkv_lnc  the Linear AFTER the LayerNorm (fc1 + GELU; qkv with the head split), fed with x16 (the RAW
 *                     stream) and W16: out[m, n] = f(rstd[m] * (acc[m, n] - mean[m] * colS[n]) + colC[n])  ==  f(Linear(LayerNorm(x)))
 * 256^2 kernel only: N % 256 == 0, M >= 1024, K % 64 == 0, f16 operands. */
int sed_gemm_nt_lnp(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias, const float* resF,
                    const void* res_hi, const void* res_lo, float* outF, void* x16, void* out_lo, float* rowpart, int ldc,
                    hipStream_t stream);
/* (sed_gemm_nt_lnp, split-plane stream: between two folded blocks the residual stream can live as two f16 planes hi + lo instead of fp32
 *  -- res_hi / res_lo != NULL: the residual is read as hi + lo instead of resF; out_lo != NULL: the result is written as x16 (hi) + out_lo
 *  and outF is left alone.  The hi plane is the next GEMM's A operand, so a producer moves 8 instead of 10 bytes per element.) */
/* (sed_gemm_nt_lnp8: the same with the lo plane as BYTES -- res_lo8 / out_lo8 are M * ldc uint8 in slab-major order [ldc / 64][M][64]
 *  (a plane private to this entry point: written and read only here) and the stream value is
 *  hi * (1 + (q - 128) * 2^-18): the f16 rounding residual (at most |hi| 2^-11) in 256 steps, the stream to ~2^-19 relative.  A producer
 *  then moves 6 bytes per element.  Planes written by one entry point must be read by the same one.) */
int sed_gemm_nt_lnp8(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias, const float* resF,
                     const void* res_hi, const void* res_lo8, float* outF, void* x16, void* out_lo8, float* rowpart, int ldc,
                     hipStream_t stream);
/* (with sed_gemm_nt_lnp8 the hi plane -- res_hi in, x16 out -- is slab-major too, [ldc / 64][M][64] f16: a K tile of the consumer and a
 *  wave's patch of the producer are contiguous runs.  sed_gemm_nt_lnc8 / sed_gemm_qkv_lnc8 are the consumers that read it: same
 *  arguments as sed_gemm_nt_lnc / sed_gemm_qkv_lnc, lda = K.  sed_gemm_nt_lnc8 with ldc = 64 (N > 64) writes its output slab-major as
 *  well, [N / 64][M][64]; sed_gemm_nt_lnp8 with lda = 64 (K > 64) reads such an A operand: the fc1 activation of a folded block.) */
int sed_gemm_nt_lnc8(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* colC, const float* colS,
                     const float* rowstat, void* outH2, int ldc, hipStream_t stream);
int sed_gemm_qkv_lnc8(const void* A, const void* W, const float* colC, const float* colS, const float* rowstat, int M, int K, int heads,
                      int seq, int seq_pad, void* q, void* k, void* v, hipStream_t stream);
int sed_ln_fold_stats(const float* rowpart, float* rowstat, int M, int S, int D, float eps, hipStream_t stream);
int sed_ln_fold_weight(const float* W, const float* gamma, const float* beta, const float* bias, void* W16, float* colS, float* colC,
                       int N, int K, hipStream_t stream);
int sed_gemm_nt_lnc(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* colC, const float* colS,
                    const float* rowstat, void* outH2, int ldc, hipStream_t stream);
int sed_gemm_qkv_lnc(const void* A, const void* W, const float* colC, const float* colS, const float* rowstat, int M, int K, int heads,
                     int seq, int seq_pad, void* q, void* k, void* v, hipStream_t stream);
/* operands of that correction: per-clip token means of a 16-bit activation x [groups * rows, K] -> [groups, K] (K % 256 == 0; every
 * step-th token), and the f16 image of scale * (w - f16(w)) for an fp32 weight of n (multiple of 4) elements */
int sed_group_colmean(const void* x, void* out, int groups, int rows, int K, int step, int f16, hipStream_t stream);
/* ... over rows of pitch ld >= K elements (the f16 half of rows [K f16 | K e4m3]) */
int sed_group_colmean_ld(const void* x, void* out, int groups, int rows, int K, int ld, int step, int f16, hipStream_t stream);
int sed_weight_residual_f16(const float* w, void* out, int64_t n, float scale, hipStream_t stream);
/* sed_gemm_nt with a narrow result: A / B are padded to N (a multiple of 128, not of 256) but only the first ncols (multiple of 4)
 * output columns exist in memory -- bias [ncols], residual and outputs [M, ldc] with ldc >= ncols.  The 16/32/64-filter layers of
 * the PMAM CNN branch (src/models/cnn/base.py:62-70) produce their [pixels, filters] matrices this way. */
int sed_gemm_nt_cols(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi, const float* bias,
                     const float* resF, float* outF, void* outH, void* outH2, const void* auxH, int ldc, float alpha, int f16,
                     int ncols, hipStream_t stream);
/* Weight gradient in TN form: dW[M,N] (fp32, ldc) += dY[T,M]^T . X[T,N], both operands row-major [token][feature] as the forward /
 * backward left them (dY bf16, X bf16 or IEEE half) -- the autograd of F.linear's weight (same reference lines as sed_gemm_nt).
 * M % 64 == 0, N % 64 == 0, any T > 0 (256 x 256 tiles; a partly valid last tile computes on whatever lies behind its rows and stores
 * only its valid part; token rows past T read as zeros); split-K over tokens chosen by the library.  `workspace` (caller-owned, optional): with >= (256 / tiles) * M * N * 4
 * bytes (tiles = ceil(M/256) * ceil(N/256)) the splits are stored there and reduced by a second launch; otherwise atomics.
 * dbias (nullable): dbias[M] += column sums of dY over the T tokens, i.e. the bias gradient of the same linear, for free. */
int sed_gemm_dw_tn(const void* dY, const void* X, int x_f16, int T, int M, int N, int ldy, int ldx, float* dW, int ldc,
                   float* dbias, float* workspace, int64_t workspace_bytes, hipStream_t stream);
/* qkv / in_proj GEMM with head-split epilogue: q,k,v [B*H,seq,64] (each nullable), transposed copies [B*H,64,seq_pad] (nullable),
 * optional rel-pos biased queries q = q+u, q2 = q+v (passt.py:332-333; transformerXL.py:382-384,497-503) */
int sed_gemm_qkv(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq, int seq_pad, void* q,
                 void* k, void* v, void* qt, void* kt, void* vt, void* q2, void* q2t, const float* pos_u,
                 const float* pos_v, int f16, hipStream_t stream);
int sed_cast_f32_bf16(const float* in, void* out, int64_t n, int f16, hipStream_t stream);
int sed_f16_to_bf16_inplace(void* p, int64_t n, hipStream_t stream);
/* split-precision operand image: fp32 [M,K] -> f16 [M,3K]; mode 0 [hi|lo|hi] (activations), 1 [hi|hi|lo] (weights);
 * mode 2: f16 [M,2K] = [hi|lo], the two-term weight image of sed_gemm_nt_w2 / sed_gemm_qkv_w2 */
int sed_split3_f16(const float* in, void* out, int64_t M, int K, int mode, hipStream_t stream);
/* in [R,C] -> outT [C,Rpad] (zero padded; nullable), optional straight 16-bit copy and fp32 column sums (+=).
 * kinds: 0 bf16, 1 f32 (input only), 2 f16 */
int sed_transpose_to_bf16(const void* in, int in_kind, int R, int C, int ldin, void* outT, int Rpad, int outT_kind,
                          void* outS, int outS_kind, float* colsum, hipStream_t stream);
/* tiny fp32 linears (AT-head query / out_proj / 768->10 classifier; src/models/pooling.py:45-51, passt_sed.py:143) */
int sed_small_linear(const float* a, const float* w, const float* b, float* out, int M, int N, int K, int act,
                     hipStream_t stream);
int sed_small_linear_bwd(const float* a, const float* w, const float* out, const float* dout, float* da, float* dw,
                         float* db, int M, int N, int K, int act, hipStream_t stream);

/* ------------------------------------------------------------------ attention */
/* encoder MHSA (src/models/passt/passt.py:335-341), flash style; Q, K, V head-split [B*H, N, 64] 16-bit (V row-major: the kernel takes
   V^T out of its LDS tile with transposing reads); O [B,N,768] 16-bit, LSE [B*H,N] (log2 domain).
   f16: bit 0 = IEEE half operands (else bf16); bit 1 = O head-major [H][B*N][64] (the slab-major A operand of sed_gemm_nt_lnp8, lda = 64);
   bit 2 (with bit 0, without bit 1) = O rows [768 f16 | 768 e4m3], pitch 1152 halfs (the A operand of sed_gemm_nt_w2f8) */
int sed_mhsa_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int N, int Npad,
                 int f16, hipStream_t stream);
int sed_mhsa_bwd_prep(const void* dO, const void* O, float* Dtmp, void* dOh, void* dOt, int B, int H, int N, int Npad,
                      int o_f16, hipStream_t stream);
/* dqkv [B*N, 3*768] bf16 (dq | dk | dv).  f16 != 0: Q, K, O are IEEE half (as the f16 forward wrote them, used for the
 * score recompute), the gradient-side operand dO is bf16; V is bf16, or with v_f16 != 0 the IEEE half tensor the forward saved (its bf16
 * operand image is made inside the kernels).  Transposed operands are taken out of row-major LDS tiles with
 * transposing reads (no Q^T / K^T / dO^T copies); dO and O are read in their token-major [B, N, 768] layout and D = rowsum(dO * O)
 * is produced by the dQ kernel into Dtmp [B*H, N] -- no pre-pass; dOh is unused (may be NULL). */
int sed_mhsa_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, float* Dtmp,
                 void* dOh, void* dqkv, int B, int H, int N, int Npad, int f16, int v_f16, hipStream_t stream);
/* Transformer-XL rel-pos attention (src/models/transformer/transformerXL.py:493-576 incl. rel_shift 254-297).  O [B, T, H 64] 16-bit, or
 * fp32 with o_f32; O_split (nullable, fp32 mode only): the [hi | lo | hi] f16 split-precision image [B T, 3 H 64] of the same values --
 * out_proj's A operand (transformerXL.py:584), written here instead of by a sed_split3_f16 pass over O */
int sed_relpos_attn_fwd(const void* Qu, const void* Qv, const void* K, const void* Vt, const void* P, void* O, void* O_split,
                        float* LSE, int B, int H, int T, int Tpad, int Rpad, int f16, int o_f32, hipStream_t stream);
int sed_relpos_attn_bwd(const void* Qu, const void* Qut, const void* Qv, const void* Qvt, const void* K, const void* Kt,
                        const void* V, const void* P, const void* Pt, const void* O, const void* dO, const float* LSE,
                        float* Dtmp, void* dOh, void* dOt, void* dqkv, void* dSt, void* Pst, float* dP, float* du, float* dv, int B,
                        int H, int T, int Tpad, int Rpad, int need_param_grads, int f16, int o_kind, hipStream_t stream);
/* (dSt, Pst: [B H, Tpad, Tpad] bf16 scratch slabs, ZERO outside the region the kernels write -- rows = keys, columns = queries.  The dQ
 *  kernel stores dS^T there for the positional-table gradient and, when Pst is given, P^T as well: dK and dV are then two contractions
 *  over the stored slabs (a streaming kernel) instead of a second recomputation of the scores; Pst = NULL keeps the recomputing kernel.) */
/* Local-window forms (PaSST_SED(decoder_win_len=...): src/models/transformer/mask.py:7-23 diagonal_mask, applied per head by
 * src/models/transformer_decoder.py:96-119).  half_width: device int32 [H], hw[h] = window_len[h] / 2 (>= 1).  Query i of head h sees key j
 * iff max(0, i - hw) <= j < min(T, i + hw): hw keys to the left, the key itself, hw - 1 to the right -- the right edge is exclusive.
 * Masked scores are -inf before the softmax: their probability and gradient are exact zeros; LSE is the log-sum-exp over the allowed
 * keys.  hw >= T is the full window.  Every other argument, layout and result is that of the unbanded entry point; key (query) tiles
 * that no query (key) of a workgroup can see are skipped.  Slabs: the dQ kernel writes every slab tile it visits in full (zeros out of
 * band) and the other kernels read only those tiles, so tiles outside the band may hold anything (e.g. an earlier full-window call). */
int sed_relpos_attn_band_fwd(const void* Qu, const void* Qv, const void* K, const void* Vt, const void* P, void* O, void* O_split,
                             float* LSE, int B, int H, int T, int Tpad, int Rpad, int f16, int o_f32,
                             const int32_t* half_width /* device, [H] */, hipStream_t stream);
int sed_relpos_attn_band_bwd(const void* Qu, const void* Qut, const void* Qv, const void* Qvt, const void* K, const void* Kt,
                             const void* V, const void* P, const void* Pt, const void* O, const void* dO, const float* LSE,
                             float* Dtmp, void* dOh, void* dOt, void* dqkv, void* dSt, void* Pst, float* dP, float* du, float* dv, int B,
                             int H, int T, int Tpad, int Rpad, int need_param_grads, int f16, int o_kind,
                             const int32_t* half_width /* device, [H] */, hipStream_t stream);

/* ------------------------------------------------------------------ norms / glue / heads / optimiser */
/* nn.LayerNorm over D=768 (passt.py:361-362,580; passt_sed.py:128; timm Block norms); y = LN(in_scale*x).
 * f16: 0 bf16 / 1 IEEE-half y_bf16 [M, D]; 4: y_bf16 is the split-precision operand image [M, 3 D] = [hi | lo | hi] f16 of the result
 * (the context-network GEMMs' A operand, transformerXL.py:31-35 -- what sed_split3_f16 would make from y_f32 in a second pass);
 * 8: y_bf16 rows are [D f16 | D e4m3] (pitch 3 D / 2 halfs), the A operand of sed_gemm_nt_w2f8 / sed_gemm_qkv_w2f8 */
int sed_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, float in_scale, void* y_bf16,
                      float* y_f32, float* mean, float* rstd, int M, int D, int f16, hipStream_t stream);
/* ... with the result written twice, as IEEE half (y_f16: the forward GEMM's operand) and as bf16 (y_bf16: the saved operand of the backward's
 * weight-gradient GEMM, rounded once from fp32) */
int sed_layernorm_fwd_dual(const float* x, const float* gamma, const float* beta, float eps, float in_scale, void* y_f16, void* y_bf16,
                           float* mean, float* rstd, int M, int D, hipStream_t stream);
int sed_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                      float in_scale, float* dx, int accumulate, float* dgamma, float* dbeta, int M, int D,
                      hipStream_t stream);
/* the same backward, also writing dx16 [M, D] = bf16 image of the residual-stream gradient it leaves in dx: the dY operand of the
 * weight-gradient and dX GEMMs of the block below (autograd of timm Block.forward, passt.py:360-363) without a separate cast pass */
int sed_layernorm_bwd_x16(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                          float in_scale, float* dx, int accumulate, float* dgamma, float* dbeta, void* dx16, int M, int D,
                          hipStream_t stream);
/* patch embedding plumbing (passt.py:302-315, 503-569) */
int sed_im2col(const float* mel, void* cols, int B, int T, int tstart, int tp, int f16, hipStream_t stream);
int sed_assemble_tokens(const float* conv, const float* cls, const float* dist, const float* new_pos,
                        const float* freq_pe, const float* time_pe, int toffset, float* x, int B, int tp,
                        hipStream_t stream);
int sed_assemble_tokens_bwd(const float* dx, void* dconv, float* dcls, float* ddist, float* dnew_pos, float* dfreq,
                            float* dtime, int toffset, int B, int tp, hipStream_t stream);
/* PaSST_SED.f_pool 'mean_pool' (passt_sed.py:199-218) */
int sed_fpool_fwd(const float* x, const float* gamma, const float* beta, float eps, float* pooled, float* mean,
                  float* rstd, int B, int tp, hipStream_t stream);
int sed_fpool_bwd(const float* dpooled, const float* x, const float* mean, const float* rstd, const float* gamma,
                  float* dtok_tmp, float* dx_acc, float* dgamma, float* dbeta, int B, int tp, hipStream_t stream);
/* the five entry points above for a sequence that holds F (1..12) of the 12 frequency rows of the patch grid -- structured frequency
 * patchout, passt.py:533-547: N = 2 + F tp, cols / conv are [B F tp, .].  `rows`: DEVICE array of the F kept rows, strictly increasing
 * values in [0, 12) (validated by the caller), or NULL for 0..F-1; it selects the mel rows, the frequency embedding added to kept row
 * f' and the column of dfreq its gradient goes to (the other columns are not touched).  The entry points above are these with
 * rows = NULL, F = 12.  F outside 1..12 returns SED_ERR_ARG. */
int sed_im2col_rows(const float* mel, void* cols, const int* rows, int F, int B, int T, int tstart, int tp, int f16, hipStream_t stream);
int sed_assemble_tokens_rows(const float* conv, const float* cls, const float* dist, const float* new_pos, const float* freq_pe,
                             const float* time_pe, const int* rows, int F, int toffset, float* x, int B, int tp, hipStream_t stream);
int sed_assemble_tokens_rows_bwd(const float* dx, void* dconv, float* dcls, float* ddist, float* dnew_pos, float* dfreq, float* dtime,
                                 const int* rows, int F, int toffset, int B, int tp, hipStream_t stream);
int sed_fpool_rows_fwd(const float* x, const float* gamma, const float* beta, float eps, float* pooled, float* mean, float* rstd,
                       int B, int tp, int F, hipStream_t stream);
int sed_fpool_rows_bwd(const float* dpooled, const float* x, const float* mean, const float* rstd, const float* gamma, float* dtok_tmp,
                       float* dx_acc, float* dgamma, float* dbeta, int B, int tp, int F, hipStream_t stream);
/* InterpolateModule linear x ratio (+ replicated last frame) (passt_sed.py:13-34,258-259) */
int sed_interp_fwd(const float* in, float* out, int B, int tin, int pad, int ratio, hipStream_t stream);
int sed_interp_bwd(const float* dout, float* din, int B, int tin, int pad, int ratio, hipStream_t stream);
/* EncoderSlideWindow merge + global/local mix (src/models/encoder_slide_window.py:16-36; passt_sed.py:266-271).
   Window w (0..nW-1) starts at output frame lefts[w] and holds tps[w] pooled frames per clip; its [B, tps[w], 768] block begins at row
   offs[w] of pooled_win.  The row ranges [offs[w], offs[w] + B tps[w]) are disjoint and tile [0, rows), rows = B sum_w tps[w]; they
   may lie in ANY order (offs need not grow with w).  Output frames of a window at or past T are dropped, frames no window covers
   get a local part of 0. */
int sed_window_mix(const float* pooled_win, const int* lefts, const int* tps, const int* offs, int nW, float* x,
                   float mix, int B, int T, int ratio, hipStream_t stream);
/* its backward (autograd of encoder_slide_window.py:16-36 + the mix of passt_sed.py:266-271, student with encoder_win=True):
   dx [B, T, 768] -> dpooled_win (same packed layout and the same lefts / tps / offs tables as pooled_win, `rows` rows in all, every
   one of them written) and dglobal = (1 - mix) dx */
int sed_window_mix_bwd(const float* dx, const int* lefts, const int* tps, const int* offs, int nW, float* dpooled_win,
                       float* dglobal, float mix, int B, int T, int ratio, int rows, hipStream_t stream);
/* MlmModule.setence_mask application (src/models/transformer/mask.py:62-85) and masked MSE (mlm_passt/train.py:36-38) */
int sed_mlm_apply(const float* x, const float* mask_token, const uint8_t* action, const int* src_idx, float* out,
                  int rows, hipStream_t stream);
int sed_mlm_apply_bwd(const float* dout, const uint8_t* action, const int* src_idx, float* dx_zeroed, float* dtoken,
                      int rows, hipStream_t stream);
/* n_masked_rows_dev (nullable): the row count as a device int, read by the kernel instead of n_masked_rows (no host sync) */
int sed_masked_mse(const float* pred, const float* target, const uint8_t* mask, int n_masked_rows, const int* n_masked_rows_dev,
                   float* loss_zeroed, float* dpred, float* dtarget, int rows, hipStream_t stream);
/* The six mean-teacher loss terms of Trainer.train and their gradients in one call (recipes/desed/finetune/train.py:160-191):
   l_strong = BCE(s_strong[:strong_n], labels[:strong_n]), l_weak = BCE(s_weak[ws], labels_weak[ws]), l_at = BCE(s_at[ws], labels_weak[ws]),
   lc_strong = MSE(s_strong, t_strong), lc_weak = MSE(s_weak, t_at), lc_at = MSE(s_at, t_at)   (ws = clips weak_lo .. weak_lo + weak_n - 1),
   total = l_strong + w_weak l_weak + w_at l_at + w_cons (lc_strong + w_weak_cons lc_weak + w_at lc_at); torch.nn.BCELoss / MSELoss
   semantics (mean reduction, log clamped at -100, BCE gradient denominator clamped at 1e-12).
   out[8] = {total, l_strong, l_weak, l_at, lc_strong, lc_weak, lc_at, 0}; scratch[8] is zeroed by the call;
   d_strong [B,C,T], d_weak [B,C], d_at [B,C] = d total / d (student outputs). */
int sed_sed_losses(const float* s_strong, const float* s_weak, const float* s_at, const float* t_strong, const float* t_at,
                   const float* labels, const float* labels_weak, int B, int C, int T, int strong_n, int weak_lo, int weak_n,
                   float w_weak, float w_weak_cons, float w_at, float w_cons, float* scratch, float* out, float* d_strong,
                   float* d_weak, float* d_at, hipStream_t stream);
/* classifier + sigmoid(x/temp) + pad mask + linear-softmax pooling (passt_sed.py:285-296) */
int sed_head_fwd(const float* x, const float* W, const float* bias, float temp, const uint8_t* pad_mask, float* strong,
                 float* weak, float* sums, int B, int T, int C, hipStream_t stream);
int sed_head_bwd(const float* x, const float* W, const float* strong, const float* sums, const float* dstrong,
                 const float* dweak, float temp, float* dx, float* dW, float* db, int B, int T, int C,
                 hipStream_t stream);
/* AttentionPooling (src/models/pooling.py:45-51): 1-query MHA over the patch tokens; kv [B,N,1536] bf16 */
int sed_attnpool_fwd(const void* kv, const float* q, float* out, float* probs, int B, int N, int H, int f16,
                     hipStream_t stream);
int sed_attnpool_bwd(const void* kv, const float* q, const float* probs, const float* dout, void* dkv, float* dq, int B,
                     int N, int H, int f16, hipStream_t stream);
/* torch.optim.AdamW step (recipes/desed/setting.py:254-258) fused with update_ema (src/utils/scheduler.py:125-130) */
int sed_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float wd, float beta1,
                  float beta2, float eps, int step, float ema_alpha, int do_adam, hipStream_t stream);

/* ---- gradient-norm clipping on the flat fp32 gradient arena (csrc/grad_clip.hip): torch.nn.utils.clip_grad_norm_ with norm_type 2 as
 * three launches without a host synchronisation.  Every sum runs in a fixed order (no float atomics): results are bit-reproducible. */
/* partial[c] = sum of g[i]^2 over chunk c; chunk_tab int32 [n_chunks, 2] = {arena offset (multiple of 4), length in floats}: a chunk lies
 * inside one tensor's slice (at most 16384 floats from the host table, transformer4sed_amd/grad_clip.py); fp32, one workgroup per chunk */
int sed_grad_sumsq_chunks(const float* g, const int32_t* chunk_tab, int n_chunks, float* partial, hipStream_t stream);
/* tensor_first_chunk int32 [n_tensors + 1] (tensor t owns chunks [first[t], first[t + 1]), possibly none).  fp64 sums in chunk, then layout
 * order: norms[t] = sqrt(sumsq_t), total_and_scale = {total = sqrt(sum_t sumsq_t), scale = min(1, max_norm / (total + 1e-6))} (torch's
 * clip coefficient, non-finite values not special-cased: error_if_nonfinite=False); max_norm <= 0: measure only, scale = 1 */
int sed_grad_norm_finalize(const float* partial, const int32_t* tensor_first_chunk, int n_tensors, float max_norm,
                           float* norms /*[n_tensors]*/, float* total_and_scale /*[2]*/, hipStream_t stream);
/* g[0..n) *= scale[0] (device scalar; n a multiple of 4).  scale >= 1: returns without reading or writing g */
int sed_scale_by_dev(float* g, int64_t n, const float* scale, hipStream_t stream);

/* every weight image of a model in one launch (what sed_transpose_to_bf16 + sed_split3_f16 produce per weight): desc is a device
 * table of n_desc x 16 int64 {fp32 master, transposed bf16 image [C, R] or 0, straight 16-bit image [R, C] or 0,
 * split-precision f16 image [R, 3C] = [hi | hi | lo] or 0, R (multiple of 16), C (multiple of 64), straight-image kind
 * (0 bf16, 2 f16), index of the weight's first 64 x 64 tile, gather plan int32 [R, C] or 0 (image element -> master element; without
 * one the master IS [R, C]), scale plan fp32 [R, C] or 0, LoRA A fp32 [r, C] or 0, LoRA B fp32 [R, r], r, LoRA scaling as float bits,
 * 0, 0}; image = gather(master) * scale + s B A (src/models/lora/layers.py:148-151: the train-mode LoRA linear W x + s B (A x) as one
 * weight; the plans: zero-padded context-network / CNN images of the PMAM model); total_tiles = sum of ceil(R / 64) * (C / 64). */
int sed_weight_images(const int64_t* desc, int n_desc, int total_tiles, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * PMAM variant of the model path: PaSST_CNN.forward (src/models/cnn_transformer/passt_cnn.py:31-88).
 * By source: csrc/lora.hip (sed_lora_*), csrc/cnn_branch.hip (convolution patches, column statistics, BatchNorm, ContextGating, dropout
 * masks), csrc/dw_narrow.hip (sed_transpose_narrow, sed_small_dw), csrc/pmam.hip (the rest).
 * ------------------------------------------------------------------------------------------------------------------------- */
/* LoRA merge W_eff = W + scaling * B A, fp32 [n_out, k_in] (src/models/lora/layers.py:120-153; r = rank, A [r, k_in], Bm [n_out, r]) */
int sed_lora_merge(const float* W, const float* A, const float* Bm, float scaling, float* out, int n_out, int k_in, int r,
                   hipStream_t stream);
/* LayerNorm of width D (multiple of 128, <= 1024): the 384-wide context network (src/models/transformer/transformerXL.py:31-35).
 * Same outputs as sed_layernorm_fwd (16-bit and/or fp32 result, per-row mean / rstd for the backward; all nullable). */
int sed_ln_fwd_any(const float* x, const float* gamma, const float* beta, float eps, float in_scale, void* y16, float* y32,
                   float* mean, float* rstd, int M, int D, int f16, hipStream_t stream);
/* MlmModule.setence_mask application on rows of width C (src/models/transformer/mask.py:62-85); see sed_mlm_apply */
int sed_mlm_apply_c(const float* x, const float* mask_token, const uint8_t* action, const int* src_idx, float* out, int rows,
                    int C, hipStream_t stream);
/* CNN branch (src/models/cnn/base.py:62-113): 3x3 / pad 1 patch gathers for the im2col GEMMs.  Layer 0 reads the mel
 * spectrogram [B, 128, T] (the reference's input.transpose(1, 2).unsqueeze(1), passt_cnn.py:51) into col [B*T*128, 64]
 * (9 taps + zeros); later layers read NHWC 16-bit activations X [B, H, W, Cp] into col [B*H*W, Kp], column = tap * C + c. */
int sed_conv0_im2col(const float* mel, void* col, int B, int T, int f16, hipStream_t stream);
/* first convolution with 16 filters, direct on the fp32 spectrogram (no patch matrix): Y [B*T*128, 16] fp32 = conv3x3(mel) + bias, Wc =
 * conv0.weight [16, 1, 3, 3] (kernel rows over time, columns over frequency); and its weight / bias gradient from dY bf16 [pixels, ldy]:
 * dW[c, tap] += sum dY[m, c] patch(m, tap) (row stride ldw >= 9), dbias[c] += sum dY[m, c] (nullable).  s1 / s2 (nullable pair): the
 * BatchNorm batch-statistics sums of Y (sed_colstats mode 0) accumulated by the same pass */
int sed_conv0_fwd16(const float* mel, const float* Wc, const float* bias, float* Y, int B, int T, float* s1, float* s2, hipStream_t stream);
int sed_conv0_dw16(const void* dY, int ldy, const float* mel, float* dW, int ldw, float* dbias, int B, int T, hipStream_t stream);
int sed_conv3x3_im2col(const void* X, void* col, int B, int H, int W, int C, int Cp, int Kp, hipStream_t stream);
/* BatchNorm2d(eps 1e-3) as the per-channel affine Z = Y * a + b (base.py:72-75): 16-bit operand of the ContextGating GEMM,
 * channels C..Cp-1 zero.  Y [M, ldy] fp32 is the convolution output. */
int sed_bn_act(const float* Y, int ldy, const float* a, const float* b, void* Z, int64_t M, int C, int Cp, int f16,
               hipStream_t stream);
/* ContextGating (base.py:19-30) + Dropout (mask [M, C] bytes, nullable; kept values * drop_scale) + AvgPool2d((ph, pw)):
 * out[b, ho, wo, c] = mean of (Y a + b) * sigmoid(L) * keep.  out16 NHWC with channel pad Cpo and/or out32 [rows, C]. */
int sed_cg_pool(const float* Y, int ldy, const float* a, const float* b, const float* L, int ldl, const uint8_t* mask,
                float drop_scale, void* out16, float* out32, int B, int H, int W, int C, int Cpo, int ph, int pw, int f16,
                hipStream_t stream);
/* 'attention' frequency pooling (src/models/pooling.py:37-51, 6 heads; passt_sed.py:211-215): kv [B*N, 1536] 16-bit (k | v of the
 * out_norm'ed tokens), q [768] projected query -> out [B*tp, 768] (16-bit and/or fp32), probs [B*tp, 6, 12] (nullable). */
int sed_fpool_attn_fwd(const void* kv, const float* q, void* out16, float* out32, float* probs, int B, int N, int tp, int f16,
                       hipStream_t stream);
/* projector merge (passt_cnn.py:57-62): out[b, j] = lerp_r1(pad1(P1))[j] + mw[0] * lerp_r2(P2)[j], F.interpolate(linear,
 * align_corners=False) arithmetic; P1 [B, tp1, C], P2 [B, tp2, C], (tp1 + pad1) * r1 == tp2 * r2 output frames. */
int sed_pmam_merge(const float* P1, const float* P2, const float* mw, float* out, int B, int tp1, int pad1, int r1, int tp2,
                   int r2, int C, hipStream_t stream);

/* --- backward of the PMAM path --- */
int sed_ln_bwd_any(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float in_scale,
                   float* dx, int accumulate, float* dgamma, float* dbeta, int M, int D, hipStream_t stream);
int sed_mlm_apply_bwd_c(const float* dout, const uint8_t* action, const int* src_idx, float* dx_zeroed, float* dtoken, int rows,
                        int C, hipStream_t stream);
/* dP1 / dP2 / d merge_weight of sed_pmam_merge (dmw += , nullable) */
int sed_pmam_merge_bwd(const float* g, const float* P2, const float* mw, float* dP1, float* dP2, float* dmw, int B, int tp1,
                       int pad1, int r1, int tp2, int r2, int C, hipStream_t stream);
/* LoRA gradients by skinny products (src/models/lora/layers.py:148-151: y = x W^T + s (x A^T) B^T, A [r, in], B [out, r]; autograd:
 * dB = s dy^T (x A^T), dA = (s dy B)^T x) -- one pass over x or dy each, the gradient of the merged weight is never formed:
 *   rowproj    out[M, r] fp32 = scale * X[M, K] (16-bit, row stride ldx) . Wm, Wm fp32 [r, K] (w_kxr 0) or [K, r] (1); K % 32 == 0, r <= 16
 *   colreduce  G += scale * sum_m P[m, j] Y[m, c], P fp32 [M, r], Y 16-bit [M, C] (row stride ldy); G fp32 [C, r] (g_cxr 1) or [r, C] (0);
 *              C % 4 == 0, r <= 8 */
int sed_lora_rowproj(const void* X, int x_f16, int M, int K, int ldx, const float* Wm, int w_kxr, int r, float scale, float* out,
                     hipStream_t stream);
int sed_lora_colreduce(const void* Y, int y_f16, int M, int C, int ldy, const float* P, int r, float scale, float* G, int g_cxr,
                       hipStream_t stream);
/* weight / bias gradient of a 16- or 32-filter layer as a streaming reduction (the autograd of the CNN branch's gate Linear and 3x3
 * convolution, src/models/cnn/base.py:19-30, 62-100, for its first layers): dW[i, j] += sum_m dY[m, i] X[m, j] (i < n in {16, 32},
 * j < k <= 512, k % 4 == 0), dbias[i] += sum_m dY[m, i] (nullable); dY bf16 [M, ldy], X 16-bit [M, ldx], dW fp32 row stride ldw */
int sed_small_dw(const void* dY, int ldy, int n, const void* X, int x_f16, int ldx, int k, float* dW, int ldw, float* dbias, int64_t M,
                 hipStream_t stream);
/* keep-masks of nn.Dropout(p) (src/models/cnn/base.py:88-89): mask[e] = 1 with probability 1 - p (resolved to 2^-16), n % 4 == 0;
 * counter-based generator keyed by `seed` (the values differ from torch's Philox stream; only the distribution belongs to the model) */
int sed_dropout_mask(uint8_t* mask, int64_t n, float p, int64_t seed, hipStream_t stream);
/* BatchNorm2d(eps, momentum) batch statistics -> per-channel affines (src/models/cnn/base.py:72-75, torch BatchNorm semantics):
 * s1 / s2 = sed_colstats(mode 0) sums over the M rows (train: running_mean / running_var updated in place, unbiased variance) or
 * nullptr (eval: the running statistics are used); a = gamma rstd, b = beta - mean a, ah = rstd, bh = -mean rstd. */
int sed_bn_finalize(const float* s1, const float* s2, const float* gamma, const float* beta, float* run_mean, float* run_var,
                    int64_t M, int C, double momentum, double eps, float* a, float* b, float* ah, float* bh, hipStream_t stream);
/* batched small gathers / scatter-adds between fp32 masters and the padded images the kernels use; desc n_desc x 8 int64, one
 * workgroup per 256 elements (first block per descriptor in field 5):
 *   gather       {src, plan int32 [n], scale fp32 [n] or 0, dst [n], n, first block, 0, 0}:  dst[e] = src[plan[e]] * scale[e]
 *   scatter_add  {gimg, plan int32 [n] or 0, scale fp32 [n] or 0, gmaster, n, first block, C | ld_i << 32, ld_j}:
 *                gmaster[plan[e]] += scale[e] * gimg[(e / C) ld_i + (e % C) ld_j] where scale[e] != 0 (plans are injective there) */
int sed_gather_f32(const int64_t* desc, int n_desc, int total_blocks, hipStream_t stream);
int sed_scatter_add_f32(const int64_t* desc, int n_desc, int total_blocks, hipStream_t stream);
/* column sums over the M rows (+= into s1, s2): mode 0: sum A, sum A^2 (BatchNorm batch statistics, base.py:72-75 in train mode);
 * mode 1: sum A, sum A * (Bm * a + b) (BatchNorm backward sums with xhat = Y * a + b) */
int sed_colstats(const float* A, int lda, const float* Bm, int ldb, const float* a, const float* b, float* s1, float* s2,
                 int64_t M, int C, int mode, hipStream_t stream);
/* sed_bn_act + the ContextGating Linear + sed_cg_pool for a 16-filter layer in one pass (base.py:19-30, 72-100): l = Wg z + bg on the fp32
 * z = Y a + b (Wg fp32 [16, 16], bg [16]); optional side outputs for the backward: the logits Lout [pixels, 16] fp32 and the 16-bit image
 * Zout [pixels, 16] of z; out16 NHWC with channel pad Cpo (multiple of 8) and / or out32 [rows, 16] as sed_cg_pool */
int sed_cg_gate16_pool(const float* Y, int ldy, const float* a, const float* b, const float* Wg, const float* bg, const uint8_t* mask,
                       float drop_scale, float* Lout, void* Zout, void* out16, float* out32, int B, int H, int W, int Cpo, int ph, int pw,
                       int f16, hipStream_t stream);
/* backward of sed_cg_gate16_pool: dz [M, 16] fp32 = direct path + Wg^T dl (the complete gradient of z), dL16 [M, 16] bf16 = dl;
 * s1 / s2 (nullable pair, with ah / bh): the BatchNorm backward sums of dz (sed_colstats mode 1) accumulated by the same pass */
int sed_cg_gate16_pool_bwd(const float* dout, const float* Y, int ldy, const float* a, const float* b, const float* L, const float* Wg,
                           const uint8_t* mask, float drop_scale, float* dz, void* dL16, int B, int H, int W, int ph, int pw,
                           const float* ah, const float* bh, float* s1, float* s2, hipStream_t stream);
/* backward of sed_cg_pool: dzd [M, ldz] fp32 (direct path into the BatchNorm output; columns C..ldz-1 zero), dL16 [M, ldl16]
 * bf16 (gate logits; columns C.. zero) */
int sed_cg_pool_bwd(const float* dout, const float* Y, int ldy, const float* a, const float* b, const float* L, int ldl,
                    const uint8_t* mask, float drop_scale, float* dzd, int ldz, void* dL16, int ldl16, int B, int H, int W, int C,
                    int ph, int pw, hipStream_t stream);
/* BatchNorm backward with batch statistics: dY bf16 [M, ldo] from dz, xhat = Y * ah + bh and the sed_colstats(mode 1) sums */
int sed_bn_bwd(const float* dz, int ldz, const float* Y, int ldy, const float* ah, const float* bh, const float* gamma,
               const float* s1, const float* s2, void* dY, int ldo, int64_t M, int C, hipStream_t stream);
/* transpose of sed_conv3x3_im2col: dcol bf16 [B*H*W, Kp] -> dX fp32 [B, H, W, C] */
int sed_col2im3x3(const void* dcol, int Kp, float* dX, int B, int H, int W, int C, hipStream_t stream);
int sed_fpool_attn_bwd(const void* kv, const float* q, const float* probs, const float* dout, void* dkv, float* dq, int B, int N,
                       int tp, int f16, hipStream_t stream);
/* LoRA factor gradients from the merged-weight gradient: dB += s dW A^T, dA += s B^T dW (src/models/lora/layers.py:148-151) */
int sed_lora_grad(const float* dW, const float* A, const float* Bm, float scaling, float* dA, float* dB, int n_out, int k_in,
                  int r, hipStream_t stream);
/* prototype-similarity BCE of the PMAM trainer (recipes/desed/pmam/train.py:82-87, 100-106): loss[0] += mean BCE over the
 * `sel`ected frames x C classes; dlogit [B*T, 768] (nullable) = d loss / d logit; post [B*T, C] (nullable) = posteriors.
 * protos [C, 768] are the row-normalised GMM means (train.py:31); labels [B, C, T].  n_selected_dev (nullable): the number of
 * selected frames as a device int, read by the kernel instead of n_selected (no host sync). */
int sed_proto_bce(const float* logit, const float* protos, const float* labels, const uint8_t* sel, int n_selected,
                  const int* n_selected_dev, float temperature, float* loss, float* dlogit, float* post, int B, int T, int C, int D,
                  hipStream_t stream);

/* transpose of a narrow 16-bit matrix (bf16 or, in_f16 != 0, IEEE half): in [R, ldin] with C = 8, 16, 24 or 32 valid columns
 * -> outT bf16 [C, Rpad] (rows R..Rpad-1 zero) + optional fp32 column sums (+=): the weight-gradient operands of the 16/32-filter
 * CNN layers (src/models/cnn/base.py:62-70) */
int sed_transpose_narrow(const void* in, int in_f16, int R, int C, int ldin, void* outT, int Rpad, float* colsum,
                         hipStream_t stream);

/* ------------------------------------------------------------------ DASM query decoder + dual-stream head (round 5, forward) */
/* fp32 GEMM on the fp32-input matrix instruction (exact fp32 products / accumulation): C[z][M,N] = act(A[z][M,K] . B[z][N,K]^T + bias[N])
 * (+ R[z][M,N], same ldc / stride as C; nullable), z < batch with element strides (0 = shared operand); act 0 none, 1 GELU, 2 ReLU;
 * K % 32 == 0, lda / ldb / strides % 4 == 0, 16-byte aligned A / B.  The precision-critical small linears of the DASM head: nn.Linear in
 * src/models/detect_any_sound/detect_any_sound.py:76-78,125,138,401-416, the in_proj / out_proj / linear1 / linear2 of
 * at_adapter.py:36-45, and the per-clip einsum('bqc,bct->bqt') of detect_any_sound.py:394. */
int sed_gemm_f32_nt(const float* A, const float* B, const float* bias, const float* R, float* C, int M, int N, int K, int lda, int ldb,
                    int ldc, int batch, int64_t strideA, int64_t strideB, int64_t strideC, int act, hipStream_t stream);
/* softmax(q k^T / sqrt(head_dim) + mask) v with Nq != Nk, fp32 (torch.nn.MultiheadAttention inside nn.TransformerDecoderLayer,
 * at_adapter.py:24-32: cross attention of the queries over the patch tokens, self attention among the queries): Q rows
 * [b * q_batch_stride + i * ldq + h * head_dim] (q_batch_stride 0 = the same queries for every clip), K / V rows [(b * Nk + j) * ld + h *
 * head_dim], O [B, Nq, ldo]; mask [Nq, Nk] bytes, non-zero = not allowed (nullable); head_dim 32 or 64. */
int sed_xattn_f32_fwd(const float* Q, const float* K, const float* V, float* O, const uint8_t* mask, int B, int H, int Nq, int Nk,
                      int head_dim, int ldq, int ldk, int ldv, int ldo, int64_t q_batch_stride, hipStream_t stream);
/* dual-stream finish (detect_any_sound.py:317-319, 394-404): logits [B,T,Q], at_logit [B,Q], pad_mask [B,T] (nullable) ->
 * at_out = sigmoid(at_logit) [B,Q] (nullable), strong [B,Q,T] = clamp(pad ? 0 : sigmoid(logit / temp) * at_out, 1e-7, 1),
 * weak [B,Q] = clamp(sum_t strong^2 / sum_t strong, 1e-7, 1).  at_logit == NULL with clamp_strong == 0: the closed-set classifier head for
 * any class count, strong = pad ? 0 : sigmoid(logit / temp) without a clamp (src/models/cnn_transformer/passt_cnn.py:74-86). */
int sed_dasm_head_fwd(const float* logits, const float* at_logit, const uint8_t* pad_mask, float temp, float* strong, float* weak,
                      float* at_out, int B, int T, int Q, int clamp_strong, hipStream_t stream);

/* ---- DASM / AudioSet-Strong TRAINING (recipes/audioset_strong/detect_any_sound/passt/train.py:66-120 `DASMTrainer.train`,
 * recipes/audioset_strong/base/passt_cnn/train.py:103-140 `Trainer.train`): the backward of everything above, fp32.
 *
 * General fp32 GEMM on v_mfma_f32_32x32x2_f32:  C[z][m][n] (+)= drop(act(sum_k A(z,m,k) B(z,n,k) + bias[n])) (+ R[z][m][n]) with
 * A(m,k) = transA ? A[k lda + m] : A[m lda + k], B(n,k) = transB ? B[k ldb + n] : B[n ldb + k] -- the three products of a Linear under
 * autograd (y = x W^T; dx = dy W: transB; dW += dy^T x: transA + transB + accumulate, split over the tokens by `ksplit` with fp32
 * atomics) and the einsum('bqc,bct->bqt') of detect_any_sound.py:378 with its gradients (batched).  Any M, N, K and leading dimensions
 * (operands that are not float4-addressable are read element-wise).  pre (nullable): the value before the activation (what the GELU
 * backward needs).  drop_p > 0: inverted dropout after the activation, before the residual, with the counter-based bits
 * keep(drop_seed, drop_site, (z M + m) N + n) that sed_gelu_bwd_f32 / sed_dropout_f32 re-evaluate (nn.TransformerDecoderLayer's
 * dropout1/2/3 and FFN dropout in train mode, at_adapter.py:37-45).  accumulate != 0: C += (no epilogue terms allowed). */
int sed_gemm_f32(const float* A, const float* B, const float* bias, const float* R, float* C, float* pre, int M, int N, int K, int lda,
                 int ldb, int ldc, int transA, int transB, int batch, int64_t strideA, int64_t strideB, int64_t strideC, int act,
                 int accumulate, int ksplit, float drop_p, int64_t drop_seed, int drop_site, hipStream_t stream);
/* sed_xattn_f32_fwd for a pass whose backward follows: also writes lse [B, H, Nq] (log2 of sum_j 2^(log2(e) s_ij)) and applies
 * attention-probability dropout (torch.nn.MultiheadAttention(dropout=p).train(): softmax -> dropout -> . v) with the bits
 * keep(seed, site, ((b H + h) Nq + i) Nk + j). */
int sed_xattn_f32_fwd_train(const float* Q, const float* K, const float* V, float* O, const uint8_t* mask, float* lse, int B, int H, int Nq,
                            int Nk, int head_dim, int ldq, int ldk, int ldv, int ldo, int64_t q_batch_stride, float drop_p, int64_t drop_seed,
                            int drop_site, hipStream_t stream);
/* its backward: dQ [B, Nq, lddq], dK / dV [B, Nk, lddk / lddv] at column h * head_dim (overwritten, packed projections are addressed in
 * place through the leading dimensions); O, dO [B, Nq, ldo]; Dq [B, H, Nq] scratch (dO_i . O_i). */
int sed_xattn_f32_bwd(const float* Q, const float* K, const float* V, const float* O, const float* dO, const float* lse, float* Dq, float* dQ,
                      float* dK, float* dV, const uint8_t* mask, int B, int H, int Nq, int Nk, int head_dim, int ldq, int ldk, int ldv, int ldo,
                      int lddq, int lddk, int lddv, int64_t q_batch_stride, float drop_p, int64_t drop_seed, int drop_site,
                      hipStream_t stream);
/* backward of sed_dasm_head_fwd: d strong [B,Q,T], d weak [B,Q], d at_out [B,Q] (each nullable) -> d logits [B,T,Q], d at_logit [B,Q].
 * at_logit == dat_logit == NULL: the closed-set head strong = sigmoid(logit / temp) for any class count (passt_cnn.py:74-86 with the 407
 * AudioSet-Strong classes).  scratch: 3 B Q floats. */
int sed_dasm_head_bwd(const float* logits, const float* at_logit, const uint8_t* pad_mask, float temp, const float* strong,
                      const float* dstrong, const float* dweak, const float* dat_out, float* dlogits, float* dat_logit, float* scratch, int B,
                      int T, int Q, int clamp_strong, hipStream_t stream);
/* out = dy o keep / (1 - p) o gelu'(pre) over n elements (keep bits of element index i: see sed_gemm_f32) */
int sed_gelu_bwd_f32(const float* dy, const float* pre, float* out, int64_t n, float drop_p, int64_t drop_seed, int drop_site,
                     hipStream_t stream);
/* out = x o keep / (1 - p) (nullable) and / or the keep bits themselves as bytes (nullable; test aid for the CPU oracle) */
int sed_dropout_f32(const float* x, float* out, uint8_t* mask_u8, int64_t n, float drop_p, int64_t drop_seed, int drop_site,
                    hipStream_t stream);
/* out = drop(act(x)) (+ res) over n elements; act 1 = GELU; dropout bits of element index i (see sed_gemm_f32) */
int sed_act_drop_res_f32(const float* x, const float* res, float* out, int64_t n, int act, float drop_p, int64_t drop_seed, int drop_site,
                         hipStream_t stream);
/* out[c] += sum_r x[r ld + c] */
int sed_colsum_f32(const float* x, float* out, int rows, int cols, int64_t ld, hipStream_t stream);
/* supervised losses of src/functional/loss/__init__.py (loss_function_factory), mean over n elements, loss[0] += value (caller zeroes),
 * grad (nullable) = d loss / d pred.  kind 0: -[(1-p)^gamma_pos t max(log p, -100) + pm^gamma_neg (1-t) max(log(1-pm), -100)],
 * pm = max(p - margin, 0): BCELoss (0, 0, 0), AsymmetricalFocalLoss(gamma, zeta), AslLoss(rp, rn, margin); kind 1: MSELoss. */
int sed_sup_loss(const float* pred, const float* target, float* loss, float* grad, int64_t n, int kind, float gamma_pos, float gamma_neg,
                 float margin, hipStream_t stream);

/* ------------------------------------------------------------------ Conformer context network (csrc/conformer.hip) */
/* The middle of ConvolutionModule.forward (src/models/transformer/conformer.py:242-270) in one pass: x [B T, 2 C] fp32 (pointwise_conv1's
 * output, bias applied) -> u = a * sigmoid(g) (a = columns 0 .. C-1, g = C .. 2C-1) -> c[t] = bias + sum_k w[k] u[t + k - 15] (w [C, 31],
 * zeros outside 0 <= t + k - 15 < T of the same clip) -> LayerNorm over C (gamma, beta, eps) -> y = n * sigmoid(n).  C = 768.
 * y16 (nullable): the operand image of the pointwise_conv2 GEMM, mode 0 bf16 [B T, C], 1 f16, 4 split precision f16 [B T, 3 C] =
 * [hi | lo | hi] (as sed_layernorm_fwd writes it); y32 (nullable): fp32 [B T, C].  conv / mean / rstd (nullable together): the
 * convolution output fp32 [B T, C] and the LayerNorm statistics [B T], what sed_conv_glu_dw_bwd reads. */
int sed_conv_glu_dw_fwd(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, float eps, void* y16,
                        float* y32, float* conv, float* mean, float* rstd, int B, int T, int C, int mode, hipStream_t stream);
/* Its backward: dy fp32 [B T, C] -> dx16 = bf16 [B T, 2 C] (gradient of pointwise_conv1's output), and dw [C, 31], dbias, dgamma,
 * dbeta [C] (each nullable) += their gradients.  Those four are sums over all frames, taken in a fixed order (per-workgroup partials in
 * `partials`, then one pass over them): the same bits in every run.  partials: scratch of min(B * ceil(T / 20), 256) * 34 * C floats. */
int sed_conv_glu_dw_bwd(const float* dy, const float* x, const float* conv, const float* mean, const float* rstd, const float* w,
                        const float* gamma, const float* beta, void* dx16, float* dw, float* dbias, float* dgamma, float* dbeta,
                        float* partials, int64_t partial_floats, int B, int T, int C, hipStream_t stream);
/* Swish of the feed-forwards (conformer.py:46-58,147-152): h fp32 [M, C] -> operand image of h * sigmoid(h) (y16, mode as above; nullable)
 * and / or its fp32 value (y32, nullable);  backward: dh16 = bf16(dy * Swish'(h)) over n elements (n % 4 == 0) */
int sed_swish_fwd(const float* h, void* y16, float* y32, int M, int C, int mode, hipStream_t stream);
int sed_swish_bwd(const float* dy, const float* h, void* dh16, int64_t n, hipStream_t stream);
/* out = res + scale * in over n fp32 elements (n % 4 == 0; res nullable; out may alias in or res), out16 (nullable) = bf16 of the result */
int sed_scale_add_f32(const float* in, const float* res, float* out, void* out16, int64_t n, float scale, hipStream_t stream);

/* ------------------------------------------------------------------ Frequency-wise transformer pooling (csrc/fpool_transformer.hip) */
/* PaSST_SED(f_pool="frequency_wise_tranformer_encoder"): src/models/pooling.py:18-34 behind src/models/passt/passt_sed.py:199-218.
 * Sequence build: x fp32 [Bx, 2 + F tp, 768] (token stream of the tapped layer, patch tokens in (f, t) order) -> xs fp32
 * [Bx tp, 1 + F, 768]: row 0 of every sequence is the tag tag_w + tag_b (linear_emb applied to 1), row 1 + f is out_norm (gamma, beta, eps)
 * of patch token (f, t).  mean / rstd (nullable together): the LayerNorm statistics [Bx tp (1 + F)] by row of xs (0 in the tag rows). */
int sed_fpool_seq_build_fwd(const float* x, const float* gamma, const float* beta, float eps, const float* tag_w, const float* tag_b,
                            float* xs, float* mean, float* rstd, int Bx, int tp, int F, hipStream_t stream);
/* Its backward: dxs fp32 [Bx tp, 1 + F, 768] -> dx (nullable) fp32 [Bx, 2 + F tp, 768], written whole (cls / dist rows zero); dgamma,
 * dbeta, dtag [768] (each nullable) += the gradients of out_norm and the sum over the sequences of row 0's gradient.  Two stages in a
 * fixed order, no atomics: the same bits in every run.  partials: scratch of min(ceil(Bx tp (1 + F) / 4), 256) * 3 * 768 floats. */
int sed_fpool_seq_build_bwd(const float* dxs, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx,
                            float* dgamma, float* dbeta, float* dtag, float* partials, int64_t partial_floats, int Bx, int tp, int F,
                            hipStream_t stream);
/* frequency_transformer_norm on row 0 of every sequence: xs fp32 [S, N, 768] -> pooled fp32 [S, 768]; mean / rstd [S] nullable together */
int sed_fpool_rownorm_fwd(const float* xs, const float* gamma, const float* beta, float eps, float* pooled, float* mean, float* rstd,
                          int S, int N, hipStream_t stream);
/* Its backward: dxs fp32 [S, N, 768] is written whole (rows 1 .. N-1 zero); dgamma / dbeta (nullable) +=, in a fixed order.
 * partials: scratch of min(ceil(S / 4), 256) * 2 * 768 floats. */
int sed_fpool_rownorm_bwd(const float* dpooled, const float* xs, const float* mean, const float* rstd, const float* gamma, float* dxs,
                          float* dgamma, float* dbeta, float* partials, int64_t partial_floats, int S, int N, hipStream_t stream);
/* softmax(q k^T 192^-0.5) v of timm's Attention for S sequences of N tokens (2 <= N <= 16) and H heads of 192: qkv [S N, 3 H 192] is the
 * packed qkv GEMM output (in_kind: 0 bf16, 1 f16, 2 fp32), out the A operand of the proj GEMM (mode 0 bf16 / 1 IEEE half: [S N, H 192];
 * 4: the split-precision image [S N, 3 H 192] = [hi | lo | hi], as sed_layernorm_fwd writes it).  fp32 arithmetic; one wave owns a
 * (sequence, head). */
int sed_attn_short_fwd(const void* qkv, void* out, int S, int N, int H, int in_kind, int mode, hipStream_t stream);
/* Its backward: dout bf16 [S N, H 192] -> dqkv bf16 [S N, 3 H 192]; the probabilities are recomputed from qkv.  No atomics. */
int sed_attn_short_bwd(const void* qkv, const void* dout, void* dqkv, int S, int N, int H, int in_kind, hipStream_t stream);

/* ---- frequency-dynamic convolution of the PaSST_CNN branch (cnn_name "FDY-CNN"; src/models/cnn/FDY_cnn.py:7-116, pool_dim 'freq', four
 * basis kernels; csrc/fdy_cnn.hip).  R = B H frame rows; every reduction runs in a fixed order (no float atomics). */
/* FDY_cnn.py:97  x.mean(dim=3): X 16-bit NHWC [R, W, Cp] (channels C.. padding) -> pm fp32 [R, C] */
int sed_fdy_freq_mean(const void* X, int f16, float* pm, int64_t R, int W, int C, int Cp, hipStream_t stream);
/* FDY_cnn.py:107  conv1d1 (cin -> hid, kernel 3, padding 1 along the frames, no bias): pm [B H, cin], W1 [hid, cin, 3] -> u [B H, hid];
 * part (nullable: eval) double [ceil(B H / 16), 2, hid]: per-workgroup sums of u and u^2 for the BatchNorm1d batch statistics */
int sed_fdy_attn_taps(const float* pm, const float* W1, float* u, double* part, int B, int H, int cin, int hid, hipStream_t stream);
/* FDY_cnn.py:108-116  bn (batch statistics from `part`, running statistics updated by torch's rule: momentum, unbiased variance; part null:
 * running statistics), relu, conv1d2 (W2 [4, hid], b2 [4]), softmax(. / temperature) -> att [R, 4]; aff [3, hid] = mean | rstd | gamma rstd */
int sed_fdy_attn_softmax(const float* u, const double* part, const float* gamma, const float* beta, float* run_mean, float* run_var,
                         const float* W2, const float* b2, float temperature, double momentum, double eps, float* aff, float* att,
                         int R, int hid, hipStream_t stream);
/* FDY_cnn.py:53-61  Y[m, o] = sum_k att[m / W, k] Y4[m, k co + o]: Y4 fp32 [M, ld4] (the GEMM of the patch matrix with the [4 co, 9 cin]
 * weight image), Y fp32 [M, ldy] (columns co.. zero) */
int sed_fdy_mix_fwd(const float* Y4, int ld4, const float* att, float* Y, int ldy, int64_t M, int W, int co, hipStream_t stream);
/* its backward: dY bf16 [R W, ldo] -> dY4 bf16 [R W, ldg4] = att (x) dY (columns 4 co.. zero), da fp32 [R, 4] = sum_{w, o} dY Y4_k */
int sed_fdy_mix_bwd(const void* dY, int ldo, const float* Y4, int ld4, const float* att, void* dY4, int ldg4, float* da, int64_t R,
                    int W, int co, hipStream_t stream);
/* backward of sed_fdy_attn_softmax and sed_fdy_attn_taps: da [B H, 4] -> dpm [B H, cin]; gW1 [hid, cin, 3], ggamma / gbeta [hid], gW2 [4, hid],
 * gb2 [4] (each nullable) +=.  batch_stats: the forward ran on batch statistics.  Scratch: dz fp32 [B H, hid], part double
 * [ceil(B H / 16), 6 hid + 4], ws fp32 of at least ceil4(6 hid + 4) + clamp(B H / 128, 1, 32) * 3 hid cin floats */
int sed_fdy_attn_bwd(const float* da, const float* att, const float* u, const float* aff, const float* pm, const float* W1,
                     const float* beta, const float* W2, float temperature, int batch_stats, float* dz, double* part, float* ws,
                     int64_t ws_floats, float* dpm, float* gW1, float* ggamma, float* gbeta, float* gW2, float* gb2, int B, int H,
                     int cin, int hid, hipStream_t stream);
/* backward of sed_fdy_freq_mean onto the input gradient sed_col2im3x3 wrote: dX fp32 [R, W, C] += dpm [R, C] / W */
int sed_fdy_mean_bwd_add(float* dX, const float* dpm, int64_t R, int W, int C, hipStream_t stream);

/* ------------------------------------------------------------------ PMAM tokenizer: full-covariance Gaussian mixture (csrc/gmm.hip) */
/* What recipes/desed/pmam/gmm.py and generate_pseudo_label.py take from pycave's GaussianMixture(covariance_type="full"): the densities
 * of every frame under every component.  With Sigma_k = L_k L_k^T:  log N(x; mu_k, Sigma_k) = -0.5 (D log 2 pi + log det Sigma_k) -
 * 0.5 |L_k^-1 (x - mu_k)|^2.
 * sed_gmm_maha: X [N, D] fp32 (row pitch ldx >= D), P [K, D, D] fp32 with row j of P_k = row j of L_k^-1 (lower triangular; the strict
 * upper triangle must be zero: d tiles above the diagonal are not read), b [K, D] = -P_k mu_k ->
 *   maha[n, k] = sum_j (sum_d X[n, d] P_k[j, d] + b_k[j])^2,   maha [N, K] packed.
 * fp32-input matrix instruction (exact fp32 products, fp32 accumulation); the whitened row is never stored; every (n, k) is written once, no
 * atomics: the same bits in every run.  D % 32 == 0, 32 <= D <= 768, 1 <= K <= 64, N >= 1, P 16-byte aligned; otherwise SED_ERR_ARG. */
int sed_gmm_maha(const float* X, const float* P, const float* b, float* maha, int64_t N, int D, int K, int64_t ldx, hipStream_t stream);
/* Posteriors from maha [N, K] and logc [K] (logc_k = log pi_k - 0.5 (D log 2 pi + log det Sigma_k), host float64 rounded to fp32), scores
 * s = logc - 0.5 maha; every output nullable: resp [N, K] = softmax_k(s) (max subtracted), logp [N] = log sum_k exp(s), argmax [N] (lowest
 * index of the largest score), colsum_part [n_blocks, K] = per-workgroup column sums of resp (n_blocks <= 65535 = the launch's grid; the
 * rows a workgroup adds and their order depend on (N, n_blocks) alone).  1 <= K <= 64.
 * sed_gmm_colsum_reduce: colsum[k] (double; accumulate != 0: +=) = sum of the n_blocks partial rows in a fixed order -- N_k without atomics. */
int sed_gmm_resp(const float* maha, const float* logc, float* resp, float* logp, int* argmax, float* colsum_part, int n_blocks, int64_t N,
                 int K, hipStream_t stream);
int sed_gmm_colsum_reduce(const float* colsum_part, int n_blocks, int K, double* colsum, int accumulate, hipStream_t stream);
/* A[n, :] = sqrt(w[n w_stride]) (X[n, :] - mu) for rows 0 .. N-1: X row pitch ldx >= D, mu [D], w = one column of resp (pointer + stride),
 * A [N, D] packed -- the operand of the M-step's covariance product A^T A (sed_gemm_f32 with transA = transB = 1).  Writes nothing else. */
int sed_gmm_center_scale(const float* X, const float* mu, const float* w, float* A, int64_t N, int D, int64_t ldx, int64_t w_stride,
                         hipStream_t stream);

/* ------------------------------------------------------------------ long-form detection (csrc/longform.hip) */
/* Detection on a recording of any length: chunks of Lc samples every `hop` samples, the chunks' frame posteriors stitched into one timeline,
 * the timeline filtered and decoded.  The reference has only an unused stub (`get_segment_scores_and_overlap_add`, src/codec/decoder.py), the
 * definitions are DESIGN.md's.  No atomics on floats and no waiting between workgroups: the same bits in every run.
 * sed_longform_gather: wav [L] -> out [nk, Lc], chunk j = samples (k0 + j) hop .. + Lc, zeros from sample L on; 16-byte accesses when
 * hop, Lc and both pointers allow, scalar otherwise.  nk <= 65535. */
int sed_longform_gather(const float* wav, float* out, int64_t L, int64_t hop, int Lc, int k0, int nk, hipStream_t stream);
/* strong [K, C, Tc], weak [K, C] or NULL -> out [Tt, C] fp32: out[t, c] = sum_k w(t - k Hf) v_k / sum_k w(t - k Hf) over the chunks k with
 * k Hf <= t < k Hf + Tc in ascending order, v_k = strong[k, c, t - k Hf] (x weak[k, c]: one fp32 multiply), w(i) = min(i + 1, Tc - i,
 * max(1, Tc - Hf)); the sum in fp32, the integer denominator exact, one division.  A frame covered by ONE chunk is copied (x weak).
 * 1 <= Hf <= Tc, 1 <= Tt <= (K - 1) Hf + Tc. */
int sed_longform_stitch(const float* strong, const float* weak, float* out, int K, int C, int Tc, int Hf, int64_t Tt, hipStream_t stream);
/* The filters of sed_median_filter_k (same modes 0 / 1 / 2, same element selected: bit-exact with it wherever it applies) on in / out [T, C]
 * for any T < 2^31: tiles of 1024 frames with a halo of real neighbours, the boundary rule at the two ends of the timeline only.  sizes [C] on
 * the device, max_size the caller's bound on them (1 .. 1024; a class whose window exceeds it comes out as NaN); modes 1 / 2 need
 * max_size <= T. */
int sed_longform_filter(const float* in, float* out, const int* sizes, int64_t T, int C, int mode, int max_size, hipStream_t stream);
/* A bank of the filters of sed_median_filter_k for the post-processing search (csrc/median_filter.hip): in [B, T, C] ->
 * out [W, B, T, C], where out[w] holds bit for bit what sed_median_filter_k(in, ., sizes + w C, scale, B, T, C, mode, max_size) writes --
 * modes 0 / 1 / 2, scale [B, C] or NULL -- for every argument set that kernel accepts (T <= 12288; the order-statistics form for modes 0 / 1
 * with max_size >= 24, T >= 256 and T + max_size + 1 <= 2048, the rank search otherwise).  sizes [W, C] on the device, one window row per
 * candidate, free per class; max_size >= 1 is the caller's bound on them and is required here (it sizes the staged column).  One
 * workgroup per (clip, class) stages the padded column and ranks it once for all W rows.  1 <= W <= 64, B, T, C >= 1; the rank-search form
 * needs T + max_size - 1 <= 16384 entries of LDS; otherwise SED_ERR_ARG, and nothing is written.  A (row, class) whose window is below 1,
 * above max_size or (modes 1 / 2) above T comes out as NaN, the other planes intact.  Deterministic: no atomics, every element written once. */
int sed_median_filter_bank(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C, int W, int mode,
                           int max_size, hipStream_t stream);
/* Score-level ensembling for a bank of weight rows (csrc/ensemble.hip): members, a device table of M pointers to
 * x_m [n, T_m, C] f32 contiguous, Tm [M] int32 on the device (1 <= T_m; the caller keeps T_m <= T), w [W, M, C] f32 on the device, already
 * normalised (sum over m = 1) -> out [W, n, T, C] f32.  Member m is resampled to T frames by the linear half-pixel rule with the source
 * coordinate in integers (T_m == T: a copy, T_m == 1: a broadcast).  mode 0: y = sum_m w v_m, m ascending, unfused fp32, bit for bit a
 * float32 host restatement; mode 1: y = sigmoid(sum_m w logit(clamp(v_m, 1e-7f, 1 - 1e-7f))), in float64, rounded to fp32 at the end.
 * decimals -1: no rounding, 0 .. 9: y = rintf(y 10^d) / 10^d.  1 <= M <= 8, 1 <= W <= 64, W M C <= 32768 (the weights' LDS), n, T, C >= 1;
 * otherwise SED_ERR_ARG, and nothing is written.  The members are read once for all W rows; grid-stride over at most 1024 workgroups of
 * 256 threads; deterministic: no atomics, every element written once. */
int sed_ensemble_bank(const float* const* members, const int* Tm, const float* w, float* out, int M, int W, int n, int T, int C, int mode,
                      int decimals, hipStream_t stream);
/* Change-detection sound event bounding boxes for a bank of K parameter rows (csrc/sebb.hip; DESIGN.md section 7f, exact in integers): in
 * [B, T, C] fp32 in [0, 1] (x scale [B, C] or NULL: one fp32 multiply), params [K, C, 3] int32 on the device = (L, tau_q, rho_q) per row and
 * class: half length of the step filter in frames (>= 1; L >= T is L = T), rint(tau 2^24) in 0 .. 2^24, rint(rho 256) in 256 .. 4096.
 * -> out [K, B, T, C] (a box's confidence on its frames, 0 elsewhere), boxes [K, B, C, cap, 2] int32 (onset frame, offset frame; onsets
 * ascending), conf [K, B, C, cap] fp32, counts [K, B, C] int32 (the true number of boxes, also where it exceeds cap), status [2] int32:
 * status[0] = 1 if some row had more than cap boxes (its first cap are written, nothing past them), status[1] = 1 if a score was NaN or
 * outside [0, 1] (clamped).  Box slots from min(count, cap) on are left untouched.  One workgroup per (clip, class); steps shared by the
 * rows with the same L of a class run once.  1 <= T <= 1024, 1 <= K <= 64, 1 <= cap <= 1024 (cap >= (T + 1) / 2 never overflows), B, C >= 1;
 * otherwise SED_ERR_ARG, and nothing is written.  Deterministic: no atomics, every element written once by a plain store. */
int sed_sebb_bank(const float* in, const float* scale, const int* params, float* out, int* boxes, float* conf, int* counts, int* status,
                  int B, int T, int C, int K, int cap, hipStream_t stream);
/* Events of post [T, C]: frame t of class c is active iff post[t, c] > th[c] (strict), every maximal run is one event.  The timeline is cut
 * into segments of `seg` frames (nseg = ceil(T / seg) <= 65535).
 * sed_longform_event_count: seg_counts [C nseg] (run starts per class and segment, class-major), seg_offs [C nseg + 1] their exclusive
 * prefix sums, cls_offs [C + 1] the first row of each class (cls_offs[C] = number of events): what the host reads to allocate.
 * sed_longform_event_write: events [n, 3] int32 rows (class, onset frame, offset frame = last active + 1), class-major, onsets ascending,
 * from the same post / th / seg and the seg_offs of the count. */
int sed_longform_event_count(const float* post, const float* th, int64_t T, int C, int seg, int* seg_counts, int* seg_offs, int* cls_offs,
                             hipStream_t stream);
int sed_longform_event_write(const float* post, const float* th, int64_t T, int C, int seg, const int* seg_offs, int* events,
                             hipStream_t stream);

#ifdef __cplusplus
}
#endif
