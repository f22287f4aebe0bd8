/*
 * sdk_hip.h - C ABI of libsdk_hip.so, the MI355X (gfx950) speaker-embedding + assignment path.
 *
 * The reference (CLIAI/speaker-diarization-toolkit) is pure Python and calls no native code;
 * its plug-in boundary is the Python class contract
 *     speaker_detection_backends/base.py:22-200   (EmbeddingBackend)
 *     speaker_detection_backends/base.py:272-293  (get_backend -> module.Backend())
 * The entry points below are what a local backend behind that contract binds (ctypes stub in
 * INTEGRATION.md).  Each one cites the reference interface whose work it performs.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success, non-zero on failure; sdk_last_error() then holds a
 *     thread-local message.  Nothing falls back to the CPU.
 *   - all data pointers are DEVICE pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()), unless a parameter is documented as host memory.
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised.
 *   - bf16 tensors are passed as uint16_t* (raw bfloat16 bits).
 *   - "rows" of an activation tensor are frames: row m = segment (m / T), frame (m % T),
 *     channel-last, row stride given explicitly (ld*, in elements).
 *   - the workspace protocol, the same for every entry point that takes (ws, ws_bytes): the caller asks the entry point's
 *     sdk_*_workspace_bytes for a byte count (0 with sdk_last_error: arguments the call would refuse too), passes a device buffer of at
 *     least that many bytes, and the library assumes nothing about its contents and writes nothing past the count.  The call checks the
 *     workspace in three steps, each with its own message, each returning non-zero before anything is written or enqueued:
 *         "<fn>: null workspace (<need> bytes needed, <sizer>)"
 *         "<fn>: workspace of <ws_bytes> bytes, <need> needed (<sizer>)"
 *         "<fn>: ws=<address> must be <align>-byte aligned"
 *     The alignment is the one stated at the entry point (DESIGN.md lists them in one table); the arrays inside are carved in a fixed
 *     order, each rounded up to 256 bytes (csrc/workspace.hpp), by the one layout function the sizer and the call share.
 *
 * STABLE SURFACE - what a backend binds (INTEGRATION.md shows the stub); SDK_ABI_VERSION changes when any of these does:
 *     sdk_abi_version  sdk_init  sdk_shutdown  sdk_last_error  sdk_get_device_info
 *     sdk_device_malloc  sdk_device_free  sdk_memcpy  sdk_stream_synchronize          device memory for hosts without an allocator of their own
 *     sdk_resample_out_len  sdk_resample_s16                                   audio -> AudioProfile format
 *     sdk_fbank_tables_bytes  sdk_fbank_tables_fill  sdk_fbank_workspace_bytes  sdk_fbank  sdk_fbank_windows          k1
 *     sdk_ingest_create / _destroy / _acquire / _commit / _submit / _release / _copy_ms          host audio -> HBM, pinned + double-buffered
 *     sdk_ecapa_workspace_bytes  sdk_ecapa_forward  sdk_ecapa_calib_floats  sdk_ecapa_forward_calib            k2
 *     sdk_ecapa_masked_workspace_bytes  sdk_ecapa_forward_masked  (diarization in the ECAPA space: S masked poolings per chunk)
 *     sdk_xvector_workspace_bytes  sdk_xvector_forward                                                  k2 (second model family)
 *     sdk_resnet_workspace_bytes  sdk_resnet_forward                                                    k2 (third model family: ResNet34)
 *     sdk_l2norm                                                                                        k3
 *     sdk_affinity_workspace_bytes  sdk_affinity_topk                                                   k4
 *     sdk_affinity_matvec_workspace_bytes  sdk_affinity_matvec  sdk_rows_gram_workspace_bytes  sdk_rows_gram
 *     sdk_rows_apply  sdk_chol_inverse  sdk_sym_eigh  sdk_rows_unit  sdk_kmeans_mindist  sdk_kmeans_assign      k6 (driven by cluster.py;
 *                                                                                                       sdk_sym_eigh by sdk_laplacian_topk)
 *     sdk_centroid_linkage_workspace_bytes  sdk_centroid_linkage                                    k6 threshold path (cluster.agglomerative_cluster)
 *     sdk_linked_linkage_workspace_bytes  sdk_linked_linkage                                        speakers across recordings: constrained, early-stopping
 *                                                                                                       centroid linkage (cluster.link_rows, diarize.link_speakers)
 *     sdk_segmentation_frames  sdk_segmentation_workspace_bytes  sdk_segmentation_forward               speaker segmentation (PyanNet, segmentation.py)
 *     sdk_powerset_decode  sdk_diarize_masks  sdk_resnet_last_map_frames  sdk_resnet_masked_workspace_bytes
 *     sdk_resnet_forward_masked  sdk_diarize_frames  sdk_diarize_reconstruct  sdk_diarize_centroids  sdk_diarize_assign
 *     sdk_diarize_assign_grouped  sdk_diarize_fold_grouped  sdk_diarize_reconstruct_grouped  sdk_diarize_first_seen  sdk_diarize_renumber
 *                                                                                                       speaker diarization (diarize.py)
 *     sdk_score_reference  sdk_score_cooccur  sdk_score_map                                             diarization error rate against a reference (score.py)
 *     sdk_score_uem  sdk_score_durations  sdk_score_jaccard                                             evaluation maps (UEM) and the Jaccard error rate (score.py)
 *     sdk_words_attribute  sdk_words_cooccur                                                            speaker-attributed transcripts: words onto the diarization
 *                                                                                                       frames, and the word-level error rate's tables (words.py)
 *     sdk_samples_runs_workspace_bytes  sdk_samples_runs  sdk_samples_score_workspace_bytes  sdk_samples_score
 *                                                                                                       speaker samples: each speaker's solo runs on the diarization
 *                                                                                                       frames, and the scores of the clips cut from them (samples.py)
 *     sdk_smooth_turns_workspace_bytes  sdk_smooth_turns                                                smoothing of the diarized turns: short pauses filled, short
 *                                                                                                       runs dropped, on the diarization frames (smooth.py)
 *     sdk_fuse_masks  sdk_fuse_cooccur  sdk_fuse_labels  sdk_fuse_vote                                  fusing several diarizations of a recording: DOVER-Lap label
 *                                                                                                       mapping and weighted voting (fuse.py)
 *     sdk_plda_transform  sdk_vbx_workspace_bytes  sdk_vbx  sdk_vbx_centroids                           VBx clustering (plda.py, cluster.vbx_cluster)
 *     sdk_vbx_hmm_workspace_bytes  sdk_vbx_hmm                                                          VBx with its HMM, rows in time order (loop_prob > 0)
 *     sdk_plda_fit_stats_workspace_bytes  sdk_plda_fit_stats  sdk_plda_project                          training the VBx PLDA from labelled rows (plda.fit)
 *     sdk_cohort_stats_workspace_bytes  sdk_cohort_stats  sdk_affinity_topk_snorm                       adaptive score normalisation (snorm.py)
 *     sdk_plda_enroll_workspace_bytes  sdk_plda_enroll  sdk_plda_score_workspace_bytes  sdk_plda_score_topk    PLDA log-likelihood-ratio scoring of
 *                                                                                                       windows against enrolled speakers (plda_score.py)
 *     sdk_trial_hist                                                                                    verification trials: two-class score histograms for EER, minDCF
 *                                                                                                       and the DET curve (trials.py)
 *     sdk_trial_calib_workspace_bytes  sdk_trial_calib                                                  verification trials: the sums of the logistic calibration
 *                                                                                                       objective, its gradient and Hessian (trials.py)
 *     sdk_trial_hist_snorm                                                                              verification trials on the cohort-normalised (AS-norm) scale: the
 *                                                                                                       histograms that tune SDK_COHORT_THRESHOLD (trials_snorm.py)
 *     sdk_kmeans_rows_workspace_bytes  sdk_kmeans_rows                                                  spherical k-means on unit rows (cluster.kmeans_cluster)
 *     sdk_stream_state_bytes  sdk_stream_reset  sdk_stream_step  sdk_stream_flush  sdk_stream_centroids streaming diarization: online speaker tracking (stream.py)
 * BUILDING BLOCKS AND KNOBS - exported for the parity tests and the A/B tools, free to change between rounds, not for binding:
 *     sdk_conv_gemm*  sdk_colstats_finish  sdk_res2net_chain*  sdk_se_*  sdk_asp_*  sdk_rows_fc  sdk_rows_fc_path  (pieces of sdk_ecapa_forward)
 *     sdk_resnet_conv2d  sdk_resnet_pool  (pieces of sdk_resnet_forward)  sdk_resnet_masked_pool  (piece of sdk_resnet_forward_masked)
 *     sdk_sincnet_frontend  sdk_bilstm_layer  (pieces of sdk_segmentation_forward)
 *     sdk_set_option  sdk_set_gemm_variant  sdk_profile_begin / _end  sdk_debug_set_ptr  sdk_affinity_plan*  sdk_affinity_block_plan*  sdk_affinity_matvec_plan  sdk_conv_gemm_hp  sdk_resample_plan
 *     sdk_seg_mean_hp  sdk_se_apply_hp  sdk_asp_stats_hp  sdk_asp_pool_hp  (the precise mode's sweeps, pieces of its forwards)
 *     sdk_allgather  sdk_laplacian_topk_workspace_bytes  sdk_laplacian_topk        k5 / k6 drivers for a non-Python host (the library holds no
 *                                                                                     communicator: the caller passes its ncclComm_t; the Python
 *                                                                                     host layer uses torch.distributed, dist.py / cluster.py)
 */
#ifndef SDK_HIP_H
#define SDK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDK_ABI_VERSION 4   /* 2: sdk_ecapa_desc.precision (round 3); 3: sdk_fbank_windows + sdk_ingest_* (round 4); 4: precision 2, sdk_fbank_fmt, SDK_GEMM_F16, lazy ingest slots (round 5); still 4 with sdk_cohort_stats* and sdk_affinity_topk_snorm, and with sdk_ecapa_forward_masked, sdk_ecapa_masked_workspace_bytes, sdk_asp_stats_masked_fmt and sdk_asp_pool_masked_fmt, and with sdk_score_reference, sdk_score_cooccur and sdk_score_map, and with sdk_plda_enroll* and sdk_plda_score*, and with sdk_trial_hist, sdk_trial_calib* and sdk_trial_hist_snorm, and with sdk_words_attribute and sdk_words_cooccur, and with sdk_samples_runs* and sdk_samples_score*, and with sdk_score_uem, sdk_score_durations and sdk_score_jaccard, and with sdk_smooth_turns*, and with sdk_fuse_masks, sdk_fuse_cooccur, sdk_fuse_labels and sdk_fuse_vote: new exports only, no struct or existing signature changes, no caller of version 4 breaks */

typedef struct sdk_ctx sdk_ctx;

typedef struct sdk_device_info {
  int device;
  int compute_units;
  int clock_khz;
  int wavefront_size;
  uint64_t hbm_bytes;
  char name[128];
  char arch[64];
} sdk_device_info;

/* ---- lifecycle (replaces Backend.__init__ of a reference backend: base.py:291-293) ---- */
int sdk_abi_version(void);
int sdk_init(int device, sdk_ctx** out);
int sdk_shutdown(sdk_ctx* ctx);
const char* sdk_last_error(void);
int sdk_get_device_info(sdk_ctx* ctx, sdk_device_info* out);
/* Device memory for hosts that bring no allocator (a C / C++ binding; the torch-free Python path lite.py that serves a one-recording CLI
 * call without the 0.8-s `import torch` - the reference constructs its backend fresh in every process, base.py:291-293).  sdk_memcpy: kind 1 =
 * host -> device, 2 = device -> host, 3 = device -> device; ordered on `stream` and COMPLETE when the call returns (the one entry point that
 * synchronises, next to sdk_stream_synchronize).  Pointers from any other allocator of the same HIP runtime (torch tensors) work equally. */
int sdk_device_malloc(sdk_ctx* ctx, size_t bytes, void** out);
int sdk_device_free(sdk_ctx* ctx, void* p);
int sdk_memcpy(sdk_ctx* ctx, void* dst, const void* src, size_t bytes, int kind, void* stream);
int sdk_stream_synchronize(sdk_ctx* ctx, void* stream);
/* A/B and test knobs: "res2net_chain_fusion" (1 default / 0 = seven conv_gemm launches), "res2net_packed_weights" (1 default /
 * 0 = the chain ignores the blob's optional fragment-ordered weight copies, ecapa_layout.h EL_CHAINPACK), "res2net_two_per_cu" (1 default /
 * 0 = 8-wave workgroups, one segment per CU), "asp_packed_weights"
 * (likewise for the ASP logit weights, EL_ASP_W2PACK), "asp_per_segment"
 * (1 default / 0 = one workgroup per (segment, 128 channels)), "h_kblocked" (1 default / 0 = sdk_ecapa_forward keeps the MFA output row-major
 * instead of K-blocked, SDK_GEMM_C_KBLOCKED below), "affinity_fast_path" / "affinity_variant" /
 * "affinity_boundary_penalty" (k = 1 affinity kernel selection and work split), "chol_pivot_rtol_ppb" / "chol_shift_ppb"
 * (sdk_chol_inverse, below), "matvec_variant" (0 default: persistent row-group kernel / 1 = round 1's
 * kernel; sums differ in the last bits only), "gemm_variant" (see sdk_set_gemm_variant).  Results do not depend on them.
 * NOT a knob - a numerical contract: "precision" 0 (default: bf16 operands, bf16 layer-boundary storage; PCM -> score within ~4e-3 of
 * the fp32 model, ~9e-4 with the host's bias correction) / 1 (fp16 hi+lo planes, three MFMAs per product: within 1e-5, ~3x the GEMM time) /
 * 2 (round 5: ONE fp16 plane - the default schedule with fp16 instead of bf16 storage and MFMA operands: ~5e-4, ~1.7e-4 bias-corrected, ~0.96x the
 * default's throughput; the ECAPA-TDNN and x-vector forwards).  The OPTION is only the default of the entry points that have no format argument: the
 * output format of sdk_fbank / sdk_fbank_windows (bf16 / planes / fp16; sdk_fbank_fmt takes it per call) and the element format the stand-alone
 * sweeps (sdk_se_gate_residual, sdk_asp_stats, sdk_asp_pool, sdk_asp_fused*, sdk_res2net_chain) read and write; each of them has a _fmt sibling
 * that takes the format (0: bf16, 2: fp16) per call instead.  The forwards take the contract from the
 * weight blob's descriptor (sdk_ecapa_desc.precision), sdk_conv_gemm from its flags (SDK_GEMM_F16): per call, no shared state. */
int sdk_set_option(sdk_ctx* ctx, const char* name, int value);
/* Diagnostics: "stamps" = device buffer [workgroups][64] of uint64 that the affinity kernel (tools/aff_timeline.py) and the
 * Res2Net chain (tools/res2net_timeline.py) fill with in-kernel wall-clock stamps; "gemm_clock" = EXACTLY [4096][2] uint64 {shader cycles, 100 MHz ticks} of each
 * conv_gemm256 workgroup's lifetime (bench.py: the clock the chip holds inside the dominant kernel; workgroups >= 4096 do not write);
 * "gemm_stamps" = EXACTLY [4096] uint64 wall-clock stamps of conv_gemm256 workgroup 0's tile phases (tools/gemm_timeline.py;
 * a buffer of its own - the clock probe never writes outside its [4096][2]).  NULL (default) = off. */
int sdk_debug_set_ptr(sdk_ctx* ctx, const char* name, void* device_ptr);

/* ---- measurement: per-kernel-family HIP-event timing on the launch stream (bench.py roofline) -- */
enum {
  SDK_K_CONV_GEMM = 0, SDK_K_SE_GATE, SDK_K_ASP_STATS, SDK_K_ROWS_FC, SDK_K_ASP_POOL, SDK_K_FBANK_TILE,
  SDK_K_FBANK_NORM, SDK_K_L2NORM, SDK_K_AFF_COARSE, SDK_K_AFF_RESCORE, SDK_K_AFF_RESCAN, SDK_K_COPY,
  SDK_K_AFF_MATVEC, SDK_K_CONV_GEMM256, SDK_K_ASP_FUSED, SDK_K_RES2NET, SDK_K_RESAMPLE, SDK_K_CONV_GEMM_HP,
  SDK_K_RESNET_CONV, SDK_K_RESNET_STEM, SDK_K_RESNET_POOL, SDK_K_COUNT
};
typedef struct sdk_profile_report {
  int32_t launches[24];
  double ms[24];          /* summed device time of the family's launches */
  double flops[24];       /* executed flops as launched (2*M*N*K for GEMMs) */
  double bytes[24];       /* compulsory bytes as launched (inputs once + outputs once) */
} sdk_profile_report;
int sdk_profile_begin(sdk_ctx* ctx);
int sdk_profile_end(sdk_ctx* ctx, sdk_profile_report* out);   /* synchronises the device */

/* ---- k1: fbank.  Input contract = audio_profiles.py:25-29 (16 kHz mono s16le). --------
 * pcm   [B, S] int16 (device)          T = 1 + S/160 frames per segment
 * tabs  packed DFT/mel tables from sdk_fbank_tables_bytes()/sdk_fbank_tables_fill(), copied to
 *       the device by the caller (16-byte aligned)
 * ws    caller scratch of sdk_fbank_workspace_bytes(B, S)
 * feats [B*T, ldf] bf16, channels 0..79 = mean-normalised log-mel, 80..ldf-1 = 0 (ldf >= 80)
 *       precise mode ("precision" 1): fp16 planes, hi in columns [0, ldf/2), lo in [ldf/2, ldf), channels >= 80 of each zero
 *       (ldf/2 >= 80, ldf % 16 == 0); the DFT then runs on fp16 MFMAs with an fp16 hi+lo table (the folded int16 samples split exactly in
 *       fp16 too: three MFMAs per product)
 */
size_t sdk_fbank_tables_bytes(void);
int sdk_fbank_tables_fill(void* host_dst, size_t bytes);          /* HOST buffer */
size_t sdk_fbank_workspace_bytes(int B, int S);                    /* fp32 log-mel scratch */
int sdk_fbank(sdk_ctx* ctx, const int16_t* pcm, int B, int S, const void* tabs,
              uint16_t* feats, int ldf, void* ws, size_t ws_bytes, void* stream);
/* The same, with the windows cut ON THE DEVICE from ONE resident recording (the boundary hands a backend a path and segments,
 * base.py:130-151; the reference cuts with ffmpeg per segment list, speechmatics_backend.py:231-281): samples [n_samples] int16 (device),
 * starts [B] int32 (device) = first sample of every window, each inside the recording; window b = samples[starts[b] .. starts[b] + S), samples
 * past the recording's end read as zero.  Bit-identical to sdk_fbank on the materialised [B, S] windows; the overlapping windows (2x the
 * samples at hop 1 s / window 2 s) never exist on the host and never cross PCIe.  n_samples < 2^31. */
int sdk_fbank_windows(sdk_ctx* ctx, const int16_t* samples, int64_t n_samples, const int32_t* starts, int B, int S, const void* tabs,
                      uint16_t* feats, int ldf, void* ws, size_t ws_bytes, void* stream);
/* Both with the output format as an ARGUMENT (precision 0 / 1 / 2, see sdk_set_option) instead of the context's "precision" option (round 5): a
 * host that runs several numerical contracts on one device - two engines, two threads - then shares no mutable state through the library.
 * sdk_ecapa_forward / sdk_xvector_forward take the contract from their descriptor alone; the features must have been written in that format. */
int sdk_fbank_fmt(sdk_ctx* ctx, const int16_t* pcm, int B, int S, const void* tabs, uint16_t* feats, int ldf, void* ws, size_t ws_bytes, int precision,
                  void* stream);
int sdk_fbank_windows_fmt(sdk_ctx* ctx, const int16_t* samples, int64_t n_samples, const int32_t* starts, int B, int S, const void* tabs,
                          uint16_t* feats, int ldf, void* ws, size_t ws_bytes, int precision, void* stream);

/* ---- ingest: host audio -> HBM, staged through pinned memory on a copy stream of its own, `depth`-deep (2 = double-buffered) so that the
 *      upload of recording i + 1 runs under the forward pass of recording i.  A slot = pinned host buffers for int16 samples and
 *      int32 window starts + their device twins, allocated on the slot's first use at the size of that upload (max_samples / max_windows bound it).
 *   sdk_ingest_acquire : next slot (ring order); *pinned_samples / *pinned_starts are HOST pointers the caller fills (a file reader can
 *                        read straight into them: no second host copy).  Fails if that slot was committed and never released; a slot
 *                        acquired and never committed (its filler gave up) is handed out again when the ring comes round.
 *   sdk_ingest_commit  : validates the start table (every start inside [0, n_samples)), enqueues the uploads on the copy stream - behind the
 *                        slot's previous consumer, without blocking the host - and makes `compute_stream` wait for them;
 *                        *dev_samples / *dev_starts are DEVICE pointers for sdk_fbank_windows (any sub-range of the table may be launched)
 *   sdk_ingest_submit  : acquire + memcpy from pageable host memory + commit
 *   sdk_ingest_release : call after the LAST kernel reading the slot has been enqueued on compute_stream; the slot's next upload waits for it
 *   sdk_ingest_copy_ms : duration / bytes of the slot's last upload (HIP events on the copy stream; synchronises with that upload) */
typedef struct sdk_ingest sdk_ingest;
int sdk_ingest_create(sdk_ctx* ctx, int64_t max_samples, int max_windows, int depth, sdk_ingest** out);
int sdk_ingest_destroy(sdk_ingest* ing);
int sdk_ingest_acquire(sdk_ingest* ing, int* ticket, int16_t** pinned_samples, int32_t** pinned_starts);   /* = _sized(max_samples, max_windows) */
/* a slot's buffers are allocated on its first use and sized to what it is asked to take (grown when a larger upload arrives; where the host
 * refuses page-locked memory the slot stages through ordinary memory): max_samples / max_windows of sdk_ingest_create are upper bounds only */
int sdk_ingest_acquire_sized(sdk_ingest* ing, int64_t n_samples, int n_windows, int* ticket, int16_t** pinned_samples, int32_t** pinned_starts);
int sdk_ingest_slot_info(sdk_ingest* ing, int slot, int64_t* cap_samples, int* pinned);
int sdk_ingest_commit(sdk_ingest* ing, int ticket, int64_t n_samples, int n_windows, int window_len, void* compute_stream,
                      const int16_t** dev_samples, const int32_t** dev_starts);
int sdk_ingest_submit(sdk_ingest* ing, const int16_t* host_samples, int64_t n_samples, const int32_t* host_starts, int n_windows,
                      int window_len, void* compute_stream, int* ticket, const int16_t** dev_samples, const int32_t** dev_starts);
int sdk_ingest_release(sdk_ingest* ing, int ticket, void* compute_stream);
int sdk_ingest_copy_ms(sdk_ingest* ing, int ticket, float* ms, double* bytes);

/* ---- k2 building blocks (ECAPA-TDNN forward; behind EmbeddingBackend.enroll_speaker /
 *      identify_speaker, base.py:107-151) -------------------------------------------------- */

#define SDK_GEMM_RELU 1u
#define SDK_GEMM_TANH 2u
/* K-BLOCKED activation layout (round 4): a [M, cols] bf16 matrix stored as [cols / 64][M][64] - element (m, c) at (c / 64) * M * 64 + m * 64 + c % 64 -
 * so that the 128-byte row piece a GEMM K-step (or an ASP channel block) takes from a row lies next to its neighbours' instead of `ld` apart.  Made for
 * the widest activation of the forward, the MFA output h [B*T, 3072]: written once (C_KBLOCKED: plain-layer shape of the 256^2 kernel only, ldc ignored),
 * read by the skinny attention-hidden GEMM (A_KBLOCKED: taps == 1, lda ignored; runs on the 128^2 kernel) and by sdk_asp_fused_kblocked. */
#define SDK_GEMM_A_KBLOCKED 4u
#define SDK_GEMM_C_KBLOCKED 8u
#define SDK_GEMM_F16 16u          /* A, W and the 2-byte outputs are fp16 (IEEE binary16) instead of bf16: the single-plane fp16 contract (precision 2) */

/* Dilated 1-D convolution over frames as one MFMA GEMM:
 *   pre[m, n] = bias[n] + ubias[m / T, n] + sum_{j<taps} sum_{c<Cin}
 *                 A[seg(m)*T + reflect(t(m) + (j - taps/2)*dil), c] * W[n, j*Cin + c]
 *   v = RELU? max(pre,0) : pre;  v = v*scale[n] + shift[n];  v = TANH? tanh(v) : v
 *   C[m,n] = bf16(v);  C32[m,n] = v;  S[m,n] = bf16(float(bf16(v)) + float(X2[m,n]))
 * Requirements: Cin % 64 == 0, N % 128 == 0, T > (taps/2)*dil, M % T == 0.
 * Any of bias/scale/shift/ubias/C/C32/X2+S may be NULL. */
typedef struct sdk_conv_gemm_args {
  const uint16_t* A;  int64_t lda;
  const uint16_t* W;               /* [N, taps*Cin] bf16, K contiguous */
  uint16_t* C;        int64_t ldc;
  float* C32;         int64_t ldc32;
  const float* bias;  const float* scale;  const float* shift;
  const float* ubias; int64_t ldub;
  const uint16_t* X2; int64_t ldx2;
  uint16_t* S;        int64_t lds;
  int M, N, Cin, taps, dil, T;
  uint32_t flags;
  /* optional fused per-segment column statistics of the stored output (SE squeeze means, ASP global
   * context): stats_mode 1 = sum, 2 = sum and sum of squares; stats_part = scratch of
   * sdk_conv_gemm_stats_bytes(); finish with sdk_colstats_finish().  Only where
   * sdk_conv_gemm_stats_fusable(M, N, T) is true. */
  int32_t stats_mode;
  float* stats_part;
  /* optional addend of the A operand, same rows/row map/channels: the GEMM consumes bf16(A + A2)
   * (Res2Net: y_{c-1} + u_c formed on the way into LDS instead of round-tripping through HBM) */
  const uint16_t* A2; int64_t lda2;
  /* > 0: the taps are PACKED along K: W is [N, round_up(taps * tap_pack, 64)] (tap-major, tap_pack channels per tap, zero K padding),
   * Cin == tap_pack (a multiple of 8, not of 64): the first layer's 5 x 80 mel channels take 7 K-steps of 64 instead of 5 x 128 -> 10 */
  int32_t tap_pack;
  int32_t reserved;
} sdk_conv_gemm_args;
int sdk_conv_gemm(sdk_ctx* ctx, const sdk_conv_gemm_args* a, void* stream);
size_t sdk_conv_gemm_stats_bytes(int M, int N, int mode);
int sdk_conv_gemm_stats_fusable(int M, int N, int T);
/* out: mode 1 -> [B, N] per-segment column means; mode 2 -> [B, 2N] mean | sqrt(max(var, 1e-12)) */
int sdk_colstats_finish(sdk_ctx* ctx, const float* stats_part, int M, int N, int T, int mode, float* out, void* stream);
/* Tuning knob (A/B measurements): 1 = 128x128 register-staged tile, 2 = 256x256 LDS-DMA tile where
 * the shape allows it (default; also settable once via $SDK_GEMM_VARIANT). */
int sdk_set_gemm_variant(int variant);

/* Squeeze-excitation gate + residual, one workgroup per segment:
 *   mean[c] = (1/T) sum_t z[b,t,c];  h = relu(W1 mean + b1);  g = sigmoid(W2 h + b2)
 *   out[b,t,c] = bf16(g[c]*z[b,t,c] + x[b,t,c])
 * w1t [C, Cse] fp32 (transposed), w2t [Cse, C] fp32 (transposed).  C % 8 == 0 and (C/8) | 256, Cse | 256.
 * With a workspace the work is split into a mean sweep, two batched FCs on the fp32 matrix pipe and an
 * apply sweep (same arithmetic, weights read once per 32 segments). */
/* Res2Net chain of one block fused per segment (T <= sdk_res2net_chain_max_frames(), 128-channel sub-bands):
 *   R[:, 128c : 128(c+1)] = y_c,  y_1 = TDNN_0(U chunk 1),  y_c = TDNN_{c-1}(bf16(U chunk c + y_{c-1})),  c = 2..nconv
 * W/bias/scale/shift: HOST arrays of nconv device pointers (W[i]: bf16 [128][3*128]).  Bit-identical to the
 * same chain expressed as nconv sdk_conv_gemm launches.  R may be U itself (in place: a segment's chunk c has been
 * read before y_c is written over it), which also leaves chunk 0 where the next layer expects it. */
int sdk_res2net_chain_max_frames(void);
int sdk_res2net_chain(sdk_ctx* ctx, const uint16_t* U, int64_t ldu, uint16_t* R, int64_t ldr, const uint16_t* const* W,
                      const float* const* bias, const float* const* scale, const float* const* shift, int nconv,
                      int B, int T, int dil, void* stream);
/* the same with the element format of U, R and W as an argument (0: bf16, 2: fp16) instead of the context's default */
int sdk_res2net_chain_fmt(sdk_ctx* ctx, const uint16_t* U, int64_t ldu, uint16_t* R, int64_t ldr, const uint16_t* const* W,
                          const float* const* bias, const float* const* scale, const float* const* shift, int nconv,
                          int B, int T, int dil, int precision, void* stream);
size_t sdk_se_workspace_bytes(int B, int C, int Cse);   /* fp32 [B,C] means + [B,Cse] hidden + [B,C] gates */
int sdk_se_gate_residual(sdk_ctx* ctx, const uint16_t* z, int64_t ldz, const uint16_t* x, int64_t ldx,
                         const float* w1t, const float* b1, const float* w2t, const float* b2,
                         uint16_t* out, int64_t ldo, int B, int T, int C, int Cse,
                         const float* mean_in,      /* optional [B, C] squeeze means already computed (fused GEMM epilogue) */
                         void* ws, size_t ws_bytes, void* stream);   /* ws may be NULL: one-kernel-per-segment form */
int sdk_se_gate_residual_fmt(sdk_ctx* ctx, const uint16_t* z, int64_t ldz, const uint16_t* x, int64_t ldx,
                             const float* w1t, const float* b1, const float* w2t, const float* b2,
                             uint16_t* out, int64_t ldo, int B, int T, int C, int Cse, const float* mean_in,
                             void* ws, size_t ws_bytes, int precision, void* stream);   /* z, x, out: 0 bf16, 2 fp16 */

/* Attentive statistics pooling pieces.
 *   sdk_asp_stats : ctx[b, 0:C] = mean_t h, ctx[b, C:2C] = sqrt(max(var_t h, 1e-12))   fp32
 *   sdk_rows_fc   : out[b, j] = act(bias[j] + sum_c (in[b,c]*in_scale[c]+in_shift[c]) * wt[c, j])
 *                   (wt [Cin, Nout] fp32 transposed; act 0 none, 1 relu, 2 sigmoid)
 *   sdk_asp_pool  : softmax over t of logits[b,t,c] -> weighted mean / std of h -> pooled[b, 0:C | C:2C]
 */
int sdk_asp_stats(sdk_ctx* ctx, const uint16_t* h, int64_t ldh, int B, int T, int C, float* out_ctx, void* stream);
/* the same with the element format of h as an argument (0: bf16, 2: fp16) instead of the context's default - per call, like sdk_fbank_fmt */
int sdk_asp_stats_fmt(sdk_ctx* ctx, const uint16_t* h, int64_t ldh, int B, int T, int C, float* out_ctx, int precision, void* stream);
int sdk_rows_fc(sdk_ctx* ctx, const float* in, int64_t ldin, const float* in_scale, const float* in_shift,
                const float* wt, const float* bias, float* out, int64_t ldout,
                int B, int Cin, int Nout, int act, void* stream);
/* which kernel sdk_rows_fc launches for these arguments (host only: no context, nothing is launched; the pointers are looked at for their
 * alignment, never read): 0 the plain kernel (any shape), 1 the matrix-pipe kernel with 4 K-slices (Cin % 32 == 0), 2 and 3 the one with
 * 16 K-slices (Cin % 128 == 0, Cin >= 2048), 3 when it also fetches the weights as 16-byte rows (Nout % 32 == 0, wt 16-byte aligned).
 * 1..3 need ldin % 4 == 0, `in` 16-byte aligned and, with an input affine (has_affine != 0), Cin <= 8192; everything else is path 0. */
int sdk_rows_fc_path(const float* in, int64_t ldin, int has_affine, const float* wt, int Cin, int Nout);
int sdk_asp_pool(sdk_ctx* ctx, const float* logits, int64_t ldl, const uint16_t* h, int64_t ldh,
                 int B, int T, int C, float* pooled, void* stream);
int sdk_asp_pool_fmt(sdk_ctx* ctx, const float* logits, int64_t ldl, const uint16_t* h, int64_t ldh,
                     int B, int T, int C, float* pooled, int precision, void* stream);   /* h: 0 bf16, 2 fp16 */
/* Fused form of (attention-logit GEMM + sdk_asp_pool) for T <= sdk_asp_fused_max_frames(): the fp32
 * logits stay in accumulator registers.  ah [B*T, A=128] bf16 attention hidden, w2 [C, A] bf16, b2 [C]. */
int sdk_asp_fused_max_frames(void);
int sdk_asp_fused(sdk_ctx* ctx, const uint16_t* ah, int64_t ldah, const uint16_t* w2, const float* b2,
                  const uint16_t* h, int64_t ldh, int B, int T, int C, int A, float* pooled, void* stream);
int sdk_asp_fused_fmt(sdk_ctx* ctx, const uint16_t* ah, int64_t ldah, const uint16_t* w2, const float* b2,
                      const uint16_t* h, int64_t ldh, int B, int T, int C, int A, float* pooled, int precision, void* stream);   /* ah, w2, h: 0 bf16, 2 fp16 */
/* The same with h in the K-blocked layout [C / 64][B*T][64] (SDK_GEMM_C_KBLOCKED above).  Only the per-segment form reads it: where
 * sdk_asp_kblocked_ok(ctx, T, C) is 0 (short or long windows, option asp_per_segment off) the call is an error and the caller keeps h row-major.
 * Bit-identical to sdk_asp_fused on the same values. */
int sdk_asp_kblocked_ok(sdk_ctx* ctx, int T, int C);
int sdk_asp_fused_kblocked(sdk_ctx* ctx, const uint16_t* ah, int64_t ldah, const uint16_t* w2, const float* b2,
                           const uint16_t* h, int B, int T, int C, int A, float* pooled, void* stream);
int sdk_asp_fused_kblocked_fmt(sdk_ctx* ctx, const uint16_t* ah, int64_t ldah, const uint16_t* w2, const float* b2,
                               const uint16_t* h, int B, int T, int C, int A, float* pooled, int precision, void* stream);

/* ---- PRECISE MODE (sdk_set_option "precision" 1; north_star: cosine scores within 1e-5 of the fp32 model, which bf16 operands miss
 *      by 4e-3 - profiles/r03_error_budget.md).  Tensors the default mode rounds to bf16 travel as fp16 hi + lo PLANES: a [rows, C]
 *      activation is [rows, ld] fp16, hi values in columns [0, C), lo values `lo` columns to the right, x = float(hi) + float(lo);
 *      the lo values are stored times 2^11 (x = float(hi) + float(lo) / 2048: always in the normal fp16 range of their hi);
 *      GEMM weights are a 256-byte header (float 1 / 2^s) + [2][N][K] fp16 planes (hi, lo) of 2^s * W, s per layer
 *      (weights_pack.hp_weight_planes); every product runs as three fp16 MFMAs (hi.hi + lo.hi + hi.lo), fp32 accumulate, fp32 epilogue
 *      with libm tanh.  Same operator as sdk_conv_gemm otherwise (Cin % 32 == 0, N % 128 == 0). */
typedef struct sdk_conv_gemm_hp_args {
  const uint16_t* A;  int64_t lda, a_lo;
  const uint16_t* W;                       /* the weight slot: header + [2][N][taps*Cin] fp16 planes */
  uint16_t* C;        int64_t ldc, c_lo;   /* planes out (may be NULL) */
  float* C32;         int64_t ldc32;       /* fp32 out (may be NULL) */
  const float* bias;  const float* scale;  const float* shift;
  const float* ubias; int64_t ldub;
  const uint16_t* X2; int64_t ldx2, x2_lo; /* S = planes(v + X2) (Res2Net running sum; may be NULL) */
  uint16_t* S;        int64_t lds, s_lo;
  int M, N, Cin, taps, dil, T;
  uint32_t flags;
} sdk_conv_gemm_hp_args;
int sdk_conv_gemm_hp(sdk_ctx* ctx, const sdk_conv_gemm_hp_args* a, void* stream);
/* The precise mode's HBM-bound sweeps on plane pairs (pieces of its forwards, exported for the parity tests).  A plane operand [B*T, C] is
 * (pointer, ld, lo): hi values at p[row * ld + c], lo values `lo` columns to the right; C % 8 == 0, ld % 8 == 0, lo % 8 == 0, lo >= C,
 * ld >= lo + C, pointer 16-byte aligned - anything else is refused before a launch.  All arithmetic fp32.
 *   sdk_seg_mean_hp:  out [B, C] fp32 = mean over the T frames of each segment (the SE squeeze)
 *   sdk_se_apply_hp:  out planes = gate[b, c] * z + x  (gate [B, C] fp32; the pair store saturates at +-65504)
 *   sdk_asp_stats_hp: out [B, 2C] fp32 = mean | sqrt(max(var, 1e-12)) over frames
 *   sdk_asp_pool_hp:  pooled [B, 2C] fp32 = softmax-over-frames weighted mean | std of h, logits [B*T, ldl] fp32 (ldl >= C) */
int sdk_seg_mean_hp(sdk_ctx* ctx, const uint16_t* z, int64_t ldz, int64_t z_lo, int B, int T, int C, float* out, void* stream);
int sdk_se_apply_hp(sdk_ctx* ctx, const uint16_t* z, int64_t ldz, int64_t z_lo, const uint16_t* x, int64_t ldx, int64_t x_lo,
                    const float* gate, uint16_t* out, int64_t ldo, int64_t o_lo, int B, int T, int C, void* stream);
int sdk_asp_stats_hp(sdk_ctx* ctx, const uint16_t* h, int64_t ldh, int64_t h_lo, int B, int T, int C, float* out, void* stream);
int sdk_asp_pool_hp(sdk_ctx* ctx, const float* logits, int64_t ldl, const uint16_t* h, int64_t ldh, int64_t h_lo, int B, int T, int C,
                    float* pooled, void* stream);

/* Whole forward: feats [B*T, ldf] bf16 -> raw embeddings emb [B, 192] fp32.
 * `wblob` is the packed device weight blob and `wdesc` (HOST) its offset table, both produced by
 * the host packer (weights_pack.py); `ws` is caller-owned scratch of sdk_ecapa_workspace_bytes(). */
typedef struct sdk_ecapa_desc {
  int32_t n_mels_padded, channels, sub_channels, scale, se_channels, attn_channels, mfa_channels, embed_dim;
  int32_t n_blocks, kernel0;
  int32_t dilation[4];
  int32_t precision;       /* 0: bf16 operand blob (default mode); 1: fp16 hi+lo plane blob (precise mode: feats are planes [B*T, ldf] with
                              the lo plane ldf/2 columns to the right, n_mels_padded = 96); must equal the context's "precision" option */
  int32_t blk0_tap_pack;   /* default mode: > 0 = the first layer's weight slot is packed along K (sdk_conv_gemm_args.tap_pack), value = mel channels per
                              tap (80); 0 = [C][kernel0 * n_mels_padded] */
  /* byte offsets into wblob; -1 = absent.  Layout of the index space: see weights_pack.py */
  int64_t off[256];
} sdk_ecapa_desc;
size_t sdk_ecapa_workspace_bytes(const sdk_ecapa_desc* d, int B, int T);
int sdk_ecapa_forward(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* wdesc,
                      const uint16_t* feats, int ldf, int B, int T,
                      void* ws, size_t ws_bytes, float* emb, void* stream);

/* Calibration pass for the host's BIAS CORRECTION of the bf16 weight rounding (weights_pack.bias_corrections): the same
 * forward (Res2Net chain unfused), additionally writing the per-segment mean | std ([B, 2 C_l] fp32, sdk_asp_stats layout) of the INPUT of every
 * corrected GEMM layer into `calib`, slots in this order: per block {tdnn1 [C], Res2Net conv 0..scale-2 [sub_channels each], tdnn2 [C]}, then
 * MFA [mfa_channels], ASP hidden [mfa_channels]; sdk_ecapa_calib_floats() = total floats.  Default-mode blobs only. */
size_t sdk_ecapa_calib_floats(const sdk_ecapa_desc* d, int B);
int sdk_ecapa_forward_calib(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* wdesc, const uint16_t* feats, int ldf, int B, int T,
                            void* ws, size_t ws_bytes, float* emb, float* calib, void* stream);

/* ---- The ECAPA-TDNN forward with S MASKED attentive statistics poolings per chunk (diarize.py with ecapa_diar.EcapaEmbedder: one per local
 *      speaker of a 10-s chunk, so that diarization's centroids live in the space of sdk_ecapa_forward, the enrolled profiles and the AS-norm
 *      cohort).  Parity with SpeechBrain / PyAnnote is unpinned, as everywhere here: THIS RULE is what the tests pin.
 *   For a chunk b the trunk of sdk_ecapa_forward - blk0, the SE-Res2Net blocks and MFA, up to h [T, Cm] - runs ONCE, bit for bit the values
 *   sdk_ecapa_forward computes at the same (B, T) (one function serves both); the SE squeeze stays over all T frames.  The mask enters at the
 *   pooling only.  For each slot s < S, w = w[b][s][0..T) >= 0 (ANY non-negative weights, not only 0 / 1), v1 = sum_t w_t:
 *     context    mu_c = sum_t w_t h_tc / v1,  sd_c = sqrt(max(sum_t w_t (h_tc - mu_c)^2 / v1, 1e-12))   (the biased form and floor of sdk_asp_stats)
 *     ubias      = Wms [mu | sd] + b in fp32 (sdk_rows_fc), one row per (b, s)
 *     hidden     a_t = tanh(BN(relu(h_t Wh + ubias))), stored in the 2-byte format
 *     logits     l_tc = a_t . W2_c + b2_c, fp32
 *     attention  m_c = max over {t : w_t > 0} of l_tc,  e_tc = w_t exp(l_tc - m_c),  alpha_tc = e_tc / sum_t e_tc; a frame with w_t = 0 enters
 *                neither the maximum nor any sum
 *     pooled     wmu_c = sum_t alpha_tc h_tc,  wsd_c = sqrt(max(sum_t alpha_tc (h_tc - wmu_c)^2, 1e-12))
 *     embedding  pooled [b S + s] = wmu | wsd, then asp_bn and fc over the B S rows -> emb [B S, embed_dim]
 *   A row depends on its own weights only.  Rows with valid[b][s] == 0 are written as zeros and their weights are never used for a division.  A
 *   row with valid != 0 and v1 <= 0 is ZEROED (not refused: the weights are device memory), in the embeddings and in both building blocks.
 *   With w == 1 this is the pooling of sdk_ecapa_forward; with 0 / 1 weights SpeechBrain's masked AttentiveStatisticsPooling with that mask.
 *   fp32 arithmetic in two (statistics) and three (pooling) sweeps, every thread's frames in order, partial sums joined in a fixed order: results are
 *   bit-identical run to run, no float atomics.
 *   Schedule: trunk (h row-major), ONE sdk_asp_stats_masked launch for the B S rows, sdk_rows_fc, then per slot sdk_conv_gemm (hidden, the slot's
 *   ubias rows: ldub = S A) + sdk_conv_gemm (logits into one reused fp32 buffer) + sdk_asp_pool_masked, sdk_rows_fc over B S rows.
 *   Refused with a message: a precision-1 blob, S < 1 or S > 8, a null pointer, too small a workspace, T not above the receptive halo.
 *   Building blocks (fmt 0: bf16 elements, 2: fp16; 1 refused), any T >= 1:
 *   sdk_asp_stats_masked_fmt: h [B*T, ldh] (C % 8 == 0, ldh % 8 == 0, ldh >= C, 16-byte aligned) read once for all S slots -> out_ctx [B S][2 C] mean | std.
 *   sdk_asp_pool_masked_fmt:  the logits [B*T, ldl] fp32 of slot s (C % 64 == 0, ldl % 4 == 0, ldh % 8 == 0, 16-byte aligned pointers) -> rows b S + s of
 *                             pooled [B S][2 C]; the other rows are not touched. */
size_t sdk_ecapa_masked_workspace_bytes(const sdk_ecapa_desc* d, int B, int T, int S);
int sdk_ecapa_forward_masked(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf, int B, int T,
                             int S, const float* w /*[B][S][T]*/, const int32_t* valid /*[B][S]*/, void* ws, size_t ws_bytes,
                             float* emb /*[B S][embed_dim]*/, void* stream);
int sdk_asp_stats_masked_fmt(sdk_ctx* ctx, const uint16_t* h, int64_t ldh, int B, int T, int C, int S, const float* w, const int32_t* valid,
                             float* out_ctx /*[B S][2 C]*/, int precision, void* stream);
int sdk_asp_pool_masked_fmt(sdk_ctx* ctx, const float* logits, int64_t ldl, const uint16_t* h, int64_t ldh, int B, int T, int C,
                            int S, int s /*slot of these logits*/, const float* w, const int32_t* valid, float* pooled /*[B S][2 C]*/,
                            int precision, void* stream);

/* ---- x-vector (plain TDNN) forward - north_star names "ECAPA-TDNN/x-vector".  Frame layers l = 0..n_frame_layers-1:
 *      dilated conv (kernel[l], dilation[l], "same" length by segment-local reflection) -> ReLU -> BatchNorm(eval), bf16 layer-boundary
 *      storage, all on sdk_conv_gemm (layer 0 with its taps packed along K when the feature width is not a multiple of 64); then statistics
 *      pooling (mean | std over frames, sdk_asp_stats) and the embedding layer (fp32, sdk_rows_fc).  feats as sdk_fbank writes them
 *      ([B*T, ldf] bf16); emb [B, embed_dim] fp32 (pre-activation of the first segment layer, the usual x-vector).
 *      off[4 l + {0,1,2,3}] = W (bf16 [cout][K]), bias, BN scale, BN shift of frame layer l; off[60] = FC weight (fp32 [2 cout_last, embed_dim],
 *      transposed), off[61] = FC bias.  cout[] are multiples of 128 (pad a 1500-wide layer to 1536 with zero weights).
 *      off[62] = numerical contract of the blob: -1 / 0 = bf16 operands (default mode); 1 = PRECISE mode (round 4): W slots are sdk_conv_gemm_hp
 *      weight slots (header + fp16 hi / lo planes), feats are fp16 planes [B*T, ldf] (lo plane ldf/2 columns to the right, n_feats = 96 padded
 *      mel channels, no tap packing), the layers run on sdk_conv_gemm_hp and the pooling on the planes; 2 = ONE fp16 plane
 *      (round 5): the default layout with fp16 bits in the W slots and in feats (sdk_fbank_fmt(..., 2, ...)), sdk_conv_gemm with SDK_GEMM_F16.
 *      The blob decides per call; the context's "precision" option is not consulted. */
typedef struct sdk_xvector_desc {
  int32_t n_frame_layers, n_feats, embed_dim, first_tap_pack;
  int32_t kernel[8], dilation[8], cin[8], cout[8];
  int64_t off[64];
} sdk_xvector_desc;
size_t sdk_xvector_workspace_bytes(const sdk_xvector_desc* d, int B, int T);
int sdk_xvector_forward(sdk_ctx* ctx, const void* wblob, const sdk_xvector_desc* d, const uint16_t* feats, int ldf, int B, int T,
                        void* ws, size_t ws_bytes, float* emb, void* stream);

/* ---- ResNet34 forward (WeSpeaker ResNet34, the PyAnnote 3.1 speaker embedding; resnet.py).  The fbank matrix is a one-channel image of
 *      height F = n_feats (mel) and width T (frames): element (f, t) of segment b is feats[b*T + t, f].  Activations are channel-last
 *      [B][F][T][C] (2-byte elements), so the final map flattens to feature c*F4 + f with no transpose.
 *        stem      3x3 conv 1 -> width[0], stride 1, zero padding 1, folded BN, ReLU
 *        layer l   blocks[l] BasicBlocks of width[l]; the first block of layers 1..3 has stride 2 and a projection shortcut (1x1 conv + BN)
 *                  block: y = relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x)); output size o = (n - 1) / 2 + 1 per strided axis
 *        pooling   temporal statistics of the last map: mean | sqrt(unbiased var + 1e-7) over t, fp32 [B, 2 * width[3] * F4]
 *        seg_1     fp32 linear layer -> emb [B, embed_dim] (sdk_rows_fc)
 *      Every conv is one sdk_resnet_conv2d launch (implicit GEMM on the MFMA pipe; BN folded at pack time: its scale multiplies W in fp32
 *      before the rounding, its shift is the conv's bias).  A projection shortcut is extra K columns of its block's conv2, so conv2 +
 *      shortcut + add is one launch.  Layer-boundary storage in the blob's 2-byte format, fp32 accumulation, fp32 pooling and seg_1.
 *      Blob slots (256-byte aligned): conv i (i = 0 the stem, then conv1, conv2 of every block in order) has its weights at off[2 i]
 *      (2-byte bits [Cout][K], K tap-major: k = (3 dy + dx) Cin + c; the stem [width[0]][9]; a downsampling conv2 has K = 9 C + Cin, the
 *      shortcut's columns last) and its fp32 bias [Cout] at off[2 i + 1]; off[66] = seg_1 weight (fp32 [2 width[3] F4, embed_dim],
 *      transposed), off[67] = seg_1 bias.  precision: 0 = bf16 operands and storage, 2 = one fp16 plane (features from
 *      sdk_fbank_fmt(..., 2, ...)); the precise mode (1) is not built for this family and is refused.  The contract comes from the
 *      descriptor alone.  T >= 9 (the last map needs two frames for an unbiased variance). */
typedef struct sdk_resnet_desc {
  int32_t n_feats, embed_dim, precision, n_layers;   /* n_layers = 4 */
  int32_t blocks[4], width[4];                       /* widths 32 / 64 / 128 / 256 (each one of those), stem width = width[0] = 32 */
  int64_t off[72];
} sdk_resnet_desc;
size_t sdk_resnet_workspace_bytes(const sdk_resnet_desc* d, int B, int T);
int sdk_resnet_forward(sdk_ctx* ctx, const void* wblob, const sdk_resnet_desc* d, const uint16_t* feats, int ldf, int B, int T,
                       void* ws, size_t ws_bytes, float* emb, void* stream);
/* One 3x3 conv (zero padding 1) of the ResNet34 forward: y = act(x (*) W + bias [+ shortcut] [+ res]), fp32 epilogue, rounded once.
 *   x [B][F][T][Cin] channel-last (Cin = 1: the stem, x is the fbank matrix [B*T, ldx] read as the image (f, t) = x[b*T + t, f]);
 *   W [Cout][ldw] 2-byte bits, ldw = 9 Cin + Csc; y [B][Fo][To][Cout] with Fo = (F - 1) / stride + 1, To likewise.
 *   sc (or NULL): projection-shortcut input [B][Fsc][Tsc][Csc], read at (stride_sc fo, stride_sc to) against W's last Csc columns;
 *   res (or NULL): identity residual [B][Fo][To][Cout].  flags: SDK_GEMM_RELU, SDK_GEMM_F16.
 *   Cin in {1, 32, 64, 128, 256} (Cin = 1: Cout = 32, stride 1, no shortcut / residual), Cout in {32, 64, 128, 256}, stride 1 or 2. */
typedef struct sdk_resnet_conv_args {
  const uint16_t* x;
  const uint16_t* W;
  const float* bias;
  const uint16_t* sc;
  const uint16_t* res;
  uint16_t* y;
  int64_t ldx;
  int32_t B, F, T, Cin, Cout, stride;
  int32_t Csc, Fsc, Tsc, stride_sc;
  uint32_t flags;
  int32_t reserved;
} sdk_resnet_conv_args;
int sdk_resnet_conv2d(sdk_ctx* ctx, const sdk_resnet_conv_args* a, void* stream);
/* The ResNet34 forward with S weighted poolings per segment (diarize.py: one per local speaker of a 10-s chunk).  The conv trunk - the conv
 *   sequence of sdk_resnet_forward, bit for bit - runs once per segment; ONE pooling launch reads the last map [B][F4][T4][C] and writes the
 *   statistics rows b S + s; seg_1 runs over the B S rows -> emb [B S, embed_dim].
 *   w [B][S][T4] fp32 >= 0 (any weights, not only 0 / 1), T4 = sdk_resnet_last_map_frames(d, T); valid [B][S] int32.  With v1 = sum w,
 *   v2 = sum w^2:  mean = sum w x / v1,  var = sum w (x - mean)^2 / (v1 - v2 / v1),  std = sqrt(var + 1e-7): two passes, fp32, frames in
 *   order, feature order as in sdk_resnet_forward; with 0 / 1 weights the unbiased statistic over the selected columns.  A row depends on
 *   its own weights only.  Rows with valid == 0 are written as zeros (a valid row needs v1 - v2 / v1 > 0: two columns).
 *   Precision 0 and 2 (1 is refused).  Workspace: sdk_resnet_masked_workspace_bytes(d, B, T, S).
 *   sdk_resnet_masked_pool: building block: the pooling alone on a last map x [B][F][T][C] (fmt 0: bf16, 2: fp16) -> out [B S][2 C F].
 *   sdk_resnet_pool: building block: the unweighted pooling of sdk_resnet_forward alone on the same layout -> out [B][2 C F]: mean = sum x
 *   (1 / T), std = sqrt(sum (x - mean)^2 (1 / (T - 1)) + 1e-7), two passes, fp32, frames in order.  T < 2 and fmt 1 are refused. */
int sdk_resnet_last_map_frames(const sdk_resnet_desc* d, int T);
size_t sdk_resnet_masked_workspace_bytes(const sdk_resnet_desc* d, int B, int T, int S);
int sdk_resnet_forward_masked(sdk_ctx* ctx, const void* wblob, const sdk_resnet_desc* d, const uint16_t* feats, int ldf, int B, int T,
                              int S, const float* w, const int32_t* valid, void* ws, size_t ws_bytes, float* emb, void* stream);
int sdk_resnet_masked_pool(sdk_ctx* ctx, const uint16_t* x, int B, int F, int T, int C, int S, const float* w, const int32_t* valid,
                           float* out, int fmt, void* stream);
int sdk_resnet_pool(sdk_ctx* ctx, const uint16_t* x, int B, int F, int T, int C, float* out, int fmt, void* stream);

/* ---- speaker segmentation: PyanNet as in pyannote segmentation-3.0 (segmentation.py; csrc/segmentation.hip).  One chunk of S >= 991
 *      samples (16 kHz mono int16) -> F(S) = ((((S - 251) / 10 + 1) / 3 - 4) / 3 - 4) / 3 frames (589 at S = 160 000; frame i sees samples
 *      [270 i, 270 i + 991)) -> log-probabilities of the 7 powerset classes {}, {0}, {1}, {2}, {0,1}, {0,2}, {1,2}.
 *   chunk source: starts == NULL: B rows of a [B][ld] int16 matrix (ld >= S, (B - 1) ld + S <= n_samples); else starts [B] int32 (device) =
 *      first sample of every chunk inside the recording samples [n_samples] (device), samples past its end read as zero - the overlapping
 *      chunks never exist on the host, as in sdk_fbank_windows.
 *   sdk_segmentation_forward : -> logp [B][F][7] fp32.  B = 0 is a no-op; S < 991, precision 1 and too small a workspace are refused.
 *   sdk_sincnet_frontend     : building block: the SincNet stages alone -> out [B F][64] fp32 frames (features 0..59, 60..63 zero).
 *   sdk_bilstm_layer         : building block: one BiLSTM layer (both directions): x [B F][ldx] fp32 (60 features for layer 0, ldx >= 64;
 *                              256 for layers 1..3; ldx % 8 == 0) -> y [B F][256] fp32 (forward | reverse); workspace >= B F 4096 bytes.
 *   sdk_segmentation_workspace_bytes(d, B, S): the forward's and the front end's workspace (0 for arguments they refuse).
 *   Descriptor: precision 0 (bf16) / 2 (fp16): the format of the weights and of the MFMA operands; activations cross the stages in fp32 and
 *   enter the MFMAs as hi + lo planes of that format.  off[] = 256-aligned byte offsets of the
 *   weight slots SDK_SEG_* in one device blob (segmentation.pack_weights writes both). */
enum {
  SDK_SEG_SINC = 0,      /* 2-byte [80][256]: the sinc filters (cos 0..39, sin 40..79), taps 251..255 zero */
  SDK_SEG_SINC_SUM,      /* fp32 [80]: sum of each rounded filter's taps */
  SDK_SEG_WAVNORM,       /* fp32 [2]: waveform InstanceNorm weight, bias */
  SDK_SEG_NORM0,         /* fp32 [2][80]: InstanceNorm weight | bias of the sinc block */
  SDK_SEG_CONV1_W,       /* 2-byte [64][416]: Conv1d(80, 60, 5), k = tap 80 + c; rows >= 60 and k >= 400 zero */
  SDK_SEG_CONV1_B,       /* fp32 [64] */
  SDK_SEG_NORM1,         /* fp32 [2][60] */
  SDK_SEG_CONV2_W,       /* 2-byte [64][320]: Conv1d(60, 60, 5) on 64-channel rows, k = tap 64 + c; c >= 60 and rows >= 60 zero */
  SDK_SEG_CONV2_B,       /* fp32 [64] */
  SDK_SEG_NORM2,         /* fp32 [2][60] */
  SDK_SEG_LSTM,          /* + 3 l: W_ih 2-byte [1024][64 | 256] (rows 512 d + gate row, gates i f g o), bias fp32 [1024] (b_ih + b_hh),
                            W_hh 2-byte [2][512][128] */
  SDK_SEG_LIN0_W = SDK_SEG_LSTM + 12,   /* 2-byte [128][256] */
  SDK_SEG_LIN0_B,        /* fp32 [128] */
  SDK_SEG_LIN1_W,        /* 2-byte [128][128] */
  SDK_SEG_LIN1_B,        /* fp32 [128] */
  SDK_SEG_CLS_W,         /* fp32 [7][128] */
  SDK_SEG_CLS_B,         /* fp32 [7] */
  SDK_SEG_SLOTS
};
typedef struct sdk_segmentation_desc {
  int32_t precision;
  int32_t reserved;
  int64_t off[32];
} sdk_segmentation_desc;
int sdk_segmentation_frames(int S);
size_t sdk_segmentation_workspace_bytes(const sdk_segmentation_desc* d, int B, int S);
int sdk_segmentation_forward(sdk_ctx* ctx, const void* wblob, const sdk_segmentation_desc* d, const int16_t* samples, int64_t n_samples,
                             const int32_t* starts, int ld, int B, int S, void* ws, size_t ws_bytes, float* logp, void* stream);
int sdk_sincnet_frontend(sdk_ctx* ctx, const void* wblob, const sdk_segmentation_desc* d, const int16_t* samples, int64_t n_samples,
                         const int32_t* starts, int ld, int B, int S, void* ws, size_t ws_bytes, float* out, void* stream);
int sdk_bilstm_layer(sdk_ctx* ctx, const void* wblob, const sdk_segmentation_desc* d, int layer, const float* x, int ldx, int B, int F,
                     void* ws, size_t ws_bytes, float* y, void* stream);

/* ---- speaker diarization (diarize.py; csrc/diarize.hip): the integer stages between the segmentation model, the masked ResNet34 forward
 *      and the clustering.  Every kernel is a gather with one owner per output element and integer arithmetic: no atomics, results
 *      bit-identical run to run.  Powerset classes as above; active(c, i, s): local speaker s is in the class of frame i of chunk c,
 *      count(c, i): the size of that class.
 *   sdk_powerset_decode : logp [C][F][7] fp32 -> cls [C][F] uint8, the argmax class (ties to the lower class; a NaN never wins).
 *   sdk_diarize_masks   : cls [B][F] -> w [B][3][T4] fp32 (the 0 / 1 pooling weights of sdk_resnet_forward_masked) and info [B][3][4] int32 =
 *        (active frames, clean frames, used_clean, valid).  Last-map column j takes frame i(j) = min(F - 1, (j F) / T4);
 *        full[j] = active(i(j), s), clean[j] = full[j] and count(i(j)) < 2; w = clean when sum clean >= 4, else full; valid = sum w >= 2.
 *        The two frame totals are counted on the F frames (clean: active and count < 2), not on columns.
 *   sdk_diarize_reconstruct : cls [C][F], starts [C] int32 ascending (first samples of the chunks), labels [C][3] int32 (cluster of each local
 *        speaker, -1: none), K clusters -> on the G = sdk_diarize_frames(n_samples) global frames (centre 270 g + 495):
 *        chunk c contributes its frame i = g + q_c, q_c = floor((135 - start_c) / 270), when 0 <= i < F (found by binary search, not a scan);
 *        act[g][k] = number of contributing chunks with an active local speaker labelled k; nc = contributing chunks; cnt = sum count(c, i);
 *        count[g] = min((2 cnt + nc) / (2 nc), 2, max_speakers) (0 when nc = 0): uint8 [G];
 *        speakers [G][2] int32: the count[g] clusters with the largest act > 0, ties to the lower cluster, padded with -1;
 *        act (or NULL) [G][K] int32.  Any K >= 1. */
int sdk_powerset_decode(sdk_ctx* ctx, const float* logp, int C, int F, uint8_t* cls, void* stream);
int sdk_diarize_masks(sdk_ctx* ctx, const uint8_t* cls, int B, int F, int T4, float* w, int32_t* info, void* stream);
int64_t sdk_diarize_frames(int64_t n_samples);
int sdk_diarize_reconstruct(sdk_ctx* ctx, const uint8_t* cls, const int32_t* starts, const int32_t* labels, int C, int F, int K,
                            int64_t n_samples, int max_speakers, uint8_t* count, int32_t* speakers, int32_t* act, void* stream);

/* ---- the assignment stage of the diarization (diarize.py "assignment"; csrc/diarize.hip): float64 arithmetic in a fixed order, one owner per
 *      output element, no atomics: bit-identical run to run.  E [3 C][d] fp32 unit rows; d a multiple of 64, at most 512.  A candidate
 *      of chunk c is a local speaker with info valid != 0 and active frames > 0; no other row of E is read (it may hold anything).
 *   sdk_diarize_centroids : rows [n] int32 ascending (rows of E), labels [n] int32 in [0, K) (both on the device) -> cent [K][d] fp32 unit
 *        rows and cent64 [K][d] float64 (or NULL), the same before the final rounding: the float64 sum of each cluster's rows in ascending
 *        row order, divided by the count, divided by its norm (clamped at 1e-300).  A cluster without rows gives a zero row; a label
 *        outside [0, K) belongs to no cluster.  rows must lie inside E: the library does not read them back to check.
 *   sdk_diarize_assign : info [C][3][4] int32 (sdk_diarize_masks), cent64 [K][d] float64 (16-byte aligned) -> labels [C][3] int32 and
 *        score [C][3] fp32 (the cosine of each row to the centroid it got, 0 where the label is -1).  Cosines are float64 dot products
 *        summed in column order.  constrained = 0: every candidate takes its largest cosine (ties to the lower cluster).  constrained = 1:
 *        per chunk with m candidates, among all maps that give n = min(m, K) candidates pairwise different clusters and the others -1,
 *        the one with the largest total cosine (summed in slot order); ties to the lexicographically smallest label tuple in slot order,
 *        -1 after every cluster.  A NaN cosine never wins.  One launch, one wave per chunk; any K >= 1, any C >= 0. */
int sdk_diarize_centroids(sdk_ctx* ctx, const float* E, const int32_t* rows, const int32_t* labels, int n, int K, int d, float* cent,
                          double* cent64, void* stream);
int sdk_diarize_assign(sdk_ctx* ctx, const float* E, const int32_t* info, const double* cent64, int C, int K, int d, int constrained,
                       int32_t* labels, float* score, void* stream);

/* ---- many recordings in one pass (diarize.Diarizer.run_many; csrc/diarize.hip): R recordings laid end to end.  chunk_off, frame_off, cent_off,
 *      cl_off [R + 1] int32 are prefix sums (chunks, global frames, final clusters, clusters of the cut) and, like every other array here, live on
 *      the DEVICE: the kernels find the recording of a chunk / frame / cluster by a binary search on them (no per-element table).  The totals
 *      (C chunks, G frames, K or Kc clusters) are passed as arguments so that no call reads the device.  Integer or float64, one owner per
 *      output element, fixed order: bit-identical run to run; the only atomic is the integer atomicMin of sdk_diarize_first_seen.
 *   sdk_diarize_assign_grouped : sdk_diarize_assign with the centroids cent_off[r] .. cent_off[r + 1] for the chunks of recording r; labels are
 *        local to the recording (0 .. K_r - 1); K_r = 0 gives -1 and score 0.  One wave per chunk, any K_r.
 *   sdk_diarize_fold_grouped : cluster.fold_small_clusters steps 2 - 4.  cent64 [Kc][d] unit centroids of the cut (sdk_diarize_centroids), sizes
 *        [Kc], eff [R] the effective minimum size.  target [Kc] (scratch): a cluster with sizes >= eff stays, every other goes to the large
 *        cluster of its recording with the largest float64 cosine (fma chain in column order; ties to the lower cluster), or to the
 *        recording's first cluster when none is large.  remap [Kc] = cent_off[r] + the kept cluster's number by first appearance (the cut's
 *        labels are canonical); the caller's cent_off must count the large clusters (1 when none).  out [n] = remap[cut[i]] (cut: the cut's
 *        global cluster of every training row; NULL with n = 0).
 *   sdk_diarize_reconstruct_grouped : thread = packed frame; sdk_diarize_reconstruct inside the chunk range and with the K_r of the frame's
 *        recording (K_r = 0 as K = 1); starts_local [C] are first samples inside the chunk's own recording, ascending per recording;
 *        n_samples [R] int64; act (or NULL) holds recording r's [G_r][max(K_r, 1)] table at act_off[r] (int64 [R + 1]).
 *   sdk_diarize_first_seen : first [K] = the least 2 g + slot at which the cluster stands in speakers of its recording (g local), INT32_MAX
 *        when never (integer atomicMin).
 *   sdk_diarize_renumber : renum [K] = rank of (first[k], k) inside the recording (diarize.appearance_order); labels [C][3] (local) are
 *        rewritten in place; the centroid rows go to cent_off[r] + renum[k] of cent_out / cent64_out (not in place). */
int sdk_diarize_assign_grouped(sdk_ctx* ctx, const float* E, const int32_t* info, const double* cent64, const int32_t* chunk_off,
                               const int32_t* cent_off, int R, int C, int d, int constrained, int32_t* labels, float* score, void* stream);
int sdk_diarize_fold_grouped(sdk_ctx* ctx, const double* cent64, const int32_t* sizes, const int32_t* cl_off, const int32_t* eff,
                             const int32_t* cent_off, int R, int Kc, int d, int32_t* target, int32_t* remap, const int32_t* cut, int n,
                             int32_t* out, void* stream);
int sdk_diarize_reconstruct_grouped(sdk_ctx* ctx, const uint8_t* cls, const int32_t* starts_local, const int32_t* labels,
                                    const int32_t* chunk_off, const int32_t* frame_off, const int64_t* n_samples, const int32_t* cent_off,
                                    int R, int C, int F, int64_t G, int max_speakers, uint8_t* count, int32_t* speakers, int32_t* act,
                                    const int64_t* act_off, void* stream);
int sdk_diarize_first_seen(sdk_ctx* ctx, const int32_t* speakers, const int32_t* frame_off, const int32_t* cent_off, int R, int64_t G, int K,
                           int32_t* first, void* stream);
int sdk_diarize_renumber(sdk_ctx* ctx, const int32_t* first, const int32_t* cent_off, const int32_t* chunk_off, int R, int K, int C, int d,
                         int32_t* renum, int32_t* labels, const float* cent, const double* cent64, float* cent_out, double* cent64_out,
                         void* stream);

/* ---- scoring a diarization against a reference (score.py; csrc/score.hip): the diarization error rate on the packed frame grid above
 *      (frame g of recording r, at frame_off[r] + g, has centre sample 270 g + 495).  frame_off, cent_off as above; turn_off, ref_off [R + 1]
 *      int32 are the prefix sums of the recordings' merged reference turns and reference speakers, co_off [R + 1] int64 those of S_r K_r.
 *      max_ref / max_hyp: the largest S_r / K_r, stated by the caller; more than 64 is refused.  Integer arithmetic only (atomic OR, atomic
 *      integer add, stores of one value): bit-identical run to run.  Three calls, in stream order; no call reads the device on the host.
 *   sdk_score_reference : turns [M][3] (s0, s1, speaker; samples; merged per speaker by the caller: score.prepare_reference) ->
 *        ref_mask [G] uint64, bit i set iff a turn of speaker i has s0 <= 270 g + 495 < s1; scored [G] uint8 = 1, but 0 on the frames with
 *        |270 g + 495 - b| < collar for a boundary b (an s0 or s1 of a turn with s1 > s0; collar in samples, 0: none), and with
 *        skip_overlap != 0 on the frames with two or more bits.  Turns with s1 <= s0 or a speaker outside 0 .. S_r - 1 are skipped.
 *   sdk_score_cooccur : over the frames with scored != 0, nref = bits of ref_mask, nhyp = entries >= 0 of speakers [G][2]: tally [R][5] int64 =
 *        (frames, sum nref, sum max(0, nref - nhyp), sum max(0, nhyp - nref), sum min(nref, nhyp)) and co (int32; recording r's
 *        [S_r][K_r] table at co_off[r], co_total cells in all) = the frames in which reference i and hypothesis j are both active (an
 *        entry >= K_r names nobody; a speaker named twice in a frame counts once).  Both are cleared first.
 *   sdk_score_map : one wave per recording, the exact maximum-weight assignment on its co table (zero-padded to square, shortest augmenting
 *        paths, int64 potentials) -> correct [R] int64, the optimum, and map [ref_off[R]] int32: the hypothesis speaker of every
 *        reference speaker in one optimal assignment, -1 where it has none or the pair never co-occurs. */
int sdk_score_reference(sdk_ctx* ctx, const int32_t* turns, const int32_t* turn_off, const int32_t* frame_off, const int32_t* ref_off, int R,
                        int M, int64_t G, int max_ref, int collar, int skip_overlap, uint64_t* ref_mask, uint8_t* scored, void* stream);
int sdk_score_cooccur(sdk_ctx* ctx, const uint64_t* ref_mask, const uint8_t* scored, const int32_t* speakers, const int32_t* frame_off,
                      const int32_t* ref_off, const int32_t* cent_off, const int64_t* co_off, int R, int64_t G, int max_ref, int max_hyp,
                      int64_t co_total, int32_t* co, int64_t* tally, void* stream);
int sdk_score_map(sdk_ctx* ctx, const int32_t* co, const int32_t* ref_off, const int32_t* cent_off, const int64_t* co_off, int R, int max_ref,
                  int max_hyp, int32_t* map, int64_t* correct, void* stream);

/* ---- scoring the DIHARD way (score.py; csrc/score_jer.hip): the evaluation map (UEM) and the tables of the Jaccard error rate, on the tables of
 *      the three calls above.  Integer arithmetic only (stores of one value, integer atomic adds, an unsigned 64-bit quotient): bit-identical
 *      run to run.  In stream order after the calls they follow; no call reads the device on the host.
 *   sdk_score_uem : after sdk_score_reference.  uem [U][2] int32 (s0, s1; samples), recording r's intervals at uem_off[r] .. uem_off[r + 1]
 *        (uem_off [R + 1] int32), sorted and disjoint (merged by the caller: score.prepare_uem) -> scored [G] = 0 on every frame whose centre
 *        270 g + 495 lies in none of its recording's intervals (s0 <= centre < s1); other frames keep what they hold.  A recording that is
 *        scored everywhere is handed the one interval [0, 2^31 - 1).  U == 0: nothing is scored.
 *   sdk_score_durations : after sdk_score_uem.  Over the frames with scored != 0: ref_frames [ref_off[R]] int32 = the frames in which
 *        reference speaker i is active (bit i of ref_mask, i < S_r), hyp_frames [cent_off[R]] int32 = the frames that name hypothesis speaker
 *        j (an entry of speakers [G][2] >= K_r names nobody; a speaker named twice in a frame counts once).  Both are cleared first.  More
 *        than 64 speakers a side is refused.
 *   sdk_score_jaccard : after sdk_score_cooccur and sdk_score_durations.  q (int32, laid out as co: recording r's [S_r][K_r] table at
 *        co_off[r]) = floor(co[i][j] * 2^30 / (ref_frames[i] + hyp_frames[j] - co[i][j])) in unsigned 64-bit arithmetic where co > 0, else
 *        0: the Jaccard index of the pair in units of 2^-30, at most 2^30 (co never exceeds ref_frames or hyp_frames).  sdk_score_map then
 *        runs on q as it stands: its `correct` is the Jaccard sum of the best assignment. */
int sdk_score_uem(sdk_ctx* ctx, const int32_t* uem, const int32_t* uem_off, const int32_t* frame_off, int R, int U, int64_t G, uint8_t* scored,
                  void* stream);
int sdk_score_durations(sdk_ctx* ctx, const uint64_t* ref_mask, const uint8_t* scored, const int32_t* speakers, const int32_t* frame_off,
                        const int32_t* ref_off, const int32_t* cent_off, int R, int64_t G, int max_ref, int max_hyp, int32_t* ref_frames,
                        int32_t* hyp_frames, void* stream);
int sdk_score_jaccard(sdk_ctx* ctx, const int32_t* co, const int32_t* ref_frames, const int32_t* hyp_frames, const int32_t* ref_off,
                      const int32_t* cent_off, const int64_t* co_off, int R, int64_t co_total, int32_t* q, void* stream);

/* ---- speaker-attributed transcripts (words.py; csrc/words.hip): the words of a transcript onto the per-frame speakers of a diarization, on
 *      the packed frame grid above.  word_off [R + 1] int32: the prefix sums of the recordings' words; frame_off, cent_off, ref_off, co_off as
 *      above.  Integer arithmetic only (integer LDS atomics, integer atomic adds): bit-identical run to run.  No call reads the device on
 *      the host.
 *   sdk_words_attribute : words [W][2] int32 (s0, s1: samples inside the word's recording), speakers [G][2] -> out [W][8] int32 = (speaker,
 *        votes, solo, span, second, second_votes, distance, g0).  One wave per word.  With n the recording's frames, g0 = min(ceil((s0 - 495)
 *        / 270), n) and g1 likewise from s1, both at least 0 (the frames whose centre lies in [s0, s1)); if g1 <= g0 the one frame nearest
 *        the midpoint m = (s0 + s1) >> 1: g0 = clamp(floor((m - 360) / 270), 0, n - 1), g1 = g0 + 1.  span = g1 - g0; g0 is local to the
 *        recording.  v[k] = the frames of the word that name speaker k (an entry < 0 or >= K_r names nobody, a speaker named twice in a
 *        frame counts once), u[k] = those that name k alone.  speaker = the k with v[k] > 0 first in the order (v descending, u descending,
 *        k ascending), votes = v, solo = u; second, second_votes = the next in that order with v > 0, else (-1, 0); distance = 0.  Every v
 *        0: the least delta in 1 .. gap_frames for which frame g0 - delta or g1 - 1 + delta, inside the word's own recording, names somebody
 *        (the earlier side first, then the first entry of the frame) gives speaker, votes = solo = 0, second = -1, distance = delta; none:
 *        speaker = distance = -1.  A recording without frames: (-1, 0, 0, 0, -1, 0, -1, 0).  max_hyp: the largest K_r, stated by the
 *        caller (the counters in LDS are sized by it; more than 1024 is refused; a K_r above it is read as max_hyp rounded up to 64).
 *   sdk_words_cooccur : rows = sdk_words_attribute's out, ref [W] int32 = the reference speaker of every word (outside 0 .. S_r - 1: not
 *        scored) -> tally [R][3] int64 = (scored words, scored words whose speaker is outside 0 .. K_r - 1, words) and co (int32; recording
 *        r's [S_r][K_r] table at co_off[r], co_total cells in all) = the scored words with reference i and speaker j.  Both are cleared
 *        first.  More than 64 speakers a side is refused; sdk_score_map then runs on co as it stands. */
int sdk_words_attribute(sdk_ctx* ctx, const int32_t* words, const int32_t* word_off, const int32_t* speakers, const int32_t* frame_off,
                        const int32_t* cent_off, int R, int W, int64_t G, int max_hyp, int gap_frames, int32_t* out, void* stream);
int sdk_words_cooccur(sdk_ctx* ctx, const int32_t* rows, const int32_t* ref, const int32_t* word_off, const int32_t* ref_off,
                      const int32_t* cent_off, const int64_t* co_off, int R, int W, int max_ref, int max_hyp, int64_t co_total, int32_t* co,
                      int64_t* tally, void* stream);

/* ---- speaker samples (samples.py; csrc/samples.hip): each diarized speaker's clean stretches of audio on the packed frame grid above, and
 *      the scores of the clips cut from them.  frame_off, cent_off as above.  Every output is bit-identical run to run: the runs are
 *      integers and every element has one owner, the scores are float64 sums in a fixed order without floating-point atomics.  No call
 *      reads the device on the host.
 *   sdk_samples_runs : speakers [G][2] -> run_off [R + 1] int32, rows [run_off[R]][4] int32 = (speaker, g0, g1, solo).  An entry < 0 or
 *        >= K_r names nobody (max_hyp: the largest K_r, stated by the caller; more than 1024 is refused and a K_r above 1024 is read as 1024) and a speaker named twice counts once; a frame that names nobody is silent, one that
 *        names exactly {k} is solo for k, any other is overlapped.  A run of k is a maximal [g0, g1) inside one recording whose first and
 *        last frames are solo for k, whose frames are all solo for k or silent and in which no more than gap_frames silent frames follow
 *        one another; solo counts its solo frames, and it is written iff solo >= min_frames (at least 1).  g0 and g1 are local to the
 *        recording; recording r's rows are run_off[r] .. run_off[r + 1] - 1, by ascending g0.  rows_cap: the rows that `rows` can hold, at
 *        least G / min_frames (the most runs G frames hold; rows is 16-byte aligned).  A segmented scan and a compaction in nine short
 *        launches (csrc/samples.hip lists them): the cost does not depend on how long the runs are.  ws: a 16-byte aligned device buffer of
 *        sdk_samples_runs_workspace_bytes(G) bytes (0 with sdk_last_error: G outside 0 .. 2^30 - 1); not read with G = 0.
 *   sdk_samples_score : E [W][d] fp32 rows on the device (read as they are: not renormalised; d a multiple of 64, at most 512), clip_off
 *        [M + 1] int32 (clip i holds the rows clip_off[i] .. clip_off[i + 1] - 1), clip_spk [M] int32 (the clip's speaker, numbered over
 *        the pack: spk_off[r] + its number inside recording r; outside 0 .. S - 1: nobody's, scored (0, 0, -1, windows, 1)), spk_off
 *        [R + 1] int32 prefix sums of the recordings' speakers, S = spk_off[R].  With c_i the float64 sum of clip i's rows, m_s the sum of
 *        the c_i of speaker s in ascending i and cos(a, b) = a . b / (sqrt(a . a) sqrt(b . b)):  mean [S][d] float64 = m_s / (the rows of
 *        speaker s), zeros without rows;  out_f [M][2] float64 = (own, rival), own = cos(c_i, m_s - c_i), 0 with alone = 1 when either
 *        has norm 0; rival = the largest cos(c_i, m_t) over the other speakers t of the clip's recording with |m_t| > 0, the lowest t at
 *        equal values, (0, -1) when there is none or |c_i| = 0;  out_i [M][3] int32 = (rival's number inside the recording or -1, the
 *        clip's rows, alone).  ws: an 8-byte aligned device buffer of sdk_samples_score_workspace_bytes(M, S, d) bytes. */
size_t sdk_samples_runs_workspace_bytes(int64_t G);
int sdk_samples_runs(sdk_ctx* ctx, const int32_t* speakers, const int32_t* frame_off, const int32_t* cent_off, int R, int64_t G,
                     int max_hyp, int gap_frames, int min_frames, int32_t* run_off, int32_t* rows, int64_t rows_cap, void* ws, size_t ws_bytes,
                     void* stream);
size_t sdk_samples_score_workspace_bytes(int M, int S, int d);
int sdk_samples_score(sdk_ctx* ctx, const float* E, int W, int d, const int32_t* clip_off, const int32_t* clip_spk, int M,
                      const int32_t* spk_off, int R, int S, double* mean, double* out_f, int32_t* out_i, void* ws, size_t ws_bytes,
                      void* stream);

/* ---- smoothing of the diarized turns (smooth.py; csrc/smooth.hip): a speaker's short pauses filled, then the short runs dropped, on the
 *      packed frame grid above.  frame_off, cent_off as above.  Integers only, one owner per frame in every launch, integer atomic sums for
 *      the tallies: bit-identical run to run.  Everything is enqueued on `stream`; nothing waits and nothing is read on the host.
 *   sdk_smooth_turns : speakers [G][2] int32, REWRITTEN in place.  An entry < 0 or >= K_r names nobody and a speaker named twice in a frame
 *        counts once (any K_r >= 0: the kernels hold no per-speaker memory).  (1) fill: a gap of k is a maximal stretch of frames that do
 *        not name k whose neighbours on both sides lie in the same recording and name k; k is a filler of every frame of a gap of at most
 *        fill_frames frames, decided on the input alone.  (2) cap: the intermediate frame names the input frame's speakers in slot order,
 *        each once, compacted to the low slot, then its fillers in ascending k until `cap` (1 or 2) speakers stand; a filler never
 *        displaces a speaker of the input.  (3) drop: with keep_frames > 0, every maximal run of consecutive frames of one recording that
 *        name k in the intermediate table and is shorter than keep_frames loses k; what remains of a frame is compacted in the same order.
 *        Empty slots hold -1.  fill_frames = keep_frames = 0 returns the canonical form of the input.  Both are at most 1024 frames; more
 *        is refused.  tallies [R][2] int32 (zeroed by the call) = per recording (filled: the (frame, speaker) pairs the intermediate
 *        table names and the input does not; dropped: those the intermediate table names and the output does not).  ws: a 16-byte aligned
 *        device buffer of sdk_smooth_turns_workspace_bytes(G) bytes (0 with sdk_last_error: G outside 0 .. 2^30 - 1); not read with G = 0. */
size_t sdk_smooth_turns_workspace_bytes(int64_t G);
int sdk_smooth_turns(sdk_ctx* ctx, int32_t* speakers, const int32_t* frame_off, const int32_t* cent_off, int R, int64_t G, int fill_frames,
                     int keep_frames, int cap, int32_t* tallies, void* ws, size_t ws_bytes, void* stream);

/* ---- fusing several diarizations of a recording (fuse.py; csrc/fuse.hip): DOVER-Lap label mapping and weighted voting on the packed frame
 *      grid above.  R recordings, each with the same H hypotheses (2 .. 8); hypothesis h of recording r is group h R + r, spk_off [H R + 1]
 *      int32 holds the prefix sums of the groups' speaker counts K (at most 64 each; max_spk: the largest, stated by the caller) and the masks
 *      are [H][G] uint64, bit k of mask[h][g] set iff speaker k of the group is active in the frame; bits at or above K name nobody.  Pairs
 *      (a, b), a < b, are numbered p = a (2 H - a - 1) / 2 + (b - a - 1), P = H (H - 1) / 2 of them; pair group q = p R + r, and co_off
 *      [P R + 1] int64 holds the prefix sums of K_a K_b.  Integers only (stores of one value, integer atomic adds): bit-identical run to
 *      run.  No call takes a workspace; each clears what it accumulates into; everything is enqueued on `stream`, nothing waits and
 *      nothing is read on the host.  Refused, with sdk_last_error: H outside 2 .. 8, max_spk above 64, G outside 0 .. 2^30 - 1, cap
 *      outside {1, 2}.
 *   sdk_fuse_masks : one hypothesis.  speakers [G][2] int32 (8-byte aligned), spk_off [R + 1] int32 (the hypothesis' slice of the table
 *        above: only differences are read) -> mask [G]: bit k set iff an entry of speakers[g] is k with 0 <= k < K_r (a name twice counts
 *        once).  One thread per frame.
 *   sdk_fuse_cooccur : all P pairs in one launch.  co (int32; pair group q's [K_a][K_b] table at co_off[q], co_total cells in all) = the
 *        frames in which bit i of mask[a] and bit j of mask[b] are both set; tally [P R][2] int64 = (sum max(n_a, n_b), sum min(n_a, n_b))
 *        with n the valid bits of a frame.  Both are cleared first.  sdk_score_map then runs on co as it stands, with P R "recordings" and
 *        the prefix sums of K_a and K_b as ref_off and cent_off: correct [P R].
 *   sdk_fuse_labels : one wave per recording.  dis [R][H][H] int64: dis[a][b] = dis[b][a] = tally[q][0] - correct[q], 0 on the diagonal;
 *        order [R][H] int32: the hypotheses by ascending D_h = sum_b dis[h][b], ties to the lower h; weight [R][H] int32: weights[h]
 *        (weights [H] int32, 1 .. 65536) when weights is not null, else rank_weight[rank of h] (rank_weight [8] int32).  label_of
 *        [spk_off[H R]] int32, the fused label of every speaker of every group: the anchor order[0] keeps its numbers and L = K_anchor; then
 *        for h = order[1], order[2], ..: A[u][j] = the sum of co(h', h)[i][j] over the earlier h' and their speakers i with label u; greedily
 *        the largest A[u][j] > 0 over unused u and unmapped j (ties to the lowest u, then the lowest j) gives label_of[h][j] = u until none
 *        is positive; the unmapped j in ascending order get L, L + 1, .. while L < 64, then -1, each -1 counted in overflow [R] int32.
 *        n_labels [R] int32 = L at the end.
 *   sdk_fuse_vote : one thread per frame.  With c_h the valid bits of mask[h][g], seen_h the labels >= 0 of those bits, v[u] = the sum of
 *        weight[r][h] over the h with u in seen_h and W the sum of the weights: n = min(cap, (2 sum_h w_h c_h + W) / (2 W)); speakers
 *        [G][2] int32 (8-byte aligned) names the labels with v > 0 first in the order (v descending, u ascending), at most n, from slot
 *        0; empty slots hold -1.  tallies [R][4] int64 = (frames that name somebody, frames that name two, frames whose H sets seen_h are
 *        all equal, overflow[r]). */
int sdk_fuse_masks(sdk_ctx* ctx, const int32_t* speakers, const int32_t* frame_off, const int32_t* spk_off, int R, int64_t G, int max_spk,
                   uint64_t* mask, void* stream);
int sdk_fuse_cooccur(sdk_ctx* ctx, const uint64_t* mask, const int32_t* frame_off, const int32_t* spk_off, const int64_t* co_off, int H, int R,
                     int64_t G, int max_spk, int64_t co_total, int32_t* co, int64_t* tally, void* stream);
int sdk_fuse_labels(sdk_ctx* ctx, const int32_t* co, const int64_t* tally, const int64_t* correct, const int32_t* spk_off, const int64_t* co_off,
                    const int32_t* rank_weight, const int32_t* weights, int H, int R, int max_spk, int64_t* dis, int32_t* order, int32_t* weight,
                    int32_t* label_of, int32_t* n_labels, int32_t* overflow, void* stream);
int sdk_fuse_vote(sdk_ctx* ctx, const uint64_t* mask, const int32_t* frame_off, const int32_t* spk_off, const int32_t* label_of,
                  const int32_t* weight, const int32_t* overflow, int H, int R, int64_t G, int max_spk, int cap, int32_t* speakers,
                  int64_t* tallies, void* stream);

/* ---- VBx clustering of the diarization (cluster.vbx_cluster, plda.py; csrc/vbx.hip): float64 arithmetic, every sum over rows over fixed 64-row
 *      blocks whose partials are combined in block order, no floating-point atomics, one owner per output element: bit-identical run to
 *      run.  n <= 65 536 rows, D = 64 or 128, any S >= 1.
 *   sdk_plda_transform : E [R][d_in] fp32 unit rows (d_in a multiple of 64, at most 512), rows [n] int32 (rows of E; must lie inside E: the
 *        library does not read them back to check), the prepared model as float64 device arrays - mean1 [d_in], lda [d_in][D0] (D0 <= 512),
 *        mean2 [D0], mu [D0], Tt [D0][D] (the first D rows of the PLDA basis T, transposed) -> X [n][D] float64:
 *        x1 = sqrt(d_in) unit(e - mean1), x2 = sqrt(D0) unit(lda^T x1 - mean2), x = (x2 - mu) Tt; unit divides by max(norm, 1e-300).
 *   sdk_vbx : X [n][D], Phi [D], the initial labels [n] int32 in [0, S) -> gamma [n][S], pi [S], elbo [max_iters] (entries from n_iter on
 *        are 0), n_iter and status (one int32 each), all on the device.  gamma0 = softmax_s(init_smoothing [label == s]), pi = 1 / S, then
 *        per iteration ii (rho = x sqrt(Phi), G_t = -(|x_t|^2 + D ln 2 pi) / 2):
 *          N_s = sum_t gamma[t][s]; invL[s][d] = 1 / (1 + (Fa / Fb) N_s Phi_d); alpha[s][d] = (Fa / Fb) invL[s][d] sum_t gamma[t][s] rho[t][d];
 *          z[t][s] = Fa (rho_t . alpha_s - sum_d (invL[s][d] + alpha[s][d]^2) Phi_d / 2 + G_t) + ln pi_s   (pi_s == 0: -inf, gamma exactly 0);
 *          lse_t = logsumexp_s z[t][s] (maximum subtracted); gamma = exp(z - lse);
 *          elbo[ii] = sum_t lse_t + (Fb / 2) sum_{s,d} (ln invL - invL - alpha^2 + 1); pi = sum_t gamma / sum_{t,s} gamma;
 *          stop after this iteration when ii > 0 and elbo[ii] - elbo[ii - 1] < epsilon (epsilon may be infinite, not NaN).
 *        Every iteration is enqueued; the stop test runs on the device and the launches after the stop leave every output untouched.
 *        status: 0, or bits 1 (a non-finite x or Phi: nothing ran, n_iter = 0), 2 (a label outside [0, S): the same), 4 (a non-finite elbo:
 *        stopped there).  The host reads n_iter and status once, after the call.  workspace: sdk_vbx_workspace_bytes (0 for arguments
 *        sdk_vbx would refuse), 256-byte aligned.
 *   sdk_vbx_centroids : gamma, pi, E, rows as above (d = E's width) -> K (one int32), keep [S] int32 (the speakers with pi > 1e-7 in
 *        their order, then -1), labels [n] int32 (or NULL: the arg-max of gamma over the kept speakers, ties to the lower), cent [S][d]
 *        fp32 and cent64 [S][d] float64 of which the first K rows are written: sum_t gamma[t][keep k] e_t in ascending row order, divided by
 *        sum_t gamma[t][keep k], divided by its norm (clamped at 1e-300) - the layout sdk_diarize_assign takes.
 *   sdk_vbx_hmm : sdk_vbx with the HMM of VBx as published: the n rows are a sequence in TIME ORDER, and P = loop_prob in [0, 1) is the
 *        probability that the speaker of row t is the speaker of row t - 1 (NaN, negative or >= 1: refused before any launch).  The
 *        transition matrix tr[i][j] = P [i == j] + (1 - P) pi_j is never formed.  Arguments, outputs, status bits, the stop test, n_iter,
 *        init_smoothing and the first iteration's pi = 1 / S are sdk_vbx's; per iteration, logp[t][s] = sdk_vbx's z[t][s] without ln pi_s, then
 *        in the log domain (ln P = log(P), ln(1 - P) = log1p(-P); logaddexp(a, b) = max + log1p(exp(min - max)), which returns the other
 *        argument exactly when one is -inf, and -inf when both are; every logsumexp with the maximum subtracted):
 *          lf[0][s] = logp[0][s] + ln pi_s;  m[t] = logsumexp_s lf[t][s];
 *          lf[t][s] = logp[t][s] + logaddexp(ln P + lf[t-1][s], (ln(1 - P) + ln pi_s) + m[t-1])                         (t >= 1)
 *          lb[n-1][s] = 0;  q_s = logp[t+1][s] + lb[t+1][s];  r = logsumexp_s(ln pi_s + q_s);
 *          lb[t][s] = logaddexp(ln P + q_s, ln(1 - P) + r)                                                              (t < n - 1)
 *          tll = m[n-1];  gamma[t][s] = exp(lf[t][s] + lb[t][s] - tll);  elbo[ii] = tll + (Fb / 2) sum_{s,d} (ln invL - invL - alpha^2 + 1);
 *          pi'_s = gamma[0][s] + ((1 - P) pi_s) sum_{t >= 1} exp(m[t-1] + logp[t][s] + lb[t][s] - tll);  pi = pi' / sum_s pi'_s
 *        (pi_s == 0: ln pi_s = -inf and gamma[:, s] is exactly 0 from then on; P == 0: ln P = -inf, the mixture of sdk_vbx up to rounding).
 *        The two passes run side by side in one launch of two single-wave workgroups, a step costing two cross-lane reductions; up to
 *        S = 256 a lane keeps its speakers in registers, above it re-reads the rows it wrote.  Sums over rows: 64-row blocks combined in
 *        block order, as sdk_vbx.  workspace: sdk_vbx_hmm_workspace_bytes (sdk_vbx's plus 3 n S + n doubles and the partials of pi'). */
int sdk_plda_transform(sdk_ctx* ctx, const float* E, int d_in, const int32_t* rows, int n, const double* mean1, const double* lda,
                       const double* mean2, const double* mu, const double* Tt, int D0, int D, double* X, void* stream);
size_t sdk_vbx_workspace_bytes(int n, int D, int S);
int sdk_vbx(sdk_ctx* ctx, const double* X, const double* Phi, const int32_t* labels, int n, int D, int S, double Fa, double Fb, int max_iters,
            double epsilon, double init_smoothing, double* gamma, double* pi, double* elbo, int32_t* n_iter, int32_t* status, void* ws,
            size_t ws_bytes, void* stream);
size_t sdk_vbx_hmm_workspace_bytes(int n, int D, int S);
int sdk_vbx_hmm(sdk_ctx* ctx, const double* X, const double* Phi, const int32_t* labels, int n, int D, int S, double Fa, double Fb, int max_iters,
                double epsilon, double init_smoothing, double loop_prob, double* gamma, double* pi, double* elbo, int32_t* n_iter,
                int32_t* status, void* ws, size_t ws_bytes, void* stream);
int sdk_vbx_centroids(sdk_ctx* ctx, const double* gamma, const double* pi, const float* E, const int32_t* rows, int n, int S, int d, int32_t* K,
                      int32_t* keep, int32_t* labels, float* cent, double* cent64, void* stream);

/* ---- training the VBx PLDA from labelled embeddings (plda.fit; csrc/plda_fit.hip): the sums over n <= 2^24 labelled rows that the host's d x d
 *      solves start from.  Float64 results; no floating-point atomics, one owner per output element; rows are cut into
 *      ceil(n / RB) fixed blocks of RB = max(512, 64 ceil(n / 16384)) rows, summed inside a block in ascending order (the scatter: four rows per
 *      f64 MFMA) and across blocks in block order; a class sum runs over the class's rows in the order of `order`: bit-identical run to run.
 *   sdk_plda_fit_stats : exactly one source - E [n][d] fp32 rows (d a multiple of 64, at most 512; with mean1 [d] every row enters as
 *        sqrt(d) unit(e - mean1), with mean1 NULL as it is) or X [n][d] float64 rows as they lie (d 1 .. 512, mean1 NULL) - and, with K > 0,
 *        labels [n] int32 and order [n] int32 (the row indices sorted by label, stably: ascending inside a class) -> counts [K] int64,
 *        sums [K][d] (zeros for a class without rows), total [d], scatter [d][d] = sum x x^T (the upper triangle is computed and mirrored:
 *        exactly symmetric; NULL skips it) and status (one int32: bit 1 = a label outside [0, K) - it is never used as an index; such rows are
 *        in total and scatter and in no class).  K = 0: labels, order, counts and sums may be NULL.  workspace:
 *        sdk_plda_fit_stats_workspace_bytes(n, d, K, scatter != NULL) (0 for arguments the call would refuse), 256-byte aligned.
 *   sdk_plda_project : E [n][d_in] fp32 rows, mean1 [d_in], lda [d_in][D0] (D0 <= 512), mean2 [D0] -> X2 [n][D0] float64:
 *        x2 = sqrt(D0) unit(lda^T sqrt(d_in) unit(e - mean1) - mean2), sdk_plda_transform's first two steps for every row. */
size_t sdk_plda_fit_stats_workspace_bytes(int n, int d, int K, int with_scatter);
int sdk_plda_fit_stats(sdk_ctx* ctx, const float* E, const double* X, const double* mean1, int n, int d, const int32_t* labels,
                       const int32_t* order, int K, int64_t* counts, double* sums, double* total, double* scatter, int32_t* status, void* ws,
                       size_t ws_bytes, void* stream);
int sdk_plda_project(sdk_ctx* ctx, const float* E, int d_in, int n, const double* mean1, const double* lda, const double* mean2, int D0,
                     double* X2, void* stream);

/* ---- spherical k-means on unit rows (cluster.kmeans_cluster; csrc/kmeans.hip): the forced speaker count of the diarization (`speakers=`) with
 *      clustering="vbx".  float64 arithmetic, no floating-point atomics, one owner per output element, every sum in one fixed order:
 *      bit-identical run to run.  n <= 65 536 rows, d a multiple of 64 up to 512, 1 <= k <= min(n, 64).
 *   sdk_kmeans_rows : E [R][d] fp32 unit rows, rows [n] int32 ascending (rows of E; must lie inside E: the library does not read them back
 *        to check) -> labels [n] int32 in [0, k) (NOT canonical; a centre may end without rows), n_iter and status (one int32 each), all on
 *        the device.  Row t below is E[rows[t]].
 *          seeding     centre 0 = row 0; centre j = the row whose largest cosine to the centres 0 .. j - 1 is least, ties to the lowest row.
 *                      A seed is a row, so each cosine is a sum of exact products, added over the columns in ascending order.
 *          assignment  label[t] = argmax_c <centre c, row t>: each cosine one float64 fma chain over the columns in ascending order; ties to
 *                      the lower centre; a NaN never wins.
 *          update      s_c = the float64 sum of the rows labelled c: per segment of 1024 rows (rows t = 1024 g .. 1024 g + 1023) in
 *                      ascending order, then the segments' partials in segment order; centre c = s_c / |s_c|.  A centre without rows, or
 *                      with |s_c| = 0, stays as it was.
 *          stop        iteration it = 0, 1, ..: assignment, then update.  The loop ends after the first assignment with it >= 1 that
 *                      changed no label, or after max_iters (1 .. 1000) assignments; n_iter counts the assignments made and labels are
 *                      those of the last one.
 *        Every iteration is enqueued; the stop test runs on the device and the launches after the stop leave every output untouched.
 *        status: 0, or 1 (a non-finite value in a row: nothing ran, n_iter = 0, labels = -1).  The host reads n_iter and status once,
 *        after the call.  workspace: sdk_kmeans_rows_workspace_bytes (0 for arguments sdk_kmeans_rows would refuse), 256-byte aligned. */
size_t sdk_kmeans_rows_workspace_bytes(int n, int d, int k);
int sdk_kmeans_rows(sdk_ctx* ctx, const float* E, const int32_t* rows, int n, int d, int k, int max_iters, int32_t* labels, int32_t* n_iter,
                    int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- adaptive score normalisation against a cohort (AS-norm; snorm.py, csrc/snorm.hip).  E [N][d], P [Pn][d] and Cn [M][d] are unit fp32 rows,
 *      16-byte aligned; d a multiple of 64, at most 512.  Scores are fp32 dot products on the fp32-input MFMA: one fused-multiply-add chain over
 *      the d columns in one fixed order, so a score depends on its two rows only (not on N, M, Pn or its place in them).  No floating-point
 *      atomics: bit-identical run to run.
 *   sdk_cohort_stats : of the M scores <e_n, c_j> of row n take the K largest (a multiset: equal scores need no tie rule), 1 <= K <= M <= 2^20;
 *        mean [N] = their mean, std [N] = their population standard deviation (divide by K), floored at 1e-6; both accumulated in float64 in
 *        a fixed order.  A non-finite row gives NaN statistics.  N = 0 is a no-op.  The rows are taken in row blocks whose [rows][M] fp32 score
 *        block is the workspace: sdk_cohort_stats_workspace_bytes (host-only; bounded in N; 0 with sdk_last_error set for arguments the call
 *        refuses), 16-byte aligned.
 *   sdk_affinity_topk_snorm : z(n, p) = ((s - mean_e[n]) / std_e[n] + (s - mean_p[p]) / std_p[p]) / 2 with s = <e_n, p_p> (formed in float64
 *        from the fp32 s and statistics, rounded once); per window the k <= 4 largest z, ties to the lower profile, a NaN z never taken ->
 *        idx [N][k] int32, score [N][k] (z), raw [N][k] (s).  Slots left without a finite candidate hold idx -1, score 0, raw 0.  Pn >= 1; when
 *        k > Pn the columns Pn .. k - 1 are NOT written.
 *   Shape refusals (d, M, K, k) come before anything else, the null context included.
 *   sdk_set_option "snorm_scores_only" 1 (bench knob, tools/snorm_bench.py): sdk_cohort_stats runs its scoring kernel only (mean, std not written). */
size_t sdk_cohort_stats_workspace_bytes(int N, int M, int K);
int sdk_cohort_stats(sdk_ctx* ctx, const float* E, int N, const float* Cn, int M, int d, int K, float* mean, float* std, void* ws,
                     size_t ws_bytes, void* stream);
int sdk_affinity_topk_snorm(sdk_ctx* ctx, const float* E, const float* mean_e, const float* std_e, int N, const float* P, const float* mean_p,
                            const float* std_p, int Pn, int d, int k, int32_t* idx, float* score, float* raw, void* stream);

/* ---- PLDA log-likelihood-ratio scoring of windows against enrolled SPEAKERS (plda_score.py states the rule; csrc/plda_score.hip).  Float64, in
 *      the space of sdk_plda_transform: D = 64 or 128 columns, within-speaker covariance I, between-speaker covariance diag(Phi).  For a speaker
 *      with pooled enrolment mean u and effective count n > 0, per column:  a = n Phi / (n Phi + 1),  v = 1 + Phi / (n Phi + 1),  g = a / v,
 *      q = -(1 / v - 1 / (1 + Phi)) / 2,  h = -a^2 / (2 v),  c = -(ln v - ln(1 + Phi)) / 2, and
 *          llr(x, s) = r_s + sum_d x_d G[s][d] + sum_d x_d^2 G[s][D + d],   G[s] = [g o u, q],   r_s = sum_d (c_d + u_d^2 h_d)
 *      = ln N(x | a u, v) - ln N(x | 0, 1 + Phi).  No floating-point atomics, one owner per output element, every sum in a fixed order:
 *      bit-identical run to run.
 *   sdk_plda_enroll : Xp [P][D] transformed profile rows (P <= 2^22), group [P] int32 (the speaker of every row, in any order), n_eff [S],
 *        Phi [D] -> G [S][2 D], r [S] (1 <= S <= 2^20) and status (one int32).  u_s = (the sum of the speaker's rows, added in ascending row
 *        order) / (their number).  A label outside [0, S) is never used as an index: the row belongs to no speaker and status bit 1 is set.
 *        A speaker without a row, or whose n_eff is not a finite number above 0: G row of zeros and r = NaN - it never wins.  A speaker's
 *        rows are found by a walk that costs (its rows)^2 / 64 index reads: meant for up to a few hundred enrolments per speaker.
 *        workspace: sdk_plda_enroll_workspace_bytes(P, S), 256-byte aligned.
 *   sdk_plda_score_topk : X [N][D] transformed windows (N <= 65 536; N = 0 is a no-op), G, r -> per window the k <= 4 largest llr, ties to the
 *        lower speaker, a NaN never taken: idx [N][k] int32, score [N][k].  Slots left without a candidate hold idx -1, score 0; when k > S
 *        the columns S .. k - 1 are NOT written.  scores (NULL to skip): the whole matrix [N][S]; score[n][j] is scores[n][idx[n][j]] bit for
 *        bit.  The kernel forms x^2 itself ([x, x^2] is never in memory) and runs the depth-2D product on the f64 MFMA; every llr is one
 *        chain in one order, so it depends on its window and its speaker only.  The speakers are cut into tiles of 64 and splits of at
 *        least 4 tiles, a function of (N, S) alone; the splits' lists are merged in split order under a strict total order, so the answer
 *        does not depend on the cut.  X and G 16-byte aligned.  workspace: sdk_plda_score_workspace_bytes(N, S, k), 256-byte aligned.
 *   Both sizers are host-only and return 0 with sdk_last_error set for arguments the calls refuse.  Shape refusals (D, S, P, N, k) come before
 *   anything else, the null context included. */
size_t sdk_plda_enroll_workspace_bytes(int P, int S);
int sdk_plda_enroll(sdk_ctx* ctx, const double* Xp, const int32_t* group, int P, int D, const double* n_eff, const double* Phi, int S, double* G,
                    double* r, int32_t* status, void* ws, size_t ws_bytes, void* stream);
size_t sdk_plda_score_workspace_bytes(int N, int S, int k);
int sdk_plda_score_topk(sdk_ctx* ctx, const double* X, int N, int D, const double* G, const double* r, int S, int k, int32_t* idx, double* score,
                        double* scores, void* ws, size_t ws_bytes, void* stream);

/* ---- verification trials: every (test row i < N, model row j < M) pair scored, classed and binned; the score matrix is never written (trials.py
 *      states the rule; csrc/trials.hip).  A [N][K], B [M][K], r [M] float64, K a multiple of 16 in 16 .. 512, 1 <= N, M <= 2^20; la, sa [N] and
 *      lb, sb [M] int32 labels and sessions.
 *          s(i, j) = r[j] + sum_k A[i][k] B[j][k]   on the f64 MFMA, one chain in one order per element
 *          t = (s - lo) * scale   one float64 subtraction, then one float64 multiplication (no FMA); scale = 2^24 / (hi - lo), formed by the caller
 *          NaN -> nan;  t < 0 -> below;  t >= 2^24 (+inf included) -> above;  else q = floor(t)
 *      Trial (i, j) is EXCLUDED when la[i] < 0 or lb[j] < 0 or (sa[i] >= 0 and sa[i] == sb[j]); else its class is 1 (target) when la[i] == lb[j],
 *      else 0.  With bin = (q >> shift) - base a trial that is neither excluded nor nan is counted exactly once: in hist[class][bin] when
 *      0 <= bin < 4096, in under[class] when (q >> shift) < base or below, in over[class] otherwise (above included).
 *      out: 8199 uint64 on the device - hist[2][4096], under[2], over[2], nan[2], excluded[1] - zeroed by the call in stream order.
 *      max_blocks: 0 = the default grid, else a cap on the number of (persistent) workgroups; the counters do not depend on it.  Integer
 *      counting only after the product: bit-identical run to run.  Refused (status 2, nothing launched): K, N, M, shift (0 .. 24), base
 *      (0 .. 2^24) or max_blocks (>= 0) outside their limits, a lo that is not finite, a scale that is not finite and above 0 (lo >= hi), a null
 *      pointer, A or B not 16-byte aligned.  sdk_set_option "trials_no_hist" 1 (bench knob, tools/trials_bench.py): the kernel without its LDS
 *      atomics; the in-range trials of a class then land in its bin 0. */
int sdk_trial_hist(sdk_ctx* ctx, const double* A, int N, const double* B, const double* r, int M, int K, const int32_t* la, const int32_t* sa,
                   const int32_t* lb, const int32_t* sb, double lo, double scale, int shift, int base, int max_blocks, uint64_t* out, void* stream);

/* ---- calibration of verification scores: one pass of the prior-weighted logistic objective over the trials of sdk_trial_hist (the same A, B, r,
 *      labels, sessions, classes, exclusions and score; trials.py states the rule; csrc/trials.hip).  With y = +1 for a target, -1 otherwise:
 *          z = a * s + c   one float64 multiplication, then one float64 addition (no FMA);   m = y z;   e = exp(-|m|)
 *          loss = max(-m, 0) + log1p(e);   p = e / (1 + e);   q = 1 / (1 + e);   w = p when m >= 0, else q;   v = p * q
 *      A trial whose score is NaN, +inf or -inf is counted in nonfinite[class] and left out of every sum.
 *      sums: [2][7] float64 on the device, per class (0 nontarget, 1 target) the sums of loss, w, w s, v, v s, (v s) s and s.
 *      counts: 5 uint64 on the device - n[2] (the trials summed, per class), nonfinite[2], excluded - zeroed by the call in stream order.
 *      No floating-point atomics: a lane adds its trials in tile order, the lanes of a wave in a fixed tree, the four waves in wave order, one
 *      row per workgroup in the workspace; a second kernel adds the rows in ascending order.  The sums are a function of the inputs and the grid
 *      alone: bit-identical run to run; another max_blocks (0 = the default grid, else a cap on the persistent workgroups) reorders additions
 *      and changes them by rounding only.  The counts do not depend on it.  workspace: sdk_trial_calib_workspace_bytes(N, M, max_blocks),
 *      256-byte aligned; the sizer is host-only and returns 0 with sdk_last_error set for arguments the call refuses.  Refused (status 2,
 *      nothing launched): K, N, M or max_blocks outside their limits, an a or c that is not finite, a null pointer, A or B not 16-byte aligned,
 *      a workspace that is null, too small or misaligned. */
size_t sdk_trial_calib_workspace_bytes(int N, int M, int max_blocks);
int sdk_trial_calib(sdk_ctx* ctx, const double* A, int N, const double* B, const double* r, int M, int K, const int32_t* la, const int32_t* sa,
                    const int32_t* lb, const int32_t* sb, double a, double c, int max_blocks, double* sums, uint64_t* counts, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- verification trials on the cohort-normalised (AS-norm) scale: sdk_trial_hist with the score replaced (trials_snorm.py states the rule;
 *      csrc/trials_snorm.hip).  A [N][K], B [M][K] float64 as for sdk_trial_hist (no r); mean_a, inv_a [N] and mean_b, inv_b [M] float64: per row the
 *      mean of its cohort scores and the RECIPROCAL of their standard deviation (the caller divides once per row: a trial costs no division).
 *          s(i, j) = sum_k A[i][k] B[j][k]   on the f64 MFMA, sdk_trial_hist's chain
 *          z = ((s - mean_a[i]) * inv_a[i] + (s - mean_b[j]) * inv_b[j]) * 0.5   six rounded float64 operations in this order (subtract, multiply,
 *              subtract, multiply, add, multiply; no FMA)
 *          t = (z - lo) * scale, then nan / below / above / q, the exclusions, the classes, bin = (q >> shift) - base and the 8199 counters of `out`
 *              exactly as sdk_trial_hist forms them; a NaN z (a NaN statistic, inf * 0) is counted in nan[class].
 *      A statistic of a row i >= N or j >= M is never read.  out is zeroed by the call in stream order; max_blocks as for sdk_trial_hist; integer
 *      counting only after z: bit-identical run to run.  Refused (status 2, nothing launched): what sdk_trial_hist refuses (K, N, M, shift, base,
 *      max_blocks, lo, scale, a null pointer - the four statistics included -, A or B not 16-byte aligned). */
int sdk_trial_hist_snorm(sdk_ctx* ctx, const double* A, int N, const double* B, int M, int K, const double* mean_a, const double* inv_a,
                         const double* mean_b, const double* inv_b, const int32_t* la, const int32_t* sa, const int32_t* lb, const int32_t* sb,
                         double lo, double scale, int shift, int base, int max_blocks, uint64_t* out, void* stream);

/* ---- audio conversion to the AudioProfile: replaces the ffmpeg subprocess the reference's backends
 *      run before upload (audio_profiles.py:70-100 `format_ffmpeg_args`; speechmatics_backend.py:231-281).
 *      x [n_in, channels] s16 interleaved -> y [n_out] s16 mono at rate_in * L / M, n_out = ceil(n_in * L / M).
 *      Channel down-mix (rounded mean) + polyphase FIR, integer arithmetic: taps [L][K] int32 Q30 (device memory,
 *      designed by the host layer, every phase summing to 2^30), int64 accumulation, round-half-up, s16 saturation;
 *      samples outside the input are zero.  Bit-exact against oracle/resample.py. -- */
int64_t sdk_resample_out_len(int64_t n_in, int L, int M);
int sdk_resample_s16(sdk_ctx* ctx, const int16_t* x, int64_t n_in, int channels, const int32_t* taps, int L, int M, int K,
                     int16_t* y, int64_t n_out, void* stream);
/* Host only: where sdk_resample_s16 stages its operands for a filter shape, the decision its launch is taken from.  Bit 0: the tap
 * table sits in LDS; bit 1: the workgroup's down-mixed input window sits in LDS (each when it fits in 64 KiB; otherwise the kernel
 * reads it from global memory).  -1: a shape sdk_resample_s16 refuses (L, M >= 1, K even and >= 2, L * K <= 2^22). */
int sdk_resample_plan(int L, int M, int K);

/* ---- k3: L2-normalise rows.  X [N, d] fp32 -> E fp32 unit rows, Eb bf16 copy,
 *      resid[n] = || E[n] - float(Eb[n]) ||_2 (rigorous per-row bf16 rounding residual).
 *      E = X[n] / max(||X[n]||, 1e-12) with the squared norm summed in fp32: a row of finite entries whose squared norm overflows fp32
 *      (entries past about 1e19 / sqrt(d)) comes back as a ZERO row (E, Eb and resid all 0), not as a unit row, and a row whose squared norm
 *      underflows is divided by the 1e-12 floor; a row with a NaN entry comes back all NaN (resid too).  E, Eb and resid may each be null: that output is skipped, the others are unchanged. -- */
int sdk_l2norm(sdk_ctx* ctx, const float* X, int N, int d, float* E, uint16_t* Eb, float* resid, void* stream);

/* ---- k4: segments x profiles cosine affinity with fused top-k (replaces the scoring a local
 *      identify_speaker performs per candidate: base.py:130-151; rows consumed by
 *      speaker_detection:1085-1127).
 *   coarse pass : bf16 MFMA  Eb [N,d] x Pb [P,d]^T, fused per-row candidate lists (no N x P matrix in HBM)
 *   exact pass  : fp32 re-score of the candidates, sorted, ties -> lowest profile index
 *   guarantee   : rows whose last coarse candidate is within the rounding margin of the k-th exact score
 *                 are re-scanned exactly in fp32 over all P, so idx/score equal an fp32 full scan
 *                 (k = 1 is the fast path: ~1 % of rows rescanned; larger k rescans more).
 * d must be 192 (= 12 MFMA k-steps), k <= 4.  idx [N,k] int32, score [N,k] fp32.
 * n_rescanned (device int32, may be NULL) receives the number of rows that took the exact path.
 *   non-finite rows : a NaN score compares with nothing and is never taken.  A slot for which no profile has a comparable score holds
 *                 idx -1, score -inf: every slot of a segment row that holds a NaN, and the slots past the comparable profiles when
 *                 profile rows hold NaNs.  idx is always in [-1, P); a caller skips idx < 0 (backend.aggregate_matches does, and
 *                 -inf clears no threshold).  All other rows keep the guarantee above.  A NaN residual (resid_e[n], or resid_p[0]
 *                 as the max over profile residuals with a NaN among them) certifies nothing: the rows it touches take the exact
 *                 rescan and are counted in n_rescanned.  The same on every path (k = 1 fast path, all its plans; general path).
 * ws: sdk_affinity_workspace_bytes(N, P). */
size_t sdk_affinity_workspace_bytes(int N, int P);
/* Host-only (no device): the k = 1 path's work decomposition, for tests.  out5 = {segment groups, profile stages per group,
 * workgroups, segments per group, record slots per segment}; *units = groups * stages; workgroup i sweeps the units
 * [i * units / workgroups, (i + 1) * units / workgroups) in (group, stage) order. */
int sdk_affinity_plan(int N, int P, int num_cu, int32_t* out5, int64_t* units);
/* Host-only: the unit range [u0, u1) of workgroup `wg` under that plan and the record slot of its first portion.  The ranges can be balanced by
 * cost instead of unit count ("affinity_boundary_penalty" p: a group boundary inside a range counts as p stages; default 0 - measured, not a robust win). */
int sdk_affinity_plan_range(int N, int P, int num_cu, int wg, int64_t* u0, int64_t* u1, int32_t* first_slot);
/* Host-only: the BLOCK plan of the coarse pass for short sweeps (config #3), for tests.  Since round 5 it is what sdk_affinity_topk takes where its cost
 * model prefers it, with two records per whole sweep (`affinity_variant` 0 = that choice, 7 = always the range plan, 8 / 12 / 13 = the block plan
 * wherever the shape fits with 1 / 2 / 3 records: the A/B pair the tests keep bit-identical).  Unit of work = a block of 32 segments with its whole
 * sweep; workgroup g owns blocks [g q, (g + 1) q), the leftover blocks are swept in `parts` stage ranges by waves with a free second slot.
 * sdk_affinity_block_plan: out6 = {1 = plan taken / 0 = the range plan stays (force != 0: taken whenever the shape fits), q, workgroups, stages per
 * sweep, parts per leftover block, leftover items}.  sdk_affinity_block_plan_wave: wave `wave` (0..7) of workgroup `wg`: out6 = {block of slot 0, block of
 * slot 1 or -1, its first stage, its end stage, its record slot, parts of that block}. */
int sdk_affinity_block_plan(int N, int P, int num_cu, int force, int32_t* out6);
int sdk_affinity_block_plan_wave(int N, int P, int num_cu, int wg, int wave, int32_t* out6);
int sdk_affinity_topk(sdk_ctx* ctx, const float* E, const uint16_t* Eb, const float* resid_e,
                      const float* P, const uint16_t* Pb, const float* resid_p,
                      int N, int Pn, int d, int k, int32_t* idx, float* score,
                      int32_t* n_rescanned, void* ws, size_t ws_bytes, void* stream);

/* ---- k6: spectral clustering pieces on the rectified cosine affinity A = max(E E^T, 0) (BASELINE.json
 *      config #5).  A is never stored: its tiles are recomputed on the matrix cores per application.
 *   sdk_affinity_matvec : Y[row0+i, :] = sum_j max(<e_i, e_j>, 0) * xscale[j] * X[j, :]   for i < rows
 *                         Eb [N,192] bf16 (ALL rows, i.e. the all-gathered embeddings), X [N,kv] fp32,
 *                         kv <= 32, xscale [N] or NULL, Y [N,kv] fp32 (only the owned rows are written).
 *                         Degrees are the case X = ones.  ws: sdk_affinity_matvec_workspace_bytes(N).
 *   sdk_rows_gram       : G [k,k] = X^T Y over n rows (order-fixed two-stage reduction)
 *   sdk_rows_apply      : Y[i,:] = scale[i] * (X[i,:] @ R),  R [k,k] row-major, scale may be NULL
 *   sdk_chol_inverse    : Rinv [k,k] = (L^T)^-1 with (G + G^T)/2 = L L^T, float64 inside (CholeskyQR without leaving the stream);
 *                         *not_spd (device int32, may be NULL) is SET to 1 if a pivot is not a number, not positive, OR at most 1e-6 of its
 *                         diagonal entry (the relative-pivot rule: column i lies within 1e-3 of the span of the columns before it, i.e.
 *                         cond(Y) > ~1e3 - beyond that the fp32 Gram matrix is rounding noise; sdk_set_option "chol_pivot_rtol_ppb", in 1e-9,
 *                         default 1000).  Never cleared: zero it once, run any number of passes, read it at the next host synchronisation.
 *                         Only a non-positive / NaN pivot is replaced (by 1, so the stream keeps running; the result is then meaningless).
 *                         "chol_shift_ppb" > 0: shifted CholeskyQR (G + s I, s = that fraction, in 1e-9, of the mean diagonal entry) for
 *                         nearly rank-deficient blocks; follow it with unshifted passes (cluster.spectral_cluster retries once that way
 *                         when the flag was raised - over-clustered or near-duplicate inputs - before it reports a lost rank)
 *   sdk_sym_eigh        : the Ritz step of sdk_laplacian_topk alone: all eigenpairs of H = (G + G^T)/2, G [k,k] fp32 row-major, 1 <= k <= 32
 *                         (anything else, or a null pointer, is refused with a message and launches nothing).  Cyclic Jacobi in float64 by one
 *                         lane, rounded to fp32 once at the end; never synchronises with the host.  lam DEVICE [k] descending, equal eigenvalues
 *                         in ascending order of the diagonal position they converged at (a diagonal G: its own index); Q DEVICE [k,k] row-major,
 *                         column c = the eigenvector of lam[c], unit length, its largest-magnitude component (the first of equals) positive.
 *   sdk_rows_unit       : rows scaled to unit length
 *   sdk_kmeans_mindist : d2[i] = (first ? : min(d2[i],)) |R[i] - centre|^2      (maximin initialisation)
 *   sdk_kmeans_assign   : label[i] = nearest of kc centres (ties -> lowest), dist2, optional per-256-row-block
 *                         partial sums [nblk, kc, k] and counts [nblk, kc]
 */
/* N at most 2^24 rows (sdk_affinity_matvec, sdk_laplacian_topk, sdk_rows_gram: more is refused, and the sizers then return 0 with sdk_last_error). */
size_t sdk_affinity_matvec_workspace_bytes(int N);
/* Host-only (no device): the mat-vec kernel's work decomposition, for tests.  out4 = {row groups of 512, j stages per group, workgroups,
 * partial-tile slots per group}; *units = groups * stages; workgroup i sweeps the units [i * units / workgroups, (i + 1) * units / workgroups)
 * in (group, stage) order and writes one partial Y tile per group it touches; a group's tiles are summed in slot order. */
int sdk_affinity_matvec_plan(int rows, int N, int num_cu, int32_t* out4, int64_t* units);
int sdk_affinity_matvec(sdk_ctx* ctx, const uint16_t* Eb, int N, int d, int row0, int rows, const float* X,
                        const float* xscale, int kv, float* Y, void* ws, size_t ws_bytes, void* stream);
/* ---- k5 / k6 for a non-Python host.  The Python host layer uses torch.distributed for the same collectives (dist.py).
 *   sdk_allgather       : ONE RCCL all-gather of equal shards (bytes_per_rank each) on the caller's communicator (an ncclComm_t passed as
 *                         void*) and stream: the [N/G, 192] embedding exchange over xGMI.  RCCL is resolved at first use (the copy already in
 *                         the process, else librccl.so.1); the library does not link it.
 *   sdk_allgather_direct: the same exchange as world - 1 PAIRWISE ncclSend / ncclRecv transfers in one RCCL group: on fully connected point-to-point
 *                         xGMI (7 links per GPU) every transfer takes its pair's direct link and all run at once (floor 0.63 ms for 8 x 96 MB),
 *                         whatever algorithm ncclAllGather itself would choose for the size (a ring: 4.4 ms).  Same bytes in `out`.
 *   sdk_laplacian_topk  : top-k eigenpairs of S = D^-1/2 A D^-1/2, A = max(E E^T, 0), by row-sharded subspace iteration (the loop of
 *                         cluster.spectral_cluster: degrees, CholeskyQR2, n_iter x [V all-gather, recomputed-affinity mat-vec, scaling,
 *                         CholeskyQR2], Ritz with a device-side k x k Jacobi eigh): never synchronises with the host.
 *                         Eb_all [N,192] bf16 = ALL embeddings (already gathered); this call owns rows [row0, row0 + rows); V [rows, k] fp32
 *                         in: any full-rank start block (e.g. seeded gaussian), out: the Ritz vectors (columns = eigenvectors, eigenvalue
 *                         descending; signs fixed by a deterministic rule on the k x k Ritz eigenvectors); eigvals DEVICE [k]; not_spd as sdk_chol_inverse (sticky, may be NULL).
 *                         comm NULL: single GPU (rows == N).  comm != NULL: every rank owns N / world rows (equal shards) and calls with the
 *                         same arguments; collectives: all-gather of D^-1/2 and of V per iteration, all-reduce of the k x k Gram matrices. */
int sdk_allgather(sdk_ctx* ctx, const void* shard, void* out, size_t bytes_per_rank, void* comm, void* stream);
int sdk_allgather_direct(sdk_ctx* ctx, const void* shard, void* out, size_t bytes_per_rank, void* comm, void* stream);
size_t sdk_laplacian_topk_workspace_bytes(int N, int k);
int sdk_laplacian_topk(sdk_ctx* ctx, const uint16_t* Eb_all, int N, int row0, int rows, int k, int n_iter, float* V, float* eigvals,
                       int32_t* not_spd, void* ws, size_t ws_bytes, void* comm, int world, void* stream);
size_t sdk_rows_gram_workspace_bytes(int n, int k);
int sdk_rows_gram(sdk_ctx* ctx, const float* X, const float* Y, int n, int k, float* G, void* ws, size_t ws_bytes, void* stream);
int sdk_rows_apply(sdk_ctx* ctx, const float* X, const float* R, const float* scale, int n, int k, float* Y, void* stream);
int sdk_chol_inverse(sdk_ctx* ctx, const float* G, int k, float* Rinv, int32_t* not_spd, void* stream);
int sdk_sym_eigh(sdk_ctx* ctx, const float* G, int k, float* Q, float* lam, void* stream);
int sdk_rows_unit(sdk_ctx* ctx, const float* X, int n, int k, float* Y, void* stream);
int sdk_kmeans_mindist(sdk_ctx* ctx, const float* R, int n, int k, const float* centre, float* d2, int first, void* stream);
int sdk_kmeans_assign(sdk_ctx* ctx, const float* R, int n, int k, const float* centres, int kc, int32_t* label,
                      float* dist2, float* part_sum, int32_t* part_cnt, void* stream);
/* ---- k6, threshold path: centroid-linkage agglomerative clustering (scipy.cluster.hierarchy.linkage(X, "centroid"): same arithmetic in
 *      float64, same layout and numbering).  G independent problems; problem g is rows offsets[g] .. offsets[g+1] of E (fp32 [N_total, dim],
 *      row stride ldE; unit rows as sdk_l2norm writes them), n_g = offsets[g+1] - offsets[g] rows, 1 <= n_g <= 65536, 1 <= dim <= 2048.
 *      offsets is HOST memory [G + 1], strictly increasing from 0.
 *   Z        DEVICE float64 [N_total - G][4]: problem g's n_g - 1 rows start at row offsets[g] - g.  Row t = (id_a, id_b, height, count):
 *            leaves are 0 .. n_g - 1, merge t creates id n_g + t, id_a < id_b, rows in merge order (centroid heights are not monotone).
 *   status   DEVICE int32 [G]: 0 ok; 1 = a non-finite row (or distance) in the problem: none of its Z rows is written; 2 = the merge loop
 *            found no finite pair (non-finite update).  The caller reads it at its next synchronisation.
 *   Distances: d_ij = sqrt(sum_c (e_ic - e_jc)^2) in float64 (difference form).  Merge x into y (x = the lower row of the closest pair; ties:
 *   lowest row, then lowest neighbour): d(k, y') = sqrt(max(0, ((n_x d_kx^2 + n_y d_ky^2) - n_x n_y d_xy^2 / (n_x + n_y)) / (n_x + n_y))),
 *   scipy's centroid Lance-Williams form; the max(0, .) is ours (scipy can return NaN there).  One workgroup per problem runs the merges.
 *   workspace: sdk_centroid_linkage_workspace_bytes (8 n_g^2 bytes of distances per problem + O(n_g)), 256-byte aligned; 0 for arguments
 *   the call refuses.  Every refusal returns non-zero, names the value in sdk_last_error() and launches nothing.
 *   sdk_set_option "ahc_distances_only" 1 (bench knob, tools/ahc_bench.py): stop after the distance and nearest-neighbour kernels (Z not written). */
size_t sdk_centroid_linkage_workspace_bytes(const int32_t* offsets, int G, int dim);
int sdk_centroid_linkage(sdk_ctx* ctx, const float* E, int ldE, int dim, const int32_t* offsets, int G, double* Z, int32_t* status,
                         void* workspace, size_t ws_bytes, void* stream);

/* ---- linked centroid linkage: sdk_centroid_linkage with forbidden pairs and an early stop (the join of speakers across recordings:
 *      cluster.link_rows, diarize.link_speakers).  E, offsets, Z's layout, distances, the update, ties and the limits are sdk_centroid_linkage's.
 *   group    DEVICE int32 [N_total]: rows i != j of one problem with group[i] == group[j] >= 0 are forbidden to each other (a negative group
 *            is a free row); two clusters are forbidden to each other when any row of one is forbidden to any row of the other.
 *   stop     a distance >= 0, or +inf.  Each step merges the ALLOWED live pair of least centroid distance; the problem ends when no allowed
 *            pair is left or that least distance exceeds stop.
 *   merges   DEVICE int32 [G]: the merges made.  Rows merges[g] .. n_g - 2 of the problem's Z are zero.
 *   status   as sdk_centroid_linkage's (1 is judged on the computed distances before any pair is masked; merges[g] is then 0 and the
 *            problem's Z rows are not written).
 *   No forbidden pair and stop = +inf: Z is sdk_centroid_linkage's bit for bit.  stop = t: merges[g] is the number of leading rows of the
 *   stop = +inf run whose height is <= t (the first row above t ends the problem), and those rows are the same.
 *   workspace: sdk_linked_linkage_workspace_bytes (the same size as sdk_centroid_linkage's).  Refusals (a null or misaligned pointer, group
 *   included; ldE < dim; bad offsets; a short workspace; stop negative or NaN) return non-zero, name the value and launch nothing.
 *   sdk_set_option "ahc_distances_only" applies here too (tools/link_bench.py). */
size_t sdk_linked_linkage_workspace_bytes(const int32_t* offsets, int G, int dim);
int sdk_linked_linkage(sdk_ctx* ctx, const float* E, int ldE, int dim, const int32_t* group, const int32_t* offsets, int G, double stop,
                       double* Z, int32_t* merges, int32_t* status, void* workspace, size_t ws_bytes, void* stream);

/* ---- streaming diarization (stream.py states the rule; csrc/stream.hip): a bank of R live streams steps together.  The embedding of the
 *      streams' due chunks is one ordinary batch (sdk_segmentation_forward .. sdk_resnet_forward_masked, sdk_l2norm); everything after it -
 *      the speaker inventory that grows online, the constrained mapping of a chunk's local speakers onto it, the rolling stitch that emits
 *      frames once their latency has passed - is ONE launch per bank step, one workgroup per stream, on a state block that stays on the device.
 *   state    DEVICE, 256-byte aligned, sdk_stream_state_bytes(R, capacity, d) bytes (0 for arguments the calls refuse), opaque.  Per stream:
 *            the emission frontier and the ring's reach (int64), K and the counts n_k (int32 [64]); the float64 sums S [capacity][d] and
 *            the unit centroids S_k / ||S_k|| [capacity][d], renewed whenever a sum changes; the ring of SDK_STREAM_RING frames: chunk
 *            count and count sum (uint16 each) and act [frame][capacity rounded up to 8] uint16.
 *   which / active   DEVICE uint8 [R]: streams with 0 are left alone - their state and their rows of every output stay bit for bit.
 *            sdk_stream_reset alone takes NULL: every stream.
 *   sdk_stream_reset      K = 0, frontier = reach = 0 (sums and ring need no clearing: a founder overwrites its sum, the ring is cleared
 *                         as it comes into reach).  A fresh state block must be reset before its first step.
 *   sdk_stream_step       stream r's chunk: unit rows E [3 r .. 3 r + 2][d] fp32, info [r][3][4] and cls [r][F] (sdk_diarize_masks,
 *                         sdk_powerset_decode), starts [r] int64 = the chunk's first sample.  The chunks of a stream must come in the order
 *                         of their starts and advance by hop (the last one by less); hop >= 270 and latency >= hop are in samples,
 *                         hold = (latency - hop) / 270 frames, and hold + hop / 270 + 2 <= SDK_STREAM_RING: the ring holds every frame
 *                         between the frontier and the newest chunk's reach (a latency of 10 s at any hop fits); delta_new in [0, 2]; max_speakers >= 0 as in sdk_diarize_reconstruct.
 *                         n_end: NULL, or DEVICE int64 [R]: n_end [r] > 0 says that the chunk is the stream's last and the stream ends at that
 *                         sample; no frame from sdk_diarize_frames(n_end [r]) on is then emitted (a zero-padded chunk reaches beyond it).
 *                         -> labels [r][3] int32, score [r][3] fp32, K [r] int32 (speakers after the step), emit_lo [r] int64 and
 *                         emit_n [r] int32: the frames emit_lo .. emit_lo + emit_n - 1 leave the ring as count [r][j] uint8 and
 *                         speakers [r][j][2] int32, j < emit_n <= SDK_STREAM_RING (rows j >= emit_n are not written).
 *   sdk_stream_flush      the end of stream r at n_samples [r] (int64): every frame not yet emitted, up to sdk_diarize_frames(n_samples [r]).
 *   sdk_stream_centroids  of the streams first .. first + count - 1, indexed from first: -> cent [r][capacity][d] fp32 unit rows (rows >= K [r]
 *                         zero), counts [r][capacity] int32 (0 there), K [r] int32, and, where sums is not NULL, the float64 sums
 *                         [r][capacity][d] (rows >= K [r] zero).
 *   d a multiple of 64, at most 512 (sdk_diarize_assign's limit); capacity 1 .. 64; 1 <= F <= SDK_STREAM_RING.  Every sum is float64 in a
 *   fixed order, every output element has one owner, there are no atomics: two runs agree bit for bit.  Refusals (a null or misaligned
 *   pointer, capacity, d, F, hop below 270, latency below hop or beyond the ring, delta_new, a short state block) return non-zero, name the value in
 *   sdk_last_error() and launch nothing. */
#define SDK_STREAM_RING 1024
#define SDK_STREAM_MAX_SPEAKERS 64
int64_t sdk_stream_state_bytes(int R, int capacity, int d);
int sdk_stream_reset(sdk_ctx* ctx, void* state, int64_t state_bytes, int R, int capacity, int d, const uint8_t* which, void* stream);
int sdk_stream_step(sdk_ctx* ctx, const float* E, const int32_t* info, const uint8_t* cls, const int64_t* starts, const uint8_t* active,
                    const int64_t* n_end, int R, int F, int d, int capacity, int hop, int latency, double delta_new, int max_speakers, void* state, int64_t state_bytes,
                    int32_t* labels, float* score, int32_t* K, int64_t* emit_lo, int32_t* emit_n, uint8_t* count, int32_t* speakers,
                    void* stream);
int sdk_stream_flush(sdk_ctx* ctx, const int64_t* n_samples, const uint8_t* active, int R, int capacity, int d, int max_speakers, void* state,
                     int64_t state_bytes, int64_t* emit_lo, int32_t* emit_n, uint8_t* count, int32_t* speakers, void* stream);
int sdk_stream_centroids(sdk_ctx* ctx, const void* state, int64_t state_bytes, int R, int capacity, int d, int first, int count, float* cent,
                         int32_t* counts, int32_t* K, double* sums, void* stream);

/* ---- the nearest-neighbour graph of eigengap spectral clustering (cluster.nmesc_cluster states the rule; csrc/nmesc.hip).  One problem per
 *      call: n rows, 2 <= n <= 65536, P = min(64, n - 1); every pointer is DEVICE memory; every call is enqueued on `stream` and reads nothing back.
 *   sdk_knn_rows     E fp32 [n][d] unit rows, d a multiple of 64, at most 512 -> idx int32 [n][P], cosv float64 [n][P]: row i's P rows j != i of
 *                    largest c(i, j), ties to the lower j, in that order.  c(i, j) is the float64 sum over the columns in ascending order of
 *                    the products E[i][t] E[j][t] (exact in float64), rounded once per addition; it is symmetric bit for bit.  A NaN
 *                    cosine ranks, and is stored, as -inf.  status int32 [2]: the number of rows that hold a non-finite value and the
 *                    lowest of them (INT_MAX: none); the lists are written either way, and those of a problem without such a row are
 *                    not affected by an earlier call that had one.
 *   sdk_knn_reverse  idx -> the incoming edges as CSR: rev_off int32 [n + 1], and for row j the entries rev_off[j] .. rev_off[j + 1] - 1 of
 *                    rev_src / rev_rank int32 [n P]: the rows i that list j, in ascending order of i, and the position of j in i's list.
 *                    Integer counting per block of 256 source rows, a scan, a fill: no order depends on scheduling.  status int32 [2]: the
 *                    entries of idx outside [0, n) (they are skipped) and the lowest row that holds one (INT_MAX: none).
 *                    workspace: sdk_knn_reverse_workspace_bytes(n, P) (4 n ceil(n / 256) bytes of counts + O(n)), 256-byte aligned; 0 for
 *                    arguments the call refuses.
 *   sdk_knn_degree   for 1 <= p <= P: deg int32 [n], deg[i] = p + the entries of row i's reverse list with rank < p (the row sum of
 *                    A_p = B_p + B_p^T, B_p(i, j) = 1 iff j is among the first p entries of list i), and dinv float64 [n] =
 *                    1 / sqrt((double)deg[i]): a correctly rounded square root, then a correctly rounded division.
 *   sdk_knn_matvec   Y = T_p X, T_p = (I + D^-1/2 A_p D^-1/2) / 2, for X fp32 [n][kv], 1 <= kv <= 32, Y fp32 [n][kv], Y != X.  For every
 *                    row i and column c, in float64, each operation rounded once and none fused:
 *                      s = 0;  for r = 0 .. p - 1, j = idx[i][r]:                                  s = s + dinv[j] * X[j][c]
 *                              for e = rev_off[i] .. rev_off[i + 1] - 1 with rev_rank[e] < p, j = rev_src[e]:  s = s + dinv[j] * X[j][c]
 *                      Y[i][c] = (float)(0.5 * (X[i][c] + dinv[i] * s))
 *                    No atomics: one thread owns an element of Y.
 *   sdk_knn_rows_fused  the lists of a MULTI-SCALE affinity (cluster.nmesc_multiscale): E_all fp32 [n_all][d] holds the unit rows of every scale
 *                    stacked, 1 <= n_all <= 8 * 65536; maps int32 [S][n] (device), 1 <= S <= 8, names for base row i and scale s its row
 *                    maps[s][i] of E_all; weights float64 [S] is HOST memory (read before the call returns).  For base rows i != j,
 *                    c_s(i, j) is sdk_knn_rows' cosine of the rows maps[s][i] and maps[s][j] (the same chain, so equal row pairs give
 *                    equal bits), and
 *                      f = 0;  for s = 0 .. S - 1:  f = f + weights[s] * c_s(i, j)      (float64, the product and the sum each rounded once)
 *                    idx / cosv [n][P] are row i's P rows j != i of largest f, ties to the lower j, and their f; a NaN f ranks, and is
 *                    stored, as -inf.  With S = 1, weight 1.0 and the identity map the outputs are sdk_knn_rows' bit for bit.
 *                    status int32 [4]: the rows of E_all that hold a non-finite value AND that a map entry names, and the lowest of
 *                    them (INT_MAX: none); the map entries outside [0, n_all), and the lowest base row i that has one (INT_MAX: none).
 *                    Nothing is read through such an entry (its row counts as zeros) and the lists of that call are not to be trusted.
 *                    No floating-point atomics, one owner per output element.
 *   Refusals (a null pointer, n, d, P other than min(64, n - 1), p outside 1 .. P, kv, S, n_all, a short or misaligned workspace) return
 *   non-zero, name the value in sdk_last_error() and launch nothing. */
int sdk_knn_rows(sdk_ctx* ctx, const float* E, int n, int d, int P, int32_t* idx, double* cosv, int32_t* status, void* stream);
int sdk_knn_rows_fused(sdk_ctx* ctx, const float* E_all, int n_all, int d, const int32_t* maps, const double* weights, int S, int n, int P,
                       int32_t* idx, double* cosv, int32_t* status, void* stream);
size_t sdk_knn_reverse_workspace_bytes(int n, int P);
int sdk_knn_reverse(sdk_ctx* ctx, const int32_t* idx, int n, int P, int32_t* rev_off, int32_t* rev_src, int32_t* rev_rank, int32_t* status,
                    void* workspace, size_t ws_bytes, void* stream);
int sdk_knn_degree(sdk_ctx* ctx, const int32_t* rev_off, const int32_t* rev_rank, int n, int P, int p, int32_t* deg, double* dinv, void* stream);
int sdk_knn_matvec(sdk_ctx* ctx, const int32_t* idx, const int32_t* rev_off, const int32_t* rev_src, const int32_t* rev_rank, const double* dinv,
                   int n, int P, int p, const float* X, int kv, float* Y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDK_HIP_H */
