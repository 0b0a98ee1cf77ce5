/*
 * libavcer_hip.so -- C ABI of the MI355X (gfx950) implementation of AVCER's inference hot path.
 *
 * AVCER (github.com/ElenaRyumina/AVCER) has no FFI/plugin layer: its seam is the Python call surface
 * of four callables and two numpy functions.  Each entry point below replaces one
 * of them; the reference location it stands in for is cited as  ref: <file>:<lines>  relative to the
 * reference's src/ directory.  The Python mirror with the reference's own call signatures lives in
 * avcer_amd/ (models.py, video_pipeline.py, audio_pipeline.py, fusion.py) and binds these symbols
 * with ctypes; INTEGRATION.md shows the stub a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative AVCER_E* code and never throws;
 *     avcer_last_error(ctx) returns a human-readable message for the last failure on that context;
 *   - all tensor pointers are DEVICE pointers owned by the caller unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are asynchronous on it;
 *   - weights and workspace are owned by the context (hipMalloc at load / first use; a call that has to
 *     grow the workspace synchronises the device once);
 *   - one context per (device, host thread): a context is not re-entrant.
 */
#ifndef AVCER_HIP_H
#define AVCER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avcer_ctx avcer_ctx;
typedef void* avcer_stream_t;

enum {
    AVCER_OK = 0,
    AVCER_EINVAL = -1,   /* bad argument / shape */
    AVCER_ENOMEM = -2,   /* device allocation failed */
    AVCER_EHIP = -3,     /* HIP runtime error (message holds hipGetErrorString) */
    AVCER_ESTATE = -4,   /* weights for this model not loaded */
    AVCER_EFORMAT = -5   /* packed weight blob malformed */
};

/* arithmetic mode of the MFMA contractions */
enum {
    AVCER_MODE_FP32 = 0, /* f32 operands, v_mfma_f32_32x32x2_f32: exact f32 FMA chains */
    AVCER_MODE_BF16 = 1, /* bf16 operands / f32 accumulate, v_mfma_f32_16x16x32_bf16: throughput mode, NOT parity-grade */
    AVCER_MODE_F16X3 = 2 /* the fast parity mode: f32-grade activations and results; every operand is carried as an fp16
                            pair hi + lo (11 + 11 significand bits) and every product as ah*wh + ah*wl + al*wh on
                            v_mfma_f32_16x16x32_f16 with f32 accumulation: 3 MFMAs per product, ~7e-8 relative error per
                            contraction (rounds 1-3 split into bf16 pairs: 4.5e-6; that mode was AVCER_MODE_BF16X3) */
};
/* Range contract of AVCER_MODE_F16X3 (csrc/split_dev.h).  Activations are stored unscaled as fp16 pairs: every
 * intermediate activation must satisfy |x| < 65504.  A larger value becomes +-inf in its hi half and NaN in hi + lo, and the
 * NaN reaches the outputs: an overflow is never a wrong finite number (tests/test_gpu_edges.py).  Because NaN is also what
 * the reference legitimately returns for an empty audio window (get_prob_audio_8_cl.py:78-92), the library COUNTS the event
 * itself: avcer_x3_overflow_count below; the host mirrors read it once per call and repeat the call in AVCER_MODE_FP32
 * (no range limit) when it is not zero.  Below 2^-3 the lo half is an fp16 subnormal: a small element carries an ABSOLUTE
 * error of at most 2^-25 -- the usable window of the f32-grade RELATIVE bound is [2^-3, 65504).  Weights are multiplied
 * by one power of two per matrix before the split (largest |w| -> [2^14, 2^15)); the inverse, also a power of two, rides
 * behind the split data (AVCER_SPLIT_TRAILER) and every consumer folds it into its epilogue, so no result depends on it.
 * Error bounds of the two parity-grade modes against the reference's CPU path are in DESIGN.md section 6 and asserted by
 * tests/test_gpu_parity_breadth.py: ONE gate of 1e-4 on probabilities for both modes at 1 x, 4 x and 8 x the synthetic
 * generator's logit scale. */

/* Bumped whenever a struct layout, an argument list or a buffer size of this header changes incompatibly; the Python binding
 * refuses a library whose avcer_abi_version() differs (avcer_amd/_lib.py).
 *   2: avcer_conv_desc grew r_sub / r_h / r_w / tile_m, avcer_bneck_chain gained out_step, avcer_set_option left (round 3);
 *      split weight buffers carry a trailer and AVCER_MODE_BF16X3 became AVCER_MODE_F16X3 (round 4).
 *   3: avcer_x3_overflow_count, avcer_profile_read_families; avcer_bneck_chain gained w2_frags (round 5).
 *   4: avcer_source_hash, avcer_set_static_back_batch, avcer_set_static_lanes, avcer_set_static_lane_range, avcer_face_decode_batch, avcer_track_faces,
 *      avcer_lsap, avcer_profile_read_launches (round 6).
 *   5: avcer_static_forward_cam, avcer_crop_resize_linear, avcer_cam_render (Grad-CAM heat maps).
 *   6: avcer_resample (source audio -> mono at the model's rate).
 *   7: avcer_weight_search_counts (fusion weight search: per-candidate argmax counts).
 *   8: avcer_audio_head_kind, avcer_audio_forward_features, avcer_gru_layer, AVCER_FAM_GRU (the GRU-head audio model ExprModelV1).
 *      avcer_fuse_videos (fusion of a set of unequal videos in one launch) joined under 8: one more symbol, nothing that
 *      existed changed; a binary without it is refused by its source hash.
 *      avcer_face_kind and avcer_dwsep (the MobileNet-0.25 RetinaFace detector: avcer_load_face / avcer_face_forward take either
 *      variant's blob) joined under 8 the same way: two more symbols, no struct layout or argument list changed.
 *      avcer_s3fd_num_priors, avcer_s3fd_detect and the kernel-level entries avcer_s3fd_stem, avcer_maxpool2, avcer_s3fd_head (the
 *      S3FD detector: avcer_load_face / avcer_face_forward take its blob as kind 3) joined under 8 the same way.
 *      avcer_jpeg_probe, avcer_jpeg_entropy_batch, avcer_jpeg_tiles, avcer_jpeg_rgb and their descriptor struct (JPEG crop files
 *      decoded behind a host entropy pass) joined under 8 the same way.
 *      avcer_jpeg_quant_tables, avcer_jpeg_plan, avcer_jpeg_forward, avcer_jpeg_write_batch (the same files WRITTEN: forward pass
 *      on the device, entropy coding on the host) joined under 8 the same way: four more symbols, the descriptor unchanged.
 *      avcer_jpeg_pack (entropy coding on the device: whole files leave it) joined under 8 the same way: one more symbol.
 *      avcer_jpeg_scan_batch, avcer_jpeg_unpack, avcer_jpeg_unpack_host with their structs avcer_jpeg_tab and avcer_jpeg_scan: entropy
 *      DECODING on the device, joined under 8 the same way: three more symbols, the descriptor unchanged.
 *      avcer_attention_long, avcer_set_audio_max_tokens, avcer_audio_max_tokens (audio windows past 256 tokens: attention that
 *      streams key tiles through LDS) joined under 8 the same way: three more symbols, nothing that existed changed.
 *      avcer_jpeg_roundtrip_tiles, avcer_jpeg_roundtrip_rgb (face crops as the files of stage 0 hold them, without the files)
 *      joined under 8 the same way: two more symbols, the descriptor unchanged.
 *      avcer_bneck_tail (the stage-3 tail kernel on caller tensors, for kernel-level tests) joined under 8 the same way: one more symbol.
 *      avcer_jpeg_frames, avcer_jpeg_entropy_batch_ex, avcer_jpeg_scan_batch_ex and the flag AVCER_JPEG_STD_TABLES (Motion-JPEG frames
 *      of an AVI file decoded into the frame batch) joined under 8 the same way: three more symbols, no struct or argument list
 *      that existed changed.
 *      avcer_annotate_frames (the result video's boxes and labels drawn into the frame batch) and its record struct avcer_draw_item
 *      joined under 8 the same way: one more symbol.
 *      avcer_tracker_create, avcer_tracker_push, avcer_tracker_last_error, avcer_tracker_destroy (the face tracker behind a handle:
 *      a video pushed in passes) joined under 8 the same way: four more symbols; avcer_track_faces keeps its argument list.
 *      avcer_resize_frames, avcer_resize_form (PIL's Image.resize of a frame batch on the device, for the detector on a smaller
 *      copy) joined under 8 the same way: two more symbols, nothing that existed changed.
 *      avcer_chart_series, avcer_chart_path (the traces of the prediction timeline chart) and the record struct avcer_chart_plan
 *      joined under 8 the same way: two more symbols, nothing that existed changed.
 *      avcer_eval_tables, avcer_eval_tables_workspace, avcer_eval_confusion (a dataset's per-video CSV tables turned into the
 *      trues / preds tables of the weight search, and a model or fusion scored on them) joined under 8 the same way: three more
 *      symbols, nothing that existed changed.
 *      avcer_dib_frames (uncompressed BGR video of an AVI file unpacked into the frame batch) joined under 8 the same way: one
 *      more symbol, nothing that existed changed.
 *      avcer_window_votes (the audio model over a corpus: softmax, argmax and per-file majority vote of the window logits) joined
 *      under 8 the same way: one more symbol, nothing that existed changed.
 *      avcer_set_skip_unread_rows, avcer_bneck_chain_keep, avcer_bneck_tail_keep (the block in front of a strided last block
 *      stores only the rows that block reads) joined under 8 the same way: three more symbols, nothing that existed changed.
 *      avcer_window_losses, avcer_ccc (validation of audio checkpoints: the epoch loss of a corpus's window logits and the
 *      concordance coefficient) joined under 8 the same way: two more symbols, nothing that existed changed.
 *      avcer_head_fit, avcer_head_apply (fitting the audio classifier head on extracted features, many runs a launch, and the
 *      logits of a feature table under many heads) joined under 8 the same way: two more symbols, nothing that existed changed.
 *      avcer_wave_augment (the waveform augmentations of the training windows) and its record struct avcer_augment_rec, and
 *      avcer_head_fit_views (avcer_head_fit with a table of feature rows per augmented view) joined under 8 the same way: two more
 *      symbols, nothing that existed changed. */
#define AVCER_ABI_VERSION 8
int avcer_abi_version(void);
/* Hash (16 hex digits) of the sources and headers this binary was compiled from, embedded at build time by
 * avcer_amd/build.py (source_hash()).  The Python binding refuses a library whose hash differs from the tree's, and bench.py
 * prints it beside the tree's hash: a stale binary with the right ABI number cannot be measured under a fresh label. */
const char* avcer_source_hash(void);

int avcer_ctx_create(int device, avcer_ctx** out);
void avcer_ctx_destroy(avcer_ctx* ctx);
const char* avcer_last_error(const avcer_ctx* ctx);

/* Run-time signal of AVCER_MODE_F16X3's range contract.  *count = how many GPU threads of this context's launches have
 * turned a FINITE activation of magnitude >= 65520 into an infinite fp16 hi half since the last reset (every split site:
 * GEMM / chain / stem epilogues, LayerNorm and GELU outputs, attention Q / K / V, the on-the-fly split of f32 operands).
 * 0: any NaN in an output came in through the input -- the reference's own result for an empty audio window.  > 0: outputs
 * produced since the last reset may hold NaN where the reference (fp32, no range limit) holds numbers
 *   ref: get_prob_video.py:107-112, get_prob_audio_8_cl.py:87-92 (fp32 forward passes)
 * -- repeat the call with AVCER_MODE_FP32.  Waits for `stream`; reset != 0 zeroes the counter behind the read.
 * count == NULL with reset != 0: an asynchronous reset queued on `stream`, nothing read, nothing waited for -- what a guarded call
 * puts in front of its launches so that counts left by earlier work on the context are not charged to it.  The counter sees the
 * launches of every stream; the read orders only behind `stream`, so join side streams into it first. */
int avcer_x3_overflow_count(avcer_ctx* ctx, int reset, int64_t* count, avcer_stream_t stream);

/* Packed weights (host pointers; the library copies them to the device and owns the copy).
 * Blob layout: see avcer_amd/packing.py (header "AVCERW01", tensor table, 64-byte aligned f32 payloads).
 *   ref: get_prob_video.py:22-25 (ResNet50 state_dict), :51-54 (LSTM state_dict),
 *        get_prob_audio_8_cl.py:52-66 (ExprModelV3 state_dict) */
int avcer_load_static(avcer_ctx* ctx, const void* blob_host, size_t nbytes);
int avcer_load_dynamic(avcer_ctx* ctx, const void* blob_host, size_t nbytes);
int avcer_load_audio(avcer_ctx* ctx, const void* blob_host, size_t nbytes);

/* Static visual model on face tiles.
 *   ref: data/utils.py:19-39 (pth_processing: NEAREST resize to 224, u8 HWC -> f32, RGB->BGR, mean subtract)
 *        architectures/video.py:115-133 (ResNet.extract_features / forward)
 *        get_prob_video.py:47-49,103-112 (fc1 forward hook "features", softmax(dim=1))
 * frames_hwc  u8 [n, in_h, in_w, 3] RGB.   logits/probs f32 [n,7] (video class order), feats f32 [n,512]
 * (fc1 output BEFORE ReLU).  Any of the three outputs may be NULL. */
int avcer_static_forward(avcer_ctx* ctx, const uint8_t* frames_hwc, int n, int in_h, int in_w, int mode,
                         float* logits, float* probs, float* feats, avcer_stream_t stream);

/* Frames per FRONT pass of the static CNN (stem, stage 1, first block of stage 2: the 55 x 55 tensors), 1..1024 (default 1024).
 * Results do not depend on it (every kernel's arithmetic per frame is independent of the batch around it). */
int avcer_set_static_batch(avcer_ctx* ctx, int frames);
/* Frames per BACK pass (rest of stage 2, stages 3-4, tail), 1..2048, or 0 = two front passes (the default: 2048 at the default
 * front pass).  The late layers' grids are small, so the back wants as many frames per launch as the 4 GiB descriptors allow
 * whatever the front pass is.  A scheduling knob like the one above: results do not depend on it. */
int avcer_set_static_back_batch(avcer_ctx* ctx, int frames);
/* Lanes of a static-CNN call: 2 (default) = a call of 32-2048 frames (avcer_set_static_lane_range) runs as two half-batches on two
 * HIP streams (the context's own second stream, forked from and joined into `stream` by events; a second workspace): below a few
 * thousand frames the grids of stages 3-4 are a fraction of a round of block slots, and the two halves fill each other's tails:
 * -4 % at 32 frames, -8 ... -12 % at 48-192, -5 % at 256-512, -2 ... -3 % at 640-1536, -1.7 % at 2048 (tools/two_lane_sweep.py,
 * profiles/r06_two_lane_sweep.txt; at 8 frames +4 %: latency chains).  1 = always on `stream` alone.  Results are bit-identical
 * either way (a frame's result does not depend on the batch around it); calls made while avcer_profile_enable is on or a debug tap
 * is armed are serial regardless, so that per-launch events stay meaningful. */
int avcer_set_static_lanes(avcer_ctx* ctx, int lanes);
/* The call sizes that take the two-lane schedule: min_frames <= n <= max_frames, 2 <= min <= max <= 4096 (default 32 .. 2048).
 * A scheduling knob: results do not depend on it. */
int avcer_set_static_lane_range(avcer_ctx* ctx, int min_frames, int max_frames);
/* AVCER_MODE_F16X3 only.  The last block of stages 1-3 of the recognition CNN is evaluated at the positions (2 oy, 2 ox) alone, so
 * of the output of the block in front of it (its residual) only those rows are ever read.  on != 0 (default): that block's fused
 * launch stores those rows only, at their full-grid addresses (csrc/fused.hip KEEP): 8.4 GB fewer bytes written per 2048 frames.
 * 0: every row is stored.  Results are bit-identical either way; calls made while a debug tap is armed store every row regardless,
 * because the blk / chain_out / tail_out taps return the whole tensor. */
int avcer_set_skip_unread_rows(avcer_ctx* ctx, int on);

/* The same model on an already preprocessed tensor, i.e. the exact argument of the reference's
 * `pth_model_static(x)`:  x f32 [n,3,224,224] (BGR, mean-subtracted).   ref: get_prob_video.py:103-109 */
int avcer_static_forward_nchw(avcer_ctx* ctx, const float* x, int n, int mode, float* logits, float* probs,
                              float* feats, avcer_stream_t stream);

/* LSTM window assembly: out[w, s, :] = relu(feats[idx[w, s], :]).
 *   ref: get_prob_video.py:115-123 (F.relu(features), 10-deep sliding window, first feature replicated x10)
 * feats f32 [*,512], idx i32 [nwin,10] (device), out f32 [nwin,10,512]. */
int avcer_gather_windows(avcer_ctx* ctx, const float* feats, const int32_t* idx, int nwin, float* out,
                         avcer_stream_t stream);

/* Dynamic visual model on windows of 10 ReLU'd fc1 features.
 *   ref: architectures/video.py:169-185 (LSTMPyTorch.forward), get_prob_video.py:122-129
 * windows f32 [n,10,512] -> logits f32 [n,7] (raw logits, no softmax). Always f32 arithmetic. */
int avcer_dynamic_forward(avcer_ctx* ctx, const float* windows, int n, float* logits, avcer_stream_t stream);
/* Same with an arithmetic mode: AVCER_MODE_F16X3 runs the projections on the split-fp16 MFMA (f32 state, f32-grade
 * results); AVCER_MODE_BF16 keeps them in f32 (the recurrence is latency-bound, not worth a third weight copy). */
int avcer_dynamic_forward_mode(avcer_ctx* ctx, const float* windows, int n, int mode, float* logits,
                               avcer_stream_t stream);

/* Audio model on padded waveform windows.
 *   ref: get_prob_audio_8_cl.py:87-92 (HF feature-extractor normalisation + audio_model(x))
 *        architectures/audio_8_cl.py:179-190 (ExprModelV3.forward), architectures/attention_layers.py:221-267
 *        transformers==4.36.2 Wav2Vec2Model (third party, config of audeering/wav2vec2-large-robust-12-ft-emotion-msp-dim)
 * wav f32 [n,t] (already padded to the window), normalize != 0 applies (x-mean)/sqrt(var+1e-7) per row first.
 * logits f32 [n, n_classes] raw logits (n_classes = 8 for ExprModelV3, 7 for ExprModelV2 weights). */
int avcer_audio_forward(avcer_ctx* ctx, const float* wav, int n, int t, int normalize, int mode,
                        float* logits, avcer_stream_t stream);
int avcer_audio_num_classes(const avcer_ctx* ctx);
/* Which head the loaded audio weights hold, recognised by avcer_load_audio from the blob's tensor names: 0 = no audio model
 * loaded, 1 = the two-layer GRU of ExprModelV1 (gru1.whh.w present), 3 = the two TransformerLayers of ExprModelV2 / V3
 * (tl1.qkv.w present).  A blob with neither or both is refused with AVCER_EINVAL.  avcer_audio_forward runs whichever is loaded.
 *   ref: architectures/audio_8_cl.py:18-72 (ExprModelV1), :75-128 (V2), :131-190 (V3); audio_7_cl.py likewise */
int avcer_audio_head_kind(const avcer_ctx* ctx);
/* avcer_audio_forward that also copies out the pooled head activations (after AdaptiveAvgPool1d(1) + ReLU, before the last
 * Linear): features f32 [n, 256] for ExprModelV1, [n, 1024] for V2 / V3; may be NULL (then this IS avcer_audio_forward).
 *   ref: the second value of the reference's get_features, audio/models/audio_expr_models.py:180-191,
 *        audio_expr_models_7_cl.py:63,130,205; consumed at net_trainer.py:512 */
int avcer_audio_forward_features(avcer_ctx* ctx, const float* wav, int n, int t, int normalize, int mode,
                                 float* logits, float* features, avcer_stream_t stream);

/* The longest window, in wav2vec2 tokens (one per 320 samples: 20 ms), that avcer_audio_forward / _features accept for the loaded
 * audio model.  Default 256 (about 5.1 s), what the attention kernels that keep a whole head's K and V in LDS can hold; range
 * 256 .. AVCER_AUDIO_MAX_TOKENS (5000 = 100 s, the rows of the reference's `pe` buffer, attention_layers.py:194-211 -- its own and
 * only length limit).  Windows of at most 256 tokens run the same launches as before whatever the limit is (bit-identical
 * results); longer ones run avcer_attention_long's kernels.  AVCER_ESTATE without a loaded audio model; AVCER_EINVAL outside
 * the range, or when the loaded transformer head's `pe` tensor has fewer rows (packing.pack_audio(sd, pe_rows=...)); the GRU head
 * has no such tensor.  avcer_load_audio resets the limit to 256: it belongs to the loaded model.
 *
 * Windows per pass: min(n, 128) at <= 256 tokens (unchanged launches, unchanged bits); max(1, 128 * 256 / tokens) above, so a
 * pass never holds more than the 32768 token rows of 128 x 256 and the carved workspace stays what it was: 128 windows of 256
 * tokens carve 9.8 GiB in the f32 and x3 modes (extractor layers 0-2: 4.0 + 2 x 2.0 GiB; 32768 token rows x 56 KiB: 1.75 GiB).
 * PEAK at 5000 tokens (one pass = 6 windows of 1 600 080 samples): 9.0 GiB in the f32 and x3 modes (extractor 3.66 + 2 x 1.83 GiB,
 * 30000 token rows 1.6 GiB, the normalised waveform and the head 0.1 GiB), 4.8 GiB in the bf16 mode.  A pass is shortened further
 * where its largest contraction operand, the first extractor layer's output [windows, samples / 5, 512], would reach the 4 GiB
 * range of a buffer descriptor (6 x 320015 x 512 x 4 B = 3.66 GiB fits); every other avcer_conv_desc of the audio path is smaller.
 * Nothing else of the forward has a fixed extent in the token count: add-PE, the positional conv, the max-pool, the head's
 * convolutions and the GRU layer's time loop are shaped by it (64-bit element indices throughout). */
#define AVCER_AUDIO_MAX_TOKENS 5000
int avcer_set_audio_max_tokens(avcer_ctx* ctx, int tokens);
int avcer_audio_max_tokens(const avcer_ctx* ctx);

/* Window slicing + padding of one waveform.
 *   ref: get_prob_audio_8_cl.py:78-86, data/utils.py:63-71 (pad_wav, "repeat"), :74-89 (pad_wav_zeros, "mean"/"constant")
 * wav f32 [len]; starts/ends i32 [n] (device) sample ranges; out f32 [n, window];
 * mode 0 = pad with the chunk mean (NaN for an empty chunk, as torch.mean does), 1 = zeros, 2 = repeat
 * (an empty chunk makes the reference raise ZeroDivisionError, data/utils.py:66; the host mirror raises the same,
 * and the kernel itself writes NaN for such a row instead of indexing with i % 0). */
int avcer_audio_chunks(avcer_ctx* ctx, const float* wav, const int32_t* starts, const int32_t* ends, int n,
                       int window, int mode, float* out, avcer_stream_t stream);

/* Source audio -> mono float32 at the model's rate: sample conversion, downmix and resampling in one launch.
 *   ref: data/utils.py:50-57 (torchaudio.load -> float32 [C, L] = int16 / 32768; wav.mean(dim=0) when C > 1;
 *        torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults)
 *        torchaudio==2.1.2 functional/functional.py _get_sinc_resample_kernel, _apply_sinc_resample_kernel (third party, BSD-2:
 *        resampling_method "sinc_interp_hann", lowpass_filter_width 6, rolloff 0.99)
 * With g = gcd(orig, new), o = orig / g, n = new / g:  base = min(o, n) * 0.99,  width = ceil(6 * o / base),
 *   k[p][j] = cos(t * pi / 12)^2 * sinc(pi * t) * base / o,  t = clamp((-p / n + (j - width) / o) * base, -6, 6),
 *   p in [0, n), j in [0, 2 * width + o),  sinc(0) = 1,  stored as float32;
 *   y[q * n + p] = sum_j k[p][j] * x[q * o + j - width],  x = 0 outside [0, len);  n_out = ceil(n * len / o).
 * The clamp makes the window zero outside |t| < 6: per phase only `span` consecutive taps from index first[p] on can be
 * non-zero, and the kernel works on that compact table (leaving out a zero tap changes no bit of the sum):
 *   taps  f32 [span][n] (device), TAP-MAJOR: taps[j * n + p] = k[p][first[p] + j];   first i32 [n] (device),
 *   0 <= first[p] and first[p] + span <= 2 * width + o for every p (the kernel clamps its staging index to both ends, so a
 *   table that breaks this yields wrong numbers, never a read outside its buffer).  avcer_amd.audio_pipeline.resample_plan builds the table on the host with
 *   torchaudio's own operations and dtypes.  Each output is accumulated in f64 (f32 products are exact there) and rounded
 *   to f32 once at the end: one f32 rounding away from the exact sum, at most as far from it as the reference's f32 conv1d.
 * src: AVCER_PCM_S16_INTERLEAVED = int16 [len][channels] as the frames lie in a WAV file, converted as s / 32768;
 *      AVCER_PCM_F32_PLANAR = f32 [channels][len] (or [len] with channels = 1).  channels > 1: the f32 sum over the channels
 *      in channel order divided by their number (exact for <= 2 channels); 1 <= channels <= AVCER_RESAMPLE_MAX_CHANNELS.
 * taps == NULL (then first == NULL, o = n = 1): equal rates, conversion and downmix alone, n_out = len (utils.py:54).
 * Limits (AVCER_EINVAL beyond them, there is no other path): o <= AVCER_RESAMPLE_MAX_O, n <= AVCER_RESAMPLE_MAX_N,
 * span <= AVCER_RESAMPLE_MAX_SPAN, len <= AVCER_RESAMPLE_MAX_LEN.  They cover every pair of the common rates 8000, 11025, 16000,
 * 22050, 32000, 44100, 48000, 96000 into 16000 (the largest: n = 640 at 11025, o = 441 at 44100, span 73 at 96000).
 * out f32 [n_out]; n_out is checked against the rule above.  len = 0: nothing is launched.  No host synchronisation. */
enum { AVCER_PCM_S16_INTERLEAVED = 0, AVCER_PCM_F32_PLANAR = 1 };
#define AVCER_RESAMPLE_MAX_O 2048
#define AVCER_RESAMPLE_MAX_N 1024
#define AVCER_RESAMPLE_MAX_SPAN 128
#define AVCER_RESAMPLE_MAX_CHANNELS 8
#define AVCER_RESAMPLE_MAX_LEN 2147483647LL
int avcer_resample(avcer_ctx* ctx, const void* src, int src_kind, int64_t len, int channels, const float* taps,
                   const int32_t* first, int o, int n, int span, int width, float* out, int64_t n_out, avcer_stream_t stream);

/* Fusion weight search: for each of `w` candidate weight sets, how often the weighted sum of `m` probability tables picks each
 * class, and how often that pick is the label.  The reference's objective (get_metrics_for_fusion: precision, F1 and recall of
 * classes 1..6 from sklearn's classification_report) is a function of these integers and the labels' own histogram, which
 * avcer_amd/weight_search.py evaluates on the host: no tolerance is involved anywhere.
 *   ref: data/utils.py:151-154 (get_weights_prob_model: predictions[0] * weights[k, 0], then += predictions[i] * weights[k, i],
 *        np.argmax(axis=-1)), :176 (get_weights_v_model) and :200 (get_weights_av_model: the same sum with one scalar weight per
 *        model), :115-122 (get_metrics_for_fusion); driven from get_pred_video.py:346-390 and get_pred_av.py:339-405
 * preds f64 [m][n][c], labels i32 [n], weights f64 [w][m][c] (a grid candidate repeats its scalar over the classes), all on the
 * device.  Per frame i and candidate k, in f64 with numpy's operation order:
 *   f[j] = preds[0][i][j] * weights[k][0][j];   f[j] = f[j] + preds[q][i][j] * weights[k][q][j]  for q = 1 .. m-1
 * where every product and every sum rounds on its own (no FMA contraction: a fused sum moves near-ties to another class);
 *   a = the first index of the maximum of f, a NaN counting as the maximum (np.argmax: the first NaN wins);
 *   pred[k][a] += 1;   tp[k][a] += 1 if labels[i] == a.   A label outside [0, c) matches no class and counts in no tp.
 * tp, pred i32 [w][c]: zeroed by the call itself in stream order, then accumulated with integer atomics, so a result does not
 * depend on the order of the blocks and two calls give the same bits.  Candidates are independent: any split of `w` into
 * several calls gives the same rows.
 * Limits (AVCER_EINVAL beyond them): 1 <= m <= AVCER_SEARCH_MAX_MODELS, 2 <= c <= AVCER_SEARCH_MAX_CLASSES,
 * 1 <= n <= AVCER_SEARCH_MAX_FRAMES, 1 <= w <= AVCER_SEARCH_MAX_CANDIDATES.  No host synchronisation. */
#define AVCER_SEARCH_MAX_MODELS 4
#define AVCER_SEARCH_MAX_CLASSES 8
#define AVCER_SEARCH_MAX_FRAMES 2147483647LL
#define AVCER_SEARCH_MAX_CANDIDATES 16777216
int avcer_weight_search_counts(avcer_ctx* ctx, const double* preds, const int32_t* labels, int64_t n, int m, int c,
                               const double* weights, int w, int32_t* tp, int32_t* pred, avcer_stream_t stream);

/* Per-frame mean of window logits.
 *   ref: get_prob_audio_8_cl.py:94-101 (logits replicated for frames [lo,hi) of each window),
 *        run.py:90 (audio_df.groupby("frames").mean())
 * win_logits f32 [n_win, c], frame_lo/hi i32 [n_win]; out f32 [n_frames, c]; count i32 [n_frames]
 * (count 0 -> row left as zeros: no window covers that frame). */
int avcer_audio_frame_mean(avcer_ctx* ctx, const float* win_logits, const int32_t* frame_lo, const int32_t* frame_hi,
                           int n_win, int c, int n_frames, float* out, int32_t* count, avcer_stream_t stream);

/* RetinaFace-R50 detector network (row f4).
 *   ref: retina_face/retina_face.py:46-115 (RetinaFace, phase "test"), retina_face_net.py:42-101 (SSH, FPN), torchvision
 *        ResNet-50 body (layer2/3/4 returned), retina_face_predictor.py:59-65 (pixels minus 104, 117, 123)
 * avcer_load_face: packed weights (avcer_amd.packing.pack_face of RetinaFace(cfg_re50).state_dict()).
 * avcer_face_forward: frames u8 [n,h,w,3] in cv2's BGR order (rgb != 0: RGB, flipped first, as the predictor does),
 *   any h, w >= 32 -> loc f32 [n,P,4], conf f32 [n,P,2] (softmaxed), landms f32 [n,P,10] with
 *   P = avcer_face_num_priors(h, w) rows in PriorBox order; feed them to avcer_face_decode. */
int avcer_load_face(avcer_ctx* ctx, const void* packed, size_t nbytes);
int avcer_face_num_priors(int h, int w);
/* The same entry points serve the reference's second detector, RetinaFace(cfg_mnet) ("mobilenet0.25": MobileNetV1 body,
 * retina_face_net.py:103-125, FPN / SSH at 64 channels with LeakyReLU(0.1), config.py:3-20): avcer_load_face takes the blob
 * pack_face makes of that state dict (it records the kind), and avcer_face_forward runs it with the same arguments and the same
 * P rows -- cfg_mnet and cfg_re50 share min_sizes, steps, variance and clip.  Modes: AVCER_MODE_FP32 and AVCER_MODE_F16X3;
 * AVCER_MODE_BF16 returns AVCER_EINVAL for this variant.  Loading a blob frees the previous detector and all its lazy copies.
 * avcer_face_kind: 0 = no detector loaded, 1 = RetinaFace-R50, 2 = RetinaFace-MobileNet-0.25, 3 = S3FD.
 *
 * The third detector, S3FD (s3fd/s3fd_net.py: VGG-16 trunk at full frame resolution, fc6 / fc7, four extras, L2Norm on the first
 * three of six head levels, ONE anchor per position), goes through the same pair: avcer_load_face takes the blob pack_face makes of
 * S3FDNet.state_dict(), avcer_face_forward runs it.  What differs for kind 3:
 *   - `rgb` means what it means to S3FDPredictor.__call__ (s3fd_predictor.py:45-52): the network eats RGB minus (123, 117, 104);
 *     rgb == 0 flips the BGR frame first;
 *   - there are no landmarks: `landms` must be NULL (non-NULL is AVCER_EINVAL; for kinds 1 and 2 NULL is);
 *   - loc f32 [n,P,4], conf f32 [n,P,2] (level 0's max-out background label taken, softmaxed) with P = avcer_s3fd_num_priors(h, w)
 *     rows in the reference's order: level by level, row-major within a level.  Per axis, with floor division: a = h/2, b = a/2,
 *     f0 = b, f1 = ceil(b/2), f2 = f1/2, f3 = f2/2, f4 = (f3-1)/2+1, f5 = (f4-1)/2+1; P = sum fh_i * fw_i (360 x 640: 19 175);
 *   - h, w >= 32; AVCER_MODE_FP32 and AVCER_MODE_F16X3 only (AVCER_MODE_BF16 is AVCER_EINVAL).  In AVCER_MODE_F16X3 the trunk's
 *     activations are sp32 pairs and every contraction epilogue counts for avcer_x3_overflow_count; the stem (conv1_1 from the u8
 *     frame) and the heads are f32 arithmetic.  Feed loc / conf to avcer_s3fd_detect. */
int avcer_face_kind(const avcer_ctx* ctx);
int avcer_s3fd_num_priors(int h, int w);
int avcer_face_forward(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int rgb, int mode, float* loc,
                       float* conf, float* landms, avcer_stream_t stream);

/* The post-decode half of RetinaFacePredictor.__call__ for a batch of frames, on the device:
 *   ref: retina_face/retina_face_predictor.py:86-108 (confidence floor, NMS, top-k, final threshold),
 *        retina_face/py_cpu_nms.py:11-39 (greedy NMS, "+1 pixel" areas, visit order = descending score).
 * dets f32 [n_frames, n_priors, 15] as avcer_face_decode writes them; out f32 [n_frames, top_k, 15] receives, per frame,
 * the kept rows in the reference's order; out_n i32 [n_frames] their number.  nms_top_k <= 6144, top_k <= 1024.
 * Equal scores are visited HIGHER prior index first: the reference's `scores.argsort()[::-1]` is an ascending sort read
 * backwards, so this is its order wherever that sort keeps ties in index order (`kind="stable"`; numpy's default sort on
 * short arrays).  On long arrays numpy's default sort does not define the order of ties, so for exactly tied scores a
 * given numpy build may visit (and keep) a different member of the tie. */
int avcer_face_nms(avcer_ctx* ctx, const float* dets, int n_frames, int n_priors, float conf_thresh, float nms_thresh,
                   int nms_top_k, int top_k, float threshold, float* out, int32_t* out_n, avcer_stream_t stream);

/* S3FD's post-processing for a batch of frames, on the device, without a host synchronisation:
 *   ref: s3fd/utils.py:6-24 (decode), :94-128 (nms_np), :131-171 (Detect), s3fd/s3fd_predictor.py:54-68 (the threshold loop).
 * loc f32 [n_frames, n_priors, 4] and conf f32 [n_frames, n_priors, 2] as avcer_face_forward writes them for kind 3, priors f32
 * [n_priors, 4] (PriorBox: face_tiles.s3fd_prior_boxes).  Per frame, in the reference's order: boxes are decoded in NORMALISED
 * coordinates with its rounding sequence (centre and size, x0 = cx - w/2, x1 = x0 + w); candidates are score > conf_thresh
 * (strict); they are visited in descending score, at most nms_top_k of them, equal scores HIGHER prior index first (see
 * avcer_face_nms); greedy NMS with area = (x1-x0)*(y1-y0) -- no "+1" -- keeps a box when iou <= nms_thresh; of the kept boxes
 * the first min(count, top_k), of those the prefix with score >= threshold; the boxes are multiplied by (w, h, w, h) in f32 last.
 * out f32 [n_frames, top_k, 5] = x0, y0, x1, y1 in pixels, score; out_n i32 [n_frames] the rows of each frame.
 * nms_top_k <= 6144, top_k <= 1024, n_frames <= 65535. */
int avcer_s3fd_detect(avcer_ctx* ctx, const float* loc, const float* conf, const float* priors, int n_frames, int n_priors, int im_h,
                      int im_w, float var0, float var1, float conf_thresh, float nms_thresh, int nms_top_k, int top_k, float threshold,
                      float* out, int32_t* out_n, avcer_stream_t stream);

/* Face stage ("next" row f4): the arithmetic either side of the RetinaFace network.
 *   avcer_face_decode  ref: data/face_detection/ibug/face_detection/retina_face/retina_face_predictor.py:70-82,
 *                            box_utils.py:210-249 (decode, decode_landm), scaled to pixels
 *     loc f32 [P,4], conf f32 [P,2] (softmaxed), landms f32 [P,10], priors f32 [P,4] (cx, cy, w, h; prior_box.py:16-33)
 *     -> dets f32 [P,15] = x0, y0, x1, y1, score, 5 x (lx, ly): the row layout the predictor returns, BEFORE its
 *     confidence filter / NMS / top-k (host side, avcer_amd/face_tiles.py, as in the reference).
 *   avcer_crop_tiles   ref: data/get_face_images.py:52-56 (crop fr[y0:y1, x0:x1]) + data/utils.py:34 (PIL NEAREST
 *                            resize to 224x224), without the JPEG file in between
 *     frames u8 [T,H,W,3], rects i32 [n,5] = frame, x0, y0, x1, y1 (end-exclusive, inside the frame),
 *     swap_rb != 0 when the frames are BGR (cv2 order) -> tiles u8 [n,224,224,3] RGB, the input of
 *     avcer_static_forward.  A rect that is empty or leaves the frame yields an all-zero tile. */
int avcer_face_decode(avcer_ctx* ctx, const float* loc, const float* conf, const float* landms, const float* priors,
                      int n_priors, int im_h, int im_w, float var0, float var1, float* dets, avcer_stream_t stream);
/* avcer_face_decode for a batch of frames in one launch: loc [T,P,4], conf [T,P,2], landms [T,P,10] (what avcer_face_forward
 * writes for T frames) -> dets [T,P,15]; the priors [P,4] are shared.  T <= 65535. */
int avcer_face_decode_batch(avcer_ctx* ctx, const float* loc, const float* conf, const float* landms, const float* priors,
                            int n_frames, int n_priors, int im_h, int im_w, float var0, float var1, float* dets,
                            avcer_stream_t stream);
int avcer_crop_tiles(avcer_ctx* ctx, const uint8_t* frames, int n_frames, int h, int w, const int32_t* rects, int n,
                     int swap_rb, uint8_t* tiles, avcer_stream_t stream);

/* Grad-CAM heat maps of the static CNN (get_prob_video.py:101-155 with flag_heatmaps, data/utils.py:92-112,
 * visualization/visualize.py:218-253).
 *   avcer_static_forward_cam: avcer_static_forward (same arguments, same logits / probs / feats bit for bit; probs required,
 *     logits and feats may be NULL) plus cam f32 [n,7,7,7]: for every frame and class k the raw map
 *     cam[f,k,y,x] = mean_c g_k[c] * A[c,y,x] over layer 4's output A, where g_k = d p_k / d A is constant over the 7 x 7
 *     positions (s = p_k (e_k - p), u = 1[h > 0] W2^T s, g_k = W1^T u / 49), before ReLU and normalisation.  f32 arithmetic in
 *     every mode; a frame's map does not depend on the frames around it.
 *   avcer_crop_resize_linear: cv2.resize(frames[f][y0:y1, x0:x1], (out_w, out_h)) with INTER_LINEAR on u8 (11-bit fixed-point
 *     weights); rects i32 [n,5] = frame, x0, y0, x1, y1 as avcer_crop_tiles takes them; swap_rb swaps the first and last channel.
 *     A rect of the output's size is copied.  A rect that is empty or leaves its frame yields zeros.  out u8 [n,out_h,out_w,3].
 *   avcer_cam_render: overlay i of n from cam[rows[i], cls[i]] (rows index the [.,7,7,7] maps and must be in range, cls in
 *     0..6): max(m, 0) / max (NaN -> 0 when nothing is positive), f32 bilinear to 224 x 224, u8 truncation, lut_bgr u8 [256,3],
 *     blend (1 - image_weight) * lut / 255 + image_weight * base_rgb / 255 with base_rgb u8 [n,224,224,3], / max, u8 ->
 *     out_bgr u8 [n,224,224,3].  Every operation rounded once in f32, as the numpy statement computes it. */
int avcer_static_forward_cam(avcer_ctx* ctx, const uint8_t* frames, int n, int in_h, int in_w, int mode, float* logits, float* probs,
                             float* feats, float* cam, avcer_stream_t stream);
int avcer_crop_resize_linear(avcer_ctx* ctx, const uint8_t* frames, int n_frames, int h, int w, const int32_t* rects, int n,
                             int swap_rb, int out_h, int out_w, uint8_t* out, avcer_stream_t stream);
int avcer_cam_render(avcer_ctx* ctx, const float* cam, const int32_t* rows, const int32_t* cls, const uint8_t* base_rgb, int n,
                     const uint8_t* lut_bgr, double image_weight, uint8_t* out_bgr, avcer_stream_t stream);

/* The drawing of the result video (video/functions/get_visualization.py:40-118: face boxes and "<label>: <p>%" lines on every
 * frame), in place in the frame batch on the device.  The claim is identity with PIL's ImageDraw, tolerance zero (avcer_amd/annotate.py
 * draw_numpy is the statement both sides are held to); cv2's anti-aliased lines and Hershey font are NOT reproduced.
 * One record per drawn item, 12 x int32: */
enum { AVCER_DRAW_OUTLINE = 0, AVCER_DRAW_FILL = 1, AVCER_DRAW_MASK = 2 };
typedef struct avcer_draw_item {
    int32_t frame;     /* which frame of the batch, 0 .. n-1 */
    int32_t kind;      /* AVCER_DRAW_* */
    int32_t x0, y0;    /* OUTLINE, FILL: first corner (inclusive); MASK: where the mask's top left pixel goes */
    int32_t x1, y1;    /* OUTLINE, FILL: last corner (inclusive), x1 >= x0 and y1 >= y0; MASK: unused */
    int32_t arg;       /* OUTLINE: border width t >= 1; FILL: coverage 1..255; MASK: integer scale k >= 1 */
    int32_t mask;      /* MASK: index into the mask table; else unused */
    int32_t colour[3]; /* 0..255 each, in the frame's own channel order (the kernel does not know BGR from RGB) */
    int32_t pad;
} avcer_draw_item;
/*   OUTLINE = ImageDraw.rectangle((x0,y0,x1,y1), outline=colour, width=t): rows y0 .. y0+t-1 and y1-t+1 .. y1 over x0 .. x1, and
 *     columns x0 .. x0+t-1 and x1-t+1 .. x1 between them; the border grows inward and the box is solid once 2t reaches a side (PIL
 *     lets the rows run past the box when t exceeds its height, and so does this).
 *   FILL = ImageDraw.bitmap((x0,y0), Image.new("L", (x1-x0+1, y1-y0+1), c), fill=colour): a rectangle of constant coverage.
 *   MASK = ImageDraw.bitmap((x0,y0), mask.resize((k*w, k*h), NEAREST), fill=colour): coverage masks[offset + (dy/k)*w + dx/k] with
 *     (offset, w, h) = table[3*mask ..]; the masks are u8 and lie back to back in `masks` (masks_bytes in all).
 *   Blend, per channel, PIL's BLEND8: t = dst*(255-c) + colour*c + 128, dst = ((t >> 8) + t) >> 8 (the sum rounded once).
 * Everything is clipped to its frame; an item wholly outside draws nothing; nothing outside `frames` u8 [n,h,w,3] is written, and
 * pixels no item covers are neither read nor written.
 * Order: `items` [m] are sorted by frame, and a frame's result is that of drawing its items one after another in list order,
 * whatever their overlap.  One thread owns one pixel and walks the frame's items; the launch is laid out by `work`, int32
 * [n_work, 8] sorted by frame, one row per frame that has items: frame, first item, one past its last item, x and y of the top left
 * pixel of the area its items cover (clipped to the frame), 64-pixel tiles per row of that area, the number of 64 x 4 tiles of all
 * rows before this one, 0.  n_tiles = the tiles of all rows.  avcer_amd/annotate.py work_table builds it.  items, masks, table and
 * work are DEVICE pointers; the caller has checked the items (Engine.annotate raises ValueError naming the item).  A record that
 * is out of range all the same is skipped by the kernel, never followed.  m = 0 or n_tiles = 0: nothing is launched. */
int avcer_annotate_frames(avcer_ctx* ctx, uint8_t* frames, int n, int h, int w, const avcer_draw_item* items, int m, const uint8_t* masks,
                          int64_t masks_bytes, const int32_t* table, int n_masks, const int32_t* work, int n_work, int64_t n_tiles,
                          avcer_stream_t stream);

/* Image.resize of a batch of RGB frames, bit for bit PIL's (Pillow's Resample.c, 8 bits per channel) for its convolution
 * filters BOX, BILINEAR, BICUBIC and LANCZOS with the default `box` and `reducing_gap=None`; HAMMING and NEAREST are not covered.
 *   ref: PIL.Image.resize; this departs from the reference on purpose (data/get_face_images.py:50 feeds the detector whole frames).
 * src u8 [n,h,w,3] -> dst u8 [n,h2,w2,3], both contiguous on the device, dst a buffer of its own.  Two separable passes with a u8
 * value between them, horizontal first; per axis with `in` source and `out` output pixels, for output o and each channel:
 *   value = clip(((1 << 21) + sum_{j < count[o]} source[first[o] + j] * kk[o][j]) >> 22, 0, 255)      (int32, arithmetic shift)
 * The table of an axis is int32 [out * (2 + k)]: first[out], count[out], kk[out][k] back to back, built on the host in double
 * exactly as Resample.c's precompute_coeffs / normalize_coeffs_8bpc build it (avcer_amd/resize.py resize_plan); an axis that
 * keeps its size gets the identity table (first = o, count = 1, kk = 1 << 22), which reproduces PIL skipping that pass.
 * xtab / ytab: the horizontal (in w, out w2, k = xk) and vertical (in h, out h2, k = yk) tables on the DEVICE; xtab_host /
 * ytab_host: the same tables on the HOST, of which first and count are read -- to refuse a table with first < 0, count > k or
 * first + count > in (AVCER_EINVAL), and to pick the form.  The kernels clamp their source index as well, so a device table that
 * differs from the checked one gives wrong numbers, never a read outside the source.
 * form: AVCER_RESIZE_CHOOSE, or one of the two forms by name (for tests; they give the same bits):
 *   AVCER_RESIZE_FUSED     one launch: a block resizes the source rows its tile's vertical taps read horizontally into LDS and runs
 *                          the vertical pass from there; AVCER_EINVAL when a tile's rows do not fit LDS (avcer_resize_form);
 *   AVCER_RESIZE_TWO_PASS  two launches through a u8 intermediate [n,h,w2,3] in the context's workspace; an unchanged axis is skipped.
 * Sides 1 .. AVCER_RESIZE_MAX_SIDE on both ends, up- and downscaling.  n = 0: nothing is launched.  No host synchronisation. */
enum { AVCER_RESIZE_CHOOSE = 0, AVCER_RESIZE_FUSED = 1, AVCER_RESIZE_TWO_PASS = 2 };
#define AVCER_RESIZE_MAX_SIDE 8192
int avcer_resize_frames(avcer_ctx* ctx, const uint8_t* src, int n, int h, int w, uint8_t* dst, int h2, int w2, const int32_t* xtab_host,
                        const int32_t* xtab, int xk, const int32_t* ytab_host, const int32_t* ytab, int yk, int form, avcer_stream_t stream);
/* The form AVCER_RESIZE_CHOOSE takes for a vertical table (HOST pointer, h2 outputs): AVCER_RESIZE_FUSED or AVCER_RESIZE_TWO_PASS;
 * AVCER_EINVAL for a null table or h2 outside 1 .. AVCER_RESIZE_MAX_SIDE.  Host code; nothing is launched. */
int avcer_resize_form(const int32_t* ytab_host, int h2);

/* The traces of the prediction timeline chart, for a batch of charts in one call: per chart the compound class of up to four
 * models against the frame number, as dotted lines in four colours.
 *   ref: run.py:272-296 (flag_save_plot_pred), visualization/visualize.py:175-215 plot_compound_expression_prediction.  matplotlib
 *   is not reproduced: the claim is identity with PIL's ImageDraw.line(width=1), tolerance zero (avcer_amd/chart.py chart_numpy is
 *   the CPU statement; frame, ticks, titles and legend are drawn behind this call by avcer_annotate_frames).
 * table: `series` rows of `stride` classes (0 .. AVCER_CHART_CLASSES - 1), int32 (elem_bytes 4) or int64 (8), on the device; chart v
 * reads the columns offset .. offset + length - 1 of every row.  Per chart a record: the plot rectangle (x0, y0, pw, ph) inside the
 * picture, the row centre yc[c] of every class (inside the rectangle), and its offset and length.  Frame i of a chart of T frames
 * stands in column x0 + ((2i + 1) * pw) / (2T) (64-bit) at row yc[class]; the trace of a series is the union of PIL's lines between
 * consecutive frames (a lone frame: its point), widened by one row up and down, clipped to the rectangle, and thinned: pixel
 * (x, y) of series s is painted iff (x + y) % 4 == s, with colours[3s .. 3s + 2].  No two series contend for a pixel.
 * plans_host / plans: the same n_charts records on the HOST (checked: AVCER_EINVAL for a rectangle that is empty or leaves the
 * picture, a row centre outside it, a length < 1 or columns behind the stride) and on the DEVICE (read by the kernels, which
 * bound every address themselves, so a device copy that differs gives wrong pixels, never an access outside table or out).
 * colours: HOST, 3 * series bytes.  out u8 [n_charts, h, w, 3] on the device, already holding the background; uncovered pixels
 * are neither read nor written.  Sides 1 .. AVCER_CHART_MAX_SIDE.  A class outside the range is clamped: the caller refuses it.
 * Two launches -- an envelope of one row interval per (chart, series, column) in the context's workspace, then the paint -- and
 * none for n_charts = 0.  No host synchronisation. */
#define AVCER_CHART_CLASSES 7
#define AVCER_CHART_MAX_SERIES 4
#define AVCER_CHART_MAX_SIDE 16384
typedef struct avcer_chart_plan {
    int32_t x0, y0, pw, ph;
    int32_t yc[AVCER_CHART_CLASSES];
    int32_t pad;
    int64_t offset, length;
} avcer_chart_plan; /* 64 bytes */
int avcer_chart_series(avcer_ctx* ctx, const void* table, int elem_bytes, int series, int64_t stride, const avcer_chart_plan* plans_host,
                       const avcer_chart_plan* plans, int n_charts, uint8_t* out, int h, int w, const uint8_t* colours,
                       avcer_stream_t stream);
/* How the envelope treats a chart of `frames` frames on a plot `pw` columns wide: AVCER_CHART_REDUCE (frames >= pw: a column holds
 * frames / pw frames or more and reduces them over a wave) or AVCER_CHART_SEGMENT (frames < pw: a column evaluates the one segment
 * that crosses it); AVCER_EINVAL for frames < 1 or pw outside 1 .. AVCER_CHART_MAX_SIDE.  Host code; nothing is launched. */
enum { AVCER_CHART_REDUCE = 1, AVCER_CHART_SEGMENT = 2 };
int avcer_chart_path(int64_t frames, int pw);

/* The face tracker between detector and tiles, for a whole video in ONE call -- HOST code and HOST pointers (the tracker is
 * sequential in time and sees a handful of boxes per frame; the reference runs it on the host too):
 *   ref: data/face_detection/ibug/face_detection/utils/simple_face_tracker.py:10-90 (IoU distance, Hungarian assignment by
 *        scipy.optimize.linear_sum_assignment, tracklets dropped on an empty frame), data/get_face_images.py:38-63
 *        (VideoPredictor.process: tracker per frame, crop rectangle fr[y0:y1, x0:x1] of every detection).
 * dets host f32 [sum(counts), ld] (x0, y0, x1, y1 first; ld >= 4), counts host i32 [n_frames] detections per frame ->
 * records host i64 [sum(counts), 6] = frame, track directory (track id - 1), x0, y0, x1, y1 (the clamped half-open crop) in the
 * reference's write order, *n_records rows.  AVCER_EINVAL where the reference raises: a zero-area detection (no track id) or an
 * empty crop; avcer_last_error names the frame (ctx may be NULL: no device is touched, errors are then the code alone).  avcer_lsap is the assignment step on its own (scipy's algorithm and
 * tie-breaking; cost host f64 [nr, nc] -> min(nr, nc) pairs sorted by row), exported for the host-logic tests. */
int avcer_track_faces(avcer_ctx* ctx, const float* dets_host, int ld, const int32_t* counts_host, int n_frames, int frame_w,
                      int frame_h, double iou_threshold, double minimum_face_size, int64_t* records_host, int64_t* n_records);
int avcer_lsap(int nr, int nc, const double* cost_host, int32_t* rows_host, int32_t* cols_host);

/* The same tracker, resumable: a video pushed in pieces gives the records of the whole.  The handle is HOST state -- the live
 * tracklets (boxes, areas, ids), the tracklet counter, and with them what an empty frame did (it drops every tracklet; the counter
 * runs on) -- carried from one push to the next.  avcer_tracker_push takes the next n_frames frames of the video, the first of
 * which is frame `first_frame` (>= 0) of the whole: arguments as avcer_track_faces, records carry the GLOBAL frame index and
 * errors name it; records_host needs room for this push's sum(counts) rows.  After an error the handle takes no further push
 * (AVCER_EINVAL, the first error's text stands).  avcer_tracker_last_error: the text of the handle's last error ("" when none).
 * avcer_tracker_create returns NULL when host memory is out.  avcer_track_faces is create + one push + destroy. */
typedef struct avcer_tracker avcer_tracker;
avcer_tracker* avcer_tracker_create(double iou_threshold, double minimum_face_size);
int avcer_tracker_push(avcer_tracker* tracker, const float* dets_host, int ld, const int32_t* counts_host, int n_frames,
                       int64_t first_frame, int frame_w, int frame_h, int64_t* records_host, int64_t* n_records);
const char* avcer_tracker_last_error(const avcer_tracker* tracker);
void avcer_tracker_destroy(avcer_tracker* tracker);

/* JPEG face crops, decoding: the files stage 0 writes and stage 1 reads back,
 *   ref: data/get_face_images.py:52-63 (cv2.imwrite of `<faces>/<track>/NNNNNN.jpg`), get_prob_video.py:79-100 (the read loop),
 *        data/utils.py:34 (PIL NEAREST resize to 224 x 224)
 * decoded without a decoder library, split where the work changes kind: marker parsing and Huffman decoding on the HOST
 * (avcer_jpeg_probe, avcer_jpeg_entropy_batch: host code and host pointers, ctx may be NULL, no device is touched), everything
 * behind the coefficients on the DEVICE (avcer_jpeg_tiles, avcer_jpeg_rgb).  The arithmetic is libjpeg's with its defaults --
 * the "islow" integer inverse DCT, fancy chroma upsampling, 16-bit fixed-point YCbCr -> RGB -- and the contract is bit-identity
 * with PIL's decode of the same file (libjpeg-turbo): a tolerance of zero, independent of the arithmetic mode.
 *
 * Handled (status AVCER_JPEG_OK): SOF0 and 8-bit SOF1, Huffman coded, ONE scan of all components; one component (grey) or three
 * read as YCbCr (a JFIF segment; else an Adobe segment with transform 1; else the component ids 1, 2, 3); luma sampling 1x1, 2x1
 * or 2x2 with chroma 1x1; 8-bit quantisation tables; DRI / RSTn, 0xFF00 stuffing, fill bytes; any APPn / COM segments; any
 * Huffman tables.  EVERYTHING else is AVCER_JPEG_NOT_HANDLED and never guessed at: no SOI at offset 0, progressive / arithmetic /
 * lossless / 12-bit files, four components, Adobe transform 0 or 2, other sampling factors, several scans, DNL, 16-bit tables,
 * bytes between segments, a bit stream that ends early, an undefined Huffman code, a coefficient index past 63, a wrong or
 * missing RSTn, a missing EOI, a dequantised coefficient outside int16, and a file whose blocks do not fit the storage given.
 * `reason` says which (csrc/jpeg.h R_*; 12 = no space).  The caller decodes such a file some other way (avcer_amd/jpeg.py: PIL).
 *
 * avcer_jpeg_desc: one file.  bw / bh: blocks per component, padded to whole MCUs (a one-component file: ceil(w / 8), ceil(h /
 * 8)); qt: each component's quantisation table in natural order; hs / vs: the first component's sampling factors as the file
 * states them; coef_block / n_blocks: where the file's coefficient blocks lie in the storage, in blocks of 64 int16 -- component
 * after component, raster order over the padded grid, each block in natural (de-zigzagged) order, not dequantised.
 *
 * avcer_jpeg_probe: the header of one file (up to its scan) -> *info; coef_block 0.
 * avcer_jpeg_entropy_batch: n files (files[i], lens[i]) -> desc[n] and the coefficients of every handled file in coeffs (room
 *   for cap_blocks blocks); files take consecutive blocks in file order, so coef_block ascends; *blocks_needed (may be NULL) =
 *   what all files with a supported header need together.  Files are decoded independently on min(16, threads) host threads,
 *   threads <= 0: 16 -- never the machine's core count; the library reads no environment, avcer_amd/jpeg.py passes
 *   min(16, OMP_NUM_THREADS or 16).  The result does not depend on the thread count.
 * avcer_jpeg_tiles: coeffs (n_blocks blocks) and desc[n] as the call above wrote them, copied to the device (both 16-byte
 *   aligned) -> tiles u8 [n,224,224,3] RGB = Image.open(file).convert("RGB").resize((224, 224), NEAREST), avcer_crop_tiles' rule;
 *   a file that is not AVCER_JPEG_OK yields a zero tile.  Only the source pixels a tile samples are colour-converted.
 * avcer_jpeg_rgb: the same files at full size -> canvas u8 [n,hmax,wmax,3] RGB, image i in the top left corner of slot i, zeros
 *   around it (and everywhere for a file that is not OK): the canvas of avcer_crop_resize_linear with rects (i, 0, 0, w, h).
 * flags i32 [n] (device, written by both calls): 1 where the inverse DCT of file i left the range inside which libjpeg's C and
 *   SIMD code agree (dequantised coefficients and pass-1 results within +-16383, samples within [-512, 511]: a corrupt stream or
 *   table, never a picture an encoder wrote); such a file's output is zero and the caller decodes it some other way, as for a
 *   file that is not OK.  Reading the flags is the caller's only reason to wait for the stream.
 * Both device calls run two kernels on `stream` (dequantisation + inverse DCT into u8 component planes in the context's
 * workspace, 64 bytes per block; then the pixels) and do not synchronise with the host. */
enum { AVCER_JPEG_OK = 0, AVCER_JPEG_NOT_HANDLED = 1 };
typedef struct avcer_jpeg_desc {
    int32_t status, reason;
    int32_t width, height, ncomp;
    int32_t hs, vs;
    int32_t bw[3], bh[3];
    int32_t tq[3];          /* quantisation table id of each component */
    int64_t coef_block, n_blocks;
    uint16_t qt[3][64];
} avcer_jpeg_desc;         /* 464 bytes */
int avcer_jpeg_probe(const uint8_t* bytes_host, size_t len, avcer_jpeg_desc* info_host);
int avcer_jpeg_entropy_batch(avcer_ctx* ctx, const uint8_t* const* files_host, const int64_t* lens_host, int n, int16_t* coeffs_host,
                             int64_t cap_blocks, avcer_jpeg_desc* desc_host, int threads, int64_t* blocks_needed);
int avcer_jpeg_tiles(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n, int32_t* flags,
                     uint8_t* tiles, avcer_stream_t stream);
int avcer_jpeg_rgb(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n, int32_t* flags,
                   uint8_t* canvas, int hmax, int wmax, avcer_stream_t stream);

/* Motion-JPEG frames: the video stream of an AVI file is a list of baseline JPEG files (avcer_amd/avi.py), decoded by the calls
 * above and below into the batch the detector and the crop kernels read,
 *   ref: data/get_face_images.py:19-24, 44-47 (cv2.VideoCapture: the frames of a recording, BGR)
 * with two additions.  The contract stays bit-identity with PIL's decode of each frame (libjpeg-turbo), tolerance zero; what cv2
 * would decode of the same stream (ffmpeg's own MJPEG decoder and colour conversion) is not claimed.
 *
 * AVCER_JPEG_STD_TABLES (a bit of `hflags`): many Motion-JPEG producers omit the DHT segments; a Huffman table 0 or 1 that the scan
 *   references and no DHT segment of the file defined is then the table of that class and id of the standard's annex K (K.3 -
 *   K.6) -- the rule of libjpeg-turbo and of ffmpeg's mjpeg2jpeg filter.  A table the file defines is the file's own; ids 2 and 3
 *   have no standard table and stay reason 8.  csrc/jpeg.h holds ONE statement of the four tables, the writer's.
 * avcer_jpeg_entropy_batch_ex / avcer_jpeg_scan_batch_ex (below, beside avcer_jpeg_scan_batch): avcer_jpeg_entropy_batch /
 *   avcer_jpeg_scan_batch with `hflags` (0 or AVCER_JPEG_STD_TABLES; any other bit: AVCER_EINVAL); with hflags 0 they ARE those
 *   calls.  Host code and host pointers, ctx may be NULL.  The calls without the argument do not change: a file without DHT stays
 *   AVCER_JPEG_NOT_HANDLED, reason 8, through them.  An assumed table reaches avcer_jpeg_unpack as any other: it is in tabs[].
 * avcer_jpeg_frames: coeffs, n_blocks, desc[n], flags as avcer_jpeg_rgb takes them -> frames u8 [n,H,W,3], frame i = file i, in
 *   RGB order or, with bgr != 0, in BGR order (what cv2 hands the reference).  EVERY file must be exactly W x H: a file that is
 *   AVCER_JPEG_OK and of another size gets flags[i] = 2 and a zero frame (flag 2 wins over flag 1); a file that is not OK or
 *   whose flag is 1 yields a zero frame as in avcer_jpeg_rgb.  Every byte of `frames` is written, none outside; `frames` needs no
 *   alignment (aligned 16-byte stores along each row, byte stores at a row's two ends).  H, W in 1..65535, n H W < 2^36.
 *   Three kernels on `stream` -- avcer_jpeg_rgb's first (dequantisation + inverse DCT into the u8 component planes of the context's
 *   JPEG workspace, 64 bytes per block), the size check, the pixels -- and no synchronisation with the host. */
#define AVCER_JPEG_STD_TABLES 1
int avcer_jpeg_entropy_batch_ex(avcer_ctx* ctx, const uint8_t* const* files_host, const int64_t* lens_host, int n, int16_t* coeffs_host,
                                int64_t cap_blocks, avcer_jpeg_desc* desc_host, int threads, int hflags, int64_t* blocks_needed);
int avcer_jpeg_frames(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n, int32_t* flags,
                      uint8_t* frames, int H, int W, int bgr, avcer_stream_t stream);

/* Uncompressed video: the frames of an AVI file whose video stream is BI_RGB device-independent bitmaps of 24 or 32 bits a pixel
 * (`ffmpeg -c:v rawvideo -pix_fmt bgr24`; avcer_amd/avi.py, avcer_amd/dib.py) unpacked into the same batch,
 *   ref: data/get_face_images.py:19-24, 44-47 (cv2.VideoCapture: the frames of a recording, BGR)
 * without a lossy transcode between the decoder's BGR frames and the detector.  There is no arithmetic; the contract is identity
 * with PIL's BMP reader on the same bytes, tolerance zero.
 * avcer_dib_frames: `span` = span_bytes file bytes on the device (any alignment), offsets i64 [n] on the device: the first byte of
 *   frame i's chunk data from `span` (any alignment; two frames may share one: a repeated frame) -> frames u8 [n,H,W,3].  A source
 *   frame is H rows of stride = (W * bits / 8 + 3) & ~3 bytes, B G R (X) per pixel, bits 24 or 32, the picture's LAST row first
 *   with bottom_up != 0.  The output rows are top-down, without the padding and the fourth byte, in BGR order with bgr != 0 and in
 *   RGB order otherwise.  Every byte of `frames` is written, none outside; `frames` needs no alignment (aligned 16-byte stores
 *   along each row, byte stores at a row's two ends).  No byte outside [span, span + span_bytes) is read (aligned 16-byte loads
 *   where they lie inside, byte loads at the span's two ends); a frame whose offset is negative or leaves fewer than stride * H
 *   bytes is written as zeros.  H, W in 1..65535, n H W < 2^36.  One kernel on `stream`, no synchronisation with the host. */
int avcer_dib_frames(avcer_ctx* ctx, const uint8_t* span, int64_t span_bytes, const int64_t* offsets, int n, uint8_t* frames, int H,
                     int W, int bits, int bottom_up, int bgr, avcer_stream_t stream);

/* The other direction: the JPEG wire format between stages 0 and 1 is written by this library as well as read.  The face folders
 * of stage 0 and the heat maps,
 *   ref: data/get_face_images.py:52-63 (cv2.imwrite of every detection's crop), get_prob_video.py:154 (cv2.imwrite of an overlay)
 * encoded without an encoder library, split at the same place: colour conversion, chroma downsampling, the forward DCT and the
 * quantisation on the DEVICE (avcer_jpeg_forward, one launch per batch, images cut straight out of the decoded frames), headers
 * and Huffman coding on the HOST (avcer_jpeg_quant_tables, avcer_jpeg_plan, avcer_jpeg_write_batch: host code and host pointers,
 * ctx may be NULL, no device is touched).  avcer_jpeg_pack, below them, is the same writer on the device.  The arithmetic is libjpeg's -- 16-bit fixed-point RGB -> YCbCr, the box filter with
 * its alternating bias, the "islow" forward DCT, division by 8 q with halves away from zero -- and the contract is BYTE-identity
 * with PIL.Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=subsampling) (libjpeg-turbo): a tolerance of zero,
 * independent of the arithmetic mode.
 *
 * Written: baseline, three components YCbCr, luma sampling 1x1 / 2x1 / 2x2 (`subsampling` 0 / 1 / 2, PIL's numbering), quality
 * 1..100, the standard Huffman tables, one scan, a JFIF 1.01 header.  Not written: grey, optimised tables, restart markers,
 * progressive files, EXIF and comments.
 *
 * Both directions share avcer_jpeg_desc and the coefficient layout.  Edges follow jcprepct.c: columns repeat the last pixel,
 * luma rows the last row; chroma rows under 2x2 repeat the last input row only to make the height even and the last DOWNSAMPLED
 * row from there down.  Dummy blocks (those that only pad luma to whole MCUs) are final when avcer_jpeg_forward returns: zero AC
 * and the DC of the block libjpeg codes before them in the MCU (jccoefct.c); avcer_jpeg_write_batch codes what it is given.
 *
 * avcer_jpeg_quant_tables: jpeg_set_quality(quality, force_baseline) -> qt[0] luma, qt[1] chroma, natural order.
 * avcer_jpeg_plan: n image sizes (sizes[2 i] = width, sizes[2 i + 1] = height) -> desc[n] as the decoder's entropy pass would
 *   fill them for the files to be written (ncomp 3, hs / vs, MCU-padded bw / bh, tq 0 1 1, qt); images take consecutive blocks in
 *   image order, so coef_block ascends; *blocks_needed (may be NULL) = their sum.  A width or height of zero or above 65535:
 *   AVCER_JPEG_NOT_HANDLED, reason 18, no blocks.
 * avcer_jpeg_forward: image i is the half-open rectangle rects[i] = (slot, x0, y0, x1, y1) (device i32 [n,5]; x1 - x0 and y1 - y0
 *   are desc[i].width and .height) of src u8 [N,H,W,3] (RGB, or BGR with bgr != 0); desc[n] as avcer_jpeg_plan wrote them, copied
 *   to the device (16-byte aligned, as coeffs) -> coeffs int16 [n_blocks, 64].  One kernel on `stream`, no synchronisation with
 *   the host.  Coordinates are clamped to the tensor: a wrong rectangle yields wrong pixels, never a read outside src.
 * avcer_jpeg_write_batch: coeffs and desc[n] on the HOST -> the files, back to back in out (room for cap_bytes); file i is
 *   out[offsets[i] .. offsets[i + 1]) (offsets host i64 [n + 1]).  Files are written independently on min(16, threads) host
 *   threads, threads <= 0: 16 -- never the machine's core count; the result does not depend on the thread count.  A file that
 *   is not written has no bytes and its desc[i] turns AVCER_JPEG_NOT_HANDLED with the reason: 12 = it does not fit cap_bytes
 *   (*bytes_needed, may be NULL, = what all files need together; nothing is written past cap_bytes), 16 = a coefficient the
 *   standard tables cannot code, 19 = a descriptor avcer_jpeg_plan did not write.  desc[i] already NOT_HANDLED is skipped. */
int avcer_jpeg_quant_tables(int quality, uint16_t qt[2][64]);
int avcer_jpeg_plan(const int32_t* sizes_host, int n, int subsampling, int quality, avcer_jpeg_desc* desc_host, int64_t* blocks_needed);
int avcer_jpeg_forward(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects, const avcer_jpeg_desc* desc, int n,
                       int bgr, int16_t* coeffs, int64_t n_blocks, avcer_stream_t stream);
int avcer_jpeg_write_batch(avcer_ctx* ctx, const int16_t* coeffs_host, avcer_jpeg_desc* desc_host, int n, uint8_t* out_host,
                           int64_t cap_bytes, int64_t* offsets_host, int threads, int64_t* bytes_needed);

/* avcer_jpeg_pack: avcer_jpeg_write_batch on the DEVICE -- headers, Huffman coding with the standard tables, byte stuffing, EOI --
 * so that the files, and not 128 bytes of coefficients per block, cross to the host.  Same contract, same bytes: file i is
 * byte-identical to what avcer_jpeg_write_batch writes from the same coefficients and descriptor (and so to PIL's file), whatever
 * n is and whichever other files share the call.
 *   coeffs int16 [n_blocks, 64] as avcer_jpeg_forward leaves them and desc[n] as avcer_jpeg_plan wrote them, both on the device
 *   (desc 16-byte aligned, not modified).  The files' block ranges may come in any order but lie inside the n_blocks blocks and
 *   share none: the n_blocks of the files of one call add up to at most n_blocks (a file past that sum is status 19).
 *   out u8 [cap_bytes], offsets i64 [n + 1], status i32 [n], bytes_needed i64 [1]: on the device.  File i is
 *   out[offsets[i] .. offsets[i + 1]); status[i] is 0 for a file that was written, else the reason, and such a file has no bytes
 *   and disturbs no other: 12 = it does not fit cap_bytes (files take the next free bytes in file order, as in
 *   avcer_jpeg_write_batch; nothing is written past cap_bytes), 16 = a coefficient the standard tables cannot code (more than 11
 *   bits of DC difference, 10 of AC), 17 = a scan of more than 2^32 - 64 bits (512 MiB: bit offsets inside a file are 32 bits
 *   wide; such a file is reported, never wrapped; byte offsets are 64 bits wide), 19 = a descriptor avcer_jpeg_plan did not write
 *   or blocks outside the storage; a desc[i] that is already NOT_HANDLED is skipped and reports its own reason.  *bytes_needed =
 *   what all codable files need together (those of status 0 or 12).
 *   Seven kernels on `stream`, no synchronisation with the host; scratch (212 bytes per block: an unstuffed block is at most
 *   ceil((20 + 63 * 26) / 8) = 208) comes from the context's JPEG workspace.  n_blocks < 2^31. */
int avcer_jpeg_pack(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n, uint8_t* out,
                    int64_t cap_bytes, int64_t* offsets, int32_t* status, int64_t* bytes_needed, avcer_stream_t stream);

/* The round trip without the file: what stage 1 of the reference sees of a crop is not the crop but the JPEG file stage 0 wrote
 * of it, read back,
 *   ref: data/get_face_images.py:52-63 (cv2.imwrite, quality 95, 4:2:0), get_prob_video.py:93-109 and data/utils.py:19-39 (read
 *        back, NEAREST to 224 x 224), data/utils.py:105 (the heat-map base image: cv2.resize of the read-back crop)
 * and Huffman coding is lossless, so that picture is quantise -> dequantise with libjpeg's arithmetic on both sides: no file and
 * no entropy pass is needed to compute it.  The contract is bit-identity with Image.open(file).convert("RGB") of the file
 * jpeg.encode_images (avcer_jpeg_forward + avcer_jpeg_write_batch, so PIL's Image.save) would write of the same rectangle: a
 * tolerance of zero, independent of the arithmetic mode.
 *
 * avcer_jpeg_roundtrip_tiles: src, N, H, W, rects, desc, n, bgr as avcer_jpeg_forward takes them (desc as avcer_jpeg_plan wrote
 *   them, 16-byte aligned on the device) -> tiles u8 [n,224,224,3] RGB as avcer_jpeg_tiles would give them for those files.
 * avcer_jpeg_roundtrip_rgb: the same images at full size -> canvas u8 [n,hmax,wmax,3] as avcer_jpeg_rgb would give it.
 * coeffs: NULL, or int16 [n_blocks, 64] (16-byte aligned) that receives exactly what avcer_jpeg_forward stores for the same call,
 *   dummy blocks included: one pass then serves the tiles and avcer_jpeg_pack / avcer_jpeg_write_batch.
 * flags i32 [n] (device, written by both calls): as avcer_jpeg_tiles writes them -- an encoder's own coefficients cannot leave the
 *   range, so a 1 there would be a finding about the kernel -- and 1 as well for a descriptor avcer_jpeg_plan did not write or
 *   whose blocks lie outside the n_blocks blocks: such an image's tile / canvas slot is zero and no pixel is stored or read
 *   through its geometry.  `coeffs` is not part of that: it receives what avcer_jpeg_forward stores, and avcer_jpeg_forward does
 *   not judge a descriptor -- the blocks [coef_block, coef_block + n_blocks) of a flagged image that lie inside the n_blocks
 *   blocks are written as it writes them.  A desc[i] that is NOT_HANDLED yields zeros and flag 0, as in avcer_jpeg_tiles, and
 *   none of its blocks is written.
 * Both calls run three kernels on `stream` -- the flags; the forward path of avcer_jpeg_forward per 8 x 8 block, unchanged, with the
 * dequantisation and the inverse DCT of avcer_jpeg_tiles' first kernel behind it in the same lanes, storing u8 component planes
 * into the context's JPEG workspace (64 bytes per block; the coefficients do not leave the chip unless `coeffs` asks for them);
 * then avcer_jpeg_tiles' / avcer_jpeg_rgb's second kernel, unchanged -- and do not synchronise with the host.  Errors: AVCER_EINVAL
 * for a NULL or misaligned pointer or a size out of range (avcer_last_error names the call), as the neighbouring calls. */
int avcer_jpeg_roundtrip_tiles(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects, const avcer_jpeg_desc* desc,
                               int n, int bgr, int16_t* coeffs_or_null, int64_t n_blocks, int32_t* flags, uint8_t* tiles,
                               avcer_stream_t stream);
int avcer_jpeg_roundtrip_rgb(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects, const avcer_jpeg_desc* desc,
                             int n, int bgr, int16_t* coeffs_or_null, int64_t n_blocks, int32_t* flags, uint8_t* canvas, int hmax,
                             int wmax, avcer_stream_t stream);

/* Huffman DECODING on the device: avcer_jpeg_entropy_batch's scan walk as self-synchronising subsequence decoding (Klein & Wiseman;
 * Weissenberger & Schmidt), so that the files' bytes, and not 128 bytes of coefficients per block, cross to the device, and no
 * host thread walks a bit stream.  Same contract as avcer_jpeg_entropy_batch, tolerance zero: the same status and reason for every
 * file, the same coefficients for every file that is OK.  avcer_jpeg_tiles and avcer_jpeg_rgb run behind it unchanged.
 *
 * avcer_jpeg_tab: one Huffman table as its DHT segment states it (bits[l] = codes of length l, bits[0] unused; the symbols).
 * avcer_jpeg_scan: one file's entropy-coded bytes -- bytes[offset .. offset + nbytes), offset a multiple of 16 -- its restart
 *   interval (0: none) and, per component, the index of its DC and AC table in the call's table list.
 *
 * avcer_jpeg_scan_batch (HOST code and host pointers, ctx may be NULL, no device is touched): the headers of n files -> desc[n]
 *   exactly as avcer_jpeg_entropy_batch leaves them before its scan walk (the same reasons, the same refusal of a header that
 *   claims more blocks than its bytes can hold, coef_block in file order), scan[n], the tables of the batch de-duplicated by
 *   content in tabs (a folder one encoder wrote carries four), and a copy of every handled file's bytes from its first
 *   entropy-coded byte to its end in bytes_host, back to back, each start 16-byte aligned.  The entropy-coded bytes are NOT walked:
 *   markers are found on the device.  A file whose bytes do not fit cap_bytes, or whose tables do not fit cap_tabs, is reason 12 and
 *   takes nothing; *bytes_needed, *n_tabs (it may exceed cap_tabs; that many are never written) and *blocks_needed say what all
 *   files with a supported header need together.  threads: as in avcer_jpeg_entropy_batch (<= 0 or > 16: 16).
 *
 * avcer_jpeg_unpack: bytes u8 [n_bytes] (16-byte aligned), scan[n], tabs[n_tabs] and desc[n] as the call above wrote them, copied
 *   to the DEVICE -> coeffs int16 [n_blocks, 64] (16-byte aligned; every OK file's blocks are written, zeros included), status i32
 *   [n] = the file's status; desc[i].status and .reason are updated in place.  A desc[i] that is already NOT_HANDLED is skipped.
 *   sub_bits: bits per subsequence, 0 = the default (512), else a multiple of 32 in [128, 2^20].  The result does not depend on it.
 *   A workgroup takes a file: marker pass (0xFF00 unstuffed, the marker sequence kept), then units of up to 256 consecutive
 *   subsequences, one thread each, decoded in rounds until no exit state changes -- at most 258 rounds, a counted loop --, a write
 *   pass, and a segmented prefix sum that turns DC differences into DC values.  No workgroup waits for another, the host reads
 *   nothing in between.  Two kernels on `stream`; scratch (n_bytes + 12 n_blocks + a few KB) comes from the context's JPEG
 *   workspace.  n_blocks < 2^31, a file's entropy-coded bytes at most 2^27 (else reason 17).  A scan record or descriptor the call
 *   above cannot have written is reason 9 and nothing is read through it.
 *
 * avcer_jpeg_unpack_host: the same phases as plain loops over the "threads" of a workgroup, on HOST pointers, no stream, ctx may be
 *   NULL.  NOT a product path: it exists so that the algorithm can be tested and run under a sanitiser on a machine without a GPU. */
typedef struct avcer_jpeg_tab {
    uint8_t bits[17];
    uint8_t vals[256];
    uint8_t pad[15];
} avcer_jpeg_tab;          /* 288 bytes */
typedef struct avcer_jpeg_scan {
    int64_t offset, nbytes;
    int32_t restart;
    int32_t dc[3], ac[3];
    int32_t pad;
} avcer_jpeg_scan;         /* 48 bytes */
int avcer_jpeg_scan_batch(avcer_ctx* ctx, const uint8_t* const* files_host, const int64_t* lens_host, int n, uint8_t* bytes_host,
                          int64_t cap_bytes, avcer_jpeg_desc* desc_host, avcer_jpeg_scan* scan_host, avcer_jpeg_tab* tabs_host, int cap_tabs,
                          int threads, int32_t* n_tabs, int64_t* bytes_needed, int64_t* blocks_needed);
/* with hflags (AVCER_JPEG_STD_TABLES, "Motion-JPEG frames" above); a video whose encoder optimised its tables per frame carries up
 * to 4 n distinct tables: size cap_tabs from *n_tabs by the two-call pattern */
int avcer_jpeg_scan_batch_ex(avcer_ctx* ctx, const uint8_t* const* files_host, const int64_t* lens_host, int n, uint8_t* bytes_host,
                             int64_t cap_bytes, avcer_jpeg_desc* desc_host, avcer_jpeg_scan* scan_host, avcer_jpeg_tab* tabs_host,
                             int cap_tabs, int threads, int hflags, int32_t* n_tabs, int64_t* bytes_needed, int64_t* blocks_needed);
int avcer_jpeg_unpack(avcer_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const avcer_jpeg_scan* scan, const avcer_jpeg_tab* tabs,
                      int n_tabs, avcer_jpeg_desc* desc, int n, int16_t* coeffs, int64_t n_blocks, int32_t* status, int sub_bits,
                      avcer_stream_t stream);
int avcer_jpeg_unpack_host(avcer_ctx* ctx, const uint8_t* bytes_host, int64_t n_bytes, const avcer_jpeg_scan* scan_host,
                           const avcer_jpeg_tab* tabs_host, int n_tabs, avcer_jpeg_desc* desc_host, int n, int16_t* coeffs_host,
                           int64_t n_blocks, int32_t* status_host, int sub_bits);

/* Probability fusion and compound-expression rule.
 *   ref: run.py:25-165 (get_c_expr_db_pred), data/utils.py:125-127 (softmax), :222-241 (get_compound_expression)
 * stat f32 [n,7] softmaxed static probs and dyn_logits f32 [n,7], both in VIDEO column order;
 * aud_mean f32 [n_aud, c>=7] per-frame mean audio logits in audio order, rows >= n_aud repeat row n_aud-1 (run.py:99-103);
 * w1 host f64 [3,7] or NULL (plain mean, run.py:113-114), w2 host f64 [3];
 * comp_prob f64 [4,n,7] and comp_argmax i32 [4,n] in the order AV, VS, VD, A. */
int avcer_fuse(avcer_ctx* ctx, const float* stat, const float* dyn_logits, const float* aud_mean, int n, int n_aud,
               int aud_c, const double* w1_host, const double* w2_host, int ce_weights_type, int ce_mask,
               double* comp_prob, int32_t* comp_argmax, avcer_stream_t stream);

/* avcer_audio_frame_mean + avcer_fuse for a CONCATENATION of videos in one launch: each frame is fused with the mean of the
 * windows of ITS OWN video that cover it, so a set of recordings of unequal length is fused at the cost of one launch and
 * without one video's windows reaching into the next (a window's frame_hi may exceed its video's frame count).
 *   ref: run.py:85-165 (get_c_expr_db_pred: group mean, tail padding with the last audio row, fusion, compound rule),
 *        get_prob_audio_8_cl.py:94-101 (a window's logits replicated for the frames [lo, hi) of its video)
 * stat, dyn_logits f32 [n_frames,7]: all videos' frames one behind the other, VIDEO column order; win_logits f32 [n_windows,c]:
 * all videos' audio windows one behind the other; frame_lo / frame_hi i32 [n_windows]: each window's span in the numbering of
 * its own video, neither decreasing within a video (what chunk_spans yields; the kernel bounds its walk with it);
 * frame_off, win_off i32 [n_videos+1]: prefix offsets of each video's frames / windows (frame_off[n_videos] = n_frames,
 * win_off[n_videos] = n_windows); n_aud i32 [n_videos]: the leading frames of video v that some window covers, >= 1 -- frames
 * behind them use the row of frame n_aud[v]-1 (run.py:99-103).  All index arrays are DEVICE pointers; n_frames and n_windows
 * are passed by value because the launch is sized from them without reading device memory: there is no host synchronisation.
 * w1_host / w2_host / ce_weights_type / ce_mask as avcer_fuse takes them.
 * comp_prob f64 [4,n_frames,7], comp_argmax i32 [4,n_frames] (AV, VS, VD, A): for the frames of video v, bit for bit what
 * avcer_audio_frame_mean + avcer_fuse give for that video alone (windows visited in index order, f64 sum, one rounding).
 * aud_mean f32 [n_frames,c] and count i32 [n_frames], each optional (NULL): what avcer_audio_frame_mean writes for that video's
 * frames (no covering window: zeros and 0).
 * AVCER_EINVAL outside n_videos >= 1, 7 <= c <= 8, 1 <= n_frames, n_windows <= 2^31-1. */
int avcer_fuse_videos(avcer_ctx* ctx, const float* stat, const float* dyn_logits, const float* win_logits,
                      const int32_t* frame_lo, const int32_t* frame_hi, const int32_t* frame_off, const int32_t* win_off,
                      const int32_t* n_aud, int n_videos, int64_t n_frames, int64_t n_windows, int c, const double* w1_host,
                      const double* w2_host, int ce_weights_type, int ce_mask, float* aud_mean, int32_t* count,
                      double* comp_prob, int32_t* comp_argmax, avcer_stream_t stream);

/* Dataset evaluation, part 1: the per-video loops of get_abaw_pred / get_afew_pred for ONE model's tables of a whole file list.
 *   ref: get_pred_av.py:77-195, get_pred_video.py (its twins), get_pred_audio.py:64-141, data/utils.py:125-127 (softmax)
 * rows f64 [n_rows, c], 7 <= c <= 8: the raw rows of all videos one behind the other; only the first 7 columns are used.
 * keys i32 [n_rows] or NULL: the audio CSV's `frames` number of each row (one row per (window, frame) pair, in no order).
 * row_off i32 [n_videos+1]: prefix offsets of the videos' rows.  key_lo i32 [n_videos], key_off i32 [n_videos+1] (keys only):
 * video v's keys lie in [key_lo[v], key_lo[v] + key_off[v+1] - key_off[v]); a row whose key lies outside belongs to no group.
 * need i32 [n_need], need_off i32 [n_videos+1]: per video the ascending kept positions (`need_index`), need_off[n_videos] = n_need.
 * out_off i32 [n_videos+1]: prefix offsets of the videos' output rows (their target lengths).  All of these are DEVICE pointers;
 * n_rows, n_slots = key_off[n_videos], n_need and n_out = out_off[n_videos] are passed by value, because launches and the workspace are
 * sized from them without reading device memory.  Per video, what the reference's loop does:
 *   1. with keys: the mean of the rows of each distinct key, the groups numbered 0, 1, .. in ascending key order
 *      (`groupby("frames").mean().reset_index()`: a kept position indexes this GROUP NUMBER, not the frame value).  A NaN is
 *      left out of its column's mean as pandas leaves it out (skipna); a column of a group with nothing else is NaN.  The sum is
 *      exact: every term is rounded once to a fixed-point grid 2^-60 of the column's largest magnitude in the group and added as
 *      an integer, so it does not depend on the order of the rows (pandas' compensated sum differs from it by < 1 ulp of the
 *      largest term).  Without keys every row is its own group.
 *   2. softmax != 0: exp(x - max) / sum over the 7 columns in index order (data/utils.py:125-127); 0: the row as it is.
 *   3. video_level == 0: output row j of the video is the group need[min(j, k - 1)], where k is the number of kept positions
 *      below the video's group count: selection, then the last surviving row repeated up to the target length
 *      (get_pred_av.py:121-129; the caller states the target, and with it that the reference extends the static table by the
 *      DYNAMIC table's deficit, :124-125).  k == 0 with a target > 0 is where the reference raises IndexError: NaN rows here.
 *      video_level != 0: ONE output row per video (out_off[v] = v, `need` unused), the mean of step 2 over all its groups
 *      (np.mean(axis=0)): a fixed tree over 256 partial sums, within n * 2^-53 of numpy's sequential sum; NaN without a group.
 * out f64 [n_out, 7].  ws: avcer_eval_tables_workspace(n_slots) bytes of device memory (0 without keys; NULL then).
 * Limits (AVCER_EINVAL beyond them): 1 <= n_videos <= AVCER_EVAL_MAX_VIDEOS, 7 <= c <= 8, 0 <= n_rows, n_slots, n_need, n_out <=
 * AVCER_EVAL_MAX_ROWS, video_level -> n_out == n_videos, keys -> key_lo, key_off and ws.  No host synchronisation. */
#define AVCER_EVAL_MAX_VIDEOS 16777216
#define AVCER_EVAL_MAX_ROWS 268435456LL
int64_t avcer_eval_tables_workspace(int64_t n_slots);
int avcer_eval_tables(avcer_ctx* ctx, const double* rows, const int32_t* keys, int64_t n_rows, int c, const int32_t* row_off,
                      const int32_t* key_lo, const int32_t* key_off, int64_t n_slots, const int32_t* need, int64_t n_need,
                      const int32_t* need_off, const int32_t* out_off, int n_videos, int64_t n_out, int softmax, int video_level, double* out, void* ws,
                      int64_t ws_bytes, avcer_stream_t stream);

/* Dataset evaluation, part 2: the prediction of a model or of a fusion and its confusion matrix (get_metrics).
 *   ref: get_pred_av.py:35-45 and its twin in get_pred_video.py, get_pred_audio.py:30-34; get_compound_expression
 *        (data/utils.py:222-241) for the audio-only submission file (get_pred_audio.py:202-228)
 * tables f64 [m][n][7] and labels i32 [n] (or NULL) on the device; w1_host f64 [m][7] and w2_host f64 [m] on the HOST, each
 * optional (NULL = ones: a product with 1.0 is the value itself).  Per row i, every product and sum rounded on its own:
 *   f = (tables[0][i] * w1[0]) * w2[0];   f = f + (tables[q][i] * w1[q]) * w2[q]  for q = 1 .. m-1
 *   compound & AVCER_EVAL_COMPOUND: f is replaced by the 7 compound-expression values of the audio order,
 *     g[j] = f[p1[j]] * u1[j] + f[p2[j]] * u2[j], u = 1 or, with AVCER_EVAL_CE_WEIGHTS, the pair's class weights over their sum;
 *     with AVCER_EVAL_CE_MASK values of f not above 1/7 count as 0 first;
 *   a = the first index of the maximum, a NaN counting as the maximum (np.argmax).
 * pred i32 [n] (optional) receives a; cm i64 [7][7] (optional, needs labels) receives the counts of (labels[i], a), zeroed by the
 * call in stream order; a label outside 0..6 is counted nowhere (confusion_matrix(labels=range(7))).  Blocks count in LDS and
 * add each non-zero cell once, with integer atomics: the result does not depend on their order.
 * Limits (AVCER_EINVAL beyond them): 1 <= m <= AVCER_EVAL_MAX_MODELS, 1 <= n <= AVCER_EVAL_MAX_ROWS, cm needs labels, one of
 * pred and cm is given.  No host synchronisation. */
#define AVCER_EVAL_MAX_MODELS 4
#define AVCER_EVAL_COMPOUND 1
#define AVCER_EVAL_CE_WEIGHTS 2
#define AVCER_EVAL_CE_MASK 4
int avcer_eval_confusion(avcer_ctx* ctx, const double* tables, const int32_t* labels, int64_t n, int m, const double* w1_host,
                         const double* w2_host, int compound, int32_t* pred, int64_t* cm, avcer_stream_t stream);

/* The audio model over a labelled corpus, the reduction behind it: window-wise majority voting grouped by file.
 *   ref: src/audio/utils/common_utils.py:74-108 (majority_voting) behind the softmax of src/audio/test_c_audio.py:48
 * logits f32 [n, c] (2 <= c <= AVCER_VOTES_MAX_CLASSES): the windows of all files one behind the other; targets i32 [n]; file_off
 * i32 [n_files + 1]: prefix offsets of the files' windows, file_off[0] = 0, ascending, file_off[n_files] = n.  All DEVICE pointers.
 * Per window i, in float32, every operation rounded on its own:
 *   a = the first index of the maximum of logits[i], a NaN counting as the maximum (np.argmax); m = that maximum;
 *   e[k] = expf(logits[i][k] - m);  s = ((e[0] + e[1]) + ..) + e[c-1];  probs[i][k] = e[k] / s;  pred[i] = a.
 *   The argmax is taken on the logits: the softmax is monotone, so it is the argmax of the probabilities wherever those differ.
 * Per file f, over its windows [file_off[f], file_off[f+1]): the counts of pred and of targets; file_pred[f] / file_target[f] =
 * the most frequent value, the SMALLEST of several equally frequent ones (pd.Series.mode(x)[0]); file_onehot[f][k] = (k ==
 * file_pred[f]).  Targets are counted in AVCER_VOTES_TARGET_MIN <= t < c (-2: a corpus without labels, -1: an unlabelled frame
 * run); one outside that range is counted nowhere.  A file without windows (or without a counted target) gets -1, and a zero row.
 * Outputs: probs f32 [n, c], pred i32 [n], file_pred i32 [n_files], file_target i32 [n_files], file_onehot i32 [n_files, c].
 * One launch; one wave per file, a lane per window and 64 windows per step, the counts in registers and a shuffle tree behind
 * them; plain vector stores, no atomics.  Offsets are clamped to [0, n] before they address anything; a window no file covers is
 * not written.  Limits (AVCER_EINVAL beyond them): 1 <= n_files <= AVCER_VOTES_MAX_FILES, 0 <= n <= AVCER_VOTES_MAX_WINDOWS,
 * 2 <= c <= AVCER_VOTES_MAX_CLASSES.  No host synchronisation. */
#define AVCER_VOTES_MAX_CLASSES 8
#define AVCER_VOTES_TARGET_MIN (-2)
#define AVCER_VOTES_MAX_FILES 16777216
#define AVCER_VOTES_MAX_WINDOWS 268435455LL
int avcer_window_votes(avcer_ctx* ctx, const float* logits, const int32_t* targets, const int32_t* file_off, int64_t n, int c,
                       int n_files, float* probs, int32_t* pred, int32_t* file_pred, int32_t* file_target, int32_t* file_onehot,
                       avcer_stream_t stream);

/* Validation of an audio checkpoint: the losses of the window logits of a corpus, batched as the DataLoader batches them.
 *   ref: src/audio/net_trainer/net_trainer.py:391-465 (iterate_model's loss bookkeeping), torch.nn.CrossEntropyLoss(weight,
 *        label_smoothing) and SoftFocalLoss behind SoftFocalLossWrapper (src/audio/loss/loss.py:125-137, 165-166)
 * logits f32 [n, c] (2 <= c <= AVCER_LOSS_MAX_CLASSES), targets i32 [n] in [0, c), weights f32 [c] or NULL (ones): DEVICE pointers.
 * Batch b owns the rows [b * batch_size, min(n, (b + 1) * batch_size)): n_batches = ceil(n / batch_size), the last may be short.
 * Per row i, in float64, every operation rounded on its own (y = targets[i], x = logits[i] widened):
 *   m = max_k x[k];  d[k] = x[k] - m;  e[k] = exp(d[k]);  s = ((e[0] + e[1]) + ..) + e[c-1]
 *   AVCER_LOSS_CE:          l = log(s);  q[k] = -(d[k] - l)  (the negative log-softmax);  a = w[y] * q[y];
 *                           g = ((w[0] * q[0] + w[1] * q[1]) + ..) + w[c-1] * q[c-1];  u = w[y]
 *                           row_loss[i] = (1 - eps) * a + (eps / c) * g          (reduction="none")
 *   AVCER_LOSS_SOFT_FOCAL:  p = min(max(e[y] / s, 1e-7), 1 - 1e-7);  f = 1 (gamma == 0), (1 - p) * (1 - p) (gamma == 2), else
 *                           pow(1 - p, gamma);  a = (w[y] * f) * (-log(p));  row_loss[i] = a          (the other classes add +-0)
 * Per batch, with A, G, U the sums of a, g, u over its n_b rows in the FIXED order below:
 *   CE: batch_loss[b] = (1 - eps) * (A / U) + (eps / c) * (G / U)  (reduction="mean" with weights);  SOFT_FOCAL: A / n_b.
 * epoch[0] = sum_b(batch_loss[b] * batch_size) / n_batches -- net_trainer.py:441,460: the short last batch counts with the full
 * batch size --; epoch[1] = sum_b(batch_loss[b] * n_b) / n, the row-weighted mean.
 * Order of every sum over rows (and, for epoch, over batches): thread t of 256 adds its items t, t + 256, .. one after the other
 * from 0.0; the 256 partial sums then fold in halves (s[t] += s[t + 128], then 64, .., 1).  There are no floating-point atomics:
 * the outputs are a pure function of the inputs.  One launch, one block per batch; the block that finishes last (an integer
 * ticket in `ticket`, i32 [1] on the device, zeroed by the call in stream order) reduces the batch losses to epoch[0..1].
 * A target outside [0, c) makes its row, its batch and the epoch NaN; nothing is indexed with it.
 * Outputs (device): row_loss f64 [n], batch_loss f64 [n_batches], epoch f64 [2].
 * Limits (AVCER_EINVAL beyond them): 1 <= n <= AVCER_VOTES_MAX_WINDOWS, 2 <= c <= AVCER_LOSS_MAX_CLASSES, batch_size >= 1,
 * kind one of the two, label_smoothing in [0, 1], gamma >= 0, both finite.  No host synchronisation. */
#define AVCER_LOSS_CE 0
#define AVCER_LOSS_SOFT_FOCAL 1
#define AVCER_LOSS_MAX_CLASSES 16
int avcer_window_losses(avcer_ctx* ctx, const float* logits, const int32_t* targets, const float* weights, int64_t n, int c, int kind,
                        double label_smoothing, double gamma, int64_t batch_size, double* row_loss, double* batch_loss, double* epoch,
                        int32_t* ticket, avcer_stream_t stream);

/* The concordance correlation coefficient of two float64 series (accuracy_utils.ccc_score, src/audio/utils/accuracy_utils.py:124-152).
 * targets, predicts f64 on the device, n elements each, element i at [i * stride] (stride 2 reads one column of an [n, t, 2]
 * valence / arousal table: v_score / a_score).  Two passes in float64, sums in the order of avcer_window_losses:
 *   mt = sum(t) / n, mp = sum(p) / n;  vy = t - mt, vx = p - mp;  sxy = sum(vx * vy), sxx = sum(vx * vx), syy = sum(vy * vy)
 *   cor = sxy / (sqrt(sxx) * sqrt(syy));  sdt = sqrt(syy / n), sdp = sqrt(sxx / n)
 *   out[0] = ((2 * cor) * sdt) * sdp / ((sdt * sdt + sdp * sdp) + (mt - mp) * (mt - mp))
 * A constant series (and n = 1) gives 0 / 0 = NaN, as numpy does.  One launch of one block.  out f64 [1] on the device.
 * Limits: 1 <= n, 1 <= stride, (n - 1) * stride < 2^40.  No host synchronisation. */
int avcer_ccc(avcer_ctx* ctx, const double* targets, const double* predicts, int64_t n, int64_t stride, double* out,
              avcer_stream_t stream);

/* Fitting the audio classifier head: the train phase of NetTrainer.run for the last layer, feature_downsample (Linear f -> c), on
 * features extracted once; k_runs independent runs (seeds, rates, losses, mixup settings) in ONE launch, one workgroup a run.
 *   ref: src/audio/net_trainer/net_trainer.py:357-467 (iterate_model), 574-604 (mixup_data), src/audio/train_c_audio.py:236-260
 *        (the losses, torch.optim.Adam, CosineAnnealingWarmRestarts stepped with epoch + idx / iters)
 * DEVICE: feats f32 [n, f]; targets i32 [n] in [0, c); class_w f32 [k_runs, c] (ones for an unweighted loss); w0 f32 [k_runs, c, f],
 * b0 f32 [k_runs, c]; order i32 [k_runs, epochs, n], per epoch a permutation of 0 .. n-1; mix_lam f32 [k_runs, epochs, n_batches] and
 * mix_index i32 [k_runs, epochs, n] (per batch a permutation of the positions 0 .. n_b-1 inside it), both NULL when no run mixes;
 * hyper_dev f64 [k_runs, AVCER_HEAD_HYPER], scratch the call fills.  HOST: hyper f64 [k_runs, AVCER_HEAD_HYPER] = kind
 * (AVCER_LOSS_CE / AVCER_LOSS_SOFT_FOCAL), label_smoothing, gamma, lr, beta1, beta2, eps, t0, eta_min, mixup (0 / 1), first_epoch (the trainer's number of
 * epoch 0 of this call: NetTrainer.run counts from 1), 0; it is checked here and copied in stream order.  n_batches = ceil(n / batch_size); batch i of epoch e holds the rows
 * order[e, i * batch_size ..], n_b of them, the last batch may be short.
 * One step (e, i), f32 unless said otherwise, every operation rounded on its own except the two fmaf chains:
 *   x[b, :] = feats[row_b, :], or with mixup lam * feats[row_b, :] + (1 - lam) * feats[row_{index[b]}, :], the label being
 *     y_b = (lam > 1 - lam) ? y : (lam < 1 - lam) ? y' : min(y, y')  (argmax of the mixed one-hot rows, first maximum);
 *   logits[b, k] = S + bias[k], S summed in this FIXED order: thread t of 256 owns the columns t, t + 256, .. and chains
 *     fmaf(x[b, col], W[k, col], .) over them upwards from 0; eight adders take 32 consecutive threads' partials each, one after
 *     the other from the first; the eight sums fold in halves ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
 *   the loss of row b exactly as avcer_window_losses states it, in f32; its sums A, G, U over the batch in that entry's order
 *     (thread b holds row b; 256 partials fold in halves); batch_loss as there;
 *   G[b, k] = d batch_loss / d logits[b, k], with p = softmax(logits[b]), W_ = ((w[0] + w[1]) + ..):
 *     CE          ((1 - eps) * (w[y] * (p[k] - [k == y])) + (eps / c) * (W_ * p[k] - w[k])) / U
 *     SOFT_FOCAL  ((D * p[y]) * ([k == y] - p[k])) / n_b,  D = w[y] * (g' * log(pc) - fo / pc) while 1e-7 <= p[y] <= 1 - 1e-7, else
 *                 0 (the clip), pc the clipped p[y], fo = (1 - pc)^gamma, g' = gamma * (1 - pc)^(gamma - 1) (0 for gamma == 0);
 *   dW[k, col] = fmaf(G[b, k], x[b, col], .) over b = 0, 1, .. from 0, by the thread that owns col;  db[k] = ((G[0, k] + G[1, k]) + ..);
 *   Adam (no weight decay, no amsgrad), step s = 1, 2, ..: m += (1 - beta1) * (g - m);  v = v * beta2 + ((1 - beta2) * g) * g;
 *     W -= step_size * (m / (sqrt(v) / bc2 + eps)), step_size = f32(lr_s / (1 - beta1^s)), bc2 = f32(sqrt(1 - beta2^s)), the two
 *     computed in double, beta^s as a running product;
 *   lr for the next step, in double: eta_min + (lr - eta_min) * (1 + cos(pi * T / t0)) / 2, T = (first_epoch + e) + i / n_batches, taken mod t0 once
 *     it reaches t0 (T_mult = 1).  The first step runs at lr.
 * There are no atomics, no tickets and no waits but workgroup barriers: a run's outputs are a pure function of its inputs, the
 * same bits alone as among k_runs.  W, b, m and v of a run stay in its workgroup's registers from the first step to the last:
 * 3 * c * f floats over 256 threads, so c * f <= AVCER_HEAD_MAX_STATE (every c <= 16 at every f <= 1024).
 * A row number outside [0, n), a mixup position outside [0, n_b) or a target outside [0, c) is checked where it is read and
 * turns the step's loss (and the weights behind it) into NaN; nothing is indexed with it.  Callers validate them beforehand.
 * Outputs (device): w_hist f32 [k_runs, epochs, c, f] and b_hist f32 [k_runs, epochs, c], the state at the end of every epoch;
 * batch_loss f32 [k_runs, epochs, n_batches]; epoch_loss f64 [k_runs, epochs] = sum_i(f64(batch_loss) * batch_size) / n_batches,
 * the short batch counting with the full size (net_trainer.py:441,460), added in double in step order.
 * Limits (AVCER_EINVAL beyond them, before any launch): 1 <= n <= AVCER_HEAD_MAX_ROWS; f a multiple of 64, 64 .. AVCER_HEAD_MAX_FEATURES;
 * 2 <= c <= AVCER_LOSS_MAX_CLASSES; c * f <= AVCER_HEAD_MAX_STATE; 1 <= batch_size <= AVCER_HEAD_MAX_BATCH; 1 <= epochs <=
 * AVCER_HEAD_MAX_EPOCHS; 1 <= k_runs <= AVCER_HEAD_MAX_RUNS; epochs * n_batches <= AVCER_HEAD_MAX_STEPS; per run a known kind,
 * label_smoothing in [0, 1], gamma >= 0, betas in [0, 1), eps >= 0, t0 an integer >= 1, first_epoch an integer >= 0, all of them, lr and eta_min finite.
 * One host-to-device copy of `hyper` in stream order; no host synchronisation beyond it. */
#define AVCER_HEAD_HYPER 12
#define AVCER_HEAD_MAX_BATCH 256
#define AVCER_HEAD_MAX_FEATURES 1024
#define AVCER_HEAD_MAX_STATE 16384
#define AVCER_HEAD_MAX_ROWS 268435455LL
#define AVCER_HEAD_MAX_EPOCHS 1048576
#define AVCER_HEAD_MAX_RUNS 1048576
#define AVCER_HEAD_MAX_STEPS 1073741824LL
#define AVCER_HEAD_MAX_HEADS 65535
int avcer_head_fit(avcer_ctx* ctx, const float* feats, const int32_t* targets, int64_t n, int f, int c, int k_runs, int epochs,
                   int batch_size, const double* hyper, double* hyper_dev, const float* class_w, const float* w0, const float* b0,
                   const int32_t* order, const float* mix_lam, const int32_t* mix_index, float* w_hist, float* b_hist,
                   float* batch_loss, double* epoch_loss, avcer_stream_t stream);

/* The logits of a feature table under many heads: logits[h, i, k] = S + b[h, k], S = sum_col feats[i, col] * w[h, k, col].
 * DEVICE: feats f32 [m, f], w f32 [heads, c, f], b f32 [heads, c] -> logits f32 [heads, m, c] (heads = runs x epochs of
 * avcer_head_fit's w_hist / b_hist).  S in a FIXED order that depends on f alone: lane l of a wave chains fmaf(x, w, .) over the
 * columns l, l + 64, .. upwards from 0; the 64 partials fold by lane exchange at distances 32, 16, 8, 4, 2, 1.  One head alone
 * gives the bits it gives among many.  One launch; one wave per four rows and head.
 * Limits: 1 <= m <= AVCER_HEAD_MAX_ROWS, f a multiple of 64 up to AVCER_HEAD_MAX_FEATURES, 2 <= c <= AVCER_LOSS_MAX_CLASSES,
 * 1 <= heads <= AVCER_HEAD_MAX_HEADS.  No host synchronisation. */
int avcer_head_apply(avcer_ctx* ctx, const float* feats, const float* w, const float* b, int64_t m, int f, int c, int heads,
                     float* logits, avcer_stream_t stream);

/* avcer_head_fit with the feature rows of every epoch taken from one of `views` tables: feats f32 [views, n, f] (the same windows
 * under `views` draws of the waveform augmentation, avcer_wave_augment), view i32 [k_runs, epochs] (device): epoch e of run r reads
 * row_b at feats[view[r, e], row_b, :], the mixup partner from the same table.  Targets, order and the mixup tables are per window
 * and do not change with the view.  A view outside [0, views) turns every step of its epoch into NaN, as an invalid row does;
 * callers validate beforehand.  Everything else is avcer_head_fit's, which is this call with views = 1 and view = NULL (all 0):
 * one kernel body serves both.  Limits: those of avcer_head_fit and 1 <= views, views * n <= AVCER_HEAD_MAX_ROWS. */
int avcer_head_fit_views(avcer_ctx* ctx, const float* feats, int views, const int32_t* view, const int32_t* targets, int64_t n, int f,
                         int c, int k_runs, int epochs, int batch_size, const double* hyper, double* hyper_dev, const float* class_w,
                         const float* w0, const float* b0, const int32_t* order, const float* mix_lam, const int32_t* mix_index,
                         float* w_hist, float* b_hist, float* batch_loss, double* epoch_loss, avcer_stream_t stream);

/* The waveform augmentations of the reference's training windows, in place on the padded windows avcer_audio_chunks(mode 1) wrote
 * and in front of the forward's normalisation: one of PolarityInversion, WhiteNoise, Gain per window, chosen on the host.
 *   ref: src/audio/train_c_audio.py:112-119 (RandomChoice([PolarityInversion(), WhiteNoise(), Gain()]) on every training window),
 *        src/audio/augmentation/wave_augmentation.py:8-108
 *        torchaudio==2.1.2 transforms/_transforms.py Vol.forward, functional/functional.py gain (third party, BSD-2): `waveform *
 *        10 ** (gain_db / 20)`, the Python float as a float32 scalar, then torch.clamp(waveform, -1, 1)
 * DEVICE: chunks f32 [n, win], changed in place; recs_dev [n] and parts f64 [n, P, 2] (P below; at least one element), scratch the call fills;
 * noise f32 [n, win] or NULL; std_out f32 [n] or NULL.  HOST: recs [n], one avcer_augment_rec per window, checked here and copied
 * in stream order.  Per window, by rec.kind:
 *   AVCER_AUGMENT_NONE      nothing: the window's bytes are neither read nor written;
 *   AVCER_AUGMENT_POLARITY  x = -x (torch.neg);
 *   AVCER_AUGMENT_NOISE     std = torch.std(window): sqrt(sum((x - mean)^2) / (win - 1)) over all win samples, the padding zeros
 *       among them, accumulated in f64 in an order that depends on win alone (below) and rounded to f32 (std_out[w], if given);
 *       noise_std = lo + (hi - lo) * rec.u in f64, lo = min_snr * (double)std, hi = max_snr * (double)std (random.uniform);
 *       x[i] = x[i] + (float)(noise_std * (double)z[i]), the sum in f32.  z[i] is lane i % 4 of Philox4x32-10 (Salmon et al.,
 *       SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key steps 0x9E3779B9, 0xBB67AE85) at counter (i / 4, 0) -- low word, high word,
 *       0, 0 -- under key (rec.key & 0xffffffff, rec.key >> 32); lanes (0, 1) and (2, 3) are Box-Muller pairs: with words a, b
 *       u1 = ((a >> 8) + 1) * 2^-24, u2 = (b >> 8) * 2^-24, r = sqrtf(-2 * logf(u1)), z = r * cospif(2 * u2), r * sinpif(2 * u2)
 *       with the accurate f32 functions: |z| <= 5.77.  win == 1 gives std = 0 / 0 = NaN and a NaN window, as the reference does; a
 *       window of zeros stays zeros; a NaN sample makes the window NaN.
 *       With `noise`: x[i] = x[i] + noise[w, i] instead (the reference's own draw fed through); std is not computed.
 *   AVCER_AUGMENT_GAIN      g = x * rec.ratio; x = g < -1 ? -1 : g > 1 ? 1 : g (torch.clamp: NaN stays).
 * The order of std: the window is cut into P = ceil(win / CH) parts of CH = 4096 * ceil(win / 2^20) samples (P <= AVCER_AUGMENT_PARTS);
 * a part's sum S_p: thread t of 256 adds the samples of its quads (four consecutive samples) t, t + 256, .. of the part upwards,
 * the 256 partials fold in halves; M_p = sum((x - S_p / len_p)^2) the same way; then mean = fold(S_p) / win and
 * sum((x - mean)^2) = fold(M_p + len_p * (S_p / len_p - mean)^2), both folds over 256 slots (those at and behind P hold 0) in halves.
 * No atomics; two launches give the same bits; a window alone gives the bits it gives among n, whatever its place and however the
 * windows are split into calls.  Two launches of n * P workgroups (one when no window is of kind 2 or `noise` is given, none when
 * all are of kind 0).  n == 0 returns at once.
 * Limits (AVCER_EINVAL beyond them, before any launch): 1 <= win <= AVCER_AUGMENT_MAX_WIN (what avcer_audio_chunks takes),
 * n * win <= AVCER_AUGMENT_MAX_ELEMS, n * P < 2^31; min_snr <= max_snr, both finite; per window a known kind, u in [0, 1), a ratio
 * that is a number.  One host-to-device copy of `recs` in stream order; no host synchronisation beyond it. */
#define AVCER_AUGMENT_NONE 0
#define AVCER_AUGMENT_POLARITY 1
#define AVCER_AUGMENT_NOISE 2
#define AVCER_AUGMENT_GAIN 3
#define AVCER_AUGMENT_PARTS 256
#define AVCER_AUGMENT_MAX_WIN 2147483647LL
#define AVCER_AUGMENT_MAX_ELEMS 1099511627776LL
typedef struct avcer_augment_rec {
    int32_t kind;   /* AVCER_AUGMENT_* */
    float ratio;    /* kind 3: 10 ** (gain_db / 20) rounded to float32 */
    double u;       /* kind 2: the window's uniform draw in [0, 1) */
    uint64_t key;   /* kind 2: the Philox key of the window's noise */
} avcer_augment_rec;
int avcer_wave_augment(avcer_ctx* ctx, float* chunks, int64_t n, int64_t win, const avcer_augment_rec* recs, avcer_augment_rec* recs_dev,
                       double min_snr, double max_snr, const float* noise, double* parts, float* std_out, avcer_stream_t stream);

/* The contraction kernel itself (implicit-GEMM convolution with fused epilogue), exported for kernel-level
 * parity tests and micro-benchmarks:  Y[m, n] = act(scale[n] * sum_k A[m,k] * W[n,k] + bias[n] (+ R[m,n]))
 * where A is gathered from an NHWC tensor.  See avcer_conv_desc. dtype: 0 = f32 in/out, 1 = bf16 in/out,
 * 2 = bf16 in / f32 out; split-fp16 ("x3") arithmetic with w pre-split by avcer_split_weight_rows: 3 = f32 in / f32 out,
 * 4 = f32 in / sp32 out, 5 = sp32 in / sp32 out (+ sp32 residual), 6 = sp32 in / f32 out (+ f32 residual);
 * 7 / 8 = 5 / 6 with w in fragment order (avcer_weight_frags): the weights-direct form of the kernel, bit-identical results,
 * for n % 256 == 0, an even number of 32-element K-steps and groups <= 1 (anything else is AVCER_EINVAL: use 5 / 6);
 * 9 / 10 = 5 / 6 with w in fragment order once more, the "skinny" form for launches of few positions (one frame or one window
 * per call, the deep layers of a small batch): one WAVE per (16 | 32 | 64 positions) x 16 channels, registers only, no LDS, no
 * barrier; bit-identical results as well.  Requires cin % 32 == 0 and n % 32 == 0 (per group), no second source (x2_cin == 0);
 * grouped convolutions are supported (one launch, as for 5 / 6); M is not limited by the kernel.  tile_m = 16, 32 or 64 picks
 * the positions per wave tile (0: the smallest tile that leaves half of the chip's SIMDs free); tile_n does not apply.  Anything
 * else is AVCER_EINVAL: use 5 / 6.  The networks choose it while (M / 32) * (n / 16) wave tiles fit the chip's SIMDs in one
 * round and M <= 4096 (csrc/gemm_forms.h prefer_skinny).
 * "sp32" storage = per aligned group of 32 channels, 32 fp16 hi values then 32 fp16 lo values (x = hi + lo), i.e. the
 * layout avcer_split_weights produces; 4 bytes per element. */
typedef struct avcer_conv_desc {
    int32_t batch, in_h, in_w;       /* input extents used for bounds (zero padding outside) */
    int32_t out_h, out_w;            /* M = batch*out_h*out_w */
    int32_t cin;                     /* contiguous channels per tap (multiple of 8; of 4 for f32; of 32 for sp32).  With more than
                                        one tap and cin not a multiple of the K-step (32 elements; 64 for bf16) a K-step may span
                                        two taps but not three: f32 input accepts cin 16, 24, 28 and any cin > 32, bf16 accepts
                                        cin 32, 48, 56 and any cin > 64; the rest (f32 4, 8, 12, 20; bf16 8, 16, 24, 40) is
                                        AVCER_EINVAL */
    int32_t kh, kw;                  /* taps; K = kh*kw*cin */
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int64_t x_stride_b, x_stride_h, x_stride_w; /* element strides of the input */
    int32_t x_coff;                  /* channel offset into the input pixel */
    int32_t n;                       /* output channels (multiple of 64) */
    int64_t y_ld; int32_t y_coff;    /* output row stride (elements) and channel offset */
    int64_t r_ld; int32_t r_coff;    /* residual row stride / offset (if residual != NULL) */
    int32_t act;                     /* 0 none, 1 relu, 2 gelu(erf), 3 gelu with the Abramowitz-Stegun 7.1.26 erf: within 4.7e-7 of
                                        the exact function (the f32 rounding of the exact form itself), a third of the
                                        instructions; what the library uses around bf16 / split-fp16 contractions */
    int32_t res_after_act;           /* 0: act(v + r), 1: act(v) + r */
    int32_t groups;                  /* 0/1 = plain; G > 1 = grouped convolution in ONE launch: group g reads input
                                        channels x_coff + g*cin, uses weight rows [g*n, (g+1)*n) of w (and scale/bias
                                        entries g*n..), and writes / adds channels y_coff + g*n, r_coff + g*n */
    /* Optional second A source for avcer_conv_gemm_dual (two fused 1x1 convolutions, e.g. ResNet conv3 + downsample):
     * K elements [kh*kw*cin, kh*kw*cin + x2_cin) of every row come from x2 at position (oy*x2_stride, ox*x2_stride). */
    int32_t x2_cin, x2_coff, x2_stride;
    int64_t x2_stride_b, x2_stride_h, x2_stride_w;
    int32_t tile_n;                  /* output-channel width of the block tile: 0 = chosen by the library, 64 or 128 (n % 128 == 0);
                                        dtypes 7 / 8 always use 256 (0 or 256).  A tuning knob: results do not depend on it. */
    /* Sub-sampled residual (r_sub > 1): the residual tensor lives on a [batch, r_h, r_w] grid of rows of r_ld elements and
     * output position (b, oy, ox) adds its row (b, oy * r_sub, ox * r_sub) -- the last bottleneck of a ResNet stage computed
     * only at the positions the next stage's stride-2 1x1 convolutions read.  0 / 1: one residual row per output row. */
    int32_t r_sub, r_h, r_w;
    int32_t tile_m;                  /* dtypes 7 / 8: positions per block tile, 0 = chosen by the library (whichever of 112 / 128
                                        leaves the cheaper last round on the 512 block slots), 112 or 128.  Dtypes 9 / 10:
                                        positions per WAVE tile, 0 = chosen by the library, 16, 32 or 64.  A tuning knob like
                                        tile_n: an element's accumulation order, hence the result, does not depend on it. */
} avcer_conv_desc;

int avcer_conv_gemm(avcer_ctx* ctx, const avcer_conv_desc* d, int dtype, const void* x, const void* w,
                    const float* scale, const float* bias, const void* residual, void* y, avcer_stream_t stream);

/* Same contraction with a second activation tensor supplying the tail of K (see avcer_conv_desc.x2_*); w is
 * [n][kh*kw*cin + x2_cin].  Both sources must be 1x1 / unpadded. */
int avcer_conv_gemm_dual(avcer_ctx* ctx, const avcer_conv_desc* d, int dtype, const void* x, const void* x2, const void* w,
                         const float* scale, const float* bias, const void* residual, void* y, avcer_stream_t stream);

/* Fused kernels of the static CNN in the split-fp16 arithmetic (csrc/fused.hip), exported for kernel-level parity tests.
 *
 * avcer_bneck_chain: the tail of one ResNet bottleneck and the head of the next in ONE launch,
 *     T2 = relu(conv3x3(T1) + b2);  OUT = relu(conv1x1(T2) + b3 + X);  T1N = relu(conv1x1(OUT) + b1n)
 *   ref: architectures/video.py:43-60 (Bottleneck.forward; stride 1, no downsample), BatchNorm folded.
 *   t1 sp32 [nb,h,w,planes], x / out sp32 [nb,h,w,4*planes], t1n sp32 [nb,h,w,planes] or NULL (then w1n, b1n NULL);
 *   w2 [planes][9*planes], w3 [4*planes][planes], w1n [planes][4*planes]: BN scale folded into the rows, then split
 *   by avcer_split_weight_rows; b2 / b3 / b1n f32 BN shifts in natural channel order.  planes = 64 or 128.
 *   ds_cin = 64 (planes 64 only, t1n required): the FIRST block of a stage without spatial stride (video.py:43-60 with
 *   i_downsample): x is the 64-channel block input sp32 [nb,h,w,64], w3 is [4*planes][planes + 64] = conv3 and the
 *   downsample convolution concatenated along K (both BN scales folded, shifts summed into b3), and nothing is added.
 *   out_step = 2 (t1n NULL, ds_cin 0): the LAST block of a stage, whose output only the next stage's stride-2 1x1
 *   convolutions read (video.py:12-19,140-149): T2 and OUT are evaluated at positions (2 oy, 2 ox) alone and out is the compact
 *   sp32 [nb, (h+1)/2, (w+1)/2, 4*planes]; t1 and x keep their [nb,h,w] grids.  out_step = 1: every position.
 *   w2_frags (may be NULL): the conv2 weights once more in MFMA fragment order (avcer_weight_frags of the same matrix).  With
 *   it, planes 64 on 55 x 55 images with a next conv1 runs the spatial-tile form (11 x 11 tiles, resident halo patch, the
 *   conv2 output channels split across the block's waves so that every weight fragment goes straight into the registers of
 *   ONE wave); results are bit-identical to the form without it.
 *
 * avcer_bneck_tail: stage 3 (planes 256), where conv2 stays a contraction launch of its own: conv3 + residual + ReLU and the next
 *   block's conv1 in ONE launch (bneck_tail2_kernel),
 *     OUT = relu(conv1x1(T2) + b3 + X);  T1N = relu(conv1x1(OUT) + b1n)
 *   ref: architectures/video.py:49-58 (the second half of Bottleneck.forward) and :45-46 of the next block, BatchNorm folded.
 *   t2 sp32 [M][256]; x / out sp32 [M][1024]; t1n sp32 [M][256] (required); w3 [1024][256], w1n [256][1024]: BN scale folded
 *   into the rows, then split by avcer_split_weight_rows; b3 [1024] / b1n [256] f32.  planes must be 256, M >= 1 and below
 *   2^20 - 1 positions (OUT is stored through a 4 GiB buffer descriptor).  The forward passes run it above 16384 positions per
 *   call and the same two contractions as avcer_conv_gemm launches below (bit-identical results).
 *
 * avcer_stem_pool: conv 7x7/2 (TF-"same" padding) + BN + ReLU + max-pool 3x3/2 in one launch,
 *   ref: architectures/video.py:63-90,98-103,116-117.  planes_hi_lo: two fp16 planes [n,230,230,4] (hi, then lo plane_bytes
 *   later) of the zero-bordered preprocessed image as avcer_static_forward builds it; w split [64][7*32] (tap rows of
 *   8 pixels x 4 channels); scale / bias f32 [64]; y sp32 [n,55,55,64]. */
int avcer_bneck_chain(avcer_ctx* ctx, int planes, int nb, int h, int w, const void* t1, const void* x, int ds_cin, int out_step,
                      void* out, void* t1n, const void* w2, const float* b2, const void* w3, const float* b3, const void* w1n,
                      const float* b1n, const void* w2_frags, avcer_stream_t stream);
int avcer_bneck_tail(avcer_ctx* ctx, int planes, int64_t M, const void* t2, const void* x, void* out, void* t1n, const void* w3,
                     const float* b3, const void* w1n, const float* b1n, avcer_stream_t stream);
/* The same two launches with a row-keep step for `out`, for kernel-level tests of what avcer_set_skip_unread_rows selects.
 *   keep = 1: every row of out is stored (avcer_bneck_chain with ds_cin 0 and out_step 1; avcer_bneck_tail with M = nb * h * w).
 *   keep = 2: only the rows at even (y, x) of each of the nb images of h x w positions are stored, at their full-grid addresses;
 *   the other rows of out keep what the caller put there.  t1n is written at every position either way.  avcer_bneck_chain_keep
 *   requires t1n / w1n / b1n (the block in front of a strided last block always has a next conv1). */
int avcer_bneck_chain_keep(avcer_ctx* ctx, int planes, int nb, int h, int w, const void* t1, const void* x, void* out, void* t1n,
                           const void* w2, const float* b2, const void* w3, const float* b3, const void* w1n, const float* b1n,
                           const void* w2_frags, int keep, avcer_stream_t stream);
int avcer_bneck_tail_keep(avcer_ctx* ctx, int planes, int nb, int h, int w, const void* t2, const void* x, void* out, void* t1n,
                          const void* w3, const float* b3, const void* w1n, const float* b1n, int keep, avcer_stream_t stream);
/* One conv_dw block of MobileNet-0.25 (retina_face_net.py:29-38) in ONE launch (csrc/mnet.hip dwsep_kernel), for kernel-level tests:
 *     T = leaky(dw3x3(X, stride, pad 1) * dw_s + dw_b);  Y = leaky(conv1x1(T) * pw_s + pw_b),  leaky = LeakyReLU(0.1)
 *   x f32 NHWC [nb,h,w,cin] -> y f32 NHWC [nb,ceil(h/stride),ceil(w/stride),cout]; T never reaches memory.
 *   (cin, cout, stride): one of (8,16,1) (16,32,2) (32,32,1) (32,64,2) (64,64,1) (64,128,2) (128,128,1) (128,256,2) (256,256,1).
 *   dw_w f32 [9][cin] (tap-major); dw_s, dw_b [cin]; pw_s, pw_b [cout]; pw_w = the pointwise matrix zero-padded to
 *   [ceil64(cout)][ceil32(cin)]: f32 in AVCER_MODE_FP32 (f32 MFMA), its avcer_split_weight_rows copy in AVCER_MODE_F16X3 (three
 *   fp16 MFMAs per term, every depthwise output split as one f32 number, |T| >= 65520 counted by avcer_x3_overflow_count). */
int avcer_dwsep(avcer_ctx* ctx, int cin, int cout, int stride, int mode, int nb, int h, int w, const float* x, const float* dw_w,
                const float* dw_s, const float* dw_b, const void* pw_w, const float* pw_s, const float* pw_b, float* y,
                avcer_stream_t stream);
/* Kernel-level entries of csrc/s3fd.hip, for tests.  `kind`: storage of the activations, 0 = f32, 2 = sp32 (AVCER_MODE_F16X3).
 *   avcer_s3fd_stem: u8 frames [n,h,w,3] -> ReLU(conv 3x3 pad 1 (3 -> 64) of RGB pixel - (123, 117, 104) + bias): y [n,h,w,64];
 *     wt f32 [27][64], taps (ky, kx, c) major; rgb == 0: the frames are BGR.
 *   avcer_maxpool2: nn.MaxPool2d(2, 2, ceil_mode) on NHWC x [n,h,w,c] -> y [n,h/2,w/2,c] (ceil_mode: ceil of both; a window over
 *     the edge takes the maximum of what exists); c a multiple of 4 (sp32: of 32).
 *   avcer_s3fd_head: one S3FD level's loc + conf 3x3 convolutions (padding 1) as one direct convolution: x [nb,h,w,c], c a multiple of
 *     256; wt f32 [9][c][n_out], columns 0-3 loc, 4.. conf; n_out 8 (level 0: conf = (max of columns 4-6, column 7)) or 6; the two
 *     conf values are softmaxed; rows go to loc [.., n_priors, 4] / conf [.., n_priors, 2] at frame * n_priors + row0.  inv_norm:
 *     NULL, or scratch for nb*h*w floats: every tap is then multiplied by 1 / (sqrt(sum_c x^2) + 1e-10) of its position (L2Norm
 *     with its weight folded into wt; an all-zero position contributes 0). */
int avcer_s3fd_stem(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int rgb, const float* wt, const float* bias, void* y,
                    int kind, avcer_stream_t stream);
int avcer_maxpool2(avcer_ctx* ctx, const void* x, void* y, int n, int h, int w, int c, int ceil_mode, int kind, avcer_stream_t stream);
int avcer_s3fd_head(avcer_ctx* ctx, const void* x, int kind, float* inv_norm, const float* wt, const float* bias, int nb, int h, int w,
                    int c, int n_out, int row0, int n_priors, float* loc, float* conf, avcer_stream_t stream);
int avcer_stem_pool(avcer_ctx* ctx, const void* planes_hi_lo, size_t plane_bytes, const void* w, const float* scale,
                    const float* bias, void* y, int n, avcer_stream_t stream);
/* The same launch fed with the u8 frames themselves ([n,in_h,in_w,3] RGB; data/utils.py:19-39 -- NEAREST resize to 224, BGR flip,
 * mean subtraction -- happens inside): raw pixel values are exact in fp16, so the stem runs two MFMAs per product, and the
 * channel means move into shifts9 f32 [9][64] = BN shift - BN scale * (sum over the taps inside the image of w * mean), one
 * row per border class 3 * row_class + col_class (0: first stem row / column, 1: interior, 2: row / column 110; see
 * avcer_amd/packing.py stem_border_shifts).  What avcer_static_forward runs in AVCER_MODE_F16X3. */
int avcer_stem_pool_u8(avcer_ctx* ctx, const uint8_t* frames, int n, int in_h, int in_w, const void* w, const float* scale,
                       const float* shifts9, void* y, avcer_stream_t stream);

/* The sp32 split of an ACTIVATION tensor (what a producer's epilogue writes with dtype 4 / 5): for every group of 32
 * elements, 32 fp16 "hi" values then 32 fp16 "lo" values with x = hi + lo (+ O(2^-22 |x|); |x| < 65504).  x f32 [numel] (a
 * multiple of 32) -> out, same size in bytes, no scaling.  Both device pointers.  NOT a weight layout: the weights of dtypes
 * 3-8 are scaled, carry a trailer and have their rows permuted (avcer_split_weight_rows below). */
int avcer_split_weights(avcer_ctx* ctx, const float* w, void* out, size_t numel, avcer_stream_t stream);

/* Bytes behind the n * k * 4 bytes of a split WEIGHT matrix that hold its scale: float [0] = the power of two a consumer
 * multiplies its accumulators by (the inverse of the scale the weights were split at), word [1] = max |w| as float bits.
 * Every buffer written by avcer_split_weight_rows / avcer_weight_frags is n * k * 4 + AVCER_SPLIT_TRAILER bytes. */
#define AVCER_SPLIT_TRAILER 256

/* The split of a WEIGHT matrix w f32 [n][k] (n, k multiples of 32) as the x3 contractions (dtype 3-6 of avcer_conv_gemm,
 * avcer_bneck_chain, avcer_stem_pool) expect it: every value times the matrix's power-of-two scale (largest magnitude ->
 * [2^14, 2^15): keeps the lo halves of all significant weights normal fp16 numbers), the layout above along K, and the rows
 * of every group of 32 output channels re-ordered so that stored row 16t + 4g + r holds channel 8g + 4t + r (t = 0,1;
 * g = 0..3; r = 0..3).  With weights as the MFMA A operand this leaves each lane with 8 consecutive output channels, i.e.
 * 16-byte pieces of the output row (direct whole-line stores).  scale / bias / residual / output stay in natural channel
 * order and in real units: the kernels undo the weight scale themselves from the trailer.
 * out: n * k * 4 + AVCER_SPLIT_TRAILER bytes. */
int avcer_split_weight_rows(avcer_ctx* ctx, const float* w, void* out, int n, int k, avcer_stream_t stream);

/* The output of avcer_split_weight_rows once more in MFMA fragment order, the weight layout of avcer_conv_gemm dtypes 7 / 8
 * (conv_gemm_wd_kernel: weight fragments go straight from global memory to the registers, only the activation tile passes
 * through LDS): [n/16][k/32][hi, lo][64 lanes][16 bytes], lane l = stored row 16 t + (l & 15), K elements 8 (l >> 4) .. + 8,
 * then the trailer.  Dtypes 9 / 10 read the same copy.  rows, out: device pointers, n * k * 4 + AVCER_SPLIT_TRAILER bytes each; n a multiple of 16, k of 32. */
int avcer_weight_frags(avcer_ctx* ctx, const void* rows, void* out, int n, int k, avcer_stream_t stream);

/* The attention kernel on its own (kernel-level parity tests): softmax(Q K^T * scale) V per (row block, head).
 *   ref: architectures/attention_layers.py:80-144 (ScaledDotProductAttention inside MultiHeadAttention), transformers
 *        Wav2Vec2Attention (eager).
 * qkv [n, s, 3 * heads * head_dim]: per token the queries of all heads, then the keys, then the values (the packed output of
 * the fused q / k / v projection); out [n, s, heads * head_dim].  head_dim 64 or 32, s <= 256.  Storage kinds: 0 = f32,
 * 1 = bf16, 2 = sp32.  (in 0, out 0): exact f32 arithmetic on the VALU; (in 1, out 1): bf16 operands on the MFMA;
 * (in 0, out 2): what AVCER_MODE_F16X3 runs -- f32 in, sp32 out (see the kernel for its arithmetic). */
/* The recurrence of one torch.nn.GRU layer on caller tensors (device pointers, f32), ONE launch with the time loop inside
 * (csrc/gru.hip): xp [n, s, 3h] = x W_ih^T + b_ih for all steps (gate order r, z, n), w_hh [3h, h], b_hh [3h] ->
 * h_seq [n, s, h], h_0 = 0.  h must be 256 (AVCER_EINVAL otherwise).  AVCER_MODE_F16X3 runs the recurrent contraction on the
 * split-fp16 MFMA (w_hh is split and put into fragment order inside the call), the other two modes on the f32 MFMA.
 *   ref: architectures/audio_8_cl.py:26,64 (nn.GRU(1024, 256, num_layers=2, batch_first=True)) */
int avcer_gru_layer(avcer_ctx* ctx, const float* xp, const float* w_hh, const float* b_hh, int n, int s, int h, int mode,
                    float* h_seq, avcer_stream_t stream);

int avcer_attention(avcer_ctx* ctx, const void* qkv, void* out, int n, int s, int heads, int head_dim, float scale,
                    int in_kind, int out_kind, avcer_stream_t stream);
/* The same function for 1 <= s <= AVCER_AUDIO_MAX_TOKENS, same tensors and storage combinations (csrc/attention.hip; DESIGN.md section 5, "Audio windows past 256 tokens"): one
 * workgroup per (row block, head, block of AVCER_ATT_LONG_QB queries); key tiles of AVCER_ATT_LONG_KT keys pass through LDS, and
 * every query row keeps a running maximum, a running denominator and rescaled accumulators (the tail tile is masked).  It always
 * runs the streaming kernels, also at s <= 256, where avcer_attention and the forward passes run the whole-head ones. */
#define AVCER_ATT_LONG_KT 128
#define AVCER_ATT_LONG_QB 128
int avcer_attention_long(avcer_ctx* ctx, const void* qkv, void* out, int n, int s, int heads, int head_dim, float scale,
                         int in_kind, int out_kind, avcer_stream_t stream);

/* Measured ceilings of the GPU this context lives on (about 0.2 s): dense 16-bit MFMA issue rate of a register-only
 * v_mfma_f32_16x16x32_f16 loop in TFLOP/s (the instruction of AVCER_MODE_F16X3; the bf16 form issues at the same rate,
 * tools/f16_probe.hip), and the bandwidth of a 1 GiB -> 1 GiB 16-byte-per-lane copy in TB/s (bytes read + bytes written).
 * bench.py prints them next to the datasheet peaks it divides by.  Uses 2 GiB of workspace. */
int avcer_measure_ceilings(avcer_ctx* ctx, double* mfma16_tflops, double* hbm_copy_tbs, avcer_stream_t stream);

/* Last launch statistics of the dominant kernel (for bench.py's roofline object): number of conv_gemm
 * launches and their summed algorithmic FLOPs since the previous call to this function. */
int avcer_gemm_stats(avcer_ctx* ctx, int64_t* launches, double* flops, int reset);

/* Live timing of the dominant kernel for bench.py's roofline object: while enabled, every conv_gemm launch is
 * bracketed by a pair of HIP events on its launch stream; avcer_profile_read synchronises, returns the summed
 * event durations (ms) and the number of launches since the last read, and rewinds the event pool. */
int avcer_profile_enable(avcer_ctx* ctx, int on);
int avcer_profile_read(avcer_ctx* ctx, double* total_ms, int64_t* launches);
/* The same events by kernel family -- what bench.py's roofline.per_family prices each family with: summed event
 * milliseconds, launches, algorithmic FLOPs and compulsory HBM bytes (every operand read once, every output written once)
 * since avcer_profile_enable / the last read.  Arrays of n_fam <= AVCER_FAM_COUNT entries.  Use INSTEAD of
 * avcer_profile_read (both rewind the event pool). */
enum {
    AVCER_FAM_GEMM = 0,    /* conv_gemm_kernel: A and W tiles through LDS */
    AVCER_FAM_GEMM_WD = 1, /* conv_gemm_wd_kernel: weight fragments direct from global memory (dtype 7 / 8) */
    AVCER_FAM_CHAIN = 2,   /* bneck_kernel: fused bottleneck chains of ResNet stages 1-2 (HBM-bound) */
    AVCER_FAM_TAIL = 3,    /* bneck_tail2_kernel: conv3 + residual + next conv1 of stage 3 */
    AVCER_FAM_STEM = 4,    /* stem_pool(_u8)_kernel */
    AVCER_FAM_SKINNY = 5,  /* conv_gemm_skinny_kernel: one wave per tile, registers only (dtype 9 / 10; launches of few positions) */
    AVCER_FAM_GRU = 6,     /* gru_layer_kernel: a GRU layer's whole recurrence, one block per 16 windows (ExprModelV1's head) */
    AVCER_FAM_COUNT = 7
};
int avcer_profile_read_families(avcer_ctx* ctx, int n_fam, double* ms, int64_t* launches, double* flops, double* bytes);
/* ... and launch by launch, in launch order (tools/wd_traffic.py matches this list with the dispatches of a rocprofv3 --pmc pass of
 * the same step): family (AVCER_FAM_*), event milliseconds, algorithmic FLOPs, compulsory HBM bytes and the contraction's
 * M, N, K (mnk [3 * max_n]) of up to max_n launches; *n = launches recorded since avcer_profile_enable / the last read.  Use
 * INSTEAD of the two reads above (all three rewind the event pool). */
int avcer_profile_read_launches(avcer_ctx* ctx, int64_t max_n, int32_t* fam, double* ms, double* flops, double* bytes, int64_t* mnk,
                                int64_t* n);

/* Debug aid for parity tests: arm a one-shot tap; the next forward pass copies up to `bytes` raw bytes of the
 * named intermediate activation (first sub-batch) into dst_dev.  Names: static "pre", "stem_conv", "stem",
 * "l1b0_c1", "l1b0_c2", "l1b0", "layer1".."layer4", "avgpool"; LSTM "lstm_h1" (layer 1's h of all steps, [n,10,512] f32) and
 * "lstm_h2" (layer 2's h after the last step, [n,256] f32), in every mode; audio "norm", "conv0", "extract", "proj",
 * "posconv", "layer0".."layer11", "w2v", "tl1", "tl2", "td0", "mp", "td4", "pooled".  Activations are NHWC / time-major,
 * f32 in AVCER_MODE_FP32, bf16 in AVCER_MODE_BF16 and sp32 (fp16 hi / lo per 32 channels, see avcer_conv_gemm) in
 * AVCER_MODE_F16X3 (residual streams "proj".."tl2", "avgpool" and the heads are always f32).
 * What differs from the reference's tensors of the same name:
 *   - "layer1", "layer2", "layer3" hold the stage output on the grid the NEXT stage reads, i.e. the reference's tensor at
 *     [:, ::2, ::2] -- [n,28,28,256], [n,14,14,512], [n,7,7,1024]: the last bottleneck of stages 1-3 is evaluated at the
 *     even positions only (its other outputs feed nothing: the next stage's 1x1 convolutions have stride 2); "layer4" is
 *     the full [n,7,7,2048];
 *   - "pre", "stem_conv", "l1b0_c2" exist in AVCER_MODE_FP32 / _BF16 only: AVCER_MODE_F16X3 preprocesses inside the fused
 *     stem and keeps conv2 outputs in registers, so those taps do not fire there.
 * The S3FD detector (NHWC, post-ReLU, in the mode's storage): "s3fd_conv1" (conv1_1, the stem kernel's output), "s3fd_conv3_3",
 * "s3fd_pool3" (the ceil_mode pool, vgg.16), "s3fd_conv4_3", "s3fd_conv5_3" (the three before their L2Norm), "s3fd_fc7",
 * "s3fd_ex1" (extras.1 = conv6_2), "s3fd_ex3" (extras.3 = conv7_2); the four floor pools "s3fd_pool1" (vgg.4), "s3fd_pool2"
 * (vgg.9), "s3fd_pool4" (vgg.23), "s3fd_pool5" (vgg.30); every contraction by its weight name, "out:vgg2.w" .. "out:vgg33.w",
 * "out:ex0.w" .. "out:ex3.w".
 * avcer_debug_tap_copied returns the number of bytes copied, or -1 if the tap did not fire (compare it with the size you
 * expect: a short copy means the tensor is smaller than the buffer, e.g. a sub-sampled stage tap). */
int avcer_debug_tap(avcer_ctx* ctx, const char* name, void* dst_dev, size_t bytes);
int64_t avcer_debug_tap_copied(const avcer_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* AVCER_HIP_H */
