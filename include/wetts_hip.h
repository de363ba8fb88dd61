/*
 * wetts_hip.h -- C ABI of libwetts_hip.so: the MI355X (gfx950) native VITS inference path.
 *
 * This is the drop-in boundary for ONE hot path of wenet-e2e/wetts: SynthesizerTrn.infer()
 * (text encoder -> duration -> length regulate -> flow^-1 -> HiFi-GAN) plus the standalone
 * monotonic-alignment search.  The reference has no FFI seam on this path (it is nn.Modules all
 * the way down), so every entry point below cites the reference Python / C++
 * interface whose arithmetic it replaces.  Citations are relative to the reference repo root.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch / HIP types in any signature (`stream` is a
 *     hipStream_t passed as void*; NULL = the default stream).
 *   - every data pointer is a DEVICE pointer owned by the caller unless the name ends in `_host`.
 *   - activations are contiguous float32, channel-first [B, C, T]; ids / lengths are int64;
 *     masks are float 0/1 [B, T] (the reference's [B,1,T] with the unit dim dropped).
 *   - all launches are stream-ordered and asynchronous; the stage calls never allocate: scratch comes
 *     from the caller's workspace (wetts_workspace_bytes()).  Device memory is allocated by wetts_create()
 *     and by the two precision setters (wetts_set_decoder_precision / wetts_set_flow_precision), which build
 *     their 16-bit / uint8 weight copies when called, on the default stream, and return after it has drained
 *     (set-up calls, like create), and by wetts_load_posterior_encoder (voice conversion, the same kind of set-up
 *     call); wetts_dynamic_quant_conv1d and wetts_set_mrf_timing are validation / measurement
 *     aids and say so at their declarations.
 *   - return value: 0 = ok, negative = error (WETTS_E_*); wetts_last_error() gives the message
 *     of the calling thread's last failure.  Kernels never fall back to a CPU path.
 *   - thread-compatible: one handle may be used from one thread at a time (the reference's
 *     VitsModel has the same contract, runtime/core/model/vits_model.h:30-66).
 */
#ifndef WETTS_HIP_H_
#define WETTS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WETTS_ABI_VERSION 12

#define WETTS_OK 0
#define WETTS_E_INVALID (-1)   /* bad argument / unsupported configuration */
#define WETTS_E_HIP (-2)       /* HIP runtime / launch error               */
#define WETTS_E_WORKSPACE (-3) /* caller workspace too small               */
#define WETTS_E_DOMAIN (-4)    /* reference would raise (spline domain...) */

/* Device-side error flags: conditions only the data can reveal, where the reference raises from
 * inside a module.  Kernels OR these bits into the int32 status word registered with
 * wetts_set_status_word(); the host reads the word back together with y_lengths (the one D2H of
 * infer()) and raises / returns like the reference does. */
#define WETTS_STATUS_SPLINE_DOMAIN 1      /* `assert (discriminant >= 0).all()` transforms.py:171 */
#define WETTS_STATUS_PHONE_ID_RANGE 2     /* nn.Embedding IndexError, encoders.py:48 */
#define WETTS_STATUS_SPEAKER_ID_RANGE 4   /* emb_g IndexError, models.py:239 */
#define WETTS_STATUS_DURATION_NONFINITE 8 /* NaN / inf durations reach .long(), models.py:256 */
#define WETTS_STATUS_ALIGN_TEXT_LONGER 16 /* some x_lengths[b] > y_lengths[b]: no monotonic alignment exists (the
                                           * reference's search, monotonic_align.py:22-57, returns a meaningless path) */
#define WETTS_STATUS_DURATION_NEGATIVE 32 /* a negative frame count given to wetts_counts_to_lengths */
#define WETTS_STATUS_SEGMENT_LONGER 64    /* wetts_slice_ids: an utterance shorter than the decoder segment, or a given
                                           * slice id outside [0, len - segment] (the reference slices out of range) */
#define WETTS_STATUS_TOKEN_ID_RANGE 128   /* wetts_frontend_*: a token id outside [0, vocab_size) (nn.Embedding IndexError) */
#define WETTS_STATUS_TYPE_ID_RANGE 256    /* wetts_frontend_*: a token type id outside [0, type_vocab_size) */
#define WETTS_STATUS_LABEL_RANGE 512      /* wetts_frontend_score*: a label that is neither -100 nor a class (torch's
                                             `IndexError: Target .. is out of bounds` in F.cross_entropy) */
#define WETTS_STATUS_LABEL_AT_PAD 1024    /* wetts_frontend_score*: a label other than -100 at a token whose mask is 0 */

#define WETTS_MAX_STAGES 8
#define WETTS_MAX_RB_KERNELS 8
#define WETTS_MAX_RB_DILATIONS 8

/* Hyper-parameters of one model.  Field meaning == ctor arguments of the reference
 * SynthesizerTrn (wetts/vits/model/models.py:19-51) as splatted from `hps.model`
 * (wetts/vits/inference.py:72-76). */
typedef struct wetts_config {
  int32_t n_vocab;
  int32_t inter_channels;  /* 192 */
  int32_t hidden_channels; /* 192 */
  int32_t filter_channels; /* 768 */
  int32_t n_heads;         /* 2   */
  int32_t n_layers;        /* 6   */
  int32_t kernel_size;     /* 3 (encoder FFN) */
  int32_t window_size;     /* 4 (attentions.py:20) */
  int32_t resblock;        /* 1 or 2 (decoders.py:35) */
  int32_t n_resblock_kernels;
  int32_t resblock_kernel_sizes[WETTS_MAX_RB_KERNELS];
  int32_t n_resblock_dilations; /* per resblock: 3 for "1", 2 for "2" */
  int32_t resblock_dilation_sizes[WETTS_MAX_RB_KERNELS][WETTS_MAX_RB_DILATIONS];
  int32_t n_upsamples;
  int32_t upsample_rates[WETTS_MAX_STAGES];
  int32_t upsample_kernel_sizes[WETTS_MAX_STAGES];
  int32_t upsample_initial_channel;
  int32_t n_speakers;   /* 0 => no emb_g, g = None */
  int32_t gin_channels; /* 256 */
  int32_t use_sdp;      /* 1: StochasticDurationPredictor, 0: DurationPredictor */
  int32_t flow_n_flows;     /* 4  (models.py:133-142) */
  int32_t flow_wn_layers;   /* 4  */
  int32_t flow_kernel_size; /* 5  */
  int32_t sdp_n_flows;      /* 4  (models.py:145-150) */
  int32_t dp_filter_channels; /* 256 (models.py:152-156) */
  /* vocoder: 0 = HiFi-GAN Generator (decoders.py:15-88, the fields above), 1 = VocosGenerator
   * (decoders.py:251-308: ConvNeXt stack + iSTFT head; examples/baker/configs/vocos.json:38-52) */
  int32_t vocoder_type;
  int32_t vocos_channels;    /* 512  */
  int32_t vocos_h_channels;  /* 1536 */
  int32_t vocos_num_layers;  /* 8    */
  int32_t istft_n_fft;       /* 1024 (vocos_out_channels = n_fft + 2) */
  int32_t istft_hop_length;  /* 256  */
  int32_t istft_win_length;  /* 1024 (must equal n_fft) */
  /* VITS2 flows (models.py:73-79, flows.py:340-360): 0 = ResidualCouplingLayer, 1 = "pre_conv"
   * (ResidualCouplingTransformersLayer, flows.py:95-177: 2-layer window-less Encoder on x0),
   * 2 = "pre_conv2" (ResidualCouplingTransformersLayer2, flows.py:16-92: 1-layer Encoder on
   * pre(x0) with the flow's kernel size and the default relative window),
   * 3 = "mono_layer_inter_residual", 4 = "mono_layer_post_residual" (the default when a config sets
   * use_transformer_flows without a type, models.py:74-75): [ResidualCouplingLayer, Flip,
   * MonoTransformerFlowLayer] per flow (flows.py:391-425); the mono layer (flows.py:242-324) is a
   * coupling on I/2 channels whose statistics come from the same 2-layer window-less Encoder + a 1x1 post,
   * 4 with residual_connection=True (reverse: x0 / 2, (x1 - m) / (1 + exp(-logs))) */
  int32_t transformer_flows;
  /* speaker-conditioned text encoder (models.py:87-101, attentions.py:39-48,74-78): at layer 2
   * x = (x + spk_emb_linear(g)) * x_mask */
  int32_t use_spk_conditioned_encoder;
  /* SynthesizerTrn(..., is_onnx=...) (models.py:50,111 -> VocosGenerator, decoders.py:279-283): the iSTFT arithmetic of a
   * Vocos model at create; see wetts_set_istft_mode().  export_onnx.py:59 forces it to 1 for every exported graph.
   * HiFi-GAN models ignore it, as the reference does. */
  int32_t is_onnx;
  int32_t reserved[6];
} wetts_config_t;

typedef struct wetts_model wetts_model_t; /* opaque */

/* ---- library / weight-blob layout (no GPU required) ------------------------------------- */

int32_t wetts_abi_version(void);
/* Message of the calling thread's last failed call.  The reference reports the same conditions as Python exceptions
 * raised from inside its modules (e.g. the spline's discriminant assert, transforms.py:171; an embedding index outside
 * its table, encoders.py:48 / models.py:239). */
const char* wetts_last_error(void);

/* The weight blob is one flat float32 array holding every inference tensor of the reference
 * state_dict in its natural PyTorch layout, weight-norm pairs already folded
 * (w = g * v / ||v||, norm over all dims but 0 -- torch.nn.utils.weight_norm dim=0, as used at
 * decoders.py:41-48,96-153, modules.py:35,49,58).  Names are the reference's state_dict keys
 * with `weight_g`/`weight_v` collapsed to `weight`.  The library is the single source of truth
 * for the order: the host loader enumerates it with these three calls.
 * Replaces: utils/task.py:31-56 load_checkpoint + decoders.py:84-88 remove_weight_norm. */
int32_t wetts_blob_num_tensors(const wetts_config_t* cfg);
/* name_buf gets a NUL-terminated key; shape gets up to 4 dims (unused = 0).
 * offset / numel are in floats. */
int32_t wetts_blob_tensor_info(const wetts_config_t* cfg, int32_t index, char* name_buf,
                               size_t name_buf_len, int64_t* offset, int64_t* numel,
                               int64_t shape[4]);
int64_t wetts_blob_numel(const wetts_config_t* cfg);

/* The posterior encoder's tensors (`enc_q`, PosteriorEncoder(spec_channels, inter, hidden, 5, 1, 16, gin_channels),
 * models.py:125-133, encoders.py:60-99) form a blob of their own, laid out like the main one (folded weight norm,
 * reference keys enc_q.pre.*, enc_q.enc.in_layers.{i}.*, enc_q.enc.res_skip_layers.{i}.*, enc_q.enc.cond_layer.* when
 * gin_channels > 0, enc_q.proj.*).  Only voice conversion needs them; the main blob does not change.  spec_channels is
 * the checkpoint's n_fft / 2 + 1 (513 for every recipe: filter_length 1024). */
int32_t wetts_posterior_blob_num_tensors(const wetts_config_t* cfg, int32_t spec_channels);
int32_t wetts_posterior_blob_tensor_info(const wetts_config_t* cfg, int32_t spec_channels, int32_t index,
                                         char* name_buf, size_t name_buf_len, int64_t* offset, int64_t* numel,
                                         int64_t shape[4]);
int64_t wetts_posterior_blob_numel(const wetts_config_t* cfg, int32_t spec_channels);

/* The duration posterior's own blob (SynthesizerTrn.duration_loss): what StochasticDurationPredictor.forward(
 * reverse=False) reads beyond the main blob (duration_predictors.py:176-195) -- dp.flows.1.* (the ConvFlow the reverse
 * pass drops), dp.post_pre / post_proj / post_convs.* and dp.post_flows.{0,1,3,5,7}.*.  Same conventions as the main
 * blob; it has no tensors for a use_sdp = 0 config. */
int32_t wetts_duration_blob_num_tensors(const wetts_config_t* cfg);
int32_t wetts_duration_blob_tensor_info(const wetts_config_t* cfg, int32_t index, char* name_buf, size_t name_buf_len,
                                        int64_t* offset, int64_t* numel, int64_t shape[4]);
int64_t wetts_duration_blob_numel(const wetts_config_t* cfg);

/* ---- model lifetime ---------------------------------------------------------------------- */

/* Builds a model on the CURRENT HIP device from a device-resident blob (e.g. the buffer an
 * RCCL broadcast just filled).  Repacks conv weights into MFMA fragment order on the device.
 * The blob may be freed after the call returns.  Replaces SynthesizerTrn.__init__ + .to(device)
 * + load_checkpoint (inference.py:72-80). */
int32_t wetts_create(const wetts_config_t* cfg, const float* blob_dev, int64_t blob_numel,
                     void* stream, wetts_model_t** out);
/* Frees the packed weights and the model (the reference: garbage collection of the nn.Module built at
 * inference.py:66-80).  Not stream-ordered: the caller synchronises the streams that used the model first. */
void wetts_destroy(wetts_model_t* m);

/* Registers the device int32 the stage calls below OR their WETTS_STATUS_* bits into (caller-owned;
 * zeroed here, stream-ordered; NULL = flags are dropped, ids are still clamped for memory safety).
 * wetts_infer() uses a word of its own workspace and maps it to its return code. */
int32_t wetts_set_status_word(const wetts_model_t* m, int32_t* status_dev, void* stream);

/* Seed of the model's own standard-normal stream (Philox4x32-10), used by wetts_infer() when
 * eps_w / eps_z are NULL -- the reference draws them with torch.randn / torch.randn_like from the global generator
 * (duration_predictors.py:257-258, models.py:267), i.e. under the caller's torch.manual_seed. */
int32_t wetts_set_seed(const wetts_model_t* m, uint64_t seed);

/* total upsampling factor (prod upsample_rates, decoders.py:30-47; the iSTFT hop for Vocos, decoders.py:283) == the
 * `hop_length` of the checkpoint's config (examples/baker/configs/v1.json:23). */
int32_t wetts_hop_length(const wetts_model_t* m);

/* Copies the model's folded float32 weights (the blob wetts_create() was given, in
 * wetts_blob_tensor_info() order) into out_dev[numel], stream-ordered.  Backs the drop-in module's
 * state_dict() (the reference saves checkpoints from it, utils/task.py:59-76). */
int32_t wetts_get_blob(const wetts_model_t* m, float* out_dev, int64_t numel, void* stream);

/* Scratch needed by any of the stage calls below for a batch of B utterances, Tx phonemes
 * (padded) and Ty frames (padded).  Pass Ty = 0 for the pre-length-regulation stages only.
 * (The reference allocates every intermediate through PyTorch's caching allocator inside infer(), models.py:228-280;
 * here no stage call allocates.) */
int64_t wetts_workspace_bytes(const wetts_model_t* m, int32_t B, int32_t Tx, int32_t Ty);

/* ---- stage entry points (stream-ordered) -------------------------------------------------- */

/* a2 emb_g lookup (models.py:238-241).  g_out [B, gin].  sid may be NULL iff n_speakers==0
 * (g_out is then zero-filled and ignored downstream, matching g=None). */
int32_t wetts_speaker_embedding(const wetts_model_t* m, const int64_t* sid, int32_t B,
                                float* g_out, void* stream);

/* a3-a7 TextEncoder.forward (encoders.py:47-57; attentions.py:70-87,225-282,403-411;
 * normalization.py:16-19; commons.py:113-117).
 *   x [B,Tx] int64, x_lengths [B] int64
 *   x_enc [B,H,Tx], stats [B,2*inter,Tx] (m_p = channels [0,inter), logs_p = the rest),
 *   x_mask [B,Tx].  g [B,gin] (may be NULL) is only read by speaker-conditioned encoders
 *   (`enc_p(x, x_lengths, g=g)`, models.py:243). */
int32_t wetts_text_encoder(const wetts_model_t* m, const int64_t* x, const int64_t* x_lengths,
                           const float* g, int32_t B, int32_t Tx, float* x_enc, float* stats,
                           float* x_mask, void* workspace, int64_t workspace_bytes, void* stream);

/* a8 StochasticDurationPredictor.forward(reverse=True) (duration_predictors.py:213-219,254-263;
 * transforms.py:47-187).  eps_w [B,2,Tx] is the caller's standard-normal draw (the reference
 * calls torch.randn at :257); it is scaled by noise_scale_w inside.  logw [B,Tx].
 * status_dev (int32[1], may be NULL = the word registered with wetts_set_status_word) gets
 * WETTS_STATUS_SPLINE_DOMAIN OR-ed in on the device if the reference would have failed
 * `assert (discriminant >= 0)` (transforms.py:171); it is NOT cleared here. */
int32_t wetts_duration_sdp(const wetts_model_t* m, const float* x_enc, const float* x_mask,
                           const float* g, const float* eps_w, float noise_scale_w, int32_t B,
                           int32_t Tx, float* logw, int32_t* status_dev, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* a9 DurationPredictor.forward (duration_predictors.py:297-311). */
int32_t wetts_duration_dp(const wetts_model_t* m, const float* x_enc, const float* x_mask,
                          const float* g, int32_t B, int32_t Tx, float* logw, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* a10 durations -> lengths (models.py:254-256): w = exp(logw)*mask*length_scale,
 * w_ceil = ceil(w) [B,Tx], cum = inclusive cumsum(w_ceil) [B,Tx] (float, exact integers),
 * y_lengths = clamp_min(sum,1) [B] int64.  The caller reads y_lengths back (the one host sync
 * the reference also has: commons.py:114-115 `length.max()`).  status_dev (may be NULL) gets
 * WETTS_STATUS_DURATION_NONFINITE when a total is NaN / inf (y_lengths[b] is then 1). */
int32_t wetts_durations_to_lengths(const float* logw, const float* x_mask, float length_scale,
                                   int32_t B, int32_t Tx, float* w_ceil, float* cum,
                                   int64_t* y_lengths, int32_t* status_dev, void* stream);

/* a10-a12 sequence_mask + generate_path + prior expansion + sampling (models.py:257-267,
 * commons.py:113-136).  Ty = max(y_lengths) chosen by the caller.
 *   frame2phone [B,Ty] int32: the working form of the alignment (index of the phoneme each
 *   frame copies, -1 = none); y_mask [B,Ty]; attn [B,Ty,Tx] (may be NULL to skip materialising
 *   the dense 0/1 path of generate_path); m_p / logs_p come from `stats` [B,2*inter,Tx];
 *   outputs m_p_exp, logs_p_exp (both may be NULL), z_p [B,inter,Ty];
 *   eps_z[b,c,t] at eps_z + b*eps_batch_stride + c*eps_channel_stride + t is the caller's
 *   standard-normal draw (torch.randn_like at models.py:267). */
int32_t wetts_length_regulate(const wetts_model_t* m, const float* stats, const float* cum,
                              const float* x_mask, const int64_t* y_lengths, const float* eps_z,
                              int64_t eps_batch_stride, int64_t eps_channel_stride,
                              float noise_scale, int32_t B, int32_t Tx, int32_t Ty,
                              int32_t* frame2phone, float* y_mask, float* attn, float* m_p_exp,
                              float* logs_p_exp, float* z_p, void* stream);

/* a13 ResidualCouplingTransformersBlock.forward(reverse=True) (flows.py:442-449,494-513;
 * modules.py:60-106; commons.py:98-105).  z_p, z_out [B,inter,Ty]; z_out is NOT masked
 * (the reference returns z unmasked, models.py:280). */
int32_t wetts_flow_reverse(const wetts_model_t* m, const float* z_p, const float* y_mask,
                           const float* g, int32_t B, int32_t Ty, float* z_out, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* a14 Generator.forward (decoders.py:63-82,157-170,205-214).  z [B,inter,L] with arbitrary
 * batch stride `z_batch_stride` (floats) so a time-slice (z*y_mask)[:,:,:max_len] or a
 * streaming chunk (export_decoder_forward, models.py:360-363) needs no copy; y_mask may be
 * NULL (no masking) or [B, >=L] with row stride mask_stride.  audio [B, L*hop]. */
int32_t wetts_hifigan(const wetts_model_t* m, const float* z, int64_t z_batch_stride,
                      int64_t z_channel_stride, const float* y_mask, int64_t mask_stride,
                      const float* g, int32_t B, int32_t L, float* audio, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* Ragged form of wetts_hifigan.  The generator has no masks (decoders.py:63-82), so in a padded batch every
 * utterance is decoded to the batch's longest -- and the reference's own CLI avoids that by synthesising one
 * utterance per call (inference.py:83-110).  This entry gives a batch that call's arithmetic: utterance b is
 * decoded over its OWN y_lengths[b] frames (int64 device array, each <= L), exactly as
 * `dec(z[b:b+1, :, :y_lengths[b]], g[b:b+1])` would decode it alone -- zero padding at its own end, tiles behind
 * its end are not computed -- while z / audio keep their dense [B, ., L] / [B, L*hop] layout; samples of row b
 * behind y_lengths[b]*hop are written as 0.  float32 ResBlock1 HiFi-GAN models (wetts_hifigan_ragged_supported
 * returns 1); same workspace as wetts_hifigan. */
int32_t wetts_hifigan_ragged_supported(const wetts_model_t* m);
int32_t wetts_hifigan_ragged(const wetts_model_t* m, const float* z, int64_t z_batch_stride,
                             int64_t z_channel_stride, const int64_t* y_lengths, const float* g,
                             int32_t B, int32_t L, float* audio, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* Decoder arithmetic: 0 = float32 (default; exact-f32 MFMA, the parity-gated path),
 * 1 = bfloat16, 2 = IEEE half activations / weights with f32 accumulation (BASELINE.json
 * configs[2] / configs[4] precision; the text encoder, duration predictor and flow stay f32).  The 16-bit weight
 * copies are packed by this call (all or nothing: a failure leaves the model unpacked and is returned here).  At 16 bit every ResBlock1 (c1, c2) pair with <= 128 channels runs as ONE fused
 * kernel (intermediate kept in LDS); OR-ing WETTS_DECODER_UNFUSED into `precision` forces the
 * two-launch form, which is bit-identical (diagnostics / tests). */
/* 3 = uint8 dynamic quantisation: the decoder graph `export_onnx.py --quant` leaves behind
 * (wetts/vits/export_onnx.py:149-157, onnxruntime quantize_dynamic with QUInt8 weights): every Conv1d
 * becomes DynamicQuantizeLinear (per launch, per tensor) -> ConvInteger (int32 accumulate, here on
 * v_mfma_i32_32x32x32_i8) -> scale + bias; ConvTranspose1d and the element-wise ops stay float32.
 * onnxruntime is absent from the reference tree, so this variant's parity is unpinned (the oracle
 * restates the published operator definitions). */
#define WETTS_DECODER_UINT8_DYNAMIC 3
#define WETTS_DECODER_UNFUSED 0x10
/* f32 HiFi-GAN: by default the k = 3 / 7 / 11 ResBlock chains of a stage run on three HIP streams forked from / joined to the
 * call's stream (they are independent until the MRF sum; one chain's launch tails are filled by the others' work).
 * OR-ing WETTS_DECODER_SERIAL into `precision` keeps every launch on the call's stream, one after the other (the round-4
 * schedule with grouped launches): bit-identical, and the form in which a kernel trace's per-kernel durations do not
 * overlap (measurement). */
#define WETTS_DECODER_SERIAL 0x20
int32_t wetts_set_decoder_precision(const wetts_model_t* m, int32_t precision);

/* iSTFT head of a Vocos model (decoders.py:300-304).  The reference has TWO, selected by the module's `is_onnx` flag:
 *   WETTS_ISTFT_TORCH (0)  torchaudio InverseSpectrogram == torch.istft(hann, center=True): frames = irfft(S) * hann,
 *                          overlap-add, DIVIDED by the overlap-added hann^2 envelope, n_fft/2 trimmed per side
 *                          -- what SynthesizerTrn.infer() of a model built by inference.py computes;
 *   WETTS_ISTFT_ONNX  (1)  OnnxSTFT.inverse (utils/stft.py:325-340): conv_transpose1d with
 *                          pinv(scale * rDFT basis)^T * hann, scale = n_fft / hop (== irfft * hann / scale), overlap-add,
 *                          same trim, NO envelope division -- what every graph export_onnx.py writes computes
 *                          (export_onnx.py:59 sets hps.model.is_onnx = True), i.e. the arithmetic behind
 *                          inference_onnx.py, cli/model.py, runtime/core/model/vits_model.cc and the Triton repos.
 *                          At hop = n_fft / 4 the interior is 0.375 x the torch.istft audio; the first and last
 *                          n_fft/2 samples differ in shape as well.
 * The mode is the config's is_onnx at create; this call switches a live model (both bases are built at create; a host
 * flag read at launch time, so it applies to the calls issued after it).  HiFi-GAN models accept and ignore it. */
#define WETTS_ISTFT_TORCH 0
#define WETTS_ISTFT_ONNX 1
int32_t wetts_set_istft_mode(const wetts_model_t* m, int32_t mode);
int32_t wetts_get_istft_mode(const wetts_model_t* m);

/* One Conv1d ("same" padding) as a dynamically quantised ONNX graph computes it -- the building block
 * of WETTS_DECODER_UINT8_DYNAMIC, exposed for validation: DynamicQuantizeLinear over the whole x,
 * per-tensor uint8 weights, ConvInteger on the int8 matrix cores, dequantise + bias.  x [B,Cin,T],
 * w [Cout,Cin,k] (natural PyTorch layout), bias [Cout] or NULL, out [B,Cout,T]; all device pointers.
 * Unlike the stage calls it allocates (packed weights, scratch) and synchronises the stream. */
int32_t wetts_dynamic_quant_conv1d(const float* x, const float* w, const float* bias, int32_t B,
                                   int32_t Cin, int32_t Cout, int32_t k, int32_t dilation,
                                   int32_t padding, int32_t T, float* out, void* stream);

/* Arithmetic of the flow's WaveNet layers (modules.py:60-87: in_layers k = 5, the gate, res_skip 1x1,
 * the residual / skip update): 0 = float32 (default, the parity-gated path), 1 = bfloat16,
 * 2 = IEEE half activations / weights with f32 accumulation and an f32 skip sum; pre / post /
 * cond_layer convs, the coupling and everything else stay f32.  BASELINE.json configs[2] ("bf16")
 * precision for the part of the step that dominates at B = 64.  The 16-bit weight copies are packed by this call. */
int32_t wetts_set_flow_precision(const wetts_model_t* m, int32_t precision);

/* ---- voice conversion (SynthesizerTrn.voice_conversion, models.py:369-376) ------------------------------------ */

/* Set-up call (like the precision setters): copies the posterior blob (wetts_posterior_blob_tensor_info order, device
 * pointer, may be freed after the call) into the model, packs the posterior encoder's convs and natural-order copies of
 * the flow's `pre` convs for the forward direction, and returns after `stream` has drained.  A second call replaces
 * the first; the caller has synchronised the streams that used the model. */
int32_t wetts_load_posterior_encoder(wetts_model_t* m, int32_t spec_channels, const float* blob_dev, int64_t numel,
                                     void* stream);

/* Scratch of wetts_posterior_encoder and wetts_flow_forward for B utterances of Ty frames. */
int64_t wetts_posterior_workspace_bytes(const wetts_model_t* m, int32_t B, int32_t Ty);

/* PosteriorEncoder.forward (encoders.py:91-99), f32:
 *   y [B, spec_channels, Ty] linear spectrogram, y_lengths [B] int64, g [B, gin] (may be NULL = g=None),
 *   eps [B, inter, Ty] the caller's standard-normal draw (torch.randn_like, encoders.py:98);
 *   z [B, inter, Ty] = (m + eps * exp(logs)) * y_mask; m_q / logs_q [B, inter, Ty] may be NULL; y_mask [B, Ty]. */
int32_t wetts_posterior_encoder(const wetts_model_t* m, const float* y, const int64_t* y_lengths, const float* g,
                                const float* eps, int32_t B, int32_t Ty, float* z, float* m_q, float* logs_q,
                                float* y_mask, void* workspace, int64_t workspace_bytes, void* stream);

/* ResidualCouplingTransformersBlock.forward(reverse=False) (flows.py:442-446) for every flow type wetts_flow_reverse
 * supports; the log-determinant is not computed (voice_conversion discards it).  z, z_p [B, inter, Ty].  Honours
 * wetts_set_flow_precision.  Needs wetts_load_posterior_encoder first. */
int32_t wetts_flow_forward(const wetts_model_t* m, const float* z, const float* y_mask, const float* g, int32_t B,
                           int32_t Ty, float* z_p, void* workspace, int64_t workspace_bytes, void* stream);

/* a15 monotonic_align.maximum_path (utils/monotonic_align.py:6-57).  Needs no model.
 *   neg_cent [B,Ty,Tx] float32 (not modified), t_ys / t_xs int32[B] (the mask sums the
 *   reference derives at :16-17), path [B,Ty,Tx] int32 (zero-filled then the 1s written),
 *   workspace >= B*Ty*Tx*4 bytes (the in-place DP table the reference keeps in `values`). */
int32_t wetts_mas(const float* neg_cent, const int32_t* t_ys, const int32_t* t_xs, int32_t B,
                  int32_t Ty, int32_t Tx, int32_t* path, void* workspace, int64_t workspace_bytes,
                  void* stream);

/* ---- forced alignment (SynthesizerTrn.forward up to the prior expansion, models.py:171-212, no gradients) ---------- */

/* Alignment scores, models.py:173-184:
 *   neg_cent[b,t,s] = sum_c ( -1/2 log 2pi - logs_p[b,c,s] - 1/2 (z_p[b,c,t] - m_p[b,c,s])^2 exp(-2 logs_p[b,c,s]) )
 * as one f32-MFMA GEMM per utterance, [Ty x 2 inter] . [2 inter x Tx], whose operands are built in LDS from
 *   z_p [B, inter, Ty] (wetts_flow_forward) and stats [B, 2*inter, Tx] (m_p | logs_p, as wetts_text_encoder writes them);
 * neither operand nor any of the reference's four intermediates is stored.  neg_cent [B, Ty, Tx].  Cells of padded
 * frames / phonemes hold finite values of no meaning (wetts_mas never reads them as band cells).  inter is the model's. */
int32_t wetts_align_scores(const wetts_model_t* m, const float* z_p, const float* stats, int32_t B, int32_t Tx,
                           int32_t Ty, float* neg_cent, void* stream);

/* x_lengths, y_lengths [B] int64 -> t_xs, t_ys [B] int32 clamped to [0, Tx] / [0, Ty]: the per-utterance extents
 * wetts_mas and wetts_path_to_durations take (the mask sums of monotonic_align.py:16-17).  ORs
 * WETTS_STATUS_ALIGN_TEXT_LONGER into the registered status word when some utterance has more phonemes than frames. */
int32_t wetts_align_lengths(const wetts_model_t* m, const int64_t* x_lengths, const int64_t* y_lengths, int32_t B,
                            int32_t Tx, int32_t Ty, int32_t* t_xs, int32_t* t_ys, void* stream);

/* path -> durations (models.py:196 `w = attn.sum(2)`): path [B,Ty,Tx] int32 0/1 (wetts_mas), t_ys / t_xs int32 [B];
 *   w [B,Tx] float (exact integers), cum [B,Tx] its inclusive cumsum (what wetts_length_regulate reads),
 *   frame2phone [B,Ty] int32 the column of the first 1 of each row, -1 for a row without one (the form
 *   wetts_length_regulate writes), attn [B,Ty,Tx] float (may be NULL) the path as the reference returns it.
 * Tx <= 16384. */
int32_t wetts_path_to_durations(const int32_t* path, const int32_t* t_ys, const int32_t* t_xs, int32_t B, int32_t Tx,
                                int32_t Ty, float* w, float* cum, int32_t* frame2phone, float* attn, void* stream);

/* Given durations -> lengths: the three outputs of wetts_durations_to_lengths from integer frame counts [B,Tx] int64
 * (w_ceil = counts * x_mask, cum, y_lengths = clamp_min(sum, 1)), with no exp(log(d)) round trip.  A negative count
 * under the mask ORs WETTS_STATUS_DURATION_NEGATIVE into status_dev (may be NULL) and counts as 0. */
int32_t wetts_counts_to_lengths(const int64_t* counts, const float* x_mask, int32_t B, int32_t Tx, float* w_ceil,
                                float* cum, int64_t* y_lengths, int32_t* status_dev, void* stream);

/* ---- teacher-forced reconstruction (models.py:214-216 and the reconstruction losses of train.py:402-432,486-488) ---- */

/* Where the decoder slice of each utterance starts, commons.py:54-56:
 *   ids[b] = int64(u[b] * float(len[b] - segment + 1)), the float32 product truncated toward zero,
 * then clamped into [0, len[b] - segment]: a u of 1.0 (the reference's torch.rand is below 1, a caller's u need not be)
 * would give len - segment + 1 and slice one frame out of range.  u [B] float (wetts_rand, or the caller's); lengths [B] int64 (NULL = every row holds T),
 * clamped into [0, T].  With ids_in [B] int64 (then u may be NULL) the caller's ids are taken instead and checked.
 * A row with len[b] < segment, or a given id outside [0, len[b] - segment], ORs WETTS_STATUS_SEGMENT_LONGER into
 * status_dev (may be NULL); its id is 0 resp. the nearest valid one, so nothing downstream reads out of bounds. */
int32_t wetts_slice_ids(const float* u, const int64_t* ids_in, const int64_t* lengths, int32_t B, int32_t T,
                        int32_t segment, int64_t* ids, int32_t* status_dev, void* stream);

/* commons.slice_segments (commons.py:41-47) with a scale: out[b,c,j] = x[b,c, ids[b]*scale + j] for
 * j < segment*scale.  x [B,C,T] with batch / channel strides in floats (time stride 1), out [B,C,segment*scale]
 * contiguous.  scale = 1 slices z or a mel spectrogram at frame ids, scale = hop the waveform at the same ids
 * (train.py:430-431).  Any C >= 1 and any alignment of base, strides and start; segment*scale <= T.  A start outside
 * [0, T - segment*scale] is clamped into it (wetts_slice_ids has flagged it). */
int32_t wetts_slice_segments(const float* x, int64_t x_batch_stride, int64_t x_channel_stride, const int64_t* ids,
                             int32_t B, int32_t C, int32_t T, int32_t segment, int32_t scale, float* out,
                             void* stream);

/* losses.kl_loss (losses.py:45-60) without gradients: kl = logs_p - logs_q - 1/2 + 1/2 (z_p - m_p)^2 exp(-2 logs_p) on
 * [B,I,T] tensors, z_mask [B,T].  partials [2,B]: the masked sums and the frame counts sum_t z_mask per utterance;
 *   per_utt[b] = partials[0][b] / partials[1][b],   total[0] = sum_b partials[0][b] / sum_b partials[1][b],
 *   total[1] = weight * total[0]  (the loss as train.py:487 weighs it, `* hps.train.c_kl`)
 * -- the divisor counts frames, not frames x channels, as the reference's does.  Frames with z_mask == 0 are not read
 * into the sum.  No floating-point atomics: every sum is formed in a fixed order that depends on an utterance's own
 * frames only, so results repeat bit for bit and a row alone gives the per_utt it gives inside a padded batch. */
int32_t wetts_kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p,
                      const float* z_mask, int32_t B, int32_t I, int32_t T, float weight, float* partials,
                      float* per_utt, float* total, void* stream);

/* F.l1_loss with its default mean (train.py:486) of two contiguous [B,N] tensors: partials [B] = sum_i |a - b| per row,
 * per_utt[b] = partials[b] / N, total[0] = sum_b partials[b] / (B*N), total[1] = weight * total[0] (`* hps.train.c_mel`).
 * Summation order as wetts_kl_loss. */
int32_t wetts_l1_loss(const float* a, const float* b, int32_t B, int64_t N, float weight, float* partials,
                      float* per_utt, float* total, void* stream);

/* ---- duration loss (models.py:196-206: `l_length` and the logw / logw_ returned with it) ----------------------------- */

/* Set-up call (like wetts_load_posterior_encoder): copies the duration blob (wetts_duration_blob_tensor_info order,
 * device pointer, may be freed after the call) into the model, packs its convs and returns after `stream` has
 * drained.  A second call replaces the first.  SDP models only. */
int32_t wetts_load_duration_posterior(wetts_model_t* m, const float* blob_dev, int64_t numel, void* stream);

/* Scratch of wetts_duration_sdp_forward for B utterances of Tx phonemes. */
int64_t wetts_duration_loss_workspace_bytes(const wetts_model_t* m, int32_t B, int32_t Tx);

/* StochasticDurationPredictor.forward(x, x_mask, w, g, reverse=False) (duration_predictors.py:206-253; the spline's
 * forward branch, transforms.py:188-206), f32, no gradients:
 *   x_enc [B,H,Tx], x_mask [B,Tx], g [B,gin] (may be NULL), w [B,Tx] frame counts, e_q [B,2,Tx] the caller's
 *   standard-normal draw (torch.randn at :229; masked inside);
 *   nll[b], logq[b] as at :251-252 and :240-242, both[b] = nll[b] + logq[b] (what the module returns; may be NULL),
 *   per_utt[b] = both[b] / sum_t x_mask[b] (models.py:199 divides by the whole batch's mask sum instead:
 *   wetts_duration_loss_total).
 * Stage outputs, each may be NULL: z_q [B,2,Tx] (the posterior flows' output), z [B,2,Tx] (the main flows' output),
 * nll_terms / logq_terms [B,Tx]: per position, minus the log-determinants nll resp. logq subtract (the splines, the Log
 * flow, the two logsigmoids), without the Gaussian terms and ElementwiseAffine's constant -- the accumulators the
 * reduction reads.  Nothing behind an utterance's length is read from w or e_q; every output is zero there.
 * A masked-in w that is negative / not finite ORs WETTS_STATUS_DURATION_NEGATIVE / _NONFINITE into status_dev (may be
 * NULL = the registered word).  No floating-point atomics: results repeat bit for bit, and the reduction of a row
 * depends on that row alone (order as wetts_kl_loss).  A row with no phoneme under the mask has nll = logq = 0 and
 * per_utt = NaN (0 / 0), and wetts_duration_loss_total of an all-empty batch divides by zero likewise, as the reference's
 * `/ torch.sum(x_mask)` does; SynthesizerTrn.duration_loss refuses an empty batch.  Needs
 * wetts_load_duration_posterior first. */
int32_t wetts_duration_sdp_forward(const wetts_model_t* m, const float* x_enc, const float* x_mask, const float* g,
                                   const float* w, const float* e_q, int32_t B, int32_t Tx, float* nll, float* logq,
                                   float* both, float* per_utt, float* z_q, float* z, float* nll_terms, float* logq_terms,
                                   int32_t* status_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* The reduction at the end of wetts_duration_sdp_forward on given stage tensors (z, e_q [B,2,Tx], the two term
 * tensors [B,Tx]): nll, logq, both = nll + logq, per_utt [B]. */
int32_t wetts_duration_reduce(const wetts_model_t* m, const float* nll_terms, const float* logq_terms, const float* z,
                              const float* e_q, const float* x_mask, int32_t B, int32_t Tx, float* nll, float* logq,
                              float* both, float* per_utt, void* stream);

/* DurationPredictor models (models.py:201-206): logw_target = log(w + 1e-6) * x_mask [B,Tx], rows[b] = sum_t (logw -
 * logw_target)^2, per_utt[b] = rows[b] / sum_t x_mask[b].  Status bits as above, into the registered word. */
int32_t wetts_duration_dp_loss(const wetts_model_t* m, const float* logw, const float* w, const float* x_mask,
                               int32_t B, int32_t Tx, float* logw_target, float* rows, float* per_utt, void* stream);

/* logw_target = log(w + 1e-6) * x_mask [B,Tx] alone (models.py:201, SDP models); nothing behind a length is read. */
int32_t wetts_duration_logw_target(const float* w, const float* x_mask, int32_t B, int32_t Tx, float* logw_target,
                                   void* stream);

/* Validation aids: the elementwise steps of wetts_duration_sdp_forward on given device tensors, no model needed.
 *   affine_forward: ElementwiseAffine forward, out [B,2,Tx] = (m + exp(logs) * (x * mask)) * mask; m, logs [2].
 *   spline_forward: one ConvFlow's spline on z [B,2,Tx] in place (channel ch0 *= mask, channel 1 - ch0 transformed) with
 *     h [B,29,Tx] the flow's projection, div = sqrt(filter_channels); acc [B,Tx] += sign * logabsdet * mask.
 *   dequant_log: z_q [B,2,Tx] (z_u at channel chu), w [B,Tx] -> z [B,2,Tx], nll_terms / logq_terms [B,Tx] accumulated.
 *   pre: post_pre, out [B,C,Tx] = weight[c] * (w under the mask) + bias[c].
 * Every one is a function of its own (b, t) alone: a row gives the same bits alone and inside a batch. */
int32_t wetts_duration_affine_forward(const float* x, const float* m, const float* logs, const float* x_mask, int32_t B,
                                      int32_t Tx, float* out, void* stream);
int32_t wetts_duration_spline_forward(float* z, int32_t ch0, const float* h, const float* x_mask, float div, int32_t B,
                                      int32_t Tx, float sign, float* acc, void* stream);
int32_t wetts_duration_dequant_log(const float* z_q, int32_t chu, const float* w, const float* x_mask, int32_t B,
                                   int32_t Tx, float* z, float* nll_terms, float* logq_terms, int32_t* status_dev,
                                   void* stream);
int32_t wetts_duration_pre(const float* w, const float* x_mask, const float* weight, const float* bias, int32_t B,
                           int32_t C, int32_t Tx, float* out, void* stream);

/* models.py:199 / :206 and train.py:485: l_length[b] = per_row[b] / sum(x_mask) with the sum over the WHOLE batch,
 * total[0] = sum_b l_length[b] (`loss_dur = torch.sum(l_length.float())`), total[1] = weight * total[0].  One wave, fixed
 * order.  per_row: nll + logq per utterance (SDP) or wetts_duration_dp_loss's rows. */
int32_t wetts_duration_loss_total(const float* per_row, const float* x_mask, int32_t B, int32_t Tx, float weight,
                                  float* l_length, float* total, void* stream);

/* a16 inference.py:100-110 output scaling: per utterance peak-normalise to 0.6 full scale,
 * clip, convert to int16.  lengths_samples [B] int64 = valid samples per row (peak is taken
 * over the valid part only when non-NULL, else over all L samples). */
int32_t wetts_audio_to_int16(const float* audio, const int64_t* lengths_samples, int32_t B,
                             int64_t L, int16_t* pcm, void* stream);

/* Standard-normal draws on the device (Philox4x32-10 + Box-Muller): what the reference gets from
 * torch.randn (duration_predictors.py:257) / torch.randn_like (models.py:267).  Element i is a
 * function of (seed, offset, i) only; a draw of n values consumes ceil(n/4) counter steps. */
int32_t wetts_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* Its uniform counterpart, torch.rand (commons.py:54): floats in [0, 1) from the low 24 bits of each Philox word times
 * 2^-24 (ATen's mapping for float).  Same (seed, offset) convention, ceil(n/4) counter steps. */
int32_t wetts_rand(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* ---- spectrograms (utils/mel_processing.py, inference side).  Need no model. ------------------------------------- */

/* The window-folded DFT basis of wetts_spectrogram for (n_fft, win): a periodic Hann window of `win` samples centred
 * in the n_fft frame (torch.stft), built in double on the device and rounded to float once.  numel() gives its size
 * in floats (-1 for invalid arguments); the caller allocates, builds once and keeps it.  Valid: even n_fft >= 4,
 * 1 <= win <= n_fft. */
int64_t wetts_stft_basis_numel(int32_t n_fft, int32_t win);
int32_t wetts_stft_basis(int32_t n_fft, int32_t win, float* basis, int64_t numel, void* stream);

/* spectrogram_torch (mel_processing.py:43-94), f32: audio [B, L] (row stride L), lengths [B] int64 valid samples per
 * row (NULL = every row holds L), basis from wetts_stft_basis(n_fft, win).  Each utterance is reflect-padded by
 * int((n_fft - hop) / 2) at ITS own length, then (center != 0) by n_fft / 2 again, as torch.stft does; spec
 * [B, n_fft / 2 + 1, T] = sqrt(re^2 + im^2 + 1e-6), frames at or past an utterance's own frame count written as zeros
 * (and all of them for an utterance too short for the reflect padding, where the reference raises: the caller checks).
 * Samples past lengths[b] are never read.  Valid: even n_fft >= 4, 1 <= hop <= n_fft, 1 <= win <= n_fft. */
int32_t wetts_spectrogram(const float* audio, const int64_t* lengths, int32_t B, int64_t L, int32_t n_fft,
                          int32_t hop, int32_t win, int32_t center, const float* basis, int32_t T, float* spec,
                          void* stream);

/* spec_to_mel_torch (mel_processing.py:97-111): mel [B, n_mels, T] = log(max(mel_basis @ spec, 1e-5)), spec
 * [B, n_bins, T], mel_basis [n_mels, n_bins] (librosa.filters.mel; the caller builds it).  frame_lengths [B] int64 may
 * be NULL; frames at or past it are written as zeros (a zero-padded batch). */
int32_t wetts_spec_to_mel(const float* spec, const float* mel_basis, const int64_t* frame_lengths, int32_t B,
                          int32_t n_bins, int32_t n_mels, int32_t T, float* mel, void* stream);

/* out[b,c,t] = x[b,c,t] * mask[b,t]  (`z * y_mask`, models.py:322). */
int32_t wetts_mask_rows(const float* x, const float* mask, int32_t B, int32_t C, int32_t T,
                        float* out, void* stream);

/* a1 SynthesizerTrn.infer (models.py:228-280) composed for native hosts (the shape of
 * runtime/core/model/vits_model.h:37 Forward()).  Synchronises the stream once internally to
 * read y_lengths.  The caller provides capacity for max_frames frames; on return
 * *frames_out = max(y_lengths) (<= max_frames, else WETTS_E_WORKSPACE), y_lengths_host[B].
 * eps_w [B,2,Tx] and eps_z [B,inter,max_frames] (row stride max_frames) are standard-normal
 * draws; either may be NULL, in which case it is drawn here from the model's Philox stream
 * (wetts_set_seed) -- eps_w as [B,2,Tx] before the duration predictor, eps_z as a packed [B,inter,*frames_out]
 * tensor once the frame count is known, the two draws the Python and C++ hosts make: a seed gives the same
 * audio whatever `max_frames` the caller passed.  Errors the reference raises from inside its modules come back as return codes
 * after that one synchronisation: WETTS_E_DOMAIN (spline discriminant, transforms.py:171; non-finite
 * durations) and WETTS_E_INVALID (phoneme / speaker id outside its table).  audio needs capacity
 * B*max_frames*hop floats and is written PACKED as [B, (*frames_out)*hop].  workspace >= wetts_infer_workspace_bytes(). */
int64_t wetts_infer_workspace_bytes(const wetts_model_t* m, int32_t B, int32_t Tx,
                                    int32_t max_frames);
int32_t wetts_infer(const wetts_model_t* m, const int64_t* x, const int64_t* x_lengths,
                    const int64_t* sid, const float* eps_w, const float* eps_z,
                    float noise_scale, float length_scale, float noise_scale_w, int32_t B,
                    int32_t Tx, int32_t max_frames, float* audio, int64_t* y_lengths_host,
                    int32_t* frames_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- measurement helpers ------------------------------------------------------------------ */

/* Algorithmic FLOPs / bytes of wetts_hifigan for one frame (SURVEY.md §8d formulas), so
 * bench.py prices the roofline from the same shapes the kernels run. */
int32_t wetts_hifigan_cost(const wetts_config_t* cfg, double* flops_per_frame,
                           double* bytes_per_frame_perconv, double* mrf_flops_per_frame,
                           double* mrf_bytes_per_frame_perconv);

/* Live timing of the dominant kernel class (every ResBlock conv of the MRF stack) inside
 * normal wetts_hifigan / wetts_infer calls: when enabled, a HIP event pair is recorded on the
 * call's stream around each stage's ResBlock launches (no synchronisation at record time).
 * wetts_read_mrf_timing synchronises the recorded events and returns the summed device time,
 * the number of MRF conv launches and of hifigan calls since enabling; set(…,0/1) resets. */
int32_t wetts_set_mrf_timing(const wetts_model_t* m, int32_t enable);
int32_t wetts_read_mrf_timing(const wetts_model_t* m, double* mrf_ms, int64_t* conv_launches,
                              int32_t* hifigan_calls);
/* Algorithmic HBM bytes of the same launches AT THE GRANULARITY THEY WERE LAUNCHED WITH, summed since enabling: per
 * launch every [B][C][T] plane it has to read or write once (a fused ResBlock / stage: x in, running sum in and out; a
 * single conv: input, residual, output).  SURVEY.md 8(d)'s per-conv figure (wetts_hifigan_cost) counts planes a fused
 * launch never moves through HBM, so a bandwidth fraction priced with it can exceed 1; this one cannot. */
int32_t wetts_read_mrf_bytes(const wetts_model_t* m, double* launched_bytes);

/* Times `iters` launches of the dominant MRF conv kernel class (all ResBlock convs of the
 * decoder) with HIP events on `stream`; returns total ms and the number of conv launches.
 * Used by bench.py for roofline.achieved. */
int32_t wetts_profile_hifigan(const wetts_model_t* m, const float* z, int64_t z_batch_stride,
                              int64_t z_channel_stride, const float* g, int32_t B, int32_t L,
                              float* audio, void* workspace, int64_t workspace_bytes, void* stream,
                              double* mrf_ms, double* total_ms, int32_t* mrf_launches);

/* ---- MultiPeriodDiscriminator and the adversarial losses (csrc/discriminator.hip) ------------------------------
 *
 * model/discriminators.py:21-124,228-254 with use_spectral_norm = false, without gradients: DiscriminatorS and
 * DiscriminatorP for the periods 2, 3, 5, 7, 11, and losses.py:6-42.  The architecture has no configuration, so the
 * blob layout is fixed: the 74 tensors `discriminators.N.convs.M.{weight,bias}` / `discriminators.N.conv_post.*` with
 * weight norm folded, Conv2d weights in their [Cout, Cin, k, 1] shape.  A handle of its own: wetts_model_t and its
 * three blobs know nothing of it. */
typedef struct wetts_disc wetts_disc_t;

int32_t wetts_disc_blob_num_tensors(void);
int32_t wetts_disc_blob_tensor_info(int32_t index, char* name_buf, size_t name_buf_len, int64_t* offset,
                                    int64_t* numel, int64_t shape[4]);
int64_t wetts_disc_blob_numel(void);
/* Copies the device blob (a set-up call like the model's create: allocates, returns after `stream` has drained). */
int32_t wetts_disc_create(const float* blob_dev, int64_t blob_numel, void* stream, wetts_disc_t** out);
void wetts_disc_destroy(wetts_disc_t* d);

/* Internal shape {rows, C, H, p} of feature map `index` (0..6: DiscriminatorS's seven layers, then six per period) for
 * B utterance PAIRS of T samples: rows = 2B * p.  A period stack's map is the contiguous [2B][p][C][H], whose
 * permutation (0, 2, 3, 1) is the reference's [2B, C, H, p]; its conv_post map is stored as the
 * reference has it, [2B][1][H][p]; DiscriminatorS's maps (p = 1) are the reference's [2B][C][T'].  The first B
 * utterances are the real ones. */
int32_t wetts_disc_fmap_shape(int32_t B, int32_t T, int32_t index, int64_t shape[4]);

/* All six stacks on y and y_hat [B, 1, T] as one batch of 2B.  fmaps_host: 37 device buffers of the shapes above, owned
 * by the caller; every layer's output is one of them, so the call needs no workspace.  T >= 6, the shortest length at
 * which every reflect pad of discriminators.py:81-84 is legal (n_pad < T for each period). */
int32_t wetts_disc_forward(const wetts_disc_t* d, const float* y, const float* y_hat, int32_t B, int32_t T,
                           float* const* fmaps_host, void* stream);

/* One layer of one stack on `rows` independent rows, with the kernels and weights the forward pass uses: the reflect
 * pad + fold + conv 0 of period stack `disc` (1..5) on rows utterances [rows, T] -> [rows * p][32][H1]; an MFMA conv
 * (layers 1..4 of a period stack, layer 5 of DiscriminatorS) on x [rows][Cin][Hin]; conv_post on `rows` utterances
 * ([rows * p][1024][H] in); a grouped conv of DiscriminatorS (layers 0..4) on x [rows][Cin][Tin]. */
int32_t wetts_disc_fold_conv0(const wetts_disc_t* d, int32_t disc, const float* y, int32_t rows, int32_t T, float* out,
                              void* stream);
int32_t wetts_disc_strided_conv(const wetts_disc_t* d, int32_t disc, int32_t layer, const float* x, int64_t rows,
                                int32_t Hin, float* out, void* stream);
int32_t wetts_disc_conv_post(const wetts_disc_t* d, int32_t disc, const float* x, int32_t rows, int32_t H, float* out,
                             void* stream);
int32_t wetts_disc_grouped_conv(const wetts_disc_t* d, int32_t layer, const float* x, int32_t rows, int32_t Tin,
                                float* out, void* stream);

/* losses.py:6-42 over n (real, generated) tensor pairs; utterance b of pair i owns the N_host[i] contiguous floats at
 * a_host[i] + b * a_bs_host[i] (g likewise).  kind 0, feature_loss: item_a[i] = mean |a - g|, scale 2.  kind 1,
 * discriminator_loss: item_a[i] = mean (1 - a)^2, item_g[i] = mean g^2.  kind 2, generator_loss: item_a[i] =
 * mean (1 - a)^2 (g unused).  total[0] = scale * the sum over items, per_utt[b] the same from utterance b's own
 * elements; sums: 2 * n * B float64 of scratch (the sums are carried in float64, in a fixed order, and round to f32 at
 * the store).  No atomics: results repeat bit for bit and
 * per_utt[b] does not depend on the batch. */
int32_t wetts_disc_losses(int32_t kind, int32_t n, const float* const* a_host, const float* const* g_host,
                          const int64_t* a_bs_host, const int64_t* g_bs_host, const int64_t* N_host, int32_t B,
                          float scale, double* sums, float* item_a, float* item_g, float* per_utt, float* total,
                          void* stream);
/* n may be 1 .. WETTS_DISC_LOSSES_MAX_ITEMS: the row sums go out in groups of at most 40 items (an item's sums do not
 * depend on its group), the totals launch reads the whole table. */
#define WETTS_DISC_LOSSES_MAX_ITEMS 128

/* ---- MultiPeriodMultiResolutionDiscriminator (csrc/mrd.hip) -------------------------------------------------------
 *
 * model/discriminators.py:127-225,256-283 without gradients: three DiscriminatorR stacks (window lengths 2048, 1024,
 * 512; hop = window / 4; no embedding) followed by the five DiscriminatorP stacks; there is no DiscriminatorS.  The
 * blob layout is fixed: `discriminators.{0,1,2}.band_convs.{b}.{l}.{weight,bias}` (b, l = 0..4, Conv2d weights
 * [Cout, Cin, 3, kf]) and `discriminators.{0,1,2}.conv_post.*`, then `discriminators.{3..7}.convs.M.*` /
 * `.conv_post.*` as in the period stacks of wetts_disc_t; weight norm folded.  216 tensors.  A handle of its own; create
 * also builds the three window-folded DFT bases and packs the band convs' weights for the matrix cores. */
typedef struct wetts_mrd wetts_mrd_t;
#define WETTS_MRD_NUM_FMAPS 93
#define WETTS_MRD_MIN_SAMPLES 1025 /* the centring reflect pad of the 2048 window needs T > 1024 */

int32_t wetts_mrd_blob_num_tensors(void);
int32_t wetts_mrd_blob_tensor_info(int32_t index, char* name_buf, size_t name_buf_len, int64_t* offset,
                                   int64_t* numel, int64_t shape[4]);
int64_t wetts_mrd_blob_numel(void);
int32_t wetts_mrd_create(const float* blob_dev, int64_t blob_numel, void* stream, wetts_mrd_t** out);
void wetts_mrd_destroy(wetts_mrd_t* d);

/* Shape of feature map `index` (0..92) for B utterance PAIRS of T samples.  Resolution r (0..2) owns the maps
 * 21 r .. 21 r + 20: band b's layers 1..4 at 21 r + 4 b + (layer - 1), each the reference's contiguous
 * [2B][32][frames][F'], and conv_post at 21 r + 20, [2B][1][frames][sum F'].  The period stacks follow at 63 + 6 d + m
 * in the internal shape {rows = 2B * p, C, H, p} of wetts_disc_fmap_shape.  frames = 1 + T / hop. */
int32_t wetts_mrd_fmap_shape(int32_t B, int32_t T, int32_t index, int64_t shape[4]);
/* Bytes of caller-provided scratch for wetts_mrd_forward: the normalised audio, one resolution's complex spectrogram
 * and its layer-0 band outputs (none of them a returned map).  Negative on a bad argument. */
int64_t wetts_mrd_workspace_bytes(int32_t B, int32_t T);
/* All eight stacks on y and y_hat [B, 1, T] as one batch of 2B (real first).  fmaps_host: 93 device buffers of the
 * shapes above, owned by the caller.  Allocates nothing.  T >= WETTS_MRD_MIN_SAMPLES. */
int32_t wetts_mrd_forward(const wetts_mrd_t* d, const float* y, const float* y_hat, int32_t B, int32_t T,
                          float* const* fmaps_host, void* workspace, int64_t workspace_bytes, void* stream);

/* The stages of one DiscriminatorR on `rows` independent utterances, with the kernels and weights the forward pass
 * uses.  normalize: y [rows][T] -> (0.8 (y - mean)) / (max |y - mean| + 1e-9), [rows][T].  spectrogram: the normalised
 * audio -> the complex STFT of resolution `res` in the INTERNAL layout [rows][2][bins][frames] (re plane, im plane;
 * frames fastest), bins = window / 2 + 1.  band_conv: layer 0..4 of all five bands in one launch; x holds the five
 * bands' inputs one after another, each [rows][Cin][frames][Fin_b] (layer 0: x is the spectrogram itself), out the five
 * outputs one after another, each [rows][32][frames][Fout_b].  conv_post: x as band_conv's layer-4 output,
 * out [rows][1][frames][sum Fout_b]. */
int32_t wetts_mrd_normalize(const float* y, int32_t rows, int32_t T, float* out, void* stream);
int32_t wetts_mrd_spectrogram(const wetts_mrd_t* d, int32_t res, const float* x, int32_t rows, int32_t T, float* spec,
                              void* stream);
int32_t wetts_mrd_band_conv(const wetts_mrd_t* d, int32_t res, int32_t layer, const float* x, int32_t rows,
                            int32_t frames, float* out, void* stream);
int32_t wetts_mrd_conv_post(const wetts_mrd_t* d, int32_t res, const float* x, int32_t rows, int32_t frames,
                            float* out, void* stream);
/* Width of band `band` (0..4) of resolution `res` after `layer` convs (layer 0 = the band's bins, 5 = what conv_post
 * reads): the reference's int(f * bins) edges and its conv arithmetic.  Negative on a bad argument. */
int32_t wetts_mrd_band_width(int32_t res, int32_t band, int32_t layer);

/* ---- VITS2 duration discriminators (csrc/duration_disc.hip) -------------------------------------------------------
 *
 * model/discriminators.py:287-449 without gradients.  version 1 = DurationDiscriminatorV1 (convs with bias only),
 * 2 = DurationDiscriminatorV2 (ReLU and a channel LayerNorm behind every conv).  The blob holds, in this order,
 * conv_1.{weight,bias} [norm_1.{gamma,beta}] conv_2.* [norm_2.*] dur_proj.* pre_out_conv_1.* [pre_out_norm_1.*]
 * pre_out_conv_2.* [pre_out_norm_2.*] output_layer.0.{weight,bias}; the bracketed tensors in version 2 only (version 1
 * constructs pre_out_norm_* and never reads them).  in_channels and filter_channels: multiples of 32 up to 256;
 * kernel_size odd, up to 7; anything else is refused.  A handle of its own. */
typedef struct wetts_durdisc wetts_durdisc_t;

int32_t wetts_durdisc_blob_num_tensors(int32_t version, int32_t in_channels, int32_t filter_channels,
                                       int32_t kernel_size);
int32_t wetts_durdisc_blob_tensor_info(int32_t version, int32_t in_channels, int32_t filter_channels,
                                       int32_t kernel_size, int32_t index, char* name_buf, size_t name_buf_len,
                                       int64_t* offset, int64_t* numel, int64_t shape[4]);
int64_t wetts_durdisc_blob_numel(int32_t version, int32_t in_channels, int32_t filter_channels, int32_t kernel_size);
int32_t wetts_durdisc_create(int32_t version, int32_t in_channels, int32_t filter_channels, int32_t kernel_size,
                             const float* blob_dev, int64_t blob_numel, void* stream, wetts_durdisc_t** out);
void wetts_durdisc_destroy(wetts_durdisc_t* d);

/* The workspace of wetts_durdisc_forward holds every stage, one after another, each rounded up to 64 floats:
 * conv_1's map [B][F][Tx], conv_2's [B][F][Tx], pre_out_conv_1's [2B][F][Tx], pre_out_conv_2's [2B][F][Tx] (each after
 * its ReLU + LayerNorm in version 2, before the next mask) and the probabilities [2B][Tx].  Rows 0..B-1 of the last
 * three belong to dur_r, rows B..2B-1 to dur_hat.  Negative on a bad argument. */
int64_t wetts_durdisc_workspace_bytes(const wetts_durdisc_t* d, int32_t B, int32_t Tx);
/* x [B][in_channels][Tx] (not pre-masked), x_mask [B][Tx], dur_r and dur_hat [B][Tx].  Four launches; allocates
 * nothing. */
int32_t wetts_durdisc_forward(const wetts_durdisc_t* d, const float* x, const float* x_mask, const float* dur_r,
                              const float* dur_hat, int32_t B, int32_t Tx, void* workspace, int64_t workspace_bytes,
                              void* stream);
/* One layer with the kernel and weights the forward pass uses, on `rows` output rows.  layer 0 conv_1, 1 conv_2,
 * 3 pre_out_conv_2: x [rows][C][Tx].  layer 2, pre_out_conv_1: x [src_rows][F][Tx] and dur [rows][Tx].  The row map:
 * output row r reads mask row r mod src_rows (x_mask [src_rows][Tx]) and, in layer 2, x row r mod src_rows.
 * out [rows][F][Tx]; prob [rows][Tx] is written by layer 3 only. */
int32_t wetts_durdisc_layer(const wetts_durdisc_t* d, int32_t layer, const float* x, const float* x_mask,
                            const float* dur, int32_t rows, int32_t src_rows, int32_t Tx, float* out, float* prob,
                            void* stream);
/* Row means of the probabilities prob_r, prob_g [B][Tx] in the reduction order of wetts_disc_losses (float64 sums, no
 * atomics).  Over all Tx positions of row b, as losses.py's means count them: r_rows = mean (1 - r)^2, g_rows = mean
 * g^2, gen_rows = mean (1 - g)^2.  Over the row's own positions (x_mask != 0): disc_per_utt = mean ((1 - r)^2 + g^2),
 * gen_per_utt = mean (1 - g)^2; NaN for a row without any. */
int32_t wetts_durdisc_row_means(const float* prob_r, const float* prob_g, const float* x_mask, int32_t B, int32_t Tx,
                                float* r_rows, float* g_rows, float* gen_rows, float* disc_per_utt,
                                float* gen_per_utt, void* stream);

/* ---- the text frontend (frontend/model.py:21-73; csrc/frontend.hip) ------------------------------------------------
 * An HF BertModel (absolute positions, last_hidden_state only), one nn.TransformerEncoderLayer(batch_first) at its
 * defaults (post-norm, ReLU, eps 1e-5, packed in_proj) and the two Linear classifiers, without gradients, f32
 * throughout.  A blob and a handle of its own.  The blob holds the reference's state_dict tensors under their own keys
 * (bert.embeddings.*, bert.encoder.layer.N.*, transform.*, phone_classifier.*, prosody_classifier.*) in natural layout,
 * each at a multiple of 4 floats; bert.pooler.* and position_ids are not part of it.
 * Limits: hidden_size a multiple of 8 up to 1024; heads of at most 96 channels (BERT's and transform's);
 * intermediate_size and transform_ff multiples of 8; T <= min(max_position_embeddings, 512).
 * Activations are token-major: [B * T][channels]. */
typedef struct wetts_frontend_config {
  int32_t vocab_size, hidden_size, num_layers, num_heads, intermediate_size, max_position_embeddings, type_vocab_size;
  float layer_norm_eps;                  /* BERT's LayerNorms (1e-12) */
  int32_t transform_heads, transform_ff; /* the TransformerEncoderLayer: 8 / 2048 at 768, 12 / 1200 at 312 */
  int32_t num_polyphones, num_prosody;
} wetts_frontend_config_t;
typedef struct wetts_frontend wetts_frontend_t;

#define WETTS_FRONTEND_EPI_BIAS 0     /* x W^T + b */
#define WETTS_FRONTEND_EPI_GELU 1     /* gelu(x W^T + b), the exact erf form */
#define WETTS_FRONTEND_EPI_RELU 2     /* relu(x W^T + b) */
#define WETTS_FRONTEND_EPI_RESIDUAL 3 /* x W^T + b + residual */

int32_t wetts_frontend_blob_num_tensors(const wetts_frontend_config_t* cfg);
int32_t wetts_frontend_blob_tensor_info(const wetts_frontend_config_t* cfg, int32_t index, char* name_buf,
                                        size_t name_buf_len, int64_t* offset, int64_t* numel, int64_t shape[4]);
int64_t wetts_frontend_blob_numel(const wetts_frontend_config_t* cfg);
int32_t wetts_frontend_create(const wetts_frontend_config_t* cfg, const float* blob_dev, int64_t blob_numel, void* stream,
                              wetts_frontend_t** out);
void wetts_frontend_destroy(wetts_frontend_t* f);
/* Bytes of scratch wetts_frontend_forward / _layer need for B rows of T tokens; negative on a bad argument. */
int64_t wetts_frontend_workspace_bytes(const wetts_frontend_t* f, int32_t B, int32_t T);
/* input_ids [B][T]; token_type_ids [B][T] or NULL (zeros); attention_mask [B][T] or NULL (ones): a key with mask 0 is
 * excluded from every attention.  phone_out [B][T][num_polyphones] and prosody_out [B][T][num_prosody]: the logits, or
 * with softmax != 0 the probabilities over the last dimension; ZEROS at a token whose mask is 0.  A token or type id
 * outside its table ORs WETTS_STATUS_TOKEN_ID_RANGE / _TYPE_ID_RANGE into *status (device int32, may be NULL) and
 * reads row 0.  T > max_position_embeddings, B < 1 and T < 1 are refused before any launch.  Allocates nothing. */
int32_t wetts_frontend_forward(const wetts_frontend_t* f, const int64_t* input_ids, const int64_t* token_type_ids,
                               const int64_t* attention_mask, int32_t B, int32_t T, int32_t softmax, float* phone_out,
                               float* prosody_out, void* workspace, int32_t* status, void* stream);
/* The stages, each with the kernel the forward pass uses.
 * _embed: word + position + type, LayerNorm -> out [B * T][hidden]; mask_out [B * T] is the mask as 1.0 / 0.0.
 * _linear: out [N][M] = x [N][K] weight[M][K]^T + bias, then WETTS_FRONTEND_EPI_*; K % 8 == 0, M % 4 == 0.
 * _add_layer_norm: out = LayerNorm(x + residual) over C (residual may be NULL; out may be x).
 * _attention: qkv [B * T][3 * heads * dk] (q | k | v) -> out [B * T][heads * dk], scores / sqrt(dk), keys with
 *   key_mask [B * T] == 0 excluded; a row without any valid key gives zeros.
 * _heads: x [N][hidden] -> both classifiers (and both softmaxes) in one launch; zeros where key_mask is 0.
 * _layer: layer `layer` (0 .. num_layers - 1 the BERT layers, num_layers = transform) in place on x [B * T][hidden]. */
int32_t wetts_frontend_embed(const wetts_frontend_t* f, const int64_t* input_ids, const int64_t* token_type_ids,
                             const int64_t* attention_mask, int32_t B, int32_t T, float* out, float* mask_out,
                             int32_t* status, void* stream);
int32_t wetts_frontend_linear(const float* x, const float* weight, const float* bias, const float* residual, int32_t N,
                              int32_t K, int32_t M, int32_t epilogue, float* out, void* stream);
int32_t wetts_frontend_add_layer_norm(const float* x, const float* residual, const float* gamma, const float* beta,
                                      float eps, int32_t N, int32_t C, float* out, void* stream);
int32_t wetts_frontend_attention(const float* qkv, const float* key_mask, int32_t B, int32_t T, int32_t heads, int32_t dk,
                                 float* out, void* stream);
int32_t wetts_frontend_heads(const wetts_frontend_t* f, const float* x, const float* key_mask, int32_t N, int32_t softmax,
                             float* phone_out, float* prosody_out, void* stream);
int32_t wetts_frontend_layer(const wetts_frontend_t* f, int32_t layer, float* x, const float* key_mask, int32_t B,
                             int32_t T, void* workspace, void* stream);
/* The decisions of cli/frontend.py:70-81 per token: choice[n] = the index i of the FIRST candidate class
 * cand[n][i], i < cand_len[n] <= max_cand, with the largest phone probability (0 without candidates); prosody[n] = the
 * LOWEST class with the largest prosody probability. */
int32_t wetts_frontend_decide(const float* phone_prob, const float* prosody_prob, const int32_t* cand,
                              const int32_t* cand_len, int32_t N, int32_t P, int32_t R, int32_t max_cand, int32_t* choice,
                              int32_t* prosody, void* stream);

/* ---- the 16-bit mode of the text frontend (csrc/frontend16.hip) ------------------------------------------------------
 * precision: 0 = f32 (the default), 1 = bf16, 2 = f16, as wetts_set_decoder_precision counts them.  With 1 or 2 set on a
 * handle, every Linear of the BERT layers and of `transform` (packed q|k|v, attention output, feed-forward in and out)
 * reads BOTH operands rounded to the type (round to nearest even; an f16 operand out of range is +-inf), with exact
 * products and f32 accumulation on the 16-bit MFMA; bias, GELU, ReLU and the residual stay f32 epilogues, and
 * everything else -- embeddings, LayerNorms, attention, both classifiers, the softmaxes, the decisions, scoring -- is
 * the f32 code unchanged.  _forward, _layer, _score and the workspace queries follow the handle's current mode.  The
 * same call gives the same bits, and a valid token's bits depend neither on the padding nor on the order of the rows;
 * but the kernel form is chosen by the token count, so a row alone and the same row in a batch need not agree to the
 * last bit (they do at f32).
 * _set_precision is a set-up call: it validates first, then packs the 16-bit copies of the weights on the device (it
 * allocates and drains the device), and changes the handle only after every check has passed; 0 frees the copies.  The
 * blob stays f32. */
int32_t wetts_frontend_set_precision(wetts_frontend_t* f, int32_t precision);
/* The Linear of that mode alone, for tests: f32 x [N][K], weight [M][K], bias [M], residual [N][M] (epilogue 3) and out
 * [N][M], every one of them 16-byte aligned; the weight is packed into `workspace` (16-byte aligned, >=
 * _linear16_workspace_bytes(K, M) bytes) on `stream` first.  precision 1 or 2.  form: 0 = the launcher's choice by N and
 * M (what the forward pass uses: 1 up to 64 tokens, beyond them 3 where ceil(M / 128) * ceil(N / 128) >= 512 and 2
 * otherwise), 1 = K split over the block's waves (64 tokens per block), 2 / 3 = tiled GEMM with 64 / 128 tokens per
 * block.  K % 8 == 0, M % 4 == 0; everything is checked before the first launch. */
int64_t wetts_frontend_linear16_workspace_bytes(int32_t K, int32_t M);
int32_t wetts_frontend_linear16(const float* x, const float* weight, const float* bias, const float* residual, int32_t N,
                                int32_t K, int32_t M, int32_t epilogue, int32_t precision, int32_t form, float* out,
                                void* workspace, int64_t workspace_bytes, void* stream);
/* For the project's own tests and bench tools only; an application needs none of the three.
 * _get_precision: the handle's mode, 0, 1 or 2; negative for a null handle.
 * _linear16_form: the form (1, 2 or 3) that form 0 takes at N tokens and M channels; negative for a bad shape.
 * form | WETTS_FRONTEND_LINEAR16_BENCH_PACKED in wetts_frontend_linear16: the workspace still holds the packed weight of
 * the caller's previous call with the same weight and precision and is not packed again, so that a measurement times
 * the Linear alone.  Nothing can check that claim: a stale workspace gives wrong results silently. */
int32_t wetts_frontend_get_precision(const wetts_frontend_t* f);
int32_t wetts_frontend_linear16_form(int32_t N, int32_t M);
#define WETTS_FRONTEND_LINEAR16_BENCH_PACKED 16

/* ---- scoring the text frontend (csrc/frontend_score.hip) ------------------------------------------------------------
 * The validation pass of frontend/train.py:43-94 (two F.cross_entropy(.., ignore_index=-100) terms, compute_accuracy),
 * the masked accuracy counts of frontend/test_polyphone.py:72-86 and the counts behind the three binary F1 scores of
 * frontend/test_prosody.py:77-102, from the eval-mode forward pass, without a logit in memory: the classifier GEMM
 * leaves one 16-byte record {maximum, sum of exp, lowest argmax, label's logit} per (tile of 32 classes, token), a
 * second launch combines a token's records, a third (one block, float64 sums in a fixed order, no float atomics)
 * reduces.  phone_labels, prosody_labels: int64 [B][T], -100 = ignored (dataset.py:19); either may be NULL = all
 * ignored.  Outputs, all on the device:
 *   nll_phone, nll_prosody [B][T] f32: (max + log sum exp(z - max)) - z[label]; 0 where the label is ignored
 *   pred_phone, pred_prosody [B][T] int32: the LOWEST class of the largest logit; -1 where attention_mask is 0
 *     (these four may be NULL)
 *   losses f32[2]: the mean nll over the scored labels of each head; NaN for a head without any (torch's 0 / 0)
 *   counts int64[22]: [0] phone labels scored, [1] of them predicted; [2], [3] the same for the prosody head;
 *     [4..12] TP, FP, FN of `x > 0`, then of `x > 1`, then of `x > 2`, over the positions 1 .. len_b of every row b,
 *     len_b = the row's count of prosody labels != -100, the slice clipped to T (test_prosody.py:91-93; a -100 label
 *     inside it counts as 0, as does the -1 prediction of a padded token); [13..21] the same nine over 1 .. len_b - 1
 *     (--exclude_end, test_prosody.py:88-89).  Counts, not scores: they add across batches.
 * A label outside [0, classes) that is not -100 ORs WETTS_STATUS_LABEL_RANGE into *status (device int32, may be NULL),
 * a label other than -100 at a token whose mask is 0 WETTS_STATUS_LABEL_AT_PAD (the reference computes on padding,
 * this project zeroes it: there is no common answer); neither token is scored.  Token / type ids: as _forward.
 * `workspace`: 16-byte aligned, workspace_bytes >= wetts_frontend_score_workspace_bytes(f, B, T).  Allocates nothing,
 * no host synchronisation. */
int64_t wetts_frontend_score_workspace_bytes(const wetts_frontend_t* f, int32_t B, int32_t T);
int32_t wetts_frontend_score(const wetts_frontend_t* f, const int64_t* input_ids, const int64_t* token_type_ids,
                             const int64_t* attention_mask, const int64_t* phone_labels, const int64_t* prosody_labels,
                             int32_t B, int32_t T, float* nll_phone, float* nll_prosody, int32_t* pred_phone,
                             int32_t* pred_prosody, float* losses, int64_t* counts, void* workspace,
                             int64_t workspace_bytes, int32_t* status, void* stream);
/* The stage: the three scoring launches on given x [B * T][hidden] and key_mask [B * T] (1.0 / 0.0), the counterpart of
 * wetts_frontend_heads.  The same workspace size serves (it uses the scoring part only). */
int32_t wetts_frontend_score_heads(const wetts_frontend_t* f, const float* x, const float* key_mask,
                                   const int64_t* phone_labels, const int64_t* prosody_labels, int32_t B, int32_t T,
                                   float* nll_phone, float* nll_prosody, int32_t* pred_phone, int32_t* pred_prosody,
                                   float* losses, int64_t* counts, void* workspace, int64_t workspace_bytes,
                                   int32_t* status, void* stream);

/* ---- training the text frontend (csrc/frontend_train.hip) -----------------------------------------------------------
 * The other half of frontend/train.py: the gradient of the loss of train.py:71-84 (loss.backward(), :99) and
 * torch.optim.AdamW's step (:184, :100).  What is trained is what the reference trains (frontend/model.py:30-31 freezes
 * BERT): the 12 `transform.*` tensors and the 4 classifier tensors, the contiguous tail of the blob.  float32 only; the
 * forward pass is the dropout-free one wetts_frontend_forward / _score compute (the reference's model.train() turns on
 * p = 0.1 dropout, whose masks come from torch's generator: out of scope).  No atomics on floats: the same call gives
 * the same bits, and they do not depend on what padded tokens hold. */
/* The trainable tail of the blob (model.py:30-31): *offset = the first float of transform.self_attn.in_proj_weight,
 * *numel = everything from there to the blob's end, alignment padding included. */
int32_t wetts_frontend_trainable_span(const wetts_frontend_config_t* cfg, int64_t* offset, int64_t* numel);
/* Bytes of scratch wetts_frontend_grad needs for B rows of T tokens (T <= 512); negative on a bad argument. */
int64_t wetts_frontend_train_workspace_bytes(const wetts_frontend_t* f, int32_t B, int32_t T);
/* train.py:71-84 and :99 on one batch: forward, loss, backward.  `grad`: the gradients in the blob's own layout of the
 * trainable span (numel floats, 16-byte aligned; its alignment padding is zeroed).  losses / counts / nll_* / pred_* /
 * status: wetts_frontend_score's own outputs from its own launches (the losses are bit-identical to it; nll_* and
 * pred_* may be null).  loss = w phone + (1 - w) prosody with w = polyphone_weight (train.py:83-84).  A head without a
 * scored label reports NaN as wetts_frontend_score does and contributes ZERO gradient (the reference's 0 / 0 would
 * destroy the model); labels flagged LABEL_RANGE / LABEL_AT_PAD are not scored and contribute none.  Allocates nothing
 * and does not synchronise. */
int32_t wetts_frontend_grad(const wetts_frontend_t* f, const int64_t* input_ids, const int64_t* token_type_ids,
                            const int64_t* attention_mask, const int64_t* phone_labels, const int64_t* prosody_labels,
                            int32_t B, int32_t T, double polyphone_weight, float* grad, float* losses, int64_t* counts,
                            float* nll_phone, float* nll_prosody, int32_t* pred_phone, int32_t* pred_prosody,
                            void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);
/* torch.optim.AdamW's single-tensor step (train.py:184 at its defaults, :100) on the handle's trainable span in place:
 * p *= 1 - lr wd; m, v updated; p -= (lr / bias_correction1) m / (sqrt(v) / sqrt(bias_correction2) + eps).  grad, m, v:
 * the span's layout.  The caller forms lr (the schedule of train.py:185-190), bias_correction1 = 1 - beta1^t and
 * bias_correction2 = 1 - beta2^t in double.  wetts_frontend_adamw is the same launch on given buffers (numel % 4 == 0). */
int32_t wetts_frontend_adamw_step(wetts_frontend_t* f, const float* grad, float* m, float* v, double lr, double beta1,
                                  double beta2, double eps, double weight_decay, double bias_correction1,
                                  double bias_correction2, void* stream);
int32_t wetts_frontend_adamw(float* p, const float* grad, float* m, float* v, int64_t numel, double lr, double beta1,
                             double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2,
                             void* stream);
/* Copies floats [offset, offset + numel) of the handle's blob to `out` (device), on the stream (train.py:215 saves them). */
int32_t wetts_frontend_read_weights(const wetts_frontend_t* f, int64_t offset, int64_t numel, float* out, void* stream);
/* The stages of the backward pass alone, each the launch the pass uses (loss.backward(), train.py:99).
 * _linear_dgrad: dx [N][K] = dy [N][M] (row stride ldy) weight [M][K]; epilogue 0 none, 1 zero where aux [N][K] <= 0
 *   (the ReLU mask from the saved activation), 2 + aux [N][K] (the residual's gradient).
 * _linear_wgrad: dw [M][K] = dy^T x over the N tokens, db [M] (may be null) = column sums of dy.
 * _layer_norm_backward: y = LayerNorm(x) gamma + beta -> dx, dgamma, dbeta (the last two may be null);
 *   workspace >= (align64(2 N) + ceil(N / 64) C) floats.
 * _attention_backward: qkv [B T][3 d], ctx = wetts_frontend_attention's output, dctx its gradient -> dqkv [B T][3 d];
 *   workspace >= 2 align64(B heads T T) floats.
 * _ce_backward: dlogits [N][P + R] = w_head / counts[head] (softmax - onehot) at scored tokens, zeros elsewhere;
 *   counts: wetts_frontend_score's 22 (device). */
int32_t wetts_frontend_linear_dgrad(const float* dy, int64_t ldy, const float* weight, int32_t N, int32_t M, int32_t K,
                                    int32_t epilogue, const float* aux, float* dx, void* stream);
int64_t wetts_frontend_linear_wgrad_workspace_bytes(int32_t N, int32_t M, int32_t K);
int32_t wetts_frontend_linear_wgrad(const float* dy, int64_t ldy, const float* x, int32_t N, int32_t M, int32_t K, float* dw,
                                    float* db, void* workspace, int64_t workspace_bytes, void* stream);
int32_t wetts_frontend_layer_norm_backward(const float* dy, const float* x, const float* gamma, float eps, int32_t N,
                                           int32_t C, float* dx, float* dgamma, float* dbeta, void* workspace,
                                           int64_t workspace_bytes, void* stream);
int32_t wetts_frontend_attention_backward(const float* qkv, const float* key_mask, const float* ctx, const float* dctx,
                                          int32_t B, int32_t T, int32_t heads, int32_t dk, float* dqkv, void* workspace,
                                          int64_t workspace_bytes, void* stream);
int32_t wetts_frontend_ce_backward(const float* phone_logits, const float* prosody_logits, const float* key_mask,
                                   const int64_t* phone_labels, const int64_t* prosody_labels, const int64_t* counts,
                                   int32_t N, int32_t P, int32_t R, double polyphone_weight, float* dlogits, void* stream);

/* ---- WavLM, its resampler and the WavLMDiscriminator (losses.py:63-153, model/discriminators.py:452-498;
 * csrc/wavlm.hip) ------------------------------------------------------------------------------------------------
 * transformers' WavLMModel in the `wavlm-base` / `wavlm-base-plus` architecture -- feat_extract_norm "group", no conv
 * bias, post-norm encoder layers, GELU, no attention mask (every row of a batch has the same length) -- without
 * gradients, f32 throughout, returning every hidden state.  A blob and a handle of its own; the blob holds the
 * model's parameters under transformers' names, each at a multiple of 4 floats, with three device layouts: the convs
 * 1 .. of the feature extractor and the positional conv are tap-major, [Cout][k][Cin]; the positional conv has its
 * weight norm folded; gru_rel_pos_const is [heads].  masked_spec_embed is not part of it.
 * Limits: conv_dim multiples of 8, the last at most 1024; hidden_size a multiple of 8 up to 1024; heads of at most 96
 * channels; intermediate_size a multiple of 8; positional groups of a multiple of 4 channels; at most 512 frames per row.
 * Activations are token-major: [B][T][channels]. */
#define WETTS_WAVLM_MAX_CONV 8
typedef struct wetts_wavlm_config {
  int32_t num_conv_layers;
  int32_t conv_dim[WETTS_WAVLM_MAX_CONV], conv_kernel[WETTS_WAVLM_MAX_CONV], conv_stride[WETTS_WAVLM_MAX_CONV];
  int32_t hidden_size, num_layers, num_heads, intermediate_size;
  int32_t pos_kernel, pos_groups;              /* num_conv_pos_embeddings, num_conv_pos_embedding_groups */
  int32_t num_buckets, max_bucket_distance;
  float layer_norm_eps;
} wetts_wavlm_config_t;
typedef struct wetts_wavlm wetts_wavlm_t;
typedef struct wetts_wavlm_disc wetts_wavlm_disc_t;

/* The bucket of a relative position key - query (T5's bidirectional rule as WavLMAttention states it: num_buckets / 2
 * per sign, exact below num_buckets / 4, then a float32 log ramp truncated to an integer and clamped); -1 on a bad
 * argument.  Host only.  The handle holds the table of every relative position it can meet. */
int32_t wetts_wavlm_bucket(int32_t num_buckets, int32_t max_bucket_distance, int32_t relative_position);
/* Frames the feature extractor leaves of L samples (floor((L - k) / s) + 1 per layer, 0 below one frame); -1 on a bad
 * config. */
int64_t wetts_wavlm_num_frames(const wetts_wavlm_config_t* cfg, int64_t L);
int32_t wetts_wavlm_blob_num_tensors(const wetts_wavlm_config_t* cfg);
int32_t wetts_wavlm_blob_tensor_info(const wetts_wavlm_config_t* cfg, int32_t index, char* name_buf, size_t name_buf_len,
                                     int64_t* offset, int64_t* numel, int64_t shape[4]);
int64_t wetts_wavlm_blob_numel(const wetts_wavlm_config_t* cfg);
int32_t wetts_wavlm_create(const wetts_wavlm_config_t* cfg, const float* blob_dev, int64_t blob_numel, void* stream,
                           wetts_wavlm_t** out);
void wetts_wavlm_destroy(wetts_wavlm_t* w);
/* Bytes of scratch wetts_wavlm_forward needs for B rows of L samples; negative on a bad argument (L below one frame
 * and more than 512 frames included). */
int64_t wetts_wavlm_workspace_bytes(const wetts_wavlm_t* w, int32_t B, int64_t L);
/* x: B rows of L samples, row b at x + b * x_bs.  hidden [num_layers + 1][B][T][hidden_size], T = the frames of L:
 * the input of every encoder layer, then the last layer's output.  Every argument is checked before the first launch.
 * Allocates nothing, no host synchronisation. */
int32_t wetts_wavlm_forward(const wetts_wavlm_t* w, const float* x, int64_t x_bs, int32_t B, int64_t L, float* hidden,
                            void* workspace, int64_t workspace_bytes, void* stream);
/* A stand-in for torchaudio.transforms.Resample at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff
 * 0.99), restated from its published arithmetic: orig, new_ the rates over their gcd, width = ceil(6 orig / (0.99
 * min(orig, new_))), kernel [new_][kernel_stride] the float32 sinc matrix (its 2 width + orig taps, then zeros up to
 * kernel_stride, a multiple of 8).  `padded` [B][padded_stride] is scratch for the zero-padded signal, padded_stride >=
 * (L / orig) * orig + kernel_stride.  out [B][(L / orig + 1) * new_]: the frames, interleaved; the caller keeps the
 * first ceil(new_ L / orig) samples of a row. */
int32_t wetts_wavlm_resample(const float* x, int64_t x_bs, int32_t B, int64_t L, int32_t orig, int32_t new_, int32_t width,
                             const float* kernel, int32_t kernel_stride, float* padded, int64_t padded_stride, float* out,
                             void* stream);
/* The stages, each with the kernels the forward pass uses.
 * _conv0: conv 0, its normalisation over time per (row, channel) (biased variance, eps 1e-5, affine), GELU
 *   -> out [B][T0][conv_dim[0]].
 * _conv: conv `layer` (1 ..) and GELU on x [B][Tin][conv_dim[layer - 1]] -> out [B][Tout][conv_dim[layer]].
 * _project: LayerNorm -> normed [N][C], Linear -> out [N][hidden_size].
 * _pos_conv: gelu of the grouped positional conv without its last column, x [B][T][hidden_size] -> out likewise.
 * _attention: the gate of layer `layer` from x [B * T][hidden_size] -> gate [B * T][heads], then attention on
 *   qkv [B * T][3 hidden_size] with logits q . k / sqrt(dk) + gate * bias(layer 0's table) -> out [B * T][hidden_size].
 * _layer: encoder layer `layer` on x -> out (not x); workspace of wetts_wavlm_layer_workspace_bytes. */
int32_t wetts_wavlm_conv0(const wetts_wavlm_t* w, const float* x, int64_t x_bs, int32_t B, int64_t L, float* out,
                          void* stream);
int32_t wetts_wavlm_conv(const wetts_wavlm_t* w, int32_t layer, const float* x, int32_t B, int64_t Tin, float* out,
                         void* stream);
int32_t wetts_wavlm_project(const wetts_wavlm_t* w, const float* x, int32_t N, float* normed, float* out, void* stream);
int32_t wetts_wavlm_pos_conv(const wetts_wavlm_t* w, const float* x, int32_t B, int32_t T, float* out, void* stream);
int32_t wetts_wavlm_attention(const wetts_wavlm_t* w, int32_t layer, const float* x, const float* qkv, int32_t B, int32_t T,
                              float* gate, float* out, void* stream);
int64_t wetts_wavlm_layer_workspace_bytes(const wetts_wavlm_t* w, int32_t B, int32_t T);
int32_t wetts_wavlm_layer(const wetts_wavlm_t* w, int32_t layer, const float* x, int32_t B, int32_t T, float* out,
                          void* workspace, void* stream);

/* WavLMDiscriminator(slm_hidden, slm_layers, initial_channel) with use_spectral_norm = false.  Blob: pre.weight
 * [c0][layers * hidden] (input channel layer * hidden + c), convs.N.weight and conv_post.weight tap-major
 * [Cout][k][Cin], the biases; weight norm folded.  hidden: `layers` buffers [rows][T][hidden], buffer l at
 * hidden + l * layer_stride -- wetts_wavlm_forward's output as it lies.  out [rows][T]. */
int32_t wetts_wavlm_disc_blob_num_tensors(int32_t hidden, int32_t layers, int32_t c0);
int32_t wetts_wavlm_disc_blob_tensor_info(int32_t hidden, int32_t layers, int32_t c0, int32_t index, char* name_buf,
                                          size_t name_buf_len, int64_t* offset, int64_t* numel, int64_t shape[4]);
int64_t wetts_wavlm_disc_blob_numel(int32_t hidden, int32_t layers, int32_t c0);
int32_t wetts_wavlm_disc_create(int32_t hidden, int32_t layers, int32_t c0, const float* blob_dev, int64_t blob_numel,
                                void* stream, wetts_wavlm_disc_t** out);
void wetts_wavlm_disc_destroy(wetts_wavlm_disc_t* d);
int64_t wetts_wavlm_disc_workspace_bytes(const wetts_wavlm_disc_t* d, int32_t rows, int32_t T);
int32_t wetts_wavlm_disc_forward(const wetts_wavlm_disc_t* d, const float* hidden, int64_t layer_stride, int32_t rows,
                                 int32_t T, float* out, void* workspace, void* stream);
/* The stages: `pre` alone -> out [rows][T][c0] (one launch per layer, each reading its buffer in place and adding to
 * out); the three k = 5 convs with leaky_relu(0.1) and conv_post on pre [rows][T][c0] -> out [rows][T]. */
int32_t wetts_wavlm_disc_pre(const wetts_wavlm_disc_t* d, const float* hidden, int64_t layer_stride, int32_t rows, int32_t T,
                             float* out, void* stream);
int32_t wetts_wavlm_disc_convs(const wetts_wavlm_disc_t* d, const float* pre, int32_t rows, int32_t T, float* out,
                               void* workspace, void* stream);

/* ---- The 16-bit conv launches, one at a time (csrc/conv16_entry.hip) -----------------------------------------------
 *
 * Each entry runs ONE launch of the 16-bit decoder / flow (conv_bf16.hip, resblock16.hip, resblock2_stage16.hip,
 * wn16.hip) on caller data, with the launch code wetts_hifigan and the 16-bit WaveNet use.  Weights arrive as f32 in
 * the reference's shapes ([Cout][Cin][k]; transposed [Cin][Cout][k]) and are packed here; activations arrive and
 * leave as the kernels' own 16-bit CHANNEL-LAST tensors [B][T][C] (bfloat16, or IEEE half with f16 != 0); bias /
 * bias_b / mask / skip / conv_post's output are f32.  Every entry allocates what it packs, synchronises `stream` and
 * frees it before it returns; shapes the launchers refuse give WETTS_E_INVALID.  Test and measurement entries: the
 * product path never calls them. */
#define WETTS_CONV16_F16 1        /* IEEE half storage (else bfloat16)                                   */
#define WETTS_CONV16_TRANSPOSED 2 /* ConvTranspose1d at rate `up` (polyphase); no residual / accumulate  */
#define WETTS_CONV16_LRELU 4      /* leaky-relu(in_slope) on the input, rounded to 16 bit                */
#define WETTS_CONV16_ACCUM 8      /* add the previous contents of `out` (the running MRF sum)            */
#define WETTS_CONV16_BASIC 16     /* ConvBParams::basic                                                  */
#define WETTS_CONV16_TAG 32       /* ConvBParams::tag (the MRF launches' own kernel symbol)              */
/* out [B][Tout][Cout] = (conv(act(x)) + bias + bias_b[b] + res [+ out]) / out_div, rounded once.  x [B][Tin][Cin];
 * Tout = Tin + 2 padding - (k - 1) dilation, transposed (Tin - 1) up - 2 padding + k; bias [Cout], bias_b [B][Cout] and
 * res [B][Tout][Cout] may be NULL. */
int32_t wetts_conv16(const float* w, const float* bias, const float* bias_b, const void* x, const void* res, void* out,
                     int32_t B, int32_t Cin, int32_t Cout, int32_t k, int32_t dilation, int32_t padding, int32_t up,
                     int32_t Tin, int32_t Tout, int32_t flags, float in_slope, float out_div, void* stream);
/* The WaveNet in_layer with the gate in its epilogue (epi_mode 1): w [2H][H][k], 'same' padding;
 * acts [B][T][H] = tanh(a) * sigmoid(b) of the rounded conv outputs (+ bias [2H], + bias_b [B][bias_b_stride]). */
int32_t wetts_conv16_wn_gate(const float* w, const float* bias, const float* bias_b, int64_t bias_b_stride, const void* x,
                             void* acts, int32_t B, int32_t H, int32_t k, int32_t dilation, int32_t T, int32_t f16,
                             void* stream);
/* The WaveNet res_skip 1x1 conv with the update in its epilogue (epi_mode 2): w [last ? H : 2H][H][1];
 * h [B][T][H] (16 bit) = (h + rs[:H]) * mask in place unless `last`; skip [B][T][H] f32 (+)= rs[H:] (= when `first`). */
int32_t wetts_conv16_wn_update(const float* w, const float* bias, const void* acts, void* h, float* skip,
                               const float* mask, int32_t B, int32_t H, int32_t T, int32_t last, int32_t first,
                               int32_t f16, void* stream);
/* The two stand-alone WaveNet kernels: xin [rows][2H] -> acts [rows][H]; rs [rows][last ? H : 2H] -> h, skip. */
int32_t wetts_wn16_gate(const void* xin, void* acts, int64_t rows, int32_t H, int32_t f16, void* stream);
int32_t wetts_wn16_update(const void* rs, void* h, float* skip, const float* mask, int32_t last, int32_t first,
                          int64_t rows, int32_t H, int32_t f16, void* stream);
/* conv_post: out [B][T] f32 = tanh(conv(lrelu_0.01(x), w [1][C][7])).  mfma != 0: k_conv_post_mfma16 (C == 32, the
 * weight padded to 32 rows and packed, epi_mode 3); 0: k_conv_post_bf16 (f32 weights). */
int32_t wetts_conv16_post(const float* w, const void* x, float* out, int32_t B, int32_t C, int32_t T, int32_t mfma,
                          int32_t f16, void* stream);
/* One ResBlock launch.  form 0: a ResBlock1 pair  out = (x + c2(lrelu(c1(lrelu(x)))) [+ out]) / out_div  (c2 at
 * dilation 1, nchain 1); 1: a ResBlock2 chain  t = x + c1(lrelu(x)), out = (t + c2(lrelu(t)) [+ out]) / out_div
 * (nchain 1); 2: a ResBlock2 stage, the sum of nchain <= 3 chains over out_div (accum must be 0).  w1 / b1 / w2 / b2:
 * nchain device pointers each ([C][C][k] and [C]); ktaps / dil1 / dil2: nchain host ints.  fused != 0 runs the fused
 * launcher; 0 runs the same arithmetic conv by conv through launch_conv_bf16 and leaves the intermediate (ft / t) of
 * chain j in mid [nchain][B][T][C] (mid is not touched when fused and may then be NULL). */
int32_t wetts_resblock16(int32_t form, int32_t fused, int32_t nchain, const float* const* w1, const float* const* b1,
                         const float* const* w2, const float* const* b2, const int32_t* ktaps, const int32_t* dil1,
                         const int32_t* dil2, const void* x, void* out, void* mid, int32_t B, int32_t C, int32_t T,
                         int32_t accum, float out_div, int32_t f16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WETTS_HIP_H_ */
