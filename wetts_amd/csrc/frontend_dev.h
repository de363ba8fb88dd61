// What csrc/frontend.hip and csrc/frontend_score.hip share: the wave reductions, the block shape of the K-split f32-MFMA
// Linear, the handle and the forward pass up to the transform layer's output.
#pragma once
#include "common.h"

#include <vector>

namespace wetts {

typedef float f32x16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float fe_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float fe_wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// fe_linear_kernel's block: 8 waves that split K in steps of 8, a ring of 4 steps in flight per wave, 64 token columns
constexpr int kFeKG = 8, kFeRing = 4, kFeNT = 64;
constexpr int kFeMaxC = 1024, kFeMaxT = 512, kFeMaxDk = 96;

struct FeBlock {  // one post-norm transformer layer
  const float *wqkv, *bqkv, *wo, *bo, *g1, *b1, *w1, *bb1, *w2, *bb2, *g2, *b2;
  int heads, ff, act;
  float eps;
  // the 16-bit copies of wqkv, wo, w1, w2 (natural [M][K] layout), null in f32 mode: wetts_frontend_set_precision
  const unsigned short *wqkv16 = nullptr, *wo16 = nullptr, *w116 = nullptr, *w216 = nullptr;
};

}  // namespace wetts

struct wetts_frontend {
  wetts_frontend_config_t cfg;
  float* blob = nullptr;
  const float *word = nullptr, *pos = nullptr, *type = nullptr, *eg = nullptr, *eb = nullptr;
  std::vector<wetts::FeBlock> blocks;  // the BERT layers, then `transform`
  const float *wp = nullptr, *bp = nullptr, *wr = nullptr, *br = nullptr;
  int precision = 0;              // 0 = f32, 1 = bf16, 2 = f16: the operands of the layers' Linears (csrc/frontend16.hip)
  unsigned short* w16 = nullptr;  // one allocation behind the blocks' 16-bit pointers
};

namespace wetts {

// floats of scratch the forward pass needs for B rows of T tokens (what wetts_frontend_workspace_bytes reports)
int64_t fe_workspace_floats(const wetts_frontend* h, int B, int T);
// The forward pass without the heads: embeddings, the BERT layers, `transform`.  *x [B * T][hidden] and *maskf [B * T]
// (1.0 / 0.0) point into `workspace`.  Checks B, T like wetts_frontend_forward; `what` names the caller in messages.
int32_t fe_hidden(const wetts_frontend* h, const int64_t* ids, const int64_t* tts, const int64_t* mask, int B, int T,
                  void* workspace, int32_t* status, hipStream_t s, const char* what, const float** x, const float** maskf);

// What the training pass (csrc/frontend_train.hip) builds on: the launchers of the forward stages (frontend.hip), the
// scoring launches (frontend_score.hip) and the blob layout.  fe_tensor_offset: a tensor's first float in the blob, -1 for
// an unknown name, the blob's size for a null name.  fe_run_block: one post-norm layer on h in place.
int64_t fe_tensor_offset(const wetts_frontend_config_t* c, const char* name);
int32_t fe_launch_linear(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int K, int M,
                         int epi, hipStream_t s);
int32_t fe_launch_add_ln(const float* x, const float* res, const float* gamma, const float* beta, float eps, int N, int C,
                         float* out, hipStream_t s);
int32_t fe_launch_attention(const float* qkv, const float* maskf, float* ctx, int B, int T, int H, int dk, hipStream_t s);
int32_t fe_launch_heads(const wetts_frontend* h, const float* x, const float* maskf, int N, int softmax, float* phone,
                        float* prosody, hipStream_t s);
int32_t fe_launch_embed(const wetts_frontend* h, const int64_t* ids, const int64_t* tts, const int64_t* mask, int B, int T,
                        float* out, float* maskf, int32_t* status, hipStream_t s);
int32_t fe_run_block(const FeBlock& k, int d, float* h, float* h2, float* ctx, float* qkv, float* ff, const float* maskf,
                     int B, int T, int prec, hipStream_t s);
int64_t fs_bytes(const wetts_frontend_config_t& c, int B, int T, int64_t* npad);
int32_t fs_launch(const wetts_frontend* h, const float* x, const float* maskf, const int64_t* lab_p, const int64_t* lab_r,
                  int B, int T, float* nll_p, float* nll_r, int32_t* pred_p, int32_t* pred_r, float* losses, int64_t* counts,
                  void* workspace, int64_t workspace_bytes, int32_t* status, hipStream_t s);

// fe_hidden after the first `layers` layers only (the BERT layers come first, `transform` is the last one)
int32_t fe_hidden_layers(const wetts_frontend* h, int layers, const int64_t* ids, const int64_t* tts, const int64_t* mask,
                         int B, int T, void* workspace, int32_t* status, hipStream_t s, const char* what, const float** x,
                         const float** maskf);

// csrc/frontend16.hip: fe_launch_linear's contract on 16-bit operands; x, bias, res and y stay f32, w16 is the packed
// copy of the weight.  precision 1 = bf16, 2 = f16; form 0 = by N and M, 1 = K-split, 2 / 3 = tiled with 64 / 128 tokens.
int32_t fe_launch_linear16(const float* x, const unsigned short* w16, const float* bias, const float* res, float* y, int N,
                           int K, int M, int epi, int precision, int form, hipStream_t s);

}  // namespace wetts
