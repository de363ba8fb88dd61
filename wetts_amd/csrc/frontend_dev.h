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

// csrc/frontend16.hip: fe_launch_linear's contract on 16-bit operands; x, bias, res and y stay f32, w16 is the packed
// copy of the weight.  precision 1 = bf16, 2 = f16; form 0 = by N and M, 1 = K-split, 2 / 3 = tiled with 64 / 128 tokens.
int32_t fe_launch_linear16(const float* x, const unsigned short* w16, const float* bias, const float* res, float* y, int N,
                           int K, int M, int epi, int precision, int form, hipStream_t s);

}  // namespace wetts
