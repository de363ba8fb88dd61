// The WavLM perceptual loss's network side (losses.py:63-153, model/discriminators.py:452-498), without gradients, f32,
// wave64, on the caller's stream: a sinc resampler (a stand-in for torchaudio.transforms.Resample at its defaults), the
// `wavlm-base` / `wavlm-base-plus` architecture of transformers' WavLMModel (group-norm feature extractor, post-norm
// encoder, gated bucketed relative position bias, every hidden state returned) and the WavLMDiscriminator head.  A blob
// and a handle each for the model and for the discriminator.
//
// Layout.  Activations are token-major from the first conv on, [B][T][C].  In that layout the window of a strided
// Conv1d -- the k input frames of an output frame -- is ONE contiguous run of k * Cin floats that starts at frame
// t * stride, so a conv whose weight is stored tap-major ([Cout][k][Cin]) is a Linear over overlapping rows.  One kernel
// serves all of them: wl_rows_gemm_kernel, the K-split f32-MFMA Linear of frontend.hip with a row address
// (batch stride, row stride) on both sides, a weight row stride, an optional bias / residual and an activation.  It runs
//   the resampler (frames of 2 width + orig samples at stride orig against the [new][2 width + orig] sinc matrix: the
//     [frame][new] output IS the interleaved signal),
//   the strided convs 1 .. 6 of the feature extractor (GELU epilogue),
//   the discriminator's `pre` (13 launches that each read ONE hidden-state buffer in place and add to the running
//     output: the 9984-channel stack is never formed), its k = 5 convs on zero-bordered buffers, and conv_post.
// New kernels beside it: conv 0 with its per-(row, channel) normalisation over time, the grouped positional conv that
// visits only the taps that meet a frame, the gate of the relative position bias, and attention with that bias formed
// on the fly.  LayerNorms and the plain Linears are frontend.hip's, through their C entries.
//
// Every output element is a function of its own batch row alone and is accumulated in an order fixed by the shapes of
// its row: a row alone and the same row inside a batch give the same bits, and so do 2B rows against two calls of B.
// No float atomics.
#include "frontend_dev.h"

#include <math.h>
#include <stdlib.h>

namespace wetts {

enum { WL_ACT_NONE = 0, WL_ACT_GELU = 1, WL_ACT_LRELU = 2 };
constexpr float kWlSlope = 0.1f;  // LRELU_SLOPE of model/discriminators.py

__device__ __forceinline__ float wl_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// ---------------------------------------------------------------------------------------------
// Y[b][t][m] = act(sum_k X[b * x_bs + t * x_rs + k] * W[m * w_rs + k] + bias[m] + res[b][t][m]),  column n = b * rows + t.
// Block shape, K split and the order of every sum: fe_linear_kernel's (8 waves over K in steps of 8, a ring of 4 steps
// in flight, the 8 partial tiles added in wave order).  K % 8 == 0; the weight rows are 16-byte aligned; VEC: so are the
// X rows (else four 4-byte loads).  res is indexed like Y and may be Y itself (each element is read by the thread that
// writes it).
struct WlGemm {
  const float* X;
  int64_t x_bs, x_rs;
  int rows, K;
  const float* W;
  int64_t w_rs;
  const float* bias;
  const float* res;
  float* Y;
  int64_t y_bs, y_rs;
  int N, M, vec_out;
};

template <bool VEC>
__device__ __forceinline__ float4 wl_ld4(const float* p) {
  if (VEC) return *reinterpret_cast<const float4*>(p);
  float4 v;
  v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
  return v;
}

template <int ACT, bool VEC>
__global__ void __launch_bounds__(64 * kFeKG)
wl_rows_gemm_kernel(const WlGemm p) {
  __shared__ float part[kFeKG][2][16][64];
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * kFeNT;
  const int N = p.N, M = p.M;
  const bool two = n0 + 32 < N;  // block-uniform: the second column tile has a column
  const int S = p.K >> 3;

  const int mr = min(m0 + l31, M - 1), c0 = min(n0 + l31, N - 1), c1 = min(n0 + 32 + l31, N - 1);
  const int b0 = c0 / p.rows, b1 = c1 / p.rows;
  const float* wr = p.W + (int64_t)mr * p.w_rs + 4 * half;
  const float* x0 = p.X + (int64_t)b0 * p.x_bs + (int64_t)(c0 - b0 * p.rows) * p.x_rs + 4 * half;
  const float* x1 = p.X + (int64_t)b1 * p.x_bs + (int64_t)(c1 - b1 * p.rows) * p.x_rs + 4 * half;

  f32x16f acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

  float4 ra[kFeRing], rb0[kFeRing], rb1[kFeRing];
#pragma unroll
  for (int i = 0; i < kFeRing; ++i) {
    const int s = w + kFeKG * i;
    if (s < S) {
      ra[i] = *reinterpret_cast<const float4*>(wr + 8 * s);
      rb0[i] = wl_ld4<VEC>(x0 + 8 * s);
      if (two) rb1[i] = wl_ld4<VEC>(x1 + 8 * s);
    }
  }
  for (int sb = w; sb < S; sb += kFeKG * kFeRing) {
#pragma unroll
    for (int i = 0; i < kFeRing; ++i) {
      const int s = sb + kFeKG * i;
      if (s < S) {
        const float4 a = ra[i], v0 = rb0[i];
        float4 v1 = v0;
        if (two) v1 = rb1[i];
        const int sn = s + kFeKG * kFeRing;
        if (sn < S) {
          ra[i] = *reinterpret_cast<const float4*>(wr + 8 * sn);
          rb0[i] = wl_ld4<VEC>(x0 + 8 * sn);
          if (two) rb1[i] = wl_ld4<VEC>(x1 + 8 * sn);
        }
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, v0.x, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, v0.y, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, v0.z, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, v0.w, acc0, 0, 0, 0);
        if (two) {
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, v1.x, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, v1.y, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, v1.z, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, v1.w, acc1, 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    part[w][0][r][lane] = acc0[r];
    part[w][1][r][lane] = acc1[r];
  }
  __syncthreads();
  // wave w: column tile w / 4, the registers 4 g .. 4 g + 3 (g = w % 4) = rows m0 + 8 g + 4 half + {0..3} of column l31
  const int t = w >> 2, g = w & 3;
  if (t == 1 && !two) return;
  const int col = n0 + 32 * t + l31, m = m0 + 8 * g + 4 * half;
  if (col >= N || m >= M) return;
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 4 * g + i;
    v[i] = ((part[0][t][r][lane] + part[1][t][r][lane]) + (part[2][t][r][lane] + part[3][t][r][lane])) +
           ((part[4][t][r][lane] + part[5][t][r][lane]) + (part[6][t][r][lane] + part[7][t][r][lane]));
  }
  const int b = col / p.rows;
  const int64_t yo = (int64_t)b * p.y_bs + (int64_t)(col - b * p.rows) * p.y_rs + m;
  if (p.vec_out) {  // M % 4 == 0 and 16-byte aligned rows of bias / res / Y
    if (p.bias) {
      const float4 bv = *reinterpret_cast<const float4*>(p.bias + m);
      v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
    }
    if (p.res) {
      const float4 rv = *reinterpret_cast<const float4*>(p.res + yo);
      v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ACT == WL_ACT_GELU) v[i] = wl_gelu(v[i]);
      if (ACT == WL_ACT_LRELU) v[i] = v[i] > 0.f ? v[i] : kWlSlope * v[i];
    }
    float4 o;
    o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
    *reinterpret_cast<float4*>(p.Y + yo) = o;
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (m + i < M) {
      float z = v[i];
      if (p.bias) z += p.bias[m + i];
      if (p.res) z += p.res[yo + i];
      if (ACT == WL_ACT_GELU) z = wl_gelu(z);
      if (ACT == WL_ACT_LRELU) z = z > 0.f ? z : kWlSlope * z;
      p.Y[yo + i] = z;
    }
}

static bool wl_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Checks the geometry and launches.  The caller guarantees that every X row holds K readable floats.
static int32_t wl_launch_gemm(WlGemm p, int act, hipStream_t s) {
  WETTS_REQUIRE(p.X && p.W && p.Y && p.N >= 1 && p.M >= 1 && p.rows >= 1, "wavlm gemm: bad argument (N=%d, M=%d)", p.N, p.M);
  WETTS_REQUIRE(p.K >= 8 && p.K % 8 == 0, "wavlm gemm: K=%d must be a multiple of 8", p.K);
  WETTS_REQUIRE(wl_al16(p.W) && p.w_rs % 4 == 0, "wavlm gemm: weight rows must be 16-byte aligned");
  WETTS_REQUIRE(act >= WL_ACT_NONE && act <= WL_ACT_LRELU, "wavlm gemm: activation %d", act);
  const int64_t ct = ((int64_t)p.N + kFeNT - 1) / kFeNT;
  WETTS_REQUIRE(ct <= 65535, "wavlm gemm: %d columns exceed one launch", p.N);
  const bool vec = wl_al16(p.X) && p.x_bs % 4 == 0 && p.x_rs % 4 == 0;
  p.vec_out = p.M % 4 == 0 && wl_al16(p.Y) && p.y_bs % 4 == 0 && p.y_rs % 4 == 0 && (!p.bias || wl_al16(p.bias)) &&
              (!p.res || wl_al16(p.res));
  const dim3 grid((unsigned)cdiv(p.M, 32), (unsigned)ct), block(64 * kFeKG);
#define WL_GEMM(A, V) hipLaunchKernelGGL((wl_rows_gemm_kernel<A, V>), grid, block, 0, s, p)
  if (vec) {
    if (act == WL_ACT_GELU) WL_GEMM(WL_ACT_GELU, true);
    else if (act == WL_ACT_LRELU) WL_GEMM(WL_ACT_LRELU, true);
    else WL_GEMM(WL_ACT_NONE, true);
  } else {
    if (act == WL_ACT_GELU) WL_GEMM(WL_ACT_GELU, false);
    else if (act == WL_ACT_LRELU) WL_GEMM(WL_ACT_LRELU, false);
    else WL_GEMM(WL_ACT_NONE, false);
  }
#undef WL_GEMM
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// The resampler's padded signal: pad[b][i] = x[b][i - width] for width <= i < width + L, else 0, i < stride.
__global__ void __launch_bounds__(256)
wl_pad_kernel(const float* __restrict__ x, int64_t x_bs, int L, int width, float* __restrict__ pad, int64_t stride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= stride) return;
  const int64_t j = i - width;
  pad[(int64_t)blockIdx.y * stride + i] = (j >= 0 && j < L) ? x[(int64_t)blockIdx.y * x_bs + j] : 0.f;
}

// ---------------------------------------------------------------------------------------------
// Conv 0 (1 -> C, k taps, no bias): y[b][t][c] = sum_j w[c][j] x[b][t * stride + j], one thread per (t, c), the taps in
// ascending order as one fma chain.
__global__ void __launch_bounds__(256)
wl_conv0_kernel(const float* __restrict__ x, int64_t x_bs, const float* __restrict__ w, int C, int k, int stride, int T0,
                float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)T0 * C) return;
  const int t = (int)(i / C), c = (int)(i - (int64_t)t * C);
  const float* xr = x + (int64_t)blockIdx.y * x_bs + (int64_t)t * stride;
  const float* wr = w + (int64_t)c * k;
  float a = 0.f;
  for (int j = 0; j < k; ++j) a = __builtin_fmaf(wr[j], xr[j], a);
  y[(int64_t)blockIdx.y * T0 * C + i] = a;
}

// GroupNorm with one channel per group, then GELU, in place on y [B][T][C]: a block serves 64 channels of one row;
// lane = channel, wave w adds the frames w, w + 4, .. in ascending order and the four partial sums are added as
// (0 + 1) + (2 + 3): the mean, then the centred squares (biased variance, as F.group_norm), then the update.
__global__ void __launch_bounds__(256)
wl_gn_gelu_kernel(float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int T,
                  int C) {
  __shared__ float part[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const bool on = c < C;
  float* col = y + (int64_t)blockIdx.y * T * C + (on ? c : 0);
  float s = 0.f;
  if (on)
    for (int t = wave; t < T; t += 4) s += col[(int64_t)t * C];
  part[0][wave][lane] = s;
  __syncthreads();
  const float mean = ((part[0][0][lane] + part[0][1][lane]) + (part[0][2][lane] + part[0][3][lane])) / (float)T;
  float s2 = 0.f;
  if (on)
    for (int t = wave; t < T; t += 4) {
      const float d = col[(int64_t)t * C] - mean;
      s2 = __builtin_fmaf(d, d, s2);
    }
  part[1][wave][lane] = s2;
  __syncthreads();
  if (!on) return;
  const float var = ((part[1][0][lane] + part[1][1][lane]) + (part[1][2][lane] + part[1][3][lane])) / (float)T;
  const float rstd = 1.f / sqrtf(var + eps), g = gamma[c], bt = beta[c];
  for (int t = wave; t < T; t += 4) {
    const float v = __builtin_fmaf((col[(int64_t)t * C] - mean) * rstd, g, bt);
    col[(int64_t)t * C] = wl_gelu(v);
  }
}

// ---------------------------------------------------------------------------------------------
// The positional conv: Conv1d(H, H, k, padding k / 2, groups) on x [B][T][H] with the weight tap-major per group,
// w [H][k][cg]; the output column T (an even kernel has one more than T) is not computed.  One thread per (b, t, co):
// only the taps j = t' - t + k / 2 that meet a frame t' in [0, T) are visited -- at T = 18 and k = 128 that is 18 of 128.
// Four partial sums (the float4 lanes of the channel run), frames ascending, added as (x + y) + (z + w); then bias, GELU.
__global__ void __launch_bounds__(256)
wl_pos_conv_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int T, int H,
                   int k, int cg, float* __restrict__ out) {
  const int co = blockIdx.x * 256 + threadIdx.x;
  if (co >= H) return;
  const int t = blockIdx.y, b = blockIdx.z, pad = k >> 1;
  const int g0 = (co / cg) * cg;
  const int lo = max(0, t - pad), hi = min(T - 1, t - pad + k - 1);
  const float* xb = x + (int64_t)b * T * H + g0;
  const float* wr = w + (int64_t)co * k * cg;
  float4 a;
  a.x = a.y = a.z = a.w = 0.f;
  for (int tp = lo; tp <= hi; ++tp) {
    const float4* xv = reinterpret_cast<const float4*>(xb + (int64_t)tp * H);
    const float4* wv = reinterpret_cast<const float4*>(wr + (int64_t)(tp - t + pad) * cg);
    for (int e = 0; e < (cg >> 2); ++e) {
      const float4 p = xv[e], q = wv[e];
      a.x = __builtin_fmaf(p.x, q.x, a.x);
      a.y = __builtin_fmaf(p.y, q.y, a.y);
      a.z = __builtin_fmaf(p.z, q.z, a.z);
      a.w = __builtin_fmaf(p.w, q.w, a.w);
    }
  }
  out[((int64_t)b * T + t) * H + co] = wl_gelu(((a.x + a.y) + (a.z + a.w)) + bias[co]);
}

// ---------------------------------------------------------------------------------------------
// The gate of the relative position bias, one thread per (token, head): p = gru_rel_pos_linear(x viewed as heads) [8],
// a = sigmoid(p0 + p1 + p2 + p3), b = sigmoid(p4 + .. + p7), gate = a (b const[h] - 1) + 2.  gate [N][heads].
__global__ void __launch_bounds__(256)
wl_gate_kernel(const float* __restrict__ x, const float* __restrict__ wg, const float* __restrict__ bg,
               const float* __restrict__ cst, int N, int heads, int dk, float* __restrict__ gate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * heads) return;
  const int h = i % heads;
  const float* xr = x + (int64_t)i * dk;  // token n's head h: n * heads * dk + h * dk
  float p[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) p[o] = 0.f;
  for (int e = 0; e < dk; ++e) {
    const float v = xr[e];
#pragma unroll
    for (int o = 0; o < 8; ++o) p[o] = __builtin_fmaf(v, wg[o * dk + e], p[o]);
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) p[o] += bg[o];
  const float sa = ((p[0] + p[1]) + p[2]) + p[3], sb = ((p[4] + p[5]) + p[6]) + p[7];
  const float a = 1.f / (1.f + expf(-sa)), bb = 1.f / (1.f + expf(-sb));
  gate[i] = a * (bb * cst[h] - 1.f) + 2.f;
}

// ---------------------------------------------------------------------------------------------
// Attention with the gated relative position bias on the packed projection qkv [N][3 d] -> ctx [N][d]: the schedule of
// fe_attention_kernel (a block of four waves serves 16 queries of one (row, head); scores, softmax, P V over key chunks
// of 64 staged in LDS) without a key mask, and with
//     score[i][j] = q_i . k_j / sqrt(dk) + gate[b][i][h] * emb[bucket[j - i]][h]
// formed as the score is stored: the [B, H, T, T] bias never exists in memory.  bucket: the handle's table over
// j - i = -(kFeMaxT - 1) .. kFeMaxT - 1; emb: layer 0's rel_attn_embed [num_buckets][heads], for every layer.
__global__ void __launch_bounds__(256)
wl_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ gate, const float* __restrict__ emb,
                    const int* __restrict__ bucket, float* __restrict__ ctx, int T, int H, int dk, float scale) {
  __shared__ float kv[64 * (kFeMaxDk + 1)];
  __shared__ float4 qs[4][kFeMaxDk];
  __shared__ float4 sc[4][kFeMaxT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int d = H * dk, ld = 3 * d, ldk = dk | 1;
  const float* base = qkv + (int64_t)b * T * ld + h * dk;
  const int q0 = qt * 16 + wave * 4;
  int qi[4];
  float gt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    qi[i] = min(q0 + i, T - 1);
    gt[i] = gate[((int64_t)b * T + qi[i]) * H + h];
  }
  for (int i = lane; i < dk; i += 64) {
    float4 q;
    q.x = base[(int64_t)qi[0] * ld + i];
    q.y = base[(int64_t)qi[1] * ld + i];
    q.z = base[(int64_t)qi[2] * ld + i];
    q.w = base[(int64_t)qi[3] * ld + i];
    qs[wave][i] = q;
  }
  const int nch = (T + 63) >> 6;
  for (int c = 0; c < nch; ++c) {
    __syncthreads();
    for (int i = tid; i < 64 * dk; i += 256) {
      const int j = i / dk, e = i - j * dk;
      const int key = min(c * 64 + j, T - 1);
      kv[j * ldk + e] = base[(int64_t)key * ld + d + e];
    }
    __syncthreads();
    float4 s;
    s.x = s.y = s.z = s.w = 0.f;
    const float* kr = kv + lane * ldk;
    for (int e = 0; e < dk; ++e) {
      const float k = kr[e];
      const float4 q = qs[wave][e];
      s.x = __builtin_fmaf(q.x, k, s.x);
      s.y = __builtin_fmaf(q.y, k, s.y);
      s.z = __builtin_fmaf(q.z, k, s.z);
      s.w = __builtin_fmaf(q.w, k, s.w);
    }
    const int key = c * 64 + lane;
    if (key < T) {
      const int* bk = bucket + (kFeMaxT - 1) + key;
      s.x = __builtin_fmaf(gt[0], emb[bk[-qi[0]] * H + h], s.x * scale);
      s.y = __builtin_fmaf(gt[1], emb[bk[-qi[1]] * H + h], s.y * scale);
      s.z = __builtin_fmaf(gt[2], emb[bk[-qi[2]] * H + h], s.z * scale);
      s.w = __builtin_fmaf(gt[3], emb[bk[-qi[3]] * H + h], s.w * scale);
      sc[wave][key] = s;
    }
  }
  // softmax (this wave's own rows of sc: no block barrier needed)
  float4 mx;
  mx.x = mx.y = mx.z = mx.w = -INFINITY;
  for (int key = lane; key < T; key += 64) {
    const float4 s = sc[wave][key];
    mx.x = fmaxf(mx.x, s.x); mx.y = fmaxf(mx.y, s.y); mx.z = fmaxf(mx.z, s.z); mx.w = fmaxf(mx.w, s.w);
  }
  mx.x = fe_wave_max(mx.x); mx.y = fe_wave_max(mx.y); mx.z = fe_wave_max(mx.z); mx.w = fe_wave_max(mx.w);
  float4 sum;
  sum.x = sum.y = sum.z = sum.w = 0.f;
  for (int key = lane; key < T; key += 64) {
    const float4 s = sc[wave][key];
    float4 p;
    p.x = expf(s.x - mx.x); p.y = expf(s.y - mx.y); p.z = expf(s.z - mx.z); p.w = expf(s.w - mx.w);
    sc[wave][key] = p;
    sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w;
  }
  sum.x = fe_wave_sum(sum.x); sum.y = fe_wave_sum(sum.y); sum.z = fe_wave_sum(sum.z); sum.w = fe_wave_sum(sum.w);
  float4 o0, o1;
  o0.x = o0.y = o0.z = o0.w = 0.f;
  o1 = o0;
  const bool hi = lane + 64 < dk;
  const int e0 = min(lane, dk - 1);
  for (int c = 0; c < nch; ++c) {
    __syncthreads();
    for (int i = tid; i < 64 * dk; i += 256) {
      const int j = i / dk, e = i - j * dk;
      const int key = min(c * 64 + j, T - 1);
      kv[j * dk + e] = base[(int64_t)key * ld + 2 * d + e];
    }
    __syncthreads();
    const int nk = min(64, T - c * 64);
    for (int j = 0; j < nk; ++j) {
      const float4 p = sc[wave][c * 64 + j];
      const float v0 = kv[j * dk + e0];
      o0.x = __builtin_fmaf(p.x, v0, o0.x);
      o0.y = __builtin_fmaf(p.y, v0, o0.y);
      o0.z = __builtin_fmaf(p.z, v0, o0.z);
      o0.w = __builtin_fmaf(p.w, v0, o0.w);
      if (hi) {
        const float v1 = kv[j * dk + lane + 64];
        o1.x = __builtin_fmaf(p.x, v1, o1.x);
        o1.y = __builtin_fmaf(p.y, v1, o1.y);
        o1.z = __builtin_fmaf(p.z, v1, o1.z);
        o1.w = __builtin_fmaf(p.w, v1, o1.w);
      }
    }
  }
  float* ob = ctx + (int64_t)b * T * d + h * dk;
  const float r0[4] = {o0.x, o0.y, o0.z, o0.w}, r1[4] = {o1.x, o1.y, o1.z, o1.w};
  const float sm[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = q0 + i;
    if (q < T) {
      if (lane < dk) ob[(int64_t)q * d + lane] = r0[i] / sm[i];
      if (hi) ob[(int64_t)q * d + lane + 64] = r1[i] / sm[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// transformers' WavLMAttention._relative_positions_bucket for one relative position (key - query): num_buckets / 2 per
// sign, exact below max_exact = num_buckets / 4, then the float32 log ramp truncated towards zero, clamped.
static int wl_bucket(int num_buckets, int max_distance, int rel) {
  const int nb = num_buckets / 2, max_exact = nb / 2;
  const int base = rel > 0 ? nb : 0, p = rel < 0 ? -rel : rel;
  if (p < max_exact) return base + p;
  float v = logf((float)p / (float)max_exact);
  v = v / (float)log((double)max_distance / (double)max_exact);
  v = v * (float)(nb - max_exact);
  const long q = (long)((float)max_exact + v);
  return base + (int)(q < nb - 1 ? q : nb - 1);
}

struct WlTensor {
  std::string name;
  int64_t offset, numel, shape[4];
};

struct WlLayout {
  std::vector<WlTensor> tensors;
  int64_t total = 0;
  void add(const std::string& name, int64_t s0, int64_t s1 = 0, int64_t s2 = 0) {
    WlTensor t;
    t.name = name;
    t.offset = total;
    t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = 0;
    t.numel = s0 * (s1 > 0 ? s1 : 1) * (s2 > 0 ? s2 : 1);
    total = align_up(total + t.numel, 4);
    tensors.push_back(t);
  }
  int64_t off(const std::string& name) const {
    for (const WlTensor& t : tensors)
      if (t.name == name) return t.offset;
    return -1;
  }
};

static int32_t wl_tensor_info(const WlLayout& L, int32_t index, char* name_buf, size_t name_buf_len, int64_t* offset,
                              int64_t* numel, int64_t shape[4]) {
  WETTS_REQUIRE(index >= 0 && index < (int32_t)L.tensors.size(), "tensor index %d out of range", index);
  const WlTensor& t = L.tensors[index];
  WETTS_REQUIRE(name_buf && name_buf_len > t.name.size(), "name buffer too small");
  strcpy(name_buf, t.name.c_str());
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  return WETTS_OK;
}

static const char* wl_config_error(const wetts_wavlm_config_t* c) {
  if (!c) return "null config";
  if (c->num_conv_layers < 2 || c->num_conv_layers > WETTS_WAVLM_MAX_CONV) return "num_conv_layers must be 2 .. 8";
  for (int i = 0; i < c->num_conv_layers; ++i) {
    if (c->conv_dim[i] < 8 || c->conv_dim[i] % 8 || c->conv_dim[i] > 4096) return "conv_dim must be multiples of 8 up to 4096";
    if (c->conv_kernel[i] < 1 || c->conv_kernel[i] > 64 || c->conv_stride[i] < 1 || c->conv_stride[i] > 64)
      return "conv_kernel and conv_stride must be 1 .. 64";
  }
  if (c->conv_dim[c->num_conv_layers - 1] > kFeMaxC) return "the last conv_dim must be at most 1024";
  if (c->hidden_size < 8 || c->hidden_size > kFeMaxC || c->hidden_size % 8) return "hidden_size must be a multiple of 8 up to 1024";
  if (c->num_layers < 1 || c->num_layers > 64) return "num_hidden_layers out of range";
  if (c->num_heads < 1 || c->hidden_size % c->num_heads || c->hidden_size / c->num_heads > kFeMaxDk)
    return "num_attention_heads must divide hidden_size into heads of at most 96";
  if (c->intermediate_size < 8 || c->intermediate_size % 8) return "intermediate_size must be a multiple of 8";
  if (c->pos_kernel < 1 || c->pos_kernel > 1024) return "num_conv_pos_embeddings out of range";
  if (c->pos_groups < 1 || c->hidden_size % c->pos_groups || (c->hidden_size / c->pos_groups) % 4)
    return "num_conv_pos_embedding_groups must divide hidden_size into groups of a multiple of 4 channels";
  if (c->num_buckets < 4 || c->num_buckets > 4096 || c->max_bucket_distance < 2) return "num_buckets / max_bucket_distance out of range";
  if (c->max_bucket_distance * 4 <= c->num_buckets) return "max_bucket_distance must exceed num_buckets / 4";
  if (!(c->layer_norm_eps > 0.f)) return "layer_norm_eps must be positive";
  return nullptr;
}

static std::string wl_layer_prefix(int i) { return "encoder.layers." + std::to_string(i) + "."; }

// transformers' parameter names.  Device layouts that differ from the state_dict's: the convs 1 .. of the feature
// extractor and the positional conv are tap-major, [Cout][k][Cin] (a window of the token-major activations is one
// run); the positional conv has its weight norm folded; gru_rel_pos_const is [heads].  q, k, v follow each other
// without a gap (hidden_size % 8 == 0): one packed [3 d][d] projection.
static WlLayout wl_layout(const wetts_wavlm_config_t* c) {
  WlLayout l;
  const int d = c->hidden_size, dk = d / c->num_heads, cl = c->conv_dim[c->num_conv_layers - 1];
  l.add("feature_extractor.conv_layers.0.conv.weight", c->conv_dim[0], c->conv_kernel[0]);
  l.add("feature_extractor.conv_layers.0.layer_norm.weight", c->conv_dim[0]);
  l.add("feature_extractor.conv_layers.0.layer_norm.bias", c->conv_dim[0]);
  for (int i = 1; i < c->num_conv_layers; ++i)
    l.add("feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight", c->conv_dim[i], c->conv_kernel[i], c->conv_dim[i - 1]);
  l.add("feature_projection.layer_norm.weight", cl);
  l.add("feature_projection.layer_norm.bias", cl);
  l.add("feature_projection.projection.weight", d, cl);
  l.add("feature_projection.projection.bias", d);
  l.add("encoder.pos_conv_embed.conv.weight", d, c->pos_kernel, d / c->pos_groups);
  l.add("encoder.pos_conv_embed.conv.bias", d);
  l.add("encoder.layer_norm.weight", d);
  l.add("encoder.layer_norm.bias", d);
  for (int i = 0; i < c->num_layers; ++i) {
    const std::string p = wl_layer_prefix(i);
    l.add(p + "attention.q_proj.weight", d, d);
    l.add(p + "attention.k_proj.weight", d, d);
    l.add(p + "attention.v_proj.weight", d, d);
    l.add(p + "attention.q_proj.bias", d);
    l.add(p + "attention.k_proj.bias", d);
    l.add(p + "attention.v_proj.bias", d);
    l.add(p + "attention.out_proj.weight", d, d);
    l.add(p + "attention.out_proj.bias", d);
    l.add(p + "attention.gru_rel_pos_linear.weight", 8, dk);
    l.add(p + "attention.gru_rel_pos_linear.bias", 8);
    l.add(p + "attention.gru_rel_pos_const", c->num_heads);
    if (i == 0) l.add(p + "attention.rel_attn_embed.weight", c->num_buckets, c->num_heads);
    l.add(p + "layer_norm.weight", d);
    l.add(p + "layer_norm.bias", d);
    l.add(p + "feed_forward.intermediate_dense.weight", c->intermediate_size, d);
    l.add(p + "feed_forward.intermediate_dense.bias", c->intermediate_size);
    l.add(p + "feed_forward.output_dense.weight", d, c->intermediate_size);
    l.add(p + "feed_forward.output_dense.bias", d);
    l.add(p + "final_layer_norm.weight", d);
    l.add(p + "final_layer_norm.bias", d);
  }
  return l;
}

struct WlBlock {
  const float *wqkv, *bqkv, *wo, *bo, *wg, *bg, *cst, *g1, *b1, *w1, *bb1, *w2, *bb2, *g2, *b2;
};

}  // namespace wetts

struct wetts_wavlm {
  wetts_wavlm_config_t cfg;
  float* blob = nullptr;
  int* bucket = nullptr;  // device, [2 kFeMaxT - 1]: the bucket of key - query
  const float* conv_w[WETTS_WAVLM_MAX_CONV] = {};
  const float *gn_g = nullptr, *gn_b = nullptr, *fp_g = nullptr, *fp_b = nullptr, *fp_w = nullptr, *fp_bias = nullptr;
  const float *pos_w = nullptr, *pos_b = nullptr, *enc_g = nullptr, *enc_b = nullptr, *emb = nullptr;
  std::vector<wetts::WlBlock> blocks;
};

struct wetts_wavlm_disc {
  int hidden = 0, layers = 0, c0 = 0;
  float* blob = nullptr;
  const float *pre_w = nullptr, *pre_b = nullptr, *cw[3] = {}, *cb[3] = {}, *post_w = nullptr, *post_b = nullptr;
};

namespace wetts {

// frames after conv layer i for L samples (floor((L - k) / s) + 1 per layer; 0 once a layer has no full window)
static void wl_lengths(const wetts_wavlm_config_t& c, int64_t L, int64_t T[WETTS_WAVLM_MAX_CONV]) {
  int64_t t = L;
  for (int i = 0; i < c.num_conv_layers; ++i) {
    t = t >= c.conv_kernel[i] ? (t - c.conv_kernel[i]) / c.conv_stride[i] + 1 : 0;
    T[i] = t;
  }
}

// regions of the forward pass's workspace, in floats: two conv buffers, then ln [N][Cl], h2, tmp, pos, ctx [N][d],
// qkv [N][3 d], ff [N][ff], gate [N][heads]
enum { WL_A, WL_B, WL_LN, WL_H2, WL_TMP, WL_POS, WL_CTX, WL_QKV, WL_FF, WL_GATE, WL_NREG };

static void wl_regions(const wetts_wavlm_config_t& c, int B, const int64_t T[WETTS_WAVLM_MAX_CONV], int64_t off[WL_NREG + 1]) {
  const int nl = c.num_conv_layers;
  const int64_t N = B * T[nl - 1], d = c.hidden_size;
  int64_t a = 0, b = 0;
  for (int i = 0; i < nl; ++i) {
    const int64_t n = B * T[i] * c.conv_dim[i];
    if (i % 2 == 0) a = n > a ? n : a; else b = n > b ? n : b;
  }
  const int64_t sizes[WL_NREG] = {a, b, N * c.conv_dim[nl - 1], N * d, N * d, N * d, N * d, 3 * N * d,
                                  N * c.intermediate_size, N * c.num_heads};
  off[0] = 0;
  for (int i = 0; i < WL_NREG; ++i) off[i + 1] = off[i] + align_up(sizes[i], 64);
}

static int32_t wl_check_rows(const wetts_wavlm* h, int B, int64_t L, int64_t T[WETTS_WAVLM_MAX_CONV], const char* what) {
  WETTS_REQUIRE(h, "%s: null handle", what);
  WETTS_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L <= 0x7fffffff / 4, "%s: B=%d, L=%lld out of range", what, B, (long long)L);
  wl_lengths(h->cfg, L, T);
  const int64_t Tl = T[h->cfg.num_conv_layers - 1];
  WETTS_REQUIRE(Tl >= 1, "%s: %lld samples are shorter than one frame of the feature extractor", what, (long long)L);
  WETTS_REQUIRE(Tl <= kFeMaxT, "%s: %lld samples give %lld frames, at most %d", what, (long long)L, (long long)Tl, kFeMaxT);
  WETTS_REQUIRE((int64_t)B * T[0] * h->cfg.conv_dim[0] <= 0x7fffffffLL * 8, "%s: %d rows of %lld samples exceed one call", what, B,
                (long long)L);
  return WETTS_OK;
}

static int32_t wl_launch_conv0(const wetts_wavlm* h, const float* x, int64_t x_bs, int B, int64_t T0, float* y, hipStream_t s) {
  const wetts_wavlm_config_t& c = h->cfg;
  const int64_t n = T0 * c.conv_dim[0];
  WETTS_REQUIRE(x && y && (n + 255) / 256 <= 0x7fffffff, "wavlm conv 0: bad argument");
  hipLaunchKernelGGL(wl_conv0_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, s, x, x_bs, h->conv_w[0],
                     c.conv_dim[0], c.conv_kernel[0], c.conv_stride[0], (int)T0, y);
  WETTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(wl_gn_gelu_kernel, dim3((unsigned)cdiv(c.conv_dim[0], 64), (unsigned)B), dim3(256), 0, s, y, h->gn_g, h->gn_b,
                     1e-5f, (int)T0, c.conv_dim[0]);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// conv layer i >= 1 on x [B][Tin][C(i-1)] -> y [B][Tout][C(i)], GELU
static int32_t wl_launch_conv(const wetts_wavlm* h, int i, const float* x, int B, int64_t Tin, int64_t Tout, float* y,
                              hipStream_t s) {
  const wetts_wavlm_config_t& c = h->cfg;
  const int ci = c.conv_dim[i - 1], co = c.conv_dim[i];
  WETTS_REQUIRE((int64_t)B * Tout <= 0x7fffffff, "wavlm conv %d: %d x %lld frames exceed one launch", i, B, (long long)Tout);
  WlGemm p = {};
  p.X = x; p.x_bs = Tin * ci; p.x_rs = (int64_t)c.conv_stride[i] * ci; p.rows = (int)Tout; p.K = c.conv_kernel[i] * ci;
  p.W = h->conv_w[i]; p.w_rs = p.K;
  p.Y = y; p.y_bs = Tout * co; p.y_rs = co; p.N = (int)(B * Tout); p.M = co;
  return wl_launch_gemm(p, WL_ACT_GELU, s);
}

static int32_t wl_launch_pos_conv(const wetts_wavlm* h, const float* x, int B, int T, float* out, hipStream_t s) {
  const wetts_wavlm_config_t& c = h->cfg;
  WETTS_REQUIRE(x && out && B >= 1 && B <= 65535 && T >= 1 && T <= kFeMaxT, "wavlm positional conv: B=%d, T=%d", B, T);
  hipLaunchKernelGGL(wl_pos_conv_kernel, dim3((unsigned)cdiv(c.hidden_size, 256), (unsigned)T, (unsigned)B), dim3(256), 0, s, x,
                     h->pos_w, h->pos_b, T, c.hidden_size, c.pos_kernel, c.hidden_size / c.pos_groups, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t wl_launch_attention(const wetts_wavlm* h, int layer, const float* x, const float* qkv, int B, int T, float* gate,
                                   float* ctx, hipStream_t s) {
  const wetts_wavlm_config_t& c = h->cfg;
  WETTS_REQUIRE(x && qkv && gate && ctx, "wavlm attention: null argument");
  WETTS_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kFeMaxT, "wavlm attention: B=%d, T=%d (at most %d)", B, T, kFeMaxT);
  WETTS_REQUIRE((int64_t)B * T * c.num_heads <= 0x7fffffff, "wavlm attention: too many tokens");
  const WlBlock& k = h->blocks[layer];
  const int N = B * T, H = c.num_heads, dk = c.hidden_size / H;
  hipLaunchKernelGGL(wl_gate_kernel, dim3((unsigned)cdiv(N * H, 256)), dim3(256), 0, s, x, k.wg, k.bg, k.cst, N, H, dk, gate);
  WETTS_LAUNCH_CHECK();
  static_assert(sizeof(float) * (64 * (kFeMaxDk + 1) + 4 * 4 * kFeMaxDk + 4 * 4 * kFeMaxT) <= 64 * 1024, "wavlm attention LDS");
  hipLaunchKernelGGL(wl_attention_kernel, dim3((unsigned)cdiv(T, 16), (unsigned)H, (unsigned)B), dim3(256), 0, s, qkv, gate, h->emb,
                     h->bucket, ctx, T, H, dk, 1.f / sqrtf((float)dk));
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// one post-norm layer: x [N][d] -> out [N][d] (out != x); ws: the forward pass's regions
static int32_t wl_run_layer(const wetts_wavlm* h, int layer, const float* x, int B, int T, float* out, float* ws,
                            const int64_t off[WL_NREG + 1], hipStream_t s) {
  const wetts_wavlm_config_t& c = h->cfg;
  const WlBlock& k = h->blocks[layer];
  const int N = B * T, d = c.hidden_size;
  float *h2 = ws + off[WL_H2], *tmp = ws + off[WL_TMP], *ctx = ws + off[WL_CTX], *qkv = ws + off[WL_QKV], *ff = ws + off[WL_FF],
        *gate = ws + off[WL_GATE];
  WETTS_TRY(wetts_frontend_linear(x, k.wqkv, k.bqkv, nullptr, N, d, 3 * d, WETTS_FRONTEND_EPI_BIAS, qkv, s));
  WETTS_TRY(wl_launch_attention(h, layer, x, qkv, B, T, gate, ctx, s));
  WETTS_TRY(wetts_frontend_linear(ctx, k.wo, k.bo, x, N, d, d, WETTS_FRONTEND_EPI_RESIDUAL, h2, s));
  WETTS_TRY(wetts_frontend_add_layer_norm(h2, nullptr, k.g1, k.b1, c.layer_norm_eps, N, d, tmp, s));
  WETTS_TRY(wetts_frontend_linear(tmp, k.w1, k.bb1, nullptr, N, d, c.intermediate_size, WETTS_FRONTEND_EPI_GELU, ff, s));
  WETTS_TRY(wetts_frontend_linear(ff, k.w2, k.bb2, tmp, N, c.intermediate_size, d, WETTS_FRONTEND_EPI_RESIDUAL, h2, s));
  return wetts_frontend_add_layer_norm(h2, nullptr, k.g2, k.b2, c.layer_norm_eps, N, d, out, s);
}

// ---- the discriminator ---------------------------------------------------------------------------------------------
static const char* wd_config_error(int hidden, int layers, int c0) {
  if (hidden < 8 || hidden % 8 || hidden > 4096) return "slm_hidden must be a multiple of 8 up to 4096";
  if (layers < 1 || layers > 64) return "slm_layers must be 1 .. 64";
  if (c0 < 8 || c0 % 8 || c0 > 1024) return "initial_channel must be a multiple of 8 up to 1024";
  return nullptr;
}

// weight norm folded; the k = 5 and k = 3 convs tap-major, [Cout][k][Cin]; pre.weight [c0][layers * hidden], input
// channel layer * hidden + c (the reference's stack / transpose / flatten)
static WlLayout wd_layout(int hidden, int layers, int c0) {
  WlLayout l;
  l.add("pre.weight", c0, (int64_t)layers * hidden);
  l.add("pre.bias", c0);
  const int ci[3] = {c0, 2 * c0, 4 * c0}, co[3] = {2 * c0, 4 * c0, 4 * c0};
  for (int i = 0; i < 3; ++i) {
    l.add("convs." + std::to_string(i) + ".weight", co[i], 5, ci[i]);
    l.add("convs." + std::to_string(i) + ".bias", co[i]);
  }
  l.add("conv_post.weight", 1, 3, 4 * c0);
  l.add("conv_post.bias", 1);
  return l;
}

// pre: out[r][t][:] = bias + sum_layers W[:, layer] hidden[layer][r][t][:], one launch per layer, each adding to `out`
static int32_t wd_launch_pre(const wetts_wavlm_disc* d, const float* hidden, int64_t layer_stride, int R, int T, float* out,
                             int64_t o_bs, hipStream_t s) {
  for (int l = 0; l < d->layers; ++l) {
    WlGemm p = {};
    p.X = hidden + l * layer_stride; p.x_bs = (int64_t)T * d->hidden; p.x_rs = d->hidden; p.rows = T; p.K = d->hidden;
    p.W = d->pre_w + (int64_t)l * d->hidden; p.w_rs = (int64_t)d->layers * d->hidden;
    p.bias = l == 0 ? d->pre_b : nullptr; p.res = l == 0 ? nullptr : out;
    p.Y = out; p.y_bs = o_bs; p.y_rs = d->c0; p.N = R * T; p.M = d->c0;
    WETTS_TRY(wl_launch_gemm(p, WL_ACT_NONE, s));
  }
  return WETTS_OK;
}

// the zero-bordered buffers [R][T + 4][C] of pre's output and the three convs' outputs, in floats
static void wd_regions(const wetts_wavlm_disc* d, int R, int T, int64_t off[5]) {
  const int ch[4] = {d->c0, 2 * d->c0, 4 * d->c0, 4 * d->c0};
  off[0] = 0;
  for (int i = 0; i < 4; ++i) off[i + 1] = off[i] + align_up((int64_t)R * (T + 4) * ch[i], 64);
}

// the three k = 5 convs with leaky_relu(0.1) and conv_post on the bordered pre buffer ws + off[0] -> out [R][T]
static int32_t wd_launch_convs(const wetts_wavlm_disc* d, int R, int T, float* ws, const int64_t off[5], float* out,
                               hipStream_t s) {
  const int ch[4] = {d->c0, 2 * d->c0, 4 * d->c0, 4 * d->c0};
  for (int i = 0; i < 3; ++i) {
    WlGemm p = {};
    p.X = ws + off[i]; p.x_bs = (int64_t)(T + 4) * ch[i]; p.x_rs = ch[i]; p.rows = T; p.K = 5 * ch[i];
    p.W = d->cw[i]; p.w_rs = p.K; p.bias = d->cb[i];
    p.Y = ws + off[i + 1] + 2 * ch[i + 1]; p.y_bs = (int64_t)(T + 4) * ch[i + 1]; p.y_rs = ch[i + 1]; p.N = R * T; p.M = ch[i + 1];
    WETTS_TRY(wl_launch_gemm(p, WL_ACT_LRELU, s));
  }
  WlGemm p = {};
  p.X = ws + off[3] + ch[3]; p.x_bs = (int64_t)(T + 4) * ch[3]; p.x_rs = ch[3]; p.rows = T; p.K = 3 * ch[3];
  p.W = d->post_w; p.w_rs = p.K; p.bias = d->post_b;
  p.Y = out; p.y_bs = T; p.y_rs = 1; p.N = R * T; p.M = 1;
  return wl_launch_gemm(p, WL_ACT_NONE, s);
}

static int32_t wd_check(const wetts_wavlm_disc* d, int R, int T, const char* what) {
  WETTS_REQUIRE(d, "%s: null handle", what);
  WETTS_REQUIRE(R >= 1 && T >= 1 && (int64_t)R * (T + 4) * 4 * d->c0 <= 0x7fffffff && (int64_t)R * T * d->hidden <= 0x7fffffff,
                "%s: rows=%d, T=%d out of range", what, R, T);
  return WETTS_OK;
}

template <class H>
static int32_t wl_copy_blob(H* h, const float* blob_dev, int64_t numel, hipStream_t s, const char* what) {
  hipError_t e = hipMalloc((void**)&h->blob, (size_t)numel * sizeof(float));
  if (e == hipSuccess) e = hipMemcpyAsync(h->blob, blob_dev, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    if (h->blob) (void)hipFree(h->blob);
    h->blob = nullptr;
    return WETTS_E_HIP;
  }
  return WETTS_OK;
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_wavlm_bucket(int32_t num_buckets, int32_t max_bucket_distance, int32_t relative_position) {
  if (num_buckets < 4 || max_bucket_distance < 2 || max_bucket_distance * 4 <= num_buckets) {
    set_error("wavlm_bucket: num_buckets=%d, max_bucket_distance=%d", num_buckets, max_bucket_distance);
    return -1;
  }
  return wl_bucket(num_buckets, max_bucket_distance, relative_position);
}

int64_t wetts_wavlm_num_frames(const wetts_wavlm_config_t* cfg, int64_t L) {
  if (const char* e = wl_config_error(cfg)) {
    set_error("wavlm config: %s", e);
    return -1;
  }
  int64_t T[WETTS_WAVLM_MAX_CONV];
  wl_lengths(*cfg, L, T);
  return T[cfg->num_conv_layers - 1];
}

int32_t wetts_wavlm_blob_num_tensors(const wetts_wavlm_config_t* cfg) {
  if (const char* e = wl_config_error(cfg)) {
    set_error("wavlm config: %s", e);
    return -1;
  }
  return (int32_t)wl_layout(cfg).tensors.size();
}

int32_t wetts_wavlm_blob_tensor_info(const wetts_wavlm_config_t* cfg, int32_t index, char* name_buf, size_t name_buf_len,
                                     int64_t* offset, int64_t* numel, int64_t shape[4]) {
  const char* e = wl_config_error(cfg);
  WETTS_REQUIRE(e == nullptr, "wavlm config: %s", e);
  return wl_tensor_info(wl_layout(cfg), index, name_buf, name_buf_len, offset, numel, shape);
}

int64_t wetts_wavlm_blob_numel(const wetts_wavlm_config_t* cfg) {
  if (const char* e = wl_config_error(cfg)) {
    set_error("wavlm config: %s", e);
    return -1;
  }
  return wl_layout(cfg).total;
}

int32_t wetts_wavlm_create(const wetts_wavlm_config_t* cfg, const float* blob_dev, int64_t blob_numel, void* stream,
                           wetts_wavlm_t** out) {
  WETTS_REQUIRE(out != nullptr && blob_dev != nullptr, "null argument");
  const char* ce = wl_config_error(cfg);
  WETTS_REQUIRE(ce == nullptr, "wavlm config: %s", ce);
  const WlLayout L = wl_layout(cfg);
  WETTS_REQUIRE(blob_numel == L.total, "blob has %lld floats, the wavlm layout needs %lld", (long long)blob_numel,
                (long long)L.total);
  wetts_wavlm* h = new wetts_wavlm();
  h->cfg = *cfg;
  int32_t rc = wl_copy_blob(h, blob_dev, blob_numel, (hipStream_t)stream, "wetts_wavlm_create");
  if (rc == WETTS_OK) {
    std::vector<int> tab(2 * kFeMaxT - 1);
    for (int r = -(kFeMaxT - 1); r <= kFeMaxT - 1; ++r)
      tab[r + kFeMaxT - 1] = wl_bucket(cfg->num_buckets, cfg->max_bucket_distance, r);
    hipError_t e = hipMalloc((void**)&h->bucket, tab.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(h->bucket, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      set_error("wetts_wavlm_create: %s", hipGetErrorString(e));
      rc = WETTS_E_HIP;
    }
  }
  if (rc != WETTS_OK) {
    if (h->bucket) (void)hipFree(h->bucket);
    if (h->blob) (void)hipFree(h->blob);
    delete h;
    return rc;
  }
  auto at = [&](const std::string& name) { return h->blob + L.off(name); };
  for (int i = 0; i < cfg->num_conv_layers; ++i)
    h->conv_w[i] = at("feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight");
  h->gn_g = at("feature_extractor.conv_layers.0.layer_norm.weight");
  h->gn_b = at("feature_extractor.conv_layers.0.layer_norm.bias");
  h->fp_g = at("feature_projection.layer_norm.weight");
  h->fp_b = at("feature_projection.layer_norm.bias");
  h->fp_w = at("feature_projection.projection.weight");
  h->fp_bias = at("feature_projection.projection.bias");
  h->pos_w = at("encoder.pos_conv_embed.conv.weight");
  h->pos_b = at("encoder.pos_conv_embed.conv.bias");
  h->enc_g = at("encoder.layer_norm.weight");
  h->enc_b = at("encoder.layer_norm.bias");
  h->emb = at("encoder.layers.0.attention.rel_attn_embed.weight");
  for (int i = 0; i < cfg->num_layers; ++i) {
    const std::string p = wl_layer_prefix(i);
    WlBlock k;
    k.wqkv = at(p + "attention.q_proj.weight");
    k.bqkv = at(p + "attention.q_proj.bias");
    k.wo = at(p + "attention.out_proj.weight");
    k.bo = at(p + "attention.out_proj.bias");
    k.wg = at(p + "attention.gru_rel_pos_linear.weight");
    k.bg = at(p + "attention.gru_rel_pos_linear.bias");
    k.cst = at(p + "attention.gru_rel_pos_const");
    k.g1 = at(p + "layer_norm.weight");
    k.b1 = at(p + "layer_norm.bias");
    k.w1 = at(p + "feed_forward.intermediate_dense.weight");
    k.bb1 = at(p + "feed_forward.intermediate_dense.bias");
    k.w2 = at(p + "feed_forward.output_dense.weight");
    k.bb2 = at(p + "feed_forward.output_dense.bias");
    k.g2 = at(p + "final_layer_norm.weight");
    k.b2 = at(p + "final_layer_norm.bias");
    h->blocks.push_back(k);
  }
  *out = h;
  return WETTS_OK;
}

void wetts_wavlm_destroy(wetts_wavlm_t* h) {
  if (!h) return;
  if (h->bucket) (void)hipFree(h->bucket);
  if (h->blob) (void)hipFree(h->blob);
  delete h;
}

int64_t wetts_wavlm_workspace_bytes(const wetts_wavlm_t* h, int32_t B, int64_t L) {
  int64_t T[WETTS_WAVLM_MAX_CONV];
  if (wl_check_rows(h, B, L, T, "wavlm_workspace_bytes") != WETTS_OK) return -1;
  int64_t off[WL_NREG + 1];
  wl_regions(h->cfg, B, T, off);
  return off[WL_NREG] * (int64_t)sizeof(float);
}

int32_t wetts_wavlm_resample(const float* x, int64_t x_bs, int32_t B, int64_t L, int32_t orig, int32_t new_, int32_t width,
                             const float* kernel, int32_t kernel_stride, float* padded, int64_t padded_stride, float* out,
                             void* stream) {
  WETTS_REQUIRE(x && kernel && padded && out, "wavlm_resample: null argument");
  WETTS_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L <= 0x7fffffff / 4, "wavlm_resample: B=%d, L=%lld", B, (long long)L);
  WETTS_REQUIRE(orig >= 1 && new_ >= 1 && width >= 1 && orig <= 1 << 20 && new_ <= 1 << 20 && width <= 1 << 20,
                "wavlm_resample: orig=%d, new=%d, width=%d", orig, new_, width);
  const int64_t frames = L / orig + 1, taps = 2 * (int64_t)width + orig;
  WETTS_REQUIRE(kernel_stride >= taps && kernel_stride % 8 == 0, "wavlm_resample: kernel_stride=%d must be a multiple of 8 of at least %lld",
                kernel_stride, (long long)taps);
  WETTS_REQUIRE(padded_stride >= (frames - 1) * orig + kernel_stride && x_bs >= L,
                "wavlm_resample: padded_stride=%lld is shorter than the %lld frames read", (long long)padded_stride, (long long)frames);
  WETTS_REQUIRE(B * frames <= 0x7fffffff && frames * new_ <= 0x7fffffff, "wavlm_resample: too many frames");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(wl_pad_kernel, dim3((unsigned)((padded_stride + 255) / 256), (unsigned)B), dim3(256), 0, s, x, x_bs, (int)L, width,
                     padded, padded_stride);
  WETTS_LAUNCH_CHECK();
  WlGemm p = {};
  p.X = padded; p.x_bs = padded_stride; p.x_rs = orig; p.rows = (int)frames; p.K = kernel_stride;
  p.W = kernel; p.w_rs = kernel_stride;
  p.Y = out; p.y_bs = frames * new_; p.y_rs = new_; p.N = (int)(B * frames); p.M = new_;
  return wl_launch_gemm(p, WL_ACT_NONE, s);
}

int32_t wetts_wavlm_conv0(const wetts_wavlm_t* h, const float* x, int64_t x_bs, int32_t B, int64_t L, float* out, void* stream) {
  int64_t T[WETTS_WAVLM_MAX_CONV];
  WETTS_TRY(wl_check_rows(h, B, L, T, "wavlm_conv0"));
  WETTS_REQUIRE(x_bs >= L, "wavlm_conv0: batch stride %lld is shorter than a row", (long long)x_bs);
  return wl_launch_conv0(h, x, x_bs, B, T[0], out, (hipStream_t)stream);
}

int32_t wetts_wavlm_conv(const wetts_wavlm_t* h, int32_t layer, const float* x, int32_t B, int64_t Tin, float* out,
                         void* stream) {
  WETTS_REQUIRE(h && x && out, "wavlm_conv: null argument");
  WETTS_REQUIRE(layer >= 1 && layer < h->cfg.num_conv_layers, "wavlm_conv: layer %d is not one of 1..%d", layer,
                h->cfg.num_conv_layers - 1);
  WETTS_REQUIRE(B >= 1 && Tin >= h->cfg.conv_kernel[layer] && Tin <= 0x7fffffff / 4, "wavlm_conv: B=%d, Tin=%lld", B, (long long)Tin);
  const int64_t Tout = (Tin - h->cfg.conv_kernel[layer]) / h->cfg.conv_stride[layer] + 1;
  return wl_launch_conv(h, layer, x, B, Tin, Tout, out, (hipStream_t)stream);
}

int32_t wetts_wavlm_project(const wetts_wavlm_t* h, const float* x, int32_t N, float* normed, float* out, void* stream) {
  WETTS_REQUIRE(h && x && normed && out && N >= 1, "wavlm_project: bad argument");
  const int cl = h->cfg.conv_dim[h->cfg.num_conv_layers - 1];
  WETTS_TRY(wetts_frontend_add_layer_norm(x, nullptr, h->fp_g, h->fp_b, h->cfg.layer_norm_eps, N, cl, normed, stream));
  return wetts_frontend_linear(normed, h->fp_w, h->fp_bias, nullptr, N, cl, h->cfg.hidden_size, WETTS_FRONTEND_EPI_BIAS, out, stream);
}

int32_t wetts_wavlm_pos_conv(const wetts_wavlm_t* h, const float* x, int32_t B, int32_t T, float* out, void* stream) {
  WETTS_REQUIRE(h, "wavlm_pos_conv: null handle");
  return wl_launch_pos_conv(h, x, B, T, out, (hipStream_t)stream);
}

int32_t wetts_wavlm_attention(const wetts_wavlm_t* h, int32_t layer, const float* x, const float* qkv, int32_t B, int32_t T,
                              float* gate, float* out, void* stream) {
  WETTS_REQUIRE(h && layer >= 0 && layer < h->cfg.num_layers, "wavlm_attention: layer %d", layer);
  return wl_launch_attention(h, layer, x, qkv, B, T, gate, out, (hipStream_t)stream);
}

int64_t wetts_wavlm_layer_workspace_bytes(const wetts_wavlm_t* h, int32_t B, int32_t T) {
  if (!h || B < 1 || T < 1 || T > kFeMaxT || (int64_t)B * T > 0x7fffffff / 4) {
    set_error("wavlm_layer_workspace_bytes: bad argument (B=%d T=%d)", B, T);
    return -1;
  }
  int64_t Tl[WETTS_WAVLM_MAX_CONV] = {}, off[WL_NREG + 1];
  Tl[h->cfg.num_conv_layers - 1] = T;
  wl_regions(h->cfg, B, Tl, off);
  return off[WL_NREG] * (int64_t)sizeof(float);
}

int32_t wetts_wavlm_layer(const wetts_wavlm_t* h, int32_t layer, const float* x, int32_t B, int32_t T, float* out,
                          void* workspace, void* stream) {
  WETTS_REQUIRE(h && x && out && workspace && x != out, "wavlm_layer: bad argument");
  WETTS_REQUIRE(layer >= 0 && layer < h->cfg.num_layers, "wavlm_layer: layer %d is not one of 0..%d", layer, h->cfg.num_layers - 1);
  WETTS_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kFeMaxT && (int64_t)B * T <= 0x7fffffff / 4, "wavlm_layer: B=%d, T=%d", B, T);
  int64_t Tl[WETTS_WAVLM_MAX_CONV] = {}, off[WL_NREG + 1];
  Tl[h->cfg.num_conv_layers - 1] = T;
  wl_regions(h->cfg, B, Tl, off);
  return wl_run_layer(h, layer, x, B, T, out, (float*)workspace, off, (hipStream_t)stream);
}

int32_t wetts_wavlm_forward(const wetts_wavlm_t* h, const float* x, int64_t x_bs, int32_t B, int64_t L, float* hidden,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  int64_t T[WETTS_WAVLM_MAX_CONV];
  WETTS_TRY(wl_check_rows(h, B, L, T, "wavlm_forward"));
  WETTS_REQUIRE(x && hidden && workspace && x_bs >= L, "wavlm_forward: bad argument");
  const wetts_wavlm_config_t& c = h->cfg;
  int64_t off[WL_NREG + 1];
  wl_regions(c, B, T, off);
  WETTS_REQUIRE(workspace_bytes >= off[WL_NREG] * (int64_t)sizeof(float), "wavlm_forward: workspace of %lld bytes, needs %lld",
                (long long)workspace_bytes, (long long)(off[WL_NREG] * sizeof(float)));
  for (int i = 1; i < c.num_conv_layers; ++i)
    WETTS_REQUIRE((int64_t)B * T[i] <= 0x7fffffff && ((int64_t)B * T[i] + kFeNT - 1) / kFeNT <= 65535,
                  "wavlm_forward: %d rows of %lld frames exceed one launch of conv %d", B, (long long)T[i], i);
  WETTS_REQUIRE((int64_t)B * T[c.num_conv_layers - 1] * c.num_heads <= 0x7fffffff,
                "wavlm_forward: %d rows of %lld frames and %d heads exceed one launch of the attention", B,
                (long long)T[c.num_conv_layers - 1], c.num_heads);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int nl = c.num_conv_layers, Tl = (int)T[nl - 1], N = B * Tl, d = c.hidden_size;
  WETTS_TRY(wl_launch_conv0(h, x, x_bs, B, T[0], ws + off[WL_A], s));
  for (int i = 1; i < nl; ++i)
    WETTS_TRY(wl_launch_conv(h, i, ws + off[(i - 1) % 2 ? WL_B : WL_A], B, T[i - 1], T[i], ws + off[i % 2 ? WL_B : WL_A], s));
  const float* feat = ws + off[(nl - 1) % 2 ? WL_B : WL_A];
  float *ln = ws + off[WL_LN], *proj = ws + off[WL_TMP], *pos = ws + off[WL_POS];
  WETTS_TRY(wetts_wavlm_project(h, feat, N, ln, proj, stream));
  WETTS_TRY(wl_launch_pos_conv(h, proj, B, Tl, pos, s));
  WETTS_TRY(wetts_frontend_add_layer_norm(proj, pos, h->enc_g, h->enc_b, c.layer_norm_eps, N, d, hidden, stream));
  for (int i = 0; i < c.num_layers; ++i)
    WETTS_TRY(wl_run_layer(h, i, hidden + (int64_t)i * N * d, B, Tl, hidden + (int64_t)(i + 1) * N * d, ws, off, s));
  return WETTS_OK;
}

// ---- the discriminator ---------------------------------------------------------------------------------------------
int32_t wetts_wavlm_disc_blob_num_tensors(int32_t hidden, int32_t layers, int32_t c0) {
  if (const char* e = wd_config_error(hidden, layers, c0)) {
    set_error("wavlm discriminator: %s", e);
    return -1;
  }
  return (int32_t)wd_layout(hidden, layers, c0).tensors.size();
}

int32_t wetts_wavlm_disc_blob_tensor_info(int32_t hidden, int32_t layers, int32_t c0, int32_t index, char* name_buf,
                                          size_t name_buf_len, int64_t* offset, int64_t* numel, int64_t shape[4]) {
  const char* e = wd_config_error(hidden, layers, c0);
  WETTS_REQUIRE(e == nullptr, "wavlm discriminator: %s", e);
  return wl_tensor_info(wd_layout(hidden, layers, c0), index, name_buf, name_buf_len, offset, numel, shape);
}

int64_t wetts_wavlm_disc_blob_numel(int32_t hidden, int32_t layers, int32_t c0) {
  if (const char* e = wd_config_error(hidden, layers, c0)) {
    set_error("wavlm discriminator: %s", e);
    return -1;
  }
  return wd_layout(hidden, layers, c0).total;
}

int32_t wetts_wavlm_disc_create(int32_t hidden, int32_t layers, int32_t c0, const float* blob_dev, int64_t blob_numel,
                                void* stream, wetts_wavlm_disc_t** out) {
  WETTS_REQUIRE(out != nullptr && blob_dev != nullptr, "null argument");
  const char* ce = wd_config_error(hidden, layers, c0);
  WETTS_REQUIRE(ce == nullptr, "wavlm discriminator: %s", ce);
  const WlLayout L = wd_layout(hidden, layers, c0);
  WETTS_REQUIRE(blob_numel == L.total, "blob has %lld floats, the wavlm discriminator layout needs %lld", (long long)blob_numel,
                (long long)L.total);
  wetts_wavlm_disc* d = new wetts_wavlm_disc();
  d->hidden = hidden; d->layers = layers; d->c0 = c0;
  const int32_t rc = wl_copy_blob(d, blob_dev, blob_numel, (hipStream_t)stream, "wetts_wavlm_disc_create");
  if (rc != WETTS_OK) {
    delete d;
    return rc;
  }
  auto at = [&](const std::string& name) { return d->blob + L.off(name); };
  d->pre_w = at("pre.weight");
  d->pre_b = at("pre.bias");
  for (int i = 0; i < 3; ++i) {
    d->cw[i] = at("convs." + std::to_string(i) + ".weight");
    d->cb[i] = at("convs." + std::to_string(i) + ".bias");
  }
  d->post_w = at("conv_post.weight");
  d->post_b = at("conv_post.bias");
  *out = d;
  return WETTS_OK;
}

void wetts_wavlm_disc_destroy(wetts_wavlm_disc_t* d) {
  if (!d) return;
  if (d->blob) (void)hipFree(d->blob);
  delete d;
}

int64_t wetts_wavlm_disc_workspace_bytes(const wetts_wavlm_disc_t* d, int32_t rows, int32_t T) {
  if (wd_check(d, rows, T, "wavlm_disc_workspace_bytes") != WETTS_OK) return -1;
  int64_t off[5];
  wd_regions(d, rows, T, off);
  return off[4] * (int64_t)sizeof(float);
}

int32_t wetts_wavlm_disc_pre(const wetts_wavlm_disc_t* d, const float* hidden, int64_t layer_stride, int32_t rows, int32_t T,
                             float* out, void* stream) {
  WETTS_TRY(wd_check(d, rows, T, "wavlm_disc_pre"));
  WETTS_REQUIRE(hidden && out && layer_stride % 4 == 0, "wavlm_disc_pre: bad argument");
  return wd_launch_pre(d, hidden, layer_stride, rows, T, out, (int64_t)T * d->c0, (hipStream_t)stream);
}

int32_t wetts_wavlm_disc_convs(const wetts_wavlm_disc_t* d, const float* pre, int32_t rows, int32_t T, float* out,
                               void* workspace, void* stream) {
  WETTS_TRY(wd_check(d, rows, T, "wavlm_disc_convs"));
  WETTS_REQUIRE(pre && out && workspace, "wavlm_disc_convs: null argument");
  int64_t off[5];
  wd_regions(d, rows, T, off);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  WETTS_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)off[4] * sizeof(float), s));
  WETTS_HIP_CHECK(hipMemcpy2DAsync(ws + 2 * d->c0, (size_t)(T + 4) * d->c0 * sizeof(float), pre, (size_t)T * d->c0 * sizeof(float),
                                   (size_t)T * d->c0 * sizeof(float), (size_t)rows, hipMemcpyDeviceToDevice, s));
  return wd_launch_convs(d, rows, T, ws, off, out, s);
}

int32_t wetts_wavlm_disc_forward(const wetts_wavlm_disc_t* d, const float* hidden, int64_t layer_stride, int32_t rows,
                                 int32_t T, float* out, void* workspace, void* stream) {
  WETTS_TRY(wd_check(d, rows, T, "wavlm_disc_forward"));
  WETTS_REQUIRE(hidden && out && workspace && layer_stride % 4 == 0, "wavlm_disc_forward: bad argument");
  int64_t off[5];
  wd_regions(d, rows, T, off);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  WETTS_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)off[4] * sizeof(float), s));
  WETTS_TRY(wd_launch_pre(d, hidden, layer_stride, rows, T, ws + 2 * d->c0, (int64_t)(T + 4) * d->c0, s));
  return wd_launch_convs(d, rows, T, ws, off, out, s);
}

}  // extern "C"
