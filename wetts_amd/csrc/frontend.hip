// The text frontend (frontend/model.py:21-73): an HF BertModel (absolute positions, last_hidden_state), one
// nn.TransformerEncoderLayer (batch_first, post-norm, ReLU) and the polyphone / prosody classifiers, without gradients.
// All f32, wave64, on the caller's stream; a blob and a handle of its own.  (wetts_frontend_set_precision, frontend16.hip:
// the layers' Linears alone may read bf16 / f16 operands; every kernel of this file is the same in that mode.)
//
// Layout.  Activations are token-major, [N = B * T][C]: a token's channels are contiguous, so the embedding gather, the
// LayerNorms, the classifier rows and the [B, T, classes] outputs are all row operations, and BOTH operands of a Linear
// (x [N][K], weight [M][K]) are contiguous along the reduction.  Tokens of all utterances are laid end to end and are the
// columns of every GEMM.
//
// Every output element is a function of its own utterance alone: a GEMM column accumulates its own k sequence in an order
// fixed by the block shape, a LayerNorm / classifier / softmax row is reduced by one wave in a fixed order, and attention
// gives a masked key the weight +0 exactly, which changes no bit of a sum.  A row alone and the same row inside a padded
// batch give the same bits.  No atomics on floats (the status word is an integer OR).
#include "frontend_dev.h"

#include <math.h>

namespace wetts {

// ---------------------------------------------------------------------------------------------
// LayerNorm over the channels of a token, one wave per token, the row in registers (C <= 1024, C % 4 == 0): lane l holds
// the float4s l, l + 64, ..; two passes (mean, then centred squares), each a per-lane sum in ascending order and the
// butterfly over the lanes.  Biased variance, as F.layer_norm.
constexpr int kFeRowV = kFeMaxC / 256;

__device__ __forceinline__ void fe_layer_norm_row(float4 v[kFeRowV], int C, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float eps, float* __restrict__ out,
                                                  int lane) {
  const int nv = C >> 2;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kFeRowV; ++i)
    if (lane + 64 * i < nv) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mean = fe_wave_sum(s) / (float)C;
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < kFeRowV; ++i)
    if (lane + 64 * i < nv) {
      v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
      s2 += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
  const float rstd = 1.f / sqrtf(fe_wave_sum(s2) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < kFeRowV; ++i)
    if (lane + 64 * i < nv) {
      const float4 g = reinterpret_cast<const float4*>(gamma)[lane + 64 * i];
      const float4 b = reinterpret_cast<const float4*>(beta)[lane + 64 * i];
      float4 o;
      o.x = __builtin_fmaf(v[i].x * rstd, g.x, b.x);
      o.y = __builtin_fmaf(v[i].y * rstd, g.y, b.y);
      o.z = __builtin_fmaf(v[i].z * rstd, g.z, b.z);
      o.w = __builtin_fmaf(v[i].w * rstd, g.w, b.w);
      reinterpret_cast<float4*>(out)[lane + 64 * i] = o;
    }
}

// word[id] + position[t] + token_type[tt] -> LayerNorm; also writes the key mask as floats (1 / 0).  An id outside its
// table sets a status bit and reads row 0.  tt == null: type 0; mask == null: every token valid.
__global__ void __launch_bounds__(256)
fe_embed_ln_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tts, const int64_t* __restrict__ mask,
                   const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int N, int T, int C, int vocab,
                   int type_vocab, float* __restrict__ out, float* __restrict__ maskf, int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  int64_t id = ids[n], tt = tts ? tts[n] : 0;
  int bits = 0;
  if (id < 0 || id >= vocab) { bits |= WETTS_STATUS_TOKEN_ID_RANGE; id = 0; }
  if (tt < 0 || tt >= type_vocab) { bits |= WETTS_STATUS_TYPE_ID_RANGE; tt = 0; }
  if (lane == 0) {
    if (bits && status) atomicOr(status, bits);
    maskf[n] = (mask == nullptr || mask[n] != 0) ? 1.f : 0.f;
  }
  const float4* w = reinterpret_cast<const float4*>(word + id * C);
  const float4* p = reinterpret_cast<const float4*>(pos + (int64_t)(n % T) * C);
  const float4* y = reinterpret_cast<const float4*>(type + tt * C);
  float4 v[kFeRowV];
#pragma unroll
  for (int i = 0; i < kFeRowV; ++i)
    if (lane + 64 * i < (C >> 2)) {
      const float4 a = w[lane + 64 * i], b = p[lane + 64 * i], c = y[lane + 64 * i];
      v[i].x = (a.x + b.x) + c.x; v[i].y = (a.y + b.y) + c.y; v[i].z = (a.z + b.z) + c.z; v[i].w = (a.w + b.w) + c.w;
    }
  fe_layer_norm_row(v, C, gamma, beta, eps, out + (int64_t)n * C, lane);
}

// out = LayerNorm(x [+ res]); out may be x
__global__ void __launch_bounds__(256)
fe_add_ln_kernel(const float* x, const float* res, const float* __restrict__ gamma, const float* __restrict__ beta,
                 float eps, int N, int C, float* out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float4* xr = reinterpret_cast<const float4*>(x + (int64_t)n * C);
  const float4* rr = res ? reinterpret_cast<const float4*>(res + (int64_t)n * C) : nullptr;
  float4 v[kFeRowV];
#pragma unroll
  for (int i = 0; i < kFeRowV; ++i)
    if (lane + 64 * i < (C >> 2)) {
      v[i] = xr[lane + 64 * i];
      if (rr) {
        const float4 r = rr[lane + 64 * i];
        v[i].x += r.x; v[i].y += r.y; v[i].z += r.z; v[i].w += r.w;
      }
    }
  fe_layer_norm_row(v, C, gamma, beta, eps, out + (int64_t)n * C, lane);
}

// ---------------------------------------------------------------------------------------------
// Linear: Y[N][M] = X[N][K] * W[M][K]^T + bias, then the epilogue; f32 MFMA 32x32x2, A = 32 weight rows, B = 32 tokens.
// At serving shapes (N of a few dozen tokens) the launch is M / 32 blocks that stream the weights once: what it needs is
// bytes in flight, not matrix throughput.  So the 32 x 32 tile of conv_small.hip with the K range split over the block's
// waves: a block is 8 waves and owns 32 output channels of 64 token columns (two accumulator tiles; the second is
// skipped where the launch has no column for it).  K is cut into steps of 8; wave w runs the steps w, w + 8, .. --
// one step of the 8 waves is one 256-byte run of every weight row -- with a ring of kFeRing steps in flight per wave.
// No LDS in the K loop: lane (r, half) reads the float4 k = 8 s + 4 half .. + 3 of weight row r and of token r, and the
// four MFMAs of a step pair equal k on both sides.
// The 8 partial tiles meet in LDS and are added in wave order, ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)): the k order of a
// column is fixed by K alone, so a token's result does not depend on N or on its neighbours.
// M % 4 == 0 and K % 8 == 0 (the launcher checks); rows / columns past M / N are read clamped and not stored.
enum { FE_EPI_BIAS = 0, FE_EPI_GELU = 1, FE_EPI_RELU = 2, FE_EPI_RES = 3 };

template <int EPI>
__global__ void __launch_bounds__(64 * kFeKG)
fe_linear_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                 const float* __restrict__ res, float* __restrict__ Y, int N, int K, int M) {
  __shared__ float part[kFeKG][2][16][64];
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * kFeNT;
  const bool two = n0 + 32 < N;  // block-uniform: the second column tile has a token
  const int S = K >> 3;

  const int mr = min(m0 + l31, M - 1), c0 = min(n0 + l31, N - 1), c1 = min(n0 + 32 + l31, N - 1);
  const float* wr = W + (int64_t)mr * K + 4 * half;
  const float* x0 = X + (int64_t)c0 * K + 4 * half;
  const float* x1 = X + (int64_t)c1 * K + 4 * half;

  f32x16f acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

  float4 ra[kFeRing], rb0[kFeRing], rb1[kFeRing];
#pragma unroll
  for (int i = 0; i < kFeRing; ++i) {
    const int s = w + kFeKG * i;
    if (s < S) {
      ra[i] = *reinterpret_cast<const float4*>(wr + 8 * s);
      rb0[i] = *reinterpret_cast<const float4*>(x0 + 8 * s);
      if (two) rb1[i] = *reinterpret_cast<const float4*>(x1 + 8 * s);
    }
  }
  for (int sb = w; sb < S; sb += kFeKG * kFeRing) {
#pragma unroll
    for (int i = 0; i < kFeRing; ++i) {
      const int s = sb + kFeKG * i;
      if (s < S) {
        const float4 a = ra[i], b0 = rb0[i];
        float4 b1 = b0;
        if (two) b1 = rb1[i];
        const int sn = s + kFeKG * kFeRing;
        if (sn < S) {
          ra[i] = *reinterpret_cast<const float4*>(wr + 8 * sn);
          rb0[i] = *reinterpret_cast<const float4*>(x0 + 8 * sn);
          if (two) rb1[i] = *reinterpret_cast<const float4*>(x1 + 8 * sn);
        }
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
        if (two) {
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
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
  // wave w: column tile w / 4, the registers 4 g .. 4 g + 3 (g = w % 4) = channels m0 + 8 g + 4 half + {0..3} of column l31
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
  const float4 b = *reinterpret_cast<const float4*>(bias + m);
  v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  if (EPI == FE_EPI_GELU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = 0.5f * v[i] * (1.f + erff(v[i] * 0.70710678118654752f));  // exact erf form
  } else if (EPI == FE_EPI_RELU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
  } else if (EPI == FE_EPI_RES) {
    const float4 r = *reinterpret_cast<const float4*>(res + (int64_t)col * M + m);
    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
  }
  float4 o;
  o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
  *reinterpret_cast<float4*>(Y + (int64_t)col * M + m) = o;
}

// ---------------------------------------------------------------------------------------------
// Key-masked attention on the packed projection qkv [N][3 d] (q | k | v, head h at h * dk) -> ctx [N][d].
// A block of four waves serves 16 queries of one (utterance, head), four per wave.  Two passes over the keys in chunks
// of 64 staged in LDS: (1) scores: lane j holds key j of the chunk and forms its dot products with the wave's four
// queries (q as [d][4], one broadcast 16-byte read per d), kept in LDS as [key][4]; then the maximum over the VALID
// keys, p = exp(s - max) (exactly 0 for a masked key) and the sum (lane l adds the keys l, l + 64, .. in ascending
// order, then the butterfly); (2) lane d (and d + 64) adds p[key] * v[key][d] over the keys in ascending order, and the
// quotient by the sum is stored.  A masked key adds +0 to every sum, so a row's bits do not depend on the padding behind
// it.  A query without any valid key gives zeros (the reference gives NaN there; no other row reads it).
constexpr int kFeQW = 4;

__global__ void __launch_bounds__(256)
fe_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ maskf, float* __restrict__ ctx, int T, int H,
                    int dk, float scale) {
  __shared__ float kv[64 * (kFeMaxDk + 1)];
  __shared__ float4 qs[4][kFeMaxDk];
  __shared__ float4 sc[4][kFeMaxT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int d = H * dk, ld = 3 * d, ldk = dk | 1;
  const float* base = qkv + (int64_t)b * T * ld + h * dk;
  const int q0 = qt * 16 + wave * kFeQW;

  const float* km = maskf + (int64_t)b * T;
  for (int i = lane; i < dk; i += 64) {
    float4 q;
    q.x = base[(int64_t)min(q0 + 0, T - 1) * ld + i];
    q.y = base[(int64_t)min(q0 + 1, T - 1) * ld + i];
    q.z = base[(int64_t)min(q0 + 2, T - 1) * ld + i];
    q.w = base[(int64_t)min(q0 + 3, T - 1) * ld + i];
    qs[wave][i] = q;
  }
  const int nch = (T + 63) >> 6;
  // pass 1: scores
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
      s.x *= scale; s.y *= scale; s.z *= scale; s.w *= scale;
      sc[wave][key] = s;
    }
  }
  // softmax over the valid keys (this wave's own rows of sc: no block barrier needed)
  float4 mx;
  mx.x = mx.y = mx.z = mx.w = -INFINITY;
  for (int key = lane; key < T; key += 64)
    if (km[key] != 0.f) {
      const float4 s = sc[wave][key];
      mx.x = fmaxf(mx.x, s.x); mx.y = fmaxf(mx.y, s.y); mx.z = fmaxf(mx.z, s.z); mx.w = fmaxf(mx.w, s.w);
    }
  mx.x = fe_wave_max(mx.x); mx.y = fe_wave_max(mx.y); mx.z = fe_wave_max(mx.z); mx.w = fe_wave_max(mx.w);
  const bool any = mx.x > -INFINITY;  // wave-uniform: the four queries share the keys
  float4 sum;
  sum.x = sum.y = sum.z = sum.w = 0.f;
  for (int key = lane; key < T; key += 64) {
    float4 p;
    p.x = p.y = p.z = p.w = 0.f;
    if (any && km[key] != 0.f) {
      const float4 s = sc[wave][key];
      p.x = expf(s.x - mx.x); p.y = expf(s.y - mx.y); p.z = expf(s.z - mx.z); p.w = expf(s.w - mx.w);
    }
    sc[wave][key] = p;
    sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w;
  }
  sum.x = fe_wave_sum(sum.x); sum.y = fe_wave_sum(sum.y); sum.z = fe_wave_sum(sum.z); sum.w = fe_wave_sum(sum.w);
  // pass 2: P V
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
  for (int i = 0; i < kFeQW; ++i) {
    const int q = q0 + i;
    if (q < T) {
      if (lane < dk) ob[(int64_t)q * d + lane] = any ? r0[i] / sm[i] : 0.f;
      if (hi) ob[(int64_t)q * d + lane + 64] = any ? r1[i] / sm[i] : 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Both classifiers and (softmax != 0) both softmaxes in one launch.  A block of 16 waves serves four tokens whose rows
// sit in LDS; the classes of BOTH heads form one list of P + R, taken four at a time by a wave (groups w, w + 16, ..) for
// all four tokens: a weight row is read once per block and the loads of four rows are in flight together (at B = 1 the
// launch is a few blocks that wait for their weights).  Per class and token, lane l adds its float4s l, l + 64, .. in
// ascending order as one fma chain and the butterfly adds the lanes: a logit depends on its own token and class alone.
// The logits go to the outputs; after a block barrier wave w < 4 turns token w's rows into probabilities in place:
// maximum, exp, the sum (lane l adds the classes l, l + 64, .., then the butterfly), the quotient.  A padded token's
// rows are zeros.
constexpr int kFeHeadWaves = 16, kFeHeadCU = 4;

__global__ void __launch_bounds__(64 * kFeHeadWaves)
fe_heads_kernel(const float* __restrict__ x, const float* __restrict__ maskf, const float* __restrict__ wp,
                const float* __restrict__ bp, const float* __restrict__ wr, const float* __restrict__ br, int N, int C, int P,
                int R, int softmax, float* phone, float* prosody) {
  __shared__ float4 xs[4][kFeMaxC / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 4, nv = C >> 2;
  for (int i = tid; i < 4 * nv; i += 64 * kFeHeadWaves) {
    const int tk = i / nv, e = i - tk * nv;
    xs[tk][e] = reinterpret_cast<const float4*>(x + (int64_t)min(n0 + tk, N - 1) * C)[e];
  }
  __syncthreads();
  const int total = P + R;
  for (int c0 = wave * kFeHeadCU; c0 < total; c0 += kFeHeadWaves * kFeHeadCU) {
    const float4* row[kFeHeadCU];
#pragma unroll
    for (int u = 0; u < kFeHeadCU; ++u) {
      const int c = min(c0 + u, total - 1);  // a class past the end repeats the last one and is not stored
      row[u] = reinterpret_cast<const float4*>(c < P ? wp + (int64_t)c * C : wr + (int64_t)(c - P) * C);
    }
    float a[kFeHeadCU][4];
#pragma unroll
    for (int u = 0; u < kFeHeadCU; ++u)
#pragma unroll
      for (int tk = 0; tk < 4; ++tk) a[u][tk] = 0.f;
    for (int e = lane; e < nv; e += 64) {
      float4 wv[kFeHeadCU];
#pragma unroll
      for (int u = 0; u < kFeHeadCU; ++u) wv[u] = row[u][e];
#pragma unroll
      for (int tk = 0; tk < 4; ++tk) {
        const float4 xv = xs[tk][e];
        // explicit fma chains: left to the compiler, the unrolled expressions contract differently (it packs them in
        // pairs), and a token's bits would depend on its place in the block
#pragma unroll
        for (int u = 0; u < kFeHeadCU; ++u)
          a[u][tk] = __builtin_fmaf(wv[u].w, xv.w, __builtin_fmaf(wv[u].z, xv.z, __builtin_fmaf(wv[u].y, xv.y, __builtin_fmaf(wv[u].x, xv.x, a[u][tk]))));
      }
    }
#pragma unroll
    for (int u = 0; u < kFeHeadCU; ++u) {
      const int c = c0 + u;
      if (c < total) {  // wave-uniform
        const bool ph = c < P;
        const float bv = ph ? bp[c] : br[c - P];
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) {
          const float z = fe_wave_sum(a[u][tk]) + bv;
          const int n = n0 + tk;
          if (lane == 0 && n < N) {
            const float o = maskf[n] != 0.f ? z : 0.f;
            if (ph) phone[(int64_t)n * P + c] = o; else prosody[(int64_t)n * R + (c - P)] = o;
          }
        }
      }
    }
  }
  if (!softmax) return;
  __syncthreads();  // the logits of this block's tokens, written by its own waves, are visible to them
  const int n = n0 + wave;
  if (wave >= 4 || n >= N || maskf[n] == 0.f) return;
#pragma unroll
  for (int hd = 0; hd < 2; ++hd) {
    float* z = hd == 0 ? phone + (int64_t)n * P : prosody + (int64_t)n * R;
    const int cnt = hd == 0 ? P : R;
    float mx = -INFINITY;
    for (int c = lane; c < cnt; c += 64) mx = fmaxf(mx, z[c]);
    mx = fe_wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < cnt; c += 64) {
      const float e = expf(z[c] - mx);
      z[c] = e;
      s += e;
    }
    s = fe_wave_sum(s);
    for (int c = lane; c < cnt; c += 64) z[c] = z[c] / s;
  }
}

// ---------------------------------------------------------------------------------------------
// The decisions of cli/frontend.py:70-81 for every token, one thread each: among the token's candidate classes
// cand[n][0 .. cand_len[n]) the FIRST one of the largest probability (list.index(max(..))), and the LOWEST prosody class
// of the largest probability (numpy's argmax).  A candidate outside [0, P) counts as -inf.
__global__ void __launch_bounds__(256)
fe_decide_kernel(const float* __restrict__ phone, const float* __restrict__ pros, const int32_t* __restrict__ cand,
                 const int32_t* __restrict__ cand_len, int N, int P, int R, int max_cand, int32_t* __restrict__ choice,
                 int32_t* __restrict__ prosody) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  int best = 0;
  float bv = -INFINITY;
  const int nc = min(cand_len[n], max_cand);
  for (int i = 0; i < nc; ++i) {
    const int c = cand[(int64_t)n * max_cand + i];
    const float v = (c >= 0 && c < P) ? phone[(int64_t)n * P + c] : -INFINITY;
    if (v > bv) { bv = v; best = i; }
  }
  choice[n] = best;
  int bp = 0;
  float pv = pros[(int64_t)n * R];
  for (int r = 1; r < R; ++r) {
    const float v = pros[(int64_t)n * R + r];
    if (v > pv) { pv = v; bp = r; }
  }
  prosody[n] = bp;
}

// ---------------------------------------------------------------------------------------------
// host side: the blob layout of a config, the handle, the launchers
struct FeTensor {
  std::string name;
  int64_t offset, numel, shape[4];
};

struct FeLayout {
  std::vector<FeTensor> tensors;
  int64_t total = 0;
  int64_t off(const std::string& name) const {
    for (const FeTensor& t : tensors)
      if (t.name == name) return t.offset;
    return -1;
  }
};

static const char* fe_config_error(const wetts_frontend_config_t* c) {
  if (!c) return "null config";
  if (c->vocab_size < 1 || c->type_vocab_size < 1 || c->max_position_embeddings < 1) return "an embedding table is empty";
  if (c->hidden_size < 8 || c->hidden_size > kFeMaxC || c->hidden_size % 8) return "hidden_size must be a multiple of 8 up to 1024";
  if (c->num_layers < 0 || c->num_layers > 64) return "num_layers out of range";
  if (c->num_heads < 1 || c->hidden_size % c->num_heads || c->hidden_size / c->num_heads > kFeMaxDk)
    return "num_heads must divide hidden_size into heads of at most 96";
  if (c->transform_heads < 1 || c->hidden_size % c->transform_heads || c->hidden_size / c->transform_heads > kFeMaxDk)
    return "transform_heads must divide hidden_size into heads of at most 96";
  if (c->intermediate_size < 8 || c->intermediate_size % 8) return "intermediate_size must be a multiple of 8";
  if (c->transform_ff < 8 || c->transform_ff % 8) return "transform_ff must be a multiple of 8";
  if (c->num_polyphones < 1 || c->num_prosody < 1) return "a classifier has no class";
  if (!(c->layer_norm_eps > 0.f)) return "layer_norm_eps must be positive";
  return nullptr;
}

// Every tensor starts at a multiple of 4 floats (16-byte rows); the q, k, v weights of a BERT layer, and their biases,
// follow each other without a gap (hidden_size % 8 == 0), so they are ONE packed [3 d][d] projection like in_proj_weight.
static FeLayout fe_layout(const wetts_frontend_config_t* c) {
  FeLayout l;
  auto add = [&](const std::string& name, int64_t s0, int64_t s1) {
    FeTensor t;
    t.name = name;
    t.offset = l.total;
    t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = 0; t.shape[3] = 0;
    t.numel = s0 * (s1 > 0 ? s1 : 1);
    l.total = align_up(l.total + t.numel, 4);
    l.tensors.push_back(t);
  };
  const int d = c->hidden_size;
  auto lin = [&](const std::string& name, int out, int in) {
    add(name + ".weight", out, in);
    add(name + ".bias", out, 0);
  };
  auto norm = [&](const std::string& name) {
    add(name + ".weight", d, 0);
    add(name + ".bias", d, 0);
  };
  add("bert.embeddings.word_embeddings.weight", c->vocab_size, d);
  add("bert.embeddings.position_embeddings.weight", c->max_position_embeddings, d);
  add("bert.embeddings.token_type_embeddings.weight", c->type_vocab_size, d);
  norm("bert.embeddings.LayerNorm");
  for (int i = 0; i < c->num_layers; ++i) {
    const std::string p = "bert.encoder.layer." + std::to_string(i) + ".";
    add(p + "attention.self.query.weight", d, d);
    add(p + "attention.self.key.weight", d, d);
    add(p + "attention.self.value.weight", d, d);
    add(p + "attention.self.query.bias", d, 0);
    add(p + "attention.self.key.bias", d, 0);
    add(p + "attention.self.value.bias", d, 0);
    lin(p + "attention.output.dense", d, d);
    norm(p + "attention.output.LayerNorm");
    lin(p + "intermediate.dense", c->intermediate_size, d);
    lin(p + "output.dense", d, c->intermediate_size);
    norm(p + "output.LayerNorm");
  }
  add("transform.self_attn.in_proj_weight", 3 * d, d);
  add("transform.self_attn.in_proj_bias", 3 * d, 0);
  lin("transform.self_attn.out_proj", d, d);
  lin("transform.linear1", c->transform_ff, d);
  lin("transform.linear2", d, c->transform_ff);
  norm("transform.norm1");
  norm("transform.norm2");
  lin("phone_classifier", c->num_polyphones, d);
  lin("prosody_classifier", c->num_prosody, d);
  return l;
}

int64_t fe_tensor_offset(const wetts_frontend_config_t* c, const char* name) {
  return name ? fe_layout(c).off(name) : fe_layout(c).total;
}

int32_t fe_launch_linear(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int K,
                                int M, int epi, hipStream_t s) {
  WETTS_REQUIRE(x && w && bias && y && N >= 1, "frontend linear: bad argument (N=%d)", N);
  WETTS_REQUIRE(K >= 8 && K % 8 == 0 && M >= 4 && M % 4 == 0, "frontend linear: K=%d must be a multiple of 8, M=%d of 4", K, M);
  WETTS_REQUIRE(epi >= FE_EPI_BIAS && epi <= FE_EPI_RES && (epi != FE_EPI_RES || res), "frontend linear: epilogue %d", epi);
  const int64_t ct = ((int64_t)N + kFeNT - 1) / kFeNT;
  WETTS_REQUIRE(ct <= 65535, "frontend linear: %d tokens exceed one launch", N);
  const dim3 grid((unsigned)cdiv(M, 32), (unsigned)ct), block(64 * kFeKG);
  switch (epi) {
    case FE_EPI_BIAS: hipLaunchKernelGGL(fe_linear_kernel<FE_EPI_BIAS>, grid, block, 0, s, x, w, bias, res, y, N, K, M); break;
    case FE_EPI_GELU: hipLaunchKernelGGL(fe_linear_kernel<FE_EPI_GELU>, grid, block, 0, s, x, w, bias, res, y, N, K, M); break;
    case FE_EPI_RELU: hipLaunchKernelGGL(fe_linear_kernel<FE_EPI_RELU>, grid, block, 0, s, x, w, bias, res, y, N, K, M); break;
    default: hipLaunchKernelGGL(fe_linear_kernel<FE_EPI_RES>, grid, block, 0, s, x, w, bias, res, y, N, K, M); break;
  }
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t fe_launch_add_ln(const float* x, const float* res, const float* gamma, const float* beta, float eps, int N,
                                int C, float* out, hipStream_t s) {
  WETTS_REQUIRE(x && gamma && beta && out && N >= 1, "frontend layer norm: bad argument (N=%d)", N);
  WETTS_REQUIRE(C >= 4 && C % 4 == 0 && C <= kFeMaxC, "frontend layer norm: C=%d must be a multiple of 4 up to %d", C, kFeMaxC);
  hipLaunchKernelGGL(fe_add_ln_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, s, x, res, gamma, beta, eps, N, C, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t fe_launch_attention(const float* qkv, const float* maskf, float* ctx, int B, int T, int H, int dk,
                                   hipStream_t s) {
  WETTS_REQUIRE(qkv && maskf && ctx, "frontend attention: null argument");
  WETTS_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kFeMaxT, "frontend attention: B=%d, T=%d (at most %d)", B, T, kFeMaxT);
  WETTS_REQUIRE(H >= 1 && H <= 65535 && dk >= 1 && dk <= kFeMaxDk, "frontend attention: %d heads of %d", H, dk);
  static_assert(sizeof(float) * (64 * (kFeMaxDk + 1) + 4 * 4 * kFeMaxDk + 4 * 4 * kFeMaxT) <= 64 * 1024,
                "frontend attention LDS");
  hipLaunchKernelGGL(fe_attention_kernel, dim3((unsigned)cdiv(T, 16), (unsigned)H, (unsigned)B), dim3(256), 0, s, qkv, maskf,
                     ctx, T, H, dk, 1.f / sqrtf((float)dk));
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t fe_launch_heads(const wetts_frontend* h, const float* x, const float* maskf, int N, int softmax, float* phone,
                               float* prosody, hipStream_t s) {
  WETTS_REQUIRE(x && maskf && phone && prosody && N >= 1, "frontend heads: bad argument (N=%d)", N);
  hipLaunchKernelGGL(fe_heads_kernel, dim3((unsigned)cdiv(N, 4)), dim3(64 * kFeHeadWaves), 0, s, x, maskf, h->wp, h->bp, h->wr, h->br, N,
                     h->cfg.hidden_size, h->cfg.num_polyphones, h->cfg.num_prosody, softmax, phone, prosody);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t fe_launch_embed(const wetts_frontend* h, const int64_t* ids, const int64_t* tts, const int64_t* mask, int B,
                               int T, float* out, float* maskf, int32_t* status, hipStream_t s) {
  WETTS_REQUIRE(ids && out && maskf, "frontend embeddings: null argument");
  WETTS_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T <= 0x7fffffff / 4, "frontend: B=%d or T=%d out of range", B, T);
  WETTS_REQUIRE(T <= h->cfg.max_position_embeddings, "frontend: T=%d exceeds the %d positions of the table", T,
                h->cfg.max_position_embeddings);
  const int N = B * T;
  hipLaunchKernelGGL(fe_embed_ln_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, s, ids, tts, mask, h->word, h->pos, h->type,
                     h->eg, h->eb, h->cfg.layer_norm_eps, N, T, h->cfg.hidden_size, h->cfg.vocab_size, h->cfg.type_vocab_size,
                     out, maskf, status);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// the regions of the workspace, in floats: h, h2, ctx [N][d], qkv [N][3d], ff [N][max ff], the key mask [N]
static void fe_regions(const wetts_frontend_config_t& c, int B, int T, int64_t off[7]) {
  const int64_t N = (int64_t)B * T, d = c.hidden_size;
  const int64_t ff = c.intermediate_size > c.transform_ff ? c.intermediate_size : c.transform_ff;
  const int64_t sizes[6] = {N * d, N * d, N * d, 3 * N * d, N * ff, N};
  off[0] = 0;
  for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + align_up(sizes[i], 64);
}

// one post-norm layer on h (in place); h2, ctx, qkv, ff are scratch.  prec != 0: the four Linears read 16-bit operands
// (frontend16.hip); everything between them is the f32 code of prec == 0.
int32_t fe_run_block(const FeBlock& k, int d, float* h, float* h2, float* ctx, float* qkv, float* ff,
                            const float* maskf, int B, int T, int prec, hipStream_t s) {
  const int N = B * T;
  auto linear = [&](const float* x, const float* w, const unsigned short* w16, const float* bias, const float* res, float* y,
                    int K, int M, int epi) -> int32_t {
    if (prec == 0) return fe_launch_linear(x, w, bias, res, y, N, K, M, epi, s);
    WETTS_REQUIRE(w16 != nullptr, "frontend: the 16-bit weights are not packed");
    return fe_launch_linear16(x, w16, bias, res, y, N, K, M, epi, prec, 0, s);
  };
  WETTS_TRY(linear(h, k.wqkv, k.wqkv16, k.bqkv, nullptr, qkv, d, 3 * d, FE_EPI_BIAS));
  WETTS_TRY(fe_launch_attention(qkv, maskf, ctx, B, T, k.heads, d / k.heads, s));
  WETTS_TRY(linear(ctx, k.wo, k.wo16, k.bo, h, h2, d, d, FE_EPI_RES));
  WETTS_TRY(fe_launch_add_ln(h2, nullptr, k.g1, k.b1, k.eps, N, d, h, s));
  WETTS_TRY(linear(h, k.w1, k.w116, k.bb1, nullptr, ff, d, k.ff, k.act));
  WETTS_TRY(linear(ff, k.w2, k.w216, k.bb2, h, h2, k.ff, d, FE_EPI_RES));
  return fe_launch_add_ln(h2, nullptr, k.g2, k.b2, k.eps, N, d, h, s);
}

int64_t fe_workspace_floats(const wetts_frontend* h, int B, int T) {
  int64_t off[7];
  fe_regions(h->cfg, B, T, off);
  return off[6];
}

int32_t fe_hidden(const wetts_frontend* h, const int64_t* ids, const int64_t* tts, const int64_t* mask, int B, int T,
                  void* workspace, int32_t* status, hipStream_t s, const char* what, const float** x, const float** maskf) {
  return fe_hidden_layers(h, (int)h->blocks.size(), ids, tts, mask, B, T, workspace, status, s, what, x, maskf);
}

int32_t fe_hidden_layers(const wetts_frontend* h, int layers, const int64_t* ids, const int64_t* tts, const int64_t* mask,
                         int B, int T, void* workspace, int32_t* status, hipStream_t s, const char* what, const float** x,
                         const float** maskf) {
  WETTS_REQUIRE(B >= 1 && T >= 1, "%s: B=%d and T=%d must be at least 1", what, B, T);
  WETTS_REQUIRE(T <= h->cfg.max_position_embeddings && T <= kFeMaxT, "%s: T=%d exceeds the %d positions", what, T,
                h->cfg.max_position_embeddings < kFeMaxT ? h->cfg.max_position_embeddings : kFeMaxT);
  WETTS_REQUIRE((int64_t)B * T <= 0x7fffffff / 4, "%s: %d x %d tokens exceed one call", what, B, T);
  int64_t off[7];
  fe_regions(h->cfg, B, T, off);
  float* ws = (float*)workspace;
  float *hb = ws + off[0], *h2 = ws + off[1], *ctx = ws + off[2], *qkv = ws + off[3], *ff = ws + off[4], *mf = ws + off[5];
  WETTS_TRY(fe_launch_embed(h, ids, tts, mask, B, T, hb, mf, status, s));
  for (int i = 0; i < layers && i < (int)h->blocks.size(); ++i)
    WETTS_TRY(fe_run_block(h->blocks[i], h->cfg.hidden_size, hb, h2, ctx, qkv, ff, mf, B, T, h->precision, s));
  *x = hb;
  *maskf = mf;
  return WETTS_OK;
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_frontend_blob_num_tensors(const wetts_frontend_config_t* cfg) {
  if (const char* e = fe_config_error(cfg)) {
    set_error("frontend config: %s", e);
    return -1;
  }
  return (int32_t)fe_layout(cfg).tensors.size();
}

int32_t wetts_frontend_blob_tensor_info(const wetts_frontend_config_t* cfg, int32_t index, char* name_buf, size_t name_buf_len,
                                        int64_t* offset, int64_t* numel, int64_t shape[4]) {
  const char* e = fe_config_error(cfg);
  WETTS_REQUIRE(e == nullptr, "frontend config: %s", e);
  const FeLayout L = fe_layout(cfg);
  WETTS_REQUIRE(index >= 0 && index < (int32_t)L.tensors.size(), "tensor index %d out of range", index);
  const FeTensor& t = L.tensors[index];
  WETTS_REQUIRE(name_buf && name_buf_len > t.name.size(), "name buffer too small");
  strcpy(name_buf, t.name.c_str());
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  return WETTS_OK;
}

int64_t wetts_frontend_blob_numel(const wetts_frontend_config_t* cfg) {
  if (const char* e = fe_config_error(cfg)) {
    set_error("frontend config: %s", e);
    return -1;
  }
  return fe_layout(cfg).total;
}

int32_t wetts_frontend_create(const wetts_frontend_config_t* cfg, const float* blob_dev, int64_t blob_numel, void* stream,
                              wetts_frontend_t** out) {
  WETTS_REQUIRE(out != nullptr && blob_dev != nullptr, "null argument");
  const char* ce = fe_config_error(cfg);
  WETTS_REQUIRE(ce == nullptr, "frontend config: %s", ce);
  const FeLayout L = fe_layout(cfg);
  WETTS_REQUIRE(blob_numel == L.total, "blob has %lld floats, the frontend layout needs %lld", (long long)blob_numel,
                (long long)L.total);
  wetts_frontend* h = new wetts_frontend();
  h->cfg = *cfg;
  hipError_t e = hipMalloc((void**)&h->blob, (size_t)blob_numel * sizeof(float));
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->blob, blob_dev, (size_t)blob_numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    set_error("wetts_frontend_create: %s", hipGetErrorString(e));
    if (h->blob) (void)hipFree(h->blob);
    delete h;
    return WETTS_E_HIP;
  }
  auto at = [&](const std::string& name) { return h->blob + L.off(name); };
  h->word = at("bert.embeddings.word_embeddings.weight");
  h->pos = at("bert.embeddings.position_embeddings.weight");
  h->type = at("bert.embeddings.token_type_embeddings.weight");
  h->eg = at("bert.embeddings.LayerNorm.weight");
  h->eb = at("bert.embeddings.LayerNorm.bias");
  for (int i = 0; i < cfg->num_layers; ++i) {
    const std::string p = "bert.encoder.layer." + std::to_string(i) + ".";
    FeBlock k;
    k.wqkv = at(p + "attention.self.query.weight");
    k.bqkv = at(p + "attention.self.query.bias");
    k.wo = at(p + "attention.output.dense.weight");
    k.bo = at(p + "attention.output.dense.bias");
    k.g1 = at(p + "attention.output.LayerNorm.weight");
    k.b1 = at(p + "attention.output.LayerNorm.bias");
    k.w1 = at(p + "intermediate.dense.weight");
    k.bb1 = at(p + "intermediate.dense.bias");
    k.w2 = at(p + "output.dense.weight");
    k.bb2 = at(p + "output.dense.bias");
    k.g2 = at(p + "output.LayerNorm.weight");
    k.b2 = at(p + "output.LayerNorm.bias");
    k.heads = cfg->num_heads;
    k.ff = cfg->intermediate_size;
    k.act = FE_EPI_GELU;
    k.eps = cfg->layer_norm_eps;
    h->blocks.push_back(k);
  }
  FeBlock k;
  k.wqkv = at("transform.self_attn.in_proj_weight");
  k.bqkv = at("transform.self_attn.in_proj_bias");
  k.wo = at("transform.self_attn.out_proj.weight");
  k.bo = at("transform.self_attn.out_proj.bias");
  k.g1 = at("transform.norm1.weight");
  k.b1 = at("transform.norm1.bias");
  k.w1 = at("transform.linear1.weight");
  k.bb1 = at("transform.linear1.bias");
  k.w2 = at("transform.linear2.weight");
  k.bb2 = at("transform.linear2.bias");
  k.g2 = at("transform.norm2.weight");
  k.b2 = at("transform.norm2.bias");
  k.heads = cfg->transform_heads;
  k.ff = cfg->transform_ff;
  k.act = FE_EPI_RELU;
  k.eps = 1e-5f;  // nn.TransformerEncoderLayer's default
  h->blocks.push_back(k);
  h->wp = at("phone_classifier.weight");
  h->bp = at("phone_classifier.bias");
  h->wr = at("prosody_classifier.weight");
  h->br = at("prosody_classifier.bias");
  *out = h;
  return WETTS_OK;
}

void wetts_frontend_destroy(wetts_frontend_t* h) {
  if (!h) return;
  if (h->blob) (void)hipFree(h->blob);
  if (h->w16) (void)hipFree(h->w16);
  delete h;
}

int64_t wetts_frontend_workspace_bytes(const wetts_frontend_t* h, int32_t B, int32_t T) {
  if (!h || B < 1 || T < 1 || (int64_t)B * T > 0x7fffffff / 4) {
    set_error("frontend_workspace_bytes: bad argument (B=%d T=%d)", B, T);
    return -1;
  }
  int64_t off[7];
  fe_regions(h->cfg, B, T, off);
  return off[6] * (int64_t)sizeof(float);
}

int32_t wetts_frontend_forward(const wetts_frontend_t* h, const int64_t* input_ids, const int64_t* token_type_ids,
                               const int64_t* attention_mask, int32_t B, int32_t T, int32_t softmax, float* phone_out,
                               float* prosody_out, void* workspace, int32_t* status, void* stream) {
  WETTS_REQUIRE(h && input_ids && phone_out && prosody_out && workspace, "null argument");
  hipStream_t s = (hipStream_t)stream;
  const float *hb, *maskf;
  WETTS_TRY(fe_hidden(h, input_ids, token_type_ids, attention_mask, B, T, workspace, status, s, "frontend_forward", &hb, &maskf));
  return fe_launch_heads(h, hb, maskf, B * T, softmax, phone_out, prosody_out, s);
}

int32_t wetts_frontend_embed(const wetts_frontend_t* h, const int64_t* input_ids, const int64_t* token_type_ids,
                             const int64_t* attention_mask, int32_t B, int32_t T, float* out, float* mask_out, int32_t* status,
                             void* stream) {
  WETTS_REQUIRE(h, "null argument");
  return fe_launch_embed(h, input_ids, token_type_ids, attention_mask, B, T, out, mask_out, status, (hipStream_t)stream);
}

int32_t wetts_frontend_linear(const float* x, const float* weight, const float* bias, const float* residual, int32_t N,
                              int32_t K, int32_t M, int32_t epilogue, float* out, void* stream) {
  return fe_launch_linear(x, weight, bias, residual, out, N, K, M, epilogue, (hipStream_t)stream);
}

int32_t wetts_frontend_add_layer_norm(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                                      int32_t N, int32_t C, float* out, void* stream) {
  return fe_launch_add_ln(x, residual, gamma, beta, eps, N, C, out, (hipStream_t)stream);
}

int32_t wetts_frontend_attention(const float* qkv, const float* key_mask, int32_t B, int32_t T, int32_t heads, int32_t dk,
                                 float* out, void* stream) {
  return fe_launch_attention(qkv, key_mask, out, B, T, heads, dk, (hipStream_t)stream);
}

int32_t wetts_frontend_heads(const wetts_frontend_t* h, const float* x, const float* key_mask, int32_t N, int32_t softmax,
                             float* phone_out, float* prosody_out, void* stream) {
  WETTS_REQUIRE(h, "null argument");
  return fe_launch_heads(h, x, key_mask, N, softmax, phone_out, prosody_out, (hipStream_t)stream);
}

int32_t wetts_frontend_layer(const wetts_frontend_t* h, int32_t layer, float* x, const float* key_mask, int32_t B, int32_t T,
                             void* workspace, void* stream) {
  WETTS_REQUIRE(h && x && key_mask && workspace, "null argument");
  WETTS_REQUIRE(layer >= 0 && layer < (int32_t)h->blocks.size(), "frontend_layer: layer %d is not one of 0..%d", layer,
                (int)h->blocks.size() - 1);
  WETTS_REQUIRE(B >= 1 && T >= 1 && T <= kFeMaxT && (int64_t)B * T <= 0x7fffffff / 4, "frontend_layer: B=%d, T=%d", B, T);
  int64_t off[7];
  fe_regions(h->cfg, B, T, off);
  float* ws = (float*)workspace;
  return fe_run_block(h->blocks[layer], h->cfg.hidden_size, x, ws + off[1], ws + off[2], ws + off[3], ws + off[4], key_mask, B,
                      T, h->precision, (hipStream_t)stream);
}

int32_t wetts_frontend_decide(const float* phone_prob, const float* prosody_prob, const int32_t* cand, const int32_t* cand_len,
                              int32_t N, int32_t P, int32_t R, int32_t max_cand, int32_t* choice, int32_t* prosody,
                              void* stream) {
  WETTS_REQUIRE(phone_prob && prosody_prob && cand && cand_len && choice && prosody, "null argument");
  WETTS_REQUIRE(N >= 1 && P >= 1 && R >= 1 && max_cand >= 1, "frontend_decide: N=%d P=%d R=%d max_cand=%d", N, P, R, max_cand);
  hipLaunchKernelGGL(fe_decide_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, phone_prob,
                     prosody_prob, cand, cand_len, N, P, R, max_cand, choice, prosody);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // extern "C"
