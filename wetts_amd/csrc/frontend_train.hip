// Training the text frontend (frontend/train.py:43-101, :184-190): the gradient of train.py:71-84's loss with respect to
// the parameters the reference trains (model.py:30-31 freezes BERT: `transform` and the two classifiers are left), and
// torch.optim.AdamW's single-tensor step on them.  f32, wave64, token-major, on the caller's stream; dropout-free.
//
//   fe_ce_bwd_kernel      dlogits [N][P + R] = w_head / n_head (softmax - onehot) at scored tokens, zeros elsewhere
//   fe_bgemm_kernel       C[I][J] = sum_k A(i, k) B(k, j) on f32 MFMA 32x32x2, both operands staged through LDS k-major:
//                         dgrad (dX = dY W, contraction over the weight's rows, A contiguous along k) and wgrad
//                         (dW = dY^T X, contraction over tokens, A contiguous along i); epilogue: ReLU mask or + residual
//   fe_split_sum_kernel   the token splits of a wgrad, added pairwise in a fixed order
//   fe_colsum_*           bias / LayerNorm gamma, beta gradients: two-stage column sums in a fixed order
//   fe_ln_bwd_kernel      LayerNorm backward of a row, one wave per token as the forward kernel
//   fe_attn_bwd_q_kernel  a wave per query: P from q, k and the mask, dP = dO V^T, delta = rowsum(dO o O),
//                         dS = P o (dP - delta), dQ; P and dS go to the workspace
//   fe_attn_bwd_kv_kernel a wave per key: dV = P^T dO, dK = scale dS^T Q over the queries in ascending order
//   fe_adamw_kernel       one launch over the trainable span, float4 per thread
//
// Determinism.  No atomics.  A GEMM element accumulates its k sequence in ascending order inside one wave (in blocks of
// 16 and 256 k, see fe_bgemm_kernel); token splits are added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)); a column sum adds rows r, r + 4, .. of a 64-row chunk, the four
// row groups as (0 + 1) + (2 + 3), the chunks in ascending order.  All of it is fixed by the shapes.  A padded token has
// dlogits = 0 exactly, every product with it is a zero, so what the forward pass left at padded rows (finite, from the
// pad ids) changes no bit; rows and columns past a tile's end are staged as zeros, never read.
//
// The attention backward follows the forward kernel's VALU schedule (no MFMA); tools/bench_frontend_train.py reports its
// share of the backward pass.
#include "frontend_dev.h"

#include <math.h>

#include <algorithm>

namespace wetts {

constexpr int kEpiBias = 0, kEpiRelu = 2, kEpiRes = 3;  // FE_EPI_* of frontend.hip
constexpr int64_t kFtIgnore = -100;

// ---------------------------------------------------------------------------------------------
// Cross-entropy backward (the derivative of train.py:73-84): one wave per token and both heads.  counts: the 22 counts
// of the scoring launch, [0] / [2] the scored labels of the phone / prosody head.  An empty head gives zeros.
__global__ void __launch_bounds__(256)
fe_ce_bwd_kernel(const float* __restrict__ zp, const float* __restrict__ zr, const float* __restrict__ maskf,
                 const int64_t* __restrict__ lab_p, const int64_t* __restrict__ lab_r, const int64_t* __restrict__ counts,
                 int N, int P, int R, float wp, float wr, float* __restrict__ dl) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const bool on = maskf[n] != 0.f;
#pragma unroll
  for (int hd = 0; hd < 2; ++hd) {
    const int M = hd == 0 ? P : R;
    const float* z = hd == 0 ? zp + (int64_t)n * P : zr + (int64_t)n * R;
    float* o = dl + (int64_t)n * (P + R) + (hd == 0 ? 0 : P);
    const int64_t* labels = hd == 0 ? lab_p : lab_r;
    const int64_t lab = labels ? labels[n] : kFtIgnore;
    const int64_t cnt = counts[hd == 0 ? 0 : 2];
    if (!on || lab < 0 || lab >= M || cnt <= 0) {  // wave-uniform
      for (int c = lane; c < M; c += 64) o[c] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int c = lane; c < M; c += 64) mx = fmaxf(mx, z[c]);
    mx = fe_wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < M; c += 64) s += expf(z[c] - mx);
    s = fe_wave_sum(s);
    const float sc = (hd == 0 ? wp : wr) / (float)cnt;
    for (int c = lane; c < M; c += 64) o[c] = sc * (expf(z[c] - mx) / s - (c == (int)lab ? 1.f : 0.f));
  }
}

// ---------------------------------------------------------------------------------------------
// The backward GEMM.  C[i][j] = sum over k in this split of A(i, k) B(k, j); A(i, k) = A[i * sai + k * sak],
// B(k, j) = B[k * ldb + j].  A block of 4 waves owns 64 x 64 outputs, wave (wi, wj) the 32 x 32 tile (32 wi, 32 wj); the
// contraction runs in steps of 16 staged in LDS k-major ([k][i] and [k][j]): lane (l31, half) reads As[2 s + half][l31],
// Bs[2 s + half][l31] for the MFMA s of a step.  A_ICONTIG: A is contiguous along i (wgrad: dY^T) -- otherwise along k
// (dgrad: dY's rows), which is the operand "staged transposed": a lane group of 32 then writes 16 k of 2 rows.  The row
// stride is 66 floats: 4-byte LDS accesses are served in two groups of 32 lanes over 32 banks, a read's group is 32
// consecutive floats of one row and a transposed write's group lands on the banks 2 k + i, all distinct -- no conflict
// in either direction (at stride 96 the transposed write was 16-way).  Elements outside I, J or the split's k range
// are staged as zeros.  blockIdx.z is the split; with more than one the tiles go to `part` [split][I][J] without an
// epilogue.  48 accumulator registers of at most 128, 8.25 KB of LDS: four blocks a CU.
constexpr int kBgK = 16, kBgLd = 66;
enum { BG_NONE = 0, BG_RELU_MASK = 1, BG_ADD = 2 };

template <bool A_ICONTIG>
__global__ void __launch_bounds__(256)
fe_bgemm_kernel(const float* __restrict__ A, int64_t sai, int64_t sak, const float* __restrict__ Bm, int64_t ldb, int I,
                int J, int K, int kchunk, int epi, const float* __restrict__ aux, int64_t ldaux, float* __restrict__ Cm,
                int64_t ldc, float* __restrict__ part) {
  __shared__ float As[kBgK][kBgLd];
  __shared__ float Bs[kBgK][kBgLd];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int w = tid >> 6, wi = w >> 1, wj = w & 1;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int kbeg = blockIdx.z * kchunk, kend = min(K, kbeg + kchunk);
  // three levels of partial sums: a step's 16 k in `a1`, 16 steps (256 k) in `a2`, those in `acc` -- the rounding error of
  // an element grows with 16 + 16 + K / 256 terms, not with K
  f32x16f acc, a2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; a2[r] = 0.f; }
  int step = 0;
  for (int kb = kbeg; kb < kend; kb += kBgK, ++step) {
    if (step == 16) {  // block-uniform
      step = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[r] += a2[r]; a2[r] = 0.f; }
    }
    f32x16f a1;
#pragma unroll
    for (int r = 0; r < 16; ++r) a1[r] = 0.f;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      {  // B: thread (kk = tid / 64 + 4 r, jj = tid % 64)
        const int kk = (tid >> 6) + 4 * r, jj = tid & 63;
        const int k = kb + kk, j = j0 + jj;
        Bs[kk][jj] = (k < kend && j < J) ? Bm[(int64_t)k * ldb + j] : 0.f;
      }
      if (A_ICONTIG) {
        const int kk = (tid >> 6) + 4 * r, ii = tid & 63;
        const int k = kb + kk, i = i0 + ii;
        As[kk][ii] = (k < kend && i < I) ? A[(int64_t)i * sai + (int64_t)k * sak] : 0.f;
      } else {
        const int kk = tid & 15, ii = (tid >> 4) + 16 * r;
        const int k = kb + kk, i = i0 + ii;
        As[kk][ii] = (k < kend && i < I) ? A[(int64_t)i * sai + (int64_t)k * sak] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kBgK / 2; ++s)
      a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + half][32 * wi + l31], Bs[2 * s + half][32 * wj + l31], a1, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) a2[r] += a1[r];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += a2[r];
  // register r: row 8 (r / 4) + 4 half + r % 4 of the wave's tile, column l31
  const int j = j0 + 32 * wj + l31;
  if (j >= J) return;
  const bool split = gridDim.z > 1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + 32 * wi + 8 * (r >> 2) + 4 * half + (r & 3);
    if (i >= I) continue;
    float v = acc[r];
    if (split) {
      part[((int64_t)blockIdx.z * I + i) * J + j] = v;
    } else {
      if (epi == BG_RELU_MASK) v = aux[(int64_t)i * ldaux + j] > 0.f ? v : 0.f;
      else if (epi == BG_ADD) v += aux[(int64_t)i * ldaux + j];
      Cm[(int64_t)i * ldc + j] = v;
    }
  }
}

// C[i][j] = the `ns` (2 .. 8) partial tiles of an element, added pairwise; a missing one counts as +0
__global__ void __launch_bounds__(256)
fe_split_sum_kernel(const float* __restrict__ part, int ns, int I, int J, float* __restrict__ Cm, int64_t ldc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, IJ = (int64_t)I * J;
  if (e >= IJ) return;
  float p[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) p[s] = s < ns ? part[s * IJ + e] : 0.f;
  Cm[(e / J) * ldc + (e % J)] = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
}

// ---------------------------------------------------------------------------------------------
// Column sums over the tokens.  Stage 1: a block owns 64 columns of a 64-row chunk; thread (g = tid / 64, c = tid % 64)
// adds the rows g, g + 4, .. of the chunk in ascending order, the four groups meet as (0 + 1) + (2 + 3).  The summand is
// a[n][c], or with x / stats the LayerNorm-gamma term a[n][c] * (x[n][c] - mean[n]) * rstd[n].  Stage 2: a thread per
// column adds the chunks in ascending order.
__global__ void __launch_bounds__(256)
fe_colsum_part_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ x, const float* __restrict__ stats,
                      int N, int C, float* __restrict__ part) {
  __shared__ float sm[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 64, r1 = min(N, r0 + 64);
  float s = 0.f;
  if (c < C)
    for (int n = r0 + g; n < r1; n += 4) {
      float v = a[(int64_t)n * lda + c];
      if (x) v *= (x[(int64_t)n * C + c] - stats[2 * n]) * stats[2 * n + 1];
      s += v;
    }
  sm[g][threadIdx.x & 63] = s;
  __syncthreads();
  if (g == 0 && c < C) part[(int64_t)blockIdx.y * C + c] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

__global__ void __launch_bounds__(256)
fe_colsum_final_kernel(const float* __restrict__ part, int chunks, int C, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = part[c];
  for (int k = 1; k < chunks; ++k) s += part[(int64_t)k * C + c];
  out[c] = s;
}

// ---------------------------------------------------------------------------------------------
// LayerNorm backward of y = LayerNorm(x) gamma + beta for a token, one wave per token, the row in registers as in
// fe_layer_norm_row (the same two passes give the same mean and rstd; biased variance):
// g = dy gamma, dx = rstd (g - mean(g) - xhat mean(g xhat)).  Also writes stats[n] = (mean, rstd) for the gamma sums.
constexpr int kFtRowV = kFeMaxC / 256;

__global__ void __launch_bounds__(256)
fe_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma, float eps, int N,
                 int C, float* __restrict__ dx, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int nv = C >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + (int64_t)n * C);
  const float4* dr = reinterpret_cast<const float4*>(dy + (int64_t)n * C);
  float4 v[kFtRowV], g[kFtRowV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kFtRowV; ++i)
    if (lane + 64 * i < nv) {
      v[i] = xr[lane + 64 * i];
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  const float mean = fe_wave_sum(s) / (float)C;
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < kFtRowV; ++i)
    if (lane + 64 * i < nv) {
      v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
      s2 += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
  const float rstd = 1.f / sqrtf(fe_wave_sum(s2) / (float)C + eps);
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int i = 0; i < kFtRowV; ++i)
    if (lane + 64 * i < nv) {
      const float4 d = dr[lane + 64 * i], ga = reinterpret_cast<const float4*>(gamma)[lane + 64 * i];
      v[i].x *= rstd; v[i].y *= rstd; v[i].z *= rstd; v[i].w *= rstd;  // xhat
      g[i].x = d.x * ga.x; g[i].y = d.y * ga.y; g[i].z = d.z * ga.z; g[i].w = d.w * ga.w;
      sg += (g[i].x + g[i].y) + (g[i].z + g[i].w);
      sgx += (g[i].x * v[i].x + g[i].y * v[i].y) + (g[i].z * v[i].z + g[i].w * v[i].w);
    }
  const float m1 = fe_wave_sum(sg) / (float)C, m2 = fe_wave_sum(sgx) / (float)C;
#pragma unroll
  for (int i = 0; i < kFtRowV; ++i)
    if (lane + 64 * i < nv) {
      float4 o;
      o.x = rstd * ((g[i].x - m1) - v[i].x * m2);
      o.y = rstd * ((g[i].y - m1) - v[i].y * m2);
      o.z = rstd * ((g[i].z - m1) - v[i].z * m2);
      o.w = rstd * ((g[i].w - m1) - v[i].w * m2);
      reinterpret_cast<float4*>(dx + (int64_t)n * C)[lane + 64 * i] = o;
    }
  if (lane == 0) {
    stats[2 * n] = mean;
    stats[2 * n + 1] = rstd;
  }
}

// ---------------------------------------------------------------------------------------------
// Attention backward on the packed projection qkv [N][3 d], the context ctx [N][d] and its gradient dctx [N][d].
// Query kernel: a block of four waves, one query each, of one (utterance, head).  Lane l holds the keys l, l + 64, ..:
// s = scale q . k, dp = dO . v; P = exp(s - max) / sum over the valid keys (+0 exactly at a masked key);
// delta = sum_e dO[e] O[e]; dS = P (dp - delta), 0 exactly at a masked key.  P and dS rows go to the workspace
// ([B][H][T][T] each); then lane e adds dQ[e] = scale sum_j dS[j] k[j][e] over the keys in ascending order.
// Only wave-private LDS: no block barrier.
constexpr int kFtKeys = kFeMaxT / 64;

__global__ void __launch_bounds__(256)
fe_attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ maskf, const float* __restrict__ ctx,
                     const float* __restrict__ dctx, int T, int H, int dk, float scale, float* __restrict__ Pw,
                     float* __restrict__ dSw, float* __restrict__ dqkv) {
  __shared__ float qs[4][kFeMaxDk], dos[4][kFeMaxDk], sds[4][kFeMaxT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, b = blockIdx.z;
  const int i = blockIdx.x * 4 + wave;
  if (i >= T) return;  // wave-uniform
  const int d = H * dk, ld = 3 * d;
  const float* base = qkv + (int64_t)b * T * ld + h * dk;
  const float* km = maskf + (int64_t)b * T;
  const int64_t row = (int64_t)b * T + i;
  float dl = 0.f;
  for (int e = lane; e < dk; e += 64) {
    const float dv = dctx[row * d + h * dk + e];
    qs[wave][e] = base[(int64_t)i * ld + e];
    dos[wave][e] = dv;
    dl = __builtin_fmaf(dv, ctx[row * d + h * dk + e], dl);
  }
  const float delta = fe_wave_sum(dl);
  __builtin_amdgcn_wave_barrier();
  float sv[kFtKeys], dp[kFtKeys];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < kFtKeys; ++c) {
    sv[c] = 0.f; dp[c] = 0.f;
    const int j = c * 64 + lane;
    if (j < T) {
      const float* kr = base + (int64_t)j * ld + d;
      const float* vr = kr + d;
      float a = 0.f, g = 0.f;
      for (int e = 0; e < dk; ++e) {
        a = __builtin_fmaf(qs[wave][e], kr[e], a);
        g = __builtin_fmaf(dos[wave][e], vr[e], g);
      }
      sv[c] = a * scale;
      dp[c] = g;
      if (km[j] != 0.f) mx = fmaxf(mx, sv[c]);
    }
  }
  mx = fe_wave_max(mx);
  const bool any = mx > -INFINITY;
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < kFtKeys; ++c) {
    const int j = c * 64 + lane;
    float p = 0.f;
    if (j < T && any && km[j] != 0.f) p = expf(sv[c] - mx);
    sv[c] = p;
    sum += p;
  }
  sum = fe_wave_sum(sum);
  float* pw = Pw + (((int64_t)b * H + h) * T + i) * T;
  float* dw = dSw + (((int64_t)b * H + h) * T + i) * T;
#pragma unroll
  for (int c = 0; c < kFtKeys; ++c) {
    const int j = c * 64 + lane;
    if (j < T) {
      const bool keep = any && km[j] != 0.f;
      const float p = keep ? sv[c] / sum : 0.f;
      const float ds = keep ? p * (dp[c] - delta) : 0.f;
      pw[j] = p;
      dw[j] = ds;
      sds[wave][j] = ds;
    }
  }
  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < dk; e += 64) {
    float a = 0.f;
    for (int j = 0; j < T; ++j) a = __builtin_fmaf(sds[wave][j], base[(int64_t)j * ld + d + e], a);
    dqkv[row * ld + h * dk + e] = a * scale;
  }
}

// Key kernel: a wave per key j of one (utterance, head); lane e adds over the queries i in ascending order
// dV[j][e] = sum_i P[i][j] dO[i][e] and dK[j][e] = scale sum_i dS[i][j] q[i][e].  A masked key's column of P and dS is
// zeros, so it receives exactly zero.
__global__ void __launch_bounds__(256)
fe_attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx, const float* __restrict__ Pw,
                      const float* __restrict__ dSw, int T, int H, int dk, float scale, float* __restrict__ dqkv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, b = blockIdx.z;
  const int j = blockIdx.x * 4 + wave;
  if (j >= T) return;
  const int d = H * dk, ld = 3 * d;
  const float* pw = Pw + ((int64_t)b * H + h) * T * T + j;
  const float* dw = dSw + ((int64_t)b * H + h) * T * T + j;
  for (int e = lane; e < dk; e += 64) {
    const float* qb = qkv + (int64_t)b * T * ld + h * dk + e;
    const float* ob = dctx + (int64_t)b * T * d + h * dk + e;
    float av = 0.f, ak = 0.f;
    for (int i = 0; i < T; ++i) {
      av = __builtin_fmaf(pw[(int64_t)i * T], ob[(int64_t)i * d], av);
      ak = __builtin_fmaf(dw[(int64_t)i * T], qb[(int64_t)i * ld], ak);
    }
    float* o = dqkv + ((int64_t)b * T + j) * ld + h * dk + e;
    o[d] = ak * scale;
    o[2 * d] = av;
  }
}

// ---------------------------------------------------------------------------------------------
// torch.optim.AdamW's single-tensor step (torch/optim/adamw.py, no amsgrad, not maximize) on n4 float4s:
//   p *= 1 - lr wd;  m += (g - m)(1 - beta1);  v = v beta2 + (1 - beta2) g g;
//   p -= step_size m / (sqrt(v) / sqrt(bias_correction2) + eps),  step_size = lr / bias_correction1.
// The scalars are formed on the host in double.  Alignment padding (g = p = m = v = 0) stays 0.
__device__ __forceinline__ void fe_adamw_one(float& p, float g, float& m, float& v, float decay, float w1, float b2, float w2,
                                             float bc2s, float eps, float step) {
  p *= decay;
  m = __builtin_fmaf(g - m, w1, m);
  v = __builtin_fmaf(w2 * g, g, v * b2);
  const float den = sqrtf(v) / bc2s + eps;
  p = p - step * (m / den);
}

__global__ void __launch_bounds__(256)
fe_adamw_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m, float4* __restrict__ v,
                int64_t n4, float decay, float w1, float b2, float w2, float bc2s, float eps, float step) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  float4 pp = p[e], mm = m[e], vv = v[e];
  const float4 gg = g[e];
  fe_adamw_one(pp.x, gg.x, mm.x, vv.x, decay, w1, b2, w2, bc2s, eps, step);
  fe_adamw_one(pp.y, gg.y, mm.y, vv.y, decay, w1, b2, w2, bc2s, eps, step);
  fe_adamw_one(pp.z, gg.z, mm.z, vv.z, decay, w1, b2, w2, bc2s, eps, step);
  fe_adamw_one(pp.w, gg.w, mm.w, vv.w, decay, w1, b2, w2, bc2s, eps, step);
  p[e] = pp; m[e] = mm; v[e] = vv;
}

// ---------------------------------------------------------------------------------------------
// launchers
constexpr int kFtMaxSplit = 8;

static int64_t ft_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int ft_splits(int K) { return std::min(kFtMaxSplit, cdiv(K, 64)); }
static int ft_kchunk(int K, int ns) { return (int)align_up((int64_t)cdiv(K, ns), kBgK); }

// floats of `part` a wgrad of [I][J] over N tokens needs
static int64_t ft_part_floats(int N, int64_t I, int64_t J) {
  const int ns = ft_splits(N);
  return ns > 1 ? ns * I * J : 0;
}

static int32_t ft_launch_bgemm(bool icontig, const float* A, int64_t sai, int64_t sak, const float* Bm, int64_t ldb, int I,
                               int J, int K, int ns, int epi, const float* aux, int64_t ldaux, float* Cm, int64_t ldc,
                               float* part, hipStream_t s) {
  WETTS_REQUIRE(A && Bm && Cm && I >= 1 && J >= 1 && K >= 1, "frontend backward gemm: bad argument (%d x %d x %d)", I, J, K);
  WETTS_REQUIRE(ns >= 1 && ns <= kFtMaxSplit && (ns == 1 || (part && epi == BG_NONE)), "frontend backward gemm: %d splits", ns);
  WETTS_REQUIRE(epi == BG_NONE || aux, "frontend backward gemm: epilogue %d without its operand", epi);
  WETTS_REQUIRE(cdiv(I, 64) <= 65535, "frontend backward gemm: %d rows exceed one launch", I);
  const int kchunk = ft_kchunk(K, ns);
  const dim3 grid((unsigned)cdiv(J, 64), (unsigned)cdiv(I, 64), (unsigned)ns), block(256);
  if (icontig)
    hipLaunchKernelGGL(fe_bgemm_kernel<true>, grid, block, 0, s, A, sai, sak, Bm, ldb, I, J, K, kchunk, epi, aux, ldaux, Cm, ldc, part);
  else
    hipLaunchKernelGGL(fe_bgemm_kernel<false>, grid, block, 0, s, A, sai, sak, Bm, ldb, I, J, K, kchunk, epi, aux, ldaux, Cm, ldc, part);
  WETTS_LAUNCH_CHECK();
  if (ns > 1) {
    hipLaunchKernelGGL(fe_split_sum_kernel, dim3((unsigned)ft_cdiv((int64_t)I * J, 256)), dim3(256), 0, s, (const float*)part, ns, I,
                       J, Cm, ldc);
    WETTS_LAUNCH_CHECK();
  }
  return WETTS_OK;
}

// dX [N][K] = dY [N][M] (row stride ldy) W [M][K], then the epilogue
static int32_t ft_dgrad(const float* dy, int64_t ldy, const float* w, int N, int M, int K, int epi, const float* aux, float* dx,
                        hipStream_t s) {
  return ft_launch_bgemm(false, dy, ldy, 1, w, K, N, K, M, 1, epi, aux, K, dx, K, nullptr, s);
}

// dW [M][K] = dY^T X over the N tokens; db [M] = column sums of dY (db may be null).  part: ft_part_floats(N, M, K);
// cpart: cdiv(N, 64) * M floats
static int32_t ft_colsum(const float* a, int64_t lda, const float* x, const float* stats, int N, int C, float* cpart, float* out,
                         hipStream_t s) {
  WETTS_REQUIRE(a && cpart && out && N >= 1 && C >= 1 && cdiv(N, 64) <= 65535, "frontend column sums: bad argument (N=%d C=%d)", N, C);
  hipLaunchKernelGGL(fe_colsum_part_kernel, dim3((unsigned)cdiv(C, 64), (unsigned)cdiv(N, 64)), dim3(256), 0, s, a, lda, x, stats,
                     N, C, cpart);
  WETTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(fe_colsum_final_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, s, (const float*)cpart, cdiv(N, 64), C, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t ft_wgrad(const float* dy, int64_t ldy, const float* x, int N, int M, int K, float* dw, float* db, float* part,
                        float* cpart, hipStream_t s) {
  WETTS_TRY(ft_launch_bgemm(true, dy, 1, ldy, x, K, M, K, N, ft_splits(N), BG_NONE, nullptr, 0, dw, K, part, s));
  if (db) WETTS_TRY(ft_colsum(dy, ldy, nullptr, nullptr, N, M, cpart, db, s));
  return WETTS_OK;
}

static int32_t ft_ln_bwd(const float* dy, const float* x, const float* gamma, float eps, int N, int C, float* dx, float* stats,
                         float* dgamma, float* dbeta, float* cpart, hipStream_t s) {
  WETTS_REQUIRE(dy && x && gamma && dx && stats && N >= 1, "frontend layer norm backward: bad argument (N=%d)", N);
  WETTS_REQUIRE(C >= 4 && C % 4 == 0 && C <= kFeMaxC, "frontend layer norm backward: C=%d must be a multiple of 4 up to %d", C, kFeMaxC);
  hipLaunchKernelGGL(fe_ln_bwd_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, s, dy, x, gamma, eps, N, C, dx, stats);
  WETTS_LAUNCH_CHECK();
  if (dgamma) WETTS_TRY(ft_colsum(dy, C, x, stats, N, C, cpart, dgamma, s));
  if (dbeta) WETTS_TRY(ft_colsum(dy, C, nullptr, nullptr, N, C, cpart, dbeta, s));
  return WETTS_OK;
}

static int32_t ft_attn_bwd(const float* qkv, const float* maskf, const float* ctx, const float* dctx, int B, int T, int H, int dk,
                           float* pw, float* dsw, float* dqkv, hipStream_t s) {
  WETTS_REQUIRE(qkv && maskf && ctx && dctx && pw && dsw && dqkv, "frontend attention backward: null argument");
  WETTS_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kFeMaxT, "frontend attention backward: B=%d, T=%d (at most %d)", B, T, kFeMaxT);
  WETTS_REQUIRE(H >= 1 && H <= 65535 && dk >= 1 && dk <= kFeMaxDk, "frontend attention backward: %d heads of %d", H, dk);
  const float scale = 1.f / sqrtf((float)dk);
  const dim3 grid((unsigned)cdiv(T, 4), (unsigned)H, (unsigned)B);
  hipLaunchKernelGGL(fe_attn_bwd_q_kernel, grid, dim3(256), 0, s, qkv, maskf, ctx, dctx, T, H, dk, scale, pw, dsw, dqkv);
  WETTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(fe_attn_bwd_kv_kernel, grid, dim3(256), 0, s, qkv, dctx, (const float*)pw, (const float*)dsw, T, H, dk, scale, dqkv);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t ft_ce_bwd(const float* zp, const float* zr, const float* maskf, const int64_t* lab_p, const int64_t* lab_r,
                         const int64_t* counts, int N, int P, int R, double w, float* dl, hipStream_t s) {
  WETTS_REQUIRE(zp && zr && maskf && counts && dl && N >= 1 && P >= 1 && R >= 1, "frontend cross-entropy backward: bad argument");
  hipLaunchKernelGGL(fe_ce_bwd_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, s, zp, zr, maskf, lab_p, lab_r, counts, N, P, R,
                     (float)w, (float)(1.0 - w), dl);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// the regions of the training workspace after the forward and scoring parts, in floats
enum { FT_QKV, FT_CTX, FT_S1, FT_H1, FT_FF, FT_S2, FT_XO, FT_ZP, FT_ZR, FT_DL, FT_DXO, FT_DS2, FT_DFF, FT_DH1, FT_DS1, FT_DCTX,
       FT_DQKV, FT_STATS, FT_PW, FT_DSW, FT_PART, FT_CPART, FT_COUNT };

static void ft_regions(const wetts_frontend_config_t& c, int B, int T, int64_t off[FT_COUNT + 1]) {
  const int64_t N = (int64_t)B * T, d = c.hidden_size, ff = c.transform_ff, P = c.num_polyphones, R = c.num_prosody;
  const int64_t H = c.transform_heads;
  int64_t wmax = 3 * d * d;
  if (ff * d > wmax) wmax = ff * d;
  if (P * d > wmax) wmax = P * d;
  int64_t cmax = 3 * d > ff ? 3 * d : ff;
  if (P + R > cmax) cmax = P + R;
  int64_t sz[FT_COUNT];
  sz[FT_QKV] = 3 * N * d; sz[FT_CTX] = N * d; sz[FT_S1] = N * d; sz[FT_H1] = N * d; sz[FT_FF] = N * ff; sz[FT_S2] = N * d;
  sz[FT_XO] = N * d; sz[FT_ZP] = N * P; sz[FT_ZR] = N * R; sz[FT_DL] = N * (P + R); sz[FT_DXO] = N * d; sz[FT_DS2] = N * d;
  sz[FT_DFF] = N * ff; sz[FT_DH1] = N * d; sz[FT_DS1] = N * d; sz[FT_DCTX] = N * d; sz[FT_DQKV] = 3 * N * d;
  sz[FT_STATS] = 2 * N; sz[FT_PW] = (int64_t)B * H * T * T; sz[FT_DSW] = sz[FT_PW];
  sz[FT_PART] = ft_splits((int)N) > 1 ? ft_splits((int)N) * wmax : 0;
  sz[FT_CPART] = ft_cdiv(N, 64) * cmax;
  off[0] = 0;
  for (int i = 0; i < FT_COUNT; ++i) off[i + 1] = off[i] + align_up(sz[i], 64);
}

static int64_t ft_span_offset(const wetts_frontend_config_t* c) { return fe_tensor_offset(c, "transform.self_attn.in_proj_weight"); }

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_frontend_trainable_span(const wetts_frontend_config_t* cfg, int64_t* offset, int64_t* numel) {
  WETTS_REQUIRE(cfg && offset && numel, "frontend_trainable_span: null argument");
  const int64_t total = wetts_frontend_blob_numel(cfg);
  if (total < 0) return WETTS_E_INVALID;
  *offset = ft_span_offset(cfg);
  *numel = total - *offset;
  return WETTS_OK;
}

int64_t wetts_frontend_train_workspace_bytes(const wetts_frontend_t* h, int32_t B, int32_t T) {
  if (!h || B < 1 || T < 1 || T > kFeMaxT || (int64_t)B * T > 0x7fffffff / 4) {
    set_error("frontend_train_workspace_bytes: bad argument (B=%d T=%d)", B, T);
    return -1;
  }
  int64_t off[FT_COUNT + 1];
  ft_regions(h->cfg, B, T, off);
  return (fe_workspace_floats(h, B, T) + off[FT_COUNT]) * (int64_t)sizeof(float) + align_up(fs_bytes(h->cfg, B, T, nullptr), 256);
}

int32_t wetts_frontend_grad(const wetts_frontend_t* h, const int64_t* input_ids, const int64_t* token_type_ids,
                            const int64_t* attention_mask, const int64_t* phone_labels, const int64_t* prosody_labels,
                            int32_t B, int32_t T, double polyphone_weight, float* grad, float* losses, int64_t* counts,
                            float* nll_phone, float* nll_prosody, int32_t* pred_phone, int32_t* pred_prosody, void* workspace,
                            int64_t workspace_bytes, int32_t* status, void* stream) {
  WETTS_REQUIRE(h && input_ids && grad && losses && counts && workspace, "frontend_grad: null argument");
  WETTS_REQUIRE(h->precision == 0, "frontend_grad: training is float32 only (the handle is in a 16-bit mode)");
  WETTS_REQUIRE(B >= 1 && T >= 1 && T <= kFeMaxT && (int64_t)B * T <= 0x7fffffff / 4, "frontend_grad: B=%d or T=%d out of range", B, T);
  WETTS_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)grad & 15) == 0, "frontend_grad: workspace and grad must be 16-byte aligned");
  const int64_t need = wetts_frontend_train_workspace_bytes(h, B, T);
  WETTS_REQUIRE(workspace_bytes >= need, "frontend_grad: the workspace has %lld bytes, %lld are needed", (long long)workspace_bytes,
                (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const wetts_frontend_config_t& c = h->cfg;
  const int N = B * T, d = c.hidden_size, ff = c.transform_ff, P = c.num_polyphones, R = c.num_prosody, H = c.transform_heads;
  const int64_t fwd = fe_workspace_floats(h, B, T);
  const int64_t sbytes = align_up(fs_bytes(c, B, T, nullptr), 256);
  char* score_ws = (char*)workspace + fwd * sizeof(float);
  float* ws = (float*)(score_ws + sbytes);
  int64_t off[FT_COUNT + 1];
  ft_regions(c, B, T, off);
  auto at = [&](int r) { return ws + off[r]; };
  const FeBlock& k = h->blocks.back();  // `transform`

  // forward: BERT (frozen), then `transform` stage by stage with the launchers of fe_run_block, every intermediate kept
  const float *h0, *maskf;
  WETTS_TRY(fe_hidden_layers(h, (int)h->blocks.size() - 1, input_ids, token_type_ids, attention_mask, B, T, workspace, status, s,
                             "frontend_grad", &h0, &maskf));
  WETTS_TRY(fe_launch_linear(h0, k.wqkv, k.bqkv, nullptr, at(FT_QKV), N, d, 3 * d, kEpiBias, s));
  WETTS_TRY(fe_launch_attention(at(FT_QKV), maskf, at(FT_CTX), B, T, H, d / H, s));
  WETTS_TRY(fe_launch_linear(at(FT_CTX), k.wo, k.bo, h0, at(FT_S1), N, d, d, kEpiRes, s));
  WETTS_TRY(fe_launch_add_ln(at(FT_S1), nullptr, k.g1, k.b1, k.eps, N, d, at(FT_H1), s));
  WETTS_TRY(fe_launch_linear(at(FT_H1), k.w1, k.bb1, nullptr, at(FT_FF), N, d, ff, kEpiRelu, s));
  WETTS_TRY(fe_launch_linear(at(FT_FF), k.w2, k.bb2, at(FT_H1), at(FT_S2), N, ff, d, kEpiRes, s));
  WETTS_TRY(fe_launch_add_ln(at(FT_S2), nullptr, k.g2, k.b2, k.eps, N, d, at(FT_XO), s));
  // the loss, the counts and the status word: the scoring launches themselves
  WETTS_TRY(fs_launch(h, at(FT_XO), maskf, phone_labels, prosody_labels, B, T, nll_phone, nll_prosody, pred_phone, pred_prosody,
                      losses, counts, score_ws, sbytes, status, s));
  WETTS_TRY(fe_launch_heads(h, at(FT_XO), maskf, N, 0, at(FT_ZP), at(FT_ZR), s));

  // backward; the gradients land at their tensors' places in the span, its alignment padding is zeroed first
  const int64_t span = ft_span_offset(&c), numel = fe_tensor_offset(&c, nullptr) - span;
  WETTS_HIP_CHECK(hipMemsetAsync(grad, 0, (size_t)numel * sizeof(float), s));
  auto g = [&](const char* name) { return grad + (fe_tensor_offset(&c, name) - span); };
  float *part = at(FT_PART), *cpart = at(FT_CPART), *dl = at(FT_DL);
  WETTS_TRY(ft_ce_bwd(at(FT_ZP), at(FT_ZR), maskf, phone_labels, prosody_labels, counts, N, P, R, polyphone_weight, dl, s));
  WETTS_TRY(ft_wgrad(dl, P + R, at(FT_XO), N, P, d, g("phone_classifier.weight"), g("phone_classifier.bias"), part, cpart, s));
  WETTS_TRY(ft_wgrad(dl + P, P + R, at(FT_XO), N, R, d, g("prosody_classifier.weight"), g("prosody_classifier.bias"), part, cpart, s));
  WETTS_TRY(ft_dgrad(dl, P + R, h->wp, N, P, d, BG_NONE, nullptr, at(FT_DS1), s));  // (FT_DS1 is free until norm1's backward)
  WETTS_TRY(ft_dgrad(dl + P, P + R, h->wr, N, R, d, BG_ADD, at(FT_DS1), at(FT_DXO), s));
  WETTS_TRY(ft_ln_bwd(at(FT_DXO), at(FT_S2), k.g2, k.eps, N, d, at(FT_DS2), at(FT_STATS), g("transform.norm2.weight"),
                      g("transform.norm2.bias"), cpart, s));
  WETTS_TRY(ft_wgrad(at(FT_DS2), d, at(FT_FF), N, d, ff, g("transform.linear2.weight"), g("transform.linear2.bias"), part, cpart, s));
  WETTS_TRY(ft_dgrad(at(FT_DS2), d, k.w2, N, d, ff, BG_RELU_MASK, at(FT_FF), at(FT_DFF), s));
  WETTS_TRY(ft_wgrad(at(FT_DFF), ff, at(FT_H1), N, ff, d, g("transform.linear1.weight"), g("transform.linear1.bias"), part, cpart, s));
  WETTS_TRY(ft_dgrad(at(FT_DFF), ff, k.w1, N, ff, d, BG_ADD, at(FT_DS2), at(FT_DH1), s));
  WETTS_TRY(ft_ln_bwd(at(FT_DH1), at(FT_S1), k.g1, k.eps, N, d, at(FT_DS1), at(FT_STATS), g("transform.norm1.weight"),
                      g("transform.norm1.bias"), cpart, s));
  WETTS_TRY(ft_wgrad(at(FT_DS1), d, at(FT_CTX), N, d, d, g("transform.self_attn.out_proj.weight"),
                     g("transform.self_attn.out_proj.bias"), part, cpart, s));
  WETTS_TRY(ft_dgrad(at(FT_DS1), d, k.wo, N, d, d, BG_NONE, nullptr, at(FT_DCTX), s));
  WETTS_TRY(ft_attn_bwd(at(FT_QKV), maskf, at(FT_CTX), at(FT_DCTX), B, T, H, d / H, at(FT_PW), at(FT_DSW), at(FT_DQKV), s));
  return ft_wgrad(at(FT_DQKV), 3 * d, h0, N, 3 * d, d, g("transform.self_attn.in_proj_weight"),
                  g("transform.self_attn.in_proj_bias"), part, cpart, s);
}

int32_t wetts_frontend_adamw(float* p, const float* grad, float* m, float* v, int64_t numel, double lr, double beta1,
                             double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2,
                             void* stream) {
  WETTS_REQUIRE(p && grad && m && v && numel >= 4 && numel % 4 == 0, "frontend_adamw: bad argument (numel=%lld)", (long long)numel);
  WETTS_REQUIRE((((uintptr_t)p | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "frontend_adamw: 16-byte alignment");
  WETTS_REQUIRE(bias_correction1 > 0. && bias_correction2 > 0., "frontend_adamw: the bias corrections must be positive");
  const int64_t n4 = numel / 4;
  WETTS_REQUIRE(ft_cdiv(n4, 256) <= 0x7fffffff, "frontend_adamw: %lld floats exceed one launch", (long long)numel);
  hipLaunchKernelGGL(fe_adamw_kernel, dim3((unsigned)ft_cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, (float4*)p,
                     (const float4*)grad, (float4*)m, (float4*)v, n4, (float)(1. - lr * weight_decay), (float)(1. - beta1),
                     (float)beta2, (float)(1. - beta2), (float)sqrt(bias_correction2), (float)eps, (float)(lr / bias_correction1));
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t wetts_frontend_adamw_step(wetts_frontend_t* h, const float* grad, float* m, float* v, double lr, double beta1,
                                  double beta2, double eps, double weight_decay, double bias_correction1,
                                  double bias_correction2, void* stream) {
  WETTS_REQUIRE(h, "frontend_adamw_step: null argument");
  WETTS_REQUIRE(h->precision == 0, "frontend_adamw_step: training is float32 only (the handle is in a 16-bit mode)");
  const int64_t span = ft_span_offset(&h->cfg), numel = fe_tensor_offset(&h->cfg, nullptr) - span;
  return wetts_frontend_adamw(h->blob + span, grad, m, v, numel, lr, beta1, beta2, eps, weight_decay, bias_correction1,
                              bias_correction2, stream);
}

int32_t wetts_frontend_read_weights(const wetts_frontend_t* h, int64_t offset, int64_t numel, float* out, void* stream) {
  WETTS_REQUIRE(h && out, "frontend_read_weights: null argument");
  const int64_t total = fe_tensor_offset(&h->cfg, nullptr);
  WETTS_REQUIRE(offset >= 0 && numel >= 1 && offset <= total - numel, "frontend_read_weights: [%lld, +%lld) is outside the blob",
                (long long)offset, (long long)numel);
  WETTS_HIP_CHECK(hipMemcpyAsync(out, h->blob + offset, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return WETTS_OK;
}

// ---- the stages alone ----
int32_t wetts_frontend_linear_dgrad(const float* dy, int64_t ldy, const float* weight, int32_t N, int32_t M, int32_t K,
                                    int32_t epilogue, const float* aux, float* dx, void* stream) {
  WETTS_REQUIRE(epilogue >= BG_NONE && epilogue <= BG_ADD && ldy >= M, "frontend_linear_dgrad: epilogue %d, ldy %lld", epilogue,
                (long long)ldy);
  return ft_dgrad(dy, ldy, weight, N, M, K, epilogue, aux, dx, (hipStream_t)stream);
}

int64_t wetts_frontend_linear_wgrad_workspace_bytes(int32_t N, int32_t M, int32_t K) {
  if (N < 1 || M < 1 || K < 1) {
    set_error("frontend_linear_wgrad_workspace_bytes: bad argument");
    return -1;
  }
  return (align_up(ft_part_floats(N, M, K), 64) + (int64_t)cdiv(N, 64) * M) * (int64_t)sizeof(float);
}

int32_t wetts_frontend_linear_wgrad(const float* dy, int64_t ldy, const float* x, int32_t N, int32_t M, int32_t K, float* dw,
                                    float* db, void* workspace, int64_t workspace_bytes, void* stream) {
  WETTS_REQUIRE(workspace && N >= 1 && M >= 1 && K >= 1 && ldy >= M, "frontend_linear_wgrad: bad argument");
  WETTS_REQUIRE(workspace_bytes >= wetts_frontend_linear_wgrad_workspace_bytes(N, M, K), "frontend_linear_wgrad: workspace too small");
  float* part = (float*)workspace;
  return ft_wgrad(dy, ldy, x, N, M, K, dw, db, part, part + align_up(ft_part_floats(N, M, K), 64), (hipStream_t)stream);
}

int32_t wetts_frontend_layer_norm_backward(const float* dy, const float* x, const float* gamma, float eps, int32_t N, int32_t C,
                                           float* dx, float* dgamma, float* dbeta, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  WETTS_REQUIRE(workspace && N >= 1 && C >= 1, "frontend_layer_norm_backward: bad argument");
  const int64_t st = align_up(2 * (int64_t)N, 64);
  WETTS_REQUIRE(workspace_bytes >= (st + (int64_t)cdiv(N, 64) * C) * (int64_t)sizeof(float),
                "frontend_layer_norm_backward: the workspace needs %lld bytes", (long long)((st + (int64_t)cdiv(N, 64) * C) * 4));
  float* stats = (float*)workspace;
  return ft_ln_bwd(dy, x, gamma, eps, N, C, dx, stats, dgamma, dbeta, stats + st, (hipStream_t)stream);
}

int32_t wetts_frontend_attention_backward(const float* qkv, const float* key_mask, const float* ctx, const float* dctx, int32_t B,
                                          int32_t T, int32_t heads, int32_t dk, float* dqkv, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  WETTS_REQUIRE(workspace && B >= 1 && T >= 1 && heads >= 1, "frontend_attention_backward: bad argument");
  const int64_t pw = align_up((int64_t)B * heads * T * T, 64);
  WETTS_REQUIRE(workspace_bytes >= 2 * pw * (int64_t)sizeof(float), "frontend_attention_backward: the workspace needs %lld bytes",
                (long long)(2 * pw * 4));
  float* w = (float*)workspace;
  return ft_attn_bwd(qkv, key_mask, ctx, dctx, B, T, heads, dk, w, w + pw, dqkv, (hipStream_t)stream);
}

int32_t wetts_frontend_ce_backward(const float* phone_logits, const float* prosody_logits, const float* key_mask,
                                   const int64_t* phone_labels, const int64_t* prosody_labels, const int64_t* counts, int32_t N,
                                   int32_t P, int32_t R, double polyphone_weight, float* dlogits, void* stream) {
  return ft_ce_bwd(phone_logits, prosody_logits, key_mask, phone_labels, prosody_labels, counts, N, P, R, polyphone_weight, dlogits,
                   (hipStream_t)stream);
}

}  // extern "C"
