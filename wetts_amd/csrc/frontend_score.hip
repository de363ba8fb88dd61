// Scoring the text frontend: what the reference computes from its logits in the validation pass of frontend/train.py:43-94
// (two F.cross_entropy(ignore_index=-100) terms and compute_accuracy), in frontend/test_polyphone.py:72-86 (masked accuracy
// counts) and in frontend/test_prosody.py:77-102 (the counts behind the three binary F1 scores) -- without a logit in HBM.
//
// The forward pass runs up to the transform layer's output x [N = B * T][hidden] (fe_hidden, frontend.hip).  Then:
//   fe_score_tile_kernel    the classifier GEMM of 32 classes of ONE head x 64 tokens per block, K split over 8 waves as
//                           fe_linear_kernel does, with a split-softmax epilogue: per (class tile, token) one 16-byte record
//                           {tile maximum, sum of exp(z - max) in ascending class order, lowest argmax, the label's logit}
//   fe_score_token_kernel   one thread per token combines its records in ascending tile order -> nll and argmax per head
//   fe_score_reduce_kernel  one block: float64 sums of the f32 nll in a fixed order, and the 22 integer counts
// The k order of a logit is fixed by `hidden` alone and a record depends on its own token alone, so a token's results do
// not depend on N or on its neighbours.  No atomics on floats.
#include "frontend_dev.h"

#include <math.h>

namespace wetts {

struct FeScoreRec {
  float mx, sum;
  int32_t arg;
  float zl;
};
static_assert(sizeof(FeScoreRec) == 16, "one 16-byte record per (class tile, token)");

constexpr int64_t kFeIgnore = -100;  // dataset.py:19 IGNORE_ID
constexpr int kFsZS = 33;            // row stride of the logits tile in LDS ([token][class], odd: no bank conflicts)

// grid: (class tiles of the phone head + class tiles of the prosody head, ceil(N / 64)).  Weight rows past the head's
// last class are read clamped (as fe_linear_kernel reads them) and left out of the maximum, the sum and the argmax.
__global__ void __launch_bounds__(64 * kFeKG)
fe_score_tile_kernel(const float* __restrict__ X, const float* __restrict__ maskf, const float* __restrict__ wp,
                     const float* __restrict__ bp, const float* __restrict__ wr, const float* __restrict__ br,
                     const int64_t* __restrict__ lab_p, const int64_t* __restrict__ lab_r, int N, int K, int P, int R,
                     int tiles_p, int64_t Npad, FeScoreRec* __restrict__ rec) {
  __shared__ float part[kFeKG][2][16][64];
  static_assert(64 * kFsZS <= kFeKG * 2 * 16 * 64, "the logits tile reuses the partial tiles' LDS");
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x, n0 = blockIdx.y * kFeNT;
  const bool ph = tile < tiles_p;  // block-uniform: a tile belongs to one head
  const float* W = ph ? wp : wr;
  const float* bias = ph ? bp : br;
  const int64_t* labels = ph ? lab_p : lab_r;
  const int M = ph ? P : R, m0 = (ph ? tile : tile - tiles_p) * 32;
  const bool two = n0 + 32 < N;  // block-uniform: the second column tile has a token
  const int S = K >> 3;

  const int mr = min(m0 + l31, M - 1), c0 = min(n0 + l31, N - 1), c1 = min(n0 + 32 + l31, N - 1);
  const float* wrow = W + (int64_t)mr * K + 4 * half;
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
      ra[i] = *reinterpret_cast<const float4*>(wrow + 8 * s);
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
          ra[i] = *reinterpret_cast<const float4*>(wrow + 8 * sn);
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
  // wave w: column tile w / 4, the registers 4 g .. 4 g + 3 (g = w % 4) = classes m0 + 8 g + 4 half + {0..3} of column l31
  const int t = w >> 2, g = w & 3;
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 4 * g + i;
    v[i] = ((part[0][t][r][lane] + part[1][t][r][lane]) + (part[2][t][r][lane] + part[3][t][r][lane])) +
           ((part[4][t][r][lane] + part[5][t][r][lane]) + (part[6][t][r][lane] + part[7][t][r][lane]));
    v[i] += bias[min(m0 + 8 * g + 4 * half + i, M - 1)];
  }
  __syncthreads();  // every partial tile is read: its LDS becomes the logits tile [64 tokens][32 classes]
  float* zt = &part[0][0][0][0];
#pragma unroll
  for (int i = 0; i < 4; ++i) zt[(32 * t + l31) * kFsZS + 8 * g + 4 * half + i] = v[i];
  __syncthreads();
  if (threadIdx.x >= 64) return;
  // one thread per token: the tile's real classes in ascending order
  const int n = n0 + (int)threadIdx.x;
  FeScoreRec out;
  out.mx = -INFINITY; out.sum = 0.f; out.arg = -1; out.zl = 0.f;  // neutral: a padded token, or one past N
  if (n < N && maskf[n] != 0.f) {
    const float* z = zt + threadIdx.x * kFsZS;
    const int cnt = min(32, M - m0);
    float mx = z[0];
    int arg = 0;
    for (int c = 1; c < cnt; ++c)
      if (z[c] > mx) { mx = z[c]; arg = c; }  // strict: the lowest index keeps a tie
    float sum = 0.f;
    for (int c = 0; c < cnt; ++c) sum += expf(z[c] - mx);
    out.mx = mx; out.sum = sum; out.arg = m0 + arg;
    if (labels) {
      const int64_t l = labels[n];
      if (l >= m0 && l < m0 + cnt) out.zl = z[l - m0];
    }
  }
  rec[(int64_t)tile * Npad + n] = out;  // n < Npad = N rounded up to the token tile
}

// One thread per token and both heads: running maximum, rescaled sum, lowest argmax over the tiles in ascending order;
// nll = (max + logf(sum)) - z_label (F.cross_entropy's per-token term, train.py:73-80); 0 where the label is ignored.
__global__ void __launch_bounds__(256)
fe_score_token_kernel(const FeScoreRec* __restrict__ rec, const float* __restrict__ maskf, const int64_t* __restrict__ lab_p,
                      const int64_t* __restrict__ lab_r, int N, int P, int R, int tiles_p, int tiles_r, int64_t Npad,
                      float* __restrict__ nll_p, float* __restrict__ nll_r, int32_t* __restrict__ pred_p,
                      int32_t* __restrict__ pred_r, int32_t* __restrict__ status) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const bool on = maskf[n] != 0.f;
  int bits = 0;
#pragma unroll
  for (int hd = 0; hd < 2; ++hd) {
    const int64_t* labels = hd == 0 ? lab_p : lab_r;
    const int M = hd == 0 ? P : R, t0 = hd == 0 ? 0 : tiles_p, nt = hd == 0 ? tiles_p : tiles_r;
    const int64_t lab = labels ? labels[n] : kFeIgnore;
    float nll = 0.f;
    int pred = -1;
    if (!on) {
      if (lab != kFeIgnore) bits |= WETTS_STATUS_LABEL_AT_PAD;
    } else {
      FeScoreRec a = rec[(int64_t)t0 * Npad + n];
      for (int t = 1; t < nt; ++t) {
        const FeScoreRec b = rec[(int64_t)(t0 + t) * Npad + n];
        if (b.mx > a.mx) {  // strict: an earlier tile keeps a tie
          a.sum = __builtin_fmaf(a.sum, expf(a.mx - b.mx), b.sum);
          a.mx = b.mx;
          a.arg = b.arg;
        } else {
          a.sum = __builtin_fmaf(b.sum, expf(b.mx - a.mx), a.sum);
        }
      }
      pred = a.arg;
      if (lab != kFeIgnore) {
        if (lab < 0 || lab >= M) bits |= WETTS_STATUS_LABEL_RANGE;
        else nll = (a.mx + logf(a.sum)) - rec[(int64_t)(t0 + (int)(lab >> 5)) * Npad + n].zl;
      }
    }
    (hd == 0 ? nll_p : nll_r)[n] = nll;
    (hd == 0 ? pred_p : pred_r)[n] = pred;
  }
  if (bits && status) atomicOr(status, bits);
}

// float64 sums in the reduction order of disc_rows_kernel (discriminator.hip) and dur_disc_row_means_kernel: thread i
// adds the elements i, i + 256, .. in ascending order into four interleaved accumulators, (a0 + a1) + (a2 + a3), the
// butterfly over the lanes, (w0 + w1) + (w2 + w3) over the waves.
__device__ __forceinline__ double fs_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double fs_block_sum(const double a[4], double* part) {
  const double v = fs_wave_sum((a[0] + a[1]) + (a[2] + a[3]));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (part[0] + part[1]) + (part[2] + part[3]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ int fs_wave_count(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One block.  losses[h] = mean nll over the scored labels of head h (NaN without any: torch's 0 / 0).
// counts: [0..1] phone total, correct (test_polyphone.py:78-82); [2..3] prosody total, correct; [4..12] TP, FP, FN at the
// thresholds > 0, > 1, > 2 over the positions 1 .. len_b of every row (test_prosody.py:83-100, len_b = the row's
// non-ignored prosody labels, the slice clipped to T as Python clips it; a -100 label inside it binarises to 0, as does
// the -1 prediction of a padded token); [13..21] the same with exclude_end (positions 1 .. len_b - 1).
__global__ void __launch_bounds__(256)
fe_score_reduce_kernel(const float* __restrict__ maskf, const int64_t* __restrict__ lab_p, const int64_t* __restrict__ lab_r,
                       const float* __restrict__ nll_p, const float* __restrict__ nll_r, const int32_t* __restrict__ pred_p,
                       const int32_t* __restrict__ pred_r, int B, int T, int P, int R, float* __restrict__ losses,
                       int64_t* __restrict__ counts) {
  __shared__ double part[4];
  __shared__ unsigned long long cnt[22];
  const int N = B * T, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 22) cnt[threadIdx.x] = 0ull;
  __syncthreads();
  int c[22];
#pragma unroll
  for (int i = 0; i < 22; ++i) c[i] = 0;
  double sp[4] = {0., 0., 0., 0.}, sr[4] = {0., 0., 0., 0.};
  int k = 0;
  for (int e = threadIdx.x; e < N; e += 256, ++k) {
    const bool on = maskf[e] != 0.f;
    if (lab_p) {
      const int64_t l = lab_p[e];
      if (on && l >= 0 && l < P) {
        sp[k & 3] += (double)nll_p[e];
        c[0] += 1;
        c[1] += (int64_t)pred_p[e] == l;
      }
    }
    if (lab_r) {
      const int64_t l = lab_r[e];
      if (on && l >= 0 && l < R) {
        sr[k & 3] += (double)nll_r[e];
        c[2] += 1;
        c[3] += (int64_t)pred_r[e] == l;
      }
    }
  }
  if (lab_r)
    for (int b = wave; b < B; b += 4) {  // a wave per row
      const int64_t* lr = lab_r + (int64_t)b * T;
      const int32_t* pr = pred_r + (int64_t)b * T;
      int len = 0;
      for (int p = lane; p < T; p += 64) len += lr[p] != kFeIgnore;
      len = fs_wave_count(len);
      const int end = min(len, T - 1);  // positions 1 .. end
      for (int p = 1 + lane; p <= end; p += 64) {
        const int64_t y = lr[p];
        const int q = pr[p];
        const bool ex = p <= len - 1;
#pragma unroll
        for (int th = 0; th < 3; ++th) {
          const bool yb = y > th, qb = q > th;
          const int tp = yb && qb, fp = !yb && qb, fn = yb && !qb;
          c[4 + 3 * th] += tp; c[5 + 3 * th] += fp; c[6 + 3 * th] += fn;
          if (ex) { c[13 + 3 * th] += tp; c[14 + 3 * th] += fp; c[15 + 3 * th] += fn; }
        }
      }
    }
#pragma unroll
  for (int i = 0; i < 22; ++i)
    if (c[i]) atomicAdd(&cnt[i], (unsigned long long)c[i]);  // integers: the order does not matter
  const double a_p = fs_block_sum(sp, part), a_r = fs_block_sum(sr, part);  // its barriers order the atomics too
  if (threadIdx.x < 22) counts[threadIdx.x] = (int64_t)cnt[threadIdx.x];
  if (threadIdx.x == 0) {
    losses[0] = (float)(a_p / (double)cnt[0]);
    losses[1] = (float)(a_r / (double)cnt[2]);
  }
}

// bytes of the scoring scratch: the records [tiles][Npad], then nll [2][Npad] f32 and pred [2][Npad] int32
int64_t fs_bytes(const wetts_frontend_config_t& c, int B, int T, int64_t* npad) {
  const int64_t Np = align_up((int64_t)B * T, kFeNT);
  if (npad) *npad = Np;
  return ((int64_t)(cdiv(c.num_polyphones, 32) + cdiv(c.num_prosody, 32)) * 16 + 16) * Np;
}

int32_t fs_launch(const wetts_frontend* h, const float* x, const float* maskf, const int64_t* lab_p,
                         const int64_t* lab_r, int B, int T, float* nll_p, float* nll_r, int32_t* pred_p, int32_t* pred_r,
                         float* losses, int64_t* counts, void* workspace, int64_t workspace_bytes, int32_t* status,
                         hipStream_t s) {
  WETTS_REQUIRE(h && x && maskf && losses && counts && workspace, "frontend_score: null argument");
  WETTS_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T <= 0x7fffffff / 4, "frontend_score: B=%d or T=%d out of range", B, T);
  const int N = B * T, P = h->cfg.num_polyphones, R = h->cfg.num_prosody, K = h->cfg.hidden_size;
  const int tiles_p = cdiv(P, 32), tiles_r = cdiv(R, 32);
  int64_t Npad;
  const int64_t need = fs_bytes(h->cfg, B, T, &Npad);
  WETTS_REQUIRE(workspace_bytes >= need, "frontend_score: the workspace has %lld bytes, %lld are needed",
                (long long)workspace_bytes, (long long)need);
  WETTS_REQUIRE(((uintptr_t)workspace & 15) == 0, "frontend_score: the workspace must be 16-byte aligned");
  const int64_t ct = Npad / kFeNT;
  WETTS_REQUIRE(ct <= 65535 && tiles_p + tiles_r <= 65535, "frontend_score: %d tokens exceed one launch", N);
  FeScoreRec* rec = (FeScoreRec*)workspace;
  float* f = (float*)(rec + (int64_t)(tiles_p + tiles_r) * Npad);
  if (!nll_p) nll_p = f;
  if (!nll_r) nll_r = f + Npad;
  if (!pred_p) pred_p = (int32_t*)(f + 2 * Npad);
  if (!pred_r) pred_r = (int32_t*)(f + 3 * Npad);
  hipLaunchKernelGGL(fe_score_tile_kernel, dim3((unsigned)(tiles_p + tiles_r), (unsigned)ct), dim3(64 * kFeKG), 0, s, x, maskf,
                     h->wp, h->bp, h->wr, h->br, lab_p, lab_r, N, K, P, R, tiles_p, Npad, rec);
  WETTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(fe_score_token_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, (const FeScoreRec*)rec, maskf, lab_p,
                     lab_r, N, P, R, tiles_p, tiles_r, Npad, nll_p, nll_r, pred_p, pred_r, status);
  WETTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(fe_score_reduce_kernel, dim3(1), dim3(256), 0, s, maskf, lab_p, lab_r, (const float*)nll_p,
                     (const float*)nll_r, (const int32_t*)pred_p, (const int32_t*)pred_r, B, T, P, R, losses, counts);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int64_t wetts_frontend_score_workspace_bytes(const wetts_frontend_t* h, int32_t B, int32_t T) {
  if (!h || B < 1 || T < 1 || (int64_t)B * T > 0x7fffffff / 4) {
    set_error("frontend_score_workspace_bytes: bad argument (B=%d T=%d)", B, T);
    return -1;
  }
  return fe_workspace_floats(h, B, T) * (int64_t)sizeof(float) + fs_bytes(h->cfg, B, T, nullptr);
}

int32_t wetts_frontend_score(const wetts_frontend_t* h, const int64_t* input_ids, const int64_t* token_type_ids,
                             const int64_t* attention_mask, const int64_t* phone_labels, const int64_t* prosody_labels,
                             int32_t B, int32_t T, float* nll_phone, float* nll_prosody, int32_t* pred_phone,
                             int32_t* pred_prosody, float* losses, int64_t* counts, void* workspace, int64_t workspace_bytes,
                             int32_t* status, void* stream) {
  WETTS_REQUIRE(h && input_ids && losses && counts && workspace, "frontend_score: null argument");
  WETTS_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T <= 0x7fffffff / 4, "frontend_score: B=%d or T=%d out of range", B, T);
  const int64_t fwd = fe_workspace_floats(h, B, T) * (int64_t)sizeof(float);
  WETTS_REQUIRE(workspace_bytes >= fwd + fs_bytes(h->cfg, B, T, nullptr),
                "frontend_score: the workspace has %lld bytes, %lld are needed", (long long)workspace_bytes,
                (long long)(fwd + fs_bytes(h->cfg, B, T, nullptr)));
  hipStream_t s = (hipStream_t)stream;
  const float *x, *maskf;
  WETTS_TRY(fe_hidden(h, input_ids, token_type_ids, attention_mask, B, T, workspace, status, s, "frontend_score", &x, &maskf));
  return fs_launch(h, x, maskf, phone_labels, prosody_labels, B, T, nll_phone, nll_prosody, pred_phone, pred_prosody, losses,
                   counts, (char*)workspace + fwd, workspace_bytes - fwd, status, s);
}

int32_t wetts_frontend_score_heads(const wetts_frontend_t* h, const float* x, const float* key_mask,
                                   const int64_t* phone_labels, const int64_t* prosody_labels, int32_t B, int32_t T,
                                   float* nll_phone, float* nll_prosody, int32_t* pred_phone, int32_t* pred_prosody,
                                   float* losses, int64_t* counts, void* workspace, int64_t workspace_bytes, int32_t* status,
                                   void* stream) {
  return fs_launch(h, x, key_mask, phone_labels, prosody_labels, B, T, nll_phone, nll_prosody, pred_phone, pred_prosody,
                   losses, counts, workspace, workspace_bytes, status, (hipStream_t)stream);
}

}  // extern "C"
