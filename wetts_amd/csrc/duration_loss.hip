// The duration loss of SynthesizerTrn.forward (models.py:196-206): the stochastic duration predictor's forward pass
// (duration_predictors.py:206-253: the variational lower bound nll + logq of given durations) and the plain
// DurationPredictor's squared error.  This file holds the device code the forward direction adds to the kernels the
// reverse pass already has -- the forward rational-quadratic spline, ElementwiseAffine forward, the dequantisation
// + Log flow, and the reductions; model.hip (wetts_duration_sdp_forward) strings them together with the convs.
//
// Log-determinants.  Two f32 accumulators [B, Tx] (nll_terms, logq_terms) are zeroed by the caller; every kernel that
// owns a position adds its signed contribution with a plain load, add and store (the kernels are serialised on the
// stream: no atomics).  The Gaussian terms and ElementwiseAffine's (logs0 + logs1) * len are added by the reduction.
//
// Reduction order: that of losses.hip.  Per utterance ONE block of 256 threads; thread i owns positions i, i + 256, ...
// of the row, skips masked ones, adds visit k into accumulator k & 3, (a0 + a1) + (a2 + a3), a butterfly over the 64
// lanes, (w0 + w1) + (w2 + w3) over the four waves through LDS.  So a row's sums depend on the row alone: a row alone
// and the same row inside a padded batch give the same bits.  The batch total is one wave.
#include <math.h>

#include "kernels.h"

namespace wetts {

namespace {

constexpr int kRedThreads = 256;
constexpr float kLog2Pi = 1.8378770664093453f;  // math.log(2 * math.pi), a python double, then f32

static inline dim3 grid1d(int64_t n, int threads) { return dim3((unsigned)((n + threads - 1) / threads)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the block's 256 threads, valid in thread 0; `part` is 4 floats of LDS (losses.hip:block_sum)
__device__ __forceinline__ float block_sum(float v, float* part) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (part[0] + part[1]) + (part[2] + part[3]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ float softplus_f(float x) {
  return x > 20.f ? x : log1pf(expf(x));  // F.softplus(beta=1, threshold=20), as kernels.hip
}

// F.logsigmoid, stable for either sign
__device__ __forceinline__ float logsigmoid_f(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

}  // namespace

// ---------------------------------------------------------------------------------------------
// ElementwiseAffine.forward (duration_predictors.py:133-138) on both channels of x [B,2,T] -> out (may alias x):
// y = (m + exp(logs) * x) * mask.  x is read as x * mask first (`e_q = randn * x_mask`, :229-230; a no-op for the
// already masked z of the main flows): a masked-out position is never read, whatever lies there.
__global__ void affine_forward_kernel(const float* x, const float* __restrict__ m, const float* __restrict__ logs,
                                      const float* __restrict__ mask, int B, int T, float* out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * T) return;
  const int t = idx % T, b = idx / T;
  const float mk = mask[idx];
  const int64_t i0 = (int64_t)b * 2 * T + t, i1 = i0 + T;
  float y0 = 0.f, y1 = 0.f;
  if (mk != 0.f) {
    // exp(logs) in double, rounded once: the scale multiplies every position ahead of a spline whose log-determinant
    // can be steep in x (a pinned scale of 10 turns one ulp of it into 1e-4 of an utterance's nll)
    const float e0 = (float)exp((double)logs[0]), e1 = (float)exp((double)logs[1]);
    y0 = (m[0] + e0 * (x[i0] * mk)) * mk;
    y1 = (m[1] + e1 * (x[i1] * mk)) * mk;
  }
  out[i0] = y0;
  out[i1] = y1;
}

int32_t k_affine_forward(const float* x, const float* m, const float* logs, const float* mask, int B, int T,
                         float* out, hipStream_t s) {
  if ((int64_t)B * T == 0) return WETTS_OK;
  hipLaunchKernelGGL(affine_forward_kernel, grid1d((int64_t)B * T, 256), dim3(256), 0, s, x, m, logs, mask, B, T, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Rational-quadratic spline, forward direction, linear tails (transforms.py:47-97, 100-147, 188-207), operation by
// operation in the reference's order and with spline_inverse_kernel's f32 constants.  One thread per (b, t).
// z [B,2,T] in place: channel ch0 *= mask, channel ch1 = spline(z[ch1]) * mask; acc[b,t] += sign * logabsdet * mask.
//
// The knot tables are never indexed at run time (that is what costs spline_inverse_kernel its scratch): the two
// cumulative sums are built in ONE fully unrolled pass over the NB compile-time bins, and while walking the pass keeps
// the (cw, cw_next, ch, ch_next) of the last bin whose left edge satisfies x >= edge_i.  The edges ascend, so that is
// searchsorted's `sum(x >= edges) - 1`; the last edge, right + 1e-6 (transforms.py:43), lies beyond every x the
// inside-interval test lets through and selects nothing.  The two derivative logits are global loads at the bin found.
template <int NB>
__global__ void spline_forward_kernel(float* __restrict__ z, int ch0, int ch1, const float* __restrict__ h,
                                      const float* __restrict__ mask, float tail, float div, int B, int T, float sign,
                                      float* __restrict__ acc) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * T) return;
  const int t = idx % T, b = idx / T;
  const float mk = mask[idx];
  float* z0 = z + ((int64_t)b * 2 + ch0) * T + t;
  float* z1 = z + ((int64_t)b * 2 + ch1) * T + t;
  const float x = *z1;
  const float* hp = h + (int64_t)b * (3 * NB - 1) * T + t;
  float outv = x, lad = 0.f;
  if (x >= -tail && x <= tail) {
    const float min_w = 1e-3f, min_h = 1e-3f, min_d = 1e-3f;
    const float one_minus = (float)(1.0 - 1e-3 * (double)NB);  // python double, then f32 (transforms.py:125)
    float uw[NB], uh[NB];  // compile-time indices only: registers
    float mxw = -INFINITY, mxh = -INFINITY;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      uw[i] = hp[(int64_t)i * T] / div;
      uh[i] = hp[(int64_t)(NB + i) * T] / div;
      mxw = fmaxf(mxw, uw[i]);
      mxh = fmaxf(mxh, uh[i]);
    }
    float smw = 0.f, smh = 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      uw[i] = expf(uw[i] - mxw);
      uh[i] = expf(uh[i] - mxh);
      smw += uw[i];
      smh += uh[i];
    }
    float cumw = 0.f, cumh = 0.f, cw_i = -tail, ch_i = -tail;
    float in_cw = -tail, in_cwn = tail, in_ch = -tail, in_chn = tail;
    int bin = 0;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      cumw += min_w + one_minus * (uw[i] / smw);
      cumh += min_h + one_minus * (uh[i] / smh);
      const float cw_n = (i == NB - 1) ? tail : (2.f * tail) * cumw + (-tail);
      const float ch_n = (i == NB - 1) ? tail : (2.f * tail) * cumh + (-tail);
      if (i == 0 || x >= cw_i) {  // edge 0 is `left` <= x
        in_cw = cw_i; in_cwn = cw_n; in_ch = ch_i; in_chn = ch_n;
        bin = i;
      }
      cw_i = cw_n;
      ch_i = ch_n;
    }
    const float in_bw = in_cwn - in_cw;
    const float in_h = in_chn - in_ch;
    const float in_delta = in_h / in_bw;
    const float cst = (float)0.5397424172369522;  // np.log(np.exp(1 - 1e-3) - 1): the end derivatives come out as 1
    const float ud0 = (bin == 0) ? cst : hp[(int64_t)(2 * NB + bin - 1) * T];
    const float ud1 = (bin == NB - 1) ? cst : hp[(int64_t)(2 * NB + bin) * T];
    const float d0 = min_d + softplus_f(ud0);
    const float d1 = min_d + softplus_f(ud1);

    const float theta = (x - in_cw) / in_bw;
    const float tomt = theta * (1.f - theta);
    const float num = in_h * (in_delta * (theta * theta) + d0 * tomt);
    const float den = in_delta + ((d0 + d1 - 2.f * in_delta) * tomt);
    outv = in_ch + num / den;
    const float omt = 1.f - theta;
    const float dnum = (in_delta * in_delta) * (d1 * (theta * theta) + 2.f * in_delta * tomt + d0 * (omt * omt));
    lad = logf(dnum) - 2.f * logf(den);
  }
  *z1 = outv * mk;
  *z0 = (*z0) * mk;
  if (mk != 0.f) acc[idx] = acc[idx] + sign * (lad * mk);
}

int32_t k_spline_forward(float* z, int ch0, int ch1, const float* h, const float* mask, int num_bins, float tail_bound,
                         float div, int B, int T, float sign, float* acc, hipStream_t s) {
  WETTS_REQUIRE(num_bins == 10, "spline forward: num_bins must be 10 (ConvFlow's default), got %d", num_bins);
  if ((int64_t)B * T == 0) return WETTS_OK;
  hipLaunchKernelGGL(spline_forward_kernel<10>, grid1d((int64_t)B * T, 128), dim3(128), 0, s, z, ch0, ch1, h, mask,
                     tail_bound, div, B, T, sign, acc);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// duration_predictors.py:235-247 in one pass: z_u, z1 = split(z_q); u = sigmoid(z_u) * mask; z0 = (w - u) * mask;
// logdet_tot_q += (logsigmoid(z_u) + logsigmoid(-z_u)) * mask, which logq SUBTRACTS; the Log flow y = log(clamp_min(z0,
// 1e-5)) * mask with logdet -y, which nll subtracts: nll_terms += y.  z = cat(y, z1).  A masked-out position writes
// zeros and reads nothing of w.  A masked-in w that is negative or not finite is flagged in the status word.
__global__ void dequant_log_kernel(const float* __restrict__ z_q, int chu, int ch1, const float* __restrict__ w,
                                   const float* __restrict__ mask, int B, int T, float* __restrict__ z,
                                   float* __restrict__ nll_terms, float* __restrict__ logq_terms,
                                   int32_t* __restrict__ status) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * T) return;
  const int t = idx % T, b = idx / T;
  const float mk = mask[idx];
  const int64_t base = (int64_t)b * 2 * T + t;
  float y = 0.f, v1 = 0.f;
  if (mk != 0.f) {
    const float zu = z_q[base + (int64_t)chu * T];
    v1 = z_q[base + (int64_t)ch1 * T];
    const float wv = w[idx];
    if (status) {
      if (!(fabsf(wv) <= 3.402823466e+38f)) atomicOr(status, WETTS_STATUS_DURATION_NONFINITE);
      else if (wv < 0.f) atomicOr(status, WETTS_STATUS_DURATION_NEGATIVE);
    }
    // sigmoid and log through double, each rounded once: w - u cancels, and the main flows scale y before a spline
    const float u = (float)(1.0 / (1.0 + exp(-(double)zu))) * mk;
    const float z0 = (wv - u) * mk;
    logq_terms[idx] = logq_terms[idx] - (logsigmoid_f(zu) + logsigmoid_f(-zu)) * mk;
    y = (float)log((double)fmaxf(z0, 1e-5f)) * mk;
    nll_terms[idx] = nll_terms[idx] + y;
  }
  z[base] = y;
  z[base + T] = v1;
}

int32_t k_dequant_log(const float* z_q, int chu, int ch1, const float* w, const float* mask, int B, int T, float* z,
                      float* nll_terms, float* logq_terms, int32_t* status, hipStream_t s) {
  if ((int64_t)B * T == 0) return WETTS_OK;
  hipLaunchKernelGGL(dequant_log_kernel, grid1d((int64_t)B * T, 256), dim3(256), 0, s, z_q, chu, ch1, w, mask, B, T, z,
                     nll_terms, logq_terms, status);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// post_pre: Conv1d(1, C, 1) of w [B,T] -> out [B,C,T] (duration_predictors.py:226).  w is read under the mask (the
// reference's w is zero behind an utterance; here nothing behind it is read).
__global__ void duration_pre_kernel(const float* __restrict__ w, const float* __restrict__ mask,
                                    const float* __restrict__ wt, const float* __restrict__ bias, int B, int C, int T,
                                    float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * C * T) return;
  const int t = (int)(idx % T);
  const int c = (int)((idx / T) % C);
  const int64_t bt = idx / ((int64_t)T * C) * T + t;
  const float wv = mask[bt] != 0.f ? w[bt] : 0.f;
  out[idx] = wt[c] * wv + bias[c];
}

int32_t k_duration_pre(const float* w, const float* mask, const float* wt, const float* bias, int B, int C, int T,
                       float* out, hipStream_t s) {
  const int64_t n = (int64_t)B * C * T;
  if (n == 0) return WETTS_OK;
  hipLaunchKernelGGL(duration_pre_kernel, grid1d(n, 256), dim3(256), 0, s, w, mask, wt, bias, B, C, T, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// out = a + b (the `g = x + h_w` of the posterior flows, :233, formed once)
__global__ void duration_add_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                    float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < n) out[idx] = a[idx] + b[idx];
}

int32_t k_duration_add(const float* a, const float* b, int64_t n, float* out, hipStream_t s) {
  if (n == 0) return WETTS_OK;
  hipLaunchKernelGGL(duration_add_kernel, grid1d(n, 256), dim3(256), 0, s, a, b, n, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// out[b, c, t] = src[b, c ^ swapped, t]: a stage tensor out of the flows in logical channel order
__global__ void duration_unswap_kernel(const float* __restrict__ src, int swapped, int B, int T,
                                       float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * 2 * T) return;
  const int t = (int)(idx % T);
  const int c = (int)((idx / T) % 2);
  const int64_t b = idx / ((int64_t)2 * T);
  out[idx] = src[(b * 2 + (c ^ swapped)) * T + t];
}

int32_t k_duration_unswap(const float* src, int swapped, int B, int T, float* out, hipStream_t s) {
  const int64_t n = (int64_t)B * 2 * T;
  if (n == 0) return WETTS_OK;
  hipLaunchKernelGGL(duration_unswap_kernel, grid1d(n, 256), dim3(256), 0, s, src, swapped, B, T, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// duration_predictors.py:240-242, 251-253 per utterance:
//   nll[b]  = sum_t mask * (nll_terms + 1/2 (log 2pi + z0^2) + 1/2 (log 2pi + z1^2)) - (logs0 + logs1) * len
//   logq[b] = sum_t mask * (logq_terms - 1/2 (log 2pi + e0^2) - 1/2 (log 2pi + e1^2)) - (qlogs0 + qlogs1) * len
// with `logs` of flows.0 and `qlogs` of post_flows.0 (ElementwiseAffine's logdet, :137), len = sum_t mask;
//   both[b] = nll + logq (what the module returns), per_utt[b] = both[b] / len.
__global__ void __launch_bounds__(kRedThreads)
duration_reduce_kernel(const float* __restrict__ nll_terms, const float* __restrict__ logq_terms,
                       const float* __restrict__ z, const float* __restrict__ e_q, const float* __restrict__ mask,
                       const float* __restrict__ logs, const float* __restrict__ qlogs, int T, float* __restrict__ nll,
                       float* __restrict__ logq, float* __restrict__ both, float* __restrict__ per_utt) {
  __shared__ float part[4];
  const int b = blockIdx.x;
  const float* mb = mask + (int64_t)b * T;
  const float* nt = nll_terms + (int64_t)b * T;
  const float* qt = logq_terms + (int64_t)b * T;
  const float* zb = z + (int64_t)b * 2 * T;
  const float* eb = e_q + (int64_t)b * 2 * T;
  float an[4] = {0.f, 0.f, 0.f, 0.f}, aq[4] = {0.f, 0.f, 0.f, 0.f};
  float cnt = 0.f;
  int k = 0;
  for (int t = threadIdx.x; t < T; t += kRedThreads) {
    const float mk = mb[t];
    if (mk == 0.f) continue;
    cnt += mk;
    const float z0 = zb[t], z1 = zb[T + t];
    const float e0 = eb[t] * mk, e1 = eb[T + t] * mk;
    an[k & 3] += (nt[t] + (0.5f * (kLog2Pi + z0 * z0) + 0.5f * (kLog2Pi + z1 * z1))) * mk;
    aq[k & 3] += (qt[t] + (-0.5f * (kLog2Pi + e0 * e0) + -0.5f * (kLog2Pi + e1 * e1))) * mk;
    ++k;
  }
  const float sn = block_sum((an[0] + an[1]) + (an[2] + an[3]), part);
  const float sq = block_sum((aq[0] + aq[1]) + (aq[2] + aq[3]), part);
  const float n = block_sum(cnt, part);
  if (threadIdx.x == 0) {
    const float vn = sn - (logs[0] + logs[1]) * n;
    const float vq = sq - (qlogs[0] + qlogs[1]) * n;
    nll[b] = vn;
    logq[b] = vq;
    both[b] = vn + vq;
    per_utt[b] = (vn + vq) / n;
  }
}

int32_t k_duration_reduce(const float* nll_terms, const float* logq_terms, const float* z, const float* e_q,
                          const float* mask, const float* logs, const float* qlogs, int B, int T, float* nll,
                          float* logq, float* both, float* per_utt, hipStream_t s) {
  WETTS_REQUIRE(B >= 1 && T >= 0, "duration_reduce: bad shape B=%d T=%d", B, T);
  hipLaunchKernelGGL(duration_reduce_kernel, dim3((unsigned)B), dim3(kRedThreads), 0, s, nll_terms, logq_terms, z, e_q,
                     mask, logs, qlogs, T, nll, logq, both, per_utt);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// models.py:203-206 per utterance (DurationPredictor models): logw_ = log(w + 1e-6) * mask, written out;
// rows[b] = sum_t (logw - logw_)^2, per_utt[b] = rows[b] / len.  Masked-out positions write 0 and read nothing of w.
__global__ void __launch_bounds__(kRedThreads)
dp_mse_kernel(const float* __restrict__ logw, const float* __restrict__ w, const float* __restrict__ mask, int T,
              float* __restrict__ target, float* __restrict__ rows, float* __restrict__ per_utt,
              int32_t* __restrict__ status) {
  __shared__ float part[4];
  const int b = blockIdx.x;
  const int64_t base = (int64_t)b * T;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float cnt = 0.f;
  int k = 0;
  for (int t = threadIdx.x; t < T; t += kRedThreads) {
    const float mk = mask[base + t];
    if (mk == 0.f) {
      target[base + t] = 0.f;
      continue;
    }
    cnt += mk;
    const float wv = w[base + t];
    if (status) {
      if (!(fabsf(wv) <= 3.402823466e+38f)) atomicOr(status, WETTS_STATUS_DURATION_NONFINITE);
      else if (wv < 0.f) atomicOr(status, WETTS_STATUS_DURATION_NEGATIVE);
    }
    const float tg = (float)log((double)(wv + 1e-6f)) * mk;  // the f32 sum's log, rounded once
    target[base + t] = tg;
    const float d = logw[base + t] - tg;
    acc[k & 3] += d * d;
    ++k;
  }
  const float sum = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), part);
  const float n = block_sum(cnt, part);
  if (threadIdx.x == 0) {
    rows[b] = sum;
    per_utt[b] = sum / n;
  }
}

int32_t k_dp_mse(const float* logw, const float* w, const float* mask, int B, int T, float* target, float* rows,
                 float* per_utt, int32_t* status, hipStream_t s) {
  WETTS_REQUIRE(B >= 1 && T >= 0, "dp_mse: bad shape B=%d T=%d", B, T);
  hipLaunchKernelGGL(dp_mse_kernel, dim3((unsigned)B), dim3(kRedThreads), 0, s, logw, w, mask, T, target, rows, per_utt,
                     status);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// logw_ = log(w + 1e-6) * mask alone (models.py:201, SDP models); masked-out positions write 0 and read nothing of w
__global__ void logw_target_kernel(const float* __restrict__ w, const float* __restrict__ mask, int64_t n,
                                   float* __restrict__ target) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float mk = mask[idx];
  target[idx] = mk != 0.f ? (float)log((double)(w[idx] + 1e-6f)) * mk : 0.f;
}

// ---------------------------------------------------------------------------------------------
// models.py:199 / :205-206 and train.py:485 (`loss_dur = torch.sum(l_length.float())`), one wave:
//   den = sum(x_mask) over the WHOLE batch (lane l adds elements l, l + 64, ... ascending, then the butterfly),
//   l_length[b] = rows[b] / den, total[0] = sum_b l_length[b] (same order over b), total[1] = weight * total[0].
__global__ void __launch_bounds__(64)
duration_total_kernel(const float* __restrict__ rows, const float* __restrict__ mask, int B, int64_t BT, float weight,
                      float* __restrict__ l_length, float* __restrict__ total) {
  float d = 0.f;
  for (int64_t i = threadIdx.x; i < BT; i += 64) d += mask[i];
  d = wave_sum(d);
  float a = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) {
    const float l = rows[b] / d;
    l_length[b] = l;
    a += l;
  }
  a = wave_sum(a);
  if (threadIdx.x == 0) {
    total[0] = a;
    total[1] = a * weight;
  }
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_duration_loss_total(const float* per_row, const float* x_mask, int32_t B, int32_t Tx, float weight,
                                  float* l_length, float* total, void* stream) {
  WETTS_REQUIRE(per_row && x_mask && l_length && total, "null argument");
  WETTS_REQUIRE(B >= 1 && Tx >= 0, "duration_loss_total: bad shape B=%d Tx=%d", B, Tx);
  hipLaunchKernelGGL(duration_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, per_row, x_mask, B,
                     (int64_t)B * Tx, weight, l_length, total);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t wetts_duration_logw_target(const float* w, const float* x_mask, int32_t B, int32_t Tx, float* logw_target,
                                   void* stream) {
  WETTS_REQUIRE(w && x_mask && logw_target, "null argument");
  WETTS_REQUIRE(B >= 0 && Tx >= 0, "duration_logw_target: bad shape B=%d Tx=%d", B, Tx);
  const int64_t n = (int64_t)B * Tx;
  if (n == 0) return WETTS_OK;
  hipLaunchKernelGGL(logw_target_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)stream, w, x_mask, n, logw_target);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---- the elementwise steps of wetts_duration_sdp_forward on given tensors (validation aids) ---------------------------
int32_t wetts_duration_affine_forward(const float* x, const float* m, const float* logs, const float* x_mask, int32_t B,
                                      int32_t Tx, float* out, void* stream) {
  WETTS_REQUIRE(x && m && logs && x_mask && out, "null argument");
  WETTS_REQUIRE(B >= 0 && Tx >= 0, "bad shape");
  return k_affine_forward(x, m, logs, x_mask, B, Tx, out, (hipStream_t)stream);
}

int32_t wetts_duration_spline_forward(float* z, int32_t ch0, const float* h, const float* x_mask, float div, int32_t B,
                                      int32_t Tx, float sign, float* acc, void* stream) {
  WETTS_REQUIRE(z && h && x_mask && acc, "null argument");
  WETTS_REQUIRE(B >= 0 && Tx >= 0 && (ch0 == 0 || ch0 == 1) && div > 0.f, "bad argument");
  return k_spline_forward(z, ch0, 1 - ch0, h, x_mask, 10, 5.0f, div, B, Tx, sign, acc, (hipStream_t)stream);
}

int32_t wetts_duration_dequant_log(const float* z_q, int32_t chu, const float* w, const float* x_mask, int32_t B,
                                   int32_t Tx, float* z, float* nll_terms, float* logq_terms, int32_t* status_dev,
                                   void* stream) {
  WETTS_REQUIRE(z_q && w && x_mask && z && nll_terms && logq_terms, "null argument");
  WETTS_REQUIRE(B >= 0 && Tx >= 0 && (chu == 0 || chu == 1), "bad argument");
  return k_dequant_log(z_q, chu, 1 - chu, w, x_mask, B, Tx, z, nll_terms, logq_terms, status_dev, (hipStream_t)stream);
}

int32_t wetts_duration_pre(const float* w, const float* x_mask, const float* weight, const float* bias, int32_t B,
                           int32_t C, int32_t Tx, float* out, void* stream) {
  WETTS_REQUIRE(w && x_mask && weight && bias && out, "null argument");
  WETTS_REQUIRE(B >= 0 && C >= 1 && Tx >= 0, "bad shape");
  return k_duration_pre(w, x_mask, weight, bias, B, C, Tx, out, (hipStream_t)stream);
}

}  // extern "C"
