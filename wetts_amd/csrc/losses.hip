// Teacher-forced reconstruction (SynthesizerTrn.forward, models.py:214-216, and the two reconstruction losses of
// train.py:402-432,486-488): the random decoder slice and the KL / L1 reductions.  All f32, wave64, on the caller's stream.
//
// Reduction order.  No floating-point atomics anywhere: a sum is formed in an order that is a function of the data's
// own extent alone.
//   * per utterance: ONE block of 256 threads.  Thread i owns the time steps (kl) or elements (l1) i, i + 256, ... and
//     adds them in ascending order into four interleaved accumulators (channel c -> accumulator c & 3 for kl, visit
//     k -> k & 3 for l1), which bounds the serial chain at a quarter of the visits; (a0 + a1) + (a2 + a3), then a
//     butterfly over the 64 lanes, then (w0 + w1) + (w2 + w3) over the four waves through LDS;
//   * a masked-out term is skipped, not added as zero, and padding lies behind an utterance's own frames: so which terms a
//     thread adds, and in which order, does not depend on the padded length -- a row alone and the same row inside a
//     padded batch give the same bits (the property the alignment kernels have);
//   * batch total: one wave; lane l adds the partials of rows l, l + 64, ... in ascending order, then the butterfly.
#include "kernels.h"

namespace wetts {

namespace {

constexpr int kRedThreads = 256;

// every lane gets the sum of the 64 lanes, formed in one fixed butterfly order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the block's 256 threads, valid in thread 0; `part` is 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* part) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (part[0] + part[1]) + (part[2] + part[3]);
  __syncthreads();
  return r;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// commons.py:54-56: ids = (u * float(len - segment + 1)).long(), the f32 product truncated toward zero, then clamped
// into [0, len - segment] (u = 1.0, which a caller's draw may hold, would give len - segment + 1).  ids_in: ids given by the
// caller, checked against the same range.  A row shorter than the segment, or an id out of range, is flagged.
__global__ void slice_ids_kernel(const float* __restrict__ u, const int64_t* __restrict__ ids_in,
                                 const int64_t* __restrict__ lengths, int B, int T, int segment,
                                 int64_t* __restrict__ ids, int32_t* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int64_t len = lengths ? lengths[b] : (int64_t)T;
  len = len < 0 ? 0 : (len > T ? T : len);
  const int64_t last = len - segment;  // the largest valid id
  int64_t id = 0;
  bool bad = last < 0;
  if (!bad) {
    if (ids_in) {
      id = ids_in[b];
      if (id < 0 || id > last) {
        bad = true;
        id = id < 0 ? 0 : last;
      }
    } else {
      id = (int64_t)(u[b] * (float)(last + 1));
      id = id < 0 ? 0 : (id > last ? last : id);
    }
  }
  ids[b] = id;
  if (bad && status) atomicOr(status, WETTS_STATUS_SEGMENT_LONGER);
}

int32_t k_slice_ids(const float* u, const int64_t* ids_in, const int64_t* lengths, int B, int T, int segment,
                    int64_t* ids, int32_t* status, hipStream_t s) {
  if (B == 0) return WETTS_OK;
  hipLaunchKernelGGL(slice_ids_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, s, u, ids_in, lengths, B, T, segment,
                     ids, status);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// commons.py:41-47: out[b, c, j] = x[b, c, ids[b] * scale + j], j < L = segment * scale.  One thread writes V
// consecutive outputs.  V = 4 needs L % 4 == 0 and a 16-byte aligned `out` (the launcher checks both: every output row
// then starts on 16 bytes); the LOAD is 16 bytes wide only where the source address is too, which also depends on the
// row's start -- src_vec says that base and strides allow it, the start is looked at here.  The start is clamped into
// [0, T - L]: an id the ids kernel flagged reads inside the tensor.
template <int V>
__global__ void slice_segments_kernel(const float* __restrict__ x, int64_t x_bs, int64_t x_cs,
                                      const int64_t* __restrict__ ids, int64_t total, int C, int T, int L, int scale,
                                      int src_vec, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int per_row = L / V;
  const int64_t row = idx / per_row;
  const int j = (int)(idx - row * per_row) * V;
  const int64_t b = row / C;
  const int c = (int)(row - b * C);
  int64_t start = ids[b] * (int64_t)scale;
  const int64_t hi = (int64_t)T - L;
  start = start < 0 ? 0 : (start > hi ? hi : start);
  const float* src = x + b * x_bs + c * x_cs + start + j;
  float* dst = out + row * L + j;
  if (V == 4) {
    float4 v;
    if (src_vec && (start & 3) == 0) {
      v = *reinterpret_cast<const float4*>(src);
    } else {
      v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3];
    }
    *reinterpret_cast<float4*>(dst) = v;
  } else {
    dst[0] = src[0];
  }
}

int32_t k_slice_segments(const float* x, int64_t x_bs, int64_t x_cs, const int64_t* ids, int B, int C, int T,
                         int segment, int scale, float* out, hipStream_t s) {
  const int64_t L64 = (int64_t)segment * scale;
  WETTS_REQUIRE(C >= 1 && segment >= 1 && scale >= 1, "slice_segments: C, segment and scale must be positive");
  WETTS_REQUIRE(L64 <= T, "slice_segments: segment * scale = %lld exceeds the %d time steps of x", (long long)L64, T);
  if (B == 0) return WETTS_OK;
  const int L = (int)L64;
  const bool vec = (L & 3) == 0 && ((uintptr_t)out & 15) == 0;
  const int src_vec = ((uintptr_t)x & 15) == 0 && (x_bs & 3) == 0 && (x_cs & 3) == 0;
  const int64_t total = (int64_t)B * C * (vec ? L / 4 : L);
  const int64_t blocks = (total + 255) / 256;
  WETTS_REQUIRE(blocks <= 0x7fffffff, "slice_segments: too many elements for one launch");
  if (blocks == 0) return WETTS_OK;
  const dim3 grid((unsigned)blocks);
  if (vec)
    hipLaunchKernelGGL(slice_segments_kernel<4>, grid, dim3(256), 0, s, x, x_bs, x_cs, ids, total, C, T, L, scale,
                       src_vec, out);
  else
    hipLaunchKernelGGL(slice_segments_kernel<1>, grid, dim3(256), 0, s, x, x_bs, x_cs, ids, total, C, T, L, scale,
                       src_vec, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// losses.py:56-59 per utterance: sums[b] = sum_{c,t} mask * (logs_p - logs_q - 1/2 + 1/2 (z_p - m_p)^2 exp(-2 logs_p)),
// frames[b] = sum_t mask.  Consecutive threads read consecutive t of one channel row.
__global__ void __launch_bounds__(kRedThreads)
kl_rows_kernel(const float* __restrict__ z_p, const float* __restrict__ logs_q, const float* __restrict__ m_p,
               const float* __restrict__ logs_p, const float* __restrict__ mask, int I, int T,
               float* __restrict__ sums, float* __restrict__ frames, float* __restrict__ per_utt) {
  __shared__ float part[4];
  const int b = blockIdx.x;
  const int64_t base = (int64_t)b * I * T;
  const float* mb = mask + (int64_t)b * T;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float cnt = 0.f;
  for (int t = threadIdx.x; t < T; t += kRedThreads) {
    const float mk = mb[t];
    if (mk == 0.f) continue;
    cnt += mk;
    for (int c = 0; c < I; ++c) {
      const int64_t i = base + (int64_t)c * T + t;
      const float lp = logs_p[i], d = z_p[i] - m_p[i];
      float kl = lp - logs_q[i] - 0.5f;
      kl += 0.5f * (d * d) * expf(-2.0f * lp);
      acc[c & 3] += kl * mk;
    }
  }
  const float sum = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), part);
  const float n = block_sum(cnt, part);
  if (threadIdx.x == 0) {
    sums[b] = sum;
    frames[b] = n;
    per_utt[b] = sum / n;
  }
}

// total[0] = (sum_b num[b]) / (den ? sum_b den[b] : den_const), both sums in the fixed order of the file comment;
// total[1] = total[0] * weight
__global__ void __launch_bounds__(64)
ratio_total_kernel(const float* __restrict__ num, const float* __restrict__ den, float den_const, float weight, int B,
                   float* __restrict__ total) {
  float a = 0.f, d = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) {
    a += num[b];
    if (den) d += den[b];
  }
  a = wave_sum(a);
  d = wave_sum(d);
  if (threadIdx.x == 0) {
    const float r = a / (den ? d : den_const);
    total[0] = r;
    total[1] = r * weight;
  }
}

int32_t k_kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, const float* mask,
                  int B, int I, int T, float weight, float* partials, float* per_utt, float* total, hipStream_t s) {
  WETTS_REQUIRE(B >= 1 && B <= 0x7fffffff / 2 && I >= 1 && T >= 0, "kl_loss: bad shape B=%d I=%d T=%d", B, I, T);
  hipLaunchKernelGGL(kl_rows_kernel, dim3((unsigned)B), dim3(kRedThreads), 0, s, z_p, logs_q, m_p, logs_p, mask, I, T,
                     partials, partials + B, per_utt);
  WETTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(ratio_total_kernel, dim3(1), dim3(64), 0, s, (const float*)partials, (const float*)(partials + B),
                     0.f, weight, B, total);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// F.l1_loss (mean) per row: sums[b] = sum_i |a[b,i] - b[b,i]|, per_utt[b] = sums[b] / N.
__global__ void __launch_bounds__(kRedThreads)
l1_rows_kernel(const float* __restrict__ a, const float* __restrict__ bb, int64_t N, float* __restrict__ sums,
               float* __restrict__ per_utt) {
  __shared__ float part[4];
  const int b = blockIdx.x;
  const float* pa = a + (int64_t)b * N;
  const float* pb = bb + (int64_t)b * N;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (int64_t i = threadIdx.x; i < N; i += kRedThreads, ++k) acc[k & 3] += fabsf(pa[i] - pb[i]);
  const float sum = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), part);
  if (threadIdx.x == 0) {
    sums[b] = sum;
    per_utt[b] = sum / (float)N;
  }
}

int32_t k_l1_loss(const float* a, const float* b, int B, int64_t N, float weight, float* partials, float* per_utt,
                  float* total, hipStream_t s) {
  WETTS_REQUIRE(B >= 1 && N >= 1, "l1_loss: bad shape B=%d N=%lld", B, (long long)N);
  hipLaunchKernelGGL(l1_rows_kernel, dim3((unsigned)B), dim3(kRedThreads), 0, s, a, b, N, partials, per_utt);
  WETTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(ratio_total_kernel, dim3(1), dim3(64), 0, s, (const float*)partials, (const float*)nullptr,
                     (float)B * (float)N, weight, B, total);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_slice_ids(const float* u, const int64_t* ids_in, const int64_t* lengths, int32_t B, int32_t T,
                        int32_t segment, int64_t* ids, int32_t* status_dev, void* stream) {
  WETTS_REQUIRE(ids && (u || ids_in), "null argument");
  WETTS_REQUIRE(B >= 0 && T >= 0 && segment >= 1, "slice_ids: bad shape B=%d T=%d segment=%d", B, T, segment);
  return k_slice_ids(u, ids_in, lengths, B, T, segment, ids, status_dev, (hipStream_t)stream);
}

int32_t wetts_slice_segments(const float* x, int64_t x_batch_stride, int64_t x_channel_stride, const int64_t* ids,
                             int32_t B, int32_t C, int32_t T, int32_t segment, int32_t scale, float* out,
                             void* stream) {
  WETTS_REQUIRE(x && ids && out, "null argument");
  WETTS_REQUIRE(B >= 0 && T >= 0, "slice_segments: negative size");
  return k_slice_segments(x, x_batch_stride, x_channel_stride, ids, B, C, T, segment, scale, out, (hipStream_t)stream);
}

int32_t wetts_kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p,
                      const float* z_mask, int32_t B, int32_t I, int32_t T, float weight, float* partials,
                      float* per_utt, float* total, void* stream) {
  WETTS_REQUIRE(z_p && logs_q && m_p && logs_p && z_mask && partials && per_utt && total, "null argument");
  return k_kl_loss(z_p, logs_q, m_p, logs_p, z_mask, B, I, T, weight, partials, per_utt, total, (hipStream_t)stream);
}

int32_t wetts_l1_loss(const float* a, const float* b, int32_t B, int64_t N, float weight, float* partials,
                      float* per_utt, float* total, void* stream) {
  WETTS_REQUIRE(a && b && partials && per_utt && total, "null argument");
  return k_l1_loss(a, b, B, N, weight, partials, per_utt, total, (hipStream_t)stream);
}

}  // extern "C"
