// Forced alignment (SynthesizerTrn.forward, models.py:171-212, without gradients): the alignment scores that feed the
// monotonic alignment search (mas.hip), and the two small kernels around the search.
//
// neg_cent (models.py:173-184) is, per utterance, one GEMM  D[Ty x Tx] = A[Ty x 2I] * B[2I x Tx]  plus a per-column
// constant:
//   neg_cent[t][s] = sum_c ( -1/2 log 2pi - logs_p[c][s] - 1/2 (z_p[c][t] - m_p[c][s])^2 exp(-2 logs_p[c][s]) )
//                  = sum_c ( (-1/2 z^2) * r  +  z * (m r) )  +  sum_c ( -1/2 log 2pi - logs - 1/2 m^2 r ),   r = exp(-2 logs)
// The reference computes it as two matmuls and two column sums through four [B,I,.] / [B,Ty,Tx] intermediates.  Here
// one v_mfma_f32_32x32x2_f32 step is ONE channel: k = 0 carries (-1/2 z^2, r), k = 1 carries (z, m r), so the lane halves
// of the MFMA operand layout (k = lane >> 5) are the two kinds of term.  Both operands are built from z_p and `stats`
// on the way into LDS and exist nowhere else; the column constant is accumulated by the threads that stage B, from the
// values they already hold, and added in the epilogue.
//
// A block of four waves owns a 64-frame x 64-phoneme tile (each wave one 32 x 32 MFMA tile) and walks the channels in
// chunks of 16.  The next chunk's raw values are fetched into registers before the MFMAs of the current one, so the
// global loads fly under the matrix work.  Every cell's arithmetic is a function of its own (t, s) and the channel
// order alone: a row computed alone and the same row inside a padded batch are bit-identical.
// Cells of padded frames / phonemes hold whatever the zero-masked inputs give (finite); the search never reads them.
#include "kernels.h"

namespace wetts {

typedef float f32x16a __attribute__((ext_vector_type(16)));

namespace {
constexpr int kAlTile = 64;   // frames and phonemes per block
constexpr int kAlCK = 16;     // channels per LDS chunk
constexpr int kAlPer = kAlCK * kAlTile / 256;  // (channel, column) cells a thread stages per operand and chunk: 4
}  // namespace

__global__ void __launch_bounds__(256)
align_scores_kernel(const float* __restrict__ z_p, const float* __restrict__ stats, int I, int Tx, int Ty,
                    float* __restrict__ neg_cent) {
  // [channel][k kind][row or column]: lane l of a wave reads [c][l >> 5][tile * 32 + (l & 31)], 32 consecutive words
  __shared__ float As[kAlCK][2][kAlTile];
  __shared__ float Bs[kAlCK][2][kAlTile];
  __shared__ float cpart[4][kAlTile];
  const int b = blockIdx.z;
  const int s0 = blockIdx.x * kAlTile, t0 = blockIdx.y * kAlTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 63, crow = tid >> 6;  // staging: column `col`, channels crow + 4 j of the chunk
  const float* zb = z_p + (int64_t)b * I * Ty;
  const float* mb = stats + (int64_t)b * 2 * I * Tx;
  const float* lb = mb + (int64_t)I * Tx;
  const bool t_ok = t0 + col < Ty, s_ok = s0 + col < Tx;
  const float kHalfLog2Pi = 0.91893853320467274178f;

  float zr[kAlPer], mr[kAlPer], lr[kAlPer];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int j = 0; j < kAlPer; ++j) {
      const int c = c0 + crow + 4 * j;
      const bool c_ok = c < I;
      zr[j] = (c_ok && t_ok) ? zb[(int64_t)c * Ty + t0 + col] : 0.f;
      mr[j] = (c_ok && s_ok) ? mb[(int64_t)c * Tx + s0 + col] : 0.f;
      lr[j] = (c_ok && s_ok) ? lb[(int64_t)c * Tx + s0 + col] : 0.f;
    }
  };

  f32x16a acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float csum = 0.f;  // this thread's share of the column constant
  const int wm = wave >> 1, wn = wave & 1;
  const int half = lane >> 5;
  const int arow = wm * 32 + (lane & 31), bcol = wn * 32 + (lane & 31);

  fetch(0);
  for (int c0 = 0; c0 < I; c0 += kAlCK) {
#pragma unroll
    for (int j = 0; j < kAlPer; ++j) {
      const int cc = crow + 4 * j;
      const bool live = (c0 + cc < I) && s_ok;  // channels past I and columns past Tx contribute nothing
      const float z = zr[j], m = mr[j], ls = lr[j];
      const float r = live ? expf(-2.f * ls) : 0.f;
      const float mrr = m * r;
      As[cc][0][col] = -0.5f * z * z;
      As[cc][1][col] = z;
      Bs[cc][0][col] = r;
      Bs[cc][1][col] = mrr;
      if (live) csum += (-kHalfLog2Pi - ls) - 0.5f * m * mrr;
    }
    __syncthreads();
    if (c0 + kAlCK < I) fetch(c0 + kAlCK);
#pragma unroll
    for (int cc = 0; cc < kAlCK; ++cc)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[cc][half][arow], Bs[cc][half][bcol], acc, 0, 0, 0);
    __syncthreads();
  }
  cpart[crow][col] = csum;
  __syncthreads();
  const float cst = (cpart[0][bcol] + cpart[1][bcol]) + (cpart[2][bcol] + cpart[3][bcol]);

  // lane holds rows 8 g + 4 (lane >> 5) + {0..3} of column lane & 31 (the 32x32 MFMA output layout)
  const int s = s0 + bcol;
  if (s >= Tx) return;
  float* ob = neg_cent + (int64_t)b * Ty * Tx;
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + wm * 32 + 8 * g + 4 * half + i;
      if (t < Ty) ob[(int64_t)t * Tx + s] = acc[4 * g + i] + cst;
    }
}

int32_t k_align_scores(const float* z_p, const float* stats, int B, int I, int Tx, int Ty, float* neg_cent,
                       hipStream_t s) {
  if (B == 0 || Tx == 0 || Ty == 0) return WETTS_OK;
  WETTS_REQUIRE(I >= 1, "align_scores: inter_channels must be positive");
  WETTS_REQUIRE(B <= 65535 && cdiv(Ty, kAlTile) <= 65535, "align_scores: batch or frame count too large for one launch");
  const dim3 grid((unsigned)cdiv(Tx, kAlTile), (unsigned)cdiv(Ty, kAlTile), (unsigned)B);
  hipLaunchKernelGGL(align_scores_kernel, grid, dim3(256), 0, s, z_p, stats, I, Tx, Ty, neg_cent);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// int64 lengths -> the int32 (t_y, t_x) pairs wetts_mas takes, clamped into the padded shape; an utterance with more
// phonemes than frames has no monotonic alignment (the reference's search returns a meaningless path): flagged.
__global__ void align_lengths_kernel(const int64_t* __restrict__ x_lengths, const int64_t* __restrict__ y_lengths,
                                     int B, int Tx, int Ty, int32_t* __restrict__ t_xs, int32_t* __restrict__ t_ys,
                                     int32_t* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int64_t tx = x_lengths[b], ty = y_lengths[b];
  tx = tx < 0 ? 0 : (tx > Tx ? Tx : tx);
  ty = ty < 0 ? 0 : (ty > Ty ? Ty : ty);
  t_xs[b] = (int32_t)tx;
  t_ys[b] = (int32_t)ty;
  if (tx > ty && status) atomicOr(status, WETTS_STATUS_ALIGN_TEXT_LONGER);
}

int32_t k_align_lengths(const int64_t* x_lengths, const int64_t* y_lengths, int B, int Tx, int Ty, int32_t* t_xs,
                        int32_t* t_ys, int32_t* status, hipStream_t s) {
  if (B == 0) return WETTS_OK;
  hipLaunchKernelGGL(align_lengths_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, s, x_lengths, y_lengths, B, Tx, Ty,
                     t_xs, t_ys, status);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// path -> durations (models.py:196 `w = attn.sum(2)`): one block per utterance.  Every wave scans whole rows of the
// 0/1 path: the first 1 of a row is the frame's phoneme (frame2phone, -1 for a row without one), every 1 counts into a
// per-phoneme LDS histogram, and the row goes out as float when the caller wants the dense attn.  Wave 0 then writes
// w and its inclusive cumsum (exact integers in float, the form wetts_length_regulate reads).
__global__ void __launch_bounds__(256)
path_to_durations_kernel(const int32_t* __restrict__ path, const int32_t* __restrict__ t_ys,
                         const int32_t* __restrict__ t_xs, int Tx, int Ty, float* __restrict__ w,
                         float* __restrict__ cum, int32_t* __restrict__ f2p, float* __restrict__ attn) {
  extern __shared__ int32_t hist[];  // [Tx]
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t_y = min(max(t_ys[b], 0), Ty), t_x = min(max(t_xs[b], 0), Tx);
  const int32_t* pb = path + (int64_t)b * Ty * Tx;
  for (int x = threadIdx.x; x < Tx; x += blockDim.x) hist[x] = 0;
  __syncthreads();
  for (int y = wave; y < Ty; y += 4) {
    const bool row_ok = y < t_y;
    int first = 0x7fffffff;
    for (int x0 = 0; x0 < Tx; x0 += 64) {
      const int x = x0 + lane;
      const bool one = row_ok && x < t_x && pb[(int64_t)y * Tx + x] != 0;
      if (one) {
        atomicAdd(&hist[x], 1);
        first = min(first, x);
      }
      if (attn && x < Tx) attn[((int64_t)b * Ty + y) * Tx + x] = one ? 1.f : 0.f;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    if (lane == 0) f2p[(int64_t)b * Ty + y] = first == 0x7fffffff ? -1 : first;
  }
  __syncthreads();
  if (wave != 0) return;
  float carry = 0.f;
  for (int x0 = 0; x0 < Tx; x0 += 64) {
    const int x = x0 + lane;
    const float wv = x < Tx ? (float)hist[x] : 0.f;
    if (x < Tx) w[(int64_t)b * Tx + x] = wv;
    float v = wv;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float n = __shfl_up(v, off, 64);
      if (lane >= off) v += n;
    }
    v += carry;
    if (x < Tx) cum[(int64_t)b * Tx + x] = v;
    carry = __shfl(v, 63, 64);
  }
}

int32_t k_path_to_durations(const int32_t* path, const int32_t* t_ys, const int32_t* t_xs, int B, int Tx, int Ty,
                            float* w, float* cum, int32_t* frame2phone, float* attn, hipStream_t s) {
  if (B == 0) return WETTS_OK;
  WETTS_REQUIRE(Tx >= 0 && Ty >= 0 && Tx <= 16384, "path_to_durations: Tx=%d outside [0, 16384]", Tx);
  hipLaunchKernelGGL(path_to_durations_kernel, dim3((unsigned)B), dim3(256), (size_t)max(Tx, 1) * sizeof(int32_t), s,
                     path, t_ys, t_xs, Tx, Ty, w, cum, frame2phone, attn);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// ---------------------------------------------------------------------------------------------
// given integer frame counts -> what durations_kernel (kernels.hip) writes from predicted durations: w_ceil = the
// masked counts, their inclusive cumsum, y_lengths = clamp_min(sum, 1).  No exp(log(d)) round trip: the counts are
// taken as they are.  A negative count under the mask is flagged and taken as 0.
__global__ __launch_bounds__(64) void counts_kernel(const int64_t* __restrict__ counts, const float* __restrict__ mask,
                                                    int T, float* __restrict__ w_ceil, float* __restrict__ cum,
                                                    int64_t* __restrict__ y_lengths, int32_t* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float carry = 0.f;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    float wc = 0.f;
    if (t < T) {
      const int64_t n = counts[(int64_t)b * T + t];
      const bool on = mask[(int64_t)b * T + t] != 0.f;
      if (on && n < 0 && status) atomicOr(status, WETTS_STATUS_DURATION_NEGATIVE);
      wc = (on && n > 0) ? (float)n : 0.f;
      w_ceil[(int64_t)b * T + t] = wc;
    }
    float v = wc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float n = __shfl_up(v, off, 64);
      if (lane >= off) v += n;
    }
    v += carry;
    if (t < T) cum[(int64_t)b * T + t] = v;
    carry = __shfl(v, 63, 64);
  }
  if (lane == 0) {
    float tot = carry < 1.f ? 1.f : carry;  // clamp_min(sum, 1)
    if (!(tot <= 9.0e15f)) {                // as durations_kernel: a total no int64 frame count can hold
      if (status) atomicOr(status, WETTS_STATUS_DURATION_NONFINITE);
      tot = 1.f;
    }
    y_lengths[b] = (int64_t)tot;
  }
}

int32_t k_counts_to_lengths(const int64_t* counts, const float* mask, int B, int T, float* w_ceil, float* cum,
                            int64_t* y_lengths, int32_t* status, hipStream_t s) {
  if (B == 0) return WETTS_OK;
  hipLaunchKernelGGL(counts_kernel, dim3((unsigned)B), dim3(64), 0, s, counts, mask, T, w_ceil, cum, y_lengths, status);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // namespace wetts
