// MultiPeriodDiscriminator (discriminators.py:21-124,228-254, use_spectral_norm = false) without gradients, and the three
// adversarial losses of losses.py:6-42.  All f32, wave64, on the caller's stream.
//
// Layout.  y and y_hat run as ONE batch of 2B utterances (real first), so every weight is fetched once.  DiscriminatorS
// works on [2B][C][T'].  DiscriminatorP(p) works on [rows = 2B * p][C][H]: row (b, w) is the 1-D sequence x[b, h * p + w],
// which turns every (k,1) / (s,1) Conv2d into a plain strided Conv1d over independent rows; the reference's
// [2B, C, H, p] is a permuted view of that buffer.  conv_post alone stores in the reference's order [2B][H][p], so its
// flattened output is contiguous.  Every layer's output is an fmap the caller owns: there is no workspace.
//
// Every output element's arithmetic is a function of its own row, position and the channel order alone (a row resolves
// its zero padding at its own H; an MFMA column accumulates its own k sequence), so a row alone and the same row inside a
// batch give the same bits, and the real half does not depend on what it is paired with.
//
// Reduction order: that of csrc/losses.hip, carried in float64.  One block of 256 threads per (item,
// utterance): thread i adds the elements i, i + 256, ... of the utterance's own contiguous block in ascending order into
// four interleaved accumulators, (a0 + a1) + (a2 + a3), the butterfly over the lanes, (w0 + w1) + (w2 + w3) over the
// waves.  The totals launch is one wave: per item, lane l adds the rows l, l + 64, ... then the butterfly; items are added
// in ascending order.  No floating-point atomics.  Each term is formed in f32 as the reference forms it; the SUMS are
// float64 and round to f32 once, at the store: the scalar losses then carry the feature maps' error and nothing of their
// own (an f32 chain over 37 layer means alone would spend half of the 4-ulp gate the oracle's floor leaves).
#include "kernels.h"

#include <vector>

namespace wetts {

typedef float f32x16d __attribute__((ext_vector_type(16)));

constexpr float kSlope = 0.1f;  // modules.LRELU_SLOPE
constexpr int kNumDisc = 6, kNumFmaps = 37;  // S: 6 convs + conv_post, each P: 5 convs + conv_post

__device__ __forceinline__ float lrelu(float v) { return v >= 0.f ? v : kSlope * v; }

// ---------------------------------------------------------------------------------------------
// Reflect pad to a multiple of p (discriminators.py:81-84), the fold, and conv 0 (1 -> 32, k 5, stride 3, pad 2) +
// leaky-relu in one pass over the waveform.  One thread per (row, h): five samples in, 32 channels out.
constexpr int kC0 = 32;

__global__ void __launch_bounds__(64)
period_fold_conv0_kernel(const float* __restrict__ y, const float* __restrict__ y_hat, int split, int T, int p, int H0,
                         int H1, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ float ws[kC0 * 5 + kC0];
  for (int i = threadIdx.x; i < kC0 * 5 + kC0; i += 64) ws[i] = i < kC0 * 5 ? w[i] : bias[i - kC0 * 5];
  __syncthreads();
  const int row = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H1) return;
  const int b = row / p, wv = row - b * p;
  const float* src = b < split ? y + (int64_t)b * T : y_hat + (int64_t)(b - split) * T;
  float v[5];
#pragma unroll
  for (int tap = 0; tap < 5; ++tap) {
    const int hin = h * 3 + tap - 2;
    float s = 0.f;
    if (hin >= 0 && hin < H0) {
      int t = hin * p + wv;
      if (t >= T) t = 2 * T - 2 - t;  // F.pad(..., "reflect") on the right; the host guarantees n_pad < T
      s = src[t];
    }
    v[tap] = s;
  }
  float* o = out + (int64_t)row * kC0 * H1 + h;
#pragma unroll 4
  for (int c = 0; c < kC0; ++c) {
    float a = 0.f;
#pragma unroll
    for (int tap = 0; tap < 5; ++tap) a = __builtin_fmaf(ws[c * 5 + tap], v[tap], a);
    o[(int64_t)c * H1] = lrelu(a + ws[kC0 * 5 + c]);
  }
}

// ---------------------------------------------------------------------------------------------
// f32 implicit-GEMM Conv1d, k 5, pad 2, stride STRIDE, over independent rows, + bias + leaky-relu:
//   D[Cout x (rows * Hout)] = W[Cout x (Cin * 5)] * B,   B[(ci, tap)][(row, h)] = x[row][ci][h * STRIDE + tap - 2]
// The GEMM's columns are the (row, h) pairs of ALL rows laid end to end, so the short rows of the deep layers
// (H = 10 for p = 11 at 8192 samples) still fill a 64-column tile; each column resolves the padding at its own row's Hin.
// A block of four waves owns 128 channels x 64 columns (a wave: two 32 x 32 MFMA tiles sharing one B operand) and
// walks Cin in chunks of 16 = 80 k values = 40 v_mfma_f32_32x32x2_f32 steps.  The weights of a chunk are 80 contiguous
// floats per channel in the natural [Cout][Cin][5] layout (no packing); rows of As are padded to 81 words, so the 32
// lanes of an A read hit 32 banks.  The next chunk is fetched into registers before the current chunk's MFMAs.  The sum
// over Cin is blocked by chunk (see the loop), which keeps the f32 rounding of a 5120-term sum near that of a short one.
// 62 KB of LDS: two blocks per CU, two waves per SIMD.
constexpr int kDM = 128, kDN = 64, kDCK = 16, kDK = kDCK * 5, kDALd = kDK + 1;

template <int STRIDE>
__global__ void __launch_bounds__(256)
strided_conv_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                         float* __restrict__ out, int64_t ncols, int Cin, int Cout, int Hin, int Hout) {
  __shared__ float As[kDM][kDALd];
  __shared__ float Bs[kDK][kDN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * kDM;
  const int64_t n0 = (int64_t)blockIdx.x * kDN;

  // B staging: this thread's column, channels cg + 4 jj of the chunk, all five taps
  const int scol = tid & 63, cg = tid >> 6;
  const int64_t sj = n0 + scol;
  const bool s_ok = sj < ncols;
  const int64_t srow = s_ok ? sj / Hout : 0;
  const int sh = s_ok ? (int)(sj - srow * Hout) : 0;
  const int hb = sh * STRIDE - 2;
  const float* xb = x + srow * Cin * Hin;
  bool tap_ok[5];
#pragma unroll
  for (int tap = 0; tap < 5; ++tap) tap_ok[tap] = s_ok && hb + tap >= 0 && hb + tap < Hin;

  float4 ar[10];
  float br[20];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int idx = tid + 256 * j, r = idx / 20, q = idx - r * 20;
      ar[j] = *reinterpret_cast<const float4*>(w + ((int64_t)(m0 + r) * Cin + c0) * 5 + q * 4);
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const float* xc = xb + (int64_t)(c0 + cg + 4 * jj) * Hin;
#pragma unroll
      for (int tap = 0; tap < 5; ++tap) br[jj * 5 + tap] = tap_ok[tap] ? xc[hb + tap] : 0.f;
    }
  };

  f32x16d zero;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero[r] = 0.f;
  f32x16d acc0 = zero, acc1 = zero;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
  const int arow = wm * 64 + (lane & 31), bcol = wn * 32 + (lane & 31);

  fetch(0);
  for (int c0 = 0; c0 < Cin; c0 += kDCK) {
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int idx = tid + 256 * j, r = idx / 20, q = idx - r * 20;
      As[r][q * 4 + 0] = ar[j].x;
      As[r][q * 4 + 1] = ar[j].y;
      As[r][q * 4 + 2] = ar[j].z;
      As[r][q * 4 + 3] = ar[j].w;
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int tap = 0; tap < 5; ++tap) Bs[(cg + 4 * jj) * 5 + tap][scol] = br[jj * 5 + tap];
    __syncthreads();
    if (c0 + kDCK < Cin) fetch(c0 + kDCK);
    // blocked summation: a chunk's 80 products meet in accumulators of their own, which then join the running sum --
    // 64 + 40 roundings on the longest chain (Cin = 1024) where one chain would have 2560
    f32x16d c0v = zero, c1v = zero;
#pragma unroll 8
    for (int kk = 0; kk < kDK / 2; ++kk) {
      const float b = Bs[2 * kk + half][bcol];
      c0v = __builtin_amdgcn_mfma_f32_32x32x2f32(As[arow][2 * kk + half], b, c0v, 0, 0, 0);
      c1v = __builtin_amdgcn_mfma_f32_32x32x2f32(As[arow + 32][2 * kk + half], b, c1v, 0, 0, 0);
    }
    acc0 += c0v;
    acc1 += c1v;
    __syncthreads();
  }

  // lane holds rows 8 g + 4 (lane >> 5) + {0..3} of column lane & 31 (the 32x32 MFMA output layout)
  const int64_t j = n0 + bcol;
  if (j >= ncols) return;
  const int64_t row = j / Hout;
  const int h = (int)(j - row * Hout);
  float* ob = out + row * Cout * Hout + h;
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = m0 + wm * 64 + 8 * g + 4 * half + i;
      ob[(int64_t)co * Hout] = lrelu(acc0[4 * g + i] + bias[co]);
      ob[(int64_t)(co + 32) * Hout] = lrelu(acc1[4 * g + i] + bias[co + 32]);
    }
}

// ---------------------------------------------------------------------------------------------
// conv_post (1024 -> 1, k 3, pad 1, no activation): a dot product per (row, h).  Thread (h, part) adds the channels
// part, part + 4, ... in ascending order into four interleaved accumulators; the four parts meet in LDS.  One block per
// row and 64 positions: the rows are short here (H = 10 .. 51 at 8192 samples) and most lanes idle, but laying the
// (row, h) pairs of all rows end to end, as the MFMA conv does, leaves 55 blocks for period 11 and measured slower
// (0.89 against 0.68 ms for the six launches at 16 x 8192).
// Stores in the reference's order: out[(row / p) * H * p + h * p + row % p].
__global__ void __launch_bounds__(256)
conv_post_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int C, int H,
                 int p, float* __restrict__ out) {
  __shared__ float part[4][64];
  const int row = blockIdx.y, hl = threadIdx.x & 63, pt = threadIdx.x >> 6;
  const int h = blockIdx.x * 64 + hl;
  const float* xr = x + (int64_t)row * C * H;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (h < H) {
    const bool lo = h - 1 >= 0, hi = h + 1 < H;
    int k = 0;
    for (int c = pt; c < C; c += 4, ++k) {
      const float* xc = xr + (int64_t)c * H + h;
      float a = acc[k & 3];
      if (lo) a = __builtin_fmaf(w[c * 3 + 0], xc[-1], a);
      a = __builtin_fmaf(w[c * 3 + 1], xc[0], a);
      if (hi) a = __builtin_fmaf(w[c * 3 + 2], xc[1], a);
      acc[k & 3] = a;
    }
  }
  part[pt][hl] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  if (pt == 0 && h < H) {
    const int b = row / p, wv = row - b * p;
    out[((int64_t)b * H + h) * p + wv] = ((part[0][hl] + part[1][hl]) + (part[2][hl] + part[3][hl])) + bias[0];
  }
}

// ---------------------------------------------------------------------------------------------
// DiscriminatorS's grouped convs (k 41, stride 4, pad 20, four input channels per group) and its ungrouped k 15 first
// layer (one input channel): a direct VALU kernel.  A block owns one (row, group, 64 output positions): the group's
// weights and the input window sit in LDS; thread (h, cs) computes the group's output channels cs, cs + 4, ...  One
// accumulator per input channel, taps in ascending order, then (a0 + a1) + (a2 + a3); + bias, leaky-relu.
// Rows >= split read x2 (the generated half of the first layer's input).
constexpr int kGMaxK = 41, kGMaxCi = 4, kGMaxCo = 16, kGT = 64, kGMaxWin = (kGT - 1) * 4 + kGMaxK;

__global__ void __launch_bounds__(256)
grouped_conv1d_kernel(const float* __restrict__ x, const float* __restrict__ x2, int split, int Cin, int Tin,
                      const float* __restrict__ w, const float* __restrict__ bias, int Cout, int groups, int K,
                      int stride, int pad, int Tout, float* __restrict__ out) {
  __shared__ float xs[kGMaxCi][kGMaxWin];
  __shared__ float ws[kGMaxCo * kGMaxCi * kGMaxK];
  const int row = blockIdx.z, g = blockIdx.y, t0 = blockIdx.x * kGT;
  const int ci_n = Cin / groups, co_n = Cout / groups;
  const int win = (kGT - 1) * stride + K;
  const float* xr = (row < split ? x + (int64_t)row * Cin * Tin : x2 + (int64_t)(row - split) * Cin * Tin) +
                    (int64_t)g * ci_n * Tin;
  for (int i = threadIdx.x; i < ci_n * win; i += 256) {
    const int ci = i / win, o = i - ci * win;
    const int t = t0 * stride - pad + o;
    xs[ci][o] = (t >= 0 && t < Tin) ? xr[(int64_t)ci * Tin + t] : 0.f;
  }
  const float* wg = w + (int64_t)g * co_n * ci_n * K;
  for (int i = threadIdx.x; i < co_n * ci_n * K; i += 256) ws[i] = wg[i];
  __syncthreads();
  const int hl = threadIdx.x & 63, cs = threadIdx.x >> 6;
  const int t = t0 + hl;
  if (t >= Tout) return;
  for (int col = cs; col < co_n; col += 4) {
    float a[kGMaxCi] = {0.f, 0.f, 0.f, 0.f};
    for (int ci = 0; ci < ci_n; ++ci) {
      const float* wr = ws + (col * ci_n + ci) * K;
      const float* xw = xs[ci] + hl * stride;
      float s = 0.f;
      for (int tap = 0; tap < K; ++tap) s = __builtin_fmaf(wr[tap], xw[tap], s);
      a[ci] = s;
    }
    const int co = g * co_n + col;
    out[((int64_t)row * Cout + co) * Tout + t] = lrelu(((a[0] + a[1]) + (a[2] + a[3])) + bias[co]);
  }
}

// ---------------------------------------------------------------------------------------------
// Reductions.  An item is one (real, generated) tensor pair whose utterance b owns the contiguous N floats at
// a + b * a_bs / g + b * g_bs.  kind 0 (feature_loss): sum |a - g|.  kind 1 (discriminator_loss): sum (1 - a)^2 and
// sum g^2.  kind 2 (generator_loss): sum (1 - a)^2 (g unused).  sums: [2][n][B] float64.
constexpr int kMaxItems = 40;  // per rows launch: 40 items are 1.6 KB of kernel arguments
constexpr int kMaxLossItems = WETTS_DISC_LOSSES_MAX_ITEMS;
struct LossItems {
  const float* a[kMaxItems];
  const float* g[kMaxItems];
  int64_t a_bs[kMaxItems], g_bs[kMaxItems], N[kMaxItems];
};
struct LossCounts {  // what the totals launch reads
  int64_t N[kMaxLossItems];
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double block_sum_d(double v, double* part) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (part[0] + part[1]) + (part[2] + part[3]);
  __syncthreads();
  return r;
}

// `it` holds the items i0 .. i0 + gridDim.y - 1 of the n (a group of a long list: an item's sums do not depend on it)
__global__ void __launch_bounds__(256)
disc_rows_kernel(LossItems it, int kind, int i0, int n, int B, double* __restrict__ sums) {
  __shared__ double part[4];
  const int b = blockIdx.x, il = blockIdx.y, i = i0 + il;
  const int64_t N = it.N[il];
  const float* pa = it.a[il] + (int64_t)b * it.a_bs[il];
  const float* pg = kind == 2 ? nullptr : it.g[il] + (int64_t)b * it.g_bs[il];
  double s0[4] = {0., 0., 0., 0.}, s1[4] = {0., 0., 0., 0.};
  int k = 0;
  for (int64_t e = threadIdx.x; e < N; e += 256, ++k) {
    const float av = pa[e];
    if (kind == 0) {
      s0[k & 3] += fabsf(av - pg[e]);
    } else {
      const float d = 1.f - av;
      s0[k & 3] += d * d;
      if (kind == 1) {
        const float gv = pg[e];
        s1[k & 3] += gv * gv;
      }
    }
  }
  const double r0 = block_sum_d((s0[0] + s0[1]) + (s0[2] + s0[3]), part);
  const double r1 = block_sum_d((s1[0] + s1[1]) + (s1[2] + s1[3]), part);
  if (threadIdx.x == 0) {
    sums[(int64_t)i * B + b] = r0;
    sums[((int64_t)n + i) * B + b] = r1;
  }
}

// item_a[i] = (sum_b sums[0][i][b]) / (B * N_i) (and item_g from sums[1], kind 1), total = scale * sum_i (item_a + item_g),
// per_utt[b] = scale * sum_i (sums[0][i][b] + sums[1][i][b]) / N_i.  One wave.
__global__ void __launch_bounds__(64)
disc_totals_kernel(LossCounts it, int kind, int n, int B, float scale, const double* __restrict__ sums,
                   float* __restrict__ item_a, float* __restrict__ item_g, float* __restrict__ per_utt,
                   float* __restrict__ total) {
  double tot = 0.;
  for (int i = 0; i < n; ++i) {
    double a = 0., g = 0.;
    for (int b = threadIdx.x; b < B; b += 64) {
      a += sums[(int64_t)i * B + b];
      g += sums[((int64_t)n + i) * B + b];
    }
    const double den = (double)B * (double)it.N[i];
    a = wave_sum_d(a) / den;
    g = wave_sum_d(g) / den;
    if (threadIdx.x == 0) {
      item_a[i] = (float)a;
      if (kind == 1) item_g[i] = (float)g;
    }
    tot += kind == 1 ? a + g : a;
  }
  if (threadIdx.x == 0) total[0] = (float)(tot * (double)scale);
  for (int b = threadIdx.x; b < B; b += 64) {
    double s = 0.;
    for (int i = 0; i < n; ++i) {
      const double Nf = (double)it.N[i];
      const double a = sums[(int64_t)i * B + b] / Nf;
      s += kind == 1 ? a + sums[((int64_t)n + i) * B + b] / Nf : a;
    }
    per_utt[b] = (float)(s * (double)scale);
  }
}

// ---------------------------------------------------------------------------------------------
// host side: the fixed architecture, its blob and the launchers
struct DiscTensor {
  std::string name;
  int64_t offset, numel, shape[4];
};

struct DiscLayout {
  std::vector<DiscTensor> tensors;
  DiscLayer layers[kNumDisc][7];
  int64_t total = 0;
};

static int n_layers(int d) { return d == 0 ? 7 : 6; }

static const DiscLayout& disc_layout() {
  static const DiscLayout L = [] {
    DiscLayout l;
    // {Cout, Cin, K, stride, pad, groups}
    const int s_spec[7][6] = {{16, 1, 15, 1, 7, 1},       {64, 16, 41, 4, 20, 4},     {256, 64, 41, 4, 20, 16},
                              {1024, 256, 41, 4, 20, 64}, {1024, 1024, 41, 4, 20, 256}, {1024, 1024, 5, 1, 2, 1},
                              {1, 1024, 3, 1, 1, 1}};
    const int p_spec[6][6] = {{32, 1, 5, 3, 2, 1},     {128, 32, 5, 3, 2, 1},   {512, 128, 5, 3, 2, 1},
                              {1024, 512, 5, 3, 2, 1}, {1024, 1024, 5, 1, 2, 1}, {1, 1024, 3, 1, 1, 1}};
    auto add = [&](const std::string& name, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
      DiscTensor t;
      t.name = name;
      t.offset = l.total;
      t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = s3;
      t.numel = s0 * (s1 > 0 ? s1 : 1) * (s2 > 0 ? s2 : 1) * (s3 > 0 ? s3 : 1);
      l.total = align_up(l.total + t.numel, 64);
      l.tensors.push_back(t);
      return t.offset;
    };
    for (int d = 0; d < kNumDisc; ++d)
      for (int m = 0; m < n_layers(d); ++m) {
        const int* sp = d == 0 ? s_spec[m] : p_spec[m];
        DiscLayer& y = l.layers[d][m];
        y.Cout = sp[0]; y.Cin = sp[1]; y.K = sp[2]; y.stride = sp[3]; y.pad = sp[4]; y.groups = sp[5];
        const bool post = m == n_layers(d) - 1;
        const std::string base = "discriminators." + std::to_string(d) +
                                 (post ? std::string(".conv_post") : ".convs." + std::to_string(m));
        y.w_off = add(base + ".weight", y.Cout, y.Cin / y.groups, y.K, d == 0 ? 0 : 1);
        y.b_off = add(base + ".bias", y.Cout, 0, 0, 0);
      }
    return l;
  }();
  return L;
}

}  // namespace wetts

struct wetts_disc {
  float* blob = nullptr;
};

namespace wetts {

static int out_len(const DiscLayer& y, int Tin) { return (Tin + 2 * y.pad - y.K) / y.stride + 1; }

// The launchers take the layer and the blob its offsets index, so that every handle that owns period stacks runs them.
static int32_t launch_fold_conv0(const DiscLayer& l, const float* blob, int p, const float* y, const float* y_hat, int split,
                                 int B2, int T, float* out, hipStream_t s) {
  const int H0 = cdiv(T, p), H1 = out_len(l, H0);
  WETTS_REQUIRE(H0 * p - T < T, "disc: T=%d is too short for the reflect pad of period %d", T, p);
  WETTS_REQUIRE((int64_t)B2 * p <= 65535, "disc: 2B * p = %lld rows exceed one launch", (long long)B2 * p);
  hipLaunchKernelGGL(period_fold_conv0_kernel, dim3((unsigned)cdiv(H1, 64), (unsigned)(B2 * p)), dim3(64), 0, s, y, y_hat,
                     split, T, p, H0, H1, blob + l.w_off, blob + l.b_off, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t launch_strided(const DiscLayer& l, const float* blob, const float* x, int64_t rows, int Hin, float* out,
                              hipStream_t s) {
  WETTS_REQUIRE(l.K == 5 && l.groups == 1 && l.Cin % kDCK == 0 && l.Cout % kDM == 0,
                "disc: a %d -> %d conv of %d taps is not an MFMA conv", l.Cin, l.Cout, l.K);
  const int Hout = out_len(l, Hin);
  const int64_t ncols = rows * Hout;
  WETTS_REQUIRE(Hin >= 1 && ncols >= 1 && (ncols + kDN - 1) / kDN <= 0x7fffffff, "disc: bad strided conv extent");
  const dim3 grid((unsigned)((ncols + kDN - 1) / kDN), (unsigned)(l.Cout / kDM));
  const float* w = blob + l.w_off;
  const float* b = blob + l.b_off;
  if (l.stride == 3)
    hipLaunchKernelGGL(strided_conv_mfma_kernel<3>, grid, dim3(256), 0, s, x, w, b, out, ncols, l.Cin, l.Cout, Hin, Hout);
  else
    hipLaunchKernelGGL(strided_conv_mfma_kernel<1>, grid, dim3(256), 0, s, x, w, b, out, ncols, l.Cin, l.Cout, Hin, Hout);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t launch_post(const DiscLayer& l, const float* blob, int p, const float* x, int B2, int H, float* out,
                           hipStream_t s) {
  WETTS_REQUIRE(H >= 1 && B2 >= 1 && (int64_t)B2 * p <= 65535, "disc: bad conv_post extent");
  hipLaunchKernelGGL(conv_post_kernel, dim3((unsigned)cdiv(H, 64), (unsigned)(B2 * p)), dim3(256), 0, s, x,
                     blob + l.w_off, blob + l.b_off, l.Cin, H, p, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t launch_grouped(const wetts_disc* h, int m, const float* x, const float* x2, int split, int rows, int Tin,
                              float* out, hipStream_t s) {
  WETTS_REQUIRE(m >= 0 && m <= 4, "disc: layer %d of DiscriminatorS is not a grouped conv", m);
  const DiscLayer& l = disc_layout().layers[0][m];
  const int Tout = out_len(l, Tin);
  WETTS_REQUIRE(Tin >= 1 && Tout >= 1 && rows >= 1 && rows <= 65535, "disc: bad grouped conv extent");
  static_assert(kGMaxCo * kGMaxCi * kGMaxK * 4 + kGMaxCi * kGMaxWin * 4 <= 64 * 1024, "grouped conv LDS");
  hipLaunchKernelGGL(grouped_conv1d_kernel, dim3((unsigned)cdiv(Tout, kGT), (unsigned)l.groups, (unsigned)rows), dim3(256),
                     0, s, x, x2, split, l.Cin, Tin, (const float*)(h->blob + l.w_off), (const float*)(h->blob + l.b_off),
                     l.Cout, l.groups, l.K, l.stride, l.pad, Tout, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// [rows, C, H, p] of fmap i (0..36) for 2B utterances of T samples
static void fmap_shape(int B2, int T, int index, int64_t shape[4]) {
  int d = 0, m = index;
  if (index >= 7) {
    d = 1 + (index - 7) / 6;
    m = (index - 7) % 6;
  }
  const int p = d == 0 ? 1 : kDiscPeriods[d - 1];
  int H = d == 0 ? T : cdiv(T, p);
  for (int i = 0; i <= m; ++i) H = out_len(disc_layout().layers[d][i], H);
  shape[0] = (int64_t)B2 * p;
  shape[1] = disc_layout().layers[d][m].Cout;
  shape[2] = H;
  shape[3] = p;
}

void disc_period_layer(int m, DiscLayer* l) {
  *l = disc_layout().layers[1][m];
  l->w_off = l->b_off = 0;
}

void disc_period_fmap_shape(const DiscLayer* layers, int p, int B2, int T, int m, int64_t shape[4]) {
  int H = cdiv(T, p);
  for (int i = 0; i <= m; ++i) H = out_len(layers[i], H);
  shape[0] = (int64_t)B2 * p;
  shape[1] = layers[m].Cout;
  shape[2] = H;
  shape[3] = p;
}

int32_t disc_period_stack(const DiscLayer* layers, const float* blob, int p, const float* y, const float* y_hat, int split,
                          int B2, int T, float* const* f, hipStream_t s) {
  int64_t shp[4];
  WETTS_TRY(launch_fold_conv0(layers[0], blob, p, y, y_hat, split, B2, T, f[0], s));
  for (int m = 1; m < 5; ++m) {
    disc_period_fmap_shape(layers, p, B2, T, m - 1, shp);
    WETTS_TRY(launch_strided(layers[m], blob, f[m - 1], (int64_t)B2 * p, (int)shp[2], f[m], s));
  }
  disc_period_fmap_shape(layers, p, B2, T, 4, shp);
  return launch_post(layers[5], blob, p, f[4], B2, (int)shp[2], f[5], s);
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_disc_blob_num_tensors(void) { return (int32_t)disc_layout().tensors.size(); }

int32_t wetts_disc_blob_tensor_info(int32_t index, char* name_buf, size_t name_buf_len, int64_t* offset, int64_t* numel,
                                    int64_t shape[4]) {
  const DiscLayout& L = disc_layout();
  WETTS_REQUIRE(index >= 0 && index < (int32_t)L.tensors.size(), "tensor index %d out of range", index);
  const DiscTensor& t = L.tensors[index];
  WETTS_REQUIRE(name_buf && name_buf_len > t.name.size(), "name buffer too small");
  strcpy(name_buf, t.name.c_str());
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  return WETTS_OK;
}

int64_t wetts_disc_blob_numel(void) { return disc_layout().total; }

int32_t wetts_disc_create(const float* blob_dev, int64_t blob_numel, void* stream, wetts_disc_t** out) {
  WETTS_REQUIRE(out != nullptr && blob_dev != nullptr, "null argument");
  WETTS_REQUIRE(blob_numel == disc_layout().total, "blob has %lld floats, the discriminator layout needs %lld",
                (long long)blob_numel, (long long)disc_layout().total);
  wetts_disc* h = new wetts_disc();
  hipError_t e = hipMalloc((void**)&h->blob, (size_t)blob_numel * sizeof(float));
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->blob, blob_dev, (size_t)blob_numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    set_error("wetts_disc_create: %s", hipGetErrorString(e));
    if (h->blob) (void)hipFree(h->blob);
    delete h;
    return WETTS_E_HIP;
  }
  *out = h;
  return WETTS_OK;
}

void wetts_disc_destroy(wetts_disc_t* h) {
  if (!h) return;
  if (h->blob) (void)hipFree(h->blob);
  delete h;
}

int32_t wetts_disc_fmap_shape(int32_t B, int32_t T, int32_t index, int64_t shape[4]) {
  WETTS_REQUIRE(shape && B >= 1 && T >= 1 && index >= 0 && index < kNumFmaps, "disc_fmap_shape: bad argument");
  fmap_shape(2 * B, T, index, shape);
  return WETTS_OK;
}

int32_t wetts_disc_fold_conv0(const wetts_disc_t* h, int32_t d, const float* y, int32_t rows, int32_t T, float* out,
                              void* stream) {
  WETTS_REQUIRE(h && y && out && d >= 1 && d < kNumDisc && rows >= 1 && T >= 1, "disc_fold_conv0: bad argument");
  return launch_fold_conv0(disc_layout().layers[d][0], h->blob, kDiscPeriods[d - 1], y, y, rows, rows, T, out,
                           (hipStream_t)stream);
}

int32_t wetts_disc_strided_conv(const wetts_disc_t* h, int32_t d, int32_t layer, const float* x, int64_t rows,
                                int32_t Hin, float* out, void* stream) {
  WETTS_REQUIRE(h && x && out && d >= 0 && d < kNumDisc && layer >= 1 && layer < n_layers(d) - 1,
                "disc_strided_conv: bad argument");
  return launch_strided(disc_layout().layers[d][layer], h->blob, x, rows, Hin, out, (hipStream_t)stream);
}

int32_t wetts_disc_conv_post(const wetts_disc_t* h, int32_t d, const float* x, int32_t rows, int32_t H, float* out,
                             void* stream) {
  WETTS_REQUIRE(h && x && out && d >= 0 && d < kNumDisc && rows >= 1, "disc_conv_post: bad argument");
  return launch_post(disc_layout().layers[d][n_layers(d) - 1], h->blob, d == 0 ? 1 : kDiscPeriods[d - 1], x, rows, H, out,
                     (hipStream_t)stream);
}

int32_t wetts_disc_grouped_conv(const wetts_disc_t* h, int32_t layer, const float* x, int32_t rows, int32_t Tin,
                                float* out, void* stream) {
  WETTS_REQUIRE(h && x && out, "null argument");
  return launch_grouped(h, layer, x, x, rows, rows, Tin, out, (hipStream_t)stream);
}

int32_t wetts_disc_forward(const wetts_disc_t* h, const float* y, const float* y_hat, int32_t B, int32_t T,
                           float* const* fmaps_host, void* stream) {
  WETTS_REQUIRE(h && y && y_hat && fmaps_host, "null argument");
  WETTS_REQUIRE(B >= 1 && B <= 2048 && T >= 6, "disc_forward: B=%d outside [1, 2048] or T=%d < 6", B, T);
  for (int i = 0; i < kNumFmaps; ++i) WETTS_REQUIRE(fmaps_host[i] != nullptr, "disc_forward: fmap %d is null", i);
  hipStream_t s = (hipStream_t)stream;
  const int B2 = 2 * B;
  // DiscriminatorS
  int Tin = T;
  for (int m = 0; m < 5; ++m) {
    WETTS_TRY(launch_grouped(h, m, m == 0 ? y : fmaps_host[m - 1], m == 0 ? y_hat : fmaps_host[m - 1], m == 0 ? B : B2,
                             B2, Tin, fmaps_host[m], s));
    Tin = out_len(disc_layout().layers[0][m], Tin);
  }
  WETTS_TRY(launch_strided(disc_layout().layers[0][5], h->blob, fmaps_host[4], B2, Tin, fmaps_host[5], s));
  WETTS_TRY(launch_post(disc_layout().layers[0][6], h->blob, 1, fmaps_host[5], B2, Tin, fmaps_host[6], s));
  // DiscriminatorP x 5
  for (int d = 1; d < kNumDisc; ++d)
    WETTS_TRY(disc_period_stack(disc_layout().layers[d], h->blob, kDiscPeriods[d - 1], y, y_hat, B, B2, T,
                                fmaps_host + 7 + 6 * (d - 1), s));
  return WETTS_OK;
}

int32_t wetts_disc_losses(int32_t kind, int32_t n, const float* const* a_host, const float* const* g_host,
                          const int64_t* a_bs_host, const int64_t* g_bs_host, const int64_t* N_host, int32_t B, float scale,
                          double* sums, float* item_a, float* item_g, float* per_utt, float* total, void* stream) {
  WETTS_REQUIRE(kind >= 0 && kind <= 2 && n >= 1 && n <= kMaxLossItems && B >= 1 && B <= 65535,
                "disc_losses: kind=%d n=%d B=%d out of range", kind, n, B);
  WETTS_REQUIRE(a_host && a_bs_host && N_host && sums && item_a && per_utt && total, "null argument");
  WETTS_REQUIRE(kind == 2 || (g_host && g_bs_host), "disc_losses: the generated tensors are missing");
  WETTS_REQUIRE(kind != 1 || item_g, "disc_losses: item_g is null");
  LossCounts cnt;
  memset(&cnt, 0, sizeof(cnt));
  for (int i = 0; i < n; ++i) {
    WETTS_REQUIRE(a_host[i] && N_host[i] >= 1 && (kind == 2 || g_host[i]), "disc_losses: item %d is empty", i);
    cnt.N[i] = N_host[i];
  }
  hipStream_t s = (hipStream_t)stream;
  for (int i0 = 0; i0 < n; i0 += kMaxItems) {
    const int m = n - i0 < kMaxItems ? n - i0 : kMaxItems;
    LossItems it;
    memset(&it, 0, sizeof(it));
    for (int i = 0; i < m; ++i) {
      it.a[i] = a_host[i0 + i];
      it.a_bs[i] = a_bs_host[i0 + i];
      it.N[i] = N_host[i0 + i];
      if (kind != 2) {
        it.g[i] = g_host[i0 + i];
        it.g_bs[i] = g_bs_host[i0 + i];
      }
    }
    hipLaunchKernelGGL(disc_rows_kernel, dim3((unsigned)B, (unsigned)m), dim3(256), 0, s, it, kind, i0, n, B, sums);
    WETTS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(disc_totals_kernel, dim3(1), dim3(64), 0, s, cnt, kind, n, B, scale, (const double*)sums, item_a, item_g,
                     per_utt, total);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // extern "C"
