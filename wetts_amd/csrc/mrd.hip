// MultiPeriodMultiResolutionDiscriminator (discriminators.py:127-225,256-283) without gradients: three DiscriminatorR
// stacks (window 2048 / 1024 / 512, hop = window / 4, no embedding) and the five DiscriminatorP stacks, which run through
// the launchers of discriminator.hip.  All f32, wave64, on the caller's stream; y and y_hat are one batch of 2B.
//
// One DiscriminatorR is: mrd_normalize_kernel (DC removal and peak normalisation per utterance), stft_cplx_kernel
// (stft.hip: re / im planes [rows][2][bins][frames], frames fastest), five launches of mrd_band_conv_mfma_kernel (one per
// layer, all five bands in one grid) and mrd_conv_post_kernel.  Layer 0's outputs and the spectrogram live in the
// caller's workspace; layers 1..4 and conv_post write the caller's feature maps in the reference's own shapes,
// [rows][32][frames][F'] and [rows][1][frames][sum F'].
//
// mrd_band_conv_mfma_kernel<KF, SF, CK>: Conv2d over (time, frequency), kernel (3, KF), stride (1, SF), zero pad
// (1, KF / 2) at the band's own edges, + bias + leaky-relu, as an f32 implicit GEMM on v_mfma_f32_32x32x2_f32:
//   D[32 x ncols] = W[32 x (Cin * 3 * KF)] * Bm,   Bm[(ci, dt, df)][(row, t, f)] = x[row][ci][t + dt - 1][f * SF + df - KF / 2]
// The columns are the (row, t, f) outputs of a band laid end to end across frames and utterances, so the narrow deep maps
// (17 x 13 at the training shape) still fill a tile.  A block of four waves owns 128 columns (a wave: one 32 x 32 tile)
// and walks Cin in chunks of CK channels = CK * 3 * KF k values.  Staging: thread (column, half of the chunk's channels)
// resolves the padding at its own t against `frames` and its own f against the band's Fin and writes its taps to
// Bs[k][column]; the MFMA's B reads are then unit-stride over the columns whatever SF is (32 lanes of a half-wave on 32
// banks; the two halves never conflict on ds_read_b32).  The weights are packed at create into A-fragment order
// ([k-step][64 lanes], 256 B per step: lane l holds W[l & 31][2 s + (l >> 5)]), one coalesced load per step that every
// block shares in L2; a chunk's steps pass through LDS with the B values so the MFMA loop waits on LDS alone.  The next
// chunk is fetched into registers before the current chunk's MFMAs.  The K sum is blocked by chunk: a chunk's products
// meet in an accumulator of their own, which then joins the running sum (16 + 27 roundings on the 864-term chain).
// Budget: KF = 9: CK = 2, 27 k-steps, Bs 27 KB + As 6.75 KB = 33.75 KB; KF = 3: CK = 8, 36 k-steps, 36 KB + 9 KB = 45 KB.
// Designed for TWO waves per SIMD (two blocks per CU): at most 256 registers a wave and 80 KB of LDS a block; the LDS
// leaves room for more where the registers allow it.
//
// Every output element's arithmetic is a function of its own utterance, position and the channel / tap order alone, so a
// row alone and the same row inside a batch give the same bits.  Reduction order of the normalisation: DESIGN.md §8.
#include "kernels.h"

#include <vector>

namespace wetts {

typedef float f32x16m __attribute__((ext_vector_type(16)));

constexpr float kMrdSlope = 0.1f;
constexpr int kMrdRes = 3, kMrdBands = 5, kMrdLayers = 5, kMrdC = 32;
constexpr int kMrdWindows[kMrdRes] = {2048, 1024, 512};
constexpr int kMrdMapsPerRes = kMrdBands * 4 + 1;  // layers 1..4 of each band, conv_post
constexpr int kMrdNumFmaps = kMrdRes * kMrdMapsPerRes + 5 * 6;
static_assert(kMrdNumFmaps == WETTS_MRD_NUM_FMAPS, "fmap count");

__device__ __forceinline__ float mrd_lrelu(float v) { return v >= 0.f ? v : kMrdSlope * v; }

// ---------------------------------------------------------------------------------------------
// x - mean, then (0.8 * x) / (max |x| + 1e-9), per utterance (discriminators.py:190-193).  One block per utterance.  The
// mean: thread i adds the elements i, i + 256, ... in ascending order into four interleaved float64 accumulators,
// (a0 + a1) + (a2 + a3), the butterfly over the lanes, (w0 + w1) + (w2 + w3) over the waves; divided in float64 and
// rounded once.  The maximum is exact in any order.  No atomics.
__global__ void __launch_bounds__(256)
mrd_normalize_kernel(const float* __restrict__ y, const float* __restrict__ y_hat, int split, int T,
                     float* __restrict__ out) {
  __shared__ double part[4];
  __shared__ float mpart[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* src = b < split ? y + (int64_t)b * T : y_hat + (int64_t)(b - split) * T;
  double s[4] = {0., 0., 0., 0.};
  int k = 0;
  for (int e = tid; e < T; e += 256, ++k) s[k & 3] += (double)src[e];
  double v = (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  const float mean = (float)(((part[0] + part[1]) + (part[2] + part[3])) / (double)T);
  float m = 0.f;
  for (int e = tid; e < T; e += 256) m = fmaxf(m, fabsf(src[e] - mean));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((tid & 63) == 0) mpart[tid >> 6] = m;
  __syncthreads();
  const float den = fmaxf(fmaxf(mpart[0], mpart[1]), fmaxf(mpart[2], mpart[3])) + 1e-9f;
  float* o = out + (int64_t)b * T;
  for (int e = tid; e < T; e += 256) o[e] = (0.8f * (src[e] - mean)) / den;
}

// ---------------------------------------------------------------------------------------------
// natural [32][K] weight -> A-fragment order [K / 2][64]
__global__ void mrd_pack_kernel(const float* __restrict__ w, int K, float* __restrict__ wpk) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (K / 2) * 64) return;
  const int lane = idx & 63, s = idx >> 6;
  wpk[idx] = w[(int64_t)(lane & 31) * K + 2 * s + (lane >> 5)];
}

// ---------------------------------------------------------------------------------------------
struct MrdBand {
  const float* x;    // band input: element (row, ci, t, f) at x[row * x_rs + ci * x_cs + t * x_ts + f * x_fs]
  float* out;        // [rows][32][frames][Fout]
  const float* wpk;  // [K / 2][64]
  const float* bias;
  int64_t x_rs, x_cs, ncols;  // ncols = rows * frames * Fout
  int x_ts, x_fs, Fin, Fout;
};
struct MrdBandTable {
  MrdBand b[kMrdBands];
};

constexpr int kMrdN = 128;  // columns per block

template <int KF, int SF, int CK>
__global__ void __launch_bounds__(256)
mrd_band_conv_mfma_kernel(MrdBandTable tb, int Cin, int frames) {
  constexpr int TAPS = 3 * KF, KC = CK * TAPS, STEPS = KC / 2, PF = KF / 2;
  constexpr int CPT = CK / 2, NA = (STEPS * 64 + 255) / 256;
  static_assert(KC % 2 == 0 && CK % 2 == 0, "chunk geometry");
  __shared__ float As[STEPS * 64];
  __shared__ float Bs[KC][kMrdN];
  const MrdBand& g = tb.b[blockIdx.y];
  const int64_t n0 = (int64_t)blockIdx.x * kMrdN;
  if (n0 >= g.ncols) return;  // the grid is sized for the widest band (uniform over the block)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Fout = g.Fout, Fin = g.Fin;
  const int64_t per = (int64_t)frames * Fout;

  // B staging: this thread's column, channels part * CPT + jj of the chunk, all taps
  const int scol = tid & (kMrdN - 1), part = tid >> 7;
  const int64_t sj = n0 + scol;
  const bool s_ok = sj < g.ncols;
  const int64_t srow = s_ok ? sj / per : 0;
  const int srem = s_ok ? (int)(sj - srow * per) : 0;
  const int st = srem / Fout, sf = srem - st * Fout;
  const int tb0 = st - 1, fb0 = sf * SF - PF;
  unsigned tmask = 0, fmask = 0;
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) tmask |= (unsigned)(s_ok && tb0 + dt >= 0 && tb0 + dt < frames) << dt;
#pragma unroll
  for (int df = 0; df < KF; ++df) fmask |= (unsigned)(fb0 + df >= 0 && fb0 + df < Fin) << df;
  const int64_t xoff = srow * g.x_rs + (int64_t)tb0 * g.x_ts + (int64_t)fb0 * g.x_fs;
  const float* __restrict__ xg = g.x;
  const float* __restrict__ wg = g.wpk;
  const int x_ts = g.x_ts, x_fs = g.x_fs;
  const int64_t x_cs = g.x_cs;

  float ar[NA];
  float br[CPT * TAPS];
  auto fetch = [&](int c0) {
    const float* wc = wg + (int64_t)(c0 / CK) * (STEPS * 64);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int idx = tid + 256 * j;
      ar[j] = idx < STEPS * 64 ? wc[idx] : 0.f;
    }
#pragma unroll
    for (int jj = 0; jj < CPT; ++jj) {
      const int64_t xc = xoff + (int64_t)(c0 + part * CPT + jj) * x_cs;
#pragma unroll
      for (int dt = 0; dt < 3; ++dt)
#pragma unroll
        for (int df = 0; df < KF; ++df) {
          const bool ok = ((tmask >> dt) & 1u) && ((fmask >> df) & 1u);
          br[jj * TAPS + dt * KF + df] = ok ? xg[xc + (int64_t)dt * x_ts + (int64_t)df * x_fs] : 0.f;
        }
    }
  };

  f32x16m zero;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero[r] = 0.f;
  f32x16m acc = zero;
  const int half = lane >> 5, bcol = wave * 32 + (lane & 31);

  fetch(0);
  for (int c0 = 0; c0 < Cin; c0 += CK) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int idx = tid + 256 * j;
      if (idx < STEPS * 64) As[idx] = ar[j];
    }
#pragma unroll
    for (int jj = 0; jj < CPT; ++jj)
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) Bs[(part * CPT + jj) * TAPS + tap][scol] = br[jj * TAPS + tap];
    __syncthreads();
    if (c0 + CK < Cin) fetch(c0 + CK);
    // blocked summation: the chunk's KC products meet in an accumulator of their own, which then joins the running sum
    f32x16m cv = zero;
#pragma unroll 9
    for (int s = 0; s < STEPS; ++s)
      cv = __builtin_amdgcn_mfma_f32_32x32x2f32(As[s * 64 + lane], Bs[2 * s + half][bcol], cv, 0, 0, 0);
    acc += cv;
    __syncthreads();
  }

  // lane holds channels 8 g + 4 (lane >> 5) + {0..3} of column lane & 31 (the 32x32 MFMA output layout)
  const int64_t j = n0 + bcol;
  if (j >= g.ncols) return;
  const int64_t row = j / per;
  const int rem = (int)(j - row * per);  // t * Fout + f
  float* ob = g.out + row * kMrdC * per + rem;
  const float* __restrict__ bias = g.bias;
#pragma unroll
  for (int gq = 0; gq < 4; ++gq)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = 8 * gq + 4 * half + i;
      ob[(int64_t)co * per] = mrd_lrelu(acc[4 * gq + i] + bias[co]);
    }
}

// ---------------------------------------------------------------------------------------------
// conv_post (32 -> 1, kernel (3, 3), pad (1, 1), no activation) over the five layer-4 band maps read in place: column c of
// the concatenation is column c - start[b] of band b, so a neighbour across a band join comes from the neighbouring
// band's map and the zero pad applies at column 0, column S - 1 and the first and last frame only.  One thread per
// output: channels in ascending order into four interleaved accumulators (channel & 3), the nine taps of a channel in
// (dt, df) order, (a0 + a1) + (a2 + a3) + bias.
struct MrdPostTable {
  const float* x[kMrdBands];  // [rows][32][frames][F[b]]
  int F[kMrdBands], start[kMrdBands + 1];
};

__global__ void __launch_bounds__(256)
mrd_conv_post_kernel(MrdPostTable tb, const float* __restrict__ w, const float* __restrict__ bias, int frames,
                     float* __restrict__ out) {
  __shared__ float ws[kMrdC * 9];
  for (int i = threadIdx.x; i < kMrdC * 9; i += 256) ws[i] = w[i];
  __syncthreads();
  const int S = tb.start[kMrdBands];
  const int row = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= frames * S) return;
  const int t = e / S, c = e - t * S;
  // the three columns: band base pointer (channel 0, frame 0, this column) and the band's channel stride
  const float* cp[3];
  int64_t cs[3];
  int F3[3];
#pragma unroll
  for (int df = 0; df < 3; ++df) {
    const int cc = c + df - 1;
    cp[df] = nullptr;
    cs[df] = 0;
    F3[df] = 0;
    if (cc < 0 || cc >= S) continue;
    int b = 0;
#pragma unroll
    for (int q = 1; q < kMrdBands; ++q) b += cc >= tb.start[q];
    const int F = tb.F[b];
    F3[df] = F;
    cs[df] = (int64_t)frames * F;
    cp[df] = tb.x[b] + (int64_t)row * kMrdC * cs[df] + (cc - tb.start[b]);
  }
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ci = 0; ci < kMrdC; ++ci) {
    float s = a[ci & 3];
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
      const int tt = t + dt - 1;
      if (tt < 0 || tt >= frames) continue;
#pragma unroll
      for (int df = 0; df < 3; ++df)
        if (cp[df]) s = __builtin_fmaf(ws[ci * 9 + dt * 3 + df], cp[df][ci * cs[df] + (int64_t)tt * F3[df]], s);
    }
    a[ci & 3] = s;
  }
  out[((int64_t)row * frames + t) * S + c] = ((a[0] + a[1]) + (a[2] + a[3])) + bias[0];
}

// ---------------------------------------------------------------------------------------------
// host side: the fixed architecture, its blob and the launchers
struct MrdTensor {
  std::string name;
  int64_t offset, numel, shape[4];
};

struct MrdConv {
  int Cin, KF, SF;
  int64_t w_off, b_off;
};

struct MrdLayout {
  std::vector<MrdTensor> tensors;
  MrdConv band[kMrdRes][kMrdBands][kMrdLayers];
  int64_t post_w[kMrdRes], post_b[kMrdRes];
  DiscLayer period[5][6];
  int64_t total = 0;
};

static const MrdLayout& mrd_layout() {
  static const MrdLayout L = [] {
    MrdLayout l;
    auto add = [&](const std::string& name, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
      MrdTensor t;
      t.name = name;
      t.offset = l.total;
      t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = s3;
      t.numel = s0 * (s1 > 0 ? s1 : 1) * (s2 > 0 ? s2 : 1) * (s3 > 0 ? s3 : 1);
      l.total = align_up(l.total + t.numel, 64);
      l.tensors.push_back(t);
      return t.offset;
    };
    // {Cin, KF, SF} of a band's five convs (discriminators.py:159-176)
    const int spec[kMrdLayers][3] = {{2, 9, 1}, {32, 9, 2}, {32, 9, 2}, {32, 9, 2}, {32, 3, 1}};
    for (int r = 0; r < kMrdRes; ++r) {
      const std::string d = "discriminators." + std::to_string(r);
      for (int b = 0; b < kMrdBands; ++b)
        for (int m = 0; m < kMrdLayers; ++m) {
          MrdConv& c = l.band[r][b][m];
          c.Cin = spec[m][0]; c.KF = spec[m][1]; c.SF = spec[m][2];
          const std::string base = d + ".band_convs." + std::to_string(b) + "." + std::to_string(m);
          c.w_off = add(base + ".weight", kMrdC, c.Cin, 3, c.KF);
          c.b_off = add(base + ".bias", kMrdC, 0, 0, 0);
        }
      l.post_w[r] = add(d + ".conv_post.weight", 1, kMrdC, 3, 3);
      l.post_b[r] = add(d + ".conv_post.bias", 1, 0, 0, 0);
    }
    for (int p = 0; p < 5; ++p)
      for (int m = 0; m < 6; ++m) {
        DiscLayer& y = l.period[p][m];
        disc_period_layer(m, &y);
        const std::string base = "discriminators." + std::to_string(kMrdRes + p) +
                                 (m == 5 ? std::string(".conv_post") : ".convs." + std::to_string(m));
        y.w_off = add(base + ".weight", y.Cout, y.Cin, y.K, 1);
        y.b_off = add(base + ".bias", y.Cout, 0, 0, 0);
      }
    return l;
  }();
  return L;
}

// Band edges (discriminators.py:155-156): int(f * n_fft) with n_fft = window // 2 + 1, in the reference's own double
// arithmetic.
static void mrd_band_edges(int res, int lo[kMrdBands], int hi[kMrdBands]) {
  const double fr[kMrdBands][2] = {{0.0, 0.1}, {0.1, 0.25}, {0.25, 0.5}, {0.5, 0.75}, {0.75, 1.0}};
  const int nb = kMrdWindows[res] / 2 + 1;
  for (int b = 0; b < kMrdBands; ++b) {
    lo[b] = (int)(fr[b][0] * nb);
    hi[b] = (int)(fr[b][1] * nb);
  }
}

// width of band b after `layer` convs (0 = the input bins)
static int mrd_width(int res, int b, int layer) {
  int lo[kMrdBands], hi[kMrdBands];
  mrd_band_edges(res, lo, hi);
  int F = hi[b] - lo[b];
  const MrdLayout& L = mrd_layout();
  for (int m = 0; m < layer; ++m) {
    const MrdConv& c = L.band[res][b][m];
    F = (F + 2 * (c.KF / 2) - c.KF) / c.SF + 1;
  }
  return F;
}

}  // namespace wetts

struct wetts_mrd {
  float* blob = nullptr;
  float* basis[wetts::kMrdRes] = {nullptr, nullptr, nullptr};
  float* wpk = nullptr;  // the packed band-conv weights, one [K / 2][64] block per (res, band, layer)
  int64_t wpk_off[wetts::kMrdRes][wetts::kMrdBands][wetts::kMrdLayers];
};

namespace wetts {

static int32_t launch_normalize(const float* y, const float* y_hat, int split, int rows, int T, float* out, hipStream_t s) {
  WETTS_REQUIRE(rows >= 1 && T >= 1, "mrd_normalize: bad extent");
  hipLaunchKernelGGL(mrd_normalize_kernel, dim3((unsigned)rows), dim3(256), 0, s, y, y_hat, split, T, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// layer `m` of all five bands of resolution `res`: in[b] / out[b] are the bands' tensors.  Layer 0 reads the spectrogram
// planes [rows][2][nb][frames] (in[b] = the spectrogram's base for every band; the band's first bin is added here).
static int32_t launch_band_conv(const wetts_mrd* h, int res, int m, const float* const* in, int rows, int frames,
                                float* const* out, hipStream_t s) {
  const MrdLayout& L = mrd_layout();
  int lo[kMrdBands], hi[kMrdBands];
  mrd_band_edges(res, lo, hi);
  const int nb = kMrdWindows[res] / 2 + 1;
  MrdBandTable tb;
  int64_t maxcols = 0;
  for (int b = 0; b < kMrdBands; ++b) {
    const MrdConv& c = L.band[res][b][m];
    MrdBand& g = tb.b[b];
    g.Fin = mrd_width(res, b, m);
    g.Fout = mrd_width(res, b, m + 1);
    WETTS_REQUIRE(g.Fin >= 1 && g.Fout >= 1, "mrd: band %d of resolution %d is empty at layer %d", b, res, m);
    if (m == 0) {
      g.x = in[b] + (int64_t)lo[b] * frames;
      g.x_rs = (int64_t)2 * nb * frames;
      g.x_cs = (int64_t)nb * frames;
      g.x_ts = 1;
      g.x_fs = frames;
    } else {
      g.x = in[b];
      g.x_rs = (int64_t)c.Cin * frames * g.Fin;
      g.x_cs = (int64_t)frames * g.Fin;
      g.x_ts = g.Fin;
      g.x_fs = 1;
    }
    g.out = out[b];
    g.wpk = h->wpk + h->wpk_off[res][b][m];
    g.bias = h->blob + c.b_off;
    g.ncols = (int64_t)rows * frames * g.Fout;
    if (g.ncols > maxcols) maxcols = g.ncols;
  }
  const int64_t tiles = (maxcols + kMrdN - 1) / kMrdN;
  WETTS_REQUIRE(tiles >= 1 && tiles <= 0x7fffffff, "mrd: bad band conv extent");
  const dim3 grid((unsigned)tiles, kMrdBands);
  const MrdConv& c0 = L.band[res][0][m];
  if (m == 0)
    hipLaunchKernelGGL((mrd_band_conv_mfma_kernel<9, 1, 2>), grid, dim3(256), 0, s, tb, c0.Cin, frames);
  else if (m < 4)
    hipLaunchKernelGGL((mrd_band_conv_mfma_kernel<9, 2, 2>), grid, dim3(256), 0, s, tb, c0.Cin, frames);
  else
    hipLaunchKernelGGL((mrd_band_conv_mfma_kernel<3, 1, 8>), grid, dim3(256), 0, s, tb, c0.Cin, frames);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t launch_mrd_post(const wetts_mrd* h, int res, const float* const* in, int rows, int frames, float* out,
                               hipStream_t s) {
  const MrdLayout& L = mrd_layout();
  MrdPostTable tb;
  tb.start[0] = 0;
  for (int b = 0; b < kMrdBands; ++b) {
    tb.x[b] = in[b];
    tb.F[b] = mrd_width(res, b, kMrdLayers);
    tb.start[b + 1] = tb.start[b] + tb.F[b];
  }
  const int64_t n = (int64_t)frames * tb.start[kMrdBands];
  WETTS_REQUIRE(rows >= 1 && rows <= 65535 && n >= 1 && n < (1ll << 31), "mrd: bad conv_post extent");
  hipLaunchKernelGGL(mrd_conv_post_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)rows), dim3(256), 0, s, tb,
                     (const float*)(h->blob + L.post_w[res]), (const float*)(h->blob + L.post_b[res]), frames, out);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int mrd_frames(int res, int T) { return 1 + T / (kMrdWindows[res] / 4); }

static void mrd_fmap_shape(int B2, int T, int index, int64_t shape[4]) {
  if (index >= kMrdRes * kMrdMapsPerRes) {
    const int d = (index - kMrdRes * kMrdMapsPerRes) / 6, m = (index - kMrdRes * kMrdMapsPerRes) % 6;
    disc_period_fmap_shape(mrd_layout().period[d], kDiscPeriods[d], B2, T, m, shape);
    return;
  }
  const int res = index / kMrdMapsPerRes, k = index % kMrdMapsPerRes;
  shape[0] = B2;
  shape[2] = mrd_frames(res, T);
  if (k == kMrdMapsPerRes - 1) {
    shape[1] = 1;
    shape[3] = 0;
    for (int b = 0; b < kMrdBands; ++b) shape[3] += mrd_width(res, b, kMrdLayers);
  } else {
    shape[1] = kMrdC;
    shape[3] = mrd_width(res, k / 4, k % 4 + 2);
  }
}

// workspace: [normalised audio][spectrogram of one resolution][its layer-0 outputs], each part 256-byte aligned and sized
// for the largest resolution
static void mrd_ws_parts(int B2, int T, int64_t* norm, int64_t* spec, int64_t* l0) {
  *norm = align_up((int64_t)B2 * T, 64);
  *spec = *l0 = 0;
  for (int r = 0; r < kMrdRes; ++r) {
    const int64_t nb = kMrdWindows[r] / 2 + 1, fr = mrd_frames(r, T);
    const int64_t sp = align_up((int64_t)B2 * 2 * nb * fr, 64), l = align_up((int64_t)B2 * kMrdC * fr * nb, 64);
    if (sp > *spec) *spec = sp;
    if (l > *l0) *l0 = l;
  }
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_mrd_blob_num_tensors(void) { return (int32_t)mrd_layout().tensors.size(); }

int32_t wetts_mrd_blob_tensor_info(int32_t index, char* name_buf, size_t name_buf_len, int64_t* offset, int64_t* numel,
                                   int64_t shape[4]) {
  const MrdLayout& L = mrd_layout();
  WETTS_REQUIRE(index >= 0 && index < (int32_t)L.tensors.size(), "tensor index %d out of range", index);
  const MrdTensor& t = L.tensors[index];
  WETTS_REQUIRE(name_buf && name_buf_len > t.name.size(), "name buffer too small");
  strcpy(name_buf, t.name.c_str());
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  return WETTS_OK;
}

int64_t wetts_mrd_blob_numel(void) { return mrd_layout().total; }

void wetts_mrd_destroy(wetts_mrd_t* h) {
  if (!h) return;
  if (h->blob) (void)hipFree(h->blob);
  if (h->wpk) (void)hipFree(h->wpk);
  for (int r = 0; r < kMrdRes; ++r)
    if (h->basis[r]) (void)hipFree(h->basis[r]);
  delete h;
}

int32_t wetts_mrd_create(const float* blob_dev, int64_t blob_numel, void* stream, wetts_mrd_t** out) {
  const MrdLayout& L = mrd_layout();
  WETTS_REQUIRE(out != nullptr && blob_dev != nullptr, "null argument");
  WETTS_REQUIRE(blob_numel == L.total, "blob has %lld floats, the MPMRD layout needs %lld", (long long)blob_numel,
                (long long)L.total);
  hipStream_t s = (hipStream_t)stream;
  wetts_mrd* h = new wetts_mrd();
  int64_t wtotal = 0;
  for (int r = 0; r < kMrdRes; ++r)
    for (int b = 0; b < kMrdBands; ++b)
      for (int m = 0; m < kMrdLayers; ++m) {
        h->wpk_off[r][b][m] = wtotal;
        wtotal += (int64_t)kMrdC * L.band[r][b][m].Cin * 3 * L.band[r][b][m].KF;
      }
  hipError_t e = hipMalloc((void**)&h->blob, (size_t)blob_numel * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&h->wpk, (size_t)wtotal * sizeof(float));
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->blob, blob_dev, (size_t)blob_numel * sizeof(float), hipMemcpyDeviceToDevice, s);
  int32_t rc = WETTS_OK;
  for (int r = 0; r < kMrdRes && e == hipSuccess && rc == WETTS_OK; ++r) {
    const int64_t n = wetts_stft_basis_numel(kMrdWindows[r], kMrdWindows[r]);
    e = hipMalloc((void**)&h->basis[r], (size_t)n * sizeof(float));
    if (e == hipSuccess) rc = wetts_stft_basis(kMrdWindows[r], kMrdWindows[r], h->basis[r], n, stream);
  }
  if (e == hipSuccess && rc == WETTS_OK) {
    for (int r = 0; r < kMrdRes; ++r)
      for (int b = 0; b < kMrdBands; ++b)
        for (int m = 0; m < kMrdLayers; ++m) {
          const MrdConv& c = L.band[r][b][m];
          const int K = c.Cin * 3 * c.KF, n = (K / 2) * 64;
          hipLaunchKernelGGL(mrd_pack_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s,
                             (const float*)(h->blob + c.w_off), K, h->wpk + h->wpk_off[r][b][m]);
        }
    e = hipGetLastError();
  }
  if (e == hipSuccess && rc == WETTS_OK) e = hipStreamSynchronize(s);
  if (e != hipSuccess || rc != WETTS_OK) {
    if (e != hipSuccess) set_error("wetts_mrd_create: %s", hipGetErrorString(e));
    wetts_mrd_destroy(h);
    return e != hipSuccess ? WETTS_E_HIP : rc;
  }
  *out = h;
  return WETTS_OK;
}

int32_t wetts_mrd_fmap_shape(int32_t B, int32_t T, int32_t index, int64_t shape[4]) {
  WETTS_REQUIRE(shape && B >= 1 && T >= WETTS_MRD_MIN_SAMPLES && index >= 0 && index < kMrdNumFmaps,
                "mrd_fmap_shape: bad argument");
  mrd_fmap_shape(2 * B, T, index, shape);
  return WETTS_OK;
}

int32_t wetts_mrd_band_width(int32_t res, int32_t band, int32_t layer) {
  if (res < 0 || res >= kMrdRes || band < 0 || band >= kMrdBands || layer < 0 || layer > kMrdLayers) return -1;
  return mrd_width(res, band, layer);
}

int64_t wetts_mrd_workspace_bytes(int32_t B, int32_t T) {
  if (B < 1 || B > 2048 || T < WETTS_MRD_MIN_SAMPLES) return -1;
  int64_t norm, spec, l0;
  mrd_ws_parts(2 * B, T, &norm, &spec, &l0);
  return (norm + spec + l0) * (int64_t)sizeof(float);
}

int32_t wetts_mrd_normalize(const float* y, int32_t rows, int32_t T, float* out, void* stream) {
  WETTS_REQUIRE(y && out, "null argument");
  return launch_normalize(y, y, rows, rows, T, out, (hipStream_t)stream);
}

int32_t wetts_mrd_spectrogram(const wetts_mrd_t* h, int32_t res, const float* x, int32_t rows, int32_t T, float* spec,
                              void* stream) {
  WETTS_REQUIRE(h && x && spec && res >= 0 && res < kMrdRes && rows >= 1, "mrd_spectrogram: bad argument");
  WETTS_REQUIRE(T >= WETTS_MRD_MIN_SAMPLES, "mrd_spectrogram: T=%d < %d", T, WETTS_MRD_MIN_SAMPLES);
  return launch_stft_cplx(x, rows, T, kMrdWindows[res], kMrdWindows[res] / 4, h->basis[res], mrd_frames(res, T), spec,
                          (hipStream_t)stream);
}

int32_t wetts_mrd_band_conv(const wetts_mrd_t* h, int32_t res, int32_t layer, const float* x, int32_t rows,
                            int32_t frames, float* out, void* stream) {
  WETTS_REQUIRE(h && x && out && res >= 0 && res < kMrdRes && layer >= 0 && layer < kMrdLayers && rows >= 1 && frames >= 1,
                "mrd_band_conv: bad argument");
  const float* in[kMrdBands];
  float* o[kMrdBands];
  int64_t io = 0, oo = 0;
  for (int b = 0; b < kMrdBands; ++b) {
    in[b] = layer == 0 ? x : x + io;
    o[b] = out + oo;
    io += (int64_t)rows * mrd_layout().band[res][b][layer].Cin * frames * mrd_width(res, b, layer);
    oo += (int64_t)rows * kMrdC * frames * mrd_width(res, b, layer + 1);
  }
  return launch_band_conv(h, res, layer, in, rows, frames, o, (hipStream_t)stream);
}

int32_t wetts_mrd_conv_post(const wetts_mrd_t* h, int32_t res, const float* x, int32_t rows, int32_t frames, float* out,
                            void* stream) {
  WETTS_REQUIRE(h && x && out && res >= 0 && res < kMrdRes && rows >= 1 && frames >= 1, "mrd_conv_post: bad argument");
  const float* in[kMrdBands];
  int64_t io = 0;
  for (int b = 0; b < kMrdBands; ++b) {
    in[b] = x + io;
    io += (int64_t)rows * kMrdC * frames * mrd_width(res, b, kMrdLayers);
  }
  return launch_mrd_post(h, res, in, rows, frames, out, (hipStream_t)stream);
}

int32_t wetts_mrd_forward(const wetts_mrd_t* h, const float* y, const float* y_hat, int32_t B, int32_t T,
                          float* const* fmaps_host, void* workspace, int64_t workspace_bytes, void* stream) {
  WETTS_REQUIRE(h && y && y_hat && fmaps_host && workspace, "null argument");
  WETTS_REQUIRE(B >= 1 && B <= 2048, "mrd_forward: B=%d outside [1, 2048]", B);
  WETTS_REQUIRE(T >= WETTS_MRD_MIN_SAMPLES,
                "mrd_forward: T=%d < %d: the centring reflect pad of the 2048 window needs more than 1024 samples", T,
                WETTS_MRD_MIN_SAMPLES);
  for (int i = 0; i < kMrdNumFmaps; ++i) WETTS_REQUIRE(fmaps_host[i] != nullptr, "mrd_forward: fmap %d is null", i);
  WETTS_REQUIRE(workspace_bytes >= wetts_mrd_workspace_bytes(B, T), "mrd_forward: workspace has %lld bytes, needs %lld",
                (long long)workspace_bytes, (long long)wetts_mrd_workspace_bytes(B, T));
  hipStream_t s = (hipStream_t)stream;
  const int B2 = 2 * B;
  int64_t n_norm, n_spec, n_l0;
  mrd_ws_parts(B2, T, &n_norm, &n_spec, &n_l0);
  float* norm = (float*)workspace;
  float* spec = norm + n_norm;
  float* l0 = spec + n_spec;
  WETTS_TRY(launch_normalize(y, y_hat, B, B2, T, norm, s));
  for (int r = 0; r < kMrdRes; ++r) {
    const int frames = mrd_frames(r, T);
    float* const* f = fmaps_host + r * kMrdMapsPerRes;
    WETTS_TRY(launch_stft_cplx(norm, B2, T, kMrdWindows[r], kMrdWindows[r] / 4, h->basis[r], frames, spec, s));
    const float* in[kMrdBands];
    float* out[kMrdBands];
    int64_t oo = 0;
    for (int b = 0; b < kMrdBands; ++b) {
      in[b] = spec;
      out[b] = l0 + oo;
      oo += (int64_t)B2 * kMrdC * frames * mrd_width(r, b, 1);
    }
    WETTS_TRY(launch_band_conv(h, r, 0, in, B2, frames, out, s));
    for (int m = 1; m < kMrdLayers; ++m) {
      for (int b = 0; b < kMrdBands; ++b) {
        in[b] = out[b];
        out[b] = f[4 * b + m - 1];
      }
      WETTS_TRY(launch_band_conv(h, r, m, in, B2, frames, out, s));
    }
    for (int b = 0; b < kMrdBands; ++b) in[b] = out[b];
    WETTS_TRY(launch_mrd_post(h, r, in, B2, frames, f[kMrdMapsPerRes - 1], s));
  }
  for (int d = 0; d < 5; ++d)
    WETTS_TRY(disc_period_stack(mrd_layout().period[d], h->blob, kDiscPeriods[d], y, y_hat, B, B2, T,
                                fmaps_host + kMrdRes * kMrdMapsPerRes + 6 * d, s));
  return WETTS_OK;
}

}  // extern "C"
