// The VITS2 duration discriminators (discriminators.py:287-449: DurationDiscriminatorV1 / V2) without gradients, and the
// row means their losses need.  All f32, wave64, on the caller's stream.
//
// Layout.  The trunk (conv_1, conv_2) runs on the B rows of hidden_x.  The head (pre_out_conv_1, pre_out_conv_2, the
// Linear + sigmoid) runs on 2B rows, dur_r's first, so every weight is read once; head row r reads trunk row r mod B and
// mask row r mod B, and the trunk's output is not duplicated.  Four launches of one kernel.
//
// Every output element is a function of its own row, position and the channel order alone: a column resolves the zero
// pad at its own row's end, accumulates its own k sequence, and its LayerNorm / Linear sums run over the channels in an
// order fixed by the block shape.  A row alone, the same row inside a padded batch and the real half under any pairing
// give the same bits.
#include "common.h"

#include <vector>

namespace wetts {

typedef float f32x16q __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// f32 implicit-GEMM Conv1d, K taps (odd, <= 7), pad K / 2, stride 1, over independent rows of Tx positions:
//   D[F x (rows * Tx)] = W[F x (Cin * K)] * Bm,   Bm[(ci, tap)][(row, t)] = in[row][ci][t + tap - K / 2] * mask[row][..]
// The columns are the (row, t) pairs of all rows laid end to end (rows are ~100 phonemes: one tile per row would idle);
// each column resolves the padding at its own row's Tx.  A block of four waves owns ALL F <= 256 output channels of its
// 64 columns -- wave (wm, wn) the 32-channel tiles wm, wm + 2, .. of the 32 columns wn -- so the channel LayerNorm is an
// epilogue: each lane adds its own 8 channels per tile in ascending order, the four (wm, half) partial sums of a column
// meet in LDS as (p0 + p1) + (p2 + p3), first for the mean, then for the centred squares.  No atomics.
// The k sum is blocked by chunk as in strided_conv_mfma_kernel: CK input channels (CK * K <= 48 k values) are staged,
// their products meet in accumulators of their own, which then join the running sum.  Weights stay in the natural
// [F][Cin][K] layout: a chunk is CK * K contiguous floats per channel, rows of As padded to an odd stride.
// MODE_CAT (pre_out_conv_1): the input channels Cx .. Cx + F - 1 are dur_proj's output formed while staging,
// (w_d[c] * dur[row][t] + b_d[c]) * mask; neither it nor the concatenation is stored.  MODE_HEAD (pre_out_conv_2): the
// epilogue also multiplies by the mask, forms the Linear(F, 1) dot product in the same fixed order and stores the sigmoid.
// 63 KB of LDS: two blocks per CU, two waves per SIMD, for F <= 192 (NT <= 3: at most 256 registers); F = 224 and 256
// hold 8 accumulator tiles per wave and run one block per CU.
constexpr int kQN = 64, kQMaxF = 256, kQMaxKC = 48, kQPer = kQMaxKC / 4;
constexpr float kQEps = 1e-5f;  // normalization.py:8
enum { MODE_PLAIN = 0, MODE_CAT = 1, MODE_HEAD = 2 };

struct DurConvParams {
  const float* x;     // [.][Cx][Tx]; output row r reads row r % x_mod
  const float* mask;  // [m_mod][Tx]; output row r reads row r % m_mod
  const float *dur, *dur2;  // MODE_CAT: [split][Tx] for rows < split, then rows - split
  const float *wd, *bd;     // dur_proj
  const float* w;           // [F][Cin][K]
  const float *bias, *gamma, *beta;
  const float *wout, *bout;  // MODE_HEAD
  float* out;                // [rows][F][Tx]
  float* prob;               // [rows][Tx]
  int64_t ncols;
  int x_mod, m_mod, split, Cx, Cin, F, K, CK, Tx;
};

// NT: 32-channel tiles per wave, ceil(F / 64).  Where F / 32 is odd, the last tile of the waves wm = 1 meets zero rows of
// As and is not stored.
template <bool LN, int MODE, int NT>
__global__ void __launch_bounds__(256, NT <= 3 ? 2 : 1) dur_disc_conv_kernel(DurConvParams p) {
  __shared__ float As[kQMaxF * (kQMaxKC + 1)];
  __shared__ float Bs[kQMaxKC * kQN];
  __shared__ float part1[4][kQN], part2[4][kQN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, KC = p.CK * K, lda = KC + 1, pad = K >> 1, Tx = p.Tx, F = p.F, Cin = p.Cin;
  const int64_t n0 = (int64_t)blockIdx.x * kQN;

  // B staging: this thread's column and the k values cg, cg + 4, .. of a chunk; what does not change from chunk to chunk
  // (the tap's offset, its mask value, its duration) is read once
  const int scol = tid & 63, cg = tid >> 6;
  const int64_t sj = n0 + scol;
  const bool s_ok = sj < p.ncols;
  const int srow = s_ok ? (int)(sj / Tx) : 0;
  const int st = s_ok ? (int)(sj - (int64_t)srow * Tx) : 0;
  const float* xb = p.x + (int64_t)(srow % p.x_mod) * p.Cx * Tx;
  const float* mb = p.mask + (int64_t)(srow % p.m_mod) * Tx;
  const float* db = nullptr;
  if (MODE == MODE_CAT) db = srow < p.split ? p.dur + (int64_t)srow * Tx : p.dur2 + (int64_t)(srow - p.split) * Tx;
  int eoff[kQPer];
  float em[kQPer], ed[kQPer];
  unsigned ok = 0;
#pragma unroll
  for (int j = 0; j < kQPer; ++j) {
    const int e = cg + 4 * j, ci = e / K, tin = st + (e - ci * K) - pad;
    const bool v = s_ok && e < KC && tin >= 0 && tin < Tx;
    eoff[j] = ci * Tx + tin;
    em[j] = v ? mb[tin] : 0.f;
    ed[j] = (MODE == MODE_CAT && v) ? db[tin] : 0.f;
    ok |= (v ? 1u : 0u) << j;
  }

  const int q4 = KC >> 2;
  float br[kQPer];
  auto fetch = [&](int c0) {
    if (MODE == MODE_CAT && c0 >= p.Cx) {
      const float* wd = p.wd + (c0 - p.Cx);
      const float* bd = p.bd + (c0 - p.Cx);
#pragma unroll
      for (int j = 0; j < kQPer; ++j) {
        const int ci = (cg + 4 * j) / K;
        br[j] = (ok >> j) & 1u ? __builtin_fmaf(wd[ci], ed[j], bd[ci]) * em[j] : 0.f;
      }
    } else {
      const float* xc = xb + (int64_t)c0 * Tx;
#pragma unroll
      for (int j = 0; j < kQPer; ++j) br[j] = (ok >> j) & 1u ? xc[eoff[j]] * em[j] : 0.f;
    }
  };

  f32x16q zero;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero[r] = 0.f;
  f32x16q acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = zero;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31, nmt = F >> 5;
  const int bcol = wn * 32 + l31;

  for (int i = F * lda + tid; i < 64 * NT * lda; i += 256) As[i] = 0.f;  // the rows of a tile beyond F
  fetch(0);
  for (int c0 = 0; c0 < Cin; c0 += p.CK) {
    // A: thread (r = tid / 4 + 64 jj, quad = tid % 4 + 4 qq); the weights are not prefetched (the registers go to the
    // accumulators), they come from L2 for every block but the first
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int r = (tid >> 2) + 64 * jj;
      if (r < F) {
        const float* wr = p.w + ((int64_t)r * Cin + c0) * K;
        float4 av[3];
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) {
          const int q = (tid & 3) + 4 * qq;
          if (q < q4) av[qq] = *reinterpret_cast<const float4*>(wr + q * 4);
        }
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) {
          const int q = (tid & 3) + 4 * qq;
          if (q < q4) {
            float* a = As + r * lda + q * 4;
            a[0] = av[qq].x;
            a[1] = av[qq].y;
            a[2] = av[qq].z;
            a[3] = av[qq].w;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kQPer; ++j)
      if (cg + 4 * j < KC) Bs[(cg + 4 * j) * kQN + scol] = br[j];
    __syncthreads();
    if (c0 + p.CK < Cin) fetch(c0 + p.CK);
    // blocked summation: a chunk's products meet in accumulators of their own, which then join the running sum
    f32x16q cv[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) cv[i] = zero;
    for (int kk = 0; kk < (KC >> 1); ++kk) {
      const float b = Bs[(2 * kk + half) * kQN + bcol];
#pragma unroll
      for (int i = 0; i < NT; ++i)
        cv[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[((wm + 2 * i) * 32 + l31) * lda + 2 * kk + half], b, cv[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] += cv[i];
    __syncthreads();
  }

  // lane holds channels 32 mt + 8 g + 4 half + {0..3} (register 4 g + ..) of column bcol, for its tiles mt = wm + 2 i
  const int64_t j = n0 + bcol;
  const bool valid = j < p.ncols;
  const int row = valid ? (int)(j / Tx) : 0;
  const int t = valid ? (int)(j - (int64_t)row * Tx) : 0;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NT; ++i)
    if (wm + 2 * i < nmt) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int co = (wm + 2 * i) * 32 + 8 * (q >> 2) + 4 * half + (q & 3);
        float a = acc[i][q] + p.bias[co];
        if (LN) a = fmaxf(a, 0.f);
        acc[i][q] = a;
        s += a;
      }
    }
  if (LN) {
    // F.layer_norm over the channels: biased variance, two passes
    part1[wm * 2 + half][bcol] = s;
    __syncthreads();
    const float mean = ((part1[0][bcol] + part1[1][bcol]) + (part1[2][bcol] + part1[3][bcol])) / (float)F;
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i)
      if (wm + 2 * i < nmt) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float d = acc[i][q] - mean;
          acc[i][q] = d;
          s2 = __builtin_fmaf(d, d, s2);
        }
      }
    part2[wm * 2 + half][bcol] = s2;
    __syncthreads();
    const float var = ((part2[0][bcol] + part2[1][bcol]) + (part2[2][bcol] + part2[3][bcol])) / (float)F;
    const float rstd = 1.f / sqrtf(var + kQEps);
#pragma unroll
    for (int i = 0; i < NT; ++i)
      if (wm + 2 * i < nmt) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int co = (wm + 2 * i) * 32 + 8 * (q >> 2) + 4 * half + (q & 3);
          acc[i][q] = __builtin_fmaf(acc[i][q] * rstd, p.gamma[co], p.beta[co]);
        }
      }
  }
  if (valid) {
    float* ob = p.out + (int64_t)row * F * Tx + t;
#pragma unroll
    for (int i = 0; i < NT; ++i)
      if (wm + 2 * i < nmt) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int co = (wm + 2 * i) * 32 + 8 * (q >> 2) + 4 * half + (q & 3);
          ob[(int64_t)co * Tx] = acc[i][q];
        }
      }
  }
  if (MODE == MODE_HEAD) {
    // (x * x_mask) -> Linear(F, 1) -> sigmoid; a masked column sums zeros and gives sigmoid(bias)
    const float mv = valid ? p.mask[(int64_t)(row % p.m_mod) * Tx + t] : 0.f;
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i)
      if (wm + 2 * i < nmt) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int co = (wm + 2 * i) * 32 + 8 * (q >> 2) + 4 * half + (q & 3);
          z = __builtin_fmaf(p.wout[co], acc[i][q] * mv, z);
        }
      }
    part1[wm * 2 + half][bcol] = z;  // every read of part1 above lies before the second barrier
    __syncthreads();
    if (valid && wm == 0 && half == 0) {
      const float zz = ((part1[0][bcol] + part1[1][bcol]) + (part1[2][bcol] + part1[3][bcol])) + p.bout[0];
      p.prob[(int64_t)row * Tx + t] = 1.f / (1.f + expf(-zz));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Row means of the probabilities, in the reduction order of disc_rows_kernel (discriminator.hip): one block of 256
// threads per row, thread i adds the elements i, i + 256, .. in ascending order into four interleaved float64
// accumulators, (a0 + a1) + (a2 + a3), the butterfly over the lanes, (w0 + w1) + (w2 + w3) over the waves.  Each term is
// formed in f32 as losses.py forms it.
__device__ __forceinline__ double dd_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double dd_block_sum(const double a[4], double* part) {
  const double v = dd_wave_sum((a[0] + a[1]) + (a[2] + a[3]));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (part[0] + part[1]) + (part[2] + part[3]);
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(256)
dur_disc_row_means_kernel(const float* __restrict__ pr, const float* __restrict__ pg, const float* __restrict__ mask, int Tx,
                          float* __restrict__ r_rows, float* __restrict__ g_rows, float* __restrict__ gen_rows,
                          float* __restrict__ disc_pu, float* __restrict__ gen_pu) {
  __shared__ double part[4];
  const int b = blockIdx.x;
  const float* r = pr + (int64_t)b * Tx;
  const float* g = pg + (int64_t)b * Tx;
  const float* m = mask + (int64_t)b * Tx;
  double sr[4] = {0., 0., 0., 0.}, sg[4] = {0., 0., 0., 0.}, sn[4] = {0., 0., 0., 0.};
  double md[4] = {0., 0., 0., 0.}, mn[4] = {0., 0., 0., 0.}, cnt[4] = {0., 0., 0., 0.};
  int k = 0;
  for (int e = threadIdx.x; e < Tx; e += 256, ++k) {
    const float rv = r[e], gv = g[e];
    const float dr = 1.f - rv, dg = 1.f - gv;
    const float tr = dr * dr, tg = gv * gv, tn = dg * dg;
    sr[k & 3] += tr;
    sg[k & 3] += tg;
    sn[k & 3] += tn;
    if (m[e] != 0.f) {
      md[k & 3] += (double)tr + (double)tg;
      mn[k & 3] += tn;
      cnt[k & 3] += 1.;
    }
  }
  const double a_r = dd_block_sum(sr, part), a_g = dd_block_sum(sg, part), a_n = dd_block_sum(sn, part);
  const double m_d = dd_block_sum(md, part), m_n = dd_block_sum(mn, part), c = dd_block_sum(cnt, part);
  if (threadIdx.x == 0) {
    r_rows[b] = (float)(a_r / (double)Tx);
    g_rows[b] = (float)(a_g / (double)Tx);
    gen_rows[b] = (float)(a_n / (double)Tx);
    disc_pu[b] = (float)(m_d / c);  // 0 / 0 = NaN for a row without phonemes
    gen_pu[b] = (float)(m_n / c);
  }
}

// ---------------------------------------------------------------------------------------------
// host side: the blob layout of a (version, in_channels, filter_channels, kernel_size), the handle, the launchers
struct DurTensor {
  std::string name;
  int64_t offset, numel, shape[4];
};

struct DurLayout {
  std::vector<DurTensor> tensors;
  int64_t total = 0;
  int64_t off(const std::string& name) const {
    for (const DurTensor& t : tensors)
      if (t.name == name) return t.offset;
    return -1;
  }
};

static bool dur_config_ok(int version, int Cin, int F, int K) {
  return (version == 1 || version == 2) && Cin >= 32 && Cin <= kQMaxF && Cin % 32 == 0 && F >= 32 && F <= kQMaxF &&
         F % 32 == 0 && K >= 1 && K <= 7 && (K & 1) == 1;
}

static DurLayout dur_layout(int version, int Cin, int F, int K) {
  DurLayout l;
  auto add = [&](const std::string& name, int64_t s0, int64_t s1, int64_t s2) {
    DurTensor t;
    t.name = name;
    t.offset = l.total;
    t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = 0;
    t.numel = s0 * (s1 > 0 ? s1 : 1) * (s2 > 0 ? s2 : 1);
    l.total = align_up(l.total + t.numel, 64);
    l.tensors.push_back(t);
  };
  auto conv = [&](const std::string& name, int ci, const char* norm) {
    add(name + ".weight", F, ci, K);
    add(name + ".bias", F, 0, 0);
    if (version == 2) {
      add(std::string(norm) + ".gamma", F, 0, 0);
      add(std::string(norm) + ".beta", F, 0, 0);
    }
  };
  conv("conv_1", Cin, "norm_1");
  conv("conv_2", F, "norm_2");
  add("dur_proj.weight", F, 1, 1);
  add("dur_proj.bias", F, 0, 0);
  conv("pre_out_conv_1", 2 * F, "pre_out_norm_1");
  conv("pre_out_conv_2", F, "pre_out_norm_2");
  add("output_layer.0.weight", 1, F, 0);
  add("output_layer.0.bias", 1, 0, 0);
  return l;
}

}  // namespace wetts

struct wetts_durdisc {
  int version = 0, Cin = 0, F = 0, K = 0;
  float* blob = nullptr;
  // per layer: weight, bias, gamma, beta (null in version 1)
  const float *w[4] = {}, *b[4] = {}, *gamma[4] = {}, *beta[4] = {};
  const float *wd = nullptr, *bd = nullptr, *wout = nullptr, *bout = nullptr;
};

namespace wetts {

static int dur_chunk_channels(int K) { return K == 1 ? 32 : K == 3 ? 16 : K == 5 ? 8 : 4; }

static int32_t launch_dur_layer(const wetts_durdisc* h, int layer, const float* x, const float* mask, const float* dur,
                                const float* dur2, int split, int rows, int src_rows, int Tx, float* out, float* prob,
                                hipStream_t s) {
  WETTS_REQUIRE(layer >= 0 && layer <= 3, "durdisc: layer %d is not one of 0..3", layer);
  WETTS_REQUIRE(x && mask && out && rows >= 1 && src_rows >= 1 && src_rows <= rows && Tx >= 1,
                "durdisc: bad layer argument (rows=%d src_rows=%d Tx=%d)", rows, src_rows, Tx);
  WETTS_REQUIRE(layer != 2 || (dur && dur2 && split >= 0 && split <= rows), "durdisc: layer 2 needs the durations");
  WETTS_REQUIRE(layer != 3 || prob, "durdisc: layer 3 needs the probability buffer");
  const int64_t ncols = (int64_t)rows * Tx;
  WETTS_REQUIRE((ncols + kQN - 1) / kQN <= 0x7fffffff, "durdisc: %lld columns exceed one launch", (long long)ncols);
  DurConvParams p;
  memset(&p, 0, sizeof(p));
  p.x = x;
  p.mask = mask;
  p.dur = dur;
  p.dur2 = dur2;
  p.split = split;
  p.wd = h->wd;
  p.bd = h->bd;
  p.w = h->w[layer];
  p.bias = h->b[layer];
  p.gamma = h->gamma[layer];
  p.beta = h->beta[layer];
  p.wout = h->wout;
  p.bout = h->bout;
  p.out = out;
  p.prob = prob;
  p.ncols = ncols;
  p.x_mod = layer == 2 ? src_rows : rows;
  p.m_mod = src_rows;
  p.Cx = layer == 0 ? h->Cin : h->F;
  p.Cin = layer == 2 ? 2 * h->F : p.Cx;
  p.F = h->F;
  p.K = h->K;
  p.CK = dur_chunk_channels(h->K);
  p.Tx = Tx;
  static_assert(kQMaxF * (kQMaxKC + 1) * 4 + kQMaxKC * kQN * 4 + 2 * 4 * kQN * 4 <= 64 * 1024, "dur disc conv LDS");
  const dim3 grid((unsigned)((ncols + kQN - 1) / kQN)), block(256);
  const bool ln = h->version == 2;
  const int nt = (h->F / 32 + 1) / 2;
#define WETTS_DUR_LAUNCH(LN_, MODE_)                                                                          \
  switch (nt) {                                                                                               \
    case 1: hipLaunchKernelGGL((dur_disc_conv_kernel<LN_, MODE_, 1>), grid, block, 0, s, p); break;           \
    case 2: hipLaunchKernelGGL((dur_disc_conv_kernel<LN_, MODE_, 2>), grid, block, 0, s, p); break;           \
    case 3: hipLaunchKernelGGL((dur_disc_conv_kernel<LN_, MODE_, 3>), grid, block, 0, s, p); break;           \
    default: hipLaunchKernelGGL((dur_disc_conv_kernel<LN_, MODE_, 4>), grid, block, 0, s, p); break;          \
  }
  if (layer == 2) {
    if (ln) WETTS_DUR_LAUNCH(true, MODE_CAT) else WETTS_DUR_LAUNCH(false, MODE_CAT)
  } else if (layer == 3) {
    if (ln) WETTS_DUR_LAUNCH(true, MODE_HEAD) else WETTS_DUR_LAUNCH(false, MODE_HEAD)
  } else {
    if (ln) WETTS_DUR_LAUNCH(true, MODE_PLAIN) else WETTS_DUR_LAUNCH(false, MODE_PLAIN)
  }
#undef WETTS_DUR_LAUNCH
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// the five regions of the workspace, in floats
static void dur_regions(int F, int B, int Tx, int64_t off[6]) {
  const int64_t map = (int64_t)B * F * Tx;
  const int64_t sizes[5] = {map, map, 2 * map, 2 * map, (int64_t)2 * B * Tx};
  off[0] = 0;
  for (int i = 0; i < 5; ++i) off[i + 1] = off[i] + align_up(sizes[i], 64);
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_durdisc_blob_num_tensors(int32_t version, int32_t in_channels, int32_t filter_channels, int32_t kernel_size) {
  if (!dur_config_ok(version, in_channels, filter_channels, kernel_size)) {
    set_error("durdisc: version %d, %d -> %d channels, %d taps is not supported", version, in_channels, filter_channels,
              kernel_size);
    return -1;
  }
  return (int32_t)dur_layout(version, in_channels, filter_channels, kernel_size).tensors.size();
}

int32_t wetts_durdisc_blob_tensor_info(int32_t version, int32_t in_channels, int32_t filter_channels, int32_t kernel_size,
                                       int32_t index, char* name_buf, size_t name_buf_len, int64_t* offset, int64_t* numel,
                                       int64_t shape[4]) {
  WETTS_REQUIRE(dur_config_ok(version, in_channels, filter_channels, kernel_size),
                "durdisc: version %d, %d -> %d channels, %d taps is not supported", version, in_channels, filter_channels,
                kernel_size);
  const DurLayout L = dur_layout(version, in_channels, filter_channels, kernel_size);
  WETTS_REQUIRE(index >= 0 && index < (int32_t)L.tensors.size(), "tensor index %d out of range", index);
  const DurTensor& t = L.tensors[index];
  WETTS_REQUIRE(name_buf && name_buf_len > t.name.size(), "name buffer too small");
  strcpy(name_buf, t.name.c_str());
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  return WETTS_OK;
}

int64_t wetts_durdisc_blob_numel(int32_t version, int32_t in_channels, int32_t filter_channels, int32_t kernel_size) {
  if (!dur_config_ok(version, in_channels, filter_channels, kernel_size)) {
    set_error("durdisc: version %d, %d -> %d channels, %d taps is not supported", version, in_channels, filter_channels,
              kernel_size);
    return -1;
  }
  return dur_layout(version, in_channels, filter_channels, kernel_size).total;
}

int32_t wetts_durdisc_create(int32_t version, int32_t in_channels, int32_t filter_channels, int32_t kernel_size,
                             const float* blob_dev, int64_t blob_numel, void* stream, wetts_durdisc_t** out) {
  WETTS_REQUIRE(out != nullptr && blob_dev != nullptr, "null argument");
  WETTS_REQUIRE(dur_config_ok(version, in_channels, filter_channels, kernel_size),
                "durdisc: version %d, %d -> %d channels, %d taps is not supported (version 1 | 2; channels: multiples of "
                "32 up to 256; taps: odd, up to 7)", version, in_channels, filter_channels, kernel_size);
  const DurLayout L = dur_layout(version, in_channels, filter_channels, kernel_size);
  WETTS_REQUIRE(blob_numel == L.total, "blob has %lld floats, the duration discriminator layout needs %lld",
                (long long)blob_numel, (long long)L.total);
  wetts_durdisc* h = new wetts_durdisc();
  h->version = version;
  h->Cin = in_channels;
  h->F = filter_channels;
  h->K = kernel_size;
  hipError_t e = hipMalloc((void**)&h->blob, (size_t)blob_numel * sizeof(float));
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->blob, blob_dev, (size_t)blob_numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    set_error("wetts_durdisc_create: %s", hipGetErrorString(e));
    if (h->blob) (void)hipFree(h->blob);
    delete h;
    return WETTS_E_HIP;
  }
  const char* convs[4] = {"conv_1", "conv_2", "pre_out_conv_1", "pre_out_conv_2"};
  const char* norms[4] = {"norm_1", "norm_2", "pre_out_norm_1", "pre_out_norm_2"};
  for (int i = 0; i < 4; ++i) {
    h->w[i] = h->blob + L.off(std::string(convs[i]) + ".weight");
    h->b[i] = h->blob + L.off(std::string(convs[i]) + ".bias");
    if (version == 2) {
      h->gamma[i] = h->blob + L.off(std::string(norms[i]) + ".gamma");
      h->beta[i] = h->blob + L.off(std::string(norms[i]) + ".beta");
    }
  }
  h->wd = h->blob + L.off("dur_proj.weight");
  h->bd = h->blob + L.off("dur_proj.bias");
  h->wout = h->blob + L.off("output_layer.0.weight");
  h->bout = h->blob + L.off("output_layer.0.bias");
  *out = h;
  return WETTS_OK;
}

void wetts_durdisc_destroy(wetts_durdisc_t* h) {
  if (!h) return;
  if (h->blob) (void)hipFree(h->blob);
  delete h;
}

int64_t wetts_durdisc_workspace_bytes(const wetts_durdisc_t* h, int32_t B, int32_t Tx) {
  if (!h || B < 1 || Tx < 1) {
    set_error("durdisc_workspace_bytes: bad argument (B=%d Tx=%d)", B, Tx);
    return -1;
  }
  int64_t off[6];
  dur_regions(h->F, B, Tx, off);
  return off[5] * (int64_t)sizeof(float);
}

int32_t wetts_durdisc_forward(const wetts_durdisc_t* h, const float* x, const float* x_mask, const float* dur_r,
                              const float* dur_hat, int32_t B, int32_t Tx, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  WETTS_REQUIRE(h && x && x_mask && dur_r && dur_hat && workspace, "null argument");
  WETTS_REQUIRE(B >= 1 && B <= (1 << 20) && Tx >= 1, "durdisc_forward: B=%d or Tx=%d out of range", B, Tx);
  int64_t off[6];
  dur_regions(h->F, B, Tx, off);
  WETTS_REQUIRE(workspace_bytes >= off[5] * (int64_t)sizeof(float), "durdisc_forward: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)(off[5] * (int64_t)sizeof(float)));
  float* ws = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  WETTS_TRY(launch_dur_layer(h, 0, x, x_mask, nullptr, nullptr, 0, B, B, Tx, ws + off[0], nullptr, s));
  WETTS_TRY(launch_dur_layer(h, 1, ws + off[0], x_mask, nullptr, nullptr, 0, B, B, Tx, ws + off[1], nullptr, s));
  WETTS_TRY(launch_dur_layer(h, 2, ws + off[1], x_mask, dur_r, dur_hat, B, 2 * B, B, Tx, ws + off[2], nullptr, s));
  return launch_dur_layer(h, 3, ws + off[2], x_mask, nullptr, nullptr, 0, 2 * B, B, Tx, ws + off[3], ws + off[4], s);
}

int32_t wetts_durdisc_layer(const wetts_durdisc_t* h, int32_t layer, const float* x, const float* x_mask, const float* dur,
                            int32_t rows, int32_t src_rows, int32_t Tx, float* out, float* prob, void* stream) {
  WETTS_REQUIRE(h, "null argument");
  return launch_dur_layer(h, layer, x, x_mask, dur, dur, rows, rows, src_rows, Tx, out, prob, (hipStream_t)stream);
}

int32_t wetts_durdisc_row_means(const float* prob_r, const float* prob_g, const float* x_mask, int32_t B, int32_t Tx,
                                float* r_rows, float* g_rows, float* gen_rows, float* disc_per_utt, float* gen_per_utt,
                                void* stream) {
  WETTS_REQUIRE(prob_r && prob_g && x_mask && r_rows && g_rows && gen_rows && disc_per_utt && gen_per_utt, "null argument");
  WETTS_REQUIRE(B >= 1 && Tx >= 1, "durdisc_row_means: B=%d or Tx=%d out of range", B, Tx);
  hipLaunchKernelGGL(dur_disc_row_means_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, prob_r, prob_g, x_mask,
                     Tx, r_rows, g_rows, gen_rows, disc_per_utt, gen_per_utt);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // extern "C"
