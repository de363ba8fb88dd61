// A ResBlock1 (c1, c2) pair at float32 in ONE launch with both convs in F(2,3) minimal-filtering form:
//
//   out = (x + c2(lrelu(c1(lrelu(x)))) [+ out]) / div          c1 at dilation d, c2 at 1, k in {7, 11} taps
//
// The tile geometry and the phases are resblock_chain32.hip's (all C rows of lrelu(x) resident in one LDS tile, the
// intermediate never leaves the CU), the MFMA loop is conv_f23_body's (conv_mfma.hip: four transform-domain accumulators
// per 32 rows x 32 output pairs, input differences taken at the B-fragment read, the packed `wf23` A stream through a
// register ring): 10 / 15 MFMAs per k-step where resblock_chain32_kernel issues 14 / 22.  A kernel of its own, because
// the form wants what that kernel cannot give: a compile-time slot count, four accumulators per 32 PAIRS, and another
// order of the f32 sums -- its results are NOT bit-identical to the conv-by-conv path (tests/test_gpu_chain_pair_f23.py
// holds it to the float64 oracle instead).  launch_resblock_chain32 decides which kernel a launch takes.
//
// Tile.  Four waves, WM = C / 32 of them over rows, WN = 4 / WM over pairs: NP = 32 WN pairs = 2 NP columns of c2.
// Tile column c is time t0 + c, t0 = ntile * NTO - S_left: the origin is a function of absolute time only, and
// PAIRING IS BY TILE COLUMN: pair q of a conv at dilation d has the base column q + d (q / d) and the partner + d (c2:
// columns 2q, 2q + 1).  So a row decoded alone, a ragged row and a second call compute every sample by the same
// instructions on the same operands -- the same bits.  c1 and c2 give a lane different columns; the intermediate
// passes through LDS anyway.
//
// Coverage.  NP pairs at dilation d cover the columns [0, cov) without holes, cov = 2d (NP / d) + (NP mod d); the
// partners of the last NP mod d pairs lie behind a hole (they are computed and written, and never read by a valid
// output).  c1 reads staged x on both sides, so all its cov outputs are exact; c2 loses hk = (k - 1) / 2 columns per
// side.  Valid outputs of the tile: columns [S_left, S_left + NTO), S_left = hk rounded up to even, NTO =
// (cov - hk - S_left) rounded down to even (t0 is even: the pair (x[2q], x[2q + 1]) is one 8-byte access); the 2 - 6
// columns that cov is short of 2 NP at d = 3, 5 are extra right-side halo.  chain_f23_geometry() is the one place that
// computes this (restated in tests/test_cpu_chain_pair_f23.py).
//
// LDS tile [C][W]: LDS column L is time t0 - M + L, M = Mmin + ((t0 - Mmin) & 3) the left margin (the staged window
// starts on a 16-byte boundary), Mmin = the widest half-width.  The row stride W is a compile-time constant (the
// k-step offsets of the B reads are instruction immediates); Wst <= W columns are staged.  Positions outside [0, Tb)
// are zero at both stages (each conv pads ITS input).
//
// Sum order, per output pair (t, t') = (base, partner) of a conv, as in conv_mfma.hip's F(2,3) section:
//   init  m0 = bias (c1)  |  ((x[t] + out[t]) + bias) (c2; `+ out` only with the running MRF sum),
//         m3 = -(the same at t'),  m1 = m2 = 0;
//   every m_q one sequential f32 fma chain: 16-channel chunk -> channel pair (k-step) -> groups -> the leftover
//   taps (k = 7: one tap on m0, m3; k = 11: the F(2,2) group on m0, m1, m3) -> the two channels of the pair;
//   y[t] = (m0 + m1) + m2,  y[t'] = (m1 - m2) - m3;   c1: lrelu(y) into the tile;  c2: y / div stored.
// Input differences and transformed weights are rounded once each (the weights at pack time, from float64).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "resblock32.h"

namespace wetts {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));

constexpr int kBufRsrcDword3 = 0x00020000;  // gfx9 family raw buffer: 32-bit data format, no swizzle

// max(x, slope*x) == (x > 0 ? x : slope*x) for 0 <= slope <= 1 (resblock_chain32.hip)
__device__ __forceinline__ float lrelu2(float x, float slope) {
  const float m = x * slope;
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(m));
  return r;
}

// LDS row stride: the widest staged window of the supported geometries (C = 32: NP = 128, k = 11 at d = 5 stages 312
// columns), a multiple of 4.  Three blocks of 32 x 320 x 4 bytes per CU.
__host__ __device__ constexpr int chain_f23_stride(int C) { return C == 32 ? 320 : 0; }

struct ChainF23Geom {
  int S_left, S_right, NTO;  // tile columns lost per side, valid outputs per tile (both S_left and NTO even)
  int Mmin;                  // widest half-width: the least left margin of the LDS tile
  int Wst;                   // staged columns per row (a multiple of 4): every column a conv reads or writes
};

// The one place that knows the tile: NP pairs per tile, npairs (c1 at dil[p], c2 at 1) pairs of k-tap convs.
// [vlo, vhi): tile columns whose value is exact at the current stage (x itself is staged on both sides).
static void chain_f23_geometry(int NP, int ktaps, const int* dil, int npairs, ChainF23Geom* g) {
  const int hk = (ktaps - 1) / 2, big = 1 << 20;
  int vlo = -big, vhi = big, m = 0, r = 0;
  for (int pr = 0; pr < npairs; ++pr) {
    const int d = dil[pr], h1 = hk * d;
    const int cov = 2 * d * (NP / d) + NP % d;           // c1's columns without holes
    const int last = (NP - 1) + d * ((NP - 1) / d) + d;  // its last partner column (written too)
    vlo = vlo + h1 > 0 ? vlo + h1 : 0;
    vhi = vhi - h1 < cov ? vhi - h1 : cov;
    if (h1 > m) m = h1;
    if (last + h1 > r) r = last + h1;
    vlo += hk;  // c2: columns 2q, 2q + 1, all of [0, 2 NP)
    vhi = vhi - hk < 2 * NP ? vhi - hk : 2 * NP;
    if (hk > m) m = hk;
    if (2 * NP - 1 + hk > r) r = 2 * NP - 1 + hk;
  }
  g->S_left = (vlo + 1) & ~1;
  g->NTO = (vhi - g->S_left) & ~1;
  g->S_right = 2 * NP - g->S_left - g->NTO;
  g->Mmin = m;
  g->Wst = (m + 3 + r + 1 + 3) & ~3;  // left margin of at most Mmin + 3, columns up to r
}

template <int C, int KT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
void resblock_chain_f23_kernel(const ResChain32Params p) {
  constexpr int WM = C / 32, WN = 4 / WM;
  constexpr int W = chain_f23_stride(C);
  constexpr int NCH = C / kConvCK;
  constexpr int RPW = C / 4;                  // staged rows per wave
  constexpr int QN = (W / 4 + 63) / 64;       // 16-byte pieces per lane per row
  constexpr int NG = KT / 3, NL = KT % 3, SQ = f23_quads(KT);
  constexpr int NS = KT == 11 ? 2 : 4;        // A register sets (conv_f23_body's ring)
  constexpr int HK = (KT - 1) / 2;
  static_assert(W > 0 && W % 4 == 0, "unsupported channel count");

  extern __shared__ __attribute__((aligned(16))) float smem_f[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int half = lane >> 5;

  int bid = blockIdx.x;
  {  // XCD-aware tile order: neighbouring tiles (shared halos) on one XCD's L2
    const int per = (p.nblocks + 7) >> 3;
    bid = (bid & 7) * per + (bid >> 3);
    if (bid >= p.nblocks) return;
  }
  const int ntile = bid % p.ntiles;
  int b = bid / p.ntiles;
  if (p.lens) b = (int)(((int64_t)b * p.bstride) % p.B);  // ragged: mix long and short utterances per XCD
  const int n0 = ntile * p.NTO;
  const int t0 = __builtin_amdgcn_readfirstlane(n0 - p.S);  // time of tile column 0 (even)
  const int M = p.Mmin + ((t0 - p.Mmin) & 3);               // left margin: (t0 - M) % 4 == 0
  const int tx0 = t0 - M;                                   // time of LDS column 0
  const int Wst = p.Wp;
  const int T = p.T;  // row stride of the [C][T] planes
  const int Tb = p.lens ? __builtin_amdgcn_readfirstlane(min((int)p.lens[b] * p.len_mul, T)) : T;
  if (n0 >= Tb) return;
  const bool interior = tx0 >= 0 && tx0 + Wst <= Tb;
  const int d = p.dil[0];

  const float* xb = p.x + (int64_t)__builtin_amdgcn_readfirstlane(b) * C * T;
  float* ob = p.out + (int64_t)__builtin_amdgcn_readfirstlane(b) * C * T;
  const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xb), 0, C * T * 4, kBufRsrcDword3);
  // descriptors whose base is (row 0, time t0): t0 < 0 in the first tile of a sequence; columns with t < 0 are never
  // accessed, so the base lying in front of the tensor there is harmless (resblock_chain32.hip)
  const __amdgpu_buffer_rsrc_t rsx0 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xb) + t0, 0, (C * T - t0) * 4, kBufRsrcDword3);
  const __amdgpu_buffer_rsrc_t rso0 = __builtin_amdgcn_make_buffer_rsrc(ob + t0, 0, (C * T - t0) * 4,
                                                                        kBufRsrcDword3);

  const int co_blk = wm * 32;
  const int q = wn * 32 + (lane & 31);  // this lane's pair, in both convs
  const int cb1 = q + d * (q / d);      // c1: base column (partner + d)
  const int cb2 = 2 * q;                // c2: base column (partner + 1)

  // packed A streams of this wave's 32 rows (conv_mfma.hip: [mt32][chunk][k-step][quad][lane][4]); the quads of k-step
  // i live in register set i mod NS and are loaded NS - 1 k-steps ahead (unconditionally: the pack has three zero
  // k-steps behind its end)
  const float4* ab1 = reinterpret_cast<const float4*>(p.wpk[0]) + ((int64_t)wm * NCH * 8 * SQ) * 64 + lane;
  const float4* ab2 = reinterpret_cast<const float4*>(p.wpk[1]) + ((int64_t)wm * NCH * 8 * SQ) * 64 + lane;
  float4 aset[NS][SQ];
  auto a_prologue = [&](const float4* abase) {
#pragma unroll
    for (int i = 0; i < NS - 1; ++i)
#pragma unroll
      for (int s = 0; s < SQ; ++s) aset[i][s] = abase[(i * SQ + s) * 64];
#pragma unroll
    for (int s = 0; s < SQ; ++s) aset[NS - 1][s] = aset[0][s];
  };
  a_prologue(ab1);  // lands behind the staging

  // ---- 1. stage lrelu(x): wave w takes rows w, w+4, ...; a lane takes aligned 16-byte pieces ----------------------
  {
    const int ppr = Wst >> 2;  // pieces per row
    constexpr int RBT = RPW > 8 ? 8 : RPW;
#pragma unroll 1
    for (int r0 = 0; r0 < RPW; r0 += RBT) {
      float4 st[RBT][QN];
      if (interior) {
#pragma unroll
        for (int r = 0; r < RBT; ++r) {
          const int soff = ((wave + 4 * (r0 + r)) * T + tx0) * 4;  // uniform, 16-byte aligned
#pragma unroll
          for (int s = 0; s < QN; ++s) {
            const int seg = lane + 64 * s;
            st[r][s] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (seg < ppr) {
              const f32x4v u = __builtin_amdgcn_raw_buffer_load_b128(rsx, lane * 16 + s * 1024, soff, 0);
              st[r][s] = make_float4(u.x, u.y, u.z, u.w);
            }
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < RBT; ++r) {
          const float* xrow = xb + (int64_t)(wave + 4 * (r0 + r)) * T;
#pragma unroll
          for (int s = 0; s < QN; ++s) {
            const int seg = lane + 64 * s;
            const int t = tx0 + 4 * seg;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (seg < ppr) {  // sequence edge: element-wise, zero outside [0, Tb)
              if (t >= 0 && t < Tb) v.x = xrow[t];
              if (t + 1 >= 0 && t + 1 < Tb) v.y = xrow[t + 1];
              if (t + 2 >= 0 && t + 2 < Tb) v.z = xrow[t + 2];
              if (t + 3 >= 0 && t + 3 < Tb) v.w = xrow[t + 3];
            }
            st[r][s] = v;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < RBT; ++r) {
        float* lrow = smem_f + (size_t)(wave + 4 * (r0 + r)) * W;
#pragma unroll
        for (int s = 0; s < QN; ++s) {
          const int seg = lane + 64 * s;
          if (seg < ppr) {
            float4 v = st[r][s];
            v.x = lrelu2(v.x, p.slope);
            v.y = lrelu2(v.y, p.slope);
            v.z = lrelu2(v.z, p.slope);
            v.w = lrelu2(v.w, p.slope);
            *reinterpret_cast<float4*>(lrow + 4 * seg) = v;
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- the conv loop (conv_f23_body's, without chunk staging: every channel is already in LDS) ---------------------
  // bl0: this lane's LDS word of (k-step 0, tap 0); k-step s reads rows 2s + half.  Raw B values a[c + off + j dd],
  // j = 0 .. KT, one k-step ahead of their use; the four differences per group are taken here.
  f32x16 m0, m1, m2, m3;
  auto conv_loop = [&](const float4* abase, const float* bl0, auto dd) {
    int st = NS - 1;  // the k-step the next prefetch loads
    float braw[2][KT + 1];
#pragma unroll
    for (int j = 0; j <= KT; ++j) braw[0][j] = bl0[j * dd];
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {
      const float* bl = bl0 + (size_t)c * kConvCK * W;
      const bool more = c + 1 < NCH;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int u = 0; u < SQ; ++u) aset[(s + NS - 1) % NS][u] = abase[((int64_t)st * SQ + u) * 64];
        ++st;
        if (s < 7 || more) {  // (s = 7: k-step 0 of the next chunk)
#pragma unroll
          for (int j = 0; j <= KT; ++j) braw[(s + 1) & 1][j] = bl[2 * (s + 1) * W + j * dd];
        }
        __builtin_amdgcn_sched_barrier(0);  // keep both prefetches ahead of this k-step's MFMAs
        auto A = [&](int slot) {
          const float4 v = aset[s % NS][slot >> 2];
          return (slot & 3) == 0 ? v.x : (slot & 3) == 1 ? v.y : (slot & 3) == 2 ? v.z : v.w;
        };
        const float* a = braw[s & 1];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const float a0 = a[3 * g], a1 = a[3 * g + 1], a2 = a[3 * g + 2], a3 = a[3 * g + 3];
          const float v0 = a0 - a2, v1 = a1 + a2, v2 = a2 - a1, v3 = a1 - a3;
          m0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * g + 0), v0, m0, 0, 0, 0);
          m1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * g + 1), v1, m1, 0, 0, 0);
          m2 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * g + 2), v2, m2, 0, 0, 0);
          m3 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * g + 3), v3, m3, 0, 0, 0);
        }
        if (NL == 1) {  // leftover tap i = 3 NG: a[t + off_i] into m0, a[t' + off_i] into m3
          m0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * NG), a[3 * NG], m0, 0, 0, 0);
          m3 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * NG + 1), a[3 * NG + 1], m3, 0, 0, 0);
        } else if (NL == 2) {  // leftover taps 3 NG, 3 NG + 1 as one F(2,2) group on m0, m1, m3
          const float a0 = a[3 * NG], a1 = a[3 * NG + 1], a2 = a[3 * NG + 2];
          const float u0 = a0 - a1, u3 = a1 - a2;
          m0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * NG + 0), u0, m0, 0, 0, 0);
          m1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * NG + 1), a1, m1, 0, 0, 0);
          m3 = __builtin_amdgcn_mfma_f32_32x32x2f32(A(4 * NG + 2), u3, m3, 0, 0, 0);
        }
        // The unused words of the last quad stay allocated to the end of the k-step: left dead, their registers are
        // reused under the 16-byte load in flight and the hazard costs an s_waitcnt vmcnt(0) behind every prefetch
        // (conv_f23_body).  No instruction is emitted.
        if (f23_slots(KT) % 4 != 0) {
          if (f23_slots(KT) % 4 <= 2) asm volatile("" : : "v"(aset[s % NS][SQ - 1].z));
          asm volatile("" : : "v"(aset[s % NS][SQ - 1].w));
        }
      }
    }
  };

  // ---- c1: m0 = b1, m3 = -b1 ----------------------------------------------------------------------------------------
  {
    const float* bp = p.bias[0] + co_blk + 4 * half;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float bv = bp[(r & 3) + 8 * (r >> 2)];
      m0[r] = bv;
      m3[r] = -bv;
      m1[r] = 0.f;
      m2[r] = 0.f;
    }
  }
  conv_loop(ab1, smem_f + (size_t)half * W + M + cb1 - HK * d, d);

  // c2's first A quads and the residual pair (x[2q], x[2q + 1]) land behind the write pass.  Stored columns only:
  // [S_left, S_left + NTO) and inside the utterance (S_left, NTO, t0 and Tb are even: a pair is stored whole or not).
  a_prologue(ab2);
  const bool ok = cb2 >= p.S && cb2 < p.S + p.NTO && t0 + cb2 < Tb;  // t0 + cb2 >= n0 >= 0 inside the window
  const int lane_off = ((co_blk + 4 * half) * T + cb2) * 4;         // bytes from (row 0, time t0)
  f32x2v xr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int soff = ((r & 3) + 8 * (r >> 2)) * T * 4;  // uniform
    xr[r] = f32x2v{0.f, 0.f};
    if (ok) xr[r] = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rsx0, lane_off, soff, 0));
  }

  // ---- ft = lrelu(c1) over the tile, zero outside [0, Tb): c2 pads ITS input ---------------------------------------
  {
    const int tc = t0 + cb1;
    const float k0 = (tc >= 0 && tc < Tb) ? 1.f : 0.f;  // (edge tiles only)
    const float k1 = (tc + d >= 0 && tc + d < Tb) ? 1.f : 0.f;
    float* w0 = smem_f + (size_t)(co_blk + 4 * half) * W + M + cb1;
    float* w1 = w0 + d;
    __syncthreads();  // every wave has finished reading lrelu(x)
    if (interior) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ro = ((r & 3) + 8 * (r >> 2)) * W;
        w0[ro] = lrelu2((m0[r] + m1[r]) + m2[r], p.slope);
        w1[ro] = lrelu2((m1[r] - m2[r]) - m3[r], p.slope);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ro = ((r & 3) + 8 * (r >> 2)) * W;
        w0[ro] = lrelu2((m0[r] + m1[r]) + m2[r], p.slope) * k0;
        w1[ro] = lrelu2((m1[r] - m2[r]) - m3[r], p.slope) * k1;
      }
    }
  }
  // the running MRF sum: requested once c1's accumulators are dead, it lands behind the barrier
  f32x2v pv[16];
  if (p.accum) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int soff = ((r & 3) + 8 * (r >> 2)) * T * 4;
      pv[r] = f32x2v{0.f, 0.f};
      if (ok) pv[r] = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rso0, lane_off, soff, 0));
    }
  }
  __syncthreads();

  // ---- c2: m0 = (x[t] [+ out[t]]) + b2, m3 = -(the same at t + 1) ---------------------------------------------------
  {
    const float* bp = p.bias[1] + co_blk + 4 * half;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float bv = bp[(r & 3) + 8 * (r >> 2)];
      float s0 = xr[r].x, s1 = xr[r].y;
      if (p.accum) {
        s0 += pv[r].x;
        s1 += pv[r].y;
      }
      m0[r] = s0 + bv;
      m3[r] = -(s1 + bv);
      m1[r] = 0.f;
      m2[r] = 0.f;
    }
  }
  conv_loop(ab2, smem_f + (size_t)half * W + M + cb2 - HK, std::integral_constant<int, 1>());

  // ---- epilogue: out = y / div, the pair as one 8-byte store -------------------------------------------------------
  auto store_all = [&](auto fin) {
    if (!ok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      f32x2v y;
      y.x = fin((m0[r] + m1[r]) + m2[r]);
      y.y = fin((m1[r] - m2[r]) - m3[r]);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, y), rso0, lane_off,
                                            ((r & 3) + 8 * (r >> 2)) * T * 4, 0);
    }
  };
  const float dv = p.out_div, dinv = 1.f / p.out_div;
  if (dv == 1.f) store_all([](float v) { return v; });
  else if (mrf_div_fast(dv)) store_all([=](float v) { return div_small_const(v, dv, dinv); });
  else store_all([=](float v) { return v / dv; });
}

// ---- dispatch: by geometry and launch size only ---------------------------------------------------------------------
static thread_local int tls_chain_f23_min_tiles = INT32_MAX;
ChainF23Scope::ChainF23Scope(int min_tiles) : prev(tls_chain_f23_min_tiles) { tls_chain_f23_min_tiles = min_tiles; }
ChainF23Scope::~ChainF23Scope() { tls_chain_f23_min_tiles = prev; }

// The geometries the kernel is built for.  C = 32, k = 7 / 11, one pair per launch: the six <32, 3> launches of the
// headline's last stage, adopted from the micro-benchmark (profiles/chain_pair_f23_microbench.txt: both classes faster in
// every run than every run of the parent's library).  Not built, and not tried: k = 3 (C = 32 / 64 whole blocks, C = 128
// pairs) and three-pair launches.  They need what this kernel does not have -- the residual pair held through c1's loop (at
// k = 7 that is 64 + 32 + a 48-register ring + 16 raw B values before any address), an lrelu(x) write-back phase between
// pairs, and at C = 128 a tile of WN = 1, 64 columns, whose halo share has to be measured -- and stay on
// resblock_chain32_kernel; the same file lists their direct-form times.
bool resblock_chain_f23_supported(const PackedConv* c1, const PackedConv* c2, int npairs, const ResChain32Params& p) {
  if (npairs != 1 || c1[0].Cin != 32 || (c1[0].ktaps != 7 && c1[0].ktaps != 11)) return false;
  if (!c1[0].wf23 || !c2[0].wf23 || c1[0].dil < 1) return false;
  if (p.lens && (p.len_mul & 1)) return false;  // pairs are stored whole: every utterance ends on an even sample
  ChainF23Geom g;
  const int dl[1] = {c1[0].dil};
  chain_f23_geometry(128, c1[0].ktaps, dl, 1, &g);
  return g.NTO > 0 && g.Wst <= chain_f23_stride(32) && (int64_t)32 * p.T * 4 < (1ll << 31);
}

// `min_tiles` in 64 x 64 output tiles, like conv_f23_min_tiles (0 forces the form wherever it is built)
bool resblock_chain_f23_take(const PackedConv* c1, const PackedConv* c2, int npairs, const ResChain32Params& p) {
  const int min_tiles = tls_chain_f23_min_tiles;
  if (min_tiles == INT32_MAX || !resblock_chain_f23_supported(c1, c2, npairs, p)) return false;
  return (int64_t)cdiv(c1[0].Cin, 64) * cdiv(p.T, 64) * p.B >= min_tiles;
}

template <int C, int KT>
static int32_t launch_chain_f23(ResChain32Params p, hipStream_t stream) {
  ChainF23Geom g;
  chain_f23_geometry(32 * (4 / (C / 32)), KT, p.dil, p.npairs, &g);
  WETTS_REQUIRE(g.NTO > 0 && g.Wst <= chain_f23_stride(C), "chain halo exceeds the F(2,3) tile");
  p.S = g.S_left;
  p.Mmin = g.Mmin;
  p.NTO = g.NTO;
  p.Wp = g.Wst;
  p.ntiles = cdiv(p.T, p.NTO);
  const int64_t nb = (int64_t)p.ntiles * p.B;
  if (nb <= 0) return WETTS_OK;
  WETTS_REQUIRE(nb < (1ll << 30), "resblock grid too large");
  WETTS_REQUIRE(p.T % 4 == 0 && ((uintptr_t)p.x & 15) == 0 && ((uintptr_t)p.out & 7) == 0,
                "chain kernel needs 16-byte aligned rows");
  p.nblocks = (int)nb;
  const unsigned grid = (unsigned)(((nb + 7) / 8) * 8);
  const size_t lds = (size_t)C * chain_f23_stride(C) * sizeof(float);
  hipLaunchKernelGGL((resblock_chain_f23_kernel<C, KT>), dim3(grid), dim3(256), lds, stream, p);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

// p: filled by launch_resblock_chain32 (dil, bias, npairs, ktaps, bstride); the weights are the F(2,3) packs
int32_t launch_resblock_chain_f23(const PackedConv* c1, const PackedConv* c2, int npairs, ResChain32Params p,
                                  hipStream_t stream) {
  WETTS_REQUIRE(resblock_chain_f23_supported(c1, c2, npairs, p), "resblock chain shape not built in F(2,3) form");
  p.wpk[0] = c1[0].wf23;
  p.wpk[1] = c2[0].wf23;
  return p.ktaps == 7 ? launch_chain_f23<32, 7>(p, stream) : launch_chain_f23<32, 11>(p, stream);
}

}  // namespace wetts
