// The 16-bit mode of the text frontend's Linears (wetts_frontend_set_precision): Y[N][M] = round16(X[N][K]) round16(W[M][K])^T
// + bias, then the epilogue, on v_mfma_f32_32x32x16_{bf16,f16}.  A = 32 weight rows, B = 32 tokens: both operands are
// contiguous along K, so lane (r, h) of a k step of 16 holds ONE 16-byte piece of ONE row, W[r][16 s + 8 h .. + 7] and
// X[r][16 s + 8 h .. + 7], and no transposed read is needed anywhere.
//
// Numerics.  Both operands are rounded to the type, round to nearest even (the weights once, by fe16_pack_kernel when the
// mode is set; the activations in registers on their way to the MFMA, v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32); products are
// exact in f32 and accumulated in f32; bias, GELU (exact erf form), ReLU and the residual are the f32 epilogues of
// fe_linear_kernel.  Everything else of the frontend stays the f32 code of frontend.hip.  An f16 operand beyond the
// type's range becomes +-inf as IEEE says.
//
// Two kernels, chosen by the shape (N and M, fe16_form):
//   fe16_ksplit_kernel   serving shapes (N <= 64): fe_linear_kernel's block -- 32 weight rows x 64 tokens, K split in
//                        steps of 16 over 8 waves with a ring of 3 steps in flight per wave, the 8 partial tiles added in
//                        LDS in wave order -- streaming each weight once, at half the bytes
//   fe16_tile_kernel     batch shapes: a tiled GEMM, 128 weight rows x 64 or 128 tokens per block of 4 waves (2 x 2), each
//                        wave 64 rows x 32 or 64 tokens = 2 or 4 accumulator tiles, K in steps of 32 through two LDS
//                        buffers (one barrier per step), both operands staged as 16-byte pieces (X converted on the way),
//                        no K split
// K % 8 == 0 makes every piece wholly inside or wholly outside K; a piece outside (the half step of K % 16 == 8, the tail
// of a 32-step) is ZERO on both sides.  Rows / tokens past M / N are read clamped and not stored.
//
// Determinism: an output element accumulates its own k sequence in an order fixed by the kernel form and K alone, so it
// does not depend on its neighbours, on the padding or on the order of the rows; the form depends on N and M, so a row alone
// and the same row in a batch may differ in the last bits (the f32 mode keeps that promise).  No atomics.  (The two tiles
// of fe16_tile_kernel add an element's k steps in the same order, so they give the same bits; only the K split differs.)
#include "conv16_dev.h"
#include "frontend_dev.h"

#include <math.h>

namespace wetts {

enum { FE16_EPI_BIAS = WETTS_FRONTEND_EPI_BIAS, FE16_EPI_GELU = WETTS_FRONTEND_EPI_GELU, FE16_EPI_RELU = WETTS_FRONTEND_EPI_RELU,
       FE16_EPI_RES = WETTS_FRONTEND_EPI_RESIDUAL };

// 8 f32 -> one 16-byte piece of 8 rounded values, k ascending
template <bool F16>
__device__ __forceinline__ uint4 fe16_piece(const float4 a, const float4 b) {
  uint4 p;
  p.x = pk2<F16>(a.x, a.y);
  p.y = pk2<F16>(a.z, a.w);
  p.z = pk2<F16>(b.x, b.y);
  p.w = pk2<F16>(b.z, b.w);
  return p;
}

// ---------------------------------------------------------------------------------------------
// f32 -> 16 bit, round to nearest even, 8 values per thread; n % 8 == 0, both pointers 16-byte aligned
template <bool F16>
__global__ void __launch_bounds__(256)
fe16_pack_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const float4 a = reinterpret_cast<const float4*>(src)[2 * i], b = reinterpret_cast<const float4*>(src)[2 * i + 1];
  reinterpret_cast<uint4*>(dst)[i] = fe16_piece<F16>(a, b);
}

// the shared epilogue: v = four consecutive channels m .. m + 3 of token `col`
template <int EPI>
__device__ __forceinline__ void fe16_store(float v[4], const float* __restrict__ bias, const float* __restrict__ res,
                                           float* __restrict__ Y, int64_t col, int m, int M) {
  const float4 b = *reinterpret_cast<const float4*>(bias + m);
  v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  if (EPI == FE16_EPI_GELU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = 0.5f * v[i] * (1.f + erff(v[i] * 0.70710678118654752f));  // exact erf form
  } else if (EPI == FE16_EPI_RELU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
  } else if (EPI == FE16_EPI_RES) {
    const float4 r = *reinterpret_cast<const float4*>(res + col * M + m);
    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
  }
  float4 o;
  o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
  *reinterpret_cast<float4*>(Y + col * M + m) = o;
}

// ---------------------------------------------------------------------------------------------
// Serving shapes.  Wave w runs the k steps w, w + 8, ..; lane (r, half) of step s reads the piece k = 16 s + 8 half of
// weight row r (16 bytes) and of its one or two tokens (32 bytes of f32 each).  One step of the 8 waves is one 256-byte
// run of every weight row.  The reduction and the store are fe_linear_kernel's.  A ring of 3 steps per wave: 384 k of
// every row in flight per block (fe_linear_kernel: 256), in registers that leave room for two blocks per CU.
constexpr int kFe16Ring = 3;

template <bool F16, int EPI>
__global__ void __launch_bounds__(64 * kFeKG)
fe16_ksplit_kernel(const float* __restrict__ X, const unsigned short* __restrict__ W, const float* __restrict__ bias,
                   const float* __restrict__ res, float* __restrict__ Y, int N, int K, int M) {
  __shared__ float part[kFeKG][2][16][64];
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * kFeNT;
  const bool two = n0 + 32 < N;  // block-uniform: the second column tile has a token
  const int S = (K + 15) >> 4;

  const int mr = min(m0 + l31, M - 1), c0 = min(n0 + l31, N - 1), c1 = min(n0 + 32 + l31, N - 1);
  const unsigned short* wr = W + (int64_t)mr * K + 8 * half;
  const float* x0 = X + (int64_t)c0 * K + 8 * half;
  const float* x1 = X + (int64_t)c1 * K + 8 * half;

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

  const uint4 z4 = {0u, 0u, 0u, 0u};
  const float4 zf = {0.f, 0.f, 0.f, 0.f};
  uint4 ra[kFe16Ring];
  float4 rb0[kFe16Ring][2], rb1[kFe16Ring][2];
  auto load = [&](int i, int s) {
    // the lane's piece lies inside K (always for half 0; for half 1 not in the last step of K % 16 == 8): else zeros
    const bool in = 16 * s + 8 * half < K;
    ra[i] = z4;
    rb0[i][0] = rb0[i][1] = rb1[i][0] = rb1[i][1] = zf;
    if (in) {
      ra[i] = *reinterpret_cast<const uint4*>(wr + 16 * s);
      rb0[i][0] = *reinterpret_cast<const float4*>(x0 + 16 * s);
      rb0[i][1] = *reinterpret_cast<const float4*>(x0 + 16 * s + 4);
      if (two) {
        rb1[i][0] = *reinterpret_cast<const float4*>(x1 + 16 * s);
        rb1[i][1] = *reinterpret_cast<const float4*>(x1 + 16 * s + 4);
      }
    }
  };
#pragma unroll
  for (int i = 0; i < kFe16Ring; ++i) {
    const int s = w + kFeKG * i;
    if (s < S) load(i, s);
  }
  for (int sb = w; sb < S; sb += kFeKG * kFe16Ring) {
#pragma unroll
    for (int i = 0; i < kFe16Ring; ++i) {
      const int s = sb + kFeKG * i;
      if (s < S) {
        const uint4 a = ra[i];
        const uint4 b0 = fe16_piece<F16>(rb0[i][0], rb0[i][1]);
        uint4 b1 = b0;
        if (two) b1 = fe16_piece<F16>(rb1[i][0], rb1[i][1]);
        const int sn = s + kFeKG * kFe16Ring;
        if (sn < S) load(i, sn);
        acc0 = mfma16<F16>(a, b0, acc0);
        if (two) acc1 = mfma16<F16>(a, b1, acc1);
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
  fe16_store<EPI>(v, bias, res, Y, (int64_t)col, m, M);
}

// ---------------------------------------------------------------------------------------------
// Batch shapes.  Block tile: 128 weight rows x 64 NT tokens, K in steps of kT16BK = 32 = two MFMA k steps.  LDS image of
// an operand tile: [row][4 pieces of 16 bytes], 64-byte rows, piece p of row r at slot p ^ ((r >> 2) & 3): a ds_read_b128
// of 16 consecutive rows at one p then covers all 64 banks once (rows 0, 4, 8, 12 would share banks without the XOR), and
// the staging writes of 16 consecutive threads cover 4 whole rows = 256 contiguous bytes.  The same XOR on both sides.
// Staging: thread t owns the pieces t and t + 256 of the weight tile and NT pieces of the token tile (piece q = row q / 4,
// slot q % 4); the loads of step kt + 1 are issued before the MFMAs of step kt and written to the other buffer after
// them, so one barrier per step suffices.
constexpr int kT16BK = 32, kT16M = 128;

__device__ __forceinline__ int fe16_lds_off(int row, int p) { return row * 64 + ((p ^ ((row >> 2) & 3)) << 4); }

template <bool F16, int EPI, int NT>
__global__ void __launch_bounds__(256)
fe16_tile_kernel(const float* __restrict__ X, const unsigned short* __restrict__ W, const float* __restrict__ bias,
                 const float* __restrict__ res, float* __restrict__ Y, int N, int K, int M) {
  constexpr int TN = 64 * NT;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][(kT16M + TN) * 64];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * kT16M, n0 = blockIdx.y * TN;

  // staging sources: row and slot of the thread's pieces (the same slot p for all of them: 256 % 4 == 0)
  const int sp = tid & 3, srow = tid >> 2;
  const unsigned short* wsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) wsrc[i] = W + (int64_t)min(m0 + srow + 64 * i, M - 1) * K + 8 * sp;
  const float* xsrc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) xsrc[i] = X + (int64_t)min(n0 + srow + 64 * i, N - 1) * K + 8 * sp;

  f32x16 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  uint4 ga[2];
  float4 gb[NT][2];
  const uint4 z4 = {0u, 0u, 0u, 0u};
  const float4 zf = {0.f, 0.f, 0.f, 0.f};
  auto gload = [&](int kt) {
    const int k0 = kt * kT16BK;
    const bool in = k0 + 8 * sp < K;  // K % 8 == 0: the piece is wholly inside K or wholly outside
#pragma unroll
    for (int i = 0; i < 2; ++i) ga[i] = z4;
#pragma unroll
    for (int i = 0; i < NT; ++i) gb[i][0] = gb[i][1] = zf;
    if (in) {
#pragma unroll
      for (int i = 0; i < 2; ++i) ga[i] = *reinterpret_cast<const uint4*>(wsrc[i] + k0);
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        gb[i][0] = *reinterpret_cast<const float4*>(xsrc[i] + k0);
        gb[i][1] = *reinterpret_cast<const float4*>(xsrc[i] + k0 + 4);
      }
    }
  };
  auto lstore = [&](int buf) {
    unsigned char* base = lds[buf];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(base + fe16_lds_off(srow + 64 * i, sp)) = ga[i];
#pragma unroll
    for (int i = 0; i < NT; ++i)
      *reinterpret_cast<uint4*>(base + kT16M * 64 + fe16_lds_off(srow + 64 * i, sp)) = fe16_piece<F16>(gb[i][0], gb[i][1]);
  };

  const int nk = (K + kT16BK - 1) / kT16BK;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;  // block-uniform
    if (more) gload(kt + 1);
    const unsigned char* base = lds[kt & 1];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int p = 2 * ks + half;
      uint4 a[2], b[NT];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const uint4*>(base + fe16_lds_off(64 * wm + 32 * i + l31, p));
#pragma unroll
      for (int j = 0; j < NT; ++j)
        b[j] = *reinterpret_cast<const uint4*>(base + kT16M * 64 + fe16_lds_off(32 * NT * wn + 32 * j + l31, p));
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = mfma16<F16>(a[i], b[j], acc[i][j]);
    }
    if (more) lstore((kt + 1) & 1);
    __syncthreads();
  }

  // register 4 g + i of a tile = weight row 8 g + 4 half + i of the tile, token l31
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = n0 + 32 * NT * wn + 32 * j + l31;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int m = m0 + 64 * wm + 32 * i + 8 * g + 4 * half;
        if (col < N && m < M) {
          float v[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          fe16_store<EPI>(v, bias, res, Y, (int64_t)col, m, M);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// Up to 64 tokens the K-split form (one column block: each weight is streamed once).  Beyond, the 128-token tile where
// its grid still has 512 blocks (two per CU of a 256-CU device, the kernel's residency) and the 64-token tile otherwise:
// at 4096 tokens M = 2304 / 3072 (576 / 768 blocks) run 12 / 20 % faster on the wide tile, M = 768 (192 blocks) 15 % slower
// (profiles/frontend16_bench.json).  A constant, not the device's CU count: the form decides the bits.
constexpr int kFe16SmallN = 64, kFe16WideBlocks = 512;

static int fe16_form(int N, int M) {
  if (N <= kFe16SmallN) return 1;
  return (int64_t)cdiv(M, kT16M) * cdiv(N, 128) >= kFe16WideBlocks ? 3 : 2;
}

static const char* fe16_linear_error(const void* x, const void* w, const void* bias, const void* res, const void* y, int N,
                                     int K, int M, int epi, int precision, int form) {
  if (!x || !w || !bias || !y || N < 1) return "bad argument (a null pointer or N < 1)";
  if (K < 8 || K % 8 || M < 4 || M % 4) return "K must be a multiple of 8 and M a multiple of 4";
  if (epi < FE16_EPI_BIAS || epi > FE16_EPI_RES || (epi == FE16_EPI_RES && !res)) return "unknown epilogue, or a residual epilogue without residual";
  if (precision != 1 && precision != 2) return "precision must be 1 (bf16) or 2 (f16)";
  if (form < 0 || form > 3) return "form must be 0 (by N), 1 (K-split), 2 (64-token tile) or 3 (128-token tile)";
  // every operand is read or written in 16-byte pieces (x and w per k piece, bias, residual and y as float4 in fe16_store)
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y | (epi == FE16_EPI_RES ? (uintptr_t)res : 0)) & 15) != 0)
    return "x, weight, bias, residual and out must be 16-byte aligned";
  return nullptr;
}

template <bool F16, int EPI>
static void fe16_launch_form(int form, const float* x, const unsigned short* w, const float* bias, const float* res, float* y,
                             int N, int K, int M, hipStream_t s) {
  if (form == 1) {
    const dim3 grid((unsigned)cdiv(M, 32), (unsigned)cdiv(N, kFeNT));
    hipLaunchKernelGGL((fe16_ksplit_kernel<F16, EPI>), grid, dim3(64 * kFeKG), 0, s, x, w, bias, res, y, N, K, M);
  } else if (form == 2) {
    const dim3 grid((unsigned)cdiv(M, kT16M), (unsigned)cdiv(N, 64));
    hipLaunchKernelGGL((fe16_tile_kernel<F16, EPI, 1>), grid, dim3(256), 0, s, x, w, bias, res, y, N, K, M);
  } else {
    const dim3 grid((unsigned)cdiv(M, kT16M), (unsigned)cdiv(N, 128));
    hipLaunchKernelGGL((fe16_tile_kernel<F16, EPI, 2>), grid, dim3(256), 0, s, x, w, bias, res, y, N, K, M);
  }
}

template <bool F16>
static void fe16_launch_epi(int epi, int form, const float* x, const unsigned short* w, const float* bias, const float* res,
                            float* y, int N, int K, int M, hipStream_t s) {
  switch (epi) {
    case FE16_EPI_BIAS: fe16_launch_form<F16, FE16_EPI_BIAS>(form, x, w, bias, res, y, N, K, M, s); break;
    case FE16_EPI_GELU: fe16_launch_form<F16, FE16_EPI_GELU>(form, x, w, bias, res, y, N, K, M, s); break;
    case FE16_EPI_RELU: fe16_launch_form<F16, FE16_EPI_RELU>(form, x, w, bias, res, y, N, K, M, s); break;
    default: fe16_launch_form<F16, FE16_EPI_RES>(form, x, w, bias, res, y, N, K, M, s); break;
  }
}

int32_t fe_launch_linear16(const float* x, const unsigned short* w16, const float* bias, const float* res, float* y, int N,
                           int K, int M, int epi, int precision, int form, hipStream_t s) {
  const char* e = fe16_linear_error(x, w16, bias, res, y, N, K, M, epi, precision, form);
  WETTS_REQUIRE(e == nullptr, "frontend linear16 (N=%d K=%d M=%d epilogue=%d precision=%d form=%d): %s", N, K, M, epi,
                precision, form, e);
  if (form == 0) form = fe16_form(N, M);
  WETTS_REQUIRE(((int64_t)N + 63) / 64 <= 65535, "frontend linear16: %d tokens exceed one launch", N);
  if (precision == 2)
    fe16_launch_epi<true>(epi, form, x, w16, bias, res, y, N, K, M, s);
  else
    fe16_launch_epi<false>(epi, form, x, w16, bias, res, y, N, K, M, s);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

static int32_t fe16_pack(const float* src, unsigned short* dst, int64_t n, int precision, hipStream_t s) {
  const int64_t n8 = n / 8;
  const dim3 grid((unsigned)((n8 + 255) / 256));
  if (precision == 2)
    hipLaunchKernelGGL(fe16_pack_kernel<true>, grid, dim3(256), 0, s, src, dst, n8);
  else
    hipLaunchKernelGGL(fe16_pack_kernel<false>, grid, dim3(256), 0, s, src, dst, n8);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int32_t wetts_frontend_set_precision(wetts_frontend_t* h, int32_t precision) {
  WETTS_REQUIRE(h != nullptr, "frontend_set_precision: null handle");
  WETTS_REQUIRE(precision >= 0 && precision <= 2, "frontend_set_precision: precision %d must be 0 (f32), 1 (bf16) or 2 (f16)",
                precision);
  if (precision == h->precision) return WETTS_OK;
  const int64_t d = h->cfg.hidden_size;
  unsigned short* buf = nullptr;
  if (precision != 0) {
    // every weight is a multiple of 8 values (hidden_size, both feed-forward widths % 8 == 0): 16-byte pieces throughout
    int64_t total = 0;
    for (const FeBlock& k : h->blocks) total += 4 * d * d + 2 * d * k.ff;
    WETTS_HIP_CHECK(hipMalloc((void**)&buf, (size_t)total * sizeof(unsigned short)));
    unsigned short* p = buf;
    int32_t rc = WETTS_OK;
    for (const FeBlock& k : h->blocks) {
      const float* src[4] = {k.wqkv, k.wo, k.w1, k.w2};
      const int64_t n[4] = {3 * d * d, d * d, d * k.ff, d * k.ff};
      for (int i = 0; i < 4 && rc == WETTS_OK; ++i) {
        rc = fe16_pack(src[i], p, n[i], precision, nullptr);
        p += n[i];
      }
    }
    if (rc == WETTS_OK && hipDeviceSynchronize() != hipSuccess) {
      set_error("frontend_set_precision: packing the weights failed: %s", hipGetErrorString(hipGetLastError()));
      rc = WETTS_E_HIP;
    }
    if (rc != WETTS_OK) {
      (void)hipFree(buf);
      return rc;
    }
  } else {
    WETTS_HIP_CHECK(hipDeviceSynchronize());  // no launch in flight reads the copies that are about to go
  }
  // every check has passed: only now does the handle change
  if (h->w16) (void)hipFree(h->w16);  // (hipFree drains the device)
  h->w16 = buf;
  unsigned short* p = buf;
  for (FeBlock& k : h->blocks) {
    if (buf) {
      k.wqkv16 = p; p += 3 * d * d;
      k.wo16 = p; p += d * d;
      k.w116 = p; p += d * k.ff;
      k.w216 = p; p += d * k.ff;
    } else {
      k.wqkv16 = k.wo16 = k.w116 = k.w216 = nullptr;
    }
  }
  h->precision = precision;
  return WETTS_OK;
}

int32_t wetts_frontend_get_precision(const wetts_frontend_t* h) {
  if (!h) {
    set_error("frontend_get_precision: null handle");
    return -1;
  }
  return h->precision;
}

int32_t wetts_frontend_linear16_form(int32_t N, int32_t M) {
  if (N < 1 || M < 4 || M % 4) {
    set_error("frontend_linear16_form: N=%d must be positive and M=%d a positive multiple of 4", N, M);
    return -1;
  }
  return fe16_form(N, M);
}

int64_t wetts_frontend_linear16_workspace_bytes(int32_t K, int32_t M) {
  if (K < 8 || K % 8 || M < 4 || M % 4) {
    set_error("frontend_linear16_workspace_bytes: K=%d must be a multiple of 8, M=%d of 4", K, M);
    return -1;
  }
  return (int64_t)K * M * (int64_t)sizeof(unsigned short);
}

int32_t wetts_frontend_linear16(const float* x, const float* weight, const float* bias, const float* residual, int32_t N,
                                int32_t K, int32_t M, int32_t epilogue, int32_t precision, int32_t form, float* out,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  const bool packed = form >= 0 && (form & WETTS_FRONTEND_LINEAR16_BENCH_PACKED) != 0;
  if (packed) form &= ~WETTS_FRONTEND_LINEAR16_BENCH_PACKED;
  const char* e = fe16_linear_error(x, weight, bias, residual, out, N, K, M, epilogue, precision, form);
  WETTS_REQUIRE(e == nullptr, "frontend_linear16 (N=%d K=%d M=%d epilogue=%d precision=%d form=%d): %s", N, K, M, epilogue,
                precision, form, e);
  const int64_t need = (int64_t)K * M * (int64_t)sizeof(unsigned short);
  WETTS_REQUIRE(workspace != nullptr && workspace_bytes >= need, "frontend_linear16: the workspace has %lld bytes, %lld are needed",
                (long long)(workspace ? workspace_bytes : 0), (long long)need);
  WETTS_REQUIRE(((uintptr_t)workspace & 15) == 0, "frontend_linear16: the workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (!packed) WETTS_TRY(fe16_pack(weight, (unsigned short*)workspace, (int64_t)K * M, precision, s));
  return fe_launch_linear16(x, (const unsigned short*)workspace, bias, residual, out, N, K, M, epilogue, precision, form, s);
}

}  // extern "C"
