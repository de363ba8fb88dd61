// STFT magnitude and log-mel on the f32 matrix cores (the reference's utils/mel_processing.py, inference side).
//
// spectrogram_torch (mel_processing.py:43-94) is a GEMM per utterance:  D[row][frame] = sum_k A[row][k] * X[k][frame]
// with X[k][f] = padded_audio[f * hop + left + k] (the frame matrix, never stored) and A the window-folded DFT basis:
//   row 0      : w[k] cos(0)                  (Re bin 0)
//   row 1      : w[k] cos(pi k)               (Re bin N/2: the Im rows of bins 0 and N/2 are identically zero, so
//                                               Re N/2 takes Im 0's slot and the basis has exactly N rows)
//   row 2b     : w[k] cos(2 pi b k / N)       (Re bin b, 1 <= b < N/2)
//   row 2b + 1 : -w[k] sin(2 pi b k / N)      (Im bin b)
// The cos / sin rows of a bin are neighbours, so the 32x32 MFMA output layout leaves both in accumulator registers
// r, r + 1 of ONE lane: the magnitude sqrt(re^2 + im^2 + 1e-6) is a lane-local epilogue.  k runs over the window's
// support only ([left, left + win) of the n_fft frame; torch centres a short window), padded to a multiple of 16
// with zero basis columns.
//
// A block owns a strip of `fs` frames of one utterance and 4 M tiles (128 basis rows).  It stages the samples the
// strip covers, (fs - 1) * hop + kp, into LDS once, resolving the reflect padding there: the reference's
// F.pad(reflect, p) and, for center=True, torch.stft's own reflect pad of n_fft / 2 applied after it -- two nested
// reflections, each at the utterance's OWN length.  Samples past lengths[b] are never read; frames past the
// utterance's frame count are written as zeros.  B operands are then read from LDS as sig[f * hop + k]; the LDS image
// keeps the strip in rows of `hop` samples padded to an odd stride, so the 32 frames of one ds_read_b32 hit 32 banks.
#include "kernels.h"

namespace wetts {

typedef float f32x16t __attribute__((ext_vector_type(16)));

namespace {

constexpr int kStftWaves = 4;            // M tiles per block
constexpr int kStftLdsCapFloats = 18432;  // 72 KB: two blocks per CU
constexpr int kStftKStep = 16;           // basis columns are padded to this (8 MFMA k-steps per unrolled group)

struct StftGeom {
  int n_fft, hop, win, left, kw, kp;  // kw: window support; kp: kw rounded up to kStftKStep
  int mtiles;                         // ceil(n_fft / 32)
  int fs, nt;                         // frames per block strip, 32-frame MFMA tiles per wave (1 or 2)
  int stride;                         // LDS row stride (odd)
  int lds_floats;
};

int stft_lds_floats(int fs, int hop, int kp, int stride) {
  const int64_t span = (int64_t)(fs - 1) * hop + kp;  // samples the strip covers (k < kp)
  return (int)(((span + hop - 1) / hop) * stride);
}

StftGeom stft_geom(int n_fft, int hop, int win) {
  StftGeom g;
  g.n_fft = n_fft;
  g.hop = hop;
  g.win = win;
  g.left = (n_fft - win) / 2;  // torch.stft pads a short window on both sides, left = (n_fft - win_length) // 2
  g.kw = win;
  g.kp = (int)align_up(win, kStftKStep);
  g.mtiles = cdiv(n_fft, 32);
  g.stride = hop % 2 == 0 ? hop + 1 : hop;
  // 64 frames (two tiles per wave: each A fragment feeds two MFMAs) when the strip fits, else 32, else as many frames
  // as fit (hop close to a large n_fft: the columns past `fs` of the 32-frame tile are computed and not stored)
  g.fs = 0;
  for (int fs : {64, 32}) {
    if (stft_lds_floats(fs, hop, g.kp, g.stride) <= kStftLdsCapFloats) {
      g.fs = fs;
      break;
    }
  }
  if (g.fs == 0) {
    g.fs = 31;
    while (g.fs > 1 && stft_lds_floats(g.fs, hop, g.kp, g.stride) > 2 * kStftLdsCapFloats) --g.fs;
  }
  g.nt = g.fs > 32 ? 2 : 1;
  g.lds_floats = stft_lds_floats(g.fs, hop, g.kp, g.stride);
  return g;
}

}  // namespace

// Packed basis, MFMA A-fragment order: [mtiles][kp / 2][64 lanes], lane l of k-step s holds
// A[row = mt * 32 + (l & 31)][k = 2 s + (l >> 5)] with k relative to `left`.  Built in double from the closed form
// (the periodic Hann window of torch.hann_window(win), k * b reduced mod N before the trig call), rounded once.
__global__ void stft_basis_kernel(int n_fft, int win, int left, int kp, int64_t n, float* __restrict__ basis) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int lane = (int)(idx & 63);
  const int64_t ks = (idx >> 6) % (kp / 2);
  const int mt = (int)((idx >> 6) / (kp / 2));
  const int row = mt * 32 + (lane & 31);
  const int k = (int)(2 * ks) + (lane >> 5);
  float v = 0.f;
  if (row < n_fft && k < win) {
    const double pi2 = 6.283185307179586476925286766559;
    const double w = 0.5 - 0.5 * cos(pi2 * k / win);
    const int b = row == 1 ? n_fft / 2 : row / 2;
    const double ang = pi2 * (double)((int64_t)b * (left + k) % n_fft) / n_fft;
    v = (float)((row & 1) && row != 1 ? -w * sin(ang) : w * cos(ang));
  }
  basis[idx] = v;
}

// reflect index of F.pad(mode="reflect"): x in [-pad, n + pad) with pad < n
__device__ __forceinline__ int64_t reflect_idx(int64_t x, int64_t n) {
  if (x < 0) x = -x;
  if (x >= n) x = 2 * (n - 1) - x;
  return x;
}

// frames of one utterance of `len` samples; 0 where torch would raise (the host rejects those before launching)
__device__ __forceinline__ int stft_frames(int64_t len, int n_fft, int hop, int p, int c) {
  if (len <= 0 || (p > 0 && p >= len) || (c > 0 && c >= len + 2 * p)) return 0;
  const int64_t padded = len + 2 * (int64_t)p + 2 * (int64_t)c;
  if (padded < n_fft) return 0;
  return (int)(1 + (padded - n_fft) / hop);
}

// The body of both STFT kernels: geometry, staging and the MFMA loop are one text; CPLX selects the epilogue at compile
// time (false: the magnitude, out [B][nb][T]; true: re and im planes, out [B][2][nb][T], im of bins 0 and N/2 = 0).
template <int NT, bool CPLX>
__device__ __forceinline__ void stft_body(const float* __restrict__ audio, const int64_t* __restrict__ lengths, int64_t L,
                                          int strips, int n_fft, int hop, int left, int kp, int p, int c, int fs, int stride,
                                          int mtiles, int T, const float* __restrict__ basis, float* __restrict__ out) {
  extern __shared__ float sig[];
  const int b = blockIdx.x / strips;
  const int f0 = (blockIdx.x % strips) * fs;
  const int nb = n_fft / 2 + 1;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int mt = blockIdx.y * kStftWaves + wave;
  int64_t len = lengths ? lengths[b] : L;
  if (len > L) len = L;  // never read past the row
  const int Tb = stft_frames(len, n_fft, hop, p, c);
  float* ob = out + (int64_t)b * (CPLX ? 2 : 1) * nb * T;
  const int64_t imo = (int64_t)nb * T;  // CPLX: offset of the im plane
  const int nf = min(fs, T - f0);  // frames of the strip inside the output
  if (f0 >= Tb) {  // the whole strip is padding: zeros, nothing read (uniform over the block)
    if (mt < mtiles) {
      for (int i = lane; i < 32 * nf; i += 64) {
        const int r = mt * 32 + i / nf, f = f0 + i % nf;
        if (r < n_fft) {
          const int bin = r == 1 ? n_fft / 2 : r / 2;
          if (r < 2 || (r & 1) == 0) {
            ob[(int64_t)bin * T + f] = 0.f;
            if (CPLX) ob[imo + (int64_t)bin * T + f] = 0.f;
          }
        }
      }
    }
    return;
  }
  // stage the strip: position q of the fully padded utterance (length len + 2p + 2c) -> sample index
  const int64_t n1 = len + 2 * (int64_t)p;       // after the reference's pad
  const int64_t npad = n1 + 2 * (int64_t)c;      // after torch.stft's centring pad
  const int64_t q0 = (int64_t)f0 * hop + left;
  const int rows = ((fs - 1) * hop + kp + hop - 1) / hop;
  const float* ab = audio + (int64_t)b * L;
  for (int i = tid; i < rows * hop; i += 64 * kStftWaves) {
    const int64_t q = q0 + i;
    float v = 0.f;
    if (q < npad) {
      int64_t x = q - c;
      if (c > 0) x = reflect_idx(x, n1);
      x -= p;
      if (p > 0) x = reflect_idx(x, len);
      v = ab[x];
    }
    sig[(i / hop) * stride + i % hop] = v;
  }
  __syncthreads();
  if (mt >= mtiles) return;

  f32x16t acc[NT];
  for (int t = 0; t < NT; ++t)
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // B operand of lane l: frame j = t * 32 + (l & 31) (clamped into the strip), sample k = 2 s + (l >> 5)
  int boff[NT];
  for (int t = 0; t < NT; ++t) boff[t] = min(t * 32 + (lane & 31), fs - 1) * stride;
  const float* ap = basis + (int64_t)mt * (kp / 2) * 64 + lane;
  const int half = lane >> 5;
  // frame j's sample k sits at LDS row j + k / hop, column k % hop: kofs = k + (k / hop) * (stride - hop), advanced
  // by 2 per k-step without a division
  const int pad = stride - hop;
  int kr = half, kofs = half;
  if (kr >= hop) { kr -= hop; kofs += pad; }
  for (int k0 = 0; k0 < kp; k0 += kStftKStep) {
    float a[kStftKStep / 2];
#pragma unroll
    for (int u = 0; u < kStftKStep / 2; ++u) a[u] = ap[(int64_t)(k0 / 2 + u) * 64];
#pragma unroll
    for (int u = 0; u < kStftKStep / 2; ++u) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], sig[boff[t] + kofs], acc[t], 0, 0, 0);
      kr += 2;
      kofs += 2;
      while (kr >= hop) { kr -= hop; kofs += pad; }
    }
  }
  // epilogue: lane holds rows 8 g + 4 (l >> 5) + {0..3} of column l & 31; registers (4 g + 2 h, 4 g + 2 h + 1) are the
  // (cos, sin) rows of one bin
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = t * 32 + (lane & 31);
    const int f = f0 + j;
    if (j >= nf) continue;
    const bool valid = f < Tb;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = mt * 32 + 8 * g + 4 * half + 2 * h;
        if (r >= n_fft) continue;
        const float re = acc[t][4 * g + 2 * h], im = acc[t][4 * g + 2 * h + 1];
        if (CPLX) {
          if (r == 0) {  // rows 0 and 1 are Re 0 and Re N/2
            ob[f] = valid ? re : 0.f;
            ob[imo + f] = 0.f;
            ob[(int64_t)(n_fft / 2) * T + f] = valid ? im : 0.f;
            ob[imo + (int64_t)(n_fft / 2) * T + f] = 0.f;
          } else {
            ob[(int64_t)(r / 2) * T + f] = valid ? re : 0.f;
            ob[imo + (int64_t)(r / 2) * T + f] = valid ? im : 0.f;
          }
        } else if (r == 0) {
          ob[f] = valid ? sqrtf(re * re + 1e-6f) : 0.f;
          ob[(int64_t)(n_fft / 2) * T + f] = valid ? sqrtf(im * im + 1e-6f) : 0.f;
        } else {
          ob[(int64_t)(r / 2) * T + f] = valid ? sqrtf(re * re + im * im + 1e-6f) : 0.f;
        }
      }
  }
}

template <int NT>
__global__ void __launch_bounds__(64 * kStftWaves)
stft_mag_kernel(const float* __restrict__ audio, const int64_t* __restrict__ lengths, int64_t L, int strips,
                int n_fft, int hop, int left, int kp, int p, int c, int fs, int stride, int mtiles, int T,
                const float* __restrict__ basis, float* __restrict__ out) {
  stft_body<NT, false>(audio, lengths, L, strips, n_fft, hop, left, kp, p, c, fs, stride, mtiles, T, basis, out);
}

// The complex spectrogram of DiscriminatorR (torchaudio's Spectrogram(power=None)): the same frames, re and im stored.
// Consecutive lanes hold consecutive frames, so the planes are kept frames-fastest and the stores stay coalesced; the band
// conv that reads them resolves the layout while it stages.
template <int NT>
__global__ void __launch_bounds__(64 * kStftWaves)
stft_cplx_kernel(const float* __restrict__ audio, int64_t L, int strips, int n_fft, int hop, int left, int kp, int c,
                 int fs, int stride, int mtiles, int T, const float* __restrict__ basis, float* __restrict__ out) {
  stft_body<NT, true>(audio, nullptr, L, strips, n_fft, hop, left, kp, 0, c, fs, stride, mtiles, T, basis, out);
}

// log(clamp(mel_basis @ spec, 1e-5)) (mel_processing.py:97-111); frames at or past frame_lengths[b] (if given) are
// written as zeros.  Block: 64 frames x 32 mel rows; thread (x = frame, y) computes rows y, y + 4, ..., y + 28.
constexpr int kMelF = 64, kMelM = 32, kMelK = 32;
__global__ void __launch_bounds__(256)
mel_log_kernel(const float* __restrict__ spec, const float* __restrict__ mel, const int64_t* __restrict__ frame_lengths,
               int nb, int nm, int T, float* __restrict__ out) {
  __shared__ float s_spec[kMelK][kMelF];
  __shared__ float s_mel[kMelM][kMelK + 1];
  const int b = blockIdx.z;
  const int f0 = blockIdx.x * kMelF, m0 = blockIdx.y * kMelM;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float* sb = spec + (int64_t)b * nb * T;
  float acc[kMelM / 4];
  for (int i = 0; i < kMelM / 4; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < nb; k0 += kMelK) {
    for (int i = threadIdx.x; i < kMelK * kMelF; i += 256) {
      const int kk = i / kMelF, ff = i % kMelF;
      s_spec[kk][ff] = (k0 + kk < nb && f0 + ff < T) ? sb[(int64_t)(k0 + kk) * T + f0 + ff] : 0.f;
    }
    for (int i = threadIdx.x; i < kMelM * kMelK; i += 256) {
      const int mm = i / kMelK, kk = i % kMelK;
      s_mel[mm][kk] = (m0 + mm < nm && k0 + kk < nb) ? mel[(int64_t)(m0 + mm) * nb + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < kMelK; ++kk) {
      const float s = s_spec[kk][tx];
#pragma unroll
      for (int i = 0; i < kMelM / 4; ++i) acc[i] = __builtin_fmaf(s_mel[ty + 4 * i][kk], s, acc[i]);
    }
    __syncthreads();
  }
  const int f = f0 + tx;
  if (f >= T) return;
  const bool valid = frame_lengths == nullptr || f < frame_lengths[b];
  float* ob = out + (int64_t)b * nm * T;
  for (int i = 0; i < kMelM / 4; ++i) {
    const int m = m0 + ty + 4 * i;
    if (m < nm) ob[(int64_t)m * T + f] = valid ? logf(fmaxf(acc[i], 1e-5f)) : 0.f;
  }
}

static int32_t stft_check(int n_fft, int hop, int win) {
  WETTS_REQUIRE(n_fft >= 4 && n_fft % 2 == 0, "stft: n_fft must be even and >= 4 (got %d)", n_fft);
  WETTS_REQUIRE(hop >= 1 && hop <= n_fft, "stft: hop must be in [1, n_fft] (got %d, n_fft %d)", hop, n_fft);
  WETTS_REQUIRE(win >= 1 && win <= n_fft, "stft: win must be in [1, n_fft] (got %d, n_fft %d)", win, n_fft);
  WETTS_REQUIRE(n_fft <= (1 << 16), "stft: n_fft above 65536 is not supported (got %d)", n_fft);
  const StftGeom g = stft_geom(n_fft, hop, win);
  WETTS_REQUIRE(g.lds_floats <= 2 * kStftLdsCapFloats,
                "stft: one frame of n_fft %d, hop %d does not fit the LDS strip", n_fft, hop);
  return WETTS_OK;
}

int32_t launch_stft_cplx(const float* audio, int rows, int T, int n_fft, int hop, const float* basis, int frames,
                         float* out, hipStream_t s) {
  WETTS_TRY(stft_check(n_fft, hop, n_fft));
  WETTS_REQUIRE(audio && basis && out && rows >= 1, "stft_cplx: bad argument");
  WETTS_REQUIRE(T > n_fft / 2 && frames == 1 + T / hop, "stft_cplx: T=%d does not give %d frames of n_fft %d, hop %d", T,
                frames, n_fft, hop);
  const StftGeom g = stft_geom(n_fft, hop, n_fft);
  const int strips = cdiv(frames, g.fs);
  WETTS_REQUIRE((int64_t)rows * strips < (1ll << 31), "stft_cplx: batch too large");
  const dim3 grid((unsigned)(rows * strips), (unsigned)cdiv(g.mtiles, kStftWaves));
  const size_t lds = (size_t)g.lds_floats * sizeof(float);
  if (g.nt == 2) {
    static signed char opt[64];
    if (lds > 64 * 1024) WETTS_REQUIRE(lds_opt_in((const void*)stft_cplx_kernel<2>, opt), "stft: LDS opt-in refused");
    hipLaunchKernelGGL(stft_cplx_kernel<2>, grid, dim3(64 * kStftWaves), lds, s, audio, (int64_t)T, strips, n_fft, hop,
                       g.left, g.kp, n_fft / 2, g.fs, g.stride, g.mtiles, frames, basis, out);
  } else {
    static signed char opt[64];
    if (lds > 64 * 1024) WETTS_REQUIRE(lds_opt_in((const void*)stft_cplx_kernel<1>, opt), "stft: LDS opt-in refused");
    hipLaunchKernelGGL(stft_cplx_kernel<1>, grid, dim3(64 * kStftWaves), lds, s, audio, (int64_t)T, strips, n_fft, hop,
                       g.left, g.kp, n_fft / 2, g.fs, g.stride, g.mtiles, frames, basis, out);
  }
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // namespace wetts

using namespace wetts;

extern "C" {

int64_t wetts_stft_basis_numel(int32_t n_fft, int32_t win) {
  if (stft_check(n_fft, 1, win) != WETTS_OK) return -1;
  const StftGeom g = stft_geom(n_fft, 1, win);
  return (int64_t)g.mtiles * 32 * g.kp;
}

int32_t wetts_stft_basis(int32_t n_fft, int32_t win, float* basis, int64_t numel, void* stream) {
  WETTS_TRY(stft_check(n_fft, 1, win));
  WETTS_REQUIRE(basis, "null argument");
  const StftGeom g = stft_geom(n_fft, 1, win);
  const int64_t n = (int64_t)g.mtiles * 32 * g.kp;
  WETTS_REQUIRE(numel >= n, "stft_basis: buffer has %lld floats, needs %lld", (long long)numel, (long long)n);
  hipLaunchKernelGGL(stft_basis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_fft,
                     win, g.left, g.kp, n, basis);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t wetts_spectrogram(const float* audio, const int64_t* lengths, int32_t B, int64_t L, int32_t n_fft,
                          int32_t hop, int32_t win, int32_t center, const float* basis, int32_t T, float* spec,
                          void* stream) {
  WETTS_TRY(stft_check(n_fft, hop, win));
  WETTS_REQUIRE(audio && basis && spec, "null argument");
  WETTS_REQUIRE(B >= 0 && L >= 0 && T >= 0, "spectrogram: negative size");
  if (B == 0 || T == 0) return WETTS_OK;
  const StftGeom g = stft_geom(n_fft, hop, win);
  const int p = (n_fft - hop) / 2;  // int((n_fft - hop_size) / 2), mel_processing.py:65
  const int c = center ? n_fft / 2 : 0;
  const int strips = cdiv(T, g.fs);
  WETTS_REQUIRE((int64_t)B * strips < (1ll << 31), "spectrogram: batch too large");
  const dim3 grid((unsigned)(B * strips), (unsigned)cdiv(g.mtiles, kStftWaves));
  const size_t lds = (size_t)g.lds_floats * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (g.nt == 2) {
    static signed char opt[64];
    if (lds > 64 * 1024) WETTS_REQUIRE(lds_opt_in((const void*)stft_mag_kernel<2>, opt), "stft: LDS opt-in refused");
    hipLaunchKernelGGL(stft_mag_kernel<2>, grid, dim3(64 * kStftWaves), lds, s, audio, lengths, L, strips, n_fft, hop,
                       g.left, g.kp, p, c, g.fs, g.stride, g.mtiles, T, basis, spec);
  } else {
    static signed char opt[64];
    if (lds > 64 * 1024) WETTS_REQUIRE(lds_opt_in((const void*)stft_mag_kernel<1>, opt), "stft: LDS opt-in refused");
    hipLaunchKernelGGL(stft_mag_kernel<1>, grid, dim3(64 * kStftWaves), lds, s, audio, lengths, L, strips, n_fft, hop,
                       g.left, g.kp, p, c, g.fs, g.stride, g.mtiles, T, basis, spec);
  }
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

int32_t wetts_spec_to_mel(const float* spec, const float* mel_basis, const int64_t* frame_lengths, int32_t B,
                          int32_t n_bins, int32_t n_mels, int32_t T, float* mel, void* stream) {
  WETTS_REQUIRE(spec && mel_basis && mel, "null argument");
  WETTS_REQUIRE(B >= 0 && T >= 0 && n_bins >= 1 && n_mels >= 1, "spec_to_mel: bad size (B %d, bins %d, mels %d, T %d)",
                B, n_bins, n_mels, T);
  if (B == 0 || T == 0) return WETTS_OK;
  const dim3 grid((unsigned)cdiv(T, kMelF), (unsigned)cdiv(n_mels, kMelM), (unsigned)B);
  hipLaunchKernelGGL(mel_log_kernel, grid, dim3(256), 0, (hipStream_t)stream, spec, mel_basis, frame_lengths, n_bins,
                     n_mels, T, mel);
  WETTS_LAUNCH_CHECK();
  return WETTS_OK;
}

}  // extern "C"
