// Stand-alone entries of the 16-bit conv launches (include/wetts_hip.h, "The 16-bit conv launches, one at a time"):
// caller data in, one launch (or the conv-by-conv form of one fused launch) through the launchers the decoder and the
// 16-bit WaveNet use, caller data out.  No kernels here and no launch code of its own: the parameter blocks are filled as
// model.hip's run_hifigan_bf16 / run_wn fill them.  tests/test_gpu_conv16.py holds every launch to float64 through these.
#include <string.h>

#include "common.h"
#include "conv_bf16.h"

namespace wetts {
namespace {

// what an entry packed / allocated, released on every way out
struct Packed16 {
  PackedConvB pc[2 * RESSTAGE2_MAX_CHAINS];
  float* wpad = nullptr;
  ~Packed16() {
    for (auto& p : pc) free_packed_bf16(&p);
    if (wpad) (void)hipFree(wpad);
  }
};

ConvBParams io16(const void* x, int Cin, int Tin, void* out, int Cout, int Tout, int B) {
  ConvBParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const unsigned short*)x;
  p.x_bs = (int64_t)Cin * Tin;
  p.Cin = Cin;
  p.Tin = Tin;
  p.in_act = IN_NONE;
  p.out = (unsigned short*)out;
  p.o_bs = (int64_t)Cout * Tout;
  p.cout = Cout;
  p.Tout = Tout;
  p.out_div = 1.f;
  p.B = B;
  return p;
}

int32_t finish(int32_t rc, hipStream_t s, const char* what) {
  // (also after a refused launch: the packing kernels may still be running on the buffers about to be freed)
  if (hipStreamSynchronize(s) != hipSuccess && rc == WETTS_OK) {
    set_error("%s: kernel failed", what);
    rc = WETTS_E_HIP;
  }
  return rc;
}

// one residual conv of the decoder's ResBlocks as run_hifigan_bf16's conv-by-conv branch launches it
int32_t rb_conv(const PackedConvB& pc, const void* x, void* out, const void* res, int C, int T, int B, int accum,
                float out_div, hipStream_t s) {
  ConvBParams p = io16(x, C, T, out, C, T, B);
  p.in_act = IN_LRELU;
  p.in_slope = 0.1f;
  p.basic = 1;
  p.tag = 1;
  p.res = (const unsigned short*)res;
  p.r_bs = (int64_t)C * T;
  p.accum = accum;
  p.out_div = out_div;
  return launch_conv_bf16(pc, p, s);
}

int32_t resblock16_run(Packed16& pk, int form, int fused, int nchain, const float* const* w1, const float* const* b1,
                       const float* const* w2, const float* const* b2, const int32_t* ktaps, const int32_t* dil1,
                       const int32_t* dil2, const void* x, void* out, void* mid, int B, int C, int T, int accum,
                       float out_div, int f16, hipStream_t s) {
  for (int j = 0; j < nchain; ++j) {
    const int k = ktaps[j], d1 = dil1[j], d2 = form == 0 ? 1 : dil2[j];
    WETTS_TRY(pack_conv_weight_bf16(w1[j], b1[j], C, C, k, d1, (k - 1) / 2 * d1, 0, 0, f16, s, &pk.pc[2 * j]));
    WETTS_TRY(pack_conv_weight_bf16(w2[j], b2[j], C, C, k, d2, (k - 1) / 2 * d2, 0, 0, f16, s, &pk.pc[2 * j + 1]));
  }
  if (fused) {
    if (form == 2) {
      const PackedConvB *c1s[RESSTAGE2_MAX_CHAINS], *c2s[RESSTAGE2_MAX_CHAINS];
      for (int j = 0; j < nchain; ++j) {
        c1s[j] = &pk.pc[2 * j];
        c2s[j] = &pk.pc[2 * j + 1];
      }
      ResStage2Params sp;
      memset(&sp, 0, sizeof(sp));
      sp.x = (const unsigned short*)x;
      sp.out = (unsigned short*)out;
      sp.T = T;
      sp.B = B;
      sp.out_div = out_div;
      sp.slope = 0.1f;
      return launch_resblock2_stage16(c1s, c2s, nchain, sp, s);
    }
    ResPairParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.x = (const unsigned short*)x;
    pp.out = (unsigned short*)out;
    pp.T = T;
    pp.B = B;
    pp.accum = accum;
    pp.out_div = out_div;
    pp.slope = 0.1f;
    if (form == 0) return launch_resblock_pair16(pk.pc[0], pk.pc[1], pp, s);
    return launch_resblock2_chain16(pk.pc[0], pk.pc[1], pp, s);
  }
  unsigned short* m16 = (unsigned short*)mid;
  const int64_t plane = (int64_t)B * T * C;
  for (int j = 0; j < nchain; ++j) {
    unsigned short* mj = m16 + j * plane;
    const int acc = (accum || j > 0) ? 1 : 0;
    const float dv = j == nchain - 1 ? out_div : 1.f;
    if (form == 0) {  // ft = c1(lrelu(x));  out = (x + c2(lrelu(ft)) [+ out]) / div
      WETTS_TRY(rb_conv(pk.pc[0], x, mj, nullptr, C, T, B, 0, 1.f, s));
      WETTS_TRY(rb_conv(pk.pc[1], mj, out, x, C, T, B, acc, dv, s));
    } else {  // t = x + c1(lrelu(x));  out = (t + c2(lrelu(t)) [+ out]) / div
      WETTS_TRY(rb_conv(pk.pc[2 * j], x, mj, x, C, T, B, 0, 1.f, s));
      WETTS_TRY(rb_conv(pk.pc[2 * j + 1], mj, out, mj, C, T, B, acc, dv, s));
    }
  }
  return WETTS_OK;
}

}  // namespace
}  // namespace wetts

using namespace wetts;

int32_t wetts_conv16(const float* w, const float* bias, const float* bias_b, const void* x, const void* res, void* out,
                     int32_t B, int32_t Cin, int32_t Cout, int32_t k, int32_t dilation, int32_t padding, int32_t up,
                     int32_t Tin, int32_t Tout, int32_t flags, float in_slope, float out_div, void* stream) {
  WETTS_REQUIRE(w && x && out && B > 0 && Cin > 0 && Cout > 0 && k > 0 && Tin > 0 && dilation > 0 && padding >= 0,
                "conv16: bad argument");
  WETTS_REQUIRE(out_div != 0.f && (flags & ~63) == 0, "conv16: bad argument");
  const int tr = (flags & WETTS_CONV16_TRANSPOSED) ? 1 : 0, f16 = (flags & WETTS_CONV16_F16) ? 1 : 0;
  const int accum = (flags & WETTS_CONV16_ACCUM) ? 1 : 0;
  if (tr) {
    WETTS_REQUIRE(up > 0 && dilation == 1, "conv16: a transposed conv needs a rate and dilation 1");
    WETTS_REQUIRE(!res && !accum && out_div == 1.f, "conv16: a transposed conv has no residual, running sum or divisor");
    WETTS_REQUIRE((int64_t)Tout == ((int64_t)Tin - 1) * up - 2 * (int64_t)padding + k && Tout > 0,
                  "conv16: Tout must be (Tin - 1) * up - 2 * padding + k");
  } else {
    WETTS_REQUIRE((int64_t)Tout == (int64_t)Tin + 2 * (int64_t)padding - (int64_t)(k - 1) * dilation && Tout > 0,
                  "conv16: Tout must be Tin + 2 * padding - (k - 1) * dilation");
  }
  hipStream_t s = (hipStream_t)stream;
  Packed16 pk;
  int32_t rc = pack_conv_weight_bf16(w, bias, Cout, Cin, k, dilation, padding, tr, tr ? up : 0, f16, s, &pk.pc[0]);
  if (rc == WETTS_OK) {
    ConvBParams p = io16(x, Cin, Tin, out, Cout, Tout, B);
    if (flags & WETTS_CONV16_LRELU) {
      p.in_act = IN_LRELU;
      p.in_slope = in_slope;
    }
    if (bias_b) {
      p.bias_b = bias_b;
      p.bias_b_stride = Cout;
    }
    p.res = (const unsigned short*)res;
    p.r_bs = (int64_t)Cout * Tout;
    p.accum = accum;
    p.out_div = out_div;
    p.basic = (flags & WETTS_CONV16_BASIC) ? 1 : 0;
    p.tag = (flags & WETTS_CONV16_TAG) ? 1 : 0;
    rc = launch_conv_bf16(pk.pc[0], p, s);
  }
  return finish(rc, s, "conv16");
}

int32_t wetts_conv16_wn_gate(const float* w, const float* bias, const float* bias_b, int64_t bias_b_stride, const void* x,
                             void* acts, int32_t B, int32_t H, int32_t k, int32_t dilation, int32_t T, int32_t f16,
                             void* stream) {
  WETTS_REQUIRE(w && x && acts && B > 0 && T > 0 && k > 0 && (k & 1) && dilation > 0, "conv16_wn_gate: bad argument");
  WETTS_REQUIRE(H >= 128 && H % 16 == 0, "conv16_wn_gate: the gate epilogue needs H >= 128, H %% 16 == 0");
  WETTS_REQUIRE(!bias_b || bias_b_stride >= 2 * (int64_t)H, "conv16_wn_gate: bias_b rows are at least 2H apart");
  hipStream_t s = (hipStream_t)stream;
  Packed16 pk;
  int32_t rc = pack_conv_weight_bf16(w, bias, 2 * H, H, k, dilation, (k - 1) / 2 * dilation, 0, 0, f16 ? 1 : 0, s,
                                     &pk.pc[0], H);
  if (rc == WETTS_OK) {
    ConvBParams p = io16(x, H, T, acts, H, T, B);
    p.bias_b = bias_b;
    p.bias_b_stride = bias_b_stride;
    p.epi_mode = 1;
    p.wn_H = H;
    rc = launch_conv_bf16(pk.pc[0], p, s);
  }
  return finish(rc, s, "conv16_wn_gate");
}

int32_t wetts_conv16_wn_update(const float* w, const float* bias, const void* acts, void* h, float* skip,
                               const float* mask, int32_t B, int32_t H, int32_t T, int32_t last, int32_t first,
                               int32_t f16, void* stream) {
  WETTS_REQUIRE(w && acts && h && skip && mask && B > 0 && T > 0, "conv16_wn_update: bad argument");
  WETTS_REQUIRE(H >= 128 && H % 16 == 0, "conv16_wn_update: the update epilogue needs H >= 128, H %% 16 == 0");
  hipStream_t s = (hipStream_t)stream;
  const int RC = last ? H : 2 * H;
  Packed16 pk;
  int32_t rc = pack_conv_weight_bf16(w, bias, RC, H, 1, 1, 0, 0, 0, f16 ? 1 : 0, s, &pk.pc[0]);
  if (rc == WETTS_OK) {
    ConvBParams p = io16(acts, H, T, nullptr, RC, T, B);
    p.epi_mode = 2;
    p.wn_H = H;
    p.wn_h = (unsigned short*)h;
    p.wn_skip = skip;
    p.wn_mask = mask;
    p.wn_last = last ? 1 : 0;
    p.wn_first = first ? 1 : 0;
    rc = launch_conv_bf16(pk.pc[0], p, s);
  }
  return finish(rc, s, "conv16_wn_update");
}

int32_t wetts_wn16_gate(const void* xin, void* acts, int64_t rows, int32_t H, int32_t f16, void* stream) {
  WETTS_REQUIRE(xin && acts && rows > 0 && H > 0, "wn16_gate: bad argument");
  hipStream_t s = (hipStream_t)stream;
  return finish(k_gate_cl16((const unsigned short*)xin, (unsigned short*)acts, rows, H, f16 ? 1 : 0, s), s, "wn16_gate");
}

int32_t wetts_wn16_update(const void* rs, void* h, float* skip, const float* mask, int32_t last, int32_t first,
                          int64_t rows, int32_t H, int32_t f16, void* stream) {
  WETTS_REQUIRE(rs && h && skip && mask && rows > 0 && H > 0, "wn16_update: bad argument");
  hipStream_t s = (hipStream_t)stream;
  return finish(k_wn_update_cl16((const unsigned short*)rs, (unsigned short*)h, skip, mask, last ? 1 : 0, first ? 1 : 0,
                                 rows, H, f16 ? 1 : 0, s),
                s, "wn16_update");
}

int32_t wetts_conv16_post(const float* w, const void* x, float* out, int32_t B, int32_t C, int32_t T, int32_t mfma,
                          int32_t f16, void* stream) {
  WETTS_REQUIRE(w && x && out && B > 0 && C > 0 && T > 0, "conv16_post: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (!mfma)
    return finish(k_conv_post_bf16((const unsigned short*)x, w, 7, B, C, T, out, f16 ? 1 : 0, s), s, "conv16_post");
  WETTS_REQUIRE(C == 32, "conv16_post: the matrix-core form is the C = 32 one");
  Packed16 pk;
  // rows 1..31 of the packed weight are zero (pack_decoder_bf16_layers)
  const size_t n = (size_t)32 * C * 7;
  WETTS_HIP_CHECK(hipMalloc((void**)&pk.wpad, n * sizeof(float)));
  int32_t rc = WETTS_OK;
  if (hipMemsetAsync(pk.wpad, 0, n * sizeof(float), s) != hipSuccess ||
      hipMemcpyAsync(pk.wpad, w, (size_t)C * 7 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    set_error("conv16_post: padding the weight failed");
    rc = WETTS_E_HIP;
  }
  if (rc == WETTS_OK) rc = pack_conv_weight_bf16(pk.wpad, nullptr, 32, C, 7, 1, 3, 0, 0, f16 ? 1 : 0, s, &pk.pc[0]);
  if (rc == WETTS_OK) rc = k_conv_post_mfma16(pk.pc[0], (const unsigned short*)x, B, C, T, out, s);
  return finish(rc, s, "conv16_post");
}

int32_t wetts_resblock16(int32_t form, int32_t fused, int32_t nchain, const float* const* w1, const float* const* b1,
                         const float* const* w2, const float* const* b2, const int32_t* ktaps, const int32_t* dil1,
                         const int32_t* dil2, const void* x, void* out, void* mid, int32_t B, int32_t C, int32_t T,
                         int32_t accum, float out_div, int32_t f16, void* stream) {
  WETTS_REQUIRE(form >= 0 && form <= 2 && w1 && b1 && w2 && b2 && ktaps && dil1 && x && out && x != out,
                "resblock16: bad argument");
  WETTS_REQUIRE(B > 0 && C > 0 && T > 0 && out_div != 0.f, "resblock16: bad argument");
  WETTS_REQUIRE(form == 2 ? (nchain >= 1 && nchain <= RESSTAGE2_MAX_CHAINS && !accum) : nchain == 1,
                "resblock16: a pair / chain is one chain, a stage 1..3 chains without a running sum");
  WETTS_REQUIRE(form == 0 || dil2, "resblock16: a ResBlock2 needs c2's dilations");
  WETTS_REQUIRE(fused || mid, "resblock16: the conv-by-conv form needs `mid`");
  for (int j = 0; j < nchain; ++j) {
    WETTS_REQUIRE(w1[j] && w2[j] && b1[j] && b2[j] && ktaps[j] > 0 && (ktaps[j] & 1) && dil1[j] > 0 && (form == 0 || dil2[j] > 0),
                  "resblock16: bad chain %d", j);
  }
  hipStream_t s = (hipStream_t)stream;
  Packed16 pk;
  const int32_t rc = resblock16_run(pk, form, fused, nchain, w1, b1, w2, b2, ktaps, dil1, dil2, x, out, mid, B, C, T,
                                    accum ? 1 : 0, out_div, f16 ? 1 : 0, s);
  return finish(rc, s, "resblock16");
}
