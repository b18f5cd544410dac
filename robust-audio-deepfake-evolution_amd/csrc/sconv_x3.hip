// Split-precision ("x3") SincNet stream of the fp32 scoring pass: the residual 2-D encoder of SincNetEncoder
// (src/models/DualStreamSEMamba.py:144-270) in eval mode with frozen BatchNorm, at fp32 accuracy on gfx950's bf16
// matrix cores. As in csrc/x3.hip an fp32 value is carried as two bf16 planes, hi = bf16(x) and lo = bf16(x - hi),
// and a convolution sums three MFMA products x_hi.w_hi + x_lo.w_hi + x_hi.w_lo with fp32 accumulation (the
// convention of rdx_hgemm_x3 and rdx_x3_posconv_fwd). The activations stay fp32 in memory (NHWC) and are split while
// they are staged in LDS; the weights come as planes, tap-major [kh * 3 + kw][co][ci].
//   rdx_x3_b0x_fwd    block 0 (one input channel) in one pass, the structure of csrc/b0fused.hip b0x_fwd_kernel:
//                     [first_bn + SELU of the raw input ->] conv1 + BN + SELU and conv_downsample in fp32 on the
//                     VALU (K = 6 and 3), each out1 row split into the LDS ring, conv2 as three MFMA products, the
//                     sum and the (1, 3) max pool in fp32
//   rdx_x3_sconv_fwd  blocks 1-5: a (1|2) x 3 convolution over 32 / 64 channels, plain or with conv1's
//                     selu(bn(acc + bias)) epilogue
// The fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 rate, i.e. 16 / 3 times slower than the three
// products per K element, and was not taken. libradhip.so only: libradhip_f16.so exports the names and returns
// RDX_EINVAL.
#include "common.h"

namespace rdx {
namespace sx3 {

#ifndef RDX_F16
constexpr float SELU_ALPHA = 1.6732632423543772848170429916717f;
constexpr float SELU_SCALE = 1.0507009873554804934193349852946f;

__device__ __forceinline__ float selu(float u) { return SELU_SCALE * (u > 0.f ? u : SELU_ALPHA * (__expf(u) - 1.0f)); }

// hi / lo bf16 bits of two floats, packed
__device__ __forceinline__ void split_pack2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = hpack2(a, b);
  lo = hpack2(a - hlo(hi), b - hhi(hi));
}

// ---- blocks 1-5: (1|2) x 3 convolution, split on staging ------------------------------------------------------------
// y[n, ho, w, co] = sum_{kr < KH, kw < 3, ci} x[n, ho - ph + kr, w + kw - 1, ci] W[kr * 3 + kw][co][ci] (zero outside
// the image). Block = 4 waves = 128 positions of one output row; its KH input rows (130 positions each) are staged as
// hi / lo bf16 images; each wave 32 positions x CO outputs as CO / 32 32x32x16 accumulators; per tap and 16-channel
// step three MFMAs against the tap's weight planes from L2.
constexpr int SX_ROWS = 128, SX_WIN = SX_ROWS + 2;

struct ConvArgs {
  const float* x;    // [N, H, W, CI]
  const hst* wh;     // [KH * 3][CO][CI] planes
  const hst* wl;
  const float* bn;   // [4][CO] (conv bias, running mean, invstd * gamma, beta) or null: plain output
  float* y;          // [N, Ho, W, CO]
  int H, W, Ho, ph;
};

template <int CI, int CO, int KH>
__global__ __launch_bounds__(256, 2) void conv_kernel(ConvArgs a) {
  constexpr int LDW = CI + 8, C4 = CI / 4, NT = CO / 32, KS = CI / 16;
  __shared__ __attribute__((aligned(16))) hel sh[KH][SX_WIN][LDW];
  __shared__ __attribute__((aligned(16))) hel sl[KH][SX_WIN][LDW];
  const int w0 = blockIdx.x * SX_ROWS, ho = blockIdx.y, n = blockIdx.z;
  const int H = a.H, W = a.W;
  for (int i = threadIdx.x; i < KH * SX_WIN * C4; i += 256) {
    const int kr = i / (SX_WIN * C4), rem = i - kr * (SX_WIN * C4);
    const int wr = rem / C4, c4 = (rem - wr * C4) * 4;
    const int hr = ho - a.ph + kr, tr = w0 - 1 + wr;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (hr >= 0 && hr < H && tr >= 0 && tr < W)
      v = *reinterpret_cast<const float4*>(a.x + (((int64_t)n * H + hr) * W + tr) * CI + c4);
    uint32_t h0, l0, h1, l1;
    split_pack2(v.x, v.y, h0, l0);
    split_pack2(v.z, v.w, h1, l1);
    *reinterpret_cast<uint2*>(&sh[kr][wr][c4]) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(&sl[kr][wr][c4]) = make_uint2(l0, l1);
  }
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
  if (w0 + 32 * w >= W) return;                  // no barrier follows
  rdx_f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nt][i] = 0.f;
#pragma unroll
  for (int t = 0; t < KH * 3; ++t) {
    const int kr = t / 3, kw = t - 3 * kr;
    hx8 bh[NT][KS], bl[NT][KS];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int64_t o = ((int64_t)t * CO + nt * 32 + r) * CI + 16 * s + 8 * hh;
        bh[nt][s] = *reinterpret_cast<const hx8*>(a.wh + o);
        bl[nt][s] = *reinterpret_cast<const hx8*>(a.wl + o);
      }
    const hel* ah = &sh[kr][32 * w + r + kw][8 * hh];
    const hel* al = &sl[kr][32 * w + r + kw][8 * hh];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const hx8 fh = *reinterpret_cast<const hx8*>(ah + 16 * s);
      const hx8 fl = *reinterpret_cast<const hx8*>(al + 16 * s);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma32x32x16(fh, bh[nt][s], acc[nt]);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma32x32x16(fl, bh[nt][s], acc[nt]);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma32x32x16(fh, bl[nt][s], acc[nt]);
    }
  }
  // C layout: column co = nt * 32 + (lane & 31), row (position) (i & 3) + 8 (i >> 2) + 4 hh
  float* yr = a.y + ((int64_t)n * a.Ho + ho) * W * CO;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = nt * 32 + r;
    float cb = 0.f, mu = 0.f, sg = 1.f, sf = 0.f;
    if (a.bn) cb = a.bn[co], mu = a.bn[CO + co], sg = a.bn[2 * CO + co], sf = a.bn[3 * CO + co];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = w0 + 32 * w + (i & 3) + 8 * (i >> 2) + 4 * hh;
      if (p < W) {
        float v = acc[nt][i];
        if (a.bn) v = selu(fmaf((v + cb) - mu, sg, sf));
        yr[(int64_t)p * CO + co] = v;
      }
    }
  }
}

// ---- block 0 in one pass ----------------------------------------------------------------------------------------------
// A 256-thread workgroup owns a strip of 42 pooled outputs (126 positions) of one utterance and walks its rows
// top-down, as b0x_fwd_kernel does. Per output row h: conv1 + BN + SELU of out1 row h + 2 in fp32 into a 3-slot LDS
// ring of hi / lo images, conv2 from out1 rows h, h + 1 (6 taps x 2 K steps x 3 products, the weight planes in
// registers), s = a + idn + bias in fp32 staged in LDS, then the (1, 3) max pool with torch's rule.
constexpr int BX_T = 256;
constexpr int BX_C = 32;
constexpr int BX_J = 42;        // pooled outputs per strip
constexpr int BX_P = 3 * BX_J;  // 126 positions per strip
constexpr int BX_IR = 136;      // out1 image rows: positions q0 - 1 .. q0 + 128 (130 used)
constexpr int BX_XW = 132;      // staged x positions q0 - 2 .. q0 + 129
constexpr int BX_SP = 36;       // fp32 pitch of the pre-pool row
constexpr int BX_IMG = BX_IR * 64;
constexpr int BX_LDS = 6 * BX_IMG + 4 * BX_XW * 4 + 128 * BX_SP * 4 + 32 * 16;
static_assert(2 * BX_LDS <= 160 * 1024, "two workgroups per CU");

// [row][32] bf16 image: 8-row x 32-channel subtiles of 512 B, the 16-byte chunk XOR-swizzled by (row >> 2) & 3
__device__ __forceinline__ int bx_img(int row, int ch) {
  return 512 * (row >> 3) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

struct B0Args {
  const float* x;     // [N, H, W]
  const float* fbn;   // (scale, shift) of first_bn, or null: x is already activated
  const float* w1;    // [32][6]
  const float* wd;    // [32][3]
  const float* bn;    // [4][32]
  const hst* w2h;     // [6][32 co][32 ci] planes
  const hst* w2l;
  const float* bias;  // [32]
  float* y;           // [N, H, Wo, 32]
  int N, H, W, Wo, rows_per;
};

__global__ __launch_bounds__(BX_T, 2) void b0x_kernel(B0Args a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* osh = lds;                                           // out1 ring, hi planes: 3 slots
  char* osl = lds + 3 * BX_IMG;                              // lo planes
  float* xr = reinterpret_cast<float*>(lds + 6 * BX_IMG);    // x ring: 4 rows of BX_XW
  float* ss = xr + 4 * BX_XW;                                // s = a + idn + bias of the current row
  float4* prec = reinterpret_cast<float4*>(ss + 128 * BX_SP);   // [32] {wd[co][0..2], bias[co]}
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int strip = blockIdx.x, n = blockIdx.y;
  const int q0 = strip * BX_P;
  const int H = a.H, W = a.W;
  const int h0 = blockIdx.z * a.rows_per, h1 = min(H, h0 + a.rows_per);
  if (h0 >= h1) return;
  // conv2's A operand (the weight planes, rows co = lane & 31) for all 6 taps x 2 K steps, in registers for the walk
  hx8 wh[6][2], wl[6][2];
#pragma unroll
  for (int t = 0; t < 6; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int o = (t * BX_C + r) * BX_C + (2 * s + hh) * 8;
      wh[t][s] = *reinterpret_cast<const hx8*>(a.w2h + o);
      wl[t][s] = *reinterpret_cast<const hx8*>(a.w2l + o);
    }
  if (tid < 32) prec[tid] = make_float4(a.wd[tid * 3], a.wd[tid * 3 + 1], a.wd[tid * 3 + 2], a.bias[tid]);
  const bool act = a.fbn != nullptr;
  const float fs = act ? a.fbn[0] : 1.f, ft = act ? a.fbn[1] : 0.f;
  // this thread's out1 channels: 8 * g8 .. + 7 (its items it = tid + 256 k all have it & 3 == tid & 3)
  const int g8 = tid & 3;
  float t1[8][6], cb[8], mu[8], sg[8], sf[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int co = g8 * 8 + k;
#pragma unroll
    for (int j = 0; j < 6; ++j) t1[k][j] = a.w1[co * 6 + j];
    cb[k] = a.bn[co];
    mu[k] = a.bn[BX_C + co];
    sg[k] = a.bn[2 * BX_C + co];
    sf[k] = a.bn[3 * BX_C + co];
  }
  const float* xn = a.x + (int64_t)n * H * W;
  // x[row][q0 - 2 + tid] from a clamped (always valid) address: no branch around the load
  auto x_raw = [&](int row) -> float {
    const int q = q0 - 2 + tid;
    const int rc = row < 0 ? 0 : (row >= H ? H - 1 : row);
    const int qc = q < 0 ? 0 : (q >= W ? W - 1 : q);
    return xn[(int64_t)rc * W + qc];
  };
  auto x_val = [&](int row, float raw) -> float {   // activated, zero outside the image
    const int q = q0 - 2 + tid;
    const float v = act ? selu(fmaf(raw, fs, ft)) : raw;
    return (row >= 0 && row < H && q >= 0 && q < W) ? v : 0.f;
  };
  auto xslot = [&](int row) -> float* { return xr + (row & 3) * BX_XW; };
  auto oslot = [&](int row) -> int { return ((row + 3) % 3) * BX_IMG; };
  // out1 row ro (0 .. H) at positions q0 - 1 + pp, pp < 130 (zero outside [0, W): conv2's padding);
  // one item = (position pp, this thread's 8 channels)
  auto out1_item = [&](const float (&v0)[3], const float (&v1)[3], int pp, int sl) {
    const int q = q0 - 1 + pp;
    const bool inside = q >= 0 && q < W;
    uint32_t oh[4], ol[4];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      float yv[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        float acc = v0[0] * t1[k + e][0];
        acc = fmaf(v0[1], t1[k + e][1], acc);
        acc = fmaf(v0[2], t1[k + e][2], acc);
        acc = fmaf(v1[0], t1[k + e][3], acc);
        acc = fmaf(v1[1], t1[k + e][4], acc);
        acc = fmaf(v1[2], t1[k + e][5], acc);
        const float u = selu(fmaf((acc + cb[k + e]) - mu[k + e], sg[k + e], sf[k + e]));
        yv[e] = inside ? u : 0.f;
      }
      split_pack2(yv[0], yv[1], oh[k >> 1], ol[k >> 1]);
    }
    const int o = sl + bx_img(pp, g8);
    *reinterpret_cast<uint4*>(osh + o) = make_uint4(oh[0], oh[1], oh[2], oh[3]);
    *reinterpret_cast<uint4*>(osl + o) = make_uint4(ol[0], ol[1], ol[2], ol[3]);
  };
  auto make_out1 = [&](int ro) {
    const float* xa = xslot(ro - 1);
    const float* xb = xslot(ro);
    const int sl = oslot(ro);
    static_assert(2 * BX_T <= 130 * 4 && 3 * BX_T >= 130 * 4, "2 or 3 items per thread");
    const int pa = tid >> 2, pb = (tid + BX_T) >> 2, pc = (tid + 2 * BX_T) >> 2;
    const bool has_c = tid + 2 * BX_T < 130 * 4;
    const int pcc = has_c ? pc : 0;
    const float a0[3] = {xa[pa], xa[pa + 1], xa[pa + 2]}, a1[3] = {xb[pa], xb[pa + 1], xb[pa + 2]};
    const float b0[3] = {xa[pb], xa[pb + 1], xa[pb + 2]}, b1[3] = {xb[pb], xb[pb + 1], xb[pb + 2]};
    const float c0[3] = {xa[pcc], xa[pcc + 1], xa[pcc + 2]}, c1[3] = {xb[pcc], xb[pcc + 1], xb[pcc + 2]};
    out1_item(a0, a1, pa, sl);
    out1_item(b0, b1, pb, sl);
    if (has_c) out1_item(c0, c1, pc, sl);
  };
  const int pw = wv * 32 + r;   // this lane's output position q0 + pw (B operand row of the MFMA)

  {  // prologue: x rows h0 - 1 .. h0 + 2, out1 rows h0 and h0 + 1
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = x_raw(h0 - 1 + i);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (tid < BX_XW) xslot(h0 - 1 + i)[tid] = x_val(h0 - 1 + i, v[i]);
  }
  __syncthreads();
  make_out1(h0);
  make_out1(h0 + 1);
  __syncthreads();
  for (int h = h0; h < h1; ++h) {
    const float xnext = x_raw(h + 3);
    rdx_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int sl = oslot(h + kh);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int o = sl + bx_img(pw + kw, 2 * s + hh);
          const hx8 xh = *reinterpret_cast<const hx8*>(osh + o);
          const hx8 xl = *reinterpret_cast<const hx8*>(osl + o);
          acc = mfma32x32x16(wh[kh * 3 + kw][s], xh, acc);   // Y^T: rows co, columns positions
          acc = mfma32x32x16(wh[kh * 3 + kw][s], xl, acc);
          acc = mfma32x32x16(wl[kh * 3 + kw][s], xh, acc);
        }
    }
    if (h + 1 < h1) make_out1(h + 2);   // the next row's second input row (slot of row h - 1: read last row)
    {  // s = (a + idn) + bias at position q0 + pw, channels 8g + 4hh + e
      const float* xh = xslot(h);
      const float x0 = xh[pw + 1], x1 = xh[pw + 2], x2 = xh[pw + 3];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4 pr = prec[8 * g + 4 * hh + e];
          const float iv = fmaf(x0, pr.x, fmaf(x1, pr.y, x2 * pr.z));
          o[e] = (acc[4 * g + e] + iv) + pr.w;
        }
        *reinterpret_cast<float4*>(ss + pw * BX_SP + 8 * g + 4 * hh) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
    if (tid < BX_XW) xslot(h + 3)[tid] = x_val(h + 3, xnext);   // the slot of x row h - 1 (no reader after the last barrier)
    __syncthreads();
    if (tid < BX_J * 4) {   // pool: (window j, 8 channels) per thread
      const int j = tid >> 2, g = tid & 3;
      const int jo = strip * BX_J + j;
      if (jo < a.Wo) {
        float best[8];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const float* sp = ss + (3 * j + t) * BX_SP + 8 * g;
          const float4 lo = *reinterpret_cast<const float4*>(sp), hi = *reinterpret_cast<const float4*>(sp + 4);
          const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (t == 0 || v[k] > best[k] || v[k] != v[k]) best[k] = v[k];   // torch max_pool2d: val > max || isnan(val)
        }
        float* yo = a.y + (((int64_t)n * H + h) * a.Wo + jo) * BX_C + 8 * g;
        *reinterpret_cast<float4*>(yo) = make_float4(best[0], best[1], best[2], best[3]);
        *reinterpret_cast<float4*>(yo + 4) = make_float4(best[4], best[5], best[6], best[7]);
      }
    }
    __syncthreads();
  }
}
#endif  // !RDX_F16

}  // namespace sx3
}  // namespace rdx

using namespace rdx;

namespace {
[[maybe_unused]] inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" int rdx_x3_b0x_fwd(const float* x, const float* fbn, const float* w1, const float* wd, const float* bn,
                              const void* w2_hi, const void* w2_lo, const float* bias, float* y, int N, int H, int W,
                              void* stream) {
  RDX_REQUIRE(x && w1 && wd && bn && w2_hi && w2_lo && bias && y && N > 0 && H > 0 && W > 0);
  if (W < 3 || N > 65535) return RDX_EUNSUPPORTED;
#ifdef RDX_F16
  return RDX_EINVAL;
#else
  RDX_REQUIRE(al16(y) && al16(w2_hi) && al16(w2_lo));
  const int Wo = W / 3;
  const int strips = (Wo + sx3::BX_J - 1) / sx3::BX_J;
  // row chunks only when the (strip, utterance) grid alone cannot fill the chip (each chunk recomputes 2 rows)
  int nz = (int)((2048 + (int64_t)strips * N - 1) / ((int64_t)strips * N));
  nz = nz < 1 ? 1 : (nz > 6 ? 6 : nz);
  const int rows_per = (H + nz - 1) / nz;
  nz = (H + rows_per - 1) / rows_per;
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sx3::b0x_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, sx3::BX_LDS);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  sx3::B0Args a{x, fbn, w1, wd, bn, (const hst*)w2_hi, (const hst*)w2_lo, bias, y, N, H, W, Wo, rows_per};
  hipLaunchKernelGGL(sx3::b0x_kernel, dim3((unsigned)strips, (unsigned)N, (unsigned)nz), dim3(sx3::BX_T), sx3::BX_LDS,
                     as_stream(stream), a);
  RDX_LAUNCH_CHECK();
  return RDX_OK;
#endif
}

extern "C" int rdx_x3_sconv_fwd(const float* x, const void* w_hi, const void* w_lo, const float* bn, float* y, int N,
                                int H, int W, int ci, int co, int kh, int ph, void* stream) {
  RDX_REQUIRE(x && w_hi && w_lo && y && N > 0 && H > 0 && W > 0);
  if ((ci != 32 && ci != 64) || (co != 32 && co != 64) || (kh != 1 && kh != 2) || (ph != 0 && ph != 1))
    return RDX_EUNSUPPORTED;
  const int Ho = H + 2 * ph - kh + 1;
  if (Ho < 1 || Ho > 65535 || N > 65535) return RDX_EUNSUPPORTED;
#ifdef RDX_F16
  return RDX_EINVAL;
#else
  RDX_REQUIRE(al16(x) && al16(w_hi) && al16(w_lo) && al16(y) && x != y);
  sx3::ConvArgs a{x, (const hst*)w_hi, (const hst*)w_lo, bn, y, H, W, Ho, ph};
  const dim3 grid((unsigned)((W + sx3::SX_ROWS - 1) / sx3::SX_ROWS), (unsigned)Ho, (unsigned)N);
  hipStream_t st = as_stream(stream);
#define SX_GO(CI, CO, KH) hipLaunchKernelGGL((sx3::conv_kernel<CI, CO, KH>), grid, dim3(256), 0, st, a)
  if (ci == 32 && co == 32) { if (kh == 1) SX_GO(32, 32, 1); else SX_GO(32, 32, 2); }
  else if (ci == 32 && co == 64) { if (kh == 1) SX_GO(32, 64, 1); else SX_GO(32, 64, 2); }
  else if (ci == 64 && co == 32) { if (kh == 1) SX_GO(64, 32, 1); else SX_GO(64, 32, 2); }
  else { if (kh == 1) SX_GO(64, 64, 1); else SX_GO(64, 64, 2); }
#undef SX_GO
  RDX_LAUNCH_CHECK();
  return RDX_OK;
#endif
}
