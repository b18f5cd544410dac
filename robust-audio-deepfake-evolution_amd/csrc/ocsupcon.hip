// OC-Softmax + supervised-contrastive criteria of one pass for gfx950: the mixup loss over the features, its
// gradient through both L2 normalisations and the centre's gradient in one launch, and the backward in one more,
// instead of the several hundred small framework kernels the module path (radhip.train.OCSoftmax / SupConLoss)
// issues per pass.
//
// Reference: src/loss.py:5-47 (OC-Softmax, learnable 1 x D centre), :49-152 (SupCon, one view, mode 'all'),
// combined by train_epoch (src/main.py:1054-1071) as lam * L(y_a) + (1 - lam) * L(y_b), L = P + lambda * S, divided
// by the accumulation steps. Restated from the math, per micro-batch of B rows f_i (D features), centre c:
//   z_i = f_i / max(|f_i|, 1e-12),  w = c / max(|c|, 1e-12),  s_i = z_i . w
//   P(y) = 1/B sum_i softplus(alpha * (y_i == 1 ? r_real - s_i : s_i - r_fake))      (softplus(x) = x for x > 20)
//   l_ij = z_i . z_j / T,  a_ij = l_ij - max_j l_ij,  E_i = sum_{j != i} exp(a_ij) + 1e-8
//   S(y) = 1/B sum_i -(T / T_base) * sum_{j in pos(i)} (a_ij - log E_i) / max(|pos(i)|, 1e-8)   (non-finite row: 0)
//   pos(i) = { j != i : y_j == y_i }
// Gradients (the row maximum is a constant, as in the reference's .detach()):
//   dP/ds_i = 1/B * sigma(u_i) * alpha * (y_i == 1 ? -1 : 1)
//   dS/dl_ij = -(T / T_base) / B * ([j in pos(i)] - |pos(i)| * exp(a_ij) / E_i) / max(|pos(i)|, 1e-8),  j != i
//   dL/dz_i = dP/ds_i * w + lambda / T * sum_j (dS/dl_ij + dS/dl_ji) z_j
//   dL/df_i = (dL/dz_i - (dL/dz_i . z_i) z_i) / |f_i|        (|f_i| < 1e-12: dL/dz_i / 1e-12, the clamp's branch)
//   dL/dw   = sum_i dP/ds_i z_i,   dL/dc = (dL/dw - (dL/dw . w) w) / |c|
// One workgroup per micro-batch keeps its normalised rows and the B x B matrix (logits, then the dS/dl
// coefficients in place) in LDS; all arithmetic is fp32; every reduction runs in a fixed order (no floating-point
// atomics), so two launches on the same inputs agree bit for bit. Micro-batch k writes its loss term and its centre
// gradient to slot k; the forward's last step adds the K loss terms in slot order, the backward the K centre
// gradients.
#include "common.h"

namespace rdx {

constexpr int OS_THREADS = 256;
constexpr int OS_WAVES = OS_THREADS / 64;
constexpr int OS_MAXB = 64;    // one lane per column of a row of the B x B matrix
constexpr int OS_MAXD = 256;   // one thread per feature of the centre gradient
constexpr float OS_EPS = 1e-12f;   // F.normalize's eps

__host__ __device__ inline int os_ldz(int D) { return D | 1; }   // odd row stride: column reads hit distinct banks
inline size_t os_lds_bytes(int B, int D) {
  return sizeof(float) * ((size_t)B * os_ldz(D) + (size_t)B * (B + 1) + 2 * (size_t)OS_MAXD + 3 * (size_t)OS_MAXB +
                          2 * OS_WAVES) + sizeof(int) * 2 * (size_t)OS_MAXB;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// softplus (torch: beta 1, threshold 20) and its derivative
__device__ __forceinline__ float os_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float os_sigmoid(float x) { return x > 20.f ? 1.0f : 1.0f / (1.0f + expf(-x)); }

struct OsArgs {
  const void* feats;
  int ld, D, B;
  const float* center;
  const int64_t* ya;
  const int64_t* yb;
  const float* lam;
  float r_real, r_fake, alpha, lambda_supcon, temp, base_temp, scale;
  float* loss;         // the scalar when the grid is one block, else unused here
  float* loss_parts;   // [grid] when the grid has more than one block
  float* dfeats;       // [R, D]
  float* dcparts;      // [grid, D], NULL without a centre
};

template <typename T>
__global__ __launch_bounds__(OS_THREADS) void ocsupcon_fwd_kernel(OsArgs a) {
  extern __shared__ float os_lds[];
  const int B = a.B, D = a.D, LDZ = os_ldz(D), LDM = B + 1;
  float* z = os_lds;                       // [B][LDZ] rows, normalised in place
  float* M = z + B * LDZ;                  // [B][LDM] logits, then the coefficients
  float* w = M + B * LDM;                  // [OS_MAXD] normalised centre
  float* dw = w + OS_MAXD;                 // [OS_MAXD]
  float* nrm = dw + OS_MAXD;               // [OS_MAXB] |f_i|
  float* g = nrm + OS_MAXB;                // [OS_MAXB] dP/ds_i (mixed)
  float* spare = g + OS_MAXB;              // [OS_MAXB]
  float* red = spare + OS_MAXB;            // [2 * OS_WAVES]
  int* la = reinterpret_cast<int*>(red + 2 * OS_WAVES);   // [OS_MAXB] labels a
  int* lb = la + OS_MAXB;                                  // [OS_MAXB] labels b
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int k = blockIdx.x;
  const int64_t r0 = (int64_t)k * B;
  const T* f = reinterpret_cast<const T*>(a.feats) + r0 * a.ld;
  const bool oc = a.center != nullptr;
  const bool sc = a.lambda_supcon != 0.f;
  const bool mix = a.yb != nullptr;
  const float l1 = a.lam ? a.lam[k] : 1.0f;
  const float l2 = mix ? 1.0f - l1 : 0.f;
  const float invB = 1.0f / (float)B;

  for (int e = tid; e < B * D; e += OS_THREADS) {
    const int i = e / D, d = e - i * D;
    z[i * LDZ + d] = ld(f, (int64_t)i * a.ld + d);
  }
  if (tid < B) {
    la[tid] = (int)a.ya[r0 + tid];
    lb[tid] = mix ? (int)a.yb[r0 + tid] : 0;
    g[tid] = 0.f;
  }
  // the centre: every wave computes |c| (the same sum in the same order), wave 0 keeps w
  float cden = 1.0f;
  bool cclamp = false;
  if (oc) {
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) ss += a.center[d] * a.center[d];
    const float cn = sqrtf(wave_sum(ss));
    cclamp = cn < OS_EPS;
    cden = fmaxf(cn, OS_EPS);
    if (wv == 0)
      for (int d = lane; d < D; d += 64) w[d] = a.center[d] / cden;
  }
  __syncthreads();

  // rows: norm, normalise in place, cosine to the centre, the OC term (one wave per row)
  float lacc = 0.f;    // this wave's loss terms (meaningful in lane 0)
  for (int i = wv; i < B; i += OS_WAVES) {
    float* zi = z + i * LDZ;
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) ss += zi[d] * zi[d];
    const float n = sqrtf(wave_sum(ss));
    const float den = fmaxf(n, OS_EPS);
    float dot = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float v = zi[d] / den;
      zi[d] = v;
      if (oc) dot += v * w[d];
    }
    if (oc) dot = wave_sum(dot);
    if (lane == 0) {
      nrm[i] = n;
      if (oc) {
        const float sa = la[i] == 1 ? -1.0f : 1.0f;
        const float ua = a.alpha * (la[i] == 1 ? a.r_real - dot : dot - a.r_fake);
        float lo = l1 * os_softplus(ua);
        float gi = l1 * os_sigmoid(ua) * a.alpha * sa;
        if (mix) {
          const float sb = lb[i] == 1 ? -1.0f : 1.0f;
          const float ub = a.alpha * (lb[i] == 1 ? a.r_real - dot : dot - a.r_fake);
          lo += l2 * os_softplus(ub);
          gi += l2 * os_sigmoid(ub) * a.alpha * sb;
        }
        lacc += lo * invB;
        g[i] = gi * invB;
      }
    }
  }
  __syncthreads();

  if (sc) {
    // logits l_ij = z_i . z_j / T (the same products in the same order for (i, j) and (j, i): symmetric to the bit)
    const float invT = 1.0f / a.temp;
    for (int p = tid; p < B * B; p += OS_THREADS) {
      const int i = p / B, j = p - i * B;
      const float* zi = z + i * LDZ;
      const float* zj = z + j * LDZ;
      float acc = 0.f;
      for (int d = 0; d < D; ++d) acc = fmaf(zi[d], zj[d], acc);
      M[i * LDM + j] = acc * invT;
    }
    __syncthreads();
    // one wave per row, lane j = column j: softmax denominator without the diagonal, the positives of both label
    // sets, the row's loss and its coefficients dS/dl_ij (times lambda / T) in place
    const float tr = a.temp / a.base_temp;
    const float cg = a.lambda_supcon * invT * tr * invB;
    for (int i = wv; i < B; i += OS_WAVES) {
      const bool in = lane < B;
      const bool off = in && lane != i;
      const float lij = in ? M[i * LDM + lane] : -INFINITY;
      const float m = wave_max(lij);
      // E_i and the log-probabilities relative to the largest OFF-diagonal logit (sh = its distance below the row
      // maximum, the diagonal's 1 / T): exp(a_ij) = exp(sh) * ex_j and E_i = exp(sh) * (se + c8), so
      // a_ij - log E_i = (l_ij - m_off) - log(se + c8) with se >= 1. The same value, without subtracting two numbers
      // near -1 / T whose difference is small (two rows, or one close neighbour: log E_i is then nearly a_ij). For an
      // off-diagonal maximum further down than exp() can undo in fp32 the row is taken relative to its maximum
      const float moff = wave_max(off ? lij : -INFINITY);
      const bool rel = moff - m > -60.f;
      const float base = rel ? moff : m;
      const float aij = lij - base;
      const float ex = off ? expf(aij) : 0.f;
      const float c8 = rel ? 1e-8f * expf(m - moff) : 1e-8f;
      const float se = wave_sum(ex);
      const float E = se + c8;
      const float lp = aij - logf(E);
      float coef = 0.f;
      float rowloss = 0.f;
      for (int s = 0; s < (mix ? 2 : 1); ++s) {
        const int* lab = s == 0 ? la : lb;
        const float wgt = s == 0 ? l1 : l2;
        const bool pos = off && lab[lane] == lab[i];
        const float np = wave_sum(pos ? 1.0f : 0.f);
        const float sp = wave_sum(pos ? lp : 0.f);
        const float nn = fmaxf(np, 1e-8f);
        const float r = -tr * sp / nn;
        if (isfinite(r)) {
          rowloss += wgt * r;
          // [j in pos] - |pos| ex_j / E = ([j in pos] c8 + ([j in pos] se - |pos| ex_j)) / E: with one positive and
          // no other row the bracket is exactly 0 and the 1e-8 term is what remains, not a rounding of 1 - ex / E
          if (off) coef -= wgt * ((pos ? c8 : 0.f) + ((pos ? se : 0.f) - np * ex)) / (nn * E);
        }
      }
      if (in) M[i * LDM + lane] = coef * cg;
      if (lane == 0) lacc += a.lambda_supcon * rowloss * invB;
    }
    __syncthreads();
  }

  // dL/dz_i, then through the row's normalisation (one wave per row, lanes over the features)
  for (int i = wv; i < B; i += OS_WAVES) {
    const float* zi = z + i * LDZ;
    float acc[OS_MAXD / 64];
    const float gi = g[i];
#pragma unroll
    for (int c = 0; c < OS_MAXD / 64; ++c) {
      const int d = lane + 64 * c;
      acc[c] = (oc && d < D) ? gi * w[d] : 0.f;
    }
    if (sc) {
      for (int j = 0; j < B; ++j) {
        const float cf = M[i * LDM + j] + M[j * LDM + i];
        const float* zj = z + j * LDZ;
#pragma unroll
        for (int c = 0; c < OS_MAXD / 64; ++c) {
          const int d = lane + 64 * c;
          if (d < D) acc[c] = fmaf(cf, zj[d], acc[c]);
        }
      }
    }
    const float n = nrm[i];
    float* out = a.dfeats + (r0 + i) * D;
    if (n < OS_EPS) {
#pragma unroll
      for (int c = 0; c < OS_MAXD / 64; ++c) {
        const int d = lane + 64 * c;
        if (d < D) out[d] = a.scale * (acc[c] / OS_EPS);
      }
    } else {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < OS_MAXD / 64; ++c) {
        const int d = lane + 64 * c;
        if (d < D) dot = fmaf(acc[c], zi[d], dot);
      }
      dot = wave_sum(dot);
#pragma unroll
      for (int c = 0; c < OS_MAXD / 64; ++c) {
        const int d = lane + 64 * c;
        if (d < D) out[d] = a.scale * ((acc[c] - dot * zi[d]) / n);
      }
    }
  }

  // the centre's gradient of this micro-batch: dL/dw (thread d), then through the centre's normalisation
  if (oc) {
    float dwd = 0.f, wd = 0.f;
    if (tid < D) {
      for (int i = 0; i < B; ++i) dwd = fmaf(g[i], z[i * LDZ + tid], dwd);
      wd = w[tid];
    }
    const float part = wave_sum(dwd * wd);
    if (lane == 0) red[wv] = part;
    __syncthreads();
    float dot = 0.f;
    for (int q = 0; q < OS_WAVES; ++q) dot += red[q];
    if (tid < D)
      a.dcparts[(int64_t)k * D + tid] = a.scale * (cclamp ? dwd / OS_EPS : (dwd - dot * wd) / cden);
  }

  if (lane == 0) red[OS_WAVES + wv] = lacc;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int q = 0; q < OS_WAVES; ++q) t += red[OS_WAVES + q];
    if (gridDim.x == 1)
      a.loss[0] = a.scale * t;
    else
      a.loss_parts[k] = a.scale * t;
  }
}

// loss = the K micro-batch terms added in slot order
__global__ void ocsupcon_loss_sum_kernel(const float* __restrict__ parts, int K, float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < K; ++k) t += parts[k];
    loss[0] = t;
  }
}

// dfeats = g * d32 in the features' dtype (elements [0, n)); dcenter[d] = g * sum_k dcparts[k][d] in slot order
// (elements [n, n + D))
template <typename T>
__global__ __launch_bounds__(OS_THREADS) void ocsupcon_bwd_kernel(const float* __restrict__ grad,
                                                                   const float* __restrict__ d32, T* __restrict__ out,
                                                                   int64_t n, const float* __restrict__ dcparts, int K,
                                                                   int D, float* __restrict__ dcenter) {
  const float s = grad[0];
  const int64_t tot = n + (dcparts ? D : 0);
  for (int64_t i = (int64_t)blockIdx.x * OS_THREADS + threadIdx.x; i < tot; i += (int64_t)gridDim.x * OS_THREADS) {
    if (i < n) {
      st(out, i, d32[i] * s);
    } else {
      const int d = (int)(i - n);
      float t = 0.f;
      for (int k = 0; k < K; ++k) t += dcparts[(int64_t)k * D + d];
      dcenter[d] = t * s;
    }
  }
}

}  // namespace rdx

using namespace rdx;

extern "C" int rdx_ocsupcon_eligible(const void* feats, int ld_, int R, int D, int B) {
  return feats && B >= 2 && B <= OS_MAXB && D >= 1 && D <= OS_MAXD && R > 0 && R % B == 0 && ld_ >= D &&
         ((uintptr_t)feats & 15) == 0;
}

extern "C" int rdx_ocsupcon_mixup_fwd(const void* feats, int feats_bf16, int ld_, int R, int D, const float* center,
                                      const int64_t* ya, const int64_t* yb, const float* lam, int rows_per_lam,
                                      float r_real, float r_fake, float alpha, float lambda_supcon, float temperature,
                                      float base_temperature, float scale, float* loss, float* loss_parts,
                                      float* dfeats, float* dcenter_parts, void* stream) {
  RDX_REQUIRE(feats && ya && loss && dfeats && R > 0 && D > 0 && rows_per_lam > 0);
  RDX_REQUIRE(center || lambda_supcon != 0.f);              // at least one of the two criteria
  RDX_REQUIRE(!center || dcenter_parts);
  RDX_REQUIRE(lambda_supcon == 0.f || (temperature > 0.f && base_temperature > 0.f));
  const int B = rows_per_lam;
  if (!rdx_ocsupcon_eligible(feats, ld_, R, D, B)) return RDX_EUNSUPPORTED;
  const int K = R / B;
  RDX_REQUIRE(K == 1 || loss_parts);
  const size_t lds = os_lds_bytes(B, D);
  hipStream_t s = as_stream(stream);
  OsArgs a{feats, ld_, D, B, center, ya, yb, lam, r_real, r_fake, alpha, lambda_supcon, temperature,
           base_temperature, scale, loss, loss_parts, dfeats, dcenter_parts};
  if (lds > 64 * 1024) {
    // only B near 64 with D above ~170 (83.8 KiB at B = 64, D = 256) passes the 64 KiB a launch gets by default.
    // Asked for on each such launch: the attribute belongs to the current device's copy of the kernel, the call is
    // host-side only and keeps no state here that threads or devices could share
    const void* fn = feats_bf16 ? reinterpret_cast<const void*>(&ocsupcon_fwd_kernel<hst>)
                                : reinterpret_cast<const void*>(&ocsupcon_fwd_kernel<float>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)os_lds_bytes(OS_MAXB, OS_MAXD));
    if (e != hipSuccess) return (int)e;
  }
  if (feats_bf16)
    hipLaunchKernelGGL(ocsupcon_fwd_kernel<hst>, dim3((unsigned)K), dim3(OS_THREADS), lds, s, a);
  else
    hipLaunchKernelGGL(ocsupcon_fwd_kernel<float>, dim3((unsigned)K), dim3(OS_THREADS), lds, s, a);
  RDX_LAUNCH_CHECK();
  if (K > 1) {
    hipLaunchKernelGGL(ocsupcon_loss_sum_kernel, dim3(1), dim3(64), 0, s, loss_parts, K, loss);
    RDX_LAUNCH_CHECK();
  }
  return RDX_OK;
}

extern "C" int rdx_ocsupcon_mixup_bwd(const float* grad, const float* dfeats, void* out, int out_bf16, int64_t n,
                                      const float* dcenter_parts, int K, int D, float* dcenter, void* stream) {
  RDX_REQUIRE(grad && dfeats && out && n > 0);
  RDX_REQUIRE(!dcenter_parts || (dcenter && K > 0 && D > 0));
  hipStream_t s = as_stream(stream);
  const int64_t tot = n + (dcenter_parts ? D : 0);
  const int64_t nb = (tot + OS_THREADS - 1) / OS_THREADS;
  const int blocks = (int)(nb < 256 ? nb : 256);
  if (out_bf16)
    hipLaunchKernelGGL(ocsupcon_bwd_kernel<hst>, dim3(blocks), dim3(OS_THREADS), 0, s, grad, dfeats, (hst*)out, n,
                       dcenter_parts, K, D, dcenter);
  else
    hipLaunchKernelGGL(ocsupcon_bwd_kernel<float>, dim3(blocks), dim3(OS_THREADS), 0, s, grad, dfeats, (float*)out, n,
                       dcenter_parts, K, D, dcenter);
  RDX_LAUNCH_CHECK();
  return RDX_OK;
}
