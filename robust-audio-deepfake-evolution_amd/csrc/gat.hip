// Attention map and aggregation of one graph-attention layer for gfx950 (RawGAT-ST's GAT_layer_T / _S / _ST,
// reference models/RawNetGatSpoofST.py:49-81; AASIST's GraphAttentionLayer is the same map with a temperature), one
// workgroup per utterance, forward and backward, fp32 throughout. The module path writes the [B, N, N, Din] pair
// product and the [B, N, N, Dout] projection to memory and takes about a dozen launches forward and twice that
// backward; here the pair tensor lives in registers.
//
// Per utterance, x [N, Din], W [Dout, Din], b [Dout], w [Dout]:
//   p[i,j,o] = b[o] + sum_d W[o,d] x[i,d] x[j,d]       s[i,j] = (sum_o w[o] tanh(p[i,j,o])) / temp
//   a[i,:]   = softmax_j(s[i,:])  (row maximum subtracted)   agg[i,:] = sum_j a[i,j] x[j,:]
// Backward, G = d agg:
//   da[i,j] = G[i] . x[j],  ds[i,j] = a[i,j] (da[i,j] - sum_k a[i,k] da[i,k]),  dp[i,j,o] = ds[i,j] / temp w[o] (1 - tanh^2)
//   dw[o] = sum_ij ds[i,j] tanh(p[i,j,o]) / temp,  db[o] = sum_ij dp[i,j,o],  dW[o,d] = sum_ij dp[i,j,o] x[i,d] x[j,d]
//   dx[j] += sum_i a[i,j] G[i];  dx[i,d] += sum_j sum_o dp[i,j,o] W[o,d] x[j,d];  dx[j,d] += sum_i sum_o dp[i,j,o] W[o,d] x[i,d]
// p is symmetric in (i, j) to the bit (x[i,d] * x[j,d] commutes and the sums run in one order), so with
// e[i,j] = (ds[i,j] + ds[j,i]) / temp and g[i,j,o] = e[i,j] w[o] (1 - tanh^2) = dp[i,j,o] + dp[j,i,o]:
//   Y[i,o,d] = sum_j g[i,j,o] x[j,d]
//   dx[i,d] (last two terms) = sum_o W[o,d] Y[i,o,d],  dW[o,d] = 1/2 sum_i x[i,d] Y[i,o,d]
//   db[o] = 1/2 sum_ij g[i,j,o],  dw[o] = 1/2 sum_ij e[i,j] tanh(p[i,j,o])
//
// Work split (256 threads = 4 waves):
//   pair phase   one thread per node pair (i, j): q[d] = x[i,d] x[j,d] in registers, W rows read from LDS as float4
//                at an address common to the wave (a broadcast, no bank conflict), x rows at an odd stride
//                (DQ + 1 floats) so that lanes j = 0..31 of a 32-lane read group land on 32 different banks
//   softmax      one wave per row, lane j = column j
//   aggregation  one thread per (i, d)
//   backward     rows in chunks of 256 / N: the pair phase leaves g of the chunk in LDS ([pair][o], the o of a wave
//                contiguous) and adds its wave's share of db / dw to that wave's own LDS slots; then wave v, lane d
//                forms Y[i, o = 4k + v, d] over j (one broadcast float4 of g per four o, one conflict-free x[j,d])
//                and from it dW (registers, over all rows) and its share of dx[i,d] (LDS, one slot per wave)
// Every sum runs in a fixed order and nothing uses atomics: the same inputs give the same bits. Each utterance
// writes its own dW / db / dw slot; the caller adds the B slots in a fixed order.
#include "common.h"

namespace rdx {

constexpr int GAT_THREADS = 256;
constexpr int GAT_WAVES = GAT_THREADS / 64;
constexpr int GAT_MAXN = 32;     // one lane per column of an attention row
constexpr int GAT_MAXD = 64;     // one lane per feature in the backward's second phase, 64 q registers per pair
constexpr int GAT_MAXO = 64;     // 16 o per wave in the backward's second phase
constexpr int GAT_LDA = GAT_MAXN + 1;

__host__ __device__ inline int gat_dq(int Din) { return Din <= 32 ? 32 : 64; }          // padded feature count
__host__ __device__ inline int gat_ko(int Dout) { return (((Dout + 3) / 4) + 3) & ~3; }  // o per wave, a multiple of 4
__host__ __device__ inline int gat_ldp(int Dout) { return 4 * gat_ko(Dout) + 4; }
__host__ __device__ inline int gat_up4(int n) { return (n + 3) & ~3; }                    // float4 reads stay aligned

inline size_t gat_fwd_lds(int N, int Din, int Dout) {
  const int DQ = gat_dq(Din);
  return sizeof(float) * ((size_t)gat_up4(N * (DQ + 1)) + (size_t)Dout * DQ + 2 * GAT_MAXO + (size_t)N * GAT_LDA);
}
inline size_t gat_bwd_lds(int N, int Din, int Dout) {
  const int DQ = gat_dq(Din);
  return sizeof(float) * (2 * (size_t)gat_up4(N * (DQ + 1)) + (size_t)Dout * DQ + 2 * GAT_MAXO +
                          2 * (size_t)gat_up4(N * GAT_LDA) + (size_t)GAT_THREADS * gat_ldp(Dout) +
                          (size_t)GAT_WAVES * N * DQ + (size_t)GAT_WAVES * 2 * GAT_MAXO);
}

__device__ __forceinline__ float gat_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// x (zero-padded to DQ features, row stride DQ + 1), W (rows of DQ, zero-padded), b and w into LDS
template <int DQ>
__device__ __forceinline__ void gat_stage(const float* __restrict__ x, const float* __restrict__ W,
                                          const float* __restrict__ b, const float* __restrict__ w, int N, int Din,
                                          int Dout, float* xs, float* Ws, float* bs, float* ws) {
  const int tid = threadIdx.x;
  for (int e = tid; e < N * DQ; e += GAT_THREADS) {
    const int i = e / DQ, d = e - i * DQ;
    xs[i * (DQ + 1) + d] = d < Din ? x[i * Din + d] : 0.f;
  }
  for (int e = tid; e < Dout * DQ; e += GAT_THREADS) {
    const int o = e / DQ, d = e - o * DQ;
    Ws[e] = d < Din ? W[o * Din + d] : 0.f;
  }
  if (tid < GAT_MAXO) {
    bs[tid] = tid < Dout ? b[tid] : 0.f;
    ws[tid] = tid < Dout ? w[tid] : 0.f;
  }
}

// p[o] of one pair from its q: four partial sums over d (d mod 4), added as ((0 + 1) + (2 + 3)) + b[o]
template <int DQ>
__device__ __forceinline__ float gat_p(const float (&q)[DQ], const float* Wo, float bo) {
  const float4* wr = reinterpret_cast<const float4*>(Wo);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int c = 0; c < DQ / 4; ++c) {
    const float4 v = wr[c];
    a0 = fmaf(v.x, q[4 * c + 0], a0);
    a1 = fmaf(v.y, q[4 * c + 1], a1);
    a2 = fmaf(v.z, q[4 * c + 2], a2);
    a3 = fmaf(v.w, q[4 * c + 3], a3);
  }
  return ((a0 + a1) + (a2 + a3)) + bo;
}

template <int DQ>
__global__ __launch_bounds__(GAT_THREADS) void gat_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                              const float* __restrict__ b,
                                                              const float* __restrict__ w, float temp, int N, int Din,
                                                              int Dout, float* __restrict__ att,
                                                              float* __restrict__ agg) {
  extern __shared__ __align__(16) float gat_lds[];
  constexpr int LDX = DQ + 1;
  float* Ws = gat_lds;                     // [Dout][DQ], 16-byte aligned rows
  float* xs = Ws + Dout * DQ;              // [N][LDX]
  float* bs = xs + gat_up4(N * LDX);       // [GAT_MAXO]
  float* ws = bs + GAT_MAXO;               // [GAT_MAXO]
  float* S = ws + GAT_MAXO;                // [N][GAT_LDA] scores, then the attention map
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t u = blockIdx.x;
  x += u * N * Din;
  gat_stage<DQ>(x, W, b, w, N, Din, Dout, xs, Ws, bs, ws);
  __syncthreads();

  for (int pr = tid; pr < N * N; pr += GAT_THREADS) {
    const int i = pr / N, j = pr - i * N;
    float q[DQ];
#pragma unroll
    for (int d = 0; d < DQ; ++d) q[d] = xs[i * LDX + d] * xs[j * LDX + d];
    float s = 0.f;
    for (int o = 0; o < Dout; ++o) s = fmaf(ws[o], tanhf(gat_p<DQ>(q, Ws + o * DQ, bs[o])), s);
    S[i * GAT_LDA + j] = s / temp;
  }
  __syncthreads();

  for (int i = wv; i < N; i += GAT_WAVES) {
    const bool in = lane < N;
    const float v = in ? S[i * GAT_LDA + lane] : -INFINITY;
    const float m = gat_wave_max(v);
    const float e = in ? expf(v - m) : 0.f;
    const float a = e / wave_sum(e);
    if (in) {
      S[i * GAT_LDA + lane] = a;
      att[(u * N + i) * N + lane] = a;
    }
  }
  __syncthreads();

  for (int e = tid; e < N * Din; e += GAT_THREADS) {
    const int i = e / Din, d = e - i * Din;
    float acc = 0.f;
    for (int j = 0; j < N; ++j) acc = fmaf(S[i * GAT_LDA + j], xs[j * LDX + d], acc);
    agg[u * N * Din + e] = acc;
  }
}

template <int DQ>
__global__ __launch_bounds__(GAT_THREADS) void gat_bwd_kernel(const float* __restrict__ dagg,
                                                              const float* __restrict__ x, const float* __restrict__ W,
                                                              const float* __restrict__ b,
                                                              const float* __restrict__ w, float temp,
                                                              const float* __restrict__ att, int N, int Din, int Dout,
                                                              float* __restrict__ dx, float* __restrict__ dW,
                                                              float* __restrict__ db, float* __restrict__ dw) {
  extern __shared__ __align__(16) float gat_lds[];
  constexpr int LDX = DQ + 1;
  const int KO = gat_ko(Dout), LDP = gat_ldp(Dout);
  float* Ws = gat_lds;                          // [Dout][DQ]
  float* DP = Ws + Dout * DQ;                   // [GAT_THREADS][LDP]: g of the chunk's pairs, o = 4k + v at v * KO + k
  float* xs = DP + GAT_THREADS * LDP;           // [N][LDX]
  float* Gs = xs + gat_up4(N * LDX);            // [N][LDX] d agg
  float* A = Gs + gat_up4(N * LDX);             // [N][GAT_LDA] attention map
  float* E = A + gat_up4(N * GAT_LDA);          // [N][GAT_LDA] ds / temp
  float* bs = E + gat_up4(N * GAT_LDA);         // [GAT_MAXO]
  float* ws = bs + GAT_MAXO;                    // [GAT_MAXO]
  float* PART = ws + GAT_MAXO;                  // [GAT_WAVES][N][DQ] each wave's share of dx's pair terms
  float* RED = PART + GAT_WAVES * N * DQ;       // [GAT_WAVES][2][GAT_MAXO] each wave's share of dw, db
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t u = blockIdx.x;
  x += u * N * Din;
  dagg += u * N * Din;
  att += u * N * N;
  dx += u * N * Din;
  gat_stage<DQ>(x, W, b, w, N, Din, Dout, xs, Ws, bs, ws);
  for (int e = tid; e < N * DQ; e += GAT_THREADS) {
    const int i = e / DQ, d = e - i * DQ;
    Gs[i * LDX + d] = d < Din ? dagg[i * Din + d] : 0.f;
  }
  for (int e = tid; e < N * N; e += GAT_THREADS) {
    const int i = e / N, j = e - i * N;
    A[i * GAT_LDA + j] = att[e];
  }
  for (int e = tid; e < GAT_WAVES * 2 * GAT_MAXO; e += GAT_THREADS) RED[e] = 0.f;
  __syncthreads();

  // ds / temp: one wave per row, lane j = column j
  for (int i = wv; i < N; i += GAT_WAVES) {
    const bool in = lane < N;
    const int j = in ? lane : 0;
    float da = 0.f;
    for (int d = 0; d < DQ; ++d) da = fmaf(Gs[i * LDX + d], xs[j * LDX + d], da);
    const float a = in ? A[i * GAT_LDA + j] : 0.f;
    const float r = wave_sum(a * da);
    if (in) E[i * GAT_LDA + j] = a * (da - r) / temp;
  }
  // dx's first term, sum_i a[i,j] G[i,d] into row j; the thread that writes element e here adds the rest at the end
  for (int e = tid; e < N * Din; e += GAT_THREADS) {
    const int j = e / Din, d = e - j * Din;
    float acc = 0.f;
    for (int i = 0; i < N; ++i) acc = fmaf(A[i * GAT_LDA + j], Gs[i * LDX + d], acc);
    dx[e] = acc;
  }
  __syncthreads();

  // wave v, lane d owns o = 4k + v (k < KO) at feature d
  const int dl = lane < DQ ? lane : 0;
  float Wreg[GAT_MAXO / GAT_WAVES], dWacc[GAT_MAXO / GAT_WAVES];
#pragma unroll
  for (int k = 0; k < GAT_MAXO / GAT_WAVES; ++k) {
    const int o = 4 * k + wv;
    Wreg[k] = o < Dout ? Ws[o * DQ + dl] : 0.f;
    dWacc[k] = 0.f;
  }

  const int R = GAT_THREADS / N;               // rows per chunk
  for (int i0 = 0; i0 < N; i0 += R) {
    {
      // pair phase: every thread runs it (wave_sum needs the whole wave), threads without a pair with e = 0
      const int il = tid / N, jj = tid - il * N;
      const bool valid = il < R && i0 + il < N;
      const int i = valid ? i0 + il : 0, j = valid ? jj : 0;
      float q[DQ];
#pragma unroll
      for (int d = 0; d < DQ; ++d) q[d] = xs[i * LDX + d] * xs[j * LDX + d];
      const float e = valid ? E[i * GAT_LDA + j] + E[j * GAT_LDA + i] : 0.f;
      for (int o = 0; o < Dout; ++o) {
        const float t = tanhf(gat_p<DQ>(q, Ws + o * DQ, bs[o]));
        const float g = e * ws[o] * (1.0f - t * t);
        DP[tid * LDP + (o & 3) * KO + (o >> 2)] = g;
        const float rw = wave_sum(e * t);
        const float rb = wave_sum(g);
        if (lane == 0) {
          RED[(wv * 2 + 0) * GAT_MAXO + o] += rw;
          RED[(wv * 2 + 1) * GAT_MAXO + o] += rb;
        }
      }
    }
    __syncthreads();
    const int Rc = N - i0 < R ? N - i0 : R;
    for (int il = 0; il < Rc; ++il) {
      const int i = i0 + il;
      float Y[GAT_MAXO / GAT_WAVES];
#pragma unroll
      for (int k = 0; k < GAT_MAXO / GAT_WAVES; ++k) Y[k] = 0.f;
      for (int j = 0; j < N; ++j) {
        const float xv = xs[j * LDX + dl];
        const float4* gp = reinterpret_cast<const float4*>(DP + (il * N + j) * LDP + wv * KO);
#pragma unroll
        for (int c = 0; c < GAT_MAXO / GAT_WAVES / 4; ++c) {
          if (4 * c < KO) {
            const float4 v = gp[c];
            Y[4 * c + 0] = fmaf(v.x, xv, Y[4 * c + 0]);
            Y[4 * c + 1] = fmaf(v.y, xv, Y[4 * c + 1]);
            Y[4 * c + 2] = fmaf(v.z, xv, Y[4 * c + 2]);
            Y[4 * c + 3] = fmaf(v.w, xv, Y[4 * c + 3]);
          }
        }
      }
      const float xi = xs[i * LDX + dl];
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < GAT_MAXO / GAT_WAVES; ++k) {
        if (4 * k + wv < Dout) {        // slots of o >= Dout in DP are never written: their Y is not used
          dWacc[k] = fmaf(xi, Y[k], dWacc[k]);
          part = fmaf(Wreg[k], Y[k], part);
        }
      }
      if (lane < DQ) PART[(wv * N + i) * DQ + lane] = part;
    }
    __syncthreads();
  }

  for (int e = tid; e < N * Din; e += GAT_THREADS) {
    const int i = e / Din, d = e - i * Din;
    float acc = dx[e];
#pragma unroll
    for (int v = 0; v < GAT_WAVES; ++v) acc += PART[(v * N + i) * DQ + d];
    dx[e] = acc;
  }
  if (dW) {
    if (lane < Din) {
#pragma unroll
      for (int k = 0; k < GAT_MAXO / GAT_WAVES; ++k) {
        const int o = 4 * k + wv;
        if (o < Dout) dW[(u * Dout + o) * Din + lane] = 0.5f * dWacc[k];
      }
    }
    if (tid < Dout) {
      float sw = 0.f, sb = 0.f;
#pragma unroll
      for (int v = 0; v < GAT_WAVES; ++v) {
        sw += RED[(v * 2 + 0) * GAT_MAXO + tid];
        sb += RED[(v * 2 + 1) * GAT_MAXO + tid];
      }
      dw[u * Dout + tid] = 0.5f * sw;
      db[u * Dout + tid] = 0.5f * sb;
    }
  }
}

inline bool gat_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace rdx

using namespace rdx;

extern "C" int rdx_gat_eligible(const void* x, int N, int Din, int Dout, float temp) {
  return x && gat_aligned(x) && N >= 1 && N <= GAT_MAXN && Din >= 1 && Din <= GAT_MAXD && Dout >= 1 &&
         Dout <= GAT_MAXO && temp > 0.f;
}

extern "C" int rdx_gat_att_fwd(const float* x, const float* W, const float* b, const float* w, float temp, int B, int N,
                               int Din, int Dout, float* att, float* agg, void* stream) {
  RDX_REQUIRE(x && W && b && w && att && agg && B > 0);
  if (!rdx_gat_eligible(x, N, Din, Dout, temp) || !gat_aligned(W) || !gat_aligned(att) || !gat_aligned(agg))
    return RDX_EUNSUPPORTED;
  hipStream_t s = as_stream(stream);
  const size_t lds = gat_fwd_lds(N, Din, Dout);     // at most 29 KiB
  if (gat_dq(Din) == 32)
    hipLaunchKernelGGL(gat_fwd_kernel<32>, dim3((unsigned)B), dim3(GAT_THREADS), lds, s, x, W, b, w, temp, N, Din,
                       Dout, att, agg);
  else
    hipLaunchKernelGGL(gat_fwd_kernel<64>, dim3((unsigned)B), dim3(GAT_THREADS), lds, s, x, W, b, w, temp, N, Din,
                       Dout, att, agg);
  RDX_LAUNCH_CHECK();
  return RDX_OK;
}

extern "C" int rdx_gat_att_bwd(const float* dagg, const float* x, const float* W, const float* b, const float* w,
                               float temp, const float* att, int B, int N, int Din, int Dout, float* dx, float* dW,
                               float* db, float* dw, void* stream) {
  RDX_REQUIRE(dagg && x && W && b && w && att && dx && B > 0);
  RDX_REQUIRE((dW && db && dw) || (!dW && !db && !dw));      // the weight gradients come together or not at all
  if (!rdx_gat_eligible(x, N, Din, Dout, temp) || !gat_aligned(W) || !gat_aligned(dagg) || !gat_aligned(att) ||
      !gat_aligned(dx))
    return RDX_EUNSUPPORTED;
  hipStream_t s = as_stream(stream);
  const size_t lds = gat_bwd_lds(N, Din, Dout);
  const bool d32 = gat_dq(Din) == 32;
  if (lds > 64 * 1024) {
    // the chunk's g buffer alone is 68 KiB at Dout = 64; above the 64 KiB a launch gets by default the limit is
    // raised on each such launch (host-side only, no state kept here), as csrc/ocsupcon.hip does
    const void* fn = d32 ? reinterpret_cast<const void*>(&gat_bwd_kernel<32>)
                         : reinterpret_cast<const void*>(&gat_bwd_kernel<64>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)gat_bwd_lds(GAT_MAXN, GAT_MAXD, GAT_MAXO));
    if (e != hipSuccess) return (int)e;
  }
  if (d32)
    hipLaunchKernelGGL(gat_bwd_kernel<32>, dim3((unsigned)B), dim3(GAT_THREADS), lds, s, dagg, x, W, b, w, temp, att,
                       N, Din, Dout, dx, dW, db, dw);
  else
    hipLaunchKernelGGL(gat_bwd_kernel<64>, dim3((unsigned)B), dim3(GAT_THREADS), lds, s, dagg, x, W, b, w, temp, att,
                       N, Din, Dout, dx, dW, db, dw);
  RDX_LAUNCH_CHECK();
  return RDX_OK;
}
