// Fused pieces of the WavLM encoder layer (stable layer norm, frozen base + LoRA q/v) for the
// Phase-6 training step: everything between the four hipBLASLt GEMMs and the MFMA attention.
//
// Reference: HF WavLMEncoderLayerStableLayerNorm / WavLMAttention / WavLMFeedForward (transformers
// modeling_wavlm.py) as run by WavLMFrontend (src/models/DualStreamSEMamba.py:292-439), with peft
// LoRA on q_proj/v_proj (src/main.py:103-158):
//     x1 = LN1(h);  gate = ga * (gb * c_h - 1) + 2,  (ga, gb) = sigmoid(sum4(Wg x1_head + bg))
//     [q k v] = x1 [Wq Wk Wv]^T + b + s * (B_q A_q drop(x1), 0, B_v A_v drop(x1))
//     h2 = h + drop(out_proj(attn(q, k, v, gate)));  x2 = LN2(h2)
//     h' = h2 + drop(W2 gelu(W1 x2 + b1) + b2)
// Layout: one, two or four waves per token row (E = 1024 = 4 chunks of 64 lanes x 4 contiguous fp32, see
// "Row layout" below), so a row's LN statistics and its 2r = 16 LoRA down-projections are wave
// reductions (combined through LDS when waves share a row) and its 16 per-head gates sums over
// 16-lane rows. The
// (combined through LDS when waves share a row) and its 16 per-head gates sums over 16-lane rows.
// The LoRA down-projection a = A drop(x1) is written next to x1 into one
// [M, E + 2r] bf16 operand, so the q/k/v GEMM (K = E + 2r against [Wqkv | s B]) applies the whole
// LoRA update with no extra GEMM; its backward returns d a in the same GEMM.
// Dropout: counter-hash masks (common.h) keyed by (layer seed, salt, m * E + e), regenerated in the
// backward; the seed lives in device memory (HIP-graph replayable).
#include "common.h"

namespace rdx {

constexpr int WL_E = 1024;
constexpr int WL_VPL = WL_E / RDX_WAVE;  // 16 fp32 per lane
constexpr int WL_R2 = 16;                // 2 * LoRA rank (q and v adapters, r = 8)

struct Drop {
  const int64_t* seed_dev;
  int salt;
  uint32_t thr;    // p * 2^32 (0: identity)
  float inv_keep;  // 1 / (1 - p)
};

__device__ __forceinline__ float drop_scale(const Drop& d, uint64_t seed, uint64_t idx) {
  return drop_keep(seed, idx, d.thr) ? d.inv_keep : 0.f;
}

// ---- Row layout of the row kernels --------------------------------------------------------------------------------
// A row is 4 chunks of WL_CHUNK = 256 elements; in chunk c lane l owns the 4 elements c * 256 + 4 l .. + 3, so one
// 16-byte fp32 instruction of a wave covers one contiguous 1 KB span and one 8-byte 16-bit instruction a contiguous
// 512 B span (lane-owns-16-contiguous touched 32 cache lines per instruction, the same 32 four times per row).
// W = 1, 2 or 4 waves share a row: wave w of the row owns the N = 4 / W chunks w * N .. w * N + N - 1, and a lane's
// value k (0 .. 4 N - 1) is element e0 + wl_elem(k), e0 = w * N * 256 + 4 lane. The helpers below take the lane's
// pointer (row + e0).
constexpr int WL_CHUNK = 4 * RDX_WAVE;
__device__ __forceinline__ constexpr int wl_elem(int k) { return (k >> 2) * WL_CHUNK + (k & 3); }

template <int N>
__device__ __forceinline__ void load_chunks(const float* p, float* v) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float4 t = *reinterpret_cast<const float4*>(p + j * WL_CHUNK);
    v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
  }
}
template <int N>
__device__ __forceinline__ void store_chunks(float* p, const float* v) {
#pragma unroll
  for (int j = 0; j < N; ++j)
    *reinterpret_cast<float4*>(p + j * WL_CHUNK) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
}
// raw 16-bit chunks (one 8-byte load each), unpacked later: keeps the unpack from pinning a wait between a row's loads
template <int N>
struct HChunks {
  uint2 q[N];
};
template <int N>
__device__ __forceinline__ HChunks<N> load_chunks_h_raw(const hst* p) {
  HChunks<N> t;
#pragma unroll
  for (int j = 0; j < N; ++j) t.q[j] = *reinterpret_cast<const uint2*>(p + j * WL_CHUNK);
  return t;
}
template <int N>
__device__ __forceinline__ void unpack_chunks_h(const HChunks<N>& t, float* v) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    v[4 * j] = hlo(t.q[j].x);
    v[4 * j + 1] = hhi(t.q[j].x);
    v[4 * j + 2] = hlo(t.q[j].y);
    v[4 * j + 3] = hhi(t.q[j].y);
  }
}
template <int N>
__device__ __forceinline__ void store_chunks_h(hst* p, const float* v) {
#pragma unroll
  for (int j = 0; j < N; ++j)
    *reinterpret_cast<uint2*>(p + j * WL_CHUNK) =
        make_uint2(hbits(v[4 * j]) | (hbits(v[4 * j + 1]) << 16), hbits(v[4 * j + 2]) | (hbits(v[4 * j + 3]) << 16));
}

// Total of the W row-waves' wave sums (every lane of a wave holds `part`), through this row's W LDS slots with one
// barrier, added in wave order 0 .. W - 1 by everyone: all lanes of the row get the bit-identical total and two runs
// agree. Every wave of the workgroup calls it (a dead row's waves too: the barrier). W = 1 is the plain wave sum.
template <int W>
__device__ __forceinline__ float row_total(float part, float* slots, int w, int lane) {
  if (W == 1) return part;
  if (lane == 0) slots[w] = part;
  __syncthreads();
  float t = slots[0];
#pragma unroll
  for (int k = 1; k < W; ++k) t += slots[k];
  return t;
}

// mean / rstd of a row held as 16 / W values per lane of W waves (two-pass, biased variance like torch); slots: this
// row's [2][W] floats of LDS
template <int W>
__device__ __forceinline__ void row_stats(const float* v, float eps, float& mean, float& rstd, float* slots, int w,
                                          int lane) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < WL_VPL / W; ++i) s += v[i];
  mean = row_total<W>(wave_sum(s), slots, w, lane) * (1.0f / WL_E);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < WL_VPL / W; ++i) {
    float d = v[i] - mean;
    q += d * d;
  }
  rstd = rsqrtf(row_total<W>(wave_sum(q), slots + W, w, lane) * (1.0f / WL_E) + eps);
}

// Sum 16 per-lane values over the wave with 17 shuffles: lane l ends with the total of index
// k(l) = 8 b5 + 4 b4 + 2 b3 + b2 (b = bits of l); lanes with l & 3 == 0 own distinct k.
__device__ __forceinline__ float wave_sum16(float* v, int lane) {
  float w8[8], w4[4], w2[2];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float r = __shfl_xor(h5 ? v[j] : v[j + 8], 32, 64);
    w8[j] = (h5 ? v[j + 8] : v[j]) + r;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float r = __shfl_xor(h4 ? w8[j] : w8[j + 4], 16, 64);
    w4[j] = (h4 ? w8[j + 4] : w8[j]) + r;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float r = __shfl_xor(h3 ? w4[j] : w4[j + 2], 8, 64);
    w2[j] = (h3 ? w4[j + 2] : w4[j]) + r;
  }
  float r = __shfl_xor(h2 ? w2[0] : w2[1], 4, 64);
  float t = (h2 ? w2[1] : w2[0]) + r;
  t += __shfl_xor(t, 2, 64);
  t += __shfl_xor(t, 1, 64);
  return t;
}
__device__ __forceinline__ int sum16_index(int lane) {
  return 8 * ((lane >> 5) & 1) + 4 * ((lane >> 4) & 1) + 2 * ((lane >> 3) & 1) + ((lane >> 2) & 1);
}

struct GateW {
  const float* wg;      // [8, 64] gru_rel_pos_linear.weight
  const float* bg;      // [8]
  const float* gconst;  // [H] gru_rel_pos_const
};

// The two gate pre-activation sums (za = z0 + .. + z3, zb = z4 + .. + z7) of the head of each of the lane's N chunks:
// a chunk holds 4 heads, one per 16-lane DPP row (head = 4 chunk + lane / 16, the lane's 4 dims at 4 (lane % 16)), so
// a head's dot products are row sums; wg in LDS. Every lane of the row gets both sums. Call with the whole wave active.
template <int N>
__device__ __forceinline__ void gate_z(const GateW& g, const float* wgp, const float* x, int lane, float* za,
                                       float* zb) {
  const int d0 = (lane & 15) * 4;
  float4 w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = *reinterpret_cast<const float4*>(wgp + j * 64 + d0);
  const float ba = g.bg[0] + g.bg[1] + g.bg[2] + g.bg[3], bb = g.bg[4] + g.bg[5] + g.bg[6] + g.bg[7];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s[j >> 2] += w[j].x * x[4 * c] + w[j].y * x[4 * c + 1] + w[j].z * x[4 * c + 2] + w[j].w * x[4 * c + 3];
    za[c] = row16_sum(s[0]) + ba;
    zb[c] = row16_sum(s[1]) + bb;
  }
}

struct Ln1Args {
  const float* h;  // [M, E] layer input (fp32 residual stream)
  const float* gamma;
  const float* beta;
  float eps;
  GateW g;
  const hst* Aq;    // [r, E] lora_A (q) in the 16-bit storage type (autocast's cast), null without LoRA
  const hst* Av;    // [r, E] lora_A (v)
  Drop dq, dv;      // LoRA dropouts (q, v)
  hst* x1;  // [M, ldx]: LN1 output in [0, E), LoRA down-projection in [E, E + 2r)
  int64_t ldx;
  float* gate;  // [M, H]
  float* mean;
  float* rstd;
  int64_t M;
  // optional residual prologue (the previous layer's last step): h = h2 + drop(delta) is computed here and
  // written to hout (h is then unused)
  const float* h2;
  const hst* delta;
  Drop dres;
  float* hout;
};

// LoRA-A of both adapters staged once per workgroup of WL_LN1_ROWS row-waves (4): [2r][E] 16-bit (the cast autocast
// applies to lora_A's weight, made once per pass by the caller), 32 KB copied with 16-byte loads. A row-wave reading
// the fp32 A from L2 itself moved 64 KB per token row and left these kernels L2-bound (26 us of the 47 us forward
// at B = 32); staging it from fp32 with the conversion here still read 64 KB per workgroup.
#ifndef WL_LN1_ROWS_DEF
#define WL_LN1_ROWS_DEF 4   // rows per workgroup of the LoRA-active LN1 kernels (one wave per row): measured, 4 rows
#endif                      // beat 8 and 2 at both pass sizes (tools/bench_wl.py)
constexpr int WL_LN1_ROWS = WL_LN1_ROWS_DEF;

// The staging of a LN1 workgroup, gate weights (2 KB fp32) and LoRA-A (32 KB 16-bit), straight from global memory
// into LDS by buffer_load ... lds (16 bytes per lane, lane-linear: one wave-instruction fills 1 KB), issued before the
// rows' own loads and retired by the waitcnt ahead of the barrier: every load of the prologue in flight at once and
// no registers. (A loop that stored each chunk as it arrived waited out one L2 round trip per chunk, 8 per thread:
// most of the LoRA kernels' extra time over the LoRA-free variant; staging through registers loads-first kept the
// round trips but the compiler sank the loads back to their stores under the row kernels' register pressure.)
typedef __attribute__((ext_vector_type(4))) int wl_i32x4;
__device__ void wl_load_lds(wl_i32x4 rsrc, __attribute__((address_space(3))) uint32_t* lds, int size, int voffset,
                            int soffset, int offset, int aux) __asm("llvm.amdgcn.raw.buffer.load.lds");
__device__ __forceinline__ wl_i32x4 wl_rsrc(const void* base, uint32_t bytes) {
  const uint64_t a = (uint64_t)base;
  wl_i32x4 r;
  r.x = (int)(uint32_t)a;
  r.y = (int)(uint32_t)(a >> 32);
  r.z = (int)bytes;
  r.w = 0x00020000;  // raw buffer, range-checked
  return r;
}
template <bool kLora, int NW>   // NW: waves of the workgroup
__device__ __forceinline__ void stage_dma(float* swg, hst* sA, const float* wg, const hst* Aq, const hst* Av) {
  constexpr int WL_A_INSTR = WL_R2 * WL_E * 2 / 1024 / NW;   // LoRA-A instructions per wave (8 at 4 waves)
  static_assert(!kLora || (NW == WL_LN1_ROWS && WL_A_INSTR % 2 == 0 && WL_A_INSTR * 1024 * NW == WL_R2 * WL_E * 2),
                "LoRA-A is staged by WL_LN1_ROWS one-wave rows: whole 1 KB instructions, half per adapter");
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv == 0) {
    const wl_i32x4 rg = wl_rsrc(wg, 8 * 64 * 4);
#pragma unroll
    for (int q = 0; q < 2; ++q)
      wl_load_lds(rg, (__attribute__((address_space(3))) uint32_t*)(reinterpret_cast<char*>(swg) + 1024 * q), 16,
                  1024 * q + 16 * lane, 0, 0, 0);
  }
  if (kLora) {
    const wl_i32x4 rq = wl_rsrc(Aq, WL_R2 / 2 * WL_E * 2), rv = wl_rsrc(Av, WL_R2 / 2 * WL_E * 2);
#pragma unroll
    for (int j = 0; j < WL_A_INSTR; ++j) {
      const int q = wv + NW * j;                       // 1 KB instruction q of the [2r][E] image
      constexpr int half = WL_R2 / 2 * WL_E * 2 / 1024; // instructions per adapter (16)
      wl_load_lds(j < WL_A_INSTR / 2 ? rq : rv,         // q < half exactly when j < WL_A_INSTR / 2 (compile time)
                  (__attribute__((address_space(3))) uint32_t*)(reinterpret_cast<char*>(sA) + 1024 * q), 16,
                  1024 * (q % half) + 16 * lane, 0, 0, 0);
    }
  }
}

// W waves per row, R rows per workgroup (see the row layout above). Dead rows (m >= M) run to the end with zeros and
// store nothing: the row reductions and the LoRA combine have barriers.
template <bool kLora, int W, int R>
__global__ __launch_bounds__(W * R * RDX_WAVE) void wl_ln1_fwd_kernel(Ln1Args a) {
  constexpr int N = 4 / W, NV = WL_VPL / W;   // chunks and values per lane
  __shared__ __attribute__((aligned(16))) hst sA[kLora ? WL_R2 * WL_E : 8];
  __shared__ __attribute__((aligned(16))) float swg[8 * 64];
  __shared__ float sred[R][2 * W];
  static_assert(!kLora || W == 1, "the LoRA-active kernels run one wave per row (no geometry measured faster)");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = wv / W, w = wv % W;
  const int64_t m = (int64_t)blockIdx.x * R + row;
  const bool live = m < a.M;  // no early return: the gate and LoRA parts follow a barrier
  const int e0 = w * N * WL_CHUNK + lane * 4;
  float v[NV], gm[NV], bt[NV], dl[NV];
  HChunks<N> dlr;
  const uint64_t sr = (a.h2 && a.dres.thr) ? attn_seed(a.dres.seed_dev, a.dres.salt) : 0;  // with the row loads
  // every global load first (one round trip): the workgroup's staging, the row, the affine parameters
  stage_dma<kLora, W * R>(swg, sA, a.g.wg, a.Aq, a.Av);
  if (live) {
    load_chunks<N>(a.h2 ? a.h2 + m * WL_E + e0 : a.h + m * WL_E + e0, v);
    if (a.h2) dlr = load_chunks_h_raw<N>(a.delta + m * WL_E + e0);
    load_chunks<N>(a.gamma + e0, gm);
    load_chunks<N>(a.beta + e0, bt);
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.f;
  }
  __builtin_amdgcn_s_waitcnt(0);   // the staging DMA (and the row) landed
  __syncthreads();
  if (live && a.h2) {
    unpack_chunks_h<N>(dlr, dl);
#pragma unroll
    for (int i = 0; i < NV; ++i)
      v[i] += dl[i] * (a.dres.thr ? drop_scale(a.dres, sr, (uint64_t)m * WL_E + e0 + wl_elem(i)) : 1.0f);
    store_chunks<N>(a.hout + m * WL_E + e0, v);
  }
  float mean, rstd;
  row_stats<W>(v, a.eps, mean, rstd, sred[row], w, lane);
  if (live) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = hround((v[i] - mean) * rstd * gm[i] + bt[i]);
    store_chunks_h<N>(a.x1 + m * a.ldx + e0, v);
    if (w == 0 && lane == 0) {
      a.mean[m] = mean;
      a.rstd[m] = rstd;
    }
    float za[N], zb[N];
    gate_z<N>(a.g, swg, v, lane, za, zb);
    if ((lane & 15) == 0) {
#pragma unroll
      for (int c = 0; c < N; ++c) {
        const int head = (w * N + c) * 4 + (lane >> 4);
        const float ga = sigmoidf_(za[c]), gb = sigmoidf_(zb[c]);
        a.gate[m * (WL_E / 64) + head] = ga * (gb * a.g.gconst[head] - 1.0f) + 2.0f;
      }
    }
  }
  if (kLora) {
    if (!live) return;
    const uint64_t sq = a.dq.thr ? attn_seed(a.dq.seed_dev, a.dq.salt) : 0;
    const uint64_t sv = a.dv.thr ? attn_seed(a.dv.seed_dev, a.dv.salt) : 0;
    // each adapter's dropped row in the 16-bit type (the reference's dropout output: lora_A's input under
    // autocast), packed in pairs, and the down-projection as packed dot products (v_dot2c_f32_*: one per pair
    // instead of 2 unpacks + 2 FMAs; the per-row VALU work of these 2r dot products was the LoRA kernels' extra time)
    uint32_t mq[NV / 2], mv[NV / 2];
#pragma unroll
    for (int j = 0; j < NV / 2; ++j) {
      const uint64_t idx = (uint64_t)m * WL_E + e0 + wl_elem(2 * j);
      mq[j] = hpack2(v[2 * j] * drop_scale(a.dq, sq, idx), v[2 * j + 1] * drop_scale(a.dq, sq, idx + 1));
      mv[j] = hpack2(v[2 * j] * drop_scale(a.dv, sv, idx), v[2 * j + 1] * drop_scale(a.dv, sv, idx + 1));
    }
    float acc[WL_R2];
#pragma unroll
    for (int k = 0; k < WL_R2; ++k) {
      const uint32_t* x = k < WL_R2 / 2 ? mq : mv;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < N; ++c) {   // 8 bytes per lane, lane-linear: conflict-free
        const uint2 wk = *reinterpret_cast<const uint2*>(sA + k * WL_E + e0 + c * WL_CHUNK);
        s = hdot2(wk.x, x[2 * c], s);
        s = hdot2(wk.y, x[2 * c + 1], s);
      }
      acc[k] = s;
    }
    const float tot = wave_sum16(acc, lane);
    if ((lane & 3) == 0) a.x1[m * a.ldx + WL_E + sum16_index(lane)] = f2h(tot);
  }
}

// h2 = h + drop(delta) (fp32, stored), x = LN(h2) (bf16), mean / rstd saved
struct AddLnArgs {
  const float* h;
  const hst* delta;
  Drop d;
  float* h2;
  const float* gamma;
  const float* beta;
  float eps;
  hst* x;
  float* mean;
  float* rstd;
  int64_t M;
};

template <int W, int R>
__global__ __launch_bounds__(W * R * RDX_WAVE) void wl_add_ln_fwd_kernel(AddLnArgs a) {
  constexpr int N = 4 / W, NV = WL_VPL / W;
  __shared__ float sred[R][2 * W];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = wv / W, w = wv % W;
  const int64_t m = (int64_t)blockIdx.x * R + row;
  const bool live = m < a.M;
  if (W == 1 && !live) return;   // more waves per row: dead rows reach the reductions' barriers
  const int e0 = w * N * WL_CHUNK + lane * 4;
  float v[NV], dl[NV], gm[NV], bt[NV];
  if (live) {
    load_chunks<N>(a.h + m * WL_E + e0, v);
    const HChunks<N> dlr = load_chunks_h_raw<N>(a.delta + m * WL_E + e0);
    load_chunks<N>(a.gamma + e0, gm);   // with the row's loads: one round trip
    load_chunks<N>(a.beta + e0, bt);
    unpack_chunks_h<N>(dlr, dl);
    const uint64_t seed = a.d.thr ? attn_seed(a.d.seed_dev, a.d.salt) : 0;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      v[i] += dl[i] * (a.d.thr ? drop_scale(a.d, seed, (uint64_t)m * WL_E + e0 + wl_elem(i)) : 1.0f);
    store_chunks<N>(a.h2 + m * WL_E + e0, v);
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.f;
  }
  float mean, rstd;
  row_stats<W>(v, a.eps, mean, rstd, sred[row], w, lane);
  if (!live) return;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = (v[i] - mean) * rstd * gm[i] + bt[i];
  store_chunks_h<N>(a.x + m * WL_E + e0, v);
  if (w == 0 && lane == 0) {
    a.mean[m] = mean;
    a.rstd[m] = rstd;
  }
}


// out = h + drop(delta) over n = M * E elements (8 per thread)
__global__ __launch_bounds__(256) void wl_residual_kernel(const float* __restrict__ h,
                                                          const hst* __restrict__ delta, Drop d,
                                                          float* __restrict__ out, int64_t n) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  const uint64_t seed = d.thr ? attn_seed(d.seed_dev, d.salt) : 0;
  float4 a0 = reinterpret_cast<const float4*>(h + i0)[0], a1 = reinterpret_cast<const float4*>(h + i0)[1];
  float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  uint4 t = *reinterpret_cast<const uint4*>(delta + i0);
  uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float dv = (j & 1) ? hhi(w[j >> 1]) : hlo(w[j >> 1]);
    x[j] += dv * (d.thr ? drop_scale(d, seed, (uint64_t)(i0 + j)) : 1.0f);
  }
  reinterpret_cast<float4*>(out + i0)[0] = make_float4(x[0], x[1], x[2], x[3]);
  reinterpret_cast<float4*>(out + i0)[1] = make_float4(x[4], x[5], x[6], x[7]);
}

// grad of drop(): out = drop_mask * g (fp32 in, bf16 out), n elements (8 per thread)
__global__ __launch_bounds__(256) void wl_dropout_bwd_kernel(const float* __restrict__ g, Drop d,
                                                             hst* __restrict__ out, int64_t n) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  const uint64_t seed = d.thr ? attn_seed(d.seed_dev, d.salt) : 0;
  float4 a0 = reinterpret_cast<const float4*>(g + i0)[0], a1 = reinterpret_cast<const float4*>(g + i0)[1];
  float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s0 = d.thr ? drop_scale(d, seed, (uint64_t)(i0 + 2 * j)) : 1.0f;
    float s1 = d.thr ? drop_scale(d, seed, (uint64_t)(i0 + 2 * j + 1)) : 1.0f;
    w[j] = hbits(x[2 * j] * s0) | (hbits(x[2 * j + 1] * s1) << 16);
  }
  *reinterpret_cast<uint4*>(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * __expf(-0.5f * x * x);
}

// y = gelu(u) (mode 0) or du = dy * gelu'(u) (mode 1); bf16, 8 elements per thread
template <int kMode>
__global__ __launch_bounds__(256) void wl_gelu_kernel(const hst* __restrict__ u,
                                                      const hst* __restrict__ dy,
                                                      hst* __restrict__ out, int64_t n) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  uint4 t = *reinterpret_cast<const uint4*>(u + i0);
  uint32_t w[4] = {t.x, t.y, t.z, t.w}, gw[4] = {0, 0, 0, 0};
  if (kMode == 1) {
    uint4 g = *reinterpret_cast<const uint4*>(dy + i0);
    gw[0] = g.x; gw[1] = g.y; gw[2] = g.z; gw[3] = g.w;
  }
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float x0 = hlo(w[j]), x1 = hhi(w[j]);
    float y0, y1;
    if (kMode == 0) {
      y0 = gelu_erf(x0);
      y1 = gelu_erf(x1);
    } else {
      y0 = hlo(gw[j]) * gelu_erf_grad(x0);
      y1 = hhi(gw[j]) * gelu_erf_grad(x1);
    }
    o[j] = hbits(y0) | (hbits(y1) << 16);
  }
  *reinterpret_cast<uint4*>(out + i0) = make_uint4(o[0], o[1], o[2], o[3]);
}

// LN backward with residual: dh = dres + rstd * (g - mean(g) - xhat * mean(g xhat)), g = dx * gamma.
// Optionally also ddrop = drop_mask * dh (bf16): the gradient into the dropout that fed h.
struct LnBwdArgs {
  const hst* dx;  // [M, ldd] (first E columns used)
  int64_t ldd;
  const float* h;  // LN input [M, E]
  const float* mean;
  const float* rstd;
  const float* gamma;
  const float* dres;  // [M, E] or null
  float* dh;          // [M, E]
  Drop d;
  hst* ddrop;  // [M, E] or null
  int64_t M;
};

// slots: this row's [2][W] floats of LDS (both sums cross the waves behind one barrier)
template <int W>
__device__ __forceinline__ void ln_bwd_row(const float* dx, const float* x, float mean, float rstd, const float* gm,
                                           float* out, float* slots, int w, int lane) {
  constexpr int NV = WL_VPL / W;
  float g[NV], xh[NV], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    xh[i] = (x[i] - mean) * rstd;
    g[i] = dx[i] * gm[i];
    s1 += g[i];
    s2 += g[i] * xh[i];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (W > 1) {
    if (lane == 0) {
      slots[w] = s1;
      slots[W + w] = s2;
    }
    __syncthreads();
    s1 = slots[0];
    s2 = slots[W];
#pragma unroll
    for (int k = 1; k < W; ++k) {   // wave order, by everyone: bit-identical in every lane and every run
      s1 += slots[k];
      s2 += slots[W + k];
    }
  }
  s1 *= 1.0f / WL_E;
  s2 *= 1.0f / WL_E;
#pragma unroll
  for (int i = 0; i < NV; ++i) out[i] = rstd * (g[i] - s1 - xh[i] * s2);
}

template <int W, int R>
__global__ __launch_bounds__(W * R * RDX_WAVE) void wl_ln_bwd_kernel(LnBwdArgs a) {
  constexpr int N = 4 / W, NV = WL_VPL / W;
  __shared__ float sred[R][2 * W];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = wv / W, w = wv % W;
  const int64_t m = (int64_t)blockIdx.x * R + row;
  const bool live = m < a.M;
  if (W == 1 && !live) return;   // more waves per row: dead rows reach the reduction's barrier
  const int e0 = w * N * WL_CHUNK + lane * 4;
  float dx[NV], x[NV], gm[NV], o[NV], r[NV];
  float mean = 0.f, rstd = 0.f;
  const uint64_t seed = (a.ddrop && a.d.thr) ? attn_seed(a.d.seed_dev, a.d.salt) : 0;
  if (live) {
    const HChunks<N> dxr = load_chunks_h_raw<N>(a.dx + m * a.ldd + e0);
    load_chunks<N>(a.h + m * WL_E + e0, x);
    load_chunks<N>(a.gamma + e0, gm);
    if (a.dres) load_chunks<N>(a.dres + m * WL_E + e0, r);     // every load of the row before the reductions
    mean = a.mean[m];
    rstd = a.rstd[m];
    unpack_chunks_h<N>(dxr, dx);
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) dx[i] = x[i] = gm[i] = 0.f;
  }
  ln_bwd_row<W>(dx, x, mean, rstd, gm, o, sred[row], w, lane);
  if (!live) return;
  if (a.dres) {
#pragma unroll
    for (int i = 0; i < NV; ++i) o[i] += r[i];
  }
  store_chunks<N>(a.dh + m * WL_E + e0, o);
  if (a.ddrop) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      o[i] *= a.d.thr ? drop_scale(a.d, seed, (uint64_t)m * WL_E + e0 + wl_elem(i)) : 1.0f;
    store_chunks_h<N>(a.ddrop + m * WL_E + e0, o);
  }
}


// LN1 backward: dx1 = dX1[:, :E] + gate backward + LoRA-A backward; dh = dres + LN1_bwd(dx1).
// Also writes the dropped LN output of each adapter (xd[0] q, xd[1] v) for the dA GEMMs.
struct Ln1BwdArgs {
  const hst* dx1;  // [M, ldx] = d [x1 | a] from the qkv GEMM backward
  int64_t ldx;
  const float* dgate;  // [M, H]
  const float* h;
  const float* mean;
  const float* rstd;
  const float* gamma;
  const float* beta;
  GateW g;
  const hst* Aq;    // [r, E] 16-bit or null
  const hst* Av;
  Drop dq, dv;
  const float* dres;  // [M, E]
  float* dh;
  hst* xd;  // [2, M, E] or null
  int64_t M;
  // optional: the gradient this layer's INPUT receives as a hidden state of the layer-weighted sum,
  // sw[0] * sg (sw a device scalar: softmax(w)_l), added into dh
  const float* sg;
  const float* sw;
  // optional: ddrop = drop_prev(dh) bf16, the gradient of the previous layer's dropped FFN output
  Drop dprev;
  hst* ddrop;
};

template <bool kLora, int W, int R>
__global__ __launch_bounds__(W * R * RDX_WAVE) void wl_ln1_bwd_kernel(Ln1BwdArgs a) {
  static_assert(!kLora || W == 1, "the LoRA-active kernels run one wave per row");
  constexpr int N = 4 / W, NV = WL_VPL / W;
  __shared__ __attribute__((aligned(16))) hst sA[kLora ? WL_R2 * WL_E : 8];
  __shared__ __attribute__((aligned(16))) float swg[8 * 64];
  __shared__ float sred[R][2 * W];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = wv / W, w = wv % W;
  const int64_t m = (int64_t)blockIdx.x * R + row;
  const bool live = m < a.M;
  const int e0 = w * N * WL_CHUNK + lane * 4;
  const int d0 = (lane & 15) * 4, head0 = w * N * 4 + (lane >> 4);   // chunk c of the lane: head head0 + 4 c
  // every row load first: h, dx1, the residual gradient, the layer-sum gradient, the affine parameters
  float x[NV], x1[NV], dx[NV], r[NV], sgv[NV], gm[NV], dg[N];
  float mean = 0.f, rstd = 0.f;
  HChunks<N> dxr;
  const uint64_t sp = (a.ddrop && a.dprev.thr) ? attn_seed(a.dprev.seed_dev, a.dprev.salt) : 0;
  stage_dma<kLora, W * R>(swg, sA, a.g.wg, a.Aq, a.Av);
  if (live) {
    load_chunks<N>(a.h + m * WL_E + e0, x);
    dxr = load_chunks_h_raw<N>(a.dx1 + m * a.ldx + e0);
    load_chunks<N>(a.dres + m * WL_E + e0, r);
    if (a.sg) load_chunks<N>(a.sg + m * WL_E + e0, sgv);
    load_chunks<N>(a.gamma + e0, gm);
    load_chunks<N>(a.beta + e0, x1);
    mean = a.mean[m];
    rstd = a.rstd[m];
#pragma unroll
    for (int c = 0; c < N; ++c) dg[c] = a.dgate[m * (WL_E / 64) + head0 + 4 * c];
  }
  __builtin_amdgcn_s_waitcnt(0);   // the staging DMA (and the row) landed
  __syncthreads();
  if (W == 1 && !live) return;  // more waves per row: dead rows go on to the reduction's barrier with zeros
  if (live) {
    unpack_chunks_h<N>(dxr, dx);
#pragma unroll
    for (int i = 0; i < NV; ++i) x1[i] = hround((x[i] - mean) * rstd * gm[i] + x1[i]);
    // gate: gate = ga (gb c - 1) + 2
    float za[N], zb[N];
    gate_z<N>(a.g, swg, x1, lane, za, zb);
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const float ga = sigmoidf_(za[c]), gb = sigmoidf_(zb[c]);
      const float gc = a.g.gconst[head0 + 4 * c];
      const float dza = dg[c] * (gb * gc - 1.0f) * ga * (1.0f - ga);
      const float dzb = dg[c] * ga * gc * gb * (1.0f - gb);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float dz = j < 4 ? dza : dzb;
        const float4 t = *reinterpret_cast<const float4*>(swg + j * 64 + d0);
        dx[4 * c] += t.x * dz;
        dx[4 * c + 1] += t.y * dz;
        dx[4 * c + 2] += t.z * dz;
        dx[4 * c + 3] += t.w * dz;
      }
    }
    if (kLora) {
      const uint64_t sq = a.dq.thr ? attn_seed(a.dq.seed_dev, a.dq.salt) : 0;
      const uint64_t sv = a.dv.thr ? attn_seed(a.dv.seed_dev, a.dv.salt) : 0;
      if (a.xd) {  // the dropped LN output of each adapter (optional; first, so that x1 dies here)
#pragma unroll
        for (int which = 0; which < 2; ++which) {
          const Drop& dd = which ? a.dv : a.dq;
          const uint64_t sd = which ? sv : sq;
          float xm[NV];
#pragma unroll
          for (int i = 0; i < NV; ++i) xm[i] = x1[i] * drop_scale(dd, sd, (uint64_t)m * WL_E + e0 + wl_elem(i));
          store_chunks_h<N>(a.xd + (which * a.M + m) * WL_E + e0, xm);
        }
      }
      // the 2r down-projection gradients of this row, packed in k pairs (one 32-byte broadcast read); the term
      // sum_k A[k][e] da[k] of each element e as packed dot products over k pairs: the two A rows k, k + 1 read at the
      // lane's elements (8 contiguous bytes per lane and chunk, conflict-free), their 16-bit halves regrouped per
      // element
      const uint4 dap[2] = {*reinterpret_cast<const uint4*>(a.dx1 + m * a.ldx + WL_E),
                            *reinterpret_cast<const uint4*>(a.dx1 + m * a.ldx + WL_E + 8)};
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        float acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = 0.f;
        const uint32_t dk[4] = {dap[which].x, dap[which].y, dap[which].z, dap[which].w};
#pragma unroll
        for (int kp = 0; kp < WL_R2 / 4; ++kp) {
          const int k = which * (WL_R2 / 2) + 2 * kp;
#pragma unroll
          for (int c = 0; c < N; ++c) {
            const uint2 ra = *reinterpret_cast<const uint2*>(sA + k * WL_E + e0 + c * WL_CHUNK);
            const uint2 rb = *reinterpret_cast<const uint2*>(sA + (k + 1) * WL_E + e0 + c * WL_CHUNK);
            const uint32_t wa[2] = {ra.x, ra.y}, wb[2] = {rb.x, rb.y};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              // v_perm_b32 (selector bytes 0-3: the second operand's bytes, 4-7: the first's)
              const uint32_t ev = __builtin_amdgcn_perm(wb[j], wa[j], 0x05040100u);   // (A[k][2j], A[k + 1][2j])
              const uint32_t od = __builtin_amdgcn_perm(wb[j], wa[j], 0x07060302u);   // (A[k][2j + 1], A[k + 1][2j + 1])
              acc[4 * c + 2 * j] = hdot2(ev, dk[kp], acc[4 * c + 2 * j]);
              acc[4 * c + 2 * j + 1] = hdot2(od, dk[kp], acc[4 * c + 2 * j + 1]);
            }
          }
        }
        const Drop& dd = which ? a.dv : a.dq;
        const uint64_t sd = which ? sv : sq;
#pragma unroll
        for (int i = 0; i < NV; ++i) dx[i] += acc[i] * drop_scale(dd, sd, (uint64_t)m * WL_E + e0 + wl_elem(i));
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) dx[i] = x[i] = gm[i] = 0.f;
  }
  float o[NV];
  ln_bwd_row<W>(dx, x, mean, rstd, gm, o, sred[row], w, lane);
  if (!live) return;
#pragma unroll
  for (int i = 0; i < NV; ++i) o[i] += r[i];
  if (a.sg) {
    const float pw = a.sw[0];
#pragma unroll
    for (int i = 0; i < NV; ++i) o[i] = fmaf(pw, sgv[i], o[i]);
  }
  store_chunks<N>(a.dh + m * WL_E + e0, o);
  if (a.ddrop) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      o[i] *= a.dprev.thr ? drop_scale(a.dprev, sp, (uint64_t)m * WL_E + e0 + wl_elem(i)) : 1.0f;
    store_chunks_h<N>(a.ddrop + m * WL_E + e0, o);
  }
}


// LoRA weight gradients of one layer, ACCUMULATED into the fp32 .grad buffers:
//   dB_q[e, k] += s sum_m dq[m, e] a_q[m, k]        dA_q[k, e] += sum_m da_q[m, k] drop_q(x1)[m, e]
// (same for v). A block owns 128 columns and 4 * RPW rows: lane = 2 adjacent columns (bf16x2 loads,
// 256 B per wave-instruction), wave w = RPW consecutive rows whose loads are all issued before the
// FMAs (no per-row branch: rows past M read row M-1 against zeroed per-row factors). The 4 waves'
// 32 x 128 partial sums are reduced through LDS, then the block adds 4096 fp32 atomics laid out so
// each wave-instruction covers 64 consecutive dwords of dA ([r, E]) or dB ([E, r]).
constexpr int WL_LG_COLS = 128;
constexpr int WL_LG_PAD = WL_LG_COLS + 1;  // LDS row stride (floats): the dB read walks k

struct LoraGradArgs {
  const hst* dqkv;  // [M, ldq]: dq at column 0, dv at column 2E
  int64_t ldq;
  const hst* x1;    // [M, ldx]: x1 in [0, E), a in [E, E + 2r)
  int64_t ldx;
  const hst* dx1;   // [M, ldd]: d a in [E, E + 2r)
  int64_t ldd;
  Drop dq, dv;
  float scale;
  float *dAq, *dBq, *dAv, *dBv;
  int64_t M;
};

__device__ __forceinline__ float2 hx2_at(const hst* p) {
  const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
  return make_float2(hlo(u), hhi(u));
}

template <int RPW>
__global__ __launch_bounds__(256, 2) void wl_lora_grad_kernel(LoraGradArgs a, int nch) {
  constexpr int ROWS = 4 * RPW;  // rows per chunk; a block walks nch chunks
  __shared__ float s_row[2][ROWS][2 * WL_R2];
  __shared__ float s_part[4][2 * WL_R2][WL_LG_PAD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e0 = blockIdx.x * WL_LG_COLS;
  const int e = e0 + 2 * lane;
  constexpr int R = WL_R2 / 2;
  float bq[2][R], bv[2][R], aq[2][R], av[2][R];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int k = 0; k < R; ++k) bq[c][k] = bv[c][k] = aq[c][k] = av[c][k] = 0.f;
  const uint64_t sq = a.dq.thr ? attn_seed(a.dq.seed_dev, a.dq.salt) : 0;
  const uint64_t sv = a.dv.thr ? attn_seed(a.dv.seed_dev, a.dv.salt) : 0;
  for (int ch = 0; ch < nch; ++ch) {
    const int64_t m0 = ((int64_t)blockIdx.y * nch + ch) * ROWS;
    float(*srow)[2 * WL_R2] = s_row[ch & 1];
    for (int t = threadIdx.x; t < ROWS * 2 * WL_R2; t += 256) {
      const int rr = t / (2 * WL_R2), c = t % (2 * WL_R2);
      const int64_t m = m0 + rr;
      float v = 0.f;
      if (m < a.M)
        v = c < WL_R2 ? h2f(a.x1[m * a.ldx + WL_E + c])
                      : h2f(a.dx1[m * a.ldd + WL_E + c - WL_R2]);
      srow[rr][c] = v;
    }
    float2 gq[RPW], gv[RPW], xx[RPW];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int64_t m = min(m0 + w * RPW + j, a.M - 1);
      gq[j] = hx2_at(a.dqkv + m * a.ldq + e);
      gv[j] = hx2_at(a.dqkv + m * a.ldq + 2 * WL_E + e);
      xx[j] = hx2_at(a.x1 + m * a.ldx + e);
    }
    __syncthreads();  // srow staged (the other buffer is still read by nobody: one barrier per chunk)
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int rr = w * RPW + j;
      const uint64_t idx = (uint64_t)min(m0 + rr, a.M - 1) * WL_E + e;
      const float g_q[2] = {gq[j].x, gq[j].y}, g_v[2] = {gv[j].x, gv[j].y};
      const float xq[2] = {xx[j].x * drop_scale(a.dq, sq, idx), xx[j].y * drop_scale(a.dq, sq, idx + 1)};
      const float xv[2] = {xx[j].x * drop_scale(a.dv, sv, idx), xx[j].y * drop_scale(a.dv, sv, idx + 1)};
      const float* f = srow[rr];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < R; ++k) {
          bq[c][k] = fmaf(g_q[c], f[k], bq[c][k]);
          bv[c][k] = fmaf(g_v[c], f[R + k], bv[c][k]);
          aq[c][k] = fmaf(f[2 * R + k], xq[c], aq[c][k]);
          av[c][k] = fmaf(f[3 * R + k], xv[c], av[c][k]);
        }
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int k = 0; k < R; ++k) {
      s_part[w][k][2 * lane + c] = bq[c][k];
      s_part[w][R + k][2 * lane + c] = bv[c][k];
      s_part[w][2 * R + k][2 * lane + c] = aq[c][k];
      s_part[w][3 * R + k][2 * lane + c] = av[c][k];
    }
  __syncthreads();
  // 4096 outputs: o < 2048 -> dA (kk = o / 128 over aq then av, col = o % 128: lanes contiguous in e);
  // o >= 2048 -> dB (which = q/v, col = rem / 8, k = rem % 8: lanes contiguous in e * r + k).
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int o = i * 256 + threadIdx.x;
    int row, col;
    float* dst;
    float mul = 1.f;
    if (o < 2048) {
      const int kk = o / WL_LG_COLS;
      col = o % WL_LG_COLS;
      row = 2 * R + kk;
      dst = kk < R ? a.dAq + (int64_t)kk * WL_E + e0 + col : a.dAv + (int64_t)(kk - R) * WL_E + e0 + col;
    } else {
      const int o2 = o - 2048, which = o2 / (WL_LG_COLS * R), rem = o2 % (WL_LG_COLS * R);
      col = rem / R;
      const int k = rem % R;
      row = which * R + k;
      dst = (which ? a.dBv : a.dBq) + (int64_t)(e0 + col) * R + k;
      mul = a.scale;
    }
    const float v = s_part[0][row][col] + s_part[1][row][col] + s_part[2][row][col] + s_part[3][row][col];
    atomicAdd(dst, mul * v);
  }
}

// Wext[:, E:E+2r] <- s * B (q rows 0..E-1 columns E..E+r-1, v rows 2E..3E-1 columns E+r..E+2r-1);
// one launch for every layer. Other rows of those columns stay zero.
__global__ __launch_bounds__(256) void wl_lora_pack_kernel(int nl, const float* const* bq, const float* const* bv,
                                                           hst* const* wext, int64_t ldw, int r,
                                                           float scale) {
  const int l = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // over 2 * E * r
  if (l >= nl || t >= 2 * (int64_t)WL_E * r) return;
  const int which = (int)(t / ((int64_t)WL_E * r));
  const int64_t rem = t % ((int64_t)WL_E * r);
  const int64_t row = rem / r;
  const int k = (int)(rem % r);
  const float* b = which ? bv[l] : bq[l];  // lora_B weight [E, r]
  const int64_t wrow = which ? 2 * WL_E + row : row;
  wext[l][wrow * ldw + WL_E + which * r + k] = f2h(scale * b[row * r + k]);
}

}  // namespace rdx

using namespace rdx;

static Drop mk_drop(const int64_t* seed_dev, int salt, float p) {
  Drop d;
  d.seed_dev = seed_dev;
  d.salt = salt;
  d.thr = (p > 0.f && seed_dev) ? (uint32_t)fminf(4294967295.0f, p * 4294967296.0f) : 0u;
  d.inv_keep = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  return d;
}

// ---- Launch geometry of the four row kernels: (waves per row, rows per workgroup) ------------------------------------
// Chosen per kernel by M: below WL_ROWS_SMALL_M the adversarial passes (B = 8, M = 1608: 1.6 one-wave rows per SIMD,
// latency-bound), from it on the clean passes (B = 32, M = 6432). The table is the A/B of tools/bench_wl.py --waves
// (profiles/r09_bench_wl_waves.jsonl): two waves per row, two rows per workgroup everywhere but the small LN1 forward
// (four waves, one row). The LoRA-active LN1 kernels stay at one wave per row, WL_LN1_ROWS rows: no other geometry
// measured faster, and their 34 KB staging per row stays what it was. WL_GEOS_* list what each kernel is
// instantiated at: its table entries and (1, 4), the one-wave form (the LoRA-active kernels' geometry, and the form the
// tests hold the others against).
struct WlGeo {
  int w, r;
};
enum { WL_K_LN1_FWD = 0, WL_K_ADD_LN = 1, WL_K_LN_BWD = 2, WL_K_LN1_BWD = 3 };
#ifndef WL_ROWS_SMALL_M
#define WL_ROWS_SMALL_M 4096
#endif
#ifndef WL_GEO_TABLE_DEF
#define WL_GEO_TABLE_DEF {{{4, 1}, {2, 2}}, {{2, 2}, {2, 2}}, {{2, 2}, {2, 2}}, {{2, 2}, {2, 2}}}
#endif
static const WlGeo kWlGeo[4][2] = WL_GEO_TABLE_DEF;   // [kernel][M >= WL_ROWS_SMALL_M]
#define WL_GEOS_LN1_FWD(X) X(1, 4) X(2, 2) X(4, 1)
#define WL_GEOS(X) X(1, 4) X(2, 2)   // add + LN forward, LN backward, LN1 backward
#define WL_GEOS_LORA(X) X(1, 4)
static_assert(WL_LN1_ROWS == 4, "WL_GEOS_LORA holds (1, WL_LN1_ROWS)");

static WlGeo g_wl_force = {0, 0};   // rdx_wl_rows_override (measurement and tests): w = 0 leaves the table in charge

static WlGeo wl_geo(int kernel, int64_t M, bool lora) {
  if (g_wl_force.w) return g_wl_force;
  return lora ? WlGeo{1, WL_LN1_ROWS} : kWlGeo[kernel][M >= WL_ROWS_SMALL_M ? 1 : 0];
}
static bool wl_geo_built(WlGeo g) {
#define WL_X(Wv, Rv) if (g.w == Wv && g.r == Rv) return true;
  WL_GEOS_LN1_FWD(WL_X)   // the union of the lists
#undef WL_X
  return false;
}

template <typename K, typename A>
static int wl_launch(K kernel, WlGeo g, const A& a, int64_t M, void* stream) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((M + g.r - 1) / g.r)), dim3(g.w * g.r * RDX_WAVE), 0, as_stream(stream), a);
  RDX_LAUNCH_CHECK();
  return 0;
}

static int ln1_fwd_launch(const Ln1Args& a, bool lora, void* stream) {
  const WlGeo g = wl_geo(WL_K_LN1_FWD, a.M, lora);
#define WL_X(Wv, Rv) \
  if (!lora && g.w == Wv && g.r == Rv) return wl_launch(wl_ln1_fwd_kernel<false, Wv, Rv>, g, a, a.M, stream);
  WL_GEOS_LN1_FWD(WL_X)
#undef WL_X
#define WL_X(Wv, Rv) \
  if (lora && g.w == Wv && g.r == Rv) return wl_launch(wl_ln1_fwd_kernel<true, Wv, Rv>, g, a, a.M, stream);
  WL_GEOS_LORA(WL_X)
#undef WL_X
  return RDX_EINVAL;
}



extern "C" {

int rdx_wl_ln1_fwd(const float* h, const float* gamma, const float* beta, float eps, const float* wg, const float* bg,
                   const float* gconst, const void* lora_aq, const void* lora_av, int r, const int64_t* seed_dev,
                   int salt_q, int salt_v, float p_lora, void* x1, int64_t ldx, float* gate, float* mean, float* rstd, int64_t M, int E,
                   void* stream) {
  RDX_REQUIRE(h && gamma && beta && wg && bg && gconst && x1 && gate && mean && rstd && M > 0);
  const bool lora = lora_aq != nullptr;
  RDX_REQUIRE(E == WL_E && (!lora || (2 * r == WL_R2 && lora_av)) && ldx >= E + (lora ? 2 * r : 0));
  RDX_REQUIRE(!lora || ((((uintptr_t)lora_aq | (uintptr_t)lora_av) & 15) == 0));
  RDX_REQUIRE(ldx % 8 == 0);
  Ln1Args a{h, gamma, beta, eps, GateW{wg, bg, gconst}, reinterpret_cast<const hst*>(lora_aq),
            reinterpret_cast<const hst*>(lora_av), mk_drop(seed_dev, salt_q, p_lora),
            mk_drop(seed_dev, salt_v, p_lora), reinterpret_cast<hst*>(x1), ldx, gate, mean, rstd, M,
            nullptr, nullptr, mk_drop(nullptr, 0, 0.f), nullptr};
  return ln1_fwd_launch(a, lora, stream);
}

int rdx_wl_res_ln1_fwd(const float* h2, const void* delta, int salt_res, float p_res, float* hout,
                       const float* gamma, const float* beta, float eps, const float* wg, const float* bg,
                       const float* gconst, const void* lora_aq, const void* lora_av, int r, const int64_t* seed_dev,
                       int salt_q, int salt_v, float p_lora, void* x1, int64_t ldx, float* gate, float* mean,
                       float* rstd, int64_t M, int E, void* stream) {
  RDX_REQUIRE(h2 && delta && hout && gamma && beta && wg && bg && gconst && x1 && gate && mean && rstd && M > 0);
  const bool lora = lora_aq != nullptr;
  RDX_REQUIRE(E == WL_E && (!lora || (2 * r == WL_R2 && lora_av)) && ldx >= E + (lora ? 2 * r : 0));
  RDX_REQUIRE(!lora || ((((uintptr_t)lora_aq | (uintptr_t)lora_av) & 15) == 0));
  RDX_REQUIRE(ldx % 8 == 0);
  Ln1Args a{nullptr, gamma, beta, eps, GateW{wg, bg, gconst}, reinterpret_cast<const hst*>(lora_aq),
            reinterpret_cast<const hst*>(lora_av), mk_drop(seed_dev, salt_q, p_lora),
            mk_drop(seed_dev, salt_v, p_lora), reinterpret_cast<hst*>(x1), ldx, gate, mean, rstd, M,
            h2, reinterpret_cast<const hst*>(delta), mk_drop(seed_dev, salt_res, p_res), hout};
  return ln1_fwd_launch(a, lora, stream);
}

int rdx_wl_add_ln_fwd(const float* h, const void* delta, const int64_t* seed_dev, int salt, float p, float* h2,
                      const float* gamma, const float* beta, float eps, void* x, float* mean, float* rstd, int64_t M,
                      int E, void* stream) {
  RDX_REQUIRE(h && delta && h2 && gamma && beta && x && mean && rstd && M > 0 && E == WL_E);
  AddLnArgs a{h, reinterpret_cast<const hst*>(delta), mk_drop(seed_dev, salt, p), h2, gamma, beta, eps,
              reinterpret_cast<hst*>(x), mean, rstd, M};
  const WlGeo g = wl_geo(WL_K_ADD_LN, M, false);
#define WL_X(Wv, Rv) if (g.w == Wv && g.r == Rv) return wl_launch(wl_add_ln_fwd_kernel<Wv, Rv>, g, a, M, stream);
  WL_GEOS(WL_X)
#undef WL_X
  return RDX_EINVAL;
}

int rdx_wl_rows_override(int waves, int rows) {
  if (waves == 0 && rows == 0) {
    g_wl_force = WlGeo{0, 0};
    return 0;
  }
  RDX_REQUIRE(wl_geo_built(WlGeo{waves, rows}));
  g_wl_force = WlGeo{waves, rows};
  return 0;
}

int rdx_wl_rows_policy(int kernel, int64_t M, int lora, int* waves, int* rows) {
  RDX_REQUIRE(kernel >= 0 && kernel < 4 && M > 0 && waves && rows);
  const WlGeo g = wl_geo(kernel, M, lora != 0);
  *waves = g.w;
  *rows = g.r;
  return 0;
}

int rdx_wl_residual(const float* h, const void* delta, const int64_t* seed_dev, int salt, float p, float* out,
                    int64_t n, void* stream) {
  RDX_REQUIRE(h && delta && out && n > 0 && n % 8 == 0);
  hipLaunchKernelGGL(wl_residual_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, as_stream(stream), h,
                     reinterpret_cast<const hst*>(delta), mk_drop(seed_dev, salt, p), out, n);
  RDX_LAUNCH_CHECK();
  return 0;
}

int rdx_wl_dropout_bwd(const float* g, const int64_t* seed_dev, int salt, float p, void* out, int64_t n,
                       void* stream) {
  RDX_REQUIRE(g && out && n > 0 && n % 8 == 0);
  hipLaunchKernelGGL(wl_dropout_bwd_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, as_stream(stream), g,
                     mk_drop(seed_dev, salt, p), reinterpret_cast<hst*>(out), n);
  RDX_LAUNCH_CHECK();
  return 0;
}

int rdx_wl_gelu(int mode, const void* u, const void* dy, void* out, int64_t n, void* stream) {
  RDX_REQUIRE(u && out && n > 0 && n % 8 == 0 && (mode == 0 || (mode == 1 && dy)));
  const auto* U = reinterpret_cast<const hst*>(u);
  const auto* DY = reinterpret_cast<const hst*>(dy);
  auto* O = reinterpret_cast<hst*>(out);
  const dim3 grid((unsigned)((n / 8 + 255) / 256));
  if (mode == 0)
    hipLaunchKernelGGL(wl_gelu_kernel<0>, grid, dim3(256), 0, as_stream(stream), U, DY, O, n);
  else
    hipLaunchKernelGGL(wl_gelu_kernel<1>, grid, dim3(256), 0, as_stream(stream), U, DY, O, n);
  RDX_LAUNCH_CHECK();
  return 0;
}

int rdx_wl_ln_bwd(const void* dx, int64_t ldd, const float* h, const float* mean, const float* rstd,
                  const float* gamma, const float* dres, float* dh, const int64_t* seed_dev, int salt, float p,
                  void* ddrop, int64_t M, int E, void* stream) {
  RDX_REQUIRE(dx && h && mean && rstd && gamma && dh && M > 0 && E == WL_E && ldd >= E && ldd % 8 == 0);
  LnBwdArgs a{reinterpret_cast<const hst*>(dx), ldd, h, mean, rstd, gamma, dres, dh,
              mk_drop(seed_dev, salt, p), reinterpret_cast<hst*>(ddrop), M};
  const WlGeo g = wl_geo(WL_K_LN_BWD, M, false);
#define WL_X(Wv, Rv) if (g.w == Wv && g.r == Rv) return wl_launch(wl_ln_bwd_kernel<Wv, Rv>, g, a, M, stream);
  WL_GEOS(WL_X)
#undef WL_X
  return RDX_EINVAL;
}

int rdx_wl_ln1_bwd_ex(const void* dx1, int64_t ldx, const float* dgate, const float* h, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, const float* wg, const float* bg,
                      const float* gconst, const void* lora_aq, const void* lora_av, int r, const int64_t* seed_dev,
                      int salt_q, int salt_v, float p_lora, const float* dres, float* dh, void* xd,
                      const float* state_grad, const float* state_weight, int salt_prev, float p_prev,
                      void* ddrop_prev, int64_t M, int E, void* stream) {
  RDX_REQUIRE(dx1 && dgate && h && mean && rstd && gamma && beta && wg && bg && gconst && dres && dh && M > 0);
  RDX_REQUIRE((state_grad == nullptr) == (state_weight == nullptr));
  const bool lora = lora_aq != nullptr;
  RDX_REQUIRE(E == WL_E && ldx % 8 == 0 && (!lora || (2 * r == WL_R2 && lora_av && ldx >= E + 2 * r)));
  RDX_REQUIRE(!lora || ((((uintptr_t)lora_aq | (uintptr_t)lora_av) & 15) == 0));
  Ln1BwdArgs a{reinterpret_cast<const hst*>(dx1), ldx, dgate, h, mean, rstd, gamma, beta,
               GateW{wg, bg, gconst}, reinterpret_cast<const hst*>(lora_aq), reinterpret_cast<const hst*>(lora_av),
               mk_drop(seed_dev, salt_q, p_lora), mk_drop(seed_dev, salt_v, p_lora),
               dres, dh, reinterpret_cast<hst*>(xd), M, state_grad, state_weight,
               mk_drop(seed_dev, salt_prev, p_prev), reinterpret_cast<hst*>(ddrop_prev)};
  const WlGeo g = wl_geo(WL_K_LN1_BWD, M, lora);
#define WL_X(Wv, Rv) \
  if (!lora && g.w == Wv && g.r == Rv) return wl_launch(wl_ln1_bwd_kernel<false, Wv, Rv>, g, a, M, stream);
  WL_GEOS(WL_X)
#undef WL_X
#define WL_X(Wv, Rv) \
  if (lora && g.w == Wv && g.r == Rv) return wl_launch(wl_ln1_bwd_kernel<true, Wv, Rv>, g, a, M, stream);
  WL_GEOS_LORA(WL_X)
#undef WL_X
  return RDX_EINVAL;
}

int rdx_wl_ln1_bwd(const void* dx1, int64_t ldx, const float* dgate, const float* h, const float* mean,
                   const float* rstd, const float* gamma, const float* beta, const float* wg, const float* bg,
                   const float* gconst, const void* lora_aq, const void* lora_av, int r, const int64_t* seed_dev,
                   int salt_q, int salt_v, float p_lora, const float* dres, float* dh, void* xd, int64_t M, int E,
                   void* stream) {
  return rdx_wl_ln1_bwd_ex(dx1, ldx, dgate, h, mean, rstd, gamma, beta, wg, bg, gconst, lora_aq, lora_av, r, seed_dev,
                           salt_q, salt_v, p_lora, dres, dh, xd, nullptr, nullptr, 0, 0.f, nullptr, M, E, stream);
}

int rdx_wl_lora_grad(const void* dqkv, int64_t ldq, const void* x1, int64_t ldx, const void* dx1, int64_t ldd,
                     const int64_t* seed_dev, int salt_q, int salt_v, float p_lora, float scale, float* daq,
                     float* dbq, float* dav, float* dbv, int64_t M, int E, int r, void* stream) {
  RDX_REQUIRE(dqkv && x1 && dx1 && daq && dbq && dav && dbv && M > 0 && E == WL_E && 2 * r == WL_R2);
  RDX_REQUIRE(ldq >= 3 * (int64_t)E && ldx >= E + 2 * r && ldd >= E + 2 * r);
  RDX_REQUIRE(ldq % 2 == 0 && ldx % 2 == 0 && ((uintptr_t)dqkv & 3) == 0 && ((uintptr_t)x1 & 3) == 0);
  LoraGradArgs a{reinterpret_cast<const hst*>(dqkv), ldq, reinterpret_cast<const hst*>(x1), ldx,
                 reinterpret_cast<const hst*>(dx1), ldd, mk_drop(seed_dev, salt_q, p_lora),
                 mk_drop(seed_dev, salt_v, p_lora), scale, daq, dbq, dav, dbv, M};
  // 32-row chunks; a block walks nch of them so the 4096 fp32 atomics it ends with are amortised over
  // >= 64 rows once M allows (atomics run at ~1.3 TB/s of added bytes chip-wide), keeping >= 400 blocks.
  const int64_t nchunk = (M + 31) / 32;
  const int nch = (int)std::max<int64_t>(1, std::min<int64_t>(8, M / 2048));
  const dim3 grid(WL_E / WL_LG_COLS, (unsigned)((nchunk + nch - 1) / nch));
  hipLaunchKernelGGL(wl_lora_grad_kernel<8>, grid, dim3(256), 0, as_stream(stream), a, nch);
  RDX_LAUNCH_CHECK();
  return 0;
}

int rdx_wl_lora_pack(int nl, const float* const* bq, const float* const* bv, void* const* wext, int64_t ldw, int r,
                     float scale, int E, void* stream) {
  RDX_REQUIRE(nl > 0 && bq && bv && wext && E == WL_E && r > 0 && ldw >= E + 2 * r);
  const int64_t n = 2 * (int64_t)E * r;
  hipLaunchKernelGGL(wl_lora_pack_kernel, dim3((unsigned)((n + 255) / 256), nl), dim3(256), 0, as_stream(stream), nl,
                     bq, bv, reinterpret_cast<hst* const*>(wext), ldw, r, scale);
  RDX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
