// Silence trimming for whole-recording scoring (radhip/recordings.py states the rule): between the conversion
// (csrc/ingest.hip) and the window gather (csrc/recwin.hip). Three kernels over the packed recordings of one chunk:
// the energy of every 320-sample frame, the per-recording plan (which frames stay and where they land) and the
// compaction. fp32, no atomics, every reduction in a fixed order: two launches give the same bits. The kernels use
// no 16-bit storage, so they are the same in both libraries.
#include "common.h"

namespace rdx {

constexpr int TRIM_F = RDX_TRIM_FRAME;   // samples per frame
// One launch covers up to TR_MAX recordings, whose places travel as kernel arguments (as the window table of
// csrc/recwin.hip does): no index table is read from memory.
constexpr int TR_MAX = 64;
struct TrimRecs {
  int64_t base[TR_MAX];    // element offset of the recording in sig
  int64_t len[TR_MAX];     // its samples
  int64_t foff[TR_MAX];    // offset of its frame 0 in e / dst
  int64_t obase[TR_MAX];   // element offset of the trimmed recording in out (compaction only)
  int32_t cum[TR_MAX + 1]; // frames of the recordings before it in this launch; cum[nrec] = all frames of the launch
};
struct TrimPlanRecs {
  int64_t foff[TR_MAX];
  int64_t len[TR_MAX];
  int32_t nf[TR_MAX];
};

// The recording that owns frame w of the launch: the last j with cum[j] <= w (w is the same in every lane, so the
// look-ups are scalar loads from the argument segment).
#define RDX_TRIM_FIND(T, nrec, w, j)              \
  int j = 0;                                      \
  for (int hi_ = (nrec); hi_ - j > 1;) {          \
    const int mid_ = (j + hi_) >> 1;              \
    if ((w) >= (T).cum[mid_]) j = mid_;           \
    else hi_ = mid_;                              \
  }

// ------------------------------------------------------------------------------- frame energy ----
// One wave per frame. Lane l squares samples l, l + 64, ..., l + 256 of the frame (each load of the wave is 256
// contiguous bytes) into one fmaf chain, and the 64 partial sums meet in wave_sum's fixed order. A partial last frame
// reads only the samples it has and is divided by their count.
__global__ __launch_bounds__(256) void trim_energy_kernel(const float* __restrict__ sig, TrimRecs T, int nrec,
                                                          float* __restrict__ e) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (w >= T.cum[nrec]) return;       // wave-uniform: wave_sum below runs with whole waves
  RDX_TRIM_FIND(T, nrec, w, j);
  const int f = w - T.cum[j];
  const int64_t s0 = (int64_t)f * TRIM_F;
  const int64_t left = T.len[j] - s0;
  const int cnt = left < TRIM_F ? (int)left : TRIM_F;
  const float* __restrict__ p = sig + T.base[j] + s0;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < TRIM_F / 64; ++k) {
    const int i = lane + 64 * k;
    const float x = i < cnt ? p[i] : 0.f;
    acc = fmaf(x, x, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) e[T.foff[j] + f] = acc / (float)cnt;
}

// ---------------------------------------------------------------------------------------- plan ----
// One workgroup per recording walks its frames in tiles of PL_TILE, thread t owning PL_ITEMS consecutive frames of a
// tile, three times:
//   1. the maximum of e (registers, then LDS across the four waves);
//   2. active[f] = e[f] > 0 && e[f] >= peak * ratio, and its inclusive prefix count P[f] into scratch. The count of
//      the tiles before lives in LDS (s_cnt);
//   3. keep[f] from two look-ups in P ("gaps": an active frame in [f - pad, f + pad]; "ends": one at or before
//      f + pad and one at or after f - pad), then the exclusive scan of the kept frames' lengths, whose carry lives
//      in LDS (s_len): dst[f] = the frame's offset in the trimmed recording, or -1.
// A recording without an active frame keeps everything. The frame counts are int32, the lengths int64.
constexpr int PL_THREADS = 256, PL_ITEMS = 4, PL_TILE = PL_THREADS * PL_ITEMS;

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// carry + (sum of v over the threads before this one); then *carry += the sum over the workgroup. Every thread of the
// workgroup calls it. The second barrier keeps wsum and *carry from being rewritten while a slower wave reads them.
template <typename C>
__device__ __forceinline__ C block_excl_scan(int v, int* wsum, C* carry) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  const C base = *carry;
  int before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < PL_THREADS / 64; ++k) {
    const int s = wsum[k];
    before += k < wave ? s : 0;
    total += s;
  }
  __syncthreads();
  if (threadIdx.x == 0) *carry = base + total;
  return base + (C)(before + incl - v);
}

__global__ __launch_bounds__(PL_THREADS) void trim_plan_kernel(const float* __restrict__ e, TrimPlanRecs T,
                                                               float ratio, int pad, int mode, int32_t* scratch,
                                                               int64_t* __restrict__ dst,
                                                               int64_t* __restrict__ kept_len) {
  __shared__ float s_max[PL_THREADS / 64];
  __shared__ int s_wsum[PL_THREADS / 64];
  __shared__ int s_cnt;
  __shared__ int64_t s_len;
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nf = T.nf[j];
  const int64_t n = T.len[j];
  const float* __restrict__ er = e + T.foff[j];
  int32_t* P = scratch + T.foff[j];
  int64_t* __restrict__ d = dst + T.foff[j];
  pad = pad < nf ? pad : nf;          // a wider reach changes nothing, and f + pad stays inside int32

  // 1. peak (energies are >= 0)
  float m = 0.f;
  for (int f = tid; f < nf; f += PL_THREADS) m = fmaxf(m, er[f]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) s_max[wave] = m;
  if (tid == 0) {
    s_cnt = 0;
    s_len = 0;
  }
  __syncthreads();
  float peak = s_max[0];
#pragma unroll
  for (int k = 1; k < PL_THREADS / 64; ++k) peak = fmaxf(peak, s_max[k]);
  const float thr = peak * ratio;

  // 2. active flags and their inclusive prefix count
  for (int t0 = 0; t0 < nf; t0 += PL_TILE) {
    const int f0 = t0 + tid * PL_ITEMS;
    int a[PL_ITEMS], v = 0;
#pragma unroll
    for (int k = 0; k < PL_ITEMS; ++k) {
      const float x = f0 + k < nf ? er[f0 + k] : 0.f;
      a[k] = (x > 0.f && x >= thr) ? 1 : 0;
      v += a[k];
    }
    int run = block_excl_scan<int>(v, s_wsum, &s_cnt);
#pragma unroll
    for (int k = 0; k < PL_ITEMS; ++k) {
      run += a[k];
      if (f0 + k < nf) P[f0 + k] = run;
    }
  }
  __syncthreads();    // s_cnt is final, and every P[f] of this recording is visible to the workgroup
  const int nact = s_cnt;

  // 3. kept frames and the exclusive scan of their lengths
  for (int t0 = 0; t0 < nf; t0 += PL_TILE) {
    const int f0 = t0 + tid * PL_ITEMS;
    int len[PL_ITEMS], v = 0;
#pragma unroll
    for (int k = 0; k < PL_ITEMS; ++k) {
      const int f = f0 + k;
      len[k] = 0;
      if (f < nf) {
        bool keep = true;
        if (nact > 0) {
          const int hi = f + pad < nf - 1 ? f + pad : nf - 1, lo = f - pad - 1;
          const int ph = P[hi], pl = lo >= 0 ? P[lo] : 0;
          keep = mode == RDX_TRIM_GAPS ? ph - pl > 0 : (ph > 0 && nact - pl > 0);
        }
        const int64_t left = n - (int64_t)f * TRIM_F;
        len[k] = keep ? (left < TRIM_F ? (int)left : TRIM_F) : 0;
      }
      v += len[k];
    }
    int64_t run = block_excl_scan<int64_t>(v, s_wsum, &s_len);
#pragma unroll
    for (int k = 0; k < PL_ITEMS; ++k) {
      if (f0 + k < nf) d[f0 + k] = len[k] > 0 ? run : -1;   // a frame that exists has at least one sample
      run += len[k];
    }
  }
  __syncthreads();
  if (tid == 0) kept_len[j] = s_len;
}

// ------------------------------------------------------------------------------------- compact ----
// One wave per source frame: a dropped frame returns at once, a kept one is copied to its place, lane l moving
// samples l, l + 64, ... as the energy pass read them.
__global__ __launch_bounds__(256) void trim_compact_kernel(const float* __restrict__ sig, TrimRecs T, int nrec,
                                                           const int64_t* __restrict__ dst, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (w >= T.cum[nrec]) return;
  RDX_TRIM_FIND(T, nrec, w, j);
  const int f = w - T.cum[j];
  const int64_t to = dst[T.foff[j] + f];
  if (to < 0) return;
  const int64_t s0 = (int64_t)f * TRIM_F;
  const int64_t left = T.len[j] - s0;
  const int cnt = left < TRIM_F ? (int)left : TRIM_F;
  const float* __restrict__ p = sig + T.base[j] + s0;
  float* __restrict__ q = out + T.obase[j] + to;
#pragma unroll
  for (int k = 0; k < TRIM_F / 64; ++k) {
    const int i = lane + 64 * k;
    if (i < cnt) q[i] = p[i];
  }
}

static inline int64_t trim_frames(int64_t len) { return (len + TRIM_F - 1) / TRIM_F; }

// The per-frame launches of the energy pass and of the compaction: recordings r0 .. r0 + nrec - 1 per launch.
template <typename Launch>
static int trim_for_each_batch(const int64_t* offs, const int64_t* lens, const int64_t* foffs, const int64_t* new_offs,
                               int R, Launch launch) {
  for (int r0 = 0; r0 < R;) {
    TrimRecs T{};
    int nrec = 0;
    int64_t frames = 0;
    while (r0 + nrec < R && nrec < TR_MAX && frames + trim_frames(lens[r0 + nrec]) <= INT32_MAX - 4) {
      const int r = r0 + nrec;
      T.base[nrec] = offs[r];
      T.len[nrec] = lens[r];
      T.foff[nrec] = foffs[r];
      T.obase[nrec] = new_offs ? new_offs[r] : 0;
      T.cum[nrec] = (int32_t)frames;
      frames += trim_frames(lens[r]);
      ++nrec;
    }
    if (nrec == 0) return RDX_EUNSUPPORTED;   // one recording of 2^31 frames or more
    T.cum[nrec] = (int32_t)frames;
    launch(T, nrec, dim3((unsigned)((frames + 3) / 4)));
    RDX_LAUNCH_CHECK();
    r0 += nrec;
  }
  return RDX_OK;
}

}  // namespace rdx

using namespace rdx;

extern "C" int rdx_trim_energy(const float* sig, const int64_t* offs, const int64_t* lens, const int64_t* foffs, int R,
                               float* e, void* stream) {
  RDX_REQUIRE(sig && offs && lens && foffs && e && R > 0);
  for (int r = 0; r < R; ++r) RDX_REQUIRE(offs[r] >= 0 && lens[r] > 0 && foffs[r] >= 0);
  return trim_for_each_batch(offs, lens, foffs, nullptr, R, [&](const TrimRecs& T, int nrec, dim3 grid) {
    hipLaunchKernelGGL(trim_energy_kernel, grid, dim3(256), 0, as_stream(stream), sig, T, nrec, e);
  });
}

extern "C" int rdx_trim_plan(const float* e, const int64_t* foffs, const int64_t* nframes, const int64_t* lens, int R,
                             float ratio, int pad, int mode, int32_t* scratch, int64_t* dst, int64_t* kept_len,
                             void* stream) {
  RDX_REQUIRE(e && foffs && nframes && lens && scratch && dst && kept_len && R > 0);
  RDX_REQUIRE(ratio > 0.f && ratio <= 1.f && pad >= 0);    // a NaN ratio fails the first comparison
  RDX_REQUIRE(mode == RDX_TRIM_ENDS || mode == RDX_TRIM_GAPS);
  for (int r = 0; r < R; ++r) {
    RDX_REQUIRE(foffs[r] >= 0 && lens[r] > 0 && nframes[r] == trim_frames(lens[r]));
    if (nframes[r] > INT32_MAX - PL_TILE) return RDX_EUNSUPPORTED;
  }
  for (int r0 = 0; r0 < R; r0 += TR_MAX) {
    const int nrec = (R - r0) < TR_MAX ? (R - r0) : TR_MAX;
    TrimPlanRecs T{};
    for (int j = 0; j < nrec; ++j) {
      T.foff[j] = foffs[r0 + j];
      T.len[j] = lens[r0 + j];
      T.nf[j] = (int32_t)nframes[r0 + j];
    }
    hipLaunchKernelGGL(trim_plan_kernel, dim3((unsigned)nrec), dim3(PL_THREADS), 0, as_stream(stream), e, T, ratio,
                       pad, mode, scratch, dst, kept_len + r0);
    RDX_LAUNCH_CHECK();
  }
  return RDX_OK;
}

extern "C" int rdx_trim_compact(const float* sig, const int64_t* offs, const int64_t* lens, const int64_t* foffs,
                                const int64_t* dst, const int64_t* new_offs, int R, float* out, void* stream) {
  RDX_REQUIRE(sig && offs && lens && foffs && dst && new_offs && out && R > 0);
  for (int r = 0; r < R; ++r) RDX_REQUIRE(offs[r] >= 0 && lens[r] > 0 && foffs[r] >= 0 && new_offs[r] >= 0);
  return trim_for_each_batch(offs, lens, foffs, new_offs, R, [&](const TrimRecs& T, int nrec, dim3 grid) {
    hipLaunchKernelGGL(trim_compact_kernel, grid, dim3(256), 0, as_stream(stream), sig, T, nrec, dst, out);
  });
}
