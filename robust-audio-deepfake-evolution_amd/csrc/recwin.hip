// Whole-recording scoring (radhip/recordings.py): the window gather that cuts a ragged set of packed recordings into
// model inputs, and the segmented reduction that turns window scores back into one record per recording. Both are
// small next to the model forward; they are written to be exact and to give the same bits on every launch.
#include "common.h"

namespace rdx {

// ------------------------------------------------------------------------------ window gather ----
// One launch covers up to WG_MAX windows, whose sources travel as kernel arguments (the host resolves
// offsets[rec[w]] + start[w] once, so the kernel reads no index table from memory).
constexpr int WG_MAX = 64;
struct WinTable {
  int64_t base[WG_MAX];   // element offset of the window's first source sample (the recording's start when tiled)
  int32_t tile[WG_MAX];   // the recording's length when it is tiled (len <= win), else 0
};

// A thread owns four consecutive output samples and stores them as one dwordx4 (win % 4 == 0 and a 16-byte aligned
// `out` keep every such group inside one row and aligned). The source of a window starts at any element offset:
// the loads are one dwordx4 where the window's source address happens to be 16-byte aligned and four dwords
// otherwise, so an odd offset costs bandwidth, never correctness.
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ sig, WinTable T, int win,
                                                            float* __restrict__ out) {
  const int w = blockIdx.y;
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= win) return;
  const float* __restrict__ src = sig + T.base[w];
  const uint32_t L = (uint32_t)T.tile[w];
  rdx_f32x4 v;
  if (L == 0) {
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      v = *reinterpret_cast<const rdx_f32x4*>(src + i);
    } else {
      v[0] = src[i];
      v[1] = src[i + 1];
      v[2] = src[i + 2];
      v[3] = src[i + 3];
    }
  } else {
    uint32_t m = (uint32_t)i % L;     // out[i] = x[i mod len]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = src[m];
      m = (m + 1 == L) ? 0 : m + 1;
    }
  }
  *reinterpret_cast<rdx_f32x4*>(out + (int64_t)w * win + i) = v;
}

// ----------------------------------------------------------------------------- segment reduce ----
// One wave per segment. Lane l folds scores seg[r] + l, + l + 64, ... in index order, then the 64 partial results
// meet in a fixed butterfly: the bits depend on the segment alone, not on the grid or on which wave ran it.
// The sum is kept in fp32 as an unevaluated pair hi + lo (two_sum, common.h): every addition's rounding error
// goes to lo, so hi + lo misses the true sum by O(n u^2) and the mean is rounded once, at the division. A plain
// fp32 chain could not promise (n - 1) u max|s| at n = 3 (two additions and the division: up to 8/3 u max|s|).
__global__ __launch_bounds__(256) void segment_reduce_kernel(const float* __restrict__ scores,
                                                             const int64_t* __restrict__ seg, int nseg,
                                                             float* __restrict__ out_mean, float* __restrict__ out_min,
                                                             float* __restrict__ out_max,
                                                             int64_t* __restrict__ out_argmin) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nseg) return;      // wave-uniform: the lane-crossing steps below run with whole waves
  const int64_t s0 = seg[r], n = seg[r + 1] - s0;
  float sum = 0.f, err = 0.f, lo = INFINITY, hi = -INFINITY;
  int64_t at = INT64_MAX;
  for (int64_t k = lane; k < n; k += 64) {
    const float v = scores[s0 + k];
    two_sum(sum, err, v);
    if (v < lo) { lo = v; at = k; }   // strict: a lane keeps the first of equal minima
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float sum2 = __shfl_xor(sum, o, 64), err2 = __shfl_xor(err, o, 64);
    two_sum(sum, err, sum2);
    err += err2;
    const float lo2 = __shfl_xor(lo, o, 64);
    const int64_t at2 = __shfl_xor(at, o, 64);
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    if (lo2 < lo || (lo2 == lo && at2 < at)) { lo = lo2; at = at2; }
  }
  if (lane == 0) {
    out_mean[r] = (float)(((double)sum + (double)err) / (double)n);
    out_min[r] = lo;
    out_max[r] = hi;
    out_argmin[r] = at;
  }
}

}  // namespace rdx

using namespace rdx;

extern "C" int rdx_window_gather(const float* sig, const int64_t* offsets, const int64_t* lens, const int64_t* rec,
                                 const int64_t* start, int nwin, int64_t win, float* out, void* stream) {
  RDX_REQUIRE(sig && offsets && lens && rec && start && out && nwin > 0 && win > 0);
  RDX_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  if (win % 4 != 0 || win > INT32_MAX - 1024) return RDX_EUNSUPPORTED;
  for (int w = 0; w < nwin; ++w) {
    RDX_REQUIRE(rec[w] >= 0);
    const int64_t L = lens[rec[w]];
    RDX_REQUIRE(L > 0 && offsets[rec[w]] >= 0 && start[w] >= 0);
    RDX_REQUIRE(L <= win ? start[w] == 0 : start[w] + win <= L);
  }
  const dim3 block(256);
  for (int w0 = 0; w0 < nwin; w0 += WG_MAX) {
    const int nw = (nwin - w0) < WG_MAX ? (nwin - w0) : WG_MAX;
    WinTable T{};
    for (int j = 0; j < nw; ++j) {
      const int64_t r = rec[w0 + j];
      const bool tiled = lens[r] <= win;
      T.base[j] = offsets[r] + (tiled ? 0 : start[w0 + j]);
      T.tile[j] = tiled ? (int32_t)lens[r] : 0;
    }
    const dim3 grid((unsigned)((win / 4 + 255) / 256), (unsigned)nw);
    hipLaunchKernelGGL(window_gather_kernel, grid, block, 0, as_stream(stream), sig, T, (int)win,
                       out + (int64_t)w0 * win);
    RDX_LAUNCH_CHECK();
  }
  return RDX_OK;
}

extern "C" int rdx_segment_reduce(const float* scores, const int64_t* seg, int nseg, float* out_mean, float* out_min,
                                  float* out_max, int64_t* out_argmin, void* stream) {
  RDX_REQUIRE(scores && seg && out_mean && out_min && out_max && out_argmin && nseg > 0);
  hipLaunchKernelGGL(segment_reduce_kernel, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, as_stream(stream), scores,
                     seg, nseg, out_mean, out_min, out_max, out_argmin);
  RDX_LAUNCH_CHECK();
  return RDX_OK;
}
