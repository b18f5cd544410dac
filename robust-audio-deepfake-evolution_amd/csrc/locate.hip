// Locating the spoofed parts of a recording (radhip/recordings.py states the rule): after the window scores exist.
// Three kernels over the recordings of one scoring pass: the per-frame score track (the overlapping windows' scores
// spread over the 320-sample frames they cover), the flagged segments of every track (threshold, bridge, discard) and
// the statistics of every segment. fp32, no atomics, every operation in a fixed order: two launches give the same
// bits. The kernels use no 16-bit storage, so they are the same in both libraries.
#include "common.h"

namespace rdx {

constexpr int LC_F = RDX_TRIM_FRAME;   // samples per frame
// One launch covers up to LC_MAX recordings, whose places travel as kernel arguments (as in csrc/trim.hip).
constexpr int LC_MAX = 64;
struct TrackRecs {
  int64_t m[LC_MAX];        // samples of the scored signal
  int64_t foff[LC_MAX];     // offset of its frame 0 in t
  int32_t cum[LC_MAX + 1];  // frames of the recordings before it in this launch; cum[nrec] = all of them
};
struct SegRecs {
  int64_t foff[LC_MAX];
  int32_t nf[LC_MAX];
};
struct StatRecs {
  int64_t foff[LC_MAX];
  int32_t cum[LC_MAX + 1];  // slots (ceil(nf / 2)) of the recordings before it in this launch
};

// The recording that owns item w of the launch: the last j with cum[j] <= w.
#define RDX_LOC_FIND(T, nrec, w, j)               \
  int j = 0;                                      \
  for (int hi_ = (nrec); hi_ - j > 1;) {          \
    const int mid_ = (j + hi_) >> 1;              \
    if ((w) >= (T).cum[mid_]) j = mid_;           \
    else hi_ = mid_;                              \
  }

// -------------------------------------------------------------------------------------- track ----
// One thread per frame. The windows that cover the frame's span [lo, hi) follow from the window rule in closed
// form: the regular windows k * hop with k * hop < hi and k * hop + win > lo, clipped to 0 .. n - 2, and the last
// window at m - win. Their overlaps with the span are integers in 1 .. 320, exact in fp32; the weighted sum is one
// fmaf chain over k ascending with the last window last, the integer weight sum is converted once and there is one
// division. n comes from seg, so every read stays inside the recording's own scores. O(win / hop) windows per frame.
__global__ __launch_bounds__(256) void track_overlap_kernel(const float* __restrict__ scores,
                                                            const int64_t* __restrict__ seg, TrackRecs T, int nrec,
                                                            int64_t hop, int64_t win, float* __restrict__ t) {
  const int w = (int)(blockIdx.x * 256 + threadIdx.x);
  if (w >= T.cum[nrec]) return;
  RDX_LOC_FIND(T, nrec, w, j);
  const int f = w - T.cum[j];
  const int64_t m = T.m[j];
  const int64_t s0 = seg[j], n = seg[j + 1] - s0;
  const float* __restrict__ s = scores + s0;
  float out;
  if (m <= win) {
    out = s[0];
  } else {
    const int64_t lo = (int64_t)f * LC_F;
    const int64_t hi = lo + LC_F < m ? lo + LC_F : m;
    int64_t k = lo >= win ? (lo - win) / hop + 1 : 0;
    int64_t k_hi = (hi - 1) / hop;
    if (k_hi > n - 2) k_hi = n - 2;
    float acc = 0.f;
    int64_t wsum = 0;
    for (; k <= k_hi; ++k) {
      const int64_t a = k * hop, e = a + win;
      const int ov = (int)((hi < e ? hi : e) - (lo > a ? lo : a));
      acc = fmaf((float)ov, s[k], acc);
      wsum += ov;
    }
    const int64_t a = m - win;
    const int ov = (int)(hi - (lo > a ? lo : a));
    if (ov > 0) {
      acc = fmaf((float)ov, s[n > 0 ? n - 1 : 0], acc);
      wsum += ov;
    }
    out = acc / (float)wsum;
  }
  t[T.foff[j] + f] = out;
}

// ----------------------------------------------------------------------------------- segments ----
// One workgroup per recording walks the positions 0 .. nf (the frames and one position past the last) in tiles of
// SG_TILE, thread t owning SG_ITEMS consecutive positions of a tile. Whether a run of flagged and bridged frames is
// over is known only at the next run's first frame, or at the recording's end, so that position reports the run
// before it, and one forward walk with three scans per tile suffices (no backward scan and no scratch memory):
//   1. exclusive max-scan of (flag[f] ? f : -1): b = the last flagged frame before f. Frame f starts a run when it
//      is flagged and b < 0 or the gap f - b - 1 is wider than merge (a gap touching frame 0 is never bridged);
//   2. exclusive max-scan of (starts[f] ? f : -1): a = the first frame of the run that ends at b;
//   3. position f reports [a, b] when it starts a run or is nf, b >= 0 and b - a + 1 >= min_frames; the exclusive
//      count of the reports is the segment's ordinal, its slot (a gap touching frame nf - 1 is never bridged either:
//      position nf reports the run up to the last flagged frame).
// The carries of the three scans between tiles live in LDS.
constexpr int SG_THREADS = 256, SG_ITEMS = 4, SG_TILE = SG_THREADS * SG_ITEMS;

// op(carry, v of the threads before this one); then *carry = op(carry, v of all threads), op = + (SUM) or max (every
// v >= -1, the identity of max here). Every thread of the workgroup calls it. The second barrier keeps wpart and
// *carry from being rewritten while a slower wave reads them.
template <bool SUM>
__device__ __forceinline__ int loc_block_excl_scan(int v, int* wpart, int* carry) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int ID = SUM ? 0 : -1;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl = SUM ? incl + u : (incl > u ? incl : u);
  }
  if (lane == 63) wpart[wave] = incl;
  int excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = ID;
  __syncthreads();
  const int base = *carry;
  int before = ID, total = ID;
#pragma unroll
  for (int k = 0; k < SG_THREADS / 64; ++k) {
    const int p = wpart[k];
    if (k < wave) before = SUM ? before + p : (before > p ? before : p);
    total = SUM ? total + p : (total > p ? total : p);
  }
  __syncthreads();
  if (SUM) {
    if (threadIdx.x == 0) *carry = base + total;
    return base + before + excl;
  }
  const int all = base > total ? base : total;
  if (threadIdx.x == 0) *carry = all;
  const int mine = before > excl ? before : excl;
  return base > mine ? base : mine;
}

__global__ __launch_bounds__(SG_THREADS) void track_segments_kernel(const float* __restrict__ t, SegRecs T, float thr,
                                                                    int merge, int min_frames,
                                                                    int32_t* __restrict__ seg_a,
                                                                    int32_t* __restrict__ seg_b,
                                                                    int32_t* __restrict__ count) {
  __shared__ int s_part[SG_THREADS / 64];
  __shared__ int s_last, s_start, s_cnt;
  const int j = blockIdx.x, tid = threadIdx.x;
  const int nf = T.nf[j];
  const float* __restrict__ tr = t + T.foff[j];
  int32_t* __restrict__ out_a = seg_a + T.foff[j];
  int32_t* __restrict__ out_b = seg_b + T.foff[j];
  merge = merge < nf ? merge : nf;    // a wider reach changes nothing
  if (tid == 0) {
    s_last = -1;
    s_start = -1;
    s_cnt = 0;
  }
  __syncthreads();
  for (int t0 = 0; t0 <= nf; t0 += SG_TILE) {
    const int f0 = t0 + tid * SG_ITEMS;
    bool flag[SG_ITEMS], st[SG_ITEMS], keep[SG_ITEMS];
    int a[SG_ITEMS], b[SG_ITEMS];
    int v = -1;
#pragma unroll
    for (int k = 0; k < SG_ITEMS; ++k) {
      const int f = f0 + k;
      flag[k] = f < nf && tr[f] < thr;    // strict; a NaN is not flagged
      if (flag[k]) v = f;
    }
    int last = loc_block_excl_scan<false>(v, s_part, &s_last);
    v = -1;
#pragma unroll
    for (int k = 0; k < SG_ITEMS; ++k) {
      const int f = f0 + k;
      b[k] = last;
      st[k] = flag[k] && (last < 0 || f - last - 1 > merge);
      if (st[k]) v = f;
      if (flag[k]) last = f;
    }
    int start = loc_block_excl_scan<false>(v, s_part, &s_start);
    v = 0;
#pragma unroll
    for (int k = 0; k < SG_ITEMS; ++k) {
      const int f = f0 + k;
      a[k] = start;
      keep[k] = (st[k] || f == nf) && b[k] >= 0 && b[k] - a[k] + 1 >= min_frames;
      v += keep[k] ? 1 : 0;
      if (st[k]) start = f;
    }
    int ord = loc_block_excl_scan<true>(v, s_part, &s_cnt);
#pragma unroll
    for (int k = 0; k < SG_ITEMS; ++k) {
      if (keep[k]) {
        out_a[ord] = a[k];
        out_b[ord] = b[k];
        ++ord;
      }
    }
  }
  __syncthreads();
  if (tid == 0) count[j] = s_cnt;
}

// -------------------------------------------------------------------------------------- stats ----
// One wave per slot; a slot at or past its recording's count returns at once. A used slot folds t[a .. b] as
// segment_reduce_kernel (csrc/recwin.hip) folds a segment: lane l takes frames a + l, a + l + 64, ... in index
// order into a two-sum pair, a minimum and its first index, and the 64 partial results meet in the same butterfly.
__global__ __launch_bounds__(256) void track_segment_stats_kernel(const float* __restrict__ t, StatRecs T, int nrec,
                                                                  const int32_t* __restrict__ seg_a,
                                                                  const int32_t* __restrict__ seg_b,
                                                                  const int32_t* __restrict__ count,
                                                                  float* __restrict__ seg_mean,
                                                                  float* __restrict__ seg_min,
                                                                  int32_t* __restrict__ seg_argmin) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (w >= T.cum[nrec]) return;       // wave-uniform: the lane-crossing steps below run with whole waves
  RDX_LOC_FIND(T, nrec, w, j);
  const int i = w - T.cum[j];
  if (i >= count[j]) return;
  const int64_t slot = T.foff[j] + i;
  const int a = seg_a[slot], n = seg_b[slot] - a + 1;
  const float* __restrict__ tr = t + T.foff[j] + a;
  float sum = 0.f, err = 0.f, lo = INFINITY;
  int at = INT32_MAX;
  for (int k = lane; k < n; k += 64) {
    const float v = tr[k];
    two_sum(sum, err, v);
    if (v < lo) { lo = v; at = k; }   // strict: a lane keeps the first of equal minima
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float sum2 = __shfl_xor(sum, o, 64), err2 = __shfl_xor(err, o, 64);
    two_sum(sum, err, sum2);
    err += err2;
    const float lo2 = __shfl_xor(lo, o, 64);
    const int at2 = __shfl_xor(at, o, 64);
    if (lo2 < lo || (lo2 == lo && at2 < at)) { lo = lo2; at = at2; }
  }
  if (lane == 0) {
    seg_mean[slot] = (float)(((double)sum + (double)err) / (double)n);
    seg_min[slot] = lo;
    seg_argmin[slot] = a + at;
  }
}

static inline int64_t loc_frames(int64_t m) { return (m + LC_F - 1) / LC_F; }

}  // namespace rdx

using namespace rdx;

extern "C" int rdx_track_overlap(const float* scores, const int64_t* seg, const int64_t* nwin, const int64_t* m,
                                 const int64_t* foffs, int R, int64_t hop, int64_t win, float* t, void* stream) {
  RDX_REQUIRE(scores && seg && nwin && m && foffs && t && R > 0);
  RDX_REQUIRE(win >= 1 && hop >= 1 && hop <= win);
  for (int r = 0; r < R; ++r) {
    RDX_REQUIRE(m[r] > 0 && foffs[r] >= 0);
    RDX_REQUIRE(nwin[r] == (m[r] <= win ? 1 : 1 + (m[r] - win + hop - 1) / hop));
  }
  for (int r0 = 0; r0 < R;) {
    TrackRecs T{};
    int nrec = 0;
    int64_t frames = 0;
    while (r0 + nrec < R && nrec < LC_MAX && frames + loc_frames(m[r0 + nrec]) <= INT32_MAX - 256) {
      const int r = r0 + nrec;
      T.m[nrec] = m[r];
      T.foff[nrec] = foffs[r];
      T.cum[nrec] = (int32_t)frames;
      frames += loc_frames(m[r]);
      ++nrec;
    }
    if (nrec == 0) return RDX_EUNSUPPORTED;   // one recording of 2^31 frames or more
    T.cum[nrec] = (int32_t)frames;
    hipLaunchKernelGGL(track_overlap_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, as_stream(stream),
                       scores, seg + r0, T, nrec, hop, win, t);
    RDX_LAUNCH_CHECK();
    r0 += nrec;
  }
  return RDX_OK;
}

extern "C" int rdx_track_segments(const float* t, const int64_t* foffs, const int64_t* nframes, int R, float thr,
                                  int merge, int min_frames, int32_t* seg_a, int32_t* seg_b, int32_t* count,
                                  void* stream) {
  RDX_REQUIRE(t && foffs && nframes && seg_a && seg_b && count && R > 0);
  RDX_REQUIRE(thr == thr && merge >= 0 && min_frames >= 1);    // a NaN threshold fails the first comparison
  for (int r = 0; r < R; ++r) {
    RDX_REQUIRE(foffs[r] >= 0 && nframes[r] > 0);
    if (nframes[r] > INT32_MAX - 2 * SG_TILE) return RDX_EUNSUPPORTED;
  }
  for (int r0 = 0; r0 < R; r0 += LC_MAX) {
    const int nrec = (R - r0) < LC_MAX ? (R - r0) : LC_MAX;
    SegRecs T{};
    for (int j = 0; j < nrec; ++j) {
      T.foff[j] = foffs[r0 + j];
      T.nf[j] = (int32_t)nframes[r0 + j];
    }
    hipLaunchKernelGGL(track_segments_kernel, dim3((unsigned)nrec), dim3(SG_THREADS), 0, as_stream(stream), t, T, thr,
                       merge, min_frames, seg_a, seg_b, count + r0);
    RDX_LAUNCH_CHECK();
  }
  return RDX_OK;
}

extern "C" int rdx_track_segment_stats(const float* t, const int64_t* foffs, const int64_t* nframes, int R,
                                       const int32_t* seg_a, const int32_t* seg_b, const int32_t* count,
                                       float* seg_mean, float* seg_min, int32_t* seg_argmin, void* stream) {
  RDX_REQUIRE(t && foffs && nframes && seg_a && seg_b && count && seg_mean && seg_min && seg_argmin && R > 0);
  for (int r = 0; r < R; ++r) {
    RDX_REQUIRE(foffs[r] >= 0 && nframes[r] > 0);
    if (nframes[r] > INT32_MAX - 2 * SG_TILE) return RDX_EUNSUPPORTED;
  }
  for (int r0 = 0; r0 < R;) {
    StatRecs T{};
    int nrec = 0;
    int64_t slots = 0;
    while (r0 + nrec < R && nrec < LC_MAX && slots + (nframes[r0 + nrec] + 1) / 2 <= INT32_MAX - 4) {
      T.foff[nrec] = foffs[r0 + nrec];
      T.cum[nrec] = (int32_t)slots;
      slots += (nframes[r0 + nrec] + 1) / 2;
      ++nrec;
    }
    T.cum[nrec] = (int32_t)slots;
    hipLaunchKernelGGL(track_segment_stats_kernel, dim3((unsigned)((slots + 3) / 4)), dim3(256), 0, as_stream(stream),
                       t, T, nrec, seg_a, seg_b, count + r0, seg_mean, seg_min, seg_argmin);
    RDX_LAUNCH_CHECK();
    r0 += nrec;
  }
  return RDX_OK;
}
