// Ingest of whole recordings (radhip/recordings.py, convert=True): interleaved float32 [frames, C] at any integer
// sample rate -> mono float32 at the model's rate, by the windowed-sinc polyphase filter of rdx_resample_kernel
// (csrc/augment.hip) evaluated on its compact taps.
//
// The dense row of phase p holds 2 * width + orig_g taps, of which only the positions with |t| < lowpass_width are
// not the clipped window's cos^2(pi / 2) (< 1e-30): first[p] .. first[p] + cnt[p] - 1, at most 2 * width + 2 of them
// whatever orig_g is. rdx_ingest_taps keeps those, ntap = max cnt per phase, tap-major (taps[j * new_g + p]) so that
// consecutive lanes, which own consecutive outputs and therefore consecutive phases, read consecutive words of the
// table from LDS (no bank conflict for any ntap) or from global memory (coalesced).
//
// Output o = i * new_g + p reads input frames m = i * orig_g - width + first[p] + j, j < ntap. m_first(o) does not
// decrease with o (first[0] >= 1, first[new_g - 1] <= orig_g + 1 and first is monotone; rdx_ingest_taps checks it), so
// a workgroup that owns outputs [o0, o0 + nout) needs the frames m_first(o0) .. m_first(o0 + nout - 1) + ntap - 1:
// about nout * orig_g / new_g + ntap of them, staged into LDS once as the mean over channels.
#include "common.h"

namespace rdx {

constexpr int IG_THREADS = 256;
constexpr int IG_MAXJOBS = 32;      // jobs per launch (the table travels as kernel arguments)
constexpr int IG_OB_MAX = 1024;     // outputs per workgroup: 4 per thread, fewer where the input span would not fit
constexpr int IG_RAW = 1024;        // interleaved floats per staging pass (two buffers of this size when C > 1)
constexpr int IG_LDS_BYTES = 64 * 1024;
constexpr int64_t IG_MAX_BLOCKS = 1 << 30;

struct IgJob {
  int64_t in_off, frames, out_off, out_len, first_off, taps_off;
  int32_t C, orig, nw, ntap, width, ob, xcap, lds_taps, blk0, pad_;
};
struct IgTable {
  IgJob j[IG_MAXJOBS];
};

struct IgPlan {
  int ob, xcap, lds_taps, lds_bytes;
};

// The tile of one (rate, channel count): taps in LDS when they fit beside the largest output block whose input span
// fits, else taps from global memory. false: not even 256 outputs' input span fits in 64 KiB.
static bool ig_plan(int orig, int nw, int ntap, int C, IgPlan* P) {
  const int64_t raw = C > 1 ? 2 * IG_RAW : 0;
  for (int lds_taps = 1; lds_taps >= 0; --lds_taps) {
    const int64_t tab = lds_taps ? (int64_t)nw * (ntap + 1) : 0;
    for (int ob = IG_OB_MAX; ob >= IG_THREADS; ob -= IG_THREADS) {
      // m_first(o) = floor(o * orig / nw - c) + 1 in exact arithmetic: the block's first and last output are at most
      // ceil((ob - 1) orig / nw) + 1 frames apart (+ 1 for a boundary decided in fp64 by rdx_ingest_taps)
      const int64_t xcap = ((int64_t)orig * (ob - 1) + nw - 1) / nw + ntap + 2;
      const int64_t bytes = 4 * (xcap + raw + tab);
      if (bytes <= IG_LDS_BYTES) {
        *P = IgPlan{ob, (int)xcap, lds_taps, (int)bytes};
        return true;
      }
    }
  }
  return false;
}

template <bool LDS_TAPS>
__device__ __forceinline__ void ig_outputs(const IgJob& J, const int32_t* __restrict__ gfirst,
                                           const float* __restrict__ gtap, const int32_t* s_first, const float* s_tap,
                                           const float* s_x, int p0, int f0, int nout, float* __restrict__ dst) {
  const int tid = threadIdx.x, nw = J.nw, ntap = J.ntap;
  auto first_at = [&](int p) { return LDS_TAPS ? s_first[p] : gfirst[p]; };
  auto tap_at = [&](int j, int p) { return LDS_TAPS ? s_tap[j * nw + p] : gtap[(int64_t)j * nw + p]; };
  // where this thread's output r starts in s_x (never past xcap - ntap: see ig_plan; the clamp costs nothing and
  // keeps a table that breaks the rule inside the tile)
  auto base_at = [&](int q, int p, int di) { return max(min(di * J.orig + first_at(p) - f0, J.xcap - ntap), 0); };
  const int nr = J.ob / IG_THREADS;
  if (IG_THREADS % nw == 0) {
    // the thread's outputs are multiples of new_g apart: one phase, every tap loaded once for all of them
    const int q0 = p0 + tid, p = q0 % nw;
    int base[IG_OB_MAX / IG_THREADS];
    float acc[IG_OB_MAX / IG_THREADS];
#pragma unroll
    for (int r = 0; r < IG_OB_MAX / IG_THREADS; ++r) {
      const int q = q0 + r * IG_THREADS;
      base[r] = (r < nr && tid + r * IG_THREADS < nout) ? base_at(q, p, q / nw) : 0;
      acc[r] = 0.f;
    }
    for (int j = 0; j < ntap; ++j) {
      const float k = tap_at(j, p);
#pragma unroll
      for (int r = 0; r < IG_OB_MAX / IG_THREADS; ++r) acc[r] = fmaf(k, s_x[base[r] + j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < IG_OB_MAX / IG_THREADS; ++r)
      if (r < nr && tid + r * IG_THREADS < nout) dst[tid + r * IG_THREADS] = acc[r];
  } else {
    for (int r = 0; r < nr; ++r) {
      const int t = tid + r * IG_THREADS;
      if (t >= nout) break;
      const int q = p0 + t, di = q / nw, p = q - di * nw;
      const int base = base_at(q, p, di);
      float acc = 0.f;
      for (int j = 0; j < ntap; ++j) acc = fmaf(tap_at(j, p), s_x[base + j], acc);
      dst[t] = acc;
    }
  }
}

__global__ __launch_bounds__(IG_THREADS) void ingest_resample_kernel(const float* __restrict__ in,
                                                                     float* __restrict__ out,
                                                                     const int32_t* __restrict__ first_all,
                                                                     const float* __restrict__ taps_all, IgTable T,
                                                                     int njobs) {
  extern __shared__ float ig_smem[];
  int jb = 0;
  while (jb + 1 < njobs && (int)blockIdx.x >= T.j[jb + 1].blk0) ++jb;
  const IgJob& J = T.j[jb];
  const int tid = threadIdx.x, C = J.C, nw = J.nw, ntap = J.ntap;
  const int64_t o0 = (int64_t)((int)blockIdx.x - J.blk0) * J.ob;
  const int nout = (int)min((int64_t)J.ob, J.out_len - o0);
  const int64_t i0 = o0 / nw;
  const int p0 = (int)(o0 - i0 * nw);
  const int32_t* __restrict__ gfirst = first_all + J.first_off;
  const float* __restrict__ gtap = taps_all + J.taps_off;

  float* s_x = ig_smem;
  float* s_raw = s_x + J.xcap;
  int32_t* s_first = reinterpret_cast<int32_t*>(s_raw + (C > 1 ? 2 * IG_RAW : 0));
  float* s_tap = reinterpret_cast<float*>(s_first + nw);
  if (J.lds_taps) {
    for (int i = tid; i < nw; i += IG_THREADS) s_first[i] = gfirst[i];
    for (int i = tid; i < nw * ntap; i += IG_THREADS) s_tap[i] = gtap[i];
  }

  // the block's input frames lo .. lo + span - 1 (frames outside [0, frames) are zero)
  const int f0 = gfirst[p0];
  const int ql = p0 + nout - 1, dil = ql / nw;
  const int span = min(dil * J.orig + gfirst[ql - dil * nw] + ntap - f0, J.xcap);
  const int64_t lo = i0 * J.orig - J.width + f0;
  const float* __restrict__ src = in + J.in_off;
  if (C == 1) {
    for (int s = tid; s < span; s += IG_THREADS) {
      const int64_t f = lo + s;
      s_x[s] = (f >= 0 && f < J.frames) ? src[f] : 0.f;
    }
  } else {
    // consecutive lanes load consecutive interleaved floats into a raw buffer; after the barrier a thread owns a
    // frame and sums its C channels in channel order. Two raw buffers: pass n + 1 loads while pass n is reduced.
    const int F = IG_RAW / C;
    const int64_t nelem = J.frames * C;
    for (int s0 = 0, pass = 0; s0 < span; s0 += F, ++pass) {
      float* buf = s_raw + (pass & 1) * IG_RAW;
      const int nf = min(F, span - s0);
      const int64_t e0 = (lo + s0) * C;
      for (int e = tid; e < nf * C; e += IG_THREADS) {
        const int64_t ge = e0 + e;
        buf[e] = (ge >= 0 && ge < nelem) ? src[ge] : 0.f;
      }
      __syncthreads();
      for (int f = tid; f < nf; f += IG_THREADS) {
        float sum = buf[f * C];
        for (int c = 1; c < C; ++c) sum += buf[f * C + c];
        s_x[s0 + f] = sum / (float)C;
      }
    }
  }
  __syncthreads();

  float* __restrict__ dst = out + J.out_off + o0;
  if (J.lds_taps) ig_outputs<true>(J, gfirst, gtap, s_first, s_tap, s_x, p0, f0, nout, dst);
  else ig_outputs<false>(J, gfirst, gtap, s_first, s_tap, s_x, p0, f0, nout, dst);
}

// t of dense position k of phase p, as rdx_resample_kernel computes it before the clip
static inline double ig_t(int k, int p, int width, int orig, int nw, double base_freq) {
  const double idx = (double)(k - width) / orig;
  return ((-(double)p) / nw + idx) * base_freq;
}

}  // namespace rdx

using namespace rdx;

extern "C" int rdx_ingest_taps(int orig_freq, int new_freq, int lowpass_width, double rolloff, int32_t* first,
                               float* taps, int64_t taps_cap, int* ntap_out, int* width_out, int* orig_g_out,
                               int* new_g_out) {
  RDX_REQUIRE(orig_freq > 0 && new_freq > 0 && lowpass_width > 0 && rolloff > 0);
  RDX_REQUIRE((first == nullptr) == (taps == nullptr));
  int a = orig_freq, b = new_freq;
  while (b) { int t = a % b; a = b; b = t; }
  const int orig = orig_freq / a, nw = new_freq / a;
  const double base_freq = (orig < nw ? orig : nw) * rolloff;
  const int width = (int)ceil((double)lowpass_width * orig / base_freq);
  const int kw = 2 * width + orig;
  const double L = (double)lowpass_width;
  auto inside = [&](int k, int p) {
    const double t = ig_t(k, p, width, orig, nw, base_freq);
    return t > -L && t < L;
  };
  // first[p]: the smallest dense position inside the window, from its closed form, settled by the fp64 test itself
  auto first_of = [&](int p) {
    int k = (int)floor(width + (double)orig * p / nw - (double)orig * L / base_freq) + 1;
    if (k < 0) k = 0;
    if (k > kw - 1) k = kw - 1;
    while (k > 0 && inside(k - 1, p)) --k;
    while (k < kw - 1 && !inside(k, p)) ++k;
    return k;
  };
  int ntap = 0, prev = 0;
  for (int p = 0; p < nw; ++p) {
    const int f = first_of(p);
    int c = 0;
    while (f + c < kw && inside(f + c, p)) ++c;
    if (c > ntap) ntap = c;
    // the kernel's tile rests on m_first not decreasing with the output index
    if (c == 0 || (p > 0 && f < prev)) return RDX_EUNSUPPORTED;
    if (p == nw - 1 && first_of(0) + orig < f) return RDX_EUNSUPPORTED;
    prev = f;
  }
  if (ntap_out) *ntap_out = ntap;
  if (width_out) *width_out = width;
  if (orig_g_out) *orig_g_out = orig;
  if (new_g_out) *new_g_out = nw;
  if (!taps) return RDX_OK;
  if (taps_cap < (int64_t)nw * ntap) return RDX_EINVAL;
  const double PI = 3.141592653589793;
  const double scale = base_freq / orig;
  for (int p = 0; p < nw; ++p) {
    const int f = first_of(p);
    first[p] = f;
    for (int j = 0; j < ntap; ++j) {
      float v = 0.f;
      if (f + j < kw && inside(f + j, p)) {   // the values rdx_resample_kernel stores for these positions
        double t = ig_t(f + j, p, width, orig, nw, base_freq);
        const double c = cos(t * PI / lowpass_width / 2.0);
        t *= PI;
        const double kv = (t == 0.0) ? 1.0 : sin(t) / t;
        v = (float)(kv * (c * c) * scale);
      }
      taps[(int64_t)j * nw + p] = v;
    }
  }
  return RDX_OK;
}

extern "C" int rdx_ingest_plan(int orig_g, int new_g, int ntap, int channels, int* block_out, int* lds_bytes_out,
                               int* taps_in_lds_out) {
  RDX_REQUIRE(orig_g > 0 && new_g > 0 && ntap > 0 && channels > 0);
  IgPlan P;
  if (channels > IG_RAW || !ig_plan(orig_g, new_g, ntap, channels, &P)) return RDX_EUNSUPPORTED;
  if (block_out) *block_out = P.ob;
  if (lds_bytes_out) *lds_bytes_out = P.lds_bytes;
  if (taps_in_lds_out) *taps_in_lds_out = P.lds_taps;
  return RDX_OK;
}

extern "C" int rdx_ingest_resample(const float* in, int64_t in_elems, float* out, int64_t out_elems,
                                   const int32_t* first, int64_t first_elems, const float* taps, int64_t taps_elems,
                                   const rdx_ingest_job* jobs, int njobs, void* stream) {
  RDX_REQUIRE(in && out && first && taps && jobs && njobs > 0);
  RDX_REQUIRE(in_elems > 0 && out_elems > 0 && first_elems > 0 && taps_elems > 0);
  // every job is checked before the first launch
  for (int i = 0; i < njobs; ++i) {
    const rdx_ingest_job& j = jobs[i];
    RDX_REQUIRE(j.frames > 0 && j.channels > 0 && j.orig_g > 0 && j.new_g > 0 && j.ntap > 0 && j.width > 0);
    RDX_REQUIRE(j.frames <= (INT64_MAX >> 16) / j.channels && j.frames <= (INT64_MAX >> 16) / j.new_g);
    RDX_REQUIRE(j.in_offset >= 0 && j.in_offset <= in_elems && j.frames * j.channels <= in_elems - j.in_offset);
    const int64_t out_len = (j.frames * j.new_g + j.orig_g - 1) / j.orig_g;
    RDX_REQUIRE(j.out_offset >= 0 && j.out_offset <= out_elems && out_len <= out_elems - j.out_offset);
    RDX_REQUIRE(j.first_offset >= 0 && j.first_offset <= first_elems && j.new_g <= first_elems - j.first_offset);
    RDX_REQUIRE(j.taps_offset >= 0 && j.taps_offset <= taps_elems &&
                (int64_t)j.new_g * j.ntap <= taps_elems - j.taps_offset);
    IgPlan P;
    if (j.channels > IG_RAW || !ig_plan(j.orig_g, j.new_g, j.ntap, j.channels, &P)) return RDX_EUNSUPPORTED;
    if ((out_len + P.ob - 1) / P.ob > IG_MAX_BLOCKS) return RDX_EUNSUPPORTED;
  }
  int i = 0;
  while (i < njobs) {
    IgTable T{};
    int n = 0, lds = 0;
    int64_t blocks = 0;
    for (; i < njobs && n < IG_MAXJOBS; ++i, ++n) {
      const rdx_ingest_job& j = jobs[i];
      IgPlan P;
      ig_plan(j.orig_g, j.new_g, j.ntap, j.channels, &P);
      const int64_t out_len = (j.frames * j.new_g + j.orig_g - 1) / j.orig_g;
      const int64_t nb = (out_len + P.ob - 1) / P.ob;
      if (n > 0 && blocks + nb > IG_MAX_BLOCKS) break;
      T.j[n] = IgJob{j.in_offset, j.frames, j.out_offset, out_len, j.first_offset, j.taps_offset, j.channels,
                     j.orig_g, j.new_g, j.ntap, j.width, P.ob, P.xcap, P.lds_taps, (int32_t)blocks, 0};
      blocks += nb;
      if (P.lds_bytes > lds) lds = P.lds_bytes;
    }
    hipLaunchKernelGGL(ingest_resample_kernel, dim3((unsigned)blocks), dim3(IG_THREADS), (size_t)lds,
                       as_stream(stream), in, out, first, taps, T, n);
    RDX_LAUNCH_CHECK();
  }
  return RDX_OK;
}
