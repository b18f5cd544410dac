// Native FLAC reader + multi-threaded batch loader (host C++, C ABI in include/radio.h).
//
// Replaces the reference's `soundfile.read(f"flac/{key}.flac")` calls in the dataset __getitem__s
// (src/data_utils.py:165, :200, :221). soundfile/libsndfile is not part of this image, and the
// reference loads one file at a time in the main process (num_workers=0 for train). Here a batch of
// files is decoded by a pool of threads straight into one caller-owned float buffer (pinned host
// memory on the train path), which is then a single H2D copy.
//
// Decoder: FLAC frames of any block size; CONSTANT, VERBATIM, FIXED (order 0..4) and LPC (order
// 1..32) subframes; wasted bits; Rice / Rice2 residuals incl. escaped partitions; independent and
// left/side, right/side, mid/side stereo; 4..32 bits per sample. Frame CRC-8 and CRC-16 are
// verified (a corrupt file is an error, as it is for libsndfile). Samples are normalised like
// libsndfile's float read: x / 2^(bps-1) (16-bit: x / 32768).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include <atomic>

#include "../../include/radio.h"
#include "../../include/radio_interleaved.h"

namespace {

struct Bits {
  const uint8_t* p;
  size_t n;       // bytes
  size_t pos;     // bit position
  bool bad;
  uint32_t read(int k) {  // k <= 32
    if (k == 0) return 0;
    if (pos + (size_t)k > n * 8) { bad = true; pos = n * 8; return 0; }
    uint64_t v = 0;
    int got = 0;
    while (got < k) {
      size_t byte = pos >> 3;
      int off = (int)(pos & 7);
      int take = 8 - off;
      if (take > k - got) take = k - got;
      uint32_t bits = ((uint32_t)p[byte] >> (8 - off - take)) & ((1u << take) - 1u);
      v = (v << take) | bits;
      got += take;
      pos += take;
    }
    return (uint32_t)v;
  }
  int32_t read_signed(int k) {
    if (k == 0) return 0;
    uint32_t v = read(k);
    if (k < 32 && (v & (1u << (k - 1)))) return (int32_t)(v | (~0u << k));
    return (int32_t)v;
  }
  uint32_t unary() {  // count zeros before the next 1
    uint32_t q = 0;
    while (true) {
      if (pos >= n * 8) { bad = true; return 0; }
      size_t byte = pos >> 3;
      int off = (int)(pos & 7);
      uint8_t rest = (uint8_t)(p[byte] << off);
      if (rest) {
        int lz = __builtin_clz((uint32_t)rest) - 24;
        q += lz;
        pos += lz + 1;
        return q;
      }
      q += 8 - off;
      pos += 8 - off;
    }
  }
  void align() { pos = (pos + 7) & ~(size_t)7; }
};

uint8_t crc8(const uint8_t* d, size_t n) {
  uint8_t c = 0;
  for (size_t i = 0; i < n; ++i) {
    c ^= d[i];
    for (int b = 0; b < 8; ++b) c = (c & 0x80) ? (uint8_t)((c << 1) ^ 0x07) : (uint8_t)(c << 1);
  }
  return c;
}

uint16_t crc16(const uint8_t* d, size_t n) {
  uint16_t c = 0;
  for (size_t i = 0; i < n; ++i) {
    c ^= (uint16_t)d[i] << 8;
    for (int b = 0; b < 8; ++b) c = (c & 0x8000) ? (uint16_t)((c << 1) ^ 0x8005) : (uint16_t)(c << 1);
  }
  return c;
}

struct StreamInfo {
  int rate = 0, channels = 0, bps = 0;
  int64_t total = 0;  // samples per channel (0 = unknown)
  int max_block = 0;
};

// parse "fLaC" + metadata; returns offset of the first frame or -1
long parse_header(const uint8_t* d, size_t n, StreamInfo* si) {
  size_t o = 0;
  if (n >= 10 && d[0] == 'I' && d[1] == 'D' && d[2] == '3') {  // ID3v2 tag in front
    size_t sz = ((size_t)(d[6] & 0x7f) << 21) | ((size_t)(d[7] & 0x7f) << 14) | ((size_t)(d[8] & 0x7f) << 7) |
                (size_t)(d[9] & 0x7f);
    o = 10 + sz;
  }
  if (o + 4 > n || memcmp(d + o, "fLaC", 4) != 0) return -1;
  o += 4;
  bool have_info = false;
  while (true) {
    if (o + 4 > n) return -1;
    int last = d[o] >> 7, type = d[o] & 0x7f;
    size_t len = ((size_t)d[o + 1] << 16) | ((size_t)d[o + 2] << 8) | d[o + 3];
    o += 4;
    if (o + len > n) return -1;
    if (type == 0) {
      if (len < 34) return -1;
      const uint8_t* s = d + o;
      si->max_block = (s[2] << 8) | s[3];
      si->rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
      si->channels = ((s[12] >> 1) & 7) + 1;
      si->bps = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
      si->total = ((int64_t)(s[13] & 0x0f) << 32) | ((int64_t)s[14] << 24) | ((int64_t)s[15] << 16) |
                  ((int64_t)s[16] << 8) | s[17];
      have_info = true;
    }
    o += len;
    if (last) break;
  }
  return have_info ? (long)o : -1;
}

bool read_utf8(Bits& b) {  // frame/sample number, value unused
  uint32_t x = b.read(8);
  int extra = 0;
  if (!(x & 0x80)) extra = 0;
  else if ((x & 0xe0) == 0xc0) extra = 1;
  else if ((x & 0xf0) == 0xe0) extra = 2;
  else if ((x & 0xf8) == 0xf0) extra = 3;
  else if ((x & 0xfc) == 0xf8) extra = 4;
  else if ((x & 0xfe) == 0xfc) extra = 5;
  else if (x == 0xfe) extra = 6;
  else return false;
  for (int i = 0; i < extra; ++i)
    if ((b.read(8) & 0xc0) != 0x80) return false;
  return !b.bad;
}

bool residual(Bits& b, int bs, int order, int64_t* out) {
  int method = (int)b.read(2);
  if (method > 1) return false;
  int pbits = method == 0 ? 4 : 5;
  uint32_t esc = method == 0 ? 15u : 31u;
  int porder = (int)b.read(4);
  int parts = 1 << porder;
  if ((bs >> porder) < order || (bs & (parts - 1))) return false;
  int i = order;
  for (int p = 0; p < parts; ++p) {
    int cnt = (bs >> porder) - (p == 0 ? order : 0);
    uint32_t k = b.read(pbits);
    if (k == esc) {
      int nb = (int)b.read(5);
      for (int j = 0; j < cnt; ++j) out[i++] = b.read_signed(nb);
    } else {
      for (int j = 0; j < cnt; ++j) {
        uint64_t q = b.unary();
        uint64_t v = (q << k) | (k ? b.read((int)k) : 0u);
        out[i++] = (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
      }
    }
    if (b.bad) return false;
  }
  return true;
}

bool subframe(Bits& b, int bs, int bps, int64_t* out) {
  if (b.read(1) != 0) return false;
  int type = (int)b.read(6);
  int wasted = 0;
  if (b.read(1)) wasted = (int)b.unary() + 1;
  int sbps = bps - wasted;
  if (sbps <= 0 || sbps > 32) return false;
  if (type == 0) {
    int64_t v = b.read_signed(sbps);
    for (int i = 0; i < bs; ++i) out[i] = v;
  } else if (type == 1) {
    for (int i = 0; i < bs; ++i) out[i] = b.read_signed(sbps);
  } else if (type >= 8 && type <= 12) {
    int order = type - 8;
    if (order > bs) return false;
    for (int i = 0; i < order; ++i) out[i] = b.read_signed(sbps);
    if (!residual(b, bs, order, out)) return false;
    for (int i = order; i < bs; ++i) {
      int64_t pr = 0;
      switch (order) {
        case 1: pr = out[i - 1]; break;
        case 2: pr = 2 * out[i - 1] - out[i - 2]; break;
        case 3: pr = 3 * out[i - 1] - 3 * out[i - 2] + out[i - 3]; break;
        case 4: pr = 4 * out[i - 1] - 6 * out[i - 2] + 4 * out[i - 3] - out[i - 4]; break;
        default: break;
      }
      out[i] += pr;
    }
  } else if (type >= 32) {
    int order = type - 31;
    if (order > bs) return false;
    for (int i = 0; i < order; ++i) out[i] = b.read_signed(sbps);
    int prec = (int)b.read(4) + 1;
    if (prec == 16) return false;
    int shift = b.read_signed(5);
    if (shift < 0) return false;
    int32_t coef[32];
    for (int j = 0; j < order; ++j) coef[j] = b.read_signed(prec);
    if (!residual(b, bs, order, out)) return false;
    for (int i = order; i < bs; ++i) {
      int64_t acc = 0;
      for (int j = 0; j < order; ++j) acc += (int64_t)coef[j] * out[i - 1 - j];
      out[i] += acc >> shift;
    }
  } else {
    return false;
  }
  if (wasted)
    for (int i = 0; i < bs; ++i) out[i] <<= wasted;
  return !b.bad;
}

// decodes every frame; writes up to `cap` interleaved frames (per-channel samples) of `channels`
// into out (float or double via T). Returns frames decoded (may exceed cap: the count is kept) or
// a negative RDX_IO_* code.
template <typename T>
int64_t decode(const uint8_t* d, size_t n, T* out, int64_t cap, StreamInfo* si_out) {
  StreamInfo si;
  long o = parse_header(d, n, &si);
  if (o < 0) return RDX_IO_EFORMAT;
  if (si_out) *si_out = si;
  std::vector<int64_t> ch[8];
  int64_t frames = 0;
  size_t pos = (size_t)o;
  while (pos + 2 <= n) {
    if (!(d[pos] == 0xff && (d[pos + 1] & 0xfe) == 0xf8)) {  // trailing junk/tags: stop
      break;
    }
    Bits b{d, n, pos * 8, false};
    b.read(15);  // sync + reserved
    b.read(1);   // blocking strategy
    int bs_code = (int)b.read(4), sr_code = (int)b.read(4), ch_code = (int)b.read(4), ss_code = (int)b.read(3);
    if (b.read(1) != 0) return RDX_IO_ECORRUPT;
    if (!read_utf8(b)) return RDX_IO_ECORRUPT;
    int bs;
    if (bs_code == 0) return RDX_IO_ECORRUPT;
    else if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576 << (bs_code - 2);
    else if (bs_code == 6) bs = (int)b.read(8) + 1;
    else if (bs_code == 7) bs = (int)b.read(16) + 1;
    else bs = 256 << (bs_code - 8);
    if (sr_code == 12) b.read(8);
    else if (sr_code == 13 || sr_code == 14) b.read(16);
    else if (sr_code == 15) return RDX_IO_ECORRUPT;
    int bps;
    static const int ss_tab[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    if (ss_code == 0) bps = si.bps;
    else if (ss_code == 3) return RDX_IO_ECORRUPT;
    else bps = ss_tab[ss_code];
    if (b.bad) return RDX_IO_ECORRUPT;
    size_t hdr_end = b.pos >> 3;
    uint8_t c8 = (uint8_t)b.read(8);
    if (c8 != crc8(d + pos, hdr_end - pos)) return RDX_IO_ECORRUPT;
    int nch;
    if (ch_code < 8) nch = ch_code + 1;
    else if (ch_code <= 10) nch = 2;
    else return RDX_IO_ECORRUPT;
    if (nch != si.channels) return RDX_IO_ECORRUPT;
    for (int c = 0; c < nch; ++c) {
      if ((int64_t)ch[c].size() < bs) ch[c].resize(bs);
      int extra = (ch_code == 8 && c == 1) || (ch_code == 9 && c == 0) || (ch_code == 10 && c == 1);
      if (!subframe(b, bs, bps + extra, ch[c].data())) return RDX_IO_ECORRUPT;
    }
    if (ch_code == 8) {         // left / side
      for (int i = 0; i < bs; ++i) ch[1][i] = ch[0][i] - ch[1][i];
    } else if (ch_code == 9) {  // side / right
      for (int i = 0; i < bs; ++i) ch[0][i] += ch[1][i];
    } else if (ch_code == 10) {  // mid / side
      for (int i = 0; i < bs; ++i) {
        int64_t mid = (ch[0][i] << 1) | (ch[1][i] & 1), side = ch[1][i];
        ch[0][i] = (mid + side) >> 1;
        ch[1][i] = (mid - side) >> 1;
      }
    }
    b.align();
    size_t body_end = b.pos >> 3;
    uint16_t c16 = (uint16_t)b.read(16);
    if (b.bad || c16 != crc16(d + pos, body_end - pos)) return RDX_IO_ECORRUPT;
    const double scale = 1.0 / (double)(1ull << (si.bps - 1));
    for (int i = 0; i < bs; ++i, ++frames) {
      if (frames >= cap) continue;
      for (int c = 0; c < nch; ++c) out[frames * nch + c] = (T)((double)ch[c][i] * scale);
    }
    pos = b.pos >> 3;
  }
  if (si.total && frames != si.total) return RDX_IO_ECORRUPT;
  return frames;
}

bool slurp(const char* path, std::vector<uint8_t>* buf) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (sz < 0) { fclose(f); return false; }
  buf->resize((size_t)sz);
  size_t got = sz ? fread(buf->data(), 1, (size_t)sz, f) : 0;
  fclose(f);
  return got == (size_t)sz;
}

}  // namespace

extern "C" {

int rdx_flac_probe(const char* path, int64_t* frames, int* channels, int* sample_rate, int* bits) {
  FILE* f = fopen(path, "rb");
  if (!f) return RDX_IO_ENOENT;
  std::vector<uint8_t> head(1 << 16);
  size_t got = fread(head.data(), 1, head.size(), f);
  fclose(f);
  StreamInfo si;
  if (parse_header(head.data(), got, &si) < 0) {
    std::vector<uint8_t> all;  // long metadata blocks: read the whole file
    if (!slurp(path, &all) || parse_header(all.data(), all.size(), &si) < 0) return RDX_IO_EFORMAT;
  }
  if (frames) *frames = si.total;
  if (channels) *channels = si.channels;
  if (sample_rate) *sample_rate = si.rate;
  if (bits) *bits = si.bps;
  return 0;
}

int rdx_flac_decode_mem(const uint8_t* data, int64_t nbytes, double* out, int64_t cap_frames,
                        int64_t* frames_out, int* channels, int* sample_rate) {
  StreamInfo si;
  int64_t r = decode<double>(data, (size_t)nbytes, out, cap_frames, &si);
  if (r < 0) return (int)r;
  if (frames_out) *frames_out = r;
  if (channels) *channels = si.channels;
  if (sample_rate) *sample_rate = si.rate;
  return r > cap_frames ? RDX_IO_ESHORT : 0;
}

int rdx_flac_read(const char* path, double* out, int64_t cap_frames, int64_t* frames_out) {
  std::vector<uint8_t> buf;
  if (!slurp(path, &buf)) return RDX_IO_ENOENT;
  return rdx_flac_decode_mem(buf.data(), (int64_t)buf.size(), out, cap_frames, frames_out, nullptr, nullptr);
}

int rdx_flac_read_batch(const char* const* paths, int n, float* out, const int64_t* offsets, const int64_t* caps,
                        int64_t* frames_out, int* status, int threads) {
  if (n < 0 || (n > 0 && (!paths || !out || !offsets || !caps || !frames_out || !status))) return RDX_IO_EARG;
  if (threads <= 0) threads = 1;
  if (threads > n) threads = n > 0 ? n : 1;
  std::atomic<int> next{0};
  auto work = [&]() {
    std::vector<uint8_t> buf;
    while (true) {
      int i = next.fetch_add(1);
      if (i >= n) break;
      frames_out[i] = 0;
      if (!slurp(paths[i], &buf)) { status[i] = RDX_IO_ENOENT; continue; }
      StreamInfo si;
      int64_t r = decode<float>(buf.data(), buf.size(), out + offsets[i], caps[i], &si);
      if (r < 0) { status[i] = (int)r; continue; }
      if (si.channels != 1) { status[i] = RDX_IO_ECHANNELS; continue; }
      frames_out[i] = r;
      status[i] = r > caps[i] ? RDX_IO_ESHORT : 0;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
  for (int i = 0; i < n; ++i)
    if (status[i]) return status[i];
  return 0;
}

int rdx_flac_read_batch_interleaved(const char* const* paths, int n, float* out, const int64_t* offsets,
                                    const int64_t* caps, const int* channels, int64_t* frames_out, int* status,
                                    int threads) {
  if (n < 0 || (n > 0 && (!paths || !out || !offsets || !caps || !channels || !frames_out || !status)))
    return RDX_IO_EARG;
  if (threads <= 0) threads = 1;
  if (threads > n) threads = n > 0 ? n : 1;
  std::atomic<int> next{0};
  auto work = [&]() {
    std::vector<uint8_t> buf;
    while (true) {
      int i = next.fetch_add(1);
      if (i >= n) break;
      frames_out[i] = 0;
      if (!slurp(paths[i], &buf)) { status[i] = RDX_IO_ENOENT; continue; }
      StreamInfo si;
      if (parse_header(buf.data(), buf.size(), &si) < 0) { status[i] = RDX_IO_EFORMAT; continue; }
      // caps[i] frames of channels[i] floats were reserved: another channel count would not fit them
      if (si.channels != channels[i]) { status[i] = RDX_IO_ECHCOUNT; continue; }
      int64_t r = decode<float>(buf.data(), buf.size(), out + offsets[i], caps[i], nullptr);
      if (r < 0) { status[i] = (int)r; continue; }
      frames_out[i] = r;
      status[i] = r > caps[i] ? RDX_IO_ESHORT : 0;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
  for (int i = 0; i < n; ++i)
    if (status[i]) return status[i];
  return 0;
}

const char* rdx_io_strerror(int code) {
  switch (code) {
    case 0: return "ok";
    case RDX_IO_ENOENT: return "cannot open/read file";
    case RDX_IO_EFORMAT: return "not a FLAC stream (no fLaC marker / STREAMINFO)";
    case RDX_IO_ECORRUPT: return "corrupt FLAC frame (bad header, subframe or CRC)";
    case RDX_IO_ESHORT: return "output capacity smaller than the decoded length";
    case RDX_IO_ECHANNELS: return "batch loader expects mono files";
    case RDX_IO_EARG: return "invalid argument";
    case RDX_IO_ECHCOUNT: return "channel count differs from the one the buffer was sized for";
    default: return "unknown radio error";
  }
}

}  // extern "C"
