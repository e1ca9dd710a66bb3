// The host stage of the JPEG decoder (header section 4f): the bytes of a baseline JPEG file -> its quantised DCT
// coefficients and quantiser tables, for csrc/jpeg_decode.hip to finish on the device.
//
//   lib/datasets/datasets.py:171-172 (Image.open(f).convert('RGB') of CocoKeypoints.__getitem__); libjpeg's jdmarker /
//   jdhuff on the way: the marker walk, the Huffman tables, the interleaved baseline scan with restart intervals
//
// Plain C++17 without a HIP header: it compiles on its own with a host compiler (tools/jpeg_entropy_check.cpp runs it
// under the sanitizers over truncated and corrupted files).  The file is hostile until proven otherwise: every read of
// `data` is bounded by `len`, every count and size that reaches the caller was checked against the limits of section 4f,
// and whatever is not plainly the served subset is refused with a reason - the caller then decodes that file elsewhere.
// Nothing here allocates, throws or keeps state between calls.
#include <cstdint>
#include <cstring>

#include "rtpose_mi355x.h"

namespace {

constexpr int kLook = 10;  // bits of the look-ahead tables

// the zig-zag position k of a coefficient -> its place in the row-major 8 x 8 block
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool defined = false;
  uint8_t counts[17];   // codes of each length 1..16
  uint8_t vals[256];
  int total = 0;
  // derived (build): codes of length l run from mincode[l] to maxcode[l] and index vals from valptr[l]
  int32_t maxcode[18];  // -1 where a length has no code
  int32_t mincode[17];
  int32_t valptr[17];
  uint16_t look[1 << kLook];  // length << 8 | symbol for codes of at most kLook bits, 0 otherwise
  // AC only: a whole coefficient (code and magnitude bits within kLook bits): value << 16 | run << 8 | bits, 0 otherwise
  int32_t fast[1 << kLook];
};

struct Parsed {
  rtpose_jpeg_info info;
  uint16_t q[4][64];  // natural order
  bool q_defined[4];
  Huff dc[4], ac[4];
  int tq[3], td[3], ta[3];
  size_t scan;  // the first byte of entropy-coded data
};

int refuse(rtpose_jpeg_info* info, int reason) {
  if (info) info->reason = reason;
  return reason;
}

inline unsigned be16(const uint8_t* p) { return (unsigned)p[0] << 8 | p[1]; }

// Annex C of the specification: sizes -> codes; a table whose codes do not fit their lengths is malformed
bool build(Huff& h, bool is_ac) {
  int code = 0, k = 0;
  memset(h.look, 0, sizeof(h.look));
  memset(h.fast, 0, sizeof(h.fast));
  for (int l = 1; l <= 16; ++l) {
    h.valptr[l] = k;
    h.mincode[l] = code;
    const int n = h.counts[l];
    if (code + n > (1 << l)) return false;
    if (l <= kLook)
      for (int i = 0; i < n; ++i) {
        const uint16_t e = (uint16_t)(l << 8 | h.vals[k + i]);
        const int first = (code + i) << (kLook - l);
        for (int j = 0; j < (1 << (kLook - l)); ++j) h.look[first + j] = e;
      }
    h.maxcode[l] = n ? code + n - 1 : -1;
    code = (code + n) << 1;
    k += n;
  }
  h.maxcode[17] = 0x7fffffff;
  if (is_ac)
    for (int i = 0; i < (1 << kLook); ++i) {
      const int e = h.look[i];
      if (!e) continue;
      const int l = e >> 8, run = (e & 255) >> 4, s = e & 15;
      if (s == 0 || s > 10 || l + s > kLook) continue;
      int v = (i >> (kLook - l - s)) & ((1 << s) - 1);
      if (v < (1 << (s - 1))) v -= (1 << s) - 1;  // the specification's EXTEND
      h.fast[i] = v * 65536 + (run << 8 | (l + s));
    }
  return true;
}

// ---- the marker walk up to and including the SOS header ----------------------------------------------------------------
int parse(const uint8_t* data, size_t len, Parsed& P) {
  rtpose_jpeg_info& I = P.info;
  memset(&I, 0, sizeof(I));
  I.struct_bytes = (uint32_t)sizeof(I);
  memset(P.q_defined, 0, sizeof(P.q_defined));
  if (!data || len < 4 || data[0] != 0xFF || data[1] != 0xD8) return refuse(&I, RTPOSE_JPEG_R_NOT_JPEG);
  size_t p = 2;
  bool frame = false;
  int ids[3] = {0, 0, 0};
  for (;;) {
    if (p >= len) return refuse(&I, RTPOSE_JPEG_R_TRUNCATED);
    if (data[p] != 0xFF) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
    while (p < len && data[p] == 0xFF) ++p;  // fill bytes
    if (p >= len) return refuse(&I, RTPOSE_JPEG_R_TRUNCATED);
    const int m = data[p++];
    if (m == 0xD9) return refuse(&I, RTPOSE_JPEG_R_TRUNCATED);  // EOI before a scan
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
    if (len - p < 2) return refuse(&I, RTPOSE_JPEG_R_TRUNCATED);
    const size_t L = be16(data + p);
    if (L < 2) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
    if (len - p < L) return refuse(&I, RTPOSE_JPEG_R_TRUNCATED);
    const uint8_t* s = data + p + 2;
    size_t n = L - 2;
    p += L;
    if (m == 0xC0) {  // SOF0
      if (frame) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      if (n < 6) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      if (s[0] != 8) return refuse(&I, RTPOSE_JPEG_R_PRECISION);
      const unsigned h = be16(s + 1), w = be16(s + 3);
      const int nc = s[5];
      if (h == 0 && w >= 1 && w <= 16384) return refuse(&I, RTPOSE_JPEG_R_DNL);  // the height comes with a DNL segment
      if (h < 1 || h > 16384 || w < 1 || w > 16384) return refuse(&I, RTPOSE_JPEG_R_SIZE);
      if (nc != 1 && nc != 3) return refuse(&I, RTPOSE_JPEG_R_COMPONENTS);
      if (n != (size_t)(6 + 3 * nc)) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      I.width = (int32_t)w;
      I.height = (int32_t)h;
      I.components = nc;
      for (int c = 0; c < nc; ++c) {
        ids[c] = s[6 + 3 * c];
        I.hsamp[c] = s[7 + 3 * c] >> 4;
        I.vsamp[c] = s[7 + 3 * c] & 15;
        P.tq[c] = s[8 + 3 * c];
        if (P.tq[c] > 3) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      }
      if (nc == 1) {
        if (I.hsamp[0] != 1 || I.vsamp[0] != 1) return refuse(&I, RTPOSE_JPEG_R_SAMPLING);
        I.mode = RTPOSE_JPEG_GRAY;
      } else {
        if (ids[0] == ids[1] || ids[0] == ids[2] || ids[1] == ids[2]) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        if (ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B') return refuse(&I, RTPOSE_JPEG_R_COLORSPACE);
        if (I.hsamp[1] != 1 || I.vsamp[1] != 1 || I.hsamp[2] != 1 || I.vsamp[2] != 1)
          return refuse(&I, RTPOSE_JPEG_R_SAMPLING);
        const int hv = I.hsamp[0] * 16 + I.vsamp[0];
        if (hv == 0x11) I.mode = RTPOSE_JPEG_444;
        else if (hv == 0x21) I.mode = RTPOSE_JPEG_422;
        else if (hv == 0x22) I.mode = RTPOSE_JPEG_420;
        else if (hv == 0x12) I.mode = RTPOSE_JPEG_440;
        else return refuse(&I, RTPOSE_JPEG_R_SAMPLING);
      }
      const int hmax = I.hsamp[0], vmax = I.vsamp[0];
      I.mcus_x = (I.width + 8 * hmax - 1) / (8 * hmax);
      I.mcus_y = (I.height + 8 * vmax - 1) / (8 * vmax);
      uint64_t words = 0;
      for (int c = 0; c < nc; ++c) {
        I.blocks_x[c] = I.mcus_x * I.hsamp[c];
        I.blocks_y[c] = I.mcus_y * I.vsamp[c];
        I.coef_offset[c] = words;
        words += (uint64_t)I.blocks_x[c] * (uint64_t)I.blocks_y[c] * 64u;
      }
      I.coef_count = words;  // at most 3 * 2048^2 * 64 < 2^30
      frame = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
      // extended, progressive, lossless, differential or arithmetic frames; arithmetic conditioning; the JPG marker
      return refuse(&I, RTPOSE_JPEG_R_FRAME);
    } else if (m == 0xC4) {  // DHT: several tables may share a segment
      while (n > 0) {
        if (n < 17) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        const int tc = s[0] >> 4, th = s[0] & 15;
        if (tc > 1 || th > 3) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        Huff& h = tc ? P.ac[th] : P.dc[th];
        int total = 0;
        h.counts[0] = 0;
        for (int l = 1; l <= 16; ++l) total += (h.counts[l] = s[l]);
        if (total > 256 || (size_t)total > n - 17) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        memcpy(h.vals, s + 17, (size_t)total);
        h.total = total;
        h.defined = false;
        if (!build(h, tc == 1)) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        h.defined = true;
        s += 17 + total;
        n -= 17 + (size_t)total;
      }
    } else if (m == 0xDB) {  // DQT
      while (n > 0) {
        const int pq = s[0] >> 4, t = s[0] & 15;
        if (pq == 1) return refuse(&I, RTPOSE_JPEG_R_QTABLE16);
        if (pq > 1 || t > 3) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        if (n < 65) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        for (int k = 0; k < 64; ++k) {
          if (s[1 + k] == 0) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
          P.q[t][kNatural[k]] = s[1 + k];
        }
        P.q_defined[t] = true;
        s += 65;
        n -= 65;
      }
    } else if (m == 0xDD) {  // DRI
      if (n != 2) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      I.restart_interval = (int32_t)be16(s);
    } else if (m == 0xDC) {
      return refuse(&I, RTPOSE_JPEG_R_DNL);
    } else if (m == 0xEE) {  // APP14: an Adobe segment sets the colour transform
      if (n >= 5 && memcmp(s, "Adobe", 5) == 0) return refuse(&I, RTPOSE_JPEG_R_ADOBE);
    } else if (m == 0xDA) {  // SOS
      if (!frame) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      const int nc = I.components;
      if (n < 1) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      if (s[0] != nc) return refuse(&I, s[0] >= 1 && s[0] <= 4 ? RTPOSE_JPEG_R_SCANS : RTPOSE_JPEG_R_SYNTAX);
      if (n != (size_t)(4 + 2 * nc)) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      for (int c = 0; c < nc; ++c) {
        if (s[1 + 2 * c] != ids[c]) return refuse(&I, RTPOSE_JPEG_R_SCANS);  // the frame's components in the frame's order
        P.td[c] = s[2 + 2 * c] >> 4;
        P.ta[c] = s[2 + 2 * c] & 15;
        if (P.td[c] > 3 || P.ta[c] > 3) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
        if (!P.dc[P.td[c]].defined || !P.ac[P.ta[c]].defined || !P.q_defined[P.tq[c]])
          return refuse(&I, RTPOSE_JPEG_R_TABLE);
        const Huff& d = P.dc[P.td[c]];
        for (int i = 0; i < d.total; ++i)
          if (d.vals[i] > 15) return refuse(&I, RTPOSE_JPEG_R_SYNTAX);
      }
      const uint8_t* t = s + 1 + 2 * nc;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) return refuse(&I, RTPOSE_JPEG_R_FRAME);  // a spectral or successive scan
      P.scan = p;
      return 0;
    }
    // APPn, COM and anything else with a length: skipped
  }
}

// ---- the bit reader: MSB first in a left-aligned 64-bit window ------------------------------------------------------
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc = 0;
  int bits = 0;  // valid bits at the top of acc; everything below them is 0
  int fake = 0;  // how many of them are zeros supplied behind the data's end or in front of a marker

  void refill() {
    if (fake == 0 && end - p >= 8) {
      uint64_t v;
      memcpy(&v, p, 8);
      const uint64_t nv = ~v;  // a byte of v is 0xFF where a byte of nv is 0: the classic zero-byte test
      if (((nv - 0x0101010101010101ull) & ~nv & 0x8080808080808080ull) == 0) {  // eight plain bytes at once
        const int k = (64 - bits) >> 3;
        if (k > 0) {
          uint64_t be = __builtin_bswap64(v);
          if (k < 8) be &= ~0ull << (64 - 8 * k);
          acc |= be >> bits;
          bits += 8 * k;
          p += k;
        }
        return;
      }
    }
    while (bits <= 56) {
      if (fake == 0 && p < end) {
        const unsigned b = *p;
        if (b != 0xFF) {
          acc |= (uint64_t)b << (56 - bits);
          bits += 8;
          ++p;
          continue;
        }
        if (end - p >= 2 && p[1] == 0x00) {  // a stuffed FF
          acc |= (uint64_t)0xFF << (56 - bits);
          bits += 8;
          p += 2;
          continue;
        }
      }
      // a marker, or the end of the data: zeros from here on, counted
      fake += 64 - bits;
      bits = 64;
    }
  }
  inline unsigned peek(int n) const { return (unsigned)(acc >> (64 - n)); }
  inline void drop(int n) {
    acc <<= n;
    bits -= n;
  }
};

// one Huffman symbol; -1 for a code in no table
inline int symbol(Bits& b, const Huff& h) {
  const int e = h.look[b.peek(kLook)];
  if (e) {
    b.drop(e >> 8);
    return e & 255;
  }
  for (int l = kLook + 1; l <= 16; ++l) {
    const int code = (int)b.peek(l);
    if (code <= h.maxcode[l]) {
      b.drop(l);
      return h.vals[h.valptr[l] + code - h.mincode[l]];
    }
  }
  return -1;
}

inline int receive_extend(Bits& b, int s) {
  int v = (int)b.peek(s);
  b.drop(s);
  if (v < (1 << (s - 1))) v -= (1 << s) - 1;
  return v;
}

inline bool in_int16(int v) { return v >= -32768 && v <= 32767; }

// one 8 x 8 block into `out` (zeroed by the caller), natural order, quantised
inline int block(Bits& b, const Huff& dc, const Huff& ac, const uint16_t* q, int& pred, int16_t* out) {
  if (b.bits < 32) b.refill();
  int s = symbol(b, dc);
  if (s < 0) return RTPOSE_JPEG_R_CODE;
  if (s > 11) return RTPOSE_JPEG_R_CATEGORY;
  if (s) {
    pred += receive_extend(b, s);
    if (!in_int16(pred)) return RTPOSE_JPEG_R_RANGE;
  }
  if (!in_int16(pred * (int)q[0])) return RTPOSE_JPEG_R_RANGE;
  out[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    if (b.bits < 32) b.refill();
    int v;
    const int f = ac.fast[b.peek(kLook)];
    if (f) {
      k += (f >> 8) & 15;
      b.drop(f & 255);
      v = f >> 16;
    } else {
      const int rs = symbol(b, ac);
      if (rs < 0) return RTPOSE_JPEG_R_CODE;
      const int r = rs >> 4;
      s = rs & 15;
      if (s == 0) {
        if (r != 15) break;  // EOB
        k += 16;
        if (k > 63) return RTPOSE_JPEG_R_RUN;
        continue;
      }
      if (s > 10) return RTPOSE_JPEG_R_CATEGORY;
      k += r;
      v = receive_extend(b, s);
    }
    if (k > 63) return RTPOSE_JPEG_R_RUN;
    const int n = kNatural[k];
    if (!in_int16(v * (int)q[n])) return RTPOSE_JPEG_R_RANGE;
    out[n] = (int16_t)v;
    ++k;
  }
  return 0;
}

}  // namespace

extern "C" {

int rtpose_jpeg_probe(const void* data, size_t len, rtpose_jpeg_info* info) {
  if (!info) return RTPOSE_JPEG_R_ARGUMENT;
  Parsed P;
  const int rc = parse(static_cast<const uint8_t*>(data), len, P);
  const int reason = P.info.reason;
  *info = P.info;
  if (rc) {  // a refusal carries no geometry a caller could act on
    memset(info, 0, sizeof(*info));
    info->struct_bytes = (uint32_t)sizeof(*info);
    info->reason = reason;
  }
  return rc;
}

int rtpose_jpeg_entropy_decode(const void* data, size_t len, const rtpose_jpeg_info* info, int16_t* coef, size_t capacity,
                               uint16_t (*qtab)[64]) {
  if (!data || !info || !coef || !qtab) return RTPOSE_JPEG_R_ARGUMENT;
  if (info->struct_bytes != sizeof(rtpose_jpeg_info)) return RTPOSE_JPEG_R_ARGUMENT;
  Parsed P;
  if (const int rc = parse(static_cast<const uint8_t*>(data), len, P)) return rc;
  // the geometry is this call's own reading of the file; the caller's info only has to agree with it
  const rtpose_jpeg_info& I = P.info;
  if (info->reason != 0 || info->width != I.width || info->height != I.height || info->mode != I.mode ||
      info->coef_count != I.coef_count)
    return RTPOSE_JPEG_R_ARGUMENT;
  if (capacity < I.coef_count) return RTPOSE_JPEG_R_CAPACITY;
  memset(coef, 0, (size_t)I.coef_count * sizeof(int16_t));
  const int nc = I.components;
  const uint8_t* bytes = static_cast<const uint8_t*>(data);
  Bits b;
  b.p = bytes + P.scan;
  b.end = bytes + len;
  int pred[3] = {0, 0, 0};
  const Huff* dc[3];
  const Huff* ac[3];
  const uint16_t* q[3];
  for (int c = 0; c < nc; ++c) {
    dc[c] = &P.dc[P.td[c]];
    ac[c] = &P.ac[P.ta[c]];
    q[c] = P.q[P.tq[c]];
  }
  const long long mcus = (long long)I.mcus_x * I.mcus_y;
  const int interval = I.restart_interval;
  int until_restart = interval, next_rst = 0;
  long long done = 0;
  for (int my = 0; my < I.mcus_y; ++my)
    for (int mx = 0; mx < I.mcus_x; ++mx) {
      for (int c = 0; c < nc; ++c)
        for (int v = 0; v < I.vsamp[c]; ++v)
          for (int h = 0; h < I.hsamp[c]; ++h) {
            const size_t by = (size_t)my * I.vsamp[c] + v, bx = (size_t)mx * I.hsamp[c] + h;
            int16_t* out = coef + I.coef_offset[c] + (by * (size_t)I.blocks_x[c] + bx) * 64;
            // what the zeros behind the data's end decode to is not the file's fault: that is a truncation
            if (const int rc = block(b, *dc[c], *ac[c], q[c], pred[c], out))
              return b.bits < b.fake ? (int)RTPOSE_JPEG_R_TRUNCATED : rc;
          }
      if (b.bits < b.fake) return RTPOSE_JPEG_R_TRUNCATED;  // the MCU used bits the file does not have
      ++done;
      if (interval && --until_restart == 0 && done < mcus) {
        // the rest of the last byte is padding; a whole unread byte in front of the marker is not this format
        if (b.bits - b.fake >= 8) return RTPOSE_JPEG_R_RST;
        const uint8_t* p = b.p;
        if (b.end - p < 2) return RTPOSE_JPEG_R_TRUNCATED;
        if (p[0] != 0xFF) return RTPOSE_JPEG_R_RST;
        while (b.end - p >= 2 && p[1] == 0xFF) ++p;
        if (b.end - p < 2) return RTPOSE_JPEG_R_TRUNCATED;
        if (p[1] != 0xD0 + next_rst) return RTPOSE_JPEG_R_RST;
        next_rst = (next_rst + 1) & 7;
        b.p = p + 2;
        b.acc = 0;
        b.bits = b.fake = 0;
        pred[0] = pred[1] = pred[2] = 0;
        until_restart = interval;
      }
    }
  // behind the last MCU: padding, then EOI.  Another scan, a DNL segment or anything else is not the served subset
  if (b.bits - b.fake >= 8) return RTPOSE_JPEG_R_TRAILING;
  const uint8_t* p = b.p;
  if (b.end - p < 2) return RTPOSE_JPEG_R_TRUNCATED;
  if (p[0] != 0xFF) return RTPOSE_JPEG_R_TRAILING;
  while (b.end - p >= 2 && p[1] == 0xFF) ++p;
  if (b.end - p < 2) return RTPOSE_JPEG_R_TRUNCATED;
  if (p[1] == 0xDA) return RTPOSE_JPEG_R_SCANS;
  if (p[1] == 0xDC) return RTPOSE_JPEG_R_DNL;
  if (p[1] >= 0xD0 && p[1] <= 0xD7) return RTPOSE_JPEG_R_RST;
  if (p[1] != 0xD9) return RTPOSE_JPEG_R_TRAILING;
  for (int c = 0; c < 3; ++c) memcpy(qtab[c], q[c < nc ? c : 0], 64 * sizeof(uint16_t));
  return 0;
}

const char* rtpose_jpeg_reason_text(int reason) {
  switch (reason) {
    case 0: return "served";
    case RTPOSE_JPEG_R_ARGUMENT: return "a NULL pointer, or an info that is not rtpose_jpeg_probe's for this file";
    case RTPOSE_JPEG_R_NOT_JPEG: return "not a JPEG file (no SOI marker)";
    case RTPOSE_JPEG_R_SYNTAX: return "a malformed marker segment";
    case RTPOSE_JPEG_R_TRUNCATED: return "the data ends before the last MCU and its EOI marker";
    case RTPOSE_JPEG_R_FRAME: return "not a baseline (SOF0, Huffman, sequential) frame";
    case RTPOSE_JPEG_R_PRECISION: return "sample precision other than 8 bits";
    case RTPOSE_JPEG_R_QTABLE16: return "a 16-bit quantiser table";
    case RTPOSE_JPEG_R_COMPONENTS: return "neither one nor three components";
    case RTPOSE_JPEG_R_ADOBE: return "an Adobe APP14 segment";
    case RTPOSE_JPEG_R_COLORSPACE: return "component ids R, G, B: not a YCbCr file";
    case RTPOSE_JPEG_R_SAMPLING: return "sampling factors other than gray 1x1 or luma 1x1, 2x1, 2x2, 1x2 over chroma 1x1";
    case RTPOSE_JPEG_R_SCANS: return "more than one scan, or a scan that does not interleave all components";
    case RTPOSE_JPEG_R_DNL: return "a DNL segment (height defined after the scan)";
    case RTPOSE_JPEG_R_SIZE: return "width or height outside 1..16384";
    case RTPOSE_JPEG_R_CATEGORY: return "a DC category above 11 or an AC size above 10";
    case RTPOSE_JPEG_R_RUN: return "a zero run past coefficient 63";
    case RTPOSE_JPEG_R_CODE: return "a Huffman code that is in no table";
    case RTPOSE_JPEG_R_TABLE: return "the scan selects a Huffman or quantiser table that was never defined";
    case RTPOSE_JPEG_R_RST: return "a missing, misplaced or wrongly numbered RSTn marker";
    case RTPOSE_JPEG_R_CAPACITY: return "capacity below the file's coefficient count";
    case RTPOSE_JPEG_R_RANGE: return "a coefficient times its quantiser entry lies outside int16";
    case RTPOSE_JPEG_R_TRAILING: return "bytes other than an EOI marker behind the last MCU";
    default: return "unknown reason";
  }
}

}  // extern "C"
