// The rules of btsbot_decode_stamps in one place: a gzip member (RFC 1952) around a raw deflate stream (RFC 1951)
// around a single-HDU FITS image.  Plain C++ that compiles as device code under hipcc (stamp_decode.hip: one stamp per
// lane) and as host code under any C++17 compiler (tools/unit/stamp_decode_check.cpp, the program the host test and the
// sanitizers run).  Nothing else decides what is accepted.
//
// What is accepted is what zlib's inflate accepts (inftrees.c / inflate.c), restated:
//   * block types stored, fixed and dynamic, any number of blocks; type 3 is an error;
//   * a dynamic block with HLIT > 286 or HDIST > 30 is an error; the code-length code must be complete; an
//     over-subscribed set is an error; an incomplete literal/length or distance set is an error unless it is a single
//     code of length 1 (Z_RLE and Z_HUFFMAN_ONLY streams carry such distance sets); a set without any code is fine
//     until a symbol is asked of it; the end-of-block code must have a length; a repeat with nothing before it or past
//     the end of the sets is an error;
//   * length symbols 286 / 287 and distance symbols 30 / 31 are errors; a distance is valid iff it is <= the bytes
//     produced so far (the stream starts with an empty window, and STAMP_CAP < 32 KiB makes the output the window).
// Departures from gzip.decompress, on purpose: the CRC32 of the trailer is NOT verified (ISIZE is), reserved FLG bits
// are refused, and bytes after the first member's trailer (a second member, padding) are UNSUPPORTED, not decoded.
//
// Safety.  Every read of the input is inside [0, len) of the stamp, every write and read of the output inside
// [0, STAMP_CAP); the bit reader never reads past the end -- running dry is BAD_DEFLATE; every loop consumes at least
// one input bit or produces at least one byte per iteration, or ends.  The input is read in bytes and in aligned 32-bit
// words that lie wholly inside the stamp, never in unaligned wide loads (stamps start at arbitrary byte offsets of the
// blob).  The output goes through an accessor (Out::get / Out::put), so that the
// kernel can interleave the outputs of the lanes of a wave in memory while the host program uses a plain array.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BTS_HD __host__ __device__
#else
#define BTS_HD
#endif

namespace stamp_core {

enum Status : int {
  ST_OK = 0,
  ST_BAD_GZIP = 1,      // not a gzip member: magic, method, reserved flags, a header that runs past the stamp
  ST_BAD_DEFLATE = 2,   // the deflate stream breaks a rule above, or ends early
  ST_TOO_LARGE = 3,     // more than STAMP_CAP bytes
  ST_BAD_TRAILER = 4,   // no 8-byte trailer, or ISIZE != bytes produced
  ST_BAD_FITS = 5,      // no END card within the output, or the data unit is shorter than the header says
  ST_UNSUPPORTED = 6    // well-formed, but outside what the device decodes: left to the host path
};

// up to four 2880-byte header blocks + the 17,280-byte data unit of a 63 x 63 float32 image
constexpr int STAMP_CAP = 28800;
constexpr int STAMP_SIDE = 63;

// canonical Huffman codes as counts per length + symbols in code order (the form of zlib's contrib/puff), and the
// code lengths of the block being read.  1020 bytes: 255 words, an odd stride for the per-lane copies in LDS
struct Tables {
  uint16_t lencnt[16], distcnt[16];
  uint16_t lensym[288];
  uint16_t distsym[30];
  uint8_t lengths[320];
};

struct Linear {   // the host's output: a plain array of STAMP_CAP bytes
  uint8_t* p;
  BTS_HD uint8_t get(uint32_t i) const { return p[i]; }
  BTS_HD void put(uint32_t i, uint8_t v) const { p[i] = v; }
};

// The bit reader.  Whole aligned 32-bit words are read where the stamp has them (a stamp starts at any byte: the bytes
// up to the first aligned address and the last few are read one at a time), and the next word is requested one refill
// before its bits are needed, so that its latency passes behind the symbols still in `hold`.
struct Bits {
  const uint8_t* p;
  int64_t pos, end;   // pos: the first byte that is in neither hold nor ahead
  uint64_t hold;
  int n;              // bits in hold
  uint32_t ahead;     // the word behind hold's bits, when has_ahead
  bool has_ahead;
  bool dry;           // asked for bits the stamp does not have
  BTS_HD static uint32_t load_word(const uint8_t* q) {
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(q, 4), 4);
    return v;
  }
  BTS_HD void refill() {
    for (;;) {
      if (has_ahead && n <= 32) {
        hold |= (uint64_t)ahead << n;
        n += 32;
        has_ahead = false;
      }
      if (has_ahead || pos >= end) return;
      if ((reinterpret_cast<uintptr_t>(p + pos) & 3u) == 0 && end - pos >= 4) {
        ahead = load_word(p + pos);
        pos += 4;
        has_ahead = true;
      } else if (n <= 56) {
        hold |= (uint64_t)p[pos++] << n;
        n += 8;
      } else {
        return;
      }
    }
  }
  BTS_HD uint32_t take(int k) {   // k <= 16
    if (n < k) refill();
    if (n < k) {
      dry = true;
      return 0;
    }
    const uint32_t v = (uint32_t)hold & ((1u << k) - 1u);
    hold >>= k;
    n -= k;
    return v;
  }
  BTS_HD void unread() {   // whole bytes read ahead go back to the stream; the bits of a started byte are dropped
    pos -= (n >> 3) + (has_ahead ? 4 : 0);
    hold = 0;
    n = 0;
    has_ahead = false;
  }
};

enum { SET_CODES = 0, SET_LENS = 1, SET_DISTS = 2, SET_FIXED = 3 };

// counts and symbols from `n` code lengths; false when zlib's inflate_table refuses the set
BTS_HD inline bool construct(uint16_t* cnt, uint16_t* sym, const uint8_t* lengths, int n, int kind) {
  for (int l = 0; l < 16; ++l) cnt[l] = 0;
  for (int s = 0; s < n; ++s) cnt[lengths[s]] += 1;
  int left = 1, maxlen = 0;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - (int)cnt[l];
    if (left < 0) return false;   // over-subscribed
    if (cnt[l]) maxlen = l;
  }
  if (kind != SET_FIXED) {
    if (maxlen == 0) {
      if (kind == SET_CODES) return false;   // zlib reads every length as 0 then and misses the end-of-block code
    } else if (left > 0 && (kind == SET_CODES || maxlen != 1)) {
      return false;   // incomplete
    }
  }
  uint16_t offs[16];
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
  for (int s = 0; s < n; ++s)
    if (lengths[s] != 0) sym[offs[lengths[s]]++] = (uint16_t)s;
  return true;
}

// one symbol; -1: the bits are no code of the set (or the stamp ran dry: b.dry)
BTS_HD inline int decode(Bits& b, const uint16_t* cnt, const uint16_t* sym) {
  if (b.n < 15) b.refill();
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    if (b.n == 0) {
      b.dry = true;
      return -1;
    }
    code |= (int)(b.hold & 1u);
    b.hold >>= 1;
    b.n -= 1;
    const int count = cnt[l];
    if (code - count < first) return sym[index + (code - first)];
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -1;
}

constexpr uint64_t pack_order(int from, int to) {   // the order of the code-length code lengths, 5 bits each
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint64_t v = 0;
  for (int i = from; i < to; ++i) v |= (uint64_t)order[i] << (5 * (i - from));
  return v;
}

// literals, lengths and distances of one block until its end-of-block code
template <class Out>
BTS_HD inline int codes(Bits& b, const Out& out, uint32_t& outn, const Tables& t) {
  for (;;) {
    int s = decode(b, t.lencnt, t.lensym);
    if (s < 0) return ST_BAD_DEFLATE;
    if (s < 256) {
      if (outn >= (uint32_t)STAMP_CAP) return ST_TOO_LARGE;
      out.put(outn++, (uint8_t)s);
      continue;
    }
    if (s == 256) return ST_OK;
    s -= 257;
    if (s >= 29) return ST_BAD_DEFLATE;
    uint32_t len;
    if (s < 8) {
      len = 3u + (uint32_t)s;
    } else if (s == 28) {
      len = 258u;
    } else {
      const int e = (s - 4) >> 2;
      len = 3u + ((4u + (uint32_t)(s & 3)) << e) + b.take(e);
    }
    const int d = decode(b, t.distcnt, t.distsym);
    if (d < 0 || d >= 30) return ST_BAD_DEFLATE;
    uint32_t dist;
    if (d < 4) {
      dist = 1u + (uint32_t)d;
    } else {
      const int e = (d >> 1) - 1;
      dist = 1u + ((2u + (uint32_t)(d & 1)) << e) + b.take(e);
    }
    if (b.dry || dist > outn) return ST_BAD_DEFLATE;
    if (outn + len > (uint32_t)STAMP_CAP) return ST_TOO_LARGE;
    // the copy, eight bytes at a time: the source bytes of a chunk are read before any of it is written (one wait for
    // the reads, not one per byte); a distance below 8 repeats a pattern that is read once
    if (dist < 8u) {
      uint64_t v = 0;
      for (uint32_t j = 0; j < dist; ++j) v |= (uint64_t)out.get(outn - dist + j) << (8 * j);
      for (uint32_t k = 0, j = 0; k < len; ++k, ++outn) {
        out.put(outn, (uint8_t)(v >> (8 * j)));
        j = j + 1 == dist ? 0 : j + 1;
      }
    } else {
      while (len != 0) {
        const uint32_t m = len < 8u ? len : 8u;
        uint64_t v = 0;
        for (uint32_t j = 0; j < m; ++j) v |= (uint64_t)out.get(outn - dist + j) << (8 * j);
        for (uint32_t j = 0; j < m; ++j) out.put(outn + j, (uint8_t)(v >> (8 * j)));
        outn += m;
        len -= m;
      }
    }
  }
}

BTS_HD inline bool dynamic_tables(Bits& b, Tables& t) {
  const int nlen = (int)b.take(5) + 257, ndist = (int)b.take(5) + 1, ncode = (int)b.take(4) + 4;
  if (b.dry || nlen > 286 || ndist > 30) return false;
  constexpr uint64_t lo = pack_order(0, 12), hi = pack_order(12, 19);
  for (int i = 0; i < 19; ++i) t.lengths[i] = 0;
  for (int i = 0; i < ncode; ++i) {
    const int at = (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
    t.lengths[at] = (uint8_t)b.take(3);
  }
  if (b.dry || !construct(t.lencnt, t.lensym, t.lengths, 19, SET_CODES)) return false;
  int idx = 0;
  while (idx < nlen + ndist) {
    const int s = decode(b, t.lencnt, t.lensym);
    if (s < 0) return false;
    if (s < 16) {
      t.lengths[idx++] = (uint8_t)s;
      continue;
    }
    int prev = 0, rep;
    if (s == 16) {
      if (idx == 0) return false;
      prev = t.lengths[idx - 1];
      rep = 3 + (int)b.take(2);
    } else if (s == 17) {
      rep = 3 + (int)b.take(3);
    } else {
      rep = 11 + (int)b.take(7);
    }
    if (b.dry || idx + rep > nlen + ndist) return false;
    while (rep--) t.lengths[idx++] = (uint8_t)prev;
  }
  if (t.lengths[256] == 0) return false;
  // (the code-length code is done with: its counts and symbols are overwritten)
  return construct(t.distcnt, t.distsym, t.lengths + nlen, ndist, SET_DISTS) &&
         construct(t.lencnt, t.lensym, t.lengths, nlen, SET_LENS);
}

BTS_HD inline void fixed_tables(Tables& t) {
  int s = 0;
  for (; s < 144; ++s) t.lengths[s] = 8;
  for (; s < 256; ++s) t.lengths[s] = 9;
  for (; s < 280; ++s) t.lengths[s] = 7;
  for (; s < 288; ++s) t.lengths[s] = 8;
  (void)construct(t.lencnt, t.lensym, t.lengths, 288, SET_FIXED);
  for (s = 0; s < 30; ++s) t.lengths[s] = 5;
  (void)construct(t.distcnt, t.distsym, t.lengths, 30, SET_FIXED);
}

// raw deflate from b.pos on; afterwards b.pos is the first byte behind the stream
template <class Out>
BTS_HD inline int inflate(Bits& b, const Out& out, uint32_t& outn, Tables& t) {
  outn = 0;
  for (;;) {
    const uint32_t last = b.take(1), type = b.take(2);
    if (b.dry) return ST_BAD_DEFLATE;
    if (type == 0) {
      b.take(b.n & 7);   // to the byte boundary
      const uint32_t len = b.take(16), nlen = b.take(16);
      if (b.dry || len != (~nlen & 0xffffu)) return ST_BAD_DEFLATE;
      b.unread();   // the block's bytes are read in place
      if ((int64_t)len > b.end - b.pos) return ST_BAD_DEFLATE;
      if (outn + len > (uint32_t)STAMP_CAP) return ST_TOO_LARGE;
      for (uint32_t k = 0; k < len; ++k) out.put(outn++, b.p[b.pos++]);
    } else if (type == 3) {
      return ST_BAD_DEFLATE;
    } else {
      if (type == 1) fixed_tables(t);
      else if (!dynamic_tables(b, t)) return ST_BAD_DEFLATE;
      const int st = codes(b, out, outn, t);
      if (st != ST_OK) return st;
    }
    if (last) break;
  }
  b.unread();
  return ST_OK;
}

// one gzip member, alone in [in, in + len): header, deflate stream, trailer.  outn = bytes produced (also on failure:
// how far it came)
template <class Out>
BTS_HD inline int gunzip(const uint8_t* in, int64_t len, const Out& out, uint32_t& outn, Tables& t) {
  outn = 0;
  if (len < 10 || in[0] != 0x1f || in[1] != 0x8b || in[2] != 8 || (in[3] & 0xe0) != 0) return ST_BAD_GZIP;
  const int flg = in[3];
  int64_t pos = 10;
  if (flg & 4) {   // FEXTRA
    if (len - pos < 2) return ST_BAD_GZIP;
    const int64_t xlen = (int64_t)in[pos] | ((int64_t)in[pos + 1] << 8);
    pos += 2;
    if (len - pos < xlen) return ST_BAD_GZIP;
    pos += xlen;
  }
  for (int bit = 8; bit <= 16; bit <<= 1) {   // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (pos < len && in[pos] != 0) ++pos;
    if (pos >= len) return ST_BAD_GZIP;
    ++pos;
  }
  if (flg & 2) {   // FHCRC
    if (len - pos < 2) return ST_BAD_GZIP;
    pos += 2;
  }
  Bits b{in, pos, len, 0u, 0, 0u, false, false};
  const int st = inflate(b, out, outn, t);
  if (st != ST_OK) return st;
  if (len - b.pos < 8) return ST_BAD_TRAILER;
  const uint8_t* tr = in + b.pos + 4;
  const uint32_t isize = (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
  if (isize != outn) return ST_BAD_TRAILER;
  if (len - b.pos > 8) return ST_UNSUPPORTED;   // another member or padding: the host path reads those
  return ST_OK;
}

// ---- FITS primary header ------------------------------------------------------------------------------------------------
BTS_HD inline bool fits_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }

// the card's keyword (bytes 0..7 without the white space around it, as str.strip() sees it) against `name`
template <class Out>
BTS_HD inline bool fits_key_is(const Out& out, uint32_t card, const char* name) {
  int a = 0, z = 8;
  while (a < z && fits_space(out.get(card + a))) ++a;
  while (z > a && fits_space(out.get(card + z - 1))) --z;
  int i = 0;
  for (; a + i < z; ++i)
    if (name[i] == 0 || out.get(card + a + i) != (uint8_t)name[i]) return false;
  return name[i] == 0;
}

// blanks, an optional sign, 1-9 digits, then blanks up to the end of the card or a '/'
template <class Out>
BTS_HD inline bool fits_int(const Out& out, uint32_t card, int& value) {
  int i = 10;
  while (i < 80 && out.get(card + i) == ' ') ++i;
  bool neg = false;
  if (i < 80 && (out.get(card + i) == '-' || out.get(card + i) == '+')) neg = out.get(card + i++) == '-';
  int v = 0, nd = 0;
  for (; i < 80; ++i, ++nd) {
    const uint8_t c = out.get(card + i);
    if (c < '0' || c > '9') break;
    if (nd >= 9) return false;
    v = v * 10 + (c - '0');
  }
  if (nd == 0) return false;
  while (i < 80 && out.get(card + i) == ' ') ++i;
  if (i < 80 && out.get(card + i) != '/') return false;
  value = neg ? -v : v;
  return true;
}

// SIMPLE's value: blanks, T, blanks, then the end of the card or a '/'
template <class Out>
BTS_HD inline bool fits_true(const Out& out, uint32_t card) {
  int i = 10;
  while (i < 80 && out.get(card + i) == ' ') ++i;
  if (i >= 80 || out.get(card + i) != 'T') return false;
  ++i;
  while (i < 80 && out.get(card + i) == ' ') ++i;
  return i >= 80 || out.get(card + i) == '/';
}

// h, w and the byte offset of the data unit of the `n` output bytes, when this is an image the device decodes:
// SIMPLE = T, NAXIS = 2, BITPIX = -32, 1 <= NAXIS1, NAXIS2 <= 63, no BSCALE / BZERO card, the data unit all there.
// A later card of the same keyword replaces an earlier one, as in a dict of the cards
template <class Out>
BTS_HD inline int parse_fits(const Out& out, uint32_t n, int& h, int& w, uint32_t& data_off) {
  h = w = 0;
  data_off = 0;
  bool simple = false, unsupported = false, have[4] = {false, false, false, false};
  int val[4] = {0, 0, 0, 0};   // BITPIX, NAXIS, NAXIS1, NAXIS2
  for (uint32_t block = 0;; block += 2880u) {
    if (n < 2880u || block > n - 2880u) return ST_BAD_FITS;
    for (uint32_t card = block; card < block + 2880u; card += 80u) {
      if (fits_key_is(out, card, "END")) {
        data_off = block + 2880u;
        if (unsupported || !simple || !have[0] || !have[1] || !have[2] || !have[3]) return ST_UNSUPPORTED;
        if (val[0] != -32 || val[1] != 2 || val[2] < 1 || val[2] > STAMP_SIDE || val[3] < 1 || val[3] > STAMP_SIDE)
          return ST_UNSUPPORTED;
        if (n - data_off < (uint32_t)(val[2] * val[3] * 4)) return ST_BAD_FITS;
        w = val[2];
        h = val[3];
        return ST_OK;
      }
      if (out.get(card + 8) != '=' || out.get(card + 9) != ' ') continue;
      if (fits_key_is(out, card, "SIMPLE")) {
        simple = fits_true(out, card);
        if (!simple) unsupported = true;
      } else if (fits_key_is(out, card, "BSCALE") || fits_key_is(out, card, "BZERO")) {
        unsupported = true;
      } else {
        const char* names[4] = {"BITPIX", "NAXIS", "NAXIS1", "NAXIS2"};
        for (int k = 0; k < 4; ++k) {
          if (!fits_key_is(out, card, names[k])) continue;
          have[k] = fits_int(out, card, val[k]);
          if (!have[k]) unsupported = true;
        }
      }
    }
  }
}

}  // namespace stamp_core
