// The rules of btsbot_decode_stamps (btsbot_amd/csrc/inflate_core.h) as a host program, for tests/test_stamp_decode_host.py
// and for a run under the sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o tools/unit/stamp_decode_check tools/unit/stamp_decode_check.cpp
//   tools/unit/stamp_decode_check stamps.bin results.bin
//
// stamps.bin:  uint32 n, then n x (uint32 length, bytes)                                  (little-endian)
// results.bin: per stamp  uint8 container status (gzip + deflate + trailer alone), uint8 status (the kernel's),
//              int32 h, int32 w, uint32 bytes inflated, those bytes when the container status is 0, and the
//              63 x 63 float32 frame (native order, image top-left, zero elsewhere) when the status is 0.
// Every stamp is copied into a heap block of exactly its length and inflated into one of exactly STAMP_CAP bytes, so a
// read or write one byte out of bounds is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../btsbot_amd/csrc/inflate_core.h"

using namespace stamp_core;

static bool read_u32(FILE* f, uint32_t& v) {
  unsigned char b[4];
  if (fread(b, 1, 4, f) != 4) return false;
  v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  return true;
}

static void write_u32(FILE* f, uint32_t v) {
  const unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
  fwrite(b, 1, 4, f);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s stamps.bin results.bin\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* res = in ? fopen(argv[2], "wb") : nullptr;
  uint32_t n = 0;
  if (!in || !res || !read_u32(in, n)) {
    fprintf(stderr, "%s: cannot open the files or read the count\n", argv[0]);
    return 2;
  }
  const int plane = STAMP_SIDE * STAMP_SIDE;
  std::vector<unsigned char> frame((size_t)plane * 4);
  for (uint32_t s = 0; s < n; ++s) {
    uint32_t len = 0;
    if (!read_u32(in, len)) return 2;
    uint8_t* stamp = (uint8_t*)malloc(len ? len : 1);
    uint8_t* outbuf = (uint8_t*)malloc(STAMP_CAP);
    Tables* tables = (Tables*)malloc(sizeof(Tables));
    if (!stamp || !outbuf || !tables || fread(stamp, 1, len, in) != len) return 2;
    const Linear out{outbuf};
    uint32_t outn = 0, data_off = 0;
    int h = 0, w = 0;
    const int gz = gunzip(stamp, (int64_t)len, out, outn, *tables);
    int st = gz;
    if (st == ST_OK) st = parse_fits(out, outn, h, w, data_off);
    if (st != ST_OK) h = w = 0;
    fputc(gz, res);
    fputc(st, res);
    write_u32(res, (uint32_t)h);
    write_u32(res, (uint32_t)w);
    write_u32(res, outn);
    if (gz == ST_OK) fwrite(outbuf, 1, outn, res);
    if (st == ST_OK) {
      memset(frame.data(), 0, frame.size());
      for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
          const uint8_t* be = outbuf + data_off + 4 * (size_t)(r * w + c);
          const uint32_t v = ((uint32_t)be[0] << 24) | ((uint32_t)be[1] << 16) | ((uint32_t)be[2] << 8) | (uint32_t)be[3];
          memcpy(frame.data() + 4 * (size_t)(r * STAMP_SIDE + c), &v, 4);
        }
      fwrite(frame.data(), 1, frame.size(), res);
    }
    free(tables);
    free(outbuf);
    free(stamp);
  }
  fclose(in);
  if (fclose(res) != 0) return 2;
  return 0;
}
