// Host run of the device inflater's decoder (mitty_amd/csrc/mh_inflate.h: bit reader, table builds, block loops,
// CRC-32 by slices) over a file of BGZF members.  Test infrastructure: built with -fsanitize=address,undefined and run
// directly by tests/test_inflate_cpu.py, which compares every verdict and every good member's bytes with zlib.
//   inflate_host IN OUT
//   IN:  per member  u32 clen, u32 isize, u32 crc, clen payload bytes (raw deflate)
//   OUT: per member  u32 status (mh::inf::ST_*), u32 n, n inflated bytes (n = isize when status is 0, else 0)
// Payload, output and tables are separate heap blocks of their exact sizes, so a read or write one byte out of range
// is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mitty_amd/csrc/mh_inflate.h"

using namespace mh::inf;

static uint32_t rd32(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: inflate_host IN OUT\n");
    return 2;
  }
  FILE *fi = fopen(argv[1], "rb");
  FILE *fo = fopen(argv[2], "wb");
  if (!fi || !fo) {
    fprintf(stderr, "cannot open files\n");
    return 2;
  }
  static const CrcPowers P = make_crc_powers();
  uint32_t *tab = (uint32_t *)malloc(256 * sizeof(uint32_t));
  for (uint32_t i = 0; i < 256; i++) tab[i] = crc_table_entry(i);
  long members = 0;
  uint8_t hdr[12];
  while (fread(hdr, 1, 12, fi) == 12) {
    const uint32_t clen = rd32(hdr), isize = rd32(hdr + 4), crc = rd32(hdr + 8);
    if (isize > (uint32_t)MAX_ISIZE) {
      fprintf(stderr, "member %ld: ISIZE %u\n", members, isize);
      return 2;
    }
    uint8_t *in = (uint8_t *)malloc(clen ? clen : 1), *out = (uint8_t *)malloc(isize ? isize : 1);
    Tables *T = (Tables *)malloc(sizeof(Tables));
    if (clen && fread(in, 1, clen, fi) != clen) {
      fprintf(stderr, "member %ld: short file\n", members);
      return 2;
    }
    if (!clen) {   // (an exact-size block: nothing of it may be read)
      free(in);
      in = (uint8_t *)malloc(0);
    }
    HostOut o{out};
    HostPolicy pol;
    uint32_t produced = 0;
    HostSource src{in};
    int32_t st = inflate_raw(src, in, (int64_t)clen, isize, o, *T, pol, &produced);
    if (st == ST_OK) {
      // the device's CRC: slices shared among 64 "lanes", XORed together
      uint32_t acc = 0, tail = 0;
      for (int lane = 0; lane < 64; lane++) {
        uint32_t a, t;
        crc_slices(out, (int)isize, P, tab, lane, 64, &a, &t);
        acc ^= a;
        tail ^= t;
      }
      if (crc_finish(acc, tail, (int)isize, P) != crc) st = ST_CRC;
    }
    const uint32_t rec[2] = {(uint32_t)st, st == ST_OK ? isize : 0};
    fwrite(rec, 4, 2, fo);
    if (st == ST_OK && isize) fwrite(out, 1, isize, fo);
    free(in);
    free(out);
    free(T);
    members++;
  }
  free(tab);
  fclose(fi);
  if (fclose(fo) != 0) return 2;
  fprintf(stderr, "members %ld\n", members);
  return 0;
}
