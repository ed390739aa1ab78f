// san_bamread — stand-alone driver for the host BAM reader (mitty_amd/csrc/mh_bamread.cpp), built by
// tests/test_score_cpu.py with -fsanitize=address,undefined and fed truncated, bit-flipped and absurd-length BAMs.
//   san_bamread <file> <threads> <chunk bytes>
// Prints "ok <records> <bytes> <checksum>" or "error <message>" and exits 0 either way: a malformed file must come
// back as an error return, and any read past a buffer is the sanitizer's report (non-zero exit).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/mitty_hip.h"

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  mh_bamfile *f = nullptr;
  int32_t rc = mh_bamfile_open(argv[1], atoi(argv[2]), &f);
  if (rc != MH_OK) {
    printf("error %s\n", mh_bamfile_error(f));
    mh_bamfile_close(f);
    return 0;
  }
  const char *text, *names;
  const int64_t *lens;
  int64_t text_len;
  int32_t n_ref;
  if (mh_bamfile_header(f, &text, &text_len, &n_ref, &names, &lens) != MH_OK) return 3;
  uint64_t sum = 0;
  for (int64_t i = 0; i < text_len; i++) sum += (uint8_t)text[i];
  for (int32_t r = 0; r < n_ref; r++) {
    sum += strlen(names) + (uint64_t)lens[r];
    names += strlen(names) + 1;
  }
  int64_t total = 0, bytes = 0;
  for (;;) {
    const uint8_t *recs;
    const int64_t *roff;
    int64_t len, n;
    rc = mh_bamfile_next(f, atoll(argv[3]), &recs, &len, &roff, &n);
    if (rc != MH_OK) {
      printf("error %s\n", mh_bamfile_error(f));
      mh_bamfile_close(f);
      return 0;
    }
    if (n == 0) break;
    if (roff[0] != 0 || roff[n] != len) return 4;
    for (int64_t i = 0; i < n; i++) {
      // what a consumer reads of a checked record: every byte, and the name as a C string
      const uint8_t *p = recs + roff[i];
      const int64_t size = roff[i + 1] - roff[i];
      for (int64_t k = 0; k < size; k++) sum += p[k];
      sum += strlen((const char *)p + 36);
      const int64_t lrn = p[12], ncig = p[16] | p[17] << 8;
      int32_t lseq;
      memcpy(&lseq, p + 20, 4);
      if (36 + lrn + 4 * ncig + (lseq + 1) / 2 + lseq > size) return 5;
    }
    total += n;
    bytes += len;
  }
  printf("ok %lld %lld %llu\n", (long long)total, (long long)bytes, (unsigned long long)sum);
  mh_bamfile_close(f);
  return 0;
}
