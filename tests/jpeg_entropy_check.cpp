// Stand-alone check of csrc/jpeg_entropy.h for the sanitizers (tests/test_jpegdec_host.py compiles it with the host compiler under
// -fsanitize=address,undefined and runs it as a child process; nothing of it is ever loaded into Python).
//
//   jpeg_entropy_check FILE...
//
// Every FILE is a (possibly damaged) JPEG stream.  Each is copied into a heap block of exactly its size, so that a read past the end
// is a sanitizer report, and decoded into a heap block of exactly the size the header asks for, likewise for writes; then once more
// into a block one byte too small, which must be refused.  A file whose name contains "_bad" must not decode.  Prints one line per
// file, exits 0 unless an expectation fails (a sanitizer report aborts with its own status).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../mopa_amd/csrc/jpeg_entropy.h"

int main(int argc, char** argv) {
  int failures = 0, ok = 0, data = 0, unsupported = 0;
  for (int i = 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* in = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
    if (n > 0 && fread(in, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
    fclose(f);
    uint8_t* exact = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);      // a block of exactly n bytes
    memcpy(exact, in, (size_t)n);
    free(in);

    JpegParsed P;
    const int rc_info = jpeg_parse(exact, n, P);
    int rc = rc_info;
    if (rc_info == MOPA_OK) {
      const int64_t need = P.h.coeff_bytes;
      int16_t* out = (int16_t*)malloc((size_t)need);
      JpegHeader h;
      rc = jpeg_entropy_decode(exact, n, &h, out, need);
      if (rc == MOPA_OK && memcmp(&h, &P.h, sizeof(h)) != 0) { printf("%s: the two headers differ\n", argv[i]); ++failures; }
      free(out);
      int16_t* small = (int16_t*)malloc((size_t)need - 2);
      if (jpeg_entropy_decode(exact, n, &h, small, need - 2) != MOPA_ERR_ARG) { printf("%s: a short buffer was accepted\n", argv[i]); ++failures; }
      free(small);
    }
    if (rc != MOPA_OK && rc != MOPA_ERR_DATA && rc != MOPA_ERR_UNSUPPORTED) { printf("%s: code %d\n", argv[i], rc); ++failures; }
    if (strstr(argv[i], "_bad") && rc == MOPA_OK) { printf("%s: decoded\n", argv[i]); ++failures; }
    if (strstr(argv[i], "_good") && rc != MOPA_OK) { printf("%s: code %d\n", argv[i], rc); ++failures; }
    ok += rc == MOPA_OK; data += rc == MOPA_ERR_DATA; unsupported += rc == MOPA_ERR_UNSUPPORTED;
    free(exact);
  }
  printf("%d files: %d decoded, %d malformed, %d unsupported, %d failures\n", argc - 1, ok, data, unsupported, failures);
  return failures ? 1 : 0;
}
