/* C caller of the Header::verify / Vote::verify crypto host forms, through
 * include/coa_verify.h alone (tests/test_gpu_messages.py builds and runs it on
 * a GPU).  Input file (little-endian), written by the test:
 *   u32 magic 0x4D414F43, nk, nh, nv, hbytes
 *   keys[nk][32]                      the committee to register
 *   header_offsets[nh + 1] (u64), header_data[hbytes]
 *   header ids[nh][32], authors[nh][32], sigs[nh][64], expected status[nh]
 *   vote ids[nv][32], rounds[nv] (u64), origins[nv][32], authors[nv][32],
 *   sigs[nv][64], expected verdicts[nv]
 * Both calls run with the committee registered, then with none registered
 * (every item through the uncached path): the outputs must equal the expected
 * ones both times.  Prints "message harness ok (<nh> headers, <nv> votes)". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "coa_verify.h"

static unsigned char* take(unsigned char** p, unsigned char* end, size_t bytes) {
  unsigned char* at = *p;
  if ((size_t)(end - at) < bytes) {
    fprintf(stderr, "vector file too short\n");
    exit(2);
  }
  *p = at + bytes;
  return at;
}

/* an aligned copy (the file's sections are not 8-byte aligned) */
static uint64_t* take_u64(unsigned char** p, unsigned char* end, size_t n) {
  uint64_t* out = malloc((n ? n : 1) * sizeof(uint64_t));
  if (!out) exit(2);
  memcpy(out, take(p, end, n * 8), n * 8);
  return out;
}

static int differ(const char* what, const uint8_t* got, const uint8_t* want, size_t n) {
  int bad = 0;
  for (size_t i = 0; i < n; i++)
    if (got[i] != want[i]) {
      if (bad++ < 8) fprintf(stderr, "%s[%zu]: got %u, expected %u\n", what, i, got[i], want[i]);
    }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s vectors.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* buf = malloc((size_t)size + 1);
  if (!buf || fread(buf, 1, (size_t)size, f) != (size_t)size) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  unsigned char *p = buf, *end = buf + size;
  uint32_t head[5];
  memcpy(head, take(&p, end, sizeof head), sizeof head);
  if (head[0] != 0x4D414F43u) {
    fprintf(stderr, "bad magic\n");
    return 2;
  }
  const size_t nk = head[1], nh = head[2], nv = head[3], hbytes = head[4];
  const uint8_t* keys = take(&p, end, nk * 32);
  uint64_t* hoff = take_u64(&p, end, nh + 1);
  const uint8_t* hdata = take(&p, end, hbytes);
  const uint8_t* hids = take(&p, end, nh * 32);
  const uint8_t* hauthors = take(&p, end, nh * 32);
  const uint8_t* hsigs = take(&p, end, nh * 64);
  const uint8_t* hexp = take(&p, end, nh);
  const uint8_t* vids = take(&p, end, nv * 32);
  uint64_t* vrounds = take_u64(&p, end, nv);
  const uint8_t* vorigins = take(&p, end, nv * 32);
  const uint8_t* vauthors = take(&p, end, nv * 32);
  const uint8_t* vsigs = take(&p, end, nv * 64);
  const uint8_t* vexp = take(&p, end, nv);
  if (p != end) {
    fprintf(stderr, "%ld trailing bytes\n", (long)(end - p));
    return 2;
  }

  int rc = coa_init(1);
  if (rc != COA_OK) {
    fprintf(stderr, "coa_init: %d (%s)\n", rc, coa_last_error());
    return 1;
  }
  /* n = 0 is COA_OK and touches no argument */
  if (coa_header_verify_many(NULL, NULL, NULL, NULL, NULL, 0, NULL) != COA_OK ||
      coa_vote_verify_many(NULL, NULL, NULL, NULL, NULL, 0, NULL) != COA_OK) {
    fprintf(stderr, "n = 0 is not COA_OK\n");
    return 1;
  }
  if (coa_message_workspace_bytes(nh > nv ? nh : nv) == 0) {
    fprintf(stderr, "workspace size is 0\n");
    return 1;
  }
  uint8_t* hgot = malloc(nh ? nh : 1);
  uint8_t* vgot = malloc(nv ? nv : 1);
  if (!hgot || !vgot) return 2;
  int bad = 0;
  for (int pass = 0; pass < 2; pass++) {
    /* pass 0: the committee's combs; pass 1: no committee, the uncached path */
    rc = coa_committee_register(keys, pass == 0 ? nk : 0);
    if (rc < 0) {
      fprintf(stderr, "coa_committee_register: %d (%s)\n", rc, coa_last_error());
      return 1;
    }
    memset(hgot, 0xee, nh);
    memset(vgot, 0xee, nv);
    rc = coa_header_verify_many(hdata, hoff, hids, hauthors, hsigs, nh, hgot);
    if (rc != COA_OK) {
      fprintf(stderr, "coa_header_verify_many: %d (%s)\n", rc, coa_last_error());
      return 1;
    }
    rc = coa_vote_verify_many(vids, vrounds, vorigins, vauthors, vsigs, nv, vgot);
    if (rc != COA_OK) {
      fprintf(stderr, "coa_vote_verify_many: %d (%s)\n", rc, coa_last_error());
      return 1;
    }
    bad += differ(pass ? "header status (no committee)" : "header status", hgot, hexp, nh);
    bad += differ(pass ? "vote verdict (no committee)" : "vote verdict", vgot, vexp, nv);
  }
  coa_shutdown();
  if (bad) {
    fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  printf("message harness ok (%zu headers, %zu votes)\n", nh, nv);
  free(hoff);
  free(vrounds);
  free(hgot);
  free(vgot);
  free(buf);
  return 0;
}
