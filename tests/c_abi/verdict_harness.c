/* A C caller of the verdict entry points of include/coa_verify.h
 * (coa_committee_register_authorities, coa_*_verdict_many, their
 * device-resident and CPU forms), compiled -std=c11 -Wall -Wextra -Werror:
 * every new prototype is used.
 *
 *   verdict_harness <case file> cpu   the CPU forms against the file's
 *                                     expected words; every GPU form must
 *                                     refuse with COA_ENODEVICE
 *   verdict_harness <case file> gpu   registers the file's committee and
 *                                     checks the host-pointer GPU forms too
 * The case file is the one tests/verdict_cases.py write_case_file describes. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "coa_verify.h"

static uint8_t* g_buf;
static size_t g_len, g_at;

/* the next `bytes` of the file in a buffer of their own (aligned for any type) */
static void* take(size_t bytes) {
  void* p = malloc(bytes + 8);
  if (!p || g_at + bytes > g_len) {
    fprintf(stderr, "case file truncated\n");
    exit(2);
  }
  memcpy(p, g_buf + g_at, bytes);
  g_at += bytes;
  return p;
}
static uint32_t take_u32(void) {
  uint32_t v;
  memcpy(&v, g_buf + g_at, 4);
  g_at += 4;
  return v;
}
static uint64_t take_u64(void) {
  uint64_t v;
  memcpy(&v, g_buf + g_at, 8);
  g_at += 8;
  return v;
}

static int differ(const uint32_t* got, const uint32_t* want, size_t n, const char* what) {
  int bad = 0;
  for (size_t i = 0; i < n; i++)
    if (got[i] != want[i]) {
      if (!bad) fprintf(stderr, "%s %zu: got %#x want %#x\n", what, i, (unsigned)got[i], (unsigned)want[i]);
      bad++;
    }
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int gpu = strcmp(argv[2], "gpu") == 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  g_len = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  g_buf = malloc(g_len + 1);
  if (!g_buf || fread(g_buf, 1, g_len, f) != g_len) return 2;
  fclose(f);
  if (g_len < 8 || memcmp(g_buf, "VRDC", 4) != 0) return 2;
  g_at = 4;
  const size_t na = take_u32();
  uint8_t* cpk = take(32 * na);
  uint32_t* stakes = take(4 * na);
  uint64_t* woff = take(8 * (na + 1));
  uint32_t* wids = take(4 * (size_t)woff[na]);
  const size_t nc = take_u32();
  const size_t hb = (size_t)take_u64(), nv = (size_t)take_u64();
  uint64_t* hoff = take(8 * (nc + 1));
  uint8_t* hdata = take(hb);
  uint8_t *ids = take(32 * nc), *origins = take(32 * nc), *hsigs = take(64 * nc);
  uint64_t *rounds = take(8 * nc), *voff = take(8 * (nc + 1));
  uint8_t *vpks = take(32 * nv), *vsigs = take(64 * nv);
  uint32_t *pc = take(4 * nc), *want = take(4 * nc);
  const size_t nh = take_u32();
  const size_t hb2 = (size_t)take_u64();
  uint64_t* hoff2 = take(8 * (nh + 1));
  uint8_t* hdata2 = take(hb2);
  uint8_t *hids = take(32 * nh), *hauth = take(32 * nh), *hsg = take(64 * nh);
  uint32_t *hpc = take(4 * nh), *hwant = take(4 * nh);
  const size_t nvt = take_u32();
  uint8_t* vids = take(32 * nvt);
  uint64_t* vrounds = take(8 * nvt);
  uint8_t *vorig = take(32 * nvt), *vauth = take(32 * nvt), *vsg = take(64 * nvt);
  uint32_t* vwant = take(4 * nvt);
  if (g_at != g_len) return 2;
  size_t nmax = nc > nh ? nc : nh;
  if (nvt > nmax) nmax = nvt;
  uint32_t* got = malloc(4 * (nmax + 1));
  uint8_t* st = calloc(nc + 1, 1);
  if (!got || !st) return 2;
  int bad = 0;

  /* the CPU forms */
  if (coa_cpu_certificate_verdict_many(hdata, hoff, ids, origins, hsigs, rounds, vpks, vsigs, voff, nc, 9, pc, cpk,
                                       stakes, wids, woff, na, got, 4) != COA_OK)
    bad++;
  bad += differ(got, want, nc, "cpu certificate");
  if (coa_cpu_certificate_verify_many(hdata, hoff, ids, origins, hsigs, rounds, vpks, vsigs, voff, nc, 9, st, 4) != COA_OK ||
      coa_cpu_certificate_verdict_from_status(hdata, hoff, ids, origins, rounds, vpks, voff, nc, pc, st, cpk, stakes,
                                              wids, woff, na, got, 1) != COA_OK)
    bad++;
  bad += differ(got, want, nc, "cpu certificate from status");
  if (coa_cpu_header_verdict_many(hdata2, hoff2, hids, hauth, hsg, nh, hpc, cpk, stakes, wids, woff, na, got, 2) != COA_OK)
    bad++;
  bad += differ(got, hwant, nh, "cpu header");
  if (coa_cpu_vote_verdict_many(vids, vrounds, vorig, vauth, vsg, nvt, cpk, stakes, wids, woff, na, got, 2) != COA_OK)
    bad++;
  bad += differ(got, vwant, nvt, "cpu vote");
  if (COA_DAG_CODE(0x4305u) != COA_DAG_AUTHORITY_REUSE || COA_DAG_VOTE_INDEX(0x4305u) != 0x43u) bad++;
  /* the workspace sizes are plain arithmetic: the crypto call's plus two words per item */
  if (coa_certificate_verdict_workspace_bytes(nc, nv) < coa_certificate_workspace_bytes(nc, nv) + 8 * nc ||
      coa_message_verdict_workspace_bytes(nh) < coa_message_workspace_bytes(nh) + 8 * nh)
    bad++;

  /* the GPU forms */
  const int want_rc = gpu ? COA_OK : COA_ENODEVICE;
  int rc = coa_committee_register_authorities(cpk, stakes, wids, woff, na);
  if (gpu ? rc != (int)na : rc != COA_ENODEVICE) bad++;
  if (coa_certificate_verdict_many(hdata, hoff, ids, origins, hsigs, rounds, vpks, vsigs, voff, nc, 9, pc, got) != want_rc)
    bad++;
  if (gpu) bad += differ(got, want, nc, "gpu certificate");
  if (coa_header_verdict_many(hdata2, hoff2, hids, hauth, hsg, nh, hpc, got) != want_rc) bad++;
  if (gpu) bad += differ(got, hwant, nh, "gpu header");
  if (coa_vote_verdict_many(vids, vrounds, vorig, vauth, vsg, nvt, got) != want_rc) bad++;
  if (gpu) bad += differ(got, vwant, nvt, "gpu vote");
  if (gpu) {
    /* n = 0 is COA_OK whatever the pointers; a null argument is COA_EINVAL */
    if (coa_certificate_verdict_many_device(0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL,
                                            NULL, NULL) != COA_OK ||
        coa_header_verdict_many_device(0, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL) != COA_OK ||
        coa_vote_verdict_many_device(0, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL) != COA_OK)
      bad++;
    if (coa_certificate_verdict_many_device(0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1, 0, NULL, NULL,
                                            NULL, NULL) != COA_EINVAL ||
        coa_header_verdict_many_device(0, NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL, NULL, NULL) != COA_EINVAL ||
        coa_vote_verdict_many_device(0, NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL, NULL) != COA_EINVAL ||
        coa_vote_verdict_many(NULL, vrounds, vorig, vauth, vsg, 1, got) != COA_EINVAL)
      bad++;
    /* plain registration leaves no protocol table */
    if (coa_committee_register(cpk, na) != (int)na ||
        coa_vote_verdict_many(vids, vrounds, vorig, vauth, vsg, nvt, got) != COA_EINVAL ||
        strstr(coa_last_error(), "without stakes") == NULL)
      bad++;
    if (coa_committee_register(NULL, 0) != 0) bad++;
  } else {
    /* host memory stands in for device pointers: the calls must refuse before touching it */
    if (coa_certificate_verdict_many_device(0, hdata, hoff, ids, origins, hsigs, rounds, vpks, vsigs, voff, nc, nv, pc,
                                            got, NULL, NULL) != COA_ENODEVICE ||
        coa_header_verdict_many_device(0, hdata2, hoff2, hids, hauth, hsg, nh, hpc, got, NULL, NULL) != COA_ENODEVICE ||
        coa_vote_verdict_many_device(0, vids, vrounds, vorig, vauth, vsg, nvt, got, NULL, NULL) != COA_ENODEVICE)
      bad++;
  }
  /* n = 0 never needs a device */
  if (coa_certificate_verdict_many(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL) != COA_OK ||
      coa_header_verdict_many(NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL) != COA_OK ||
      coa_vote_verdict_many(NULL, NULL, NULL, NULL, NULL, 0, NULL) != COA_OK)
    bad++;
  printf("verdict harness (%s): %zu certificates, %zu headers, %zu votes, %d bad\n", gpu ? "gpu" : "cpu", nc, nh, nvt,
         bad);
  return bad != 0;
}
