/* A C caller of the aggregation queue's verdict requests
 * (coa_queue_submit_certificate_verdict[_borrowed], coa_queue_submit_header_verdict,
 * coa_queue_submit_vote_verdict, coa_queue_verdict_stats), compiled -std=c11
 * -Wall -Wextra -Werror: every new prototype is used.
 *
 *   queue_verdict_harness <case file> gpu   registers the file's committee,
 *       submits every case from 4 producer threads (certificates copied and
 *       borrowed in turn) and compares each callback's word with the file's
 *   queue_verdict_harness <case file> cpu   no device: every request is
 *       accepted and answered with COA_ENODEVICE and the failed word
 * In both modes a payload count that overruns its header is refused at
 * submission.  The case file is the one tests/verdict_cases.py
 * write_case_file describes. */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "coa_verify.h"

#define PRODUCERS 4

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

/* one request's answer, written by the callback (each slot by one callback) */
typedef struct {
  int status;
  size_t n;
  uint32_t word;
  int calls;
} answer_t;

static void on_word(void* user, int status, const uint8_t* verdicts, size_t n) {
  answer_t* a = user;
  a->status = status;
  a->n = n;
  a->word = 0xffffffffu;
  if (verdicts && n == 4) memcpy(&a->word, verdicts, 4);
  __atomic_add_fetch(&a->calls, 1, __ATOMIC_RELEASE);
}

static coa_queue* g_q;
static size_t g_nc, g_nh, g_nvt;
static uint64_t *g_hoff, *g_rounds, *g_voff, *g_hoff2, *g_vrounds;
static uint8_t *g_hdata, *g_ids, *g_origins, *g_hsigs, *g_vpks, *g_vsigs, *g_hdata2, *g_hids, *g_hauth, *g_hsg;
static uint8_t *g_vids, *g_vorig, *g_vauth, *g_vsg;
static uint32_t *g_pc, *g_hpc;
static answer_t* g_ans; /* certificates, then headers, then votes */
static int g_refused[PRODUCERS];

static void* producer(void* arg) {
  const size_t t = (size_t)(uintptr_t)arg;
  const size_t total = g_nc + g_nh + g_nvt;
  for (size_t k = t; k < total; k += PRODUCERS) {
    int rc;
    if (k < g_nc) {
      const size_t c = k, nv = (size_t)(g_voff[c + 1] - g_voff[c]);
      const uint8_t* hdr = g_hdata + g_hoff[c];
      const size_t hlen = (size_t)(g_hoff[c + 1] - g_hoff[c]);
      rc = (c & 1 ? coa_queue_submit_certificate_verdict_borrowed : coa_queue_submit_certificate_verdict)(
          g_q, hdr, hlen, g_ids + 32 * c, g_origins + 32 * c, g_hsigs + 64 * c, g_rounds[c], g_vpks + 32 * g_voff[c],
          g_vsigs + 64 * g_voff[c], nv, g_pc[c], on_word, &g_ans[k]);
    } else if (k < g_nc + g_nh) {
      const size_t i = k - g_nc;
      rc = coa_queue_submit_header_verdict(g_q, g_hdata2 + g_hoff2[i], (size_t)(g_hoff2[i + 1] - g_hoff2[i]),
                                           g_hids + 32 * i, g_hauth + 32 * i, g_hsg + 64 * i, g_hpc[i], on_word,
                                           &g_ans[k]);
    } else {
      const size_t i = k - g_nc - g_nh;
      rc = coa_queue_submit_vote_verdict(g_q, g_vids + 32 * i, g_vrounds[i], g_vorig + 32 * i, g_vauth + 32 * i,
                                         g_vsg + 64 * i, on_word, &g_ans[k]);
    }
    if (rc != COA_OK) g_refused[t]++;
  }
  return NULL;
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
  g_nc = take_u32();
  const size_t hb = (size_t)take_u64(), nv = (size_t)take_u64();
  g_hoff = take(8 * (g_nc + 1));
  g_hdata = take(hb);
  g_ids = take(32 * g_nc), g_origins = take(32 * g_nc), g_hsigs = take(64 * g_nc);
  g_rounds = take(8 * g_nc), g_voff = take(8 * (g_nc + 1));
  g_vpks = take(32 * nv), g_vsigs = take(64 * nv);
  g_pc = take(4 * g_nc);
  uint32_t* want = take(4 * g_nc);
  g_nh = take_u32();
  const size_t hb2 = (size_t)take_u64();
  g_hoff2 = take(8 * (g_nh + 1));
  g_hdata2 = take(hb2);
  g_hids = take(32 * g_nh), g_hauth = take(32 * g_nh), g_hsg = take(64 * g_nh);
  g_hpc = take(4 * g_nh);
  uint32_t* hwant = take(4 * g_nh);
  g_nvt = take_u32();
  g_vids = take(32 * g_nvt);
  g_vrounds = take(8 * g_nvt);
  g_vorig = take(32 * g_nvt), g_vauth = take(32 * g_nvt), g_vsg = take(64 * g_nvt);
  uint32_t* vwant = take(4 * g_nvt);
  if (g_at != g_len) return 2;
  const size_t total = g_nc + g_nh + g_nvt;
  g_ans = calloc(total + 1, sizeof(answer_t));
  if (!g_ans) return 2;
  int bad = 0;

  const int rc = coa_committee_register_authorities(cpk, stakes, wids, woff, na);
  if (gpu ? rc != (int)na : rc != COA_ENODEVICE) bad++;
  g_q = coa_queue_create(1u << 16, 2000);
  if (!g_q) return 2;

  /* refused at submission: a null argument, and a count that overruns its header */
  answer_t never = {0, 0, 0, 0};
  const size_t h0 = (size_t)(g_hoff2[1] - g_hoff2[0]);
  const uint32_t over = (uint32_t)(h0 < 40 ? 1 : (h0 - 40) / 36 + 1);
  if (coa_queue_submit_header_verdict(g_q, g_hdata2, h0, g_hids, g_hauth, g_hsg, over, on_word, &never) != COA_EINVAL ||
      coa_queue_submit_header_verdict(g_q, g_hdata2, h0, g_hids, g_hauth, NULL, 0, on_word, &never) != COA_EINVAL ||
      coa_queue_submit_vote_verdict(g_q, g_vids, 1, g_vorig, g_vauth, g_vsg, NULL, &never) != COA_EINVAL ||
      coa_queue_submit_vote_verdict(NULL, g_vids, 1, g_vorig, g_vauth, g_vsg, on_word, &never) != COA_EINVAL ||
      coa_queue_verdict_stats(NULL, NULL, NULL, NULL, NULL) != COA_EINVAL)
    bad++;
  const size_t c0 = (size_t)(g_hoff[1] - g_hoff[0]), v0 = (size_t)(g_voff[1] - g_voff[0]);
  const uint32_t cover = (uint32_t)(c0 < 40 ? 1 : (c0 - 40) / 36 + 1);
  if (coa_queue_submit_certificate_verdict(g_q, g_hdata, c0, g_ids, g_origins, g_hsigs, g_rounds[0], g_vpks, g_vsigs, v0,
                                           cover, on_word, &never) != COA_EINVAL ||
      coa_queue_submit_certificate_verdict_borrowed(g_q, g_hdata, c0, g_ids, g_origins, g_hsigs, g_rounds[0], g_vpks,
                                                    g_vsigs, v0, cover, on_word, &never) != COA_EINVAL)
    bad++;

  pthread_t th[PRODUCERS];
  for (size_t t = 0; t < PRODUCERS; t++)
    if (pthread_create(&th[t], NULL, producer, (void*)(uintptr_t)t) != 0) return 2;
  for (size_t t = 0; t < PRODUCERS; t++) {
    pthread_join(th[t], NULL);
    bad += g_refused[t];
  }
  if (coa_queue_flush(g_q) != COA_OK) bad++;
  if (never.calls) bad++;

  int shown = 0;
  for (size_t k = 0; k < total; k++) {
    const answer_t* a = &g_ans[k];
    const uint32_t w = k < g_nc ? want[k] : k < g_nc + g_nh ? hwant[k - g_nc] : vwant[k - g_nc - g_nh];
    const int ok = __atomic_load_n(&a->calls, __ATOMIC_ACQUIRE) == 1 && a->n == 4 &&
                   (gpu ? a->status == COA_OK && a->word == w && COA_DAG_CODE(a->word) != COA_DAG_VOTES_OPEN
                        : a->status == COA_ENODEVICE && a->word == COA_DAG_INVALID_SIGNATURE);
    if (!ok) {
      if (!shown++)
        fprintf(stderr, "request %zu: %d callbacks, status %d, n %zu, word %#x want %#x\n", k, a->calls, a->status, a->n,
                (unsigned)a->word, (unsigned)w);
      bad++;
    }
  }
  uint64_t vc = 0, vh = 0, vv = 0, vw = 0, launches = 0, items = 0, groups = 0;
  if (coa_queue_verdict_stats(g_q, &vc, &vh, &vv, &vw) != COA_OK || coa_queue_stats(g_q, &launches, &items, &groups) != COA_OK)
    bad++;
  if (vc != g_nc || vh != g_nh || vv != g_nvt || vw == 0 || vw > launches || items != g_nh + g_nvt || groups != g_nc) bad++;
  coa_queue_metrics_t m;
  if (coa_queue_metrics(g_q, &m) != COA_OK || m.requests != total) bad++;
  if (gpu && (m.failed_windows != 0 || m.retried_windows != 0)) bad++;
  if (coa_queue_destroy(g_q) != COA_OK) bad++;
  if (gpu && coa_committee_register(NULL, 0) != 0) bad++;
  printf("queue verdict harness (%s): %zu certificates, %zu headers, %zu votes, %llu verdict windows, %d bad\n",
         gpu ? "gpu" : "cpu", g_nc, g_nh, g_nvt, (unsigned long long)vw, bad);
  return bad != 0;
}
