// The engine's CPU path (csrc/coa_cpu.cpp) when many threads make their
// FIRST call at once -- what the Rust binding does when the GPU fails and
// every in-flight verification moves over (rust/crypto/src/degrade.rs).  The
// curve constants are built on first use; a thread that could see them partly
// built (B's table still zero) would accept every signature that decodes and
// is not of small order.  So T threads spin on one flag, are released
// together, and each makes one engine call on a valid input and one on that
// input with a message bit flipped (threads 2j and 2j+1 share entry j mod 6,
// the odd one forged first):
//   0 coa_cpu_ed25519_verify_strict        3 coa_cpu_certificate_verify_many
//   1 coa_cpu_ed25519_verify_strict_many   4 coa_cpu_header_verify_many
//   2 coa_cpu_ed25519_verify_batch_groups_z  5 coa_cpu_vote_verify_many
// A process has one first call, so tests/test_sanitizers.py runs this many
// times, under ThreadSanitizer, ASan + UBSan and plain -O2.
//
// usage: cpu_first_call <threads> <cpu_vectors.bin> <vote.bin>
//   cpu_vectors.bin  as for cpu_path_driver.cpp: the first valid vector with a
//                    32-byte message and the first valid group of >= 2
//   vote.bin         id(32) round(u64 LE) origin(32) author(32) sig(64): one
//                    valid vote (the vectors hold no signature over a
//                    Vote::digest and the CPU path has no signer)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "coa_verify.h"

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

struct Inputs {
  uint8_t msg[32], pk[32], sig[64];                              // a valid signature
  uint8_t gmsg[32];                                              // a valid batch group
  std::vector<uint8_t> gpks, gsigs, gzs;
  uint8_t vid[32], vorigin[32], vauthor[32], vsig[64];           // a valid vote
  uint64_t vround = 0;
};

static bool load(const char* vectors, const char* vote, Inputs& in) {
  FILE* f = fopen(vectors, "rb");
  if (!f) return false;
  char magic[4];
  uint32_t n = 0, groups = 0;
  if (!rd(f, magic, 4) || memcmp(magic, "CPUV", 4) != 0 || !rd(f, &n, 4)) return false;
  bool have = false;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t len = 0;
    uint8_t pk[32], sig[64], expect = 0;
    if (!rd(f, &len, 4)) return false;
    std::vector<uint8_t> m(len + 1);
    if ((len && !rd(f, m.data(), len)) || !rd(f, pk, 32) || !rd(f, sig, 64) || !rd(f, &expect, 1)) return false;
    if (!have && len == 32 && expect == 1) {
      memcpy(in.msg, m.data(), 32);
      memcpy(in.pk, pk, 32);
      memcpy(in.sig, sig, 64);
      have = true;
    }
  }
  if (!have || !rd(f, &groups, 4)) return false;
  have = false;
  for (uint32_t g = 0; g < groups; g++) {
    uint8_t msg[32], expect = 0;
    uint32_t k = 0;
    if (!rd(f, msg, 32) || !rd(f, &k, 4)) return false;
    std::vector<uint8_t> p(32 * k + 1), s(64 * k + 1), z(16 * k + 1);
    for (uint32_t j = 0; j < k; j++)
      if (!rd(f, &p[32 * j], 32) || !rd(f, &s[64 * j], 64) || !rd(f, &z[16 * j], 16)) return false;
    if (!rd(f, &expect, 1)) return false;
    if (!have && k >= 2 && expect == 1) {
      memcpy(in.gmsg, msg, 32);
      in.gpks = p, in.gsigs = s, in.gzs = z;
      have = true;
    }
  }
  fclose(f);
  if (!have) return false;
  f = fopen(vote, "rb");
  if (!f) return false;
  const bool ok = rd(f, in.vid, 32) && rd(f, &in.vround, 8) && rd(f, in.vorigin, 32) && rd(f, in.vauthor, 32) &&
                  rd(f, in.vsig, 64);
  fclose(f);
  return ok;
}

// Entry `kind` on the valid input, or on the forged one: how many of its
// answers accept (-1: the call itself failed) and how many it gives.
static int accepted(const Inputs& in, int kind, bool forged, int& answers) {
  uint8_t m[32];
  memcpy(m, kind == 2 ? in.gmsg : kind == 5 ? in.vid : in.msg, 32);
  if (forged) m[0] ^= 1;
  // the header the certificate and header entries hash: its digest is not the
  // id, which only sets COA_CERT_BAD_HEADER_ID; the signature bit is the answer
  const uint8_t hdata[1] = {0};
  const uint64_t hoff[2] = {0, 1}, voff[2] = {0, 0}, rounds[1] = {1};
  uint8_t st[2] = {0xff, 0xff};
  answers = 1;
  switch (kind) {
    case 0:
      return coa_cpu_ed25519_verify_strict(m, 32, in.pk, in.sig) == COA_OK;
    case 1: {
      uint8_t m2[64], pk2[64], sig2[128];
      for (int i = 0; i < 2; i++) {
        memcpy(m2 + 32 * i, m, 32);
        memcpy(pk2 + 32 * i, in.pk, 32);
        memcpy(sig2 + 64 * i, in.sig, 64);
      }
      answers = 2;
      if (coa_cpu_ed25519_verify_strict_many(m2, 32, pk2, sig2, 2, st, 2) != COA_OK) return -1;
      return (st[0] == 0) + (st[1] == 0);
    }
    case 2: {
      const uint64_t off[2] = {0, in.gpks.size() / 32};
      if (coa_cpu_ed25519_verify_batch_groups_z(m, in.gpks.data(), in.gsigs.data(), off, 1, in.gzs.data(), st, 1) !=
          COA_OK)
        return -1;
      return st[0] == 0;
    }
    case 3:
      if (coa_cpu_certificate_verify_many(hdata, hoff, m, in.pk, in.sig, rounds, nullptr, nullptr, voff, 1, 5, st, 1) !=
              COA_OK ||
          (st[0] & ~(COA_CERT_BAD_HEADER_ID | COA_CERT_BAD_HEADER_SIG)))
        return -1;
      return !(st[0] & COA_CERT_BAD_HEADER_SIG);
    case 4:
      if (coa_cpu_header_verify_many(hdata, hoff, m, in.pk, in.sig, 1, st, 1) != COA_OK ||
          (st[0] & ~(COA_CERT_BAD_HEADER_ID | COA_CERT_BAD_HEADER_SIG)))
        return -1;
      return !(st[0] & COA_CERT_BAD_HEADER_SIG);
    default:
      if (coa_cpu_vote_verify_many(m, &in.vround, in.vorigin, in.vauthor, in.vsig, 1, st, 1) != COA_OK) return -1;
      return st[0] == 0;
  }
}

int main(int argc, char** argv) {
  Inputs in;
  const int T = argc > 1 ? atoi(argv[1]) : 0;
  if (argc < 4 || T < 1 || T > 256 || !load(argv[2], argv[3], in)) {
    fprintf(stderr, "usage: %s <threads> <cpu_vectors.bin> <vote.bin>\n", argv[0]);
    return 2;
  }
  std::atomic<int> ready{0}, valid_rejected{0}, forged_accepted{0}, failed{0};
  std::atomic<bool> go{false};
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++)
    th.emplace_back([&, t] {
      ready.fetch_add(1);
      while (!go.load(std::memory_order_acquire)) {
      }
      for (int step = 0; step < 2; step++) {
        const bool forged = (step == 1) != (t % 2 == 1);
        int answers = 0;
        const int acc = accepted(in, (t / 2) % 6, forged, answers);
        if (acc < 0)
          failed.fetch_add(1);
        else if (forged)
          forged_accepted.fetch_add(acc);
        else
          valid_rejected.fetch_add(answers - acc);
      }
    });
  while (ready.load() < T) {
  }
  go.store(true, std::memory_order_release);
  for (auto& x : th) x.join();
  const int wrong = valid_rejected + forged_accepted + failed;
  if (wrong) {
    printf("first calls WRONG: %d threads, %d valid rejected, %d forged accepted, %d calls failed\n", T,
           valid_rejected.load(), forged_accepted.load(), failed.load());
    return 1;
  }
  printf("first calls ok: %d threads, 0 wrong\n", T);
  return 0;
}
