// The verdict calls of the engine's CPU path (csrc/coa_cpu.cpp:
// coa_cpu_*_verdict_many, csrc/coa_protocol.h) under ASan + UBSan: every case
// of the case file (tests/verdict_cases.py write_case_file describes it)
// through the certificate, header and vote forms on 1 and 4 threads, the
// protocol checks alone over supplied status bits, and the validation of the
// committee arrays that coa_committee_register_authorities shares.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "coa_verify.h"

namespace {

struct Reader {
  std::vector<uint8_t> buf;
  size_t at = 0;
  bool ok = true;
  template <class T>
  std::vector<T> take(size_t n) {
    std::vector<T> v(n + 1);  // never empty: data() stays a valid pointer
    if (at + n * sizeof(T) > buf.size()) {
      ok = false;
      return v;
    }
    if (n) std::memcpy(v.data(), buf.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
  }
  uint64_t u64() { return take<uint64_t>(1)[0]; }
  uint32_t u32() { return take<uint32_t>(1)[0]; }
};

int mismatches(const std::vector<uint32_t>& got, const std::vector<uint32_t>& want, size_t n, const char* what) {
  int bad = 0;
  for (size_t i = 0; i < n; i++)
    if (got[i] != want[i]) {
      if (!bad) fprintf(stderr, "%s %zu: got %#x want %#x\n", what, i, got[i], want[i]);
      bad++;
    }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  Reader r;
  uint8_t chunk[1 << 16];
  for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) r.buf.insert(r.buf.end(), chunk, chunk + k);
  fclose(f);
  if (r.take<uint8_t>(4)[0] != 'V') return 2;
  const uint32_t na = r.u32();
  auto cpk = r.take<uint8_t>(32 * (size_t)na);
  auto stakes = r.take<uint32_t>(na);
  auto woff = r.take<uint64_t>((size_t)na + 1);
  auto wids = r.take<uint32_t>(woff[na]);
  int bad = 0;

  // certificates
  const uint32_t nc = r.u32();
  const uint64_t hb = r.u64(), nv = r.u64();
  auto hoff = r.take<uint64_t>((size_t)nc + 1);
  auto hdata = r.take<uint8_t>(hb);
  auto ids = r.take<uint8_t>(32 * (size_t)nc);
  auto origins = r.take<uint8_t>(32 * (size_t)nc);
  auto hsigs = r.take<uint8_t>(64 * (size_t)nc);
  auto rounds = r.take<uint64_t>(nc);
  auto voff = r.take<uint64_t>((size_t)nc + 1);
  auto vpks = r.take<uint8_t>(32 * nv);
  auto vsigs = r.take<uint8_t>(64 * nv);
  auto pc = r.take<uint32_t>(nc);
  auto want = r.take<uint32_t>(nc);
  if (!r.ok) return 2;
  for (int threads : {1, 4}) {
    std::vector<uint32_t> got(nc + 1, 0xffffffffu);
    if (coa_cpu_certificate_verdict_many(hdata.data(), hoff.data(), ids.data(), origins.data(), hsigs.data(),
                                         rounds.data(), vpks.data(), vsigs.data(), voff.data(), nc, 5, pc.data(),
                                         cpk.data(), stakes.data(), wids.data(), woff.data(), na, got.data(),
                                         threads) != COA_OK)
      bad++;
    bad += mismatches(got, want, nc, "certificate");
  }
  // the protocol checks alone: with all-zero status bits no crypto error can
  // be answered, and a word that is not a crypto error must not change
  {
    std::vector<uint8_t> st(nc + 1, 0);
    std::vector<uint32_t> got(nc + 1, 0xffffffffu);
    if (coa_cpu_certificate_verdict_from_status(hdata.data(), hoff.data(), ids.data(), origins.data(), rounds.data(),
                                                vpks.data(), voff.data(), nc, pc.data(), st.data(), cpk.data(),
                                                stakes.data(), wids.data(), woff.data(), na, got.data(), 3) != COA_OK)
      bad++;
    for (uint32_t i = 0; i < nc; i++) {
      const uint32_t code = got[i] & 0xffu, w = want[i] & 0xffu;
      const bool crypto = w == COA_DAG_INVALID_HEADER_ID || w == COA_DAG_INVALID_SIGNATURE || w == COA_DAG_INVALID_VOTES;
      if (code == COA_DAG_INVALID_HEADER_ID || code == COA_DAG_INVALID_SIGNATURE || code == COA_DAG_INVALID_VOTES ||
          code == COA_DAG_VOTES_OPEN || (!crypto && got[i] != want[i]))
        bad++;
    }
  }
  // a payload count that overruns its header: COA_EINVAL for the call
  if (nc) {
    std::vector<uint32_t> over(pc), got(nc + 1);
    over[nc - 1] = (uint32_t)((hoff[nc] - hoff[nc - 1]) / 36 + 1);
    if (coa_cpu_certificate_verdict_many(hdata.data(), hoff.data(), ids.data(), origins.data(), hsigs.data(),
                                         rounds.data(), vpks.data(), vsigs.data(), voff.data(), nc, 5, over.data(),
                                         cpk.data(), stakes.data(), wids.data(), woff.data(), na, got.data(),
                                         2) != COA_EINVAL)
      bad++;
  }

  // headers
  const uint32_t nh = r.u32();
  const uint64_t hb2 = r.u64();
  auto hoff2 = r.take<uint64_t>((size_t)nh + 1);
  auto hdata2 = r.take<uint8_t>(hb2);
  auto hids = r.take<uint8_t>(32 * (size_t)nh);
  auto hauth = r.take<uint8_t>(32 * (size_t)nh);
  auto hsg = r.take<uint8_t>(64 * (size_t)nh);
  auto hpc = r.take<uint32_t>(nh);
  auto hwant = r.take<uint32_t>(nh);
  // votes
  const uint32_t nvt = r.u32();
  auto vids = r.take<uint8_t>(32 * (size_t)nvt);
  auto vrounds = r.take<uint64_t>(nvt);
  auto vorig = r.take<uint8_t>(32 * (size_t)nvt);
  auto vauth = r.take<uint8_t>(32 * (size_t)nvt);
  auto vsg = r.take<uint8_t>(64 * (size_t)nvt);
  auto vwant = r.take<uint32_t>(nvt);
  if (!r.ok || r.at != r.buf.size()) return 2;
  for (int threads : {1, 4}) {
    std::vector<uint32_t> got(nh + 1, 0xffffffffu);
    if (coa_cpu_header_verdict_many(hdata2.data(), hoff2.data(), hids.data(), hauth.data(), hsg.data(), nh, hpc.data(),
                                    cpk.data(), stakes.data(), wids.data(), woff.data(), na, got.data(),
                                    threads) != COA_OK)
      bad++;
    bad += mismatches(got, hwant, nh, "header");
    std::vector<uint32_t> gv(nvt + 1, 0xffffffffu);
    if (coa_cpu_vote_verdict_many(vids.data(), vrounds.data(), vorig.data(), vauth.data(), vsg.data(), nvt, cpk.data(),
                                  stakes.data(), wids.data(), woff.data(), na, gv.data(), threads) != COA_OK)
      bad++;
    bad += mismatches(gv, vwant, nvt, "vote");
  }

  // the committee arrays: what registration rejects, through the n = 0 calls
  auto committee_rc = [&](const std::vector<uint8_t>& k, const std::vector<uint32_t>& s,
                          const std::vector<uint32_t>& w, const std::vector<uint64_t>& o, size_t n) {
    return coa_cpu_vote_verdict_many(nullptr, nullptr, nullptr, nullptr, nullptr, 0, k.data(), s.data(), w.data(),
                                     o.data(), n, nullptr, 1);
  };
  if (committee_rc(cpk, stakes, wids, woff, na) != COA_OK) bad++;
  if (committee_rc(cpk, stakes, wids, woff, 0) != COA_OK) bad++;
  if (na >= 2) {
    auto dup = cpk;
    std::memcpy(&dup[32 * (size_t)(na - 1)], &dup[0], 32);
    if (committee_rc(dup, stakes, wids, woff, na) != COA_EINVAL) bad++;
    auto heavy = stakes;
    heavy[0] = 0x7fffffffu;
    heavy[1] = 1;
    if (committee_rc(cpk, heavy, wids, woff, na) != COA_EINVAL) bad++;
    auto back = woff;
    back[1] = back[2] + 1;
    if (committee_rc(cpk, stakes, wids, back, na) != COA_EINVAL) bad++;
  }
  {
    const size_t n = COA_MAX_AUTHORITIES + 1;
    std::vector<uint8_t> k(32 * n, 0);
    for (size_t i = 0; i < n; i++) {
      k[32 * i] = (uint8_t)i;
      k[32 * i + 1] = (uint8_t)(i >> 8);
    }
    std::vector<uint32_t> s(n, 1), w(n, 0);
    std::vector<uint64_t> o(n + 1);
    for (size_t i = 0; i <= n; i++) o[i] = i;
    if (committee_rc(k, s, w, o, n) != COA_EINVAL) bad++;
    if (committee_rc(k, s, w, o, n - 1) != COA_OK) bad++;
  }
  printf("verdict path ok: %u certificates, %u headers, %u votes, %d bad\n", nc, nh, nvt, bad);
  return bad != 0;
}
