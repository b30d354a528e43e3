// Host build of the two host-compilable headers of the committee kernels for
// tests/test_job_rules_host.py and tests/test_cert_scratch_host.py.
#include "coa_cert_scratch.h"
#include "coa_job_bits.h"

extern "C" {
uint32_t rule_latency(uint32_t pre, int r_ok, int eq) { return coa_rule_latency(pre, r_ok != 0, eq != 0); }
uint32_t rule_throughput(uint32_t pre, int eq) { return coa_rule_throughput(pre, eq != 0); }
uint32_t job_word(uint32_t status, uint32_t pre, uint32_t code) { return coa_job_word(status, pre, code); }
uint32_t job_status(uint32_t w) { return coa_job_status(w); }
uint32_t job_pre(uint32_t w) { return coa_job_pre(w); }
uint32_t job_code(uint32_t w) { return coa_job_code(w); }
// prefix bits in the order s, A, small A, torsion, strict, uncached, none, small P
void job_bits(uint32_t* out) {
  const uint32_t b[8] = {COA_JOB_S,      COA_JOB_A,        COA_JOB_SMALL_A, COA_JOB_TORSION,
                         COA_JOB_STRICT, COA_JOB_UNCACHED, COA_JOB_NONE,    COA_JOB_SMALL_P};
  for (int i = 0; i < 8; i++) out[i] = b[i];
}

// out: ctr, slab, cdig, total, counts, bin, perm (dword offsets), bytes, jcap, sorts
void cert_scratch(uint64_t jobs, uint64_t lanes, int digests, int key_order, uint64_t* out) {
  const CertScratch s(jobs, lanes, digests != 0, key_order != 0);
  const uint64_t v[10] = {s.ctr, s.slab, s.cdig, s.total, s.counts, s.bin, s.perm, s.bytes, s.jcap, s.sorts};
  for (int i = 0; i < 10; i++) out[i] = v[i];
}
}
