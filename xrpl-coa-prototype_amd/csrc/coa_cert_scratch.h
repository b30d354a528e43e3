// The device scratch of the throughput kernels (k_cert_verify, k_msg_verify)
// as one layout: what coa_cert_scratch_bytes / coa_msg_scratch_bytes size and
// what the launchers carve (coa_committee.hip).  Host code only (no HIP), so
// tests/test_cert_scratch_host.py builds it with plain g++.
#pragma once
#include <cstddef>
#include <cstdint>

// key-order sort (k_job_count, k_job_scan, k_job_place)
#define COA_SORT_BINS 4096
#define COA_SORT_WGS 256
// smallest call the key-order sort pays for (its three launches)
#define COA_SORT_MIN_JOBS 16384
// uint4 rows of one job slot in the slab (pscr_put, coa_committee.hip)
#define PSCR_ROWS 9

// chunk counter | slab (lanes x jcap job slots) | Certificate::digest per
// certificate (`digests`: the certificate kernel; at most one per job) |
// key-order sort, only for a call that may sort (key_order and at least
// COA_SORT_MIN_JOBS jobs): bin totals / cursors [COA_SORT_BINS], counts
// [COA_SORT_WGS][COA_SORT_BINS], each job's bin [jobs], the permutation [jobs]
// (~4.2 MB + 8 B per job; a latency or pipelined-chunk workspace does not
// carry it).  Offsets in dwords from the scratch pointer; a section that is
// not there has offset 0.  Every section starts on 16 bytes but the
// permutation, which follows the jobs' bins without a gap (dword reads).
struct CertScratch {
  uint32_t jcap;  // signature chunks one wave may take (its slab capacity)
  bool sorts;     // the sort sections are there
  static constexpr size_t ctr = 0, slab = 64;  // [0, 256) holds the chunk counter
  size_t cdig = 0, total = 0, counts = 0, bin = 0, perm = 0;
  size_t bytes;

  CertScratch(uint64_t jobs, uint64_t lanes, bool digests, bool key_order) {
    // the even share of the chunks plus slack for the waves that run ahead
    const uint64_t waves = lanes / 64, chunks = (jobs + 63) / 64;
    jcap = (uint32_t)((chunks + waves - 1) / waves + 2);
    sorts = digests && key_order && jobs >= COA_SORT_MIN_JOBS;
    size_t end = slab + (size_t)(lanes * jcap * PSCR_ROWS * 4);
    if (digests) {
      cdig = end;
      end += (size_t)(jobs ? jobs : 1) * 8;
    }
    if (sorts) {
      total = end + 64;
      counts = total + COA_SORT_BINS;
      bin = counts + (size_t)COA_SORT_BINS * COA_SORT_WGS;
      perm = bin + (size_t)jobs;
      end = perm + (size_t)jobs;
    }
    bytes = end * 4;
  }
};
