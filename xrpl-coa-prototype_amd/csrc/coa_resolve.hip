// Open certificates decided on the device (coa_certificate_votes_resolve_device):
// the certificates a device-resident verdict call left at COA_DAG_VOTES_OPEN
// get dalek 1.0.1 verify_batch's answer over (Certificate::digest, votes) --
// the exact random-linear-combination check of coa_batch.hip -- without the
// host seeing a word: which certificates are open, how many votes they hold
// and where each vote's term goes are decided by the first kernel and read
// from its count words by the others.  Grids are sized by the host's upper
// bounds (the vote cap, the certificate count).
//
// Kernels, in stream order:
//   k_open_scan        one block: the ascending list of open certificates,
//                      the exclusive prefix of their vote counts (cut at the
//                      cap) and the count words
//   k_resolve_prepare  one lane per open vote: its certificate from the
//                      prefix, Certificate::digest (hashed by one lane per
//                      certificate and block), k = H(R || A || digest) mod l,
//                      the weight z (given, or k_batch_z's block)
//   k_resolve_terms    one lane per open vote: coa_batch::term, the body of
//                      k_batch_terms, with the vote's bytes at its position in
//                      the call and its slot at its position among the open votes
//   k_resolve_sum      one workgroup per open certificate: coa_batch::group_ok,
//                      the body of k_batch_reduce, and the verdict word
#include "coa_batch_dev.h"  // first: it keeps coa_fe.h's uniform comba columns

#include "coa_keycache.h"
#include "coa_resolve.h"
#include "coa_resolve_ws.h"
#include "coa_verify.h"

#define SCAN_BLOCK 1024
#define PREP_BLOCK 256

static_assert(COA_RESOLVE_SCRATCH_PER_LANE == COA_BATCH_SCRATCH_PER_LANE, "the term's scratch");

namespace {

// Votes of certificate i, or more than the cap holds when its offsets are
// not ordered inside the call's vote arrays (it then never fits, and no kernel
// reads a vote outside them).
COA_DEV uint64_t votes_of(const uint64_t* __restrict__ voff, uint32_t i, uint32_t n_votes, uint32_t cap) {
  const uint64_t lo = voff[i], hi = voff[i + 1];
  return (lo <= hi && hi <= n_votes) ? hi - lo : (uint64_t)cap + 1;
}

// open certificate owning open vote j: the last oc with pre[oc] <= j
// (pre[0] = 0 <= j < pre[nres]; a certificate without votes owns none)
COA_DEV uint32_t open_of(const uint32_t* __restrict__ pre, uint32_t nres, uint32_t j) {
  uint32_t lo = 0, hi = nres;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pre[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace

// One block.  Thread t owns certificates [t * per, (t + 1) * per): it counts
// its open ones and their votes, the block scans both sums (k_job_scan's
// scan), and the thread walks its range again with its exclusive starts.  An
// open certificate is taken while the votes of every open certificate up to
// and including it fit the cap, so the taken ones are a prefix of the open
// ones in index order and a certificate's rank among the open ones is its
// slot.  counts: [0] open found, [1] taken, [2] their votes, [3] 0.
__global__ void __launch_bounds__(SCAN_BLOCK) k_open_scan(const uint32_t* __restrict__ verdicts,
                                                          const uint64_t* __restrict__ voff, uint32_t n,
                                                          uint32_t n_votes, uint32_t cap, uint32_t* __restrict__ idx,
                                                          uint32_t* __restrict__ pre, uint32_t* __restrict__ counts,
                                                          uint32_t* __restrict__ counts_out) {
  __shared__ uint32_t pc[SCAN_BLOCK];
  __shared__ uint64_t pv[SCAN_BLOCK];
  __shared__ uint32_t taken, taken_votes;
  const uint32_t t = threadIdx.x, per = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
  if (t == 0) {
    taken = 0;
    taken_votes = 0;
  }
  uint32_t oc = 0;
  uint64_t ov = 0;
  for (uint32_t i = lo; i < hi; i++)
    if (COA_DAG_CODE(verdicts[i]) == COA_DAG_VOTES_OPEN) {
      oc++;
      ov += votes_of(voff, i, n_votes, cap);
    }
  pc[t] = oc;
  pv[t] = ov;
  __syncthreads();
  for (uint32_t o = 1; o < SCAN_BLOCK; o <<= 1) {  // inclusive scan of the per-thread sums
    const uint32_t xc = t >= o ? pc[t - o] : 0u;
    const uint64_t xv = t >= o ? pv[t - o] : 0ull;
    __syncthreads();
    pc[t] += xc;
    pv[t] += xv;
    __syncthreads();
  }
  uint32_t ci = pc[t] - oc, mine = 0, end = 0;  // exclusive starts of this thread's range
  uint64_t vi = pv[t] - ov;
  for (uint32_t i = lo; i < hi; i++)
    if (COA_DAG_CODE(verdicts[i]) == COA_DAG_VOTES_OPEN) {
      const uint64_t nv = votes_of(voff, i, n_votes, cap);
      if (vi + nv <= cap) {
        idx[ci] = i;
        pre[ci] = (uint32_t)vi;
        mine++;
        end = (uint32_t)(vi + nv);
      }
      ci++;
      vi += nv;
    }
  if (mine) {
    atomicAdd(&taken, mine);
    atomicMax(&taken_votes, end);
  }
  __syncthreads();
  if (t == 0) {
    pre[taken] = taken_votes;
    const uint32_t c[COA_RESOLVE_COUNT_WORDS] = {pc[SCAN_BLOCK - 1], taken, taken_votes, 0u};
#pragma unroll
    for (int j = 0; j < COA_RESOLVE_COUNT_WORDS; j++) counts[j] = c[j];
    if (counts_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) counts_out[j] = c[j];
    }
  }
}

// Open votes in chunks of PREP_BLOCK, one per block and pass.  A certificate's
// first vote inside the chunk hashes Certificate::digest into the block's LDS
// slot of its own lane; the certificate's other votes in the chunk read it
// there (a certificate that crosses a chunk boundary is hashed once per chunk).
__global__ void __launch_bounds__(PREP_BLOCK) k_resolve_prepare(ResolveArgs a, const uint32_t* __restrict__ idx,
                                                                const uint32_t* __restrict__ pre,
                                                                const uint32_t* __restrict__ counts,
                                                                uint32_t* __restrict__ kbuf,
                                                                uint32_t* __restrict__ zbuf) {
  using namespace coa_kc;
  __shared__ uint32_t dig[PREP_BLOCK * 8];
  const uint32_t nres = counts[1], nvotes = counts[2];
  for (uint32_t base = blockIdx.x * PREP_BLOCK; base < nvotes; base += gridDim.x * PREP_BLOCK) {
    const uint32_t j = base + threadIdx.x;
    const bool live = j < nvotes;
    uint32_t cert = 0, src = 0, lead = 0;
    if (live) {
      const uint32_t oc = open_of(pre, nres, j), p = pre[oc];
      cert = idx[oc];
      src = (uint32_t)a.voff[cert] + (j - p);
      lead = p > base ? p - base : 0;  // the lane of the certificate's first vote in this chunk
      if (threadIdx.x == lead) {
        uint32_t h[8], origin[8];
        load8(h, a.ids + (uint64_t)cert * 8);
        load8(origin, a.origins + (uint64_t)cert * 8);
        round_origin_digest(h, a.rounds[cert], origin);
#pragma unroll
        for (int q = 0; q < 8; q++) dig[lead * 8 + q] = h[q];
      }
    }
    __syncthreads();
    if (live) {
      uint32_t msg[8], aw[8], rw[8], sw[8];
#pragma unroll
      for (int q = 0; q < 8; q++) msg[q] = dig[lead * 8 + q];
      const uint32_t* sg = reinterpret_cast<const uint32_t*>(a.vsigs + (uint64_t)src * 64);
      load8(aw, reinterpret_cast<const uint32_t*>(a.vpks + (uint64_t)src * 32));
      load8(rw, sg);
      load8(sw, sg + 8);
      sc k;
      challenge(k, rw, aw, msg);
      uint4* ko = reinterpret_cast<uint4*>(kbuf + (uint64_t)j * 8);
      ko[0] = make_uint4(k.v[0], k.v[1], k.v[2], k.v[3]);
      ko[1] = make_uint4(k.v[4], k.v[5], k.v[6], k.v[7]);
      uint32_t z[4];
      if (a.zs) {
#pragma unroll
        for (int q = 0; q < 4; q++) z[q] = a.zs[(uint64_t)src * 4 + q];
      } else {
        // the group is the certificate's index and i the vote's position in
        // the call: the weight does not depend on what else is open
        coa_batch::z_derive(z, a.seed, cert, src, k.v, sw);
      }
      *reinterpret_cast<uint4*>(zbuf + (uint64_t)j * 4) = make_uint4(z[0], z[1], z[2], z[3]);
    }
    __syncthreads();  // the next pass overwrites dig
  }
}

__global__ void __launch_bounds__(BATCH_BLOCK, 2) k_resolve_terms(ResolveArgs a, const uint32_t* __restrict__ idx,
                                                               const uint32_t* __restrict__ pre,
                                                               const uint32_t* __restrict__ counts,
                                                               const uint32_t* __restrict__ kbuf,
                                                               const uint32_t* __restrict__ zbuf,
                                                               uint32_t* __restrict__ terms,
                                                               uint8_t* __restrict__ flags, uint32_t* __restrict__ scr,
                                                               const uint32_t* __restrict__ btab_g) {
  __shared__ __attribute__((aligned(16))) uint32_t btab[COA_BTAB_DWORDS];
  coa_batch::btab_load(btab, btab_g);
  const uint32_t nres = counts[1], nvotes = counts[2];
  const uint32_t lanes = gridDim.x * blockDim.x;
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t j = lane; j < nvotes; j += lanes) {
    const uint32_t oc = open_of(pre, nres, j);
    const uint32_t src = (uint32_t)a.voff[idx[oc]] + (j - pre[oc]);
    coa_batch::term(a.vpks, a.vsigs, src, kbuf, zbuf, j, terms, flags, scr, lanes, lane, btab);
  }
}

// Workgroup g: open certificate idx[g], terms [pre[g], pre[g + 1]).
__global__ void __launch_bounds__(BATCH_BLOCK) k_resolve_sum(const uint32_t* __restrict__ idx,
                                                             const uint32_t* __restrict__ pre,
                                                             const uint32_t* __restrict__ counts,
                                                             const uint32_t* __restrict__ terms,
                                                             const uint8_t* __restrict__ flags,
                                                             uint32_t* __restrict__ verdicts) {
  __shared__ __attribute__((aligned(16))) uint32_t pts[BATCH_BLOCK * 32];
  __shared__ int bad;
  const uint32_t g = blockIdx.x;
  if (g >= counts[1]) return;  // past the open certificates taken
  const bool ok = coa_batch::group_ok(pre[g], pre[g + 1], terms, flags, pts, &bad);
  if (threadIdx.x == 0) verdicts[idx[g]] = ok ? COA_DAG_OK : COA_DAG_INVALID_VOTES;
}

hipError_t coa_launch_votes_resolve(const ResolveArgs& a, uint8_t* ws, const uint32_t* btab, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const ResolveWs L(a.n, a.n_votes, a.cap);
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws + L.counts);
  uint32_t* idx = reinterpret_cast<uint32_t*>(ws + L.idx);
  uint32_t* pre = reinterpret_cast<uint32_t*>(ws + L.pre);
  uint32_t* kbuf = reinterpret_cast<uint32_t*>(ws + L.k);
  uint32_t* zbuf = reinterpret_cast<uint32_t*>(ws + L.z);
  uint32_t* terms = reinterpret_cast<uint32_t*>(ws + L.terms);
  uint8_t* flags = ws + L.flags;
  uint32_t* scr = reinterpret_cast<uint32_t*>(ws + L.scr);
  hipLaunchKernelGGL(k_open_scan, dim3(1), dim3(SCAN_BLOCK), 0, s, a.verdicts, a.voff, a.n, a.n_votes, L.cap, idx, pre,
                     counts, a.counts_out);
  if (L.cap) {  // a call without votes has only empty certificates to close
    const uint32_t chunks = (L.cap + PREP_BLOCK - 1) / PREP_BLOCK;
    hipLaunchKernelGGL(k_resolve_prepare, dim3(chunks < 4096 ? chunks : 4096), dim3(PREP_BLOCK), 0, s, a, idx, pre,
                       counts, kbuf, zbuf);
    hipLaunchKernelGGL(k_resolve_terms, dim3(L.lanes / BATCH_BLOCK), dim3(BATCH_BLOCK), 0, s, a, idx, pre, counts, kbuf,
                       zbuf, terms, flags, scr, btab);
  }
  hipLaunchKernelGGL(k_resolve_sum, dim3(a.n), dim3(BATCH_BLOCK), 0, s, idx, pre, counts, terms, flags, a.verdicts);
  return hipGetLastError();
}
