// The aggregation queue's counters (coa_queue.cpp; host code only, no HIP):
// the wait-time tally every answering thread keeps, and one lane's metrics --
// what a window and a resolver pass book into them and how they add up into
// coa_queue_metrics_t.  A metric is named here where it is declared, produced
// and read; a reset is the assignment of a fresh LaneMetrics.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "coa_queue.h"

namespace coa_q {

// Wait-time histogram: bucket 0 is < 1 us; bucket 8e + m + 1 covers
// [2^e (1 + m/8), 2^e (1 + (m+1)/8)) microseconds (the exponent and the top
// three mantissa bits of the double: no log per request).
constexpr int HB = 8 * 40;
inline int wait_bucket(double us) {
  if (!(us >= 1.0)) return 0;
  uint64_t bits;
  std::memcpy(&bits, &us, 8);
  const int e = (int)((bits >> 52) & 0x7ff) - 1023, m = (int)((bits >> 49) & 7);
  return std::min(HB - 1, 8 * e + m + 1);
}
inline double bucket_mid(int b) {
  if (b == 0) return 0.5;
  const int e = (b - 1) / 8, m = (b - 1) % 8;
  return std::ldexp(1.0 + (m + 0.5) / 8.0, e);
}
inline double hist_percentile(const uint64_t* hist, double q) {
  uint64_t total = 0;
  for (int b = 0; b < HB; b++) total += hist[b];
  if (total == 0) return 0.0;
  const double want = q * (double)total;
  uint64_t run = 0;
  for (int b = 0; b < HB; b++) {
    run += hist[b];
    if ((double)run >= want) return bucket_mid(b);
  }
  return bucket_mid(HB - 1);
}

// Submit -> callback wait times of the requests one thread answered: each
// run of callbacks and each resolver pass fills its own and merges it into
// the lane's under the lane's lock.
struct WaitTally {
  uint64_t hist[HB] = {};
  uint64_t n = 0;  // requests answered
  double sum = 0.0, max = 0.0;
  void add(double us) {
    n++;
    sum += us;
    max = std::max(max, us);
    hist[wait_bucket(us)]++;
  }
  void merge(const WaitTally& o) {
    for (int b = 0; b < HB; b++) hist[b] += o.hist[b];
    n += o.n;
    sum += o.sum;
    max = std::max(max, o.max);
  }
};

// One lane's metrics, kept under the lane's lock (the most items pending at
// once is an atomic beside it: producers raise it without the lock).
struct LaneMetrics {
  int64_t epoch_ns = 0;  // the lane's creation or its last reset
  WaitTally wait;        // every answered request, the resolver's included
  uint64_t windows = 0, max_window = 0, max_in_flight = 0;  // booked at the launch
  uint64_t sig = 0, batch = 0, cert = 0, dig = 0, hdr = 0, vote = 0;
  uint64_t msg_lat = 0, msg_tp = 0;  // message windows by the backend's route
  // verdict requests by kind (each also counted in cert / hdr / vote) and the
  // windows that held one (coa_queue_verdict_stats)
  uint64_t v_cert = 0, v_hdr = 0, v_vote = 0, v_windows = 0;
  uint64_t retried = 0, recovered = 0, failed = 0;
  // the slowest window (launch call -> outputs in host memory) and the
  // longest wait for a free slot
  double window_us_max = 0.0, window_max_at_ms = 0.0, window_max_dev_us = 0.0, slot_wait_us_max = 0.0;
  uint64_t window_max_items = 0;
  uint32_t window_max_kinds = 0;
  uint64_t deferred = 0, passes = 0;
  double resolve_us_max = 0.0;
  double stage_us[COA_QSTAGES] = {};

  // An answered window: launched at t_launch, its outputs in host memory
  // window_us later; `waits` are the requests answered with it (those left to
  // the resolver are booked by its pass).
  void record(const Launch& L, int64_t t_launch, double window_us, bool retried_window, const WaitTally& waits) {
    wait.merge(waits);
    for (int k = 0; k < COA_QSTAGES; k++) stage_us[k] += (double)L.stage_ns[k] * 1e-3;
    sig += L.nv + L.nhd + L.nvt;  // a message is one signature
    hdr += L.nhd;
    vote += L.nvt;
    if (L.msg_route == Launch::MSG_LATENCY) msg_lat++;
    if (L.msg_route == Launch::MSG_THROUGHPUT) msg_tp++;
    v_cert += L.n_vc;
    v_hdr += L.n_vh;
    v_vote += L.n_vvt;
    if (L.verdicts()) v_windows++;
    batch += L.ng;
    cert += L.nc;
    dig += L.nd;
    if (retried_window) {
      retried++;
      if (L.rc == COA_OK) recovered++;
    }
    if (window_us > window_us_max) {
      window_us_max = window_us;
      window_max_items = L.items();
      window_max_kinds = L.kinds();
      window_max_at_ms = (double)(t_launch - epoch_ns) * 1e-6;
      window_max_dev_us = (double)L.stage_ns[COA_QSTAGE_DEVICE_WAIT] * 1e-3;
    }
    slot_wait_us_max = std::max(slot_wait_us_max, (double)L.slot_wait_ns * 1e-3);
    if (L.rc != COA_OK) failed++;
  }

  // A resolver pass: the backend's decision took resolve_us, the callbacks of
  // the requests in `waits` callbacks_us.
  void record_pass(const WaitTally& waits, double resolve_us, double callbacks_us) {
    wait.merge(waits);
    deferred += waits.n;
    passes++;
    resolve_us_max = std::max(resolve_us_max, resolve_us);
    stage_us[COA_QSTAGE_RESOLVE] += resolve_us;
    stage_us[COA_QSTAGE_CALLBACKS] += callbacks_us;
  }

  // This lane's share of the queue's metrics: counts and stage times add up,
  // maxima are the larger lane's, the slowest window is described by the lane
  // that had it.  The wait times are merged into `waits`, from which the
  // caller takes the mean and the percentiles over all lanes.
  void add_to(coa_queue_metrics_t& out, WaitTally& waits) const {
    waits.merge(wait);
    out.requests += wait.n;
    out.windows += windows;
    out.signatures += sig;
    out.batches += batch;
    out.certificates += cert;
    out.digests += dig;
    out.max_window = std::max(out.max_window, max_window);
    out.max_in_flight = std::max(out.max_in_flight, max_in_flight);
    out.retried_windows += retried;
    out.recovered_windows += recovered;
    out.failed_windows += failed;
    if (window_us_max > out.window_us_max) {
      out.window_us_max = window_us_max;
      out.window_max_items = window_max_items;
      out.window_max_kinds = window_max_kinds;
      out.window_max_at_ms = window_max_at_ms;
      out.window_max_device_us = window_max_dev_us;
    }
    out.slot_wait_us_max = std::max(out.slot_wait_us_max, slot_wait_us_max);
    out.deferred_requests += deferred;
    out.resolver_passes += passes;
    out.resolve_us_max = std::max(out.resolve_us_max, resolve_us_max);
    for (int s = 0; s < COA_QSTAGES; s++) out.stage_us[s] += stage_us[s];
  }
};

}  // namespace coa_q
