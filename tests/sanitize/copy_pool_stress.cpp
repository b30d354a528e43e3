// Stress of csrc/coa_hostpool.h's CopyPool (the host copy threads that pack the
// aggregation queue's windows): 4 caller threads, each issuing 200 copies of
// 1-5 MB at once, so several jobs are in progress on the pool together; every
// copy is compared with its source.  The header is host-only (no HIP);
// tests/test_sanitizers.py builds this under TSan and under ASan + UBSan.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "coa_hostpool.h"

using namespace coa_rt;

int main() {
  std::vector<std::thread> th;
  std::atomic<int> bad{0};
  for (int t = 0; t < 4; t++)
    th.emplace_back([&, t] {
      for (int it = 0; it < 200; it++) {
        const size_t n = (size_t)(1 << 20) * (1 + (it + t) % 5) + 12345;
        std::vector<uint8_t> a(n), b(n, 0);
        for (size_t i = 0; i < n; i += 4093) a[i] = (uint8_t)(i * 7 + t + it);
        std::vector<Seg> segs;
        for (size_t o = 0; o < n; o += 300000) segs.push_back({b.data() + o, a.data() + o, std::min<size_t>(300000, n - o)});
        CopyPool::get().copy(segs);
        if (a != b) bad++;
      }
    });
  for (auto& x : th) x.join();
  printf("copy pool ok: %d bad\n", bad.load());
  return bad.load() != 0;
}
