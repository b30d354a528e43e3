// The host-only pieces of the runtime, run stand-alone under sanitizers
// (tests/test_runtime_host_sanitize.py; no HIP, nothing preloaded):
//  * csrc/coa_env.h: every switch reader on an unset, empty, "0", clamp-edge,
//    beyond-the-clamp and non-numeric value, against a table written out from
//    the expressions the sites used before the readers existed (atoi / atol /
//    atof / strtoull, string compare, "first char not '0'", and their clamps);
//  * csrc/coa_offsets.h: the monotone check, the rebased offsets, the 72-byte
//    digest input against a literal;
//  * csrc/coa_hostpool.h: Worker, tasks submitted from two threads.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "coa_env.h"
#include "coa_hostpool.h"
#include "coa_offsets.h"

using namespace coa_rt;

static int bad = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      bad++;                                                     \
      printf("FAIL line %d: %s [%s]\n", __LINE__, #cond, what); \
    }                                                            \
  } while (0)

static const char* const UNSET = nullptr;
static const char* what = "";
static void set(const char* name, const char* value) {
  static std::string label;
  label = std::string(name) + "=" + (value ? value : "<unset>");
  what = label.c_str();
  if (value) setenv(name, value, 1);
  else unsetenv(name);
}

// the sites' own expressions around a reader, as they stand in the engine
static long cert_chunk_jobs() {
  const long v = env_int("COA_CERT_CHUNK_JOBS", 0);
  return v >= (1 << 12) ? v : (1l << 17);
}
static long queue_slots(long dflt) {
  const long v = env_int("COA_QUEUE_SLOTS", 0);
  return v >= 1 && v <= 8 ? v : dflt;
}

struct IntCase {
  const char* value;
  long want;
};

static void check_env() {
  // integer clamped to a range: COA_CERT_BUFFERS (atoi, 2..4, default 3)
  for (IntCase c : {IntCase{UNSET, 3}, {"", 2}, {"0", 2}, {"1", 2}, {"2", 2}, {"3", 3}, {"4", 4}, {"5", 4}, {"9", 4},
                    {"-1", 2}, {"many", 2}}) {
    set("COA_CERT_BUFFERS", c.value);
    EXPECT(env_int("COA_CERT_BUFFERS", 3, 2, 4) == c.want);
  }
  // COA_CERT_RAMP (atoi, 0..4, default 1)
  for (IntCase c : {IntCase{UNSET, 1}, {"", 0}, {"0", 0}, {"-1", 0}, {"1", 1}, {"4", 4}, {"5", 4}, {"7", 4}, {"x", 0}}) {
    set("COA_CERT_RAMP", c.value);
    EXPECT(env_int("COA_CERT_RAMP", 1, 0, 4) == c.want);
  }
  // COA_PACK_THREADS (atoi, 1..16, default 8)
  for (IntCase c : {IntCase{UNSET, 8}, {"", 1}, {"0", 1}, {"1", 1}, {"16", 16}, {"17", 16}, {"abc", 1}}) {
    set("COA_PACK_THREADS", c.value);
    EXPECT(env_int("COA_PACK_THREADS", 8, 1, 16) == c.want);
  }
  // the queue's: COA_QUEUE_HELPERS (0..15, unset: the lane's default as it is),
  // COA_QUEUE_COLLECTORS (1..4, default 2), COA_QUEUE_IDLE_LAUNCH (0..64),
  // COA_QUEUE_DIGEST_MAX (at least 1, default 96)
  for (IntCase c : {IntCase{UNSET, 3}, {"", 0}, {"0", 0}, {"-3", 0}, {"15", 15}, {"16", 15}, {"99", 15}, {"h", 0}}) {
    set("COA_QUEUE_HELPERS", c.value);
    EXPECT(env_int("COA_QUEUE_HELPERS", 3, 0, 15) == c.want);
  }
  for (IntCase c : {IntCase{UNSET, 2}, {"", 1}, {"0", 1}, {"1", 1}, {"4", 4}, {"5", 4}, {"two", 1}}) {
    set("COA_QUEUE_COLLECTORS", c.value);
    EXPECT(env_int("COA_QUEUE_COLLECTORS", 2, 1, 4) == c.want);
  }
  for (IntCase c : {IntCase{UNSET, 0}, {"", 0}, {"0", 0}, {"-1", 0}, {"64", 64}, {"65", 64}, {"z", 0}}) {
    set("COA_QUEUE_IDLE_LAUNCH", c.value);
    EXPECT(env_int("COA_QUEUE_IDLE_LAUNCH", 0, 0, 64) == c.want);
  }
  for (IntCase c : {IntCase{UNSET, 96}, {"", 1}, {"0", 1}, {"-7", 1}, {"1", 1}, {"500", 500}, {"q", 1}}) {
    set("COA_QUEUE_DIGEST_MAX", c.value);
    EXPECT(env_int("COA_QUEUE_DIGEST_MAX", 96, 1, 0x7fffffff) == c.want);
  }
  // plain integer: COA_REGISTER_CUS (atoi, default 0; the site tests <= 0)
  for (IntCase c : {IntCase{UNSET, 0}, {"", 0}, {"0", 0}, {"128", 128}, {"-5", -5}, {"cus", 0}}) {
    set("COA_REGISTER_CUS", c.value);
    EXPECT(env_int("COA_REGISTER_CUS", 0) == c.want);
  }
  // COA_CERT_CHUNK_JOBS (atol; below 2^12, or no number: the default 2^17)
  for (IntCase c : {IntCase{UNSET, 1 << 17}, {"", 1 << 17}, {"0", 1 << 17}, {"100", 1 << 17}, {"4095", 1 << 17},
                    {"4096", 4096}, {"4097", 4097}, {"1000000", 1000000}, {"-4096", 1 << 17}, {"jobs", 1 << 17}}) {
    set("COA_CERT_CHUNK_JOBS", c.value);
    EXPECT(cert_chunk_jobs() == c.want);
  }
  // COA_QUEUE_SLOTS (atoi; 1..8, anything else: the default)
  for (IntCase c : {IntCase{UNSET, 2}, {"", 2}, {"0", 2}, {"1", 1}, {"8", 8}, {"9", 2}, {"s", 2}}) {
    set("COA_QUEUE_SLOTS", c.value);
    EXPECT(queue_slots(2) == c.want);
  }
  // unsigned with default: COA_LAT_MAX (strtoull, default 2048), COA_MIN_SHARD
  // (65,536), COA_MSM_MIN (16,384), COA_FAULT_SHARD (0; "all" reads as 0)
  for (IntCase c : {IntCase{UNSET, 2048}, {"", 0}, {"0", 0}, {"1", 1}, {"4096", 4096}, {"lat", 0}, {"12ab", 12}}) {
    set("COA_LAT_MAX", c.value);
    EXPECT(env_u64("COA_LAT_MAX", 2048) == (unsigned long long)c.want);
  }
  set("COA_LAT_MAX", "18446744073709551615");
  EXPECT(env_u64("COA_LAT_MAX", 2048) == 18446744073709551615ull);
  set("COA_MIN_SHARD", UNSET);
  EXPECT(env_u64("COA_MIN_SHARD", 65536) == 65536);
  set("COA_MSM_MIN", UNSET);
  EXPECT(env_u64("COA_MSM_MIN", 16384) == 16384);
  set("COA_FAULT_SHARD", "all");
  EXPECT(env_u64("COA_FAULT_SHARD", 0) == 0 && env_is("COA_FAULT_SHARD", "all"));
  set("COA_FAULT_SHARD", "3");
  EXPECT(env_u64("COA_FAULT_SHARD", 0) == 3 && !env_is("COA_FAULT_SHARD", "all"));
  // MB as double, in bytes: COA_KEY_WCOMB_MB (atof, default 16 GiB)
  struct {
    const char* value;
    double want;
  } mb[] = {{UNSET, 16384.0 * 1048576.0}, {"", 0.0}, {"0", 0.0}, {"1", 1048576.0}, {"1.5", 1572864.0},
            {"131072", 131072.0 * 1048576.0}, {"-2", -2097152.0}, {"mb", 0.0}};
  for (auto& c : mb) {
    set("COA_KEY_WCOMB_MB", c.value);
    EXPECT(env_mb("COA_KEY_WCOMB_MB", 16384.0) == c.want);
  }
  set("COA_QUEUE_TRACE_SLOW_US", "250.5");
  EXPECT(env_double("COA_QUEUE_TRACE_SLOW_US", 0) == 250.5);
  set("COA_QUEUE_TRACE_SLOW_US", UNSET);
  EXPECT(env_double("COA_QUEUE_TRACE_SLOW_US", 7.0) == 7.0);
  // exact string match: COA_VERIFY_IMPL=full, COA_WCOMB=0, COA_CERT_LANES=1|64
  struct {
    const char* value;
    bool want;
  } is[] = {{UNSET, false}, {"", false}, {"full", true}, {"fullx", false}, {"ful", false}, {"FULL", false}, {" full", false}};
  for (auto& c : is) {
    set("COA_VERIFY_IMPL", c.value);
    EXPECT(env_is("COA_VERIFY_IMPL", "full") == c.want);
  }
  for (const char* v : {UNSET, "", "0", "00", "1", "64", "064"}) {
    set("COA_CERT_LANES", v);
    EXPECT(env_is("COA_CERT_LANES", "64") == (v && std::string(v) == "64"));
    EXPECT(env_is("COA_CERT_LANES", "1") == (v && std::string(v) == "1"));
    EXPECT(env_is("COA_CERT_LANES", "0") == (v && std::string(v) == "0"));
  }
  // on/off by the first character: COA_QUEUE_DIRECT, COA_QUEUE_INLINE, COA_QUEUE_KEYSORT
  struct {
    const char* value;
    bool dflt, want;
  } on[] = {{UNSET, true, true}, {UNSET, false, false}, {"", false, true}, {"0", true, false}, {"01", true, false},
            {"1", false, true}, {"10", false, true}, {"no", false, true}, {"off", false, true}};
  for (auto& c : on) {
    set("COA_QUEUE_DIRECT", c.value);
    EXPECT(env_on("COA_QUEUE_DIRECT", c.dflt) == c.want);
  }
  // the text itself: COA_QUEUE_LANES, and "is it set at all"
  set("COA_QUEUE_LANES", UNSET);
  EXPECT(env_str("COA_QUEUE_LANES") == nullptr);
  set("COA_QUEUE_LANES", "verify,digest");
  EXPECT(env_str("COA_QUEUE_LANES") && std::string(env_str("COA_QUEUE_LANES")) == "verify,digest");
}

static void check_offsets() {
  what = "offsets";
  const uint64_t one[] = {5}, equal[] = {3, 3, 3}, up[] = {0, 4, 4, 9, 20}, down[] = {0, 8, 4}, last_down[] = {0, 4, 8, 7};
  EXPECT(offsets_monotone(nullptr, 0));  // no item: nothing is read
  EXPECT(offsets_monotone(one, 0));
  EXPECT(offsets_monotone(equal, 2));
  EXPECT(offsets_monotone(up, 4));
  EXPECT(!offsets_monotone(down, 2));
  EXPECT(offsets_monotone(down, 1));  // only [0, n] is looked at
  EXPECT(!offsets_monotone(last_down, 3) && offsets_monotone(last_down, 2));

  const uint64_t off[] = {7, 9, 9, 15, 40, 41};  // n = 5
  EXPECT((rebased_offsets(off, 0, 5) == std::vector<uint64_t>{0, 2, 2, 8, 33, 34}));
  EXPECT((rebased_offsets(off, 2, 4) == std::vector<uint64_t>{0, 6, 31}));
  EXPECT((rebased_offsets(off, 4, 5) == std::vector<uint64_t>{0, 1}));
  EXPECT((rebased_offsets(off, 3, 3) == std::vector<uint64_t>{0}));  // empty range: its one boundary
  EXPECT((rebased_offsets(up, 0, 4) == std::vector<uint64_t>{0, 4, 4, 9, 20}));

  uint8_t id[32], origin[32], got[kDigestInput + 1];
  for (int i = 0; i < 32; i++) {
    id[i] = (uint8_t)(0x10 + i);
    origin[i] = (uint8_t)(0xe0 - i);
  }
  got[kDigestInput] = 0x5a;  // guard
  digest_input(got, id, 0x0123456789abcdefull, origin);  // a round beyond 2^32
  const uint8_t want[kDigestInput] = {
      0x10, 0x11, 0x12, 0x13, 0x14, 0x15, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x1b, 0x1c, 0x1d, 0x1e, 0x1f, 0x20, 0x21,
      0x22, 0x23, 0x24, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x2b, 0x2c, 0x2d, 0x2e, 0x2f,  // id
      0xef, 0xcd, 0xab, 0x89, 0x67, 0x45, 0x23, 0x01,                                      // round, little endian
      0xe0, 0xdf, 0xde, 0xdd, 0xdc, 0xdb, 0xda, 0xd9, 0xd8, 0xd7, 0xd6, 0xd5, 0xd4, 0xd3, 0xd2, 0xd1, 0xd0, 0xcf,
      0xce, 0xcd, 0xcc, 0xcb, 0xca, 0xc9, 0xc8, 0xc7, 0xc6, 0xc5, 0xc4, 0xc3, 0xc2, 0xc1};  // origin
  EXPECT(std::memcmp(got, want, kDigestInput) == 0 && got[kDigestInput] == 0x5a);
  digest_input(got, id, 1ull << 32, origin);
  EXPECT(got[32] == 0 && got[35] == 0 && got[36] == 1 && got[37] == 0 && got[39] == 0);
}

// Two threads submit kTasks tasks each to one Worker: every future answers
// its own task's code and message, a thread's tasks ran in the order it
// submitted them, every task ran on the worker's thread, after its start hook.
static thread_local bool t_hooked = false;
static void check_worker() {
  what = "worker";
  constexpr int kTasks = 8;
  std::vector<int> ran;  // task ids in the order they ran (the worker's thread only)
  int unhooked = 0;
  {
    Worker w([] { t_hooked = true; });
    std::vector<std::future<TaskResult>> futs[2];
    std::vector<std::thread> th;
    for (int t = 0; t < 2; t++)
      th.emplace_back([&, t] {
        for (int k = 0; k < kTasks; k++) {
          const int id = t * 100 + k;
          futs[t].push_back(w.submit([&ran, &unhooked, id] {
            if (!t_hooked) unhooked++;
            ran.push_back(id);
            return TaskResult(id % 3 ? -id : 0, id % 3 ? "task " + std::to_string(id) : std::string());
          }));
        }
      });
    for (auto& x : th) x.join();
    for (int t = 0; t < 2; t++)
      for (int k = 0; k < kTasks; k++) {
        const int id = t * 100 + k;
        const TaskResult r = futs[t][k].get();
        EXPECT(r.first == (id % 3 ? -id : 0));
        EXPECT(r.second == (id % 3 ? "task " + std::to_string(id) : std::string()));
      }
  }  // ~Worker joins its thread: `ran` is ours again
  EXPECT(ran.size() == 2 * kTasks && unhooked == 0 && !t_hooked);
  int next[2] = {0, 0};
  for (int id : ran) EXPECT(id % 100 == next[id / 100]++);
}

int main() {
  check_env();
  check_offsets();
  check_worker();
  printf("runtime host ok: %d bad\n", bad);
  return bad != 0;
}
