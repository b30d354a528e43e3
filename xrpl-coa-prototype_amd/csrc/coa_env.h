// The typed readers of the engine's COA_* environment switches (host-only, no
// HIP): every switch is read through one of these, so an unset, empty or
// non-numeric value means the same thing at every site.  Numbers parse as
// strtol / strtoull / strtod do: leading text that is no number reads as 0.
// A reader reads the environment when it is called; whether a switch is read
// per call or once is its site's choice.
#pragma once

#include <cstdlib>
#include <cstring>

namespace coa_rt __attribute__((visibility("hidden"))) {

// The switch's text, or null when it is unset.
inline const char* env_str(const char* name) { return getenv(name); }

// Set to exactly `value`.
inline bool env_is(const char* name, const char* value) {
  const char* v = getenv(name);
  return v && std::strcmp(v, value) == 0;
}

// On/off by the first character: "0..." is off, anything else (the empty
// string too) is on; unset: dflt.
inline bool env_on(const char* name, bool dflt) {
  const char* v = getenv(name);
  return v ? v[0] != '0' : dflt;
}

// Unsigned decimal; unset: dflt.
inline unsigned long long env_u64(const char* name, unsigned long long dflt) {
  const char* v = getenv(name);
  return v ? strtoull(v, nullptr, 10) : dflt;
}

// Signed decimal; unset: dflt.
inline long env_int(const char* name, long dflt) {
  const char* v = getenv(name);
  return v ? strtol(v, nullptr, 10) : dflt;
}

// Signed decimal clamped to [lo, hi]; unset: dflt as it is.
inline long env_int(const char* name, long dflt, long lo, long hi) {
  const char* v = getenv(name);
  if (!v) return dflt;
  const long x = strtol(v, nullptr, 10);
  return x < lo ? lo : (x > hi ? hi : x);
}

// Floating point; unset: dflt.
inline double env_double(const char* name, double dflt) {
  const char* v = getenv(name);
  return v ? atof(v) : dflt;
}

// A size given in MiB, as bytes; unset: dflt_mb MiB.
inline double env_mb(const char* name, double dflt_mb) { return env_double(name, dflt_mb) * 1048576.0; }

}  // namespace coa_rt
