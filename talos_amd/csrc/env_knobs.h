// env_knobs.h — the readers of the TLSGPU_* environment knobs.  No HIP and no
// host-only includes: host_internal.h includes it for the .cpp units, and a
// .hip whose launcher reads knobs (chacha_kernels.hip) includes it directly.
//   env_on       set and not starting with '0' (unset, empty and "0" are off)
//   env_not_off  anything but a value starting with '0' (unset and empty are on)
//   env_uint     strtoull in `base` of a set, non-empty value, else `dflt`
//   env_starts   set and starting with `c` ('\0': set and empty) — for the
//                two knobs whose long-standing parsing the three above cannot say
#pragma once
#include <cstdint>
#include <cstdlib>

namespace tg {

inline bool env_on(const char* name) { const char* v = getenv(name); return v && *v && *v != '0'; }
inline bool env_not_off(const char* name) { const char* v = getenv(name); return !(v && *v == '0'); }
inline uint64_t env_uint(const char* name, uint64_t dflt, int base) {
  const char* v = getenv(name);
  return v && *v ? strtoull(v, nullptr, base) : dflt;
}
inline bool env_starts(const char* name, char c) { const char* v = getenv(name); return v && *v == c; }

}  // namespace tg
