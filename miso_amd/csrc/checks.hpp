// The pointer predicates of the C ABI layer: what capi.hip and the C entry points of hash_sdf.hip state their argument
// checks with.
#pragma once
#include <stdint.h>

namespace miso {

template <class... P> inline bool aligned(uintptr_t bytes, const P*... p) {   // NULL passes: optional pointers
  return ((... | (uintptr_t)p) & (bytes - 1)) == 0;
}
template <class... P> inline bool all_set(const P*... p) { return (... && (p != nullptr)); }
template <class... P> inline bool set_if(int64_t n, const P*... p) { return n <= 0 || all_set(p...); }   // non-NULL when n > 0

}  // namespace miso
