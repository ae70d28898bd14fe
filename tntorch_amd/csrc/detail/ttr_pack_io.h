// 16-byte packs of a contiguous vector of n elements for the streaming kernels whose bits must not depend on the alignment of
// their pointers (ttr_ritz.hip, ttr_cg.hip): the wide and the element path fill the same pack registers.
#pragma once
#include "../ttr_common.h"

namespace ttr {

// elements [base, base + V) of x as one pack: one 16-byte load where WIDE and the pack lies inside n, element by element (zeros
// past n) otherwise
template <typename T, int V, bool WIDE>
__device__ __forceinline__ Pack<T, V> pack_load(const T* __restrict__ x, int64_t base, int64_t n) {
  Pack<T, V> p;
  if (WIDE && base + V <= n) {
    p = *reinterpret_cast<const Pack<T, V>*>(x + base);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) p.v[v] = base + v < n ? x[base + v] : T(0);
  }
  return p;
}

template <typename T, int V, bool WIDE>
__device__ __forceinline__ void pack_store(T* __restrict__ x, int64_t base, int64_t n, const Pack<T, V>& p) {
  if (WIDE && base + V <= n) {
    *reinterpret_cast<Pack<T, V>*>(x + base) = p;
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (base + v < n) x[base + v] = p.v[v];
  }
}

}  // namespace ttr
