// Grouping of P samples by one index column on the device: a counting sort without a host round trip (histogram, scan with
// per-group tile offsets, scatter of sample ids), and the validation of an index column.  Shared by ttr_index.hip
// (ttr_gather_chain, ttr_gather_step) and ttr_ttlookup.hip (ttr_ttm_lookup_step): one copy of the kernels, compiled into each
// unit that includes this file (they sit in an unnamed namespace, so every unit owns its instances and nothing is exported).
//
// DEVICE code, unlike ttr_internal.h next to it: include it only from a unit that launches these kernels.
//
//   validate_kernel   ORs *flag with 1 when an entry of the column lies outside its extent
//   histogram_kernel  cnt[v] += number of samples with index v                        (cnt zeroed by the caller)
//   scan_kernel       off[v] = exclusive scan of cnt; toff[v] = exclusive scan of the tiles of kGroupTileRows rows that group v
//                     needs when every sample brings `ra` rows, toff[I] = their total
//   scatter_kernel    perm[off[v] + k] = the k-th sample (in no particular order) with index v   (cursor zeroed by the caller)
// Every kernel but validate_kernel returns at entry when *flag is set.
//   enqueue_group_sort  (host) the three launches above for one column
//   group_of_tile       (device) the group a row tile of a consumer's step kernel belongs to
#pragma once
#include "../ttr_common.h"

namespace ttr {
namespace {

constexpr int kGroupTileRows = 64;  // rows per tile of the consumers' step kernels
constexpr int kLdsBins = 1024;      // mode sizes up to this histogram / scatter in LDS first

struct IdxCol {
  const void* p;
  int64_t stride;
  int is64;
};

__device__ __forceinline__ int64_t load_idx(const IdxCol& c, int64_t q) {
  return c.is64 ? ((const int64_t*)c.p)[q * c.stride] : (int64_t)((const int32_t*)c.p)[q * c.stride];
}

// wrapped index of point q, or -1 when out of range; wrap == 0: negative values are out of range too (row maps)
__device__ __forceinline__ int64_t idx_value(const IdxCol& c, int64_t q, int64_t I, int wrap = 1) {
  int64_t v = load_idx(c, q);
  if (v < 0 && wrap) v += I;
  return (v < 0 || v >= I) ? -1 : v;
}

__global__ void __launch_bounds__(kThreads) validate_kernel(IdxCol c, int64_t P, int64_t I, int32_t* flag, int wrap) {
  int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  bool bad = q < P && idx_value(c, q, I, wrap) < 0;
  if (__any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(flag, 1);
}

__global__ void __launch_bounds__(kThreads) histogram_kernel(IdxCol c, int64_t P, int64_t I, int32_t* cnt, const int32_t* flag) {
  __shared__ int32_t h[kLdsBins];
  if (*flag) return;
  const bool lds = I <= kLdsBins;
  if (lds)
    for (int v = threadIdx.x; v < I; v += kThreads) h[v] = 0;
  __syncthreads();
  int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q < P) {
    int64_t v = idx_value(c, q, I);
    if (v >= 0) {
      if (lds)
        atomicAdd(&h[v], 1);
      else
        atomicAdd(&cnt[v], 1);
    }
  }
  __syncthreads();
  if (lds)
    for (int v = threadIdx.x; v < I; v += kThreads)
      if (h[v]) atomicAdd(&cnt[v], h[v]);
}

// one workgroup: off[v] = exclusive scan of cnt, toff[v] = exclusive scan of the tiles of each group (toff[I] = total)
__global__ void __launch_bounds__(1024) scan_kernel(const int32_t* cnt, int64_t I, int64_t ra, int64_t* off, int64_t* toff,
                                                    const int32_t* flag) {
  __shared__ int64_t s0[1024], s1[1024];
  __shared__ int64_t carry0, carry1;
  if (*flag) return;
  if (threadIdx.x == 0) carry0 = carry1 = 0;
  __syncthreads();
  for (int64_t base = 0; base < I; base += 1024) {
    int64_t v = base + threadIdx.x;
    int64_t c = v < I ? cnt[v] : 0;
    int64_t a = c, t = (c * ra + kGroupTileRows - 1) / kGroupTileRows;
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = t;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
      int64_t x0 = threadIdx.x >= d ? s0[threadIdx.x - d] : 0, x1 = threadIdx.x >= d ? s1[threadIdx.x - d] : 0;
      __syncthreads();
      s0[threadIdx.x] += x0;
      s1[threadIdx.x] += x1;
      __syncthreads();
    }
    if (v < I) {
      off[v] = carry0 + s0[threadIdx.x] - a;
      toff[v] = carry1 + s1[threadIdx.x] - t;
    }
    __syncthreads();
    if (threadIdx.x == 1023) {
      carry0 += s0[1023];
      carry1 += s1[1023];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) toff[I] = carry1;
}

// perm[off[v] + k] = the k-th point (in no particular order) whose index is v.  The order inside a group does not matter: every
// row's result depends on its own inputs only.
__global__ void __launch_bounds__(kThreads) scatter_kernel(IdxCol c, int64_t P, int64_t I, const int64_t* off, int32_t* cursor,
                                                           int64_t* perm, const int32_t* flag) {
  __shared__ int32_t h[kLdsBins], base[kLdsBins];
  if (*flag) return;
  const bool lds = I <= kLdsBins;
  if (lds)
    for (int v = threadIdx.x; v < I; v += kThreads) h[v] = 0;
  __syncthreads();
  int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t v = q < P ? idx_value(c, q, I) : -1;
  int32_t local = 0;
  if (v >= 0 && lds) local = atomicAdd(&h[v], 1);
  __syncthreads();
  if (lds)
    for (int u = threadIdx.x; u < I; u += kThreads)
      if (h[u]) base[u] = atomicAdd(&cursor[u], h[u]);
  __syncthreads();
  if (v >= 0) {
    int64_t pos = lds ? (int64_t)base[v] + local : (int64_t)atomicAdd(&cursor[v], 1);
    perm[off[v] + pos] = q;
  }
}

// The group of row tile `mt` of the grouped row space (tiles of kGroupTileRows rows that never straddle two groups): the largest
// v with toff[v] <= mt, found by thread 0 and handed round through *s_v, a word of the caller's LDS (a workgroup barrier: all
// threads call this).  For mt < toff[I].  The tile's first row is row (mt - toff[v]) kGroupTileRows of the group's.
__device__ __forceinline__ int64_t group_of_tile(const int64_t* toff, int64_t I, int64_t mt, int64_t* s_v) {
  if (threadIdx.x == 0) {
    int64_t hi = I - 1, lo = 0;   // (hi declared first: the other order swaps the operands of an addition in both callers)
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (toff[mid] <= mt) lo = mid; else hi = mid - 1;
    }
    *s_v = lo;
  }
  __syncthreads();
  return *s_v;
}

// The counting sort of the P samples by column c, enqueued: perm lists the samples group by group, off / toff as scan_kernel
// leaves them.  cnt and cursor ([I] each) are zeroed by the caller.
inline void enqueue_group_sort(IdxCol c, int64_t P, int64_t I, int64_t ra, int32_t* cnt, int32_t* cursor, int64_t* off, int64_t* toff,
                               int64_t* perm, const int32_t* flag, hipStream_t stream) {
  const unsigned pb = (unsigned)((P + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(histogram_kernel, dim3(pb), dim3(kThreads), 0, stream, c, P, I, cnt, flag);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, I, ra, off, toff, flag);
  hipLaunchKernelGGL(scatter_kernel, dim3(pb), dim3(kThreads), 0, stream, c, P, I, off, cursor, perm, flag);
}

}  // namespace
}  // namespace ttr
