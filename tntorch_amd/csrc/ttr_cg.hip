// One conjugate-gradient step of the local solves behind tt_amen_solve (ttamen.py) in three launches on the
// vectors v, r, p, Bp of n elements, and their extern "C" entries (profiling kind misc).  Streaming kernels with 256-thread
// blocks, HBM- or launch-bound; the matvec Bp = B p between two steps is the caller's.
//   ttr_cg_dot        part[0][g] = workgroup g's share of p . Bp, in double.  One pass, 16-byte packs.
//   ttr_cg_update     every workgroup adds part[0][*] in increasing g (the launch-boundary reduce: the sum of a launch finished in
//                     the next launch's prologue), forms alpha in double, updates its slice of v and r in place and writes its share
//                     of r . r (of the rounded r) to part[1][g]; workgroup 0 records the step in `state`.
//   ttr_cg_direction  every workgroup adds part[1][*], forms beta, and writes its slice of p = r + beta p; workgroup 0 stores the
//                     next rs.
// The recurrences are those of ttsolve._cg:
//   active = rs > thr2, good = pBp > 0, live = active & good, alpha = live ? rs / pBp : 0, v += alpha p, r -= alpha Bp,
//   rs' = r . r, beta = live ? rs' / max(rs, tiny) : 0, p = r + beta p.
// A step that is not live writes no vector and carries rs over (_cg sets p = r there, which no later step of a frozen solve reads
// and which a solve with p^T B p <= 0 does not survive: the driver raises on the count).
// state (fp64[8]).  [0], [1]: rs, read by step s from slot s & 1, written by its direction launch to slot 1 - (s & 1); [2]: thr2,
// the caller's, never written; [3]: the count of active steps with pBp <= 0; [4]: live, [5]: alpha, [6]: pBp of the last update;
// [7]: beta of the last direction.  Within one launch the words that are read ([s & 1], [2], and [4] in the direction launch) are
// never the words that are written (update: [3] .. [6]; direction: [1 - (s & 1)], [7]); [3] is read and written by one thread.
// Summation order.  Pack q (elements q V .. q V + V - 1, V = 16 bytes / sizeof(T)) belongs to thread q % 256 of workgroup
// (q / 256) % parts, which adds its packs in increasing q and a pack's elements in increasing index, one fma per product; the 64
// lanes of a wave meet in wave_sum, the four waves and then the workgroups in increasing order.  All three launches run `parts`
// workgroups, a function of n and the dtype (the rule of ritz_parts), so every sum is one fixed expression of n and the dtype:
// aligned or not, the bits are the same.  The scalar path (a pointer off a 16-byte boundary, and the last pack of an n that is no
// multiple of V) loads the same elements one by one into the same pack registers; past n they are zeros, which add nothing.
// Every index is bounded by n; `part` is bounded by workspace_bytes (checked on the host).  No atomics, no cooperative launch: the
// launches are ordered by the stream.
#include "detail/ttr_internal.h"
#include "detail/ttr_pack_io.h"

namespace ttr {

constexpr int kCgPacksPerThread = 4;   // as ritz_parts: a further workgroup joins per 256 * 4 packs

inline int cg_parts(int dtype, int64_t n) {
  const int64_t V = 16 / elem_size(dtype);
  const int64_t g = ceil_div(ceil_div(n, V), (int64_t)kThreads * kCgPacksPerThread);
  return (int)(g < 1 ? 1 : (g > TTR_CG_MAX_PARTS ? TTR_CG_MAX_PARTS : g));
}

inline int64_t cg_workspace_bytes(int dtype, int64_t n) { return 2 * (int64_t)cg_parts(dtype, n) * (int64_t)sizeof(double); }

// the sum of rows[0 .. nparts) in increasing order, in every thread (`stage` holds TTR_CG_MAX_PARTS doubles)
__device__ __forceinline__ double cg_finish_sum(const double* __restrict__ rows, int nparts, double* stage) {
  for (int i = threadIdx.x; i < nparts; i += kThreads) stage[i] = rows[i];
  __syncthreads();
  double s = stage[0];
  for (int g = 1; g < nparts; ++g) s += stage[g];
  return s;
}

// the workgroup's sum of acc (lanes in wave_sum, the four waves in increasing order) stored by thread 0
__device__ __forceinline__ void cg_store_share(double acc, double* red, double* out) {
  const double s = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
    for (int w = 1; w < kThreads / kWave; ++w) t += red[w];
    *out = t;
  }
}

template <typename T, bool WIDE>
__global__ __launch_bounds__(kThreads) void cg_dot_kernel(int64_t n, const T* __restrict__ P, const T* __restrict__ BP,
                                                          double* __restrict__ part) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ double red[kThreads / kWave];
  double acc = 0.0;
  const int64_t npacks = (n + V - 1) / V;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
    const int64_t base = q * V;
    const Pack<T, V> p = pack_load<T, V, WIDE>(P, base, n), bp = pack_load<T, V, WIDE>(BP, base, n);
#pragma unroll
    for (int v = 0; v < V; ++v) acc = fma((double)p.v[v], (double)bp.v[v], acc);
  }
  cg_store_share(acc, red, part + blockIdx.x);
}

template <typename T, bool WIDE>
__global__ __launch_bounds__(kThreads) void cg_update_kernel(int slot, int64_t n, int nparts, double* __restrict__ part,
                                                             const T* __restrict__ P, const T* __restrict__ BP, T* __restrict__ X,
                                                             T* __restrict__ R, double* __restrict__ state) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ double stage[TTR_CG_MAX_PARTS];
  __shared__ double red[kThreads / kWave];
  const double pBp = cg_finish_sum(part, nparts, stage);
  const double rs = state[slot], thr2 = state[2];
  const bool active = rs > thr2, good = pBp > 0.0, live = active && good;
  const double alpha = live ? rs / pBp : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (active && !good) state[3] += 1.0;
    state[4] = live ? 1.0 : 0.0;
    state[5] = alpha;
    state[6] = pBp;
  }
  double acc = 0.0;
  if (live) {
    const int64_t npacks = (n + V - 1) / V;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
      const int64_t base = q * V;
      const Pack<T, V> p = pack_load<T, V, WIDE>(P, base, n), bp = pack_load<T, V, WIDE>(BP, base, n);
      Pack<T, V> x = pack_load<T, V, WIDE>(X, base, n), r = pack_load<T, V, WIDE>(R, base, n);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        x.v[v] = (T)fma(alpha, (double)p.v[v], (double)x.v[v]);
        r.v[v] = (T)fma(-alpha, (double)bp.v[v], (double)r.v[v]);
        const double rd = (double)r.v[v];          // of the ROUNDED r: the norm of what is stored
        acc = fma(rd, rd, acc);
      }
      pack_store<T, V, WIDE>(X, base, n, x);
      pack_store<T, V, WIDE>(R, base, n, r);
    }
  }
  cg_store_share(acc, red, part + nparts + blockIdx.x);   // a step that is not live: zeros, which the direction launch ignores
}

template <typename T, bool WIDE>
__global__ __launch_bounds__(kThreads) void cg_direction_kernel(int slot, int64_t n, int nparts, const double* __restrict__ part,
                                                                const T* __restrict__ R, T* __restrict__ P,
                                                                double* __restrict__ state) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ double stage[TTR_CG_MAX_PARTS];
  const double rsn = cg_finish_sum(part + nparts, nparts, stage);
  const double rs = state[slot];
  const bool live = state[4] != 0.0;
  const double beta = live ? rsn / fmax(rs, (double)Num<T>::tiny()) : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state[1 - slot] = live ? rsn : rs;
    state[7] = beta;
  }
  if (!live) return;
  const int64_t npacks = (n + V - 1) / V;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
    const int64_t base = q * V;
    const Pack<T, V> r = pack_load<T, V, WIDE>(R, base, n);
    Pack<T, V> p = pack_load<T, V, WIDE>(P, base, n);
#pragma unroll
    for (int v = 0; v < V; ++v) p.v[v] = (T)fma(beta, (double)p.v[v], (double)r.v[v]);
    pack_store<T, V, WIDE>(P, base, n, p);
  }
}

// do the n-element vectors at a and b share a byte?
inline bool cg_overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

// the checks the three launches share; `vecs`: the launch's nv vectors, none of which may be null or overlap another
inline int cg_check(const char* who, int dtype, int64_t n, const void* const* vecs, int nv, const double* part,
                    int64_t workspace_bytes, bool rest) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(n >= 1, TTR_E_INVALID, "%s: n = %lld < 1", who, (long long)n);
  TTR_REQUIRE(n < (int64_t(1) << 57), TTR_E_UNSUPPORTED, "%s: vectors too long", who);
  bool ok = part != nullptr && rest;
  for (int i = 0; i < nv; ++i) ok = ok && vecs[i] != nullptr;
  TTR_REQUIRE(ok, TTR_E_INVALID, "%s: null pointer", who);
  for (int i = 0; i < nv; ++i)
    for (int j = i + 1; j < nv; ++j)
      TTR_REQUIRE(!cg_overlap(vecs[i], vecs[j], n * elem_size(dtype)), TTR_E_INVALID, "%s: the vectors overlap", who);
  TTR_REQUIRE(workspace_bytes >= cg_workspace_bytes(dtype, n), TTR_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", who,
              (long long)workspace_bytes, (long long)cg_workspace_bytes(dtype, n));
  return TTR_OK;
}

}  // namespace ttr

using namespace ttr;

extern "C" {

int ttr_cg_parts(int dtype, int64_t n) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_cg_parts: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 1, TTR_E_INVALID, "ttr_cg_parts: n = %lld < 1", (long long)n);
  return cg_parts(dtype, n);
}

int64_t ttr_cg_workspace_bytes(int dtype, int64_t n) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_cg_workspace_bytes: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 1, TTR_E_INVALID, "ttr_cg_workspace_bytes: n = %lld < 1", (long long)n);
  return cg_workspace_bytes(dtype, n);
}

int ttr_cg_dot(int dtype, int64_t n, const void* p, const void* Bp, double* part, int64_t workspace_bytes, void* stream) {
  const void* vecs[2] = {p, Bp};
  if (int e = cg_check("ttr_cg_dot", dtype, n, vecs, 2, part, workspace_bytes, true)) return e;
  const int parts = cg_parts(dtype, n);
  const bool wide = aligned16(p) && aligned16(Bp);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)parts), dim3(kThreads), 0, s, n, (const T*)p, (const T*)Bp, part);
    };
    if (wide) launch(cg_dot_kernel<T, true>);
    else launch(cg_dot_kernel<T, false>);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_cg_update(int dtype, int step, int64_t n, const void* p, const void* Bp, void* v, void* r, double* part,
                  int64_t workspace_bytes, double* state, void* stream) {
  const void* vecs[4] = {p, Bp, v, r};
  if (int e = cg_check("ttr_cg_update", dtype, n, vecs, 4, part, workspace_bytes, state != nullptr)) return e;
  TTR_REQUIRE(step >= 0, TTR_E_INVALID, "ttr_cg_update: step = %d < 0", step);
  const int parts = cg_parts(dtype, n);
  const bool wide = aligned16(p) && aligned16(Bp) && aligned16(v) && aligned16(r);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)parts), dim3(kThreads), 0, s, step & 1, n, parts, part, (const T*)p, (const T*)Bp,
                         (T*)v, (T*)r, state);
    };
    if (wide) launch(cg_update_kernel<T, true>);
    else launch(cg_update_kernel<T, false>);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_cg_direction(int dtype, int step, int64_t n, const void* r, void* p, const double* part, int64_t workspace_bytes,
                     double* state, void* stream) {
  const void* vecs[2] = {r, p};
  if (int e = cg_check("ttr_cg_direction", dtype, n, vecs, 2, part, workspace_bytes, state != nullptr)) return e;
  TTR_REQUIRE(step >= 0, TTR_E_INVALID, "ttr_cg_direction: step = %d < 0", step);
  const int parts = cg_parts(dtype, n);
  const bool wide = aligned16(r) && aligned16(p);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)parts), dim3(kThreads), 0, s, step & 1, n, parts, part, (const T*)r, (T*)p, state);
    };
    if (wide) launch(cg_direction_kernel<T, true>);
    else launch(cg_direction_kernel<T, false>);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // extern "C"
