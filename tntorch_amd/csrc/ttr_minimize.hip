// The minimisation step of TT-cross (cross.py:342-359, `_minimize`), one call per evaluated fibre block:
//   ttr_minimize_step   e[m] <- pi/2 - atan(e[m] - m0), and the running best sample (value, position) updated from the block
// with m0 = the best value so far (0 before the first one), read before anything is written.
//
// Pass 1 (minimize_pass_kernel) streams e once: 16-byte loads, the transform, 16-byte stores, and per lane the lexicographic
// minimum of (original value, index) over its finite entries.  A workgroup takes whole chunks of TTR_MINIMIZE_BLOCK_ELEMS
// consecutive elements of the 16-byte aligned body of e (chunk c goes to workgroup c mod gridDim.x: at most kMaxBlocks
// workgroups, so that the partials stay a few KB), a thread 4 (fp32) or 8 (fp64) packs of a chunk at distance 256 packs: all of
// them are loaded before the first is used.  The fewer than 2 V elements before the first and after the last aligned pack (a
// view that starts off a 16-byte boundary, a length that is no multiple of V) are single elements of workgroup 0.  The lanes'
// minima are combined across the wave (shuffles) and across the 4 waves (LDS); a workgroup writes ONE partial (value, index,
// non-finite seen) to the workspace.
//
// Pass 2 (minimize_update_kernel), one workgroup, launched behind pass 1 on the same stream: the minimum of the partials, the
// comparison with the state and, where the block's minimum is strictly smaller (or the state is empty), the new best value and
// its position lset[a, 1:] ++ [i] ++ rset[c, :-1].  A kernel boundary orders the partials against their reader: no ticket, no
// fence argument.  Every comparison is exact and (value, index) is a total order on the finite entries (-0.0 == +0.0: the lower
// index wins), so the result does not depend on how the reduction is split.  No atomics of any kind.
#include "detail/ttr_internal.h"

#include <math.h>

namespace ttr {

namespace {

constexpr int kBlockElems = TTR_MINIMIZE_BLOCK_ELEMS;
constexpr int64_t kMaxBlocks = 2048;   // 256 CUs x 8 workgroups: a memory-bound grid is capped there and strides over the chunks
constexpr int64_t kNone = INT64_MAX;   // index of "no finite entry seen"

__device__ __forceinline__ float atan_t(float x) { return atanf(x); }
__device__ __forceinline__ double atan_t(double x) { return atan(x); }

template <typename T>
__device__ __forceinline__ T inf_t() {
  return T(__builtin_huge_valf());
}

// (bv, bi) <- min((bv, bi), (v, i)) in the order: smaller value first, then smaller index
template <typename T>
__device__ __forceinline__ void key_min(T& bv, int64_t& bi, T v, int64_t i) {
  if (v < bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// The minimum over the 256 threads of a workgroup, valid in thread 0; `bad` <- any thread's bad
template <typename T>
__device__ __forceinline__ void block_key_min(T& bv, int64_t& bi, int& bad) {
  __shared__ T sv[kThreads / kWave];
  __shared__ int64_t si[kThreads / kWave];
  __shared__ int sb[kThreads / kWave];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T ov = __shfl_xor(bv, off, kWave);
    const int64_t oi = (int64_t)__shfl_xor((long long)bi, off, kWave);
    key_min(bv, bi, ov, oi);
  }
  bad = __any(bad) ? 1 : 0;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sv[w] = bv;
    si[w] = bi;
    sb[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kThreads / kWave; ++k) {
      key_min(bv, bi, sv[k], si[k]);
      bad |= sb[k];
    }
  }
}

template <typename T>
struct MinArgs {
  T* e;
  int64_t M;
  int64_t head;      // elements before the first 16-byte aligned one (all of e where it holds no aligned pack)
  int64_t nv;        // aligned packs
  int64_t nchunks;   // chunks of kBlockElems elements the packs form
  const T* best;
  const int32_t* flags;
  int64_t* p_idx;    // partials: one per workgroup
  T* p_val;
  int32_t* p_bad;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void minimize_pass_kernel(MinArgs<T> a) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int VC = kBlockElems / V;   // packs per chunk
  constexpr int VPT = VC / kThreads;    // packs per thread and chunk
  static_assert(VC % kThreads == 0, "a chunk is a whole number of packs per thread");
  using P = Pack<T, V>;
  const T m0 = a.flags[0] ? *a.best : T(0);
  const T half_pi = T(1.5707963267948966);
  T bv = inf_t<T>();
  int64_t bi = kNone;
  int bad = 0;
  auto one = [&](T v, int64_t i) -> T {
    if (__builtin_isfinite(v))
      key_min(bv, bi, v, i);
    else
      bad = 1;
    return half_pi - atan_t(v - m0);
  };

  P* body = reinterpret_cast<P*>(a.e + a.head);
  for (int64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    const int64_t v0 = c * VC + threadIdx.x;
    P p[VPT];
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int64_t vi = v0 + (int64_t)k * kThreads;
      if (vi < a.nv) p[k] = body[vi];
    }
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int64_t vi = v0 + (int64_t)k * kThreads;
      if (vi < a.nv) {
#pragma unroll
        for (int j = 0; j < V; ++j) p[k].v[j] = one(p[k].v[j], a.head + vi * V + j);
        body[vi] = p[k];
      }
    }
  }
  if (blockIdx.x == 0) {  // the elements outside the aligned packs: fewer than V in front, fewer than V behind
    const int64_t t = threadIdx.x;
    const int64_t i = t < a.head ? t : a.head + a.nv * V + (t - a.head);
    if (i < a.M) a.e[i] = one(a.e[i], i);
  }

  block_key_min(bv, bi, bad);
  if (threadIdx.x == 0) {
    a.p_idx[blockIdx.x] = bi;
    a.p_val[blockIdx.x] = bv;
    a.p_bad[blockIdx.x] = bad;
  }
}

template <typename T>
struct UpdateArgs {
  int64_t nparts;
  const int64_t* p_idx;
  const T* p_val;
  const int32_t* p_bad;
  int64_t I, Rb;
  const int64_t* lset;
  int64_t ld_lset, nl;
  const int64_t* rset;
  int64_t ld_rset, nr;
  T* best;
  int64_t* pos;
  int32_t* flags;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void minimize_update_kernel(UpdateArgs<T> a) {
  __shared__ int64_t s_m;
  T bv = inf_t<T>();
  int64_t bi = kNone;
  int bad = 0;
  for (int64_t p = threadIdx.x; p < a.nparts; p += kThreads) {
    key_min(bv, bi, a.p_val[p], a.p_idx[p]);
    bad |= a.p_bad[p];
  }
  block_key_min(bv, bi, bad);
  if (threadIdx.x == 0) {
    int64_t m = kNone;
    if (bad) {
      a.flags[1] = 1;   // the state is otherwise left alone
    } else if (bi != kNone && (!a.flags[0] || bv < *a.best)) {
      *a.best = bv;
      a.flags[0] = 1;
      m = bi;
    }
    s_m = m;
  }
  __syncthreads();
  const int64_t m = s_m;
  if (m == kNone) return;
  const int64_t c = m % a.Rb, ai = m / a.Rb;
  const int64_t i = ai % a.I, r = ai / a.I;
  const int64_t N = a.nl + 1 + a.nr;
  for (int64_t k = threadIdx.x; k < N; k += kThreads)
    a.pos[k] = k < a.nl ? a.lset[r * a.ld_lset + 1 + k] : k == a.nl ? i : a.rset[c * a.ld_rset + (k - a.nl - 1)];
}

int64_t minimize_blocks(int64_t M) {  // an upper bound of the workgroups of pass 1 (reached where e is 16-byte aligned)
  const int64_t n = ceil_div(M, kBlockElems);
  return n < 1 ? 1 : n > kMaxBlocks ? kMaxBlocks : n;
}

int64_t minimize_ws_bytes(int64_t M) { return align256(minimize_blocks(M) * (int64_t)(sizeof(int64_t) + 8 + sizeof(int32_t))); }

template <typename T>
int minimize_launch(T* e, int64_t M, int64_t I, int64_t Rb, const int64_t* lset, int64_t ld_lset, int64_t nl, const int64_t* rset,
                    int64_t ld_rset, int64_t nr, T* best, int64_t* pos, int32_t* flags, char* ws, hipStream_t stream) {
  constexpr int V = 16 / (int)sizeof(T);
  MinArgs<T> a;
  a.e = e;
  a.M = M;
  const int64_t off = (int64_t)(((uintptr_t)e & 15) / sizeof(T));   // e is aligned to its element size (checked)
  a.head = off ? V - off : 0;
  if (a.head > M) a.head = M;
  a.nv = (M - a.head) / V;
  a.nchunks = ceil_div(a.nv * V, kBlockElems);
  const int64_t nblk = a.nchunks < 1 ? 1 : a.nchunks > kMaxBlocks ? kMaxBlocks : a.nchunks;   // <= minimize_blocks(M)
  a.best = best;
  a.flags = flags;
  a.p_idx = reinterpret_cast<int64_t*>(ws);
  a.p_val = reinterpret_cast<T*>(ws + nblk * 8);
  a.p_bad = reinterpret_cast<int32_t*>(ws + nblk * 16);
  UpdateArgs<T> u;
  u.nparts = nblk;
  u.p_idx = a.p_idx;
  u.p_val = a.p_val;
  u.p_bad = a.p_bad;
  u.I = I;
  u.Rb = Rb;
  u.lset = lset;
  u.ld_lset = ld_lset;
  u.nl = nl;
  u.rset = rset;
  u.ld_rset = ld_rset;
  u.nr = nr;
  u.best = best;
  u.pos = pos;
  u.flags = flags;
  ProfScope prof(TTR_PROF_MISC, stream);
  hipLaunchKernelGGL((minimize_pass_kernel<T>), dim3((unsigned)nblk), dim3(kThreads), 0, stream, a);
  TTR_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((minimize_update_kernel<T>), dim3(1), dim3(kThreads), 0, stream, u);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int64_t ttr_minimize_workspace_bytes(int dtype, int64_t M) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_minimize_step: bad dtype %d", dtype);
  TTR_REQUIRE(M >= 1, TTR_E_INVALID, "ttr_minimize_step: bad size M = %lld", (long long)M);
  return minimize_ws_bytes(M);
}

extern "C" int ttr_minimize_step(int dtype, void* e, int64_t Ra, int64_t I, int64_t Rb, const void* lset, int64_t ld_lset, int64_t nl,
                                 const void* rset, int64_t ld_rset, int64_t nr, void* best, void* pos, void* flags, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  const char* who = "ttr_minimize_step";
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(Ra >= 1 && I >= 1 && Rb >= 1, TTR_E_INVALID, "%s: bad sizes Ra = %lld, I = %lld, Rb = %lld", who, (long long)Ra,
              (long long)I, (long long)Rb);
  TTR_REQUIRE(nl >= 0 && nr >= 0, TTR_E_INVALID, "%s: bad position lengths nl = %lld, nr = %lld", who, (long long)nl, (long long)nr);
  TTR_REQUIRE(e && lset && rset && best && pos && flags, TTR_E_INVALID, "%s: null pointer", who);
  TTR_REQUIRE((double)Ra * (double)I * (double)Rb < 9.0e18 / 64.0, TTR_E_UNSUPPORTED, "%s: block too large", who);
  TTR_REQUIRE((Ra == 1 || ld_lset >= nl + 1) && (Rb == 1 || ld_rset >= nr + 1), TTR_E_INVALID,
              "%s: row strides %lld, %lld below the row lengths %lld, %lld", who, (long long)ld_lset, (long long)ld_rset,
              (long long)(nl + 1), (long long)(nr + 1));
  TTR_REQUIRE((double)Ra * (double)ld_lset < 9.0e18 / 64.0 && (double)Rb * (double)ld_rset < 9.0e18 / 64.0, TTR_E_UNSUPPORTED,
              "%s: index sets too large", who);
  TTR_REQUIRE(((uintptr_t)e % (uintptr_t)elem_size(dtype)) == 0 && ((uintptr_t)best % (uintptr_t)elem_size(dtype)) == 0, TTR_E_INVALID,
              "%s: e and best must be aligned to the element size", who);
  const int64_t M = Ra * I * Rb;
  const int64_t need = minimize_ws_bytes(M);
  TTR_REQUIRE(workspace && workspace_bytes >= need, TTR_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who,
              (long long)(workspace ? workspace_bytes : 0), (long long)need);
  TTR_REQUIRE(((uintptr_t)workspace & 7) == 0, TTR_E_INVALID, "%s: workspace must be 8-byte aligned", who);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return minimize_launch<T>(static_cast<T*>(e), M, I, Rb, static_cast<const int64_t*>(lset), ld_lset, nl,
                              static_cast<const int64_t*>(rset), ld_rset, nr, static_cast<T*>(best), static_cast<int64_t*>(pos),
                              static_cast<int32_t*>(flags), static_cast<char*>(workspace), (hipStream_t)stream);
  });
}
