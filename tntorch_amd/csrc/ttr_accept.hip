// Level-by-level enumeration of the strings a mask accepts (automata.py:84-128 `accepted_inputs`, a Python recursion with one matmul
// per prefix there).  The frontier at mode mu is the productive prefixes in lexicographic order: prefix p has a left vector
// L[p, :] (fp64 [P, r]), a first output row off[p] and a count cnt[p] of output rows.  Per mode:
//   ttr_accept_count   C[p, i] = rint(L[p, :] . fiber[:, i])  (int64 [P, I]), fiber = core x_3 right_{mu+1} [r, I]
//   ttr_accept_expand  for slot k of the compacted children, (p, i) = divmod(idx[k], I):
//                        Lnew[k, :] = L[p, :] @ core[:, i, :]      (skipped at the last mode)
//                        offnew[k] = childoff[p, i], cntnew[k] = C[p, i]
//                      then every output row s of Xs[:, mu] receives the symbol of the slot whose run [offnew[k], offnew[k] + cntnew[k])
//                      holds it, and the consistency word is ORed.
// Only the slots listed in idx are expanded: the children of unproductive prefixes are never computed.
//
// Everything is fp64 whatever the cores' dtype (path counts are integers and stay exact up to 2^53): fp32 cores and fibers are
// converted at the load.  Integer-valued inputs give the same bits in any order of summation.
//
// count: one thread per (p, i), a loop over r; the lanes of a wave cover consecutive (p, i), so L[p, a] is one address per run of
// I lanes and fiber[a, i] I consecutive addresses.
// expand, first kernel: one thread per (k, b), b the column of Lnew; a run of r' lanes shares L[p, a] (one address) and reads r'
// consecutive elements of core[a, i, :]; the stores of Lnew are consecutive across the lanes.  The lane b = 0 stores offnew[k] and
// cntnew[k].  The first P threads also check their parent: every C[p, i] >= 0 and sum_i C[p, i] == cnt[p].
// expand, second kernel: one thread per output row s (grid-stride), a binary search for the last k with offnew[k] <= s, one
// 8-byte store at Xs[s, mu].  A run of one slot may span millions of rows at the first modes, so the rows, not the slots, are
// spread over the threads.
//
// Bounds: every store is indexed by a thread's own slot k < K, row s < S or parent; the only data-dependent addresses are LOADS
// at idx[k], which is checked against [0, P I) (outside: the slot is skipped and TTR_ACCEPT_BAD_INDEX is ORed).  The search
// terminates with 0 <= k < K for any content of offnew.  All stores are plain 8-byte vector stores; the word is ORed with one
// vector atomic, only where a check fails.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int kMaxRank = 1024;        // r and r': the kernels loop over r per output, untiled
constexpr double kExact = 9007199254740992.0;  // 2^53

template <typename T>
struct CountArgs {
  int64_t P, r, I;
  const double* L;
  const T* fiber;
  int64_t* C;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void accept_count_kernel(CountArgs<T> a) {
  const int64_t total = a.P * a.I;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < total; g += (int64_t)gridDim.x * kThreads) {
    const int64_t p = g / a.I, i = g - p * a.I;
    const double* Lp = a.L + p * a.r;
    const T* f = a.fiber + i;
    double acc = 0.0;
    for (int64_t k = 0; k < a.r; ++k) acc = fma(Lp[k], (double)f[k * a.I], acc);
    // beyond +-2^53 (or NaN) nothing is exact: saturate, the sums then disagree with their parent and expand flags it
    acc = fmin(fmax(rint(acc), -kExact), kExact);
    a.C[g] = (int64_t)acc;
  }
}

template <typename T>
struct ExpandArgs {
  int64_t P, r, I, rn, K, N, mu, S;
  const double* L;
  const T* core;
  const int64_t* C;
  const int64_t* childoff;
  const int64_t* cnt;
  const int64_t* idx;
  double* Lnew;  // null at the last mode
  int64_t* offnew;
  int64_t* cntnew;
  int64_t* Xs;
  int* flag;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void accept_expand_kernel(ExpandArgs<T> a) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g < a.P) {  // parent check
    int64_t sum = 0;
    bool neg = false;
    for (int64_t i = 0; i < a.I; ++i) {
      const int64_t c = a.C[g * a.I + i];
      neg |= c < 0;
      sum += c;
    }
    const int bits = (neg ? TTR_ACCEPT_NEGATIVE : 0) | (sum != a.cnt[g] ? TTR_ACCEPT_SUM_MISMATCH : 0);
    if (bits) atomicOr(a.flag, bits);
  }
  const int64_t cols = a.Lnew ? a.rn : 1;
  if (g >= a.K * cols) return;
  const int64_t k = g / cols, b = g - k * cols;
  const int64_t pos = a.idx[k];
  if (pos < 0 || pos >= a.P * a.I) {
    if (b == 0) atomicOr(a.flag, TTR_ACCEPT_BAD_INDEX);
    return;
  }
  const int64_t p = pos / a.I, i = pos - p * a.I;
  if (b == 0) {
    a.offnew[k] = a.childoff[pos];
    a.cntnew[k] = a.C[pos];
  }
  if (!a.Lnew) return;
  const double* Lp = a.L + p * a.r;
  const T* c = a.core + i * a.rn + b;  // core[x, i, b] = c[x I rn]
  const int64_t cs = a.I * a.rn;
  double acc = 0.0;
  for (int64_t x = 0; x < a.r; ++x) acc = fma(Lp[x], (double)c[x * cs], acc);
  a.Lnew[k * a.rn + b] = acc;
}

__global__ __launch_bounds__(kThreads) void accept_fill_kernel(int64_t S, int64_t N, int64_t mu, int64_t I, int64_t K,
                                                               const int64_t* __restrict__ offnew, const int64_t* __restrict__ idx,
                                                               int64_t* __restrict__ Xs) {
  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < S; s += (int64_t)gridDim.x * kThreads) {
    int64_t lo = 0, hi = K;  // the last k in [0, K) with offnew[k] <= s (k = 0 when there is none)
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (offnew[mid] <= s) lo = mid; else hi = mid;
    }
    const int64_t pos = idx[lo];
    Xs[s * N + mu] = pos >= 0 ? pos % I : 0;
  }
}

inline unsigned grid_for(int64_t threads, int64_t cap) {
  const int64_t blocks = ceil_div(threads, kThreads);
  return (unsigned)(blocks < cap ? (blocks < 1 ? 1 : blocks) : cap);
}

template <typename T>
int count_impl(CountArgs<T> a, hipStream_t stream) {
  ProfScope prof(TTR_PROF_MISC, stream);
  hipLaunchKernelGGL((accept_count_kernel<T>), dim3(grid_for(a.P * a.I, 8192)), dim3(kThreads), 0, stream, a);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

template <typename T>
int expand_impl(ExpandArgs<T> a, hipStream_t stream) {
  ProfScope prof(TTR_PROF_MISC, stream);
  const int64_t work = a.K * (a.Lnew ? a.rn : 1);
  const int64_t threads = work > a.P ? work : a.P;
  hipLaunchKernelGGL((accept_expand_kernel<T>), dim3((unsigned)ceil_div(threads, kThreads)), dim3(kThreads), 0, stream, a);
  TTR_HIP_CHECK(hipGetLastError());
  if (a.K > 0 && a.S > 0) {
    hipLaunchKernelGGL(accept_fill_kernel, dim3(grid_for(a.S, 8192)), dim3(kThreads), 0, stream, a.S, a.N, a.mu, a.I, a.K,
                       (const int64_t*)a.offnew, a.idx, a.Xs);
    TTR_HIP_CHECK(hipGetLastError());
  }
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_accept_max_rank(void) { return kMaxRank; }

extern "C" int ttr_accept_count(int dtype, int64_t P, int64_t r, int64_t I, const void* L, const void* fiber, void* C, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_accept_count: bad dtype %d", dtype);
  TTR_REQUIRE(P >= 1 && r >= 1 && I >= 1, TTR_E_INVALID, "ttr_accept_count: bad sizes P = %lld, r = %lld, I = %lld", (long long)P,
              (long long)r, (long long)I);
  TTR_REQUIRE(r <= kMaxRank, TTR_E_INVALID, "ttr_accept_count: rank %lld above the limit of %d (ttr_accept_max_rank)", (long long)r,
              kMaxRank);
  TTR_REQUIRE(I <= 2147483647LL && (double)P * (double)I < 4.0e18 / 8.0, TTR_E_UNSUPPORTED, "ttr_accept_count: frontier too large");
  TTR_REQUIRE(L && fiber && C, TTR_E_INVALID, "ttr_accept_count: null pointer");
  TTR_REQUIRE(C != L && C != fiber, TTR_E_INVALID, "ttr_accept_count: C must not be an input");
  return by_dtype(dtype, [&](auto t) {   // (L is fp64 for both dtypes)
    using T = decltype(t);
    return count_impl<T>({P, r, I, (const double*)L, (const T*)fiber, (int64_t*)C}, (hipStream_t)stream);
  });
}

extern "C" int ttr_accept_expand(int dtype, int64_t P, int64_t r, int64_t I, int64_t rn, int64_t K, int64_t N, int64_t mu, int64_t S,
                                 const void* L, const void* core, const void* C, const void* childoff, const void* cnt,
                                 const void* idx, void* Lnew, void* offnew, void* cntnew, void* Xs, void* flag, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_accept_expand: bad dtype %d", dtype);
  TTR_REQUIRE(P >= 1 && r >= 1 && I >= 1 && rn >= 1 && K >= 0 && S >= 0 && N >= 1 && mu >= 0 && mu < N, TTR_E_INVALID,
              "ttr_accept_expand: bad sizes P = %lld, core [%lld, %lld, %lld], K = %lld, S = %lld, mode %lld of %lld", (long long)P,
              (long long)r, (long long)I, (long long)rn, (long long)K, (long long)S, (long long)mu, (long long)N);
  TTR_REQUIRE(r <= kMaxRank && rn <= kMaxRank, TTR_E_INVALID,
              "ttr_accept_expand: ranks %lld, %lld above the limit of %d (ttr_accept_max_rank)", (long long)r, (long long)rn, kMaxRank);
  TTR_REQUIRE(K <= P * I, TTR_E_INVALID, "ttr_accept_expand: %lld slots from %lld children", (long long)K, (long long)(P * I));
  TTR_REQUIRE(I <= 2147483647LL && (double)P * (double)I < 4.0e18 / 8.0 && (double)S * (double)N < 4.0e18 / 8.0 &&
                  (double)K * (double)rn < 2147483647.0 * kThreads && (double)P < 2147483647.0 * kThreads,
              TTR_E_UNSUPPORTED, "ttr_accept_expand: frontier too large");
  TTR_REQUIRE(L && core && C && childoff && cnt && flag, TTR_E_INVALID, "ttr_accept_expand: null pointer");
  TTR_REQUIRE(K == 0 || (idx && offnew && cntnew), TTR_E_INVALID, "ttr_accept_expand: null pointer (slots)");
  TTR_REQUIRE(K == 0 || S == 0 || Xs, TTR_E_INVALID, "ttr_accept_expand: null pointer (Xs)");
  return by_dtype(dtype, [&](auto t) {   // (L and Lnew are fp64 for both dtypes)
    using T = decltype(t);
    return expand_impl<T>({P, r, I, rn, K, N, mu, S, (const double*)L, (const T*)core, (const int64_t*)C, (const int64_t*)childoff,
                           (const int64_t*)cnt, (const int64_t*)idx, (double*)Lnew, (int64_t*)offnew, (int64_t*)cntnew, (int64_t*)Xs,
                           (int*)flag},
                          (hipStream_t)stream);
  });
}
