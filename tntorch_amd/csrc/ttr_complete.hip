// TT completion by alternating least squares (interpolation.py:9-119): the per-slice least-squares step of one core.
//
// For core mu (ranks r0, r1, K = r0 r1) every sample p contributes the Khatri-Rao row k_p = L_p (x) R_p, k_p[a r1 + b] =
// L_p[a] R_p[b], to the system of its slice i = X[p, mu].  The reference forms the design matrix of each slice explicitly and
// calls lstsq per slice; here
//   ttr_als_normal   accumulates G = sum w_p^2 k_p k_p^T and h = sum w_p^2 y_p k_p per TASK (a run of at most a few thousand
//                    samples of one slice, in the order of the mode's sample permutation) on the matrix cores, the rows k_p formed
//                    on the fly from LDS-staged L / R rows: the P x K design matrix never exists in memory;
//   ttr_spd_solve    sums the tasks of each slice on load and solves G x = h by Cholesky, one workgroup per slice, and writes x
//                    straight into the new core; a slice whose pivot falls to K eps max(diag G) or below is flagged and left to
//                    the minimum-norm fallback (ttr_eigh_trunc + ttr_gemm + ttr_pinv_finish).
#include "detail/ttr_internal.h"

namespace ttr {
namespace {

constexpr int kTilesPerWave = 4;                                   // 16 x 16 accumulator tiles a wave holds at once
constexpr int kTilesPerGroup = kTilesPerWave * (kThreads / kWave);  // tiles of G one workgroup computes
constexpr int64_t kMaxK = 1024;
constexpr int64_t kStageBytes = 48 * 1024;  // LDS for the staged sample rows of ttr_als_normal
constexpr int64_t kSolveLdsBytes = 60 * 1024;  // + the static reduction buffer: below the 64 KiB default

__device__ __forceinline__ void tile_of(int q, int& ti, int& tj) {  // q-th tile of the lower triangle, row by row
  int t = (int)((sqrtf(8.f * (float)q + 1.f) - 1.f) * 0.5f);
  while (t * (t + 1) / 2 > q) --t;
  while ((t + 1) * (t + 2) / 2 <= q) ++t;
  ti = t;
  tj = q - t * (t + 1) / 2;
}

// grid (ntasks, tile groups).  LDS: S staged samples of w L (S x r0), R (S x r1), w y (S) and their ids.
template <typename T>
__global__ void __launch_bounds__(kThreads) als_normal_kernel(int r0, int r1, int S, const T* __restrict__ L, int64_t ldl,
                                                              const T* __restrict__ R, int64_t ldr, const T* __restrict__ w,
                                                              const T* __restrict__ y, const int64_t* __restrict__ perm,
                                                              const int64_t* __restrict__ tb, const int64_t* __restrict__ te,
                                                              T* __restrict__ Gp, T* __restrict__ hp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* sL = (T*)smem_raw;
  T* sR = sL + (int64_t)S * r0;
  T* sWY = sR + (int64_t)S * r1;
  int64_t* sQ = (int64_t*)(sWY + S);
  using M = Mfma<T>;
  const int K = r0 * r1;
  const int nT = (K + 15) / 16;
  const int ntiles = nT * (nT + 1) / 2;
  const int64_t task = blockIdx.x;
  const int group = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t b = tb[task], e = te[task];

  // this lane's Khatri-Rao coordinates in each of the wave's tiles: row i (A operand) and column j (B operand)
  int ia[kTilesPerWave], ib[kTilesPerWave], ja[kTilesPerWave], jb[kTilesPerWave], tI[kTilesPerWave], tJ[kTilesPerWave];
  bool live[kTilesPerWave];
#pragma unroll
  for (int u = 0; u < kTilesPerWave; ++u) {
    const int q = group * kTilesPerGroup + wave * kTilesPerWave + u;
    live[u] = q < ntiles;
    int ti = 0, tj = 0;
    if (live[u]) tile_of(q, ti, tj);
    tI[u] = ti;
    tJ[u] = tj;
    const int i = ti * 16 + (lane & 15), j = tj * 16 + (lane & 15);
    ia[u] = i < K ? i / r1 : -1;
    ib[u] = i < K ? i % r1 : 0;
    ja[u] = j < K ? j / r1 : -1;
    jb[u] = j < K ? j % r1 : 0;
  }
  typename M::Acc acc[kTilesPerWave];
#pragma unroll
  for (int u = 0; u < kTilesPerWave; ++u) acc[u] = M::zero();
  const bool do_h = group == 0;
  T hacc[kMaxK / kThreads];
#pragma unroll
  for (int u = 0; u < (int)(kMaxK / kThreads); ++u) hacc[u] = T(0);

  for (int64_t c0 = b; c0 < e; c0 += S) {
    const int n = (int)min((int64_t)S, e - c0);
    __syncthreads();
    for (int p = tid; p < S; p += kThreads) sQ[p] = p < n ? perm[c0 + p] : -1;
    __syncthreads();
    for (int x = tid; x < S * r0; x += kThreads) {
      const int p = x / r0, a = x - p * r0;
      const int64_t q = sQ[p];
      sL[x] = q >= 0 ? (w ? w[q] : T(1)) * L[q * ldl + a] : T(0);
    }
    for (int x = tid; x < S * r1; x += kThreads) {
      const int p = x / r1, c = x - p * r1;
      const int64_t q = sQ[p];
      sR[x] = q >= 0 ? R[q * ldr + c] : T(0);
    }
    for (int p = tid; p < S; p += kThreads) {
      const int64_t q = sQ[p];
      sWY[p] = q >= 0 ? (w ? w[q] : T(1)) * y[q] : T(0);
    }
    __syncthreads();
    const int kq = lane >> 4;
    for (int k0 = 0; k0 < n; k0 += 4) {
      const int p = k0 + kq;  // p < S: S is a multiple of 4 and rows past n are zero
#pragma unroll
      for (int u = 0; u < kTilesPerWave; ++u) {
        if (!live[u]) continue;
        const T av = ia[u] >= 0 ? sL[p * r0 + ia[u]] * sR[p * r1 + ib[u]] : T(0);
        const T bv = ja[u] >= 0 ? sL[p * r0 + ja[u]] * sR[p * r1 + jb[u]] : T(0);
        acc[u] = M::mma(av, bv, acc[u]);
      }
    }
    if (do_h) {
#pragma unroll
      for (int u = 0; u < (int)(kMaxK / kThreads); ++u) {
        const int c = tid + u * kThreads;
        if (c < K) {
          const int a = c / r1, bb = c - a * r1;
          T s = hacc[u];
          for (int p = 0; p < n; ++p) s += sWY[p] * (sL[p * r0 + a] * sR[p * r1 + bb]);
          hacc[u] = s;
        }
      }
    }
  }

  T* G = Gp + task * (int64_t)K * K;
#pragma unroll
  for (int u = 0; u < kTilesPerWave; ++u) {
    if (!live[u]) continue;
    const int j = tJ[u] * 16 + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = tI[u] * 16 + M::row(lane, reg);
      if (i < K && j < K && (tI[u] != tJ[u] || i >= j)) {  // diagonal tiles: the lower half, mirrored (G is exactly symmetric)
        G[(int64_t)i * K + j] = acc[u][reg];
        G[(int64_t)j * K + i] = acc[u][reg];
      }
    }
  }
  if (do_h) {
#pragma unroll
    for (int u = 0; u < (int)(kMaxK / kThreads); ++u) {
      const int c = tid + u * kThreads;
      if (c < K) hp[task * K + c] = hacc[u];
    }
  }
}

struct XOut {  // solution entry k of item `it` -> X[it * s_item + (k / inner) * s_a + (k % inner) * s_b]
  int64_t inner, s_item, s_a, s_b;
  __device__ __forceinline__ int64_t at(int64_t it, int k) const { return it * s_item + (k / inner) * s_a + (k % inner) * s_b; }
};

template <typename T>
__device__ void sum_parts(int K, const T* __restrict__ Gp, const T* __restrict__ hp, int64_t p0, int64_t p1, T* A, T* z) {
  const int64_t KK = (int64_t)K * K;
  for (int64_t x = threadIdx.x; x < KK; x += kThreads) {
    T s = T(0);
    for (int64_t p = p0; p < p1; ++p) s += Gp[p * KK + x];
    A[x] = s;
  }
  for (int k = threadIdx.x; k < K; k += kThreads) {
    T s = T(0);
    for (int64_t p = p0; p < p1; ++p) s += hp[p * K + k];
    z[k] = s;
  }
}

// One workgroup per item.  LDS == true: the K x K matrix and h live in LDS; false: they are factored in place in Gsum / hsum
// (global memory, L2-resident), which a flagged item then overwrites with its summed system again.
template <typename T, bool LDS>
__global__ void __launch_bounds__(kThreads) spd_solve_kernel(int K, const T* __restrict__ Gp, const T* __restrict__ hp,
                                                             const int64_t* __restrict__ poff, int64_t pbase, T* __restrict__ X,
                                                             XOut xo, T* __restrict__ Gsum, T* __restrict__ hsum,
                                                             int32_t* __restrict__ status, const int64_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ T red[kThreads];
  const int64_t it = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t p0 = poff[it] - pbase, p1 = poff[it + 1] - pbase;
  const int64_t KK = (int64_t)K * K;
  T* A = LDS ? (T*)smem_raw : Gsum + it * KK;
  T* z = LDS ? (T*)smem_raw + KK : hsum + it * K;
  sum_parts<T>(K, Gp, hp, p0, p1, A, z);
  __syncthreads();
  T m = T(0);
  for (int k = tid; k < K; k += kThreads) m = fmax(m, A[(int64_t)k * K + k]);
  red[tid] = m;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  const T tol = T(K) * Num<T>::eps() * red[0];
  bool ok = !(counts && counts[it] < K);  // fewer samples than unknowns: singular whatever the rounding of the pivots
  for (int j = 0; ok && j < K; ++j) {  // right-looking Cholesky, lower triangle (`ok` is block-uniform)
    __syncthreads();
    const T d = A[(int64_t)j * K + j];
    if (!(d > tol)) {  // (block-uniform: every thread read the same value after the barrier; NaN fails too)
      ok = false;
      break;
    }
    const T ljj = sqrt(d), rinv = T(1) / ljj;
    for (int i = j + 1 + tid; i < K; i += kThreads) A[(int64_t)i * K + j] *= rinv;
    __syncthreads();
    if (tid == 0) A[(int64_t)j * K + j] = ljj;
    const int mrest = K - 1 - j;
    for (int64_t x = tid; x < (int64_t)mrest * mrest; x += kThreads) {
      const int ii = (int)(x / mrest), kk = (int)(x - (int64_t)ii * mrest);
      if (kk <= ii) {
        const int i = j + 1 + ii, k = j + 1 + kk;
        A[(int64_t)i * K + k] -= A[(int64_t)i * K + j] * A[(int64_t)k * K + j];
      }
    }
  }
  if (!ok) {
    if (tid == 0) status[it] = 0;
    __syncthreads();
    sum_parts<T>(K, Gp, hp, p0, p1, Gsum + it * KK, hsum + it * K);  // the fallback solves the summed system
    return;
  }
  for (int j = 0; j < K; ++j) {  // L v = h
    __syncthreads();
    const T v = z[j] / A[(int64_t)j * K + j];
    __syncthreads();
    if (tid == 0) z[j] = v;
    for (int i = j + 1 + tid; i < K; i += kThreads) z[i] -= A[(int64_t)i * K + j] * v;
  }
  for (int j = K - 1; j >= 0; --j) {  // L^T x = v
    __syncthreads();
    const T v = z[j] / A[(int64_t)j * K + j];
    __syncthreads();
    if (tid == 0) z[j] = v;
    for (int i = tid; i < j; i += kThreads) z[i] -= A[(int64_t)j * K + i] * v;
  }
  __syncthreads();
  for (int k = tid; k < K; k += kThreads) X[xo.at(it, k)] = z[k];
  if (tid == 0) status[it] = 1;
}

// x = V diag(lambda+) t for the flagged items (status 0): lambda = sigma^2 (ttr_eigh_trunc, TTR_EIG_RAW), lambda+ = 1 / lambda
// above K eps lambda_max and 0 at or below it; t = V^T h.
template <typename T>
__global__ void __launch_bounds__(kThreads) pinv_finish_kernel(int K, const T* __restrict__ V, const T* __restrict__ sigma,
                                                               const T* __restrict__ t, const int32_t* __restrict__ status,
                                                               T* __restrict__ X, XOut xo) {
  __shared__ T c[kMaxK];
  const int64_t it = blockIdx.x;
  if (status[it] != 0) return;
  const T* s = sigma + it * K;
  const T cut = T(K) * Num<T>::eps() * (s[0] * s[0]);
  for (int k = threadIdx.x; k < K; k += kThreads) {
    const T lam = s[k] * s[k];
    c[k] = lam > cut ? t[it * K + k] / lam : T(0);
  }
  __syncthreads();
  const T* Vi = V + it * (int64_t)K * K;
  for (int m = threadIdx.x; m < K; m += kThreads) {
    T acc = T(0);
    for (int k = 0; k < K; ++k) acc += Vi[(int64_t)m * K + k] * c[k];
    X[xo.at(it, m)] = acc;
  }
}

int64_t stage_rows(int dtype, int64_t r0, int64_t r1) {  // samples staged per pass of ttr_als_normal: a multiple of 4, <= 256
  const int64_t es = elem_size(dtype);
  int64_t S = kStageBytes / ((r0 + r1 + 1) * es + 8);
  S = S > 256 ? 256 : S;
  return S & ~(int64_t)3;
}

}  // namespace
}  // namespace ttr

using namespace ttr;

extern "C" int64_t ttr_als_normal_groups(int64_t r0, int64_t r1) {
  const int64_t nT = (r0 * r1 + 15) / 16;
  return ceil_div(nT * (nT + 1) / 2, kTilesPerGroup);
}

extern "C" int ttr_als_normal(int dtype, int64_t ntasks, int64_t r0, int64_t r1, const void* L, int64_t ldl, const void* R,
                              int64_t ldr, const void* w, const void* y, const void* perm, const void* task_begin,
                              const void* task_end, void* Gp, void* hp, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_als_normal: bad dtype %d", dtype);
  TTR_REQUIRE(ntasks >= 0 && r0 >= 1 && r1 >= 1 && ldl >= r0 && ldr >= r1, TTR_E_INVALID, "ttr_als_normal: bad sizes");
  TTR_REQUIRE(r0 * r1 <= kMaxK, TTR_E_UNSUPPORTED, "ttr_als_normal: r0 * r1 = %lld above %lld", (long long)(r0 * r1),
              (long long)kMaxK);
  TTR_REQUIRE(ntasks < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_als_normal: too many tasks");
  if (ntasks == 0) return TTR_OK;
  TTR_REQUIRE(L && R && y && perm && task_begin && task_end && Gp && hp, TTR_E_INVALID, "ttr_als_normal: NULL argument");
  const int64_t S = stage_rows(dtype, r0, r1);
  TTR_REQUIRE(S >= 4, TTR_E_UNSUPPORTED, "ttr_als_normal: ranks too large to stage");
  const int64_t es = elem_size(dtype);
  const size_t lds = (size_t)(S * (r0 + r1 + 1) * es + S * 8);
  const dim3 grid((unsigned)ntasks, (unsigned)ttr_als_normal_groups(r0, r1));
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(als_normal_kernel<T>, grid, dim3(kThreads), lds, s, (int)r0, (int)r1, (int)S, (const T*)L, ldl, (const T*)R, ldr,
                       (const T*)w, (const T*)y, (const int64_t*)perm, (const int64_t*)task_begin, (const int64_t*)task_end, (T*)Gp,
                       (T*)hp);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

template <typename T>
static int spd_solve_typed(int64_t n_items, int64_t K, const void* Gp, const void* hp, const void* part_off, int64_t part_base,
                           void* X, XOut xo, void* Gsum, void* hsum, void* status, const void* counts, hipStream_t s) {
  const size_t lds = (size_t)((K * K + K) * (int64_t)sizeof(T));
  if ((int64_t)lds <= kSolveLdsBytes)
    hipLaunchKernelGGL((spd_solve_kernel<T, true>), dim3((unsigned)n_items), dim3(kThreads), lds, s, (int)K, (const T*)Gp,
                       (const T*)hp, (const int64_t*)part_off, part_base, (T*)X, xo, (T*)Gsum, (T*)hsum, (int32_t*)status,
                       (const int64_t*)counts);
  else
    hipLaunchKernelGGL((spd_solve_kernel<T, false>), dim3((unsigned)n_items), dim3(kThreads), 0, s, (int)K, (const T*)Gp,
                       (const T*)hp, (const int64_t*)part_off, part_base, (T*)X, xo, (T*)Gsum, (T*)hsum, (int32_t*)status,
                       (const int64_t*)counts);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

extern "C" int ttr_spd_solve(int dtype, int64_t n_items, int64_t K, const void* Gp, const void* hp, const void* part_off,
                             int64_t part_base, void* X, int64_t inner, int64_t s_item, int64_t s_a, int64_t s_b, void* Gsum,
                             void* hsum, void* status, const void* counts, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_spd_solve: bad dtype %d", dtype);
  TTR_REQUIRE(n_items >= 0 && K >= 1 && inner >= 1, TTR_E_INVALID, "ttr_spd_solve: bad sizes");
  TTR_REQUIRE(K <= kMaxK, TTR_E_UNSUPPORTED, "ttr_spd_solve: K = %lld above %lld", (long long)K, (long long)kMaxK);
  TTR_REQUIRE(n_items < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_spd_solve: too many items");
  if (n_items == 0) return TTR_OK;
  TTR_REQUIRE(Gp && hp && part_off && X && Gsum && hsum && status, TTR_E_INVALID, "ttr_spd_solve: NULL argument");
  const XOut xo{inner, s_item, s_a, s_b};
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) {
    return spd_solve_typed<decltype(t)>(n_items, K, Gp, hp, part_off, part_base, X, xo, Gsum, hsum, status, counts, s);
  });
}

extern "C" int ttr_pinv_finish(int dtype, int64_t n_items, int64_t K, const void* V, const void* sigma, const void* t,
                               const void* status, void* X, int64_t inner, int64_t s_item, int64_t s_a, int64_t s_b,
                               void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_pinv_finish: bad dtype %d", dtype);
  TTR_REQUIRE(n_items >= 0 && K >= 1 && inner >= 1, TTR_E_INVALID, "ttr_pinv_finish: bad sizes");
  TTR_REQUIRE(K <= kMaxK, TTR_E_UNSUPPORTED, "ttr_pinv_finish: K = %lld above %lld", (long long)K, (long long)kMaxK);
  if (n_items == 0) return TTR_OK;
  TTR_REQUIRE(V && sigma && t && status && X, TTR_E_INVALID, "ttr_pinv_finish: NULL argument");
  const XOut xo{inner, s_item, s_a, s_b};
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(pinv_finish_kernel<T>, dim3((unsigned)n_items), dim3(kThreads), 0, s, (int)K, (const T*)V, (const T*)sigma,
                       (const T*)t, (const int32_t*)status, (T*)X, xo);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}
