// ttr_maxvol: maximum-volume row selection of tall matrices A [B, N, r] (maxvol.py:115-170, py_maxvol), for TT-cross.
//
//   index[b] = r rows of A[b] whose r x r submatrix has (locally) maximal |det|;  C[b] = A[b] A[b][index]^-1  [N, r]
//
// Steps, each one launch over row blocks of kRows rows (grid.y = batch item):
//   1. LU with partial pivoting of A (as getrf): launch k eliminates column k - 1 with the pivot chosen by launch k - 1 and
//      proposes the pivot of column k.  Row swaps are not performed: every row carries its LAPACK position pos[row] (a row
//      swap of getrf exchanges two positions), so the pivot of column k is the row of largest |W[row, k]| among rows at
//      positions >= k, ties to the smallest POSITION -- idamax's first index in the permuted order.  index = the rows at
//      positions 0 .. r-1.
//   2. C = A A_I^-1 solved fresh: A_I = A[index] is inverted in one workgroup (Gauss-Jordan with partial pivoting in LDS), the
//      product A X runs over the row blocks with a fixed FMA order (k = 0 .. r-1), so an item's result does not depend on the
//      batch it was computed in.
//   3. Swaps (Sherman-Morrison-Woodbury).  The reference keeps C transposed, (r, N), and takes
//      divmod(abs(C).argmax(), N): the FIRST maximum of |C^T| in row-major order.  Here C is [N, r]; the element C[n, q] has
//      the flat key q * N + n, and the pivot (n = p, q) is the largest |C| with ties to the SMALLEST key.  While
//      |C[p, q]| > tol and fewer than max_iters swaps were made: index[q] = p and
//          C[n, k] <- C[n, k] + (C[p, k] - delta_kq) * (-C[n, q] / C[p, q])      (dger of the reference, x = row p - e_q)
//      C is ping-ponged between two buffers: a launch reads one and writes the other, so no block overwrites the pivot row
//      another block still reads.  Each block leaves its argmax partial (|value|, key); every block of the next launch
//      reduces ALL partials in the same order, so all blocks agree on the pivot without atomics or fences, and checks the
//      stop condition: when it holds, block 0 records done / swap count and every block returns (as do all later launches).
//      The host enqueues max_iters + 1 swap launches and reads nothing back.  There is no cross-workgroup synchronisation but
//      the launch boundaries.
//   4. The final C is solved fresh from the final index as in step 2 (not the C carried through up to max_iters rank-1
//      updates).
//
// NaN values count as 0 in every argmax, so a pivot is always a valid row (nonsense in, nonsense out, never out of bounds).
#include "detail/ttr_internal.h"

namespace ttr {
namespace {

constexpr int kRows = 16;       // rows of C per block
constexpr int64_t kMaxR = 128;  // r x r inverse in LDS (fp64: 128 KB)

struct Part {  // argmax partial of one block
  double v;
  int64_t key;
};

__device__ __forceinline__ bool better(double v, int64_t key, double bv, int64_t bkey) {
  return v > bv || (v == bv && key < bkey);
}

template <typename T>
__device__ __forceinline__ double absval(T x) {
  double a = fabs((double)x);
  return a == a ? a : 0.0;  // NaN -> 0
}

// block-wide argmax of (v, key) -> result in every thread (uses sv / sk, kThreads entries)
__device__ __forceinline__ void block_argmax(double& v, int64_t& key, double* sv, int64_t* sk) {
  const int tid = threadIdx.x;
  sv[tid] = v;
  sk[tid] = key;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s && better(sv[tid + s], sk[tid + s], sv[tid], sk[tid])) {
      sv[tid] = sv[tid + s];
      sk[tid] = sk[tid + s];
    }
    __syncthreads();
  }
  v = sv[0];
  key = sk[0];
  __syncthreads();
}

// reduce the nblk partials of one item (same order in every block)
__device__ __forceinline__ void reduce_parts(const Part* parts, int64_t nblk, double& v, int64_t& key, double* sv, int64_t* sk) {
  v = -1.0;
  key = INT64_MAX;
  for (int64_t q = threadIdx.x; q < nblk; q += kThreads) {
    Part p = parts[q];
    if (better(p.v, p.key, v, key)) {
      v = p.v;
      key = p.key;
    }
  }
  block_argmax(v, key, sv, sk);
}

// LU launch k (0 <= k <= r): apply pivot k-1 (position bookkeeping, elimination of column k-1), propose pivot k, and at k == r
// write index[pos] = row for the r pivot rows.  W [N, r] is the working copy of A.
template <typename T>
__global__ void __launch_bounds__(kThreads) lu_kernel(const T* __restrict__ A, int64_t sa, T* __restrict__ W, int64_t N, int64_t r,
                                                      int64_t k, int64_t* __restrict__ pos, const Part* __restrict__ pin,
                                                      Part* __restrict__ pout, int64_t nblk, int64_t* __restrict__ index) {
  __shared__ double sv[kThreads];
  __shared__ int64_t sk[kThreads];
  __shared__ T prow_v[kMaxR];
  __shared__ T lrow[kRows];
  __shared__ int64_t spos[kRows];
  const int64_t b = blockIdx.y, row0 = (int64_t)blockIdx.x * kRows;
  const int tid = threadIdx.x;
  const T* Ab = A + b * sa;
  T* Wb = W + b * N * r;
  int64_t* posb = pos + b * N;
  const int nr = (int)min((int64_t)kRows, N - row0);
  double bv = -1.0;
  int64_t bkey = INT64_MAX;
  if (k == 0) {
    for (int e = tid; e < nr * r; e += kThreads) {
      const int i = e / (int)r, c = e % (int)r;
      const int64_t row = row0 + i;
      const T x = Ab[row * r + c];
      Wb[row * r + c] = x;
      if (c == 0 && better(absval(x), row * N + row, bv, bkey)) {
        bv = absval(x);
        bkey = row * N + row;
      }
    }
    if (tid < nr) posb[row0 + tid] = row0 + tid;
  } else {
    double pv;
    int64_t pkey;
    reduce_parts(pin + b * nblk, nblk, pv, pkey, sv, sk);
    const int64_t prow = pkey % N, ppos = pkey / N;
    if (tid < nr) {  // getrf's swap of positions k-1 and ppos, seen from each of this block's rows
      const int64_t row = row0 + tid;
      int64_t p = posb[row];
      if (row == prow)
        p = k - 1;
      else if (p == k - 1)
        p = ppos;
      posb[row] = p;
      spos[tid] = p;
    }
    for (int64_t c = k - 1 + tid; c < r; c += kThreads) prow_v[c] = Wb[prow * r + c];  // the pivot row is final: nobody writes it
    __syncthreads();
    if (k < r) {
      const T rpiv = T(1) / prow_v[k - 1];
      if (tid < nr) lrow[tid] = spos[tid] > k - 1 ? Wb[(row0 + tid) * r + (k - 1)] * rpiv : T(0);
      __syncthreads();
      const int w = (int)(r - k);
      for (int e = tid; e < nr * w; e += kThreads) {
        const int i = e / w;
        const int64_t c = k + e % w, row = row0 + i;
        if (spos[i] <= k - 1) continue;
        const T x = fma(-lrow[i], prow_v[c], Wb[row * r + c]);
        Wb[row * r + c] = x;
        if (c == k && better(absval(x), spos[i] * N + row, bv, bkey)) {
          bv = absval(x);
          bkey = spos[i] * N + row;
        }
      }
    } else if (tid < nr && spos[tid] < r) {
      index[b * r + spos[tid]] = row0 + tid;
    }
  }
  if (k < r) {
    block_argmax(bv, bkey, sv, sk);
    if (tid == 0) pout[b * nblk + blockIdx.x] = Part{bv, bkey};
  }
}

// X[b] = A[b][index[b]]^-1 (r x r), one workgroup per item: in-place Gauss-Jordan with partial pivoting in LDS
template <typename T>
__global__ void __launch_bounds__(kThreads) inverse_kernel(const T* __restrict__ A, int64_t sa, int64_t N, int64_t r,
                                                           const int64_t* __restrict__ index, T* __restrict__ X) {
  extern __shared__ __align__(16) unsigned char smem[];
  T* a = (T*)smem;  // [r][r]
  __shared__ T f[kMaxR];
  __shared__ int piv[kMaxR];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, R = (int)r;
  for (int e = tid; e < R * R; e += kThreads) {
    int64_t row = index[b * r + e / R];
    row = row < 0 ? 0 : (row >= N ? N - 1 : row);
    a[e] = A[b * sa + row * r + e % R];
  }
  __syncthreads();
  for (int k = 0; k < R; ++k) {
    if (tid < kWave) {  // pivot search in column k, first maximum
      double bv = -1.0;
      int bi = k;
      for (int i = k + tid; i < R; i += kWave) {
        const double v = absval(a[i * R + k]);
        if (v > bv) {
          bv = v;
          bi = i;
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      if (tid == 0) piv[k] = bi;
    }
    __syncthreads();
    const int p = piv[k];
    if (p != k)
      for (int c = tid; c < R; c += kThreads) {
        const T t = a[k * R + c];
        a[k * R + c] = a[p * R + c];
        a[p * R + c] = t;
      }
    __syncthreads();
    const T d = T(1) / a[k * R + k];
    __syncthreads();
    if (tid == 0) a[k * R + k] = T(1);
    __syncthreads();
    for (int c = tid; c < R; c += kThreads) a[k * R + c] *= d;
    for (int i = tid; i < R; i += kThreads) f[i] = a[i * R + k];
    __syncthreads();
    for (int e = tid; e < R * R; e += kThreads) {
      const int i = e / R, c = e % R;
      if (i == k) continue;
      const T base = c == k ? T(0) : a[e];
      a[e] = fma(-f[i], a[k * R + c], base);
    }
    __syncthreads();
  }
  for (int k = R - 1; k >= 0; --k) {
    const int p = piv[k];
    if (p != k)
      for (int i = tid; i < R; i += kThreads) {
        const T t = a[i * R + k];
        a[i * R + k] = a[i * R + p];
        a[i * R + p] = t;
      }
    __syncthreads();
  }
  for (int e = tid; e < R * R; e += kThreads) X[b * r * r + e] = a[e];
}

// C[b] = A[b] X[b] over row blocks (FMA order k = 0 .. r-1); with `pout`, also the argmax partials of |C| (key q * N + n)
template <typename T>
__global__ void __launch_bounds__(kThreads) product_kernel(const T* __restrict__ A, int64_t sa, const T* __restrict__ X, int64_t N,
                                                           int64_t r, T* __restrict__ C, int64_t sc, Part* __restrict__ pout,
                                                           int64_t nblk) {
  __shared__ double sv[kThreads];
  __shared__ int64_t sk[kThreads];
  const int64_t b = blockIdx.y, row0 = (int64_t)blockIdx.x * kRows;
  const int tid = threadIdx.x;
  const int nr = (int)min((int64_t)kRows, N - row0);
  const T* Xb = X + b * r * r;
  double bv = -1.0;
  int64_t bkey = INT64_MAX;
  for (int e = tid; e < nr * r; e += kThreads) {
    const int64_t row = row0 + e / (int)r, c = e % (int)r;
    const T* a = A + b * sa + row * r;
    T acc = T(0);
    for (int64_t k = 0; k < r; ++k) acc = fma(a[k], Xb[k * r + c], acc);
    C[b * sc + row * r + c] = acc;
    if (better(absval(acc), c * N + row, bv, bkey)) {
      bv = absval(acc);
      bkey = c * N + row;
    }
  }
  if (pout) {
    block_argmax(bv, bkey, sv, sk);
    if (tid == 0) pout[b * nblk + blockIdx.x] = Part{bv, bkey};
  }
}

// swap launch t (0 <= t <= max_iters): see the file comment, step 3.  status[b] = {done, swaps}.
template <typename T>
__global__ void __launch_bounds__(kThreads) swap_kernel(const T* __restrict__ Cin, T* __restrict__ Cout, int64_t N, int64_t r,
                                                        int64_t t, int64_t max_iters, double tol, const Part* __restrict__ pin,
                                                        Part* __restrict__ pout, int64_t nblk, int32_t* status,
                                                        int64_t* __restrict__ index) {
  __shared__ double sv[kThreads];
  __shared__ int64_t sk[kThreads];
  __shared__ T xrow[kMaxR];
  __shared__ T tmp[kRows];
  const int64_t b = blockIdx.y, row0 = (int64_t)blockIdx.x * kRows;
  const int tid = threadIdx.x;
  if (status[2 * b]) return;
  double pv;
  int64_t pkey;
  reduce_parts(pin + b * nblk, nblk, pv, pkey, sv, sk);
  if (!(pv > tol) || t >= max_iters) {
    if (blockIdx.x == 0 && tid == 0) {
      status[2 * b] = 1;
      status[2 * b + 1] = (int32_t)t;
    }
    return;
  }
  const int64_t q = pkey / N, p = pkey % N;
  const T* Cb = Cin + b * N * r;
  T* Ob = Cout + b * N * r;
  for (int64_t c = tid; c < r; c += kThreads) xrow[c] = Cb[p * r + c] - (c == q ? T(1) : T(0));
  const T alpha = T(-1) / Cb[p * r + q];
  const int nr = (int)min((int64_t)kRows, N - row0);
  if (tid < nr) tmp[tid] = alpha * Cb[(row0 + tid) * r + q];
  __syncthreads();
  double bv = -1.0;
  int64_t bkey = INT64_MAX;
  for (int e = tid; e < nr * r; e += kThreads) {
    const int i = e / (int)r;
    const int64_t c = e % (int)r, row = row0 + i;
    const T x = fma(xrow[c], tmp[i], Cb[row * r + c]);
    Ob[row * r + c] = x;
    if (better(absval(x), c * N + row, bv, bkey)) {
      bv = absval(x);
      bkey = c * N + row;
    }
  }
  block_argmax(bv, bkey, sv, sk);
  if (tid == 0) pout[b * nblk + blockIdx.x] = Part{bv, bkey};
  if (blockIdx.x == 0 && tid == 0) index[b * r + q] = p;
}

struct Layout {
  int64_t c0, c1, x, pos, parts, status, total;
};

Layout layout(int64_t esize, int64_t N, int64_t r, int64_t batch) {
  const int64_t nblk = (N + kRows - 1) / kRows;
  Layout L{};
  int64_t o = 0;
  L.c0 = o; o += align256(batch * N * r * esize);
  L.c1 = o; o += align256(batch * N * r * esize);
  L.x = o; o += align256(batch * r * r * esize);
  L.pos = o; o += align256(batch * N * 8);
  L.parts = o; o += align256(2 * batch * nblk * (int64_t)sizeof(Part));
  L.status = o; o += align256(batch * 2 * 4);
  L.total = o;
  return L;
}

template <typename T>
int maxvol_impl(int64_t batch, int64_t N, int64_t r, const T* A, int64_t sa, double tol, int64_t max_iters, int64_t* index, T* C,
                int64_t sc, int32_t* status, char* ws, const Layout& L, hipStream_t stream) {
  const int64_t nblk = (N + kRows - 1) / kRows;
  T* C0 = (T*)(ws + L.c0);
  T* C1 = (T*)(ws + L.c1);
  T* X = (T*)(ws + L.x);
  int64_t* pos = (int64_t*)(ws + L.pos);
  Part* parts[2] = {(Part*)(ws + L.parts), (Part*)(ws + L.parts) + batch * nblk};
  if (!status) status = (int32_t*)(ws + L.status);
  TTR_HIP_CHECK(hipMemsetAsync(status, 0, batch * 2 * sizeof(int32_t), stream));
  const dim3 grid((unsigned)nblk, (unsigned)batch);
  // 1. LU pivots (W = C1)
  for (int64_t k = 0; k <= r; ++k)
    hipLaunchKernelGGL(lu_kernel<T>, grid, dim3(kThreads), 0, stream, A, sa, C1, N, r, k, pos, parts[(k + 1) % 2], parts[k % 2],
                       nblk, index);
  // 2. C = A A_I^-1 into C0, partials into parts[0]
  const size_t lds = (size_t)(r * r * sizeof(T));
  // static LDS (pivots, multipliers) comes on top: set the dynamic size always
  TTR_HIP_CHECK(hipFuncSetAttribute((const void*)inverse_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(inverse_kernel<T>, dim3((unsigned)batch), dim3(kThreads), lds, stream, A, sa, N, r, index, X);
  hipLaunchKernelGGL(product_kernel<T>, grid, dim3(kThreads), 0, stream, A, sa, X, N, r, C0, N * r, parts[0], nblk);
  // 3. swaps: launch t reads C[t % 2] and parts[t % 2]
  for (int64_t t = 0; t <= max_iters; ++t) {
    T* cin = t % 2 == 0 ? C0 : C1;
    T* cout = t % 2 == 0 ? C1 : C0;
    hipLaunchKernelGGL(swap_kernel<T>, grid, dim3(kThreads), 0, stream, cin, cout, N, r, t, max_iters, tol, parts[t % 2],
                       parts[(t + 1) % 2], nblk, status, index);
  }
  // 4. fresh C from the final index
  hipLaunchKernelGGL(inverse_kernel<T>, dim3((unsigned)batch), dim3(kThreads), lds, stream, A, sa, N, r, index, X);
  hipLaunchKernelGGL(product_kernel<T>, grid, dim3(kThreads), 0, stream, A, sa, X, N, r, C, sc, (Part*)nullptr, nblk);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace
}  // namespace ttr

using namespace ttr;

extern "C" int64_t ttr_maxvol_workspace_bytes(int dtype, int64_t N, int64_t r, int64_t batch) {
  if (!dtype_ok(dtype) || N < 1 || r < 1 || batch < 1) return -1;
  return layout(elem_size(dtype), N, r, batch).total;
}

extern "C" int ttr_maxvol(int dtype, int64_t batch, int64_t N, int64_t r, const void* A, int64_t stride_ab, double tol,
                          int64_t max_iters, void* index, void* C, int64_t stride_cb, void* status, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_maxvol: bad dtype %d", dtype);
  TTR_REQUIRE(batch >= 1 && r >= 1 && N > r, TTR_E_INVALID, "ttr_maxvol: bad sizes (batch %lld, N %lld, r %lld; needs N > r)",
              (long long)batch, (long long)N, (long long)r);
  TTR_REQUIRE(max_iters >= 0, TTR_E_INVALID, "ttr_maxvol: max_iters %lld < 0", (long long)max_iters);
  TTR_REQUIRE(A && index && C, TTR_E_INVALID, "ttr_maxvol: NULL argument");
  TTR_REQUIRE(stride_ab >= N * r && stride_cb >= N * r, TTR_E_INVALID, "ttr_maxvol: batch strides below N * r");
  TTR_REQUIRE(r <= kMaxR, TTR_E_UNSUPPORTED, "ttr_maxvol: r %lld above %lld", (long long)r, (long long)kMaxR);
  TTR_REQUIRE(batch <= 65535, TTR_E_UNSUPPORTED, "ttr_maxvol: batch %lld above 65535", (long long)batch);
  TTR_REQUIRE(N < ((int64_t)1 << 31) / kMaxR, TTR_E_UNSUPPORTED, "ttr_maxvol: N %lld too large", (long long)N);
  const Layout L = layout(elem_size(dtype), N, r, batch);
  TTR_REQUIRE(workspace && workspace_bytes >= L.total, TTR_E_WORKSPACE, "ttr_maxvol: workspace %lld < %lld bytes",
              (long long)workspace_bytes, (long long)L.total);
  hipStream_t s = (hipStream_t)stream;
  if (tol < 1.0) tol = 1.0;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return maxvol_impl<T>(batch, N, r, (const T*)A, stride_ab, tol, max_iters, (int64_t*)index, (T*)C, stride_cb, (int32_t*)status,
                          (char*)workspace, L, s);
  });
}
