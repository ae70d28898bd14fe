// One Rayleigh-Ritz step of the three-vector LOBPCG behind tt_eigsh (tteigs.py) in two launches on the six
// vectors X, AX, W, AW, P, AP of n elements, and their extern "C" entries (profiling kind misc).  Both are streaming kernels
// with 256-thread blocks, HBM- or launch-bound.
//   ttr_ritz_gram     part[g][0..12) = workgroup g's share of S = V^T V and T = V^T A V, V = [X W P], in double: upper triangles,
//                     S (xx, xw, xp, ww, wp, pp) then T (x.ax, x.aw, x.ap, w.aw, w.ap, p.ap).  One pass, 16-byte packs.
//   ttr_ritz_update   every workgroup adds the partials in increasing g (the launch-boundary reduce: the sum of a launch finished in
//                     the next launch's prologue), one thread solves the 3 x 3 pencil (T, S) in double, and the workgroup updates
//                     its slice of the vectors in place; workgroup 0 writes `state` and accumulates `sweep`.
// Summation order.  Pack p (elements p V .. p V + V - 1, V = 16 bytes / sizeof(T)) belongs to thread p % 256 of workgroup
// (p / 256) % parts, which adds its packs in increasing p and a pack's elements in increasing index, one fma per product; the 64
// lanes of a wave meet in wave_sum, the four waves and then the workgroups in increasing order.  `parts` is a function of n and the
// dtype (ritz_parts), so every sum is one fixed expression of n and the dtype: aligned or not, the bits are the same.
// The scalar path (a pointer off a 16-byte boundary, and the last pack of an n that is no multiple of V) loads the same elements
// one by one into the same pack registers; past n they are zeros, which add nothing.
// Every index is bounded by n; `part` is bounded by workspace_bytes (checked on the host); state and sweep are 8 and 4 doubles.
// No atomics, no cooperative launch: the two launches are ordered by the stream.
#include "detail/ttr_internal.h"
#include "detail/ttr_pack_io.h"

namespace ttr {

constexpr int kRitzSums = 12;
constexpr int kRitzPacksPerThread = 4;   // a further workgroup joins per 256 * 4 packs (4096 fp32 / 2048 fp64 elements)

inline int ritz_parts(int dtype, int64_t n) {
  const int64_t V = 16 / elem_size(dtype);
  const int64_t g = ceil_div(ceil_div(n, V), (int64_t)kThreads * kRitzPacksPerThread);
  return (int)(g < 1 ? 1 : (g > TTR_RITZ_MAX_PARTS ? TTR_RITZ_MAX_PARTS : g));
}

// KIND 0: TTR_RITZ_INIT (X, AX only); 1: a step whose P is zero (P, AP not read); 2: a step
template <typename T, bool WIDE, int KIND>
__global__ __launch_bounds__(kThreads) void ritz_gram_kernel(int64_t n, const T* __restrict__ X, const T* __restrict__ AX,
                                                             const T* __restrict__ W, const T* __restrict__ AW,
                                                             const T* __restrict__ P, const T* __restrict__ AP,
                                                             double* __restrict__ part) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ double red[kThreads / kWave][kRitzSums];
  double acc[kRitzSums];
#pragma unroll
  for (int j = 0; j < kRitzSums; ++j) acc[j] = 0.0;
  const int64_t npacks = (n + V - 1) / V;
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < npacks; p += (int64_t)gridDim.x * kThreads) {
    const int64_t base = p * V;
    const Pack<T, V> x = pack_load<T, V, WIDE>(X, base, n), ax = pack_load<T, V, WIDE>(AX, base, n);
    Pack<T, V> w, aw, pp, ap;
    if (KIND >= 1) {
      w = pack_load<T, V, WIDE>(W, base, n);
      aw = pack_load<T, V, WIDE>(AW, base, n);
    }
    if (KIND == 2) {
      pp = pack_load<T, V, WIDE>(P, base, n);
      ap = pack_load<T, V, WIDE>(AP, base, n);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const double xd = (double)x.v[v], axd = (double)ax.v[v];
      acc[0] = fma(xd, xd, acc[0]);
      acc[6] = fma(xd, axd, acc[6]);
      if (KIND >= 1) {
        const double wd = (double)w.v[v], awd = (double)aw.v[v];
        acc[1] = fma(xd, wd, acc[1]);
        acc[3] = fma(wd, wd, acc[3]);
        acc[7] = fma(xd, awd, acc[7]);
        acc[9] = fma(wd, awd, acc[9]);
        if (KIND == 2) {
          const double pd = (double)pp.v[v], apd = (double)ap.v[v];
          acc[2] = fma(xd, pd, acc[2]);
          acc[4] = fma(wd, pd, acc[4]);
          acc[5] = fma(pd, pd, acc[5]);
          acc[8] = fma(xd, apd, acc[8]);
          acc[10] = fma(wd, apd, acc[10]);
          acc[11] = fma(pd, apd, acc[11]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kRitzSums; ++j) {
    const double s = wave_sum(acc[j]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < kRitzSums) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < kThreads / kWave; ++w) s += red[w][threadIdx.x];
    part[(int64_t)blockIdx.x * kRitzSums + threadIdx.x] = s;
  }
}

// ------------------------------------------------------------------ the 3 x 3 pencil, one thread, double
// One Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q); r is the third index.  v?p / v?q: columns p and q of the
// eigenvector matrix.  A zero a_pq rotates nothing, so a row and column of zeros stays out of every rotation.
__device__ __forceinline__ void ritz_rot(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p, double& v0q,
                                         double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double tau = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));   // (tau^2 = inf: t = 0, the identity)
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  double r = apr;
  apr = c * r - s * aqr;
  aqr = s * r + c * aqr;
  r = v0p, v0p = c * r - s * v0q, v0q = s * r + c * v0q;
  r = v1p, v1p = c * r - s * v1q, v1q = s * r + c * v1q;
  r = v2p, v2p = c * r - s * v2q, v2q = s * r + c * v2q;
}

// Cyclic Jacobi: on exit a[0], a[3], a[5] (the diagonal of the upper triangle 00 01 02 11 12 22) are the eigenvalues and column j
// of v (row-major 3 x 3) the eigenvector of the j-th.  Converges quadratically; the sweep count is bounded.
__device__ __forceinline__ void ritz_jacobi3(double (&a)[6], double (&v)[9]) {
  v[0] = v[4] = v[8] = 1.0;
  v[1] = v[2] = v[3] = v[5] = v[6] = v[7] = 0.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = fabs(a[1]) + fabs(a[2]) + fabs(a[4]);
    if (off <= 1e-20 * (fabs(a[0]) + fabs(a[3]) + fabs(a[5]))) break;
    ritz_rot(a[0], a[3], a[1], a[2], a[4], v[0], v[1], v[3], v[4], v[6], v[7]);   // (0, 1), r = 2
    ritz_rot(a[0], a[5], a[2], a[1], a[4], v[0], v[2], v[3], v[5], v[6], v[8]);   // (0, 2), r = 1
    ritz_rot(a[3], a[5], a[4], a[1], a[2], v[1], v[2], v[4], v[5], v[7], v[8]);   // (1, 2), r = 0
  }
}

// The extreme Ritz pair of (T, S) (upper triangles g[6..12), g[0..6)): S is scaled to unit diagonal (a zero diagonal drops the
// direction), the eigendirections of the scaled S below TTR_RITZ_DROP eps of its largest eigenvalue are dropped, the whitened
// problem is solved.  c is scaled to c^T S c = 1 with c[0] >= 0, theta = c^T T c.  Returns the number of directions kept.
// (the host mirror: _hostops.ritz_pencil)
__device__ __forceinline__ int ritz_pencil(const double* g, int which, double eps, double (&c)[3], double& theta) {
  const double S[6] = {g[0], g[1], g[2], g[3], g[4], g[5]}, Tm[6] = {g[6], g[7], g[8], g[9], g[10], g[11]};
  const double i0 = S[0] > 0.0 ? 1.0 / sqrt(S[0]) : 0.0, i1 = S[3] > 0.0 ? 1.0 / sqrt(S[3]) : 0.0, i2 = S[5] > 0.0 ? 1.0 / sqrt(S[5]) : 0.0;
  double a[6] = {S[0] > 0.0 ? 1.0 : 0.0, S[1] * i0 * i1, S[2] * i0 * i2, S[3] > 0.0 ? 1.0 : 0.0, S[4] * i1 * i2, S[5] > 0.0 ? 1.0 : 0.0};
  double q[9];
  ritz_jacobi3(a, q);
  const double thr = (double)TTR_RITZ_DROP * eps * fmax(a[0], fmax(a[3], a[5]));
  const bool k0 = a[0] > thr, k1 = a[3] > thr, k2 = a[5] > thr;
  const double w0 = k0 ? 1.0 / sqrt(a[0]) : 0.0, w1 = k1 ? 1.0 / sqrt(a[3]) : 0.0, w2 = k2 ? 1.0 / sqrt(a[5]) : 0.0;
  // Z = Q diag(w), rows i, columns j
  const double z[9] = {q[0] * w0, q[1] * w1, q[2] * w2, q[3] * w0, q[4] * w1, q[5] * w2, q[6] * w0, q[7] * w1, q[8] * w2};
  const double t00 = Tm[0] * i0 * i0, t01 = Tm[1] * i0 * i1, t02 = Tm[2] * i0 * i2, t11 = Tm[3] * i1 * i1, t12 = Tm[4] * i1 * i2,
               t22 = Tm[5] * i2 * i2;
  // U = Ts Z, M = Z^T U
  double u[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    u[0 + j] = t00 * z[0 + j] + t01 * z[3 + j] + t02 * z[6 + j];
    u[3 + j] = t01 * z[0 + j] + t11 * z[3 + j] + t12 * z[6 + j];
    u[6 + j] = t02 * z[0 + j] + t12 * z[3 + j] + t22 * z[6 + j];
  }
  double m[9];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) m[3 * j + k] = z[0 + j] * u[0 + k] + z[3 + j] * u[3 + k] + z[6 + j] * u[6 + k];
  const double sg = which == TTR_RITZ_LA ? -1.0 : 1.0;    // the largest of M is the smallest of -M
  double b[6] = {sg * m[0], sg * 0.5 * (m[1] + m[3]), sg * 0.5 * (m[2] + m[6]), sg * m[4], sg * 0.5 * (m[5] + m[7]), sg * m[8]};
  const double big = 2.0 * (fabs(b[0]) + fabs(b[3]) + fabs(b[5]) + 2.0 * (fabs(b[1]) + fabs(b[2]) + fabs(b[4])) + 1.0);
  if (!k0) b[0] += big;   // a dropped direction: never the smallest
  if (!k1) b[3] += big;
  if (!k2) b[5] += big;
  double y[9];
  ritz_jacobi3(b, y);
  int js = 0;
  double lam = b[0];
  if (b[3] < lam) js = 1, lam = b[3];
  if (b[5] < lam) js = 2, lam = b[5];
  const double y0 = js == 0 ? y[0] : (js == 1 ? y[1] : y[2]), y1 = js == 0 ? y[3] : (js == 1 ? y[4] : y[5]),
               y2 = js == 0 ? y[6] : (js == 1 ? y[7] : y[8]);
  double c0 = i0 * (z[0] * y0 + z[1] * y1 + z[2] * y2), c1 = i1 * (z[3] * y0 + z[4] * y1 + z[5] * y2),
         c2 = i2 * (z[6] * y0 + z[7] * y1 + z[8] * y2);
  const double nrm2 = c0 * (S[0] * c0 + S[1] * c1 + S[2] * c2) + c1 * (S[1] * c0 + S[3] * c1 + S[4] * c2) +
                      c2 * (S[2] * c0 + S[4] * c1 + S[5] * c2);
  double sc = 1.0 / sqrt(nrm2);
  if (c0 < 0.0) sc = -sc;
  c0 *= sc, c1 *= sc, c2 *= sc;
  theta = c0 * (Tm[0] * c0 + Tm[1] * c1 + Tm[2] * c2) + c1 * (Tm[1] * c0 + Tm[3] * c1 + Tm[4] * c2) +
          c2 * (Tm[2] * c0 + Tm[4] * c1 + Tm[5] * c2);
  c[0] = c0, c[1] = c1, c[2] = c2;
  return (int)k0 + (int)k1 + (int)k2;
}

// HASP: P and AP are there (read and written); otherwise they count as zeros and are not touched
template <typename T, bool WIDE, bool HASP>
__global__ __launch_bounds__(kThreads) void ritz_update_kernel(int mode, int which, int first, int64_t n, double rel, int nparts,
                                                               const double* __restrict__ part, T* __restrict__ X,
                                                               T* __restrict__ AX, T* __restrict__ W, const T* __restrict__ AW,
                                                               T* __restrict__ P, T* __restrict__ AP, double* __restrict__ state,
                                                               double* __restrict__ sweep) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ double stage[TTR_RITZ_MAX_PARTS * kRitzSums];
  __shared__ double g[kRitzSums];
  __shared__ double coef[5];   // c0, c1, c2, theta', 1 when the vectors are written
  for (int i = threadIdx.x; i < nparts * kRitzSums; i += kThreads) stage[i] = part[i];
  __syncthreads();
  if (threadIdx.x < kRitzSums) {
    double s = stage[threadIdx.x];
    for (int r = 1; r < nparts; ++r) s += stage[r * kRitzSums + threadIdx.x];
    g[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    bool finite = true;
    for (int j = 0; j < kRitzSums; ++j) finite = finite && isfinite(g[j]);
    const int flags = finite ? (g[0] == 0.0 ? 2 : 0) : 1;
    double c[3] = {1.0, 0.0, 0.0}, theta = 0.0, res = 0.0;
    int frozen = 0, kept = 0;
    if (flags == 0) {
      if (mode == TTR_RITZ_INIT) {
        c[0] = 1.0 / sqrt(g[0]);
        theta = g[6] / g[0];
        kept = 1;
      } else {
        theta = g[6] / g[0];
        res = g[3] > 0.0 ? sqrt(g[3] / (g[3] + theta * theta * g[0])) : 0.0;
        frozen = res <= rel ? 1 : 0;
        if (!frozen) kept = ritz_pencil(g, which, (double)Num<T>::eps(), c, theta);
      }
    }
    coef[0] = c[0], coef[1] = c[1], coef[2] = c[2], coef[3] = theta;
    coef[4] = (flags == 0 && !frozen) ? 1.0 : 0.0;
    if (blockIdx.x == 0) {
      state[0] = theta, state[1] = res, state[2] = (double)frozen, state[3] = (double)flags;
      state[4] = c[0], state[5] = c[1], state[6] = c[2], state[7] = (double)kept;
      if (first) sweep[0] = fmax(sweep[0], res);
      if (flags != 0) sweep[1] += 1.0;
      sweep[2] = theta;
      sweep[3] = (double)((int)sweep[3] | flags);
    }
  }
  __syncthreads();
  if (coef[4] == 0.0) return;
  const double c0 = coef[0], c1 = coef[1], c2 = coef[2], theta = coef[3];
  const int64_t npacks = (n + V - 1) / V;
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < npacks; p += (int64_t)gridDim.x * kThreads) {
    const int64_t base = p * V;
    Pack<T, V> x = pack_load<T, V, WIDE>(X, base, n), ax = pack_load<T, V, WIDE>(AX, base, n);
    Pack<T, V> w, pn, apn;
    if (mode == TTR_RITZ_INIT) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        x.v[v] = (T)(c0 * (double)x.v[v]);
        ax.v[v] = (T)(c0 * (double)ax.v[v]);
        w.v[v] = (T)fma(-theta, (double)x.v[v], (double)ax.v[v]);
        pn.v[v] = T(0);
      }
      apn = pn;
    } else {
      const Pack<T, V> w0 = pack_load<T, V, WIDE>(W, base, n), aw = pack_load<T, V, WIDE>(AW, base, n);
      Pack<T, V> p0, ap0;
      if (HASP) {
        p0 = pack_load<T, V, WIDE>(P, base, n);
        ap0 = pack_load<T, V, WIDE>(AP, base, n);
      }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        double pd = c1 * (double)w0.v[v], apd = c1 * (double)aw.v[v];
        if (HASP) {
          pd = fma(c2, (double)p0.v[v], pd);
          apd = fma(c2, (double)ap0.v[v], apd);
        }
        x.v[v] = (T)fma(c0, (double)x.v[v], pd);
        ax.v[v] = (T)fma(c0, (double)ax.v[v], apd);
        pn.v[v] = (T)pd;
        apn.v[v] = (T)apd;
        w.v[v] = (T)fma(-theta, (double)x.v[v], (double)ax.v[v]);   // of the ROUNDED X and AX: the residual of what is stored
      }
    }
    pack_store<T, V, WIDE>(X, base, n, x);
    pack_store<T, V, WIDE>(AX, base, n, ax);
    pack_store<T, V, WIDE>(W, base, n, w);
    if (HASP) {
      pack_store<T, V, WIDE>(P, base, n, pn);
      pack_store<T, V, WIDE>(AP, base, n, apn);
    }
  }
}

}  // namespace ttr

using namespace ttr;

extern "C" {

int ttr_ritz_parts(int dtype, int64_t n) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_ritz_parts: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 1, TTR_E_INVALID, "ttr_ritz_parts: n = %lld < 1", (long long)n);
  return ritz_parts(dtype, n);
}

int64_t ttr_ritz_workspace_bytes(int dtype, int64_t n) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_ritz_workspace_bytes: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 1, TTR_E_INVALID, "ttr_ritz_workspace_bytes: n = %lld < 1", (long long)n);
  return (int64_t)ritz_parts(dtype, n) * kRitzSums * (int64_t)sizeof(double);
}

int ttr_ritz_gram(int dtype, int mode, int64_t n, const void* X, const void* AX, const void* W, const void* AW, const void* P,
                  const void* AP, double* part, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_ritz_gram: bad dtype %d", dtype);
  TTR_REQUIRE(mode == TTR_RITZ_INIT || mode == TTR_RITZ_STEP, TTR_E_INVALID, "ttr_ritz_gram: bad mode %d", mode);
  TTR_REQUIRE(n >= 1, TTR_E_INVALID, "ttr_ritz_gram: n = %lld < 1", (long long)n);
  TTR_REQUIRE(n < (int64_t(1) << 57), TTR_E_UNSUPPORTED, "ttr_ritz_gram: vectors too long");
  TTR_REQUIRE(X && AX && part && (mode == TTR_RITZ_INIT || (W && AW)) && ((P == nullptr) == (AP == nullptr)), TTR_E_INVALID,
              "ttr_ritz_gram: null pointer");
  const int parts = ritz_parts(dtype, n);
  TTR_REQUIRE(workspace_bytes >= (int64_t)parts * kRitzSums * (int64_t)sizeof(double), TTR_E_WORKSPACE,
              "ttr_ritz_gram: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
              (long long)((int64_t)parts * kRitzSums * (int64_t)sizeof(double)));
  const int kind = mode == TTR_RITZ_INIT ? 0 : (P ? 2 : 1);
  const bool wide = aligned16(X) && aligned16(AX) && (kind < 1 || (aligned16(W) && aligned16(AW))) &&
                    (kind < 2 || (aligned16(P) && aligned16(AP)));
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)parts), dim3(kThreads), 0, s, n, (const T*)X, (const T*)AX, (const T*)W, (const T*)AW,
                         (const T*)P, (const T*)AP, part);
    };
    if (wide) {
      if (kind == 0) launch(ritz_gram_kernel<T, true, 0>);
      else if (kind == 1) launch(ritz_gram_kernel<T, true, 1>);
      else launch(ritz_gram_kernel<T, true, 2>);
    } else {
      if (kind == 0) launch(ritz_gram_kernel<T, false, 0>);
      else if (kind == 1) launch(ritz_gram_kernel<T, false, 1>);
      else launch(ritz_gram_kernel<T, false, 2>);
    }
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_ritz_update(int dtype, int mode, int which, int first, int64_t n, double rel, const double* part, void* X, void* AX, void* W,
                    const void* AW, void* P, void* AP, double* state, double* sweep, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_ritz_update: bad dtype %d", dtype);
  TTR_REQUIRE(mode == TTR_RITZ_INIT || mode == TTR_RITZ_STEP, TTR_E_INVALID, "ttr_ritz_update: bad mode %d", mode);
  TTR_REQUIRE(which == TTR_RITZ_SA || which == TTR_RITZ_LA, TTR_E_INVALID, "ttr_ritz_update: bad which %d", which);
  TTR_REQUIRE(n >= 1, TTR_E_INVALID, "ttr_ritz_update: n = %lld < 1", (long long)n);
  TTR_REQUIRE(n < (int64_t(1) << 57), TTR_E_UNSUPPORTED, "ttr_ritz_update: vectors too long");
  TTR_REQUIRE(rel >= 0.0, TTR_E_INVALID, "ttr_ritz_update: rel must not be negative");
  TTR_REQUIRE(part && X && AX && W && state && sweep && (mode == TTR_RITZ_INIT || AW) && ((P == nullptr) == (AP == nullptr)),
              TTR_E_INVALID, "ttr_ritz_update: null pointer");
  const int parts = ritz_parts(dtype, n);
  const bool wide = aligned16(X) && aligned16(AX) && aligned16(W) && (mode == TTR_RITZ_INIT || aligned16(AW)) &&
                    (!P || (aligned16(P) && aligned16(AP)));
  const int64_t V = 16 / elem_size(dtype);
  int64_t grid = ceil_div(ceil_div(n, V), (int64_t)kThreads * 2);
  if (grid > 2048) grid = 2048;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, mode, which, first, n, rel, parts, part, (T*)X, (T*)AX, (T*)W,
                         (const T*)AW, (T*)P, (T*)AP, state, sweep);
    };
    if (wide) {
      if (P) launch(ritz_update_kernel<T, true, true>);
      else launch(ritz_update_kernel<T, true, false>);
    } else {
      if (P) launch(ritz_update_kernel<T, false, true>);
      else launch(ritz_update_kernel<T, false, false>);
    }
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // extern "C"
