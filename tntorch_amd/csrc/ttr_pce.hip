// Sparse polynomial-chaos regression (interpolation.py:347-630 `PCEInterpolator`): the design matrix of a tensor-product
// polynomial basis and its product with a coefficient vector, streaming kernels for gfx950:
//   ttr_pce_design   M[p, c] = prod_n B(p, n, coords[c, n])
//   ttr_pce_predict  y[p]    = sum_c coef[c] prod_n B(p, n, coords[c, n])
// with the basis value B(p, n, s) = sum_k Z[p, n]^k Psi[n, k, s] (Horner, from k = S - 1 down).
//
// Both kernels first evaluate the N S basis values of a TILE of points into LDS, once: Psi is staged in LDS in chunks of whole
// modes (at most kPsiElems values), item (point, n, s) -> one thread, consecutive threads consecutive points, so that the Psi
// reads of a wave are one address.  The coordinate table is staged in LDS in tiles, every entry checked against [0, S) as it
// is staged and kept as one byte (kBad for an entry outside: that candidate's product is 0 and `flag` gets bit 0) -- no address
// is ever formed from an unchecked coordinate.
//
// design: lane = candidate.  The tile of TP <= 64 points is stored point-major, a point's N S values contiguous (rows padded to
// an odd length: the evaluation writes down a column).  A wave reads the coordinates of its 64 candidates as 64 consecutive
// bytes of the mode-major tile [n][TC] (TC = 256 candidates; 128 or 64 where C or the coordinate bytes of N modes allow no
// more: the waves a narrower tile frees take other points of the tile) and gathers B at a wave-uniform (point, n): S <= 16 consecutive doubles, distinct banks.
// Four points per thread are in flight.  The store of a wave is 64 consecutive c of one row of M: coalesced along c.  The
// workgroups of one point tile (gridDim.y of them, where the point tiles alone would not fill the device) take every
// gridDim.y-th candidate tile.
//
// predict: lane = point.  The tile of PB <= 256 points (as many as kBasisElems allows; a whole number of waves where that is 64
// or more) is stored value-major, [n S + s][PB].  The coordinates (candidate-major tile [TC][N]) and the coefficient of a candidate
// are wave-uniform LDS reads, the gather of B at a wave-uniform (n, s) is 64 consecutive doubles.  A thread adds the terms of
// its point in increasing c.
//
// All arithmetic is in fp64 registers for both dtypes, rounded once at the store.  No atomics (the flag is a plain store of
// old | 1: every writer writes the same bit), no workgroup talks to another, no scratch: tiles and with them the order of
// every product and sum follow from (P, N, S, C) and the dtype alone.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int kMaxOrder = 16;       // S: a gather over s touches 16 doubles = 32 distinct banks
constexpr int kMaxBasis = 256;      // N S
constexpr int kBasisElems = 4096;   // doubles of basis values per workgroup (32 KB)
constexpr int kPsiElems = 1024;     // doubles of Psi staged at once: 4 modes at S = 16
constexpr int kDesignCoordBytes = 16384;
constexpr int kPredictCoordBytes = 8192;
constexpr int kPredictMaxTile = 1024;   // candidates per tile of ttr_pce_predict (their coefficients: 8 KB)
constexpr int64_t kFillBlocks = 1024;   // design: split the candidate tiles over gridDim.y while there are fewer workgroups
constexpr unsigned char kBad = 255;

template <typename T>
struct PceArgs {
  int64_t P, C;
  int N, S;
  const T* Z;
  int64_t sz0, sz1;
  const T* Psi;
  const int64_t* coords;
  const T* coef;   // predict
  T* out;          // M resp. y
  int64_t ldm;     // design
  int* flag;
  int tp;          // points per tile
  int row;         // design: doubles per point row (N S padded to odd)
  int tc;          // candidates per tile
  int nm;          // modes of Psi staged at once
};

// The basis values of the np points from p0 on: B[pt * sp + (n S + s) * sj].  Every thread of the workgroup takes part.
template <typename T>
__device__ __forceinline__ void eval_basis(const PceArgs<T>& a, double* __restrict__ psi, double* __restrict__ B, int64_t p0, int np,
                                           int sp, int sj) {
  const int S = a.S, SS = a.S * a.S, nt = blockDim.x, t = threadIdx.x;
  for (int n0 = 0; n0 < a.N; n0 += a.nm) {
    const int nm = a.N - n0 < a.nm ? a.N - n0 : a.nm;
    __syncthreads();   // (the readers of the chunk before)
    for (int i = t; i < nm * SS; i += nt) psi[i] = (double)a.Psi[(int64_t)n0 * SS + i];
    __syncthreads();
    for (int it = t; it < nm * S * a.tp; it += nt) {
      const int js = it / a.tp, pt = it - js * a.tp;
      if (pt >= np) continue;
      const int nl = js / S, s = js - nl * S;
      const double z = (double)a.Z[(p0 + pt) * a.sz0 + (int64_t)(n0 + nl) * a.sz1];
      const double* q = psi + nl * SS + s;
      double acc = q[(S - 1) * S];
      for (int k = S - 2; k >= 0; --k) acc = fma(acc, z, q[k * S]);
      B[pt * sp + (n0 * S + js) * sj] = acc;
    }
  }
  __syncthreads();
}

// one checked coordinate as a byte
__device__ __forceinline__ unsigned char checked(int64_t v, int S, bool& bad) {
  if (v < 0 || v >= (int64_t)S) {
    bad = true;
    return kBad;
  }
  return (unsigned char)v;
}

__device__ __forceinline__ void raise_flag(int* flag) {
  volatile int* f = flag;
  *f = *f | 1;
}

extern __shared__ __attribute__((aligned(16))) double pce_smem[];

template <typename T>
__global__ __launch_bounds__(kThreads) void pce_design_kernel(PceArgs<T> a) {
  double* psi = pce_smem;
  double* B = psi + kPsiElems;
  unsigned char* cd = reinterpret_cast<unsigned char*>(B + a.tp * a.row);   // [N][tc]
  const int t = threadIdx.x, N = a.N, S = a.S, tc = a.tc;
  const int64_t p0 = (int64_t)blockIdx.x * a.tp;
  const int np = a.P - p0 < a.tp ? (int)(a.P - p0) : a.tp;
  eval_basis<T>(a, psi, B, p0, np, a.row, 1);
  const int cl = t % tc, pg = t / tc, npg = kThreads / tc;   // tc is 64, 128 or 256: a wave has one pg
  const int64_t ctiles = (a.C + tc - 1) / tc;
  bool bad = false;
  for (int64_t ct = blockIdx.y; ct < ctiles; ct += gridDim.y) {
    const int64_t c0 = ct * tc;
    const int nc = a.C - c0 < tc ? (int)(a.C - c0) : tc;
    __syncthreads();   // (the readers of the tile before)
    for (int i = t; i < nc * N; i += kThreads) {
      const int c = i / N, n = i - c * N;
      cd[n * tc + c] = checked(a.coords[c0 * N + i], S, bad);
    }
    __syncthreads();
    if (cl >= nc) continue;
    T* Mc = a.out + c0 + cl;
    for (int pt = pg; pt < np; pt += 4 * npg) {
      int row[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = pt + u * npg;
        row[u] = (q < np ? q : np - 1) * a.row;   // (rows past the tile repeat its last point; they are not stored)
      }
      double pr[4] = {1.0, 1.0, 1.0, 1.0};
      bool zero = false;
      for (int n = 0; n < N; ++n) {
        const unsigned char s = cd[n * tc + cl];
        zero = zero || s == kBad;
        const int off = n * S + (s == kBad ? 0 : (int)s);
#pragma unroll
        for (int u = 0; u < 4; ++u) pr[u] *= B[row[u] + off];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = pt + u * npg;
        if (q < np) Mc[(p0 + q) * a.ldm] = (T)(zero ? 0.0 : pr[u]);
      }
    }
  }
  if (bad) raise_flag(a.flag);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pce_predict_kernel(PceArgs<T> a) {
  double* psi = pce_smem;
  double* B = psi + kPsiElems;                 // [N S][tp]
  double* cf = B + a.N * a.S * a.tp;           // [tc]
  unsigned char* cd = reinterpret_cast<unsigned char*>(cf + a.tc);   // [tc][N]
  const int t = threadIdx.x, nt = blockDim.x, N = a.N, S = a.S, tp = a.tp;
  const int64_t p0 = (int64_t)blockIdx.x * tp;
  const int np = a.P - p0 < tp ? (int)(a.P - p0) : tp;
  eval_basis<T>(a, psi, B, p0, np, 1, tp);
  bool bad = false;
  double acc = 0.0;
  const double* Bp = B + (t < np ? t : 0);
  for (int64_t c0 = 0; c0 < a.C; c0 += a.tc) {
    const int nc = a.C - c0 < a.tc ? (int)(a.C - c0) : a.tc;
    __syncthreads();   // (the readers of the tile before)
    for (int i = t; i < nc * N; i += nt) cd[i] = checked(a.coords[c0 * N + i], S, bad);
    for (int i = t; i < nc; i += nt) cf[i] = (double)a.coef[c0 + i];
    __syncthreads();
    if (t >= np) continue;
    int c = 0;
    for (; c + 4 <= nc; c += 4) {   // four candidates in flight, added in increasing c
      double pr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) pr[u] = 1.0;
      bool zero[4] = {false, false, false, false};
      for (int n = 0; n < N; ++n) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned char s = cd[(c + u) * N + n];   // wave-uniform
          zero[u] = zero[u] || s == kBad;
          pr[u] *= Bp[(n * S + (s == kBad ? 0 : (int)s)) * tp];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = fma(cf[c + u], zero[u] ? 0.0 : pr[u], acc);
    }
    for (; c < nc; ++c) {
      double pr = 1.0;
      bool zero = false;
      for (int n = 0; n < N; ++n) {
        const unsigned char s = cd[c * N + n];
        zero = zero || s == kBad;
        pr *= Bp[(n * S + (s == kBad ? 0 : (int)s)) * tp];
      }
      acc = fma(cf[c], zero ? 0.0 : pr, acc);
    }
  }
  if (t < np) a.out[p0 + t] = (T)acc;
  if (bad) raise_flag(a.flag);
}

int pce_check(const char* who, int dtype, int64_t P, int64_t N, int64_t S, int64_t C, const void* Z, const void* Psi,
              const void* coords, const void* out, const void* flag) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(P >= 1 && N >= 1 && S >= 1 && C >= 1, TTR_E_INVALID, "%s: bad sizes P = %lld, N = %lld, S = %lld, C = %lld", who,
              (long long)P, (long long)N, (long long)S, (long long)C);
  TTR_REQUIRE(S <= kMaxOrder, TTR_E_INVALID, "%s: S = %lld exceeds ttr_pce_max_order() = %d", who, (long long)S, kMaxOrder);
  TTR_REQUIRE(N * S <= kMaxBasis, TTR_E_INVALID, "%s: N S = %lld exceeds ttr_pce_max_basis() = %d", who, (long long)(N * S), kMaxBasis);
  TTR_REQUIRE(Z && Psi && coords && out && flag, TTR_E_INVALID, "%s: null pointer", who);
  TTR_REQUIRE(P < ((int64_t)1 << 34) && C < ((int64_t)1 << 40), TTR_E_INVALID, "%s: P = %lld or C = %lld too large", who,
              (long long)P, (long long)C);
  return TTR_OK;
}

template <typename T>
int design_impl(PceArgs<T> a, hipStream_t stream) {
  const int ns = a.N * a.S;
  a.row = ns | 1;
  a.tp = kBasisElems / a.row < kWave ? kBasisElems / a.row : kWave;   // 64 points, 15 at N S = 256
  a.tc = a.N <= kDesignCoordBytes / 256 ? 256 : a.N <= kDesignCoordBytes / 128 ? 128 : 64;
  while (a.tc > kWave && a.C <= a.tc / 2) a.tc /= 2;   // few candidates: the other waves of the workgroup take points, not idle lanes
  a.nm = kPsiElems / (a.S * a.S);
  const int64_t ptiles = ceil_div(a.P, a.tp), ctiles = ceil_div(a.C, a.tc);
  int64_t gy = ceil_div(kFillBlocks, ptiles);
  gy = gy < ctiles ? gy : ctiles;
  const size_t lds = sizeof(double) * (kPsiElems + (size_t)a.tp * a.row) + (size_t)a.N * a.tc;
  ProfScope prof(TTR_PROF_MISC, stream);
  hipLaunchKernelGGL((pce_design_kernel<T>), dim3((unsigned)ptiles, (unsigned)gy), dim3(kThreads), lds, stream, a);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

template <typename T>
int predict_impl(PceArgs<T> a, hipStream_t stream) {
  const int ns = a.N * a.S;
  int pb = kBasisElems / ns;   // >= 16
  pb = pb >= kThreads ? kThreads : pb >= kWave ? pb / kWave * kWave : pb;
  a.tp = pb;
  a.row = 0;
  int tc = kPredictCoordBytes / a.N;   // >= 32
  tc = tc < kPredictMaxTile ? tc : kPredictMaxTile;
  a.tc = (int64_t)tc < a.C ? tc : (int)a.C;
  a.nm = kPsiElems / (a.S * a.S);
  const int threads = pb < kWave ? kWave : pb;
  const size_t lds = sizeof(double) * (kPsiElems + (size_t)ns * pb + a.tc) + (size_t)a.tc * a.N;
  ProfScope prof(TTR_PROF_MISC, stream);
  hipLaunchKernelGGL((pce_predict_kernel<T>), dim3((unsigned)ceil_div(a.P, pb)), dim3(threads), lds, stream, a);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_pce_max_order(void) { return kMaxOrder; }

extern "C" int ttr_pce_max_basis(void) { return kMaxBasis; }

extern "C" int ttr_pce_design(int dtype, int64_t P, int64_t N, int64_t S, int64_t C, const void* Z, int64_t sz0, int64_t sz1,
                              const void* Psi, const void* coords, void* M, int64_t ldm, void* flag, void* stream) {
  const int rc = pce_check("ttr_pce_design", dtype, P, N, S, C, Z, Psi, coords, M, flag);
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(ldm >= C, TTR_E_INVALID, "ttr_pce_design: ldm = %lld < C = %lld", (long long)ldm, (long long)C);
  TTR_REQUIRE((double)P * (double)ldm < 9.0e18 / 64.0, TTR_E_INVALID, "ttr_pce_design: M too large");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return design_impl<T>({P, C, (int)N, (int)S, (const T*)Z, sz0, sz1, (const T*)Psi, (const int64_t*)coords, nullptr, (T*)M, ldm, (int*)flag},
                          (hipStream_t)stream);
  });
}

extern "C" int ttr_pce_predict(int dtype, int64_t P, int64_t N, int64_t S, int64_t C, const void* Z, int64_t sz0, int64_t sz1,
                               const void* Psi, const void* coords, const void* coef, void* y, void* flag, void* stream) {
  const int rc = pce_check("ttr_pce_predict", dtype, P, N, S, C, Z, Psi, coords, y, flag);
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(coef, TTR_E_INVALID, "ttr_pce_predict: null pointer");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return predict_impl<T>({P, C, (int)N, (int)S, (const T*)Z, sz0, sz1, (const T*)Psi, (const int64_t*)coords, (const T*)coef, (T*)y, 0,
                            (int*)flag},
                           (hipStream_t)stream);
  });
}
