// Mode-wise convolution of two TT cores, slice-wise Kronecker in the ranks (tools.py:579-647 `convolve`, computed exactly):
//   ttr_core_convolve  out[r1 S1 + s1, k, r2 S2 + s2] = sum_i a[r1, i, r2] c[s1, k + lo - i, s2],   0 <= k < K
// (terms whose second index leaves [0, J) are absent).  The rank layout is ttr_core_kron's (ttr_cp.hip); the window (lo, K) of the
// full result of I + J - 1 entries is an argument, so a cropped mode ('same', 'valid') is never computed in full.
//
// One workgroup owns one output row (r1, s1), a tile of kTileC = 64 of the contiguous R2 S2 columns and a tile of TK = 16 V
// values of k, V = the elements of a 16-byte store (4 / 2) when R2 S2 and `out` allow it, else 1.  The sum runs over the SHORTER
// mode, P = min(I, J) terms whichever argument that is, in chunks of at most kMaxTaps: per chunk the workgroup stages, expanded to
// the tile's columns, the chunk's fibres of the short operand and the TK + chunk - 1 entries of the long operand they meet, with
// zeros where the long index leaves its mode -- the inner loop has no bounds test.  A thread owns V columns and 4 consecutive k:
// per term one LDS read of the short operand (the same address for every k: a broadcast) and 4 of the long one, 16-byte reads for
// V > 1, conflict-free (the rows are 64 elements, the lanes of a row consecutive).  Every output is accumulated in registers in the
// input precision (FMA), terms in increasing order of the short index, across the chunks, and is stored exactly once, 64
// consecutive columns per k: no atomics, bit-identical from run to run.  LDS per workgroup: (2 kMaxTaps + TK - 1) * 64 elements
// (fp32: 31.75 KiB at V = 4; fp64: 47.5 KiB at V = 2).
//
// Every index comes from validated host arguments; global offsets are 64-bit.  Loads outside the tile's columns, the chunk or
// the long mode are replaced by zeros, stores outside [0, K) x [0, R2 S2) are skipped.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int kMaxTaps = 32;  // terms of the sum staged in LDS at once; above it the sum is chunked
constexpr int kTileC = 64;    // output columns per workgroup
constexpr int kKPT = 4;       // consecutive k per thread

template <typename T>
struct ConvArgs {
  int64_t R1, I, R2, S1, J, S2, lo, K;
  int64_t ctiles, ktiles;  // tiles of the columns and of k
  const T* a;
  const T* c;
  T* out;
};

__device__ __forceinline__ float fma_t(float x, float y, float z) { return fmaf(x, y, z); }
__device__ __forceinline__ double fma_t(double x, double y, double z) { return fma(x, y, z); }

// A_SHORT: the sum runs over a's mode (I <= J), else over c's
template <typename T, int V, bool A_SHORT>
__global__ __launch_bounds__(kThreads) void core_convolve_kernel(ConvArgs<T> p) {
  constexpr int TK = 4 * V * kKPT;          // 256 / (64 / V) rows of threads, kKPT values of k each
  constexpr int LROWS = TK + kMaxTaps - 1;  // entries of the long operand one chunk meets
  __shared__ __attribute__((aligned(16))) T sS[kMaxTaps][kTileC];
  __shared__ __attribute__((aligned(16))) T sL[LROWS][kTileC];

  // block -> (row, column tile, k tile), k fastest
  const int64_t b = blockIdx.x;
  const int64_t kt = b % p.ktiles, rest = b / p.ktiles;
  const int64_t ct = rest % p.ctiles, row = rest / p.ctiles;
  const int64_t r1 = row / p.S1, s1 = row - r1 * p.S1;
  const int64_t C = p.R2 * p.S2, col0 = ct * kTileC, k0 = kt * TK;
  const int64_t P = A_SHORT ? p.I : p.J, Q = A_SHORT ? p.J : p.I;

  const int t = threadIdx.x;
  // staging: a thread owns one column of the tile and every 4th row
  const int scol = t & (kTileC - 1), srow = t >> 6;
  const int64_t gcol = col0 + scol;
  const bool col_ok = gcol < C;
  const int64_t r2 = col_ok ? gcol / p.S2 : 0, s2 = col_ok ? gcol - r2 * p.S2 : 0;
  const T* afib = p.a + r1 * p.I * p.R2 + r2;  // a[r1, i, r2] = afib[i R2]
  const T* cfib = p.c + s1 * p.J * p.S2 + s2;  // c[s1, j, s2] = cfib[j S2]
  const T* sfib = A_SHORT ? afib : cfib;
  const T* lfib = A_SHORT ? cfib : afib;
  const int64_t sstr = A_SHORT ? p.R2 : p.S2, lstr = A_SHORT ? p.S2 : p.R2;

  // compute: V columns, kKPT consecutive k
  constexpr int LPR = kTileC / V;  // lanes per row of the tile
  const int tc0 = (t % LPR) * V, kk0 = (t / LPR) * kKPT;
  T acc[kKPT][V];
#pragma unroll
  for (int kk = 0; kk < kKPT; ++kk)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[kk][e] = T(0);

  for (int64_t p0 = 0; p0 < P; p0 += kMaxTaps) {
    const int pc = (int)(P - p0 < kMaxTaps ? P - p0 : kMaxTaps);
    // term p0 + pp of output k0 + kk reads the long operand at k0 + kk + lo - p0 - pp = base + (kk - pp + pc - 1)
    const int64_t base = k0 + p.lo - p0 - (pc - 1);
    if (p0 > 0) __syncthreads();  // the previous chunk has been read
    for (int r = srow; r < pc; r += kThreads / kTileC) sS[r][scol] = col_ok ? sfib[(p0 + r) * sstr] : T(0);
    const int lrows = TK + pc - 1;
    for (int r = srow; r < lrows; r += kThreads / kTileC) {
      const int64_t g = base + r;
      sL[r][scol] = (col_ok && g >= 0 && g < Q) ? lfib[g * lstr] : T(0);
    }
    __syncthreads();
    for (int pp = 0; pp < pc; ++pp) {
      const Pack<T, V> s = *reinterpret_cast<const Pack<T, V>*>(&sS[pp][tc0]);
      const int lr = kk0 - pp + pc - 1;
#pragma unroll
      for (int kk = 0; kk < kKPT; ++kk) {
        const Pack<T, V> l = *reinterpret_cast<const Pack<T, V>*>(&sL[lr + kk][tc0]);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[kk][e] = fma_t(s.v[e], l.v[e], acc[kk][e]);
      }
    }
  }

  const int64_t col = col0 + tc0;
  if (col >= C) return;  // (V > 1: C is a multiple of V, so a pack lies inside or outside as a whole)
#pragma unroll
  for (int kk = 0; kk < kKPT; ++kk) {
    const int64_t k = k0 + kk0 + kk;
    if (k < p.K) {
      Pack<T, V> o;
#pragma unroll
      for (int e = 0; e < V; ++e) o.v[e] = acc[kk][e];
      *reinterpret_cast<Pack<T, V>*>(p.out + (row * p.K + k) * C + col) = o;
    }
  }
}

template <typename T, int V>
int launch(ConvArgs<T> p, hipStream_t stream) {
  constexpr int TK = 4 * V * kKPT;
  p.ctiles = ceil_div(p.R2 * p.S2, kTileC);
  p.ktiles = ceil_div(p.K, TK);
  const double blocks = (double)p.R1 * (double)p.S1 * (double)p.ctiles * (double)p.ktiles;
  TTR_REQUIRE(blocks <= 2147483647.0, TTR_E_UNSUPPORTED, "ttr_core_convolve: %.0f workgroups do not fit a 32-bit grid", blocks);
  const dim3 grid((unsigned)(p.R1 * p.S1 * p.ctiles * p.ktiles)), block(kThreads);
  ProfScope prof(TTR_PROF_MISC, stream);
  if (p.I <= p.J) hipLaunchKernelGGL((core_convolve_kernel<T, V, true>), grid, block, 0, stream, p);
  else hipLaunchKernelGGL((core_convolve_kernel<T, V, false>), grid, block, 0, stream, p);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

template <typename T>
int convolve_impl(ConvArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool wide = (p.R2 * p.S2) % VW == 0 && aligned16(p.out);
  return wide ? launch<T, VW>(p, stream) : launch<T, 1>(p, stream);
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_core_convolve_max_taps(void) { return kMaxTaps; }

extern "C" int ttr_core_convolve(int dtype, int64_t R1, int64_t I, int64_t R2, int64_t S1, int64_t J, int64_t S2, int64_t lo,
                                 int64_t K, const void* a, const void* c, void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_core_convolve: bad dtype %d", dtype);
  TTR_REQUIRE(R1 >= 1 && I >= 1 && R2 >= 1 && S1 >= 1 && J >= 1 && S2 >= 1 && K >= 1, TTR_E_INVALID,
              "ttr_core_convolve: bad sizes [%lld, %lld, %lld] x [%lld, %lld, %lld], K = %lld", (long long)R1, (long long)I,
              (long long)R2, (long long)S1, (long long)J, (long long)S2, (long long)K);
  const int64_t lim = 2147483647LL;
  TTR_REQUIRE(R1 <= lim && I <= lim && R2 <= lim && S1 <= lim && J <= lim && S2 <= lim, TTR_E_UNSUPPORTED,
              "ttr_core_convolve: an extent does not fit 32 bits");
  TTR_REQUIRE(lo >= 0 && K <= I + J - 1 && lo <= I + J - 1 - K, TTR_E_INVALID,
              "ttr_core_convolve: window (lo = %lld, K = %lld) outside the full result of %lld entries", (long long)lo, (long long)K,
              (long long)(I + J - 1));
  TTR_REQUIRE(a && c && out, TTR_E_INVALID, "ttr_core_convolve: null pointer");
  TTR_REQUIRE(out != a && out != c, TTR_E_INVALID, "ttr_core_convolve: out must not be an input");
  TTR_REQUIRE(R1 * S1 <= lim && R2 * S2 <= lim && (double)R1 * (double)S1 * (double)K * (double)R2 * (double)S2 < 9.0e18 / 64.0,
              TTR_E_UNSUPPORTED, "ttr_core_convolve: result too large");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return convolve_impl<T>({R1, I, R2, S1, J, S2, lo, K, 0, 0, (const T*)a, (const T*)c, (T*)out}, (hipStream_t)stream);
  });
}
