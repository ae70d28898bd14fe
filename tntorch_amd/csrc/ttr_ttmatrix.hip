// One step of the product of a TT-matrix / CP-matrix with a dense batch (matrix.py:420-468 `tt_multiply`, `cp_multiply`; DESIGN
// section 24), for gfx950:
//   ttr_ttm_step   Y[dd, o, s] = sum_i sum_r X[i, dd, r] G[r, i, o, s]     X [I, D, R], G [R, I, O, S] -> Y [D, O, S]
//   ttr_cpm_step   Y[dd, o, r] = sum_i X[i, dd, r] C[i, o, r]              X [I, D, R] or [I, D], C [I, O, R] -> Y [D, O, R]
// All operands are contiguous and read / written where they lie: Y of step k, read as [I_{k+1}, D_{k+1}, r_{k+1}], IS the X of
// step k + 1, so a chain of steps never permutes, pads or copies anything.
//
// ttr_ttm_step is a GEMM with M = D, N = O S and K = I R on v_mfma_{f32,f64}_16x16x4 whose K index k = i R + r has TWO strides in
// the left operand: A(dd, k) = X[i D R + dd R + r], B(k, n) = G[(r I + i) N + n].  A workgroup (4 waves) owns a kBM x kBN tile of
// Y and walks K in tiles of kBK through LDS; wave w multiplies rows 16 w .. 16 w + 15 of the tile with all of its <= 4 column
// tiles of 16 (a column tile that starts at or past N is skipped: the last step, N = O < 16, is one MFMA per quad of k).  Tiles
// past the grid are walked with a grid stride; the n tiles of one m tile are neighbours in that order (they share the rows of X).
//
// Loading the A tile.  The k of a K tile [k0, k0 + kBK) fall into SEGMENTS of equal i: [max(k0, i R), min(k0 + kBK, (i + 1) R)),
// w = its length.  Inside a segment the kBM x w elements X[i, dd0 + m, r_lo + j] are runs of w consecutive addresses, R apart --
// one run of kBM R when the segment is a whole i -- so the threads walk the tile in the order (segment, m, j): element e of the
// tile has q = e / kBM inside its segment (which gives i = (k0 + q) / R), then m and j from e - kBM (k_lo - k0) by w.  Nothing
// in this depends on R dividing anything: a quad of k that straddles two i simply has its halves in two segments, loaded from
// their own addresses into neighbouring LDS columns.  Where R is a power of two every segment has w = min(R, kBK) and the two
// divisions are shifts (the P2 instances); any other R divides.  Where R is a multiple of 16 bytes of elements and X is 16-byte
// aligned the same walk is done in packs of that size (every pack lies inside one run of r): one 16-byte load and one LDS
// store per pack; likewise the B tile where N is such a multiple and G is aligned.  The arithmetic does not change.
// k >= K (the tail of the last K tile, and all but K columns when K < 4), rows >= D and columns >= N are stored to LDS as zeros
// and never read from or written to global memory; the quads of k wholly past K are not multiplied at all.
//
// No workspace, no atomics, no split of K across workgroups: every Y element is one chain of MFMA accumulations in increasing k,
// its order fixed by the five extents and the dtype: the same call gives the same bits.
// The LDS strides, stage_pack, the tile decode and the multiply of one quad of k are detail/ttr_mfma_tile.h's, shared with the
// other TT-matrix step kernels.
//
// ttr_cpm_step is a streaming kernel on the vector ALUs: a thread owns a pack of 16 bytes of consecutive r of one (dd, o) where R
// is a multiple of that and C, Y (and X, where it has a rank axis) are 16-byte aligned (else one element, same arithmetic) and
// sums over i, increasing, with fma from 0, four i in flight.  Neighbouring threads are neighbouring packs of Y; X[i, dd, :] is re-read by the O threads of a dd from the cache.
#include "detail/ttr_internal.h"
#include "detail/ttr_mfma_tile.h"

namespace ttr {

namespace {

constexpr int kBM = TTR_TTM_TILE_M, kBN = TTR_TTM_TILE_N, kBK = TTR_TTM_TILE_K;
constexpr int kLdb = ld_kmajor(kBN);          // B tile, [k][n]

template <typename T>
struct TtmArgs {
  int64_t D;
  uint32_t I, R, K, N;      // K = I R, N = O S: both below 2^31
  int rsh, wsh, vsh;        // P2 instances, in packs of VA = 1 << vsh elements: R = 1 << rsh, segment width min(R, kBK) = 1 << wsh
  const T* X;
  const T* G;
  T* Y;
  int64_t mtiles, ntiles;
};

// VA / VB: elements per load of the A / B tile (1, or 16 bytes' worth where R resp. N is a multiple of that and X resp. G is
// 16-byte aligned: every pack then lies inside one run of r resp. one row of G, and inside the tile or outside it as a whole)
template <typename T, bool P2, int VA, int VB>
__global__ __launch_bounds__(kThreads) void ttm_step_kernel(TtmArgs<T> p) {
  constexpr int LDA = ld_rowmajor<T>(kBK);    // A tile, [m][k]
  __shared__ __attribute__((aligned(16))) T As[kBM * LDA];
  __shared__ __attribute__((aligned(16))) T Bs[kBK * kLdb];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tiles = p.mtiles * p.ntiles;
  const int64_t DR = p.D * (int64_t)p.R;
  constexpr uint32_t BKu = kBK / VA;          // the A loader counts k in packs of VA: R, k0 and kBK are multiples of VA
  const uint32_t Ru = p.R / VA;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const TilePos<kBN> tp(tile, p.ntiles, p.N);
    const int64_t dd0 = tp.mt * kBM;
    const uint32_t n0 = tp.n0;
    const int ncols = tp.ncols, ntl = tp.ntl;
    typename Mfma<T>::Acc acc[kBN / 16];
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t) acc[t] = Mfma<T>::zero();

    for (uint32_t k0 = 0; k0 < p.K; k0 += kBK) {
      // ---- A tile: As[m][k - k0] = X[i, dd0 + m, r], walked in the order (segment of equal i, m, r)
      const uint32_t k0u = k0 / VA;
#pragma unroll
      for (int it = 0; it < kBM * (int)BKu / kThreads; ++it) {
        const uint32_t e = (uint32_t)(it * kThreads + tid);
        const uint32_t kq = k0u + e / kBM;                                 // a k (in packs) inside the element's segment
        const uint32_t i = P2 ? kq >> p.rsh : kq / Ru;
        const uint64_t seg_lo = (uint64_t)i * Ru, seg_hi = seg_lo + Ru;
        const uint32_t k_lo = seg_lo > k0u ? (uint32_t)seg_lo : k0u;
        const uint32_t k_hi = seg_hi < (uint64_t)k0u + BKu ? (uint32_t)seg_hi : k0u + BKu;
        const uint32_t w = k_hi - k_lo;
        const uint32_t local = e - kBM * (k_lo - k0u);                     // < kBM w
        const uint32_t m = P2 ? local >> p.wsh : local / w;
        const uint32_t ku = k_lo + (local - m * w);
        stage_pack<T, VA>(As + m * LDA + (ku - k0u) * VA,
                          p.X + ((int64_t)i * DR + (dd0 + m) * (int64_t)p.R + (ku - (uint32_t)seg_lo) * VA), i < p.I && dd0 + m < p.D);
      }
      // ---- B tile: Bs[k - k0][n - n0] = G[(r I + i) N + n]
#pragma unroll
      for (int it = 0; it < kBK * kBN / VB / kThreads; ++it) {
        constexpr int per_row = kBN / VB;
        const int kk = it * (kThreads / per_row) + tid / per_row, n = (tid % per_row) * VB;
        const uint32_t k = k0 + kk;
        const uint32_t i = P2 ? k >> (p.rsh + p.vsh) : k / p.R;
        const uint32_t r = k - i * p.R;
        stage_pack<T, VB>(Bs + kk * kLdb + n, p.G + (((int64_t)r * p.I + i) * (int64_t)p.N + n0 + n), k < p.K && n < ncols);
      }
      __syncthreads();
      const int quads = (live_extent(p.K, k0, kBK) + 3) / 4;
      const T* a_row = As + (wave * 16 + (lane & 15)) * LDA + (lane >> 4);
      const T* b_col = Bs + (lane >> 4) * kLdb + (lane & 15);
      for (int q = 0; q < quads; ++q) mma_quad<T, kBN / 16, 16>(acc, a_row[q * 4], b_col + q * 4 * kLdb, ntl);
      __syncthreads();   // (the next K tile, or the next tile of Y, overwrites As / Bs)
    }
    // ---- store: lane holds column lane & 15 of rows Mfma<T>::row(lane, 0 .. 3) of each column tile
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t) {
      const int n = t * 16 + (lane & 15);
      if (n < ncols) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t dd = dd0 + wave * 16 + Mfma<T>::row(lane, reg);
          if (dd < p.D) p.Y[dd * (int64_t)p.N + n0 + n] = acc[t][reg];
        }
      }
    }
  }
}

inline int log2_exact(uint32_t v) {   // of a power of two
  int s = 0;
  while ((1u << s) < v) ++s;
  return s;
}

template <typename T>
int ttm_impl(TtmArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  p.mtiles = ceil_div(p.D, kBM);
  p.ntiles = ceil_div((int64_t)p.N, kBN);
  const dim3 grid = capped_grid(p.mtiles * p.ntiles);
  const bool p2 = (p.R & (p.R - 1)) == 0;
  const bool va = p.R % VW == 0 && aligned16(p.X), vb = p.N % VW == 0 && aligned16(p.G);
  if (p2) {
    p.vsh = va ? log2_exact(VW) : 0;
    p.rsh = log2_exact(p.R) - p.vsh;
    p.wsh = log2_exact(p.R < (uint32_t)kBK ? p.R : (uint32_t)kBK) - p.vsh;
  }
  ProfScope prof(TTR_PROF_GEMM, stream);
  auto launch = [&](auto P2) {
    by_pack_width<T>(va, [&](auto VA) {
      by_pack_width<T>(vb, [&](auto VB) {
        hipLaunchKernelGGL((ttm_step_kernel<T, decltype(P2)::value, decltype(VA)::value, decltype(VB)::value>), grid, dim3(kThreads),
                           0, stream, p);
      });
    });
  };
  if (p2) launch(std::true_type{});
  else launch(std::false_type{});
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

// ------------------------------------------------------------------ ttr_cpm_step
template <typename T>
struct CpmArgs {
  int64_t I, D, O, R;
  const T* X;
  const T* C;
  T* Y;
};

template <typename T, int P, bool XR>
__global__ __launch_bounds__(kThreads) void cpm_step_kernel(CpmArgs<T> p) {
  const int64_t RP = p.R / P, packs = p.D * p.O * RP;
  const int64_t xrow = XR ? p.R : 1, xslab = p.D * xrow, cslab = p.O * p.R;
  const bool narrow = packs <= 0xffffffffLL;   // (uniform) the two divisions in 32 bits: 64-bit ones cost more than the step's loads
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < packs; e += (int64_t)gridDim.x * kThreads) {
    int64_t row, dd;   // row = dd O + o
    if (narrow) {
      row = (uint32_t)e / (uint32_t)RP;
      dd = (uint32_t)row / (uint32_t)p.O;
    } else {
      row = e / RP;
      dd = row / p.O;
    }
    const int64_t r0 = (e - row * RP) * P, o = row - dd * p.O;
    const T* x = p.X + dd * xrow + (XR ? r0 : 0);
    const T* c = p.C + o * p.R + r0;
    T acc[P];
#pragma unroll
    for (int j = 0; j < P; ++j) acc[j] = T(0);
#pragma unroll 4
    for (int64_t i = 0; i < p.I; ++i) {
      T cv[P], xv[P];
      if (P > 1) {
        const Pack<T, P> cp = *reinterpret_cast<const Pack<T, P>*>(c + i * cslab);
#pragma unroll
        for (int j = 0; j < P; ++j) cv[j] = cp.v[j];
      } else {
        cv[0] = c[i * cslab];
      }
      if (XR && P > 1) {
        const Pack<T, P> xp = *reinterpret_cast<const Pack<T, P>*>(x + i * xslab);
#pragma unroll
        for (int j = 0; j < P; ++j) xv[j] = xp.v[j];
      } else {
        const T x0 = x[i * xslab];
#pragma unroll
        for (int j = 0; j < P; ++j) xv[j] = x0;
      }
#pragma unroll
      for (int j = 0; j < P; ++j) acc[j] = fma(xv[j], cv[j], acc[j]);
    }
    T* y = p.Y + row * p.R + r0;
    if (P > 1) {
      Pack<T, P> out;
#pragma unroll
      for (int j = 0; j < P; ++j) out.v[j] = acc[j];
      *reinterpret_cast<Pack<T, P>*>(y) = out;
    } else {
      y[0] = acc[0];
    }
  }
}

template <typename T, int P>
void cpm_launch(const CpmArgs<T>& p, bool xr, hipStream_t stream) {
  const dim3 grid = capped_grid(ceil_div(p.D * p.O * (p.R / P), kThreads));
  if (xr) hipLaunchKernelGGL((cpm_step_kernel<T, P, true>), grid, dim3(kThreads), 0, stream, p);
  else hipLaunchKernelGGL((cpm_step_kernel<T, P, false>), grid, dim3(kThreads), 0, stream, p);
}

template <typename T>
int cpm_impl(const CpmArgs<T>& p, bool xr, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  // (x_has_rank = 0: X is read one element at a time, whatever its address)
  const bool packed = p.R % VW == 0 && aligned16(p.C) && aligned16(p.Y) && (!xr || aligned16(p.X));
  ProfScope prof(TTR_PROF_MISC, stream);
  if (packed) cpm_launch<T, VW>(p, xr, stream);
  else cpm_launch<T, 1>(p, xr, stream);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_ttm_step(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S, const void* X, const int64_t* x_strides,
                            const void* G, const int64_t* g_strides, void* Y, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_ttm_step: bad dtype %d", dtype);
  TTR_REQUIRE(I >= 1 && D >= 1 && R >= 1 && O >= 1 && S >= 1, TTR_E_INVALID,
              "ttr_ttm_step: bad sizes I = %lld, D = %lld, R = %lld, O = %lld, S = %lld", (long long)I, (long long)D, (long long)R,
              (long long)O, (long long)S);
  TTR_REQUIRE(X && x_strides && G && g_strides && Y, TTR_E_INVALID, "ttr_ttm_step: null pointer");
  TTR_REQUIRE(X != Y && G != Y, TTR_E_INVALID, "ttr_ttm_step: Y must not be X or G");
  const int64_t lim = 2147483647;
  TTR_REQUIRE(D <= lim && (double)I * (double)R <= (double)lim && (double)O * (double)S <= (double)lim, TTR_E_UNSUPPORTED,
              "ttr_ttm_step: D, I R and O S must be at most 2^31 - 1");
  TTR_REQUIRE((double)I * (double)R * (double)D < 9.0e18 / 64.0 && (double)O * (double)S * (double)D < 9.0e18 / 64.0 &&
                  (double)I * (double)R * (double)O * (double)S < 9.0e18 / 64.0,
              TTR_E_UNSUPPORTED, "ttr_ttm_step: operand too large");
  const int64_t xs[3] = {I, D, R}, gs[4] = {R, I, O, S};
  TTR_REQUIRE(contiguous(xs, x_strides, 3), TTR_E_UNSUPPORTED, "ttr_ttm_step: X [I, D, R] must be contiguous");
  TTR_REQUIRE(contiguous(gs, g_strides, 4), TTR_E_UNSUPPORTED, "ttr_ttm_step: G [R, I, O, S] must be contiguous");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    TtmArgs<T> p{};
    p.D = D;
    p.I = (uint32_t)I;
    p.R = (uint32_t)R;
    p.K = (uint32_t)(I * R);
    p.N = (uint32_t)(O * S);
    p.X = (const T*)X;
    p.G = (const T*)G;
    p.Y = (T*)Y;
    return ttm_impl<T>(p, (hipStream_t)stream);
  });
}

extern "C" int ttr_cpm_step(int dtype, int64_t I, int64_t D, int64_t O, int64_t R, int x_has_rank, const void* X, const void* C,
                            void* Y, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_cpm_step: bad dtype %d", dtype);
  TTR_REQUIRE(I >= 1 && D >= 1 && O >= 1 && R >= 1, TTR_E_INVALID, "ttr_cpm_step: bad sizes I = %lld, D = %lld, O = %lld, R = %lld",
              (long long)I, (long long)D, (long long)O, (long long)R);
  TTR_REQUIRE(x_has_rank == 0 || x_has_rank == 1, TTR_E_INVALID, "ttr_cpm_step: x_has_rank must be 0 or 1");
  TTR_REQUIRE(X && C && Y, TTR_E_INVALID, "ttr_cpm_step: null pointer");
  TTR_REQUIRE(X != Y && C != Y, TTR_E_INVALID, "ttr_cpm_step: Y must not be X or C");
  TTR_REQUIRE((double)I * (double)D * (double)R < 9.0e18 / 64.0 && (double)D * (double)O * (double)R < 9.0e18 / 64.0 &&
                  (double)I * (double)O * (double)R < 9.0e18 / 64.0,
              TTR_E_UNSUPPORTED, "ttr_cpm_step: operand too large");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return cpm_impl<T>(CpmArgs<T>{I, D, O, R, (const T*)X, (const T*)C, (T*)Y}, x_has_rank != 0, (hipStream_t)stream);
  });
}
