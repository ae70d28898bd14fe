// ttr_ttm_lookup_step: one step of the row lookup of a TT-matrix (lookup.py `tt_lookup`), for gfx950:
//
//   Y[p, dd, o, s] = sum_r X[xrow ? xrow[p] : p, dd, r] * G[r, idx[p], o, s]      X [rows_x, D, R], G [R, I, O, S] -> Y [P, D, O, S]
//
// Every sample p multiplies its own D x R block of X by ITS slice G[:, idx[p], :, :] (R x N, N = O S).  Samples that ask for the
// same slice share the right operand, so they are grouped by idx with the device counting sort of detail/ttr_group.h
// (histogram, scan with per-group tile offsets, scatter of sample ids: no host round trip, no readback of the counts) and the
// step becomes one GEMM per group: the rows of group v are the (sample, dd) pairs of its samples, cnt[v] D of them, cut into
// tiles of 64.  A workgroup (4 waves) owns 64 rows x 64 columns of one group: it stages the gathered X rows ([m][k], the row
// base addresses computed once per tile) and the slice ([k][n]) through LDS in chunks of 32 r and multiplies on
// v_mfma_{f32,f64}_16x16x4 -- wave w the rows 16 w .. 16 w + 15 with the live column tiles of 16 -- and stores row m to
// Y[perm[..], dd, :, :], contiguous along (o, s).  D need not divide 64: a sample's rows may lie in two tiles.  Rows past the
// group, columns past N and r past R are zeros in LDS and are never read from or written to global memory; column tiles of 16
// that start at or past N and quads of r wholly past R are not multiplied.  Tiles are walked with a grid stride, the column
// tiles of one row tile next to each other (they share the gathered rows).
//
// Every element of Y is one chain of MFMA accumulations over the quads of r in increasing order -- its order fixed by R and the
// dtype alone -- of its own X row and its own slice column; what else sits in the tile only fills other rows of the MFMA.  So
// a row's bits do not depend on P, on the other samples, on where the scatter's atomics put the sample inside its group, or on
// xrow being NULL or the identity.  No atomics on floating-point data, no split of R across workgroups.
//
// X rows are loaded in 16-byte packs where R is a multiple of 16 bytes of elements and X is aligned (every row then starts on a
// pack), the slice likewise where N and the strides of G are such multiples, (o, s) is one contiguous axis and G is aligned;
// the arithmetic is the same.  The LDS strides, stage_pack, the live extents and the multiply of one quad of k are
// detail/ttr_mfma_tile.h's, shared with the other TT-matrix step kernels; the search for a row tile's group is ttr_group.h's.
//
// Index validation runs first (idx wraps negative values as in torch, xrow does not): a bad entry ORs *oob_flag with 1, and
// every later kernel returns at entry when the word is set -- on entry or by this call.  The word is never cleared here: the
// steps of a chain share it.
#include "detail/ttr_internal.h"
#include "detail/ttr_group.h"
#include "detail/ttr_mfma_tile.h"

namespace ttr {
namespace {

constexpr int kBM = kGroupTileRows, kBN = 64, kBK = 32;
constexpr int kLdb = ld_kmajor(kBN);  // slice tile, [k][n]

template <typename T>
struct LookupArgs {
  int64_t P, D, I;
  uint32_t R, N, S;  // N = O S; S = N where (o, s) is one contiguous axis (column n then lies at offset n)
  int64_t gr, gi, go;
  const T* X;
  const T* G;
  T* Y;
  IdxCol idx;
  const int64_t* xrow;  // NULL: sample p reads X[p]
  int64_t xstride;
  const int32_t* cnt;
  const int64_t* off;
  const int64_t* toff;
  const int64_t* perm;
  const int32_t* flag;
  int64_t mtiles, ntiles;  // mtiles: an upper bound of toff[I]
};

template <typename T, int VA, int VB>
__global__ __launch_bounds__(kThreads) void lookup_step_kernel(LookupArgs<T> p) {
  constexpr int LDA = ld_rowmajor<T>(kBK);  // X tile, [m][k]
  __shared__ __attribute__((aligned(16))) T As[kBM * LDA];
  __shared__ __attribute__((aligned(16))) T Bs[kBK * kLdb];
  __shared__ int64_t xoff[kBM], yoff[kBM];
  __shared__ int64_t s_v;
  if (*p.flag) return;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t live_mtiles = p.toff[p.I];
  const int64_t tiles = live_mtiles * p.ntiles;  // <= mtiles ntiles
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t mt = tile / p.ntiles;
    const uint32_t n0 = (uint32_t)(tile - mt * p.ntiles) * kBN;
    const int64_t v = group_of_tile(p.toff, p.I, mt, &s_v);
    const int64_t rbeg = p.off[v] * p.D + (mt - p.toff[v]) * kBM;   // rows of the tile in grouped row space: (slot, dd)
    const int64_t rend = (p.off[v] + p.cnt[v]) * p.D;
    if (tid < kBM) {
      const int64_t row = rbeg + tid;
      int64_t xo = -1, yo = -1;
      if (row < rend) {
        const int64_t q = row / p.D, dd = row - q * p.D;
        const int64_t s = p.perm[q];
        const int64_t xr = p.xrow ? p.xrow[s * p.xstride] : s;
        xo = (xr * p.D + dd) * (int64_t)p.R;
        yo = (s * p.D + dd) * (int64_t)p.N;
      }
      xoff[tid] = xo;
      yoff[tid] = yo;
    }
    const int ncols = live_extent(p.N, n0, kBN);  // live columns of this tile, >= 1
    const int ntl = (ncols + 15) / 16;            // live column tiles of 16
    // the slice column this thread stages (the same in every chunk of r)
    constexpr int per_row = kBN / VB;
    const int bn = (tid % per_row) * VB;
    const bool bn_live = bn < ncols;
    int64_t bcol = 0;
    if (bn_live) {
      const uint32_t n = n0 + bn, o = n / p.S;
      bcol = (int64_t)o * p.go + (n - o * p.S);
    }
    const T* Gs = p.G + v * p.gi + bcol;
    typename Mfma<T>::Acc acc[kBN / 16];
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t) acc[t] = Mfma<T>::zero();
    __syncthreads();  // xoff / yoff

    for (uint32_t k0 = 0; k0 < p.R; k0 += kBK) {
      // ---- X tile: As[m][k - k0] = X[row m][k]
#pragma unroll
      for (int it = 0; it < kBM * (kBK / VA) / kThreads; ++it) {
        const int e = it * kThreads + tid;
        const int m = e / (kBK / VA), kk = (e % (kBK / VA)) * VA;
        const int64_t base = xoff[m];
        stage_pack<T, VA>(As + m * LDA + kk, p.X + (base + k0 + kk), base >= 0 && k0 + kk < p.R);
      }
      // ---- slice tile: Bs[k - k0][n - n0] = G[k, v, n]
#pragma unroll
      for (int it = 0; it < kBK * per_row / kThreads; ++it) {
        const int kk = it * (kThreads / per_row) + tid / per_row;
        const uint32_t k = k0 + kk;
        stage_pack<T, VB>(Bs + kk * kLdb + bn, Gs + (int64_t)k * p.gr, bn_live && k < p.R);
      }
      __syncthreads();
      const int quads = (live_extent(p.R, k0, kBK) + 3) / 4;
      const T* a_row = As + (wave * 16 + (lane & 15)) * LDA + (lane >> 4);
      const T* b_col = Bs + (lane >> 4) * kLdb + (lane & 15);
      for (int q = 0; q < quads; ++q) mma_quad<T, kBN / 16, 16>(acc, a_row[q * 4], b_col + q * 4 * kLdb, ntl);
      __syncthreads();  // (the next chunk, or the next tile, overwrites As / Bs)
    }
    // ---- store: lane holds column lane & 15 of rows Mfma<T>::row(lane, 0 .. 3) of each column tile
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t base = yoff[wave * 16 + Mfma<T>::row(lane, reg)];
      if (base < 0) continue;
#pragma unroll
      for (int t = 0; t < kBN / 16; ++t) {
        const int n = t * 16 + (lane & 15);
        if (n < ncols) p.Y[base + n0 + n] = acc[t][reg];
      }
    }
    __syncthreads();  // (the next tile overwrites xoff / yoff / s_v)
  }
}

struct Layout {
  int64_t cnt, cursor, off, toff, perm, total;
};

Layout layout(int64_t P, int64_t I) {
  Layout L{};
  int64_t o = 0;
  L.cnt = o; o += I * 4;                 // cnt and cursor are neighbours: one memset clears both
  L.cursor = o; o += align256(I * 4);
  o = align256(o);
  L.off = o; o += align256(I * 8);
  L.toff = o; o += align256((I + 1) * 8);
  L.perm = o; o += align256(std::max<int64_t>(P, 1) * 8);
  L.total = o;
  return L;
}

template <typename T>
int lookup_impl(LookupArgs<T> p, int64_t rows_x, int32_t* flag, char* ws, const Layout& L, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int32_t* cursor = (int32_t*)(ws + L.cursor);
  int64_t* off = (int64_t*)(ws + L.off);
  int64_t* toff = (int64_t*)(ws + L.toff);
  int64_t* perm = (int64_t*)(ws + L.perm);
  p.cnt = cnt;
  p.off = off;
  p.toff = toff;
  p.perm = perm;
  p.flag = flag;
  p.mtiles = ceil_div(p.P * p.D, kBM) + p.I;  // every group rounds up by less than one tile
  p.ntiles = ceil_div((int64_t)p.N, kBN);
  const dim3 grid = capped_grid(p.mtiles * p.ntiles);
  const unsigned pb = (unsigned)ceil_div(p.P, kThreads);
  const bool va = p.R % VW == 0 && aligned16(p.X);
  const bool vb = p.S == p.N && p.N % VW == 0 && p.gr % VW == 0 && p.gi % VW == 0 && aligned16(p.G);
  ProfScope prof(TTR_PROF_GEMM, stream);
  hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, stream, p.idx, p.P, p.I, flag, 1);
  if (p.xrow) {
    IdxCol cx{p.xrow, p.xstride, 1};
    hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, stream, cx, p.P, rows_x, flag, 0);  // no wrap: rows 0 .. rows_x-1
  }
  TTR_HIP_CHECK(hipMemsetAsync(cnt, 0, 2 * p.I * sizeof(int32_t), stream));
  enqueue_group_sort(p.idx, p.P, p.I, p.D, cnt, cursor, off, toff, perm, flag, stream);
  by_pack_width<T>(va, [&](auto VA) {
    by_pack_width<T>(vb, [&](auto VB) {
      hipLaunchKernelGGL((lookup_step_kernel<T, decltype(VA)::value, decltype(VB)::value>), grid, dim3(kThreads), 0, stream, p);
    });
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace
}  // namespace ttr

using namespace ttr;

extern "C" int64_t ttr_ttm_lookup_workspace_bytes(int64_t P, int64_t I) {
  if (P < 0 || I < 1 || I >= ((int64_t)1 << 31)) return TTR_E_INVALID;
  return layout(P, I).total;
}

extern "C" int ttr_ttm_lookup_step(int dtype, int64_t P, int64_t rows_x, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S,
                                   const void* X, const void* xrow, const void* G, const int64_t* g_strides, const void* idx,
                                   int64_t stride_idx, void* Y, void* oob_flag, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_ttm_lookup_step: bad dtype %d", dtype);
  TTR_REQUIRE(P >= 0 && rows_x >= 1 && D >= 1 && R >= 1 && I >= 1 && O >= 1 && S >= 1, TTR_E_INVALID,
              "ttr_ttm_lookup_step: bad sizes P = %lld, rows_x = %lld, D = %lld, R = %lld, I = %lld, O = %lld, S = %lld", (long long)P,
              (long long)rows_x, (long long)D, (long long)R, (long long)I, (long long)O, (long long)S);
  if (P == 0) return TTR_OK;
  TTR_REQUIRE(X && G && g_strides && idx && Y && oob_flag, TTR_E_INVALID, "ttr_ttm_lookup_step: null pointer");
  TTR_REQUIRE(X != Y && G != Y && idx != Y && xrow != Y, TTR_E_INVALID, "ttr_ttm_lookup_step: Y must not be one of the inputs");
  TTR_REQUIRE(P == 1 || stride_idx >= 1, TTR_E_INVALID, "ttr_ttm_lookup_step: stride_idx %lld < 1", (long long)stride_idx);
  const double lim = 2147483647.0;
  TTR_REQUIRE((double)D * (double)R <= lim && (double)O * (double)S <= lim && (double)P * (double)D <= lim &&
                  (double)I <= lim && (double)rows_x <= lim,
              TTR_E_UNSUPPORTED, "ttr_ttm_lookup_step: D R, O S, P D, I and rows_x must be at most 2^31 - 1");
  TTR_REQUIRE((double)rows_x * (double)D * (double)R < 9.0e18 / 64.0 && (double)P * (double)D * (double)O * (double)S < 9.0e18 / 64.0,
              TTR_E_UNSUPPORTED, "ttr_ttm_lookup_step: operand too large");
  // G [R, I, O, S]: unit stride along s, no negative stride; the stride of an extent-1 axis is free
  const int64_t gr = R > 1 ? g_strides[0] : 0, gi = I > 1 ? g_strides[1] : 0, go = O > 1 ? g_strides[2] : S;
  TTR_REQUIRE((S == 1 || g_strides[3] == 1) && gr >= 0 && gi >= 0 && go >= 0, TTR_E_UNSUPPORTED,
              "ttr_ttm_lookup_step: G [R, I, O, S] needs a unit stride along S and no negative stride");
  TTR_REQUIRE((double)R * (double)gr + (double)I * (double)gi + (double)O * (double)go < 9.0e18 / 64.0, TTR_E_UNSUPPORTED,
              "ttr_ttm_lookup_step: G too large");
  const Layout L = layout(P, I);
  TTR_REQUIRE(workspace && workspace_bytes >= L.total, TTR_E_WORKSPACE, "ttr_ttm_lookup_step: workspace %lld < %lld bytes",
              (long long)workspace_bytes, (long long)L.total);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    LookupArgs<T> p{};
    p.P = P;
    p.D = D;
    p.I = I;
    p.R = (uint32_t)R;
    p.N = (uint32_t)(O * S);
    p.S = go == S ? p.N : (uint32_t)S;
    p.gr = gr;
    p.gi = gi;
    p.go = go;
    p.X = (const T*)X;
    p.G = (const T*)G;
    p.Y = (T*)Y;
    p.idx = IdxCol{idx, P > 1 ? stride_idx : 1, 1};
    p.xrow = (const int64_t*)xrow;
    p.xstride = P > 1 ? stride_idx : 1;
    return lookup_impl<T>(p, rows_x, (int32_t*)oob_flag, (char*)workspace, L, (hipStream_t)stream);
  });
}
