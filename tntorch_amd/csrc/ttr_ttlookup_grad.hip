// The backward of one step of the TT-matrix row lookup (ttr_ttm_lookup_step, ttr_ttlookup.hip) and the segmented row sum that
// pools a bag and sums the first core's gradient (embedding.py `tt_embedding`, `tt_embedding_bag`), for gfx950.
// With X [rows_x, D, R], G [R, I, O, S], Y[p, dd, o, s] = sum_r X[xrow ? xrow[p] : p, dd, r] G[r, idx[p], o, s] and N = O S:
//
//   ttr_ttm_lookup_grad_core    dG[r, i, o, s] = sum_{p: idx[p] = i} sum_dd X[xrow ? xrow[p] : p, dd, r] dY[p, dd, o, s]
//   ttr_ttm_lookup_grad_input   dX[p, dd, r]   = sum_{o, s} dY[p, dd, o, s] G[r, idx[p], o, s]
//   ttr_segment_sum             out[b, :]      = sum_{q = seg[b]}^{seg[b + 1] - 1} (w ? w[src(q)] : 1) Y[src(q), :],  src(q) = perm ? perm[q] : q
//
// Both gradient entries take `perm`, the sample ids grouped by wrapped idx (a stable sort done once by the caller and shared by
// the two): they sort nothing, they count the groups (ttr_group.h's histogram) and scan the counts, all on the device.
//
// ttr_ttm_lookup_grad_core.  Slice i is ONE GEMM with M = R, N = O S and K = (samples of the slice) x D: K row (q, dd) of the
// slice is row dd of X[xrow[perm[off_i + q]]] (R contiguous elements, the M axis) and row dd of dY[perm[off_i + q]] (N
// contiguous elements), so both tiles lie in LDS with k along the rows, As[k][m] and Bs[k][n], and a sample brings D R resp. D N
// contiguous elements.  The element offsets of 256 K rows are worked out at once (one row per thread: perm, the row map, one
// division) and kept in LDS for the eight K tiles of 32 they cover.  A slice's K range is cut into slabs of slab_rows rows
// (ttr_ttm_lookup_grad_core_slab_rows: a function of its seven arguments only); the slabs of all slices are numbered by a scan
// on the device, and a workgroup (4 waves) owns one (slab, 64 x 64 tile of (r, n)) pair, wave w the rows 16 w .. 16 w + 15.  A
// slice of one slab writes dG; the slabs of the others write partial tiles to the workspace [slab, R, N], and the second launch
// adds them in increasing slab order, one chain per element, and writes exact zeros for the slices nobody asked for.  No
// atomics on floating-point data: a slab's chain runs in increasing (q, dd), so the same inputs and the same perm give the same
// bits, and so do xrow = NULL and the identity map.
//
// ttr_ttm_lookup_grad_input.  The forward kernel with the slice staged transposed: the rows of group v are the (sample, dd)
// pairs of its samples in tiles of 64, K = (o, s) is the contiguous axis of dY AND of G, and N = R: As[m][k] = dY[p, dd, k],
// Bs[c][k] = G[n0 + c, v, k], read with G's four strides under the forward's rules.  K is never split: every element of dX is
// one chain of MFMA accumulations in increasing (o, s) of its own dY row and its own slice row; a row's bits do not depend on
// P, on the other samples or on the order inside a group.
//
// ttr_segment_sum.  A workgroup owns one segment and one block of 64 V columns (V = the elements of a 16-byte pack where C is a
// multiple of that and Y is 16-byte aligned, else 1); its four waves take consecutive quarters of the segment, every lane sums
// its V columns over the wave's rows in order, and the four wave sums are added in wave order through LDS.  Accumulation is in
// fp64 with one rounding at the store: fp32 products are exact in fp64; fp64 sums are compensated (TwoSum, the product's error
// from an fma), so the result is the rounded exact sum up to O(len u^2).  A fixed order: the same call gives the same bits.
// Empty segments give zeros.  A long segment sits on ceil(C / (64 V)) workgroups and is not split further.
//
// Index validation runs first in the two gradient entries (idx wraps negative values as in torch; perm and xrow do not): a bad
// entry ORs *oob_flag with 1, and every later kernel returns at entry when the word is set -- on entry or by this call.
// ttr_segment_sum has no flag word: it clamps seg to [0, P] and skips a src outside [0, P), so it never reads out of bounds.
// The LDS strides, stage_pack, the live extents and the multiply of one quad of k are detail/ttr_mfma_tile.h's; the histogram,
// the scan of the row tiles, the validation and the search for a tile's group are detail/ttr_group.h's.
#include "detail/ttr_internal.h"
#include "detail/ttr_group.h"
#include "detail/ttr_mfma_tile.h"

namespace ttr {
namespace {

constexpr int kBM = kGroupTileRows, kBN = 64, kBK = 32;
constexpr int kLdk = ld_kmajor(kBN);          // a tile stored [k][m or n]
constexpr int kOffRows = kThreads;            // K rows whose offsets are worked out at once (one per thread)
constexpr int64_t kTargetGroups = 1024;       // slab rule: workgroups the K rows of all slices are spread over
constexpr int64_t kMinSlab = 256;             // slab rule: K rows below which a slice is never cut

// off[v] = exclusive scan of cnt; soff[v] = exclusive scan of the slabs of `rows` K rows that slice v needs when every sample
// brings `ra` rows, soff[I] = their total.  One workgroup; ttr_group.h's scan_kernel with the rows of a slab a run-time value.
__global__ void __launch_bounds__(1024) slab_scan_kernel(const int32_t* cnt, int64_t I, int64_t ra, int64_t rows, int64_t* off,
                                                         int64_t* soff, const int32_t* flag) {
  __shared__ int64_t s0[1024], s1[1024];
  __shared__ int64_t carry0, carry1;
  if (*flag) return;
  if (threadIdx.x == 0) carry0 = carry1 = 0;
  __syncthreads();
  for (int64_t base = 0; base < I; base += 1024) {
    const int64_t v = base + threadIdx.x;
    const int64_t c = v < I ? cnt[v] : 0;
    const int64_t a = c, t = (c * ra + rows - 1) / rows;
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = t;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
      const int64_t x0 = threadIdx.x >= d ? s0[threadIdx.x - d] : 0, x1 = threadIdx.x >= d ? s1[threadIdx.x - d] : 0;
      __syncthreads();
      s0[threadIdx.x] += x0;
      s1[threadIdx.x] += x1;
      __syncthreads();
    }
    if (v < I) {
      off[v] = carry0 + s0[threadIdx.x] - a;
      soff[v] = carry1 + s1[threadIdx.x] - t;
    }
    __syncthreads();
    if (threadIdx.x == 1023) {
      carry0 += s0[1023];
      carry1 += s1[1023];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) soff[I] = carry1;
}

// ------------------------------------------------------------------ ttr_ttm_lookup_grad_core
template <typename T>
struct GradCoreArgs {
  int64_t P, D, I, slab;    // slab: K rows per slab, a multiple of kBK
  uint32_t R, N;            // N = O S
  const T* X;
  const T* dY;
  T* dG;
  T* part;                  // [slab, R, N]: the partial tiles of the slices of several slabs
  const int64_t* xrow;      // NULL: sample p reads X[p]
  int64_t xstride;
  IdxCol idx;
  const int32_t* cnt;
  const int64_t* off;
  const int64_t* soff;
  const int64_t* perm;
  const int32_t* flag;
  int64_t mtiles, ntiles;
};

template <typename T, int VA, int VB>
__global__ __launch_bounds__(kThreads) void lookup_grad_core_kernel(GradCoreArgs<T> p) {
  __shared__ __attribute__((aligned(16))) T As[kBK * kLdk];   // As[k - k0][m - m0] = X[row k][m]
  __shared__ __attribute__((aligned(16))) T Bs[kBK * kLdk];   // Bs[k - k0][n - n0] = dY[row k][n]
  __shared__ int64_t xoff[kOffRows], yoff[kOffRows];          // element offsets of the K rows kb .. kb + 255, -1 past the slab
  __shared__ int64_t s_v;
  if (*p.flag) return;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tiles = p.mtiles * p.ntiles;
  const int64_t items = p.soff[p.I] * tiles;   // <= (ceil(P D / slab) + I) tiles
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t g = item / tiles, tile = item - g * tiles;   // the tiles of one slab are neighbours: they share its rows
    const int64_t mt = tile / p.ntiles;
    const uint32_t m0 = (uint32_t)mt * kBM, n0 = (uint32_t)(tile - mt * p.ntiles) * kBN;
    const int mrows = live_extent(p.R, m0, kBM), ncols = live_extent(p.N, n0, kBN);   // both >= 1
    const int ntl = (ncols + 15) / 16;
    const bool wave_live = wave * 16 < mrows;
    const int64_t v = group_of_tile(p.soff, p.I, g, &s_v);   // the slice of slab g (a barrier)
    const int64_t nslab = p.soff[v + 1] - p.soff[v];
    const int64_t krows = (int64_t)p.cnt[v] * p.D;
    const int64_t kbeg = (g - p.soff[v]) * p.slab, kend = kbeg + p.slab < krows ? kbeg + p.slab : krows;
    const int64_t gbase = p.off[v];
    typename Mfma<T>::Acc acc[kBN / 16];
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t) acc[t] = Mfma<T>::zero();

    for (int64_t kb = kbeg; kb < kend; kb += kOffRows) {
      {
        const int64_t row = kb + tid;
        int64_t xo = -1, yo = -1;
        if (row < kend) {
          const int64_t q = row / p.D, dd = row - q * p.D;
          const int64_t s = p.perm[gbase + q];
          const int64_t xr = p.xrow ? p.xrow[s * p.xstride] : s;
          xo = (xr * p.D + dd) * (int64_t)p.R;
          yo = (s * p.D + dd) * (int64_t)p.N;
        }
        xoff[tid] = xo;
        yoff[tid] = yo;
      }
      __syncthreads();
      const int64_t kbend = kb + kOffRows < kend ? kb + kOffRows : kend;
      for (int64_t k0 = kb; k0 < kbend; k0 += kBK) {
        const int ko = (int)(k0 - kb);
        constexpr int a_row = kBM / VA, b_row = kBN / VB;
#pragma unroll
        for (int it = 0; it < kBK * a_row / kThreads; ++it) {
          const int e = it * kThreads + tid;
          const int kk = e / a_row, mm = (e % a_row) * VA;
          const int64_t base = xoff[ko + kk];
          stage_pack<T, VA>(As + kk * kLdk + mm, p.X + (base + m0 + mm), base >= 0 && mm < mrows);
        }
#pragma unroll
        for (int it = 0; it < kBK * b_row / kThreads; ++it) {
          const int e = it * kThreads + tid;
          const int kk = e / b_row, nn = (e % b_row) * VB;
          const int64_t base = yoff[ko + kk];
          stage_pack<T, VB>(Bs + kk * kLdk + nn, p.dY + (base + n0 + nn), base >= 0 && nn < ncols);
        }
        __syncthreads();
        if (wave_live) {
          const int quads = (live_extent(kbend, k0, kBK) + 3) / 4;
          const T* a_col = As + (lane >> 4) * kLdk + wave * 16 + (lane & 15);
          const T* b_col = Bs + (lane >> 4) * kLdk + (lane & 15);
          for (int q = 0; q < quads; ++q) mma_quad<T, kBN / 16, 16>(acc, a_col[q * 4 * kLdk], b_col + q * 4 * kLdk, ntl);
        }
        __syncthreads();   // (the next K tile, or the next block of offsets, overwrites As / Bs / xoff / yoff)
      }
    }
    if (!wave_live) continue;   // (wave-uniform; the next item starts with a barrier all waves reach)
    // ---- store: lane holds column lane & 15 of rows Mfma<T>::row(lane, 0 .. 3) of each column tile
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int mm = wave * 16 + Mfma<T>::row(lane, reg);
      if (mm >= mrows) continue;
      const int64_t m = m0 + mm;
      T* out = nslab == 1 ? p.dG + (m * p.I + v) * (int64_t)p.N : p.part + (g * (int64_t)p.R + m) * (int64_t)p.N;
#pragma unroll
      for (int t = 0; t < kBN / 16; ++t) {
        const int n = t * 16 + (lane & 15);
        if (n < ncols) out[n0 + n] = acc[t][reg];
      }
    }
  }
}

// dG[r, i, n] of the slices that are not one slab: zeros for a slice without samples, else the sum of its partial tiles in
// increasing slab order (one chain per element: the association depends on the slice's slab count alone)
template <typename T>
__global__ __launch_bounds__(kThreads) void lookup_grad_core_reduce(GradCoreArgs<T> p) {
  if (*p.flag) return;
  const int64_t total = (int64_t)p.R * p.I * p.N;
  for (int64_t x = (int64_t)blockIdx.x * kThreads + threadIdx.x; x < total; x += (int64_t)gridDim.x * kThreads) {
    const int64_t ri = x / p.N, n = x - ri * p.N;
    const int64_t r = ri / p.I, i = ri - r * p.I;
    const int64_t s0 = p.soff[i], ns = p.soff[i + 1] - s0;
    if (ns == 1) continue;   // written by its one slab
    T s = T(0);
    for (int64_t j = 0; j < ns; ++j) s += p.part[((s0 + j) * (int64_t)p.R + r) * (int64_t)p.N + n];
    p.dG[x] = s;
  }
}

int64_t grad_core_slab_rows(int64_t P, int64_t D, int64_t R, int64_t O, int64_t S) {
  const int64_t tiles = ceil_div(R, kBM) * ceil_div(O * S, kBN);
  const int64_t want = tiles < kTargetGroups ? kTargetGroups / tiles : 1;
  const int64_t rows = align_up(ceil_div(std::max<int64_t>(P * D, 1), want), kBK);
  return rows > kMinSlab ? rows : kMinSlab;
}

struct CoreLayout {
  int64_t cnt, off, soff, part, total;
};

CoreLayout core_layout(int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S) {
  CoreLayout L{};
  int64_t o = 0;
  L.cnt = o; o += align256(I * 4);
  L.off = o; o += align256(I * 8);
  L.soff = o; o += align256((I + 1) * 8);
  L.part = o;
  const int64_t maxslabs = ceil_div(P * D, grad_core_slab_rows(P, D, R, O, S)) + I;   // every slice rounds up by less than one
  o += align256(maxslabs * R * O * S * elem_size(dtype));
  L.total = o;
  return L;
}

// the checks the gradient entries and their queries share (sizes only); `who` names the entry in the message
int grad_sizes_check(const char* who, int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(P >= 0 && D >= 1 && R >= 1 && I >= 1 && O >= 1 && S >= 1, TTR_E_INVALID,
              "%s: bad sizes P = %lld, D = %lld, R = %lld, I = %lld, O = %lld, S = %lld", who, (long long)P, (long long)D, (long long)R,
              (long long)I, (long long)O, (long long)S);
  const double lim = 2147483647.0;
  TTR_REQUIRE((double)D * (double)R <= lim && (double)O * (double)S <= lim && (double)P * (double)D <= lim && (double)I <= lim,
              TTR_E_UNSUPPORTED, "%s: D R, O S, P D and I must be at most 2^31 - 1", who);
  TTR_REQUIRE((double)P * (double)D * (double)R < 9.0e18 / 64.0 && (double)P * (double)D * (double)O * (double)S < 9.0e18 / 64.0 &&
                  (double)R * (double)I * (double)O * (double)S < 9.0e18 / 64.0,
              TTR_E_UNSUPPORTED, "%s: operand too large", who);
  return TTR_OK;
}

// validation of idx, perm and xrow, and the histogram of idx into cnt (zeroed here)
int enqueue_counts(IdxCol idx, const int64_t* perm, const int64_t* xrow, int64_t xstride, int64_t rows_x, int64_t P, int64_t I,
                   int32_t* cnt, int32_t* flag, hipStream_t stream) {
  const unsigned pb = (unsigned)ceil_div(P, kThreads);
  hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, stream, idx, P, I, flag, 1);
  IdxCol cp{perm, 1, 1};
  hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, stream, cp, P, P, flag, 0);   // no wrap: samples 0 .. P - 1
  if (xrow) {
    IdxCol cx{xrow, xstride, 1};
    hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, stream, cx, P, rows_x, flag, 0);
  }
  TTR_HIP_CHECK(hipMemsetAsync(cnt, 0, I * sizeof(int32_t), stream));
  hipLaunchKernelGGL(histogram_kernel, dim3(pb), dim3(kThreads), 0, stream, idx, P, I, cnt, flag);
  return TTR_OK;
}

template <typename T>
int grad_core_impl(GradCoreArgs<T> p, int64_t rows_x, int32_t* flag, char* ws, const CoreLayout& L, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int64_t* off = (int64_t*)(ws + L.off);
  int64_t* soff = (int64_t*)(ws + L.soff);
  p.cnt = cnt;
  p.off = off;
  p.soff = soff;
  p.part = (T*)(ws + L.part);
  p.flag = flag;
  p.mtiles = ceil_div((int64_t)p.R, kBM);
  p.ntiles = ceil_div((int64_t)p.N, kBN);
  const int64_t maxslabs = ceil_div(p.P * p.D, p.slab) + p.I;
  const bool va = p.R % VW == 0 && aligned16(p.X), vb = p.N % VW == 0 && aligned16(p.dY);
  ProfScope prof(TTR_PROF_GEMM, stream);
  const int rc = enqueue_counts(p.idx, p.perm, p.xrow, p.xstride, rows_x, p.P, p.I, cnt, flag, stream);
  if (rc != TTR_OK) return rc;
  hipLaunchKernelGGL(slab_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, p.I, p.D, p.slab, off, soff, flag);
  by_pack_width<T>(va, [&](auto VA) {
    by_pack_width<T>(vb, [&](auto VB) {
      hipLaunchKernelGGL((lookup_grad_core_kernel<T, decltype(VA)::value, decltype(VB)::value>), capped_grid(maxslabs * p.mtiles * p.ntiles),
                         dim3(kThreads), 0, stream, p);
    });
  });
  hipLaunchKernelGGL(lookup_grad_core_reduce<T>, capped_grid(ceil_div((int64_t)p.R * p.I * p.N, kThreads)), dim3(kThreads), 0, stream, p);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

// ------------------------------------------------------------------ ttr_ttm_lookup_grad_input
template <typename T>
struct GradInputArgs {
  int64_t P, D, I;
  uint32_t R, K, S;         // K = O S; S = K where (o, s) is one contiguous axis of G (element k then lies at offset k)
  int64_t gr, gi, go;
  const T* dY;
  const T* G;
  T* dX;
  IdxCol idx;
  const int32_t* cnt;
  const int64_t* off;
  const int64_t* toff;
  const int64_t* perm;
  const int32_t* flag;
  int64_t mtiles, ntiles;   // mtiles: an upper bound of toff[I]
};

template <typename T, int VA, int VB>
__global__ __launch_bounds__(kThreads) void lookup_grad_input_kernel(GradInputArgs<T> p) {
  constexpr int LDR = ld_rowmajor<T>(kBK);    // both tiles stored [m or c][k]
  __shared__ __attribute__((aligned(16))) T As[kBM * LDR];   // As[m][k - k0] = dY[row m][k]
  __shared__ __attribute__((aligned(16))) T Bs[kBN * LDR];   // Bs[c][k - k0] = G[n0 + c, v, k]
  __shared__ int64_t roff[kBM];               // (sample, dd) row of the tile's row m, -1 past the group
  __shared__ int64_t s_v;
  if (*p.flag) return;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tiles = p.toff[p.I] * p.ntiles;   // <= mtiles ntiles
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t mt = tile / p.ntiles;
    const uint32_t n0 = (uint32_t)(tile - mt * p.ntiles) * kBN;
    const int64_t v = group_of_tile(p.toff, p.I, mt, &s_v);
    const int64_t rbeg = p.off[v] * p.D + (mt - p.toff[v]) * kBM;   // rows of the tile in grouped row space: (slot, dd)
    const int64_t rend = (p.off[v] + p.cnt[v]) * p.D;
    if (tid < kBM) {
      const int64_t row = rbeg + tid;
      int64_t ro = -1;
      if (row < rend) {
        const int64_t q = row / p.D, dd = row - q * p.D;
        ro = p.perm[q] * p.D + dd;
      }
      roff[tid] = ro;
    }
    const int ncols = live_extent(p.R, n0, kBN);  // live columns (r) of this tile, >= 1
    const int ntl = (ncols + 15) / 16;
    const T* Gv = p.G + v * p.gi;
    typename Mfma<T>::Acc acc[kBN / 16];
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t) acc[t] = Mfma<T>::zero();
    __syncthreads();  // roff

    for (uint32_t k0 = 0; k0 < p.K; k0 += kBK) {
      constexpr int a_row = kBK / VA, b_row = kBK / VB;
#pragma unroll
      for (int it = 0; it < kBM * a_row / kThreads; ++it) {
        const int e = it * kThreads + tid;
        const int m = e / a_row, kk = (e % a_row) * VA;
        const int64_t base = roff[m];
        stage_pack<T, VA>(As + m * LDR + kk, p.dY + (base * (int64_t)p.K + k0 + kk), base >= 0 && k0 + kk < p.K);
      }
#pragma unroll
      for (int it = 0; it < kBN * b_row / kThreads; ++it) {
        const int e = it * kThreads + tid;
        const int c = e / b_row, kk = (e % b_row) * VB;
        const uint32_t k = k0 + kk;
        const bool live = c < ncols && k < p.K;
        int64_t ko = 0;
        if (live) {
          const uint32_t o = k / p.S;
          ko = (int64_t)(n0 + c) * p.gr + (int64_t)o * p.go + (k - o * p.S);
        }
        stage_pack<T, VB>(Bs + c * LDR + kk, Gv + ko, live);
      }
      __syncthreads();
      const int quads = (live_extent(p.K, k0, kBK) + 3) / 4;
      const T* a_ptr = As + (wave * 16 + (lane & 15)) * LDR + (lane >> 4);
      const T* b_ptr = Bs + (lane & 15) * LDR + (lane >> 4);
      for (int q = 0; q < quads; ++q) mma_quad<T, kBN / 16, 16 * LDR>(acc, a_ptr[q * 4], b_ptr + q * 4, ntl);
      __syncthreads();  // (the next chunk, or the next tile, overwrites As / Bs)
    }
    // ---- store: lane holds column lane & 15 of rows Mfma<T>::row(lane, 0 .. 3) of each column tile
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t base = roff[wave * 16 + Mfma<T>::row(lane, reg)];
      if (base < 0) continue;
#pragma unroll
      for (int t = 0; t < kBN / 16; ++t) {
        const int n = t * 16 + (lane & 15);
        if (n < ncols) p.dX[base * (int64_t)p.R + n0 + n] = acc[t][reg];
      }
    }
    __syncthreads();  // (the next tile overwrites roff / s_v)
  }
}

struct InputLayout {
  int64_t cnt, off, toff, total;
};

InputLayout input_layout(int64_t I) {
  InputLayout L{};
  int64_t o = 0;
  L.cnt = o; o += align256(I * 4);
  L.off = o; o += align256(I * 8);
  L.toff = o; o += align256((I + 1) * 8);
  L.total = o;
  return L;
}

template <typename T>
int grad_input_impl(GradInputArgs<T> p, int32_t* flag, char* ws, const InputLayout& L, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int64_t* off = (int64_t*)(ws + L.off);
  int64_t* toff = (int64_t*)(ws + L.toff);
  p.cnt = cnt;
  p.off = off;
  p.toff = toff;
  p.flag = flag;
  p.mtiles = ceil_div(p.P * p.D, kBM) + p.I;  // every group rounds up by less than one tile
  p.ntiles = ceil_div((int64_t)p.R, kBN);
  const bool va = p.K % VW == 0 && aligned16(p.dY);
  const bool vb = p.S == p.K && p.K % VW == 0 && p.gr % VW == 0 && p.gi % VW == 0 && aligned16(p.G);
  ProfScope prof(TTR_PROF_GEMM, stream);
  const int rc = enqueue_counts(p.idx, p.perm, nullptr, 1, 0, p.P, p.I, cnt, flag, stream);
  if (rc != TTR_OK) return rc;
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, p.I, p.D, off, toff, flag);
  by_pack_width<T>(va, [&](auto VA) {
    by_pack_width<T>(vb, [&](auto VB) {
      hipLaunchKernelGGL((lookup_grad_input_kernel<T, decltype(VA)::value, decltype(VB)::value>), capped_grid(p.mtiles * p.ntiles),
                         dim3(kThreads), 0, stream, p);
    });
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

// ------------------------------------------------------------------ ttr_segment_sum
template <typename T>
struct SegArgs {
  int64_t B, P, C, cblocks;
  const T* Y;
  const T* w;               // NULL: ones
  const int64_t* perm;      // NULL: src(q) = q
  const int64_t* seg;
  T* out;
};

// s + c is the running sum: s the fp64 head; c, for fp64 data, the sum of the roundings of s (TwoSum) and of the products (fma)
template <typename T>
__device__ __forceinline__ void seg_add(double& s, double& c, double w, T y) {
  if constexpr (sizeof(T) == 4) {
    s += w * (double)y;   // the product of two fp32 values is exact in fp64
  } else {
    const double pr = __dmul_rn(w, y), pe = __fma_rn(w, y, -pr);
    const double t = __dadd_rn(s, pr), bp = t - s;
    c += ((s - (t - bp)) + (pr - bp)) + pe;
    s = t;
  }
}

template <typename T, int V>
__global__ __launch_bounds__(kThreads) void segment_sum_kernel(SegArgs<T> p) {
  constexpr int NW = kThreads / kWave, kUnroll = 4;
  __shared__ double red_s[NW][kWave * V], red_c[NW][kWave * V];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t items = p.B * p.cblocks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = item / p.cblocks, c0 = (item - b * p.cblocks) * (kWave * V) + lane * V;
    int64_t beg = p.seg[b], end = p.seg[b + 1];
    beg = beg < 0 ? 0 : (beg > p.P ? p.P : beg);
    end = end < beg ? beg : (end > p.P ? p.P : end);
    const int64_t per = (end - beg + NW - 1) / NW;             // the wave's run of the segment
    const int64_t q0 = beg + wave * per < end ? beg + wave * per : end, q1 = q0 + per < end ? q0 + per : end;
    double s[V], c[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = c[j] = 0.0;
    if (c0 < p.C) {
      for (int64_t q = q0; q < q1; q += kUnroll) {
        Pack<T, V> y[kUnroll];
        double wq[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          wq[u] = 0.0;
#pragma unroll
          for (int j = 0; j < V; ++j) y[u].v[j] = T(0);
          if (q + u < q1) {
            const int64_t src = p.perm ? p.perm[q + u] : q + u;
            if (src >= 0 && src < p.P) {
              wq[u] = p.w ? (double)p.w[src] : 1.0;
              y[u] = *reinterpret_cast<const Pack<T, V>*>(p.Y + (src * p.C + c0));
            }
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
          for (int j = 0; j < V; ++j) seg_add<T>(s[j], c[j], wq[u], y[u].v[j]);   // (a row past the run adds 0 * 0)
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      red_s[wave][lane * V + j] = s[j];
      red_c[wave][lane * V + j] = c[j];
    }
    __syncthreads();
    if (wave == 0 && c0 < p.C) {
      Pack<T, V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        double ts = red_s[0][lane * V + j], tc = red_c[0][lane * V + j];
#pragma unroll
        for (int w = 1; w < NW; ++w) {   // the wave sums in wave order
          seg_add<double>(ts, tc, 1.0, red_s[w][lane * V + j]);
          tc += red_c[w][lane * V + j];
        }
        o.v[j] = (T)(ts + tc);           // the one rounding
      }
      *reinterpret_cast<Pack<T, V>*>(p.out + (b * p.C + c0)) = o;
    }
    __syncthreads();  // (the next item overwrites red_s / red_c)
  }
}

template <typename T>
int segment_sum_impl(SegArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool wide = p.C % VW == 0 && aligned16(p.Y) && aligned16(p.out);
  ProfScope prof(TTR_PROF_MISC, stream);
  by_pack_width<T>(wide, [&](auto V) {
    constexpr int v = decltype(V)::value;
    p.cblocks = ceil_div(p.C, (int64_t)kWave * v);
    hipLaunchKernelGGL((segment_sum_kernel<T, v>), capped_grid(p.B * p.cblocks), dim3(kThreads), 0, stream, p);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace
}  // namespace ttr

using namespace ttr;

extern "C" int64_t ttr_ttm_lookup_grad_core_slab_rows(int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S) {
  const int rc = grad_sizes_check("ttr_ttm_lookup_grad_core_slab_rows", dtype, P, D, R, I, O, S);
  if (rc != TTR_OK) return rc;
  return grad_core_slab_rows(P, D, R, O, S);
}

extern "C" int64_t ttr_ttm_lookup_grad_core_workspace_bytes(int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S) {
  const int rc = grad_sizes_check("ttr_ttm_lookup_grad_core_workspace_bytes", dtype, P, D, R, I, O, S);
  if (rc != TTR_OK) return rc;
  return core_layout(dtype, P, D, R, I, O, S).total;
}

extern "C" int ttr_ttm_lookup_grad_core(int dtype, int64_t P, int64_t rows_x, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S,
                                        const void* X, const void* xrow, const void* dY, const void* idx, int64_t stride_idx,
                                        const void* perm, void* dG, void* oob_flag, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  const char* who = "ttr_ttm_lookup_grad_core";
  const int rc = grad_sizes_check(who, dtype, P, D, R, I, O, S);
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(rows_x >= 1, TTR_E_INVALID, "%s: bad size rows_x = %lld", who, (long long)rows_x);
  TTR_REQUIRE(dG && oob_flag && (P == 0 || (X && dY && idx && perm)), TTR_E_INVALID, "%s: null pointer", who);
  TTR_REQUIRE(dG != X && dG != dY && dG != idx && dG != perm && dG != xrow, TTR_E_INVALID, "%s: dG must not be one of the inputs", who);
  TTR_REQUIRE(P <= 1 || stride_idx >= 1, TTR_E_INVALID, "%s: stride_idx %lld < 1", who, (long long)stride_idx);
  TTR_REQUIRE((double)rows_x <= 2147483647.0 && (double)rows_x * (double)D * (double)R < 9.0e18 / 64.0, TTR_E_UNSUPPORTED,
              "%s: X too large", who);
  const CoreLayout L = core_layout(dtype, P, D, R, I, O, S);
  TTR_REQUIRE(workspace && workspace_bytes >= L.total, TTR_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who,
              (long long)(workspace ? workspace_bytes : 0), (long long)L.total);
  TTR_REQUIRE(workspace != X && workspace != dY && workspace != dG, TTR_E_INVALID, "%s: the workspace must not be an operand", who);
  if (P == 0) {  // no samples: every slice is empty
    TTR_HIP_CHECK(hipMemsetAsync(dG, 0, (size_t)(R * I * O * S * elem_size(dtype)), (hipStream_t)stream));
    return TTR_OK;
  }
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    GradCoreArgs<T> p{};
    p.P = P;
    p.D = D;
    p.I = I;
    p.slab = grad_core_slab_rows(P, D, R, O, S);
    p.R = (uint32_t)R;
    p.N = (uint32_t)(O * S);
    p.X = (const T*)X;
    p.dY = (const T*)dY;
    p.dG = (T*)dG;
    p.xrow = (const int64_t*)xrow;
    p.xstride = P > 1 ? stride_idx : 1;
    p.idx = IdxCol{idx, P > 1 ? stride_idx : 1, 1};
    p.perm = (const int64_t*)perm;
    return grad_core_impl<T>(p, rows_x, (int32_t*)oob_flag, (char*)workspace, L, (hipStream_t)stream);
  });
}

extern "C" int64_t ttr_ttm_lookup_grad_input_workspace_bytes(int64_t P, int64_t I) {
  if (P < 0 || I < 1 || I >= ((int64_t)1 << 31)) return TTR_E_INVALID;
  return input_layout(I).total;
}

extern "C" int ttr_ttm_lookup_grad_input(int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S, const void* dY,
                                         const void* G, const int64_t* g_strides, const void* idx, int64_t stride_idx,
                                         const void* perm, void* dX, void* oob_flag, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
  const char* who = "ttr_ttm_lookup_grad_input";
  const int rc = grad_sizes_check(who, dtype, P, D, R, I, O, S);
  if (rc != TTR_OK) return rc;
  if (P == 0) return TTR_OK;
  TTR_REQUIRE(dY && G && g_strides && idx && perm && dX && oob_flag, TTR_E_INVALID, "%s: null pointer", who);
  TTR_REQUIRE(dX != dY && dX != G && dX != idx && dX != perm, TTR_E_INVALID, "%s: dX must not be one of the inputs", who);
  TTR_REQUIRE(P == 1 || stride_idx >= 1, TTR_E_INVALID, "%s: stride_idx %lld < 1", who, (long long)stride_idx);
  // G [R, I, O, S]: unit stride along s, no negative stride; the stride of an extent-1 axis is free
  const int64_t gr = R > 1 ? g_strides[0] : 0, gi = I > 1 ? g_strides[1] : 0, go = O > 1 ? g_strides[2] : S;
  TTR_REQUIRE((S == 1 || g_strides[3] == 1) && gr >= 0 && gi >= 0 && go >= 0, TTR_E_UNSUPPORTED,
              "%s: G [R, I, O, S] needs a unit stride along S and no negative stride", who);
  TTR_REQUIRE((double)R * (double)gr + (double)I * (double)gi + (double)O * (double)go < 9.0e18 / 64.0, TTR_E_UNSUPPORTED,
              "%s: G too large", who);
  const InputLayout L = input_layout(I);
  TTR_REQUIRE(workspace && workspace_bytes >= L.total, TTR_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who,
              (long long)(workspace ? workspace_bytes : 0), (long long)L.total);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    GradInputArgs<T> p{};
    p.P = P;
    p.D = D;
    p.I = I;
    p.R = (uint32_t)R;
    p.K = (uint32_t)(O * S);
    p.S = go == S ? p.K : (uint32_t)S;
    p.gr = gr;
    p.gi = gi;
    p.go = go;
    p.dY = (const T*)dY;
    p.G = (const T*)G;
    p.dX = (T*)dX;
    p.idx = IdxCol{idx, P > 1 ? stride_idx : 1, 1};
    p.perm = (const int64_t*)perm;
    return grad_input_impl<T>(p, (int32_t*)oob_flag, (char*)workspace, L, (hipStream_t)stream);
  });
}

extern "C" int ttr_segment_sum(int dtype, int64_t B, int64_t P, int64_t C, const void* Y, const void* w, const void* perm,
                               const void* seg, void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_segment_sum: bad dtype %d", dtype);
  TTR_REQUIRE(B >= 0 && P >= 0 && C >= 1, TTR_E_INVALID, "ttr_segment_sum: bad sizes B = %lld, P = %lld, C = %lld", (long long)B,
              (long long)P, (long long)C);
  if (B == 0) return TTR_OK;
  TTR_REQUIRE(seg && out && (P == 0 || Y), TTR_E_INVALID, "ttr_segment_sum: null pointer");
  TTR_REQUIRE(out != Y && out != w && out != perm && out != seg, TTR_E_INVALID, "ttr_segment_sum: out must not be one of the inputs");
  TTR_REQUIRE((double)P * (double)C < 9.0e18 / 64.0 && (double)B * (double)C < 9.0e18 / 64.0, TTR_E_UNSUPPORTED,
              "ttr_segment_sum: operand too large");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    SegArgs<T> p{};
    p.B = B;
    p.P = P;
    p.C = C;
    p.Y = (const T*)Y;
    p.w = (const T*)w;
    p.perm = (const int64_t*)perm;
    p.seg = (const int64_t*)seg;
    p.out = (T*)out;
    return segment_sum_impl<T>(p, (hipStream_t)stream);
  });
}
