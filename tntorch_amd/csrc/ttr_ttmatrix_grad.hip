// The backward of one step of the TT-matrix product (ttr_ttm_step, ttr_ttmatrix.hip), for gfx950.  With
// X [I, D, R], G [R, I, O, S] and Y[dd, o, s] = sum_{i, r} X[i, dd, r] G[r, i, o, s]:
//   ttr_ttm_grad_input   dX[i, dd, r]  = sum_{o, s} dY[dd, o, s] G[r, i, o, s]       M = D, N = I R, K = O S
//   ttr_ttm_grad_core    dG[r, i, o, s] = sum_dd   X[i, dd, r]  dY[dd, o, s]         M = I R, N = O S, K = D
// Both on v_mfma_{f32,f64}_16x16x4, operands and accumulators in the dtype, all operands contiguous and read / written where they
// lie.  The layout identity of the forward chain holds backwards: dX of step k, as it lies, IS dY of step k - 1.
//
// ttr_ttm_grad_input.  K = O S is contiguous in BOTH operands: row dd of dY, and row (r I + i) of G for column n = i R + r.  A
// workgroup (4 waves) owns a kBM x kBN tile of the (dd, n) plane and walks K in tiles of kBK through LDS, both tiles stored row by
// row with K along the row (so the B operand is read the way the A operand is); wave w multiplies rows 16 w .. 16 w + 15 with the
// <= 4 live column tiles of 16.  K is never split: every dX element is one chain of MFMA accumulations in increasing k.  The row
// of G behind each of the tile's columns is worked out once per tile (64 divisions, kept in LDS), not once per K tile.
// The store is the mirror of the forward's two-stride load: the accumulators go to LDS (over the operand tiles), and the tile's
// columns fall into SEGMENTS of equal i, [max(n0, i R), min(n0 + kBN, (i + 1) R)), w = its length; inside a segment the kBM x w
// elements dX[i, dd0 + m, r_lo + j] are runs of w consecutive addresses, R apart -- one run of kBM R when the segment is a whole
// i -- so the threads walk the tile in the order (segment, m, j) and neighbouring threads store neighbouring addresses; in packs
// of 16 bytes where R is a multiple of that and dX is 16-byte aligned (every pack then lies inside one run of r).
//
// ttr_ttm_grad_core.  K = D is the SLOW axis of both operands: X[i] is [D, R] and dY is [D, O S], row-major.  The output is small
// (I R x O S) and K is long, so D is cut into slabs of slab_rows and a workgroup owns one (kBM x kBN tile of (m, n), slab) pair.
// Both tiles lie in LDS with k along the rows: As[k][m], Bs[k][n].  The m = i R + r of a tile fall into segments of equal i as
// above; inside a segment the kD x w elements X[i, k, r_lo + j] are runs of w, R apart (one run of kD R for a whole i), walked in
// the order (segment, k, j).  Where a thread's elements lie does not depend on the K tile, so the segment arithmetic is done once
// per tile of the output, before the K loop.  With one slab the tile is scattered straight to dG (row m = i R + r goes to row
// r I + i); with several, the partial tiles go to the workspace [nslab, I R, O S] and a second launch sums them IN SLAB ORDER (in
// eight runs of consecutive slabs, the run sums then in run order: ttm_grad_core_reduce) and scatters.  The K tile after the one
// being multiplied is loaded into registers meanwhile.  No atomics in either entry: the same call gives the same bits.
//
// slab_rows is a function of the six arguments only (never of the device): with tiles = ceil(I R / 64) ceil(O S / 64) and
// want = max(1, 1024 / tiles) slabs, slab_rows = max(256, ceil(D / want) rounded up to a multiple of 32).  So every D up to 256
// is one slab, about 1024 workgroups share a long D, and a slab is never shorter than 8 K tiles.
//
// In LDS, rows >= D, columns past the output and k past K are zeros; they are never read from or written to global memory, and
// column tiles of 16 past N and quads of k past K are not multiplied.
// The LDS strides, stage_pack, ttr_ttm_grad_input's tile decode and the live k of a K tile are detail/ttr_mfma_tile.h's, shared
// with the other TT-matrix step kernels.
#include "detail/ttr_internal.h"
#include "detail/ttr_mfma_tile.h"

namespace ttr {

namespace {

constexpr int kBM = 64, kBN = 64, kBK = 32;
constexpr int kLdk = ld_kmajor(kBN);          // a tile stored [k][m or n]
constexpr int kLdc = ld_staged(kBN);          // the staged output tile
constexpr int64_t kTargetGroups = 1024;       // slab rule: workgroups a long D is spread over
constexpr int64_t kMinSlab = 256;             // slab rule: rows below which D is never cut

// ------------------------------------------------------------------ ttr_ttm_grad_input
template <typename T>
struct GradInputArgs {
  int64_t D;
  uint32_t I, R, N, K;      // N = I R, K = O S: both below 2^31
  const T* dY;
  const T* G;
  T* dX;
  int64_t mtiles, ntiles;
};

// VL: elements per load of both operand tiles (1, or 16 bytes' worth where K is a multiple of that and dY and G are 16-byte
// aligned); VS: elements per store (likewise, R and dX)
template <typename T, int VL, int VS>
__global__ __launch_bounds__(kThreads) void ttm_grad_input_kernel(GradInputArgs<T> p) {
  constexpr int LDR = ld_rowmajor<T>(kBK);    // a tile stored [m or n][k], as ttr_ttm_step's A tile
  constexpr int kOperands = 2 * kBM * LDR, kStaged = kBM * kLdc;
  __shared__ __attribute__((aligned(16))) T smem[kOperands > kStaged ? kOperands : kStaged];
  __shared__ int64_t Goff[kBN];               // element offset of the row of G behind column n0 + c of the tile, -1 past N
  T* As = smem;                               // As[m][k - k0] = dY[dd0 + m, k]
  T* Bs = smem + kBM * LDR;                   // Bs[c][k - k0] = G[(r I + i) K + k], n0 + c = i R + r
  T* Cs = smem;                               // the staged output tile, after the K loop
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tiles = p.mtiles * p.ntiles;
  const int64_t DR = p.D * (int64_t)p.R;
  constexpr uint32_t BNu = kBN / VS;          // the store counts columns in packs of VS: R, n0 and kBN are multiples of VS
  const uint32_t Ru = p.R / VS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const TilePos<kBN> tp(tile, p.ntiles, p.N);
    const int64_t dd0 = tp.mt * kBM;
    const uint32_t n0 = tp.n0;
    const int ncols = tp.ncols, ntl = tp.ntl;
    if (tid < kBN) {
      const uint32_t n = n0 + tid, i = n / p.R, r = n - i * p.R;
      Goff[tid] = tid < ncols ? ((int64_t)r * p.I + i) * (int64_t)p.K : -1;
    }
    __syncthreads();
    typename Mfma<T>::Acc acc[kBN / 16];
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t) acc[t] = Mfma<T>::zero();

    for (uint32_t k0 = 0; k0 < p.K; k0 += kBK) {
      constexpr int per_row = kBK / VL;
#pragma unroll
      for (int it = 0; it < kBM * per_row / kThreads; ++it) {
        const int row = it * (kThreads / per_row) + tid / per_row, kk = (tid % per_row) * VL;
        const bool klive = k0 + kk < p.K;
        stage_pack<T, VL>(As + row * LDR + kk, p.dY + ((dd0 + row) * (int64_t)p.K + k0 + kk), klive && dd0 + row < p.D);
        const int64_t go = Goff[row];
        stage_pack<T, VL>(Bs + row * LDR + kk, p.G + (go + k0 + kk), klive && go >= 0);
      }
      __syncthreads();
      const int quads = (live_extent(p.K, k0, kBK) + 3) / 4;
      const T* a_row = As + (wave * 16 + (lane & 15)) * LDR + (lane >> 4);
      const T* b_row = Bs + (lane & 15) * LDR + (lane >> 4);
      for (int q = 0; q < quads; ++q) {
        const T a = a_row[q * 4];
#pragma unroll
        for (int t = 0; t < kBN / 16; ++t)
          if (t < ntl) acc[t] = Mfma<T>::mma(a, b_row[t * 16 * LDR + q * 4], acc[t]);
      }
      __syncthreads();   // (the next K tile, or the staged output, overwrites As / Bs)
    }
    // ---- stage: lane holds column lane & 15 of rows Mfma<T>::row(lane, 0 .. 3) of each column tile
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) Cs[(wave * 16 + Mfma<T>::row(lane, reg)) * kLdc + t * 16 + (lane & 15)] = acc[t][reg];
    __syncthreads();
    // ---- store: dX[i, dd0 + m, r] = Cs[m][i R + r - n0], walked in the order (segment of equal i, m, r)
    const uint32_t n0u = n0 / VS;
#pragma unroll 4
    for (int it = 0; it < kBM * (int)BNu / kThreads; ++it) {
      const uint32_t e = (uint32_t)(it * kThreads + tid);
      const uint32_t nq = n0u + e / kBM;                                   // a column (in packs) inside the element's segment
      const uint32_t i = nq / Ru;
      const uint64_t seg_lo = (uint64_t)i * Ru, seg_hi = seg_lo + Ru;
      const uint32_t c_lo = seg_lo > n0u ? (uint32_t)seg_lo : n0u;
      const uint32_t c_hi = seg_hi < (uint64_t)n0u + BNu ? (uint32_t)seg_hi : n0u + BNu;
      const uint32_t w = c_hi - c_lo;
      const uint32_t local = e - kBM * (c_lo - n0u);                       // < kBM w
      const uint32_t m = local / w;
      const uint32_t cu = c_lo + (local - m * w);
      if (i < p.I && dd0 + m < p.D)
        *reinterpret_cast<Pack<T, VS>*>(p.dX + ((int64_t)i * DR + (dd0 + m) * (int64_t)p.R + (cu - (uint32_t)seg_lo) * VS)) =
            *reinterpret_cast<const Pack<T, VS>*>(Cs + m * kLdc + (cu - n0u) * VS);
    }
    __syncthreads();   // (the next tile overwrites Goff and Cs)
  }
}

template <typename T>
int grad_input_impl(GradInputArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  p.mtiles = ceil_div(p.D, kBM);
  p.ntiles = ceil_div((int64_t)p.N, kBN);
  const dim3 grid = capped_grid(p.mtiles * p.ntiles);
  const bool vl = p.K % VW == 0 && aligned16(p.dY) && aligned16(p.G), vs = p.R % VW == 0 && aligned16(p.dX);
  ProfScope prof(TTR_PROF_GEMM, stream);
  by_pack_width<T>(vl, [&](auto VL) {
    by_pack_width<T>(vs, [&](auto VS) {
      hipLaunchKernelGGL((ttm_grad_input_kernel<T, decltype(VL)::value, decltype(VS)::value>), grid, dim3(kThreads), 0, stream, p);
    });
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

// ------------------------------------------------------------------ ttr_ttm_grad_core
template <typename T>
struct GradCoreArgs {
  int64_t D, slab, nslab;
  uint32_t I, R, M, N;      // M = I R, N = O S: both below 2^31
  const T* X;
  const T* dY;
  T* dG;
  T* part;                  // [nslab, M, N], used where nslab > 1
  int64_t mtiles, ntiles;
};

// VA / VB: elements per load of the X / dY tile (1, or 16 bytes' worth where R resp. N is a multiple of that and X resp. dY is
// 16-byte aligned: every pack then lies inside one run of r resp. one row of dY)
template <typename T, int VA, int VB>
__global__ __launch_bounds__(kThreads) void ttm_grad_core_kernel(GradCoreArgs<T> p) {
  __shared__ __attribute__((aligned(16))) T As[kBK * kLdk];   // As[k - k0][m - m0] = X[i, k, r]
  __shared__ __attribute__((aligned(16))) T Bs[kBK * kLdk];   // Bs[k - k0][n - n0] = dY[k, n]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tiles = p.mtiles * p.ntiles, items = tiles * p.nslab;
  const int64_t DR = p.D * (int64_t)p.R;
  constexpr uint32_t BMu = kBM / VA;          // the A loader counts m in packs of VA: R, m0 and kBM are multiples of VA
  constexpr int kIterA = kBK * (int)BMu / kThreads;
  const uint32_t Ru = p.R / VA;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t slab = item / tiles, tile = item - slab * tiles;   // the tiles of one slab are neighbours: they share its rows
    const int64_t mt = tile / p.ntiles;
    const uint32_t m0 = (uint32_t)mt * kBM, n0 = (uint32_t)(tile - mt * p.ntiles) * kBN;
    const int mrows = p.M - m0 < (uint32_t)kBM ? (int)(p.M - m0) : kBM;   // live rows of this tile, >= 1
    const int ncols = p.N - n0 < (uint32_t)kBN ? (int)(p.N - n0) : kBN;   // live columns, >= 1
    const int ntl = (ncols + 15) / 16;
    const bool wave_live = wave * 16 < mrows;
    const int64_t kbeg = slab * p.slab, kend = kbeg + p.slab < p.D ? kbeg + p.slab : p.D;
    // ---- where this thread's elements of every A tile lie: the order (segment of equal i, k, r)
    int64_t a_src[kIterA];                    // element offset into X at k = 0, -1 where i >= I
    int a_dst[kIterA], a_k[kIterA];
    const uint32_t m0u = m0 / VA;
#pragma unroll
    for (int it = 0; it < kIterA; ++it) {
      const uint32_t e = (uint32_t)(it * kThreads + tid);
      const uint32_t mq = m0u + e / kBK;                                   // an m (in packs) inside the element's segment
      const uint32_t i = mq / Ru;
      const uint64_t seg_lo = (uint64_t)i * Ru, seg_hi = seg_lo + Ru;
      const uint32_t c_lo = seg_lo > m0u ? (uint32_t)seg_lo : m0u;
      const uint32_t c_hi = seg_hi < (uint64_t)m0u + BMu ? (uint32_t)seg_hi : m0u + BMu;
      const uint32_t w = c_hi - c_lo;
      const uint32_t local = e - kBK * (c_lo - m0u);                       // < kBK w
      const uint32_t kk = local / w;
      const uint32_t cu = c_lo + (local - kk * w);
      a_k[it] = (int)kk;
      a_dst[it] = (int)(kk * kLdk + (cu - m0u) * VA);
      a_src[it] = i < p.I ? (int64_t)i * DR + (int64_t)kk * p.R + (cu - (uint32_t)seg_lo) * VA : -1;
    }
    typename Mfma<T>::Acc acc[kBN / 16];
#pragma unroll
    for (int t = 0; t < kBN / 16; ++t) acc[t] = Mfma<T>::zero();

    // the K tile after the one being multiplied is on its way from global memory into registers meanwhile: the two barriers of
    // a K tile order LDS traffic only, so they do not wait for those loads
    constexpr int per_row = kBN / VB, kIterB = kBK * per_row / kThreads;
    const int b_k = tid / per_row, b_n = (tid % per_row) * VB;   // this thread's B elements: rows b_k + it (kThreads / per_row)
    Pack<T, VA> ra[kIterA];
    Pack<T, VB> rb[kIterB];
    auto fetch = [&](int64_t k0) {
#pragma unroll
      for (int it = 0; it < kIterA; ++it) {
#pragma unroll
        for (int j = 0; j < VA; ++j) ra[it].v[j] = T(0);
        if (a_src[it] >= 0 && k0 + a_k[it] < kend) ra[it] = *reinterpret_cast<const Pack<T, VA>*>(p.X + (a_src[it] + k0 * (int64_t)p.R));
      }
#pragma unroll
      for (int it = 0; it < kIterB; ++it) {
        const int kk = it * (kThreads / per_row) + b_k;
#pragma unroll
        for (int j = 0; j < VB; ++j) rb[it].v[j] = T(0);
        if (k0 + kk < kend && b_n < ncols) rb[it] = *reinterpret_cast<const Pack<T, VB>*>(p.dY + ((k0 + kk) * (int64_t)p.N + n0 + b_n));
      }
    };
    fetch(kbeg);
    for (int64_t k0 = kbeg; k0 < kend; k0 += kBK) {
#pragma unroll
      for (int it = 0; it < kIterA; ++it) *reinterpret_cast<Pack<T, VA>*>(As + a_dst[it]) = ra[it];
#pragma unroll
      for (int it = 0; it < kIterB; ++it)
        *reinterpret_cast<Pack<T, VB>*>(Bs + (it * (kThreads / per_row) + b_k) * kLdk + b_n) = rb[it];
      lds_barrier();
      if (k0 + kBK < kend) fetch(k0 + kBK);
      if (wave_live) {
        const int quads = (live_extent(kend, k0, kBK) + 3) / 4;
        const T* a_col = As + (lane >> 4) * kLdk + wave * 16 + (lane & 15);
        const T* b_col = Bs + (lane >> 4) * kLdk + (lane & 15);
        for (int q = 0; q < quads; ++q) {
          const T a = a_col[q * 4 * kLdk];
#pragma unroll
          for (int t = 0; t < kBN / 16; ++t)
            if (t < ntl) acc[t] = Mfma<T>::mma(a, b_col[q * 4 * kLdk + t * 16], acc[t]);
        }
      }
      lds_barrier();   // (the next K tile, or the next item, overwrites As / Bs)
    }
    if (!wave_live) continue;   // (wave-uniform; no barrier follows in this iteration)
    // ---- store: one slab: row m = i R + r of the tile is row r I + i of dG; several: the partial tile, compact
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int mm = wave * 16 + Mfma<T>::row(lane, reg);
      if (mm >= mrows) continue;
      const uint32_t m = m0 + mm;
      T* out;
      if (p.nslab == 1) {
        const uint32_t i = m / p.R, r = m - i * p.R;
        out = p.dG + ((int64_t)r * p.I + i) * (int64_t)p.N;
      } else {
        out = p.part + (slab * (int64_t)p.M + m) * (int64_t)p.N;
      }
#pragma unroll
      for (int t = 0; t < kBN / 16; ++t) {
        const int n = t * 16 + (lane & 15);
        if (n < ncols) out[n0 + n] = acc[t][reg];
      }
    }
  }
}

// dG[r, i, n] = sum over the slabs of part[slab, i R + r, n], in slab order: the slabs are cut into kRedGroups runs of
// ceil(nslab / kRedGroups) consecutive slabs, a thread sums one run in increasing slab order, and the run sums are added in run
// order.  The association depends on nslab alone, so the same call gives the same bits; one thread per element summing all
// the slabs in one chain was latency-bound (up to 1024 dependent rounds for an output of a few hundred elements).
// A workgroup owns kRedCols consecutive elements x (one 128-byte line of fp32 partials per slab) x kRedGroups runs.
constexpr int kRedGroups = 8, kRedCols = kThreads / kRedGroups;

template <typename T>
__global__ __launch_bounds__(kThreads) void ttm_grad_core_reduce(GradCoreArgs<T> p) {
  __shared__ T sums[kRedGroups][kRedCols];
  const int64_t MN = (int64_t)p.M * p.N, chunks = (MN + kRedCols - 1) / kRedCols;
  const int grp = threadIdx.x / kRedCols, col = threadIdx.x % kRedCols;
  const int64_t per = (p.nslab + kRedGroups - 1) / kRedGroups;
  const int64_t s0 = grp * per, s1 = s0 + per < p.nslab ? s0 + per : p.nslab;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t x = chunk * kRedCols + col;
    T s = T(0);
    if (x < MN) {
#pragma unroll 8
      for (int64_t slab = s0; slab < s1; ++slab) s += p.part[slab * MN + x];
    }
    sums[grp][col] = s;
    __syncthreads();
    if (grp == 0 && x < MN) {
      T total = sums[0][col];
#pragma unroll
      for (int g = 1; g < kRedGroups; ++g) total += sums[g][col];   // (a run past the last slab holds 0)
      const int64_t m = x / p.N;
      const uint32_t n = (uint32_t)(x - m * p.N), i = (uint32_t)m / p.R, r = (uint32_t)m - i * p.R;
      p.dG[((int64_t)r * p.I + i) * (int64_t)p.N + n] = total;
    }
    __syncthreads();   // (the next chunk overwrites sums)
  }
}

int64_t grad_core_slab_rows(int64_t I, int64_t D, int64_t R, int64_t O, int64_t S) {
  const int64_t tiles = ceil_div(I * R, kBM) * ceil_div(O * S, kBN);
  const int64_t want = tiles < kTargetGroups ? kTargetGroups / tiles : 1;
  const int64_t rows = align_up(ceil_div(D, want), kBK);
  return rows > kMinSlab ? rows : kMinSlab;
}

template <typename T>
int grad_core_impl(GradCoreArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  p.mtiles = ceil_div((int64_t)p.M, kBM);
  p.ntiles = ceil_div((int64_t)p.N, kBN);
  const dim3 grid = capped_grid(p.mtiles * p.ntiles * p.nslab);
  const bool va = p.R % VW == 0 && aligned16(p.X), vb = p.N % VW == 0 && aligned16(p.dY);
  ProfScope prof(TTR_PROF_GEMM, stream);
  by_pack_width<T>(va, [&](auto VA) {
    by_pack_width<T>(vb, [&](auto VB) {
      hipLaunchKernelGGL((ttm_grad_core_kernel<T, decltype(VA)::value, decltype(VB)::value>), grid, dim3(kThreads), 0, stream, p);
    });
  });
  if (p.nslab > 1)
    hipLaunchKernelGGL(ttm_grad_core_reduce<T>, capped_grid(ceil_div((int64_t)p.M * p.N, kRedCols)), dim3(kThreads), 0, stream, p);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

// the checks the four entries share (sizes only); `who` names the entry in the message
int grad_sizes_check(const char* who, int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(I >= 1 && D >= 1 && R >= 1 && O >= 1 && S >= 1, TTR_E_INVALID, "%s: bad sizes I = %lld, D = %lld, R = %lld, O = %lld, S = %lld",
              who, (long long)I, (long long)D, (long long)R, (long long)O, (long long)S);
  const int64_t lim = 2147483647;
  TTR_REQUIRE(D <= lim && (double)I * (double)R <= (double)lim && (double)O * (double)S <= (double)lim, TTR_E_UNSUPPORTED,
              "%s: D, I R and O S must be at most 2^31 - 1", who);
  TTR_REQUIRE((double)I * (double)R * (double)D < 9.0e18 / 64.0 && (double)O * (double)S * (double)D < 9.0e18 / 64.0 &&
                  (double)I * (double)R * (double)O * (double)S < 9.0e18 / 64.0,
              TTR_E_UNSUPPORTED, "%s: operand too large", who);
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_ttm_grad_input(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S, const void* dY, const void* G,
                                  void* dX, void* stream) {
  const int rc = grad_sizes_check("ttr_ttm_grad_input", dtype, I, D, R, O, S);
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(dY && G && dX, TTR_E_INVALID, "ttr_ttm_grad_input: null pointer");
  TTR_REQUIRE(dX != dY && dX != G, TTR_E_INVALID, "ttr_ttm_grad_input: dX must not be dY or G");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    GradInputArgs<T> p{};
    p.D = D;
    p.I = (uint32_t)I;
    p.R = (uint32_t)R;
    p.N = (uint32_t)(I * R);
    p.K = (uint32_t)(O * S);
    p.dY = (const T*)dY;
    p.G = (const T*)G;
    p.dX = (T*)dX;
    return grad_input_impl<T>(p, (hipStream_t)stream);
  });
}

extern "C" int64_t ttr_ttm_grad_core_slab_rows(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S) {
  const int rc = grad_sizes_check("ttr_ttm_grad_core_slab_rows", dtype, I, D, R, O, S);
  if (rc != TTR_OK) return rc;
  return grad_core_slab_rows(I, D, R, O, S);
}

extern "C" int64_t ttr_ttm_grad_core_workspace_bytes(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S) {
  const int rc = grad_sizes_check("ttr_ttm_grad_core_workspace_bytes", dtype, I, D, R, O, S);
  if (rc != TTR_OK) return rc;
  const int64_t nslab = ceil_div(D, grad_core_slab_rows(I, D, R, O, S));
  return nslab > 1 ? nslab * I * R * O * S * elem_size(dtype) : 0;
}

extern "C" int ttr_ttm_grad_core(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S, const void* X, const void* dY,
                                 void* dG, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = grad_sizes_check("ttr_ttm_grad_core", dtype, I, D, R, O, S);
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(X && dY && dG, TTR_E_INVALID, "ttr_ttm_grad_core: null pointer");
  TTR_REQUIRE(dG != X && dG != dY, TTR_E_INVALID, "ttr_ttm_grad_core: dG must not be X or dY");
  const int64_t slab = grad_core_slab_rows(I, D, R, O, S), nslab = ceil_div(D, slab);
  const int64_t need = nslab > 1 ? nslab * I * R * O * S * elem_size(dtype) : 0;
  TTR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), TTR_E_WORKSPACE, "ttr_ttm_grad_core: workspace %lld < %lld bytes",
              (long long)(workspace ? workspace_bytes : 0), (long long)need);
  TTR_REQUIRE(need == 0 || (workspace != X && workspace != dY && workspace != dG), TTR_E_INVALID,
              "ttr_ttm_grad_core: the workspace must not be an operand");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    GradCoreArgs<T> p{};
    p.D = D;
    p.slab = slab;
    p.nslab = nslab;
    p.I = (uint32_t)I;
    p.R = (uint32_t)R;
    p.M = (uint32_t)(I * R);
    p.N = (uint32_t)(O * S);
    p.X = (const T*)X;
    p.dY = (const T*)dY;
    p.dG = (T*)dG;
    p.part = (T*)workspace;
    return grad_core_impl<T>(p, (hipStream_t)stream);
  });
}
