// One core of a TT-matrix product that stays in TT format (ttalgebra.py `tt_apply`, `tt_matmul`), for gfx950:
//   ttr_core_compose  out[r S1 + a, p, q, s S2 + b] = sum_j A[r, p, j, s] B[a, j, q, b]
//                     A [R1, P, J, R2], B [S1, J, Q, S2] -> out [R1 S1, P, Q, R2 S2]
// The rank layout is ttr_core_kron's (the first operand's rank major).  P = 1 is a core of vec(t) @ M, Q = 1 one of M @ vec(u),
// the general case one of A @ B.  All three operands are contiguous.
//
// Seen as a GEMM the rows are m = (r, p, s), s fastest (M = R1 P R2 of them), the columns n = (a, q, b), b fastest (N = S1 Q S2)
// and K = J: A(m, j) = A[(rp J + j) R2 + s] with rp = m / R2, B(j, n) = B[((a J + j) Q + q) S2 + b] with aq = n / S2.  The offset of
// an output element is a sum of a row part and a column part,
//   off(m, n) = (r S1 P + p) Q R2 S2 + s S2   +   (a P Q + q) R2 S2 + b,
// and the output (E = M N elements) is far larger than the inputs ((M + N) J): the kernel writes E elements once for 2 J E flops
// and re-reads the operands from the cache, so for the J of a mode (2 .. 64) it is a STORE kernel, and the tile is laid out for
// the store.
//
// A workgroup (4 waves) owns one TTR_COMPOSE_TILE_M x TTR_COMPOSE_TILE_N tile, n tiles fastest (neighbours share the rows of A).
// J is walked in chunks of TTR_COMPOSE_TILE_K through LDS, both operand tiles k-major ([k][m], [k][n]: lanes are consecutive m
// resp. n, which are consecutive addresses inside one rp resp. aq; row stride 80, so the operand reads of an MFMA are
// conflict-free); wave w multiplies rows 16 w .. 16 w + 15 with the <= 4 live column tiles of 16 on v_mfma_{f32,f64}_16x16x4, quads
// of j with a zero-filled tail.  Every output element is ONE chain from 0 in increasing j, whatever its place in a tile.
//
// Store.  The accumulators go to LDS (over the operand tiles) and are written out in MEMORY order.  The columns of a tile fall
// into segments of equal aq, [max(aq S2, n0), min((aq + 1) S2, n0 + 64, N)), of width w; inside a segment the rows m of equal rp
// are S2 apart in memory -- one contiguous run when w = S2.  The tile is therefore walked in the order (segment, m, b): element
// e has the column e / 64 inside its segment, which gives the segment's (lo, w) from a table, then m = (e - 64 lo) / w -- by a
// multiplication with ceil(2^20 / w) from the same table, exact for e < 4096 and w <= 64 -- and b.  Consecutive lanes are
// consecutive addresses along a run, a wave's store covers 256 contiguous bytes (fp32) wherever R2 S2 has them, and where S2 >= 64
// the order is the row-major one.  The row and column parts of the offset come from two more tables, built once per tile (two
// divisions per row and per column, 32-bit while M and N fit).  16-byte packs where S2 is a multiple of the pack (every segment
// and every row of a run then starts on a pack) and `out` is 16-byte aligned; scalar stores with the same arithmetic and the
// same order otherwise -- they are as contiguous per wave, the pack only saves instructions.
//
// No workspace, no atomics, every element written exactly once.  j >= J is staged as zeros in both tiles and never read; a row
// >= M or a column >= N of a short tile stages row 0 resp. column 0 of its operand (a valid address) and is never written.
// Global offsets are 64-bit.  The LDS strides, the live extents and the tested form of the multiply of one quad of j are
// detail/ttr_mfma_tile.h's, shared with the other TT-matrix step kernels.
#include "detail/ttr_internal.h"
#include "detail/ttr_mfma_tile.h"

namespace ttr {

namespace {

constexpr int kTM = TTR_COMPOSE_TILE_M, kTN = TTR_COMPOSE_TILE_N, kTK = TTR_COMPOSE_TILE_K;
static_assert(kTM == 64 && kTN == 64, "the loaders, the wave split and the store walk are written for 64 x 64 tiles");
static_assert(kTK % 4 == 0 && kTK % (kThreads / 64) == 0, "a chunk of j is whole MFMA quads and whole loader passes");
constexpr int kLd = ld_kmajor(kTM);   // operand tiles, [k][m] and [k][n]
constexpr int kLdc = ld_staged(kTN);  // staged output tile
constexpr int kMagicShift = 20; // m = (local * ceil(2^20 / w)) >> 20 is local / w for local < 4096, w <= 64 (4095 * 63 < 2^20)

template <typename T>
struct ComposeArgs {
  int64_t R1, P, J, R2, S1, Q, S2;
  int64_t M, N;      // R1 P R2, S1 Q S2
  int64_t ntiles;    // column tiles
  const T* A;
  const T* B;
  T* out;
};

// x = q d + rem; in 32 bits where the caller knows that x and d fit (uniform)
__device__ __forceinline__ void divmod(int64_t x, int64_t d, bool narrow, int64_t& q, int64_t& rem) {
  if (narrow) {
    const uint32_t qq = (uint32_t)x / (uint32_t)d;
    q = qq;
    rem = (uint32_t)x - qq * (uint32_t)d;
  } else {
    q = x / d;
    rem = x - q * d;
  }
}

// N rows of both operand tiles, 4 j apart: the 2 N loads are issued before the first LDS store waits for one of them
template <typename T, int N>
__device__ __forceinline__ void stage_passes(const T* __restrict__ pa, const T* __restrict__ pb, int64_t astep, int64_t bstep,
                                             T* __restrict__ as_w, T* __restrict__ bs_w) {
  T va[N], vb[N];
#pragma unroll
  for (int it = 0; it < N; ++it) {
    va[it] = pa[it * astep];
    vb[it] = pb[it * bstep];
  }
#pragma unroll
  for (int it = 0; it < N; ++it) {
    as_w[it * (kThreads / 64) * kLd] = va[it];
    bs_w[it * (kThreads / 64) * kLd] = vb[it];
  }
}

// V: elements per store (1, or 16 bytes' worth where S2 is a multiple of that and out is 16-byte aligned)
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void core_compose_kernel(ComposeArgs<T> p) {
  constexpr int kOperands = 2 * kTK * kLd, kStage = kTM * kLdc;
  __shared__ __attribute__((aligned(16))) T smem[kOperands > kStage ? kOperands : kStage];
  __shared__ int64_t s_rowoff[kTM], s_coloff[kTN];
  __shared__ int s_lo[kTN], s_w[kTN], s_magic[kTN];
  T* As = smem;               // [kTK][kLd]
  T* Bs = smem + kTK * kLd;   // [kTK][kLd]
  T* Cs = smem;               // [kTM][kLdc], once the operands have been read

  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);   // (uniform: kept in a scalar register)
  const int64_t mt = (int64_t)blockIdx.x / p.ntiles, nt = (int64_t)blockIdx.x - mt * p.ntiles;
  const int64_t m0 = mt * kTM, n0 = nt * kTN;
  const int mrows = live_extent(p.M, m0, kTM), ncols = live_extent(p.N, n0, kTN);   // live rows and columns of this tile, >= 1
  const int ntl = (ncols + 15) / 16;                          // live column tiles of 16
  const bool narrow = p.M <= 0xffffffffLL && p.N <= 0xffffffffLL;
  const int64_t RS = p.R2 * p.S2;

  // ---- row c and column c of the tile (every wave computes them for its loads; wave 0 writes the store tables)
  const int c = tid & 63;
  const bool row_ok = c < mrows, col_ok = c < ncols;
  int64_t abase = 0, bbase = 0;
  if (row_ok) {
    int64_t rp, s, r, pp;
    divmod(m0 + c, p.R2, narrow, rp, s);
    divmod(rp, p.P, narrow, r, pp);
    abase = rp * p.J * p.R2 + s;   // A[r, pp, j, s] = A[abase + j R2]
    if (wave == 0) s_rowoff[c] = ((r * p.S1 * p.P + pp) * p.Q) * RS + s * p.S2;
  }
  if (col_ok) {
    int64_t aq, b, a, qq;
    divmod(n0 + c, p.S2, narrow, aq, b);
    divmod(aq, p.Q, narrow, a, qq);
    bbase = (a * p.J * p.Q + qq) * p.S2 + b;   // B[a, j, qq, b] = B[bbase + j Q S2]
    if (wave == 0) {
      s_coloff[c] = (a * p.P * p.Q + qq) * RS + b;
      const int64_t seg_lo = aq * p.S2 > n0 ? aq * p.S2 : n0;
      int64_t seg_hi = (aq + 1) * p.S2;
      if (seg_hi > n0 + ncols) seg_hi = n0 + ncols;
      const int w = (int)(seg_hi - seg_lo);   // 1 .. 64
      s_lo[c] = (int)(seg_lo - n0);
      s_w[c] = w;
      s_magic[c] = ((1 << kMagicShift) + w - 1) / w;
    }
  }
  const int64_t bstep = p.Q * p.S2;

  typename Mfma<T>::Acc acc[kTN / 16];
#pragma unroll
  for (int t = 0; t < kTN / 16; ++t) acc[t] = Mfma<T>::zero();
  const bool wave_live = wave * 16 < mrows;

  // wave w stages the rows k = w, w + 4, ... of both operand tiles: its pointers step by 4 j per pass
  const T* pa = p.A + abase + wave * p.R2;
  const T* pb = p.B + bbase + wave * bstep;
  const int64_t astep = (kThreads / 64) * p.R2, bstep4 = (kThreads / 64) * bstep;
  for (int64_t j0 = 0; j0 < p.J; j0 += kTK) {
    const int klive = live_extent(p.J, j0, kTK);
    const int quads = (klive + 3) / 4;   // the quads that are multiplied: only their rows are staged, the tail as zeros
    // `full` passes in which all four waves have a live j: straight-line code per count, all loads in flight together, then
    // the LDS stores.  A dead row or column (abase = 0, bbase = 0) reads A[0, 0, j, 0] resp. B[0, j, 0, 0] -- valid for a live
    // j -- and what it stages reaches only outputs that are never stored.  The pass that holds the tail of J stores zeros for
    // the dead j in BOTH tiles (a uniform branch), so a live output never sees 0 x garbage.
    constexpr int kPasses = kTK / (kThreads / 64);
    const int full = klive >> 2, tail = klive & 3;
    T* as_w = As + wave * kLd + c;
    T* bs_w = Bs + wave * kLd + c;
    switch (full) {
      case 8: stage_passes<T, 8>(pa, pb, astep, bstep4, as_w, bs_w); break;
      case 7: stage_passes<T, 7>(pa, pb, astep, bstep4, as_w, bs_w); break;
      case 6: stage_passes<T, 6>(pa, pb, astep, bstep4, as_w, bs_w); break;
      case 5: stage_passes<T, 5>(pa, pb, astep, bstep4, as_w, bs_w); break;
      case 4: stage_passes<T, 4>(pa, pb, astep, bstep4, as_w, bs_w); break;
      case 3: stage_passes<T, 3>(pa, pb, astep, bstep4, as_w, bs_w); break;
      case 2: stage_passes<T, 2>(pa, pb, astep, bstep4, as_w, bs_w); break;
      case 1: stage_passes<T, 1>(pa, pb, astep, bstep4, as_w, bs_w); break;
      default: break;
    }
    if (tail) {
      T va = T(0), vb = T(0);
      if (wave < tail) {
        va = pa[full * astep];
        vb = pb[full * bstep4];
      }
      as_w[full * (kThreads / 64) * kLd] = va;
      bs_w[full * (kThreads / 64) * kLd] = vb;
    }
    pa += kPasses * astep;
    pb += kPasses * bstep4;
    __syncthreads();
    if (wave_live) {
      const T* a_row = As + (lane >> 4) * kLd + wave * 16 + (lane & 15);
      const T* b_col = Bs + (lane >> 4) * kLd + (lane & 15);
      if (ntl == kTN / 16) {   // a full tile of columns: no test per MFMA, the operand reads of a quad issue together
        for (int q = 0; q < quads; ++q) {
          const T a = a_row[q * 4 * kLd];
          T b[kTN / 16];
#pragma unroll
          for (int t = 0; t < kTN / 16; ++t) b[t] = b_col[q * 4 * kLd + t * 16];
#pragma unroll
          for (int t = 0; t < kTN / 16; ++t) acc[t] = Mfma<T>::mma(a, b[t], acc[t]);
        }
      } else {
        for (int q = 0; q < quads; ++q) mma_quad<T, kTN / 16, 16>(acc, a_row[q * 4 * kLd], b_col + q * 4 * kLd, ntl);
      }
    }
    __syncthreads();   // (the next chunk, or the staged output, overwrites As / Bs)
  }

  // ---- stage: lane holds column lane & 15 of rows Mfma<T>::row(lane, 0 .. 3) of each column tile
  if (wave_live) {
#pragma unroll
    for (int t = 0; t < kTN / 16; ++t)
      if (t < ntl) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) Cs[(wave * 16 + Mfma<T>::row(lane, reg)) * kLdc + t * 16 + (lane & 15)] = acc[t][reg];
      }
  }
  __syncthreads();

  // ---- store in memory order: (segment of equal aq, m, b)
  const int total = kTM * ncols;   // the dead rows of a short tile are walked and skipped
  for (int e = tid * V; e < total; e += kThreads * V) {
    const int col = e >> 6;        // a column inside the element's segment
    const int lo = s_lo[col], w = s_w[col];
    const uint32_t local = (uint32_t)(e - (lo << 6));
    const int m = (int)((local * (uint32_t)s_magic[col]) >> kMagicShift);
    const int n = lo + (int)local - m * w;
    if (m < mrows) {
      T* dst = p.out + s_rowoff[m] + s_coloff[n];
      const T* src = Cs + m * kLdc + n;
      *reinterpret_cast<Pack<T, V>*>(dst) = *reinterpret_cast<const Pack<T, V>*>(src);
    }
  }
}

template <typename T>
int compose_impl(ComposeArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  p.M = p.R1 * p.P * p.R2;
  p.N = p.S1 * p.Q * p.S2;
  p.ntiles = ceil_div(p.N, kTN);
  const int64_t mtiles = ceil_div(p.M, kTM);
  TTR_REQUIRE((double)mtiles * (double)p.ntiles <= 2147483647.0, TTR_E_UNSUPPORTED,
              "ttr_core_compose: %.0f workgroups do not fit a 32-bit grid", (double)mtiles * (double)p.ntiles);
  const dim3 grid((unsigned)(mtiles * p.ntiles)), block(kThreads);
  const bool wide = p.S2 % VW == 0 && aligned16(p.out);
  ProfScope prof(TTR_PROF_GEMM, stream);
  if (wide) hipLaunchKernelGGL((core_compose_kernel<T, VW>), grid, block, 0, stream, p);
  else hipLaunchKernelGGL((core_compose_kernel<T, 1>), grid, block, 0, stream, p);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_core_compose(int dtype, int64_t R1, int64_t P, int64_t J, int64_t R2, int64_t S1, int64_t Q, int64_t S2,
                                const void* A, const void* B, void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_core_compose: bad dtype %d", dtype);
  TTR_REQUIRE(R1 >= 1 && P >= 1 && J >= 1 && R2 >= 1 && S1 >= 1 && Q >= 1 && S2 >= 1, TTR_E_INVALID,
              "ttr_core_compose: bad sizes [%lld, %lld, %lld, %lld] x [%lld, %lld, %lld, %lld]", (long long)R1, (long long)P,
              (long long)J, (long long)R2, (long long)S1, (long long)J, (long long)Q, (long long)S2);
  TTR_REQUIRE(A && B && out, TTR_E_INVALID, "ttr_core_compose: null pointer");
  TTR_REQUIRE(out != A && out != B, TTR_E_INVALID, "ttr_core_compose: out must not be an input");
  const int64_t lim = 2147483647LL;
  TTR_REQUIRE(R1 <= lim && P <= lim && J <= lim && R2 <= lim && S1 <= lim && Q <= lim && S2 <= lim, TTR_E_UNSUPPORTED,
              "ttr_core_compose: an extent does not fit 32 bits");
  TTR_REQUIRE(R1 * S1 <= lim && R2 * S2 <= lim, TTR_E_UNSUPPORTED, "ttr_core_compose: a rank product does not fit 32 bits");
  const double big = 9.0e18 / 64.0;
  TTR_REQUIRE((double)R1 * (double)P * (double)J * (double)R2 < big && (double)S1 * (double)J * (double)Q * (double)S2 < big &&
                  (double)R1 * (double)S1 * (double)P * (double)Q * (double)R2 * (double)S2 < big,
              TTR_E_UNSUPPORTED, "ttr_core_compose: operand too large");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    ComposeArgs<T> p{};
    p.R1 = R1, p.P = P, p.J = J, p.R2 = R2, p.S1 = S1, p.Q = Q, p.S2 = S2;
    p.A = (const T*)A, p.B = (const T*)B, p.out = (T*)out;
    return compose_impl<T>(p, (hipStream_t)stream);
  });
}
