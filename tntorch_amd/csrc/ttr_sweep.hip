// Fused kernels of the right-to-left truncation sweep (gfx950): everything that touches the 64 x (I r) right
// unfolding M of a core between the push-left and the new core.
//
//   ttr_rowgram   G  = M M^T                        (pass 1 of the two-pass 'svd' truncation, and 'eig')   round.py:104-109
//   ttr_rotgram   G2 = (V1^T M)(V1^T M)^T           (pass 2: Gram matrix of the ROTATED rows; the rotated matrix itself is
//                                                    never written -- it only exists 16 columns at a time in registers)
//   ttr_project   right = diag(1/sigma) (V1 V2r)^T M,  left = (V1 V2r) diag(sigma)                          round.py:163-172
//
// All three stream M once, 16 (projection: 32) columns per wave and step, and keep every intermediate in MFMA accumulator registers:
//   * the rotated 16-column slab is computed TRANSPOSED (slab^T = M_c^T V1: A operand = 16 x 4 pieces of M read straight
//     from global memory, B operand = V1 from LDS), which leaves it in the accumulator layout
//     lane (g, cl), register r  <->  slab[row 16 t + cl][column 4 g + r];
//   * in that layout the accumulator registers ARE both MFMA operands of the Gram update
//     G[16 ti + i][16 tj + j] += sum_c slab[16 ti + i][c] slab[16 tj + j][c]  (A[i][k]: lane i + 16 k, B[k][j]: lane j + 16 k,
//     k <-> column 4 k + r): no LDS round trip, no transposition, 10 of the 16 tiles (symmetry).
// Arithmetic per 16 columns and wave: 64 + 40 MFMA 16x16x4 for the rotation + Gram (AI = 64 flop/B: bound by the fp32
// MFMA rate, which equals the vector rate on gfx950), 32 for the projection to rank 32 (AI = 11 flop/B: HBM-bound).
#include <type_traits>

#include "detail/ttr_internal.h"

namespace ttr {

constexpr int KLD = 80;  // leading dimension of the LDS images [k][i]: fragment reads (16 i x 2 k per 32 lanes) hit 32 banks

template <typename T>
struct SweepArgs {
  int R;            // rows of M (<= 64)
  int64_t n;        // columns of M
  const T* M;
  int64_t ldm, strideM;
  const T* V1;      // R x R or nullptr
  int64_t ldv1, strideV1;
  // rowgram / rotgram
  T* G;             // [batch][nsplit][R][R]
  int nsplit;
  const int32_t* skip;  // optional [batch]: != 0 -> this item's workgroups return at once (its G is not written)
  const int32_t* rows32;  // optional [batch] (rowgram, project): != 0 -> rows 32.. of this item's M are exactly zero and are not loaded
  // project
  const T* V2;      // R x R (columns = directions), first ro used
  int64_t ldv2, strideV2;
  const T* sigma;   // [ro] per item (nullable: no scaling)
  int64_t stride_sigma;
  int ro;           // output rank (<= 64)
  int scale_right;  // 1: right rows divided by sigma (round.py:168), left columns multiplied by sigma
  T* right;         // ro x n
  int64_t ldr, strideR;
  T* left;          // R x ro (nullable)
  int64_t ldl, strideL;
  int stagger;      // TTR_KNOB_SWEEP_STAGGER: 0 = columns in order, 1 = project staggered per item, 2 = the Gram kernels as well
  // project, pass-through items of the two-pass truncation (TTR_KNOB_FLAT_PASS; nullptr: none): flat[b] != 0 -> this item's V2 is
  // the identity and its sigma is pass 1's, neither of which is loaded: U = V1[:, :ro], scales from sigma1 (needs V1)
  const int32_t* flat;
  const T* sigma1;
  int64_t stride_sigma1;
};

// One entry of V1 as the product V1 I leaves it in an MFMA accumulator that started at +0: the value itself, and +0 for -0.
template <typename T>
__device__ __forceinline__ T times_identity(T x) { return x + T(0); }

__host__ __device__ inline void split_range(int64_t chunks, int nsplit, int split, int64_t& c0, int64_t& c1) {
  const int64_t per = (chunks + nsplit - 1) / nsplit;
  c0 = (int64_t)split * per;
  c1 = c0 + per < chunks ? c0 + per : chunks;
}

// N consecutive elements with one (or two) wide loads when the caller established the alignment, element-wise otherwise
template <typename T, int N>
__device__ __forceinline__ Pack<T, N> load_pack(const T* __restrict__ p, bool aligned, int64_t valid) {
  Pack<T, N> out;
  if (aligned && valid >= N) {
    typedef T VT __attribute__((ext_vector_type(N)));
    const VT x = *reinterpret_cast<const VT*>(p);
#pragma unroll
    for (int i = 0; i < N; ++i) out.v[i] = x[i];
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) out.v[i] = (i < valid) ? p[i] : T(0);
  }
  return out;
}

// ---------------------------------------------------------------- Gram matrix of the (rotated) rows
template <typename T, bool IDENT>
__global__ __launch_bounds__(kThreads) void rotgram_kernel(SweepArgs<T> p) {
  using M = Mfma<T>;
  using Acc = typename M::Acc;
  constexpr int RED = 4 * 10 * 256;  // per-wave partial tiles for the final reduction
  constexpr int VSZ = 64 * KLD;
  __shared__ __attribute__((aligned(16))) T smem[RED > VSZ ? RED : VSZ];
  T* Vl = smem;  // V1 as [k][row], zero padded to 64 x 64
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.y;
  if (p.skip && p.skip[b] != 0) return;  // (block-uniform) pass 2 is not needed for this item: see ttr_spectrum_flat
  const int split = blockIdx.x;
  const T* __restrict__ Mp = p.M + b * p.strideM;
  const int R = p.R;
  if constexpr (!IDENT) {
    const T* __restrict__ V1 = p.V1 + b * p.strideV1;
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int k = idx >> 6, j = idx & 63;
      Vl[k * KLD + j] = (k < R && j < R) ? V1[(int64_t)k * p.ldv1 + j] : T(0);
    }
    __syncthreads();
  }
  Acc G[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) G[i] = M::zero();
  // (row tiles of an item whose rows 32.. are exactly zero -- rows32 -- are skipped: 3 of the 10 tile products remain)
  const int ntl = (IDENT && p.rows32 && p.rows32[b] != 0 && R > 32) ? 2 : 4;
  auto gram_update = [&](const Acc (&mw)[4]) {
    int idx = 0;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = ti; tj < 4; ++tj) {
        if (tj < ntl) {   // block-uniform
#pragma unroll
          for (int r = 0; r < 4; ++r) G[idx] = M::mma(mw[ti][r], mw[tj][r], G[idx]);
        }
        ++idx;
      }
  };
  if constexpr (IDENT) {
    // 16 columns per step: lane (g, cl) register r <-> M[16 t + cl][c0 + 4 g + r] (any assignment of the 16 columns to
    // (g, r) serves the Gram sum): four consecutive elements, one 16-byte load per row tile
    const bool al = ((p.ldm & 3) == 0) && ((reinterpret_cast<uintptr_t>(Mp) & (4 * sizeof(T) - 1)) == 0);
    int64_t cb, ce;
    split_range((p.n + 15) / 16, p.nsplit, split, cb, ce);
    // (the next step's loads are issued before the current step's MFMAs: with 4 waves per SIMD the 40 MFMAs of a step do not
    // cover an HBM round trip)
    // (rows32: the carry of a bond whose QR packed its rows -- ttr_qr_factor_pushed on an R factor of numerical rank <= 32 -- has
    // exactly zero rows 32..: they are not loaded, their Gram tiles come out as the zeros they are)
    const int Rl = (p.rows32 && p.rows32[b] != 0 && R > 32) ? 32 : R;
    auto load_slab = [&](int64_t c, Acc (&mw)[4]) {
      const int64_t col = c * 16 + 4 * g;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = 16 * t + cl;
        const Pack<T, 4> x = load_pack<T, 4>(Mp + (int64_t)row * p.ldm + col, al, row < Rl ? p.n - col : 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) mw[t][r] = x.v[r];
      }
    };
    // (step order: see project_kernel; the Gram sums are accumulated in an item-dependent order when staggered, knob value 2)
    const int64_t nsteps = ce > cb + wave ? (ce - cb - wave + 3) / 4 : 0;
    const int64_t rot = (p.stagger >= 2 && nsteps > 1) ? (int64_t)(b % nsteps) : 0;
    auto step_c = [&](int64_t sidx) { int64_t sq = sidx + rot; if (sq >= nsteps) sq -= nsteps; return cb + wave + 4 * sq; };
    Acc cur[4], nxt[4];
    if (nsteps > 0) load_slab(step_c(0), cur);
    for (int64_t sidx = 0; sidx < nsteps; ++sidx) {
      const bool more = sidx + 1 < nsteps;
      if (more) load_slab(step_c(sidx + 1), nxt);
      gram_update(cur);
      if (more) {
#pragma unroll
        for (int t = 0; t < 4; ++t) cur[t] = nxt[t];
      }
    }
  } else {
    // 16 columns per step; A operand = 16 x 4 pieces of M straight from global memory (four 64-byte row segments per
    // load).  The kernel runs at ~80 % of the fp32 MFMA rate like this (measured): wider loads only cost registers.
    int64_t cb, ce;
    split_range((p.n + 15) / 16, p.nsplit, split, cb, ce);
    const int Rl = (p.rows32 && p.rows32[b] != 0 && R > 32) ? 32 : R;   // (zero rows 32..: not loaded -- they may not even be written)
    auto load_cols = [&](int64_t c, T (&a)[16]) {
      const int64_t c0 = c * 16;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const int k = 4 * ks + g;
        a[ks] = (k < Rl && c0 + cl < p.n) ? Mp[(int64_t)k * p.ldm + c0 + cl] : T(0);
      }
    };
    const int64_t nsteps = ce > cb + wave ? (ce - cb - wave + 3) / 4 : 0;
    const int64_t rot = (p.stagger >= 2 && nsteps > 1) ? (int64_t)(b % nsteps) : 0;
    auto step_c = [&](int64_t sidx) { int64_t sq = sidx + rot; if (sq >= nsteps) sq -= nsteps; return cb + wave + 4 * sq; };
    T a[16], an[16];
    if (nsteps > 0) load_cols(step_c(0), a);
    for (int64_t sidx = 0; sidx < nsteps; ++sidx) {
      const bool more = sidx + 1 < nsteps;
      if (more) load_cols(step_c(sidx + 1), an);  // in flight under this step's 104 MFMAs (two waves per SIMD do not cover an HBM round trip)
      Acc mw[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        mw[t] = M::zero();
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) mw[t] = M::mma(a[ks], Vl[(4 * ks + g) * KLD + 16 * t + cl], mw[t]);
      }
      gram_update(mw);
      if (more) {
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) a[ks] = an[ks];
      }
    }
  }
  // reduce the four waves' partial tiles and write the block's partial Gram matrix (both triangles)
  __syncthreads();  // Vl is dead: smem becomes the reduction buffer
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) smem[(wave * 10 + i) * 256 + lane * 4 + r] = G[i][r];
  __syncthreads();
  T* __restrict__ Gout = p.G + ((int64_t)b * p.nsplit + split) * R * R;
  for (int idx = tid; idx < 10 * 256; idx += kThreads) {
    const int tile = idx >> 8, e = idx & 255, ln = e >> 2, r = e & 3;
    const T v = (smem[idx] + smem[2560 + idx]) + (smem[5120 + idx] + smem[7680 + idx]);
    int ti = 0, rem = tile;  // tile -> (ti, tj), ti <= tj, row-major over the upper triangle of a 4 x 4 tile grid
    while (rem >= 4 - ti) { rem -= 4 - ti; ++ti; }
    const int tj = ti + rem;
    const int row = 16 * ti + M::row(ln, r), col = 16 * tj + (ln & 15);
    if (row < R && col < R) {
      Gout[row * R + col] = v;
      if (ti != tj) Gout[col * R + row] = v;
    }
  }
}

// ---------------------------------------------------------------- projection onto the kept directions
// LDS image of U = V1 V2[:, :ro] shared by the projection kernels: rows k in blocks of 16 (one block per wave of the
// prologue), block stride UBLK, row stride KLD -- so that a wave can write ITS 16 rows over the V1 rows only it reads.
constexpr int V1LD = 82;            // V1 as [k][m]: A-operand reads (16 k x 2 m per 32 lanes: words 82 cl + g) hit 32 banks
constexpr int UBLK = 16 * V1LD;     // 1312 >= 16 * KLD
__device__ __forceinline__ int urow(int k) { return (k >> 4) * UBLK + (k & 15) * KLD; }

// REST: the second launch of a two-instance projection (project_typed) -- the items project_rows32_kernel has served return at once
template <typename T, bool REST = false>
__global__ __launch_bounds__(kThreads, (sizeof(T) == 4 ? 4 : 1)) void project_kernel(SweepArgs<T> p) {
  if constexpr (REST) {
    if (p.rows32[blockIdx.y] != 0) return;  // (block-uniform)
  }
  using M = Mfma<T>;
  using Acc = typename M::Acc;
  // V2[:, :ro] as [m][i], zero padded (prologue only: leading dimension 72 instead of the conflict-free 80 -- with it the three
  // arrays take 39.7 KB, FOUR workgroups per CU instead of three; the main loop has no software prefetch (stores sit between
  // its loads, and a prefetched step's loads then wait in the same in-order counter: measured 416 -> 700 us), so the HBM
  // round trip is covered by the number of resident waves alone)
  constexpr int V2LD = 72;
  __shared__ __attribute__((aligned(16))) T V2l[64 * V2LD];
  __shared__ __attribute__((aligned(16))) T V1l[64 * V1LD];  // V1 as [k][m]; wave w then overwrites ITS rows 16 w .. 16 w + 15
  T* Ul = V1l;                                               // with U rows (urow()): no other wave reads them before
  __shared__ T isg[64];  // 1 / sigma of the output rows (TTR_SCALE_DIV semantics: 0 below the smallest normal), or 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.y;
  const int split = blockIdx.x;
  const T* __restrict__ Mp = p.M + b * p.strideM;
  const int R = p.R, ro = p.ro;
  const int nt = (ro + 15) / 16;
  const T* __restrict__ V2 = p.V2 + b * p.strideV2;
  // (block-uniform, decided once ahead of every load) pass-through item: V2 = I and sigma = sigma1, see SweepArgs::flat
  const bool flat = p.flat && p.V1 && p.flat[b] != 0;
  const T* __restrict__ sg = flat ? p.sigma1 + b * p.stride_sigma1 : (p.sigma ? p.sigma + b * p.stride_sigma : nullptr);
  T* __restrict__ Lo = (p.left && split == 0) ? p.left + b * p.strideL : nullptr;
  // ---- prologue: U = V1 V2[:, :ro] on the matrix cores (or U = V2[:, :ro]); split 0 also emits left = U diag(sigma)
  if (!flat) {
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int m = idx >> 6, i = idx & 63;
      V2l[m * V2LD + i] = (m < R && i < ro) ? V2[(int64_t)m * p.ldv2 + i] : T(0);
    }
  }
  if (tid < 64) {
    T sc = T(1);
    if (p.scale_right && sg && tid < ro) {
      const T x = sg[tid];
      sc = (fabs((double)x) < (double)Num<T>::tiny()) ? T(0) : T(1) / x;
    }
    isg[tid] = sc;
  }
  if (flat) {  // U = V1[:, :ro], what the product with the identity gives: straight into the image
    const T* __restrict__ V1 = p.V1 + b * p.strideV1;
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int k = idx >> 6, i = idx & 63;
      Ul[urow(k) + i] = (k < R && i < ro) ? times_identity(V1[(int64_t)k * p.ldv1 + i]) : T(0);
    }
  } else if (p.V1) {
    const T* __restrict__ V1 = p.V1 + b * p.strideV1;
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int k = idx >> 6, m = idx & 63;
      V1l[k * V1LD + m] = (k < R && m < R) ? V1[(int64_t)k * p.ldv1 + m] : T(0);
    }
    __syncthreads();
    // wave w: rows 16 w .. 16 w + 15 of U.  All four tiles are computed before the first one is stored (the stores
    // overwrite the wave's own V1 rows), and go straight from the accumulators to LDS.
    Acc u0 = M::zero(), u1 = M::zero(), u2 = M::zero(), u3 = M::zero();
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const T a = V1l[(16 * wave + cl) * V1LD + 4 * ks + g];
      u0 = M::mma(a, V2l[(4 * ks + g) * V2LD + cl], u0);
      u1 = M::mma(a, V2l[(4 * ks + g) * V2LD + 16 + cl], u1);
      u2 = M::mma(a, V2l[(4 * ks + g) * V2LD + 32 + cl], u2);
      u3 = M::mma(a, V2l[(4 * ks + g) * V2LD + 48 + cl], u3);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T* dst = Ul + urow(16 * wave + M::row(lane, r)) + cl;
      dst[0] = u0[r];
      dst[16] = u1[r];
      dst[32] = u2[r];
      dst[48] = u3[r];
    }
  } else {
    __syncthreads();
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int k = idx >> 6, i = idx & 63;
      Ul[urow(k) + i] = V2l[k * V2LD + i];
    }
  }
  __syncthreads();
  if (Lo) {  // left = U diag(sigma), coalesced, from the LDS image
    for (int idx = tid; idx < R * ro; idx += kThreads) {
      const int k = idx / ro, i = idx - k * ro;
      const T u = Ul[urow(k) + i];
      Lo[(int64_t)k * p.ldl + i] = (p.scale_right && sg) ? u * sg[i] : u;
    }
  }
  // ---- main loop: 16 SL columns per step as SL interleaved 16-column slabs (columns c0 + SL i + u): one 4 SL-byte load of M per
  // row and lane (whole 128-byte lines per 16 lanes) and 4 SL-byte stores of the result; SL = 2 (see the end of the kernel).
  T* __restrict__ Ro = p.right + b * p.strideR;
  const bool al2 = ((p.ldm & 1) == 0) && ((p.ldr & 1) == 0) && ((reinterpret_cast<uintptr_t>(Mp) & (2 * sizeof(T) - 1)) == 0) &&
                   ((reinterpret_cast<uintptr_t>(Ro) & (2 * sizeof(T) - 1)) == 0);
  const int Rl = (p.rows32 && p.rows32[b] != 0 && R > 32) ? 32 : R;   // (see rotgram_kernel: zero rows are not loaded)
  // Step order: every item's rows lie ldm elements apart (8 KB at the metric's bonds) and every item is aligned alike, so
  // workgroups that walk their columns in step would keep hitting the same HBM channels (address bits 8 .. 12 are the column's;
  // measured on ttr_orth_fixup, profiles/r05_orth_stamps.txt).  Item b starts at step b mod nsteps and wraps around; the columns
  // are independent of each other, so the result is bit-identical in any order.  (TTR_KNOB_SWEEP_STAGGER = 0: in order.)
  // NK = K steps that carry data (round 6): a `rows32` item (rows 32.. exactly zero: not loaded) used to multiply its 8 zero K steps
  // all the same -- half of the kernel's MFMAs (counters: the matrix pipe 43 % busy on the metric's input); skipped products add
  // a * 0 to their accumulators: bit-identical
  auto main_loop = [&](auto NKC, auto SLC) {
    constexpr int NK = decltype(NKC)::value, SL = decltype(SLC)::value;
    const bool al = al2;
    // the split (nsplit: pick_split) is defined on 32-column chunks; a wave's steps walk its share SL * 16 columns at a time
    int64_t cb, ce;
    split_range((p.n + 31) / 32, p.nsplit, split, cb, ce);
    const int64_t col_b = cb * 32, col_e = ce * 32 < p.n ? ce * 32 : p.n;
    const int64_t nch = (col_e - col_b + 16 * SL - 1) / (16 * SL);
    const int64_t nsteps = nch > wave ? (nch - wave + 3) / 4 : 0;
    const int64_t rot = (p.stagger && nsteps > 1) ? (int64_t)(b % nsteps) : 0;
    for (int64_t sidx = 0; sidx < nsteps; ++sidx) {
      int64_t sq = sidx + rot;
      if (sq >= nsteps) sq -= nsteps;
      const int64_t col = col_b + (wave + 4 * sq) * (16 * SL) + SL * cl;
      const int64_t lim = col_e - col;     // columns of this lane's group inside the split's share
      T bm[SL][NK];
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const int k = 4 * ks + g;
        const Pack<T, SL> x = load_pack<T, SL>(Mp + (int64_t)k * p.ldm + col, al, (k < Rl && lim > 0) ? lim : 0);
#pragma unroll
        for (int u = 0; u < SL; ++u) bm[u][ks] = x.v[u];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < nt) {
          Acc acc[SL];
#pragma unroll
          for (int u = 0; u < SL; ++u) acc[u] = M::zero();
#pragma unroll
          for (int ks = 0; ks < NK; ++ks) {
            const T af = Ul[urow(4 * ks + g) + 16 * t + cl];
#pragma unroll
            for (int u = 0; u < SL; ++u) acc[u] = M::mma(af, bm[u][ks], acc[u]);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + M::row(lane, r);
            if (row < ro && lim > 0) {
              const T sc = isg[row];
              T* dst = Ro + (int64_t)row * p.ldr + col;
              if (al && lim >= SL) {
                typedef T VT __attribute__((ext_vector_type(SL)));
                VT o;
#pragma unroll
                for (int u = 0; u < SL; ++u) o[u] = acc[u][r] * sc;
                *reinterpret_cast<VT*>(dst) = o;
              } else {
#pragma unroll
                for (int u = 0; u < SL; ++u)
                  if (u < lim) dst[u] = acc[u][r] * sc;
              }
            }
          }
        }
      }
    }
  };
  using I2 = std::integral_constant<int, 2>;
  using I8 = std::integral_constant<int, 8>;
  using I16 = std::integral_constant<int, 16>;
  // SL = 4 (16-byte accesses, four interleaved slabs) measured SLOWER and is no longer built: profiles/HISTORY.md, "Retired
  // compile-time variants"
  if (Rl <= 32) {
    main_loop(I8{}, I2{});
  } else {
    main_loop(I16{}, I2{});
  }
}

// ---------------------------------------------------------------- lean builds for `rows32` items (fp32 launches, R = 64)
// The carry of a packed bond has exactly zero rows 32..: on the metric EVERY item of the six large bonds.  The generic kernels
// above skip the zero rows' loads and products, but they are built for 64 rows: 128 registers and 40 KB of LDS, four workgroups
// per CU, one slab (rowgram) or one step (project) of 2 - 4 KB in flight per wave.  These instances hold what a 32-row item
// needs -- <= 64 registers and 12 KB of LDS, eight workgroups per CU -- and compute the same sums in the same order: their results
// are the generic kernels' bit for bit.  Items without the flag return at once; the generic instance serves them in a launch of
// its own (gram_typed, project_typed).  Measured per large bond of the metric (4096 items, profiles/HISTORY.md): rowgram 260 ->
// 244 us, project 460 -> 438 us on average, + 4.4 - 5.3 us for each returning launch.  The Gram kernel takes the same time at 3 .. 8 workgroups
// per CU and with two or three slabs ahead: the ring and the unconditional loads are what it gains from, not the occupancy.
constexpr int kLeanAhead = 3;  // rowgram: slabs requested ahead of the one being multiplied (a ring of kLeanAhead + 1)

template <typename T>
__global__ __launch_bounds__(kThreads, 8) void rowgram_rows32_kernel(SweepArgs<T> p) {
  using M = Mfma<T>;
  using Acc = typename M::Acc;
  __shared__ __attribute__((aligned(16))) T red[4 * 3 * 256];  // per-wave partial tiles (0,0), (0,1), (1,1)
  static_assert(std::is_same<T, float>::value, "slab loads and the write-out below assume the fp32 accumulator layout");
  const int tid = threadIdx.x, lane = tid & 63, cl = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (the step counts below are scalars: plain branches)
  const int64_t b = blockIdx.y;
  if (p.rows32[b] == 0) return;  // (block-uniform)
  const int split = blockIdx.x;
  const T* __restrict__ Mp = p.M + b * p.strideM;
  Acc G[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) G[i] = M::zero();
  // chunks, steps and their order as in rotgram_kernel<T, true>: wave w takes chunks cb + w + 4 sq in ascending sq
  const bool al = ((p.ldm & 3) == 0) && ((reinterpret_cast<uintptr_t>(Mp) & (4 * sizeof(T) - 1)) == 0);
  int64_t cb, ce;
  split_range((p.n + 15) / 16, p.nsplit, split, cb, ce);
  auto gram_update = [&](const Acc (&mw)[2]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) G[0] = M::mma(mw[0][r], mw[0][r], G[0]);
#pragma unroll
    for (int r = 0; r < 4; ++r) G[1] = M::mma(mw[0][r], mw[1][r], G[1]);
#pragma unroll
    for (int r = 0; r < 4; ++r) G[2] = M::mma(mw[1][r], mw[1][r], G[2]);
  };
  const int64_t nsteps = ce > cb + wave ? (ce - cb - wave + 3) / 4 : 0;
  const int64_t rot = (p.stagger >= 2 && nsteps > 1) ? (int64_t)(b % nsteps) : 0;
  auto step_c = [&](int64_t sidx) { int64_t sq = sidx + rot; if (sq >= nsteps) sq -= nsteps; return cb + wave + 4 * sq; };
  // Slab ring: step s lives in slot s mod NS; its loads are issued kLeanAhead steps early, into the slot the previous step has
  // just left.  The loop has no stores and the loads return in order, so every step waits for its own slab only -- provided the
  // compiler can count them: WIDE (aligned rows, whole chunks: the block's share ends inside n) issues every load
  // unconditionally, and the steady state below tests no step index.
  constexpr int NS = kLeanAhead + 1;
  auto run = [&](auto WIDEC) {
    constexpr bool WIDE = decltype(WIDEC)::value;
    auto load_slab = [&](int64_t c, Acc (&mw)[2]) {
      const int64_t col = c * 16 + 4 * g;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const T* src = Mp + (int64_t)(16 * t + cl) * p.ldm + col;
        if constexpr (WIDE) {
          mw[t] = *reinterpret_cast<const Acc*>(src);
        } else {
          const Pack<T, 4> x = load_pack<T, 4>(src, al, p.n - col);
#pragma unroll
          for (int r = 0; r < 4; ++r) mw[t][r] = x.v[r];
        }
      }
    };
    Acc slab[NS][2];
    int64_t s0 = 0;
    if (nsteps >= NS + kLeanAhead) {  // steady state: NS steps per round, as long as each of them has a slab to request
#pragma unroll
      for (int d = 0; d < kLeanAhead; ++d) load_slab(step_c(d), slab[d]);
      do {
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          load_slab(step_c(s0 + u + kLeanAhead), slab[(u + kLeanAhead) % NS]);
          __builtin_amdgcn_sched_barrier(0);  // (the scheduler would gather the ring's loads at the end of the body, behind one wait for all)
          gram_update(slab[u]);
          __builtin_amdgcn_sched_barrier(0);
        }
        s0 += NS;
      } while (s0 + NS + kLeanAhead <= nsteps);
    } else {
#pragma unroll
      for (int d = 0; d < kLeanAhead; ++d)
        if (d < nsteps) load_slab(step_c(d), slab[d]);
    }
    for (; s0 < nsteps; s0 += NS) {
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const int64_t sidx = s0 + u;
        if (sidx < nsteps) {  // (wave-uniform)
          if (sidx + kLeanAhead < nsteps) load_slab(step_c(sidx + kLeanAhead), slab[(u + kLeanAhead) % NS]);
          gram_update(slab[u]);
        }
      }
    }
  };
  if (al && ce * 16 <= p.n) run(std::true_type{});
  else run(std::false_type{});
  // reduce the four waves' partial tiles, (w0 + w1) + (w2 + w3) as in the generic kernel, and write the whole 64 x 64 partial:
  // both triangles of the 32 x 32 block, zeros around it
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * 3 + i) * 256 + lane * 4 + r] = G[i][r];
  __syncthreads();
  T* __restrict__ Gout = p.G + ((int64_t)b * p.nsplit + split) * 64 * 64;
  for (int idx = tid; idx < 64 * 64; idx += kThreads) {
    const int row = idx >> 6, col = idx & 63;
    T v = T(0);
    if (row < 32 && col < 32) {
      // tile (ti, tj), ti <= tj, holds element (i, j) in lane 16 (i / 4) + j, register i mod 4; the lower triangle mirrors (0, 1)
      const bool low = row >= 16 && col < 16;
      const int i = (low ? col : row) & 15, j = (low ? row : col) & 15;
      const int tile = (row >> 4) + (col >> 4);
      const int e = tile * 256 + ((i >> 2) * 16 + j) * 4 + (i & 3);
      v = (red[e] + red[768 + e]) + (red[1536 + e] + red[2304 + e]);
    }
    Gout[idx] = v;
  }
}

constexpr int ULD = 48;  // leading dimension of the lean projection's 32-column image [k][i]: the fragment reads of a wave (16 i x
                         // 4 k: words 48 g + cl) hit 64 different banks

template <typename T>
__global__ __launch_bounds__(kThreads, 8) void project_rows32_kernel(SweepArgs<T> p) {
  using M = Mfma<T>;
  using Acc = typename M::Acc;
  __shared__ __attribute__((aligned(16))) T Wl[64 * ULD];  // V2[:, :ro] as [m][i], zero padded to 32 columns; then U as [k][i]
  __shared__ T isg[32];                                    // as in project_kernel
  static_assert(std::is_same<T, float>::value, "the store addresses below assume the fp32 accumulator layout");
  const int tid = threadIdx.x, lane = tid & 63, cl = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: the step's range test below is a plain branch)
  const int64_t b = blockIdx.y;
  if (p.rows32[b] == 0) return;  // (block-uniform)
  const int split = blockIdx.x;
  const T* __restrict__ Mp = p.M + b * p.strideM;
  const int ro = p.ro;           // <= 32, R = 64 (project_typed)
  const int nt = (ro + 15) / 16;
  const T* __restrict__ V2 = p.V2 + b * p.strideV2;
  const bool flat = p.flat && p.V1 && p.flat[b] != 0;  // (block-uniform, ahead of every load) as in project_kernel
  const T* __restrict__ sg = flat ? p.sigma1 + b * p.stride_sigma1 : (p.sigma ? p.sigma + b * p.stride_sigma : nullptr);
  T* __restrict__ Lo = (p.left && split == 0) ? p.left + b * p.strideL : nullptr;
  // ---- prologue: the sums of project_kernel's in the same order.  V1 is not staged: wave w reads ITS 16 rows straight from global
  // memory as the A operand (lane (g, cl), K step ks <-> V1[16 w + cl][4 ks + g]), and U replaces V2 in the one image.
  // A pass-through item's image is V1[:, :ro] itself.
  if (flat) {
    const T* __restrict__ V1 = p.V1 + b * p.strideV1;
    for (int idx = tid; idx < 64 * 32; idx += kThreads) {
      const int k = idx >> 5, i = idx & 31;
      Wl[k * ULD + i] = (i < ro) ? times_identity(V1[(int64_t)k * p.ldv1 + i]) : T(0);
    }
  } else {
    for (int idx = tid; idx < 64 * 32; idx += kThreads) {
      const int m = idx >> 5, i = idx & 31;
      Wl[m * ULD + i] = (i < ro) ? V2[(int64_t)m * p.ldv2 + i] : T(0);
    }
  }
  if (tid < 32) {
    T sc = T(1);
    if (p.scale_right && sg && tid < ro) {
      const T x = sg[tid];
      sc = (fabs((double)x) < (double)Num<T>::tiny()) ? T(0) : T(1) / x;
    }
    isg[tid] = sc;
  }
  if (p.V1 && !flat) {
    const T* __restrict__ V1 = p.V1 + b * p.strideV1 + (int64_t)(16 * wave + cl) * p.ldv1 + g;
    T a[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) a[ks] = V1[4 * ks];
    __syncthreads();
    Acc u0 = M::zero(), u1 = M::zero();
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      u0 = M::mma(a[ks], Wl[(4 * ks + g) * ULD + cl], u0);
      u1 = M::mma(a[ks], Wl[(4 * ks + g) * ULD + 16 + cl], u1);
    }
    __syncthreads();  // every wave has read V2: U takes its place
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T* dst = Wl + (16 * wave + M::row(lane, r)) * ULD + cl;
      dst[0] = u0[r];
      dst[16] = u1[r];
    }
  }
  __syncthreads();
  if (Lo) {  // left = U diag(sigma): all 64 rows
    for (int idx = tid; idx < 64 * ro; idx += kThreads) {
      const int k = idx / ro, i = idx - k * ro;
      const T u = Wl[k * ULD + i];
      Lo[(int64_t)k * p.ldl + i] = (p.scale_right && sg) ? u * sg[i] : u;
    }
  }
  // ---- main loop: project_kernel's with NK = 8 and SL = 2 (same steps, same stagger, same K order).  Rows 0 .. 31 of U are all
  // it multiplies by: the wave's 16 fragments stay in registers.
  T af[2][8];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) af[t][ks] = Wl[(4 * ks + g) * ULD + 16 * t + cl];
  T* __restrict__ Ro = p.right + b * p.strideR;
  const bool al = ((p.ldm & 1) == 0) && ((p.ldr & 1) == 0) && ((reinterpret_cast<uintptr_t>(Mp) & (2 * sizeof(T) - 1)) == 0) &&
                  ((reinterpret_cast<uintptr_t>(Ro) & (2 * sizeof(T) - 1)) == 0);
  int64_t cb, ce;
  split_range((p.n + 31) / 32, p.nsplit, split, cb, ce);
  const int64_t col_b = cb * 32, col_e = ce * 32 < p.n ? ce * 32 : p.n;
  const int64_t nch = (col_e - col_b + 31) / 32;
  const int64_t nsteps = nch > wave ? (nch - wave + 3) / 4 : 0;
  const int64_t rot = (p.stagger && nsteps > 1) ? (int64_t)(b % nsteps) : 0;
  // (addresses: the lane's part g ldm + col / 4 g ldr + col once per step, its column behind an empty asm so that the compiler adds
  // the wave-uniform row offsets per access instead of keeping sixteen 64-bit row pointers -- they do not fit 64 registers)
  const T* __restrict__ Mg = Mp + (int64_t)g * p.ldm;
  T* __restrict__ Rg = Ro + (int64_t)M::row(lane, 0) * p.ldr;
  // WHOLE: aligned rows and the wave's 32 columns all inside the share -- every access of the step is unconditional.  (With the
  // guarded accesses of load_pack in the one path the compiler, short of registers, waits for each load before the next.)
  typedef T VT __attribute__((ext_vector_type(2)));
  auto step = [&](auto WHOLEC, const T* mk, T* rk, int64_t lim) {
    constexpr bool WHOLE = decltype(WHOLEC)::value;
    T bm[2][8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const T* src = mk + (int64_t)(4 * ks) * p.ldm;
      if constexpr (WHOLE) {
        const VT x = *reinterpret_cast<const VT*>(src);
        bm[0][ks] = x[0];
        bm[1][ks] = x[1];
      } else {
        const Pack<T, 2> x = load_pack<T, 2>(src, al, lim > 0 ? lim : 0);
        bm[0][ks] = x.v[0];
        bm[1][ks] = x.v[1];
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t < nt) {
        Acc acc[2] = {M::zero(), M::zero()};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
          for (int u = 0; u < 2; ++u) acc[u] = M::mma(af[t][ks], bm[u][ks], acc[u]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * t + M::row(lane, r);
          if (row < ro && (WHOLE || lim > 0)) {
            const T sc = isg[row];
            T* dst = rk + (int64_t)(16 * t + r) * p.ldr;  // (fp32 layout: M::row(lane, r) = M::row(lane, 0) + r -- a scalar offset)
            if (WHOLE || (al && lim >= 2)) {
              VT o;
              o[0] = acc[0][r] * sc;
              o[1] = acc[1][r] * sc;
              *reinterpret_cast<VT*>(dst) = o;
            } else {
              dst[0] = acc[0][r] * sc;
              if (lim > 1) dst[1] = acc[1][r] * sc;
            }
          }
        }
      }
    }
  };
  for (int64_t sidx = 0; sidx < nsteps; ++sidx) {
    int64_t sq = sidx + rot;
    if (sq >= nsteps) sq -= nsteps;
    const int64_t cw = col_b + (wave + 4 * sq) * 32;  // (wave-uniform) the step's first column
    int64_t col = cw + 2 * cl;
    asm volatile("" : "+v"(col));
    const T* mk = Mg + col;
    T* rk = Rg + col;
    if (al && cw + 32 <= col_e) step(std::true_type{}, mk, rk, 2);
    else step(std::false_type{}, mk, rk, col_e - col);  // (columns of the lane's pair inside the split's share)
  }
}


// ================================================================ tall matrices (dense TT-SVD steps): M is rows x n, n <= 64
// The first (largest) step of a dense right-to-left TT-SVD truncates a (prod I_1..I_{N-1}) x I_N unfolding: millions of
// rows, at most 64 columns, and the whole input tensor in bytes.  Same register technique with the roles of rows and
// columns exchanged -- the contraction runs over the ROWS, 16 per wave and step:
//   ttr_colgram    G = M^T M                (ROT = false: the 16 x 16 pieces of M are loaded straight into the accumulator
//                                            layout, 64-byte row segments) or G = (M V1)^T (M V1) (ROT = true: the rotated
//                                            16-row slab is an MFMA product whose A operand is read with 16-byte loads)
//   ttr_colproject left = M U [diag(1/sigma)]  (rows x ro),  right = [diag(sigma)] U^T (ro x n),  U = V1 V2[:, :ro]
// 'svd' therefore reads the tensor three times and writes only the carry (ro / n of its size) -- no rotated copy.
constexpr int CLD = 68;  // LDS images [k][j] read with k = 16 kk + 4 g + u: 4 * 68 = 16 mod 32 -> the two lane rows of a
                         // 32-lane group hit disjoint banks

template <typename T>
struct ColArgs {
  int64_t rows;
  int n;
  const T* M;
  int64_t ldm, strideM;
  const T* V1;
  int64_t ldv1, strideV1;
  T* G;        // [batch][nsplit][n][n]
  int nsplit;
  const int32_t* skip;  // optional [batch]: != 0 -> the item's workgroups return at once (colgram; see ttr_spectrum_flat)
  const T* V2;
  int64_t ldv2, strideV2;
  const T* sigma;
  int64_t stride_sigma;
  int ro;
  int left_ortho;  // 1: left columns divided by sigma, right rows multiplied (round.py:173-178); 0: plain (round.py:179-182)
  T* left;
  int64_t ldl, strideL;
  T* right;
  int64_t ldr, strideR;
};

template <typename T, bool ROT>
__global__ __launch_bounds__(kThreads, (sizeof(T) == 4 ? (ROT ? 3 : 4) : 1)) void colgram_kernel(ColArgs<T> p) {
  using M = Mfma<T>;
  using Acc = typename M::Acc;
  constexpr int RED = 4 * 10 * 256;
  constexpr int VSZ = 64 * CLD;
  __shared__ __attribute__((aligned(16))) T smem[RED > VSZ ? RED : VSZ];
  T* Vl = smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.y;
  if (p.skip && p.skip[b] != 0) return;
  const int split = blockIdx.x;
  const T* __restrict__ Mp = p.M + b * p.strideM;
  const int n = p.n;
  if constexpr (ROT) {
    const T* __restrict__ V1 = p.V1 + b * p.strideV1;
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int k = idx >> 6, j = idx & 63;
      Vl[k * CLD + j] = (k < n && j < n) ? V1[(int64_t)k * p.ldv1 + j] : T(0);
    }
    __syncthreads();
  }
  Acc G[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) G[i] = M::zero();
  int64_t cb, ce;
  split_range((p.rows + 15) / 16, p.nsplit, split, cb, ce);
  const bool al = ((p.ldm & 3) == 0) && ((reinterpret_cast<uintptr_t>(Mp) & (4 * sizeof(T) - 1)) == 0);
  const int ntl = (n + 15) >> 4;  // column tiles that exist: the Gram tiles beyond them are zero (n = 32: 3 of the 10 tile pairs)
  auto gram_update = [&](const Acc (&mw)[4]) {
    int idx = 0;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = ti; tj < 4; ++tj) {
        if (tj < ntl) {  // (wave-uniform)
#pragma unroll
          for (int r = 0; r < 4; ++r) G[idx] = M::mma(mw[ti][r], mw[tj][r], G[idx]);
        }
        ++idx;
      }
  };
  if constexpr (!ROT) {
    // lane (g, cl), register r <-> M[r0 + 4 g + r][16 t + cl]; the next slab's loads are issued before this slab's MFMAs (the
    // loop has no stores: the loads of two slabs per wave are in flight -- four workgroups per CU do not cover an HBM round trip)
    auto load_slab = [&](int64_t c, Acc (&mw)[4]) {
      const int64_t r0 = c * 16;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = r0 + 4 * g + r;
          const int col = 16 * t + cl;
          mw[t][r] = (row < p.rows && col < n) ? Mp[row * p.ldm + col] : T(0);
        }
    };
    if (ntl <= 2) {  // (measured: at n = 32 the prefetch gives 2.6 -> 4.4 TB/s together with the tile skip; at n = 64 it costs 7 %)
      Acc cur[4], nxt[4];
      int64_t c = cb + wave;
      if (c < ce) load_slab(c, cur);
      for (; c < ce; c += 4) {
        const bool more = c + 4 < ce;
        if (more) load_slab(c + 4, nxt);
        gram_update(cur);
        if (more) {
#pragma unroll
          for (int t = 0; t < 4; ++t) cur[t] = nxt[t];
        }
      }
    } else {
      for (int64_t c = cb + wave; c < ce; c += 4) {
        Acc mw[4];
        load_slab(c, mw);
        gram_update(mw);
      }
    }
  } else {
    for (int64_t c = cb + wave; c < ce; c += 4) {
      const int64_t r0 = c * 16;
      Acc mw[4];
      // A operand: lane (i = cl, g) holds M[r0 + cl][16 kk + 4 g + u]; K step (kk, u) <-> k = 16 kk + 4 g + u
      T a[4][4];
      const int64_t row = r0 + cl;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int col = 16 * kk + 4 * g;
        const Pack<T, 4> x = load_pack<T, 4>(Mp + row * p.ldm + col, al, row < p.rows ? n - col : 0);
#pragma unroll
        for (int u = 0; u < 4; ++u) a[kk][u] = x.v[u];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        mw[t] = M::zero();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int u = 0; u < 4; ++u) mw[t] = M::mma(a[kk][u], Vl[(16 * kk + 4 * g + u) * CLD + 16 * t + cl], mw[t]);
      }
      gram_update(mw);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) smem[(wave * 10 + i) * 256 + lane * 4 + r] = G[i][r];
  __syncthreads();
  T* __restrict__ Gout = p.G + ((int64_t)b * p.nsplit + split) * n * n;
  for (int idx = tid; idx < 10 * 256; idx += kThreads) {
    const int tile = idx >> 8, e = idx & 255, ln = e >> 2, r = e & 3;
    const T v = (smem[idx] + smem[2560 + idx]) + (smem[5120 + idx] + smem[7680 + idx]);
    int ti = 0, rem = tile;
    while (rem >= 4 - ti) { rem -= 4 - ti; ++ti; }
    const int tj = ti + rem;
    const int row = 16 * ti + M::row(ln, r), col = 16 * tj + (ln & 15);
    if (row < n && col < n) {
      Gout[row * n + col] = v;
      if (ti != tj) Gout[col * n + row] = v;
    }
  }
}

// out[b][e] = sum_p in[b][p][e]  (fixed order: deterministic).  skip[b] != 0 (colgram_kernel's flags, same item numbering): the item's
// partials were never written -- they are not read, and out[b] is not written
template <typename T>
__global__ __launch_bounds__(kThreads) void sum_parts_kernel(const T* __restrict__ in, T* __restrict__ out, int parts, int64_t count,
                                                             const int32_t* __restrict__ skip) {
  const int64_t b = blockIdx.y;
  if (skip && skip[b] != 0) return;  // (block-uniform)
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < count; e += (int64_t)gridDim.x * kThreads) {
    T s = T(0);
    for (int q = 0; q < parts; ++q) s += in[((int64_t)b * parts + q) * count + e];
    out[b * count + e] = s;
  }
}

// HASV1 = false (U = V2[:, :ro] given: no prologue product): the kernel keeps 17 KB of LDS instead of 55 KB -- six workgroups per
// CU instead of two.  Its main loop cannot prefetch (the step's stores sit between the loads and their use in one in-order
// counter, see project_kernel), so the HBM round trip is covered by resident waves alone; the host shim forms U with one small
// GEMM for tall inputs.
template <typename T, bool HASV1>
__global__ __launch_bounds__(kThreads) void colproject_kernel(ColArgs<T> p) {
  using M = Mfma<T>;
  using Acc = typename M::Acc;
  constexpr int V1LD = 66;
  __shared__ __attribute__((aligned(16))) T V2l[HASV1 ? 64 * KLD : 4];   // V2[:, :ro] as [m][i] (prologue only)
  __shared__ __attribute__((aligned(16))) T V1l[HASV1 ? 64 * V1LD : 4];  // V1 as [k][m] (prologue only)
  __shared__ __attribute__((aligned(16))) T Ul[64 * CLD];    // U = V1 V2[:, :ro] as [k][i], zero padded
  __shared__ T csc[64];                                      // column scale of left (1 / sigma or 1)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.y;
  const int split = blockIdx.x;
  const T* __restrict__ Mp = p.M + b * p.strideM;
  const int n = p.n, ro = p.ro;
  const int nt = (ro + 15) / 16;
  const T* __restrict__ V2 = p.V2 + b * p.strideV2;
  const T* __restrict__ sg = p.sigma ? p.sigma + b * p.stride_sigma : nullptr;
  T* __restrict__ Rt = (p.right && split == 0) ? p.right + b * p.strideR : nullptr;
  if constexpr (HASV1) {
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int m = idx >> 6, i = idx & 63;
      V2l[m * KLD + i] = (m < n && i < ro) ? V2[(int64_t)m * p.ldv2 + i] : T(0);
    }
    const T* __restrict__ V1 = p.V1 + b * p.strideV1;
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int k = idx >> 6, m = idx & 63;
      V1l[k * V1LD + m] = (k < n && m < n) ? V1[(int64_t)k * p.ldv1 + m] : T(0);
    }
  } else {
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int k = idx >> 6, i = idx & 63;
      Ul[k * CLD + i] = (k < n && i < ro) ? V2[(int64_t)k * p.ldv2 + i] : T(0);
    }
  }
  if (tid < 64) {
    T sc = T(1);
    if (p.left_ortho && sg && tid < ro) {
      const T x = sg[tid];
      sc = (fabs((double)x) < (double)Num<T>::tiny()) ? T(0) : T(1) / x;
    }
    csc[tid] = sc;
  }
  __syncthreads();
  if constexpr (HASV1) {  // wave w: rows 16 w .. 16 w + 15 of U, straight from the accumulators to LDS
    Acc u0 = M::zero(), u1 = M::zero(), u2 = M::zero(), u3 = M::zero();
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const T a = V1l[(16 * wave + cl) * V1LD + 4 * ks + g];
      u0 = M::mma(a, V2l[(4 * ks + g) * KLD + cl], u0);
      u1 = M::mma(a, V2l[(4 * ks + g) * KLD + 16 + cl], u1);
      u2 = M::mma(a, V2l[(4 * ks + g) * KLD + 32 + cl], u2);
      u3 = M::mma(a, V2l[(4 * ks + g) * KLD + 48 + cl], u3);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T* dst = Ul + (16 * wave + M::row(lane, r)) * CLD + cl;
      dst[0] = u0[r];
      dst[16] = u1[r];
      dst[32] = u2[r];
      dst[48] = u3[r];
    }
    __syncthreads();
  }
  if (Rt) {  // right = [diag(sigma)] U^T, coalesced, from the LDS image
    for (int idx = tid; idx < ro * n; idx += kThreads) {
      const int i = idx / n, k = idx - i * n;
      const T u = Ul[k * CLD + i];
      Rt[(int64_t)i * p.ldr + k] = (p.left_ortho && sg) ? u * sg[i] : u;
    }
  }
  T* __restrict__ Lo = p.left + b * p.strideL;
  const bool al = ((p.ldm & 3) == 0) && ((reinterpret_cast<uintptr_t>(Mp) & (4 * sizeof(T) - 1)) == 0);
  int64_t cb, ce;
  split_range((p.rows + 15) / 16, p.nsplit, split, cb, ce);
  for (int64_t c = cb + wave; c < ce; c += 4) {
    const int64_t r0 = c * 16;
    T a[4][4];
    const int64_t row = r0 + cl;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int col = 16 * kk + 4 * g;
      const Pack<T, 4> x = load_pack<T, 4>(Mp + row * p.ldm + col, al, row < p.rows ? n - col : 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) a[kk][u] = x.v[u];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nt) {
        Acc acc = M::zero();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int u = 0; u < 4; ++u) acc = M::mma(a[kk][u], Ul[(16 * kk + 4 * g + u) * CLD + 16 * t + cl], acc);
        const int col = 16 * t + cl;
        const T sc = csc[col < 64 ? col : 0];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t orow = r0 + M::row(lane, r);
          if (orow < p.rows && col < ro) Lo[orow * p.ldl + col] = acc[r] * sc;
        }
      }
    }
  }
}

static int col_split(int64_t rows, int64_t batch) {
  const int64_t chunks = (rows + 15) / 16;
  int64_t want = (4096 + batch - 1) / batch;
  int64_t maxs = chunks / 16;  // >= 4 steps per wave
  if (maxs < 1) maxs = 1;
  int64_t s = want < maxs ? want : maxs;
  if (s > 4096) s = 4096;
  return (int)(s < 1 ? 1 : s);
}

int64_t colgram_workspace_bytes(int dtype, int64_t rows, int64_t n, int64_t batch) {
  const int sp = col_split(rows, batch);
  return sp > 1 ? (int64_t)sp * batch * n * n * (dtype == TTR_F64 ? 8 : 4) : 0;
}

template <typename T>
static int colgram_typed(int64_t rows, int64_t n, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM,
                         const void* V1, int64_t ldv1, int64_t strideV1, void* G, void* ws, int64_t ws_bytes,
                         hipStream_t stream, const int32_t* skip) {
  const int sp = col_split(rows, batch);
  TTR_REQUIRE(sp == 1 || (ws && ws_bytes >= (int64_t)sp * batch * n * n * (int64_t)sizeof(T)), TTR_E_WORKSPACE,
              "ttr_colgram: workspace too small");
  ColArgs<T> p{};
  p.rows = rows; p.n = (int)n; p.M = (const T*)Mx; p.ldm = ldm; p.strideM = strideM;
  p.V1 = (const T*)V1; p.ldv1 = ldv1; p.strideV1 = strideV1;
  p.G = sp == 1 ? (T*)G : (T*)ws; p.nsplit = sp;
  ProfScope prof(V1 ? TTR_PROF_ROTGRAM : TTR_PROF_ROWGRAM, stream);
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    ColArgs<T> q = p;
    q.M = p.M + b0 * strideM;
    if (V1) q.V1 = p.V1 + b0 * strideV1;
    q.G = p.G + b0 * sp * n * n;
    q.skip = skip ? skip + b0 : nullptr;
    const dim3 grid((unsigned)sp, (unsigned)nb);
    if (V1) hipLaunchKernelGGL((colgram_kernel<T, true>), grid, dim3(kThreads), 0, stream, q);
    else hipLaunchKernelGGL((colgram_kernel<T, false>), grid, dim3(kThreads), 0, stream, q);
    if (sp > 1) {
      int64_t gx = ceil_div(n * n, kThreads);
      hipLaunchKernelGGL(sum_parts_kernel<T>, dim3((unsigned)gx, (unsigned)nb), dim3(kThreads), 0, stream,
                         (const T*)q.G, (T*)G + b0 * n * n, sp, n * n, q.skip);
    }
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int colgram_dispatch(int dtype, int64_t rows, int64_t n, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM,
                     const void* V1, int64_t ldv1, int64_t strideV1, void* G, void* ws, int64_t ws_bytes, hipStream_t stream,
                     const int32_t* skip) {
  TTR_REQUIRE(n >= 1 && n <= 64, TTR_E_UNSUPPORTED, "ttr_colgram: %lld columns (the fused kernels hold <= 64)", (long long)n);
  if (dtype == TTR_F32) return colgram_typed<float>(rows, n, batch, Mx, ldm, strideM, V1, ldv1, strideV1, G, ws, ws_bytes, stream, skip);
  return colgram_typed<double>(rows, n, batch, Mx, ldm, strideM, V1, ldv1, strideV1, G, ws, ws_bytes, stream, skip);
}

template <typename T>
static int colproject_typed(int64_t rows, int64_t n, int64_t ro, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM,
                            const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2, int64_t strideV2,
                            const void* sigma, int64_t stride_sigma, int left_ortho, void* left, int64_t ldl,
                            int64_t strideL, void* right, int64_t ldr, int64_t strideR, hipStream_t stream) {
  ColArgs<T> p{};
  p.rows = rows; p.n = (int)n; p.M = (const T*)Mx; p.ldm = ldm; p.strideM = strideM;
  p.V1 = (const T*)V1; p.ldv1 = ldv1; p.strideV1 = strideV1;
  p.V2 = (const T*)V2; p.ldv2 = ldv2; p.strideV2 = strideV2;
  p.sigma = (const T*)sigma; p.stride_sigma = stride_sigma; p.ro = (int)ro; p.left_ortho = left_ortho;
  p.left = (T*)left; p.ldl = ldl; p.strideL = strideL;
  p.right = (T*)right; p.ldr = ldr; p.strideR = strideR;
  p.nsplit = col_split(rows, batch);
  ProfScope prof(TTR_PROF_PROJECT, stream);
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    ColArgs<T> q = p;
    q.M = p.M + b0 * strideM;
    if (V1) q.V1 = p.V1 + b0 * strideV1;
    q.V2 = p.V2 + b0 * strideV2;
    if (sigma) q.sigma = p.sigma + b0 * stride_sigma;
    q.left = p.left + b0 * strideL;
    if (right) q.right = p.right + b0 * strideR;
    if (q.V1) hipLaunchKernelGGL((colproject_kernel<T, true>), dim3((unsigned)p.nsplit, (unsigned)nb), dim3(kThreads), 0, stream, q);
    else hipLaunchKernelGGL((colproject_kernel<T, false>), dim3((unsigned)p.nsplit, (unsigned)nb), dim3(kThreads), 0, stream, q);
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int colproject_dispatch(int dtype, int64_t rows, int64_t n, int64_t ro, int64_t batch, const void* Mx, int64_t ldm,
                        int64_t strideM, const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2,
                        int64_t strideV2, const void* sigma, int64_t stride_sigma, int left_ortho, void* left, int64_t ldl,
                        int64_t strideL, void* right, int64_t ldr, int64_t strideR, hipStream_t stream) {
  TTR_REQUIRE(n >= 1 && n <= 64 && ro >= 1 && ro <= n, TTR_E_UNSUPPORTED,
              "ttr_colproject: %lld columns / %lld kept (the fused kernel holds <= 64 columns)", (long long)n, (long long)ro);
  if (dtype == TTR_F32)
    return colproject_typed<float>(rows, n, ro, batch, Mx, ldm, strideM, V1, ldv1, strideV1, V2, ldv2, strideV2, sigma,
                                   stride_sigma, left_ortho, left, ldl, strideL, right, ldr, strideR, stream);
  return colproject_typed<double>(rows, n, ro, batch, Mx, ldm, strideM, V1, ldv1, strideV1, V2, ldv2, strideV2, sigma,
                                  stride_sigma, left_ortho, left, ldl, strideL, right, ldr, strideR, stream);
}

int g_sweep_stagger = 1;   // ttr_debug_set_knob(TTR_KNOB_SWEEP_STAGGER)
int g_sweep_lean = 1;      // ttr_debug_set_knob(TTR_KNOB_SWEEP_LEAN)
int g_flat_pass = 1;       // ttr_debug_set_knob(TTR_KNOB_FLAT_PASS): 0 = pass-through items take the identity round trip (A/B)
// launches of fewer items run the generic instance alone (latency-bound sizes: a second launch costs more than the build gains)
constexpr int64_t kLeanMinItems = 256;

static int pick_split(int64_t n, int64_t batch) {
  const int64_t chunks = (n + 31) / 32;        // (the projection walks 32 columns per step and wave)
  int64_t want = (2048 + batch - 1) / batch;  // aim at >= 2048 workgroups on the 256 CUs ...
  int64_t maxs = chunks / 8;                  // ... but keep >= 2 steps per wave
  if (maxs < 1) maxs = 1;
  int64_t s = want < maxs ? want : maxs;
  if (s > 64) s = 64;
  return (int)(s < 1 ? 1 : s);
}

int sweep_gram_parts(int64_t n, int64_t batch) { return pick_split(n, batch); }

template <typename T>
static int gram_typed(int64_t R, int64_t n, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM, const void* V1,
                      int64_t ldv1, int64_t strideV1, void* G, int64_t nsplit, hipStream_t stream, const int32_t* skip,
                      const int32_t* rows32) {
  SweepArgs<T> p{};
  p.skip = skip;
  p.rows32 = rows32;
  p.R = (int)R; p.n = n; p.M = (const T*)Mx; p.ldm = ldm; p.strideM = strideM;
  p.V1 = (const T*)V1; p.ldv1 = ldv1; p.strideV1 = strideV1;
  p.G = (T*)G; p.nsplit = (int)nsplit;
  p.stagger = g_sweep_stagger;
  if (work_census_on()) {
    // executed work per item: rows32 items load / multiply 32 of the R rows; pass-through items (skip) of the rotated pass do
    // nothing.  Gram: 10 of the 16 tiles (symmetry); rotation V1^T M: R x Reff x n.
    const double s = (double)sizeof(T), sym = 10.0 / 16.0;
    auto gr = [&](double Re) { return 2.0 * Re * Re * (double)n * sym + (V1 ? 2.0 * (double)R * Re * (double)n : 0.0); };
    const double fl[4] = {gr((double)R), gr(R > 32 ? 32.0 : (double)R), 0.0, 0.0};
    const double by[4] = {s * R * (double)n, s * (R > 32 ? 32.0 : (double)R) * (double)n, 0.0, 0.0};
    work_items(V1 ? TTR_PROF_ROTGRAM : TTR_PROF_ROWGRAM, rows32, skip, batch, fl, by, stream);
  }
  ProfScope prof(V1 ? TTR_PROF_ROTGRAM : TTR_PROF_ROWGRAM, stream);
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    SweepArgs<T> q = p;
    q.M = p.M + b0 * strideM;
    if (V1) q.V1 = p.V1 + b0 * strideV1;
    q.G = p.G + b0 * nsplit * R * R;
    if (skip) q.skip = skip + b0;
    if (rows32) q.rows32 = rows32 + b0;
    const dim3 grid((unsigned)nsplit, (unsigned)nb);
    if constexpr (std::is_same<T, float>::value) {
      // two instances (TTR_KNOB_SWEEP_LEAN; the pattern of QrLevel::live_half): the lean build takes the `rows32` items, and the
      // generic one sees their flags as its `skip` flags
      if (g_sweep_lean && !V1 && !skip && rows32 && R == 64 && nb >= kLeanMinItems) {
        hipLaunchKernelGGL(rowgram_rows32_kernel<T>, grid, dim3(kThreads), 0, stream, q);
        q.skip = q.rows32;
      }
    }
    if (V1) hipLaunchKernelGGL((rotgram_kernel<T, false>), grid, dim3(kThreads), 0, stream, q);
    else hipLaunchKernelGGL((rotgram_kernel<T, true>), grid, dim3(kThreads), 0, stream, q);
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int sweep_gram_dispatch(int dtype, int64_t R, int64_t n, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM,
                        const void* V1, int64_t ldv1, int64_t strideV1, void* G, int64_t nsplit, hipStream_t stream,
                        const int32_t* skip, const int32_t* rows32) {
  TTR_REQUIRE(R >= 1 && R <= 64, TTR_E_UNSUPPORTED, "ttr_rowgram / ttr_rotgram: %lld rows (the fused kernels hold <= 64)",
              (long long)R);
  TTR_REQUIRE(nsplit >= 1 && nsplit <= 65535, TTR_E_INVALID, "ttr_rowgram / ttr_rotgram: bad split %lld", (long long)nsplit);
  if (dtype == TTR_F32) return gram_typed<float>(R, n, batch, Mx, ldm, strideM, V1, ldv1, strideV1, G, nsplit, stream, skip, rows32);
  return gram_typed<double>(R, n, batch, Mx, ldm, strideM, V1, ldv1, strideV1, G, nsplit, stream, skip, rows32);
}

template <typename T>
static int project_typed(int64_t R, int64_t n, int64_t ro, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM,
                         const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2, int64_t strideV2,
                         const void* sigma, int64_t stride_sigma, int scale_right, void* right, int64_t ldr,
                         int64_t strideR, void* left, int64_t ldl, int64_t strideL, hipStream_t stream, const int32_t* rows32,
                         const int32_t* flat, const void* sigma1, int64_t stride_sigma1) {
  SweepArgs<T> p{};
  p.rows32 = rows32;
  if (g_flat_pass && flat && V1) {   // (TTR_KNOB_FLAT_PASS = 0: the flags are ignored -- every item loads its V2 and sigma)
    p.flat = flat; p.sigma1 = (const T*)sigma1; p.stride_sigma1 = stride_sigma1;
  }
  p.R = (int)R; p.n = n; p.M = (const T*)Mx; p.ldm = ldm; p.strideM = strideM;
  p.V1 = (const T*)V1; p.ldv1 = ldv1; p.strideV1 = strideV1;
  p.V2 = (const T*)V2; p.ldv2 = ldv2; p.strideV2 = strideV2;
  p.sigma = (const T*)sigma; p.stride_sigma = stride_sigma; p.ro = (int)ro; p.scale_right = scale_right;
  p.right = (T*)right; p.ldr = ldr; p.strideR = strideR;
  p.left = (T*)left; p.ldl = ldl; p.strideL = strideL;
  p.nsplit = pick_split(n, batch);
  p.stagger = g_sweep_stagger;
  if (work_census_on()) {   // right = U^T M: ro x Reff x n; reads Reff rows, writes ro rows
    const double s = (double)sizeof(T), Re = R > 32 ? 32.0 : (double)R;
    const double fl[4] = {2.0 * R * (double)ro * (double)n, 2.0 * Re * (double)ro * (double)n, 0.0, 0.0};
    const double by[4] = {s * (R + ro) * (double)n, s * (Re + ro) * (double)n, 0.0, 0.0};
    work_items(TTR_PROF_PROJECT, rows32, nullptr, batch, fl, by, stream);
  }
  ProfScope prof(TTR_PROF_PROJECT, stream);
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    SweepArgs<T> q = p;
    q.M = p.M + b0 * strideM;
    if (V1) q.V1 = p.V1 + b0 * strideV1;
    q.V2 = p.V2 + b0 * strideV2;
    if (sigma) q.sigma = p.sigma + b0 * stride_sigma;
    q.right = p.right + b0 * strideR;
    if (left) q.left = p.left + b0 * strideL;
    if (rows32) q.rows32 = rows32 + b0;
    if (p.flat) { q.flat = p.flat + b0; q.sigma1 = p.sigma1 + b0 * stride_sigma1; }
    const dim3 grid((unsigned)p.nsplit, (unsigned)nb);
    bool two = false;
    if constexpr (std::is_same<T, float>::value) {   // two instances, as in gram_typed
      two = g_sweep_lean && rows32 && R == 64 && ro <= 32 && nb >= kLeanMinItems;
      if (two) {
        hipLaunchKernelGGL(project_rows32_kernel<T>, grid, dim3(kThreads), 0, stream, q);
        hipLaunchKernelGGL((project_kernel<T, true>), grid, dim3(kThreads), 0, stream, q);
      }
    }
    if (!two) hipLaunchKernelGGL((project_kernel<T, false>), grid, dim3(kThreads), 0, stream, q);
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int sweep_project_dispatch(int dtype, int64_t R, int64_t n, int64_t ro, int64_t batch, const void* Mx, int64_t ldm,
                           int64_t strideM, const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2,
                           int64_t strideV2, const void* sigma, int64_t stride_sigma, int scale_right, void* right,
                           int64_t ldr, int64_t strideR, void* left, int64_t ldl, int64_t strideL, hipStream_t stream,
                           const int32_t* rows32, const int32_t* flat, const void* sigma1, int64_t stride_sigma1) {
  TTR_REQUIRE(R >= 1 && R <= 64 && ro >= 1 && ro <= R, TTR_E_UNSUPPORTED,
              "ttr_project: %lld rows / %lld kept (the fused kernel holds <= 64 rows)", (long long)R, (long long)ro);
  if (dtype == TTR_F32)
    return project_typed<float>(R, n, ro, batch, Mx, ldm, strideM, V1, ldv1, strideV1, V2, ldv2, strideV2, sigma,
                                stride_sigma, scale_right, right, ldr, strideR, left, ldl, strideL, stream, rows32, flat, sigma1,
                                stride_sigma1);
  return project_typed<double>(R, n, ro, batch, Mx, ldm, strideM, V1, ldv1, strideV1, V2, ldv2, strideV2, sigma,
                               stride_sigma, scale_right, right, ldr, strideR, left, ldl, strideL, stream, rows32, flat, sigma1,
                                stride_sigma1);
}

}  // namespace ttr
