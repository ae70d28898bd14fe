// ttr_orth_fixup: orthonormal completion of the kept directions of a truncation whose singular value lies below the resolution
// of the input -- what the V of a LAPACK SVD gives the reference for free (round.py:96).  Three forms, chosen by the entry at the
// end of this file; all of them leave live vectors untouched, keep genuine remainders and replace a vector whose remainder
// collapses by a hashed pseudo-random one:
//   orth_fixup_kernel         more than 64 vectors: one 256-thread block per item, modified Gram-Schmidt vector by vector (twice)
//   orth_fixup_block_kernel   up to 64 vectors: one block per item and launch; per round the Gram matrix on MFMA 16x16x4 (column
//                             chunks of 256 / 128 through dynamic LDS, orth_fixup_lds_bytes), Gram-Schmidt of the dead rows in
//                             coefficient space (double, LDS), X_dead <- W X on MFMA
//   orth_init / orth_coef / orth_apply_kernel   the same rounds as three launches for batches that fill the chip
//                             (TTR_KNOB_ORTH_SPLIT, orth_split_ok); the Gram matrix comes from ttr_sweep.hip's rowgram kernel, grid
//                             of the apply launch: (column splits, items); workspace layout: orth_split_layout
// Every global index is bounded by r (vectors), n (elements) and the batch, all validated by the entry; the LDS images are sized
// for the launch's r rounded up to whole 16 x 16 tiles.
#include "detail/ttr_internal.h"

namespace ttr {

// One workgroup per batch item; see ttr_orth_fixup in the header.
template <typename T>
__global__ __launch_bounds__(kThreads) void orth_fixup_kernel(int r, int64_t n, T* __restrict__ X, int64_t vs, int64_t es,
                                                              int64_t strideX, const T* __restrict__ sigma,
                                                              int64_t stride_sigma, double dead_rel,
                                                              const int32_t* __restrict__ rank_dev) {
  __shared__ double red[kThreads / kWave];
  const int64_t b = blockIdx.x;
  if (rank_dev) r = rank_dev[b] < r ? rank_dev[b] : r;  // vectors beyond the selected rank are cut away by the caller later
  const T* __restrict__ sg = sigma + b * stride_sigma;
  const double s0 = (double)sg[0];
  int first = r;
  for (int i = 0; i < r; ++i)
    if (!((double)sg[i] > dead_rel * s0)) { first = i; break; }  // (also catches NaN / zero sigma_0)
  if (first >= r) return;
  T* __restrict__ Xb = X + b * strideX;
  const int tid = threadIdx.x;
  for (int i = first; i < r; ++i) {
    T* __restrict__ xi = Xb + (int64_t)i * vs;
    for (int attempt = 0; attempt < 3; ++attempt) {
      double n0 = 0.0;
      for (int64_t k = tid; k < n; k += kThreads) { const double v = (double)xi[k * es]; n0 += v * v; }
      n0 = block_sum(n0, red);
      bool regenerate = !(n0 > 0.0) || !(n0 < 1e300);
      if (!regenerate) {
        for (int pass = 0; pass < 2; ++pass)
          for (int j = 0; j < i; ++j) {  // modified Gram-Schmidt against every finished vector
            const T* __restrict__ xj = Xb + (int64_t)j * vs;
            double d = 0.0;
            for (int64_t k = tid; k < n; k += kThreads) d += (double)xj[k * es] * (double)xi[k * es];
            d = block_sum(d, red);
            for (int64_t k = tid; k < n; k += kThreads) xi[k * es] = (T)((double)xi[k * es] - d * (double)xj[k * es]);
          }
        double n1 = 0.0;
        for (int64_t k = tid; k < n; k += kThreads) { const double v = (double)xi[k * es]; n1 += v * v; }
        n1 = block_sum(n1, red);
        if (n1 > 1e-6 * n0) {  // a genuine remainder: normalise and go on
          const double inv = 1.0 / sqrt(n1);
          for (int64_t k = tid; k < n; k += kThreads) xi[k * es] = (T)((double)xi[k * es] * inv);
          break;
        }
        regenerate = true;  // the vector lay in the span of the previous ones
      }
      if (regenerate) {  // hashed pseudo-random replacement (deterministic), orthogonalised by the next attempt
        for (int64_t k = tid; k < n; k += kThreads) {
          uint32_t h = (uint32_t)(k * 2654435761u) ^ (uint32_t)((i + 1) * 40503u) ^ (uint32_t)((attempt + 1) * 97u);
          h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
          xi[k * es] = (T)((double)(h >> 8) * (1.0 / 8388608.0) - 1.0);
        }
        __syncthreads();
      }
    }
  }
}

// Block variant of the kernel above for r <= 64 vectors (every bond of the rounding sweeps): the sequential modified
// Gram-Schmidt of the kernel above walks the whole vector two times per (dead vector, earlier vector) pair with a block
// reduction each -- 51 ms per metric step on a decaying-spectrum batch whose kept directions 17 .. 31 of every bond lie below
// the resolution (SURVEY 8d's second input variant, measured).  Here one ROUND is: the Gram matrix S = X X^T of all r vectors
// (one pass, column chunks through LDS, products and sums in double), Gram-Schmidt of the dead
// rows IN COEFFICIENT SPACE against everything before them (r x r matrices in LDS, double; the live rows are orthonormal
// already and stay untouched), then X_dead <- W X in a second pass.  A dead vector whose remainder collapses (below 1 % of its
// norm, or a zero / non-finite vector) is replaced by a hashed pseudo-random one, which the next round orthogonalises.  A second
// round when a remainder lost more than half of its squared norm ("twice is enough": the second sees a Gram matrix within
// rounding of the identity), a third / fourth only after a replacement.  Same semantics as the kernel above: genuine remainders are kept, live vectors are not touched.
constexpr int kOfMaxE = 32;        // tile elements per thread: r x CW <= 32 x 256 (CW = 256 up to 32 vectors, 128 above)

inline size_t orth_fixup_lds_bytes(int r, int cw, size_t es) {
  const int r4 = (r + 15) & ~15;   // whole 16 x 16 MFMA tiles
  return (size_t)r4 * (cw + 4) * es + 2 * (size_t)r4 * (r4 + 1) * 8 + 2 * 64 * 8 + 64 * 4 + 16;
}

// kOfCW: columns per chunk (a chunk = one global round trip + two barriers: 64 columns left the kernel latency-bound on
// them); kOfLd: tile row stride
// V2 (round 5, the CW = 256 instance, i.e. up to 32 vectors -- every bond of a rank-32 rounding): the same two passes per round with
// their inner loops rebuilt around the LDS.  Round 4's loops issued one ds_read_b32 per MFMA operand and waited for it (184 VGPRs:
// two waves per SIMD, nothing to hide the latency with): 12 us per 32 x 256 chunk and pass, measured (profiles/r05_decay_probe.txt:
// 0.76 ms per launch and round at B = 2048) against ~1 us of MFMA time.  Here (a) the Gram pass reads its operands as ds_read_b128
// with the K index permuted (lane (i, q) takes columns 16 g + 4 q + j for the j-th MFMA of column group g: any K order is a valid
// sum), computes only the tile rows that hold dead vectors, and the four waves split the chunk's 16-column groups (partials added
// through S in wave order: deterministic); (b) the apply pass keeps its W operands in registers for the whole pass and reads the
// tile with a K permutation that spreads a wave's four K rows over all 64 banks.
template <typename T, int kOfCW, bool V2>
__global__ __launch_bounds__(kThreads, V2 ? 2 : 1) void orth_fixup_block_kernel(int r, int64_t n, T* __restrict__ X, int64_t vs, int64_t es,
                                                                    int64_t strideX, const T* __restrict__ sigma,
                                                                    int64_t stride_sigma, double dead_rel,
                                                                    const int32_t* __restrict__ rank_dev, int max_rounds,
                                                                    double* __restrict__ census, long long* __restrict__ dbg,
                                                                    const int32_t* __restrict__ skip_items, int round0) {
  constexpr int kOfLd = kOfCW + 4;
  // (`skip_items` / `round0`: this launch finishes what the three-launch rounds left over -- items flagged done return at once, the
  // others continue with round number round0, which only enters the hashed replacement vectors)
  if (skip_items && skip_items[blockIdx.x] != 0) return;
  // (diagnostics, ttr_debug_set_qr_stamps with TTR_KNOB_QR_STAMP_BX = -1: item 0 stamps its phases -- start, then per round: Gram
  // pass done, coefficients done, apply pass done)
  int dbgi = 0;
  auto ostamp = [&]() { if (dbg && blockIdx.x == 0 && threadIdx.x == 0) dbg[dbgi++] = (long long)clock64(); };
  ostamp();
  extern __shared__ __attribute__((aligned(16))) unsigned char of_smem[];
  const int r_launch = r;
  const int64_t b = blockIdx.x;
  if (rank_dev) r = rank_dev[b] < r ? rank_dev[b] : r;
  const T* __restrict__ sg = sigma + b * stride_sigma;
  const double s0 = (double)sg[0];
  int first = r;
  for (int i = 0; i < r; ++i)
    if (!((double)sg[i] > dead_rel * s0)) { first = i; break; }  // (also catches NaN / zero sigma_0)
  if (first >= r) return;
  // carve the dynamic LDS (sized for the launch's r, rounded up to whole 16 x 16 MFMA tiles)
  const int r4 = (r_launch + 15) & ~15;
  const int ls = r4 + 1;                                   // row stride of S / W
  double* S = reinterpret_cast<double*>(of_smem);          // [r4][ls]
  double* W = S + (size_t)r4 * ls;
  double* tv = W + (size_t)r4 * ls;                        // [64]
  double* pj = tv + 64;
  int* regen = reinterpret_cast<int*>(pj + 64);            // [64]
  int* any_regen = regen + 64;
  T* tile = reinterpret_cast<T*>(any_regen + 4);           // [r4][kOfLd]
  T* __restrict__ Xb = X + b * strideX;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int nt = (r + 15) >> 4;              // 16-row tiles that hold vectors
  const bool vec_contig = es == 1;           // vectors are rows of a row-major matrix (else: columns, es = row stride)
  const int ne = (r * kOfCW + kThreads - 1) / kThreads;    // tile elements per thread (<= kOfMaxE)
  // rows of the tile beyond r are read by the 16 x 16 MFMA tiles: keep them zero
  for (int idx = r * kOfLd + tid; idx < r4 * kOfLd; idx += kThreads) tile[idx] = T(0);

  // chunk c0 .. c0 + 63 of all r vectors: global -> registers (issued one chunk ahead), registers -> LDS
  auto fetch = [&](int64_t c0, T* reg) {
    const int cw = (int)((n - c0) < kOfCW ? (n - c0) : kOfCW);
#pragma unroll
    for (int e = 0; e < kOfMaxE; ++e) {
      if (e >= ne) break;
      const int idx = tid + e * kThreads;
      int i, c;
      if (vec_contig) { i = idx / kOfCW; c = idx - i * kOfCW; } else { c = idx / r; i = idx - c * r; }
      reg[e] = (i < r && c < cw) ? Xb[(int64_t)i * vs + (c0 + c) * es] : T(0);
    }
  };
  auto stage = [&](const T* reg) {
#pragma unroll
    for (int e = 0; e < kOfMaxE; ++e) {
      if (e >= ne) break;
      const int idx = tid + e * kThreads;
      int i, c;
      if (vec_contig) { i = idx / kOfCW; c = idx - i * kOfCW; } else { c = idx / r; i = idx - c * r; }
      if (i < r && c < kOfCW) {
        const T v = reg[e];
        tile[i * kOfLd + c] = (v - v == T(0)) ? v : T(0);   // (non-finite entries of a dead vector count as zero: 0 x NaN would poison the products)
      }
    }
  };

  // Chunk order.  Every item's vectors lie 4 n bytes apart (8 KB at the metric's bonds), so the 32 row pieces of chunk c of EVERY
  // item share their address bits 10 .. 12: workgroups that walk their chunks in step keep hitting the same eighth of the HBM
  // channels (measured, round 5: 13.5 us per 32 KB chunk and workgroup = 1.2 TB/s chip-wide with the loads of a whole chunk in
  // flight per workgroup; profiles/r05_orth_stamps.txt).  V2: item b starts at chunk b mod nch and wraps around -- at any moment
  // the resident workgroups cover all chunk phases.  (The Gram sums are then added in an item-dependent order: double
  // accumulation across chunks, so an item's result depends on its position in the batch at the 1e-16 level of S only.)
  const int nch = (int)((n + kOfCW - 1) / kOfCW);
  const int rot = V2 ? (int)(b % nch) : 0;
  auto chunk_c0 = [&](int tq) { int c = tq + rot; if (c >= nch) c -= nch; return (int64_t)c * kOfCW; };
  if (census && round0 == 0 && tid == 0) atomicAdd(census + TTR_PROF_NKINDS + TTR_PROF_MISC, 1.0);   // census: items with dead rows ...
  if (round0 > 0) census = nullptr;   // (the item and its first rounds were counted by the three-launch rounds)
  for (int round = round0; round < max_rounds; ++round) {
    if (census && tid == 0) atomicAdd(census + TTR_PROF_MISC, 1.0);                   // ... and the rounds they took
    // ---- S = X X^T on the matrix cores: wave w owns the 16-row tile w of S (all column tiles); fp32 accumulators are
    // flushed into double sums after every chunk (64 products per entry), fp64 accumulates in place
    double sacc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) sacc[u][v] = 0.0;
    T reg[kOfMaxE];
    fetch(chunk_c0(0), reg);
    for (int tq = 0; tq < nch; ++tq) {
      __syncthreads();
      stage(reg);
      __syncthreads();
      if (tq + 1 < nch) fetch(chunk_c0(tq + 1), reg);   // the next chunk's loads fly under this chunk's products
      if constexpr (V2) {
        // nt <= 2 tile rows; sacc[2 tr + v] = tile (tr, v) of S for the tile rows tr >= tr0 that hold dead vectors
        typename Mfma<T>::Acc acc[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] = Mfma<T>::zero();
        const int tr0 = first >> 4;
        const T* __restrict__ xr = tile + (lane & 15) * kOfLd + 4 * (lane >> 4);
#pragma unroll
        for (int g = 0; g < kOfCW / 64; ++g) {
          const int k0 = 16 * (wv + 4 * g);
          typedef T tv4 __attribute__((ext_vector_type(4)));
          const tv4 x0 = *reinterpret_cast<const tv4*>(xr + k0);
          const tv4 x1 = nt > 1 ? *reinterpret_cast<const tv4*>(xr + 16 * kOfLd + k0) : tv4{0, 0, 0, 0};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (tr0 == 0) {
              acc[0] = Mfma<T>::mma(x0[j], x0[j], acc[0]);
              if (nt > 1) acc[1] = Mfma<T>::mma(x0[j], x1[j], acc[1]);
            }
            if (nt > 1) {
              acc[2] = Mfma<T>::mma(x1[j], x0[j], acc[2]);
              acc[3] = Mfma<T>::mma(x1[j], x1[j], acc[3]);
            }
          }
        }
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int u = 0; u < 4; ++u) sacc[v][u] += (double)acc[v][u];
      } else {
      if (wv < nt) {
        typename Mfma<T>::Acc acc[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] = Mfma<T>::zero();
        const T* __restrict__ arow = tile + (16 * wv + (lane & 15)) * kOfLd + (lane >> 4);
#pragma unroll 4
        for (int k0 = 0; k0 < kOfCW; k0 += 4) {
          const T a = arow[k0];
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (v < nt) acc[v] = Mfma<T>::mma(a, tile[(16 * v + (lane & 15)) * kOfLd + k0 + (lane >> 4)], acc[v]);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int u = 0; u < 4; ++u) sacc[v][u] += (double)acc[v][u];
      }
      }
    }
    __syncthreads();
    if constexpr (V2) {
      // the four waves' partial sums, added in wave order (deterministic); tile (tr, v) lives in sacc[2 tr + v]
      for (int w = 0; w < 4; ++w) {
        if (wv == w) {
#pragma unroll
          for (int tv = 0; tv < 4; ++tv) {
            const int tr = tv >> 1, v = tv & 1;
            if (tr < (first >> 4) || tr >= nt || v >= nt) continue;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              double* dst = S + (16 * tr + Mfma<T>::row(lane, u)) * ls + 16 * v + (lane & 15);
              *dst = (w == 0 ? 0.0 : *dst) + sacc[tv][u];
            }
          }
        }
        __syncthreads();
      }
    } else {
    if (wv < nt) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (v < nt) {
#pragma unroll
          for (int u = 0; u < 4; ++u) S[(16 * wv + Mfma<T>::row(lane, u)) * ls + 16 * v + (lane & 15)] = sacc[v][u];
        }
    }
    }
    if (tid < 64) regen[tid] = 0;
    if (tid == 0) { any_regen[0] = 0; any_regen[1] = 0; }
    __syncthreads();
    ostamp();
    // ---- the dead rows against everything before them, in coefficient space (double).  The live rows are orthonormal
    // (S_LL = I to rounding), so the remainders x_d - S_dL x_L have the Gram matrix C = S_DD - S_DL S_LD; with C = L L^T
    // (Cholesky) the rows of  L^-1 [-S_DL, I]  are the coefficients of the orthonormalised dead vectors.  A pivot below 1e-4
    // of the vector's own squared norm (or a zero vector) = the remainder collapsed: that row is replaced.
    const int nd = r - first;
    double* Cm = W;                                      // nd x nd, stride ls
    for (int idx = tid; idx < nd * nd; idx += kThreads) {
      const int ia = idx / nd, ib = idx - ia * nd;
      const double* __restrict__ sa = S + (size_t)(first + ia) * ls;
      const double* __restrict__ sb = S + (size_t)(first + ib) * ls;
      double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
      int k = 0;
      for (; k + 3 < first; k += 4) { c0 += sa[k] * sb[k]; c1 += sa[k + 1] * sb[k + 1]; c2 += sa[k + 2] * sb[k + 2]; c3 += sa[k + 3] * sb[k + 3]; }
      for (; k < first; ++k) c0 += sa[k] * sb[k];
      Cm[ia * ls + ib] = sa[first + ib] - ((c0 + c1) + (c2 + c3));
    }
    __syncthreads();
    for (int a = 0; a < nd; ++a) {                       // right-looking Cholesky, lower triangle in place
      const double piv = Cm[a * ls + a], saa = S[(first + a) * ls + first + a];
      const bool bad = !(saa > 0.0) || !(saa < 1e300) || !(piv > 1e-4 * saa);
      const double dinv = bad ? 0.0 : 1.0 / sqrt(piv);
      __syncthreads();                                   // (everybody has read the pivot)
      if (tid > a && tid < nd) Cm[tid * ls + a] *= dinv; // (collapsed: the column is removed)
      if (tid == a) Cm[a * ls + a] = bad ? 1.0 : piv * dinv;
      if (tid == 0 && bad) { regen[first + a] = 1; any_regen[0] = 1; }
      if (tid == 0 && !(piv > 0.5 * saa)) any_regen[1] = 1;   // lost more than half of its squared norm: orthogonalise twice
      __syncthreads();
      if (!bad) {
        const int rem = nd - a - 1;
        for (int idx = tid; idx < rem * rem; idx += kThreads) {
          const int i = a + 1 + idx / rem, j = a + 1 + idx % rem;
          if (j <= i) Cm[i * ls + j] -= Cm[i * ls + a] * Cm[j * ls + a];
        }
      }
      __syncthreads();
    }
    // Z = [-S_DL, I] in place over the dead rows of S, then the forward substitution L W_D = Z row by row (S is not needed any more)
    for (int idx = tid; idx < nd * r4; idx += kThreads) {
      const int ia = idx / r4, k = idx - ia * r4;
      double* __restrict__ zr = S + (size_t)(first + ia) * ls;
      zr[k] = k < first ? -zr[k] : (k == first + ia ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int a = 0; a < nd; ++a) {
      if (tid < r4) {
        double* __restrict__ za = S + (size_t)(first + a) * ls;
        double w = 0.0;
        if (!regen[first + a]) {
          double w0 = za[tid], w1 = 0.0, w2 = 0.0, w3 = 0.0;
          const double* __restrict__ la = Cm + (size_t)a * ls;
          int bq = 0;
          for (; bq + 3 < a; bq += 4) {
            w0 -= la[bq] * S[(size_t)(first + bq) * ls + tid];
            w1 -= la[bq + 1] * S[(size_t)(first + bq + 1) * ls + tid];
            w2 -= la[bq + 2] * S[(size_t)(first + bq + 2) * ls + tid];
            w3 -= la[bq + 3] * S[(size_t)(first + bq + 3) * ls + tid];
          }
          for (; bq < a; ++bq) w0 -= la[bq] * S[(size_t)(first + bq) * ls + tid];
          w = ((w0 + w1) + (w2 + w3)) / la[a];
        }
        za[tid] = w;
      }
      __syncthreads();
    }
    ostamp();
    // ---- X_dead <- W X  (regenerated rows: hashed pseudo-random values, orthogonalised by the next round)
    fetch(chunk_c0(0), reg);
    for (int tq = 0; tq < nch; ++tq) {
      const int64_t c0 = chunk_c0(tq);
      const int cw = (int)((n - c0) < kOfCW ? (n - c0) : kOfCW);
      __syncthreads();
      stage(reg);
      __syncthreads();
      if (tq + 1 < nch) fetch(chunk_c0(tq + 1), reg);
      // wave w: the 16-column blocks w, w + 4, .. of the chunk, every 16-row tile that holds dead rows; W (double in LDS) is the A
      // operand in the matrix precision -- the second round sees W = I + O(first round's error), which restores full accuracy
      for (int cb = wv; cb < kOfCW / 16; cb += 4)
      for (int it = first >> 4; it < nt; ++it) {
        typename Mfma<T>::Acc acc = Mfma<T>::zero();
        const double* __restrict__ wrow = S + (size_t)(16 * it + (lane & 15)) * ls + (lane >> 4);   // (the dead rows of S hold W_D now)
        const T* __restrict__ bcol = tile + (lane >> 4) * kOfLd + 16 * cb + (lane & 15);
        for (int k0 = 0; k0 < 16 * nt; k0 += 4) acc = Mfma<T>::mma((T)wrow[k0], bcol[k0 * kOfLd], acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int d = 16 * it + Mfma<T>::row(lane, u), c = 16 * cb + (lane & 15);
          if (d < first || d >= r || c >= cw) continue;
          T out = acc[u];
          if (regen[d]) {
            const int64_t k = c0 + c;
            uint32_t h = (uint32_t)(k * 2654435761u) ^ (uint32_t)((d + 1) * 40503u) ^ (uint32_t)((round + 1) * 97u);
            h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
            out = (T)((double)(h >> 8) * (1.0 / 8388608.0) - 1.0);
          }
          Xb[(int64_t)d * vs + (c0 + c) * es] = out;
        }
      }
    }
    __syncthreads();
    // "twice is enough" (Kahan / Parlett): a remainder that kept at least 1 / sqrt(2) of its vector's norm is orthogonal to
    // the others to ~1.4 eps already -- the second round is only run when some vector lost more (or was replaced).  (Measured,
    // round 4: on the decaying-spectrum batch every item needs it -- the dead rows are mostly leakage of the live ones.  Starting
    // the dead rows from hashed vectors instead, one round: 11.3 -> 6.7 ms per step, but the approximation error of that batch
    // rose from 8.6e-6 to 2.4e-5 -- the dead rows do carry part of the tail; not taken.)
    ostamp();
    if (!any_regen[0] && (round >= 1 || !any_regen[1])) break;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ttr_orth_fixup for LARGE batches (round 5): the same rounds -- Gram matrix, coefficients, X_dead <- W X -- as three launches per
// round instead of one workgroup per item.  Why: the single-workgroup kernel above keeps one 32 KB chunk in flight per workgroup
// and walks an item's 256 KB four times; even with the staggered chunk order a pass costs 8 us per chunk (cycle stamps,
// profiles/r05_orth_stamps.txt), i.e. ~2 TB/s chip-wide.  The Gram pass IS ttr_rowgram on the r x n matrix of vectors (split-K
// partials, 16-byte loads, two slabs in flight per wave: 4 TB/s class), and the apply pass is a streaming kernel of the same
// build (below).  Per-item control flow lives in flag arrays: skip[round][b] != 0 = item b takes no part in that round.
// Small batches keep the single launch (three launches per round and bond would add ~40 dependent launches to a B = 1 call).
constexpr int kOrthSplitRounds = 2;
struct OrthSplitWs {
  int64_t off_g, off_w, off_regen, off_skip, total;
  int parts;    // Gram partials of a ttr_rowgram launch
  int nsplit;   // column splits of the apply launch (grid x)
  int fparts;   // Gram partials written by a FUSED apply launch (one per wave and column split)
};
static OrthSplitWs orth_split_layout(int64_t r, int64_t n, int64_t batch, int64_t es, int max_rounds) {
  OrthSplitWs w{};
  const int64_t r4 = (r + 15) & ~15LL;
  w.parts = n >= 2048 ? 4 : (n >= 1024 ? 2 : 1);   // short fp32 accumulation chains: the partials are summed in double
  w.nsplit = (int)ceil_div(2048, batch);           // aim at >= 2048 workgroups, >= 8 slabs per wave
  const int64_t slabs = (n + 15) / 16;
  if (w.nsplit > slabs / 32) w.nsplit = (int)(slabs / 32);
  if (w.nsplit < 1) w.nsplit = 1;
  w.fparts = 4 * w.nsplit;
  int64_t off = 0;
  w.off_g = off; off += align_up(batch * (w.parts > w.fparts ? w.parts : w.fparts) * r * r * es, 256);
  w.off_w = off; off += align_up(batch * r4 * r4 * es, 256);
  w.off_regen = off; off += align_up(batch * 8, 256);                       // one 64-bit mask per item
  w.off_skip = off; off += align_up((int64_t)(max_rounds + 1) * batch * 4, 256);
  w.total = off;
  return w;
}

template <typename T>
__global__ void orth_init_kernel(int r, int64_t batch, const T* __restrict__ sigma, int64_t stride_sigma, double dead_rel,
                                 const int32_t* __restrict__ rank_dev, int32_t* __restrict__ skip0) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  if (rank_dev) r = rank_dev[b] < r ? rank_dev[b] : r;
  const T* __restrict__ sg = sigma + b * stride_sigma;
  const double s0 = (double)sg[0];
  int first = r;
  for (int i = 0; i < r; ++i)
    if (!((double)sg[i] > dead_rel * s0)) { first = i; break; }
  skip0[b] = first >= r ? 1 : 0;
}

// Coefficients of one round (the middle section of orth_fixup_block_kernel, verbatim): S = sum of the Gram partials (double),
// Cholesky of the dead rows' Schur complement, W_D = L^-1 [-S_DL, I].  Writes W (matrix precision), the regeneration mask and
// the next round's skip flag.
template <typename T>
__global__ __launch_bounds__(kThreads) void orth_coef_kernel(int r, const T* __restrict__ Gp, int parts, T* __restrict__ Wg,
                                                             unsigned long long* __restrict__ regen_mask, const int32_t* __restrict__ skip_now,
                                                             int32_t* __restrict__ skip_next, const T* __restrict__ sigma,
                                                             int64_t stride_sigma, double dead_rel, const int32_t* __restrict__ rank_dev,
                                                             int round, double* __restrict__ census) {
  extern __shared__ __attribute__((aligned(16))) unsigned char oc_smem[];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  if (skip_now[b] != 0) { if (tid == 0) skip_next[b] = 1; return; }
  const int r_launch = r;
  if (rank_dev) r = rank_dev[b] < r ? rank_dev[b] : r;
  const T* __restrict__ sg = sigma + b * stride_sigma;
  const double s0 = (double)sg[0];
  int first = r;
  for (int i = 0; i < r; ++i)
    if (!((double)sg[i] > dead_rel * s0)) { first = i; break; }
  const int r4 = (r_launch + 15) & ~15;
  const int ls = r4 + 1;
  double* S = reinterpret_cast<double*>(oc_smem);   // [r4][ls]
  double* W = S + (size_t)r4 * ls;
  int* regen = reinterpret_cast<int*>(W + (size_t)r4 * ls);   // [64]
  int* any_regen = regen + 64;
  if (census && tid == 0) {
    if (round == 0) atomicAdd(census + TTR_PROF_NKINDS + TTR_PROF_MISC, 1.0);
    atomicAdd(census + TTR_PROF_MISC, 1.0);
  }
  const T* __restrict__ G = Gp + b * (int64_t)parts * r_launch * r_launch;
  for (int idx = tid; idx < r4 * r4; idx += kThreads) {
    const int i = idx / r4, j = idx - i * r4;
    double v = 0.0;
    if (i < r_launch && j < r_launch)
      for (int pt = 0; pt < parts; ++pt) v += (double)G[(int64_t)pt * r_launch * r_launch + i * r_launch + j];
    S[i * ls + j] = v;
  }
  if (tid < 64) regen[tid] = 0;
  if (tid == 0) { any_regen[0] = 0; any_regen[1] = 0; }
  __syncthreads();
  // a dead vector with a non-finite entry has a non-finite diagonal: it counts as the zero vector (replaced below); its row and
  // column must not poison the others (the single-launch kernel zeroes such entries when it stages the vectors)
  for (int d = first; d < r; ++d) {
    const double sdd = S[d * ls + d];
    if (!(sdd - sdd == 0.0)) {
      __syncthreads();
      for (int k = tid; k < r4; k += kThreads) { S[d * ls + k] = 0.0; S[k * ls + d] = 0.0; }
      __syncthreads();
    }
  }
  for (int idx = tid; idx < (r - first) * r4; idx += kThreads) {   // (other non-finite entries of dead rows: treated as zero)
    const int d = first + idx / r4, k = idx % r4;
    const double v = S[d * ls + k];
    if (!(v - v == 0.0)) { S[d * ls + k] = 0.0; S[k * ls + d] = 0.0; }
  }
  __syncthreads();
  const int nd = r - first;
  double* Cm = W;
  for (int idx = tid; idx < nd * nd; idx += kThreads) {
    const int ia = idx / nd, ib = idx - ia * nd;
    const double* __restrict__ sa = S + (size_t)(first + ia) * ls;
    const double* __restrict__ sb = S + (size_t)(first + ib) * ls;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    int k = 0;
    for (; k + 3 < first; k += 4) { c0 += sa[k] * sb[k]; c1 += sa[k + 1] * sb[k + 1]; c2 += sa[k + 2] * sb[k + 2]; c3 += sa[k + 3] * sb[k + 3]; }
    for (; k < first; ++k) c0 += sa[k] * sb[k];
    Cm[ia * ls + ib] = sa[first + ib] - ((c0 + c1) + (c2 + c3));
  }
  __syncthreads();
  for (int a = 0; a < nd; ++a) {
    const double piv = Cm[a * ls + a], saa = S[(first + a) * ls + first + a];
    const bool bad = !(saa > 0.0) || !(saa < 1e300) || !(piv > 1e-4 * saa);
    const double dinv = bad ? 0.0 : 1.0 / sqrt(piv);
    __syncthreads();
    if (tid > a && tid < nd) Cm[tid * ls + a] *= dinv;
    if (tid == a) Cm[a * ls + a] = bad ? 1.0 : piv * dinv;
    if (tid == 0 && bad) { regen[first + a] = 1; any_regen[0] = 1; }
    if (tid == 0 && !(piv > 0.5 * saa)) any_regen[1] = 1;
    __syncthreads();
    if (!bad) {
      const int rem = nd - a - 1;
      for (int idx = tid; idx < rem * rem; idx += kThreads) {
        const int i = a + 1 + idx / rem, j = a + 1 + idx % rem;
        if (j <= i) Cm[i * ls + j] -= Cm[i * ls + a] * Cm[j * ls + a];
      }
    }
    __syncthreads();
  }
  for (int idx = tid; idx < nd * r4; idx += kThreads) {
    const int ia = idx / r4, k = idx - ia * r4;
    double* __restrict__ zr = S + (size_t)(first + ia) * ls;
    zr[k] = k < first ? -zr[k] : (k == first + ia ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int a = 0; a < nd; ++a) {
    if (tid < r4) {
      double* __restrict__ za = S + (size_t)(first + a) * ls;
      double w = 0.0;
      if (!regen[first + a]) {
        double w0 = za[tid], w1 = 0.0, w2 = 0.0, w3 = 0.0;
        const double* __restrict__ la = Cm + (size_t)a * ls;
        int bq = 0;
        for (; bq + 3 < a; bq += 4) {
          w0 -= la[bq] * S[(size_t)(first + bq) * ls + tid];
          w1 -= la[bq + 1] * S[(size_t)(first + bq + 1) * ls + tid];
          w2 -= la[bq + 2] * S[(size_t)(first + bq + 2) * ls + tid];
          w3 -= la[bq + 3] * S[(size_t)(first + bq + 3) * ls + tid];
        }
        for (; bq < a; ++bq) w0 -= la[bq] * S[(size_t)(first + bq) * ls + tid];
        w = ((w0 + w1) + (w2 + w3)) / la[a];
      }
      za[tid] = w;
    }
    __syncthreads();
  }
  // W_D in the matrix precision (rows below `first` are never applied: zero), mask, next round's flag
  T* __restrict__ Wb = Wg + b * (int64_t)r4 * r4;
  for (int idx = tid; idx < r4 * r4; idx += kThreads) {
    const int i = idx / r4, k = idx - i * r4;
    Wb[idx] = (i >= first && i < r) ? (T)S[(size_t)i * ls + k] : T(0);
  }
  if (tid == 0) {
    unsigned long long m = 0ull;
    for (int d = first; d < r; ++d) if (regen[d]) m |= 1ull << d;
    regen_mask[b] = m;
    skip_next[b] = (any_regen[0] || (round == 0 && any_regen[1])) ? 0 : 1;
  }
}

// X_dead <- W X, streamed: grid (column splits, items); a wave walks 16-column slabs (every item starts at another slab: the
// columns are independent), the vectors of a slab are the B operand straight from global memory (four 64-byte row segments per
// load, the next slab's loads in flight under this slab's products), W is the A operand from an LDS image.
//
// GRAM (at most 32 vectors): the launch also leaves the Gram matrix of the vectors AS IT WROTE THEM -- what the next round's
// coefficients are computed from -- so that the next round does not read the item again for it (ttr_rowgram on 32 x 2048 items:
// 0.35 ms per launch at B = 4096, a quarter of the round).  The MFMA products of the apply pass have the columns on the lanes'
// N index; the Gram product contracts over the columns, so a slab's 32 x 16 tile (live rows as loaded, dead rows as computed)
// goes through a per-wave LDS tile and comes back with the columns on K.  Only the dead row tiles' rows of the Gram matrix are
// formed (orth_coef_kernel reads nothing else); every wave writes its own partial: Gnext[b][4 split + wave][r][r], the others
// zero.
constexpr int kOrthXtLd = 17;
template <typename T, bool GRAM>
__global__ __launch_bounds__(kThreads) void orth_apply_kernel(int r, int64_t n, T* __restrict__ X, int64_t vs, int64_t strideX,
                                                              const T* __restrict__ Wg, const unsigned long long* __restrict__ regen_mask,
                                                              const int32_t* __restrict__ skip_now, const T* __restrict__ sigma,
                                                              int64_t stride_sigma, double dead_rel, const int32_t* __restrict__ rank_dev,
                                                              int round, int nsplit, T* __restrict__ Gnext) {
  using M = Mfma<T>;
  __shared__ T Wl[64 * 65];
  __shared__ T Xt[GRAM ? 4 * 32 * kOrthXtLd : 1];
  const int64_t b = blockIdx.y;
  if (skip_now[b] != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, g = lane >> 4;
  const int r_launch = r;
  if (rank_dev) r = rank_dev[b] < r ? rank_dev[b] : r;
  const T* __restrict__ sg = sigma + b * stride_sigma;
  const double s0 = (double)sg[0];
  int first = r;
  for (int i = 0; i < r; ++i)
    if (!((double)sg[i] > dead_rel * s0)) { first = i; break; }
  const int r4 = (r_launch + 15) & ~15;
  const int nt = (r + 15) >> 4, it0 = first >> 4;
  const T* __restrict__ Wb = Wg + b * (int64_t)r4 * r4;
  for (int idx = tid; idx < r4 * r4; idx += kThreads) Wl[(idx / r4) * 65 + idx % r4] = Wb[idx];
  const unsigned long long rm = regen_mask[b];
  __syncthreads();
  T* __restrict__ Xb = X + b * strideX;
  const int64_t slabs = (n + 15) / 16, per = (slabs + nsplit - 1) / nsplit;
  const int64_t cb = (int64_t)blockIdx.x * per, ce = cb + per < slabs ? cb + per : slabs;
  const int64_t nsteps = ce > cb + wave ? (ce - cb - wave + 3) / 4 : 0;
  const int64_t rot = nsteps > 1 ? (int64_t)(b % nsteps) : 0;
  auto step_c = [&](int64_t sidx) { int64_t sq = sidx + rot; if (sq >= nsteps) sq -= nsteps; return cb + wave + 4 * sq; };
  const int nks = r4 >> 2;
  constexpr int KS = GRAM ? 8 : 16;   // k-steps of four vectors held per slab (GRAM: at most 32 vectors)
  auto load_cols = [&](int64_t c, T (&a)[KS]) {
    const int64_t col = c * 16 + cl;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + g;
      T v = (ks < nks && k < r_launch && col < n) ? Xb[(int64_t)k * vs + col] : T(0);
      a[ks] = (v - v == T(0)) ? v : T(0);   // (non-finite entries of a dead vector count as zero)
    }
  };
  T a[KS], an[KS];
  T* const xt = Xt + (GRAM ? wave * 32 * kOrthXtLd : 0);
  typename M::Acc Gacc[2][2] = {{M::zero(), M::zero()}, {M::zero(), M::zero()}};
  if (nsteps > 0) load_cols(step_c(0), a);
  for (int64_t sidx = 0; sidx < nsteps; ++sidx) {
    const int64_t c = step_c(sidx);
    if (sidx + 1 < nsteps) load_cols(step_c(sidx + 1), an);
    if constexpr (GRAM) {   // the slab as loaded (columns beyond n: zeros); the dead rows are overwritten below
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        if (ks < nks) xt[(4 * ks + g) * kOrthXtLd + cl] = a[ks];
    }
    for (int it = it0; it < nt; ++it) {
      typename M::Acc acc = M::zero();
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        if (ks < nks) acc = M::mma(Wl[(16 * it + cl) * 65 + 4 * ks + g], a[ks], acc);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int d = 16 * it + M::row(lane, u);
        const int64_t col = c * 16 + cl;
        if (d < first || d >= r || col >= n) continue;
        T out = acc[u];
        if ((rm >> d) & 1ull) {
          uint32_t h = (uint32_t)(col * 2654435761u) ^ (uint32_t)((d + 1) * 40503u) ^ (uint32_t)((round + 1) * 97u);
          h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
          out = (T)((double)(h >> 8) * (1.0 / 8388608.0) - 1.0);
        }
        Xb[(int64_t)d * vs + col] = out;
        if constexpr (GRAM) xt[d * kOrthXtLd + cl] = out;
      }
    }
    if constexpr (GRAM) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (one wave, in-order LDS: the tile is complete)
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        if (it >= it0 && it < nt) {   // (wave-uniform)
          T pa[4];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) pa[s4] = xt[(16 * it + cl) * kOrthXtLd + 4 * s4 + g];
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) {
            if (jt < nt) {
#pragma unroll
              for (int s4 = 0; s4 < 4; ++s4) Gacc[it][jt] = M::mma(pa[s4], xt[(16 * jt + cl) * kOrthXtLd + 4 * s4 + g], Gacc[it][jt]);
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the reads are done before the next slab's tile is written)
    }
    if (sidx + 1 < nsteps) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
    }
  }
  if constexpr (GRAM) {
    T* __restrict__ Gp = Gnext + ((b * nsplit + blockIdx.x) * 4 + wave) * (int64_t)r_launch * r_launch;
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = 16 * it + M::row(lane, u), j = 16 * jt + cl;
          if (i < r_launch && j < r_launch) Gp[i * r_launch + j] = Gacc[it][jt][u];
        }
  }
}

int g_orth_rounds = 4;   // ttr_debug_set_knob(TTR_KNOB_ORTH_ROUNDS): rounds of the block orthonormal completion (diagnostics)
int g_orth_v2 = 2;       // ttr_debug_set_knob(TTR_KNOB_ORTH_V2): 0 = round 4's inner loops, 1 = round 5's, 2 = + the three-launch rounds' fused Gram (A/B)
// ttr_debug_set_knob(TTR_KNOB_ORTH_SPLIT): batches from this size (per launch, i.e. per sub-batch stream) take the three-launch
// rounds; 0 = never.  Where most kept directions lie below the resolution (sigma ~ 2^-j) the rounds cost 6.0 instead of 8.4 ms per
// 2048-train step (B = 4096: step 50.4 -> 44.5 ms, 650 k -> 736 k cores/s); a batch WITHOUT dead directions pays for 13 launches
// per bond that exit at once instead of one: nothing measurable from 2048 items per launch (headline at B = 4096, four
// alternations: 25.515 vs 25.524 ms), 0.3 - 2 % at 1024 (profiles/r05_orth_split_ab.txt, r05_orth_split_headline_ab.txt) --
// hence the threshold.
int g_orth_split = 2048;

// (vectors as rows of a row-major matrix, at most 64 of them, at least 512 elements each, a batch that fills the chip)
static bool orth_split_ok(int64_t r, int64_t n, int64_t batch, int64_t elem_stride) {
  return g_orth_split > 0 && batch >= g_orth_split && batch <= 65535 && elem_stride == 1 && r >= 2 && r <= 64 && n >= 512;
}

template <typename T>
static int orth_split_run(int64_t r, int64_t n, int64_t batch, T* X, int64_t vs, int64_t strideX, const T* sigma, int64_t stride_sigma,
                          double dead_rel, const int32_t* rank_dev, char* ws, hipStream_t s) {
  const int dtype = sizeof(T) == 4 ? TTR_F32 : TTR_F64;
  const OrthSplitWs L = orth_split_layout(r, n, batch, sizeof(T), g_orth_rounds);
  T* G = (T*)(ws + L.off_g);
  T* Wg = (T*)(ws + L.off_w);
  unsigned long long* regen = (unsigned long long*)(ws + L.off_regen);
  int32_t* skip = (int32_t*)(ws + L.off_skip);
  double* census = work_census_dev();
  {
    ProfScope prof(TTR_PROF_MISC, s);
    hipLaunchKernelGGL(orth_init_kernel<T>, dim3((unsigned)ceil_div(batch, kThreads)), dim3(kThreads), 0, s, (int)r, batch, sigma, stride_sigma,
                       dead_rel, rank_dev, skip);
  }
  const int r4 = ((int)r + 15) & ~15;
  const size_t lds = 2 * (size_t)r4 * (r4 + 1) * 8 + 64 * 4 + 16;
  const int nsplit = L.nsplit;
  // at most 32 vectors: round k's apply launch leaves the Gram matrix round k + 1 starts from (orth_apply_kernel<T, true>)
  const bool fuse = g_orth_v2 >= 2 && r4 <= 32;
  // Two rounds ("twice is enough"); what is left after them -- items whose remainders collapsed and were replaced by hashed
  // vectors: rare -- is finished by the single-launch kernel (one launch that exits at once where nothing is left, instead of
  // six more launches per bond that do).
  const int nrounds = g_orth_rounds < kOrthSplitRounds ? g_orth_rounds : kOrthSplitRounds;
  for (int round = 0; round < nrounds; ++round) {
    const int32_t* sk = skip + (int64_t)round * batch;
    TTR_HIP_CHECK(hipGetLastError());
    const bool have_gram = fuse && round > 0;   // left by the previous round's apply launch
    if (!have_gram) {
      const int rc = sweep_gram_dispatch(dtype, r, n, batch, X, vs, strideX, nullptr, 0, 0, G, L.parts, s, sk, nullptr);
      if (rc != TTR_OK) return rc;
    }
    ProfScope prof(TTR_PROF_MISC, s);
    auto kern = orth_coef_kernel<T>;
    if (lds > 64 * 1024) TTR_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(kThreads), lds, s, (int)r, (const T*)G, have_gram ? L.fparts : L.parts, Wg, regen,
                       sk, skip + (int64_t)(round + 1) * batch, sigma, stride_sigma, dead_rel, rank_dev, round, census);
    if (fuse && round + 1 < nrounds)
      hipLaunchKernelGGL((orth_apply_kernel<T, true>), dim3((unsigned)nsplit, (unsigned)batch), dim3(kThreads), 0, s, (int)r, n, X, vs,
                         strideX, (const T*)Wg, (const unsigned long long*)regen, sk, sigma, stride_sigma, dead_rel, rank_dev, round,
                         nsplit, G);
    else
      hipLaunchKernelGGL((orth_apply_kernel<T, false>), dim3((unsigned)nsplit, (unsigned)batch), dim3(kThreads), 0, s, (int)r, n, X, vs,
                         strideX, (const T*)Wg, (const unsigned long long*)regen, sk, sigma, stride_sigma, dead_rel, rank_dev, round,
                         nsplit, (T*)nullptr);
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace ttr

using namespace ttr;

extern "C" {

int64_t ttr_orth_fixup_workspace_bytes(int dtype, int64_t r, int64_t n, int64_t batch, int64_t elem_stride) {
  if (!dtype_ok(dtype) || !orth_split_ok(r, n, batch, elem_stride)) return 0;
  return orth_split_layout(r, n, batch, elem_size(dtype), g_orth_rounds).total;
}

int ttr_orth_fixup(int dtype, int64_t r, int64_t n, int64_t batch, void* X, int64_t vec_stride, int64_t elem_stride,
                   int64_t strideX, const void* sigma, int64_t stride_sigma, double dead_rel, const int32_t* rank_dev,
                   void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_orth_fixup: bad dtype %d", dtype);
  TTR_REQUIRE(r >= 0 && n >= 0 && batch >= 0 && r <= 2147483647LL, TTR_E_INVALID, "ttr_orth_fixup: bad sizes");
  if (batch == 0 || r == 0 || n == 0) return TTR_OK;
  TTR_REQUIRE(X && sigma, TTR_E_INVALID, "ttr_orth_fixup: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int32_t* of_skip = nullptr;   // (set when the three-launch rounds ran first: what they left over goes to the single launch)
  int of_round0 = 0;
  if (workspace && orth_split_ok(r, n, batch, elem_stride) &&
      workspace_bytes >= orth_split_layout(r, n, batch, elem_size(dtype), g_orth_rounds).total) {
    const int rc = dtype == TTR_F32
                       ? orth_split_run<float>(r, n, batch, (float*)X, vec_stride, strideX, (const float*)sigma, stride_sigma, dead_rel,
                                               rank_dev, (char*)workspace, s)
                       : orth_split_run<double>(r, n, batch, (double*)X, vec_stride, strideX, (const double*)sigma, stride_sigma, dead_rel,
                                                rank_dev, (char*)workspace, s);
    if (rc != TTR_OK) return rc;
    of_round0 = g_orth_rounds < kOrthSplitRounds ? g_orth_rounds : kOrthSplitRounds;
    if (of_round0 >= g_orth_rounds) return TTR_OK;
    of_skip = (const int32_t*)((char*)workspace + orth_split_layout(r, n, batch, elem_size(dtype), g_orth_rounds).off_skip) +
              (int64_t)of_round0 * batch;
  }
  ProfScope prof(TTR_PROF_MISC, s);
  if (r <= 64) {  // the block variant (Gram matrix + coefficient-space Gram-Schmidt + one small product per round)
    const int cw = r <= 32 ? 256 : 128;
    const size_t lds = orth_fixup_lds_bytes((int)r, cw, elem_size(dtype));
#define TTR_OF_LAUNCH(T_, CW_, V2_)                                                                                             \
    do {                                                                                                                          \
      auto kern = orth_fixup_block_kernel<T_, CW_, V2_>;                                                                          \
      if (lds > 64 * 1024) TTR_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
      hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(kThreads), lds, s, (int)r, n, (T_*)X, vec_stride, elem_stride, strideX, \
                         (const T_*)sigma, stride_sigma, dead_rel, rank_dev, g_orth_rounds, work_census_dev(),                       \
                         g_qr_dbg_bx == -1 ? g_qr_dbg : nullptr, of_skip, of_round0);                                             \
    } while (0)
    if (dtype == TTR_F32) {
      if (cw == 256 && g_orth_v2) TTR_OF_LAUNCH(float, 256, true);
      else if (cw == 256) TTR_OF_LAUNCH(float, 256, false);
      else TTR_OF_LAUNCH(float, 128, false);
    } else {   // (fp64: round 4's loops -- the V2 instance would spill at two waves per SIMD)
      if (cw == 256) TTR_OF_LAUNCH(double, 256, false);
      else TTR_OF_LAUNCH(double, 128, false);
    }
#undef TTR_OF_LAUNCH
  } else if (dtype == TTR_F32)
    hipLaunchKernelGGL(orth_fixup_kernel<float>, dim3((unsigned)batch), dim3(kThreads), 0, s, (int)r, n, (float*)X,
                       vec_stride, elem_stride, strideX, (const float*)sigma, stride_sigma, dead_rel, rank_dev);
  else
    hipLaunchKernelGGL(orth_fixup_kernel<double>, dim3((unsigned)batch), dim3(kThreads), 0, s, (int)r, n, (double*)X,
                       vec_stride, elem_stride, strideX, (const double*)sigma, stride_sigma, dead_rel, rank_dev);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // extern "C"
