// Sparse TT-SVD from samples (interpolation.py:122-218, `sparse_tt_svd`): the Gram matrix of a sparse unfolding and the
// projection of that unfolding onto the kept eigenvectors, without ever scattering the samples into the dense nrows x ncols
// matrix D of the reference's `sparse_covariance` / `full_times_sparse`.
//
// The unfolding of step n is a BLOCK TABLE: column c (a distinct index suffix) owns the blocks colptr[c] .. colptr[c + 1), block
// b sits at mode index blk_i[b] (ascending inside a column) and carries r dense values V[b][0 .. r) -- the rows (a, blk_i[b]),
// row index a * I + blk_i[b], of that column of D.
//
//   ttr_sparse_keys     index validation into a flag word + the linear sort key of every sample
//   ttr_sparse_levels   per sorted sample, the deepest mode in which it differs from its predecessor (column boundaries of every
//                       step) + the repeated-position flag
//   ttr_sparse_gram     G = D D^T: G[(a,i),(b,j)] = sum over the columns c that hold both i and j of V_ci[a] V_cj[b]
//   ttr_sparse_project  W[c] = sum over the blocks b of column c of V_b @ core[:, blk_i[b], :], core read from U through strides
//
// Every output element is one thread's ordered sum (fma chain in ascending column / ascending mode-index order); partial matrices
// of a split i list are summed in part order.  No floating-point atomics: results are bit-identical from run to run.
#include "detail/ttr_internal.h"

namespace ttr {
namespace {

constexpr int kCh = 32;       // blocks of an i list staged per pass
constexpr int kJtMax = 64;    // widest j range of a workgroup
constexpr int kRt = 32;       // widest rank tile (a or b) of a workgroup
constexpr int kAcc = 8;       // accumulators per thread: a tile holds at most kAcc * kThreads output elements
constexpr int kLs = kCh + 1;  // padded stride of the per-j match lists (bank spread)
constexpr int64_t kPartBlocks = 2048;             // blocks of one i list per partial, on average
constexpr int64_t kPartBytes = (int64_t)256 << 20;  // budget of the partial matrices

struct GramGeom {
  int r, I, TA, TB, Jt, nTA, nTB, nJ, parts;
};

GramGeom gram_geom(int dtype, int64_t r, int64_t I, int64_t nb) {
  GramGeom g;
  g.r = (int)r;
  g.I = (int)I;
  g.TA = (int)(r < kRt ? r : kRt);
  g.TB = g.TA;
  int64_t jt = (int64_t)kAcc * kThreads / ((int64_t)g.TA * g.TB);
  jt = jt > kJtMax ? kJtMax : jt;
  jt = jt > I ? I : jt;
  g.Jt = (int)(jt < 1 ? 1 : jt);
  g.nTA = (int)ceil_div(r, g.TA);
  g.nTB = g.nTA;
  g.nJ = (int)ceil_div(I, g.Jt);
  const int64_t es = elem_size(dtype), n = r * I;
  int64_t p = ceil_div(nb > 0 ? nb : 1, I * kPartBlocks);
  p = p > 16 ? 16 : p;
  while (p > 1 && p * n * n * es > kPartBytes) --p;
  g.parts = (int)p;
  return g;
}

// One workgroup: mode index i (blockIdx.y), one (j range, a tile, b tile) (blockIdx.x), one part of i's block list (blockIdx.z).
// Per pass over kCh blocks of the list: (1) every wave scans the columns of its blocks from the block itself to the column's end
// (the partners with j >= i) and notes the ones inside the j range, (2) one thread per j compacts its matches in list order,
// (3) every thread applies the matches of its elements' j: acc += V_ci[a] * V_cj[b].
template <typename T>
__global__ void __launch_bounds__(kThreads) sparse_gram_kernel(GramGeom g, int64_t nb, int64_t C,
                                                               const int32_t* __restrict__ colptr,
                                                               const int32_t* __restrict__ blk_i,
                                                               const int32_t* __restrict__ blkcol,
                                                               const int32_t* __restrict__ ilist,
                                                               const int32_t* __restrict__ iptr, const T* __restrict__ V,
                                                               int64_t ldv, T* __restrict__ Gp) {
  __shared__ int s_partner[kCh * kJtMax];
  __shared__ int s_lp[kJtMax * kLs];
  __shared__ unsigned char s_lch[kJtMax * kLs];
  __shared__ int s_cnt[kJtMax];
  __shared__ T s_vi[kCh * kRt];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.y, part = blockIdx.z;
  int t = blockIdx.x;
  const int tb = t % g.nTB;
  t /= g.nTB;
  const int ta = t % g.nTA, tj = t / g.nTA;
  const int j0 = tj * g.Jt, a0 = ta * g.TA, b0 = tb * g.TB;
  const int jn = min(g.Jt, g.I - j0), an = min(g.TA, g.r - a0), bn = min(g.TB, g.r - b0);
  if (j0 + jn - 1 < i) return;  // j < i: mirrored by the finishing kernel

  const int E = g.Jt * g.TA * g.TB;
  T acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = T(0);

  int64_t q_lo = iptr[i], q_hi = iptr[i + 1];
  q_lo = q_lo < 0 ? 0 : q_lo;
  q_hi = q_hi > nb ? nb : q_hi;
  const int64_t len = q_hi > q_lo ? q_hi - q_lo : 0;
  const int64_t per = (len + g.parts - 1) / g.parts;
  const int64_t qs = q_lo + (int64_t)part * per;
  const int64_t qe = qs + per < q_hi ? qs + per : q_hi;

  for (int64_t q0 = qs; q0 < qe; q0 += kCh) {
    const int nch = (int)(qe - q0 < kCh ? qe - q0 : kCh);
    for (int x = tid; x < kCh * kJtMax; x += kThreads) s_partner[x] = -1;
    for (int x = tid; x < nch * g.TA; x += kThreads) {
      const int ch = x / g.TA, aa = x % g.TA;
      const int64_t B = ilist[q0 + ch];
      s_vi[ch * kRt + aa] = (aa < an && B >= 0 && B < nb) ? V[B * ldv + a0 + aa] : T(0);
    }
    __syncthreads();
    for (int ch = wave; ch < nch; ch += kThreads / kWave) {
      const int64_t B = ilist[q0 + ch];
      if (B < 0 || B >= nb) continue;
      const int64_t c = blkcol[B];
      if (c < 0 || c >= C) continue;
      int64_t end = colptr[c + 1];
      end = end > nb ? nb : end;
      for (int64_t Bp = B + lane; Bp < end; Bp += kWave) {
        const int64_t j = blk_i[Bp];
        if (j >= j0 + jn) break;  // ascending inside a column
        if (j >= j0 && j >= i) s_partner[ch * kJtMax + (int)(j - j0)] = (int)Bp;
      }
    }
    __syncthreads();
    if (tid < jn) {
      int n = 0;
      for (int ch = 0; ch < nch; ++ch) {
        const int p = s_partner[ch * kJtMax + tid];
        if (p >= 0) {
          s_lp[tid * kLs + n] = p;
          s_lch[tid * kLs + n] = (unsigned char)ch;
          ++n;
        }
      }
      s_cnt[tid] = n;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
      const int e = tid + k * kThreads;
      if (e < E) {
        const int bb = e % g.TB, aa = (e / g.TB) % g.TA, jj = e / (g.TB * g.TA);
        if (jj < jn && aa < an && bb < bn) {
          const int n = s_cnt[jj];
          T s = acc[k];
          for (int m = 0; m < n; ++m) {
            const int p = s_lp[jj * kLs + m], ch = s_lch[jj * kLs + m];
            s = fma(s_vi[ch * kRt + aa], V[(int64_t)p * ldv + b0 + bb], s);
          }
          acc[k] = s;
        }
      }
    }
    __syncthreads();
  }

  const int64_t n = (int64_t)g.r * g.I;
  T* out = Gp + (int64_t)part * n * n;
#pragma unroll
  for (int k = 0; k < kAcc; ++k) {
    const int e = tid + k * kThreads;
    if (e < E) {
      const int bb = e % g.TB, aa = (e / g.TB) % g.TA, jj = e / (g.TB * g.TA);
      if (jj < jn && aa < an && bb < bn)
        out[((int64_t)(a0 + aa) * g.I + i) * n + (int64_t)(b0 + bb) * g.I + j0 + jj] = acc[k];
    }
  }
}

// G[R][Cc] = sum over the parts, in part order, of the computed element: (R, Cc) itself where j >= i, its mirror image otherwise.
// (i == j blocks are computed on both sides of the diagonal from the same products in the same order.)
template <typename T>
__global__ void __launch_bounds__(kThreads) sparse_gram_finish_kernel(int I, int64_t n, int parts, const T* __restrict__ Gp,
                                                                      T* __restrict__ G, int64_t ldg) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= n * n) return;
  const int64_t R = idx / n, Cc = idx % n;
  const int64_t src = (Cc % I) >= (R % I) ? R * n + Cc : Cc * n + R;
  T s = Gp[src];
  for (int p = 1; p < parts; ++p) s += Gp[(int64_t)p * n * n + src];
  G[R * ldg + Cc] = s;
}

// W[c][k] = sum over the blocks b of column c (ascending mode index), a = 0 .. r-1, of V[b][a] * U[a * I + blk_i[b]][k].
// min(q, 256) threads per column, consecutive threads on consecutive k (U's rows are read coalesced).
template <typename T>
__global__ void __launch_bounds__(kThreads) sparse_project_kernel(int r, int I, int q, int64_t nb, int64_t C,
                                                                  const int32_t* __restrict__ colptr,
                                                                  const int32_t* __restrict__ blk_i, const T* __restrict__ V,
                                                                  int64_t ldv, const T* __restrict__ U, int64_t su_row,
                                                                  int64_t su_col, T* __restrict__ W, int64_t ldw) {
  const int qq = q < kThreads ? q : kThreads, cpw = kThreads / qq;
  const int lc = threadIdx.x / qq, k0 = threadIdx.x % qq;
  const int64_t c = (int64_t)blockIdx.x * cpw + lc;
  if (lc >= cpw || c >= C) return;
  int64_t b_lo = colptr[c], b_hi = colptr[c + 1];
  b_lo = b_lo < 0 ? 0 : b_lo;
  b_hi = b_hi > nb ? nb : b_hi;
  for (int k = k0; k < q; k += qq) {
    T s = T(0);
    for (int64_t b = b_lo; b < b_hi; ++b) {
      const int64_t i = blk_i[b];
      if (i < 0 || i >= I) continue;
      const T* v = V + b * ldv;
      const T* u = U + i * su_row + (int64_t)k * su_col;
      for (int a = 0; a < r; ++a) s = fma(v[a], u[(int64_t)a * I * su_row], s);
    }
    W[c * ldw + k] = s;
  }
}

__global__ void __launch_bounds__(kThreads) sparse_validate_kernel(int64_t P, int N, const int64_t* __restrict__ X, int64_t sx0,
                                                                   int64_t sx1, const int64_t* __restrict__ shape,
                                                                   int32_t* flag) {
  const int64_t total = P * N;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int n = (int)(e % N);
    const int64_t x = X[(e / N) * sx0 + n * sx1];
    bad |= x < 0 || x >= shape[n];
  }
  if (bad) atomicOr(flag, 1);
}

// key = ((x_N I_{N-1} + x_{N-1}) ... ) I_1 + x_1: x_N is the major key, x_1 the minor one
__global__ void __launch_bounds__(kThreads) sparse_keys_kernel(int64_t P, int N, const int64_t* __restrict__ X, int64_t sx0,
                                                               int64_t sx1, const int64_t* __restrict__ shape,
                                                               const int32_t* __restrict__ flag, int64_t* __restrict__ key) {
  if (*flag & 1) return;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  int64_t k = 0;
  for (int n = N - 1; n >= 0; --n) k = k * shape[n] + X[p * sx0 + n * sx1];
  key[p] = k;
}

// lev[p] = the deepest mode (1-based) in which sorted sample p differs from sorted sample p - 1; N for p = 0; 0 (and flag bit 1)
// for a repeated position.  Sample p of the sorted order is row perm[p] of X.
__global__ void __launch_bounds__(kThreads) sparse_levels_kernel(int64_t P, int N, const int64_t* __restrict__ X, int64_t sx0,
                                                                 int64_t sx1, const int32_t* __restrict__ perm,
                                                                 int32_t* __restrict__ lev, int32_t* flag) {
  if (*flag & 1) return;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  int l = N;
  if (p > 0) {
    const int64_t r0 = perm[p], r1 = perm[p - 1];
    if (r0 < 0 || r0 >= P || r1 < 0 || r1 >= P) {
      atomicOr(flag, 1);
      return;
    }
    l = 0;
    for (int n = N - 1; n >= 0; --n)
      if (X[r0 * sx0 + n * sx1] != X[r1 * sx0 + n * sx1]) {
        l = n + 1;
        break;
      }
    if (l == 0) atomicOr(flag, 2);
  }
  lev[p] = l;
}


// ------------------------------------------------------------------ grouping the blocks by mode index (stable counting sort)
constexpr int kGroupMaxI = 4096;  // bins held in LDS

int64_t group_chunk(int64_t nb) {  // blocks per workgroup: at most 1024 chunks
  const int64_t c = ceil_div(nb > 0 ? nb : 1, 1024);
  return align_up(c < 4096 ? 4096 : c, kThreads);
}

// hist[chunk][i] = blocks of the chunk at mode index i
__global__ void __launch_bounds__(kThreads) sparse_group_count_kernel(int64_t nb, int I, int64_t chunk,
                                                                      const int32_t* __restrict__ blk_i,
                                                                      int32_t* __restrict__ hist) {
  __shared__ int s_h[kGroupMaxI];
  for (int x = threadIdx.x; x < I; x += kThreads) s_h[x] = 0;
  __syncthreads();
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
  for (int64_t b = b0 + threadIdx.x; b < b1; b += kThreads) {
    const int v = blk_i[b];
    if (v >= 0 && v < I) atomicAdd(&s_h[v], 1);
  }
  __syncthreads();
  for (int x = threadIdx.x; x < I; x += kThreads) hist[(int64_t)blockIdx.x * I + x] = s_h[x];
}

// One workgroup: hist[chunk][i] <- iptr[i] + blocks at i in the chunks before; iptr[I + 1] = the groups
__global__ void __launch_bounds__(kThreads) sparse_group_scan_kernel(int I, int nchunks, int32_t* __restrict__ hist,
                                                                     int32_t* __restrict__ iptr) {
  __shared__ int s_t[kGroupMaxI + 1];
  for (int i = threadIdx.x; i < I; i += kThreads) {
    int run = 0;
    for (int c = 0; c < nchunks; ++c) {
      const int h = hist[(int64_t)c * I + i];
      hist[(int64_t)c * I + i] = run;
      run += h;
    }
    s_t[i] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < I; ++i) {
      const int h = s_t[i];
      s_t[i] = run;
      run += h;
    }
    s_t[I] = run;
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= I; i += kThreads) iptr[i] = s_t[i];
  for (int i = threadIdx.x; i < I; i += kThreads) {
    const int base = s_t[i];
    for (int c = 0; c < nchunks; ++c) hist[(int64_t)c * I + i] += base;
  }
}

// ilist[position] = block, in block order within a mode index: 256 blocks at a time, each thread ranks its block among the
// earlier ones of the same mode index in the tile
__global__ void __launch_bounds__(kThreads) sparse_group_scatter_kernel(int64_t nb, int I, int64_t chunk,
                                                                        const int32_t* __restrict__ blk_i,
                                                                        const int32_t* __restrict__ hist,
                                                                        int32_t* __restrict__ ilist) {
  __shared__ int s_off[kGroupMaxI];
  __shared__ int s_v[kThreads];
  for (int x = threadIdx.x; x < I; x += kThreads) s_off[x] = hist[(int64_t)blockIdx.x * I + x];
  __syncthreads();
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
  for (int64_t t0 = b0; t0 < b1; t0 += kThreads) {
    const int64_t b = t0 + threadIdx.x;
    int v = -1;
    if (b < b1) {
      v = blk_i[b];
      if (v < 0 || v >= I) v = -1;
    }
    s_v[threadIdx.x] = v;
    __syncthreads();
    int before = 0, after = 0;
    if (v >= 0) {
      for (int k = 0; k < kThreads; ++k) {
        const int same = s_v[k] == v;
        before += same && k < (int)threadIdx.x;
        after += same && k > (int)threadIdx.x;
      }
      const int pos = s_off[v] + before;
      if (pos >= 0 && pos < nb) ilist[pos] = (int32_t)b;
    }
    __syncthreads();
    if (v >= 0 && after == 0) s_off[v] += before + 1;  // the last block of its mode index in the tile
    __syncthreads();
  }
}

}  // namespace
}  // namespace ttr

using namespace ttr;

extern "C" int ttr_sparse_keys(int64_t P, int64_t N, const void* X, int64_t sx0, int64_t sx1, const void* shape, void* key,
                               void* flag, void* stream) {
  TTR_REQUIRE(P >= 0 && N >= 1, TTR_E_INVALID, "ttr_sparse_keys: bad sizes");
  TTR_REQUIRE(N < ((int64_t)1 << 20) && P < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_sparse_keys: too many modes or samples");
  TTR_REQUIRE(flag, TTR_E_INVALID, "ttr_sparse_keys: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) {
    TTR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    return TTR_OK;
  }
  TTR_REQUIRE(X && shape, TTR_E_INVALID, "ttr_sparse_keys: NULL argument");
  TTR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
  int64_t nblk = ceil_div(P * N, kThreads);
  nblk = nblk > 4096 ? 4096 : nblk;
  hipLaunchKernelGGL(sparse_validate_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, s, P, (int)N, (const int64_t*)X, sx0, sx1,
                     (const int64_t*)shape, (int32_t*)flag);
  if (key)
    hipLaunchKernelGGL(sparse_keys_kernel, dim3((unsigned)ceil_div(P, kThreads)), dim3(kThreads), 0, s, P, (int)N,
                       (const int64_t*)X, sx0, sx1, (const int64_t*)shape, (const int32_t*)flag, (int64_t*)key);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

extern "C" int ttr_sparse_levels(int64_t P, int64_t N, const void* X, int64_t sx0, int64_t sx1, const void* perm, void* lev,
                                 void* flag, void* stream) {
  TTR_REQUIRE(P >= 0 && N >= 1, TTR_E_INVALID, "ttr_sparse_levels: bad sizes");
  TTR_REQUIRE(N < ((int64_t)1 << 20) && P < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_sparse_levels: too many modes or samples");
  if (P == 0) return TTR_OK;
  TTR_REQUIRE(X && perm && lev && flag, TTR_E_INVALID, "ttr_sparse_levels: NULL argument");
  hipLaunchKernelGGL(sparse_levels_kernel, dim3((unsigned)ceil_div(P, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, P,
                     (int)N, (const int64_t*)X, sx0, sx1, (const int32_t*)perm, (int32_t*)lev, (int32_t*)flag);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

extern "C" int64_t ttr_sparse_group_workspace_bytes(int64_t nb, int64_t I) {
  TTR_REQUIRE(nb >= 0 && I >= 1, TTR_E_INVALID, "ttr_sparse_group_workspace_bytes: bad sizes");
  TTR_REQUIRE(I <= kGroupMaxI && nb < ((int64_t)1 << 31), TTR_E_UNSUPPORTED,
              "ttr_sparse_group_workspace_bytes: I = %lld above %d, or too many blocks", (long long)I, kGroupMaxI);
  return ceil_div(nb > 0 ? nb : 1, group_chunk(nb)) * I * (int64_t)sizeof(int32_t);
}

extern "C" int ttr_sparse_group(int64_t nb, int64_t I, const void* blk_i, void* ilist, void* iptr, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  const int64_t need = ttr_sparse_group_workspace_bytes(nb, I);
  if (need < 0) return (int)need;
  TTR_REQUIRE(iptr && workspace && (nb == 0 || (blk_i && ilist)), TTR_E_INVALID, "ttr_sparse_group: NULL argument");
  TTR_REQUIRE(workspace_bytes >= need, TTR_E_WORKSPACE, "ttr_sparse_group: workspace too small");
  const int64_t chunk = group_chunk(nb), nchunks = ceil_div(nb > 0 ? nb : 1, chunk);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sparse_group_count_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, nb, (int)I, chunk,
                     (const int32_t*)blk_i, (int32_t*)workspace);
  hipLaunchKernelGGL(sparse_group_scan_kernel, dim3(1), dim3(kThreads), 0, s, (int)I, (int)nchunks, (int32_t*)workspace,
                     (int32_t*)iptr);
  if (nb > 0)
    hipLaunchKernelGGL(sparse_group_scatter_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, nb, (int)I, chunk,
                       (const int32_t*)blk_i, (const int32_t*)workspace, (int32_t*)ilist);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

static int sparse_gram_check(const char* who, int dtype, int64_t r, int64_t I, int64_t nb) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(r >= 1 && I >= 1 && nb >= 0, TTR_E_INVALID, "%s: bad sizes", who);
  const int64_t lim = ttr_eigh_max_n(dtype);
  TTR_REQUIRE(r <= lim && I <= lim && r * I <= lim, TTR_E_UNSUPPORTED, "%s: r * I = %lld above %lld", who, (long long)(r * I),
              (long long)lim);
  TTR_REQUIRE(nb < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "%s: too many blocks", who);
  return TTR_OK;
}

extern "C" int64_t ttr_sparse_gram_parts(int dtype, int64_t r, int64_t I, int64_t nb) {
  const int st = sparse_gram_check("ttr_sparse_gram_parts", dtype, r, I, nb);
  if (st != TTR_OK) return st;
  return gram_geom(dtype, r, I, nb).parts;
}

extern "C" int64_t ttr_sparse_gram_workspace_bytes(int dtype, int64_t r, int64_t I, int64_t nb) {
  const int st = sparse_gram_check("ttr_sparse_gram_workspace_bytes", dtype, r, I, nb);
  if (st != TTR_OK) return st;
  const int64_t n = r * I;
  return gram_geom(dtype, r, I, nb).parts * n * n * elem_size(dtype);
}

template <typename T>
static void sparse_gram_launch(const GramGeom& g, int64_t nb, int64_t C, const void* colptr, const void* blk_i,
                               const void* blkcol, const void* ilist, const void* iptr, const void* V, int64_t ldv, void* G,
                               int64_t ldg, void* ws, hipStream_t s) {
  const int64_t n = (int64_t)g.r * g.I;
  const dim3 grid((unsigned)(g.nJ * g.nTA * g.nTB), (unsigned)g.I, (unsigned)g.parts);
  hipLaunchKernelGGL(sparse_gram_kernel<T>, grid, dim3(kThreads), 0, s, g, nb, C, (const int32_t*)colptr, (const int32_t*)blk_i,
                     (const int32_t*)blkcol, (const int32_t*)ilist, (const int32_t*)iptr, (const T*)V, ldv, (T*)ws);
  hipLaunchKernelGGL(sparse_gram_finish_kernel<T>, dim3((unsigned)ceil_div(n * n, kThreads)), dim3(kThreads), 0, s, g.I, n,
                     g.parts, (const T*)ws, (T*)G, ldg);
}

extern "C" int ttr_sparse_gram(int dtype, int64_t r, int64_t I, int64_t nb, int64_t C, const void* colptr, const void* blk_i,
                               const void* blkcol, const void* ilist, const void* iptr, const void* V, int64_t ldv, void* G,
                               int64_t ldg, void* workspace, int64_t workspace_bytes, void* stream) {
  const int st = sparse_gram_check("ttr_sparse_gram", dtype, r, I, nb);
  if (st != TTR_OK) return st;
  TTR_REQUIRE(C >= 0 && C <= nb && ldv >= r && ldg >= r * I, TTR_E_INVALID, "ttr_sparse_gram: bad sizes");
  TTR_REQUIRE(colptr && blk_i && blkcol && ilist && iptr && V && G && workspace, TTR_E_INVALID,
              "ttr_sparse_gram: NULL argument");
  const GramGeom g = gram_geom(dtype, r, I, nb);
  const int64_t n = r * I;
  TTR_REQUIRE(workspace_bytes >= g.parts * n * n * elem_size(dtype), TTR_E_WORKSPACE,
              "ttr_sparse_gram: workspace too small");
  TTR_REQUIRE((int64_t)g.nJ * g.nTA * g.nTB < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_sparse_gram: too many tiles");
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) { sparse_gram_launch<decltype(t)>(g, nb, C, colptr, blk_i, blkcol, ilist, iptr, V, ldv, G, ldg, workspace, s); });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

extern "C" int ttr_sparse_project(int dtype, int64_t r, int64_t I, int64_t q, int64_t nb, int64_t C, const void* colptr,
                                  const void* blk_i, const void* V, int64_t ldv, const void* U, int64_t su_row, int64_t su_col,
                                  void* W, int64_t ldw, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_sparse_project: bad dtype %d", dtype);
  TTR_REQUIRE(r >= 1 && I >= 1 && q >= 1 && nb >= 0 && C >= 0 && C <= nb && ldv >= r && ldw >= q, TTR_E_INVALID,
              "ttr_sparse_project: bad sizes");
  const int64_t lim = ttr_eigh_max_n(dtype);
  TTR_REQUIRE(r <= lim && I <= lim && r * I <= lim && q <= r * I, TTR_E_UNSUPPORTED,
              "ttr_sparse_project: r * I = %lld above %lld, or q above r * I", (long long)(r * I), (long long)lim);
  TTR_REQUIRE(nb < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_sparse_project: too many blocks");
  if (C == 0) return TTR_OK;
  TTR_REQUIRE(colptr && blk_i && V && U && W, TTR_E_INVALID, "ttr_sparse_project: NULL argument");
  const int64_t qq = q < kThreads ? q : kThreads, cpw = kThreads / qq;
  const dim3 grid((unsigned)ceil_div(C, cpw));
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(sparse_project_kernel<T>, grid, dim3(kThreads), 0, s, (int)r, (int)I, (int)q, nb, C, (const int32_t*)colptr,
                       (const int32_t*)blk_i, (const T*)V, ldv, (const T*)U, su_row, su_col, (T*)W, ldw);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}
