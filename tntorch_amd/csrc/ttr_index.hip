// ttr_gather_chain: batched TT point evaluation (the index-array block of tensor.py:1019-1434).
//
//   out[b, :, p, :] = G_a[b][:, i_a[p], :] @ G_{a+1}[b][:, i_{a+1}[p], :] @ ... @ G_z[b][:, i_z[p], :]
//
// The reference evaluates this with one einsum per mode over the gathered slices [r, P, r'] (tensor.py:1357-1378): every point
// re-reads a whole R x R' slice of every core.  Here the running product X (one row per (point, r_a-row) pair) is carried from
// mode to mode, and for each mode the points are grouped by their index value with a device counting sort (histogram, scan,
// scatter of point ids).  A step then multiplies 64 gathered X rows that share one index value by that value's slice, staged
// once per tile in LDS: a slice is read once per tile of 64 rows instead of once per point.
//
// Small P skips the sort: the same step kernel takes one tile per point (the "direct" path).  Every output element is the FMA
// chain over k = 0 .. r-1 of its own row and the slice column, in that order, in both paths, so a point's value does not depend
// on which other points share the call or on the path taken.
//
// Index validation: the first pass checks every index of every mode (-I <= i < I, negative values wrap as in torch) and ORs a
// device word; every later kernel returns at entry when the word is set, so out-of-range input writes nothing but that word.
#include "detail/ttr_internal.h"
#include "detail/ttr_group.h"

namespace ttr {
namespace {

// (IdxCol, the validation and the counting sort -- histogram, scan, scatter -- live in detail/ttr_group.h, shared with
// ttr_ttlookup.hip)
constexpr int kTileRows = kGroupTileRows;   // X rows per step tile
constexpr int kTileCols = 64;   // output columns per step tile
constexpr int kTileK = 32;      // k chunk staged in LDS

// X[b, p, i, :] = G[b, i, v(p), :]  (first mode of the chain)
template <typename T>
__global__ void __launch_bounds__(kThreads) gather_kernel(const T* __restrict__ G, int64_t gb, int64_t gr, int64_t gi, int64_t gj,
                                                          IdxCol c, int64_t P, int64_t I, int64_t ra, int64_t rb, T* __restrict__ X,
                                                          int64_t xb, int64_t xp, int64_t xi, int64_t xj, const int32_t* flag) {
  if (*flag) return;
  const int64_t b = blockIdx.y;
  const int64_t n = P * ra * rb;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
    int64_t j = e % rb, row = e / rb, i = row % ra, p = row / ra;
    int64_t v = idx_value(c, p, I);
    if (v < 0) continue;
    X[b * xb + p * xp + i * xi + j * xj] = G[b * gb + i * gr + v * gi + j * gj];
  }
}

// Y[row] = X[row] @ G[b][:, v, :] for the X rows of one tile (all with index value v): 64 rows x 64 columns per workgroup, k in
// chunks of 32 through LDS, 4 x 4 outputs per thread.  Every output is fma(x[k], s[k][j], acc) for k = 0, 1, ..., r - 1.
// direct: tile t covers rows [t_in_point * 64, ...) of point t / tiles_per_point, no permutation.
// xmap (ttr_gather_step; NULL otherwise): point p reads X point xmap[p] instead of p.
template <typename T>
__global__ void __launch_bounds__(kThreads) step_kernel(const T* __restrict__ X, int64_t xb, int64_t xp, int64_t xi,
                                                        const T* __restrict__ G, int64_t gb, int64_t gr, int64_t gi, int64_t gj,
                                                        IdxCol c, int64_t P, int64_t I, int64_t ra, int64_t r, int64_t rn,
                                                        T* __restrict__ Y, int64_t yb, int64_t yp, int64_t yi, int64_t yj, int direct,
                                                        const int32_t* cnt, const int64_t* off, const int64_t* toff,
                                                        const int64_t* perm, const int32_t* flag, const int64_t* xmap) {
  __shared__ T xs[kTileK][kTileRows + 4];
  __shared__ T ss[kTileK][kTileCols + 4];
  __shared__ int64_t xrow[kTileRows], yrow[kTileRows];
  __shared__ int64_t s_v;
  if (*flag) return;
  const int64_t t = blockIdx.x, b = blockIdx.z, j0 = (int64_t)blockIdx.y * kTileCols;
  int64_t v, rbeg, rend;  // tile rows [rbeg, rend) in grouped row space; row -> point (perm) * ra + i
  if (direct) {
    const int64_t tpp = (ra + kTileRows - 1) / kTileRows;
    const int64_t p = t / tpp;
    if (p >= P) return;
    rbeg = p * ra + (t % tpp) * kTileRows;
    rend = min(rbeg + kTileRows, (p + 1) * ra);
    v = idx_value(c, p, I);
  } else {
    if (t >= toff[I]) return;
    v = group_of_tile(toff, I, t, &s_v);
    rbeg = off[v] * ra + (t - toff[v]) * kTileRows;
    rend = min(rbeg + kTileRows, (off[v] + cnt[v]) * ra);
  }
  const int tid = threadIdx.x;
  if (tid < kTileRows) {
    int64_t row = rbeg + tid;
    if (row < rend) {
      int64_t q = row / ra, i = row % ra;
      int64_t p = direct ? q : perm[q];
      xrow[tid] = b * xb + (xmap ? xmap[p] : p) * xp + i * xi;
      yrow[tid] = b * yb + p * yp + i * yi;
    } else {
      xrow[tid] = yrow[tid] = -1;
    }
  }
  const T* Gs = G + b * gb + v * gi;
  const int tx = tid & 15, ty = tid >> 4;
  T acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[a][d] = T(0);
  for (int64_t k0 = 0; k0 < r; k0 += kTileK) {
    const int kn = (int)min((int64_t)kTileK, r - k0);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kTileRows * kTileK / kThreads; ++e) {
      int idx = e * kThreads + tid, row = idx / kTileK, k = idx % kTileK;
      int64_t base = xrow[row];
      xs[k][row] = (base >= 0 && k < kn) ? X[base + k0 + k] : T(0);
    }
#pragma unroll
    for (int e = 0; e < kTileK * kTileCols / kThreads; ++e) {
      int idx = e * kThreads + tid, k = idx / kTileCols, j = idx % kTileCols;
      ss[k][j] = (k < kn && j0 + j < rn) ? Gs[(k0 + k) * gr + (j0 + j) * gj] : T(0);
    }
    __syncthreads();
    for (int k = 0; k < kn; ++k) {
      T xv[4], sv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xv[a] = xs[k][ty * 4 + a];
#pragma unroll
      for (int d = 0; d < 4; ++d) sv[d] = ss[k][tx * 4 + d];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[a][d] = fma(xv[a], sv[d], acc[a][d]);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int64_t base = yrow[ty * 4 + a];
    if (base < 0) continue;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      int64_t j = j0 + tx * 4 + d;
      if (j < rn) Y[base + j * yj] = acc[a][d];
    }
  }
}

constexpr int64_t kMaxRank = 512;
constexpr int64_t kDefaultDirectMax = 1024;  // tools/index_bench.py --direct-sweep: direct 0.23 ms vs sorted 0.25 ms at P = 1024, 0.44 vs 0.27 at 4096

struct Layout {
  int64_t x0, x1, cnt, cursor, off, toff, perm, total;
};

Layout layout(int64_t esize, int64_t nmodes, const int64_t* ranks, const int64_t* sizes, int64_t P, int64_t batch) {
  int64_t ra = ranks[0], wmax = 0, Imax = 1;
  for (int64_t n = 1; n < nmodes; ++n) wmax = std::max(wmax, ranks[n]);  // widths of the intermediate products
  for (int64_t n = 0; n < nmodes; ++n) Imax = std::max(Imax, sizes[n]);
  Layout L{};
  int64_t xbytes = nmodes > 1 ? align256(batch * P * ra * wmax * esize) : 0;
  int64_t o = 0;
  L.x0 = o; o += xbytes;
  L.x1 = o; o += nmodes > 2 ? xbytes : 0;
  L.cnt = o; o += align256(Imax * 4);
  L.cursor = o; o += align256(Imax * 4);
  L.off = o; o += align256(Imax * 8);
  L.toff = o; o += align256((Imax + 1) * 8);
  L.perm = o; o += align256(std::max<int64_t>(P, 1) * 8);
  L.total = o;
  return L;
}

template <typename T>
int gather_chain_impl(int64_t nmodes, int64_t batch, int64_t P, const int64_t* ranks, const int64_t* sizes,
                      const void* const* cores, const int64_t* cs, int idx_dtype, const void* const* idx, const int64_t* idx_strides,
                      void* out, int64_t ob, int64_t orr, int64_t op, int64_t oc, int64_t direct_max, int32_t* flag,
                      char* ws, const Layout& L, hipStream_t stream) {
  TTR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int32_t), stream));
  const unsigned pb = (unsigned)((P + kThreads - 1) / kThreads);
  for (int64_t n = 0; n < nmodes; ++n) {
    IdxCol c{idx[n], idx_strides[n], idx_dtype};
    hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, stream, c, P, sizes[n], flag, 1);
  }
  const bool direct = P <= (direct_max < 0 ? kDefaultDirectMax : direct_max);
  const int64_t ra = ranks[0];
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int32_t* cursor = (int32_t*)(ws + L.cursor);
  int64_t* off = (int64_t*)(ws + L.off);
  int64_t* toff = (int64_t*)(ws + L.toff);
  int64_t* perm = (int64_t*)(ws + L.perm);
  T* X = nullptr;
  int64_t xb = 0, xp = 0, xi = 0;
  for (int64_t n = 0; n < nmodes; ++n) {
    const T* G = (const T*)cores[n];
    const int64_t* g = cs + 4 * n;
    const int64_t r = ranks[n], rn = ranks[n + 1], I = sizes[n];
    IdxCol c{idx[n], idx_strides[n], idx_dtype};
    const bool last = n == nmodes - 1;
    // destination of this mode: `out` for the last one, else an X buffer [B, P, ra, rn] (ping-pong)
    T* Y = last ? (T*)out : (T*)(ws + (n % 2 == 0 ? L.x0 : L.x1));
    int64_t yb = last ? ob : P * ra * rn, yp = last ? op : ra * rn, yi = last ? orr : rn, yj = last ? oc : 1;
    if (n == 0) {
      int64_t elems = P * ra * rn;
      unsigned gx = (unsigned)std::min<int64_t>((elems + kThreads - 1) / kThreads, 65536);
      hipLaunchKernelGGL(gather_kernel<T>, dim3(gx, (unsigned)batch), dim3(kThreads), 0, stream, G, g[0], g[1], g[2], g[3], c, P,
                         I, ra, rn, Y, yb, yp, yi, yj, flag);
    } else {
      int64_t tiles;
      if (direct) {
        tiles = P * ((ra + kTileRows - 1) / kTileRows);
      } else {
        TTR_HIP_CHECK(hipMemsetAsync(cnt, 0, I * sizeof(int32_t), stream));
        TTR_HIP_CHECK(hipMemsetAsync(cursor, 0, I * sizeof(int32_t), stream));
        enqueue_group_sort(c, P, I, ra, cnt, cursor, off, toff, perm, flag, stream);
        tiles = (P * ra + kTileRows - 1) / kTileRows + I;  // upper bound: blocks past toff[I] return at once
      }
      dim3 grid((unsigned)tiles, (unsigned)((rn + kTileCols - 1) / kTileCols), (unsigned)batch);
      hipLaunchKernelGGL(step_kernel<T>, grid, dim3(kThreads), 0, stream, X, xb, xp, xi, G, g[0], g[1], g[2], g[3], c, P, I, ra,
                         r, rn, Y, yb, yp, yi, yj, direct ? 1 : 0, cnt, off, toff, perm, flag, (const int64_t*)nullptr);
    }
    X = Y;
    xb = yb;
    xp = yp;
    xi = yi;
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace
}  // namespace ttr

using namespace ttr;

extern "C" int64_t ttr_gather_chain_workspace_bytes(int dtype, int64_t nmodes, const int64_t* ranks, const int64_t* sizes,
                                                    int64_t P, int64_t batch) {
  if (!dtype_ok(dtype) || nmodes < 1 || !ranks || !sizes || P < 0 || batch < 1) return -1;
  return layout(elem_size(dtype), nmodes, ranks, sizes, P, batch).total;
}

extern "C" int ttr_gather_chain(int dtype, int64_t nmodes, int64_t batch, int64_t P, const int64_t* ranks, const int64_t* sizes,
                                const void* const* cores, const int64_t* core_strides, int idx_dtype, const void* const* idx,
                                const int64_t* idx_strides, void* out, int64_t stride_ob, int64_t stride_or, int64_t stride_op,
                                int64_t stride_oc, int64_t direct_max_points, void* oob_flag, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_gather_chain: bad dtype %d", dtype);
  TTR_REQUIRE(idx_dtype == 0 || idx_dtype == 1, TTR_E_INVALID, "ttr_gather_chain: idx_dtype must be 0 (int32) or 1 (int64)");
  TTR_REQUIRE(nmodes >= 1 && batch >= 1 && P >= 0, TTR_E_INVALID, "ttr_gather_chain: bad sizes (nmodes %lld, batch %lld, P %lld)",
              (long long)nmodes, (long long)batch, (long long)P);
  TTR_REQUIRE(ranks && sizes && cores && core_strides && idx && idx_strides && oob_flag, TTR_E_INVALID,
              "ttr_gather_chain: NULL argument");
  for (int64_t n = 0; n <= nmodes; ++n)
    TTR_REQUIRE(ranks[n] >= 1, TTR_E_INVALID, "ttr_gather_chain: rank %lld < 1", (long long)ranks[n]);
  for (int64_t n = 0; n < nmodes; ++n) {
    TTR_REQUIRE(sizes[n] >= 1, TTR_E_INVALID, "ttr_gather_chain: mode size %lld < 1", (long long)sizes[n]);
    // an empty device tensor has a null data pointer: with P == 0 no index column is read
    TTR_REQUIRE(cores[n] && (idx[n] || P == 0), TTR_E_INVALID, "ttr_gather_chain: NULL core or index column %lld", (long long)n);
    TTR_REQUIRE(sizes[n] < (int64_t)1 << 31, TTR_E_UNSUPPORTED, "ttr_gather_chain: mode size %lld", (long long)sizes[n]);
  }
  for (int64_t n = 0; n <= nmodes; ++n)
    TTR_REQUIRE(ranks[n] <= kMaxRank, TTR_E_UNSUPPORTED, "ttr_gather_chain: rank %lld above %lld", (long long)ranks[n],
                (long long)kMaxRank);
  TTR_REQUIRE(batch <= 65535, TTR_E_UNSUPPORTED, "ttr_gather_chain: batch %lld above 65535", (long long)batch);
  int64_t Imax = 0;
  for (int64_t n = 0; n < nmodes; ++n) Imax = std::max(Imax, sizes[n]);
  TTR_REQUIRE(P * ((ranks[0] + kTileRows - 1) / kTileRows) + Imax < ((int64_t)1 << 31), TTR_E_UNSUPPORTED,
              "ttr_gather_chain: too many points (%lld)", (long long)P);
  Layout L = layout(elem_size(dtype), nmodes, ranks, sizes, P, batch);
  TTR_REQUIRE(workspace && workspace_bytes >= L.total, TTR_E_WORKSPACE, "ttr_gather_chain: workspace %lld < %lld bytes",
              (long long)workspace_bytes, (long long)L.total);
  TTR_REQUIRE(out || P == 0, TTR_E_INVALID, "ttr_gather_chain: NULL output");
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) return hipMemsetAsync(oob_flag, 0, sizeof(int32_t), s) == hipSuccess ? TTR_OK : TTR_E_HIP;
  return by_dtype(dtype, [&](auto t) {
    return gather_chain_impl<decltype(t)>(nmodes, batch, P, ranks, sizes, cores, core_strides, idx_dtype, idx, idx_strides, out,
                                          stride_ob, stride_or, stride_op, stride_oc, direct_max_points, (int32_t*)oob_flag,
                                          (char*)workspace, L, s);
  });
}

// One step of the chain with a row map on its input (the interface update of TT-cross, cross.py:400-448):
//   Y[p, :] = X[xrow[p], :] @ G[:, idx[p], :]      X [rows_x, r] (row stride ldx), G [r, I, rn] (strides gr, gi, gj), Y [P, rn]
// xrow == NULL reads X[p].  Both index vectors (int64) are validated on the device first (idx wraps negative values as in
// torch, xrow does not: a row map entry must be in 0 .. rows_x-1); out-of-range input sets *oob_flag and writes nothing else.  The direct path of ttr_gather_chain (one tile per point), so no workspace and no host synchronisation.
extern "C" int ttr_gather_step(int dtype, int64_t P, int64_t rows_x, int64_t r, int64_t rn, int64_t I, const void* X, int64_t ldx,
                               const void* xrow, const void* G, int64_t gr, int64_t gi, int64_t gj, const void* idx, void* Y,
                               int64_t ldy, void* oob_flag, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_gather_step: bad dtype %d", dtype);
  TTR_REQUIRE(P >= 0 && rows_x >= 1 && r >= 1 && rn >= 1 && I >= 1, TTR_E_INVALID, "ttr_gather_step: bad sizes");
  TTR_REQUIRE(X && G && oob_flag && ((idx && Y) || P == 0), TTR_E_INVALID, "ttr_gather_step: NULL argument");
  TTR_REQUIRE(I < ((int64_t)1 << 31) && rows_x < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_gather_step: sizes too large");
  TTR_REQUIRE(r <= kMaxRank && rn <= kMaxRank, TTR_E_UNSUPPORTED, "ttr_gather_step: rank above %lld", (long long)kMaxRank);
  TTR_REQUIRE(P < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_gather_step: too many points (%lld)", (long long)P);
  hipStream_t s = (hipStream_t)stream;
  int32_t* flag = (int32_t*)oob_flag;
  TTR_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
  if (P == 0) return TTR_OK;
  const unsigned pb = (unsigned)((P + kThreads - 1) / kThreads);
  IdxCol c{idx, 1, 1};
  hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, s, c, P, I, flag, 1);
  if (xrow) {
    IdxCol cx{xrow, 1, 1};
    hipLaunchKernelGGL(validate_kernel, dim3(pb), dim3(kThreads), 0, s, cx, P, rows_x, flag, 0);  // no wrap: rows 0 .. rows_x-1
  }
  const dim3 grid((unsigned)P, (unsigned)((rn + kTileCols - 1) / kTileCols), 1);
  // (written out, not by_dtype: launched from a generic lambda here, the two step_kernel instances leave the compiler in the
  // other order, and the code object is kept byte-identical)
  if (dtype == TTR_F32)
    hipLaunchKernelGGL(step_kernel<float>, grid, dim3(kThreads), 0, s, (const float*)X, (int64_t)0, ldx, (int64_t)0, (const float*)G,
                       (int64_t)0, gr, gi, gj, c, P, I, (int64_t)1, r, rn, (float*)Y, (int64_t)0, ldy, (int64_t)0, (int64_t)1, 1,
                       (const int32_t*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr, flag,
                       (const int64_t*)xrow);
  else
    hipLaunchKernelGGL(step_kernel<double>, grid, dim3(kThreads), 0, s, (const double*)X, (int64_t)0, ldx, (int64_t)0,
                       (const double*)G, (int64_t)0, gr, gi, gj, c, P, I, (int64_t)1, r, rn, (double*)Y, (int64_t)0, ldy, (int64_t)0,
                       (int64_t)1, 1, (const int32_t*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr,
                       (const int64_t*)nullptr, flag, (const int64_t*)xrow);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}
