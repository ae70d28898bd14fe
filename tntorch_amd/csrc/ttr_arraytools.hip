// Array tools on one TT core (tools.py:266-325 `ttm` with a vector, ops.py:6-30 `cumsum`), streaming kernels for gfx950:
//   ttr_mode_scan    Y[r, i, c] = sum_{i' <= i} X[r, i', c]          the running sum along the middle axis of X [R, I, C]
//   ttr_mode_reduce  Y[r, c]    = scale * sum_i w[i] X[r, i, c]      the weighted reduction of that axis (w == NULL: ones)
//
// A core is R slabs of a row-major [I, C] matrix that is scanned / reduced down its columns.  A thread owns a PACK of P
// consecutive c of one row: P = 16 bytes of elements when C is a multiple of that, else 1 -- P follows from C and the dtype alone.
// When the pointers and the strides are multiples of 16 bytes too, a pack is one 16-byte load / store, else P scalar ones: the
// arithmetic is the same, so the bits of the result do not depend on where the buffers lie.
//
// A wave covers a TILE of tw <= 64 packs of a row (CP = C / P packs per row are cut into ceil(CP / 64) tiles of equal width) and
// g = 64 / tw consecutive rows at once: lane = (i_sub, c), a contiguous run of the slab for every C, down to C = 1 (the last
// core), where the 64 lanes are 64 consecutive i.  The g rows of a step are combined across lanes at lane distance tw -- a
// Hillis-Steele scan (__shfl_up) resp. a tree reduction (__shfl_down) -- and a step's carry is the last row of the step before
// (read from that lane).  kUnroll steps are loaded before the first is used: the loads do not wait for the carry chain.
//
// Where the items (r, tile) are too few to fill the device and the mode is long (a first core [1, 4096, 64]), the kSplitWaves
// waves of a workgroup take contiguous chunks of I of one item: every wave sums its chunk, the chunk totals pass through LDS, and
// a wave adds the totals of the earlier chunks, in chunk order, as the carry it starts its scan with (the scan reads its chunk a
// second time: from the cache, the chunk of a wave was just read) resp. wave 0 adds all of them and stores.  While such a launch
// has fewer than kSplitItems workgroups, the tiles are halved (down to one pack: g = 64 rows per step, runs of 16 bytes a row
// apart) as long as every wave keeps a full step: [1, 4096, 64] in fp32 is 16 workgroups instead of one.  No workgroup talks
// to another, nothing is atomic, there is no scratch: tiling, chunks and with them the order of every sum follow from (R, I, C)
// and the dtype alone.  Both dtypes accumulate in fp64 registers and round once, at the store.  Rows outside a wave's chunk and
// packs outside the tile are never loaded or stored; every extent and stride comes from validated host arguments.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int kSplitWaves = 16;        // waves of a workgroup that share one item along I (the split kernels: 1024 threads)
constexpr int kUnroll = 4;             // steps of g rows in flight per wave
constexpr int64_t kMaxBlocks = 2048;   // 256 CUs x 8 blocks; the rest of the items is walked with a grid stride
constexpr int64_t kEnoughItems = 1024; // one wave per SIMD of the device: from here on an item is one wave's
constexpr int64_t kSplitItems = 256;   // the split kernels: one workgroup per CU; below it the tiles are narrowed

template <typename T>
struct ArrArgs {
  int64_t R, I, C;
  const T* X;
  const T* w;      // ttr_mode_reduce: [I] or null
  T* Y;
  int64_t sr, si;  // element strides of Y (its last axis has stride 1); ttr_mode_reduce: si unused
  double scale;    // ttr_mode_reduce
  int64_t CP, tiles, chunk;  // packs per row, tiles per row, rows per wave (split kernels; else I)
  int tw, g;                 // packs per tile, rows per step: g tw <= 64
};

template <typename T, int P, bool AL>
__device__ __forceinline__ void load_pack(const T* __restrict__ src, double (&x)[P]) {
  if (AL) {
    const Pack<T, P> v = *reinterpret_cast<const Pack<T, P>*>(src);
#pragma unroll
    for (int e = 0; e < P; ++e) x[e] = (double)v.v[e];
  } else {
#pragma unroll
    for (int e = 0; e < P; ++e) x[e] = (double)src[e];
  }
}

template <typename T, int P, bool AL>
__device__ __forceinline__ void store_pack(T* __restrict__ dst, const double (&x)[P]) {
  if (AL) {
    Pack<T, P> o;
#pragma unroll
    for (int e = 0; e < P; ++e) o.v[e] = (T)x[e];
    *reinterpret_cast<Pack<T, P>*>(dst) = o;
  } else {
#pragma unroll
    for (int e = 0; e < P; ++e) dst[e] = (T)x[e];
  }
}

// acc <- its sum over the g rows of a step, valid in the lanes of row 0 (lanes past g tw hold zeros)
template <int P>
__device__ __forceinline__ void rows_sum(double (&acc)[P], int lane, int tw, int g) {
  int s = 1;
  while (s < g) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
    const int d = s * tw;
#pragma unroll
    for (int e = 0; e < P; ++e) {
      const double y = __shfl_down(acc[e], d, kWave);
      if (lane + d < kWave) acc[e] += y;
    }
  }
}

// The sum of the rows [i_lo, i_hi) of one tile, times w: every lane its own rows i_sub, i_sub + g, ... in increasing order.
template <typename T, int P, bool AL, bool WEIGHTED>
__device__ __forceinline__ void chunk_sum(const ArrArgs<T>& p, const T* __restrict__ Xc, bool active, int isub, int64_t i_lo, int64_t i_hi,
                                          double (&acc)[P]) {
#pragma unroll
  for (int e = 0; e < P; ++e) acc[e] = 0.0;
  for (int64_t i0 = i_lo; i0 < i_hi; i0 += (int64_t)kUnroll * p.g) {
    double x[kUnroll][P], wi[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = i0 + (int64_t)u * p.g + isub;
      const bool ok = active && i < i_hi;
      wi[u] = 1.0;
      if (ok) {
        load_pack<T, P, AL>(Xc + i * p.C, x[u]);
        if (WEIGHTED) wi[u] = (double)p.w[i];
      } else {
#pragma unroll
        for (int e = 0; e < P; ++e) x[u][e] = 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
#pragma unroll
      for (int e = 0; e < P; ++e) acc[e] = WEIGHTED ? fma(wi[u], x[u][e], acc[e]) : acc[e] + x[u][e];
  }
}

template <typename T, int P, bool AL, int NW>
__global__ __launch_bounds__(NW == 1 ? kThreads : NW * kWave) void mode_scan_kernel(ArrArgs<T> p) {
  __shared__ double tot[NW][NW == 1 ? 1 : kWave][P];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int isub = lane / p.tw, cl = lane - isub * p.tw;
  const int64_t items = p.R * p.tiles;
  const int64_t first = NW == 1 ? (int64_t)blockIdx.x * (kThreads / kWave) + wave : (int64_t)blockIdx.x;
  const int64_t stride = NW == 1 ? (int64_t)gridDim.x * (kThreads / kWave) : (int64_t)gridDim.x;
  for (int64_t item = first; item < items; item += stride) {
    const int64_t r = item / p.tiles, col = (item - r * p.tiles) * p.tw + cl;
    const bool active = isub < p.g && col < p.CP;
    const int64_t lo = NW == 1 ? 0 : (int64_t)wave * p.chunk;
    const int64_t i_lo = lo < p.I ? lo : p.I, i_hi = i_lo + p.chunk < p.I ? i_lo + p.chunk : p.I;
    const T* Xc = p.X + r * p.I * p.C + col * P;
    T* Yc = p.Y + r * p.sr + col * P;
    double carry[P];
#pragma unroll
    for (int e = 0; e < P; ++e) carry[e] = 0.0;
    if constexpr (NW > 1) {   // the exclusive prefix of the earlier chunks, in chunk order
      double acc[P];
      chunk_sum<T, P, AL, false>(p, Xc, active, isub, i_lo, i_hi, acc);
      rows_sum<P>(acc, lane, p.tw, p.g);
      if (isub == 0) {
#pragma unroll
        for (int e = 0; e < P; ++e) tot[wave][cl][e] = acc[e];
      }
      __syncthreads();
      for (int k = 0; k < wave; ++k)
#pragma unroll
        for (int e = 0; e < P; ++e) carry[e] += tot[k][cl][e];
      __syncthreads();   // (the next item's totals overwrite these)
    }
    const int last = (p.g - 1) * p.tw + cl;   // the lane of this column in the last row of a step
    for (int64_t i0 = i_lo; i0 < i_hi; i0 += (int64_t)kUnroll * p.g) {
      double x[kUnroll][P];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = i0 + (int64_t)u * p.g + isub;
        if (active && i < i_hi) {
          load_pack<T, P, AL>(Xc + i * p.C, x[u]);
        } else {
#pragma unroll
          for (int e = 0; e < P; ++e) x[u][e] = 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = i0 + (int64_t)u * p.g + isub;
        for (int d = p.tw; d < p.g * p.tw; d <<= 1) {
#pragma unroll
          for (int e = 0; e < P; ++e) {
            const double y = __shfl_up(x[u][e], d, kWave);
            if (lane >= d) x[u][e] += y;
          }
        }
#pragma unroll
        for (int e = 0; e < P; ++e) x[u][e] += carry[e];
        if (active && i < i_hi) store_pack<T, P, AL>(Yc + i * p.si, x[u]);
#pragma unroll
        for (int e = 0; e < P; ++e) carry[e] = __shfl(x[u][e], last, kWave);   // (rows past i_hi added zeros: the total so far)
      }
    }
  }
}

template <typename T, int P, bool AL, int NW, bool WEIGHTED>
__global__ __launch_bounds__(NW == 1 ? kThreads : NW * kWave) void mode_reduce_kernel(ArrArgs<T> p) {
  __shared__ double tot[NW][NW == 1 ? 1 : kWave][P];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int isub = lane / p.tw, cl = lane - isub * p.tw;
  const int64_t items = p.R * p.tiles;
  const int64_t first = NW == 1 ? (int64_t)blockIdx.x * (kThreads / kWave) + wave : (int64_t)blockIdx.x;
  const int64_t stride = NW == 1 ? (int64_t)gridDim.x * (kThreads / kWave) : (int64_t)gridDim.x;
  for (int64_t item = first; item < items; item += stride) {
    const int64_t r = item / p.tiles, col = (item - r * p.tiles) * p.tw + cl;
    const bool active = isub < p.g && col < p.CP;
    const int64_t lo = NW == 1 ? 0 : (int64_t)wave * p.chunk;
    const int64_t i_lo = lo < p.I ? lo : p.I, i_hi = i_lo + p.chunk < p.I ? i_lo + p.chunk : p.I;
    double acc[P];
    chunk_sum<T, P, AL, WEIGHTED>(p, p.X + r * p.I * p.C + col * P, active, isub, i_lo, i_hi, acc);
    rows_sum<P>(acc, lane, p.tw, p.g);
    if constexpr (NW > 1) {   // the chunk totals, added in chunk order by wave 0
      if (isub == 0) {
#pragma unroll
        for (int e = 0; e < P; ++e) tot[wave][cl][e] = acc[e];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int e = 0; e < P; ++e) acc[e] = 0.0;
        for (int k = 0; k < NW; ++k)
#pragma unroll
          for (int e = 0; e < P; ++e) acc[e] += tot[k][cl][e];
      }
      __syncthreads();
    }
    if (wave == 0 || NW == 1) {
      if (active && isub == 0) {
#pragma unroll
        for (int e = 0; e < P; ++e) acc[e] *= p.scale;
        store_pack<T, P, AL>(p.Y + r * p.sr + col * P, acc);
      }
    }
  }
}

// tiling and chunks of a core for packs of P elements; true: the waves of a workgroup split I
template <typename T>
bool plan(ArrArgs<T>& p, int P) {
  p.CP = p.C / P;
  p.tiles = ceil_div(p.CP, kWave);
  p.tw = (int)ceil_div(p.CP, p.tiles);
  p.g = kWave / p.tw;
  const bool split = p.R * p.tiles < kEnoughItems && p.I >= (int64_t)kSplitWaves * p.g;
  if (split) {   // narrower tiles, more rows per step: more workgroups, as long as every wave still has a step of its own
    while (p.R * p.tiles < kSplitItems && p.tw > 1) {
      const int tw = (p.tw + 1) / 2;
      if (p.I < (int64_t)kSplitWaves * (kWave / tw)) break;
      p.tw = tw;
      p.tiles = ceil_div(p.CP, tw);
    }
    p.g = kWave / p.tw;
  }
  p.chunk = split ? align_up(ceil_div(p.I, kSplitWaves), p.g) : p.I;
  return split;
}

template <typename T>
dim3 grid_for(const ArrArgs<T>& p, bool split) {
  const int64_t blocks = split ? p.R * p.tiles : ceil_div(p.R * p.tiles, kThreads / kWave);
  return dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks));
}

template <typename T, int P, bool AL>
void scan_launch(const ArrArgs<T>& p, bool split, hipStream_t stream) {
  if (split) hipLaunchKernelGGL((mode_scan_kernel<T, P, AL, kSplitWaves>), grid_for(p, true), dim3(kSplitWaves * kWave), 0, stream, p);
  else hipLaunchKernelGGL((mode_scan_kernel<T, P, AL, 1>), grid_for(p, false), dim3(kThreads), 0, stream, p);
}

template <typename T, int P, bool AL>
void reduce_launch(const ArrArgs<T>& p, bool split, hipStream_t stream) {
  if (split) {
    if (p.w) hipLaunchKernelGGL((mode_reduce_kernel<T, P, AL, kSplitWaves, true>), grid_for(p, true), dim3(kSplitWaves * kWave), 0, stream, p);
    else hipLaunchKernelGGL((mode_reduce_kernel<T, P, AL, kSplitWaves, false>), grid_for(p, true), dim3(kSplitWaves * kWave), 0, stream, p);
  } else {
    if (p.w) hipLaunchKernelGGL((mode_reduce_kernel<T, P, AL, 1, true>), grid_for(p, false), dim3(kThreads), 0, stream, p);
    else hipLaunchKernelGGL((mode_reduce_kernel<T, P, AL, 1, false>), grid_for(p, false), dim3(kThreads), 0, stream, p);
  }
}

template <typename T>
int scan_impl(ArrArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool packed = p.C % VW == 0;
  const bool al = packed && p.sr % VW == 0 && p.si % VW == 0 && aligned16(p.X) && aligned16(p.Y);
  const bool split = plan(p, packed ? VW : 1);
  ProfScope prof(TTR_PROF_MISC, stream);
  if (al) scan_launch<T, VW, true>(p, split, stream);
  else if (packed) scan_launch<T, VW, false>(p, split, stream);
  else scan_launch<T, 1, false>(p, split, stream);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

template <typename T>
int reduce_impl(ArrArgs<T> p, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool packed = p.C % VW == 0;
  const bool al = packed && p.sr % VW == 0 && aligned16(p.X) && aligned16(p.Y);
  const bool split = plan(p, packed ? VW : 1);
  ProfScope prof(TTR_PROF_MISC, stream);
  if (al) reduce_launch<T, VW, true>(p, split, stream);
  else if (packed) reduce_launch<T, VW, false>(p, split, stream);
  else reduce_launch<T, 1, false>(p, split, stream);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_mode_scan(int dtype, int64_t R, int64_t I, int64_t C, const void* X, const int64_t* x_strides, void* Y,
                             const int64_t* y_strides, void* stream) {
  int rc = core_check("ttr_mode_scan", dtype, R, I, C, X, x_strides, Y, "Y", y_strides != nullptr);
  if (rc != TTR_OK) return rc;
  int64_t sr, si;
  rc = strided_y_check("ttr_mode_scan", R, I, C, y_strides, &sr, &si);
  if (rc != TTR_OK) return rc;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return scan_impl<T>({R, I, C, (const T*)X, nullptr, (T*)Y, sr, si, 1.0}, (hipStream_t)stream);
  });
}

extern "C" int ttr_mode_reduce(int dtype, int64_t R, int64_t I, int64_t C, const void* X, const int64_t* x_strides, const void* w,
                               double scale, void* Y, const int64_t* y_strides, void* stream) {
  const int rc = core_check("ttr_mode_reduce", dtype, R, I, C, X, x_strides, Y, "Y", y_strides != nullptr);
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(w != Y, TTR_E_INVALID, "ttr_mode_reduce: w and Y must be different buffers");
  // Y [R, C] with element strides (sr, 1) and rows that do not overlap; the stride of an extent-1 axis is free
  const int64_t sr = R > 1 ? y_strides[0] : C;
  TTR_REQUIRE((C == 1 || y_strides[1] == 1) && sr >= C, TTR_E_UNSUPPORTED,
              "ttr_mode_reduce: Y needs element strides (sr, 1) with sr >= C");
  TTR_REQUIRE((double)R * (double)sr < 9.0e18 / 64.0, TTR_E_UNSUPPORTED, "ttr_mode_reduce: Y too large");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return reduce_impl<T>({R, I, C, (const T*)X, (const T*)w, (T*)Y, sr, 0, scale}, (hipStream_t)stream);
  });
}
