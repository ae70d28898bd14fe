// Differential operators on one TT core (derivatives.py:72-130 `partial`, 286-302 `laplacian`), streaming kernels for gfx950:
//   ttr_mode_diff     Y = (inv_step S)^order X along the middle axis of X [R, I, C]
//   ttr_laplace_core  the block core [[A, D], [0, A]] (first: [A D], last: [D ; A]) with D = (inv_step S)^2 A, in one launch
// S is the reference's central-difference matrix: interior rows e[i+1] - e[i-1], row 0 = 2 (e[1] - e[0]), row I-1 =
// 2 (e[I-1] - e[I-2]) (its linearly extrapolated edge), or roll(-1) - roll(+1) when periodic; I = 1 gives zeros.
//
// Both kernels walk the flattened (i, c) axis of one slab X[r] with the lanes: the neighbours of a row lie at +- C elements, so
// every load of a wave is one contiguous run for every C, C = 1 (the last core) included.  A thread owns V consecutive c of one
// row (V = 16 bytes when C, the strides and the pointers allow it, else one element), loads the 2 order + 1 rows around its own
// into registers -- the overlap between threads is served by the caches, X leaves HBM once -- and applies the `order` passes
// there: pass p is valid on the rows within order - p of the thread's own, so the centre survives all of them.  The window is
// held in fp64 for both dtypes and rounded once, at the store: the kernels are bound by memory traffic, so the wider arithmetic
// costs nothing, the passes of one launch do not round to fp32 in between, and where (inv_step S)^order annihilates the data
// exactly (S^3 = 0 for I = 3, S^2 = 0 for I = 2: the rows of the lower power coincide) fp32 input gives the exact zero that the
// fp64 pass gives instead of cancellation noise at eps times the lower power.  Rows outside [0, I) are never read (periodic:
// wrapped), and every extent and stride comes from validated host arguments.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int kDiffMaxOrder = 4;   // passes fused into one launch: 2 * 4 + 1 rows of V values in registers
constexpr int64_t kMaxBlocks = 2048;  // 256 CUs x 8 blocks; the rest of the items is walked with a grid stride

template <typename T>
struct DiffArgs {
  int64_t R, I, C;
  const T* X;
  T* Y;
  int64_t sr, si;  // element strides of Y (its last axis has stride 1); ttr_laplace_core: unused
  int pos;         // ttr_laplace_core only
  double s;
};

// rows i - O .. i + O of the slab Xr [I, C] at columns c .. c + V - 1; rows outside [0, I) are wrapped (PER) or left zero
template <typename T, int O, int V, bool PER>
__device__ __forceinline__ void load_window(const T* __restrict__ Xr, int64_t I, int64_t C, int64_t i, int64_t c, double (&w)[2 * O + 1][V]) {
#pragma unroll
  for (int k = 0; k <= 2 * O; ++k) {
    int64_t g = i - O + k;
    bool ok = true;
    if (PER) {
      g %= I;
      if (g < 0) g += I;
    } else {
      ok = g >= 0 && g < I;
    }
    if (ok) {
      const Pack<T, V> x = *reinterpret_cast<const Pack<T, V>*>(Xr + g * C + c);
#pragma unroll
      for (int e = 0; e < V; ++e) w[k][e] = (double)x.v[e];
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) w[k][e] = 0.0;
    }
  }
}

// O passes in place; afterwards w[O] is row i of (s S)^O X
template <int O, int V, bool PER>
__device__ __forceinline__ void apply_passes(int64_t I, int64_t i, double s, double (&w)[2 * O + 1][V]) {
  // one IEEE subtraction and one IEEE multiplication per pass and entry, as the host mirror performs them: a product contracted
  // into the next pass's subtraction would round differently, and the two sides would disagree in the last bit
#pragma clang fp contract(off)
  using T = double;
#pragma unroll
  for (int p = 1; p <= O; ++p) {
    T prev[V];
#pragma unroll
    for (int e = 0; e < V; ++e) prev[e] = w[p - 1][e];
#pragma unroll
    for (int k = p; k <= 2 * O - p; ++k) {
      const int64_t g = i - O + k;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const T cur = w[k][e];
        T y;
        if (PER) {
          y = (w[k + 1][e] - prev[e]) * s;
        } else if (g < 0 || g >= I || I == 1) {
          y = T(0);
        } else if (g == 0) {
          y = T(2) * (w[k + 1][e] - cur) * s;
        } else if (g == I - 1) {
          y = T(2) * (cur - prev[e]) * s;
        } else {
          y = (w[k + 1][e] - prev[e]) * s;
        }
        w[k][e] = y;
        prev[e] = cur;
      }
    }
  }
}

template <typename T, int V>
__device__ __forceinline__ void store(T* dst, const double (&x)[V]) {
  Pack<T, V> o;
#pragma unroll
  for (int e = 0; e < V; ++e) o.v[e] = (T)x[e];
  *reinterpret_cast<Pack<T, V>*>(dst) = o;
}

template <typename T, int O, int V, bool PER>
__global__ __launch_bounds__(kThreads) void mode_diff_kernel(DiffArgs<T> p) {
  const int64_t JV = p.I * p.C / V, total = p.R * JV;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t item = (int64_t)blockIdx.x * kThreads + threadIdx.x; item < total; item += stride) {
    const int64_t r = item / JV, j = (item - r * JV) * V;
    const int64_t i = j / p.C, c = j - i * p.C;
    double w[2 * O + 1][V];
    load_window<T, O, V, PER>(p.X + r * p.I * p.C, p.I, p.C, i, c, w);
    apply_passes<O, V, PER>(p.I, i, p.s, w);
    store<T, V>(p.Y + r * p.sr + i * p.si + c, w[O]);
  }
}

template <typename T, int V, bool PER>
__global__ __launch_bounds__(kThreads) void laplace_core_kernel(DiffArgs<T> p) {
  const int64_t JV = p.I * p.C / V, total = p.R * JV;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t wide = p.pos == 2 ? p.C : 2 * p.C;  // row length of `out`
  for (int64_t item = (int64_t)blockIdx.x * kThreads + threadIdx.x; item < total; item += stride) {
    const int64_t r = item / JV, j = (item - r * JV) * V;
    const int64_t i = j / p.C, c = j - i * p.C;
    double w[5][V], a[V], z[V];   // (fp32 -> fp64 -> fp32 is the identity: the copies of A stay bit-identical)
    load_window<T, 2, V, PER>(p.X + r * p.I * p.C, p.I, p.C, i, c, w);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      a[e] = w[2][e];
      z[e] = 0.0;
    }
    apply_passes<2, V, PER>(p.I, i, p.s, w);
    T* top = p.Y + (r * p.I + i) * wide + c;              // block row of A's own rank index
    T* bot = p.Y + ((p.R + r) * p.I + i) * wide + c;      // the second block row (middle and last cores)
    if (p.pos == 2) {            // [D ; A]
      store<T, V>(top, w[2]);
      store<T, V>(bot, a);
    } else {                     // [A D] and, for a middle core, [0 A] below it
      store<T, V>(top, a);
      store<T, V>(top + p.C, w[2]);
      if (p.pos == 1) {
        store<T, V>(bot, z);
        store<T, V>(bot + p.C, a);
      }
    }
  }
}

unsigned grid_for(int64_t total) {
  const int64_t blocks = ceil_div(total, kThreads);
  return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

template <typename T, int V, bool PER>
void mode_diff_launch_o(const DiffArgs<T>& p, int order, hipStream_t stream) {
  const dim3 grid(grid_for(p.R * (p.I * p.C / V))), block(kThreads);
  switch (order) {
    case 1: hipLaunchKernelGGL((mode_diff_kernel<T, 1, V, PER>), grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL((mode_diff_kernel<T, 2, V, PER>), grid, block, 0, stream, p); break;
    case 3: hipLaunchKernelGGL((mode_diff_kernel<T, 3, V, PER>), grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL((mode_diff_kernel<T, 4, V, PER>), grid, block, 0, stream, p); break;
  }
}

template <typename T>
int mode_diff_impl(DiffArgs<T> p, int order, int periodic, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool wide = p.C % VW == 0 && p.sr % VW == 0 && p.si % VW == 0 && aligned16(p.X) && aligned16(p.Y);
  ProfScope prof(TTR_PROF_MISC, stream);
  if (wide) {
    if (periodic) mode_diff_launch_o<T, VW, true>(p, order, stream);
    else mode_diff_launch_o<T, VW, false>(p, order, stream);
  } else {
    if (periodic) mode_diff_launch_o<T, 1, true>(p, order, stream);
    else mode_diff_launch_o<T, 1, false>(p, order, stream);
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

template <typename T>
int laplace_core_impl(DiffArgs<T> p, int periodic, hipStream_t stream) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool wide = p.C % VW == 0 && aligned16(p.X) && aligned16(p.Y);
  const dim3 block(kThreads);
  ProfScope prof(TTR_PROF_MISC, stream);
  if (wide) {
    const dim3 grid(grid_for(p.R * (p.I * p.C / VW)));
    if (periodic) hipLaunchKernelGGL((laplace_core_kernel<T, VW, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((laplace_core_kernel<T, VW, false>), grid, block, 0, stream, p);
  } else {
    const dim3 grid(grid_for(p.R * p.I * p.C));
    if (periodic) hipLaunchKernelGGL((laplace_core_kernel<T, 1, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((laplace_core_kernel<T, 1, false>), grid, block, 0, stream, p);
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_mode_diff_max_order(void) { return kDiffMaxOrder; }

extern "C" int ttr_mode_diff(int dtype, int64_t R, int64_t I, int64_t C, int order, int periodic, double inv_step, const void* X,
                             const int64_t* x_strides, void* Y, const int64_t* y_strides, void* stream) {
  int rc = core_check("ttr_mode_diff", dtype, R, I, C, X, x_strides, Y, "the output");
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(y_strides, TTR_E_INVALID, "ttr_mode_diff: null pointer");
  TTR_REQUIRE(order >= 1, TTR_E_INVALID, "ttr_mode_diff: order %d < 1", order);
  TTR_REQUIRE(order <= kDiffMaxOrder, TTR_E_UNSUPPORTED, "ttr_mode_diff: order %d above the fused limit %d (chain calls)", order,
              kDiffMaxOrder);
  int64_t sr, si;
  rc = strided_y_check("ttr_mode_diff", R, I, C, y_strides, &sr, &si);
  if (rc != TTR_OK) return rc;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return mode_diff_impl<T>({R, I, C, (const T*)X, (T*)Y, sr, si, 0, inv_step}, order, periodic != 0, (hipStream_t)stream);
  });
}

extern "C" int ttr_laplace_core(int dtype, int64_t R, int64_t I, int64_t C, int pos, int periodic, double inv_step, const void* X,
                                const int64_t* x_strides, void* out, void* stream) {
  const int rc = core_check("ttr_laplace_core", dtype, R, I, C, X, x_strides, out, "the output");
  if (rc != TTR_OK) return rc;
  TTR_REQUIRE(pos >= 0 && pos <= 2, TTR_E_INVALID, "ttr_laplace_core: pos %d is none of 0 (first), 1 (middle), 2 (last)", pos);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return laplace_core_impl<T>({R, I, C, (const T*)X, (T*)out, 0, 0, pos, inv_step}, periodic != 0, (hipStream_t)stream);
  });
}
