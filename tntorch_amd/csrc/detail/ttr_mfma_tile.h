// The parts of a tile kernel on v_mfma_{f32,f64}_16x16x4 that the TT-matrix step kernels share: ttm_step_kernel
// (ttr_ttmatrix.hip), ttm_grad_input_kernel and ttm_grad_core_kernel (ttr_ttmatrix_grad.hip), lookup_step_kernel
// (ttr_ttlookup.hip) and core_compose_kernel (ttr_ttcompose.hip).  In all of them a workgroup of 4 waves owns a 64 x 64 tile of
// the output, walks K through LDS in chunks, and wave w multiplies rows 16 w .. 16 w + 15 of the tile with the <= 4 live column
// tiles of 16, one quad of k per MFMA.  One copy of every part, compiled into each unit that includes this file (unnamed
// namespace: every unit owns its instances and nothing is exported).
//
// DEVICE code, like ttr_group.h next to it and unlike ttr_internal.h: include it only from a unit whose kernels use it.
//
// What is here is what could be lifted out of those kernels WITHOUT moving one instruction of any of their instances (DESIGN
// section 3 lists what could not, and so stays written out in the kernels).  Every helper wraps straight-line code, or a loop
// the compiler unrolls in full, and is __forceinline__; none owns a loop with a run-time trip count: the loop over the quads of
// a K tile stays in the kernel.
#pragma once
#include "../ttr_common.h"

namespace ttr {
namespace {

// ------------------------------------------------------------------ LDS row strides, in elements, of the tiles
// a tile stored k-major, [k][m or n], `width` columns: the 4 (fp64: 2) k of an operand read fall into disjoint banks
constexpr int ld_kmajor(int width) { return width + 16; }
// a tile stored row-major, [m or n][k], `depth` k per row (36 fp32 / 34 fp64 for 32): conflict-free operand reads; rows stay
// 16-byte aligned
template <typename T>
constexpr int ld_rowmajor(int depth) { return depth + 16 / (int)sizeof(T); }
// the staged output tile, [m][n]: the 4 rows a lane group writes are 16 banks apart; rows stay 16-byte aligned
constexpr int ld_staged(int width) { return width + 4; }

// A pack of V consecutive elements from global memory to LDS (both aligned to the pack where V > 1), or V zeros where !live:
// `src` is not read then
template <typename T, int V>
__device__ __forceinline__ void stage_pack(T* __restrict__ dst, const T* __restrict__ src, bool live) {
  Pack<T, V> v;
#pragma unroll
  for (int j = 0; j < V; ++j) v.v[j] = T(0);
  if (live) v = *reinterpret_cast<const Pack<T, V>*>(src);
  *reinterpret_cast<Pack<T, V>*>(dst) = v;
}

// the part of [start, start + tile) below `total` (> start): the live rows or columns of an edge tile, the live k of the last
// K tile
template <typename I>
__device__ __forceinline__ int live_extent(I total, I start, int tile) {
  return total - start < (I)tile ? (int)(total - start) : tile;
}

// Tile `tile` of a grid with ntiles column tiles (BN columns each) per row tile, the column tiles fastest -- neighbours share
// the rows of the left operand -- of an output with N < 2^31 columns
template <int BN>
struct TilePos {
  int64_t mt;     // row tile
  uint32_t n0;    // first column
  int ncols;      // live columns, >= 1
  int ntl;        // live column tiles of 16
  __device__ __forceinline__ TilePos(int64_t tile, int64_t ntiles, uint32_t N) {
    mt = tile / ntiles;
    n0 = (uint32_t)(tile - mt * ntiles) * BN;
    ncols = live_extent(N, n0, BN);
    ntl = (ncols + 15) / 16;
  }
};

// One quad of k against the live column tiles: acc[t] += a x b[t BT], BT the distance of two column tiles in the B tile (16
// where it is stored k-major).  A column tile that starts at or past N is skipped.
template <typename T, int NT, int BT>
__device__ __forceinline__ void mma_quad(typename Mfma<T>::Acc (&acc)[NT], T a, const T* b, int ntl) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < ntl) acc[t] = Mfma<T>::mma(a, b[t * BT], acc[t]);
}

}  // namespace
}  // namespace ttr
