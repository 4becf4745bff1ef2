// leaf_schur.h - the tiles of the Schur update of a split level whose fronts have no children (k_leaf_schur,
// kernels_front_update.inc).  Constants shared by the kernel and the plan, and the item rule as pure host functions
// (no device, no handle), like xcd_place.h and multi_slices.h.
//
// A front with u update rows has ceil(u / edge) tile rows and one item per tile (I, J), J <= I, of its lower triangle,
// part = (I << 16) | J: edge 64 for k_front_schur, LEAF_EDGE for k_leaf_schur.
#pragma once
#include <cstddef>

namespace hipfact {

constexpr int LEAF_NB = 3;                // 16 x 16 blocks per wave and direction: 2 x 2 waves, 9 accumulators each
constexpr int LEAF_EDGE = 32 * LEAF_NB;   // rows (and columns) of a tile
constexpr int LEAF_KCH = 16;              // pivots per staged chunk
// doubles between two pivots of a strip in LDS: the edge and 16 more, so that the lanes l and l + 16 of a ds_read_b64
// (pivots k and k + 1 of an MFMA operand) fall on opposite halves of the 64-bank row
constexpr int LEAF_LS = LEAF_EDGE + 16;

// A level takes the tiles of LEAF_EDGE rows only if it has at least this many of 64 rows - one per CU of an MI355X.
// Below that every 64-row tile has a CU to itself, and the level lasts as long as its longest item: a tile of
// LEAF_EDGE rows is 9 blocks per wave where the 64-row tile is 4.
constexpr int LEAF_MIN_TILES = 256;

inline int schur_tile_rows(int u, int edge) { return (u + edge - 1) / edge; }
// Schur items of a front with u >= 0 update rows at that tile edge
inline int schur_items(int u, int edge) {
  const int nt = schur_tile_rows(u, edge);
  return nt * (nt + 1) / 2;
}
// dynamic LDS of k_leaf_schur on a level whose widest front has wp (padded) pivots: the pivots, then two strips
inline size_t leaf_schur_lds(size_t wp) { return (wp + 2 * (size_t)LEAF_LS * LEAF_KCH) * sizeof(double); }

}  // namespace hipfact
