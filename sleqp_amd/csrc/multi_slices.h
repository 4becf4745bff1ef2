// multi_slices.h - how the blocked solve cuts a tall front into row slices (pure host functions: no device, no handle)
//
// A front with u update rows has nt = ceil(u / 16) tiles of 16 rows: the unit of the forward sweep's MFMA tiles and of
// the backward sweep's chunks.  With a slice height of S rows (option multi_slice_rows; 0: off) the front becomes
// nslice = max(1, u / S) items, slice k owning the tiles [nt k / nslice, nt (k + 1) / nslice): the slices differ by at
// most one tile, every slice has at least S / 16 of them, and a front with u < 2 S stays ONE item, which runs the
// unsliced path of the kernels.  The item lists of the sweeps (runtime_multi.inc) and hipfact_debug_multi_slices are
// both built from multi_slices below.
#pragma once

namespace hipfact {

constexpr int MULTI_SLICE_ROWS_MAX = 4096;

// 0, or a multiple of 16 in [16, MULTI_SLICE_ROWS_MAX]
inline bool multi_slice_rows_valid(long long S) {
  return S == 0 || (S >= 16 && S <= MULTI_SLICE_ROWS_MAX && S % 16 == 0);
}

inline int multi_tiles(int u) { return (u + 15) >> 4; }

// slices of a front with u >= 0 update rows (S valid)
inline int multi_nslice(int u, int S) { return S > 0 && u / S > 1 ? u / S : 1; }

// first tile of slice k (k = nslice: one past the last tile)
inline int multi_slice_tile(int u, int nslice, int k) { return (int)((long long)multi_tiles(u) * k / nslice); }

}  // namespace hipfact
