// block_term_items.h - the work list of the dot kernel of a block-diagonal quasi-Newton term (hipfact_block_term,
// krylov_hess_op.inc stage 1b'), as a pure host rule: no device, no handle (the idiom of condest_rule.h / ritz_rule.h;
// hipfact_debug_block_items hands it to the tests).
//
// From block_end alone: block b covers the rows [block_end[b-1], block_end[b]) and is cut into ITEMS by its length,
//   short  len <= BT_SHORT            one item, ONE THREAD: rows ascending, one running sum per column, no tree.
//                                     Consecutive short blocks sit on consecutive threads, so a wave's loads of a column
//                                     cover one contiguous row range.
//   wave   BT_SHORT < len <= BT_WAVE  one item, ONE WAVE: lane l takes the rows begin + l, + 64, ... ascending, then the
//                                     shuffle tree of wave_sum per column.
//   long   len > BT_WAVE              ceil(len / BT_SEG) items of BT_SEG rows (the last one shorter), one workgroup of FB
//                                     threads each: thread t takes the rows first + t, + FB, ... ascending, block_partials;
//                                     a second launch adds a block's segments in segment order (block_totals).
// The summation order of every w_bk = sum_{i in b} V_ik x_i is therefore a function of block_end and of the rank ceiling
// (which only selects the template instance), and of nothing else: not of the device, the grid, the other blocks'
// values or the entry point.
// The list is ordered long, wave, short (ascending by block, a long block's segments ascending by row): the workgroups
// [0, nlong) of the dot launch are the segments, so a segment's partial sits at its blockIdx; then ceil(nwave / (FB/64))
// workgroups of waves, then ceil(nshort / FB) workgroups of threads.
//
// BT_SHORT, BT_WAVE and BT_SEG: the start values 32 / 1024 / 4096 lost a sweep over block lengths on both edges (a thread
// on 32 rows and a wave on 1024 were slower than the next class on one row more) and left a long block with too few
// workgroups; 8 / 256 / 512 are what was run after them, two processes per figure, and no finer search was made
// (EXPERIMENTS.md, "Block term").  They are part of the summation order: changing one changes bits.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace hipfact {

constexpr int BT_SHORT = 8;
constexpr int BT_WAVE = 256;
constexpr int BT_SEG = 512;

enum BlockItemClass { BT_CLASS_SHORT = 0, BT_CLASS_WAVE = 1, BT_CLASS_LONG = 2 };

struct BlockItem {
  int cls;    // BlockItemClass
  int block;  // the block it belongs to
  int row0;   // its first row
  int rows;   // its row count (>= 1)
};

struct BlockItems {
  std::vector<BlockItem> items;  // long | wave | short
  int nlong = 0, nwave = 0, nshort = 0;  // items per class (nlong: segments)
  // the long blocks, ascending: block, first segment (= index into `items`), segments
  std::vector<int> long_block, long_seg0, long_nseg;
  std::vector<int> row_blk;  // per row: its block, -1 in the linear range
};

static inline int block_item_class(int len) { return len <= BT_SHORT ? BT_CLASS_SHORT : len <= BT_WAVE ? BT_CLASS_WAVE : BT_CLASS_LONG; }

// block_end: strictly ascending, first > 0, last <= n (false otherwise; 1 <= nblocks <= n)
static inline bool block_ends_ok(int n, int nblocks, const int* block_end) {
  if (n < 1 || nblocks < 1 || nblocks > n || !block_end) return false;
  int prev = 0;
  for (int b = 0; b < nblocks; ++b) {
    if (block_end[b] <= prev || block_end[b] > n) return false;
    prev = block_end[b];
  }
  return true;
}

// what hipfact_block_term_set refuses in its values, or null (have_V: a V was given; coef[b * rank + k] is read for
// k < block_rank[b] only)
static inline const char* block_values_bad(int n, int nblocks, int rank, const int* block_rank, const double* scale,
                                           const double* coef, bool have_V, long long ld) {
  if (rank < 0 || rank > 32) return "rank outside 0 .. 32";
  if (!block_rank || !scale) return "no block_rank or scale";
  if (rank > 0 && (!have_V || !coef)) return "rank > 0 without V or coef";
  if (rank > 0 && ld < n) return "leading dimension below n";
  for (int b = 0; b < nblocks; ++b) {
    if (block_rank[b] < 0 || block_rank[b] > rank) return "block_rank outside 0 .. rank";
    if (!std::isfinite(scale[b])) return "non-finite scale";
    for (int k = 0; k < block_rank[b]; ++k)
      if (!std::isfinite(coef[(size_t)b * rank + k])) return "non-finite coefficient";
  }
  return nullptr;
}

static inline bool block_items_build(int n, int nblocks, const int* block_end, BlockItems* out) {
  if (!block_ends_ok(n, nblocks, block_end)) return false;
  BlockItems& B = *out;
  B = BlockItems();
  B.row_blk.assign((size_t)n, -1);
  std::vector<BlockItem> wave, shrt;
  int begin = 0;
  for (int b = 0; b < nblocks; ++b) {
    const int end = block_end[b], len = end - begin;
    for (int i = begin; i < end; ++i) B.row_blk[(size_t)i] = b;
    const int cls = block_item_class(len);
    if (cls == BT_CLASS_SHORT)
      shrt.push_back({cls, b, begin, len});
    else if (cls == BT_CLASS_WAVE)
      wave.push_back({cls, b, begin, len});
    else {
      B.long_block.push_back(b);
      B.long_seg0.push_back((int)B.items.size());
      int nseg = 0;
      for (int r = begin; r < end; r += BT_SEG, ++nseg) B.items.push_back({cls, b, r, end - r < BT_SEG ? end - r : BT_SEG});
      B.long_nseg.push_back(nseg);
    }
    begin = end;
  }
  B.nlong = (int)B.items.size();
  B.nwave = (int)wave.size();
  B.nshort = (int)shrt.size();
  B.items.insert(B.items.end(), wave.begin(), wave.end());
  B.items.insert(B.items.end(), shrt.begin(), shrt.end());
  return true;
}

}  // namespace hipfact
