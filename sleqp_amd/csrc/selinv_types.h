// selinv_types.h - what a launch of the selected-inverse sweep needs (kernels_selinv.inc, runtime_selinv.inc)
#pragma once
#include "device_types.h"

namespace hipfact {

constexpr int SELINV_WG = 256;    // threads of a workgroup of the sweep: four waves, a 16-row MFMA strip each
constexpr int SELINV_ROWS = 64;   // update rows of a W / Z_UF item
constexpr int SELINV_COLS = 16;   // columns of a Z_UU item
constexpr int SELINV_TILES = 4;   // 16 x 16 tiles of the lower triangle of Z_FF per item

// One launch covers the fronts level_sn[begin .. begin + gridDim.x); blockIdx.y is the item of the front (a block whose
// front has fewer items returns at once).  W and Z have the layout of the factor arena L (an r x w panel per front at
// SnDesc::Loff, W in the rows below the pivot block); G holds the u x u block Z_UU of front s at guoff[s].
struct SelinvIn {
  const SnDesc* sn;
  const int* level_sn;
  const int* rel;
  const long long* guoff;
  const double* L;
  double* W;
  double* Z;
  double* G;
  int begin;
};

// the extraction kernels: the tree's arrays for selinv_offset (selinv_host.h) and the maps of the caller's numbering
struct SelinvLookup {
  int nsuper;
  const int* c0;
  const int* sn_r;
  const long long* rowptr;
  const int* rows;
  const long long* Loff;
};

// what the saddle-mode extraction kernels need (kernels_selinv.inc describes the table)
struct SelinvSaddle {
  SelinvLookup T;
  const int* iperm;    // vertex of M -> pivot position
  const int* latemap;  // variable -> its late index, -1: ordinary
  const int* kind;
  const int* Kp;
  const int* Ki;
  const double* Kval;
  const int* vmap;
  const int* cmap;
  const double* dscale;  // by pivot position
  const double* Z;
  int n, my, N, cut;
  int fake_absent;  // test hook (option selinv_fake_absent): > 0 treats every request slot q with q % fake_absent == 0 as not served
};

// a block of the fallback: column j < nb of the N x 16 block is the unit vector e_ind[j], and component ind[j] of its
// solution goes to out[dst[j]]
struct SelinvCols {
  int ind[16];
  long long dst[16];
};

}  // namespace hipfact
