// kernels_qn.inc - the kernels of hipfact_qn_ring_build (runtime_qn_ring.inc; the rule is qn_gram_rule.h): the Gram
// matrix G = X^T X of the used pairs X = [S Y] read from the ring in place, and the combination V = X C.
// (the translation unit kernels_qn.hip: a code object of its own, the others compile to the bytes they had)
// S and Y are n x memory column-major with an EVEN leading dimension ld on a 16-byte aligned base; used pair j (0 =
// oldest) lives in column slots.s[j] of both.  No atomics, no waits between workgroups: a launch boundary is the only
// ordering.  Every sum has a fixed order and the grid of every kernel follows from n alone (hipfact_qn_gram_shape): the
// same pushes give the same bits.

// ---- G = X^T X, per-workgroup partials -------------------------------------------------------------------------------
// Three 16 x 16 blocks S^T S, S^T Y, Y^T Y on the f64 matrix cores, 4 rows per instruction.  A workgroup owns the rows
// [blockIdx.x rows_per_wg, ... + rows_per_wg) in tiles of QN_TILE rows.  A tile is staged in LDS as 32 columns (S: 0 ..
// 15, Y: 16 .. 31) of QN_TILE rows by coalesced column loads - a wave reads 64 consecutive rows of one column, 512 B; a
// direct operand load from the column-major X would touch 16 columns x 32 B per wave.  Columns >= L and rows >= n enter
// as 0.0 through the guard and are never read (unused slots and the padding row may hold anything).
// The operand of k-step k0 is tile[column li][row k0 + lk] (li = lane & 15, lk = lane >> 4): both the A operand
// A[i = li][k = lk] = X[k, i] and the B operand B[k = lk][j = li] = X[k, j].  ds_read_b64 serves the lanes 0 .. 31 and
// 32 .. 63 in one LDS cycle each when the 32 double indices differ mod 32: li QN_LD + lk with lk in {0, 1} (or {2, 3})
// does for QN_LD = 2 mod 32 (2 li + lk covers 0 .. 31).
// Wave w takes the k-steps 4 w .. 4 w + 3 of every tile, in that order, into its own accumulators; at the end the four
// waves' accumulators are added in wave order.  part[768 b + 256 blk + 16 j + i]: entry (i, j) of block blk of workgroup b.
constexpr int QN_TILE = HIPFACT_QN_TILE;
constexpr int QN_LD = QN_TILE + 2;
static_assert(QN_LD % 32 == 2, "conflict-free operand reads");
static_assert(QN_TILE == 64 && FB == 256, "the staging and the deal of the k-steps are written for 4 waves x 4 k-steps");

__global__ __launch_bounds__(FB) void k_qn_gram(int n, int L, const double* __restrict__ S, const double* __restrict__ Y,
                                                long long ld, QnSlots slots, int rows_per_wg, double* __restrict__ part) {
  __shared__ double sh[3 * 4 * FB];  // the tile (32 QN_LD doubles), then the waves' accumulators
  static_assert(32 * QN_LD <= 3 * 4 * FB, "the tile fits");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  d4_t ss = {0.0, 0.0, 0.0, 0.0}, sy = {0.0, 0.0, 0.0, 0.0}, yy = {0.0, 0.0, 0.0, 0.0};
  const long long begin = (long long)blockIdx.x * rows_per_wg;
  const long long end = begin + rows_per_wg < n ? begin + rows_per_wg : n;
  for (long long r0 = begin; r0 < end; r0 += QN_TILE) {
    // stage: this wave's columns wave, wave + 4, ..., row r0 + lane of each
    const long long row = r0 + lane;
    double v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = wave + 4 * e, cc = c & 15;
      v[e] = 0.0;
      if (cc < L && row < n) v[e] = (c < 16 ? S : Y)[(long long)slots.s[cc] * ld + row];
    }
    __syncthreads();  // (the reads of the last tile are done)
#pragma unroll
    for (int e = 0; e < 8; ++e) sh[(wave + 4 * e) * QN_LD + lane] = v[e];
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k0 = 4 * (4 * wave + ks) + lk;
      const double as = sh[li * QN_LD + k0], ay = sh[(16 + li) * QN_LD + k0];
      ss = MFMA_F64(as, as, ss);
      sy = MFMA_F64(as, ay, sy);
      yy = MFMA_F64(ay, ay, yy);
    }
  }
  __syncthreads();
  // acc[q] of a lane is entry (i = lk + 4 q, j = li) of its block
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    sh[((wave * 3 + 0) * 4 + q) * 64 + lane] = ss[q];
    sh[((wave * 3 + 1) * 4 + q) * 64 + lane] = sy[q];
    sh[((wave * 3 + 2) * 4 + q) * 64 + lane] = yy[q];
  }
  __syncthreads();
  {
    const int q = wave, i = lk + 4 * q, j = li;  // (this thread's entry of each block)
    double* __restrict__ out = part + (size_t)blockIdx.x * 768;
#pragma unroll
    for (int blk = 0; blk < 3; ++blk) {
      double a = 0.0;
#pragma unroll
      for (int w = 0; w < FB / 64; ++w) a += sh[((w * 3 + blk) * 4 + q) * 64 + lane];
      out[256 * blk + 16 * j + i] = a;
    }
  }
}

// ... and G itself (2L x 2L, column-major, leading dimension 2L) from the nwg partials per entry, in the order of
// block_totals: 96 workgroups, eight entries each.  Only the entries i <= j of S^T S and Y^T Y are used, and every value
// is written to (i, j) and (j, i): G is symmetric bit for bit.
__global__ __launch_bounds__(FB) void k_qn_gram_totals(int L, const double* __restrict__ part, int nwg, double* __restrict__ G) {
  double tot[8];
  block_totals<8>(part + 8 * blockIdx.x, nwg, 768, tot);
  const int m = 2 * L;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if ((int)threadIdx.x != k) continue;
    const int e = 8 * blockIdx.x + k, blk = e >> 8, j = (e >> 4) & 15, i = e & 15;
    if (i >= L || j >= L) continue;
    if (blk == 1) {
      G[i + m * (L + j)] = tot[k];
      G[(L + j) + m * i] = tot[k];
    } else if (i <= j) {
      const int o = blk == 0 ? 0 : L;
      G[(o + i) + m * (o + j)] = tot[k];
      G[(o + j) + m * (o + i)] = tot[k];
    }
  }
}

// ---- V = X C ------------------------------------------------------------------------------------------------------------
// V[i, k] = sum_c X[i, c] C[c, k], k < rank <= RC, c ascending over the 2L columns of X, by fused multiply-adds from 0.
// C (2L x rank, column-major, leading dimension 2L) is staged in LDS as Cs[c RC + k], zero behind the rank; a thread owns
// the rows 2 q and 2 q + 1 (16 bytes per access, coalesced over the wave) and keeps its 2 RC sums in registers, so that X
// is read once; the last row of an odd n is thread 0's of workgroup 0 (the padding row is not read).  Columns >= rank of
// V are not written.
template <int RC>
__global__ __launch_bounds__(FB) void k_qn_combine(int n, int L, int rank, const double* __restrict__ S,
                                                   const double* __restrict__ Y, long long ld, QnSlots slots,
                                                   const double* __restrict__ C, double* __restrict__ V) {
  __shared__ double Cs[32 * RC];
  const int m = 2 * L;
  for (int e = threadIdx.x; e < 32 * RC; e += FB) {
    const int c = e / RC, k = e % RC;
    Cs[e] = (c < m && k < rank) ? C[c + m * k] : 0.0;
  }
  __syncthreads();
  const int npair = n >> 1;
  const long long ldh = ld >> 1;
  for (int q = blockIdx.x * FB + threadIdx.x; q < npair; q += gridDim.x * FB) {
    double2 acc[RC];
#pragma unroll
    for (int k = 0; k < RC; ++k) acc[k] = make_double2(0.0, 0.0);
#pragma unroll 4
    for (int c = 0; c < m; ++c) {
      const double* __restrict__ col = (c < L ? S : Y) + (long long)slots.s[c < L ? c : c - L] * ld;
      const double2 x = reinterpret_cast<const double2*>(col)[q];
#pragma unroll
      for (int k = 0; k < RC; ++k) {
        const double ck = Cs[c * RC + k];
        acc[k].x = fma(x.x, ck, acc[k].x);
        acc[k].y = fma(x.y, ck, acc[k].y);
      }
    }
    double2* __restrict__ V2 = reinterpret_cast<double2*>(V) + q;
#pragma unroll
    for (int k = 0; k < RC; ++k)
      if (k < rank) V2[(long long)k * ldh] = acc[k];
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const long long i = n - 1;
    for (int k = 0; k < rank; ++k) {
      double a = 0.0;
      for (int c = 0; c < m; ++c)
        a = fma(((c < L ? S : Y) + (long long)slots.s[c < L ? c : c - L] * ld)[i], Cs[c * RC + k], a);
      V[i + (long long)k * ld] = a;
    }
  }
}
