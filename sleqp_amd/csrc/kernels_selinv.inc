// kernels_selinv.inc - the selected inverse Z = M^-1 on the pattern of L + L^T (Takahashi's equations), front by front
// from the roots down (part of the translation unit kernels_selinv.hip; the recurrence and the layout are described in
// selinv_host.h, the launch sequence in runtime_selinv.inc)
//
// Four kernels, all on v_mfma_f64_16x16x4_f64 but the gather.  Lane (li, lk) = (lane & 15, lane >> 4) of a wave holds
// A[i = li][k = lk] and B[k = lk][j = li] and gets D[i = lk + 4 q][j = li], q < 4 (kernels_solve_multi.inc).  A wave
// owns the entries it writes from the first to the last term of their sums and walks k upwards: every sum has a fixed
// order given by the front's shape alone.  NO workgroup waits for another one, and none hands anything to another one
// inside a launch - the level boundary is the launch boundary: a front reads its parent's Z panel and Z_UU, both
// complete since an earlier launch (a parent's level is higher than its children's).
//
// Every load is guarded by the front's own w, u: operands beyond the edge are zero, stores beyond it do not happen.

// X[k, j] of X = inv(L11): unit lower triangular, strictly lower part in the pivot block of the panel P (ld = r)
__device__ __forceinline__ double selinv_x(const double* __restrict__ P, int r, int w, int k, int j) {
  if (k >= w || j >= w || k < j) return 0.0;
  return k == j ? 1.0 : P[k + (long long)j * r];
}

// W = L21 X for the fronts of a level: item = 64 update rows, a wave per strip of 16
__global__ __launch_bounds__(SELINV_WG) void k_selinv_w(SelinvIn A) {
  const SnDesc S = A.sn[A.level_sn[A.begin + blockIdx.x]];
  const int w = S.w, r = S.r, u = r - w;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int a0 = blockIdx.y * SELINV_ROWS + wave * 16;
  if (a0 >= u) return;
  const double* __restrict__ P = A.L + S.Loff;
  double* __restrict__ Wp = A.W + S.Loff + w;
  const int nbk = (w + 15) >> 4, a = a0 + li;
  for (int jb = 0; jb < nbk; ++jb) {
    const int j = 16 * jb + li;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 16 * jb; k0 < w; k0 += 4) {  // (X[k, j] = 0 for k < j)
      const int k = k0 + lk;
      const double av = (a < u && k < w) ? P[w + a + (long long)k * r] : 0.0;
      acc = MFMA_F64(av, selinv_x(P, r, w, k, j), acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = a0 + lk + 4 * q;
      if (row < u && j < w) Wp[row + (long long)j * r] = acc[q];
    }
  }
}

// Z_UU of the fronts of a level from their parents: item = 16 columns of the u x u block
__global__ __launch_bounds__(SELINV_WG) void k_selinv_gather(SelinvIn A) {
  const int s = A.level_sn[A.begin + blockIdx.x];
  const SnDesc S = A.sn[s];
  const int u = S.r - S.w, b0 = blockIdx.y * SELINV_COLS;
  if (b0 >= u || S.parent < 0) return;
  const SnDesc Sp = A.sn[S.parent];
  const int wp = Sp.w, rp = Sp.r, up = rp - wp;
  const double* __restrict__ Zpar = A.Z + Sp.Loff;
  const double* __restrict__ Gp = A.G + A.guoff[S.parent];
  const int* __restrict__ rel = A.rel + S.reloff;
  double* __restrict__ G = A.G + A.guoff[s];
  const int nb = u - b0 < SELINV_COLS ? u - b0 : SELINV_COLS;
  for (int idx = threadIdx.x; idx < u * nb; idx += SELINV_WG) {
    const int a = idx % u, b = b0 + idx / u;
    const int pa = rel[a], pb = rel[b];
    const int lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
    // a pair whose smaller position is a pivot column of the parent lies in its Z panel, the others in its Z_UU
    G[a + (long long)b * u] = lo < wp ? Zpar[hi + (long long)lo * rp] : Gp[(hi - wp) + (long long)(lo - wp) * up];
  }
}

// Z_UF = -Z_UU W: item = 64 update rows, a wave per strip of 16 rows and all the columns (eight column blocks at a time).
// W is the operand all four waves share: it goes through LDS in chunks of SELINV_KC rows, copied with k fastest (the
// direction in which the column-major panel is contiguous) into Ws[column][k] with a leading dimension of 36 doubles -
// the 64 lanes of an operand read (16 columns x 4 rows) then fall on 32 different 8-byte banks twice each, the least a
// 512-byte read can do.  Z_UU is read once, by the wave that owns the rows.  The sums run over k upwards, four terms
// per MFMA, whatever the chunking: it changes no bit.
constexpr int SELINV_KC = 32, SELINV_LDK = 36;
__global__ __launch_bounds__(SELINV_WG) void k_selinv_uf(SelinvIn A) {
  __shared__ double Ws[128 * SELINV_LDK];
  const int s = A.level_sn[A.begin + blockIdx.x];
  const SnDesc S = A.sn[s];
  const int w = S.w, r = S.r, u = r - w;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  if ((int)blockIdx.y * SELINV_ROWS >= u) return;  // (the whole workgroup: the barriers below see all of it or none)
  const int a0 = blockIdx.y * SELINV_ROWS + wave * 16;
  const bool live = a0 < u;  // (a wave past the last row still copies its share of W)
  const double* __restrict__ G = A.G + A.guoff[s];
  const double* __restrict__ Wp = A.W + S.Loff + w;
  double* __restrict__ Zp = A.Z + S.Loff + w;
  const int nbk = (w + 15) >> 4, a = a0 + li;
  for (int jg = 0; jg < nbk; jg += 8) {
    const int jw = w - 16 * jg < 128 ? w - 16 * jg : 128;  // columns of this group
    d4_t acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < u; kc += SELINV_KC) {
      __syncthreads();  // (the chunk before has been consumed)
      for (int idx = tid; idx < SELINV_KC * jw; idx += SELINV_WG) {
        const int kk = idx % SELINV_KC, jj = idx / SELINV_KC, k = kc + kk;
        Ws[jj * SELINV_LDK + kk] = k < u ? Wp[k + (long long)(16 * jg + jj) * r] : 0.0;
      }
      __syncthreads();
      if (live)
        for (int k0 = 0; k0 < SELINV_KC && kc + k0 < u; k0 += 4) {
          const int k = kc + k0 + lk;
          const double av = (a < u && k < u) ? G[a + (long long)k * u] : 0.0;  // (Z_UU is symmetric: row a, read down column k)
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const int jj = 16 * t + li;
            if (jg + t < nbk) acc[t] = MFMA_F64(av, jj < jw ? Ws[jj * SELINV_LDK + k0 + lk] : 0.0, acc[t]);
          }
        }
    }
    if (live) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int j = 16 * (jg + t) + li;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = a0 + lk + 4 * q;
          if (jg + t < nbk && row < u && j < w) Zp[row + (long long)j * r] = -acc[t][q];
        }
      }
    }
  }
}

// Z_FF = X^T diag(1 / d) X - W^T Z_UF: item = four 16 x 16 tiles (ib >= jb) of the lower triangle, a wave each; the
// entries on and below the diagonal are written and mirrored, so that the block is symmetric bit for bit
__global__ __launch_bounds__(SELINV_WG) void k_selinv_ff(SelinvIn A) {
  const SnDesc S = A.sn[A.level_sn[A.begin + blockIdx.x]];
  const int w = S.w, r = S.r, u = r - w;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int nbk = (w + 15) >> 4, t = blockIdx.y * SELINV_TILES + wave;
  if (t >= nbk * (nbk + 1) / 2) return;
  int ib = 0;
  while ((ib + 1) * (ib + 2) / 2 <= t) ++ib;
  const int jb = t - ib * (ib + 1) / 2;
  const double* __restrict__ P = A.L + S.Loff;
  const double* __restrict__ Wp = A.W + S.Loff + w;
  double* __restrict__ Zp = A.Z + S.Loff;
  const int i = 16 * ib + li, j = 16 * jb + li;
  d4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 16 * ib; k0 < w; k0 += 4) {  // (X[k, i] = 0 for k < i)
    const int k = k0 + lk;
    const double xj = selinv_x(P, r, w, k, j);
    acc = MFMA_F64(selinv_x(P, r, w, k, i), k < w ? xj / P[k + (long long)k * r] : 0.0, acc);
  }
  for (int k0 = 0; k0 < u; k0 += 4) {
    const int k = k0 + lk;
    const double av = (k < u && i < w) ? -Wp[k + (long long)i * r] : 0.0;
    const double bv = (k < u && j < w) ? Zp[w + k + (long long)j * r] : 0.0;
    acc = MFMA_F64(av, bv, acc);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = 16 * ib + lk + 4 * q;
    if (row < w && j < w && row >= j) {
      Zp[row + (long long)j * r] = acc[q];
      Zp[j + (long long)row * r] = acc[q];
    }
  }
}

// ---- extraction in generic mode (M = K in pivot order): the caller's index i is pivot position iperm[i]

// *bad |= 1 when an index of the request lies outside [0, N) (run in front of the extraction: such a call writes nothing)
__global__ __launch_bounds__(FB) void k_selinv_check_idx(int N, long long n, const int* __restrict__ idx, int* __restrict__ bad) {
  for (long long q = blockIdx.x * (long long)FB + threadIdx.x; q < n; q += (long long)gridDim.x * FB)
    if (idx[q] < 0 || idx[q] >= N) atomicOr(bad, 1);
}

// out[q] = (K^-1)_ii for i = idx[q] (idx null: i = q)
__global__ __launch_bounds__(FB) void k_selinv_diag_generic(SelinvLookup T, const int* __restrict__ iperm, int N, long long n,
                                                            const int* __restrict__ idx, const double* __restrict__ Z,
                                                            double* __restrict__ out) {
  for (long long q = blockIdx.x * (long long)FB + threadIdx.x; q < n; q += (long long)gridDim.x * FB) {
    const int i = idx ? idx[q] : (int)q;
    if (i < 0 || i >= N) continue;
    const int p = iperm[i];
    const long long off = selinv_offset(T.nsuper, T.c0, T.sn_r, T.rowptr, T.rows, T.Loff, p, p);
    out[q] = off >= 0 ? Z[off] : __builtin_nan("");
  }
}

// out[q] = (K^-1)_ij at (row[q], col[q]); a pair outside the structure gets a quiet NaN and is counted in part[block]
__global__ __launch_bounds__(FB) void k_selinv_entries_generic(SelinvLookup T, const int* __restrict__ iperm, int N, long long n,
                                                               const int* __restrict__ row, const int* __restrict__ col,
                                                               const double* __restrict__ Z, double* __restrict__ out,
                                                               unsigned long long* __restrict__ part) {
  __shared__ unsigned long long cnt[FB];
  unsigned long long mine = 0;
  for (long long q = blockIdx.x * (long long)FB + threadIdx.x; q < n; q += (long long)gridDim.x * FB) {
    const int i = row[q], j = col[q];
    long long off = -1;
    if (i >= 0 && i < N && j >= 0 && j < N) off = selinv_offset(T.nsuper, T.c0, T.sn_r, T.rowptr, T.rows, T.Loff, iperm[i], iperm[j]);
    out[q] = off >= 0 ? Z[off] : __builtin_nan("");
    mine += off < 0;
  }
  cnt[threadIdx.x] = mine;
  __syncthreads();
  for (int s = FB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) cnt[threadIdx.x] += cnt[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = cnt[0];
}

// ---- the fallback: unit-vector columns of the blocked solve

// X (N x 16, ld = N): column j < nb is e_ind[j], the others are zero
__global__ __launch_bounds__(FB) void k_selinv_units(int N, int nb, SelinvCols C, double* __restrict__ X) {
  const long long total = (long long)N * 16;
  for (long long q = blockIdx.x * (long long)FB + threadIdx.x; q < total; q += (long long)gridDim.x * FB) {
    const int j = (int)(q / N), i = (int)(q - (long long)j * N);
    X[q] = (j < nb && i == C.ind[j]) ? 1.0 : 0.0;
  }
}

// out[dst[j]] = X[ind[j], j]: component i of K^-1 e_i
__global__ __launch_bounds__(64) void k_selinv_pick(int N, int nb, SelinvCols C, const double* __restrict__ X, double* __restrict__ out) {
  const int j = threadIdx.x;
  if (j < nb && j < 16) out[C.dst[j]] = X[C.ind[j] + (long long)j * N];
}

// ---- extraction in saddle mode: K = [I A^T; A 0] in the caller's numbering, Z = M^-1 = D Z^ D with the row scales D
// (powers of two: every product with them is exact), a_j = column j of the working-set rows.  The handle's K keeps the
// column of a variable fixed by an active bound whole (vmap marks it), unless the plan itself eliminated the bounds
// (`cut`: such a column holds its diagonal only, and the unit row of its bound cannot be served).
//     free ordinary variable j            1 - a_j^T Z a_j
//     variable fixed by an active bound   0
//     working-set row                     -Z_rr
//     late variable                       -Z_ii            (K^-1 = -J M^-1 J on rows and late variables, J = diag(I, -I))
//     unit row of the bound on x_j        -1 - a_j^T Z a_j
// kind[i] for a position i >= n of the caller's vectors: s >= 0 structure row s, -2 - j the unit row of the bound on x_j,
// -1 neither (k_selinv_kinds; the array is preset to -1).
__global__ __launch_bounds__(FB) void k_selinv_kinds(int n, int my, const int* __restrict__ vmap, const int* __restrict__ cmap,
                                                     int N, int* __restrict__ kind) {
  const int total = my > n ? my : n;
  for (int t = blockIdx.x * FB + threadIdx.x; t < total; t += gridDim.x * FB) {
    if (t < my) {
      const int e = cmap ? cmap[t] : n + t;
      if (e >= n && e < N) kind[e] = t;
    }
    if (t < n && vmap) {
      const int v = vmap[t];
      if (v >= n && v < N) kind[v] = -2 - t;
    }
  }
}

// a_j^T Z a_j by the 64 lanes of a wave: pair q = (e, e') of the column's entries goes to lane q % 64; the lane sums
// run over q upwards, the shuffle tree is fixed.  ok <- false when a pair is outside the structure.  Every lane
// returns the sum.
__device__ __forceinline__ double selinv_quad(const SelinvSaddle& A, int j, int lane, bool& ok) {
  const int e0 = A.Kp[j], c = A.Kp[j + 1] - e0;
  double s = 0.0;
  int bad = 0;
  for (long long q = lane; q < (long long)c * c; q += 64) {
    const int ea = e0 + (int)(q / c), eb = e0 + (int)(q % c);
    const int ra = A.Ki[ea] - A.n, rb = A.Ki[eb] - A.n;
    if (ra < 0 || rb < 0) continue;  // (the unit diagonal)
    if (A.cmap && (A.cmap[ra] < 0 || A.cmap[rb] < 0)) continue;  // (a row outside the working set)
    const int pa = A.iperm[ra], pb = A.iperm[rb];
    const long long off = selinv_offset(A.T.nsuper, A.T.c0, A.T.sn_r, A.T.rowptr, A.T.rows, A.T.Loff, pa, pb);
    if (off < 0) {
      bad = 1;
      continue;
    }
    s += (A.Kval[ea] * A.dscale[pa]) * (A.Kval[eb] * A.dscale[pb]) * A.Z[off];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if (bad) ok = false;
  return s;
}

// out[q] = (K^-1)_ii for i = idx[q] (idx null: i = q), a wave per index; need[q] = 1 and a NaN where the selected
// inverse cannot serve the index (an entry outside the structure, the unit row of a bound on a cut column); *nneed
// counts them
__global__ __launch_bounds__(FB) void k_selinv_diag_saddle(SelinvSaddle A, long long n, const int* __restrict__ idx,
                                                           double* __restrict__ out, int* __restrict__ need,
                                                           unsigned long long* __restrict__ nneed) {
  const int lane = threadIdx.x & 63;
  for (long long q = blockIdx.x * (long long)(FB / 64) + (threadIdx.x >> 6); q < n; q += (long long)gridDim.x * (FB / 64)) {
    const int i = idx ? idx[q] : (int)q;
    if (i < 0 || i >= A.N) continue;
    bool ok = !(A.fake_absent > 0 && q % A.fake_absent == 0);
    double v = 0.0;
    int vertex = -1;  // >= 0: the value is -Z at this vertex of M
    if (i < A.n) {
      if (A.vmap && A.vmap[i] >= 0) v = 0.0;
      else if (A.latemap[i] >= 0) vertex = A.my + A.latemap[i];
      else v = 1.0 - selinv_quad(A, i, lane, ok);
    } else {
      const int k = A.kind[i];
      if (k >= 0) vertex = k;
      else if (k <= -2 && !A.cut) v = -1.0 - selinv_quad(A, -2 - k, lane, ok);
      else ok = false;
    }
    if (vertex >= 0) {
      const int p = A.iperm[vertex];
      const long long off = selinv_offset(A.T.nsuper, A.T.c0, A.T.sn_r, A.T.rowptr, A.T.rows, A.T.Loff, p, p);
      if (off < 0) ok = false;
      else v = -(A.dscale[p] * A.dscale[p] * A.Z[off]);
    }
    if (lane == 0) {
      out[q] = ok ? v : __builtin_nan("");
      need[q] = ok ? 0 : 1;
      if (!ok) atomicAdd(nneed, 1ull);
    }
  }
}

// out[q] = (K^-1)_ij for i and j both working-set rows or late variables with the pair in the structure:
// -s_i s_j d_i d_j Z^_ij, s = -1 for a late variable; a quiet NaN, counted in part[block], for every other pair
__global__ __launch_bounds__(FB) void k_selinv_entries_saddle(SelinvSaddle A, long long n, const int* __restrict__ row,
                                                              const int* __restrict__ col, double* __restrict__ out,
                                                              unsigned long long* __restrict__ part) {
  __shared__ unsigned long long cnt[FB];
  unsigned long long mine = 0;
  for (long long q = blockIdx.x * (long long)FB + threadIdx.x; q < n; q += (long long)gridDim.x * FB) {
    int vx[2];
    double sg[2];
    const int ij[2] = {row[q], col[q]};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int i = ij[t];
      vx[t] = -1;
      sg[t] = 1.0;
      if (i < 0 || i >= A.N) continue;
      if (i < A.n) {
        if (!(A.vmap && A.vmap[i] >= 0) && A.latemap[i] >= 0) {
          vx[t] = A.my + A.latemap[i];
          sg[t] = -1.0;
        }
      } else if (A.kind[i] >= 0) {
        vx[t] = A.kind[i];
      }
    }
    long long off = -1;
    int pa = 0, pb = 0;
    if (vx[0] >= 0 && vx[1] >= 0) {
      pa = A.iperm[vx[0]];
      pb = A.iperm[vx[1]];
      off = selinv_offset(A.T.nsuper, A.T.c0, A.T.sn_r, A.T.rowptr, A.T.rows, A.T.Loff, pa, pb);
    }
    out[q] = off >= 0 ? -(sg[0] * sg[1]) * (A.dscale[pa] * A.dscale[pb] * A.Z[off]) : __builtin_nan("");
    mine += off < 0;
  }
  cnt[threadIdx.x] = mine;
  __syncthreads();
  for (int s = FB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) cnt[threadIdx.x] += cnt[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = cnt[0];
}
