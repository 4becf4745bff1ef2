// kernels_solve_level.inc - level-scheduled solves (solve_fused = 0, and every solve after a dataflow timeout)
// (part of the translation unit kernels_solve.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// Level-scheduled solves.  y holds the right-hand side in pivot order on entry
// and the solution on exit.  Forward: children -> parents, the coupling to the
// ancestors travels as update vectors (deterministic, no atomics).  Backward:
// parents -> children, gathers the ancestors' solution.
// ---------------------------------------------------------------------------

// forward step of one front (all threads of the block; lds: r + 9 w + 1024 doubles)
__device__ __forceinline__ void dev_fwd_front(const SnDesc& S, const SnDesc* __restrict__ sn,
                                              const double* __restrict__ L, const int* __restrict__ rel,
                                              const int* __restrict__ child_idx, double* __restrict__ y,
                                              double* __restrict__ uvec, double* lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = S.w, r = S.r, u = r - w;
  const double* __restrict__ P = L + S.Loff;
  double* f = lds;              // r
  double* xs = f + r;           // w
  double* ps = xs + w;          // 8 x w partial sums of the triangular product
  double* part = ps + 8 * w;    // <= 1024 partial sums of the rectangular product
  for (int t = tid; t < r; t += SB) f[t] = (t < w) ? y[S.c0 + t] : 0.0;
  __syncthreads();
  for (int ci = S.child_begin; ci < S.child_end; ++ci) {
    const SnDesc Cd = sn[child_idx[ci]];
    const int uc = Cd.r - Cd.w;
    const double* __restrict__ uv = uvec + Cd.uoff;
    const int* __restrict__ rc = rel + Cd.reloff;
    for (int a = tid; a < uc; a += SB) f[rc[a]] += uv[a];
    __syncthreads();
  }
  // x = inv(L11) f_top: row k, eighth p of the column range [0, k)
  {
    const int k = tid & 127, p = tid >> 7;
    if (k < w) {
      const int lo = (int)(((long long)k * p) >> 3), hi = (int)(((long long)k * (p + 1)) >> 3);
      const double* Xk = P + k;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      int t = lo;
      for (; t + 3 < hi; t += 4) {
        s0 += Xk[(long long)t * r] * f[t];
        s1 += Xk[(long long)(t + 1) * r] * f[t + 1];
        s2 += Xk[(long long)(t + 2) * r] * f[t + 2];
        s3 += Xk[(long long)(t + 3) * r] * f[t + 3];
      }
      for (; t < hi; ++t) s0 += Xk[(long long)t * r] * f[t];
      ps[p * w + k] = (s0 + s1) + (s2 + s3);
    }
  }
  __syncthreads();
  for (int k = tid; k < w; k += SB) {
    double s = f[k];
#pragma unroll
    for (int p = 0; p < 8; ++p) s += ps[p * w + k];
    xs[k] = s;
    y[S.c0 + k] = s;
  }
  __syncthreads();
  if (u > 0) {
    // u_s = f_below - L21 x: 64-row chunks x column slices, fixed-order reduction
    const int nchunk = (u + 63) >> 6;
    const int nslice = nchunk >= 16 ? 1 : 16 / nchunk;
    if (nslice == 1) {
      double* __restrict__ us = uvec + S.uoff;
      for (int ch = wave; ch < nchunk; ch += 16) {
        const int a = (ch << 6) + lane;
        if (a < u) {
          const double* Lr = P + w + a;
          double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
          int k = 0;
          for (; k + 3 < w; k += 4) {
            s0 += Lr[(long long)k * r] * xs[k];
            s1 += Lr[(long long)(k + 1) * r] * xs[k + 1];
            s2 += Lr[(long long)(k + 2) * r] * xs[k + 2];
            s3 += Lr[(long long)(k + 3) * r] * xs[k + 3];
          }
          for (; k < w; ++k) s0 += Lr[(long long)k * r] * xs[k];
          us[a] = f[w + a] - ((s0 + s1) + (s2 + s3));
        }
      }
    } else {
      const int ch = wave % nchunk, sl = wave / nchunk;
      if (sl < nslice) {
        const int a = (ch << 6) + lane;
        const int lo = (int)(((long long)w * sl) / nslice), hi = (int)(((long long)w * (sl + 1)) / nslice);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (a < u) {
          const double* Lr = P + w + a;
          int k = lo;
          for (; k + 3 < hi; k += 4) {
            s0 += Lr[(long long)k * r] * xs[k];
            s1 += Lr[(long long)(k + 1) * r] * xs[k + 1];
            s2 += Lr[(long long)(k + 2) * r] * xs[k + 2];
            s3 += Lr[(long long)(k + 3) * r] * xs[k + 3];
          }
          for (; k < hi; ++k) s0 += Lr[(long long)k * r] * xs[k];
        }
        part[sl * (nchunk << 6) + (ch << 6) + lane] = (s0 + s1) + (s2 + s3);
      }
      __syncthreads();
      double* __restrict__ us = uvec + S.uoff;
      for (int a = tid; a < u; a += SB) {
        double s = 0.0;
        for (int sl2 = 0; sl2 < nslice; ++sl2) s += part[sl2 * (nchunk << 6) + a];
        us[a] = f[w + a] - s;
      }
    }
  }
}

__global__ __launch_bounds__(SB) void k_fwd_level(const SnDesc* __restrict__ sn, const int* __restrict__ level_sn,
                                                  const double* __restrict__ L, const int* __restrict__ rel,
                                                  const int* __restrict__ child_idx, double* __restrict__ y,
                                                  double* __restrict__ uvec, const int* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  if (skip && *skip) return;
  const SnDesc S = sn[level_sn[blockIdx.x]];
  dev_fwd_front(S, sn, L, rel, child_idx, y, uvec, lds);
}


// backward step of one front (lds: u + w doubles)
__device__ __forceinline__ void dev_bwd_front(const SnDesc& S, const double* __restrict__ L,
                                              const int* __restrict__ rows, double* __restrict__ y, double* lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = S.w, r = S.r, u = r - w;
  const double* __restrict__ P = L + S.Loff;
  const int* __restrict__ rw = rows + S.rowoff + w;
  double* g = lds;      // u
  double* v = lds + u;  // w
  // columns of this wave: k = 4 (wave + 16 p) + c, p = 0, 1 (w <= 128)
  const bool pre = (u <= 256);
  double lv[2][4][4];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = 4 * (wave + 16 * p) + c;
      const double* col = P + (long long)k * r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int a = lane + 64 * q;
        lv[p][c][q] = (pre && k < w && a < u) ? col[w + a] : 0.0;
      }
    }
  for (int a = tid; a < u; a += SB) g[a] = y[rw[a]];
  __syncthreads();
  // v_k = z_k / d_k - L21(:,k)^T g
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (4 * (wave + 16 * p) >= w) continue;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (pre) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int a = lane + 64 * q;
          if (a < u) s[c] += lv[p][c][q] * g[a];
        }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 4 * (wave + 16 * p) + c;
        if (k < w) {
          const double* col = P + w + (long long)k * r;
          for (int a = lane; a < u; a += 64) s[c] += col[a] * g[a];
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] += __shfl_down(s[c], o, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 4 * (wave + 16 * p) + c;
        if (k < w) v[k] = y[S.c0 + k] / P[k + (long long)k * r] - s[c];
      }
    }
  }
  // fragments of inv(L11) for the second product (in flight across the barrier)
  double xv[2][4][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = 4 * (wave + 16 * p) + c;
      const double* col = P + (long long)k * r;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int t = k + 1 + lane + 64 * q;
        xv[p][c][q] = (k < w && t < w) ? col[t] : 0.0;
      }
    }
  __syncthreads();
  // x_k = v_k + inv(L11)(:,k)^T v below the diagonal
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (4 * (wave + 16 * p) >= w) continue;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = 4 * (wave + 16 * p) + c;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int t = k + 1 + lane + 64 * q;
        if (k < w && t < w) s[c] += xv[p][c][q] * v[t];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] += __shfl_down(s[c], o, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 4 * (wave + 16 * p) + c;
        if (k < w) y[S.c0 + k] = v[k] + s[c];
      }
    }
  }
}


// Backward step of a front with u <= 256 update rows, both products on the matrix cores: a GEMV
// as an MFMA whose B operand repeats the vector in all 16 columns wastes 15/16 of the flops,
// but it needs no cross-lane reduction at all (a wave-level shuffle tree costs ~500 VALU
// instructions per wave, and with 16 waves per CU that is microseconds on the critical path).
//   v = z / d - L21^T g      wave (kb, sp): 16 pivot columns x one slice of the update rows
//   x = v + strict_lower(inv(L11))^T v
// Slices are added in a fixed order through LDS.
// lds (doubles): 4 ceil(u/4) | wp + 4 | wp | 256 | ceil(u/2)
__device__ __forceinline__ void dev_bwd_small(const SnDesc& S, const double* __restrict__ L,
                                              const int* __restrict__ rows, double* __restrict__ y, double* lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int c0 = S.c0, w = S.w, r = S.r, u = r - w;
  const int nbk = (w + 15) >> 4, wp = nbk << 4;
  const int nsplit = 16 / nbk;  // >= 2
  const int kb = wave % nbk, sp = wave / nbk;
  const bool active = sp < nsplit;
  const int nac = (u + 3) >> 2;  // chunks of 4 update rows, <= 64
  const int c_lo = nac * sp / nsplit, c_hi = nac * (sp + 1) / nsplit;
  const int k = 16 * kb + li;
  const double* __restrict__ P = L + S.Loff;
  const int* __restrict__ rw = rows + S.rowoff + w;
  double* g = lds;                // 4 nac
  double* v = g + 4 * nac;        // wp + 4 (zero beyond w)
  double* ypre = v + wp + 4;      // z_k / d_k
  double* part = ypre + wp;       // nsplit x wp <= 256 partial sums
  int* rwb = reinterpret_cast<int*>(part + 256);
  for (int a = tid; a < 4 * nac; a += SB) {
    if (a < u)
      rwb[a] = rw[a];
    else
      g[a] = 0.0;
  }
  for (int t = tid; t < wp + 4; t += SB) {
    if (t < w)
      ypre[t] = y[c0 + t] / P[t + (long long)t * r];
    else
      v[t] = 0.0;
  }
  // (requested last: the staging loops above then run without these 64 registers live)
  double lv[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int a = 4 * (c_lo + j) + lk;
    lv[j] = (active && c_lo + j < c_hi && k < w && a < u) ? P[w + a + (long long)k * r] : 0.0;
  }
  __syncthreads();
  for (int a = tid; a < u; a += SB) g[a] = y[rwb[a]];
  __syncthreads();
  if (active) {
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 32; ++j)
      if (c_lo + j < c_hi) acc = MFMA_F64(lv[j], g[4 * (c_lo + j) + lk], acc);
    if (li == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) part[sp * wp + 16 * kb + lk + 4 * q] = acc[q];
    }
  }
  // strict lower part of inv(L11)^T: chunks of 4 rows t below the first column of the block
  const int ntc = (w + 3) >> 2;
  const int cnt = ntc - 4 * kb;
  const int t_lo = 4 * kb + cnt * sp / nsplit, t_hi = 4 * kb + cnt * (sp + 1) / nsplit;
  double xf[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int t = 4 * (t_lo + j) + lk;
    xf[j] = (active && t_lo + j < t_hi && k < w && t < w && t > k) ? P[t + (long long)k * r] : 0.0;
  }
  __syncthreads();
  for (int t = tid; t < w; t += SB) {
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += part[q * wp + t];
    v[t] = ypre[t] - s;
  }
  __syncthreads();
  if (active) {
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (t_lo + j < t_hi) {
        const int t = 4 * (t_lo + j) + lk;
        acc = MFMA_F64(xf[j], v[t], acc);
      }
    if (li == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) part[sp * wp + 16 * kb + lk + 4 * q] = acc[q];
    }
  }
  __syncthreads();
  for (int t = tid; t < w; t += SB) {
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += part[q * wp + t];
    y[c0 + t] = v[t] + s;
  }
}

__global__ __launch_bounds__(SB) void k_bwd_level(const SnDesc* __restrict__ sn, const int* __restrict__ level_sn,
                                                  const double* __restrict__ L, const int* __restrict__ rows,
                                                  double* __restrict__ y, const int* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  if (skip && *skip) return;
  const SnDesc S = sn[level_sn[blockIdx.x]];
  if (S.r - S.w <= 256)
    dev_bwd_small(S, L, rows, y, lds);
  else
    dev_bwd_front(S, L, rows, y, lds);
}
