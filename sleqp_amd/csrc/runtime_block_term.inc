// runtime_block_term.inc - the block-diagonal quasi-Newton term of the Hessian operator as an object of the handle
// (hipfact_block_term, include/hipfact.h; abi_block_term.inc holds its entry points, krylov_hess_op.inc the operator it
// is a part of, block_term_items.h the work list of its dot kernel, kernels_block_term.inc the kernels)
// (part of the single translation unit hipfact.hip; included from there, in this order)

// The structure (fixed): the items and the row map on the device.  The values (one _set per SQP iteration): block_rank,
// scale and coef - coef with the stride RC of the rank ceiling, as u has it - on the device, V with the caller.  u and
// the segment partials of the long blocks are buffers of the TERM, not of the handle: a product writes nothing else.
struct hipfact_block_term {
  hipfact_handle* h = nullptr;
  int n = 0, nblocks = 0;
  int nlong = 0, nwave = 0, nshort = 0, nlong_blocks = 0;
  DevBuf d_items, d_long, d_row_blk;   // int4 per item | (block, first segment, segments) per long block | n ints
  DevBuf d_brank, d_scale, d_coef;     // nblocks ints | nblocks doubles | nblocks x RC doubles
  DevBuf d_u, d_part;                  // nblocks x RC doubles | nlong x RC doubles
  int rank = 0;                        // columns of V (0: every block is scale_b I)
  int rc = 8;                          // the rank ceiling the buffers are laid out for
  const double* V = nullptr;
  long long ld = 0;
};

// stage 1b' of a product with x (hess_op_stage1), queued on the handle's stream, and the term's fields of the rows
static int block_term_stage1(hipfact_handle* h, const hipfact_block_term* T, const double* x, HessRows* R) {
  if (T->rank > 0) {
    const int grid = T->nlong + (T->nwave + FB / 64 - 1) / (FB / 64) + (T->nshort + FB - 1) / FB;
    with_rank_ceiling(T->rank, [&](auto ceiling) {
      constexpr int RC = decltype(ceiling)::value;
      hipLaunchKernelGGL(k_blk_dots<RC>, dim3(grid), dim3(FB), 0, h->stream, T->nlong, T->nwave, T->nshort,
                         T->d_items.as<int4>(), T->d_brank.as<int>(), T->d_coef.as<double>(), T->V, T->ld, x,
                         T->d_part.as<double>(), T->d_u.as<double>());
      if (T->nlong_blocks > 0)
        hipLaunchKernelGGL(k_blk_totals<RC>, dim3(T->nlong_blocks), dim3(FB), 0, h->stream, T->d_long.as<int>(),
                           T->d_brank.as<int>(), T->d_coef.as<double>(), T->d_part.as<double>(), T->d_u.as<double>());
    });
    HCHECK(h, hipGetLastError());
  }
  R->bmap = T->d_row_blk.as<int>();
  R->bu = T->d_u.as<double>();
  R->brank = T->d_brank.as<int>();
  R->bscale = T->d_scale.as<double>();
  R->bv = T->V;
  R->bld = T->ld;
  R->bstride = T->rc;
  return HIPFACT_OK;
}

// a buffer of `bytes` in `fresh` when `cur` is too small for them (false: out of device memory; `cur` is untouched
// either way, so that a call that cannot have all its buffers leaves the term as it was)
static bool block_term_grow(DevBuf& fresh, const DevBuf& cur, size_t bytes) {
  if (cur.bytes >= std::max<size_t>(bytes, 16)) return true;
  if (fresh.ensure(std::max<size_t>(bytes, 16)) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}
