"""References for the block-diagonal quasi-Newton term of the Hessian operator (hipfact_block_term), shared by
test_block_term_host.py, test_block_term.py and test_block_term_shim.py: the structures at the edges of the dot
kernel's classes, random terms with NaN in every cell that must not be read, the assembled matrix, and
`reference_product` of low_rank_ref.py extended to the block term in numpy.longdouble with the bound of every entry."""
import numpy as np

from low_rank_ref import LD, U, dense_recursion


def structures(consts):
    """name -> (n, block_end): every block length at which the dot kernel changes its class or its segment count, the
    constants as the library reports them (block_items(...)[2]); a last end at n and one below n"""
    S, W, G = consts["short"], consts["wave"], consts["seg"]

    def ends(lengths, lin):
        e = np.cumsum(lengths)
        return int(e[-1] + lin), e.astype(np.int32)

    return {
        "short_wave_edges": ends([1, 2, S - 1, S, S + 1, W - 1, W, W + 1, 3, 1], 5),  # a linear range of 5 rows
        "segment_edges": ends([G - 1, 2, G, G + 1], 0),  # the last end at n
        "three_segments": ends([1, 2 * G + 1, W + 1, 2], 7),
        "all_ones": ends([1] * 300, 0),  # nblocks = n
        "one_block": ends([300], 0),  # nblocks = 1
        "one_block_lin": ends([257], 43),
    }


def row_blocks(n, block_end):
    rb = np.full(n, -1, dtype=np.int64)
    begin = 0
    for b, end in enumerate(block_end):
        rb[begin:end] = b
        begin = end
    return rb


def random_term(n, block_end, rank, seed, poison=np.nan, ranks=None):
    """(block_rank, scale, coef (nblocks x rank), V (n x rank)): block ranks mixed over 0, 1, rank and values between,
    `poison` in every cell of V that must not be read - the linear range and the rows of column k in a block with
    block_rank <= k - and in the unread cells of coef"""
    rng = np.random.default_rng(seed)
    nb = len(block_end)
    if ranks is None:
        ranks = rng.integers(0, rank + 1, nb)
        first = [rank, 0, 1, max(rank - 1, 0), rank // 2]  # (the first blocks: the full rank, none, one, ...)
        ranks[:len(first)] = first[:nb]
    ranks = np.minimum(np.asarray(ranks, dtype=np.int32), rank)
    scale = rng.standard_normal(nb)
    coef = rng.standard_normal((nb, rank))
    V = rng.standard_normal((n, rank))
    rb = row_blocks(n, block_end)
    V[rb < 0] = poison
    for k in range(rank):
        V[(rb >= 0) & (ranks[np.maximum(rb, 0)] <= k), k] = poison
        coef[ranks <= k, k] = poison
    return ranks, scale, coef, V


def assembled(n, block_end, block_rank, scale, coef, V):
    """blockdiag_b(scale_b I + V_b diag(c_b) V_b') (+) 0 as a dense longdouble matrix"""
    B = np.zeros((n, n), dtype=LD)
    begin = 0
    for b, end in enumerate(block_end):
        r = int(block_rank[b])
        Vb = np.asarray(V[begin:end, :r], dtype=LD)
        B[begin:end, begin:end] = LD(scale[b]) * np.eye(end - begin, dtype=LD) + (Vb * np.asarray(coef[b][:r], dtype=LD)) @ Vb.T
        begin = end
    return B


def block_recursion(kind, block_end, S, Y, npairs, memory, n):
    """the dense longdouble recursion of low_rank_ref.py per block, assembled block-diagonally; returns (B, scales,
    skipped) - a block without pairs is the identity, the linear range zero"""
    B = np.zeros((n, n), dtype=LD)
    scales, skipped = [], []
    begin = 0
    for b, end in enumerate(block_end):
        if npairs[b] == 0:
            B[begin:end, begin:end] = np.eye(end - begin, dtype=LD)
            scales.append(LD(1))
        else:
            Bb, sc, _, sk = dense_recursion(kind, S[begin:end, :npairs[b]], Y[begin:end, :npairs[b]], memory)
            B[begin:end, begin:end] = Bb
            scales.append(sc)
            skipped += [(b, j) for j in sk]
        begin = end
    return B, scales, skipped


def reference_product(n, Hfull, J, x, shift, term=None, e=None):
    """H x for H = H_user + sym(H0) + J' J + shift I + blockdiag_b(scale_b I + V_b diag(c_b) V_b') (+) 0 in
    numpy.longdouble and the bound of every entry.  Hfull: sym(H0) as CSR or None; J: r x n sparse or None; term:
    (block_end, block_rank, scale, coef, V) or None; e: the vector H_user x as the device product leaves it, or None.

    Bound of entry i, derived as low_rank_ref.reference_product derives its own: every term of the row's sum - e_i,
    H0_ij x_j, J_ei t_e, V_ik u_bk, scale_b x_i, shift x_i - goes through at most one rounding per term of the sums it
    stands in.  The row has `terms` terms and its longest t entry `longest`; in a row of block b the term adds r_b fused
    multiply-adds, plus 2 for u_bk = c_bk w_bk and the shuffle tree over a longer lane set, plus one term scale_b x_i:
    (terms + longest + r_b + 3) 2^-53 S_i with S_i the absolute sum of the terms.  On top the error w_bk carries in: a
    sum of len_b terms in any order, plus the segment and wave trees, is off by at most (len_b + 2) 2^-53
    sum_{j in b} |V_jk x_j|, and it enters row i with the weight |V_ik c_bk|.  Rows of the linear range get no term at
    all."""
    xl = x.astype(LD)
    want = np.zeros(n, dtype=LD)
    s_abs = np.zeros(n, dtype=LD)
    terms = np.zeros(n, dtype=np.int64)
    longest = np.zeros(n, dtype=np.int64)
    if e is not None:
        want += e.astype(LD)
        s_abs += np.abs(e.astype(LD))
        terms += 1
    if Hfull is not None:
        for i in range(n):
            c, v = Hfull.indices[Hfull.indptr[i]:Hfull.indptr[i + 1]], Hfull.data[Hfull.indptr[i]:Hfull.indptr[i + 1]].astype(LD)
            want[i] += (v * xl[c]).sum()
            s_abs[i] += np.abs(v * xl[c]).sum()
            terms[i] += c.size
    if J is not None and J.shape[0] > 0:
        r = J.shape[0]
        Jr, Jc = J.tocsr(), J.tocsc()
        t = np.zeros(r, dtype=LD)
        t_abs = np.zeros(r, dtype=LD)
        t_len = np.diff(Jr.indptr)
        for q in range(r):
            c, v = Jr.indices[Jr.indptr[q]:Jr.indptr[q + 1]], Jr.data[Jr.indptr[q]:Jr.indptr[q + 1]].astype(LD)
            t[q] = (v * xl[c]).sum()
            t_abs[q] = np.abs(v * xl[c]).sum()
        for i in range(n):
            q, v = Jc.indices[Jc.indptr[i]:Jc.indptr[i + 1]], Jc.data[Jc.indptr[i]:Jc.indptr[i + 1]].astype(LD)
            want[i] += (v * t[q]).sum()
            s_abs[i] += (np.abs(v) * t_abs[q]).sum()
            terms[i] += q.size
            longest[i] = int(t_len[q].max()) if q.size else 0
    if shift != 0.0:
        want += LD(shift) * xl
        s_abs += np.abs(LD(shift) * xl)
        terms += 1
    carried = np.zeros(n, dtype=LD)
    if term is not None:
        block_end, block_rank, scale, coef, V = term
        begin = 0
        for b, end in enumerate(block_end):
            rb = int(block_rank[b])
            xb = xl[begin:end]
            want[begin:end] += LD(scale[b]) * xb
            s_abs[begin:end] += np.abs(LD(scale[b]) * xb)
            terms[begin:end] += 1
            if rb > 0:
                Vb = np.asarray(V[begin:end, :rb], dtype=LD)
                cb = np.asarray(coef[b][:rb], dtype=LD)
                w = (Vb * xb[:, None]).sum(axis=0)
                w_abs = np.abs(Vb * xb[:, None]).sum(axis=0)
                u = cb * w
                want[begin:end] += (Vb * u).sum(axis=1)
                s_abs[begin:end] += np.abs(Vb * u).sum(axis=1)
                terms[begin:end] += rb + 2
                carried[begin:end] = (np.abs(Vb * cb) * w_abs).sum(axis=1) * (end - begin + 2) * LD(U)
            begin = end
    bound = (terms + longest) * LD(U) * s_abs + carried
    return want, bound
