// runtime_qn_ring.inc - the quasi-Newton term built on the device from pairs kept in HBM, as an object of the handle
// (hipfact_qn_ring, include/hipfact.h; abi_qn_ring.inc holds its entry points, qn_gram_rule.h the rule that turns the
// Gram matrix into coefficients, kernels_qn.inc the kernels)
// (part of the single translation unit hipfact.hip; included from there, in this order)

// S and Y (n x memory) and V (n x 2 memory) in HBM, column-major with ld = n rounded up to even.  The slots of S and Y are
// circular: pair number p (counted from the last reset) lives in column p % memory, a push overwrites the oldest one and
// nothing is moved.  A build leaves G, C, coef and the outcome on the host; `built` says that they belong to the pairs
// as they stand.
struct hipfact_qn_ring {
  hipfact_handle* h = nullptr;
  int n = 0, kind = 0, memory = 0;
  long long ld = 0;
  long pushed = 0;  // pairs pushed since the last reset
  DevBuf d_S, d_Y, d_V;
  DevBuf d_part, d_G, d_C;  // 768 doubles per workgroup of k_qn_gram | 32 x 32 | 32 x 32
  PinBuf h_G, h_C;          // 32 x 32 doubles each
  int nwg = 1, rows_per_wg = HIPFACT_QN_TILE;
  bool built = false;
  int used = 0, rank = 0;
  unsigned damped = 0u, skipped = 0u;
  double scale = 1.0;
  double coef[2 * HIPFACT_QN_MAX_PAIRS] = {0.0};
  double G[4 * HIPFACT_QN_MAX_PAIRS * HIPFACT_QN_MAX_PAIRS] = {0.0};  // 2 used x 2 used, column-major, of the last build
};

// the slot list of the used pairs, oldest first
static QnSlots qn_ring_slots(const hipfact_qn_ring* R, int* used) {
  QnSlots sl;
  const int L = (int)std::min<long>(R->pushed, R->memory);
  for (int j = 0; j < 16; ++j) sl.s[j] = j < L ? (int)((R->pushed - L + j) % R->memory) : 0;
  *used = L;
  return sl;
}
