// One-call same-message verification (blsgpu_verify_same_message): the glue between the randomized sums of k_awr.hip
// and the pairing kernels of k_miller.hip / k_group.hip.  Nothing here is heavy: each kernel is a lane per item that
// gathers what the existing kernels left on the device into the layout the next one reads (SoA, element i, word w at
// base[w * stride + i], so a wave's loads and stores per limb are 64 consecutive words).
//   k_same_group_items   per group: P_g = sum r_k pk_k (Jacobian, k_awr_sum) times the batch inverse of its z -> the
//                        affine pk_aff of the Miller loop, the group's AWR code and its include flag
//   k_same_retry_items   per retried set: its key (table entry or 96-byte encoding) as the affine P, its decoded
//                        signature as a Jacobian S (z = 1), its code and include flag -- a one-set CoreVerify, r = 1
//   k_same_results       verdicts and codes -> set_result / group_result
#include "k_common.hpp"

// The group's status as k_awr_serialize forms it: EMPTY_AGGREGATE, or the code of its lowest-index rejected set (the
// key's when both the key and the signature of that set are rejected).
BLS_INL int same_group_code(const AwrBuffers& a, uint32_t g) {
  if (a.group_first[g + 1] == a.group_first[g]) return BLS_EMPTY_AGGREGATE;
  const uint32_t kp = a.err_k[g], ks = a.err_k[a.n_groups + g];
  return kp <= ks ? a.err_c[g] : a.err_c[a.n_groups + g];
}

// inv: 1 / z of sum_pk (launch_batch_inv, stride n_groups; 0 for the identity).  A group enters the pairing check
// (include) when AWR accepted it and P_g is finite: P_g equal to the identity counts as a failed check.
__global__ __launch_bounds__(WAVE) void k_same_group_items(AwrBuffers a, const uint32_t* inv, uint32_t* pk_aff,
                                                           uint8_t* include, int8_t* code) {
  const uint32_t g = blockIdx.x * WAVE + threadIdx.x;
  if (g >= a.n_groups) return;
  const int st = same_group_code(a, g);
  g1a out;
  out.x = fp_zero();
  out.y = fp_zero();
  bool inc = false;
  if (st == BLS_OK) {
    const g1j R = ld_g1j(a.sum_pk, a.n_groups, g);
    if (!jac_is_inf(R)) {
      const fp zi = ld_fp(inv, a.n_groups, g, 0);
      const fp zi2 = fp_sqr(zi);
      out.x = fp_mul(R.x, zi2);
      out.y = fp_mul(R.y, fp_mul(zi2, zi));
      inc = true;
    }
  }
  st_g1a(pk_aff, a.n_groups, g, out);
  include[g] = inc ? 1 : 0;
  code[g] = (int8_t)st;
}

// Retried set q = set list[q] of the call (n_retry of them; the outputs' stride).  Its first error is the key's, then
// the signature's (k_job_mask's precedence); an identity signature has no error and is not included, so it answers 0.
__global__ __launch_bounds__(WAVE) void k_same_retry_items(AwrBuffers a, const uint32_t* list, uint32_t n_retry,
                                                           uint32_t* pk_aff, uint32_t* S, uint8_t* include,
                                                           int8_t* code) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  if (q >= n_retry) return;
  const uint32_t k = list[q];
  g1a P;
  P.x = fp_zero();
  P.y = fp_zero();
  int st = BLS_OK;
  if (a.pk_bytes) {
    uint8_t raw[96];
    const uint4* src = reinterpret_cast<const uint4*>(a.pk_bytes + (size_t)k * 96);
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const uint4 v = src[c];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; j++) raw[16 * c + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
    bool inf = false;
    g1a d;
    st = pk_decode96(raw, d, inf);
    if (st == BLS_OK && inf) st = BLS_PK_IS_INFINITY;
    if (st == BLS_OK) P = d;
  } else {
    const uint32_t idx = a.pk_index[k];
    if (idx >= a.pk_table_n)
      st = BLS_DEVICE_ERROR;  // (the runtime refuses such calls; the kernel's own guard)
    else
      P = ld_pktab(a.pk_table, idx);
  }
  if (st == BLS_OK) st = a.sig_status[k];
  const bool inc = st == BLS_OK && !(a.sig_flags[k] & SF_SIG_INF);
  st_g1a(pk_aff, n_retry, q, P);
  st_g2j(S, n_retry, q, inc ? jac_from_aff(ld_g2a(a.sig_aff, a.n, k)) : jac_infinity<fp2>());
  include[q] = inc ? 1 : 0;
  code[q] = (int8_t)st;
}

// Group phase (RETRY false), one lane per set and per group: group g is accepted when it was included and its check
// held; every set of an accepted group answers 1, every other set 0 until the retry phase answers for it.
// group_result: 1, 0, or -EMPTY_AGGREGATE for an empty group.
// Retry phase (RETRY true), one lane per retried set q: set_result[list[q]] = -code, or its own check's verdict.
template <bool RETRY>
__global__ __launch_bounds__(WAVE) void k_same_results(const uint32_t* group_first, uint32_t n_groups, uint32_t n_sets,
                                                       const uint32_t* list, uint32_t n_retry, const uint8_t* include,
                                                       const int8_t* code, const uint8_t* ok, int8_t* set_result,
                                                       int8_t* group_result) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  if (RETRY) {
    if (q >= n_retry) return;
    const int c = code[q];
    set_result[list[q]] = (int8_t)(c ? -c : (include[q] && ok[q]) ? 1 : 0);
    return;
  }
  if (q < n_groups) {
    const int c = code[q];
    group_result[q] = (int8_t)(c == BLS_EMPTY_AGGREGATE ? -BLS_EMPTY_AGGREGATE : (include[q] && ok[q]) ? 1 : 0);
  }
  if (q < n_sets) {
    // the group of set q: the last g with group_first[g] <= q (empty groups before it share that offset)
    uint32_t lo = 0, hi = n_groups;  // group_first[lo] <= q < group_first[hi]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (group_first[mid] <= q)
        lo = mid;
      else
        hi = mid;
    }
    set_result[q] = (include[lo] && ok[lo]) ? 1 : 0;
  }
}

static inline dim3 grid_for(uint32_t n) { return dim3((n + WAVE - 1) / WAVE); }

void launch_same_group_items(const AwrBuffers& a, const uint32_t* inv, uint32_t* pk_aff, uint8_t* include, int8_t* code,
                             hipStream_t s) {
  if (a.n_groups)
    hipLaunchKernelGGL(k_same_group_items, grid_for(a.n_groups), dim3(WAVE), 0, s, a, inv, pk_aff, include, code);
}
void launch_same_retry_items(const AwrBuffers& a, const uint32_t* list, uint32_t n_retry, uint32_t* pk_aff, uint32_t* S,
                             uint8_t* include, int8_t* code, hipStream_t s) {
  if (n_retry)
    hipLaunchKernelGGL(k_same_retry_items, grid_for(n_retry), dim3(WAVE), 0, s, a, list, n_retry, pk_aff, S, include,
                       code);
}
void launch_same_group_results(const uint32_t* group_first, uint32_t n_groups, uint32_t n_sets, const uint8_t* include,
                               const int8_t* code, const uint8_t* ok, int8_t* set_result, int8_t* group_result,
                               hipStream_t s) {
  const uint32_t n = n_groups > n_sets ? n_groups : n_sets;
  if (n)
    hipLaunchKernelGGL(k_same_results<false>, grid_for(n), dim3(WAVE), 0, s, group_first, n_groups, n_sets, nullptr, 0u,
                       include, code, ok, set_result, group_result);
}
void launch_same_retry_results(const uint32_t* list, uint32_t n_retry, const uint8_t* include, const int8_t* code,
                               const uint8_t* ok, int8_t* set_result, hipStream_t s) {
  if (n_retry)
    hipLaunchKernelGGL(k_same_results<true>, grid_for(n_retry), dim3(WAVE), 0, s, nullptr, 0u, 0u, list, n_retry,
                       include, code, ok, set_result, nullptr);
}
