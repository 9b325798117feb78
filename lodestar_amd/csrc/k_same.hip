// One-call same-message verification (blsgpu_verify_same_message): the glue between the randomized sums of k_awr.hip
// and the pairing kernels of k_miller.hip / k_group.hip.  Nothing here is heavy: each kernel is a lane per item that
// gathers what the existing kernels left on the device into the layout the next one reads (SoA, element i, word w at
// base[w * stride + i], so a wave's loads and stores per limb are 64 consecutive words).
//   k_same_group_items   per group: P_g = sum r_k pk_k (Jacobian, k_awr_sum) times the batch inverse of its z -> the
//                        affine pk_aff of the Miller loop, the group's AWR code and its include flag
//   k_same_retry_items   per retried set: its key (table entry or 96-byte encoding) as the affine P, its decoded
//                        signature as a Jacobian S (z = 1), its code and include flag -- a one-set CoreVerify, r = 1
//   k_same_results       verdicts and codes -> set_result / group_result
// With BLSGPU_SAME_BLOCK_CHECK the groups' Miller values are checked a block of groups at a time:
//   k_same_block_sum        one wave per block: S_b = sum S_g over the block's included groups (at most 16 G2 additions
//                           per lane, then an LDS tree), beside the groups' Miller loops
//   k_same_block_pairs      F_b = prod F_g over them as a tree of cooperative Fp12 products, a launch per level
//   k_same_block_results    block verdicts -> set_result / group_result
//   k_same_gather           the groups of failed blocks: F_g, S_g into compact arrays for their own checks (the descent)
//   k_same_descent_results  those checks' verdicts -> set_result / group_result
#include "k_common.hpp"
#include "gt_wave.hpp"

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

// ---- BLSGPU_SAME_BLOCK_CHECK: one check per block of SAME_BLOCK_GROUPS groups ------------------------
// Block b = groups [SAME_BLOCK_GROUPS b, min(n_groups, SAME_BLOCK_GROUPS (b + 1))).  F_b = the product of F_g (W_FP12,
// stride n_groups) and S_b = the sum of S_g (W_G2J, stride n_groups) over the block's groups with include[g].
//
// S_b and any[b] (whether the block has an included group), one wave per block: each lane folds the groups lane,
// lane + 64, .. of its block (at most 16 Jacobian additions), then a 6-level LDS tree as in k_group_reduce.  It needs
// only the sums and the include flags, so the call runs it beside the groups' Miller loops.  Output: stride n_blocks,
// the layout k_group_check and k_group_sig_miller_lane read.
__global__ __launch_bounds__(WAVE) void k_same_block_sum(const uint32_t* S_in, const uint8_t* include, uint32_t n_groups,
                                                         uint32_t n_blocks, uint32_t* S_out, uint8_t* any) {
  __shared__ uint32_t red[WAVE * W_G2J];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  const uint32_t first = b * SAME_BLOCK_GROUPS;
  if (b >= n_blocks || first >= n_groups) return;  // (the whole wave leaves: no barrier is left waiting)
  const uint32_t last = n_groups - first < SAME_BLOCK_GROUPS ? n_groups : first + SAME_BLOCK_GROUPS;
  g2j S = jac_infinity<fp2>();
  bool have = false;
#pragma unroll 1
  for (uint32_t g = first + lane; g < last; g += WAVE)
    if (include[g]) {
      S = jac_add(S, ld_g2j(S_in, n_groups, g));
      have = true;
    }
#pragma unroll 1
  for (int h = WAVE / 2; h >= 1; h >>= 1) {
    if (lane >= (uint32_t)h && lane < (uint32_t)(2 * h)) st_g2j(red, WAVE, lane - h, S);
    __syncthreads();
    if (lane < (uint32_t)h) S = jac_add(S, ld_g2j(red, WAVE, lane));
    __syncthreads();
  }
  const unsigned long long m = __ballot(have);
  if (lane == 0) {
    st_g2j(S_out, n_blocks, b, S);
    any[b] = m ? 1 : 0;
  }
}

// F_b as a product tree, one launch per level and one 128-lane workgroup per product (gt_wave.hpp gtw_mul, as
// k_f_pairs): a level of `width` outputs per block writes out[b * width + i] = in[2 (b * width + i)] * in[.. + 1].
// FIRST: the inputs are the groups' F_g, entry i of block b being group SAME_BLOCK_GROUPS b + i; a group past n_groups
// or without include[g] counts as one, so every later level finds all of its inputs written.  The levels never touch
// F_g itself (the descent reads it again); the last level (width 1) writes F_b, stride n_blocks, in the layout
// k_group_check / k_group_check6 read.  A one-wave form (each lane folding 16 groups, then an LDS tree of lane-serial
// fp12_mul, as k_group_reduce) was measured first and was slower: DESIGN.md 4.4.
template <bool FIRST>
__global__ __launch_bounds__(GTW_LANES) void k_same_block_pairs(const uint32_t* in, uint32_t in_stride,
                                                                const uint8_t* include, uint32_t n_groups,
                                                                uint32_t width, uint32_t* out, uint32_t out_stride) {
  __shared__ uint32_t A[GTW_FP12], B[GTW_FP12], S[108 * BLS_NL];
  const uint32_t t = threadIdx.x, o = blockIdx.x;
  uint32_t e0 = 2 * o, e1 = 2 * o + 1;
  bool h0 = true, h1 = true;
  if (FIRST) {
    e0 = (o / width) * SAME_BLOCK_GROUPS + 2 * (o % width);
    e1 = e0 + 1;
    h0 = e0 < n_groups && include[e0];
    h1 = e1 < n_groups && include[e1];
  }
  if (!h0 || !h1) {  // (uniform over the workgroup) at most one factor: a copy of it, or one
    const uint32_t e = h0 ? e0 : e1;
    for (uint32_t w = t; w < W_FP12; w += GTW_LANES)
      out[(size_t)w * out_stride + o] = (h0 || h1) ? in[(size_t)w * in_stride + e] : (w < BLS_NL ? FP_ONE.l[w] : 0u);
    return;
  }
  for (uint32_t w = t; w < W_FP12; w += GTW_LANES) {
    A[gtw_lds_word(w)] = in[(size_t)w * in_stride + e0];
    B[gtw_lds_word(w)] = in[(size_t)w * in_stride + e1];
  }
  gtw_sync();
  gtw_mul<false>(A, A, B, S, t);
  for (uint32_t w = t; w < W_FP12; w += GTW_LANES) out[(size_t)w * out_stride + o] = A[gtw_lds_word(w)];
}

// the group of set q: the last g with group_first[g] <= q (empty groups before it share that offset)
BLS_INL uint32_t same_group_of(const uint32_t* group_first, uint32_t n_groups, uint32_t q) {
  uint32_t lo = 0, hi = n_groups;  // group_first[lo] <= q < group_first[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (group_first[mid] <= q)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// Block phase results, one lane per set and per group (as k_same_results<false>): an included group of a block that
// held at least one (any) and whose check held (ok) is accepted, with every set of it; every other group answers 0
// (-EMPTY_AGGREGATE when empty) until the descent or the retry phase answers for it.
__global__ __launch_bounds__(WAVE) void k_same_block_results(const uint32_t* group_first, uint32_t n_groups,
                                                             uint32_t n_sets, const uint8_t* include, const int8_t* code,
                                                             const uint8_t* any, const uint8_t* ok, int8_t* set_result,
                                                             int8_t* group_result) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  if (q < n_groups) {
    const uint32_t b = q / SAME_BLOCK_GROUPS;
    group_result[q] =
        (int8_t)(code[q] == BLS_EMPTY_AGGREGATE ? -BLS_EMPTY_AGGREGATE : (include[q] && any[b] && ok[b]) ? 1 : 0);
  }
  if (q < n_sets) {
    const uint32_t g = same_group_of(group_first, n_groups, q), b = g / SAME_BLOCK_GROUPS;
    set_result[q] = (include[g] && any[b] && ok[b]) ? 1 : 0;
  }
}

// Descent: the listed groups' F_g and S_g (stride n_groups) into compact arrays of stride n_listed, lane per (listed
// group, word) as k_f_gather; words [0, W_FP12) are F's, the next W_G2J are S's.
__global__ __launch_bounds__(WAVE) void k_same_gather(const uint32_t* F_in, const uint32_t* S_in, uint32_t n_groups,
                                                      const uint32_t* list, uint32_t n_listed, uint32_t* F_out,
                                                      uint32_t* S_out) {
  const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= n_listed * (W_FP12 + W_G2J)) return;
  const uint32_t q = i % n_listed, w = i / n_listed, g = list[q];
  if (w < W_FP12)
    F_out[(size_t)w * n_listed + q] = F_in[(size_t)w * n_groups + g];
  else
    S_out[(size_t)(w - W_FP12) * n_listed + q] = S_in[(size_t)(w - W_FP12) * n_groups + g];
}

// Descent results, one lane per listed group and per set: listed group list[q] (ascending) answers its own check's
// verdict ok[q], and so does every set of it; what is not listed keeps the block phase's answer.
__global__ __launch_bounds__(WAVE) void k_same_descent_results(const uint32_t* group_first, uint32_t n_groups,
                                                               uint32_t n_sets, const uint32_t* list, uint32_t n_listed,
                                                               const uint8_t* ok, int8_t* set_result,
                                                               int8_t* group_result) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  if (q < n_listed) group_result[list[q]] = ok[q] ? 1 : 0;
  if (q < n_sets) {
    const uint32_t g = same_group_of(group_first, n_groups, q);
    uint32_t lo = 0, hi = n_listed;  // the first position with list[lo] >= g
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (list[mid] < g)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < n_listed && list[lo] == g) set_result[q] = ok[lo] ? 1 : 0;
  }
}

static inline dim3 grid_for(uint32_t n) { return dim3((n + WAVE - 1) / WAVE); }

void launch_same_block_sum(const uint32_t* S, const uint8_t* include, uint32_t n_groups, uint32_t n_blocks,
                           uint32_t* S_out, uint8_t* any, hipStream_t s) {
  if (n_blocks)
    hipLaunchKernelGGL(k_same_block_sum, dim3(n_blocks), dim3(WAVE), 0, s, S, include, n_groups, n_blocks, S_out, any);
}
uint32_t same_block_tree_width(uint32_t n_groups) {
  const uint32_t in_block = n_groups < SAME_BLOCK_GROUPS ? n_groups : SAME_BLOCK_GROUPS;
  uint32_t w = 1;
  while (2 * w < in_block) w *= 2;
  return w;
}
void launch_same_block_prod(const uint32_t* F, const uint8_t* include, uint32_t n_groups, uint32_t n_blocks,
                            uint32_t* T0, uint32_t* T1, uint32_t* F_out, hipStream_t s) {
  if (!n_blocks) return;
  uint32_t width = same_block_tree_width(n_groups);
  const uint32_t* in = F;
  uint32_t in_stride = n_groups;
  for (int level = 0;; level++, width /= 2) {
    const uint32_t n_out = n_blocks * width;
    uint32_t* out = width == 1 ? F_out : (level & 1) ? T1 : T0;
    if (level == 0)
      hipLaunchKernelGGL(k_same_block_pairs<true>, dim3(n_out), dim3(GTW_LANES), 0, s, in, in_stride, include, n_groups,
                         width, out, n_out);
    else
      hipLaunchKernelGGL(k_same_block_pairs<false>, dim3(n_out), dim3(GTW_LANES), 0, s, in, in_stride, nullptr, 0u, width,
                         out, n_out);
    if (width == 1) break;
    in = out, in_stride = n_out;
  }
}
void launch_same_block_results(const uint32_t* group_first, uint32_t n_groups, uint32_t n_sets, const uint8_t* include,
                               const int8_t* code, const uint8_t* any, const uint8_t* ok, int8_t* set_result,
                               int8_t* group_result, hipStream_t s) {
  const uint32_t n = n_groups > n_sets ? n_groups : n_sets;
  if (n)
    hipLaunchKernelGGL(k_same_block_results, grid_for(n), dim3(WAVE), 0, s, group_first, n_groups, n_sets, include, code,
                       any, ok, set_result, group_result);
}
void launch_same_gather(const uint32_t* F, const uint32_t* S, uint32_t n_groups, const uint32_t* list,
                        uint32_t n_listed, uint32_t* F_out, uint32_t* S_out, hipStream_t s) {
  if (n_listed)
    hipLaunchKernelGGL(k_same_gather, grid_for(n_listed * (W_FP12 + W_G2J)), dim3(WAVE), 0, s, F, S, n_groups, list,
                       n_listed, F_out, S_out);
}
void launch_same_descent_results(const uint32_t* group_first, uint32_t n_groups, uint32_t n_sets, const uint32_t* list,
                                 uint32_t n_listed, const uint8_t* ok, int8_t* set_result, int8_t* group_result,
                                 hipStream_t s) {
  const uint32_t n = n_listed > n_sets ? n_listed : n_sets;
  if (n)
    hipLaunchKernelGGL(k_same_descent_results, grid_for(n), dim3(WAVE), 0, s, group_first, n_groups, n_sets, list,
                       n_listed, ok, set_result, group_result);
}

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
