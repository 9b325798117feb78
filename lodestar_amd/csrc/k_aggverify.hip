// Batched AggregateVerify (blsgpu_aggregate_verify): the glue between the decodes, hash_to_G2 and the pairing kernels
// of k_miller.hip / k_group.hip, and the check with no second operand.  A job of k (key, message) pairs and one
// signature is k + 1 Miller items: the signature rides along as the pair (-g1, sig), in the job's own accumulators, so
// the job costs one shared-squaring multi-pairing and one final exponentiation:
//   FinalExp( prod_k MillerLoop(pk_k, H(m_k)) * MillerLoop(-g1, sig) ) == 1
// Items (stride n_items = pairs + jobs): pair k is item k, job j's signature item is item n_pairs + j.  G2 columns
// (stride nm = unique messages + jobs): message u is column u, job j's signature is column n_umsg + j.
//   k_av_pair_items   lane per pair: its key (table entry, trusted 96-byte encoding, or KeyValidate's output) as the
//                     affine P of item k, the pair's error code and its message column
//   k_av_job_items    lane per job: the job's status (empty, else its lowest-index rejected key, else its signature's
//                     error), first_bad, whether the job is checked (no error, finite signature), the decoded signature
//                     as G2 column n_umsg + j, the signature item, and the include bytes of all the job's items
//   k_av_reduce_lane  lane per job: F_j = the product of the job's chunk values (calls of many small jobs; otherwise
//                     k_group_reduce, a wave per job)
//   k_av_check        ok[j] = FinalExp(F_j) == 1: one cooperative workgroup per job (gt_wave.hpp), or six lanes per job
//                     (gt6.hpp); jobs that are not checked are skipped
//   k_av_results      job_result[j] = -code, or the verdict
#include "k_common.hpp"
#include "gt_wave.hpp"
#include "gt6.hpp"

__global__ __launch_bounds__(WAVE) void k_av_pair_items(AvBuffers a) {
  const uint32_t k = blockIdx.x * WAVE + threadIdx.x;
  if (k >= a.n_pairs) return;
  g1a P;
  P.x = fp_zero();
  P.y = fp_zero();
  int st = a.kv_status ? (int)a.kv_status[k] : BLS_OK;
  if (st != BLS_OK) {
    // (KeyValidate rejected the key: its 96 output bytes are zero)
  } else if (a.pk_bytes) {
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
  st_g1a(a.pk_aff, a.n_items, k, P);
  a.msg_idx[k] = a.pair_msg[k];
  a.pair_code[k] = (int8_t)st;
}

// Keys before the signature (k_job_mask's precedence); an identity signature has no error and is not checked, so the
// job answers 0.  A job that is not checked keeps every item switched off: its accumulators stay 1, its signature
// column is flagged MF_H_INF (no lines are computed for it) and k_av_check skips it.
__global__ __launch_bounds__(WAVE) void k_av_job_items(AvBuffers a) {
  const uint32_t j = blockIdx.x * WAVE + threadIdx.x;
  if (j >= a.n_jobs) return;
  const uint32_t first = a.job_first[j], last = a.job_first[j + 1];
  int st = BLS_OK;
  uint32_t bad = 0xffffffffu;
  if (first == last) {
    st = BLS_EMPTY_AGGREGATE;
  } else {
    for (uint32_t k = first; k < last && st == BLS_OK; k++) {
      st = a.pair_code[k];
      if (st != BLS_OK) bad = k;
    }
    if (st == BLS_OK) st = a.sig_status[j];
  }
  const bool chk = st == BLS_OK && !(a.sig_flags[j] & SF_SIG_INF);
  const uint32_t item = a.n_pairs + j, col = a.n_umsg + j;
  g2a S;
  S.x = fp2_zero();
  S.y = fp2_zero();
  if (chk) S = ld_g2a(a.sig_aff, a.n_jobs, j);
  st_g2a(a.h_aff, a.nm, col, S);
  a.mflags[col] = chk ? 0 : MF_H_INF;
  g1a P;
  P.x = G1_GEN_X;
  P.y = G1_NEG_GEN_Y;
  st_g1a(a.pk_aff, a.n_items, item, P);
  a.msg_idx[item] = col;
  a.include[item] = chk ? 1 : 0;
  for (uint32_t k = first; k < last; k++) a.include[k] = chk ? 1 : 0;
  a.job_code[j] = (int8_t)st;
  a.checked[j] = chk ? 1 : 0;
  a.first_bad[j] = bad;
}

STAGE_KERNEL_W(BLSGPU_WPE_GRP) void k_av_reduce_lane(const uint32_t* f_chunk, uint32_t stride, const uint32_t* f_ranges,
                                                    uint32_t n_jobs, uint32_t* F_out) {
  const uint32_t j = blockIdx.x * WAVE + threadIdx.x;
  if (j >= n_jobs) return;
  const uint32_t first = f_ranges[2 * j], last = f_ranges[2 * j + 1];
  fp12 F = first < last ? ld_fp12(f_chunk, stride, first) : fp12_one();
#pragma unroll 1
  for (uint32_t c = first + 1; c < last; c++) F = fp12_mul(F, ld_fp12(f_chunk, stride, c));
  st_fp12(F_out, n_jobs, j, F);
}

// One GTW_LANES workgroup per job: the final exponentiation as cooperative Fp12 arithmetic (k_group_check without its
// second operand).  F in HBM: SoA tower layout, stride n_jobs; in LDS: the w-basis.
__global__ __launch_bounds__(GTW_LANES) void k_av_check(const uint32_t* F_in, uint32_t n_jobs, const uint8_t* checked,
                                                        uint8_t* ok) {
  __shared__ GtwLds sh;
  const uint32_t t = threadIdx.x, j = blockIdx.x;
  if (j >= n_jobs) return;
  if (!checked[j]) {  // (uniform over the workgroup)
    if (t == 0) ok[j] = 0;
    return;
  }
  for (uint32_t w = t; w < W_FP12; w += GTW_LANES) sh.F[gtw_lds_word(w)] = F_in[(size_t)w * n_jobs + j];
  gtw_sync();
  gtw_final_exp(sh.F, sh.W, sh.S, t);
  if (t == 0) ok[j] = fp12_is_one(gtw_to_reg(sh.F)) ? 1 : 0;
}

// Six lanes per job (gt6.hpp, as k_group_check6): ten jobs per wave.
STAGE_KERNEL_W(BLSGPU_WPE_GRP) void k_av_check6(const uint32_t* F_in, uint32_t n_jobs, const uint8_t* checked,
                                               uint8_t* ok) {
  const uint32_t lane = threadIdx.x, grp = lane / 6, k = lane % 6;
  const uint32_t j = blockIdx.x * ACC6_GROUPS + grp;
  if (grp >= ACC6_GROUPS || j >= n_jobs) return;  // whole groups leave together
  if (!checked[j]) {                              // (the same on the six lanes of a group)
    if (k == 0) ok[j] = 0;
    return;
  }
  const G6 g{(int)(grp * 6), k};
  const int w0 = ((k & 1) ? 3 : 0) * 2 * W_FP + (int)(k >> 1) * 2 * W_FP;
  const fp2 F = ld_fp2(F_in, n_jobs, j, w0);
  const bool one = g6_is_one(g6_final_exp(F, g), g);
  if (k == 0) ok[j] = one ? 1 : 0;
}

__global__ __launch_bounds__(WAVE) void k_av_results(uint32_t n_jobs, const int8_t* code, const uint8_t* checked,
                                                     const uint8_t* ok, int8_t* job_result) {
  const uint32_t j = blockIdx.x * WAVE + threadIdx.x;
  if (j >= n_jobs) return;
  const int c = code[j];
  job_result[j] = (int8_t)(c ? -c : (checked[j] && ok[j]) ? 1 : 0);
}

static inline dim3 grid_for(uint32_t n) { return dim3((n + WAVE - 1) / WAVE); }

void launch_av_pair_items(const AvBuffers& a, hipStream_t s) {
  if (a.n_pairs) hipLaunchKernelGGL(k_av_pair_items, grid_for(a.n_pairs), dim3(WAVE), 0, s, a);
}
void launch_av_job_items(const AvBuffers& a, hipStream_t s) {
  if (a.n_jobs) hipLaunchKernelGGL(k_av_job_items, grid_for(a.n_jobs), dim3(WAVE), 0, s, a);
}
void launch_av_reduce_lane(const uint32_t* f_chunk, uint32_t stride, const uint32_t* f_ranges, uint32_t n_jobs,
                           uint32_t* F, hipStream_t s) {
  if (n_jobs)
    hipLaunchKernelGGL(k_av_reduce_lane, grid_for(n_jobs), dim3(WAVE), 0, s, f_chunk, stride, f_ranges, n_jobs, F);
}
void launch_av_check(const uint32_t* F, uint32_t n_jobs, const uint8_t* checked, uint8_t* ok, bool lane, hipStream_t s) {
  if (!n_jobs) return;
  if (lane)
    hipLaunchKernelGGL(k_av_check6, dim3((n_jobs + ACC6_GROUPS - 1) / ACC6_GROUPS), dim3(WAVE), 0, s, F, n_jobs, checked,
                       ok);
  else
    hipLaunchKernelGGL(k_av_check, dim3(n_jobs), dim3(GTW_LANES), 0, s, F, n_jobs, checked, ok);
}
void launch_av_results(uint32_t n_jobs, const int8_t* code, const uint8_t* checked, const uint8_t* ok,
                       int8_t* job_result, hipStream_t s) {
  if (n_jobs) hipLaunchKernelGGL(k_av_results, grid_for(n_jobs), dim3(WAVE), 0, s, n_jobs, code, checked, ok, job_result);
}
