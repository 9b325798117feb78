// aggregateWithRandomness for many groups at once (blsgpu_aggregate_with_randomness): per group P = sum r_k pk_k in
// G1 and S = sum r_k sig_k in G2 over the sets' trusted keys (table entries or 96-byte encodings) and the signatures
// k_sig_decode left in sig_aff (k_sig.hip), r_k the batch scalar of set k's word (k_common.hpp jac_mul_scalar_word),
// and the serialization of both sums.  One kernel template serves both groups (F = fp: keys, fp2: signatures); the
// lanes of a group combine by the forms of seg_sum.hpp, as k_sigagg.hip does.  A call with groups larger than their
// lanes take at one go is split (awr_parts.hpp): the same kernel sums parts of the groups and k_awr_fold adds each
// group's parts, so that a large group runs on as many waves as the chip has free.
#include "k_common.hpp"
#include "seg_sum.hpp"

// Set k's point.  Returns its status; *skip = it adds nothing (an identity signature).
BLS_INL int awr_point(const AwrBuffers& a, uint32_t k, g1j& P, bool& skip) {
  skip = false;
  g1a q;
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
    int st = pk_decode96(raw, q, inf);
    if (st == BLS_OK && inf) st = BLS_PK_IS_INFINITY;
    if (st != BLS_OK) return st;
  } else {
    const uint32_t idx = a.pk_index[k];
    if (idx >= a.pk_table_n) return BLS_DEVICE_ERROR;  // (the runtime refuses such calls; the kernel's own guard)
    q = ld_pktab(a.pk_table, idx);
  }
  P = jac_from_aff(q);
  return BLS_OK;
}
BLS_INL int awr_point(const AwrBuffers& a, uint32_t k, g2j& P, bool& skip) {
  const int st = a.sig_status[k];
  skip = st == BLS_OK && (a.sig_flags[k] & SF_SIG_INF);
  if (st == BLS_OK && !skip) P = jac_from_aff(ld_g2a(a.sig_aff, a.n, k));
  return st;
}

// One lane's share of group [first, last): sets first + t, first + t + L, ...; each finite point is scaled by its
// set's scalar and added to the lane's sum.  The window table of the scaling is the lane's column q of a.tab (entries
// 0..7, laid out as PipelineBuffers.scal_tab: SoA, stride a.tab_n); entry 8 keeps the running sum meanwhile, so the
// scaling has the register file to itself (k_sig_scale fills it).  The lane's error is its first: k ascends.
template <class F>
BLS_INL void awr_strided(const AwrBuffers& a, uint32_t first, uint32_t last, uint32_t t, uint32_t L, uint32_t q,
                         jac<F>& acc, uint32_t& err_k, int& err) {
#pragma unroll 1
  for (uint32_t k = first + t; k < last; k += L) {
    jac<F> P;
    bool skip;
    const int st = awr_point(a, k, P, skip);
    if (st != BLS_OK) {
      if (err == 0) {
        err = st;
        err_k = k;
      }
      continue;
    }
    if (skip) continue;
    // (the column's addresses are recomputed per set: hoisted out of the loop they are spilled, 445 registers' worth)
    const uint32_t qq = opaque_u32(q);
    tab_st(a.tab, a.tab_n, qq, 8, acc);
    const jac<F> R = jac_mul_scalar_word(P, a.words[k], a.tab, a.tab_n, qq);
    acc = jac_add(tab_ld<F>(a.tab, a.tab_n, opaque_u32(q), 8), R);
  }
}

BLS_INL uint32_t* awr_sums(const AwrBuffers& a, const g1j*) { return a.sum_pk; }
BLS_INL uint32_t* awr_sums(const AwrBuffers& a, const g2j*) { return a.sum_sig; }
template <class F>
BLS_INL void awr_store(const AwrBuffers& a, uint32_t g, const jac<F>& acc, uint32_t err_k, int err) {
  constexpr int which = sizeof(F) == sizeof(fp) ? 0 : 1;
  uint32_t* o = awr_sums(a, (const jac<F>*)0);
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&acc);
#pragma unroll
  for (int w = 0; w < (int)(sizeof(jac<F>) / 4); w++) o[(size_t)w * a.n_groups + g] = s[w];
  a.err_k[which * a.n_groups + g] = err_k;
  a.err_c[which * a.n_groups + g] = (int8_t)err;
}

// L lanes per group: 64 = one wave per group with the LDS tree, 32 / 16 / 8 = lane groups with the shuffle butterfly
// (64 / L groups per wave), 1 = a lane per group.  One wave per SIMD: the scaling takes the whole register file.
template <class F, int L>
STAGE_KERNEL_W(1) void k_awr_sum(AwrBuffers a) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;  // < a.tab_n: the launch is tab_n lanes
  const uint32_t t = q % L, g = q / L;
  const bool on = g < a.n_groups;  // whole groups: L divides WAVE, so a group never straddles a wave
  const uint32_t first = on ? a.group_first[g] : 0, last = on ? a.group_first[g + 1] : 0;
  jac<F> acc = jac_infinity<F>();
  uint32_t my_err_k = 0xffffffffu;
  int my_err = 0;
  awr_strided<F>(a, first, last, t, L, q, acc, my_err_k, my_err);
  if constexpr (L == WAVE) {
    __shared__ uint32_t red[SEG_SLOTS * (sizeof(jac<F>) / 4)];
    __shared__ uint32_t err_k[WAVE];
    __shared__ int32_t err_c[WAVE];
    uint32_t bk;
    int bc;
    seg_wave_first_error(err_k, err_c, t, my_err_k, my_err, bk, bc);
    if (last - first > 1) seg_wave_tree(acc, red, t);  // (uniform per workgroup)
    my_err_k = bk;
    my_err = bc;
  } else {
    seg_butterfly<F, L>(acc, my_err_k, my_err);
  }
  if (on && t == 0) awr_store<F>(a, g, acc, my_err_k, my_err);
}

// ---- split calls (awr_parts.hpp): k_awr_sum ran over the parts; group g's sum is the sum of its parts -------------
// One lane's share of the parts [first, last) of a group: parts first + t, first + t + L, ...  Each goes through the
// complete addition: two parts' sums may be equal, opposite or the identity.  The error is the lowest set index.
template <class F>
BLS_INL void awr_fold_strided(const AwrBuffers& p, uint32_t first, uint32_t last, uint32_t t, uint32_t L, jac<F>& acc,
                              uint32_t& err_k, int& err) {
  constexpr int which = sizeof(F) == sizeof(fp) ? 0 : 1;
  const uint32_t* sums = awr_sums(p, (const jac<F>*)0);
#pragma unroll 1
  for (uint32_t q = first + t; q < last; q += L) {
    jac<F> P;
    uint32_t* d = reinterpret_cast<uint32_t*>(&P);
#pragma unroll
    for (int w = 0; w < (int)(sizeof(jac<F>) / 4); w++) d[w] = sums[(size_t)w * p.n_groups + q];
    acc = jac_add(acc, P);
    const uint32_t k = p.err_k[which * p.n_groups + q];
    if (k < err_k) {
      err_k = k;
      err = p.err_c[which * p.n_groups + q];
    }
  }
}

// L lanes per group, the forms of k_sigagg.hip: 64 = a wave per group with the LDS tree, 32 / 16 / 8 = lane groups with
// the shuffle butterfly, 1 = a lane per group.  A few additions per lane: no occupancy bound is asked for.
template <class F, int L>
__global__ __launch_bounds__(WAVE) void k_awr_fold(AwrBuffers p, AwrBuffers a, const uint32_t* group_part) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  const uint32_t t = q % L, g = q / L;
  const bool on = g < a.n_groups;  // whole groups: L divides WAVE, so a group never straddles a wave
  const uint32_t first = on ? group_part[g] : 0, last = on ? group_part[g + 1] : 0;
  jac<F> acc = jac_infinity<F>();
  uint32_t my_err_k = 0xffffffffu;
  int my_err = 0;
  awr_fold_strided<F>(p, first, last, t, L, acc, my_err_k, my_err);
  if constexpr (L == WAVE) {
    __shared__ uint32_t red[SEG_SLOTS * (sizeof(jac<F>) / 4)];
    __shared__ uint32_t err_k[WAVE];
    __shared__ int32_t err_c[WAVE];
    uint32_t bk;
    int bc;
    seg_wave_first_error(err_k, err_c, t, my_err_k, my_err, bk, bc);
    if (last - first > 1) seg_wave_tree(acc, red, t);  // (uniform per workgroup)
    my_err_k = bk;
    my_err = bc;
  } else {
    seg_butterfly<F, L>(acc, my_err_k, my_err);
  }
  if (on && t == 0) awr_store<F>(a, g, acc, my_err_k, my_err);
}

// Both sums' toBytes(), one lane per group (one Fp and one Fp2 inversion each): P in 48 (compressed) or 96 bytes, S in
// 96 (compressed) or 192; the identity encoding for a sum equal to the identity, zeros for a rejected or empty group.
// The group's status is EMPTY_AGGREGATE, or the code of its lowest-index rejected set -- the key's when both the key
// and the signature of that set are rejected (the reference holds deserialized keys before it reads a signature).
__global__ __launch_bounds__(WAVE) void k_awr_serialize(AwrBuffers a, uint8_t* out_pk, uint32_t out_pk_len,
                                                        uint8_t* out_sig, uint32_t out_sig_len, int8_t* status,
                                                        uint32_t* first_bad) {
  const uint32_t g = blockIdx.x * WAVE + threadIdx.x;
  if (g >= a.n_groups) return;
  const uint32_t kp = a.err_k[g], ks = a.err_k[a.n_groups + g];
  const bool key_first = kp <= ks;
  const uint32_t bad = key_first ? kp : ks;
  int st = key_first ? a.err_c[g] : a.err_c[a.n_groups + g];
  if (a.group_first[g + 1] == a.group_first[g]) st = BLS_EMPTY_AGGREGATE;
  uint8_t buf[192];
  for (int k = 0; k < 192; k++) buf[k] = 0;
  if (st == BLS_OK) {
    g1a p;
    if (!jac_to_aff(ld_g1j(a.sum_pk, a.n_groups, g), p)) {
      buf[0] = out_pk_len == 48 ? 0xc0 : 0x40;
    } else if (out_pk_len == 48) {
      g1a_compress(p, buf);
    } else {
      g1a_to_be96(p, buf);
    }
  }
  uint8_t* o = out_pk + (size_t)g * out_pk_len;
  for (uint32_t k = 0; k < out_pk_len; k++) o[k] = buf[k];
  for (int k = 0; k < 96; k++) buf[k] = 0;
  if (st == BLS_OK) {
    g2a s;
    if (!jac_to_aff(ld_g2j(a.sum_sig, a.n_groups, g), s)) {
      buf[0] = out_sig_len == 96 ? 0xc0 : 0x40;
    } else if (out_sig_len == 96) {
      g2a_compress(s, buf);
    } else {
      g2a_to_be192(s, buf);
    }
  }
  o = out_sig + (size_t)g * out_sig_len;
  for (uint32_t k = 0; k < out_sig_len; k++) o[k] = buf[k];
  status[g] = (int8_t)st;
  first_bad[g] = st == BLS_OK || st == BLS_EMPTY_AGGREGATE ? 0xffffffffu : bad;
}

uint32_t awr_launch_lanes(uint32_t n_groups, uint32_t L) {
  return (uint32_t)(((uint64_t)n_groups * L + WAVE - 1) / WAVE) * WAVE;
}

template <class F>
static void launch_awr_sum(const AwrBuffers& a, uint32_t L, hipStream_t s) {
  if (!a.n_groups) return;
  const dim3 grid(a.tab_n / WAVE);
#define AWR_SUM(l) hipLaunchKernelGGL((k_awr_sum<F, l>), grid, dim3(WAVE), 0, s, a)
  switch (L) {
    case 64: AWR_SUM(64); break;
    case 32: AWR_SUM(32); break;
    case 16: AWR_SUM(16); break;
    case 8: AWR_SUM(8); break;
    default: AWR_SUM(1); break;
  }
#undef AWR_SUM
}
void launch_awr_sum_pk(const AwrBuffers& a, uint32_t L, hipStream_t s) { launch_awr_sum<fp>(a, L, s); }
void launch_awr_sum_sig(const AwrBuffers& a, uint32_t L, hipStream_t s) { launch_awr_sum<fp2>(a, L, s); }
void launch_awr_sums(const AwrBuffers& a, uint32_t L, hipStream_t s) {
  launch_awr_sum_pk(a, L, s);
  launch_awr_sum_sig(a, L, s);
}
template <class F>
static void launch_awr_fold(const AwrBuffers& p, const AwrBuffers& a, const uint32_t* group_part, uint32_t L,
                            hipStream_t s) {
  if (!a.n_groups) return;
  const dim3 grid(awr_launch_lanes(a.n_groups, L) / WAVE);
#define AWR_FOLD(l) hipLaunchKernelGGL((k_awr_fold<F, l>), grid, dim3(WAVE), 0, s, p, a, group_part)
  switch (L) {
    case 64: AWR_FOLD(64); break;
    case 32: AWR_FOLD(32); break;
    case 16: AWR_FOLD(16); break;
    case 8: AWR_FOLD(8); break;
    default: AWR_FOLD(1); break;
  }
#undef AWR_FOLD
}
void launch_awr_fold_pk(const AwrBuffers& parts, const AwrBuffers& a, const uint32_t* group_part, uint32_t L,
                        hipStream_t s) {
  launch_awr_fold<fp>(parts, a, group_part, L, s);
}
void launch_awr_fold_sig(const AwrBuffers& parts, const AwrBuffers& a, const uint32_t* group_part, uint32_t L,
                         hipStream_t s) {
  launch_awr_fold<fp2>(parts, a, group_part, L, s);
}
void launch_awr_serialize(const AwrBuffers& a, uint8_t* out_pk, uint32_t out_pk_len, uint8_t* out_sig,
                          uint32_t out_sig_len, int8_t* status, uint32_t* first_bad, hipStream_t s) {
  if (a.n_groups)
    hipLaunchKernelGGL(k_awr_serialize, dim3((a.n_groups + WAVE - 1) / WAVE), dim3(WAVE), 0, s, a, out_pk, out_pk_len,
                       out_sig, out_sig_len, status, first_bad);
}
