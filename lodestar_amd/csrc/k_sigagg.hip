// Signature.aggregate(sigs.map(fromBytes)).toBytes() for many groups at once (blsgpu_aggregate_signatures): the
// segmented G2 sum over the signatures k_sig_decode left in sig_aff (k_sig.hip), and its serialization.  The G2 twin
// of k_pk_aggregate / k_pk_aggregate_g / k_pk_serialize (k_pk.hip).
#include "k_common.hpp"
#include "seg_sum.hpp"

// One lane's share of group [first, last): the sum of the signatures k = first + t, first + t + L, ... that take(k)
// admits, k ascending.  The mixed addition keeps its doubling and cancelling branches (curve.hpp).
template <class Take>
BLS_INL void g2_sum_strided(const uint32_t* sig_aff, uint32_t n, uint32_t first, uint32_t last, uint32_t t, uint32_t L,
                            g2j& acc, Take take) {
#pragma unroll 1
  for (uint32_t k = first + t; k < last; k += L)
    if (take(k)) acc = jac_add_aff(acc, ld_g2a(sig_aff, n, k));
}

// blsgpu_aggregate_signatures: a rejected signature (decode or subgroup status) is the lane's error when it is the
// lane's first -- k ascends, so that is the lane's lowest index; an identity signature adds nothing.
BLS_INL void sig_agg_strided(const PipelineBuffers& b, uint32_t first, uint32_t last, uint32_t t, uint32_t L, g2j& acc,
                             uint32_t& err_k, int& err) {
  g2_sum_strided(b.sig_aff, b.n, first, last, t, L, acc, [&](uint32_t k) {
    const int st = b.status[k];
    if (st != BLS_OK) {
      if (err == 0) {
        err = st;
        err_k = k;
      }
      return false;
    }
    return !(b.flags[k] & SF_SIG_INF);
  });
}

// blsgpu_verify_same_message_agg: the sets that verified (set_result 1, so decoded, in the subgroup and finite) and
// that the caller's mask admits (include null: all); `count` is how many the lane summed.
BLS_INL void same_agg_strided(const uint32_t* sig_aff, uint32_t n, const int8_t* set_result, const uint8_t* include,
                              uint32_t first, uint32_t last, uint32_t t, uint32_t L, g2j& acc, uint32_t& count) {
  g2_sum_strided(sig_aff, n, first, last, t, L, acc, [&](uint32_t k) {
    const bool take = set_result[k] == 1 && (!include || include[k]);
    count += take ? 1u : 0u;
    return take;
  });
}

// One wave per group: strided partial sums, then the LDS tree of seg_sum.hpp (WAVE / 2 slots of W_G2J words = 10.5
// KB).  The group's first error is the lowest signature index of any lane.
__global__ __launch_bounds__(WAVE) void k_sig_aggregate(PipelineBuffers b, const uint32_t* group_first,
                                                        uint32_t n_groups, uint32_t* agg, int8_t* agg_status,
                                                        uint32_t* first_bad) {
  __shared__ uint32_t red[SEG_SLOTS * W_G2J];
  __shared__ uint32_t err_k[WAVE];
  __shared__ int32_t err_c[WAVE];
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t first = group_first[g], last = group_first[g + 1];
  g2j acc = jac_infinity<fp2>();
  uint32_t my_err_k = 0xffffffffu;
  int my_err = 0;
  sig_agg_strided(b, first, last, lane, WAVE, acc, my_err_k, my_err);
  uint32_t bk;
  int bc;
  seg_wave_first_error(err_k, err_c, lane, my_err_k, my_err, bk, bc);
  if (lane == 0) {
    agg_status[g] = (int8_t)bc;
    first_bad[g] = bk;
  }
  if (last - first > 1) seg_wave_tree(acc, red, lane);  // (uniform per workgroup)
  if (lane == 0) st_g2j(agg, n_groups, g, acc);
}

// The same sum on L lanes per group (64 / L groups per wave; L = 32, 16, 8 or 1), the partial sums combined by the
// in-register butterfly of seg_sum.hpp (84 words per level, no LDS, no barrier).  L = 1 is a lane per group, no
// butterfly: the one-to-three-signature pool insert.
template <int L>
__global__ __launch_bounds__(WAVE) void k_sig_aggregate_g(PipelineBuffers b, const uint32_t* group_first,
                                                          uint32_t n_groups, uint32_t* agg, int8_t* agg_status,
                                                          uint32_t* first_bad) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x, t = q % L;
  const uint32_t g = q / L;
  const bool on = g < n_groups;  // whole groups: L divides WAVE, so a group never straddles a wave
  const uint32_t first = on ? group_first[g] : 0, last = on ? group_first[g + 1] : 0;
  g2j acc = jac_infinity<fp2>();
  uint32_t my_err_k = 0xffffffffu;
  int my_err = 0;
  sig_agg_strided(b, first, last, t, L, acc, my_err_k, my_err);
  seg_butterfly<fp2, L>(acc, my_err_k, my_err);
  if (on && t == 0) {
    agg_status[g] = (int8_t)my_err;
    first_bad[g] = my_err_k;
    st_g2j(agg, n_groups, g, acc);
  }
}

// Signature.toBytes() of group g's sum into out[out_len * g]: 96-byte compressed or 192-byte uncompressed, the
// identity encoding for a sum equal to the identity, zeros when the group has no sum to show (!have).  One Fp2
// inversion, the cost model of k_pk_serialize.
BLS_INL void sig_agg_encode(const uint32_t* agg, uint32_t n_groups, uint32_t g, bool have, uint8_t* out,
                            uint32_t out_len) {
  uint8_t buf[192];
  for (int k = 0; k < 192; k++) buf[k] = 0;
  if (have) {
    g2a a;
    if (!jac_to_aff(ld_g2j(agg, n_groups, g), a)) {
      buf[0] = out_len == 96 ? 0xc0 : 0x40;
    } else if (out_len == 96) {
      g2a_compress(a, buf);
    } else {
      g2a_to_be192(a, buf);
    }
  }
  uint8_t* o = out + (size_t)g * out_len;
  for (uint32_t k = 0; k < out_len; k++) o[k] = buf[k];
}

// Every group's sum, one lane per group: zeros for a rejected or empty group.  agg_status[g] holds the group's first
// signature error and leaves as the group's status (EMPTY_AGGREGATE for a group with no signatures).
__global__ __launch_bounds__(WAVE) void k_sig_agg_serialize(const uint32_t* group_first, uint32_t n_groups,
                                                            const uint32_t* agg, int8_t* agg_status, uint8_t* out,
                                                            uint32_t out_len) {
  const uint32_t g = blockIdx.x * WAVE + threadIdx.x;
  if (g >= n_groups) return;
  const int st = group_first[g + 1] == group_first[g] ? BLS_EMPTY_AGGREGATE : agg_status[g];
  sig_agg_encode(agg, n_groups, g, st == BLS_OK, out, out_len);
  agg_status[g] = (int8_t)st;
}

// ---- blsgpu_verify_same_message_agg: each group's sum over the sets that verified ------------------
// The same launch forms over a mask instead of the decode status: set_result as the retry phase left it, and the
// caller's include bytes (nullable).  agg (W_G2J SoA, stride n_groups) = the sum, count[g] = the sets summed.
__global__ __launch_bounds__(WAVE) void k_same_agg(const uint32_t* sig_aff, uint32_t n_sets, const int8_t* set_result,
                                                   const uint8_t* include, const uint32_t* group_first,
                                                   uint32_t n_groups, uint32_t* agg, uint32_t* count) {
  __shared__ uint32_t red[SEG_SLOTS * W_G2J];
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t first = group_first[g], last = group_first[g + 1];
  g2j acc = jac_infinity<fp2>();
  uint32_t c = 0;
  same_agg_strided(sig_aff, n_sets, set_result, include, first, last, lane, WAVE, acc, c);
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) c += (uint32_t)__shfl_xor((int)c, m);
  if (last - first > 1) seg_wave_tree(acc, red, lane);  // (uniform per workgroup)
  if (lane == 0) {
    st_g2j(agg, n_groups, g, acc);
    count[g] = c;
  }
}

template <int L>
__global__ __launch_bounds__(WAVE) void k_same_agg_g(const uint32_t* sig_aff, uint32_t n_sets, const int8_t* set_result,
                                                     const uint8_t* include, const uint32_t* group_first,
                                                     uint32_t n_groups, uint32_t* agg, uint32_t* count) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x, t = q % L;
  const uint32_t g = q / L;
  const bool on = g < n_groups;  // whole groups: L divides WAVE, so a group never straddles a wave
  const uint32_t first = on ? group_first[g] : 0, last = on ? group_first[g + 1] : 0;
  g2j acc = jac_infinity<fp2>();
  uint32_t c = 0;
  same_agg_strided(sig_aff, n_sets, set_result, include, first, last, t, L, acc, c);
#pragma unroll
  for (int m = L / 2; m >= 1; m >>= 1) c += (uint32_t)__shfl_xor((int)c, m);
  uint32_t no_err_k = 0xffffffffu;  // (the butterfly also carries a first error: there is none here)
  int no_err = 0;
  seg_butterfly<fp2, L>(acc, no_err_k, no_err);
  if (on && t == 0) {
    st_g2j(agg, n_groups, g, acc);
    count[g] = c;
  }
}

// One lane per group: zeros for a group that summed nothing, the identity encoding for a sum equal to the identity.
__global__ __launch_bounds__(WAVE) void k_same_agg_serialize(uint32_t n_groups, const uint32_t* agg,
                                                             const uint32_t* count, uint8_t* out, uint32_t out_len) {
  const uint32_t g = blockIdx.x * WAVE + threadIdx.x;
  if (g >= n_groups) return;
  sig_agg_encode(agg, n_groups, g, count[g] != 0, out, out_len);
}

void launch_sig_aggregate(const PipelineBuffers& b, const uint32_t* group_first, uint32_t n_groups, uint32_t n_sigs,
                          uint32_t* agg, int8_t* agg_status, uint32_t* first_bad, hipStream_t s) {
  if (!n_groups) return;
  const uint32_t L = sig_agg_lanes(n_groups, n_sigs);
  const dim3 grid((uint32_t)(((uint64_t)n_groups * L + WAVE - 1) / WAVE));
#define SIGAGG_G(l) \
  hipLaunchKernelGGL(k_sig_aggregate_g<l>, grid, dim3(WAVE), 0, s, b, group_first, n_groups, agg, agg_status, first_bad)
  switch (L) {
    case 64:
      hipLaunchKernelGGL(k_sig_aggregate, dim3(n_groups), dim3(WAVE), 0, s, b, group_first, n_groups, agg, agg_status,
                         first_bad);
      break;
    case 32: SIGAGG_G(32); break;
    case 16: SIGAGG_G(16); break;
    case 8: SIGAGG_G(8); break;
    default: SIGAGG_G(1); break;
  }
#undef SIGAGG_G
}
void launch_sig_agg_serialize(const uint32_t* group_first, uint32_t n_groups, const uint32_t* agg, int8_t* agg_status,
                              uint8_t* out, uint32_t out_len, hipStream_t s) {
  if (n_groups)
    hipLaunchKernelGGL(k_sig_agg_serialize, dim3((n_groups + WAVE - 1) / WAVE), dim3(WAVE), 0, s, group_first,
                       n_groups, agg, agg_status, out, out_len);
}

void launch_same_agg(const uint32_t* sig_aff, uint32_t n_sets, const int8_t* set_result, const uint8_t* include,
                     const uint32_t* group_first, uint32_t n_groups, uint32_t* agg, uint32_t* count, uint8_t* out,
                     uint32_t out_len, hipStream_t s) {
  if (!n_groups) return;
  const uint32_t L = sig_agg_lanes(n_groups, n_sets);
  const dim3 grid((uint32_t)(((uint64_t)n_groups * L + WAVE - 1) / WAVE));
#define SAMEAGG_G(l)                                                                                            \
  hipLaunchKernelGGL(k_same_agg_g<l>, grid, dim3(WAVE), 0, s, sig_aff, n_sets, set_result, include, group_first, \
                     n_groups, agg, count)
  switch (L) {
    case 64:
      hipLaunchKernelGGL(k_same_agg, dim3(n_groups), dim3(WAVE), 0, s, sig_aff, n_sets, set_result, include,
                         group_first, n_groups, agg, count);
      break;
    case 32: SAMEAGG_G(32); break;
    case 16: SAMEAGG_G(16); break;
    case 8: SAMEAGG_G(8); break;
    default: SAMEAGG_G(1); break;
  }
#undef SAMEAGG_G
  hipLaunchKernelGGL(k_same_agg_serialize, dim3((n_groups + WAVE - 1) / WAVE), dim3(WAVE), 0, s, n_groups, agg, count,
                     out, out_len);
}
