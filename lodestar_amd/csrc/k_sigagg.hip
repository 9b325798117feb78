// Signature.aggregate(sigs.map(fromBytes)).toBytes() for many groups at once (blsgpu_aggregate_signatures): the
// segmented G2 sum over the signatures k_sig_decode left in sig_aff (k_sig.hip), and its serialization.  The G2 twin
// of k_pk_aggregate / k_pk_aggregate_g / k_pk_serialize (k_pk.hip).
#include "k_common.hpp"
#include "seg_sum.hpp"

// One lane's share of group [first, last): signatures first + t, first + t + L, ...  A rejected signature (decode or
// subgroup status) is the lane's error when it is the lane's first -- k ascends, so that is the lane's lowest index;
// an identity signature adds nothing.
BLS_INL void sig_agg_strided(const PipelineBuffers& b, uint32_t first, uint32_t last, uint32_t t, uint32_t L, g2j& acc,
                             uint32_t& err_k, int& err) {
#pragma unroll 1
  for (uint32_t k = first + t; k < last; k += L) {
    const int st = b.status[k];
    if (st != BLS_OK) {
      if (err == 0) {
        err = st;
        err_k = k;
      }
      continue;
    }
    if (b.flags[k] & SF_SIG_INF) continue;
    acc = jac_add_aff(acc, ld_g2a(b.sig_aff, b.n, k));
  }
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

// Signature.toBytes() of every group's sum, one lane per group (one Fp2 inversion each, the cost model of
// k_pk_serialize): 96-byte compressed or 192-byte uncompressed; the identity encoding for a sum equal to the
// identity, zeros for a rejected or empty group.  agg_status[g] holds the group's first signature error and leaves as
// the group's status (EMPTY_AGGREGATE for a group with no signatures).
__global__ __launch_bounds__(WAVE) void k_sig_agg_serialize(const uint32_t* group_first, uint32_t n_groups,
                                                            const uint32_t* agg, int8_t* agg_status, uint8_t* out,
                                                            uint32_t out_len) {
  const uint32_t g = blockIdx.x * WAVE + threadIdx.x;
  if (g >= n_groups) return;
  const int st = group_first[g + 1] == group_first[g] ? BLS_EMPTY_AGGREGATE : agg_status[g];
  uint8_t buf[192];
  for (int k = 0; k < 192; k++) buf[k] = 0;
  if (st == BLS_OK) {
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
  agg_status[g] = (int8_t)st;
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
