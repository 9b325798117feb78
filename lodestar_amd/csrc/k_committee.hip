// The committee store's sums and blsgpu_aggregate_pubkeys_bits: a set's aggregated key read from its
// committees' participation bits.  A nearly full committee is taken by complement -- its stored sum minus the absent
// keys -- so a set of a 512-member committee with 5 % absent gathers ~27 table rows instead of ~486.
#include "committee_bits.hpp"
#include "seg_sum.hpp"

static_assert(COMMITTEE_SUM_WORDS == W_CSUM && W_CSUM == W_PKTAB, "a stored sum is shaped like a table row");

// A row of the pubkey table or of the stored sums (both W_PKTAB words, eight 16-byte loads): the affine point, and the
// row's first pad word (0 in a table row; COMMITTEE_SUM_IS_IDENTITY in the row of a sum equal to the identity).
__device__ __forceinline__ uint32_t ld_row(const uint32_t* row, g1a& r) {
  const uint4* q = reinterpret_cast<const uint4*>(row);
  uint32_t w[W_PKTAB];
#pragma unroll
  for (int k = 0; k < W_PKTAB / 4; k++) {
    const uint4 v = q[k];
    w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
  }
#pragma unroll
  for (int l = 0; l < BLS_NL; l++) r.x.l[l] = w[l], r.y.l[l] = w[BLS_NL + l];
  return w[2 * BLS_NL];
}
// the sum of a committee as its stored row: affine, or the flag and zeros for the identity
__device__ __forceinline__ void st_csum(uint32_t* sums, uint32_t c, const g1j& p) {
  g1a a;
  const bool finite = jac_to_aff(p, a);
  uint32_t w[W_CSUM];
#pragma unroll
  for (int l = 0; l < BLS_NL; l++) w[l] = finite ? a.x.l[l] : 0, w[BLS_NL + l] = finite ? a.y.l[l] : 0;
  w[2 * BLS_NL] = finite ? 0 : COMMITTEE_SUM_IS_IDENTITY;
  w[2 * BLS_NL + 1] = 0, w[2 * BLS_NL + 2] = 0, w[2 * BLS_NL + 3] = 0;
  uint4* q = reinterpret_cast<uint4*>(sums + (size_t)c * W_CSUM);
#pragma unroll
  for (int k = 0; k < W_CSUM / 4; k++) q[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// Committee sums at upload, L lanes per committee (64 / L committees per wave): strided partial sums of the members'
// keys, then the in-register butterfly of seg_sum.hpp.  The runtime refuses a member beyond the table before launching;
// the kernel's own guard skips one.
template <int L>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_committee_sums(CommitteeStore st,
                                                                                                  uint32_t c0,
                                                                                                  uint32_t n) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x, t = q % L, ci = q / L;
  const bool on = ci < n;  // whole groups: a group never straddles a wave (L divides WAVE)
  const uint32_t c = c0 + (on ? ci : 0);
  const uint32_t first = on ? st.first[c] : 0, last = on ? st.first[c + 1] : 0;
  g1j acc = jac_infinity<fp>();
  for (uint32_t k = first + t; k < last; k += L) {
    const uint32_t idx = st.members[k];
    if (idx < st.pk_table_n) acc = jac_add_aff(acc, ld_pktab(st.pk_table, idx));
  }
  uint32_t err_k = 0xffffffffu;
  int err = 0;
  seg_butterfly<fp, L>(acc, err_k, err);
  if (on && t == 0) st_csum(st.sums, c, acc);
}

// The bits call, L lanes per set: committee_bits_lane_sum (committee_bits.hpp) per lane, the butterfly, and lane 0
// stores the set's sum where k_pk_serialize reads it.
template <int L>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_pk_bits(CommitteeStore st,
                                                                                           CommitteeBits a) {
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x, t = q % L, si = q / L;
  const bool on = si < a.n_sets;
  const uint32_t set = on ? si : 0;
  CommitteeBitsSet cs;
  const uint32_t s0 = a.set_seg_first[set], b0 = a.set_bits_first[set];
  cs.seg_desc = a.seg_desc + s0;
  cs.n_segs = on ? a.set_seg_first[set + 1] - s0 : 0;
  cs.bits = a.bits + b0;
  cs.n_bytes = a.set_bits_first[set + 1] - b0;
  cs.committee_first = st.first;
  cs.members = st.members;
  g1j acc = committee_bits_lane_sum(cs, t, L, [&](bool stored, uint32_t i, g1a& q) {
    return ld_row((stored ? st.sums : st.pk_table) + (size_t)i * W_PKTAB, q) != COMMITTEE_SUM_IS_IDENTITY;
  });
  uint32_t err_k = 0xffffffffu;
  int err = 0;
  seg_butterfly<fp, L>(acc, err_k, err);
  if (on && t == 0) {
    a.status[2 * a.n_sets + set] = 0;
    st_g1j(a.pk_jac, a.n_sets, set, acc);
  }
}

void launch_committee_sums(const CommitteeStore& st, uint32_t c0, uint32_t n, hipStream_t s) {
  if (!n) return;
  const uint32_t lanes = 1024 * WAVE;
  const uint32_t L = (uint64_t)n * 64 <= lanes ? 64 : (uint64_t)n * 32 <= 2 * lanes ? 32 : (uint64_t)n * 16 <= 2 * lanes ? 16 : 8;
  const dim3 grid((uint32_t)(((uint64_t)n * L + WAVE - 1) / WAVE));
  switch (L) {
    case 64: hipLaunchKernelGGL(k_committee_sums<64>, grid, dim3(WAVE), 0, s, st, c0, n); break;
    case 32: hipLaunchKernelGGL(k_committee_sums<32>, grid, dim3(WAVE), 0, s, st, c0, n); break;
    case 16: hipLaunchKernelGGL(k_committee_sums<16>, grid, dim3(WAVE), 0, s, st, c0, n); break;
    default: hipLaunchKernelGGL(k_committee_sums<8>, grid, dim3(WAVE), 0, s, st, c0, n); break;
  }
}

void launch_pk_bits(const CommitteeStore& st, const CommitteeBits& a, uint32_t L, hipStream_t s) {
  if (!a.n_sets) return;
  const dim3 grid((uint32_t)(((uint64_t)a.n_sets * L + WAVE - 1) / WAVE));
  switch (L) {
    case 64: hipLaunchKernelGGL(k_pk_bits<64>, grid, dim3(WAVE), 0, s, st, a); break;
    case 32: hipLaunchKernelGGL(k_pk_bits<32>, grid, dim3(WAVE), 0, s, st, a); break;
    case 16: hipLaunchKernelGGL(k_pk_bits<16>, grid, dim3(WAVE), 0, s, st, a); break;
    default: hipLaunchKernelGGL(k_pk_bits<8>, grid, dim3(WAVE), 0, s, st, a); break;
  }
}
