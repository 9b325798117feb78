// Launchers for the verification-pipeline kernels (k_*.hip), called by pipeline.cpp and helpers.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "awr_parts.hpp"

// Word counts of the SoA records (element i, word w at base[w * stride + i])
#define W_FP 14
#define W_G1A (2 * W_FP)
#define W_G1J (3 * W_FP)
#define W_G2A (4 * W_FP)
#define W_G2J (6 * W_FP)
#define W_FP12 (12 * W_FP)
// Pubkey table entries: AoS, 32 words (x limbs, y limbs, pad) = one 128-byte line per key
#define W_PKTAB 32
// Miller-loop line coefficients per message: 68 steps x (l0, c1, c4)
#define MILLER_STEPS 68
#define W_LINE (3 * 2 * W_FP)

// set flags (uint8 per set)
#define SF_SIG_INF 1u
// per-message flags
#define MF_H_INF 1u

struct PipelineBuffers {
  uint32_t n;  // SoA stride of per-set arrays (>= n_sets)
  // ---- inputs
  const uint8_t* sigs;
  const uint32_t* sig_len;
  uint32_t sig_stride;
  // public keys: pk_bytes && !set_pk_first: one 96-B key per set; pk_bytes && set_pk_first: set i aggregates
  // keys [set_pk_first[i], set_pk_first[i+1]) of pk_bytes; !pk_bytes: table entries pk_index[...]
  const uint8_t* pk_bytes;
  const uint32_t* set_pk_first;
  const uint32_t* pk_index;
  const uint32_t* pk_table;  // AoS W_PKTAB words per key
  uint32_t pk_table_n;
  // aggregation list: k_pk_aggregate runs one wave per set agg_sets[0 .. n_agg) (all sets when null); with
  // pk_direct1, a set of exactly one key skips it and k_pk_finish reads / decodes that key itself
  const uint32_t* agg_sets;
  uint32_t n_agg;
  uint32_t pk_direct1;
  const uint64_t* scalars;  // batch scalar words (k_common.hpp jac_mul_scalar_word), 0 = r = 1
  uint32_t* scal_tab;       // signed-window tables: 8 x W_G2J words per set (SoA, stride n)
  const uint32_t* job_first_set;  // [n_jobs + 1], shard-relative
  uint32_t n_jobs;
  // messages, deduplicated per call: set i signs umsgs[msg_idx[i]]
  const uint8_t* umsgs;
  const uint32_t* msg_idx;
  uint32_t n_umsg;
  uint32_t nm;  // SoA stride of per-message arrays (>= n_umsg)
  // pairing units (same-message merging): unit u = the included sets unit_sets[unit_set_first[u] ..
  // unit_set_first[u+1]) of one batch group, all signing umsgs[unit_msg[u]]; P_u = sum r_i pk_i
  uint32_t n_units;
  const uint32_t* unit_set_first;
  const uint32_t* unit_sets;
  const uint32_t* unit_msg;
  // ---- intermediates
  uint32_t* sig_aff;  // W_G2A, per set
  uint32_t* h_aff;    // W_G2A, per message
  uint32_t* h_jac;    // W_G2J, per message: H(m) before the batched affine conversion (k_inv.hip)
  uint32_t* h_norm;   // W_FP, per message: N(d) of the hash prep, then N(z) of h_jac
  uint32_t* h_prep;   // 7 x W_FP2, per message: the hash_to_G2 state across its batched inversion (k_hash.hip)
  uint32_t* h_q;      // 2 x W_G2J, per message: the two mapped points iso3(SSWU(u_j)) (stride 2 nm, k_hash.hip)
  uint32_t* inv_buf;     // W_FP, per max(set, message): batch inversion output of the message branch (k_inv.hip)
  uint32_t* inv_buf_pk;  // W_FP, per set: the pubkey branch's (the two branches run on different streams)
  uint32_t* pk_jac;   // W_G1J, per set (aggregate)
  uint32_t* pk_aff;   // W_G1A, per set (r * pk, affine)
  uint32_t* rsig;     // W_G2J, per set
  uint32_t* unit_p;   // W_G1A, per unit (stride n)
  // Miller chunks: chunk c multiplies the Miller values of items chunk_items[chunk_first[c] ..
  // chunk_first[c+1]) (sets, or units) into ONE accumulator with shared squarings -> f_chunk[c]
  uint32_t n_chunks;
  const uint32_t* chunk_first;
  const uint32_t* chunk_items;
  uint32_t* f_chunk;  // W_FP12, per chunk (stride n)
  uint32_t* lines;    // Miller lines, per message: MILLER_STEPS x W_LINE words, step-major SoA (stride nm)
  uint8_t* flags;     // [n]: sig flags
  uint8_t* mflags;    // [nm]: message flags
  uint8_t* unit_ok;   // [n]: unit has a finite P_u
  int8_t* status;     // [3n]: signature status, pubkey status, aggregation status
  int8_t* job_err;    // [n_jobs]: first pubkey/signature error of the job (0 = clean)
  uint8_t* include;   // [n]: set belongs to a clean job (enters the batch equation)
};

// coop: small and mid-size runs -- the [|z|] chains (subgroup check, cofactor clearing) as cooperative 16-lane
// doublings (g2_coop.hpp), for latency; exclusive: each cooperative workgroup takes a CU to itself (small runs only:
// beyond ~one workgroup per CU the padding serializes the launch)
// (decoded: recorded after the decode, before the small-run subgroup checks)
// (subgroup false: Signature.fromBytes(.., validate = false) -- the decode alone, no subgroup-check kernel)
void launch_sig_decode(const PipelineBuffers& b, uint32_t n_sets, hipStream_t s, bool coop = false,
                       hipEvent_t decoded = nullptr, bool exclusive = true, bool subgroup = true);
// spec[i] = the signature of set i decoded (the speculative MSM's include mask)
void launch_spec_mask(const PipelineBuffers& b, uint32_t n_sets, uint8_t* spec, hipStream_t s);
void launch_hash_prep(const PipelineBuffers& b, hipStream_t s);
void launch_hash_map(const PipelineBuffers& b, const uint32_t* inv, hipStream_t s);
void launch_hash_to_g2(const PipelineBuffers& b, hipStream_t s, bool coop = false,
                       bool exclusive = true);  // over the unique messages
void launch_pk_aggregate(const PipelineBuffers& b, uint32_t n_sets, hipStream_t s);
void launch_pk_finish(const PipelineBuffers& b, uint32_t n_sets, hipStream_t s);
// batched affine conversions (Montgomery's simultaneous inversion, k_inv.hip): r_i pk_i -> pk_aff, H(m) -> h_aff
void launch_batch_inv(const uint32_t* src, uint32_t src_stride, int w0, uint32_t* dst, uint32_t n, hipStream_t s);
void launch_pk_affine(const PipelineBuffers& b, uint32_t n_sets, hipStream_t s);
void launch_h_affine(const PipelineBuffers& b, hipStream_t s);
// r_i sig_i -> b.rsig for the sets list[0 .. n) (all sets when list is null), G2 window tables in b.scal_tab
void launch_sig_scale(const PipelineBuffers& b, uint32_t n_sets, hipStream_t s, const uint32_t* list = nullptr);
// S_r = sum r_i sig_i over the included sets of each range, as a bucket MSM (k_msm.hip, msm.hpp).  Range r is the
// slices [range_slices[r], range_slices[r+1]); slice s is the sets [slices[2s], slices[2s+1]) (<= MSM_SLICE of
// them).  B: MSM_BUCKET_WORDS words per slice, W: MSM_WINDOW_WORDS per range; S: W_G2J SoA, stride n_ranges.
#ifndef MSM_SLICE
#define MSM_SLICE 256
#endif
#define MSM_BUCKET_WORDS (128 * W_G2J)
#define MSM_WINDOW_WORDS (16 * W_G2J)
// lane_tail: the Horner passes on two lanes per range instead of cooperative 16-lane groups (merged runs)
// tree_slices: the most slices of any range; > 2 sums each range's slices by a pairwise tree of launches before the
// window pass (latency-bound runs with short slices), else the window lanes sum them serially
void launch_sig_msm(const PipelineBuffers& b, const uint32_t* slices, uint32_t n_slices, const uint32_t* range_slices,
                    uint32_t n_ranges, uint32_t* B, uint32_t* W, uint32_t* S, hipStream_t s, bool lane_tail = false,
                    uint32_t tree_slices = 0);
// per-job error status and the per-set include mask of the batch equation
void launch_job_mask(const PipelineBuffers& b, hipStream_t s);
// P_u = sum over the unit's included sets of r_i pk_i (affine)
void launch_unit_aggregate(const PipelineBuffers& b, hipStream_t s);
// Miller lines of every unique message
void launch_miller_lines(const PipelineBuffers& b, hipStream_t s);
// the same on two lanes per message (k_miller_lines2: mid-size runs, latency)
void launch_miller_lines2(const PipelineBuffers& b, hipStream_t s);
// Miller values of the chunks (items are units when `units`, else sets): f_chunk[c] = prod over the chunk's
// active items of MillerLoop(P_item, H(m_item)), one lane per chunk, the Fp12 squarings shared
void launch_miller_accx(const PipelineBuffers& b, bool units, hipStream_t s);
// Step segments of the one-lane accumulation (miller_plan.hpp): segment j covers steps [first[j], first[j + 1]) and
// holds dbl[j] doubling steps.  With n > 1 lane (chunk c, segment j) writes the value of its own steps to slot
// j * n_chunks + c of f_chunk (n * n_chunks <= the stride); launch_group_fold puts the groups' segment heads together.
#define MILLER_MAX_SEGS 8
struct MillerSegs {
  uint32_t n;
  uint32_t first[MILLER_MAX_SEGS + 1];
  uint32_t dbl[MILLER_MAX_SEGS];
};
void launch_miller_acc(const PipelineBuffers& b, bool units, hipStream_t s, const MillerSegs* segs = nullptr);
// the same for chunks of ONE item each, two lanes per pairing (k_miller.hip k_miller_acc2: mid-size runs, latency)
void launch_miller_acc2(const PipelineBuffers& b, bool units, hipStream_t s);
// the same on SIX lanes per chunk, one w-basis Fp2 coefficient of f per lane (k_miller_acc6: 2k-16k-pairing runs)
void launch_miller_acc6(const PipelineBuffers& b, bool units, hipStream_t s);
// the same for chunks of ONE item each, as one cooperative 128-lane workgroup per pairing (lines on the fly; small
// runs, for latency)
// (exclusive: each workgroup takes a CU to itself -- k_common.hpp exclusive_cu_lds -- for latency-bound small runs;
// BLSGPU_EXCLUSIVE_SMALL=0 turns it off everywhere)
#ifndef BLSGPU_EXCLUSIVE_SMALL
#define BLSGPU_EXCLUSIVE_SMALL 1
#endif
void launch_miller_coop(const PipelineBuffers& b, bool units, hipStream_t s, bool exclusive = false);
// Batch groups: group g covers Miller chunks [f_ranges[2g], f_ranges[2g+1]).
// reduce: F_g = prod f_chunk over chunks [f_ranges[2g], f_ranges[2g+1]) (W_FP12 SoA, stride n_groups); S_g comes
// from launch_sig_msm (or, in the fallback, from per-set scalings summed by launch_group_reduce_lane)
void launch_group_reduce(const PipelineBuffers& b, const uint32_t* f_ranges, uint32_t n_groups, uint32_t* F,
                         hipStream_t s);
// the same F_g as a product tree (k_group.hip): runs[0 .. n_runs) (first, end) chunk runs multiplied lane-serially
// into their first chunk, then the pair levels (pairs up to level_end[0], then up to level_end[1], ...: f[dst] *=
// f[src], one cooperative workgroup per pair), then F_g = f[first chunk of g]
// (segs with n > 1: the tree was planned per (segment, group) over the segment-major slots and f_ranges holds
// segs->n * n_groups ranges, range j * n_groups + g = group g's slots of segment j; their heads go to H (W_FP12 SoA,
// stride segs->n * n_groups) and F_g is their Horner fold, k_group.hip k_f_fold)
void launch_group_tree(const PipelineBuffers& b, const uint32_t* f_ranges, uint32_t n_groups, const uint32_t* runs,
                       uint32_t n_runs, const uint32_t* pairs, const std::vector<uint32_t>& level_end, uint32_t* F,
                       hipStream_t s, const MillerSegs* segs = nullptr, uint32_t* H = nullptr);
// check: ok_g = FinalExp(F_g * MillerLoop(-g1, S_g)) == 1
// (sel: check only the entries sel[0 .. n_sel), verdict q -> ok[q])
// (G: MillerLoop(-g1, S_g) precomputed by launch_group_sig_miller, W_FP12 SoA stride n_groups; null = computed here)
// (lane: one lane per check instead of a cooperative workgroup -- the fallback's large launches under load; G null)
void launch_group_check(const uint32_t* S, const uint32_t* F, uint32_t n_groups, uint8_t* ok, hipStream_t s,
                        const uint32_t* sel = nullptr, uint32_t n_sel = 0, const uint32_t* G = nullptr,
                        bool exclusive = false, bool lane = false);
// six lanes per check (k_group_check6, gt6.hpp): ok = FinalExp(F * G) == 1 with G = MillerLoop(-g1, S) precomputed
// (launch_group_sig_miller; sel: check only entries sel[0 .. n_sel), verdict q -> ok[q])
void launch_group_check6(const uint32_t* F, const uint32_t* G, uint32_t n_groups, uint8_t* ok, hipStream_t s,
                         const uint32_t* sel = nullptr, uint32_t n_sel = 0);
// the whole check on six lanes: S's Miller lines one lane per entry (k_check_lines, into `lines`: n_groups x 68 x W_LINE
// words; flags: n_groups bytes), then MillerLoop(-g1, S), F * G and the final exponentiation on six lanes per check
void launch_check6_miller(const uint32_t* S, const uint32_t* F, uint32_t n_groups, uint8_t* ok, hipStream_t s,
                          const uint32_t* sel, uint32_t n_sel, uint32_t* lines, uint8_t* flags);
// G[sel[q]] = MillerLoop(-g1, S[sel[q]]) on one lane per entry (all n_groups entries when sel is null)
void launch_group_sig_miller_sel(const uint32_t* S, uint32_t n_groups, const uint32_t* sel, uint32_t n_sel, uint32_t* G,
                                 hipStream_t s);
// lane: one lane per group (pairing.hpp miller_loop) instead of a three-wave cooperative workgroup (merged runs)
void launch_group_sig_miller(const uint32_t* S, uint32_t n_groups, uint32_t* G, hipStream_t s, bool exclusive = false,
                             bool lane = false);
// lane-per-item forms (one lane per range / sub-group) for the fallback's many tiny ranges
void launch_copy_words(uint32_t* dst, const uint32_t* src, size_t n, hipStream_t s);
void launch_group_reduce_lane(const PipelineBuffers& b, const uint32_t* set_ranges, const uint32_t* f_ranges,
                              uint32_t n_groups, uint32_t* S, uint32_t* F, hipStream_t s);
void launch_range_combine_lane(const uint32_t* S_in, const uint32_t* F_in, uint32_t n_in, const uint32_t* ranges,
                               uint32_t n_out, uint32_t* S_out, uint32_t* F_out, hipStream_t s);
// fallback sub-groups: S_out[r] = sum, F_out[r] = prod of the per-job entries ranges[2r] .. ranges[2r+1]
void launch_range_combine(const uint32_t* S_in, const uint32_t* F_in, uint32_t n_in, const uint32_t* ranges,
                          uint32_t n_out, uint32_t* S_out, uint32_t* F_out, hipStream_t s);
// pubkey table upload: decode 96-byte affine encodings into table entries, per-entry status
void launch_pk_table_fill(const uint8_t* pk96, uint32_t n, uint32_t* table_dst, int8_t* status, hipStream_t s);
// the same from 48-byte compressed encodings (pk48 16-byte aligned): a row and a status per key, an all-zero row for a
// rejected one; validate adds the G1 subgroup check (KeyValidate) to the decompression
void launch_pk_table_fill48(const uint8_t* pk48, uint32_t n, uint32_t* table_dst, int8_t* status, bool validate,
                            hipStream_t s);
// table rows [first, first + n) -> out[out_len k] (16-byte aligned), out_len 96 (big-endian x || y) or 48 (compressed)
void launch_pk_table_read(const uint32_t* table, uint32_t first, uint32_t n, uint8_t* out, uint32_t out_len,
                          hipStream_t s);
// serialize the per-set aggregate (pk_jac) to 96-byte uncompressed or 48-byte compressed encodings
void launch_pk_serialize(const PipelineBuffers& b, uint32_t n_sets, uint8_t* out, uint32_t out_len, hipStream_t s);
// The committee store (k_committee.hip): committee c is members[first[c] .. first[c + 1]) (table
// indices) and keeps the sum of its members' keys in sums[W_CSUM c ..], a row shaped like a table row: affine x | y and
// four pad words, the first of them 1 (x, y zero) when the sum is the identity.
#define W_CSUM 32
struct CommitteeStore {
  const uint32_t* first;
  const uint32_t* members;
  uint32_t* sums;
  const uint32_t* pk_table;
  uint32_t pk_table_n;
};
// sums of committees [c0, c0 + n): the segmented G1 sum on the lanes per committee launch_pk_aggregate would take
void launch_committee_sums(const CommitteeStore& st, uint32_t c0, uint32_t n, hipStream_t s);
// blsgpu_aggregate_pubkeys_bits: every set's aggregated key from its participation bits, on L lanes per set (64, 32,
// 16 or 8: committee_plan.hpp lanes), into pk_jac (W_G1J SoA, stride n_sets), with status[2 n_sets + set] = 0.  Set s
// owns segments seg_desc[set_seg_first[s] .. set_seg_first[s + 1]) and the bit string at bits + set_bits_first[s].
struct CommitteeBits {
  uint32_t n_sets;
  const uint32_t* set_seg_first;
  const uint32_t* seg_desc;
  const uint32_t* set_bits_first;
  const uint8_t* bits;
  uint32_t* pk_jac;
  int8_t* status;
};
void launch_pk_bits(const CommitteeStore& st, const CommitteeBits& a, uint32_t L, hipStream_t s);
// KeyValidate of untrusted 48/96-byte pubkeys (decode + G1 subgroup check) -> 96-byte uncompressed
void launch_key_validate(const uint8_t* pks, uint32_t n, uint32_t pk_len, uint32_t stride, uint8_t* out96,
                         int8_t* status, hipStream_t s);
// Signature.aggregate over groups of decoded signatures (k_sigagg.hip; b fills sig_aff, flags, status and n as
// launch_sig_decode left them): group g sums signatures [group_first[g], group_first[g+1]) into agg (W_G2J SoA,
// stride n_groups), agg_status[g] / first_bad[g] = the code and index of its first rejected signature (0 / 0xffffffff).
// Lanes per group, by group count and mean group size: a wave per group (64, LDS tree) while that leaves SIMDs idle
// (<= 1,024 groups), then the fewest lanes of 32, 16, 8 (shuffle butterfly) that still give every SIMD a wave
// (n_groups * L >= 65,536 lanes), then one lane per group; never more lanes than the next form above the mean group
// size, and one lane for groups of up to three signatures (the pool insert: a butterfly level costs a full Jacobian
// addition, more than the serial mixed additions it saves).  Non-increasing in n_groups for a given n_sigs.
inline uint32_t sig_agg_lanes(uint32_t n_groups, uint32_t n_sigs) {
  if (n_groups == 0) return 1;
  const uint64_t n = n_groups, lanes = 1024 * 64;
  const uint32_t by_count = n * 64 <= lanes ? 64 : n * 32 <= 2 * lanes ? 32 : n * 16 <= 2 * lanes ? 16
                            : n * 8 <= 2 * lanes ? 8 : 1;
  const uint64_t mean = ((uint64_t)n_sigs + n - 1) / n;
  const uint32_t by_size = mean <= 3 ? 1 : mean <= 8 ? 8 : mean <= 16 ? 16 : mean <= 32 ? 32 : 64;
  return by_count < by_size ? by_count : by_size;
}
void launch_sig_aggregate(const PipelineBuffers& b, const uint32_t* group_first, uint32_t n_groups, uint32_t n_sigs,
                          uint32_t* agg, int8_t* agg_status, uint32_t* first_bad, hipStream_t s);
// Signature.toBytes() of the sums: out[out_len * g], out_len 96 (compressed) or 192; zeros for a rejected or empty
// group; agg_status[g] becomes the group's status (EMPTY_AGGREGATE for an empty group)
void launch_sig_agg_serialize(const uint32_t* group_first, uint32_t n_groups, const uint32_t* agg, int8_t* agg_status,
                              uint8_t* out, uint32_t out_len, hipStream_t s);
// blsgpu_verify_same_message_agg (k_sigagg.hip): group g's sum over its sets k with set_result[k] == 1 and (include
// null or include[k]), from sig_aff (stride n_sets) as launch_sig_decode left it, on the lanes of
// sig_agg_lanes(n_groups, n_sets); agg (W_G2J SoA, stride n_groups), count[g] = the sets summed, out[out_len * g] = Signature.toBytes() of the
// sum (zeros when count[g] is 0)
void launch_same_agg(const uint32_t* sig_aff, uint32_t n_sets, const int8_t* set_result, const uint8_t* include,
                     const uint32_t* group_first, uint32_t n_groups, uint32_t* agg, uint32_t* count, uint8_t* out,
                     uint32_t out_len, hipStream_t s);
// aggregateWithRandomness over groups of sets (k_awr.hip): group g owns sets [group_first[g], group_first[g+1]); per
// group P = sum r_k pk_k (G1) and S = sum r_k sig_k (G2), r_k the batch scalar of words[k] (never 0).
struct AwrBuffers {
  uint32_t n;         // sets; SoA stride of sig_aff
  uint32_t n_groups;  // SoA stride of sum_pk / sum_sig
  const uint32_t* group_first;
  const uint64_t* words;
  // trusted keys: pk_bytes[96 k] (uncompressed), or table entry pk_index[k] when pk_bytes is null
  const uint8_t* pk_bytes;
  const uint32_t* pk_index;
  const uint32_t* pk_table;
  uint32_t pk_table_n;
  // signatures as launch_sig_decode left them
  const uint32_t* sig_aff;
  const uint8_t* sig_flags;
  const int8_t* sig_status;
  // window scratch: 9 entries of W_G2J words per launched lane (8 window entries laid out as scal_tab, stride tab_n,
  // and the lane's running sum), shared by the G1 and the G2 kernel
  uint32_t* tab;
  uint32_t tab_n;  // launched lanes: awr_launch_lanes(n_groups, L)
  uint32_t* sum_pk;   // W_G1J per group
  uint32_t* sum_sig;  // W_G2J per group
  uint32_t* err_k;    // [2 n_groups]: lowest rejected set index per group (0xffffffff = none), keys then signatures
  int8_t* err_c;      // [2 n_groups]: its code
};
#define AWR_TAB_WORDS (9 * W_G2J)
// (the lanes per group, awr_lanes, and the cut of large groups into parts are awr_parts.hpp)
uint32_t awr_launch_lanes(uint32_t n_groups, uint32_t L);
// sum_pk / sum_sig and the per-group first errors, on L lanes per group (a.tab_n = awr_launch_lanes(n_groups, L))
void launch_awr_sums(const AwrBuffers& a, uint32_t L, hipStream_t s);
// its two halves on their own: sum_pk and the keys' first errors / sum_sig and the signatures'.  They share nothing
// but a.tab, so two copies of `a` with different window scratch may run on two streams at once.
void launch_awr_sum_pk(const AwrBuffers& a, uint32_t L, hipStream_t s);
void launch_awr_sum_sig(const AwrBuffers& a, uint32_t L, hipStream_t s);
// A split call (awr_parts.hpp): the sums above run over the parts -- `parts` is the call's `a` with group_first = the
// parts' first sets, n_groups = the parts and sum_pk / sum_sig / err_k / err_c part-sized -- and these fold them: group
// g's parts are [group_part[g], group_part[g + 1]); its Jacobian sum and its first error (the lowest set index over
// the parts) go where the unsplit sums leave them, a.sum_pk / a.sum_sig / a.err_k / a.err_c (stride a.n_groups).  The
// fold is a plain segmented sum of the parts on L = awr_parts::fold_lanes(..) lanes per group (64, 32, 16, 8 or 1).
void launch_awr_fold_pk(const AwrBuffers& parts, const AwrBuffers& a, const uint32_t* group_part, uint32_t L,
                        hipStream_t s);
void launch_awr_fold_sig(const AwrBuffers& parts, const AwrBuffers& a, const uint32_t* group_part, uint32_t L,
                         hipStream_t s);
// One-call same-message verification (k_same.hip, blsgpu_verify_same_message).
// per group: pk_aff (W_G1A, stride n_groups) = sum_pk times inv = 1 / z (launch_batch_inv), code = the group's AWR
// status, include = accepted by AWR with a finite P
void launch_same_group_items(const AwrBuffers& a, const uint32_t* inv, uint32_t* pk_aff, uint8_t* include, int8_t* code,
                             hipStream_t s);
// per retried set q = set list[q]: pk_aff (W_G1A) and S (W_G2J, the decoded signature with z = 1), stride n_retry;
// code = its first error (key, then signature), include = no error and a finite signature
void launch_same_retry_items(const AwrBuffers& a, const uint32_t* list, uint32_t n_retry, uint32_t* pk_aff, uint32_t* S,
                             uint8_t* include, int8_t* code, hipStream_t s);
// group_result[g] = 1 / 0 / -EMPTY_AGGREGATE and set_result[k] = 1 for every set of an accepted group, else 0
void launch_same_group_results(const uint32_t* group_first, uint32_t n_groups, uint32_t n_sets, const uint8_t* include,
                               const int8_t* code, const uint8_t* ok, int8_t* set_result, int8_t* group_result,
                               hipStream_t s);
// set_result[list[q]] = -code[q], or include[q] && ok[q]
void launch_same_retry_results(const uint32_t* list, uint32_t n_retry, const uint8_t* include, const int8_t* code,
                               const uint8_t* ok, int8_t* set_result, hipStream_t s);
// BLSGPU_SAME_BLOCK_CHECK: groups per block (the default of option "group_sets", as a constant: helper calls read no
// option; blsgpu_same_message_blocks is the rule)
#ifndef SAME_BLOCK_GROUPS
#define SAME_BLOCK_GROUPS 1024u
#endif
// per block b of SAME_BLOCK_GROUPS groups: S_out (W_G2J, stride n_blocks) = sum S_g (stride n_groups) over its groups
// with include[g], any[b] = whether it had one
void launch_same_block_sum(const uint32_t* S, const uint8_t* include, uint32_t n_groups, uint32_t n_blocks,
                           uint32_t* S_out, uint8_t* any, hipStream_t s);
// F_out (W_FP12, stride n_blocks) = prod F_g (stride n_groups) over the same groups, as a product tree: the first level
// has same_block_tree_width(n_groups) products per block (the least power of two that pairs up a block's groups), each
// level half the one before; levels alternate between T0 (n_blocks * width Fp12) and T1 (half of that), F is not written
uint32_t same_block_tree_width(uint32_t n_groups);
void launch_same_block_prod(const uint32_t* F, const uint8_t* include, uint32_t n_groups, uint32_t n_blocks,
                            uint32_t* T0, uint32_t* T1, uint32_t* F_out, hipStream_t s);
// group_result[g] = -EMPTY_AGGREGATE, or include[g] && any[b] && ok[b] for g's block b; set_result[k] the same 1 / 0
void launch_same_block_results(const uint32_t* group_first, uint32_t n_groups, uint32_t n_sets, const uint8_t* include,
                               const int8_t* code, const uint8_t* any, const uint8_t* ok, int8_t* set_result,
                               int8_t* group_result, hipStream_t s);
// F_out / S_out (stride n_listed) = F / S (stride n_groups) of the groups list[0 .. n_listed)
void launch_same_gather(const uint32_t* F, const uint32_t* S, uint32_t n_groups, const uint32_t* list,
                        uint32_t n_listed, uint32_t* F_out, uint32_t* S_out, hipStream_t s);
// group_result[list[q]] = ok[q], and set_result of every set of a listed group (list ascending)
void launch_same_descent_results(const uint32_t* group_first, uint32_t n_groups, uint32_t n_sets, const uint32_t* list,
                                 uint32_t n_listed, const uint8_t* ok, int8_t* set_result, int8_t* group_result,
                                 hipStream_t s);
// Batched AggregateVerify (k_aggverify.hip, blsgpu_aggregate_verify): job j owns pairs [job_first[j], job_first[j+1])
// and one signature.  Items (stride n_items = n_pairs + n_jobs): pair k is item k, job j's (-g1, signature) item is
// item n_pairs + j.  G2 columns (stride nm = n_umsg + n_jobs): unique message u is column u, job j's signature is
// column n_umsg + j.
struct AvBuffers {
  uint32_t n_pairs, n_jobs, n_items, n_umsg, nm;
  const uint32_t* job_first;
  // keys: pk_bytes[96 k] (trusted uncompressed, or launch_key_validate's output with its status in kv_status), or
  // table entry pk_index[k] when pk_bytes is null
  const uint8_t* pk_bytes;
  const int8_t* kv_status;  // null: the keys are trusted
  const uint32_t* pk_index;
  const uint32_t* pk_table;
  uint32_t pk_table_n;
  const uint32_t* pair_msg;  // [n_pairs]: the pair's unique message
  // the jobs' signatures as launch_sig_decode left them (stride n_jobs)
  const uint32_t* sig_aff;
  const uint8_t* sig_flags;
  const int8_t* sig_status;
  uint32_t* pk_aff;    // W_G1A per item
  uint32_t* msg_idx;   // [n_items]: the item's G2 column
  uint8_t* include;    // [n_items]
  int8_t* pair_code;   // [n_pairs]: the key's error
  uint32_t* h_aff;     // W_G2A per column
  uint8_t* mflags;     // [nm]
  uint8_t* checked;    // [n_jobs]: no error and a finite signature: the job reaches the pairing check
  int8_t* job_code;    // [n_jobs]: EMPTY_AGGREGATE, the lowest-index rejected key's code, else the signature's
  uint32_t* first_bad; // [n_jobs]: that key's pair index, 0xffffffff when no key was rejected
};
// per pair: pk_aff, msg_idx, pair_code
void launch_av_pair_items(const AvBuffers& a, hipStream_t s);
// per job: job_code, first_bad, checked, the signature's G2 column and its flag, the signature item and the include
// bytes of every item of the job (set for a checked job, cleared for every other)
void launch_av_job_items(const AvBuffers& a, hipStream_t s);
// F[j] (W_FP12, stride n_jobs) = prod f_chunk over chunks [f_ranges[2j], f_ranges[2j+1]) on one lane per job (one for
// an empty range); launch_group_reduce is the wave-per-job form
void launch_av_reduce_lane(const uint32_t* f_chunk, uint32_t stride, const uint32_t* f_ranges, uint32_t n_jobs,
                           uint32_t* F, hipStream_t s);
// ok[j] = checked[j] && FinalExp(F[j]) == 1: a cooperative workgroup per job, or (lane) six lanes per job
void launch_av_check(const uint32_t* F, uint32_t n_jobs, const uint8_t* checked, uint8_t* ok, bool lane, hipStream_t s);
// job_result[j] = -code[j], or checked[j] && ok[j]
void launch_av_results(uint32_t n_jobs, const int8_t* code, const uint8_t* checked, const uint8_t* ok,
                       int8_t* job_result, hipStream_t s);
// both sums' toBytes(): out_pk[out_pk_len * g] (48 compressed / 96), out_sig[out_sig_len * g] (96 compressed / 192),
// zeros for a rejected or empty group; status[g] / first_bad[g] = the group's status and its rejected set's index
void launch_awr_serialize(const AwrBuffers& a, uint8_t* out_pk, uint32_t out_pk_len, uint8_t* out_sig,
                          uint32_t out_sig_len, int8_t* status, uint32_t* first_bad, hipStream_t s);
// SSZ signing roots (SigningData / AttestationData hash_tree_root)
void launch_signing_roots(int kind, const uint8_t* in, uint32_t n, uint32_t in_stride, const uint8_t* domain,
                          uint32_t domain_stride, uint8_t* out, hipStream_t s);
// debug ops (blsgpu_debug_op)
void launch_debug_op(int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                     int32_t* status, hipStream_t s);
// the field tower's raw-limb hooks (ops 32..68, tower_debug.hpp): 128-lane workgroups, strides multiples of 4
void launch_debug_tower(int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                        int32_t* status, hipStream_t s);
// the point formulas' raw-limb hooks (ops 69..107, curve_debug.hpp): the same launch shape and stride rule
void launch_debug_curve(int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                        int32_t* status, hipStream_t s);
// the multi-lane engines' raw-limb hooks (ops 108..157, coop_debug.hpp): each engine in its production launch shape
// (an element per lane pair, per six lanes, per 16-lane group, per block); the same stride rule; `status` zeroed by
// the caller (a g2c element flagged off writes nothing)
void launch_debug_coop(int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                       int32_t* status, hipStream_t s);
