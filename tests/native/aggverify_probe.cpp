// Host probe of lodestar_amd/csrc/aggverify_plan.hpp and helper_layout.hpp's hl::AggVerify
// (tests/test_aggregate_verify_host.py): the two headers alone, no HIP.
#include "../../lodestar_amd/csrc/aggverify_plan.hpp"
#include "../../lodestar_amd/csrc/helper_layout.hpp"

namespace avp = aggverify_plan;
namespace hl = helper_layout;

extern "C" {

uint32_t probe_form(uint32_t n_items, int lane_flag) { return avp::form(n_items, lane_flag != 0); }
uint32_t probe_chunk_items(const uint32_t* job_first, uint32_t n_jobs, uint32_t form, int lane_flag) {
  return avp::chunk_items_for(job_first, n_jobs, form, lane_flag != 0);
}
uint32_t probe_lane_reduce_max() { return avp::kLaneReduceMax; }

// out = (jobs, items, chunks) of the planned jobs (planned nullable: every non-empty job)
void probe_count(const uint32_t* job_first, uint32_t n_jobs, const uint8_t* planned, uint32_t k, uint32_t* out) {
  const avp::Counts c = avp::count(job_first, n_jobs, planned, k);
  out[0] = c.jobs, out[1] = c.items, out[2] = c.chunks;
}

// chunk_first (room for pairs + jobs + 1), chunk_items (pairs + jobs), f_ranges (2 n_jobs); returns the chunk count
uint32_t probe_plan(const uint32_t* job_first, uint32_t n_jobs, const uint8_t* planned, uint32_t k,
                    uint32_t* chunk_first, uint32_t* chunk_items, uint32_t* f_ranges, uint32_t* n_items) {
  const avp::Plan p = avp::build(job_first, n_jobs, planned, k);
  for (size_t i = 0; i < p.chunk_first.size(); i++) chunk_first[i] = p.chunk_first[i];
  for (size_t i = 0; i < p.chunk_items.size(); i++) chunk_items[i] = p.chunk_items[i];
  for (size_t i = 0; i < p.f_ranges.size(); i++) f_ranges[i] = p.f_ranges[i];
  *n_items = (uint32_t)p.chunk_items.size();
  return p.n_chunks();
}

// Every field of hl::AggVerify as (arena, offset, size in the arena's units), arenas 0 d_in (bytes), 1 d_bytes
// (bytes), 2 d_work (words); then the totals.  Returns the field count; out has room for 3 x 40 entries.
uint32_t probe_layout(uint64_t J, uint64_t n, uint64_t U, uint64_t C, uint64_t sig_stride, int keys_are_bytes,
                      uint64_t pk_len, int validate, uint64_t* out, uint64_t* totals) {
  const hl::AggVerify l(J, n, U, C, sig_stride, keys_are_bytes != 0, pk_len, validate != 0);
  const uint64_t T = l.T, M = l.M;
  const uint64_t f[][3] = {
      {0, l.gf, (J + 1) * 4}, {0, l.len, J * 4}, {0, l.sigs, J * sig_stride}, {0, l.keys, l.key_bytes},
      {0, l.umsg, U * 32}, {0, l.pmsg, n * 4}, {0, l.cf, (C + 1) * 4}, {0, l.ci, T * 4}, {0, l.fr, 2 * J * 4},
      {0, l.kv96, validate ? n * 96 : 0},
      {1, l.b_st, J}, {1, l.b_fl, J}, {1, l.b_kv, validate ? n : 0}, {1, l.b_code, n}, {1, l.b_mf, M}, {1, l.b_inc, T},
      {1, l.b_chk, J}, {1, l.b_jcode, J}, {1, l.b_ok, J}, {1, l.b_res, J}, {1, l.b_fb, J * 4},
      {2, 0, J * hl::kG2A}, {2, l.w_pk_aff, T * hl::kG1A}, {2, l.w_midx, T}, {2, l.w_fchunk, T * hl::kFp12},
      {2, l.w_F, J * hl::kFp12}, {2, l.w_minv, M * hl::kFp}, {2, l.w_haff, M * hl::kG2A}, {2, l.w_hjac, M * hl::kG2J},
      {2, l.w_hnorm, M * hl::kFp}, {2, l.w_hprep, M * 14 * hl::kFp}, {2, l.w_hq, M * 2 * hl::kG2J}};
  const uint32_t nf = sizeof f / sizeof f[0];
  for (uint32_t i = 0; i < nf; i++)
    for (int c = 0; c < 3; c++) out[3 * i + c] = f[i][c];
  totals[0] = l.in_total, totals[1] = l.bytes_total, totals[2] = l.work_words, totals[3] = l.lines_words;
  totals[4] = l.T, totals[5] = l.M;
  return nf;
}
}
