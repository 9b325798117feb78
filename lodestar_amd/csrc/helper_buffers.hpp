// From layouts to kernel arguments for the helper calls that run three branches (helpers.cpp: verify_same_message,
// blsgpu_aggregate_verify): the functions here fill the kernels' buffer structs (kernels.h) with pointers into
// Device::helper's arenas at the offsets helper_layout.hpp names.  They copy and launch nothing.
#pragma once
#include "helper_layout.hpp"
#include "runtime_internal.hpp"

namespace blsgpu_rt __attribute__((visibility("hidden"))) {

// The message branch: U unique messages at `umsgs` are hashed to the first U of M G2 columns (hl::MsgBranch `m` in
// d_work, flags at `mflags`, Miller lines in d_lines).
inline PipelineBuffers msg_branch(Slot& sl, const helper_layout::MsgBranch& m, const uint8_t* umsgs, uint32_t U,
                                  uint32_t M, uint8_t* mflags) {
  uint32_t* w = sl.d_work.p;
  PipelineBuffers pm{};
  pm.umsgs = umsgs;
  pm.n_umsg = U;
  pm.nm = M;
  pm.inv_buf = w + m.inv;
  pm.h_aff = w + m.h_aff;
  pm.h_jac = w + m.h_jac;
  pm.h_norm = w + m.h_norm;
  pm.h_prep = w + m.h_prep;
  pm.h_q = w + m.h_q;
  pm.mflags = mflags;
  pm.lines = sl.d_lines.p;
  return pm;
}

// blsgpu_aggregate_verify's inputs: job j owns pairs [job_first[j], job_first[j + 1]) and one signature
struct AvArgs {
  uint32_t J, n;  // jobs, pairs
  const uint32_t* job_first;
  const uint8_t* pk_bytes;
  uint32_t pk_len;
  const uint32_t* pk_index;
  const uint8_t* sigs;
  uint32_t sig_stride;
  const uint32_t* sig_len;
  uint32_t flags;
  bool validate() const { return (flags & BLSGPU_AV_VALIDATE_KEYS) != 0; }
  bool lane_flag() const { return (flags & BLSGPU_AV_LANE_FORMS) != 0; }
};
// Where everything of such a call lies (hl::AggVerify `l`; U unique messages, C Miller chunks)
struct AvCall {
  PipelineBuffers pb;  // the signature decode: one signature per job
  PipelineBuffers pm;  // the message branch: U hashed columns of the M = U + J
  AvBuffers av;        // the item kernels' view (k_aggverify.hip): pairs, jobs, the T items and the M columns
  PipelineBuffers px;  // the Miller accumulation over the T items and the M columns
};
inline AvCall av_buffers(Device& d, const helper_layout::AggVerify& l, const AvArgs& a, uint32_t U, uint32_t C) {
  Slot& sl = d.helper;
  uint8_t* din = sl.d_in.p;
  uint8_t* db = sl.d_bytes.p;
  uint32_t* w = sl.d_work.p;
  const bool validate = a.validate();
  AvCall c{};
  PipelineBuffers& pb = c.pb;
  pb.n = a.J;
  pb.sigs = din + l.sigs;
  pb.sig_len = reinterpret_cast<uint32_t*>(din + l.len);
  pb.sig_stride = a.sig_stride;
  pb.sig_aff = w;
  pb.flags = db + l.b_fl;
  pb.status = reinterpret_cast<int8_t*>(db + l.b_st);
  c.pm = msg_branch(sl, l.msg(), din + l.umsg, U, (uint32_t)l.M, db + l.b_mf);
  AvBuffers& av = c.av;
  av.n_pairs = a.n;
  av.n_jobs = a.J;
  av.n_items = (uint32_t)l.T;
  av.n_umsg = U;
  av.nm = (uint32_t)l.M;
  av.job_first = reinterpret_cast<uint32_t*>(din + l.gf);
  av.pk_bytes = !a.pk_bytes ? nullptr : validate ? din + l.kv96 : din + l.keys;
  av.kv_status = validate ? reinterpret_cast<int8_t*>(db + l.b_kv) : nullptr;
  av.pk_index = a.pk_bytes ? nullptr : reinterpret_cast<uint32_t*>(din + l.keys);
  av.pk_table = d.table.p;
  av.pk_table_n = d.table_n;
  av.pair_msg = reinterpret_cast<uint32_t*>(din + l.pmsg);
  av.sig_aff = pb.sig_aff;
  av.sig_flags = pb.flags;
  av.sig_status = pb.status;
  av.pk_aff = w + l.w_pk_aff;
  av.msg_idx = w + l.w_midx;
  av.include = db + l.b_inc;
  av.pair_code = reinterpret_cast<int8_t*>(db + l.b_code);
  av.h_aff = c.pm.h_aff;
  av.mflags = c.pm.mflags;
  av.checked = db + l.b_chk;
  av.job_code = reinterpret_cast<int8_t*>(db + l.b_jcode);
  av.first_bad = reinterpret_cast<uint32_t*>(db + l.b_fb);
  PipelineBuffers& px = c.px = c.pm;
  px.n = (uint32_t)l.T;
  px.n_umsg = (uint32_t)l.M;
  px.pk_aff = av.pk_aff;
  px.include = av.include;
  px.msg_idx = av.msg_idx;
  px.n_chunks = C;
  px.chunk_first = reinterpret_cast<uint32_t*>(din + l.cf);
  px.chunk_items = reinterpret_cast<uint32_t*>(din + l.ci);
  px.f_chunk = w + l.w_fchunk;
  return c;
}

}  // namespace blsgpu_rt
