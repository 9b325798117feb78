// The run path of libblsgpu: one device's shard of a call (or of a merged batch) as one pipeline run.  run_shard is a
// short sequence of phases: the run's plan (run_plan.hpp, plain arithmetic, tested without a GPU), the staging of its
// inputs, the stream DAG of its batch pass, the sorting of the group verdicts, the fallback of failed groups' jobs.
// runtime.cpp (calls, dispatchers, the ABI) enters through run_call_shard.
#include <stdio.h>

#include "runtime_internal.hpp"

using namespace blsgpu_rt;

namespace {

static_assert(kFp == W_FP && kG1A == W_G1A && kG1J == W_G1J && kG2A == W_G2A && kG2J == W_G2J && kFp12 == W_FP12 &&
                  kMsmSlice == MSM_SLICE && kMsmBucketWords == MSM_BUCKET_WORDS && kMsmWindowWords == MSM_WINDOW_WORDS,
              "run_plan.hpp");
static_assert(miller_plan::kSteps == MILLER_STEPS && miller_plan::kMaxSegments == MILLER_MAX_SEGS, "miller_plan.hpp");

// (segs: step segments, one-lane form only)
void launch_miller_acc_auto(const PipelineBuffers& pb, bool units, hipStream_t st, uint32_t mk, const Options& opt,
                            const MillerSegs* segs = nullptr) {
  switch (acc_form(mk, pb.n_chunks, opt.miller_lanes, opt.acc6_max, opt.miller_pairs != 0)) {
    case AccForm::six: launch_miller_acc6(pb, units, st); break;
    case AccForm::pairs: launch_miller_accx(pb, units, st); break;
    case AccForm::two: launch_miller_acc2(pb, units, st); break;
    case AccForm::one: launch_miller_acc(pb, units, st, segs); break;
  }
}

// Host-side timing of run formation (diagnostics): BLSGPU_HOST_TRACE=1 prints, per run, the milliseconds spent
// merging calls, in the host prep before the input copy, and in total before the batch pass is queued.
bool host_trace() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_HOST_TRACE");
    return v && v[0] == '1';
  }();
  return on;
}
thread_local std::chrono::steady_clock::time_point tl_prep_t0;  // run_shard entered

// What the phases of one run share besides its plan and its PipelineBuffers: the device, the slot, the call's options
// and stats, and the run's streams.
// DAG of one run on the device's streams (shared by its slots):
//   signatures (s):    input copy -> decode -> [pubkeys done] job mask -> MSM -> MillerLoop(-g1, S_g)
//   messages (sm):     hash_to_G2 -> affine -> Miller lines -> [job mask done] Miller accumulation -> F reduction
//   pubkeys (sp):      aggregate -> r_i pk_i -> affine
//   tail (stl):        [S_g Miller + F done] final exponentiation per group -> results copy
// With stream pairs (BLSGPU_STREAM_PAIRS) the pubkey and tail branches run on the run's signature stream (they are
// short next to the message branch; see sp below for small runs) and consecutive runs use the other pair; without,
// each branch has its own stream shared by every run.
struct Run {
  Device& d;
  Slot& sl;
  const Options& opt;
  blsgpu_stats& st;
  uint64_t grow0;  // tl_async_grow before the run's first buffer growth
  hipStream_t s = nullptr, sm = nullptr, sp = nullptr, stl = nullptr;
  hipStream_t smsm = nullptr;  // the other pair's message stream (speculative MSM), else s
};

void pick_streams(Run& r, const RunPlan& plan) {
  Device& d = r.d;
  Slot& sl = r.sl;
  // the urgent slot runs on its own two stream pairs (Device::ust), every run on pair 0 with pair 1 idle beside it
  hipStream_t* const dst = sl.urgent ? d.ust : d.st;
  const int npairs = sl.urgent ? 2 : d.npairs;
  const int par = sl.urgent ? 0 : BLSGPU_STREAM_PAIRS ? (int)(d.run_seq.fetch_add(1) % (uint32_t)npairs) : 0;
  const int other = (par + 1) % npairs;
  r.s = BLSGPU_STREAM_PAIRS ? dst[2 * par] : dst[kSig];
  // A small run that found the device idle puts its pubkey branch on the other pair's (idle) signature stream, beside
  // its own signature decode and subgroup checks instead of in front of them: the signature branch was a small
  // call's critical path (C1 serial trace: 7.25 ms vs the message branch's 6.15).
  r.sm = BLSGPU_STREAM_PAIRS ? dst[2 * par + 1] : dst[kMsg];
  r.sp = BLSGPU_STREAM_PAIRS ? (plan.f.small && sl.alone ? dst[2 * other] : r.s) : dst[kPk];
  r.stl = BLSGPU_STREAM_PAIRS ? r.s : dst[kTail];
  if (r.opt.serial) r.sm = r.sp = r.stl = r.s;
  r.smsm = plan.f.spec ? dst[2 * other + 1] : r.s;
}

// Grows the slot's buffers for the batch pass, stages the inputs in the pinned arena (one transfer) and points
// PipelineBuffers at the device arenas.  scal_words: the shard's batch scalar words (shard_scalars' rule).
void stage_inputs(Run& r, const RunPlan& p, const blsgpu_batch& b, const uint64_t* scal_words, PipelineBuffers& pb) {
  Slot& sl = r.sl;
  const uint32_t n = p.n, nj = p.nj, s0 = p.s0, stride = p.stride;
  const InArena& in = p.in;
  sl.set_stream(r.s);  // buffer growth of the batch pass, ordered before the input copy on the same stream
  sl.h_in.ensure(in.bytes);
  sl.d_in.ensure(in.bytes);
  uint8_t* const hin = sl.h_in.p;
  // scalars: the caller applies shard_scalars' rule (each merged call its own key, in the calls' own set order)
  memcpy(hin + in.scal, scal_words, (size_t)n * 8);
  uint32_t* hjobs = reinterpret_cast<uint32_t*>(hin + in.jobs);
  for (uint32_t j = 0; j < nj; j++) hjobs[j] = p.job_sets(j).first;
  hjobs[nj] = n;
  uint8_t* hsigs = hin + in.sigs;
  uint32_t* hsiglen = reinterpret_cast<uint32_t*>(hin + in.siglen);
  if (b.sig_stride == p.sig_w) {  // one block (the decoder reads only the bytes a set's length makes valid)
    memcpy(hsigs, b.sigs + (size_t)s0 * p.sig_w, (size_t)n * p.sig_w);
    memcpy(hsiglen, b.sig_len + s0, (size_t)n * 4);
  } else {
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t len = b.sig_len[s0 + i];
      const uint32_t cl = (len == 96 || len == 192) ? len : 0;
      memcpy(hsigs + (size_t)i * p.sig_w, b.sigs + (size_t)(s0 + i) * b.sig_stride, cl);
      hsiglen[i] = len;
    }
  }
  for (uint32_t u = 0; u < p.n_umsg; u++)
    memcpy(hin + in.umsg + (size_t)u * 32, b.msgs + (size_t)(s0 + p.uniq[u]) * 32, 32);
  memcpy(hin + in.midx, p.msg_idx.data(), (size_t)n * 4);
  uint32_t* hranges = reinterpret_cast<uint32_t*>(hin + in.ranges);
  for (uint32_t g = 0; g < p.ng0; g++) {
    hranges[2 * g] = p.group_sets(g).first;
    hranges[2 * g + 1] = p.group_sets(g).second;
  }
  memcpy(hin + in.franges, p.ft.f_rng.data(), p.ft.f_rng.size() * 4);
  memcpy(hin + in.cfirst, p.chunk_first.data(), p.chunk_first.size() * 4);
  memcpy(hin + in.citems, p.chunk_items.data(), p.chunk_items.size() * 4);
  if (!p.agg_sets.empty()) memcpy(hin + in.agg, p.agg_sets.data(), p.agg_sets.size() * 4);
  if (!p.slices.empty()) memcpy(hin + in.slices, p.slices.data(), p.slices.size() * 4);
  memcpy(hin + in.rslices, p.range_slices.data(), p.range_slices.size() * 4);
  if (!p.ft.ftree.empty()) memcpy(hin + in.ftree, p.ft.ftree.data(), p.ft.ftree.size() * 4);
  if (p.merged) {
    memcpy(hin + in.ufirst, p.unit_first.data(), (size_t)(p.n_units + 1) * 4);
    memcpy(hin + in.usets, p.unit_sets.data(), p.unit_sets.size() * 4);
    memcpy(hin + in.umsgi, p.unit_msg.data(), (size_t)p.n_units * 4);
  }
  const bool keyed = p.table_mode || p.bytes_agg;  // per-set key ranges
  if (keyed) {
    uint32_t* hpkfirst = reinterpret_cast<uint32_t*>(hin + in.pk_first);
    for (uint32_t i = 0; i <= n; i++) hpkfirst[i] = b.set_pk_first[s0 + i] - p.pk_base;
    if (p.table_mode)
      memcpy(hin + in.pk_keys, b.pk_index + p.pk_base, (size_t)p.npk * 4);
    else
      memcpy(hin + in.pk_keys, b.pk_bytes + (size_t)p.pk_base * 96, (size_t)p.npk * 96);
  } else {
    memcpy(hin + in.pk_keys, b.pk_bytes + (size_t)s0 * 96, (size_t)n * 96);
  }

  sl.d_bytes.ensure(p.by.total);
  sl.d_res.ensure(p.res.bytes);
  sl.h_res.ensure(p.res.bytes);
  sl.d_S.ensure(p.S_words());
  sl.d_F.ensure(p.F_words());
  sl.d_G.ensure(p.G_words());
  sl.d_msmB.ensure(p.msmB_words());
  sl.d_msmW.ensure(p.msmW_words());
  sl.d_work.ensure(p.work.words);
  sl.d_lines.ensure(p.lines_words());
  if (p.f.keep_f) sl.d_fkeep.ensure(p.fkeep_words());
  if (p.f.segs > 1) sl.d_fseg.ensure(p.fseg_words());
  if (p.f.rsig_spec) sl.d_fb.ensure(p.fb_words());
  uint8_t* const din = sl.d_in.p;
  auto words = [&](size_t o) { return reinterpret_cast<uint32_t*>(din + o); };

  memset(&pb, 0, sizeof pb);
  pb.n = stride;
  pb.sigs = din + in.sigs;
  pb.sig_len = words(in.siglen);
  pb.sig_stride = p.sig_w;
  pb.pk_bytes = p.table_mode ? nullptr : din + in.pk_keys;
  pb.set_pk_first = keyed ? words(in.pk_first) : nullptr;
  pb.pk_index = p.table_mode ? words(in.pk_keys) : nullptr;
  pb.pk_table = r.d.table.p;
  pb.pk_table_n = r.d.table_n;
  pb.agg_sets = words(in.agg);
  pb.n_agg = (uint32_t)p.agg_sets.size();
  pb.pk_direct1 = 1;
  pb.scalars = reinterpret_cast<uint64_t*>(din + in.scal);
  pb.job_first_set = words(in.jobs);
  pb.n_jobs = nj;
  pb.umsgs = din + in.umsg;
  pb.msg_idx = words(in.midx);
  pb.n_umsg = p.n_umsg;
  pb.nm = p.nm;
  pb.n_units = p.n_units;
  pb.unit_set_first = words(in.ufirst);
  pb.unit_sets = words(in.usets);
  pb.unit_msg = words(in.umsgi);
  pb.n_chunks = p.n_chunks;
  pb.chunk_first = words(in.cfirst);
  pb.chunk_items = words(in.citems);
  uint32_t* const w = sl.d_work.p;
  const WorkArena& k = p.work;
  pb.sig_aff = w + k.sig_aff;
  pb.pk_jac = w + k.pk_jac;
  pb.pk_aff = w + k.pk_aff;
  pb.rsig = nullptr;  // S comes from the MSM (k_msm.hip), not from per-set scalings
  pb.f_chunk = w + k.f_chunk;
  pb.scal_tab = w + k.scal_tab;
  if (p.merged) pb.unit_p = w + k.unit_p;
  pb.inv_buf = w + k.inv_buf;
  pb.inv_buf_pk = w + k.inv_buf_pk;
  pb.h_aff = w + k.h_aff;
  pb.h_jac = w + k.h_jac;
  pb.h_norm = w + k.h_norm;
  pb.h_prep = w + k.h_prep;
  pb.h_q = w + k.h_q;
  pb.lines = sl.d_lines.p;
  uint8_t* const db = sl.d_bytes.p;
  pb.flags = db + p.by.flags;
  pb.mflags = db + p.by.mflags;
  pb.unit_ok = db + p.by.unit_ok;
  pb.status = reinterpret_cast<int8_t*>(db + p.by.status);
  pb.include = db + p.by.include;
  pb.job_err = reinterpret_cast<int8_t*>(sl.d_res.p + p.res.job_err);
}

// Enqueues the run's batch pass: the input copy, the four branches and the results copy (Run, above, draws the DAG).
void enqueue_batch_pass(Run& r, const RunPlan& p, const PipelineBuffers& pb) {
  Device& d = r.d;
  Slot& sl = r.sl;
  const Options& opt = r.opt;
  const Forms& f = p.f;
  const uint32_t n = p.n, ng0 = p.ng0, stride = p.stride;
  const bool merged = p.merged, coop = f.coop, excl = f.excl, spec = f.spec, keyed = p.table_mode || p.bytes_agg;
  const bool prof = opt.profile;
  const hipStream_t s = r.s, sm = r.sm, sp = r.sp, smsm = r.smsm;
  uint8_t* const din = sl.d_in.p;
  MillerSegs msegs{};
  msegs.n = p.segments.n;
  for (uint32_t j = 0; j <= msegs.n; j++) msegs.first[j] = p.segments.first[j];
  for (uint32_t j = 0; j < msegs.n; j++) msegs.dbl[j] = p.segments.dbl[j];
  auto beg = [&](int k, hipStream_t st) {
    if (prof) HIPCHK(hipEventRecord(sl.ev[2 * k], st));
  };
  auto end = [&](int k, hipStream_t st) {
    if (prof) HIPCHK(hipEventRecord(sl.ev[2 * k + 1], st));
  };
  std::unique_lock<std::mutex> enq(d.enq_mu, std::defer_lock);
  if (!sl.urgent) enq.lock();  // the urgent lane's streams are its own: nothing to keep in order with
  r.st.host_ms = ms_since(tl_run_t0);  // the slot picked the run -> its input copy is queued
  if (host_trace())
    fprintf(stderr,
            "[blsgpu host] run %u sets: merge %.2f ms, prep %.2f ms (dedupe %.2f, structure %.2f), pick-to-copy %.2f "
            "ms, %zu B in, %u Miller chunks of %u x %u segments\n",
            n, tl_merge_ms, ms_since(tl_prep_t0), p.t_dedupe_ms, p.t_struct_ms, ms_since(tl_run_t0), p.in.bytes,
            p.n_chunks, f.mk, f.segs);
  // The input copy goes on the run's signature stream, or (copy_stream, when none of the run's buffers was
  // reallocated in that stream's order) on the device's table stream: a previous run's tail still queued on the
  // signature stream of this pair then delays only this run's signature branch, not its message branch
  const bool own_copy = opt.copy_stream && !opt.serial && !sl.urgent && tl_async_grow == r.grow0;
  hipStream_t sc = own_copy ? d.table_stream : s;
  HIPCHK(hipMemcpyAsync(din, sl.h_in.p, p.in.bytes, hipMemcpyHostToDevice, sc));
  HIPCHK(hipEventRecord(sl.join_in, sc));
  if (own_copy) HIPCHK(hipStreamWaitEvent(s, sl.join_in, 0));
  HIPCHK(hipStreamWaitEvent(sm, sl.join_in, 0));
  HIPCHK(hipStreamWaitEvent(sp, sl.join_in, 0));
  // messages
  beg(1, sm);
  launch_hash_to_g2(pb, sm, f.coop_g2, excl);
  launch_h_affine(pb, sm);
  end(1, sm);
  beg(kStages, sm);
  if (!coop) {
    // two lanes per message while one lane each would leave SIMDs idle (the same rule as the accumulation's)
    const bool two = opt.lines_lanes == 2;  // lane pairs, two waves per SIMD: C2 +2-4% (profiles/r05_pairs_ab.json)
    if (two)
      launch_miller_lines2(pb, sm);
    else
      launch_miller_lines(pb, sm);
  }
  end(kStages, sm);
  // pubkeys
  beg(2, sp);
  if (keyed && pb.n_agg) launch_pk_aggregate(pb, n, sp);
  end(2, sp);
  beg(3, sp);
  launch_pk_finish(pb, n, sp);
  launch_pk_affine(pb, n, sp);
  end(3, sp);
  HIPCHK(hipEventRecord(sl.join_pk, sp));
  // signatures, then the batch equation.  A small run on an idle device starts its MSM speculatively right after
  // the decode, on the other pair's (idle) message stream, over the sets that decoded (spec mask), while the
  // subgroup checks, the pubkeys and the job mask finish: S then includes the sets the job mask drops later (a
  // failed subgroup check or pubkey, a job's other sets).  That only changes the failure path: a group whose S
  // holds a dropped set fails its equation (barring a negligible r_i coincidence; an infinity signature never
  // enters, and a dropped valid signature is in G2, so its term e(-g1, r sig) != 1) and its jobs are re-checked one
  // by one with exact masks (the fallback), while a clean group's S is exact.  Saves the MSM's ~1.5 ms on the
  // signature branch of a 128-set call.
  PipelineBuffers pbm = pb;
  if (spec) pbm.include = sl.d_bytes.p + p.by.spec;
  beg(0, s);
  launch_sig_decode(pb, n, s, f.coop_g2, spec ? sl.join_dec : nullptr, excl);
  end(0, s);
  const uint32_t* d_slices = reinterpret_cast<uint32_t*>(din + p.in.slices);
  const uint32_t* d_rslices = reinterpret_cast<uint32_t*>(din + p.in.rslices);
  if (f.rsig_spec) {  // after the pubkey branch on sp (its own work comes first) and the decode (+ subgroup checks)
    HIPCHK(hipEventRecord(sl.join_rsig, s));
    HIPCHK(hipStreamWaitEvent(sp, sl.join_rsig, 0));
    PipelineBuffers pq = pb;
    pq.rsig = sl.d_fb.p;
    pq.scal_tab = sl.d_fb.p + (size_t)stride * W_G2J;
    launch_sig_scale(pq, n, sp);
    HIPCHK(hipEventRecord(sl.join_rsig, sp));
  }
  if (spec) {
    HIPCHK(hipStreamWaitEvent(smsm, sl.join_dec, 0));
    launch_spec_mask(pb, n, pbm.include, smsm);
    launch_sig_msm(pbm, d_slices, p.n_slices, d_rslices, ng0, sl.d_msmB.p, sl.d_msmW.p, sl.d_S.p, smsm, false,
                   f.msm_tree);
    HIPCHK(hipEventRecord(sl.join_msm, smsm));
  }
  HIPCHK(hipStreamWaitEvent(s, sl.join_pk, 0));
  beg(4, s);
  launch_job_mask(pb, s);
  HIPCHK(hipEventRecord(sl.join_mask, s));
  // the message branch continues with the Miller accumulation once the include mask exists
  HIPCHK(hipStreamWaitEvent(sm, sl.join_mask, 0));
  beg(5, sm);
  if (merged) launch_unit_aggregate(pb, sm);
  if (coop)
    launch_miller_coop(pb, merged, sm, excl);
  else if (f.seg_plan)
    launch_miller_acc(pb, merged, sm, &msegs);
  else
    launch_miller_acc_auto(pb, merged, sm, f.mk, opt, &msegs);
  end(5, sm);
  if (f.keep_f && opt.keep_copy == 1)
    launch_copy_words(sl.d_fkeep.p, pb.f_chunk, (size_t)stride * W_FP12, sm);
  else if (f.keep_f)
    HIPCHK(hipMemcpyAsync(sl.d_fkeep.p, pb.f_chunk, (size_t)stride * W_FP12 * 4, hipMemcpyDeviceToDevice, sm));
  const uint32_t* d_franges = reinterpret_cast<uint32_t*>(din + p.in.franges);
  beg(6, sm);
  const uint32_t* d_ftree = reinterpret_cast<uint32_t*>(din + p.in.ftree);
  launch_group_tree(pb, d_franges, ng0, d_ftree, p.ft.n_fruns, d_ftree + 2 * (size_t)p.ft.n_fruns, p.ft.f_level_end,
                    sl.d_F.p, sm, &msegs, sl.d_fseg.p);
  end(6, sm);
  HIPCHK(hipEventRecord(sl.join_msg, sm));
  if (spec)
    HIPCHK(hipStreamWaitEvent(s, sl.join_msm, 0));
  else
    launch_sig_msm(pb, d_slices, p.n_slices, d_rslices, ng0, sl.d_msmB.p, sl.d_msmW.p, sl.d_S.p, s,
                   f.lane_tail && (opt.lane_tail_parts & 1), f.msm_tree);
  end(4, s);
  // MillerLoop(-g1, S_g) of every group now, while the message branch still runs -- or (tail_on_msg) after it, on
  // the pair's high-priority message stream with the final exponentiations: a run's cooperative tail kernels then
  // take free SIMDs before the next runs' stage kernels, and they never hold the signature stream the next run on
  // this pair copies its inputs on
  const bool tail_msg = opt.tail_on_msg && !opt.serial && BLSGPU_STREAM_PAIRS;
  hipStream_t sg = s;
  // spec_gsm: a speculative run (the device was idle when it formed) runs MillerLoop(-g1, S) right behind its MSM on
  // the other pair's message stream (high priority, nothing else queued on it yet): it starts on a nearly idle chip.
  // On the signature stream it would wait behind the run's own Miller accumulation and then behind the next run's
  // stage kernels -- a three-wave workgroup gets no CU while another run's waves fill every SIMD -- and it held the
  // burst's first run, and so the pair, for ~36 ms of the driver's 20-step window.  Measured equal (the next runs then
  // wait behind it on the other pair instead, profiles/r06_ramp_ab.json): off by default.
  if (spec && opt.spec_gsm && !tail_msg) sg = smsm;
  if (tail_msg) {
    HIPCHK(hipEventRecord(sl.join_gsm, s));
    HIPCHK(hipStreamWaitEvent(sm, sl.join_gsm, 0));
    sg = r.stl = sm;
  }
  const hipStream_t stl = r.stl;
  beg(kStages + 1, sg);
  launch_group_sig_miller(sl.d_S.p, ng0, sl.d_G.p, sg, excl && coop, f.lane_tail && (opt.lane_tail_parts & 2));
  end(kStages + 1, sg);
  HIPCHK(hipEventRecord(sl.join_gsm, sg));
  HIPCHK(hipStreamWaitEvent(stl, sl.join_gsm, 0));
  HIPCHK(hipStreamWaitEvent(stl, sl.join_msg, 0));
  if (f.rsig_spec) HIPCHK(hipStreamWaitEvent(stl, sl.join_rsig, 0));  // the run completes with its r_i sig_i
  beg(7, stl);
  launch_group_check(sl.d_S.p, sl.d_F.p, ng0, sl.d_res.p + p.res.ok, stl, nullptr, 0, sl.d_G.p, excl && coop);
  end(7, stl);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sl.h_res.p, sl.d_res.p, p.res.ok + ng0, hipMemcpyDeviceToHost, stl));
  HIPCHK(hipEventRecord(sl.done, stl));
}

// Waits for the batch pass, releases the run's pipeline place and counts the run in the call's stats.
void wait_batch_pass(Run& r, const RunPlan& p) {
  Device& d = r.d;
  Slot& sl = r.sl;
  blsgpu_stats& st = r.st;
  if (r.opt.early_release && !r.opt.serial) {
    // the run leaves the in-flight count once its message branch is done: its remaining tail (the signature side's
    // window sums / Horner / MillerLoop(-g1, S) and the final exponentiations) is short on a chip with room and must
    // not hold a pipeline place while the next runs' heavy kernels starve it
    HIPCHK(hipEventSynchronize(sl.join_msg));
    release_inflight(d, sl);
  }
  HIPCHK(hipEventSynchronize(sl.done));
  if (batch_rand::take_injection(g_fail_run_skip, g_fail_run_count)) throw HipError{hipErrorLaunchFailure};
  release_inflight(d, sl);
  st.groups += p.ng0;
  st.unique_messages += p.n_umsg;
  st.pairing_units += p.n_items;
  st.miller_chunks += p.n_chunks;
  st.run_sets = p.n;
  if (r.opt.profile) {
    for (int k = 0; k < kStages; k++) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, sl.ev[2 * k], sl.ev[2 * k + 1]));
      if (k == 5 || k == 7) {  // Miller stage = lines + accumulation; group check = MillerLoop(-g1, S) + final exp.
        const int x = k == 5 ? kStages : kStages + 1;
        float ml = 0;
        HIPCHK(hipEventElapsedTime(&ml, sl.ev[2 * x], sl.ev[2 * x + 1]));
        ms += ml;
      }
      st.stage_ms[k] += ms;
    }
  }
}

// Diagnostics (BLSGPU_FB_VERIFY=1): the fallback again from its inputs into fresh buffers once the device is idle
// -- r_i sig_i, S_j / F_j, one cooperative check per job -- compared with the first pass's S_j, F_j (as they
// are now in d_S / d_F), its uploaded lists, its results as read and as they are now in d_ok, and the answers.
void verify_fallback(Run& r, const RunPlan& p, const FallbackPlan& fp, const PipelineBuffers& pr, hipStream_t sfb,
                     const std::vector<uint32_t>& retry, const std::vector<uint32_t>& sel, const std::vector<int>& jr) {
  Slot& sl = r.sl;
  const uint32_t nr = fp.nr, stride = p.stride;
  const uint32_t* hl = sl.h_list.p;
  HIPCHK(hipDeviceSynchronize());
  const size_t wS = (size_t)W_G2J * nr, wF = (size_t)W_FP12 * nr;
  std::vector<uint32_t> S1(wS), F1(wF), S2(wS), F2(wF), L(fp.o_sel);
  std::vector<uint8_t> ok_now(sel.size() + 1), ok2(nr);
  HIPCHK(hipMemcpy(S1.data(), sl.d_S.p, wS * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(F1.data(), sl.d_F.p, wF * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(L.data(), sl.d_list.p, fp.o_sel * 4, hipMemcpyDeviceToHost));
  if (!sel.empty()) HIPCHK(hipMemcpy(ok_now.data(), sl.d_ok.p, sel.size(), hipMemcpyDeviceToHost));
  uint32_t *t_rs = nullptr, *t_S = nullptr, *t_F = nullptr;
  uint8_t* t_ok = nullptr;
  HIPCHK(hipMalloc((void**)&t_rs, (size_t)stride * 9 * W_G2J * 4));
  HIPCHK(hipMalloc((void**)&t_S, wS * 4));
  HIPCHK(hipMalloc((void**)&t_F, wF * 4));
  HIPCHK(hipMalloc((void**)&t_ok, nr));
  PipelineBuffers pq = pr;
  pq.rsig = t_rs;
  pq.scal_tab = t_rs + (size_t)stride * W_G2J;
  launch_sig_scale(pq, (uint32_t)fp.rset.size(), sfb, sl.d_list.p + fp.o_rset);
  launch_group_reduce_lane(pq, sl.d_list.p, sl.d_list.p + fp.o_rf, nr, t_S, t_F, sfb);
  launch_group_check(t_S, t_F, nr, t_ok, sfb, nullptr, 0, nullptr, false, false);
  HIPCHK(hipStreamSynchronize(sfb));
  HIPCHK(hipMemcpy(S2.data(), t_S, wS * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(F2.data(), t_F, wF * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ok2.data(), t_ok, nr, hipMemcpyDeviceToHost));
  (void)hipFree(t_rs), (void)hipFree(t_S), (void)hipFree(t_F), (void)hipFree(t_ok);
  // S / F are stored structure-of-arrays (word w of job q at w * nr + q)
  uint32_t sdiff = 0, fdiff = 0, vdiff = 0, stale = 0, ldiff = 0, first_v = UINT32_MAX, last_v = 0;
  for (uint32_t q = 0; q < nr; q++) {
    bool ds = false, df = false;
    for (size_t w = 0; w < W_G2J && !ds; w++) ds = S1[w * nr + q] != S2[w * nr + q];
    for (size_t w = 0; w < W_FP12 && !df; w++) df = F1[w * nr + q] != F2[w * nr + q];
    sdiff += ds, fdiff += df;
    if ((jr[retry[q]] == 1) != (ok2[q] != 0)) {
      vdiff++;
      first_v = std::min(first_v, q);
      last_v = q;
    }
  }
  for (size_t k = 0; k < fp.o_sel; k++) ldiff += L[k] != hl[k];
  for (size_t k = 0; k < sel.size(); k++) stale += (ok_now[k] != 0) != (sl.h_ok.p[k] != 0);
  if (vdiff || sdiff || fdiff || stale || ldiff)
    fprintf(stderr, "[blsgpu fbverify] %u-set run, %u retried jobs (nsub %u, direct %d, busy %d, keep_f %d, rsig_spec "
            "%d, spec %d, coop %d, lanes %d): answers that differ on re-check %u (q %u-%u), S_j differ %u, F_j differ "
            "%u, results read vs now %u, list words %zu\n", p.n, nr, fp.nsub, (int)fp.direct, (int)fp.busy,
            (int)p.f.keep_f, (int)p.f.rsig_spec, (int)p.f.spec, (int)p.f.coop,
            (int)fp.lane_checks((uint32_t)sel.size()), vdiff, first_v, last_v, sdiff, fdiff, stale, (size_t)ldiff);
  else
    fprintf(stderr, "[blsgpu fbverify] ok: %u-set run, %u retried jobs\n", p.n, nr);
}

// The fallback (run_plan.hpp plan_fallback): every retried job's own verdict into jr, in one or two check rounds.
void run_fallback(Run& r, const RunPlan& p, const PipelineBuffers& pb, const std::vector<uint32_t>& retry,
                  std::vector<int>& jr) {
  Slot& sl = r.sl;
  const Options& opt = r.opt;
  blsgpu_stats& st = r.st;
  // the fallback runs on the slot's own stream (the batch pass is complete: sl.done was waited for), its buffers grow
  // there
  const hipStream_t sfb = sl.fb ? sl.fb : r.stl;
  sl.set_stream(sfb);
  const FallbackPlan fp = plan_fallback(p, retry, opt, sl.alone);
  const uint32_t nr = fp.nr, nsub = fp.nsub, stride = p.stride;
  const bool rsig_spec = p.f.rsig_spec;
  // One check launch of `count` entries (sel null: entries 0 .. ng): cooperative checks (small runs, idle device), or
  // for many checks under load MillerLoop(-g1, S) one lane per entry and the final exponentiation on six lanes per
  // check (fb_check6, gt6.hpp), or everything one lane per check
  auto fb_check = [&](const uint32_t* S, const uint32_t* F, uint32_t ng, uint8_t* ok, const uint32_t* sel,
                      uint32_t count) {
    if (fp.lane_checks(count) && opt.fb_check6 == 2) {  // the Miller loop on six lanes too, from stored lines
      sl.d_lines.ensure((size_t)ng * kMillerLineWords);
      sl.d_fbflags.ensure(ng);
      launch_check6_miller(S, F, ng, ok, sfb, sel, count, sl.d_lines.p, sl.d_fbflags.p);
    } else if (fp.lane_checks(count) && opt.fb_check6) {
      sl.d_G.ensure((size_t)W_FP12 * ng);
      launch_group_sig_miller_sel(S, ng, sel, count, sl.d_G.p, sfb);
      launch_group_check6(F, sl.d_G.p, ng, ok, sfb, sel, count);
    } else {
      launch_group_check(S, F, ng, ok, sfb, sel, count, nullptr, false, fp.lane_checks(count));
    }
  };
  sl.h_list.ensure(fp.words);
  sl.d_list.ensure(fp.words);
  uint32_t* hl = sl.h_list.p;
  memcpy(hl, fp.rr.data(), fp.rr.size() * 4);
  memcpy(hl + fp.o_rf, fp.rf.data(), fp.rf.size() * 4);
  memcpy(hl + fp.o_rfirst, fp.rfirst.data(), fp.rfirst.size() * 4);
  memcpy(hl + fp.o_ritems, fp.ritems.data(), fp.ritems.size() * 4);
  memcpy(hl + fp.o_rsl, fp.rsl.data(), fp.rsl.size() * 4);
  memcpy(hl + fp.o_rrs, fp.rrs.data(), fp.rrs.size() * 4);
  memcpy(hl + fp.o_rset, fp.rset.data(), fp.rset.size() * 4);
  if (nsub) memcpy(hl + fp.o_sub, fp.subr.data(), fp.subr.size() * 4);
  sl.d_ok.ensure(nr + nsub);
  sl.h_ok.ensure(nr + nsub);
  sl.d_S.ensure((size_t)W_G2J * (nr + nsub));
  sl.d_F.ensure((size_t)W_FP12 * (nr + nsub));
  uint32_t* const dS = sl.d_S.p;  // per-job S_j, F_j (stride nr), then the sub-groups' (stride nsub)
  uint32_t* const dF = sl.d_F.p;
  uint32_t* const dS_sub = sl.d_S.p + (size_t)W_G2J * nr;
  uint32_t* const dF_sub = sl.d_F.p + (size_t)W_FP12 * nr;
  uint32_t* const dl = sl.d_list.p;
  HIPCHK(hipMemcpyAsync(dl, hl, fp.o_sel * 4, hipMemcpyHostToDevice, sfb));
  PipelineBuffers pr = pb;
  pr.n_chunks = fp.nc;
  pr.chunk_first = dl + fp.o_rfirst;
  pr.chunk_items = dl + fp.o_ritems;
  if (p.f.keep_f) {
    pr.f_chunk = sl.d_fkeep.p;  // the batch pass's values: no Miller loop is recomputed
  } else {
    st.fallback_miller += (uint32_t)fp.ritems.size();
    if (p.f.coop)  // no stored lines in a cooperative run: the per-job chunks hold one set each (mk = 1)
      launch_miller_coop(pr, false, sfb);
    else
      launch_miller_acc_auto(pr, false, sfb, p.f.mk_whole, opt);
  }
  st.fallback_jobs += nr;
  if (fp.small_jobs) {
    // r_i sig_i for the retried sets (G2 window tables and results in the fallback's own buffers), unless the batch
    // pass already formed them (rsig_spec: every set of the run, by set index)
    if (!rsig_spec) sl.d_fb.ensure(p.fb_words());
    pr.rsig = sl.d_fb.p;
    pr.scal_tab = sl.d_fb.p + (size_t)stride * W_G2J;
    if (!rsig_spec) launch_sig_scale(pr, (uint32_t)fp.rset.size(), sfb, dl + fp.o_rset);
    launch_group_reduce_lane(pr, dl, dl + fp.o_rf, nr, dS, dF, sfb);
  } else {
    sl.d_msmB.ensure((size_t)MSM_BUCKET_WORDS * std::max<uint32_t>(fp.nrs, 1));
    sl.d_msmW.ensure((size_t)MSM_WINDOW_WORDS * nr);
    launch_sig_msm(pr, dl + fp.o_rsl, fp.nrs, dl + fp.o_rrs, nr, sl.d_msmB.p, sl.d_msmW.p, dS, sfb);
    launch_group_reduce(pr, dl + fp.o_rf, nr, dF, sfb);
  }
  std::vector<uint32_t> sel;  // jobs to check on their own
  if (nsub) {
    if (nsub >= kFbLaneMin)
      launch_range_combine_lane(dS, dF, nr, dl + fp.o_sub, nsub, dS_sub, dF_sub, sfb);
    else
      launch_range_combine(dS, dF, nr, dl + fp.o_sub, nsub, dS_sub, dF_sub, sfb);
    fb_check(dS_sub, dF_sub, nsub, sl.d_ok.p + nr, nullptr, nsub);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sl.h_ok.p + nr, sl.d_ok.p + nr, nsub, hipMemcpyDeviceToHost, sfb));
    HIPCHK(hipEventRecord(sl.done, sfb));
    HIPCHK(hipEventSynchronize(sl.done));
    for (uint32_t t = 0; t < nsub; t++)
      for (uint32_t q = fp.subr[2 * t]; q < fp.subr[2 * t + 1]; q++) {
        if (sl.h_ok.p[nr + t]) jr[retry[q]] = 1;
        else sel.push_back(q);
      }
  } else {
    for (uint32_t q = 0; q < nr; q++) sel.push_back(q);
  }
  if (!sel.empty()) {
    const uint32_t ns = (uint32_t)sel.size();
    memcpy(hl + fp.o_sel, sel.data(), (size_t)ns * 4);
    HIPCHK(hipMemcpyAsync(dl + fp.o_sel, hl + fp.o_sel, (size_t)ns * 4, hipMemcpyHostToDevice, sfb));
    fb_check(dS, dF, nr, sl.d_ok.p, dl + fp.o_sel, ns);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sl.h_ok.p, sl.d_ok.p, ns, hipMemcpyDeviceToHost, sfb));
    HIPCHK(hipEventRecord(sl.done, sfb));
    HIPCHK(hipEventSynchronize(sl.done));
    for (uint32_t k = 0; k < ns; k++) jr[retry[sel[k]]] = sl.h_ok.p[k] ? 1 : 0;
  }
  if (fb_verify() && fp.small_jobs) verify_fallback(r, p, fp, pr, sfb, retry, sel, jr);
}

// a failed group whose clean jobs all verify on their own: its batch equation was computed wrong (the random
// combination of valid sets always holds)
void report_spurious_groups(Run& r, const RunPlan& p, const Classified& c) {
  for (uint32_t g : c.failed_g) {
    const uint32_t first = p.group_jobs[g].first, end = p.group_jobs[g].second;
    bool all_ok = true;
    for (uint32_t j = first; j < end && all_ok; j++)
      if (c.jr[j] != 1 && c.jr[j] >= 0) all_ok = false;  // errors (negative) are not in the equation
    if (all_ok) {
      r.d.spurious_groups.fetch_add(1, std::memory_order_relaxed);
      fprintf(stderr, "[blsgpu] device %d: batch group %u (jobs %u-%u) of a %u-set run failed its equation while "
              "every job verifies on its own (spec %d, merged %d, coop %d, mk %u)\n", r.d.id, g, first, end - 1, p.n,
              (int)p.f.spec, (int)p.merged, (int)p.f.coop, p.f.mk);
    }
  }
}

// Runs one device's shard on one slot.  Writes job_result[job_begin..job_end).
// A slot's run leaves the device's in-flight count (once): its batch pass is complete on the GPU, so another slot
// may start the next run while this one finishes on the host (results, fallback round trips).
// With `pool` (group_policy 1), the groups are the list's job ranges (run_plan.hpp plan_run, classify_groups).
// scal_words: the shard's batch scalar words (shard_scalars' rule, in the batch's set order); seed: the message
// index's hash key.
int run_shard(Device& d, Slot& sl, const blsgpu_batch& b, const Shard& sh, int8_t* job_result, uint64_t seed,
              const Options& opt, uint32_t max_index, blsgpu_stats& st, const uint64_t* scal_words,
              const std::vector<GroupPlanEntry>* pool = nullptr) {
  if (sh.job_end == sh.job_begin) return BLSGPU_OK;
  HIPCHK(hipSetDevice(d.id));
  tl_prep_t0 = std::chrono::steady_clock::now();
  Run r{d, sl, opt, st, tl_async_grow};
  // the device's table must hold every index of the call (checked per device, under its table lock: a
  // call may race an upload that has reached some devices only)
  const bool table_keys = !b.pk_bytes && b.set_pk_first && b.set_pk_first[sh.set_end] > b.set_pk_first[sh.set_begin];
  if (table_keys && max_index >= d.table_n) return BLSGPU_ERR_ARGS;
  RunEnv env;
  env.urgent = sl.urgent, env.alone = sl.alone;
  env.stream_pairs = BLSGPU_STREAM_PAIRS, env.exclusive_small = BLSGPU_EXCLUSIVE_SMALL;
  {
    std::lock_guard<std::mutex> lk(d.fail_mu);
    env.fail_rate = d.fail_rate;
  }
  const RunPlan plan = plan_run(b, sh, opt, env, seed, pool,
                                host_trace() ? +[]() -> double { return ms_since(tl_prep_t0); } : nullptr);
  pick_streams(r, plan);
  PipelineBuffers pb;
  stage_inputs(r, plan, b, scal_words, pb);
  enqueue_batch_pass(r, plan, pb);
  wait_batch_pass(r, plan);
  Classified c = classify_groups(plan, reinterpret_cast<const int8_t*>(sl.h_res.p + plan.res.job_err),
                                 sl.h_res.p + plan.res.ok, plan.f.spec);
  st.batch_retries += c.batch_retries;
  st.batch_sigs_success += c.batch_sigs_success;
  if (!c.retry.empty()) run_fallback(r, plan, pb, c.retry, c.jr);
  report_spurious_groups(r, plan, c);
  for (uint32_t j = 0; j < plan.nj; j++) job_result[sh.job_begin + j] = (int8_t)c.jr[j];
  if (!pool && plan.ng0) {  // the device's invalid-set rate estimate (group_adapt)
    std::lock_guard<std::mutex> lk(d.fail_mu);
    d.fail_rate = next_fail_rate(plan, c.jr, d.fail_rate);
  }
  return BLSGPU_OK;
}

// group_policy 1: the reference pool's grouping on the GPU (run_plan.hpp plan_pool_groups).  The jobs are laid out
// group after group (one permuted batch),
// run as one pipeline with that group plan, and each call gets the first rejection of its jobs in job order, else
// false if a job is false, else true (Promise.all over the call's jobs, index.ts:165-173; oracle/blscpu.c
// blscpu_verify_jobs applies the same rule).
int run_pool_policy(Device& d, Slot& sl, const blsgpu_batch& b, const Shard& sh, int8_t* job_result, uint64_t seed,
                    const Options& opt, uint32_t max_index, blsgpu_stats& st, const uint64_t* scal_words) {
  const uint32_t s0 = sh.set_begin, n = sh.set_end - sh.set_begin;
  const PoolPlan pp = plan_pool_groups(b.job_first_set, b.job_flags, sh.job_begin, sh.job_end);
  const std::vector<PoolSub>& subs = pp.subs;
  const std::vector<uint32_t>& order = pp.order;
  const int mode = pk_mode(b);
  const uint32_t ns = (uint32_t)subs.size();
  std::vector<uint32_t> jfs{0}, siglen, spf{0}, pki;
  std::vector<uint8_t> flags, msgs, sigs, pkb;
  std::vector<uint64_t> scal;
  jfs.reserve(ns + 1);
  siglen.reserve(n);
  scal.reserve(n);
  msgs.reserve((size_t)n * 32);
  sigs.reserve((size_t)n * b.sig_stride);
  for (uint32_t x : order) {
    const PoolSub& u = subs[x];
    jfs.push_back(jfs.back() + u.e - u.a);
    flags.push_back(u.batchable ? 1 : 0);
    for (uint32_t i = u.a; i < u.e; i++) {
      siglen.push_back(b.sig_len[i]);
      sigs.insert(sigs.end(), b.sigs + (size_t)i * b.sig_stride, b.sigs + (size_t)(i + 1) * b.sig_stride);
      msgs.insert(msgs.end(), b.msgs + (size_t)i * 32, b.msgs + (size_t)i * 32 + 32);
      scal.push_back(scal_words[i - s0]);
      if (mode == 1) {
        pkb.insert(pkb.end(), b.pk_bytes + (size_t)i * 96, b.pk_bytes + (size_t)(i + 1) * 96);
      } else {
        const uint32_t k0 = b.set_pk_first[i], k1 = b.set_pk_first[i + 1];
        spf.push_back(spf.back() + k1 - k0);
        if (mode == 0)
          pki.insert(pki.end(), b.pk_index + k0, b.pk_index + k1);
        else
          pkb.insert(pkb.end(), b.pk_bytes + (size_t)k0 * 96, b.pk_bytes + (size_t)k1 * 96);
      }
    }
  }
  blsgpu_batch pb{};
  pb.n_sets = n;
  pb.n_jobs = ns;
  pb.job_first_set = jfs.data();
  pb.job_flags = flags.data();
  pb.pk_bytes = mode ? pkb.data() : nullptr;
  pb.set_pk_first = mode == 1 ? nullptr : spf.data();
  pb.pk_index = mode == 0 ? pki.data() : nullptr;
  pb.msgs = msgs.data();
  pb.sigs = sigs.data();
  pb.sig_len = siglen.data();
  pb.sig_stride = b.sig_stride;
  std::vector<int8_t> sub_res(std::max<uint32_t>(ns, 1), 0);
  const Shard all{0, ns, 0, n};
  const int rc = run_shard(d, sl, pb, all, sub_res.data(), seed, opt, max_index, st, scal.data(), &pp.groups);
  if (rc != BLSGPU_OK) return rc;
  std::vector<uint32_t> pos(ns);
  for (uint32_t k = 0; k < ns; k++) pos[order[k]] = k;
  std::vector<uint8_t> seen(sh.job_end - sh.job_begin, 0);
  for (uint32_t j = sh.job_begin; j < sh.job_end; j++) job_result[j] = 1;
  for (uint32_t x = 0; x < ns; x++) {
    const uint32_t call = subs[x].call;
    const int8_t r = sub_res[pos[x]];
    if (seen[call - sh.job_begin]) continue;
    if (r < 0) {
      job_result[call] = r;
      seen[call - sh.job_begin] = 1;
    } else if (r == 0) {
      job_result[call] = 0;
    }
  }
  return BLSGPU_OK;
}

}  // namespace

namespace blsgpu_rt __attribute__((visibility("hidden"))) {

void release_inflight(Device& d, Slot& sl) {
  {
    std::lock_guard<std::mutex> lk(d.q_mu);
    if (!sl.in_flight) return;
    sl.in_flight = false;
    d.runs_inflight--;
  }
  d.q_cv.notify_all();
}

// One shard of a call (or a merged batch) under the call's group policy.
int run_call_shard(Device& d, Slot& sl, const blsgpu_batch& b, const Shard& sh, int8_t* job_result, uint64_t seed,
                   const Options& opt, uint32_t max_index, blsgpu_stats& st, const uint64_t* scal_words) {
  if (opt.group_policy == 1) return run_pool_policy(d, sl, b, sh, job_result, seed, opt, max_index, st, scal_words);
  return run_shard(d, sl, b, sh, job_result, seed, opt, max_index, st, scal_words);
}

}  // namespace blsgpu_rt
