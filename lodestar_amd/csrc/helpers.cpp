// The synchronous helper calls of libblsgpu (include/blsgpu.h): aggregation, same-message verification, AggregateVerify,
// key validation, signing roots and the debug ops.  Each runs start to finish on device 0 under Device::helper_mu, on
// table_stream, in Device::helper's buffers; helper_call is the envelope they share and helper_layout.hpp says where
// every field of their device arenas lies.  The asynchronous verification pipeline is runtime.cpp and pipeline.cpp.
#include "aggverify_plan.hpp"
#include "awr_parts.hpp"
#include "committee_plan.hpp"
#include "helper_buffers.hpp"
#include "helper_layout.hpp"
#include "runtime_internal.hpp"
#include "same_plan.hpp"

using namespace blsgpu_rt;
namespace hl = helper_layout;
namespace avp = aggverify_plan;
namespace sp = same_plan;
namespace cmp = committee_plan;

static_assert(cmp::kNoComplement == BLSGPU_BITS_NO_COMPLEMENT && cmp::kErrArgs == BLSGPU_ERR_ARGS &&
                  cmp::kMaxUploadMembers == 1u << 20,
              "committee_plan.hpp restates include/blsgpu.h");
static_assert(hl::kFp == W_FP && hl::kG1A == W_G1A && hl::kG1J == W_G1J && hl::kG2A == W_G2A && hl::kG2J == W_G2J &&
                  hl::kFp12 == W_FP12 && hl::kAwrTabWords == AWR_TAB_WORDS && hl::kMillerLineWords == kMillerLineWords,
              "helper_layout.hpp restates the element widths of kernels.h");
static_assert(sp::kBlockGroups == SAME_BLOCK_GROUPS && sp::kBlockGroups == 1024,
              "same_plan.hpp restates the block size of kernels.h; include/blsgpu.h documents blocks of 1024 groups");
static_assert(avp::kCoopMax == sp::kCoopMax, "one form threshold for the same-message calls and AggregateVerify");

namespace {

// The envelope of every helper call: registers the call with the context (BLSGPU_ERR_CLOSED once it is closing),
// takes device 0's helper lock -- and its table lock, shared, when the call reads the pubkey table -- selects the
// device and runs body(device), whose value is the call's.  A HIP failure anywhere inside is BLSGPU_DEVICE_ERROR.
template <class Body>
int helper_call(blsgpu_ctx* ctx, bool reads_table, Body body) {
  if (!enter(ctx)) return BLSGPU_ERR_CLOSED;
  struct Leave {
    blsgpu_ctx* ctx;
    ~Leave() { leave(ctx); }
  } leave_on_exit{ctx};
  Device& d = *ctx->devs[0];
  try {
    std::lock_guard<std::mutex> helper(d.helper_mu);
    std::shared_lock<std::shared_mutex> tl(d.table_mu, std::defer_lock);
    if (reads_table) tl.lock();
    HIPCHK(hipSetDevice(d.id));
    return body(d, d.helper, d.table_stream);
  } catch (HipError&) {
    return BLSGPU_DEVICE_ERROR;
  }
}

// Grows a buffer of the committee store to `need` words, keeping its first `keep` (DevBuf::ensure keeps nothing): the
// way the pubkey table grows.  Ends synchronized when it grew.
void grow_keeping(DevBuf<uint32_t>& b, size_t keep, size_t need, hipStream_t s) {
  if (need <= b.cap) return;
  DevBuf<uint32_t> nb;
  nb.ensure(std::max(need, b.cap + b.cap / 2));
  if (keep) HIPCHK(hipMemcpyAsync(nb.p, b.p, keep * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  b.release();
  b = nb;
}
// the device's committee store and pubkey table as the kernels take them (under table_mu)
CommitteeStore committee_store(Device& d) {
  return CommitteeStore{d.cm_first.p, d.cm_members.p, d.cm_sums.p, d.table.p, d.table_n};
}

// The grouped calls' inputs: signatures [group_first[g], group_first[g + 1]) form group g; the same-message calls
// add one key per signature, bytes or table indices.
struct Grouped {
  uint32_t G;
  const uint32_t* group_first;
  const uint8_t* sigs;
  uint32_t sig_stride;
  const uint32_t* sig_len;
  const uint8_t* pk_bytes = nullptr;
  const uint32_t* pk_index = nullptr;
  uint32_t n = 0;  // group_first[G], set by check_group_layout
};

// BLSGPU_OK and total = first[count], or BLSGPU_ERR_ARGS: the offsets start at 0, never decrease and end at most at
// 2^20 (group_first of the grouped calls, job_first of blsgpu_aggregate_verify).
int check_offsets(const uint32_t* first, uint32_t count, uint32_t& total) {
  if (first[0] != 0) return BLSGPU_ERR_ARGS;
  for (uint32_t g = 0; g < count; g++)
    if (first[g + 1] < first[g]) return BLSGPU_ERR_ARGS;
  total = first[count];
  return total > (1u << 20) ? BLSGPU_ERR_ARGS : BLSGPU_OK;
}
// BLSGPU_ERR_ARGS for a 192-byte signature under a stride below 192
int check_sig_lens(const uint32_t* sig_len, uint32_t n_sigs, uint32_t sig_stride) {
  if (sig_stride < 192)
    for (uint32_t k = 0; k < n_sigs; k++)
      if (sig_len[k] == 192) return BLSGPU_ERR_ARGS;
  return BLSGPU_OK;
}
// BLSGPU_OK and a.n, or BLSGPU_ERR_ARGS: both checks on a grouped call's signatures
int check_group_layout(Grouped& a) {
  if (int e = check_offsets(a.group_first, a.G, a.n)) return e;
  return check_sig_lens(a.sig_len, a.n, a.sig_stride);
}

// What both same-message calls refuse before anything is written or reaches the device: no entropy for the call's
// scalars (else `words` and the message index's hash key) and, under the table lock, a table index past the table.
int same_begin(const Device& d, const Grouped& a, uint64_t seed, std::vector<uint64_t>& words, uint64_t& hash_key) {
  batch_rand::Key key;
  if (!resolve_key(seed, key, hash_key)) return BLSGPU_ERR_ENTROPY;
  words.resize(a.n);
  batch_rand::words(key, 0, a.n, words.data());
  if (a.pk_index)
    for (uint32_t k = 0; k < a.n; k++)
      if (a.pk_index[k] >= d.table_n) return BLSGPU_ERR_ARGS;
  return BLSGPU_OK;
}

// Copies group_first | sig_len | sigs to the fields gf, len, sigs of layout `l` in d_in and describes the signatures to
// the decode: points at the start of d_work, flags and status bytes where the caller says.
template <class Layout>
PipelineBuffers sig_inputs(Slot& sl, const Grouped& a, const Layout& l, uint8_t* flags, uint8_t* status,
                           hipStream_t s) {
  uint8_t* din = sl.d_in.p;
  HIPCHK(hipMemcpyAsync(din + l.gf, a.group_first, (size_t)(a.G + 1) * 4, hipMemcpyHostToDevice, s));
  if (a.n) {
    HIPCHK(hipMemcpyAsync(din + l.len, a.sig_len, (size_t)a.n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.sigs, a.sigs, (size_t)a.n * a.sig_stride, hipMemcpyHostToDevice, s));
  }
  PipelineBuffers pb{};
  pb.n = a.n;
  pb.sigs = din + l.sigs;
  pb.sig_len = reinterpret_cast<uint32_t*>(din + l.len);
  pb.sig_stride = a.sig_stride;
  pb.sig_aff = sl.d_work.p;
  pb.flags = flags;
  pb.status = reinterpret_cast<int8_t*>(status);
  return pb;
}

// The start both same-message calls share (`l`: hl::Awr or hl::Same): the inputs words | group_first | sig_len | sigs |
// keys go to d_in, and the signature decode (pb) and the randomized sums (the value) are told where everything of
// theirs lies: inputs in d_in, points, window scratch and sums in d_work, the b_ byte fields at `bytes`.
template <class Layout>
AwrBuffers same_inputs(Device& d, const Grouped& a, const Layout& l, uint8_t* bytes, const uint64_t* words,
                       uint32_t lanes, hipStream_t s, PipelineBuffers& pb) {
  uint8_t* din = d.helper.d_in.p;
  uint32_t* w = d.helper.d_work.p;
  pb = sig_inputs(d.helper, a, l.in, bytes + l.b_fl, bytes + l.b_st, s);
  if (a.n) {
    HIPCHK(hipMemcpyAsync(din + l.in.words, words, (size_t)a.n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.in.keys, a.pk_bytes ? (const void*)a.pk_bytes : (const void*)a.pk_index,
                          l.in.key_bytes, hipMemcpyHostToDevice, s));
  }
  AwrBuffers ab{};
  ab.n = a.n;
  ab.n_groups = a.G;
  ab.group_first = reinterpret_cast<uint32_t*>(din + l.in.gf);
  ab.words = reinterpret_cast<uint64_t*>(din + l.in.words);
  ab.pk_bytes = a.pk_bytes ? din + l.in.keys : nullptr;
  ab.pk_index = a.pk_bytes ? nullptr : reinterpret_cast<uint32_t*>(din + l.in.keys);
  ab.pk_table = d.table.p;
  ab.pk_table_n = d.table_n;
  ab.sig_aff = pb.sig_aff;
  ab.sig_flags = pb.flags;
  ab.sig_status = pb.status;
  ab.tab = w + l.w_tab;
  ab.tab_n = lanes;
  ab.sum_pk = w + l.w_sum_pk;
  ab.sum_sig = w + l.w_sum_sig;
  ab.err_k = reinterpret_cast<uint32_t*>(bytes + l.b_ek);
  ab.err_c = reinterpret_cast<int8_t*>(bytes + l.b_ec);
  return ab;
}

// The randomized sums of both same-message calls when the call is split (awr_parts.hpp; `on` false: it is not, and
// the sums run as they always did).  Copies the plan's part_first and group_part to their fields of hl::AwrParts `lp`
// in d_parts -- they go up with the inputs -- and keeps the call's `ab` as the sums over the parts take it: the parts
// for groups, part-sized sums and errors in d_parts (ab.tab_n is the parts' launched lanes already).
struct AwrSplit {
  bool on = false;
  AwrBuffers parts;
  const uint32_t* group_part = nullptr;
  uint32_t L_fold = 1;  // lanes per group of the fold
};
AwrSplit awr_split_upload(Slot& sl, const hl::AwrParts& lp, const awr_parts::Plan& ap, const AwrBuffers& ab,
                          hipStream_t s) {
  AwrSplit sp;
  if (!ap.split()) return sp;
  uint8_t* dp = reinterpret_cast<uint8_t*>(sl.d_parts.p);
  HIPCHK(hipMemcpyAsync(dp + lp.pf, ap.part_first.data(), ap.part_first.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dp + lp.gp, ap.group_part.data(), ap.group_part.size() * 4, hipMemcpyHostToDevice, s));
  sp.on = true;
  sp.L_fold = ap.L_fold;
  sp.group_part = reinterpret_cast<uint32_t*>(dp + lp.gp);
  sp.parts = ab;
  sp.parts.group_first = reinterpret_cast<uint32_t*>(dp + lp.pf);
  sp.parts.n_groups = ap.n_parts;
  sp.parts.sum_pk = reinterpret_cast<uint32_t*>(dp + lp.sum_pk);
  sp.parts.sum_sig = reinterpret_cast<uint32_t*>(dp + lp.sum_sig);
  sp.parts.err_k = reinterpret_cast<uint32_t*>(dp + lp.ek);
  sp.parts.err_c = reinterpret_cast<int8_t*>(dp + lp.ec);
  return sp;
}
// sum_pk / sum_sig of `a` and its groups' first errors, on L lanes per group: in one launch, or -- a split call -- over
// the parts (in a's window scratch) and folded.  Everything after them reads the same fields of `a` either way.
void awr_sum_pk(const AwrBuffers& a, const AwrSplit& sp, uint32_t L, hipStream_t s) {
  if (!sp.on) return launch_awr_sum_pk(a, L, s);
  AwrBuffers p = sp.parts;
  p.tab = a.tab;
  launch_awr_sum_pk(p, L, s);
  launch_awr_fold_pk(p, a, sp.group_part, sp.L_fold, s);
}
void awr_sum_sig(const AwrBuffers& a, const AwrSplit& sp, uint32_t L, hipStream_t s) {
  if (!sp.on) return launch_awr_sum_sig(a, L, s);
  AwrBuffers p = sp.parts;
  p.tab = a.tab;
  launch_awr_sum_sig(p, L, s);
  launch_awr_fold_sig(p, a, sp.group_part, sp.L_fold, s);
}

// ---- what blsgpu_verify_same_message and blsgpu_aggregate_verify share ----------------------------------------
// (their messages are deduplicated and packed by unique_messages, run_plan.hpp.)  The three branches of such a call: signatures on the helper stream s, keys on sb, messages on sc (all s when
// `serial`: BLSGPU_SAME_SERIAL, diagnostics of the same-message call).  Device::same_st and same_ev are created by
// the first call that needs them.
struct Branches {
  hipStream_t s, sb, sc;
  bool serial;
  hipEvent_t* ev;
};
Branches branches(Device& d, hipStream_t s, bool serial) {
  if (!d.same_st[0]) {
    for (auto& e : d.same_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithFlags(&d.same_st[1], hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&d.same_st[0], hipStreamNonBlocking));
  }
  return Branches{s, serial ? s : d.same_st[0], serial ? s : d.same_st[1], serial, d.same_ev};
}
// Forks sb and sc from what s holds (the input copy), enqueues a on s, b on sb and c on sc, and joins both into s
template <class A, class B, class C>
void three_branches(const Branches& br, A a, B b, C c) {
  HIPCHK(hipEventRecord(br.ev[0], br.s));
  if (!br.serial) {
    HIPCHK(hipStreamWaitEvent(br.sb, br.ev[0], 0));
    HIPCHK(hipStreamWaitEvent(br.sc, br.ev[0], 0));
  }
  a(br.s);
  b(br.sb);
  HIPCHK(hipEventRecord(br.ev[1], br.sb));
  c(br.sc);
  HIPCHK(hipEventRecord(br.ev[2], br.sc));
  if (!br.serial) {
    HIPCHK(hipStreamWaitEvent(br.s, br.ev[1], 0));
    HIPCHK(hipStreamWaitEvent(br.s, br.ev[2], 0));
  }
}
// Runs body(sized); body sets `sized` once the call's buffers have their sizes, that is before its first launch.  On
// a HIP failure after that no branch may outlive the call -- the next helper call reuses, and may grow, the buffers
// they work on -- so all three streams are drained before the error goes on to helper_call.
template <class Body>
void drained_on_error(Device& d, Body body) {
  bool sized = false;
  try {
    body(sized);
  } catch (HipError&) {
    if (sized) {
      (void)hipStreamSynchronize(d.table_stream);
      for (hipStream_t x : d.same_st)
        if (x) (void)hipStreamSynchronize(x);
    }
    throw;
  }
}

// The message branch (pm: msg_branch, helper_buffers.hpp): H(m) affine (cooperative hashing for few messages, as small verification runs) and, for the lane forms, its lines
void launch_msg_branch(const PipelineBuffers& pm, bool lines, hipStream_t s) {
  launch_hash_to_g2(pm, s, pm.n_umsg <= 4096, false);
  launch_h_affine(pm, s);
  if (lines) launch_miller_lines2(pm, s);
}

// ---- one-call same-message verification (the host decisions are same_plan.hpp) ---------
// diagnostics (tools/bench_same_message.py): the three branches of the group phase on one stream
inline bool same_serial() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_SAME_SERIAL");
    return v && v[0] == '1';
  }();
  return on;
}
// The aggregate outputs of blsgpu_verify_same_message_agg; blsgpu_verify_same_message has none.
struct SameAggOut {
  const uint8_t* include;  // [n_sets], nullable
  uint8_t* out_sig;
  uint32_t out_sig_len;
  uint32_t* count;
};
// One same-message call on the device: its sizes and streams and where the group phase's fields lie (hl::Same).
struct SameCall {
  uint32_t G, n, flags, L;  // L: lanes of the randomized sums
  Branches br;
  PipelineBuffers pb, pm;  // the signature decode, the message branch
  AwrBuffers ab, ab_pk;    // the randomized sums S_g (ab.sum_sig) and P_g (ab.sum_pk; its own window scratch)
  AwrSplit split;          // how both run when the call is split into parts
  uint32_t *pk_aff, *inv, *F, *Gs;  // per group: the affine P_g, 1 / z of P_g, the Miller value, MillerLoop(-g1, S_g)
  uint8_t *inc, *ok;                // per group: include flag, verdict
  int8_t *code, *gres, *sres;       // per group: code, group_result; per set: set_result
  const uint32_t *gmsg, *iota;      // per group: message index; 0, 1, .., G
  bool lane(uint32_t n_items) const { return sp::form(n_items, flags) != 0; }
};
// Copies the call's inputs to d_in (hl::Same `l`) and says where everything of the group phase lies.
SameCall same_upload(Device& d, const Branches& br, const Grouped& a, uint32_t flags, const hl::Same& l,
                     const hl::AwrParts& lp, const awr_parts::Plan& ap, uint32_t lanes, const uint64_t* words,
                     const std::vector<uint8_t>& umsgs, const uint32_t* gmsg, const uint32_t* iota) {
  Slot& sl = d.helper;
  uint8_t* din = sl.d_in.p;
  uint8_t* db = sl.d_bytes.p;
  uint32_t* w = sl.d_work.p;
  const uint32_t G = a.G, U = (uint32_t)(umsgs.size() / 32);
  SameCall c{};
  c.G = G, c.n = a.n, c.flags = flags, c.L = ap.L, c.br = br;
  c.ab = same_inputs(d, a, l, db, words, lanes, br.s, c.pb);
  c.split = awr_split_upload(sl, lp, ap, c.ab, br.s);
  HIPCHK(hipMemcpyAsync(din + l.umsg, umsgs.data(), (size_t)U * 32, hipMemcpyHostToDevice, br.s));
  HIPCHK(hipMemcpyAsync(din + l.gmsg, gmsg, (size_t)G * 4, hipMemcpyHostToDevice, br.s));
  HIPCHK(hipMemcpyAsync(din + l.iota, iota, (size_t)(G + 1) * 4, hipMemcpyHostToDevice, br.s));
  c.ab_pk = c.ab;  // the G1 sum runs beside the G2 sum: its own window scratch
  c.ab_pk.tab = w + l.w_tab_pk;
  c.pm = msg_branch(sl, l.msg(), din + l.umsg, U, U, db + l.b_mf);
  c.pk_aff = w + l.w_pk_aff, c.inv = w + l.w_inv, c.F = w + l.w_F, c.Gs = w + l.w_G;
  c.inc = db + l.b_inc, c.ok = db + l.b_ok;
  c.code = reinterpret_cast<int8_t*>(db + l.b_code);
  c.gres = reinterpret_cast<int8_t*>(db + l.b_gres);
  c.sres = reinterpret_cast<int8_t*>(db + l.b_sres);
  c.gmsg = reinterpret_cast<uint32_t*>(din + l.gmsg);
  c.iota = reinterpret_cast<uint32_t*>(din + l.iota);
  return c;
}

// Miller values and checks of one phase, in two halves.  Miller half: item i < n_items pairs pk_aff[i] (W_G1A, stride
// n_items) with H(msg_idx[i]) when include[i], F_i (W_FP12, stride n_items).  iota = 0, 1, .., n_items: one item per
// Miller chunk.  Check half: ok[i] = FinalExp(F_i * MillerLoop(-g1, S_i)) == 1 with S (W_G2J, stride n_items).
// Cooperative form: k_miller_coop, and k_group_check with its own Miller loop.  Lane form: the messages' stored lines
// (pm.lines), k_miller_acc6 (six lanes per pairing), MillerLoop(-g1, S) on one lane per item (into Gs) and the final
// exponentiation on six (k_group_check6).
void same_miller_half(const PipelineBuffers& pm, uint32_t n_items, const uint32_t* iota, uint32_t* pk_aff,
                      uint8_t* include, const uint32_t* msg_idx, uint32_t* F, bool lane, hipStream_t s) {
  PipelineBuffers pb = pm;
  pb.n = n_items;
  pb.pk_aff = pk_aff;
  pb.include = include;
  pb.msg_idx = msg_idx;
  pb.n_chunks = n_items;
  pb.chunk_first = iota;
  pb.chunk_items = iota;
  pb.f_chunk = F;
  if (!lane)
    launch_miller_coop(pb, false, s, false);
  else
    launch_miller_acc6(pb, false, s);
}
void same_check_half(uint32_t n_items, const uint32_t* S, const uint32_t* F, uint32_t* Gs, uint8_t* ok, bool lane,
                     hipStream_t s) {
  if (!lane) {
    launch_group_check(S, F, n_items, ok, s);
  } else {
    launch_group_sig_miller(S, n_items, Gs, s, false, true);
    launch_group_check6(F, Gs, n_items, ok, s);
  }
}

// Group phase, first part: three branches from the input copy, joined into s, then every group's item.
void same_group_items(const SameCall& c) {
  three_branches(
      c.br,
      [&](hipStream_t s) {  // signatures: decode + subgroup check (cooperative for small calls), S_g
        launch_sig_decode(c.pb, c.n, s, c.n <= 4096, nullptr, false, true);
        awr_sum_sig(c.ab, c.split, c.L, s);
      },
      [&](hipStream_t sb) {  // keys: P_g and the batch inverses of its z
        awr_sum_pk(c.ab_pk, c.split, c.L, sb);
        launch_batch_inv(c.ab.sum_pk, c.G, 2 * W_FP, c.inv, c.G, sb);
      },
      [&](hipStream_t sc) {  // messages: H(m) affine, and in the lane form its Miller lines
        launch_msg_branch(c.pm, c.lane(c.G), sc);
      });
  launch_same_group_items(c.ab, c.inv, c.pk_aff, c.inc, c.code, c.br.s);
}
// Group phase without blocks: one pairing check per group.  Ends synchronized, group_result in h_grp.
void same_group_checks(const SameCall& c, int8_t* h_grp) {
  hipStream_t s = c.br.s;
  same_miller_half(c.pm, c.G, c.iota, c.pk_aff, c.inc, c.gmsg, c.F, c.lane(c.G), s);
  same_check_half(c.G, c.ab.sum_sig, c.F, c.Gs, c.ok, c.lane(c.G), s);
  launch_same_group_results(c.ab.group_first, c.G, c.n, c.inc, c.code, c.ok, c.sres, c.gres, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_grp, c.gres, c.G, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));  // every branch was joined into s: all three streams are idle
}
// Block phase: F_b, S_b per block of groups and one check per block.  S_b needs the sums and the
// include flags only: it runs on sb, beside the Miller loops, and is joined into s before the check.  Ends
// synchronized: h_any, h_ok per block, h_inc and h_grp per group.
void same_block_phase(const SameCall& c, Slot& sl, const hl::SameBlocks& lb, uint32_t NB, uint8_t* h_any,
                      uint8_t* h_ok, uint8_t* h_inc, int8_t* h_grp) {
  hipStream_t s = c.br.s, sb = c.br.sb;
  uint32_t* bw = sl.d_msmW.p;
  uint32_t* b_F = bw + lb.w_F;
  uint32_t* b_S = bw + lb.w_S;
  uint8_t* b_any = sl.d_res.p + lb.b_any;
  uint8_t* b_ok = sl.d_res.p + lb.b_ok;
  HIPCHK(hipEventRecord(c.br.ev[0], s));
  if (!c.br.serial) HIPCHK(hipStreamWaitEvent(sb, c.br.ev[0], 0));
  launch_same_block_sum(c.ab.sum_sig, c.inc, c.G, NB, b_S, b_any, sb);
  HIPCHK(hipEventRecord(c.br.ev[1], sb));
  same_miller_half(c.pm, c.G, c.iota, c.pk_aff, c.inc, c.gmsg, c.F, c.lane(c.G), s);
  launch_same_block_prod(c.F, c.inc, c.G, NB, bw + lb.w_T0, bw + lb.w_T1, b_F, s);
  if (!c.br.serial) HIPCHK(hipStreamWaitEvent(s, c.br.ev[1], 0));
  same_check_half(NB, b_S, b_F, bw + lb.w_G, b_ok, c.lane(NB), s);
  launch_same_block_results(c.ab.group_first, c.G, c.n, c.inc, c.code, b_any, b_ok, c.sres, c.gres, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_any, b_any, NB, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_ok, b_ok, NB, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_inc, c.inc, c.G, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_grp, c.gres, c.G, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));  // every branch was joined into s: all three streams are idle
}
// Descent: the listed groups (same_plan::descent_list), each checked from its own F_g, S_g in the descent's buffers
// (hl::SameBlocks `ld`).  Ends synchronized, h_grp rewritten.
void same_descent(const SameCall& c, Slot& sl, const hl::SameBlocks& ld, const std::vector<uint32_t>& listed,
                  int8_t* h_grp) {
  hipStream_t s = c.br.s;
  const uint32_t nl = (uint32_t)listed.size();
  uint32_t* dw = sl.d_fkeep.p;
  uint8_t* l_ok = sl.d_fbflags.p;
  HIPCHK(hipMemcpyAsync(dw + ld.d_list, listed.data(), (size_t)nl * 4, hipMemcpyHostToDevice, s));
  launch_same_gather(c.F, c.ab.sum_sig, c.G, dw + ld.d_list, nl, dw + ld.d_F, dw + ld.d_S, s);
  same_check_half(nl, dw + ld.d_S, dw + ld.d_F, dw + ld.d_G, l_ok, c.lane(nl), s);
  launch_same_descent_results(c.ab.group_first, c.G, c.n, dw + ld.d_list, nl, l_ok, c.sres, c.gres, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_grp, c.gres, c.G, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
}
// Retry phase: the listed sets (same_plan::retry_list), each on its own with r = 1, in the retry buffers (hl::SameRetry
// `r`; riota = 0, 1, .., nr).  build_lines: the lane forms' lines are not there yet.  Enqueued only.
// (the driver calls it after a synchronize: none of these is in use by an earlier phase)
void grow_retry_buffers(Slot& sl, const hl::SameRetry& r, bool lane) {
  sl.d_list.ensure(r.list_words);
  sl.d_ok.ensure(r.ok_bytes);
  sl.d_fb.ensure(r.fb_words);
  sl.d_S.ensure(r.S_words);
  sl.d_F.ensure(r.F_words);
  if (lane) sl.d_G.ensure(r.F_words);
}
void same_retry_phase(const SameCall& c, Slot& sl, const hl::SameRetry& r, const sp::Retry& rt,
                      const std::vector<uint32_t>& riota, bool build_lines) {
  hipStream_t s = c.br.s;
  const uint32_t nr = (uint32_t)rt.sets.size();
  const bool lane = c.lane(nr);
  uint32_t* dl = sl.d_list.p;
  HIPCHK(hipMemcpyAsync(dl, rt.sets.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dl + r.msg, rt.msg.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dl + r.iota, riota.data(), (size_t)(nr + 1) * 4, hipMemcpyHostToDevice, s));
  uint8_t* r_inc = sl.d_ok.p;
  int8_t* r_code = reinterpret_cast<int8_t*>(sl.d_ok.p + r.code);
  uint8_t* r_ok = sl.d_ok.p + r.ok;
  launch_same_retry_items(c.ab, dl, nr, sl.d_fb.p, sl.d_S.p, r_inc, r_code, s);
  if (build_lines) launch_miller_lines2(c.pm, s);
  same_miller_half(c.pm, nr, dl + r.iota, sl.d_fb.p, r_inc, dl + r.msg, sl.d_F.p, lane, s);
  same_check_half(nr, sl.d_S.p, sl.d_F.p, sl.d_G.p, r_ok, lane, s);
  launch_same_retry_results(dl, nr, r_inc, r_code, r_ok, c.sres, s);
  HIPCHK(hipGetLastError());
}
// Aggregate phase: each group's sum over the sets that answered 1, from the signatures decoded once, in the aggregate
// buffer `da` (hl::SameAgg `la`; the include bytes went up with the inputs).  Enqueued only.
void same_aggregate_phase(const SameCall& c, const hl::SameAgg& la, const SameAggOut& agg, uint8_t* da,
                          std::vector<uint8_t>& h_agg, std::vector<uint32_t>& h_cnt) {
  hipStream_t s = c.br.s;
  launch_same_agg(c.pb.sig_aff, c.n, c.sres, agg.include ? da + la.inc : nullptr, c.ab.group_first, c.G,
                  reinterpret_cast<uint32_t*>(da + la.sums), reinterpret_cast<uint32_t*>(da + la.count), da + la.out,
                  agg.out_sig_len, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_agg.data(), da + la.out, h_agg.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_cnt.data(), da + la.count, (size_t)c.G * 4, hipMemcpyDeviceToHost, s));
}

// What a same-message call brings back; it reaches the caller only on BLSGPU_OK
struct SameHost {
  std::vector<int8_t> set, grp;
  std::vector<uint8_t> agg;
  std::vector<uint32_t> cnt;
  blsgpu_same_message_stats st;
};
// The device side of both same-message verification calls, under helper_call: the driver of the phases above.  It
// shows what grows where, which host vectors live until the final synchronize, and when the Miller lines are built.
int same_message_on_device(Device& d, Slot& sl, hipStream_t s, const Grouped& a, const uint8_t* msgs, uint64_t seed,
                           uint32_t flags, const SameAggOut* agg, SameHost& h) {
  const uint32_t n = a.n, G = a.G;
  std::vector<uint64_t> words;
  uint64_t hash_key = 0;
  if (int e = same_begin(d, a, seed, words, hash_key)) return e;
  // group g signs unique message gmsg[g].  These host vectors are copied from: they live until the final synchronize
  std::vector<uint32_t> gmsg, iota((size_t)G + 1), listed, riota;
  const std::vector<uint8_t> umsgs = unique_messages(msgs, G, sp::msg_key(hash_key), gmsg);
  std::vector<uint8_t> h_blk, h_inc;  // (copied to)
  sp::Retry rt;                       // (rt.sets, rt.msg)
  const awr_parts::Plan ap = awr_parts::plan(a.group_first, G);  // (ap.part_first, ap.group_part)
  for (uint32_t g = 0; g <= G; g++) iota[g] = g;
  const uint32_t U = (uint32_t)(umsgs.size() / 32);
  h.st.unique_messages = U;
  drained_on_error(d, [&](bool& sized) {
    const Branches br = branches(d, s, same_serial());
    const auto t0 = std::chrono::steady_clock::now();
    const bool lane_g = sp::form(G, flags) != 0;
    const uint32_t lanes = awr_launch_lanes(ap.n_parts, ap.L);  // (n_parts = G unless the call is split)
    const hl::Same l(G, n, U, a.sig_stride, a.pk_bytes != nullptr, lanes);
    const hl::AwrParts lp(G, ap.n_parts);
    // every buffer of the group phase grows here, while none of the three streams has work (each call ends with all
    // of them synchronized); the retry phase grows only buffers the group phase does not use, after its synchronize
    sl.d_in.ensure(l.in_total);
    sl.d_bytes.ensure(l.bytes_total);
    sl.d_work.ensure(l.work_words);
    if (lane_g) sl.d_lines.ensure(l.lines_words);
    if (ap.split()) sl.d_parts.ensure(lp.total_words);
    // BLSGPU_SAME_BLOCK_CHECK: the block phase's buffers grow here too; the descent's, like the retry phase's, after
    // the synchronize before it, and they are buffers no other phase uses
    const uint32_t NB = sp::blocks(G, flags);
    const hl::SameBlocks lb(NB, NB ? same_block_tree_width(G) : 0, 0);
    if (NB) {
      sl.d_msmW.ensure(lb.work_words);
      sl.d_res.ensure(lb.bytes_total);
    }
    // the aggregate phase's buffer too: one no other phase of the call uses
    const hl::SameAgg la(G, n, agg ? agg->out_sig_len : 0);
    if (agg) sl.d_msmB.ensure(la.total_words);
    sized = true;
    SameCall c = same_upload(d, br, a, flags, l, lp, ap, lanes, words.data(), umsgs, gmsg.data(), iota.data());
    uint8_t* da = agg ? reinterpret_cast<uint8_t*>(sl.d_msmB.p) : nullptr;
    if (agg && agg->include && n) HIPCHK(hipMemcpyAsync(da + la.inc, agg->include, n, hipMemcpyHostToDevice, s));
    same_group_items(c);
    const bool have_lines = lane_g;  // the message branch builds the Miller lines only for a lane-form group phase
    if (!NB) {
      same_group_checks(c, h.grp.data());
    } else {
      h_blk.resize(2 * (size_t)NB), h_inc.resize(G);  // any | ok per block; include per group
      same_block_phase(c, sl, lb, NB, h_blk.data(), h_blk.data() + NB, h_inc.data(), h.grp.data());
      h.st.form |= sp::kFormBlocks;
      listed = sp::descent_list(G, NB, h_blk.data(), h_blk.data() + NB, h_inc.data());
      if (const uint32_t nl = (uint32_t)listed.size()) {
        const hl::SameBlocks ld(NB, 0, nl);
        sl.d_fkeep.ensure(ld.descent_words);
        sl.d_fbflags.ensure(ld.d_ok_bytes);
        same_descent(c, sl, ld, listed, h.grp.data());
        h.st.form |= c.lane(nl) ? sp::kFormDescent | sp::kFormDescentLane : sp::kFormDescent;
      }
    }
    if (lane_g) h.st.form |= sp::kFormGroupLane;
    rt = sp::retry_list(a.group_first, G, h.grp.data(), gmsg.data());
    const uint32_t nr = (uint32_t)rt.sets.size();
    h.st.groups_accepted = rt.groups_accepted;
    h.st.groups_retried = rt.groups_retried;
    h.st.retry_sets = nr;
    if (nr) {
      // after a synchronize of all three streams, and buffers the earlier phases do not use -- but for d_lines, which
      // grows only when the group phase left it unused
      const bool lane_r = c.lane(nr);
      const hl::SameRetry r(nr);
      grow_retry_buffers(sl, r, lane_r);
      if (lane_r && !have_lines) {
        sl.d_lines.ensure(l.lines_words);
        c.pm.lines = sl.d_lines.p;
      }
      riota.resize((size_t)nr + 1);
      for (uint32_t q = 0; q <= nr; q++) riota[q] = q;
      same_retry_phase(c, sl, r, rt, riota, lane_r && !have_lines);
      if (lane_r) h.st.form |= sp::kFormRetryLane;
    }
    if (agg) same_aggregate_phase(c, la, *agg, da, h.agg, h.cnt);
    if (n) HIPCHK(hipMemcpyAsync(h.set.data(), c.sres, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    h.st.device_ms = ms_since(t0);
  });
  return BLSGPU_OK;
}

// Both same-message verification calls.  agg null: blsgpu_verify_same_message, which launches what it always
// launched.  Else the aggregate phase follows the retry phase.
int verify_same_message(blsgpu_ctx* ctx, uint32_t n_groups, const uint32_t* group_first, const uint8_t* msgs,
                        const uint8_t* pk_bytes, const uint32_t* pk_index, const uint8_t* sigs, uint32_t sig_stride,
                        const uint32_t* sig_len, uint64_t seed, uint32_t flags, int8_t* set_result,
                        int8_t* group_result, blsgpu_same_message_stats* stats, const SameAggOut* agg) {
  if (!ctx || ctx->devs.empty() || !group_first || !msgs || !sigs || !sig_len || !set_result) return BLSGPU_ERR_ARGS;
  if ((pk_bytes != nullptr) == (pk_index != nullptr)) return BLSGPU_ERR_ARGS;
  if (sig_stride < 96 || (flags & ~(BLSGPU_SAME_LANE_FORMS | BLSGPU_SAME_BLOCK_CHECK))) return BLSGPU_ERR_ARGS;
  if (agg && (agg->out_sig_len != 96 && agg->out_sig_len != 192)) return BLSGPU_ERR_ARGS;
  if (agg && n_groups && (!agg->out_sig || !agg->count)) return BLSGPU_ERR_ARGS;
  if (n_groups == 0) {
    if (stats) memset(stats, 0, sizeof *stats);
    return BLSGPU_OK;
  }
  Grouped a{n_groups, group_first, sigs, sig_stride, sig_len, pk_bytes, pk_index};
  if (int e = check_group_layout(a)) return e;
  const uint32_t n = a.n, G = n_groups;
  SameHost h;
  h.set.resize(n), h.grp.resize(G), h.agg.resize(agg ? (size_t)G * agg->out_sig_len : 0), h.cnt.resize(agg ? G : 0);
  memset(&h.st, 0, sizeof h.st);
  const int rc = helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    return same_message_on_device(d, sl, s, a, msgs, seed, flags, agg, h);
  });
  if (rc == BLSGPU_OK) {  // results reach the caller only when every one of them was computed
    if (n) memcpy(set_result, h.set.data(), n);
    if (group_result) memcpy(group_result, h.grp.data(), G);
    if (stats) *stats = h.st;
    if (agg) {
      memcpy(agg->out_sig, h.agg.data(), h.agg.size());
      memcpy(agg->count, h.cnt.data(), (size_t)G * 4);
    }
  }
  return rc;
}

// ---- batched AggregateVerify -----------------------------------------------------------------------------------
// A job's signature is one more pair of the job, (-g1, sig): k pairs are k + 1 Miller items in the job's own
// accumulators and one final exponentiation (aggverify_plan.hpp, k_aggverify.hip).
// (its inputs AvArgs and where everything lies, AvCall, are helper_buffers.hpp.)
// Copies the call's inputs and its plan to d_in (hl::AggVerify `l`)
void av_upload(Slot& sl, const hl::AggVerify& l, const AvArgs& a, const avp::Plan& plan,
               const std::vector<uint8_t>& umsgs, const uint32_t* pmsg, hipStream_t s) {
  uint8_t* din = sl.d_in.p;
  const uint32_t J = a.J, C = plan.n_chunks();
  HIPCHK(hipMemcpyAsync(din + l.gf, a.job_first, (size_t)(J + 1) * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(din + l.len, a.sig_len, (size_t)J * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(din + l.sigs, a.sigs, (size_t)J * a.sig_stride, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(din + l.fr, plan.f_ranges.data(), (size_t)2 * J * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(din + l.cf, plan.chunk_first.data(), (size_t)(C + 1) * 4, hipMemcpyHostToDevice, s));
  if (!plan.chunk_items.empty())
    HIPCHK(hipMemcpyAsync(din + l.ci, plan.chunk_items.data(), plan.chunk_items.size() * 4, hipMemcpyHostToDevice, s));
  if (a.n) {
    HIPCHK(hipMemcpyAsync(din + l.keys, a.pk_bytes ? (const void*)a.pk_bytes : (const void*)a.pk_index, l.key_bytes,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.umsg, umsgs.data(), umsgs.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.pmsg, pmsg, (size_t)a.n * 4, hipMemcpyHostToDevice, s));
  }
}
// Three branches from the input copy, joined into s, then every job's signature item
void av_items(Slot& sl, const Branches& br, const hl::AggVerify& l, const AvArgs& a, const AvCall& c, bool lane) {
  three_branches(
      br,
      [&](hipStream_t s) {  // signatures: decode + subgroup check (cooperative for small calls)
        launch_sig_decode(c.pb, a.J, s, a.J <= 4096, nullptr, false, true);
      },
      [&](hipStream_t sb) {  // keys: KeyValidate when they are untrusted, then every pair's affine point and code
        if (a.validate())
          launch_key_validate(sl.d_in.p + l.keys, a.n, a.pk_len, a.pk_len, sl.d_in.p + l.kv96,
                              reinterpret_cast<int8_t*>(sl.d_bytes.p + l.b_kv), sb);
        launch_av_pair_items(c.av, sb);
      },
      [&](hipStream_t sc) {  // messages: H(m) affine, and in the lane form the Miller lines of those columns
        launch_msg_branch(c.pm, lane, sc);
      });
  launch_av_job_items(c.av, br.s);
}
// Accumulate, reduce to F_j, check and write the results to d_res (enqueued only)
void av_check(Slot& sl, const hl::AggVerify& l, const avp::CallPlan& p, const AvCall& c, int8_t* d_res,
              hipStream_t s) {
  const uint32_t J = c.av.n_jobs, U = c.av.n_umsg;
  uint32_t* F = sl.d_work.p + l.w_F;
  uint8_t* d_ok = sl.d_bytes.p + l.b_ok;
  const uint32_t* d_fr = reinterpret_cast<uint32_t*>(sl.d_in.p + l.fr);
  if (!p.lane) {
    launch_miller_coop(c.px, false, s, false);
  } else {
    // the signature columns' lines: columns U .. M - 1, addressed as a call of J columns in the same arrays
    PipelineBuffers ps = c.pm;
    ps.n_umsg = J;
    ps.h_aff = c.pm.h_aff + U;
    ps.mflags = c.pm.mflags + U;
    ps.lines = c.pm.lines + U;
    launch_miller_lines2(ps, s);
    launch_miller_acc(c.px, false, s);
  }
  if (p.lane_reduce)
    launch_av_reduce_lane(c.px.f_chunk, c.px.n, d_fr, J, F, s);
  else
    launch_group_reduce(c.px, d_fr, J, F, s);
  launch_av_check(F, J, c.av.checked, d_ok, p.lane, s);
  launch_av_results(J, c.av.job_code, c.av.checked, d_ok, d_res, s);
  HIPCHK(hipGetLastError());
}

}  // namespace

extern "C" {

int blsgpu_aggregate_pubkeys(blsgpu_ctx* ctx, const blsgpu_batch* b, uint8_t* out, uint32_t out_len,
                             int8_t* status) {
  if (!ctx || ctx->devs.empty() || !b || !out || !status || (out_len != 48 && out_len != 96)) return BLSGPU_ERR_ARGS;
  const uint32_t n = b->n_sets;
  if (n == 0) return BLSGPU_OK;
  if (!b->pk_bytes && (!b->set_pk_first || !b->pk_index)) return BLSGPU_ERR_ARGS;
  return helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    // (set_pk_first: a synthetic 1-key-per-set layout in single-key bytes mode)
    std::vector<uint32_t> spf(n + 1);
    for (uint32_t i = 0; i <= n; i++) spf[i] = b->set_pk_first ? b->set_pk_first[i] : i;
    const uint32_t npk = spf[n];
    if (!b->pk_bytes)
      for (uint32_t k = 0; k < npk; k++)
        if (b->pk_index[k] >= d.table_n) return BLSGPU_ERR_ARGS;
    const hl::AggPubkeys l(n, npk, b->pk_bytes != nullptr, out_len);
    sl.d_in.ensure(l.total);
    sl.d_work.ensure(l.work_words);
    uint8_t* din = sl.d_in.p;
    HIPCHK(hipMemcpyAsync(din + l.spf, spf.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.keys, b->pk_bytes ? (const void*)b->pk_bytes : (const void*)b->pk_index,
                          l.key_bytes, hipMemcpyHostToDevice, s));
    PipelineBuffers pb{};
    pb.n = n;
    pb.set_pk_first = reinterpret_cast<uint32_t*>(din + l.spf);
    pb.pk_bytes = b->pk_bytes ? din + l.keys : nullptr;
    pb.pk_index = b->pk_bytes ? nullptr : reinterpret_cast<uint32_t*>(din + l.keys);
    pb.pk_table = d.table.p;
    pb.pk_table_n = d.table_n;
    pb.pk_jac = sl.d_work.p;
    pb.status = reinterpret_cast<int8_t*>(din + l.st);
    launch_pk_aggregate(pb, n, s);
    launch_pk_serialize(pb, n, din + l.out, out_len, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, din + l.out, (size_t)n * out_len, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, din + l.st, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSGPU_OK;
  });
}

int blsgpu_aggregate_signatures(blsgpu_ctx* ctx, uint32_t n_groups, const uint32_t* group_first,
                                const uint8_t* sigs, uint32_t sig_stride, const uint32_t* sig_len, uint32_t flags,
                                uint8_t* out, uint32_t out_len, int8_t* status, uint32_t* first_bad) {
  if (!ctx || ctx->devs.empty() || !group_first || !sigs || !sig_len || !out || !status) return BLSGPU_ERR_ARGS;
  if ((out_len != 96 && out_len != 192) || sig_stride < 96 || (flags & ~BLSGPU_AGG_VALIDATE)) return BLSGPU_ERR_ARGS;
  if (n_groups == 0) return BLSGPU_OK;
  Grouped a{n_groups, group_first, sigs, sig_stride, sig_len};
  if (int e = check_group_layout(a)) return e;
  const uint32_t n = a.n, G = n_groups;
  return helper_call(ctx, false, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    const hl::AggSigs l(G, n, sig_stride, out_len);
    sl.d_in.ensure(l.total);
    sl.d_work.ensure(l.work_words);
    uint8_t* din = sl.d_in.p;
    const PipelineBuffers pb = sig_inputs(sl, a, l, din + l.fl, din + l.st, s);
    const uint32_t* d_first = reinterpret_cast<uint32_t*>(din + l.gf);
    uint32_t* agg = sl.d_work.p + l.w_agg;
    int8_t* d_gst = reinterpret_cast<int8_t*>(din + l.gst);
    uint32_t* d_fb = reinterpret_cast<uint32_t*>(din + l.fb);
    // small calls (the pool insert) take the cooperative subgroup check, as small verification runs do
    launch_sig_decode(pb, n, s, n <= 4096, nullptr, false, (flags & BLSGPU_AGG_VALIDATE) != 0);
    launch_sig_aggregate(pb, d_first, G, n, agg, d_gst, d_fb, s);
    launch_sig_agg_serialize(d_first, G, agg, d_gst, din + l.out, out_len, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, din + l.out, (size_t)G * out_len, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, din + l.gst, G, hipMemcpyDeviceToHost, s));
    if (first_bad) HIPCHK(hipMemcpyAsync(first_bad, din + l.fb, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSGPU_OK;
  });
}

uint32_t blsgpu_sig_agg_lanes(uint32_t n_groups, uint32_t n_sigs) { return sig_agg_lanes(n_groups, n_sigs); }

int blsgpu_randomness_words(uint32_t n, uint64_t seed, uint64_t* words) {
  if (n && !words) return BLSGPU_ERR_ARGS;
  batch_rand::Key key;
  uint64_t hash_key = 0;
  if (!resolve_key(seed, key, hash_key)) return BLSGPU_ERR_ENTROPY;
  batch_rand::words(key, 0, n, words);
  return BLSGPU_OK;
}

int blsgpu_aggregate_with_randomness(blsgpu_ctx* ctx, uint32_t n_groups, const uint32_t* group_first,
                                     const uint8_t* pk_bytes, const uint32_t* pk_index, const uint8_t* sigs,
                                     uint32_t sig_stride, const uint32_t* sig_len, uint64_t seed, uint8_t* out_pk,
                                     uint32_t out_pk_len, uint8_t* out_sig, uint32_t out_sig_len, int8_t* status,
                                     uint32_t* first_bad) {
  if (!ctx || ctx->devs.empty() || !group_first || !sigs || !sig_len || !out_pk || !out_sig || !status)
    return BLSGPU_ERR_ARGS;
  if ((pk_bytes != nullptr) == (pk_index != nullptr)) return BLSGPU_ERR_ARGS;
  if ((out_pk_len != 48 && out_pk_len != 96) || (out_sig_len != 96 && out_sig_len != 192) || sig_stride < 96)
    return BLSGPU_ERR_ARGS;
  if (n_groups == 0) return BLSGPU_OK;
  Grouped a{n_groups, group_first, sigs, sig_stride, sig_len, pk_bytes, pk_index};
  if (int e = check_group_layout(a)) return e;
  const uint32_t n = a.n, G = n_groups;
  const awr_parts::Plan ap = awr_parts::plan(group_first, G);  // copied from: it lives until the final synchronize
  return helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    std::vector<uint64_t> words;
    uint64_t hash_key = 0;
    if (int e = same_begin(d, a, seed, words, hash_key)) return e;
    const uint32_t L = ap.L, lanes = awr_launch_lanes(ap.n_parts, L);  // (n_parts = G unless the call is split)
    const hl::Awr l(G, n, sig_stride, pk_bytes != nullptr, out_pk_len, out_sig_len, lanes);
    const hl::AwrParts lp(G, ap.n_parts);
    sl.d_in.ensure(l.total);
    sl.d_work.ensure(l.work_words);
    if (ap.split()) sl.d_parts.ensure(lp.total_words);
    uint8_t* din = sl.d_in.p;
    PipelineBuffers pb;
    const AwrBuffers ab = same_inputs(d, a, l, din, words.data(), lanes, s, pb);
    const AwrSplit split = awr_split_upload(sl, lp, ap, ab, s);
    int8_t* d_gst = reinterpret_cast<int8_t*>(din + l.gst);
    uint32_t* d_fb = reinterpret_cast<uint32_t*>(din + l.fb);
    // small calls take the cooperative subgroup check, as small verification runs do
    launch_sig_decode(pb, n, s, n <= 4096, nullptr, false, true);
    awr_sum_pk(ab, split, L, s);
    awr_sum_sig(ab, split, L, s);
    launch_awr_serialize(ab, din + l.opk, out_pk_len, din + l.osig, out_sig_len, d_gst, d_fb, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_pk, din + l.opk, (size_t)G * out_pk_len, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_sig, din + l.osig, (size_t)G * out_sig_len, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, din + l.gst, G, hipMemcpyDeviceToHost, s));
    if (first_bad) HIPCHK(hipMemcpyAsync(first_bad, din + l.fb, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSGPU_OK;
  });
}

uint32_t blsgpu_awr_lanes(uint32_t n_groups, uint32_t n_sets) { return awr_lanes(n_groups, n_sets); }

int blsgpu_awr_parts(uint32_t n_groups, const uint32_t* group_first, uint32_t* part_sets, uint32_t* n_parts,
                     uint32_t* part_first) {
  if ((n_groups && !group_first) || !part_sets || !n_parts) return BLSGPU_ERR_ARGS;
  uint32_t n = 0;
  if (n_groups)  // (a call of no groups is accepted before its group_first is read, as the calls described accept it)
    if (int e = check_offsets(group_first, n_groups, n)) return e;
  const awr_parts::Plan ap = awr_parts::plan(group_first, n_groups);
  *part_sets = ap.part_sets;
  *n_parts = ap.n_parts;
  if (part_first) {
    const uint32_t* src = ap.split() ? ap.part_first.data() : group_first;
    if (n_groups) memcpy(part_first, src, ((size_t)ap.n_parts + 1) * 4);
    else part_first[0] = 0;
  }
  return BLSGPU_OK;
}

// ---- one-call same-message verification: the rules are same_plan.hpp, the phases and their driver are above
uint32_t blsgpu_same_message_form(uint32_t n_items, uint32_t flags) { return sp::form(n_items, flags); }
uint32_t blsgpu_same_message_blocks(uint32_t n_groups, uint32_t flags) { return sp::blocks(n_groups, flags); }

int blsgpu_verify_same_message(blsgpu_ctx* ctx, uint32_t n_groups, const uint32_t* group_first, const uint8_t* msgs,
                               const uint8_t* pk_bytes, const uint32_t* pk_index, const uint8_t* sigs,
                               uint32_t sig_stride, const uint32_t* sig_len, uint64_t seed, uint32_t flags,
                               int8_t* set_result, int8_t* group_result, blsgpu_same_message_stats* stats) {
  return verify_same_message(ctx, n_groups, group_first, msgs, pk_bytes, pk_index, sigs, sig_stride, sig_len, seed,
                             flags, set_result, group_result, stats, nullptr);
}

int blsgpu_verify_same_message_agg(blsgpu_ctx* ctx, uint32_t n_groups, const uint32_t* group_first,
                                   const uint8_t* msgs, const uint8_t* pk_bytes, const uint32_t* pk_index,
                                   const uint8_t* sigs, uint32_t sig_stride, const uint32_t* sig_len, uint64_t seed,
                                   uint32_t flags, int8_t* set_result, int8_t* group_result,
                                   blsgpu_same_message_stats* stats, const uint8_t* agg_include, uint8_t* out_sig,
                                   uint32_t out_sig_len, uint32_t* agg_count) {
  const SameAggOut agg{agg_include, out_sig, out_sig_len, agg_count};
  return verify_same_message(ctx, n_groups, group_first, msgs, pk_bytes, pk_index, sigs, sig_stride, sig_len, seed,
                             flags, set_result, group_result, stats, &agg);
}

uint32_t blsgpu_same_message_agg_lanes(uint32_t n_groups, uint32_t n_sets) { return sig_agg_lanes(n_groups, n_sets); }

// ---- batched AggregateVerify: argument checks, plan, buffers, three branches, checks, stats
uint32_t blsgpu_aggregate_verify_form(uint32_t n_items, uint32_t flags) {
  return avp::form(n_items, (flags & BLSGPU_AV_LANE_FORMS) != 0);
}

int blsgpu_aggregate_verify(blsgpu_ctx* ctx, uint32_t n_jobs, const uint32_t* job_first, const uint8_t* msgs,
                            const uint8_t* pk_bytes, uint32_t pk_len, const uint32_t* pk_index, const uint8_t* sigs,
                            uint32_t sig_stride, const uint32_t* sig_len, uint32_t flags, int8_t* job_result,
                            uint32_t* first_bad, blsgpu_aggregate_verify_stats* stats) {
  if (!ctx || ctx->devs.empty() || !job_first || !msgs || !sigs || !sig_len || !job_result) return BLSGPU_ERR_ARGS;
  if ((pk_bytes != nullptr) == (pk_index != nullptr)) return BLSGPU_ERR_ARGS;
  if (sig_stride < 96 || (flags & ~(BLSGPU_AV_VALIDATE_KEYS | BLSGPU_AV_LANE_FORMS))) return BLSGPU_ERR_ARGS;
  const bool validate = (flags & BLSGPU_AV_VALIDATE_KEYS) != 0;
  if (validate ? (!pk_bytes || (pk_len != 48 && pk_len != 96)) : (pk_bytes && pk_len != 96)) return BLSGPU_ERR_ARGS;
  if (n_jobs == 0) {
    if (stats) memset(stats, 0, sizeof *stats);
    return BLSGPU_OK;
  }
  if (n_jobs > (1u << 20)) return BLSGPU_ERR_ARGS;  // (before job_first is read)
  AvArgs a{n_jobs, 0, job_first, pk_bytes, pk_len, pk_index, sigs, sig_stride, sig_len, flags};
  if (int e = check_offsets(job_first, n_jobs, a.n)) return e;
  if (int e = check_sig_lens(sig_len, n_jobs, sig_stride)) return e;
  const uint32_t J = n_jobs, n = a.n;
  std::vector<int8_t> h_res(J);
  std::vector<uint32_t> h_fb(J);
  std::vector<uint8_t> h_chk(J);
  blsgpu_aggregate_verify_stats st;
  memset(&st, 0, sizeof st);
  const int rc = helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    if (pk_index)
      for (uint32_t k = 0; k < n; k++)
        if (pk_index[k] >= d.table_n) return BLSGPU_ERR_ARGS;
    // messages, deduplicated over the whole call: pair k signs unique message pmsg[k]
    std::vector<uint32_t> pmsg;
    const std::vector<uint8_t> umsgs = unique_messages(msgs, n, avp::kMsgKey, pmsg);
    const uint32_t U = (uint32_t)(umsgs.size() / 32);
    const avp::CallPlan p = avp::plan_call(job_first, J, a.lane_flag());
    st.pairs = n;
    st.unique_messages = U;
    st.form = p.lane ? 1 : 0;
    drained_on_error(d, [&](bool& sized) {
      const Branches br = branches(d, s, false);
      const auto t0 = std::chrono::steady_clock::now();
      const hl::AggVerify l(J, n, U, p.n_chunks, sig_stride, pk_bytes != nullptr, pk_len, validate);
      // every buffer grows here, while none of the three streams has work (each call ends with all of them synchronized)
      sl.d_in.ensure(l.in_total);
      sl.d_bytes.ensure(l.bytes_total);
      sl.d_work.ensure(l.work_words);
      if (p.lane) sl.d_lines.ensure(l.lines_words);
      sized = true;
      av_upload(sl, l, a, p.plan, umsgs, pmsg.data(), s);
      const AvCall c = av_buffers(d, l, a, U, p.n_chunks);
      int8_t* d_res = reinterpret_cast<int8_t*>(sl.d_bytes.p + l.b_res);
      av_items(sl, br, l, a, c, p.lane);
      av_check(sl, l, p, c, d_res, s);
      HIPCHK(hipMemcpyAsync(h_res.data(), d_res, J, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(h_fb.data(), c.av.first_bad, (size_t)J * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(h_chk.data(), c.av.checked, J, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));  // every branch was joined into s: all three streams are idle
      st.device_ms = ms_since(t0);
    });
    const avp::Counts done = avp::count(job_first, J, h_chk.data(), p.k);
    st.jobs_checked = done.jobs;
    st.miller_items = done.items;
    st.miller_chunks = done.chunks;
    return BLSGPU_OK;
  });
  if (rc == BLSGPU_OK) {  // results reach the caller only when every one of them was computed
    memcpy(job_result, h_res.data(), J);
    if (first_bad) memcpy(first_bad, h_fb.data(), (size_t)J * 4);
    if (stats) *stats = st;
  }
  return rc;
}

int blsgpu_key_validate(blsgpu_ctx* ctx, uint32_t n, const uint8_t* pks, uint32_t pk_len, uint32_t stride,
                        uint8_t* out96, int8_t* status) {
  if (!ctx || ctx->devs.empty() || !pks || !status || stride < pk_len) return BLSGPU_ERR_ARGS;
  if (pk_len != 48 && pk_len != 96) return BLSGPU_ERR_ARGS;
  if (n == 0) return BLSGPU_OK;
  return helper_call(ctx, false, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    const hl::KeyValidate l(n, stride);
    sl.d_in.ensure(l.total);
    uint8_t* din = sl.d_in.p;
    HIPCHK(hipMemcpyAsync(din, pks, (size_t)n * stride, hipMemcpyHostToDevice, s));
    launch_key_validate(din, n, pk_len, stride, din + l.out, reinterpret_cast<int8_t*>(din + l.st), s);
    HIPCHK(hipGetLastError());
    if (out96) HIPCHK(hipMemcpyAsync(out96, din + l.out, (size_t)n * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, din + l.st, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSGPU_OK;
  });
}

int blsgpu_pubkeys_read(blsgpu_ctx* ctx, uint32_t first_index, uint32_t n, uint8_t* out, uint32_t out_len) {
  if (!ctx || ctx->devs.empty() || (out_len != 48 && out_len != 96)) return BLSGPU_ERR_ARGS;
  if (n == 0) return BLSGPU_OK;
  if (!out) return BLSGPU_ERR_ARGS;
  return helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    if ((uint64_t)first_index + n > d.table_n) return BLSGPU_ERR_ARGS;
    const hl::PubkeysRead l(n, out_len);
    sl.d_in.ensure(l.total);
    uint8_t* din = sl.d_in.p;
    launch_pk_table_read(d.table.p, first_index, n, din + l.out, out_len, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, din + l.out, (size_t)n * out_len, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSGPU_OK;
  });
}

// ---- the committee store and the aggregation from participation bits (the host decisions are
// committee_plan.hpp, the kernels k_committee.hip)
uint32_t blsgpu_committees_count(const blsgpu_ctx* ctx) {
  if (!ctx || ctx->devs.empty()) return 0;
  Device& d = *ctx->devs[0];
  std::shared_lock<std::shared_mutex> lk(d.table_mu);
  return d.cm_n;
}

int blsgpu_committees_upload(blsgpu_ctx* ctx, uint32_t first_committee, uint32_t n, const uint32_t* committee_first,
                             const uint32_t* members) {
  if (!ctx || ctx->devs.empty()) return BLSGPU_ERR_ARGS;
  if (!enter(ctx)) return BLSGPU_ERR_CLOSED;
  struct Leave {
    blsgpu_ctx* ctx;
    ~Leave() { leave(ctx); }
  } leave_on_exit{ctx};
  Device& d = *ctx->devs[0];
  try {
    // the helper lock for table_stream, the table lock exclusively: no bits call reads the store meanwhile
    std::lock_guard<std::mutex> helper(d.helper_mu);
    std::unique_lock<std::shared_mutex> tl(d.table_mu);
    if (cmp::check_upload(first_committee, n, committee_first, members, d.cm_n, d.table_n)) return BLSGPU_ERR_ARGS;
    HIPCHK(hipSetDevice(d.id));
    hipStream_t s = d.table_stream;
    // truncate; a HIP failure below leaves the store so
    d.cm_n = first_committee;
    d.cm_first_host.resize((size_t)first_committee + 1, 0);
    if (n == 0) return BLSGPU_OK;
    const uint32_t base = d.cm_first_host[first_committee], total = committee_first[n], count = first_committee + n;
    // (entry first_committee of cm_first is rewritten below with the rest: the kept part ends before it)
    grow_keeping(d.cm_first, first_committee, (size_t)count + 1, s);
    grow_keeping(d.cm_members, base, (size_t)base + total, s);
    grow_keeping(d.cm_sums, (size_t)first_committee * W_CSUM, (size_t)count * W_CSUM, s);
    std::vector<uint32_t> first((size_t)n + 1);  // copied from: lives until the synchronize
    for (uint32_t c = 0; c <= n; c++) first[c] = base + committee_first[c];
    HIPCHK(hipMemcpyAsync(d.cm_first.p + first_committee, first.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.cm_members.p + base, members, (size_t)total * 4, hipMemcpyHostToDevice, s));
    launch_committee_sums(committee_store(d), first_committee, n, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    d.cm_first_host.insert(d.cm_first_host.end(), first.begin() + 1, first.end());
    d.cm_n = count;
    return BLSGPU_OK;
  } catch (HipError&) {
    return BLSGPU_DEVICE_ERROR;
  }
}

uint32_t blsgpu_committee_bits_mode(uint32_t size, uint32_t present, uint32_t flags) {
  return cmp::mode(size, present, flags);
}
uint32_t blsgpu_committee_bits_lanes(uint32_t n_sets, uint32_t n_items) { return cmp::lanes(n_sets, n_items); }

int blsgpu_aggregate_pubkeys_bits(blsgpu_ctx* ctx, uint32_t n_sets, const uint32_t* set_seg_first,
                                  const uint32_t* seg_committee, const uint32_t* set_bits_first, const uint8_t* bits,
                                  uint32_t flags, uint8_t* out, uint32_t out_len, int8_t* status,
                                  blsgpu_committee_bits_stats* stats) {
  if (!ctx || ctx->devs.empty()) return BLSGPU_ERR_ARGS;
  if (cmp::check_call(n_sets, set_seg_first, seg_committee, set_bits_first, bits, flags, out, out_len, status))
    return BLSGPU_ERR_ARGS;
  if (n_sets == 0) {
    if (stats) memset(stats, 0, sizeof *stats);
    return BLSGPU_OK;
  }
  const uint32_t n = n_sets;
  std::vector<uint8_t> h_out((size_t)n * out_len);  // results reach the caller only when every one was computed
  std::vector<int8_t> h_st(n);
  blsgpu_committee_bits_stats st{};
  const int rc = helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    cmp::Plan p;  // (copied from: lives until the synchronize)
    if (cmp::make_plan(n, set_seg_first, seg_committee, set_bits_first, bits, flags, d.cm_first_host.data(), d.cm_n, p))
      return BLSGPU_ERR_ARGS;
    const auto t0 = std::chrono::steady_clock::now();
    const hl::AggPubkeysBits l(n, p.n_segs, p.bits_bytes, out_len);
    sl.d_in.ensure(l.total);
    sl.d_work.ensure(l.work_words);
    uint8_t* din = sl.d_in.p;
    HIPCHK(hipMemcpyAsync(din + l.ssf, set_seg_first, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.sbf, set_bits_first, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.present, p.present_first.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    if (p.n_segs) HIPCHK(hipMemcpyAsync(din + l.seg, p.seg_desc.data(), (size_t)p.n_segs * 4, hipMemcpyHostToDevice, s));
    if (p.bits_bytes) HIPCHK(hipMemcpyAsync(din + l.bits, bits, p.bits_bytes, hipMemcpyHostToDevice, s));
    CommitteeBits a{};
    a.n_sets = n;
    a.set_seg_first = reinterpret_cast<uint32_t*>(din + l.ssf);
    a.seg_desc = reinterpret_cast<uint32_t*>(din + l.seg);
    a.set_bits_first = reinterpret_cast<uint32_t*>(din + l.sbf);
    a.bits = din + l.bits;
    a.pk_jac = sl.d_work.p;
    a.status = reinterpret_cast<int8_t*>(din + l.st);
    launch_pk_bits(committee_store(d), a, p.counts.lanes, s);
    // k_pk_serialize as blsgpu_aggregate_pubkeys runs it: a set's keys are its set bits (EMPTY_AGGREGATE for none)
    PipelineBuffers pb{};
    pb.n = n;
    pb.set_pk_first = reinterpret_cast<uint32_t*>(din + l.present);
    pb.pk_jac = a.pk_jac;
    pb.status = a.status;
    launch_pk_serialize(pb, n, din + l.out, out_len, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out.data(), din + l.out, h_out.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_st.data(), din + l.st, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const cmp::Counts& c = p.counts;
    st.segments = c.segments, st.segments_complemented = c.segments_complemented, st.keys_present = c.keys_present;
    st.keys_added = c.keys_added, st.keys_subtracted = c.keys_subtracted, st.lanes = c.lanes;
    st.device_ms = ms_since(t0);
    return BLSGPU_OK;
  });
  if (rc == BLSGPU_OK) {
    memcpy(out, h_out.data(), h_out.size());
    memcpy(status, h_st.data(), n);
    if (stats) *stats = st;
  }
  return rc;
}

int blsgpu_signing_roots(blsgpu_ctx* ctx, int kind, uint32_t n, const uint8_t* objects, uint32_t object_stride,
                         const uint8_t* domains, uint32_t domain_stride, uint8_t* out32) {
  if (!ctx || ctx->devs.empty() || !objects || !domains || !out32) return BLSGPU_ERR_ARGS;
  const uint32_t obj_len = kind == BLSGPU_ROOT_OBJECT ? 32 : (kind == BLSGPU_ROOT_ATTESTATION_DATA ? 128 : 0);
  if (!obj_len || object_stride < obj_len || (domain_stride != 0 && domain_stride < 32)) return BLSGPU_ERR_ARGS;
  if (n == 0) return BLSGPU_OK;
  return helper_call(ctx, false, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    const hl::SigningRoots l(n, object_stride, domain_stride);
    sl.d_in.ensure(l.total);
    uint8_t* din = sl.d_in.p;
    HIPCHK(hipMemcpyAsync(din, objects, (size_t)n * object_stride, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(din + l.dom, domains, l.dom_bytes, hipMemcpyHostToDevice, s));
    launch_signing_roots(kind, din, n, object_stride, din + l.dom, domain_stride, din + l.out, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out32, din + l.out, 32 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSGPU_OK;
  });
}

int blsgpu_debug_op(blsgpu_ctx* ctx, int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out,
                    uint32_t out_stride, int32_t* status) {
  if (!ctx || ctx->devs.empty() || !in || !out || !status) return BLSGPU_ERR_ARGS;
  // the bytes each op reads per element and writes per element (k_debug.hip): a smaller stride is refused here, so a
  // test hook can never read or write past its buffers on the device
  struct OpSize {
    int op;
    uint32_t in, out;
  };
  static const OpSize kOpSizes[] = {{0, 96, 48},    {1, 194, 192},  {2, 32, 192},   {3, 288, 576},  {4, 576, 576},
                                    {5, 104, 96},   {6, 200, 192},  {7, 64, 96},    {8, 32, 96},    {9, 200, 2880},
                                    {10, 104, 1440}, {11, 840, 56}, {16, 576, 576}, {17, 288, 576}, {18, 384, 192},
      // the field tower's raw-limb hooks (tower_debug.hpp): 56 bytes per Fp value in and out, predicates write nothing
      {32, 112, 56}, {33, 56, 56}, {34, 224, 112}, {35, 112, 112}, {36, 168, 112}, {37, 112, 56},
      {38, 112, 56}, {39, 56, 56}, {40, 56, 56}, {41, 56, 56}, {42, 56, 56}, {43, 56, 56},
      {44, 56, 56}, {45, 56, 56}, {46, 112, 56}, {47, 112, 112}, {48, 56, 0}, {49, 112, 0},
      {50, 672, 0}, {51, 56, 56}, {52, 56, 56}, {53, 112, 112}, {54, 336, 336}, {55, 672, 672},
      {56, 112, 112}, {57, 672, 336}, {58, 560, 336}, {59, 560, 336}, {60, 1344, 672}, {61, 672, 672},
      {62, 1008, 672}, {63, 1344, 672}, {64, 672, 672}, {65, 672, 672}, {66, 672, 672}, {67, 672, 672},
      {68, 672, 672},
      // the point formulas' hooks (curve_debug.hpp): Jacobian (x, y, z) / affine (x, y), G1 69..85, G2 86..107
      {69, 168, 168}, {70, 168, 168}, {71, 168, 168}, {72, 336, 168}, {73, 336, 168}, {74, 336, 168},
      {75, 280, 168}, {76, 280, 168}, {77, 280, 168}, {78, 168, 168}, {79, 168, 0}, {80, 336, 0},
      {81, 168, 112}, {82, 168, 168}, {83, 168, 168}, {84, 112, 0}, {85, 112, 0},
      {86, 336, 336}, {87, 336, 336}, {88, 336, 336}, {89, 672, 336}, {90, 672, 336}, {91, 672, 336},
      {92, 560, 336}, {93, 560, 336}, {94, 560, 336}, {95, 336, 336}, {96, 336, 0}, {97, 672, 0},
      {98, 336, 224}, {99, 336, 336}, {100, 336, 336}, {101, 336, 336}, {102, 336, 336}, {103, 336, 336},
      {104, 224, 336}, {105, 224, 0}, {106, 224, 0}, {107, 224, 0}};
  const OpSize* sz = nullptr;
  for (const OpSize& o : kOpSizes)
    if (o.op == op) sz = &o;
  // the multi-lane engines' hooks (coop_debug.hpp): lacc_fin 108, lane pairs 109..131, six-lane groups 132..141, g2c
  // groups 142..144 (a flag slot, the point, the addend), the workgroup GT engine 145..157
  static const OpSize kCoopSizes[] = {
      {108, 112, 56}, {109, 224, 112}, {110, 112, 112}, {111, 112, 112}, {112, 112, 112}, {113, 112, 0},
      {114, 224, 112}, {115, 448, 112}, {116, 336, 112}, {117, 336, 112}, {118, 336, 112}, {119, 672, 336},
      {120, 672, 672}, {121, 1008, 672}, {122, 336, 672}, {123, 560, 672}, {124, 336, 336}, {125, 672, 336},
      {126, 560, 336}, {127, 336, 336}, {128, 336, 0}, {129, 336, 336}, {130, 336, 336}, {131, 336, 336},
      {132, 1344, 672}, {133, 672, 672}, {134, 672, 672}, {135, 672, 672}, {136, 672, 672}, {137, 672, 672},
      {138, 1120, 672}, {139, 672, 0}, {140, 672, 672}, {141, 672, 672}, {142, 728, 336}, {143, 728, 336},
      {144, 728, 336}, {145, 1344, 672}, {146, 1344, 672}, {147, 1344, 672}, {148, 672, 672}, {149, 1008, 672},
      {150, 672, 672}, {151, 672, 672}, {152, 672, 672}, {153, 672, 672}, {154, 672, 672}, {155, 672, 672},
      {156, 672, 672}, {157, 336, 672}};
  for (const OpSize& o : kCoopSizes)
    if (o.op == op) sz = &o;
  // lane pairs again (coop_debug.hpp COOP_OP_PAIR2): n doublings (the point, then the count's slot), the [|z|] chain
  // from a Jacobian / an affine point
  static const OpSize kPair2Sizes[] = {{160, 392, 336}, {161, 336, 336}, {162, 224, 336}};
  for (const OpSize& o : kPair2Sizes)
    if (o.op == op) sz = &o;
  if (!sz || in_stride < sz->in || out_stride < sz->out) return BLSGPU_ERR_ARGS;
  const bool tower = op >= 32;  // limb words are read and written as uint32: word-aligned elements only
  if (tower && (in_stride % 4 || out_stride % 4 || out_stride == 0)) return BLSGPU_ERR_ARGS;
  if (n == 0) return BLSGPU_OK;
  return helper_call(ctx, false, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    struct Temp {  // its own allocations, not the helper's arenas: freed however the call ends
      void* p = nullptr;
      ~Temp() {
        if (p) (void)hipFree(p);
      }
    } din, dout, dst;
    HIPCHK(hipMalloc(&din.p, (size_t)n * in_stride));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * out_stride));
    HIPCHK(hipMalloc(&dst.p, (size_t)n * 4));
    HIPCHK(hipMemcpyAsync(din.p, in, (size_t)n * in_stride, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dout.p, 0, (size_t)n * out_stride, s));
    if (op >= 108) {  // (coop_debug.hpp COOP_OP_FIRST)
      HIPCHK(hipMemsetAsync(dst.p, 0, (size_t)n * 4, s));
      launch_debug_coop(op, n, (uint8_t*)din.p, in_stride, (uint8_t*)dout.p, out_stride, (int32_t*)dst.p, s);
    } else if (op >= 69)  // (curve_debug.hpp CRV_OP_FIRST)
      launch_debug_curve(op, n, (uint8_t*)din.p, in_stride, (uint8_t*)dout.p, out_stride, (int32_t*)dst.p, s);
    else if (tower)
      launch_debug_tower(op, n, (uint8_t*)din.p, in_stride, (uint8_t*)dout.p, out_stride, (int32_t*)dst.p, s);
    else
      launch_debug_op(op, n, (uint8_t*)din.p, in_stride, (uint8_t*)dout.p, out_stride, (int32_t*)dst.p, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * out_stride, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, dst.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSGPU_OK;
  });
}

}  // extern "C"
