// The synchronous helper calls of libblsgpu (include/blsgpu.h): aggregation, same-message verification, AggregateVerify,
// key validation, signing roots and the debug ops.  Each runs start to finish on device 0 under Device::helper_mu, on
// table_stream, in Device::helper's buffers; helper_call is the envelope they share and helper_layout.hpp says where
// every field of their device arenas lies.  The asynchronous verification pipeline is runtime.cpp and pipeline.cpp.
#include "aggverify_plan.hpp"
#include "helper_layout.hpp"
#include "runtime_internal.hpp"

using namespace blsgpu_rt;
namespace hl = helper_layout;
namespace avp = aggverify_plan;

static_assert(hl::kFp == W_FP && hl::kG1A == W_G1A && hl::kG1J == W_G1J && hl::kG2A == W_G2A && hl::kG2J == W_G2J &&
                  hl::kFp12 == W_FP12 && hl::kAwrTabWords == AWR_TAB_WORDS && hl::kMillerLineWords == kMillerLineWords,
              "helper_layout.hpp restates the element widths of kernels.h");

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

// BLSGPU_OK and a.n, or BLSGPU_ERR_ARGS: group_first starts at 0 and never decreases, at most 2^20 signatures, and
// no 192-byte signature under a stride below 192.
int check_group_layout(Grouped& a) {
  if (a.group_first[0] != 0) return BLSGPU_ERR_ARGS;
  for (uint32_t g = 0; g < a.G; g++)
    if (a.group_first[g + 1] < a.group_first[g]) return BLSGPU_ERR_ARGS;
  a.n = a.group_first[a.G];
  if (a.n > (1u << 20)) return BLSGPU_ERR_ARGS;
  if (a.sig_stride < 192)
    for (uint32_t k = 0; k < a.n; k++)
      if (a.sig_len[k] == 192) return BLSGPU_ERR_ARGS;
  return BLSGPU_OK;
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
  return helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    std::vector<uint64_t> words;
    uint64_t hash_key = 0;
    if (int e = same_begin(d, a, seed, words, hash_key)) return e;
    const uint32_t L = awr_lanes(G, n), lanes = awr_launch_lanes(G, L);
    const hl::Awr l(G, n, sig_stride, pk_bytes != nullptr, out_pk_len, out_sig_len, lanes);
    sl.d_in.ensure(l.total);
    sl.d_work.ensure(l.work_words);
    uint8_t* din = sl.d_in.p;
    PipelineBuffers pb;
    const AwrBuffers ab = same_inputs(d, a, l, din, words.data(), lanes, s, pb);
    int8_t* d_gst = reinterpret_cast<int8_t*>(din + l.gst);
    uint32_t* d_fb = reinterpret_cast<uint32_t*>(din + l.fb);
    // small calls take the cooperative subgroup check, as small verification runs do
    launch_sig_decode(pb, n, s, n <= 4096, nullptr, false, true);
    launch_awr_sums(ab, L, s);
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

// ---- one-call same-message verification ------------------------------------------------------------------------
// A phase of at most kSameCoopMax pairings takes the cooperative kernels (a workgroup per Miller loop and per check:
// latency), a larger one the lane forms (throughput).  512 is the coop_max option's default, taken as a constant: the
// helper calls read no option.
constexpr uint32_t kSameCoopMax = 512;
uint32_t blsgpu_same_message_form(uint32_t n_items, uint32_t flags) {
  return (flags & BLSGPU_SAME_LANE_FORMS) || n_items > kSameCoopMax ? 1u : 0u;
}
// BLSGPU_SAME_BLOCK_CHECK: groups per block, the group_sets option's default as a constant (as kSameCoopMax above)
static_assert(SAME_BLOCK_GROUPS == 1024, "include/blsgpu.h documents blocks of 1024 groups");
uint32_t blsgpu_same_message_blocks(uint32_t n_groups, uint32_t flags) {
  return flags & BLSGPU_SAME_BLOCK_CHECK ? n_groups / SAME_BLOCK_GROUPS + (n_groups % SAME_BLOCK_GROUPS ? 1u : 0u) : 0u;
}
namespace {
// diagnostics (tools/bench_same_message.py): the three branches of the group phase on one stream
inline bool same_serial() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_SAME_SERIAL");
    return v && v[0] == '1';
  }();
  return on;
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
void same_pairing_phase(const PipelineBuffers& pm, uint32_t n_items, const uint32_t* iota, uint32_t* pk_aff,
                        uint8_t* include, const uint32_t* msg_idx, const uint32_t* S, uint32_t* F, uint32_t* Gs,
                        uint8_t* ok, bool lane, hipStream_t s) {
  same_miller_half(pm, n_items, iota, pk_aff, include, msg_idx, F, lane, s);
  same_check_half(n_items, S, F, Gs, ok, lane, s);
}
// The aggregate outputs of blsgpu_verify_same_message_agg; blsgpu_verify_same_message has none.
struct SameAggOut {
  const uint8_t* include;  // [n_sets], nullable
  uint8_t* out_sig;
  uint32_t out_sig_len;
  uint32_t* count;
};

// The body of both same-message verification calls.  agg null: blsgpu_verify_same_message, which launches what it
// always launched.  Else the aggregate phase follows the retry phase.
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
  std::vector<int8_t> h_set(n), h_grp(G);
  std::vector<uint8_t> h_agg(agg ? (size_t)G * agg->out_sig_len : 0);
  std::vector<uint32_t> h_cnt(agg ? G : 0);
  blsgpu_same_message_stats st;
  memset(&st, 0, sizeof st);
  const int rc = helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    std::vector<uint64_t> words;
    uint64_t hash_key = 0;
    if (int e = same_begin(d, a, seed, words, hash_key)) return e;
    // messages, deduplicated as plan_run does (run_plan.hpp): group g signs unique message gmsg[g]
    std::vector<uint32_t> gmsg(G), uniq;
    {
      MsgIndex mi(G, hash_key ^ 0x6a09e667f3bcc908ull);
      for (uint32_t g = 0; g < G; g++) gmsg[g] = mi.find_or_add(msgs, g, uniq);
    }
    const uint32_t U = (uint32_t)uniq.size();
    st.unique_messages = U;
    bool streams_used = false;
    try {
      if (!d.same_st[0]) {
        for (auto& e : d.same_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipStreamCreateWithFlags(&d.same_st[1], hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&d.same_st[0], hipStreamNonBlocking));
      }
      const auto t0 = std::chrono::steady_clock::now();
      const bool serial = same_serial();
      hipStream_t sb = serial ? s : d.same_st[0], sc = serial ? s : d.same_st[1];
      const bool lane_g = blsgpu_same_message_form(G, flags) != 0;
      const uint32_t L = awr_lanes(G, n), lanes = awr_launch_lanes(G, L);
      const hl::Same l(G, n, U, sig_stride, pk_bytes != nullptr, lanes);
      // every buffer of the group phase grows here, while none of the three streams has work (each call ends with all
      // of them synchronized); the retry phase grows only buffers the group phase does not use, after its synchronize
      sl.d_in.ensure(l.in_total);
      sl.d_bytes.ensure(l.bytes_total);
      sl.d_work.ensure(l.work_words);
      if (lane_g) sl.d_lines.ensure(l.lines_words);
      // BLSGPU_SAME_BLOCK_CHECK: the block phase's buffers grow here too; the descent's, like the retry phase's, after
      // the synchronize before it, and they are buffers no other phase uses
      const uint32_t NB = blsgpu_same_message_blocks(G, flags);
      const hl::SameBlocks lb(NB, NB ? same_block_tree_width(G) : 0, 0);
      if (NB) {
        sl.d_msmW.ensure(lb.work_words);
        sl.d_res.ensure(lb.bytes_total);
      }
      // the aggregate phase's buffer too: one no other phase of the call uses
      const hl::SameAgg la(G, n, agg ? agg->out_sig_len : 0);
      if (agg) sl.d_msmB.ensure(la.total_words);
      streams_used = true;
      uint8_t* din = sl.d_in.p;
      uint8_t* db = sl.d_bytes.p;
      uint32_t* w = sl.d_work.p;
      std::vector<uint32_t> iota((size_t)G + 1);
      for (uint32_t g = 0; g <= G; g++) iota[g] = g;
      std::vector<uint8_t> umsgs((size_t)U * 32);
      for (uint32_t u = 0; u < U; u++) memcpy(umsgs.data() + (size_t)u * 32, msgs + (size_t)uniq[u] * 32, 32);
      PipelineBuffers pb;  // the signature decode
      const AwrBuffers ab = same_inputs(d, a, l, db, words.data(), lanes, s, pb);
      HIPCHK(hipMemcpyAsync(din + l.umsg, umsgs.data(), (size_t)U * 32, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(din + l.gmsg, gmsg.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(din + l.iota, iota.data(), (size_t)(G + 1) * 4, hipMemcpyHostToDevice, s));
      uint8_t* da = agg ? reinterpret_cast<uint8_t*>(sl.d_msmB.p) : nullptr;
      if (agg && agg->include && n) HIPCHK(hipMemcpyAsync(da + la.inc, agg->include, n, hipMemcpyHostToDevice, s));
      AwrBuffers ab_pk = ab;  // the G1 sum runs beside the G2 sum: its own window scratch
      ab_pk.tab = w + l.w_tab_pk;
      uint32_t* g_pk_aff = w + l.w_pk_aff;
      uint32_t* g_inv = w + l.w_inv;
      uint32_t* g_F = w + l.w_F;
      uint32_t* g_G = w + l.w_G;
      PipelineBuffers pm{};  // the message branch
      pm.umsgs = din + l.umsg;
      pm.n_umsg = U;
      pm.nm = U;
      pm.inv_buf = w + l.w_minv;
      pm.h_aff = w + l.w_haff;
      pm.h_jac = w + l.w_hjac;
      pm.h_norm = w + l.w_hnorm;
      pm.h_prep = w + l.w_hprep;
      pm.h_q = w + l.w_hq;
      pm.mflags = db + l.b_mf;
      pm.lines = sl.d_lines.p;
      uint8_t* g_inc = db + l.b_inc;
      int8_t* g_code = reinterpret_cast<int8_t*>(db + l.b_code);
      uint8_t* g_ok = db + l.b_ok;
      int8_t* d_gres = reinterpret_cast<int8_t*>(db + l.b_gres);
      int8_t* d_sres = reinterpret_cast<int8_t*>(db + l.b_sres);
      const uint32_t* d_gmsg = reinterpret_cast<uint32_t*>(din + l.gmsg);
      const uint32_t* d_iota = reinterpret_cast<uint32_t*>(din + l.iota);
      // ---- group phase: three branches from the input copy, joined into s
      HIPCHK(hipEventRecord(d.same_ev[0], s));
      if (!serial) {
        HIPCHK(hipStreamWaitEvent(sb, d.same_ev[0], 0));
        HIPCHK(hipStreamWaitEvent(sc, d.same_ev[0], 0));
      }
      // (a) signatures: decode + subgroup check (cooperative for small calls, as small verification runs), S_g
      launch_sig_decode(pb, n, s, n <= 4096, nullptr, false, true);
      launch_awr_sum_sig(ab, L, s);
      // (b) keys: P_g and the batch inverses of its z
      launch_awr_sum_pk(ab_pk, L, sb);
      launch_batch_inv(ab.sum_pk, G, 2 * W_FP, g_inv, G, sb);
      HIPCHK(hipEventRecord(d.same_ev[1], sb));
      // (c) messages: H(m) affine, and in the lane form its Miller lines
      bool have_lines = false;
      launch_hash_to_g2(pm, sc, U <= 4096, false);
      launch_h_affine(pm, sc);
      if (lane_g) {
        launch_miller_lines2(pm, sc);
        have_lines = true;
      }
      HIPCHK(hipEventRecord(d.same_ev[2], sc));
      if (!serial) {
        HIPCHK(hipStreamWaitEvent(s, d.same_ev[1], 0));
        HIPCHK(hipStreamWaitEvent(s, d.same_ev[2], 0));
      }
      launch_same_group_items(ab, g_inv, g_pk_aff, g_inc, g_code, s);
      std::vector<uint32_t> listed;  // (alive until the final synchronize: it is copied from)
      if (!NB) {
        same_pairing_phase(pm, G, d_iota, g_pk_aff, g_inc, d_gmsg, ab.sum_sig, g_F, g_G, g_ok, lane_g, s);
        launch_same_group_results(ab.group_first, G, n, g_inc, g_code, g_ok, d_sres, d_gres, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_grp.data(), d_gres, G, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));  // every branch was joined into s: all three streams are idle
      } else {
        // ---- block phase: F_b, S_b per block of groups and one check per block.  S_b needs the sums
        // and the include flags only: it runs on sb, beside the Miller loops, and is joined into s before the check.
        const bool lane_b = blsgpu_same_message_form(NB, flags) != 0;
        uint32_t* bw = sl.d_msmW.p;
        uint32_t* b_F = bw + lb.w_F;
        uint32_t* b_S = bw + lb.w_S;
        uint8_t* b_any = sl.d_res.p + lb.b_any;
        uint8_t* b_ok = sl.d_res.p + lb.b_ok;
        HIPCHK(hipEventRecord(d.same_ev[0], s));
        if (!serial) HIPCHK(hipStreamWaitEvent(sb, d.same_ev[0], 0));
        launch_same_block_sum(ab.sum_sig, g_inc, G, NB, b_S, b_any, sb);
        HIPCHK(hipEventRecord(d.same_ev[1], sb));
        same_miller_half(pm, G, d_iota, g_pk_aff, g_inc, d_gmsg, g_F, lane_g, s);
        launch_same_block_prod(g_F, g_inc, G, NB, bw + lb.w_T0, bw + lb.w_T1, b_F, s);
        if (!serial) HIPCHK(hipStreamWaitEvent(s, d.same_ev[1], 0));
        same_check_half(NB, b_S, b_F, sl.d_msmW.p + lb.w_G, b_ok, lane_b, s);
        launch_same_block_results(ab.group_first, G, n, g_inc, g_code, b_any, b_ok, d_sres, d_gres, s);
        HIPCHK(hipGetLastError());
        std::vector<uint8_t> h_blk(2 * (size_t)NB), h_inc(G);
        HIPCHK(hipMemcpyAsync(h_blk.data(), b_any, NB, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_blk.data() + NB, b_ok, NB, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_inc.data(), g_inc, G, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_grp.data(), d_gres, G, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));  // every branch was joined into s: all three streams are idle
        st.form |= 4;
        // ---- descent: the included groups of the failed blocks, each checked from its own F_g, S_g.  A failed block
        // with one included group has its answer already: that group failed.
        for (uint32_t b = 0; b < NB; b++) {
          if (!h_blk[b] || h_blk[NB + b]) continue;
          const uint32_t first = b * SAME_BLOCK_GROUPS, last = std::min<uint64_t>(G, (uint64_t)first + SAME_BLOCK_GROUPS);
          const size_t before = listed.size();
          for (uint32_t g = first; g < last; g++)
            if (h_inc[g]) listed.push_back(g);
          if (listed.size() - before == 1) listed.pop_back();
        }
        const uint32_t nl = (uint32_t)listed.size();
        if (nl) {
          const bool lane_d = blsgpu_same_message_form(nl, flags) != 0;
          const hl::SameBlocks ld(NB, 0, nl);
          sl.d_fkeep.ensure(ld.descent_words);
          sl.d_fbflags.ensure(ld.d_ok_bytes);
          uint32_t* dw = sl.d_fkeep.p;
          uint8_t* l_ok = sl.d_fbflags.p;
          HIPCHK(hipMemcpyAsync(dw + ld.d_list, listed.data(), (size_t)nl * 4, hipMemcpyHostToDevice, s));
          launch_same_gather(g_F, ab.sum_sig, G, dw + ld.d_list, nl, dw + ld.d_F, dw + ld.d_S, s);
          same_check_half(nl, dw + ld.d_S, dw + ld.d_F, dw + ld.d_G, l_ok, lane_d, s);
          launch_same_descent_results(ab.group_first, G, n, dw + ld.d_list, nl, l_ok, d_sres, d_gres, s);
          HIPCHK(hipGetLastError());
          HIPCHK(hipMemcpyAsync(h_grp.data(), d_gres, G, hipMemcpyDeviceToHost, s));
          HIPCHK(hipStreamSynchronize(s));
          st.form |= lane_d ? 8 | 16 : 8;
        }
      }
      if (lane_g) st.form |= 1;
      // ---- retry phase: every set of a non-empty group whose check did not hold, on its own with r = 1
      std::vector<uint32_t> rlist, rmsg, riota;  // (alive until the final synchronize: they are copied from)
      for (uint32_t g = 0; g < G; g++) {
        if (group_first[g + 1] == group_first[g]) continue;
        if (h_grp[g] == 1) {
          st.groups_accepted++;
          continue;
        }
        st.groups_retried++;
        for (uint32_t k = group_first[g]; k < group_first[g + 1]; k++) {
          rlist.push_back(k);
          rmsg.push_back(gmsg[g]);
        }
      }
      const uint32_t nr = (uint32_t)rlist.size();
      st.retry_sets = nr;
      if (nr) {
        const bool lane_r = blsgpu_same_message_form(nr, flags) != 0;
        const hl::SameRetry r(nr);
        sl.d_list.ensure(r.list_words);
        sl.d_ok.ensure(r.ok_bytes);
        sl.d_fb.ensure(r.fb_words);
        sl.d_S.ensure(r.S_words);
        sl.d_F.ensure(r.F_words);
        if (lane_r) sl.d_G.ensure(r.F_words);
        if (lane_r && !have_lines) {
          sl.d_lines.ensure(l.lines_words);
          pm.lines = sl.d_lines.p;
        }
        riota.resize((size_t)nr + 1);
        for (uint32_t q = 0; q <= nr; q++) riota[q] = q;
        uint32_t* dl = sl.d_list.p;
        HIPCHK(hipMemcpyAsync(dl, rlist.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dl + r.msg, rmsg.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dl + r.iota, riota.data(), (size_t)(nr + 1) * 4, hipMemcpyHostToDevice, s));
        uint8_t* r_inc = sl.d_ok.p;
        int8_t* r_code = reinterpret_cast<int8_t*>(sl.d_ok.p + r.code);
        uint8_t* r_ok = sl.d_ok.p + r.ok;
        launch_same_retry_items(ab, dl, nr, sl.d_fb.p, sl.d_S.p, r_inc, r_code, s);
        if (lane_r && !have_lines) launch_miller_lines2(pm, s);
        same_pairing_phase(pm, nr, dl + r.iota, sl.d_fb.p, r_inc, dl + r.msg, sl.d_S.p, sl.d_F.p, sl.d_G.p, r_ok, lane_r,
                           s);
        launch_same_retry_results(dl, nr, r_inc, r_code, r_ok, d_sres, s);
        HIPCHK(hipGetLastError());
        if (lane_r) st.form |= 2;
      }
      // ---- aggregate phase: each group's sum over the sets that answered 1, from the signatures decoded once
      if (agg) {
        launch_same_agg(pb.sig_aff, n, d_sres, agg->include ? da + la.inc : nullptr, ab.group_first, G,
                        reinterpret_cast<uint32_t*>(da + la.sums), reinterpret_cast<uint32_t*>(da + la.count),
                        da + la.out, agg->out_sig_len, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_agg.data(), da + la.out, h_agg.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_cnt.data(), da + la.count, (size_t)G * 4, hipMemcpyDeviceToHost, s));
      }
      if (n) HIPCHK(hipMemcpyAsync(h_set.data(), d_sres, n, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      st.device_ms = ms_since(t0);
    } catch (HipError&) {
      // no branch may outlive the call: the next helper call reuses, and may grow, the buffers they work on
      if (streams_used) {
        (void)hipStreamSynchronize(d.table_stream);
        for (hipStream_t x : d.same_st)
          if (x) (void)hipStreamSynchronize(x);
      }
      throw;
    }
    return BLSGPU_OK;
  });
  if (rc == BLSGPU_OK) {  // results reach the caller only when every one of them was computed
    if (n) memcpy(set_result, h_set.data(), n);
    if (group_result) memcpy(group_result, h_grp.data(), G);
    if (stats) *stats = st;
    if (agg) {
      memcpy(agg->out_sig, h_agg.data(), h_agg.size());
      memcpy(agg->count, h_cnt.data(), (size_t)G * 4);
    }
  }
  return rc;
}
}  // namespace

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

// ---- batched AggregateVerify -----------------------------------------------------------------------------------
// A job's signature is one more pair of the job, (-g1, sig): k pairs are k + 1 Miller items in the job's own
// accumulators and one final exponentiation (aggverify_plan.hpp, k_aggverify.hip).
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
  if (n_jobs > (1u << 20) || job_first[0] != 0) return BLSGPU_ERR_ARGS;
  for (uint32_t j = 0; j < n_jobs; j++)
    if (job_first[j + 1] < job_first[j]) return BLSGPU_ERR_ARGS;
  const uint32_t J = n_jobs, n = job_first[J];
  if (n > (1u << 20)) return BLSGPU_ERR_ARGS;
  if (sig_stride < 192)
    for (uint32_t j = 0; j < J; j++)
      if (sig_len[j] == 192) return BLSGPU_ERR_ARGS;
  std::vector<int8_t> h_res(J);
  std::vector<uint32_t> h_fb(J);
  std::vector<uint8_t> h_chk(J);
  blsgpu_aggregate_verify_stats st;
  memset(&st, 0, sizeof st);
  const int rc = helper_call(ctx, true, [&](Device& d, Slot& sl, hipStream_t s) -> int {
    if (pk_index)
      for (uint32_t k = 0; k < n; k++)
        if (pk_index[k] >= d.table_n) return BLSGPU_ERR_ARGS;
    // messages, deduplicated over the whole call: pair k signs unique message pmsg[k].  The call draws no randomness,
    // so the index is keyed by a constant (the key only spreads the table's probes; equality is by memcmp).
    std::vector<uint32_t> pmsg(n), uniq;
    {
      MsgIndex mi(n, 0xbb67ae8584caa73bull);
      for (uint32_t k = 0; k < n; k++) pmsg[k] = mi.find_or_add(msgs, k, uniq);
    }
    const uint32_t U = (uint32_t)uniq.size();
    // every non-empty job is planned: which of them the device rejects is known only after the decodes, and their
    // items are switched off by the include bytes (one synchronize less than reading the status back first)
    const avp::Counts planned = avp::count(job_first, J, nullptr, 1);
    const bool lane = blsgpu_aggregate_verify_form(planned.items, flags) != 0;
    const uint32_t kc = avp::chunk_items_for(job_first, J, lane ? 1 : 0, (flags & BLSGPU_AV_LANE_FORMS) != 0);
    const avp::Plan plan = avp::build(job_first, J, nullptr, kc);
    const uint32_t C = plan.n_chunks();
    // jobs of few chunks: a lane per job multiplies its chunk values; else a wave per job
    const bool lane_reduce = lane && (uint64_t)C <= (uint64_t)avp::kLaneReduceMax * planned.jobs;
    st.pairs = n;
    st.unique_messages = U;
    st.form = lane ? 1 : 0;
    bool streams_used = false;
    try {
      if (!d.same_st[0]) {
        for (auto& e : d.same_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipStreamCreateWithFlags(&d.same_st[1], hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&d.same_st[0], hipStreamNonBlocking));
      }
      const auto t0 = std::chrono::steady_clock::now();
      hipStream_t sb = d.same_st[0], sc = d.same_st[1];
      const hl::AggVerify l(J, n, U, C, sig_stride, pk_bytes != nullptr, pk_len, validate);
      // every buffer grows here, while none of the three streams has work (each call ends with all of them synchronized)
      sl.d_in.ensure(l.in_total);
      sl.d_bytes.ensure(l.bytes_total);
      sl.d_work.ensure(l.work_words);
      if (lane) sl.d_lines.ensure(l.lines_words);
      streams_used = true;
      uint8_t* din = sl.d_in.p;
      uint8_t* db = sl.d_bytes.p;
      uint32_t* w = sl.d_work.p;
      std::vector<uint8_t> umsgs((size_t)U * 32);
      for (uint32_t u = 0; u < U; u++) memcpy(umsgs.data() + (size_t)u * 32, msgs + (size_t)uniq[u] * 32, 32);
      HIPCHK(hipMemcpyAsync(din + l.gf, job_first, (size_t)(J + 1) * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(din + l.len, sig_len, (size_t)J * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(din + l.sigs, sigs, (size_t)J * sig_stride, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(din + l.fr, plan.f_ranges.data(), (size_t)2 * J * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(din + l.cf, plan.chunk_first.data(), (size_t)(C + 1) * 4, hipMemcpyHostToDevice, s));
      if (!plan.chunk_items.empty())
        HIPCHK(hipMemcpyAsync(din + l.ci, plan.chunk_items.data(), plan.chunk_items.size() * 4, hipMemcpyHostToDevice, s));
      if (n) {
        HIPCHK(hipMemcpyAsync(din + l.keys, pk_bytes ? (const void*)pk_bytes : (const void*)pk_index, l.key_bytes,
                              hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(din + l.umsg, umsgs.data(), (size_t)U * 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(din + l.pmsg, pmsg.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
      }
      PipelineBuffers pb{};  // the signature decode: one signature per job
      pb.n = J;
      pb.sigs = din + l.sigs;
      pb.sig_len = reinterpret_cast<uint32_t*>(din + l.len);
      pb.sig_stride = sig_stride;
      pb.sig_aff = w;
      pb.flags = db + l.b_fl;
      pb.status = reinterpret_cast<int8_t*>(db + l.b_st);
      PipelineBuffers pm{};  // the message branch: U hashed columns of the M = U + J
      pm.umsgs = din + l.umsg;
      pm.n_umsg = U;
      pm.nm = (uint32_t)l.M;
      pm.inv_buf = w + l.w_minv;
      pm.h_aff = w + l.w_haff;
      pm.h_jac = w + l.w_hjac;
      pm.h_norm = w + l.w_hnorm;
      pm.h_prep = w + l.w_hprep;
      pm.h_q = w + l.w_hq;
      pm.mflags = db + l.b_mf;
      pm.lines = sl.d_lines.p;
      AvBuffers av{};
      av.n_pairs = n;
      av.n_jobs = J;
      av.n_items = (uint32_t)l.T;
      av.n_umsg = U;
      av.nm = (uint32_t)l.M;
      av.job_first = reinterpret_cast<uint32_t*>(din + l.gf);
      av.pk_bytes = !pk_bytes ? nullptr : validate ? din + l.kv96 : din + l.keys;
      av.kv_status = validate ? reinterpret_cast<int8_t*>(db + l.b_kv) : nullptr;
      av.pk_index = pk_bytes ? nullptr : reinterpret_cast<uint32_t*>(din + l.keys);
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
      av.h_aff = pm.h_aff;
      av.mflags = pm.mflags;
      av.checked = db + l.b_chk;
      av.job_code = reinterpret_cast<int8_t*>(db + l.b_jcode);
      av.first_bad = reinterpret_cast<uint32_t*>(db + l.b_fb);
      uint32_t* F = w + l.w_F;
      uint8_t* d_ok = db + l.b_ok;
      int8_t* d_res = reinterpret_cast<int8_t*>(db + l.b_res);
      // ---- three branches from the input copy, joined into s
      HIPCHK(hipEventRecord(d.same_ev[0], s));
      HIPCHK(hipStreamWaitEvent(sb, d.same_ev[0], 0));
      HIPCHK(hipStreamWaitEvent(sc, d.same_ev[0], 0));
      // (a) signatures: decode + subgroup check (cooperative for small calls, as small verification runs)
      launch_sig_decode(pb, J, s, J <= 4096, nullptr, false, true);
      // (b) keys: KeyValidate when they are untrusted, then every pair's affine point and code
      if (validate)
        launch_key_validate(din + l.keys, n, pk_len, pk_len, din + l.kv96, reinterpret_cast<int8_t*>(db + l.b_kv), sb);
      launch_av_pair_items(av, sb);
      HIPCHK(hipEventRecord(d.same_ev[1], sb));
      // (c) messages: H(m) affine, and in the lane form the Miller lines of those columns
      launch_hash_to_g2(pm, sc, U <= 4096, false);
      launch_h_affine(pm, sc);
      if (lane) launch_miller_lines2(pm, sc);
      HIPCHK(hipEventRecord(d.same_ev[2], sc));
      HIPCHK(hipStreamWaitEvent(s, d.same_ev[1], 0));
      HIPCHK(hipStreamWaitEvent(s, d.same_ev[2], 0));
      launch_av_job_items(av, s);
      PipelineBuffers px = pm;  // the Miller accumulation over the T items and the M columns
      px.n = (uint32_t)l.T;
      px.n_umsg = (uint32_t)l.M;
      px.pk_aff = av.pk_aff;
      px.include = av.include;
      px.msg_idx = av.msg_idx;
      px.n_chunks = C;
      px.chunk_first = reinterpret_cast<uint32_t*>(din + l.cf);
      px.chunk_items = reinterpret_cast<uint32_t*>(din + l.ci);
      px.f_chunk = w + l.w_fchunk;
      const uint32_t* d_fr = reinterpret_cast<uint32_t*>(din + l.fr);
      if (!lane) {
        launch_miller_coop(px, false, s, false);
      } else {
        // the signature columns' lines: columns U .. M - 1, addressed as a call of J columns in the same arrays
        PipelineBuffers ps = pm;
        ps.n_umsg = J;
        ps.h_aff = pm.h_aff + U;
        ps.mflags = pm.mflags + U;
        ps.lines = pm.lines + U;
        launch_miller_lines2(ps, s);
        launch_miller_acc(px, false, s);
      }
      if (lane_reduce)
        launch_av_reduce_lane(px.f_chunk, px.n, d_fr, J, F, s);
      else
        launch_group_reduce(px, d_fr, J, F, s);
      launch_av_check(F, J, av.checked, d_ok, lane, s);
      launch_av_results(J, av.job_code, av.checked, d_ok, d_res, s);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(h_res.data(), d_res, J, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(h_fb.data(), av.first_bad, (size_t)J * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(h_chk.data(), av.checked, J, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));  // every branch was joined into s: all three streams are idle
      st.device_ms = ms_since(t0);
    } catch (HipError&) {
      // no branch may outlive the call: the next helper call reuses, and may grow, the buffers they work on
      if (streams_used) {
        (void)hipStreamSynchronize(d.table_stream);
        for (hipStream_t x : d.same_st)
          if (x) (void)hipStreamSynchronize(x);
      }
      throw;
    }
    const avp::Counts done = avp::count(job_first, J, h_chk.data(), kc);
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
