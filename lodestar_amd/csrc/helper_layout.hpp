// Device-arena layouts of the synchronous helper calls (helpers.cpp): per call one struct of named offsets, computed
// by its constructor from the call's sizes, fields in arena order.  No HIP here: tests/native/layout_probe.cpp includes
// this header alone and tests/test_helper_layout.py compares every offset and total with the formulas in Python.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace helper_layout {

// words per element, as kernels.h defines them (helpers.cpp asserts that the two agree)
constexpr size_t kFp = 14, kG1A = 2 * kFp, kG1J = 3 * kFp, kG2A = 4 * kFp, kG2J = 6 * kFp, kFp12 = 12 * kFp;
constexpr size_t kAwrTabWords = 9 * kG2J;              // window scratch per lane of the randomized sums
constexpr size_t kMillerLineWords = 68 * 3 * 2 * kFp;  // stored Miller lines per message

// Appends fields to an arena: take(size) returns the field's offset and moves on to the next multiple of `align`.
// `end` is where the last field ends (the total of an arena with no padding after it), `at` that end rounded up.
struct Carve {
  size_t align = 256, at = 0, end = 0;
  size_t take(size_t size) {
    const size_t o = at;
    end = o + size, at = (end + align - 1) / align * align;
    return o;
  }
};

// blsgpu_aggregate_pubkeys.  d_in: set_pk_first | keys | out | status.  d_work: a Jacobian sum per set.
struct AggPubkeys {
  size_t spf, keys, out, st, total, key_bytes, work_words;
  AggPubkeys(size_t n, size_t npk, bool keys_are_bytes, size_t out_len) {
    Carve c;
    key_bytes = npk * (keys_are_bytes ? 96 : 4);
    spf = c.take((n + 1) * 4), keys = c.take(key_bytes), out = c.take(n * out_len), st = c.take(3 * n);
    total = c.end, work_words = n * kG1J;
  }
};

// blsgpu_aggregate_pubkeys_bits: n sets over n_segs segments, bits_bytes bytes of bit strings.  d_in: set_seg_first |
// segment descriptors | set_bits_first | bits | present_first (a set's running count of set bits: what k_pk_serialize
// reads as set_pk_first) | out | status.  d_work: a Jacobian sum per set.
struct AggPubkeysBits {
  size_t ssf, seg, sbf, bits, present, out, st, total, work_words;
  AggPubkeysBits(size_t n, size_t n_segs, size_t bits_bytes, size_t out_len) {
    Carve c;
    ssf = c.take((n + 1) * 4), seg = c.take(n_segs * 4), sbf = c.take((n + 1) * 4), bits = c.take(bits_bytes);
    present = c.take((n + 1) * 4), out = c.take(n * out_len), st = c.take(3 * n);
    total = c.end, work_words = n * kG1J;
  }
};

// blsgpu_aggregate_signatures.  d_in: group_first | sig_len | sigs | out | first_bad | group status | signature
// status | signature flags.  d_work: sig_aff | a Jacobian sum per group (w_agg).
struct AggSigs {
  size_t gf, len, sigs, out, fb, gst, st, fl, total, w_agg, work_words;
  AggSigs(size_t G, size_t n, size_t sig_stride, size_t out_len) {
    Carve c;
    gf = c.take((G + 1) * 4), len = c.take(n * 4), sigs = c.take(n * sig_stride), out = c.take(G * out_len);
    fb = c.take(G * 4), gst = c.take(G), st = c.take(n), fl = c.take(n), total = c.end;
    w_agg = n * kG2A, work_words = w_agg + G * kG2J;
  }
};

// What both same-message calls begin their d_in with: words | group_first | sig_len | sigs | keys.
struct SameInput {
  size_t words, gf, len, sigs, keys, key_bytes;
  SameInput() {}
  SameInput(Carve& c, size_t G, size_t n, size_t sig_stride, bool keys_are_bytes) {
    key_bytes = n * (keys_are_bytes ? 96 : 4);
    words = c.take(n * 8), gf = c.take((G + 1) * 4), len = c.take(n * 4), sigs = c.take(n * sig_stride);
    keys = c.take(key_bytes);
  }
};

// The message branch of the same-message calls and of blsgpu_aggregate_verify, M G2 columns wide, in d_work (words):
// batch-inverse scratch | H(m) affine | Jacobian | its norm | the map's scratch | the cofactor clearing's.  hl::Same and
// hl::AggVerify carve it here and keep the six offsets as their fields w_minv .. w_hq; msg() hands them on as one.
struct MsgBranch {
  size_t inv, h_aff, h_jac, h_norm, h_prep, h_q;
  MsgBranch(size_t a, size_t b, size_t c, size_t d, size_t e, size_t f)
      : inv(a), h_aff(b), h_jac(c), h_norm(d), h_prep(e), h_q(f) {}
  MsgBranch(Carve& w, size_t M) {
    inv = w.take(M * kFp), h_aff = w.take(M * kG2A), h_jac = w.take(M * kG2J), h_norm = w.take(M * kFp);
    h_prep = w.take(M * 14 * kFp), h_q = w.take(M * 2 * kG2J);
  }
  void put(size_t& a, size_t& b, size_t& c, size_t& d, size_t& e, size_t& f) const {
    a = inv, b = h_aff, c = h_jac, d = h_norm, e = h_prep, f = h_q;
  }
};

// blsgpu_aggregate_with_randomness.  d_in: the shared inputs | out_pk | out_sig | first_bad | error indices | group
// status | error codes | signature status | signature flags (the b_ fields are those hl::Same keeps in d_bytes).
// d_work: sig_aff | window scratch | sum_pk | sum_sig.
struct Awr {
  SameInput in;
  size_t opk, osig, fb, b_ek, gst, b_ec, b_st, b_fl, total;
  size_t w_tab, w_sum_pk, w_sum_sig, work_words;
  Awr(size_t G, size_t n, size_t sig_stride, bool keys_are_bytes, size_t out_pk_len, size_t out_sig_len,
      size_t lanes) {
    Carve c, w{1};
    in = SameInput(c, G, n, sig_stride, keys_are_bytes);
    opk = c.take(G * out_pk_len), osig = c.take(G * out_sig_len), fb = c.take(G * 4), b_ek = c.take(G * 8);
    gst = c.take(G), b_ec = c.take(2 * G), b_st = c.take(n), b_fl = c.take(n), total = c.end;
    w.take(n * kG2A);  // sig_aff, at 0
    w_tab = w.take(lanes * kAwrTabWords), w_sum_pk = w.take(G * kG1J), w_sum_sig = w.take(G * kG2J);
    work_words = w.end;
  }
};

// blsgpu_verify_same_message, group phase (U unique messages).
//   d_in:    the shared inputs | unique messages | group message indices | iota
//   d_bytes: error indices | error codes | signature status | signature flags | message flags | group include |
//            group code | group verdict | group_result | set_result
//   d_work:  sig_aff | window scratch of the G2 sum | of the G1 sum | sum_pk | sum_sig | pk_aff | 1 / z | F | G |
//            message branch (msg(), U columns);  d_lines: the messages' Miller lines
struct Same {
  SameInput in;
  size_t umsg, gmsg, iota, in_total;
  size_t b_ek, b_ec, b_st, b_fl, b_mf, b_inc, b_code, b_ok, b_gres, b_sres, bytes_total;
  size_t w_tab, w_tab_pk, w_sum_pk, w_sum_sig, w_pk_aff, w_inv, w_F, w_G;
  size_t w_minv, w_haff, w_hjac, w_hnorm, w_hprep, w_hq, work_words, lines_words;
  MsgBranch msg() const { return MsgBranch(w_minv, w_haff, w_hjac, w_hnorm, w_hprep, w_hq); }
  Same(size_t G, size_t n, size_t U, size_t sig_stride, bool keys_are_bytes, size_t lanes) {
    Carve c, b, w{1};
    in = SameInput(c, G, n, sig_stride, keys_are_bytes);
    umsg = c.take(U * 32), gmsg = c.take(G * 4), iota = c.take((G + 1) * 4), in_total = c.at;
    b_ek = b.take(G * 8), b_ec = b.take(2 * G), b_st = b.take(n), b_fl = b.take(n), b_mf = b.take(U);
    b_inc = b.take(G), b_code = b.take(G), b_ok = b.take(G), b_gres = b.take(G), b_sres = b.take(n);
    bytes_total = b.at;
    w.take(n * kG2A);  // sig_aff, at 0
    w_tab = w.take(lanes * kAwrTabWords), w_tab_pk = w.take(lanes * kAwrTabWords);
    w_sum_pk = w.take(G * kG1J), w_sum_sig = w.take(G * kG2J), w_pk_aff = w.take(G * kG1A);
    w_inv = w.take(G * kFp), w_F = w.take(G * kFp12), w_G = w.take(G * kFp12);
    MsgBranch(w, U).put(w_minv, w_haff, w_hjac, w_hnorm, w_hprep, w_hq);
    work_words = w.end, lines_words = U * kMillerLineWords;
  }
};

// What a split call of blsgpu_aggregate_with_randomness or blsgpu_verify_same_message adds (awr_parts.hpp: its G groups
// cut into n_parts parts), in a buffer of its own (d_parts; hl::Awr and hl::Same are as for a call of the parts' launched
// lanes), sized with the call's other buffers.  Byte offsets, every field on a 256-byte boundary:
//   the parts' sum_pk | sum_sig (Jacobian, stride n_parts) | error indices (keys then signatures) | part_first (the
//   parts' first sets and n, copied up with the inputs) | group_part (the groups' first parts and n_parts, likewise) |
//   error codes
struct AwrParts {
  size_t sum_pk, sum_sig, ek, pf, gp, ec, total, total_words;
  AwrParts(size_t G, size_t n_parts) {
    Carve c;
    sum_pk = c.take(n_parts * kG1J * 4), sum_sig = c.take(n_parts * kG2J * 4), ek = c.take(n_parts * 8);
    pf = c.take((n_parts + 1) * 4), gp = c.take((G + 1) * 4), ec = c.take(2 * n_parts);
    total = c.at, total_words = total / 4;
  }
};

// blsgpu_verify_same_message, retry phase of nr sets.  d_list (words): list | message indices | iota.  d_ok (bytes):
// include | code | verdict.  d_fb, d_S, d_F (and d_G): an affine key, a Jacobian signature, an Fp12 value per set.
struct SameRetry {
  size_t msg, iota, list_words, code, ok, ok_bytes, fb_words, S_words, F_words;
  SameRetry(size_t nr) {
    Carve c, b;
    c.take(nr * 4);  // list, at 0
    msg = c.take(nr * 4) / 4, iota = c.take((nr + 1) * 4) / 4, list_words = c.end / 4;
    b.take(nr);  // include, at 0
    code = b.take(nr), ok = b.take(nr), ok_bytes = b.at;
    fb_words = nr * kG1A, S_words = nr * kG2J, F_words = nr * kFp12;
  }
};

// blsgpu_verify_same_message with BLSGPU_SAME_BLOCK_CHECK: what the block phase and the descent add, in buffers of
// their own (hl::Same and hl::SameRetry are as without the flag).  Every region starts on a 256-byte boundary.
//   block phase of nb blocks whose product tree starts `width` products wide per block, sized with the group phase's
//   buffers:
//     d_msmW (words): F_b | S_b | G_b (an Fp12, a Jacobian G2, MillerLoop(-g1, S_b) per block; stride nb) | T0 | T1 (the
//                     tree's levels in turn: nb * width Fp12, and half of that)
//     d_res (bytes):  any (the block has an included group) | ok (its check's verdict)
//   descent over nl listed groups, grown after the block phase's synchronize:
//     d_fkeep (words):   list | F | S | G (stride nl);  d_fbflags (bytes): ok
struct SameBlocks {
  size_t w_F, w_S, w_G, w_T0, w_T1, work_words, b_any, b_ok, bytes_total;
  size_t d_list, d_F, d_S, d_G, descent_words, d_ok_bytes;
  SameBlocks(size_t nb, size_t width, size_t nl) {
    Carve w, b, d;
    w_F = w.take(nb * kFp12 * 4) / 4, w_S = w.take(nb * kG2J * 4) / 4, w_G = w.take(nb * kFp12 * 4) / 4;
    w_T0 = w.take(nb * width * kFp12 * 4) / 4, w_T1 = w.take(nb * (width / 2) * kFp12 * 4) / 4;
    work_words = w.at / 4;
    b_any = b.take(nb), b_ok = b.take(nb), bytes_total = b.at;
    d_list = d.take(nl * 4) / 4, d_F = d.take(nl * kFp12 * 4) / 4, d_S = d.take(nl * kG2J * 4) / 4;
    d_G = d.take(nl * kFp12 * 4) / 4, descent_words = d.at / 4, d_ok_bytes = nl;
  }
};

// blsgpu_verify_same_message_agg: what the aggregate phase adds, in a buffer of its own (d_msmB, which no phase of the
// call uses; hl::Same, hl::SameRetry and hl::SameBlocks are as without it), sized with the group phase's buffers.  Byte
// offsets, every field on a 256-byte boundary:
//   include (a byte per set, copied up with the inputs) | sums (a Jacobian G2 per group, stride G) | counts (a word per
//   group) | out (out_len bytes per group)
struct SameAgg {
  size_t inc, sums, count, out, total, total_words;
  SameAgg(size_t G, size_t n, size_t out_len) {
    Carve c;
    inc = c.take(n), sums = c.take(G * kG2J * 4), count = c.take(G * 4), out = c.take(G * out_len);
    total = c.at, total_words = total / 4;
  }
};

// blsgpu_aggregate_verify: J jobs over n pairs, U unique messages, C planned Miller chunks (aggverify_plan.hpp).
// Items: pair k is item k, job j's (-g1, signature) item is item n + j, so the per-item arrays have stride T = n + J;
// G2 columns: unique message u is column u, job j's signature column U + j, so the per-message arrays have stride
// M = U + J.  `validate`: the keys go through KeyValidate first (kv96, b_kv).
//   d_in:    job_first | sig_len | sigs | keys | unique messages | pair message indices | chunk_first | chunk_items |
//            f_ranges (a job's chunk range) | kv96 (the validated keys, 96 bytes each)
//   d_bytes: signature status | signature flags | KeyValidate status | pair code | message flags | include | checked |
//            job code | verdict | job_result | first_bad
//   d_work:  sig_aff | pk_aff | msg_idx | f_chunk | F | message branch (msg(), M columns)
//   d_lines: the Miller lines of the M columns (lane form)
struct AggVerify {
  size_t T, M, key_bytes;
  size_t gf, len, sigs, keys, umsg, pmsg, cf, ci, fr, kv96, in_total;
  size_t b_st, b_fl, b_kv, b_code, b_mf, b_inc, b_chk, b_jcode, b_ok, b_res, b_fb, bytes_total;
  size_t w_pk_aff, w_midx, w_fchunk, w_F, w_minv, w_haff, w_hjac, w_hnorm, w_hprep, w_hq, work_words, lines_words;
  MsgBranch msg() const { return MsgBranch(w_minv, w_haff, w_hjac, w_hnorm, w_hprep, w_hq); }
  AggVerify(size_t J, size_t n, size_t U, size_t C, size_t sig_stride, bool keys_are_bytes, size_t pk_len,
            bool validate) {
    Carve c, b, w{1};
    T = n + J, M = U + J;
    key_bytes = n * (keys_are_bytes ? pk_len : 4);
    gf = c.take((J + 1) * 4), len = c.take(J * 4), sigs = c.take(J * sig_stride), keys = c.take(key_bytes);
    umsg = c.take(U * 32), pmsg = c.take(n * 4), cf = c.take((C + 1) * 4), ci = c.take(T * 4);
    fr = c.take(2 * J * 4), kv96 = c.take(validate ? n * 96 : 0), in_total = c.at;
    b_st = b.take(J), b_fl = b.take(J), b_kv = b.take(validate ? n : 0), b_code = b.take(n), b_mf = b.take(M);
    b_inc = b.take(T), b_chk = b.take(J), b_jcode = b.take(J), b_ok = b.take(J), b_res = b.take(J), b_fb = b.take(J * 4);
    bytes_total = b.at;
    w.take(J * kG2A);  // sig_aff, at 0
    w_pk_aff = w.take(T * kG1A), w_midx = w.take(T), w_fchunk = w.take(T * kFp12), w_F = w.take(J * kFp12);
    MsgBranch(w, M).put(w_minv, w_haff, w_hjac, w_hnorm, w_hprep, w_hq);
    work_words = w.end, lines_words = M * kMillerLineWords;
  }
};

// blsgpu_key_validate.  d_in: keys | out (96 bytes each) | status.
struct KeyValidate {
  size_t keys, out, st, total;
  KeyValidate(size_t n, size_t stride) {
    Carve c;
    keys = c.take(n * stride), out = c.take(n * 96), st = c.take(n), total = c.end;
  }
};

// blsgpu_pubkeys_read.  d_in: out (out_len bytes per row: the staging buffer k_pk_table_read fills 16 bytes at a time).
struct PubkeysRead {
  size_t out, total;
  PubkeysRead(size_t n, size_t out_len) {
    Carve c;
    out = c.take(n * out_len), total = c.end;
  }
};

// blsgpu_signing_roots.  d_in: objects | domains (one per object, or one for all when domain_stride is 0) | roots.
struct SigningRoots {
  size_t objects, dom, out, total, dom_bytes;
  SigningRoots(size_t n, size_t object_stride, size_t domain_stride) {
    Carve c;
    dom_bytes = (domain_stride ? n : 1) * (domain_stride ? domain_stride : 32);
    objects = c.take(n * object_stride), dom = c.take(dom_bytes), out = c.take(32 * n), total = c.end;
  }
};

}  // namespace helper_layout
