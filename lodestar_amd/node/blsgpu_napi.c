/* N-API addon over the libblsgpu C ABI (include/blsgpu.h): the binding a Lodestar maintainer loads from
 * packages/beacon-node/src/chain/bls/gpu/ (INTEGRATION.md).  It only marshals: every input array is
 * copied by blsgpu_submit() before it returns, so JS may reuse its buffers as soon as submit() returns
 * (the reference structured-clones the same data, multithread/index.ts:157-164).  Completion runs on a
 * runtime thread and is bridged to the JS main thread with a napi_threadsafe_function, where the Promise
 * resolves (or rejects on a call-level failure: a device error never becomes `false`,
 * multithread/index.ts:368-375).
 *
 * Exports:
 *   init(devices: number[] | null) -> ctx (external)             blsgpu_init
 *   close(ctx)                                                    blsgpu_destroy  (IBlsVerifier.close)
 *   deviceCount(ctx) -> number                                    blsgpu_device_count
 *   uploadPubkeys(ctx, firstIndex, Uint8Array 96*n)               blsgpu_pubkeys_upload (index2pubkey)
 *   uploadPubkeysCompressed(ctx, firstIndex, Uint8Array 48*n, validate) -> {status: Int8Array, firstBad: number}
 *     blsgpu_pubkeys_upload_compressed (synchronous; state.validators[i].pubkey as it is, decompressed on the device):
 *     a rejected key is reported (status[k] its blst code, firstBad the lowest rejected index, nothing stored;
 *     firstBad 0xffffffff = all stored), only a call-level code throws
 *   readPubkeys(ctx, firstIndex, n, outLen 48|96) -> Buffer       blsgpu_pubkeys_read (synchronous)
 *   pubkeysCount(ctx) -> number                                   blsgpu_pubkeys_count
 *   setOption(ctx, key, value)                                    blsgpu_set_option
 *   codeName(code) -> string                                      blsgpu_code_name
 *   submit(ctx, req) -> Promise<{results: Int8Array, groups, batchRetries, batchSigsSuccess, deviceMs, ...,
 *                                 urgentLane}>
 *     req = {jobFirstSet: Uint32Array, jobFlags?: Uint8Array (BLSGPU_JOB_BATCHABLE 1 | BLSGPU_JOB_URGENT 2),
 *            pkBytes?: Uint8Array,
 *            setPkFirst?: Uint32Array, pkIndex?: Uint32Array, msgs: Uint8Array, sigs: Uint8Array,
 *            sigLen: Uint32Array, sigStride: number, seed?: number}              blsgpu_submit
 *     (pkBytes alone: one 96-B key per set; pkBytes + setPkFirst: bytes-aggregate; setPkFirst + pkIndex:
 *      device table)
 *   keyValidate(ctx, Uint8Array, pkLen) -> {pk96, status}        blsgpu_key_validate (synchronous)
 *   aggregateSignatures(ctx, sigs: Uint8Array, sigLen: Uint32Array, sigStride, groupFirst: Uint32Array, validate,
 *                       outLen 96|192) -> Promise<{out: Uint8Array, status: Int8Array, firstBad: Uint32Array}>
 *     blsgpu_aggregate_signatures as napi_create_async_work: the inputs are copied before it returns, the C call
 *     runs on a libuv worker thread and the promise settles on the main thread (the event loop is never blocked).
 *     close(ctx) throws while such calls are outstanding: the JS class waits for them first.
 *   aggregateWithRandomness(ctx, groupFirst: Uint32Array, pkBytes: Uint8Array | null, pkIndex: Uint32Array | null,
 *                           sigs: Uint8Array, sigLen: Uint32Array, sigStride, seed, outPkLen 48|96, outSigLen 96|192)
 *       -> Promise<{outPk: Uint8Array, outSig: Uint8Array, status: Int8Array, firstBad: Uint32Array}>
 *     blsgpu_aggregate_with_randomness as napi_create_async_work, the same lifetime rules as aggregateSignatures
 *     (seed 0 = fresh scalars; a non-zero seed, an integer below 2^53, only for comparison runs).
 *   verifySameMessage(ctx, groupFirst: Uint32Array, msgs: Uint8Array (32 bytes per group), pkBytes: Uint8Array | null,
 *                     pkIndex: Uint32Array | null, sigs: Uint8Array, sigLen: Uint32Array, sigStride, seed, flags)
 *       -> Promise<{setResult: Int8Array, groupResult: Int8Array, stats: {groupsAccepted, groupsRetried, retrySets,
 *                   uniqueMessages, form, deviceMs}}>
 *     blsgpu_verify_same_message as napi_create_async_work, the same lifetime rules as aggregateWithRandomness.
 *     flags: BLSGPU_SAME_LANE_FORMS (1) and BLSGPU_SAME_BLOCK_CHECK (4); any other bit is a RangeError here.
 *   verifySameMessageAggregate(ctx, groupFirst, msgs, pkBytes, pkIndex, sigs, sigLen, sigStride, seed, flags,
 *                              include: Uint8Array | null (a byte per set; 0 = verified but not summed), outSigLen 96|192)
 *       -> Promise<{setResult, groupResult, stats (as verifySameMessage), outSig: Uint8Array (outSigLen bytes per group,
 *                   zeros for a group that summed nothing), aggCount: Uint32Array}>
 *     blsgpu_verify_same_message_agg as napi_create_async_work, the same lifetime rules as verifySameMessage.
 *   aggregateVerify(ctx, jobFirst: Uint32Array, msgs: Uint8Array (32 bytes per pair), pkBytes: Uint8Array | null, pkLen,
 *                   pkIndex: Uint32Array | null, sigs: Uint8Array (one per job), sigLen: Uint32Array, sigStride, flags)
 *       -> Promise<{jobResult: Int8Array, firstBad: Uint32Array, stats: {pairs, uniqueMessages, millerItems,
 *                   millerChunks, form, jobsChecked, deviceMs}}>
 *     blsgpu_aggregate_verify as napi_create_async_work, the same lifetime rules as verifySameMessage.
 *     flags: BLSGPU_AV_VALIDATE_KEYS (1, pkBytes of pkLen 48 or 96) and BLSGPU_AV_LANE_FORMS (2); any other bit, and
 *     array sizes that do not fit jobFirst, are a RangeError here.
 *   debugInject(what, skip, count)                                blsgpu_debug_inject (only with BLSGPU_FAULT_INJECTION=1)
 */
#define NAPI_VERSION 6
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "blsgpu.h"

#define CHECK(env, call)                                                   \
  do {                                                                     \
    if ((call) != napi_ok) {                                               \
      napi_throw_error((env), NULL, "blsgpu_napi: N-API call failed: " #call); \
      return NULL;                                                         \
    }                                                                      \
  } while (0)

typedef struct {
  blsgpu_ctx* ctx;
  uint32_t agg_pending; /* aggregateSignatures / aggregateWithRandomness calls queued or running (main thread only) */
} CtxBox;

typedef struct {
  int8_t* results;
  uint32_t n_jobs;
  blsgpu_stats stats;
  int status;
  napi_deferred deferred;
  napi_threadsafe_function tsfn;
} Call;

static napi_value throw_code(napi_env env, const char* what, int rc) {
  char msg[160];
  const char* name = blsgpu_code_name(rc);
  snprintf(msg, sizeof msg, "%s: %s", what, name ? name : "unknown blsgpu error");
  napi_throw_error(env, name, msg);
  return NULL;
}

static void ctx_finalize(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  CtxBox* box = (CtxBox*)data;
  if (box->ctx) blsgpu_destroy(box->ctx);
  free(box);
}

static CtxBox* get_box(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, NULL, "blsgpu_napi: expected a context from init()");
    return NULL;
  }
  return (CtxBox*)p;
}

static CtxBox* get_open_box(napi_env env, napi_value v) {
  CtxBox* box = get_box(env, v);
  if (box && !box->ctx) {
    throw_code(env, "blsgpu", BLSGPU_ERR_CLOSED);
    return NULL;
  }
  return box;
}

static napi_value Init(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int devs[64];
  int n = 0;
  if (argc >= 1) {
    bool is_arr = false;
    napi_is_array(env, argv[0], &is_arr);
    if (is_arr) {
      uint32_t len = 0;
      CHECK(env, napi_get_array_length(env, argv[0], &len));
      for (uint32_t i = 0; i < len && n < 64; i++) {
        napi_value e;
        CHECK(env, napi_get_element(env, argv[0], i, &e));
        int32_t d;
        CHECK(env, napi_get_value_int32(env, e, &d));
        devs[n++] = d;
      }
    }
  }
  blsgpu_ctx* ctx = NULL;
  int rc = blsgpu_init(n ? devs : NULL, n, &ctx);
  if (rc != BLSGPU_OK) return throw_code(env, "blsgpu_init", rc);
  CtxBox* box = (CtxBox*)calloc(1, sizeof(CtxBox));
  box->ctx = ctx;
  napi_value out;
  CHECK(env, napi_create_external(env, box, ctx_finalize, NULL, &out));
  return out;
}

static napi_value Close(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  CtxBox* box = get_box(env, argv[0]);
  if (!box) return NULL;
  if (box->ctx && box->agg_pending) {
    /* a queued worker still holds the context: destroying it now would free it under that call */
    napi_throw_error(env, "BLSGPU_ERR_ARGS", "close: aggregation calls are outstanding");
    return NULL;
  }
  if (box->ctx) {
    /* waits for in-flight submissions (their callbacks are queued on the tsfn), fails queued ones */
    blsgpu_destroy(box->ctx);
    box->ctx = NULL;
  }
  return NULL;
}

static napi_value DeviceCount(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  napi_value out;
  CHECK(env, napi_create_int32(env, blsgpu_device_count(box->ctx), &out));
  return out;
}

static int get_typed(napi_env env, napi_value obj, const char* key, napi_typedarray_type want, void** data,
                     size_t* len, int required) {
  bool has = false;
  *data = NULL;
  *len = 0;
  if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return required ? -1 : 0;
  napi_value v;
  napi_get_named_property(env, obj, key, &v);
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t == napi_undefined || t == napi_null) return required ? -1 : 0;
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (!is_ta) return -1;
  napi_typedarray_type type;
  napi_value ab;
  size_t off;
  if (napi_get_typedarray_info(env, v, &type, len, data, &ab, &off) != napi_ok) return -1;
  if (type != want) return -1;
  return 1;
}

static napi_value UploadPubkeys(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  uint32_t first;
  CHECK(env, napi_get_value_uint32(env, argv[1], &first));
  napi_typedarray_type type;
  size_t len;
  void* data;
  napi_value ab;
  size_t off;
  if (napi_get_typedarray_info(env, argv[2], &type, &len, &data, &ab, &off) != napi_ok || type != napi_uint8_array ||
      len % 96) {
    napi_throw_type_error(env, NULL, "uploadPubkeys: expected a Uint8Array of 96-byte uncompressed pubkeys");
    return NULL;
  }
  int rc = blsgpu_pubkeys_upload(box->ctx, first, (const uint8_t*)data, (uint32_t)(len / 96));
  if (rc != BLSGPU_OK) return throw_code(env, "uploadPubkeys", rc);
  return NULL;
}

/* uploadPubkeysCompressed(ctx, firstIndex, Uint8Array 48*n, validate) -> {status: Int8Array, firstBad}  (synchronous) */
static napi_value UploadPubkeysCompressed(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "uploadPubkeysCompressed(ctx, firstIndex, pk48, validate)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  uint32_t first;
  CHECK(env, napi_get_value_uint32(env, argv[1], &first));
  napi_typedarray_type type;
  size_t len = 0;
  void* data = NULL;
  if (napi_get_typedarray_info(env, argv[2], &type, &len, &data, NULL, NULL) != napi_ok || type != napi_uint8_array ||
      len % 48) {
    napi_throw_type_error(env, NULL, "uploadPubkeysCompressed: expected a Uint8Array of 48-byte compressed pubkeys");
    return NULL;
  }
  bool validate = false;
  if (argc >= 4) napi_coerce_to_bool(env, argv[3], &argv[3]), napi_get_value_bool(env, argv[3], &validate);
  uint32_t n = (uint32_t)(len / 48), first_bad = 0xffffffffu;
  napi_value ab_st, st, fb, out;
  void* p_st = NULL;
  CHECK(env, napi_create_arraybuffer(env, n ? n : 1, &p_st, &ab_st));
  memset(p_st, 0, n ? n : 1);
  int rc = blsgpu_pubkeys_upload_compressed(box->ctx, first, (const uint8_t*)data, n, validate ? BLSGPU_PK_VALIDATE : 0,
                                            (int8_t*)p_st, &first_bad);
  if (rc >= BLSGPU_ERR_ARGS || rc == BLSGPU_DEVICE_ERROR) return throw_code(env, "uploadPubkeysCompressed", rc);
  CHECK(env, napi_create_typedarray(env, napi_int8_array, n, ab_st, 0, &st));
  CHECK(env, napi_create_uint32(env, first_bad, &fb));
  CHECK(env, napi_create_object(env, &out));
  napi_set_named_property(env, out, "status", st);
  napi_set_named_property(env, out, "firstBad", fb);
  return out;
}

/* readPubkeys(ctx, firstIndex, n, outLen 48|96) -> Buffer of n * outLen bytes  (synchronous) */
static napi_value ReadPubkeys(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4) {
    napi_throw_type_error(env, NULL, "readPubkeys(ctx, firstIndex, n, outLen)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  uint32_t first = 0, n = 0, out_len = 0;
  CHECK(env, napi_get_value_uint32(env, argv[1], &first));
  CHECK(env, napi_get_value_uint32(env, argv[2], &n));
  CHECK(env, napi_get_value_uint32(env, argv[3], &out_len));
  if (out_len != 48 && out_len != 96) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "readPubkeys: outLen must be 48 or 96");
    return NULL;
  }
  /* the range is checked before anything of its size is allocated (the library checks it again under its lock) */
  if (n && (uint64_t)first + n > blsgpu_pubkeys_count(box->ctx)) return throw_code(env, "readPubkeys", BLSGPU_ERR_ARGS);
  napi_value buf;
  void* p = NULL;
  CHECK(env, napi_create_buffer(env, (size_t)n * out_len, &p, &buf));
  int rc = blsgpu_pubkeys_read(box->ctx, first, n, (uint8_t*)p, out_len);
  if (rc != BLSGPU_OK) return throw_code(env, "readPubkeys", rc);
  return buf;
}

static napi_value PubkeysCount(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  napi_value out;
  CHECK(env, napi_create_uint32(env, blsgpu_pubkeys_count(box->ctx), &out));
  return out;
}

static napi_value SetOption(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  char key[64];
  size_t kl;
  CHECK(env, napi_get_value_string_utf8(env, argv[1], key, sizeof key, &kl));
  int64_t value;
  CHECK(env, napi_get_value_int64(env, argv[2], &value));
  int rc = blsgpu_set_option(box->ctx, key, value);
  if (rc != BLSGPU_OK) return throw_code(env, "setOption", rc);
  return NULL;
}

static napi_value GetOption(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  char key[64];
  size_t kl;
  CHECK(env, napi_get_value_string_utf8(env, argv[1], key, sizeof key, &kl));
  int64_t value = 0;
  int rc = blsgpu_get_option(box->ctx, key, &value);
  if (rc != BLSGPU_OK) return throw_code(env, "getOption", rc);
  napi_value out;
  CHECK(env, napi_create_int64(env, value, &out));
  return out;
}

static napi_value CodeName(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t code;
  CHECK(env, napi_get_value_int32(env, argv[0], &code));
  const char* name = blsgpu_code_name(code);
  napi_value out;
  if (!name) {
    CHECK(env, napi_get_null(env, &out));
  } else {
    CHECK(env, napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &out));
  }
  return out;
}

/* runtime thread */
static void on_done(void* user, int status) {
  Call* c = (Call*)user;
  c->status = status;
  napi_call_threadsafe_function(c->tsfn, c, napi_tsfn_blocking);
}

static void set_num(napi_env env, napi_value obj, const char* key, double v) {
  napi_value x;
  napi_create_double(env, v, &x);
  napi_set_named_property(env, obj, key, x);
}

/* JS main thread */
static void settle_on_main(napi_env env, napi_value js_cb, void* context, void* data) {
  (void)js_cb;
  (void)context;
  Call* c = (Call*)data;
  if (env != NULL) {
    if (c->status != BLSGPU_OK) {
      const char* name = blsgpu_code_name(c->status);
      napi_value msg, code, err;
      napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &msg);
      napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &code);
      napi_create_error(env, code, msg, &err);
      napi_reject_deferred(env, c->deferred, err);
    } else {
      napi_value out, ab, arr;
      void* dst;
      napi_create_object(env, &out);
      napi_create_arraybuffer(env, c->n_jobs, &dst, &ab);
      if (c->n_jobs) memcpy(dst, c->results, c->n_jobs);
      napi_create_typedarray(env, napi_int8_array, c->n_jobs, ab, 0, &arr);
      napi_set_named_property(env, out, "results", arr);
      set_num(env, out, "groups", c->stats.groups);
      set_num(env, out, "batchRetries", c->stats.batch_retries);
      set_num(env, out, "batchSigsSuccess", c->stats.batch_sigs_success);
      set_num(env, out, "devicesUsed", c->stats.devices_used);
      set_num(env, out, "deviceMs", c->stats.device_ms);
      set_num(env, out, "uniqueMessages", c->stats.unique_messages);
      set_num(env, out, "pairingUnits", c->stats.pairing_units);
      set_num(env, out, "urgentLane", c->stats.urgent_lane);
      napi_resolve_deferred(env, c->deferred, out);
    }
  }
  napi_release_threadsafe_function(c->tsfn, napi_tsfn_release);
  free(c->results);
  free(c);
}

static napi_value Submit(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) {
    napi_throw_type_error(env, NULL, "submit(ctx, req)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  napi_value req = argv[1];
  void *jfs, *flags, *pkb, *spf, *pki, *msgs, *sigs, *slen;
  size_t n_jfs, n_flags, n_pkb, n_spf, n_pki, n_msgs, n_sigs, n_slen;
  if (get_typed(env, req, "jobFirstSet", napi_uint32_array, &jfs, &n_jfs, 1) < 0 || n_jfs < 1 ||
      get_typed(env, req, "jobFlags", napi_uint8_array, &flags, &n_flags, 0) < 0 ||
      get_typed(env, req, "pkBytes", napi_uint8_array, &pkb, &n_pkb, 0) < 0 ||
      get_typed(env, req, "setPkFirst", napi_uint32_array, &spf, &n_spf, 0) < 0 ||
      get_typed(env, req, "pkIndex", napi_uint32_array, &pki, &n_pki, 0) < 0 ||
      get_typed(env, req, "msgs", napi_uint8_array, &msgs, &n_msgs, 1) < 0 ||
      get_typed(env, req, "sigs", napi_uint8_array, &sigs, &n_sigs, 1) < 0 ||
      get_typed(env, req, "sigLen", napi_uint32_array, &slen, &n_slen, 1) < 0) {
    napi_throw_type_error(env, NULL, "submit: malformed request (typed arrays expected)");
    return NULL;
  }
  uint32_t stride = 192;
  napi_value v;
  bool has = false;
  if (napi_has_named_property(env, req, "sigStride", &has) == napi_ok && has) {
    napi_get_named_property(env, req, "sigStride", &v);
    napi_get_value_uint32(env, v, &stride);
  }
  double seed_d = 0;
  if (napi_has_named_property(env, req, "seed", &has) == napi_ok && has) {
    napi_get_named_property(env, req, "seed", &v);
    napi_get_value_double(env, v, &seed_d);
  }
  uint32_t n_jobs = (uint32_t)n_jfs - 1, n_sets = (uint32_t)n_slen;
  /* shape checks on the host before anything reaches the device */
  int ok = ((const uint32_t*)jfs)[n_jobs] == n_sets && n_msgs == 32ull * n_sets &&
           n_sigs >= (size_t)stride * n_sets && (!flags || n_flags == n_jobs);
  if (pkb && !spf) ok = ok && n_pkb == 96ull * n_sets;  /* one key per set */
  else if (pkb) ok = ok && n_spf == n_sets + 1ull && 96ull * ((const uint32_t*)spf)[n_sets] <= n_pkb;  /* bytes aggregate */
  else ok = ok && spf && n_spf == n_sets + 1ull && ((const uint32_t*)spf)[n_sets] <= n_pki;  /* device table */
  if (!ok) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "submit: inconsistent array sizes");
    return NULL;
  }
  blsgpu_batch b;
  memset(&b, 0, sizeof b);
  b.n_sets = n_sets;
  b.n_jobs = n_jobs;
  b.job_first_set = (const uint32_t*)jfs;
  b.job_flags = (const uint8_t*)flags;
  b.pk_bytes = (const uint8_t*)pkb;
  b.set_pk_first = (const uint32_t*)spf;
  b.pk_index = (const uint32_t*)pki;
  b.msgs = (const uint8_t*)msgs;
  b.sigs = (const uint8_t*)sigs;
  b.sig_len = (const uint32_t*)slen;
  b.sig_stride = stride;
  b.seed = (uint64_t)seed_d; /* 0 = OS CSPRNG scalars (production) */

  Call* c = (Call*)calloc(1, sizeof(Call));
  c->n_jobs = n_jobs;
  c->results = (int8_t*)calloc(n_jobs ? n_jobs : 1, 1);
  napi_value promise, name;
  CHECK(env, napi_create_promise(env, &c->deferred, &promise));
  CHECK(env, napi_create_string_utf8(env, "blsgpu_submit", NAPI_AUTO_LENGTH, &name));
  CHECK(env, napi_create_threadsafe_function(env, NULL, NULL, name, 0, 1, NULL, NULL, NULL, settle_on_main,
                                             &c->tsfn));
  int rc = blsgpu_submit(box->ctx, &b, c->results, &c->stats, on_done, c);
  if (rc != BLSGPU_OK) {
    /* nothing was queued: settle synchronously through the same path */
    c->status = rc;
    settle_on_main(env, NULL, NULL, c);
  }
  return promise;
}

/* keyValidate(ctx, Uint8Array pks, pkLen 48|96) -> {pk96: Uint8Array, status: Int8Array}  (synchronous) */
static napi_value KeyValidate(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "keyValidate(ctx, pks, pkLen)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  napi_typedarray_type t;
  size_t len = 0;
  void* data = NULL;
  if (napi_get_typedarray_info(env, argv[1], &t, &len, &data, NULL, NULL) != napi_ok || t != napi_uint8_array) {
    napi_throw_type_error(env, NULL, "keyValidate: pks must be a Uint8Array");
    return NULL;
  }
  uint32_t pk_len = 0;
  napi_get_value_uint32(env, argv[2], &pk_len);
  if ((pk_len != 48 && pk_len != 96) || len % pk_len) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "keyValidate: pkLen must be 48 or 96 and divide the input");
    return NULL;
  }
  uint32_t n = (uint32_t)(len / pk_len);
  napi_value ab_pk, ab_st, pk96, st, out;
  void *p_pk = NULL, *p_st = NULL;
  CHECK(env, napi_create_arraybuffer(env, 96 * (size_t)n, &p_pk, &ab_pk));
  CHECK(env, napi_create_arraybuffer(env, n ? n : 1, &p_st, &ab_st));
  int rc = blsgpu_key_validate(box->ctx, n, (const uint8_t*)data, pk_len, pk_len, (uint8_t*)p_pk, (int8_t*)p_st);
  if (rc != BLSGPU_OK) return throw_code(env, "blsgpu_key_validate", rc);
  CHECK(env, napi_create_typedarray(env, napi_uint8_array, 96 * (size_t)n, ab_pk, 0, &pk96));
  CHECK(env, napi_create_typedarray(env, napi_int8_array, n, ab_st, 0, &st));
  CHECK(env, napi_create_object(env, &out));
  napi_set_named_property(env, out, "pk96", pk96);
  napi_set_named_property(env, out, "status", st);
  return out;
}

/* aggregateSignatures: one blsgpu_aggregate_signatures call as async work */
typedef struct {
  CtxBox* box;
  uint32_t n_groups, stride, flags, out_len;
  uint32_t* group_first;
  uint32_t* sig_len;
  uint8_t* sigs;
  uint8_t* out;
  int8_t* status;
  uint32_t* first_bad;
  int rc;
  napi_deferred deferred;
  napi_async_work work;
} AggCall;

static void agg_free(AggCall* a) {
  free(a->group_first);
  free(a->sig_len);
  free(a->sigs);
  free(a->out);
  free(a->status);
  free(a->first_bad);
  free(a);
}

/* libuv worker thread */
static void agg_execute(napi_env env, void* data) {
  (void)env;
  AggCall* a = (AggCall*)data;
  a->rc = blsgpu_aggregate_signatures(a->box->ctx, a->n_groups, a->group_first, a->sigs, a->stride, a->sig_len,
                                      a->flags, a->out, a->out_len, a->status, a->first_bad);
}

static napi_value copy_out(napi_env env, napi_typedarray_type type, const void* src, size_t count, size_t elem) {
  napi_value ab, arr;
  void* dst = NULL;
  napi_create_arraybuffer(env, count * elem, &dst, &ab);
  if (count) memcpy(dst, src, count * elem);
  napi_create_typedarray(env, type, count, ab, 0, &arr);
  return arr;
}

/* JS main thread */
static void agg_complete(napi_env env, napi_status st, void* data) {
  AggCall* a = (AggCall*)data;
  a->box->agg_pending--;
  if (st != napi_ok || a->rc != BLSGPU_OK) {
    const char* name = blsgpu_code_name(st != napi_ok ? BLSGPU_ERR_CLOSED : a->rc);
    napi_value msg, code, err;
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &msg);
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &code);
    napi_create_error(env, code, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
  } else {
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "out", copy_out(env, napi_uint8_array, a->out, (size_t)a->n_groups * a->out_len, 1));
    napi_set_named_property(env, out, "status", copy_out(env, napi_int8_array, a->status, a->n_groups, 1));
    napi_set_named_property(env, out, "firstBad", copy_out(env, napi_uint32_array, a->first_bad, a->n_groups, 4));
    napi_resolve_deferred(env, a->deferred, out);
  }
  napi_delete_async_work(env, a->work);
  agg_free(a);
}

static void* dup_bytes(const void* src, size_t n) {
  void* p = malloc(n ? n : 1);
  if (p && n) memcpy(p, src, n);
  return p;
}

static napi_value AggregateSignatures(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 7) {
    napi_throw_type_error(env, NULL, "aggregateSignatures(ctx, sigs, sigLen, sigStride, groupFirst, validate, outLen)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  napi_typedarray_type t_sigs, t_len, t_gf;
  size_t n_bytes = 0, n_len = 0, n_gf = 0;
  void *sigs = NULL, *slen = NULL, *gf = NULL;
  if (napi_get_typedarray_info(env, argv[1], &t_sigs, &n_bytes, &sigs, NULL, NULL) != napi_ok ||
      t_sigs != napi_uint8_array ||
      napi_get_typedarray_info(env, argv[2], &t_len, &n_len, &slen, NULL, NULL) != napi_ok ||
      t_len != napi_uint32_array ||
      napi_get_typedarray_info(env, argv[4], &t_gf, &n_gf, &gf, NULL, NULL) != napi_ok || t_gf != napi_uint32_array) {
    napi_throw_type_error(env, NULL, "aggregateSignatures: sigs Uint8Array, sigLen and groupFirst Uint32Array expected");
    return NULL;
  }
  uint32_t stride = 0, out_len = 0;
  bool validate = true;
  napi_get_value_uint32(env, argv[3], &stride);
  napi_coerce_to_bool(env, argv[5], &argv[5]);
  napi_get_value_bool(env, argv[5], &validate);
  napi_get_value_uint32(env, argv[6], &out_len);
  /* shape checks on the host before anything is queued */
  int ok = n_gf >= 1 && stride >= 96 && (out_len == 96 || out_len == 192) && ((const uint32_t*)gf)[0] == 0;
  for (size_t g = 0; ok && g + 1 < n_gf; g++) ok = ((const uint32_t*)gf)[g + 1] >= ((const uint32_t*)gf)[g];
  ok = ok && ((const uint32_t*)gf)[n_gf - 1] == n_len && n_len <= (1u << 20) && n_bytes >= (size_t)stride * n_len;
  for (size_t k = 0; ok && stride < 192 && k < n_len; k++) ok = ((const uint32_t*)slen)[k] != 192;
  if (!ok) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "aggregateSignatures: inconsistent array sizes");
    return NULL;
  }
  AggCall* a = (AggCall*)calloc(1, sizeof(AggCall));
  a->box = box;
  a->n_groups = (uint32_t)n_gf - 1;
  a->stride = stride;
  a->flags = validate ? BLSGPU_AGG_VALIDATE : 0;
  a->out_len = out_len;
  a->group_first = (uint32_t*)dup_bytes(gf, n_gf * 4);
  a->sig_len = (uint32_t*)dup_bytes(slen, n_len * 4);
  a->sigs = (uint8_t*)dup_bytes(sigs, (size_t)stride * n_len);
  a->out = (uint8_t*)calloc((size_t)a->n_groups * out_len + 1, 1);
  a->status = (int8_t*)calloc((size_t)a->n_groups + 1, 1);
  a->first_bad = (uint32_t*)calloc((size_t)a->n_groups + 1, 4);
  napi_value promise, name;
  if (!a->group_first || !a->sig_len || !a->sigs || !a->out || !a->status || !a->first_bad ||
      napi_create_promise(env, &a->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu_aggregate_signatures", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, agg_execute, agg_complete, a, &a->work) != napi_ok) {
    agg_free(a);
    napi_throw_error(env, NULL, "aggregateSignatures: could not queue the call");
    return NULL;
  }
  box->agg_pending++;
  if (napi_queue_async_work(env, a->work) != napi_ok) {
    box->agg_pending--;
    napi_delete_async_work(env, a->work);
    agg_free(a);
    napi_throw_error(env, NULL, "aggregateSignatures: could not queue the call");
    return NULL;
  }
  return promise;
}

/* aggregateWithRandomness: one blsgpu_aggregate_with_randomness call as async work */
typedef struct {
  CtxBox* box;
  uint32_t n_groups, stride, out_pk_len, out_sig_len;
  uint64_t seed;
  uint32_t* group_first;
  uint8_t* pk_bytes;
  uint32_t* pk_index;
  uint32_t* sig_len;
  uint8_t* sigs;
  uint8_t* out_pk;
  uint8_t* out_sig;
  int8_t* status;
  uint32_t* first_bad;
  int rc;
  napi_deferred deferred;
  napi_async_work work;
} AwrCall;

static void awr_free(AwrCall* a) {
  free(a->group_first);
  free(a->pk_bytes);
  free(a->pk_index);
  free(a->sig_len);
  free(a->sigs);
  free(a->out_pk);
  free(a->out_sig);
  free(a->status);
  free(a->first_bad);
  free(a);
}

/* libuv worker thread */
static void awr_execute(napi_env env, void* data) {
  (void)env;
  AwrCall* a = (AwrCall*)data;
  a->rc = blsgpu_aggregate_with_randomness(a->box->ctx, a->n_groups, a->group_first, a->pk_bytes, a->pk_index, a->sigs,
                                           a->stride, a->sig_len, a->seed, a->out_pk, a->out_pk_len, a->out_sig,
                                           a->out_sig_len, a->status, a->first_bad);
}

/* JS main thread */
static void awr_complete(napi_env env, napi_status st, void* data) {
  AwrCall* a = (AwrCall*)data;
  a->box->agg_pending--;
  if (st != napi_ok || a->rc != BLSGPU_OK) {
    const char* name = blsgpu_code_name(st != napi_ok ? BLSGPU_ERR_CLOSED : a->rc);
    napi_value msg, code, err;
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &msg);
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &code);
    napi_create_error(env, code, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
  } else {
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "outPk",
                            copy_out(env, napi_uint8_array, a->out_pk, (size_t)a->n_groups * a->out_pk_len, 1));
    napi_set_named_property(env, out, "outSig",
                            copy_out(env, napi_uint8_array, a->out_sig, (size_t)a->n_groups * a->out_sig_len, 1));
    napi_set_named_property(env, out, "status", copy_out(env, napi_int8_array, a->status, a->n_groups, 1));
    napi_set_named_property(env, out, "firstBad", copy_out(env, napi_uint32_array, a->first_bad, a->n_groups, 4));
    napi_resolve_deferred(env, a->deferred, out);
  }
  napi_delete_async_work(env, a->work);
  awr_free(a);
}

/* a typed array of the wanted type, or null / undefined (*data stays NULL); -1 = anything else */
static int opt_typed(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* len) {
  napi_valuetype vt;
  *data = NULL;
  *len = 0;
  if (napi_typeof(env, v, &vt) != napi_ok) return -1;
  if (vt == napi_null || vt == napi_undefined) return 0;
  napi_typedarray_type t;
  if (napi_get_typedarray_info(env, v, &t, len, data, NULL, NULL) != napi_ok || t != want) return -1;
  if (!*data) *data = (void*)""; /* an empty array is still "given" */
  return 0;
}

static napi_value AggregateWithRandomness(napi_env env, napi_callback_info info) {
  size_t argc = 10;
  napi_value argv[10];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 10) {
    napi_throw_type_error(env, NULL,
                          "aggregateWithRandomness(ctx, groupFirst, pkBytes, pkIndex, sigs, sigLen, sigStride, seed, "
                          "outPkLen, outSigLen)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  size_t n_gf = 0, n_pkb = 0, n_pki = 0, n_bytes = 0, n_len = 0;
  void *gf = NULL, *pkb = NULL, *pki = NULL, *sigs = NULL, *slen = NULL;
  if (opt_typed(env, argv[1], napi_uint32_array, &gf, &n_gf) || !gf ||
      opt_typed(env, argv[2], napi_uint8_array, &pkb, &n_pkb) ||
      opt_typed(env, argv[3], napi_uint32_array, &pki, &n_pki) ||
      opt_typed(env, argv[4], napi_uint8_array, &sigs, &n_bytes) || !sigs ||
      opt_typed(env, argv[5], napi_uint32_array, &slen, &n_len) || !slen) {
    napi_throw_type_error(env, NULL,
                          "aggregateWithRandomness: groupFirst, pkIndex, sigLen Uint32Array; pkBytes, sigs Uint8Array");
    return NULL;
  }
  uint32_t stride = 0, out_pk_len = 0, out_sig_len = 0;
  double seed = 0;
  napi_get_value_uint32(env, argv[6], &stride);
  napi_get_value_double(env, argv[7], &seed);
  napi_get_value_uint32(env, argv[8], &out_pk_len);
  napi_get_value_uint32(env, argv[9], &out_sig_len);
  /* shape checks on the host before anything is queued */
  const uint32_t* gfw = (const uint32_t*)gf;
  int ok = n_gf >= 1 && stride >= 96 && (out_pk_len == 48 || out_pk_len == 96) &&
           (out_sig_len == 96 || out_sig_len == 192) && gfw[0] == 0 && (pkb != NULL) != (pki != NULL) && seed >= 0 &&
           seed < 9007199254740992.0;
  for (size_t g = 0; ok && g + 1 < n_gf; g++) ok = gfw[g + 1] >= gfw[g];
  ok = ok && gfw[n_gf - 1] == n_len && n_len <= (1u << 20) && n_bytes >= (size_t)stride * n_len;
  ok = ok && (pkb ? n_pkb == 96 * n_len : n_pki == n_len);
  for (size_t k = 0; ok && stride < 192 && k < n_len; k++) ok = ((const uint32_t*)slen)[k] != 192;
  if (!ok) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "aggregateWithRandomness: inconsistent array sizes");
    return NULL;
  }
  AwrCall* a = (AwrCall*)calloc(1, sizeof(AwrCall));
  a->box = box;
  a->n_groups = (uint32_t)n_gf - 1;
  a->stride = stride;
  a->out_pk_len = out_pk_len;
  a->out_sig_len = out_sig_len;
  a->seed = (uint64_t)seed;
  a->group_first = (uint32_t*)dup_bytes(gf, n_gf * 4);
  if (pkb) a->pk_bytes = (uint8_t*)dup_bytes(pkb, n_pkb);
  if (pki) a->pk_index = (uint32_t*)dup_bytes(pki, n_pki * 4);
  a->sig_len = (uint32_t*)dup_bytes(slen, n_len * 4);
  a->sigs = (uint8_t*)dup_bytes(sigs, (size_t)stride * n_len);
  a->out_pk = (uint8_t*)calloc((size_t)a->n_groups * out_pk_len + 1, 1);
  a->out_sig = (uint8_t*)calloc((size_t)a->n_groups * out_sig_len + 1, 1);
  a->status = (int8_t*)calloc((size_t)a->n_groups + 1, 1);
  a->first_bad = (uint32_t*)calloc((size_t)a->n_groups + 1, 4);
  napi_value promise, name;
  if (!a->group_first || (!a->pk_bytes && !a->pk_index) || !a->sig_len || !a->sigs || !a->out_pk || !a->out_sig ||
      !a->status || !a->first_bad || napi_create_promise(env, &a->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu_aggregate_with_randomness", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, awr_execute, awr_complete, a, &a->work) != napi_ok) {
    awr_free(a);
    napi_throw_error(env, NULL, "aggregateWithRandomness: could not queue the call");
    return NULL;
  }
  box->agg_pending++;
  if (napi_queue_async_work(env, a->work) != napi_ok) {
    box->agg_pending--;
    napi_delete_async_work(env, a->work);
    awr_free(a);
    napi_throw_error(env, NULL, "aggregateWithRandomness: could not queue the call");
    return NULL;
  }
  return promise;
}

/* verifySameMessage: one blsgpu_verify_same_message call as async work (lifetimes as aggregateWithRandomness: every
 * input is copied before the call returns, the outputs are the call's own until its completion on the main thread, and
 * the context stays open while the call is pending -- close() waits for agg_pending) */
typedef struct {
  CtxBox* box;
  uint32_t n_groups, n_sets, stride, flags;
  uint64_t seed;
  uint32_t* group_first;
  uint8_t* msgs;
  uint8_t* pk_bytes;
  uint32_t* pk_index;
  uint32_t* sig_len;
  uint8_t* sigs;
  int8_t* set_result;
  int8_t* group_result;
  /* verifySameMessageAggregate only (agg): the mask (nullable), the groups' aggregates and their counts */
  int agg;
  uint32_t out_sig_len;
  uint8_t* include;
  uint8_t* out_sig;
  uint32_t* agg_count;
  blsgpu_same_message_stats stats;
  int rc;
  napi_deferred deferred;
  napi_async_work work;
} SameCall;

static void same_free(SameCall* a) {
  free(a->group_first);
  free(a->msgs);
  free(a->pk_bytes);
  free(a->pk_index);
  free(a->sig_len);
  free(a->sigs);
  free(a->set_result);
  free(a->group_result);
  free(a->include);
  free(a->out_sig);
  free(a->agg_count);
  free(a);
}

/* libuv worker thread */
static void same_execute(napi_env env, void* data) {
  (void)env;
  SameCall* a = (SameCall*)data;
  if (a->agg) {
    a->rc = blsgpu_verify_same_message_agg(a->box->ctx, a->n_groups, a->group_first, a->msgs, a->pk_bytes, a->pk_index,
                                           a->sigs, a->stride, a->sig_len, a->seed, a->flags, a->set_result,
                                           a->group_result, &a->stats, a->include, a->out_sig, a->out_sig_len,
                                           a->agg_count);
    return;
  }
  a->rc = blsgpu_verify_same_message(a->box->ctx, a->n_groups, a->group_first, a->msgs, a->pk_bytes, a->pk_index,
                                     a->sigs, a->stride, a->sig_len, a->seed, a->flags, a->set_result, a->group_result,
                                     &a->stats);
}

static void set_u32(napi_env env, napi_value obj, const char* key, uint32_t v) {
  napi_value x;
  napi_create_uint32(env, v, &x);
  napi_set_named_property(env, obj, key, x);
}

/* JS main thread */
static void same_complete(napi_env env, napi_status st, void* data) {
  SameCall* a = (SameCall*)data;
  a->box->agg_pending--;
  if (st != napi_ok || a->rc != BLSGPU_OK) {
    const char* name = blsgpu_code_name(st != napi_ok ? BLSGPU_ERR_CLOSED : a->rc);
    napi_value msg, code, err;
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &msg);
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &code);
    napi_create_error(env, code, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
  } else {
    napi_value out, stats, ms;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "setResult", copy_out(env, napi_int8_array, a->set_result, a->n_sets, 1));
    napi_set_named_property(env, out, "groupResult", copy_out(env, napi_int8_array, a->group_result, a->n_groups, 1));
    napi_create_object(env, &stats);
    set_u32(env, stats, "groupsAccepted", a->stats.groups_accepted);
    set_u32(env, stats, "groupsRetried", a->stats.groups_retried);
    set_u32(env, stats, "retrySets", a->stats.retry_sets);
    set_u32(env, stats, "uniqueMessages", a->stats.unique_messages);
    set_u32(env, stats, "form", a->stats.form);
    napi_create_double(env, a->stats.device_ms, &ms);
    napi_set_named_property(env, stats, "deviceMs", ms);
    napi_set_named_property(env, out, "stats", stats);
    if (a->agg) {
      napi_set_named_property(env, out, "outSig",
                              copy_out(env, napi_uint8_array, a->out_sig, (size_t)a->n_groups * a->out_sig_len, 1));
      napi_set_named_property(env, out, "aggCount", copy_out(env, napi_uint32_array, a->agg_count, a->n_groups, 4));
    }
    napi_resolve_deferred(env, a->deferred, out);
  }
  napi_delete_async_work(env, a->work);
  same_free(a);
}

/* verifySameMessage (agg 0: ten arguments) and verifySameMessageAggregate (agg 1: include and outSigLen after them) */
static napi_value verify_same_message_call(napi_env env, napi_callback_info info, int agg) {
  size_t argc = 12;
  napi_value argv[12];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < (agg ? 12u : 10u)) {
    napi_throw_type_error(env, NULL,
                          agg ? "verifySameMessageAggregate(ctx, groupFirst, msgs, pkBytes, pkIndex, sigs, sigLen, "
                                "sigStride, seed, flags, include, outSigLen)"
                              : "verifySameMessage(ctx, groupFirst, msgs, pkBytes, pkIndex, sigs, sigLen, sigStride, "
                                "seed, flags)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  size_t n_gf = 0, n_msg = 0, n_pkb = 0, n_pki = 0, n_bytes = 0, n_len = 0;
  void *gf = NULL, *msgs = NULL, *pkb = NULL, *pki = NULL, *sigs = NULL, *slen = NULL;
  if (opt_typed(env, argv[1], napi_uint32_array, &gf, &n_gf) || !gf ||
      opt_typed(env, argv[2], napi_uint8_array, &msgs, &n_msg) || !msgs ||
      opt_typed(env, argv[3], napi_uint8_array, &pkb, &n_pkb) ||
      opt_typed(env, argv[4], napi_uint32_array, &pki, &n_pki) ||
      opt_typed(env, argv[5], napi_uint8_array, &sigs, &n_bytes) || !sigs ||
      opt_typed(env, argv[6], napi_uint32_array, &slen, &n_len) || !slen) {
    napi_throw_type_error(env, NULL,
                          "verifySameMessage: groupFirst, pkIndex, sigLen Uint32Array; msgs, pkBytes, sigs Uint8Array");
    return NULL;
  }
  size_t n_inc = 0;
  void* inc = NULL;
  uint32_t out_sig_len = 0;
  if (agg) {
    if (opt_typed(env, argv[10], napi_uint8_array, &inc, &n_inc)) {
      napi_throw_type_error(env, NULL, "verifySameMessageAggregate: include is a Uint8Array or null");
      return NULL;
    }
    napi_get_value_uint32(env, argv[11], &out_sig_len);
  }
  uint32_t stride = 0, flags = 0;
  double seed = 0;
  napi_get_value_uint32(env, argv[7], &stride);
  napi_get_value_double(env, argv[8], &seed);
  napi_get_value_uint32(env, argv[9], &flags);
  /* shape checks on the host before anything is queued */
  const uint32_t* gfw = (const uint32_t*)gf;
  int ok = n_gf >= 1 && stride >= 96 && !(flags & ~(BLSGPU_SAME_LANE_FORMS | BLSGPU_SAME_BLOCK_CHECK)) && gfw[0] == 0 &&
           (pkb != NULL) != (pki != NULL) && seed >= 0 && seed < 9007199254740992.0 && n_msg == 32 * (n_gf - 1);
  for (size_t g = 0; ok && g + 1 < n_gf; g++) ok = gfw[g + 1] >= gfw[g];
  ok = ok && gfw[n_gf - 1] == n_len && n_len <= (1u << 20) && n_bytes >= (size_t)stride * n_len;
  ok = ok && (pkb ? n_pkb == 96 * n_len : n_pki == n_len);
  for (size_t k = 0; ok && stride < 192 && k < n_len; k++) ok = ((const uint32_t*)slen)[k] != 192;
  if (agg) ok = ok && (out_sig_len == 96 || out_sig_len == 192) && (!inc || n_inc == n_len);
  if (!ok) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "verifySameMessage: inconsistent array sizes");
    return NULL;
  }
  SameCall* a = (SameCall*)calloc(1, sizeof(SameCall));
  if (!a) {
    napi_throw_error(env, NULL, "verifySameMessage: could not queue the call");
    return NULL;
  }
  a->box = box;
  a->n_groups = (uint32_t)n_gf - 1;
  a->n_sets = (uint32_t)n_len;
  a->stride = stride;
  a->flags = flags;
  a->seed = (uint64_t)seed;
  a->group_first = (uint32_t*)dup_bytes(gf, n_gf * 4);
  a->msgs = (uint8_t*)dup_bytes(msgs, n_msg);
  if (pkb) a->pk_bytes = (uint8_t*)dup_bytes(pkb, n_pkb);
  if (pki) a->pk_index = (uint32_t*)dup_bytes(pki, n_pki * 4);
  a->sig_len = (uint32_t*)dup_bytes(slen, n_len * 4);
  a->sigs = (uint8_t*)dup_bytes(sigs, (size_t)stride * n_len);
  a->set_result = (int8_t*)calloc((size_t)n_len + 1, 1);
  a->group_result = (int8_t*)calloc((size_t)a->n_groups + 1, 1);
  a->agg = agg;
  int agg_ok = 1;
  if (agg) {
    a->out_sig_len = out_sig_len;
    if (inc) a->include = (uint8_t*)dup_bytes(inc, n_inc);
    a->out_sig = (uint8_t*)calloc((size_t)a->n_groups * out_sig_len + 1, 1);
    a->agg_count = (uint32_t*)calloc((size_t)a->n_groups + 1, 4);
    agg_ok = (!inc || a->include) && a->out_sig && a->agg_count;
  }
  napi_value promise, name;
  if (!a->group_first || !a->msgs || (!a->pk_bytes && !a->pk_index) || !a->sig_len || !a->sigs || !a->set_result ||
      !a->group_result || !agg_ok || napi_create_promise(env, &a->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu_verify_same_message", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, same_execute, same_complete, a, &a->work) != napi_ok) {
    same_free(a);
    napi_throw_error(env, NULL, "verifySameMessage: could not queue the call");
    return NULL;
  }
  box->agg_pending++;
  if (napi_queue_async_work(env, a->work) != napi_ok) {
    box->agg_pending--;
    napi_delete_async_work(env, a->work);
    same_free(a);
    napi_throw_error(env, NULL, "verifySameMessage: could not queue the call");
    return NULL;
  }
  return promise;
}

static napi_value VerifySameMessage(napi_env env, napi_callback_info info) {
  return verify_same_message_call(env, info, 0);
}
static napi_value VerifySameMessageAggregate(napi_env env, napi_callback_info info) {
  return verify_same_message_call(env, info, 1);
}

/* aggregateVerify: one blsgpu_aggregate_verify call as async work (lifetimes as verifySameMessage: every input is
 * copied before the call returns, the outputs are the call's own until its completion on the main thread, and the
 * context stays open while the call is pending -- close() waits for agg_pending) */
typedef struct {
  CtxBox* box;
  uint32_t n_jobs, pk_len, stride, flags;
  uint32_t* job_first;
  uint8_t* msgs;
  uint8_t* pk_bytes;
  uint32_t* pk_index;
  uint32_t* sig_len;
  uint8_t* sigs;
  int8_t* job_result;
  uint32_t* first_bad;
  blsgpu_aggregate_verify_stats stats;
  int rc;
  napi_deferred deferred;
  napi_async_work work;
} AvCall;

static void av_free(AvCall* a) {
  free(a->job_first);
  free(a->msgs);
  free(a->pk_bytes);
  free(a->pk_index);
  free(a->sig_len);
  free(a->sigs);
  free(a->job_result);
  free(a->first_bad);
  free(a);
}

/* libuv worker thread */
static void av_execute(napi_env env, void* data) {
  (void)env;
  AvCall* a = (AvCall*)data;
  a->rc = blsgpu_aggregate_verify(a->box->ctx, a->n_jobs, a->job_first, a->msgs, a->pk_bytes, a->pk_len, a->pk_index,
                                  a->sigs, a->stride, a->sig_len, a->flags, a->job_result, a->first_bad, &a->stats);
}

/* JS main thread */
static void av_complete(napi_env env, napi_status st, void* data) {
  AvCall* a = (AvCall*)data;
  a->box->agg_pending--;
  if (st != napi_ok || a->rc != BLSGPU_OK) {
    const char* name = blsgpu_code_name(st != napi_ok ? BLSGPU_ERR_CLOSED : a->rc);
    napi_value msg, code, err;
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &msg);
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &code);
    napi_create_error(env, code, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
  } else {
    napi_value out, stats, ms;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "jobResult", copy_out(env, napi_int8_array, a->job_result, a->n_jobs, 1));
    napi_set_named_property(env, out, "firstBad", copy_out(env, napi_uint32_array, a->first_bad, a->n_jobs, 4));
    napi_create_object(env, &stats);
    set_u32(env, stats, "pairs", a->stats.pairs);
    set_u32(env, stats, "uniqueMessages", a->stats.unique_messages);
    set_u32(env, stats, "millerItems", a->stats.miller_items);
    set_u32(env, stats, "millerChunks", a->stats.miller_chunks);
    set_u32(env, stats, "form", a->stats.form);
    set_u32(env, stats, "jobsChecked", a->stats.jobs_checked);
    napi_create_double(env, a->stats.device_ms, &ms);
    napi_set_named_property(env, stats, "deviceMs", ms);
    napi_set_named_property(env, out, "stats", stats);
    napi_resolve_deferred(env, a->deferred, out);
  }
  napi_delete_async_work(env, a->work);
  av_free(a);
}

static napi_value AggregateVerify(napi_env env, napi_callback_info info) {
  size_t argc = 10;
  napi_value argv[10];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 10) {
    napi_throw_type_error(env, NULL,
                          "aggregateVerify(ctx, jobFirst, msgs, pkBytes, pkLen, pkIndex, sigs, sigLen, sigStride, flags)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  size_t n_jf = 0, n_msg = 0, n_pkb = 0, n_pki = 0, n_bytes = 0, n_len = 0;
  void *jf = NULL, *msgs = NULL, *pkb = NULL, *pki = NULL, *sigs = NULL, *slen = NULL;
  if (opt_typed(env, argv[1], napi_uint32_array, &jf, &n_jf) || !jf ||
      opt_typed(env, argv[2], napi_uint8_array, &msgs, &n_msg) || !msgs ||
      opt_typed(env, argv[3], napi_uint8_array, &pkb, &n_pkb) ||
      opt_typed(env, argv[5], napi_uint32_array, &pki, &n_pki) ||
      opt_typed(env, argv[6], napi_uint8_array, &sigs, &n_bytes) || !sigs ||
      opt_typed(env, argv[7], napi_uint32_array, &slen, &n_len) || !slen) {
    napi_throw_type_error(env, NULL,
                          "aggregateVerify: jobFirst, pkIndex, sigLen Uint32Array; msgs, pkBytes, sigs Uint8Array");
    return NULL;
  }
  uint32_t pk_len = 0, stride = 0, flags = 0;
  napi_get_value_uint32(env, argv[4], &pk_len);
  napi_get_value_uint32(env, argv[8], &stride);
  napi_get_value_uint32(env, argv[9], &flags);
  /* shape checks on the host before anything is queued */
  const uint32_t* jfw = (const uint32_t*)jf;
  const int validate = (flags & BLSGPU_AV_VALIDATE_KEYS) != 0;
  int ok = n_jf >= 1 && stride >= 96 && !(flags & ~(BLSGPU_AV_VALIDATE_KEYS | BLSGPU_AV_LANE_FORMS)) && jfw[0] == 0 &&
           (pkb != NULL) != (pki != NULL) && n_len == n_jf - 1 && n_len <= (1u << 20) &&
           n_bytes >= (size_t)stride * n_len;
  for (size_t j = 0; ok && j + 1 < n_jf; j++) ok = jfw[j + 1] >= jfw[j];
  const size_t n_pairs = ok ? jfw[n_jf - 1] : 0;
  ok = ok && n_pairs <= (1u << 20) && n_msg == 32 * n_pairs;
  if (ok && pkb)
    ok = (validate ? (pk_len == 48 || pk_len == 96) : pk_len == 96) && n_pkb == (size_t)pk_len * n_pairs;
  else if (ok)
    ok = !validate && n_pki == n_pairs;
  for (size_t k = 0; ok && stride < 192 && k < n_len; k++) ok = ((const uint32_t*)slen)[k] != 192;
  if (!ok) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "aggregateVerify: inconsistent array sizes");
    return NULL;
  }
  AvCall* a = (AvCall*)calloc(1, sizeof(AvCall));
  if (!a) {
    napi_throw_error(env, NULL, "aggregateVerify: could not queue the call");
    return NULL;
  }
  a->box = box;
  a->n_jobs = (uint32_t)n_jf - 1;
  a->pk_len = pk_len;
  a->stride = stride;
  a->flags = flags;
  a->job_first = (uint32_t*)dup_bytes(jf, n_jf * 4);
  a->msgs = (uint8_t*)dup_bytes(msgs, n_msg);
  if (pkb) a->pk_bytes = (uint8_t*)dup_bytes(pkb, n_pkb);
  if (pki) a->pk_index = (uint32_t*)dup_bytes(pki, n_pki * 4);
  a->sig_len = (uint32_t*)dup_bytes(slen, n_len * 4);
  a->sigs = (uint8_t*)dup_bytes(sigs, (size_t)stride * n_len);
  a->job_result = (int8_t*)calloc((size_t)a->n_jobs + 1, 1);
  a->first_bad = (uint32_t*)calloc((size_t)a->n_jobs + 1, 4);
  napi_value promise, name;
  if (!a->job_first || !a->msgs || (!a->pk_bytes && !a->pk_index) || !a->sig_len || !a->sigs || !a->job_result ||
      !a->first_bad || napi_create_promise(env, &a->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu_aggregate_verify", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, av_execute, av_complete, a, &a->work) != napi_ok) {
    av_free(a);
    napi_throw_error(env, NULL, "aggregateVerify: could not queue the call");
    return NULL;
  }
  box->agg_pending++;
  if (napi_queue_async_work(env, a->work) != napi_ok) {
    box->agg_pending--;
    napi_delete_async_work(env, a->work);
    av_free(a);
    napi_throw_error(env, NULL, "aggregateVerify: could not queue the call");
    return NULL;
  }
  return promise;
}

/* uploadCommittees(ctx, firstCommittee, committeeFirst Uint32Array [n + 1], members Uint32Array)  (synchronous, like
 * uploadPubkeys): blsgpu_committees_upload */
static napi_value UploadCommittees(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4) {
    napi_throw_type_error(env, NULL, "uploadCommittees(ctx, firstCommittee, committeeFirst, members)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  uint32_t first = 0;
  CHECK(env, napi_get_value_uint32(env, argv[1], &first));
  napi_typedarray_type t_cf, t_mem;
  size_t n_cf = 0, n_mem = 0;
  void *cf = NULL, *mem = NULL;
  if (napi_get_typedarray_info(env, argv[2], &t_cf, &n_cf, &cf, NULL, NULL) != napi_ok || t_cf != napi_uint32_array ||
      napi_get_typedarray_info(env, argv[3], &t_mem, &n_mem, &mem, NULL, NULL) != napi_ok ||
      t_mem != napi_uint32_array) {
    napi_throw_type_error(env, NULL, "uploadCommittees: committeeFirst and members Uint32Array expected");
    return NULL;
  }
  /* the arrays must be as long as the offsets say before the library reads them */
  if (n_cf < 1 || n_cf - 1 > 0xffffffffu || ((const uint32_t*)cf)[n_cf - 1] != n_mem)
    return throw_code(env, "uploadCommittees", BLSGPU_ERR_ARGS);
  const uint32_t n = (uint32_t)(n_cf - 1);
  int rc = blsgpu_committees_upload(box->ctx, first, n, n ? (const uint32_t*)cf : NULL, n ? (const uint32_t*)mem : NULL);
  if (rc != BLSGPU_OK) return throw_code(env, "uploadCommittees", rc);
  return NULL;
}

static napi_value CommitteesCount(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  napi_value out;
  CHECK(env, napi_create_uint32(env, blsgpu_committees_count(box->ctx), &out));
  return out;
}

/* aggregatePubkeysFromBits: one blsgpu_aggregate_pubkeys_bits call as async work, with the lifetime rules of
 * aggregateSignatures (inputs copied before it returns; close() refuses while a call is outstanding) */
typedef struct {
  CtxBox* box;
  uint32_t n_sets, flags, out_len;
  uint32_t* set_seg_first;
  uint32_t* seg_committee;
  uint32_t* set_bits_first;
  uint8_t* bits;
  uint8_t* out;
  int8_t* status;
  blsgpu_committee_bits_stats stats;
  int rc;
  napi_deferred deferred;
  napi_async_work work;
} BitsCall;

static void bits_free(BitsCall* a) {
  free(a->set_seg_first);
  free(a->seg_committee);
  free(a->set_bits_first);
  free(a->bits);
  free(a->out);
  free(a->status);
  free(a);
}

/* libuv worker thread */
static void bits_execute(napi_env env, void* data) {
  (void)env;
  BitsCall* a = (BitsCall*)data;
  a->rc = blsgpu_aggregate_pubkeys_bits(a->box->ctx, a->n_sets, a->set_seg_first, a->seg_committee, a->set_bits_first,
                                        a->bits, a->flags, a->out, a->out_len, a->status, &a->stats);
}

/* JS main thread */
static void bits_complete(napi_env env, napi_status st, void* data) {
  BitsCall* a = (BitsCall*)data;
  a->box->agg_pending--;
  if (st != napi_ok || a->rc != BLSGPU_OK) {
    const char* name = blsgpu_code_name(st != napi_ok ? BLSGPU_ERR_CLOSED : a->rc);
    napi_value msg, code, err;
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &msg);
    napi_create_string_utf8(env, name ? name : "BLSGPU_DEVICE_ERROR", NAPI_AUTO_LENGTH, &code);
    napi_create_error(env, code, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
  } else {
    napi_value out, stats;
    napi_create_object(env, &out);
    napi_create_object(env, &stats);
    set_u32(env, stats, "segments", a->stats.segments);
    set_u32(env, stats, "segmentsComplemented", a->stats.segments_complemented);
    set_u32(env, stats, "keysPresent", a->stats.keys_present);
    set_u32(env, stats, "keysAdded", a->stats.keys_added);
    set_u32(env, stats, "keysSubtracted", a->stats.keys_subtracted);
    set_u32(env, stats, "lanes", a->stats.lanes);
    set_num(env, stats, "deviceMs", a->stats.device_ms);
    napi_set_named_property(env, out, "out", copy_out(env, napi_uint8_array, a->out, (size_t)a->n_sets * a->out_len, 1));
    napi_set_named_property(env, out, "status", copy_out(env, napi_int8_array, a->status, a->n_sets, 1));
    napi_set_named_property(env, out, "stats", stats);
    napi_resolve_deferred(env, a->deferred, out);
  }
  napi_delete_async_work(env, a->work);
  bits_free(a);
}

static napi_value AggregatePubkeysFromBits(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 7) {
    napi_throw_type_error(
        env, NULL, "aggregatePubkeysFromBits(ctx, setSegFirst, segCommittee, setBitsFirst, bits, noComplement, outLen)");
    return NULL;
  }
  CtxBox* box = get_open_box(env, argv[0]);
  if (!box) return NULL;
  napi_typedarray_type t[4];
  size_t len[4] = {0, 0, 0, 0};
  void* p[4] = {NULL, NULL, NULL, NULL};
  const napi_typedarray_type want[4] = {napi_uint32_array, napi_uint32_array, napi_uint32_array, napi_uint8_array};
  for (int k = 0; k < 4; k++)
    if (napi_get_typedarray_info(env, argv[1 + k], &t[k], &len[k], &p[k], NULL, NULL) != napi_ok || t[k] != want[k]) {
      napi_throw_type_error(env, NULL,
                            "aggregatePubkeysFromBits: setSegFirst, segCommittee, setBitsFirst Uint32Array and bits "
                            "Uint8Array expected");
      return NULL;
    }
  bool no_complement = false;
  uint32_t out_len = 0;
  napi_coerce_to_bool(env, argv[5], &argv[5]);
  napi_get_value_bool(env, argv[5], &no_complement);
  napi_get_value_uint32(env, argv[6], &out_len);
  /* shape checks on the host before anything is queued: the arrays are as long as the offsets say (the library checks
   * the offsets themselves, the committee ids and the bit strings) */
  const uint32_t *ssf = (const uint32_t*)p[0], *sbf = (const uint32_t*)p[2];
  int ok = len[0] >= 1 && len[2] == len[0] && len[0] - 1 <= (1u << 20) && (out_len == 48 || out_len == 96);
  ok = ok && ssf[len[0] - 1] <= len[1] && sbf[len[2] - 1] <= len[3];
  if (!ok) {
    napi_throw_range_error(env, "BLSGPU_ERR_ARGS", "aggregatePubkeysFromBits: inconsistent array sizes");
    return NULL;
  }
  BitsCall* a = (BitsCall*)calloc(1, sizeof(BitsCall));
  a->box = box;
  a->n_sets = (uint32_t)len[0] - 1;
  a->flags = no_complement ? BLSGPU_BITS_NO_COMPLEMENT : 0;
  a->out_len = out_len;
  a->set_seg_first = (uint32_t*)dup_bytes(p[0], len[0] * 4);
  a->seg_committee = (uint32_t*)dup_bytes(p[1], len[1] * 4);
  a->set_bits_first = (uint32_t*)dup_bytes(p[2], len[2] * 4);
  a->bits = (uint8_t*)dup_bytes(p[3], len[3]);
  a->out = (uint8_t*)calloc((size_t)a->n_sets * out_len + 1, 1);
  a->status = (int8_t*)calloc((size_t)a->n_sets + 1, 1);
  napi_value promise, name;
  if (!a->set_seg_first || !a->seg_committee || !a->set_bits_first || !a->bits || !a->out || !a->status ||
      napi_create_promise(env, &a->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu_aggregate_pubkeys_bits", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, bits_execute, bits_complete, a, &a->work) != napi_ok) {
    bits_free(a);
    napi_throw_error(env, NULL, "aggregatePubkeysFromBits: could not queue the call");
    return NULL;
  }
  box->agg_pending++;
  if (napi_queue_async_work(env, a->work) != napi_ok) {
    box->agg_pending--;
    napi_delete_async_work(env, a->work);
    bits_free(a);
    napi_throw_error(env, NULL, "aggregatePubkeysFromBits: could not queue the call");
    return NULL;
  }
  return promise;
}

/* debugInject(what, skip, count): blsgpu_debug_inject (test hook; BLSGPU_INJECT_ENTROPY 1, BLSGPU_INJECT_DEVICE 2) */
static napi_value DebugInject(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "debugInject(what, skip, count)");
    return NULL;
  }
  int32_t what = 0;
  int64_t skip = 0, count = 0;
  napi_get_value_int32(env, argv[0], &what);
  napi_get_value_int64(env, argv[1], &skip);
  napi_get_value_int64(env, argv[2], &count);
  int rc = blsgpu_debug_inject(what, skip, count);
  if (rc != BLSGPU_OK) return throw_code(env, "blsgpu_debug_inject", rc);
  return NULL;
}

static napi_value ModuleInit(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"init", NULL, Init, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"close", NULL, Close, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"deviceCount", NULL, DeviceCount, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"uploadPubkeys", NULL, UploadPubkeys, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"uploadPubkeysCompressed", NULL, UploadPubkeysCompressed, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"readPubkeys", NULL, ReadPubkeys, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"pubkeysCount", NULL, PubkeysCount, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"setOption", NULL, SetOption, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"getOption", NULL, GetOption, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"codeName", NULL, CodeName, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"submit", NULL, Submit, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"keyValidate", NULL, KeyValidate, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"aggregateSignatures", NULL, AggregateSignatures, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"aggregateWithRandomness", NULL, AggregateWithRandomness, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"verifySameMessage", NULL, VerifySameMessage, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"verifySameMessageAggregate", NULL, VerifySameMessageAggregate, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"aggregateVerify", NULL, AggregateVerify, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"uploadCommittees", NULL, UploadCommittees, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"committeesCount", NULL, CommitteesCount, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
      {"aggregatePubkeysFromBits", NULL, AggregatePubkeysFromBits, NULL, NULL, NULL, (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable), NULL},
  };
  napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
  /* the fault-injection test hook is exported, by its own definition, only to processes started with
   * BLSGPU_FAULT_INJECTION=1 (the library refuses to arm it otherwise) */
  const char* fi = getenv("BLSGPU_FAULT_INJECTION");
  if (fi && fi[0] == '1' && fi[1] == 0) {
    napi_property_descriptor inject = {"debugInject", NULL, DebugInject, NULL, NULL, NULL,
                                       (napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable),
                                       NULL};
    napi_define_properties(env, exports, 1, &inject);
  }
  napi_value v;
  napi_create_int32(env, BLSGPU_ABI_VERSION, &v);
  napi_set_named_property(env, exports, "abiVersion", v);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, ModuleInit)
