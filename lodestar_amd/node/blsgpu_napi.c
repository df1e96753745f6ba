/*
 * blsgpu.node — N-API binding of libblsgpu.so for Node (the reference's own runtime).
 *
 * Exposes the C-ABI (include/blsgpu.h) to JavaScript; BlsGpuVerifier.js builds the
 * IBlsVerifier (packages/beacon-node/src/chain/bls/interface.ts:20-46) on top.
 * Verification goes through bgv_verify_async: the library's dispatcher threads run it and
 * hand the completion to the main thread through a napi_threadsafe_function, which
 * resolves the Promise, like the reference's worker round trip
 * (multithread/index.ts:290-381).  No libuv pool thread is held while a batch runs.
 *
 * Lifetime: the ctx value is an external over a small wrapper.  close(ctx) is idempotent:
 * it closes the library context (queued and in-flight verifies complete first, later
 * calls reject with QUEUE_ABORTED) but does not free it; the memory is released by the
 * external's finalizer, which cannot run while a verify holds a reference to the ctx.
 *
 *   init(devices?: number[]) -> ctx
 *   pubkeysPut(ctx, firstIndex, keys: Uint8Array, fmt: 48 | 96)
 *   pubkeysPutAsync(ctx, firstIndex, keys, fmt) -> Promise<void>  (on a libuv pool thread)
 *   keygen(ctx, sks: Uint8Array, cacheFirst: number) -> Uint8Array (48-B pubkeys)
 *   sign(ctx, sks: Uint8Array, msgs: Uint8Array) -> Uint8Array (96-B signatures)
 *   verify(ctx, jobs: {sets: {pkIndices: Uint32Array | pkBytes: Uint8Array (n x 96),
 *                             msg: Uint8Array, sig: Uint8Array}[], batchable: boolean}[],
 *          mode: 0 | 1) -> Promise<Int32Array>   (1 valid, 0 invalid, -code error)
 *   verifyAccumulate(ctx, jobs (sets may carry pool: number), mode)
 *          -> Promise<{codes, stats, added: Uint8Array}>   (bgv_verify_accumulate_async)
 *   sigpoolOpen(ctx, id), sigpoolDropRange(ctx, firstId, count) -> number
 *   sigpoolGet(ctx, ids: Uint32Array) -> Promise<{status, count, sigs}>  (on a libuv pool thread)
 *   sigpoolOpenBits(ctx, id, nBits); verifyAccumulateBits(ctx, jobs, mode) -> Promise<{codes, stats,
 *          outcome: Uint8Array}>   (bgv_verify_accumulate_bits_async)
 *   sigpoolGetBits(ctx, ids) / sigpoolSum(ctx, ids, lengths) -> Promise<{status, count, sigs, bits,
 *          nBits, stride}>  (on a libuv pool thread)
 *   strerror(code) -> string
 *   close(ctx)
 * SURVEY 8(f) entry points and parity hooks (synchronous):
 *   aggregatePubkeys(ctx, indices: Uint32Array) -> Uint8Array (96-B uncompressed)
 *   hashToG2(ctx, msg: Uint8Array) -> Uint8Array (192-B uncompressed)
 *   pubkeysValidate(ctx, keys48) -> {status: Int32Array, uncompressed: Uint8Array}
 *   aggregateSignatures(ctx, aggregates: Uint8Array[][]) -> {status: Int32Array, sigs: Uint8Array}
 *   depositsVerify(ctx, keys48, msgs32, sigs96) -> Int32Array (1 | 0)
 */
#include <node_api.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/blsgpu.h"

#define CHECK(env, x)                                         \
  do {                                                        \
    if ((x) != napi_ok) {                                     \
      napi_throw_error((env), NULL, "blsgpu: N-API failure"); \
      return NULL;                                            \
    }                                                         \
  } while (0)

static napi_value throw_code(napi_env env, int rc) {
  napi_throw_error(env, NULL, bgv_strerror(rc));
  return NULL;
}

typedef struct {
  bgv_ctx* c;
  int closed;                    /* close() was called: every entry point rejects */
  uint32_t inflight;             /* async verifies not yet completed */
  napi_threadsafe_function tsfn; /* completions from the dispatcher threads */
  int tsfn_released;             /* released by close() or finalized by the runtime */
  int owners;                    /* the ctx external and the tsfn: freed when both are gone */
} addon_ctx;

static void addon_unref(addon_ctx* a) {
  if (--a->owners == 0) {
    bgv_destroy(a->c);
    free(a);
  }
}

static addon_ctx* get_actx(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok) return NULL;
  return (addon_ctx*)p;
}

/* the library context of an open addon context, else NULL (the caller throws) */
static bgv_ctx* get_ctx(napi_env env, napi_value v) {
  addon_ctx* a = get_actx(env, v);
  return a && !a->closed ? a->c : NULL;
}

#define OPEN_CTX(env, v, ctx)                                 \
  bgv_ctx* ctx = get_ctx((env), (v));                         \
  do {                                                        \
    if (!ctx) return throw_code((env), -BGV_E_CLOSED);        \
  } while (0)

static int get_bytes(napi_env env, napi_value v, uint8_t** data, size_t* len) {
  napi_typedarray_type t;
  size_t n, off;
  void* d;
  napi_value ab;
  if (napi_get_typedarray_info(env, v, &t, &n, &d, &ab, &off) != napi_ok) return -1;
  if (t == napi_uint8_array) {
    *data = (uint8_t*)d;
    *len = n;
    return 0;
  }
  if (t == napi_uint32_array) {
    *data = (uint8_t*)d;
    *len = n * 4;
    return 0;
  }
  return -1;
}

typedef struct {
  addon_ctx* actx;
  napi_ref ctx_ref; /* keeps the ctx external (and its finalizer) alive */
  bgv_job* jobs;
  size_t njobs;
  bgv_set* sets;
  bgv_pkbits* pkbits; /* beside sets; handed to the library only when a set names a committee */
  int any_committee;
  bgv_pkspan* spans; /* beside sets; handed to the library instead when a set names several committees */
  int any_span;
  size_t nsets;
  int mode;
  int32_t* codes;
  bgv_stats stats;
  int rc;
  napi_deferred deferred;
  napi_ref* refs; /* keep every input buffer alive until completion */
  size_t nrefs;
  /* verifyAggregate (1): the sets' `agg` tags beside sets, and the aggregates' outputs;
   * verifyAccumulate (2): the sets' `pool` tags in tags, and per set whether it was added;
   * verifyAccumulateBits (3): as 2 with the sets' positions in poolbits, and per set its outcome */
  int aggregate;
  uint8_t* added;
  bgv_poolbits* poolbits;
  uint32_t* tags;
  size_t naggs;
  uint8_t* agg96;
  int32_t* agg_status;
  uint32_t* agg_count;
} verify_req;

static void verify_call_js(napi_env env, napi_value js_cb, void* context, void* data);
static void addon_finalize(napi_env env, void* data, void* hint);
static void tsfn_finalized(napi_env env, void* data, void* hint);

static napi_value js_init(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int devs[64];
  int ndev = 0;
  if (argc >= 1) {
    bool is_arr = false;
    napi_is_array(env, argv[0], &is_arr);
    if (is_arr) {
      uint32_t n = 0;
      napi_get_array_length(env, argv[0], &n);
      for (uint32_t i = 0; i < n && i < 64; ++i) {
        napi_value e;
        napi_get_element(env, argv[0], i, &e);
        napi_get_value_int32(env, e, &devs[ndev++]);
      }
    }
  }
  bgv_ctx* ctx = NULL;
  int rc = bgv_init(ndev ? devs : NULL, ndev, &ctx);
  if (rc) return throw_code(env, rc);
  addon_ctx* a = (addon_ctx*)calloc(1, sizeof(addon_ctx));
  a->c = ctx;
  a->owners = 2;
  napi_value out, name;
  if (napi_create_string_utf8(env, "blsgpu.verify.done", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_threadsafe_function(env, NULL, NULL, name, 0, 1, a, tsfn_finalized, NULL, verify_call_js,
                                      &a->tsfn) != napi_ok ||
      napi_unref_threadsafe_function(env, a->tsfn) != napi_ok ||
      napi_create_external(env, a, addon_finalize, NULL, &out) != napi_ok) {
    bgv_destroy(ctx);
    free(a);
    napi_throw_error(env, NULL, "blsgpu: N-API failure");
    return NULL;
  }
  return out;
}

/* close(ctx): idempotent; the library drains queued and in-flight verifies (their
 * completions still resolve), and every later call rejects with QUEUE_ABORTED. */
static napi_value js_close(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  addon_ctx* a = get_actx(env, argv[0]);
  if (a && !a->closed) {
    a->closed = 1;
    bgv_close(a->c);  /* every queued completion has been handed to the tsfn */
    if (!a->tsfn_released) {
      a->tsfn_released = 1;
      napi_release_threadsafe_function(a->tsfn, napi_tsfn_release);  /* delivers them, then finalizes */
    }
  }
  return NULL;
}

static napi_value js_strerror(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  int32_t code = 0;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  napi_get_value_int32(env, argv[0], &code);
  CHECK(env, napi_create_string_utf8(env, bgv_strerror(code), NAPI_AUTO_LENGTH, &out));
  return out;
}

static napi_value js_pubkeys_put(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t first = 0;
  int32_t fmt = 48;
  uint8_t* keys;
  size_t len;
  napi_get_value_uint32(env, argv[1], &first);
  if (get_bytes(env, argv[2], &keys, &len)) return throw_code(env, -BGV_E_ARG);
  napi_get_value_int32(env, argv[3], &fmt);
  int rc = bgv_pubkeys_put(ctx, first, keys, len / (size_t)fmt, fmt);
  if (rc) return throw_code(env, rc);
  return NULL;
}

/* pubkeysPutAsync(ctx, firstIndex, keys, fmt) -> Promise<void>: bgv_pubkeys_put on a libuv pool
 * thread, so a validator-set growth (EpochContext.addPubkey, epochContext.ts:702-705) never
 * blocks the event loop; the library decodes into staging memory without holding up running
 * verifies.  Rejects with an Error whose .bgvCode is the negative library code (-BGV_E_ARG for
 * a gap in the indices: nothing was written; a BLST code: the run was committed with the
 * undecodable indices marked). */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref ctx_ref, keys_ref;
  bgv_ctx* c;
  uint32_t first;
  const uint8_t* keys;
  size_t n;
  int fmt, rc;
} put_req;

static void put_execute(napi_env env, void* data) {
  (void)env;
  put_req* r = (put_req*)data;
  r->rc = bgv_pubkeys_put(r->c, r->first, r->keys, r->n, r->fmt);
}

static void put_complete(napi_env env, napi_status status, void* data) {
  put_req* r = (put_req*)data;
  if (status == napi_ok && r->rc == 0) {
    napi_value undef;
    napi_get_undefined(env, &undef);
    napi_resolve_deferred(env, r->deferred, undef);
  } else {
    const int rc = status == napi_ok ? r->rc : -BGV_E_ARG;
    napi_value msg, err, code;
    napi_create_string_utf8(env, bgv_strerror(rc), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int32(env, rc, &code);
    napi_set_named_property(env, err, "bgvCode", code);
    napi_reject_deferred(env, r->deferred, err);
  }
  napi_delete_reference(env, r->ctx_ref);
  napi_delete_reference(env, r->keys_ref);
  napi_delete_async_work(env, r->work);
  free(r);
}

static napi_value js_pubkeys_put_async(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4], promise, name;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t* keys;
  size_t len;
  uint32_t first = 0;
  int32_t fmt = 48;
  napi_get_value_uint32(env, argv[1], &first);
  if (get_bytes(env, argv[2], &keys, &len)) return throw_code(env, -BGV_E_ARG);
  napi_get_value_int32(env, argv[3], &fmt);
  if (fmt != 48 && fmt != 96) return throw_code(env, -BGV_E_ARG);
  put_req* r = (put_req*)calloc(1, sizeof(put_req));
  r->c = ctx;
  r->first = first;
  r->keys = keys;
  r->n = len / (size_t)fmt;
  r->fmt = fmt;
  if (napi_create_promise(env, &r->deferred, &promise) != napi_ok ||
      napi_create_reference(env, argv[0], 1, &r->ctx_ref) != napi_ok ||
      napi_create_reference(env, argv[2], 1, &r->keys_ref) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu.pubkeysPut", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, put_execute, put_complete, r, &r->work) != napi_ok ||
      napi_queue_async_work(env, r->work) != napi_ok) {
    napi_throw_error(env, NULL, "blsgpu: N-API failure");
    return NULL;
  }
  return promise;
}

static napi_value js_keygen(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], ab, out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t* sks;
  size_t len;
  int64_t first = -1;
  if (get_bytes(env, argv[1], &sks, &len)) return throw_code(env, -BGV_E_ARG);
  napi_get_value_int64(env, argv[2], &first);
  void* dst;
  CHECK(env, napi_create_arraybuffer(env, 48 * (len / 32), &dst, &ab));
  int rc = bgv_keygen(ctx, sks, len / 32, first, (uint8_t*)dst);
  if (rc) return throw_code(env, rc);
  CHECK(env, napi_create_typedarray(env, napi_uint8_array, 48 * (len / 32), ab, 0, &out));
  return out;
}

static napi_value js_sign(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], ab, out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t *sks, *msgs;
  size_t l1, l2;
  if (get_bytes(env, argv[1], &sks, &l1) || get_bytes(env, argv[2], &msgs, &l2) || l1 != l2)
    return throw_code(env, -BGV_E_ARG);
  void* dst;
  CHECK(env, napi_create_arraybuffer(env, 96 * (l1 / 32), &dst, &ab));
  int rc = bgv_sign(ctx, sks, msgs, l1 / 32, (uint8_t*)dst);
  if (rc) return throw_code(env, rc);
  CHECK(env, napi_create_typedarray(env, napi_uint8_array, 96 * (l1 / 32), ab, 0, &out));
  return out;
}

/* ---- SURVEY 8(f) entry points and parity hooks (synchronous: low volume) ---- */

static napi_value new_bytes(napi_env env, size_t n, void** dst) {
  napi_value ab, out;
  if (napi_create_arraybuffer(env, n, dst, &ab) != napi_ok) return NULL;
  if (napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &out) != napi_ok) return NULL;
  return out;
}

static napi_value new_int32s(napi_env env, const int32_t* src, size_t n) {
  napi_value ab, out;
  void* dst;
  if (napi_create_arraybuffer(env, 4 * n, &dst, &ab) != napi_ok) return NULL;
  if (n) memcpy(dst, src, 4 * n);
  if (napi_create_typedarray(env, napi_int32_array, n, ab, 0, &out) != napi_ok) return NULL;
  return out;
}

/* aggregatePubkeys(ctx, indices: Uint32Array) -> Uint8Array(96): PublicKey.aggregate +
 * toBytes(uncompressed) over cached keys (chain/bls/utils.ts:5-16). */
static napi_value js_aggregate_pubkeys(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t* idx;
  size_t len;
  if (get_bytes(env, argv[1], &idx, &len) || len % 4) return throw_code(env, -BGV_E_ARG);
  void* dst;
  napi_value out = new_bytes(env, 96, &dst);
  if (!out) return throw_code(env, -BGV_E_ARG);
  int rc = bgv_aggregate_pubkeys(ctx, (const uint32_t*)idx, len / 4, (uint8_t*)dst);
  if (rc) return throw_code(env, rc);
  return out;
}

/* committeePut(ctx, id, indices: Uint32Array): the committee's validator indices and their pubkey
 * sum onto the device(s) under id (bgv_committee_put); sets then name {committee, bits, nBits}.
 * committeeDrop(ctx, id) frees the id. */
static napi_value js_committee_put(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t id = 0;
  uint8_t* idx;
  size_t len;
  if (argc < 3 || napi_get_value_uint32(env, argv[1], &id) != napi_ok || get_bytes(env, argv[2], &idx, &len) ||
      len % 4)
    return throw_code(env, -BGV_E_ARG);
  int rc = bgv_committee_put(ctx, id, (const uint32_t*)idx, len / 4);
  if (rc) return throw_code(env, rc);
  return NULL;
}

static napi_value js_committee_drop(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t id = 0;
  if (argc < 2 || napi_get_value_uint32(env, argv[1], &id) != napi_ok) return throw_code(env, -BGV_E_ARG);
  int rc = bgv_committee_drop(ctx, id);
  if (rc) return throw_code(env, rc);
  return NULL;
}

/* committeeDropRange(ctx, firstId, count) -> number: bgv_committee_drop_range, the live ids of the
 * range dropped (host-only work). */
static napi_value js_committee_drop_range(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t first = 0, count = 0;
  if (argc < 3 || napi_get_value_uint32(env, argv[1], &first) != napi_ok ||
      napi_get_value_uint32(env, argv[2], &count) != napi_ok)
    return throw_code(env, -BGV_E_ARG);
  int rc = bgv_committee_drop_range(ctx, first, count);
  if (rc < 0) return throw_code(env, rc);
  CHECK(env, napi_create_int32(env, rc, &out));
  return out;
}

/* sigpoolOpen(ctx, id): a device-resident signature pool entry, empty (bgv_sigpool_open; host work
 * after the first call, which allocates the accumulators).
 * sigpoolDropRange(ctx, firstId, count) -> number: bgv_sigpool_drop_range, the live ids dropped. */
static napi_value js_sigpool_open(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t id = 0;
  if (argc < 2 || napi_get_value_uint32(env, argv[1], &id) != napi_ok) return throw_code(env, -BGV_E_ARG);
  int rc = bgv_sigpool_open(ctx, id);
  if (rc) return throw_code(env, rc);
  return NULL;
}

/* sigpoolOpenBits(ctx, id, nBits): bgv_sigpool_open_bits */
static napi_value js_sigpool_open_bits(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t id = 0, nbits = 0;
  if (argc < 3 || napi_get_value_uint32(env, argv[1], &id) != napi_ok ||
      napi_get_value_uint32(env, argv[2], &nbits) != napi_ok)
    return throw_code(env, -BGV_E_ARG);
  int rc = bgv_sigpool_open_bits(ctx, id, nbits);
  if (rc) return throw_code(env, rc);
  return NULL;
}

static napi_value js_sigpool_drop_range(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t first = 0, count = 0;
  if (argc < 3 || napi_get_value_uint32(env, argv[1], &first) != napi_ok ||
      napi_get_value_uint32(env, argv[2], &count) != napi_ok)
    return throw_code(env, -BGV_E_ARG);
  int rc = bgv_sigpool_drop_range(ctx, first, count);
  if (rc < 0) return throw_code(env, rc);
  CHECK(env, napi_create_int32(env, rc, &out));
  return out;
}

/* sigpoolGet(ctx, ids: Uint32Array) -> Promise<{status: Int32Array, count: Uint32Array, sigs:
 * Uint8Array (n x 96 compressed)}>: bgv_sigpool_get on a libuv pool thread (it waits for the
 * device); rejects with an Error whose .bgvCode is the negative library code.  sigpoolGetBits and
 * sigpoolSum share the request and its two callbacks. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref ctx_ref;
  bgv_ctx* c;
  uint32_t* ids;
  size_t n;
  uint8_t* out96;
  uint32_t* count;
  int32_t* status;
  int rc;
  /* sigpoolGetBits (kind 1): the fields and n_bits; sigpoolSum (kind 2): n is the number of groups,
   * ids the groups' ids one after the other, groups their lists, stride the bytes per group in bits */
  int kind;
  uint8_t* bits;
  uint32_t* nbits;
  bgv_poolgroup* groups;
  size_t stride;
} pool_get_req;

static void pool_get_execute(napi_env env, void* data) {
  (void)env;
  pool_get_req* r = (pool_get_req*)data;
  if (r->kind == 2)
    r->rc = bgv_sigpool_sum(r->c, r->groups, r->n, r->out96, r->count, r->status, r->bits, r->stride, r->nbits);
  else if (r->kind == 1)
    r->rc = bgv_sigpool_get_bits(r->c, r->ids, r->n, r->out96, r->count, r->status, r->bits, r->nbits);
  else
    r->rc = bgv_sigpool_get(r->c, r->ids, r->n, r->out96, r->count, r->status);
}

static void pool_get_complete(napi_env env, napi_status status, void* data) {
  pool_get_req* r = (pool_get_req*)data;
  if (status == napi_ok && r->rc == 0) {
    napi_value out, st = new_int32s(env, r->status, r->n), cab, carr, sigs;
    void* dst;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "status", st);
    napi_create_arraybuffer(env, 4 * r->n, &dst, &cab);
    if (r->n) memcpy(dst, r->count, 4 * r->n);
    napi_create_typedarray(env, napi_uint32_array, r->n, cab, 0, &carr);
    napi_set_named_property(env, out, "count", carr);
    sigs = new_bytes(env, 96 * r->n, &dst);
    if (r->n) memcpy(dst, r->out96, 96 * r->n);
    napi_set_named_property(env, out, "sigs", sigs);
    if (r->kind) { /* bits: n x stride bytes, nBits: Uint32Array, stride */
      napi_value bits, nab, narr, sv;
      bits = new_bytes(env, r->stride * r->n, &dst);
      if (r->n) memcpy(dst, r->bits, r->stride * r->n);
      napi_set_named_property(env, out, "bits", bits);
      napi_create_arraybuffer(env, 4 * r->n, &dst, &nab);
      if (r->n) memcpy(dst, r->nbits, 4 * r->n);
      napi_create_typedarray(env, napi_uint32_array, r->n, nab, 0, &narr);
      napi_set_named_property(env, out, "nBits", narr);
      napi_create_uint32(env, (uint32_t)r->stride, &sv);
      napi_set_named_property(env, out, "stride", sv);
    }
    napi_resolve_deferred(env, r->deferred, out);
  } else {
    const int rc = status == napi_ok ? r->rc : -BGV_E_ARG;
    napi_value msg, err, code;
    napi_create_string_utf8(env, bgv_strerror(rc), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int32(env, rc, &code);
    napi_set_named_property(env, err, "bgvCode", code);
    napi_reject_deferred(env, r->deferred, err);
  }
  napi_delete_reference(env, r->ctx_ref);
  napi_delete_async_work(env, r->work);
  free(r->ids);
  free(r->out96);
  free(r->count);
  free(r->status);
  free(r->bits);
  free(r->nbits);
  free(r->groups);
  free(r);
}

/* sigpoolGet(ctx, ids) and, kind 1, sigpoolGetBits(ctx, ids) -> Promise<{status, count, sigs, bits:
 * Uint8Array (n x stride), nBits: Uint32Array, stride: BGV_SIGPOOL_BITS_BYTES}>
 * (bgv_sigpool_get_bits), on a libuv pool thread like sigpoolGet */
static napi_value sigpool_get_start(napi_env env, napi_callback_info info, int kind) {
  size_t argc = 2;
  napi_value argv[2], promise, name;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t* ids;
  size_t len;
  napi_typedarray_type tt = napi_uint8_array;
  bool is_ta = false;
  if (argc < 2) return throw_code(env, -BGV_E_ARG);
  napi_is_typedarray(env, argv[1], &is_ta);
  if (is_ta) napi_get_typedarray_info(env, argv[1], &tt, NULL, NULL, NULL, NULL);
  if (!is_ta || tt != napi_uint32_array || get_bytes(env, argv[1], &ids, &len)) return throw_code(env, -BGV_E_ARG);
  pool_get_req* r = (pool_get_req*)calloc(1, sizeof(pool_get_req));
  r->c = ctx;
  r->n = len / 4;
  r->ids = (uint32_t*)calloc(r->n ? r->n : 1, sizeof(uint32_t)); /* a copy: the caller may reuse its array */
  if (r->n) memcpy(r->ids, ids, 4 * r->n);
  r->out96 = (uint8_t*)calloc(r->n ? r->n : 1, 96);
  r->count = (uint32_t*)calloc(r->n ? r->n : 1, sizeof(uint32_t));
  r->status = (int32_t*)calloc(r->n ? r->n : 1, sizeof(int32_t));
  r->kind = kind;
  if (kind) {
    r->stride = BGV_SIGPOOL_BITS_BYTES;
    r->bits = (uint8_t*)calloc(r->n ? r->n : 1, BGV_SIGPOOL_BITS_BYTES);
    r->nbits = (uint32_t*)calloc(r->n ? r->n : 1, sizeof(uint32_t));
  }
  if (napi_create_promise(env, &r->deferred, &promise) != napi_ok ||
      napi_create_reference(env, argv[0], 1, &r->ctx_ref) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu.sigpoolGet", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, pool_get_execute, pool_get_complete, r, &r->work) != napi_ok ||
      napi_queue_async_work(env, r->work) != napi_ok) {
    napi_throw_error(env, NULL, "blsgpu: N-API failure");
    return NULL;
  }
  return promise;
}

static napi_value js_sigpool_get(napi_env env, napi_callback_info info) { return sigpool_get_start(env, info, 0); }
static napi_value js_sigpool_get_bits(napi_env env, napi_callback_info info) { return sigpool_get_start(env, info, 1); }

/* sigpoolSum(ctx, ids: Uint32Array, lengths: Uint32Array) -> Promise<{status, count, sigs, bits, nBits,
 * stride}>: bgv_sigpool_sum over lengths.length groups, group g being the next lengths[g] ids; on a
 * libuv pool thread.  stride is BGV_SIGPOOL_BITS_BYTES times the longest group (at most
 * BGV_MAX_SUM_ENTRIES), which every group's field fits. */
static napi_value js_sigpool_sum(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], promise, name;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t *ids, *lens;
  size_t ilen, llen;
  napi_typedarray_type ti = napi_uint8_array, tl = napi_uint8_array;
  bool ta_i = false, ta_l = false;
  if (argc < 3) return throw_code(env, -BGV_E_ARG);
  napi_is_typedarray(env, argv[1], &ta_i);
  napi_is_typedarray(env, argv[2], &ta_l);
  if (ta_i) napi_get_typedarray_info(env, argv[1], &ti, NULL, NULL, NULL, NULL);
  if (ta_l) napi_get_typedarray_info(env, argv[2], &tl, NULL, NULL, NULL, NULL);
  if (!ta_i || !ta_l || ti != napi_uint32_array || tl != napi_uint32_array || get_bytes(env, argv[1], &ids, &ilen) ||
      get_bytes(env, argv[2], &lens, &llen))
    return throw_code(env, -BGV_E_ARG);
  const size_t ng = llen / 4, ni = ilen / 4;
  size_t total = 0, longest = 1;
  for (size_t g = 0; g < ng; ++g) {
    const uint32_t l = ((const uint32_t*)lens)[g];
    if (l == 0 || l > BGV_MAX_SUM_ENTRIES) return throw_code(env, -BGV_E_ARG);
    total += l;
    if (l > longest) longest = l;
  }
  if (total != ni || ng > 65536) return throw_code(env, -BGV_E_ARG);
  pool_get_req* r = (pool_get_req*)calloc(1, sizeof(pool_get_req));
  r->c = ctx;
  r->kind = 2;
  r->n = ng;
  r->ids = (uint32_t*)calloc(ni ? ni : 1, sizeof(uint32_t)); /* a copy: the caller may reuse its arrays */
  if (ni) memcpy(r->ids, ids, 4 * ni);
  r->groups = (bgv_poolgroup*)calloc(ng ? ng : 1, sizeof(bgv_poolgroup));
  for (size_t g = 0, at = 0; g < ng; ++g) {
    r->groups[g].ids = r->ids + at;
    r->groups[g].n_ids = ((const uint32_t*)lens)[g];
    at += r->groups[g].n_ids;
  }
  r->stride = BGV_SIGPOOL_BITS_BYTES * longest;
  r->out96 = (uint8_t*)calloc(ng ? ng : 1, 96);
  r->count = (uint32_t*)calloc(ng ? ng : 1, sizeof(uint32_t));
  r->status = (int32_t*)calloc(ng ? ng : 1, sizeof(int32_t));
  r->bits = (uint8_t*)calloc(ng ? ng : 1, r->stride);
  r->nbits = (uint32_t*)calloc(ng ? ng : 1, sizeof(uint32_t));
  if (napi_create_promise(env, &r->deferred, &promise) != napi_ok ||
      napi_create_reference(env, argv[0], 1, &r->ctx_ref) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu.sigpoolSum", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, pool_get_execute, pool_get_complete, r, &r->work) != napi_ok ||
      napi_queue_async_work(env, r->work) != napi_ok) {
    napi_throw_error(env, NULL, "blsgpu: N-API failure");
    return NULL;
  }
  return promise;
}

/* shufflingPut(ctx, firstId, seed: Uint8Array(32), activeIndices: Uint32Array, slots,
 * committeesPerSlot, rounds) -> Promise<Uint32Array>: bgv_shuffling_put on a libuv pool thread (the
 * device call never holds the event loop); resolves to the epoch's shuffling
 * (IEpochShuffling.shuffling, util/epochShuffling.ts:90-96), rejects with an Error whose .bgvCode
 * is the negative library code. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref ctx_ref, act_ref, out_ref;
  bgv_ctx* c;
  uint32_t first, slots, cps, rounds;
  uint8_t seed[32];
  const uint32_t* active;
  uint32_t* out;
  size_t n;
  int rc;
} shuf_req;

static void shuf_execute(napi_env env, void* data) {
  (void)env;
  shuf_req* r = (shuf_req*)data;
  r->rc = bgv_shuffling_put(r->c, r->first, r->seed, r->active, r->n, r->slots, r->cps, r->rounds, r->out);
}

static void shuf_complete(napi_env env, napi_status status, void* data) {
  shuf_req* r = (shuf_req*)data;
  napi_value out;
  if (status == napi_ok && r->rc == 0 && napi_get_reference_value(env, r->out_ref, &out) == napi_ok) {
    napi_resolve_deferred(env, r->deferred, out);
  } else {
    const int rc = status == napi_ok && r->rc ? r->rc : -BGV_E_ARG;
    napi_value msg, err, code;
    napi_create_string_utf8(env, bgv_strerror(rc), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int32(env, rc, &code);
    napi_set_named_property(env, err, "bgvCode", code);
    napi_reject_deferred(env, r->deferred, err);
  }
  napi_delete_reference(env, r->ctx_ref);
  napi_delete_reference(env, r->act_ref);
  napi_delete_reference(env, r->out_ref);
  napi_delete_async_work(env, r->work);
  free(r);
}

static napi_value js_shuffling_put(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7], promise, name, ab, out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t *seed, *act;
  size_t seed_len, act_len;
  uint32_t first = 0, slots = 0, cps = 0, rounds = 0;
  if (argc < 7 || napi_get_value_uint32(env, argv[1], &first) != napi_ok ||
      get_bytes(env, argv[2], &seed, &seed_len) || seed_len != 32 || get_bytes(env, argv[3], &act, &act_len) ||
      act_len % 4 || act_len == 0 || napi_get_value_uint32(env, argv[4], &slots) != napi_ok ||
      napi_get_value_uint32(env, argv[5], &cps) != napi_ok || napi_get_value_uint32(env, argv[6], &rounds) != napi_ok)
    return throw_code(env, -BGV_E_ARG);
  void* dst;
  CHECK(env, napi_create_arraybuffer(env, act_len, &dst, &ab));
  CHECK(env, napi_create_typedarray(env, napi_uint32_array, act_len / 4, ab, 0, &out));
  shuf_req* r = (shuf_req*)calloc(1, sizeof(shuf_req));
  r->c = ctx;
  r->first = first;
  r->slots = slots;
  r->cps = cps;
  r->rounds = rounds;
  memcpy(r->seed, seed, 32);
  r->active = (const uint32_t*)act;
  r->out = (uint32_t*)dst;
  r->n = act_len / 4;
  if (napi_create_promise(env, &r->deferred, &promise) != napi_ok ||
      napi_create_reference(env, argv[0], 1, &r->ctx_ref) != napi_ok ||
      napi_create_reference(env, argv[3], 1, &r->act_ref) != napi_ok ||
      napi_create_reference(env, out, 1, &r->out_ref) != napi_ok ||
      napi_create_string_utf8(env, "blsgpu.shufflingPut", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, shuf_execute, shuf_complete, r, &r->work) != napi_ok ||
      napi_queue_async_work(env, r->work) != napi_ok) {
    napi_throw_error(env, NULL, "blsgpu: N-API failure");
    return NULL;
  }
  return promise;
}

/* proposers(ctx, seeds: Uint8Array(32 k), activeIndices: Uint32Array, effectiveBalanceIncrements:
 * Uint8Array, maxIncr, rounds) -> Promise<Uint32Array(k)> (bgv_proposers; 0xFFFFFFFF: no proposer)
 * and syncCommitteePut(ctx, id, seed: Uint8Array(32), activeIndices, effectiveBalanceIncrements,
 * maxIncr, size, rounds) -> Promise<{indices: Uint32Array(size), aggregatePubkey: Uint8Array(48)}>
 * (bgv_sync_committee_put), both on a libuv pool thread like shufflingPut and rejecting with an
 * Error whose .bgvCode is the negative library code.  proposersElectra and syncCommitteePutElectra
 * are the same two under Electra's rule (bgv_proposers_electra, bgv_sync_committee_put_electra):
 * effectiveBalanceIncrements is a Uint16Array, everything else as above. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref ctx_ref, seed_ref, act_ref, eff_ref, out_ref, agg_ref;
  bgv_ctx* c;
  int sync;    /* syncCommitteePut, else proposers */
  int electra; /* eff holds uint16_t, the calls are the _electra ones */
  uint32_t id, n_seeds, max_incr, size, rounds;
  const uint8_t* seeds;
  const void* eff;
  const uint32_t* active;
  size_t n, n_eff;
  uint32_t* out;
  uint8_t* agg;
  int rc;
} samp_req;

static void samp_execute(napi_env env, void* data) {
  (void)env;
  samp_req* r = (samp_req*)data;
  if (r->sync && r->electra)
    r->rc = bgv_sync_committee_put_electra(r->c, r->id, r->seeds, r->active, r->n, (const uint16_t*)r->eff, r->n_eff,
                                           r->max_incr, r->size, r->rounds, r->out, r->agg);
  else if (r->sync)
    r->rc = bgv_sync_committee_put(r->c, r->id, r->seeds, r->active, r->n, (const uint8_t*)r->eff, r->n_eff,
                                   r->max_incr, r->size, r->rounds, r->out, r->agg);
  else if (r->electra)
    r->rc = bgv_proposers_electra(r->c, r->seeds, r->n_seeds, r->active, r->n, (const uint16_t*)r->eff, r->n_eff,
                                  r->max_incr, r->rounds, r->out);
  else
    r->rc = bgv_proposers(r->c, r->seeds, r->n_seeds, r->active, r->n, (const uint8_t*)r->eff, r->n_eff, r->max_incr,
                          r->rounds, r->out);
}

static void samp_complete(napi_env env, napi_status status, void* data) {
  samp_req* r = (samp_req*)data;
  napi_value out, agg, res;
  int ok = status == napi_ok && r->rc == 0 && napi_get_reference_value(env, r->out_ref, &out) == napi_ok;
  if (ok && r->sync) {
    ok = napi_get_reference_value(env, r->agg_ref, &agg) == napi_ok && napi_create_object(env, &res) == napi_ok &&
         napi_set_named_property(env, res, "indices", out) == napi_ok &&
         napi_set_named_property(env, res, "aggregatePubkey", agg) == napi_ok;
    out = res;
  }
  if (ok) {
    napi_resolve_deferred(env, r->deferred, out);
  } else {
    const int rc = status == napi_ok && r->rc ? r->rc : -BGV_E_ARG;
    napi_value msg, err, code;
    napi_create_string_utf8(env, bgv_strerror(rc), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int32(env, rc, &code);
    napi_set_named_property(env, err, "bgvCode", code);
    napi_reject_deferred(env, r->deferred, err);
  }
  napi_delete_reference(env, r->ctx_ref);
  napi_delete_reference(env, r->seed_ref);
  napi_delete_reference(env, r->act_ref);
  napi_delete_reference(env, r->eff_ref);
  napi_delete_reference(env, r->out_ref);
  if (r->agg_ref) napi_delete_reference(env, r->agg_ref);
  napi_delete_async_work(env, r->work);
  free(r);
}

/* argv[0] the context, then for sync [id, seed, active, eff, maxIncr, size, rounds], else
 * [seeds, active, eff, maxIncr, rounds]; eff a Uint16Array when electra, else a Uint8Array */
static napi_value samp_start(napi_env env, napi_callback_info info, int sync, int electra) {
  size_t argc = 8;
  napi_value argv[8], promise, name, ab, out, agg = NULL;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  const size_t a = sync ? 2 : 1; /* where the seeds are */
  uint8_t *seeds, *act;
  void* eff;
  size_t seeds_len, act_len, n_eff; /* n_eff counts elements: bytes, or uint16_t when electra */
  uint32_t id = 0, max_incr = 0, size = 0, rounds = 0;
  napi_typedarray_type act_type, eff_type;
  if (argc < (sync ? 8u : 6u) || (sync && napi_get_value_uint32(env, argv[1], &id) != napi_ok) ||
      get_bytes(env, argv[a], &seeds, &seeds_len) || seeds_len == 0 || seeds_len % 32 || (sync && seeds_len != 32) ||
      get_bytes(env, argv[a + 1], &act, &act_len) || act_len == 0 ||
      napi_get_typedarray_info(env, argv[a + 1], &act_type, NULL, NULL, NULL, NULL) != napi_ok ||
      act_type != napi_uint32_array ||
      napi_get_typedarray_info(env, argv[a + 2], &eff_type, &n_eff, &eff, NULL, NULL) != napi_ok || n_eff == 0 ||
      eff_type != (electra ? napi_uint16_array : napi_uint8_array) ||
      napi_get_value_uint32(env, argv[a + 3], &max_incr) != napi_ok ||
      (sync && napi_get_value_uint32(env, argv[a + 4], &size) != napi_ok) ||
      napi_get_value_uint32(env, argv[sync ? 7 : 5], &rounds) != napi_ok || (sync && (size < 1 || size > 65536)) ||
      seeds_len / 32 > 1024)
    return throw_code(env, -BGV_E_ARG);
  const size_t n_out = sync ? size : seeds_len / 32;
  void *dst, *agg_dst = NULL;
  CHECK(env, napi_create_arraybuffer(env, 4 * n_out, &dst, &ab));
  CHECK(env, napi_create_typedarray(env, napi_uint32_array, n_out, ab, 0, &out));
  if (sync && !(agg = new_bytes(env, 48, &agg_dst))) return throw_code(env, -BGV_E_ARG);
  samp_req* r = (samp_req*)calloc(1, sizeof(samp_req));
  r->c = ctx;
  r->sync = sync;
  r->electra = electra;
  r->id = id;
  r->n_seeds = (uint32_t)(seeds_len / 32);
  r->max_incr = max_incr;
  r->size = size;
  r->rounds = rounds;
  r->seeds = seeds;
  r->active = (const uint32_t*)act;
  r->n = act_len / 4;
  r->eff = eff;
  r->n_eff = n_eff;
  r->out = (uint32_t*)dst;
  r->agg = (uint8_t*)agg_dst;
  if (napi_create_promise(env, &r->deferred, &promise) != napi_ok ||
      napi_create_reference(env, argv[0], 1, &r->ctx_ref) != napi_ok ||
      napi_create_reference(env, argv[a], 1, &r->seed_ref) != napi_ok ||
      napi_create_reference(env, argv[a + 1], 1, &r->act_ref) != napi_ok ||
      napi_create_reference(env, argv[a + 2], 1, &r->eff_ref) != napi_ok ||
      napi_create_reference(env, out, 1, &r->out_ref) != napi_ok ||
      (sync && napi_create_reference(env, agg, 1, &r->agg_ref) != napi_ok) ||
      napi_create_string_utf8(env, sync ? "blsgpu.syncCommitteePut" : "blsgpu.proposers", NAPI_AUTO_LENGTH, &name) !=
          napi_ok || /* one resource name for both rules */
      napi_create_async_work(env, NULL, name, samp_execute, samp_complete, r, &r->work) != napi_ok ||
      napi_queue_async_work(env, r->work) != napi_ok) {
    napi_throw_error(env, NULL, "blsgpu: N-API failure");
    return NULL;
  }
  return promise;
}

static napi_value js_proposers(napi_env env, napi_callback_info info) { return samp_start(env, info, 0, 0); }
static napi_value js_sync_committee_put(napi_env env, napi_callback_info info) { return samp_start(env, info, 1, 0); }
static napi_value js_proposers_electra(napi_env env, napi_callback_info info) { return samp_start(env, info, 0, 1); }
static napi_value js_sync_committee_put_electra(napi_env env, napi_callback_info info) {
  return samp_start(env, info, 1, 1);
}

/* aggregateCommitteeBits(ctx, id, bits: Uint8Array, nBits) -> Uint8Array(96): the aggregate of the
 * committee members whose bit is set, through the verify path's kernel (parity hook). */
static napi_value js_aggregate_committee_bits(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t id = 0, nbits = 0;
  uint8_t* bits;
  size_t len;
  if (argc < 4 || napi_get_value_uint32(env, argv[1], &id) != napi_ok || get_bytes(env, argv[2], &bits, &len) ||
      napi_get_value_uint32(env, argv[3], &nbits) != napi_ok || len != ((size_t)nbits + 7) / 8)
    return throw_code(env, -BGV_E_ARG);
  void* dst;
  napi_value out = new_bytes(env, 96, &dst);
  if (!out) return throw_code(env, -BGV_E_ARG);
  int rc = bgv_aggregate_committee_bits(ctx, id, bits, nbits, (uint8_t*)dst);
  if (rc) return throw_code(env, rc);
  return out;
}

/* hashToG2(ctx, msg: Uint8Array) -> Uint8Array(192) uncompressed (x.c1|x.c0|y.c1|y.c0) */
static napi_value js_hash_to_g2(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t* msg;
  size_t len;
  if (get_bytes(env, argv[1], &msg, &len)) return throw_code(env, -BGV_E_ARG);
  uint32_t l32 = (uint32_t)len;
  void* dst;
  napi_value out = new_bytes(env, 192, &dst);
  if (!out) return throw_code(env, -BGV_E_ARG);
  int rc = bgv_hash_to_g2(ctx, msg, &l32, 1, (uint8_t*)dst);
  if (rc) return throw_code(env, rc);
  return out;
}

/* pubkeysValidate(ctx, keys48: Uint8Array (n x 48)) -> {status: Int32Array (0 | -BLST code),
 * uncompressed: Uint8Array (n x 96)}: PublicKey.fromBytes(pk, affine, validate=true) per key
 * (state-transition/src/block/processDeposit.ts:64). */
static napi_value js_pubkeys_validate(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t* keys;
  size_t len;
  if (get_bytes(env, argv[1], &keys, &len) || len % 48) return throw_code(env, -BGV_E_ARG);
  const size_t n = len / 48;
  int32_t* st = (int32_t*)calloc(n ? n : 1, sizeof(int32_t));
  void* dst;
  napi_value recs = new_bytes(env, 96 * n, &dst);
  if (!recs) {
    free(st);
    return throw_code(env, -BGV_E_ARG);
  }
  int rc = bgv_pubkeys_validate(ctx, keys, n, st, (uint8_t*)dst);
  if (rc) {
    free(st);
    return throw_code(env, rc);
  }
  napi_value out, status = new_int32s(env, st, n);
  free(st);
  CHECK(env, napi_create_object(env, &out));
  CHECK(env, napi_set_named_property(env, out, "status", status));
  CHECK(env, napi_set_named_property(env, out, "uncompressed", recs));
  return out;
}

/* aggregateSignatures(ctx, aggregates: Uint8Array[][]) -> {status: Int32Array, sigs: Uint8Array
 * (naggs x 96 compressed)}: Signature.aggregate over validated signatures, one entry per
 * op-pool aggregate (chain/opPools/attestationPool.ts:184-187 and siblings). */
static napi_value js_aggregate_signatures(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint32_t naggs = 0;
  if (napi_get_array_length(env, argv[1], &naggs) != napi_ok) return throw_code(env, -BGV_E_ARG);
  uint32_t* counts = (uint32_t*)calloc(naggs ? naggs : 1, sizeof(uint32_t));
  size_t total = 0;
  for (uint32_t a = 0; a < naggs; ++a) {
    napi_value agg;
    napi_get_element(env, argv[1], a, &agg);
    if (napi_get_array_length(env, agg, &counts[a]) != napi_ok) {
      free(counts);
      return throw_code(env, -BGV_E_ARG);
    }
    total += counts[a];
  }
  /* records are zero-padded to 96 B; lens carries the received size (BLST_INVALID_SIZE) */
  uint8_t* raw = (uint8_t*)calloc(total ? total : 1, 96);
  uint32_t* lens = (uint32_t*)calloc(total ? total : 1, sizeof(uint32_t));
  int32_t* st = (int32_t*)calloc(naggs ? naggs : 1, sizeof(int32_t));
  size_t k = 0;
  int bad = 0;
  for (uint32_t a = 0; a < naggs && !bad; ++a) {
    napi_value agg;
    napi_get_element(env, argv[1], a, &agg);
    for (uint32_t i = 0; i < counts[a]; ++i, ++k) {
      napi_value s;
      uint8_t* d;
      size_t l;
      napi_get_element(env, agg, i, &s);
      if (get_bytes(env, s, &d, &l)) {
        bad = 1;
        break;
      }
      memcpy(raw + 96 * k, d, l < 96 ? l : 96);
      lens[k] = (uint32_t)l;
    }
  }
  void* dst;
  napi_value sigs = bad ? NULL : new_bytes(env, 96 * (size_t)naggs, &dst);
  int rc = sigs ? bgv_aggregate_signatures(ctx, raw, lens, counts, naggs, (uint8_t*)dst, st) : -BGV_E_ARG;
  napi_value status = rc ? NULL : new_int32s(env, st, naggs);
  free(raw);
  free(lens);
  free(counts);
  free(st);
  if (rc) return throw_code(env, rc);
  napi_value out;
  CHECK(env, napi_create_object(env, &out));
  CHECK(env, napi_set_named_property(env, out, "status", status));
  CHECK(env, napi_set_named_property(env, out, "sigs", sigs));
  return out;
}

/* depositsVerify(ctx, keys48, msgs32, sigs96) -> Int32Array (1 valid, 0 invalid): the
 * deposit signature check of processDeposit.ts:62-70. */
static napi_value js_deposits_verify(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  OPEN_CTX(env, argv[0], ctx);
  uint8_t *keys, *msgs, *sigs;
  size_t lk, lm, ls;
  if (get_bytes(env, argv[1], &keys, &lk) || get_bytes(env, argv[2], &msgs, &lm) ||
      get_bytes(env, argv[3], &sigs, &ls) || lk % 48 || lm != 32 * (lk / 48) || ls != 96 * (lk / 48))
    return throw_code(env, -BGV_E_ARG);
  const size_t n = lk / 48;
  int32_t* valid = (int32_t*)calloc(n ? n : 1, sizeof(int32_t));
  int rc = bgv_deposits_verify(ctx, keys, msgs, sigs, n, valid);
  napi_value out = rc ? NULL : new_int32s(env, valid, n);
  free(valid);
  if (rc) return throw_code(env, rc);
  return out;
}

/* ---- verify: bgv_verify_async + threadsafe completion + Promise ----------- */
static void free_req_heap(verify_req* r) {
  free(r->refs);
  free(r->jobs);
  free(r->sets);
  free(r->pkbits);
  free(r->spans);
  free(r->codes);
  free(r->tags);
  free(r->agg96);
  free(r->agg_status);
  free(r->agg_count);
  free(r->added);
  free(r->poolbits);
  free(r);
}

static void free_req(napi_env env, verify_req* r) {
  for (size_t i = 0; i < r->nrefs; ++i) napi_delete_reference(env, r->refs[i]);
  if (r->ctx_ref) napi_delete_reference(env, r->ctx_ref);
  free_req_heap(r);
}

static void settle(napi_env env, verify_req* r) {
  if (r->rc) {
    napi_value err, msg;
    napi_create_string_utf8(env, bgv_strerror(r->rc), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, r->deferred, err);
    return;
  }
  napi_value ab, arr;
  void* dst;
  napi_create_arraybuffer(env, 4 * r->njobs, &dst, &ab);
  memcpy(dst, r->codes, 4 * r->njobs);
  napi_create_typedarray(env, napi_int32_array, r->njobs, ab, 0, &arr);
  /* codes.stats: the call's BlsWorkResult-style counters (multithread/types.ts:24-36) */
  napi_value st, v;
  napi_create_object(env, &st);
  napi_create_double(env, (double)r->stats.batch_retries, &v);
  napi_set_named_property(env, st, "batchRetries", v);
  napi_create_double(env, (double)r->stats.batch_sigs_success, &v);
  napi_set_named_property(env, st, "batchSigsSuccess", v);
  napi_create_double(env, (double)r->stats.device_groups, &v);
  napi_set_named_property(env, st, "deviceGroups", v);
  napi_create_double(env, (double)r->stats.sets_verified, &v);
  napi_set_named_property(env, st, "setsVerified", v);
  napi_create_double(env, r->stats.device_ms, &v);
  napi_set_named_property(env, st, "deviceMs", v);
  napi_create_double(env, r->stats.wall_ms, &v);
  napi_set_named_property(env, st, "wallMs", v);
  napi_set_named_property(env, arr, "stats", st);
  if (!r->aggregate) {
    napi_resolve_deferred(env, r->deferred, arr);
    return;
  }
  /* verifyAggregate: {codes, stats, aggs: {status, count, sigs}}; verifyAccumulate: {codes, stats, added} */
  napi_value res, aggs, sab, sarr, cab, carr, sigs;
  napi_create_object(env, &res);
  napi_set_named_property(env, res, "codes", arr);
  napi_set_named_property(env, res, "stats", st);
  if (r->aggregate >= 2) {
    napi_value added = new_bytes(env, r->nsets, &dst);
    if (r->nsets) memcpy(dst, r->added, r->nsets);
    napi_set_named_property(env, res, r->aggregate == 3 ? "outcome" : "added", added);
    napi_resolve_deferred(env, r->deferred, res);
    return;
  }
  napi_create_object(env, &aggs);
  napi_create_arraybuffer(env, 4 * r->naggs, &dst, &sab);
  memcpy(dst, r->agg_status, 4 * r->naggs);
  napi_create_typedarray(env, napi_int32_array, r->naggs, sab, 0, &sarr);
  napi_set_named_property(env, aggs, "status", sarr);
  napi_create_arraybuffer(env, 4 * r->naggs, &dst, &cab);
  memcpy(dst, r->agg_count, 4 * r->naggs);
  napi_create_typedarray(env, napi_uint32_array, r->naggs, cab, 0, &carr);
  napi_set_named_property(env, aggs, "count", carr);
  sigs = new_bytes(env, 96 * r->naggs, &dst);
  memcpy(dst, r->agg96, 96 * r->naggs);
  napi_set_named_property(env, aggs, "sigs", sigs);
  napi_set_named_property(env, res, "aggs", aggs);
  napi_resolve_deferred(env, r->deferred, res);
}

/* main thread: a verify finished on a dispatcher thread */
static void verify_call_js(napi_env env, napi_value js_cb, void* context, void* data) {
  (void)js_cb;
  (void)context;
  verify_req* r = (verify_req*)data;
  if (env) {
    addon_ctx* a = r->actx;
    settle(env, r);
    if (--a->inflight == 0 && !a->tsfn_released) napi_unref_threadsafe_function(env, a->tsfn);
    free_req(env, r);
  } else {
    /* environment teardown drained the queue: no JS to settle (the promise dies with the
     * environment) and no env for the references (they die with it too); free the heap part */
    free_req_heap(r);
  }
}

/* dispatcher thread (library): codes and stats are filled; hop to the main thread */
static void verify_done(void* user, int rc) {
  verify_req* r = (verify_req*)user;
  r->rc = rc;
  napi_call_threadsafe_function(r->actx->tsfn, r, napi_tsfn_nonblocking);
}

/* the runtime finalized the tsfn (after close() released it, or at environment teardown) */
static void tsfn_finalized(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  addon_ctx* a = (addon_ctx*)data;
  a->tsfn_released = 1;
  addon_unref(a);
}

/* the ctx external was collected: no verify references it any more */
static void addon_finalize(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  addon_ctx* a = (addon_ctx*)data;
  if (!a) return;
  if (!a->closed) {
    a->closed = 1;
    bgv_close(a->c);
  }
  if (!a->tsfn_released) {
    a->tsfn_released = 1;
    napi_release_threadsafe_function(a->tsfn, napi_tsfn_abort);
  }
  addon_unref(a);
}

/* verify(ctx, jobs, mode) resolves to the codes (an Int32Array with .stats); verifyAggregate(ctx,
 * jobs, mode), whose sets may carry `agg: number` (the aggregate the set's signature joins when its
 * job is accepted; bgv_verify_aggregate), to {codes, stats, aggs: {status, count, sigs}} with one
 * entry per aggregate 0 .. the largest agg given; verifyAccumulate(ctx, jobs, mode), whose sets may
 * carry `pool: number` (the open signature pool entry the set's signature is added to when its job
 * is accepted; bgv_verify_accumulate), to {codes, stats, added: Uint8Array (1 per set that was added)};
 * verifyAccumulateBits(ctx, jobs, mode), whose sets carry `pool` and, for an entry with bits,
 * `poolNBits` with `poolBit` (the set's position) or `poolBits` (its field, a Uint8Array of
 * ceil(poolNBits / 8) bytes; bgv_verify_accumulate_bits), to {codes, stats, outcome: Uint8Array
 * (BGV_POOL_* per set)} */
static napi_value verify_start(napi_env env, napi_callback_info info, int aggregate) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  addon_ctx* a = get_actx(env, argv[0]);
  if (!a || a->closed) { /* the Promise rejects (QUEUE_ABORTED), as every verify outcome is async */
    napi_deferred d;
    napi_value promise, err, msg;
    CHECK(env, napi_create_promise(env, &d, &promise));
    napi_create_string_utf8(env, bgv_strerror(-BGV_E_CLOSED), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, d, err);
    return promise;
  }
  verify_req* r = (verify_req*)calloc(1, sizeof(verify_req));
  r->actx = a;
  r->aggregate = aggregate;
  int32_t mode = 0;
  if (argc >= 3) napi_get_value_int32(env, argv[2], &mode);
  r->mode = mode;
  uint32_t njobs = 0;
  napi_get_array_length(env, argv[1], &njobs);
  r->njobs = njobs;
  r->jobs = (bgv_job*)calloc(njobs ? njobs : 1, sizeof(bgv_job));
  r->codes = (int32_t*)calloc(njobs ? njobs : 1, sizeof(int32_t));
  size_t cap = 64;
  r->sets = (bgv_set*)calloc(cap, sizeof(bgv_set));
  r->pkbits = (bgv_pkbits*)calloc(cap, sizeof(bgv_pkbits));
  r->spans = (bgv_pkspan*)calloc(cap, sizeof(bgv_pkspan));
  r->tags = (uint32_t*)calloc(cap, sizeof(uint32_t));
  if (aggregate == 3) r->poolbits = (bgv_poolbits*)calloc(cap, sizeof(bgv_poolbits));
  size_t refcap = 256;
  r->refs = (napi_ref*)calloc(refcap, sizeof(napi_ref));
  for (uint32_t j = 0; j < njobs; ++j) {
    napi_value job, sets, bval;
    napi_get_element(env, argv[1], j, &job);
    napi_get_named_property(env, job, "sets", &sets);
    napi_get_named_property(env, job, "batchable", &bval);
    bool batchable = false;
    napi_get_value_bool(env, bval, &batchable);
    uint32_t ns = 0;
    napi_get_array_length(env, sets, &ns);
    r->jobs[j].first_set = (uint32_t)r->nsets;
    r->jobs[j].n_sets = ns;
    r->jobs[j].batchable = batchable;
    for (uint32_t k = 0; k < ns; ++k) {
      if (r->nsets == cap) {
        cap *= 2;
        r->sets = (bgv_set*)realloc(r->sets, cap * sizeof(bgv_set));
        r->pkbits = (bgv_pkbits*)realloc(r->pkbits, cap * sizeof(bgv_pkbits));
        r->spans = (bgv_pkspan*)realloc(r->spans, cap * sizeof(bgv_pkspan));
        r->tags = (uint32_t*)realloc(r->tags, cap * sizeof(uint32_t));
        if (aggregate == 3) r->poolbits = (bgv_poolbits*)realloc(r->poolbits, cap * sizeof(bgv_poolbits));
      }
      if (r->nrefs + 4 > refcap) {
        refcap *= 2;
        r->refs = (napi_ref*)realloc(r->refs, refcap * sizeof(napi_ref));
      }
      napi_value s, pk, msg, sig;
      napi_get_element(env, sets, k, &s);
      /* pkIndices (validator indices into the device cache), pkBytes (n x 96-B uncompressed), or
       * committee + bits + nBits (the members of a committee stored with committeePut whose bit is
       * set, SSZ bit order: bgv_pkbits), or committees (a Uint32Array of ids) + bits + nBits (one
       * bitfield over those committees in order: bgv_pkspan) */
      bool by_index = false, by_committee = false, by_span = false;
      napi_has_named_property(env, s, "committees", &by_span);
      napi_has_named_property(env, s, "committee", &by_committee);
      by_committee = by_committee || by_span;
      napi_has_named_property(env, s, "pkIndices", &by_index);
      napi_get_named_property(env, s, by_committee ? "bits" : by_index ? "pkIndices" : "pkBytes", &pk);
      napi_get_named_property(env, s, "msg", &msg);
      napi_get_named_property(env, s, "sig", &sig);
      bgv_pkbits* pb = &r->pkbits[r->nsets];
      pb->committee = BGV_NO_COMMITTEE;
      pb->n_bits = 0;
      pb->bits = NULL;
      memset(&r->spans[r->nsets], 0, sizeof(bgv_pkspan));
      r->tags[r->nsets] = BGV_NO_AGG;
      bool tagged = false;
      if (aggregate) napi_has_named_property(env, s, aggregate >= 2 ? "pool" : "agg", &tagged);
      if (aggregate == 3) { /* poolNBits with poolBit (one position) or poolBits (a field; the library copies it) */
        bgv_poolbits* pq = &r->poolbits[r->nsets];
        bool has_n = false, has_bit = false, has_bits = false;
        memset(pq, 0, sizeof(*pq));
        napi_has_named_property(env, s, "poolNBits", &has_n);
        napi_has_named_property(env, s, "poolBit", &has_bit);
        napi_has_named_property(env, s, "poolBits", &has_bits);
        if (has_n) {
          napi_value nv, bv;
          uint8_t* bd;
          size_t bl;
          int bad = napi_get_named_property(env, s, "poolNBits", &nv) != napi_ok ||
                    napi_get_value_uint32(env, nv, &pq->n_bits) != napi_ok || has_bit == has_bits;
          if (!bad && has_bit)
            bad = napi_get_named_property(env, s, "poolBit", &bv) != napi_ok ||
                  napi_get_value_uint32(env, bv, &pq->bit) != napi_ok;
          if (!bad && has_bits) {
            bad = napi_get_named_property(env, s, "poolBits", &bv) != napi_ok || get_bytes(env, bv, &bd, &bl) ||
                  bl != ((size_t)pq->n_bits + 7) / 8 || bl == 0;
            if (!bad) pq->bits = bd; /* read inside the submit below, on this thread */
          }
          if (bad) {
            free_req(env, r);
            return throw_code(env, -BGV_E_ARG);
          }
        }
      }
      if (tagged) {
        napi_value av;
        uint32_t tag = 0;
        napi_get_named_property(env, s, aggregate >= 2 ? "pool" : "agg", &av);
        if (napi_get_value_uint32(env, av, &tag) != napi_ok || tag >= (aggregate >= 2 ? BGV_MAX_SIGPOOL : (1u << 20))) {
          free_req(env, r);
          return throw_code(env, -BGV_E_ARG);
        }
        r->tags[r->nsets] = tag;
        if ((size_t)tag + 1 > r->naggs) r->naggs = (size_t)tag + 1;
      }
      bgv_set* st = &r->sets[r->nsets++];
      memset(st, 0, sizeof(*st));
      uint8_t *pkd, *md, *sd;
      size_t pkl, ml, sl;
      if (get_bytes(env, pk, &pkd, &pkl) || get_bytes(env, msg, &md, &ml) || get_bytes(env, sig, &sd, &sl) ||
          ml != 32 || (!by_index && !by_committee && pkl % 96)) {
        free_req(env, r);
        return throw_code(env, -BGV_E_ARG);
      }
      if (by_span) {
        napi_value cv, nv;
        uint8_t* cd;
        size_t cl;
        uint32_t nbits = 0;
        napi_typedarray_type tt = napi_uint8_array;
        bool is_ta = false;
        napi_get_named_property(env, s, "committees", &cv);
        napi_get_named_property(env, s, "nBits", &nv);
        napi_is_typedarray(env, cv, &is_ta);
        if (is_ta) napi_get_typedarray_info(env, cv, &tt, NULL, NULL, NULL, NULL);
        if (!is_ta || tt != napi_uint32_array || get_bytes(env, cv, &cd, &cl) || cl == 0 ||
            napi_get_value_uint32(env, nv, &nbits) != napi_ok || pkl != ((size_t)nbits + 7) / 8) {
          free_req(env, r);
          return throw_code(env, -BGV_E_ARG);
        }
        bgv_pkspan* sp = &r->spans[r->nsets - 1];
        sp->committees = (const uint32_t*)cd;
        sp->n_committees = (uint32_t)(cl / 4);
        sp->n_bits = nbits;
        sp->bits = pkd;
        r->any_span = 1;
        napi_create_reference(env, cv, 1, &r->refs[r->nrefs++]);
      } else if (by_committee) {
        napi_value cv, nv;
        uint32_t cid = 0, nbits = 0;
        napi_get_named_property(env, s, "committee", &cv);
        napi_get_named_property(env, s, "nBits", &nv);
        if (napi_get_value_uint32(env, cv, &cid) != napi_ok || napi_get_value_uint32(env, nv, &nbits) != napi_ok ||
            cid == BGV_NO_COMMITTEE || pkl != ((size_t)nbits + 7) / 8) {
          free_req(env, r);
          return throw_code(env, -BGV_E_ARG);
        }
        pb->committee = cid;
        pb->n_bits = nbits;
        pb->bits = pkd;
        r->any_committee = 1;
      } else if (by_index) {
        st->n_pk = (uint32_t)(pkl / 4);
        st->pk_indices = (const uint32_t*)pkd;
      } else {
        st->n_pk = (uint32_t)(pkl / 96);
        st->pk_bytes = pkd;
      }
      st->msg = md;
      st->sig = sd;
      st->sig_len = (uint32_t)sl;
      napi_create_reference(env, pk, 1, &r->refs[r->nrefs++]);
      napi_create_reference(env, msg, 1, &r->refs[r->nrefs++]);
      napi_create_reference(env, sig, 1, &r->refs[r->nrefs++]);
    }
  }
  napi_value promise;
  CHECK(env, napi_create_promise(env, &r->deferred, &promise));
  /* the ctx external stays alive (no finalizer) until this request completes */
  CHECK(env, napi_create_reference(env, argv[0], 1, &r->ctx_ref));
  if (a->inflight++ == 0) napi_ref_threadsafe_function(env, a->tsfn);
  int rc;
  if (aggregate >= 2) {
    r->added = (uint8_t*)calloc(r->nsets ? r->nsets : 1, 1);
  } else if (aggregate) {
    r->agg96 = (uint8_t*)calloc(r->naggs ? r->naggs : 1, 96);
    r->agg_status = (int32_t*)calloc(r->naggs ? r->naggs : 1, sizeof(int32_t));
    r->agg_count = (uint32_t*)calloc(r->naggs ? r->naggs : 1, sizeof(uint32_t));
  }
  if (r->any_span || (aggregate && r->any_committee)) { /* the one-committee sets of the call as spans of one committee */
    for (size_t i = 0; i < r->nsets; ++i)
      if (r->pkbits[i].committee != BGV_NO_COMMITTEE) {
        r->spans[i].committees = &r->pkbits[i].committee;
        r->spans[i].n_committees = 1;
        r->spans[i].n_bits = r->pkbits[i].n_bits;
        r->spans[i].bits = r->pkbits[i].bits;
      }
    r->any_span = 1;
  }
  if (aggregate == 3) {
    rc = bgv_verify_accumulate_bits_async(a->c, r->jobs, r->njobs, r->sets, r->nsets, r->any_span ? r->spans : NULL,
                                          r->mode, r->tags, r->poolbits, r->codes, r->added, &r->stats, verify_done, r);
  } else if (aggregate == 2) {
    rc = bgv_verify_accumulate_async(a->c, r->jobs, r->njobs, r->sets, r->nsets, r->any_span ? r->spans : NULL, r->mode,
                                     r->tags, r->codes, r->added, &r->stats, verify_done, r);
  } else if (aggregate) {
    rc = bgv_verify_aggregate_async(a->c, r->jobs, r->njobs, r->sets, r->nsets, r->any_span ? r->spans : NULL, r->mode,
                                    r->tags, r->naggs, r->codes, r->agg96, r->agg_status, r->agg_count, &r->stats,
                                    verify_done, r);
  } else if (r->any_span) {
    rc = bgv_verify_spans_async(a->c, r->jobs, r->njobs, r->sets, r->nsets, r->spans, r->mode, r->codes, &r->stats,
                                verify_done, r);
  } else {
    rc = bgv_verify_bits_async(a->c, r->jobs, r->njobs, r->sets, r->nsets, r->any_committee ? r->pkbits : NULL,
                               r->mode, r->codes, &r->stats, verify_done, r);
  }
  if (rc) { /* rejected before queueing (closed, bad arguments): settle now */
    r->rc = rc;
    settle(env, r);
    if (--a->inflight == 0) napi_unref_threadsafe_function(env, a->tsfn);
    free_req(env, r);
  }
  return promise;
}

static napi_value js_verify(napi_env env, napi_callback_info info) { return verify_start(env, info, 0); }
static napi_value js_verify_aggregate(napi_env env, napi_callback_info info) { return verify_start(env, info, 1); }
static napi_value js_verify_accumulate(napi_env env, napi_callback_info info) { return verify_start(env, info, 2); }
static napi_value js_verify_accumulate_bits(napi_env env, napi_callback_info info) {
  return verify_start(env, info, 3);
}

#define METHOD_ATTR ((napi_property_attributes)(napi_writable | napi_enumerable | napi_configurable))

static napi_value init_module(napi_env env, napi_value exports) {
  napi_property_descriptor d[] = {
      {"init", NULL, js_init, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"close", NULL, js_close, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"strerror", NULL, js_strerror, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"pubkeysPut", NULL, js_pubkeys_put, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"pubkeysPutAsync", NULL, js_pubkeys_put_async, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"keygen", NULL, js_keygen, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"sign", NULL, js_sign, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"verify", NULL, js_verify, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"verifyAggregate", NULL, js_verify_aggregate, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"verifyAccumulate", NULL, js_verify_accumulate, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"sigpoolOpen", NULL, js_sigpool_open, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"sigpoolDropRange", NULL, js_sigpool_drop_range, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"sigpoolGet", NULL, js_sigpool_get, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"verifyAccumulateBits", NULL, js_verify_accumulate_bits, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"sigpoolOpenBits", NULL, js_sigpool_open_bits, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"sigpoolGetBits", NULL, js_sigpool_get_bits, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"sigpoolSum", NULL, js_sigpool_sum, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"aggregatePubkeys", NULL, js_aggregate_pubkeys, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"committeePut", NULL, js_committee_put, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"committeeDrop", NULL, js_committee_drop, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"committeeDropRange", NULL, js_committee_drop_range, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"shufflingPut", NULL, js_shuffling_put, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"proposers", NULL, js_proposers, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"syncCommitteePut", NULL, js_sync_committee_put, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"proposersElectra", NULL, js_proposers_electra, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"syncCommitteePutElectra", NULL, js_sync_committee_put_electra, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"aggregateCommitteeBits", NULL, js_aggregate_committee_bits, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"hashToG2", NULL, js_hash_to_g2, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"pubkeysValidate", NULL, js_pubkeys_validate, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"aggregateSignatures", NULL, js_aggregate_signatures, NULL, NULL, NULL, METHOD_ATTR, NULL},
      {"depositsVerify", NULL, js_deposits_verify, NULL, NULL, NULL, METHOD_ATTR, NULL},
  };
  napi_define_properties(env, exports, sizeof(d) / sizeof(d[0]), d);
  napi_value n;
  napi_create_int32(env, bgv_device_count(), &n);
  napi_set_named_property(env, exports, "deviceCount", n);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init_module)
