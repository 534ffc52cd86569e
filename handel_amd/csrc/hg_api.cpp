// hg_api.cpp — host side of the C ABI declared in include/handel_gpu.h: the
// context's lifetime, the message, the registry and the single-check calls.
// Aggregate verification is in hg_aggregate.cpp, its GT tables in
// hg_gttables.cpp, the service lanes in hg_lanes.cpp, its random-linear-
// combination form in hg_rlc.cpp, packet intake and the stores in hg_intake.cpp, the batches
// whose checks each carry their own message in hg_msgs.cpp; the state they
// share is hg_ctx.h.
//
// Mirrors the reference's call structure:
//   Constructor / G2Base           -> hg_create (+ the G2Base line table)
//   registry PublicKey.Unmarshal   -> hg_registry_load (simul/lib/nodes.go:44-64)
//   hashedMessage                  -> hg_set_message (once per message)
//   PublicKey.VerifySignature      -> hg_verify_batch
//   processing.go verifySignature  -> hg_verify_aggregate (hg_aggregate.cpp)
// Error precedence follows the order in which the reference surfaces errors:
// unmarshal (at parse time) > bitset/level check > hashedMessage EOF >
// nil-aggregate panic > pairing verdict.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hg_ctx.h"
#include "hg_sha256.h"

namespace {

__global__ void k_fill_codes(int32_t* c, int n, int32_t from, int32_t to) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && c[i] == from) c[i] = to;
}
}  // namespace

// config 2, in its split form (launch_verify_split: the Miller loop on a
// compact team region, the 12-lane final exponentiation) on split_ws where
// verify_split_for chose it (hg_set_verify_split); false: refused, nothing ran
static bool timed_verify(hg_ctx* c, const CheckIn* in, int n, int32_t* codes, hipStream_t s,
                         uint8_t* split_ws = nullptr) {
  PhaseTimer t(c, HG_PHASE_VERIFY, s);
  bool ok = true;
  if (split_ws) ok = launch_verify_split(in, n, c->d_lines.p, c->cur.d_h.p, codes, split_ws, s);
  else launch_verify(in, n, c->d_lines.p, c->cur.d_h.p, codes, s);
  t.stop();
  return ok;
}

static bool same_msg(const std::vector<uint8_t>& m, const uint8_t* msg, size_t len) {
  return m.size() == len && (len == 0 || memcmp(m.data(), msg, len) == 0);
}

// hashedMessage into d_h (the caller holds the lock); HG_OK or HG_ERR_HASH_EOF.
// The context keeps two messages (bn256/go/bn256.go:210-218: H and with it
// every GT table is fixed per message): the current one and the previous one.
// Switching back to the previous message swaps the two sets and keeps its
// tables; a third message takes over the older set's buffers (level 0, its
// tables rebuilt on demand). The hash and any later rebuild run in
// submission order, after every submission that still reads the old set.
int set_message_locked(hg_ctx* c, const uint8_t* msg, size_t len) {
  HG_CHECK(c, hipSetDevice(c->device));
  if (c->cur.has_msg && same_msg(c->cur.msg, msg, len)) return c->cur.hash_eof ? HG_ERR_HASH_EOF : HG_OK;
  if (c->alt.has_msg && same_msg(c->alt.msg, msg, len)) {
    std::swap(c->cur, c->alt);
    return c->cur.hash_eof ? HG_ERR_HASH_EOF : HG_OK;
  }
  // the current set becomes the cached one; the new message takes the other
  if (c->cur.has_msg) std::swap(c->cur, c->alt);
  if (!c->cur.d_h.p) HG_CHECK(c, c->cur.d_h.alloc(1));
  uint8_t d[32];
  sha256(msg, len, d);
  uint32_t k[8];
  c->cur.has_msg = false;
  c->cur.gt_level = 0;  // these buffers hold e(H, .) of an evicted message
  c->cur.gt_requests = 0;
  c->cur.msg.assign(msg, msg + len);
  c->cur.hash_eof = !hash_scalar(d, k);
  if (c->cur.hash_eof) {
    c->cur.has_msg = true;
    return HG_ERR_HASH_EOF;
  }
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->d_k.p, k, sizeof k, hipMemcpyHostToDevice, c->stream));
  launch_hash_point(c->d_k.p, c->cur.d_h.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  c->cur.has_msg = true;
  return HG_OK;
}

static int verify_batch_device_locked(hg_ctx* c, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                                      int32_t* d_codes, hipStream_t s) {
  if (!c->cur.has_msg) {
    c->err = "hg_set_message was not called";
    return HG_ERR_ARG;
  }
  HG_CHECK(c, c->ws.checks.ensure(n));
  const bool split = verify_split_for(c->verify_split, n);
  if (split) HG_CHECK(c, c->ws.sig_lines.ensure(verify_split_ws_bytes((int)n)));
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  PhaseTimer all(c, HG_PHASE_SUBMIT, s);
  launch_decode_checks(d_pks, d_sigs, (int)n, c->flavor, c->ws.checks.p, d_codes, s);
  if (c->cur.hash_eof) k_fill_codes<<<nb(n), 256, 0, s>>>(d_codes, (int)n, HG_OK, HG_ERR_HASH_EOF);
  else if (!timed_verify(c, c->ws.checks.p, (int)n, d_codes, s, split ? c->ws.sig_lines.p : nullptr)) {
    c->err = "hg_verify_batch: batch too large for the split form";
    return HG_ERR_ARG;
  }
  all.stop();
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

static int verify_batch_host_locked(hg_ctx* c, const uint8_t* pks, const uint8_t* sigs, size_t n, int32_t* codes) {
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 128));
  HG_CHECK(c, c->bytes_b.ensure(n * 64));
  HG_CHECK(c, c->ws.codes_c.ensure(n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, pks, n * 128, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, sigs, n * 64, hipMemcpyHostToDevice, c->stream));
  int rc = verify_batch_device_locked(c, c->bytes_a.p, c->bytes_b.p, n, c->ws.codes_c.p, c->stream);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(codes, c->ws.codes_c.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

static int sign_locked(hg_ctx* c, const uint8_t* scalars_be, size_t n, uint8_t* sigs_out) {
  if (!c->cur.has_msg) {
    c->err = "hg_set_message was not called";
    return HG_ERR_ARG;
  }
  if (c->cur.hash_eof) return HG_ERR_HASH_EOF;
  if (n == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 64));
  HG_CHECK(c, c->bytes_b.ensure(n * 32));
  HG_CHECK(c, c->ws.pts1.ensure(n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, scalars_be, n * 32, hipMemcpyHostToDevice, c->stream));
  launch_g1_mul(c->cur.d_h.p, c->bytes_b.p, (int)n, c->ws.pts1.p, c->stream);
  launch_encode_g1(c->ws.pts1.p, (int)n, c->bytes_a.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(sigs_out, c->bytes_a.p, n * 64, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

extern "C" {

int hg_version(void) { return 2; }

const char* hg_code_string(int code, int flavor) { return code_text(code, flavor); }

const char* hg_processing_error_string(int code, int flavor) { return processing_text(code, flavor); }

int hg_context_simds(hg_ctx* c) {
  if (!c) return 0;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) return 0;
  return 4 * cus;  // CDNA: four SIMDs per compute unit
}

int hg_context_flavor(hg_ctx* c) { return c ? c->flavor : -1; }

const char* hg_last_error(hg_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int hg_create(int device, int flavor, hg_ctx** out) {
  if (!out || (flavor != HG_FLAVOR_GO && flavor != HG_FLAVOR_CF)) return HG_ERR_ARG;
  *out = nullptr;
  hg_ctx* c = new hg_ctx();
  c->device = device;
  c->flavor = flavor;
  c->pinned_level = gt_forced_level();
  c->pol.overlap = gt_overlap();
  c->verify_split = sig_env().verify_split;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = c->stream.create(hipStreamNonBlocking);
  if (e == hipSuccess) e = c->d_lines.alloc(kLineTabEntries);
  if (e == hipSuccess) e = c->cur.d_h.alloc(1);
  if (e == hipSuccess) e = c->d_k.alloc(8);
  if (e != hipSuccess) {
    fprintf(stderr, "hg_create: %s\n", hipGetErrorString(e));
    delete c;
    return HG_ERR_DEVICE;
  }
  launch_g2_lines(c->d_lines.p, c->stream);
  if (check_launch(c) != HG_OK || hipStreamSynchronize(c->stream) != hipSuccess) {
    fprintf(stderr, "hg_create: %s\n", c->err.c_str());
    delete c;
    return HG_ERR_DEVICE;
  }
  // a pair of consecutive lines whose w^3 coefficient vanishes has an all-zero
  // record (k_g2_lines): a fact about the curve's constants that never holds
  std::vector<PairCoef> pairs(kNumPairs);
  bool pairs_ok = hipMemcpy(pairs.data(), line_pairs(c->d_lines.p), kNumPairs * sizeof(PairCoef),
                            hipMemcpyDeviceToHost) == hipSuccess;
  for (const PairCoef& pc : pairs) {
    uint32_t any = 0;
    for (int l = 0; l < 10; l++) any |= pc.xi.x.l[l] | pc.xi.y.l[l];
    pairs_ok = pairs_ok && any != 0;
  }
  if (!pairs_ok) {
    fprintf(stderr, "hg_create: a G2Base line pair has no w^3 coefficient\n");
    delete c;
    return HG_ERR_DEVICE;
  }
  *out = c;
  return HG_OK;
}

void hg_destroy(hg_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->ws.side) (void)hipStreamSynchronize(c->ws.side);
  if (c->last_ev) (void)hipEventSynchronize(c->last_ev);  // a submission on a caller stream
  delete c;
}

int hg_sync(hg_ctx* c) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  if (c->last_ev) HG_CHECK(c, hipEventSynchronize(c->last_ev));
  return HG_OK;
}

int hg_set_message(hg_ctx* c, const uint8_t* msg, size_t len) {
  if (!c || (!msg && len)) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return set_message_locked(c, msg, len);
}

int hg_registry_load(hg_ctx* c, const uint8_t* pks, size_t n, int32_t* codes) {
  if (!c || (!pks && n)) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  // until every table is rebuilt the context has no registry: a failure below
  // leaves it empty (every aggregate request then fails its range check)
  c->nreg = 0;
  c->reg_gen++;
  c->block_levels = 0;
  c->cur.gt_level = 0;
  c->cur.gt_requests = 0;
  c->alt.gt_level = 0;  // both messages' tables are e(H, .) of the old registry
  c->alt.gt_requests = 0;
  c->gt_cap = 2;
  c->oom_cap = 2;
  // the previous registry's membership check must be done before its buffer is reused
  if (c->sub_pending) HG_CHECK(c, hipEventSynchronize(c->ev_sub));
  c->sub_pending = false;
  c->reg_non_g2 = 0;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  HG_CHECK(c, c->reg.ensure(n));
  HG_CHECK(c, c->bytes_a.ensure(n * 128));
  HG_CHECK(c, c->codes_a.ensure(n));
  HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, pks, n * 128, hipMemcpyHostToDevice, c->stream));
  launch_decode_g2(c->bytes_a.p, (int)n, c->flavor, c->reg.p, c->codes_a.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  std::vector<int32_t> h(n);
  if (n) HG_CHECK(c, hipMemcpyAsync(h.data(), c->codes_a.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  int bad = 0;
  for (size_t i = 0; i < n; i++) bad |= h[i] != HG_OK;
  if (codes && n) memcpy(codes, h.data(), n * 4);
  if (bad) {
    c->err = "registry contains keys that fail to unmarshal";
    return HG_ERR_PK_UNMARSHAL;
  }
  // go flavor: x/crypto accepts any on-twist key (bn256/go/bn256.go:113-120);
  // count the keys outside G2 on the side stream (cf rejected them in the
  // decode above); the decode is complete (synchronised above)
  bool pending = false;
  if (c->flavor == HG_FLAVOR_GO && n) {
    HG_CHECK(c, ensure_side(c->ws));
    if (!c->ev_sub) HG_CHECK(c, c->ev_sub.create(hipEventDisableTiming));
    HG_CHECK(c, c->sub_count.ensure(1));
    HG_CHECK(c, hipMemsetAsync(c->sub_count.p, 0, sizeof(int), c->ws.side));
    launch_g2_subgroup(c->reg.p, (int)n, c->sub_count.p, c->ws.side);
    rc = check_launch(c);
    if (rc) return rc;
    HG_CHECK(c, hipEventRecord(c->ev_sub, c->ws.side));
    (void)hipStreamQuery(c->ws.side);  // flush: the check runs now, beside whatever follows
    pending = true;
  }
  // sums of the aligned power-of-two blocks (Handel's level ranges), level by level
  int K = 0;
  while (K < 23 && ((size_t)1 << K) < n) K++;
  std::vector<size_t> nbk(K + 1, 0);
  nbk[0] = n;
  size_t total = 0;
  for (int k = 1; k <= K; k++) {
    nbk[k] = (n + ((size_t)1 << k) - 1) >> k;
    c->block_base[k] = (int)total;
    total += nbk[k];
  }
  if (total) {
    HG_CHECK(c, c->blocks.ensure(total));
    for (int k = 1; k <= K; k++) {
      const PointG2* src = k == 1 ? c->reg.p : c->blocks.p + c->block_base[k - 1];
      launch_block_sums(src, (int)nbk[k - 1], c->blocks.p + c->block_base[k], (int)nbk[k], c->stream);
    }
    rc = check_launch(c);
    if (rc) return rc;
  }
  const size_t nwin = (n + 7) / 8;
  if (nwin) {
    HG_CHECK(c, c->wsum.ensure(nwin * 256));
    launch_window_sums(c->reg.p, (int)n, c->wsum.p, (int)nwin, c->stream);
    rc = check_launch(c);
    if (rc) return rc;
  }
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  c->block_levels = K;
  c->nreg = n;
  c->sub_pending = pending;
  return HG_OK;
}

size_t hg_registry_size(hg_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  return c->nreg;
}

int hg_verify_batch_device(hg_ctx* c, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n, int32_t* d_codes,
                           void* stream) {
  if (!c || (n && (!d_pks || !d_sigs || !d_codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return verify_batch_device_locked(c, d_pks, d_sigs, n, d_codes, s);
}

int hg_pack_verdicts_device(hg_ctx* c, const int32_t* d_codes, size_t n, uint8_t* d_bits, void* stream) {
  if (!c || (n && (!d_codes || !d_bits)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  launch_pack_verdicts(d_codes, (int)n, d_bits, s);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

int hg_verify_batch(hg_ctx* c, const uint8_t* pks, const uint8_t* sigs, size_t n, int32_t* codes) {
  if (!c || (n && (!pks || !sigs || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return verify_batch_host_locked(c, pks, sigs, n, codes);
}

int hg_verify_batch_msg(hg_ctx* c, const uint8_t* msg, size_t len, const uint8_t* pks, const uint8_t* sigs, size_t n,
                        int32_t* codes) {
  if (!c || (!msg && len) || (n && (!pks || !sigs || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = set_message_locked(c, msg, len);
  if (rc != HG_OK && rc != HG_ERR_HASH_EOF) return rc;
  if (n == 0) return HG_OK;
  return verify_batch_host_locked(c, pks, sigs, n, codes);
}

int hg_combine_g1(hg_ctx* c, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out, int32_t* codes) {
  if (!c || (n && (!a || !b || !out || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 64));
  HG_CHECK(c, c->bytes_b.ensure(n * 64));
  HG_CHECK(c, c->ws.pts1.ensure(n));
  HG_CHECK(c, c->pts1b.ensure(n));
  HG_CHECK(c, c->codes_a.ensure(n));
  HG_CHECK(c, c->ws.codes_b.ensure(n));
  HG_CHECK(c, c->ws.codes_c.ensure(n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, a, n * 64, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, b, n * 64, hipMemcpyHostToDevice, c->stream));
  launch_decode_g1(c->bytes_a.p, (int)n, c->flavor, c->ws.pts1.p, c->codes_a.p, c->stream);
  launch_decode_g1(c->bytes_b.p, (int)n, c->flavor, c->pts1b.p, c->ws.codes_b.p, c->stream);
  launch_merge_codes(c->codes_a.p, c->ws.codes_b.p, (int)n, c->ws.codes_c.p, c->stream);
  launch_g1_combine(c->ws.pts1.p, c->pts1b.p, (int)n, c->bytes_a.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out, c->bytes_a.p, n * 64, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(codes, c->ws.codes_c.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_combine_g2(hg_ctx* c, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out, int32_t* codes) {
  if (!c || (n && (!a || !b || !out || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 128 * 2));
  HG_CHECK(c, c->ws.pts2.ensure(n * 3));
  HG_CHECK(c, c->codes_a.ensure(n));
  HG_CHECK(c, c->ws.codes_b.ensure(n));
  HG_CHECK(c, c->ws.codes_c.ensure(n));
  uint8_t* d = c->bytes_a.p;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(d, a, n * 128, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(d + n * 128, b, n * 128, hipMemcpyHostToDevice, c->stream));
  launch_decode_g2(d, (int)n, c->flavor, c->ws.pts2.p, c->codes_a.p, c->stream);
  launch_decode_g2(d + n * 128, (int)n, c->flavor, c->ws.pts2.p + n, c->ws.codes_b.p, c->stream);
  launch_merge_codes(c->codes_a.p, c->ws.codes_b.p, (int)n, c->ws.codes_c.p, c->stream);
  launch_g2_combine(c->ws.pts2.p, c->ws.pts2.p + n, (int)n, c->ws.pts2.p + 2 * n, c->stream);
  launch_encode_g2(c->ws.pts2.p + 2 * n, (int)n, d, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out, d, n * 128, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(codes, c->ws.codes_c.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_pair(hg_ctx* c, const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out, int32_t* codes) {
  if (!c || (n && (!g1s || !g2s || !gt_out || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 384));
  HG_CHECK(c, c->bytes_b.ensure(n * 64));
  HG_CHECK(c, c->ws.pts1.ensure(n));
  HG_CHECK(c, c->ws.pts2.ensure(n));
  HG_CHECK(c, c->codes_a.ensure(n));
  HG_CHECK(c, c->ws.codes_b.ensure(n));
  HG_CHECK(c, c->ws.codes_c.ensure(n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, g2s, n * 128, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, g1s, n * 64, hipMemcpyHostToDevice, c->stream));
  launch_decode_g2(c->bytes_a.p, (int)n, HG_FLAVOR_GO, c->ws.pts2.p, c->codes_a.p, c->stream);
  launch_decode_g1(c->bytes_b.p, (int)n, HG_FLAVOR_GO, c->ws.pts1.p, c->ws.codes_b.p, c->stream);
  launch_merge_codes(c->codes_a.p, c->ws.codes_b.p, (int)n, c->ws.codes_c.p, c->stream);
  launch_pair(c->ws.pts1.p, c->ws.pts2.p, (int)n, c->d_lines.p, c->bytes_a.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(gt_out, c->bytes_a.p, n * 384, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(codes, c->ws.codes_c.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_keygen(hg_ctx* c, const uint8_t* scalars_be, size_t n, uint8_t* pks_out) {
  if (!c || (n && (!scalars_be || !pks_out)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 128));
  HG_CHECK(c, c->bytes_b.ensure(n * 32));
  HG_CHECK(c, c->ws.pts2.ensure(n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, scalars_be, n * 32, hipMemcpyHostToDevice, c->stream));
  launch_g2_mul_base(c->bytes_b.p, (int)n, c->ws.pts2.p, c->stream);
  launch_encode_g2(c->ws.pts2.p, (int)n, c->bytes_a.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(pks_out, c->bytes_a.p, n * 128, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_sign(hg_ctx* c, const uint8_t* scalars_be, size_t n, uint8_t* sigs_out) {
  if (!c || (n && (!scalars_be || !sigs_out)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return sign_locked(c, scalars_be, n, sigs_out);
}

int hg_sign_msg(hg_ctx* c, const uint8_t* msg, size_t len, const uint8_t* scalars_be, size_t n, uint8_t* sigs_out) {
  if (!c || (!msg && len) || (n && (!scalars_be || !sigs_out)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = set_message_locked(c, msg, len);
  if (rc != HG_OK) return rc;
  return sign_locked(c, scalars_be, n, sigs_out);
}

int hg_debug_fp12(hg_ctx* c, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
  if (!c || (n && (!a || !b || !out)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  const int base_op = op & 255;  // bits 8..: repetitions (k_fp12_op)
  if (base_op > 10 || base_op == 9) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 384 * 3));
  uint8_t* d = c->bytes_a.p;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(d, a, n * 384, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(d + n * 384, b, n * 384, hipMemcpyHostToDevice, c->stream));
  launch_fp12_op(op, d, d + n * 384, (int)n, d + 2 * n * 384, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out, d + 2 * n * 384, n * 384, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

// One bound team-program instance on n raw team regions (bn256_xprobe.hip)
int hg_debug_xinst(hg_ctx* c, int inst, int form, const uint32_t* in, size_t n, uint32_t* out, int* region_elems) {
  if (!c) return HG_ERR_ARG;
  const int elems = xprobe_region_elems(inst, form);
  if (elems == 0) return HG_ERR_ARG;  // no such instance, no such form, or not a form of its layout
  if ((n && (!in || !out)) || n > (size_t)1 << 20) return HG_ERR_ARG;
  if (region_elems) *region_elems = elems;
  if (n == 0) return HG_OK;
  const size_t bytes = n * (size_t)elems * 40;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(2 * bytes));
  uint8_t* d = c->bytes_a.p;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(d, in, bytes, hipMemcpyHostToDevice, c->stream));
  launch_xprobe(inst, form, (const uint32_t*)d, (int)n, (uint32_t*)(d + bytes), c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out, d + bytes, bytes, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

// One per-thread primitive of bn256_fp.h / bn256_curve.h on n cases of raw limbs (bn256_fprobe.hip)
int hg_debug_field(hg_ctx* c, int op, const uint32_t* in, size_t n, uint32_t* out, int* in_words, int* out_words) {
  if (!c) return HG_ERR_ARG;
  int wi = 0, wo = 0;
  if (!fprobe_words(op, &wi, &wo)) return HG_ERR_ARG;
  if ((n && (!in || !out)) || n > (size_t)1 << 20) return HG_ERR_ARG;
  if (in_words) *in_words = wi;
  if (out_words) *out_words = wo;
  if (n == 0) return HG_OK;
  const size_t bytes_in = n * (size_t)wi * 4, bytes_out = n * (size_t)wo * 4;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(bytes_in + bytes_out));
  uint8_t* d = c->bytes_a.p;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(d, in, bytes_in, hipMemcpyHostToDevice, c->stream));
  launch_fprobe(op, (const uint32_t*)d, (int)n, (uint32_t*)(d + bytes_in), c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out, d + bytes_in, bytes_out, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

// kernel: a SigForm by its number (bn256_sigform.h), whatever sig_form() would choose
int hg_sig_pairing_device(hg_ctx* c, const uint8_t* d_sigs, size_t n, uint8_t* d_fe, int kernel, void* stream) {
  if (!c || (n && (!d_sigs || !d_fe)) || n > (size_t)INT32_MAX || kernel < 0 || kernel > 4) return HG_ERR_ARG;
  const SigForm form = (SigForm)kernel;
  if (sig_form_12(form) && n > (size_t)kSig12MaxN) return HG_ERR_ARG;  // k_sig_lines: 4 n threads in int
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, c->ws.sig_lines.ensure(sig_form_ws_bytes(form, (int)n)));
  if (!launch_sig_form(form, d_sigs, c->flavor, (int)n, c->d_lines.p, c->ws.sig_lines.p, (Gt*)d_fe, s)) return HG_ERR_ARG;
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

int hg_diag_read(hg_ctx* c, uint64_t* out, size_t n) {
  if (!c || !out) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  if (c->last_ev) HG_CHECK(c, hipEventSynchronize(c->last_ev));
  return diag_read(out, n) == 0 ? HG_OK : HG_ERR_ARG;
}

size_t hg_context_bytes(hg_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  // the line table, the hash scalar and both messages' H (counted from creation)
  size_t b = c->d_lines.bytes() + c->d_k.bytes() + 2 * sizeof(PointG1);
  b += c->reg.bytes() + c->blocks.bytes() + c->wsum.bytes();
  b += c->bytes_a.bytes() + c->bytes_b.bytes() + c->pts1b.bytes();
  b += c->codes_a.bytes() + c->reqs.bytes() + c->words.bytes();
  b += c->cur.table_bytes() + c->alt.table_bytes();
  b += c->ws.bytes();
  for (const hg_lane* l : c->lanes) b += l->bytes();
  b += c->sub_count.bytes() + c->pkts.bytes();
  b += c->msgs.bytes();  // nothing until the first multi-message call (it builds the G1 base table)
  return b;
}

int hg_timing_enable(hg_ctx* c, int on) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->timing = on != 0;
  return HG_OK;
}

int hg_timing_read_phase(hg_ctx* c, int phase, double* total_ms, int* launches) {
  if (!c || !total_ms || !launches || phase < 0 || phase >= HG_NUM_PHASES) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  double tot = 0;
  int k = 0;
  auto& ev = c->events[phase];
  int rc = HG_OK;
  for (auto& pr : ev) {
    float ms = 0;
    hipError_t e = hipEventSynchronize(pr.second);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.first, pr.second);
    if (e != hipSuccess && rc == HG_OK) {
      c->err = std::string("hg_timing_read_phase: ") + hipGetErrorString(e);
      rc = HG_ERR_DEVICE;
    }
    tot += ms;
    k++;
  }
  ev.clear();
  *total_ms = tot;
  *launches = k;
  return rc;
}

int hg_timing_read(hg_ctx* c, double* total_ms, int* launches) {
  return hg_timing_read_phase(c, HG_PHASE_VERIFY, total_ms, launches);
}

int hg_debug_fp_mul(hg_ctx* c, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
  if (!c || (n && (!a || !b || !out)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 32 * 3));
  uint32_t* da = (uint32_t*)c->bytes_a.p;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(da, a, n * 32, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(da + 8 * n, b, n * 32, hipMemcpyHostToDevice, c->stream));
  launch_fp_mul(da, da + 8 * n, (int)n, da + 16 * n, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out, da + 16 * n, n * 32, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

}  // extern "C"
